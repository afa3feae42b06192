"""Segmenting with a trained model: the outbound half of the pipeline, the mirror of the loop body of the reference's
test_model.py:242-309 (model(image), torch.argmax(outputs, dim=1), the per-sample per-class Dice / IoU, pred_classes.cpu()).

  predict_labels(model, x, target=None)         uint8 (N, D, H, W) label map, and with a target the exact per-sample counts
  predict_labels_ensemble(models, x, flips)     the label map of the softmax average over mirrored views and / or several models
  predict_labels_sliding(models, x, window)     the same outputs from overlapping windows blended with a Gaussian importance map
  pseudo_labels(models, x, threshold)           the confident voxels of such a prediction as an int64 training target, the rest
                                                set to an ignore value (self-training: TrainStep(ignore_index=...).step takes it)
  per_sample_dice_iou(counts, classes)          [{class: (dice, iou)}] per sample from those counts (test_model.py:265-276)
  segment_scan(model, image, affine, dataset)   a scan as stored -> its label map as stored: resample, predict, restore; the restore
                                                is the order-0 gather of the label map ("nearest") or, from the votes, the order-1
                                                zoom per class with the argmax on the stored grid ("linear", restore_labels_soft)

The logits never reach memory: the network runs with logits = NULL (mi3d_unet_infer) and the 1x1x1 head, the argmax and the counts
are one pass over the decoder output (mi3d_unet_head_labels), which writes 1 byte per voxel where the logits route writes 16 and
re-reads them twice.  Every label is the first maximum of exactly the logits model(x) would return.  The arrays of the loop's preview figure (visualize_prediction, test_model.py:299-305)
are preview.prediction_panels' work, on the device as well.  Test-time flips (the eight mirrored views random_flip trains with)
and model ensembles vote in the same place: per view one pass over the decoder output does head -> softmax -> add into a
float32 vote volume at the mirrored voxel (mi3d_unet_head_votes), and the last view's pass ends in the argmax, so neither the
logits nor the probabilities of a view are ever written.  Sliding windows (predict_labels_sliding, segment_scan(window=...)) for
models trained on patches (spatial.RandAffineElastic(spatial_size=...)) vote there too: per window one pass does head -> softmax ->
importance weight -> add into the window's sub-box of ONE float32 accumulator (mi3d_unet_head_votes_window), and a finishing pass
divides by the weight sum and takes the argmax (mi3d_votes_finish).  The schedule and the Gaussian importance map follow MONAI's
sliding_window_inference(roi_size, overlap, mode="gaussian") as documented; MONAI is not available to the tests, so that parity is
UNPINNED: the contract is include/mi3d.h, restated in numpy by tests/sliding_ref.py.  File reading / writing and drawing
(matplotlib) stay outside; so do padding modes for windows larger than the volume (the window is clipped instead).  So do, for the soft restore:
several scans per call, per-class counts against a ground truth on the stored grid, and zoom orders other than 1 and 0.
"""
import math

import torch

from . import _lib, components, engine, metrics, preprocess, resample
from ._lib import Mi3dError, stream_ptr

CT_WINDOW = (-160.0, 240.0)      # preprocess.preprocess_ct's defaults (utils/dataloader.py:111-117)


def predict_labels(model, x, target=None):
    """torch.argmax(model(x), dim=1) as uint8 (N, D, H, W) for a model in eval(); with target (N, 1, D, H, W) also the exact
    int64 (N, 3C + 1) counts {n_inter[C], n_pred[C], n_label[C], n_correct} of every sample (metrics.class_counts sums them
    over the batch).  Same checks, compute dtype and descriptor as model(x) (engine.plan_call), and the bits of the logits that
    model(x) returns under torch.no_grad() (the inference route, test_model.py:242).  Nothing synchronises."""
    what = "predict_labels"
    _lib.require_cuda(x, what)
    if model.training:
        raise Mi3dError(f"{what}: the model is in train() mode; call model.eval() (test_model.py:226)")
    if model.output_activation is not None:
        raise Mi3dError(f"{what}: the model has an output_activation; the argmax of activated logits is not this path "
                        "(take torch.argmax of model(x))")
    x = x.detach().contiguous().float()
    plan = engine.plan_call(model, x)
    desc = plan.desc
    n, c, v = desc.N, desc.out_channels, desc.D * desc.H * desc.W
    labels = counts = head_ws = None
    if target is not None:
        _lib.require_cuda(target, what)
        if target.numel() != n * v:
            raise Mi3dError(f"{what}: target shape {tuple(target.shape)} does not match the input {tuple(x.shape)}")
        labels = target.reshape(n, v)
        labels = (labels if labels.dtype == torch.int64 else labels.long()).contiguous()
        head_bytes = _lib.lib().mi3d_head_labels_workspace_bytes(n, c)
        if head_bytes == 0:
            raise Mi3dError(f"{what}: {c} classes unsupported")
        head_ws = torch.empty(head_bytes, dtype=torch.uint8, device=x.device)
        counts = torch.empty((n, 3 * c + 1), dtype=torch.int64, device=x.device)
    # everything is checked: launch
    plan.own_workspace(x.device)
    out = torch.empty((n, desc.D, desc.H, desc.W), dtype=torch.uint8, device=x.device)
    plan.infer(x, stream=stream_ptr())
    plan.head_labels(labels=labels, out=out, counts=counts, head_ws=head_ws, stream=stream_ptr())
    return out if target is None else (out, counts)


FLIPS8 = tuple(range(8))         # every mirrored view random_flip trains with (utils/dataloader.py:207-213): bit 0 W, bit 1 H, bit 2 D
NO_FLIP = (0,)


def _flip_dims(code):
    """The dims of an (N, C, D, H, W) tensor that flip code `code` mirrors."""
    return [dim for bit, dim in ((1, 4), (2, 3), (4, 2)) if code & bit]


def predict_labels_ensemble(models, x, flips=FLIPS8, target=None, confidence=False, votes=False):
    """Labels of the softmax average over views.  A view is (a model, a flip code); the views are model-major in the order given:

        p_v    = softmax(m(torch.flip(x, dims of f)), dim=1) flipped back, float32, on the bits of the logits m(...) returns
        votes  = ((p_0 + p_1) + p_2) + ...                float32 adds in view order
        labels = first maximum of votes over the classes  uint8 (N, D, H, W)

    models: one model or a sequence of models with equal out_channels; flips: a sequence of codes (FLIPS8, NO_FLIP, ...).
    Returns the labels, then, for whichever were asked for and in this order: the counts of predict_labels (target), the
    confidence votes[label] / views as float (N, D, H, W), the mean probabilities votes / views as float (N, C, D, H, W).
    Per view: torch.flip, the network with logits = NULL, and ONE pass over the decoder output (mi3d_unet_head_votes) that does
    head -> softmax -> add at the mirrored voxel; the last view's pass ends in the argmax.  The checks of predict_labels, for
    every model, before the first launch.  No atomics: the same inputs give the same bits.  Nothing synchronises."""
    what = "predict_labels_ensemble"
    models, flips = _check_views(what, models, flips)
    _lib.require_cuda(x, what)
    x = x.detach().contiguous().float()
    plans = [engine.plan_call(m, x) for m in models]
    desc = plans[0].desc
    n, c, v = desc.N, desc.out_channels, desc.D * desc.H * desc.W
    labels = counts = head_ws = None
    if target is not None:
        _lib.require_cuda(target, what)
        if target.numel() != n * v:
            raise Mi3dError(f"{what}: target shape {tuple(target.shape)} does not match the input {tuple(x.shape)}")
        labels = target.reshape(n, v)
        labels = (labels if labels.dtype == torch.int64 else labels.long()).contiguous()
        head_bytes = _lib.lib().mi3d_head_votes_workspace_bytes(n, c)
        if head_bytes == 0:
            raise Mi3dError(f"{what}: {c} classes unsupported")
        head_ws = torch.empty(head_bytes, dtype=torch.uint8, device=x.device)
        counts = torch.empty((n, 3 * c + 1), dtype=torch.int64, device=x.device)
    # everything is checked: launch
    views = len(models) * len(flips)
    out = torch.empty((n, desc.D, desc.H, desc.W), dtype=torch.uint8, device=x.device)
    conf = torch.empty((n, desc.D, desc.H, desc.W), dtype=torch.float32, device=x.device) if confidence else None
    vol = None
    if votes or views > 1:
        vol = torch.empty((n, c, desc.D, desc.H, desc.W), dtype=torch.float32, device=x.device)
    flipped = [x if f == 0 else torch.flip(x, _flip_dims(f)) for f in flips]
    view = 0
    for plan in plans:
        plan.own_workspace(x.device)
        for f, xf in zip(flips, flipped):
            last = view == views - 1
            plan.infer(xf, stream=stream_ptr())
            plan.head_votes(flip=f, view=view, views=views, flags=_lib.VOTES_KEEP if votes else 0, votes=vol,
                            out=out if last else None, confidence=conf if last else None, labels=labels if last else None,
                            counts=counts if last else None, head_ws=head_ws if last else None, stream=stream_ptr())
            view += 1
        plan.release_workspace()          # stream-ordered: the next model's workspace may reuse the memory
    result = [out]
    if target is not None:
        result.append(counts)
    if confidence:
        result.append(conf)
    if votes:
        result.append(vol.div_(float(views)) if views > 1 else vol)
    return result[0] if len(result) == 1 else tuple(result)


WINDOW_MODES = ("gaussian", "constant")


def window_starts(n, window, overlap):
    """The ascending window starts along an axis of n voxels (the schedule of include/mi3d.h mi3d_head_votes_window's callers):
    roi = min(window, n); [0] if roi == n; else the distinct min(i * interval, n - roi) for i < ceil((n - roi) / interval) + 1
    with interval = max(int(roi * (1 - overlap)), 1).  Every index is covered, the last start is clamped to n - roi."""
    roi = min(int(window), int(n))
    if roi == n:
        return [0]
    interval = max(int(roi * (1 - overlap)), 1)
    k = -(-(n - roi) // interval) + 1
    return sorted({min(i * interval, n - roi) for i in range(k)})


def importance_tables(roi, mode="gaussian", sigma_scale=0.125):
    """One float32 table per axis of a window of sides `roi` (host tensors): "gaussian" g[i] = float32(exp(-0.5 * ((i - (r - 1) / 2)
    / (sigma_scale * r))**2)) computed in float64, "constant" ones.  The weight of a window voxel is (g_d[d] * g_h[h]) * g_w[w] in
    float32.  The tables are bitwise symmetric (the offsets from the centre are exact), so a flipped view carries the same weight."""
    if mode not in WINDOW_MODES:
        raise Mi3dError(f"importance_tables: mode is one of {WINDOW_MODES}, got {mode!r}")
    if mode == "constant":
        return [torch.ones(int(r), dtype=torch.float32) for r in roi]
    return [torch.tensor([math.exp(-0.5 * ((i - (r - 1) / 2) / (sigma_scale * r)) ** 2) for i in range(int(r))], dtype=torch.float64).float()
            for r in roi]


def norm_tables(sizes, roi, starts, tables):
    """mi3d_votes_finish's n_d, n_h, n_w (host float32 tensors): n_axis[i] = the float32 rounding of the float64 sum, in ascending
    start order, of that axis's table entries over the windows that cover index i."""
    out = []
    for n, r, st, g in zip(sizes, roi, starts, tables):
        g64 = g.double().tolist()
        total = [0.0] * n
        for s in st:
            for j in range(r):
                total[s + j] = total[s + j] + g64[j]
        out.append(torch.tensor(total, dtype=torch.float64).float())
    return out


def _check_views(what, models, flips):
    """The checks predict_labels_ensemble and predict_labels_sliding share; returns the two lists."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    flips = list(flips)
    if not models or not flips:
        raise Mi3dError(f"{what}: at least one model and one flip code are needed")
    for f in flips:
        if not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < 8:
            raise Mi3dError(f"{what}: flip code {f!r} is not an integer in [0, 8) (bit 0: W, bit 1: H, bit 2: D)")
    for m in models:
        if m.training:
            raise Mi3dError(f"{what}: a model is in train() mode; call model.eval() (test_model.py:226)")
        if m.output_activation is not None:
            raise Mi3dError(f"{what}: a model has an output_activation; the votes are the softmax of raw logits")
        if m.final_conv.out_channels != models[0].final_conv.out_channels:
            raise Mi3dError(f"{what}: the models disagree on out_channels ({m.final_conv.out_channels} and "
                            f"{models[0].final_conv.out_channels})")
    return models, flips


def predict_labels_sliding(models, x, window=(96, 96, 96), overlap=0.5, mode="gaussian", sigma_scale=0.125, flips=NO_FLIP,
                           window_batch=1, target=None, confidence=False, votes=False):
    """Sliding-window inference with importance-weighted votes (the role of MONAI's sliding_window_inference(roi_size, overlap,
    mode="gaussian"); unpinned against MONAI, the contract is include/mi3d.h mi3d_head_votes_window / mi3d_votes_finish):

        windows = the Cartesian product of window_starts per axis, D outermost; a window larger than the volume is clipped to it
        views   = (model, window, flip code): model-major, then window-major, flip-minor in the order given
        acc     = sum over the views, in that order, of weight(x) * softmax(m(flip(crop)))[flipped back], float32, per voxel
        labels  = first maximum of acc;  confidence = acc[label] / norm;  mean probabilities = acc / norm,
                  norm = the weight sum at the voxel (norm_tables) * (models * flips)

    x: (N, Cin, D, H, W); the volumes are processed one after another.  Returns what predict_labels_ensemble returns, in the same
    order (votes=True: the normalised mean probabilities).  The windows are cropped (and mirrored) with torch slicing and stacked
    window_batch views at a time: the batch follows the view order, so every window_batch gives the same bits.  Per batch: the
    network with logits = NULL and ONE pass over the decoder output per window (mi3d_unet_head_votes_window), so neither the
    logits nor the probabilities of a window are ever written; one finishing pass per volume (mi3d_votes_finish).  The checks
    of predict_labels_ensemble plus window, overlap, mode, sigma_scale and window_batch, before the first launch.  No atomics: the
    same inputs give the same bits.  Nothing is read back and nothing waits for the device; the six small tables (three weight,
    three norm) are built on the host and uploaded per call."""
    what = "predict_labels_sliding"
    models, flips = _check_views(what, models, flips)
    _lib.require_cuda(x, what)
    if x.dim() != 5:
        raise Mi3dError(f"{what}: x is (N, C, D, H, W), got shape {tuple(x.shape)}")
    window = tuple(window) if isinstance(window, (list, tuple)) else (window,) * 3
    if len(window) != 3 or any(not isinstance(w, int) or isinstance(w, bool) or w < 1 for w in window):
        raise Mi3dError(f"{what}: window is three positive integers, got {window!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0 <= overlap < 1:
        raise Mi3dError(f"{what}: overlap {overlap!r} is not in [0, 1)")
    if mode not in WINDOW_MODES:
        raise Mi3dError(f"{what}: mode is one of {WINDOW_MODES}, got {mode!r}")
    if not sigma_scale > 0:
        raise Mi3dError(f"{what}: sigma_scale {sigma_scale!r} is not positive")
    if not isinstance(window_batch, int) or isinstance(window_batch, bool) or window_batch < 1:
        raise Mi3dError(f"{what}: window_batch {window_batch!r} is not a positive integer")
    x = x.detach().contiguous().float()
    n, cin = x.shape[:2]
    sizes = tuple(x.shape[2:])
    roi = tuple(min(w, s) for w, s in zip(window, sizes))
    starts = [window_starts(s, w, overlap) for s, w in zip(sizes, window)]
    views = [((od, oh, ow), f) for od in starts[0] for oh in starts[1] for ow in starts[2] for f in flips]
    batches = [views[i:i + window_batch] for i in range(0, len(views), window_batch)]
    full, tail = len(batches[0]), len(batches[-1])
    # one plan per model for the window shape, and one for the smaller last batch; plan_call reads the shape only
    shapes = [torch.empty((b, cin) + roi, device="meta") for b in ((full,) if tail == full else (full, tail))]
    plans = [[engine.plan_call(m, s) for s in shapes] for m in models]
    c, v = plans[0][0].desc.out_channels, sizes[0] * sizes[1] * sizes[2]
    if v >= 2 ** 31:
        raise Mi3dError(f"{what}: a volume of {v} voxels (below 2^31)")
    tgt = counts = head_ws = None
    if target is not None:
        _lib.require_cuda(target, what)
        if target.numel() != n * v:
            raise Mi3dError(f"{what}: target shape {tuple(target.shape)} does not match the input {tuple(x.shape)}")
        tgt = target.reshape(n, v)
        tgt = (tgt if tgt.dtype == torch.int64 else tgt.long()).contiguous()
    head_bytes = _lib.lib().mi3d_head_votes_workspace_bytes(1, c)
    if head_bytes == 0:
        raise Mi3dError(f"{what}: {c} classes unsupported")
    if target is not None:
        head_ws = torch.empty(head_bytes, dtype=torch.uint8, device=x.device)
        counts = torch.empty((n, 3 * c + 1), dtype=torch.int64, device=x.device)
    tables = importance_tables(roi, mode, sigma_scale)
    norms = [t.to(x.device) for t in norm_tables(sizes, roi, starts, tables)]
    tables = [t.to(x.device) for t in tables]
    host = [(_lib.int_table([f for _, f in b]), _lib.int_table([k for o, _ in b for k in o])) for b in batches]
    # everything is checked: launch
    out = torch.empty((n,) + sizes, dtype=torch.uint8, device=x.device)
    conf = torch.empty((n,) + sizes, dtype=torch.float32, device=x.device) if confidence else None
    mean = torch.empty((n, c) + sizes, dtype=torch.float32, device=x.device) if votes else None
    for i in range(n):
        acc = mean[i].zero_() if votes else torch.zeros((c,) + sizes, dtype=torch.float32, device=x.device)
        for per_model in plans:
            for plan in per_model:          # the full batches, then the smaller last one: still the view order
                plan.own_workspace(x.device)
                for b, (fl, og) in zip(batches, host):
                    if len(b) != plan.desc.N:
                        continue
                    crops = [x[i, :, od:od + roi[0], oh:oh + roi[1], ow:ow + roi[2]] for (od, oh, ow), _ in b]
                    crops = [t if f == 0 else torch.flip(t, [d - 1 for d in _flip_dims(f)]) for t, (_, f) in zip(crops, b)]
                    plan.infer(torch.stack(crops), stream=stream_ptr())
                    plan.head_votes_window(flips=fl, tables=tables, origins=og, acc=acc, stream=stream_ptr())
                plan.release_workspace()          # stream-ordered: the next plan's workspace may reuse the memory
        rows = [None if t is None else t[i].data_ptr() for t in (out, conf, tgt, counts)]
        _lib.call("mi3d_votes_finish", acc.data_ptr(), c, *sizes, *[t.data_ptr() for t in norms], len(models) * len(flips),
                  _lib.VOTES_NORMALIZE if votes else 0, *rows, _lib.ptr(head_ws), stream_ptr())
    result = [out]
    if target is not None:
        result.append(counts)
    if confidence:
        result.append(conf)
    if votes:
        result.append(mean)
    return result[0] if len(result) == 1 else tuple(result)


def pseudo_labels_from(labels, confidence, n_classes, threshold=0.9, ignore_index=255):
    """The pseudo-label pass alone (mi3d_pseudo_labels) on a uint8 label map and its float32 confidence map, both (N, D, H, W):
    target (N, 1, D, H, W) int64 = the label where confidence >= threshold[label], else ignore_index, and the int64 table
    (N, C + 1) of the voxels kept per class and, last, ignored per sample.  threshold: a float or one float per class.  A NaN
    confidence is ignored.  Nothing synchronises."""
    what = "pseudo_labels"
    _lib.require_cuda(labels, what)
    _lib.require_cuda(confidence, what)
    if labels.dtype != torch.uint8 or confidence.dtype != torch.float32 or labels.shape != confidence.shape or labels.dim() < 2:
        raise Mi3dError(f"{what}: expected a uint8 label map and a float32 confidence map of one shape (N, ...), got "
                        f"{labels.dtype} {tuple(labels.shape)} and {confidence.dtype} {tuple(confidence.shape)}")
    c = int(n_classes)
    thr = [float(threshold)] * c if isinstance(threshold, (int, float)) else [float(t) for t in threshold]
    if len(thr) != c:
        raise Mi3dError(f"{what}: {len(thr)} thresholds for {c} classes")
    ignore_index = metrics.check_ignore_index(ignore_index)
    if ignore_index is None:
        raise Mi3dError(f"{what}: ignore_index is required")
    labels, confidence = labels.contiguous(), confidence.contiguous()
    n = labels.shape[0]
    target = torch.empty((n, 1) + tuple(labels.shape[1:]), dtype=torch.int64, device=labels.device)
    table = torch.empty((n, c + 1), dtype=torch.int64, device=labels.device)
    _lib.call("mi3d_pseudo_labels", _lib.ptr(labels), _lib.ptr(confidence), n, labels.numel() // n, c, (_lib.f32 * c)(*thr), ignore_index,
              _lib.ptr(target), _lib.ptr(table), stream_ptr())
    return target, table


def pseudo_labels(models, x, threshold=0.9, ignore_index=255, flips=NO_FLIP, window=None, **sliding_kw):
    """Self-training targets on an unlabelled batch: predict with predict_labels_ensemble(confidence=True), or with
    predict_labels_sliding(window=window, **sliding_kw) when a window is given, keep the voxels whose confidence reaches the
    threshold of their class and set the others to ignore_index (pseudo_labels_from).  Returns (target int64 (N, 1, D, H, W),
    table int64 (N, C + 1)); the target is what TrainStep(ignore_index=ignore_index).step(x, target) takes.  The models are in
    eval() mode, as for every prediction here.  Quantile or class-balanced thresholds are not offered."""
    if window is None:
        if sliding_kw:
            raise Mi3dError(f"pseudo_labels: {sorted(sliding_kw)} belong to a sliding-window prediction (give window=...)")
        labels, conf = predict_labels_ensemble(models, x, flips=flips, confidence=True)
    else:
        labels, conf = predict_labels_sliding(models, x, window=window, flips=flips, confidence=True, **sliding_kw)
    first = models[0] if isinstance(models, (list, tuple)) else models
    return pseudo_labels_from(labels, conf, first.final_conv.out_channels, threshold, ignore_index)


def per_sample_dice_iou(counts, classes=(1, 2, 3)):
    """One {class: (dice, iou)} of Python floats per sample from predict_labels' (N, 3C + 1) counts, by the formula of
    test_model.py:269-276 (a class absent from the sample's label, or one the model does not have, scores 0.0 for both).
    One host copy of the counts, like the reference's .item() calls."""
    rows = counts.cpu().tolist() if isinstance(counts, torch.Tensor) else [list(r) for r in counts]
    if not rows or any(len(r) != len(rows[0]) or len(r) % 3 != 1 for r in rows):
        raise Mi3dError(f"per_sample_dice_iou: (N, 3C + 1) counts expected, got rows of {[len(r) for r in rows]}")
    return [metrics.dice_iou_from_counts(r, len(r) // 3, classes) for r in rows]


RESTORE_MODES = ("nearest", "linear")


def _clean(labels, keep_largest, fill_holes, connectivity):
    """segment_scan's clean-up of one map: components.keep_largest, then components.fill_holes, each where asked for ->
    (the map, the records of the steps that ran)."""
    records = []
    if keep_largest is not None:
        records.append(components.keep_largest(labels, keep=keep_largest, connectivity=connectivity))
        labels = records[-1].labels
    if fill_holes is not None:
        records.append(components.fill_holes(labels, classes=fill_holes, connectivity=connectivity))
        labels = records[-1].labels
    return labels, records


def segment_scan(model, image, affine, dataset_name, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192), keep_largest=None,
                 connectivity=1, flips=None, models=None, restore="nearest", window=None, overlap=0.5, window_mode="gaussian",
                 fill_holes=None):
    """A decoded scan AS STORED and its 4x4 affine -> (uint8 labels with the scan's shape and strides, uint8 labels on the
    training grid, affine of the grid).  A composition only: resample.resample_scan (CT window fused into the last store for
    '_ct' names, preprocess.preprocess_mri afterwards otherwise: the dispatch of preprocess.preprocess), predict_labels,
    resample.restore_labels.  keep_largest: a dict {class: components to keep} such as components.ORGANS; the grid map is then
    cleaned by components.keep_largest (with `connectivity`) before it is restored, the second element is the cleaned grid map
    and a fourth, the Cleaned record (stats, status), is appended.  None: no cleaning, three elements.
    flips / models: with either, the grid map is predict_labels_ensemble's over `models` (default: the model) and `flips` (default
    NO_FLIP), e.g. flips=FLIPS8 for mirroring on all three axes; with both None it is predict_labels', bit for bit as before.
    restore: "nearest" (the default) is the route above.  "linear" restores from the probabilities: the grid prediction is
    predict_labels_ensemble(models or the model, flips or NO_FLIP, votes=True) and the stored map is
    resample.restore_labels_soft of its votes (order-1 zoom per class, argmax on the stored grid), so organ boundaries are not the
    staircase of an upsampled label map.  keep_largest then cleans the STORED map, after the restore: the first element is the
    cleaned stored map, the second the UNCLEANED grid map, and the Cleaned record describes the stored map.  Any other value
    raises before anything is launched.
    window: None (the default) leaves every route above bit for bit as it is.  With a window (three ints) the grid prediction is
    predict_labels_sliding's over `models` (default: the model) and `flips` (default NO_FLIP) with `overlap` and mode
    `window_mode`; restore="linear" feeds its normalised mean probabilities to resample.restore_labels_soft; keep_largest
    composes as above.
    fill_holes: None (the default) leaves every route above and what it returns as it is.  A tuple of classes: the map that
    keep_largest cleans (the grid map for restore="nearest", the stored map for restore="linear"), after keep_largest where both
    are given, has its enclosed holes filled by components.fill_holes(classes=fill_holes, connectivity=connectivity); that element is
    then the filled map and the Filled record (stats, summary, status) is appended as the last element."""
    if restore not in RESTORE_MODES:
        raise Mi3dError(f"segment_scan: restore is one of {RESTORE_MODES}, got {restore!r}")
    if window is not None and window_mode not in WINDOW_MODES:
        raise Mi3dError(f"segment_scan: window_mode is one of {WINDOW_MODES}, got {window_mode!r}")

    def ensemble(x, **kw):           # the grid prediction over views: sliding windows with a window, else the whole grid at once
        who, fl = model if models is None else models, NO_FLIP if flips is None else flips
        if window is None:
            return predict_labels_ensemble(who, x, flips=fl, **kw)
        return predict_labels_sliding(who, x, window=window, overlap=overlap, mode=window_mode, flips=fl, **kw)
    ct = dataset_name.lower().endswith("_ct")
    grid, _, grid_affine = resample.resample_scan(image, affine, target_spacing=target_spacing, target_shape=target_shape,
                                                  ct_window=CT_WINDOW if ct else None)
    if not ct:
        grid = preprocess.preprocess_mri(grid)
    if restore == "linear":
        on_grid, votes = ensemble(grid[None, None], votes=True)
        stored = resample.restore_labels_soft(votes, affine, image)
        if keep_largest is None and fill_holes is None:
            return stored, on_grid[0], grid_affine
        stored, records = _clean(stored, keep_largest, fill_holes, connectivity)
        return (stored, on_grid[0], grid_affine, *records)
    if flips is None and models is None and window is None:
        on_grid = predict_labels(model, grid[None, None])[0]
    else:
        on_grid = ensemble(grid[None, None])[0]
    if keep_largest is None and fill_holes is None:
        return resample.restore_labels(on_grid, affine, image), on_grid, grid_affine
    on_grid, records = _clean(on_grid, keep_largest, fill_holes, connectivity)
    return (resample.restore_labels(on_grid, affine, image), on_grid, grid_affine, *records)
