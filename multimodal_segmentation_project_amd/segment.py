"""Segmenting with a trained model: the outbound half of the pipeline, the mirror of the loop body of the reference's
test_model.py:242-309 (model(image), torch.argmax(outputs, dim=1), the per-sample per-class Dice / IoU, pred_classes.cpu()).

  predict_labels(model, x, target=None)         uint8 (N, D, H, W) label map, and with a target the exact per-sample counts
  predict_labels_ensemble(models, x, flips)     the label map of the softmax average over mirrored views and / or several models
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
logits nor the probabilities of a view are ever written.  File reading / writing, drawing (matplotlib) and sliding windows
(every scan is squeezed onto the training grid, so there is no window to slide) stay outside.  So do, for the soft restore:
several scans per call, per-class counts against a ground truth on the stored grid, and zoom orders other than 1 and 0.
"""
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


def per_sample_dice_iou(counts, classes=(1, 2, 3)):
    """One {class: (dice, iou)} of Python floats per sample from predict_labels' (N, 3C + 1) counts, by the formula of
    test_model.py:269-276 (a class absent from the sample's label, or one the model does not have, scores 0.0 for both).
    One host copy of the counts, like the reference's .item() calls."""
    rows = counts.cpu().tolist() if isinstance(counts, torch.Tensor) else [list(r) for r in counts]
    if not rows or any(len(r) != len(rows[0]) or len(r) % 3 != 1 for r in rows):
        raise Mi3dError(f"per_sample_dice_iou: (N, 3C + 1) counts expected, got rows of {[len(r) for r in rows]}")
    return [metrics.dice_iou_from_counts(r, len(r) // 3, classes) for r in rows]


RESTORE_MODES = ("nearest", "linear")


def segment_scan(model, image, affine, dataset_name, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192), keep_largest=None,
                 connectivity=1, flips=None, models=None, restore="nearest"):
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
    raises before anything is launched."""
    if restore not in RESTORE_MODES:
        raise Mi3dError(f"segment_scan: restore is one of {RESTORE_MODES}, got {restore!r}")
    ct = dataset_name.lower().endswith("_ct")
    grid, _, grid_affine = resample.resample_scan(image, affine, target_spacing=target_spacing, target_shape=target_shape,
                                                  ct_window=CT_WINDOW if ct else None)
    if not ct:
        grid = preprocess.preprocess_mri(grid)
    if restore == "linear":
        on_grid, votes = predict_labels_ensemble(model if models is None else models, grid[None, None],
                                                 flips=NO_FLIP if flips is None else flips, votes=True)
        stored = resample.restore_labels_soft(votes, affine, image)
        if keep_largest is None:
            return stored, on_grid[0], grid_affine
        cleaned = components.keep_largest(stored, keep=keep_largest, connectivity=connectivity)
        return cleaned.labels, on_grid[0], grid_affine, cleaned
    if flips is None and models is None:
        on_grid = predict_labels(model, grid[None, None])[0]
    else:
        on_grid = predict_labels_ensemble(model if models is None else models, grid[None, None],
                                          flips=NO_FLIP if flips is None else flips)[0]
    if keep_largest is None:
        return resample.restore_labels(on_grid, affine, image), on_grid, grid_affine
    cleaned = components.keep_largest(on_grid, keep=keep_largest, connectivity=connectivity)
    return resample.restore_labels(cleaned.labels, affine, image), cleaned.labels, grid_affine, cleaned
