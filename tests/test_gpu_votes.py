"""GPU tests of the flip / model ensemble votes: mi3d_head_votes (head + softmax + add into the vote volume at the mirrored
voxel, one view per call, the last one ending in argmax, counts and confidence) and segment.predict_labels_ensemble /
segment_scan(flips=, models=) on the whole network.

Reference, input families, allowance and label rule: tests/votes_ref.py (float64 numpy, pinned by tests/test_votes_ref_cpu.py).
`saturated` is compared bit for bit, `spaced` against mi3d_head_labels, `gauss` and the network under the allowance
K_VOTES * views * 2^-24 and the band rule.  Each test prints the worst |delta| / allowance it saw (-s)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_ref as O  # noqa: E402
import votes_ref as VR  # noqa: E402
from test_gpu_segment import NET_CASES  # noqa: E402

import multimodal_segmentation_project_amd as mi  # noqa: E402
from multimodal_segmentation_project_amd import _lib, preprocess, resample, segment  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError, call, ptr  # noqa: E402

DEV = "cuda:0"
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
KEEP = _lib.VOTES_KEEP
LAYOUT_IDS = ["bf16-cin16", "bf16-cin32-stride40", "fp32-cin5"]


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _device_view(view, layout, rng):
    """Operands of a view on the device; the channels beyond Cin (the other half of a concat buffer) hold noise."""
    z, w, b = view
    dtype, cin, zcs = layout
    buf = rng.standard_normal(z.shape[:2] + (zcs,)).astype(np.float32) * 100.0
    buf[:, :, :cin] = z
    zd = torch.from_numpy(buf).to(DEV).to(TORCH_DT[dtype]).contiguous()
    return zd, torch.from_numpy(w.astype(np.float32)).to(DEV), torch.from_numpy(b.astype(np.float32)).to(DEV)


class Run:
    """The outputs of one sequence of mi3d_head_votes calls, every buffer pre-filled with a sentinel."""

    def __init__(self, dviews, shape, layout, c, flips, *, keep=True, confidence=True, target=None):
        n, d, h, w = shape
        nv = len(flips)
        self.votes = torch.full((n, c, d, h, w), -7.0, device=DEV)
        self.labels = torch.full((n, d, h, w), 255, dtype=torch.uint8, device=DEV)
        self.conf = torch.full((n, d, h, w), -7.0, device=DEV) if confidence else None
        self.counts = ws = None
        if target is not None:
            self.counts = torch.full((n, 3 * c + 1), -1, dtype=torch.int64, device=DEV)
            ws = torch.empty(_lib.lib().mi3d_head_votes_workspace_bytes(n, c), dtype=torch.uint8, device=DEV)
        for i, ((zd, wd, bd), f) in enumerate(zip(dviews, flips)):
            last = i == nv - 1
            call("mi3d_head_votes", int(layout[0] == "bf16"), ptr(zd), layout[2], layout[1], ptr(wd), ptr(bd), c, n, d, h, w, f, i, nv,
                 KEEP if keep else 0, ptr(self.votes), ptr(self.labels) if last else None, ptr(self.conf) if last else None,
                 ptr(target) if last else None, ptr(self.counts) if last else None, ptr(ws) if last else None, None)


def _numpy_counts(pred, target, c):
    rows = []
    for p, t in zip(pred, target):
        rows.append([int(((p == k) & (t == k)).sum()) for k in range(c)] + [int((p == k).sum()) for k in range(c)]
                    + [int((t == k).sum()) for k in range(c)] + [int((p == t).sum())])
    return np.array(rows, dtype=np.int64)


def _confidence_of(votes32, labels, views):
    """votes[label] / float(views) in IEEE float32, from the device's own totals."""
    top = np.take_along_axis(votes32, labels[:, None].astype(np.int64), axis=1)[:, 0]
    return top / np.float32(views)


def _family_cases(layout, c):
    for shape in VR.SHAPES:
        for flips in VR.FLIP_SEQUENCES:
            yield shape, flips


@pytest.mark.parametrize("c", VR.CLASSES)
@pytest.mark.parametrize("layout", VR.LAYOUTS, ids=LAYOUT_IDS)
def test_saturated_votes_labels_and_confidence_bit_for_bit(layout, c):
    """Every p is exactly 0, 1, 1/2 or 1/4, so totals, labels (ties between views fall to the lower class) and confidence equal
    the float64 reference exactly: pins the mirror map, the view order, the three modes and the tails with no tolerance."""
    for shape, flips in _family_cases(layout, c):
        case = (shape, layout, c, flips)
        views = VR.make_views("saturated", shape, layout, c, flips)
        want = VR.votes_from_logits([VR.head_logits(*v, shape) for v in views], flips)
        want_labels, _ = VR.labels_and_margin(want)
        rng = np.random.default_rng(VR.case_seed(*case))
        dviews = [_device_view(v, layout, rng) for v in views]
        run = Run(dviews, shape, layout, c, flips)
        votes, labels, conf = _host(run.votes), _host(run.labels), _host(run.conf)
        assert np.array_equal(votes, want.astype(np.float32)), case
        assert np.array_equal(labels, want_labels), case
        assert np.array_equal(conf, _confidence_of(votes, labels, len(flips))), case
        # without MI3D_VOTES_KEEP the last pass does not write the total: the volume holds the views before it (or nothing)
        lean = Run(dviews, shape, layout, c, flips, keep=False, confidence=False)
        before_last = VR.votes_from_logits([VR.head_logits(*v, shape) for v in views[:-1]], flips[:-1]) if len(flips) > 1 else None
        assert np.array_equal(_host(lean.labels), want_labels), case
        assert np.array_equal(_host(lean.votes), np.full_like(votes, -7.0) if before_last is None else before_last.astype(np.float32)), case


@pytest.mark.parametrize("c", VR.CLASSES)
@pytest.mark.parametrize("layout", VR.LAYOUTS, ids=LAYOUT_IDS)
def test_single_unflipped_view_labels_as_head_labels_does(layout, c):
    """`spaced` logits: the softmax keeps their order, so one view with flip 0 must give mi3d_head_labels' labels exactly; a NULL
    vote volume is allowed there."""
    for shape in VR.SHAPES:
        (view,) = VR.make_views("spaced", shape, layout, c, (0,))
        rng = np.random.default_rng(VR.case_seed(shape, layout, c, (0,)))
        zd, wd, bd = _device_view(view, layout, rng)
        n, d, h, w = shape
        want = torch.full((n, d * h * w), 255, dtype=torch.uint8, device=DEV)
        call("mi3d_head_labels", int(layout[0] == "bf16"), ptr(zd), layout[2], layout[1], ptr(wd), ptr(bd), c, n, d * h * w, ptr(want),
             None, None, None, None)
        got = torch.full((n, d, h, w), 255, dtype=torch.uint8, device=DEV)
        call("mi3d_head_votes", int(layout[0] == "bf16"), ptr(zd), layout[2], layout[1], ptr(wd), ptr(bd), c, n, d, h, w, 0, 0, 1, 0,
             None, ptr(got), None, None, None, None, None)
        assert np.array_equal(_host(got).reshape(n, -1), _host(want)), (shape, layout, c)
        assert np.array_equal(_host(want).reshape(n, d, h, w), VR.head_logits(*view, shape).argmax(1)), (shape, layout, c)


@pytest.mark.parametrize("c", VR.CLASSES)
@pytest.mark.parametrize("layout", VR.LAYOUTS, ids=LAYOUT_IDS)
def test_gauss_votes_within_the_allowance_and_labels_by_the_band_rule(layout, c):
    """Also here: counts equal numpy's from the returned labels for a target with out-of-range values, confidence equals
    votes[label] / views bitwise, and a second run gives the same bits."""
    worst = 0.0
    for shape, flips in _family_cases(layout, c):
        case = (shape, layout, c, flips)
        nv = len(flips)
        views = VR.make_views("gauss", shape, layout, c, flips)
        want = VR.votes_from_logits([VR.head_logits(*v, shape) for v in views], flips)
        rng = np.random.default_rng(VR.case_seed(*case))
        dviews = [_device_view(v, layout, rng) for v in views]
        n, v = shape[0], shape[1] * shape[2] * shape[3]
        target = rng.integers(0, c, (n, v))
        bad = rng.random((n, v)) < 0.2
        target[bad] = rng.choice(np.array([-1, c, 255, 2 ** 32 + 1]), int(bad.sum()))
        run = Run(dviews, shape, layout, c, flips, target=torch.from_numpy(target).to(DEV))
        votes, labels, conf, counts = _host(run.votes), _host(run.labels), _host(run.conf), _host(run.counts)
        ratio = float(np.abs(votes.astype(np.float64) - want).max() / VR.allowance(nv))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
        assert VR.label_errors(labels, want, nv) == 0, case
        # the label is the first maximum of the device's own totals, whatever the band allows
        assert np.array_equal(labels, votes.argmax(1)), case
        assert np.array_equal(conf, _confidence_of(votes, labels, nv)), case
        assert np.array_equal(counts, _numpy_counts(labels.reshape(n, -1), target, c)), case
        again = Run(dviews, shape, layout, c, flips, target=torch.from_numpy(target).to(DEV))
        assert torch.equal(again.votes, run.votes) and torch.equal(again.labels, run.labels) and torch.equal(again.conf, run.conf), case
        assert torch.equal(again.counts, run.counts), case
    print(f"gauss {layout} C={c}: worst |delta| / allowance = {worst:.3f}")


def test_head_votes_argument_errors_leave_the_outputs_untouched():
    n, d, h, w, cin, c = 1, 2, 4, 8, 16, 4
    z = torch.zeros((n, d * h * w, cin), device=DEV)
    wt = torch.zeros((c, cin), device=DEV)
    votes = torch.full((n, c, d, h, w), -7.0, device=DEV)
    labels = torch.full((n, d, h, w), 255, dtype=torch.uint8, device=DEV)
    conf = torch.full((n, d, h, w), -7.0, device=DEV)
    tgt = torch.zeros((n, d * h * w), dtype=torch.int64, device=DEV)
    counts = torch.full((n, 3 * c + 1), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty(_lib.lib().mi3d_head_votes_workspace_bytes(n, c), dtype=torch.uint8, device=DEV)

    def go(match, *, dtype=0, zp=ptr(z), zcs=cin, cin_=cin, wp=ptr(wt), cout=c, n_=n, d_=d, flip=0, view=0, views=1, flags=0,
           vp=ptr(votes), lp=ptr(labels), cp=None, tp=None, kp=None, wsp=None):
        with pytest.raises(Mi3dError, match=match):
            call("mi3d_head_votes", dtype, zp, zcs, cin_, wp, None, cout, n_, d_, h, w, flip, view, views, flags, vp, lp, cp, tp, kp, wsp, None)

    go("null", zp=None)
    go("null", wp=None)
    go("dtype", dtype=2)
    go("channels", zcs=8)
    go("channels", cin_=0)
    go("classes", cout=9)
    go("classes", cout=0)
    go("batch", n_=0)
    go("volume", d_=0)
    go("volume", d_=2 ** 30)
    go("flip", flip=8)
    go("flip", flip=-1)
    go("view", views=0)
    go("view", view=1)
    go("view", view=-1, views=2, lp=None)
    go("flags", flags=2)
    go("last view", view=0, views=2)                                   # labels on an earlier view
    go("last view", view=0, views=2, lp=None, cp=ptr(conf))
    go("last view", view=0, views=2, lp=None, tp=ptr(tgt), kp=ptr(counts), wsp=ptr(ws))
    go("labels_out", lp=None)
    go("come together", tp=ptr(tgt))
    go("come together", kp=ptr(counts))
    go("workspace", tp=ptr(tgt), kp=ptr(counts))
    go("vote volume", vp=None, view=1, views=2)
    go("vote volume", vp=None, view=0, views=2, lp=None)
    go("vote volume", vp=None, flags=KEEP)
    assert _lib.lib().mi3d_head_votes_workspace_bytes(1, 9) == 0
    assert bool((_host(votes) == -7.0).all()) and bool((_host(labels) == 255).all()) and bool((_host(conf) == -7.0).all())
    assert bool((_host(counts) == -1).all())


# ---- the whole network ----------------------------------------------------------------------------------------------------------
def _model(seed, classes, features, dtype):
    torch.manual_seed(seed)
    kw = {} if features is None else {"features": features}
    model = mi.UNet3D(in_channels=1, out_channels=classes, dropout_rate=0.0, **kw).to(DEV).eval()
    model.compute_dtype = TORCH_DT[dtype]
    with torch.no_grad():          # as test_gpu_segment: keeps the activations O(1), so the label map is not one class
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.fill_(0.1)
    return model


def _view_logits(models, x, flips):
    """The logits of every view on the existing route, model-major: model(torch.flip(x, dims of f)) on the host, float64."""
    out = []
    with torch.no_grad():
        for m in models:
            for f in flips:
                dims = segment._flip_dims(f)
                out.append(_host(m(torch.flip(x, dims) if dims else x)).astype(np.float64))
    return out


@pytest.mark.parametrize("shape,features", NET_CASES, ids=["16x16x16-N2", "18x20x17-odd", "6x10x7-odd-small"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_labels_ensemble_against_the_models_own_logits(dtype, shape, features):
    """Eight flips of one model, two models x two flips, three views (a total that float(views) does not divide exactly) and
    NO_FLIP against predict_labels.  The reference votes come from model(torch.flip(x, ...)) on the logits route."""
    classes = 4
    a, b = _model(7, classes, features, dtype), _model(8, classes, features, dtype)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=gen).to(DEV)
    n = shape[0]
    target = torch.randint(0, classes, (n, 1) + shape[2:], generator=gen).to(DEV)
    worst = 0.0
    for models, flips in (([a], segment.FLIPS8), ([a, b], (0, 5)), ([b], (6, 0, 3)), ([a], segment.NO_FLIP)):
        nv = len(models) * len(flips)
        want = VR.votes_from_logits(_view_logits(models, x, flips), list(flips) * len(models))
        assert VR.band_share(want, nv) <= VR.BAND_CAP
        labels, counts, conf, mean = segment.predict_labels_ensemble(models if len(models) > 1 else models[0], x, flips=flips,
                                                                     target=target, confidence=True, votes=True)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n,) + shape[2:]
        assert conf.dtype == torch.float32 and tuple(conf.shape) == (n,) + shape[2:]
        assert mean.dtype == torch.float32 and tuple(mean.shape) == (n, classes) + shape[2:]
        lab, cf, mn = _host(labels), _host(conf), _host(mean)
        # mean = total / views: one more float32 rounding on top of the total's allowance
        ratio = float(np.abs(mn.astype(np.float64) * nv - want).max() / (VR.allowance(nv) + nv * VR.U))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (flips, ratio)
        assert VR.label_errors(lab, want, nv) == 0, flips
        # confidence = total[label] / views in IEEE float32; the mean is torch's division of the same totals, which is the same
        # number where views is a power of two (exact) and within an ulp otherwise
        top = np.take_along_axis(mn, lab[:, None].astype(np.int64), axis=1)[:, 0]
        assert np.array_equal(cf, top) if nv & (nv - 1) == 0 else bool((np.abs(cf - top) <= np.spacing(top)).all()), flips
        assert np.array_equal(_host(counts), _numpy_counts(lab.reshape(n, -1), _host(target).reshape(n, -1), classes)), flips
        assert len(np.unique(lab)) > 1
        # the plain call returns the same labels, and a second call the same bits
        assert torch.equal(segment.predict_labels_ensemble(models, x, flips=flips), labels)
        again = segment.predict_labels_ensemble(models, x, flips=flips, confidence=True, votes=True)
        assert torch.equal(again[0], labels) and torch.equal(again[1], conf) and torch.equal(again[2], mean)
    # NO_FLIP (the last round): predict_labels' labels outside the band
    plain = _host(segment.predict_labels(a, x))
    _, margin = VR.labels_and_margin(want)
    clear = margin > 2.0 * VR.allowance(1)
    assert np.array_equal(lab[clear], plain[clear]) and clear.mean() >= 1.0 - VR.BAND_CAP
    print(f"network {dtype} {shape}: worst |delta| / allowance = {worst:.3f}")


def test_segment_scan_routes_flips_and_models_through_the_ensemble():
    a, b = _model(3, 4, None, "bf16"), _model(4, 4, None, "bf16")
    rng = np.random.default_rng(21)
    grid_shape = (16, 16, 16)
    perm, signs = (2, 0, 1), (-1, 1, -1)
    scan = O.store_as(rng.integers(-1024, 3000, (7, 10, 13)).astype(np.int16), perm, signs)
    image = torch.from_numpy(np.ascontiguousarray(scan)).to(DEV)
    aff = O.affine_for(perm, signs)
    x, _, want_aff = resample.resample_scan(image, aff, target_shape=grid_shape)
    x = preprocess.preprocess(x, "chaos_mri")
    # both None: today's route and bits
    stored, on_grid, grid_aff = segment.segment_scan(a, image, aff, "chaos_mri", target_shape=grid_shape)
    want_grid = segment.predict_labels(a, x[None, None])[0]
    assert torch.equal(on_grid, want_grid) and torch.equal(stored, resample.restore_labels(want_grid, aff, image))
    for kw, models, flips in (({"flips": segment.FLIPS8}, a, segment.FLIPS8), ({"models": [a, b]}, [a, b], segment.NO_FLIP),
                              ({"flips": (0, 7), "models": [b, a]}, [b, a], (0, 7))):
        stored, on_grid, grid_aff = segment.segment_scan(a, image, aff, "chaos_mri", target_shape=grid_shape, **kw)
        want_grid = segment.predict_labels_ensemble(models, x[None, None], flips=flips)[0]
        assert on_grid.dtype == torch.uint8 and tuple(on_grid.shape) == grid_shape and torch.equal(on_grid, want_grid), kw
        assert np.array_equal(grid_aff, want_aff)
        assert tuple(stored.shape) == scan.shape and torch.equal(stored, resample.restore_labels(want_grid, aff, image)), kw


def test_predict_labels_ensemble_refuses_what_is_not_its_path():
    x = torch.zeros((1, 1, 16, 16, 16), device=DEV)
    model = _model(0, 4, None, "bf16")
    before = _lib.launches
    with pytest.raises(Mi3dError, match="eval"):
        segment.predict_labels_ensemble([model, mi.UNet3D(in_channels=1, out_channels=4).to(DEV).train()], x)
    with pytest.raises(Mi3dError, match="out_channels"):
        segment.predict_labels_ensemble([model, mi.UNet3D(in_channels=1, out_channels=2).to(DEV).eval()], x)
    with pytest.raises(Mi3dError, match="flip code"):
        segment.predict_labels_ensemble(model, x, flips=(0, 8))
    with pytest.raises(Mi3dError, match="target"):
        segment.predict_labels_ensemble(model, x, target=torch.zeros((1, 1, 8, 8, 8), dtype=torch.int64, device=DEV))
    assert _lib.launches == before
