"""GPU tests of the preview figure (preview.py, csrc/preview.hip) against the arrays the reference's own visualize_prediction
recorded (tests/golden/preview.npz) and against the numpy restatement tests/preview_ref.py that tests/test_preview_cpu.py pins to
them.  Every comparison is exact: counts and indices are integers, float64 panels are the reference's values (NaN positions
included; a signed zero is not distinguished, np.array_equal does not), float32 panels are np.float32 of them and uint8 panels
(255 * value).astype(np.uint8) with 0 on NaN pixels.

Shapes: preview_ref.SHAPES are ragged against 16-byte vectors, 64-lane waves and a workgroup's span, with the long axis fastest
and slowest.  None of them lets a uint8 label row be read 16 bytes at a time or a uint8 panel row be stored so, so two more are
run against the restatement: (16, 32, 48), where every kernel takes its vector form, and (2, 3, 1040), a row of 65 16-byte lanes
(two chunks of the fastest axis)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as P  # noqa: E402

from multimodal_segmentation_project_amd import preview  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402

DEV = "cuda:0"
ALL_SHAPES = P.SHAPES + ((16, 32, 48), (2, 3, 1040))
DTYPES = {torch.float64: np.float64, torch.float32: np.float32, torch.uint8: np.uint8}
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")  # noqa: E731


@functools.lru_cache(maxsize=None)
def case(name, shape):
    return P.make_case(name, shape)


@functools.lru_cache(maxsize=None)
def reference_panels(name, shape):
    return P.panels(*case(name, shape))


@functools.lru_cache(maxsize=None)
def reference_stack(name, shape, axis):
    image, label, _ = case(name, shape)
    return P.overlay_stack(image, label, axis)


def dev(a, layout="C"):
    """The array on the device, C-ordered, Fortran-ordered, or as a permuted view of a contiguous (W, D, H) tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if layout == "F":
        return t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    if layout == "P":
        return t.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert layout == "C"
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check_panels(got, best, want, want_best, np_dtype, what):
    assert best.dtype == torch.int32 and np.array_equal(host(best), want_best), (what, host(best), want_best)
    flat = [host(t) for row in got for t in row]
    for i, (g, w) in enumerate(zip(flat, want)):
        w = w if i % 3 == 0 else P.as_dtype(w, np_dtype)
        assert P.same_values(g, np.ascontiguousarray(w)), (what, i, g.dtype, g.shape, w.shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name,shape", P.RECORDED, ids=[P.key(c, s) for c, s in P.RECORDED])
def test_panels_equal_the_recorded_figure(golden, name, shape, dtype):
    g, pre = golden("preview"), P.key(name, shape)
    image, label, pred = dev(g[f"{pre}/image"]), dev(g[f"{pre}/label"]).long(), dev(g[f"{pre}/pred"])
    got, best = preview.prediction_panels(image[None], label[None, None], pred[None], dtype=dtype)      # squeezed as np.squeeze does
    check_panels(got, best, [g[f"{pre}/panel_{i}"] for i in range(9)], g[f"{pre}/best"], DTYPES[dtype], pre)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids)
@pytest.mark.parametrize("name", P.CASES)
def test_every_case_on_every_shape(name, shape):
    image, label, pred = case(name, shape)
    want, want_best = reference_panels(name, shape)
    counts = preview.foreground_profiles(dev(label))
    for a, (c, w) in enumerate(zip(counts, P.foreground_profiles(label))):
        assert c.dtype == torch.int64 and np.array_equal(host(c), w), (name, shape, a)
    for c, w in zip(preview.foreground_profiles(dev(label.astype(np.uint8))), P.foreground_profiles(label)):
        assert np.array_equal(host(c), w)
    assert np.array_equal(host(preview.best_slices(dev(label))), want_best)
    # int64 target + uint8 prediction (segment.predict_labels' dtype), then uint8 target + int64 prediction
    got, best = preview.prediction_panels(dev(image), dev(label), dev(pred))
    check_panels(got, best, want, want_best, np.float64, (name, shape))
    got, best = preview.prediction_panels(dev(image), dev(label.astype(np.uint8)), dev(pred).long(), dtype=torch.uint8)
    check_panels(got, best, want, want_best, np.uint8, (name, shape))


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids)
def test_stack_and_slices(shape, axis):
    image, label, _ = case("big_label", shape)
    want = reference_stack("big_label", shape, axis)
    di, dl = dev(image), dev(label)
    stacks = {}
    for dtype, np_dtype in DTYPES.items():
        stacks[dtype] = got = host(preview.overlay_stack(di, dl, axis=axis, dtype=dtype))
        assert P.same_values(got, P.as_dtype(want, np_dtype)), (shape, axis, dtype)
    n = shape[axis]
    for k in sorted({0, n // 2, n - 1}):
        for dtype in DTYPES:
            assert P.same_values(host(preview.overlay_slice(di, dl, axis, k, dtype=dtype)), stacks[dtype][k]), (shape, axis, k, dtype)
    k = n // 3
    on_device = torch.tensor(k, device=DEV)                                   # 0-dim int64
    got = host(preview.overlay_slice(di, dl, axis, on_device, rot90=True))
    assert P.same_values(got, np.ascontiguousarray(np.rot90(want[k])))
    got = host(preview.overlay_slice(di, dl.to(torch.uint8), axis, torch.tensor([k], device=DEV, dtype=torch.int32), dtype=torch.float32))
    assert P.same_values(got, want[k].astype(np.float32))


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("shape", ((17, 33, 65), (16, 32, 48)), ids=ids)
def test_int16_image_stack(shape, axis):
    image, label, _ = case("random", shape)
    image = np.round(image).astype(np.int16)
    want = P.overlay_stack(image, label, axis)
    for layout in "CF":
        got = host(preview.overlay_stack(dev(image, layout), dev(label, layout), axis=axis, dtype=torch.float64))
        assert P.same_values(got, want), (shape, axis, layout)


def test_flat_slices_hold_nan_where_the_reference_does():
    shape = (17, 33, 65)
    image, label, pred = case("flat", shape)
    want, _ = reference_panels("flat", shape)
    got, _ = preview.prediction_panels(dev(image), dev(label), dev(pred), dtype=torch.float32)
    for i in (1, 2, 4, 5, 7, 8):
        g = host(got[i // 3][i % 3])
        assert np.isnan(want[i]).any() and not np.isnan(want[i]).all()
        assert np.array_equal(np.isnan(g), np.isnan(want[i]))
    stack = host(preview.overlay_stack(dev(np.full(shape, 3.25, dtype=np.float32)), dev(label), axis=1, dtype=torch.uint8))
    assert P.same_values(stack, P.as_dtype(P.overlay_stack(np.full(shape, 3.25, dtype=np.float32), label, 1), np.uint8))


def _everything(image, label, pred):
    """Every output of the module for one input triple, as host arrays."""
    out = [host(c) for c in preview.foreground_profiles(label)]
    out.append(host(preview.best_slices(label)))
    for dtype in DTYPES:
        got, best = preview.prediction_panels(image, label, pred, dtype=dtype)
        out += [host(t) for row in got for t in row] + [host(best)]
        out += [host(preview.overlay_stack(image, label, axis=a, dtype=dtype)) for a in (0, 1, 2)]
    return out


def _bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ids)
def test_strides_do_not_change_a_bit(shape):
    image, label, pred = case("random", shape)
    want = _everything(dev(image), dev(label), dev(pred))
    for layout in "FP":
        di, dl, dp = dev(image, layout), dev(label, layout), dev(pred, layout)
        assert not di.is_contiguous() or min(shape) == 1
        got = _everything(di, dl, dp)
        assert len(got) == len(want) and all(_bitwise(g, w) for g, w in zip(got, want)), (shape, layout)
    # each volume with strides of its own
    got = _everything(dev(image, "F"), dev(label, "P"), dev(pred, "C"))
    assert all(_bitwise(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("shape", ((17, 33, 65), (4, 6, 300), (16, 32, 48)), ids=ids)
def test_two_runs_give_the_same_bits(shape):
    image, label, pred = case("big_label", shape)
    for layout in "CF":
        args = dev(image, layout), dev(label, layout), dev(pred, layout)
        first, second = _everything(*args), _everything(*args)
        assert all(_bitwise(a, b) for a, b in zip(first, second))


def test_bad_arguments_raise_before_any_launch():
    from multimodal_segmentation_project_amd import _lib
    image, label, pred = (dev(a) for a in case("random", (5, 7, 9)))
    torch.cuda.synchronize()
    before = _lib.launches
    with pytest.raises(Mi3dError, match="shapes differ"):
        preview.prediction_panels(image, label, pred[:, :, :8].contiguous())
    with pytest.raises(Mi3dError, match="3-D"):
        preview.overlay_stack(image[0], label[0])
    with pytest.raises(Mi3dError, match="not dense"):
        preview.foreground_profiles(label[:, ::2])
    with pytest.raises(Mi3dError, match="label is torch.uint8 or torch.int64"):
        preview.overlay_stack(image, label.float())
    for axis, n in enumerate(image.shape):
        with pytest.raises(Mi3dError, match=f"index {n} is outside axis {axis}"):
            preview.overlay_slice(image, label, axis, n)
    with pytest.raises(Mi3dError, match="no CPU fallback"):
        preview.overlay_stack(image, label.cpu())
    assert _lib.launches == before
