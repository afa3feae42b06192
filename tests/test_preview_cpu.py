"""The preview figure's yardstick and host side, no GPU needed.

tests/golden/preview.npz holds the nine arrays the reference's own visualize_prediction (test_model.py:66-193) handed to imshow
(tools/gen_golden.py --only preview).  The numpy restatement tests/preview_ref.py is pinned to them here, value for value with
NaN positions included, and is then the reference of tests/test_gpu_preview.py on shapes the fixture does not hold.  The host
checks of preview.py are run on CPU tensors: each must raise for its own reason before the device is looked at."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preview_ref as P  # noqa: E402

from multimodal_segmentation_project_amd import preview  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402

RECORDED = [pytest.param(c, s, id=P.key(c, s)) for c, s in P.RECORDED]


@pytest.mark.parametrize("case,shape", RECORDED)
def test_restatement_equals_the_recorded_figure(golden, case, shape):
    g, pre = golden("preview"), P.key(case, shape)
    image, label, pred = P.make_case(case, shape)
    assert np.array_equal(image, g[f"{pre}/image"]) and np.array_equal(label, g[f"{pre}/label"]) and np.array_equal(pred, g[f"{pre}/pred"])
    panels, best = P.panels(image, label, pred)
    assert np.array_equal(best, g[f"{pre}/best"]) and best.dtype == np.int32
    for i, p in enumerate(panels):
        assert P.same_values(p, g[f"{pre}/panel_{i}"]), (pre, i)


def test_recorded_shapes_and_dtypes(golden):
    g = golden("preview")
    d, h, w = shape = (17, 33, 65)
    pre = P.key("random", shape)
    assert [g[f"{pre}/panel_{i}"].shape for i in range(9)] == [(h, d), (h, d, 3), (h, d, 3), (w, h), (w, h, 3), (w, h, 3), (w, d), (w, d, 3),
                                                                (w, d, 3)]
    assert [g[f"{pre}/panel_{i}"].dtype for i in range(3)] == [np.float32, np.float64, np.float64]


@pytest.mark.parametrize("shape", P.SHAPES)
def test_cases_choose_the_slices_they_are_built_for(shape):
    assert list(P.best_slices(P.make_case("tie", shape)[1])) == [max(n // 3, 1) for n in shape]
    assert list(P.best_slices(P.make_case("background", shape)[1])) == [n // 2 for n in shape]
    assert list(P.best_slices(P.make_case("last", shape)[1])) == [n - 1 for n in shape]
    _, label, _ = P.make_case("tie", shape)
    for a, c in enumerate(P.foreground_profiles(label)):
        assert c[max(shape[a] // 3, 1)] == c[shape[a] - 1] == c.max() == 4
    _, big, _ = P.make_case("big_label", shape)
    assert (big >= 4).any() and np.array_equal(P.foreground_profiles(big)[0], (big != 0).sum(axis=(1, 2)))


def test_flat_slice_is_nan_exactly_where_no_colour_lands(golden):
    g, pre = golden("preview"), P.key("flat", P.SHAPES[0])
    label, pred, best = g[f"{pre}/label"], g[f"{pre}/pred"], g[f"{pre}/best"]
    for v, a in enumerate(P.VIEW_AXES):
        for j, lab in ((1, label), (2, pred)):
            grey = np.rot90(~np.isin(P.take_slice(lab, a, best[a]), (1, 2, 3)))
            panel = g[f"{pre}/panel_{3 * v + j}"]
            assert grey.any() and not grey.all()
            assert np.array_equal(np.isnan(panel), np.repeat(grey[..., None], 3, axis=-1))
    big = golden("preview")[P.key("big_label", P.SHAPES[0]) + "/panel_1"]
    assert not np.isnan(big).any()


def test_output_dtypes():
    ov = np.array([[[0.0, 0.65, 1.0], [np.nan, 0.5, 0.9999999]]])
    assert P.as_dtype(ov, np.float64) is ov
    assert P.as_dtype(ov, np.float32).dtype == np.float32
    assert P.as_dtype(ov, np.uint8).tolist() == [[[0, 165, 255], [0, 127, 254]]]          # truncation; NaN -> 0


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def _volumes(shape=(4, 5, 6)):
    return torch.zeros(shape), torch.zeros(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.uint8)


def test_mismatched_shapes():
    image, label, pred = _volumes()
    with pytest.raises(Mi3dError, match="shapes differ"):
        preview.overlay_stack(image, label[:, :, :5].contiguous())
    with pytest.raises(Mi3dError, match="shapes differ"):
        preview.prediction_panels(image, label, pred[:3])
    with pytest.raises(Mi3dError, match="shapes differ"):
        preview.overlay_slice(image[1:], label, 0, 0)


def test_two_dimensional_input():
    image, label, _ = _volumes()
    with pytest.raises(Mi3dError, match="3-D"):
        preview.foreground_profiles(label[0])
    with pytest.raises(Mi3dError, match="3-D"):
        preview.overlay_stack(image[0], label[0])
    with pytest.raises(Mi3dError, match="3-D"):
        preview.best_slices(torch.zeros((2, 4, 5, 6), dtype=torch.uint8))          # only singleton leading dims are squeezed


def test_non_dense_view():
    image, label, pred = _volumes((4, 6, 8))
    with pytest.raises(Mi3dError, match="not dense"):
        preview.foreground_profiles(label[:, ::2])
    with pytest.raises(Mi3dError, match="not dense"):
        preview.prediction_panels(image[:, :, 1:], label[:, :, 1:].contiguous(), pred[:, :, 1:].contiguous())
    with pytest.raises(Mi3dError, match="not dense"):
        preview.overlay_stack(image, label[:1].expand(4, 6, 8))          # stride 0


def test_dtypes():
    image, label, pred = _volumes()
    with pytest.raises(Mi3dError, match="label is torch.uint8 or torch.int64"):
        preview.foreground_profiles(image)
    with pytest.raises(Mi3dError, match="label is torch.uint8 or torch.int64"):
        preview.overlay_stack(image, label.float())
    with pytest.raises(Mi3dError, match="prediction is torch.uint8 or torch.int64"):
        preview.prediction_panels(image, label, pred.to(torch.int32))
    with pytest.raises(Mi3dError, match="image is torch.float32 or torch.int16"):
        preview.overlay_stack(image.double(), label)
    with pytest.raises(Mi3dError, match="overlays are float64, float32 or uint8"):
        preview.overlay_stack(image, label, dtype=torch.float16)


def test_index_and_axis():
    image, label, _ = _volumes()
    for axis, n in enumerate(image.shape):
        for k in (-1, n):
            with pytest.raises(Mi3dError, match=f"index {k} is outside axis {axis} of {n} slices"):
                preview.overlay_slice(image, label, axis, k)
    with pytest.raises(Mi3dError, match="neither an integer nor a device tensor"):
        preview.overlay_slice(image, label, 0, 1.0)
    with pytest.raises(Mi3dError, match="one int32 or int64 element"):
        preview.overlay_slice(image, label, 0, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(Mi3dError, match="axis 3 is not 0, 1 or 2"):
        preview.overlay_stack(image, label, axis=3)


def test_no_cpu_fallback():
    image, label, pred = _volumes()
    for fn in (lambda: preview.foreground_profiles(label), lambda: preview.best_slices(pred), lambda: preview.overlay_stack(image, label),
               lambda: preview.overlay_slice(image, label, 1, 2), lambda: preview.prediction_panels(image, label, pred)):
        with pytest.raises(Mi3dError, match="no CPU fallback"):
            fn()


def test_leading_singleton_dims_are_squeezed():
    label = torch.zeros((1, 1, 4, 5, 6), dtype=torch.int64)
    with pytest.raises(Mi3dError, match="no CPU fallback"):          # every shape check passed
        preview.prediction_panels(torch.zeros((1, 4, 5, 6)), label, torch.zeros((4, 5, 6), dtype=torch.uint8))
