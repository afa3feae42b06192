"""GPU mirror of the reference's preview figure: visualize_prediction (test_model.py:66-193, called at :299-305 on host copies of
the whole image, label and prediction) and the per-slice overlay of the slider in visualize_nifti.py:29-52.  Only what is drawn
leaves the device: nine 2-D arrays per sample, or one RGB stack per scan.

  foreground_profiles(labels)                        np.sum(label > 0, axis=others) per axis: three int64 device tensors
  best_slices(labels)                                find_best_slice for axes 0, 1, 2: int32 (3,) on the device
  overlay_slice(image, labels, axis, index, ...)     create_overlay of one slice, optionally np.rot90'd
  prediction_panels(image, label, pred)              the 3 x 3 figure's arrays and the three slice indices
  overlay_stack(image, labels, axis)                 create_overlay of every slice of an axis: (n, A, B, 3)

Volumes are 3-D device tensors, dense with any strides (a permuted view, a Fortran-ordered scan, the outputs of
segment.segment_scan and resample.resample_scan as they are); leading singleton dims are squeezed as np.squeeze does at
test_model.py:72-73.  Images are float32 or int16 and must be finite, labels uint8 or int64.  Nothing here synchronises; slice
indices chosen on the device stay there.  Matplotlib, PNG and NIfTI writing stay outside.  Kernels: csrc/preview.hip.
"""
import ctypes as C
import operator

import torch

from . import _lib
from ._lib import Mi3dError, call, ptr, stream_ptr
from ._volume import _IMAGE, _LABEL, _strides, _volume3

VIEW_AXES = (2, 0, 1)          # figure rows: axial, sagittal, coronal (test_model.py:94-96)
_OUT = {torch.float64: _lib.OVERLAY_F64, torch.float32: _lib.OVERLAY_F32, torch.uint8: _lib.OVERLAY_U8}


def _same(what, first, *others):
    for t in others:
        if tuple(t.shape) != tuple(first.shape):
            raise Mi3dError(f"{what}: shapes differ: {tuple(first.shape)} and {tuple(t.shape)}")
    for t in (first, *others):
        _lib.require_cuda(t, what)
        if t.device != first.device:
            raise Mi3dError(f"{what}: tensors on {first.device} and {t.device}")


def _stride_array(t):
    return (C.c_int64 * 3)(*_strides(t))


def _axis(axis, what):
    if axis not in (0, 1, 2):
        raise Mi3dError(f"{what}: axis {axis!r} is not 0, 1 or 2")
    return int(axis)


def _out_code(dtype, what):
    if dtype not in _OUT:
        raise Mi3dError(f"{what}: overlays are float64, float32 or uint8, got {dtype}")
    return _OUT[dtype]


def _slice_shape(shape, axis, rot90):
    a, b = [n for i, n in enumerate(shape) if i != axis]
    return (b, a) if rot90 else (a, b)


def _profiles(labels, code):
    """Zeroed counts of all three axes in one int64 tensor, filled by one read of the labels."""
    d, h, w = labels.shape
    counts = torch.zeros(d + h + w, dtype=torch.int64, device=labels.device)
    call("mi3d_foreground_profiles", ptr(labels), code, d, h, w, *_strides(labels), ptr(counts), stream_ptr())
    return counts


def foreground_profiles(labels):
    """[np.sum(labels > 0, axis=(1, 2)), np.sum(labels > 0, axis=(0, 2)), np.sum(labels > 0, axis=(0, 1))] as int64 device tensors
    (find_best_slice, test_model.py:77-82): exact, one read of the volume, the same bits every run."""
    what = "foreground_profiles"
    labels, code = _volume3(labels, _LABEL, "label", what)
    _same(what, labels)
    d, h, _ = labels.shape
    counts = _profiles(labels, code)
    return [counts[:d], counts[d:d + h], counts[d + h:]]


def _best(labels, code):
    counts = _profiles(labels, code)
    best = torch.empty(3, dtype=torch.int32, device=labels.device)
    call("mi3d_best_slices", ptr(counts), *labels.shape, ptr(best), stream_ptr())
    return best


def best_slices(labels):
    """find_best_slice (test_model.py:75-91) for axes 0, 1, 2 as an int32 (3,) device tensor: the first slice with the most voxels
    > 0, the middle slice n // 2 where there is none."""
    what = "best_slices"
    labels, code = _volume3(labels, _LABEL, "label", what)
    _same(what, labels)
    return _best(labels, code)


def _render(image, icode, labels, lcode, axis, mode, index, k, rot90, dtype, ocode, out_shape, n_slots):
    keys = torch.zeros(2 * n_slots, dtype=torch.int32, device=image.device)
    call("mi3d_slice_minmax", ptr(image), icode, *image.shape, *_strides(image), axis, mode, ptr(index), k, ptr(keys), stream_ptr())
    out = torch.empty(out_shape, dtype=dtype, device=image.device)
    outs = (C.c_void_p * 1)(out.data_ptr())
    call("mi3d_overlay_render", ptr(image), icode, _stride_array(image), ptr(labels), lcode, _stride_array(labels), None, 0, None,
         *image.shape, axis, mode, ptr(index), k, int(bool(rot90)), ptr(keys), ocode, outs, stream_ptr())
    return out


def overlay_slice(image, labels, axis, index, rot90=False, dtype=torch.float64):
    """create_overlay(image_slice, label_slice) (test_model.py:103-125, visualize_nifti.py:29-52) of slice `index` of `axis`:
    (A, B, 3), or np.rot90 of it, (B, A, 3), as test_model.py:129-178 draws it.  index: a Python int (checked), or a 0-dim /
    one-element integer device tensor such as best_slices(labels)[axis], read on the device and clamped to the axis.
    dtype: float64 the reference's bits, float32 one rounding of them, uint8 (255 * overlay).astype(np.uint8) with NaN as 0."""
    what = "overlay_slice"
    image, icode = _volume3(image, _IMAGE, "image", what)
    labels, lcode = _volume3(labels, _LABEL, "label", what)
    axis, ocode = _axis(axis, what), _out_code(dtype, what)
    k = 0
    if isinstance(index, torch.Tensor):
        if index.numel() != 1 or index.dtype not in (torch.int32, torch.int64):
            raise Mi3dError(f"{what}: a device index is one int32 or int64 element, got {tuple(index.shape)} {index.dtype}")
    else:
        try:
            k, index = operator.index(index), None
        except TypeError:
            raise Mi3dError(f"{what}: index {index!r} is neither an integer nor a device tensor") from None
        if not 0 <= k < image.shape[axis]:
            raise Mi3dError(f"{what}: index {k} is outside axis {axis} of {image.shape[axis]} slices")
    _same(what, image, labels)
    if index is not None:
        _lib.require_cuda(index, what)
        if index.device != image.device:
            raise Mi3dError(f"{what}: the index is on {index.device}, the image on {image.device}")
        index = index.reshape(1).to(torch.int32)
    return _render(image, icode, labels, lcode, axis, _lib.PREVIEW_ONE, index, k, rot90, dtype, ocode,
                   (*_slice_shape(image.shape, axis, rot90), 3), 1)


def overlay_stack(image, labels, axis=2, dtype=torch.uint8):
    """create_overlay of EVERY slice of `axis`, each normalised by its own minimum and maximum: (n, A, B, 3), the slider of
    visualize_nifti.py:54-73 for all positions at once (not rotated, as there).  Two launches: the per-slice min / max, the render."""
    what = "overlay_stack"
    image, icode = _volume3(image, _IMAGE, "image", what)
    labels, lcode = _volume3(labels, _LABEL, "label", what)
    axis, ocode = _axis(axis, what), _out_code(dtype, what)
    _same(what, image, labels)
    n = image.shape[axis]
    return _render(image, icode, labels, lcode, axis, _lib.PREVIEW_STACK, None, 0, False, dtype, ocode,
                   (n, *_slice_shape(image.shape, axis, False), 3), n)


def prediction_panels(image, label, pred, dtype=torch.float64):
    """The arrays of the reference's 3 x 3 figure (test_model.py:127-179) and the slice indices it chooses from `label`:
    ([[raw, ground-truth overlay, prediction overlay] for axial (axis 2), sagittal (axis 0), coronal (axis 1)], int32 (3,) indices by
    axis).  Every array is np.rot90'd as the figure's: raw float32 (H, W), overlays `dtype` (H, W, 3).  label and pred may differ in
    dtype and strides (an int64 target, the uint8 map of segment.predict_labels).  Four kernel launches (profiles, best slices,
    three min / max pairs, nine panels) behind the one zero fill of their workspace; no host synchronisation."""
    what = "prediction_panels"
    image, icode = _volume3(image, _IMAGE, "image", what)
    label, lcode = _volume3(label, _LABEL, "label", what)
    pred, pcode = _volume3(pred, _LABEL, "prediction", what)
    ocode = _out_code(dtype, what)
    _same(what, image, label, pred)
    lib, dev, (d, h, w) = _lib.lib(), image.device, image.shape
    ws_bytes = lib.mi3d_preview_workspace_bytes(d, h, w)
    if ws_bytes == 0:
        raise Mi3dError(f"{what}: a side of {tuple(image.shape)} is outside the library's range")
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device=dev)          # counts | best (16 bytes) | keys
    counts, best, keys = ws[:d + h + w], ws[d + h + w:d + h + w + 2].view(torch.int32)[:3], ws[d + h + w + 2:].view(torch.int32)
    panels, outs = [], []
    for a in VIEW_AXES:
        r, c = _slice_shape(image.shape, a, True)
        row = [torch.empty((r, c), dtype=torch.float32, device=dev), torch.empty((r, c, 3), dtype=dtype, device=dev),
               torch.empty((r, c, 3), dtype=dtype, device=dev)]
        panels.append(row)
        outs += [t.data_ptr() for t in row]
    outs = (C.c_void_p * 9)(*outs)
    call("mi3d_foreground_profiles", ptr(label), lcode, d, h, w, *_strides(label), ptr(counts), stream_ptr())
    call("mi3d_best_slices", ptr(counts), d, h, w, ptr(best), stream_ptr())
    call("mi3d_slice_minmax", ptr(image), icode, d, h, w, *_strides(image), 0, _lib.PREVIEW_THREE, ptr(best), 0, ptr(keys), stream_ptr())
    call("mi3d_overlay_render", ptr(image), icode, _stride_array(image), ptr(label), lcode, _stride_array(label), ptr(pred), pcode,
         _stride_array(pred), d, h, w, 0, _lib.PREVIEW_THREE, ptr(best), 0, 1, ptr(keys), ocode, outs, stream_ptr())
    return panels, best
