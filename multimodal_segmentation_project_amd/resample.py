"""GPU mirror of the resampling that puts a decoded scan on the training grid: the four scipy.ndimage.zoom calls of the
reference's offline scripts (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same calls in
chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94).  File decoding, RAS reorientation and the
TotalSegmentator label merge stay outside: they are file and header work, not arithmetic.

  zoom_output_shape(shape, factors)        scipy's output-shape rule
  axis_table(n_in, n_out, order)           float64 host tables of one axis (tap indices / weights, or nearest indices)
  zoom(volume, factors, order)             zoom(volume, factors, order=order, mode='nearest', prefilter=False), order 3 or 0
  resample_to_grid(image, spacing, ...)    the two-stage chain of the scripts (isotropic spacing, then the target shape)
  resample_labels_to_grid(label, spacing)  its label half alone: both order-0 stages composed into one gather

Everything that decides WHICH voxels are read (coordinates, floor, rounding, clamping, spline weights) is computed here on
the host in float64 exactly as scipy does it; the kernels (csrc/resample.hip) only gather and sum.
"""
import collections

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError, call, ptr, stream_ptr

# one row of a cubic table as the kernel reads it (csrc/resample.hip CubicRow, include/mi3d.h)
_ROW = np.dtype([("idx", "<i4", (4,)), ("w", "<f8", (4,))])
assert _ROW.itemsize == 48

TABLE_CACHE_SIZE = 256     # device tables kept (least recently used first out); one chain with labels uses at most 9
_device_tables = collections.OrderedDict()     # (n_in, n_out, order, device) -> device tensor
table_uploads = 0          # host-to-device table copies made so far (a stream of same-shaped scans adds none)


def zoom_output_shape(shape, factors):
    """Per axis int(round(n_in * factor)), Python's round (ties to even), factor a float64."""
    f = _factors(factors, len(shape))
    return tuple(int(round(int(n) * z)) for n, z in zip(shape, f))


def _factors(factors, ndim):
    f = np.asarray(factors, dtype=np.float64)
    if f.ndim == 0:
        f = np.full(ndim, float(f))
    if f.shape != (ndim,):
        raise Mi3dError(f"zoom: {ndim} axes need one factor or {ndim}, got shape {f.shape}")
    return [float(z) for z in f]


def _coords(n_in, n_out):
    # scipy recomputes the zoom from the two shapes: (n_in - 1) / (n_out - 1), and 1 for a single output
    z = float(n_in - 1) / float(n_out - 1) if n_out > 1 else 1.0
    return np.arange(n_out, dtype=np.float64) * z


def axis_table(n_in, n_out, order):
    """Host tables of one axis, one row per output index.
    order 0: int32 (n_out,) input index floor(c + 0.5), clamped.
    order 3: (int32 (n_out, 4) tap indices floor(c) - 1 .. floor(c) + 2, each clamped; float64 (n_out, 4) B-spline weights)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise Mi3dError(f"axis_table: sides must be positive, got {n_in} -> {n_out}")
    cc = _coords(n_in, n_out)
    if order == 0:
        return np.clip(np.floor(cc + 0.5), 0, n_in - 1).astype(np.int32)
    if order != 3:
        raise Mi3dError(f"axis_table: order {order} is not supported (3 = cubic B-spline, 0 = nearest)")
    f = np.floor(cc)
    t = cc - f
    idx = np.clip(f[:, None] + np.arange(-1.0, 3.0)[None, :], 0, n_in - 1).astype(np.int32)
    w = np.stack([(1.0 - t) ** 3 / 6.0,
                  (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
                  (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0,
                  t ** 3 / 6.0], axis=1)
    return idx, w


def _upload(host, device):
    global table_uploads
    table_uploads += 1
    return torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1)).to(device)


def _cached(key, build, device):
    """Device copy of a host table: uploaded on first use, then served from an LRU of TABLE_CACHE_SIZE entries, so scans
    of ever-new shapes cannot pile tables up for the life of the process.  An evicted tensor that a queued launch still
    reads stays valid: torch's allocator reuses a block only in stream order."""
    t = _device_tables.get(key)
    if t is None:
        t = _device_tables[key] = _upload(build(), device)
        while len(_device_tables) > TABLE_CACHE_SIZE:
            _device_tables.popitem(last=False)
    else:
        _device_tables.move_to_end(key)
    return t


def _cubic_rows(n_in, n_out):
    rows = np.zeros(int(n_out), dtype=_ROW)
    rows["idx"], rows["w"] = axis_table(n_in, n_out, 3)
    return rows


def _device_table(n_in, n_out, order, device):
    key = (int(n_in), int(n_out), order, str(device))
    return _cached(key, lambda: _cubic_rows(n_in, n_out) if order == 3 else axis_table(n_in, n_out, 0), device)


def _composed_index_table(n_in, n_mid, n_out, device):
    """Two order-0 zooms along one axis as ONE gather: table1[table2]."""
    key = (int(n_in), (int(n_mid), int(n_out)), 0, str(device))
    return _cached(key, lambda: compose_index_tables(axis_table(n_in, n_mid, 0), axis_table(n_mid, n_out, 0)), device)


def compose_index_tables(first, second):
    return np.ascontiguousarray(first[second], dtype=np.int32)


def clear_table_cache():
    _device_tables.clear()


def _check_volume(volume, what):
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise Mi3dError(f"{what}: one 3-D volume (D, H, W) expected, got {tuple(getattr(volume, 'shape', ()))}")
    _lib.require_cuda(volume, what)
    if min(volume.shape) < 1:
        raise Mi3dError(f"{what}: zero-sized axis in {tuple(volume.shape)}")


def _check_out_shape(shape, what):
    if min(shape) < 1:
        raise Mi3dError(f"{what}: the zoom leaves no voxel on some axis (output shape {tuple(shape)})")
    return tuple(int(n) for n in shape)


def _image(volume, what):
    if not volume.is_floating_point():
        raise Mi3dError(f"{what}: order 3 needs a floating-point volume, got {volume.dtype}")
    return volume.contiguous().float()


def _check_integer(volume, what):
    if volume.is_floating_point() or volume.is_complex() or volume.dtype == torch.bool:
        raise Mi3dError(f"{what}: order 0 needs an integer volume, got {volume.dtype}")


def _labels(volume, what):
    _check_integer(volume, what)
    return volume.contiguous().long()


def _cubic(x, out_shape, out=None, ct_window=None):
    dev = x.device
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    tabs = [_device_table(n, m, 3, dev) for n, m in zip(x.shape, out_shape)]
    lo, hi = (float(ct_window[0]), float(ct_window[1])) if ct_window is not None else (0.0, 1.0)
    call("mi3d_zoom3_cubic", ptr(x), ptr(out), *x.shape, *out_shape, ptr(tabs[0]), out_shape[0], ptr(tabs[1]), out_shape[1],
         ptr(tabs[2]), out_shape[2], int(ct_window is not None), lo, hi, stream_ptr())
    return out


def _nearest(x, out_shape, tabs):
    out = torch.empty(out_shape, dtype=torch.int64, device=x.device)
    call("mi3d_zoom3_nearest_i64", ptr(x), ptr(out), *x.shape, *out_shape, ptr(tabs[0]), out_shape[0], ptr(tabs[1]),
         out_shape[1], ptr(tabs[2]), out_shape[2], stream_ptr())
    return out


def zoom(volume, factors, order=3):
    """scipy.ndimage.zoom(volume, factors, order=order, mode='nearest', prefilter=False) of one 3-D device tensor.
    order 3: floating input -> float32; order 0: integer input -> int64."""
    if order not in (0, 3):
        raise Mi3dError(f"zoom: order {order} is not supported (3 = cubic B-spline, 0 = nearest)")
    _check_volume(volume, "zoom")
    x = _image(volume, "zoom") if order == 3 else _labels(volume, "zoom")
    out_shape = _check_out_shape(zoom_output_shape(x.shape, factors), "zoom")
    if order == 3:
        return _cubic(x, out_shape)
    return _nearest(x, out_shape, [_device_table(n, m, 0, x.device) for n, m in zip(x.shape, out_shape)])


def chain_shapes(shape, spacing, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192)):
    """(stage-1 factors, stage-1 shape, stage-2 factors) of the scripts' chain (amos_ct_resample.py:56,64-66)."""
    scale = np.asarray(spacing, dtype=np.float64) / np.asarray(target_spacing, dtype=np.float64)
    if scale.shape != (3,):
        raise Mi3dError(f"resample_to_grid: spacing and target_spacing need three values, got {spacing} / {target_spacing}")
    shape1 = _check_out_shape(zoom_output_shape(shape, scale), "resample_to_grid")
    factors2 = [int(target_shape[i]) / shape1[i] for i in range(3)]
    shape2 = zoom_output_shape(shape1, factors2)
    if tuple(shape2) != tuple(int(n) for n in target_shape):
        raise Mi3dError(f"resample_to_grid: stage 2 gives {shape2}, not the target {tuple(target_shape)}")
    return [float(z) for z in scale], shape1, factors2


def resample_labels_to_grid(label, spacing, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192)):
    """The label half of the chain (amos_ct_resample.py:93,97): both order-0 zooms as ONE gather of the voxels that are kept."""
    _check_volume(label, "resample_labels_to_grid")
    lab = _labels(label, "resample_labels_to_grid")
    _, shape1, _ = chain_shapes(lab.shape, spacing, target_spacing, target_shape)
    target = tuple(int(n) for n in target_shape)
    tabs = [_composed_index_table(n, m, o, lab.device) for n, m, o in zip(lab.shape, shape1, target)]
    return _nearest(lab, target, tabs)


def _workspace(shape1, device):
    nbytes = _lib.lib().mi3d_zoom3_workspace_bytes(*shape1)
    if nbytes == 0:
        msg = _lib.lib().mi3d_last_error()
        raise Mi3dError(f"mi3d_zoom3_workspace_bytes{tuple(shape1)} failed: {msg.decode() if msg else '?'}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws[:4 * shape1[0] * shape1[1] * shape1[2]].view(torch.float32).view(shape1)


def resample_to_grid(image, spacing, label=None, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192), ct_window=None):
    """The two-stage chain of the resampling scripts: zoom by spacing / target_spacing, then zoom to target_shape.
    Returns the float32 image on the target grid, and with `label` also the int64 label (both order-0 stages composed into
    one gather).  ct_window=(lo, hi) fuses preprocess_ct(lo, hi) into the last store."""
    _check_volume(image, "resample_to_grid")
    x = _image(image, "resample_to_grid")
    if len(target_shape) != 3:
        raise Mi3dError(f"resample_to_grid: target_shape needs three sides, got {target_shape}")
    if ct_window is not None and not float(ct_window[1]) > float(ct_window[0]):
        raise Mi3dError(f"resample_to_grid: empty CT window {ct_window}")
    if label is not None:
        _check_volume(label, "resample_to_grid")
        if tuple(label.shape) != tuple(image.shape):
            raise Mi3dError(f"resample_to_grid: label {tuple(label.shape)} and image {tuple(image.shape)} differ in shape")
        _check_integer(label, "resample_to_grid")            # before anything is launched
    _, shape1, _ = chain_shapes(x.shape, spacing, target_spacing, target_shape)
    target = tuple(int(n) for n in target_shape)
    stage1 = _workspace(shape1, x.device)
    _cubic(x, shape1, out=stage1)
    out = _cubic(stage1, target, ct_window=ct_window)
    if label is None:
        return out
    return out, resample_labels_to_grid(label, spacing, target_spacing, target_shape)
