"""GPU mirror of the resampling that puts a decoded scan on the training grid: the four scipy.ndimage.zoom calls of the
reference's offline scripts (scripts/resampling/amos_ct_resample.py:56-70,93-97; the same calls in
chaos_resample.py:53,63,83,87 and resample_totalseg_ras_mri.py:57,65,92,94), and what those scripts do around them per scan:
reorient_to_ras (amos_ct_resample.py:29-36), the spacing from the reoriented affine (:51), the output affine (:77-78) and the
TotalSegmentator mask merge (resample_totalseg_ras_mri.py:77-96).  File decoding (and get_fdata's scl_slope / scl_inter
scaling) stays outside: callers pass the decoded array as it is stored, and its affine.

  zoom_output_shape(shape, factors)        scipy's output-shape rule
  axis_table(n_in, n_out, order)           float64 host tables of one axis (tap indices / weights, or nearest indices)
  zoom(volume, factors, order)             zoom(volume, factors, order=order, mode='nearest', prefilter=False), order 3 or 0
  resample_to_grid(image, spacing, ...)    the two-stage chain of the scripts (isotropic spacing, then the target shape)
  resample_labels_to_grid(label, spacing)  its label half alone: both order-0 stages composed into one gather
  reorient_to_ras(volume, affine)          the scripts' reorient_to_ras of a stored device tensor: (RAS volume, new affine)
  resample_scan(image, affine, ...)        the whole per-scan body: (image on the grid, label or None, output affine)
  merge_masks_to_grid(masks, affine, ...)  the label of resample_scan(masks=...) alone
  restore_labels(labels, affine, stored)   the way back: uint8 labels on the grid put onto the scan as stored (one order-0 gather)
  restore_labels_soft(votes, affine, stored)  the soft way back: float32 class votes on the grid zoomed linearly (order 1) onto
                                           the scan as stored and the argmax taken there, in one gather

A stored scan is any dense 3-D device tensor: a permutation of a contiguous array, such as the tensor made from nibabel's
Fortran-ordered array without a host copy; int16 / uint8 / float32 images, uint8 / int16 / int64 labels, uint8 / float32 masks.
Its orientation comes from the affine (orientation.py).  The kernels read it in place through element strides; flips go into
the tables: they are built in RAS order exactly as below and index i of a flipped axis then becomes n - 1 - i (the zoom is not
bitwise symmetric under a flip, so a table built in stored order would pick other voxels).

Everything that decides WHICH voxels are read (coordinates, floor, rounding, clamping, spline weights) is computed here on
the host in float64 exactly as scipy does it; the kernels (csrc/resample.hip) only gather and sum.
"""
import collections

import numpy as np
import torch

from . import _lib, orientation
from ._lib import Mi3dError, call, ptr, stream_ptr

# one row of a cubic table as the kernel reads it (csrc/resample.hip CubicRow, include/mi3d.h)
_ROW = np.dtype([("idx", "<i4", (4,)), ("w", "<f8", (4,))])
assert _ROW.itemsize == 48
# one row of a linear table (csrc/resample.hip LerpRow, include/mi3d.h mi3d_lerp_row)
_ROW1 = np.dtype([("idx", "<i4", (2,)), ("w", "<f8", (2,))])
assert _ROW1.itemsize == 24

TABLE_CACHE_SIZE = 256     # device tables kept (least recently used first out); one chain with labels uses at most 9
_device_tables = collections.OrderedDict()     # (n_in, order or kind, output side(s), device, flipped) -> device tensor
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


def _flipped(idx, n_in, flip):
    """The one place a flip reaches a finished index table: RAS index i of an axis stored reversed is stored index n_in - 1 - i."""
    return (int(n_in) - 1 - idx).astype(np.int32) if flip else idx


def axis_table(n_in, n_out, order, flip=False):
    """Host tables of one axis, one row per output index.
    order 0: int32 (n_out,) input index floor(c + 0.5), clamped.
    order 3: (int32 (n_out, 4) tap indices floor(c) - 1 .. floor(c) + 2, each clamped; float64 (n_out, 4) B-spline weights).
    order 1: (int32 (n_out, 2) tap indices floor(c), floor(c) + 1, each clamped; float64 (n_out, 2) weights 1 - t, t).
    flip: the axis is stored reversed: the finished indices i become n_in - 1 - i, the weights stay."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise Mi3dError(f"axis_table: sides must be positive, got {n_in} -> {n_out}")
    cc = _coords(n_in, n_out)
    if order == 0:
        return _flipped(np.clip(np.floor(cc + 0.5), 0, n_in - 1).astype(np.int32), n_in, flip)
    if order not in (1, 3):
        raise Mi3dError(f"axis_table: order {order} is not supported (3 = cubic B-spline, 1 = linear, 0 = nearest)")
    f = np.floor(cc)
    t = cc - f
    if order == 1:
        idx = np.clip(f[:, None] + np.arange(0.0, 2.0)[None, :], 0, n_in - 1).astype(np.int32)
        return _flipped(idx, n_in, flip), np.stack([1.0 - t, t], axis=1)
    idx = np.clip(f[:, None] + np.arange(-1.0, 3.0)[None, :], 0, n_in - 1).astype(np.int32)
    w = np.stack([(1.0 - t) ** 3 / 6.0,
                  (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
                  (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0,
                  t ** 3 / 6.0], axis=1)
    return _flipped(idx, n_in, flip), w


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


def cubic_rows(n_in, n_out, flip=False):
    """The order-3 table of one axis in the kernel's row format."""
    rows = np.zeros(int(n_out), dtype=_ROW)
    rows["idx"], rows["w"] = axis_table(n_in, n_out, 3, flip)
    return rows


def linear_rows(n_in, n_out, flip=False):
    """The order-1 table of one axis in the kernel's row format."""
    rows = np.zeros(int(n_out), dtype=_ROW1)
    rows["idx"], rows["w"] = axis_table(n_in, n_out, 1, flip)
    return rows


def composed_index_table(n_in, n_mid, n_out, flip=False):
    """Two order-0 zooms along one axis as ONE gather: table1[table2]; both built in RAS order, the result remapped for a flip."""
    return _flipped(compose_index_tables(axis_table(n_in, n_mid, 0), axis_table(n_mid, n_out, 0)), n_in, flip)


def _host_table(n_in, sides, order, flip):
    if order == 3:
        return cubic_rows(n_in, *sides, flip)
    if order == "restore":
        return _restore_table(n_in, *sides, flip)
    if order == "restore1":
        return _restore_table(n_in, *sides, flip, linear_rows)
    return composed_index_table(n_in, *sides, flip) if len(sides) == 2 else axis_table(n_in, *sides, 0, flip)


def _device_table(n_in, n_out, order, device, flip=False):
    """The device table of one axis, through the cache.  order 3: cubic rows; order 0: nearest indices, or for n_out =
    (n_mid, n_out) the composed ones; order "restore": restore_labels' table from a grid of n_in onto n_out; "restore1":
    restore_labels_soft's linear rows."""
    sides = n_out if isinstance(n_out, tuple) else (int(n_out),)
    return _cached((int(n_in), order, *sides, device, bool(flip)), lambda: _host_table(n_in, sides, order, flip), device)


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


_RasView = collections.namedtuple("_RasView", "shape strides flips device")


def _ras(volume):
    """A contiguous RAS tensor presented as a _Stored one, for the launch wrappers: its sides, their dense strides, no flips."""
    _, h, w = volume.shape
    return _RasView(volume.shape, (h * w, w, 1), (False, False, False), volume.device)


def _gather(entry, source, code, src, out_shape, dtype, tabs, tail=(), out=None):
    """The one launch form of the cubic, nearest and merge entries: source of dtype `code` seen through `src` (a _Stored, or a
    contiguous tensor presented as one), the output and its three tables with their row counts."""
    if out is None:
        out = torch.empty(out_shape, dtype=dtype, device=src.device)
    call(entry, source, code, *src.strides, ptr(out), *src.shape, *out_shape, ptr(tabs[0]), out_shape[0], ptr(tabs[1]), out_shape[1],
         ptr(tabs[2]), out_shape[2], *tail, stream_ptr())
    return out


def _cubic(x, src, code, out_shape, out=None, ct_window=None):
    tabs = [_device_table(n, m, 3, src.device, f) for n, m, f in zip(src.shape, out_shape, src.flips)]
    lo, hi = (float(ct_window[0]), float(ct_window[1])) if ct_window is not None else (0.0, 1.0)
    return _gather("mi3d_zoom3_cubic_src", ptr(x), code, src, out_shape, torch.float32, tabs, (int(ct_window is not None), lo, hi), out)


def _index_tables(src, shapes):
    """Order-0 tables onto shapes[-1]; two shapes (stage 1, target) give both stages composed into one gather."""
    return [_device_table(n, sides, 0, src.device, f) for n, sides, f in zip(src.shape, zip(*shapes), src.flips)]


def _nearest(x, src, code, *shapes):
    return _gather("mi3d_zoom3_nearest_src", ptr(x), code, src, shapes[-1], torch.int64, _index_tables(src, shapes))


def _merge(tensors, values, code, src, *shapes):
    m = _lib.MaskList()
    m.n = len(tensors)
    for k, (t, v) in enumerate(zip(tensors, values)):
        m.mask[k], m.value[k] = ptr(t), v
    return _gather("mi3d_merge_masks3", m, code, src, shapes[-1], torch.int64, _index_tables(src, shapes))


def zoom(volume, factors, order=3):
    """scipy.ndimage.zoom(volume, factors, order=order, mode='nearest', prefilter=False) of one 3-D device tensor.
    order 3: floating input -> float32; order 0: integer input -> int64."""
    if order not in (0, 3):
        raise Mi3dError(f"zoom: order {order} is not supported (3 = cubic B-spline, 0 = nearest)")
    _check_volume(volume, "zoom")
    x = _image(volume, "zoom") if order == 3 else _labels(volume, "zoom")
    out_shape = _check_out_shape(zoom_output_shape(x.shape, factors), "zoom")
    if order == 3:
        return _cubic(x, _ras(x), _lib.SRC_F32, out_shape)
    return _nearest(x, _ras(x), _lib.SRC_I64, out_shape)


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
    return _nearest(lab, _ras(lab), _lib.SRC_I64, shape1, tuple(int(n) for n in target_shape))


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
    what = "resample_to_grid"
    _check_volume(image, what)
    x = _image(image, what)
    target = _check_chain(what, target_shape, ct_window, image, label)
    if label is not None:
        _check_integer(label, what)                          # before anything is launched
    _, shape1, _ = chain_shapes(x.shape, spacing, target_spacing, target_shape)
    out = _cubic_chain(x, _ras(x), _lib.SRC_F32, _workspace(shape1, x.device), target, ct_window)
    if label is None:
        return out
    return out, resample_labels_to_grid(label, spacing, target_spacing, target_shape)


def _check_chain(what, target_shape, ct_window=None, image=None, label=None):
    """What resample_to_grid and resample_scan check alike; the target shape as a tuple of ints."""
    if len(target_shape) != 3:
        raise Mi3dError(f"{what}: target_shape needs three sides, got {target_shape}")
    if ct_window is not None and not float(ct_window[1]) > float(ct_window[0]):
        raise Mi3dError(f"{what}: empty CT window {ct_window}")
    if label is not None:
        _check_volume(label, what)
        if tuple(label.shape) != tuple(image.shape):
            raise Mi3dError(f"{what}: label {tuple(label.shape)} and image {tuple(image.shape)} differ in shape")
    return tuple(int(n) for n in target_shape)


def _cubic_chain(x, src, code, stage, target, ct_window):
    """Both cubic stages: x seen through src onto the stage-1 workspace, that onto the target."""
    _cubic(x, src, code, tuple(stage.shape), out=stage)
    return _cubic(stage, _ras(stage), _lib.SRC_F32, target, ct_window=ct_window)


# ---- scans as stored ----------------------------------------------------------------------------------------------------------
_IMAGE_DTYPES = {torch.uint8: _lib.SRC_U8, torch.int16: _lib.SRC_I16, torch.float32: _lib.SRC_F32}
_LABEL_DTYPES = {torch.uint8: _lib.SRC_U8, torch.int16: _lib.SRC_I16, torch.int64: _lib.SRC_I64}
_MASK_DTYPES = {torch.uint8: _lib.SRC_U8, torch.float32: _lib.SRC_F32}
MAX_MASKS = _lib.MAX_MASKS

# Stage 1 of resample_scan by the RAS axis (0 = D, 1 = H, 2 = W) that is fastest in memory: "fused" reads the stored scan
# inside the cubic kernel (mi3d_zoom3_cubic_src), "reorient" makes the float32 RAS copy (mi3d_reorient3) and runs the contiguous
# kernel on it.  Both give the same bits, so the choice is invisible.  tools/time_resample.py has the rows that decide it per class;
# they have not been measured yet, so the defaults are provisional: "reorient" where W is not fastest in
# memory (a coalesced copy plus the measured contiguous kernel bounds the cost; fused, every tap of a lane is another cache
# line), "fused" where it is (the same access pattern as the contiguous kernel, without the float32 copy).
STAGE1_FORMS = ("fused", "reorient")
STAGE1_DEFAULT = {0: "reorient", 1: "reorient", 2: "fused"}


class _Stored:
    """A stored tensor seen in RAS order: sides, element strides and flips of the RAS axes, and the reoriented affine."""

    def __init__(self, volume, affine, what):
        _check_volume(volume, what)
        self._set_layout(tuple(volume.shape), tuple(volume.stride()), affine, what)
        self.device = volume.device

    @classmethod
    def of_layout(cls, shape, strides, affine, what):
        """The same view of a dense (shape, strides) layout that need not exist yet (restore_labels' destination)."""
        self = cls.__new__(cls)
        self._set_layout(tuple(int(n) for n in shape), tuple(int(s) for s in strides), affine, what)
        self.device = None
        return self

    def _set_layout(self, shape, strides, affine, what):
        if len(shape) != 3 or len(strides) != 3 or min(shape) < 1:
            raise Mi3dError(f"{what}: a 3-D layout without an empty axis is expected, got shape {shape} strides {strides}")
        orientation.check_dense(shape, strides, what)
        amap = orientation.axis_map(affine, shape, strides)
        self.shape = tuple(n for n, _, _ in amap)
        self.strides = tuple(max(int(s), 1) if n > 1 else 1 for n, s, _ in amap)
        self.flips = tuple(f and n > 1 for n, _, f in amap)
        self.affine = orientation.reoriented_affine(affine, shape)
        self.layout = (shape, tuple(s for n, s in zip(shape, strides) if n > 1))
        # which RAS axis is fastest in memory (the one with stride 1 and more than one element; W where there is none)
        self.fastest = next((a for a in (2, 1, 0) if self.shape[a] > 1 and self.strides[a] == 1), 2)

    @property
    def identity(self):
        d, h, w = self.shape
        return not any(self.flips) and all(n == 1 or s == c for n, s, c in zip(self.shape, self.strides, (h * w, w, 1)))

    def ras_view(self, volume):
        """The volume itself where its axes are the RAS axes, else the view of its memory in RAS order (no flips: a view
        cannot hold one).  Contiguous where `identity` holds, e.g. for an F-ordered array stored with its axes reversed."""
        if tuple(volume.shape) == self.shape and all(n == 1 or s == t for n, s, t in zip(self.shape, self.strides, volume.stride())):
            return volume
        return volume.as_strided(self.shape, self.strides, volume.storage_offset())

    @property
    def flip_mask(self):
        return sum(1 << a for a in range(3) if self.flips[a])


def _check_dtype(volume, table, what, kind):
    code = table.get(volume.dtype)
    if code is None:
        raise Mi3dError(f"{what}: a stored {kind} is {' / '.join(str(d).replace('torch.', '') for d in table)}, got {volume.dtype}")
    return code


def _check_same_layout(other, image, src, what, kind):
    _check_volume(other, what)
    if other.device != image.device:
        raise Mi3dError(f"{what}: the {kind} is on {other.device}, the image on {image.device}")
    layout = (tuple(other.shape), tuple(s for n, s in zip(other.shape, other.stride()) if n > 1))
    if layout != src.layout:
        raise Mi3dError(f"{what}: the {kind} (shape {tuple(other.shape)}, strides {other.stride()}) is not laid out as the image "
                        f"(shape {tuple(image.shape)}, strides {image.stride()})")


def _reorient(volume, src, code, as_label):
    """The contiguous RAS copy of a stored volume; the volume itself (seen with the RAS axes) where its memory already is that."""
    if src.identity and volume.dtype == (torch.int64 if as_label else torch.float32):
        return src.ras_view(volume)
    out = torch.empty(src.shape, dtype=torch.int64 if as_label else torch.float32, device=volume.device)
    call("mi3d_reorient3", ptr(volume), code, ptr(out), int(as_label), *src.shape, *src.strides, src.flip_mask, stream_ptr())
    return out


def reorient_to_ras(volume, affine, as_label=None):
    """reorient_to_ras of the scripts (amos_ct_resample.py:29-36) for a stored device tensor: (contiguous RAS volume, affine of
    that volume as host float64).  Images (uint8 / int16 / float32) come back as float32, labels (uint8 / int16 / int64) as int64;
    as_label picks the kind where the dtype allows both (default: int64 is a label, everything else an image).  A volume
    whose memory already is contiguous RAS of the output dtype is returned as it is, or as the view of it with the RAS axes."""
    what = "reorient_to_ras"
    src = _Stored(volume, affine, what)
    if as_label is None:
        as_label = volume.dtype == torch.int64
    code = _check_dtype(volume, _LABEL_DTYPES if as_label else _IMAGE_DTYPES, what, "label" if as_label else "image")
    return _reorient(volume, src, code, as_label), src.affine


def _check_masks(masks, what):
    """[(tensor, value), ...] -> (tensors, values, dtype code); all of one layout, dtype and device."""
    masks = list(masks)
    if len(masks) > MAX_MASKS:
        raise Mi3dError(f"{what}: {len(masks)} masks, at most {MAX_MASKS} are merged in one call")
    tensors, values = [], []
    for k, entry in enumerate(masks):
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise Mi3dError(f"{what}: masks is a list of (tensor, value) pairs; entry {k} is not")
        t, v = entry
        _check_volume(t, what)
        if int(v) != v or not -2 ** 63 <= int(v) < 2 ** 63:
            raise Mi3dError(f"{what}: the value of mask {k} is not an int64: {v!r}")
        tensors.append(t)
        values.append(int(v))
    code = _lib.SRC_U8
    for k, t in enumerate(tensors):
        code = _check_dtype(t, _MASK_DTYPES, what, "mask")
        if t.dtype != tensors[0].dtype:
            raise Mi3dError(f"{what}: mask {k} is {t.dtype}, mask 0 is {tensors[0].dtype}")
    return tensors, values, code


def _out_affine(src, target_spacing):
    out = src.affine.copy()
    out[:3, :3] = np.diag(np.asarray(target_spacing, dtype=np.float64))      # amos_ct_resample.py:77-78
    return out


def merge_masks_to_grid(masks, affine, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192)):
    """The label of resample_scan(masks=...) alone: per-organ masks [(tensor, value), ...] as stored, all with this affine,
    merged on the target grid in one gather (resample_totalseg_ras_mri.py:77-96).  Later entries win.  An empty list gives
    zeros on the current device (no mask file was found)."""
    what = "merge_masks_to_grid"
    tensors, values, code = _check_masks(masks, what)
    target = _check_chain(what, target_shape)
    if not tensors:
        orientation.io_orientation(affine)
        return torch.zeros(target, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    src = _Stored(tensors[0], affine, what)
    for k, t in enumerate(tensors[1:], 1):
        _check_same_layout(t, tensors[0], src, what, f"mask {k}")
    _, shape1, _ = chain_shapes(src.shape, orientation.spacing_of(src.affine), target_spacing, target)
    return _merge(tensors, values, code, src, shape1, target)


def resample_scan(image, affine, label=None, masks=None, target_spacing=(1.0, 1.0, 1.0), target_shape=(192, 192, 192),
                  ct_window=None, stage1=None):
    """The per-scan body of the resampling scripts for a decoded scan AS STORED and its 4x4 affine: orientation from the
    affine, spacing from the reoriented affine (amos_ct_resample.py:51), the two-stage cubic chain with stage 1 reading the
    stored tensor in place, and the label either from `label` (one composed order-0 gather) or from masks=[(tensor, value),
    ...] (the TotalSegmentator merge, one gather for up to 8 masks).  Returns (float32 image, int64 label or None, output
    affine): the reoriented affine with diag(target_spacing) as its 3x3 part (:77-78), host float64.
    The bits are those of resample_to_grid on the host-reoriented float32 copy.  stage1 picks the form of stage 1
    (STAGE1_FORMS; None = STAGE1_DEFAULT of the scan's memory-fastest axis)."""
    what = "resample_scan"
    src = _Stored(image, affine, what)
    code = _check_dtype(image, _IMAGE_DTYPES, what, "image")
    target = _check_chain(what, target_shape, ct_window, image, label)
    if stage1 is not None and stage1 not in STAGE1_FORMS:
        raise Mi3dError(f"{what}: stage1 is one of {STAGE1_FORMS} or None, got {stage1!r}")
    if label is not None and masks is not None:
        raise Mi3dError(f"{what}: pass label or masks, not both")
    if label is not None:
        _check_same_layout(label, image, src, what, "label")
        label_code = _check_dtype(label, _LABEL_DTYPES, what, "label")
    if masks is not None:
        tensors, values, mask_code = _check_masks(masks, what)
        for k, t in enumerate(tensors):
            _check_same_layout(t, image, src, what, f"mask {k}")
    _, shape1, _ = chain_shapes(src.shape, orientation.spacing_of(src.affine), target_spacing, target)
    # everything is checked: launch
    stage = _workspace(shape1, src.device)
    if (stage1 or STAGE1_DEFAULT[src.fastest]) == "fused":
        out = _cubic_chain(image, src, code, stage, target, ct_window)      # a contiguous float32 scan takes the contiguous kernel
    else:
        ras = _reorient(image, src, code, False)
        out = _cubic_chain(ras, _ras(ras), _lib.SRC_F32, stage, target, ct_window)
    out_label = None
    if label is not None:
        out_label = _nearest(label, src, label_code, shape1, target)
    elif masks is not None:
        out_label = _merge(tensors, values, mask_code, src, shape1, target)
    return out, out_label, _out_affine(src, target_spacing)


# ---- labels from the grid back onto the scan as stored -------------------------------------------------------------------------
def _nearest_rows(n_grid, n_ras):
    return axis_table(n_grid, n_ras, 0)


def _restore_table(n_grid, n_ras, flip, rows=_nearest_rows):
    """Not _flipped: here the flipped axis is the OUTPUT's, so the table is read backwards and its values (grid indices, and the
    weights of linear_rows) stay."""
    t = rows(n_grid, n_ras)
    return np.ascontiguousarray(t[::-1]) if flip else t


def restore_tables(grid_shape, affine, shape, strides, what="restore_labels"):
    """Host side of restore_labels for a dense destination layout (shape, strides) with this affine: (RAS sides, element strides
    of the RAS axes in the destination, three int32 tables).  Table a holds, per destination index along RAS axis a, the grid
    index it takes: axis_table(n_grid, n_ras, 0), built in RAS order and read backwards where the axis is stored flipped
    (stored index i is RAS index n - 1 - i).  out[sum_a i_a * stride_a] = grid[t_d[i_d], t_h[i_h], t_w[i_w]]."""
    if len(grid_shape) != 3 or min(grid_shape) < 1:
        raise Mi3dError(f"{what}: a 3-D grid without an empty axis is expected, got {tuple(grid_shape)}")
    dst = _Stored.of_layout(shape, strides, affine, what)
    return dst.shape, dst.strides, [_restore_table(g, n, f) for g, n, f in zip(grid_shape, dst.shape, dst.flips)]


def _stored_layout(stored, source, what, kind):
    """(shape, strides) of `stored`: the stored tensor (which must be on the device of `source`, the `kind` on the grid) or a pair."""
    if isinstance(stored, torch.Tensor):
        if stored.device != source.device:
            raise Mi3dError(f"{what}: the stored scan is on {stored.device}, the {kind} on {source.device}")
        return tuple(stored.shape), tuple(stored.stride())
    try:
        shape, strides = (tuple(int(v) for v in part) for part in stored)
    except (TypeError, ValueError):
        raise Mi3dError(f"{what}: `stored` is the stored tensor or a (shape, strides) pair, got {stored!r}") from None
    return shape, strides


def restore_labels(labels, affine, stored):
    """A uint8 (Dg, Hg, Wg) label map on the training grid put back onto the scan as stored: scipy.ndimage.zoom(labels,
    ras_shape / grid_shape, order=0, mode='nearest', prefilter=False) (one zoom: the intermediate shape of the inbound chain
    carries no information for an order-0 gather), then the inverse of reorient_to_ras, as ONE gather that writes the stored
    layout in memory order.  `stored` is the stored scan tensor (only its shape, strides and device are read) or a (shape,
    strides) pair of a dense layout; `affine` is the stored scan's.  Returns a uint8 tensor with that shape and those strides,
    ready for a NIfTI writer next to the scan's own affine."""
    what = "restore_labels"
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or min(labels.shape) < 1:
        raise Mi3dError(f"{what}: one 3-D label map (Dg, Hg, Wg) expected, got {tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype != torch.uint8:
        raise Mi3dError(f"{what}: the label map is uint8 (segment.predict_labels' output), got {labels.dtype}")
    shape, strides = _stored_layout(stored, labels, what, "labels")
    dst = _Stored.of_layout(shape, strides, affine, what)
    _lib.require_cuda(labels, what)
    # everything is checked: launch
    grid = labels.contiguous()
    dev = grid.device
    tabs = [_device_table(g, n, "restore", dev, f) for g, n, f in zip(grid.shape, dst.shape, dst.flips)]
    out = torch.empty_strided(shape, strides, dtype=torch.uint8, device=dev)
    call("mi3d_restore_labels3", ptr(grid), *grid.shape, ptr(out), *dst.shape, *dst.strides, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]),
         stream_ptr())
    return out


MIN_CLASSES, MAX_CLASSES = 2, 8      # what the head kernels and mi3d_restore_votes3 accept


def restore_labels_soft(votes, affine, stored, confidence=False):
    """A float32 (C, Dg, Hg, Wg) vote volume on the training grid (segment.predict_labels_ensemble(..., votes=True); a leading
    batch axis of 1 is dropped) put back onto the scan as stored: per class scipy.ndimage.zoom(votes[k], ras_shape / grid_shape,
    order=1, mode='nearest', prefilter=False), the first maximum over the classes on the DESTINATION grid, then the inverse of
    reorient_to_ras, as ONE gather that writes the stored layout in memory order.  The interpolation is nested, W innermost,
    then H, then D, in float64 with every product and sum rounded on its own (include/mi3d.h mi3d_restore_votes3), so the bits
    do not depend on the orientation or the layout.  `stored` and `affine` as for restore_labels.  Returns a uint8 tensor with the
    stored shape and strides; with confidence=True also the float32 tensor of that layout holding the winning class's
    interpolated vote.  Every check runs before the first launch."""
    what = "restore_labels_soft"
    if isinstance(votes, torch.Tensor) and votes.dim() == 5 and votes.shape[0] == 1:
        votes = votes[0]
    if not isinstance(votes, torch.Tensor) or votes.dim() != 4 or min(votes.shape) < 1:
        raise Mi3dError(f"{what}: one 4-D vote volume (C, Dg, Hg, Wg) expected, got {tuple(getattr(votes, 'shape', ()))}")
    if votes.dtype != torch.float32:
        raise Mi3dError(f"{what}: the vote volume is float32 (segment.predict_labels_ensemble's votes), got {votes.dtype}")
    if not MIN_CLASSES <= votes.shape[0] <= MAX_CLASSES:
        raise Mi3dError(f"{what}: {votes.shape[0]} classes, {MIN_CLASSES} to {MAX_CLASSES} are supported (the range of the head kernels)")
    shape, strides = _stored_layout(stored, votes, what, "votes")
    dst = _Stored.of_layout(shape, strides, affine, what)
    _lib.require_cuda(votes, what)
    # everything is checked: launch
    vol = votes.contiguous()
    dev = vol.device
    tabs = [_device_table(g, n, "restore1", dev, f) for g, n, f in zip(vol.shape[1:], dst.shape, dst.flips)]
    out = torch.empty_strided(shape, strides, dtype=torch.uint8, device=dev)
    conf = torch.empty_strided(shape, strides, dtype=torch.float32, device=dev) if confidence else None
    call("mi3d_restore_votes3", ptr(vol), *vol.shape, ptr(out), ptr(conf), *dst.shape, *dst.strides, ptr(tabs[0]), ptr(tabs[1]),
         ptr(tabs[2]), stream_ptr())
    return (out, conf) if confidence else out
