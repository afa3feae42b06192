"""Connected components of a label map on the GPU: drop the spurious islands of a predicted map (keep 1 spleen, 1 liver, 2 kidneys),
fill the enclosed holes the organs are left with, and read off the organ volumes, without the map leaving the device.  The reference writes its predictions out uncleaned
(test_model.py:299-309); the contract is what a user does with them on the host: scipy.ndimage.label(labels == c,
scipy.ndimage.generate_binary_structure(3, connectivity)) per class, np.bincount of the ids, np.isin of the kept ones.

  component_roots(labels, connectivity=1, classes=None)      int32 roots, C-contiguous, -1 off-component
  keep_largest(labels, keep=ORGANS, connectivity=1, ...)     Cleaned(labels, stats, status, classes)
  fill_holes(labels, classes=(1, 2, 3), connectivity=1, ...)  Filled(labels, stats, summary, status, classes)
  organ_volumes_ml(stats, affine)                            per sample {class: (ml_before, ml_kept)}

A volume is (D, H, W) or (N, D, H, W), N independent samples, uint8 (segment.predict_labels' output) or int64 (a target), dense
with any strides per sample.  Two voxels are in one component iff they are in the same sample, carry the same selected value
(1..255; 0 and int64 values outside 0..255 never are) and are joined by a path of neighbours of that value; connectivity 1, 2, 3
is 6, 18, 26 neighbours.  The ROOT of a component is the C-order index d * H * W + h * W + w of its first voxel within the sample,
so the labelling is canonical; components of one (sample, class) are ranked by (size descending, root ascending).  Every output
has the same bits on every run.  Nothing here synchronises.  Kernels: csrc/components.hip.

fill_holes is the second half of the usual clean-up pair (keep the largest components, fill the holes) and goes directly behind
keep_largest, which turns a wrong-class island inside an organ into a pocket of 0 inside it.  A BACKGROUND COMPONENT is a component
of labels == 0 of one sample under generate_binary_structure(3, connectivity); its RING is every position that is not in it but
is such a neighbour of one of its voxels, positions outside the volume included; it is ENCLOSED iff no ring position lies outside
the volume (none of its voxels lies on a face of the sample).  An enclosed component is filled with v iff every ring voxel carries
the same value v, v is a listed class and the component has at most max_size voxels; every other voxel is copied.  The host
route: scipy.ndimage.label(labels == 0, structure), per component binary_dilation(comp, structure) & ~comp on a copy padded by one
voxel and np.unique on that ring; on a map with one class c it is scipy.ndimage.binary_fill_holes(labels == c, structure) * c.
monai.transforms.FillHoles states the same idea (enclosed background, one enclosing label, applied_labels); this contract is not
pinned against MONAI.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError, call, ptr, stream_ptr
from ._volume import _connectivity, _integer, _samples, _strides, _workspace

ORGANS = {1: 1, 2: 1, 3: 2}          # spleen, liver, kidneys (the classes of test_model.py:265): how many of each a body has
MAX_CLASSES, MAX_KEEP = _lib.COMPONENTS_MAX_CLASSES, _lib.COMPONENTS_MAX_KEEP
STATS_COLUMNS = 3 + 2 * MAX_KEEP      # n_components, voxels_before, voxels_kept, MAX_KEEP sizes, MAX_KEEP roots

Cleaned = collections.namedtuple("Cleaned", "labels stats status classes")
Cleaned.__doc__ = """keep_largest's result.  labels: the cleaned map (dtype, shape and strides of the input).  stats: int64 device
tensor (N, len(classes), 19), or (len(classes), 19) for a 3-D input; per class [n_components, voxels_before, voxels_kept, the
sizes of the kept components in rank order (0 where fewer), their roots (-1 where fewer)].  status: int32 device scalar, 0 unless
a kernel gave up (then labels and stats mean nothing).  classes: the listed class values, one per stats row."""


Filled = collections.namedtuple("Filled", "labels stats summary status classes")
Filled.__doc__ = """fill_holes' result.  labels: the filled map (dtype, shape and strides of the input).  stats: int64 device tensor
(N, len(classes), 2), or (len(classes), 2) for a 3-D input; per class [holes filled, voxels filled].  summary: int64 device tensor
(N, 4) or (4,): [enclosed background components, filled, mixed (a ring of two or more values), skipped (a single ring value that is
unlisted or outside 1..255, or a size above max_size)]; enclosed = filled + mixed + skipped.  status: int32 device scalar, 0 unless
a kernel gave up (then the rest means nothing).  classes: the listed class values, one per stats row."""


def component_roots(labels, connectivity=1, classes=None):
    """The root of every voxel's component as int32, C-contiguous, shape of `labels`; -1 where the voxel's value is not selected.
    classes: the selected values (any iterable of integers in 1..255), None for every value 1..255.  At the voxels of class c this
    is np.unique(ids, return_index=True)[1][ids - 1] of ids = scipy.ndimage.label(labels == c, structure)[0].  The same for every
    memory layout of the same logical volume.  The status word is not returned: keep_largest hands it out."""
    what = "component_roots"
    t, code, _ = _samples(labels, what)
    connectivity = _connectivity(connectivity, what)
    select = (C.c_uint8 * 256)()
    for v in range(1, 256) if classes is None else classes:
        v = _integer(v, what, "class")
        if not 1 <= v <= 255:
            raise Mi3dError(f"{what}: class {v} cannot be selected: values 1..255 can")
        select[v] = 1
    _lib.require_cuda(t, what)
    nbytes = _workspace("mi3d_components_workspace_bytes", t, what)
    # everything is checked: allocate and launch
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    status = torch.empty((), dtype=torch.int32, device=t.device)
    roots = torch.empty(labels.shape, dtype=torch.int32, device=t.device)
    call("mi3d_component_roots", ptr(t), code, *t.shape, *_strides(t), connectivity, select, ptr(roots), ptr(status), ptr(ws), nbytes,
         stream_ptr())
    return roots


def _keep_table(keep, what):
    if not isinstance(keep, dict) or not keep:
        raise Mi3dError(f"{what}: keep is a non-empty dict {{class: how many components to keep}}, got {keep!r}")
    if len(keep) > MAX_CLASSES:
        raise Mi3dError(f"{what}: at most {MAX_CLASSES} classes can be listed, got {len(keep)}")
    table = sorted((_integer(c, what, "class"), _integer(k, what, "keep count")) for c, k in keep.items())
    for c, k in table:
        if not 1 <= c <= 255:
            raise Mi3dError(f"{what}: class {c} cannot be listed: values 1..255 can")
        if not 1 <= k <= MAX_KEEP:
            raise Mi3dError(f"{what}: class {c} keeps {k} components; 1..{MAX_KEEP} expected")
    if len({c for c, _ in table}) != len(table):
        raise Mi3dError(f"{what}: a class is listed twice in {keep!r}")
    return table


def keep_largest(labels, keep=ORGANS, connectivity=1, min_size=1, fill=0):
    """Keep, of every listed class, its keep[class] largest components (of at least min_size voxels); every other voxel of a listed
    class becomes `fill`; voxels of other values (0, unlisted classes, int64 values outside 0..255) are copied.  Returns
    Cleaned(labels, stats, status, classes); classes are keep's keys in ascending order.  The host route it replaces: per class
    ids, n = scipy.ndimage.label(labels == c, structure); sizes = np.bincount(ids.ravel())[1:]; the keep[c] first of a stable
    argsort of -sizes; labels[(labels == c) & ~np.isin(ids, kept + 1)] = fill.  Every argument is checked before the first launch."""
    what = "keep_largest"
    t, code, single = _samples(labels, what)
    connectivity = _connectivity(connectivity, what)
    table = _keep_table(keep, what)
    min_size, fill = _integer(min_size, what, "min_size"), _integer(fill, what, "fill")
    if min_size < 1:
        raise Mi3dError(f"{what}: min_size {min_size} is below 1")
    if not 0 <= fill <= 255:
        raise Mi3dError(f"{what}: fill {fill} is outside 0..255")
    _lib.require_cuda(t, what)
    nbytes = _workspace("mi3d_components_workspace_bytes", t, what)
    # everything is checked: allocate and launch
    n, nc = t.shape[0], len(table)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    status = torch.empty((), dtype=torch.int32, device=t.device)
    stats = torch.empty((n, nc, STATS_COLUMNS), dtype=torch.int64, device=t.device)
    out = torch.empty_strided(labels.shape, labels.stride(), dtype=labels.dtype, device=t.device)
    values, counts = (C.c_int32 * nc)(*[c for c, _ in table]), (C.c_int32 * nc)(*[k for _, k in table])
    call("mi3d_keep_components", ptr(t), code, *t.shape, *_strides(t), connectivity, nc, values, counts, min_size, fill, ptr(out),
         ptr(stats), ptr(status), ptr(ws), nbytes, stream_ptr())
    return Cleaned(out, stats[0] if single else stats, status, tuple(c for c, _ in table))


def _class_list(classes, what):
    try:
        table = sorted(_integer(c, what, "class") for c in classes)
    except TypeError:
        raise Mi3dError(f"{what}: classes is a non-empty iterable of class values, got {classes!r}") from None
    if not 1 <= len(table) <= MAX_CLASSES:
        raise Mi3dError(f"{what}: 1 to {MAX_CLASSES} classes can be listed, got {len(table)}")
    for c in table:
        if not 1 <= c <= 255:
            raise Mi3dError(f"{what}: class {c} cannot be listed: values 1..255 can")
    if len(set(table)) != len(table):
        raise Mi3dError(f"{what}: a class is listed twice in {classes!r}")
    return table


def fill_holes(labels, classes=(1, 2, 3), connectivity=1, max_size=None):
    """Fill every enclosed background component whose ring carries one listed class with that class (the definitions are in the
    module docstring); max_size: fill only components of at most that many voxels, None for no limit.  Every other voxel is
    copied: open components, enclosed ones with a ring of two or more values, and ones whose single ring value is unlisted or an
    int64 value outside 1..255 (all int64 values outside 0..255 count as one ring value).  Returns Filled(labels, stats, summary,
    status, classes); classes in ascending order.  Every argument is checked before the first launch."""
    what = "fill_holes"
    t, code, single = _samples(labels, what)
    connectivity = _connectivity(connectivity, what)
    table = _class_list(classes, what)
    limit = 0          # the library's "no limit"
    if max_size is not None:
        limit = _integer(max_size, what, "max_size")
        if not 1 <= limit < 2 ** 63:
            raise Mi3dError(f"{what}: max_size {limit} is outside 1..2^63 - 1 (None: no limit)")
    _lib.require_cuda(t, what)
    nbytes = _workspace("mi3d_fill_holes_workspace_bytes", t, what)
    # everything is checked: allocate and launch
    n, nc = t.shape[0], len(table)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    status = torch.empty((), dtype=torch.int32, device=t.device)
    stats = torch.empty((n, nc, 2), dtype=torch.int64, device=t.device)
    summary = torch.empty((n, 4), dtype=torch.int64, device=t.device)
    out = torch.empty_strided(labels.shape, labels.stride(), dtype=labels.dtype, device=t.device)
    call("mi3d_fill_holes", ptr(t), code, *t.shape, *_strides(t), connectivity, nc, (C.c_int32 * nc)(*table), limit, ptr(out), ptr(stats),
         ptr(summary), ptr(status), ptr(ws), nbytes, stream_ptr())
    return Filled(out, stats[0] if single else stats, summary[0] if single else summary, status, tuple(table))


def organ_volumes_ml(stats, affine, status=None, classes=None):
    """[{class: (ml_before, ml_kept)}] per sample (one dict for the stats of a 3-D input): voxels * |det(affine[:3, :3])| / 1000 in
    float64 on the host, the volume of a voxel in mm^3 from the affine of the grid the map lives on.  stats: a Cleaned record, or
    its stats table with `classes` (default: ORGANS' keys) and optionally `status`.  One host copy of the table, like
    segment.per_sample_dice_iou; raises if a given status is not 0."""
    what = "organ_volumes_ml"
    if isinstance(stats, Cleaned):
        stats, status, classes = stats.stats, stats.status, stats.classes
    classes = tuple(sorted(ORGANS)) if classes is None else tuple(classes)
    if status is not None and int(status) != 0:
        raise Mi3dError(f"{what}: the labelling gave up (status {int(status)}); its table means nothing")
    rows = np.asarray(stats.cpu() if isinstance(stats, torch.Tensor) else stats)
    if rows.ndim not in (2, 3) or rows.shape[-1] != STATS_COLUMNS or rows.shape[-2] != len(classes):
        raise Mi3dError(f"{what}: a (N, {len(classes)}, {STATS_COLUMNS}) or ({len(classes)}, {STATS_COLUMNS}) table expected for classes "
                        f"{classes}, got {rows.shape}")
    a = np.asarray(affine.cpu() if isinstance(affine, torch.Tensor) else affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise Mi3dError(f"{what}: a 4x4 affine expected, got {a.shape}")
    mm3 = abs(float(np.linalg.det(a[:3, :3])))
    per_sample = [{c: (float(r[1]) * mm3 / 1000.0, float(r[2]) * mm3 / 1000.0) for c, r in zip(classes, sample)}
                  for sample in rows.reshape(-1, *rows.shape[-2:])]
    return per_sample[0] if rows.ndim == 2 else per_sample
