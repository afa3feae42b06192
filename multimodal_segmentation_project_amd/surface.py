"""Surface distances between a predicted label map and its target on the GPU: the exact Euclidean distance transform and, from it,
the Hausdorff distance, its percentile (HD95), the average symmetric surface distance (ASSD) and the surface Dice (NSD) per class,
without the maps leaving the device.  CHAOS ranks by ASSD and the maximum symmetric surface distance, AMOS by Dice and NSD; the
reference computes overlap figures only (test_model.py:265-276), so the contract is what a user does on the host, the conventions
of monai.metrics and medpy: the surface M & ~scipy.ndimage.binary_erosion(M, generate_binary_structure(3, connectivity)) of
M = (labels == c), and distances from scipy.ndimage.distance_transform_edt(~surface, sampling=spacing).

  distance_to(mask, spacing=(1, 1, 1), squared=False)         float64 distance of every voxel to the nearest non-zero voxel of mask
  surface_mask(labels, cls, connectivity=1)                   uint8, 1 on the surface of labels == cls
  surface_distances(pred, target, classes=(1, 2, 3), ...)     SurfaceStats(counts, table, classes, percentile, tolerances)
  surface_metrics(stats)                                      per sample {class: {"hd", "hd95", "assd", "nsd", "n_pred", "n_target"}}
  signed_distance_maps(labels, classes=(1, 2, 3), ...)        float32 (..., K, D, H, W): the maps of the boundary loss

A map is (D, H, W) or (N, D, H, W), N independent samples, uint8 (segment.predict_labels' output) or int64 (a target), dense with
any strides per sample; spacing is (sd, sh, sw) in mm per voxel.  The squared distance is defined separably in float64 (g1, g2, g3
of include/mi3d.h) so that it has one value: the GPU gives exactly the minimum of those expressions, which is scipy's distance bit
for bit where every term is exact (unit spacing, (2.5, 0.75, 0.75), ...) and within rounding elsewhere.  Every output has the same
bits on every run and for every memory layout of the same maps.  Nothing here synchronises.  Kernels: csrc/surface.hip.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, orientation
from ._lib import Mi3dError, call, ptr, stream_ptr
from ._volume import _connectivity, _integer, _samples, _strides, _workspace

MAX_CLASSES, MAX_TOLERANCES = _lib.COMPONENTS_MAX_CLASSES, _lib.SURFACE_MAX_TOLERANCES
COUNT_COLUMNS, TABLE_COLUMNS = _lib.SURFACE_COUNT_COLUMNS, _lib.SURFACE_TABLE_COLUMNS

SurfaceStats = collections.namedtuple("SurfaceStats", "counts table classes percentile tolerances")
SurfaceStats.__doc__ = """surface_distances' result.  counts: int64 device tensor (N, len(classes), 10), or (len(classes), 10) for
3-D inputs; per class [surface voxels of pred, of target, then per direction (pred to target, target to pred) how many squared
distances are <= tolerance^2 for each of up to 4 tolerances].  table: float64 device tensor (..., 8); per direction [the largest
squared distance, the squared distances of rank floor((n - 1) q) and ceil((n - 1) q), the sum of the distances]; +inf, +inf,
+inf, 0 for a direction without voxels.  classes, percentile, tolerances: as given."""


def _spacing(spacing, affine, what):
    if spacing is not None and affine is not None:
        raise Mi3dError(f"{what}: give spacing or affine, not both")
    if affine is not None:
        spacing = orientation.spacing_of(affine)
    if spacing is None:
        return (1.0, 1.0, 1.0)
    try:
        s = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise Mi3dError(f"{what}: spacing {spacing!r} is not three numbers") from None
    if len(s) != 3 or not all(math.isfinite(v) and v > 0.0 for v in s):
        raise Mi3dError(f"{what}: spacing {s} is not three positive finite numbers (mm per voxel along d, h, w)")
    return s


def distance_to(mask, spacing=(1, 1, 1), squared=False):
    """The distance in mm of every voxel to the nearest non-zero voxel of `mask` (bool, uint8 or int64; (D, H, W) or (N, D, H, W)):
    float64, C-contiguous, shape of `mask`; +inf throughout a sample whose mask is empty.  Equals
    scipy.ndimage.distance_transform_edt(~mask, sampling=spacing) per sample.  squared=True returns the squared distance g3 of
    include/mi3d.h itself, which is exact; the root is taken by torch.sqrt."""
    what = "distance_to"
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    t, code, _ = _samples(mask, what)
    s = _spacing(spacing, None, what)
    _lib.require_cuda(t, what)
    nbytes = _workspace("mi3d_surface_workspace_bytes", t, what, 1)
    # everything is checked: allocate and launch
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    out = torch.empty(mask.shape, dtype=torch.float64, device=t.device)
    call("mi3d_distance_transform", ptr(t), code, *t.shape, *_strides(t), (C.c_double * 3)(*s), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out if squared else out.sqrt_()


def surface_mask(labels, cls, connectivity=1):
    """uint8, C-contiguous, shape of `labels`: 1 where a voxel of class `cls` has a neighbour (connectivity 1, 2, 3 = 6, 18, 26
    neighbours) of another value or outside the volume.  Equals M & ~scipy.ndimage.binary_erosion(M,
    scipy.ndimage.generate_binary_structure(3, connectivity)) of M = (labels == cls)."""
    what = "surface_mask"
    t, code, _ = _samples(labels, what)
    cls = _class(cls, what)
    connectivity = _connectivity(connectivity, what)
    _lib.require_cuda(t, what)
    out = torch.empty(labels.shape, dtype=torch.uint8, device=t.device)
    call("mi3d_surface_mask", ptr(t), code, *t.shape, *_strides(t), connectivity, cls, ptr(out), stream_ptr())
    return out


def _class(v, what):
    v = _integer(v, what, "class")
    if not -2 ** 31 <= v < 2 ** 31:
        raise Mi3dError(f"{what}: class {v} is not a 32-bit value")
    return v


def surface_distances(pred, target, classes=(1, 2, 3), spacing=None, affine=None, connectivity=1, percentile=95.0, tolerances_mm=(1.0,)):
    """The surface-distance table of every listed class between `pred` and `target` ((D, H, W) or (N, D, H, W), same shape, each
    uint8 or int64 with its own dense strides; a target (N, 1, D, H, W) is accepted as segment.predict_labels accepts it).  Returns
    SurfaceStats(counts, table, classes, percentile, tolerances), on the device; surface_metrics turns it into figures.  Give the
    voxel size as spacing=(sd, sh, sw) in mm or as the affine of the grid the maps live on (orientation.spacing_of); neither means
    1 mm.  The host route it replaces, per class c and direction: distance_transform_edt(~S(target == c), sampling=spacing)
    [S(pred == c)] with S the surface of surface_mask, then max, numpy.percentile(., percentile), sum and (. <= tolerance).sum().
    Every argument is checked before the first launch."""
    what = "surface_distances"
    if isinstance(target, torch.Tensor) and isinstance(pred, torch.Tensor) and target.dim() == 5 and target.shape[1] == 1 and pred.dim() == 4:
        target = target[:, 0]
    p, pcode, single = _samples(pred, what)
    t, tcode, _ = _samples(target, what)
    if pred.shape != target.shape:
        raise Mi3dError(f"{what}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    classes = _classes(classes, what)
    s = _spacing(spacing, affine, what)
    connectivity = _connectivity(connectivity, what)
    try:
        percentile, tolerances = float(percentile), tuple(float(v) for v in tolerances_mm)
    except (TypeError, ValueError):
        raise Mi3dError(f"{what}: percentile {percentile!r} and tolerances_mm {tolerances_mm!r} are numbers") from None
    if not 0.0 <= percentile <= 100.0:
        raise Mi3dError(f"{what}: percentile {percentile} is outside [0, 100]")
    if len(tolerances) > MAX_TOLERANCES:
        raise Mi3dError(f"{what}: at most {MAX_TOLERANCES} tolerances, got {len(tolerances)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in tolerances):
        raise Mi3dError(f"{what}: tolerances_mm {tolerances} are finite numbers >= 0")
    _lib.require_cuda(p, what)
    _lib.require_cuda(t, what)
    if p.device != t.device:
        raise Mi3dError(f"{what}: pred is on {p.device}, target on {t.device}")
    nc = len(classes)
    nbytes = _workspace("mi3d_surface_workspace_bytes", p, what, nc)
    # everything is checked: allocate and launch
    n = p.shape[0]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    counts = torch.empty((n, nc, COUNT_COLUMNS), dtype=torch.int64, device=p.device)
    table = torch.empty((n, nc, TABLE_COLUMNS), dtype=torch.float64, device=p.device)
    call("mi3d_surface_distances", ptr(p), pcode, *_strides(p), ptr(t), tcode, *_strides(t), *p.shape, connectivity, nc,
         (C.c_int32 * nc)(*classes), (C.c_double * 3)(*s), percentile / 100.0, len(tolerances), (C.c_double * max(len(tolerances), 1))(*tolerances),
         ptr(counts), ptr(table), ptr(ws), nbytes, stream_ptr())
    return SurfaceStats(counts[0] if single else counts, table[0] if single else table, classes, percentile, tolerances)


def _classes(classes, what):
    try:
        classes = tuple(_class(c, what) for c in classes)
    except TypeError:
        raise Mi3dError(f"{what}: classes {classes!r} is not a sequence of integers") from None
    if not 1 <= len(classes) <= MAX_CLASSES:
        raise Mi3dError(f"{what}: 1 to {MAX_CLASSES} classes can be listed, got {len(classes)}")
    if len(set(classes)) != len(classes):
        raise Mi3dError(f"{what}: a class is listed twice in {classes!r}")
    return classes


def signed_distance_maps(labels, classes=(1, 2, 3), spacing=None, affine=None, inner_offset=None):
    """The signed distance map of every listed class of a target, what metrics.boundary_loss and TrainStep(boundary_weight=...)
    multiply the probabilities with (Kervadec et al., MIDL 2019): float32 (..., K, D, H, W) for labels (D, H, W), (N, D, H, W) or
    (N, 1, D, H, W), uint8 or int64 with any dense strides per sample.  Per class, with M = (labels == c): outside M the distance in
    mm to the nearest voxel of the class, inside M minus (the distance to the nearest voxel outside it - inner_offset); an absent
    class and a class that fills its sample give an all-zero map (include/mi3d.h, mi3d_signed_distance_maps).  Off those two cases
    this is one_hot2dist's edt(~M, sampling) * ~M - (edt(M, sampling) - 1) * M when inner_offset is 1.  inner_offset=None: the
    smallest of the three spacings, which is 1 at unit spacing and at any other the largest offset with phi <= 0 inside the class
    (a literal 1 at 0.75 mm gives +0.25 there).  spacing / affine: as surface_distances.  Every argument is checked before the
    first launch; nothing synchronises; the same bits on every run and for every layout of the same map."""
    what = "signed_distance_maps"
    five = isinstance(labels, torch.Tensor) and labels.dim() == 5
    if five:
        if labels.shape[1] != 1:
            raise Mi3dError(f"{what}: labels {tuple(labels.shape)}: a 5-D map is (N, 1, D, H, W)")
        labels = labels[:, 0]
    t, code, single = _samples(labels, what)
    classes = _classes(classes, what)
    s = _spacing(spacing, affine, what)
    if inner_offset is None:
        inner_offset = min(s)
    try:
        inner_offset = float(inner_offset)
    except (TypeError, ValueError):
        raise Mi3dError(f"{what}: inner_offset {inner_offset!r} is not a number") from None
    if not (math.isfinite(inner_offset) and inner_offset >= 0.0):
        raise Mi3dError(f"{what}: inner_offset {inner_offset} is not a finite number >= 0")
    _lib.require_cuda(t, what)
    nc = len(classes)
    nbytes = _workspace("mi3d_signed_distance_workspace_bytes", t, what, nc)
    # everything is checked: allocate and launch
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    out = torch.empty((t.shape[0], nc) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    call("mi3d_signed_distance_maps", ptr(t), code, *t.shape, *_strides(t), nc, (C.c_int32 * nc)(*classes), (C.c_double * 3)(*s), inner_offset,
         ptr(out), ptr(ws), nbytes, stream_ptr())
    return out[0] if single else out


def _directed(n, table, q):
    """(max, percentile) of one direction with n > 0 voxels from its table columns: roots of the squared entries, and numpy's linear
    interpolation lo + (hi - lo) * frac between the two order statistics."""
    at = (n - 1) * q
    frac = at - math.floor(at)
    lo, hi = math.sqrt(table[1]), math.sqrt(table[2])
    return math.sqrt(table[0]), lo if lo == hi else lo + (hi - lo) * frac


def surface_metrics(stats):
    """[{class: {"hd", "hd95", "assd", "nsd", "n_pred", "n_target"}}] per sample (one dict for the stats of 3-D inputs) from a
    SurfaceStats, in float64 on the host; one host copy of the two tables, like segment.per_sample_dice_iou.  With A and B the
    distances of the two directions: hd = max(max A, max B), hd95 = max of the two percentiles (stats.percentile, 95 by default),
    assd = (sum A + sum B) / (|A| + |B|), nsd = one figure per tolerance, (#{a <= tol} + #{b <= tol}) / (|A| + |B|).  A class
    whose surface is empty in exactly one map has hd = hd95 = assd = inf and nsd = 0; in both, all four are nan."""
    what = "surface_metrics"
    if not isinstance(stats, SurfaceStats):
        raise Mi3dError(f"{what}: a SurfaceStats (the result of surface_distances) expected, got {type(stats).__name__}")
    counts, table = np.asarray(stats.counts.cpu()), np.asarray(stats.table.cpu())
    nc, nt, q = len(stats.classes), len(stats.tolerances), stats.percentile / 100.0
    if counts.ndim not in (2, 3) or counts.shape[-2:] != (nc, COUNT_COLUMNS) or table.shape != counts.shape[:-1] + (TABLE_COLUMNS,):
        raise Mi3dError(f"{what}: counts {counts.shape} and table {table.shape} do not fit {nc} classes")
    per_sample = []
    for crows, trows in zip(counts.reshape(-1, nc, COUNT_COLUMNS), table.reshape(-1, nc, TABLE_COLUMNS)):
        sample = {}
        for c, cnt, tab in zip(stats.classes, crows.tolist(), trows.tolist()):
            n_pred, n_target = cnt[0], cnt[1]
            if n_pred == 0 and n_target == 0:
                hd = hd95 = assd = math.nan
                nsd = (math.nan,) * nt
            elif n_pred == 0 or n_target == 0:
                hd = hd95 = assd = math.inf
                nsd = (0.0,) * nt
            else:
                (hd_a, p_a), (hd_b, p_b) = _directed(n_pred, tab[0:4], q), _directed(n_target, tab[4:8], q)
                hd, hd95 = max(hd_a, hd_b), max(p_a, p_b)
                assd = (tab[3] + tab[7]) / (n_pred + n_target)
                nsd = tuple((cnt[2 + k] + cnt[2 + MAX_TOLERANCES + k]) / (n_pred + n_target) for k in range(nt))
            sample[c] = {"hd": hd, "hd95": hd95, "assd": assd, "nsd": nsd, "n_pred": n_pred, "n_target": n_target}
        per_sample.append(sample)
    return per_sample[0] if counts.ndim == 2 else per_sample
