"""Numpy restatement of surface.py (csrc/surface.hip) by its definitions, the case tables of its tests and their allowances.  No
scipy and no torch: the GPU tests import it.  tests/test_surface_cpu.py pins it to scipy.ndimage for every case.

  surface(labels, cls, connectivity)                      bool: voxels of labels == cls with a neighbour outside the class or the volume
  dist2(features, spacing)                                float64 g3: the squared distance to the nearest True voxel, +inf if none
  stats(pred, target, classes, spacing, ...)              (counts (.., 10) int64, table (.., 8) float64) as mi3d_surface_distances
  metrics(pred, target, classes, spacing, ...)            the dicts of surface.surface_metrics

The squared distance is defined separably, every operation an IEEE double operation rounded on its own:
  g1[d,h,w] = min over w' with F[d,h,w'] of fl((sw (w - w'))^2), +inf without one;  g2[d,h,w] = min over h' of fl(g1[d,h',w] +
  fl((sh (h - h'))^2));  g3[d,h,w] = min over d' of fl(g2[d',h,w] + fl((sd (d - d'))^2)).
Here each axis is one explicit (L, L) cost matrix added to the lines and a min: nothing clever, so nothing to get wrong.

Allowances (U = 2^-53, the unit roundoff of float64).  None on the exact spacings: there every product s k, its square and every
sum is an integer multiple of 2^-8 far below 2^53, hence exact, and all routes agree bit for bit.
  G3_RTOL     the kernel against g3 on a rounded spacing, the bound this comparison was specified with: two candidate sums, each
              of three rounded terms and two rounded adds, can differ by 3 U g3.  The kernel evaluates the very expressions above
              in the order above, so the GPU test asserts the bound and then equality as well.
  SCIPY_RTOL  sqrt(g3) against scipy.ndimage.distance_transform_edt on a rounded spacing.  scipy finds the nearest feature c* with
              its Voronoi transform and returns sqrt(fl(fl(td + th) + tw)) of the same rounded terms t = fl(fl(s k)^2), added from
              the other end.  For one candidate with exact term sum T, two rounded adds in any order give T (1 + e), |e| <= 2 U
              (first order), so the two orders differ by 4 U T.  The candidates may differ too: a term is (s k)^2 (1 + e'),
              |e'| <= 3 U, so the candidate with the smallest true distance has a T within 6 U of the smallest T.  Together
              10 U on g3, 5 U on its root, plus one rounding (U) of each of the two roots: 7 U, and 8 U covers the second-order terms.
  sum_allowance(n, total, rounded)
              the kernel's sum of n roots against math.fsum of numpy's: any order of n - 1 rounded adds is within
              (n - 1) U total (1 + (n - 1) U + ...) of the exact sum, and each root may be one spacing (2 U relative) from
              numpy's correctly rounded one: (n + 1) U total, written with the 1 / (1 - n U) that bounds the higher-order terms.
              On a rounded spacing each g3 may differ by G3_RTOL, its root by half that: + 1.5 U total.
"""
import functools
import itertools
import math

import numpy as np

U = 2.0 ** -53
G3_RTOL = 3 * U
SCIPY_RTOL = 8 * U
MAX_TOLERANCES = 4
COUNT_COLUMNS, TABLE_COLUMNS = 2 + 2 * MAX_TOLERANCES, 8
EXACT_SPACINGS = ((1.0, 1.0, 1.0), (2.5, 0.75, 0.75), (3.0, 1.0, 1.5))
ROUNDED_SPACING = (5.0, 0.782, 0.782)
SPACINGS = EXACT_SPACINGS + (ROUNDED_SPACING,)


def sum_allowance(n, total, rounded=False):
    if n == 0 or not math.isfinite(total):
        return 0.0
    k = n + 1 + (1.5 if rounded else 0.0)
    return k * U * total / (1.0 - k * U)


# ---- the definitions --------------------------------------------------------------------------------------------------------------
def offsets(connectivity):
    """generate_binary_structure(3, connectivity) without its centre: offsets with at most `connectivity` non-zero coordinates."""
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= connectivity]


def _surface3(lab, cls, connectivity):
    m = lab == cls
    padded = np.pad(m, 1, constant_values=False)          # border_value = 0: outside the volume is outside the class
    d, h, w = m.shape
    inner = m.copy()
    for od, oh, ow in offsets(connectivity):
        inner &= padded[1 + od:1 + od + d, 1 + oh:1 + oh + h, 1 + ow:1 + ow + w]
    return m & ~inner


def surface(labels, cls, connectivity=1):
    labels = np.asarray(labels)
    if labels.ndim == 4:
        return np.stack([_surface3(s, cls, connectivity) for s in labels])
    return _surface3(labels, cls, connectivity)


def _axis_min(g, axis, s):
    """min over x' of fl(g[x'] + fl(fl(s (x - x'))^2)) along `axis`, by the (L, L) matrix of the offset costs."""
    n = g.shape[axis]
    k = np.arange(n, dtype=np.float64)
    cost = (s * (k[:, None] - k[None, :])) ** 2          # [x', x]; the product is rounded, then its square
    lines = np.moveaxis(g, axis, -1)
    with np.errstate(invalid="ignore"):
        best = (lines[..., :, None] + cost).min(axis=-2)
    return np.moveaxis(best, -1, axis)


def _dist2_3(f, spacing):
    g = np.where(f, 0.0, np.inf)          # 0 + cost = cost, inf + cost = inf: g1 exactly as defined
    for axis in (2, 1, 0):
        g = _axis_min(g, axis, float(spacing[axis]))
    return g


def dist2(features, spacing=(1.0, 1.0, 1.0)):
    features = np.asarray(features) != 0
    if features.ndim == 4:
        return np.stack([_dist2_3(f, spacing) for f in features])
    return _dist2_3(features, spacing)


def order_statistics(values, q):
    """(value of rank floor((n - 1) q), value of rank ceil((n - 1) q), frac) of a non-empty array."""
    v = np.sort(values)
    at = (len(v) - 1) * q
    return v[math.floor(at)], v[math.ceil(at)], at - math.floor(at)


def _stats3(pred, target, classes, spacing, connectivity, percentile, tolerances):
    counts = np.zeros((len(classes), COUNT_COLUMNS), dtype=np.int64)
    table = np.zeros((len(classes), TABLE_COLUMNS), dtype=np.float64)
    q = percentile / 100.0
    for row, trow, c in zip(counts, table, classes):
        p, g = _surface3(pred, c, connectivity), _surface3(target, c, connectivity)
        row[0], row[1] = p.sum(), g.sum()
        for direction, (query, feature) in enumerate(((p, g), (g, p))):
            cols = trow[4 * direction:4 * direction + 4]
            if not query.any():
                cols[:] = (np.inf, np.inf, np.inf, 0.0)
                continue
            g3 = _dist2_3(feature, spacing)[query]
            lo, hi, _ = order_statistics(g3, q)
            cols[:] = (g3.max(), lo, hi, math.fsum(np.sqrt(g3)) if np.isfinite(g3).all() else np.inf)
            for t, tol in enumerate(tolerances):
                row[2 + MAX_TOLERANCES * direction + t] = (g3 <= tol * tol).sum()
    return counts, table


def stats(pred, target, classes=(1, 2, 3), spacing=(1.0, 1.0, 1.0), connectivity=1, percentile=95.0, tolerances=(1.0,)):
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 3:
        return _stats3(pred, target, classes, spacing, connectivity, percentile, tolerances)
    parts = [_stats3(p, t, classes, spacing, connectivity, percentile, tolerances) for p, t in zip(pred, target)]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def _metrics3(counts, table, classes, percentile, tolerances):
    out, q, nt = {}, percentile / 100.0, len(tolerances)
    for c, cnt, tab in zip(classes, counts.tolist(), table.tolist()):
        n_pred, n_target = cnt[0], cnt[1]
        if n_pred == 0 and n_target == 0:
            hd = hd95 = assd = math.nan
            nsd = (math.nan,) * nt
        elif n_pred == 0 or n_target == 0:
            hd = hd95 = assd = math.inf
            nsd = (0.0,) * nt
        else:
            hd, hd95 = 0.0, 0.0
            for n, cols in ((n_pred, tab[0:4]), (n_target, tab[4:8])):
                at = (n - 1) * q
                lo, hi = math.sqrt(cols[1]), math.sqrt(cols[2])
                hd, hd95 = max(hd, math.sqrt(cols[0])), max(hd95, lo if lo == hi else lo + (hi - lo) * (at - math.floor(at)))
            assd = (tab[3] + tab[7]) / (n_pred + n_target)
            nsd = tuple((cnt[2 + t] + cnt[2 + MAX_TOLERANCES + t]) / (n_pred + n_target) for t in range(nt))
        out[c] = {"hd": hd, "hd95": hd95, "assd": assd, "nsd": nsd, "n_pred": n_pred, "n_target": n_target}
    return out


def metrics(pred, target, classes=(1, 2, 3), spacing=(1.0, 1.0, 1.0), connectivity=1, percentile=95.0, tolerances=(1.0,)):
    counts, table = stats(pred, target, classes, spacing, connectivity, percentile, tolerances)
    if counts.ndim == 2:
        return _metrics3(counts, table, classes, percentile, tolerances)
    return [_metrics3(c, t, classes, percentile, tolerances) for c, t in zip(counts, table)]


# ---- the cases: the smallest inputs at which a kernel can go wrong ----------------------------------------------------------------
# Sides: W in {1, 17, 63, 64, 65, 130} (the wave and word seams of the w pass), D and H in {1, 2, 7, 19}.
def _points(shape, *points, dtype=np.uint8):
    a = np.zeros(shape, dtype=dtype)
    for p in points:
        a[p] = 1
    return a


def _sites(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def checkerboard(shape):
    d, h, w = np.indices(shape)
    return ((d + h + w) % 2).astype(np.uint8)


def _far_row():
    """Row (0, 0) has features at both ends only: from w = 65 the nearest is 65 voxels away on the left and 64 on the right, each in
    another 64-voxel word than the voxel; row (0, 1) has none and takes everything from its neighbour."""
    return _points((1, 2, 130), (0, 0, 0), (0, 0, 129))


def _empty_and_full():
    a = np.zeros((2, 2, 7, 65), dtype=np.uint8)
    a[1] = 1
    return a


def _int64_mask():
    a = np.zeros((7, 2, 63), dtype=np.int64)
    a[1, 0, 5], a[6, 1, 62], a[3, 1, 40] = 300, -5, 1 << 40
    return a


MASKS = {
    "corner": lambda: _points((7, 19, 65), (0, 0, 0)),
    "centre": lambda: _points((7, 7, 63), (3, 3, 31)),
    "ties": lambda: _points((2, 7, 17), (0, 3, 4), (0, 3, 12)),          # the plane w = 8 is equidistant from both
    "empty": lambda: np.zeros((2, 7, 64), dtype=np.uint8),
    "full": lambda: np.ones((2, 2, 17), dtype=np.uint8),
    "plane": lambda: _points((7, 19, 17), (3,)),
    "row": lambda: _points((7, 7, 65), (2, 5)),
    "column": lambda: _points((7, 19, 64), (4, slice(None), 9)),
    "checkerboard": lambda: checkerboard((7, 2, 65)),
    "rand002": lambda: _sites((19, 17, 130), 0.002, 11),          # long envelopes
    "rand02": lambda: _sites((19, 17, 130), 0.02, 12),            # dominated parabolas
    "rand30": lambda: _sites((19, 17, 130), 0.3, 13),             # dense
    "diagonal": lambda: _points((7, 7, 17), (3, 3, 3), (6, 0, 0), (0, 6, 0), (0, 0, 6)),          # from (0, 0, 0): 27 < 36 along any axis
    "far_row": _far_row,
    "thin_w1": lambda: _sites((19, 7, 1), 0.2, 14),
    "line_w": lambda: _sites((1, 1, 130), 0.02, 15),
    "empty_and_full": _empty_and_full,          # N = 2: nothing leaks from the full sample into the empty one
    "int64": _int64_mask,                       # 300, a negative value and one beyond 32 bits are features like any non-zero
}
LAYOUT_MASK = "rand02"          # the case run in all six axis orders


def _iid4(shape, seed, dtype=np.uint8):
    return np.random.default_rng(seed).integers(0, 4, shape).astype(dtype)


def balls(shape, centres_radii_classes, salt, seed=0):
    d, h, w = np.indices(shape)
    vol = np.zeros(shape, dtype=np.uint8)
    for (cd, ch, cw), rad, c in centres_radii_classes:
        vol[(d - cd) ** 2 + (h - ch) ** 2 + (w - cw) ** 2 <= rad * rad] = c
    rng = np.random.default_rng(seed)
    noise = rng.random(shape) < salt
    vol[noise] = rng.integers(1, 4, int(noise.sum())).astype(np.uint8)
    return vol


def _wide_values():
    """int64: classes 1 and 2 in stripes, a block of 300, a block of -2 and scattered -1: 300 and -2 are classes like any other."""
    a = np.zeros((7, 19, 66), dtype=np.int64)
    a[:, 0::2, :] = 1
    a[:, 1::2, :] = 2
    a[1:6, 3:9, 10:30] = 300
    a[2:7, 10:19, 40:66] = -2
    a[0, :, 33] = -1
    return a


# name -> (builder, classes whose surface is compared)
LABELS = {
    "iid4": (lambda: _iid4((7, 19, 65), 21), (1, 3)),
    "iid4_w1": (lambda: _iid4((19, 7, 1), 22), (2,)),
    "iid4_d1": (lambda: _iid4((1, 2, 130), 23), (1,)),
    "ball": (lambda: balls((19, 19, 63), (((9, 9, 30), 7, 2),), 0.0), (2, 1)),          # class 1 is absent
    "all_one": (lambda: np.ones((7, 7, 64), dtype=np.uint8), (1,)),                    # only the volume's edge is surface
    "one_voxel": (lambda: _points((7, 7, 17), (3, 3, 8)), (1,)),
    "wide_values": (_wide_values, (1, 300, -2, -1)),
    "two_samples": (lambda: np.stack([_iid4((2, 7, 65), 24), np.ones((2, 7, 65), dtype=np.uint8)]), (1,)),
}
LAYOUT_LABELS = "iid4"


def _ball_pair():
    """Two balls as classes 1 and 2 and 0.2 % salt of classes 1..3 (class 3 is salt alone); the prediction is the same pair shifted
    by (1, 2, 3) with other salt."""
    shape = (40, 40, 70)
    target = balls(shape, (((20, 14, 22), 9, 1), ((19, 24, 48), 12, 2)), 0.002, 1)
    pred = balls(shape, (((21, 16, 25), 9, 1), ((20, 26, 51), 12, 2)), 0.002, 2)
    return pred, target


def _absent():
    """Class 1 in both maps, 2 in pred only, 3 in target only, 4 in neither; class 5 is one voxel in each (its own surface)."""
    pred, target = np.zeros((7, 19, 65), dtype=np.uint8), np.zeros((7, 19, 65), dtype=np.uint8)
    pred[1:5, 2:9, 3:40] = 1
    target[2:6, 3:11, 5:45] = 1
    pred[5:7, 12:17, 50:64] = 2
    target[0:2, 14:19, 1:30] = 3
    pred[6, 0, 64], target[0, 18, 0] = 5, 5
    return pred, target


def _identical():
    a = _iid4((7, 7, 63), 31)
    return a, a.copy()


def _few():
    """Class 1: one surface voxel in pred (n = 1: lo == hi at every percentile) against three in target; class 2: two in pred at
    different distances from target's single one (n = 2: frac = 0.5 at the median, 0.95 at 95)."""
    pred, target = np.zeros((2, 7, 17), dtype=np.int64), np.zeros((2, 7, 17), dtype=np.int64)
    pred[0, 3, 4] = 1
    target[0, 3, 9], target[1, 0, 0], target[0, 6, 16] = 1, 1, 1
    pred[1, 1, 2], pred[1, 5, 12] = 2, 2
    target[1, 2, 4] = 2
    return pred, target


def _two_samples():
    p0, t0 = _absent()
    return np.stack([p0, t0]), np.stack([t0, t0])          # sample 1 is identical maps


PAIRS = {"ball_pair": _ball_pair, "absent": _absent, "identical": _identical, "few": _few, "two_samples": _two_samples}
TOLERANCES = (1.0, 2.0, 1.5, 0.0)
# (pair, classes, spacing, connectivity, percentile, tolerances)
METRICS = [("ball_pair", (1, 2, 3), s, 1, 95.0, TOLERANCES) for s in SPACINGS] + [
    ("ball_pair", (1, 2, 3), (1.0, 1.0, 1.0), 3, 50.0, (1.0,)),
    ("ball_pair", (2,), (3.0, 1.0, 1.5), 2, 100.0, ()),
    ("ball_pair", (3, 1), (2.5, 0.75, 0.75), 1, 0.0, (2.0, 0.0)),
    ("absent", (1, 2, 3, 4, 5), (1.0, 1.0, 1.0), 1, 95.0, TOLERANCES),
    ("absent", (5, 1), ROUNDED_SPACING, 2, 50.0, (1.0,)),
    ("identical", (1, 2, 3), (2.5, 0.75, 0.75), 1, 95.0, TOLERANCES),
    ("few", (1, 2), (1.0, 1.0, 1.0), 1, 95.0, (1.0,)),
    ("few", (1, 2), (3.0, 1.0, 1.5), 1, 50.0, TOLERANCES),
    ("few", (2, 1), ROUNDED_SPACING, 1, 0.0, (1.0,)),
    ("few", (1, 2), (1.0, 1.0, 1.0), 3, 100.0, (1.0,)),
    ("two_samples", (1, 2, 3, 4, 5), (3.0, 1.0, 1.5), 1, 95.0, TOLERANCES),
]
# which classes of a pair have an empty surface in pred only, in target only, in both
EMPTINESS = {"absent": {"pred": (3,), "target": (2,), "both": (4,)}}


@functools.lru_cache(maxsize=None)
def mask(name):
    a = MASKS[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def labels(name):
    a = LABELS[name][0]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pair(name):
    p, t = PAIRS[name]()
    p.setflags(write=False), t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def mask_dist2(name, spacing):
    g = dist2(mask(name), spacing)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def metrics_case(k):
    """(counts, table, dicts) of METRICS[k], computed once."""
    name, classes, spacing, connectivity, percentile, tolerances = METRICS[k]
    counts, table = stats(*pair(name), classes, spacing, connectivity, percentile, tolerances)
    counts.setflags(write=False), table.setflags(write=False)
    if counts.ndim == 2:
        return counts, table, _metrics3(counts, table, classes, percentile, tolerances)
    return counts, table, [_metrics3(c, t, classes, percentile, tolerances) for c, t in zip(counts, table)]


def is_exact(spacing):
    return tuple(spacing) in EXACT_SPACINGS
