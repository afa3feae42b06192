"""Plain float64 numpy model of the soft restore (include/mi3d.h mi3d_restore_votes3, resample.restore_labels_soft): float32 class
votes on the training grid zoomed linearly onto the RAS sides of a scan, the first maximum over the classes taken there, and the
result stored under an orientation (orient_ref.store_as, the inverse of reorient_to_ras).  The checker of
tests/test_gpu_restore_soft.py: written from the contract, independent of the product module (it imports nothing of it), and pinned
to scipy.ndimage.zoom(order=1, mode='nearest', prefilter=False) by tests/test_restore_soft_cpu.py.

    per axis   z = (n_grid - 1) / (n - 1), 1.0 for n = 1;  c = i * z;  f = floor(c);  t = c - f
               taps clip(f, 0, n_grid - 1), clip(f + 1, 0, n_grid - 1);  weights 1.0 - t, t
    r(a, b) = p[k, d_a, h_b, w_0] * ww0 + p[k, d_a, h_b, w_1] * ww1
    s(a)    = r(a, 0) * wh0 + r(a, 1) * wh1
    v_k     = s(0) * wd0 + s(1) * wd1          float64; numpy's a * w0 + b * w1 on arrays rounds each product and the sum
    label = first maximum of v_k;  confidence = float32(v_label)

The kernel does the same operations in the same order without contraction, so the GPU tests compare with array_equal.

Input families (votes_of)
    gauss    softmax of N(0, 2^2) logits, rounded to float32
    sum8     the same times 8, as a kept vote total of eight views is: nothing may assume p <= 1
    onehot   saturated maps of random 2 x 2 x 2 blobs: between two blobs the votes tie (0.5 / 0.5 at a midpoint), and the first
             maximum decides
    dyadic   multiples of 2^-6 in [0, 1]
On EXACT_SHAPES, where n - 1 = 2^j (n_grid - 1) on every axis, t is a multiple of 2^-j and every product and sum of the last two
families is exact: the model, scipy and the kernel must agree to the bit.

The bound against scipy.  u = 2^-53, P = max|p|.  Both sides start from the same float64 weights (1.0 - t and t, t = c - floor(c)),
which are >= 0 and sum to 1 per axis up to the one rounding of 1.0 - t, and both evaluate the same convex combination E of eight
taps, |E| <= P; they differ in how they round.  Every partial result is a non-negative-weighted
combination of taps with weights summing to at most 1, so its magnitude is at most P and one rounding adds at most u P (weighted down
by the weights still to come).  The model: a value passes through one rounded product and one rounded sum per level: three levels,
|model - E| <= 6 u P to first order.  scipy: per tap the coefficient times the three weights (3 rounded
products), then the eight terms added in turn starting from 0 (the first add is exact, 7 rounded sums of non-negative-weighted terms):
|scipy - E| <= (3 + 7) u P.  |model - scipy| <= (6 + 10) u P = K_VALUE u P with K_VALUE = 16; second-order terms are below 2^-40 of
that.  A worst case of one-sided roundings, which no input reaches:
    measured maximum of |model - scipy| / (u P) over CASES and IDENTITY (tests/test_restore_soft_cpu.py prints it with -s): 2.0
"""
import collections
import functools

import numpy as np

U64 = 2.0 ** -53
K_VALUE = 16.0
BAND_CAP = 0.01             # votes_ref.BAND_CAP's figure
FAMILIES = ("gauss", "sum8", "onehot", "dyadic")
EXACT_FAMILIES = ("onehot", "dyadic")

Case = collections.namedtuple("Case", "name family classes grid ras")

GRID, RAS = (5, 6, 7), (9, 17, 13)                  # the orientation case: three different upsampling ratios, one of them 2
EXACT_SHAPES = ((5, 3, 4), (9, 17, 13))             # 8 = 2 * 4, 16 = 8 * 2, 12 = 4 * 3
# Store pieces.  The kernel cuts a row into 16-byte pieces (unaligned head, whole pieces, tail) only where the stored-fastest axis is
# NOT the grid's W; where it is, consecutive lanes store consecutive bytes and alignment does not matter.  So the lengths come three
# times, with the long side on RAS W, D and H, and the GPU test stores each with the long side fastest in memory: rows of F bytes
# start at multiples of F, so an odd F gives every alignment; 16 has neither head nor tail, 37 and 50 have a head, two or more whole
# pieces and a tail of several bytes on some rows, 1 is a fastest axis of one element.  walk() restates the launcher's choice and
# tests/test_restore_soft_cpu.py asserts from it where each stored case lands.
PIECE_LENGTHS = (1, 15, 16, 17, 37, 50)
PIECE_STORES = {          # long side -> (RAS sides for length f, [(perm, signs, memory order) that make the long side fastest])
    "W": (lambda f: (3, 5, f), [((0, 1, 2), (1, 1, 1), "C"), ((0, 1, 2), (1, 1, -1), "C"), ((2, 0, 1), (-1, 1, -1), "F")]),
    "D": (lambda f: (f, 7, 3), [((0, 1, 2), (1, 1, 1), "F"), ((0, 1, 2), (-1, 1, 1), "F"), ((2, 1, 0), (1, -1, 1), "C")]),
    "H": (lambda f: (3, f, 5), [((0, 2, 1), (1, 1, 1), "C"), ((0, 2, 1), (1, 1, -1), "C"), ((1, 2, 0), (-1, 1, 1), "F")]),
}

CASES = (
    [Case("orient", "gauss", 4, GRID, RAS)]
    + [Case(f"{fam}-C{c}", fam, c, *EXACT_SHAPES) for c in (2, 3, 4, 8) for fam in FAMILIES]
    + [Case(f"piece{side}-F{f}", "gauss", 3, (4, 5, 6), PIECE_STORES[side][0](f)) for side in "WDH" for f in PIECE_LENGTHS]
    + [Case("grid-side-1", "gauss", 3, (1, 5, 6), (3, 7, 17)), Case("ras-side-1", "sum8", 3, (4, 5, 6), (7, 1, 18)),
       Case("down", "gauss", 4, (12, 12, 12), (5, 7, 4))]
)
IDENTITY = Case("identity", "gauss", 4, GRID, GRID)   # every t is 0: not in CASES, two of the three mutants are the model there


def case(name):
    return next(c for c in CASES + [IDENTITY] if c.name == name)


def layout(shape, order):
    """Element strides of a dense stored shape, C-ordered or Fortran-ordered."""
    d, h, w = shape
    return (h * w, w, 1) if order == "C" else (1, d, d * h)


def walk(ras, perm, signs, order):
    """Where a stored case lands in the kernel, restated from the launcher: the RAS axes by increasing stored stride, an axis of one
    element last (F, M, S); lane = 0 where F is RAS W (no pieces), 1 where M is, 2 where S is.  Returns (lane, length of F, per row
    of the destination (head, whole 16-byte pieces, tail) for a 16-byte aligned buffer)."""
    stored = tuple(ras[a] for a in perm)
    strides = layout(stored, order)
    stride = [strides[list(perm).index(a)] for a in range(3)]
    f, m, s = sorted(range(3), key=lambda a: (ras[a] <= 1, stride[a]))
    lane = 0 if f == 2 else 1 if m == 2 else 2
    rows = []
    for i in range(ras[s]):
        for j in range(ras[m]):
            head = min(-(i * stride[s] + j * stride[m]) % 16, ras[f]) if ras[f] > 1 else 0
            rows.append((head, (ras[f] - head) // 16, (ras[f] - head) % 16))
    return lane, ras[f], rows


# ---------------------------------------------------------------------------------------------- input families
def votes_of(c):
    """float32 (C, Dg, Hg, Wg) votes of a case, from a generator seeded by the case."""
    rng = np.random.default_rng([FAMILIES.index(c.family), c.classes, *c.grid, *c.ras])
    shape = (c.classes,) + tuple(c.grid)
    if c.family in ("gauss", "sum8"):
        lg = rng.standard_normal(shape) * 2.0
        e = np.exp(lg - lg.max(axis=0, keepdims=True))
        p = (e / e.sum(axis=0, keepdims=True)).astype(np.float32)
        return p * np.float32(8.0) if c.family == "sum8" else p
    if c.family == "onehot":
        coarse = rng.integers(0, c.classes, tuple((n + 1) // 2 for n in c.grid))
        lab = coarse.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:c.grid[0], :c.grid[1], :c.grid[2]]
        return (lab[None] == np.arange(c.classes)[:, None, None, None]).astype(np.float32)
    if c.family == "dyadic":
        return (rng.integers(0, 65, shape) / 64.0).astype(np.float32)
    raise ValueError(c.family)


# ---------------------------------------------------------------------------------------------- the model
def taps(n_grid, n):
    """(idx0, idx1, w0, w1) of one axis, one entry per RAS index."""
    z = float(n_grid - 1) / float(n - 1) if n > 1 else 1.0
    c = np.arange(n, dtype=np.float64) * z
    f = np.floor(c)
    t = c - f
    return (np.clip(f, 0, n_grid - 1).astype(np.int64), np.clip(f + 1.0, 0, n_grid - 1).astype(np.int64), 1.0 - t, t)


def taps_swapped(n_grid, n):
    i0, i1, w0, w1 = taps(n_grid, n)
    return i0, i1, w1, w0


def taps_round(n_grid, n):
    """round for floor"""
    z = float(n_grid - 1) / float(n - 1) if n > 1 else 1.0
    c = np.arange(n, dtype=np.float64) * z
    f = np.round(c)
    t = c - f
    return (np.clip(f, 0, n_grid - 1).astype(np.int64), np.clip(f + 1.0, 0, n_grid - 1).astype(np.int64), 1.0 - t, t)


def taps_grid_mode(n_grid, n):
    """the n_grid / n coordinate mapping of grid_mode=True"""
    c = np.arange(n, dtype=np.float64) * (float(n_grid) / float(n))
    f = np.floor(c)
    t = c - f
    return (np.clip(f, 0, n_grid - 1).astype(np.int64), np.clip(f + 1.0, 0, n_grid - 1).astype(np.int64), 1.0 - t, t)


MUTANTS = {"weights swapped": taps_swapped, "round for floor": taps_round, "grid_mode coordinates": taps_grid_mode}


def zoom_votes(p, ras, taps_fn=taps):
    """v (C, D, H, W) float64 of votes p (C, Dg, Hg, Wg): W first, then H, then D.  Taking the W level on every grid row and then
    selecting the H and D taps gives the values of the nested formula: the same operands meet in the same operations."""
    p = np.asarray(p, dtype=np.float64)
    (d0, d1, wd0, wd1), (h0, h1, wh0, wh1), (w0, w1, ww0, ww1) = (taps_fn(g, n) for g, n in zip(p.shape[1:], ras))
    r = p[:, :, :, w0] * ww0 + p[:, :, :, w1] * ww1
    s = r[:, :, h0, :] * wh0[:, None] + r[:, :, h1, :] * wh1[:, None]
    return s[:, d0] * wd0[:, None, None] + s[:, d1] * wd1[:, None, None]


def labels_confidence(v):
    """(uint8 first maximum over the classes, float32 of its value)."""
    lab = v.argmax(axis=0)
    return lab.astype(np.uint8), np.take_along_axis(v, lab[None], axis=0)[0].astype(np.float32)


Model = collections.namedtuple("Model", "votes values labels confidence")


@functools.lru_cache(maxsize=None)
def model(c):
    """The case's votes and the model's result in RAS order, computed once and shared (callers must not write into it)."""
    p = votes_of(c)
    v = zoom_votes(p, c.ras)
    lab, conf = labels_confidence(v)
    for a in (p, v, lab, conf):
        a.setflags(write=False)
    return Model(p, v, lab, conf)


def bound(p):
    return K_VALUE * U64 * float(np.abs(p).max())


def top_two_gap(v):
    srt = np.sort(v, axis=0)
    return srt[-1] - srt[-2]
