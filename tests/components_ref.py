"""Numpy restatement of components.py (csrc/components.hip) by its definitions, and the case table of its tests.  No scipy and no
torch: the GPU tests import it.  tests/test_components_cpu.py pins it to scipy.ndimage.label for every case and connectivity.

  roots(labels, connectivity, classes)               int32 root of every voxel's component, -1 off-component
  keep(labels, keep, connectivity, min_size, fill)   (cleaned map, stats table, classes)

A component: voxels of one sample with the same selected value (1..255) joined by a path of neighbours of that value, connectivity
1 / 2 / 3 = offsets with at most that many non-zero coordinates (generate_binary_structure(3, c)).  Its root: the C-order index of
its first voxel within the sample.  Ranking within a (sample, class): size descending, root ascending.
"""
import itertools

import numpy as np

T = 8                    # the tile sides of csrc/components.hip along d and h (MI3D_COMPONENTS_TILE); a tile is 64 voxels along w
MAX_KEEP = 8
STATS_COLUMNS = 3 + 2 * MAX_KEEP
ORGANS = {1: 1, 2: 1, 3: 2}


def _forward_offsets(connectivity):
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0) and sum(c != 0 for c in o) <= connectivity]


def _pair_views(a, off):
    lo = tuple(slice(max(-o, 0), a.shape[i] - max(o, 0)) for i, o in enumerate(off))
    hi = tuple(slice(max(o, 0), a.shape[i] - max(-o, 0)) for i, o in enumerate(off))
    return a[lo], a[hi]


def _roots3(lab, connectivity, classes):
    sel = (lab >= 1) & (lab <= 255)
    if classes is not None:
        sel &= np.isin(lab, list(classes))
    n = lab.size
    r = np.where(sel, np.arange(n, dtype=np.int64).reshape(lab.shape), n)
    pairs = []
    for off in _forward_offsets(connectivity):
        (la, lb), (sa, sb) = _pair_views(lab, off), _pair_views(sel, off)
        eq = sa & sb & (la == lb)
        if eq.any():
            pairs.append((*_pair_views(r, off), eq))
    while True:          # minimum over the neighbours, then pointer jumping, to the fixpoint: the minimum index of the component
        before = r.copy()
        for ra, rb, eq in pairs:
            m = np.minimum(ra, rb)
            np.minimum(ra, m, out=ra, where=eq)          # the two views overlap: lower, never overwrite
            np.minimum(rb, m, out=rb, where=eq)
        table = np.append(r.ravel(), n)
        for _ in range(3):
            table = table[table]
        r[...] = table[:n].reshape(lab.shape)
        if np.array_equal(r, before):
            break
    return np.where(sel, r, -1).astype(np.int32)


def roots(labels, connectivity=1, classes=None):
    labels = np.asarray(labels)
    if labels.ndim == 4:
        return np.stack([_roots3(s, connectivity, classes) for s in labels])
    return _roots3(labels, connectivity, classes)


def _keep3(lab, table, connectivity, min_size, fill):
    r = roots(lab, connectivity, [c for c, _ in table])
    sizes = np.bincount(r[r >= 0], minlength=1)
    out, stats = lab.copy(), np.zeros((len(table), STATS_COLUMNS), dtype=np.int64)
    stats[:, 3 + MAX_KEEP:] = -1
    for row, (c, k) in zip(stats, table):
        own = np.unique(r[lab == c])                                     # ascending roots
        order = own[np.argsort(-sizes[own], kind="stable")]              # size descending, root ascending
        kept = [x for x in order[:k] if sizes[x] >= min_size]
        row[0], row[1], row[2] = len(own), sizes[own].sum(), sizes[kept].sum() if kept else 0
        row[3:3 + len(kept)] = sizes[kept] if kept else []
        row[3 + MAX_KEEP:3 + MAX_KEEP + len(kept)] = kept
        out[(lab == c) & ~np.isin(r, kept)] = fill
    return out, stats


def keep(labels, keep=ORGANS, connectivity=1, min_size=1, fill=0):
    """(cleaned map, int64 stats (N, classes, 19) or (classes, 19) for a 3-D map, classes in ascending order)."""
    labels = np.asarray(labels)
    table = sorted(keep.items())
    classes = tuple(c for c, _ in table)
    if labels.ndim == 3:
        return (*_keep3(labels, table, connectivity, min_size, fill), classes)
    parts = [_keep3(s, table, connectivity, min_size, fill) for s in labels]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), classes


# ---- the cases: the smallest inputs that break a wrong kernel --------------------------------------------------------------------
def _sites(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _iid4(shape, seed):
    return np.random.default_rng(seed).integers(0, 4, shape).astype(np.uint8)


def serpentine(shape):
    """One one-voxel-wide boustrophedon path through the whole volume: a single component whose root 0 has to travel back across
    every seam.  Even slices carry the path (even rows full, joined at alternating ends), odd slices one linking voxel."""
    d, h, w = shape
    plane = np.zeros((h, w), dtype=np.uint8)
    rows = range(0, h, 2)
    for k, row in enumerate(rows):
        plane[row] = 1
        if row + 2 < h:
            plane[row + 1, w - 1 if k % 2 == 0 else 0] = 1
    end = (rows[-1], w - 1 if (len(rows) - 1) % 2 == 0 else 0)          # where the path that starts at (0, 0) leaves the plane
    vol = np.zeros(shape, dtype=np.uint8)
    vol[0::2] = plane
    for j, z in enumerate(range(1, d - 1, 2)):
        vol[z][end if j % 2 == 0 else (0, 0)] = 1
    return vol


def comb(shape):
    """Teeth along h at every other w of the even slices, joined only along the LAST row, the slices only at its last voxel: the
    minimum has to propagate against the scan order."""
    vol = np.zeros(shape, dtype=np.uint8)
    vol[0::2, :, 0::2] = 1
    vol[0::2, -1, :] = 1
    vol[:, -1, -1] = 1
    return vol


def checkerboard(shape):
    d, h, w = np.indices(shape)
    return ((d + h + w) % 2).astype(np.uint8)


def touching_cubes():
    """Two cubes that touch only along an edge (one component from connectivity 2) and two that touch only at a corner
    (connectivity 3), each pair across the seams of four / eight tiles."""
    vol = np.zeros((2 * T + 3, 12, 70), dtype=np.uint8)
    vol[1:4, 5:8, 61:64] = 1
    vol[1:4, 8:11, 64:67] = 1
    vol[5:8, 5:8, 61:64] = 1
    vol[8:11, 8:11, 64:67] = 1
    return vol


def interleaved():
    """Stripes of classes 1 and 2 (never to merge), a block of class 3 and, in int64, the out-of-range value 300."""
    vol = np.zeros((T + 1, T + 1, 66), dtype=np.int64)
    vol[:, 0::2, :] = 1
    vol[:, 1::2, :] = 2
    vol[2:5, 3:7, 10:20] = 3
    vol[6:9, 0:4, 40:66] = 300
    vol[0, :, 30] = 0
    return vol


def blobs():
    """Class 1: components of sizes 5, 5 and 2 (equal sizes: the lower root wins); class 2: one of size 3; class 4 absent; class 5
    unlisted."""
    vol = np.zeros((T + 1, T - 1, 65), dtype=np.uint8)
    vol[0, 0, 60:65] = 1
    vol[4, 3, 2:7] = 1
    vol[8, 6, 63:65] = 1
    vol[2, 2:5, 40] = 2
    vol[5, 5, 5:9] = 5
    return vol


def two_samples():
    """N = 2 identical samples whose first and last rows are foreground: sample 0's last row and sample 1's first row are
    neighbours in memory and must not merge."""
    s = np.zeros((T, T + 1, 65), dtype=np.uint8)
    s[0, 0, :] = 1
    s[-1, -1, :] = 1
    s[3, 4, 10:12] = 2
    return np.stack([s, s])


def balls(side, centres_radii_classes, salt, seed=0):
    """Balls of the given classes and `salt` (a fraction) of voxels overwritten by random classes 1..3, default_rng(seed)."""
    d, h, w = np.indices((side,) * 3 if isinstance(side, int) else side)
    vol = np.zeros(d.shape, dtype=np.uint8)
    for (cd, ch, cw), rad, c in centres_radii_classes:
        vol[(d - cd) ** 2 + (h - ch) ** 2 + (w - cw) ** 2 <= rad * rad] = c
    rng = np.random.default_rng(seed)
    noise = rng.random(vol.shape) < salt
    vol[noise] = rng.integers(1, 4, int(noise.sum())).astype(np.uint8)
    return vol


def organs96():
    return balls(96, (((45, 30, 30), 15, 1), ((50, 65, 45), 22, 2), ((30, 45, 75), 9, 3), ((65, 45, 75), 9, 3)), 0.002)


# name -> builder of a (D, H, W) or (N, D, H, W) array.  Sides: W in {1, 17, 63, 64, 65, 66, 70, 130}; D, H in {1, T - 1, T, T + 1, 2T + 3}
# and one volume smaller than a tile in every axis.  Site densities .31 / .14 / .10 are near the percolation thresholds of
# connectivity 1 / 2 / 3: ragged clusters that cross many seams.
CASES = {
    "perc31": lambda: _sites((2 * T + 3, T + 1, 130), 0.31, 1),
    "perc14": lambda: _sites((T + 1, 2 * T + 3, 65), 0.14, 2),
    "perc10": lambda: _sites((T, T - 1, 63), 0.10, 3),
    "iid4": lambda: _iid4((T - 1, T, 64), 4),
    "thin_w1": lambda: _iid4((2 * T + 3, T + 1, 1), 5),
    "flat_d1": lambda: _sites((1, 2 * T + 3, 65), 0.31, 6),
    "flat_h1": lambda: _iid4((T + 1, 1, 130), 7),
    "small": lambda: _iid4((3, 5, 17), 8),
    "serpentine": lambda: serpentine((2 * T + 3, T + 1, 130)),
    "comb": lambda: comb((T + 1, 2 * T + 3, 65)),
    "checkerboard": lambda: checkerboard((T + 1, T, 65)),
    "touching_cubes": touching_cubes,
    "interleaved": interleaved,
    "blobs": blobs,
    "all_foreground": lambda: np.ones((T + 1, T + 1, 65), dtype=np.uint8),
    "two_samples": two_samples,
    "organs96": organs96,          # 96^3: four balls of radii 15, 22, 9, 9 as classes 1, 2, 3, 3 and 0.2 % salt
}

# (case, keep, min_size, fill): every case with ORGANS, and the ranking edge cases
KEEPS = [(name, ORGANS, 1, 0) for name in CASES] + [
    ("blobs", {1: 1, 2: 3, 4: 1}, 1, 0),          # equal sizes: the lower root; k above the count; an absent class
    ("blobs", {1: 2, 2: 1}, 1, 7),                # fill != 0
    ("blobs", {1: 3, 2: 1}, 4, 0),                # min_size drops class 2's rank-0 component and class 1's third
    ("blobs", {1: 8, 2: 8, 5: 8}, 6, 9),          # min_size above every size of class 1 and 2
    ("checkerboard", {1: 8}, 1, 0),               # connectivity 1: V / 2 components of size 1, ranked by root alone
    ("iid4", {3: 2, 1: 8}, 2, 255),
    ("interleaved", {1: 2, 2: 2}, 1, 0),          # class 3 and the value 300 unlisted: unchanged and uncounted
]
