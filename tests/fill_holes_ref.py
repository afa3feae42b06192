"""Numpy restatement of components.fill_holes (csrc/components.hip) by its definitions, and the case table of its tests.  No scipy
and no torch: the GPU tests import it.  tests/test_fill_holes_cpu.py pins it to the scipy route (scipy.ndimage.label of the
background, binary_dilation per component, np.unique of the ring; binary_fill_holes on one-class maps) for every case and
connectivity.

  fill(labels, classes, connectivity, max_size)   (filled map, stats (.., classes, 2), summary (.., 4), classes ascending)

A background component: a component of labels == 0 of one sample under generate_binary_structure(3, connectivity).  Its ring: the
positions that are not in it but are such neighbours of one of its voxels, positions outside the volume included.  Enclosed: no
ring position outside the volume.  Filled with v: enclosed, every ring voxel carries v, v is listed, at most max_size voxels
(None: no limit).  stats per listed class: holes filled, voxels filled.  summary: enclosed, filled, mixed (two or more ring values),
skipped (one ring value, unlisted or outside 1..255, or too large).  All int64 values outside 0..255 are ONE ring value.

The keyword switches of fill() each break one rule; tests/test_fill_holes_cpu.py shows that the case table sees every one of them.
"""
import itertools

import numpy as np

import components_ref as C

OTHER, OUTSIDE = 256, 257          # ring codes above every label value: any int64 value outside 0..255; a position outside the volume
NO_RING = np.iinfo(np.int64).max


def _offsets(connectivity):
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0) and sum(c != 0 for c in o) <= connectivity]


def _fill3(lab, classes, connectivity, max_size, face_rule=True, mixed_takes_min=False, ring_connectivity=None, any_class=False):
    background = lab == 0
    out = lab.copy()
    stats, summary = np.zeros((len(classes), 2), dtype=np.int64), np.zeros(4, dtype=np.int64)
    if not background.any():
        return out, stats, summary
    roots = C._roots3(background.astype(np.uint8), connectivity, (1,)).ravel()
    codes = lab.astype(np.int64)
    codes = np.pad(np.where((codes >= 0) & (codes <= 255), codes, OTHER), 1, constant_values=OUTSIDE)
    at = np.flatnonzero(background)
    mine = roots[at]
    d, h, w = np.unravel_index(at, lab.shape)
    lo, hi = np.full(lab.size, NO_RING), np.zeros(lab.size, dtype=np.int64)
    for dd, dh, dw in _offsets(connectivity if ring_connectivity is None else ring_connectivity):
        c = codes[d + 1 + dd, h + 1 + dh, w + 1 + dw]
        ring = c != 0 if face_rule else (c != 0) & (c != OUTSIDE)
        np.minimum.at(lo, mine[ring], c[ring])
        np.maximum.at(hi, mine[ring], c[ring])
    sizes = np.bincount(mine, minlength=lab.size)
    value_of = np.zeros(lab.size, dtype=np.int64)          # per root: the value its component is filled with, 0 for none
    for r in np.unique(mine):
        if hi[r] == 0 or hi[r] == OUTSIDE:          # no ring at all (only where a rule is broken), or open
            continue
        summary[0] += 1
        one = lo[r] == hi[r] or mixed_takes_min
        listed = 1 <= lo[r] <= 255 if any_class else lo[r] in classes
        if one and listed and (max_size is None or sizes[r] <= max_size):
            summary[1] += 1
            value_of[r] = lo[r]
            if lo[r] in classes:
                stats[classes.index(lo[r])] += (1, sizes[r])
        else:
            summary[2 if not one else 3] += 1
    filled = value_of[mine]
    out.ravel()[at[filled > 0]] = filled[filled > 0]
    return out, stats, summary


def fill(labels, classes=(1, 2, 3), connectivity=1, max_size=None, **broken):
    """(filled map, int64 stats (N, classes, 2) and summary (N, 4), un-batched for a 3-D map, classes in ascending order)."""
    labels = np.asarray(labels)
    classes = tuple(sorted(classes))
    if labels.ndim == 3:
        return (*_fill3(labels, classes, connectivity, max_size, **broken), classes)
    parts = [_fill3(s, classes, connectivity, max_size, **broken) for s in labels]
    return (*(np.stack([p[k] for p in parts]) for k in range(3)), classes)


MUTANTS = {
    "no_face_rule": dict(face_rule=False),                 # positions outside the volume are no part of the ring
    "mixed_takes_min": dict(mixed_takes_min=True),         # a ring of several values fills with the smallest
    "ring_connectivity_1": dict(ring_connectivity=1),      # the ring by faces only, whatever the connectivity
    "any_class": dict(any_class=True),                     # the list of classes is ignored
}


# ---- the cases: the smallest inputs that break a wrong kernel --------------------------------------------------------------------
T = C.T
BOX = (2 * T + 3, 12, 70)


def punched_slabs(density, seed, shape=(2 * T + 3, 17, 130)):
    """Classes 1 / 2 / 3 in thirds along h, a fraction `density` of the voxels punched to 0: hundreds of small holes, ringed by one
    class inside a slab and by two across a slab boundary, in every tile and across every seam."""
    vol = np.empty(shape, dtype=np.uint8)
    third = -(-shape[1] // 3)
    for k in range(3):
        vol[:, k * third:(k + 1) * third] = k + 1
    vol[np.random.default_rng(seed).random(shape) < density] = 0
    return vol


def box(dtype=np.uint8):
    """A box of class 2 with walls two voxels thick around one cavity of 11 x 4 x 61 = 2684 voxels that crosses the tile seams at
    d = 8 and w = 64; background around it."""
    vol = np.zeros(BOX, dtype=dtype)
    vol[2:17, 2:10, 3:68] = 2
    vol[4:15, 4:8, 5:66] = 0
    return vol


def box_corner_channel():
    """The box with a channel from the cavity's corner to the outside whose voxels touch only at corners: the cavity is enclosed at
    connectivity 1 and 2 and open at 3."""
    vol = box()
    vol[3, 3, 4] = vol[2, 2, 3] = 0
    return vol


def box_edge_channel():
    """The box with a channel whose voxels touch only along edges: open from connectivity 2."""
    vol = box()
    vol[3, 3, 30] = vol[2, 2, 30] = 0
    return vol


def box_with_block():
    """A block of class 3 floats in the cavity: the ring carries 2 and 3, nothing is filled."""
    vol = box()
    vol[8:10, 5:7, 30:34] = 3
    return vol


def int64_walls():
    """int64: a cavity ringed by the value 300 alone (skipped), one ringed by 300 and 2 (mixed), one ringed by 2 and -7 (mixed) and
    one ringed by 1 alone (filled)."""
    vol = np.zeros((T + 1, 2 * T + 3, 65), dtype=np.int64)
    vol[1:6, 1:6, 1:8] = 300
    vol[2:5, 2:5, 2:7] = 0
    vol[1:6, 7:12, 60:65] = 2
    vol[1:6, 7:12, 62:65] = 300
    vol[2:5, 8:11, 61:64] = 0
    vol[3:8, 13:18, 20:30] = 2
    vol[3:8, 13:18, 25:30] = -7
    vol[4:7, 14:17, 21:29] = 0
    vol[3:8, 1:6, 30:40] = 1
    vol[4:7, 2:5, 31:39] = 0
    return vol


def one_voxel():
    vol = np.full((T - 1, T + 1, 63), 3, dtype=np.uint8)
    vol[3, 4, 31] = 0
    return vol


def diagonal_neighbours():
    """Three one-voxel holes in class 3: one with class 3 all around, one with a voxel of class 1 across an edge, one with a voxel of
    class 2 across a corner.  By faces every ring carries 3 alone; the second is mixed from connectivity 2, the third at 3."""
    vol = np.full((T + 1, T - 1, 65), 3, dtype=np.uint8)
    vol[2, 2, 10] = vol[4, 3, 62] = vol[6, 4, 30] = 0
    vol[5, 3, 63] = 1
    vol[7, 5, 31] = 2
    return vol


def two_samples():
    """N = 2: sample 0 has a cavity in class 1; sample 1 has the same cavity opened to the face d = 0.  Sample 0's last row and
    sample 1's first row are background and neighbours in memory: both are open, each within its own sample."""
    s = np.ones((T, T + 1, 65), dtype=np.uint8)
    s[3:5, 3:6, 20:40] = 0
    a, b = s.copy(), s.copy()
    a[-1, -1, :] = 0
    b[0, 0, :] = 0
    b[0:3, 4, 25] = 0
    return np.stack([a, b])


def organs48():
    """48^3: balls of classes 1, 2, 3, 3 with 0.2 % salt of random classes, then small pockets of 0 cut into every ball, one of
    them with a voxel of another class on its ring."""
    vol = C.balls(48, (((22, 15, 15), 8, 1), ((25, 32, 22), 11, 2), ((15, 22, 37), 5, 3), ((33, 22, 37), 5, 3)), 0.002)
    vol[22:24, 15:17, 14:17] = 0
    vol[24:27, 31:34, 20:24] = 0
    vol[25, 32, 19] = 1          # a voxel of another class on that pocket's ring: mixed at every connectivity
    vol[20, 28, 18] = 0
    vol[15, 22, 37] = 0
    vol[33, 22, 36:38] = 0
    return vol


# name -> builder of a (D, H, W) or (N, D, H, W) array.  Sides: W in {1, 63, 64, 65, 70, 130}; D, H in {1, T - 1, T, T + 1, 12, 17, 2T + 3}
CASES = {
    "punched25": lambda: punched_slabs(0.25, 11),
    "punched10": lambda: punched_slabs(0.10, 12),
    "punched06": lambda: punched_slabs(0.06, 13),
    "box": box,
    "box_corner_channel": box_corner_channel,
    "box_edge_channel": box_edge_channel,
    "box_with_block": box_with_block,
    "int64_walls": int64_walls,
    "all_background": lambda: np.zeros((T, T + 1, 65), dtype=np.uint8),
    "all_foreground": lambda: np.full((T + 1, T, 64), 2, dtype=np.uint8),
    "one_voxel": one_voxel,
    "diagonal_neighbours": diagonal_neighbours,
    "flat_d1": lambda: C._iid4((1, 2 * T + 3, 65), 21),
    "flat_h1": lambda: C._iid4((T + 1, 1, 130), 22),
    "thin_w1": lambda: C._iid4((2 * T + 3, T + 1, 1), 23),
    "two_samples": two_samples,
    "organs48": organs48,
}
PUNCHED = {"punched25": 1, "punched10": 2, "punched06": 3}          # the connectivity each density is chosen for
SINGLE_CLASS = {"box": 2, "box_corner_channel": 2, "box_edge_channel": 2, "all_background": 2, "all_foreground": 2, "one_voxel": 3,
                "two_samples": 1}          # maps of one class c: binary_fill_holes(labels == c) * c is the contract too

# (case, classes, max_size): every case with the default classes and no limit, then class subsets and size limits
FILLS = [(name, (1, 2, 3), None) for name in CASES] + [
    ("punched25", (1, 3), None),          # the holes of class 2 are skipped
    ("punched10", (3,), None),
    ("punched25", (1, 2, 3), 1),          # one-voxel holes only
    ("punched06", (2, 1), 2),
    ("box", (1, 3), None),                # the one hole is ringed by an unlisted class
    ("box", (2,), 2683),                  # one voxel too large
    ("box", (2,), 2684),
    ("organs48", (2,), 5),
    ("int64_walls", (1, 2, 255), None),
]
