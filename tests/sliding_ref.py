"""Numpy reference for sliding-window inference with importance-weighted votes: csrc/head_loss.hip's window pass and finishing pass
(mi3d_head_votes_window, mi3d_votes_finish) and segment.predict_labels_sliding.  The checker of tests/test_gpu_sliding.py: written
from the contract in include/mi3d.h, independent of the product module (it imports nothing of it), its schedule pinned by
brute force and its Gaussian table by scipy in tests/test_sliding_ref_cpu.py.  UNPINNED against MONAI's sliding_window_inference,
which the schedule and the importance map are modelled on: MONAI is not available to the tests.

    Per axis   roi = min(window, n); starts [0] if roi == n, else the distinct min(i * interval, n - roi), i < ceil((n - roi) /
               interval) + 1, interval = max(int(roi * (1 - overlap)), 1), ascending.
    Windows    the Cartesian product of the three start lists, D outermost, W innermost.
    Views      (window, flip code), window-major and flip-minor; bit 0 of a code mirrors W, bit 1 H, bit 2 D within the window.
    Tables     "gaussian" g[i] = float32(exp(-0.5 * ((i - (roi - 1) / 2) / (sigma_scale * roi))**2)) from float64; "constant" ones.
    Weight     (g_d[d] * g_h[h]) * g_w[w] in float32, each product rounded on its own.
    Votes      acc[c][o + x] += weight(x) * softmax(logits of the view)[c], flipped back, in view order.
    Finish     labels = first maximum of acc; norm = ((n_d[d] * n_h[h]) * n_w[w]) * float32(views per window) with n_axis[i] the
               float32 rounding of the float64 sum (ascending starts) of the axis table over the windows covering i;
               confidence = acc[label] / norm; means = acc / norm.

Two models of the votes: float64 (accumulate64: the reference the allowance is measured from, with S, the float64 sum of the float32
weights at a voxel) and FLOAT32-STEPWISE (accumulate32: np.float32 product, then np.float32 add, per view, on the float32 rounding
of the float64 softmax), which the `saturated` family must match bit for bit: its p are exactly 0, 1, 1/2 or 1/4, so only the
float32 operations the contract names remain.  Families, layouts, class counts and head_logits are tests/votes_ref.py's.

Allowance on a vote total: K_SLIDE * S(v) * 2^-24, RELATIVE to the weight sum at the voxel (the corner weights of a Gaussian window
are ~1e-8 of the centre's, so an absolute bound would not see them).  K_SLIDE is 4 x the largest ratio |float32 torch - float64| /
(S * 2^-24) over CASES x the families, CLASSES, LAYOUTS, FLIP_SEQUENCES and MODES, float32 torch being F.softmax, torch.flip,
multiply and a sequential add on the CPU (measured by tests/test_sliding_ref_cpu.py::test_float32_torch_stays_within_a_quarter_
of_the_allowance, which prints the ratios with -s).  The factor 4 is for the kernel's ~1-ulp exponential and reciprocal: the rule
of tests/votes_ref.py and tests/loss_ref.py.

    family       largest ratio, float32 torch on the CPU
    saturated    13.06     (gaussian weights; 0 with constant ones, where every term is a multiple of 1/4)
    spaced        5.88
    gauss         7.10
    K_SLIDE = 4 x 13.06 -> 53
The ratio grows with the number of views that cover a voxel (a sequential float32 sum of n terms errs by up to ~n roundings of
the running total); in volume (5, 7, 13) with window (4, 4, 8) and eight flips up to 18 windows x 8 flips = 144 views meet.
The largest band share over the table at this K is 0.26 %.

    MI355X kernel at this K, worst |delta| / allowance over the cases of tests/test_gpu_sliding.py: 0.13 on the operator cases
    (`spaced`, 3 classes), 0.10 on the whole network.  A record, not a bound.

Labels: the reference's wherever margin > 2 x allowance, elsewhere a class within 2 x allowance of the top (votes_ref's band rule
with the per-voxel allowance).  At most BAND_CAP = 1 % of a case's voxels may lie in the band: a condition on the INPUTS, asserted
from the float64 reference alone by the CPU test for every case.
"""
import math

import numpy as np

import votes_ref as VR

U = VR.U
K_SLIDE = 53.0              # 4 x 13.06, the largest float32-torch ratio of the table above
BAND_CAP = VR.BAND_CAP
SIGMA_SCALE = 0.125
FAMILIES, LAYOUTS, CLASSES = VR.FAMILIES, VR.LAYOUTS, VR.CLASSES

# operator-level case table: (volume, window, overlap), the smallest shapes at which the indexing can go wrong
CASES = (((5, 7, 13), (4, 4, 8), 0.5),      # odd W: one-voxel route; clamped last start on every axis
         ((8, 8, 12), (8, 8, 8), 0.25),     # window equals the volume on two axes; aligned 4-voxel route, origins 0 and 4
         ((4, 8, 16), (4, 8, 8), 0.75),     # W % 4 == 0 but W origins 0, 2, 4, 6, 8: unaligned origins leave the vector route
         ((6, 10, 21), (4, 6, 8), 0.5),     # 30 windows; interior voxels covered by 8 of them
         ((3, 8, 8), (4, 8, 8), 0.5))       # window clipped to the volume: one window
FLIP_SEQUENCES = ((0,), tuple(range(8)), (3, 0, 6))
MODES = ("gaussian", "constant")
SAMPLES_PER_CALL = (1, 2, 3)


# ------------------------------------------------------------------------------------------------ schedule and tables
def window_starts(n, window, overlap):
    roi = min(window, n)
    if roi == n:
        return [0]
    interval = max(int(roi * (1 - overlap)), 1)
    k = int(math.ceil((n - roi) / interval)) + 1
    out = []
    for i in range(k):
        s = min(i * interval, n - roi)
        if s not in out:
            out.append(s)
    return sorted(out)


def schedule(volume, window, overlap):
    """(roi, the three start lists, the window origins D outermost)."""
    roi = tuple(min(w, n) for w, n in zip(window, volume))
    starts = [window_starts(n, w, overlap) for n, w in zip(volume, window)]
    return roi, starts, [(a, b, c) for a in starts[0] for b in starts[1] for c in starts[2]]


def view_list(origins, flips):
    return [(o, f) for o in origins for f in flips]


def importance_tables(roi, mode, sigma_scale=SIGMA_SCALE):
    if mode == "constant":
        return [np.ones(r, np.float32) for r in roi]
    assert mode == "gaussian"
    return [np.array([math.exp(-0.5 * ((i - (r - 1) / 2) / (sigma_scale * r)) ** 2) for i in range(r)], np.float64).astype(np.float32)
            for r in roi]


def weight32(tables):
    """(d, h, w) float32 weights of a window: (g_d * g_h) * g_w, each product rounded to float32."""
    gd, gh, gw = (np.asarray(t, np.float32) for t in tables)
    return (gd[:, None, None] * gh[None, :, None]) * gw[None, None, :]


def norm_tables(volume, roi, starts, tables):
    out = []
    for n, r, st, g in zip(volume, roi, starts, tables):
        total = [0.0] * n
        for s in st:
            for j in range(r):
                total[s + j] = total[s + j] + float(g[j])
        out.append(np.array(total, np.float64).astype(np.float32))
    return out


def norm32(norms, views_per_window):
    """(D, H, W) float32: ((n_d * n_h) * n_w) * float32(views per window), each product rounded."""
    return weight32(norms) * np.float32(views_per_window)


# ------------------------------------------------------------------------------------------------ cases
def case_seed(case, layout, c, flips):
    (vol, win, ov) = case
    return list(vol) + list(win) + [int(ov * 100), layout[1], layout[2], c] + [int(f) for f in flips]


def make_case(family, case, layout, c, flips, one_head=False):
    """Operands of a case: z (views, v, cin), w (views, c, cin), b (views, c) (float64 holding dyadic values, votes_ref's families),
    the views [(origin, flip)] and the exact logits (views, C, d, h, w) of every view on its FLIPPED window.  Every view has a
    head of its own, as votes_ref.make_views gives the views of an ensemble (with one head the few distinct probabilities of
    `spaced` tie exactly between two windows far too often for the band cap); one_head: the first view's head for all of them,
    which is what several samples of ONE call share."""
    roi, _, origins = schedule(*case)
    views = view_list(origins, flips)
    rng = np.random.default_rng([FAMILIES.index(family)] + case_seed(case, layout, c, flips))
    ops = [VR.make_view(family, rng, 1, roi[0] * roi[1] * roi[2], layout[1], c) for _ in views]
    z = np.concatenate([o[0] for o in ops])
    w, b = np.stack([ops[0 if one_head else i][1] for i in range(len(ops))]), np.stack([ops[0 if one_head else i][2] for i in range(len(ops))])
    logits = np.concatenate([VR.head_logits(z[i:i + 1], w[i], b[i], (1,) + roi) for i in range(len(ops))])
    return z, w, b, views, logits


# ------------------------------------------------------------------------------------------------ votes
def _box(o, roi):
    return tuple(slice(a, a + r) for a, r in zip(o, roi))


def accumulate64(logits, views, tables, volume):
    """acc (C, D, H, W) float64 in view order and S (D, H, W), the float64 sum of the float32 weights at every voxel."""
    roi = logits.shape[2:]
    wt = weight32(tables).astype(np.float64)
    acc = np.zeros((logits.shape[1],) + tuple(volume))
    s = np.zeros(tuple(volume))
    for lg, (o, f) in zip(logits, views):
        p = VR.flip(VR.softmax64(lg[None])[0], f)
        acc[(slice(None),) + _box(o, roi)] += wt * p
        s[_box(o, roi)] += wt
    return acc, s


def accumulate32(logits, views, tables, volume, weights=None, unflip=True):
    """The float32-stepwise model: per view np.float32 product, then np.float32 add, on the float32 rounding of the float64
    softmax.  weights / unflip: for the mutants of the CPU test (another weight association; the mirrored gather skipped)."""
    roi = logits.shape[2:]
    wt = weight32(tables) if weights is None else np.asarray(weights, np.float32)
    acc = np.zeros((logits.shape[1],) + tuple(volume), np.float32)
    for lg, (o, f) in zip(logits, views):
        p = VR.softmax64(lg[None])[0].astype(np.float32)
        p = VR.flip(p, f) if unflip else p
        box = (slice(None),) + _box(o, roi)
        acc[box] = acc[box] + wt * p
    return acc


def finish32(acc, norm, normalize=True):
    """labels uint8, confidence float32 and (with normalize) the means, float32 IEEE divisions, from float32 totals."""
    acc = np.asarray(acc, np.float32)
    labels = acc.argmax(axis=0).astype(np.uint8)
    top = np.take_along_axis(acc, labels[None].astype(np.int64), axis=0)[0]
    return labels, top / norm, (acc / norm[None] if normalize else None)


def labels_and_margin(acc):
    labels, margin = VR.labels_and_margin(acc[None])
    return labels[0], margin[0]


def allowance(s, k=K_SLIDE):
    return k * np.asarray(s, np.float64) * U


def band_share(acc, s):
    return float((labels_and_margin(acc)[1] <= 2.0 * allowance(s)).mean())


def label_errors(got, acc, s):
    """Voxels whose label breaks the rule: the reference's wherever margin > 2 x allowance, else a class of the band."""
    want, margin = labels_and_margin(acc)
    a2 = 2.0 * allowance(s)
    g = np.asarray(got).astype(np.int64)
    if g.max(initial=0) >= acc.shape[0]:
        return int(g.size)
    mine = np.take_along_axis(acc, g[None], axis=0)[0]
    in_band = mine >= acc.max(axis=0) - a2
    return int(np.count_nonzero(np.where(margin > a2, g != want, ~in_band)))


def torch_float32_acc(logits, views, tables, volume):
    """What the allowance is calibrated on: F.softmax, torch.flip, multiply and a sequential add in float32 on the CPU."""
    import torch
    import torch.nn.functional as F
    roi = logits.shape[2:]
    wt = torch.from_numpy(weight32(tables))
    acc = torch.zeros((logits.shape[1],) + tuple(volume), dtype=torch.float32)
    for lg, (o, f) in zip(logits, views):
        p = F.softmax(torch.from_numpy(np.asarray(lg, np.float32)), dim=0)
        ax = [a % 4 for a in VR.flip_axes(f)]
        p = torch.flip(p, ax) if ax else p
        box = (slice(None),) + _box(o, roi)
        acc[box] = acc[box] + wt * p
    return acc.numpy()
