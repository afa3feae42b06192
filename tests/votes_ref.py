"""Plain float64 numpy reference for the flip / model ensemble votes of csrc/head_loss.hip (mi3d_head_votes,
segment.predict_labels_ensemble), the input families the tests run it on and the allowance a float32 implementation is held to.
The checker of tests/test_gpu_votes.py: written from the contract in include/mi3d.h, independent of the product module (it
imports nothing of it), and pinned to float64 torch by tests/test_votes_ref_cpu.py.

    A view is (operands of a head, flip code f): bit 0 of f mirrors W, bit 1 H, bit 2 D.  For the views in the order given
    L_v    = z_v @ w_v^T + b_v              the logits of the head on the FLIPPED input, (N, C, D, H, W)
    p_v    = softmax(L_v, axis=1)           float64
    votes  = sum_v flip_back(p_v)           in view order
    labels = first maximum of votes over the classes;  margin = top vote - second vote

The operands of every family are dyadic (z bf16-exact, every product and partial sum exact in float32), so the float64 logits
ARE the float32 logits of any fused-multiply-add chain: the reference and the kernel start from the same numbers, as
test_gpu_segment._dyadic arranges for the label tests.

Families
    saturated   z has one non-zero channel (1 or 2) per voxel and w gives the winners of that channel 1024 and the others a
                small non-positive integer: the maximum is shared by 1, 2 or 4 classes and leads by >= 1024, so exp underflows
                to exactly 0 in float32 AND in float64 and every p is exactly 0, 1, 1/2 or 1/4.  Every vote is a small multiple of
                1/4: exact in both precisions in any order.  Votes and labels must equal the reference bit for bit, ties between
                views (which fall to the lower class) included.
    spaced      one non-zero channel (+-1 or +-2) per voxel, the classes' weights for it distinct multiples of 2^-6: the logits
                of a voxel are >= 2^-6 apart, so p keeps the order of the logits with ~2^17 ulps to spare and a single unflipped view must
                label as mi3d_head_labels does.
    gauss       dense random dyadic operands (z multiples of 1/8 in [-4, 4], w of 2^-12, bias of 1/2: 23 bits
                at the most, and exact ties between classes are rare).

Allowance on a vote total: K_VOTES * views * 2^-24 (absolute: a vote total is at most `views`).  K_VOTES is 4 x the largest
ratio |float32 torch - float64| / (views * 2^-24) over CASES and the families above, float32 torch being F.softmax, torch.flip
and a sequential sum on the CPU (measured by tests/test_votes_ref_cpu.py::test_float32_torch_stays_within_a_quarter_of_the_
allowance, which prints the ratios with -s).  The margin of 4 is for the kernel's two ~1-ulp hardware approximations (exponential,
reciprocal), where torch's CPU path has libm and a true division: the rule of tests/loss_ref.py.

    family       largest ratio, float32 torch on the CPU
    saturated    0       (exact)
    spaced       3.00
    gauss        4.18
    K_VOTES = 4 x 4.18 -> 17

Labels: equal to the reference wherever margin > 2 x allowance, elsewhere one of the classes whose vote is within 2 x allowance
of the top one (the band).  The band may hold at most BAND_CAP = 1 % of a case's voxels: a condition on the INPUTS, asserted
from the reference alone by the CPU test for every case.

    MI355X kernel at this K, worst |delta| / allowance over the cases of tests/test_gpu_votes.py: 0.25 on the operator cases
    (gauss, 8 classes), 0.17 on the whole network.  A record, not a bound.
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of float32 (round to nearest)
K_VOTES = 17.0              # 4 x 4.18, the largest float32-torch ratio of the table above
BAND_CAP = 0.01
LEAD = 1024.0               # saturated: exp(-1024) is 0 in float64 as well

# operator-level case table: shapes (N, D, H, W), layouts (dtype, Cin, channel stride), class counts, view sequences
SHAPES = ((2, 3, 5, 7),     # V = 105, N * V odd: no vector width divides it, the second sample starts unaligned
          (1, 4, 6, 40),    # V = 960: less than one block of 4-voxel groups
          (1, 9, 16, 24),   # V = 3456: several blocks, the last one ragged
          (3, 2, 2, 2),     # two groups per sample, every group crosses rows and planes
          (1, 1, 1, 70))    # one row; V % 4 != 0
LAYOUTS = (("bf16", 16, 16), ("bf16", 32, 40), ("fp32", 5, 5))
CLASSES = (2, 3, 4, 8)
FLIP_SEQUENCES = tuple((f,) for f in range(8)) + (tuple(range(8)), (3, 0, 6))     # singles, all eight, one MIDDLE pass
FAMILIES = ("saturated", "spaced", "gauss")


def cases():
    """Every (shape, layout, classes, flips) of the table."""
    for shape in SHAPES:
        for layout in LAYOUTS:
            for c in CLASSES:
                for flips in FLIP_SEQUENCES:
                    yield shape, layout, c, flips


def case_seed(shape, layout, c, flips):
    return [int(x) for x in shape] + [layout[1], layout[2], c] + [int(f) for f in flips]


def flip_axes(code):
    """Axes of an (..., D, H, W) array that flip code `code` mirrors."""
    return tuple(ax for bit, ax in ((1, -1), (2, -2), (4, -3)) if code & bit)


def flip(a, code):
    ax = flip_axes(code)
    return np.flip(a, ax) if ax else a


# ---------------------------------------------------------------------------------------------- input families
def make_view(family, rng, n, v, cin, c):
    """Operands of one view: z (n, v, cin), w (c, cin), b (c), float64 holding dyadic values."""
    if family == "gauss":
        z = np.clip(np.round(rng.standard_normal((n, v, cin)) * 8.0) / 8.0, -4.0, 4.0)
        w = np.clip(np.round(rng.standard_normal((c, cin)) * 0.3 * 4096.0) / 4096.0, -1.0, 1.0)
        b = rng.integers(-2, 3, c) / 2.0
        return z, w, b
    chan = rng.integers(0, cin, (n, v))
    amp = rng.integers(1, 3, (n, v)).astype(np.float64)
    if family == "spaced":
        amp *= rng.choice(np.array([-1.0, 1.0]), (n, v))
    z = np.zeros((n, v, cin))
    np.put_along_axis(z, chan[..., None], amp[..., None], axis=2)
    w = np.zeros((c, cin))
    if family == "saturated":
        sizes = [s for s in (1, 2, 4) if s <= c]
        for j in range(cin):
            win = rng.choice(c, size=sizes[rng.integers(0, len(sizes))], replace=False)
            w[:, j] = -rng.integers(0, 9, c)
            w[win, j] = LEAD
        return z, w, np.full(c, 3.0)
    if family == "spaced":
        for j in range(cin):
            w[:, j] = (rng.choice(257, size=c, replace=False) - 128) / 64.0
        return z, w, np.full(c, 0.5)
    raise ValueError(family)


def make_views(family, shape, layout, c, flips):
    """One set of operands per view of a case, from a generator seeded by the case."""
    rng = np.random.default_rng([FAMILIES.index(family)] + case_seed(shape, layout, c, flips))
    n, v = shape[0], shape[1] * shape[2] * shape[3]
    return [make_view(family, rng, n, v, layout[1], c) for _ in flips]


def head_logits(z, w, b, shape):
    """(N, C, D, H, W) float64 logits of a view's operands; asserts that they are exact in float32."""
    n, d, h, wd = shape
    lg = z @ w.T + b
    assert np.array_equal(lg.astype(np.float32).astype(np.float64), lg)
    return np.ascontiguousarray(lg.reshape(n, d, h, wd, -1).transpose(0, 4, 1, 2, 3))


# ---------------------------------------------------------------------------------------------- reference
def softmax64(lg):
    a = np.asarray(lg, np.float64)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def votes_from_logits(logits, flips):
    """votes (N, C, D, H, W) float64 from the per-view logits (each on its flipped input), summed in view order."""
    total = None
    for lg, f in zip(logits, flips):
        p = flip(softmax64(lg), f)
        total = p if total is None else total + p
    return np.array(total, order="C", copy=True)          # (a flipped view has negative strides)


def labels_and_margin(votes):
    """First maximum over the classes (uint8) and top vote - second vote (inf for a single class)."""
    labels = votes.argmax(axis=1).astype(np.uint8)
    if votes.shape[1] == 1:
        return labels, np.full(labels.shape, np.inf)
    srt = np.sort(votes, axis=1)
    return labels, srt[:, -1] - srt[:, -2]


def allowance(views, k=K_VOTES):
    return k * views * U


def band_share(votes, views):
    """Share of the voxels whose margin is within 2 x allowance: where the label is not pinned."""
    return float((labels_and_margin(votes)[1] <= 2.0 * allowance(views)).mean())


def label_errors(got, votes, views):
    """Number of voxels whose label breaks the rule: the reference's wherever margin > 2 x allowance, else a class of the band."""
    want, margin = labels_and_margin(votes)
    a2 = 2.0 * allowance(views)
    g = np.asarray(got).astype(np.int64)
    if g.max(initial=0) >= votes.shape[1]:
        return int(g.size)
    mine = np.take_along_axis(votes, g[:, None], axis=1)[:, 0]
    in_band = mine >= votes.max(axis=1) - a2
    return int(np.count_nonzero(np.where(margin > a2, g != want, ~in_band)))


def torch_float32_votes(logits, flips):
    """What the allowance is calibrated on: F.softmax, torch.flip and a sequential sum in float32 on the CPU."""
    import torch
    import torch.nn.functional as F
    total = None
    for lg, f in zip(logits, flips):
        p = F.softmax(torch.from_numpy(np.asarray(lg, np.float32)), dim=1)
        ax = [a % 5 for a in flip_axes(f)]
        p = torch.flip(p, ax) if ax else p
        total = p if total is None else total + p
    return total.numpy()
