"""Plain float64 references of the input pipeline's per-volume kernels (csrc/preproc.hip) and the inputs their tests share
(TEST INFRASTRUCTURE: tests/test_gpu_preproc_ops.py holds the kernels to these, tests/test_preproc_ops_ref_cpu.py holds these
to oracle/preproc_ref.py, to the recorded fixture and to their own mutants).

Written from what the library documents (include/mi3d.h "Input pipeline", preprocess.py), not from the kernels:

  ct(x, lo, hi)       clip to the window, (v - lo) / (hi - lo), float64
  mri(x, p_low, p_high)
      mean = float32(mean64(x));  sd = float32(sqrt(mean64((x - mean)^2))) + float32(1e-8)      (that addition in float32)
      z    = (x - mean) / sd in float32
      order statistics of z from np.sort; virtual index q / 100 * (n - 1) = floor rank k + fraction g (np.percentile,
      method 'linear'); low / high = float32(a + (b - a) * g) evaluated in float64
      out  = (clip(z, low, high) - low) / (high - low + 1e-8) in float64
  remap(label, kind)  kind 0 identity, 1 the AMOS table, 2 the CHAOS grey-value ranges, on int64

`mri` also takes the two mutants the CPU self-test uses to show that the GPU comparison would notice them: a floor rank
moved by a few places (`rank_shift`) and the interpolation weight g replaced by 1 - g (`flip_weight`).

The input builders return shuffled float32 vectors.  What makes a rank error visible is the gap between neighbouring order
statistics relative to high - low; smooth data lose it as n grows (a gap is ~1 / n of the range), `pedestal` keeps it at
any n by putting all but 4w values into three ties and a ladder of 2w well-separated rungs around either percentile."""
import collections

import numpy as np

CT_WINDOW = (-160.0, 240.0)
CT_WINDOWS = (CT_WINDOW, (-100.0, 300.5))
CT_SIZES = (1, 255, 257, 524291)
REMAP_SIZES = (1, 317, 524291)
MRI_ATOL = 1e-6               # GPU kernel against mri(); see test_gpu_preproc_ops.py
ORACLE_ATOL = 2.5e-7          # float32 numpy oracle against mri(): a condition on the inputs
MUTANT_MOVES = 1e-3           # what a mutant has to move the output by, at least


# ------------------------------------------------------------------------------------------------------------- models
def ct(x, lo=CT_WINDOW[0], hi=CT_WINDOW[1]):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    v = np.clip(np.asarray(x, np.float32).astype(np.float64), lo, hi)
    return (v - lo) / (hi - lo)


def zscore(x):
    """(z, mean, sd) of the MRI model: float64 moments rounded to float32, float32 z."""
    x = np.asarray(x, np.float32).ravel()
    mean = np.float32(np.mean(x.astype(np.float64)))
    var = np.mean((x.astype(np.float64) - np.float64(mean)) ** 2)
    sd = np.float32(np.float32(np.sqrt(var)) + np.float32(1e-8))
    z = ((x - mean) / sd).astype(np.float32)
    return z, mean, sd


def ranks(n, q):
    """Floor rank and fraction of np.percentile's virtual index q / 100 * (n - 1); q is a float32 value like the ABI's."""
    v = float(np.float32(q)) / 100.0 * (n - 1)
    k = int(np.floor(v))
    return k, v - k


def mri(x, p_low=1.0, p_high=99.0, rank_shift=(0, 0), flip_weight=False, prepared=None):
    """Returns (out float64, low, high, (k_low, k_high), (g_low, g_high)).  `prepared` = (z, np.sort(z)) of the same x
    saves the sort when one input is evaluated several times."""
    z, s = prepared if prepared is not None else prepare(x)
    n = z.size
    bounds, ks, gs = [], [], []
    for q, shift in ((p_low, rank_shift[0]), (p_high, rank_shift[1])):
        k, g = ranks(n, q)
        kf = min(max(k + shift, 0), n - 1)
        kc = min(kf + 1, n - 1)
        w = 1.0 - g if flip_weight else g
        a, b = float(s[kf]), float(s[kc])
        bounds.append(np.float32(a + (b - a) * w))
        ks.append(k)
        gs.append(g)
    low, high = bounds
    z64 = z.astype(np.float64)
    out = (np.clip(z64, float(low), float(high)) - float(low)) / (float(high) - float(low) + 1e-8)
    return out, low, high, tuple(ks), tuple(gs)


def prepare(x):
    z = zscore(x)[0]
    return z, np.sort(z)


def rank_mutants(n, p_low, p_high):
    """The rank shifts (d_low, d_high) by one place that the clamp to [0, n - 1] does not undo."""
    out = []
    for side, q in ((0, p_low), (1, p_high)):
        k = ranks(n, q)[0]
        for d in (-1, 1):
            if min(max(k + d, 0), n - 1) != k:
                out.append((d, 0) if side == 0 else (0, d))
    return out


def weight_mutant_counts(g):
    """The flipped weight is only held to MUTANT_MOVES where g is not within 0.05 of 0, 0.5 or 1 (|1 - 2g| >= 0.1)."""
    return all(abs(g - c) > 0.05 + 1e-9 for c in (0.0, 0.5, 1.0))


def compare(got, want):
    """The comparison both test files make: max |delta| and whether the voxels clipped at either end are the same."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    delta = float(np.abs(got.astype(np.float64) - want).max())
    same_low = np.array_equal(got == got.min(), want == want.min())
    same_high = np.array_equal(got == got.max(), want == want.max())
    return delta, same_low, same_high


AMOS_TABLE = {0: 0, 1: 1, 2: 3, 3: 3, 6: 2}                                  # spleen 1, kidneys 2 | 3 -> 3, liver 6 -> 2, else 0
CHAOS_RANGES = (((55, 70), 2), ((110, 135), 3), ((175, 200), 3), ((240, 255), 1))   # liver, right / left kidney, spleen, else 0


def remap(label, kind):
    label = np.asarray(label, np.int64)
    if kind == 0:
        return label.copy()
    out = np.zeros_like(label)
    if kind == 1:
        for old, new in AMOS_TABLE.items():
            out[label == old] = new
    elif kind == 2:
        for (lo, hi), new in CHAOS_RANGES:
            out[(label >= lo) & (label <= hi)] = new
    else:
        raise ValueError(kind)
    return out


def remap_values():
    """Every integer of [-8, 300] and the int64 extremes a 32-bit truncation would fold onto a class."""
    extra = [2 ** 31 - 1, 2 ** 31, 2 ** 32 + 1, 2 ** 32 + 6, 2 ** 32 + 60, -(2 ** 32) + 1, np.iinfo(np.int64).min,
             np.iinfo(np.int64).max]
    return np.concatenate([np.arange(-8, 301, dtype=np.int64), np.array(extra, np.int64)])


def remap_input(n, seed):
    """n labels: the whole value set first (as far as it fits), random members of it after."""
    vals = remap_values()
    rng = np.random.default_rng(seed)
    out = vals[rng.integers(0, vals.size, n)]
    m = min(n, vals.size)
    out[:m] = rng.permutation(vals)[:m]
    return out


def okey(z):
    """Order-preserving 32-bit key of a float32: sign bit flipped for positives, all bits for negatives."""
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def shared_key_bytes(a, b):
    """How many leading key bytes two float32 values share (0..4)."""
    ka, kb = (int(okey(np.array([v], np.float32))[0]) for v in (a, b))
    n = 0
    for shift in (24, 16, 8, 0):
        if (ka >> shift) != (kb >> shift):
            break
        n += 1
    return n


# ------------------------------------------------------------------------------------------------------------- inputs
def ladder(n, kind, seed=0):
    """n distinct values.  'lin': equal steps; 'geo': signed geometric spacing +-exp(U(-3, 9))."""
    rng = np.random.default_rng(seed)
    if kind == "lin":
        x = ((np.arange(n, dtype=np.float64) - 0.3 * n) * 0.37).astype(np.float32)
    elif kind == "geo":
        x = (rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(-3.0, 9.0, n))).astype(np.float32)
    else:
        raise ValueError(kind)
    assert np.unique(x).size == n
    return rng.permutation(x)


def background(n, seed=0):
    """40 % exact zeros (air) and a gamma foreground: the low percentile falls inside a long tie."""
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, 120.0, n).astype(np.float32) + np.float32(1.0)
    x[:(2 * n) // 5] = 0.0
    return rng.permutation(x)


def pedestal(n, p_low, p_high, w=16, seed=0):
    """Sorted: a tie at -900 | 2w rungs -800 + 20 i + U(0, 10) around the low rank | a tie at 100 | 2w rungs
    300 + 20 i + U(0, 10) around the high rank | a tie at 5000.  Neighbouring rungs are 10 to 30 apart whatever n."""
    rng = np.random.default_rng(seed)
    k0, k1 = ranks(n, p_low)[0], ranks(n, p_high)[0]
    a0 = min(max(k0 - w + 1, 0), n - 2 * w)
    b0 = min(max(k1 - w + 1, 0), n - 2 * w)
    assert b0 >= a0 + 2 * w, "the two ladders overlap: n too small for these percentiles"
    s = np.empty(n, np.float64)
    s[:a0] = -900.0
    s[a0:a0 + 2 * w] = -800.0 + 20.0 * np.arange(2 * w) + rng.uniform(0.0, 10.0, 2 * w)
    s[a0 + 2 * w:b0] = 100.0
    s[b0:b0 + 2 * w] = 300.0 + 20.0 * np.arange(2 * w) + rng.uniform(0.0, 10.0, 2 * w)
    s[b0 + 2 * w:] = 5000.0
    x = s.astype(np.float32)
    assert np.all(np.diff(x[a0:a0 + 2 * w]) >= 10.0) and np.all(np.diff(x[b0:b0 + 2 * w]) >= 10.0)
    return rng.permutation(x)


def straddle(n=202, seed=0):
    """Three far-negative outliers and n - 3 distinct values of [10, 20]: the order statistics under the 1st percentile
    (ranks 2 and 3 at n = 202) have z-scores of opposite sign, so their keys differ in the top bit."""
    rng = np.random.default_rng(seed)
    m = n - 3
    pos = 10.0 + 10.0 * (np.arange(m) + rng.uniform(0.0, 0.5, m)) / m
    x = np.concatenate([np.array([-1000.0, -990.0, -980.0]) + rng.uniform(0.0, 1.0, 3), pos]).astype(np.float32)
    assert np.unique(x).size == n
    s = np.sort(zscore(x)[0])
    k = ranks(n, 1.0)[0]
    assert s[k] < 0.0 < s[k + 1], "the low pair does not straddle zero"
    return rng.permutation(x)


def signed_zeros(seed=0):
    """1001 small integers, symmetric about zero (so the mean is exactly 0 in any summation order), 200 of them -0.0 and
    201 +0.0: z holds zeros of both signs, which compare equal and have different keys."""
    rng = np.random.default_rng(seed)
    side = np.arange(1, 301, dtype=np.float32)
    x = np.concatenate([-side, np.full(200, -0.0, np.float32), np.zeros(201, np.float32), side])
    z = zscore(x)[0]
    zero = z == 0.0
    assert np.signbit(z[zero]).any() and not np.signbit(z[zero]).all()
    return rng.permutation(x)


# -------------------------------------------------------------------------------------------------------------- cases
# One list for both test files.  mutants: which reference mutants the CPU self-test holds to MUTANT_MOVES on this input.
#   'all'  rank shifts and the flipped weight (pedestal: rungs >= 10 apart, high - low <= 1730 raw units; geometric ladder)
#   'rank' rank shifts only: on an equal-step ladder one rank is worth 1 / (0.98 (n - 1)) of the output range whatever its
#          scale, 1.02e-3 at n = 1000 and 2.5e-4 at n = 4097, and the flipped weight |1 - 2g| of that: 4.8e-4 at n = 257
#          (g = 0.56), the one ladder size whose g is more than 0.05 away from 0, 0.5 and 1
#   'none' inputs that are there for another reason (ties at the percentile, key bytes) and hide a rank by construction
Case = collections.namedtuple("Case", "id builder args n p_low p_high mutants")

LADDER_SIZES = (2, 3, 101, 102, 201, 255, 256, 257, 1000, 4097)
PEDESTAL_SIZES = (4097, 65537, 262147, 524291, 1048583)        # the last three pass 1024 x 256 (sums, histograms) and 2048 x 256 (apply)
PEDESTAL_PAIRS = ((1.0, 99.0), (0.5, 99.5), (25.0, 75.0), (2.5, 97.5))
DENSE_LADDER = 1048583                                         # equal steps close enough to share three key bytes


def _cases():
    out = []
    for n in LADDER_SIZES:
        # n = 2, 3 are there for the clamped ranks: at most one voxel lies between the bounds (none at n = 2, and the middle
        # one of three geometric values need not sit where it shows)
        out.append(Case(f"ladder-lin-{n}", "ladder", ("lin",), n, 1.0, 99.0, "rank" if 3 <= n <= 1000 else "none"))
        out.append(Case(f"ladder-geo-{n}", "ladder", ("geo",), n, 1.0, 99.0, "all" if 101 <= n <= 1000 else "none"))
    out.append(Case(f"ladder-lin-{DENSE_LADDER}", "ladder", ("lin",), DENSE_LADDER, 1.0, 99.0, "none"))
    for n in PEDESTAL_SIZES:
        for pl, ph in PEDESTAL_PAIRS + (((0.0, 100.0),) if n <= 4097 else ()):
            out.append(Case(f"pedestal-{n}-{pl:g}-{ph:g}", "pedestal", (pl, ph), n, pl, ph, "all"))
    for n in (4097, 262147):
        out.append(Case(f"background-{n}", "background", (), n, 1.0, 99.0, "none"))
    out.append(Case("straddle-202", "straddle", (), 202, 1.0, 99.0, "none"))
    out.append(Case("signed-zeros-1001", "signed_zeros", (), 1001, 35.0, 85.0, "none"))
    return out


MRI_CASES = _cases()
_BUILDERS = {"ladder": ladder, "pedestal": pedestal, "background": background, "straddle": straddle,
             "signed_zeros": signed_zeros}


def build(case, seed=0):
    if case.builder == "signed_zeros":
        x = signed_zeros(seed)
    elif case.builder == "pedestal":
        x = pedestal(case.n, *case.args, seed=seed)
    elif case.builder == "ladder":
        x = ladder(case.n, *case.args, seed=seed)
    else:
        x = _BUILDERS[case.builder](case.n, seed=seed)
    assert x.dtype == np.float32 and x.size == case.n
    return x


def ct_input(n, lo, hi, seed=0):
    """Values at, just inside and just outside both window edges, +-inf, a spread over many magnitudes, and normal HU."""
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(lo), np.float32(hi)
    inf = np.float32(np.inf)
    edge = np.array([lo, np.nextafter(lo, inf), np.nextafter(lo, -inf), hi, np.nextafter(hi, inf), np.nextafter(hi, -inf), inf,
                     -inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-40, -1e-40], np.float32)
    x = rng.normal(40.0, 250.0, n).astype(np.float32)
    m = n // 4
    x[:m] = (rng.choice([-1.0, 1.0], m) * np.exp(rng.uniform(-20.0, 80.0, m))).astype(np.float32)
    x = rng.permutation(x)
    k = min(n, edge.size)
    x[:k] = edge[:k]
    return x
