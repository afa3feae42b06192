"""float64 reference for the inference forward's folded-BatchNorm conv routes (one half of a DoubleConv block through
mi3d_conv3_infer_forward), the case table of tests/test_gpu_conv_infer_ops.py and the route the plan's conv3_bn_half_infer gives
each case.  Rounding helpers, the convolution, the route predicates and the dyadic draws are those of tests/conv_ref.py.

    scale = gamma / sqrt(running_var + eps)        fbias = (bias - running_mean) * scale + beta
    z     = relu(conv(x, w * scale) + fbias)

Exact inputs (every bitwise case): eps = 0, running_var in {1/4, 1, 4}, gamma = s * sqrt(running_var) with s in
{+-1/2, 3/4, +-1, 5/4, +-3/2, 2}, so scale = s exactly; running_mean in k/4 (|k| <= 8), beta in k/8 (|k| <= 8); x in k/8, w in k/16,
bias in k/4 (|k| <= 8, no offset).  w * scale = (k/16) * s has at most 4 + 3 = 7 significant bits: a bf16 number, so the bf16 weight
image is exact.  fbias is a multiple of 1/16 below 16: exact in fp32.  A product x * (w * scale) is a multiple of 1/512 (s is a
multiple of 1/4), so with

    512 * (sum|x * w * scale| + |fbias|) < 2^24        at every output            (4 * exactness_margin)

every partial sum, in any order and under any K split, is exact in fp32; the accumulator a kernel rounds is the exact value and
the stored bf16 is its round-to-nearest-even image after the ReLU, bit for bit."""
import functools

import numpy as np

import conv_ref as R

EPS_REAL = float(np.float32(1e-5))       # the entry takes eps as a C float: the reference folds with that float's value
SCALES = np.array([-0.5, 0.5, 0.75, -1.0, 1.0, 1.25, -1.5, 1.5, 2.0])
VARS = np.array([0.25, 1.0, 4.0])


# ------------------------------------------------------------------------------------------------ the operation
def fold_f64(gamma, beta, rm, rv, bias, eps):
    """(scale, fbias) in float64; bias None = no conv bias"""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    scale = f(gamma) / np.sqrt(f(rv) + np.float64(eps))
    b = f(bias) if bias is not None else np.zeros_like(scale)
    return scale, (b - f(rm)) * scale + f(beta)


def conv_folded_f64(x, w, scale, fbias):
    """conv(x, w * scale) + fbias, NCDHW, float64: the value in front of the ReLU"""
    return R.conv3d_f64(x, np.asarray(w, np.float64) * np.asarray(scale, np.float64).reshape(-1, 1, 1, 1, 1),
                        np.array(fbias, np.float64))


def infer_f64(x, w, scale, fbias):
    return np.maximum(conv_folded_f64(x, w, scale, fbias), 0.0)


def abs_sum_f64(x, w, scale):
    """sum|x * w * scale| per output: what the rounding of the weights and the fp32 accumulation scale with"""
    return conv_folded_f64(np.abs(x), np.abs(w), np.abs(scale), np.zeros(len(scale)))


# ------------------------------------------------------------------------------------------------ the route
def predict_infer_route(case, routes=None, zcs=None):
    """(conv, ksplit) of mi3d_conv3_infer_route: the conv codes of mi3d_conv3_bn_route.  The split-K scratch is handed over only
    to an output whose rows are 16-byte aligned (zcs % 8 == 0); without it a small-geometry layer runs a single pass."""
    r = dict(R.DEFAULT_ROUTES, **(routes or {}))
    cin, cout, g, bf = case["cin"], case["cout"], case["geo"], case["dtype"] == 1
    zcs = cout if zcs is None else zcs
    if bf and cin % 16 == 0 and cout % 16 == 0 and cin >= 16:
        if R.persist_ok(cin, cout, g, r):
            return (2, 1)
        if R.big_geo(g):
            return (3, 1)
        return (4, R.pick_ksplit(cin, cout, g) if zcs % 8 == 0 else 1)
    if bf and cin == 1 and cout % 16 == 0:
        return (1, 1)
    return (0, 1)


# ------------------------------------------------------------------------------------------------ the case table
def _geo(name):
    c = R.CASES[name]
    return dict(cin=c["cin"], cout=c["cout"], geo=c["geo"], dtype=c["dtype"])


def _case(base, route, data=None, planar=False, **over):
    return dict(_geo(base), **over, route=route, data=data, planar=planar)


# name: the shape of the conv_ref case of that name (the smallest that reaches the route, ragged on purpose) and the route
# (conv, ksplit) the default switches must give it.  data: the case whose inputs and reference this one shares.
CASES = {
    "c1_16":                 _case("c1_16", (1, 1)),                       # fp32 image in
    "c1_32":                 _case("c1_32", (1, 1)),
    "persist_thin":          _case("persist_thin", (2, 1)),
    "persist_2chunk":        _case("persist_2chunk", (2, 1)),              # two K chunks
    "persist_2chunk_planar": _case("persist_2chunk", (2, 1), data="persist_2chunk", planar=True),      # x in two [M][16] planes
    "big_16_32":             _case("big_16_32", (3, 1)),                   # 16-byte store
    "big_32_32":             _case("big_32_32", (3, 1)),
    "big_64_16":             _case("big_64_16", (3, 1)),                   # one output block: 8-byte store
    "small_16_32":           _case("small_16_32", (4, 1)),
    "small_tiny":            _case("small_tiny", (4, 1)),
    "sk2_32_64":             _case("sk2_32_64", (4, 2)),                   # stand-alone split-K finish with ReLU
    "sk2_32_16":             _case("sk2_32_16", (4, 2)),
    "sk4_64_128":            _case("sk4_64_128", (4, 4)),
    "sk8_128_256":           _case("sk8_128_256", (4, 8)),
    "sk16_256_256":          _case("sk16_256_256", (4, 16)),
    "direct_f32":            _case("direct_f32", (0, 1)),
    "direct_bf16":           _case("direct_f32", (0, 1), cin=2, dtype=1),  # the direct kernel with bf16 in and out
}
PERSIST_CASES = [k for k, c in CASES.items() if c["route"][0] == 2]
TILE_CASES = [k for k, c in CASES.items() if c["route"][0] in (3, 4)]
SPLITK_CASES = [k for k, c in CASES.items() if c["route"][1] > 1]
# name -> seed, where the default (the name's letters) misses a condition of the CPU test: five channels are few draws, and the
# defaults left 18 % (direct_f32) and 28 % (direct_bf16) of the outputs on one side of zero
SEEDS = {"direct_f32": 2, "direct_bf16": 1}


def draw_fold_exact(rng, cout):
    rv = rng.choice(VARS, cout)
    s = rng.choice(SCALES, cout)
    gamma = s * np.sqrt(rv)
    rm = rng.integers(-8, 9, cout) / 4
    beta = rng.integers(-8, 9, cout) / 8
    return tuple(a.astype(np.float32) for a in (gamma, beta, rm, rv))


def _freeze(k):
    for v in k.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Exact inputs and the float64 reference of one case; computed once, read-only.  pre = the value in front of the ReLU."""
    c = CASES[name]
    if c["data"]:
        return _freeze(dict(case_data(c["data"]), **c, name=name))
    n, d, h, w = c["geo"]
    cin, cout = c["cin"], c["cout"]
    rng = np.random.default_rng(SEEDS.get(name, 1000 + sum(map(ord, name))))
    x, wgt, b = R.dyadic_conv_inputs(rng, n, cin, cout, d, h, w, offset=False)
    gamma, beta, rm, rv = draw_fold_exact(rng, cout)
    scale, fbias = fold_f64(gamma, beta, rm, rv, b, 0.0)
    pre = conv_folded_f64(x, wgt, scale, fbias)
    return _freeze(dict(c, name=name, x=x, w=wgt, b=b, gamma=gamma, beta=beta, rm=rm, rv=rv, eps=0.0, scale=scale, fbias=fbias,
                        pre=pre, exact=np.maximum(pre, 0.0)))


# ------------------------------------------------------------------------------------------------ the fold with the real eps
REAL_CASES = ("persist_thin", "sk4_64_128", "direct_f32")


def draw_fold_real(rng, cout, with_bias=True):
    """random statistics: running_var uniform in [0.05, 4] with one channel at 0.0 exactly (scale = gamma / sqrt(eps))"""
    rv = rng.uniform(0.05, 4.0, cout).astype(np.float32)
    rv[int(rng.integers(0, cout))] = 0.0
    gamma = ((rng.random(cout) + 0.5) * np.where(rng.random(cout) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = (rng.standard_normal(cout) * 0.3).astype(np.float32)
    rm = (rng.standard_normal(cout) * 0.5).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.5).astype(np.float32) if with_bias else None
    return gamma, beta, rm, rv, bias


@functools.lru_cache(maxsize=None)
def real_case_data(name):
    """Normal x (bf16 numbers where the layer reads bf16), normal weights, random statistics, eps = 1e-5: the float64 reference and
    the derived per-element bound of |z - infer_f64|:
        (2^-9 + (27*Cin + 3) * 2^-24) * sum|x*w*scale|      bf16 rounding of w*scale (not for fp32) + fp32 accumulation
      + 2^-23 * |fbias|
      + half a bf16 spacing at |ref| + that                 (bf16 outputs only)"""
    c = CASES[name]
    n, d, h, w = c["geo"]
    cin, cout, bf = c["cin"], c["cout"], c["dtype"] == 1
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    x = rng.standard_normal((n, cin, d, h, w)).astype(np.float32)
    if bf:
        x = R.bf16_rne(x)
    wgt = (rng.standard_normal((cout, cin, 3, 3, 3)) * 0.1).astype(np.float32)
    gamma, beta, rm, rv, b = draw_fold_real(rng, cout)
    scale, fbias = fold_f64(gamma, beta, rm, rv, b, EPS_REAL)
    ref = infer_f64(x, wgt, scale, fbias)
    bound = ((2.0 ** -9 if bf else 0.0) + (27 * cin + 3) * 2.0 ** -24) * abs_sum_f64(x, wgt, scale) + \
        2.0 ** -23 * np.abs(fbias).reshape(1, -1, 1, 1, 1)
    if bf:
        bound = bound + half_spacing(np.abs(ref) + bound)
    return _freeze(dict(c, name=name, x=x, w=wgt, b=b, gamma=gamma, beta=beta, rm=rm, rv=rv, eps=EPS_REAL, scale=scale, fbias=fbias,
                        exact=ref, bound=bound))


def half_spacing(a):
    """half the distance between neighbouring bf16 numbers at magnitude a (8 significant bits): 2^(floor(log2 a) - 8); 0 at 0"""
    a = np.abs(np.asarray(a, np.float64))
    return np.where(a > 0, np.exp2(np.floor(np.log2(np.maximum(a, 1e-300))) - 8), 0.0)


def f32_neighbours(v):
    """float32(v) and its two fp32 neighbours, as a [3][...] float32 array"""
    c = np.asarray(v, np.float64).astype(np.float32)
    return np.stack([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))])
