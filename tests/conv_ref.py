"""float64 reference for the training forward's conv + BatchNorm-statistics routes (one half of a DoubleConv block), the case
table of tests/test_gpu_conv_fwd_ops.py, and a plain-Python restatement of the route predicates of conv3_mfma.hip / bn.hip /
plan.hip that says where each case's shape lands.

Inputs are the dyadic family of the per-operator conv tests: x in k/8, w in k/16, bias in k/4 (|k| <= 8), plus an integer
per-channel offset on the bias (|offset| <= 8) so that the channel means are not ~0.  Every product x*w is a multiple of
1/128 and the bias a multiple of 32/128, so with

    128 * sum|x*w| + 128 * |bias| < 2^24        at every output            (exactness_margin)

every partial sum, in any order and under any K split, is an integer multiple of 1/128 below 2^24/128: exact in fp32.  The
accumulator a kernel rounds is then the exact value, and the stored bf16 must be its round-to-nearest-even image, bit for bit.
Values of magnitude >= 2 that are odd multiples of 1/128 are not bf16 numbers (bf16 keeps 8 significant bits); in [2, 4) the odd
multiples of 1/128 are exact ties.  The BatchNorm statistics are those of the ROUNDED values."""
import functools

import numpy as np
import torch

EPS = 1e-5
MOMENTUM = 0.1
CUS = 256                    # compute units of an MI355X: the persistent grid is two workgroups per CU


# ------------------------------------------------------------------------------------------------ rounding
def bf16_bits(a):
    """float array -> uint16 bit patterns of round-to-nearest-even bf16 (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_rne(a):
    """float array -> float32 array of the bf16-rounded values."""
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(a))


def assert_bf16_rne_bits(stored, exact, what):
    """stored: channels-last bf16 tensor [N][D][H][W][C] (any device, any strides); exact: NCDHW array of the exact values.
    Every element's bit pattern must be that of round-to-nearest-even bf16 of the exact value: no tolerance."""
    got = stored.contiguous().view(torch.int16).cpu().numpy().transpose(0, 4, 1, 2, 3)
    want = bf16_bits(exact).view(np.int16).reshape(np.shape(exact))
    bad = got != want
    if bad.any():
        idx = np.argwhere(bad)[:8]          # (n, c, d, h, w) of the first mismatches
        vals = [(float(stored[i[0], i[2], i[3], i[4], i[1]]), float(np.asarray(exact)[tuple(i)])) for i in idx]
        raise AssertionError((what, "stored bf16 != bf16_rne(exact)", int(bad.sum()), idx.tolist(), vals))


def is_tie(a):
    """exactly halfway between two neighbouring bf16 numbers"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & 0xFFFF) == 0x8000


# ------------------------------------------------------------------------------------------------ the operation
def conv3d_f64(x, w, b):
    """Conv3d(k=3, p=1), NCDHW, in float64 (torch CPU).  On the dyadic inputs every sum is exact in float64 in any order."""
    y = torch.nn.functional.conv3d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)),
                                   torch.from_numpy(np.asarray(b, np.float64)), padding=1)
    return y.numpy()


def exactness_margin(x, w, b):
    """max over the outputs of 128 * sum|x*w| + 128 * |bias|; the bitwise claims need it below 2^24"""
    ones = np.zeros_like(np.asarray(b, np.float64))
    s = conv3d_f64(np.abs(x), np.abs(w), ones) + np.abs(np.asarray(b, np.float64)).reshape(1, -1, 1, 1, 1)
    return 128.0 * float(s.max())


def bn_stats_f64(y, gamma, beta, rm0, rv0, momentum=MOMENTUM, eps=EPS):
    """Train-mode BatchNorm3d statistics of y (NCDHW) in float64: mean, invstd, A = gamma*invstd, B = beta - mean*A, and the
    running buffers after one update (unbiased variance)."""
    y = np.asarray(y, np.float64)
    m = y.size // y.shape[1]
    mean = y.mean(axis=(0, 2, 3, 4))
    var = ((y - mean.reshape(1, -1, 1, 1, 1)) ** 2).mean(axis=(0, 2, 3, 4))
    inv = 1.0 / np.sqrt(var + eps)
    A = np.asarray(gamma, np.float64) * inv
    B = np.asarray(beta, np.float64) - mean * A
    rm = (1 - momentum) * np.asarray(rm0, np.float64) + momentum * mean
    rv = (1 - momentum) * np.asarray(rv0, np.float64) + momentum * var * m / max(m - 1, 1)
    return dict(mean=mean, var=var, inv=inv, A=A, B=B, rm=rm, rv=rv, sum=y.sum(axis=(0, 2, 3, 4)), sumsq=(y * y).sum(axis=(0, 2, 3, 4)))


def apply_f64(y, A, B, scale):
    """z = scale[n, c] * relu(A*y + B) in float64 (scale None = 1)"""
    z = np.maximum(np.asarray(y, np.float64) * A.reshape(1, -1, 1, 1, 1) + B.reshape(1, -1, 1, 1, 1), 0.0)
    return z if scale is None else z * np.asarray(scale, np.float64)[:, :, None, None, None]


# ------------------------------------------------------------------------------------------------ route predicates
def cdiv(a, b):
    return -(-a // b)


DEFAULT_ROUTES = dict(conv8=1, splitk_ticket=1, no_persist=0, wide_bn=3, no_small_bn=0)
SPLITK_TARGET, PERSIST_16_32_TILES, TK_COUNTERS = 128, 1024, 4096
SMALL_ROWS, WIDE_ROWS, WIDE_J, WNT, MAXC_BN, BN_BLK, BN_MAXBLK, SMALL_ELEMS = 128, 1024, 8, 1024, 256, 256, 1024, 2 << 20


def big_geo(g):
    return g[3] >= 32 and g[2] >= 16


def tiles16(g):              # 4 x 8 x 16 tiles
    return g[0] * cdiv(g[1], 4) * cdiv(g[2], 8) * cdiv(g[3], 16)


def tiles8(g):               # 4 x 8 x 8 tiles
    return g[0] * cdiv(g[1], 4) * cdiv(g[2], 8) * cdiv(g[3], 8)


def persist_ok(cin, cout, g, r):
    if (cin, cout) == (16, 32) and tiles16(g) < PERSIST_16_32_TILES:
        return False
    return big_geo(g) and (cin, cout) in ((16, 16), (32, 16), (16, 32)) and not r["no_persist"]


def workgroups8(cout, g):
    return tiles8(g) * (cout // (32 if cout % 32 == 0 else 16))


def pick_ksplit(cin, cout, g):
    if big_geo(g):
        return 1
    wgs, nchunk, k = workgroups8(cout, g), cin // 16, 1
    while wgs * k < SPLITK_TARGET and k * 2 <= nchunk and nchunk % (k * 2) == 0 and k < 16:
        k *= 2
    return k


def stat_blocks(cin, cout, g, r):
    if persist_ok(cin, cout, g, r):
        return min(tiles16(g), 2 * CUS)
    return tiles16(g) if big_geo(g) else tiles8(g)


def ticket_ok(cin, cout, g, r):
    if not r["splitk_ticket"] or not r["conv8"] or big_geo(g) or persist_ok(cin, cout, g, r):
        return False
    return pick_ksplit(cin, cout, g) > 1 and workgroups8(cout, g) <= TK_COUNTERS


def pow2(c):
    return c & (c - 1) == 0


def bn_small(c, m, r):
    return 4 <= c <= MAXC_BN and pow2(c) and m * c <= SMALL_ELEMS and not r["no_small_bn"]


def rows_route_ok(c, m, rows, r):
    if not (r["wide_bn"] & 1) or rows < 1 or m * c >= 1 << 31:
        return False
    if rows <= SMALL_ROWS:
        return 4 <= c <= MAXC_BN and pow2(c)
    return bool(r["wide_bn"] & 2) and rows <= WIDE_ROWS and 8 <= c <= MAXC_BN and pow2(c) and rows * c <= WIDE_J * WNT * 2


def predict_route(case, routes=None):
    """(conv, ksplit, ticket, stats, rows) of mi3d_conv3_bn_route for a case of the table under the given route switches, and the
    consumer of the rows ('thin' <= 128 rows, 'wide' up to 1024, 'finalize', '' none)."""
    r = dict(DEFAULT_ROUTES, **(routes or {}))
    cin, cout, g, bf = case["cin"], case["cout"], case["geo"], case["dtype"] == 1
    m = g[0] * g[1] * g[2] * g[3]
    mfma = bf and cin % 16 == 0 and cout % 16 == 0 and cin >= 16
    c1 = bf and cin == 1 and cout % 16 == 0
    conv, ks, tk, fused, rows = 0, 1, 0, False, 0
    if mfma:
        conv = 2 if persist_ok(cin, cout, g, r) else 3 if big_geo(g) else 4
        ks = 1 if conv == 2 else pick_ksplit(cin, cout, g)
        tk = int(ticket_ok(cin, cout, g, r))
        fused = bool(tk) or ks == 1
        rows = stat_blocks(cin, cout, g, r)
    elif c1:
        conv, fused, rows = 1, True, min(tiles16(g), 1024)
    if fused:
        ok = bf and rows_route_ok(cout, m, rows, r)
        return dict(conv=conv, ksplit=ks, ticket=tk, stats=1 if ok else 2, rows=rows,
                    consumer=("thin" if rows <= SMALL_ROWS else "wide") if ok else "finalize")
    small = bn_small(cout, m, r)
    if ks > 1:               # split-K partials finished by the statistics pass: one row per thread
        per_blk = BN_BLK // (cout // 8)
        nblk = min(cdiv(m, per_blk), BN_MAXBLK)
    else:                    # a statistics pass over y
        per_blk = BN_BLK // (cout // 8 if cout % 8 == 0 else cout)
        want = cdiv(m, per_blk * 4)
        if want < 256:
            want = min(cdiv(m, per_blk), 256)
        nblk = min(max(want, 1), BN_MAXBLK)
    rows = min(nblk, SMALL_ROWS) if small else 0
    return dict(conv=conv, ksplit=ks, ticket=0, stats=3 if ks > 1 else 0, rows=rows, consumer="thin" if small else "finalize")


# ------------------------------------------------------------------------------------------------ the case table
def _case(cin, cout, geo, conv, ksplit=1, ticket=0, stats=1, rows=0, consumer="thin", dtype=1, pooled=False, drop=False, oracle=True):
    return dict(cin=cin, cout=cout, geo=geo, dtype=dtype, pooled=pooled, drop=drop, oracle=oracle,
                route=dict(conv=conv, ksplit=ksplit, ticket=ticket, stats=stats, rows=rows, consumer=consumer))


# name: shape, and the route the DEFAULT switches must give it (conv, ksplit, ticket, stats, rows, who consumes the rows).
# oracle: small enough for the C oracle's scalar loops (the CPU test compares the float64 reference with it).
CASES = {
    "c1_16":          _case(1, 16, (2, 5, 9, 17), conv=1, rows=2 * 2 * 2 * 2),             # every mask of conv3_c1_fwd, W = 1 mod 16
    "c1_32":          _case(1, 32, (1, 6, 17, 35), conv=1, rows=2 * 3 * 3),                # second output block
    "persist_thin":   _case(16, 16, (1, 5, 17, 35), conv=2, rows=18),
    "persist_wide":   _case(16, 16, (2, 17, 33, 49), conv=2, rows=200, consumer="wide", oracle=False),
    "persist_2chunk": _case(32, 16, (1, 7, 18, 33), conv=2, rows=2 * 3 * 3),
    "persist_16_32":  _case(16, 32, (1, 61, 63, 130), conv=2, rows=512, consumer="wide", oracle=False),   # 1152 tiles >= 1024
    "big_16_32":      _case(16, 32, (1, 5, 17, 35), conv=3, rows=18),
    "big_32_32":      _case(32, 32, (2, 6, 17, 35), conv=3, rows=36),
    "big_64_16":      _case(64, 16, (1, 5, 16, 33), conv=3, rows=2 * 2 * 3),
    "small_16_32":    _case(16, 32, (2, 5, 9, 12), conv=4, rows=2 * 2 * 2 * 2),            # nchunk = 1: cannot split
    "small_tiny":     _case(16, 16, (1, 3, 5, 7), conv=4, rows=1),                         # volume smaller than one tile
    "small_finalize": _case(16, 16, (4, 37, 70, 30), conv=4, stats=2, rows=1440, consumer="finalize", oracle=False),
    "sk2_32_64":      _case(32, 64, (1, 5, 9, 12), conv=4, ksplit=2, ticket=1, rows=8),
    "sk2_32_16":      _case(32, 16, (1, 5, 9, 12), conv=4, ksplit=2, ticket=1, rows=8),
    "sk4_64_128":     _case(64, 128, (1, 6, 6, 6), conv=4, ksplit=4, ticket=1, rows=2),
    "sk4_256_256":    _case(256, 256, (2, 6, 6, 6), conv=4, ksplit=4, ticket=1, rows=4, pooled=True, oracle=False),
    "sk8_128_256":    _case(128, 256, (2, 3, 3, 3), conv=4, ksplit=8, ticket=1, rows=2),
    "sk16_256_256":   _case(256, 256, (1, 3, 3, 3), conv=4, ksplit=16, ticket=1, rows=1),
    "direct_f32":     _case(4, 5, (2, 5, 9, 17), conv=0, stats=0, rows=0, consumer="finalize", dtype=0),
    "persist_pool":   _case(16, 16, (2, 4, 16, 32), conv=2, rows=8, pooled=True, drop=True),
}
SPLITK_CASES = [k for k, c in CASES.items() if c["route"]["ksplit"] > 1]
PERSIST_CASES = [k for k, c in CASES.items() if c["route"]["conv"] == 2]
ONE_PASS_MFMA_CASES = [k for k, c in CASES.items() if c["route"]["conv"] in (3, 4) and c["route"]["ksplit"] == 1]
ROW_FED_CASES = [k for k, c in CASES.items() if c["route"]["stats"] == 1]


def dyadic_conv_inputs(rng, n, cin, cout, d, h, w, offset=True):
    x = rng.integers(-8, 9, (n, cin, d, h, w)).astype(np.float32) / 8
    wgt = rng.integers(-8, 9, (cout, cin, 3, 3, 3)).astype(np.float32) / 16
    b = rng.integers(-8, 9, cout).astype(np.float32) / 4
    if offset:
        b = b + rng.integers(-8, 9, cout).astype(np.float32)
    return x, wgt, b


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs and the float64 reference of one case; computed once, read-only."""
    c = CASES[name]
    n, d, h, w = c["geo"]
    cin, cout = c["cin"], c["cout"]
    rng = np.random.default_rng(sum(map(ord, name)))
    x, wgt, b = dyadic_conv_inputs(rng, n, cin, cout, d, h, w)
    gamma = ((rng.random(cout) + 0.5) * np.where(rng.random(cout) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = (rng.standard_normal(cout) * 0.3).astype(np.float32)
    rm0, rv0 = (rng.standard_normal(cout) * 0.1).astype(np.float32), (rng.random(cout) + 0.5).astype(np.float32)
    scale = None
    if c["drop"]:
        scale = (rng.random((n, cout)) >= 0.5).astype(np.float32) * 2.0
        scale[:, 0] = (0.0, 2.0)                 # the samples differ, whatever was drawn
    exact = conv3d_f64(x, wgt, b)
    y_ref = bf16_rne(exact) if c["dtype"] == 1 else exact.astype(np.float32)
    st = bn_stats_f64(y_ref, gamma, beta, rm0, rv0)
    k = dict(c, name=name, x=x, w=wgt, b=b, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, scale=scale, exact=exact, y_ref=y_ref,
             st=st, st_acc=bn_stats_f64(exact, gamma, beta, rm0, rv0), z_ref=apply_f64(y_ref, st["A"], st["B"], scale))
    for v in list(k.values()) + list(st.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return k
