"""float64 reference for the decoder's up step (ConvTranspose3d(k=2, s=2) into the up half of a concat buffer, nearest resize where the
skip is larger), the case table of tests/test_gpu_up_ops.py, and a plain-Python restatement of the launch predicates of
upconv_mfma.hip / upconv.hip / pool.hip that says where each case's shape lands.

The operation is a per-voxel GEMM (ci) x (co, tap) followed by a 2x2x2 pixel shuffle; the reference is that matmul in float64.
The resize reference is torch.nn.functional.interpolate(mode="nearest") and its autograd adjoint on CPU tensors (see nearest_f64).

Dyadic inputs: x and gy in k/8, w in k/16, bias in k/4, all |k| <= 8; dW0 in k/16 and db0 in k/4 for accumulate = 1.  Every
product x*w and gy*w is a multiple of 1/128, every x*gy a multiple of 1/64, every gy a multiple of 1/8, so with

    128 * (|b| + sum|x*w|) < 2^24 at every y,   128 * sum|gy*w| < 2^24 at every dx,
    64 * (|dW0| + sum|x*gy|) < 2^24 at every weight,   8 * (|db0| + sum|gy|) < 2^24                      (exactness_margins)

every partial sum the kernels can form -- per MFMA, per wave, per workgroup, per slab, in any order -- is an integer multiple of
its unit below 2^24 units: exact in fp32.  y and dx are then bf16_rne(exact) bit for bit, dW and db the exact values.

Non-dyadic runs use conv_bwd_ref.acc_bound / half_spacing with n = Cin (y), 8 * Cout (dx), M (dW), 8 * M (db)."""
import functools

import numpy as np
import torch

from conv_ref import bf16_rne, cdiv  # noqa: F401

UV_MFMA, UV_DIRECT, CB_DIRECT = 128, 32, 32
DEFAULT_ROUTES = dict(no_fused_upbwd=0, no_upbwd_carry=0)
FWD_KEYS = ("kind", "gy", "tap_split", "wide", "strided", "resized")
BWD_KEYS = ("kind", "ksplit", "persistent", "slabs", "slab_ew", "wgrad_blocks", "dgrad_blocks", "pending", "resized")
LEAVE_PENDING, SECOND_WORKSPACE = 1, 2


# ------------------------------------------------------------------------------------------------ the operation
def _xm(x):
    n, c, d, h, w = x.shape
    return np.asarray(x, np.float64).transpose(0, 2, 3, 4, 1).reshape(-1, c)


def _gm(gy):
    """(N, Cout, 2D, 2H, 2W) -> [M][(co, a, b, c)]: the inverse pixel shuffle"""
    n, co, d2, h2, w2 = gy.shape
    g = np.asarray(gy, np.float64).reshape(n, co, d2 // 2, 2, h2 // 2, 2, w2 // 2, 2)
    return g.transpose(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, co * 8)


def convT2_f64(x, w, b=None):
    """ConvTranspose3d(k=2, s=2), NCDHW, float64: one matmul (ci) x (co, tap) and the pixel shuffle.  w (Cin, Cout, 2, 2, 2)"""
    n, cin, d, h, wd = x.shape
    cout = w.shape[1]
    o = _xm(x) @ np.asarray(w, np.float64).reshape(cin, cout * 8)
    o = o.reshape(n, d, h, wd, cout, 2, 2, 2).transpose(0, 4, 1, 5, 2, 6, 3, 7).reshape(n, cout, 2 * d, 2 * h, 2 * wd)
    return o if b is None else o + np.asarray(b, np.float64).reshape(1, -1, 1, 1, 1)


def convT2_bwd_f64(x, w, gy, need_dx=True):
    """dx (None if not needed), dW, db of convT2_f64"""
    n, cin, d, h, wd = x.shape
    cout = w.shape[1]
    gm = _gm(gy)
    dx = None
    if need_dx:
        dx = (gm @ np.asarray(w, np.float64).reshape(cin, cout * 8).T).reshape(n, d, h, wd, cin).transpose(0, 4, 1, 2, 3)
    dW = (_xm(x).T @ gm).reshape(cin, cout, 2, 2, 2)
    return dx, dW, np.asarray(gy, np.float64).sum(axis=(0, 2, 3, 4))


# torch computes the source index of a nearest resize in the arithmetic of the tensor: float for float32 / bfloat16 tensors -- what the
# model runs and what pool.hip restates -- and double for float64 tensors.  The two differ where dst * in / out is an integer that
# float arithmetic just misses ((in, out) = (24, 74), dst 37: 11 in float, 12 in double; test_up_ref_cpu.py pins that).  The
# reference therefore runs F.interpolate and its autograd adjoint on float32 CPU tensors and returns float64: the resize copies, and
# the adjoint adds at most a few dozen dyadic values, so float32 holds every value of the tests exactly (the callers assert it).
def _exact_f32(a):
    a = np.asarray(a, np.float64)
    f = a.astype(np.float32)
    assert (f.astype(np.float64) == a).all(), "the resize reference needs values float32 holds exactly"
    return torch.from_numpy(f)


def nearest_f64(x, size):
    """F.interpolate(x, size=size, mode="nearest") with the float-tensor index map (NCDHW array in, float64 array out)"""
    return torch.nn.functional.interpolate(_exact_f32(x), size=tuple(size), mode="nearest").numpy().astype(np.float64)


def nearest_bwd_f64(gy, in_size):
    """the adjoint of nearest_f64 by autograd: gradient with respect to an input of spatial size in_size.  Sums of at most
    prod(ceil(out / in) + 1) values; exact in float32 when they are small integers over a power of two (asserted: the float64 sum
    of |gy| over each source's destinations, times the grid, stays below 2^24)"""
    g = _exact_f32(gy)
    x = torch.zeros(g.shape[:2] + tuple(in_size), dtype=torch.float32, requires_grad=True)
    y = torch.nn.functional.interpolate(x, size=g.shape[2:], mode="nearest")
    y.backward(g)
    gx = x.grad.numpy().astype(np.float64)
    x2 = torch.zeros_like(x, requires_grad=True)
    torch.nn.functional.interpolate(x2, size=g.shape[2:], mode="nearest").backward(g.abs())
    assert float(x2.grad.max()) * 128.0 < 2.0 ** 24            # values are multiples of 1/128 at the finest
    return gx


def nearest_dests(n_in, n_out):
    """per source index, the destination indices torch's nearest resize of a float32 tensor reads it from (one axis)"""
    src = torch.nn.functional.interpolate(torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in), size=n_out, mode="nearest")
    src = src.reshape(-1).numpy().astype(np.int64)
    return [np.nonzero(src == i)[0] for i in range(n_in)]


def up_f64(x, w, b, size):
    y = convT2_f64(x, w, b)
    return y if tuple(size) == y.shape[2:] else nearest_f64(y, size)


def up_bwd_f64(x, w, gup, need_dx=True):
    d2 = tuple(2 * s for s in x.shape[2:])
    g = gup if gup.shape[2:] == d2 else nearest_bwd_f64(gup, d2)
    return convT2_bwd_f64(x, w, g, need_dx)


def exactness_margins(x, w, b, gy, dw0=None, db0=None):
    """(128 * max(|b| + sum|x*w|), 128 * max sum|gy*w|, 64 * max(|dW0| + sum|x*gy|), 8 * max(|db0| + sum|gy|)) from the data"""
    ax, aw, ag = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(gy, np.float64))
    y = convT2_f64(ax, aw, np.abs(b))
    dx, dW, db = convT2_bwd_f64(ax, aw, ag)
    dW = dW + (0 if dw0 is None else np.abs(dw0))
    db = db + (0 if db0 is None else np.abs(db0))
    return 128.0 * float(y.max()), 128.0 * float(dx.max()), 64.0 * float(dW.max()), 8.0 * float(db.max())


# ------------------------------------------------------------------------------------------------ the resize windows (pool.hip)
def nn_src(dst, scale, n_in):
    """nn_src of pool.hip in the kernel's float arithmetic: min(floor(fl32(dst) * scale), in - 1), scale = fl32(in) / fl32(out)"""
    s = int(np.floor(np.float32(dst) * scale))
    return min(s, n_in - 1)


def window_new(i, scale, n_in, n_out):
    """nn_window of pool.hip: [i / scale - 1, (i + 1) / scale + 1] in float, clipped; the last source index runs to out - 1"""
    lo = int(np.float32(i) / scale) - 1
    hi = n_out - 1 if i >= n_in - 1 else int(np.float32(i + 1) / scale) + 1
    return max(lo, 0), min(hi, n_out - 1)


def window_old(i, scale, n_in, n_out):
    """the window the adjoint used before: four candidates from i / scale - 1"""
    lo = int(np.float32(i) / scale) - 1
    return max(lo, 0), min(lo + 3, n_out - 1)


def gathered(window, n_in, n_out):
    """per source index, the destinations the adjoint kernel sums with the given candidate window and the nn_src filter"""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)      # nn_src of every destination
    out = []
    for i in range(n_in):
        lo, hi = window(i, scale, n_in, n_out)
        out.append(lo + np.nonzero(src[lo:hi + 1] == i)[0])
    return out


# ------------------------------------------------------------------------------------------------ launch predicates
def wave_grid(m):
    return max(1, min(4096, cdiv(m, 64)))


def mfma_supported(cin, cout, xcs, ycs):
    return (cin % 32 == 0 and cout % 16 == 0 and xcs % 8 == 0 and ycs % 8 == 0 and cin // 32 in (1, 2, 4, 8)
            and cout // 4 in (4, 8, 16, 32))


def _resized(g, go):
    return go is not None and tuple(go) != (2 * g[1], 2 * g[2], 2 * g[3])


def fwd_route(dt, cin, cout, g, go=None, xcs=None, ucs=None, aligned=True):
    """every forward field of mi3d_up_route.  g = (N, D, H, W) of the input; ucs / aligned: stride and 16-byte alignment of the up half"""
    m = g[0] * g[1] * g[2] * g[3]
    rs = _resized(g, go)
    xcs = cin if xcs is None else xcs
    ycs = cout if rs else (2 * cout if ucs is None else ucs)
    if rs:
        aligned = True                                   # the temporary
    if not (dt == 1 and mfma_supported(cin, cout, xcs, ycs)):
        return dict(kind=0, gy=cdiv(cout, 8), tap_split=0, wide=0, strided=0, resized=int(rs))
    gx, gy = wave_grid(m), 1
    while gx * gy < 512 and gy < cout // 16:
        gy *= 2
    gz = 8 if gx * gy < 512 and not (cin == 32 and cout == 16) else 1
    wide = gz == 1 and ycs % 8 == 0 and aligned
    return dict(kind=1, gy=gy, tap_split=int(gz == 8), wide=int(wide), strided=int(cdiv(m, 16) > gx * 4), resized=int(rs))


def slab_ew(sz, mfma):
    if mfma:
        return 8 if sz < 16384 else 32
    return 1 if sz < 128 else 4 if sz < 1024 else 8 if sz < 16384 else 32


def bwd_grids(cin, cout, g, fused=True):
    """the MFMA backward's grids: dict(ksp, nsb, wg=(x, y, z), dg=(x, y), persistent).  fused: the one-launch route (its caps)"""
    m = g[0] * g[1] * g[2] * g[3]
    gx, gy = wave_grid(m), 1
    while gx * gy < 512 and gy < cin // 16:
        gy *= 2
    gkx = cdiv(m, 16)
    ksp = gx * gy < 512 and cout // 4 >= 8 and gkx * (cin // 16) <= 8192
    nws = cin * cout * 8
    groups = (cin // 32) * cdiv(cout, 32)
    ntile = cdiv(m, UV_MFMA)
    if fused:
        wcap, dcap = (128 if nws >= 65536 else 192 if nws >= 16384 else 256), 256
        nsb = min(ntile, cdiv(wcap, groups))
        if not ksp and gx * gy > dcap:
            gx = max(1, dcap // gy)
    else:
        nsb = min(ntile, cdiv(512, groups))
    dg = (gkx, cin // 16) if ksp else (gx, gy)
    return dict(ksp=ksp, nsb=nsb, wg=(nsb, cin // 32, cdiv(cout, 32)), dg=dg, persistent=(not ksp) and gkx > dg[0] * 4)


def bwd_route(dt, cin, cout, g, go=None, xcs=None, gucs=None, dxcs=None, dx=True, dw=True, routes=None, flags=0):
    """every backward field of mi3d_up_route"""
    r = dict(DEFAULT_ROUTES, **(routes or {}))
    m = g[0] * g[1] * g[2] * g[3]
    rs = _resized(g, go)
    xcs = cin if xcs is None else xcs
    gcs = cout if rs else (2 * cout if gucs is None else gucs)
    dxcs = cin if dxcs is None else dxcs
    out = dict(kind=0, ksplit=0, persistent=0, slabs=0, slab_ew=0, wgrad_blocks=0, dgrad_blocks=0, pending=0, resized=int(rs))
    sz = cin * cout * 8 + cout
    if not (dt == 1 and mfma_supported(cin, cout, xcs, gcs) and (not dx or dxcs % 4 == 0)):
        nsb = min(cdiv(m, UV_DIRECT), cdiv(512, cdiv(cin, CB_DIRECT) * cdiv(cout, CB_DIRECT)))
        out.update(slabs=nsb, slab_ew=slab_ew(sz, False), wgrad_blocks=nsb * cdiv(cin, CB_DIRECT) * cdiv(cout, CB_DIRECT),
                   dgrad_blocks=cdiv(m, 256) * cdiv(cin, 8) if dx else 0)
        return out
    fused = dx and dw and not r["no_fused_upbwd"]
    q = bwd_grids(cin, cout, g, fused)
    out["kind"] = 1 if fused else 2 if (dx and dw) else 3 if dx else 4
    if dx:
        out.update(ksplit=int(q["ksp"]), persistent=int(q["persistent"]), dgrad_blocks=q["dg"][0] * q["dg"][1])
    if dw:
        out.update(slabs=q["nsb"], slab_ew=slab_ew(sz, True), wgrad_blocks=q["wg"][0] * q["wg"][1] * q["wg"][2])
        out["pending"] = int(bool(flags & LEAVE_PENDING))
    return out


def interleave(b, nw, nd, mutant=False):
    """upconv_mfma_bwd_fused_kernel's map from block index to (is weight-gradient block, index within its kind).  mutant: idx = b >> 1
    in the whole-groups range too (the mutation run of the pull request that added this file)"""
    m = min(nw, nd)
    m16 = (2 * m) & ~15
    if b < m16:
        xcd, k = b & 7, b >> 3
        return (k & 1) == 0, (b >> 1 if mutant else (k >> 1) * 8 + xcd)
    if b < 2 * m:
        return (b & 1) == 0, b >> 1
    return nw > nd, m + (b - 2 * m)


def interleave_ranges(nw, nd):
    """(blocks in whole groups of 16, blocks of the middle range, surplus blocks, which kind the surplus is)"""
    m = min(nw, nd)
    m16 = (2 * m) & ~15
    return m16, 2 * m - m16, nw + nd - 2 * m, ("w" if nw > nd else "d" if nd > nw else "")


# ------------------------------------------------------------------------------------------------ the case table
def _fwd(gy, tap_split=0, wide=1, strided=0, kind=1):
    return dict(kind=kind, gy=gy, tap_split=tap_split, wide=wide, strided=strided, resized=0)


def _bwd(kind, ksplit, persistent, slabs, ew, nw, nd):
    return dict(kind=kind, ksplit=ksplit, persistent=persistent, slabs=slabs, slab_ew=ew, wgrad_blocks=nw, dgrad_blocks=nd, pending=0,
                resized=0)


def _case(shape, fwd, bwd, dtype=1, seed=0, big_bias=False, oracle=False):
    n, cin, cout, d, h, w = shape
    return dict(cin=cin, cout=cout, geo=(n, d, h, w), dtype=dtype, fwd=fwd, bwd=bwd, seed=seed, big_bias=big_bias, oracle=oracle)


# name: (N, Cin, Cout, D, H, W) with the INPUT geometry, the forward route into an interleaved concat half (ucs = 2 Cout, 16-byte
# aligned) and the backward route of the fused launch, both under the default switches.  The smallest shapes that reach each
# branch, computed from the launchers; tests/test_up_ref_cpu.py re-derives every entry from the predicates above.
# big_bias: |bias| = 2 on every channel (K = 32 and 64: the sum of so few products alone rarely leaves the exactly representable
# range |y| < 2, and a bias drawn from all of k/4 does not move enough channels out of it).
CASES = {
    # hoist + wide, M % 16 = 2; backward S = 4 fused: middle range 4, data surplus 6
    "hoist_wide":      _case((2, 32, 16, 3, 5, 7), _fwd(1), _bwd(1, 0, 0, 2, 8, 2, 8), big_bias=True, oracle=True),
    # backward S = 4 persistent data loop (549 voxel groups on 128 x 4 waves); m16 = 128, middle range 10, M % 128 = 71
    "persist_s4":      _case((1, 32, 16, 13, 27, 25), _fwd(1), _bwd(1, 0, 1, 69, 8, 69, 256), big_bias=True),
    # forward tap split; backward S = 8 K-split, middle range 12, tails 7 / 7
    "tapsplit_ksp8":   _case((1, 64, 32, 9, 13, 11), _fwd(2, tap_split=1, wide=0), _bwd(1, 1, 0, 11, 32, 22, 324), big_bias=True),
    # forward wide, KS = 2, COBN = 2, no hoist, M % 16 = 1; backward S = 8 NOT K-split, persistent; slabs fused 96 / stand-alone 128
    "wide_ks2":        _case((1, 64, 32, 17, 31, 31), _fwd(2), _bwd(1, 0, 1, 96, 32, 192, 256), big_bias=True),
    # forward wide with the cob loop (gy = 1 < COBN = 2)
    "wide_cob_ks2":    _case((1, 64, 32, 33, 32, 32), _fwd(1), None, big_bias=True),
    # forward wide KS = 4 (gy = 4); backward S = 16 not K-split, persistent
    "wide_ks4":        _case((1, 128, 64, 19, 21, 21), _fwd(4), _bwd(1, 0, 1, 16, 32, 128, 256)),
    # forward wide KS = 8, gy = 8; backward S = 32 not K-split
    "wide_ks8":        _case((1, 256, 128, 13, 19, 17), _fwd(8), _bwd(1, 0, 1, 4, 32, 128, 256)),
    # forward wide KS = 8 with the cob loop (gy = 4 < 8)
    "wide_cob_ks8":    _case((1, 256, 128, 21, 20, 20), _fwd(4), None),
    # backward weight-gradient surplus (nw 32 > nd 16), K-split S = 32
    "wsurplus_ksp32":  _case((1, 256, 128, 2, 3, 2), _fwd(8, tap_split=1, wide=0), _bwd(1, 1, 0, 1, 32, 32, 16), oracle=True),
    # nw == nd: everything in the middle range; Cin = 32 with Cout = 128
    "middle_32_128":   _case((1, 32, 128, 2, 3, 5), _fwd(8, tap_split=1, wide=0), _bwd(1, 1, 0, 1, 32, 4, 4), big_bias=True, oracle=True),
    # Cout = 16 (one co block, second plane zero) with Cin / 32 > 1; slab sums of 32 and of 8 elements per block
    "cout16_cin128":   _case((1, 128, 16, 3, 5, 7), _fwd(1, tap_split=1, wide=0), _bwd(1, 0, 0, 1, 32, 4, 16), oracle=True),
    "cout16_cin64":    _case((1, 64, 16, 5, 7, 9), _fwd(1, tap_split=1, wide=0), _bwd(1, 0, 0, 3, 8, 6, 20), big_bias=True),
    # forward only: the grid-stride loop (gx = 4096, M = 266240) with wide + hoist
    "stride_hoist":    _case((1, 32, 16, 65, 64, 64), _fwd(1, strided=1), None, big_bias=True),
}
BWD_CASES = [k for k, c in CASES.items() if c["bwd"] is not None]
# the shapes of the non-dyadic runs
NORMAL_CASES = ("wide_ks2", "wsurplus_ksp32")

# direct kernels: (dtype, shape) -> what it reaches.  Forward route kind 0 with gy = ceil(Cout / 8); backward kind 0
DIRECT_CASES = {
    "f32_odd":      _case((2, 6, 3, 3, 2, 4), _fwd(1, wide=0, kind=0), _bwd(0, 0, 0, 2, 4, 2, 1), dtype=0, oracle=True),      # scalar paths
    "f32_tail":     _case((1, 24, 12, 4, 5, 3), _fwd(2, wide=0, kind=0), _bwd(0, 0, 0, 2, 8, 2, 3), dtype=0, oracle=True),     # 32-block tail
    "f32_two_ci":   _case((1, 40, 20, 3, 4, 5), _fwd(3, wide=0, kind=0), _bwd(0, 0, 0, 2, 8, 4, 5), dtype=0, oracle=True),     # 32 + 8
    "f32_tiles":    _case((1, 8, 4, 17, 31, 32), _fwd(1, wide=0, kind=0), _bwd(0, 0, 0, 512, 4, 512, 66), dtype=0),            # 527 tiles on 512
    "bf16_48_24":   _case((1, 48, 24, 5, 6, 7), _fwd(3, wide=0, kind=0), _bwd(0, 0, 0, 7, 8, 14, 6)),
    "bf16_96_48":   _case((1, 96, 48, 3, 4, 5), _fwd(6, wide=0, kind=0), _bwd(0, 0, 0, 2, 32, 12, 12)),
    "bf16_512_256": _case((1, 512, 256, 2, 2, 3), _fwd(32, wide=0, kind=0), _bwd(0, 0, 0, 1, 32, 128, 64)),
}

# the up step through a resize: (case shape, output geometry)
RESIZED_CASES = {
    "resized_32_16": ((1, 32, 16, 4, 3, 5), (9, 7, 11)),
    "resized_64_32": ((1, 64, 32, 4, 3, 5), (8, 7, 10)),
}


def dyadic_up_inputs(rng, n, cin, cout, d, h, w, big_bias=False):
    """x, gy in k/8, w in k/16, bias in k/4 (|k| = 8 with big_bias), dW0 in k/16, db0 in k/4; |k| <= 8 throughout"""
    x = rng.integers(-8, 9, (n, cin, d, h, w)).astype(np.float32) / 8
    wgt = rng.integers(-8, 9, (cin, cout, 2, 2, 2)).astype(np.float32) / 16
    b = rng.integers(-8, 9, cout).astype(np.float32) / 4
    if big_bias:
        b = np.where(rng.integers(0, 2, cout) > 0, 2.0, -2.0).astype(np.float32)
    gy = rng.integers(-8, 9, (n, cout, 2 * d, 2 * h, 2 * w)).astype(np.float32) / 8
    dw0 = rng.integers(-8, 9, wgt.shape).astype(np.float32) / 16
    db0 = rng.integers(-8, 9, cout).astype(np.float32) / 4
    return x, wgt, b, gy, dw0, db0


def all_cases():
    return dict(CASES, **DIRECT_CASES)


@functools.lru_cache(maxsize=None)
def case_data(name, need_ref=True):
    """Dyadic inputs and the float64 results of one case; computed once, read-only.  need_ref = False: inputs only (the
    grid-stride case, whose reference is one fp32 matmul in the test)."""
    c = all_cases()[name]
    n, d, h, w = c["geo"]
    rng = np.random.default_rng(sum(map(ord, name)) + 11 + c["seed"])
    x, wgt, b, gy, dw0, db0 = dyadic_up_inputs(rng, n, c["cin"], c["cout"], d, h, w, c["big_bias"])
    k = dict(c, name=name, x=x, w=wgt, b=b)
    if need_ref:
        k["y"] = convT2_f64(x, wgt, b)
        if c["bwd"] is not None:
            dx, dW, db = convT2_bwd_f64(x, wgt, gy)
            k.update(gy=gy, dw0=dw0, db0=db0, dx=dx, dW=dW, db=db)
    for v in k.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return k


def inexact_share(exact):
    """share of the values that are not bf16 numbers"""
    e = np.asarray(exact, np.float64)
    return float((bf16_rne(e.astype(np.float32)).astype(np.float64) != e).mean())
