"""float64 reference for the training backward's BatchNorm + conv routes (one half of a DoubleConv block), the case table of
tests/test_gpu_conv_bwd_ops.py, and a plain-Python restatement of the route predicates of conv3_mfma.hip / bn.hip / plan.hip
(conv3_bn_half_backward) that says where each case's shape lands.

Dyadic inputs: x in k/8, w in k/16, dy in k/8 with |k| <= 8 (|k| <= 4 for dy at the large shape).  Every product x*dy is a
multiple of 1/64, every dy*w a multiple of 1/128, every dy a multiple of 1/8, so with

    64 * sum|x*dy| < 2^24 at every weight,   128 * sum|dy*w| < 2^24 at every dx,   8 * sum|dy| < 2^24       (exactness_margins)

every partial sum -- per workgroup, per slab, per split-K part, in any order -- is an integer multiple of the unit below 2^24
units: exact in fp32.  dW and db are then the exact values, a dx left as split-K partials sums to the exact value, and a stored
bf16 dx is its round-to-nearest-even image, bit for bit.

Non-dyadic runs (BatchNorm on): the conv's gradients are compared with the float64 gradients OF THE dy THE CALL RETURNED, within
the bound of an fp32 accumulation of n products in any order, first order in u = 2^-24 with (1 + 2^-10) for the rest:

    |got - ref| <= n * u * sum|terms| * (1 + 2^-10)          n = M for dW and db, 27 * Cout for dx         (acc_bound)

(the products of two bf16 numbers are exact in fp32; an MFMA sum of n terms makes fewer than n roundings, each below u times a
partial sum that sum|terms| bounds).  A bf16 dx adds half a spacing at the magnitude of a value that far from the reference."""
import functools

import numpy as np
import torch

import conv_ref as R
from conv_ref import CUS, bf16_rne, big_geo, cdiv, persist_ok, tiles16, tiles8  # noqa: F401

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
BWD_SPLITK_TARGET, FUSED_WGRAD_TARGET = 128, 288
TILE_LAYOUT_FLOATS, EW32_FLOATS = 800 * 1024, 16 * 1024
DEFAULT_ROUTES = dict(R.DEFAULT_ROUTES, no_fused_bwd=0, no_fused_bwd_p=0, no_fused_bwd_big=0, no_defer_tail=0)
ROUTE_KEYS = ("bn", "riders", "dz_ks", "conv", "dgrad_ks", "dx_ks", "slabs", "slab_layout", "slab_ew", "pending")
ALLOW_PARTIALS, DEFER, LEAVE_PENDING = 1, 2, 4


# ------------------------------------------------------------------------------------------------ the operation
def conv3d_bwd_f64(x, w, dy, need_dx=True):
    """Conv3d(k=3, p=1) backward in float64 (torch CPU autograd): dx (None if not needed), dW, db"""
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(need_dx)
    wt = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    torch.nn.functional.conv3d(xt, wt, padding=1).backward(torch.from_numpy(np.asarray(dy, np.float64)))
    return (xt.grad.numpy() if need_dx else None), wt.grad.numpy(), np.asarray(dy, np.float64).sum(axis=(0, 2, 3, 4))


def bn_bwd_f64(y, dz, scale, gamma, mean, inv, a, b):
    """BatchNorm3d(train) + ReLU + Dropout3d backward with the statistics the forward saved (stat = mean, inv, a, b), float64:
    dyh = dz * scale * [fl32(a*y + b) > 0];  dy = gamma*inv*(dyh - mean(dyh) - xhat*mean(dyh*xhat));  dgamma, dbeta"""
    per = lambda v: np.asarray(v, np.float64).reshape(1, -1, 1, 1, 1)  # noqa: E731
    y = np.asarray(y, np.float64)
    pre = (y * per(a) + per(b)).astype(np.float32)
    s = 1.0 if scale is None else np.asarray(scale, np.float64)[:, :, None, None, None]
    dyh = np.asarray(dz, np.float64) * np.where(pre > 0, s, 0.0)
    xhat = (y - per(mean)) * per(inv)
    m = y.size // y.shape[1]
    dbeta, dgamma = dyh.sum(axis=(0, 2, 3, 4)), (dyh * xhat).sum(axis=(0, 2, 3, 4))
    dy = per(gamma) * per(inv) * (dyh - per(dbeta) / m - xhat * per(dgamma) / m)
    return dy, dgamma, dbeta


def exactness_margins(x, w, dy, exact=True):
    """(64 * max over the weights of sum|x*dy|, 128 * max over dx of sum|dy*w|, 8 * max sum|dy|).  exact = False: upper bounds of the
    first two that need no convolution (max|x| * sum|dy| per output channel; 27 * sum over co of max|dy| * max|w|)."""
    ax, aw, ady = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(dy, np.float64))
    s_dy = ady.sum(axis=(0, 2, 3, 4))
    if exact:
        gx, gw, _ = conv3d_bwd_f64(ax, aw, ady)
        return 64.0 * float(gw.max()), 128.0 * float(gx.max()), 8.0 * float(s_dy.max())
    return (64.0 * float(ax.max() * s_dy.max()), 128.0 * 27.0 * float((ady.max(axis=(0, 2, 3, 4)) * aw.max(axis=(1, 2, 3, 4))).sum()),
            8.0 * float(s_dy.max()))


def acc_bound(n, abs_terms):
    """fp32 accumulation of n products in any order (module docstring)"""
    return n * U * np.asarray(abs_terms, np.float64) * SLACK


def half_spacing(a):
    """half the distance between neighbouring bf16 numbers at magnitude a: 2^(floor(log2 a) - 8); 0 at 0"""
    a = np.abs(np.asarray(a, np.float64))
    return np.where(a > 0, np.exp2(np.floor(np.log2(np.maximum(a, 1e-300))) - 8), 0.0)


def conv_bwd_bounds(x, w, dy, cout, bf16_dx, ref_dx):
    """(bound dx or None, bound dW, bound db) against the float64 gradients of this dy"""
    gx, gw, gb = conv3d_bwd_f64(np.abs(x), np.abs(w), np.abs(dy), need_dx=ref_dx is not None)
    m = dy.size // dy.shape[1]
    bx = None
    if ref_dx is not None:
        bx = acc_bound(27 * cout, gx)
        if bf16_dx:
            bx = bx + half_spacing(np.abs(ref_dx) + bx)
    return bx, acc_bound(m, gw), acc_bound(m, gb)


# ------------------------------------------------------------------------------------------------ route predicates
def workgroups8(cout, g):
    return tiles8(g) * (cout // (32 if cout % 32 == 0 else 16))


def pick_ksplit(cin, cout, g, target=BWD_SPLITK_TARGET):
    """conv3_mfma.hip pick_ksplit of a (cin -> cout) launch with a workgroup target (<= 128)"""
    if big_geo(g):
        return 1
    wgs, nchunk, k = workgroups8(cout, g), cin // 16, 1
    while wgs * k < target and k * 2 <= nchunk and nchunk % (k * 2) == 0 and k < 16:
        k *= 2
    return k


def mfma_class(dt, cin, cout):
    return dt == 1 and cin % 16 == 0 and cout % 16 == 0 and cin >= 16


def fused_persist_ok(cin, cout, g, r):
    return persist_ok(cout, cin, g, r) and not r["no_fused_bwd"] and not r["no_fused_bwd_p"]        # persist_ok of the SWAPPED channels


def fused_ok(cin, cout, dxcs, g, r):
    if big_geo(g) and (persist_ok(cout, cin, g, r) or r["no_fused_bwd_big"]):
        return False
    return cin % 32 == 0 and dxcs % 8 == 0 and not r["no_fused_bwd"]


def wg_target(cin, cout, dxcs, g, r):
    return CUS if fused_persist_ok(cin, cout, g, r) else FUSED_WGRAD_TARGET if fused_ok(cin, cout, dxcs, g, r) else 0


def wgrad_slabs(cin, cout, g, target=0):
    """wgrad_cfg: one round of workgroups (target, default two per CU) over the (co block, ci block) groups"""
    groups, ntiles = (cout // 16) * (cin // 16), tiles16(g)
    want = max((target if target > 0 else 2 * CUS) // groups, 1)
    return cdiv(ntiles, cdiv(ntiles, want))


def slab_sum(layout0, cin, cout, dw=True):
    """(layout, ew) of slab_job_make / wgrad_slab_sum for a slab of Cout*Cin*27 + Cout floats"""
    sz = cout * cin * 27 + cout
    if layout0:
        return 0, 1 if sz < 128 else 4 if sz < 1024 else 8 if sz < EW32_FLOATS else 32
    if dw and sz >= TILE_LAYOUT_FLOATS:
        return 2, 0
    return 1, 8 if sz < EW32_FLOATS else 32


def bn_small(c, m, r):
    return R.bn_small(c, m, r)


def vec8_ok(c, *strides):
    return c % 8 == 0 and all(s % 8 == 0 for s in strides) and c // 8 <= 256


def predict_route(case, routes=None, flags=0, bn=True, riders=0, dz_ks=0, need_dx=True):
    """every field of mi3d_conv3_bn_bwd_route for a case of the table under the given route switches and entry flags"""
    r = dict(DEFAULT_ROUTES, **(routes or {}))
    cin, cout, g, dt = case["cin"], case["cout"], case["geo"], case["dtype"]
    m = g[0] * g[1] * g[2] * g[3]
    mfma, c1 = mfma_class(dt, cin, cout), dt == 1 and cin == 1 and cout % 16 == 0
    dx = need_dx and not c1
    dxcs = cin
    out = dict(bn=(2 if bn_small(cout, m, r) else 1) if bn else 0, riders=riders if bn else 0, dz_ks=dz_ks, conv=0, dgrad_ks=0,
               dx_ks=0, slabs=0, slab_layout=0, slab_ew=0, pending=0)
    allow = bool(flags & ALLOW_PARTIALS) and dx and dxcs % 8 == 0 and not r["no_defer_tail"]
    ks_standalone = pick_ksplit(cout, cin, g) if (mfma and dxcs % 8 == 0 and not persist_ok(cout, cin, g, r)) else 1
    if not mfma:
        out["conv"] = 1 if c1 else 0
        out["dgrad_ks"] = 1 if dx else 0
        if c1:
            out["slabs"] = min(tiles16(g), 1024)
            out["slab_layout"], out["slab_ew"] = slab_sum(True, 1, cout)
    elif flags & DEFER:
        out["conv"], out["dgrad_ks"] = 6, ks_standalone if dx else 0
        out["dx_ks"] = ks_standalone if allow and ks_standalone > 1 else 0
        out["slabs"] = wgrad_slabs(cin, cout, g, wg_target(cin, cout, dxcs if dx else 8, g, r))
        out["slab_layout"], out["slab_ew"] = slab_sum(False, cin, cout)
    elif dx and fused_persist_ok(cin, cout, g, r):
        out["conv"], out["dgrad_ks"] = 2, 1
        out["slabs"] = wgrad_slabs(cin, cout, g, CUS)
        out["slab_layout"], out["slab_ew"] = slab_sum(False, cin, cout)
    elif dx and fused_ok(cin, cout, dxcs, g, r):
        ks = pick_ksplit(cout, cin, g)
        out["conv"], out["dgrad_ks"] = 3 if big_geo(g) else 4, ks
        out["dx_ks"] = ks if allow and ks > 1 else 0
        out["slabs"] = wgrad_slabs(cin, cout, g, FUSED_WGRAD_TARGET)
        out["slab_layout"], out["slab_ew"] = slab_sum(False, cin, cout)
    else:
        out["conv"], out["dgrad_ks"] = 5, ks_standalone if dx else 0       # the stand-alone input gradient never leaves partials
        out["slabs"] = wgrad_slabs(cin, cout, g, 0)
        out["slab_layout"], out["slab_ew"] = slab_sum(False, cin, cout)
    if flags & LEAVE_PENDING:
        # the sum waits unless the launch summed its slabs itself: the fused launch's tail kernel (split-K dx finished there), the
        # direct kernels
        tail = out["conv"] == 4 and out["dgrad_ks"] > 1 and out["dx_ks"] == 0
        out["pending"] = int((mfma or c1) and not tail)
    return out


# ------------------------------------------------------------------------------------------------ the case table
def _case(cin, cout, geo, conv, dgrad_ks=1, slabs=0, layout=1, ew=8, bn=2, dtype=1, kmax_dy=8, oracle=True):
    return dict(cin=cin, cout=cout, geo=geo, dtype=dtype, kmax_dy=kmax_dy, oracle=oracle,
                route=dict(bn=bn, riders=0, dz_ks=0, conv=conv, dgrad_ks=dgrad_ks, dx_ks=0, slabs=slabs, slab_layout=layout, slab_ew=ew,
                           pending=0))


# name: shape, and the route the DEFAULT switches must give it with BatchNorm on and flags 0.  The smallest shapes that reach each
# route; ragged on purpose.  oracle: small enough for the C oracle's scalar loops.
CASES = {
    "persist_11":   _case(16, 16, (1, 5, 17, 35), conv=2, slabs=18),                                  # 2 x 3 x 3 tiles, one per slab
    "persist_12":   _case(16, 32, (1, 7, 18, 33), conv=2, slabs=18, ew=8),
    "persist_21":   _case(32, 16, (1, 61, 63, 130), conv=2, slabs=128, ew=8, bn=1, kmax_dy=4, oracle=False),   # 1152 tiles >= 1024
    "big_32_32":    _case(32, 32, (2, 6, 17, 35), conv=3, slabs=36, ew=32),
    "big_32_16":    _case(32, 16, (1, 5, 17, 35), conv=3, slabs=18, ew=8),                            # below 1024 tiles: not persistent
    "small_32_16":  _case(32, 16, (2, 5, 9, 12), conv=4, slabs=8, ew=8),
    "sk2_64_32":    _case(64, 32, (2, 5, 9, 12), conv=4, dgrad_ks=2, slabs=8, ew=32),
    "sk8_128_256":  _case(128, 256, (2, 6, 6, 6), conv=4, dgrad_ks=8, slabs=2, layout=2, ew=0, oracle=False),
    "sk16_256_256": _case(256, 256, (1, 3, 3, 3), conv=4, dgrad_ks=16, slabs=1, layout=2, ew=0),
    "pair_16_32":   _case(16, 32, (2, 5, 9, 12), conv=5, dgrad_ks=2, slabs=8, ew=8),
    "pair_48_16":   _case(48, 16, (1, 5, 9, 12), conv=5, slabs=4, ew=32),
    "c1_16":        _case(1, 16, (2, 5, 9, 17), conv=1, dgrad_ks=0, slabs=16, layout=0, ew=4),
    "direct_f32":   _case(4, 5, (2, 5, 9, 17), conv=0, slabs=0, layout=0, ew=0, bn=1, dtype=0),         # C = 5: finalize launch
}
FUSED_CASES = [k for k, c in CASES.items() if c["route"]["conv"] in (2, 3, 4)]
SPLITK_CASES = [k for k, c in CASES.items() if c["route"]["dgrad_ks"] > 1]
MFMA_CASES = [k for k, c in CASES.items() if c["route"]["conv"] in (2, 3, 4, 5)]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Dyadic inputs and the float64 gradients of one case, and the saved forward state of the BatchNorm runs; computed once,
    read-only.  The large case's float64 reference is one CPU convolution backward (a few seconds)."""
    c = CASES[name]
    n, d, h, w = c["geo"]
    cin, cout = c["cin"], c["cout"]
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    x, wgt, b = R.dyadic_conv_inputs(rng, n, cin, cout, d, h, w)
    km = c["kmax_dy"]
    dy = rng.integers(-km, km + 1, (n, cout, d, h, w)).astype(np.float32) / 8
    first = cin == 1
    dx, dW, db = conv3d_bwd_f64(x, wgt, dy, need_dx=not first)
    pre_w = rng.integers(-8, 9, wgt.shape).astype(np.float32) / 4          # dyadic prefill of an accumulate = 1 run
    pre_b = rng.integers(-8, 9, cout).astype(np.float32) / 4
    # the BatchNorm runs: y = the forward's stored conv output (dyadic, bf16_rne for bf16), its float64 statistics as the saved
    # fp32 stat, dropout scales 0 / 2, negative gammas, dz dyadic in k/4 as in test_gpu_bn_ops (dbeta's allowance counts on it)
    gamma = ((rng.random(cout) + 0.5) * np.where(rng.random(cout) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = (rng.standard_normal(cout) * 0.3).astype(np.float32)
    scale = (rng.random((n, cout)) >= 0.5).astype(np.float32) * 2.0
    scale[:, 0] = (0.0, 2.0)[:n] if n > 1 else (2.0,)
    exact_y = R.conv3d_f64(x, wgt, b)
    y = bf16_rne(exact_y) if c["dtype"] == 1 else exact_y.astype(np.float32)
    st = R.bn_stats_f64(y, gamma, beta, np.zeros(cout), np.ones(cout))
    stat = np.stack([st["mean"], st["inv"], st["A"], st["B"]]).astype(np.float32)
    dz = (rng.integers(-8, 9, (n, cout, d, h, w)) / 4.0).astype(np.float32)
    k = dict(c, name=name, x=x, w=wgt, dy=dy, dx=dx, dW=dW, db=db, pre_w=pre_w, pre_b=pre_b, gamma=gamma, beta=beta, scale=scale, y=y,
             stat=stat, dz=dz)
    for v in k.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return k
