"""BatchNorm / ReLU / Dropout3d (/ MaxPool) per operator through the C ABI against the C oracle: the instantiations of bn.hip that
no other per-operator test reaches -- fp32 (VEC = 1 and VEC = 8), the un-paired bf16 pool kernel (C = 24), a channel stride
of 2C (the concat buffer's layout), the eval path, and the finalize-launch route at small size (no_small_bn = 1).

Inputs are the small dyadic numbers of test_gpu_round3.py (bf16 holds them exactly; sum and sum of squares of y, and the
sum of dz * mask, are exact in fp32 in any order), N = 2 with per-sample Dropout3d scales 0 or 2.

Allowances.  stat, the running buffers, nbt, dgamma, dbeta and the bf16 tensors: those of
test_bn_relu_drop_bf16_vec8_per_op_vs_c_oracle.  pooled: exact.  fp32 z and dy: per-element bounds derived from the
kernels' formulas, u = 2^-24, first order, (1 + 2^-10) for the higher orders:

  z.  The oracle gives fl32(y*A + B) * s with A = gamma*inv, B = beta - mean*A in double.  The kernel computes one fma with
  a = fl32(A), b = fl32(B) (its statistics are double sums of exact fp32 partials), ReLU, one multiply by s:
      |z - z_ref| <= s*u*(|y*A| + |B|)  [a, b]  + u|z| [fma] + u|z| [*s] + u|z_ref| [the oracle's own rounding]
  A value the ReLU cuts on one side only is smaller than the first term, so the same bound holds across the cut.

  dy.  Reference: bn_train_bwd with the saved fp32 mean, inv: g*(dyh - c1 - xhat*c2), g = gamma*inv, which is
  g*dyh - k*y + (k*mean - g*c1), k = g*c2*inv.  The kernel evaluates fma(g'*m, dz, fma(-k', y, B')) in fp32 with
      g' = fl32(gamma*inv_double): 2u from g;   c1' = fl32(S1/M), S1 exact: u;
      c2' = fl32(S2'/M), S2' a fp32 sum, in some order, of M terms t = dyh*(y - mean)*inv of three roundings each:
            dc2 <= u|c2| + (M + 2)*u*sum|t| / M          (any summation order: (M - 1)*u*sum|t|)
      k' = fl(fl(g'*c2')*inv):  dk <= 4u|k| + |g*inv|*dc2
      B' = fl(k'*mean - fl(g'*c1')):  dB <= dk*|mean| + u|k*mean| + 4u|g*c1| + u|B|
      |dy - dy_ref| <= 3u|g*dyh| [g', g'*m] + dk*|y| + dB + u|B - k*y| [inner fma] + u|dy| [outer] + u|dy_ref| [oracle]
  The mask needs the sign of fma(y, a, b): the CPU test asserts that on these inputs |y*A + B| exceeds the error of the fma
  everywhere, so kernel and oracle cut at the same elements.

test_fp32_bounds_hold_for_a_float32_restatement (not gpu) checks that a float32 numpy restatement of both formulas stays
inside these bounds against the float64 oracle on these very inputs."""
import numpy as np
import pytest
import torch

import multimodal_segmentation_project_amd as mi  # noqa: F401
from multimodal_segmentation_project_amd import _lib
from multimodal_segmentation_project_amd._lib import call, ptr

DEV = "cuda:0"
U = 2.0 ** -24
HALF_ULP = 2.0 ** -8
EPS = 1e-5
SLACK = 1.0 + 2.0 ** -10

# name: (dtype, C, (D, H, W), channel stride / C, routes)      N = 2 everywhere
CASES = {
    "f32_c5": (0, 5, (3, 5, 7), 1, {}),                                 # VEC = 1, G = 5
    "f32_c8": (0, 8, (3, 5, 7), 1, {}),                                 # VEC = 8, consumer prologue (SMALL / TRAIN)
    "f32_c8_stride": (0, 8, (3, 5, 7), 2, {}),                          # ycs = zcs = dzcs = dycs = 2C
    "f32_c8_finalize": (0, 8, (3, 5, 7), 1, {"no_small_bn": 1}),        # bn_stats_finalize / bn_bwd_finalize, SMALL = false
    "bf16_c24_pool": (1, 24, (4, 6, 10), 1, {}),                        # C / 8 = 3: the un-paired pool kernel
    "f32_c5_pool": (0, 5, (4, 6, 10), 1, {}),                           # VEC = 1 pool kernel
    "bf16_c16_pool_finalize": (1, 16, (4, 6, 10), 1, {"no_small_bn": 1}),   # paired pool kernel, TRAIN = false
}
_cache = {}


def dyadic(rng, shape, lo=-16, hi=16, den=8.0):
    return (rng.integers(lo, hi + 1, shape) / den).astype(np.float32)


def case_data(orc, name):
    """Inputs (NCDHW float32, bf16-exact) and the oracle's forward of one case; computed once, never modified."""
    if name not in _cache:
        dt, c, (d, h, w), cs, route = CASES[name]
        n = 2
        rng = np.random.default_rng(sum(map(ord, name)))
        y = dyadic(rng, (n, c, d, h, w)) + (rng.integers(-8, 9, (1, c, 1, 1, 1)) / 4.0).astype(np.float32)
        dz = dyadic(rng, (n, c, d, h, w), -8, 8, 4.0)
        gamma = ((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.3, -1.0, 1.0)).astype(np.float32)
        beta = (rng.standard_normal(c) * 0.3).astype(np.float32)
        rm0, rv0 = (rng.standard_normal(c) * 0.1).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
        scale = (rng.random((n, c)) >= 0.5).astype(np.float32) * 2.0
        scale[:, 0] = (0.0, 2.0)                                            # the samples differ, whatever was drawn
        k = dict(dt=dt, n=n, c=c, d=d, h=h, w=w, cs=cs, route=route, y=y, dz=dz, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, scale=scale)
        k["yhat"], k["mean"], k["inv"], k["rm"], k["rv"] = orc.bn_train_fwd(y, gamma, beta, rm0, rv0, 0.1, EPS)
        k["z"] = orc.relu_drop_fwd(k["yhat"], scale)
        for v in k.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = k
    return _cache[name]


def per_c(a):
    return np.asarray(a, np.float64).reshape(1, -1, 1, 1, 1)


def z_bound(y, A, B, s, z_ref):
    """A, B per channel in double, s per (sample, channel); see the module docstring."""
    s = np.asarray(s, np.float64)[:, :, None, None, None]
    return SLACK * (s * U * (np.abs(y * per_c(A)) + np.abs(per_c(B))) + 3 * U * np.abs(z_ref))


def bwd_ref(orc, k, mean32, inv32, a32, b32):
    """The oracle's backward chain with the statistics the forward saved, and the dy bound of the module docstring."""
    y, c = k["y"].astype(np.float64), k["c"]
    m = k["n"] * k["d"] * k["h"] * k["w"]
    yhat_k = (y * per_c(a32) + per_c(b32)).astype(np.float32)
    dyh = orc.relu_drop_bwd(yhat_k, k["dz"], k["scale"])
    dy_ref, dg_ref, db_ref = orc.bn_train_bwd(k["y"], dyh, k["gamma"], mean32, inv32)
    mean, inv = per_c(mean32), per_c(inv32)
    g = per_c(k["gamma"]) * inv
    t = dyh.astype(np.float64) * (y - mean) * inv
    c1, c2 = per_c(dyh.sum(axis=(0, 2, 3, 4), dtype=np.float64) / m), per_c(t.sum(axis=(0, 2, 3, 4)) / m)
    dc2 = U * np.abs(c2) + (m + 2) * U * per_c(np.abs(t).sum(axis=(0, 2, 3, 4))) / m
    kk = g * c2 * inv
    dk = 4 * U * np.abs(kk) + np.abs(g * inv) * dc2
    Bh = kk * mean - g * c1
    dB = dk * np.abs(mean) + U * np.abs(kk * mean) + 4 * U * np.abs(g * c1) + U * np.abs(Bh)
    bound = SLACK * (3 * U * np.abs(g * dyh) + dk * np.abs(y) + dB + U * np.abs(Bh - kk * y) + 2 * U * np.abs(dy_ref))
    return dy_ref, dg_ref, db_ref, bound, dyh


def within(got, ref, bound, what):
    bad = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) > bound
    assert not bad.any(), (what, int(bad.sum()), float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))


def close_bf16(got, ref, abs_tol, what):
    within(got, ref, HALF_ULP * 1.001 * np.abs(ref) + abs_tol, what)


@pytest.mark.parametrize("name", ["f32_c5", "f32_c8", "f32_c8_stride", "f32_c8_finalize"])
def test_fp32_bounds_hold_for_a_float32_restatement(orc, name):
    """CPU: float32 numpy arithmetic in the kernels' order (fp32 accumulation of S2 included) stays inside z_bound and the
    dy bound against the float64 oracle, and no element sits on the ReLU cut."""
    k = case_data(orc, name)
    f = np.float32
    y64, y32 = k["y"].astype(np.float64), k["y"]
    m = k["n"] * k["d"] * k["h"] * k["w"]
    mean = y64.mean(axis=(0, 2, 3, 4))
    var = (y64 * y64).mean(axis=(0, 2, 3, 4)) - mean * mean
    inv = 1.0 / np.sqrt(var + f(EPS).astype(np.float64))
    A, B = k["gamma"].astype(np.float64) * inv, k["beta"].astype(np.float64) - mean * k["gamma"].astype(np.float64) * inv
    a32, b32 = A.astype(f), B.astype(f)
    np.testing.assert_allclose(mean.astype(f), k["mean"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(inv.astype(f), k["inv"], rtol=2e-6)
    pre = (y64 * per_c(a32) + per_c(b32)).astype(f)                      # the fma: one rounding of an exact double product-sum
    assert (np.abs(y64 * per_c(A) + per_c(B)) > 8 * U * (np.abs(y64 * per_c(A)) + np.abs(per_c(B)))).all()
    s = k["scale"][:, :, None, None, None]
    z32 = np.maximum(pre, f(0)) * s
    within(z32, k["z"], z_bound(y64, A, B, k["scale"], k["z"]), "z")
    mean32, inv32 = mean.astype(f), inv.astype(f)
    dy_ref, _, _, bound, dyh = bwd_ref(orc, k, mean32, inv32, a32, b32)
    sh = (1, -1, 1, 1, 1)
    mask = np.where(pre > 0, s, f(0)).astype(f)
    dyh32 = k["dz"] * mask
    np.testing.assert_array_equal(dyh32, dyh)
    t32 = dyh32 * (y32 - mean32.reshape(sh)) * inv32.reshape(sh)
    s2 = np.zeros(k["c"], f)
    for row in np.moveaxis(t32, 1, -1).reshape(-1, k["c"]):                  # worst order: one sequential fp32 sum
        s2 = s2 + row
    c1 = (dyh32.sum(axis=(0, 2, 3, 4), dtype=np.float64) / m).astype(f)
    c2 = (s2.astype(np.float64) / m).astype(f)
    kk = a32 * c2 * inv32
    Bp = kk * mean32 - a32 * c1
    inner = ((-kk).reshape(sh).astype(np.float64) * y64 + Bp.reshape(sh).astype(np.float64)).astype(f)
    dy32 = ((a32.reshape(sh) * mask).astype(np.float64) * k["dz"].astype(np.float64) + inner.astype(np.float64)).astype(f)
    within(dy32, dy_ref, bound, "dy")


def cl(a, dt, cs=1, fill=0.0):
    """NCDHW float array -> channels-last device tensor [N][D][H][W][cs * C] (the first C channels hold the data)."""
    n, c = a.shape[:2]
    t = torch.full((n,) + tuple(a.shape[2:]) + (cs * c,), fill, dtype=torch.float32)
    t[..., :c] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 4, 1)))
    return t.to(DEV).to(torch.bfloat16 if dt else torch.float32)


def ncdhw(t, c):
    return t[..., :c].float().cpu().numpy().transpose(0, 4, 1, 2, 3)


def dev_state(k):
    g_d, b_d = torch.from_numpy(k["gamma"].copy()).to(DEV), torch.from_numpy(k["beta"].copy()).to(DEV)
    rm, rv = torch.from_numpy(k["rm0"].copy()).to(DEV), torch.from_numpy(k["rv0"].copy()).to(DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    drop = torch.from_numpy(k["scale"].copy()).to(DEV)
    ws = torch.zeros(_lib.lib().mi3d_bn_workspace_bytes(k["c"]), dtype=torch.uint8, device=DEV)
    return g_d, b_d, rm, rv, nbt, drop, ws, torch.empty(4 * k["c"], device=DEV)


def check_stats(k, stat, rm, rv, nbt):
    st = stat.cpu().numpy().reshape(4, k["c"])
    np.testing.assert_allclose(st[0], k["mean"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(st[1], k["inv"], rtol=2e-6)
    np.testing.assert_allclose(st[2], k["gamma"] * k["inv"], rtol=2e-6)
    np.testing.assert_allclose(rm.cpu().numpy(), k["rm"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(rv.cpu().numpy(), k["rv"], rtol=2e-6)
    assert int(nbt) == 1
    return st


def check_z(k, z):
    if k["dt"]:
        close_bf16(z, k["z"], 2e-6, "z")
    else:
        A = k["gamma"].astype(np.float64) * k["inv"].astype(np.float64)      # inv to 2e-6 (check_stats): second order in the bound
        B = k["beta"].astype(np.float64) - k["mean"].astype(np.float64) * A
        within(z, k["z"], z_bound(k["y"].astype(np.float64), A, B, k["scale"], k["z"]), "z")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32_c5", "f32_c8", "f32_c8_stride", "f32_c8_finalize"])
def test_bn_relu_drop_fp32_per_op_vs_c_oracle(orc, name):
    """mi3d_bn_relu_drop_forward / _backward in fp32: bn_stats / bn_apply / bn_bwd_reduce / bn_bwd_apply <float, 1 | 8>, through
    the consumer prologue, the finalize launches (no_small_bn) and a channel stride of 2C (the other half stays untouched)."""
    k = case_data(orc, name)
    c, cs = k["c"], k["cs"]
    m, v, s = k["n"] * k["d"] * k["h"] * k["w"], k["d"] * k["h"] * k["w"], k["cs"] * k["c"]
    ycl, dzcl = cl(k["y"], 0, cs), cl(k["dz"], 0, cs)
    g_d, b_d, rm, rv, nbt, drop, ws, stat = dev_state(k)
    z, dy = torch.full_like(ycl, 77.0), torch.full_like(ycl, 77.0)
    with _lib.routes(**k["route"]):
        call("mi3d_bn_relu_drop_forward", 0, ptr(ycl), s, c, m, v, ptr(g_d), ptr(b_d), ptr(rm), ptr(rv), ptr(nbt), 0.1, EPS, 1,
             ptr(drop), ptr(z), s, ptr(stat), ptr(ws), None)
        st = check_stats(k, stat, rm, rv, nbt)
        check_z(k, ncdhw(z, c))
        dg, db = torch.full((c,), 7.0, device=DEV), torch.full((c,), -3.0, device=DEV)
        dy_ref, dg_ref, db_ref, bound, _ = bwd_ref(orc, k, st[0], st[1], st[2], st[3])
        scale_g = np.sqrt(m) * 4.0
        for acc in (0, 1):
            call("mi3d_bn_relu_drop_backward", 0, ptr(dzcl), s, ptr(ycl), s, c, m, v, ptr(stat), ptr(drop), ptr(dy), s, ptr(dg),
                 ptr(db), acc, ptr(ws), None)
            f = acc + 1
            np.testing.assert_allclose(db.cpu().numpy(), f * db_ref, rtol=0, atol=f * 1e-4 * max(1.0, float(np.abs(db_ref).max()) * 1e-3))
            np.testing.assert_allclose(dg.cpu().numpy(), f * dg_ref, rtol=2e-5, atol=f * 2e-6 * scale_g)
            within(ncdhw(dy, c), dy_ref, bound, "dy")
    if cs > 1:
        assert bool((z[..., c:] == 77.0).all()) and bool((dy[..., c:] == 77.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bf16_c24_pool", "f32_c5_pool", "bf16_c16_pool_finalize"])
def test_bn_apply_pool_per_op_vs_c_oracle(orc, name):
    """mi3d_bn_relu_drop_pool_forward: the un-paired bf16 kernel (C = 24), the scalar fp32 kernel (C = 5) and the paired kernel
    behind a finalize launch: z as above, pooled = the oracle's pool of the kernel's own z, and the two-launch route bit for bit."""
    k = case_data(orc, name)
    n, c, d, h, w, dt = k["n"], k["c"], k["d"], k["h"], k["w"], k["dt"]
    m, v = n * d * h * w, d * h * w
    ycl = cl(k["y"], dt)
    outs = []
    with _lib.routes(**k["route"]):
        for fused in (True, False):
            g_d, b_d, rm, rv, nbt, drop, ws, stat = dev_state(k)
            z = torch.empty_like(ycl)
            pooled = torch.empty((n, d // 2, h // 2, w // 2, c), device=DEV, dtype=ycl.dtype)
            if fused:
                call("mi3d_bn_relu_drop_pool_forward", dt, ptr(ycl), c, c, n, d, h, w, ptr(g_d), ptr(b_d), ptr(rm), ptr(rv), ptr(nbt),
                     0.1, EPS, ptr(drop), ptr(z), c, ptr(pooled), c, ptr(stat), ptr(ws), None)
            else:
                call("mi3d_bn_relu_drop_forward", dt, ptr(ycl), c, c, m, v, ptr(g_d), ptr(b_d), ptr(rm), ptr(rv), ptr(nbt), 0.1, EPS, 1,
                     ptr(drop), ptr(z), c, ptr(stat), ptr(ws), None)
                call("mi3d_maxpool2_forward", dt, ptr(z), c, c, n, d, h, w, ptr(pooled), c, None)
            check_stats(k, stat, rm, rv, nbt)
            outs.append((z, pooled, stat, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                   # fused == two launches, bit for bit
    check_z(k, ncdhw(outs[0][0], c))
    np.testing.assert_array_equal(ncdhw(outs[0][1], c), orc.maxpool2_fwd(ncdhw(outs[0][0], c)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32_c5", "bf16_c24_pool"])
def test_bn_relu_drop_eval_per_op_vs_c_oracle(orc, name):
    """training = 0: bn_eval_stats and the TRAIN = false apply kernels; the running buffers and nbt stay as they were."""
    k = case_data(orc, name)
    c, dt = k["c"], k["dt"]
    m, v = k["n"] * k["d"] * k["h"] * k["w"], k["d"] * k["h"] * k["w"]
    ycl = cl(k["y"], dt)
    g_d, b_d, rm, rv, nbt, drop, ws, stat = dev_state(k)
    z = torch.empty_like(ycl)
    call("mi3d_bn_relu_drop_forward", dt, ptr(ycl), c, c, m, v, ptr(g_d), ptr(b_d), ptr(rm), ptr(rv), ptr(nbt), 0.1, EPS, 0,
         ptr(drop), ptr(z), c, ptr(stat), ptr(ws), None)
    inv = 1.0 / np.sqrt(k["rv0"].astype(np.float64) + np.float64(np.float32(EPS)))
    st = stat.cpu().numpy().reshape(4, c)
    np.testing.assert_array_equal(st[0], k["rm0"])
    np.testing.assert_allclose(st[1], inv, rtol=2e-6)
    np.testing.assert_allclose(st[2], k["gamma"] * inv, rtol=2e-6)
    np.testing.assert_array_equal(rm.cpu().numpy(), k["rm0"])
    np.testing.assert_array_equal(rv.cpu().numpy(), k["rv0"])
    assert int(nbt) == 0
    z_ref = orc.relu_drop_fwd(orc.bn_eval_fwd(k["y"], k["gamma"], k["beta"], k["rm0"], k["rv0"], EPS), k["scale"])
    if dt:
        close_bf16(ncdhw(z, c), z_ref, 2e-6, "z")
    else:
        A = k["gamma"].astype(np.float64) * inv
        within(ncdhw(z, c), z_ref, z_bound(k["y"].astype(np.float64), A, k["beta"].astype(np.float64) - k["rm0"].astype(np.float64) * A,
                                           k["scale"], z_ref), "z")
