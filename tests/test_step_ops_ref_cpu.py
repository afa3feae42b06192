"""Host side of the per-operator step tests (no GPU): the float64 references of tests/step_ops_ref.py, which
tests/test_gpu_step_ops.py checks the kernels against, are themselves pinned to torch on the CPU (and the C oracle's
step operators to them); the MaxPool inputs meet their tie conditions; the single-step AdamW bounds hold, with margin,
for a float32 numpy evaluation of the same formula; and the ABI rejects bad arguments of these operators before any launch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_ops_ref as S  # noqa: E402

from multimodal_segmentation_project_amd import _lib  # noqa: E402


# ---------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("lr,wd,eps", S.ADAMW_HYPERS)
def test_adamw_ref_is_torch_adamw_in_float64_over_50_steps(lr, wd, eps):
    rng = np.random.default_rng(0)
    n = 257
    p0 = rng.standard_normal(n)
    grads = rng.standard_normal((50, n)) * np.exp(rng.uniform(-6, 2, (50, 1)))
    h32 = [float(np.float32(x)) for x in (lr, S.B1, S.B2, eps, wd)]            # the reference rounds them to float32
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=h32[0], betas=(h32[1], h32[2]), eps=h32[3], weight_decay=h32[4])
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 51):
        tp.grad = torch.tensor(grads[t - 1])
        opt.step()
        p, m, v = S.adamw_ref(p, grads[t - 1], m, v, lr, S.B1, S.B2, eps, wd, t)
    st = opt.state[tp]
    np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


def test_adamw_grad_scale_is_a_premultiplied_gradient():
    p, g, m, v = S.adamw_state(100, 3)
    a = S.adamw_ref(p, g, m, v, 1e-3, S.B1, S.B2, 1e-8, 0.01, 7, grad_scale=0.25)
    b = S.adamw_ref(p, g.astype(np.float64) * 0.25, m, v, 1e-3, S.B1, S.B2, 1e-8, 0.01, 7)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_adamw_single_step_bounds_hold_for_a_float32_evaluation():
    """The bounds of adamw_step_bounds against a float32 numpy evaluation of the same formula, over the grids the GPU test
    uses.  They have to hold here, or they are not bounds that a correct float32 kernel can be held to; the worst ratio is printed."""
    worst = np.zeros(3)
    for (lr, wd, eps) in S.ADAMW_HYPERS:
        for t in S.ADAMW_STEPS:
            for gmag in S.ADAMW_GMAGS:
                for gs in S.ADAMW_GRAD_SCALES:
                    st = S.adamw_state(20000, 11, gmag)
                    ref = S.adamw_ref(*st, lr, S.B1, S.B2, eps, wd, t, gs)
                    bnd = S.adamw_step_bounds(*st, lr, S.B1, S.B2, eps, wd, t, gs)
                    got = S.adamw_f32(*st, lr, S.B1, S.B2, eps, wd, t, gs)
                    for k in range(3):
                        worst[k] = max(worst[k], float((np.abs(got[k].astype(np.float64) - ref[k]) / bnd[k]).max()))
    print("float32 numpy restatement, worst |delta| / bound: p %.3f  m %.3f  v %.3f" % tuple(worst))
    assert (worst <= 1.0).all(), worst


def test_c_oracle_adamw_and_linear_agree_with_the_references(orc):
    p, g, m, v = S.adamw_state(1000, 5)
    for t in (1, 10, 1000):
        h = [float(np.float32(x)) for x in (1e-3, S.B1, S.B2, 1e-8, 0.01)]
        got = orc.adamw_step(p, g, m, v, *h, t)
        ref = S.adamw_ref(p, g, m, v, *h, t)
        bnd = S.adamw_step_bounds(p, g, m, v, *h, t)
        for a, r, b in zip(got, ref, bnd):
            assert (np.abs(a.astype(np.float64) - r) <= b).all()
    rng = np.random.default_rng(1)
    x, w, b, gy = (rng.standard_normal(s).astype(np.float32) for s in ((5, 70), (7, 70), (7,), (5, 7)))
    tol = 70 * S.U * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b))
    assert (np.abs(orc.linear_fwd(x, w, b) - S.linear_ref(x, w, b)) <= tol).all()
    gx, gw, gb = orc.linear_bwd(x, w, gy)
    rx, rw, rb = S.linear_bwd_ref(x, w, S.linear_ref(x, w, b), gy)
    np.testing.assert_allclose(gx, rx, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gw, rw, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gb, rb, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- MaxPool3d
@pytest.mark.parametrize("case", S.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_references_are_torch_max_pool3d_and_inputs_are_tie_heavy(case):
    C, N, D, H, W = case
    z, dp, dskip = S.pool_inputs(C, N, D, H, W, S.POOL_SEED)
    for a in (z, dp, dskip, dp.reshape(-1)[:1] + dskip.reshape(-1)[:1]):
        assert np.array_equal(S.bf16_round(a), a)                                   # every operand is bf16-exact
    frac, firsts = S.pool_tie_stats(z)
    print(f"{case}: tied windows {frac:.3f}, first-maximum positions {sorted(firsts)}")
    assert frac >= 0.5
    assert firsts == set(range(8))
    w = S._windows(z)
    if w[..., 0].size >= 64:                                                        # the tiny cases cannot hold everything
        assert (w == 0).any() and (w.max(axis=-1) < 0).any()                        # zeros; negative-only windows
        assert (w.min(axis=-1) == w.max(axis=-1)).any()                             # all-equal windows
    zt = torch.tensor(z.transpose(0, 4, 1, 2, 3), dtype=torch.float64, requires_grad=True)
    out = F.max_pool3d(zt, 2, 2)
    out.backward(torch.tensor(dp.transpose(0, 4, 1, 2, 3), dtype=torch.float64))
    want_dz = zt.grad.numpy().transpose(0, 2, 3, 4, 1)
    for dt in ("f32", "bf16"):
        assert np.array_equal(S.maxpool2_fwd_ref(z, dt), out.detach().numpy().transpose(0, 2, 3, 4, 1))
        assert np.array_equal(S.maxpool2_bwd_ref(z, dp, None, dt), want_dz)
        assert np.array_equal(S.maxpool2_bwd_ref(z, dp, dskip, dt), want_dz + dskip)    # exact: dyadic, bf16-representable
        assert np.array_equal(S.bf16_round(want_dz + dskip), (want_dz + dskip).astype(np.float32))


def test_bf16_rounding_is_torchs_round_to_nearest_even():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 6, 4096).astype(np.float32),
                        S.bf16_to_f32(np.arange(0x3F80, 0x3F90, dtype=np.uint16)) + np.float32(2.0 ** -8),      # exact halfway cases
                        np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 3.0e38], np.float32)]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(S.bf16_round(x).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(S.bf16_bits(x), (want.view(np.uint32) >> 16).astype(np.uint16))


# ---------------------------------------------------------------------------------------------------- DANN head
@pytest.mark.parametrize("relu,use_drop,use_b", [(0, False, True), (1, False, True), (1, True, True), (0, True, False)])
def test_linear_reference_is_torch_linear_in_float64(relu, use_drop, use_b):
    rng = np.random.default_rng(4)
    M, K, No = 5, 70, 7
    x, w, b, gy = rng.standard_normal((M, K)), rng.standard_normal((No, K)), rng.standard_normal(No), rng.standard_normal((M, No))
    drop = np.where(rng.random((M, No)) < 0.2, 0.0, 1.25) if use_drop else None
    gw0, gb0 = rng.standard_normal((No, K)), rng.standard_normal(No)
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    y = F.linear(tx, tw, tb if use_b else None)
    if relu:
        y = F.relu(y)
    if use_drop:
        y = y * torch.tensor(drop)
    y.backward(torch.tensor(gy))
    yr = S.linear_ref(x, w, b if use_b else None, relu, drop)
    np.testing.assert_allclose(yr, y.detach().numpy(), rtol=1e-13, atol=1e-13)
    gx, gw, gb = S.linear_bwd_ref(x, w, yr, gy, relu, drop, gx_scale=-0.2, accumulate=1, gw0=gw0, gb0=gb0)
    np.testing.assert_allclose(gx, float(np.float32(-0.2)) * tx.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(gw, gw0 + tw.grad.numpy(), rtol=1e-12, atol=1e-13)
    if use_b:
        np.testing.assert_allclose(gb, gb0 + tb.grad.numpy(), rtol=1e-12, atol=1e-13)
    gx1, gw1, gb1 = S.linear_bwd_ref(x, w, yr, gy, relu, drop)
    np.testing.assert_allclose(gw1, tw.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(gx1, tx.grad.numpy(), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("M,C", [(1, 2), (4, 5), (33, 64)])
def test_softmax_ce_reference_is_torch_cross_entropy_in_float64(M, C):
    rng = np.random.default_rng(M * 100 + C)
    z = rng.standard_normal((M, C)) * 5
    z[0, 0], z[0, -1] = 80.0, -80.0
    z[M // 2] = 3.0
    lab = rng.integers(0, C, M)
    tz = torch.tensor(z, requires_grad=True)
    loss = F.cross_entropy(tz, torch.tensor(lab))
    (loss * -0.5).backward()
    rl, rd = S.softmax_ce_rows_ref(z, lab, -0.5)
    assert abs(rl - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    np.testing.assert_allclose(rd, tz.grad.numpy(), rtol=1e-12, atol=1e-16)


# ---------------------------------------------------------------------------------------------------- Dropout RNG
def test_dropout_generator_restatement():
    assert int(S._mix64(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF          # splitmix64's first output for seed 0
    seed, ctr = 0xF123456789ABCDEF, 0xFFFFFFFFFFFFFF00                                # the counter wraps inside the draw
    a, c1 = S.dropout_scales_ref(seed, ctr, 1000, 0.2)
    b, _ = S.dropout_scales_ref(seed, ctr, 1000, 0.2)
    assert a.dtype == np.float32 and np.array_equal(a, b) and c1 == (ctr + 1000) % 2 ** 64
    a1, c = S.dropout_scales_ref(seed, ctr, 300, 0.2)
    a2, c = S.dropout_scales_ref(seed, c, 700, 0.2)
    assert c == c1 and np.array_equal(np.concatenate([a1, a2]), a)                    # split draw == single draw
    assert set(np.unique(a).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.2)))}
    assert not np.array_equal(a, S.dropout_scales_ref(seed + 1, ctr, 1000, 0.2)[0])
    assert (S.dropout_scales_ref(seed, ctr, 1000, 0.0)[0] == 1.0).all()
    assert (S.dropout_scales_ref(seed, ctr, 1000, 1.0)[0] == 0.0).all()
    for p, c in S.RNG_EDGE_HITS.items():                                              # u == p exactly: kept (u >= p)
        assert float(S.dropout_uniforms_ref(S.RNG_EDGE_SEED, c - 3, 8)[3]) == p
        assert S.dropout_scales_ref(S.RNG_EDGE_SEED, c - 3, 8, p)[0][3] == (1.0 if p == 0 else 2.0)
    n = 1 << 20
    for p in (0.1, 0.5):
        keep = float((S.dropout_scales_ref(1234, 0, n, p)[0] != 0).mean())
        assert abs(keep - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


# ---------------------------------------------------------------------------------------------------- ABI arguments
def test_abi_rejects_bad_step_operator_arguments_without_launching():
    """Null pointers and non-positive sizes are argument errors (< 0) before anything is launched (this machine has no GPU:
    a launch would fail differently).  p is never dereferenced."""
    lib = _lib.lib()
    p = 4096
    assert lib.mi3d_linear_forward(p, p, p, p, 0, 8, 8, 0, None, None) < 0
    assert lib.mi3d_linear_forward(p, p, p, None, 4, 8, 8, 0, None, None) < 0
    for (M, K, No) in [(0, 8, 8), (4, 0, 8), (4, 8, 0), (-1, 8, 8)]:
        assert lib.mi3d_linear_backward(p, p, p, p, M, K, No, 1, None, p, p, p, 0, 1.0, p, None) < 0, (M, K, No)
        assert b"positive" in lib.mi3d_last_error()
    assert lib.mi3d_linear_backward(p, p, p, p, 4, 8, 8, 1, None, p, p, p, 0, 1.0, None, None) < 0     # no workspace
    assert lib.mi3d_linear_backward(None, p, p, p, 4, 8, 8, 1, None, p, p, p, 0, 1.0, p, None) < 0
    for (M, C) in [(0, 2), (-3, 2), (4, 0)]:
        assert lib.mi3d_softmax_ce_rows(p, p, M, C, p, p, 1.0, None) < 0, (M, C)
        assert b"positive" in lib.mi3d_last_error()
    assert lib.mi3d_softmax_ce_rows(p, p, 4, 65, p, p, 1.0, None) < 0 and b"> 64" in lib.mi3d_last_error()
    assert lib.mi3d_softmax_ce_rows(None, p, 4, 2, p, p, 1.0, None) < 0
    assert lib.mi3d_softmax_ce_rows(p, None, 4, 2, p, p, 1.0, None) < 0
    assert lib.mi3d_scale(p, p, -1, 1.0, None, None) < 0
    assert lib.mi3d_scale(None, p, 4, 1.0, None, None) < 0
    h = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0)
    assert lib.mi3d_adamw_step(p, p, p, p, -1, *h, p, None) < 0
    assert lib.mi3d_adamw_step(p, p, p, p, 4, *h, None, None) < 0
    assert lib.mi3d_adamw_step(p, None, p, p, 4, *h, p, None) < 0
    assert lib.mi3d_adamw_apply(p, p, p, None, 4, *h, p, 0, None) < 0
    assert lib.mi3d_adamw_apply(None, None, None, None, 0, *h, None, 1, None) < 0
    assert lib.mi3d_dropout_scales(p, 4, 1.5, p, None) < 0
    assert lib.mi3d_dropout_scales(p, 4, -0.1, p, None) < 0
    assert lib.mi3d_dropout_scales(p, -1, 0.5, p, None) < 0
    assert lib.mi3d_dropout_scales(p, 4, 0.5, None, None) < 0
    assert lib.mi3d_maxpool2_forward(0, p, 8, 8, 1, 1, 4, 4, p, 8, None) < 0
    assert lib.mi3d_maxpool2_backward(0, p, 8, p, 8, None, 8, p, 8, 8, 1, 4, 1, 4, None) < 0
    assert lib.mi3d_maxpool2_backward(0, p, 8, p, 8, None, 8, None, 8, 8, 1, 4, 4, 4, None) < 0
    assert lib.mi3d_ncdhw_to_ndhwc(0, None, p, 4, 4, 1, 8, None) < 0
    assert lib.mi3d_ndhwc_to_ncdhw(0, p, 4, None, 4, 1, 8, None) < 0
