"""CPU checks of tests/conv_bwd_ref.py: the exactness condition of the dyadic inputs per case, the case table against the Python
restatement of the route predicates, the fp32 accumulation bound against float32 numpy restatements in two orders, and the float64
reference against the C oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bwd_ref as B  # noqa: E402
import conv_ref as R  # noqa: E402


@pytest.mark.parametrize("name", list(B.CASES))
def test_dyadic_partial_sums_are_exact_in_fp32(name):
    """The condition of the module docstring, per case (the large case by its convolution-free upper bounds), for the plain run and
    for the accumulate = 1 run onto the dyadic prefill (multiples of 1/4 = 16/64: same unit; run at the oracle-sized cases)."""
    k = B.case_data(name)
    mw, mx, mb = B.exactness_margins(k["x"], k["w"], k["dy"], exact=k["oracle"])
    pre = 64.0 * float(np.abs(k["pre_w"]).max())
    f = 2 if k["oracle"] else 1
    assert f * mw + pre < 2 ** 24 and mx < 2 ** 24 and f * mb + 8 * float(np.abs(k["pre_b"]).max()) < 2 ** 24, (name, mw, mx, mb)
    for q in ("x", "w", "dy", "dz", "y"):            # every input is a bf16 number: the device tensors hold exactly these values
        if k["dtype"] == 1 and not (q == "x" and k["cin"] == 1):
            assert (R.bf16_rne(k[q]) == k[q]).all(), (name, q)
    if k["dx"] is not None:                          # the cases are not trivial: some dx need rounding to bf16
        assert k["dtype"] == 0 or (R.bf16_rne(k["dx"]) != k["dx"]).any()


@pytest.mark.parametrize("name", list(B.CASES))
def test_case_table_is_what_the_predicates_say(name):
    c = B.CASES[name]
    assert B.predict_route(c) == c["route"], (name, B.predict_route(c), c["route"])
    cin, cout, g = c["cin"], c["cout"], c["geo"]
    r = B.DEFAULT_ROUTES
    want = {"persist_11": 2, "persist_12": 2, "persist_21": 2, "big_32_32": 3, "big_32_16": 3, "small_32_16": 4, "sk2_64_32": 4,
            "sk8_128_256": 4, "sk16_256_256": 4, "pair_16_32": 5, "pair_48_16": 5, "c1_16": 1, "direct_f32": 0}[name]
    assert c["route"]["conv"] == want
    if name == "persist_21":
        assert R.tiles16(g) == 1152 and B.fused_persist_ok(cin, cout, g, r) and not B.bn_small(cout, np.prod(g), r)
    if name == "big_32_16":
        assert R.tiles16(g) < R.PERSIST_16_32_TILES and not B.fused_persist_ok(cin, cout, g, r)
    if name in B.FUSED_CASES:                        # the deferred pair cuts the slabs like the fused launch, at its split factor
        d = B.predict_route(c, flags=B.DEFER)
        assert (d["conv"], d["slabs"], d["dgrad_ks"]) == (6, c["route"]["slabs"], c["route"]["dgrad_ks"])
        assert B.wg_target(cin, cout, cin, g, r) == (R.CUS if want == 2 else B.FUSED_WGRAD_TARGET)
    if name in B.SPLITK_CASES:
        assert B.predict_route(c, flags=B.ALLOW_PARTIALS)["dx_ks"] == (c["route"]["dgrad_ks"] if want == 4 else 0)
        assert B.predict_route(c, {"no_defer_tail": 1}, flags=B.ALLOW_PARTIALS)["dx_ks"] == 0


def test_predicates_under_the_route_switches():
    c = B.CASES
    assert B.predict_route(c["persist_11"], {"no_fused_bwd_p": 1})["conv"] == 5           # 16 -> 16: Cin % 32 != 0, no generic fusion
    assert B.predict_route(c["persist_21"], {"no_fused_bwd_p": 1})["conv"] == 5           # its input gradient stays persistent
    assert B.predict_route(c["persist_21"], {"no_persist": 1})["conv"] == 3
    assert B.predict_route(c["big_32_32"], {"no_fused_bwd_big": 1})["conv"] == 5
    assert B.predict_route(c["sk2_64_32"], {"no_fused_bwd_big": 1})["conv"] == 4          # the switch is about the 16-wide tile only
    for name in B.FUSED_CASES:
        p = B.predict_route(c[name], {"no_fused_bwd": 1})
        assert p["conv"] == 5 and p["slabs"] == B.wgrad_slabs(c[name]["cin"], c[name]["cout"], c[name]["geo"], 0)
    assert B.predict_route(c["sk2_64_32"], {"no_small_bn": 1})["bn"] == 1
    # slab counts of wgrad_cfg for the three targets at a shape where they differ: 3 x 8 x 9 = 216 tiles... of a 32 -> 32 layer
    g = (1, 12, 64, 144)
    assert R.tiles16(g) == 216 and [B.wgrad_slabs(32, 32, g, t) for t in (0, 256, 288)] == [108, 54, 72]
    assert B.slab_sum(False, 256, 128) == (2, 0) and B.slab_sum(False, 128, 128)[0] == 1
    assert B.slab_sum(False, 16, 32) == (1, 8) and B.slab_sum(False, 32, 32) == (1, 32) and B.slab_sum(True, 1, 16) == (0, 4)
    assert B.vec8_ok(16, 16, 32) and not B.vec8_ok(5, 5) and not B.vec8_ok(8, 12)


def _terms_dw(x, dy):
    """float32 products x[v + tap, ci] * dy[v, co] as [M][Cout][Cin][27]"""
    n, cin, d, h, w = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))
    cols = [xp[:, :, a:a + d, b:b + h, c:c + w] for a in range(3) for b in range(3) for c in range(3)]
    xs = np.stack(cols, axis=-1).transpose(0, 2, 3, 4, 1, 5).reshape(-1, 1, cin, 27)
    return xs * dy.transpose(0, 2, 3, 4, 1).reshape(-1, dy.shape[1], 1, 1)


def _terms_dx(dy, w):
    """float32 products dy[v - tap, co] * w[co, ci, tap] as [27 * Cout][N][Cin][D][H][W]"""
    n, cout, d, h, ww = dy.shape
    dp = np.pad(dy, ((0, 0), (0, 0), (1, 1), (1, 1), (1, 1)))
    out = []
    for a in range(3):
        for b in range(3):
            for c in range(3):
                sh = dp[:, :, 2 - a:2 - a + d, 2 - b:2 - b + h, 2 - c:2 - c + ww]
                out += [sh[:, co, None] * w[None, co, :, a, b, c, None, None, None] for co in range(cout)]
    return np.stack(out)


def _sum_two_orders(t):
    """float32 sums over axis 0: one sequential chain, and pairwise within tiles of 64 terms then a chain over the tiles"""
    seq = np.add.accumulate(t, axis=0, dtype=np.float32)[-1]
    tiles = [t[i:i + 64].sum(axis=0, dtype=np.float32) for i in range(0, t.shape[0], 64)]
    return seq, np.add.accumulate(np.stack(tiles), axis=0, dtype=np.float32)[-1]


@pytest.mark.parametrize("name", ["pair_48_16", "direct_f32", "small_32_16"])
def test_acc_bound_holds_for_float32_restatements(name):
    """Non-dyadic dy (bf16 numbers for the bf16 cases): fp32 sums of the exact products, sequentially and pairwise over tiles, stay
    inside acc_bound against the float64 gradients; a bf16 dx inside acc_bound + half a spacing."""
    k = B.case_data(name)
    rng = np.random.default_rng(5)
    dy = rng.standard_normal(k["dy"].shape).astype(np.float32)
    if k["dtype"] == 1:
        dy = R.bf16_rne(dy)
    x, w = k["x"], k["w"]
    gx, gw, gb = B.conv3d_bwd_f64(x, w, dy)
    bx, bw, bb = B.conv_bwd_bounds(x, w, dy, k["cout"], k["dtype"] == 1, gx)
    assert (bw > 0).all() and (bw < 1e-2 * np.abs(gw).max()).all()                   # the bound is a real constraint
    for got in _sum_two_orders(_terms_dw(x, dy)):
        got = got.reshape(k["cout"], k["cin"], 27).astype(np.float64)
        assert (np.abs(got - gw.reshape(k["cout"], k["cin"], 27)) <= bw.reshape(k["cout"], k["cin"], 27)).all()
    for got in _sum_two_orders(dy.transpose(0, 2, 3, 4, 1).reshape(-1, k["cout"])):
        assert (np.abs(got.astype(np.float64) - gb) <= bb).all()
    for got in _sum_two_orders(_terms_dx(dy, w)):
        if k["dtype"] == 1:
            got = R.bf16_rne(got)
        assert (np.abs(got.astype(np.float64) - gx) <= bx).all()


@pytest.mark.parametrize("name", [n for n, c in B.CASES.items() if c["oracle"]])
def test_float64_reference_agrees_with_the_c_oracle(orc, name):
    """Dyadic inputs: the oracle's fp32 outputs are the float64 values rounded once.  BatchNorm backward: the oracle against the
    float64 restatement with the same saved statistics, to fp32 rounding of values of that size."""
    k = B.case_data(name)
    gx, gw, gb = orc.conv3d_bwd(k["x"], k["w"], k["dy"])
    np.testing.assert_array_equal(gw, k["dW"].astype(np.float32))
    np.testing.assert_array_equal(gb, k["db"].astype(np.float32))
    if k["dx"] is not None:
        np.testing.assert_array_equal(gx, k["dx"].astype(np.float32))
    mean, inv, a, b = k["stat"]
    dy, dg, dbeta = B.bn_bwd_f64(k["y"], k["dz"], k["scale"], k["gamma"], mean, inv, a, b)
    yhat = (k["y"].astype(np.float64) * a.reshape(1, -1, 1, 1, 1) + b.reshape(1, -1, 1, 1, 1)).astype(np.float32)
    dyh = orc.relu_drop_bwd(yhat, k["dz"], k["scale"])
    o_dy, o_dg, o_db = orc.bn_train_bwd(k["y"], dyh, k["gamma"], mean, inv)
    np.testing.assert_allclose(o_db, dbeta, rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(o_dg, dg, rtol=2.0 ** -23, atol=2.0 ** -23 * float(np.abs(dg).max()))
    np.testing.assert_allclose(o_dy, dy, rtol=2.0 ** -22, atol=2.0 ** -22 * float(np.abs(dy).max()))
