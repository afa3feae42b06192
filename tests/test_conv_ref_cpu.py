"""CPU checks of tests/conv_ref.py: the conditions the bitwise claims of tests/test_gpu_conv_fwd_ops.py (and of the tightened
per-operator conv tests) rest on, and where each case of the table lands among the forward's routes.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

# Share of outputs that are not bf16 numbers.  An output is a multiple of 1/128; it is a bf16 number iff |y| < 2 or its low bits
# vanish, so of the outputs with |y| >= 2 at least half (the odd multiples) are not.  The bias offset (integers in [-8, 8]) puts
# |bias| >= 2 on about 13 of 17 channels, and the sum of >= 27 products spreads y by >= 0.5 around it: a floor of one fifth
# holds with room on every bf16 case.
MIN_INEXACT_SHARE = 0.2
BF16_CASES = [k for k, c in R.CASES.items() if c["dtype"] == 1]


def test_bf16_rne_is_torchs_cpu_conversion_ties_included():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 37, (rng.integers(-4096, 4097, 4096) / 128).astype(np.float32),
                        np.array([0.0, -0.0, 2 + 1 / 128, 2 + 3 / 128, -(2 + 1 / 128), 3 + 127 / 128, 255.5, 256.5 + 0.5, 1e-30, 3e38],
                                 np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16)
    np.testing.assert_array_equal(R.bf16_bits(a).view(np.int16), want.view(torch.int16).numpy())
    np.testing.assert_array_equal(R.bf16_rne(a), want.float().numpy())
    ties = R.is_tie(a)
    assert ties[8192 + 2] and ties[8192 + 3] and ties[8192 + 4] and not ties[8192]
    # a tie goes to the even neighbour: 2 + 1/128 -> 2 (mantissa 0), 2 + 3/128 -> 2 + 4/128
    assert R.bf16_rne(np.float32(2 + 1 / 128)) == 2.0 and R.bf16_rne(np.float32(2 + 3 / 128)) == np.float32(2 + 4 / 128)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_inputs_make_fp32_accumulation_exact(name):
    k = R.case_data(name)
    margin = R.exactness_margin(k["x"], k["w"], k["b"])
    assert margin < 2 ** 24, (name, margin)
    # everything is a multiple of 1/128, so float32 holds the exact value
    assert np.array_equal(k["exact"] * 128, np.round(k["exact"] * 128))
    assert np.array_equal(k["exact"].astype(np.float32).astype(np.float64), k["exact"])


@pytest.mark.parametrize("name", BF16_CASES)
def test_rounding_shows_in_the_statistics(name):
    """statistics of the rounded values != statistics of the accumulators, by more than the GPU test allows"""
    k = R.case_data(name)
    inexact = k["y_ref"].astype(np.float64) != k["exact"]
    share, ties = float(inexact.mean()), int(R.is_tie(k["exact"].astype(np.float32)).sum())
    print(f"{name}: {share:.3f} of the outputs are not bf16 numbers, {ties} exact ties, max|y| {np.abs(k['exact']).max():.2f}")
    assert share >= MIN_INEXACT_SHARE, (name, share)
    a, b = k["st"], k["st_acc"]
    d_mean = np.abs(a["mean"] - b["mean"]) / (1e-6 * np.abs(a["mean"]) + 1e-6)
    d_inv = np.abs(a["inv"] - b["inv"]) / (2e-6 * np.abs(a["inv"]))
    assert max(d_mean.max(), d_inv.max()) > 4.0, (name, d_mean.max(), d_inv.max())


def test_exact_ties_occur():
    n = {name: int(R.is_tie(R.case_data(name)["exact"].astype(np.float32)).sum()) for name in BF16_CASES if R.CASES[name]["oracle"]}
    assert all(v > 0 for v in n.values()), n
    # and both directions of a tie are taken: rounded up and rounded down
    k = R.case_data("persist_thin")
    t = R.is_tie(k["exact"].astype(np.float32))
    diff = (k["y_ref"].astype(np.float64) - k["exact"])[t]
    assert (diff > 0).any() and (diff < 0).any()


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items() if c["oracle"]])
def test_reference_agrees_with_the_c_oracle(orc, name):
    k = R.case_data(name)
    np.testing.assert_array_equal(orc.conv3d_fwd(k["x"], k["w"], k["b"]), k["exact"].astype(np.float32))
    if k["dtype"] == 1 and name in ("persist_thin", "sk2_32_64", "c1_16"):
        # the oracle's BatchNorm of the rounded values against the float64 statistics
        _, sm, si, rm, rv = orc.bn_train_fwd(k["y_ref"], k["gamma"], k["beta"], k["rm0"], k["rv0"], R.MOMENTUM, R.EPS)
        np.testing.assert_allclose(sm, k["st"]["mean"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(si, k["st"]["inv"], rtol=1e-6)
        np.testing.assert_allclose(rm, k["st"]["rm"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(rv, k["st"]["rv"], rtol=1e-6)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_lands_on_the_route_the_table_names(name):
    c = R.CASES[name]
    assert R.predict_route(c) == c["route"], name
    n, d, h, w = c["geo"]
    if c["pooled"]:
        assert d % 2 == 0 and h % 2 == 0 and w % 2 == 0


def test_table_reaches_every_route_and_every_consumer():
    routes = [c["route"] for c in R.CASES.values()]
    assert {r["conv"] for r in routes} == {0, 1, 2, 3, 4}
    assert {r["ksplit"] for r in routes} == {1, 2, 4, 8, 16}
    assert {r["consumer"] for r in routes if r["stats"] == 1} == {"thin", "wide"}
    assert {r["stats"] for r in routes} == {0, 1, 2}
    # ragged on purpose: some side of every MFMA case but the pooled ones is no multiple of its tile
    for name, c in R.CASES.items():
        if c["route"]["conv"] in (1, 2, 3, 4) and not c["pooled"]:
            n, d, h, w = c["geo"]
            tx = 8 if c["route"]["conv"] == 4 else 16
            assert d % 4 or h % 8 or w % tx, name
    # the persistent 16 -> 32 kernel needs >= 1024 tiles; one tile less and the case would silently run the 16-wide kernel
    assert R.tiles16(R.CASES["persist_16_32"]["geo"]) >= R.PERSIST_16_32_TILES
    assert R.CASES["persist_wide"]["route"]["rows"] > R.SMALL_ROWS and R.CASES["small_finalize"]["route"]["rows"] > R.WIDE_ROWS


def test_route_switches_move_the_cases_as_the_gpu_test_expects():
    for name in R.SPLITK_CASES:
        c = R.CASES[name]
        for sw in ({"splitk_ticket": 0}, {"conv8": 0}):
            r = R.predict_route(c, sw)
            assert (r["conv"], r["ksplit"], r["ticket"], r["stats"]) == (4, c["route"]["ksplit"], 0, 3), (name, sw, r)
            assert 1 <= r["rows"] <= R.SMALL_ROWS
    for name in R.PERSIST_CASES:
        r = R.predict_route(R.CASES[name], {"no_persist": 1})
        tiles = R.tiles16(R.CASES[name]["geo"])           # one row per tile: 1152 rows (persist_16_32) need the finalize launch
        assert r["conv"] == 3 and r["rows"] == tiles and r["stats"] == (1 if tiles <= R.WIDE_ROWS else 2), (name, r)
    for name in R.ROW_FED_CASES:
        r = R.predict_route(R.CASES[name], {"wide_bn": 0})
        assert r["stats"] == 2 and r["rows"] == R.CASES[name]["route"]["rows"], (name, r)
    assert set(R.ONE_PASS_MFMA_CASES) == {"big_16_32", "big_32_32", "big_64_16", "small_16_32", "small_tiny", "small_finalize"}


def _shapes(fn):
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == "shape":
            return list(mark.args[1])
    return []


def test_existing_conv_tests_inputs_meet_the_exactness_condition():
    """The tightened tests (test_conv3_mfma_vs_c_oracle, test_conv3_backward_kernels_of_the_step_exact,
    test_conv3_fused_persist_16to32_exact, test_upconv_mfma_vs_c_oracle, test_upconv_backward_exact) draw x, dy in k/8 and w in
    k/16 with |k| <= 8 (bias k/4): |x*w| <= 1/2 in units of 1/128.  Worst case over ANY draw: a 3x3x3 conv sums 27*C products
    (C = Cin for y, Cout for dx), a 2x2x2 stride-2 transposed conv Cin products for y and 8*Cout for dx."""
    import test_gpu_parity as P
    import test_gpu_round2 as R2
    lim = 2 ** 24
    conv = _shapes(P.test_conv3_mfma_vs_c_oracle) + _shapes(R2.test_conv3_backward_kernels_of_the_step_exact) + [(1, 32, 16, 64, 64, 128)]
    up = _shapes(P.test_upconv_mfma_vs_c_oracle) + _shapes(R2.test_upconv_backward_exact)
    assert len(conv) >= 15 and len(up) >= 9
    for n, cin, cout, d, h, w in conv:
        assert 128 * (27 * cin * 0.5 + 2) < lim and 128 * 27 * cout * 0.5 < lim
    for n, cin, cout, d, h, w in up:
        assert 128 * (cin * 0.5 + 2) < lim and 128 * 8 * cout * 0.5 < lim


def test_statistics_pass_needs_double_sums_where_the_mean_is_large():
    """bn_stats_kernel on direct_f32 (fp32, M = 1530, C = 5: 30 blocks of 51 rows, one row per thread), restated in numpy.  Running
    fp32 block sums of y^2 (what the kernel did before) miss the invstd allowance of 2e-6 where |mean| is about 6 std; double
    sums rounded to fp32 once per block (what it does now) keep it."""
    k = R.case_data("direct_f32")
    assert R.predict_route(k)["stats"] == 0
    y = np.ascontiguousarray(k["exact"].astype(np.float32).transpose(0, 2, 3, 4, 1)).reshape(-1, k["cout"])
    m, rows = y.shape[0], 51                          # BLK / C rows per block
    assert m == 30 * rows
    f = np.float32

    def inv_of(block_sums):
        s, q = np.zeros(k["cout"]), np.zeros(k["cout"])
        for b in range(0, m, rows):
            bs, bq = block_sums(y[b:b + rows])
            s, q = s + bs.astype(np.float64), q + bq.astype(np.float64)
        mean = s / m
        return 1.0 / np.sqrt(q / m - mean * mean + np.float64(f(R.EPS)))

    def running_fp32(blk):
        a0, a1 = np.zeros(k["cout"], f), np.zeros(k["cout"], f)
        for row in blk:
            a0, a1 = a0 + row, a1 + row * row
        return a0, a1

    def double_once(blk):
        d = blk.astype(np.float64)
        return d.sum(0).astype(f), (d * d).astype(f).astype(np.float64).sum(0).astype(f)      # a thread's y^2 rounded, then the block sum

    ref = k["st"]["inv"]
    err_old, err_new = np.abs(inv_of(running_fp32) - ref) / ref, np.abs(inv_of(double_once) - ref) / ref
    print("invstd relative error per channel: running fp32", err_old, "double", err_new)
    assert err_old.max() > 2e-6 and err_new.max() < 0.5e-6
    ratio = (k["st"]["mean"] ** 2 + k["st"]["var"]) / k["st"]["var"]
    assert ratio.max() > 30          # the magnification of one rounding of the sum of squares
