"""CPU checks of tests/infer_ref.py: the conditions on the INPUTS that the bitwise claims of tests/test_gpu_conv_infer_ops.py rest
on, for every case of the table, and where each case lands among the inference forward's routes.  These are conditions, not
measurements: a case that misses one gets another seed (infer_ref.SEEDS), never another threshold.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402
import infer_ref as I  # noqa: E402

TABLE = {   # the issue's table, restated: name -> (Cin, Cout, dtype, geometry from conv_ref, route)
    "c1_16": ("c1_16", 1, 16, 1, (1, 1)), "c1_32": ("c1_32", 1, 32, 1, (1, 1)),
    "persist_thin": ("persist_thin", 16, 16, 1, (2, 1)), "persist_2chunk": ("persist_2chunk", 32, 16, 1, (2, 1)),
    "persist_2chunk_planar": ("persist_2chunk", 32, 16, 1, (2, 1)),
    "big_16_32": ("big_16_32", 16, 32, 1, (3, 1)), "big_32_32": ("big_32_32", 32, 32, 1, (3, 1)), "big_64_16": ("big_64_16", 64, 16, 1, (3, 1)),
    "small_16_32": ("small_16_32", 16, 32, 1, (4, 1)), "small_tiny": ("small_tiny", 16, 16, 1, (4, 1)),
    "sk2_32_64": ("sk2_32_64", 32, 64, 1, (4, 2)), "sk2_32_16": ("sk2_32_16", 32, 16, 1, (4, 2)), "sk4_64_128": ("sk4_64_128", 64, 128, 1, (4, 4)),
    "sk8_128_256": ("sk8_128_256", 128, 256, 1, (4, 8)), "sk16_256_256": ("sk16_256_256", 256, 256, 1, (4, 16)),
    "direct_f32": ("direct_f32", 4, 5, 0, (0, 1)), "direct_bf16": ("direct_f32", 2, 5, 1, (0, 1)),
}


def test_table_is_the_issues_table():
    assert list(I.CASES) == list(TABLE)
    for name, (geo_of, cin, cout, dtype, route) in TABLE.items():
        c = I.CASES[name]
        assert (c["cin"], c["cout"], c["dtype"], c["geo"], c["route"]) == (cin, cout, dtype, R.CASES[geo_of]["geo"], route), name
    assert not {"persist_16_32", "persist_wide", "small_finalize", "sk4_256_256"} & set(I.CASES)
    assert I.CASES["persist_2chunk_planar"]["planar"] and I.case_data("persist_2chunk_planar")["x"] is I.case_data("persist_2chunk")["x"]


@pytest.mark.parametrize("name", list(I.CASES))
def test_case_inputs_make_the_folded_conv_exact(name):
    k = I.case_data(name)
    cout = k["cout"]
    # the draws are the issue's
    assert k["eps"] == 0.0 and set(np.unique(k["rv"])) <= set(I.VARS) and set(np.unique(k["scale"])) <= set(I.SCALES)
    assert np.array_equal(k["gamma"].astype(np.float64), k["scale"] * np.sqrt(k["rv"].astype(np.float64)))
    assert np.array_equal(k["rm"] * 4, np.round(k["rm"] * 4)) and np.abs(k["rm"]).max() <= 2
    assert np.array_equal(k["beta"] * 8, np.round(k["beta"] * 8)) and np.abs(k["beta"]).max() <= 1
    assert np.abs(k["b"]).max() <= 2          # offset=False
    # the bf16 weight image is exact, the folded bias is exact in fp32
    ws = k["w"].astype(np.float64) * k["scale"].reshape(-1, 1, 1, 1, 1)
    assert np.array_equal(R.bf16_rne(ws).astype(np.float64), ws), name
    assert np.array_equal(k["fbias"].astype(np.float32).astype(np.float64), k["fbias"])
    margin = R.exactness_margin(k["x"], ws, k["fbias"])
    assert margin < 2 ** 24, (name, margin)
    # products are multiples of 1/512, not of 1/128: the condition that makes every partial sum exact is four times as strict
    assert 4 * margin < 2 ** 24, (name, 4 * margin)
    assert np.array_equal(k["pre"] * 512, np.round(k["pre"] * 512))
    assert np.array_equal(k["pre"].astype(np.float32).astype(np.float64), k["pre"])
    # the ReLU has work to do in every direction
    pre = k["pre"]
    neg, pos = float((pre < 0).mean()), float((pre > 0).mean())
    both = int(((pre < 0).any(axis=(0, 2, 3, 4)) & (pre > 0).any(axis=(0, 2, 3, 4))).sum())
    ties = int(R.is_tie(k["exact"].astype(np.float32))[pre >= 0].sum())
    print(f"{name}: margin {margin:.0f}, {neg:.3f} negative, {pos:.3f} positive, {both}/{cout} channels with both signs, {ties} exact ties")
    assert neg >= 0.25 and pos >= 0.25, (name, neg, pos)
    assert 2 * both >= cout, (name, both)
    assert ties >= 1, name
    assert I.predict_infer_route(k) == k["route"], name


def test_fold_f64_on_the_exact_draws_and_by_hand():
    k = I.case_data("persist_thin")
    assert np.array_equal(k["fbias"], (k["b"].astype(np.float64) - k["rm"]) * k["scale"] + k["beta"])
    s, f = I.fold_f64([2.0], [0.5], [1.0], [4.0], None, 0.0)
    assert s[0] == 1.0 and f[0] == -0.5                     # bias None = 0: (0 - 1) * 1 + 0.5
    s, f = I.fold_f64([3.0], [0.0], [0.0], [0.0], [2.0], I.EPS_REAL)
    assert s[0] == 3.0 / np.sqrt(np.float64(np.float32(1e-5))) and f[0] == 2.0 * s[0]


def test_infer_f64_is_relu_of_the_conv_with_scaled_weights():
    k = I.case_data("direct_f32")
    y = R.conv3d_f64(k["x"], k["w"], np.zeros(k["cout"]))
    want = np.maximum(y * k["scale"].reshape(1, -1, 1, 1, 1) + k["fbias"].reshape(1, -1, 1, 1, 1), 0.0)
    np.testing.assert_array_equal(I.infer_f64(k["x"], k["w"], k["scale"], k["fbias"]), want)      # exact inputs: no rounding anywhere
    assert (want == 0).mean() > 0.25


def test_route_prediction_under_the_switches_and_strides():
    for name in I.TILE_CASES:             # the four-wave kernels keep the code and the split factor
        assert I.predict_infer_route(I.CASES[name], {"conv8": 0}) == I.CASES[name]["route"], name
    for name in I.PERSIST_CASES:
        assert I.predict_infer_route(I.CASES[name], {"no_persist": 1}) == (3, 1), name
        assert not R.persist_ok(I.CASES[name]["cin"], I.CASES[name]["cout"], I.CASES[name]["geo"], dict(R.DEFAULT_ROUTES, no_persist=1))
    for name in ("small_16_32", "sk2_32_16"):          # rows of Cout + 4 bf16 are not 16-byte aligned: no split-K scratch
        c = I.CASES[name]
        assert (c["cout"] + 4) % 8 != 0 and (c["cout"] + 4) % 4 == 0
        assert I.predict_infer_route(c, None, c["cout"] + 4) == (4, 1), name
    for name in ("c1_16", "persist_thin", "big_16_32", "big_64_16", "sk2_32_64", "direct_bf16"):      # the concat buffer's stride
        c = I.CASES[name]
        assert I.predict_infer_route(c, None, 2 * c["cout"]) == c["route"], name
    assert {c["route"] for c in I.CASES.values()} == {(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (4, 2), (4, 4), (4, 8), (4, 16)}


@pytest.mark.parametrize("name", I.REAL_CASES)
def test_real_eps_bound_is_derived_and_small(name):
    """the bound of the real-eps cases: positive everywhere, made of the derived terms only, and far below the values it guards
    (a kernel that dropped the ReLU would miss it)"""
    k = I.real_case_data(name)
    assert k["eps"] == float(np.float32(1e-5)) and (k["rv"] == 0.0).sum() >= 1 and k["rv"].max() <= 4.0
    assert k["rv"][k["rv"] > 0].min() >= np.float32(0.05)
    assert (k["bound"] > 0).all()
    pre = I.conv_folded_f64(k["x"], k["w"], k["scale"], k["fbias"])
    assert (pre < 0).mean() > 0.25 and (pre > 0).mean() > 0.25
    # dropping the ReLU moves the negative outputs by |pre|: beyond the bound for nearly all of them
    assert (np.abs(pre[pre < 0]) > k["bound"][pre < 0]).mean() > 0.95


def test_f32_neighbours():
    v = np.array([1.0, -3.5, 1e-3])
    nb = I.f32_neighbours(v)
    assert nb.shape == (3, 3) and (nb[0] < nb[1]).all() and (nb[1] < nb[2]).all()
    assert nb[2][0] == np.float32(1 + 2.0 ** -23) and nb[0][0] == np.float32(1 - 2.0 ** -24)
