"""CPU checks of tests/up_ref.py, the reference and case table of tests/test_gpu_up_ops.py: the float64 transposed conv against
torch and the C oracle, every route claim of the table against the Python launch predicates, the exactness condition of the dyadic
data, the share of outputs that rounding changes, the fused backward's interleave map, and the resize adjoint's candidate window
against torch for every (in, out) of the sweep."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import up_ref as U  # noqa: E402

MIN_INEXACT_SHARE = 0.2          # the floor of tests/test_conv_ref_cpu.py
# dx = sum of 8 Cout >= 128 products k1 k2 / 128 with k uniform on -8..8 (variance 24 each, 576 per product): standard deviation
# >= 271 grid steps, so P(256 <= |k| < 512) ~ 0.29 (half of those odd) and P(|k| >= 512) ~ 0.06 (three quarters not representable):
# 0.187 at Cout = 16, more above.  There is no bias to move dx, so its floor is set below that figure, not at 0.2.
MIN_INEXACT_SHARE_DX = 0.15
ORACLE_CASES = [k for k, c in U.all_cases().items() if c["oracle"]]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_float64_reference_is_torchs_transposed_conv_and_the_c_oracle(orc, name):
    k = U.case_data(name)
    x, w, b, gy = (torch.from_numpy(np.asarray(k[q], np.float64)) for q in ("x", "w", "b", "gy"))
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = torch.nn.functional.conv_transpose3d(x, w, b, stride=2)
    y.backward(gy)
    for got, want in ((k["y"], y.detach()), (k["dx"], x.grad), (k["dW"], w.grad), (k["db"], b.grad)):
        assert (got == want.numpy()).all()                 # dyadic data: float64 sums are exact in any order
    oy = orc.convT2_fwd(k["x"], k["w"], k["b"])
    ox, ow, ob = orc.convT2_bwd(k["x"], k["w"], k["gy"])
    for got, want in ((oy, k["y"]), (ox, k["dx"]), (ow, k["dW"]), (ob, k["db"])):
        assert (got.astype(np.float64) == want).all()      # ... and so are the oracle's fp32 sums (exactness condition below)


def test_resize_reference_adjoint_matches_its_forward():
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, (2, 3, 5, 3, 7)).astype(np.float64)
    gy = rng.integers(-8, 9, (2, 3, 12, 8, 16)).astype(np.float64)
    assert float((U.nearest_f64(x, (12, 8, 16)) * gy).sum()) == float((x * U.nearest_bwd_f64(gy, (5, 3, 7))).sum())


@pytest.mark.parametrize("name", list(U.all_cases()))
def test_table_route_is_the_predicates_route(name):
    c = U.all_cases()[name]
    assert U.fwd_route(c["dtype"], c["cin"], c["cout"], c["geo"]) == c["fwd"], name
    if c["bwd"] is not None:
        assert U.bwd_route(c["dtype"], c["cin"], c["cout"], c["geo"]) == c["bwd"], name


def _ranges(name):
    c = U.CASES[name]
    return U.interleave_ranges(c["bwd"]["wgrad_blocks"], c["bwd"]["dgrad_blocks"])


def test_every_named_branch_has_a_case():
    C, m = U.CASES, lambda c: c["geo"][0] * c["geo"][1] * c["geo"][2] * c["geo"][3]  # noqa: E731
    f = lambda n: C[n]["fwd"]  # noqa: E731
    b = lambda n: C[n]["bwd"]  # noqa: E731
    # forward: hoist + wide with a ragged last group; tap split; wide at KS = 2, 4, 8 with gy = COBN; the cob loop at KS = 2 and 8;
    # the grid-stride loop
    assert C["hoist_wide"]["cin"] == 32 and f("hoist_wide")["wide"] == 1 and m(C["hoist_wide"]) % 16 == 2
    assert f("tapsplit_ksp8")["tap_split"] == 1 and f("tapsplit_ksp8")["wide"] == 0
    for n, ks in (("wide_ks2", 2), ("wide_ks4", 4), ("wide_ks8", 8)):
        assert C[n]["cin"] // 32 == ks and f(n)["wide"] == 1 and f(n)["tap_split"] == 0 and f(n)["gy"] == C[n]["cout"] // 16
    assert m(C["wide_ks2"]) % 16 == 1
    for n in ("wide_cob_ks2", "wide_cob_ks8"):
        assert f(n)["wide"] == 1 and f(n)["gy"] < C[n]["cout"] // 16
    assert f("stride_hoist")["strided"] == 1 and m(C["stride_hoist"]) > 262144 and all(f(n)["strided"] == 0 for n in C if n != "stride_hoist")
    # an unaligned up half: all 8 taps in one workgroup, narrow stores
    c = C["wide_ks2"]
    assert U.fwd_route(1, c["cin"], c["cout"], c["geo"], ucs=2 * c["cout"] + 8, aligned=False) == dict(f("wide_ks2"), wide=0)
    # backward: S = 4 / 8 / 16 / 32 without the K split, each persistent; the K split at S = 8 and 32
    for n, s in (("persist_s4", 4), ("wide_ks2", 8), ("wide_ks4", 16), ("wide_ks8", 32)):
        assert C[n]["cout"] // 4 == s and b(n)["ksplit"] == 0 and b(n)["persistent"] == 1
    assert b("tapsplit_ksp8")["ksplit"] == 1 and b("wsurplus_ksp32")["ksplit"] == 1 and b("hoist_wide")["persistent"] == 0
    # the interleave map's ranges
    assert _ranges("hoist_wide") == (0, 4, 6, "d") and _ranges("persist_s4")[:2] == (128, 10) and _ranges("tapsplit_ksp8")[:2] == (32, 12)
    assert _ranges("wsurplus_ksp32") == (32, 0, 16, "w") and _ranges("middle_32_128") == (0, 8, 0, "")
    assert m(C["persist_s4"]) % 128 == 71 and m(C["tapsplit_ksp8"]) % 16 == 7 and m(C["tapsplit_ksp8"]) % 128 == 7
    # the stand-alone pair cuts other slabs than the fused launch
    c = C["wide_ks2"]
    assert b("wide_ks2")["slabs"] == 96 and U.bwd_route(1, c["cin"], c["cout"], c["geo"], routes={"no_fused_upbwd": 1})["slabs"] == 128
    # Cout = 16 beside Cin / 32 > 1, both slab-sum widths
    assert (C["cout16_cin128"]["cout"], b("cout16_cin128")["slab_ew"], b("cout16_cin64")["slab_ew"]) == (16, 32, 8)
    # direct kernels: odd channels, a 32-channel block tail, two ci blocks, the weight kernel striding over tiles, bf16 shapes the
    # MFMA path rejects
    D = U.DIRECT_CASES
    assert all(c["fwd"]["kind"] == 0 and c["bwd"]["kind"] == 0 for c in D.values())
    assert D["f32_tail"]["cin"] % 32 == 24 and D["f32_tail"]["cout"] % 8 == 4 and D["f32_two_ci"]["cin"] == 32 + 8
    assert U.cdiv(m(D["f32_tiles"]), U.UV_DIRECT) > D["f32_tiles"]["bwd"]["slabs"] == 512
    assert all(not U.mfma_supported(D[n]["cin"], D[n]["cout"], 8, 8) for n in D if D[n]["dtype"] == 1)
    for (n, cin, cout, d, h, w), go in U.RESIZED_CASES.values():
        assert U.fwd_route(1, cin, cout, (n, d, h, w), go)["resized"] == 1 and U.bwd_route(1, cin, cout, (n, d, h, w), go)["kind"] == 1


@pytest.mark.parametrize("name", [k for k in U.all_cases() if k != "stride_hoist"])
def test_dyadic_data_keeps_every_partial_sum_exact(name):
    k = U.case_data(name)
    if k["bwd"] is None:
        m = (128.0 * float(U.convT2_f64(np.abs(k["x"]), np.abs(k["w"]), np.abs(k["b"])).max()),)
    else:
        m = U.exactness_margins(k["x"], k["w"], k["b"], k["gy"], k["dw0"], k["db0"])
    print(name, "grid steps:", m)
    assert max(m) < 2.0 ** 24, (name, m)


def test_grid_stride_case_is_exact_by_its_bound():
    """(1, 32, 16, 65, 64, 64): |y| <= |b| + sum over 32 channels of max|x| * max|w| per channel, no 34 M-element reference"""
    k = U.case_data("stride_hoist", need_ref=False)
    bound = 128.0 * (np.abs(k["b"]).max() + (np.abs(k["x"]).max(axis=(0, 2, 3, 4)) * np.abs(k["w"]).max(axis=(1, 2, 3, 4))).sum())
    assert bound < 2.0 ** 24


@pytest.mark.parametrize("name", list(U.CASES))
def test_rounding_changes_a_fifth_of_the_forward_outputs(name):
    """Share of y that is not a bf16 number (the bit check proves nothing on values that need no rounding).  Measured, y / dx:
    hoist_wide 0.256 / 0.190, persist_s4 0.258 / 0.188, tapsplit_ksp8 0.276 / 0.299, wide_ks2 0.275 / 0.299, wide_cob_ks2 0.274,
    wide_ks4 0.233 / 0.411, wide_ks8 0.328 / 0.519, wide_cob_ks8 0.324, wsurplus_ksp32 0.316 / 0.529, middle_32_128 0.255 / 0.497,
    cout16_cin128 0.224 / 0.191, cout16_cin64 0.273 / 0.189, stride_hoist 0.258 (its first two slices).  The K = 32 and K = 64
    cases carry |bias| = 2 on every channel (big_bias): with a bias drawn from all of k/4 they measured 0.10 - 0.19."""
    if name == "stride_hoist":
        k = U.case_data(name, need_ref=False)
        y = U.convT2_f64(k["x"][:, :, :2], k["w"], k["b"])
    else:
        k = U.case_data(name)
        y = k["y"]
    share = U.inexact_share(y)
    print(f"{name}: y {share:.3f}" + (f" dx {U.inexact_share(k['dx']):.3f}" if k["bwd"] is not None else ""))
    assert share >= MIN_INEXACT_SHARE, (name, share)
    if k["bwd"] is not None:
        assert U.inexact_share(k["dx"]) >= MIN_INEXACT_SHARE_DX, name


@pytest.mark.parametrize("name", U.BWD_CASES)
def test_interleave_map_is_a_bijection(name):
    b = U.CASES[name]["bwd"]
    nw, nd = b["wgrad_blocks"], b["dgrad_blocks"]
    seen = sorted(U.interleave(i, nw, nd) for i in range(nw + nd))
    assert seen == sorted([(False, i) for i in range(nd)] + [(True, i) for i in range(nw)]), name
    # idx = b >> 1 in the whole-groups range as well is no bijection: blocks of one kind would run twice and others never
    if U.interleave_ranges(nw, nd)[0] >= 16:
        assert len({U.interleave(i, nw, nd, mutant=True) for i in range(nw + nd)}) < nw + nd


def test_resize_adjoint_window_finds_torchs_destinations():
    """the new candidate range with the nn_src filter, in the kernel's float arithmetic, against F.interpolate for in 1..48 and
    out 1..3 in + 2; the range it replaces loses a destination on 1074 of those pairs, (5,12), (3,8), (7,16) among them"""
    missed_old = 0
    for n_in in range(1, 49):
        for n_out in range(1, 3 * n_in + 3):
            want = U.nearest_dests(n_in, n_out)
            got = U.gathered(U.window_new, n_in, n_out)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (n_in, n_out)
            old = U.gathered(U.window_old, n_in, n_out)
            lost = any(len(a) < len(b) for a, b in zip(old, want))
            missed_old += lost
            if (n_in, n_out) in ((5, 12), (3, 8), (7, 16)):
                assert lost, (n_in, n_out)
            if n_out in (n_in, n_in + 1):
                assert not lost, (n_in, n_out)            # what the plan asks for was never wrong
    assert missed_old == 1074, missed_old


def test_float_and_double_index_maps_differ_where_the_reference_says():
    """why the resize reference runs on float32 tensors: torch indexes a float64 tensor in double, and (24, 74) shows it"""
    a = torch.arange(24, dtype=torch.float32)
    f32 = torch.nn.functional.interpolate(a.reshape(1, 1, 24), size=74, mode="nearest").reshape(-1)
    f64 = torch.nn.functional.interpolate(a.double().reshape(1, 1, 24), size=74, mode="nearest").reshape(-1)
    assert (float(f32[37]), float(f64[37])) == (11.0, 12.0)
    bf = torch.nn.functional.interpolate(a.bfloat16().reshape(1, 1, 24), size=74, mode="nearest").reshape(-1)
    assert torch.equal(bf.float(), f32)                       # bfloat16 tensors index as float32 tensors do
    for n_in in (7, 8, 9, 23, 24):                            # the geometries the plan asks for: no such case
        for n_out in (n_in, n_in + 1):
            x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in)
            assert torch.equal(torch.nn.functional.interpolate(x, size=n_out, mode="nearest").double(),
                               torch.nn.functional.interpolate(x.double(), size=n_out, mode="nearest"))


def test_scalar_nn_src_is_the_vector_form():
    for n_in, n_out in ((5, 12), (7, 16), (48, 146), (13, 5)):
        scale = np.float32(n_in) / np.float32(n_out)
        want = np.concatenate([np.full(len(a), i) for i, a in enumerate(U.nearest_dests(n_in, n_out))])
        assert [U.nn_src(a, scale, n_in) for a in range(n_out)] == sorted(want.tolist())
