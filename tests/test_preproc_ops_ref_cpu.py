"""Host side of the input-pipeline operator tests (no GPU, no library): shows on the references alone that what
tests/test_gpu_preproc_ops.py asserts means something.  For every MRI case of tests/preproc_ops_ref.py (the list the GPU file
runs):

  * the float32 numpy oracle (oracle/preproc_ref.py, generalised here to any percentile pair) agrees with the float64 model to
    ORACLE_ATOL = 2.5e-7 — the kernel does that oracle's float32 operations, so the GPU tolerance of 1e-6 is about its
    summation order and nothing else;
  * the reference mutants (a floor rank moved by one, the interpolation weight flipped) move the model's output by at least
    MUTANT_MOVES = 1e-3, a thousand GPU tolerances, through the very comparison the GPU file makes;
  * the inputs have the properties they are there for (key bytes of the low pair, the sign straddle, signed zeros).
The models also reproduce the recorded outputs of the reference's own dataloader (tests/golden/preproc.npz).

Run with -s for the measured figures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_ops_ref as R  # noqa: E402

from oracle import preproc_ref  # noqa: E402

_CACHE = {}


def case_data(case):
    """(x, prepared, model output tuple) of a case, computed once."""
    if case.id not in _CACHE:
        x = R.build(case)
        prep = R.prepare(x)
        _CACHE[case.id] = (x, prep, R.mri(x, case.p_low, case.p_high, prepared=prep))
    return _CACHE[case.id]


def oracle_mri(image, p_low, p_high):
    """oracle/preproc_ref.preprocess_mri (utils/dataloader.py:128-144 in float32 numpy) for any percentile pair."""
    mean = np.mean(image)
    std = np.std(image)
    image = (image - mean) / (std + np.float32(1e-8))
    low, high = np.percentile(image, [float(np.float32(p_low)), float(np.float32(p_high))]).astype(np.float32)
    image = np.clip(image, low, high)
    out = (image - low) / (high - low + np.float32(1e-8))
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("case", R.MRI_CASES, ids=lambda c: c.id)
def test_float32_oracle_agrees_with_the_model(case):
    x, prep, (want, low, high, ks, gs) = case_data(case)
    delta, same_low, same_high = R.compare(oracle_mri(x, case.p_low, case.p_high), want)
    print(f"{case.id}: oracle - model {delta:.2e}  low {low:.6f} high {high:.6f} ranks {ks} g {gs[0]:.3f} {gs[1]:.3f}")
    assert delta <= R.ORACLE_ATOL
    assert same_low and same_high
    assert want.min() == 0.0 and abs(want.max() - 1.0) < 1e-7
    if (case.p_low, case.p_high) == (1.0, 99.0):
        assert R.compare(preproc_ref.preprocess_mri(x), want)[0] <= R.ORACLE_ATOL


@pytest.mark.parametrize("case", [c for c in R.MRI_CASES if c.mutants != "none"], ids=lambda c: c.id)
def test_mutants_of_the_model_are_caught(case):
    x, prep, (want, low, high, ks, gs) = case_data(case)
    shifts = R.rank_mutants(case.n, case.p_low, case.p_high)
    assert shifts, "every rank mutant is clamped away: the case pins nothing"
    moved = []
    for shift in shifts:
        delta = R.compare(R.mri(x, case.p_low, case.p_high, rank_shift=shift, prepared=prep)[0], want)[0]
        moved.append((f"rank{shift}", delta))
    if case.mutants == "all" and any(R.weight_mutant_counts(g) for g in gs):
        delta = R.compare(R.mri(x, case.p_low, case.p_high, flip_weight=True, prepared=prep)[0], want)[0]
        moved.append(("1-g", delta))
    print(f"{case.id}: " + "  ".join(f"{k} {v:.2e}" for k, v in moved))
    for name, delta in moved:
        assert delta >= R.MUTANT_MOVES, name


def test_case_list_holds_every_size_and_percentile_pair():
    ids = {c.id for c in R.MRI_CASES}
    assert len(ids) == len(R.MRI_CASES)
    for n in (2, 3, 101, 102, 201, 255, 256, 257, 1000, 4097):
        assert f"ladder-lin-{n}" in ids and f"ladder-geo-{n}" in ids
    for n in (4097, 65537, 262147, 524291, 1048583):
        for pair in ("1-99", "0.5-99.5", "25-75", "2.5-97.5"):
            assert f"pedestal-{n}-{pair}" in ids
        assert (f"pedestal-{n}-0-100" in ids) == (n <= 4097)
    assert {"background-4097", "background-262147", "straddle-202", "signed-zeros-1001"} <= ids
    assert max(c.n for c in R.MRI_CASES) <= 2_100_000
    # integral virtual indices, clamped ceil ranks
    assert R.ranks(101, 1.0) == (1, 0.0) and R.ranks(201, 99.0) == (198, 0.0)
    assert R.ranks(2, 99.0)[0] == 0 and R.ranks(3, 99.0)[0] == 1


def _low_pair(x, q=1.0):
    s = np.sort(R.zscore(x)[0])
    k = R.ranks(x.size, q)[0]
    return s[k], s[min(k + 1, x.size - 1)]


def test_low_pairs_part_in_every_radix_pass():
    """How many leading key bytes the floor / ceil pair of the low percentile shares decides in which of the four radix
    passes the two selections stop sharing a histogram.  z has unit variance whatever the input's scale, so neighbours
    at the 1st percentile (|z| in [1, 4)) have one sign and nearly one exponent unless the data are sparse there: a
    different TOP byte needs a sign change (n = 2, `straddle`) — geometric spacing alone does not give it, its low pair
    shares the top byte from n = 101 on like the equal-step ladder's.  Equal steps are 3.46 / n apart: under 2^16 float32
    spacings from n = 1000 on (two shared bytes) and under 2^8 only at the dense ladder's n (three shared bytes: the
    last pass alone tells them apart).  Ties share all four.  Between them the cases cover every depth."""
    shared = {}
    for n in R.LADDER_SIZES + (R.DENSE_LADDER,):
        for kind in ("lin", "geo") if n != R.DENSE_LADDER else ("lin",):
            a, b = _low_pair(R.ladder(n, kind))
            assert a < b
            shared[kind, n] = R.shared_key_bytes(a, b)
    print({f"{k}-{n}": v for (k, n), v in shared.items()})
    assert shared["lin", 2] == shared["geo", 2] == 0
    assert all(shared[kind, n] == 1 for kind in ("lin", "geo") for n in (101, 102, 201, 255, 256, 257))
    assert shared["lin", 1000] == shared["lin", 4097] == 2 and shared["lin", R.DENSE_LADDER] == 3
    assert shared["geo", 1000] <= 2 and shared["geo", 4097] <= 2
    assert R.shared_key_bytes(*_low_pair(R.straddle(202))) == 0
    a, b = _low_pair(R.background(4097))
    assert a == b and R.shared_key_bytes(a, b) == 4
    # the key is order preserving, zeros of either sign included
    z = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    assert np.all(np.diff(R.okey(z).astype(np.int64)) > 0)


def test_straddle_and_signed_zero_inputs():
    x = R.straddle(202)                                   # the builder asserts the sign condition itself; restated here
    s = np.sort(R.zscore(x)[0])
    k, g = R.ranks(202, 1.0)
    assert (k, round(g, 6)) == (2, 0.01) and s[2] < 0 < s[3]
    assert R.shared_key_bytes(s[2], s[3]) == 0
    z = R.zscore(R.signed_zeros())[0]
    assert R.zscore(R.signed_zeros())[1] == 0.0
    assert np.signbit(z[z == 0]).sum() == 200 and (z == 0).sum() == 401
    want, low, high, ks, gs = R.mri(R.signed_zeros(), 35.0, 85.0)
    assert low == 0.0 and high > 0.0
    # the low percentile of `background` lies inside the tie: a rank moved by one changes nothing, as in a real MRI
    x = R.background(4097)
    prep = R.prepare(x)
    base = R.mri(x, prepared=prep)[0]
    assert np.array_equal(base, R.mri(x, rank_shift=(1, 0), prepared=prep)[0])
    assert np.count_nonzero(x == 0.0) == (2 * 4097) // 5


def test_pedestal_layout():
    for n, (pl, ph) in ((4097, (1.0, 99.0)), (4097, (0.0, 100.0)), (65537, (25.0, 75.0))):
        s = np.sort(R.pedestal(n, pl, ph))
        for q in (pl, ph):
            k = R.ranks(n, q)[0]
            near = s[max(k - 2, 0):min(k + 4, n)]
            assert np.all(np.diff(near) >= 10.0), (n, q)
        assert np.unique(s).size == 64 + len({-900.0, 100.0, 5000.0} & set(s.tolist()))


def test_models_reproduce_the_recorded_dataloader_outputs(golden):
    g = golden("preproc")
    for name in (str(n) for n in g["names"]):
        x = g[f"{name}/image_in"]
        want = R.ct(x) if name.endswith("_ct") else R.mri(x)[0].reshape(x.shape)
        np.testing.assert_allclose(want, g[f"{name}/image_out"], rtol=0, atol=2e-6, err_msg=name)
        kind = 1 if name.startswith("amos") else 2 if name.startswith("chaos") else 0
        np.testing.assert_array_equal(R.remap(g[f"{name}/label_in"], kind), g[f"{name}/label_out"], err_msg=name)


def test_remap_model_and_its_boundary_mutants():
    v = R.remap_values()
    assert v.dtype == np.int64 and v.size == 309 + 8
    for kind in (0, 1, 2):
        np.testing.assert_array_equal(R.remap(v, kind), preproc_ref.remap_labels(v, ("ts", "amos", "chaos")[kind]))
    chaos = dict(zip(v.tolist(), R.remap(v, 2).tolist()))
    for (lo, hi), new in R.CHAOS_RANGES:
        assert chaos[lo] == chaos[hi] == new and chaos[lo - 1] == 0 and chaos[hi + 1] == 0
    amos = dict(zip(v.tolist(), R.remap(v, 1).tolist()))
    assert [amos[i] for i in range(-1, 8)] == [0, 0, 1, 3, 3, 0, 0, 2, 0]
    for big in (2 ** 32 + 1, 2 ** 32 + 6, 2 ** 32 + 60, -(2 ** 32) + 1, 2 ** 31, np.iinfo(np.int64).min):
        assert amos[big] == 0 and chaos[big] == 0
    # a CHAOS boundary moved by one, or labels truncated to 32 bits, differ from the model on this value set
    moved = np.where((v >= 55) & (v <= 71), 2, R.remap(v, 2))
    assert not np.array_equal(moved, R.remap(v, 2))
    trunc = (v & 0xFFFFFFFF).astype(np.int64)
    assert not np.array_equal(R.remap(trunc, 1), R.remap(v, 1)) and not np.array_equal(R.remap(trunc, 2), R.remap(v, 2))
    for n in R.REMAP_SIZES:
        x = R.remap_input(n, 1)
        assert x.size == n and (n < v.size or set(v.tolist()) <= set(x.tolist()))


def test_ct_model_and_inputs():
    for lo, hi in R.CT_WINDOWS:
        for n in R.CT_SIZES:
            x = R.ct_input(n, lo, hi)
            want = R.ct(x, lo, hi)
            assert x.size == n and np.isfinite(want).all() and want.min() >= 0.0 and want.max() <= 1.0
            assert np.all(want[x <= np.float32(lo)] == 0.0) and np.all(want[x >= np.float32(hi)] == 1.0)
            finite = np.isfinite(x)
            got = preproc_ref.preprocess_ct(x[finite], np.float32(lo), np.float32(hi))
            assert got.dtype == np.float32 and np.abs(got - want[finite]).max() <= 1e-7
        x = R.ct_input(255, lo, hi)
        inside = (x > np.float32(lo)) & (x < np.float32(hi))
        assert np.isinf(x).sum() >= 2 and inside.any() and 0.0 < R.ct(x, lo, hi)[inside].min() < 1e-6
