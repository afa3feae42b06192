"""CPU tests of the warp model tests/warp_ref.py (the checker of tests/test_gpu_warp.py) and of the host side of spatial.warp:
the noise against a plain-Python restatement of the hash, the smoothing against scipy.ndimage.correlate1d, coordinates / image / label
against scipy.ndimage.map_coordinates fed the model's own coordinates, exact cases, the mutants the GPU tests must be able to catch,
and the host helpers (affine_matrix, gaussian_taps, RandAffineElastic's draw order).  Bounds are derived in warp_ref's docstrings and
asserted as derived; measured ratios are printed (-s)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as R  # noqa: E402

from multimodal_segmentation_project_amd import spatial  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402

ndi = pytest.importorskip("scipy.ndimage")
CASE_IDS = [c.name for c in R.CASES]
SCIPY_MODE = {"border": "nearest", "zeros": "constant"}


# ---------------------------------------------------------------------------------------------- noise
def _mix_py(x):
    x = (x + 0x9E3779B97F4A7C15) & R.MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & R.MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & R.MASK
    return x ^ (x >> 31)


@pytest.mark.parametrize("seed", [0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1])
def test_noise_equals_the_plain_integer_restatement(seed):
    counters = list(range(200)) + [3 * 192 ** 3 - 1 - i for i in range(100)] + [2 ** 31 + 5, 2 ** 40 + 7]
    got = R.noise_at(seed, np.array(counters, dtype=np.uint64))
    want = [(((_mix_py(_mix_py(seed) ^ c) >> 40) - 2 ** 23) / 2.0 ** 23) for c in counters]
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), np.array(want))


def test_noise_values_are_dyadics_in_range_and_components_differ():
    u = R.noise((6, 7, 9), 5)
    k = u.astype(np.float64) * 2.0 ** 23
    assert np.array_equal(k, np.round(k)) and k.min() >= -2 ** 23 and k.max() < 2 ** 23
    assert abs(float(u.mean())) < 0.1 and 0.25 < float(u.var()) < 0.42          # uniform on [-1, 1): variance 1/3
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(u[a], u[b])
    assert not np.array_equal(u, R.noise((6, 7, 9), 6))


# ---------------------------------------------------------------------------------------------- smoothing
@pytest.mark.parametrize("shape,sigma,skew", [(s, g, False) for s, g in R.FIELD_CASES] + [(s, g, True) for s, g in R.SKEWED_FIELD_CASES])
def test_smoothing_against_correlate1d(shape, sigma, skew):
    g = R.skewed_taps(sigma) if skew else R.gaussian_taps(sigma)
    u = R.noise(shape, 7)
    want = u.astype(np.float64)
    for axis in (3, 2, 1):
        want = ndi.correlate1d(want, g, axis=axis, mode="constant", cval=0.0)
    got = R.smooth(u, g)
    assert got.dtype == np.float32
    err, bound = float(np.abs(got.astype(np.float64) - want).max()), R.smooth_bound(g)
    print(f"smooth {shape} sigma {sigma} skew {skew}: R = {g.size // 2}, max error / bound = {err / bound:.3f}")
    assert err <= bound
    assert float(np.abs(want).max()) > 100 * bound          # the comparison is not vacuous


def test_reversed_table_changes_every_skewed_field():
    for shape, sigma in R.SKEWED_FIELD_CASES:
        g = R.skewed_taps(sigma)
        assert not np.array_equal(g, g[::-1])
        assert not np.array_equal(R.field(shape, g, 3), R.field(shape, g, 3, reverse=True))
    for c in R.CASES:          # and with it the field every gather case reads
        g = R.skewed_taps(c.sigma)
        u, ur = R.model(c).field, R.field(c.out_shape, g, c.seed, reverse=True)
        assert not np.array_equal(u, ur)
        x, lab = R.inputs_of(c)
        s = R.coords(c.in_shape, c.out_shape, R.model(c).matrix, R.model(c).translate, ur, c.magnitude)
        for pad in R.PADDINGS:
            assert not np.array_equal(R.image_values(x, s, pad).astype(np.float32), R.model(c).image_out[pad]), (c.name, pad)
            assert not np.array_equal(R.label_values(lab, s, pad), R.model(c).label_out[pad]), (c.name, pad)


# ---------------------------------------------------------------------------------------------- coordinates, image, label
@pytest.mark.parametrize("name", CASE_IDS)
def test_cases_against_map_coordinates(name):
    c = R.case(name)
    m = R.model(c)
    # the coordinates, restated voxel by voxel in Python floats (IEEE double, one rounding per operation)
    rng = np.random.default_rng(1)
    for _ in range(40):
        o = tuple(int(rng.integers(0, n)) for n in c.out_shape)
        p = [(float(o[a]) - (c.out_shape[a] - 1) / 2.0) + c.magnitude * float(m.field[(a,) + o]) for a in range(3)]
        for a in range(3):
            want = ((m.matrix[a, 0] * p[0] + m.matrix[a, 1] * p[1]) + m.matrix[a, 2] * p[2]) + ((c.in_shape[a] - 1) / 2.0 + c.translate[a])
            assert m.coords[(a,) + o] == want
    flat = m.coords.reshape(3, -1)
    bound = R.image_bound(m.image)
    for pad in R.PADDINGS:
        for ch in range(c.channels):
            want_lab = ndi.map_coordinates(m.label[ch], flat, order=0, mode=SCIPY_MODE[pad], cval=0).reshape(c.out_shape)
            assert np.array_equal(m.label_out[pad][ch], want_lab), (name, pad, ch)
            want = ndi.map_coordinates(m.image[ch].astype(np.float64), flat, order=1, mode=SCIPY_MODE[pad], cval=0.0).reshape(c.out_shape)
            err = float(np.abs(m.values[pad][ch] - want).max())
            print(f"{name} {pad} channel {ch}: max error / (2^-53 max|x|) = {err / (R.U64 * float(np.abs(m.image).max())):.2f} (bound {R.K_IMAGE})")
            assert err <= bound, (name, pad, ch)


def test_far_case_samples_outside_for_over_a_third():
    m = R.model(R.case("far"))
    assert R.outside(m.coords, R.case("far").in_shape).mean() > 1 / 3
    assert not R.outside(m.coords, R.case("far").in_shape).all()
    for c in R.CASES:          # every case exercises the padding test on some voxels
        assert R.outside(R.model(c).coords, c.in_shape).any(), c.name


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_change_every_case(mutant):
    for c in R.CASES:
        good, bad = R.model(c), R.model(c, mutant)
        for pad in R.PADDINGS:
            assert not np.array_equal(good.image_out[pad], bad.image_out[pad]), (mutant, c.name, pad)
            assert not np.array_equal(good.label_out[pad], bad.label_out[pad]), (mutant, c.name, pad)


# ---------------------------------------------------------------------------------------------- exact cases
def _volume(shape, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.integers(0, 16, shape, dtype=np.int64)


def test_identity_returns_the_input_bitwise():
    x, lab = _volume((2, 5, 6, 7))
    for ip in R.PADDINGS:
        img, out = R.warp(x, lab, image_padding=ip, label_padding=ip)
        assert np.array_equal(img.view(np.uint32), x.view(np.uint32)) and np.array_equal(out, lab)


def test_flip_and_quarter_turn_matrices():
    x, lab = _volume((2, 6, 6, 6), 1)
    img, out = R.warp(x, lab, matrix=np.diag([-1.0, 1.0, 1.0]))
    assert np.array_equal(img, np.flip(x, 1)) and np.array_equal(out, np.flip(lab, 1))
    # s_h = -p_w, s_w = p_h: out[h, w] = in[n - 1 - w, h], which is np.rot90 from W towards H
    quarter = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    img, out = R.warp(x, lab, matrix=quarter, image_padding="zeros")
    assert np.array_equal(img, np.rot90(x, 1, axes=(3, 2))) and np.array_equal(out, np.rot90(lab, 1, axes=(3, 2)))
    # the product's affine_matrix at an exact quarter turn is that matrix up to cos(pi/2) = 6e-17
    assert np.abs(spatial.affine_matrix((math.pi / 2, 0, 0)) - quarter).max() < 1e-15


def test_smaller_grid_is_the_centred_crop_and_larger_grid_the_centred_zero_pad():
    x, lab = _volume((2, 8, 9, 10), 2)
    img, out = R.warp(x, lab, out_shape=(4, 5, 6), image_padding="zeros")
    assert np.array_equal(img, x[:, 2:6, 2:7, 2:8]) and np.array_equal(out, lab[:, 2:6, 2:7, 2:8])
    img, out = R.warp(x, lab, out_shape=(12, 11, 16), image_padding="zeros")
    want_x, want_lab = np.zeros((2, 12, 11, 16), np.float32), np.zeros((2, 12, 11, 16), np.int64)
    want_x[:, 2:10, 1:10, 3:13], want_lab[:, 2:10, 1:10, 3:13] = x, lab
    assert np.array_equal(img, want_x) and np.array_equal(out, want_lab)
    img, _ = R.warp(x, None, out_shape=(12, 11, 16), image_padding="border")          # border: the edge values repeat
    assert np.array_equal(img[:, :2, 1:10, 3:13], np.repeat(x[:, :1], 2, axis=1))


# ---------------------------------------------------------------------------------------------- host
def test_affine_matrix_literals():
    assert np.array_equal(spatial.affine_matrix(), np.eye(3))
    assert np.array_equal(spatial.affine_matrix(scale=(2.0, 0.5, 1.5)), np.diag([2.0, 0.5, 1.5]))
    c, s = math.cos(0.3), math.sin(0.3)
    assert np.array_equal(spatial.affine_matrix((0.3, 0, 0)), np.array([[1, 0, 0], [0, c, -s], [0, s, c]]))
    assert np.array_equal(spatial.affine_matrix((0, 0.3, 0)), np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]))
    assert np.array_equal(spatial.affine_matrix((0, 0, 0.3)), np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]))
    got = spatial.affine_matrix((0.1, 0.2, 0.3), (1.1, 0.9, 1.05))
    want = np.array([[1.0299227, -0.26066653, 0.2086028], [0.34429101, 0.85023224, -0.10273556], [-0.17527959, 0.1384128, 1.02392884]])
    assert got.dtype == np.float64 and np.abs(got - want).max() < 5e-9
    assert np.array_equal(got, R.affine_matrix((0.1, 0.2, 0.3), (1.1, 0.9, 1.05)))
    with pytest.raises(Mi3dError):
        spatial.affine_matrix((0.1, 0.2))


def test_gaussian_taps_literals():
    g = spatial.gaussian_taps(0.6)
    assert g.dtype == np.float64 and g.size == 5
    assert np.allclose(g, [0.00619421, 0.19611872, 0.59534324, 0.19611872, 0.00619421], rtol=0, atol=5e-9)
    for sigma, radius in ((0.6, 2), (2, 6), (8, 24), (3, 9), (1, 3), (10.5, 32)):
        g = spatial.gaussian_taps(sigma)
        assert g.size == 2 * radius + 1 and np.array_equal(g, g[::-1]) and np.array_equal(g, R.gaussian_taps(sigma))
        assert 0.99 < g.sum() < 1.0 and g.min() > 0.0 and g.argmax() == radius          # truncated at 3 sigma, not renormalised
    assert abs(spatial.gaussian_taps(2)[0] - 0.00240274) < 5e-9 and abs(spatial.gaussian_taps(8)[0] - 0.00055687) < 5e-9
    assert abs(spatial.gaussian_taps(2)[6] - 0.19741265) < 5e-9 and abs(spatial.gaussian_taps(8)[24] - 0.04983534) < 5e-9
    assert spatial.gaussian_taps(10.9).size // 2 == R.MAX_RADIUS + 1
    with pytest.raises(Mi3dError):
        spatial.gaussian_taps(0.0)


def test_rand_affine_elastic_draw_order_and_reproducibility():
    tf = spatial.RandAffineElastic(rotate_range=(0.1, 0.2, 0.3), scale_range=(0.1, 0.05, 0.2), sigma_range=(5, 8),
                                   magnitude_range=(100, 200), prob=0.9).set_random_state(42)
    p = tf.draw()
    rs = np.random.RandomState(42)
    assert rs.rand() < 0.9
    rotate = [rs.uniform(-r, r) for r in (0.1, 0.2, 0.3)]
    scale = [1.0 + rs.uniform(-r, r) for r in (0.1, 0.05, 0.2)]
    assert np.array_equal(p["matrix"], spatial.affine_matrix(rotate, scale))
    assert p["sigma"] == rs.uniform(5, 8) and p["magnitude"] == rs.uniform(100, 200)
    assert p["seed"] == int(rs.randint(0, 2 ** 63, dtype=np.int64)) and 0 <= p["seed"] < 2 ** 63
    q = tf.draw()
    assert q["sigma"] != p["sigma"] and q["seed"] != p["seed"]
    again = spatial.RandAffineElastic(rotate_range=(0.1, 0.2, 0.3), scale_range=(0.1, 0.05, 0.2), prob=0.9).set_random_state(42)
    for want in (p, q):
        got = again.draw()
        assert np.array_equal(got["matrix"], want["matrix"]) and {k: got[k] for k in ("sigma", "magnitude", "seed")} == \
            {k: want[k] for k in ("sigma", "magnitude", "seed")}
    # parts left out leave their draws out
    tf = spatial.RandAffineElastic(rotate_range=None, sigma_range=None).set_random_state(7)
    p, rs = tf.draw(), np.random.RandomState(7)
    rs.rand()
    assert np.array_equal(p["matrix"], np.diag([1.0 + rs.uniform(-0.1, 0.1) for _ in range(3)]))
    assert p["sigma"] is None and p["magnitude"] is None and p["seed"] is None
    assert tf.R.rand() == rs.rand()
    tf = spatial.RandAffineElastic(rotate_range=None, scale_range=None).set_random_state(7)
    p, rs = tf.draw(), np.random.RandomState(7)
    rs.rand()
    assert np.array_equal(p["matrix"], np.eye(3)) and p["sigma"] == rs.uniform(5, 8)


def test_prob_zero_passes_through_and_consumes_one_draw():
    tf = spatial.RandAffineElastic(prob=0.0).set_random_state(5)
    sample = {"image": np.zeros((1, 2, 3, 4), np.float32), "label": np.zeros((1, 2, 3, 4), np.int64), "name": "case"}
    out = tf(sample)
    assert out is not sample and out.keys() == sample.keys() and all(out[k] is sample[k] for k in sample)
    rs = np.random.RandomState(5)
    rs.rand()
    assert tf.R.rand() == rs.rand()
    assert spatial.RandAffineElastic(prob=0.0).set_random_state(5).draw() is None


def test_argument_errors_raise_before_any_launch():
    x, lab = np.zeros((1, 2, 3, 4), np.float32), np.zeros((1, 2, 3, 4), np.int64)
    for kw in ({"sigma": 2.0}, {"magnitude": 3.0}, {"seed": 1}, {"image_padding": "reflect"}, {"label_padding": "wrap"},
               {"matrix": np.eye(2)}, {"translate": (1, 2)}, {"out_shape": (2, 3)}, {"out_shape": (2, 0, 3)},
               {"sigma": 2.0, "magnitude": 1.0, "field": np.zeros((3, 2, 3, 4), np.float32)}):
        with pytest.raises(Mi3dError):
            spatial.warp(x, lab, **kw)
    with pytest.raises(Mi3dError):
        spatial.warp(x, np.zeros((1, 2, 3, 5), np.int64))
    with pytest.raises(Mi3dError):
        spatial.warp(None, None)
    with pytest.raises(Mi3dError):
        spatial.warp(np.zeros((2, 3, 4), np.float32), None)
    for kw in ({"rotate_range": (0.1, 0.1)}, {"sigma_range": (8, 5)}, {"sigma_range": (0, 5)}, {"image_padding": "reflect"},
               {"spatial_size": (96, 96)}, {"magnitude_range": None}):
        with pytest.raises(Mi3dError):
            spatial.RandAffineElastic(**kw)
    with pytest.raises(Mi3dError):
        spatial.displacement_field((4, 4, 4))
    with pytest.raises(Mi3dError):
        spatial.displacement_field((4, 4), sigma=1.0)
    with pytest.raises(Mi3dError):
        spatial.displacement_field((4, 4, 4), taps=np.ones(4))
