"""GPU tests of components.py (csrc/components.hip): connected components, the k largest per class and the cleaned map, against
tests/components_ref.py, which tests/test_components_cpu.py pins to scipy.ndimage.label.  Every comparison is exact (array_equal /
torch.equal): roots, sizes, counts and labels are integers and the labelling is canonical.  The status word is 0 everywhere.

Shapes and patterns are components_ref.CASES: W in {1, 63, 64, 65, 130}, D and H in {1, T - 1, T, T + 1, 2T + 3} with T the tile
side, a volume smaller than a tile in every axis, percolating noise, a serpentine, a comb, a checkerboard, cubes that touch along
an edge / at a corner across tile seams, interleaved classes, ranking ties, two samples, and the 96^3 organ-like map."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as R  # noqa: E402
import orient_ref as O  # noqa: E402

import multimodal_segmentation_project_amd as mi  # noqa: E402
from multimodal_segmentation_project_amd import _lib, components, resample, segment  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError, ptr  # noqa: E402

DEV = "cuda:0"
CONNECTIVITIES = (1, 2, 3)
PERMS = list(itertools.permutations(range(3)))          # (2, 1, 0) is Fortran order


@functools.lru_cache(maxsize=None)
def case(name):
    a = R.CASES[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference_roots(name, connectivity, classes=None):
    return R.roots(case(name), connectivity, classes)


@functools.lru_cache(maxsize=None)
def reference_keep(k, connectivity):
    name, keep, min_size, fill = R.KEEPS[k]
    return R.keep(case(name), keep, connectivity, min_size, fill)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached cases are read-only


def laid_out(t, perm):
    """The same logical (D, H, W) tensor stored with its axes in the order `perm`, slowest first."""
    inverse = [perm.index(i) for i in range(3)]
    return t.permute(*perm).contiguous().permute(*inverse)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check_cleaned(got, want, like):
    out, stats, classes = want
    assert int(got.status) == 0
    assert got.classes == classes
    assert got.labels.dtype == like.dtype and got.labels.shape == like.shape and got.labels.stride() == like.stride()
    assert got.stats.dtype == torch.int64 and np.array_equal(host(got.stats), stats)
    assert np.array_equal(host(got.labels), out)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_component_roots_equal_the_reference(name, connectivity):
    a = case(name)
    got = components.component_roots(dev(a), connectivity)
    assert got.dtype == torch.int32 and got.is_contiguous() and got.shape == a.shape
    assert np.array_equal(host(got), reference_roots(name, connectivity))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_component_roots_of_selected_classes_only(connectivity):
    for name, classes in (("iid4", (1, 3)), ("interleaved", (2,)), ("small", (3,))):
        got = components.component_roots(dev(case(name)), connectivity, classes)
        assert np.array_equal(host(got), reference_roots(name, connectivity, classes))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("k", range(len(R.KEEPS)), ids=lambda k: f"{R.KEEPS[k][0]}-{k}")
def test_keep_largest_equals_the_reference(k, connectivity):
    name, keep, min_size, fill = R.KEEPS[k]
    t = dev(case(name))
    got = components.keep_largest(t, keep=keep, connectivity=connectivity, min_size=min_size, fill=fill)
    check_cleaned(got, reference_keep(k, connectivity), t)


def test_keep_largest_defaults_are_the_organs_at_connectivity_1():
    k = [c[0] for c in R.KEEPS].index("organs96")
    got = components.keep_largest(dev(case("organs96")))
    check_cleaned(got, reference_keep(k, 1), dev(case("organs96")))
    stats = host(got.stats)
    assert (stats[:, 0] > np.array([1, 1, 2])).all()                        # the salt made islands
    assert (stats[:, 3 + R.MAX_KEEP] >= 0).all() and stats[2, 4] > 0         # a spleen, a liver, two kidneys kept


def test_all_foreground_is_one_component_with_root_0():
    a = case("all_foreground")
    for connectivity in CONNECTIVITIES:
        assert int(components.component_roots(dev(a), connectivity).abs().max()) == 0
        got = components.keep_largest(dev(a), keep={1: 3}, connectivity=connectivity)
        row = host(got.stats)[0]
        assert int(got.status) == 0 and list(row[:5]) == [1, a.size, a.size, a.size, 0] and list(row[11:13]) == [0, -1]
        assert np.array_equal(host(got.labels), a)


def test_checkerboard_ranking_is_decided_by_the_root_alone():
    a = case("checkerboard")
    got = components.keep_largest(dev(a), keep={1: 8}, connectivity=1)
    row = host(got.stats)[0]
    first = np.flatnonzero(a.ravel())[:8]
    assert int(got.status) == 0 and row[0] == a.sum() and list(row[3:11]) == [1] * 8 and list(row[11:19]) == list(first)
    for connectivity in (2, 3):
        row = host(components.keep_largest(dev(a), keep={1: 8}, connectivity=connectivity).stats)[0]
        assert list(row[:5]) == [1, a.sum(), a.sum(), a.sum(), 0] and row[11] == first[0]


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64), ids=("uint8", "int64"))
@pytest.mark.parametrize("connectivity", (1, 3))
def test_every_layout_gives_the_same_roots_and_keeps_its_strides(connectivity, dtype):
    a = R._iid4((R.T + 1, 2 * R.T + 3, 65), 31)
    want_roots = R.roots(a, connectivity)
    want = R.keep(a.astype(np.int64 if dtype == torch.int64 else np.uint8), {1: 2, 2: 1, 3: 8}, connectivity, 2, 0)
    seen = set()
    for perm in PERMS:
        t = laid_out(dev(a).to(dtype), perm)
        seen.add(t.stride())
        roots = components.component_roots(t, connectivity)
        assert roots.is_contiguous() and np.array_equal(host(roots), want_roots)
        check_cleaned(components.keep_largest(t, keep={1: 2, 2: 1, 3: 8}, connectivity=connectivity, min_size=2), want, t)
    d, h, w = a.shape
    assert len(seen) == 6 and (1, d, d * h) in seen          # Fortran order among them


def test_int64_values_outside_a_byte_pass_through():
    a = case("interleaved").copy()
    a[0, 0, 0:3] = (-1, 256, 257)                             # 256 and 257 are not classes 0 and 1
    t = dev(a)
    for connectivity in CONNECTIVITIES:
        check_cleaned(components.keep_largest(t, keep={1: 1, 2: 8}, connectivity=connectivity), R.keep(a, {1: 1, 2: 8}, connectivity), t)
        assert np.array_equal(host(components.component_roots(t, connectivity)), R.roots(a, connectivity))
    assert (host(components.component_roots(t))[a > 255] == -1).all()


def test_samples_never_merge_and_may_lie_apart():
    a = case("two_samples")
    k = [c[0] for c in R.KEEPS].index("two_samples")
    for connectivity in CONNECTIVITIES:
        got = components.keep_largest(dev(a), connectivity=connectivity)
        check_cleaned(got, reference_keep(k, connectivity), dev(a))
        stats = host(got.stats)
        assert np.array_equal(stats[0], stats[1]) and stats[0, 0, 0] == 2
    # the samples as every other volume of a (2, 2, D, H, W) tensor, each Fortran-ordered
    wide = torch.zeros((2, 2) + a.shape[1:], dtype=torch.uint8, device=DEV).permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)
    wide[:, 1] = 9
    wide[:, 0] = dev(a)
    t = wide[:, 0]
    assert not t.is_contiguous()
    got = components.keep_largest(t, keep={1: 1, 2: 1}, connectivity=1)
    check_cleaned(got, R.keep(a, {1: 1, 2: 1}, 1), t)
    assert np.array_equal(host(components.component_roots(t)), reference_roots("two_samples", 1))
    assert int(wide[:, 1].min()) == 9 and int(wide[:, 1].max()) == 9


def test_two_calls_give_identical_bits():
    for name, connectivity in (("organs96", 3), ("perc31", 1), ("serpentine", 2)):
        t = dev(case(name))
        a, b = components.keep_largest(t, connectivity=connectivity), components.keep_largest(t, connectivity=connectivity)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.stats, b.stats) and int(a.status) == 0 and int(b.status) == 0
        assert torch.equal(components.component_roots(t, connectivity), components.component_roots(t, connectivity))


def test_argument_errors_launch_nothing():
    good = dev(case("small"))
    before = _lib.launches
    for kw, match in ((dict(labels=good.float()), "uint8 or torch.int64"), (dict(labels=good[:, :, ::2]), "not dense"),
                      (dict(labels=good[0]), "label volume expected"), (dict(connectivity=4), "connectivity"), (dict(keep={0: 1}), "1..255"),
                      (dict(keep={1: 9}), "1..8 expected"), (dict(keep={c: 1 for c in range(1, 10)}), "at most 8"),
                      (dict(fill=256), "fill"), (dict(min_size=0), "min_size"), (dict(labels=good.cpu()), "no CPU fallback")):
        kw = dict(kw)
        with pytest.raises(Mi3dError, match=match):
            components.keep_largest(kw.pop("labels", good), **kw)
    with pytest.raises(Mi3dError, match="cannot be selected"):
        components.component_roots(good, classes=(0,))
    assert _lib.launches == before
    # the library's own checks: a negative code, a message, and the outputs as they were
    lib = _lib.lib()
    n, (d, h, w) = 1, good.shape
    nbytes = lib.mi3d_components_workspace_bytes(n, d, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full_like(good, 77)
    stats = torch.full((1, 2, components.STATS_COLUMNS), -7, dtype=torch.int64, device=DEV)
    status = torch.full((), -3, dtype=torch.int32, device=DEV)
    ints = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def keep(conn=1, nc=2, values=(1, 2), ks=(1, 1), min_size=1, fill=0, ws_bytes=nbytes, strides=(d * h * w, h * w, w, 1), dtype=_lib.SRC_U8):
        return lib.mi3d_keep_components(ptr(good), dtype, n, d, h, w, *strides, conn, nc, ints(*values), ints(*ks), min_size, fill, ptr(out),
                                        ptr(stats), ptr(status), ptr(ws), ws_bytes, None)

    for bad in (dict(conn=0), dict(conn=4), dict(nc=0), dict(nc=9, values=(1,) * 9, ks=(1,) * 9), dict(values=(0, 2)), dict(values=(1, 256)),
                dict(values=(2, 2)), dict(ks=(0, 1)), dict(ks=(1, 9)), dict(min_size=0), dict(fill=-1), dict(fill=256),
                dict(ws_bytes=nbytes - 1), dict(strides=(d * h * w, h * w, w, 0)), dict(dtype=_lib.SRC_F32)):
        assert keep(**bad) < 0 and lib.mi3d_last_error()
    select = (C.c_uint8 * 256)()
    select[0] = 1
    roots = torch.full(good.shape, -9, dtype=torch.int32, device=DEV)
    assert lib.mi3d_component_roots(ptr(good), _lib.SRC_U8, n, d, h, w, d * h * w, h * w, w, 1, 1, select, ptr(roots), ptr(status), ptr(ws),
                                    nbytes, None) < 0
    assert int(out.min()) == 77 and int(out.max()) == 77 and int(stats.max()) == -7 and int(status) == -3 and int(roots.max()) == -9
    assert keep() == 0 and int(status) == 0 and int(stats[0, 0, 1]) == int((good == 1).sum())


def test_segment_scan_cleans_the_grid_map_before_it_is_restored():
    torch.manual_seed(3)
    model = mi.UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).to(DEV).eval()
    model.compute_dtype = torch.bfloat16
    with torch.no_grad():          # keeps an untrained network's logits apart, so the map is not one class
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.fill_(0.1)
    rng = np.random.default_rng(21)
    perm, signs = (2, 0, 1), (-1, 1, -1)
    scan = O.store_as(rng.integers(-1024, 3000, (7, 10, 13)).astype(np.int16), perm, signs)
    d, h, w = scan.shape
    image = torch.empty_strided(scan.shape, (1, d, d * h), dtype=torch.int16, device=DEV)
    image.copy_(torch.from_numpy(np.ascontiguousarray(scan)))
    aff = O.affine_for(perm, signs)
    target = (16, 16, 16)
    plain = segment.segment_scan(model, image, aff, "amos_ct", target_shape=target)
    assert len(plain) == 3 and torch.equal(plain[0], segment.segment_scan(model, image, aff, "amos_ct", target_shape=target, keep_largest=None)[0])
    for connectivity in (1, 3):
        stored, on_grid, grid_aff, cleaned = segment.segment_scan(model, image, aff, "amos_ct", target_shape=target,
                                                                  keep_largest=components.ORGANS, connectivity=connectivity)
        x, _, want_aff = resample.resample_scan(image, aff, target_shape=target, ct_window=segment.CT_WINDOW)
        raw = segment.predict_labels(model, x[None, None])[0]
        assert torch.equal(raw, plain[1])
        want = components.keep_largest(raw, keep=components.ORGANS, connectivity=connectivity)
        check_cleaned(want, R.keep(host(raw), R.ORGANS, connectivity), raw)
        assert isinstance(cleaned, components.Cleaned) and int(cleaned.status) == 0 and on_grid is cleaned.labels
        assert torch.equal(on_grid, want.labels) and torch.equal(cleaned.stats, want.stats) and np.array_equal(grid_aff, want_aff)
        assert stored.dtype == torch.uint8 and stored.stride() == image.stride()
        assert torch.equal(stored, resample.restore_labels(want.labels, aff, image))
        volumes = components.organ_volumes_ml(cleaned, grid_aff)
        assert sorted(volumes) == [1, 2, 3] and all(kept <= before for before, kept in volumes.values())
