"""Pins tests/fill_holes_ref.py, the reference of the GPU tests of components.fill_holes, to the host route it replaces: for every
case of its table and every connectivity the filled map, the stats and the summary are rebuilt from scipy.ndimage.label(labels == 0,
generate_binary_structure(3, connectivity)), per component binary_dilation(comp, structure) & ~comp on a copy padded by one voxel and
np.unique on that ring, and compared with array_equal; one-class maps also against scipy.ndimage.binary_fill_holes.  Then the
counts the case table promises, the four broken variants of the model (each must be seen by a case), and the argument checks of
components.fill_holes that need no device."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_holes_ref as R  # noqa: E402

from multimodal_segmentation_project_amd import _lib, components  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402

ndimage = pytest.importorskip("scipy.ndimage")
CONNECTIVITIES = (1, 2, 3)
PAD = -(2 ** 40)          # what the padded copy carries outside the volume: no label of any case


@functools.lru_cache(maxsize=None)
def case(name):
    a = R.CASES[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def model(k, connectivity):
    name, classes, max_size = R.FILLS[k]
    return R.fill(case(name), classes, connectivity, max_size)


def scipy_fill3(sample, classes, connectivity, max_size):
    structure = ndimage.generate_binary_structure(3, connectivity)
    padded = np.pad(sample.astype(np.int64), 1, constant_values=PAD)
    ids, n = ndimage.label(padded == 0, structure)
    out, stats, summary = padded.copy(), np.zeros((len(classes), 2), dtype=np.int64), np.zeros(4, dtype=np.int64)
    for j, box in enumerate(ndimage.find_objects(ids), start=1):
        box = tuple(slice(s.start - 1, s.stop + 1) for s in box)          # the component and its ring: the padding keeps this inside
        comp = ids[box] == j
        ring = ndimage.binary_dilation(comp, structure) & ~comp
        values = np.unique(padded[box][ring])
        if PAD in values:
            continue          # open
        summary[0] += 1
        # every int64 value outside 0..255 is one ring value
        values = np.unique(np.where((values >= 0) & (values <= 255), values, R.OTHER))
        if len(values) > 1:
            summary[2] += 1
        elif values[0] in classes and (max_size is None or comp.sum() <= max_size):
            summary[1] += 1
            stats[classes.index(values[0])] += (1, comp.sum())
            out[box][comp] = values[0]
        else:
            summary[3] += 1
    return out[1:-1, 1:-1, 1:-1].astype(sample.dtype), stats, summary


def scipy_fill(labels, classes, connectivity, max_size):
    classes = tuple(sorted(classes))
    if labels.ndim == 3:
        return scipy_fill3(labels, classes, connectivity, max_size)
    parts = [scipy_fill3(s, classes, connectivity, max_size) for s in labels]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("k", range(len(R.FILLS)), ids=lambda k: f"{R.FILLS[k][0]}-{k}")
def test_the_model_equals_the_scipy_route(k, connectivity):
    name, classes, max_size = R.FILLS[k]
    out, stats, summary, listed = model(k, connectivity)
    want = scipy_fill(case(name), classes, connectivity, max_size)
    assert listed == tuple(sorted(classes)) and out.dtype == case(name).dtype
    assert np.array_equal(out, want[0]) and np.array_equal(stats, want[1]) and np.array_equal(summary, want[2])
    assert (summary[..., 0] == summary[..., 1:].sum(axis=-1)).all() and (stats[..., 0].sum(axis=-1) == summary[..., 1]).all()
    changed = out != case(name)
    assert (case(name)[changed] == 0).all() and changed.sum() == stats[..., 1].sum()


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(R.SINGLE_CLASS))
def test_one_class_maps_equal_binary_fill_holes(name, connectivity):
    c, a = R.SINGLE_CLASS[name], case(name)
    assert set(np.unique(a)) <= {0, c}
    out = model([f[0] for f in R.FILLS].index(name), connectivity)[0]
    structure = ndimage.generate_binary_structure(3, connectivity)
    for got, sample in zip(out.reshape(-1, *a.shape[-3:]), a.reshape(-1, *a.shape[-3:])):
        assert np.array_equal(got, ndimage.binary_fill_holes(sample == c, structure) * c)


def default(name, connectivity):
    return model([f[0] for f in R.FILLS].index(name), connectivity)


def test_the_cases_hold_what_their_names_promise():
    for name, connectivity in R.PUNCHED.items():
        summary = default(name, connectivity)[2]
        assert summary[1] >= 100 and summary[2] >= 100, (name, summary)
    cavity = 11 * 4 * 61
    assert cavity > 2000
    for connectivity in CONNECTIVITIES:
        out, stats, summary, _ = default("box", connectivity)
        assert list(summary) == [1, 1, 0, 0] and list(stats[1]) == [1, cavity] and (out[2:17, 2:10, 3:68] == 2).all()
        open_at = {"box_corner_channel": 3, "box_edge_channel": 2}
        for name, first_open in open_at.items():
            out, stats, summary, _ = default(name, connectivity)
            closed = connectivity < first_open
            assert (stats[1, 1] >= cavity) == closed and (out[4:15, 4:8, 5:66] == (2 if closed else 0)).all(), (name, connectivity)
        out, stats, summary, _ = default("box_with_block", connectivity)
        assert list(summary) == [1, 0, 1, 0] and np.array_equal(out, case("box_with_block"))
        out, stats, summary, _ = default("int64_walls", connectivity)
        assert list(summary) == [4, 1, 2, 1] and list(stats[:, 0]) == [1, 0, 0] and out.dtype == np.int64
        assert (out[2:5, 2:5, 2:7] == 0).all() and (out[4:7, 2:5, 31:39] == 1).all()
        for name in ("all_background", "all_foreground", "flat_d1", "flat_h1", "thin_w1"):
            out, stats, summary, _ = default(name, connectivity)
            assert np.array_equal(out, case(name)) and not summary.any() and not stats.any(), name
        out, stats, summary, _ = default("one_voxel", connectivity)
        assert list(summary) == [1, 1, 0, 0] and list(stats[2]) == [1, 1] and (out == 3).all()
        out, stats, summary, _ = default("diagonal_neighbours", connectivity)
        assert list(summary) == [3, 4 - connectivity, connectivity - 1, 0] and list(stats[2]) == [4 - connectivity] * 2
        out, stats, summary, _ = default("two_samples", connectivity)
        assert summary.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0]] and stats[:, 0].tolist() == [[1, 2 * 3 * 20], [0, 0]]
        assert np.array_equal(out[1], case("two_samples")[1]) and (out[0, -1, -1] == 0).all()
        out, stats, summary, _ = default("organs48", connectivity)
        assert (stats[:, 0] >= 1).all() and summary[2] >= 1 and (out[24:27, 31:34, 20:24] == 0).all(), (connectivity, stats, summary)
    for name in ("flat_d1", "flat_h1", "thin_w1"):
        assert (case(name) == 0).any() and (case(name) != 0).any()


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_every_broken_model_is_seen_by_a_case(mutant):
    seen = []
    for k, (name, classes, max_size) in enumerate(R.FILLS):
        for connectivity in CONNECTIVITIES:
            got = R.fill(case(name), classes, connectivity, max_size, **R.MUTANTS[mutant])
            if not all(np.array_equal(g, w) for g, w in zip(got[:3], model(k, connectivity)[:3])):
                seen.append((name, k, connectivity))
    assert seen, mutant
    if mutant == "no_face_rule":
        assert {"two_samples", "flat_d1", "all_background"} & {s[0] for s in seen}
    if mutant == "mixed_takes_min":
        assert "box_with_block" in {s[0] for s in seen}
    if mutant == "ring_connectivity_1":
        assert {s[2] for s in seen} == {2, 3} and "diagonal_neighbours" in {s[0] for s in seen}


def test_max_size_and_the_class_list_each_change_a_case():
    fills = [f[0] for f in R.FILLS]
    for k, (name, classes, max_size) in enumerate(R.FILLS):
        if classes == (1, 2, 3) and max_size is None:
            continue
        # at a connectivity above the one a density is chosen for, the background of a punched map percolates and few holes are left
        same = [np.array_equal(model(fills.index(name), connectivity)[0], model(k, connectivity)[0]) for connectivity in CONNECTIVITIES]
        if (name, max_size) == ("box", 2684) or name == "int64_walls":          # the limit that just fits; a list that fills the same hole
            assert all(same)
        else:
            assert not all(same), (name, classes, max_size)
    big, small = model(R.FILLS.index(("box", (2,), 2684)), 1), model(R.FILLS.index(("box", (2,), 2683)), 1)
    assert list(big[2]) == [1, 1, 0, 0] and list(small[2]) == [1, 0, 0, 1]
    assert list(model(R.FILLS.index(("box", (1, 3), None)), 1)[2]) == [1, 0, 0, 1]


def test_argument_errors_need_no_device():
    good = torch.zeros((3, 5, 17), dtype=torch.uint8)
    before = _lib.launches
    for kw, match in ((dict(labels=good.float()), "uint8 or torch.int64"), (dict(labels=good[:, :, ::2]), "not dense"),
                      (dict(labels=good[0]), "label volume expected"), (dict(connectivity=4), "connectivity"), (dict(classes=(0,)), "1..255"),
                      (dict(classes=(256,)), "1..255"), (dict(classes=()), "1 to 8 classes"), (dict(classes=range(1, 10)), "1 to 8 classes"),
                      (dict(classes=(2, 2)), "listed twice"), (dict(classes=(1.5,)), "not an integer"), (dict(classes=3), "iterable"),
                      (dict(max_size=0), "max_size"), (dict(max_size=-1), "max_size"), (dict(max_size=2.5), "not an integer"),
                      (dict(), "no CPU fallback")):
        kw = dict(kw)
        with pytest.raises(Mi3dError, match=match):
            components.fill_holes(kw.pop("labels", good), **kw)
    assert _lib.launches == before
