"""CPU tests of the host orientation algebra (orientation.py) and of the flip-remapped resampling tables (resample.py).

There is no nibabel here and none is recorded: the oracle is geometry.  For the 48 signed axis permutations, plain and under
three oblique rotations, every voxel of the reoriented array must keep its world coordinate, the new affine must have its
largest entry per column on the diagonal and positive, and its spacing must be the stored spacing permuted.  The rotations stay
at 31 degrees or less: at 45 the closest axis is a tie decided by rounding, and a test there would pin noise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_ref as O  # noqa: E402

from multimodal_segmentation_project_amd import orientation, resample  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402

CASES = [(p, s, r) for p, s in O.signed_permutations() for r in O.ROTATIONS]


def test_case_count():
    assert len(O.signed_permutations()) == 48 and len(CASES) == 192


@pytest.mark.parametrize("rot", O.ROTATIONS, ids=["plain", "x20", "y-17", "z31"])
def test_orientation_geometry(rot):
    index = np.arange(np.prod(O.SHAPE)).reshape(O.SHAPE)
    stored_ijk = np.stack(np.unravel_index(index.ravel(), O.SHAPE), axis=0)          # (3, n) by flat stored index
    for perm, signs in O.signed_permutations():
        aff = O.affine_for(perm, signs, rot=rot)
        ornt = orientation.io_orientation(aff)
        assert np.array_equal(ornt, O.ornt_of(perm, signs)), (perm, signs)
        assert np.array_equal(orientation.ras_transform(aff), ornt)
        new_aff = orientation.reoriented_affine(aff, O.SHAPE)
        assert np.array_equal(new_aff, aff @ orientation.inv_ornt_aff(ornt, O.SHAPE))
        ras = O.reorient(index, ornt)
        assert ras.shape == orientation.ras_shape(ornt, O.SHAPE)
        # every voxel keeps its world coordinate
        r_ijk = np.stack(np.unravel_index(np.arange(ras.size), ras.shape), axis=0)
        world_new = new_aff[:3, :3] @ r_ijk + new_aff[:3, 3:]
        world_old = aff[:3, :3] @ stored_ijk[:, ras.ravel()] + aff[:3, 3:]
        assert np.allclose(world_new, world_old, rtol=0, atol=1e-9), (perm, signs)
        # closest to RAS: the largest entry of each column is on the diagonal, and positive
        m = new_aff[:3, :3]
        assert np.array_equal(np.argmax(np.abs(m), axis=0), np.arange(3)) and np.all(np.diag(m) > 0)
        want_spacing = np.asarray(O.SPACING)[np.argsort(perm)]
        assert np.allclose(orientation.spacing_of(new_aff), want_spacing, rtol=1e-14, atol=0)
        assert np.allclose(orientation.spacing_of(aff), O.SPACING, rtol=1e-14, atol=0)


@pytest.mark.parametrize("order", ["C", "F"])
def test_axis_map_gather_equals_reorientation(order):
    index = np.arange(np.prod(O.SHAPE), dtype=np.int64).reshape(O.SHAPE)
    stored = np.ascontiguousarray(index) if order == "C" else np.asfortranarray(index)
    strides = tuple(s // stored.itemsize for s in stored.strides)
    memory = stored.ravel(order="K")                                                 # the buffer as it lies in memory
    assert memory.flags.c_contiguous and (order == "C") == (strides[2] == 1)
    for perm, signs in O.signed_permutations():
        for rot in O.ROTATIONS[:2]:
            aff = O.affine_for(perm, signs, rot=rot)
            amap = orientation.axis_map(aff, stored.shape, strides)
            offs = []
            for n, s, flipped in amap:
                i = np.arange(n)
                offs.append((n - 1 - i if flipped else i) * s)
            got = memory[offs[0][:, None, None] + offs[1][None, :, None] + offs[2][None, None, :]]
            assert np.array_equal(got, O.reorient(stored, orientation.io_orientation(aff))), (perm, signs)


@pytest.mark.parametrize("n_in,n_mid,n_out", [(14, 23, 11), (9, 5, 12), (5, 5, 5), (7, 1, 3)])
def test_flipped_tables_are_the_ras_tables_remapped(n_in, n_mid, n_out):
    t0 = resample.axis_table(n_in, n_mid, 0)
    assert np.array_equal(resample.axis_table(n_in, n_mid, 0, flip=True), n_in - 1 - t0)
    idx, w = resample.axis_table(n_in, n_mid, 3)
    fidx, fw = resample.axis_table(n_in, n_mid, 3, flip=True)
    assert np.array_equal(fidx, n_in - 1 - idx) and np.array_equal(fw, w) and fidx.dtype == np.int32
    rows, frows = resample.cubic_rows(n_in, n_mid), resample.cubic_rows(n_in, n_mid, flip=True)
    assert np.array_equal(frows["idx"], n_in - 1 - rows["idx"]) and np.array_equal(frows["w"], rows["w"])
    comp = resample.composed_index_table(n_in, n_mid, n_out)
    assert np.array_equal(comp, t0[resample.axis_table(n_mid, n_out, 0)])
    fcomp = resample.composed_index_table(n_in, n_mid, n_out, flip=True)
    assert np.array_equal(fcomp, n_in - 1 - comp) and fcomp.dtype == np.int32
    for t in (fidx, fcomp, resample.axis_table(n_in, n_mid, 0, flip=True)):
        assert t.min() >= 0 and t.max() <= n_in - 1


def test_a_table_built_in_stored_order_would_differ():
    t = resample.axis_table(14, 23, 0)
    assert not np.array_equal(14 - 1 - t, t[::-1])      # round-half-up is not mirror symmetric: the remap must come last


def test_unusable_inputs_raise():
    good = O.affine_for((0, 1, 2), (1, 1, 1))
    zero_col = good.copy()
    zero_col[:3, 1] = 0
    for bad in (lambda: orientation.io_orientation(zero_col),
                lambda: orientation.reoriented_affine(zero_col, O.SHAPE),
                lambda: orientation.io_orientation(np.eye(3)),
                lambda: orientation.io_orientation(np.zeros((4, 4))),
                lambda: orientation.spacing_of(np.ones((3, 4))),
                lambda: orientation.axis_map(good, (5, 9), (9, 1)),
                lambda: orientation.inv_ornt_aff([[0, 1], [0, 1], [2, 1]], O.SHAPE),
                lambda: orientation.check_dense((5, 9, 14), (126, 14, 0)),             # stride 0
                lambda: orientation.check_dense((5, 9, 14), (144, 16, 1)),             # padded rows
                lambda: orientation.check_dense((5, 9, 14), (9, 1, 1)),                # overlapping
                lambda: orientation.check_dense((5, 9, 14), (252, 28, 2)),             # every second element
                lambda: resample.merge_masks_to_grid([(None, 1)] * 9, good)):                # 9 masks
        with pytest.raises(Mi3dError):
            bad()
    for shape, strides in (((5, 9, 14), (126, 14, 1)), ((5, 9, 14), (1, 5, 45)), ((5, 9, 14), (14, 70, 1)), ((1, 9, 1), (7, 1, 3))):
        orientation.check_dense(shape, strides)


@pytest.mark.parametrize("shape", [O.SHAPE, (1, 9, 14), (5, 1, 1), (4, 4, 4)])
def test_contiguous_ras_memory_comes_back_with_the_ras_axes(shape, monkeypatch):
    """Memory that already is contiguous RAS (an F-ordered array stored with reversed axes, say) needs no copy, but the tensor
    handed on must have the RAS axes, not the stored ones.  The view is plain stride arithmetic, so a host tensor shows it."""
    import torch
    from multimodal_segmentation_project_amd import _lib
    monkeypatch.setattr(_lib, "require_cuda", lambda *a, **k: None)
    x = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    stored = {"C": torch.from_numpy(x), "F": torch.from_numpy(np.ascontiguousarray(x.transpose(2, 1, 0))).permute(2, 1, 0)}
    seen = 0
    for order, xd in stored.items():
        for perm, signs in O.signed_permutations():
            src = resample._Stored(xd, O.affine_for(perm, signs), "test")
            if not src.identity:
                continue
            seen += 1
            view = src.ras_view(xd)
            want = np.ascontiguousarray(O.reorient(x, O.ornt_of(perm, signs)))
            assert view.is_contiguous() and view.data_ptr() == xd.data_ptr() and tuple(view.shape) == want.shape
            assert np.array_equal(view.numpy(), want), (order, perm, signs)
    assert seen >= 2        # at least the plain C-ordered array and the reversed F-ordered one


def test_nine_masks_raise_through_resample_scan(monkeypatch):
    """The image is a good (host) tensor, so what raises is the count of the masks; eight of them pass that check and fail
    only at the first entry, which is no tensor."""
    import torch
    from multimodal_segmentation_project_amd import _lib
    monkeypatch.setattr(_lib, "require_cuda", lambda *a, **k: None)
    image = torch.zeros(O.SHAPE, dtype=torch.int16)
    good = O.affine_for((0, 1, 2), (1, 1, 1))
    with pytest.raises(Mi3dError, match="9 masks"):
        resample.resample_scan(image, good, masks=[(None, 1)] * 9)
    with pytest.raises(Mi3dError, match="3-D volume"):
        resample.resample_scan(image, good, masks=[(None, 1)] * 8)
