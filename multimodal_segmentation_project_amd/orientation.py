"""Host orientation algebra of the resampling scripts' reorient_to_ras (scripts/resampling/amos_ct_resample.py:29-36, the
same body in chaos_resample.py and resample_totalseg_ras_mri.py): which stored axis is closest to which world axis, the
matrix that undoes the reordering, the reoriented affine and its voxel spacing.  numpy float64 only: no GPU, no nibabel.

  io_orientation(affine)             (3, 2): per stored axis the RAS axis it becomes and its direction (+1 / -1)
  ras_transform(affine)              the transform from that orientation to ('R', 'A', 'S'): the orientation itself
  inv_ornt_aff(ornt, shape)          4x4 matrix taking reoriented voxel indices back to stored voxel indices
  reoriented_affine(affine, shape)   affine @ inv_ornt_aff: the affine of the reoriented array
  spacing_of(affine)                 column norms of the 3x3 part (amos_ct_resample.py:51)
  axis_map(affine, shape, strides)   per RAS axis (D, H, W): (side, element stride of the stored tensor, flipped)

The functions are written from the definitions of these operations, not from nibabel's source, and no nibabel run is
recorded anywhere: parity with nibabel is by construction and by geometry (tests/test_orientation_cpu.py: every reoriented
voxel keeps its world coordinate, the new affine is diagonal-dominant and positive, the spacing is the stored one permuted).
"""
import numpy as np

from ._lib import Mi3dError


def _affine(affine):
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise Mi3dError(f"orientation: a 4x4 affine is expected, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise Mi3dError("orientation: the affine has non-finite entries")
    return a


def io_orientation(affine):
    """(3, 2) float64: row i = (RAS axis that stored axis i is closest to, +1 or -1 for its direction)."""
    a = _affine(affine)
    rzs = a[:3, :3]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1.0
    rs = rzs / zooms
    # the closest rotation: polar factor P Qs of the SVD, without the directions the matrix does not span
    p, s, qs = np.linalg.svd(rs)
    keep = s > s.max() * 3 * np.finfo(s.dtype).eps
    r = p[:, keep] @ qs[keep]
    ornt = np.zeros((3, 2))
    for in_ax in range(3):
        col = r[:, in_ax]
        if np.allclose(col, 0):
            raise Mi3dError(f"orientation: stored axis {in_ax} has no direction in this affine (zero column)")
        out_ax = int(np.argmax(np.abs(col)))
        ornt[in_ax] = out_ax, (-1.0 if col[out_ax] < 0 else 1.0)
        r[out_ax, :] = 0          # no output axis twice
    return ornt


def ras_transform(affine):
    """Transform from the affine's orientation to ('R', 'A', 'S').  The target is the identity orientation, so it is the
    orientation itself (amos_ct_resample.py:30-32)."""
    return io_orientation(affine)


def _ornt(ornt):
    o = np.asarray(ornt, dtype=np.float64)
    if o.shape != (3, 2) or sorted(int(v) for v in o[:, 0]) != [0, 1, 2] or not np.all(np.abs(o[:, 1]) == 1):
        raise Mi3dError(f"orientation: not an orientation of three axes: {o.tolist()}")
    return o


def inv_ornt_aff(ornt, shape):
    """4x4 matrix from voxel indices of the reoriented array to voxel indices of the stored array of `shape`: the rows of
    the identity permuted by the output axes, then diag(flips, 1) with the translation flip * c - c, c = -(shape - 1) / 2,
    which mirrors a flipped axis about its centre."""
    o = _ornt(ornt)
    shape = np.asarray(shape, dtype=np.float64)
    if shape.shape != (3,):
        raise Mi3dError(f"orientation: three sides expected, got {shape.tolist()}")
    reorder = np.eye(4)[[int(v) for v in o[:, 0]] + [3], :]
    flip = np.diag(list(o[:, 1]) + [1.0])
    c = -(shape - 1) / 2.0
    flip[:3, 3] = o[:, 1] * c - c
    return flip @ reorder


def reoriented_affine(affine, shape):
    """Affine of the array reoriented to RAS (amos_ct_resample.py:35)."""
    a = _affine(affine)
    return a @ inv_ornt_aff(io_orientation(a), shape)


def spacing_of(affine):
    a = _affine(affine)
    return np.sqrt((a[:3, :3] ** 2).sum(axis=0))


def ras_shape(ornt, shape):
    o = _ornt(ornt)
    src = np.argsort(o[:, 0])
    return tuple(int(shape[int(i)]) for i in src)


def axis_map(affine, shape, strides):
    """What a kernel needs to read a stored array in RAS order: for each RAS axis (D, H, W) the tuple
    (side, element stride in the stored tensor, flipped).  Index r of a flipped axis is stored index side - 1 - r."""
    o = io_orientation(affine)
    if len(shape) != 3 or len(strides) != 3:
        raise Mi3dError(f"orientation: a 3-D array is expected, got shape {tuple(shape)} strides {tuple(strides)}")
    src = np.argsort(o[:, 0])          # RAS axis j is stored axis src[j]
    return tuple((int(shape[int(i)]), int(strides[int(i)]), bool(o[int(i), 1] < 0)) for i in src)


def check_dense(shape, strides, what="orientation"):
    """Raise unless (shape, strides) is a permutation of a contiguous array: every element once, no gap, no overlap."""
    if len(shape) != len(strides):
        raise Mi3dError(f"{what}: shape {tuple(shape)} and strides {tuple(strides)} differ in length")
    expect = 1
    for n, s in sorted(((int(n), int(s)) for n, s in zip(shape, strides) if int(n) != 1), key=lambda p: p[1]):
        if n < 1 or s != expect:
            raise Mi3dError(f"{what}: the tensor is not dense (shape {tuple(shape)}, strides {tuple(strides)}): "
                            "a permutation of a contiguous array is expected, without padding, overlap or stride 0")
        expect *= n
