"""numpy restatement of what the resampling scripts do around their zoom calls (scripts/resampling/amos_ct_resample.py:29-36,
resample_totalseg_ras_mri.py:77-96): applying an orientation to an array, and the per-organ mask merge.  The checker of the
orientation tests: independent of the product module, written from the operations' definitions (flip the marked stored axes,
then transpose so that stored axis i lands on its output axis)."""
import itertools

import numpy as np

SHAPE = (5, 9, 14)
SPACING = (0.7, 1.3, 5.0)
ROTATIONS = (None, (0, 20.0), (1, -17.0), (2, 31.0))      # (world axis, degrees): well away from the 45-degree tie


def signed_permutations():
    """The 48 orientations: (perm, signs) = stored axis i runs along world axis perm[i] in direction signs[i]."""
    return [(p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]


def rotation(axis, degrees):
    c, s = np.cos(np.deg2rad(degrees)), np.sin(np.deg2rad(degrees))
    a, b = [i for i in range(3) if i != axis]
    r = np.eye(3)
    r[a, a], r[a, b], r[b, a], r[b, b] = c, -s, s, c
    return r


def affine_for(perm, signs, spacing=SPACING, rot=None, origin=(-31.5, 12.25, 100.0)):
    """Affine of a stored array whose axis i runs along world axis perm[i], direction signs[i], step spacing[i]."""
    a = np.eye(4)
    m = np.zeros((3, 3))
    for i in range(3):
        m[perm[i], i] = signs[i] * spacing[i]
    if rot is not None:
        m = rotation(*rot) @ m
    a[:3, :3] = m
    a[:3, 3] = origin
    return a


def reorient(arr, ornt):
    """Apply an orientation ((3, 2): output axis and direction per stored axis): flip, then transpose."""
    ornt = np.asarray(ornt)
    for ax in range(3):
        if ornt[ax, 1] < 0:
            arr = np.flip(arr, axis=ax)
    return arr.transpose(np.argsort(ornt[:, 0]))


def store_as(ras, perm, signs):
    """The inverse: how a RAS array is stored under (perm, signs); reorient(store_as(x)) == x."""
    arr = np.transpose(ras, perm)
    for ax in range(3):
        if signs[ax] < 0:
            arr = np.flip(arr, axis=ax)
    return arr


def ornt_of(perm, signs):
    return np.array([[perm[i], signs[i]] for i in range(3)], dtype=np.float64)


def merge_loop(resized_masks, values, shape):
    """The script's loop (resample_totalseg_ras_mri.py:82-96) over the already resized masks, in list order."""
    combined = np.zeros(shape, dtype=np.int64)
    for m, v in zip(resized_masks, values):
        combined[m > 0] = v
    return combined
