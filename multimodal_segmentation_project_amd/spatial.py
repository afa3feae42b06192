"""GPU mirror of the reference's two spatial augmentation helpers (utils/dataloader.py):

  random_flip(image, label)                 :207-213  np.flip over axes 1, 2, 3, each when random.random() > 0.5
  random_rotate(image, label, max_angle)    :215-221  one scipy.ndimage.rotate(..., reshape=False, mode='nearest') in a randomly
                                                      chosen plane, order=1 for the image and order=0 for the label

The host draws the few random scalars from Python's `random` module in the reference's order, so random.seed(k) reproduces the
reference's decisions; the per-voxel work is one gather pass over image and label (`mi3d_plane_affine`, csrc/spatial.hip).

  rotation_plane(plane_shape, angle)        (matrix, offset) of the rotation as scipy.ndimage.rotate computes them, float64
  flip_rotate(image, label, flips, ...)     the deterministic call: flips, then one in-plane rotation or affine map, one launch
  random_flip / random_rotate               the reference's names and signatures
  SpatialTransform(flip, max_angle)         dict-in / dict-out like CombinedTransform; draws flip then rotate, ONE launch

    tf, aug = SpatialTransform(), combined_transform()
    sample = aug(tf({'image': image, 'label': label}))      # spatial first, then the intensity chain

The MONAI RandAffined / Rand3DElasticd block that the reference leaves commented out (:227-248) is not mirrored.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import Mi3dError, call, ptr, stream_ptr
from .augment import _device_volume

PLANES = [(1, 2), (1, 3), (2, 3)]      # random_rotate's list, in its order (utils/dataloader.py:216)

try:
    from scipy.special import cosdg as _cosdg, sindg as _sindg
except ImportError:                    # labels lying exactly on a rounding boundary may then differ from scipy's (rotation_plane)
    _cosdg = _sindg = None


def rotation_plane(plane_shape, angle):
    """(matrix, offset) of scipy.ndimage.rotate(angle, reshape=False) for a plane of shape (n0, n1), as scipy computes them:
    c, s = cosdg(angle), sindg(angle); matrix = [[c, s], [-s, c]]; offset = (n - 1) / 2 - matrix @ ((n - 1) / 2), float64.
    Where scipy.special does not import, c and s come from math.cos / math.sin(math.radians(angle)), which can differ from
    cosdg / sindg in the last bits (and are not exact at multiples of 90 degrees): an output voxel whose source coordinate lies
    exactly on a rounding boundary of floor(cc + 0.5) may then read another label than scipy's rotate would."""
    n = np.asarray(plane_shape, dtype=np.int64)
    if n.shape != (2,) or n.min() < 1:
        raise Mi3dError(f"rotation_plane: a plane has two positive sides, got {tuple(plane_shape)}")
    angle = float(angle)
    if _cosdg is not None:
        c, s = float(_cosdg(angle)), float(_sindg(angle))
    else:
        c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    matrix = np.array([[c, s], [-s, c]], dtype=np.float64)
    centre = (n - 1) / 2
    return matrix, centre - matrix @ centre


def _plane_axes(axes):
    try:
        a = sorted(int(x) + 4 if int(x) < 0 else int(x) for x in axes)
    except (TypeError, ValueError):
        a = []
    if len(a) != 2 or not 1 <= a[0] < a[1] <= 3:
        raise Mi3dError(f"flip_rotate: axes must be two different spatial axes of (C, D, H, W) out of 1, 2, 3, got {axes}")
    return a


def flip_rotate(image, label, flips=(False, False, False), angle=None, axes=None, matrix=None, offset=None):
    """rotate(flip(image)), rotate(flip(label)) of one (C, D, H, W) sample in ONE launch; either of image / label may be None.
    flips: reverse axis 1, 2, 3 (np.flip).  Then EITHER angle (degrees) with axes: scipy.ndimage.rotate(x, angle, axes=axes,
    reshape=False, mode='nearest'), order=1 for the image and order=0 for the label, OR matrix (2x2) and offset (2) with axes:
    scipy.ndimage.affine_transform of every plane parallel to the two axes, same orders and mode; neither: the flips alone.
    float32 image / int64 label CUDA tensors (numpy or CPU inputs are uploaded); returns fresh tensors (image, label)."""
    if image is None and label is None:
        raise Mi3dError("flip_rotate: image and label are both None")
    flips = tuple(bool(f) for f in flips)
    if len(flips) != 3:
        raise Mi3dError(f"flip_rotate: flips takes one flag per axis 1, 2, 3, got {len(flips)}")
    if angle is not None and (matrix is not None or offset is not None):
        raise Mi3dError("flip_rotate: give angle OR matrix and offset, not both")
    if (matrix is None) != (offset is None):
        raise Mi3dError("flip_rotate: matrix and offset come together")
    if (angle is not None or matrix is not None) and axes is None:
        raise Mi3dError("flip_rotate: a rotation needs axes, the two axes of its plane")
    ax = _plane_axes(axes) if axes is not None else [1, 2]
    shapes = {tuple(x.shape) for x in (image, label) if x is not None}
    if len(shapes) != 1:
        raise Mi3dError(f"flip_rotate: image and label differ in shape: {sorted(shapes)}")
    shape = shapes.pop()
    if len(shape) != 4 or min(shape) < 1:
        raise Mi3dError(f"flip_rotate: expected a non-empty (C, D, H, W) volume, got shape {shape}")
    if angle is not None:
        matrix, offset = rotation_plane((shape[ax[0]], shape[ax[1]]), angle)
    elif matrix is None:
        matrix, offset = np.eye(2), np.zeros(2)
    matrix, offset = np.ascontiguousarray(matrix, dtype=np.float64), np.ascontiguousarray(offset, dtype=np.float64)
    if matrix.shape != (2, 2) or offset.shape != (2,):
        raise Mi3dError(f"flip_rotate: matrix must be 2x2 and offset 2, got {matrix.shape} and {offset.shape}")
    x = _device_volume(image, torch.float32) if image is not None else None
    y = _device_volume(label, torch.int64) if label is not None else None
    if x is not None and y is not None and x.device != y.device:
        raise Mi3dError(f"flip_rotate: image on {x.device}, label on {y.device}")
    out_x = torch.empty_like(x) if x is not None else None
    out_y = torch.empty_like(y) if y is not None else None
    dp = C.POINTER(C.c_double)
    call("mi3d_plane_affine", ptr(x), ptr(out_x), ptr(y), ptr(out_y), *shape, ax[0], ax[1], matrix.ctypes.data_as(dp),
         offset.ctypes.data_as(dp), sum(int(f) << k for k, f in enumerate(flips)), stream_ptr())
    return out_x, out_y


def _draw_flips(rng):
    return tuple(rng.random() > 0.5 for _ in (1, 2, 3))                  # utils/dataloader.py:208-210


def _draw_rotation(rng, max_angle):
    angle = rng.uniform(-max_angle, max_angle)                           # :217
    return angle, rng.choice(PLANES)                                     # :218


def random_flip(image, label):
    """utils/dataloader.py:207-213, the draws taken from Python's `random` module in the same order."""
    return flip_rotate(image, label, flips=_draw_flips(random))


def random_rotate(image, label, max_angle=15):
    """utils/dataloader.py:215-221, the draws taken from Python's `random` module in the same order."""
    angle, axes = _draw_rotation(random, max_angle)
    return flip_rotate(image, label, angle=angle, axes=axes)


class SpatialTransform:
    """random_flip then random_rotate of {'image': ..., 'label': ...} in one launch; other keys pass through.  flip=False or
    max_angle=None leaves that transform (and its draws) out.  rng: a random.Random; default, the `random` module itself."""

    def __init__(self, flip=True, max_angle=15, rng=None):
        self.flip, self.max_angle, self.rng = bool(flip), max_angle, rng if rng is not None else random

    def draw(self):
        """(flips, angle or None, axes or None), drawn as random_flip followed by random_rotate would."""
        flips = _draw_flips(self.rng) if self.flip else (False, False, False)
        angle, axes = _draw_rotation(self.rng, self.max_angle) if self.max_angle is not None else (None, None)
        return flips, angle, axes

    def __call__(self, sample):
        flips, angle, axes = self.draw()
        out = dict(sample)
        image, label = flip_rotate(sample.get("image"), sample.get("label"), flips=flips, angle=angle, axes=axes)
        if image is not None:
            out["image"] = image
        if label is not None:
            out["label"] = label
        return out
