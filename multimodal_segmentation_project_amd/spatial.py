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

The MONAI RandAffined / Rand3DElasticd block that the reference lists and leaves commented out (:227-248) is one smoothed random
displacement field (`mi3d_elastic_field`) and one gather (`mi3d_warp3`, csrc/warp.hip) that reads image and label through the SAME
coordinates, so the two cannot drift apart as two independently drawn RandAffined calls would:

  affine_matrix(rotate, scale)              float64 3x3, R_d @ R_h @ R_w @ diag(scale), acting on sampling coordinates (a pull)
  gaussian_taps(sigma)                      MONAI's GaussianFilter(sigma, truncated=3.0, approx="erf") table, float64, not renormalised
  displacement_field(shape, sigma, seed)    (3, D, H, W) float32: counter-hash noise in [-1, 1) smoothed along W, H, D, zero padded
  warp(image, label, matrix, ...)           the deterministic call: affine map + magnitude * field, one launch for image and label
  RandAffineElastic(...)                    dict-in / dict-out; draws from a numpy RandomState, ONE field call and ONE gather

    tf = RandAffineElastic(spatial_size=(96, 96, 96)).set_random_state(seed)      # also the random 96^3 patch of a 192^3 grid
    sample = combined_transform()(tf({'image': image, 'label': label}))

The arithmetic is stated operation by operation in include/mi3d.h and restated in float64 numpy by tests/warp_ref.py, which is pinned
to scipy.ndimage.correlate1d / map_coordinates; the GPU equals that model bit for bit.  Two differences from MONAI, both unpinned
(MONAI is not installed): the noise is a counter hash of (seed, voxel), not RandomState.uniform; coordinates are voxel-centred about
(n - 1) / 2 of each grid, not grid_sample's normalised ones.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import ELASTIC_MAX_RADIUS, PAD_BORDER, PAD_ZEROS, Mi3dError, call, ptr, stream_ptr
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


# ---------------------------------------------------------------------------------------- affine + elastic warp (csrc/warp.hip)
PADDING = {"border": PAD_BORDER, "zeros": PAD_ZEROS}


def affine_matrix(rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """float64 3x3 matrix R_d @ R_h @ R_w @ diag(scale) over the axes (D, H, W).  rotate = (rd, rh, rw) in radians; R_x turns the
    plane of the other two axes about axis x, counter-clockwise from the first of them towards the second:
        R_d = [[1, 0, 0], [0, c, -s], [0, s, c]]    R_h = [[c, 0, s], [0, 1, 0], [-s, 0, c]]    R_w = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    with c, s = cos, sin of that axis' angle.  The matrix maps OUTPUT coordinates to SAMPLING coordinates (a pull, as MONAI's
    affine grid): scale > 1 samples further out, so the content shrinks."""
    try:
        (rd, rh, rw), (sd, sh, sw) = (float(r) for r in rotate), (float(x) for x in scale)
    except (TypeError, ValueError):
        raise Mi3dError(f"affine_matrix: rotate and scale take three numbers each, got {rotate} and {scale}") from None
    (cd, sd_), (ch, sh_), (cw, sw_) = ((math.cos(a), math.sin(a)) for a in (rd, rh, rw))
    r_d = np.array([[1, 0, 0], [0, cd, -sd_], [0, sd_, cd]], dtype=np.float64)
    r_h = np.array([[ch, 0, sh_], [0, 1, 0], [-sh_, 0, ch]], dtype=np.float64)
    r_w = np.array([[cw, -sw_, 0], [sw_, cw, 0], [0, 0, 1]], dtype=np.float64)
    return r_d @ r_h @ r_w @ np.diag(np.array([sd, sh, sw], dtype=np.float64))


def gaussian_taps(sigma):
    """The float64 table g[-R..R] of MONAI's GaussianFilter(sigma, truncated=3.0, approx="erf"): R = int(max(3 sigma, 0.5) + 0.5),
    t = 0.70710678 / |sigma|, g[x] = max(0, 0.5 (erf(t (x + 0.5)) - erf(t (x - 0.5)))).  Not renormalised."""
    sigma = float(sigma)
    if not sigma > 0.0 or not math.isfinite(sigma):
        raise Mi3dError(f"gaussian_taps: sigma must be positive and finite, got {sigma}")
    radius = int(max(sigma * 3.0, 0.5) + 0.5)
    t = 0.70710678 / abs(sigma)
    return np.array([max(0.0, 0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5)))) for x in range(-radius, radius + 1)],
                    dtype=np.float64)


def _grid_shape(shape, what):
    try:
        shape = tuple(int(n) for n in shape)
    except (TypeError, ValueError):
        shape = ()
    if len(shape) != 3 or min(shape) < 1:
        raise Mi3dError(f"{what}: expected three positive sides (D, H, W), got {shape}")
    return shape


def displacement_field(shape, sigma=None, seed=0, taps=None, device=None):
    """(3, D, H, W) float32 CUDA tensor: component a displaces along axis a of (D, H, W), in units of `magnitude` voxels.  Noise
    in [-1, 1) from the counter hash of (seed, component, voxel), smoothed with gaussian_taps(sigma) along W, H, D with zeros beyond
    the volume (include/mi3d.h mi3d_elastic_field).  taps: another odd-length float64 table instead of sigma's."""
    shape = _grid_shape(shape, "displacement_field")
    if (sigma is None) == (taps is None):
        raise Mi3dError("displacement_field: give sigma OR taps")
    taps = np.ascontiguousarray(gaussian_taps(sigma) if taps is None else taps, dtype=np.float64)
    if taps.ndim != 1 or taps.size % 2 != 1:
        raise Mi3dError(f"displacement_field: taps must be a 1-D table of odd length, got shape {taps.shape}")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise Mi3dError(f"displacement_field: seed must fit 64 unsigned bits, got {seed}")
    if not torch.cuda.is_available():
        raise Mi3dError("displacement_field: no GPU (the MI355X HIP path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(device):
        field = torch.empty((3,) + shape, dtype=torch.float32, device=device)
        nbytes = _lib.lib().mi3d_elastic_workspace_bytes(*shape)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        call("mi3d_elastic_field", ptr(field), *shape, seed, taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size // 2, ptr(ws), nbytes,
             stream_ptr())
    return field


def warp(image, label, matrix=None, translate=None, sigma=None, magnitude=None, seed=None, out_shape=None, image_padding="border",
         label_padding="zeros", field=None):
    """Affine + elastic warp of one (C, D, H, W) sample in ONE gather; either of image / label may be None.  Per output voxel o the
    sampling point is  matrix @ (o - (no - 1)/2 + magnitude * u[o]) + (n - 1)/2 + translate  (include/mi3d.h mi3d_warp3): the image
    is read with scipy.ndimage.map_coordinates(order=1), the label with order=0, both through the same coordinates.
    matrix: 3x3 (default identity, see affine_matrix), translate: 3 (default 0), in input voxels.  The field u is EITHER drawn here,
    displacement_field(out_shape, sigma, seed), OR given as `field` (3, Do, Ho, Wo); both need magnitude.  out_shape (Do, Ho, Wo)
    defaults to the input's; a smaller one is a centred crop window, a larger one pads.  Padding: "border" (scipy mode='nearest') or
    "zeros" (mode='constant', cval=0).  float32 image / int64 label CUDA tensors (numpy or CPU inputs are uploaded); returns fresh
    tensors (image, label)."""
    if image is None and label is None:
        raise Mi3dError("warp: image and label are both None")
    for mode in (image_padding, label_padding):
        if mode not in PADDING:
            raise Mi3dError(f"warp: unknown padding mode {mode!r}; one of {sorted(PADDING)}")
    if sigma is not None and field is not None:
        raise Mi3dError("warp: give sigma (with seed) OR field, not both")
    if (sigma is not None or field is not None) and magnitude is None:
        raise Mi3dError("warp: a displacement field needs magnitude")
    if magnitude is not None and sigma is None and field is None:
        raise Mi3dError("warp: magnitude without sigma or field")
    if seed is not None and sigma is None:
        raise Mi3dError("warp: seed without sigma")
    shapes = {tuple(x.shape) for x in (image, label) if x is not None}
    if len(shapes) != 1:
        raise Mi3dError(f"warp: image and label differ in shape: {sorted(shapes)}")
    shape = shapes.pop()
    if len(shape) != 4 or min(shape) < 1:
        raise Mi3dError(f"warp: expected a non-empty (C, D, H, W) volume, got shape {shape}")
    out_shape = shape[1:] if out_shape is None else _grid_shape(out_shape, "warp: out_shape")
    matrix = np.ascontiguousarray(np.eye(3) if matrix is None else matrix, dtype=np.float64)
    translate = np.ascontiguousarray(np.zeros(3) if translate is None else translate, dtype=np.float64)
    if matrix.shape != (3, 3) or translate.shape != (3,):
        raise Mi3dError(f"warp: matrix must be 3x3 and translate 3, got {matrix.shape} and {translate.shape}")
    x = _device_volume(image, torch.float32) if image is not None else None
    y = _device_volume(label, torch.int64) if label is not None else None
    if x is not None and y is not None and x.device != y.device:
        raise Mi3dError(f"warp: image on {x.device}, label on {y.device}")
    device = (x if x is not None else y).device
    if sigma is not None:
        field = displacement_field(out_shape, sigma, 0 if seed is None else seed, device=device)
    elif field is not None:
        if not isinstance(field, torch.Tensor) or not field.is_cuda or field.dtype != torch.float32 or field.device != device:
            raise Mi3dError("warp: field must be a float32 CUDA tensor on the sample's device (displacement_field makes one)")
        if tuple(field.shape) != (3,) + tuple(out_shape):
            raise Mi3dError(f"warp: field has shape {tuple(field.shape)}, the output grid wants {(3,) + tuple(out_shape)}")
        field = field.contiguous()
    with torch.cuda.device(device):
        out_x = torch.empty((shape[0],) + tuple(out_shape), dtype=torch.float32, device=device) if x is not None else None
        out_y = torch.empty((shape[0],) + tuple(out_shape), dtype=torch.int64, device=device) if y is not None else None
        dp = C.POINTER(C.c_double)
        call("mi3d_warp3", ptr(x), ptr(out_x), ptr(y), ptr(out_y), *shape, *out_shape, matrix.ctypes.data_as(dp),
             translate.ctypes.data_as(dp), ptr(field), 0.0 if magnitude is None else float(magnitude), PADDING[image_padding],
             PADDING[label_padding], stream_ptr())
    return out_x, out_y


def _range3(r, what):
    if r is None:
        return None
    try:
        r = tuple(float(v) for v in r)
    except (TypeError, ValueError):
        r = ()
    if len(r) != 3 or min(r) < 0.0:
        raise Mi3dError(f"RandAffineElastic: {what} takes three non-negative half-widths, got {r}")
    return r


def _range2(r, what):
    if r is None:
        return None
    try:
        r = tuple(float(v) for v in r)
    except (TypeError, ValueError):
        r = ()
    if len(r) != 2 or not 0.0 <= r[0] <= r[1]:
        raise Mi3dError(f"RandAffineElastic: {what} takes (low, high) with 0 <= low <= high, got {r}")
    return r


class RandAffineElastic:
    """The reference's commented-out RandAffined + Rand3DElasticd (utils/dataloader.py:227-248) on {'image': ..., 'label': ...}, one
    field call and one gather; other keys pass through.  draw() takes from a numpy RandomState, in this order:
        1. the apply decision, rand() < prob                       (always drawn)
        2. three angles, uniform(-r, r) per axis D, H, W           (rotate_range; None: no draws, no rotation)
        3. three scales, 1 + uniform(-r, r) per axis               (scale_range; None: no draws, scale 1)
        4. sigma, uniform(sigma_range)                             (sigma_range; None: no draws 4-6, no field)
        5. magnitude, uniform(magnitude_range)
        6. the field's seed, randint(0, 2^63)
    Draws 2-6 are skipped when the decision is "no".  Then the sample passes through unchanged, or, with spatial_size, is cut to the
    centred window of that size.  spatial_size (Do, Ho, Wo): the output grid (the 96^3 training patch of a 192^3 grid); None keeps
    the input's.  The parameters of draw() replay through warp(image, label, **params)."""

    def __init__(self, rotate_range=(0.1, 0.1, 0.1), scale_range=(0.1, 0.1, 0.1), sigma_range=(5, 8), magnitude_range=(100, 200),
                 prob=1.0, spatial_size=None, image_padding="border", label_padding="zeros"):
        self.rotate_range, self.scale_range = _range3(rotate_range, "rotate_range"), _range3(scale_range, "scale_range")
        self.sigma_range = _range2(sigma_range, "sigma_range")
        self.magnitude_range = _range2(magnitude_range, "magnitude_range") if self.sigma_range is not None else None
        if self.sigma_range is not None and self.magnitude_range is None:
            raise Mi3dError("RandAffineElastic: sigma_range needs magnitude_range")
        if self.sigma_range is not None and not 0.0 < self.sigma_range[0]:
            raise Mi3dError(f"RandAffineElastic: sigma must be positive, got {self.sigma_range}")
        self.prob = float(prob)
        self.spatial_size = None if spatial_size is None else _grid_shape(spatial_size, "RandAffineElastic: spatial_size")
        for mode in (image_padding, label_padding):
            if mode not in PADDING:
                raise Mi3dError(f"RandAffineElastic: unknown padding mode {mode!r}; one of {sorted(PADDING)}")
        self.image_padding, self.label_padding = image_padding, label_padding
        self.set_random_state(None)

    def set_random_state(self, seed=None):
        self.R = np.random.RandomState(seed)
        return self

    def draw(self):
        """None when the apply decision is "no"; otherwise the keyword arguments of warp() for this sample: matrix, sigma, magnitude,
        seed (the last three None without sigma_range)."""
        R = self.R
        if not R.rand() < self.prob:
            return None
        rotate = tuple(float(R.uniform(-r, r)) for r in self.rotate_range) if self.rotate_range is not None else (0.0, 0.0, 0.0)
        scale = tuple(1.0 + float(R.uniform(-r, r)) for r in self.scale_range) if self.scale_range is not None else (1.0, 1.0, 1.0)
        p = {"matrix": affine_matrix(rotate, scale), "sigma": None, "magnitude": None, "seed": None}
        if self.sigma_range is not None:
            p["sigma"] = float(R.uniform(*self.sigma_range))
            p["magnitude"] = float(R.uniform(*self.magnitude_range))
            p["seed"] = int(R.randint(0, 2 ** 63, dtype=np.int64))
        return p

    def __call__(self, sample):
        p = self.draw()
        out = dict(sample)
        if p is None and self.spatial_size is None:
            return out
        image, label = warp(sample.get("image"), sample.get("label"), out_shape=self.spatial_size, image_padding=self.image_padding,
                            label_padding=self.label_padding, **(p or {}))
        if image is not None:
            out["image"] = image
        if label is not None:
            out["label"] = label
        return out
