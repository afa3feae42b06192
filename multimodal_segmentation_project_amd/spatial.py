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

    tf = RandAffineElastic(spatial_size=(96, 96, 96)).set_random_state(seed)      # and the centred 96^3 window of a 192^3 grid
    sample = combined_transform()(tf({'image': image, 'label': label}))

RandAffineElastic alone always cuts the CENTRED window.  Where the window goes is the patch sampler's part (csrc/patch.hip): MONAI's
RandCropByPosNegLabeld / RandCropByLabelClassesd without np.nonzero, without an index list and without a count reaching the host:

  PatchSampler(spatial_size, group_of, weights)   draws (sample, group, 64-bit word) per patch on the host, counts never needed
  RandCropByPosNegLabel / RandCropByLabelClasses  its two configurations; dict in, a list of num_samples dicts out
  pick_starts(label, sample, group, rnd, ...)     count + pick on the device: the r-th voxel of a group, r = mulhi64(word, count)
  crop_patches(image, label, starts, size)        K windows of image and label in one launch, starts read from device memory
  warp(..., start=) / RandAffineElastic(crop=)    the affine + elastic gather placed on a picked start instead of on the centre

    crop = RandCropByPosNegLabel((96, 96, 96), pos=2, neg=1, num_samples=2).set_random_state(seed)
    patches = crop({'image': image, 'label': label})        # 2 dicts; crop.last_batch holds the stacked (2, C, 96, 96, 96) tensors

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
from ._lib import ELASTIC_MAX_RADIUS, PAD_BORDER, PAD_ZEROS, PATCH_BLOCK, Mi3dError, call, ptr, stream_ptr
from ._volume import _integer, _samples, _strides, _workspace
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
         label_padding="zeros", field=None, start=None):
    """Affine + elastic warp of one (C, D, H, W) sample in ONE gather; either of image / label may be None.  Per output voxel o the
    sampling point is  matrix @ (o - (no - 1)/2 + magnitude * u[o]) + (n - 1)/2 + translate  (include/mi3d.h mi3d_warp3): the image
    is read with scipy.ndimage.map_coordinates(order=1), the label with order=0, both through the same coordinates.
    matrix: 3x3 (default identity, see affine_matrix), translate: 3 (default 0), in input voxels.  The field u is EITHER drawn here,
    displacement_field(out_shape, sigma, seed), OR given as `field` (3, Do, Ho, Wo); both need magnitude.  out_shape (Do, Ho, Wo)
    defaults to the input's; a smaller one is a centred crop window, a larger one pads.  Padding: "border" (scipy mode='nearest') or
    "zeros" (mode='constant', cval=0).  start: None, or three int32 on the device (a row of pick_starts' starts), the input voxel under
    the window's first voxel: the window's middle then sits at start + (no - 1)/2 instead of (n - 1)/2 (mi3d_warp3_at); the values are
    read by the kernel, never by the host.  float32 image / int64 label CUDA tensors (numpy or CPU inputs are uploaded); returns fresh
    tensors (image, label)."""
    if image is None and label is None:
        raise Mi3dError("warp: image and label are both None")
    if start is not None and not (isinstance(start, torch.Tensor) and start.is_cuda and start.dtype == torch.int32 and
                                  tuple(start.shape) == (3,) and start.is_contiguous()):
        raise Mi3dError("warp: start is a contiguous int32 CUDA tensor of 3 (a row of pick_starts' starts)")
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
    if start is not None and start.device != device:
        raise Mi3dError(f"warp: start on {start.device}, the sample on {device}")
    with torch.cuda.device(device):
        out_x = torch.empty((shape[0],) + tuple(out_shape), dtype=torch.float32, device=device) if x is not None else None
        out_y = torch.empty((shape[0],) + tuple(out_shape), dtype=torch.int64, device=device) if y is not None else None
        dp = C.POINTER(C.c_double)
        args = (ptr(x), ptr(out_x), ptr(y), ptr(out_y), *shape, *out_shape, matrix.ctypes.data_as(dp), translate.ctypes.data_as(dp),
                ptr(field), 0.0 if magnitude is None else float(magnitude), PADDING[image_padding], PADDING[label_padding])
        if start is None:
            call("mi3d_warp3", *args, stream_ptr())
        else:
            call("mi3d_warp3_at", *args, ptr(start), stream_ptr())
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
    the input's.  The parameters of draw() replay through warp(image, label, **params).
    crop: None, or a PatchSampler that places the window.  Each call then takes ONE location from the sampler's own RandomState
    (crop.draw_one(); the draws above do not move), picks its start on the device from channel 0 of the label (count -> pick) and
    runs the gather there, warp(start=); the output grid is spatial_size, or the sampler's where that is None.  The location of the
    last call stays in crop.last_draw and crop.last_pick = (starts, voxel, picked, counts)."""

    def __init__(self, rotate_range=(0.1, 0.1, 0.1), scale_range=(0.1, 0.1, 0.1), sigma_range=(5, 8), magnitude_range=(100, 200),
                 prob=1.0, spatial_size=None, image_padding="border", label_padding="zeros", crop=None):
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
        if crop is not None and not isinstance(crop, PatchSampler):
            raise Mi3dError(f"RandAffineElastic: crop is a PatchSampler, got {type(crop).__name__}")
        self.crop = crop
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
        if self.crop is not None:
            image, label = self.crop.warp_at(sample.get("image"), sample.get("label"), out_shape=self.spatial_size,
                                             image_padding=self.image_padding, label_padding=self.label_padding, **(p or {}))
        elif p is None and self.spatial_size is None:
            return out
        else:
            image, label = warp(sample.get("image"), sample.get("label"), out_shape=self.spatial_size,
                                image_padding=self.image_padding, label_padding=self.label_padding, **(p or {}))
        if image is not None:
            out["image"] = image
        if label is not None:
            out["label"] = label
        return out


# ------------------------------------------------------------------------- foreground-balanced patch sampling (csrc/patch.hip)
MAX_GROUPS = _lib.COMPONENTS_MAX_CLASSES
NO_GROUP = 255
MAX_DRAWS = 65535
_PICKABLE = (torch.uint8, torch.int64)


def _group_table(group_of, what):
    """(the 256-byte host table, G = 1 + the largest group it names) of a sequence of 256 entries in 0..7 or 255."""
    try:
        entries = [_integer(g, what, "group_of entry") for g in group_of]
    except TypeError:
        raise Mi3dError(f"{what}: group_of is a sequence of 256 integers, got {type(group_of).__name__}") from None
    if len(entries) != 256:
        raise Mi3dError(f"{what}: group_of has one entry per label value 0..255, got {len(entries)}")
    for v, g in enumerate(entries):
        if not (0 <= g < MAX_GROUPS or g == NO_GROUP):
            raise Mi3dError(f"{what}: group_of[{v}] = {g} is neither a group 0..{MAX_GROUPS - 1} nor {NO_GROUP} (in no group)")
    named = [g for g in entries if g != NO_GROUP]
    if not named:
        raise Mi3dError(f"{what}: group_of names no group")
    return (C.c_uint8 * 256)(*entries), max(named) + 1


def _pick_view(label, what):
    """The (N, D, H, W) view of the label a location is picked from, its dtype code and whether it came as (D, H, W)."""
    if isinstance(label, torch.Tensor) and label.dim() == 5:
        if label.shape[1] != 1:
            raise Mi3dError(f"{what}: a (N, 1, D, H, W) label has one channel, got {tuple(label.shape)}")
        label = label[:, 0]
    return _samples(label, what)


def _window(spatial_size, sides, what):
    size = _grid_shape(spatial_size, f"{what}: spatial_size")
    if any(s > n for s, n in zip(size, sides)):
        raise Mi3dError(f"{what}: a window of {size} does not fit a volume of {tuple(int(n) for n in sides)}")
    return size


def _draw_arrays(sample, group, rnd, n, groups, what):
    """The three host arrays of K draws, checked: sample in [0, n), group in [0, groups), rnd a 64-bit word."""
    try:
        sample, group = [_integer(v, what, "sample") for v in sample], [_integer(v, what, "group") for v in group]
        rnd = [_integer(v, what, "rnd") for v in rnd]
    except TypeError:
        raise Mi3dError(f"{what}: sample, group and rnd are sequences of integers") from None
    k = len(sample)
    if len(group) != k or len(rnd) != k:
        raise Mi3dError(f"{what}: sample, group and rnd differ in length: {k}, {len(group)}, {len(rnd)}")
    if not 1 <= k <= MAX_DRAWS:
        raise Mi3dError(f"{what}: 1 to {MAX_DRAWS} draws, got {k}")
    for i in range(k):
        if not 0 <= sample[i] < n:
            raise Mi3dError(f"{what}: draw {i} names sample {sample[i]} of {n}")
        if not 0 <= group[i] < groups:
            raise Mi3dError(f"{what}: draw {i} names group {group[i]} of {groups}")
        if not 0 <= rnd[i] < 2 ** 64:
            raise Mi3dError(f"{what}: draw {i}: rnd {rnd[i]} is not an unsigned 64-bit word")
    return k, (C.c_int32 * k)(*sample), (C.c_int32 * k)(*group), (C.c_uint64 * k)(*rnd)


def pick_starts(label, sample, group, rnd, spatial_size, group_of):
    """Where K windows go, found on the device: (starts (K, 3) int32, voxel (K,) int32, picked (K,) int32, counts (N, G) int64), all
    CUDA tensors (include/mi3d.h mi3d_patch_count / mi3d_patch_pick).  label: (D, H, W), (N, D, H, W) or (N, 1, D, H, W), uint8 or
    int64 on the GPU, dense with any strides; counts is (G,) for a (D, H, W) label.  group_of: 256 entries, the group 0..7 of every
    label value or 255 for none; G = 1 + the largest group.  Draw k takes the r-th voxel (C order, from 0) of group[k] in sample[k],
    r = floor(rnd[k] * count / 2^64); where that group is absent it takes voxel floor(rnd[k] * V / 2^64) and picked[k] is -1,
    else picked[k] = group[k].  starts[k] = clamp(voxel's coordinates - size // 2, 0, sides - size).  sample, group, rnd: host
    sequences of K integers (PatchSampler.draw makes them).  Two launches; nothing synchronises and no count reaches the host."""
    what = "pick_starts"
    t, code, single = _pick_view(label, what)
    table, groups = _group_table(group_of, what)
    size = _window(spatial_size, t.shape[1:], what)
    k, c_sample, c_group, c_rnd = _draw_arrays(sample, group, rnd, t.shape[0], groups, what)
    _lib.require_cuda(t, what)
    nbytes = _workspace("mi3d_patch_workspace_bytes", t, what)
    # everything is checked: allocate and launch
    with torch.cuda.device(t.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
        counts = torch.empty((t.shape[0], groups), dtype=torch.int64, device=t.device)
        starts = torch.empty((k, 3), dtype=torch.int32, device=t.device)
        voxel = torch.empty(k, dtype=torch.int32, device=t.device)
        picked = torch.empty(k, dtype=torch.int32, device=t.device)
        call("mi3d_patch_count", ptr(t), code, *t.shape, *_strides(t), table, ptr(counts), ptr(ws), nbytes, stream_ptr())
        call("mi3d_patch_pick", ptr(t), code, *t.shape, *_strides(t), table, k, c_sample, c_group, c_rnd, _lib.int_table(size),
             ptr(starts), ptr(voxel), ptr(picked), ptr(ws), nbytes, stream_ptr())
    return starts, voxel, picked, counts[0] if single else counts


def crop_patches(image, label, starts, spatial_size):
    """K windows of one (C, D, H, W) sample in ONE launch: (image (K, C, Do, Ho, Wo) float32, label (K, C, Do, Ho, Wo) int64); either
    of image / label may be None.  starts: (K, 3) int32 on the device (pick_starts makes them), read by the kernel, never by the
    host; a start is clamped to [0, sides - size] where it is used.  A copy: every bit pattern of the image is kept.  float32
    image / int64 label CUDA tensors (numpy or CPU inputs are uploaded)."""
    what = "crop_patches"
    if image is None and label is None:
        raise Mi3dError(f"{what}: image and label are both None")
    shapes = {tuple(x.shape) for x in (image, label) if x is not None}
    if len(shapes) != 1:
        raise Mi3dError(f"{what}: image and label differ in shape: {sorted(shapes)}")
    shape = shapes.pop()
    if len(shape) != 4 or min(shape) < 1:
        raise Mi3dError(f"{what}: expected a non-empty (C, D, H, W) volume, got shape {shape}")
    size = _window(spatial_size, shape[1:], what)
    if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.dtype == torch.int32 and starts.dim() == 2 and
            starts.shape[1] == 3 and starts.is_contiguous()):
        raise Mi3dError(f"{what}: starts is a contiguous (K, 3) int32 CUDA tensor (pick_starts makes one)")
    k = starts.shape[0]
    if not 1 <= k <= MAX_DRAWS:
        raise Mi3dError(f"{what}: 1 to {MAX_DRAWS} windows, got {k}")
    x = _device_volume(image, torch.float32) if image is not None else None
    y = _device_volume(label, torch.int64) if label is not None else None
    for v in (x, y):
        if v is not None and v.device != starts.device:
            raise Mi3dError(f"{what}: starts on {starts.device}, the sample on {v.device}")
    with torch.cuda.device(starts.device):
        out_x = torch.empty((k, shape[0]) + size, dtype=torch.float32, device=starts.device) if x is not None else None
        out_y = torch.empty((k, shape[0]) + size, dtype=torch.int64, device=starts.device) if y is not None else None
        call("mi3d_patch_crop", ptr(x), ptr(out_x), ptr(y), ptr(out_y), k, *shape, *size, ptr(starts), stream_ptr())
    return out_x, out_y


class PatchSampler:
    """Random windows of spatial_size, oversampled on chosen label groups.  group_of: 256 entries, the group 0..7 of every label value or
    255 for "in no group"; weights: one non-negative number per group, how often a window is centred on a voxel of that group.
    draw(n_volumes) takes from a numpy RandomState, per volume and per sample of it, in this order:
        1. the group: rand(), mapped through the cumulative normalised weights (a zero-weight group is never drawn)
        2. the voxel's rank as a 64-bit word: randint(0, 2^64, dtype=uint64)
    The word becomes a rank on the device, floor(word * count / 2^64), so the host never learns a count: the stream of draws differs
    from MONAI's randint(len(indices)).  A group that a scan lacks falls back to a uniformly drawn voxel (picked = -1).
    Called on {'image': (C, D, H, W), 'label': (C, D, H, W)} it returns a list of num_samples dicts whose image / label are views of one
    stacked (K, C, Do, Ho, Wo) allocation; other keys pass through; locations come from channel 0 of the label.  last_batch =
    (image, label, starts, picked) of the last call, all on the device."""

    def __init__(self, spatial_size, group_of, weights, num_samples=1):
        what = type(self).__name__
        self.spatial_size = _grid_shape(spatial_size, f"{what}: spatial_size")
        _, self.n_groups = _group_table(group_of, what)
        self.group_of = tuple(int(g) for g in group_of)
        try:
            w = np.array([float(v) for v in weights], dtype=np.float64)
        except (TypeError, ValueError):
            raise Mi3dError(f"{what}: weights takes one number per group, got {weights!r}") from None
        if w.shape != (self.n_groups,) or not np.isfinite(w).all() or w.min() < 0.0 or not w.sum() > 0.0:
            raise Mi3dError(f"{what}: {self.n_groups} non-negative finite weights with a positive sum expected, got {tuple(w)}")
        self.weights = w
        self._cum = np.cumsum(w) / w.sum()
        self._last = int(np.flatnonzero(w)[-1])          # rounding of the last cumulative value never reaches a zero-weight group
        self.num_samples = _integer(num_samples, what, "num_samples")
        if not 1 <= self.num_samples <= MAX_DRAWS:
            raise Mi3dError(f"{what}: num_samples {self.num_samples} is outside 1..{MAX_DRAWS}")
        self.last_batch = self.last_draw = self.last_pick = None
        self.set_random_state(None)

    def set_random_state(self, seed=None):
        self.R = np.random.RandomState(seed)
        return self

    def draw_one(self):
        """(group, word) of one window: draws 1 and 2 of the documented order."""
        group = min(int(np.searchsorted(self._cum, self.R.rand(), side="right")), self._last)
        return group, int(self.R.randint(0, 2 ** 64, dtype=np.uint64))

    def draw(self, n_volumes=1):
        """The three host arrays of pick_starts for num_samples windows in each of n_volumes volumes: (sample int32, group int32,
        rnd uint64), volume by volume."""
        n = _integer(n_volumes, type(self).__name__, "n_volumes")
        if not 1 <= n * self.num_samples <= MAX_DRAWS:
            raise Mi3dError(f"{type(self).__name__}: {n} volumes x {self.num_samples} samples is outside 1..{MAX_DRAWS} draws")
        pairs = [self.draw_one() for _ in range(n * self.num_samples)]
        return (np.repeat(np.arange(n, dtype=np.int32), self.num_samples), np.array([g for g, _ in pairs], dtype=np.int32),
                np.array([r for _, r in pairs], dtype=np.uint64))

    def _volumes(self, image, label, what):
        """(float32 image or None, int64 label, the map locations are picked from) of one sample, on the device."""
        if label is None:
            raise Mi3dError(f"{what}: a label is needed to place the window")
        x = _device_volume(image, torch.float32) if image is not None else None
        y = _device_volume(label, torch.int64)
        if x is not None and (x.shape != y.shape or x.device != y.device):
            raise Mi3dError(f"{what}: image {tuple(x.shape)} on {x.device}, label {tuple(y.shape)} on {y.device}")
        as_stored = isinstance(label, torch.Tensor) and label.is_cuda and label.dtype in _PICKABLE
        return x, y, (label if as_stored else y)[0]          # a uint8 map is counted as it is stored: an eighth of the bytes

    def __call__(self, sample):
        what = type(self).__name__
        x, y, pick_from = self._volumes(sample.get("image"), sample.get("label"), what)
        _window(self.spatial_size, y.shape[1:], what)
        _pick_view(pick_from, what)
        # everything is checked: draw, then count, pick and crop on the device
        starts, _, picked, _ = pick_starts(pick_from, *self.draw(1), self.spatial_size, self.group_of)
        image, label = crop_patches(x, y, starts, self.spatial_size)
        self.last_batch = (image, label, starts, picked)
        out = []
        for k in range(self.num_samples):
            d = dict(sample)
            if image is not None:
                d["image"] = image[k]
            d["label"] = label[k]
            out.append(d)
        return out

    def warp_at(self, image, label, out_shape=None, **warp_args):
        """warp(image, label, out_shape=..., start=the start of ONE freshly drawn location, **warp_args): what
        RandAffineElastic(crop=self) runs.  out_shape None: the sampler's spatial_size."""
        what = type(self).__name__
        size = self.spatial_size if out_shape is None else _grid_shape(out_shape, f"{what}: out_shape")
        x, y, pick_from = self._volumes(image, label, what)
        _window(size, y.shape[1:], what)
        _pick_view(pick_from, what)
        group, word = self.last_draw = self.draw_one()
        self.last_pick = pick_starts(pick_from, [0], [group], [word], size, self.group_of)
        return warp(x, y, out_shape=size, start=self.last_pick[0][0], **warp_args)


class RandCropByPosNegLabel(PatchSampler):
    """MONAI's RandCropByPosNegLabeld: windows centred on foreground (label > 0, group 1) with weight pos and on background
    (label == 0, group 0) with weight neg.  image_threshold is not supported; the stream of draws is not MONAI's (PatchSampler)."""

    def __init__(self, spatial_size, pos=1.0, neg=1.0, num_samples=1):
        super().__init__(spatial_size, [0] + [1] * 255, (neg, pos), num_samples)


class RandCropByLabelClasses(PatchSampler):
    """MONAI's RandCropByLabelClassesd: one group per class 0..num_classes-1 (at most 8), a window centred on class c with weight
    ratios[c]; ratios None: uniform.  Label values >= num_classes are in no group."""

    def __init__(self, spatial_size, ratios=None, num_classes=4, num_samples=1):
        n = _integer(num_classes, "RandCropByLabelClasses", "num_classes")
        if not 1 <= n <= MAX_GROUPS:
            raise Mi3dError(f"RandCropByLabelClasses: num_classes {n} is outside 1..{MAX_GROUPS}")
        super().__init__(spatial_size, list(range(n)) + [NO_GROUP] * (256 - n), (1.0,) * n if ratios is None else ratios, num_samples)
