"""float64 numpy restatement of the reference's spatial helpers (utils/dataloader.py:207-221): np.flip over axes 1, 2, 3 and
scipy.ndimage.rotate(x, angle, axes=plane, reshape=False, mode='nearest'), order=1 for the image and order=0 for the label, on
(C, D, H, W) arrays.  The checker of the spatial tests: written from scipy's documented behaviour, independent of the product
module, pinned to scipy and to the reference's own functions by tests/golden/spatial*.npz (tests/test_spatial_cpu.py) and,
where scipy imports, against scipy directly.

Arithmetic per output voxel with plane indices (o0, o1), every operation a separate IEEE double operation (numpy fuses none):
    cc_i = (o0*M[i][0] + o1*M[i][1]) + off[i]       products, their sum, THEN the offset; clamped to [0, n_i - 1]
    label  x[floor(cc_0 + 0.5), floor(cc_1 + 0.5)]
    image  f = floor(cc), t = cc - f, upper tap min(f + 1, n - 1); weights (1-t0)(1-t1), (1-t0)t1, t0(1-t1), t0 t1;
           weight * value summed in the order (f0,f1), (f0,f1+1), (f0+1,f1), (f0+1,f1+1); one rounding to float32

The allowance for an image voxel (derived, not measured): np.spacing(float32(|want|)) + 2^-50 * max|input|.  scipy multiplies
value * w0 * w1 where this file multiplies value * (w0 * w1), and a device may add the four terms in another order: each such
double sum is within 4 * 2^-53 * max|input| of the exact one, well inside the second term; two correctly rounded float32
casts of doubles that close differ by at most one float32 spacing, the first term."""
import math

import numpy as np

PLANES = [(1, 2), (1, 3), (2, 3)]
ANGLES = [0.0, 15.0, -15.0, 7.3, 45.0, 90.0, 1e-3]
SHAPES = [(1, 7, 9, 12), (1, 16, 16, 16), (2, 5, 8, 8), (1, 12, 10, 7)]
INPUTS = ["plain", "wide", "cancel"]          # tests/golden/spatial_rotate_<input>.npz


def case_key(shape, plane, angle_index):
    return "s" + "x".join(str(n) for n in shape) + f"/p{plane[0]}{plane[1]}/a{angle_index}"


def rotation(plane_shape, angle):
    """(matrix, offset) as scipy.ndimage.rotate builds them; scipy.special's cosdg / sindg where it imports."""
    try:
        from scipy.special import cosdg, sindg
        c, s = float(cosdg(angle)), float(sindg(angle))
    except ImportError:
        c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    m = np.array([[c, s], [-s, c]])
    centre = (np.asarray(plane_shape, dtype=np.float64) - 1) / 2
    return m, centre - m @ centre


def coords(n0, n1, matrix, offset):
    """Clamped source coordinates (cc0, cc1), each (n0, n1) float64."""
    o0 = np.arange(n0, dtype=np.float64)[:, None]
    o1 = np.arange(n1, dtype=np.float64)[None, :]
    m, off = np.asarray(matrix, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    cc0 = (o0 * m[0, 0] + o1 * m[0, 1]) + off[0]
    cc1 = (o0 * m[1, 0] + o1 * m[1, 1]) + off[1]
    return np.clip(cc0, 0.0, n0 - 1.0), np.clip(cc1, 0.0, n1 - 1.0)


def _to_front(x, plane):
    """View with the two plane axes first: (n0, n1, rest...)."""
    return np.moveaxis(x, plane, (0, 1))


def flip(x, flips):
    for axis, f in zip((1, 2, 3), flips):
        if f:
            x = np.flip(x, axis=axis)
    return x


def affine_label(label, plane, matrix, offset, flips=(False, False, False)):
    x = _to_front(flip(np.asarray(label), flips), plane)
    cc0, cc1 = coords(x.shape[0], x.shape[1], matrix, offset)
    i0, i1 = np.floor(cc0 + 0.5).astype(np.int64), np.floor(cc1 + 0.5).astype(np.int64)
    return np.ascontiguousarray(np.moveaxis(x[i0, i1], (0, 1), plane))


def affine_image64(image, plane, matrix, offset, flips=(False, False, False)):
    """The float64 sum before the one rounding."""
    x = _to_front(flip(np.asarray(image), flips), plane).astype(np.float64)
    n0, n1 = x.shape[:2]
    cc0, cc1 = coords(n0, n1, matrix, offset)
    f0, f1 = np.floor(cc0), np.floor(cc1)
    t0, t1 = cc0 - f0, cc1 - f1
    lo0, lo1 = f0.astype(np.int64), f1.astype(np.int64)
    hi0, hi1 = np.minimum(lo0 + 1, n0 - 1), np.minimum(lo1 + 1, n1 - 1)
    ex = (...,) + (None,) * (x.ndim - 2)
    a0, a1 = 1.0 - t0, 1.0 - t1
    s = (a0 * a1)[ex] * x[lo0, lo1]
    s = s + (a0 * t1)[ex] * x[lo0, hi1]
    s = s + (t0 * a1)[ex] * x[hi0, lo1]
    s = s + (t0 * t1)[ex] * x[hi0, hi1]
    return np.ascontiguousarray(np.moveaxis(s, (0, 1), plane))


def affine_image(image, plane, matrix, offset, flips=(False, False, False)):
    return affine_image64(image, plane, matrix, offset, flips).astype(np.float32)


def rotate(image, label, angle, plane, flips=(False, False, False)):
    """rotate(flip(image)), rotate(flip(label)); either may be None."""
    ref = image if image is not None else label
    m, off = rotation((ref.shape[plane[0]], ref.shape[plane[1]]), angle)
    return (affine_image(image, plane, m, off, flips) if image is not None else None,
            affine_label(label, plane, m, off, flips) if label is not None else None)


def allowance(want, x_in):
    """Per-voxel bound on |got - want| for float32 images (module docstring)."""
    want = np.asarray(want, dtype=np.float32)
    return np.spacing(np.abs(want)).astype(np.float64) + 2.0 ** -50 * float(np.abs(x_in).max())


def assert_image_close(got, want, x_in, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = allowance(want, x_in)
    worst = float((err / tol).max())
    print(f"{what}: max |delta| / allowance {worst:.3f}, voxels not bit-equal {int((got != want).sum())} of {got.size}")
    assert worst <= 1.0, what
