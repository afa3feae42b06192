"""Plain float64 numpy model of the affine + elastic warp (include/mi3d.h mi3d_elastic_field / mi3d_warp3, spatial.displacement_field /
spatial.warp): the checker of tests/test_gpu_warp.py, written from the contract, independent of the product module (it imports
nothing of it), and pinned to scipy.ndimage.correlate1d / map_coordinates by tests/test_warp_ref_cpu.py.

    noise    r = mix64a(mix64a(seed) ^ (a V + idx)), k = r >> 40, (k - 2^23) 2^-23 as float32: exact dyadics in [-1, 1)
    taps     g[x] = max(0, 0.5 (erf(t (x + 0.5)) - erf(t (x - 0.5)))), t = 0.70710678 / |sigma|, x = -R..R, R = int(max(3 sigma, 0.5) + 0.5)
    smooth   out[i] = sum_j g[j] src[i + j] along W, then H, then D; zeros beyond the volume; a float64 running sum in ascending j,
             each product and each sum rounded on its own; one rounding to float32 per pass
    coords   c = o - (no - 1)/2;  p = c + magnitude u[o];  s_a = ((M[a][0] p_0 + M[a][1] p_1) + M[a][2] p_2) + ((n_a - 1)/2 + t_a)
    outside  any s_a that is not 0 <= s_a <= n_a - 1 (a NaN is outside); then s is clamped to [0, n - 1]
    image    f = floor(s), t = s - f, upper tap min(f + 1, n - 1); lo (1 - t) + hi t along W, then H, then D; float32 of that
    label    the voxel floor(s + 0.5)
    padding  border: as above; zeros: 0 where outside

The running sum starts from 0.0 and a skipped tap adds nothing, which equals adding its 0.0 product: the model pads with zeros and
adds every tap.  numpy's elementwise a * b + c * d rounds each product and the sum, as the kernel does with contraction off, so the
GPU tests compare with array_equal.

CASES is the one list the CPU and the GPU tests share.  Every case has a non-symmetric matrix, a translation, a field smoothed with an
ASYMMETRIC table and an output grid that differs from the input grid, so that each mutant below changes every case's outputs: a
kernel that transposes the matrix, permutes the field's components, centres the output grid on the input's size or walks the tap
table backwards cannot pass the GPU tests.
"""
import collections
import functools
import math

import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24
K_IMAGE = 16.0          # |model - map_coordinates| <= K_IMAGE 2^-53 max|x| (derived in image_bound's docstring)
MASK = (1 << 64) - 1
MAX_RADIUS = 32


# ---------------------------------------------------------------------------------------------- noise
def mix64a(x):
    """splitmix64's output function on x + golden ratio, on uint64 arrays (numpy wraps modulo 2^64)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def noise_at(seed, counter):
    """float32 noise of the counters a * V + idx (any integer array)."""
    k = mix64a(mix64a(np.uint64(seed)) ^ np.asarray(counter, dtype=np.uint64)) >> np.uint64(40)
    return ((k.astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)


def noise(shape, seed):
    """(3, D, H, W) float32."""
    v = int(np.prod(shape))
    return noise_at(seed, np.arange(3 * v, dtype=np.uint64)).reshape((3,) + tuple(shape))


# ---------------------------------------------------------------------------------------------- taps and smoothing
def gaussian_taps(sigma):
    radius = int(max(float(sigma) * 3.0, 0.5) + 0.5)
    t = 0.70710678 / abs(float(sigma))
    return np.array([max(0.0, 0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5)))) for x in range(-radius, radius + 1)])


def skewed_taps(sigma):
    """An asymmetric table: the Gaussian one tilted by +-30 % across its width."""
    g = gaussian_taps(sigma)
    r = g.size // 2
    return g * (1.0 + 0.3 * np.arange(-r, r + 1) / max(r, 1))


def smooth_axis(src, g, axis):
    """float32 of sum_j g[j] src[i + j] along one axis of a float32 array, zeros beyond it, float64 running sum in ascending j."""
    r = g.size // 2
    x = np.moveaxis(np.asarray(src, dtype=np.float64), axis, -1)
    n = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (n + 2 * r,))
    pad[..., r:r + n] = x
    acc = np.zeros_like(x)
    for j in range(-r, r + 1):
        acc = acc + g[j + r] * pad[..., r + j:r + j + n]
    return np.ascontiguousarray(np.moveaxis(acc.astype(np.float32), -1, axis))


def smooth(u, g, reverse=False):
    """The three passes W, H, D over a (3, D, H, W) float32 array.  reverse: the mutant that walks the table backwards."""
    g = np.asarray(g, dtype=np.float64)[::-1] if reverse else np.asarray(g, dtype=np.float64)
    for axis in (3, 2, 1):
        u = smooth_axis(u, g, axis)
    return u


def field(shape, taps, seed, reverse=False):
    return smooth(noise(shape, seed), taps, reverse)


def smooth_bound(g):
    """Bound on |model - three float64 correlate1d calls| for noise in [-1, 1].  G = sum |g|: a value after pass k is at most G^k.
    The model rounds to float32 after every pass, a relative 2^-24 each: e1 <= 2^-24 G, e2 <= G e1 + 2^-24 G^2, e3 <= G e2 + 2^-24 G^3
    = 3 2^-24 G^3.  Both sides sum n = 2R + 1 float64 products per pass, at most (n + 1) 2^-53 relative each, carried through the
    later passes with a factor G per pass: 2 sides x 3 passes x (n + 1) 2^-53 G^3.  Second-order terms are below 2^-20 of that."""
    big_g = float(np.abs(g).sum())
    return (3.0 * U32 + 6.0 * (g.size + 1) * U64) * big_g ** 3


# ---------------------------------------------------------------------------------------------- coordinates and the gather
def coords(in_shape, out_shape, matrix, translate, u=None, magnitude=0.0, mutant=None):
    """s (3, Do, Ho, Wo) float64, before the outside test and the clamp."""
    m = np.asarray(matrix, dtype=np.float64)
    t = np.asarray(translate, dtype=np.float64)
    if mutant == "matrix transposed":
        m = m.T
    if mutant == "field permuted" and u is not None:
        u = u[[1, 2, 0]]
    centre_of = in_shape if mutant == "centre of input" else out_shape
    o = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in out_shape), indexing="ij")
    p = [o[a] - (centre_of[a] - 1) / 2.0 for a in range(3)]
    if u is not None:
        p = [p[a] + float(magnitude) * u[a].astype(np.float64) for a in range(3)]
    return np.stack([((m[a, 0] * p[0] + m[a, 1] * p[1]) + m[a, 2] * p[2]) + ((in_shape[a] - 1) / 2.0 + t[a]) for a in range(3)])


MUTANTS = ("matrix transposed", "field permuted", "centre of input")


def outside(s, in_shape):
    top = np.array(in_shape, dtype=np.float64).reshape(3, 1, 1, 1) - 1.0
    return (~((s >= 0.0) & (s <= top))).any(axis=0)          # not 0 <= s <= n - 1: a NaN is outside


def clamp(s, in_shape):
    top = np.array(in_shape, dtype=np.float64).reshape(3, 1, 1, 1) - 1.0
    return np.minimum(np.maximum(s, 0.0), top)


def image_values(x, s, padding):
    """float64 (C, Do, Ho, Wo) values of the image x (C, D, H, W) at s, before the rounding to float32."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1:]
    out = outside(s, n)
    sc = clamp(s, n)
    f = np.floor(sc)
    t = sc - f
    lo = f.astype(np.int64)
    hi = np.minimum(lo + 1, np.array(n).reshape(3, 1, 1, 1) - 1)

    def level_w(d, h):
        return x[:, d, h, lo[2]] * (1.0 - t[2]) + x[:, d, h, hi[2]] * t[2]

    def level_h(d):
        return level_w(d, lo[1]) * (1.0 - t[1]) + level_w(d, hi[1]) * t[1]

    v = level_h(lo[0]) * (1.0 - t[0]) + level_h(hi[0]) * t[0]
    return np.where(out[None], 0.0, v) if padding == "zeros" else v


def label_values(lab, s, padding):
    lab = np.asarray(lab)
    n = lab.shape[1:]
    out = outside(s, n)
    i = np.floor(clamp(s, n) + 0.5).astype(np.int64)
    v = lab[:, i[0], i[1], i[2]]
    return np.where(out[None], 0, v).astype(lab.dtype) if padding == "zeros" else v


def image_bound(x):
    """Bound on |image_values - map_coordinates(order=1)| at the same coordinates: u = 2^-53, P = max|x|.  Both sides evaluate the
    same convex combination of eight taps from the same float64 weights (1 - t and t); every partial result is at most P in magnitude.
    The model rounds one product and one sum per level, three levels: 6 u P to first order.  scipy multiplies each tap by its three
    weights (3 roundings) and adds the eight terms in turn (7 roundings): 10 u P.  Together K_IMAGE = 16, the soft restore's figure."""
    return K_IMAGE * U64 * float(np.abs(x).max())


# ---------------------------------------------------------------------------------------------- host restatements
def affine_matrix(rotate, scale):
    """R_d @ R_h @ R_w @ diag(scale), the product module's documented convention, restated."""
    (cd, sd), (ch, sh), (cw, sw) = ((math.cos(a), math.sin(a)) for a in rotate)
    r_d = np.array([[1, 0, 0], [0, cd, -sd], [0, sd, cd]], dtype=np.float64)
    r_h = np.array([[ch, 0, sh], [0, 1, 0], [-sh, 0, ch]], dtype=np.float64)
    r_w = np.array([[cw, -sw, 0], [sw, cw, 0], [0, 0, 1]], dtype=np.float64)
    return r_d @ r_h @ r_w @ np.diag(np.asarray(scale, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- cases
# The field table of the issue: (shape, sigma).  R = 2, 6, 9, 3, 3, 32.
FIELD_CASES = (((5, 7, 9), 0.6), ((12, 10, 70), 2.0), ((4, 4, 4), 3.0), ((3, 1, 130), 1.0), ((2, 3, 1), 1.0), ((6, 6, 40), 10.5))
# the same route with an asymmetric table: a kernel that walks the table backwards fails these
SKEWED_FIELD_CASES = (((5, 7, 9), 0.6), ((3, 5, 70), 2.0))

Case = collections.namedtuple("Case", "name channels in_shape out_shape rotate scale translate sigma magnitude seed")

CASES = (
    Case("c1-w7", 1, (6, 7, 9), (5, 6, 7), (0.3, -0.2, 0.25), (1.1, 0.9, 1.05), (0.3, -0.4, 0.2), 0.6, 1.5, 11),
    Case("c3-w8", 3, (5, 6, 7), (6, 5, 8), (-0.2, 0.3, 0.15), (0.9, 1.1, 0.95), (-0.25, 0.5, 0.1), 0.8, 2.0, 12),
    Case("c1-w66", 1, (4, 5, 40), (3, 4, 66), (0.1, 0.05, -0.2), (1.05, 0.95, 0.7), (0.2, 0.1, -0.7), 1.0, 3.0, 13),
    Case("c3-w1", 3, (5, 6, 4), (6, 7, 1), (0.4, 0.2, -0.3), (0.8, 0.9, 1.0), (0.1, 0.2, 0.3), 0.6, 1.0, 14),
    Case("d1-w12", 1, (6, 7, 8), (1, 5, 12), (0.2, -0.3, 0.1), (1.0, 1.2, 0.8), (0.6, -0.1, 0.2), 0.7, 1.5, 15),
    Case("far", 1, (6, 7, 9), (7, 8, 8), (0.2, 0.1, -0.1), (1.1, 1.0, 0.9), (0.1, -0.2, 0.3), 0.6, 30.0, 16),
    Case("up", 3, (4, 5, 6), (7, 8, 12), (-0.1, 0.2, 0.3), (1.0, 0.9, 1.1), (0.0, 0.3, -0.2), 0.9, 1.0, 17),
    Case("in-w66", 1, (3, 4, 66), (4, 3, 7), (0.05, -0.1, 0.2), (0.9, 1.1, 4.0), (0.2, -0.3, 1.5), 0.6, 2.5, 18),
)
PADDINGS = ("border", "zeros")


def case(name):
    return next(c for c in CASES if c.name == name)


def inputs_of(c):
    """(float32 image, int64 label) of a case, (C, D, H, W), from a generator seeded by the case."""
    rng = np.random.default_rng([c.seed, c.channels, *c.in_shape])
    shape = (c.channels,) + tuple(c.in_shape)
    return rng.standard_normal(shape).astype(np.float32), rng.integers(0, 16, shape, dtype=np.int64)


Model = collections.namedtuple("Model", "image label matrix translate field coords values image_out label_out")


@functools.lru_cache(maxsize=None)
def model(c, mutant=None):
    """The case's inputs and the model's results, computed once and shared (callers must not write into them).  values / image_out /
    label_out are dicts over PADDINGS."""
    x, lab = inputs_of(c)
    m, t = affine_matrix(c.rotate, c.scale), np.array(c.translate, dtype=np.float64)
    u = field(c.out_shape, skewed_taps(c.sigma), c.seed)
    s = coords(c.in_shape, c.out_shape, m, t, u, c.magnitude, mutant)
    values = {p: image_values(x, s, p) for p in PADDINGS}
    image_out = {p: v.astype(np.float32) for p, v in values.items()}
    label_out = {p: label_values(lab, s, p) for p in PADDINGS}
    for a in (x, lab, m, t, u, s, *values.values(), *image_out.values(), *label_out.values()):
        a.setflags(write=False)
    return Model(x, lab, m, t, u, s, values, image_out, label_out)


def warp(image, label, matrix=None, translate=None, u=None, magnitude=0.0, out_shape=None, image_padding="border",
         label_padding="zeros"):
    """The model as one call on arbitrary inputs: (float32 image or None, label or None)."""
    first = image if image is not None else label
    in_shape = first.shape[1:]
    out_shape = in_shape if out_shape is None else tuple(out_shape)
    s = coords(in_shape, out_shape, np.eye(3) if matrix is None else matrix, np.zeros(3) if translate is None else translate, u, magnitude)
    return (image_values(image, s, image_padding).astype(np.float32) if image is not None else None,
            label_values(label, s, label_padding) if label is not None else None)
