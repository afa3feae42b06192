"""Numpy float64 restatement of the two contracts of the boundary loss (include/mi3d.h: mi3d_signed_distance_maps,
mi3d_boundary_loss), the case lists of their tests and the allowances.  No scipy and no torch: the GPU tests import it.
tests/test_boundary_ref_cpu.py pins the maps to scipy.ndimage.distance_transform_edt, the term to float64 torch autograd, measures the
allowance constants with float32 torch and shows that the case lists catch the mutants below.

  signed_maps(labels, classes, spacing, inner_offset)      float32 (.., K, D, H, W); g3 is surface_ref.dist2, so it has one value
  term(logits, phi, channels, labels, ignore_index, ...)   (weight L, dlogits (N, C, V), float64)
  value_allowance / grad_allowance                         what a float32 evaluation of the term may be off by

The maps have no allowance: a = sqrt(g3(x, M)), b = sqrt(g3(x, ~M)) in double (numpy's sqrt is correctly rounded),
phi = (float32)a outside M, (float32)(0 - (b - inner_offset)) inside, 0 where the distance needed is +inf; bit for bit.

The term, float32 against this model (u = 2^-24).  With w_j = max z - z_j >= 0 and S = sum_i p_i (1 + w_i), a float32 softmax has
    e(p_j) = p_j (3 + w_j + S)            (loss_ref.sum_allowances: the rounded difference z_j - max moves the exponential's argument by
                                           u w_j; the exponential, the reciprocal and the product are one rounding each; se carries S)
    e(t)   = sum_k |phi_k| e(p_k) + K sum_k p_k |phi_k|                         t = sum_k p_k phi_k: K products, K - 1 adds
    e(g_j) = (|phi~_j| + T) (e(p_j) + 3 p_j) + p_j e(t),  T = sum_k p_k |phi_k|   g_j = s p_j (phi~_j - t): the difference, two products
in units of u, no cancellation credited.  Allowances:
    value      K_VALUE u |weight| sum_x e(t)(x) / (N K V)  (the kernel adds the float32 terms in double: nothing for the sum itself;
               float32 torch's own pairwise float32 sum is inside the measured constant)  + u |weight L| for the rounding of the result
    dlogits    K_GRAD u |s| e(g_j) + 2^-126 |s| max|phi|   per element (the floor: probabilities flushed to zero)
An ADD flag costs one more float32 addition, u (|what was there| + |what was added|), which the GPU test adds itself.
The divisor is N K V whether or not voxels are ignored; an ignored voxel has t = 0 and a zero gradient.

Measured (test_boundary_ref_cpu.py::test_allowance_constants, float32 torch on the CPU over TERM_CASES; never against the kernel):
    largest |float32 torch - model| / unit:   value 0.157   dlogits 0.786
    kept x 4:                                 K_VALUE = 0.63, K_GRAD = 3.15
"""
import functools

import numpy as np

import surface_ref as S

U = 2.0 ** -24
TINY = 2.0 ** -126
K_VALUE = 0.63          # 4 x 0.157 (module docstring)
K_GRAD = 3.15           # 4 x 0.786
# The model against float64 torch autograd: the same units at u = 2^-53.  The units credit every rounding of a voxel; torch's pairwise
# float64 sum of the mean adds at most log2(N K V) < 23 roundings of sum |p phi| <= (value unit) / 4, which the constant 8 covers.
U64 = 2.0 ** -53
K_F64 = 8.0
ADD_LOSS, ADD_GRAD = 1, 2
MAP_MUTANTS = ("minus_one", "sign_flipped")
TERM_MUTANTS = ("div_nv", "no_t")


# ---- the maps -------------------------------------------------------------------------------------------------------------------
def default_offset(spacing):
    return float(min(spacing))


def _signed3(lab, cls, spacing, off, mutant):
    m = lab == cls
    with np.errstate(invalid="ignore"):
        a, b = np.sqrt(S.dist2(m, spacing)), np.sqrt(S.dist2(~m, spacing))
        inner = 0.0 - (b - (1.0 if mutant == "minus_one" else off))
        if mutant == "sign_flipped":
            inner = b - off
        phi = np.where(m, inner, a)
    phi[~np.isfinite(np.where(m, b, a))] = 0.0
    return phi.astype(np.float32)


def signed_maps(labels, classes, spacing=(1.0, 1.0, 1.0), inner_offset=None, mutant=None):
    labels = np.asarray(labels)
    off = default_offset(spacing) if inner_offset is None else float(inner_offset)
    if labels.ndim == 3:
        return np.stack([_signed3(labels, c, spacing, off, mutant) for c in classes])
    return np.stack([np.stack([_signed3(lab, c, spacing, off, mutant) for c in classes]) for lab in labels])


def _blobs(shape, seed, dtype=np.uint8):
    """Classes 1..3 as boxes on background 0, with a little salt: every class has an inside, an outside and thin spurs."""
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, dtype=dtype)
    d, h, w = shape
    a[d // 4:d // 4 + max(d // 2, 1), 0:max(h // 2, 1), w // 8:w // 8 + max(w // 3, 1)] = 1
    a[0:max(d // 3, 1), h // 2:h, w // 2:w] = 2
    a[d // 2:d, h // 3:h, 0:max(w // 5, 1)] = 3
    salt = rng.random(shape) < 0.03
    a[salt] = rng.integers(0, 4, int(salt.sum())).astype(dtype)
    return a


def _single_voxel():
    a = np.zeros((9, 8, 7), dtype=np.uint8)
    a[4, 3, 2] = 2
    return a


def _absent_full():
    """Sample 0 is all class 1 (full: zero map; class 2 absent: zero map), sample 1 has both."""
    a = np.ones((2, 9, 8, 7), dtype=np.uint8)
    a[1] = _blobs((9, 8, 7), 5)
    return a


SPACINGS = ((1.0, 1.0, 1.0), (2.5, 0.75, 0.75))
# name -> (builder, classes)
MAP_LABELS = {
    "one": (lambda: np.full((1, 1, 1), 1, dtype=np.uint8), (1, 2)),                       # 1 x 1 x 1: class 1 full, class 2 absent
    "row70": (lambda: _blobs((5, 7, 70), 1), (1, 2, 3)),                                  # a row crossing a 64-lane word
    "box987": (lambda: _blobs((9, 8, 7), 2), (1, 2, 3)),
    "n2k1": (lambda: np.stack([_blobs((9, 8, 7), 3), _blobs((9, 8, 7), 4)]), (2,)),
    "n2k3": (lambda: np.stack([_blobs((5, 7, 70), 3), _blobs((5, 7, 70), 4)]), (3, 1, 0)),  # the background is a class like any other
    "int64": (lambda: _blobs((9, 8, 7), 6, np.int64) * 100, (100, 300, 7)),              # 300 does not fit a byte; 7 is absent
    "absent_full": (_absent_full, (1, 2)),
    "single_voxel": (_single_voxel, (2,)),
}
LAYOUT_LABELS = "row70"          # the case also run Fortran-ordered and permuted
# (labels, spacing, inner_offset): both spacings and the default offset everywhere, offset 0 and a literal 1 on two
MAP_CASES = [(name, sp, None) for name in MAP_LABELS for sp in SPACINGS] + [
    ("box987", SPACINGS[0], 0.0), ("row70", SPACINGS[1], 0.0), ("box987", SPACINGS[1], 1.0)]


@functools.lru_cache(maxsize=None)
def map_labels(name):
    a = MAP_LABELS[name][0]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def map_case(k):
    name, spacing, off = MAP_CASES[k]
    phi = signed_maps(map_labels(name), MAP_LABELS[name][1], spacing, off)
    phi.setflags(write=False)
    return phi


# ---- the term -------------------------------------------------------------------------------------------------------------------
def _softmax(z):
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    return e / e.sum(axis=1, keepdims=True), mx - z


def _counts(labels, ignore_index, shape):
    if labels is None:
        return np.ones(shape, dtype=bool)
    return np.asarray(labels) != ignore_index


def term(logits, phi, channels, labels=None, ignore_index=None, weight=1.0, grad_scale=1.0, mutant=None):
    """(weight L, dlogits) of mi3d_boundary_loss in float64: logits (N, C, V), phi (N, K, V), labels (N, V) or None."""
    z, f = np.asarray(logits, np.float64), np.asarray(phi, np.float64)
    N, C, V = z.shape
    K = len(channels)
    p, _ = _softmax(z)
    m = _counts(labels, ignore_index, (N, V))
    full = np.zeros_like(z)          # phi~
    full[:, list(channels)] = f
    t = (p * full).sum(axis=1)       # (N, V)
    div = float(N) * V if mutant == "div_nv" else float(N) * K * V
    value = float(weight) * float((t * m).sum()) / div
    inner = full if mutant == "no_t" else full - t[:, None]
    grad = float(grad_scale) * float(weight) * p * inner / div * m[:, None]
    return value, grad


def units(logits, phi, channels, labels=None, ignore_index=None):
    """(sum over the voxels that count of e(t), e(g) per element (N, C, V)) in units of u, before the scale: module docstring."""
    z, f = np.asarray(logits, np.float64), np.abs(np.asarray(phi, np.float64))
    N, C, V = z.shape
    K = len(channels)
    p, w = _softmax(z)
    m = _counts(labels, ignore_index, (N, V))
    s_all = (p * (1.0 + w)).sum(axis=1, keepdims=True)
    ep = p * (3.0 + w + s_all)
    full = np.zeros_like(z)
    full[:, list(channels)] = f
    T = (p * full).sum(axis=1, keepdims=True)
    et = (full * ep).sum(axis=1, keepdims=True) + K * T
    eg = (full + T) * (ep + 3.0 * p) + p * et
    return float((et[:, 0] * m).sum()), eg * m[:, None]


def value_allowance(logits, phi, channels, labels=None, ignore_index=None, weight=1.0, value=0.0, k=K_VALUE):
    N, C, V = np.asarray(logits).shape
    et, _ = units(logits, phi, channels, labels, ignore_index)
    return k * U * abs(weight) * et / (float(N) * len(channels) * V) + U * abs(value)


def grad_allowance(logits, phi, channels, labels=None, ignore_index=None, weight=1.0, grad_scale=1.0, k=K_GRAD):
    N, C, V = np.asarray(logits).shape
    s = abs(float(weight) * float(grad_scale)) / (float(N) * len(channels) * V)
    _, eg = units(logits, phi, channels, labels, ignore_index)
    return k * U * s * eg + TINY * s * float(np.abs(phi).max(initial=0.0))


def make_logits(family, N, C, V, seed):
    rng = np.random.default_rng(seed)
    if family == "gauss":
        z = rng.normal(0.0, 3.0, (N, C, V))
    elif family == "confident":          # one class far ahead: the others' probabilities are e^-10 and smaller
        z = rng.normal(0.0, 2.0, (N, C, V))
        z[np.arange(N)[:, None], rng.integers(0, C, (N, V)), np.arange(V)[None, :]] += 14.0
    elif family == "ties":               # multiples of 1/4: equal maxima and exact differences
        z = rng.integers(-8, 9, (N, C, V)) / 4.0
    else:
        raise KeyError(family)
    return z.astype(np.float32)


def make_phi(N, K, V, seed):
    """Signed values of a few voxels' scale with exact zeros among them (an absent class gives a zero map: the last one is one)."""
    rng = np.random.default_rng(seed + 1000)
    f = rng.normal(0.0, 6.0, (N, K, V)).astype(np.float32)
    f[rng.random((N, K, V)) < 0.05] = 0.0
    if K > 1:
        f[0, K - 1] = 0.0
    return f


def make_labels(mask, N, C, V, ignore_index, seed):
    """int64 (N, V) labels with `ignore_index` on the voxels of the mask family, or None for "none"."""
    if mask == "none":
        return None
    rng = np.random.default_rng(seed + 2000)
    lab = rng.integers(0, C, (N, V)).astype(np.int64)
    if mask == "random30":
        lab[rng.random((N, V)) < 0.3] = ignore_index
    elif mask == "runs":                 # whole runs of 4 and more: groups of four voxels that are all, partly and not ignored
        on = np.repeat(rng.random((N, (V + 6) // 7)) < 0.4, 7, axis=1)[:, :V]
        lab[on] = ignore_index
    elif mask == "all":
        lab[:] = ignore_index
    elif mask == "unused":               # labels given, nothing ignored
        pass
    else:
        raise KeyError(mask)
    return lab


V_BLOCKS = 4 * (256 * 3 + 37)          # 3220: four workgroups per sample on the 16-byte route, a ragged last one
V_STRIDE = 1200000                     # beyond 682 workgroups x 1024 voxels per sample at N = 3: the grid stride, ragged last pass
# (family, N, C, V, offset in elements, channels, mask family, ignore_index, weight, grad_scale, flags)
TERM_CASES = [
    ("gauss", 2, 4, 512, 0, (1, 2, 3), "none", None, 1.0, 1.0, 0),
    ("gauss", 2, 4, 315, 0, (1, 2, 3), "none", None, 1.0, 1.0, 0),                      # the scalar route
    ("gauss", 2, 4, 512, 1, (1, 2, 3), "none", None, 1.0, 1.0, 0),                      # pointers off by one element: scalar route
    ("gauss", 2, 2, 512, 0, (1,), "random30", 255, 0.25, 1.0, 0),
    ("confident", 2, 2, 315, 0, (0, 1), "runs", -100, 1.0, 0.5, ADD_GRAD),
    ("gauss", 2, 4, 512, 0, (0, 3), "runs", 255, 2.0, 0.5, ADD_GRAD | ADD_LOSS),        # channel 0 listed
    ("ties", 2, 4, 315, 0, (3, 1), "random30", 1, 1.0, 1.0, ADD_LOSS),                  # non-ascending; the ignore value is a class
    ("confident", 2, 5, 512, 0, (4, 0, 2), "none", None, 1.0, 1.0, 0),
    ("gauss", 2, 5, 315, 1, (1, 2, 3, 4), "random30", 255, 1.0, 0.5, ADD_GRAD),
    ("gauss", 2, 8, 512, 0, (7, 6, 5, 4, 3, 2, 1, 0), "runs", 255, 1.0, 1.0, 0),        # every channel, descending
    ("confident", 1, 8, 315, 0, (5,), "none", None, -1.5, 1.0, 0),
    ("gauss", 2, 4, 512, 0, (1, 2, 3), "all", 255, 1.0, 1.0, ADD_GRAD | ADD_LOSS),      # every voxel ignored: nothing moves
    ("gauss", 2, 4, 315, 0, (1, 2, 3), "all", 255, 1.0, 1.0, 0),                        # ... and zeros are stored
    ("gauss", 2, 3, 512, 0, (2, 1), "unused", 255, 1.0, 1.0, 0),                        # labels given, none ignored
    ("gauss", 2, 4, V_BLOCKS, 0, (1, 2, 3), "random30", 255, 1.0, 1.0, 0),              # several workgroups per sample
    ("gauss", 1, 3, 1, 0, (1,), "none", None, 1.0, 1.0, 0),                             # one voxel
    ("ties", 3, 2, V_STRIDE, 0, (1,), "runs", 255, 1.0, 1.0, ADD_GRAD),                 # the grid stride
    ("gauss", 2, 4, 512, 0, (1, 2, 3), "random30", 255, 0.0, 1.0, ADD_GRAD | ADD_LOSS),  # weight 0: the term is there and adds zeros
]
TERM_IDS = ["%02d-%s-%dx%dx%d+%d-ch%s-%s-w%g-gs%g-f%d" % (i, c[0], c[1], c[2], c[3], c[4], "".join(map(str, c[5])), c[6], c[8], c[9], c[10])
            for i, c in enumerate(TERM_CASES)]
CPU_MAX_V = 4096          # the CPU checks that need torch run the cases up to this size; the larger ones differ in size alone


@functools.lru_cache(maxsize=None)
def term_case(i):
    """(logits, phi, labels or None, value, grad) of TERM_CASES[i], computed once; the arrays are read-only."""
    family, N, C, V, off, ch, mask, ign, weight, gs, flags = TERM_CASES[i]
    z, f, lab = make_logits(family, N, C, V, 10 + i), make_phi(N, len(ch), V, 10 + i), make_labels(mask, N, C, V, ign, 10 + i)
    value, grad = term(z, f, ch, lab, ign, weight, gs)
    for a in (z, f, lab, grad):
        if a is not None:
            a.setflags(write=False)
    return z, f, lab, value, grad
