"""Numpy float64 restatement of the contract of the entropy term (include/mi3d.h: mi3d_entropy_loss), the case list of its tests and
the allowances.  No scipy and no torch: the GPU tests import it.  tests/test_entropy_ref_cpu.py pins the model to float64 torch
autograd of -sum softmax * log_softmax / (N V ln C), measures the allowance constants with a float32 numpy restatement of the kernel's
formula (term32 below) and shows that the case list catches the mutants below.

  term(logits, labels, ignore_index, mode, ...)            (weight L, dlogits (N, C, V), float64)
  term32(...)                                              the same chain in float32, operation by operation as the kernel writes it
  value_allowance / grad_allowance                         what a float32 evaluation of the term may be off by

Per voxel: d_j = z_j - max z, e_j = exp(d_j), se = sum e_j, p_j = e_j / se, H = log(se) - sum_j p_j d_j, q_j = log(se) - d_j - H;
L = sum_selected H / (N V ln C), dlogits[j] = s p_j q_j with s = grad_scale weight / (N V ln C).

float32 against this model (u = 2^-24), in units of u, no cancellation credited.  With w_j = -d_j >= 0, S = sum_i p_i (1 + w_i),
W = sum_j p_j w_j and lse = log(se), so that H = lse + W:
    e(p_j) = p_j (3 + w_j + S)                  (boundary_ref.units: the rounded difference z_j - max moves the exponential's argument by
                                                 u w_j; expf, the reciprocal and the product are one rounding each; se carries S)
    e(lse) = S + 2 lse                          se carries S relative, which is log's absolute error; logf itself up to 2 roundings
    e(pd)  = sum_j w_j e(p_j) + (C + 1) W       pd = sum_j p_j d_j: C products of a rounded d_j, C - 1 adds
    e(H)   = e(lse) + e(pd) + H                 the difference, one rounding
    e(g_j) = |q_j| (e(p_j) + 3 p_j) + p_j (e(lse) + w_j + (lse + w_j) + e(H) + |q_j|)
                                                a = lse - d_j (d_j's rounding, one rounding), q = a - H (one rounding), then the
                                                products with p_j and with the rounded scale s
Allowances:
    value      K_VALUE u |weight| sum_selected e(H) / (N V ln C)   (the kernel adds the float32 H in double: nothing for the sum itself)
               + u |weight L| for the rounding of the result + the floor below per selected voxel
    dlogits    K_GRAD u |s| e(g_j) + 2^-126 |s| 128               per element (the floor: probabilities flushed to zero)
An ADD flag costs one more float32 addition, u (|what was there| + |what was added|), which the GPU test adds itself.
The divisor is N V ln C whatever is selected; an unselected voxel adds nothing and has a zero gradient.
The saturated family (one class 128 above the rest) is not a matter of allowances: expf(-128) is 0 in float32, so se = 1, lse = 0, every
product is 0 and the GPU tests assert a literal 0.0 for the value and every gradient element.

Measured (test_entropy_ref_cpu.py::test_allowance_constants, term32 on the CPU over CASES; never against the kernel):
    largest |term32 - model| / unit:   value 0.290   dlogits 0.693
    kept x 4:                          K_VALUE = 1.16, K_GRAD = 2.78
(the headroom boundary_ref's K_VALUE / K_GRAD have over their measured ratios: x 4, rounded up by less than 10 %).
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
K_VALUE = 1.16          # 4 x 0.290 (module docstring)
K_GRAD = 2.78           # 4 x 0.693
ALL, COUNTED, IGNORED = 0, 1, 2
ADD_LOSS, ADD_GRAD = 1, 2
MUTANTS = ("no_lnc", "div_selected", "no_h", "swapped")


def select(labels, ignore_index, mode, shape):
    """bool (N, V): the voxels `mode` selects."""
    if mode == ALL:
        return np.ones(shape, dtype=bool)
    hit = np.asarray(labels) == ignore_index
    return hit if mode == IGNORED else ~hit


def _chain(z):
    mx = z.max(axis=1, keepdims=True)
    d = z - mx
    e = np.exp(d)
    se = e.sum(axis=1, keepdims=True)
    return d, e / se, np.log(se)


def term(logits, labels=None, ignore_index=None, mode=ALL, weight=1.0, grad_scale=1.0, mutant=None):
    """(weight L, dlogits) of mi3d_entropy_loss in float64: logits (N, C, V), labels (N, V) or None."""
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    if mutant == "swapped" and mode != ALL:
        mode = COUNTED if mode == IGNORED else IGNORED
    m = select(labels, ignore_index, mode, (N, V))
    d, p, lse = _chain(z)
    h = lse[:, 0] - (p * d).sum(axis=1)          # (N, V)
    div = float(N) * V * math.log(C)
    if mutant == "no_lnc":
        div = float(N) * V
    elif mutant == "div_selected":
        div = max(int(m.sum()), 1) * math.log(C)
    value = float(weight) * float((h * m).sum()) / div
    q = lse - d if mutant == "no_h" else lse - d - h[:, None]
    grad = float(grad_scale) * float(weight) * p * q / div * m[:, None]
    return value, grad


def term32(logits, labels=None, ignore_index=None, mode=ALL, weight=1.0, grad_scale=1.0):
    """The kernel's chain restated in float32 numpy, one rounding per operation in the kernel's order (sums over the classes in
    ascending order); the H of the selected voxels are added in double, the result is rounded once."""
    f = np.float32
    z = np.asarray(logits, f)
    N, C, V = z.shape
    m = select(labels, ignore_index, mode, (N, V))
    mx = z.max(axis=1)
    d = [z[:, j] - mx for j in range(C)]
    e = [np.exp(dj) for dj in d]
    se = e[0].copy()
    for j in range(1, C):
        se = se + e[j]
    inv, lse = f(1.0) / se, np.log(se)
    p = [ej * inv for ej in e]
    pd = np.zeros_like(se)
    for j in range(C):
        pd = pd + p[j] * d[j]
    h = lse - pd
    assert all(a.dtype == f for a in (se, inv, lse, pd, h))
    w_over = float(weight) / (float(N) * V * math.log(C))
    value = float(f(float(h.astype(np.float64)[m].sum()) * w_over))
    s = f(grad_scale) * f(w_over)
    grad = np.stack([s * p[j] * (lse - d[j] - h) for j in range(C)], axis=1)
    assert grad.dtype == f
    return value, grad * m[:, None]


def units(logits, labels=None, ignore_index=None, mode=ALL):
    """(sum over the selected voxels of e(H), the number of selected voxels, e(g) per element (N, C, V)) in units of u."""
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    m = select(labels, ignore_index, mode, (N, V))
    d, p, lse = _chain(z)
    w = -d
    S = (p * (1.0 + w)).sum(axis=1, keepdims=True)
    W = (p * w).sum(axis=1, keepdims=True)
    ep = p * (3.0 + w + S)
    else_ = S + 2.0 * lse
    epd = (w * ep).sum(axis=1, keepdims=True) + (C + 1.0) * W
    h = lse + W
    eh = else_ + epd + h
    q = np.abs(lse + w - h)
    eg = q * (ep + 3.0 * p) + p * (else_ + w + (lse + w) + eh + q)
    return float((eh[:, 0] * m).sum()), int(m.sum()), eg * m[:, None]


def value_allowance(logits, labels=None, ignore_index=None, mode=ALL, weight=1.0, value=0.0, k=K_VALUE):
    N, C, V = np.asarray(logits).shape
    eh, count, _ = units(logits, labels, ignore_index, mode)
    div = float(N) * V * math.log(C)
    return k * U * abs(weight) * eh / div + U * abs(value) + TINY * 128.0 * C * count * abs(weight) / div


def grad_allowance(logits, labels=None, ignore_index=None, mode=ALL, weight=1.0, grad_scale=1.0, k=K_GRAD):
    N, C, V = np.asarray(logits).shape
    s = abs(float(weight) * float(grad_scale)) / (float(N) * V * math.log(C))
    _, _, eg = units(logits, labels, ignore_index, mode)
    return k * U * s * eg + TINY * s * 128.0


FAMILIES = ("gauss", "confident", "ties", "offset", "saturated", "uniform")


def make_logits(family, N, C, V, seed):
    rng = np.random.default_rng(seed)
    hot = (np.arange(N)[:, None], rng.integers(0, C, (N, V)), np.arange(V)[None, :])
    if family == "gauss":
        z = rng.normal(0.0, 3.0, (N, C, V))
    elif family == "confident":          # one class far ahead: the others' probabilities are e^-10 and smaller
        z = rng.normal(0.0, 2.0, (N, C, V))
        z[hot] += 14.0
    elif family == "ties":               # multiples of 1/4: equal maxima and exact differences
        z = rng.integers(-8, 9, (N, C, V)) / 4.0
    elif family == "offset":             # +1e4 on every logit: only the max subtraction keeps the exponentials finite
        z = rng.normal(0.0, 3.0, (N, C, V)) + 1e4
    elif family == "saturated":          # one class 128 above the rest, which are equal: expf underflows to 0, H = 0 exactly
        z = np.broadcast_to(rng.integers(-4, 5, (N, 1, V)).astype(np.float64), (N, C, V)).copy()
        z[hot] += 128.0
    elif family == "uniform":            # all logits of a voxel equal: H = ln C, the gradient is 0
        z = np.broadcast_to(rng.normal(0.0, 3.0, (N, 1, V)), (N, C, V)).copy()
    else:
        raise KeyError(family)
    return z.astype(np.float32)


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
# (family, N, C, V, offset in elements, mode, mask family, ignore_index, weight, grad_scale, flags)
CASES = [
    ("gauss", 2, 4, 512, 0, ALL, "none", None, 1.0, 1.0, 0),
    ("gauss", 2, 4, 70, 0, ALL, "none", None, 1.0, 1.0, 0),                             # V % 4 != 0: the scalar route
    ("gauss", 1, 3, 1, 0, ALL, "none", None, 1.0, 1.0, 0),                              # one voxel
    ("gauss", 2, 4, V_BLOCKS, 0, IGNORED, "random30", 255, 1.0, 1.0, 0),                # several workgroups per sample
    ("gauss", 2, 4, V_BLOCKS + 1, 0, COUNTED, "random30", 255, 1.0, 1.0, ADD_GRAD),     # 3221: the scalar route, several workgroups
    ("gauss", 2, 4, 512, 1, ALL, "none", None, 1.0, 1.0, 0),                            # pointers off by one element: scalar route
    ("gauss", 2, 4, V_BLOCKS + 1, 1, IGNORED, "runs", 255, 1.0, 0.5, ADD_GRAD),         # both
    ("confident", 2, 2, 512, 0, IGNORED, "random30", 255, 0.25, 1.0, 0),
    ("confident", 2, 8, 70, 0, COUNTED, "runs", -100, 1.0, 0.5, ADD_GRAD),
    ("ties", 3, 3, 512, 0, IGNORED, "runs", 1, 1.0, 1.0, ADD_LOSS),                     # the ignore value is a class
    ("ties", 2, 4, 70, 0, COUNTED, "random30", 1, 2.0, 0.5, ADD_GRAD | ADD_LOSS),
    ("offset", 2, 4, 512, 0, ALL, "none", None, 1.0, 1.0, 0),
    ("offset", 1, 8, 70, 0, IGNORED, "random30", 255, -1.5, 1.0, ADD_LOSS),             # a negative weight
    ("saturated", 2, 4, 512, 0, ALL, "none", None, 1.0, 1.0, 0),                        # exactly 0.0 everywhere
    ("saturated", 2, 3, 70, 0, COUNTED, "random30", 255, 1.0, 1.0, 0),
    ("uniform", 2, 4, 512, 0, ALL, "none", None, 1.0, 1.0, 0),                          # H / ln C = 1, gradient 0
    ("uniform", 3, 2, 70, 0, IGNORED, "runs", 255, 1.0, 0.5, 0),
    ("gauss", 2, 4, 512, 0, ALL, "unused", 255, 1.0, 1.0, 0),                           # mode ALL with labels given: not read
    ("gauss", 2, 4, 512, 0, ALL, "random30", 255, 1.0, 1.0, ADD_GRAD),                  # ... even where they say ignore
    ("gauss", 2, 4, 512, 0, ALL, "runs", 255, 1.0, 1.0, ADD_LOSS),
    ("gauss", 2, 4, 512, 0, ALL, "all", 255, 1.0, 1.0, 0),
    ("gauss", 2, 3, 512, 0, COUNTED, "unused", 255, 1.0, 1.0, 0),                       # nothing ignored: COUNTED is everything
    ("gauss", 2, 3, 512, 0, IGNORED, "unused", 255, 1.0, 1.0, ADD_GRAD | ADD_LOSS),     # ... and IGNORED nothing: nothing moves
    ("gauss", 2, 4, 512, 0, IGNORED, "all", 255, 1.0, 1.0, ADD_GRAD),                   # everything ignored: IGNORED is everything
    ("gauss", 2, 4, 70, 0, COUNTED, "all", 255, 1.0, 1.0, 0),                           # ... and COUNTED nothing: zeros are stored
    ("gauss", 2, 4, 512, 0, COUNTED, "all", 255, 1.0, 1.0, ADD_GRAD | ADD_LOSS),
    ("gauss", 2, 5, 512, 0, COUNTED, "runs", 255, 1.0, 1.0, ADD_LOSS),
    ("gauss", 2, 8, 512, 0, IGNORED, "runs", 255, 1.0, 1.0, ADD_GRAD | ADD_LOSS),
    ("gauss", 2, 2, 512, 0, COUNTED, "random30", 255, -0.5, 0.5, 0),
    ("ties", 3, 2, V_STRIDE, 0, IGNORED, "runs", 255, 1.0, 1.0, ADD_GRAD),              # the grid stride, once
    ("gauss", 2, 4, 512, 0, IGNORED, "random30", 255, 0.0, 1.0, ADD_GRAD | ADD_LOSS),   # weight 0: the term is there and adds zeros
]
MODE_NAMES = ("all", "counted", "ignored")
IDS = ["%02d-%s-%dx%dx%d+%d-%s-%s-w%g-gs%g-f%d" % (i, c[0], c[1], c[2], c[3], c[4], MODE_NAMES[c[5]], c[6], c[8], c[9], c[10])
       for i, c in enumerate(CASES)]
CPU_MAX_V = 4096          # the CPU checks that need torch run the cases up to this size; the larger one differs in size alone


@functools.lru_cache(maxsize=None)
def case(i):
    """(logits, labels or None, value, grad) of CASES[i], computed once; the arrays are read-only."""
    family, N, C, V, off, mode, mask, ign, weight, gs, flags = CASES[i]
    z, lab = make_logits(family, N, C, V, 10 + i), make_labels(mask, N, C, V, ign, 10 + i)
    value, grad = term(z, lab, ign, mode, weight, gs)
    for a in (z, lab, grad):
        if a is not None:
            a.setflags(write=False)
    return z, lab, value, grad
