"""Plain float64 numpy references for the small operators that run in every training step: flat AdamW, the Dropout3d mask
generator, the DANN head (Linear, row softmax-CE), MaxPool3d(2, 2) forward / backward and bf16 rounding.  The checker of
tests/test_gpu_step_ops.py: written from torch's documented semantics and from the generator documented in
include/mi3d.h / csrc/misc.hip, independent of the product module (it imports nothing of it), and pinned to torch on
the CPU by tests/test_step_ops_ref_cpu.py."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


# ---------------------------------------------------------------------------------------------------- bf16
def bf16_bits(x):
    """float32 -> the uint16 bit pattern of the nearest bfloat16, ties to even (finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(x):
    """The float32 value of x rounded once to bfloat16 (round to nearest even)."""
    return bf16_to_f32(bf16_bits(x)).reshape(np.shape(x))


def to_storage(x, dtype):
    """One rounding of a float64 result to the storage type: 'f32' or 'bf16' (through float32: exact for the dyadic sums of
    the tests, which is where it is used)."""
    y = np.asarray(x, dtype=np.float64).astype(np.float32)
    return bf16_round(y) if dtype == "bf16" else y


# ---------------------------------------------------------------------------------------------------- AdamW
def _hyper32(*h):
    return [float(np.float32(x)) for x in h]


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale=1.0, info=False):
    """torch's single-tensor AdamW (amsgrad off, maximize off), step number t >= 1, in float64:
         p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2
         denom = sqrt(v)/sqrt(1 - b2^t) + eps;  p -= lr/(1 - b1^t) * m/denom
    with g pre-multiplied by grad_scale.  The hyperparameters are rounded to float32 first (the ABI takes floats);
    everything else, the bias corrections included, is float64 (1 - b1**t in float32 cancels badly at small t).
    Returns (p', m', v'); info=True adds a dict with the pieces the error bounds need."""
    lr, b1, b2, eps, wd, gs = _hyper32(lr, b1, b2, eps, wd, grad_scale)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * gs
    p1 = p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** float(t)) + eps
    step_size = lr / (1.0 - b1 ** float(t))
    update = step_size * m1 / denom
    p2 = p1 - update
    if info:
        return p2, m1, v1, dict(g=g, m_terms=np.abs(b1 * m) + np.abs((1.0 - b1) * g), denom=denom, step_size=step_size,
                                update=update)
    return p2, m1, v1


def adamw_step_bounds(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale=1.0):
    """Per-element allowances for ONE float32 AdamW step from identical state against adamw_ref, u = 2^-24:

         |dm| <= 4u (|b1 m| + |(1-b1) g|)
         |dv| <= 4u v'
         |dp| <= 2u (|p| + |p'|) + 8u |update| + step_size * bound(m) / denom

    Derivation (every float32 operation is one rounding of relative size <= u; 1 - b1 and 1 - b2 are exact in float32 for
    b in [0.5, 1]):
      m' = b1*m + (1-b1)*(g*gs): the scaling of g, the two products and the sum are at most three roundings on the
         gradient term and two on the moment term, so 3u(|b1 m| + |(1-b1) g|) to first order; 4u leaves one u for a
         different contraction of the multiply-adds.
      v' = b2*v + (1-b2)*g^2 has only non-negative terms, so relative errors do not amplify: the rounding of g*gs enters
         twice, then two products and the sum, i.e. <= 5u on the gradient term and 2u on the moment term in the very
         worst case; the roundings are independent and at most u/2 on average, and 4u v' is what the whole has to stay in.
      p' = p(1 - lr wd) - update: the decay factor and its product with p are within 2u|p|, the final subtraction within
         u|p'| (the allowance takes 2u|p'| so that the stored float32 result itself is covered).  update = step_size *
         m'/denom carries the error of m' (third term, first order: step_size * bound(m)/denom) and relative errors from
         step_size (float32 bias correction and a division: 2u), sqrt(v') (half the 4u of v', plus the root's own u), the
         division by sqrt(1 - b2^t) (its rounding to float32 and the division: 2u), the addition of eps (u; eps > 0 only
         damps what came before), the division m'/denom and the product with step_size (2u).  The sum is <= 10u only if
         every rounding is at its maximum and of the same sign; 8u is the allowance, and a float32 numpy restatement of
         the same formula stays below 0.6 of each of the three bounds (asserted in tests/test_step_ops_ref_cpu.py).
    Returns (bound_p, bound_m, bound_v) as float64 arrays."""
    p2, m1, v1, d = adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale, info=True)
    bm = 4 * U * d["m_terms"]
    bv = 4 * U * v1
    bp = 2 * U * (np.abs(np.asarray(p, np.float64)) + np.abs(p2)) + 8 * U * np.abs(d["update"]) + d["step_size"] * bm / d["denom"]
    return bp, bm, bv


def adamw_f32(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale=1.0):
    """The same step in float32 numpy arithmetic with float64 bias corrections rounded to float32: what a float32
    implementation is expected to give up to contraction and root / division rounding.  Used to show on the CPU that the
    bounds above are attainable with margin, never as a reference."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    bc1 = f(1.0 - float(b1) ** float(t))
    bc2s = f(np.sqrt(1.0 - float(b2) ** float(t)))
    step_size = lr / bc1
    g = g * gs
    p = p * (f(1) - lr * wd)
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    denom = np.sqrt(v) / bc2s + eps
    p = p - step_size * (m / denom)
    return p, m, v


# ---------------------------------------------------------------------------------------------------- Dropout RNG
_M64 = (1 << 64) - 1


def _mix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dropout_uniforms_ref(seed, ctr, n):
    """u_i = (mix64(mix64(seed) ^ (ctr + i)) >> 40) * 2^-24 as float32 (exact: 24 bits), uint64 wrap-around arithmetic."""
    with np.errstate(over="ignore"):
        s = _mix64(np.array([int(seed) & _M64], dtype=np.uint64))
        r = _mix64(s ^ (np.uint64(int(ctr) & _M64) + np.arange(n, dtype=np.uint64)))
    return (r >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_scales_ref(seed, ctr, n, p):
    """Bit-exact restatement of the Dropout3d mask generator: r_i = mix64(mix64(seed) ^ (ctr + i)) (splitmix64 finaliser),
    u_i = (r_i >> 40) * 2^-24, keep iff u_i >= p, kept value float32(1)/(float32(1) - p) in float32 arithmetic (0 when
    p = 1).  Returns (float32[n], new counter = (ctr + n) mod 2^64)."""
    p32 = np.float32(p)
    u = dropout_uniforms_ref(seed, ctr, n)
    keep = np.float32(1) / (np.float32(1) - p32) if p32 < 1 else np.float32(0)
    return np.where(u >= p32, keep, np.float32(0)).astype(np.float32), (int(ctr) + int(n)) & _M64


# counters at which seed RNG_EDGE_SEED draws u == 0 and u == 0.5 exactly (found by search; asserted on the CPU): the only
# draws that tell `u >= p` from `u > p`, each of probability 2^-24
RNG_EDGE_SEED = 0x0123456789ABCDEF
RNG_EDGE_HITS = {0.0: 1872294, 0.5: 14617712}


# ---------------------------------------------------------------------------------------------------- DANN head
def linear_ref(x, w, b=None, relu=0, drop=None):
    """y = act(x w^T + b) * drop, float64.  x (M, K), w (Nout, K), b (Nout) or None, drop (M, Nout) or None."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    s = x @ w.T
    if b is not None:
        s = s + np.asarray(b, np.float64)[None, :]
    if relu:
        s = np.where(s > 0, s, 0.0)
    if drop is not None:
        s = s * np.asarray(drop, np.float64)
    return s


def linear_bwd_ref(x, w, y, gy, relu=0, drop=None, gx_scale=1.0, accumulate=0, gw0=None, gb0=None):
    """Backward of linear_ref given its OUTPUT y (the ReLU mask is y > 0: a pre-activation of exactly 0 passes no
    gradient).  gx = gx_scale * dL/dx (never accumulated); gw, gb are added to gw0, gb0 when accumulate.  float64."""
    x, w, y, gy = (np.asarray(a, np.float64) for a in (x, w, y, gy))
    gpre = gy.copy()
    if drop is not None:
        gpre = gpre * np.asarray(drop, np.float64)
    if relu:
        gpre = np.where(y > 0, gpre, 0.0)
    gx = float(np.float32(gx_scale)) * (gpre @ w)
    gw, gb = gpre.T @ x, gpre.sum(axis=0)
    if accumulate:
        gw, gb = gw + np.asarray(gw0, np.float64), gb + np.asarray(gb0, np.float64)
    return gx, gw, gb


def softmax_ce_rows_ref(logits, labels, scale=1.0):
    """nn.CrossEntropyLoss (mean) over the M rows of logits (M, C) and dlogits = scale * (softmax - onehot) / M; float64."""
    z = np.asarray(logits, np.float64)
    M = z.shape[0]
    zs = z - z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(zs).sum(axis=1))
    lab = np.asarray(labels, np.int64)
    loss = float((lse - zs[np.arange(M), lab]).mean())
    sm = np.exp(zs - lse[:, None])
    sm[np.arange(M), lab] -= 1.0
    return loss, float(np.float32(scale)) * sm / M


# ---------------------------------------------------------------------------------------------------- MaxPool3d(2, 2)
def _windows(z):
    """channels-last (N, D, H, W, C) -> (N, Do, Ho, Wo, C, 8), the last axis in (d, h, w) scan order; odd sizes floored."""
    N, D, H, W, C = z.shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    zz = z[:, :2 * Do, :2 * Ho, :2 * Wo].reshape(N, Do, 2, Ho, 2, Wo, 2, C)
    return zz.transpose(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, Do, Ho, Wo, C, 8)


def maxpool2_argmax(z):
    """Index 0..7 = 4a + 2b + c of the FIRST maximum of each window in (d, h, w) scan order (torch's choice)."""
    return np.argmax(_windows(np.asarray(z, np.float64)), axis=-1)


def maxpool2_fwd_ref(z, dtype="f32"):
    """MaxPool3d(kernel 2, stride 2) of channels-last z (N, D, H, W, C): (N, D//2, H//2, W//2, C)."""
    return to_storage(_windows(np.asarray(z, np.float64)).max(axis=-1), dtype)


def maxpool2_bwd_ref(z, dp, dskip=None, dtype="f32"):
    """dz (N, D, H, W, C): the pooled gradient dp goes to the first maximum of its window, the optional skip gradient is
    added everywhere (voxels outside every window receive only it, or zero); one rounding to the storage type."""
    z = np.asarray(z, np.float64)
    N, D, H, W, C = z.shape
    Do, Ho, Wo = D // 2, H // 2, W // 2
    arg = maxpool2_argmax(z)
    hot = (arg[..., None] == np.arange(8)) * np.asarray(dp, np.float64)[..., None]          # (N, Do, Ho, Wo, C, 8)
    hot = hot.reshape(N, Do, Ho, Wo, C, 2, 2, 2).transpose(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, 2 * Do, 2 * Ho, 2 * Wo, C)
    dz = np.zeros(z.shape, np.float64) if dskip is None else np.asarray(dskip, np.float64).copy()
    dz[:, :2 * Do, :2 * Ho, :2 * Wo] += hot
    return to_storage(dz, dtype)


POOL_LEVELS = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5], dtype=np.float32)          # bf16-exact, ascending


def pool_inputs(C, N, D, H, W, seed):
    """Tie-heavy MaxPool inputs (channels-last float32, every value bf16-exact).  Each window is built around a chosen
    first maximum: position k (uniform in 0..7; the first eight windows take each position once, so that even an
    eight-window case has them all) holds the maximum, a level of POOL_LEVELS above the lowest; the positions before k are
    strictly lower, the positions after k at most equal, and four windows in five with k < 7 repeat the maximum at a later
    position.  A tenth of the windows (past the first eight) are all-equal; a third have a negative maximum; zero is a
    level.  Voxels outside every window are random levels.  dp and dskip are multiples of 1/4 and 1/8 with |.| <= 4 and
    |.| <= 1, so dskip + dp is exact in bf16.  Returns (z, dp, dskip)."""
    rng = np.random.default_rng(seed)
    Do, Ho, Wo = D // 2, H // 2, W // 2
    nwin = N * Do * Ho * Wo * C
    k = rng.integers(0, 8, nwin)
    k[:8] = rng.permutation(8)
    mi = rng.integers(1, len(POOL_LEVELS), nwin)                    # level of the maximum: at least one level lies below
    r = rng.integers(0, 1 << 30, (nwin, 8))
    pos = np.arange(8)[None, :]
    lev = np.where(pos < k[:, None], r % mi[:, None], np.where(pos == k[:, None], mi[:, None], r % (mi[:, None] + 1)))
    tie = (rng.random(nwin) < 0.8) & (k < 7)
    later = k + 1 + rng.integers(0, 1 << 30, nwin) % np.maximum(7 - k, 1)
    rows = np.nonzero(tie)[0]
    lev[rows, later[rows]] = mi[rows]
    equal = (rng.random(nwin) < 0.1) & (np.arange(nwin) >= 8)
    lev[equal] = mi[equal][:, None]
    z = POOL_LEVELS[rng.integers(0, len(POOL_LEVELS), (N, D, H, W, C))]
    win = POOL_LEVELS[lev].reshape(N, Do, Ho, Wo, C, 2, 2, 2).transpose(0, 1, 5, 2, 6, 3, 7, 4)
    z[:, :2 * Do, :2 * Ho, :2 * Wo] = win.reshape(N, 2 * Do, 2 * Ho, 2 * Wo, C)
    dp = (rng.integers(-16, 17, (N, Do, Ho, Wo, C)) / 4.0).astype(np.float32)
    dskip = (rng.integers(-8, 9, (N, D, H, W, C)) / 8.0).astype(np.float32)
    return np.ascontiguousarray(z, dtype=np.float32), dp, dskip


def pool_tie_stats(z):
    """(fraction of windows whose maximum occurs more than once, the set of first-maximum positions that occur)."""
    w = _windows(np.asarray(z, np.float64))
    tied = (w == w.max(axis=-1, keepdims=True)).sum(axis=-1) > 1
    return float(tied.mean()), set(np.unique(np.argmax(w, axis=-1)).tolist())


# (C, N, D, H, W) of the MaxPool tests and the seed whose inputs meet the tie conditions (checked on the CPU)
POOL_CASES = [(8, 2, 4, 6, 4), (16, 1, 2, 2, 6), (32, 2, 4, 4, 8), (64, 1, 6, 4, 4), (128, 1, 4, 4, 4), (256, 1, 2, 4, 4),   # pair, G = 1..32
              (512, 1, 2, 2, 4), (24, 2, 4, 4, 4), (48, 1, 2, 6, 4),                                                       # one thread, VEC = 8
              (5, 2, 4, 6, 4), (3, 1, 5, 7, 9),                                                                            # VEC = 1
              (16, 1, 5, 7, 9), (32, 2, 3, 4, 5), (8, 1, 2, 3, 2)]                                                         # odd sizes
POOL_SEED = 7


def adamw_state(n, seed, gmag=1.0):
    """A generic mid-training optimizer state (float32): parameters ~ N(0, 1), gradients ~ gmag * N(0, 1), first moments of
    the gradients' size and either sign, second moments positive and of the size of g^2."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (gmag * rng.standard_normal(n)).astype(np.float32)
    m = (0.3 * gmag * rng.standard_normal(n)).astype(np.float32)
    v = (gmag * gmag * rng.uniform(0.01, 1.0, n)).astype(np.float32)
    return p, g, m, v


ADAMW_HYPERS = [(1e-3, 0.01, 1e-8), (1e-2, 0.1, 1e-8), (1e-3, 0.0, 1e-3)]          # (lr, weight decay, eps); betas 0.9, 0.999
ADAMW_STEPS = [1, 10, 1000, 100000]
ADAMW_GMAGS = [1e-6, 1e-3, 1.0, 1e3]
ADAMW_GRAD_SCALES = [1.0, 0.25, 1.0 / 3.0]
B1, B2 = 0.9, 0.999
