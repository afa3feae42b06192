"""Plain float64 numpy references for the loss family and the metrics of csrc/head_loss.hip, the input families the tests
run them on, and the allowances a float32 implementation is held to.  The checker of tests/test_gpu_loss_ops.py: written
from the formulas of the reference's utils/metrics.py (combined_loss, tversky_loss, combined_ce_tversky_loss,
distillation_loss, the 'dice' variant, calculate_iou / calculate_dice / calculate_accuracy) and from the comments of
include/mi3d.h, independent of the product module (it imports nothing of it), and pinned to float64 torch autograd, to the
reference-run fixtures and to central differences by tests/test_loss_ref_cpu.py.

    L = w_ce * CE_mean + w_reg * mean_{c>=1} R_c + w_kd * T^2 * mean_{n,c,v} KL(p_t^T || p_s^T)
    R_c = 1 - (2 I_c + eps) / (P_c + T_c + eps)                          soft Dice       (region_kind 1)
    R_c = 1 - (I_c + eps) / (I_c + a (P_c - I_c) + b (T_c - I_c) + eps)  Tversky(a, b)   (region_kind 2)
    I_c = sum p_c [t = c],  P_c = sum p_c,  T_c = sum [t = c]     over all N * V voxels

The 20 `coef` floats the backward runs on: A[0..8), B[8..16), ce_s, kd_s, loss, 0 with
    A_c = w_reg/(C-1) * dR_c/dI_c,  B_c = w_reg/(C-1) * dR_c/dP_c  (c >= 1, else 0),  ce_s = w_ce/M,  kd_s = w_kd*T/(M*C)
    dL/dz_k = go * ( ce_s (p_k - [t=k]) + p_k (g_k - sum_j g_j p_j) + kd_s (ps_k - pt_k) ),   g_c = A_c [t=c] + B_c

The constants K of the allowances are 4 x the largest ratio |float32 torch - float64| / (allowance at K = 1) over the input
families below (measured by tests/test_loss_ref_cpu.py::test_float32_torch_stays_within_a_quarter_of_every_allowance, which
prints them with -s; F.cross_entropy / F.softmax / F.kl_div / autograd on the CPU).  The margin of 4 is for the kernel's
three ~1-ulp hardware approximations (exponential, logarithm, reciprocal) and a different contraction of the multiply-adds,
where torch's CPU path has a true division and libm.

    family        sums: ce     kl      I       P        dlogits
    gauss            0.35    0.014   0.45    0.28       4.21
    confident        0.010   0.015   0.38    0.78       3.92
    extreme          0.43    0.049   0.36    0.49       4.46
    near_perfect     0.001   0.020   0.50    0.53       2.52
    absent           0.38    0.099   0.39    0.38       3.74
    ties             0.43    0.021   0.44    0.71       4.69
    largest          0.785 (P, confident)               4.69 (ties, extreme teacher)
    K = 4 x largest: K_SUM = 3.2, K_DLOGITS = 19
  (worst over C in {2, 3, 4, 5, 8}, N x V = 2 x 3220, with and without a teacher.  The sums are torch's own float32 sums, so
  their ratios contain the rounding of torch's summation as well as the per-voxel term errors that K_SUM scales; with the
  simpler dlogits unit that gives every p_j the argument growth of the output class, `confident` needs 18 and `absent` 12.)
    MI355X kernels at these K, worst |delta| / allowance over the cases of tests/test_gpu_loss_ops.py: loss and coef 0.64 (0.97 on one
    row of 63 voxels), dlogits 0.25 on every family but `extreme` (0.88).
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -126          # smallest normal float32: what a flushed subnormal probability can be off by
MAXC = 8                    # MI3D_MAX_CLASSES
NCOEF = 20                  # MI3D_LOSS_COEF_FLOATS

K_SUM = 3.2                 # 4 x 0.785, the largest float32-torch ratio of the table above
K_DLOGITS = 19.0            # 4 x 4.69

# name -> (w_ce, region_kind, w_reg, alpha, beta, eps): the loss choices of the reference's training script
LOSSES = {
    "combined": (1.0, 1, 1.0, 0.0, 0.0, 1e-5), "dice": (0.0, 1, 1.0, 0.0, 0.0, 1e-5),
    "tversky": (0.0, 2, 1.0, 0.5, 0.5, 1e-6), "ce_tversky": (0.3, 2, 0.7, 0.5, 0.5, 1e-6),
    "ce_tversky73": (0.3, 2, 0.7, 0.7, 0.3, 1e-6), "ce": (1.0, 0, 0.0, 0.0, 0.0, 1e-6),
}


def make_cfg(kind, kd_alpha=None, temperature=1.0):
    """The fields of mi3d_loss_cfg as a plain dict.  kd_alpha: distillation_loss(alpha, temperature) = alpha * (0.3 CE + 0.7
    Tversky(0.7, 0.3)) + (1 - alpha) * T^2 * KL."""
    if kd_alpha is not None:
        w_ce, rk, w_reg, a, b, eps = 0.3 * kd_alpha, 2, 0.7 * kd_alpha, 0.7, 0.3, 1e-6
        return dict(w_ce=w_ce, region_kind=rk, w_reg=w_reg, alpha=a, beta=b, eps=eps, w_kd=1.0 - kd_alpha, temperature=temperature)
    w_ce, rk, w_reg, a, b, eps = LOSSES[kind]
    return dict(w_ce=w_ce, region_kind=rk, w_reg=w_reg, alpha=a, beta=b, eps=eps, w_kd=0.0, temperature=temperature)


def cfg32(cfg):
    """The configuration as the ABI sees it: every float field rounded to float32 (returned as Python floats).  A dict with
    exact=True is left alone: for comparisons with float64 code that uses the decimal constants."""
    out = dict(cfg)
    if out.get("exact"):
        return out
    for k in ("w_ce", "w_reg", "alpha", "beta", "eps", "w_kd", "temperature"):
        out[k] = float(np.float32(cfg[k]))
    return out


# ---------------------------------------------------------------------------------------------- input families
FAMILIES = ("gauss", "confident", "extreme", "near_perfect", "absent", "ties")


def make_inputs(family, N, C, V, seed):
    """(logits float32 (N, C, V), labels int64 (N, V)) of one family, from a seeded numpy generator.
      gauss         sigma = 3 logits, uniform labels
      confident     sigma = 1 plus a margin of 14 on the label's class; 1 % of the voxels carry the margin on another class
      extreme       sigma = 30
      near_perfect  sigma = 1 plus a margin of 8 on the label's class, class 1 covering half the volume
      absent        sigma = 3; the last class never occurs in the labels and its logit is -20 everywhere
      ties          logits from {-1, -0.0, +0.0, +1}"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, size=(N, V))
    g = rng.standard_normal((N, C, V))
    onehot = lambda l: (np.arange(C)[None, :, None] == l[:, None, :])
    if family == "gauss":
        z = 3.0 * g
    elif family == "confident":
        wrong = rng.random((N, V)) < 0.01
        tgt = np.where(wrong, (lab + 1 + rng.integers(0, max(C - 1, 1), size=(N, V))) % C, lab)
        z = g + 14.0 * onehot(tgt)
    elif family == "extreme":
        z = 30.0 * g
    elif family == "near_perfect":
        half = rng.random((N, V)) < 0.5
        lab = np.where(half, 1, lab)
        z = g + 8.0 * onehot(lab)
    elif family == "absent":
        a = C - 1
        lab = rng.integers(0, max(C - 1, 1), size=(N, V))
        z = 3.0 * g
        z[:, a, :] = -20.0
    elif family == "ties":
        z = np.array([-1.0, -0.0, 0.0, 1.0])[rng.integers(0, 4, size=(N, C, V))]
    else:
        raise ValueError(family)
    return z.astype(np.float32), lab.astype(np.int64)


def make_teacher(kind, N, C, V, seed):
    """Teacher logits float32 (N, C, V): 'gauss' sigma = 1.2, 'extreme' sigma = 30 (probabilities underflow to 0)."""
    rng = np.random.default_rng(seed + 7919)
    return ({"gauss": 1.2, "extreme": 30.0}[kind] * rng.standard_normal((N, C, V))).astype(np.float32)


def tied_share(logits):
    """Share of the voxels whose maximum logit is attained by more than one class."""
    z = np.asarray(logits, np.float64)
    return float(((z == z.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean())


# ---------------------------------------------------------------------------------------------- loss
def _softmax(z, inv_t=1.0):
    """p, log p and w = max - argument (>= 0) of softmax(z * inv_t) over axis 1, float64."""
    a = z * inv_t
    mx = a.max(axis=1, keepdims=True)
    e = np.exp(a - mx)
    se = e.sum(axis=1, keepdims=True)
    return e / se, (a - mx) - np.log(se), mx - a


def _onehot(labels, C):
    return (np.arange(C)[None, :, None] == np.asarray(labels)[:, None, :]).astype(np.float64)


def loss_scalars(ce_sum, kl_sum, I, P, T, N, C, V, cfg):
    """Loss and the 20 coefficients from the global sums (float64; `cfg` already rounded by cfg32)."""
    M = float(N) * float(V)
    A, B = np.zeros(MAXC), np.zeros(MAXC)
    sc = cfg["w_reg"] / (C - 1) if C > 1 else 0.0
    eps, al, be = cfg["eps"], cfg["alpha"], cfg["beta"]
    reg = 0.0
    for c in range(1, C):
        if cfg["region_kind"] == 1:
            Uc = P[c] + T[c]
            reg += 1.0 - (2.0 * I[c] + eps) / (Uc + eps)
            A[c] = -2.0 / (Uc + eps) * sc
            B[c] = (2.0 * I[c] + eps) / (Uc + eps) ** 2 * sc
        elif cfg["region_kind"] == 2:
            num = I[c] + eps
            den = I[c] + al * (P[c] - I[c]) + be * (T[c] - I[c]) + eps
            reg += 1.0 - num / den
            A[c] = (-1.0 / den + num / den ** 2 * (1.0 - al - be)) * sc
            B[c] = num / den ** 2 * al * sc
    if C > 1:
        reg /= C - 1
    temp = cfg["temperature"]
    loss = cfg["w_ce"] * ce_sum / M + cfg["w_reg"] * reg + cfg["w_kd"] * temp * temp * kl_sum / (M * C)
    coef = np.zeros(NCOEF)
    coef[:MAXC], coef[MAXC:2 * MAXC] = A, B
    coef[2 * MAXC], coef[2 * MAXC + 1], coef[2 * MAXC + 2] = cfg["w_ce"] / M, cfg["w_kd"] * temp / (M * C), loss
    return loss, coef


def dlogits_from_coef(logits, labels, coef, cfg, teacher=None, grad_out=1.0):
    """The per-voxel gradient formula on given coefficients, float64: what the backward kernel computes from `coef`."""
    cfg = cfg32(cfg)
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    coef = np.asarray(coef, np.float64)
    A, B = coef[:C].reshape(1, C, 1), coef[MAXC:MAXC + C].reshape(1, C, 1)
    ce_s, kd_s = coef[2 * MAXC], coef[2 * MAXC + 1]
    p, _, _ = _softmax(z)
    oh = _onehot(labels, C)
    g = A * oh + B
    d = ce_s * (p - oh) + p * (g - (g * p).sum(axis=1, keepdims=True))
    if cfg["w_kd"] != 0.0:
        it = 1.0 / cfg["temperature"]
        d = d + kd_s * (_softmax(z, it)[0] - _softmax(np.asarray(teacher, np.float64), it)[0])
    return float(grad_out) * d


def seg_loss_ref(logits, labels, cfg, teacher=None):
    """float64 loss family on logits (N, C, V), labels (N, V), optional teacher (N, C, V).  Returns a dict:
    loss; I, P, T (C each); ce_sum, kl_sum; coef (20 float64, the layout of the header); dlogits (N, C, V) for an upstream
    gradient of 1, analytically through the global sums."""
    cfg = cfg32(cfg)
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    p, logp, _ = _softmax(z)
    oh = _onehot(labels, C)
    ce_sum = float(-(logp * oh).sum())
    I, P, T = (p * oh).sum(axis=(0, 2)), p.sum(axis=(0, 2)), oh.sum(axis=(0, 2))
    kl_sum = 0.0
    if cfg["w_kd"] != 0.0:
        if teacher is None:
            raise ValueError("distillation weight without teacher logits")
        it = 1.0 / cfg["temperature"]
        _, lps, _ = _softmax(z, it)
        pt, lpt, _ = _softmax(np.asarray(teacher, np.float64), it)
        kl_sum = float(np.where(pt > 0.0, pt * (lpt - lps), 0.0).sum())
    loss, coef = loss_scalars(ce_sum, kl_sum, I, P, T, N, C, V, cfg)
    return dict(loss=loss, I=I, P=P, T=T, ce_sum=ce_sum, kl_sum=kl_sum, coef=coef,
                dlogits=dlogits_from_coef(z, labels, coef, cfg, teacher))


# ---------------------------------------------------------------------------------------------- metrics
def class_counts_ref(logits, labels):
    """Exact int64 counts {n_inter[C], n_pred[C], n_label[C], n_correct} of pred = first-maximum argmax against labels."""
    z = np.asarray(logits)
    C = z.shape[1]
    pred = np.argmax(z, axis=1)                  # first maximum; -0.0 == +0.0
    lab = np.asarray(labels).reshape(pred.shape)
    out = np.zeros(3 * C + 1, np.int64)
    for c in range(C):
        out[c] = np.count_nonzero((pred == c) & (lab == c))
        out[C + c] = np.count_nonzero(pred == c)
        out[2 * C + c] = np.count_nonzero(lab == c)
    out[3 * C] = np.count_nonzero(pred == lab)
    return out


def metrics_from_counts(counts, C, D, M):
    """calculate_iou / calculate_dice / calculate_accuracy on exact counts with the reference's float32 arithmetic: the class
    loop is range(1, min(D, C)) (it runs over pred.size(1) AFTER the argmax, i.e. the first spatial extent); a class counts
    only when present in the labels; intersection.float(), the int64 sum n_pred + n_label converted once, float32 quotients;
    valid = max(valid, 1).  Returns float32 (iou, dice, accuracy)."""
    f = np.float32
    iou, dice, valid = f(0), f(0), 0
    for c in range(1, min(D, C)):
        if counts[2 * C + c] > 0:
            inter = f(int(counts[c]))
            s = f(int(counts[C + c]) + int(counts[2 * C + c]))
            iou = f(iou + f(f(inter + f(1e-5)) / f(f(s - inter) + f(1e-5))))
            dice = f(dice + f(f(f(2) * inter + f(1e-5)) / f(s + f(1e-5))))
            valid += 1
    dv = f(max(valid, 1))
    return np.array([f(iou / dv), f(dice / dv), f(float(int(counts[3 * C])) / float(M))], np.float32)


def seg_metrics_ref(logits, labels, D):
    z = np.asarray(logits)
    return metrics_from_counts(class_counts_ref(z, labels), z.shape[1], D, z.shape[0] * z.shape[2])


# ---------------------------------------------------------------------------------------------- allowances
def fwd_adds_per_thread(N, V, vv, threads=256, maxblk=512):
    """Additions into one float32 per-thread accumulator of the forward pass: the grid is capped at `maxblk` blocks over all
    samples (at least one per sample), a thread owns `vv` consecutive voxels per grid-stride pass."""
    want = -(-(V // vv) // threads)
    blocks = max(1, min(want, max(maxblk // N, 1)))
    return -(-V // (blocks * threads * vv)) * vv


def sum_allowances(logits, labels, cfg, teacher=None, adds=1, k=K_SUM):
    """Allowances for the global sums {ce, kl, I[C], P[C]} of a float32 single pass against seg_loss_ref, first order in u:

        allow(S) = u (adds + 6) sum_i |x_i|  +  k u sum_i e_i  +  n TINY

    Accumulation (first term, derived, not calibrated): every term goes through at most `adds` additions of its thread's float32
    accumulator and the 6 levels of the 64-lane tree, each one rounding <= u of the running sum <= sum |x_i|; float64 from
    there on.  T_c is an exact integer and has no allowance.
    Per-voxel term error e_i (second term, in units of u, scaled by the calibrated k), with w_c = max z - z_c >= 0:
      p_c = exp(z_c - max) / se: the rounded difference z_c - max moves the exponential's argument by u w_c, the exponential,
         the reciprocal and the product are one rounding each, se carries sum_j p_j (1 + w_j):
             e(p_c) = p_c (3 + w_c + sum_j p_j (1 + w_j))                     -> terms of P_c, and of I_c where t = c
      CE term lse - z_t with lse = max + log(se) in float32: roundings of lse and of the difference, log's own, and d log(se)
         = d se / se:    e(ce) = 2 |lse| + |lse - z_t| + 1 + sum_j p_j (1 + w_j)
      KL term sum_c pt_c (lpt_c - lps_c), lp_c = z_c/T - lse: e(lp_c) = 2 |z_c/T| + 2 |lse| + 1 + sum_j p_j (1 + w_j) per side,
             e(kl) = sum_c [ e(pt_c) |lpt_c - lps_c| + pt_c (e(lpt_c) + e(lps_c) + (C + 1) |lpt_c - lps_c|) ]
    The last term covers probabilities below 2^-126 flushed to zero (n = number of terms; for KL times |lpt - lps|)."""
    cfg = cfg32(cfg)
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    acc = 0.0 if adds is None else U * (adds + 6)          # adds=None: the per-voxel term errors alone

    def parts(zz, it):
        p, lp, w = _softmax(zz, it)
        spw = (p * (1.0 + w)).sum(axis=1, keepdims=True)
        lse = (zz * it) - lp                               # same for every class
        return p, lp, p * (3.0 + w + spw), spw, lse
    p, lp, ep, spw, lse = parts(z, 1.0)
    oh = _onehot(labels, C)
    n = N * V
    out = {"I": acc * (p * oh).sum(axis=(0, 2)) + k * U * (ep * oh).sum(axis=(0, 2)) + n * TINY,
           "P": acc * p.sum(axis=(0, 2)) + k * U * ep.sum(axis=(0, 2)) + n * TINY}
    ce = -(lp * oh).sum(axis=1)
    e_ce = 2.0 * np.abs(lse[:, 0]) + ce + 1.0 + spw[:, 0]
    out["ce"] = acc * ce.sum() + k * U * e_ce.sum()
    out["kl"] = 0.0
    if cfg["w_kd"] != 0.0:
        it = 1.0 / cfg["temperature"]
        zt = np.asarray(teacher, np.float64)
        ps, lps, _, spws, lses = parts(z, it)
        pt, lpt, ept, spwt, lset = parts(zt, it)
        d = np.abs(lpt - lps)
        e_lp = (2.0 * np.abs(z * it) + 2.0 * np.abs(lses) + 1.0 + spws) + (2.0 * np.abs(zt * it) + 2.0 * np.abs(lset) + 1.0 + spwt)
        e_kl = ept * d + pt * (e_lp + (C + 1) * d)
        out["kl"] = acc * (pt * d).sum() + k * U * e_kl.sum() + TINY * d.sum()
    return out


def coef_allowances(ref, sums, N, C, V, cfg):
    """Allowances (loss, coef[20]) from those of the sums, propagated through the closed forms of loss_scalars by the absolute
    values of their partial derivatives, plus one float32 rounding (u |value|) for what is stored.  With U = P + T + eps:
      Dice     r = (2I + eps)/U:  dr = 2 dI/U + r dP/U;   A = -2/U: dA = |A| dP/U;   B = (2I + eps)/U^2: dB = 2 dI/U^2 + 2 B dP/U
               (for a class absent from labels and predictions U ~ eps and B ~ 1/eps: dB is dominated by dP/eps^2-sized terms)
      Tversky  num = I + eps, den = I (1 - a - b) + a P + b T + eps (the kernel forms P - I and T - I from the float32-summed
               I and P, so their errors enter den directly): dden = |1 - a - b| dI + a dP, q = num/den: dq = dI/den + q dden/den,
               A = -1/den + (1 - a - b) num/den^2: dA = dden/den^2 + |1 - a - b| (dI/den^2 + 2 num dden/den^3)
               B = a num/den^2:                    dB = a (dI/den^2 + 2 num dden/den^3)
    ce_s and kd_s depend on the configuration alone: one rounding."""
    cfg = cfg32(cfg)
    M = float(N) * float(V)
    I, P, T = ref["I"], ref["P"], ref["T"]
    dI, dP = sums["I"], sums["P"]
    sc = cfg["w_reg"] / (C - 1) if C > 1 else 0.0
    eps, al, be = cfg["eps"], cfg["alpha"], cfg["beta"]
    dcoef = np.zeros(NCOEF)
    dreg = 0.0
    for c in range(1, C):
        if cfg["region_kind"] == 1:
            Uc = P[c] + T[c] + eps
            r = (2.0 * I[c] + eps) / Uc
            dreg += 2.0 * dI[c] / Uc + r * dP[c] / Uc
            dA = 2.0 / Uc * dP[c] / Uc
            dB = 2.0 * dI[c] / Uc ** 2 + 2.0 * (r / Uc) * dP[c] / Uc
        elif cfg["region_kind"] == 2:
            num = I[c] + eps
            den = I[c] + al * (P[c] - I[c]) + be * (T[c] - I[c]) + eps
            k1 = abs(1.0 - al - be)
            dden = k1 * dI[c] + al * dP[c]
            dreg += dI[c] / den + num / den * dden / den
            dA = dden / den ** 2 + k1 * (dI[c] / den ** 2 + 2.0 * num * dden / den ** 3)
            dB = al * (dI[c] / den ** 2 + 2.0 * num * dden / den ** 3)
        else:
            dA = dB = 0.0
        dcoef[c], dcoef[MAXC + c] = sc * dA, sc * dB
    if C > 1:
        dreg /= C - 1
    temp = cfg["temperature"]
    dloss = cfg["w_ce"] * sums["ce"] / M + cfg["w_reg"] * dreg + cfg["w_kd"] * temp * temp * sums["kl"] / (M * C)
    dcoef[2 * MAXC + 2] = dloss
    dcoef += U * np.abs(ref["coef"])
    return dloss + U * abs(ref["loss"]), dcoef


def dlogits_allowance(logits, labels, coef, cfg, teacher=None, grad_out=1.0, k=K_DLOGITS):
    """Per-element allowance of a float32 evaluation of dlogits_from_coef on the same `coef`:

        allow_c = k u |go| ( (|ce_s| (p_c + [c = t]) + p_c (|g_c| + sum_j |g_j| p_j)) (1 + w_c)
                             + p_c sum_j |g_j| p_j (1 + w_j)
                             + |kd_s| (ps_c (1 + ws_c) + pt_c (1 + wt_c)) )  +  floor
        floor   = 2^-126 |go| (|ce_s| + max|A| + max|B| + |kd_s|)

    The first and third lines are the sum of the absolute values of the terms of the per-voxel formula (no cancellation is
    credited), each with the argument growth of its own softmax: w_c = max z - z_c enters the relative error of p_c (the
    rounded difference z_c - max moves the exponential's argument by u w_c; for the two distillation softmaxes the arguments
    are z / T).  The second line is the error of the inner product sum_j g_j p_j itself, in which every p_j carries its OWN
    w_j: at the confident class (w_c = 0) of a well-predicted voxel the whole value is -p_c sum_{j != c} B_j p_j, made of
    probabilities e^-14 whose relative error is 15 u, and for an absent class B_j ~ 1/eps multiplies a p_j ~ e^-17.  Without
    that line float32 torch itself needs k = 18 on `confident` and 12 on `absent` (with it: the table in the module
    docstring).  The floor covers probabilities below 2^-126 flushed to zero, whose relative error is unbounded."""
    cfg = cfg32(cfg)
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    coef = np.asarray(coef, np.float64)
    A, B = np.abs(coef[:C]).reshape(1, C, 1), np.abs(coef[MAXC:MAXC + C]).reshape(1, C, 1)
    ce_s, kd_s, go = abs(coef[2 * MAXC]), abs(coef[2 * MAXC + 1]), abs(float(grad_out))
    p, _, w = _softmax(z)
    oh = _onehot(labels, C)
    g = A * oh + B
    s = (ce_s * (p + oh) + p * (g + (g * p).sum(axis=1, keepdims=True))) * (1.0 + w) + p * (g * p * (1.0 + w)).sum(axis=1, keepdims=True)
    if cfg["w_kd"] != 0.0:
        it = 1.0 / cfg["temperature"]
        ps, _, ws = _softmax(z, it)
        pt, _, wt = _softmax(np.asarray(teacher, np.float64), it)
        s = s + kd_s * (ps * (1.0 + ws) + pt * (1.0 + wt))
    else:
        kd_s = 0.0
    return k * U * go * s + TINY * go * (ce_s + A.max() + B.max() + kd_s)
