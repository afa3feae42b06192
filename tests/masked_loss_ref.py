"""Plain float64 numpy model of the ignore value of the loss family (include/mi3d.h, "Ignore value": the `_masked` entries of
csrc/head_loss.hip) and of mi3d_pseudo_labels, on top of tests/loss_ref.py: the loss, the 20 coefficients, dlogits, the fused
metric counts and the three metrics, the allowances re-derived for M_valid, the mask families and the case table of
tests/test_gpu_masked_loss.py.  It imports loss_ref (families, cfg32, the K constants) and nothing of the product; it is pinned to
float64 torch autograd, to loss_ref itself and to its own mutants by tests/test_masked_loss_ref_cpu.py.

With m_v = [t_v != ignore_index] and M_valid = sum m_v over all N * V voxels:
    CE_mean = sum m_v (lse_v - z_v[t_v]) / M_valid   (0 when M_valid = 0),   I_c, P_c, T_c: the sums of loss_ref times m_v
    the distillation term over ALL voxels, divisor N * V * C;   ce_s = w_ce / M_valid (0 when M_valid = 0), kd_s unchanged
    dlogits: the unmasked expression where m_v = 1;  go * kd_s (ps - pt) where m_v = 0 (A = B = ce_s = 0 in that expression)
    counts without the ignored voxels, accuracy = n_correct / M_valid (0 when M_valid = 0)

Allowances.  A select contributes no rounding, so an ignored voxel adds nothing to the allowance of ce, I or P: those are
loss_ref.sum_allowances on the compacted valid voxels (the per-voxel terms are sums over voxels, so compaction is exact); kl
keeps every voxel.  `adds` stays the additions of a thread's accumulator over ALL its voxels (an ignored voxel still adds a
zero: no rounding, but the bound does not credit that).  coef_allowances runs on M_valid for the CE part; dlogits_allowance
is loss_ref's where m_v = 1 and its distillation part alone where m_v = 0 (without a teacher: 0, an exact zero is required).

Allowance constants: the rule of loss_ref.py (4 x the largest |float32 torch - float64| / allowance at K = 1) re-run on the
masked inputs by test_masked_loss_ref_cpu.py::test_float32_torch_stays_within_a_quarter_of_every_allowance, which prints the
ratios with -s; measured there (worst over C in {2, 3, 4, 5, 8}, N x V = 2 x 3220, every input family with and without a
teacher, ignore_index walking through IGNORES, K = 1):
    mask family    sums: ce     kl      I       P        dlogits where counted   where ignored
    none             0.497   0.099   0.503   0.785         4.692                   4.236   (ignore_index 0 / 1 ignore a class)
    random30         0.667   0.099   0.589   0.605         4.844                   6.125
    runs             0.728   0.099   0.686   0.686         4.334                   6.369
    sample           0.561   0.099   0.608   0.506         4.520                   6.369
    class            0.627   0.099   0.452   0.565         4.737                   6.369
    all_but_one      0.289   0.099   0.454   0.781         1.999                   6.402
    all              0       0.099   0       0             -                       6.402
    largest          0.785 (P, none)                       4.844 (random30)        6.402
  sums: inside K_SUM / 4 = 0.8, so loss_ref's K_SUM = 3.2 holds for every mask family and is used unchanged.
  dlogits where the voxel counts: random30 needs 4 x 4.844 = 19.4 -> K_DLOGITS = 20 here (loss_ref: 19).
  dlogits where it is ignored: the allowance is the distillation part alone, which in loss_ref's table never stood alone (the CE
  and region parts of the same element widened it); float32 torch needs 6.40 of it -> K_DLOGITS_IGNORED = 4 x 6.402 = 26.
The constants come from float32 torch on the CPU alone; they were not tuned against the kernels.
"""
import numpy as np

import loss_ref as L

K_SUM = L.K_SUM
K_DLOGITS = 20.0                            # 4 x 4.844, the largest float32-torch ratio at a voxel that counts (module docstring)
K_DLOGITS_IGNORED = 26.0                    # 4 x 6.402, the largest at an ignored voxel
MASKS = ("none", "random30", "runs", "sample", "class", "all_but_one", "all")
IGNORES = (255, -100, "C", 0, 1)            # "C": the class count itself, the first value past the range
MUTANTS = ("ce_div_nv", "p_unmasked", "t_counts_ignored", "kd_masked", "ce_grad_on_ignored", "n_pred_counts_ignored",
           "acc_over_nv")


# ---------------------------------------------------------------------------------------------- mask families
def make_mask(family, labels, C, seed):
    """Boolean (N, V) `ignored` of one family on labels (N, V), from a seeded generator.
      none         nothing                     random30     iid 30 %
      runs         runs of 64..256 consecutive voxels per sample, starts alternately aligned to 64 and not: whole empty waves and
                   whole float4 groups
      sample       sample 0 entirely           class        every voxel of foreground class 1 (class 0 when C = 1)
      all_but_one  everything but one voxel    all          everything"""
    rng = np.random.default_rng(seed + 104729)
    N, V = labels.shape
    ig = np.zeros((N, V), bool)
    if family == "none":
        pass
    elif family == "random30":
        ig = rng.random((N, V)) < 0.3
    elif family == "runs":
        for n in range(N):
            pos, aligned = 0, True
            while pos < V:
                start = pos + int(rng.integers(16, 200))
                if aligned:
                    start = -(-start // 64) * 64
                else:
                    start += 1 if start % 64 == 0 else 0
                length = int(rng.integers(64, 257))
                ig[n, start:start + length] = True
                pos, aligned = start + length, not aligned
    elif family == "sample":
        ig[0] = True
    elif family == "class":
        ig = labels == (1 if C > 1 else 0)
    elif family == "all_but_one":
        ig[:] = True
        ig[N - 1, V // 2] = False
    elif family == "all":
        ig[:] = True
    else:
        raise ValueError(family)
    return ig


def ignore_value(ignore, C):
    return C if ignore == "C" else int(ignore)


def apply_mask(labels, ignored, ignore_index):
    """The labels the entry sees: ignore_index where `ignored`.  (A voxel that carried ignore_index already is ignored too:
    inside the class range the value takes the whole class with it.)"""
    return np.where(ignored, np.int64(ignore_index), labels).astype(np.int64)


# ---------------------------------------------------------------------------------------------- loss
def _valid(labels, ignore_index):
    return np.asarray(labels) != ignore_index


def masked_loss_ref(logits, labels, cfg, ignore_index, teacher=None, mutant=None):
    """The masked loss family in float64; the dict of loss_ref.seg_loss_ref plus M_valid.  mutant: one of MUTANTS, a wrong
    reading of the contract that the case table has to tell from the right one (test_masked_loss_ref_cpu.py)."""
    cfg = L.cfg32(cfg)
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    lab = np.asarray(labels)
    m = _valid(lab, ignore_index)
    mm = m[:, None, :].astype(np.float64)
    p, logp, _ = L._softmax(z)
    oh = L._onehot(np.where(m, lab, -1), C)                        # no class where ignored
    oh_sums = L._onehot(lab, C) if mutant == "t_counts_ignored" else oh
    ce_sum = float(-(logp * oh).sum())
    I, T = (p * oh_sums).sum(axis=(0, 2)), oh_sums.sum(axis=(0, 2))
    P = (p if mutant == "p_unmasked" else p * mm).sum(axis=(0, 2))
    M_valid = int(m.sum())
    kl_sum = 0.0
    if cfg["w_kd"] != 0.0:
        if teacher is None:
            raise ValueError("distillation weight without teacher logits")
        it = 1.0 / cfg["temperature"]
        _, lps, _ = L._softmax(z, it)
        pt, lpt, _ = L._softmax(np.asarray(teacher, np.float64), it)
        kl = np.where(pt > 0.0, pt * (lpt - lps), 0.0)
        kl_sum = float((kl * mm if mutant == "kd_masked" else kl).sum())
    # the region part and A, B from loss_ref's closed forms (w_ce = w_kd = 0 there: 0 + x + 0 is x exactly), then the CE term
    # over M_valid and the distillation term over N * V * C, added in loss_ref's order
    reg_loss, coef = L.loss_scalars(0.0, 0.0, I, P, T, N, C, V, dict(cfg, w_ce=0.0, w_kd=0.0))
    M = float(N) * float(V)
    Mce = M if mutant == "ce_div_nv" else float(M_valid)
    temp = cfg["temperature"]
    ce_mean = cfg["w_ce"] * ce_sum / Mce if Mce > 0 else 0.0
    loss = ce_mean + reg_loss + cfg["w_kd"] * temp * temp * kl_sum / (M * C)
    coef[2 * L.MAXC] = cfg["w_ce"] / Mce if Mce > 0 else 0.0
    coef[2 * L.MAXC + 1] = cfg["w_kd"] * temp / (M * C)
    coef[2 * L.MAXC + 2] = loss
    return dict(loss=loss, I=I, P=P, T=T, ce_sum=ce_sum, kl_sum=kl_sum, coef=coef, M_valid=M_valid,
                dlogits=masked_dlogits_from_coef(z, lab, coef, cfg, ignore_index, teacher, mutant=mutant))


def _kd_only(coef):
    c = np.array(coef, np.float64)
    c[:2 * L.MAXC + 1] = 0.0                                       # A = B = ce_s = 0
    return c


def masked_dlogits_from_coef(logits, labels, coef, cfg, ignore_index, teacher=None, grad_out=1.0, mutant=None):
    """The per-voxel gradient on given coefficients: loss_ref.dlogits_from_coef where the voxel counts, the same expression
    with A = B = ce_s = 0 (grad_out * kd) where it is ignored."""
    lab = np.asarray(labels)
    m = _valid(lab, ignore_index)
    full = L.dlogits_from_coef(logits, np.where(m, lab, -1), coef, cfg, teacher, grad_out)
    if mutant == "kd_masked":
        ign = np.zeros_like(full)
    elif mutant == "ce_grad_on_ignored":
        c = _kd_only(coef)
        c[2 * L.MAXC] = np.asarray(coef, np.float64)[2 * L.MAXC]
        ign = L.dlogits_from_coef(logits, lab, c, cfg, teacher, grad_out)
    else:
        ign = L.dlogits_from_coef(logits, lab, _kd_only(coef), cfg, teacher, grad_out)
    return np.where(m[:, None, :], full, ign)


# ---------------------------------------------------------------------------------------------- metrics
def masked_counts_ref(logits, labels, ignore_index, mutant=None):
    """Exact int64 {n_inter[C], n_pred[C], n_label[C], n_correct} of the voxels that count."""
    z = np.asarray(logits)
    C = z.shape[1]
    pred = np.argmax(z, axis=1)
    lab = np.asarray(labels).reshape(pred.shape)
    m = _valid(lab, ignore_index)
    out = np.zeros(3 * C + 1, np.int64)
    for c in range(C):
        out[c] = np.count_nonzero((pred == c) & (lab == c) & m)
        out[C + c] = np.count_nonzero(pred == c) if mutant == "n_pred_counts_ignored" else np.count_nonzero((pred == c) & m)
        out[2 * C + c] = np.count_nonzero((lab == c) & m)
    out[3 * C] = np.count_nonzero((pred == lab) & m)
    return out


def masked_metrics_ref(logits, labels, ignore_index, D, mutant=None):
    """float32 (iou, dice, accuracy): loss_ref.metrics_from_counts on the masked counts, accuracy over M_valid (0 when 0)."""
    z = np.asarray(logits)
    N, C, V = z.shape
    cnt = masked_counts_ref(z, labels, ignore_index, mutant)
    mv = N * V if mutant == "acc_over_nv" else int(_valid(labels, ignore_index).sum())
    out = L.metrics_from_counts(cnt, C, D, max(mv, 1))
    if mv == 0:
        out[2] = np.float32(0)
    return out


# ---------------------------------------------------------------------------------------------- allowances
def masked_sum_allowances(logits, labels, cfg, ignore_index, teacher=None, adds=1, k=K_SUM):
    """loss_ref.sum_allowances for {ce, I, P} on the compacted valid voxels (N = 1, V = M_valid) and for kl on every voxel."""
    z = np.asarray(logits, np.float64)
    N, C, V = z.shape
    m = _valid(labels, ignore_index)
    zc = np.ascontiguousarray(z.transpose(1, 0, 2)[:, m])[None]                   # (1, C, M_valid)
    lc = np.asarray(labels)[m][None]
    out = L.sum_allowances(zc, lc, dict(L.cfg32(cfg), w_kd=0.0), None, adds=adds, k=k)
    if L.cfg32(cfg)["w_kd"] != 0.0:
        out["kl"] = L.sum_allowances(z, np.where(m, labels, 0), cfg, teacher, adds=adds, k=k)["kl"]
    return out


def masked_coef_allowances(ref, sums, N, C, V, cfg):
    """loss_ref.coef_allowances with the CE sum over M_valid: d(w_ce ce / M_valid) = w_ce d(ce) / M_valid, handed over as the
    allowance of a sum that is divided by N * V; nothing when M_valid = 0 (the term is an exact 0)."""
    s = dict(sums)
    mv = ref["M_valid"]
    s["ce"] = sums["ce"] * (float(N) * float(V)) / mv if mv > 0 else 0.0
    return L.coef_allowances(ref, s, N, C, V, cfg)


def masked_dlogits_allowance(logits, labels, coef, cfg, ignore_index, teacher=None, grad_out=1.0, k=K_DLOGITS, k_ignored=K_DLOGITS_IGNORED):
    """loss_ref.dlogits_allowance at constant k where the voxel counts; where it is ignored, the distillation part of that
    allowance alone, at constant k_ignored."""
    lab = np.asarray(labels)
    m = _valid(lab, ignore_index)
    full = L.dlogits_allowance(logits, np.where(m, lab, -1), coef, cfg, teacher, grad_out, k)
    if L.cfg32(cfg)["w_kd"] != 0.0:
        ign = L.dlogits_allowance(logits, np.where(m, lab, -1), _kd_only(coef), cfg, teacher, grad_out, k_ignored)
    else:
        ign = np.zeros_like(full)
    return np.where(m[:, None, :], full, ign)


# ---------------------------------------------------------------------------------------------- pseudo-labels
def pseudo_labels_ref(labels, confidence, thresholds, ignore_index):
    """target int64 = label where label < C and confidence >= thresholds[label] (NaN compares false), else ignore_index; table
    int64 (N, C + 1): kept per class, then ignored, per sample.  labels uint8 (N, V), confidence float32 (N, V)."""
    lab = np.asarray(labels).astype(np.int64)
    conf = np.asarray(confidence, np.float32)
    thr = np.asarray(thresholds, np.float32)
    C = thr.size
    known = lab < C
    with np.errstate(invalid="ignore"):
        keep = known & (conf >= thr[np.where(known, lab, 0)])
    target = np.where(keep, lab, np.int64(ignore_index))
    table = np.zeros((lab.shape[0], C + 1), np.int64)
    for c in range(C):
        table[:, c] = (keep & (lab == c)).sum(axis=1)
    table[:, C] = (~keep).sum(axis=1)
    return target, table


# ---------------------------------------------------------------------------------------------- the case table
V0 = 4 * (256 * 3 + 37)                     # 3220, as tests/test_gpu_loss_ops.py
KD72, KD34 = ("kd", 0.7, 2.0), ("kd", 0.3, 4.0)
A, B_, AM, S63, S1, BIG = (2, V0, 0), (2, V0 + 1, 0), (2, V0, 1), (1, 63, 0), (1, 1, 0), (64, 17556, 0)
# (family, (N, V, off), C, loss, teacher kind, grad_out, mask family, ignore)     instantiation NC, VV, EXACT, TEACH
CASES = [
    ("gauss", A, 4, "combined", None, None, "none", 255),                # 4 4 E -
    ("gauss", A, 4, "combined", None, None, "random30", 255),            # 4 4 E -
    ("gauss", A, 3, "dice", None, 0.5, "runs", -100),                    # 4 4 - -
    ("gauss", A, 2, "combined", None, None, "sample", "C"),              # 4 4 - -
    ("gauss", A, 5, "ce_tversky73", None, 3.0, "class", 255),            # 8 4 - -
    ("gauss", A, 8, "combined", None, None, "random30", 1),              # 8 4 E -   the value inside the range: class 1 goes too
    ("gauss", A, 4, "tversky", None, None, "all_but_one", 0),            # 4 4 E -
    ("gauss", A, 4, "combined", None, None, "all", 255),                 # 4 4 E -   the documented zeros
    ("gauss", A, 3, KD72, "gauss", None, "random30", 255),               # 4 4 - T
    ("gauss", A, 4, KD72, "extreme", 3.0, "runs", 1),                    # 4 4 E T
    ("gauss", A, 5, KD34, "gauss", None, "none", -100),                  # 8 4 - T
    ("gauss", A, 8, KD72, "gauss", 0.5, "all", "C"),                     # 8 4 E T   the loss is the distillation term alone
    ("gauss", B_, 2, KD72, "gauss", None, "runs", 255),                  # 4 1 - T
    ("gauss", B_, 4, KD34, "gauss", 0.5, "sample", 0),                   # 4 1 E T
    ("gauss", B_, 5, KD72, "gauss", None, "class", "C"),                 # 8 1 - T
    ("gauss", B_, 8, KD34, "extreme", None, "random30", -100),           # 8 1 E T
    ("gauss", B_, 3, "ce", None, None, "random30", 1),                   # 4 1 - -
    ("gauss", B_, 4, "combined", None, None, "runs", 255),               # 4 1 E -
    ("gauss", B_, 5, "dice", None, None, "none", 255),                   # 8 1 - -
    ("gauss", B_, 8, "tversky", None, 3.0, "all_but_one", -100),         # 8 1 E -
    ("gauss", AM, 4, "combined", None, None, "random30", 255),           # 4 1 E -   scalar route chosen by alignment
    ("gauss", AM, 8, KD72, "gauss", None, "runs", 0),                    # 8 1 E T
    ("confident", A, 4, "combined", None, None, "class", 255),           # 4 4 E -
    ("extreme", A, 4, "combined", None, 0.5, "random30", -100),          # 4 4 E -
    ("near_perfect", A, 4, "tversky", None, None, "runs", 255),          # 4 4 E -
    ("absent", A, 4, "dice", None, None, "random30", "C"),               # 4 4 E -
    ("ties", A, 4, "combined", None, None, "random30", 255),             # 4 4 E -   tied maxima in the masked metric counts
    ("ties", B_, 8, "ce_tversky73", None, None, "class", 1),             # 8 1 E -
    ("gauss", S63, 4, "combined", None, None, "random30", 255),          # 4 1 E -   less than one wave
    ("gauss", S63, 8, KD72, "gauss", None, "all", 255),                  # 8 1 E T
    ("gauss", S1, 3, "combined", None, 3.0, "none", 255),                # 4 1 - -   one voxel, counted
    ("gauss", S1, 3, "combined", None, 3.0, "all", 255),                 # 4 1 - -   one voxel, ignored
    ("gauss", BIG, 3, "combined", None, None, "runs", 255),              # 4 4 - -   the grid stride, ragged last pass
    ("ties", BIG, 2, KD72, "gauss", None, "random30", "C"),              # 4 4 - T
]
IDS = ["%02d-%s-%dx%d+%d-C%d-%s-%s-ig%s%s" % (i, c[0], c[1][0], c[1][1], c[1][2], c[2], c[3] if isinstance(c[3], str) else "kd%g" % c[3][1],
                                              c[6], c[7], "-go%g" % c[5] if c[5] else "") for i, c in enumerate(CASES)]


def case_inputs(i):
    """Inputs of row i: dict(N, V, off, C, cfg, z, lab (with the ignore value in place), teacher, go, ignore, D)."""
    fam, (N, V, off), Cc, loss, tk, go, mask, ignore = CASES[i]
    cfg = L.make_cfg(None, loss[1], loss[2]) if isinstance(loss, tuple) else L.make_cfg(loss)
    z, lab = L.make_inputs(fam, N, Cc, V, seed=700 + i)
    teacher = L.make_teacher(tk, N, Cc, V, seed=700 + i) if tk else None
    ig = ignore_value(ignore, Cc)
    lab = apply_mask(lab, make_mask(mask, lab, Cc, seed=700 + i), ig)
    return dict(N=N, V=V, off=off, C=Cc, cfg=cfg, z=z, lab=lab, teacher=teacher, go=go, ignore=ig, mask=mask, D=(1, 2, Cc, Cc + 3)[i % 4])
