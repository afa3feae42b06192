"""Pins tests/loss_ref.py (the float64 references and allowances behind tests/test_gpu_loss_ops.py) so that it cannot
drift together with the product: against float64 torch autograd restating the reference's loss functions, against the
reference-run fixtures of tests/golden/losses_metrics.npz, against central differences, against the literal torch lines of
the metric functions, and the allowances against float32 torch (inside K / 4) and against a deliberately wrong gradient."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_metrics.npz")
V0 = 4 * (256 * 3 + 37)


# ------------------------------------------------------------------------------ torch restatements (any dtype)
def t_dice_part(pred, target):
    p = F.softmax(pred, dim=1)
    out = 0
    for c in range(1, p.size(1)):
        pm, tm = p[:, c], (target == c).to(pred.dtype)
        out = out + 1 - (2.0 * (pm * tm).sum() + 1e-5) / (pm.sum() + tm.sum() + 1e-5)
    return out / (p.size(1) - 1)


def t_tversky(pred, target, alpha, beta, eps=1e-6):
    p = F.softmax(pred, dim=1)
    out = 0
    for c in range(1, p.size(1)):
        pm, tm = p[:, c], (target == c).to(pred.dtype)
        tp, fp, fn = (pm * tm).sum(), (pm * (1 - tm)).sum(), ((1 - pm) * tm).sum()
        out = out + 1 - (tp + eps) / (tp + alpha * fp + beta * fn + eps)
    return out / (p.size(1) - 1)


def t_loss(name, pred, target, teacher=None, kd_alpha=None, temp=None):
    """pred (N, C, V), target (N, V): the reference's loss functions by name; kd_alpha selects distillation_loss."""
    if kd_alpha is not None:
        seg = 0.3 * F.cross_entropy(pred, target) + 0.7 * t_tversky(pred, target, 0.7, 0.3)
        kl = F.kl_div(F.log_softmax(pred / temp, dim=1), F.softmax(teacher / temp, dim=1), reduction="none").mean() * temp ** 2
        return kd_alpha * seg + (1 - kd_alpha) * kl
    if name == "combined":
        return F.cross_entropy(pred, target) + t_dice_part(pred, target)
    if name == "dice":
        return t_dice_part(pred, target)
    if name == "tversky":
        return t_tversky(pred, target, 0.5, 0.5)
    if name == "ce_tversky":
        return 0.3 * F.cross_entropy(pred, target) + 0.7 * t_tversky(pred, target, 0.5, 0.5)
    if name == "ce_tversky73":
        return 0.3 * F.cross_entropy(pred, target) + 0.7 * t_tversky(pred, target, 0.7, 0.3)
    if name == "ce":
        return F.cross_entropy(pred, target)
    raise KeyError(name)


def ref_exact(z, lab, cfg, teacher=None):
    """seg_loss_ref without the float32 rounding of the configuration (the torch restatements use the decimal constants)."""
    return L.seg_loss_ref(z, lab, dict(cfg, exact=True), teacher)


# ------------------------------------------------------------------------------ float64 autograd
@pytest.mark.parametrize("C", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("family", ["gauss", "near_perfect", "absent"])
def test_loss_and_gradient_against_float64_autograd(C, family):
    N, V = 2, 61
    z, lab = L.make_inputs(family, N, C, V, seed=10 * C + len(family))
    teacher = L.make_teacher("gauss", N, C, V, seed=C)
    cases = [(n, None, None) for n in ("combined", "dice", "tversky", "ce_tversky", "ce_tversky73", "ce")]
    cases += [("kd", 0.7, 2.0), ("kd", 0.3, 4.0)]
    for name, ka, temp in cases:
        cfg = L.make_cfg(name, ka, temp) if ka is not None else L.make_cfg(name)
        r = ref_exact(z, lab, cfg, teacher if ka is not None else None)
        zt = torch.from_numpy(z).double().requires_grad_(True)
        l = t_loss(name, zt, torch.from_numpy(lab), torch.from_numpy(teacher).double(), ka, temp)
        l.backward()
        g = zt.grad.numpy()
        assert abs(r["loss"] - l.item()) <= 1e-12 * abs(l.item()), (name, C, family)
        d = np.abs(r["dlogits"] - g)
        assert np.linalg.norm(d) <= 1e-12 * np.linalg.norm(g), (name, C, family)
        assert (d <= 1e-12 * np.abs(g) + 1e-12 * np.linalg.norm(g) / np.sqrt(g.size)).all(), (name, C, family, d.max())
        assert r["loss"] == r["coef"][2 * L.MAXC + 2] and r["coef"][2 * L.MAXC + 3] == 0.0


def test_gradient_against_central_differences():
    N, C, V = 1, 3, 5
    z, lab = L.make_inputs("gauss", N, C, V, seed=4)
    z = z.astype(np.float64) / 3.0
    teacher = L.make_teacher("gauss", N, C, V, seed=4)
    for cfg in (L.make_cfg("combined"), L.make_cfg("ce_tversky73"), L.make_cfg(None, 0.7, 2.0)):
        tch = teacher if cfg["w_kd"] else None
        g = L.seg_loss_ref(z, lab, cfg, tch)["dlogits"]
        h = 1e-6
        for idx in np.ndindex(z.shape):
            zp, zm = z.copy(), z.copy()
            zp[idx] += h
            zm[idx] -= h
            fd = (L.seg_loss_ref(zp, lab, cfg, tch)["loss"] - L.seg_loss_ref(zm, lab, cfg, tch)["loss"]) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-8 + 1e-7 * abs(g[idx]), (idx, fd, g[idx])


def test_dlogits_rebuilt_from_coef_alone():
    """The gradient is a function of (logits, labels, teacher, coef) only: rebuilt from the 20 numbers by the per-voxel formula
    it equals float64 autograd, for an upstream gradient too; and the float32-rounded coef the kernel is fed moves it by no
    more than the rounding of the coefficients."""
    N, C, V = 2, 5, 97
    z, lab = L.make_inputs("gauss", N, C, V, seed=2)
    teacher = L.make_teacher("gauss", N, C, V, seed=2)
    cfg = L.make_cfg(None, 0.3, 4.0)
    r = ref_exact(z, lab, cfg, teacher)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    (3.0 * t_loss("kd", zt, torch.from_numpy(lab), torch.from_numpy(teacher).double(), 0.3, 4.0)).backward()
    d = L.dlogits_from_coef(z, lab, r["coef"], dict(cfg, exact=True), teacher, grad_out=3.0)
    d32 = L.dlogits_from_coef(z, lab, r["coef"].astype(np.float32), dict(cfg, exact=True), teacher, grad_out=3.0)
    g = zt.grad.numpy()
    assert np.abs(d - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(d32 - d).max() <= 4 * L.U * np.abs(g).max()
    assert np.abs(d32 - d).max() > 0


# ------------------------------------------------------------------------------ fixtures
FIXTURE_LOSSES = {"combined": "combined", "default_fn": "combined", "tversky55": "tversky", "tversky_fn": "tversky",
                  "ce_tversky73": "ce_tversky73", "ce_tversky55": "ce_tversky", "dice": "dice"}


def _fixture_cases():
    g = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in g.files})


@pytest.mark.parametrize("case", _fixture_cases())
def test_reference_run_fixtures(case):
    """Every case of the fixture file (float32 results of the reference's own functions): losses and gradients at the
    tolerances test_losses_golden grants the product on the same numbers, the float64 run to 1e-9, the three metrics as
    test_metrics_golden."""
    g = np.load(GOLDEN)
    z = g[f"{case}/logits"]
    n, c = z.shape[:2]
    d = z.shape[2]
    z = z.reshape(n, c, -1)
    lab = g[f"{case}/labels"].reshape(n, -1)
    for name, kind in FIXTURE_LOSSES.items():
        if f"{case}/{name}/loss" not in g.files:
            continue
        r = L.seg_loss_ref(z, lab, L.make_cfg(kind))
        np.testing.assert_allclose(r["loss"], g[f"{case}/{name}/loss"], rtol=2e-5, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(r["dlogits"], g[f"{case}/{name}/grad"].reshape(n, c, -1), rtol=2e-3, atol=3e-7, err_msg=name)
    if f"{case}/combined64/loss" in g.files:
        r = ref_exact(z, lab, L.make_cfg("combined"))
        np.testing.assert_allclose(r["loss"], g[f"{case}/combined64/loss"], rtol=1e-9)
        gr = g[f"{case}/combined64/grad"].reshape(n, c, -1)
        assert np.abs(r["dlogits"] - gr).max() <= 1e-9 * np.abs(gr).max()
    for alpha, temp in ((0.7, 2.0), (0.3, 4.0)):
        key = f"{case}/distill_a{alpha}_t{temp}"
        if key + "/loss" not in g.files:
            continue
        r = L.seg_loss_ref(z, lab, L.make_cfg(None, alpha, temp), g[f"{case}/teacher"].reshape(n, c, -1))
        np.testing.assert_allclose(r["loss"], g[key + "/loss"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(r["dlogits"], g[key + "/grad"].reshape(n, c, -1), rtol=2e-3, atol=3e-7)
    if f"{case}/calculate_iou" in g.files:
        m = L.seg_metrics_ref(z, lab, d)
        for i, k in enumerate(("calculate_iou", "calculate_dice", "calculate_accuracy")):
            np.testing.assert_allclose(float(m[i]), g[f"{case}/{k}"], rtol=1e-6, atol=1e-7, err_msg=k)


# ------------------------------------------------------------------------------ metrics
def t_metrics(pred5, target5):
    """The literal lines of calculate_iou / calculate_dice / calculate_accuracy on (B, C, D, H, W) / (B, 1, D, H, W)."""
    target = target5.squeeze(1)
    pred = torch.argmax(pred5, dim=1)
    iou, dice, valid = 0, 0, 0
    for c in range(1, pred.size(1)):
        pm, tm = pred == c, target == c
        if tm.sum() > 0:
            inter = (pm & tm).sum().float()
            union = pm.sum() + tm.sum() - inter
            iou += (inter + 1e-5) / (union + 1e-5)
            dice += (2. * inter + 1e-5) / (pm.sum() + tm.sum() + 1e-5)
            valid += 1
    acc = (pred == target).float().mean()
    return np.array([float(iou / max(valid, 1)), float(dice / max(valid, 1)), float(acc)], np.float32)


@pytest.mark.parametrize("family", ["gauss", "ties", "confident", "absent"])
@pytest.mark.parametrize("C,dhw", [(2, (3, 5, 7)), (4, (2, 8, 9)), (4, (1, 9, 11)), (5, (8, 4, 5)), (8, (3, 6, 7)), (8, (11, 3, 4))])
def test_metrics_and_counts_against_the_literal_torch_lines(family, C, dhw):
    """D < C, D == 1 (no class enters), D > C; tie-heavy logits (first maximum, -0.0 == +0.0)."""
    N, V = 2, int(np.prod(dhw))
    z, lab = L.make_inputs(family, N, C, V, seed=C + dhw[0])
    if family == "ties":
        assert L.tied_share(z) >= 0.25
    zt, lt = torch.from_numpy(z).reshape(N, C, *dhw), torch.from_numpy(lab).reshape(N, 1, *dhw)
    want = t_metrics(zt, lt)
    got = L.seg_metrics_ref(z, lab, dhw[0])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    cnt = L.class_counts_ref(z, lab)
    pc, lc = torch.argmax(zt, dim=1), lt.squeeze(1)
    for c in range(C):
        assert cnt[c] == int(((pc == c) & (lc == c)).sum())
        assert cnt[C + c] == int((pc == c).sum()) and cnt[2 * C + c] == int((lc == c).sum())
    assert cnt[3 * C] == int((pc == lc).sum()) == cnt[:C].sum()
    # per-class evaluation lines (absent class -> skipped) on the same counts
    for c in range(1, C):
        pm, lm = pc == c, lc == c
        if lm.sum() > 0:
            inter = (pm & lm).sum().float()
            dice = ((2. * inter + 1e-5) / (pm.sum() + lm.sum() + 1e-5)).item()
            f = np.float32
            mine = f(f(f(2) * f(cnt[c]) + f(1e-5)) / f(f(int(cnt[C + c]) + int(cnt[2 * C + c])) + f(1e-5)))
            assert mine == f(dice)


def test_metrics_no_class_present_and_counts_beyond_float32():
    f = np.float32
    C = 3
    cnt = np.zeros(3 * C + 1, np.int64)
    cnt[2 * C] = cnt[C] = cnt[0] = cnt[3 * C] = 100                        # background only
    assert np.array_equal(L.metrics_from_counts(cnt, C, 4, 100), np.array([0, 0, 1], f))
    # inter = 2^24 + 1 and n_pred + n_label = 2^25 + 3 are not float32 numbers: the conversions round them
    C, V = 2, (1 << 24) + 4
    cnt = np.array([1, V - 3, 3, V - 3, 2, V - 2, V - 2], np.int64)
    m = L.metrics_from_counts(cnt, C, 2, V)
    inter, s = f(1 << 24), f((1 << 25) + 4)
    assert f(V - 3) == inter and f(2 * V - 5) == s
    assert m[0] == f(f(inter + f(1e-5)) / f(f(s - inter) + f(1e-5))) and m[1] == f(f(f(2) * inter + f(1e-5)) / f(s + f(1e-5)))
    assert m[2] == f((V - 2) / V)


# ------------------------------------------------------------------------------ allowances
def _families(C):
    """(family, teacher kind or None, cfg) rows: every input family, with and without a teacher."""
    rows = []
    for i, fam in enumerate(L.FAMILIES):
        rows.append((fam, None, L.make_cfg(("combined", "tversky", "ce_tversky", "dice", "combined", "ce_tversky73")[i])))
        rows.append((fam, "extreme" if fam in ("extreme", "ties") else "gauss", L.make_cfg(None, (0.7, 0.3)[i % 2], (2.0, 4.0)[i % 2])))
    return rows


def _torch32(z, lab, cfg, teacher, coef32, go):
    """float32 torch on the CPU: the four sums by F.cross_entropy / F.softmax / F.kl_div, and the gradient by autograd of the
    loss linearised in the sums at the given coefficients (its gradient is the per-voxel formula on `coef`, which is what the
    backward kernel is given)."""
    c = L.cfg32(cfg)
    N, C, V = z.shape
    zt = torch.from_numpy(z).requires_grad_(True)
    lt = torch.from_numpy(lab)
    oh = F.one_hot(lt, C).permute(0, 2, 1).float()
    p = F.softmax(zt, dim=1)
    ce = F.cross_entropy(zt, lt, reduction="sum")
    I, P = (p * oh).sum(dim=(0, 2)), p.sum(dim=(0, 2))
    A, B = torch.from_numpy(coef32[:C].copy()), torch.from_numpy(coef32[L.MAXC:L.MAXC + C].copy())
    lin = float(coef32[2 * L.MAXC]) * ce + (A * I).sum() + (B * P).sum()
    kl = torch.zeros(())
    if c["w_kd"] != 0.0:
        T = c["temperature"]
        kl = F.kl_div(F.log_softmax(zt / T, dim=1), F.softmax(torch.from_numpy(teacher) / T, dim=1), reduction="sum")
        lin = lin + float(coef32[2 * L.MAXC + 1]) * T * kl
    (go * lin).backward()
    return dict(ce=float(ce.detach()), kl=float(kl.detach()), I=I.detach().numpy().astype(np.float64), P=P.detach().numpy().astype(np.float64),
                dlogits=zt.grad.numpy().astype(np.float64))


def _ratios(fam, tk, cfg, C, N, V, seed, k_sum, k_dl):
    z, lab = L.make_inputs(fam, N, C, V, seed)
    teacher = L.make_teacher(tk, N, C, V, seed) if tk else None
    r = L.seg_loss_ref(z, lab, cfg, teacher)
    coef32 = r["coef"].astype(np.float32)
    go = 3.0 if seed % 2 else 0.5
    t = _torch32(z, lab, cfg, teacher, coef32, go)
    sa = L.sum_allowances(z, lab, cfg, teacher, adds=None, k=k_sum)
    out = {"ce": abs(t["ce"] - r["ce_sum"]) / sa["ce"],
           "I": float((np.abs(t["I"] - r["I"]) / sa["I"]).max()), "P": float((np.abs(t["P"] - r["P"]) / sa["P"]).max())}
    if teacher is not None:
        out["kl"] = abs(t["kl"] - r["kl_sum"]) / sa["kl"]
    want = L.dlogits_from_coef(z, lab, coef32, cfg, teacher, go)
    out["dlogits"] = float((np.abs(t["dlogits"] - want) / L.dlogits_allowance(z, lab, coef32, cfg, teacher, go, k=k_dl)).max())
    return out


def test_float32_torch_stays_within_a_quarter_of_every_allowance():
    """The reference's own arithmetic in float32 against float64, on every input family, C in {2, 3, 4, 5, 8}, with and
    without a teacher: inside K / 4 of each allowance (the accumulation term of the sums left out: torch adds in another
    order).  Prints the ratios at K = 1, from which the constants in loss_ref.py were set."""
    worst = {}
    for C in (2, 3, 4, 5, 8):
        for j, (fam, tk, cfg) in enumerate(_families(C)):
            q = _ratios(fam, tk, cfg, C, 2, V0, 1000 * C + j, 1.0, 1.0)
            for name, v in q.items():
                worst[(fam, name)] = max(worst.get((fam, name), 0.0), v)
    for fam in L.FAMILIES:
        print("%-13s" % fam, "  ".join("%s %.4f" % (n, worst.get((fam, n), 0.0)) for n in ("ce", "kl", "I", "P", "dlogits")))
    top_s = max(v for (f, n), v in worst.items() if n != "dlogits")
    top_d = max(v for (f, n), v in worst.items() if n == "dlogits")
    print("largest: sums %.4f  dlogits %.4f   K_SUM %.3g  K_DLOGITS %.3g" % (top_s, top_d, L.K_SUM, L.K_DLOGITS))
    assert top_s <= L.K_SUM / 4 and top_d <= L.K_DLOGITS / 4
    assert top_s >= L.K_SUM / 8 and top_d >= L.K_DLOGITS / 8, "the constants are no longer 4 x what float32 torch needs"


def test_a_perturbed_gradient_is_rejected():
    """One element moved by 8 x its allowance fails the comparison the GPU module makes; the unperturbed float32 one passes."""
    C, N, V = 4, 2, V0
    for fam, tk, cfg in _families(C):
        z, lab = L.make_inputs(fam, N, C, V, 77)
        teacher = L.make_teacher(tk, N, C, V, 77) if tk else None
        coef32 = L.seg_loss_ref(z, lab, cfg, teacher)["coef"].astype(np.float32)
        want = L.dlogits_from_coef(z, lab, coef32, cfg, teacher)
        allow = L.dlogits_allowance(z, lab, coef32, cfg, teacher)
        got = _torch32(z, lab, cfg, teacher, coef32, 1.0)["dlogits"]
        assert (np.abs(got - want) <= allow).all()
        rng = np.random.default_rng(5)
        for _ in range(8):
            idx = tuple(rng.integers(0, s) for s in want.shape)
            bad = got.copy()
            bad[idx] = want[idx] + 8.0 * allow[idx]
            assert not (np.abs(bad - want) <= allow).all()
        assert (allow > 0).all() and np.isfinite(allow).all()


def test_allowances_of_loss_and_coef_follow_the_sums():
    """coef_allowances: a float32-summed (I, P, ce, kl) pushed through the closed forms stays inside the propagated
    allowance; sums moved to the edge of theirs move the Tversky / Dice coefficients by no more than first order predicts."""
    for C in (2, 4, 8):
        for j, (fam, tk, cfg) in enumerate(_families(C)):
            N, V = 2, V0
            z, lab = L.make_inputs(fam, N, C, V, 300 + j)
            teacher = L.make_teacher(tk, N, C, V, 300 + j) if tk else None
            r = L.seg_loss_ref(z, lab, cfg, teacher)
            t = _torch32(z, lab, cfg, teacher, r["coef"].astype(np.float32), 1.0)
            sa = L.sum_allowances(z, lab, cfg, teacher, adds=L.fwd_adds_per_thread(N, V, 4))
            dl, dc = L.coef_allowances(r, sa, N, C, V, cfg)
            loss32, coef32 = L.loss_scalars(t["ce"], t["kl"], t["I"], t["P"], r["T"], N, C, V, L.cfg32(cfg))
            assert abs(loss32 - r["loss"]) <= dl, (fam, C)
            assert (np.abs(coef32 - r["coef"]) <= dc).all(), (fam, C, np.abs(coef32 - r["coef"]) / np.maximum(dc, 1e-300))
            # sums at the edge of their allowances, signs chosen against each other
            for sI, sP in ((1, -1), (-1, 1), (1, 1)):
                _, ce = L.loss_scalars(r["ce_sum"], r["kl_sum"], r["I"] + sI * sa["I"], r["P"] + sP * sa["P"], r["T"], N, C, V, L.cfg32(cfg))
                ok = np.abs(ce - r["coef"])[:16] <= 1.05 * dc[:16] + 1e-300
                assert ok.all(), (fam, C, sI, sP)


def test_fwd_adds_per_thread():
    assert L.fwd_adds_per_thread(2, V0, 4) == 4 and L.fwd_adds_per_thread(2, V0 + 1, 1) == 1
    assert L.fwd_adds_per_thread(64, 17556, 4) == 12                        # 8 blocks per sample: three passes of 8 192 voxels
    assert L.fwd_adds_per_thread(512, 68, 4) == 4 and L.fwd_adds_per_thread(1, 1, 1) == 1
    assert L.fwd_adds_per_thread(64, 17556, 1, threads=1024) == 3           # head + loss: 1024 voxels per workgroup pass
