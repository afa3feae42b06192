"""Pins tests/masked_loss_ref.py (the float64 model of the ignore value behind tests/test_gpu_masked_loss.py and
tests/test_gpu_masked_step.py) on the CPU: against float64 torch autograd with F.cross_entropy(ignore_index=), against
loss_ref.py itself (no voxel ignored: exactly; the compacted valid voxels: to float64 rounding), the documented zeros, the
mutants that the case table has to turn red, the allowances against float32 torch, and the pseudo-label model.

The ratios |float32 torch - float64| / allowance at K = 1 that test_float32_torch_stays_within_a_quarter_of_every_allowance
measures (printed with -s) are tabulated in the docstring of masked_loss_ref.py, with the constants they lead to.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402
import masked_loss_ref as ML  # noqa: E402
from test_loss_ref_cpu import _families  # noqa: E402

V0 = ML.V0


# ------------------------------------------------------------------------------ torch restatements with the mask written out
def t_region(pred, target, ignore, kind, alpha, beta, eps):
    p = F.softmax(pred, dim=1)
    m = (target != ignore).to(pred.dtype)
    out = 0
    for c in range(1, p.size(1)):
        pm, tm = p[:, c] * m, (target == c).to(pred.dtype) * m
        if kind == 1:
            out = out + 1 - (2.0 * (pm * tm).sum() + eps) / (pm.sum() + tm.sum() + eps)
        else:
            tp, fp, fn = (pm * tm).sum(), (pm * (m - tm)).sum(), ((m - pm) * tm).sum()
            out = out + 1 - (tp + eps) / (tp + alpha * fp + beta * fn + eps)
    return out / (p.size(1) - 1)


def t_masked_loss(cfg, pred, target, ignore, teacher=None):
    """The loss family of a configuration dict (decimal constants) with torch's ignore_index on CE, the mask on the region sums
    and the distillation term of test_loss_ref_cpu.py over every voxel."""
    out = 0
    if cfg["w_ce"] != 0.0:
        # F.cross_entropy needs the ignored target outside the gather only when it is out of range: it accepts any ignore_index
        out = out + cfg["w_ce"] * F.cross_entropy(pred, target, ignore_index=ignore, reduction="mean")
    if cfg["region_kind"] != 0 and pred.size(1) > 1:
        out = out + cfg["w_reg"] * t_region(pred, target, ignore, cfg["region_kind"], cfg["alpha"], cfg["beta"], cfg["eps"])
    if cfg["w_kd"] != 0.0:
        T = cfg["temperature"]
        kl = F.kl_div(F.log_softmax(pred / T, dim=1), F.softmax(teacher / T, dim=1), reduction="none").mean() * T ** 2
        out = out + cfg["w_kd"] * kl
    return out


CFGS = [("combined", None), ("dice", None), ("tversky", None), ("ce_tversky73", None), ("ce", None), (None, (0.7, 2.0)), (None, (0.3, 4.0))]


def _cfg(name, kd):
    return L.make_cfg(None, kd[0], kd[1]) if kd else L.make_cfg(name)


def _torch_safe_target(lab, ignore, C):
    """torch's cross_entropy asserts 0 <= t < C for targets that are not ignore_index; the model's labels satisfy that."""
    return torch.from_numpy(lab)


@pytest.mark.parametrize("mask", ML.MASKS)
@pytest.mark.parametrize("family", ["gauss", "near_perfect", "absent"])
def test_loss_and_gradient_against_float64_autograd(family, mask):
    """Every (input family, mask family, loss kind, teacher) combination, C and ignore_index walking through their values:
    loss and dlogits against float64 autograd."""
    k = 0
    for name, kd in CFGS:
        for C in (2, 3, 4, 5, 8):
            ignore = ML.ignore_value(ML.IGNORES[k % len(ML.IGNORES)], C)
            k += 1
            N, V = 2, 331
            z, lab = L.make_inputs(family, N, C, V, seed=10 * C + k)
            lab = ML.apply_mask(lab, ML.make_mask(mask, lab, C, seed=k), ignore)
            teacher = L.make_teacher("gauss", N, C, V, seed=C)
            cfg = dict(_cfg(name, kd), exact=True)
            r = ML.masked_loss_ref(z, lab, cfg, ignore, teacher if kd else None)
            if r["M_valid"] == 0 and cfg["w_ce"] != 0.0:
                continue                               # torch returns NaN there: test_all_ignored_gives_the_documented_zeros
            zt = torch.from_numpy(z).double().requires_grad_(True)
            l = t_masked_loss(cfg, zt, _torch_safe_target(lab, ignore, C), ignore, torch.from_numpy(teacher).double())
            if not torch.is_tensor(l) or not l.requires_grad:
                assert r["loss"] == 0.0 and not r["dlogits"].any()
                continue
            l.backward()
            g = zt.grad.numpy()
            what = (name, kd, C, family, mask, ignore)
            assert abs(r["loss"] - l.item()) <= 1e-12 * max(abs(l.item()), 1e-3), what
            d = np.abs(r["dlogits"] - g)
            assert np.linalg.norm(d) <= 1e-12 * max(np.linalg.norm(g), 1e-9), what
            assert (d <= 1e-12 * np.abs(g) + 1e-12 * np.linalg.norm(g) / np.sqrt(g.size) + 1e-300).all(), what
            assert r["loss"] == r["coef"][2 * L.MAXC + 2] and r["coef"][2 * L.MAXC + 3] == 0.0


def test_no_voxel_ignored_is_loss_ref_exactly():
    for j, (name, kd) in enumerate(CFGS):
        for C in (2, 4, 8):
            z, lab = L.make_inputs("gauss", 2, C, 257, seed=j)
            teacher = L.make_teacher("gauss", 2, C, 257, seed=j) if kd else None
            cfg = _cfg(name, kd)
            a, b = ML.masked_loss_ref(z, lab, cfg, 255, teacher), L.seg_loss_ref(z, lab, cfg, teacher)
            assert a["loss"] == b["loss"] and np.array_equal(a["coef"], b["coef"]) and np.array_equal(a["dlogits"], b["dlogits"])
            for key in ("I", "P", "T"):
                assert np.array_equal(a[key], b[key])
            assert np.array_equal(ML.masked_counts_ref(z, lab, 255), L.class_counts_ref(z, lab))
            assert np.array_equal(ML.masked_metrics_ref(z, lab, 255, 3).view(np.uint32), L.seg_metrics_ref(z, lab, 3).view(np.uint32))
            c32 = b["coef"].astype(np.float32)
            assert np.array_equal(ML.masked_dlogits_allowance(z, lab, c32, cfg, 255, teacher, k=L.K_DLOGITS), L.dlogits_allowance(z, lab, c32, cfg, teacher))


@pytest.mark.parametrize("mask", ["random30", "runs", "sample", "class", "all_but_one"])
def test_without_a_teacher_it_is_loss_ref_on_the_compacted_voxels(mask):
    for j, (name, kd) in enumerate(CFGS[:5]):
        C = (2, 3, 4, 5, 8)[j]
        ignore = ML.ignore_value(ML.IGNORES[j], C)
        z, lab = L.make_inputs("gauss", 2, C, 1021, seed=j)
        lab = ML.apply_mask(lab, ML.make_mask(mask, lab, C, seed=j), ignore)
        m = lab != ignore
        cfg = _cfg(name, kd)
        a = ML.masked_loss_ref(z, lab, cfg, ignore)
        zc, lc = np.ascontiguousarray(z.transpose(1, 0, 2)[:, m])[None], lab[m][None]
        b = L.seg_loss_ref(zc, lc, cfg)
        assert a["M_valid"] == lc.size
        assert abs(a["loss"] - b["loss"]) <= 1e-13 * max(abs(b["loss"]), 1.0)
        np.testing.assert_allclose(a["coef"], b["coef"], rtol=1e-12, atol=1e-300)
        dc = a["dlogits"].transpose(1, 0, 2)[:, m][None]
        np.testing.assert_allclose(dc, b["dlogits"], rtol=1e-10, atol=1e-18)
        assert not a["dlogits"].transpose(1, 0, 2)[:, ~m].any()                     # zero where ignored
        cnt = ML.masked_counts_ref(z, lab, ignore)
        assert np.array_equal(cnt, L.class_counts_ref(zc, lc))
        assert np.array_equal(ML.masked_metrics_ref(z, lab, ignore, 4).view(np.uint32), L.seg_metrics_ref(zc, lc, 4).view(np.uint32))


def test_all_ignored_gives_the_documented_zeros():
    C = 4
    z, lab = L.make_inputs("gauss", 2, C, 97, seed=3)
    teacher = L.make_teacher("gauss", 2, C, 97, seed=3)
    lab[:] = 255
    r = ML.masked_loss_ref(z, lab, L.make_cfg("combined"), 255)
    # CE mean 0; every region term is 1 - eps / eps = 0; ce_s = 0; no gradient
    assert r["M_valid"] == 0 and r["loss"] == 0.0 and r["coef"][2 * L.MAXC] == 0.0 and not r["dlogits"].any()
    assert not ML.masked_counts_ref(z, lab, 255).any()
    assert np.array_equal(ML.masked_metrics_ref(z, lab, 255, 4), np.zeros(3, np.float32))
    cfg = L.make_cfg(None, 0.7, 2.0)
    k = ML.masked_loss_ref(z, lab, cfg, 255, teacher)
    full = L.seg_loss_ref(z, np.zeros_like(lab), cfg, teacher)
    c = L.cfg32(cfg)
    kd_term = c["w_kd"] * c["temperature"] ** 2 * full["kl_sum"] / (2 * 97 * C)
    assert k["loss"] == kd_term > 0 and k["dlogits"].any()
    want = L.dlogits_from_coef(z, lab, ML._kd_only(k["coef"]), cfg, teacher)
    assert np.array_equal(k["dlogits"], want)


# ------------------------------------------------------------------------------ mutants
def _detects(i, mutant):
    """Does row i of the case table tell the mutant from the model, by the comparisons tests/test_gpu_masked_loss.py makes?"""
    d = ML.case_inputs(i)
    z, lab, cfg, ig, tch = d["z"], d["lab"], d["cfg"], d["ignore"], d["teacher"]
    if mutant in ("n_pred_counts_ignored", "acc_over_nv"):
        a, b = ML.masked_metrics_ref(z, lab, ig, d["D"]), ML.masked_metrics_ref(z, lab, ig, d["D"], mutant)
        return (not np.array_equal(ML.masked_counts_ref(z, lab, ig), ML.masked_counts_ref(z, lab, ig, mutant))
                or not np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    ref, bad = ML.masked_loss_ref(z, lab, cfg, ig, tch), ML.masked_loss_ref(z, lab, cfg, ig, tch, mutant)
    vv = 4 if (d["V"] % 4 == 0 and d["off"] == 0) else 1
    sa = ML.masked_sum_allowances(z, lab, cfg, ig, tch, adds=L.fwd_adds_per_thread(d["N"], d["V"], vv))
    dl, dc = ML.masked_coef_allowances(ref, sa, d["N"], d["C"], d["V"], cfg)
    if abs(bad["loss"] - ref["loss"]) > 2 * dl or (np.abs(bad["coef"] - ref["coef"]) > 2 * dc).any():
        return True
    coef32 = ref["coef"].astype(np.float32)
    go = d["go"] or 1.0
    want = ML.masked_dlogits_from_coef(z, lab, coef32, cfg, ig, tch, go)
    got = ML.masked_dlogits_from_coef(z, lab, coef32, cfg, ig, tch, go, mutant)
    return bool((np.abs(got - want) > 2 * ML.masked_dlogits_allowance(z, lab, coef32, cfg, ig, tch, go)).any())


@pytest.mark.parametrize("mutant", ML.MUTANTS)
def test_the_case_table_turns_every_mutant_red(mutant):
    """Each wrong reading of the contract differs from the model by more than twice the allowance (or in an exact count / a
    metric bit) on at least one row of the GPU test's table."""
    rows = [i for i in range(len(ML.CASES)) if ML.CASES[i][1][0] * ML.CASES[i][1][1] <= 2 * (V0 + 1)]       # the small rows suffice
    red = [i for i in rows if _detects(i, mutant)]
    print(mutant, "red on rows", red)
    assert red, mutant


def test_the_model_passes_its_own_comparisons():
    for i in range(0, len(ML.CASES), 5):
        if ML.CASES[i][1][0] == 64:
            continue
        assert not _detects(i, None)


# ------------------------------------------------------------------------------ allowances against float32 torch
def _torch32_masked(z, lab, ignore, cfg, teacher, coef32, go):
    """test_loss_ref_cpu._torch32 with the mask: the four sums in float32 torch (CE by F.cross_entropy(ignore_index=)), and the
    gradient by autograd of the loss linearised in the sums at the given coefficients."""
    c = L.cfg32(cfg)
    N, C, V = z.shape
    zt = torch.from_numpy(z).requires_grad_(True)
    lt = torch.from_numpy(lab)
    m = (lt != ignore)
    oh = (F.one_hot(torch.where(m, lt, torch.zeros_like(lt)).clamp(0, C - 1), C).permute(0, 2, 1) * m[:, None, :]).float()
    p = F.softmax(zt, dim=1)
    ce = F.cross_entropy(zt, lt, ignore_index=ignore, reduction="sum")
    I, P = (p * oh).sum(dim=(0, 2)), (p * m[:, None, :].float()).sum(dim=(0, 2))
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


def _q(delta, allow):
    """max |delta| / allowance; a zero allowance demands a zero delta."""
    delta, allow = np.atleast_1d(np.abs(delta)), np.atleast_1d(allow)
    assert (delta[allow == 0.0] == 0.0).all()
    nz = allow > 0.0
    return float((delta[nz] / allow[nz]).max()) if nz.any() else 0.0


def test_float32_torch_stays_within_a_quarter_of_every_allowance():
    """The allowance rule of loss_ref.py re-run on the masked inputs: float32 torch inside K / 4 of every allowance for every
    mask family (the accumulation term left out: adds=None).  Prints the ratios at K = 1 (module docstring)."""
    worst = {}
    for C in (2, 3, 4, 5, 8):
        for j, (fam, tk, cfg) in enumerate(_families(C)):
            for mi, mask in enumerate(ML.MASKS):
                seed = 1000 * C + j
                ignore = ML.ignore_value(ML.IGNORES[(j + mi) % len(ML.IGNORES)], C)
                z, lab = L.make_inputs(fam, 2, C, V0, seed)
                lab = ML.apply_mask(lab, ML.make_mask(mask, lab, C, seed), ignore)
                teacher = L.make_teacher(tk, 2, C, V0, seed) if tk else None
                r = ML.masked_loss_ref(z, lab, cfg, ignore, teacher)
                coef32 = r["coef"].astype(np.float32)
                go = 3.0 if seed % 2 else 0.5
                t = _torch32_masked(z, lab, ignore, cfg, teacher, coef32, go)
                sa = ML.masked_sum_allowances(z, lab, cfg, ignore, teacher, adds=None, k=1.0)
                q = {"ce": _q(t["ce"] - r["ce_sum"], sa["ce"]), "I": _q(t["I"] - r["I"], sa["I"]), "P": _q(t["P"] - r["P"], sa["P"])}
                if teacher is not None:
                    q["kl"] = _q(t["kl"] - r["kl_sum"], sa["kl"])
                want = ML.masked_dlogits_from_coef(z, lab, coef32, cfg, ignore, teacher, go)
                al = ML.masked_dlogits_allowance(z, lab, coef32, cfg, ignore, teacher, go, k=1.0, k_ignored=1.0)
                m3 = np.broadcast_to((lab != ignore)[:, None, :], want.shape)
                q["dlogits"] = _q((t["dlogits"] - want)[m3], al[m3])
                q["ignored"] = _q((t["dlogits"] - want)[~m3], al[~m3])
                for name, v in q.items():
                    worst[(mask, name)] = max(worst.get((mask, name), 0.0), v)
    for mask in ML.MASKS:
        print("%-13s" % mask, "  ".join("%s %.4f" % (n, worst.get((mask, n), 0.0)) for n in ("ce", "kl", "I", "P", "dlogits", "ignored")))
    top_s = max(v for (f, n), v in worst.items() if n not in ("dlogits", "ignored"))
    top_d = max(v for (f, n), v in worst.items() if n == "dlogits")
    top_i = max(v for (f, n), v in worst.items() if n == "ignored")
    print("largest: sums %.4f  dlogits %.4f  at ignored voxels %.4f   K_SUM %.3g  K_DLOGITS %.3g  K_DLOGITS_IGNORED %.3g"
          % (top_s, top_d, top_i, ML.K_SUM, ML.K_DLOGITS, ML.K_DLOGITS_IGNORED))
    assert top_s <= ML.K_SUM / 4 and top_d <= ML.K_DLOGITS / 4 and top_i <= ML.K_DLOGITS_IGNORED / 4
    assert top_d >= ML.K_DLOGITS / 8 and top_i >= ML.K_DLOGITS_IGNORED / 8, "the constants are no longer 4 x what float32 torch needs"


# ------------------------------------------------------------------------------ mask families and pseudo-labels
def test_mask_families():
    lab = np.random.default_rng(0).integers(0, 4, size=(2, V0)).astype(np.int64)
    assert not ML.make_mask("none", lab, 4, 1).any() and ML.make_mask("all", lab, 4, 1).all()
    assert abs(ML.make_mask("random30", lab, 4, 1).mean() - 0.3) < 0.03
    assert ML.make_mask("all_but_one", lab, 4, 1).sum() == lab.size - 1
    s = ML.make_mask("sample", lab, 4, 1)
    assert s[0].all() and not s[1].any()
    assert np.array_equal(ML.make_mask("class", lab, 4, 1), lab == 1)
    r = ML.make_mask("runs", lab, 4, 1)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], r[0].astype(np.int8), [0]])))
    starts, ends = edges[0::2], edges[1::2]
    assert (ends - starts >= 64).all() and (starts % 64 == 0).any() and (starts % 64 != 0).any()
    waves = r[0][:V0 // 64 * 64].reshape(-1, 64)
    assert waves.all(axis=1).any() and r[0][:V0 // 4 * 4].reshape(-1, 4).all(axis=1).any()      # whole waves, whole float4 groups


def test_pseudo_label_model():
    lab = np.array([[0, 1, 2, 3, 1, 1, 7, 2]], np.uint8)
    conf = np.array([[0.5, 0.9, np.nan, 1.0, 0.89999, 0.95, 1.0, 0.0]], np.float32)
    tgt, tab = ML.pseudo_labels_ref(lab, conf, [0.0, 0.9, 0.0, 1.0], 255)
    assert tgt.dtype == np.int64 and tab.dtype == np.int64
    assert tgt.tolist() == [[0, 1, 255, 3, 255, 1, 255, 2]]        # NaN and a label past C are ignored; at the threshold is kept
    assert tab.tolist() == [[1, 2, 1, 1, 3]] and tab.sum() == lab.size
