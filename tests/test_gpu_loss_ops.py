"""Per-operator GPU tests of the loss and metric kernels of csrc/head_loss.hip through the C ABI (_lib.call), each against the
plain float64 references of tests/loss_ref.py (pinned on the CPU by tests/test_loss_ref_cpu.py): mi3d_seg_loss_forward,
mi3d_seg_loss_metrics_forward, mi3d_seg_loss_backward, mi3d_seg_metrics, mi3d_seg_class_counts and the head-fused
mi3d_head_loss_forward / _backward.

Every comparison is an exact equality or goes through an allowance function of loss_ref.py (derivations there; the constants
are 4 x what float32 torch needs on the same inputs).  Integer counts and the three metrics are compared exactly.  Every
output buffer is padded with a sentinel that must survive bitwise.

CASES below is the table of (input family, N x V, pointer offset, C, loss, teacher, upstream gradient) the loss tests run;
the comment on each row names the template instantiation (NC, VV, EXACT, TEACH) of seg_loss_fwd_kernel / seg_loss_bwd_kernel
it selects.  Both forward entry points run on every row (METRICS on and off), and the backward runs every row with V % 4 == 0
on both the vector and the scalar route.

Worst |delta| / allowance measured on an MI355X (the tests print every case with -s):
  forward, loss and coef:  <= 0.64 on every row but 1 x 63 (0.97); the slots that depend on the configuration alone have one float32
                           rounding as their whole allowance, so a ratio near 1 there is a correctly rounded value
  backward, per element:   <= 0.25 on gauss / confident / near_perfect / absent / ties, 0.84 and 0.88 on the two `extreme` rows
                           without a teacher (sigma = 30: the exponential's argument reaches -100 and its error grows with it)
  head + loss:             forward <= 0.63; dz 0.88 ... 0.97 (a correctly rounded bf16 store reaches its half ulp), dW <= 0.03, db <= 0.001
What the tests found in the kernels as they were: with a teacher the vector and the scalar instantiation of seg_loss_bwd_kernel
differed by one ulp in a few elements (row 13), because kd_s (ps - pt) was left to implicit contraction; it is now evaluated as
written (kd_voxel).  mi3d_seg_loss_backward also accepted a distillation weight without teacher logits and silently dropped the term.
Mutation check on the device (each mutant library against this file, first red test): A and B swapped in dlogits_voxel ->
test_seg_loss_backward[00]; kd_s without the factor T -> test_seg_loss_forward[05]; Dice B with (U + eps) unsquared ->
test_seg_loss_forward[00]; `>=` in the argmax of seg_metrics_kernel -> test_seg_metrics_and_class_counts[2], of the fused loss
pass -> test_seg_loss_forward[33]; the ballots of a partly filled wave dropped -> test_seg_loss_forward[00]; inv_t applied to the
student only -> test_seg_loss_forward[05]; eps = 1e-6 in the Dice branch -> test_seg_loss_forward[29]; the scalar route stopping
at V - V % 4 -> test_seg_loss_backward[05].
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as L  # noqa: E402

from multimodal_segmentation_project_amd import _lib  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr  # noqa: E402

DEV = "cuda:0"
SENT = -776.0
PAD = 8                              # sentinel elements on either side of every output
BF16_U = 2.0 ** -8                   # unit roundoff of bfloat16 (8 significant bits)
V0 = 4 * (256 * 3 + 37)              # 3220: four 256-thread blocks of float4 groups, the last wave partly empty


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ccfg(cfg):
    c = _lib.LossCfg()
    c.w_ce, c.region_kind, c.w_reg, c.alpha, c.beta, c.eps, c.w_kd, c.temperature = (
        cfg["w_ce"], cfg["region_kind"], cfg["w_reg"], cfg["alpha"], cfg["beta"], cfg["eps"], cfg["w_kd"], cfg["temperature"])
    return c


class In:
    """A read-only device array whose payload starts `off` elements into the allocation (torch allocations are 512-byte
    aligned: off = 1 takes float32 data off 16 bytes and int64 data off 16 bytes too)."""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a)
        h = np.zeros(a.size + off + 4, a.dtype)
        h[off:off + a.size] = a.ravel()
        self.t = torch.from_numpy(h).to(DEV)
        self.ptr = self.t.data_ptr() + off * a.dtype.itemsize


class Out:
    """A device output [PAD sentinels | off sentinels | n payload | PAD sentinels]; get() checks that only the payload changed."""

    def __init__(self, n, dtype=np.float32, off=0):
        self.dtype, self.lo, self.n = np.dtype(dtype), PAD + off, n
        self.fill = np.full(PAD + off + n + PAD, SENT, np.float32).astype(dtype)
        self.t = torch.from_numpy(self.fill.copy()).to(DEV)
        self.ptr = self.t.data_ptr() + self.lo * self.dtype.itemsize

    def raw(self):
        return self.t.cpu().numpy()

    def untouched(self):
        return np.array_equal(bits(self.raw()), bits(self.fill))

    def get(self):
        h = self.raw()
        out = np.concatenate([h[:self.lo], h[self.lo + self.n:]])
        assert np.array_equal(bits(out), bits(np.concatenate([self.fill[:self.lo], self.fill[self.lo + self.n:]]))), "wrote outside"
        return h[self.lo:self.lo + self.n].copy()


def workspaces(c):
    lib = _lib.lib()
    c = min(max(c, 1), L.MAXC)
    return (torch.empty(lib.mi3d_seg_loss_workspace_bytes(c), dtype=torch.uint8, device=DEV),
            torch.empty(lib.mi3d_seg_metrics_workspace_bytes(c), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ the case table
KD72, KD34 = ("kd", 0.7, 2.0), ("kd", 0.3, 4.0)
A, B_, AM, S63, S1, BIG, WIDE = (2, V0, 0), (2, V0 + 1, 0), (2, V0, 1), (1, 63, 0), (1, 1, 0), (64, 17556, 0), (512, 68, 0)
# (family, (N, V, off), C, loss, teacher kind, grad_out)          instantiation NC, VV, EXACT, TEACH  [what else it reaches]
CASES = [
    ("gauss", A, 2, "combined", None, None),                      # 4 4 - -   (C = 2)
    ("gauss", A, 3, "dice", None, 0.5),                           # 4 4 - -
    ("gauss", A, 4, "tversky", None, None),                       # 4 4 E -
    ("gauss", A, 5, "ce_tversky73", None, 3.0),                   # 8 4 - -
    ("gauss", A, 8, "combined", None, None),                      # 8 4 E -
    ("gauss", B_, 2, KD72, "gauss", None),                        # 4 1 - T   scalar route with a teacher, V % 4 = 1
    ("gauss", B_, 4, KD34, "gauss", 0.5),                         # 4 1 E T
    ("gauss", B_, 5, KD72, "gauss", None),                        # 8 1 - T
    ("gauss", B_, 8, KD34, "extreme", None),                      # 8 1 E T   teacher probabilities underflow: pt > 0 guard
    ("gauss", B_, 3, "ce", None, None),                           # 4 1 - -
    ("gauss", B_, 4, "combined", None, None),                     # 4 1 E -
    ("gauss", B_, 5, "dice", None, None),                         # 8 1 - -
    ("gauss", B_, 8, "tversky", None, 3.0),                       # 8 1 E -
    ("gauss", A, 3, KD72, "gauss", None),                         # 4 4 - T
    ("gauss", A, 4, KD72, "extreme", 3.0),                        # 4 4 E T
    ("gauss", A, 5, KD34, "gauss", None),                         # 8 4 - T
    ("gauss", A, 8, KD72, "gauss", 0.5),                          # 8 4 E T
    ("gauss", AM, 4, "combined", None, None),                     # 4 1 E -   scalar route chosen by alignment, V % 4 == 0
    ("gauss", AM, 8, KD72, "gauss", None),                        # 8 1 E T   the same with a teacher
    ("confident", A, 4, "combined", None, None),                  # 4 4 E -   CE terms log(1 + e^-14)
    ("confident", A, 5, "ce", None, 0.5),                         # 8 4 - -
    ("confident", B_, 2, "ce_tversky73", None, None),             # 4 1 - -
    ("confident", A, 8, KD34, "gauss", None),                     # 8 4 E T
    ("extreme", A, 4, "combined", None, 0.5),                     # 4 4 E -   probabilities flushed to zero
    ("extreme", B_, 8, "tversky", None, None),                    # 8 1 E -
    ("extreme", A, 3, KD72, "extreme", None),                     # 4 4 - T
    ("near_perfect", A, 4, "tversky", None, None),                # 4 4 E -   P - I, T - I cancel
    ("near_perfect", A, 2, "ce_tversky73", None, 3.0),            # 4 4 - -
    ("near_perfect", B_, 5, "tversky", None, None),               # 8 1 - -
    ("absent", A, 4, "dice", None, None),                         # 4 4 E -   B ~ 1/eps for the absent class
    ("absent", A, 8, "combined", None, None),                     # 8 4 E -
    ("absent", B_, 2, "combined", None, None),                    # 4 1 - -   no foreground voxel at all
    ("absent", A, 3, KD72, "gauss", None),                        # 4 4 - T
    ("ties", A, 4, "combined", None, None),                       # 4 4 E -   tied maxima in the fused metric counts
    ("ties", B_, 8, "ce_tversky73", None, None),                  # 8 1 E -
    ("ties", AM, 2, "dice", None, None),                          # 4 1 - -
    ("gauss", S63, 4, "combined", None, None),                    # 4 1 E -   less than one wave
    ("gauss", S1, 3, "combined", None, 3.0),                      # 4 1 - -   one voxel
    ("gauss", S63, 8, KD72, "gauss", None),                       # 8 1 E T
    ("gauss", BIG, 3, "combined", None, None),                    # 4 4 - -   8 blocks per sample: three grid-stride passes, ragged last
    ("ties", BIG, 2, KD72, "gauss", None),                        # 4 4 - T   ballots in the ragged last pass on tied logits
    ("gauss", WIDE, 4, "combined", None, None),                   # 4 4 E -   one block per sample, N at the limit
    ("ties", WIDE, 5, "dice", None, 0.5),                         # 8 4 - -
]
IDS = ["%02d-%s-%dx%d+%d-C%d-%s%s" % (i, c[0], c[1][0], c[1][1], c[1][2], c[2], c[3] if isinstance(c[3], str) else "kd%g" % c[3][1],
                                      "-go%g" % c[5] if c[5] else "") for i, c in enumerate(CASES)]


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Inputs and float64 reference of row i (computed once; the arrays are never written to)."""
    fam, (N, V, off), Cc, loss, tk, go = CASES[i]
    cfg = L.make_cfg(None, loss[1], loss[2]) if isinstance(loss, tuple) else L.make_cfg(loss)
    z, lab = L.make_inputs(fam, N, Cc, V, seed=100 + i)
    teacher = L.make_teacher(tk, N, Cc, V, seed=100 + i) if tk else None
    if fam == "ties":
        assert L.tied_share(z) >= 0.25
    ref = L.seg_loss_ref(z, lab, cfg, teacher)
    return dict(N=N, V=V, off=off, C=Cc, cfg=cfg, z=z, lab=lab, teacher=teacher, go=go, ref=ref, D=(1, 2, Cc, Cc + 3)[i % 4])


def run_forward(z, lab, teacher, cfg, off, metrics, D=0):
    N, Cc, V = z.shape
    zi, li = In(z, off), In(lab, off)
    ti = In(teacher, off) if teacher is not None else None
    loss, coef, met = Out(1), Out(L.NCOEF), Out(3)
    lws, mws = workspaces(Cc)
    if metrics:
        call("mi3d_seg_loss_metrics_forward", zi.ptr, li.ptr, ti.ptr if ti else None, N, Cc, D, V, C.byref(ccfg(cfg)), loss.ptr,
             coef.ptr, met.ptr, ptr(lws), ptr(mws), None)
        return loss.get(), coef.get(), met.get()
    call("mi3d_seg_loss_forward", zi.ptr, li.ptr, ti.ptr if ti else None, N, Cc, V, C.byref(ccfg(cfg)), loss.ptr, coef.ptr, ptr(lws), None)
    assert met.untouched()
    return loss.get(), coef.get(), None


def check_loss_coef(d, loss, coef, adds, what):
    """loss and the 20 coefficients within their allowances; returns the worst |delta| / allowance."""
    ref = d["ref"]
    sa = L.sum_allowances(d["z"], d["lab"], d["cfg"], d["teacher"], adds=adds)
    dl, dc = L.coef_allowances(ref, sa, d["N"], d["C"], d["V"], d["cfg"])
    q = abs(float(loss[0]) - ref["loss"]) / dl
    assert q <= 1.0, f"{what}: loss {float(loss[0])!r} against {ref['loss']!r}: |delta|/allowance {q:.3f}"
    assert bits(loss)[0] == bits(coef)[2 * L.MAXC + 2] and coef[2 * L.MAXC + 3] == 0.0
    delta = np.abs(coef.astype(np.float64) - ref["coef"])
    zero = dc == 0.0
    assert (delta[zero] == 0.0).all(), f"{what}: coef slots that must be exactly zero: {coef[zero]}"
    qc = delta[~zero] / dc[~zero]
    assert (qc <= 1.0).all(), f"{what}: coef |delta|/allowance {qc.max():.3f}\n got {coef}\n ref {ref['coef']}\n allowance {dc}"
    return max(q, float(qc.max()))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_seg_loss_forward(i):
    """mi3d_seg_loss_forward and mi3d_seg_loss_metrics_forward: loss and all 20 coef within the allowances propagated from the
    float32 sums; the two entry points give the same bits; reruns are bitwise equal; the fused metrics equal seg_metrics_ref
    bit for bit (integer counts, then the reference's float32 arithmetic)."""
    d = case_data(i)
    vv = 4 if (d["V"] % 4 == 0 and d["off"] == 0) else 1
    adds = L.fwd_adds_per_thread(d["N"], d["V"], vv)
    l0, c0, _ = run_forward(d["z"], d["lab"], d["teacher"], d["cfg"], d["off"], False)
    l1, c1, m1 = run_forward(d["z"], d["lab"], d["teacher"], d["cfg"], d["off"], True, d["D"])
    l2, c2, m2 = run_forward(d["z"], d["lab"], d["teacher"], d["cfg"], d["off"], True, d["D"])
    q = check_loss_coef(d, l0, c0, adds, IDS[i])
    assert np.array_equal(bits(l0), bits(l1)) and np.array_equal(bits(c0), bits(c1)), "loss-only and loss + metrics entry points differ"
    assert np.array_equal(bits(l1), bits(l2)) and np.array_equal(bits(c1), bits(c2)) and np.array_equal(bits(m1), bits(m2)), "rerun differs"
    want = L.seg_metrics_ref(d["z"], d["lab"], d["D"])
    assert np.array_equal(bits(m1), bits(want)), f"metrics {m1} against {want} (D = {d['D']})"
    print(f"{IDS[i]}: forward worst |delta|/allowance {q:.3f}")


def run_backward(d, coef32, off):
    N, Cc, V = d["z"].shape
    zi, li = In(d["z"], off), In(d["lab"], off)
    ti = In(d["teacher"], off) if d["teacher"] is not None else None
    ci = In(coef32)
    go = torch.tensor([d["go"]], dtype=torch.float32, device=DEV) if d["go"] else None
    out = Out(N * Cc * V, off=off)
    call("mi3d_seg_loss_backward", zi.ptr, li.ptr, ti.ptr if ti else None, N, Cc, V, C.byref(ccfg(d["cfg"])), ci.ptr, ptr(go), out.ptr, None)
    return out.get().reshape(N, Cc, V)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_seg_loss_backward(i):
    """mi3d_seg_loss_backward on the float32-rounded reference coef (so that the per-voxel kernel is isolated from the finalize):
    every element within its allowance; the vector and the scalar route (pointers one element off 16 bytes) give identical
    bits; nothing is written outside dlogits."""
    d = case_data(i)
    coef32 = d["ref"]["coef"].astype(np.float32)
    go = d["go"] or 1.0
    got = run_backward(d, coef32, d["off"])
    want = L.dlogits_from_coef(d["z"], d["lab"], coef32, d["cfg"], d["teacher"], go)
    allow = L.dlogits_allowance(d["z"], d["lab"], coef32, d["cfg"], d["teacher"], go)
    assert np.isfinite(got).all()
    q = np.abs(got.astype(np.float64) - want) / allow
    k = np.unravel_index(int(q.argmax()), q.shape)
    assert (q <= 1.0).all(), (f"{IDS[i]}: {int((q > 1).sum())} of {q.size} elements outside; worst |delta|/allowance {q.max():.3f} at {k}: "
                              f"got {got[k]!r} want {want[k]!r} logits {d['z'][k[0], :, k[2]]} label {d['lab'][k[0], k[2]]}")
    if d["V"] % 4 == 0:
        other = run_backward(d, coef32, 1 - d["off"])
        assert np.array_equal(bits(got), bits(other)), "vector and scalar route differ"
    print(f"{IDS[i]}: backward worst |delta|/allowance {q.max():.3f}")


# ------------------------------------------------------------------------------------------------ metrics and counts
def run_metrics(z, lab, D, off=0):
    N, Cc, V = z.shape
    zi, li = In(z, off), In(lab, off)
    _, mws = workspaces(Cc)
    met, cnt = Out(3), Out(3 * Cc + 1, np.int64)
    call("mi3d_seg_metrics", zi.ptr, li.ptr, N, Cc, D, V, met.ptr, ptr(mws), None)
    call("mi3d_seg_class_counts", zi.ptr, li.ptr, N, Cc, V, cnt.ptr, ptr(mws), None)
    return met.get(), cnt.get()


@pytest.mark.parametrize("Cc", [2, 3, 4, 5, 8])
def test_seg_metrics_and_class_counts(Cc):
    """mi3d_seg_metrics / mi3d_seg_class_counts on every family (tied maxima above all: the first maximum wins, -0.0 == +0.0),
    vector route, V % 4 != 0, misaligned pointers, less than a wave, many samples with a ragged last pass; D in {1, 2, C, C + 3}:
    counts exactly equal, n_correct == sum n_inter, the three metrics bit for bit."""
    k = 0
    for fam in L.FAMILIES:
        shapes = (A, B_, AM, S63)
        if fam in ("gauss", "ties"):                   # 8 blocks per sample: two grid-stride passes, the second ragged
            shapes += ((64, 4 * 2048 + 4 * 77 + 3 * (Cc % 2), 0),)
        for N, V, off in shapes:
            z, lab = L.make_inputs(fam, N, Cc, V, seed=500 + 10 * Cc + k)
            if fam == "ties" and V >= 63:
                assert L.tied_share(z) >= 0.25
            D = (1, 2, Cc, Cc + 3)[k % 4]
            k += 1
            met, cnt = run_metrics(z, lab, D, off)
            want = L.class_counts_ref(z, lab)
            assert np.array_equal(cnt, want), (fam, N, V, off, cnt, want)
            assert cnt[3 * Cc] == cnt[:Cc].sum()
            wm = L.seg_metrics_ref(z, lab, D)
            assert np.array_equal(bits(met), bits(wm)), (fam, N, V, off, D, met, wm)


def test_seg_metrics_no_class_present():
    """Labels all background: no class enters, valid = max(0, 1), iou = dice = 0; accuracy from the counts."""
    for Cc, V in ((2, V0), (5, V0 + 1)):
        z, _ = L.make_inputs("gauss", 2, Cc, V, seed=9)
        lab = np.zeros((2, V), np.int64)
        met, cnt = run_metrics(z, lab, Cc)
        assert np.array_equal(cnt, L.class_counts_ref(z, lab))
        want = L.seg_metrics_ref(z, lab, Cc)
        assert want[0] == 0 and want[1] == 0 and np.array_equal(bits(met), bits(want))


def test_counts_beyond_float32_integers():
    """N = 1, C = 2, V = 2^24 + 4, built on the device: every voxel predicted and labelled class 1 except three, so that
    inter = 2^24 + 1 and n_pred + n_label = 2^25 + 3 are integers float32 cannot hold: the conversions of the finalize round
    them as the reference's .float() does.  Counts exact, the three metrics bit for bit, from all three entry points."""
    V = (1 << 24) + 4
    lg = torch.zeros((1, 2, V), device=DEV)
    lg[0, 1] = 1.0
    lab = torch.ones((1, V), dtype=torch.int64, device=DEV)
    a, b, c = 5, V // 2 + 1, V - 1
    lg[0, 0, [a, b, c]] = 2.0                          # predicted 0 at three voxels
    lab[0, [b, c]] = 0                                 # a: label 1; b, c: label 0
    want_cnt = np.array([2, V - 3, 3, V - 3, 2, V - 2, V - 1], np.int64)
    assert np.float32(want_cnt[1]) != want_cnt[1] and np.float32(want_cnt[3] + want_cnt[5]) != want_cnt[3] + want_cnt[5]
    assert np.array_equal(L.class_counts_ref(lg.cpu().numpy(), lab.cpu().numpy()), want_cnt)
    want = L.metrics_from_counts(want_cnt, 2, 2, V)
    lws, mws = workspaces(2)
    met, cnt, met2, loss, coef = Out(3), Out(7, np.int64), Out(3), Out(1), Out(L.NCOEF)
    call("mi3d_seg_metrics", ptr(lg), ptr(lab), 1, 2, 2, V, met.ptr, ptr(mws), None)
    call("mi3d_seg_class_counts", ptr(lg), ptr(lab), 1, 2, V, cnt.ptr, ptr(mws), None)
    call("mi3d_seg_loss_metrics_forward", ptr(lg), ptr(lab), None, 1, 2, 2, V, C.byref(ccfg(L.make_cfg("combined"))), loss.ptr, coef.ptr,
         met2.ptr, ptr(lws), ptr(mws), None)
    assert np.array_equal(cnt.get(), want_cnt)
    assert np.array_equal(bits(met.get()), bits(want)), (met.get(), want)
    assert np.array_equal(bits(met2.get()), bits(want)), (met2.get(), want)
    assert np.isfinite(loss.get()).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone():
    """N = 513, C = 9, C = 0 and a distillation weight without teacher logits: a negative code, a mi3d_last_error() text, and
    no output buffer written."""
    lib = _lib.lib()
    V = 8
    z = In(np.zeros(513 * 9 * V, np.float32))
    lab = In(np.zeros(513 * V, np.int64))
    coef_in = In(np.zeros(L.NCOEF, np.float32))
    lws, mws = workspaces(L.MAXC)
    plain, kd = ccfg(L.make_cfg("combined")), ccfg(L.make_cfg(None, 0.7, 2.0))

    def refused(rc, outs, what):
        assert rc < 0, (what, rc)
        msg = lib.mi3d_last_error()
        assert msg and len(msg) > 8, what
        for o in outs:
            assert o.untouched(), what
        return msg

    for N, Cc, cfg, what in ((513, 4, plain, "N = 513"), (2, 9, plain, "C = 9"), (2, 0, plain, "C = 0"), (2, 4, kd, "no teacher")):
        loss, coef, met, cnt, dl = Out(1), Out(L.NCOEF), Out(3), Out(28, np.int64), Out(2 * 9 * V)
        rc = lib.mi3d_seg_loss_forward(z.ptr, lab.ptr, None, N, Cc, V, C.byref(cfg), loss.ptr, coef.ptr, ptr(lws), None)
        msg = refused(rc, (loss, coef), "mi3d_seg_loss_forward " + what)
        if what == "C = 9":
            assert b"9" in msg
        rc = lib.mi3d_seg_loss_metrics_forward(z.ptr, lab.ptr, None, N, Cc, 4, V, C.byref(cfg), loss.ptr, coef.ptr, met.ptr, ptr(lws),
                                               ptr(mws), None)
        refused(rc, (loss, coef, met), "mi3d_seg_loss_metrics_forward " + what)
        if what != "no teacher":
            rc = lib.mi3d_seg_metrics(z.ptr, lab.ptr, N, Cc, 4, V, met.ptr, ptr(mws), None)
            refused(rc, (met,), "mi3d_seg_metrics " + what)
            rc = lib.mi3d_seg_class_counts(z.ptr, lab.ptr, N, Cc, V, cnt.ptr, ptr(mws), None)
            refused(rc, (cnt,), "mi3d_seg_class_counts " + what)
        if what != "N = 513":                           # the backward has one block row per sample and no batch limit
            rc = lib.mi3d_seg_loss_backward(z.ptr, lab.ptr, None, N, Cc, V, C.byref(cfg), coef_in.ptr, None, dl.ptr, None)
            refused(rc, (dl,), "mi3d_seg_loss_backward " + what)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ head + loss
def head_inputs(N, V, cin, Cc, seed):
    """Dyadic bf16 activations (k/4), weights (k/8) and bias (k/4): every product is a multiple of 1/32 and the sums stay
    below 2^7, so the float32 logits are exact whatever the order of the multiply-adds."""
    rng = np.random.default_rng(seed)
    zb = rng.integers(-6, 7, size=(N, V, cin)).astype(np.float64) / 4.0
    w = rng.integers(-8, 9, size=(Cc, cin)).astype(np.float64) / 8.0
    b = rng.integers(-4, 5, size=Cc).astype(np.float64) / 4.0
    logits = np.einsum("nvi,ci->ncv", zb, w) + b[None, :, None]
    assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits)
    return zb, w, b, logits


HEAD_CASES = [   # (N, V, Cin, C, loss, teacher kind, D)
    (2, V0, 16, 4, "combined", None, 4),              # EXACT, one pass, last wave partly empty
    (2, V0 + 1, 16, 3, "ce_tversky73", None, 2),      # C < 4, odd V
    (2, V0, 16, 2, KD72, "gauss", 5),                 # TEACH
    (64, 17556, 16, 4, "dice", None, 4),              # 8 workgroups per sample: second trip of the unrolled loop ragged
    (64, 9193, 16, 3, KD34, "gauss", 3),              # the second group of the first trip partly out of range
    (2, V0 + 1, 32, 4, "combined", None, 4),          # Cin = 32: rows read from memory (forward only)
    (3, 1021, 32, 2, KD72, "extreme", 1),
]


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "%dx%d-cin%d-C%d-%s" % (c[0], c[1], c[2], c[3], c[4] if isinstance(c[4], str) else "kd"))
def test_head_loss_against_the_float64_chain(case):
    """mi3d_head_loss_forward / _backward against float64: the kept logits are exact (dyadic inputs), so loss_ref applies to them
    directly.  Loss, coef and metrics as for the unfused entry points.  Backward (Cin = 16) on the reference coef:
      dz   stored bf16: |delta| <= 2^-8 |exact| (half an ulp) + sum_c |w_c| (allow(dl_c) + 2^-8 |dl_c|); the second term is the
           propagated dlogits allowance and the rounding of dlogits to the bf16 operand of the matrix-core product (w is exact);
      dW   |delta| <= sum_v |z| (allow(dl) + 2^-8 |dl|) + M u sum_v |z dl|     (float32 accumulation over M = N V voxels)
      db   |delta| <= sum_v allow(dl) + M u sum_v |dl|                         (dlogits summed unrounded in float32)
    Cin = 32 has no fused backward: mi3d_head_loss_supported says 0 and the call fails with an argument error."""
    N, V, cin, Cc, loss, tk, D = case
    lib = _lib.lib()
    cfg = L.make_cfg(None, loss[1], loss[2]) if isinstance(loss, tuple) else L.make_cfg(loss)
    zb, w, b, logits = head_inputs(N, V, cin, Cc, seed=V + cin + Cc)
    lab = np.random.default_rng(V).integers(0, Cc, size=(N, V)).astype(np.int64)
    teacher = L.make_teacher(tk, N, Cc, V, seed=V) if tk else None
    zt = torch.from_numpy(zb.astype(np.float32)).to(DEV).bfloat16()
    wt, bt = torch.from_numpy(w.astype(np.float32)).to(DEV), torch.from_numpy(b.astype(np.float32)).to(DEV)
    li = In(lab)
    ti = In(teacher) if tk else None
    lws, mws = workspaces(Cc)
    res = []
    for keep in (True, False, True):
        lo, coef, met, kept = Out(1), Out(L.NCOEF), Out(3), Out(N * Cc * V)
        call("mi3d_head_loss_forward", ptr(zt), cin, cin, ptr(wt), ptr(bt), li.ptr, ti.ptr if ti else None, N, Cc, D, V, C.byref(ccfg(cfg)),
             lo.ptr, coef.ptr, met.ptr, ptr(lws), ptr(mws), kept.ptr if keep else None, None)
        if not keep:
            assert kept.untouched()
        res.append((lo.get(), coef.get(), met.get(), kept.get() if keep else None))
    assert np.array_equal(res[0][3].reshape(N, Cc, V).astype(np.float64), logits), "kept logits are not the exact head"
    for r in res[1:]:
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(r[:3], res[0][:3])), "rerun / no kept logits changes the results"
    ref = L.seg_loss_ref(logits, lab, cfg, teacher)
    d = dict(ref=ref, z=logits, lab=lab, cfg=cfg, teacher=teacher, N=N, C=Cc, V=V)
    q = check_loss_coef(d, res[0][0], res[0][1], L.fwd_adds_per_thread(N, V, 1, threads=1024), "head_loss_forward")
    want = L.seg_metrics_ref(logits, lab, D)
    assert np.array_equal(bits(res[0][2]), bits(want)), (res[0][2], want)
    print(f"head forward {case}: worst |delta|/allowance {q:.3f}")

    wsb = lib.mi3d_conv1_workspace_bytes(cin, Cc)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    coef32 = ref["coef"].astype(np.float32)
    ci = In(coef32)
    go = torch.tensor([0.5], device=DEV)
    dzt = torch.full((N * V * cin + 2 * PAD,), SENT, dtype=torch.bfloat16, device=DEV)
    dW, db = Out(Cc * cin), Out(Cc)
    args = (ptr(zt), cin, cin, ptr(wt), ptr(bt), li.ptr, ti.ptr if ti else None, N, Cc, V, C.byref(ccfg(cfg)), ci.ptr, ptr(go),
            dzt.data_ptr() + 2 * PAD, cin, dW.ptr, db.ptr, 0, ptr(ws), wsb, None)
    if cin != 16:
        assert lib.mi3d_head_loss_supported(1, cin, Cc, C.byref(ccfg(cfg))) == 0
        rc = lib.mi3d_head_loss_backward(*args)
        assert rc < 0 and lib.mi3d_last_error(), rc
        torch.cuda.synchronize()
        assert dW.untouched() and db.untouched() and bool((dzt.float() == SENT).all())
        return
    assert lib.mi3d_head_loss_supported(1, cin, Cc, C.byref(ccfg(cfg))) == 1
    call("mi3d_head_loss_backward", *args)
    h = dzt.float().cpu().numpy().astype(np.float64)
    assert (h[:PAD] == SENT).all() and (h[-PAD:] == SENT).all(), "dz: wrote outside"
    gdz = h[PAD:-PAD].reshape(N, V, cin)
    dl = L.dlogits_from_coef(logits, lab, coef32, cfg, teacher, 0.5)
    al = L.dlogits_allowance(logits, lab, coef32, cfg, teacher, 0.5)
    e = al + BF16_U * np.abs(dl)                                        # error of the bf16 operand made from dlogits
    M = float(N * V)
    edz = np.einsum("ncv,ci->nvi", dl, w)
    adz = BF16_U * np.abs(edz) + np.einsum("ncv,ci->nvi", e, np.abs(w)) + L.TINY
    qz = np.abs(gdz - edz) / adz
    assert (qz <= 1.0).all(), f"dz: worst |delta|/allowance {qz.max():.3f}"
    eW = np.einsum("ncv,nvi->ci", dl, zb)
    aW = np.einsum("ncv,nvi->ci", e, np.abs(zb)) + M * L.U * np.einsum("ncv,nvi->ci", np.abs(dl), np.abs(zb))
    qW = np.abs(dW.get().reshape(Cc, cin) - eW) / aW
    eb = dl.sum(axis=(0, 2))
    ab = al.sum(axis=(0, 2)) + M * L.U * np.abs(dl).sum(axis=(0, 2))
    qb = np.abs(db.get() - eb) / ab
    assert (qW <= 1.0).all() and (qb <= 1.0).all(), f"dW {qW.max():.3f} db {qb.max():.3f}"
    print(f"head backward {case}: worst |delta|/allowance dz {qz.max():.3f} dW {qW.max():.3f} db {qb.max():.3f}")
