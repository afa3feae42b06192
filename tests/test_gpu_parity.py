"""GPU parity tests: the HIP path (through the C ABI) vs golden vectors from the reference and vs the CPU oracle.

Tolerances: fp32 path = kernels accumulate in fp32 in a different order than torch's CPU kernels, so
1e-4-class relative tolerances; bf16 path = activations stored in bf16 (8 significant bits), compared with
norm-relative tolerances per tensor (SURVEY §7 hard part 9) and Dice within 1e-3 (BASELINE north_star).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multimodal_segmentation_project_amd as mi
from multimodal_segmentation_project_amd import metrics as M
from multimodal_segmentation_project_amd import unet_dann
from multimodal_segmentation_project_amd.dann import DomainDiscriminator, domain_ce, grad_reverse
from multimodal_segmentation_project_amd.unet import DoubleConv, UNet3D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_ref import assert_bf16_rne_bits  # noqa: E402

DEV = "cuda:0"
LOSS_CASES = ["uniform", "absent2", "single0", "onehot", "c3_noncubic"]


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load_sd(mod, g, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}
    mod.load_state_dict(sd, strict=True)


# ------------------------------------------------------------------------------------------------ per-op
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 3e-2)])
def test_doubleconv_golden(golden, dtype, tol):
    """Stand-alone DoubleConv (conv3/BN/ReLU fwd+bwd per-op entry points), odd channels 3->5, volume 6x5x7."""
    g = golden("doubleconv")
    m = DoubleConv(3, 5, dropout_rate=0.0)
    load_sd(m, g, "sd0/")
    m = m.to(DEV).train()
    m.compute_dtype = dtype
    x = t(g["x"]).requires_grad_(True)
    out = m(x)
    out.backward(t(g["go"]))
    assert relerr(out.detach().cpu(), g["out"]) < tol
    assert relerr(x.grad.cpu(), g["gx"]) < 3 * tol
    for k, p in m.named_parameters():
        ref = g["grad/" + k]
        if np.abs(ref).max() < 1e-4:        # conv bias in front of train-mode BN: analytically zero
            # bf16: the sum of bf16-rounded dy is rounding noise of size ~2^-9*|dy|*sqrt(M), not a parity quantity
            assert p.grad.abs().max().item() < (1e-3 if dtype == torch.float32 else 0.5)
        else:
            assert relerr(p.grad.cpu(), ref) < 5 * tol, k
    sd = m.state_dict()
    for k in ("double_conv.1.running_mean", "double_conv.5.running_var", "double_conv.1.running_var"):
        assert relerr(sd[k].cpu(), g["sd1/" + k]) < max(tol, 1e-5), k
    assert int(sd["double_conv.1.num_batches_tracked"]) == 1


def test_conv_bn_pool_upconv_vs_c_oracle(orc):
    """fp32 per-op entry points vs the C oracle on ragged shapes (non-multiple-of-tile sizes, odd channels)."""
    import ctypes as C
    from multimodal_segmentation_project_amd import _lib
    from multimodal_segmentation_project_amd._lib import call, ptr
    rng = np.random.default_rng(0)
    s = None
    for (n, cin, cout, d, h, w) in [(1, 1, 16, 9, 10, 11), (2, 16, 16, 5, 9, 17), (1, 24, 8, 4, 4, 4), (2, 3, 5, 6, 5, 7),
                                    (1, 32, 48, 4, 6, 8)]:
        x = rng.standard_normal((n, cin, d, h, w), dtype=np.float32)
        wgt = (rng.standard_normal((cout, cin, 3, 3, 3), dtype=np.float32) * 0.2)
        b = rng.standard_normal(cout).astype(np.float32)
        gy = rng.standard_normal((n, cout, d, h, w), dtype=np.float32)
        xcl = t(x.transpose(0, 2, 3, 4, 1))
        gcl = t(gy.transpose(0, 2, 3, 4, 1))
        wd, bd = t(wgt), t(b)          # keep alive: launches are asynchronous
        wsb = _lib.lib().mi3d_conv3_workspace_bytes(cin, cout, n, d, h, w)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        y = torch.empty((n, d, h, w, cout), device=DEV)
        call("mi3d_conv3_forward", 0, 0, ptr(xcl), cin, cin, ptr(wd), ptr(bd), ptr(y), cout, cout, n, d, h, w,
             ptr(ws), wsb, s)
        ref = orc.conv3d_fwd(x, wgt, b)
        np.testing.assert_allclose(y.cpu().numpy().transpose(0, 4, 1, 2, 3), ref, rtol=2e-4, atol=2e-4)
        dx = torch.empty_like(xcl)
        dW = torch.empty((cout, cin, 3, 3, 3), device=DEV)
        db = torch.empty(cout, device=DEV)
        call("mi3d_conv3_backward", 0, 0, ptr(xcl), cin, cin, ptr(wd), ptr(gcl), cout, cout, ptr(dx), cin, ptr(dW),
             ptr(db), 0, n, d, h, w, ptr(ws), wsb, s)
        rgx, rgw, rgb = orc.conv3d_bwd(x, wgt, gy)
        np.testing.assert_allclose(dx.cpu().numpy().transpose(0, 4, 1, 2, 3), rgx, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(dW.cpu().numpy(), rgw, rtol=2e-4, atol=5e-4)
        np.testing.assert_allclose(db.cpu().numpy(), rgb, rtol=2e-4, atol=5e-4)
    # maxpool with ties + skip add, and upconv
    x = rng.integers(0, 3, (2, 8, 4, 6, 4)).astype(np.float32)
    gp = rng.standard_normal((2, 8, 2, 3, 2), dtype=np.float32)
    sk = rng.standard_normal(x.shape, dtype=np.float32)
    xcl, gpcl, skcl = t(x.transpose(0, 2, 3, 4, 1)), t(gp.transpose(0, 2, 3, 4, 1)), t(sk.transpose(0, 2, 3, 4, 1))
    p = torch.empty((2, 2, 3, 2, 8), device=DEV)
    call("mi3d_maxpool2_forward", 0, ptr(xcl), 8, 8, 2, 4, 6, 4, ptr(p), 8, s)
    np.testing.assert_array_equal(p.cpu().numpy().transpose(0, 4, 1, 2, 3), orc.maxpool2_fwd(x))
    dz = torch.empty_like(xcl)
    call("mi3d_maxpool2_backward", 0, ptr(gpcl), 8, ptr(xcl), 8, ptr(skcl), 8, ptr(dz), 8, 8, 2, 4, 6, 4, s)
    np.testing.assert_allclose(dz.cpu().numpy().transpose(0, 4, 1, 2, 3), orc.maxpool2_bwd(x, gp) + sk, atol=1e-6)
    for (n, cin, cout, d, h, w) in [(2, 6, 3, 3, 2, 4), (1, 32, 16, 2, 3, 2)]:
        x = rng.standard_normal((n, cin, d, h, w), dtype=np.float32)
        wgt = rng.standard_normal((cin, cout, 2, 2, 2), dtype=np.float32) * 0.3
        b = rng.standard_normal(cout).astype(np.float32)
        gy = rng.standard_normal((n, cout, 2 * d, 2 * h, 2 * w), dtype=np.float32)
        xcl, gcl = t(x.transpose(0, 2, 3, 4, 1)), t(gy.transpose(0, 2, 3, 4, 1))
        wd, bd = t(wgt), t(b)
        wsb = _lib.lib().mi3d_upconv2_workspace_bytes(cin, cout, n, d, h, w)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        y = torch.empty((n, 2 * d, 2 * h, 2 * w, cout), device=DEV)
        call("mi3d_upconv2_forward", 0, ptr(xcl), cin, cin, ptr(wd), ptr(bd), ptr(y), cout, cout, n, d, h, w,
             ptr(ws), wsb, s)
        np.testing.assert_allclose(y.cpu().numpy().transpose(0, 4, 1, 2, 3), orc.convT2_fwd(x, wgt, b), rtol=2e-4, atol=2e-4)
        dx, dW, db = torch.empty_like(xcl), torch.empty((cin, cout, 2, 2, 2), device=DEV), torch.empty(cout, device=DEV)
        call("mi3d_upconv2_backward", 0, ptr(xcl), cin, cin, ptr(wd), ptr(gcl), cout, cout, ptr(dx), cin, ptr(dW),
             ptr(db), 0, n, d, h, w, ptr(ws), wsb, s)
        rgx, rgw, rgb = orc.convT2_bwd(x, wgt, gy)
        np.testing.assert_allclose(dx.cpu().numpy().transpose(0, 4, 1, 2, 3), rgx, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(dW.cpu().numpy(), rgw, rtol=2e-4, atol=5e-4)
        np.testing.assert_allclose(db.cpu().numpy(), rgb, rtol=2e-4, atol=5e-4)


# ------------------------------------------------------------------------------------------ losses / metrics
@pytest.mark.parametrize("case", LOSS_CASES)
def test_losses_golden(golden, case):
    g = golden("losses_metrics")
    fns = {
        "combined": M.combined_loss,
        "default_fn": M.get_loss_fn("anything"),
        "tversky55": lambda p, y: M.tversky_loss(p, y, alpha=0.5, beta=0.5),
        "tversky_fn": M.get_loss_fn("tversky"),
        "ce_tversky73": M.combined_ce_tversky_loss,
        "ce_tversky55": M.get_loss_fn("ce_tversky"),
        "dice": M.get_loss_fn("dice"),
    }
    lb = t(g[f"{case}/labels"])
    for name, fn in fns.items():
        z = t(g[f"{case}/logits"]).requires_grad_(True)
        l = fn(z, lb)
        l.backward()
        np.testing.assert_allclose(l.item(), g[f"{case}/{name}/loss"], rtol=2e-5, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(z.grad.cpu().numpy(), g[f"{case}/{name}/grad"], rtol=2e-3, atol=3e-7, err_msg=name)
    for alpha, temp in ((0.7, 2.0), (0.3, 4.0)):
        z = t(g[f"{case}/logits"]).requires_grad_(True)
        l = M.distillation_loss(z, t(g[f"{case}/teacher"]), lb, alpha, temp)
        (3.0 * l).backward()        # upstream gradient scaling goes through the device-scalar grad_out
        np.testing.assert_allclose(l.item(), g[f"{case}/distill_a{alpha}_t{temp}/loss"], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(z.grad.cpu().numpy() / 3.0, g[f"{case}/distill_a{alpha}_t{temp}/grad"], rtol=2e-3, atol=3e-7)


@pytest.mark.parametrize("case", LOSS_CASES + ["q1_d2", "nofg"])
def test_metrics_golden(golden, case):
    g = golden("losses_metrics")
    lg, lb = t(g[f"{case}/logits"]), t(g[f"{case}/labels"])
    np.testing.assert_allclose(float(M.calculate_iou(lg, lb)), g[f"{case}/calculate_iou"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(float(M.calculate_dice(lg, lb)), g[f"{case}/calculate_dice"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(float(M.calculate_accuracy(lg, lb)), g[f"{case}/calculate_accuracy"], rtol=1e-6, atol=1e-7)


def test_loss_metrics_vs_oracle_large(orc):
    """64^3 N=2 random logits: HIP loss/grad/metric counts vs the C oracle (two-stage reductions at scale)."""
    gen = torch.Generator().manual_seed(3)
    lg = 3.0 * torch.randn(2, 4, 64, 64, 64, generator=gen)
    lb = torch.randint(0, 4, (2, 1, 64, 64, 64), generator=gen)
    z = lg.to(DEV).requires_grad_(True)
    l = M.combined_loss(z, lb.to(DEV))
    l.backward()
    ref_l, ref_g = orc.seg_loss(lg.numpy(), lb.numpy(), "combined")
    np.testing.assert_allclose(l.item(), ref_l, rtol=1e-5)
    assert relerr(z.grad.cpu(), ref_g) < 1e-4
    m = orc.seg_metrics(lg.numpy(), lb.numpy())
    out = M.calculate_all(lg.to(DEV), lb.to(DEV)).cpu().numpy()
    np.testing.assert_allclose(out, [m["iou"], m["dice"], m["acc"]], rtol=1e-6)


# ------------------------------------------------------------------------------------------------ whole net
# test_small_unet_golden_fp32's rule for "equals the golden fixture" on the fp32 path
SMALL_LOGITS_TOL = dict(rtol=1e-3, atol=2e-4)
SMALL_LOSS_RTOL = 1e-5
SMALL_GRAD_ZERO, SMALL_GRAD_ZERO_TOL, SMALL_GRAD_TOL = 1e-5, 1e-4, 2e-3      # a gradient that is analytically zero / any other, norm-relative
SMALL_BN_TOL = dict(rtol=1e-4, atol=1e-5)


def test_small_unet_golden_fp32(golden):
    """Complete fixture: every weight, every gradient, BN buffers, eval logits (2 levels, odd channels, 8x12x4)."""
    g = golden("small_unet")
    m = UNet3D(in_channels=2, out_channels=3, features=[4, 8], dropout_rate=0.0)
    load_sd(m, g, "sd0/")
    m = m.to(DEV).train()
    m.compute_dtype = torch.float32
    x, y = t(g["x"]), t(g["y"])
    logits = m(x)
    loss = M.combined_loss(logits, y)
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits"], **SMALL_LOGITS_TOL)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=SMALL_LOSS_RTOL)
    for k, p in m.named_parameters():
        ref = g["grad/" + k]
        if np.abs(ref).max() < SMALL_GRAD_ZERO:
            assert p.grad.abs().max().item() < SMALL_GRAD_ZERO_TOL, k
        else:
            assert relerr(p.grad.cpu(), ref) < SMALL_GRAD_TOL, (k, relerr(p.grad.cpu(), ref))
    sd = m.state_dict()
    for k, v in g.items():
        if k.startswith("sd1/"):
            np.testing.assert_allclose(sd[k[4:]].cpu().numpy(), v, err_msg=k, **SMALL_BN_TOL)
    m.eval()
    with torch.no_grad():
        le = m(x)
    np.testing.assert_allclose(le.cpu().numpy(), g["logits_eval"], **SMALL_LOGITS_TOL)


def _default_model(cls=UNet3D, seed=0):
    torch.manual_seed(seed)
    return cls(in_channels=1, out_channels=4, dropout_rate=0.0)


def _synth(n, s, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 1, s, s, s, generator=gen)
    y = torch.randint(0, 4, (n, 1, s, s, s), generator=gen)
    return x, y


@pytest.mark.parametrize("tag,n,s", [("s16n2", 2, 16), ("s32n1", 1, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_default_unet_golden(golden, tag, n, s, dtype):
    """The 5.65 M-parameter default net from the reference's seeded init: logits, loss, metrics, all grad norms."""
    g = golden("default_unet")
    m = _default_model().to(DEV).train()
    m.compute_dtype = dtype
    x, y = _synth(n, s, 1234)
    x, y = x.to(DEV), y.to(DEV)
    logits = m(x)
    loss = M.combined_loss(logits, y)
    loss.backward()
    fp32 = dtype == torch.float32
    assert relerr(logits.detach().cpu(), g[f"{tag}/logits"]) < (2e-4 if fp32 else 1.5 * float(g[f"{tag}/autocast_bf16/logits_relerr"]))
    np.testing.assert_allclose(loss.item(), g[f"{tag}/loss"], rtol=2e-5 if fp32 else 2e-3)
    # Dice within 1e-3 of the reference (BASELINE north_star); fp32: tight
    assert abs(float(M.calculate_dice(logits, y)) - float(g[f"{tag}/dice"])) < (1e-5 if fp32 else 1e-3)
    assert abs(float(M.calculate_iou(logits, y)) - float(g[f"{tag}/iou"])) < (1e-5 if fp32 else 1e-3)
    assert abs(float(M.calculate_accuracy(logits, y)) - float(g[f"{tag}/acc"])) < (1e-5 if fp32 else 2e-3)
    names = list(g["grad_names"])
    ref_norms = g[f"{tag}/grad_norms"]
    # bf16 yardstick: the reference's OWN autocast-bf16 run deviates from its fp32 run by this much per parameter
    # (16^3: median 0.41, 32^3: median 0.25); the HIP bf16 path must stay within 1.5x of that (floor 0.05)
    yard = dict(zip(names, g[f"{tag}/autocast_bf16/grad_relerr"]))
    params = dict(m.named_parameters())
    for k, rn in zip(names, ref_norms):
        gn = float(params[k].grad.double().norm())
        if rn < 1e-5:       # conv bias in front of train-mode BN: analytically zero, roundoff only
            assert np.isfinite(gn) and (gn < 1e-3 or not fp32), k
        else:
            assert abs(gn - rn) / rn < (5e-3 if fp32 else max(0.05, 1.5 * yard[k])), (k, gn, rn)
    for k in [kk[len(tag) + 6:] for kk in g if kk.startswith(f"{tag}/grad/")]:
        ref = g[f"{tag}/grad/{k}"]
        if np.linalg.norm(ref) < 1e-5:
            continue
        e = relerr(params[k].grad.cpu(), ref)
        assert e < (5e-3 if fp32 else max(0.05, 1.5 * yard[k])), (k, e, yard[k])
    sd = m.state_dict()
    bn = np.concatenate([sd[k].cpu().numpy().ravel() for k in g[f"{tag}/bn_keys"]])
    assert relerr(bn, g[f"{tag}/bn_after1"]) < (1e-4 if fp32 else 2e-2)


def test_adamw_trajectory_golden(golden):
    """5 optimizer steps (torch.optim.AdamW drives our Parameters in place) on the learnable blocky problem."""
    g = golden("default_unet")
    m = _default_model().to(DEV).train()
    m.compute_dtype = torch.float32
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(2, 1, 16, 16, 16, generator=gen)
    _ = torch.randint(0, 4, (2, 1, 16, 16, 16), generator=gen)
    zz, yy, xx = torch.meshgrid(torch.arange(16), torch.arange(16), torch.arange(16), indexing="ij")
    lab = ((zz // 4) + (yy // 4) + (xx // 4)) % 4
    y = lab[None, None].expand(2, 1, 16, 16, 16).contiguous().long()
    x = y.float() / 3.0 + 0.1 * x
    x, y = x.to(DEV), y.to(DEV)
    losses, dices = [], []
    for _ in range(5):
        opt.zero_grad()
        o = m(x)
        l = M.combined_loss(o, y)
        l.backward()
        opt.step()
        losses.append(l.item())
        dices.append(float(M.calculate_dice(o, y)))
    np.testing.assert_allclose(losses, g["traj/loss"], rtol=2e-3)
    np.testing.assert_allclose(dices, g["traj/dice"], atol=2e-3)


def test_dann_step_golden(golden):
    """One DANN step (train_dann.py:268-285): two forwards, GRL, discriminator, single backward."""
    g = golden("dann")
    # GRL
    f = t(g["grl/x"]).requires_grad_(True)
    r = grad_reverse(f, 0.2)
    r.backward(t(g["grl/go"]))
    np.testing.assert_allclose(r.detach().cpu().numpy(), g["grl/out"])
    np.testing.assert_allclose(f.grad.cpu().numpy(), g["grl/gx"], rtol=1e-6)
    # discriminator eval forward/backward
    torch.manual_seed(3)
    disc = DomainDiscriminator(256)
    sd = disc.state_dict()
    keys = sorted(sd.keys())
    dig = np.array([[float(sd[k].double().sum()), float(sd[k].double().abs().sum())] for k in keys])
    np.testing.assert_allclose(dig, g["disc/param_digest"], rtol=1e-12)
    disc = disc.to(DEV).eval()
    feats = t(g["disc/feats"]).requires_grad_(True)
    pred = disc(feats)
    l = domain_ce(pred, torch.tensor([0, 0, 1, 1], device=DEV))
    l.backward()
    np.testing.assert_allclose(pred.detach().cpu().numpy(), g["disc/pred"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(l.item(), g["disc/loss"], rtol=1e-5)
    np.testing.assert_allclose(feats.grad.cpu().numpy(), g["disc/gfeats"], rtol=1e-3, atol=1e-6)
    for k, p in disc.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g["disc/grad/" + k], rtol=1e-3, atol=1e-6, err_msg=k)
    # full step
    seg = _default_model(unet_dann.UNet3D).to(DEV).train()
    seg.compute_dtype = torch.float32
    torch.manual_seed(3)
    disc = DomainDiscriminator(256)
    for mod in disc.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    disc = disc.to(DEV).train()
    xs, ys, xt = t(g["step/xs"]), t(g["step/ys"]), t(g["step/xt"])
    lam = 0.2
    so, sf = seg(xs, return_features=True)
    task = M.combined_loss(so, ys)
    _, tf = seg(xt, return_features=True)
    sp = disc(grad_reverse(sf, lam))
    tp = disc(grad_reverse(tf, lam))
    dl = domain_ce(torch.cat([sp, tp]), torch.tensor([0, 0, 1, 1], device=DEV))
    total = task + lam * dl
    total.backward()
    # 16^3 input -> 1x1x1 bottleneck: BatchNorm over M=2 values per channel amplifies fp32 roundoff
    np.testing.assert_allclose(sf.detach().cpu().numpy(), g["step/sfeat"], rtol=5e-3, atol=2e-3)
    np.testing.assert_allclose(tf.detach().cpu().numpy(), g["step/tfeat"], rtol=5e-3, atol=2e-3)
    np.testing.assert_allclose(task.item(), g["step/task"], rtol=2e-5)
    np.testing.assert_allclose(dl.item(), g["step/domain"], rtol=2e-5)
    np.testing.assert_allclose(total.item(), g["step/total"], rtol=2e-5)
    params = dict(seg.named_parameters())
    for k, rn in zip(list(g["step/seg_grad_names"]), g["step/seg_grad_norms"]):
        gn = float(params[k].grad.double().norm())
        if rn < 1e-5:
            assert gn < 1e-3, k
        else:
            assert abs(gn - rn) / rn < 5e-3, (k, gn, rn)
    for k, p in disc.named_parameters():
        assert relerr(p.grad.cpu(), g["step/disc_grad/" + k]) < 2e-3, k
    sd = seg.state_dict()
    bn = np.concatenate([sd[k].cpu().numpy().ravel() for k in sorted(k for k in sd if "running" in k)])
    assert relerr(bn, g["step/bn_after"]) < 1e-4
    seg.eval()
    with torch.no_grad():
        o, none = seg(xs)
    assert none is None
    assert relerr(o.cpu(), g["eval/logits"]) < 5e-4


def test_distill_step_golden(golden):
    """distill_unet.py:107-115: student(train) + teacher(eval, no_grad) + distillation_loss."""
    g = golden("distill")
    student = _default_model(seed=0).to(DEV).train()
    teacher = _default_model(seed=1)
    tsd = teacher.state_dict()
    off = 0
    for k in g["teacher_bn_keys"]:
        n = tsd[k].numel()
        tsd[k].copy_(torch.from_numpy(g["teacher_bn"][off:off + n]))
        off += n
    teacher = teacher.to(DEV).eval()
    student.compute_dtype = teacher.compute_dtype = torch.float32
    x, y = _synth(2, 16, 1234)
    x, y = x.to(DEV), y.to(DEV)
    s = student(x)
    with torch.no_grad():
        tl = teacher(x)
    l = M.distillation_loss(s, tl, y, 0.7, 2.0)
    l.backward()
    assert relerr(tl.cpu(), g["teacher_logits"]) < 5e-4
    assert relerr(s.detach().cpu(), g["student_logits"]) < 5e-4
    np.testing.assert_allclose(l.item(), g["loss"], rtol=5e-5)
    for (k, p), rn in zip(student.named_parameters(), g["grad_norms"]):
        gn = float(p.grad.double().norm())
        if rn > 1e-5:
            assert abs(gn - rn) / rn < 5e-3, (k, gn, rn)


def test_second_backward_through_a_node_is_refused():
    """The autograd node gives its workspace back after the backward.  A second backward through the same node
    (retain_graph=True) must be refused by the library's argument check (NULL workspace) before anything is launched, never
    run on the freed block."""
    from multimodal_segmentation_project_amd._lib import Mi3dError
    torch.manual_seed(0)
    m = UNet3D(in_channels=1, out_channels=4).to(DEV).train()
    m.compute_dtype = torch.float32
    loss = m(torch.randn(1, 1, 16, 16, 16, device=DEV)).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(Mi3dError, match="null pointer"):
        loss.backward()


def test_dropout_semantics():
    """Dropout3d: channel-wise masks with scale 1/(1-p) (models/unet.py:14,18); injected masks are honoured,
    generated masks have the right keep rate; eval mode ignores dropout."""
    import ctypes as C
    from multimodal_segmentation_project_amd import _lib, engine
    m = _default_model().to(DEV).train()
    m.dropout_rate = 0.5
    m.compute_dtype = torch.float32
    x, _ = _synth(1, 16, 7)
    x = x.to(DEV)
    desc = engine.build_desc(m, x, torch.float32)
    n = _lib.lib().mi3d_unet_dropout_count(C.byref(desc))
    sc = engine.make_drop_scales(m, desc, 0.5, x.device)
    vals = sc.unique().cpu().tolist()
    assert set(vals) <= {0.0, 2.0} and n == sc.numel()
    assert 0.35 < (sc == 0).float().mean().item() < 0.65
    sc2 = engine.make_drop_scales(m, desc, 0.5, x.device)
    assert not torch.equal(sc, sc2)             # counter advanced
    # all-ones injected mask == no dropout
    m._mi3d_injected_drop_scales = torch.ones(n)
    a = m(x)
    m._mi3d_injected_drop_scales = None
    m.dropout_rate = 0.0
    torch.manual_seed(0)
    m2 = _default_model().to(DEV).train()
    m2.compute_dtype = torch.float32
    b = m2(x)
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_determinism_and_scale_96(dtype):
    """BASELINE config-2 shape (96^3, N=2): finite outputs, bitwise run-to-run reproducibility of loss and
    gradients (two-stage reductions, no float atomics), and linearity of backward in the upstream gradient."""
    m = _default_model().to(DEV).train()
    m.compute_dtype = dtype
    x, y = _synth(2, 96, 1234)
    x, y = x.to(DEV), y.to(DEV)

    def run(scale):
        for p in m.parameters():
            p.grad = None
        for b in m.buffers():          # restore BN buffers so both runs start from the same state
            pass
        o = m(x)
        l = M.combined_loss(o, y)
        (scale * l).backward()
        return l.item(), [p.grad.clone() for p in m.parameters()], o

    l1, g1, o1 = run(1.0)
    l2, g2, o2 = run(1.0)
    assert np.isfinite(l1) and l1 == l2
    assert torch.equal(o1, o2)
    for a, b in zip(g1, g2):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    l3, g3, _ = run(2.0)
    for a, b in zip(g1, g3):
        assert relerr((b / 2).cpu(), a.cpu()) < (1e-5 if dtype == torch.float32 else 2e-2)
    assert tuple(o1.shape) == (2, 4, 96, 96, 96) and o1.dtype == torch.float32


def test_layout_and_kernel_choices_are_invisible(routes):
    """The full-resolution planar skip/up layout, the persistent conv kernels and the MFMA path are scheduling /
    layout choices: switching them off (environment switches read per call) must not change the results beyond the
    summation-order noise of a different kernel (planar vs interleaved: bitwise, same kernels and order)."""
    m = _default_model().to(DEV).train()
    m.compute_dtype = torch.bfloat16
    x, y = _synth(2, 32, 77)
    x, y = x.to(DEV), y.to(DEV)

    def run():
        for p in m.parameters():
            p.grad = None
        o = m(x)
        l = M.combined_loss(o, y)
        l.backward()
        return l.item(), o.detach().clone(), [p.grad.clone() for p in m.parameters()]

    l0, o0, g0 = run()
    routes.set("no_planar", 1)
    l1, o1, g1 = run()
    assert l0 == l1 and torch.equal(o0, o1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # BN-apply + max-pool in one launch vs two: the pooled value is the maximum of the same rounded activations -> bitwise
    routes.set("no_pool_fuse", 1)
    l4, o4, g4 = run()
    assert l0 == l4 and torch.equal(o0, o4)
    for a, b in zip(g0, g4):
        assert torch.equal(a, b)
    routes.reset("no_pool_fuse")
    # fused backward launches (dgrad + wgrad, upconv data + weight gradient) off: same kernels bodies, only the
    # weight-gradient slab partition (summation order) changes
    routes.set("no_fused_bwd", 1)
    routes.set("no_fused_upbwd", 1)
    l3, o3, g3 = run()
    assert l3 == l0 and torch.equal(o3, o0)
    va = torch.cat([a.flatten() for a in g0]).cpu()
    vb = torch.cat([b.flatten() for b in g3]).cpu()
    assert relerr(vb, va) < 1e-3
    routes.set("no_persist", 1)          # generic one-tile-per-workgroup kernels everywhere
    l2, o2, g2 = run()
    assert abs(l2 - l0) < 2e-3 * abs(l0)
    assert relerr(o2.cpu(), o0.cpu()) < 2e-2
    # gradients: two different bf16 kernel sets, each within the reference's own autocast error of fp32 (goldens); the
    # small deep-level tensors are rounding-noise dominated at 32^3, so compare the whole gradient vector
    va = torch.cat([a.flatten() for a in g0]).cpu()
    vb = torch.cat([b.flatten() for b in g2]).cpu()
    assert relerr(vb, va) < 0.1


@pytest.mark.parametrize("shape", [(1, 16, 16, 5, 9, 17), (2, 32, 16, 6, 17, 35), (1, 16, 32, 4, 16, 48),
                                   (1, 64, 32, 4, 8, 8), (1, 32, 64, 3, 6, 6), (1, 16, 16, 8, 16, 32)])
def test_conv3_mfma_vs_c_oracle(orc, shape):
    """bf16 MFMA implicit-GEMM conv (forward, input-gradient, weight-gradient) vs the C oracle on ragged volumes.
    Inputs are small dyadic rationals (exact in bf16), so the only error is the final bf16 rounding of the output, and
    the fp32-accumulated weight / bias gradients must be exact (atol 1e-5 against values that are multiples of 1/64)."""
    from multimodal_segmentation_project_amd import _lib
    from multimodal_segmentation_project_amd._lib import call, ptr
    n, cin, cout, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-8, 9, (n, cin, d, h, w)).astype(np.float32) / 8
    wgt = rng.integers(-8, 9, (cout, cin, 3, 3, 3)).astype(np.float32) / 16
    b = rng.integers(-8, 9, cout).astype(np.float32) / 4
    gy = rng.integers(-8, 9, (n, cout, d, h, w)).astype(np.float32) / 8
    xcl = t(x.transpose(0, 2, 3, 4, 1)).bfloat16()
    gcl = t(gy.transpose(0, 2, 3, 4, 1)).bfloat16()
    wd, bd = t(wgt), t(b)
    wsb = _lib.lib().mi3d_conv3_workspace_bytes(cin, cout, n, d, h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    y = torch.empty((n, d, h, w, cout), device=DEV, dtype=torch.bfloat16)
    call("mi3d_conv3_forward", 1, 1, ptr(xcl), cin, cin, ptr(wd), ptr(bd), ptr(y), cout, cout, n, d, h, w, ptr(ws), wsb, None)
    ref = orc.conv3d_fwd(x, wgt, b)
    got = y.float().cpu().numpy().transpose(0, 4, 1, 2, 3)
    assert np.abs(got - ref).max() <= np.abs(ref).max() * 2 ** -8 + 1e-6
    assert_bf16_rne_bits(y, ref, "y")               # every partial sum is exact in fp32: the stored value is bf16_rne(exact)
    dx = torch.empty_like(xcl)
    dW = torch.empty((cout, cin, 3, 3, 3), device=DEV)
    db = torch.empty(cout, device=DEV)
    call("mi3d_conv3_backward", 1, 1, ptr(xcl), cin, cin, ptr(wd), ptr(gcl), cout, cout, ptr(dx), cin, ptr(dW), ptr(db), 0,
         n, d, h, w, ptr(ws), wsb, None)
    rgx, rgw, rgb = orc.conv3d_bwd(x, wgt, gy)
    gotx = dx.float().cpu().numpy().transpose(0, 4, 1, 2, 3)
    assert np.abs(gotx - rgx).max() <= np.abs(rgx).max() * 2 ** -8 + 1e-6
    assert_bf16_rne_bits(dx, rgx, "dx")
    np.testing.assert_allclose(dW.cpu().numpy(), rgw, rtol=0, atol=1e-5)
    np.testing.assert_allclose(db.cpu().numpy(), rgb, rtol=0, atol=1e-5)


@pytest.mark.parametrize("shape", [(1, 16, 5, 9, 17), (2, 16, 8, 16, 32), (1, 32, 4, 8, 16)])
def test_conv3_first_layer_wgrad_mfma(orc, shape):
    """First layer (Cin=1, fp32 image, bf16 dy): weight/bias gradient on the matrix cores vs the C oracle."""
    from multimodal_segmentation_project_amd import _lib
    from multimodal_segmentation_project_amd._lib import call, ptr
    n, cout, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-8, 9, (n, 1, d, h, w)).astype(np.float32) / 8
    wgt = rng.integers(-8, 9, (cout, 1, 3, 3, 3)).astype(np.float32) / 16
    gy = rng.integers(-8, 9, (n, cout, d, h, w)).astype(np.float32) / 8
    xd = t(x)
    gcl = t(gy.transpose(0, 2, 3, 4, 1)).bfloat16()
    wd = t(wgt)
    wsb = _lib.lib().mi3d_conv3_workspace_bytes(1, cout, n, d, h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dW = torch.empty((cout, 1, 3, 3, 3), device=DEV)
    db = torch.empty(cout, device=DEV)
    call("mi3d_conv3_backward", 0, 1, ptr(xd), 1, 1, ptr(wd), ptr(gcl), cout, cout, None, 1, ptr(dW), ptr(db), 0,
         n, d, h, w, ptr(ws), wsb, None)
    _, rgw, rgb = orc.conv3d_bwd(x, wgt, gy)
    np.testing.assert_allclose(dW.cpu().numpy(), rgw, rtol=0, atol=1e-5)
    np.testing.assert_allclose(db.cpu().numpy(), rgb, rtol=0, atol=1e-5)


@pytest.mark.parametrize("shape", [(2, 32, 16, 3, 5, 7), (1, 64, 32, 4, 4, 6), (1, 256, 128, 2, 3, 2), (1, 128, 64, 3, 3, 3)])
def test_upconv_mfma_vs_c_oracle(orc, shape):
    """bf16 MFMA ConvTranspose3d(k2,s2): forward (strided write into a wider concat buffer), dx, dW, db."""
    from multimodal_segmentation_project_amd import _lib
    from multimodal_segmentation_project_amd._lib import call, ptr
    n, cin, cout, d, h, w = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(-8, 9, (n, cin, d, h, w)).astype(np.float32) / 8
    wgt = rng.integers(-8, 9, (cin, cout, 2, 2, 2)).astype(np.float32) / 16
    b = rng.integers(-8, 9, cout).astype(np.float32) / 4
    gy = rng.integers(-8, 9, (n, cout, 2 * d, 2 * h, 2 * w)).astype(np.float32) / 8
    xcl = t(x.transpose(0, 2, 3, 4, 1)).bfloat16()
    wd, bd = t(wgt), t(b)
    wsb = _lib.lib().mi3d_upconv2_workspace_bytes(cin, cout, n, d, h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    # output goes to channels [cout, 2cout) of a [.., 2cout] buffer, like the plan's concat buffer
    cat = torch.zeros((n, 2 * d, 2 * h, 2 * w, 2 * cout), device=DEV, dtype=torch.bfloat16)
    call("mi3d_upconv2_forward", 1, ptr(xcl), cin, cin, ptr(wd), ptr(bd), cat.data_ptr() + 2 * cout, 2 * cout, cout,
         n, d, h, w, ptr(ws), wsb, None)
    ref = orc.convT2_fwd(x, wgt, b)
    got = cat[..., cout:].float().cpu().numpy().transpose(0, 4, 1, 2, 3)
    assert np.abs(got - ref).max() <= np.abs(ref).max() * 2 ** -8 + 1e-6
    assert_bf16_rne_bits(cat[..., cout:], ref, "y")
    assert float(cat[..., :cout].abs().max()) == 0.0
    gcat = torch.zeros_like(cat)
    gcat[..., cout:] = t(gy.transpose(0, 2, 3, 4, 1)).bfloat16()
    dx = torch.empty_like(xcl)
    dW, db = torch.empty((cin, cout, 2, 2, 2), device=DEV), torch.empty(cout, device=DEV)
    call("mi3d_upconv2_backward", 1, ptr(xcl), cin, cin, ptr(wd), gcat.data_ptr() + 2 * cout, 2 * cout, cout, ptr(dx), cin,
         ptr(dW), ptr(db), 0, n, d, h, w, ptr(ws), wsb, None)
    rgx, rgw, rgb = orc.convT2_bwd(x, wgt, gy)
    gotx = dx.float().cpu().numpy().transpose(0, 4, 1, 2, 3)
    assert np.abs(gotx - rgx).max() <= np.abs(rgx).max() * 2 ** -8 + 1e-6
    assert_bf16_rne_bits(dx, rgx, "dx")
    np.testing.assert_allclose(dW.cpu().numpy(), rgw, rtol=0, atol=1e-5)
    np.testing.assert_allclose(db.cpu().numpy(), rgb, rtol=0, atol=1e-5)


@pytest.mark.gpu
def test_eval_per_class_metrics_and_counts():
    """per-class Dice/IoU of test_model.py:255-276 (absent class -> 0.0) and the exact count pass,
    against a literal torch restatement of those lines on the CPU."""
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 4, 12, 20, 28, generator=g)
    label = torch.randint(0, 3, (2, 1, 12, 20, 28), generator=g)          # class 3 absent from the labels
    got = M.per_class_dice_iou(logits.to(DEV), label.to(DEV))
    pred_classes = torch.argmax(logits, dim=1)
    label_classes = label.squeeze(1)
    for c in (1, 2, 3):
        pm, lm = pred_classes == c, label_classes == c
        if lm.sum() > 0:
            inter = (pm & lm).sum().float()
            dice = ((2. * inter + 1e-5) / (pm.sum() + lm.sum() + 1e-5)).item()
            iou = ((inter + 1e-5) / (pm.sum() + lm.sum() - inter + 1e-5)).item()
        else:
            dice = iou = 0.0
        assert abs(got[c][0] - dice) < 1e-6 and abs(got[c][1] - iou) < 1e-6, (c, got[c], dice, iou)
    assert got[3] == (0.0, 0.0)
    cnt = M.class_counts(logits.to(DEV), label.to(DEV)).cpu()
    for c in range(4):
        assert cnt[c].item() == int(((pred_classes == c) & (label_classes == c)).sum())
        assert cnt[4 + c].item() == int((pred_classes == c).sum())
        assert cnt[8 + c].item() == int((label_classes == c).sum())
    assert cnt[12].item() == int((pred_classes == label_classes).sum())
