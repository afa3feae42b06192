"""GPU tests of the entropy term at the step level: TrainStep(entropy_weight=..., entropy_on=...) and DannStep(entropy_weight=...),
against the steps without the keyword, the unfused route, the float64 model of tests/entropy_ref.py on the logits the step left, and
the module paths `combined_loss + w * entropy_loss` / `task + lambda * domain + w * entropy_loss(target logits)` through model(x)
autograd.  32^3, N = 2, 4 classes, dropout 0: the smallest volume the step tests use (tests/test_gpu_boundary_step.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entropy_ref as E  # noqa: E402

from multimodal_segmentation_project_amd import dann, unet_dann  # noqa: E402
from multimodal_segmentation_project_amd import metrics as M  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402
from multimodal_segmentation_project_amd.trainer import DannStep, TrainStep  # noqa: E402
from multimodal_segmentation_project_amd.unet import UNet3D  # noqa: E402

DEV = "cuda:0"
S, N, IG, CLASSES = 32, 2, 255, (1, 2, 3)
KW = dict(lr=1e-3, weight_decay=0.01, compute_dtype=torch.bfloat16)
# tests/test_gpu_round2.py, check_summary (the DannStep-against-the-reference's-module-loop tests test_config4_dann96_reference_fixture
# and test_dann_native_step_small_goldens): per-tensor relative error of the float32 segmentation gradients < FP32_GRAD_TOL = 1e-2
DANN_GRAD_TOL = 1e-2


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def synth(seed, ignored=0.0):
    """Blocky labels with the image correlated to them (as tests/test_gpu_boundary_step.py's synth), a share of the voxels ignored."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), torch.arange(S), indexing="ij")
    lab = ((zz // (S // 4)) + (yy // (S // 4)) + (xx // (S // 4))) % 4
    y = lab[None, None].expand(N, 1, S, S, S).contiguous().long()
    x = y.float() / 3.0 + 0.1 * torch.randn(N, 1, S, S, S, generator=g)
    if ignored > 0.0:
        y = torch.where(torch.rand(y.shape, generator=g) < ignored, torch.full_like(y, IG), y)
    return x.to(DEV), y.to(DEV)


def model(seed=3, cls=UNet3D):
    torch.manual_seed(seed)
    return cls(in_channels=1, out_channels=4, dropout_rate=0.0).to(DEV).train()


def snapshot(ts, m):
    return ([p.detach().clone().cpu() for p in m.parameters()], ts.arena.m.clone().cpu(), ts.arena.v.clone().cpu())


def same_state(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def run(x, y, steps=2, weights=None, **kw):
    """`steps` steps of a fresh model; weights: the entropy_weight set in front of each step.  (outputs, state, fused_head)."""
    m = model()
    ts = TrainStep(m, **{**KW, **kw})
    outs = []
    for k in range(steps):
        if weights is not None:
            ts.entropy_weight = weights[k]
        outs.append(ts.step(x, y).cpu())
    res = (outs, snapshot(ts, m), ts._static["fused_head"])
    ts.close()
    return res


def same_run(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and same_state(a[1], b[1])


def named_grads(m):
    return {k: p.grad.detach().clone().cpu() for k, p in m.named_parameters()}


def worst_and_moved(got, ref, plain, floor=1e-7):
    """Largest per-tensor relative error of got against ref, and of plain against ref, over the tensors the fused-against-unfused
    step tests compare (not the conv biases in front of a train-mode BatchNorm: analytically zero)."""
    worst, moved = 0.0, 0.0
    for k in ref:
        if float(ref[k].double().norm()) < floor or k.endswith("double_conv.0.bias") or k.endswith("double_conv.4.bias"):
            continue
        worst, moved = max(worst, relerr(got[k], ref[k])), max(moved, relerr(plain[k], ref[k]))
    return worst, moved


# ---- TrainStep ------------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_nothing_changes():
    x, y = synth(77)
    plain, none = run(x, y), run(x, y, entropy_weight=None)
    assert plain[2] and none[2] and same_run(plain, none)
    m = model()
    ts = TrainStep(m, **KW)
    ts.step(x, y)
    assert ts.entropy_weight is None and not hasattr(ts._static, "ent_ws") and ts._static["logits"] is None
    with pytest.raises(Mi3dError):
        ts.entropy_weight = 1.0
    ts.close()
    for bad in (dict(entropy_weight=float("nan")), dict(entropy_weight="x"), dict(entropy_weight=1.0, entropy_on="some", ignore_index=IG)):
        with pytest.raises(Mi3dError):
            TrainStep(model(), **KW, **bad)


def test_entropy_on_ignored_needs_an_ignore_index():
    with pytest.raises(Mi3dError):
        TrainStep(model(), **KW, entropy_weight=0.1)
    with pytest.raises(Mi3dError):
        TrainStep(model(), **KW, entropy_weight=0.1, entropy_on="ignored")
    for on in ("all", "counted"):
        TrainStep(model(), **KW, entropy_weight=0.1, entropy_on=on).close()
    TrainStep(model(), **KW, entropy_weight=0.1, ignore_index=IG).close()


def test_weight_zero_gives_the_unfused_route(routes):
    x, y = synth(77, 0.3)
    zero = run(x, y, entropy_weight=0.0, ignore_index=IG)
    every = run(x, y, entropy_weight=0.0, entropy_on="all", ignore_index=IG)
    routes.set("no_head_loss", 1)
    unfused = run(x, y, ignore_index=IG)
    assert not zero[2] and not unfused[2] and same_run(zero, unfused) and same_run(every, unfused)


def module_grads(x, y, w, on, ignore=None, dtype=torch.float32, dist=None, bw=0.0):
    """The gradients of combined_loss + w * entropy_loss (+ bw * boundary_loss) through model(x) autograd."""
    m = model()
    m.compute_dtype = dtype
    logits = m(x)
    kw = dict(ignore_index=ignore) if ignore is not None else {}
    ekw = dict(target=y, ignore_index=ignore, on=on) if ignore is not None else {}
    total = M.combined_loss(logits, y, **kw) + w * M.entropy_loss(logits, **ekw)
    if dist is not None:
        total = total + bw * M.boundary_loss(logits, dist, CLASSES, **(dict(target=y, ignore_index=ignore) if ignore is not None else {}))
    total.backward()
    return named_grads(m)


@pytest.mark.parametrize("on,ignored", [("ignored", 0.3), ("counted", 0.3), ("all", 0.0)])
def test_step_with_a_weight_equals_the_model_and_the_module_path(on, ignored):
    """lr = 0.  bf16: loss = overlap + weight * the model's L on the logits the step left, inside the allowance (the overlap loss is
    that of the same step at weight 0), the term at least 100 x the allowance.  The parameter gradients equal the module path's
    within the bound of the fused-against-unfused step tests (per-tensor relative error < 1e-3, the same two bias exclusions) with
    float32 activations, for the reason tests/test_gpu_boundary_step.py gives: the step folds the weight into the kernel's scale
    and autograd multiplies afterwards, a last-bit difference of dlogits that a bf16 backward would re-round layer by layer."""
    x, y = synth(5, ignored)
    w = 2.0
    ig = IG if ignored else None
    mode = E.MODE_NAMES.index(on)
    kw = dict(lr=0.0, weight_decay=0.0, compute_dtype=torch.bfloat16, ignore_index=ig, entropy_on=on)
    t0 = TrainStep(model(), **kw, entropy_weight=0.0)
    overlap = t0.step(x, y).cpu()
    t0.close()
    ts = TrainStep(model(), **kw, entropy_weight=w)
    out = ts.step(x, y).cpu()
    st = ts._static
    assert not st["fused_head"] and ts.entropy_weight == w
    assert torch.equal(out[1:], overlap[1:])
    z = st["logits"].cpu().numpy().reshape(N, 4, -1)
    ts.close()
    lab = y.cpu().numpy().reshape(N, -1) if ignored else None
    value, _ = E.term(z, lab, ig, mode, w)
    want = float(overlap[0]) + value
    allow = E.value_allowance(z, lab, ig, mode, w, value) + E.U * (abs(float(overlap[0])) + abs(want))
    print(f"loss {float(out[0])!r} against {want!r}: off by {abs(float(out[0]) - want):.3e} of {allow:.3e}; entropy part {value!r}")
    assert abs(value) > 100 * allow and abs(float(out[0]) - want) <= allow
    m32 = model()
    t32 = TrainStep(m32, **{**kw, "compute_dtype": torch.float32}, entropy_weight=w)
    t32.step(x, y)
    got = named_grads(m32)
    t32.close()
    ref, plain = module_grads(x, y, w, on, ig), module_grads(x, y, 0.0, on, ig)
    worst, moved = worst_and_moved(got, ref, plain)
    print(f"step against the module path at 32^3, float32: worst per-tensor gradient relerr {worst}; the term moves a tensor by up to {moved}")
    assert worst < 1e-3 < moved


def test_graph_equals_eager_and_a_new_weight_takes_effect():
    x, y = synth(9, 0.3)
    weights = (0.5, 0.5, 2.0)
    eager = run(x, y, steps=3, weights=weights, entropy_weight=0.5, ignore_index=IG)
    graph = run(x, y, steps=3, weights=weights, entropy_weight=0.5, ignore_index=IG, use_graph=True)
    assert same_run(eager, graph)
    fixed = run(x, y, steps=3, entropy_weight=0.5, ignore_index=IG, use_graph=True)
    assert torch.equal(fixed[0][1], graph[0][1]) and not torch.equal(fixed[0][2], graph[0][2])


def test_grad_accum_two():
    """Two micro-steps on one batch: each returns the undivided loss of the accum = 1 step, the accumulated gradient is that step's
    (halves add up; scaling by 1/2 is exact), captured equals eager."""
    x, y = synth(11, 0.3)
    kw = dict(lr=0.0, weight_decay=0.0, compute_dtype=torch.bfloat16, entropy_weight=2.0, ignore_index=IG)
    m1 = model()
    t1 = TrainStep(m1, **kw)
    o1 = t1.step(x, y).cpu()
    g1 = named_grads(m1)
    t1.close()
    m2 = model()
    t2 = TrainStep(m2, **kw, grad_accum=2)
    o2 = [t2.step(x, y).cpu() for _ in range(2)]
    g2 = named_grads(m2)
    t2.close()
    assert torch.equal(o2[0], o1) and torch.equal(o2[1], o1)
    assert max(relerr(g2[k], g1[k]) for k in g1 if float(g1[k].double().norm()) >= 1e-7) < 1e-5
    eager = run(x, y, steps=4, entropy_weight=2.0, ignore_index=IG, grad_accum=2)
    graph = run(x, y, steps=4, entropy_weight=2.0, ignore_index=IG, grad_accum=2, use_graph=True)
    assert same_run(eager, graph)


def test_boundary_and_entropy_together_equal_the_module_path():
    """Both keywords: the boundary pass, then the entropy pass, behind the loss backward; float32 gradients against
    combined_loss + bw * boundary_loss + w * entropy_loss, under the same bound, and the loss is the sum of the three parts."""
    x, y = synth(5, 0.3)
    w, bw = 2.0, 0.75
    kw = dict(lr=0.0, weight_decay=0.0, compute_dtype=torch.float32, ignore_index=IG)
    parts = []
    for extra in (dict(boundary_weight=0.0, entropy_weight=0.0), dict(boundary_weight=bw, entropy_weight=0.0),
                  dict(boundary_weight=0.0, entropy_weight=w), dict(boundary_weight=bw, entropy_weight=w)):
        m = model()
        ts = TrainStep(m, **kw, **extra)
        parts.append(float(ts.step(x, y).cpu()[0]))
        got, dist = named_grads(m), ts._static["dist"].clone()
        ts.close()
    overlap, with_b, with_e, both = parts
    assert abs(both - (with_b + with_e - overlap)) <= 8 * E.U * (abs(overlap) + abs(with_b) + abs(with_e)) and with_e > overlap
    ref = module_grads(x, y, w, "ignored", IG, dist=dist, bw=bw)
    without_e = module_grads(x, y, 0.0, "ignored", IG, dist=dist, bw=bw)
    without_b = module_grads(x, y, w, "ignored", IG)
    worst, moved_e = worst_and_moved(got, ref, without_e)
    _, moved_b = worst_and_moved(got, ref, without_b)
    print(f"both terms against the module path: worst per-tensor gradient relerr {worst}; entropy moves up to {moved_e}, boundary {moved_b}")
    assert worst < 1e-3 < min(moved_e, moved_b)


# ---- DannStep -------------------------------------------------------------------------------------------------------------------
LAM = 0.2


def dann_batches():
    xs, ys = synth(21)
    xt, _ = synth(22)
    return xs, ys, xt


def make_dann(**kw):
    seg = model(0, unet_dann.UNet3D)
    torch.manual_seed(3)
    disc = dann.DomainDiscriminator(256).to(DEV).train()
    for mod in disc.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    step = DannStep(seg, disc, **{**dict(loss="combined", lambda_domain=LAM, lr=1e-3, weight_decay=0.01, compute_dtype=torch.bfloat16), **kw})
    return seg, disc, step


def dann_run(steps=2, weights=None, **kw):
    """(outputs, segmenter parameters, discriminator parameters, target logits or None) after `steps` steps on one batch."""
    xs, ys, xt = dann_batches()
    seg, disc, step = make_dann(**kw)
    outs = []
    for k in range(steps):
        if weights is not None:
            step.entropy_weight = weights[k]
        outs.append(step.step(xs, ys, xt).cpu())
    st = step._static
    t_logits = st["t_logits"].cpu() if step.entropy_weight is not None else None
    res = (outs, step.arena.p.clone().cpu(), step.disc_arena.p.clone().cpu(), t_logits)
    step.close()
    return res


def same_dann(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_dann_without_the_keyword_nothing_changes():
    plain, none = dann_run(), dann_run(entropy_weight=None)
    assert all(o.shape == (5,) for o in plain[0] + none[0]) and same_dann(plain, none)
    seg, disc, step = make_dann()
    step.step(*dann_batches())
    assert step.entropy_weight is None and not hasattr(step._static, "t_logits") and step._static["metrics"].shape == (5,)
    with pytest.raises(Mi3dError):
        step.entropy_weight = 1.0
    step.close()
    with pytest.raises(Mi3dError):
        make_dann(entropy_weight=float("inf"))


def test_dann_with_a_weight_six_values_and_the_model():
    """Six values; the first five of the first step are bitwise those of the step without the keyword (the source graph and the
    discriminator run what they ran); the sixth is entropy_weight * the model's L on the target logits, inside the allowance.  Two
    runs give the same bits, and the target forward on its own stream gives the bits of the serial order."""
    w = 2.0
    plain, a, b = dann_run(), dann_run(entropy_weight=w), dann_run(entropy_weight=w)
    assert all(o.shape == (6,) for o in a[0]) and torch.equal(a[0][0][:5], plain[0][0])
    assert same_dann(a, b)
    assert not torch.equal(a[1], plain[1])          # the term reached the parameters
    serial = dann_run(entropy_weight=w, overlap_forwards=False)
    assert same_dann(a, serial) and torch.equal(a[3], serial[3])
    z = a[3].numpy().reshape(N, 4, -1)          # the target logits of the last step
    value, _ = E.term(z, weight=w)
    allow = E.value_allowance(z, weight=w, value=value)
    got = float(a[0][-1][5])
    print(f"sixth value {got!r} against {value!r}: off by {abs(got - value):.3e} of {allow:.3e}")
    assert abs(got - value) <= allow and value > 100 * allow
    zero = dann_run(entropy_weight=0.0)
    assert float(zero[0][0][5]) == 0.0 and torch.equal(zero[0][0][:5], plain[0][0])


def dann_module_grads(w):
    """task + lambda * domain + w * entropy_loss(target logits) through the modules' autograd (train_dann.py:268-285), float32."""
    xs, ys, xt = dann_batches()
    seg = model(0, unet_dann.UNet3D)
    seg.compute_dtype = torch.float32
    torch.manual_seed(3)
    disc = dann.DomainDiscriminator(256).to(DEV).train()
    for mod in disc.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    s_logits, s_feat = seg(xs, return_features=True)
    t_logits, t_feat = seg(xt, return_features=True)
    preds = torch.cat([disc(dann.grad_reverse(s_feat, LAM)), disc(dann.grad_reverse(t_feat, LAM))])
    labels = torch.cat([torch.zeros(N, dtype=torch.int64), torch.ones(N, dtype=torch.int64)]).to(DEV)
    total = M.combined_loss(s_logits, ys) + LAM * dann.domain_ce(preds, labels)
    if w is not None:
        total = total + w * M.entropy_loss(t_logits)
    total.backward()
    return named_grads(seg), named_grads(disc)


def test_dann_gradients_equal_the_module_path():
    """lr = 0, float32.  Segmenter and discriminator gradients of the step against the module path, per tensor, under the bound of
    the existing DannStep-against-module-loop tests (tests/test_gpu_round2.py check_summary: FP32_GRAD_TOL = 1e-2); the decoder and
    final_conv gradients move by more than that bound against the step without the keyword (there the target batch never reaches
    them), and the step without the keyword meets its own module path under the same bound."""
    w = 2.0
    xs, ys, xt = dann_batches()
    got = {}
    for key, kw in (("plain", {}), ("entropy", dict(entropy_weight=w))):
        seg, disc, step = make_dann(lr=0.0, weight_decay=0.0, compute_dtype=torch.float32, **kw)
        step.step(xs, ys, xt)
        got[key] = (named_grads(seg), named_grads(disc))
        step.close()
    ref_seg, ref_disc = dann_module_grads(w)
    plain_seg, _ = dann_module_grads(None)
    worst, _ = worst_and_moved(got["entropy"][0], ref_seg, ref_seg, floor=1e-6)
    worst_plain, _ = worst_and_moved(got["plain"][0], plain_seg, plain_seg, floor=1e-6)
    worst_disc = max(relerr(got["entropy"][1][k], ref_disc[k]) for k in ref_disc)
    moved = {k: relerr(got["plain"][0][k], got["entropy"][0][k]) for k in ref_seg
             if (k.startswith("decoder") or k.startswith("upconvs") or k.startswith("final_conv")) and float(ref_seg[k].double().norm()) >= 1e-6
             and not k.endswith("double_conv.0.bias") and not k.endswith("double_conv.4.bias")}
    print(f"DannStep against the module path, float32: segmenter {worst} (without the keyword {worst_plain}), discriminator {worst_disc}; "
          f"decoder / head tensors move by {min(moved.values())} .. {max(moved.values())}")
    assert worst < DANN_GRAD_TOL and worst_plain < DANN_GRAD_TOL and worst_disc < DANN_GRAD_TOL
    assert any(k.startswith("final_conv") for k in moved) and min(moved.values()) > DANN_GRAD_TOL


def test_dann_graph_equals_eager_accumulation_and_a_new_weight():
    weights = (0.5, 0.5, 2.0)
    eager = dann_run(steps=3, weights=weights, entropy_weight=0.5)
    graph = dann_run(steps=3, weights=weights, entropy_weight=0.5, use_graph=True)
    assert same_dann(eager, graph)
    fixed = dann_run(steps=3, entropy_weight=0.5, use_graph=True)
    assert torch.equal(fixed[0][1], graph[0][1]) and not torch.equal(fixed[0][2], graph[0][2])
    eager2 = dann_run(steps=4, entropy_weight=2.0, grad_accum=2)
    graph2 = dann_run(steps=4, entropy_weight=2.0, grad_accum=2, use_graph=True)
    assert same_dann(eager2, graph2)
    one = dann_run(steps=1, entropy_weight=2.0)
    assert torch.equal(eager2[0][0], one[0][0])          # the values are undivided by the accumulation count
