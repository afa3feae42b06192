"""GPU tests of the boundary term at the step level: TrainStep(boundary_weight=...), against the step without the keyword, the
unfused route, the float64 model of tests/boundary_ref.py on the logits the step left, and the module path
`combined_loss + w * boundary_loss` through model(x) autograd.  32^3, N = 2, bf16, 4 classes, dropout 0: the smallest volume the
step tests use (tests/test_gpu_masked_step.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as B  # noqa: E402

from multimodal_segmentation_project_amd import metrics as M  # noqa: E402
from multimodal_segmentation_project_amd import surface  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError  # noqa: E402
from multimodal_segmentation_project_amd.trainer import TrainStep  # noqa: E402
from multimodal_segmentation_project_amd.unet import UNet3D  # noqa: E402

DEV = "cuda:0"
S, N, IG, CLASSES = 32, 2, 255, (1, 2, 3)
KW = dict(lr=1e-3, weight_decay=0.01, compute_dtype=torch.bfloat16)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def synth(seed, ignored=0.0):
    """Blocky labels with the image correlated to them (as tests/test_gpu_masked_step.py's synth), a share of the voxels ignored."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), torch.arange(S), indexing="ij")
    lab = ((zz // (S // 4)) + (yy // (S // 4)) + (xx // (S // 4))) % 4
    y = lab[None, None].expand(N, 1, S, S, S).contiguous().long()
    x = y.float() / 3.0 + 0.1 * torch.randn(N, 1, S, S, S, generator=g)
    if ignored > 0.0:
        y = torch.where(torch.rand(y.shape, generator=g) < ignored, torch.full_like(y, IG), y)
    return x.to(DEV), y.to(DEV)


def model(seed=3):
    torch.manual_seed(seed)
    return UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).to(DEV).train()


def snapshot(ts, m):
    return ([p.detach().clone().cpu() for p in m.parameters()], ts.arena.m.clone().cpu(), ts.arena.v.clone().cpu())


def same_state(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def run(x, y, steps=2, weights=None, dist=None, **kw):
    """`steps` steps of a fresh model; weights: the boundary_weight set in front of each step.  (outputs, state, fused_head)."""
    m = model()
    ts = TrainStep(m, **{**KW, **kw})
    outs = []
    for k in range(steps):
        if weights is not None:
            ts.boundary_weight = weights[k]
        outs.append(ts.step(x, y, dist=dist).cpu() if dist is not None else ts.step(x, y).cpu())
    res = (outs, snapshot(ts, m), ts._static["fused_head"])
    ts.close()
    return res


def same_run(a, b):
    return all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and same_state(a[1], b[1])


def test_without_the_keyword_nothing_changes():
    x, y = synth(77)
    plain, none = run(x, y), run(x, y, boundary_weight=None)
    assert plain[2] and none[2] and same_run(plain, none)
    m = model()
    ts = TrainStep(m, **KW)
    ts.step(x, y)
    assert ts.boundary_weight is None and not hasattr(ts._static, "dist") and ts._static["logits"] is None
    with pytest.raises(Mi3dError):
        ts.boundary_weight = 1.0
    with pytest.raises(Mi3dError):
        ts.step(x, y, dist=torch.zeros((N, 3, S, S, S), device=DEV))
    ts.close()
    for bad in (dict(boundary_weight=float("nan")), dict(boundary_weight="x"), dict(boundary_weight=1.0, boundary_classes=(1, 1)),
                dict(boundary_weight=1.0, boundary_spacing=(1, 0, 1))):
        with pytest.raises(Mi3dError):
            TrainStep(model(), **KW, **bad)
    ts = TrainStep(model(), **KW, boundary_weight=1.0, boundary_classes=(1, 4))          # the head has channels 0..3
    with pytest.raises(Mi3dError):
        ts.step(x, y)
    ts.close()


def test_weight_zero_gives_the_unfused_route(routes):
    x, y = synth(77)
    zero = run(x, y, boundary_weight=0.0)
    routes.set("no_head_loss", 1)
    unfused = run(x, y)
    assert not zero[2] and not unfused[2] and same_run(zero, unfused)


def module_grads(x, y, dist, w, ignore=None, dtype=torch.bfloat16):
    """The gradients of combined_loss + w * boundary_loss through model(x) autograd."""
    m = model()
    m.compute_dtype = dtype
    logits = m(x)
    kw = dict(ignore_index=ignore) if ignore is not None else {}
    bkw = dict(target=y, ignore_index=ignore) if ignore is not None else {}
    (M.combined_loss(logits, y, **kw) + w * M.boundary_loss(logits, dist, CLASSES, **bkw)).backward()
    return {k: p.grad.detach().clone().cpu() for k, p in m.named_parameters()}


@pytest.mark.parametrize("ignored", [0.0, 0.3], ids=["all_voxels", "ignore_index_255"])
def test_step_with_a_weight_equals_the_model_and_the_module_path(ignored):
    """lr = 0.  bf16: loss = overlap + weight * the model's L on the logits the step left, inside the allowance (the overlap loss is
    that of the same step at weight 0).  The parameter gradients equal the module path's within the bound of the
    fused-against-unfused step tests (per-tensor relative error < 1e-3, the same two bias exclusions), with float32 activations:
    the step folds the weight into the kernel's scale and autograd multiplies afterwards, so the two dlogits differ in the last
    bit of some elements (relative 3e-8 measured), and a bf16 backward re-rounds such a difference up to bf16's own step at every
    layer (measured at 0.75 and bf16: 3e-5 at upconvs.3 growing to 8e-3 at encoder.3, while at weight 0 every gradient is
    bitwise the module path's).  With float32 activations the comparison measures the step and not that noise."""
    x, y = synth(5, ignored)
    w = 0.75
    ig = IG if ignored else None
    kw = dict(lr=0.0, weight_decay=0.0, compute_dtype=torch.bfloat16, ignore_index=ig)
    m0 = model()
    t0 = TrainStep(m0, **kw, boundary_weight=0.0)
    overlap = t0.step(x, y).cpu()
    t0.close()
    m = model()
    ts = TrainStep(m, **kw, boundary_weight=w)
    out = ts.step(x, y).cpu()
    st = ts._static
    assert not st["fused_head"] and st["dist"].shape == (N, 3, S, S, S) and st["dist"].dtype == torch.float32
    assert torch.equal(out[1:], overlap[1:])
    z = st["logits"].cpu().numpy().reshape(N, 4, -1)
    phi = st["dist"].cpu().numpy().reshape(N, 3, -1)
    dist = st["dist"].clone()
    ts.close()
    lab = y.cpu().numpy().reshape(N, -1) if ignored else None
    assert np.array_equal(phi.view(np.uint32), B.signed_maps(y.cpu().numpy()[:, 0], CLASSES).reshape(N, 3, -1).view(np.uint32))
    value, _ = B.term(z, phi, CLASSES, lab, ig, w)
    want = float(overlap[0]) + value
    allow = B.value_allowance(z, phi, CLASSES, lab, ig, w, value) + B.U * (abs(float(overlap[0])) + abs(want))
    print(f"loss {float(out[0])!r} against {want!r}: off by {abs(float(out[0]) - want):.3e} of {allow:.3e}; boundary part {value!r}")
    assert abs(value) > 100 * allow and abs(float(out[0]) - want) <= allow
    m32 = model()
    t32 = TrainStep(m32, **{**kw, "compute_dtype": torch.float32}, boundary_weight=w)
    t32.step(x, y)
    got = {k: p.grad.detach().clone().cpu() for k, p in m32.named_parameters()}
    t32.close()
    ref = module_grads(x, y, dist, w, ig, torch.float32)
    plain = module_grads(x, y, dist, 0.0, ig, torch.float32)
    worst, moved = 0.0, 0.0
    for k in ref:
        if float(ref[k].double().norm()) < 1e-7 or k.endswith("double_conv.0.bias") or k.endswith("double_conv.4.bias"):
            continue
        worst, moved = max(worst, relerr(got[k], ref[k])), max(moved, relerr(plain[k], ref[k]))
    print(f"step against the module path at 32^3, float32: worst per-tensor gradient relerr {worst}; the term moves a tensor by up to {moved}")
    assert worst < 1e-3 < moved


def test_a_given_dist_equals_the_computed_one():
    x, y = synth(9)
    dist = surface.signed_distance_maps(y, CLASSES)
    assert same_run(run(x, y, boundary_weight=0.5), run(x, y, boundary_weight=0.5, dist=dist))
    other = run(x, y, boundary_weight=0.5, dist=dist * 2.0)          # the buffer is read
    assert not torch.equal(other[0][0], run(x, y, boundary_weight=0.5, steps=1)[0][0])


def test_graph_equals_eager_and_a_new_weight_takes_effect():
    x, y = synth(9, 0.3)
    weights = (0.5, 0.5, 2.0)
    eager = run(x, y, steps=3, weights=weights, boundary_weight=0.5, ignore_index=IG)
    graph = run(x, y, steps=3, weights=weights, boundary_weight=0.5, ignore_index=IG, use_graph=True)
    assert same_run(eager, graph)
    fixed = run(x, y, steps=3, boundary_weight=0.5, ignore_index=IG, use_graph=True)
    assert torch.equal(fixed[0][1], graph[0][1]) and not torch.equal(fixed[0][2], graph[0][2])


def test_grad_accum_two():
    """Two micro-steps on one batch: each returns the undivided loss of the accum = 1 step, the accumulated gradient is that step's
    (halves add up; scaling by 1/2 is exact), captured equals eager."""
    x, y = synth(11)
    kw = dict(lr=0.0, weight_decay=0.0, compute_dtype=torch.bfloat16, boundary_weight=0.75)
    m1 = model()
    t1 = TrainStep(m1, **kw)
    o1 = t1.step(x, y).cpu()
    g1 = {k: p.grad.detach().clone().cpu() for k, p in m1.named_parameters()}
    t1.close()
    m2 = model()
    t2 = TrainStep(m2, **kw, grad_accum=2)
    o2 = [t2.step(x, y).cpu() for _ in range(2)]
    g2 = {k: p.grad.detach().clone().cpu() for k, p in m2.named_parameters()}
    t2.close()
    assert torch.equal(o2[0], o1) and torch.equal(o2[1], o1)
    assert max(relerr(g2[k], g1[k]) for k in g1 if float(g1[k].double().norm()) >= 1e-7) < 1e-5
    eager = run(x, y, steps=4, boundary_weight=0.75, grad_accum=2)
    graph = run(x, y, steps=4, boundary_weight=0.75, grad_accum=2, use_graph=True)
    assert same_run(eager, graph)
