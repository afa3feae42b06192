"""Time the entropy term at the sizes a user trains at: python tools/time_entropy.py [--out FILE] [--no-step]

Device events, one pair per repeat, 3 warm-up + 30 timed repeats; every row gives the median and the spread (min .. max).  Call rows
include the host side of the call (the ctypes launches).

  term   mi3d_entropy_loss at 96^3, N = 2, C = 4 on static buffers, as each step calls it: ADD_LOSS | ADD_GRAD on the ignored voxels
         (30 % of them) for TrainStep, value and gradient stored over every voxel for DannStep, and the value alone; beside each the
         bytes it moves (4 C read + 4 C written per voxel, + 4 C under ADD_GRAD, + 8 with labels) and what they cost at 8 TB/s
  torch  the same value and gradient by log_softmax -> sum -> backward on the same card
  step   TrainStep.step_static at 96^3 x N 2, bf16: the default step, the unfused route without the term, and entropy_weight=0.1;
         DannStep.step_static with and without entropy_weight (with it the target graph's decoder backward runs: real extra work)"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_segmentation_project_amd import _lib  # noqa: E402
from multimodal_segmentation_project_amd import metrics as M  # noqa: E402

WARM, REPS = 3, 30
HBM = 8e12          # bytes per second
IG = 255


def timed(fn):
    for _ in range(WARM):
        fn()
    marks = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        marks.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in marks]


def row(what, us, more=""):
    return f"  {what:78s} {statistics.median(us):10.1f} us  (min {min(us):.1f} .. max {max(us):.1f}){more}"


def batch(n, side, ignored):
    g = torch.Generator().manual_seed(0)
    zz, yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), torch.arange(side), indexing="ij")
    lab = ((zz // (side // 4)) + (yy // (side // 4)) + (xx // (side // 4))) % 4
    y = lab[None, None].expand(n, 1, side, side, side).contiguous().long()
    x = y.float() / 3.0 + 0.1 * torch.randn(n, 1, side, side, side, generator=g)
    if ignored > 0.0:
        y = torch.where(torch.rand(y.shape, generator=g) < ignored, torch.full_like(y, IG), y)
    return x.cuda(), y.cuda()


def term_rows(lines):
    n, c, v = 2, 4, 96 ** 3
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn((n, c, v), device="cuda", generator=g) * 3.0
    lab = batch(n, 96, 0.3)[1].reshape(n, v)
    d, loss = torch.zeros_like(z), torch.zeros((), device="cuda")
    scale = torch.ones((), device="cuda")
    ws = M.entropy_workspace(n, v, "cuda")
    s = _lib.stream_ptr()
    masked = dict(labels=lab, ignore_index=IG, mode=_lib.ENT_IGNORED)
    for what, kw, per_voxel in (("IGNORED, ADD_LOSS | ADD_GRAD (as TrainStep calls it)",
                                 dict(dlogits=d, flags=_lib.ENT_ADD_LOSS | _lib.ENT_ADD_GRAD, **masked), 12 * c + 8),
                                ("ALL, value and gradient stored (as DannStep calls it)", dict(dlogits=d), 8 * c),
                                ("ALL, value alone", dict(), 4 * c)):
        us = timed(lambda: M.entropy_term(z, weight=0.1, grad_scale=scale, loss_out=loss, workspace=ws, stream=s, **kw))
        nbytes = n * v * per_voxel
        floor = nbytes / HBM * 1e6
        lines.append(row(f"mi3d_entropy_loss 96^3 x N 2, C 4: {what}", us,
                         f"  {nbytes / 1e6:.1f} MB = {floor:.1f} us at 8 TB/s: {100 * floor / statistics.median(us):.0f} % of the roofline"))
    zt = z.clone().requires_grad_(True)

    def torch_route():
        zt.grad = None
        ls = torch.log_softmax(zt, dim=1)
        (-(ls.exp() * ls).sum() / (n * v * math.log(c)) * 0.1).backward()

    lines.append(row("torch on the same card: log_softmax -> sum -> backward, every voxel", timed(torch_route)))


def step_rows(lines):
    from multimodal_segmentation_project_amd import unet_dann
    from multimodal_segmentation_project_amd.dann import DomainDiscriminator
    from multimodal_segmentation_project_amd.trainer import DannStep, TrainStep
    from multimodal_segmentation_project_amd.unet import UNet3D
    n, side = 2, 96
    x, y = batch(n, side, 0.3)
    for what, kw, route in (("default step (head folded into the loss), ignore_index=255", {}, 0),
                            ("unfused route (no_head_loss), no entropy term", {}, 1),
                            ("entropy_weight=0.1 on the ignored voxels (unfused route + the term)", dict(entropy_weight=0.1), 0)):
        with _lib.routes(no_head_loss=route):
            torch.manual_seed(3)
            m = UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).cuda().train()
            ts = TrainStep(m, lr=1e-3, compute_dtype=torch.bfloat16, ignore_index=IG, **kw)
            ts.load_batch(x, y)
            lines.append(row(f"TrainStep.step_static 96^3 x N 2 bf16, eager: {what}", timed(ts.step_static)))
            ts.close()
    xs, ys = batch(n, side, 0.0)
    xt = 1.0 - xs
    for what, kw in (("as it always was (five values)", {}), ("entropy_weight=0.1 (target head, term and decoder backward)", dict(entropy_weight=0.1))):
        torch.manual_seed(3)
        seg = unet_dann.UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).cuda().train()
        disc = DomainDiscriminator(256).cuda().train()
        ds = DannStep(seg, disc, lr=1e-3, compute_dtype=torch.bfloat16, **kw)
        ds.load_batch(xs, ys, xt)
        lines.append(row(f"DannStep.step_static 96^3 x N 2 + 2 bf16, eager: {what}", timed(ds.step_static)))
        ds.close()


class Lines(list):
    """The rows, printed as they come."""

    def append(self, s):
        print(s, flush=True)
        super().append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the rows to this file")
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_entropy.py needs a GPU (there is no CPU fallback)")
    lines = Lines()
    lines.append(f"tools/time_entropy.py: device events, {WARM} warm-up + {REPS} timed repeats, median (min .. max); {torch.cuda.get_device_name(0)}")
    term_rows(lines)
    if not a.no_step:
        step_rows(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
