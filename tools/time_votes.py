"""Time the flip / model ensemble votes at the size a user runs them: python tools/time_votes.py [--out FILE]

Device events, one pair per repeat, 3 warm-up + 10 timed repeats; every row gives the median and the spread (min .. max) of the
repeats.  Rows that are compared run in the same process, alternating repeat by repeat.  Bytes are algorithmic, from the shapes;
"of peak" is bytes / 8 TB/s (HBM is the bound of every kernel here) over the median.

  1. the three passes of mi3d_head_votes on a bf16 decoder output with 16 channels, 4 classes, 192^3, N = 1, next to
     mi3d_head_labels on the same input.  Per voxel 2 * 16 B of z and
         FIRST   4 C written              MIDDLE  4 C read + 4 C written              LAST  4 C read + 1 B of label
     (head_labels: the 1 B of label alone).  Two inputs and two vote volumes alternate, so a timed read is not a re-hit of the
     Infinity Cache.  MIDDLE is timed unflipped and with all three axes mirrored; LAST also with confidence and the kept total.
  2. the eight-view call against the torch route it replaces, 192^3, N = 1, bf16:
       new       segment.predict_labels_ensemble(model, x, FLIPS8)
       replaced  per view model(torch.flip(x)) -> torch.softmax -> torch.flip -> add; torch.argmax at the end
     and the single-view segment.predict_labels for scale."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_segmentation_project_amd as mi  # noqa: E402
from multimodal_segmentation_project_amd import _lib, segment  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr  # noqa: E402

PEAK = 8e12
WARM, REPS = 3, 10
GRID = (192, 192, 192)
CIN, C = 16, 4


def timed(fns):
    """fns: callables fn(i) that run alternately, repeat by repeat; returns per callable the list of REPS times in microseconds."""
    for i in range(WARM):
        for fn in fns:
            fn(i)
    marks = [[] for _ in fns]
    for i in range(REPS):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            marks[k].append((a, b))
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1e3 for a, b in m] for m in marks]


def row(what, us, nbytes=None):
    med = statistics.median(us)
    s = f"  {what:62s} {med:10.1f} us  (min {min(us):.1f} .. max {max(us):.1f})"
    if nbytes is not None:
        s += f"  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.3f} TB/s  {nbytes / PEAK * 1e6 / med:6.3f} of peak (HBM, 8 TB/s)"
    return s


class Passes:
    """The operands of the pass timings and one callable per row."""

    def __init__(self):
        d, h, w = GRID
        self.v = v = d * h * w
        g = torch.Generator(device="cuda").manual_seed(1)
        self.zs = [torch.randn((1, v, CIN), device="cuda", generator=g).to(torch.bfloat16) for _ in range(2)]
        self.w, self.b = torch.randn((C, CIN), device="cuda", generator=g) * 0.3, torch.randn(C, device="cuda", generator=g) * 0.1
        self.votes = [torch.rand((1, C, d, h, w), device="cuda", generator=g) for _ in range(2)]
        self.labels = torch.empty((1, d, h, w), dtype=torch.uint8, device="cuda")
        self.conf = torch.empty((1, d, h, w), device="cuda")
        self.s = torch.cuda.current_stream().cuda_stream

    def vote(self, view, flip=7, flags=0, conf=False):
        """A pass of a three-view sequence: view 0 FIRST, 1 MIDDLE, 2 LAST."""
        last = view == 2

        def fn(i):
            call("mi3d_head_votes", 1, ptr(self.zs[i % 2]), CIN, CIN, ptr(self.w), ptr(self.b), C, 1, *GRID, flip, view, 3, flags,
                 ptr(self.votes[i % 2]), ptr(self.labels) if last else None, ptr(self.conf) if last and conf else None, None, None,
                 None, self.s)
        return fn

    def head_labels(self):
        def fn(i):
            call("mi3d_head_labels", 1, ptr(self.zs[i % 2]), CIN, CIN, ptr(self.w), ptr(self.b), C, 1, self.v, ptr(self.labels), None,
                 None, None, self.s)
        return fn


def passes(lines):
    p = Passes()
    v, z = p.v, 2 * CIN
    rows = [("head_labels (no target)", p.head_labels(), z + 1),
            ("head_votes FIRST, flip 7", p.vote(0), z + 4 * C),
            ("head_votes MIDDLE, flip 0", p.vote(1, flip=0), z + 8 * C),
            ("head_votes MIDDLE, flip 7", p.vote(1), z + 8 * C),
            ("head_votes LAST, flip 7", p.vote(2), z + 4 * C + 1),
            ("head_votes LAST, flip 7, + confidence + kept total", p.vote(2, flags=_lib.VOTES_KEEP, conf=True), z + 8 * C + 1 + 4)]
    # row k takes input (i + k) % 2: consecutive calls never read the same input
    times = timed([(lambda i, fn=fn, k=k: fn(i + k)) for k, (_, fn, _) in enumerate(rows)])
    lines.append(f"passes of mi3d_head_votes, {GRID} N = 1 bf16, Cin = {CIN}, {C} classes, {v} voxels")
    for (what, _, per_voxel), us in zip(rows, times):
        lines.append(row(what, us, per_voxel * v))


def routes(lines):
    torch.manual_seed(0)
    model = mi.UNet3D(in_channels=1, out_channels=C, dropout_rate=0.0).cuda().eval()
    model.compute_dtype = torch.bfloat16
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.fill_(0.1)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((1, 1) + GRID, device="cuda", generator=g)

    def new(i):
        return segment.predict_labels_ensemble(model, x, flips=segment.FLIPS8)

    def old(i):
        total = None
        with torch.no_grad():
            for f in segment.FLIPS8:
                dims = segment._flip_dims(f)
                p = torch.softmax(model(torch.flip(x, dims) if dims else x), dim=1)
                p = torch.flip(p, dims) if dims else p
                total = p if total is None else total.add_(p)
        return torch.argmax(total, dim=1)

    def single(i):
        return segment.predict_labels(model, x)

    differ = int((new(0).long() != old(0)).sum())
    t_new, t_old, t_one = timed([new, old, single])
    lines.append(f"eight-view route, {GRID} N = 1 bf16 (voxels whose label differs between the two routes: {differ} of {x.numel()})")
    lines.append(row("new: predict_labels_ensemble(model, x, FLIPS8)", t_new))
    lines.append(row("replaced: 8 x (model(flip) -> softmax -> flip -> add), argmax", t_old))
    lines.append(row("for scale: predict_labels(model, x), one view", t_one))
    d = statistics.median(t_new) - statistics.median(t_old)
    lines.append(f"  new - replaced (medians): {d:+.1f} us; new - 8 x one view: {statistics.median(t_new) - 8 * statistics.median(t_one):+.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the rows to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_votes.py needs a GPU (there is no CPU fallback)")
    lines = [f"tools/time_votes.py: device events, {WARM} warm-up + {REPS} timed repeats, median (min .. max); "
             f"{torch.cuda.get_device_name(0)}"]
    passes(lines)
    torch.cuda.empty_cache()
    routes(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
