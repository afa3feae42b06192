"""Time surface.distance_to and surface.surface_distances at the sizes a user runs them: python tools/time_surface.py [--out FILE] [--no-host]

Device events, one pair per repeat, 3 warm-up + 10 timed repeats that rotate over 3 distinct input sets (the same balls, salt of
other seeds); every row gives the median and the spread (min .. max).  Call rows include the host side of the call (output and
workspace allocation, the ctypes launches).  Kernel rows come from one more profiled pass (torch.profiler, device durations by
kernel name, summed per call, median over its repeats); where the profiler reports no kernels the rows say so.

Inputs: a 192^3 pair of uint8 maps, C-ordered, spacing (1, 1, 1): the target is balls of radii 30, 45, 18, 18 as classes 1, 2, 3, 3
plus 0.2 % salt of random classes, the prediction the same balls shifted by (2, 3, 4) voxels with other salt; and a Fortran-ordered
512 x 512 x 100 pair of the same kind (the balls scaled to the box) at spacing (0.782, 0.782, 5.0).  distance_to is timed on the
surface of class 2 (what the metrics walk towards), on the foreground of the map (dense: short walks) and on a single voxel in a
corner (the longest walks the h and d passes can take).  Beside them the host route (scipy.ndimage.binary_erosion and
distance_transform_edt per class and direction, one process) on a host copy, if scipy imports."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from multimodal_segmentation_project_amd import surface  # noqa: E402
import surface_ref  # noqa: E402

NVOL, WARM, REPS = 3, 3, 10
BALLS_192 = (((90, 60, 60), 30, 1), ((100, 130, 90), 45, 2), ((60, 90, 150), 18, 3), ((130, 90, 150), 18, 3))
SHIFT = (2, 3, 4)
CLASSES = (1, 2, 3)
KERNELS = ("surface_kernel", "nonzero_kernel", "w_kernel", "line_kernel", "query_kernel", "select_kernel")


def inputs(shape, order):
    """NVOL (pred, target) pairs on the device."""
    scale = [s / 192.0 for s in shape]
    lo = min(scale)
    out = []
    for seed in range(NVOL):
        pair = []
        for shift, sd in ((SHIFT, 100 + seed), ((0, 0, 0), seed)):
            balls = [(tuple((c + o) * s for c, o, s in zip(centre, shift, scale)), r * lo, cls) for centre, r, cls in BALLS_192]
            t = torch.from_numpy(surface_ref.balls(shape, balls, 0.002, sd)).cuda()
            pair.append(t if order == "C" else t.permute(2, 1, 0).contiguous().permute(2, 1, 0))
        out.append(tuple(pair))
    return out


def timed(fn):
    for i in range(WARM):
        fn(i % NVOL)
    marks = []
    for i in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i % NVOL)
        b.record()
        marks.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in marks]


def kernel_times(fn):
    """{kernel: [device microseconds per call]} of one profiled pass of REPS calls, by substring of the kernel's name."""
    from torch.profiler import ProfilerActivity, profile
    out = {k: [] for k in KERNELS}
    for i in range(REPS):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(i % NVOL)
            torch.cuda.synchronize()
        for k in KERNELS:
            us = [float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)) for ev in prof.events() if k in ev.name]
            if us:
                out[k].append(sum(us))
    return out


def row(what, us):
    return f"  {what:66s} {statistics.median(us):10.1f} us  (min {min(us):.1f} .. max {max(us):.1f})"


def host_route(pred, target, spacing, ndimage):
    """{class: (hd, hd95, assd)} the way monai.metrics / medpy users compute them."""
    structure = ndimage.generate_binary_structure(3, 1)
    out = {}
    for c in CLASSES:
        p, g = pred == c, target == c
        sp, sg = p & ~ndimage.binary_erosion(p, structure), g & ~ndimage.binary_erosion(g, structure)
        a = ndimage.distance_transform_edt(~sg, sampling=spacing)[sp]
        b = ndimage.distance_transform_edt(~sp, sampling=spacing)[sg]
        out[c] = (max(a.max(), b.max()), max(np.percentile(a, 95), np.percentile(b, 95)), (a.sum() + b.sum()) / (a.size + b.size))
    return out


def volume_rows(shape, order, spacing, lines, host):
    pairs = inputs(shape, order)
    v = int(np.prod(shape))
    lines.append(f"{shape} {order}-ordered uint8 pair, strides {tuple(pairs[0][0].stride())}, {v} voxels, spacing {spacing}")
    edges = [surface.surface_mask(t, 2) for _, t in pairs]
    corner = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    corner[0, 0, 0] = 1
    lines.append(row("distance_to(the surface of class 2), squared", timed(lambda i: surface.distance_to(edges[i], spacing, squared=True))))
    lines.append(row("distance_to(the foreground of the map), squared", timed(lambda i: surface.distance_to(pairs[i][1], spacing, squared=True))))
    lines.append(row("distance_to(one voxel in a corner), squared: the longest walks", timed(lambda i: surface.distance_to(corner, spacing, squared=True))))
    call = lambda i: surface.surface_distances(pairs[i][0], pairs[i][1], classes=CLASSES, spacing=spacing)  # noqa: E731
    lines.append(row(f"surface_distances, classes {CLASSES}, total ({2 + 4 * len(CLASSES)} kernels, {1 + len(CLASSES)} fills)", timed(call)))
    try:
        per = kernel_times(call)
    except Exception as ex:          # the profiler is an optional part of the torch build
        per = {}
        lines.append(f"  kernel rows: not measured ({type(ex).__name__}: {ex})")
    for k in KERNELS:
        if per.get(k):
            lines.append(row(f"  {k}, all launches of a call", per[k]))
    got = surface.surface_metrics(call(0))
    for c in CLASSES:
        m = got[c]
        lines.append(f"  class {c}: hd {m['hd']:.4f} hd95 {m['hd95']:.4f} assd {m['assd']:.4f} nsd(1 mm) {m['nsd'][0]:.4f} surface voxels "
                     f"{m['n_pred']} / {m['n_target']}")
    if not host:
        return
    try:
        from scipy import ndimage
    except ImportError:
        lines.append("  host route: not measured (scipy does not import here)")
        return
    p, t = pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy()
    t0 = time.perf_counter()
    want = host_route(p, t, spacing, ndimage)
    took = time.perf_counter() - t0
    worst = max(abs(got[c][key] - w) / max(w, 1e-300) for c in CLASSES for key, w in zip(("hd", "hd95", "assd"), want[c]))
    lines.append(f"  {'host route: binary_erosion + distance_transform_edt per class and direction, once':66s} {took * 1e6:10.1f} us"
                 f"  largest relative difference of hd, hd95, assd: {worst:.2e}")


class Lines(list):
    """The rows, printed as they come."""

    def append(self, s):
        print(s, flush=True)
        super().append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the rows to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_surface.py needs a GPU (there is no CPU fallback)")
    lines = Lines()
    lines.append(f"tools/time_surface.py: device events, {WARM} warm-up + {REPS} timed repeats over {NVOL} input sets, median (min .. max); "
                 f"{torch.cuda.get_device_name(0)}")
    for shape, order, spacing in (((192, 192, 192), "C", (1.0, 1.0, 1.0)), ((512, 512, 100), "F", (0.782, 0.782, 5.0))):
        volume_rows(shape, order, spacing, lines, not a.no_host)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
