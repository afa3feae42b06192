"""Time the outbound half at the size a user runs it: python tools/time_segment.py [--out FILE]

Device events, one pair per repeat, 3 warm-up + 10 timed repeats; every row gives the median and the spread (min .. max) of the
repeats.  Where two routes are compared they run in the same process, alternating repeat by repeat.  Bytes are algorithmic, from
the shapes; "of peak" is bytes / 8 TB/s (HBM is the bound of every kernel here) over the median.

  1. the label route against the route it replaces, 192^3, N = 1, bf16:
       new       segment.predict_labels(model, x, target)                     (infer with logits = NULL, then head + argmax + counts)
       replaced  model(x) -> torch.argmax(dim=1) -> metrics.class_counts      (logits written, re-read twice, int64 map written)
  2. the head + argmax + counts kernel alone (mi3d_head_labels on a bf16 decoder output with 16 channels, target given):
     (2 * 16 + 1 + 8) B per voxel.  Two inputs of 283 MB each alternate, so a timed read is not a re-hit of the Infinity Cache.
  3. the restore kernel, 192^3 -> 512 x 512 x 100 uint8: C-ordered and Fortran-ordered destination, identity and one flipped and
     permuted orientation each; 26 MB written + 7 MB read (the 7 MB source stays in the Infinity Cache between repeats, as it
     would right after predict_labels).  The rows time the kernel through the C entry point with the tables uploaded once; one more
     row gives resample.restore_labels as a caller sees it (orientation algebra in numpy, one allocation, the launch).
  4. the device-to-host copy a caller waits for: the 7 MB uint8 map, and the 57 MB int64 map of the replaced route."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import multimodal_segmentation_project_amd as mi  # noqa: E402
from multimodal_segmentation_project_amd import _lib, metrics, resample, segment  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr  # noqa: E402
import orient_ref  # noqa: E402      affine_for: the affine of a stored array with a given axis order and directions

PEAK = 8e12
WARM, REPS = 3, 10
GRID = (192, 192, 192)
STORED = (512, 512, 100)


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


def label_routes(lines):
    torch.manual_seed(0)
    model = mi.UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).cuda().eval()
    model.compute_dtype = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((1, 1) + GRID, device="cuda", generator=g)
    target = torch.randint(0, 4, (1, 1) + GRID, device="cuda", generator=g)

    def new(i):
        return segment.predict_labels(model, x, target)

    def old(i):
        with torch.no_grad():
            logits = model(x)
        return torch.argmax(logits, dim=1), metrics.class_counts(logits, target)

    labels, counts = new(0)
    pred, total = old(0)
    same = bool(torch.equal(labels.long(), pred)) and bool(torch.equal(counts.sum(0), total))
    t_new, t_old = timed([new, old])
    lines.append(f"label route, {GRID} N = 1 bf16 (labels and counts of the two routes equal: {same})")
    lines.append(row("new: predict_labels with a target", t_new))
    lines.append(row("replaced: model(x) -> torch.argmax -> metrics.class_counts", t_old))
    d = statistics.median(t_new) - statistics.median(t_old)
    lines.append(f"  new - replaced (medians): {d:+.1f} us; spread of the replaced route: {max(t_old) - min(t_old):.1f} us")
    return labels, pred


def head_kernel(lines):
    v, cin, c = int(np.prod(GRID)), 16, 4
    g = torch.Generator(device="cuda").manual_seed(1)
    zs = [torch.randn((1, v, cin), device="cuda", generator=g).to(torch.bfloat16) for _ in range(2)]
    ts = [torch.randint(0, c, (1, v), device="cuda", generator=g) for _ in range(2)]
    w, b = torch.randn((c, cin), device="cuda", generator=g) * 0.3, torch.randn(c, device="cuda", generator=g) * 0.1
    out = torch.empty((1, v), dtype=torch.uint8, device="cuda")
    counts = torch.empty((1, 3 * c + 1), dtype=torch.int64, device="cuda")
    ws = torch.empty(_lib.lib().mi3d_head_labels_workspace_bytes(1, c), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def fn(i):
        call("mi3d_head_labels", 1, ptr(zs[i % 2]), cin, cin, ptr(w), ptr(b), c, 1, v, ptr(out), ptr(ts[i % 2]), ptr(counts), ptr(ws), s)

    (us,) = timed([fn])
    lines.append("head + argmax + counts kernel (with its per-sample finalize launch), bf16, Cin = 16, 4 classes, target given")
    lines.append(row(f"mi3d_head_labels, {v} voxels", us, (2 * cin + 1 + 8) * v))


def restore_kernel(lines, labels):
    grid = labels[0].contiguous()
    nbytes = int(np.prod(STORED)) + int(np.prod(GRID))
    lines.append(f"restore kernel (mi3d_restore_labels3, tables uploaded once), {GRID} -> {STORED} uint8")
    s = torch.cuda.current_stream().cuda_stream
    for order in ("C", "F"):
        d, h, w = STORED
        strides = (h * w, w, 1) if order == "C" else (1, d, d * h)
        for perm, signs in (((0, 1, 2), (1, 1, 1)), ((2, 0, 1), (-1, 1, -1))):
            aff = orient_ref.affine_for(perm, signs)
            ras_shape, ras_strides, host = resample.restore_tables(GRID, aff, STORED, strides)
            tabs = [torch.from_numpy(t).cuda() for t in host]
            outs = [torch.empty_strided(STORED, strides, dtype=torch.uint8, device="cuda") for _ in range(2)]

            def kernel(i):
                call("mi3d_restore_labels3", ptr(grid), *GRID, ptr(outs[i % 2]), *ras_shape, *ras_strides, ptr(tabs[0]), ptr(tabs[1]),
                     ptr(tabs[2]), s)

            (us,) = timed([kernel])
            assert torch.equal(outs[0], resample.restore_labels(grid, aff, (STORED, strides)))
            lines.append(row(f"{order}-ordered destination, stored axes {perm} directions {signs}", us, nbytes))
    d, h, w = STORED
    aff, layout = orient_ref.affine_for((2, 0, 1), (-1, 1, -1)), (STORED, (1, d, d * h))
    (us,) = timed([lambda i: resample.restore_labels(grid, aff, layout)])
    lines.append(row("resample.restore_labels with its host side, F-ordered, stored axes (2, 0, 1)", us))


def host_copies(lines, labels, pred):
    t_u8, t_i64 = timed([lambda i: labels.cpu(), lambda i: pred.cpu()])
    lines.append("device-to-host copy of the label map (tensor.cpu(), pageable host memory)")
    lines.append(row(f"uint8 {tuple(labels.shape)}", t_u8, labels.numel()))
    lines.append(row(f"int64 {tuple(pred.shape)} (the replaced route)", t_i64, pred.numel() * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the rows to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_segment.py needs a GPU (there is no CPU fallback)")
    lines = [f"tools/time_segment.py: device events, {WARM} warm-up + {REPS} timed repeats, median (min .. max); "
             f"{torch.cuda.get_device_name(0)}"]
    labels, pred = label_routes(lines)
    head_kernel(lines)
    restore_kernel(lines, labels)
    host_copies(lines, labels, pred)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
