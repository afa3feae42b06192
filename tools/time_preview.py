"""Time the preview figure at the sizes a user runs it: python tools/time_preview.py [--out FILE] [--no-host]

Device events, one pair per repeat, 3 warm-up + 10 timed repeats that rotate over 3 distinct input sets (at 192^3 a set is 28 MB
of float32 image + 57 MB of int64 label + 7 MB of uint8 prediction, so between two uses of one set more than the 256 MB Infinity
Cache passes through); every row gives the median and the spread (min .. max).  Times include the host side of the call (output
and workspace allocation, the ctypes launches).  Bytes are algorithmic, from the shapes: what the call must read and write once;
"of peak" is bytes / 8 TB/s over the median (HBM bounds every kernel here).

Volumes: the (192, 192, 192) training grid, C-ordered, and a (512, 512, 100) scan as stored, C-ordered and Fortran-ordered.
  profile pass   preview.foreground_profiles, int64 and uint8 labels
  panel set      preview.prediction_panels (float64 panels, int64 label, uint8 prediction): profiles, best slices, min / max, render
  stack          preview.overlay_stack along axis 2, uint8 and float32 (per-slice min / max, then the render), and its first launch alone
Beside them the route the reference takes (test_model.py:299-305): .cpu() of the image, the int64 label and the int64 prediction
(pageable host memory, host clock around the copies, which end synchronised), then the numpy restatement of visualize_prediction's
arithmetic (tests/preview_ref.py, no drawing), and for the slider of visualize_nifti.py the restatement of every slice's overlay as
uint8, run once."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from multimodal_segmentation_project_amd import _lib, preview  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr, stream_ptr  # noqa: E402
import preview_ref  # noqa: E402

PEAK = 8e12
NVOL, WARM, REPS = 3, 3, 10
VOLUMES = (((192, 192, 192), "C"), ((512, 512, 100), "C"), ((512, 512, 100), "F"))


def timed(fn):
    """fn(i) runs one repeat on input set i % NVOL; returns the REPS times in microseconds."""
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


def host_timed(fn, reps):
    """Host clock around fn(i), which must end synchronised; microseconds."""
    out = []
    for i in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i % NVOL)
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def row(what, us, nbytes=None):
    med = statistics.median(us)
    s = f"  {what:66s} {med:11.1f} us  (min {min(us):.1f} .. max {max(us):.1f})"
    if nbytes is not None:
        s += f"  {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e6:6.3f} TB/s  {nbytes / PEAK * 1e6 / med:6.3f} of peak (HBM, 8 TB/s)"
    return s


def laid_out(t, order):
    return t if order == "C" else t.permute(2, 1, 0).contiguous().permute(2, 1, 0)


def minmax_alone(image, axis):
    """The first of overlay_stack's two launches: the zeroed keys and mi3d_slice_minmax for every slice of the axis."""
    keys = torch.zeros(2 * image.shape[axis], dtype=torch.int32, device=image.device)
    call("mi3d_slice_minmax", ptr(image), _lib.SRC_F32, *image.shape, *image.stride(), axis, _lib.PREVIEW_STACK, None, 0, ptr(keys),
         stream_ptr())
    return keys


def volume_rows(shape, order, lines, host):
    g = torch.Generator(device="cuda").manual_seed(0)
    n = int(np.prod(shape))
    images = [laid_out(torch.randn(shape, device="cuda", generator=g) * 300.0, order) for _ in range(NVOL)]
    labels = [laid_out(torch.randint(0, 4, shape, device="cuda", generator=g), order) for _ in range(NVOL)]
    labels8 = [t.to(torch.uint8) for t in labels]                  # elementwise: keeps the strides
    preds = [laid_out(torch.randint(0, 4, shape, device="cuda", generator=g, dtype=torch.uint8), order) for _ in range(NVOL)]
    assert all(t.stride() == images[0].stride() for t in labels8 + preds)
    d, h, w = shape
    panel_px = d * h + h * w + d * w
    lines.append(f"{shape} {order}-ordered, strides {tuple(images[0].stride())}")
    lines.append(row("profile pass, int64 label", timed(lambda i: preview.foreground_profiles(labels[i])), 8 * n))
    lines.append(row("profile pass, uint8 label", timed(lambda i: preview.foreground_profiles(labels8[i])), n))
    lines.append(row("panel set, float64 (int64 label, uint8 prediction)",
                     timed(lambda i: preview.prediction_panels(images[i], labels[i], preds[i])), 8 * n + panel_px * (4 + 8 + 1 + 4 + 48)))
    lines.append(row("per-slice min / max along axis 2 alone (the stack's first launch)", timed(lambda i: minmax_alone(images[i], 2)), 4 * n))
    lines.append(row("stack along axis 2, uint8 (uint8 label)",
                     timed(lambda i: preview.overlay_stack(images[i], labels8[i], axis=2)), n * (4 + 4 + 1 + 3)))
    lines.append(row("stack along axis 2, float32 (uint8 label)",
                     timed(lambda i: preview.overlay_stack(images[i], labels8[i], axis=2, dtype=torch.float32)), n * (4 + 4 + 1 + 12)))
    if not host:
        return
    preds64 = [t.long() for t in preds]
    copies = host_timed(lambda i: (images[i].cpu(), labels[i].cpu(), preds64[i].cpu()), REPS)
    lines.append(row("reference route: .cpu() of image, int64 label, int64 prediction", copies, (4 + 8 + 8) * n))
    hi, hl, hp = images[0].cpu().numpy(), labels[0].cpu().numpy(), preds64[0].cpu().numpy()
    lines.append(row("reference route: numpy restatement of the nine panels", host_timed(lambda i: preview_ref.panels(hi, hl, hp), 3)))

    def slider(i):
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in range(shape[2]):
                preview_ref.as_dtype(preview_ref.overlay(hi[:, :, k], hl[:, :, k]), np.uint8)

    lines.append(row("reference route: numpy overlay of every slice of axis 2, as uint8", host_timed(slider, 1)))
    got, best = preview.prediction_panels(images[0], labels[0], preds[0])
    want, want_best = preview_ref.panels(hi, hl, hp)
    same = np.array_equal(best.cpu().numpy(), want_best) and all(
        np.array_equal(t.cpu().numpy(), w, equal_nan=True) for t, w in zip([t for r in got for t in r], want))
    lines.append(f"  panels and indices of the two routes equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the rows to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the reference's host route")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_preview.py needs a GPU (there is no CPU fallback)")
    lines = [f"tools/time_preview.py: device events, {WARM} warm-up + {REPS} timed repeats over {NVOL} input sets, median (min .. max); "
             f"{torch.cuda.get_device_name(0)}"]
    for shape, order in VOLUMES:
        volume_rows(shape, order, lines, not a.no_host)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
