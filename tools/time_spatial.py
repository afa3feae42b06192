"""Time the spatial augmentation at the training grid: python tools/time_spatial.py [--no-scipy]

One 192^3 sample, float32 image + int64 label, (C, D, H, W) = (1, 192, 192, 192).  Device events, 3 warm-up + 20 timed repeats
that rotate over 3 distinct input pairs.  A repeat reads 85 MB and writes 85 MB; between two uses of one input pair the loop
moves 425 MB of other data (two other pairs read, three outputs written), more than the 256 MB Infinity Cache, so a timed read
is not a re-hit of what the previous use left there.  Bytes are algorithmic (image 4 B and label 8 B per voxel, each read
once and written once); the last column is the fraction of bytes / 8 TB/s that was achieved.  The time includes the host side
of the call (two output allocations, the ctypes launch).  Where scipy imports, the same calls are timed once on the CPU."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_segmentation_project_amd import spatial  # noqa: E402

PEAK = 8e12
NVOL, WARM, REPS = 3, 3, 20
SHAPE = (1, 192, 192, 192)
ANGLE = 11.0


def timed(fn):
    """fn(i) runs one repeat on sample i % NVOL; returns microseconds per repeat."""
    for i in range(WARM):
        fn(i % NVOL)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(REPS):
        fn(i % NVOL)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_spatial.py needs a GPU (there is no CPU fallback)")
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.rand(SHAPE, device="cuda", generator=g) for _ in range(NVOL)]
    labs = [torch.randint(0, 4, SHAPE, device="cuda", generator=g) for _ in range(NVOL)]
    n = int(np.prod(SHAPE))
    both, image_only = 2 * (4 + 8) * n, 2 * 4 * n
    flips = (True, False, True)
    rows = [(f"rotate {ANGLE} deg, plane {p}", timed(lambda i, p=p: spatial.flip_rotate(imgs[i], labs[i], angle=ANGLE, axes=p)), both)
            for p in spatial.PLANES]
    rows.append(("pure flip (D and W)", timed(lambda i: spatial.flip_rotate(imgs[i], labs[i], flips=flips)), both))
    rows += [(f"flip + rotate fused, plane {p}",
              timed(lambda i, p=p: spatial.flip_rotate(imgs[i], labs[i], flips=flips, angle=ANGLE, axes=p)), both) for p in spatial.PLANES]
    rows.append(("rotate, plane (1, 2), image only", timed(lambda i: spatial.flip_rotate(imgs[i], None, angle=ANGLE, axes=(1, 2))), image_only))
    rows.append(("rotate, plane (2, 3), image only", timed(lambda i: spatial.flip_rotate(imgs[i], None, angle=ANGLE, axes=(2, 3))), image_only))
    print(f"spatial augmentation of one {SHAPE} float32 image + int64 label")
    for what, us, nbytes in rows:
        print(f"  {what:40s} {us:10.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / us / 1e6:7.3f} TB/s  "
              f"{nbytes / PEAK * 1e6 / us:6.3f} of bytes / 8 TB/s")
    if "--no-scipy" in sys.argv:
        return
    try:
        from scipy.ndimage import rotate
    except ImportError:
        print("  scipy: not available")
        return
    x, lab = imgs[0].cpu().numpy(), labs[0].cpu().numpy()
    for p, (what, us, _) in zip(spatial.PLANES, rows):
        t0 = time.perf_counter()
        rotate(x, ANGLE, axes=p, reshape=False, order=1, mode="nearest")
        rotate(lab, ANGLE, axes=p, reshape=False, order=0, mode="nearest")
        cpu = time.perf_counter() - t0
        print(f"  scipy (one core), the same two rotate calls, plane {p}: {cpu:.2f} s = {cpu * 1e6 / us:.0f} x the device time")


if __name__ == "__main__":
    main()
