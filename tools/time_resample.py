"""Time the resampling kernels at real scan sizes: python tools/time_resample.py [--no-scipy]

Two scans: an AMOS-like CT (512x512x100 at 0.7x0.7x5.0 mm -> 358x358x500 -> 192^3) and an MRI-like volume that is
upsampled on every axis (256x256x30 at 1.7x1.7x8.0 mm -> 435x435x240 -> 192^3).  Device events, 3 warm-up + 20 timed
repeats that rotate over 3 distinct input volumes.  For the CT case (105 MB inputs, 256 MB intermediates) no timed read
can re-hit what the previous repeat left in the 256 MB Infinity Cache; the MRI inputs are 7.9 MB each, so all three stay
cached and that case's stage-1 row times a cached read (its 182 MB write dominates the bytes).  Bytes are algorithmic (input read once + output written once); the last column is the fraction of
bytes / 8 TB/s that was achieved.  Where scipy imports, the same chain is timed once on the CPU for the ratio.

Then the same CT AS STORED (int16, one flip), once for each axis that can be fastest in memory, three ways: (a) what a caller had
to do before resample_scan existed, torch.flip(x.permute(...), dims).contiguous().float() and then resample_to_grid, copy and
chain timed separately; (b) reorient_to_ras + the chain; (c) stage 1 reading the stored tensor in place.  Each row is timed
SPREAD times and printed as median [min .. max].  Last, the 4-mask merge against the torch sequence it replaces."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_segmentation_project_amd import resample  # noqa: E402

PEAK = 8e12
NVOL, WARM, REPS = 3, 3, 20


def timed(fn):
    """fn(i) runs one repeat on volume i % NVOL; returns microseconds per repeat."""
    for i in range(WARM):
        fn(i % NVOL)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(REPS):
        fn(i % NVOL)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3


def case(name, shape, spacing, use_scipy):
    target = (192, 192, 192)
    fac1, shape1, fac2 = resample.chain_shapes(shape, spacing)
    n0, n1, n2 = (int(np.prod(s)) for s in (shape, shape1, target))
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = [torch.rand(shape, device="cuda", generator=g) * 2500.0 - 1000.0 for _ in range(NVOL)]
    labs = [torch.randint(0, 16, shape, device="cuda", generator=g) for _ in range(NVOL)]
    mids = [resample.zoom(x, fac1, order=3) for x in imgs]
    print(f"{name}: {shape} at {spacing} mm -> {shape1} -> {target}")
    rows = [("stage 1 (cubic, to 1 mm)", timed(lambda i: resample.zoom(imgs[i], fac1, order=3)), 4 * (n0 + n1)),
            ("stage 2 (cubic, to 192^3)", timed(lambda i: resample.zoom(mids[i], fac2, order=3)), 4 * (n1 + n2)),
            ("image chain (stage 1 + stage 2)", timed(lambda i: resample.resample_to_grid(imgs[i], spacing)), 4 * (n0 + 2 * n1 + n2)),
            ("image chain + fused CT window", timed(lambda i: resample.resample_to_grid(imgs[i], spacing, ct_window=(-160.0, 240.0))),
             4 * (n0 + 2 * n1 + n2)),
            ("label gather (both stages composed)", timed(lambda i: resample.resample_labels_to_grid(labs[i], spacing)), 16 * n2)]
    for what, us, nbytes in rows:
        print(f"  {what:40s} {us:10.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / us / 1e6:7.3f} TB/s  "
              f"{nbytes / PEAK * 1e6 / us:6.3f} of bytes / 8 TB/s")
    total = rows[2][1] + rows[4][1]
    print(f"  image chain + label gather: {total / 1e3:.3f} ms per scan")
    if use_scipy:
        try:
            from scipy.ndimage import zoom
        except ImportError:
            print("  scipy: not available")
            return total
        x, lab = imgs[0].cpu().numpy().astype(np.float64), labs[0].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        y1 = zoom(x, fac1, order=3, mode="nearest", prefilter=False)
        zoom(y1, fac2, order=3, mode="nearest", prefilter=False)
        l1 = zoom(lab, fac1, order=0, mode="nearest", prefilter=False)
        zoom(l1, fac2, order=0, mode="nearest", prefilter=False)
        cpu = time.perf_counter() - t0
        print(f"  scipy (one core, float64), same four calls: {cpu:.1f} s = {cpu * 1e6 / total:.0f} x the device time")
    return total


SPREAD = 3


def spread(fn):
    t = sorted(timed(fn) for _ in range(SPREAD))
    return t[SPREAD // 2], t[0], t[-1]


def stored_cases():
    from multimodal_segmentation_project_amd import orientation
    ras_shape, ras_spacing, target = (512, 512, 100), (0.7, 0.7, 5.0), (192, 192, 192)
    g = torch.Generator(device="cuda").manual_seed(1)
    ras = [(torch.rand(ras_shape, device="cuda", generator=g) * 2500.0 - 1000.0).to(torch.int16) for _ in range(NVOL)]
    organ = [[(torch.rand(ras_shape, device="cuda", generator=g) < 0.2).to(torch.uint8) for _ in range(4)] for _ in range(NVOL)]
    print(f"AMOS-like CT as stored: int16, RAS shape {ras_shape} at {ras_spacing} mm, one flipped axis; us as median [min .. max] of {SPREAD} runs")
    # perm: stored axis i is RAS axis perm[i]; the LAST stored axis is the fastest in memory
    for name, perm, flip_ax in (("W (C-ordered RAS)", (0, 1, 2), 0), ("H", (0, 2, 1), 1), ("D (a Fortran-ordered RAS array)", (2, 1, 0), 2)):
        inv = tuple(int(i) for i in np.argsort(perm))
        signs = [-1.0 if i == flip_ax else 1.0 for i in range(3)]
        aff = np.eye(4)
        aff[:3, :3] = 0.0
        for i in range(3):
            aff[perm[i], i] = signs[i] * ras_spacing[perm[i]]

        def store(v):
            return torch.flip(v.permute(*perm), (flip_ax,)).contiguous()

        def to_ras(x):          # what the parent commit's caller does on the device
            return torch.flip(x.permute(*inv), (perm[flip_ax],)).contiguous().float()

        xs = [store(v) for v in ras]
        spacing = orientation.spacing_of(orientation.reoriented_affine(aff, tuple(xs[0].shape)))
        copies = [to_ras(x) for x in xs]
        want = resample.resample_to_grid(copies[0], spacing)
        for form in resample.STAGE1_FORMS:
            assert torch.equal(resample.resample_scan(xs[0], aff, stage1=form)[0], want), form
        assert torch.equal(resample.reorient_to_ras(xs[0], aff)[0], copies[0])
        print(f"  memory-fastest RAS axis {name}: stored shape {tuple(xs[0].shape)}")
        rows = [("(a) torch flip + permute + contiguous + float", spread(lambda i: to_ras(xs[i]))),
                ("(a) chain on that copy (parent's resample_to_grid)", spread(lambda i: resample.resample_to_grid(copies[i], spacing))),
                ("(a) copy + chain", spread(lambda i: resample.resample_to_grid(to_ras(xs[i]), spacing))),
                ("    reorient_to_ras alone", spread(lambda i: resample.reorient_to_ras(xs[i], aff))),
                ("(b) resample_scan, stage1='reorient'", spread(lambda i: resample.resample_scan(xs[i], aff, stage1="reorient"))),
                ("(c) resample_scan, stage1='fused'", spread(lambda i: resample.resample_scan(xs[i], aff, stage1="fused")))]
        for what, (med, lo, hi) in rows:
            print(f"    {what:52s} {med:10.1f} us  [{lo:10.1f} .. {hi:10.1f}]")
        if perm == (2, 1, 0):
            ms = [[store(m) for m in vol] for vol in organ]
            values = (1, 2, 3, 3)

            def torch_merge(i):
                out = torch.zeros(target, dtype=torch.int64, device="cuda")
                for m, v in zip(ms[i], values):
                    lab = resample.resample_labels_to_grid(torch.flip(m.permute(*inv), (perm[flip_ax],)).contiguous().long(), spacing)
                    out[lab > 0] = v
                return out

            def merge(i):
                return resample.merge_masks_to_grid(list(zip(ms[i], values)), aff)

            assert torch.equal(torch_merge(0), merge(0))
            for what, (med, lo, hi) in (("4-mask merge, torch: 4 x (copy + long + gather + assign)", spread(torch_merge)),
                                        ("4-mask merge, merge_masks_to_grid (one gather)", spread(merge))):
                print(f"    {what:52s} {med:10.1f} us  [{lo:10.1f} .. {hi:10.1f}]")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_resample.py needs a GPU (there is no CPU fallback)")
    use_scipy = "--no-scipy" not in sys.argv
    case("AMOS-like CT", (512, 512, 100), (0.7, 0.7, 5.0), use_scipy)
    case("MRI-like, upsampled on every axis", (256, 256, 30), (1.7, 1.7, 8.0), use_scipy)
    stored_cases()


if __name__ == "__main__":
    main()
