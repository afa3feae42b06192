"""Time the foreground-balanced patch sampler (spatial.pick_starts / crop_patches / RandCropByPosNegLabel, csrc/patch.hip) on one 192^3
scan -> K = 2 and 4 patches of 96^3, against the torch route on the same card (torch.nonzero -> index -> .tolist() -> K slices ->
torch.stack):

    python tools/time_patch.py [--reps 30] [--size 192] [--only-ours]

Device events around every single call, after warm-up; median, minimum and maximum over the repetitions.  "of 8 TB/s" is the bytes
the kernel has to move (counted below from the shapes) over the time, as a share of the card's 8 TB/s HBM peak.  The three entries are
timed one by one on preallocated buffers; the whole call includes its allocations and the host draws.  The torch route synchronises
twice per call (the row count of nonzero, the .tolist()); its spread is printed beside its median."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_segmentation_project_amd import _lib, spatial  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr, stream_ptr  # noqa: E402

PEAK = 8e12
DEV = "cuda"
POS_NEG = [0] + [1] * 255


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us), min(us), max(us)


def row(name, t, nbytes=None):
    med, lo, hi = t
    share = f"{nbytes / (med * 1e-6) / PEAK * 100:6.2f} % of 8 TB/s ({nbytes / 1e6:.2f} MB)" if nbytes else ""
    print(f"{name:74s} {med:10.1f} us  [{lo:9.1f} .. {hi:9.1f}]  {share}", flush=True)


def entries(lab, k, size, reps, tag):
    """mi3d_patch_count and mi3d_patch_pick on one label map (D, H, W), each alone on preallocated buffers."""
    t = lab[None]
    code = _lib.SRC_U8 if lab.dtype == torch.uint8 else _lib.SRC_I64
    strides = [max(int(s), 1) for s in t.stride()]
    table = (C.c_uint8 * 256)(*POS_NEG)
    nbytes = _lib.lib().mi3d_patch_workspace_bytes(*t.shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    counts = torch.empty((1, 2), dtype=torch.int64, device=DEV)
    starts, voxel, picked = (torch.empty(s, dtype=torch.int32, device=DEV) for s in ((k, 3), (k,), (k,)))
    rng = np.random.RandomState(0)
    sample, group = (C.c_int32 * k)(*[0] * k), (C.c_int32 * k)(*[1] * k)
    rnd = (C.c_uint64 * k)(*[int(rng.randint(0, 2 ** 64, dtype=np.uint64)) for _ in range(k)])
    v, blocks = lab.numel(), -(-lab.numel() // spatial.PATCH_BLOCK)
    row(f"ours: count {tag}, 1 launch + the memset of the counts",
        timed(lambda: call("mi3d_patch_count", ptr(t), code, *t.shape, *strides, table, ptr(counts), ptr(ws), nbytes, stream_ptr()), reps),
        v * lab.element_size() + 8 * 4 * blocks)
    # per draw: the group's block counts, then the one block of labels
    row(f"ours: pick K = {k} {tag}, 1 launch",
        timed(lambda: call("mi3d_patch_pick", ptr(t), code, *t.shape, *strides, table, k, sample, group, rnd, _lib.int_table(size),
                           ptr(starts), ptr(voxel), ptr(picked), ptr(ws), nbytes, stream_ptr()), reps),
        k * (4 * blocks + spatial.PATCH_BLOCK * lab.element_size()))
    return starts


def torch_route(x, lab, k, size, rng):
    """What a user writes today: the index list of the foreground, K rows of it on the host, K slices, one stack."""
    idx = torch.nonzero(lab[0] > 0)                                   # synchronises: the row count
    rows = idx[torch.from_numpy(rng.randint(0, idx.shape[0], k))].tolist()      # synchronises: the copy to the host
    img, out = [], []
    for centre in rows:
        st = [min(max(c - s // 2, 0), n - s) for c, s, n in zip(centre, size, lab.shape[1:])]
        sl = (slice(None),) + tuple(slice(a, a + s) for a, s in zip(st, size))
        img.append(x[sl])
        out.append(lab[sl])
    return torch.stack(img), torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--only-ours", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_patch.py measures on the GPU"
    big, half = (a.size,) * 3, (a.size // 2,) * 3
    gen = torch.Generator().manual_seed(0)
    x = torch.rand((1,) + big, generator=gen).to(DEV)
    lab64 = torch.zeros((1,) + big, dtype=torch.int64)
    q = a.size // 4
    lab64[0, q:2 * q, q // 2:q + q // 2, 2 * q:3 * q] = torch.randint(1, 4, (q, q, q), generator=gen)      # 1.6 % foreground, off centre
    lab64 = lab64.to(DEV)
    lab8 = lab64.to(torch.uint8)
    lab8f = lab8[0].permute(2, 1, 0).contiguous().permute(2, 1, 0)                                        # Fortran order: D fastest
    assert lab8f.stride() == (1, a.size, a.size * a.size) and torch.equal(lab8f, lab8[0])
    print(f"{torch.cuda.get_device_name(0)}; {a.reps} repetitions, median [min .. max]; {a.size}^3 -> K patches of {half[0]}^3, "
          f"{float((lab64 > 0).float().mean()) * 100:.2f} % foreground")
    vo = float(np.prod(half))
    for k in (2, 4):
        for tag, lab in (("int64 C order", lab64[0]), ("uint8 C order", lab8[0]), ("uint8 Fortran order (strided)", lab8f)):
            starts = entries(lab, k, half, a.reps, tag)
        # image + label read once over the windows and written once
        row(f"ours: crop K = {k} (image + label), 1 launch", timed(lambda: spatial.crop_patches(x, lab64, starts, half), a.reps),
            2 * k * vo * (4 + 8))
        for tag, lab in (("int64 label", lab64), ("uint8 label", lab8)):
            tf = spatial.RandCropByPosNegLabel(half, pos=1.0, neg=1.0, num_samples=k).set_random_state(0)
            sample = {"image": x, "label": lab}
            row(f"ours: RandCropByPosNegLabel K = {k}, {tag}, whole call (draws + count + pick + crop)", timed(lambda: tf(sample), a.reps))
        if not a.only_ours:
            rng = np.random.RandomState(0)
            row(f"torch: nonzero -> index -> tolist -> {k} slices -> stack (int64 label)", timed(lambda: torch_route(x, lab64, k, half, rng), a.reps))


if __name__ == "__main__":
    main()
