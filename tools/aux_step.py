#!/usr/bin/env python3
"""Diagnostic (round 4): aux-stream weight gradients on / off IN ONE PROCESS (two step objects on identically seeded models,
TrainStep(aux_wgrad=True / False), timed in alternating blocks): ms per step, four rounds.  python tools/aux_step.py"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import multimodal_segmentation_project_amd as mi  # noqa: E402
from multimodal_segmentation_project_amd.trainer import TrainStep  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    x, y = bench.synth(2, 96, 1234)
    steps = {}
    for name, aux in (("aux", True), ("chain", False)):
        torch.manual_seed(0)
        model = mi.UNet3D(in_channels=1, out_channels=4, dropout_rate=0.0).to(dev).train()
        ts = TrainStep(model, loss="combined", lr=1e-3, weight_decay=0.01, compute_dtype=torch.bfloat16, use_graph=False,
                       aux_wgrad=aux)
        ts.load_batch(x.to(dev), y.to(dev))
        steps[name] = ts

    def run(ts, n=40):
        for _ in range(3):
            ts.step_static()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts.step_static()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for rep in range(4):
        print("   ".join(f"{name} {run(ts):.4f}" for name, ts in steps.items()), flush=True)


if __name__ == "__main__":
    main()
