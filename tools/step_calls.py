#!/usr/bin/env python3
"""The library calls of a step, as text that two trees can be diffed on.

    python tools/step_calls.py --out calls.txt          every configuration, one child process each (its own time limit)
    python tools/step_calls.py --config train_bf16      one configuration, to stdout (--append FILE: to the end of FILE)

A configuration runs three micro-steps of one host path (TrainStep, DannStep, evaluate, model(x) through autograd,
predict_labels) on UNet3D(1->4), N = 2, 32^3.  `_lib.lib` is replaced with a recording proxy, and DataParallelComm.reduce_bucket,
DataParallelComm.average_ and torch.cuda.Stream.wait_stream are wrapped; nothing else of the package is touched, so the same
file runs against any tree that has these names.  One line per call: the name, scalars as given, structs as bytes, every
pointer / stream / event as p<index of its first appearance in the run>, pointer tables element by element (consecutive indices
as a..b).  Size and capability queries (no stream, no device memory) are listed at the end as sorted counts: their order
is not behaviour.  The stream probe (trainer.concurrent_stream) launches a number of stand-in kernels that depends on its own
timing: recording pauses inside it.
"""
import argparse
import collections
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG_SECONDS = 150
_QUERY_ENDS = ("_bytes", "_count", "_supported", "_params", "_buffers", "_segments", "_get_route", "_last_error")


class Recorder:
    def __init__(self, real, sigs):
        self.real, self.sigs = real, sigs
        self.ids, self.lines, self.queries, self.paused = {}, [], collections.Counter(), 0

    def h(self, v):
        v = getattr(v, "value", v)
        if not v:
            return "0"
        return "p%d" % self.ids.setdefault(int(v), len(self.ids))

    def table(self, arr):
        out, run = [], []
        for tok in [self.h(e) for e in arr] + [None]:
            if run and tok is not None and tok != "0" and run[-1] != "0" and int(tok[1:]) == int(run[-1][1:]) + 1:
                run.append(tok)
                continue
            if run:
                out.append(run[0] if len(run) == 1 else f"{run[0]}..{run[-1]}")
            run = [tok]
        return "[" + " ".join(out) + "]"

    def fmt(self, typ, a):
        if isinstance(a, C.Array):
            return self.table(a) if a._type_ is C.c_void_p else "[" + " ".join(str(e) for e in a) + "]"
        if typ is C.c_void_p:
            return self.h(a)
        if typ is C.c_char_p:
            return repr(a)
        if isinstance(typ, type) and issubclass(typ, C._Pointer):
            if a is None:
                return "0"
            obj = getattr(a, "_obj", a)          # byref(x) -> x
            if isinstance(obj, C.c_void_p):
                return "out:" + self.h(obj)
            if isinstance(obj, C.Structure):
                return bytes(obj).hex()
            return "out:" + repr(obj.value)
        return repr(a)

    def line(self, text):
        if not self.paused:
            self.lines.append(text)

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        types = self.sigs[name][1]

        def wrapped(*args):
            rc = fn(*args)
            if self.paused:
                return rc
            assert len(args) == len(types), name
            text = name + " " + " ".join(self.fmt(t, a) for t, a in zip(types, args))       # after the call: out-arguments are filled
            if name.endswith(_QUERY_ENDS) or "_num_" in name:
                self.queries[f"{text} -> {rc!r}"] += 1
            else:
                self.lines.append(text)
            return rc
        return wrapped

    def dump(self, out):
        for l in self.lines:
            print(l, file=out)
        for q in sorted(self.queries):
            print(f"query x{self.queries[q]} {q}", file=out)


def install():
    import torch
    from multimodal_segmentation_project_amd import _lib, dp, trainer
    rec = Recorder(_lib.lib(), _lib._SIGS)
    _lib.lib = lambda: rec
    cur = lambda: rec.h(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    reduce_bucket, average_, wait_stream = dp.DataParallelComm.reduce_bucket, dp.DataParallelComm.average_, torch.cuda.Stream.wait_stream
    probe = trainer.concurrent_stream

    def rb(self, seg):
        rec.line(f"reduce_bucket {seg} on {cur()}")
        return reduce_bucket(self, seg)

    def av(self, t):
        rec.line(f"average_ {rec.h(t.data_ptr())} {t.numel()} on {cur()}")
        return average_(self, t)

    def ws(self, other):
        rec.line(f"wait_stream {rec.h(self.cuda_stream)} {rec.h(other.cuda_stream)}")
        return wait_stream(self, other)

    def paused_probe(*a, **kw):
        rec.paused += 1
        try:
            st = probe(*a, **kw)
        finally:
            rec.paused -= 1
        rec.line(f"concurrent_stream {kw.get('role', 'aux')} -> {rec.h(st.cuda_stream)}")
        return st
    dp.DataParallelComm.reduce_bucket, dp.DataParallelComm.average_, torch.cuda.Stream.wait_stream = rb, av, ws
    trainer.concurrent_stream = paused_probe
    return rec


# ---- configurations: name -> (kind, options)
def _train(**kw):
    return ("train", kw)


CONFIGS = {
    "train_bf16": _train(),
    "train_fp32": _train(fp32=True),
    "accum2_last_batch": _train(step=dict(grad_accum=2), last_on_third=True),
    "zero_grad_quirk": _train(step=dict(grad_accum=2, reference_zero_grad_quirk=True)),
    "frozen_encoder": _train(freeze=True),
    "dropout": _train(dropout=0.1),
    "injected_scales": _train(inject=True),
    "keep_logits": _train(step=dict(keep_logits=True)),
    "distill_overlap": _train(teacher=True),
    "distill_serial": _train(teacher=True, step=dict(overlap_teacher=False)),
    "use_graph": _train(step=dict(use_graph=True)),
    "no_aux_wgrad": _train(step=dict(aux_wgrad=False)),
    "evaluate": _train(evaluate=True),
    "evaluate_keep_logits": _train(evaluate=True, step=dict(keep_logits=True)),
    "comm_marks": _train(comm=True),
    "comm_no_marks": _train(comm=True, env=dict(MI3D_NO_MARKS="1")),
    "comm_serial": _train(comm=True, env=dict(MI3D_COMM_SERIAL="1")),
    "comm_graph_segments": _train(comm=True, step=dict(use_graph=True)),
    "comm_accum2": _train(comm=True, step=dict(grad_accum=2)),
    "comm_frozen_encoder": _train(comm=True, freeze=True),
    "comm_fp32": _train(comm=True, fp32=True),
    "dann_overlap_bf16": ("dann", {}),
    "dann_serial_bf16": ("dann", dict(step=dict(overlap_forwards=False))),
    "dann_overlap_fp32": ("dann", dict(fp32=True)),
    "dann_serial_fp32": ("dann", dict(fp32=True, step=dict(overlap_forwards=False))),
    "dann_dropout_accum2": ("dann", dict(dropout=0.1, step=dict(grad_accum=2))),
    "dann_use_graph": ("dann", dict(step=dict(use_graph=True))),
    "dann_evaluate": ("dann", dict(evaluate=True)),
    "dann_comm": ("dann", dict(comm=True)),
    "dann_comm_graph_segments": ("dann", dict(comm=True, step=dict(use_graph=True))),
    "autograd_train": ("autograd", {}),
    "autograd_train_dropout": ("autograd", dict(dropout=0.1)),
    "autograd_train_gap": ("autograd", dict(gap=True)),
    "autograd_eval": ("autograd", dict(eval=True)),
    "predict_labels": ("predict", {}),
    "predict_labels_target": ("predict", dict(target=True)),
}


def run_config(name, out):
    kind, o = CONFIGS[name]
    os.environ.update(o.get("env", {}))
    import torch
    import torch.distributed as dist
    import multimodal_segmentation_project_amd as mi
    from multimodal_segmentation_project_amd import segment, unet_dann
    from multimodal_segmentation_project_amd.dann import DomainDiscriminator
    from multimodal_segmentation_project_amd.trainer import DannStep, TrainStep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if o.get("comm"):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29547")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(2, 1, 32, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 4, (2, 1, 32, 32, 32), generator=g).to(dev)
    xt = torch.rand(2, 1, 32, 32, 32, generator=g).to(dev)
    dt = torch.float32 if o.get("fp32") else torch.bfloat16
    cls = unet_dann.UNet3D if (kind == "dann" or o.get("gap")) else mi.UNet3D
    model = cls(in_channels=1, out_channels=4, dropout_rate=o.get("dropout", 0.0)).to(dev).train()
    rec = install()
    kw = dict(compute_dtype=dt, force_comm=bool(o.get("comm")), **o.get("step", {}))
    if kind == "train":
        if o.get("freeze"):
            for p in model.encoder.parameters():
                p.requires_grad_(False)
        teacher = mi.UNet3D(in_channels=1, out_channels=4).to(dev).eval() if o.get("teacher") else None
        ts = TrainStep(model, loss="combined", kd_teacher=teacher, **kw)
        if o.get("inject"):
            n = ts._prepare(x)["drop"].numel()
            model._mi3d_injected_drop_scales = (torch.rand(n, generator=g) < 0.9).float() / 0.9
        for i in range(3):
            if o.get("evaluate"):
                model.eval()
                ts.evaluate(x, y)
            else:
                ts.step(x, y, last_batch=bool(o.get("last_on_third")) and i == 2)
    elif kind == "dann":
        torch.manual_seed(3)
        disc = DomainDiscriminator(256).to(dev).train()
        ts = DannStep(model, disc, loss="ce_tversky", lambda_domain=0.2, **kw)
        for i in range(3):
            if o.get("evaluate"):
                ts.evaluate(x, y)
            else:
                ts.step(x, y, xt)
    elif kind == "autograd":
        ts = None
        model.compute_dtype = dt
        if o.get("eval"):
            model.eval()
        for i in range(3):
            if o.get("eval"):
                with torch.no_grad():
                    model(x)
                try:        # an eval-mode forward with autograd on, then its refused backward
                    model(x).sum().backward()
                except RuntimeError as e:
                    rec.line(f"raised {type(e).__name__}")
            elif o.get("gap"):
                logits, gap = model(x, return_features=True)
                (logits.sum() + gap.sum()).backward()
            else:
                model(x).sum().backward()
    else:
        ts = None
        model.eval()
        for i in range(3):
            segment.predict_labels(model, x, y if o.get("target") else None)
    torch.cuda.synchronize()
    if ts is not None:
        ts.close()
    print(f"== {name}", file=out)
    rec.dump(out)
    out.flush()
    if o.get("comm"):
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--append", help="with --config: write to the end of this file (libraries print on stdout too)")
    ap.add_argument("--out", help="all configurations, each in a child process under its own time limit; the first failure stops")
    a = ap.parse_args()
    if a.config:
        with (open(a.append, "a") if a.append else sys.stdout) as f:
            run_config(a.config, f)
        return
    if not a.out:
        ap.error("--config NAME or --out FILE")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name in CONFIGS:
        r = subprocess.run(["timeout", "-k", "10", str(CONFIG_SECONDS), sys.executable, os.path.abspath(__file__), "--config", name,
                            "--append", a.out], stdout=subprocess.DEVNULL)
        if r.returncode != 0:
            sys.exit(f"step_calls: configuration {name} ended with status {r.returncode}: stopping")
        print(f"{name}: done", flush=True)


if __name__ == "__main__":
    main()
