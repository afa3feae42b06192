"""What the whole-network entries (mi3d_unet_*) do with the memory their caller owns.  engine.Plan.own_workspace and engine.LossGroup
take the arena, the metrics, the loss coefficients and the two loss workspaces from torch.empty, and nothing ever zeroes them: a
fresh device block is zero and a recycled one usually holds the last step's right answer, so neither shows a slot that is read
before it is written.  Here the entries run through engine.Plan on buffers of tests/guarded.py, with the helpers of
tests/test_gpu_caller_memory.py (Op, poisoned, reused, refused):

  poison independence   every sequence three times, the arena and the loss workspaces filled with 0x00, 0xA5 and 0xFF (NaN in
                        float32 and bfloat16, -1 in the ticket counters) and every output prefilled with another value each time:
                        all outputs agree bit for bit, and run 0 equals the float64 reference (tests/network_ref.py) under the rule
                        of the whole-network test that already exists for that path;
  guard bands           the arena is exactly mi3d_unet_workspace_bytes at 256 bytes and no stricter, every output exactly its
                        extent, BatchNorm buffers in/out inside bands, and every band is intact after every sequence;
  stale reuse           the call sequences the trainer produces, in ONE arena that is never refilled, each against its run alone;
  refusals              workspace_bytes - 1, an arena 128 bytes off its alignment and a NULL arena, for every entry: a negative
                        status, a message, and no byte of the arena, the loss workspaces or any output changed.

The rules for "equals the reference" are imported, not invented: test_gpu_round2.test_odd_sizes_default_net_vs_oracle (logits
norm-relative, loss relative, fp32 gradients norm-relative; it has no bf16 gradient rule, and neither has this file: bf16
gradients are held to bit equality across the fills and to being finite), test_gpu_parity.test_small_unet_golden_fp32 for the
small net, test_gpu_masked_step's model on the kept logits for the fused head + loss (loss within the model's allowance, metrics
bit for bit), test_gpu_segment's argmax of the entry's own logits for the labels, and the allowances and band rules of
tests/votes_ref.py and tests/sliding_ref.py for the votes.  The loss workspaces take no size argument, so there is no
one-byte-short call for them."""
import copy
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
import loss_ref as L  # noqa: E402
import masked_loss_ref as ML  # noqa: E402
import network_ref as NR  # noqa: E402
import sliding_ref as SR  # noqa: E402
import votes_ref as VR  # noqa: E402
from test_gpu_caller_memory import Op, poisoned, refused, reused, run, workspace  # noqa: E402
from test_gpu_parity import SMALL_BN_TOL, SMALL_GRAD_TOL, SMALL_GRAD_ZERO, SMALL_GRAD_ZERO_TOL, SMALL_LOGITS_TOL, SMALL_LOSS_RTOL  # noqa: E402
from test_gpu_round2 import FP32_GRAD_TOL, ODD_GRAD_NORM_FLOOR, ODD_LOGITS_TOL, ODD_LOSS_RTOL, relerr  # noqa: E402

from multimodal_segmentation_project_amd import _lib, engine, segment  # noqa: E402
from multimodal_segmentation_project_amd._lib import Mi3dError, call, ptr_table, stream_ptr  # noqa: E402

DEV = "cuda:0"
F32, F64, I64, U8 = torch.float32, torch.float64, torch.int64, torch.uint8
ALL = sorted(NR.CASES)
BF16 = [n for n in ALL if NR.CASES[n]["dtype"] == "bf16"]            # the cases that have the fused head + loss
PAIRS = [n for n in ALL if NR.CASES[n]["shape"][0] == 2]             # two window samples in one call
LOSS_ALIGN = 256          # include/mi3d.h documents no alignment for the loss workspaces; the wrappers hand over torch's blocks
CFG = L.make_cfg("combined")


class At:
    """A device address where engine.Plan takes a tensor; shape: for the one argument whose extents the call layer reads."""

    def __init__(self, address, shape=None):
        self.address, self.shape = int(address), shape

    def data_ptr(self):
        return self.address


def at(address):
    return At(address) if address else None


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def status(fn, *args, **kw):
    """The library's status of a call through the host layer, which raises on a negative one."""
    try:
        fn(*args, **kw)
    except Mi3dError as e:
        return int(re.search(r"\(code (-?\d+)\)", str(e)).group(1))
    return 0


def first_failure(*steps):
    for step in steps:
        rc = step()
        if rc != 0:
            return rc
    return 0


def ccfg():
    c = _lib.LossCfg()
    c.w_ce, c.region_kind, c.w_reg, c.alpha, c.beta, c.eps, c.w_kd, c.temperature = (
        CFG["w_ce"], CFG["region_kind"], CFG["w_reg"], CFG["alpha"], CFG["beta"], CFG["eps"], CFG["w_kd"], CFG["temperature"])
    return c


@functools.lru_cache(maxsize=None)
def aux_streams():
    """One aux stream of the lowest priority class and four events, for the life of the process (as the trainer keeps them)."""
    h = C.c_void_p()
    call("mi3d_stream_create", 1, C.byref(h))
    return h, ptr_table([_lib.new_event() for _ in range(4)])


class Net:
    """One case on the device: the model with the reference's seeded init, its Plan (no workspace of its own), the inputs."""

    def __init__(self, name):
        case, spec = NR.CASES[name], NR.net_of(name)
        self.name, self.fp32, self.small = name, case["dtype"] == "fp32", case["net"] == "small"
        self.model = NR.new_model(name).to(DEV)
        self.plan = engine.Plan(self.model, NR.input_shape(name), NR.TORCH_DT[case["dtype"]])
        assert self.plan.ws_bytes == case["ws_bytes"], (name, self.plan.ws_bytes)
        self.params = list(self.model.named_parameters())
        self.buffers = list(self.model.named_buffers())
        sd = NR.state_dict(name)
        self.train_buffers = {k: sd[k].numpy() for k, _ in self.buffers}
        self.eval_buffers = NR.eval_buffers(name)
        i = NR.inputs(name)
        self.x, self.y, self.ym, self.dgap = dev(i["x"]), dev(i["y"]), dev(i["y_masked"]), dev(i["dgap"])
        self.n, self.dims, self.classes = case["shape"][0], tuple(case["shape"][1:]), spec["out_channels"]
        self.v = int(np.prod(self.dims))
        self.levels = len(spec["features"])
        self.segments = 2 * self.levels + 2
        self.n_encoder = 8 * (self.levels + 1)          # parameters of the encoder and the bottleneck: what the DANN target pass reaches
        self.cfg = ccfg()
        self.fused = bool(_lib.lib().mi3d_unet_head_loss_supported(self.plan.d, C.byref(self.cfg)))
        self.loss_side = {"loss_ws": (_lib.lib().mi3d_seg_loss_workspace_bytes(self.classes), LOSS_ALIGN),
                          "met_ws": (_lib.lib().mi3d_seg_metrics_workspace_bytes(self.classes), LOSS_ALIGN)}

    # ---- what the outputs look like
    def logits_spec(self):
        return dict(shape=(self.n, self.classes) + self.dims, dtype=F32)

    def gap_spec(self):
        return dict(shape=(self.n, 2 * NR.net_of(self.name)["features"][-1]), dtype=F32)

    def grad_specs(self, count=None):
        return {"g/" + k: dict(shape=tuple(p.shape), dtype=F32) for k, p in self.params[:count]}

    def buffer_specs(self):
        return {"b/" + k: dict(shape=tuple(b.shape), dtype=I64 if b.dtype == torch.int64 else F32) for k, b in self.buffers}

    def buffer_init(self, which):
        return {"b/" + k: v for k, v in (self.train_buffers if which == "train" else self.eval_buffers).items()}

    def loss_specs(self):
        return {"metrics": dict(shape=(4,), dtype=F32), "coef": dict(shape=(_lib.LOSS_COEF_FLOATS,), dtype=F32)}

    # ---- the call layer on the caller's memory
    def bind(self, ws, nbytes, o):
        """The Plan on this arena, its buffer and gradient tables pointing at the guarded outputs of `o` that exist."""
        p = copy.copy(self.plan)
        p.ws_ptr, p.ws_bytes = ws, nbytes
        p.set_tables(buffers=[at(o.get("b/" + k)) for k, _ in self.buffers], grads=[o.get("g/" + k) for k, _ in self.params])
        return p

    def loss(self, o, masked=False):
        """A LossGroup whose metrics, coefficients and workspaces are the guarded ones."""
        lg = engine.LossGroup(self.cfg, self.classes, DEV, ignore_index=NR.IGNORE if masked else None)
        lg.metrics, lg.coef, lg.loss_ws, lg.met_ws = At(o["metrics"]), At(o["coef"]), At(o["loss_ws"]), At(o["met_ws"])
        lg.fwd = (*lg.cfg_args, o["metrics"], o["coef"], o["metrics"] + 4, o["loss_ws"], o["met_ws"])
        return lg


@functools.lru_cache(maxsize=None)
def net(name):
    return Net(name)


# ---- the references' rules ------------------------------------------------------------------------------------------------------
def finite(got):
    for k, a in got.items():
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), k


def logits_equal(nt, got, ref):
    if nt.small:
        np.testing.assert_allclose(got, ref, **SMALL_LOGITS_TOL)
    else:
        assert relerr(got, ref) < ODD_LOGITS_TOL[nt.fp32], (nt.name, relerr(got, ref))


def loss_equal(nt, got, ref):
    np.testing.assert_allclose(float(got), ref, rtol=SMALL_LOSS_RTOL if nt.small else ODD_LOSS_RTOL[nt.fp32])


def grads_equal(nt, got, ref, base=None):
    """fp32 only (the rule the existing tests have); got: name -> array of the "g/" outputs, base: what they started from."""
    if not nt.fp32:
        return
    for k, want in ref.items():
        if want is None or "g/" + k not in got:
            continue
        mine = got["g/" + k].astype(np.float64) - (0.0 if base is None else base["g/" + k].astype(np.float64))
        if nt.small:
            if np.abs(want).max() < SMALL_GRAD_ZERO:
                assert np.abs(mine).max() < SMALL_GRAD_ZERO_TOL, k
            else:
                assert relerr(mine, want) < SMALL_GRAD_TOL, (k, relerr(mine, want))
        elif float(np.linalg.norm(want)) > ODD_GRAD_NORM_FLOOR:
            assert relerr(mine, want) < FP32_GRAD_TOL, (nt.name, k, relerr(mine, want))


def buffers_equal(nt, got):
    """The BatchNorm buffers after a training forward: the golden's for the small net (the only rule there is)."""
    if nt.small:
        for k, want in NR.reference(nt.name, "train")["buffers"].items():
            np.testing.assert_allclose(got["b/" + k], want, err_msg=k, **SMALL_BN_TOL)
    for k, _ in nt.buffers:
        if k.endswith("num_batches_tracked"):
            assert int(got["b/" + k]) == int(nt.train_buffers[k]) + 1, k


def head_loss_equal(nt, got, labels, ignore):
    """test_gpu_masked_step.check_against_model for any N and D: the loss within the model's allowance on the kept logits, the
    three metrics bit for bit."""
    z = got["logits"].reshape(nt.n, nt.classes, -1)
    lab = labels.cpu().numpy().reshape(nt.n, -1).astype(np.int64)
    ref = ML.masked_loss_ref(z, lab, CFG, ignore)
    sums = ML.masked_sum_allowances(z, lab, CFG, ignore, adds=L.fwd_adds_per_thread(nt.n, z.shape[2], 1, threads=1024))
    dl, _ = ML.masked_coef_allowances(ref, sums, nt.n, nt.classes, z.shape[2], CFG)
    assert abs(float(got["metrics"][0]) - ref["loss"]) <= dl, (nt.name, float(got["metrics"][0]), ref["loss"], dl)
    want = ML.masked_metrics_ref(z, lab, ignore, nt.dims[0])
    G.same_bits([got["metrics"][1:4], want], nt.name + " metrics against the model on the kept logits")


def counts_of(pred, target, c):
    rows = []
    for p, t in zip(pred, target):
        rows.append([int(((p == k) & (t == k)).sum()) for k in range(c)] + [int((p == k).sum()) for k in range(c)]
                    + [int((t == k).sum()) for k in range(c)] + [int((p == t).sum())])
    return np.array(rows, dtype=np.int64)


# ---- training sequences ---------------------------------------------------------------------------------------------------------
def step_op(name, aux=False, per_segment=False, accumulate=False):
    """forward(training = 1) -> loss and metrics of the logits -> their gradient -> backward: the unfused step."""
    nt = net(name)
    outs = dict(logits=nt.logits_spec(), gap=nt.gap_spec(), dlogits=nt.logits_spec(), **nt.loss_specs(), **nt.grad_specs(), **nt.buffer_specs())
    init = nt.buffer_init("train")
    if accumulate:          # gradients that start from a seeded content: only the arena is poisoned
        rng = np.random.default_rng(7)
        init.update({"g/" + k: (1e-3 * rng.standard_normal(tuple(p.shape))).astype(np.float32) for k, p in nt.params})

    def call_(ws, nbytes, o):
        p, lg, s = nt.bind(ws, nbytes, o), nt.loss(o), stream_ptr()
        stream, events = aux_streams() if aux else (None, None)
        cuts = [(k, k + 1) for k in range(nt.segments)] if per_segment else [(0, nt.segments)]
        return first_failure(
            lambda: status(p.forward, nt.x, training=engine.TRAIN, logits=At(o["logits"]), gap=At(o["gap"]), stream=s),
            lambda: status(call, "mi3d_seg_loss_metrics_forward", o["logits"], nt.y.data_ptr(), None, nt.n, nt.classes, nt.dims[0], nt.v, *lg.fwd, s),
            lambda: status(call, "mi3d_seg_loss_backward", o["logits"], nt.y.data_ptr(), None, nt.n, nt.classes, nt.v, *lg.cfg_args, o["coef"],
                           None, o["dlogits"], s),
            *[lambda a=a, b=b: status(p.backward, nt.x, dlogits=At(o["dlogits"]), accumulate=int(accumulate), start=a, end=b, stream=s,
                                      aux=stream, events=events, join=1) for a, b in cuts])

    def check(got):
        ref = NR.reference(name, "train")
        finite(got)
        logits_equal(nt, got["logits"], ref["logits"])
        loss_equal(nt, got["metrics"][0], ref["loss"])
        grads_equal(nt, got, ref["grads"], base=init if accumulate else None)
        buffers_equal(nt, got)

    tag = "".join(t for t, on in ((" aux", aux), (" per segment", per_segment), (" accumulate", accumulate)) if on)
    return Op(f"{name} step{tag}", nt.plan.ws_bytes, 256, outs, call_, check, init=init, side=nt.loss_side)


def fused_op(name, masked=False, head_alone=False, switches=None, routes=None):
    """forward_loss -> backward_loss (head_alone: forward without logits -> head_loss_forward -> backward_loss); masked: the
    `_masked` entries on labels of which about a quarter carry the ignore value.  switches: route switches set through `routes`."""
    nt = net(name)
    assert nt.fused, name
    labels = nt.ym if masked else nt.y
    outs = dict(logits=nt.logits_spec(), gap=nt.gap_spec(), **nt.loss_specs(), **nt.grad_specs(), **nt.buffer_specs())

    def call_(ws, nbytes, o):
        for k, v in (switches or {}).items():
            routes.set(k, v)
        p, lg, s = nt.bind(ws, nbytes, o), nt.loss(o, masked), stream_ptr()
        if head_alone:
            fwd = [lambda: status(p.forward, nt.x, training=engine.TRAIN, logits=None, gap=At(o["gap"]), stream=s),
                   lambda: status(p.head_loss_forward, lg, labels=labels, logits=At(o["logits"]), stream=s)]
        else:
            fwd = [lambda: status(p.forward_loss, nt.x, lg, training=engine.TRAIN, labels=labels, logits=At(o["logits"]), gap=At(o["gap"]), stream=s)]
        return first_failure(*fwd, lambda: status(p.backward_loss, nt.x, lg, labels=labels, grad_scale=None, start=0, end=nt.segments, stream=s))

    def check(got):
        ref = NR.reference(name, "train")
        finite(got)
        logits_equal(nt, got["logits"], ref["logits"])
        if not masked:
            loss_equal(nt, got["metrics"][0], ref["loss"])
        head_loss_equal(nt, got, labels, NR.IGNORE if masked else -1)
        buffers_equal(nt, got)

    tag = (" masked" if masked else "") + (" head alone" if head_alone else "") + (f" {switches}" if switches else "")
    return Op(f"{name} fused step{tag}", nt.plan.ws_bytes, 256, outs, call_, check, init=nt.buffer_init("train"), side=nt.loss_side)


def target_op(name):
    """The DANN target pass: forward without logits, backward with dlogits = NULL, dgap given and the decoder's gradient entries NULL."""
    nt = net(name)
    outs = dict(gap=nt.gap_spec(), **nt.grad_specs(nt.n_encoder), **nt.buffer_specs())

    def call_(ws, nbytes, o):
        p, s = nt.bind(ws, nbytes, o), stream_ptr()
        return first_failure(
            lambda: status(p.forward, nt.x, training=engine.TRAIN, logits=None, gap=At(o["gap"]), stream=s),
            lambda: status(p.backward, nt.x, dlogits=None, dgap=nt.dgap, gap_scale=NR.GAP_SCALE, start=0, end=nt.segments, stream=s))

    def check(got):
        finite(got)
        grads_equal(nt, got, NR.reference(name, "dgap")["grads"])
        buffers_equal(nt, got)

    return Op(f"{name} target pass", nt.plan.ws_bytes, 256, outs, call_, check, init=nt.buffer_init("train"))


def forward_op(name, training):
    """mi3d_unet_forward alone: training 0 (running statistics: the buffers stay as they are), 1, 1 | 4."""
    nt = net(name)
    which = "train" if training else "eval"
    outs = dict(logits=nt.logits_spec(), gap=nt.gap_spec(), **nt.buffer_specs())
    init = nt.buffer_init(which)

    def call_(ws, nbytes, o):
        p = nt.bind(ws, nbytes, o)
        return status(p.forward, nt.x, training=training, logits=At(o["logits"]), gap=At(o["gap"]), stream=stream_ptr())

    def check(got):
        finite(got)
        logits_equal(nt, got["logits"], NR.reference(name, which)["logits"])
        if training:
            buffers_equal(nt, got)
        else:
            for k, want in init.items():
                G.same_bits([got[k], np.asarray(want).reshape(got[k].shape)], k + " after an eval-mode forward")

    return Op(f"{name} forward training={training}", nt.plan.ws_bytes, 256, outs, call_, check, init=init)


def deferred_op(name):
    """forward(training = 2) into double[2C] side buffers -> mi3d_unet_bn_apply_deferred: the buffers of forward(training = 1)."""
    nt = net(name)
    means = [(k, b) for k, b in nt.buffers if k.endswith("running_mean")]
    outs = dict(logits=nt.logits_spec(), gap=nt.gap_spec(), **nt.buffer_specs(), **{"s/" + k: dict(shape=(2 * b.numel(),), dtype=F64) for k, b in means})

    def call_(ws, nbytes, o):
        p, s = nt.bind(ws, nbytes, o), stream_ptr()
        side = copy.copy(p)
        side.set_tables(buffers=[at(o["s/" + k] if k.endswith("running_mean") else o["b/" + k]) for k, _ in nt.buffers])
        return first_failure(
            lambda: status(side.forward, nt.x, training=engine.BN_PUBLISH, logits=At(o["logits"]), gap=At(o["gap"]), stream=s),
            lambda: status(p.bn_apply_deferred, side, stream=s))

    def check(got):
        finite(got)
        plain = forward_op(name, engine.TRAIN)
        want = run(plain, workspace(plain))
        for k in want:
            G.same_bits([want[k], got[k]], f"{name} {k}: deferred update against forward(training = 1)")
        buffers_equal(nt, got)

    return Op(f"{name} forward training=2 + apply", nt.plan.ws_bytes, 256, outs, call_, check, init=nt.buffer_init("train"))


# ---- inference sequences --------------------------------------------------------------------------------------------------------
def labels_op(name):
    """infer -> head_labels with a target: labels, counts, and the logits and GAP of the same infer."""
    nt = net(name)
    outs = dict(logits=nt.logits_spec(), gap=nt.gap_spec(), labels=dict(shape=(nt.n,) + nt.dims, dtype=U8),
                counts=dict(shape=(nt.n, 3 * nt.classes + 1), dtype=I64), **nt.buffer_specs())
    init = nt.buffer_init("eval")
    side = {"head_ws": (_lib.lib().mi3d_head_labels_workspace_bytes(nt.n, nt.classes), 8)}

    def call_(ws, nbytes, o):
        p, s = nt.bind(ws, nbytes, o), stream_ptr()
        return first_failure(
            lambda: status(p.infer, nt.x, logits=At(o["logits"]), gap=At(o["gap"]), stream=s),
            lambda: status(p.head_labels, labels=nt.y, out=At(o["labels"]), counts=At(o["counts"]), head_ws=At(o["head_ws"]), stream=s))

    def check(got):
        finite(got)
        logits_equal(nt, got["logits"], NR.reference(name, "eval")["logits"])
        want = got["logits"].argmax(1).astype(np.uint8)          # test_gpu_segment: the first maximum of the entry's own logits
        assert np.array_equal(got["labels"], want) and (nt.small or len(np.unique(want)) > 1)          # (the golden net predicts one class)
        assert np.array_equal(got["counts"], counts_of(want.reshape(nt.n, -1), nt.y.cpu().numpy().reshape(nt.n, -1), nt.classes))
        for k, v in init.items():
            G.same_bits([got[k], np.asarray(v).reshape(got[k].shape)], k + " after infer")

    return Op(f"{name} infer + head_labels", nt.plan.ws_bytes, 256, outs, call_, check, init=init, side=side)


def votes_op(name, flips=(0, 5)):
    """infer -> head_votes for every flip view, the last one ending in labels, confidence and counts."""
    nt = net(name)
    views = len(flips)
    xs = [nt.x if f == 0 else torch.flip(nt.x, segment._flip_dims(f)).contiguous() for f in flips]
    outs = dict(votes=nt.logits_spec(), labels=dict(shape=(nt.n,) + nt.dims, dtype=U8), confidence=dict(shape=(nt.n,) + nt.dims, dtype=F32),
                counts=dict(shape=(nt.n, 3 * nt.classes + 1), dtype=I64), **{f"logits{i}": nt.logits_spec() for i in range(views)},
                **nt.buffer_specs())
    side = {"head_ws": (_lib.lib().mi3d_head_votes_workspace_bytes(nt.n, nt.classes), 8)}

    def call_(ws, nbytes, o):
        p, s = nt.bind(ws, nbytes, o), stream_ptr()
        steps = []
        for i, (f, x) in enumerate(zip(flips, xs)):
            last = i == views - 1
            steps.append(lambda i=i, x=x: status(p.infer, x, logits=At(o[f"logits{i}"]), stream=s))
            steps.append(lambda i=i, f=f, last=last: status(
                p.head_votes, flip=f, view=i, views=views, flags=_lib.VOTES_KEEP, votes=At(o["votes"]), out=at(last and o["labels"]),
                confidence=at(last and o["confidence"]), labels=nt.y if last else None, counts=at(last and o["counts"]),
                head_ws=at(last and o["head_ws"]), stream=s))
        return first_failure(*steps)

    def check(got):
        finite(got)
        want = VR.votes_from_logits([got[f"logits{i}"].astype(np.float64) for i in range(views)], list(flips))
        assert VR.band_share(want, views) <= VR.BAND_CAP
        assert float(np.abs(got["votes"].astype(np.float64) - want).max()) <= VR.allowance(views)
        assert VR.label_errors(got["labels"], want, views) == 0 and (nt.small or len(np.unique(got["labels"])) > 1)
        top = np.take_along_axis(got["votes"], got["labels"][:, None].astype(np.int64), axis=1)[:, 0]
        G.same_bits([got["confidence"], top / np.float32(views)], "confidence = votes[label] / views in float32")
        assert np.array_equal(got["counts"], counts_of(got["labels"].reshape(nt.n, -1), nt.y.cpu().numpy().reshape(nt.n, -1), nt.classes))

    return Op(f"{name} infer + head_votes {flips}", nt.plan.ws_bytes, 256, outs, call_, check, init=nt.buffer_init("eval"), side=side, keep=xs)


def window_op(name, flips=(0, 3), origins=((0, 0, 0), (2, 4, 8))):
    """infer -> head_votes_window: the N = 2 samples as two windows at different origins of a larger accumulator."""
    nt = net(name)
    assert nt.n == len(flips) == len(origins) == 2
    volume = tuple(max(o[a] for o in origins) + nt.dims[a] for a in range(3))
    tables = SR.importance_tables(nt.dims, "gaussian")
    dtab = [dev(t) for t in tables]
    outs = dict(logits=nt.logits_spec(), acc=dict(shape=(nt.classes,) + volume, dtype=F32), **nt.buffer_specs())
    init = dict(nt.buffer_init("eval"), acc=np.zeros((nt.classes,) + volume, np.float32))          # the accumulator is added to
    fl, og = _lib.int_table(flips), _lib.int_table([k for o in origins for k in o])

    def call_(ws, nbytes, o):
        p, s = nt.bind(ws, nbytes, o), stream_ptr()
        return first_failure(
            lambda: status(p.infer, nt.x, logits=At(o["logits"]), stream=s),
            lambda: status(p.head_votes_window, flips=fl, tables=dtab, origins=og, acc=At(o["acc"], (nt.classes,) + volume), stream=s))

    def check(got):
        finite(got)
        want, s = SR.accumulate64(got["logits"].astype(np.float64), list(zip(origins, flips)), tables, volume)
        assert bool((np.abs(got["acc"].astype(np.float64) - want) <= SR.allowance(s)[None]).all())
        assert float(np.abs(want).max()) > 0

    return Op(f"{name} infer + head_votes_window", nt.plan.ws_bytes, 256, outs, call_, check, init=init, keep=dtab)


# ---- poison independence and guard bands ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_step_does_not_depend_on_what_the_arena_held(name):
    """forward -> backward over all segments in one call; the same on two streams, whose outputs equal the single-stream run bit for
    bit (include/mi3d.h); and one backward call per segment, as _UNetFn.backward makes them."""
    one = poisoned(step_op(name))
    two = poisoned(step_op(name, aux=True))
    for k in one:
        G.same_bits([one[k], two[k]], f"{name} {k}: aux stream against single stream")
    poisoned(step_op(name, per_segment=True))


@pytest.mark.parametrize("name", ALL)
def test_accumulating_backward_and_target_pass_do_not_depend_on_what_the_arena_held(name):
    poisoned(step_op(name, accumulate=True))
    got = poisoned(target_op(name))
    assert any(np.abs(got[k]).max() > 0 for k in got if k.startswith("g/"))


@pytest.mark.parametrize("name", BF16)
def test_fused_head_loss_steps_do_not_depend_on_what_their_memory_held(name):
    """forward_loss -> backward_loss unmasked and masked, and forward without logits -> head_loss_forward -> backward_loss,
    metrics and coefficients among the compared outputs.  The two routes to the head give the same bits."""
    whole = poisoned(fused_op(name))
    poisoned(fused_op(name, masked=True))
    alone = poisoned(fused_op(name, head_alone=True))
    for k in whole:
        G.same_bits([whole[k], alone[k]], f"{name} {k}: head_loss_forward against forward_loss")
    masked_alone = poisoned(fused_op(name, masked=True, head_alone=True))
    assert float(masked_alone["metrics"][0]) != float(alone["metrics"][0])


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("training", [0, 1, 1 | engine.THIN_CONSUMERS, 2])
def test_forward_does_not_depend_on_what_the_arena_held(name, training):
    poisoned(deferred_op(name) if training == 2 else forward_op(name, training))


@pytest.mark.parametrize("name", ALL)
def test_inference_does_not_depend_on_what_the_arena_held(name):
    poisoned(labels_op(name))
    poisoned(votes_op(name))
    if name in PAIRS:
        poisoned(window_op(name))


# ---- stale reuse ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_f32", "deep_bf16"])
def test_an_evaluation_between_two_steps_in_one_arena(name):
    reused(step_op(name), labels_op(name))
    reused(step_op(name), votes_op(name))


def test_other_shape_other_mask_and_other_routes_in_the_same_bytes(routes):
    """step(deep_bf16), step(flat_bf16), step(deep_bf16): another N, geometry and other ticket layers; a masked step, an unmasked
    one, a masked one; and a step under splitk_ticket = 0 before and after one under the default."""
    reused(fused_op("deep_bf16"), fused_op("flat_bf16"))
    reused(fused_op("flat_bf16", masked=True), fused_op("flat_bf16"))
    reused(fused_op("deep_bf16", switches={"splitk_ticket": 0}, routes=routes), fused_op("deep_bf16", switches={"splitk_ticket": 1}, routes=routes))


@pytest.mark.parametrize("name", ["deep_bf16", "ragged_bf16"])
def test_an_eval_forward_before_a_ticket_forward(name):
    """forward(training = 0) leaves its split-K scratch and never touches the ticket counters; the training forward after it
    clears them in its pack launch."""
    reused(forward_op(name, 0), step_op(name))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def entry_ops(name):
    """Every whole-network entry as a single call (a refused call needs no state from an earlier one)."""
    nt = net(name)
    grads, bufs, loss = nt.grad_specs(), nt.buffer_specs(), nt.loss_specs()
    logits, gap = nt.logits_spec(), nt.gap_spec()
    labels8, counts = dict(shape=(nt.n,) + nt.dims, dtype=U8), dict(shape=(nt.n, 3 * nt.classes + 1), dtype=I64)
    head = {"head_ws": (_lib.lib().mi3d_head_votes_workspace_bytes(nt.n, nt.classes), 8)}
    tables = [dev(t) for t in SR.importance_tables(nt.dims, "gaussian")]
    fl, og = _lib.int_table([0] * nt.n), _lib.int_table([0] * (3 * nt.n))

    def op(entry, outs, body, side=None, which="train"):
        def call_(ws, nbytes, o):
            return status(body, nt.bind(ws, nbytes, o), o, stream_ptr())
        return Op(f"{name} {entry}", nt.plan.ws_bytes, 256, outs, call_, None, init=nt.buffer_init(which) if any(k.startswith("b/") for k in outs) else None,
                  side=side, keep=tables)

    ops = [op(f"mi3d_unet_forward training={t}", dict(logits=logits, gap=gap, **bufs),
              lambda p, o, s, t=t: p.forward(nt.x, training=t, logits=At(o["logits"]), gap=At(o["gap"]), stream=s)) for t in (0, 1, 2, 5)]
    ops.append(op("mi3d_unet_infer", dict(logits=logits, gap=gap, **bufs),
                  lambda p, o, s: p.infer(nt.x, logits=At(o["logits"]), gap=At(o["gap"]), stream=s), which="eval"))
    ops.append(op("mi3d_unet_backward", dict(dlogits=logits, **grads),
                  lambda p, o, s: p.backward(nt.x, dlogits=At(o["dlogits"]), dgap=nt.dgap, start=0, end=nt.segments, stream=s)))
    for masked in (False, True):
        lab = nt.ym if masked else nt.y
        tag = "_masked" if masked else ""
        ops.append(op("mi3d_unet_forward_loss" + tag, dict(logits=logits, gap=gap, **loss, **bufs),
                      lambda p, o, s, m=masked, lab=lab: p.forward_loss(nt.x, nt.loss(o, m), labels=lab, logits=At(o["logits"]), gap=At(o["gap"]), stream=s),
                      side=nt.loss_side))
        ops.append(op("mi3d_unet_head_loss_forward" + tag, dict(logits=logits, **loss),
                      lambda p, o, s, m=masked, lab=lab: p.head_loss_forward(nt.loss(o, m), labels=lab, logits=At(o["logits"]), stream=s),
                      side=nt.loss_side))
        ops.append(op("mi3d_unet_backward_loss" + tag, dict(**loss, **grads),
                      lambda p, o, s, m=masked, lab=lab: p.backward_loss(nt.x, nt.loss(o, m), labels=lab, grad_scale=None, start=0, end=nt.segments, stream=s),
                      side=nt.loss_side))
    ops.append(op("mi3d_unet_head_labels", dict(labels=labels8, counts=counts),
                  lambda p, o, s: p.head_labels(labels=nt.y, out=At(o["labels"]), counts=At(o["counts"]), head_ws=At(o["head_ws"]), stream=s), side=head))
    ops.append(op("mi3d_unet_head_votes", dict(votes=logits, labels=labels8, confidence=dict(shape=(nt.n,) + nt.dims, dtype=F32), counts=counts),
                  lambda p, o, s: p.head_votes(flip=0, view=0, views=1, flags=_lib.VOTES_KEEP, votes=At(o["votes"]), out=At(o["labels"]),
                                               confidence=At(o["confidence"]), labels=nt.y, counts=At(o["counts"]), head_ws=At(o["head_ws"]), stream=s),
                  side=head))
    ops.append(op("mi3d_unet_head_votes_window", dict(acc=dict(shape=(nt.classes,) + nt.dims, dtype=F32)),
                  lambda p, o, s: p.head_votes_window(flips=fl, tables=tables, origins=og, acc=At(o["acc"], (nt.classes,) + nt.dims), stream=s)))
    return ops


@pytest.mark.parametrize("name", ["flat_bf16", "small_f32"])
def test_every_entry_refuses_an_arena_it_cannot_use(name):
    """One byte short, 128 bytes off the alignment, and NULL: a negative status and a message before anything is written."""
    ops = entry_ops(name)
    assert len(ops) == 12 + 3          # the twelve entries, mi3d_unet_forward once per training value
    for op in ops:
        refused(op)
        refused(op, misalign=128)
        refused(op, null=True, needle=b"null pointer")
