"""TrainStep / DannStep — the reference's per-step hot loops as native, hipGraph-capturable kernel sequences with
data-parallel gradient all-reduce over RCCL.

    TrainStep   train_unet.py:220-252 (== finetune_ct.py:159-191), distill_unet.py:107-133
        zero_grad -> model(images) -> loss_fn -> backward(loss/accum) -> [all-reduce grads / world] -> AdamW.step
        -> calculate_{iou,dice,accuracy} -> gather(loss, iou, dice, acc).mean()
    DannStep    train_dann.py:233-300
        source fwd -> target fwd (full net) -> GAP x2 -> grad_reverse x2 -> discriminator -> CE
        -> total = task + lambda*domain (lambda applied twice, Q3) -> ONE backward over both graphs -> two AdamW steps

Design (MI355X-first, not a DDP translation):
  * parameters, gradients and AdamW moments live in flat fp32 arenas (22.6 MB each); nn.Parameters are views, so
    state_dict()/load_state_dict() keep working, while the optimizer is ONE kernel and gradient all-reduce operates
    on contiguous arena ranges (no bucket copy-in/copy-out).
  * backward runs as runs of segments with TWO exchanges by default (dp.bucket_ranges): after encoder.L-1's segment the
    arena range [encoder.L-1 .. final_conv] (97 % of the gradient bytes) is all-reduced on a side stream (RCCL over xGMI)
    while the bandwidth-heavy encoder.L-2..0 backward runs; [encoder.0..L-2] follows at the end (dp.bucket_ranges(fine=True):
    four readiness-ordered buckets, measured slower).  The four scalar gathers of the reference (C4) are one 4-float all-reduce
    that rides on the first exchange.
  * a step is captured into hipGraphs: ONE graph at world 1; at world > 1 the step is launched eagerly (or, on request, as
    one graph per comm-free run of kernels with the all-reduces between them: RCCL calls stay outside the graphs).
  * BatchNorm statistics are per-GPU local (DDP + BatchNorm3d semantics); the per-forward buffer broadcast of DDP
     is replaced by `sync_buffers()` before eval/checkpoint.
  * no host synchronisation inside step(); results are device tensors.
"""
import ctypes as C
import math
import os

import torch
import torch.distributed as dist

from . import _lib, engine, surface
from ._lib import Mi3dError, call, ptr, ptr_table, stream_ptr
from .engine import BN_PUBLISH, THIN_CONSUMERS, TRAIN
from . import metrics as M
from .dp import DataParallelComm, ParamArena

_LOSS_TABLE = {      # name -> (w_ce, region_kind, w_reg, alpha, beta, eps); train_unet.py:178-205
    "combined": (1.0, 1, 1.0, 0.0, 0.0, 1e-5), "dice": (0.0, 1, 1.0, 0.0, 0.0, 1e-5),
    "tversky": (0.0, 2, 1.0, 0.5, 0.5, 1e-6), "ce_tversky": (0.3, 2, 0.7, 0.5, 0.5, 1e-6),
    "ce": (1.0, 0, 0.0, 0.0, 0.0, 1e-6),
}


def _loss_cfg(kind, kd_alpha=None, temperature=2.0):
    if kd_alpha is not None:      # distillation_loss, utils/metrics.py:169-190
        return M._cfg(0.3 * kd_alpha, 2, 0.7 * kd_alpha, 0.7, 0.3, 1e-6, 1.0 - kd_alpha, temperature)
    if kind not in _LOSS_TABLE:
        raise Mi3dError(f"unknown loss {kind!r}: one of {sorted(_LOSS_TABLE)} (train_unet.py:538 --loss choices)")
    return M._cfg(*_LOSS_TABLE[kind])


def _finite_weight(value, name="boundary_weight"):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise Mi3dError(f"{name} {value!r} is not a number") from None
    if not math.isfinite(value):
        raise Mi3dError(f"{name} {value} is not finite")
    return value


def _priority_stream(device, cls):
    """torch stream object around a hipStream_t of priority class cls (-1 highest, 0 middle, +1 lowest; mi3d_stream_create).
    The handle lives as long as the process: streams are few and are shared through the per-device cache below."""
    h = C.c_void_p()
    call("mi3d_stream_create", int(cls), C.byref(h))
    st = torch.cuda.ExternalStream(h.value, device=device)
    st.mi3d_handle = h
    return st


_STREAM_CACHE = {}      # (device index, role) -> stream chosen by concurrent_stream
_CAPTURE_STREAMS = {}   # device index -> the stream hipGraph captures run on (nothing else ever does)


def _capture_stream(device):
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _CAPTURE_STREAMS:
        _CAPTURE_STREAMS[key] = _priority_stream(dev, 0)
    return _CAPTURE_STREAMS[key]


def concurrent_stream(device, candidates=6, hold_us=300, role="aux"):
    """A stream whose kernels really run BESIDE those of the current (compute) stream.  HIP multiplexes streams onto a few
    hardware queues, and two streams that share a queue execute strictly one after the other (measured with rocprofv3: the
    default stream and the 8th stream created in a process both sat on queue 4, and a collective kernel on the latter ran
    between, not beside, the backward kernels -- profiles/r03_dp_streams.txt).  So the stream is CHOSEN by a measurement: a
    stand-in kernel that holds a few workgroups for `hold_us` is launched on the candidate and on the compute stream; if the
    pair takes about one hold time they overlap (minimum of three timed repetitions: a busy GPU only ever makes a pair look
    slower).  The first candidate is a high-priority stream (its own queue on this runtime).  The choice is cached per
    (device, role): every step object of a process shares it and the probe runs once.  When no candidate overlaps, the last
    one is returned with mi3d_concurrent = False and a RuntimeWarning: the step is still correct, only nothing will run
    beside the compute stream."""
    import warnings
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), role)
    if key in _STREAM_CACHE:
        return _STREAM_CACHE[key]
    main = torch.cuda.current_stream(device)
    buf = torch.zeros(1024, dtype=torch.float32, device=device)
    best = None
    for i in range(candidates):
        c = torch.cuda.Stream(device=device, priority=-1 if i == 0 else 0)
        times = []
        for rep in range(4):                       # first pass loads the code object
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            e0.record(main)
            c.wait_stream(main)
            call("mi3d_debug_occupy_cus", 4, hold_us, buf.data_ptr(), buf.numel(), c.cuda_stream)
            call("mi3d_debug_occupy_cus", 4, hold_us, buf.data_ptr(), buf.numel(), main.cuda_stream)
            main.wait_stream(c)
            e1.record(main)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        c.mi3d_overlap_us = min(times[1:])
        c.mi3d_concurrent = c.mi3d_overlap_us < 1.5 * hold_us
        best = c
        if c.mi3d_concurrent:
            break
    if not best.mi3d_concurrent:
        warnings.warn(f"concurrent_stream: none of {candidates} candidate streams ran beside the compute stream on {dev} "
                      f"(pair time {best.mi3d_overlap_us:.0f} us for 2 x {hold_us} us): aux-stream work will serialise",
                      RuntimeWarning, stacklevel=2)
    _STREAM_CACHE[key] = best
    return best


class ArenaAdamW(torch.optim.Optimizer):
    """`param_groups` surface of the arena optimizer, so that torch.optim.lr_scheduler objects (the reference's
    ReduceLROnPlateau(mode='max', patience=10, factor=0.1, min_lr=1e-6), train_unet.py:381,442) can drive the learning
    rate: `scheduler = ReduceLROnPlateau(step.optimizer, ...); scheduler.step(val_dice)`.  The update itself is the
    fused kernel inside TrainStep.step(); calling .step() here is an error."""

    def __init__(self, params, lr, betas, eps, weight_decay):
        super().__init__(list(params), dict(lr=float(lr), betas=tuple(betas), eps=float(eps),
                                            weight_decay=float(weight_decay)))

    def step(self, closure=None):
        raise Mi3dError("ArenaAdamW.step(): the AdamW update runs inside TrainStep.step() / DannStep.step()")


class _Graphs:
    """hipGraph executables of one static state: variant -> [(graph_exec, comm_fn_or_None), ...]"""

    def __init__(self):
        self.by_variant = {}
        self.hyper = None

    def drop(self):
        for segs in self.by_variant.values():
            for g, _ in segs:
                if g is not None and g.value:
                    _lib.lib().mi3d_graph_destroy(g)
        self.by_variant = {}


class _State:
    """Static buffers of one (input shape, compute dtype, trainable set, mode).  Attributes; st["name"] reads them as well
    (tests and tools do) and raises KeyError for a name this state does not have."""

    def __getitem__(self, name):
        try:
            return getattr(self, name)
        except AttributeError:
            raise KeyError(name) from None


def _segment_runs(nseg, due):
    """The backward as runs of segments: (start, end, buckets, is_last) for every run [start, end) that ends behind a segment with
    gradient buckets due (due: segment -> buckets complete after it) or behind the last one.  One C call per run: kernels of
    adjacent segments share launches (a weight-gradient slab sum rides in the next BatchNorm reduction), which a call
    boundary would cut."""
    start = 0
    for seg in range(nseg):
        buckets = tuple(due.get(seg) or ())
        if buckets or seg == nseg - 1:
            yield start, seg + 1, buckets, seg == nseg - 1
            start = seg + 1


class _StepBase:
    """Arena / communication / graph machinery and the static state shared by TrainStep and DannStep."""
    _n_metrics = 4

    def _init_common(self, model, lr, weight_decay, betas, eps, grad_accum, process_group, compute_dtype, use_graph,
                     force_comm):
        self.model = model
        self.accum = int(grad_accum)
        if self.accum < 1:
            raise Mi3dError("grad_accum must be >= 1")
        self.micro = 0
        self.dtype = compute_dtype
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        p0 = next(model.parameters())
        _lib.require_cuda(p0, type(self).__name__)
        self.device = p0.device
        self.arena = ParamArena(model.parameters(), self.device)
        self.optimizer = ArenaAdamW(model.parameters(), lr, betas, eps, weight_decay)
        n_levels = len(model.encoder)
        # MI3D_FORCE_COMM=1 / force_comm: drive the bucket path (side stream, all-reduce, joins, segmented graphs) even
        # at world 1 -- a 1-rank RCCL group on the 1-GPU box exercises the real code path
        self.force_comm = bool(force_comm) or os.environ.get("MI3D_FORCE_COMM", "0") == "1"
        self.do_comm = self.world > 1 or (self.force_comm and dist.is_available() and dist.is_initialized())
        self.comm = DataParallelComm(self.arena, n_levels, process_group, force=self.do_comm)
        # the exchange stream must sit on another hardware queue than the compute stream (see concurrent_stream)
        self.comm_stream = concurrent_stream(self.device, role="comm") if self.do_comm else None
        # MI3D_NO_MARKS=1: exchange points cut the backward into calls instead of marks; MI3D_COMM_SERIAL=1: every bucket behind
        # the last segment, on the compute stream (TrainStep)
        self.no_marks = bool(os.environ.get("MI3D_NO_MARKS"))
        self.comm_serial = bool(os.environ.get("MI3D_COMM_SERIAL"))
        self._mark_handles = []          # exchange-mark events (mi3d_unet_backward_marks)
        self.use_graph = bool(use_graph)
        self.keep_logits = False
        self._statics = {}
        self._static = None
        self.inv_accum = torch.full((), 1.0 / self.accum, dtype=torch.float32, device=self.device)
        self._closed = False

    # ---- static state for one (shape, dtype, trainable set, mode)
    def _prepare(self, x, mode="train"):
        dt = self.dtype or engine.resolve_compute_dtype(self.model)
        # frozen parameters (requires_grad=False: encoder/bottleneck freezing of train_unet.py:31-43, finetune_ct.py:270-304)
        # are part of the static state: they get no gradient, no optimizer update, and trailing all-frozen backward
        # segments are not run at all
        trainable = tuple(bool(p.requires_grad) for p in self.arena.params)
        key = (tuple(x.shape), dt, trainable, mode)
        st = self._statics.get(key)
        if st is None:
            st = self._new_state(key, self.cfg if mode == "train" else self.eval_cfg)
            self._extend(st)
            self._statics[key] = st
        if mode == "train":
            self._static = st
        return st

    def _new_state(self, key, cfg):
        """What every step needs: the Plan with its workspace, input / label / logits buffers, the loss group and, for training,
        the Dropout scale buffer and whether the head folds into the loss."""
        shape, dt, trainable, mode = key
        dev = self.device
        st = _State()
        st.mode, st.trainable, st.graphs = mode, trainable, _Graphs()
        st.plan = engine.Plan(self.model, shape, dt, params=self.arena.params,
                              grads=[g if t else None for g, t in zip(self.arena.grad_ptrs(), trainable)]).own_workspace(dev)
        desc = st.desc = st.plan.desc
        st.L = desc.n_levels
        st.x = torch.empty(shape, dtype=torch.float32, device=dev)
        st.y = torch.empty((desc.N, desc.D * desc.H * desc.W), dtype=torch.int64, device=dev)
        st.loss = engine.LossGroup(cfg, desc.out_channels, dev, self._n_metrics, ignore_index=getattr(self, "ignore_index", None))
        st.metrics = st.loss.metrics
        st.logits_shape = (desc.N, desc.out_channels, desc.D, desc.H, desc.W)
        keep = True
        if mode == "train":
            st.fused_head = (not _lib.get_route("no_head_loss") and
                             _lib.lib().mi3d_unet_head_loss_supported(st.plan.d, st.loss.cfg_ref) == 1)
            st.drop = torch.empty(_lib.lib().mi3d_unet_dropout_count(st.plan.d), dtype=torch.float32, device=dev)
            # the fused head never writes logits / dlogits: there is no buffer to read stale values from (ts._static["logits"]
            # is None; keep_logits=True keeps a copy)
            keep = not st.fused_head or self.keep_logits
            st.dlogits = torch.empty(st.logits_shape, dtype=torch.float32, device=dev) if keep else None
        st.logits = torch.empty(st.logits_shape, dtype=torch.float32, device=dev) if keep else None
        return st

    def _extend(self, st):
        pass

    # ---- the step surface: each class declares step() / load_batch() with its own arguments over these two
    def _load(self, st, non_blocking, **tensors):
        """Copy a batch into the static buffers named by the keywords, in their order."""
        for name, t in tensors.items():
            st[name].copy_(t.reshape(st[name].shape), non_blocking=non_blocking)

    def step_static(self, last_batch=False):
        """Run on the data already resident in the static buffers (bench path: inputs in HBM when timing starts)."""
        st = self._static
        if st is None:
            raise Mi3dError("step_static() before any step()/load_batch()")
        self._run(st, last_batch=last_batch)      # a partial window on the last batch: the (first, True) variant (captured like the others)
        return st.metrics

    # ---- optimizer surface
    @property
    def lr(self):
        return self.optimizer.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        """Learning rate (also reachable through `self.optimizer.param_groups`, i.e. torch LR schedulers).  The value
        is a kernel argument: captured step graphs are re-captured on the next step when it changed."""
        for g in self.optimizer.param_groups:
            g["lr"] = float(value)

    def _hyper(self):
        g = self.optimizer.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))

    def _drop_graphs(self):
        for st in self._statics.values():
            st.graphs.drop()

    def close(self):
        """Destroy captured graph executables and events (also run by __del__)."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        try:
            self._drop_graphs()
            for e in getattr(self, "_mark_handles", []):
                _lib.lib().mi3d_event_destroy(e)
            self._mark_handles = []
            self._close_extra()
        except Exception:      # noqa: BLE001  (interpreter shutdown: the library may already be gone)
            pass

    def _close_extra(self):
        pass

    def __del__(self):
        self.close()

    # ---- DDP construction semantics: rank 0's parameters and buffers win
    def broadcast_parameters(self):
        self.comm.broadcast_parameters(self.model.buffers())

    def sync_buffers(self):
        self.comm.sync_buffers(self.model.buffers())

    # ---- exchange points
    def _on_comm_stream(self, fn):
        """Run fn on the communication stream, ordered after everything enqueued so far on the compute stream; the
        compute stream keeps going."""
        cs = self.comm_stream
        cs.wait_stream(torch.cuda.current_stream())
        aux = getattr(self, "aux_stream", None)
        if aux is not None:        # gradients the deferred weight-gradient kernels are still writing (TrainStep aux_wgrad)
            cs.wait_stream(aux)
        with torch.cuda.stream(cs):
            fn()

    def _join_comm(self):
        torch.cuda.current_stream().wait_stream(self.comm_stream)

    def _adamw(self, arena, ranges, hyper, s):
        lr, b1, b2, eps, wd = hyper
        for k, (lo, hi) in enumerate(ranges):
            call("mi3d_adamw_apply", arena.p.data_ptr() + 4 * lo, arena.g.data_ptr() + 4 * lo,
                 arena.m.data_ptr() + 4 * lo, arena.v.data_ptr() + 4 * lo, hi - lo, lr, b1, b2, eps, wd, 1.0,
                 ptr(arena.step), int(k == len(ranges) - 1), s)

    @staticmethod
    def _trainable_ranges(arena, trainable):
        ranges = []
        for i, t in enumerate(trainable):
            if not t:
                continue
            lo, hi = arena.range_of(i, i + 1)
            if ranges and ranges[-1][1] == lo:
                ranges[-1] = (ranges[-1][0], hi)
            else:
                ranges.append((lo, hi))
        return ranges

    # ---- graph capture / replay.  `variant` = (first micro-step of an accumulation window, boundary micro-step)
    def _variant(self):
        return (self.micro % self.accum == 0, (self.micro + 1) % self.accum == 0)

    def _run(self, st, last_batch=False):
        """last_batch: the final batch of an epoch.  The reference's loaders are accelerator.prepare()'d (train_unet.py:384),
        so accelerate's accumulate() forces gradient sync + optimizer.step on the LAST batch of every epoch and restarts its
        step count (GradientState.end_of_dataloader; train_dann.py:287 does the same by hand): the micro-step becomes a
        boundary whatever its position in the window, and the next epoch starts a fresh window."""
        self._check_mode()
        variant = self._variant()
        bump = 1
        if last_batch and not variant[1]:
            variant = (variant[0], True)
            bump = self.accum - (self.micro % self.accum)
        if not self.use_graph:
            self._enqueue(st, variant, lambda fn: fn())
            self.micro += bump
            return
        gr = st.graphs
        hyper = self._hyper()
        if gr.hyper != hyper:
            gr.drop()
            gr.hyper = hyper
        segs = gr.by_variant.get(variant)
        if segs is None:
            segs = gr.by_variant[variant] = self._capture(st, variant)
        for g, fn in segs:
            call("mi3d_graph_launch", g, stream_ptr())
            if fn is not None:
                fn()
        self.micro += bump

    def _mutable_state(self):
        """Tensors a step execution modifies (snapshot/restore around the capture warm-up)."""
        a = self.arena
        return [a.p, a.g, a.m, a.v, a.step] + list(self.model.buffers()) + [engine._rng_state(self.model, self.device)]

    def _capture(self, st, variant):
        """Capture one micro-step into hipGraph(s).  A warm-up execution is needed first (lazy code-object loading
        must not happen inside the capture); it runs on a snapshot of all mutable state, which is restored afterwards,
        so capturing is invisible to the training trajectory.  Communication functions are not captured: they cut the
        graph, and replay launches them between the segments."""
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream())
        segs = []
        with torch.cuda.stream(s):
            state = self._mutable_state()
            snap = [t.clone() for t in state]
            self._enqueue(st, variant, lambda fn: fn())
            if self.do_comm:
                self._join_comm()
                self.comm_stream.synchronize()
            s.synchronize()
            for t, c in zip(state, snap):
                t.copy_(c)
            s.synchronize()
        # The capture itself runs on a PRIVATE stream that never carries a collective.  The warm-up above issued the last bucket's
        # all-reduce on `s` (and torch hands out `s` from a pool other step objects' exchange streams come from): the process
        # group's watchdog thread polls the end events of such work for up to its 100 ms period, and a poll that meets a stream
        # in capture ends the capture with hipErrorCapturedEvent (seen once in ~10 runs of the forced-exchange test).
        cs = _capture_stream(self.device)
        cs.wait_stream(s)
        with torch.cuda.stream(cs):
            def cut(fn):
                g = C.c_void_p()
                call("mi3d_graph_end", cs.cuda_stream, C.byref(g))
                segs.append((g, fn))
                call("mi3d_graph_begin", cs.cuda_stream)

            call("mi3d_graph_begin", cs.cuda_stream)
            try:
                self._enqueue(st, variant, cut)
            finally:
                g = C.c_void_p()
                call("mi3d_graph_end", cs.cuda_stream, C.byref(g))
                segs.append((g, None))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.current_stream().wait_stream(cs)
        return segs


class TrainStep(_StepBase):
    def __init__(self, model, loss="combined", lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8,
                 grad_accum=1, kd_teacher=None, kd_alpha=0.7, kd_temperature=2.0, process_group=None,
                 compute_dtype=None, use_graph=False, aux_wgrad=None, reference_zero_grad_quirk=False,
                 force_comm=False, overlap_teacher=True, keep_logits=False, ignore_index=None, boundary_weight=None,
                 boundary_classes=(1, 2, 3), boundary_spacing=(1, 1, 1), entropy_weight=None, entropy_on="ignored"):
        """aux_wgrad: the backward's critical path is the input-gradient chain alone -- the weight gradients of the decoder's
        full-resolution convs and of all deep-level convs run on a second stream (include/mi3d.h, mi3d_unet_backward: aux_stream),
        forked from the chain at most three times and joined in front of the optimizer; bit-identical results.  None (default):
        on for eager launches without a gradient exchange, off under use_graph -- this runtime's hipGraph executor spreads a forked graph over three hardware
        queues and replays it at half speed (4.4 vs 2.2 ms, profiles/r04_defer_graph_streams.txt), eager launches do not.
        keep_logits: the step folds the 1x1x1 head into the loss and never writes the logits (mi3d_unet_forward_loss); True
        keeps a copy in the static buffer `logits` for callers that read them after step().
        ignore_index: voxels labelled with this value count neither in the loss (CE mean over the voxels that do, region sums,
        gradient) nor in the metrics, in step() and evaluate(), on both head routes, eager and under use_graph; with kd_teacher the
        distillation term stays over every voxel (include/mi3d.h, "Ignore value").  None (default): the step as it always was.
        boundary_weight: a float (0.0 included) adds boundary_weight * the boundary loss of Kervadec et al. (include/mi3d.h,
        mi3d_boundary_loss) over the logit channels boundary_classes to the loss and its gradient to the logits' gradient, one
        pass directly behind the loss backward.  The step then keeps head and loss apart (fused_head is False: the logits have to
        exist).  The signed distance maps are the static buffer `dist`: given to step() / load_batch() as dist=, or computed
        from the labels at boundary_spacing (mm per voxel; surface.signed_distance_maps) right after the load, outside any
        captured graph.  The property boundary_weight may be raised between epochs; like lr it is a kernel argument, so a
        captured graph is captured again.  The returned loss is overlap + boundary_weight * L, undivided by the accumulation
        count like the rest; ignored voxels add nothing to L, the distillation term is untouched.  Out of scope: evaluate()
        keeps reporting the overlap loss alone, DannStep has no such term, and the term is not folded into the fused head +
        loss pass.  None (default): no new buffer, no new launch, the step as it always was.
        entropy_weight: a float (0.0 included) adds entropy_weight * the entropy of the prediction (MinEnt of ADVENT, Vu et al.;
        include/mi3d.h, mi3d_entropy_loss) over the voxels entropy_on selects to the loss and its gradient to the logits' gradient:
        one pass directly behind the loss backward (behind the boundary pass when both are set), in front of any exchange.
        entropy_on: "ignored" (default) = the voxels labelled ignore_index, where the loss is otherwise silent (needs ignore_index);
        "counted" = the others; "all" = every voxel.  Like boundary_weight the keyword keeps head and loss apart, the property
        entropy_weight may be set between steps (a captured graph is captured again), and the returned loss is overlap (+ boundary)
        + entropy_weight * L, undivided by the accumulation count.  evaluate() is untouched.  None (default): no buffer, no launch.
        reference_zero_grad_quirk: train_unet.py:222 / finetune_ct.py:161 call optimizer.zero_grad() INSIDE
        accelerator.accumulate(), where accelerate only really zeroes on the boundary micro-step -> the gradient the
        reference applies is grad(last micro-batch)/accum.  False (default): accumulate all micro-batches
        (what distill_unet.py:114-115 does and what the flag's name promises); True: reproduce the reference's
        train/finetune behaviour bit for bit (non-boundary micro-steps still run forward, BN statistics and metrics)."""
        cfg = _loss_cfg(loss, kd_alpha if kd_teacher is not None else None, kd_temperature)     # validates the name first
        self.ignore_index = M.check_ignore_index(ignore_index)      # read by _new_state when the loss group is made
        self._boundary_weight, self.boundary_classes, self.boundary_spacing = None, None, None
        if boundary_weight is not None:
            self._boundary_weight = _finite_weight(boundary_weight)
            self.boundary_classes = M.check_channels(boundary_classes, 8, "TrainStep")      # against the head's channels in _extend
            self.boundary_spacing = surface._spacing(boundary_spacing, None, "TrainStep")
        self._entropy_weight, self.entropy_on = None, None
        if entropy_weight is not None:
            self._entropy_weight = _finite_weight(entropy_weight, "entropy_weight")
            M.entropy_mode(entropy_on, "TrainStep")
            if entropy_on == "ignored" and self.ignore_index is None:
                raise Mi3dError('TrainStep: entropy_on="ignored" selects the voxels labelled ignore_index, and none was given')
            self.entropy_on = entropy_on
        self._init_common(model, lr, weight_decay, betas, eps, grad_accum, process_group, compute_dtype, use_graph,
                          force_comm)
        self.teacher = kd_teacher
        self.loss_kind = loss
        self.cfg = cfg
        self.keep_logits = bool(keep_logits)
        # evaluate(): train_unet.py:259-305 uses the training loss_fn; distill_unet.py:149 uses combined_loss
        self.eval_cfg = _loss_cfg("combined" if kd_teacher is not None else loss)
        self.quirk = bool(reference_zero_grad_quirk) and kd_teacher is None
        if kd_teacher is not None:
            self._check_teacher(kd_teacher)
        # distillation (distill_unet.py:107-112): the frozen teacher's forward does not depend on the student's -- it runs on
        # its own stream beside the student forward (fork after the batch is in place, join in front of the loss; both
        # branches are captured into the one step graph).  Separate workspaces and logits: results are bitwise those of the
        # serial order.  Both forwards are long chains that leave most CUs idle at the deep levels, so they interleave.
        self.kd_stream = concurrent_stream(self.device, role="kd") if (kd_teacher is not None and overlap_teacher) else None
        # second compute stream: the deferred weight-gradient kernels run beside the data-gradient chain (mi3d_unet_backward)
        # (priority classes measured at 96^3, eager: high 2.111 / normal 2.121 / low 2.124 ms -- profiles/r04_experiments_aux_wgrad.txt)
        if aux_wgrad is None:
            # not with a gradient exchange either: the deferred deep-level weight gradients are 95 % of the gradient bytes and
            # finish ~150 us before the end of the backward, so the big all-reduce bucket (dp.bucket_ranges) would lose the
            # 0.45 ms of encoder backward it hides under; the exchange is worth more than the ~20 us the deferral buys
            aux_wgrad = not use_graph and not self.do_comm
        self.aux_stream = concurrent_stream(self.device) if aux_wgrad else None
        self._event_handles = [_lib.new_event() for _ in range(4)] if aux_wgrad else []
        self._events = ptr_table(self._event_handles) if aux_wgrad else None
        if self.world > 1:
            self.broadcast_parameters()

    def _close_extra(self):
        for e in self._event_handles:
            _lib.lib().mi3d_event_destroy(e)
        self._event_handles = []

    def _check_teacher(self, teacher):
        """distill_unet.py:20-29 loads the teacher with map_location: it must end up on the student's device with
        the student's architecture, else the kernels would dereference foreign addresses."""
        sp, tp = list(self.model.parameters()), list(teacher.parameters())
        sb, tb = list(self.model.buffers()), list(teacher.buffers())
        if len(sp) != len(tp) or len(sb) != len(tb):
            raise Mi3dError(f"kd_teacher has {len(tp)} parameters / {len(tb)} buffers, the student {len(sp)} / {len(sb)}: "
                            "teacher and student must be the same UNet3D architecture (distill_unet.py:214-215)")
        for kind, mine, theirs in (("parameter", sp, tp), ("buffer", sb, tb)):
            for i, (a, b) in enumerate(zip(mine, theirs)):
                if b.device != self.device:
                    raise Mi3dError(f"kd_teacher {kind} {i} is on {b.device}, the student on {self.device}: move the "
                                    "teacher with .to(device) first (no CPU fallback)")
                if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
                    raise Mi3dError(f"kd_teacher {kind} {i}: shape/dtype {tuple(b.shape)}/{b.dtype} != student's "
                                    f"{tuple(a.shape)}/{a.dtype}")
                if not b.is_contiguous():
                    raise Mi3dError(f"kd_teacher {kind} {i} is not contiguous")

    def reset_optimizer(self):
        """What rebuilding ``optim.AdamW`` does in the reference when the encoder is (un)frozen
        (train_unet.py:413-431, finetune_ct.py:374-381): moments and step count start from zero."""
        self.arena.m.zero_()
        self.arena.v.zero_()
        self.arena.step.zero_()
        self._drop_graphs()
        self._statics = {}
        self._static = None

    @property
    def boundary_weight(self):
        return self._boundary_weight

    @boundary_weight.setter
    def boundary_weight(self, value):
        """The weight of the boundary term; only a step built with one has the term (and the buffers) to weigh."""
        if self._boundary_weight is None:
            raise Mi3dError("TrainStep was built without boundary_weight: the step has no boundary term to weigh")
        self._boundary_weight = _finite_weight(value)

    @property
    def entropy_weight(self):
        return self._entropy_weight

    @entropy_weight.setter
    def entropy_weight(self, value):
        """The weight of the entropy term; only a step built with one has the term (and the workspace) to weigh."""
        if self._entropy_weight is None:
            raise Mi3dError("TrainStep was built without entropy_weight: the step has no entropy term to weigh")
        self._entropy_weight = _finite_weight(value, "entropy_weight")

    def _hyper(self):
        return super()._hyper() + (self._boundary_weight, self._entropy_weight)

    def _new_state(self, key, cfg):
        st = super()._new_state(key, cfg)
        extra = self._boundary_weight is not None or self._entropy_weight is not None
        if key[3] == "train" and extra and st.fused_head:
            # a term on the logits reads them and adds into their gradient: head and loss stay apart
            st.fused_head = False
            st.logits = torch.empty(st.logits_shape, dtype=torch.float32, device=self.device)
            st.dlogits = torch.empty(st.logits_shape, dtype=torch.float32, device=self.device)
        return st

    # ---- TrainStep's part of a static state: the segment and exchange schedule, the teacher
    def _extend(self, st):
        if st.mode != "train":
            return
        desc, trainable, dev = st.desc, st.trainable, self.device
        if self._boundary_weight is not None:
            if max(self.boundary_classes) >= desc.out_channels:
                raise Mi3dError(f"TrainStep: boundary_classes {self.boundary_classes} are logit channels below {desc.out_channels}")
            st.dist = torch.zeros((desc.N, len(self.boundary_classes), desc.D, desc.H, desc.W), dtype=torch.float32, device=dev)
            st.bd_ws = M.boundary_workspace(desc.N, desc.D * desc.H * desc.W, dev)
        if self._entropy_weight is not None:
            if not 2 <= desc.out_channels <= 8:
                raise Mi3dError(f"TrainStep: the entropy term takes 2 to 8 logit channels, the head has {desc.out_channels}")
            st.ent_ws = M.entropy_workspace(desc.N, desc.D * desc.H * desc.W, dev)
        st.opt_ranges = self._trainable_ranges(self.arena, trainable)
        last = -1
        r = (C.c_int * 4)()
        for seg in range(2 * st.L + 2):
            _lib.check(_lib.lib().mi3d_unet_segment_params(st.plan.d, seg, r), "mi3d_unet_segment_params")
            idx = list(range(r[0], r[1])) + (list(range(r[2], r[3])) if r[2] >= 0 else [])
            if any(trainable[i] for i in idx):
                last = seg
        st.nseg_run = last + 1
        # exchange schedule: bucket -> the segment after which it is complete AND will still be run; buckets with
        # no trainable parameter are not reduced at all
        sched = {}
        for seg, (lo, hi) in self.comm.buckets.items():
            live = any(t and lo <= o < hi for o, t in zip(self.arena.offsets, trainable))
            if live and last >= 0:
                sched.setdefault(min(seg, last), []).append(seg)
        if self.comm_serial and sched and last >= 0:
            # every bucket behind the last segment, on the compute stream: no second hardware queue in the step at all (any
            # kernel on another queue costs this step 100-250 us on this runtime, profiles/r04_experiments_second_queue.txt),
            # at the price of an all-reduce that hides under nothing
            sched = {last: [b for sg in sorted(sched) for b in sched[sg]]}
        st.comm_after = sched
        if self.teacher is not None:
            st.teacher = st.plan.sibling(dev, params=list(self.teacher.parameters()), buffers=list(self.teacher.buffers()))
            st.t_logits = torch.empty(st.logits_shape, dtype=torch.float32, device=dev)

    def _check_mode(self):
        if not self.model.training:
            raise Mi3dError("TrainStep.step() on a model in eval mode: the backward kernels use batch statistics "
                            "(train_unet.py:208 calls model.train() first); use evaluate() for eval-mode passes")

    # ---- the kernel sequence of one micro-step (everything on the current stream except the all-reduces)
    def _enqueue(self, st, variant, comm):
        first, boundary = variant
        s = stream_ptr()
        # Q2: see reference_zero_grad_quirk in __init__
        if self.quirk:
            accumulate, run_backward = 0, boundary
        else:
            accumulate, run_backward = (0 if first else 1), True
        drop, t_logits = self._forward_loss(st, s)
        self._backward_exchange(st, s, comm, drop, t_logits, accumulate, boundary, run_backward)
        if boundary:
            self._adamw(self.arena, st.opt_ranges, self._hyper()[:5], s)

    def _forward_loss(self, st, s):
        """Dropout scales, the teacher's forward, the student's forward with loss and metrics.  Returns (drop, t_logits)."""
        model, plan, loss = self.model, st.plan, st.loss
        drop = engine.fill_drop_scales(st.drop, float(getattr(model, "dropout_rate", 0.0)),
                                       lambda: engine._rng_state(model, self.device),
                                       getattr(model, "_mi3d_injected_drop_scales", None), s)
        teacher, ks = (st.teacher if self.teacher is not None else None), self.kd_stream
        if teacher is not None and ks is not None:
            ks.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ks):
                teacher.infer(st.x, logits=st.t_logits, stream=ks.cuda_stream)
        fused = st.fused_head
        keep = st.logits if self.keep_logits else None
        if fused and teacher is None:
            # 1x1x1 head + loss + metrics in one pass: the logits are never written (mi3d.h, mi3d_unet_forward_loss)
            plan.forward_loss(st.x, loss, drop=drop, labels=st.y, logits=keep, stream=s)
        else:
            # distillation with a fused head: the student's body now, its head + loss after the join with the teacher's stream
            plan.forward(st.x, drop=drop, logits=None if fused else st.logits, stream=s)
        t_logits = None
        if teacher is not None:
            if ks is not None:
                torch.cuda.current_stream().wait_stream(ks)
            else:
                # frozen teacher (distill_unet.py:109-111): the BatchNorm-folded inference forward
                teacher.infer(st.x, logits=st.t_logits, stream=s)
            t_logits = st.t_logits
            if fused:
                plan.head_loss_forward(loss, labels=st.y, teacher=t_logits, logits=keep, stream=s)
        # loss + metrics (SURVEY Q1 loop bound D) of the same logits in one pass (replaces 3 argmaxes + 2(D-1) host syncs)
        if not fused:
            loss.metrics_forward(st.logits, st.y, teacher=t_logits, stream=s)
        return drop, t_logits

    def _backward_exchange(self, st, s, comm, drop, t_logits, accumulate, boundary, run_backward):
        """The backward in runs of segments, with the gradient exchange (and the metrics' all-reduce) between them."""
        # the four scalar gathers fused into one 4-float all-reduce; it rides on the first gradient exchange
        # point (one fork of the comm stream less) and is in flight under the rest of the backward
        met = st.metrics
        met_pending = self.do_comm
        joined = False

        def exchange(buckets):
            """The collectives of one exchange point; whichever comes first takes the metrics along."""
            nonlocal met_pending
            with_met, met_pending = met_pending, False

            def fn():
                if with_met:
                    self.comm.average_(met)
                for k in buckets:
                    self.comm.reduce_bucket(k)
            return fn

        if run_backward:
            if not st.fused_head:
                st.loss.backward(st.logits, st.y, st.dlogits, teacher=t_logits, grad_scale=self.inv_accum, stream=s)
            self._logit_terms(st, s, True)
            nseg = st.nseg_run
            due = st.comm_after if (self.do_comm and boundary) else {}
            aux = self.aux_stream.cuda_stream if self.aux_stream is not None else None
            aux_open = False        # aux-stream work of an earlier call that nothing on the compute stream has waited for yet
            # exchange marks (include/mi3d.h, mi3d_unet_backward_marks): an eagerly launched step keeps the backward ONE call;
            # the library records an event when a bucket's gradients are complete and the exchange stream waits for THAT.
            # Recomputed every step: use_graph may be flipped on a live object, boundary changes per micro-step
            mid = [(sg, tuple(due[sg])) for sg in range(nseg - 1) if due.get(sg)]
            use_marks = bool(mid) and not self.use_graph and aux is None and len(mid) <= 4 and not self.no_marks
            if use_marks:
                while len(self._mark_handles) < len(mid):
                    self._mark_handles.append(_lib.new_event())
                call("mi3d_unet_backward_marks", (C.c_int * len(mid))(*[sg for sg, _ in mid]),
                     ptr_table(self._mark_handles[:len(mid)]), len(mid))
                due = {sg: b for sg, b in due.items() if sg >= nseg - 1}       # one run; only the last exchange is left to it
            for start, end, buckets, last in _segment_runs(nseg, due):
                # the compute stream joins the aux stream at the end of the LAST call only (in front of the optimizer); a call
                # that is followed by a gradient exchange leaves the join to the exchange stream (_on_comm_stream), so the
                # deep-level weight gradients keep running under the next segments.  Segmented graphs end a capture at every
                # exchange: there every call joins
                join = 1 if (last or self.use_graph or aux is None) else 0
                aux_open = aux_open or (aux is not None and not join)
                kw = dict(drop=drop, accumulate=accumulate, start=start, end=end, stream=s, aux=aux, events=self._events, join=join)
                if st.fused_head:
                    st.plan.backward_loss(st.x, st.loss, labels=st.y, teacher=t_logits, grad_scale=self.inv_accum, **kw)
                else:
                    st.plan.backward(st.x, dlogits=st.dlogits, **kw)
                if use_marks:
                    cs = self.comm_stream
                    for i, (sg, b) in enumerate(mid):
                        fn = exchange(b)
                        call("mi3d_stream_wait_event", cs.cuda_stream, self._mark_handles[i])
                        with torch.cuda.stream(cs):
                            fn()
                if buckets and not last:
                    comm(lambda fn=exchange(buckets): self._on_comm_stream(fn))
                elif buckets:
                    # the exchange behind the LAST segment has nothing left to hide under: it runs on the compute stream
                    # itself, after the join with the exchange stream (collectives of one communicator never overlap each
                    # other) -- one fork / join pair per step instead of two (a cross-queue dependency costs ~12 us)
                    joined = True
                    comm(self._join_comm)
                    comm(exchange(buckets))
            if aux_open:       # the last call may have had nothing for the aux stream: join what earlier calls left there
                torch.cuda.current_stream().wait_stream(self.aux_stream)
        else:
            self._logit_terms(st, s, False)
        if met_pending:
            comm(lambda: self._on_comm_stream(lambda: self.comm.average_(met)))
        if self.do_comm and not joined:
            comm(self._join_comm)

    def _logit_terms(self, st, s, with_grad):
        """The terms on the logits beside the overlap loss, each loss += weight * L and, with_grad, dlogits += its gradient: one
        pass each directly behind the loss backward, the boundary term (mi3d_boundary_loss) then the entropy term
        (mi3d_entropy_loss), in front of any exchange, so the metrics' all-reduce carries them.  Nothing without their keywords."""
        masked = self.ignore_index is not None
        dlogits = st.dlogits if with_grad else None
        if self._boundary_weight is not None:
            M.boundary_term(st.logits, st.dist, self.boundary_classes, labels=st.y if masked else None, ignore_index=self.ignore_index,
                            weight=self._boundary_weight, grad_scale=self.inv_accum, loss_out=st.metrics, dlogits=dlogits,
                            flags=_lib.BD_ADD_LOSS | (_lib.BD_ADD_GRAD if with_grad else 0), workspace=st.bd_ws, stream=s)
        if self._entropy_weight is not None:
            # without an ignore value every voxel counts: "counted" is "all"
            M.entropy_term(st.logits, labels=st.y if masked else None, ignore_index=self.ignore_index,
                           mode=M.ENTROPY_MODES[self.entropy_on] if masked else _lib.ENT_ALL, weight=self._entropy_weight,
                           grad_scale=self.inv_accum, loss_out=st.metrics, dlogits=dlogits,
                           flags=_lib.ENT_ADD_LOSS | (_lib.ENT_ADD_GRAD if with_grad else 0), workspace=st.ent_ws, stream=s)

    def _load_batch(self, images, labels, dist, non_blocking):
        st = self._prepare(images)
        if self._boundary_weight is None:
            if dist is not None:
                raise Mi3dError("TrainStep was built without boundary_weight: it has no use for dist")
            self._load(st, non_blocking, x=images, y=labels)
        elif dist is not None:
            self._load(st, non_blocking, x=images, y=labels, dist=dist)
        else:
            self._load(st, non_blocking, x=images, y=labels)
            d = st.desc
            st.dist.copy_(surface.signed_distance_maps(st.y.view(d.N, d.D, d.H, d.W), self.boundary_classes, spacing=self.boundary_spacing))

    def load_batch(self, images, labels, dist=None):
        """Copy a batch into the static buffers (then step_static() runs on it).  dist: TrainStep(boundary_weight=...)."""
        self._load_batch(images, labels, dist, False)

    def step(self, images, labels, last_batch=False, dist=None):
        """One micro-step on (images (N,Cin,D,H,W) float, labels (N,1,D,H,W) int64).  Returns a device float32[4]
        tensor {loss, iou, dice, acc} (already averaged over ranks when world > 1).
        last_batch=True on the final batch of an epoch: the optimizer steps there even inside an accumulation window and
        the next epoch starts a new window, as accelerate does for the reference's prepared loaders (see _run).
        dist: the signed distance maps (N, K, D, H, W) float32 of a step built with boundary_weight; None computes them."""
        self._load_batch(images, labels, dist, True)
        return self.step_static(last_batch=last_batch)

    @torch.no_grad()
    def evaluate(self, images, labels):
        """model.eval() forward + loss + metrics (train_unet.py:259-305: the TRAINING loss_fn; distill_unet.py:136-160:
        combined_loss), averaged over ranks like the reference's gather().mean(); returns device float32[4].  Has its own
        static state: a validation batch of another shape (the reference validates with batch 1) does not disturb the
        captured training graph.  Under data parallelism rank 0's BatchNorm buffers are broadcast first: DDP broadcasts them at
        every forward, so the reference validates with rank 0's running statistics on every rank."""
        if self.do_comm:
            self.sync_buffers()
        st = self._prepare(images, mode="eval")
        st.x.copy_(images)
        st.y.copy_(labels.reshape(st.y.shape))
        plan, loss, s = st.plan, st.loss, stream_ptr()
        fused = (not _lib.get_route("no_head_loss") and not self.keep_logits and
                 _lib.lib().mi3d_unet_head_loss_supported(plan.d, loss.cfg_ref) == 1)
        if fused:       # head + loss + metrics on the decoder output: the validation logits are never written either
            plan.infer(st.x, stream=s)
            plan.head_loss_forward(loss, labels=st.y, stream=s)
        else:
            plan.infer(st.x, logits=st.logits, stream=s)
            loss.metrics_forward(st.logits, st.y, stream=s)
        out = st.metrics.clone()
        self.comm.average_(out)
        return out


class DannStep(_StepBase):
    """Native DANN micro-step (train_dann.py:233-300), single-GPU or data-parallel.

    Kernel sequence: source forward (workspace A, GAP -> feat[0:N]) ; target forward (workspace B, the FULL net as the
    reference runs it, Q4; GAP -> feat[N:2N]) ; loss + metrics on the source logits ; discriminator MLP forward on the
    2N feature rows (rows are independent, so the reference's two calls are one) ; row CE with labels [0]*N + [1]*N ;
    discriminator backward (its parameter gradients carry the lambda of `total = task + lambda*domain`) ; U-Net
    backward of the source graph (dlogits and dgap, gap_scale = -lambda = the gradient reversal, so the encoder sees
    -lambda^2 dL_dom/df, Q3) interleaved segment by segment with the backward of the target graph (dgap only:
    bottleneck + encoder, accumulating into the same gradient arena) ; two arena AdamW updates.
    Under DP the discriminator arena is one more bucket, in flight under the whole U-Net backward.

    entropy_weight: a float (0.0 included) adds entropy minimisation on the target batch (MinEnt of ADVENT, Vu et al.; include/mi3d.h,
    mi3d_entropy_loss), the companion of the adversarial loss and the only way the target batch reaches the decoder and the head:
    total = task + lambda * domain + entropy_weight * L_ent.  The target forward then writes its logits (static `t_logits`), one pass
    over them in mode ALL stores the gradient (static `t_dlogits`, scaled by 1 / grad_accum) and the weighted value (a sixth
    metrics slot), and the target graph's backward runs EVERY segment, decoder included, with dlogits and dgap: the target's decoder
    backward is real extra work.  step() then returns float32[6]; task_loss stays the reference's figure.  The property
    entropy_weight may be set between steps; like lr it is a kernel argument, so a captured graph is captured again.  None
    (default): five values and the kernels the step always launched."""
    _n_metrics = 5

    def __init__(self, seg_model, disc_model, loss="ce_tversky", lambda_domain=0.1, lr=1e-3, weight_decay=0.01,
                 betas=(0.9, 0.999), eps=1e-8, grad_accum=1, process_group=None, compute_dtype=None, use_graph=False,
                 force_comm=False, overlap_forwards=True, entropy_weight=None):
        self._entropy_weight = None
        if entropy_weight is not None:
            self._entropy_weight = _finite_weight(entropy_weight, "entropy_weight")
            self._n_metrics = 6          # per instance: task, iou, dice, acc, domain, weighted target entropy
        self._init_common(seg_model, lr, weight_decay, betas, eps, grad_accum, process_group, compute_dtype, use_graph,
                          force_comm)
        # The target forward does not depend on the source forward (train_dann.py:268-272): it runs on its own stream beside it.
        # Both are forwards of ONE model in train mode, i.e. both update the same BatchNorm running statistics, source first:
        # the target forward runs with the update DEFERRED (mi3d_unet_forward training = 2 publishes its batch statistics as
        # doubles) and mi3d_unet_bn_apply_deferred applies it after the join -- buffers bit-identical to the serial order.
        self.fwd_stream = concurrent_stream(self.device, role="fwd") if overlap_forwards else None
        self.disc = disc_model
        self.lam = float(lambda_domain)
        self.cfg = _loss_cfg(loss)
        self.eval_cfg = self.cfg
        self.lins = [disc_model.net[0], disc_model.net[3], disc_model.net[6], disc_model.net[8]]
        self.disc_p = [float(disc_model.net[2].p), float(disc_model.net[5].p)]
        for p in disc_model.parameters():
            _lib.require_cuda(p, "DannStep discriminator")
        self.disc_arena = ParamArena(disc_model.parameters(), self.device)
        # train_dann.py:421-422: both optimizers share lr / weight decay
        self.disc_optimizer = ArenaAdamW(disc_model.parameters(), lr, betas, eps, weight_decay)
        if self.world > 1:
            self.broadcast_parameters()
            dist.broadcast(self.disc_arena.p, src=0, group=process_group)

    def _hyper(self):
        g = self.disc_optimizer.param_groups[0]
        return super()._hyper() + (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                   float(g["weight_decay"]), self._entropy_weight)

    @property
    def entropy_weight(self):
        return self._entropy_weight

    @entropy_weight.setter
    def entropy_weight(self, value):
        """The weight of the target entropy term; only a step built with one has the term (and the buffers) to weigh."""
        if self._entropy_weight is None:
            raise Mi3dError("DannStep was built without entropy_weight: the step has no entropy term to weigh")
        self._entropy_weight = _finite_weight(value, "entropy_weight")

    def _mutable_state(self):
        d = self.disc_arena
        return super()._mutable_state() + [d.p, d.g, d.m, d.v, d.step, self._disc_rng()]

    def _disc_rng(self):
        st = getattr(self.disc, "_mi3d_rng_state", None)
        if st is None or st.device != self.device:
            st = torch.tensor([(torch.initial_seed() + 0x5DEECE66D) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64,
                              device=self.device)
            self.disc._mi3d_rng_state = st
        return st

    def _check_mode(self):
        if not self.model.training or not self.disc.training:
            raise Mi3dError("DannStep.step() needs both models in train mode (train_dann.py:226-227)")

    def _prepare(self, xs, xt):
        if tuple(xs.shape) != tuple(xt.shape):
            raise Mi3dError(f"source batch {tuple(xs.shape)} and target batch {tuple(xt.shape)} must have one shape "
                            "(train_dann.py:399-400: both loaders use args.batch_size)")
        if not all(p.requires_grad for p in self.arena.params):
            raise Mi3dError("DannStep: frozen segmentation parameters are not supported")
        return super()._prepare(xs)

    def _extend(self, st):
        """DannStep's part of a static state: the target graph (input, workspace, Dropout scales), the discriminator's
        activations and the side table of the deferred BatchNorm update."""
        desc, dev = st.desc, self.device
        n, F = desc.N, 2 * desc.features[st.L - 1]
        if self.lins[0].in_features != F:
            raise Mi3dError(f"discriminator expects {self.lins[0].in_features} features, the bottleneck has {F}")
        st.xt = torch.empty_like(st.x)
        st.drop_t = torch.empty_like(st.drop)
        st.feat = torch.empty((2 * n, F), dtype=torch.float32, device=dev)
        st.dfeat = torch.empty((2 * n, F), dtype=torch.float32, device=dev)
        st.gap, st.dgap = (st.feat[:n], st.feat[n:]), (st.dfeat[:n], st.dfeat[n:])       # (source rows, target rows)
        st.domain_loss = st.metrics[4:5]                  # metrics = task, iou, dice, acc, domain (, weighted target entropy)
        if self._entropy_weight is not None:
            if not 2 <= desc.out_channels <= 8:
                raise Mi3dError(f"DannStep: the entropy term takes 2 to 8 logit channels, the head has {desc.out_channels}")
            st.t_logits = torch.empty(st.logits_shape, dtype=torch.float32, device=dev)
            st.t_dlogits = torch.empty(st.logits_shape, dtype=torch.float32, device=dev)
            st.entropy_loss = st.metrics[5:6]
            st.ent_ws = M.entropy_workspace(n, desc.D * desc.H * desc.W, dev)
        widths = [l.out_features for l in self.lins]
        st.acts = [torch.empty((2 * n, w), dtype=torch.float32, device=dev) for w in widths]
        st.gacts = [torch.empty((2 * n, w), dtype=torch.float32, device=dev) for w in widths]
        st.lin_ws = torch.empty(2 * n * max(widths), dtype=torch.float32, device=dev)
        st.ddrop = [torch.empty((2 * n, widths[i]), dtype=torch.float32, device=dev) for i in (0, 1)]
        st.dlabels = torch.cat([torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64)]).to(dev)
        # the target graph: the source's tables and a workspace of its own; when its forward runs beside the source's, the side
        # buffers of the deferred BatchNorm update (double[2C] per layer) stand in the running_mean slots of its buffer table
        side = None
        if self.fwd_stream is not None:
            bufs = st.plan.buffers
            st.side = torch.zeros(sum(2 * b.numel() for b in bufs[::3]), dtype=torch.float64, device=dev)
            side, off = [], 0
            for i, b in enumerate(bufs):
                side.append(st.side[off:off + 2 * b.numel()] if i % 3 == 0 else None)
                off += 2 * b.numel() if i % 3 == 0 else 0
        st.target = st.plan.sibling(dev, buffers=side)
        st.opt_ranges = [(0, self.arena.numel)]

    def _enqueue(self, st, variant, comm):
        first, boundary = variant
        s = stream_ptr()
        seg, disc, src, tgt, loss = self.model, self.disc, st.plan, st.target, st.loss
        accumulate = 0 if first else 1
        n, lam = st.desc.N, self.lam
        # Dropout3d masks: one independent draw per forward (source, then target), like two module calls
        p = float(getattr(seg, "dropout_rate", 0.0))
        rng = lambda: engine._rng_state(seg, self.device)      # noqa: E731
        injected = getattr(seg, "_mi3d_injected_drop_scales", None) or (None, None)       # tests: (source scales, target scales)
        drop_s = engine.fill_drop_scales(st.drop, p, rng, injected[0], s)
        drop_t = engine.fill_drop_scales(st.drop_t, p, rng, injected[1], s)
        (gap_s, gap_t), fs = st.gap, self.fwd_stream
        ent = self._entropy_weight is not None
        t_logits = st.t_logits if ent else None      # without the entropy term the target logits are never read: the head is not run
        if fs is not None:
            fs.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(fs):
                tgt.forward(st.xt, drop=drop_t, training=BN_PUBLISH | THIN_CONSUMERS, logits=t_logits, gap=gap_t, stream=fs.cuda_stream)
        fused = st.fused_head
        beside = TRAIN | THIN_CONSUMERS      # two forwards side by side; also in the serial order, so that both orders run the
        #                                      same kernels and stay bitwise equal
        if fused:       # source head + loss + metrics in one pass, logits never written (mi3d_unet_forward_loss)
            src.forward_loss(st.x, loss, drop=drop_s, training=beside, labels=st.y, gap=gap_s, stream=s)
        else:
            src.forward(st.x, drop=drop_s, training=beside, logits=st.logits, gap=gap_s, stream=s)
        if fs is not None:
            torch.cuda.current_stream().wait_stream(fs)
            src.bn_apply_deferred(tgt, stream=s)
        else:
            tgt.forward(st.xt, drop=drop_t, training=beside, logits=t_logits, gap=gap_t, stream=s)
        if not fused:
            loss.metrics_forward(st.logits, st.y, stream=s)
            loss.backward(st.logits, st.y, st.dlogits, grad_scale=self.inv_accum, stream=s)
        if ent:
            # entropy minimisation on every target voxel: the weighted value to its metrics slot, the gradient STORED to t_dlogits
            M.entropy_term(st.t_logits, mode=_lib.ENT_ALL, weight=self._entropy_weight, grad_scale=self.inv_accum,
                           loss_out=st.entropy_loss, dlogits=st.t_dlogits, workspace=st.ent_ws, stream=s)
        # ---- discriminator on the 2N feature rows (train_dann.py:34-49,276-283)
        dinj = getattr(disc, "_mi3d_injected_drop_scales", None) or (None, None)      # tests: [mask after net.1, mask after net.4]
        dd = [engine.fill_drop_scales(st.ddrop[i], self.disc_p[i], self._disc_rng, dinj[i], s) for i in (0, 1)] + [None, None]
        relus = (1, 1, 1, 0)
        feat = inp = st.feat
        for i, l in enumerate(self.lins):
            call("mi3d_linear_forward", ptr(inp), ptr(l.weight), ptr(l.bias), ptr(st.acts[i]), 2 * n, l.in_features,
                 l.out_features, relus[i], ptr(dd[i]), s)
            inp = st.acts[i]
        # domain_loss = CE/accum (train_dann.py:283); its gradient enters `total` with weight lambda (:285)
        call("mi3d_softmax_ce_rows", ptr(st.acts[3]), ptr(st.dlabels), 2 * n, 2, ptr(st.domain_loss),
             ptr(st.gacts[3]), lam / self.accum, s)
        da = self.disc_arena
        dgp = da.grad_ptrs()
        for i in (3, 2, 1, 0):
            l = self.lins[i]
            x_in = feat if i == 0 else st.acts[i - 1]
            gx = st.dfeat if i == 0 else st.gacts[i - 1]
            call("mi3d_linear_backward", ptr(x_in), ptr(l.weight), ptr(st.acts[i]), ptr(st.gacts[i]), 2 * n,
                 l.in_features, l.out_features, relus[i], ptr(dd[i]), ptr(gx), dgp[2 * i], dgp[2 * i + 1], accumulate, 1.0,
                 ptr(st.lin_ws), s)
        do_comm = self.do_comm and boundary
        if self.do_comm:
            met = st.metrics
            comm(lambda: self._on_comm_stream(lambda: self.comm.average_(met)))
        if do_comm:
            dg = da.g
            comm(lambda: self._on_comm_stream(lambda: self.comm.average_(dg)))
        # ---- one backward over both graphs, run by run: gradient reversal = gap_scale -lambda
        L = st.L
        due = {sg: (sg,) for sg in self.comm.buckets} if do_comm else {}
        for start, end, buckets, _ in _segment_runs(2 * L + 2, due):
            kw = dict(drop=drop_s, dgap=st.dgap[0], gap_scale=-lam, accumulate=accumulate, start=start, end=end, stream=s)
            if fused:
                src.backward_loss(st.x, loss, labels=st.y, grad_scale=self.inv_accum, **kw)
            else:
                src.backward(st.x, dlogits=st.dlogits, **kw)
            # without the entropy term the target graph has no decoder part; with it every segment runs, head and decoder included
            t0 = start if ent else max(start, L + 1)
            if end > t0:
                tgt.backward(st.xt, drop=drop_t, dlogits=st.t_dlogits if ent else None, dgap=st.dgap[1], gap_scale=-lam, accumulate=1,
                             start=t0, end=end, stream=s)
            for k in buckets:
                comm(lambda k=k: self._on_comm_stream(lambda: self.comm.reduce_bucket(k)))
        if self.do_comm:
            comm(self._join_comm)
        if boundary:
            h = self._hyper()
            self._adamw(self.arena, st.opt_ranges, h[:5], s)
            self._adamw(self.disc_arena, [(0, self.disc_arena.numel)], h[5:10], s)

    def load_batch(self, source_images, source_labels, target_images):
        self._load(self._prepare(source_images, target_images), False, x=source_images, xt=target_images, y=source_labels)

    def step(self, source_images, source_labels, target_images, last_batch=False):
        """One micro-step.  Returns device float32[5] = {task_loss, iou, dice, acc, domain_loss} (source-domain metrics,
        train_dann.py:291-299; losses un-divided by the accumulation count like the reference's running sums); built with
        entropy_weight, float32[6]: entropy_weight * the target batch's entropy term comes last (task_loss stays the reference's).
        last_batch: train_dann.py:287 also steps on the final batch of an epoch."""
        self._load(self._prepare(source_images, target_images), True, x=source_images, xt=target_images, y=source_labels)
        return self.step_static(last_batch=last_batch)

    @torch.no_grad()
    def evaluate(self, images, labels):
        """train_dann.py:304-327: eval-mode source-domain validation with the training loss_fn."""
        from . import unet_dann  # noqa: F401
        was = self.model.training
        self.model.eval()
        try:
            logits, _ = self.model(images, return_features=False)
        finally:
            self.model.train(was)
        n, c, v, lab = M._prep(logits, labels)
        loss = engine.LossGroup(self.eval_cfg, c, self.device)
        loss.metrics_forward(logits, lab, stream=stream_ptr())
        out = loss.metrics
        self.comm.average_(out)
        return out
