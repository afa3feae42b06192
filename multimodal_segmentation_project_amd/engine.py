"""Host-side engine: binds the reference's nn.Module surface to the whole-network HIP plan (csrc/plan.hip).

``Plan`` is the call layer every host path goes through: it owns the descriptor, the pointer tables and the argument order of
each mi3d_unet_* entry; ``LossGroup`` is what the loss calls share.  One autograd node per network forward: ``_UNetFn.forward`` makes ONE C call that launches every forward kernel,
``_UNetFn.backward`` makes one C call per backward segment (so data-parallel gradient all-reduces can be
interleaved, see dp.py).  PyTorch only owns memory (params, buffers, logits, the workspace) and the stream.

Reference surface mirrored here: models/unet.py:64-90 and models/unet_dann.py:65-98 (forward), the autograd
backward triggered by train_unet.py:225 / train_dann.py:286.
"""
import copy
import ctypes as C

import torch

from . import _lib
from ._lib import UNetDesc, call, ptr, ptr_table, stream_ptr

_default_compute_dtype = None


def set_compute_dtype(dtype):
    """Process-wide internal activation dtype: torch.float32 (exact path), torch.bfloat16 (fast path) or None
    (= follow torch.autocast, fp32 outside it).  Mirrors accelerate's mixed_precision flag (train_unet.py:533)."""
    global _default_compute_dtype
    if dtype not in (None, torch.float32, torch.bfloat16):
        raise _lib.Mi3dError(f"unsupported compute dtype {dtype}")
    _default_compute_dtype = dtype


def resolve_compute_dtype(model):
    dt = getattr(model, "compute_dtype", None)
    if dt is None:
        dt = _default_compute_dtype
    if dt is None:
        if torch.is_autocast_enabled():
            # fp16 autocast (the reference's shipped setting, run_training.sh:28) maps to bf16 here: same MFMA
            # rate on gfx950, fp32 range, no GradScaler needed (loss scaling still passes through: backward is linear)
            dt = torch.bfloat16
        else:
            dt = torch.float32
    return dt


def build_desc(model, x, dtype):
    """Descriptor for the input x (a tensor or its shape)."""
    shape = tuple(getattr(x, "shape", x))
    if len(shape) != 5:
        raise _lib.Mi3dError(f"expected a (N,C,D,H,W) input, got shape {shape}")
    feats = [blk.double_conv[0].out_channels for blk in model.encoder]
    if len(feats) > _lib.MAX_LEVELS:
        raise _lib.Mi3dError(f"{len(feats)} levels > {_lib.MAX_LEVELS}")
    d = UNetDesc()
    d.in_channels = model.encoder[0].double_conv[0].in_channels
    d.out_channels = model.final_conv.out_channels
    d.n_levels = len(feats)
    for i, f in enumerate(feats):
        d.features[i] = f
    d.N, d.D, d.H, d.W = shape[0], shape[2], shape[3], shape[4]
    if shape[1] != d.in_channels:
        raise _lib.Mi3dError(f"input has {shape[1]} channels, model expects {d.in_channels}")
    d.dtype = _lib.dtype_code(dtype)
    bn = model.encoder[0].double_conv[1]
    if bn.momentum is None:
        raise _lib.Mi3dError("BatchNorm3d(momentum=None) (cumulative moving average) is not supported; the reference "
                             "uses the default momentum 0.1 (models/unet.py:12,16)")
    d.bn_momentum = bn.momentum
    d.bn_eps = bn.eps
    return d


def _rng_state(model, device):
    st = getattr(model, "_mi3d_rng_state", None)
    if st is None or st.device != device:
        st = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        model._mi3d_rng_state = st
    return st


def fill_drop_scales(buf, p, rng, injected=None, stream=None):
    """Dropout scales into the device float buffer `buf`: the injected ones (tests), or ONE mi3d_dropout_scales draw of rate p
    that advances the device RNG state `rng` (a callable: a draw that does not happen creates no state).  Returns buf, or None
    for "no dropout" (p = 0 and nothing injected)."""
    if injected is not None:
        if injected.numel() != buf.numel():
            raise _lib.Mi3dError(f"injected dropout scales have {injected.numel()} entries, plan needs {buf.numel()}")
        buf.copy_(injected.reshape(buf.shape))
        return buf
    if p > 0.0:
        call("mi3d_dropout_scales", ptr(buf), buf.numel(), p, ptr(rng()), stream_ptr() if stream is None else stream)
        return buf
    return None


def make_drop_scales(model, desc, p, device, injected=None):
    """Dropout3d channel scales for all 2*(2L+1) dropout layers (models/unet.py:14,18) in ONE kernel launch: a new buffer holding
    the injected scales or a draw of rate p; None when p == 0 and nothing is injected."""
    out = torch.empty(_lib.lib().mi3d_unet_dropout_count(C.byref(desc)), dtype=torch.float32, device=device)
    return fill_drop_scales(out, float(p), lambda: _rng_state(model, device), injected)


# `training` of Plan.forward / forward_loss (include/mi3d.h, mi3d_unet_forward): 0 = eval mode (running statistics), else
TRAIN = 1               # batch statistics, running statistics updated in place
BN_PUBLISH = 2          # batch statistics, the update deferred: (mean, unbiased variance) published as doubles into the side buffers
#                         the running_mean slots of the buffer table point at; Plan.bn_apply_deferred applies them later
THIN_CONSUMERS = 4      # or-ed to either: another forward runs beside this one, the BatchNorm apply passes stay thin


HEAD_VOTES = "mi3d_unet_head_votes"      # Plan.head_votes' entry; its argument order is written down there and nowhere else
HEAD_VOTES_WINDOW = "mi3d_unet_head_votes_window"      # Plan.head_votes_window's, likewise


class LossGroup:
    """What the loss calls share: the configuration, metrics = {loss, iou, dice, acc, ...} (device float[n_metrics]; the loss
    is written to [0], the three metrics to [1:4]), the 20 loss coefficients the backward reads, and the two workspaces.
    ignore_index (None: every voxel counts): the label value the loss and the metrics leave out; the calls then go to the
    `_masked` entries (include/mi3d.h, "Ignore value"), which take it right after the configuration."""

    def __init__(self, cfg, classes, device, n_metrics=4, ignore_index=None):
        lib = _lib.lib()
        self.cfg = cfg
        self.ignore_index = ignore_index
        self.masked = "" if ignore_index is None else "_masked"                      # suffix of every loss entry
        self.cfg_args = (C.byref(cfg),) if ignore_index is None else (C.byref(cfg), int(ignore_index))
        self.metrics = torch.empty(n_metrics, dtype=torch.float32, device=device)
        self.coef = torch.empty(_lib.LOSS_COEF_FLOATS, dtype=torch.float32, device=device)
        self.loss_ws = torch.empty(lib.mi3d_seg_loss_workspace_bytes(classes), dtype=torch.uint8, device=device)
        self.met_ws = torch.empty(lib.mi3d_seg_metrics_workspace_bytes(classes), dtype=torch.uint8, device=device)
        m = self.metrics.data_ptr()
        self.cfg_ref = C.byref(cfg)
        self.fwd = (*self.cfg_args, m, ptr(self.coef), m + 4, ptr(self.loss_ws), ptr(self.met_ws))      # as every forward takes them

    def metrics_forward(self, logits, labels, *, teacher=None, stream):
        """Loss + metrics of (N, C, D, H, W) float logits in one pass (mi3d_seg_loss_metrics_forward)."""
        n, c, d = logits.shape[:3]
        call("mi3d_seg_loss_metrics_forward" + self.masked, ptr(logits), ptr(labels), ptr(teacher), n, c, d, logits.numel() // (n * c),
             *self.fwd, stream)

    def backward(self, logits, labels, dlogits, *, teacher=None, grad_scale, stream):
        """dlogits = grad_scale[0] * d loss / d logits (mi3d_seg_loss_backward) from the coefficients the forward left."""
        n, c = logits.shape[:2]
        call("mi3d_seg_loss_backward" + self.masked, ptr(logits), ptr(labels), ptr(teacher), n, c, logits.numel() // (n * c),
             *self.cfg_args, ptr(self.coef), ptr(grad_scale), ptr(dlogits), stream)


class Plan:
    """One whole-network call sequence: descriptor, workspace size (queried once), parameter / buffer / gradient pointer tables
    and, after own_workspace(), the workspace.  One method per mi3d_unet_* entry, keyword arguments, tensors (or None) for
    pointers: the argument order of include/mi3d.h is written down here and nowhere else."""

    def __init__(self, model, shape, dtype, params=None, buffers=None, grads=None):
        self.desc = build_desc(model, shape, dtype)
        self.d = C.byref(self.desc)
        self.ws_bytes = _lib.lib().mi3d_unet_workspace_bytes(self.d)
        if self.ws_bytes == 0:
            _lib.check(-1, "mi3d_unet_workspace_bytes")
        self.ws = self.ws_ptr = self.gtab = None
        self.set_tables(list(model.parameters()) if params is None else params,
                        list(model.buffers()) if buffers is None else buffers, grads)

    def set_tables(self, params=None, buffers=None, grads=None):
        """Tables from tensors (grads: device addresses, None = no gradient wanted); what is None stays."""
        if params is not None:
            self.params, self.ptab = list(params), ptr_table([p.data_ptr() for p in params])
        if buffers is not None:
            self.buffers, self.btab = list(buffers), ptr_table([ptr(b) for b in buffers])
        if grads is not None:
            self.gtab = ptr_table(list(grads))

    def own_workspace(self, device):
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.ws_ptr = self.ws.data_ptr()
        return self

    def release_workspace(self):
        """Give the workspace back; a call made afterwards passes NULL, which the library refuses."""
        self.ws = self.ws_ptr = None

    def sibling(self, device, **tables):
        """A second call sequence of the same descriptor with a workspace of its own (the distillation teacher, DANN's target
        graph); tables that are not given are shared."""
        p = copy.copy(self)
        p.set_tables(**tables)
        return p.own_workspace(device)

    def forward(self, x, *, drop=None, training=TRAIN, logits=None, gap=None, stream):
        call("mi3d_unet_forward", self.d, ptr(x), self.ptab, self.btab, ptr(drop), training, ptr(logits), ptr(gap),
             self.ws_ptr, self.ws_bytes, stream)

    def infer(self, x, *, logits=None, gap=None, stream):
        call("mi3d_unet_infer", self.d, ptr(x), self.ptab, self.btab, ptr(logits), ptr(gap), self.ws_ptr, self.ws_bytes, stream)

    def forward_loss(self, x, loss, *, drop=None, training=TRAIN, labels, teacher=None, logits=None, gap=None, stream):
        call("mi3d_unet_forward_loss" + loss.masked, self.d, ptr(x), self.ptab, self.btab, ptr(drop), training, ptr(labels), ptr(teacher),
             *loss.fwd, ptr(logits), ptr(gap), self.ws_ptr, self.ws_bytes, stream)

    def head_loss_forward(self, loss, *, labels, teacher=None, logits=None, stream):
        call("mi3d_unet_head_loss_forward" + loss.masked, self.d, self.ptab, ptr(labels), ptr(teacher), *loss.fwd, ptr(logits),
             self.ws_ptr, self.ws_bytes, stream)

    def backward(self, x, *, drop=None, dlogits=None, dgap=None, gap_scale=1.0, accumulate=0, start, end, stream, aux=None,
                 events=None, join=1):
        call("mi3d_unet_backward", self.d, ptr(x), self.ptab, self.gtab, ptr(drop), ptr(dlogits), ptr(dgap), gap_scale,
             accumulate, start, end, self.ws_ptr, self.ws_bytes, stream, aux, events, join)

    def backward_loss(self, x, loss, *, drop=None, labels, teacher=None, grad_scale, dgap=None, gap_scale=1.0, accumulate=0,
                      start, end, stream, aux=None, events=None, join=1):
        call("mi3d_unet_backward_loss" + loss.masked, self.d, ptr(x), self.ptab, self.gtab, ptr(drop), ptr(labels), ptr(teacher), *loss.cfg_args,
             ptr(loss.coef), ptr(grad_scale), ptr(dgap), gap_scale, accumulate, start, end, self.ws_ptr, self.ws_bytes, stream,
             aux, events, join)

    def head_labels(self, *, labels=None, out, counts=None, head_ws=None, stream):
        call("mi3d_unet_head_labels", self.d, self.ptab, ptr(labels), ptr(out), ptr(counts), ptr(head_ws), self.ws_ptr,
             self.ws_bytes, stream)

    def head_votes(self, *, flip, view, views, flags=0, votes=None, out=None, confidence=None, labels=None, counts=None, head_ws=None,
                   stream):
        """One view of a flip / model ensemble on the decoder output the last infer() left (mi3d_unet_head_votes)."""
        call(HEAD_VOTES, self.d, self.ptab, flip, view, views, flags, ptr(votes), ptr(out), ptr(confidence), ptr(labels),
             ptr(counts), ptr(head_ws), self.ws_ptr, self.ws_bytes, stream)

    def head_votes_window(self, *, flips, tables, origins, acc, stream):
        """The window samples of the decoder output the last infer() left, weighted by `tables` (g_d, g_h, g_w) and added into
        acc (C, D, H, W) at `origins` (mi3d_unet_head_votes_window).  flips, origins: host tables (_lib.int_table), one code and
        three ints per sample."""
        call(HEAD_VOTES_WINDOW, self.d, self.ptab, flips, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), origins, ptr(acc),
             acc.shape[1], acc.shape[2], acc.shape[3], self.ws_ptr, self.ws_bytes, stream)

    def bn_apply_deferred(self, side, *, stream):
        """side: the Plan whose buffer table holds the side buffers a BN_PUBLISH forward filled."""
        call("mi3d_unet_bn_apply_deferred", self.d, self.btab, side.btab, stream)


def _outputs(desc, want_gap, device):
    logits = torch.empty((desc.N, desc.out_channels, desc.D, desc.H, desc.W), dtype=torch.float32, device=device)
    gap = None
    if want_gap:
        gap = torch.empty((desc.N, 2 * desc.features[desc.n_levels - 1]), dtype=torch.float32, device=device)
    return logits, gap


class _Hold:
    """Per-call context handed to the autograd node (not a tensor)."""
    __slots__ = ("plan", "training", "want_gap", "segment_hook")


class _UNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hold, x, drop, *params):
        plan = hold.plan.own_workspace(x.device)
        logits, gap = _outputs(plan.desc, hold.want_gap, x.device)
        plan.forward(x, drop=drop, training=int(hold.training), logits=logits, gap=gap, stream=stream_ptr())
        ctx.hold, ctx.drop = hold, drop
        ctx.save_for_backward(x, *params)
        ctx.set_materialize_grads(False)
        if gap is None:
            return logits
        return logits, gap

    @staticmethod
    def backward(ctx, dlogits, dgap=None):
        hold = ctx.hold
        plan = hold.plan
        x, *params = ctx.saved_tensors
        if dlogits is None and dgap is None:
            return (None, None, None) + (None,) * len(params)
        if not hold.training:
            # the backward kernels implement train-mode BatchNorm (batch statistics); an eval-mode forward normalised
            # with running statistics, whose gradient is a different formula
            raise _lib.Mi3dError("backward through a UNet3D forward that ran in eval mode is not supported: call "
                                 "model.train() (train_unet.py:208) or wrap evaluation in torch.no_grad()")
        if dlogits is not None:
            dlogits = dlogits.contiguous().float()
        if dgap is not None:
            dgap = dgap.contiguous().float()
        # without a logits gradient only encoder + bottleneck parameters receive gradient (DANN target pass)
        n_live = len(params) if dlogits is not None else 8 * (plan.desc.n_levels + 1)
        grads = [torch.empty_like(p) if (i < n_live and ctx.needs_input_grad[3 + i]) else None
                 for i, p in enumerate(params)]
        plan.set_tables(grads=[ptr(g) for g in grads])
        for seg in range(2 * plan.desc.n_levels + 2):      # one call per segment: the hook may exchange gradients between them (dp.py)
            plan.backward(x, drop=ctx.drop, dlogits=dlogits, dgap=dgap, start=seg, end=seg + 1, stream=stream_ptr())
            if hold.segment_hook is not None:
                hold.segment_hook(seg, grads)
        plan.release_workspace()
        return (None, None, None) + tuple(grads)


def plan_call(model, x):
    """The checked Plan of a whole-network call on the float32 (N,C,D,H,W) device input x (no workspace yet).  Shared by
    unet_forward and segment.predict_labels."""
    params = list(model.parameters())
    for p in params:
        _lib.require_cuda(p, "UNet3D parameter")
    plan = Plan(model, x.shape, resolve_compute_dtype(model), params=params)
    expect = _lib.lib().mi3d_unet_num_params(plan.d)
    if len(params) != expect or len(plan.buffers) != _lib.lib().mi3d_unet_num_buffers(plan.d):
        raise _lib.Mi3dError(f"module has {len(params)} parameters / {len(plan.buffers)} buffers, plan expects {expect}")
    return plan


def unet_forward(model, x, want_gap=False):
    """Shared body of unet.UNet3D.forward and unet_dann.UNet3D.forward."""
    _lib.require_cuda(x, "UNet3D.forward")
    x = x.detach().contiguous().float() if not x.requires_grad else x.contiguous().float()
    plan = plan_call(model, x)
    if not model.training and not (torch.is_grad_enabled() and any(q.requires_grad for q in plan.params)):
        # inference (train_unet.py:259-305 evaluate, test_model.py:242-251, the distillation teacher): BatchNorm folded
        # into the convs, no saved activations, no autograd node
        plan.own_workspace(x.device)
        logits, gap = _outputs(plan.desc, want_gap, x.device)
        plan.infer(x, logits=logits, gap=gap, stream=stream_ptr())
    else:
        hold = _Hold()
        hold.plan, hold.training, hold.want_gap = plan, bool(model.training), bool(want_gap)
        hold.segment_hook = getattr(model, "_mi3d_segment_hook", None)
        drop = None
        p = float(getattr(model, "dropout_rate", 0.0))
        injected = getattr(model, "_mi3d_injected_drop_scales", None)
        if model.training and (p > 0.0 or injected is not None):
            drop = make_drop_scales(model, plan.desc, p, x.device, injected)
        out = _UNetFn.apply(hold, x, drop, *plan.params)
        logits, gap = out if want_gap else (out, None)
    if model.output_activation is not None:
        logits = model.output_activation(logits)
    return logits, gap
