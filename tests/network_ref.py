"""The whole-network cases of tests/test_gpu_network_memory.py: the case table, the walk of every layer of a case through the route
predictors (tests/conv_ref.py, tests/up_ref.py and the backward's class of build_plan in
multimodal_segmentation_project_amd/csrc/plan.hip), seeded inputs and models, and
the float64 references (oracle/torch_ref.py with autograd on the CPU), computed once per case.  No GPU, nothing of the library
beyond the module classes that hold the parameters.

    name         net                                       N x D x H x W     why
    small_f32    in 2, out 3, features [4, 8] (golden)     2 x  8 x 12 x  4   direct kernels, in_channels > 1 (xcl), golden for every gradient
    deep_bf16    default (in 1, out 4, [16, 32, 64, 128])  1 x 16 x 16 x 32   first-layer MFMA, persistent 16->16 and 32->16 at level 0, the
                                                                              8-wide tile unsplit (encoder.1 half 0), ticket 2, 4, 8, 16 below
    flat_bf16    default                                   2 x 16 x 16 x 16   no persistent layer, a ticket layer at level 0 (decoder.3 half 0), N = 2
    ragged_bf16  default                                   1 x 21 x 20 x 36   persistent kernels with a ragged last tile in D (21 = 5 * 4 + 1),
                                                                              H (20 = 2 * 8 + 4) and W (36 = 2 * 16 + 4); odd D at level 0 (unfused
                                                                              pool) and nearest resizes at levels 0 and 2
    deep_f32     default                                   1 x 16 x 16 x 32   the fp32 statistics pass and the direct kernels on the default widths

(1 x 20 x 20 x 36 lands on the persistent kernels too, but 20 is five whole 4-deep tiles: 21 is the nearest D with a ragged one.)
Layer names: <block>.<half>, block = encoder.l / bottleneck / decoder.i as in the module; decoder.i works at level L - 1 - i.
"""
import functools
import os

import numpy as np
import torch

import conv_ref as CR
import up_ref as UR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_FEATURES = (16, 32, 64, 128)
IGNORE = 255
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}

# name: net, (N, D, H, W), dtype, and mi3d_unet_workspace_bytes of the case (recorded from the build this table was written with:
# a change of the arena's layout has to change these on purpose)
CASES = {
    "small_f32":   dict(net="small", shape=(2, 8, 12, 4), dtype="fp32", ws_bytes=2145024),
    "deep_bf16":   dict(net="default", shape=(1, 16, 16, 32), dtype="bf16", ws_bytes=53214976),
    "flat_bf16":   dict(net="default", shape=(2, 16, 16, 16), dtype="bf16", ws_bytes=75240192),
    "ragged_bf16": dict(net="default", shape=(1, 21, 20, 36), dtype="bf16", ws_bytes=58904064),
    "deep_f32":    dict(net="default", shape=(1, 16, 16, 32), dtype="fp32", ws_bytes=78661888),
}
NETS = {"small": dict(in_channels=2, out_channels=3, features=(4, 8)), "default": dict(in_channels=1, out_channels=4, features=DEFAULT_FEATURES)}

# What the table above promises, layer by layer: (conv route, split-K factor, ticket) of the training forward under the default
# switches.  tests/test_network_cases_cpu.py compares the walk with it, so a retune that moves a case off its route fails there.
PROMISED = {
    "small_f32":   {"encoder.0.0": (0, 1, 0), "bottleneck.1": (0, 1, 0)},
    "deep_bf16":   {"encoder.0.0": (1, 1, 0), "encoder.0.1": (2, 1, 0), "decoder.3.0": (2, 1, 0), "decoder.3.1": (2, 1, 0),
                    "encoder.1.0": (4, 1, 0), "encoder.1.1": (4, 2, 1), "encoder.2.1": (4, 4, 1), "encoder.3.1": (4, 8, 1),
                    "bottleneck.1": (4, 16, 1)},
    "flat_bf16":   {"encoder.0.0": (1, 1, 0), "encoder.0.1": (4, 1, 0), "decoder.3.0": (4, 2, 1), "decoder.3.1": (4, 1, 0)},
    "ragged_bf16": {"encoder.0.0": (1, 1, 0), "encoder.0.1": (2, 1, 0), "decoder.3.0": (2, 1, 0), "decoder.3.1": (2, 1, 0)},
    "deep_f32":    {"encoder.0.0": (0, 1, 0), "bottleneck.1": (0, 1, 0), "decoder.3.1": (0, 1, 0)},
}


def net_of(name):
    return NETS[CASES[name]["net"]]


def input_shape(name):
    n, d, h, w = CASES[name]["shape"]
    return (n, net_of(name)["in_channels"], d, h, w)


# ------------------------------------------------------------------------------------------------ the walk
def levels(name):
    """(L, channels per level incl. the bottleneck, (N, D, H, W) per level) as build_plan lays them out."""
    feats = list(net_of(name)["features"])
    n, d, h, w = CASES[name]["shape"]
    L = len(feats)
    return L, feats + [2 * feats[-1]], [(n, d >> l, h >> l, w >> l) for l in range(L + 1)]


def conv_layers(name):
    """Every 3x3x3 conv of the case in forward order: dict(name, block, half, level, cin, cout, geo, pooled)."""
    L, C, geo = levels(name)
    out = []
    for b in range(2 * L + 1):
        if b < L:
            block, level, cin, cout = f"encoder.{b}", b, (net_of(name)["in_channels"] if b == 0 else C[b - 1]), C[b]
        elif b == L:
            block, level, cin, cout = "bottleneck", L, C[L - 1], C[L]
        else:
            i = b - L - 1
            level = L - 1 - i
            block, cin, cout = f"decoder.{i}", 2 * C[level], C[level]
        g = geo[level]
        even = all(s % 2 == 0 for s in g[1:])
        for h in range(2):
            out.append(dict(name=f"{block}.{h}", block=b, half=h, level=level, cin=cin if h == 0 else cout, cout=cout, geo=g,
                            pooled=b < L and h == 1 and even))
    return out


def defer_class(layer, L, conv):
    """HalfP::defer of build_plan from the layer's forward route `conv` (conv_ref.predict_route: 2, 3 and 4 are the MFMA layer
    class, so the class predicate lives in conv_ref alone): 0 = the fused backward launch (and every layer that is not MFMA),
    1 = a decoder layer at a 16-wide-tile level, 2 = any MFMA layer at a deep level."""
    if conv not in (2, 3, 4):
        return 0
    if not CR.big_geo(layer["geo"]):
        return 2
    return 1 if layer["block"] > L else 0


def walk(name, routes=None):
    """{layer name: dict(conv, ksplit, ticket, stats, rows, consumer, defer)} and {upconvs.i: dict(kind, resized, ...)}."""
    L, C, geo = levels(name)
    bf16 = CASES[name]["dtype"] == "bf16"
    convs = {}
    for k in conv_layers(name):
        r = CR.predict_route(dict(cin=k["cin"], cout=k["cout"], geo=k["geo"], dtype=int(bf16)), routes)
        convs[k["name"]] = dict(r, defer=defer_class(k, L, r["conv"]))
    ups = {}
    for i in range(L):
        l = L - 1 - i
        ups[f"upconvs.{i}"] = UR.fwd_route(int(bf16), 2 * C[l], C[l], geo[l + 1], go=geo[l][1:])
    return convs, ups


def ragged_axes(name):
    """The axes (D, H, W) in which the full-resolution volume ends in a partial 4 x 8 x 16 tile."""
    _, d, h, w = CASES[name]["shape"]
    return (d % 4 != 0, h % 8 != 0, w % 16 != 0)


# ------------------------------------------------------------------------------------------------ models and inputs
def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def state_dict(name):
    """The model's float32 state_dict on the CPU: the golden fixture's for `small`, the reference's seeded init (seed 0, as
    default_model of the GPU tests) for `default`."""
    from multimodal_segmentation_project_amd.unet import UNet3D
    net = net_of(name)
    if CASES[name]["net"] == "small":
        g = _golden("small_unet")
        return {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd0/")}
    torch.manual_seed(0)
    m = UNet3D(in_channels=net["in_channels"], out_channels=net["out_channels"], dropout_rate=0.0)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def new_model(name):
    from multimodal_segmentation_project_amd.unet import UNet3D
    net = net_of(name)
    m = UNet3D(in_channels=net["in_channels"], out_channels=net["out_channels"], features=list(net["features"]), dropout_rate=0.0)
    m.load_state_dict(state_dict(name), strict=True)
    return m


def eval_buffers(name):
    """The BatchNorm buffers of the eval-mode sequences: the golden fixture's after its step for `small`; for `default` mean 0 and
    variance 0.1, which keeps the activations O(1) so that the label map is not one class (as tests/test_gpu_votes.py does)."""
    if CASES[name]["net"] == "small":
        g = _golden("small_unet")
        return {k[4:]: v for k, v in g.items() if k.startswith("sd1/") and ("running" in k or "num_batches" in k)}
    out = {}
    for k, v in state_dict(name).items():
        if "running" in k or "num_batches" in k:
            out[k] = np.full(tuple(v.shape), 0.1, np.float32) if k.endswith("running_var") else v.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x float32 (N, Cin, D, H, W), labels int64 (N, 1, D, H, W), masked labels (about a quarter at IGNORE; with N > 1 the last
    sample keeps every label) and dgap float32 (N, 2 * features[-1]): seeded, read-only numpy."""
    net = net_of(name)
    shape = input_shape(name)
    n = shape[0]
    if CASES[name]["net"] == "small":
        g = _golden("small_unet")
        x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
        assert tuple(x.shape) == shape, (tuple(x.shape), shape)
    else:
        gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
        x = torch.randn(shape, generator=gen)
        y = torch.randint(0, net["out_channels"], (n, 1) + shape[2:], generator=gen)
    gen = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    drop = torch.rand(y.shape, generator=gen) < 0.25
    if n > 1:
        drop[-1] = False
    ym = torch.where(drop, torch.full_like(y, IGNORE), y)
    dgap = torch.randn(n, 2 * net["features"][-1], generator=gen)
    out = dict(x=x.numpy(), y=y.numpy().astype(np.int64), y_masked=ym.numpy().astype(np.int64), dgap=dgap.numpy())
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ float64 references
def _sd64(name, grad):
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state_dict(name).items()}
    if grad:
        for k, v in sd.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)
    return sd


def _grads(sd):
    return {k: (v.grad.numpy().copy() if v.grad is not None else None) for k, v in sd.items() if v.requires_grad}


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _frozen(a)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """mode 'train': logits, gap, loss (combined), grads of the loss, the BatchNorm buffers after the forward;
            'dgap': grads of GAP_SCALE * sum(gap * dgap) (the DANN target pass: decoder entries None);
            'eval': logits and gap of the eval-mode forward.  float64 on the CPU, autograd for the gradients."""
    from oracle import torch_ref
    i = inputs(name)
    x = torch.from_numpy(i["x"].copy()).double()
    if mode == "eval":
        sd = _sd64(name, False)
        sd.update({k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in eval_buffers(name).items()})
        with torch.no_grad():
            lo, gap, _ = torch_ref.unet3d_forward(sd, x, train=False, return_features=True)
        return _frozen(dict(logits=lo.numpy(), gap=gap.numpy()))
    sd = _sd64(name, True)
    lo, gap, updates = torch_ref.unet3d_forward(sd, x, train=True, return_features=True)
    out = dict(logits=lo.detach().numpy(), gap=gap.detach().numpy())
    if mode == "train":
        loss = torch_ref.seg_loss(lo, torch.from_numpy(i["y"].copy()), "combined")
        loss.backward()
        out.update(loss=float(loss.detach()), buffers={k: v.detach().numpy() for k, v in updates.items()})
    elif mode == "dgap":
        (GAP_SCALE * (gap * torch.from_numpy(i["dgap"].copy()).double()).sum()).backward()
    else:
        raise KeyError(mode)
    out["grads"] = _grads(sd)
    return _frozen(out)


GAP_SCALE = -0.5          # gradient reversal folds in as gap_scale = -lambda (train_dann.py:29)
