"""The decoder's up step per operator, through mi3d_up_forward / mi3d_up_backward / mi3d_nearest_resize_*: the entries run the function
pair the whole-network plan calls (up_half_forward / up_half_backward), so the temporary + resize, the MFMA or direct launcher and
the slab-sum slots are the plan's.

Every run asserts the route the entry reports against tests/up_ref.py (the table under the default switches, the Python
predicates otherwise), then the values:
  dyadic data     y and dx bits = bf16_rne(exact), dW and db equal to the float64 values (plus a dyadic prefill with accumulate = 1);
                  fp32 outputs of the direct kernels equal to the float64 values.  tests/test_up_ref_cpu.py asserts the exactness
                  condition per case
  argument forms  db NULL, dx only, weights only, the stand-alone pair: dx bit for bit the fused launch's, dW / db exact
  pending sums    left pending and launched alone / carried by a BatchNorm-backward reduction / written to the second slab region:
                  bit for bit the immediate sum
  normal data     within half a bf16 spacing plus conv_bwd_ref.acc_bound of the float64 result
  resize          forward, adjoint and sum(gx) == sum(gy) against torch on the CPU, on integer data

Concat buffers, padding channels, outputs and workspaces hold a non-zero sentinel pattern before every call; what a call must not
write is compared bit for bit afterwards."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multimodal_segmentation_project_amd as mi  # noqa: F401,E402
from multimodal_segmentation_project_amd import _lib  # noqa: E402
from multimodal_segmentation_project_amd._lib import call, ptr  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bwd_ref as B  # noqa: E402
import conv_ref as R  # noqa: E402
import up_ref as U  # noqa: E402
from test_gpu_bn_ops import within  # noqa: E402
from test_gpu_conv_bwd_ops import run as conv_bn_run  # noqa: E402

DEV = "cuda:0"
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A          # bf16 1.5e16 / fp32 1.5e16: finite, so a kernel that reads one shows it in the values


def tdt_of(dt):
    return torch.bfloat16 if dt == 1 else torch.float32


def sentinel(shape, tdt):
    t = torch.empty(shape, device=DEV, dtype=tdt)
    if tdt == torch.bfloat16:
        t.view(torch.int16).fill_(SENT16)
    else:
        t.view(torch.int32).fill_(SENT32)
    return t


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def is_sentinel(t):
    return bool((bits(t) == (SENT16 if t.dtype == torch.bfloat16 else SENT32)).all())


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (what, int((bits(a) != bits(b)).sum()))


def cl_into(a, tdt, cs=None, off=0):
    """NCDHW array -> channels [off, off + C) of a channels-last sentinel buffer of channel stride cs; (buffer, view)"""
    a = np.asarray(a, np.float32)
    c = a.shape[1]
    buf = sentinel(a.shape[:1] + a.shape[2:] + (cs or c,), tdt)
    view = buf[..., off:off + c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 4, 1))).to(DEV).to(tdt))
    return buf, view


def ncdhw(t):
    return t.float().cpu().numpy().transpose(0, 4, 1, 2, 3).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, copy=True)).to(DEV)


def workspace(k):
    n, d, h, w = k["geo"]
    nb = _lib.lib().mi3d_up_workspace_bytes(k["dtype"], k["cin"], k["cout"], n, d, h, w)
    assert nb > 0
    return torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)


def region(k, which):
    n, d, h, w = k["geo"]
    nbytes = C.c_size_t()
    off = _lib.lib().mi3d_up_workspace_region(k["dtype"], k["cin"], k["cout"], n, d, h, w, which, C.byref(nbytes))
    return off, nbytes.value


LAYOUTS = {"cat": (2, 1), "planar": (1, 0), "unaligned": None}


def forward(k, layout="cat", xpad=0, go=None, x=None, w=None, b=None):
    """one mi3d_up_forward; layout: cat = the upper half of an interleaved buffer (ucs = 2 Cout), planar = a buffer of its own
    (ucs = Cout), unaligned = 4 channels into a buffer of Cout + 8.  Returns the up half, the route and the untouched rest."""
    n, d, h, wd = k["geo"]
    cin, cout, tdt = k["cin"], k["cout"], tdt_of(k["dtype"])
    go = go or (2 * d, 2 * h, 2 * wd)
    xbuf, _ = cl_into(k["x"] if x is None else x, tdt, cin + xpad)
    ucs, off = (cout + 8, 4) if layout == "unaligned" else (LAYOUTS[layout][0] * cout, LAYOUTS[layout][1] * cout)
    buf = sentinel((n,) + tuple(go) + (ucs,), tdt)
    wgt, bias, ws, route = dev(k["w"] if w is None else w), dev(k["b"] if b is None else b), workspace(k), _lib.UpRoute()
    call("mi3d_up_forward", k["dtype"], ptr(xbuf), cin + xpad, cin, ptr(wgt), ptr(bias), buf.data_ptr() + off * buf.element_size(), ucs,
         cout, n, d, h, wd, go[0], go[1], go[2], C.byref(route), ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    rest = torch.cat([buf[..., :off], buf[..., off + cout:]], dim=-1)
    assert is_sentinel(rest), (k["name"], layout, "the call wrote outside its half")
    if xpad:
        assert is_sentinel(xbuf[..., cin:])
    return dict(y=buf[..., off:off + cout], route={q: getattr(route, q) for q in U.FWD_KEYS})


def backward(k, flags=0, accumulate=0, dx=True, dw=True, db=True, go=None, gy=None, x=None, w=None, xpad=0):
    """one mi3d_up_backward on the upper half of an interleaved gradient buffer whose other half holds the sentinel"""
    n, d, h, wd = k["geo"]
    cin, cout, tdt = k["cin"], k["cout"], tdt_of(k["dtype"])
    xbuf, _ = cl_into(k["x"] if x is None else x, tdt, cin + xpad)
    gbuf, _ = cl_into(k["gy"] if gy is None else gy, tdt, 2 * cout, cout)
    go = go or (2 * d, 2 * h, 2 * wd)
    wgt, ws, route, pend = dev(k["w"] if w is None else w), workspace(k), _lib.UpRoute(), _lib.PendingSum()
    dxb = sentinel((n, d, h, wd, cin + xpad), tdt) if dx else None
    if accumulate:
        dW, dbt = dev(k["dw0"]), dev(k["db0"])
    else:
        dW, dbt = sentinel(k["w"].shape, torch.float32), sentinel((cout,), torch.float32)
    call("mi3d_up_backward", k["dtype"], ptr(xbuf), cin + xpad, cin, ptr(wgt), gbuf.data_ptr() + cout * gbuf.element_size(), 2 * cout, cout,
         ptr(dxb), cin + xpad, ptr(dW) if dw else None, ptr(dbt) if db else None, accumulate, n, d, h, wd, go[0], go[1], go[2], flags,
         C.byref(pend), C.byref(route), ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    if dx and xpad:
        assert is_sentinel(dxb[..., cin:])
    return dict(dx=dxb[..., :cin] if dx else None, dW=dW, db=dbt, ws=ws, pend=pend, keep=(xbuf, gbuf, wgt),
                route={q: getattr(route, q) for q in U.BWD_KEYS})


def check_y(k, o, exact=None):
    exact = k["y"] if exact is None else exact
    if k["dtype"] == 1:
        R.assert_bf16_rne_bits(o["y"], exact, (k["name"], "y"))
    else:
        assert (ncdhw(o["y"]) == exact).all(), (k["name"], "y")


def check_grads(k, o, pre=False, dx=True, dw=True, db=True, ref=None):
    rdx, rdW, rdb = ref or (k["dx"], k["dW"], k["db"])
    if dw:
        want = rdW + (k["dw0"].astype(np.float64) if pre else 0.0)
        got = o["dW"].cpu().numpy().astype(np.float64)
        assert (got == want).all(), (k["name"], "dW", int((got != want).sum()), float(np.abs(got - want).max()))
    else:
        assert pre or is_sentinel(o["dW"])
    if db:
        want = rdb + (k["db0"].astype(np.float64) if pre else 0.0)
        got = o["db"].cpu().numpy().astype(np.float64)
        assert (got == want).all(), (k["name"], "db", int((got != want).sum()), float(np.abs(got - want).max()))
    else:
        assert pre or is_sentinel(o["db"])
    if dx:
        if k["dtype"] == 1:
            R.assert_bf16_rne_bits(o["dx"], rdx, (k["name"], "dx"))
        else:
            assert (ncdhw(o["dx"]) == rdx).all(), (k["name"], "dx")


MFMA_FWD = [n for n in U.CASES if n != "stride_hoist"]


# ---------------------------------------------------------------------------------------------- MFMA forward
@pytest.mark.parametrize("layout", ["cat", "planar"])
@pytest.mark.parametrize("name", MFMA_FWD)
def test_mfma_forward_route_and_bits(name, layout):
    k = U.case_data(name)
    o = forward(k, layout)
    want = k["fwd"] if layout == "cat" else U.fwd_route(1, k["cin"], k["cout"], k["geo"], ucs=k["cout"])
    assert o["route"] == want, (name, o["route"], want)
    assert want["kind"] == 1 and want["wide"] == k["fwd"]["wide"]
    check_y(k, o)


@pytest.mark.parametrize("name", ["hoist_wide", "wide_ks2", "tapsplit_ksp8"])
def test_mfma_forward_input_stride_wider_than_cin(name):
    k = U.case_data(name)
    o = forward(k, xpad=8)
    assert o["route"] == k["fwd"]
    check_y(k, o)


def test_mfma_forward_up_half_not_16_byte_aligned():
    """y four channels into a wider buffer: all 8 taps in one workgroup with 8-byte stores, the same bits"""
    k = U.case_data("wide_ks2")
    o = forward(k, "unaligned")
    want = U.fwd_route(1, k["cin"], k["cout"], k["geo"], ucs=k["cout"] + 8, aligned=False)
    assert o["route"] == want and (want["wide"], want["tap_split"]) == (0, 0), (o["route"], want)
    check_y(k, o)
    same_bits(o["y"], forward(k)["y"], "narrow against wide stores")


def test_mfma_forward_grid_stride_loop():
    """(1, 32, 16, 65, 64, 64): 16640 voxel groups on 4096 x 4 waves, wide + hoist into a planar half.  The reference is one fp32
    matmul, exact under the dyadic condition (test_up_ref_cpu.py), rounded by torch's CPU conversion (= bf16_rne,
    test_conv_ref_cpu.py)"""
    k = U.case_data("stride_hoist", need_ref=False)
    o = forward(k, "planar")
    want = U.fwd_route(1, k["cin"], k["cout"], k["geo"], ucs=k["cout"])
    assert o["route"] == want == dict(k["fwd"]), (o["route"], want)
    n, d, h, w = k["geo"]
    cin, cout = k["cin"], k["cout"]
    xm = torch.from_numpy(np.ascontiguousarray(k["x"].transpose(0, 2, 3, 4, 1))).reshape(-1, cin)
    acc = xm @ torch.from_numpy(k["w"].reshape(cin, cout * 8).copy())                                  # [M][(co, a, b, c)] fp32, exact
    acc = acc.reshape(n, d, h, w, cout, 2, 2, 2) + torch.from_numpy(k["b"].copy()).reshape(1, 1, 1, 1, cout, 1, 1, 1)
    ref = acc.permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(n, 2 * d, 2 * h, 2 * w, cout).to(torch.bfloat16)
    got = o["y"].contiguous().cpu()
    assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16)), int((got.view(torch.int16) != ref.view(torch.int16)).sum())


# ---------------------------------------------------------------------------------------------- MFMA backward
@pytest.mark.parametrize("name", U.BWD_CASES)
def test_mfma_backward_route_and_exact_gradients(name):
    k = U.case_data(name)
    o = backward(k)
    assert o["route"] == k["bwd"], (name, o["route"], k["bwd"])
    check_grads(k, o)
    a = backward(k, accumulate=1)
    assert a["route"] == k["bwd"]
    check_grads(k, a, pre=True)


@pytest.mark.parametrize("name", ["hoist_wide", "wide_ks2"])
def test_mfma_backward_strides_wider_than_cin(name):
    k = U.case_data(name)
    o = backward(k, xpad=8)
    assert o["route"] == k["bwd"]
    check_grads(k, o)


@pytest.mark.parametrize("name", U.BWD_CASES)
def test_mfma_backward_argument_forms(routes, name):
    """db NULL; dx only (kind 3); weights only (kind 4); the stand-alone pair (kind 2): against the fused launch on the same data
    dx is bit-identical, dW / db exact"""
    k = U.case_data(name)
    g, dt = k["geo"], 1
    fused = backward(k)
    pr = lambda **kw: U.bwd_route(dt, k["cin"], k["cout"], g, **kw)  # noqa: E731
    o = backward(k, db=False)
    assert o["route"] == k["bwd"]
    check_grads(k, o, db=False)
    same_bits(o["dx"], fused["dx"], "dx without db")
    o = backward(k, dw=False, db=False)
    assert o["route"] == pr(dw=False) and o["route"]["kind"] == 3, o["route"]
    check_grads(k, o, dw=False, db=False)
    same_bits(o["dx"], fused["dx"], "dx alone")
    o = backward(k, dx=False)
    assert o["route"] == pr(dx=False) and o["route"]["kind"] == 4, o["route"]
    check_grads(k, o, dx=False)
    o = backward(k, dx=False, db=False)
    assert o["route"]["kind"] == 4
    check_grads(k, o, dx=False, db=False)
    routes.set("no_fused_upbwd", 1)
    o = backward(k)
    assert o["route"] == pr(routes={"no_fused_upbwd": 1}) and o["route"]["kind"] == 2, o["route"]
    check_grads(k, o)
    same_bits(o["dx"], fused["dx"], "dx of the stand-alone pair")
    a = backward(k, accumulate=1)
    check_grads(k, a, pre=True)


# ---------------------------------------------------------------------------------------------- pending sums
def pending_runs(k, **data):
    """the immediate sum, the sum left pending and launched alone, the sum carried by a BatchNorm-backward reduction, and both with
    the slabs in the second region"""
    now = backward(k, **data)
    alone = backward(k, flags=U.LEAVE_PENDING, **data)
    assert alone["route"] == dict(now["route"], pending=1), alone["route"]
    assert is_sentinel(alone["dW"]) and is_sentinel(alone["db"])                    # nothing summed yet
    same_bits(alone["dx"], now["dx"], "dx")
    call("mi3d_pending_sum_launch", C.byref(alone["pend"]), None)
    torch.cuda.synchronize()
    rider = backward(k, flags=U.LEAVE_PENDING, **data)
    kb = B.case_data("pair_48_16")
    ob = conv_bn_run(kb, bn=True, riders=[rider["pend"], _lib.PendingSum()])
    assert ob["route"]["riders"] == 1
    ref = conv_bn_run(kb, bn=True)
    for q in ("dy", "dx", "dW", "db", "dgamma", "dbeta"):
        same_bits(ob[q], ref[q], ("carrier", q))
    off, nbytes = region(k, 2)
    second = backward(k, flags=U.SECOND_WORKSPACE, **data)
    assert bool((second["ws"][off:off + nbytes] == 0xA5).all()), "the first slab region was written"
    assert second["route"] == now["route"]
    second_left = backward(k, flags=U.SECOND_WORKSPACE | U.LEAVE_PENDING, **data)
    assert second_left["route"]["pending"] == 1 and is_sentinel(second_left["dW"])
    assert bool((second_left["ws"][off:off + nbytes] == 0xA5).all())
    call("mi3d_pending_sum_launch", C.byref(second_left["pend"]), None)
    torch.cuda.synchronize()
    off2, nb2 = region(k, 3)
    assert bool((now["ws"][off2:off2 + nb2] == 0xA5).all()), "the second slab region was written without the flag"
    for q in ("dW", "db"):
        same_bits(alone[q], rider[q], (q, "launched alone against carried"))
        same_bits(alone[q], now[q], (q, "pending against immediate"))
        same_bits(second[q], now[q], (q, "second region"))
        same_bits(second_left[q], now[q], (q, "second region, pending"))
    same_bits(second["dx"], now["dx"], "dx, second region")
    return now, alone, rider


@pytest.mark.parametrize("name", U.BWD_CASES)
def test_pending_sum_launched_alone_carried_and_in_the_second_region(name):
    k = U.case_data(name)
    now, alone, rider = pending_runs(k)
    for o in (now, alone, rider):
        check_grads(k, o)


# ---------------------------------------------------------------------------------------------- normal data
def normal_data(name):
    c = U.CASES[name]
    n, d, h, w = c["geo"]
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    rn = lambda *s: R.bf16_rne(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    return dict(x=rn(n, c["cin"], d, h, w), w=rn(c["cin"], c["cout"], 2, 2, 2), b=rn(c["cout"]), gy=rn(n, c["cout"], 2 * d, 2 * h, 2 * w))


@pytest.mark.parametrize("name", U.NORMAL_CASES)
def test_normal_data_within_the_accumulation_bound(name):
    """seeded standard-normal inputs rounded to bf16: y and dx within half a bf16 spacing plus acc_bound(terms, sum|terms|) of the
    float64 result (Cin + 1 terms for y, 8 Cout for dx), dW and db within acc_bound (M and 8 M terms); the pending sums bit for bit"""
    k, q = U.case_data(name), normal_data(name)
    n, d, h, w = k["geo"]
    m, cin, cout = n * d * h * w, k["cin"], k["cout"]
    ax, aw, ab, ag = (np.abs(q[s]).astype(np.float64) for s in ("x", "w", "b", "gy"))
    o = forward(k, x=q["x"], w=q["w"], b=q["b"])
    assert o["route"] == k["fwd"]
    ref = U.convT2_f64(q["x"], q["w"], q["b"])
    by = B.acc_bound(cin + 1, U.convT2_f64(ax, aw, ab))
    within(ncdhw(o["y"]), ref, by + B.half_spacing(np.abs(ref) + by), (name, "y"))
    now, _, _ = pending_runs(k, x=q["x"], w=q["w"], gy=q["gy"])
    assert now["route"] == k["bwd"]
    rdx, rdW, rdb = U.convT2_bwd_f64(q["x"], q["w"], q["gy"])
    sdx, sdW, sdb = U.convT2_bwd_f64(ax, aw, ag)
    bx = B.acc_bound(8 * cout, sdx)
    within(ncdhw(now["dx"]), rdx, bx + B.half_spacing(np.abs(rdx) + bx), (name, "dx"))
    within(now["dW"].cpu().numpy(), rdW, B.acc_bound(m, sdW), (name, "dW"))
    within(now["db"].cpu().numpy(), rdb, B.acc_bound(8 * m, sdb), (name, "db"))


# ---------------------------------------------------------------------------------------------- direct kernels
@pytest.mark.parametrize("name", list(U.DIRECT_CASES))
def test_direct_kernels_route_and_exact_values(name):
    k = U.case_data(name)
    for layout in ("cat", "planar"):
        o = forward(k, layout)
        assert o["route"] == k["fwd"] and o["route"]["kind"] == 0, (name, o["route"])
        check_y(k, o)
    o = backward(k)
    assert o["route"] == k["bwd"] and o["route"]["kind"] == 0, (name, o["route"], k["bwd"])
    check_grads(k, o)
    a = backward(k, accumulate=1)
    check_grads(k, a, pre=True)
    o = backward(k, dx=False)
    assert o["route"] == U.bwd_route(k["dtype"], k["cin"], k["cout"], k["geo"], dx=False)
    check_grads(k, o, dx=False)


def test_direct_forward_input_not_16_byte_aligned():
    """fp32, Cin = 8, x one element into its allocation: the scalar-load forward kernel (CIC = 1) and the scalar-store input gradient"""
    k = U.case_data("f32_tiles")
    n, d, h, w = k["geo"]
    cin, cout = k["cin"], k["cout"]
    flat = sentinel((n * d * h * w * cin + 1,), torch.float32)
    x = flat[1:].view(n, d, h, w, cin)
    x.copy_(torch.from_numpy(np.ascontiguousarray(k["x"].transpose(0, 2, 3, 4, 1))).to(DEV))
    assert x.data_ptr() % 16 == 4
    buf = sentinel((n, 2 * d, 2 * h, 2 * w, 2 * cout), torch.float32)
    wgt, bias, ws, route = dev(k["w"]), dev(k["b"]), workspace(k), _lib.UpRoute()
    call("mi3d_up_forward", 0, ptr(x), cin, cin, ptr(wgt), ptr(bias), buf.data_ptr() + cout * 4, 2 * cout, cout, n, d, h, w, 2 * d, 2 * h,
         2 * w, C.byref(route), ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert route.kind == 0 and is_sentinel(buf[..., :cout]) and is_sentinel(flat[:1])
    assert (ncdhw(buf[..., cout:]) == k["y"]).all()


# ---------------------------------------------------------------------------------------------- nearest resize
def resize_pair(dt, c, n, gi, go, rng, xcs=None, ycs=None, xoff=0, yoff=0):
    """forward and adjoint of one geometry on integer data against torch on the CPU"""
    tdt = tdt_of(dt)
    x = rng.integers(-8, 9, (n, c) + tuple(gi)).astype(np.float32)
    gy = rng.integers(-8, 9, (n, c) + tuple(go)).astype(np.float32)
    xbuf, _ = cl_into(x, tdt, xcs or c, xoff)
    gbuf, _ = cl_into(gy, tdt, ycs or c, yoff)
    ybuf, gxbuf = sentinel((n,) + tuple(go) + (ycs or c,), tdt), sentinel((n,) + tuple(gi) + (xcs or c,), tdt)
    es = xbuf.element_size()
    call("mi3d_nearest_resize_forward", dt, xbuf.data_ptr() + xoff * es, xcs or c, c, n, gi[0], gi[1], gi[2], ybuf.data_ptr() + yoff * es,
         ycs or c, go[0], go[1], go[2], None)
    call("mi3d_nearest_resize_backward", dt, gbuf.data_ptr() + yoff * es, ycs or c, c, n, go[0], go[1], go[2],
         gxbuf.data_ptr() + xoff * es, xcs or c, gi[0], gi[1], gi[2], None)
    torch.cuda.synchronize()
    what = (dt, c, gi, go)
    y, gx = ncdhw(ybuf[..., yoff:yoff + c]), ncdhw(gxbuf[..., xoff:xoff + c])
    assert (y == U.nearest_f64(x, go)).all(), (what, "forward")
    want = U.nearest_bwd_f64(gy, gi)
    assert (gx == want).all(), (what, "adjoint", int((gx != want).sum()))
    assert (gx.sum(axis=(0, 2, 3, 4)) == gy.astype(np.float64).sum(axis=(0, 2, 3, 4))).all(), (what, "sum gx != sum gy")
    for buf, off in ((ybuf, yoff), (gxbuf, xoff)):
        assert is_sentinel(torch.cat([buf[..., :off], buf[..., off + c:]], dim=-1)), (what, "wrote outside its channels")


def sweep_outs(n_in):
    return sorted({n_in, n_in + 1, 2 * n_in, 2 * n_in + 1, 3 * n_in + 2, max(1, n_in - 1), (n_in + 1) // 2})


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_resize_per_axis_sweep(axis, dt):
    """in 1..24 against out in {in, in + 1, 2 in, 2 in + 1, 3 in + 2, in - 1, ceil(in / 2)} on one axis, the other two (2, 3) -> (3, 2)
    and back; C = 5 with wider strides on both sides.  Sums of at most 4 * 2 * 2 integers |k| <= 8: exact in bf16"""
    rng = np.random.default_rng(100 + 10 * axis + dt)
    others = [(2, 3), (3, 2)]
    for n_in in range(1, 25):
        for n_out in sweep_outs(n_in):
            gi, go = [0, 0, 0], [0, 0, 0]
            gi[axis], go[axis] = n_in, n_out
            for j, ax in enumerate(a for a in range(3) if a != axis):
                gi[ax], go[ax] = others[j]
            resize_pair(dt, 5, 1, gi, go, rng, xcs=8, ycs=11, xoff=2, yoff=3)


GEO3 = [((8, 6, 4), (9, 7, 5)), ((8, 6, 4), (9, 6, 5)), ((8, 6, 4), (8, 6, 4)), ((5, 3, 7), (12, 8, 16))]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("gi,go", GEO3)
def test_resize_3d_into_and_out_of_a_concat_half(gi, go, dt):
    """N = 2, C = 16: the temporary (stride 16) against the upper half of an interleaved buffer (stride 32), as the plan runs it;
    (5,3,7) -> (12,8,16) sums up to 27 values per voxel"""
    resize_pair(dt, 16, 2, gi, go, np.random.default_rng(sum(gi) + sum(go) + dt), xcs=16, ycs=32, yoff=16)


@pytest.mark.parametrize("dt", [0, 1])
def test_resize_grid_stride(dt):
    """C = 1, more than 2048 * 256 voxels on the side the kernel's grid covers: the forward over (81,81,41) outputs, the adjoint
    over (81,81,41) inputs"""
    rng = np.random.default_rng(81 + dt)
    assert 2 * 81 * 81 * 41 > 2048 * 256
    resize_pair(dt, 1, 2, (40, 40, 20), (81, 81, 41), rng)
    resize_pair(dt, 1, 2, (81, 81, 41), (40, 40, 20), rng)


@pytest.mark.parametrize("name", list(U.RESIZED_CASES))
def test_up_step_through_the_resize(name):
    """the transposed conv into the temporary, nearest resize into the concat half, and the adjoint: convT2_f64 then nearest_f64"""
    shape, go = U.RESIZED_CASES[name]
    n, cin, cout, d, h, w = shape
    rng = np.random.default_rng(sum(shape) + sum(go))
    x, wgt, b, _, dw0, db0 = U.dyadic_up_inputs(rng, n, cin, cout, d, h, w, big_bias=True)
    gup = rng.integers(-8, 9, (n, cout) + go).astype(np.float32) / 8
    k = dict(name=name, cin=cin, cout=cout, geo=(n, d, h, w), dtype=1, x=x, w=wgt, b=b, gy=gup, dw0=dw0, db0=db0)
    o = forward(k, go=go)
    want = U.fwd_route(1, cin, cout, k["geo"], go)
    assert o["route"] == want and want["resized"] == 1 and want["kind"] == 1, (o["route"], want)
    check_y(k, o, U.up_f64(x, wgt, b, go))
    ref = U.up_bwd_f64(x, wgt, gup)
    m = U.exactness_margins(x, wgt, b, U.nearest_bwd_f64(gup, (2 * d, 2 * h, 2 * w)), dw0, db0)
    assert max(m) < 2.0 ** 24
    for acc in (0, 1):
        ob = backward(k, go=go, accumulate=acc)
        wantb = U.bwd_route(1, cin, cout, k["geo"], go)
        assert ob["route"] == wantb and wantb["resized"] == 1 and wantb["kind"] == 1, (ob["route"], wantb)
        check_grads(k, ob, pre=bool(acc), ref=ref)
