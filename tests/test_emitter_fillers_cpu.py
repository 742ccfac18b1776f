"""The fillers of ops.py that engine.StepPlan.maxpool / convT / convT_head / conv1x1 / gap / linear call leave in a program op, byte for byte,
what those emitters wrote field by field before they called the fillers (their base() / head() closures and per-kind patches, restated here
once).  CPU tensors, host only: nothing is launched.  Workspaces are left out on both sides: the engine points them at the shared arena
afterwards (StepPlan.finalize)."""
import ctypes as C
import itertools

import pytest
import torch

from multi_task_breast_cancer_amd import ops

L = ops.L
N, PLANAR, C8 = 2, L.LAYOUT_PLANAR, L.LAYOUT_C8


def _t(numel=8, dtype=torch.float32):
    return torch.empty(numel, dtype=dtype)


def _op(kind, member):
    op = L.Op()
    op.kind = kind
    return op, getattr(op.u, member)


def _same(got, want, what):
    assert isinstance(got, L.Op) and got.kind == want.kind and got.tag == 0 and bytes(got) == bytes(want), what


# ------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("c8,half,fold,acc", [(False, False, False, 0), (False, True, False, 1), (True, False, False, 0), (True, False, True, 0),
                                             (True, True, True, 1), (True, True, False, 1)])
def test_maxpool(c8, half, fold, acc):
    """half: x and y are the second halves of batch-concatenated (2N-image) tensors -- dense strides, addresses inside the parents' buffers; an
    odd plane (10 x 6 pooled to 5 x 3) where y's stride is not x's over four."""
    Cc, H, W, compute = 16, (8 if c8 else 10), (8 if c8 else 6), 2
    xbs, ybs = Cc * H * W, Cc * (H // 2) * (W // 2)
    dt = torch.int16 if c8 else torch.float32
    xp, yp = _t(2 * N * xbs, dt), _t(2 * N * ybs, dt)
    x, y = (xp[N * xbs:], yp[N * ybs:]) if half else (xp[:N * xbs], yp[:N * ybs])
    arg, dy, dx = _t(N * ybs // 8, torch.int16), _t(N * ybs), _t(N * xbs)

    def base(kind):
        op, a = _op(kind, "pool")
        a.N, a.C, a.H, a.W = N, Cc, H, W
        if c8:
            a.layout, a.type16 = C8, compute
        a.x, a.x_batch_stride = x.data_ptr(), xbs
        a.y, a.y_batch_stride = y.data_ptr(), ybs
        return op, a

    mode = dict(compute=compute if c8 else 0, strides=dict(x=xbs, y=ybs, dy=ybs, dx=xbs))
    ptrs = dict(x=x, y=y, argmax=arg if fold else None) if c8 else dict(x=x, y=y)
    want, a = base(L.OP_POOL_FWD)
    if fold:
        a.argmax = arg.data_ptr()
    _same(ops.maxpool_case_args(L.OP_POOL_FWD, N, Cc, H, W, ptrs=ptrs, argmax=fold, **mode), want, "fwd")
    want, a = base(L.OP_POOL_BWD)
    a.dy, a.dy_batch_stride = dy.data_ptr(), ybs
    a.dx, a.dx_batch_stride, a.accumulate_dx = dx.data_ptr(), xbs, acc
    _same(ops.maxpool_case_args(L.OP_POOL_BWD, N, Cc, H, W, ptrs=dict(ptrs, dy=dy, dx=dx), acc_dx=bool(acc), **mode), want, "bwd")


# ------------------------------------------------------------------ transposed convolution
def _convT_base(kind, shape, x, xbs, w, bias, y, ybs):
    op, a = _op(kind, "convT")
    a.N, a.Cin, a.Cout, a.H, a.W, a.k = shape
    a.x, a.x_batch_stride = x.data_ptr(), xbs
    a.w = w.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.y, a.y_batch_stride = y.data_ptr(), ybs
    return op, a


@pytest.mark.parametrize("fwd,with_bias", itertools.product(("planar", "y_c8", "x_c8"), (True, False)))
def test_convT_forward(fwd, with_bias):
    compute, shape = 1, (N, 48, 24, 8, 8, 2)
    x, x8, w, bias, y, y8 = _t(), _t(8, torch.int16), _t(), (_t() if with_bias else None), _t(), _t(8, torch.int16)
    xbs, ybs = 48 * 64, 24 * 256
    want, a = _convT_base(L.OP_CONVT_FWD, shape, x, xbs, w, bias, y, ybs)
    ptrs, mode = dict(x=x, w=w, bias=bias, y=y), {}
    if fwd != "planar":
        a.y, a.y_layout, a.y_type = y8.data_ptr(), C8, compute
        ptrs, mode = dict(ptrs, y=y8), dict(compute=compute, y_c8=True)
    if fwd == "x_c8":
        a.x, a.x_layout = x8.data_ptr(), C8
        ptrs, mode = dict(ptrs, x=x8), dict(mode, x_c8=True)
    _same(ops.convT_case_op(L.OP_CONVT_FWD, *shape, ptrs=ptrs, strides=dict(x=xbs, y=ybs, dy=ybs, dx=xbs), **mode), want, fwd)


@pytest.mark.parametrize("lp,g16,with_bias,acc_dw,acc_dx", [(0, False, True, 0, 0), (1, False, True, 1, 1), (1, True, True, 0, 0), (2, True, False, 1, 1),
                                                           (2, False, False, 0, 1)])
def test_convT_backward(lp, g16, with_bias, acc_dw, acc_dx):
    """Both gradient ops carry x, w, bias and y (the planar ones, whatever the forward read); lp = the MFMA operand type, g16 = dy as 16-bit
    planes of that type.  x as 16-bit planes is a patch behind the emission (StepPlan._narrow_activations): the filler's x16 writes what
    that patch leaves."""
    shape = (N, 48, 24, 8, 8, 2)
    x, w, bias, y, dw, dx, x16 = _t(), _t(), (_t() if with_bias else None), _t(), _t(), _t(), _t(8, torch.int16)
    dbias = _t() if with_bias else None
    dy = _t(8, torch.int16 if g16 else torch.float32)
    xbs, ybs = 48 * 64, 24 * 256
    strides = dict(x=xbs, y=ybs, dy=ybs, dx=xbs)
    grads = dict(x=x, w=w, bias=bias, y=y, dy=dy, dw=dw, dbias=dbias)
    mode = dict(compute=lp, dy16=g16, strides=strides)

    def wgrad():
        op, a = _convT_base(L.OP_CONVT_WGRAD, shape, x, xbs, w, bias, y, ybs)
        a.compute = lp
        a.dy, a.dy_batch_stride, a.dy_type16 = dy.data_ptr(), ybs, (lp if g16 else 0)
        a.accumulate_dw = acc_dw
        a.dw = dw.data_ptr()
        if with_bias:
            a.dbias = dbias.data_ptr()
        return op, a

    want, a = wgrad()
    _same(ops.convT_case_op(L.OP_CONVT_WGRAD, *shape, ptrs=grads, acc_dw=bool(acc_dw), workspace=False, **mode), want, "wgrad")
    if g16:
        want, a = wgrad()
        a.x, a.x_type16 = x16.data_ptr(), lp
        _same(ops.convT_case_op(L.OP_CONVT_WGRAD, *shape, ptrs=dict(grads, x=x16), acc_dw=bool(acc_dw), x16=True, workspace=False, **mode), want, "wgrad x16")
    want, a = _convT_base(L.OP_CONVT_DGRAD, shape, x, xbs, w, bias, y, ybs)
    a.compute = lp
    a.dy, a.dy_batch_stride, a.dy_type16 = dy.data_ptr(), ybs, (lp if g16 else 0)
    a.dx, a.dx_batch_stride, a.accumulate_dx = dx.data_ptr(), xbs, acc_dx
    _same(ops.convT_case_op(L.OP_CONVT_DGRAD, *shape, ptrs=dict(grads, dx=dx), acc_dx=bool(acc_dx), **mode), want, "dgrad")


def test_convT_gradients_without_the_carried_pointers_are_as_before():
    """A caller that hands in only what the call reads gets the struct it got before the fillers carried anything."""
    shape, w, dy, dx, x, dw = (N, 48, 24, 8, 8, 2), _t(), _t(), _t(), _t(), _t()
    a = ops.convT_case_args(L.OP_CONVT_DGRAD, *shape, ptrs={"w": w, "dy": dy, "dx": dx})
    assert (a.x, a.bias, a.y) == (None, None, None)
    a = ops.convT_case_args(L.OP_CONVT_WGRAD, *shape, ptrs={"x": x, "w": w, "dy": dy, "dw": dw, "dbias": None}, workspace=False)
    assert (a.bias, a.y) == (None, None) and a.x == x.data_ptr()
    op = ops.conv1x1_case_args(L.OP_CONV1_DGRAD, N, 24, 1, 8, 8, ptrs={"x": x, "w": w, "dy": dy, "dx": dx})
    assert (op.u.conv1.bias, op.u.conv1.y) == (None, None)
    for kind in (L.OP_CONVT_DGRAD, L.OP_CONVT_WGRAD):          # the dummies of the kernel-name queries carry nothing either
        a = ops.convT_case_args(kind, *shape)
        assert (a.bias, a.y) == (None, None) and (kind == L.OP_CONVT_WGRAD or a.x is None)


# ------------------------------------------------------------------ the fused ConvT + 1x1 head pair
@pytest.mark.parametrize("acc,acc_dx", [((0, 0, 0, 0), 0), ((1, 1, 0, 1), 1)])
def test_convT_head_pair(acc, acc_dx):
    Cin, cmid, R, k, H, W = 48, 24, 1, 2, 8, 8
    wT, bT, w1, b1, Wc, bc, G, gb, dwT, dbT, dw1, db1, x, y, dy, dx = (_t() for _ in range(16))
    xbs, ybs = Cin * H * W, R * H * k * W * k

    def head(kind):
        op, a = _op(kind, "head")
        a.Cin, a.Cmid, a.R, a.k = Cin, cmid, R, k
        a.wT, a.bT, a.w1, a.b1 = wT.data_ptr(), bT.data_ptr(), w1.data_ptr(), b1.data_ptr()
        a.Wc, a.bc, a.G, a.gb = Wc.data_ptr(), bc.data_ptr(), G.data_ptr(), gb.data_ptr()
        return op, a

    shape, strides = (N, Cin, R, H, W, k), dict(x=xbs, y=ybs, dy=ybs, dx=xbs)
    fuse = dict(wT=wT, bT=bT, w1=w1, b1=b1, Wc=Wc, bc=bc, G=G, gb=gb)
    ptrs = dict(x=x, w=Wc, bias=bc, y=y)
    grads = dict(ptrs, dy=dy, dw=G, dbias=gb)
    _same(ops.head_case_args(L.OP_HEAD_COMBINE, Cin, cmid, R, k, ptrs=fuse), head(L.OP_HEAD_COMBINE)[0], "combine")
    _same(ops.convT_case_op(L.OP_CONVT_FWD, *shape, ptrs=ptrs, strides=strides), _convT_base(L.OP_CONVT_FWD, shape, x, xbs, Wc, bc, y, ybs)[0], "fwd")
    want, a = _convT_base(L.OP_CONVT_WGRAD, shape, x, xbs, Wc, bc, y, ybs)
    a.dy, a.dy_batch_stride = dy.data_ptr(), ybs
    a.dw, a.dbias, a.accumulate_dw = G.data_ptr(), gb.data_ptr(), 0
    _same(ops.convT_case_op(L.OP_CONVT_WGRAD, *shape, ptrs=grads, strides=strides, workspace=False), want, "wgrad")
    want, a = head(L.OP_HEAD_EXPAND)
    a.acc_wT, a.acc_bT, a.acc_w1, a.acc_b1 = acc
    a.dwT, a.dbT, a.dw1, a.db1 = dwT.data_ptr(), dbT.data_ptr(), dw1.data_ptr(), db1.data_ptr()
    _same(ops.head_case_args(L.OP_HEAD_EXPAND, Cin, cmid, R, k, ptrs=dict(fuse, dwT=dwT, dbT=dbT, dw1=dw1, db1=db1), acc=list(acc)), want, "expand")
    want, a = _convT_base(L.OP_CONVT_DGRAD, shape, x, xbs, Wc, bc, y, ybs)
    a.dy, a.dy_batch_stride = dy.data_ptr(), ybs
    a.dx, a.dx_batch_stride, a.accumulate_dx = dx.data_ptr(), xbs, acc_dx
    _same(ops.convT_case_op(L.OP_CONVT_DGRAD, *shape, ptrs=dict(grads, dx=dx), strides=strides, acc_dx=bool(acc_dx)), want, "dgrad")


# ------------------------------------------------------------------ 1x1 convolution
@pytest.mark.parametrize("c8,cout,acc_dw,acc_dx", [(False, 3, 0, 0), (False, 1, 1, 1), (True, 1, 0, 1), (True, 4, 1, 0)])
def test_conv1x1(c8, cout, acc_dw, acc_dx):
    Cin, H, W, compute = 24, 8, 8, 1
    x, w, bias, y, dy, dx, dw, dbias = _t(8, torch.int16 if c8 else torch.float32), _t(), _t(), _t(), _t(), _t(), _t(), _t()
    xbs = Cin * H * W

    def base(kind):
        op, a = _op(kind, "conv1")
        a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, cout
        if c8:
            a.x, a.x_batch_stride, a.x_layout, a.x_type = x.data_ptr(), xbs, C8, compute
        else:
            a.x, a.x_batch_stride = x.data_ptr(), xbs
        a.w, a.bias, a.y = w.data_ptr(), bias.data_ptr(), y.data_ptr()
        return op, a

    shape, mode = (N, Cin, cout, H, W), dict(compute=compute if c8 else 0, strides=dict(x=xbs, dx=xbs))
    ptrs = dict(x=x, w=w, bias=bias, y=y)
    grads = dict(ptrs, dy=dy, dw=dw, dbias=dbias)
    _same(ops.conv1x1_case_args(L.OP_CONV1_FWD, *shape, ptrs=ptrs, **mode), base(L.OP_CONV1_FWD)[0], "fwd")
    want, a = base(L.OP_CONV1_WGRAD)
    a.dy, a.accumulate_dw = dy.data_ptr(), acc_dw
    a.dw, a.dbias = dw.data_ptr(), dbias.data_ptr()
    _same(ops.conv1x1_case_args(L.OP_CONV1_WGRAD, *shape, ptrs=grads, acc_dw=bool(acc_dw), workspace=False, **mode), want, "wgrad")
    want, a = base(L.OP_CONV1_DGRAD)
    a.dy = dy.data_ptr()
    a.dx, a.dx_batch_stride, a.accumulate_dx = dx.data_ptr(), xbs, acc_dx
    _same(ops.conv1x1_case_args(L.OP_CONV1_DGRAD, *shape, ptrs=dict(grads, dx=dx), acc_dx=bool(acc_dx), **mode), want, "dgrad")


# ------------------------------------------------------------------ global average pool, Linear
def test_gap():
    Cc, H, W = 24, 4, 4
    x, y, dy, dx = _t(), _t(), _t(), _t()

    def base(kind):
        op, a = _op(kind, "gap")
        a.N, a.C, a.H, a.W = N, Cc, H, W
        a.x, a.y = x.data_ptr(), y.data_ptr()
        return op, a

    _same(ops.gap_case_args(L.OP_GAP_FWD, N, Cc, H, W, ptrs=dict(x=x, y=y)), base(L.OP_GAP_FWD)[0], "fwd")
    want, a = base(L.OP_GAP_BWD)
    a.dy, a.dx = dy.data_ptr(), dx.data_ptr()
    _same(ops.gap_case_args(L.OP_GAP_BWD, N, Cc, H, W, ptrs=dict(x=x, y=y, dy=dy, dx=dx)), want, "bwd")


@pytest.mark.parametrize("relu,in_f,needs_dx,acc_dw", [(True, 96, True, 0), (False, 96, True, 1), (True, 8192, False, 0), (False, 8192, True, 0)])
def test_linear(relu, in_f, needs_dx, acc_dw):
    """in_f = 8192: a wide input (from L.LINEAR_WIDE_MIN_IN on the library asks for a workspace; the engine queries it on the filled struct)."""
    out_f = 16
    x, w, bias, y, dy, dx, dw, dbias = (_t() for _ in range(8))

    def base(kind):
        op, a = _op(kind, "linear")
        a.N, a.In, a.Out, a.relu = N, in_f, out_f, 1 if relu else 0
        a.x, a.w, a.bias, a.y = x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr()
        return op, a

    ptrs = dict(x=x, w=w, bias=bias, y=y)
    got = ops.linear_case_args(L.OP_LINEAR_FWD, N, in_f, out_f, ptrs=ptrs, relu=relu, workspace=False)
    _same(got, base(L.OP_LINEAR_FWD)[0], "fwd")
    want, a = base(L.OP_LINEAR_BWD)
    a.dy = dy.data_ptr()
    a.dx = dx.data_ptr() if needs_dx else None
    a.accumulate_dw = acc_dw
    a.dw, a.dbias = dw.data_ptr(), dbias.data_ptr()
    got = ops.linear_case_args(L.OP_LINEAR_BWD, N, in_f, out_f, ptrs=dict(ptrs, dy=dy, dx=dx if needs_dx else None, dw=dw, dbias=dbias), relu=relu,
                               acc_dw=bool(acc_dw), workspace=False)
    _same(got, want, "bwd")
    lib = L.load()
    assert int(lib.mtbc_linear_workspace(C.byref(got.u.linear), 1)) == int(lib.mtbc_linear_workspace(C.byref(want.u.linear), 1))
    assert C.sizeof(L.Op) == len(bytes(got))
