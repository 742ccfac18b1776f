"""The k = 2 ConvT backward as ONE launch (convT2_bwd_fused_kernel, selected by the program runner for an OP_CONVT_WGRAD with the OP_CONVT_DGRAD
of the same up-convolution right behind it): dW, dbias and dx must be BIT-IDENTICAL to the two launches -- the same program run op by
op, and the public mtbc_convT_wgrad / mtbc_convT_dgrad entry points, which keep their kernels.  Shapes are the smallest at which the
decomposition can go wrong (the split plan gives at least 8 steps of 32 pixels per split): several splits, a short last split, splits
that straddle images, two and four blocks of 48 input channels, a ragged block, the odd channel-tile count (CT = 1), the six-wave
workgroup of Cout = 96."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.engine import Program, _mk  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTUNetPlusPlus  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def _g(seed):
    return torch.Generator().manual_seed(1993 + seed)


class Problem:
    """Operands of one up-convolution's backward; strided = every activation tensor is a channel-range view of a wider buffer."""

    def __init__(self, N, Cin, Cout, H, W, compute, strided=False, seed=0):
        g = _g(seed + N + Cin + Cout + H + W + compute)
        self.shape, self.compute = (N, Cin, Cout, H, W), compute
        self.dt = torch.bfloat16 if compute == 1 else torch.float16
        ex, ey = (8, 4) if strided else (0, 0)             # extra channels in front of / behind the view
        self.xbuf = torch.randn(N, Cin + 2 * ex, H, W, generator=g).to(DEV).to(self.dt)
        self.dybuf = torch.randn(N, Cout + 2 * ey, 2 * H, 2 * W, generator=g).to(DEV).to(self.dt)
        self.x16, self.dy16 = self.xbuf[:, ex:ex + Cin], self.dybuf[:, ey:ey + Cout]
        self.w = (torch.randn(Cin, Cout, 2, 2, generator=g) * 0.1).to(DEV)
        self.pre_dx = torch.randn(N, Cin + 2 * ex, H, W, generator=g).to(DEV)
        self.pre_dw = torch.randn(Cin, Cout, 2, 2, generator=g).to(DEV)
        self.pre_db = torch.randn(Cout, generator=g).to(DEV)
        self.ex = ex


class Outputs:
    def __init__(self, pb):
        N, Cin, Cout, H, W = pb.shape
        self.dxbuf = pb.pre_dx.clone()
        self.dx = self.dxbuf[:, pb.ex:pb.ex + Cin]
        self.dw, self.db = pb.pre_dw.clone(), pb.pre_db.clone()


def _wgrad_op(pb, out, acc_dw, bias, keep):
    N, Cin, Cout, H, W = pb.shape
    op = _mk(L.OP_CONVT_WGRAD)
    a = op.u.convT
    a.N, a.H, a.W, a.Cin, a.Cout, a.k = N, H, W, Cin, Cout, 2
    a.x, a.x_batch_stride, a.x_type16 = pb.x16.data_ptr(), pb.xbuf[0].numel(), pb.compute
    a.w = pb.w.data_ptr()
    a.compute = pb.compute
    a.dy, a.dy_batch_stride, a.dy_type16 = pb.dy16.data_ptr(), pb.dybuf[0].numel(), pb.compute
    a.dw, a.accumulate_dw = out.dw.data_ptr(), acc_dw
    if bias:
        a.dbias = out.db.data_ptr()
    nbytes = L.load().mtbc_convT_wgrad_workspace(C.byref(a))
    ws = torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    keep.append(ws)
    return op


def _dgrad_op(pb, out, acc_dx):
    N, Cin, Cout, H, W = pb.shape
    op = _mk(L.OP_CONVT_DGRAD)
    a = op.u.convT
    a.N, a.H, a.W, a.Cin, a.Cout, a.k = N, H, W, Cin, Cout, 2
    a.x, a.x_batch_stride = pb.x16.data_ptr(), pb.xbuf[0].numel()
    a.w = pb.w.data_ptr()
    a.compute = pb.compute
    a.dy, a.dy_batch_stride, a.dy_type16 = pb.dy16.data_ptr(), pb.dybuf[0].numel(), pb.compute
    a.dx, a.dx_batch_stride, a.accumulate_dx = out.dx.data_ptr(), out.dxbuf[0].numel(), acc_dx
    return op


def _pair(pb, acc_dx, acc_dw, bias):
    """[OP_CONVT_WGRAD, OP_CONVT_DGRAD] the way engine.emit_bwd fills them, with outputs of its own."""
    out, keep = Outputs(pb), [pb]
    prog = Program([_wgrad_op(pb, out, acc_dw, bias, keep), _dgrad_op(pb, out, acc_dx)], keep + [out])
    return prog, out


def _same(a, b, bias):
    assert torch.equal(a.dw, b.dw), "dW"
    assert torch.equal(a.dxbuf, b.dxbuf), "dx (and the channels around the view, which nobody may touch)"
    assert torch.equal(a.db, b.db), "dbias"           # without a bias gradient both still hold the pre-fill


CASES = [
    # N, Cin, Cout, H, W, accumulate_dx, accumulate_dw, dbias, strided
    (3, 48, 48, 16, 16, 0, 0, True, False),        # 24 steps -> 3 splits; several reduced partials
    (3, 48, 48, 16, 24, 1, 1, True, False),        # 36 steps -> 5 splits, the last one short; splits straddle images
    (2, 96, 48, 8, 16, 0, 1, False, True),         # two 48-channel input blocks; one split of 8 steps
    (2, 64, 24, 16, 16, 1, 0, True, True),         # ragged second input block; odd channel-tile count (CT = 1)
    (2, 64, 24, 16, 16, 0, 0, False, False),
    (1, 192, 96, 8, 8, 1, 0, False, False),        # deep-level proportions: few pixels, long K, the six-wave workgroup
    (1, 192, 96, 8, 8, 0, 1, True, False),
]


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W,acc_dx,acc_dw,bias,strided", CASES)
def test_one_launch_equals_the_two_launches_bit_for_bit(N, Cin, Cout, H, W, acc_dx, acc_dw, bias, strided, compute):
    pb = Problem(N, Cin, Cout, H, W, compute, strided)
    whole, a = _pair(pb, acc_dx, acc_dw, bias)
    whole.run()                                    # the pair inside one range: one launch where the fused kernel takes the shape
    split, b = _pair(pb, acc_dx, acc_dw, bias)
    split.run(0, 1)                                # op by op: the two launches
    split.run(1, 1)
    _same(a, b, bias)
    # ... and the public entry points (dense tensors; they take no pre-filled dW)
    x16c, dy16c = pb.x16.contiguous().view(torch.int16), pb.dy16.contiguous().view(torch.int16)
    if not acc_dw:
        dw, db = ops.convT_wgrad(x16c, pb.w, dy16c, 2, want_bias=bias, compute=compute, dy16=True, x16=True)
        assert torch.equal(a.dw, dw)
        if bias:
            assert torch.equal(a.db, db)
    dx = ops.convT_dgrad(torch.empty(N, Cin, H, W, device=DEV), pb.w, dy16c, 2, dx=pb.pre_dx[:, pb.ex:pb.ex + Cin].contiguous(),
                         accumulate=bool(acc_dx), compute=compute, dy16=True)
    assert torch.equal(a.dx, dx)


def test_the_reference_itself_is_sound_against_fp64():
    """(3, 48, 48, 16, 24) bf16 against fp64 on the rounded operands, with the tolerances test_ops_gpu.py has for the same kernels
    (test_convT_wgrad_reads_16bit_planar_x: 1e-4, test_convT_backward_reads_16bit_planar_dy: 1e-5, each x max(1, max |want|))."""
    N, Cin, Cout, H, W = 3, 48, 48, 16, 24
    pb = Problem(N, Cin, Cout, H, W, 1)
    prog, out = _pair(pb, 0, 0, True)
    prog.run()
    x, dy = pb.x16.double().cpu(), pb.dy16.double().cpu()
    want_dw = torch.einsum("nchw,ndhawb->cdab", x, dy.view(N, Cout, H, 2, W, 2))
    err = (out.dw.cpu().double() - want_dw).abs().max().item()
    print(f"dW: max err {err:.3e}, max |want| {want_dw.abs().max().item():.3e}")
    assert err <= 1e-4 * max(1.0, want_dw.abs().max().item())
    want_dx = F.conv2d(dy, pb.w.cpu().to(pb.dt).double(), stride=2)
    err = (out.dx.cpu().double() - want_dx).abs().max().item()
    print(f"dx: max err {err:.3e}, max |want| {want_dx.abs().max().item():.3e}")
    assert err <= 1e-5 * max(1.0, want_dx.abs().max().item())
    want_db = dy.sum(dim=(0, 2, 3))
    assert (out.db.cpu().double() - want_db).abs().max().item() <= 1e-4 * max(1.0, want_db.abs().max().item())


@pytest.mark.parametrize("compute", [1, 2])
def test_a_range_boundary_between_the_two_ops_changes_nothing(compute):
    """[WGRAD, DGRAD, WGRAD'] run as ranges (0, 1) + (1, 2): the first pair is cut by the boundary, the second WGRAD has nothing behind
    it -- neither may be fused with anything, and everything equals the pair run inside one range."""
    pb = Problem(3, 48, 48, 16, 24, compute)
    whole, a = _pair(pb, 1, 0, True)
    whole.run(0, 2)
    out, out2, keep = Outputs(pb), Outputs(pb), [pb]
    three = Program([_wgrad_op(pb, out, 0, True, keep), _dgrad_op(pb, out, 1), _wgrad_op(pb, out2, 0, True, keep)], keep + [out, out2])
    three.run(0, 1)
    three.run(1, 2)
    _same(a, out, True)
    assert torch.equal(out2.dw, a.dw) and torch.equal(out2.db, a.db)
    assert torch.equal(out2.dxbuf, pb.pre_dx)             # the lone WGRAD wrote no dx
    # the same three ops in ONE range: the pair fused, the lone WGRAD on its own
    o3, o4, keep = Outputs(pb), Outputs(pb), [pb]
    three = Program([_wgrad_op(pb, o3, 0, True, keep), _dgrad_op(pb, o3, 1), _wgrad_op(pb, o4, 0, True, keep)], keep + [o3, o4])
    three.run()
    _same(a, o3, True)
    assert torch.equal(o4.dw, a.dw) and torch.equal(o4.db, a.db) and torch.equal(o4.dxbuf, pb.pre_dx)


def _five_steps(op_by_op):
    seed_everything(1993)
    m = MTUNetPlusPlus(in_channels=1, out_channels=1, n_classes=3, deep_supervision=True).to(DEV)
    m.set_compute("bf16")
    step = T.FusedTrainStep(m, FusedAdam(m, lr=1e-3, eps=1e-4), alpha=0.5, graph=False)
    pairs = 0
    for s in range(5):
        img, mask, label = O.synthetic_batch(2, 64, 64, seed=70 + s)
        st = step.load_batch(img.to(DEV), mask.to(DEV), label.to(DEV))
        bwd = st.programs["bwd"]
        pairs = sum(1 for i in range(bwd.n - 1)
                    if bwd.array[i].kind == L.OP_CONVT_WGRAD and bwd.array[i + 1].kind == L.OP_CONVT_DGRAD)
        if op_by_op and "run" not in vars(bwd):          # test-local: every op in a range of its own, so nothing is fused
            whole = bwd.run
            bwd.run = lambda first=0, count=None, stream=None: [whole(i, 1, stream) for i in range(first, first + (bwd.n - first if count is None else count))]
        step.run(st)
    step.check_nan()
    return m.flat_p.clone(), pairs


def test_five_training_steps_are_the_same_steps():
    """bf16 MTUNetPlusPlus, N = 2, 64 x 64: five fused steps against the same five with the backward program run op by op."""
    fused, pairs = _five_steps(False)
    plain, _ = _five_steps(True)
    assert pairs > 0, "the backward program has no WGRAD/DGRAD pair: the test would compare nothing"
    assert torch.equal(fused, plain)
