"""The two ops Multi_BTSUNet adds, on the GPU: nearest 2x up-sampling (bit copies forward, a fixed-order 2 x 2 sum backward) and the
batch-shared Linear kernels of a wide input (fp64 cases in the form and with the bounds of tests/test_ops_gpu.py's Linear cases)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402
from oracle import layout_reference as LR  # noqa: E402

DEV = torch.device("cuda:0")


def _ops_gpu():
    import test_ops_gpu as OPS
    return OPS


def _up(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _strided(vals, stride, G):
    """(N, ...) values laid out with a batch stride of `stride` elements inside a guarded buffer; the gaps hold 7.0."""
    N, per = vals.shape[0], vals[0].numel()
    flat = torch.full((N * stride,), 7.0)
    for n in range(N):
        flat[n * stride:n * stride + per] = vals[n].reshape(-1)
    return G(flat)


def _unstrided(flat, shape, stride):
    per = int(np.prod(shape[1:]))
    return torch.stack([flat[n * stride:n * stride + per].view(*shape[1:]) for n in range(shape[0])])


# shape, what is strided (batch stride = dense + 2), the kernels the forward / backward must take
PLANAR = [((2, 16, 16, 16), None, "upsample2_fwd_kernel", "upsample2_bwd_kernel"),                    # the float4 forms; 2048 threads
          ((1, 5, 3, 5), None, "upsample2_fwd_scalar_kernel", "upsample2_bwd_scalar_kernel"),        # odd W
          ((2, 8, 8, 8), "in", "upsample2_fwd_scalar_kernel", "upsample2_bwd_scalar_kernel")]        # the scalar forms by the batch stride
C8_SHAPES = [(2, 8, 4, 4), (3, 24, 8, 12)]                                                            # channel-blocked forward, bf16 and fp16


def up2_case_ops():
    """The op (dummy pointers) of every up-sampling call the three tests below make on the rows of PLANAR and C8_SHAPES: what the launch-coverage
    guard of tests/test_mt_btsunet_launches_gpu.py keys these cases by (tests/step_programs.py _small_op_key)."""
    made = []
    for (N, Cc, H, W), strided, _, _ in PLANAR:
        xs = Cc * H * W + (2 if strided else 0)
        made.append(ops.upsample2_case_args(L.OP_UPSAMPLE2_FWD, N, Cc, H, W, strides=dict(x=xs)))
        made += [ops.upsample2_case_args(L.OP_UPSAMPLE2_BWD, N, Cc, H, W, acc_dx=acc, strides=dict(dx=xs)) for acc in (False, True)]
    made += [ops.upsample2_case_args(L.OP_UPSAMPLE2_FWD, *shape, compute=compute) for shape in C8_SHAPES for compute in (1, 2)]
    return made


@pytest.mark.parametrize("shape,strided,kf,kb", PLANAR, ids=["float4", "oddW", "stride"])
def test_planar_forward_is_repeat_interleave_bit_for_bit(shape, strided, kf, kb):
    OPS = _ops_gpu()
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(11 + W)
    x = torch.randn(*shape, generator=g)
    x.view(-1)[:6] = torch.tensor([float("nan"), -0.0, 0.0, float("inf"), -float("inf"), 1.4e-45])      # a copy moves every bit pattern
    dense = Cc * H * W
    xs = dense + 2 if strided else dense
    X = _strided(x, xs, OPS._Guarded) if strided else OPS._Guarded(x)
    Y = OPS._Guarded(torch.full((N, Cc, 2 * H, 2 * W), 1993.0))
    op = ops.upsample2_case_args(L.OP_UPSAMPLE2_FWD, N, Cc, H, W, ptrs=dict(x=X, y=Y), strides=dict(x=xs))
    assert ops.op_kernel_name(op) == kf
    ops.small_op_launch(op)
    torch.cuda.synchronize()
    got, intact = Y.read()
    assert intact, "memory around y was written"
    assert torch.equal(_bits(got), _bits(_up(x)))
    xin, xintact = X.read()
    assert xintact and torch.equal(_bits(xin), _bits(X.cpu)), "x was written"
    if not strided:
        assert torch.equal(_bits(ops.upsample2_fwd(x.to(DEV)).cpu()), _bits(_up(x)))      # the eager wrapper


@pytest.mark.parametrize("compute", [1, 2], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", C8_SHAPES)
def test_c8_forward_is_the_pack_of_the_upsampled_planes(shape, compute):
    OPS = _ops_gpu()
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(5 * Cc + compute)
    x = torch.randn(*shape, generator=g)
    x.view(-1)[:5] = torch.tensor([float("nan"), -0.0, float("inf"), 65504.0, 1e-8])
    x8 = LR.c8_pack(x.numpy().reshape(N, Cc, H * W), compute)                               # uint16 [N][C/8][HW][8]
    want = LR.c8_pack(_up(x).numpy().reshape(N, Cc, 4 * H * W), compute)
    X = OPS._Guarded(torch.from_numpy(x8.view(np.int16).copy()))
    Y = OPS._Guarded(torch.full((N, Cc // 8, 4 * H * W, 8), 0x5a5a, dtype=torch.int16))
    op = ops.upsample2_case_args(L.OP_UPSAMPLE2_FWD, N, Cc, H, W, ptrs=dict(x=X, y=Y), compute=compute)
    assert ops.op_kernel_name(op) == "upsample2_c8_fwd_kernel"
    ops.small_op_launch(op)
    torch.cuda.synchronize()
    got, intact = Y.read()
    assert intact, "memory around y was written"
    assert np.array_equal(got.numpy().view(np.uint16), want)
    xin, xintact = X.read()
    assert xintact and torch.equal(xin, X.cpu)
    y8 = ops.upsample2_fwd(ops.C8(torch.from_numpy(x8.view(np.int16).copy()).to(DEV), shape, compute))      # the eager wrapper on a C8 tensor
    assert y8.shape == (N, Cc, 2 * H, 2 * W) and np.array_equal(y8.data.cpu().numpy().view(np.uint16), want)


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("shape,strided,kf,kb", PLANAR, ids=["float4", "oddW", "stride"])
def test_backward_sums_each_window_in_the_stated_order(shape, strided, kf, kb, acc):
    """dx (+)= (dy[2h,2w] + dy[2h,2w+1]) + (dy[2h+1,2w] + dy[2h+1,2w+1]) in fp32.  Three (accumulate: four) IEEE additions with no other
    arithmetic: the same expression in float32 torch on the CPU gives the same bits, and that is asserted.  Against fp64 the error of that
    expression is at most a few fp32 ulps of the largest term; the figure is printed and barred at twice what the CPU's fp32 sum shows
    on the same data (the two are equal when the bits are).  Measured on an MI355X, in ulps of the largest term, store / accumulate: float4
    1.649 / 2.220, odd W 0.734 / 1.032, strided 1.246 / 2.377 -- on the device and on the CPU alike, bit-equal in all six cases."""
    OPS = _ops_gpu()
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(31 + W + int(acc))
    dy = torch.randn(N, Cc, 2 * H, 2 * W, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 4, (N, Cc, 2 * H, 2 * W), generator=g)
    pre = torch.randn(*shape, generator=g)
    dense = Cc * H * W
    xs = dense + 2 if strided else dense
    DY = OPS._Guarded(dy)
    DX = _strided(pre, xs, OPS._Guarded) if strided else OPS._Guarded(pre)
    op = ops.upsample2_case_args(L.OP_UPSAMPLE2_BWD, N, Cc, H, W, ptrs=dict(dy=DY, dx=DX), acc_dx=acc, strides=dict(dx=xs))
    assert ops.op_kernel_name(op) == kb
    ops.small_op_launch(op)
    torch.cuda.synchronize()
    flat, intact = DX.read()
    assert intact, "memory around dx was written"
    got = _unstrided(flat, shape, xs) if strided else flat
    if strided:
        gaps = torch.cat([flat[n * xs + dense:(n + 1) * xs] for n in range(N)])
        assert bool((gaps == 7.0).all()), "the floats between the images of dx were written"
    d = lambda a, b: dy[:, :, a::2, b::2]      # noqa: E731
    want32 = (d(0, 0) + d(0, 1)) + (d(1, 0) + d(1, 1))
    want64 = (d(0, 0).double() + d(0, 1).double()) + (d(1, 0).double() + d(1, 1).double())
    if acc:
        want32, want64 = want32 + pre, want64 + pre.double()
    big = torch.stack([d(0, 0).abs(), d(0, 1).abs(), d(1, 0).abs(), d(1, 1).abs()] + ([pre.abs()] if acc else [])).max(dim=0).values.double()
    ulp = big * 2.0 ** -23
    e_gpu, e_cpu = ((got.double() - want64).abs() / ulp).max().item(), ((want32.double() - want64).abs() / ulp).max().item()
    print(f"{kb} acc={acc}: error in ulps of the largest term: device {e_gpu:.3f}, float32 on the CPU {e_cpu:.3f}; bit-equal {torch.equal(_bits(got), _bits(want32))}")
    # each inner sum is at most 2 x the largest term (half an ulp of it: 1 ulp of the term), the outer one 4 x (2 ulps), the accumulate 5 x (4)
    assert e_cpu <= (8.0 if acc else 4.0)
    assert e_gpu <= 2.0 * e_cpu
    assert torch.equal(_bits(got), _bits(want32))
    dyin, dyintact = DY.read()
    assert dyintact and torch.equal(_bits(dyin), _bits(dy)), "dy was written"
    if not strided:
        eager = ops.upsample2_bwd(dy.to(DEV), pre.to(DEV).clone() if acc else None, accumulate=acc)
        assert torch.equal(_bits(eager.cpu()), _bits(want32))


# ------------------------------------------------------------------------------------------------ the batch-shared Linear kernels
_WF = "linear_wide_fwd_kernel + linear_wide_reduce_kernel"
_WIDE_CASES = [
    ("lin_fwd", (2, 8192, 256), dict(relu=True), ()),          # exact zeros where the ReLU cut
    ("lin_bwd", (2, 8192, 256), dict(relu=True), ()),          # the model's layer: the masked gradient, dx in eight ranges of outputs
    ("lin_fwd", (7, 16384, 32), {}, ()),
    ("lin_bwd", (7, 16384, 32), {}, ()),
    ("lin_fwd", (33, 8192, 40), dict(bias=False), ()),         # Out not a multiple of the wave's four rows; five passes, the last with one sample
    ("lin_bwd", (33, 8192, 40), dict(relu=True), ()),          # ... nor of a range of outputs (two ranges of 20: five groups of four)
    ("lin_fwd", (65, 8192, 32), {}, ()),                       # beyond one pass of eight samples: nine
    ("lin_bwd", (65, 8192, 32), {}, ()),
    ("lin_bwd", (2, 8192, 256), dict(relu=True, dx=False), ()),
    ("lin_bwd", (7, 16384, 32), dict(acc_dw=True), ()),
    ("lin_bwd", (9, 4096, 8), {}, ()),                         # the threshold itself, one range of outputs: dx written without a reduction
]


@pytest.mark.parametrize("case", _WIDE_CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-{','.join(sorted(c[2]))}" for c in _WIDE_CASES])
def test_wide_linear_cases_match_fp64(case):
    """tests/test_ops_gpu.py's own Linear runner, references and bounds (y, dx: 1e-5 x max |ref|; dW, dbias: 1e-4 x max(1, max |ref|); exact
    zeros where the ReLU cut; inputs, unasked outputs, canaries and the floats behind the workspace untouched) on shapes the batch-shared
    kernels take."""
    OPS = _ops_gpu()
    name = ops.op_kernel_name(OPS._small_case_ops(case)[0])
    if case[2].get("dx", True) or case[0] == "lin_fwd":
        assert "linear_wide_" in name, name
    OPS.test_small_op_step_instances_match_fp64(case)


def _launch_linear(kind, N, In, Out, seed, relu=True):
    g = torch.Generator().manual_seed(seed)
    T = dict(x=torch.randn(N, In, generator=g), w=torch.randn(Out, In, generator=g) * In ** -0.5, bias=torch.randn(Out, generator=g) * 0.1,
             dy=torch.randn(N, Out, generator=g))
    T = {k: v.to(DEV) for k, v in T.items()}
    T["y"] = torch.relu(T["x"] @ T["w"].t() + T["bias"]) if kind == L.OP_LINEAR_BWD else torch.full((N, Out), 3.0, device=DEV)
    T.update(dx=torch.full((N, In), 3.0, device=DEV), dw=torch.full((Out, In), 3.0, device=DEV), dbias=torch.full((Out,), 3.0, device=DEV))
    op = ops.linear_case_args(kind, N, In, Out, ptrs=T, relu=relu)
    ops.small_op_launch(op)
    torch.cuda.synchronize()
    return ops.op_kernel_name(op), {k: T[k].clone() for k in ("y", "dx", "dw", "dbias")}


def test_below_the_threshold_the_old_kernels_run_and_the_switch_restores_them_above_it():
    F_, B_ = L.OP_LINEAR_FWD, L.OP_LINEAR_BWD
    below = L.LINEAR_WIDE_MIN_IN - 4
    on = [_launch_linear(k, 3, below, 24, 5) for k in (F_, B_)]
    assert on[0][0] == "linear_fwd_kernel" and on[1][0] == "linear_mask_kernel + linear_dx_kernel [Out>=8] + linear_dw_kernel"
    wide = [_launch_linear(k, 3, 8192, 24, 6) for k in (F_, B_)]
    assert wide[0][0] == _WF and "linear_wide_dx_kernel" in wide[1][0]
    assert ops.linear_wide(False) is True
    try:
        off = [_launch_linear(k, 3, below, 24, 5) for k in (F_, B_)]
        old = [_launch_linear(k, 3, 8192, 24, 6) for k in (F_, B_)]
        # the switch set: a wide case is a case of the per-sample kernels again, launches checked against the plan, results against fp64
        _ops_gpu().test_small_op_step_instances_match_fp64(("lin_bwd", (2, 8192, 256), dict(relu=True), ()))
    finally:
        assert ops.linear_wide(True) is False
    for a, b in zip(on, off):                # below the threshold: the same launches, the same bits, switch or no switch
        assert a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert old[0][0] == "linear_fwd_kernel" and old[1][0] == "linear_mask_kernel + linear_dx_kernel [Out>=8] + linear_dw_kernel"
    # ... and above it both arms compute the same layer: y and dx within the forward bound of the fp64 cases of each other's scale, dW by the same kernel
    for k, tol in (("y", 2e-5), ("dx", 2e-5)):
        a, b = wide[0 if k == "y" else 1][1][k], old[0 if k == "y" else 1][1][k]
        assert (a - b).abs().max().item() <= tol * b.abs().max().item(), k
    assert torch.equal(wide[1][1]["dw"], old[1][1]["dw"]) and torch.equal(wide[1][1]["dbias"], old[1][1]["dbias"])


def test_two_runs_of_a_wide_case_are_bit_equal():
    for kind in (L.OP_LINEAR_FWD, L.OP_LINEAR_BWD):
        a, b = _launch_linear(kind, 11, 16384, 40, 9), _launch_linear(kind, 11, 16384, 40, 9)
        assert "linear_wide_" in a[0] and a[0] == b[0]
        assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]), kind
