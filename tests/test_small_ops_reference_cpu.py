"""oracle/small_ops_reference.py -- the fp64 references the element-wise small-op tests of tests/test_ops_gpu.py compare the kernels with --
against torch.nn.functional and its autograd in fp64: two independent formulations of the same operator.  Continuous results agree to
rounding (1e-12 x max |ref|); the max-pool is a selection and is compared exactly, NaN and the sign of zero included."""
import pytest
import torch
import torch.nn.functional as F

from oracle import small_ops_reference as R

NAN, INF = float("nan"), float("inf")


def _g(*k):
    return torch.Generator().manual_seed(1993 + sum((i + 1) * v for i, v in enumerate(k)))


def _same(got, want, what):
    assert got.dtype == torch.float64 and got.shape == want.shape, what
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * want.abs().max().item(), f"{what}: {err:.3e}"


def _identical(got, want, what):
    """Equal as bit patterns up to the NaN payload: NaN where NaN, else the same value with the same sign of zero."""
    assert got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN positions"
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok]) and torch.equal(torch.signbit(got[ok]), torch.signbit(want[ok])), what


# windows in (0,0), (0,1), (1,0), (1,1) order -> (expected maximum, expected position)
WINDOWS = [
    ([NAN, 1, 2, 3], 0), ([1, NAN, 2, 3], 1), ([1, 2, NAN, 3], 2), ([1, 2, 3, NAN], 3),      # a NaN is the maximum wherever it sits
    ([1, NAN, NAN, 3], 2), ([NAN, 5, 1, NAN], 3), ([INF, NAN, 1, 2], 1),                     # every NaN replaces the maximum: the LAST NaN; a NaN beats +inf
    ([INF, 1, 2, 3], 0), ([1, 2, INF, INF], 2), ([-INF, -INF, -INF, -INF], 0), ([-INF, -3, -INF, -5], 1),
    ([7, 7, 1, 2], 0), ([7, 1, 7, 2], 0), ([7, 1, 2, 7], 0), ([1, 7, 7, 2], 1), ([1, 7, 2, 7], 1), ([1, 2, 7, 7], 2), ([4, 4, 4, 4], 0),
    ([-0.0, 0.0, 0.0, -0.0], 0), ([0.0, -0.0, -0.0, 0.0], 0), ([-1, -0.0, 0.0, -2], 1), ([-1, 0.0, -0.0, -2], 1),      # -0 == +0: the first of them
]


def test_fp64_maxpool_reference_on_crafted_windows_matches_aten():
    """NaN at every position, two NaNs, infinities, equal maxima at every pair of positions and -0 / +0 ties: value, position and routing,
    against the table above AND against ATen's max_pool2d with indices."""
    x = torch.tensor([w for w, _ in WINDOWS], dtype=torch.float64).reshape(1, len(WINDOWS), 2, 2)
    pos = torch.tensor([p for _, p in WINDOWS])
    assert torch.equal(R.maxpool_argmax(x).reshape(-1), pos)
    want = x.reshape(-1, 4)[torch.arange(len(WINDOWS)), pos].reshape(1, -1, 1, 1)
    _identical(R.maxpool_fwd64(x), want, "value")
    y, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    _identical(R.maxpool_fwd64(x), y, "value against ATen")
    assert torch.equal(R.maxpool_argmax(x), idx), "position against ATen"        # a 2 x 2 plane: the flat index is the window position
    dy = torch.arange(1.0, len(WINDOWS) + 1, dtype=torch.float64).reshape(1, -1, 1, 1)
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(dy)
    assert torch.equal(R.maxpool_bwd64(x, dy), xr.grad), "routing against ATen"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,C,H,W", [(2, 8, 6, 10), (1, 16, 4, 4), (3, 3, 8, 2)])
def test_fp64_maxpool_reference_matches_aten(N, C, H, W, dtype):
    """Random planes with many ties (few distinct values), some NaN and signed zeros: exact against ATen in fp64 on the same stored values."""
    g = _g(N, C, H, W)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).double() * 0.5
    x[torch.rand(N, C, H, W, generator=g) < 0.05] = NAN
    x[torch.rand(N, C, H, W, generator=g) < 0.1] = -0.0
    x = x.to(dtype)
    dy = torch.randn(N, C, H // 2, W // 2, generator=g, dtype=torch.float64)
    xr = x.double().requires_grad_(True)
    y, idx = F.max_pool2d(xr, 2, 2, return_indices=True)
    y.backward(dy)
    _identical(R.maxpool_fwd64(x), y.detach(), "value")
    arg = R.maxpool_argmax(x)
    oy, ox = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    assert torch.equal((2 * oy + arg // 2) * W + 2 * ox + arg % 2, idx), "position"
    assert torch.equal(R.maxpool_bwd64(x, dy), xr.grad), "routing"
    if C % 8 == 0:
        codes = R.maxpool_argmax_codes(x)
        assert codes.shape == (N, C // 8, (H // 2) * (W // 2))
        for c in range(C):
            assert torch.equal((codes[:, c // 8] >> (2 * (c % 8))) & 3, arg[:, c].reshape(N, -1))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 5, 3, 4, 6), (3, 16, 1, 2, 2), (1, 8, 10, 3, 5)])
def test_fp64_conv1x1_reference_matches_torch_autograd(N, Cin, Cout, H, W, bias):
    g = _g(N, Cin, Cout, H, W)
    x = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, 1, 1, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
    dy = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b)
    y.backward(dy)
    _same(R.conv1x1_fwd64(x.detach(), w.detach(), None if b is None else b.detach()), y.detach(), "forward")
    _same(R.conv1x1_dx64(dy, w.detach()), x.grad, "dx")
    _same(R.conv1x1_dw64(x.detach(), dy), w.grad.reshape(Cout, Cin), "dW")
    if bias:
        _same(R.conv1x1_dbias64(dy), b.grad, "dbias")


@pytest.mark.parametrize("N,C,H,W", [(2, 5, 5, 7), (3, 2, 16, 16), (1, 9, 1, 1)])
def test_fp64_gap_reference_matches_torch_autograd(N, C, H, W):
    g = _g(N, C, H, W)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(N, C, generator=g, dtype=torch.float64)
    y = F.adaptive_avg_pool2d(x, 1).flatten(1)
    y.backward(dy)
    _same(R.gap_fwd64(x.detach()), y.detach(), "forward")
    _same(R.gap_bwd64(dy, H, W), x.grad, "dx")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,In,Out", [(11, 70, 13), (3, 16, 3), (1, 5, 9)])
def test_fp64_linear_reference_matches_torch_autograd(N, In, Out, bias, relu):
    g = _g(N, In, Out)
    x = torch.randn(N, In, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Out, In, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Out, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
    dy = torch.randn(N, Out, generator=g, dtype=torch.float64)
    y = F.linear(x, w, b)
    y = F.relu(y) if relu else y
    y.backward(dy)
    got = R.linear_fwd64(x.detach(), w.detach(), None if b is None else b.detach(), relu)
    _same(got, y.detach(), "forward")
    if relu:
        assert bool((got == 0).any()) and bool((got > 0).any())
    dx, dw, db = R.linear_bwd64(x.detach(), w.detach(), y.detach(), dy, relu)
    _same(dx, x.grad, "dx")
    _same(dw, w.grad, "dW")
    if bias:
        _same(db, b.grad, "dbias")


def test_fp64_linear_reference_masks_on_the_stored_output():
    """The ReLU mask is y > 0 on the y it is GIVEN: an output stored as exactly 0 passes no gradient, whatever the pre-activation was."""
    x, w = torch.tensor([[1.0, 2.0]]), torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    dx, dw, db = R.linear_bwd64(x, w, torch.tensor([[0.0, 2.0]]), torch.tensor([[5.0, 7.0]]), True)
    assert torch.equal(dx, torch.tensor([[0.0, 7.0]], dtype=torch.float64))
    assert torch.equal(dw, torch.tensor([[0.0, 0.0], [7.0, 14.0]], dtype=torch.float64)) and torch.equal(db, torch.tensor([0.0, 7.0], dtype=torch.float64))


@pytest.mark.parametrize("with_bT,with_b1", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("Cin,Cmid,Rg,k", [(6, 5, 1, 2), (4, 7, 3, 4), (3, 2, 3, 8)])
def test_fp64_head_reference_matches_the_two_layers(Cin, Cmid, Rg, k, with_bT, with_b1):
    """Wc / bc reproduce Conv2d_1x1(ConvTranspose2d_k(x)); the expansion of the combined layer's gradients is the two layers' autograd."""
    g = _g(Cin, Cmid, Rg, k)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64, requires_grad=True)      # noqa: E731
    x, wT, w1 = mk(2, Cin, 3, 5), mk(Cin, Cmid, k, k), mk(Rg, Cmid, 1, 1)
    bT, b1 = (mk(Cmid) if with_bT else None), (mk(Rg) if with_b1 else None)
    dy = torch.randn(2, Rg, 3 * k, 5 * k, generator=g, dtype=torch.float64)
    y = F.conv2d(F.conv_transpose2d(x, wT, bT, stride=k), w1, b1)
    y.backward(dy)
    d = lambda t: None if t is None else t.detach()      # noqa: E731
    Wc, bc = R.head_combine64(d(wT), d(bT), d(w1), d(b1))
    Wc.requires_grad_(True), bc.requires_grad_(True)
    yc = F.conv_transpose2d(x.detach(), Wc, bc, stride=k)
    _same(yc.detach(), y.detach(), "combined forward")
    yc.backward(dy)
    dwT, dbT, dw1, db1 = R.head_expand64(d(wT), d(bT), d(w1), Wc.grad, bc.grad)
    _same(dwT, wT.grad, "dwT")
    _same(dw1, w1.grad.reshape(Rg, Cmid), "dw1")
    if with_bT:
        _same(dbT, bT.grad, "dbT")
    if with_b1:
        _same(db1, b1.grad, "db1")


def test_fp64_small_op_references_take_lower_precision_operands_as_stored():
    """fp32 / 16-bit operands are cast, never rounded again: the result is the fp64 result on the same values."""
    g = _g(7)
    x, w = torch.randn(2, 8, 4, 4, generator=g).bfloat16(), torch.randn(3, 8, 1, 1, generator=g).half()
    assert torch.equal(R.conv1x1_fwd64(x, w, None), R.conv1x1_fwd64(x.double(), w.double(), None))
    assert torch.equal(R.gap_fwd64(x), R.gap_fwd64(x.double()))
    assert torch.equal(R.maxpool_fwd64(x), R.maxpool_fwd64(x.double()))
