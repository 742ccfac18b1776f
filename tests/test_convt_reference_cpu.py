"""oracle/convt_reference.py -- the fp64 reference the element-wise ConvT tests of tests/test_ops_gpu.py compare the kernels with -- against
torch.nn.functional.conv_transpose2d and its autograd in fp64: two independent formulations of the same operator agree to rounding."""
import pytest
import torch
import torch.nn.functional as F

from oracle import convt_reference as R


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,Cin,Cout,H,W,k", [(2, 5, 3, 4, 6, 2), (3, 7, 1, 5, 3, 4), (1, 4, 6, 2, 5, 8), (2, 24, 16, 8, 16, 2)])
def test_fp64_convT_reference_matches_torch_autograd(N, Cin, Cout, H, W, k, bias):
    g = torch.Generator().manual_seed(1993 + N + Cin + Cout + H + W + k)
    x = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cin, Cout, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
    dy = torch.randn(N, Cout, H * k, W * k, generator=g, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, b, stride=k)
    y.backward(dy)

    def same(got, want, what):
        assert got.dtype == torch.float64 and got.shape == want.shape, what
        err = (got - want).abs().max().item()
        assert err <= 1e-12 * want.abs().max().item(), f"{what}: {err:.3e}"

    same(R.convT_fwd64(x.detach(), w.detach(), None if b is None else b.detach(), k), y.detach(), "forward")
    same(R.convT_dx64(dy, w.detach(), k), x.grad, "dx")
    same(R.convT_dw64(x.detach(), dy, k), w.grad, "dW")
    if bias:
        same(R.convT_dbias64(dy), b.grad, "dbias")


def test_fp64_convT_reference_takes_lower_precision_operands_as_stored():
    """fp32 / 16-bit operands are cast, never rounded again: the result is the fp64 result on the same values."""
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(2, 8, 4, 4, generator=g).bfloat16(), torch.randn(8, 4, 2, 2, generator=g).half()
    assert torch.equal(R.convT_fwd64(x, w, None, 2), R.convT_fwd64(x.double(), w.double(), None, 2))
