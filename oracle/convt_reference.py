"""Plain fp64 reference of ConvTranspose2d with kernel == stride == k and its three gradients, written on the (N, C, H, k, W, k) view of
the up-sampled tensor: output pixel (k i + a, k j + b) depends on input pixel (i, j) and weight tap (a, b) only, so every part is one
contraction.  Operands are taken as they are (cast to fp64, never rounded): a test rounds them to the stored type first.

    y[n, d, k i + a, k j + b] = bias[d] + sum_c x[n, c, i, j] w[c, d, a, b]          weight layout = torch (Cin, Cout, k, k)

tests/test_convt_reference_cpu.py checks these four against torch.nn.functional.conv_transpose2d and its autograd."""
from __future__ import annotations

from typing import Optional

import torch


def _view6(t: torch.Tensor, k: int) -> torch.Tensor:
    N, C, Hk, Wk = t.shape
    assert Hk % k == 0 and Wk % k == 0, (tuple(t.shape), k)
    return t.reshape(N, C, Hk // k, k, Wk // k, k)


def convT_fwd64(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], k: int) -> torch.Tensor:
    """(N, Cin, H, W), (Cin, Cout, k, k), (Cout) or None -> (N, Cout, kH, kW), fp64."""
    N, _, H, W = x.shape
    assert w.shape[0] == x.shape[1] and tuple(w.shape[2:]) == (k, k), (tuple(x.shape), tuple(w.shape), k)
    y = torch.einsum("nchw,cdab->ndhawb", x.double(), w.double()).reshape(N, w.shape[1], H * k, W * k)
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def convT_dx64(dy: torch.Tensor, w: torch.Tensor, k: int) -> torch.Tensor:
    """(N, Cout, kH, kW), (Cin, Cout, k, k) -> dL/dx (N, Cin, H, W), fp64."""
    return torch.einsum("ndhawb,cdab->nchw", _view6(dy.double(), k), w.double())


def convT_dw64(x: torch.Tensor, dy: torch.Tensor, k: int) -> torch.Tensor:
    """(N, Cin, H, W), (N, Cout, kH, kW) -> dL/dw (Cin, Cout, k, k), fp64."""
    return torch.einsum("nchw,ndhawb->cdab", x.double(), _view6(dy.double(), k))


def convT_dbias64(dy: torch.Tensor) -> torch.Tensor:
    """(N, Cout, kH, kW) -> dL/dbias (Cout), fp64."""
    return dy.double().sum(dim=(0, 2, 3))
