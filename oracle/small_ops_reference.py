"""Plain fp64 references of the small ops of a training step: MaxPool2d(2, 2), the 1x1 convolution, AdaptiveAvgPool2d(1) + Flatten, Linear
(+ ReLU) and the combined ConvTranspose2d(k = s) + Conv2d(1x1) deep-supervision head, each with its gradients.  Operands are taken as they
are (cast to fp64, never rounded): a test rounds them to the stored type first.  Every cast to fp64 is exact, so the max-pool -- a
selection, not arithmetic -- returns stored values bit for bit, NaN and the sign of zero included.

tests/test_small_ops_reference_cpu.py checks all of them against torch.nn.functional and its autograd in fp64."""
from __future__ import annotations

from typing import Optional, Tuple

import torch


# ------------------------------------------------------------------ MaxPool2d(2, 2)
def _windows(x: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the window positions in the order (0,0), (0,1), (1,0), (1,1)."""
    N, C, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0, tuple(x.shape)
    return x.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def maxpool_argmax(x: torch.Tensor) -> torch.Tensor:
    """Position 0 .. 3 of each window's maximum by ATen's max_pool2d scan: in the order (0,0), (0,1), (1,0), (1,1) an element replaces the
    running maximum when it is greater OR a NaN.  So: the FIRST of equal maxima (-0 and +0 are equal), and a NaN is the maximum wherever it
    sits -- of several NaN the LAST one, since each replaces the one before.  (N, C, H/2, W/2) int64."""
    v = _windows(x.double())
    m, arg = v[..., 0], torch.zeros(v.shape[:-1], dtype=torch.int64)
    for q in range(1, 4):
        c = v[..., q]
        take = (c > m) | torch.isnan(c)
        m, arg = torch.where(take, c, m), torch.where(take, torch.full_like(arg, q), arg)
    return arg


def maxpool_fwd64(x: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) -> the element at maxpool_argmax of every window, fp64 (exact: NaN stays NaN, -0 stays -0)."""
    return _windows(x.double()).gather(-1, maxpool_argmax(x).unsqueeze(-1)).squeeze(-1)


def maxpool_argmax_codes(x: torch.Tensor) -> torch.Tensor:
    """mtbc_maxpool_args.argmax: (N, C/8, H/2 * W/2) int64 codes, bits [2c + 1 : 2c] = maxpool_argmax of channel 8g + c."""
    arg = maxpool_argmax(x)
    N, C, oH, oW = arg.shape
    assert C % 8 == 0, C
    a = arg.reshape(N, C // 8, 8, oH * oW)
    return sum(a[:, :, c] << (2 * c) for c in range(8))


def maxpool_bwd64(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dL/dx (N, C, H, W), fp64: each dy element at maxpool_argmax of its window, zero elsewhere."""
    N, C, H, W = x.shape
    d = torch.zeros(N, C, H // 2, W // 2, 4, dtype=torch.float64)
    d.scatter_(-1, maxpool_argmax(x).unsqueeze(-1), dy.double().unsqueeze(-1))
    return d.reshape(N, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)


# ------------------------------------------------------------------ Conv2d(k = 1), weight (Cout, Cin) or (Cout, Cin, 1, 1)
def _w2(w: torch.Tensor) -> torch.Tensor:
    return w.double().reshape(w.shape[0], w.shape[1])


def conv1x1_fwd64(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    y = torch.einsum("nchw,dc->ndhw", x.double(), _w2(w))
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def conv1x1_dx64(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return torch.einsum("ndhw,dc->nchw", dy.double(), _w2(w))


def conv1x1_dw64(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin), fp64."""
    return torch.einsum("nchw,ndhw->dc", x.double(), dy.double())


def conv1x1_dbias64(dy: torch.Tensor) -> torch.Tensor:
    return dy.double().sum(dim=(0, 2, 3))


# ------------------------------------------------------------------ AdaptiveAvgPool2d(1) + Flatten
def gap_fwd64(x: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) -> (N, C), fp64."""
    return x.double().mean(dim=(2, 3))


def gap_bwd64(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """(N, C) -> (N, C, H, W), fp64."""
    N, C = dy.shape
    return (dy.double() / (H * W)).view(N, C, 1, 1).expand(N, C, H, W).contiguous()


# ------------------------------------------------------------------ Linear (+ ReLU), weight (Out, In)
def linear_fwd64(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    y = x.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    return y.clamp_min(0.0) if relu else y


def linear_bwd64(x: torch.Tensor, w: torch.Tensor, y: Optional[torch.Tensor], dy: torch.Tensor,
                 relu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx (N, In), dW (Out, In), dbias (Out)), fp64.  With relu the gradient passes where the STORED output y is > 0 (y is then needed)."""
    g = dy.double()
    if relu:
        g = torch.where(y.double() > 0, g, torch.zeros_like(g))
    return g @ w.double(), g.t() @ x.double(), g.sum(dim=0)


# ------------------------------------------------------------------ ConvTranspose2d(Cin -> Cmid, k = s) + Conv2d(Cmid -> R, 1x1) as one ConvT
def head_combine64(wT: torch.Tensor, bT: Optional[torch.Tensor], w1: torch.Tensor,
                   b1: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """wT (Cin, Cmid, k, k), bT (Cmid) or None, w1 (R, Cmid[, 1, 1]), b1 (R) or None -> Wc (Cin, R, k, k), bc (R):
    Wc[ci, r, a, b] = sum_co wT[ci, co, a, b] w1[r, co];  bc[r] = sum_co bT[co] w1[r, co] + b1[r]."""
    w1_ = _w2(w1)
    Wc = torch.einsum("cmab,rm->crab", wT.double(), w1_)
    bc = torch.zeros(w1_.shape[0], dtype=torch.float64)
    if bT is not None:
        bc = bc + w1_ @ bT.double()
    if b1 is not None:
        bc = bc + b1.double()
    return Wc, bc


def head_expand64(wT: torch.Tensor, bT: Optional[torch.Tensor], w1: torch.Tensor, G: torch.Tensor,
                  gb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The gradients G of Wc and gb of bc mapped back onto the four parameter tensors: (dwT (Cin, Cmid, k, k), dbT (Cmid), dw1 (R, Cmid), db1 (R)).
    Without bT the gb * bT term of dw1 is absent."""
    w1_, G_, gb_ = _w2(w1), G.double(), gb.double()
    dwT = torch.einsum("crab,rm->cmab", G_, w1_)
    dbT = gb_ @ w1_
    dw1 = torch.einsum("crab,cmab->rm", G_, wT.double())
    if bT is not None:
        dw1 = dw1 + gb_.view(-1, 1) * bT.double().view(1, -1)
    return dwT, dbT, dw1, gb_.clone()
