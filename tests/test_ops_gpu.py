"""Per-op parity of the HIP kernels (through the C-ABI) against the same torch op on the CPU in fp32.
Tolerances are written per test; integer results are bit-exact."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import ops  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
from step_programs import (COLLECTORS, PLAN, STEP_PROGRAMS, _c8_key, _conv3_key, _convT_key, _dparam_key, _instnorm_key, _pack_key,  # noqa: E402
                           _small_op_key, _wgrad_plan_key, _wview_key, assert_all_tested, assert_op_kinds_claimed, assert_rows_needed, survey,
                           table_keys)

DEV = "cuda:0"


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, want, rtol, atol, what=""):
    got = got.detach().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, max |want| {want.abs().max().item():.3e}"


# (N, segs, Cout, H, W): geometry wide / 16-wide / 8x8, multi-segment virtual concat, ragged channel tiles
CONV_CASES = [
    (2, [8], 16, 32, 32),
    (1, [24, 48], 24, 40, 64),          # UNet++ level-0 style node, H not a multiple of 8
    (2, [24, 24, 24, 48], 24, 16, 32),
    (3, [16], 40, 16, 16),              # 16-wide geometry, Cout not a multiple of 16
    (2, [96, 96], 96, 16, 16),          # MT=3 x 2 blocks
    (5, [32], 80, 8, 8),                # 8x8 geometry: 4 images / block, ragged batch
    (6, [64, 64], 320, 8, 8),
    (1, [8], 8, 24, 48),                # width not a multiple of 32
    (2, [128], 64, 32, 32),
    (2, [320, 320, 320], 512, 16, 16),  # MTnnUNet classifier conv at 256^2 input
    (2, [320], 320, 8, 8),              # bottleneck, fewer images than a block holds
    (2, [320, 320], 256, 16, 16),
    (1, [384, 384, 384], 512, 16, 16),  # UNet++ classifier conv
    (2, [48], 48, 32, 32),              # 48-channel output blocks (3 tiles, 384-thread wgrad blocks)
    (2, [24, 24], 48, 16, 16),
    (3, [64], 144, 8, 8),
]


@pytest.mark.parametrize("N,segs,Cout,H,W", CONV_CASES)
def test_conv3x3_mfma_fwd_dgrad_wgrad(N, segs, Cout, H, W):
    g = _g(N * 1000 + Cout + H)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    xcat = torch.cat(xs, 1).requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = F.conv2d(xcat, wr, br, padding=1)
    z.backward(dz)
    dxs_ref = torch.split(xcat.grad, segs, dim=1)

    xd = [x.to(DEV) for x in xs]
    wd, bd, dzd = w.to(DEV), b.to(DEV), dz.to(DEV)
    pf, pd = ops.conv3x3_pack(wd)
    zg = ops.conv3x3_fwd(xd, wd, bd, packed=pf)
    _close(zg, z.detach(), 2e-5, 2e-5, "fwd")
    # dgrad: first segment overwritten, the others accumulate onto a preset value
    pre = [torch.randn(N, c, H, W, generator=g) for c in segs]
    dxd = [p.to(DEV).clone() for p in pre]
    acc = [0] + [1] * (len(segs) - 1)
    ops.conv3x3_dgrad(dzd, wd, dxd, acc, packed=pd)
    for i, (got, want) in enumerate(zip(dxd, dxs_ref)):
        _close(got, want + (pre[i] if acc[i] else 0), 2e-5, 5e-5, f"dgrad seg {i}")
    dw, db = ops.conv3x3_wgrad(xd, dzd, tuple(w.shape), want_bias=True)
    scale = max(1.0, wr.grad.abs().max().item())
    _close(dw, wr.grad, 1e-4, 2e-5 * scale, "wgrad")
    _close(db, br.grad, 1e-4, 1e-4 * max(1.0, br.grad.abs().max().item()), "dbias")
    # shared-module accumulation (F10)
    dw2, _ = ops.conv3x3_wgrad(xd, dzd, tuple(w.shape), dw=dw.clone(), accumulate=True)
    _close(dw2, 2 * wr.grad, 1e-4, 4e-5 * scale, "wgrad accumulate")


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 1, 32, 64, 64), (1, 3, 5, 7, 9), (2, 12, 8, 4, 4), (1, 8, 8, 2, 2),
                                             (3, 1, 24, 40, 24), (2, 2, 5, 8, 12)])
def test_conv3x3_direct_path(N, Cin, Cout, H, W):
    g = _g(Cin * 7 + H)
    x = (torch.rand(N, Cin, H, W, generator=g) * 255.0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    dz = torch.randn(N, Cout, H, W, generator=g)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, None, padding=1)
    z.backward(dz)
    xd, wd, dzd = x.to(DEV), w.to(DEV), dz.to(DEV)
    zg = ops.conv3x3_fwd([xd], wd, None, packed=None)
    _close(zg, z.detach(), 1e-5, 1e-3, "direct fwd")
    dx = torch.zeros_like(xd)
    ops.conv3x3_dgrad(dzd, wd, [dx], [0], packed=None)
    _close(dx, xr.grad, 1e-5, 1e-5, "direct dgrad")
    dw, _ = ops.conv3x3_wgrad([xd], dzd, tuple(w.shape))
    _close(dw, wr.grad, 1e-4, 1e-4 * max(1.0, wr.grad.abs().max().item()), "direct wgrad")


@pytest.mark.parametrize("N,Cout,H,W", [(2, 24, 64, 64), (1, 5, 8, 12), (3, 32, 40, 24)])
def test_stem_kernel_equals_direct_kernel_bitwise(N, Cout, H, W):
    """Cin == 1: the vectorised stem kernel keeps the direct kernel's fmaf order -> identical bits (bias included)."""
    g = _g(Cout + H)
    x = (torch.rand(N, 1, H, W, generator=g) * 255.0).to(DEV)
    w = (torch.randn(Cout, 1, 3, 3, generator=g) * 0.1).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    assert torch.equal(ops.conv3x3_fwd([x], w, b), ops.conv3x3_fwd([x], w, b, force_direct=True))
    assert torch.equal(ops.conv3x3_fwd([x], w, None), ops.conv3x3_fwd([x], w, None, force_direct=True))


def test_conv3x3_mfma_equals_direct_kernel():
    g = _g(11)
    x = torch.randn(2, 16, 32, 32, generator=g).to(DEV)
    w = (torch.randn(24, 16, 3, 3, generator=g) * 0.1).to(DEV)
    pf, _ = ops.conv3x3_pack(w)
    a = ops.conv3x3_fwd([x], w, None, packed=pf)
    b = ops.conv3x3_fwd([x], w, None, packed=pf, force_direct=True)
    _close(a, b.cpu(), 1e-5, 1e-5, "mfma vs direct")


@pytest.mark.parametrize("compute", [0, 1, 2])
def test_pack_many_equals_single_packs(compute):
    """The batched weight-image launch must write bit-for-bit what the per-tensor entry points write (110 tensors:
    more than one kernel-argument batch of 96)."""
    g = torch.Generator().manual_seed(5)
    shapes = [(24, 1), (24, 24), (48, 72), (40, 16), (96, 288), (7, 13), (384, 192)] * 8
    ws = [torch.randn(co, ci, 3, 3, generator=g).to(DEV) for co, ci in shapes[:55]]
    many = ops.conv3x3_pack_many(ws, compute)
    for w, (pf, pd) in zip(ws, many):
        rf, rd = ops.conv3x3_pack_lp(w, compute) if compute else ops.conv3x3_pack(w)
        assert torch.equal(pf, rf) and torch.equal(pd, rd), tuple(w.shape)


@pytest.mark.parametrize("N,C,H,W,affine,slope", [(2, 24, 256, 256, True, 0.1), (3, 5, 64, 64, False, 0.01),
                                                      (1, 3, 512, 512, True, 0.1), (2, 2, 300, 304, False, 0.01),
                                                   (2, 7, 32, 32, True, 0.1), (4, 320, 8, 8, False, 0.01),
                                                   (2, 3, 16, 16, True, 0.1), (1, 2, 6, 5, True, 0.1),
                                                   (1, 2, 2, 2, False, 0.01)])
def test_instnorm_lrelu_fwd_bwd(N, C, H, W, affine, slope):
    g = _g(C + H)
    z = torch.randn(N, C, H, W, generator=g) * 3.0 + 1.5
    gamma = (torch.rand(C, generator=g) + 0.5) if affine else None
    beta = (torch.randn(C, generator=g) * 0.3) if affine else None
    dy = torch.randn(N, C, H, W, generator=g)
    zr = z.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True) if affine else None
    br = beta.clone().requires_grad_(True) if affine else None
    y = F.leaky_relu(F.instance_norm(zr, weight=gr, bias=br, eps=1e-5), slope)
    y.backward(dy)
    zd, dyd = z.to(DEV), dy.to(DEV)
    gd, bd = (gamma.to(DEV), beta.to(DEV)) if affine else (None, None)
    yg, mean, rstd = ops.instnorm_lrelu_fwd(zd, gd, bd, 1e-5, slope)
    _close(yg, y.detach(), 1e-5, 2e-5, "in fwd")
    _close(mean.view(N, C), z.mean(dim=(2, 3)), 1e-5, 1e-5, "mean")
    dz, dg, db = ops.instnorm_lrelu_bwd(zd, dyd, mean, rstd, gd, bd, 1e-5, slope)
    _close(dz, zr.grad, 1e-4, 2e-5, "in bwd")
    if affine:
        _close(dg, gr.grad, 1e-4, 1e-3, "dgamma")
        _close(db, br.grad, 1e-4, 1e-3, "dbeta")
    dbp = torch.empty(C, device=DEV)
    dz2, _, _ = ops.instnorm_lrelu_bwd(zd, dyd.clone(), mean, rstd, gd, bd, 1e-5, slope, inplace=True, dbias_pre=dbp)
    assert torch.equal(dz2, dz)                       # in-place form is bit-identical
    # gradient fan-in: dy split into 3 private contributions must give the same dz as their sum
    parts = [torch.randn(N, C, H, W, generator=g) for _ in range(2)]
    first = dy - parts[0] - parts[1]
    dz3, _, _ = ops.instnorm_lrelu_bwd(zd, first.to(DEV), mean, rstd, gd, bd, 1e-5, slope, dy_extra=[p_.to(DEV) for p_ in parts])
    _close(dz3, zr.grad, 1e-4, 3e-5, "in bwd with fan-in extras")
    want = dz.double().sum(dim=(0, 2, 3)).cpu()       # fused conv-bias gradient = sum of the dz it just wrote
    assert (dbp.cpu().double() - want).abs().max().item() <= 1e-5 * dz.abs().sum(dim=(0, 2, 3)).max().item() + 1e-6


@pytest.mark.parametrize("N,Cin,Cout,H,W,k", [(2, 48, 48, 16, 16, 2), (1, 96, 48, 8, 8, 2), (2, 20, 12, 6, 10, 2),
                                               (2, 64, 64, 8, 8, 4), (1, 128, 128, 4, 4, 8), (3, 32, 32, 5, 3, 4),
                                               (3, 40, 6, 8, 16, 2), (2, 100, 52, 16, 8, 2), (5, 48, 48, 32, 32, 2),
                                               (2, 16, 2, 4, 8, 2), (1, 192, 96, 8, 8, 2)])
def test_convT_fwd_dgrad_wgrad(N, Cin, Cout, H, W, k):
    g = _g(Cin + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, k, k, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(N, Cout, H * k, W * k, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, br, stride=k)
    y.backward(dy)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    _close(ops.convT_fwd(xd, wd, bd, k), y.detach(), 2e-5, 2e-5, "convT fwd")
    _close(ops.convT_dgrad(xd, wd, dyd, k), xr.grad, 2e-5, 5e-5, "convT dgrad")
    pre = torch.randn(N, Cin, H, W, generator=g)
    _close(ops.convT_dgrad(xd, wd, dyd, k, dx=pre.to(DEV).clone(), accumulate=True), xr.grad + pre, 2e-5, 5e-5, "convT dgrad acc")
    dw, db = ops.convT_wgrad(xd, wd, dyd, k)
    _close(dw, wr.grad, 1e-4, 2e-5 * max(1.0, wr.grad.abs().max().item()), "convT wgrad")
    _close(db, br.grad, 1e-4, 1e-4 * max(1.0, br.grad.abs().max().item()), "convT dbias")
    if k == 2 and (H * W) % 32 == 0 and W % 8 == 0 and Cout % 2 == 0:
        # 16-bit operand modes of the k == 2 backward kernels (shapes the generic fp32 kernel takes ignore `compute`):
        # the same sums over rounded operands
        for mode, lp in ((1, torch.bfloat16), (2, torch.float16)):
            r = lambda t: t.to(lp).float()
            xq, wq, dq = r(x).requires_grad_(True), r(w).requires_grad_(True), r(dy)
            F.conv_transpose2d(xq, wq, None, stride=k).backward(dq)
            _close(ops.convT_dgrad(xd, wd, dyd, k, compute=mode), xq.grad, 2e-5, 5e-5, f"convT dgrad lp{mode}")
            dwq, _ = ops.convT_wgrad(xd, wd, dyd, k, compute=mode)
            _close(dwq, wq.grad, 1e-4, 2e-5 * max(1.0, wq.grad.abs().max().item()), f"convT wgrad lp{mode}")


def test_dice_multihead_matches_oracle():
    g = _g(9)
    N, H, W = 3, 64, 64
    xs = [torch.randn(N, 1, H, W, generator=g) * 2 for _ in range(4)]
    t = (torch.rand(N, 1, H, W, generator=g) > 0.7).float()
    t[1] = 0                                              # empty mask (class "normal")
    weights = [1 / 4, 1 / 3, 1 / 2, 1.0]
    xr = [x.clone().requires_grad_(True) for x in xs]
    each = [O.dice_loss_sigmoid_sq(x, t) for x in xr]
    total = sum(wi * e for wi, e in zip(weights, each))
    (0.35 * total).backward()
    loss, dxs = ops.dice_multihead([x.to(DEV) for x in xs], t.to(DEV), weights, gscale=0.35)
    loss = loss.cpu()
    for i in range(4):
        assert abs(loss[i].item() - each[i].item()) < 2e-6
        _close(dxs[i], xr[i].grad, 1e-4, 1e-9, f"dice dx head {i}")
    assert abs(loss[4].item() - total.item()) < 5e-6
    # closed form: zero logits, zero target -> 1 - 1/(.25 HW + 1)
    z = torch.zeros(2, 1, 16, 16, device=DEV)
    l0, _ = ops.dice_multihead([z], z.clone(), [1.0])
    assert abs(l0[0].item() - (1 - 1 / (0.25 * 256 + 1))) < 1e-6


def test_focal_matches_reference_goldens(golden_dir):
    import os
    gold = np.load(os.path.join(golden_dir, "focal.npz"))
    t = lambda k: torch.from_numpy(gold[k]).to(DEV)
    l, _ = ops.focal(t("x1"), t("t1"))
    assert abs(l.item() - 0.20617523789405823) < 1e-6          # SURVEY A8 known answer
    l, _ = ops.focal(t("x2"), t("t2"))
    assert abs(l.item() - float(gold["y2"])) < 1e-6
    l, _ = ops.focal(t("x2"), t("t3"))
    assert abs(l.item() - float(gold["y3"])) < 1e-6
    l, _ = ops.focal(t("x2"), t("t2"), weight=t("w"))
    assert abs(l.item() - float(gold["y4"])) < 1e-6
    for tk in ("t2", "t3"):
        x = torch.from_numpy(gold["x2"]).clone().requires_grad_(True)
        (0.65 * O.focal_loss_soft(x, torch.from_numpy(gold[tk]))).backward()
        _, dx = ops.focal(t("x2"), t(tk), gscale=0.65)
        _close(dx, x.grad, 1e-4, 1e-7, "focal dx")


def test_adam_matches_torch():
    g = _g(21)
    n = 10_003 // 4 * 4
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * 10 ** float(e) for e in (-6, -3, 0, -2)]
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-4, eps=1e-4)
    pd, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step, gr in enumerate(grads, start=1):
        pr.grad = gr.clone()
        opt.step()
        ops.adam_step(pd, gr.to(DEV), m, v, lr=1e-4, step=step, eps=1e-4)
        _close(pd, pr.detach(), 0, 2e-7, f"adam step {step}")
    # grad_scale (data-parallel averaging) and zero_grad
    gd = (grads[0] * 8).to(DEV)
    p1, p2 = p0.to(DEV), p0.to(DEV)
    ops.adam_step(p1, gd, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), 1e-4, 1, grad_scale=0.125, zero_grad=True)
    ops.adam_step(p2, grads[0].to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), 1e-4, 1)
    assert torch.allclose(p1, p2, atol=1e-8) and float(gd.abs().max()) == 0.0


def test_dice_counts_exact(golden_dir):
    import os
    from multi_task_breast_cancer_amd.trainer import dice_counts, dice_score_from_counts
    gold = np.load(os.path.join(golden_dir, "dice_score.npz"))
    gt = torch.from_numpy(gold["gt"]).float()
    seg = torch.from_numpy(gold["seg"])
    logits = torch.where(seg, torch.tensor(3.0), torch.tensor(-3.0))
    c = dice_counts(logits.to(DEV), gt.to(DEV))
    assert abs(dice_score_from_counts(c) - float(gold["k_rand"])) < 1e-12
    tp = float((seg & (gt > 0)).sum()); fp = float((seg & (gt == 0)).sum()); fn = float((~seg & (gt > 0)).sum())
    assert c.tolist() == [tp, fp, fn]                                # integer counts: bit-exact
    z = torch.zeros(1, 1, 8, 8, device=DEV)
    assert dice_score_from_counts(dice_counts(z - 1, z)) == 1.0       # empty / empty -> 1 (metrics.py:262-263)


# ------------------------------------------------------------------ full-size properties (BASELINE.json configs[1] shapes)
@pytest.mark.parametrize("compute,tol", [(0, 2e-5), (1, 5e-3)])
@pytest.mark.parametrize("segs,Cout,H", [([24, 24, 48], 24, 256), ([48], 48, 128)])
def test_conv3x3_adjoint_identities_at_bench_size(compute, tol, segs, Cout, H):
    """At N=32 the CPU oracle is too slow to be the checker; the bilinear form is: for y = conv(x; w),
    <y, dz> = <x, dgrad(dz; w)> = <w, wgrad(x, dz)>.  Any indexing / padding / segment bug breaks one of the three.
    (16-bit mode: each side rounds its own operands, so the identities hold to the rounding level only.)"""
    N, W = 32, H
    g = _g(H + Cout)
    xs = [torch.randn(N, c, H, W, generator=g).to(DEV) for c in segs]
    cin = sum(segs)
    w = (torch.randn(Cout, cin, 3, 3, generator=g) * 0.05).to(DEV)
    dz = torch.randn(N, Cout, H, W, generator=g).to(DEV)
    if compute:
        pf, pd = ops.conv3x3_pack_lp(w, compute)
    else:
        pf, pd = ops.conv3x3_pack(w)
    y = ops.conv3x3_fwd(xs, w, None, packed=pf, compute=compute)
    dxs = [torch.zeros_like(x) for x in xs]
    ops.conv3x3_dgrad(dz, w, dxs, [0] * len(xs), packed=pd, compute=compute)
    dw, _ = ops.conv3x3_wgrad(xs, dz, tuple(w.shape), compute=compute)
    s_y = (y.double() * dz.double()).sum().item()
    s_x = sum((x.double() * d.double()).sum().item() for x, d in zip(xs, dxs))
    s_w = (w.double() * dw.double()).sum().item()
    scale = y.double().norm().item() * dz.double().norm().item()
    assert abs(s_y - s_x) < tol * scale and abs(s_y - s_w) < tol * scale, (s_y, s_x, s_w, scale)
    # linearity in x (forward), exact-fp32 mode only: conv(2x) = 2 conv(x) bit for bit (a power of two commutes with RNE)
    if compute == 0:
        y2 = ops.conv3x3_fwd([2.0 * x for x in xs], w, None, packed=pf)
        assert torch.equal(y2, 2.0 * y)


def test_instnorm_and_convT_properties_at_bench_size():
    N, C, H = 32, 24, 256
    g = _g(77)
    z = (torch.randn(N, C, H, H, generator=g) * 3.0 + 1.5).to(DEV)
    y, mean, rstd = ops.instnorm_lrelu_fwd(z, None, None, slope=1.0)   # slope 1: plain instance norm
    m = y.double().mean(dim=(2, 3))
    v = y.double().var(dim=(2, 3), unbiased=False)
    assert m.abs().max().item() < 1e-5 and (v - 1.0).abs().max().item() < 1e-4
    # ConvT k=2: <convT(x; w), dy> = <x, dgrad(dy; w)> = <w, wgrad(x, dy)>
    x = torch.randn(N, 48, 128, 128, generator=g).to(DEV)
    w = (torch.randn(48, 48, 2, 2, generator=g) * 0.1).to(DEV)
    dy = torch.randn(N, 48, 256, 256, generator=g).to(DEV)
    yt = ops.convT_fwd(x, w, None, 2)
    dx = ops.convT_dgrad(x, w, dy, 2)
    dw, _ = ops.convT_wgrad(x, w, dy, 2, want_bias=False)
    s_y = (yt.double() * dy.double()).sum().item()
    s_x = (x.double() * dx.double()).sum().item()
    s_w = (w.double() * dw.double()).sum().item()
    scale = yt.double().norm().item() * dy.double().norm().item()
    assert abs(s_y - s_x) < 2e-5 * scale and abs(s_y - s_w) < 2e-5 * scale, (s_y, s_x, s_w)


@pytest.mark.parametrize("N,Cin,Cmid,R,H,W,k", [(2, 16, 12, 1, 8, 8, 8), (1, 24, 20, 3, 6, 10, 4), (3, 32, 32, 1, 16, 16, 2)])
def test_fused_convT_1x1_head_equals_the_two_layers(N, Cin, Cmid, R, H, W, k):
    """MTnnUNet.py:106-116: ConvTranspose2d(k = s) then Conv2d 1x1, no non-linearity in between == one transposed conv
    with combined weights; forward and every parameter gradient against autograd of the two layers."""
    g = _g(Cin + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    wT = torch.randn(Cin, Cmid, k, k, generator=g) * 0.2
    bT = torch.randn(Cmid, generator=g)
    w1 = torch.randn(R, Cmid, 1, 1, generator=g) * 0.3
    b1 = torch.randn(R, generator=g)
    dout = torch.randn(N, R, H * k, W * k, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, wT, bT, w1, b1)]
    y = F.conv2d(F.conv_transpose2d(leaves[0], leaves[1], leaves[2], stride=k), leaves[3], leaves[4])
    y.backward(dout)
    got = ops.convT_head_fwd_bwd(*(t.to(DEV) for t in (x, wT, bT, w1, b1)), k, dout.to(DEV))
    want = [y.detach()] + [t.grad for t in leaves]
    for name, a, b in zip(("y", "dx", "dwT", "dbT", "dw1", "db1"), got, want):
        _close(a, b, 1e-4, 2e-5 * max(1.0, b.abs().max().item()), "head " + name)


# ------------------------------------------------------------------ 16-bit channel-blocked operands (MTBC_LAYOUT_C8)
def _round16(t, compute):
    return (t.bfloat16() if compute == 1 else t.half()).float()


C8_CASES = [
    (2, [8], 16, 32, 32),
    (1, [24, 48], 24, 40, 64),          # two segments, H not a multiple of the tile
    (2, [24, 24, 24, 48], 24, 16, 32),  # 4 segments, 120 channels: the last 32-channel chunk is ragged
    (3, [16], 40, 16, 16),              # 16-wide geometry, Cout not a multiple of 16
    (5, [32], 80, 8, 8),                # 8x8 geometry: 4 images per block, ragged batch
    (1, [8], 8, 24, 48),                # width not a multiple of 32
    (2, [144], 24, 36, 64),             # >1 chunk, rows not a multiple of 4
    (2, [96, 96], 96, 16, 16),
    (2, [48], 48, 32, 32),
]


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", C8_CASES)
def test_conv3x3_c8_operands(N, segs, Cout, H, W, compute):
    """fwd / dgrad read the SAME rounded values in the SAME MFMA order as the planar 16-bit path -> bit-identical;
    wgrad (another split and tile order) and dbias are checked against fp64 on the rounded operands."""
    g = _g(N * 77 + Cout + H + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    xd = [x.to(DEV) for x in xs]
    wd, bd, dzd = w.to(DEV), b.to(DEV), dz.to(DEV)
    pf, pd = ops.conv3x3_pack_lp(wd, compute)
    x8 = [ops.C8.pack(x, compute) for x in xd]
    dz8 = ops.C8.pack(dzd, compute)

    z_planar = ops.conv3x3_fwd(xd, wd, bd, packed=pf, compute=compute)
    z_c8 = ops.conv3x3_fwd_c8(x8, wd, bd, pf)
    assert torch.equal(z_c8, z_planar), f"fwd differs: {(z_c8 - z_planar).abs().max().item():.3e}"

    pre = [torch.randn(N, c, H, W, generator=g) for c in segs]
    acc = [0] + [1] * (len(segs) - 1)
    d_planar = [p.to(DEV).clone() for p in pre]
    d_c8 = [p.to(DEV).clone() for p in pre]
    ops.conv3x3_dgrad(dzd, wd, d_planar, acc, packed=pd, compute=compute)
    ops.conv3x3_dgrad_c8(dz8, wd, d_c8, acc, pd)
    for i in range(len(segs)):
        assert torch.equal(d_c8[i], d_planar[i]), f"dgrad seg {i} differs"

    xr = _round16(torch.cat(xs, 1), compute).double().requires_grad_(False)
    dzr = _round16(dz, compute).double()
    wref = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wref, padding=1).backward(dzr)
    dw, db = ops.conv3x3_wgrad_c8(x8, dz8, tuple(w.shape), want_bias=True)
    scale = max(1.0, wref.grad.abs().max().item())
    _close(dw, wref.grad.float(), 1e-5, 2e-5 * scale, "wgrad c8")
    dbr = dzr.sum((0, 2, 3)).float()
    _close(db, dbr, 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "dbias c8")
    dw2, db2 = ops.conv3x3_wgrad_c8(x8, dz8, tuple(w.shape), want_bias=False, dw=dw.clone(), accumulate=True)
    _close(dw2, 2 * wref.grad.float(), 1e-5, 4e-5 * scale, "wgrad c8 accumulate")


# shapes that take the wide-block / rolling-row weight-gradient kernel (conv3x3_wgrad_c8w_kernel: Cin >= 64 on maps >= 128 wide)
C8W_CASES = [
    (8, [24, 24, 24], 24, 20, 128),            # image -> XCD block mapping (N % 8 == 0); Cin = 72: a half-empty last input tile; 5 row steps in segments of 2, 2 and 1
    (2, [24, 24, 24, 24, 48], 24, 256, 256),   # 144 -> 24 @256x256: two input-channel blocks (5 + 4 tiles), 64 steps per strip in 16 segments of 4
    (1, [48, 48], 48, 130, 128),               # 48 outputs = 3 tiles in one block; H not a multiple of the 4-row step; one image; 33 steps in 17 segments of 2 (the last: 1)
    (2, [96, 96], 96, 32, 160),                # 2 output-channel blocks x 3 input-channel blocks; 5 strips of 4 segments of 2 steps
    (2, [64], 40, 36, 144),                    # Cout = 40: blocks of 32 + 8 channels; W not a multiple of the 32-column strip; 9 steps in 5 segments of 2 (the last: 1)
    (3, [96, 48, 48], 48, 12, 256),            # 192 -> 48: three input-channel blocks; 3 steps in segments of 2 and 1: no segment fills the ring; N % 8 != 0
]


# ... and the image-tile kernel of the 16 x 16 maps (conv3x3_wgrad_c8i_kernel: Cin >= 64, Cout >= 32)
C8I_CASES = [
    (5, [64], 40, 16, 16),                     # Cout = 40: blocks of 32 + 8 channels; 5 image ranges of one image
    (9, [96, 48, 48], 48, 16, 16),             # three segments, 192 -> 48: three input-channel blocks of 4 tiles; 48 outputs in one block; 9 ranges of one image
    (16, [264], 64, 16, 16),                   # 16.5 input tiles: four blocks, the last tile half empty; 16 ranges of one image
    (3, [72], 96, 16, 16),                     # 4.5 input tiles in one block; 2 output-channel blocks of 48
    (1, [64], 48, 16, 16),                     # ONE image range: without bias / accumulation the blocks store straight into dw (no reduction launch)
]


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", C8W_CASES + C8I_CASES)
def test_conv3x3_wgrad_c8_wide_blocks(N, segs, Cout, H, W, compute):
    """conv3x3_wgrad_c8w_kernel (all output channels x <= 80 input channels per block, rows staged once in an LDS ring, DMA of the
    next rows under the MFMAs) against fp64 on the rounded operands: weight and bias gradient, the no-bias kernel instance,
    accumulation into dw -- ragged rows / columns / channel tiles / batch."""
    g = _g(N * 31 + Cout + H + W + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    dz = torch.randn(N, Cout, H, W, generator=g)
    x8 = [ops.C8.pack(x.to(DEV), compute) for x in xs]
    dz8 = ops.C8.pack(dz.to(DEV), compute)
    xr = _round16(torch.cat(xs, 1), compute).double()
    dzr = _round16(dz, compute).double()
    ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dzr, padding=1).float()
    dbr = dzr.sum((0, 2, 3)).float()
    scale = max(1.0, ref.abs().max().item())
    dw, db = ops.conv3x3_wgrad_c8(x8, dz8, (Cout, Cin, 3, 3), want_bias=True)
    _close(dw, ref, 1e-5, 2e-5 * scale, "wgrad c8w")
    _close(db, dbr, 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "dbias c8w")
    dw1, _ = ops.conv3x3_wgrad_c8(x8, dz8, (Cout, Cin, 3, 3), want_bias=False)
    _close(dw1, ref, 1e-5, 2e-5 * scale, "wgrad c8w (no-bias instance)")
    dw2, _ = ops.conv3x3_wgrad_c8(x8, dz8, (Cout, Cin, 3, 3), want_bias=False, dw=dw1.clone(), accumulate=True)
    _close(dw2, 2 * ref, 1e-5, 4e-5 * scale, "wgrad c8w accumulate")
    again, _ = ops.conv3x3_wgrad_c8(x8, dz8, (Cout, Cin, 3, 3), want_bias=False)
    assert torch.equal(again, dw1), "not deterministic"


# the in-kernel split-K reduction across its tree shapes: (N, segs, Cout, H, W) -> channel blocks x splits / levels, as mtbc_conv3x3_wgrad_plan reports them
FIXUP_CASES = [
    (16, [24], 24, 256, 256),                  # 32 x 32 kernel, ONE channel block, 8192 tiles dealt evenly over 1024 splits: three levels of fan-in 11
    (8, [48], 48, 128, 128),                   # 4 channel blocks x 256 splits (1024 tiles dealt evenly, 4 each): three levels of 7
    (4, [96], 96, 64, 64),                     # 9 channel blocks x 64 splits of 2 tiles (128 tiles: below the 1024 of the even deal): two levels of 8
    (8, [96], 96, 128, 128),                   # wide-block kernel (W = 128, Cin >= 64), 2 x 2 channel blocks: 4 strips x 4 row segments of 8 steps x 8 images = 128 splits, three levels of 6, ragged last group
    (2, [192], 192, 32, 32),                   # 36 channel blocks x 16 splits of one tile: two levels of 4
    (2, [384], 192, 32, 32),                   # 72 channel blocks x 8 splits of 2 tiles: one level
    (8, [24, 24, 24], 24, 256, 256),           # wide-block kernel: 8 strips x 8 row segments of 8 steps x 8 images = 512 splits of image-major leaves (N % 8 == 0), three levels of 8
    (3, [96, 48, 48], 48, 128, 128),           # wide-block kernel, N % 8 != 0: leaf = split; 4 strips x 11 segments of 3 steps (the last: 2) x 3 images = 132 splits, three levels of 6
    (32, [192], 384, 16, 16),                  # image-tile kernel: 24 channel blocks x 8 ranges of 4 images = one level
    (6, [384], 384, 16, 16),                   # image-tile kernel: 6 ranges of one image
    (1, [64], 48, 16, 16),                     # ONE split: with bias / accumulation the single row goes through the top level
]


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", FIXUP_CASES)
def test_conv3x3_wgrad_c8_in_kernel_split_k_reduction(N, segs, Cout, H, W, compute):
    """Round 4: the split-K partials of the channel-blocked weight gradients are summed INSIDE the launch by the last-arriving block of
    each group of rows (mtbc_conv3x3_args.wgrad_sync; conv3x3.hip splitk_fixup) instead of by a reduction launch.  Against fp64 on the
    rounded operands, like the reduction-launch path (which must agree with it to fp32 re-association); bit-identical from run to run
    (sums are taken in row order, not arrival order); with bias, and accumulating into dw; the counter buffer is all zeros afterwards
    (every group's winner resets its counter), so one buffer serves every launch of a stream.  Backward of nn.Conv2d,
    MTUNetPlusPlus.py:47-81 / training_multitask.py:102."""
    g = _g(N * 17 + Cout + H + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    dz = torch.randn(N, Cout, H, W, generator=g)
    x8 = [ops.C8.pack(x.to(DEV), compute) for x in xs]
    dz8 = ops.C8.pack(dz.to(DEV), compute)
    xr = _round16(torch.cat(xs, 1), compute).double()
    dzr = _round16(dz, compute).double()
    ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dzr, padding=1).float()
    dbr = dzr.sum((0, 2, 3)).float()
    scale = max(1.0, ref.abs().max().item())
    shape = (Cout, Cin, 3, 3)
    dw, db = ops.conv3x3_wgrad_c8(x8, dz8, shape, want_bias=True)
    sync = ops.wgrad_sync_buffer(DEV, 4)
    assert int(sync.abs().sum().item()) == 0, "counters not back at zero"
    _close(dw, ref, 1e-5, 2e-5 * scale, "wgrad, in-kernel reduction")
    _close(db, dbr, 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "dbias, in-kernel reduction")
    old, dbo = ops.conv3x3_wgrad_c8(x8, dz8, shape, want_bias=True, in_kernel_reduce=False)
    _close(old, ref, 1e-5, 2e-5 * scale, "wgrad, reduction launch")
    _close(dw, old.cpu(), 1e-5, 1e-5 * scale, "the two reductions agree")
    _close(db, dbo.cpu(), 1e-5, 1e-5 * max(1.0, dbr.abs().max().item()), "the two bias reductions agree")
    for _ in range(3):
        again, dba = ops.conv3x3_wgrad_c8(x8, dz8, shape, want_bias=True)
        assert torch.equal(again, dw) and torch.equal(dba, db), "not deterministic"
    dw1, _ = ops.conv3x3_wgrad_c8(x8, dz8, shape, want_bias=False)
    _close(dw1, ref, 1e-5, 2e-5 * scale, "no-bias instance")
    dw2, _ = ops.conv3x3_wgrad_c8(x8, dz8, shape, want_bias=False, dw=dw1.clone(), accumulate=True)
    _close(dw2, 2 * ref, 1e-5, 4e-5 * scale, "accumulate")
    assert int(sync.abs().sum().item()) == 0, "counters not back at zero"


EXTRA16_CASES = [(2, [24, 24, 24, 24, 24, 24], 24, 256, 256),   # 144->24 @256x256: the bench's widest level-0 node
                 (1, [384, 384, 384], 512, 16, 16),             # K = 1152 x 9: the longest accumulation of the step
                 (16, [24, 24], 24, 256, 256)]                  # enough 16 x 32 tiles for the 8-wave (512-pixel) blocks


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", C8_CASES + EXTRA16_CASES)
def test_conv3x3_16bit_fwd_dgrad_match_fp64_on_rounded_operands(N, segs, Cout, H, W, compute):
    """The oracle of the 16-bit forward / dgrad kernels (channel-blocked AND planar staging): fp64 conv2d / conv2d_input
    on operands rounded (RNE) to the MFMA's 16-bit type -- x and w forward, dz and w backward -- i.e. exact products,
    fp32 accumulation being the only difference.  Tolerance 1e-5 relative to the output scale (fp32 accumulation over
    K <= 10368 terms: ~ sqrt(K) * 2^-24 * |terms|), the standard wgrad_c8 already meets."""
    g = _g(N * 131 + Cout + H + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    xr, wr, dzr = _round16(torch.cat(xs, 1), compute).double(), _round16(w, compute).double(), _round16(dz, compute).double()
    z_ref = F.conv2d(xr, wr, b.double(), padding=1)
    dx_ref = torch.nn.grad.conv2d_input(xr.shape, wr, dzr, padding=1)
    dxs_ref = torch.split(dx_ref, segs, dim=1)

    xd = [x.to(DEV) for x in xs]
    wd, bd, dzd = w.to(DEV), b.to(DEV), dz.to(DEV)
    pf, pd = ops.conv3x3_pack_lp(wd, compute)
    x8 = [ops.C8.pack(x, compute) for x in xd]
    dz8 = ops.C8.pack(dzd, compute)
    zs = z_ref.abs().max().item()
    for name, z in (("c8", ops.conv3x3_fwd_c8(x8, wd, bd, pf)), ("planar", ops.conv3x3_fwd(xd, wd, bd, packed=pf, compute=compute))):
        err = (z.cpu().double() - z_ref).abs().max().item()
        assert err <= 1e-5 * zs, f"fwd {name}: max err {err:.3e} vs scale {zs:.3e}"
    pre = [torch.randn(N, c, H, W, generator=g) for c in segs]
    acc = [0] + [1] * (len(segs) - 1)
    ds = dx_ref.abs().max().item()
    for name in ("c8", "planar"):
        d = [p.to(DEV).clone() for p in pre]
        if name == "c8":
            ops.conv3x3_dgrad_c8(dz8, wd, d, acc, pd)
        else:
            ops.conv3x3_dgrad(dzd, wd, d, acc, packed=pd, compute=compute)
        for i in range(len(segs)):
            want = dxs_ref[i] + (pre[i].double() if acc[i] else 0)
            err = (d[i].cpu().double() - want).abs().max().item()
            assert err <= 1e-5 * max(ds, want.abs().max().item()), f"dgrad {name} seg {i}: max err {err:.3e} vs scale {ds:.3e}"


def test_conv3x3_c8_rejects_what_it_cannot_run():
    from multi_task_breast_cancer_amd import _lib as L
    x = torch.randn(1, 8, 8, 10, generator=_g(1)).to(DEV)      # W % 4 != 0: the fp32 output needs 16-byte rows
    w = torch.randn(8, 8, 3, 3, generator=_g(2)).to(DEV)
    pf, _ = ops.conv3x3_pack_lp(w, 1)
    with pytest.raises(L.MtbcError):
        ops.conv3x3_fwd_c8([ops.C8.pack(x, 1)], w, None, pf)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 48, 48, 16, 16), (3, 24, 24, 8, 12), (1, 64, 40, 16, 8), (2, 16, 8, 4, 8)])
def test_convT_forward_into_channel_blocked_output_equals_planar_then_pack(N, Cin, Cout, H, W, compute):
    g = _g(N + Cin + Cout + H)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cin, Cout, 2, 2, generator=g) * 0.2).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    want = ops.C8.pack(ops.convT_fwd(x, w, b, 2), compute)
    got = ops.convT_fwd_c8(x, w, b, 2, compute)
    assert got.shape == want.shape and torch.equal(got.data, want.data)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W,affine", [(2, 24, 256, 256, True), (3, 8, 64, 64, False), (2, 16, 12, 20, True), (1, 48, 128, 128, True)])
def test_instnorm_16bit_planar_outputs_are_the_rounded_fp32_outputs(N, C, H, W, affine, compute):
    """y16 / dz16 = RNE of the fp32 y / dz bit for bit, the fp32 side results (statistics, parameter gradients) do not
    change, and pack16 of the planes equals pack of the fp32 tensor."""
    g = _g(N + C + H + compute)
    z = (torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV) if affine else None
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV) if affine else None
    dt = torch.bfloat16 if compute == 1 else torch.float16
    y, mean, rstd = ops.instnorm_lrelu_fwd(z, gamma, beta, slope=0.1)
    y16, mean2, rstd2 = ops.instnorm_lrelu_fwd(z, gamma, beta, slope=0.1, out16=compute)
    assert torch.equal(y16.view(dt), y.to(dt)) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    db1, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dz, dg, dbt = ops.instnorm_lrelu_bwd(z, dy, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db1)
    dz16, dg2, dbt2 = ops.instnorm_lrelu_bwd(z, dy, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db2, out16=compute)
    assert torch.equal(dz16.view(dt), dz.to(dt)) and torch.equal(db1, db2)
    if affine:
        assert torch.equal(dg, dg2) and torch.equal(dbt, dbt2)
    if C % 8 == 0:
        assert torch.equal(ops.C8.pack16(y16, compute).data, ops.C8.pack(y, compute).data)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W,affine", [(2, 24, 256, 256, True), (3, 48, 128, 128, True), (2, 96, 64, 64, False),
                                            (5, 16, 32, 32, True), (2, 8, 16, 16, True), (3, 8, 8, 8, False), (32, 24, 256, 256, True),
                                            (4, 24, 512, 512, True)])
def test_cooperative_instnorm_into_channel_blocked_layout(N, C, H, W, affine, compute):
    """The split-plane cooperative kernels (teams of workgroups exchanging partial statistics through a mailbox) against
    the one-plane-per-workgroup kernels: statistics to fp32 re-association, outputs to one 16-bit ulp of the rounded
    fp32 result, parameter gradients to fp32 re-association; launched repeatedly (mailbox epochs) and never giving up
    a poll."""
    g = _g(N + C + H + compute)
    z = (torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV) if affine else None
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV) if affine else None
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    y, mean, rstd = ops.instnorm_lrelu_fwd(z, gamma, beta, slope=0.1)
    for rep in range(3):
        y8, mean2, rstd2, yp = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1, compute=compute, want_planar=rep == 1)
    assert torch.allclose(mean2, mean, rtol=1e-5, atol=1e-6) and torch.allclose(rstd2, rstd, rtol=1e-5, atol=1e-6)
    got = y8.unpack()
    assert bool(((got - y).abs() <= ulp * y.abs() + 1e-5).all()), (got - y).abs().max().item()
    db1, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dz, dg, dbt = ops.instnorm_lrelu_bwd(z, dy, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db1)
    for rep in range(2):
        dz8, dg2, dbt2 = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db2, compute=compute)
    gotz = dz8.unpack()
    scale = dz.abs().max().item()
    assert bool(((gotz - dz).abs() <= ulp * dz.abs() + 2e-6 * scale).all()), (gotz - dz).abs().max().item()
    # the bias gradient of a conv in front of InstanceNorm is mathematically zero: both kernels return the rounding noise
    # of a sum over N*H*W terms, which scales with the sum of |dz|
    noise = 1e-6 * dz.abs().sum((0, 2, 3)).max().item()
    assert (db2 - db1).abs().max().item() <= max(1e-3, noise)
    if affine:
        assert torch.allclose(dg2, dg, rtol=1e-4, atol=1e-3 * max(1.0, dg.abs().max().item()))
        assert torch.allclose(dbt2, dbt, rtol=1e-4, atol=1e-3 * max(1.0, dbt.abs().max().item()))
    assert ops.coop_error(DEV) == 0


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 48, 48, 16, 16), (3, 24, 24, 8, 12), (1, 64, 40, 16, 8), (2, 96, 48, 8, 8),
                                            (2, 384, 192, 4, 8), (1, 512, 512, 8, 4), (2, 16, 8, 4, 8)])
def test_convT_forward_on_the_16bit_mfma_with_channel_blocked_tensors(N, Cin, Cout, H, W, compute):
    """x and w rounded to the 16-bit type, fp32 accumulation, bias, ONE rounding of the result: against fp64 on the
    rounded operands, to one 16-bit ulp."""
    g = _g(N + Cin + Cout + H + compute)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 2, 2, generator=g) * (1.0 / Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    want = F.conv_transpose2d(_round16(x, compute).double(), _round16(w, compute).double(), b.double(), stride=2).float()
    got = ops.convT_fwd_c8_lp(ops.C8.pack(x.to(DEV), compute), w.to(DEV), b.to(DEV), 2).unpack().cpu()
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    assert bool(((got - want).abs() <= ulp * want.abs() + 1e-5).all()), (got - want).abs().max().item()


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W", [(2, 24, 256, 256), (3, 8, 16, 24), (1, 48, 32, 32), (2, 16, 64, 16)])
def test_maxpool_on_channel_blocked_tensors(N, C, H, W, compute):
    """forward == fp32 pool of the stored values, re-packed, bit for bit; backward == the fp32 kernel run on the stored
    (unpacked) values, bit for bit, overwrite and accumulate (ties of rounded values included: the test data has many)."""
    g = _g(N + C + H + compute)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    x8 = ops.C8.pack(x, compute)
    xs = x8.unpack()                                         # the stored values
    y8 = ops.maxpool2_fwd_c8(x8)
    want = ops.C8.pack(ops.maxpool2_fwd(xs), compute)
    assert y8.shape == want.shape and torch.equal(y8.data, want.data)
    assert torch.equal(y8.data, ops.C8.pack(ops.maxpool2_fwd(x), compute).data)      # max commutes with the rounding
    dy = torch.randn(N, C, H // 2, W // 2, generator=g).to(DEV)
    assert torch.equal(ops.maxpool2_bwd_c8(x8, dy), ops.maxpool2_bwd(xs, dy))
    pre = torch.randn(N, C, H, W, generator=g).to(DEV)
    assert torch.equal(ops.maxpool2_bwd_c8(x8, dy, dx=pre.clone(), accumulate=True), ops.maxpool2_bwd(xs, dy, dx=pre.clone(), accumulate=True))
    # a window with a tie among its rounded maxima, first-maximum routing checked explicitly
    t = torch.zeros(1, 8, 8, 8, device=DEV)
    t[0, :, 0, 1] = 1.0; t[0, :, 1, 0] = 1.0 + 2.0 ** -12        # both round to 1.0 in bf16 AND fp16: (0,1) comes first
    g1 = ops.maxpool2_bwd_c8(ops.C8.pack(t, compute), torch.ones(1, 8, 4, 4, device=DEV))
    assert g1[0, 0, 0, 1].item() == 1.0 and g1[0, 0, 1, 0].item() == 0.0


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 24, 1, 256, 256), (3, 16, 1, 32, 32), (2, 24, 3, 64, 48), (1, 64, 8, 16, 16)])
def test_conv1x1_head_on_channel_blocked_input(N, Cin, Cout, H, W, compute):
    """forward == the fp32 1x1 kernel on the stored values bit for bit (same fmaf chain); weight / bias gradient against
    fp64 on the stored values (another summation order)."""
    g = _g(N + Cin + Cout + H + compute)
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.3).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    dy = torch.randn(N, Cout, H, W, generator=g).to(DEV)
    x8 = ops.C8.pack(x, compute)
    xs = x8.unpack()
    assert torch.equal(ops.conv1x1_fwd_c8(x8, w, b), ops.conv1x1_fwd(xs, w, b))
    dw, db = ops.conv1x1_wgrad_c8(x8, w, dy)
    wr = torch.zeros(Cout, Cin, 1, 1, dtype=torch.float64, requires_grad=True)
    F.conv2d(xs.cpu().double(), wr).backward(dy.cpu().double())
    _close(dw, wr.grad.float(), 1e-5, 2e-5 * max(1.0, wr.grad.abs().max().item()), "conv1x1 c8 wgrad")
    dbr = dy.cpu().double().sum((0, 2, 3)).float()
    _close(db, dbr, 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "conv1x1 c8 dbias")
    dw2, db2 = ops.conv1x1_wgrad_c8(x8, w, dy, accumulate=True, dw=dw.clone(), db=db.clone())
    _close(dw2, 2 * wr.grad.float(), 1e-5, 4e-5 * max(1.0, wr.grad.abs().max().item()), "conv1x1 c8 wgrad accumulate")
    _close(db2, 2 * dbr, 1e-5, 4e-5 * max(1.0, dbr.abs().max().item()), "conv1x1 c8 dbias accumulate")


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", [(2, [24, 48], 24, 40, 64), (2, [48], 24, 256, 256), (3, [16, 16], 40, 16, 16), (5, [32, 8], 80, 8, 8)])
def test_conv3x3_dgrad_into_16bit_planar_segment(N, segs, Cout, H, W, compute):
    """mtbc_seg.accumulate = 2: the LAST dx segment is written as 16-bit planes = the fp32 result of the same launch rounded
    to nearest even, bit for bit; the other segments are untouched by the mode."""
    g = _g(N + Cout + H + compute)
    Cin = sum(segs)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    dz8 = ops.C8.pack(torch.randn(N, Cout, H, W, generator=g).to(DEV), compute)
    _, pd = ops.conv3x3_pack_lp(w, compute)
    ref = [torch.zeros(N, c, H, W, device=DEV) for c in segs]
    ops.conv3x3_dgrad_c8(dz8, w, ref, [0] * len(segs), pd)
    got = [torch.zeros(N, c, H, W, device=DEV) for c in segs[:-1]] + [torch.zeros(N, segs[-1], H, W, dtype=torch.int16, device=DEV)]
    ops.conv3x3_dgrad_c8(dz8, w, got, [0] * (len(segs) - 1) + [2], pd)
    dt = torch.bfloat16 if compute == 1 else torch.float16
    for a, b in zip(got[:-1], ref[:-1]):
        assert torch.equal(a, b)
    assert torch.equal(got[-1].view(dt), ref[-1].to(dt))


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 48, 48, 32, 32), (3, 96, 48, 8, 16), (1, 384, 192, 8, 8), (2, 48, 24, 16, 8), (2, 56, 40, 16, 16),
                                            (2, 512, 256, 8, 8), (32, 96, 48, 64, 64), (2, 24, 12, 16, 16)])
def test_convT_backward_reads_16bit_planar_dy(N, Cin, Cout, H, W, compute):
    """dy_type16: the k = 2 ConvT dgrad / wgrad on a 16-bit planar dy must equal the same kernels fed the fp32 tensor with
    the same (representable) values, bit for bit -- they rounded an fp32 dy to exactly these operands while loading it."""
    g = _g(N + Cin + Cout + H + compute)
    dt = torch.bfloat16 if compute == 1 else torch.float16
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cin, Cout, 2, 2, generator=g) * 0.1).to(DEV)
    dy16 = torch.randn(N, Cout, 2 * H, 2 * W, generator=g).to(DEV).to(dt)
    dy = dy16.float()
    dy16i = dy16.view(torch.int16)
    dx_ref = ops.convT_dgrad(x, w, dy, 2, compute=compute)
    dx = ops.convT_dgrad(x, w, dy16i, 2, compute=compute, dy16=True)
    assert torch.equal(dx, dx_ref)
    pre = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    assert torch.equal(ops.convT_dgrad(x, w, dy16i, 2, dx=pre.clone(), accumulate=True, compute=compute, dy16=True),
                       ops.convT_dgrad(x, w, dy, 2, dx=pre.clone(), accumulate=True, compute=compute))
    dw_ref, db_ref = ops.convT_wgrad(x, w, dy, 2, compute=compute)
    dw, db = ops.convT_wgrad(x, w, dy16i, 2, compute=compute, dy16=True)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    # and against fp64 on the rounded operands (the oracle of the mode)
    r = lambda t: t.to(dt).double()
    want = F.conv2d(dy.cpu().double(), r(w.cpu()), stride=2)
    assert (dx.cpu().double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", C8_CASES + [(2, [24, 24, 24, 24, 24, 24], 24, 256, 256), (16, [24, 24], 24, 256, 256),
                                                        (1, [384, 384, 384], 512, 16, 16), (2, [192], 192, 32, 32)])
def test_conv3x3_channel_blocked_16bit_output_is_the_rounded_fp32_output(N, segs, Cout, H, W, compute):
    """out_layout = C8 (forward) / segment mode 3 (dgrad): the conv output / input gradient of the 16-bit modes stored as a
    channel-blocked 16-bit tensor = the fp32 planar result of the same launch, + bias, rounded once (RNE) -- the MFMAs only
    run transposed (channels on the rows)."""
    if Cout % 8:
        pytest.skip("channel-blocked outputs hold multiples of 8 channels")
    g = _g(N * 53 + Cout + H + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    xd = [x.to(DEV) for x in xs]
    wd, bd, dzd = w.to(DEV), b.to(DEV), dz.to(DEV)
    pf, pd = ops.conv3x3_pack_lp(wd, compute)
    x8 = [ops.C8.pack(x, compute) for x in xd]
    dz8 = ops.C8.pack(dzd, compute)
    z = ops.conv3x3_fwd_c8(x8, wd, bd, pf)
    z8 = ops.conv3x3_fwd_c8(x8, wd, bd, pf, out_c8=True)
    assert z8.data.shape == (N, Cout // 8, H * W, 8)
    want = ops.C8.pack(z, compute)
    assert torch.equal(z8.data, want.data), f"fwd: {(z8.unpack() - want.unpack()).abs().max().item():.3e}"
    if all(c % 8 == 0 for c in segs):
        d32 = [torch.empty(N, c, H, W, device=DEV) for c in segs]
        ops.conv3x3_dgrad_c8(dz8, wd, d32, [0] * len(segs), pd)
        d8 = [ops.C8(torch.empty(N, c // 8, H * W, 8, dtype=torch.int16, device=DEV), (N, c, H, W), compute) for c in segs]
        ops.conv3x3_dgrad_c8(dz8, wd, d8, [3] * len(segs), pd)
        for i in range(len(segs)):
            assert torch.equal(d8[i].data, ops.C8.pack(d32[i], compute).data), f"dgrad seg {i}"


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W,affine", [(2, 24, 256, 256, True), (3, 48, 128, 128, True), (2, 96, 64, 64, False), (5, 16, 32, 32, True),
                                            (2, 8, 16, 16, True), (3, 8, 8, 8, False), (2, 16, 24, 40, True), (1, 24, 96, 96, True)])
def test_instnorm_on_channel_blocked_16bit_inputs(N, C, H, W, affine, compute):
    """z_layout / dy_layout = C8: InstanceNorm + LeakyReLU forward / backward reading the conv output (and the gradient)
    as 16-bit channel-blocked tensors = the same kernels on the unpacked fp32 planes (the statistics are those of the stored
    values): bit for bit where one workgroup owns a plane group; the cooperative kernels may split a plane differently per
    variant (team size follows the variant's register count), so there to fp32 re-association / one 16-bit ulp.  A planar
    fp32 partial gradient (dy_extra) is added in fp32 while loading."""
    g = _g(N + C + H + 7 * compute)
    z = (torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV)
    ex = torch.randn(N, C, H, W, generator=g).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV) if affine else None
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV) if affine else None
    z8, dy8 = ops.C8.pack(z, compute), ops.C8.pack(dy, compute)
    zr, dyr = z8.unpack(), dy8.unpack()
    ya, mean_a, rstd_a, ypa = ops.instnorm_lrelu_fwd_c8(zr, gamma, beta, slope=0.1, compute=compute, want_planar=True)
    yb, mean_b, rstd_b, ypb = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, want_planar=True)
    solo = H * W <= 4096
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10

    def same8(a8, b8, exact=solo):
        if exact:
            return torch.equal(a8.data, b8.data)
        a_, b_ = a8.unpack(), b8.unpack()
        return bool(((a_ - b_).abs() <= ulp * b_.abs() + 2e-6 * b_.abs().max()).all())

    def same(a_, b_):
        return torch.equal(a_, b_) if solo else torch.allclose(a_, b_, rtol=1e-5, atol=1e-5 * max(1.0, b_.abs().max().item()))

    assert same(mean_a, mean_b) and same(rstd_a, rstd_b)
    assert same8(ya, yb) and same(ypa, ypb)
    # ... and they ARE the statistics of the stored values
    ref_mean = zr.double().mean((2, 3)).reshape(-1)
    assert torch.allclose(mean_b.double(), ref_mean, rtol=1e-5, atol=1e-5)
    for extra in (None, ex):
        db1, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        da, dga, dba = ops.instnorm_lrelu_bwd_c8(zr, dyr + (extra if extra is not None else 0), mean_b, rstd_b, gamma, beta, slope=0.1, dbias_pre=db1, compute=compute)
        db, dgb, dbb = ops.instnorm_lrelu_bwd_c8(z8, dy8, mean_b, rstd_b, gamma, beta, slope=0.1, dbias_pre=db2, dy_extra=extra)
        # (backward: the variants are separate instantiations whose fused multiply-adds may be contracted differently)
        assert same8(da, db, False), (da.unpack() - db.unpack()).abs().max().item()
        noise = 1e-6 * da.unpack().abs().sum((0, 2, 3)).max().item()
        assert (db1 - db2).abs().max().item() <= max(1e-3, noise)
        if affine:
            assert torch.allclose(dga, dgb, rtol=1e-4, atol=1e-3 * max(1.0, dga.abs().max().item())) and torch.allclose(dba, dbb, rtol=1e-4, atol=1e-3 * max(1.0, dba.abs().max().item()))
    # mixed: channel-blocked z with a planar fp32 gradient
    dc, _, _ = ops.instnorm_lrelu_bwd_c8(z8, dyr, mean_b, rstd_b, gamma, beta, slope=0.1)
    dd, _, _ = ops.instnorm_lrelu_bwd_c8(zr, dyr, mean_b, rstd_b, gamma, beta, slope=0.1, compute=compute)
    assert same8(dc, dd, False)
    assert ops.coop_error(DEV) == 0


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", [(2, [24], 24, 256, 256), (16, [24, 24], 24, 256, 256), (2, [48], 48, 128, 128), (3, [16], 40, 16, 16),
                                             (5, [32], 80, 8, 8), (2, [96, 96], 96, 16, 16), (1, [24, 48], 24, 40, 64), (2, [8], 16, 36, 64)])
def test_instnorm_statistics_from_the_conv_epilogue(N, segs, Cout, H, W, compute):
    """mtbc_conv3x3_args.stats_partial: the forward conv's epilogue leaves {sum, sum of squares} of its STORED (rounded)
    outputs per image, pixel subset and channel; summed they are the plane sums of the stored tensor, and the InstanceNorm
    forward fed with them (finalize + one streaming pass) equals the channel-group kernels that reduce the tensor
    themselves: statistics to fp32 re-association, outputs to one 16-bit ulp."""
    g = _g(N * 19 + Cout + H + compute)
    Cin = sum(segs)
    xs = [(torch.randn(N, c, H, W, generator=g) + 0.3).to(DEV) for c in segs]
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(DEV), (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    pf, _ = ops.conv3x3_pack_lp(w, compute)
    x8 = [ops.C8.pack(x, compute) for x in xs]
    z8, part = ops.conv3x3_fwd_c8(x8, w, b, pf, out_c8=True, stats=True)
    assert torch.equal(z8.data, ops.conv3x3_fwd_c8(x8, w, b, pf, out_c8=True).data)      # the statistics change nothing else
    assert not torch.isnan(part).any(), "a (image, subset, channel) entry was not written"
    zr = z8.unpack().double()
    tot = part.double().sum(1)                                                            # (N, Cout, 2)
    s_ref, q_ref = zr.sum((2, 3)), (zr * zr).sum((2, 3))
    assert torch.allclose(tot[..., 0].cpu(), s_ref.cpu(), rtol=1e-5, atol=1e-5 * q_ref.abs().max().item() ** 0.5 * H * W ** 0.5)
    assert torch.allclose(tot[..., 1].cpu(), q_ref.cpu(), rtol=1e-5, atol=1e-3)
    ya, mean_a, rstd_a, ypa = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, want_planar=True)
    yb, mean_b, rstd_b, ypb = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, want_planar=True, stats=part)
    assert torch.allclose(mean_a, mean_b, rtol=1e-5, atol=1e-5) and torch.allclose(rstd_a, rstd_b, rtol=2e-5, atol=1e-6)
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    ua, ub = ya.unpack(), yb.unpack()
    assert bool(((ua - ub).abs() <= ulp * ua.abs() + 1e-5).all()), (ua - ub).abs().max().item()
    assert torch.allclose(ypa, ypb, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("N,K,C,H,W,affine", [(2, 48, 24, 256, 256, True), (2, 96, 48, 128, 128, True), (3, 96, 96, 64, 64, False), (2, 40, 16, 16, 16, True),
                                              (5, 32, 80, 8, 8, False), (1, 72, 24, 40, 64, True), (2, 192, 192, 32, 32, True)])
def test_gathered_dgrad_prepares_the_instnorm_backward(N, K, C, H, W, affine, extra, compute):
    """mtbc_conv3x3_args.norm_z / out_partial: a forward-type launch over the consumers' dz (the gathered dgrad) writes the
    tensor's gradient once in 16 bits -- its fp32 sum plus the other readers' fp32 partial, one RNE -- and leaves the two
    reductions of the InstanceNorm + LeakyReLU backward in stats_partial; the backward fed with them (finalize + one streaming
    pass) equals the channel-group kernel that reduces the tensors itself."""
    g = _g(N * 23 + K + C + H + compute)
    dzs = ops.C8.pack((torch.randn(N, K, H, W, generator=g)).to(DEV), compute)             # the consumers' dz, side by side
    wg = (torch.randn(C, K, 3, 3, generator=g) * (2.0 / (9 * K)) ** 0.5).to(DEV)             # their gathered weights
    z8 = ops.C8.pack((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV), compute)      # the tensor's own conv output
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV) if affine else None
    beta = (torch.randn(C, generator=g) * 0.1).to(DEV) if affine else None
    ex = torch.randn(N, C, H, W, generator=g).to(DEV) if extra else None
    pf, _ = ops.conv3x3_pack_lp(wg, compute)
    _, mean, rstd, _ = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1)
    dy32 = ops.conv3x3_fwd_c8([dzs], wg, None, pf)                                           # fp32 planar result of the same launch
    dy8, part = ops.conv3x3_fwd_c8([dzs], wg, None, pf, out_c8=True, norm=(z8, mean, rstd, gamma, beta, 0.1), out_partial=ex)
    want8 = ops.C8.pack(dy32 + ex if extra else dy32, compute)
    assert torch.equal(dy8.data, want8.data)
    assert not torch.isnan(part).any()
    # the reductions, recomputed from the stored tensors
    zr, dyr = z8.unpack().double(), dy8.unpack().double()
    xh = (zr - mean.double().view(N, C, 1, 1)) * rstd.double().view(N, C, 1, 1)
    pre = xh * (gamma.double().view(1, C, 1, 1) if affine else 1.0) + (beta.double().view(1, C, 1, 1) if affine else 0.0)
    gg = dyr * torch.where(pre > 0, 1.0, 0.1)
    tot = part.double().sum(1)
    s1, s2 = gg.sum((2, 3)), (gg * xh).sum((2, 3))
    scale = gg.abs().sum((2, 3)).max().item()
    assert (tot[..., 0] - s1).abs().max().item() <= 1e-5 * scale and (tot[..., 1] - s2).abs().max().item() <= 3e-5 * scale * max(1.0, xh.abs().max().item())
    db1, db2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    da, dga, dba = ops.instnorm_lrelu_bwd_c8(z8, dy8, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db1)
    db, dgb, dbb = ops.instnorm_lrelu_bwd_c8(z8, dy8, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db2, stats=part)
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    ua, ub = da.unpack(), db.unpack()
    assert bool(((ua - ub).abs() <= ulp * ua.abs() + 2e-6 * ua.abs().max()).all()), (ua - ub).abs().max().item()
    assert torch.equal(db2, torch.zeros_like(db2))                     # a conv bias in front of a norm: its gradient IS zero
    if affine:
        assert torch.allclose(dga, dgb, rtol=1e-4, atol=1e-3 * max(1.0, dga.abs().max().item()))
        assert torch.allclose(dba, dbb, rtol=1e-4, atol=1e-3 * max(1.0, dba.abs().max().item()))


BF16_OUT_FP16_CASES = [(2, [24], 24, 256, 256), (2, [48], 48, 128, 128), (3, [96], 96, 64, 64), (2, [96, 96], 96, 16, 16), (5, [32], 80, 8, 8)]


@pytest.mark.parametrize("N,segs,Cout,H,W", BF16_OUT_FP16_CASES)
def test_bf16_mode_conv_output_stored_as_fp16(N, segs, Cout, H, W):
    """out_type = 2 / z_type = 2: in the bf16 mode the conv output z is stored as fp16 (same 2 bytes, 11 significant bits,
    saturated at +-65504) while the MFMA operands and the activation stay bf16: the stored tensor = the fp32 planar result of the
    same launch, clamped and rounded once to fp16; its InstanceNorm (statistics from the epilogue, and the channel-group kernels
    in both directions) = the same kernels fed with that fp16 tensor unpacked to fp32 planes."""
    g = _g(N * 29 + Cout + H)
    Cin = sum(segs)
    xs = [(torch.randn(N, c, H, W, generator=g) + 0.2).to(DEV) for c in segs]
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    b[0] = 1.0e5                                          # one channel past the fp16 range: it must saturate, not overflow
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(DEV), (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    pf, _ = ops.conv3x3_pack_lp(w, 1)
    x8 = [ops.C8.pack(x, 1) for x in xs]
    z32 = ops.conv3x3_fwd_c8(x8, w, b, pf)
    z8, part = ops.conv3x3_fwd_c8(x8, w, b, pf, out_c8=True, out_fp16=True, stats=True)
    assert z8.compute == 2
    want = ops.C8.pack(z32.clamp(-65504.0, 65504.0), 2)
    assert torch.equal(z8.data, want.data)
    zr = z8.unpack()
    assert bool(torch.isfinite(zr).all()) and zr[:, 0].abs().max().item() == 65504.0
    tot = part.double().sum(1)
    assert torch.allclose(tot[..., 0].cpu(), zr.double().sum((2, 3)).cpu(), rtol=1e-5, atol=1e-2)
    # InstanceNorm forward: statistics from the epilogue, bf16 activation
    y_a, mean_a, rstd_a, _ = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, compute=1, stats=part)
    y_b, mean_b, rstd_b, _ = ops.instnorm_lrelu_fwd_c8(zr, gamma, beta, slope=0.1, compute=1)
    y_c, mean_c, rstd_c, _ = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, compute=1)
    assert y_a.compute == 1
    for m_, r_, y_ in ((mean_a, rstd_a, y_a), (mean_c, rstd_c, y_c)):
        assert torch.allclose(m_[Cout > 1:], mean_b[Cout > 1:], rtol=1e-5, atol=1e-3) and torch.allclose(r_, rstd_b, rtol=3e-5, atol=1e-7)
        ua, ub = y_.unpack(), y_b.unpack()
        assert bool(((ua - ub).abs() <= 2.0 ** -7 * ub.abs() + 1e-5).all()), (ua - ub).abs().max().item()
    # backward: fp16 z, fp32 planar dy (the default plan) and bf16 channel-blocked dy
    dy = torch.randn(N, Cout, H, W, generator=g).to(DEV)
    dz_a, _, _ = ops.instnorm_lrelu_bwd_c8(z8, dy, mean_b, rstd_b, gamma, beta, slope=0.1, compute=1)
    dz_b, _, _ = ops.instnorm_lrelu_bwd_c8(zr, dy, mean_b, rstd_b, gamma, beta, slope=0.1, compute=1)
    dy8 = ops.C8.pack(dy, 1)
    dz_c, _, _ = ops.instnorm_lrelu_bwd_c8(z8, dy8, mean_b, rstd_b, gamma, beta, slope=0.1)
    dz_d, _, _ = ops.instnorm_lrelu_bwd_c8(zr, dy8.unpack(), mean_b, rstd_b, gamma, beta, slope=0.1, compute=1)
    for a_, b_ in ((dz_a, dz_b), (dz_c, dz_d)):
        assert a_.compute == 1
        ua, ub = a_.unpack(), b_.unpack()
        assert bool(((ua - ub).abs() <= 2.0 ** -7 * ub.abs() + 2e-6 * ub.abs().max()).all()), (ua - ub).abs().max().item()


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W,with_dy", [(2, 24, 256, 256, True), (2, 24, 256, 256, False), (3, 48, 64, 64, True), (2, 16, 16, 16, False), (1, 24, 96, 96, True)])
def test_instnorm_backward_forms_the_rank1_head_gradient(N, C, H, W, with_dy, compute):
    """mtbc_instnorm_args.dy_rank1 / dy_rank1_w: the input gradient of a one-output 1x1 head, w[c] * dyhead[n, pixel], is formed
    inside the InstanceNorm backward = the same backward with that tensor written out and added to dy (or standing for a dy
    nothing else wrote)."""
    g = _g(N + C + H + 3 * compute)
    z = ops.C8.pack((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV), compute)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV) if with_dy else None
    dyh = torch.randn(N, 1, H, W, generator=g).to(DEV)
    wh = torch.randn(C, generator=g).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    _, mean, rstd, _ = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1)
    full = wh.view(1, C, 1, 1) * dyh + (dy if with_dy else 0)
    db1, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    a_, dga, dba = ops.instnorm_lrelu_bwd_c8(z, full.contiguous(), mean, rstd, gamma, beta, slope=0.1, dbias_pre=db1, compute=compute)
    b_, dgb, dbb, hdw, hdb = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, dbias_pre=db2, compute=compute, rank1=(dyh, wh),
                                                       rank1_grads=True)
    # ... and the head's own gradients: the weight gradient contracts the STORED activation (what the head's forward read)
    y8, _, _, _ = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1, compute=compute)
    yr = y8.unpack().double()
    dw_ref = (yr * dyh.double()).sum((0, 2, 3))
    assert torch.allclose(hdw.double(), dw_ref, rtol=2e-4, atol=2e-4 * max(1.0, dw_ref.abs().max().item())), (hdw.double() - dw_ref).abs().max().item()
    assert abs(hdb.item() - dyh.double().sum().item()) <= 1e-4 * max(1.0, dyh.abs().sum().item() ** 0.5 * 10)
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    ua, ub = a_.unpack(), b_.unpack()
    assert bool(((ua - ub).abs() <= ulp * ua.abs() + 2e-6 * ua.abs().max()).all()), (ua - ub).abs().max().item()
    assert torch.allclose(dga, dgb, rtol=1e-4, atol=1e-3 * max(1.0, dga.abs().max().item()))
    assert torch.allclose(dba, dbb, rtol=1e-4, atol=1e-3 * max(1.0, dba.abs().max().item()))


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,C,H,W,with_dy", [(2, 24, 256, 256, True), (2, 48, 128, 128, False), (3, 96, 64, 64, True), (2, 16, 16, 16, False), (1, 24, 96, 80, True)])
def test_instnorm_backward_routes_the_maxpool_gradient(N, C, H, W, with_dy, compute):
    """mtbc_maxpool_args.argmax + mtbc_instnorm_args.dy_pool: the backward of MaxPool2d(2,2) formed inside the InstanceNorm
    backward of the tensor it pooled = the pool's own backward kernel writing its fp32 tensor, added to dy (or standing for a dy
    nothing else wrote).  Ties included (equal activations in a window: the FIRST maximum gets the gradient)."""
    g = _g(N + C + H + 5 * compute)
    z = ops.C8.pack((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV), compute)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    y8, mean, rstd, _ = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1)
    yp8, arg = ops.maxpool2_fwd_c8(y8, want_argmax=True)
    assert torch.equal(yp8.data, ops.maxpool2_fwd_c8(y8).data)
    dyp = torch.randn(N, C, H // 2, W // 2, generator=g).to(DEV)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV) if with_dy else None
    routed = ops.maxpool2_bwd_c8(y8, dyp)                                     # the pool's own backward (fp32 planar, 3/4 zeros)
    assert int((routed != 0).sum()) <= dyp.numel()
    full = routed + dy if with_dy else routed
    a_, dga, dba = ops.instnorm_lrelu_bwd_c8(z, full.contiguous(), mean, rstd, gamma, beta, slope=0.1, compute=compute)
    b_, dgb, dbb = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, compute=compute, pool=(dyp, arg))
    ulp = 2.0 ** -7 if compute == 1 else 2.0 ** -10
    ua, ub = a_.unpack(), b_.unpack()
    assert bool(((ua - ub).abs() <= ulp * ua.abs() + 2e-6 * ua.abs().max()).all()), (ua - ub).abs().max().item()
    assert torch.allclose(dga, dgb, rtol=1e-4, atol=1e-3 * max(1.0, dga.abs().max().item()))
    assert torch.allclose(dba, dbb, rtol=1e-4, atol=1e-3 * max(1.0, dba.abs().max().item()))


@pytest.mark.parametrize("N,C,H,W", [(2, 48, 128, 128), (3, 96, 64, 64), (2, 16, 16, 16)])
def test_instnorm_backward_adds_a_second_planar_gradient(N, C, H, W):
    """fp32 planar dy + n_dy_extra = 1: the gathered dgrad's own output buffer added while loading = the backward of the sum."""
    g = _g(N + C + H)
    z = ops.C8.pack((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV), 2)
    dy, ex = torch.randn(N, C, H, W, generator=g).to(DEV), torch.randn(N, C, H, W, generator=g).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    _, mean, rstd, _ = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1, compute=1)
    a_, _, _ = ops.instnorm_lrelu_bwd_c8(z, (dy + ex).contiguous(), mean, rstd, gamma, beta, slope=0.1, compute=1)
    b_, _, _ = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, compute=1, dy_extra=ex)
    ua, ub = a_.unpack(), b_.unpack()
    assert bool(((ua - ub).abs() <= 2.0 ** -7 * ua.abs() + 2e-6 * ua.abs().max()).all()), (ua - ub).abs().max().item()


STEM16_CASES = [(2, 24, 256, 256), (3, 32, 40, 24), (1, 8, 8, 12), (2, 24, 96, 96)]          # (N, Cout, H, W)


@pytest.mark.parametrize("compute,out_fp16", [(1, True), (1, False), (2, False)])
@pytest.mark.parametrize("N,Cout,H,W", STEM16_CASES)
def test_stem_conv_on_the_16bit_path(N, Cout, H, W, compute, out_fp16):
    """The 1-channel stem in the 16-bit modes: fp32 operands and the stem kernel's fmaf order, output channel-blocked 16-bit
    (= the fp32 stem output, clamped for fp16 storage, rounded once) + InstanceNorm statistics of the stored values; its weight
    gradient from a channel-blocked dz = the fp32 weight-gradient kernel on the unpacked dz."""
    g = _g(N + Cout + H + compute)
    x = (torch.rand(N, 1, H, W, generator=g) * 255.0).to(DEV)
    w = (torch.randn(Cout, 1, 3, 3, generator=g) * 0.05).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    z32 = ops.conv3x3_fwd([x], w, b)
    z8, part = ops.conv3x3_stem_fwd_c8(x, w, b, compute, out_fp16=out_fp16, stats=True)
    t = 2 if out_fp16 else compute
    want = ops.C8.pack(z32.clamp(-65504.0, 65504.0) if t == 2 else z32, t)
    assert z8.compute == t and torch.equal(z8.data, want.data)
    assert not torch.isnan(part).any()
    zr = z8.unpack().double()
    tot = part.double().sum(1)
    assert torch.allclose(tot[..., 0].cpu(), zr.sum((2, 3)).cpu(), rtol=1e-5, atol=1e-2)
    assert torch.allclose(tot[..., 1].cpu(), (zr * zr).sum((2, 3)).cpu(), rtol=1e-5, atol=1e-1)
    dz = torch.randn(N, Cout, H, W, generator=g).to(DEV)
    dz8 = ops.C8.pack(dz, compute)
    dw_ref, _ = ops.conv3x3_wgrad([x], dz8.unpack(), tuple(w.shape))
    dw, _ = ops.conv3x3_wgrad_c8([x], dz8, tuple(w.shape))
    assert torch.allclose(dw, dw_ref, rtol=1e-4, atol=1e-4 * max(1.0, dw_ref.abs().max().item())), (dw - dw_ref).abs().max().item()


@pytest.mark.parametrize("N,C,H,W", [(2, 24, 256, 256), (3, 96, 64, 64), (2, 16, 16, 16)])
def test_deferred_instnorm_parameter_gradients_equal_the_immediate_ones(N, C, H, W):
    """defer_dparams + mtbc_instnorm_dparam_many: the per-plane partials left in the workspace, reduced by the batched entry point
    = the reduction inside mtbc_instnorm_lrelu_bwd, bit for bit (same summation order)."""
    g = _g(N + C + H)
    z = ops.C8.pack((torch.randn(N, C, H, W, generator=g) * 2 + 0.5).to(DEV), 2)
    dy = torch.randn(N, C, H, W, generator=g).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    _, mean, rstd, _ = ops.instnorm_lrelu_fwd_c8(z, gamma, beta, slope=0.1, compute=1)
    b1, b2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    a_, dga, dba = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, compute=1, dbias_pre=b1)
    b_, dgb, dbb = ops.instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma, beta, slope=0.1, compute=1, dbias_pre=b2, defer_dparams=True)
    assert torch.equal(a_.data, b_.data) and torch.equal(dga, dgb) and torch.equal(dba, dbb) and torch.equal(b1, b2)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,segs,Cout,H,W", [(2, [24], 24, 256, 256), (2, [48], 48, 128, 128), (3, [96], 96, 64, 64), (2, [32], 16, 16, 24)])
def test_streaming_instnorm_also_writes_the_maxpool(N, segs, Cout, H, W, compute):
    """mtbc_instnorm_args.pool_y8 / pool_arg: the streaming normalisation (statistics from the conv epilogue) writes the 2x2
    max-pool of the activation it stores and the pool's argmax codes = the pool kernel run on that activation, bit for bit."""
    g = _g(N * 31 + Cout + H + compute)
    Cin = sum(segs)
    xs = [(torch.randn(N, c, H, W, generator=g) + 0.3).to(DEV) for c in segs]
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(DEV), (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    pf, _ = ops.conv3x3_pack_lp(w, compute)
    z8, part = ops.conv3x3_fwd_c8([ops.C8.pack(x, compute) for x in xs], w, None, pf, out_c8=True, stats=True)
    y_a, mean_a, rstd_a, yp_a = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, stats=part, want_planar=True)
    y_b, mean_b, rstd_b, yp_b, pool8, parg = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, stats=part, want_planar=True, want_pool=True)
    assert torch.equal(y_a.data, y_b.data) and torch.equal(yp_a, yp_b) and torch.equal(mean_a, mean_b) and torch.equal(rstd_a, rstd_b)
    ref8, refarg = ops.maxpool2_fwd_c8(y_b, want_argmax=True)
    assert torch.equal(pool8.data, ref8.data) and torch.equal(parg, refarg)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("N,segs,Cout,H,W", [(2, [24], 24, 256, 256), (2, [48], 48, 128, 128), (3, [96], 96, 64, 64), (2, [32], 16, 16, 24),
                                             (2, [192], 192, 8, 8)])
def test_streaming_instnorm_writes_16bit_planes(N, segs, Cout, H, W, compute, pool):
    """mtbc_instnorm_args.y16 beside y8: the planar copy of the activation as 16-bit planes of the output type = the fp32
    planes rounded once (RNE) = the values of the channel-blocked copy, bit for bit; y8 / statistics / pooled outputs as
    without it."""
    g = _g(N * 37 + Cout + H + compute)
    Cin = sum(segs)
    dt = torch.bfloat16 if compute == 1 else torch.float16
    xs = [(torch.randn(N, c, H, W, generator=g) + 0.3).to(DEV) for c in segs]
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(DEV)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(DEV), (torch.randn(Cout, generator=g) * 0.1).to(DEV)
    pf, _ = ops.conv3x3_pack_lp(w, compute)
    z8, part = ops.conv3x3_fwd_c8([ops.C8.pack(x, compute) for x in xs], w, None, pf, out_c8=True, stats=True)
    ref = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, stats=part, want_planar=True, want_pool=pool)
    got = ops.instnorm_lrelu_fwd_c8(z8, gamma, beta, slope=0.1, stats=part, planar16=True, want_pool=pool)
    assert torch.equal(got[0].data, ref[0].data) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    assert got[3].dtype == torch.int16 and torch.equal(got[3].view(dt), ref[3].to(dt))
    assert torch.equal(got[3].view(dt).float(), got[0].unpack())
    if pool:
        assert torch.equal(got[4].data, ref[4].data) and torch.equal(got[5], ref[5])


def test_instnorm_16bit_planes_need_the_streaming_pass():
    """y16 beside y8 without conv-epilogue statistics is refused (MTBC_E_UNSUPPORTED), not silently ignored."""
    from multi_task_breast_cancer_amd import _lib as L
    z = torch.randn(2, 16, 16, 16, generator=_g(5)).to(DEV)
    with pytest.raises(L.MtbcError):
        ops.instnorm_lrelu_fwd_c8(z, compute=1, planar16=True)


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 48, 48, 32, 32), (3, 96, 48, 8, 16), (1, 384, 192, 8, 8), (2, 40, 24, 16, 8), (32, 96, 48, 64, 64)])
def test_convT_wgrad_reads_16bit_planar_x(N, Cin, Cout, H, W, compute):
    """x_type16: the k = 2 ConvT weight gradient on 16-bit planes of x (and dy) = the same kernel fed the fp32 tensors with the
    same (representable) values, bit for bit; fp32 x that is NOT representable gives the same result as its rounded planes."""
    from multi_task_breast_cancer_amd import _lib as L
    g = _g(N + Cin + Cout + H + compute)
    dt = torch.bfloat16 if compute == 1 else torch.float16
    x = torch.randn(N, Cin, H, W, generator=g).to(DEV)
    w = (torch.randn(Cin, Cout, 2, 2, generator=g) * 0.1).to(DEV)
    dy16 = torch.randn(N, Cout, 2 * H, 2 * W, generator=g).to(DEV).to(dt)
    x16 = x.to(dt)
    dw_ref, db_ref = ops.convT_wgrad(x, w, dy16.view(torch.int16), 2, compute=compute, dy16=True)
    dw, db = ops.convT_wgrad(x16.view(torch.int16), w, dy16.view(torch.int16), 2, compute=compute, dy16=True, x16=True)
    if N * H * W <= 4096:       # both launches split the pixels the same way (8 steps per split): the same sums in the same order
        assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    else:                       # the 16-bit-planes launch takes fewer, longer splits: fp32 re-association of the split sums
        assert (dw - dw_ref).abs().max().item() <= 1e-5 * dw_ref.abs().max().item()
        assert (db - db_ref).abs().max().item() <= 1e-5 * db_ref.abs().max().item()
    want = torch.einsum("nchw,ndhawb->cdab", x16.double().cpu(), dy16.double().cpu().view(N, Cout, H, 2, W, 2))
    assert (dw.cpu().double() - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    with pytest.raises(L.MtbcError):        # 16-bit x with an fp32 dy: no kernel, refused
        ops.convT_wgrad(x16.view(torch.int16), w, dy16.float(), 2, compute=compute, x16=True)


def test_program_run_on_two_streams_orders_a_forked_section():
    """mtbc_program_run_ms (MTBC_OP_SET_STREAM / EVENT_RECORD / EVENT_WAIT): ops between a fork and its join run on the second stream,
    ordered behind what the main stream had issued before the fork, and the main stream waits at the join.  (The step plan no longer
    emits forked sections -- two-stream backward measured slower, DESIGN.md -- so the entry point is exercised here.)"""
    import ctypes as C
    from multi_task_breast_cancer_amd import _lib as L
    from multi_task_breast_cancer_amd.engine import _mk
    lib = L.load()
    N, Cc, HW = 2, 16, 4096
    g = _g(5)
    x = torch.randn(N, Cc, 64, 64, generator=g).to(DEV)
    a8 = torch.zeros(N, Cc // 8, HW, 8, dtype=torch.int16, device=DEV)
    back = torch.zeros_like(x)
    ev = [C.c_void_p(), C.c_void_p()]
    for h in ev:
        L.check(lib.mtbc_event_create(C.byref(h)), "event_create")

    def sync(kind, event=0, index=0):
        op = _mk(kind)
        op.u.sync.event, op.u.sync.index = (ev[event] if kind != L.OP_SET_STREAM else None), index
        return op

    pack = _mk(L.OP_C8_PACK)
    pack.u.c8pack.src, pack.u.c8pack.src_batch_stride, pack.u.c8pack.dst = x.data_ptr(), Cc * HW, a8.data_ptr()
    pack.u.c8pack.N, pack.u.c8pack.C, pack.u.c8pack.HW, pack.u.c8pack.compute = N, Cc, HW, 1
    # main: pack | fork -> side: (waits for the pack) nothing else | join ; then unpack on the caller's side through the ordinary entry
    ops_ = [pack, sync(L.OP_EVENT_RECORD, 0), sync(L.OP_SET_STREAM, index=1), sync(L.OP_EVENT_WAIT, 0),
            sync(L.OP_EVENT_RECORD, 1), sync(L.OP_SET_STREAM, index=0), sync(L.OP_EVENT_WAIT, 1)]
    arr = (L.Op * len(ops_))(*ops_)
    side = torch.cuda.Stream()
    streams = (C.c_void_p * 2)(torch.cuda.current_stream().cuda_stream, side.cuda_stream)
    failed = C.c_int32(-1)
    L.check(lib.mtbc_program_run_ms(arr, 0, len(ops_), streams, 2, C.byref(failed)), "program_run_ms")
    L.check(lib.mtbc_c8_unpack(a8.data_ptr(), back.data_ptr(), N, Cc, HW, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "unpack")
    torch.cuda.synchronize()
    assert torch.equal(back, x.to(torch.bfloat16).float())
    for h in ev:
        lib.mtbc_event_destroy(h)


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_focal_one_logit_is_bce_with_logits(gamma):
    """mtbc_focal_fwd_bwd with C == 1: the binary head's criterion.  gamma = 0, alpha = 1 = torch.nn.BCEWithLogitsLoss() (the reference's
    choice for n_classes == 2, experiment_init.py:241-242), loss and gradient; gamma = 2 = the focal modulation of the same per-sample term."""
    g = _g(12)
    x = (torch.randn(37, 1, generator=g) * 4.0)
    x[0, 0], x[1, 0] = 30.0, -30.0                      # saturated logits: the stable form
    t = torch.randint(0, 2, (37, 1), generator=g).float()
    xr = x.clone().double().requires_grad_(True)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(xr, t.double(), reduction="none")
    ref = ((1.0 - torch.exp(-ce)) ** gamma * ce).mean() if gamma else torch.nn.BCEWithLogitsLoss()(xr, t.double())
    ref.backward()
    loss, dx = ops.focal(x.to(DEV), t.to(DEV), alpha=1.0, gamma=gamma, gscale=0.65)
    assert abs(loss.item() - ref.item()) < 1e-6 * max(1.0, abs(ref.item()))
    _close(dx, (0.65 * xr.grad).float(), 1e-5, 1e-7, "d BCE / d logit")


def test_focal_gamma_zero_is_cross_entropy():
    """`classification_criterion: CE` (experiment_init.py:257-261): torch.nn.CrossEntropyLoss(reduction='mean') on the one-hot float target =
    the focal kernel with gamma = 0 (what FusedTrainStep(cls_criterion="CE") runs), with and without class weights."""
    g = _g(13)
    x = torch.randn(29, 3, generator=g) * 3.0
    t = torch.nn.functional.one_hot(torch.randint(0, 3, (29,), generator=g), 3).float()
    for w in (None, torch.tensor([0.2, 0.5, 0.3])):
        xr = x.clone().double().requires_grad_(True)
        # FocalLoss.forward's reduction (criterions.py:14-24 with gamma = 0): mean over samples of the weighted per-sample CE
        ce = -(torch.log_softmax(xr, 1) * t.double() * (w.double() if w is not None else 1.0)).sum(1)
        ref = ce.mean()
        ref.backward()
        loss, dx = ops.focal(x.to(DEV), t.to(DEV), alpha=1.0, gamma=0.0, weight=None if w is None else w.to(DEV))
        assert abs(loss.item() - ref.item()) < 1e-6 * max(1.0, abs(ref.item()))
        _close(dx, xr.grad.float(), 1e-5, 1e-7, "d CE / d logits")
        if w is None:
            assert abs(loss.item() - torch.nn.CrossEntropyLoss()(x, t).item()) < 1e-6


# ------------------------------------------------------------------ the instances the benchmark's step programs launch, element by element
# (N, segs, Cout, H, W, mode, wgrad): mode "bf16" = compute 1, conv output stored as fp16 (O8 = 3) and in fp32 planes (O8 = 0);
# "f16" = compute 2, output fp16 channel-blocked (O8 = 1) and fp32 planes; "f32" = the parity mode (fp32 planar operands).  Every
# case also runs the dgrad into multi-segment fp32 planes (first segment overwritten, the others accumulated) and, with `wgrad`,
# the weight gradient.  The smallest batch that reaches each instance; the kernel always runs the whole batch.
BENCH_CASES = [
    (16, [24], 24, 256, 256, "bf16", False),               # 8-wave blocks (t16 * mblocks = 2048), configs[1] level 0
    (16, [24, 24], 24, 264, 256, "bf16", False),           # 8-wave blocks, H not a multiple of 16 (a half 16-row tile), two segments
    (8, [48], 48, 128, 128, "bf16", True),                 # MT = 3 at 128 x 128 (ntiles * mblocks = 512)
    (8, [48, 48], 40, 128, 128, "bf16", False),            # MT = 3, Cout = 40: the last 16-channel tile of the block 8 / 16 full
    (16, [96], 96, 64, 64, "bf16", True),                  # MT = 3, two channel blocks at 64 x 64
    (32, [192], 192, 32, 32, "bf16", False),               # configs[1] level 3
    (32, [384, 384, 384], 512, 16, 16, "bf16", False),     # 16 x 16 maps past the ring budget: MT = 2 forward, MT = 3 dgrad (K = 1152 x 9)
    (32, [384], 384, 16, 16, "bf16", True),                # the ring kernel at bench batch
    (16, [192], 192, 32, 32, "bf16", False),               # the ring kernel on 32 x 32 maps (a half-batch launch of configs[1])
    (64, [48], 384, 16, 16, "bf16", False),                # 16 x 16 maps, MT = 3 without the ring (reads < 96 channels)
    (16, [24], 24, 512, 512, "f16", False),                # configs[4] level 0: 8-wave blocks, fp16 channel-blocked output
    (8, [48, 48], 40, 128, 128, "f16", False),             # MT = 3, ragged last channel tile, O8 = 1
    (16, [96, 96], 96, 32, 32, "f16", True),               # the ring kernel with fp16 operands
    (16, [24], 32, 128, 128, "f16", False),                # MT = 2 in 4-wave blocks (t16 * mblocks = 512), O8 = 1
    (8, [24], 24, 256, 256, "f32", True),                  # conv3x3_igemm_dma_kernel<2, 0, 2>
    (8, [48], 40, 128, 128, "f32", False),                 # <3, 0, 2>, Cout = 40: a half-empty last channel tile
    (8, [24, 24], 48, 128, 128, "f32", True),              # <3, 0, 2>, two segments
    (8, [96], 48, 64, 64, "f32", True),                    # the 48-channel (3-tile) weight-gradient blocks without the 24-channel packing
    (32, [384, 384, 384], 512, 16, 16, "f32", False),      # <2, 1, 2> forward, <3, 1, 2> dgrad
    (4, [1], 24, 256, 256, "f32", True),                   # the fp32 stem: stem forward kernel, direct dgrad, small-Cin wgrad + bias sums
]
_BENCH_MODE = {"bf16": dict(compute=1, c8=True), "f16": dict(compute=2, c8=True), "f32": {}}


def _bench_case_calls(N, segs, Cout, H, W, mode, wgrad):
    """(op, conv3x3_case_args keywords) of every launch test_conv3x3_bench_instances_match_fp64 makes for this case, in order."""
    m = _BENCH_MODE[mode]
    calls = []
    if mode != "f32":
        calls.append((ops.L.OP_CONV3_FWD, dict(m, out_c8=True, out_fp16=mode == "bf16")))
    calls += [(ops.L.OP_CONV3_FWD, m), (ops.L.OP_CONV3_DGRAD, m)]
    if wgrad:
        calls.append((ops.L.OP_CONV3_WGRAD, m))
    return calls


def _ulp16(v, compute):
    """Spacing of the 16-bit type (1 bf16, 2 fp16) at |v| (fp64 tensor)."""
    mant, emin = (7, -126) if compute == 1 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def _ref_images(N, H, W):
    """Images the fp64 reference is computed for: the first two, the last, and every image of the last block (4 images per
    block on 8 x 8 maps, one elsewhere)."""
    per = 4 if (H, W) == (8, 8) else 1
    return sorted({0, min(1, N - 1), N - 1} | set(range((N - 1) // per * per, N)))


@pytest.mark.parametrize("N,segs,Cout,H,W,mode,wgrad", BENCH_CASES)
def test_conv3x3_bench_instances_match_fp64(N, segs, Cout, H, W, mode, wgrad):
    """The forward / dgrad / wgrad instances of the benchmark's step programs (tests/test_ops_gpu.py::test_step_programs_launch_only_
    reference_tested_conv3x3_instances) against an fp64 conv on the operands the MFMA reads (rounded RNE to its 16-bit type, or fp32):
    fp32 results within 1e-5 of the output scale, 16-bit stored outputs within one unit in the last place of the stored type of the
    fp64 result (+ the same accumulation allowance).  fwd / dgrad are per image: the reference covers _ref_images, every other image
    must be finite.  The launches made are exactly the instances mtbc_conv3x3_kernel_name plans for the case."""
    m = _BENCH_MODE[mode]
    compute = m.get("compute", 0)
    g = _g(N * 7919 + Cout * 31 + H + compute)
    Cin = sum(segs)
    xs = [torch.randn(N, c, H, W, generator=g) for c in segs]
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g)
    dz = torch.randn(N, Cout, H, W, generator=g)
    rnd = (lambda t: _round16(t, compute)) if compute else (lambda t: t)
    idx = _ref_images(N, H, W)
    xr, wr, dzr = rnd(torch.cat(xs, 1)).double(), rnd(w).double(), rnd(dz).double()
    z_ref = F.conv2d(xr[idx], wr, b.double(), padding=1)
    dx_ref = torch.nn.grad.conv2d_input((len(idx), Cin, H, W), wr, dzr[idx], padding=1)
    zs, ds = z_ref.abs().max().item(), dx_ref.abs().max().item()

    xd = [x.to(DEV) for x in xs]
    wd, bd, dzd = w.to(DEV), b.to(DEV), dz.to(DEV)
    pre = [torch.randn(N, c, H, W, generator=g) for c in segs]
    acc = [0] + [1] * (len(segs) - 1)
    dx = [p.to(DEV) for p in pre]
    ops.launched = []
    try:
        if compute:
            pf, pd = ops.conv3x3_pack_lp(wd, compute)
            x8 = [ops.C8.pack(x, compute) for x in xd]
            dz8 = ops.C8.pack(dzd, compute)
            ops.launched.clear()                   # (packing is no conv3x3 launch; keep the list to the checked calls)
            z16 = ops.conv3x3_fwd_c8(x8, wd, bd, pf, out_c8=True, out_fp16=mode == "bf16")
            z = ops.conv3x3_fwd_c8(x8, wd, bd, pf)
            ops.conv3x3_dgrad_c8(dz8, wd, dx, acc, pd)
            if wgrad:
                dw, db = ops.conv3x3_wgrad_c8(x8, dz8, (Cout, Cin, 3, 3), want_bias=True, in_kernel_reduce=False)
        else:
            pf, pd = ops.conv3x3_pack(wd)
            z = ops.conv3x3_fwd(xd, wd, bd, packed=pf)
            ops.conv3x3_dgrad(dzd, wd, dx, acc, packed=pd)
            if wgrad:
                dw, db = ops.conv3x3_wgrad(xd, dzd, (Cout, Cin, 3, 3), want_bias=True)
        torch.cuda.synchronize()
        made = list(ops.launched)
    finally:
        ops.launched = None
    planned = [(op, ops.conv3x3_case_kernel(op, N, segs, Cout, H, W, **kw)) for op, kw in _bench_case_calls(N, segs, Cout, H, W, mode, wgrad)]
    assert made == planned, (made, planned)

    z = z.cpu()
    assert bool(torch.isfinite(z).all()), "fwd: non-finite output"
    err = (z[idx].double() - z_ref).abs().max().item()
    assert err <= 1e-5 * zs, f"fwd ({planned[1 if compute else 0][1]}): max err {err:.3e} vs scale {zs:.3e}"
    if compute:
        st = 2 if mode == "bf16" else compute           # the stored type: fp16 for the bf16 mode's conv outputs
        s = z16.unpack().cpu()
        assert bool(torch.isfinite(s).all()), "stored fwd: non-finite output"
        d = (s[idx].double() - z_ref).abs()
        bound = _ulp16(z_ref, st) + 1e-5 * zs
        worst = (d / bound).max().item()
        assert worst <= 1.0, f"stored fwd ({planned[0][1]}): {worst:.3f} x (one ulp of the stored type + 1e-5 x scale)"
    dx_ref = torch.split(dx_ref, segs, dim=1)
    for i in range(len(segs)):
        got = dx[i].cpu()
        assert bool(torch.isfinite(got).all()), f"dgrad seg {i}: non-finite"
        want = dx_ref[i] + (pre[i][idx].double() if acc[i] else 0)
        err = (got[idx].double() - want).abs().max().item()
        assert err <= 1e-5 * max(ds, want.abs().max().item()), f"dgrad seg {i}: max err {err:.3e} vs scale {ds:.3e}"
    if wgrad:
        ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dzr, padding=1)
        dbr = dzr.sum((0, 2, 3))
        scale = max(1.0, ref.abs().max().item())          # the wgrad tests' standard (test_conv3x3_c8_operands)
        _close(dw, ref.float(), 1e-5, 2e-5 * scale, f"wgrad ({planned[-1][1]})")
        _close(db, dbr.float(), 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "dbias")


# ------------------------------------------------------------------ the 3x3 convolution launches of the step programs, keyed by their arguments
# (op, N, segs, Cout, H, W, mode): one row per coverage key (tests/step_programs.py _conv3_key) of profiles/conv3x3_step_keys.txt that no older
# fp64 test of this file makes; mode = the keywords of ops.conv3x3_case_args, as the engine fills the struct (engine.py conv_cell,
# _gathered_dgrad, _conv_cell_backward).  Shapes: the key holds neither N nor the map size, so each row takes the fewest pixels -- of at
# least 2 images (3 for a weight gradient), 20 rows and 48 columns where the step's map is that large: a ragged last tile in both directions --
# at which the dummy-pointer struct has the key of the step's launch (in brackets: that launch).
F_, D_, W_ = ops.L.OP_CONV3_FWD, ops.L.OP_CONV3_DGRAD, ops.L.OP_CONV3_WGRAD
CONV3_STEP_CASES = [
    (F_, 4, [48, 48, 48], 48, 512, 48, dict(compute=1, c8=True, bias=False, out_accumulate=True)),                      # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 144 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (F_, 4, [48, 48], 48, 512, 48, dict(compute=1, c8=True, bias=False, out_accumulate=True)),                          # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 96 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (F_, 48, [96, 96], 96, 20, 48, dict(compute=1, c8=True, bias=False, out_accumulate=True)),                          # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 192 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (F_, 32, [320, 256], 320, 20, 16, dict(compute=1, c8=True, bias=False)),                                            # conv3x3_igemm_c8_kernel<2, 1, false, 4, 0>  [64 x 576 -> 320 @ 16 x 16 in MTnnUNet bf16]
    (F_, 64, [24, 24, 24, 24], 24, 20, 512, dict(compute=1, c8=True, bias=False)),                                      # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [32 x 96 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 64, [24, 24], 24, 20, 512, dict(compute=1, c8=True, bias=False)),                                              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [32 x 48 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 12, [128], 256, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),         # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>  [64 x 128 -> 256 @ 32 x 32 in MTnnUNet bf16]
    (F_, 2, [1], 32, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),             # conv3x3_stem_fwd_c8_kernel<true>  [64 x 1 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (F_, 2, [320], 320, 8, 8, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),            # conv3x3_igemm_c8_kernel<1, 2, false, 4, 3>  [64 x 320 -> 320 @ 8 x 8 in MTnnUNet bf16]
    (F_, 2, [32], 16, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),            # conv3x3_igemm_c8_kernel<1, 0, false, 4, 3>  [64 x 32 -> 16 @ 256 x 256 in MTnnUNet bf16]
    (F_, 24, [256, 256], 128, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),    # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>  [64 x 512 -> 128 @ 32 x 32 in MTnnUNet bf16]
    (F_, 32, [256], 320, 20, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),         # conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>  [64 x 256 -> 320 @ 16 x 16 in MTnnUNet bf16]
    (F_, 32, [320, 320], 256, 20, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),    # conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>  [64 x 640 -> 256 @ 16 x 16 in MTnnUNet bf16]
    (F_, 64, [32], 32, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),          # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>  [64 x 32 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (F_, 64, [64, 64], 32, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, bias=False, stats=True)),      # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>  [64 x 128 -> 32 @ 128 x 128 in MTnnUNet bf16]
    (F_, 16, [384, 384, 384], 512, 20, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),           # conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>  [32 x 1152 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (F_, 16, [512], 512, 20, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                     # conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (F_, 2, [192], 384, 16, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                      # conv3x3_igemm_c8_ring_kernel<3, 1, false, 3, 3>  [32 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (F_, 2, [1], 24, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                         # conv3x3_stem_fwd_c8_kernel<true>  [32 x 1 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 32, [192], 384, 20, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                     # conv3x3_igemm_c8_kernel<3, 1, false, 4, 3>  [64 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (F_, 4, [24], 48, 512, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                       # conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>  [32 x 24 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (F_, 4, [48, 48, 48], 48, 512, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),               # conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>  [32 x 144 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (F_, 4, [48, 48], 48, 512, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                   # conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>  [32 x 96 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (F_, 48, [96, 96], 96, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                   # conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>  [32 x 192 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (F_, 48, [96], 96, 20, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                       # conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (F_, 64, [24, 24, 48], 24, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>  [32 x 96 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 64, [24, 48], 24, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                  # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>  [32 x 72 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 64, [24], 24, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),                      # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>  [32 x 24 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (F_, 4, [48, 48, 48], 48, 512, 48, dict(compute=2, c8=True, bias=False, out_accumulate=True)),                      # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 144 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (F_, 4, [48, 48], 48, 512, 48, dict(compute=2, c8=True, bias=False, out_accumulate=True)),                          # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 96 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (F_, 48, [96, 96], 96, 20, 48, dict(compute=2, c8=True, bias=False, out_accumulate=True)),                          # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 192 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (F_, 64, [24, 24, 24, 24], 24, 20, 512, dict(compute=2, c8=True, bias=False)),                                      # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0>  [16 x 96 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (F_, 64, [24, 24], 24, 20, 512, dict(compute=2, c8=True, bias=False)),                                              # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0>  [16 x 48 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (F_, 4, [24], 48, 512, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                                      # conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>  [16 x 24 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (F_, 4, [48, 48, 48], 48, 512, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                              # conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>  [16 x 144 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (F_, 4, [48, 48], 48, 512, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                                  # conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>  [16 x 96 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (F_, 48, [96, 96], 96, 20, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                                  # conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>  [16 x 192 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (F_, 48, [96], 96, 20, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                                      # conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>  [16 x 96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (F_, 6, [384, 384, 384], 512, 20, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                           # conv3x3_igemm_c8_kernel<2, 0, true, 4, 1>  [16 x 1152 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (F_, 6, [512], 512, 20, 48, dict(compute=2, c8=True, out_c8=True, stats=True)),                                     # conv3x3_igemm_c8_kernel<2, 0, true, 4, 1>  [16 x 512 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (F_, 64, [24, 24, 48], 24, 20, 512, dict(compute=2, c8=True, out_c8=True, stats=True)),                             # conv3x3_igemm_c8_kernel<2, 0, true, 8, 1>  [16 x 96 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (F_, 64, [24, 48], 24, 20, 512, dict(compute=2, c8=True, out_c8=True, stats=True)),                                 # conv3x3_igemm_c8_kernel<2, 0, true, 8, 1>  [16 x 72 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (F_, 64, [24], 24, 20, 512, dict(compute=2, c8=True, out_c8=True, stats=True)),                                     # conv3x3_igemm_c8_kernel<2, 0, true, 8, 1>  [16 x 24 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (F_, 16, [512], 512, 20, 16, dict()),                                                                               # conv3x3_igemm_dma_kernel<2, 1, 2>  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (F_, 2, [192], 384, 16, 16, dict()),                                                                                # conv3x3_igemm_dma_kernel<1, 1, 2>  [32 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (F_, 32, [192], 384, 20, 16, dict()),                                                                               # conv3x3_igemm_dma_kernel<3, 1, 2>  [64 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (F_, 4, [24, 48], 24, 512, 48, dict()),                                                                             # conv3x3_igemm_dma_kernel<2, 0, 2>  [32 x 72 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (F_, 4, [24], 48, 512, 48, dict()),                                                                                 # conv3x3_igemm_dma_kernel<3, 0, 2>  [32 x 24 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (D_, 24, [48, 48, 48, 48], 48, 20, 48, dict(accumulate=[0, 0, 0, 0])),                                              # conv3x3_igemm_dma_kernel<3, 0, 2>  [32 x 192 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (D_, 12, [384, 384, 384], 512, 20, 16, dict(accumulate=[0, 0, 0])),                                                 # conv3x3_igemm_dma_kernel<3, 1, 2>  [32 x 1152 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (D_, 16, [512], 512, 20, 16, dict(accumulate=[0])),                                                                 # conv3x3_igemm_dma_kernel<2, 1, 2>  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (D_, 2, [192], 384, 16, 16, dict(accumulate=[0])),                                                                  # conv3x3_igemm_dma_kernel<1, 1, 2>  [64 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (D_, 32, [384], 384, 20, 16, dict(accumulate=[0])),                                                                 # conv3x3_igemm_dma_kernel<3, 1, 2>  [64 x 384 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (D_, 32, [48, 48, 48], 48, 20, 48, dict(accumulate=[1, 1, 0])),                                                     # conv3x3_igemm_dma_kernel<3, 0, 2>  [32 x 144 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (D_, 32, [24, 24, 24, 48], 24, 20, 48, dict(accumulate=[1, 1, 1, 0])),                                              # conv3x3_igemm_dma_kernel<3, 0, 2>  [32 x 120 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (D_, 2, [192], 384, 16, 16, dict(accumulate=[1])),                                                                  # conv3x3_igemm_dma_kernel<1, 1, 2>  [32 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (D_, 12, [384, 384, 384], 512, 20, 16, dict(compute=1, c8=True, accumulate=[0, 0, 0])),                             # conv3x3_igemm_c8_kernel<3, 1, false, 4, 0>  [32 x 1152 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (D_, 16, [320, 320], 256, 20, 16, dict(compute=1, c8=True, accumulate=[0, 0])),                                     # conv3x3_igemm_c8_kernel<2, 1, false, 4, 0>  [64 x 640 -> 256 @ 16 x 16 in nnUNet bf16]
    (D_, 24, [24, 48], 24, 20, 512, dict(compute=1, c8=True, accumulate=[0, 2])),                                       # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [32 x 72 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (D_, 24, [96, 96], 96, 20, 48, dict(compute=1, c8=True, accumulate=[0, 2])),                                        # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 192 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (D_, 32, [32, 32], 32, 20, 512, dict(compute=1, c8=True, accumulate=[0, 2])),                                       # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [64 x 64 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (D_, 48, [48, 48], 48, 20, 48, dict(compute=1, c8=True, accumulate=[0, 2])),                                        # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 96 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (D_, 16, [512], 512, 20, 16, dict(compute=1, c8=True, accumulate=[0])),                                             # conv3x3_igemm_c8_kernel<2, 1, false, 4, 0>  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (D_, 2, [320], 320, 8, 8, dict(compute=1, c8=True, accumulate=[0])),                                                # conv3x3_igemm_c8_kernel<1, 2, false, 4, 0>  [64 x 320 -> 320 @ 8 x 8 in MTnnUNet bf16]
    (D_, 32, [384], 384, 20, 16, dict(compute=1, c8=True, accumulate=[0])),                                             # conv3x3_igemm_c8_kernel<3, 1, false, 4, 0>  [64 x 384 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (D_, 4, [24], 48, 512, 48, dict(compute=1, c8=True, accumulate=[0])),                                               # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0>  [32 x 24 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (D_, 48, [64], 64, 20, 48, dict(compute=1, c8=True, accumulate=[0])),                                               # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0>  [64 x 64 -> 64 @ 64 x 64 in MTnnUNet bf16]
    (D_, 64, [32], 16, 20, 512, dict(compute=1, c8=True, accumulate=[0])),                                              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [64 x 32 -> 16 @ 256 x 256 in MTnnUNet bf16]
    (D_, 64, [32], 32, 20, 512, dict(compute=1, c8=True, accumulate=[0])),                                              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>  [64 x 32 -> 32 @ 128 x 128 in MTnnUNet bf16]
    (D_, 2, [192], 384, 16, 16, dict(compute=1, c8=True, accumulate=[1])),                                              # conv3x3_igemm_c8_ring_kernel<3, 1, false, 0, 3>  [32 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (D_, 32, [320], 256, 20, 16, dict(compute=1, c8=True, accumulate=[1])),                                             # conv3x3_igemm_c8_kernel<2, 1, false, 4, 0>  [64 x 320 -> 256 @ 16 x 16 in MTnnUNet bf16]
    (D_, 4, [48], 24, 512, 48, dict(compute=1, c8=True, accumulate=[2])),                                               # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 48 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (D_, 48, [96], 96, 20, 48, dict(compute=1, c8=True, accumulate=[2])),                                               # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (D_, 4, [384, 384, 384], 512, 20, 48, dict(compute=2, c8=True, accumulate=[0, 0, 0])),                              # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 1152 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (D_, 24, [24, 48], 24, 20, 512, dict(compute=2, c8=True, accumulate=[0, 2])),                                       # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0>  [16 x 72 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (D_, 24, [96, 96], 96, 20, 48, dict(compute=2, c8=True, accumulate=[0, 2])),                                        # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 192 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (D_, 48, [48, 48], 48, 20, 48, dict(compute=2, c8=True, accumulate=[0, 2])),                                        # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 96 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (D_, 12, [384], 384, 20, 48, dict(compute=2, c8=True, accumulate=[0])),                                             # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [32 x 384 -> 384 @ 32 x 32 in MTUNetPlusPlus f16]
    (D_, 4, [48], 48, 512, 48, dict(compute=2, c8=True, accumulate=[0])),                                               # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 48 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (D_, 6, [512], 512, 20, 48, dict(compute=2, c8=True, accumulate=[0])),                                              # conv3x3_igemm_c8_kernel<2, 0, true, 4, 0>  [16 x 512 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (D_, 2, [192], 384, 20, 32, dict(compute=2, c8=True, accumulate=[1])),                                              # conv3x3_igemm_c8_ring_kernel<3, 0, true, 0, 3>  [16 x 192 -> 384 @ 32 x 32 in MTUNetPlusPlus f16]
    (D_, 4, [48], 24, 512, 48, dict(compute=2, c8=True, accumulate=[2])),                                               # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 48 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (D_, 48, [96], 96, 20, 48, dict(compute=2, c8=True, accumulate=[2])),                                               # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0>  [16 x 96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (W_, 3, [1], 24, 20, 48, dict(bias=False)),                                                                         # conv3x3_wgrad_smallcin_kernel + splitk_reduce  [32 x 1 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (W_, 3, [24, 24, 24, 24, 48], 24, 20, 48, dict(bias=False)),                                                        # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce  [32 x 144 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (W_, 3, [24, 24, 48], 24, 20, 48, dict(bias=False)),                                                                # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce  [32 x 96 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (W_, 3, [24], 24, 20, 48, dict(bias=False)),                                                                        # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce  [32 x 24 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (W_, 3, [384, 384, 384], 512, 16, 16, dict(bias=False)),                                                            # conv3x3_wgrad_mfma_kernel<1, 2, false> + splitk_reduce  [32 x 1152 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (W_, 3, [48, 48, 48, 48], 48, 20, 48, dict(bias=False)),                                                            # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce  [32 x 192 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (W_, 3, [48, 48, 48], 48, 20, 48, dict(bias=False)),                                                                # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce  [32 x 144 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (W_, 3, [48], 48, 20, 48, dict(bias=False)),                                                                        # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce  [32 x 48 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (W_, 3, [48], 96, 20, 48, dict(bias=False)),                                                                        # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce  [32 x 48 -> 96 @ 64 x 64 in MTUNetPlusPlus f32]
    (W_, 3, [512], 512, 16, 16, dict(bias=False)),                                                                      # conv3x3_wgrad_mfma_kernel<1, 2, false> + splitk_reduce  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (W_, 3, [96, 96, 96], 96, 20, 48, dict(bias=False)),                                                                # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce  [32 x 288 -> 96 @ 64 x 64 in MTUNetPlusPlus f32]
    (W_, 3, [96], 96, 20, 48, dict(bias=False)),                                                                        # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus f32]
    (W_, 3, [1], 24, 20, 48, dict(compute=1, c8=True, bias=False)),                                                     # conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce  [32 x 1 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (W_, 3, [1], 32, 20, 48, dict(compute=1, c8=True, bias=False)),                                                     # conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce  [64 x 1 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (W_, 3, [24, 24, 24, 24, 48], 24, 20, 128, dict(compute=1, c8=True, bias=False)),                                   # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce  [32 x 144 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (W_, 3, [24, 24, 48], 24, 20, 128, dict(compute=1, c8=True, bias=False)),                                           # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce  [32 x 96 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (W_, 3, [24], 24, 20, 48, dict(compute=1, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce  [32 x 24 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (W_, 3, [32, 32], 32, 20, 128, dict(compute=1, c8=True, bias=False)),                                               # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce  [64 x 64 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (W_, 3, [320, 320], 256, 16, 16, dict(compute=1, c8=True, bias=False)),                                             # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce  [64 x 640 -> 256 @ 16 x 16 in MTnnUNet bf16]
    (W_, 3, [320], 320, 8, 8, dict(compute=1, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<false, 1> + splitk_reduce  [64 x 320 -> 320 @ 8 x 8 in MTnnUNet bf16]
    (W_, 3, [384, 384, 384], 512, 16, 16, dict(compute=1, c8=True, bias=False)),                                        # conv3x3_wgrad_c8i_kernel<false, 2, false>  [32 x 1152 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (W_, 3, [384], 384, 16, 16, dict(compute=1, c8=True, bias=False)),                                                  # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce  [64 x 384 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (W_, 3, [48, 48, 48, 48], 48, 20, 128, dict(compute=1, c8=True, bias=False)),                                       # conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce  [32 x 192 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (W_, 3, [48, 48, 48], 48, 20, 128, dict(compute=1, c8=True, bias=False)),                                           # conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce  [32 x 144 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (W_, 3, [48], 48, 20, 48, dict(compute=1, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce  [32 x 48 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (W_, 3, [512], 512, 16, 16, dict(compute=1, c8=True, bias=False)),                                                  # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (W_, 3, [64], 64, 20, 128, dict(compute=1, c8=True, bias=False)),                                                   # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce  [64 x 64 -> 64 @ 128 x 128 in MTnnUNet bf16]
    (W_, 3, [96, 96, 96], 96, 20, 48, dict(compute=1, c8=True, bias=False)),                                            # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce  [32 x 288 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (W_, 3, [96], 96, 20, 48, dict(compute=1, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (W_, 3, [192, 192], 192, 20, 48, dict(compute=2, c8=True, bias=False)),                                             # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce  [16 x 384 -> 192 @ 64 x 64 in MTUNetPlusPlus f16]
    (W_, 3, [1], 24, 20, 48, dict(compute=2, c8=True, bias=False)),                                                     # conv3x3_wgrad_stem_c8_kernel<true> + splitk_reduce  [16 x 1 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (W_, 3, [24, 24, 24, 24, 48], 24, 20, 128, dict(compute=2, c8=True, bias=False)),                                   # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce  [16 x 144 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (W_, 3, [24, 24, 48], 24, 20, 128, dict(compute=2, c8=True, bias=False)),                                           # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce  [16 x 96 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (W_, 3, [24], 24, 20, 48, dict(compute=2, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce  [16 x 24 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (W_, 3, [384, 384, 384], 512, 20, 32, dict(compute=2, c8=True, bias=False)),                                        # conv3x3_wgrad_c8_kernel<true, 0>  [16 x 1152 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (W_, 3, [48, 48, 48, 48], 48, 20, 128, dict(compute=2, c8=True, bias=False)),                                       # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce  [16 x 192 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (W_, 3, [48, 48, 48], 48, 20, 128, dict(compute=2, c8=True, bias=False)),                                           # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce  [16 x 144 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (W_, 3, [48], 48, 20, 48, dict(compute=2, c8=True, bias=False)),                                                    # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce  [16 x 48 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (W_, 3, [512], 512, 20, 32, dict(compute=2, c8=True, bias=False)),                                                  # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce  [16 x 512 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (W_, 3, [96, 96, 96], 96, 20, 128, dict(compute=2, c8=True, bias=False)),                                           # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce  [16 x 288 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (W_, 3, [96], 96, 20, 128, dict(compute=2, c8=True, bias=False)),                                                   # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce  [16 x 96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
]


def _conv3_case_id(case):
    op, N, segs, Cout, H, W, mode = case
    flags = "-".join(k if v is True else f"{k}{v}".replace(" ", "") for k, v in mode.items() if v is not False and k not in ("c8", "compute"))
    return f"{ {F_: 'fwd', D_: 'dgrad', W_: 'wgrad'}[op]}-{('f32', 'bf16', 'f16')[mode.get('compute', 0)]}-{N}x{'+'.join(map(str, segs))}-{Cout}@{H}x{W}" \
        + (f"-{flags}" if flags else "") + ("-nobias" if mode.get("bias") is False and op == F_ else "")


_NAN16 = 0x7fff          # a NaN in bf16 and in fp16: what a 16-bit destination holds before the launch


@pytest.mark.parametrize("case", CONV3_STEP_CASES, ids=_conv3_case_id)
def test_conv3x3_step_instances_match_fp64(case):
    """One launch through ops.conv3x3_launch with the struct of conv3x3_case_args(ptrs=...), which must be the launch the row's dummy-pointer
    struct plans, against a plain fp64 computation on the CPU on the operands the kernel reads: rounded RNE to the 16-bit type where it reads
    16-bit values (channel-blocked operands, the 16-bit weight images), fp32 otherwise (the fp32 mode; the stem's image and weights).
      forward / gathered dgrad   F.conv2d (+ bias, + the prefill with out_accumulate) on _ref_images, every other image finite; fp32 planes within
                                 1e-5 x the output scale, 16-bit stored outputs within one ulp of the stored type + 1e-5 x scale
                                 (test_conv3x3_bench_instances_match_fp64)
      statistics                 summed over the slots against fp64 sum / sum of squares of the stored output read back, no NaN slot left; the
                                 bounds of test_instnorm_statistics_from_the_conv_epilogue
      dgrad                      conv2d_input; code 0 overwrites (NaN before), code 1 adds to a random prefill: 1e-5 x scale; code 2 (16-bit
                                 planes) and code 3 (channel-blocked): one ulp of the type + 1e-5 x scale
      weight gradient            conv2d_weight over the WHOLE batch, _close(dw, ref, 1e-5, 2e-5 * max(1, |ref|max)) (test_conv3x3_c8_operands),
                                 with accumulate_dw on the sum with a random prefill; without dbias the buffer offered to nobody keeps its marker;
                                 a name without a reduction = the direct store: the workspace keeps its pre-fill; run twice, bit-identical."""
    op, N, segs, Cout, H, W, mode = case
    # the norm-backward epilogue of a gathered dgrad (norm_z, out_partial) and the in-kernel split-K reduction: no step program launches them
    # (profiles/conv3x3_step_keys.txt); test_gathered_dgrad_prepares_the_instnorm_backward and FIXUP_CASES hold their checks
    assert not set(mode) & {"norm", "out_partial", "in_kernel_reduce", "dx_c8", "packed"}, mode
    lib, dev = ops.L.load(), torch.device(DEV)
    compute, c8 = mode.get("compute", 0), mode.get("c8", False)
    Cin, HW = sum(segs), H * W
    stem = len(segs) == 1 and segs[0] <= ops.L.STEM_MAX_CIN
    # (a row of another module's table -- tests/test_mt_btsunet_launches_gpu.py calls this test with its own -- draws from behind the table's seeds)
    row = CONV3_STEP_CASES.index(case) if case in CONV3_STEP_CASES else len(CONV3_STEP_CASES) + sum(segs) + 3 * op + 7 * compute + W
    g = torch.Generator(device=dev).manual_seed(row * 7919 + N * 31 + Cout + H)
    rand = lambda *shape: torch.randn(*shape, generator=g, device=dev)                                        # noqa: E731
    rnd = lambda t: _round16(t, compute)                                                                       # noqa: E731
    dummy = ops.conv3x3_case_args(op, N, segs, Cout, H, W, **mode)
    planned = [(op, ops.conv3x3_kernel_name(dummy, op))]
    idx = _ref_images(N, H, W)
    w = rand(Cout, Cin, 3, 3) * (2.0 / (9 * Cin)) ** 0.5
    ptrs = {"w": w}

    def launch(p):
        ops.launched = []
        try:
            ops.conv3x3_launch(ops.conv3x3_case_args(op, N, segs, Cout, H, W, ptrs=p, **mode), op)
            torch.cuda.synchronize()
            assert ops.launched == planned, (ops.launched, planned)
        finally:
            ops.launched = None

    def check16(what, got16, shape, st, want, scale, blocked):
        """A 16-bit stored tensor (channel-blocked or planes, int16 storage of type st): finite everywhere, the images idx against `want`."""
        got = _planes_of(got16.cpu(), shape, st) if blocked else _from16(got16.cpu(), st)
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite or unwritten value"
        worst = ((got[idx] - want).abs() / (_ulp16(want, st) + 1e-5 * scale)).max().item()
        print(f"{what}: {worst:.3f} x (one ulp of the stored type + 1e-5 x scale)")
        assert worst <= 1.0, f"{what} ({planned[0][1]}): {worst:.3f} x (one ulp of the stored type + 1e-5 x scale)"
        return got

    def check32(what, got, want, scale):
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite or unwritten value"
        err = (got[idx].double() - want).abs().max().item()
        print(f"{what}: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 1e-5 * scale, f"{what} ({planned[0][1]}): max err {err:.3e} vs scale {scale:.3e}"

    if op == F_:
        xs = [rand(N, c, H, W) for c in segs]
        b = rand(Cout) if mode.get("bias", True) else None
        sixteen = c8 and not stem               # the MFMA reads 16-bit values; the stem computes in fp32 on the fp32 image and weights
        ptrs.update({"in": [_c8_of(x, compute) for x in xs] if sixteen else xs, "bias": b})
        if not stem:
            ptrs["w_packed"] = ops.conv3x3_pack_lp(w, compute)[0] if compute else ops.conv3x3_pack(w)[0]
        out_c8, st = mode.get("out_c8", False), (2 if mode.get("out_fp16") else compute)
        pre = rand(N, Cout, H, W) if mode.get("out_accumulate") else None
        if out_c8:
            out = torch.full((N, Cout // 8, HW, 8), _NAN16, dtype=torch.int16, device=dev)
        else:
            out = pre.clone() if pre is not None else torch.full((N, Cout, H, W), float("nan"), device=dev)
        ptrs["out"] = out
        if mode.get("stats"):
            slots = lib.mtbc_conv3x3_stats_slots(C.byref(dummy))
            assert slots > 0, "no epilogue statistics for this launch"
            ptrs["stats_partial"] = torch.full((N, slots, Cout, 2), float("nan"), device=dev)
        launch(ptrs)
        xr = torch.cat([x[idx] for x in xs], 1).cpu()
        xr, wr = (rnd(xr), rnd(w.cpu())) if sixteen else (xr, w.cpu())
        ref = F.conv2d(xr.double(), wr.double(), None if b is None else b.cpu().double(), padding=1)
        scale = ref.abs().max().item()
        if pre is not None:
            ref = ref + pre[idx].cpu().double()
            scale = max(scale, ref.abs().max().item())
        if out_c8:
            stored = check16("stored fwd", out, (N, Cout, H, W), st, ref, scale, True)
        else:
            check32("fwd", out, ref, scale)
        if mode.get("stats"):
            part = ptrs["stats_partial"].cpu()
            assert not torch.isnan(part).any(), "a (image, subset, channel) entry was not written"
            tot = part.double().sum(1)                                                            # (N, Cout, 2)
            s_ref, q_ref = stored.sum((2, 3)), (stored * stored).sum((2, 3))
            print(f"statistics: sum err {(tot[..., 0] - s_ref).abs().max().item():.3e}, sum of squares err {(tot[..., 1] - q_ref).abs().max().item():.3e}")
            assert torch.allclose(tot[..., 0], s_ref, rtol=1e-5, atol=1e-5 * q_ref.abs().max().item() ** 0.5 * H * W ** 0.5), "statistics: sum"
            assert torch.allclose(tot[..., 1], q_ref, rtol=1e-5, atol=1e-3), "statistics: sum of squares"
    elif op == D_:
        codes = mode["accumulate"]
        dz = rand(N, Cout, H, W)
        ptrs.update({"dout": _c8_of(dz, compute) if c8 else dz, "w_packed": ops.conv3x3_pack_lp(w, compute)[1] if compute else ops.conv3x3_pack(w)[1]})
        pre, dxs = [], []
        for c, code in zip(segs, codes):
            pre.append(rand(N, c, H, W) if code == 1 else None)
            if code >= 2:
                dxs.append(torch.full((N, c // 8, HW, 8) if code == 3 else (N, c, H, W), _NAN16, dtype=torch.int16, device=dev))
            else:
                dxs.append(pre[-1].clone() if code == 1 else torch.full((N, c, H, W), float("nan"), device=dev))
        ptrs["in"] = dxs
        launch(ptrs)
        dzr, wr = dz[idx].cpu(), w.cpu()
        dzr, wr = (rnd(dzr), rnd(wr)) if compute else (dzr, wr)
        ref = torch.nn.grad.conv2d_input((len(idx), Cin, H, W), wr.double(), dzr.double(), padding=1)
        ds = ref.abs().max().item()
        for i, (want, code) in enumerate(zip(torch.split(ref, segs, dim=1), codes)):
            if code >= 2:
                check16(f"dgrad seg {i} (code {code})", dxs[i], (N, segs[i], H, W), compute, want, ds, code == 3)
            else:
                want = want + (pre[i][idx].cpu().double() if code == 1 else 0)
                check32(f"dgrad seg {i} (code {code})", dxs[i], want, max(ds, want.abs().max().item()))
    else:
        xs, dz = [rand(N, c, H, W) for c in segs], rand(N, Cout, H, W)
        acc, want_bias = mode.get("accumulate_dw", False), mode.get("bias", True)
        pre = rand(Cout, Cin, 3, 3) if acc else torch.full((Cout, Cin, 3, 3), float("nan"), device=dev)
        db_pre = rand(Cout) if acc else torch.full((Cout,), float("nan"), device=dev)
        ws_mark = torch.full((dummy.workspace_bytes // 4 + 64,), 1993.0, device=dev)
        idle = torch.full((Cout,), 1993.0, device=dev)              # the dbias buffer of a launch without dbias: handed to nobody
        ptrs.update({"in": xs if (stem or not c8) else [_c8_of(x, compute) for x in xs], "dout": _c8_of(dz, compute) if c8 else dz})
        runs = []
        for _ in range(2):
            dw, ws = pre.clone(), ws_mark.clone()
            db = db_pre.clone() if want_bias else None
            ptrs.update({"dw": dw, "dbias": db, "workspace": ws, "wgrad_sync": ops.wgrad_sync_buffer(dev, dummy.wgrad_sync_bytes)})
            launch(ptrs)
            runs.append((dw, db, ws))
        dw, db, ws = runs[0]
        assert torch.equal(dw, runs[1][0]) and (db is None or torch.equal(db, runs[1][1])), "not deterministic"
        assert torch.equal(idle, torch.full_like(idle, 1993.0))
        if " + " not in planned[0][1]:              # the direct store: nothing was staged through the workspace
            assert torch.equal(ws, ws_mark), "direct store: the workspace was written"
        xr, dzr = torch.cat(xs, 1).cpu(), dz.cpu()
        xr = rnd(xr) if compute and not stem else xr
        dzr = rnd(dzr) if compute else dzr
        ref = torch.nn.grad.conv2d_weight(xr.double(), (Cout, Cin, 3, 3), dzr.double(), padding=1)
        dbr = dzr.double().sum((0, 2, 3))
        if acc:
            ref, dbr = ref + pre.cpu().double(), dbr + db_pre.cpu().double()
        print(f"wgrad: max err {(dw.cpu().double() - ref).abs().max().item():.3e} vs scale {ref.abs().max().item():.3e}")
        _close(dw, ref.float(), 1e-5, 2e-5 * max(1.0, ref.abs().max().item()), f"wgrad ({planned[0][1]})")
        if want_bias:
            _close(db, dbr.float(), 1e-5, 2e-5 * max(1.0, dbr.abs().max().item()), "dbias")


def _reference_tested_conv3x3_calls():
    """(op, (N, segs, Cout, H, W), mode, table) of every conv3x3 call that a test of this file checks element by element against fp64 -- the
    rows of WGRAD_PLAN_CASES aside --, from the tests' own case tables.  Tests that compare two kernels with each other, or a kernel with an
    fp32 reference, do not count: test_conv3x3_mfma_fwd_dgrad_wgrad, the forward / dgrad half of test_conv3x3_c8_operands,
    test_stem_conv_on_the_16bit_path, test_bf16_mode_conv_output_stored_as_fp16, test_instnorm_statistics_from_the_conv_epilogue."""
    calls = [(op, (N, segs, Cout, H, W), mode, "CONV3_STEP_CASES") for op, N, segs, Cout, H, W, mode in CONV3_STEP_CASES]      # test_conv3x3_step_instances_match_fp64
    for case in BENCH_CASES:                                     # test_conv3x3_bench_instances_match_fp64
        calls += [(op, case[:5], kw, "BENCH_CASES") for op, kw in _bench_case_calls(*case)]
    for compute in (1, 2):
        m = dict(compute=compute, c8=True)
        fix, nobias = dict(m, in_kernel_reduce=True), dict(m, in_kernel_reduce=True, bias=False)
        for case in C8_CASES:                                    # test_conv3x3_c8_operands: the weight gradients
            calls += [(W_, case, fix, "C8_CASES"), (W_, case, dict(nobias, accumulate_dw=True), "C8_CASES")]
        for case in C8_CASES + EXTRA16_CASES:                    # test_conv3x3_16bit_fwd_dgrad_match_fp64_on_rounded_operands
            calls += [(op, case, kw, "C8_CASES + EXTRA16_CASES") for op in (F_, D_) for kw in (m, dict(compute=compute))]
        for table, cases in (("C8W_CASES", C8W_CASES), ("C8I_CASES", C8I_CASES)):      # test_conv3x3_wgrad_c8_wide_blocks
            for case in cases:
                calls += [(W_, case, fix, table), (W_, case, nobias, table), (W_, case, dict(nobias, accumulate_dw=True), table)]
        for case in FIXUP_CASES:                                 # test_conv3x3_wgrad_c8_in_kernel_split_k_reduction
            calls += [(W_, case, kw, "FIXUP_CASES") for kw in (fix, m, nobias, dict(nobias, accumulate_dw=True))]
    return calls


def _reference_tested_conv3x3_keys():
    """The (op, _conv3_key) of _reference_tested_conv3x3_calls, through dummy-pointer structs (ops.conv3x3_case_args)."""
    return {(op, _conv3_key(ops.conv3x3_case_args(op, *case, **kw), op)) for op, case, kw, _ in _reference_tested_conv3x3_calls()}


def test_step_programs_launch_only_reference_tested_conv3x3_instances():
    """Surveys (builds, does not run) the step programs of the benchmark's configurations and keys every 3x3 conv launch by
    tests/step_programs.py _conv3_key -- the launches mtbc_conv3x3_kernel_name plans, reduction included, and the branches the arguments
    select: each must be the key of a call that a test of this file checks against fp64.  A new dispatch path or a new combination of
    arguments that no such test makes fails here, named with its program and shape (profiles/conv3x3_step_keys.txt: the listing)."""
    L = ops.L
    assert_all_tested("conv3x3", _reference_tested_conv3x3_keys(), [survey(p) for p in STEP_PROGRAMS] + [survey(STEP_PROGRAMS[0], 64)],
                      required=(L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD))


# ------------------------------------------------------------------ the 3x3 weight gradients of the step programs, keyed by their split plans
# (N, segs, Cout, H, W, mode): one row per plan key (tests/step_programs.py _wgrad_plan_key: the kernel_name string + the class of the plan
# mtbc_conv3x3_wgrad_plan reports) that the surveyed step programs launch and no older weight-gradient case of this file makes, run through
# test_conv3x3_step_instances_match_fp64.  Shapes: of the channel counts and map sizes at which the dummy-pointer struct has the plan key of the
# step's launch, the one with the fewest multiply-adds N * H * W * Cin * Cout (the fp64 reference on the CPU is the cost of a case), then the
# fewest pixels; one segment (the plan reads Cin, not the segments: the _conv3_key rows above hold those).  Behind each row: its plan key, and in
# brackets the first launch it stands for (profiles/conv3x3_step_keys.txt lists them all).
_PB, _PH, _P32 = dict(compute=1, c8=True, bias=False), dict(compute=2, c8=True, bias=False), dict(bias=False)
WGRAD_PLAN_CASES = [
    (32, [8], 384, 64, 48, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (even, tiles>=3, ragged, crosses, splitk_reduce<16> x2+x1)  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (16, [144], 8, 128, 48, _PB),         # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (even, tiles>=3, ragged, crosses, splitk_reduce<16> x8+x2+x1)  [32 x 48 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16]
    (48, [8], 320, 44, 48, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (even, tiles>=3, splitk_reduce<16> x2)  [64 x 128+128 -> 64 @ 64 x 64 in MTnnUNet bf16]
    (32, [840], 8, 64, 64, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (even, tiles>=3, splitk_reduce<4> x8)  [32 x 96+96+96 -> 96 @ 64 x 64 in MTUNetPlusPlus bf16: 32 splits need 27 .. 32 channel blocks]
    (9, [512], 40, 16, 48, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, crosses, splitk_reduce<4> x2)  [64 x 256+256 -> 128 @ 32 x 32 in MTnnUNet bf16]
    (3, [384], 40, 64, 48, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, crosses, splitk_reduce<4> x8)  [64 x 128 -> 256 @ 32 x 32 in MTnnUNet bf16]
    (2, [72], 512, 44, 48, _PB),          # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2+x1)  [32 x 192 -> 192 @ 32 x 32 in MTUNetPlusPlus bf16]
    (4, [8], 384, 96, 48, _PB),           # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x2)  [64 x 128 -> 128 @ 32 x 32 in MTnnUNet bf16]
    (40, [512], 40, 12, 8, _PB),          # conv3x3_wgrad_c8_kernel<false, 1> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2+x1)  [64 x 320 -> 320 @ 8 x 8 in MTnnUNet bf16]
    (9, [256], 512, 16, 16, _PB),         # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce (images>=3, ciblocks>1, splitk_reduce<4> x1)  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus bf16]
    (24, [96], 320, 16, 16, _PB),         # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce (images>=3, ciblocks>1, splitk_reduce<4> x2)  [64 x 256 -> 256 @ 16 x 16 in MTnnUNet bf16]
    (40, [512], 40, 16, 16, _PB),         # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce (images>=3, short_last_range, ciblocks>1, splitk_reduce<4> x2+x1)  [64 x 256 -> 320 @ 16 x 16 in MTnnUNet bf16]
    (24, [192], 384, 16, 16, _PB),        # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce (images>=3, ciblocks>1, splitk_reduce<4> x2)  [64 x 192 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (40, [96], 384, 16, 16, _PB),         # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce (images>=3, short_last_range, ciblocks>1, splitk_reduce<4> x2+x1)  [64 x 384 -> 384 @ 16 x 16 in MTUNetPlusPlus bf16]
    (8, [384], 8, 12, 512, _PB),          # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, ragged_cit, splitk_reduce<16> x8)  [32 x 24+24+24+24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (8, [192], 8, 12, 512, _PB),          # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [32 x 24+24+24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (16, [64], 40, 12, 512, _PB),         # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, splitk_reduce<16> x8)  [64 x 32+32 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (8, [64], 8, 48, 512, _PB),           # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, splitk_reduce<64, 16> x8)  [32 x 24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (8, [96], 96, 12, 512, _PB),          # conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [32 x 48+48+48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (8, [144], 96, 24, 256, _PB),         # conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, ragged_cit, splitk_reduce<16> x8)  [32 x 48+48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (8, [96], 96, 24, 256, _PB),          # conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [32 x 48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus bf16]
    (32, [1], 8, 128, 512, _PB),          # conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce (bands=16, splitk_reduce<64, 16> x8)  [32 x 1 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (16, [144], 8, 128, 48, _PH),         # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (even, tiles>=3, ragged, crosses, splitk_reduce<16> x8+x2+x1)  [16 x 48 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (3, [384], 512, 8, 48, _PH),          # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, crosses, splitk_reduce<4> x1)  [16 x 512 -> 512 @ 32 x 32 in MTUNetPlusPlus f16]
    (2, [72], 512, 44, 48, _PH),          # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2+x1)  [32 x 384 -> 384 @ 32 x 32 in MTUNetPlusPlus f16]
    (8, [384], 8, 12, 512, _PH),          # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, ragged_cit, splitk_reduce<16> x8)  [16 x 24+24+24+24+48 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (8, [192], 8, 12, 512, _PH),          # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [16 x 24+24+24+48 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (8, [64], 8, 48, 512, _PH),           # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, splitk_reduce<64, 16> x8)  [16 x 24+48 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (8, [384], 48, 12, 256, _PH),         # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, ragged_cit, splitk_reduce<16> x2)  [16 x 96+96+96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (8, [96], 96, 12, 384, _PH),          # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x2)  [16 x 96+96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (8, [96], 96, 12, 512, _PH),          # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [16 x 48+48+48+48 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (8, [144], 96, 24, 256, _PH),         # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, ragged_cit, splitk_reduce<16> x8)  [16 x 48+48+48 -> 48 @ 256 x 256 in MTUNetPlusPlus f16]
    (8, [96], 96, 24, 256, _PH),          # conv3x3_wgrad_c8w_kernel<true, 3, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [16 x 96 -> 96 @ 128 x 128 in MTUNetPlusPlus f16]
    (16, [1], 8, 128, 512, _PH),          # conv3x3_wgrad_stem_c8_kernel<true> + splitk_reduce (bands=16, splitk_reduce<64, 16> x2)  [16 x 1 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (7, [8], 320, 44, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x2+x1)  [32 x 96 -> 96 @ 64 x 64 in MTUNetPlusPlus f32]
    (2, [96], 384, 44, 48, _P32),         # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2+x1)  [32 x 96+96+96 -> 96 @ 64 x 64 in MTUNetPlusPlus f32]
    (8, [8], 192, 96, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [32 x 24+24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (5, [72], 8, 256, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x8+x2+x1)  [32 x 24+24+24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (7, [24], 8, 512, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<64, 16> x8+x2+x1)  [32 x 24 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (8, [144], 8, 96, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [32 x 24+24+24+24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (16, [72], 8, 96, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles>=3, splitk_reduce<64, 16> x2)  [32 x 24+48 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
    (8, [192], 40, 44, 48, _P32),         # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x2+x1)  [32 x 48+48+48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (11, [96], 40, 64, 48, _P32),         # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x8+x2+x1)  [32 x 48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (8, [144], 40, 44, 48, _P32),         # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x2+x1)  [32 x 48+48+48 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (8, [72], 40, 96, 48, _P32),          # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [32 x 48 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (32, [24], 40, 96, 48, _P32),         # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce (fixed, tiles>=3, splitk_reduce<64, 16> x8)  [32 x 24 -> 48 @ 128 x 128 in MTUNetPlusPlus f32]
    (5, [320], 512, 12, 8, _P32),         # conv3x3_wgrad_mfma_kernel<1, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x1)  [32 x 512 -> 512 @ 16 x 16 in MTUNetPlusPlus f32]
    (8, [320], 320, 12, 8, _P32),         # conv3x3_wgrad_mfma_kernel<1, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2+x1)  [64 x 384 -> 384 @ 16 x 16 in MTUNetPlusPlus f32]
    (32, [1], 8, 32, 512, _P32),          # conv3x3_wgrad_smallcin_kernel + splitk_reduce (bands=4, splitk_reduce<16> x8)  [32 x 1 -> 24 @ 256 x 256 in MTUNetPlusPlus f32]
]


def _wgrad_plan_case_id(case):
    return _conv3_case_id((W_,) + tuple(case))


@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=_wgrad_plan_case_id)
def test_conv3x3_wgrad_plan_cases_match_fp64(case):
    """The weight-gradient check of test_conv3x3_step_instances_match_fp64 -- the whole batch against fp64 conv2d_weight on the operands the
    kernel reads, _close(dw, ref, 1e-5, 2e-5 * max(1, |ref|max)), run twice bit-identically, launched == planned -- at the shape of the row."""
    test_conv3x3_step_instances_match_fp64((W_,) + tuple(case))


def _wgrad_plan_tables():
    """{table name: {(W_, plan key): the first row that makes it}} of every weight-gradient call this file checks against fp64, the older tables
    first (C8_CASES, C8W_CASES, C8I_CASES, FIXUP_CASES, the wgrad rows of BENCH_CASES and CONV3_STEP_CASES), WGRAD_PLAN_CASES last."""
    tables = {}
    for op, case, kw, table in _reference_tested_conv3x3_calls():
        if op == W_:
            tables.setdefault(table, {}).setdefault((W_, _wgrad_plan_key(ops.conv3x3_case_args(W_, *case, **kw))), (case, kw))
    for case in WGRAD_PLAN_CASES:
        tables.setdefault("WGRAD_PLAN_CASES", {}).setdefault((W_, _wgrad_plan_key(ops.conv3x3_case_args(W_, *case[:5], **case[5]))), case)
    return tables


def _older_wgrad_plan_keys():
    return {key for table, keys in _wgrad_plan_tables().items() if table != "WGRAD_PLAN_CASES" for key in keys}


def _reference_tested_wgrad_plan_keys():
    """The (W_, _wgrad_plan_key) of every weight-gradient call that a test of this file checks against fp64: all the tables of _wgrad_plan_tables."""
    return {key for keys in _wgrad_plan_tables().values() for key in keys}


def _wgrad_plan_surveys():
    return [survey(p) for p in STEP_PROGRAMS] + [survey(STEP_PROGRAMS[0], 64)]


def test_step_programs_launch_only_reference_tested_wgrad_plans():
    """Keys every OP_CONV3_WGRAD op of the surveyed step programs by tests/step_programs.py _wgrad_plan_key -- the kernel_name string + the
    class of the plan mtbc_conv3x3_wgrad_plan reports for the op's own arguments: how the kernel walks its pixels and what reduces its
    partials, which plan_wgrad decides from N and the map size -- : each must be the plan key of a weight-gradient call that a test of this
    file checks against fp64.  A change of plan_wgrad, of the batch or of a map size that gives a launch a plan class no case has fails here,
    named with its program, plan key and shape.  The print-out lists every weight-gradient launch under its plan key with the table that
    answers for it (profiles/conv3x3_step_keys.txt)."""
    answers = {}
    for table, keys in _wgrad_plan_tables().items():
        for key in keys:
            answers.setdefault(key, table)
    assert_all_tested("conv3x3-wgrad-plan", set(answers), _wgrad_plan_surveys(), required=(W_,), answers=answers)


def test_wgrad_plan_cases_are_all_needed():
    """Every row of WGRAD_PLAN_CASES makes a plan key that a surveyed program launches, that no older table makes and that no other row
    makes: no dead and no double rows, and deleting one fails the guard above."""
    older = {**dict.fromkeys(COLLECTORS, ()), PLAN: _older_wgrad_plan_keys()}
    assert_rows_needed("WGRAD_PLAN_CASES", _wgrad_plan_surveys(), older, table_keys(wgrad_plan=WGRAD_PLAN_CASES), [WGRAD_PLAN_CASES])


# ------------------------------------------------------------------ the InstanceNorm + LeakyReLU launches of the step programs, element by element
def _bits16(t, st):
    """fp32 / fp64 values -> int16 storage of their rounding (to nearest even) to the 16-bit type st (1 bf16, 2 fp16)."""
    return (t.float().bfloat16() if st == 1 else t.float().half()).view(torch.int16)


def _from16(i, st):
    """int16 storage of the 16-bit type st -> fp64 values."""
    return i.contiguous().view(torch.bfloat16 if st == 1 else torch.float16).double()


def _c8_of(t, st):
    """(N,C,H,W) values -> MTBC_LAYOUT_C8 int16 storage [N][C/8][H*W][8], built on the CPU."""
    N, C, H, W = t.shape
    return _bits16(t, st).reshape(N, C // 8, 8, H * W).permute(0, 1, 3, 2).contiguous()


def _planes_of(i, shape, st):
    """MTBC_LAYOUT_C8 int16 storage -> fp64 (N,C,H,W)."""
    N, C, H, W = shape
    return _from16(i.reshape(N, C // 8, H * W, 8).permute(0, 1, 3, 2).reshape(N, C, H, W), st)


def _lrelu64(pre, slope):
    return torch.where(pre > 0, pre, pre * slope)


def _inorm_stats64(z, eps):
    mean = z.mean((2, 3), keepdim=True)
    var = ((z - mean) ** 2).mean((2, 3), keepdim=True)          # biased, over H*W
    return mean, 1.0 / torch.sqrt(var + eps)


def _inorm_repair_sign(z, zst, gamma, beta, eps):
    """The kernels decide `pre > 0` in fp32: an element whose fp64 pre lies within rounding of zero could take the other branch and differ
    by the factor slope.  Such elements are not masked; the INPUT is moved on the CPU before the launch: while any element has
    |pre| < 1e-4 (|gamma xhat| + |beta| + 1), it moves away from its plane's mean by one step of its stored type -- or, where that step
    cannot leave the band (fp32 z: a 2^-20 relative step changes pre by ~1e-6), by 2.5 band widths in units of z -- and the statistics
    are recomputed.  (gamma is drawn at least 0.25 away from zero, so that step stays a few 1e-3 of the plane's spread.)  At most three
    passes, none may remain.  Returns the repaired z (fp64, exactly representable in its stored type)."""
    for npass in range(4):
        mean, rstd = _inorm_stats64(z, eps)
        xhat = (z - mean) * rstd
        band = 1e-4 * ((gamma * xhat).abs() + beta.abs() + 1)
        bad = (gamma * xhat + beta).abs() < band
        if not bool(bad.any()):
            return z
        if npass == 3:
            break
        step = z.abs() * 2.0 ** -20 if zst is None else _ulp16(z, zst)
        step = torch.maximum(step, 2.5 * band / (gamma.abs() * rstd))
        away = torch.where(z >= mean, 1.0, -1.0)
        moved = z + away * step
        if zst is None:
            moved = moved.float().double()
        else:
            r = _from16(_bits16(moved, zst), zst)
            moved = torch.where((r - z) * away > 0, r, z + away * _ulp16(z, zst))      # (at least one step of the stored type)
        z = torch.where(bad, moved, z)
    raise AssertionError(f"{int(bad.sum())} elements still within rounding of pre = 0 after three repair passes")


# One case = ONE mtbc_instnorm_lrelu_fwd / _bwd call (+ the deferred reduction behind it): (backward, N, C, H, W, instnorm_case_args keywords).
# Shapes: the smallest that reach the key; the team plans (T, rounds) are those mtbc_instnorm_kernel_name reports on an MI355X and are
# pinned by the guard below through the step programs' own keys, not computed here.
_BF = dict(compute=1, out="c8", z="c8f16")          # the bf16 mode: conv outputs stored as fp16, everything else bf16
_FP = dict(compute=2, out="c8", z="c8")             # the fp16 mode
INORM_CASES = []
_AFF = dict(affine=True, slope=0.1)            # MTUNetPlusPlus: affine norm, slope 0.1 (MONAI ADN); MTnnUNet: no affine, slope 0.01
_NOA = dict(affine=False, slope=0.01)
_DEF = dict(dbias=True, defer=True)            # conv bias gradient from the same pass, parameter gradients reduced later (MTBC_OP_IN_DPARAM)
# ---- forward, the streaming pass behind the conv epilogue's statistics (every forward launch of the 16-bit step programs).
#      stats_slots <= 64: FIN (the workgroup finalizes its own channels), above: the finalize launch in front.  Planes of one and of several
#      workgroups (512 pixels each; 256 windows with the pool), H*W no multiple of either.
for _m, _shapes in ((_BF, [(2, 16, 12, 20), (3, 8, 24, 36)]), (_FP, [(2, 16, 24, 36), (1, 24, 12, 20)])):
    for _slots, _hw in ((5, 0), (64, 1), (65, 1), (130, 0)):
        _N, _C, _H, _W = _shapes[_hw]
        _st = dict(_m, stats_slots=_slots)
        INORM_CASES += [
            (False, _N, _C, _H, _W, dict(_st, **_AFF)),
            (False, _N, _C, _H, _W, dict(_st, **_AFF, planar=True)),
            (False, _N, _C, _H, _W, dict(_st, **_AFF, planar16=True)),
            (False, _N, _C, _H, _W, dict(_st, **_AFF, pool=True)),
            (False, _N, _C, _H, _W, dict(_st, **_AFF, pool=True, planar16=True)),
        ]
        if _m is _BF:
            INORM_CASES += [
                (False, _N, _C, _H, _W, dict(_st, **_NOA)),
                (False, _N, _C, _H, _W, dict(_st, **_NOA, planar=True)),
                (False, _N, _C, _H, _W, dict(_st, **_NOA, planar16=True)),
                (False, _N, _C, _H, _W, dict(_st, **_NOA, pool=True)),
            ]
INORM_CASES += [
    (False, 2, 8, 48, 60, dict(_BF, stats_slots=64, **_AFF, pool=True, planar16=True)),       # 2880 pixels: 6 workgroups per plane group, the last one ragged
    (False, 2, 8, 48, 60, dict(_FP, stats_slots=90, **_AFF, planar16=True)),
    (False, 1, 8, 8, 8, dict(_BF, stats_slots=1, **_NOA, planar=True)),                        # the deepest level: one subset, a quarter of a workgroup
    (False, 1, 8, 6, 10, dict(_BF, stats_slots=3, **_NOA, pool=True, pool_arg=False)),         # the pooled output without argmax codes
]
# ---- forward, the channel-group kernels computing their own statistics (no step program launches them today; every solo block size, teams on
#      planes that are no multiple of 2048 pixels: 96 x 96 = 9 slabs of 1024, 96 x 80 = 15 slabs of 512)
INORM_CASES += [
    (False, 2, 8, 6, 10, dict(compute=1, out="c8", **_AFF)),
    (False, 2, 16, 12, 20, dict(_BF, **_AFF, planar=True)),
    (False, 1, 8, 24, 36, dict(_FP, **_NOA)),
    (False, 1, 8, 48, 60, dict(compute=1, out="c8", z="c8", **_AFF, planar=True)),
    (False, 1, 8, 96, 96, dict(_BF, **_AFF, planar=True)),
    (False, 1, 8, 96, 80, dict(_FP, **_AFF)),
]
# ---- forward / backward, the fp32 kernels of norm.hip (the parity mode): every (VPT, block size) the dispatcher chooses, planes that fill the
#      last block partly.  Backward in place over dy, as the step programs run it.
_F32B = dict(**_AFF, dbias=True, inplace=True)
INORM_CASES += [
    (False, 2, 3, 12, 20, _AFF), (False, 2, 3, 28, 36, _AFF), (False, 2, 3, 60, 68, _AFF), (False, 1, 3, 120, 136, _AFF), (False, 1, 2, 250, 260, _AFF),
    (True, 2, 3, 12, 20, _F32B), (True, 2, 3, 32, 32, _F32B), (True, 2, 3, 60, 68, _F32B), (True, 1, 3, 128, 128, _F32B), (True, 1, 2, 250, 260, _F32B),
    (True, 2, 3, 7, 9, dict(**_NOA, n_extra=2)),                     # in_bwd_kernel<false>: H*W % 4 != 0, two more gradient contributions, no parameters
]
# ---- backward, one workgroup per (image, channel group): planes up to 64 x 64.  bf16 mode: z stored as fp16 (ZC8 = 2); fp16 mode: ZC8 = 1.
for _N, _C, _H, _W in ((2, 16, 12, 20), (2, 8, 24, 36), (1, 16, 48, 60)):
    INORM_CASES += [
        (True, _N, _C, _H, _W, dict(_BF, **_NOA)),
        (True, _N, _C, _H, _W, dict(_BF, **_NOA, pool=True)),
        (True, _N, _C, _H, _W, dict(_BF, **_AFF, **_DEF)),
    ]
INORM_CASES += [
    (True, 2, 8, 24, 36, dict(_BF, **_AFF, **_DEF, pool=True)),
    (True, 1, 16, 48, 60, dict(_BF, **_AFF, **_DEF, pool=True)),
    (True, 3, 8, 6, 10, dict(_BF, **_NOA)),
    (True, 2, 8, 24, 36, dict(_FP, **_AFF, **_DEF)),
    (True, 1, 16, 48, 60, dict(_FP, **_AFF, **_DEF)),
    (True, 1, 16, 48, 60, dict(_FP, **_AFF, **_DEF, pool=True)),
    (True, 2, 8, 24, 36, dict(_BF, **_AFF, dbias=True, acc=True)),                                   # immediate reduction onto prefilled gradients (shared modules)
    (True, 2, 8, 24, 36, dict(_BF, **_AFF, dy="c8", n_extra=1, rank1=True, rank1_grads=True, rank1_acc=True, pool=True, dbias=True)),      # DY8 = 2, every folded term at once
    (True, 2, 8, 12, 20, dict(_FP, **_AFF, dy="c8", **_DEF)),                                        # DY8 = 1
]
# ---- backward, teams.  reserve_cus leaves one to three teams resident, so that a few items already take several rounds over the mailbox
#      (the step programs: 96 .. 192 items on 24 teams and fewer); the same instance in one round beside it.
#      "rounds" (not an argument: the test's expectation of the plan the query reports, 1 or ">1") is asserted after the launch.
_T32, _T8, _T128 = (1, 16, 256, 256, 240), (2, 24, 128, 128, 248), (1, 16, 512, 512, 192)
_R1 = dict(rank1=True, rank1_grads=True)
for _m, _plans in ((_BF, (_T32, _T8)), (_FP, (_T32, _T8, _T128))):
    for _N, _C, _H, _W, _r in _plans:
        INORM_CASES += [
            (True, _N, _C, _H, _W, dict(_m, **_AFF, **_DEF, reserve_cus=_r, rounds=">1")),
            (True, _N, _C, _H, _W, dict(_m, **_AFF, **_DEF, pool=True, reserve_cus=_r, rounds=">1")),
        ]
        if _m is _BF:
            INORM_CASES += [
                (True, _N, _C, _H, _W, dict(_m, **_NOA, reserve_cus=_r, rounds=">1")),
                (True, _N, _C, _H, _W, dict(_m, **_NOA, pool=True, reserve_cus=_r, rounds=">1")),
            ]
for _m, (_N, _C, _H, _W, _r) in ((_BF, _T32), (_FP, _T128)):          # the level-0 tensors a one-output 1x1 head reads: its gradient and its own dW / db from the same pass
    INORM_CASES += [
        (True, _N, _C, _H, _W, dict(_m, **_AFF, **_DEF, **_R1, reserve_cus=_r, rounds=">1")),
        (True, _N, _C, _H, _W, dict(_m, **_AFF, **_DEF, **_R1, dy=None, reserve_cus=_r, rounds=">1")),
    ]
INORM_CASES += [
    (True, 1, 16, 256, 256, dict(_BF, **_NOA, **_R1, dy=None, reserve_cus=240, rounds=">1")),
    (True, 1, 16, 256, 256, dict(_BF, **_AFF, **_DEF, **_R1, rounds=1)),                              # the instance and arguments of the _T32 rank-1 case above, every team resident: ONE round
    (True, 2, 24, 256, 256, dict(_BF, **_AFF, **_DEF, **_R1, pool=True, rounds=1)),                   # every folded term at once, 6 items in one round
    (True, 2, 24, 256, 256, dict(_BF, **_AFF, **_DEF, **_R1, pool=True, reserve_cus=64, rounds=1)),   # ... and with the data-parallel reserve
    (True, 1, 8, 96, 96, dict(_BF, **_AFF, **_DEF, pool=True)),                                       # planes that are no multiple of 2048 pixels
    (True, 1, 8, 96, 80, dict(_FP, **_AFF, dbias=True, **_R1, rank1_acc=True)),
]
# ---- 16-bit PLANES out of the fp32-z kernels of norm.hip (y16 / dz16 without y8 / dz8: what a 16-bit cell runs when the channel-group kernels
#      do not take its shape): the same instances as the fp32 cases above, stored through in_cvt4
for _c in (1, 2):
    INORM_CASES += [
        (False, 2, 3, 12, 20, dict(compute=_c, out="p16", **_AFF)), (False, 2, 3, 60, 68, dict(compute=_c, out="p16", **_NOA)),
        (False, 1, 2, 250, 260, dict(compute=_c, out="p16", **_AFF)),
        (True, 2, 3, 12, 20, dict(compute=_c, out="p16", **_AFF, dbias=True)), (True, 2, 3, 60, 68, dict(compute=_c, out="p16", **_NOA, dbias=True)),
        (True, 1, 2, 250, 260, dict(compute=_c, out="p16", **_AFF, dbias=True, n_extra=1)),
    ]
# ---- backward, the streaming pass behind a gathered dgrad's epilogue sums (no step program launches it today): dbias_pre is exactly zero
INORM_CASES += [
    (True, 2, 16, 24, 36, dict(_BF, **_AFF, dy="c8", dbias=True, stats_slots=7)),
    (True, 1, 8, 48, 60, dict(_FP, **_NOA, dy="c8", dbias=True, stats_slots=70)),
]


def _inorm_case_id(case):
    b, N, C, H, W, mode = case
    return ("bwd" if b else "fwd") + f"-{N}x{C}x{H}x{W}-" + ",".join(f"{k}={v}" for k, v in mode.items())


def _inorm_args(backward, N, C, H, W, mode, ptrs=None):
    return ops.instnorm_case_args(backward, N, C, H, W, ptrs=ptrs, **{k: v for k, v in mode.items() if k != "rounds"})


def _inorm_case_calls(case):
    """[(op, launches as mtbc_instnorm_kernel_name plans them, coverage key)] of the calls a case makes, from dummy arguments (nothing is launched)."""
    backward, N, C, H, W, mode = case
    a = _inorm_args(backward, N, C, H, W, mode)
    calls = [(ops.L.OP_IN_BWD if backward else ops.L.OP_IN_FWD, ops.instnorm_kernel_name(a, backward), _instnorm_key(a, backward))]
    if backward and mode.get("defer"):
        calls.append((ops.L.OP_IN_DPARAM, "in_dparam_many_kernel", _dparam_key(ops.instnorm_dparam_desc(a, 1 << 20)[0])))
    return calls


@pytest.mark.parametrize("case", INORM_CASES, ids=_inorm_case_id)
def test_instnorm_step_instances_match_fp64(case):
    """Every InstanceNorm + LeakyReLU launch of the benchmark's step programs (test_step_programs_launch_only_reference_tested_instnorm_
    instances) against a plain fp64 computation of the WHOLE fused operation on the CPU, on the stored inputs (z / dy rounded to their 16-bit
    types where the launch reads 16 bits; mean / rstd of the backward = the fp64 statistics rounded to fp32) -- nothing a HIP kernel computed
    enters the reference.  Forward: biased statistics over H*W, y = lrelu(gamma xhat + beta), the 2 x 2 max-pool of the STORED y and the first
    maximum's position.  Backward: g = (dy + dy_extra + w[c] dyhead + routed pool gradient) * (pre > 0 ? 1 : slope),
    dz = gamma rstd (g - mean g - xhat mean(g xhat)), dgamma = sum g xhat, dbeta = sum g, dbias_pre = sum dz, head dW = sum y_stored dyhead,
    head db = sum dyhead; "accumulate" adds onto prefilled values; deferred parameter gradients are read after mtbc_instnorm_dparam_many.
    Bounds: 16-bit stored outputs one unit in the last place of the stored type + 1e-5 x scale, fp32 outputs 1e-5 x scale, argmax codes
    exact, the parameter gradients as in the tests of the single features; outputs a call does not ask for stay untouched.  `made` is what
    mtbc_instnorm_kernel_name says for the REAL arguments just before each call (ops.launched), `planned` the same query on the table's entry
    with dummy pointers: the launches are not observed -- that name and launch agree rests on the dispatchers launching from the NormChoice
    they print."""
    backward, N, C, H, W, mode = case
    L = ops.L
    compute, out, zkind = mode.get("compute", 0), mode.get("out", "f32"), mode.get("z", "f32")
    affine, eps, slope = mode.get("affine", True), mode.get("eps", 1e-5), mode.get("slope", 0.01)
    zst = None if zkind == "f32" else (2 if zkind == "c8f16" else compute)
    HW, G8 = H * W, C // 8
    g = _g(N * 7919 + C * 131 + H * 17 + W + 3 * compute + int(backward))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)       # noqa: E731
    gamma = (1.0 + 0.3 * rn(C)) if affine else torch.ones(C, dtype=torch.float64)
    gamma = torch.where(gamma.abs() < 0.25, torch.where(gamma < 0, -0.25, 0.25), gamma)       # (the repair step divides by |gamma|)
    beta = 0.3 * rn(C) if affine else torch.zeros(C, dtype=torch.float64)
    gamma, beta = gamma.float().double().view(1, C, 1, 1), beta.float().double().view(1, C, 1, 1)
    z = rn(N, C, H, W) * (0.5 + torch.rand(1, C, 1, 1, generator=g, dtype=torch.float64)) + 0.5 * rn(1, C, 1, 1)
    z = z.float().double() if zst is None else _from16(_bits16(z, zst), zst)
    z = _inorm_repair_sign(z, zst, gamma, beta, eps)
    mean, rstd = _inorm_stats64(z, eps)

    dev = {}            # field name -> device tensor (ops.instnorm_case_args(ptrs=...))
    nan32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)      # noqa: E731
    nan16 = lambda *s: torch.full(s, -1, dtype=torch.int16, device=DEV)                    # noqa: E731  (0xffff: a NaN of both types)
    dev["z"] = (z.float() if zst is None else _c8_of(z, zst)).to(DEV)
    if affine:
        dev["gamma"], dev["beta"] = gamma.flatten().float().to(DEV), beta.flatten().float().to(DEV)
    if out == "c8":
        dev["coop_state"] = ops.coop_state(DEV)
    oH, oW = H // 2, W // 2
    pos = ((torch.arange(H) & 1) << 1).view(H, 1) | (torch.arange(W) & 1).view(1, W)       # a pixel's position in its 2 x 2 window

    if not backward:
        dev["mean"], dev["rstd"] = nan32(N * C), nan32(N * C)
        slots = mode.get("stats_slots", 0)
        if slots:       # what the conv epilogue leaves: {sum, sum of squares} of the stored z per (image, pixel subset, channel), fp32
            parts = torch.tensor_split(z.reshape(N, C, HW), slots, dim=2)
            dev["stats_partial"] = torch.stack([torch.stack([p_.sum(2), (p_ * p_).sum(2)], dim=2) for p_ in parts], dim=1).float().to(DEV)
        for name, shape in (("y8", (N, G8, HW, 8)), ("y16", (N, C, H, W)), ("pool_y8", (N, G8, oH * oW, 8)), ("pool_arg", (N, G8, oH * oW))):
            dev[name] = nan16(*shape)
        dev["y"] = nan32(N, C, H, W)
        a = _inorm_args(False, N, C, H, W, mode)           # (dummy pointers: is the chunked-statistics workspace wanted?)
        dev["workspace"] = torch.empty(max(4, a.workspace_bytes // 4), dtype=torch.float32, device=DEV)
    else:
        dev["mean"], dev["rstd"] = mean.flatten().float().to(DEV), rstd.flatten().float().to(DEV)
        mean, rstd = mean.float().double(), rstd.float().double()       # the backward's inputs are the stored fp32 statistics
        dykind = mode.get("dy", "f32")
        gsum = torch.zeros(N, C, H, W, dtype=torch.float64)
        if dykind is not None:
            dy = rn(N, C, H, W)
            dy = _from16(_bits16(dy, compute), compute) if dykind == "c8" else dy.float().double()
            dev["dy"] = (_c8_of(dy, compute) if dykind == "c8" else dy.float()).to(DEV)
            gsum += dy
        for k in range(mode.get("n_extra", 0)):
            e = (0.5 * rn(N, C, H, W)).float().double()
            dev[f"dy_extra{k}"] = e.float().to(DEV)
            gsum += e
        if mode.get("rank1"):
            dyh, wh = rn(N, 1, H, W).float().double(), (0.5 * rn(C)).float().double()
            dev["dy_rank1"], dev["dy_rank1_w"] = dyh.float().to(DEV), wh.float().to(DEV)
            gsum += wh.view(1, C, 1, 1) * dyh
            hdw0, hdb0 = rn(C).float(), rn(1).float()               # prefilled: "accumulate" adds onto them, otherwise overwritten
            dev["dy_rank1_dw"], dev["dy_rank1_db"] = hdw0.to(DEV), hdb0.to(DEV)
        if mode.get("pool"):
            pg = rn(N, C, oH, oW).float().double()
            code = torch.randint(0, 4, (N, C, oH, oW), generator=g)
            up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)       # noqa: E731
            gsum += torch.where(up(code) == pos, up(pg), torch.zeros((), dtype=torch.float64))
            packed = (code.reshape(N, G8, 8, oH * oW) << (2 * torch.arange(8)).view(1, 1, 8, 1)).sum(2)
            dev["dy_pool"], dev["dy_pool_arg"] = pg.float().to(DEV), torch.where(packed >= 32768, packed - 65536, packed).to(torch.int16).to(DEV)
        dg0, db0, dbp0 = rn(C).float(), rn(C).float(), rn(C).float()
        dev["dgamma"], dev["dbeta"], dev["dbias_pre"] = dg0.to(DEV), db0.to(DEV), dbp0.to(DEV)
        dev["dz8"], dev["dz16"], dev["dz"] = nan16(N, G8, HW, 8), nan16(N, C, H, W), nan32(N, C, H, W)
        dev["workspace"] = torch.empty(N * (C + 1) * 262, dtype=torch.float32, device=DEV)

    if backward and mode.get("stats_slots"):        # what a gathered dgrad's epilogue leaves: {sum g, sum g xhat} per (image, pixel subset, channel), fp32
        gy_, xh_ = (gsum * torch.where(gamma * ((z - mean) * rstd) + beta > 0, 1.0, slope)).reshape(N, C, HW), ((z - mean) * rstd).reshape(N, C, HW)
        parts = zip(torch.tensor_split(gy_, mode["stats_slots"], dim=2), torch.tensor_split(xh_, mode["stats_slots"], dim=2))
        dev["stats_partial"] = torch.stack([torch.stack([g_.sum(2), (g_ * x_).sum(2)], dim=2) for g_, x_ in parts], dim=1).float().to(DEV)
    a = _inorm_args(backward, N, C, H, W, mode, ptrs=dev)
    outputs = ("y", "y8", "y16", "pool_y8", "pool_arg") if not backward else ("dz", "dz8", "dz16", "dgamma", "dbeta", "dbias_pre", "dy_rank1_dw", "dy_rank1_db")
    unasked = {n: dev[n].clone() for n in outputs if n in dev and not getattr(a, n)}        # their pointers are NULL in `a`: nothing may write them
    ops.launched = []
    try:
        ops.instnorm_launch(a, backward)
        if backward and mode.get("defer"):
            ops.instnorm_dparam_many(ops.instnorm_dparam_desc(a, dev["workspace"].data_ptr()))
        torch.cuda.synchronize()
        made = list(ops.launched)
    finally:
        ops.launched = None
    planned = _inorm_case_calls(case)
    print(_inorm_case_id(case), "->", made)
    assert made == [(op, name) for op, name, _ in planned], (made, planned)
    assert _instnorm_key(a, backward) == planned[0][2]          # the same argument-selected branches as the table's entry
    assert ops.coop_error(DEV) == 0
    if "rounds" in mode:        # the plan the case is in the table for
        rounds = int(re.search(r"rounds=(\d+)", made[0][1]).group(1))
        assert (rounds == 1) if mode["rounds"] == 1 else (rounds > 1), made[0][1]
    for n, before in unasked.items():
        assert torch.equal(dev[n].view(torch.int16), before.view(torch.int16)), f"{n} was not asked for and was written"

    xhat = (z - mean) * rstd
    pre = gamma * xhat + beta
    y = _lrelu64(pre, slope)

    def stored16(got, ref, st, what):
        bound = _ulp16(ref, st) + 1e-5 * ref.abs().max().item()
        worst = ((got - ref).abs() / bound).max().item()
        print(f"  {what}: {worst:.3f} x (one ulp of the stored type + 1e-5 x scale)")
        assert worst <= 1.0, f"{what}: {worst:.3f} x (one ulp of the stored type + 1e-5 x scale)"

    def fp32(got, ref, what):
        err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
        print(f"  {what}: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 1e-5 * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"

    if not backward:
        _close(dev["mean"], mean.flatten().float(), 1e-5, 1e-5 * max(1.0, z.abs().max().item()), "mean")
        _close(dev["rstd"], rstd.flatten().float(), 3e-5, 0.0, "rstd")
        if out == "c8":
            stored16(_planes_of(dev["y8"].cpu(), (N, C, H, W), compute), y, compute, "y8")
            if mode.get("planar16"):
                stored16(_from16(dev["y16"].cpu(), compute), y, compute, "y16")
            elif mode.get("planar"):
                fp32(dev["y"].cpu(), y, "y")
            if mode.get("pool"):
                win = _from16(_bits16(y, compute), compute).reshape(N, C, oH, 2, oW, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, oH, oW, 4)
                stored16(_planes_of(dev["pool_y8"].cpu(), (N, C, oH, oW), compute), win.max(4).values, compute, "pool_y8")
                if mode.get("pool_arg", True):
                    got = (dev["pool_arg"].cpu().int() & 0xffff).view(N, G8, 1, oH * oW) >> (2 * torch.arange(8, dtype=torch.int32)).view(1, 1, 8, 1) & 3
                    assert torch.equal(got.reshape(N, C, oH, oW).long(), win.argmax(4)), "pool_arg"        # (torch.argmax: the first maximum)
        elif out == "p16":
            stored16(_from16(dev["y16"].cpu(), compute), y, compute, "y16")
        else:
            fp32(dev["y"].cpu(), y, "y")
        return

    gy = gsum * torch.where(pre > 0, 1.0, slope)
    m1, m2 = gy.mean((2, 3), keepdim=True), (gy * xhat).mean((2, 3), keepdim=True)
    dz = gamma * rstd * (gy - m1 - xhat * m2)
    if out == "c8":
        stored16(_planes_of(dev["dz8"].cpu(), (N, C, H, W), compute), dz, compute, "dz8")
    elif out == "p16":
        stored16(_from16(dev["dz16"].cpu(), compute), dz, compute, "dz16")
    else:
        fp32(dev["dy" if mode.get("inplace") else "dz"].cpu(), dz, "dz")
    pre_acc = 1.0 if mode.get("acc") else 0.0
    if affine:
        dg_ref, db_ref = (gy * xhat).sum((0, 2, 3)) + pre_acc * dg0.double(), gy.sum((0, 2, 3)) + pre_acc * db0.double()
        _close(dev["dgamma"], dg_ref.float(), 1e-4, 1e-3 * max(1.0, dg_ref.abs().max().item()), "dgamma")
        _close(dev["dbeta"], db_ref.float(), 1e-4, 1e-3 * max(1.0, db_ref.abs().max().item()), "dbeta")
    if mode.get("dbias"):
        if mode.get("stats_slots"):          # in front of a norm the conv-bias gradient is mathematically zero: written as exact zeros
            assert torch.equal(dev["dbias_pre"].cpu(), torch.zeros(C)), "dbias_pre with stats_partial"
        ref = dz.sum((0, 2, 3)) + pre_acc * dbp0.double()
        err, bound = (dev["dbias_pre"].cpu().double() - ref).abs().max().item(), max(1e-3, 1e-6 * dz.abs().sum((0, 2, 3)).max().item())
        print(f"  dbias_pre: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"dbias_pre: max err {err:.3e}, bound {bound:.3e}"
    if mode.get("rank1") and mode.get("rank1_grads"):
        r1_acc = 1.0 if mode.get("rank1_acc") else 0.0
        hdw = (_from16(_bits16(y, compute), compute) * dyh).sum((0, 2, 3)) + r1_acc * hdw0.double()
        hdb = dyh.sum().view(1) + r1_acc * hdb0.double()
        _close(dev["dy_rank1_dw"], hdw.float(), 2e-4, 2e-4 * max(1.0, hdw.abs().max().item()), "head dW")
        _close(dev["dy_rank1_db"], hdb.float(), 2e-4, 2e-4 * max(1.0, hdb.abs().max().item()), "head db")


def _reference_tested_instnorm_keys():
    """(op, key) of every call test_instnorm_step_instances_match_fp64 makes, from its case table."""
    return {(op, key) for case in INORM_CASES for op, _, key in _inorm_case_calls(case)}


def test_step_programs_launch_only_reference_tested_instnorm_instances():
    """Surveys (builds, does not run) the benchmark's four step programs, and the first one as a data-parallel rank builds it
    (coop_reserve_cus = 64), for the coverage key of every MTBC_OP_IN_FWD / _IN_BWD / _IN_DPARAM op: each must be the key of a call that
    test_instnorm_step_instances_match_fp64 makes.  A plan change -- another instance, team size, a second round, a new argument-selected
    branch -- that no fp64 case reaches fails here; _instnorm_key / _dparam_key (tests/step_programs.py), INORM_CASES and
    _reference_tested_instnorm_keys are the places to edit.  A missing key is named with (N, C, H, W) of an op that has it ((N, C) of a
    parameter-gradient reduction)."""
    tested = _reference_tested_instnorm_keys()
    one, many = ({(k[0].replace(r, "rounds"), k[1]) for _, k in tested if r in k[0]} for r in ("rounds=1", "rounds>1"))
    assert one & many, "no instance is tested both in one round and in several with the same arguments"
    assert_all_tested("InstanceNorm", tested, [survey(p) for p in STEP_PROGRAMS] + [survey(STEP_PROGRAMS[0], 64)],
                      required=(ops.L.OP_IN_FWD, ops.L.OP_IN_BWD))


# ------------------------------------------------------------------ the transposed-convolution launches of the step programs, element by element
# (kind, N, Cin, Cout, H, W, k, mode, strided): kind "fwd" / "dgrad" / "wgrad" = one call through ops.convT_launch, "pair" = [OP_CONVT_WGRAD,
# OP_CONVT_DGRAD] through engine.Program (the fused kernel where the runner takes the pair, the two calls' launches otherwise).  mode: the
# keywords of ops.convT_case_args.  strided: the activation tensors that are channel ranges [8, 8 + C) of a buffer 16 channels wider.  Each
# row is the smallest problem that reaches its instance and still has the structure that can go wrong there: steps are 32 pixels, the weight
# gradient's plan gives a split at least 8 steps, so N * H * W / 256 splits; input channels go in blocks of 48, output channels in tiles of 8.
_B16 = dict(compute=1, dy16=True, x16=True)          # the 16-bit modes' backward: dy and x as 16-bit planes of the compute type
_F16 = dict(compute=2, dy16=True, x16=True)
_XY, _DYDX, _XDY, _ALL = ("x", "y"), ("dy", "dx"), ("x", "dy"), ("x", "dy", "dx")
CONVT_CASES = [
    # ---- forward, 16-bit MFMA on channel-blocked x and y: convT2_fwd_lp_c8_kernel<MTC, F16>, MTC by the LDS budget
    ("fwd", 3, 96, 48, 8, 16, 2, dict(compute=1, x_c8=True, y_c8=True), _XY),                  # MTC = 3; 12 tasks = 3 blocks; x and y views
    ("fwd", 2, 56, 40, 16, 16, 2, dict(compute=2, x_c8=True, y_c8=True), ()),                  # MTC = 3; Cin = 56: 8 kpad columns; Cout % 16 == 8: padded last tile with bias
    ("fwd", 2, 128, 128, 8, 8, 2, dict(compute=1, x_c8=True, y_c8=True), ()),                  # MTC = 3, dense; MTnnUNet's 128 -> 128: the third channel block 32 of 48 wide
    ("fwd", 2, 192, 96, 8, 8, 2, dict(compute=1, x_c8=True, y_c8=True), ()),                   # MTC = 2 by LDS (Cin = 192); three channel blocks
    ("fwd", 2, 224, 64, 8, 8, 2, dict(compute=1, x_c8=True, y_c8=True, bias=False), _XY),      # MTC = 2 at the first Cin that needs it; views; no bias
    ("fwd", 2, 48, 48, 8, 16, 2, dict(compute=2, x_c8=True, y_c8=True), ("y",)),               # MTC = 3, fp16: the U-Net++ 48 -> 48 into a view
    ("fwd", 2, 256, 40, 8, 8, 2, dict(compute=2, x_c8=True, y_c8=True), ()),                   # MTC = 2 by LDS (Cin = 256), dense; Cout % 16 == 8
    ("fwd", 3, 40, 24, 8, 16, 2, dict(compute=2, x_c8=True, y_c8=True), _XY),                  # MTC = 2 by Cout; Cin = 40: 24 kpad columns; Cout % 16 == 8
    ("fwd", 1, 384, 192, 8, 8, 2, dict(compute=1, x_c8=True, y_c8=True), ()),                  # MTC = 1 by LDS (Cin = 384): 12 channel blocks
    ("fwd", 2, 320, 320, 8, 8, 2, dict(compute=1, x_c8=True, y_c8=True, bias=False), _XY),     # MTC = 1, MTnnUNet's 320-wide level (kpad = 320); no bias
    ("fwd", 1, 288, 64, 8, 8, 2, dict(compute=2, x_c8=True, y_c8=True), ()),                   # MTC = 1 by LDS at the first Cin that needs it, dense
    ("fwd", 2, 24, 8, 8, 16, 2, dict(compute=2, x_c8=True, y_c8=True), _XY),                   # MTC = 1 by Cout = 8: half a channel tile
    # ---- forward, fp32 x into a channel-blocked 16-bit y: convT2_fwd_c8_kernel<KI, F16>
    ("fwd", 2, 24, 24, 8, 16, 2, dict(compute=1, y_c8=True), _XY),                             # KI = 8; Cout % 16 == 8
    ("fwd", 2, 32, 40, 16, 16, 2, dict(compute=2, y_c8=True, bias=False), ("x",)),             # KI = 8 full; Cout % 16 == 8, no bias
    ("fwd", 3, 48, 48, 8, 16, 2, dict(compute=1, y_c8=True), _XY),                             # KI = 12; the U-Net++ 48 -> 48
    ("fwd", 2, 40, 8, 16, 16, 2, dict(compute=2, y_c8=True), _XY),                             # KI = 12 ragged (10 of 12); Cout = 8
    ("fwd", 2, 64, 48, 8, 8, 2, dict(compute=1, y_c8=True), _XY),                              # KI = 16 full
    ("fwd", 2, 56, 24, 16, 16, 2, dict(compute=2, y_c8=True), _XY),                            # KI = 16 ragged (14 of 16)
    # ---- forward, fp32: convT2_fwd_lds_kernel<KI> and the generic GEMM convT_fwd_kernel<k>
    ("fwd", 2, 20, 12, 8, 16, 2, {}, ()),                                                      # KI = 8 ragged
    ("fwd", 3, 48, 48, 16, 16, 2, {}, _XY),                                                    # KI = 12
    ("fwd", 2, 48, 24, 8, 16, 2, {}, ()),                                                      # KI = 12, dense
    ("fwd", 2, 64, 40, 8, 8, 2, dict(bias=False), _XY),                                        # KI = 16, no bias
    ("fwd", 2, 96, 48, 8, 8, 2, {}, _XY),                                                      # generic k = 2: Cin above the LDS kernel's 64
    ("fwd", 2, 20, 12, 6, 10, 2, dict(bias=False), ()),                                        # generic k = 2: a 60-pixel map (one ragged 64-column block)
    ("fwd", 2, 96, 48, 6, 10, 2, {}, ()),                                                      # generic k = 2, dense, with bias
    ("fwd", 2, 64, 1, 8, 8, 4, {}, ()),                                                        # the fused heads, dense: Cout = 1, k = 4
    ("fwd", 2, 32, 1, 8, 8, 2, {}, ("x",)),                                                    # the fused heads: Cout = 1, M = 4 rows
    ("fwd", 2, 64, 1, 6, 10, 4, {}, ("x",)),                                                   # ... k = 4: M = 16
    ("fwd", 2, 128, 1, 4, 4, 8, {}, ()),                                                       # ... k = 8: M = 64
    ("fwd", 2, 16, 3, 4, 4, 8, {}, _XY),                                                       # generic k = 8, Cout > 1, views
    ("fwd", 3, 24, 5, 5, 9, 4, {}, ()),                                                        # generic k = 4, Cout > 1, odd map
    # ---- dgrad, 16-bit dy: weights in LDS (Cout % 8 == 0 and <= 256), else the direct kernel with D = 2 | 4
    ("dgrad", 3, 48, 48, 8, 16, 2, dict(compute=1, dy16=True), _DYDX),                         # convT2_dgrad_lds_kernel<1, 4>; 12 tasks; views
    ("dgrad", 2, 64, 256, 8, 8, 2, dict(compute=2, dy16=True, acc_dx=True), _DYDX),            # <2, 4>: the last Cout with weights in LDS; ragged second input block
    ("dgrad", 2, 96, 192, 8, 8, 2, dict(compute=1, dy16=True, acc_dx=True), ("dy",)),          # <1, 4>, accumulate, two input blocks
    ("dgrad", 2, 48, 320, 8, 8, 2, dict(compute=1, dy16=True), _DYDX),                         # direct <1, true, 4>: MTnnUNet's 320-wide level, past the LDS gate
    ("dgrad", 1, 320, 320, 8, 16, 2, dict(compute=2, dy16=True, acc_dx=True), _DYDX),          # direct <2, true, 4>; ragged last input block (320 = 6 x 48 + 32)
    ("dgrad", 2, 40, 20, 8, 16, 2, dict(compute=1, dy16=True), _DYDX),                         # direct <1, true, 2>: Cout % 8 != 0
    ("dgrad", 3, 24, 12, 8, 8, 2, dict(compute=2, dy16=True, acc_dx=True), _DYDX),             # direct <2, true, 2>
    # ---- dgrad, fp32 dy: convT2_dgrad_kernel<LP, false, 2> and the generic GEMM
    ("dgrad", 2, 48, 24, 8, 16, 2, {}, _DYDX),                                                 # <0>
    ("dgrad", 2, 56, 40, 8, 8, 2, dict(compute=1, acc_dx=True), _DYDX),                        # <1>
    ("dgrad", 2, 96, 48, 8, 8, 2, dict(compute=2), _DYDX),                                     # <2>
    ("dgrad", 2, 20, 12, 6, 10, 2, dict(acc_dx=True), ()),                                     # generic k = 2 (60-pixel map)
    ("dgrad", 2, 32, 1, 8, 8, 2, {}, ("dx",)),                                                 # the fused heads: Cout = 1 (odd: never the direct kernel), K = 4
    ("dgrad", 2, 32, 1, 8, 16, 2, {}, ()),                                                     # ... as the programs have them: dense, stored; two column blocks
    ("dgrad", 2, 64, 1, 6, 10, 4, {}, ()),
    ("dgrad", 2, 128, 1, 4, 4, 8, {}, ()),
    ("dgrad", 2, 64, 1, 6, 10, 4, dict(acc_dx=True), ("dx",)),                                 # ... k = 4
    ("dgrad", 2, 128, 1, 4, 4, 8, dict(acc_dx=True), ("dx",)),                                 # ... k = 8
    ("dgrad", 3, 24, 5, 5, 9, 4, {}, ()),                                                      # generic k = 4, Cout > 1
    # ---- wgrad, x and dy as 16-bit planes: convT2_wgrad16_kernel<LP, 2, 2> (even tile count) / <LP, 1, 4> (odd), XCD task order from 8 splits
    ("wgrad", 1, 48, 48, 16, 16, 2, _B16, ()),                                                 # <1, 2, 2>, 8 steps: one split, stored straight
    ("wgrad", 3, 64, 16, 16, 24, 2, dict(_F16, acc_dw=True, bias=False), _XDY),                # <2, 2, 2>, 36 steps: 5 splits, the last short, straddling images
    ("wgrad", 2, 96, 32, 32, 32, 2, dict(_B16, acc_dw=True), ()),                              # <1, 2, 2> xcd: 8 splits, one per XCD
    ("wgrad", 3, 48, 192, 24, 40, 2, dict(_F16, bias=False), _XDY),                            # <2, 2, 2> xcd: 90 steps = 12 splits (4 phantoms), the last 2 steps
    ("wgrad", 2, 40, 24, 8, 16, 2, dict(_B16, bias=False), _XDY),                              # <1, 1, 4>: one split; ragged input block
    ("wgrad", 3, 56, 40, 16, 24, 2, dict(_F16, acc_dw=True), ()),                              # <2, 1, 4>: 5 splits, short last
    ("wgrad", 3, 48, 8, 32, 32, 2, dict(_B16, acc_dw=True), _XDY),                             # <1, 1, 4> xcd: 12 splits (4 phantoms); Cout = 8
    ("wgrad", 3, 64, 24, 24, 40, 2, _F16, _XDY),                                               # <2, 1, 4> xcd: 12 splits, the last 2 steps
    # ---- wgrad, 16-bit dy with fp32 x, fp32 operands, and the generic GEMM
    ("wgrad", 3, 48, 24, 16, 24, 2, dict(compute=1, dy16=True), _XDY),                         # convT2_wgrad_kernel<1, true, 2>, 5 splits
    ("wgrad", 2, 96, 48, 8, 16, 2, dict(compute=2, dy16=True, acc_dw=True, bias=False), _XDY), # <2, true, 2>, one split
    ("wgrad", 3, 20, 12, 16, 24, 2, {}, _XDY),                                                 # <0, false, 2>: ragged input block and channel tile
    ("wgrad", 2, 48, 48, 8, 16, 2, dict(compute=1, acc_dw=True), _XDY),                        # <1, false, 2>
    ("wgrad", 1, 96, 40, 16, 16, 2, dict(compute=2, bias=False), ("x",)),                      # <2, false, 2>
    ("wgrad", 2, 32, 1, 8, 16, 2, {}, ("x",)),                                                 # the k = 2 head: Cout = 1 takes the direct kernel (one eighth of a tile)
    ("wgrad", 3, 32, 1, 16, 24, 2, {}, ()),                                                    # ... dense, 5 splits
    ("wgrad", 2, 64, 1, 6, 10, 4, {}, ()),                                                     # the fused heads on the generic kernel as the programs have them: dense
    ("wgrad", 2, 128, 1, 4, 4, 8, {}, ()),
    ("wgrad", 2, 20, 12, 6, 10, 2, dict(acc_dw=True), ()),                                     # generic k = 2 + channel_sums
    ("wgrad", 2, 32, 1, 6, 10, 2, {}, ("x",)),                                                 # the fused heads on the generic kernel: Cout = 1
    ("wgrad", 2, 64, 1, 6, 10, 4, {}, ("x",)),                                                 # ... k = 4
    ("wgrad", 2, 128, 1, 4, 4, 8, dict(bias=False), _XDY),                                     # ... k = 8
    ("wgrad", 3, 24, 5, 5, 9, 4, dict(acc_dw=True), ()),                                       # generic k = 4, Cout > 1
    # ---- the program runner's pair, fused: convT2_bwd_fused_kernel<LP, CT, NW, ACC>; the grid is 8 x cdiv(splits, 8) x input blocks
    ("pair", 2, 64, 24, 16, 16, 2, _B16, _ALL),                                                # <1, 1, 3, false>: 2 splits; ragged second input block
    ("pair", 3, 40, 24, 16, 24, 2, dict(_B16, acc_dx=True, acc_dw=True, bias=False), _ALL),    # <1, 1, 3, true>: 5 splits, short last, straddling images
    ("pair", 3, 56, 24, 32, 32, 2, dict(_F16, bias=False), _ALL),                              # <2, 1, 3, false>: 12 splits, 4 phantoms
    ("pair", 1, 48, 24, 16, 16, 2, dict(_F16, acc_dx=True), _ALL),                             # <2, 1, 3, true>: one split
    ("pair", 3, 48, 48, 32, 32, 2, _B16, _ALL),                                                # <1, 2, 3, false>: 12 splits, 4 phantoms
    ("pair", 2, 96, 48, 32, 32, 2, dict(_B16, acc_dx=True, acc_dw=True), _ALL),                # <1, 2, 3, true>: 8 splits
    ("pair", 3, 48, 48, 16, 24, 2, dict(_F16, acc_dw=True), _ALL),                             # <2, 2, 3, false>: 5 splits
    ("pair", 2, 96, 48, 8, 16, 2, dict(_F16, acc_dx=True, bias=False), _ALL),                  # <2, 2, 3, true>: one split
    ("pair", 1, 192, 96, 8, 8, 2, dict(_B16, bias=False), _ALL),                               # <1, 2, 6, false>: the six-wave workgroup, one split of 2 steps
    ("pair", 3, 96, 96, 16, 24, 2, dict(_B16, acc_dx=True), _ALL),                             # <1, 2, 6, true>: 5 splits
    ("pair", 3, 64, 96, 24, 40, 2, dict(_F16, acc_dw=True), _ALL),                             # <2, 2, 6, false>: 12 splits (4 phantoms), the last 2 steps
    ("pair", 2, 192, 96, 8, 16, 2, dict(_F16, acc_dx=True), _ALL),                             # <2, 2, 6, true>
    # ... and the argument sets the programs have: dense tensors, dbias, dW stored
    ("pair", 2, 48, 48, 16, 16, 2, _B16, ()),                                                  # <1, 2, 3, false>: 2 splits
    ("pair", 3, 96, 48, 16, 24, 2, dict(_B16, acc_dx=True), ()),                               # <1, 2, 3, true>: 5 splits, short last
    ("pair", 3, 48, 48, 32, 32, 2, _F16, ()),                                                  # <2, 2, 3, false>: 12 splits, 4 phantoms
    ("pair", 2, 96, 48, 16, 16, 2, dict(_F16, acc_dx=True), ()),                               # <2, 2, 3, true>: 2 splits
    # ---- the pair where the fused kernel does not take it: the two calls' launches
    ("pair", 3, 48, 192, 24, 40, 2, _B16, ()),                                                 # wgrad16 <1, 2, 2> xcd: 12 splits, the last 2 steps + dgrad_lds; dense
    ("pair", 2, 96, 256, 32, 32, 2, dict(_B16, acc_dx=True), ()),                              # ... 8 splits; Cout = 256, the last with weights in LDS (MTnnUNet 256 -> 256)
    ("pair", 2, 48, 192, 32, 32, 2, _F16, ()),                                                 # wgrad16 <2, 2, 2> xcd + dgrad_lds <2, 4>
    ("pair", 3, 96, 256, 24, 40, 2, dict(_F16, acc_dx=True), ()),
    ("pair", 3, 320, 320, 8, 16, 2, dict(compute=1), ()),                                      # MTnnUNet's deepest up-conv: fp32 x and dy, bf16 MFMAs, 2 splits
    ("pair", 3, 32, 32, 16, 24, 2, dict(compute=1, dy16=True, acc_dx=True), ()),               # MTnnUNet's top level: 16-bit dy, fp32 x
    ("pair", 3, 48, 48, 16, 24, 2, {}, ()),                                                    # the fp32 mode, dense
    ("pair", 3, 192, 96, 8, 16, 2, dict(acc_dx=True), ()),                                     # ... accumulating, two splits
    ("pair", 3, 48, 192, 32, 32, 2, _B16, _ALL),                                               # Cout = 192 (12 waves): wgrad16 <1, 2, 2> xcd + dgrad_lds
    ("pair", 1, 384, 192, 8, 8, 2, dict(_F16, acc_dx=True), ()),                               # the deepest U-Net++ up-conv, one split
    ("pair", 2, 64, 320, 8, 16, 2, dict(_B16, acc_dx=True), ()),                               # MTnnUNet's 320-wide level: wgrad16 + the direct D = 4 dgrad
    ("pair", 3, 48, 48, 16, 24, 2, dict(acc_dx=True), _ALL),                                   # fp32: convT2_wgrad_kernel<0> + convT2_dgrad_kernel<0>
]


def _convT_case_id(case):
    kind, N, Cin, Cout, H, W, k, mode, strided = case
    return f"{kind}-{N}x{Cin}>{Cout}x{H}x{W}k{k}-" + ",".join(f"{n}={int(v)}" for n, v in sorted(mode.items())) + ("-" + "+".join(strided) if strided else "")


_CT_PAD = 8           # channels in front of and behind a view


def _convT_case_args(case, op, ptrs=None):
    """ops.convT_case_args of one call of a case (dummy pointers without ptrs)."""
    kind, N, Cin, Cout, H, W, k, mode, strided = case
    chans = dict(x=(Cin, H * W), y=(Cout, H * W * k * k), dy=(Cout, H * W * k * k), dx=(Cin, H * W))
    strides = {n: (chans[n][0] + 2 * _CT_PAD) * chans[n][1] for n in strided}
    return ops.convT_case_args(op, N, Cin, Cout, H, W, k, ptrs=ptrs, strides=strides, **mode)


def _convT_case_calls(case, ptrs=None):
    """[(kind, op, args, args of the DGRAD behind it or None)] of the launches a case makes."""
    L = ops.L
    kind = case[0]
    if kind == "pair":
        return [(kind, L.OP_CONVT_WGRAD, _convT_case_args(case, L.OP_CONVT_WGRAD, ptrs), _convT_case_args(case, L.OP_CONVT_DGRAD, ptrs))]
    op = {"fwd": L.OP_CONVT_FWD, "dgrad": L.OP_CONVT_DGRAD, "wgrad": L.OP_CONVT_WGRAD}[kind]
    return [(kind, op, _convT_case_args(case, op, ptrs), None)]


class _CtTensor:
    """One activation tensor of a case on the device: `fmt` "f32" planes, "p16" 16-bit planes, "c8" 16-bit channel-blocked of type st;
    `view` (what the kernel is given) is channels [pad, pad + C) of `buf`.  `cpu` keeps the buffer as uploaded."""

    def __init__(self, vals, fmt, st, pad, g):
        N, C, H, W = vals.shape
        wide = torch.randn(N, C + 2 * pad, H, W, generator=g)
        wide[:, pad:pad + C] = vals
        self.fmt, self.st, self.pad, self.shape = fmt, st, pad, (N, C, H, W)
        if fmt == "f32":
            self.cpu = wide
        elif fmt == "p16":
            self.cpu = _bits16(wide, st)
        else:
            self.cpu = _c8_of(wide, st)
        self.buf = self.cpu.to(DEV)
        q = pad // 8 if fmt == "c8" else pad
        c = C // 8 if fmt == "c8" else C
        self.view = self.buf[:, q:q + c]
        self._sl = slice(q, q + c)

    def data_ptr(self):
        return self.view.data_ptr()

    def read(self):
        """(values of the view as fp64 (N, C, H, W), True when everything around the view still holds what was uploaded)"""
        got = self.buf.cpu()
        keep = torch.ones(got.shape[1], dtype=torch.bool)
        keep[self._sl] = False
        untouched = torch.equal(got[:, keep], self.cpu[:, keep])
        v = got[:, self._sl]
        if self.fmt == "f32":
            return v.double(), untouched
        if self.fmt == "p16":
            return _from16(v, self.st), untouched
        return _planes_of(v.contiguous(), self.shape, self.st), untouched


@pytest.mark.parametrize("case", CONVT_CASES, ids=_convT_case_id)
def test_convT_step_instances_match_fp64(case):
    """Every transposed-convolution instance the dispatchers of convt2.hip / pool_up.hip can pick outside the A/B probe switches -- the ones
    the benchmark's step programs launch among them (test_step_programs_launch_only_reference_tested_convT_instances) -- against the plain
    fp64 reference of oracle/convt_reference.py on the STORED operands: inputs are drawn on the CPU and rounded RNE to the type the mode
    stores or the MFMA reads, so the kernel's own rounding is the identity.  Every element of every output is compared:
      fp32 forward and dx     max error <= 1e-5 x max |ref|                       (test_conv3x3_bench_instances_match_fp64)
      16-bit stored forward   per element within one unit in the last place of the stored type at the fp64 value + 1e-5 x max |ref| (_ulp16)
      dW, dbias               max error <= 1e-4 x max(1, max |ref|)               (test_convT_wgrad_reads_16bit_planar_x)
      accumulate              against ref + pre-fill, the same bound on the larger of the two scales
    Outputs are pre-filled; what a call was not asked for (no dbias, a lone WGRAD's dx, a lone DGRAD's dW) and the channels around a view
    keep their pre-fill bit for bit.  The launches made are exactly what mtbc_convT_kernel_name plans for the case's dummy arguments."""
    from multi_task_breast_cancer_amd.engine import Program, _mk
    from oracle import convt_reference as R
    L = ops.L
    kind, N, Cin, Cout, H, W, k, mode, strided = case
    compute = mode.get("compute", 0)
    fwd = kind == "fwd"
    g = _g(1993 + 7919 * N + 31 * Cin + 17 * Cout + H * W + k + 3 * compute + len(strided))
    # operand rounding: the forward on fp32 x is exact fp32 whatever y's type; everything else with compute != 0 reads 16-bit operands
    lp = compute if (not fwd or mode.get("x_c8")) else 0
    rnd = (lambda t: _round16(t, lp)) if lp else (lambda t: t)
    x = rnd(torch.randn(N, Cin, H, W, generator=g))
    w = rnd(torch.randn(Cin, Cout, k, k, generator=g) * (1.0 / Cin) ** 0.5)
    b = torch.randn(Cout, generator=g)
    dy = rnd(torch.randn(N, Cout, H * k, W * k, generator=g))
    pad = lambda n: _CT_PAD if n in strided else 0      # noqa: E731
    xfmt = "c8" if mode.get("x_c8") else "p16" if mode.get("x16") else "f32"
    T = dict(x=_CtTensor(x, xfmt, compute, pad("x"), g), w=w.to(DEV))
    pre = {}
    if fwd:
        pre["y"] = torch.randn(N, Cout, H * k, W * k, generator=g)
        T["y"] = _CtTensor(pre["y"], "c8" if mode.get("y_c8") else "f32", compute, pad("y"), g)
        T["bias"] = b.to(DEV)
    else:
        T["dy"] = _CtTensor(dy, "p16" if mode.get("dy16") else "f32", compute, pad("dy"), g)
        pre["dx"] = torch.randn(N, Cin, H, W, generator=g)
        T["dx"] = _CtTensor(pre["dx"], "f32", 0, pad("dx"), g)
        pre["dw"], pre["dbias"] = torch.randn(Cin, Cout, k, k, generator=g), torch.randn(Cout, generator=g)
        T["dw"], T["dbias"] = pre["dw"].to(DEV), pre["dbias"].to(DEV)
        # the workspace the library asks for, NaN so that a partial row nobody wrote shows in dW, inside a larger allocation: room for the 7
        # phantom splits a grid rounded up to 8 x cdiv(splits, 8) can have, which must come back untouched
        nfloat = max(4, (max(int(c[2].workspace_bytes) for c in _convT_case_calls(case)) + 3) // 4)
        slack = torch.full((nfloat + 8 * (Cin * Cout * k * k + Cout),), float("nan"), device=DEV)
        slack[nfloat:] = 1993.0
        T["workspace"] = slack[:nfloat]
    planned = [(op, ops.convT_kernel_name(a, op, nxt)) for _, op, a, nxt in _convT_case_calls(case)]
    calls = _convT_case_calls(case, T)
    assert [(op, ops.convT_kernel_name(a, op, nxt)) for _, op, a, nxt in calls] == planned, "the real pointers plan something else than the dummies"
    ops.launched = []
    try:
        for _, op, a, nxt in calls:
            if kind == "wgrad":
                a.dx, a.dx_batch_stride = T["dx"].data_ptr(), Cin * H * W          # a lone WGRAD has no business with dx
            if nxt is None:
                ops.convT_launch(a, op)
            else:
                two = [_mk(L.OP_CONVT_WGRAD), _mk(L.OP_CONVT_DGRAD)]
                two[0].u.convT, two[1].u.convT = a, nxt
                ops.convT_note(a, op, nxt)
                Program(two, [T]).run()
        torch.cuda.synchronize()
        made = list(ops.launched)
    finally:
        ops.launched = None
    assert made == planned, (made, planned)
    name = planned[0][1]

    worst = {}

    def check_max(what, got, ref, tol, floor, prefill=None):
        want = ref if prefill is None else ref + prefill.double()
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
        scale = max(floor, ref.abs().max().item(), want.abs().max().item())
        err = (got - want).abs().max().item()
        worst[what] = err / (tol * scale)
        return f"{what} ({name}): max err {err:.3e} against {tol:g} x {scale:.3e}"

    msgs = []
    xr, wr, dyr = x.double(), w.double(), dy.double()
    if fwd:
        ref = R.convT_fwd64(xr, wr, b if mode.get("bias", True) else None, k)
        got, untouched = T["y"].read()
        assert untouched, "y: the channels around the view were written"
        if mode.get("y_c8"):
            assert bool(torch.isfinite(got).all()), "stored y: non-finite"
            bound = _ulp16(ref, compute) + 1e-5 * ref.abs().max().item()
            worst["y16"] = ((got - ref).abs() / bound).max().item()
            msgs.append(f"stored y ({name}): {worst['y16']:.3f} x (one ulp of the stored type + 1e-5 x scale)")
        else:
            msgs.append(check_max("y", got, ref, 1e-5, 0.0))
    has_dx, has_dw = kind in ("dgrad", "pair"), kind in ("wgrad", "pair")
    if not fwd:
        got, untouched = T["dx"].read()
        assert untouched, "dx: the channels around the view were written"
        if has_dx:
            msgs.append(check_max("dx", got, R.convT_dx64(dyr, wr, k), 1e-5, 0.0, pre["dx"] if mode.get("acc_dx") else None))
        else:
            assert torch.equal(got.float(), pre["dx"]), "a lone WGRAD wrote dx"
        if has_dw:
            acc = mode.get("acc_dw")
            msgs.append(check_max("dW", T["dw"].cpu().double(), R.convT_dw64(xr, dyr, k), 1e-4, 1.0, pre["dw"] if acc else None))
            if mode.get("bias", True):
                msgs.append(check_max("dbias", T["dbias"].cpu().double(), R.convT_dbias64(dyr), 1e-4, 1.0, pre["dbias"] if acc else None))
            else:
                assert torch.equal(T["dbias"].cpu(), pre["dbias"]), "dbias was written without being asked for"
        else:
            assert torch.equal(T["dw"].cpu(), pre["dw"]) and torch.equal(T["dbias"].cpu(), pre["dbias"]), "a lone DGRAD wrote dW / dbias"
    if not fwd:
        assert bool((slack[nfloat:] == 1993.0).all()), "the memory behind the workspace was written"
    for n in ("x", "dy"):             # inputs, and the channels around their views, are read-only
        if n in T:
            assert torch.equal(T[n].buf.cpu(), T[n].cpu), f"{n} was written"
    print(f"{_convT_case_id(case)}: {name}: worst error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    bad = [m for m, v in zip(msgs, worst.values()) if not v <= 1.0]
    assert not bad, "; ".join(bad)


def _reference_tested_convT_keys():
    """(kind, key) of every call test_convT_step_instances_match_fp64 makes, from its case table's argument structs."""
    return {(kind, _convT_key(a, op, nxt)) for case in CONVT_CASES for kind, op, a, nxt in _convT_case_calls(case)}


def test_step_programs_launch_only_reference_tested_convT_instances():
    """Surveys (builds, does not run) the benchmark's four step programs for the coverage key of every MTBC_OP_CONVT_FWD / _DGRAD / _WGRAD op
    -- of the pair where a WGRAD has the DGRAD of the same up-convolution right behind it, which is what the program runner looks at --:
    each must be the key of a call that test_convT_step_instances_match_fp64 makes.  A plan change -- another instance, the XCD order or the
    fused kernel where it was not, a new argument-selected branch -- that no fp64 case reaches fails here; _convT_key (tests/step_programs.py),
    CONVT_CASES and _reference_tested_convT_keys are the places to edit.  A missing key is named with (N, Cin, Cout, H, W, k) of an op that has it."""
    assert_all_tested("transposed-convolution", _reference_tested_convT_keys(), [survey(p) for p in STEP_PROGRAMS], required=("fwd", "pair"))


# ------------------------------------------------------------------ the max-pool, 1x1, GAP, Linear and fused-head launches of the step programs, element by element
# kind -> (the *_case_args helper of ops.py, the op kind)
_SMALL_FAMILY = {"pool_fwd": ("maxpool", ops.L.OP_POOL_FWD), "pool_bwd": ("maxpool", ops.L.OP_POOL_BWD),
                 "c1_fwd": ("conv1x1", ops.L.OP_CONV1_FWD), "c1_dgrad": ("conv1x1", ops.L.OP_CONV1_DGRAD), "c1_wgrad": ("conv1x1", ops.L.OP_CONV1_WGRAD),
                 "gap_fwd": ("gap", ops.L.OP_GAP_FWD), "gap_bwd": ("gap", ops.L.OP_GAP_BWD),
                 "lin_fwd": ("linear", ops.L.OP_LINEAR_FWD), "lin_bwd": ("linear", ops.L.OP_LINEAR_BWD),
                 "head_combine": ("head", ops.L.OP_HEAD_COMBINE), "head_expand": ("head", ops.L.OP_HEAD_EXPAND)}


def _both16(kind, shape, mode, strided):
    """A 16-bit case in bf16 and in fp16."""
    return [(kind, shape, dict(mode, compute=c), strided) for c in (1, 2)]


# (kind, shape, mode, strided).  shape: pool / GAP (N, C, H, W), 1x1 (N, Cin, Cout, H, W), Linear (N, In, Out), head (Cin, Cmid, R, k).  mode: the
# keywords of the kind's ops.*_case_args helper; compute = 1 | 2: x (and the pool's y) 16-bit channel-blocked of that type.  strided: the
# activation tensors that are channel ranges [8, 8 + C) of a buffer 16 channels wider.  Each row is the smallest problem that reaches its launch
# and still has the structure that can go wrong there: more than one block of 256 threads with a ragged last one, several images, a second
# ragged channel group.  Rows marked (P) make a key one of the four step programs has today (their tensors are all dense); every other row is
# there because the standard is every instance the dispatchers can pick and every branch the arguments can select.
_PV, _BV = ("x", "y"), ("x", "dy", "dx")
SMALL_OP_CASES = [
    # ---- max-pool forward, fp32 planes: the float4 kernel (one thread = two windows), the scalar kernel where W % 4 != 0
    ("pool_fwd", (3, 5, 12, 40), {}, _PV),                               # 900 threads: four blocks, the last ragged; x and y views
    ("pool_fwd", (2, 3, 8, 8), {}, ()),                                  # (P) dense, 48 threads
    ("pool_fwd", (1, 5, 6, 10), {}, ()),                                 # scalar kernel: W % 4 != 0
    ("pool_fwd", (3, 5, 10, 14), {}, _PV),                               # scalar kernel, 525 threads, views
    # ---- max-pool forward, 16-bit channel-blocked, with and without the argmax codes
    *_both16("pool_fwd", (3, 16, 16, 16), dict(argmax=True), _PV),       # 384 threads: two blocks, ragged
    *_both16("pool_fwd", (3, 16, 16, 16), {}, _PV),
    *_both16("pool_fwd", (2, 8, 4, 8), dict(argmax=True), ()),           # dense
    *_both16("pool_fwd", (3, 16, 16, 16), {}, ("x",)),                   # a view of a concat buffer pooled into a dense tensor
    *_both16("pool_fwd", (2, 8, 4, 8), {}, ()),
    *_both16("pool_fwd", (3, 16, 16, 16), dict(argmax=True), ("x",)),
    # ---- max-pool backward: overwrite and accumulate, views and dense
    ("pool_bwd", (3, 5, 12, 20), {}, _BV),                               # 900 threads
    ("pool_bwd", (3, 5, 12, 20), dict(acc_dx=True), _BV),
    ("pool_bwd", (2, 3, 8, 8), {}, ()),                                  # (P)
    ("pool_bwd", (2, 3, 8, 8), dict(acc_dx=True), ()),                   # (P)
    ("pool_bwd", (3, 5, 12, 20), {}, ("x", "dx")),
    ("pool_bwd", (3, 5, 12, 20), dict(acc_dx=True), ("x", "dx")),
    *_both16("pool_bwd", (3, 16, 16, 16), {}, _BV),
    *_both16("pool_bwd", (3, 16, 16, 16), dict(acc_dx=True), _BV),
    *_both16("pool_bwd", (2, 8, 4, 8), {}, ()),
    *_both16("pool_bwd", (2, 8, 4, 8), dict(acc_dx=True), ()),
    # ---- 1x1 forward, fp32 planes: thread = 4 pixels x 8 output channels; 288 threads per image = two blocks, ragged; Cout = 10: a second, ragged group
    ("c1_fwd", (2, 12, 1, 32, 36), {}, ("x",)),
    ("c1_fwd", (2, 12, 1, 32, 36), {}, ()),                              # (P)
    ("c1_fwd", (2, 12, 1, 32, 36), dict(bias=False), ()),
    ("c1_fwd", (2, 12, 3, 32, 36), {}, ()),
    ("c1_fwd", (2, 12, 3, 32, 36), dict(bias=False), ("x",)),
    ("c1_fwd", (2, 12, 10, 32, 36), {}, ("x",)),
    ("c1_fwd", (2, 12, 10, 32, 36), dict(bias=False), ()),
    # ---- 1x1 input gradient: Cout = 10 adds the second group's sum to what the first stored (cog > 0)
    ("c1_dgrad", (2, 12, 1, 32, 36), {}, ("dx",)),
    ("c1_dgrad", (2, 12, 1, 32, 36), {}, ()),                            # (P)
    ("c1_dgrad", (2, 12, 1, 32, 36), dict(acc_dx=True), ()),
    ("c1_dgrad", (2, 12, 1, 32, 36), dict(acc_dx=True), ("dx",)),
    ("c1_dgrad", (2, 12, 10, 32, 36), {}, ()),
    ("c1_dgrad", (2, 12, 10, 32, 36), {}, ("dx",)),
    ("c1_dgrad", (2, 12, 10, 32, 36), dict(acc_dx=True), ()),
    ("c1_dgrad", (2, 12, 10, 32, 36), dict(acc_dx=True), ("dx",)),
    # ---- 1x1 weight gradient, fp32 planes: one partial per image, the reducer instance by the image count, the bias gradient's plane sums
    ("c1_wgrad", (3, 12, 3, 8, 8), {}, ("x",)),                          # splitk_reduce<4>, 64-thread plane sums
    ("c1_wgrad", (3, 12, 3, 8, 8), dict(bias=False), ()),
    ("c1_wgrad", (3, 12, 3, 8, 8), dict(bias=False, acc_dw=True), ("x",)),
    ("c1_wgrad", (3, 12, 10, 8, 8), {}, ()),
    ("c1_wgrad", (40, 12, 3, 8, 8), dict(acc_dw=True), ()),              # splitk_reduce<16>: more than 32 images
    ("c1_wgrad", (40, 12, 1, 8, 8), {}, ("x",)),
    ("c1_wgrad", (256, 12, 2, 4, 4), {}, ()),                            # splitk_reduce<64, 16>: 256 images
    ("c1_wgrad", (2, 12, 1, 64, 64), {}, ("x",)),                        # H * W = 4096: 256-thread plane sums
    ("c1_wgrad", (2, 12, 1, 64, 64), {}, ()),                            # (P)
    ("c1_wgrad", (2, 12, 1, 63, 64), dict(acc_dw=True), ()),             # H * W = 4032: the last plane size with 64 threads
    # ---- 1x1 on a 16-bit channel-blocked x: forward (one lane = one pixel; 320 pixels = two blocks, ragged) and weight gradient
    *_both16("c1_fwd", (2, 8, 1, 16, 20), {}, ("x",)),                   # Cin = 8: one channel group
    *_both16("c1_fwd", (2, 24, 1, 16, 20), {}, ()),                      # (P)
    *_both16("c1_fwd", (2, 24, 3, 16, 20), dict(bias=False), ()),
    *_both16("c1_fwd", (3, 16, 8, 16, 20), {}, ("x",)),                  # Cout = 8: every accumulator used
    *_both16("c1_wgrad", (2, 8, 1, 16, 20), {}, ("x",)),                 # nblk = 1
    *_both16("c1_wgrad", (2, 24, 1, 16, 20), {}, ()),
    *_both16("c1_wgrad", (2, 24, 3, 16, 20), dict(bias=False, acc_dw=True), ()),
    *_both16("c1_wgrad", (2, 16, 8, 16, 20), dict(acc_dw=True), ("x",)),
    *_both16("c1_wgrad", (2, 16, 3, 90, 92), {}, ("x",)),                # nblk = 2: chunks of 4140 pixels = 16 rounds of 256 threads + 44
    *_both16("c1_wgrad", (1, 8, 1, 112, 112), dict(bias=False), ()),     # nblk = 3: chunks of 4182, the last 4180
    *_both16("c1_wgrad", (1, 8, 1, 256, 512), {}, ()),                   # nblk = 32, the cap, at the smallest plane that reaches it
    *_both16("c1_wgrad", (1, 8, 1, 256, 512), dict(acc_dw=True), ("x",)),
    # ---- GAP: one wave per plane, four planes per block; 15 and 12 planes, a plane shorter than a wave, H * W % 64 != 0
    ("gap_fwd", (3, 5, 5, 7), {}, ()), ("gap_bwd", (3, 5, 5, 7), {}, ()),
    ("gap_fwd", (2, 6, 16, 16), {}, ()), ("gap_bwd", (2, 6, 16, 16), {}, ()),
    ("gap_fwd", (3, 5, 32, 32), {}, ()), ("gap_bwd", (3, 5, 32, 32), {}, ()),        # (P) all six
    # ---- Linear: (11, 70, 13) = both eight-wide unrolled loops and both tails, In = 70 a ragged second round of the forward's wave
    ("lin_fwd", (11, 70, 13), dict(relu=True), ()),                      # (P)
    ("lin_fwd", (11, 70, 13), {}, ()),                                   # (P)
    ("lin_fwd", (3, 256, 3), dict(bias=False), ()),
    ("lin_fwd", (3, 256, 3), dict(relu=True, bias=False), ()),
    ("lin_fwd", (16, 512, 256), dict(relu=True), ()),                    # (P)
    ("lin_bwd", (11, 70, 13), dict(relu=True, acc_dw=True), ()),
    ("lin_bwd", (11, 70, 13), {}, ()),
    ("lin_bwd", (11, 70, 3), {}, ()),                                    # (P) the logits layer: N >= 8 with Out < 8
    ("lin_bwd", (4, 70, 13), dict(relu=True), ()),                       # fewer than eight samples: the plain loop of linear_dw_kernel alone
    ("lin_bwd", (3, 256, 3), {}, ()),                                    # no unrolled loop at all
    ("lin_bwd", (3, 256, 3), dict(dx=False), ()),
    ("lin_bwd", (3, 256, 3), dict(relu=True, dx=False, acc_dw=True), ()),
    ("lin_bwd", (16, 512, 256), dict(relu=True), ()),                    # (P)
    ("lin_bwd", (16, 512, 256), dict(relu=True, dx=False), ()),
    ("lin_bwd", (16, 512, 256), dict(acc_dw=True), ()),
    # ---- the fused ConvT + 1x1 head: Cin * k * k = 320 / 288 / 768 (the 256-thread reduction of dw1, ragged), R = 1 and 3
    ("head_combine", (20, 7, 3, 4), {}, ()),                             # (P)
    ("head_combine", (72, 5, 1, 2), {}, ()),                             # (P)
    ("head_combine", (12, 6, 1, 8), {}, ()),                             # (P)
    ("head_combine", (72, 5, 1, 2), dict(bT=False), ()),
    ("head_combine", (12, 6, 3, 8), dict(b1=False), ()),
    ("head_expand", (20, 7, 3, 4), {}, ()),                              # (P)
    ("head_expand", (72, 5, 1, 2), {}, ()),                              # (P)
    ("head_expand", (12, 6, 1, 8), {}, ()),                              # (P)
    ("head_expand", (72, 5, 1, 2), dict(bT=False, acc=(1, 0, 0, 0)), ()),
    ("head_expand", (12, 6, 1, 8), dict(dbT=False, acc=(0, 0, 1, 0)), ()),
    ("head_expand", (12, 6, 3, 8), dict(db1=False, acc=(0, 1, 0, 0)), ()),
    ("head_expand", (20, 7, 1, 4), dict(acc=(0, 0, 0, 1)), ()),
    ("head_expand", (20, 7, 3, 2), dict(acc=(1, 1, 1, 1)), ()),
]


def _small_case_id(case):
    kind, shape, mode, strided = case
    return f"{kind}-" + "x".join(str(v) for v in shape) + "-" + ",".join(f"{n}={v if isinstance(v, tuple) else int(v)}" for n, v in sorted(mode.items())) + \
        ("-" + "+".join(strided) if strided else "")


def _small_case_ops(case, ptrs=None):
    """[op] of the launches a case makes, through the kind's ops.*_case_args helper (dummy pointers without ptrs)."""
    kind, shape, mode, strided = case
    helper, opk = _SMALL_FAMILY[kind]
    kw = dict(mode)
    if helper == "maxpool":
        _, Cc, H, W = shape
        per = dict(x=H * W, y=H * W // 4, dy=H * W // 4, dx=H * W)
        kw["strides"] = {n: (Cc + 2 * _CT_PAD) * per[n] for n in strided}
    elif helper == "conv1x1":
        _, Cin, _, H, W = shape
        kw["strides"] = {n: (Cin + 2 * _CT_PAD) * H * W for n in strided}
    return [getattr(ops, helper + "_case_args")(opk, *shape, ptrs=ptrs, **kw)]


_NAN, _INF = float("nan"), float("inf")
# 2x2 windows in (0,0), (0,1), (1,0), (1,1) order, written over the first and the last windows of every pool input: NaN at each position, two
# NaNs, infinities, equal maxima at each pair of positions, -0 / +0 ties, and two values that are equal only once rounded to 16 bits
_POOL_WINDOWS = [
    [_NAN, 1, 2, 3], [1, _NAN, 2, 3], [1, 2, _NAN, 3], [1, 2, 3, _NAN], [1, _NAN, _NAN, 3], [_NAN, 5, 1, _NAN], [_INF, _NAN, 1, 2],
    [_INF, 1, 2, 3], [1, 2, _INF, _INF], [-_INF, -_INF, -_INF, -_INF], [-_INF, -3, -_INF, -5],
    [7, 7, 1, 2], [7, 1, 7, 2], [7, 1, 2, 7], [1, 7, 7, 2], [1, 7, 2, 7], [1, 2, 7, 7], [4, 4, 4, 4],
    [-0.0, 0.0, 0.0, -0.0], [0.0, -0.0, -0.0, 0.0], [-1, -0.0, 0.0, -2], [-1, 0.0, -0.0, -2],
    [0.5, 1.0, 1.0 + 2.0 ** -12, 0.25],
]


def _craft_pool_windows(x):
    N, Cc, H, W = x.shape
    oH, oW = H // 2, W // 2
    total = N * Cc * oH * oW
    assert total >= 2 * len(_POOL_WINDOWS), total
    for i, wv in enumerate(_POOL_WINDOWS):
        for f in (i, total - 1 - i):
            ox, t = f % oW, f // oW
            oy, t = t % oH, t // oH
            x[t // Cc, t % Cc, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = torch.tensor(wv, dtype=x.dtype).reshape(2, 2)
    return x


def _same_bits(a, b):
    """Equal as stored words (a NaN equals the same NaN)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _identical64(got, want):
    """fp64 values equal up to the NaN payload: NaN where NaN, else the same value with the same sign of zero."""
    ok = ~torch.isnan(want)
    return got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[ok], want[ok]) and \
        torch.equal(torch.signbit(got[ok]), torch.signbit(want[ok]))


class _Guarded:
    """A dense tensor on the device with a canary of 64 elements on each side; `cpu` keeps what was uploaded."""
    PAD, MARK = 64, 1993

    def __init__(self, vals):
        self.cpu, n = vals.clone(), vals.numel()
        flat = torch.full((n + 2 * self.PAD,), self.MARK, dtype=vals.dtype)
        flat[self.PAD:self.PAD + n] = vals.reshape(-1)
        self.buf = flat.to(DEV)
        self.view = self.buf[self.PAD:self.PAD + n].view(vals.shape)

    def data_ptr(self):
        return self.view.data_ptr()

    def numel(self):
        return self.view.numel()

    def read(self):
        """(the tensor as it is now, True when both canaries still hold their mark)"""
        got = self.buf.cpu()
        return got[self.PAD:-self.PAD].view(self.cpu.shape), bool((got[:self.PAD] == self.MARK).all() and (got[-self.PAD:] == self.MARK).all())


class _Bounds:
    """Collects worst error / bound per output of a case (the bounds of test_convT_step_instances_match_fp64)."""

    def __init__(self, name):
        self.name, self.worst, self.msgs = name, {}, []

    def check(self, what, got, ref, tol, floor, prefill=None):
        want = ref if prefill is None else ref + prefill.double()
        got = got.double()
        assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
        scale = max(floor, ref.abs().max().item(), want.abs().max().item())
        err = (got - want).abs().max().item()
        self.worst[what] = err / (tol * scale)
        self.msgs.append(f"{what} ({self.name}): max err {err:.3e} against {tol:g} x {scale:.3e}")

    def fwd(self, what, got, ref, prefill=None):          # fp32 forward and dx outputs
        self.check(what, got, ref, 1e-5, 0.0, prefill)

    def param(self, what, got, ref, prefill=None):        # parameter gradients
        self.check(what, got, ref, 1e-4, 1.0, prefill)

    def out(self, what, t, ref, bound, prefill=None):
        """A _Guarded output against its reference -- or, with ref None, untouched: it was not asked for."""
        got, intact = t.read()
        assert intact, f"{what}: the memory around it was written"
        if ref is None:
            assert _same_bits(got, t.cpu), f"{what} was written without being asked for"
        else:
            bound(what, got, ref, t.cpu if prefill else None)


def _small_launch(case, T):
    """Launches the case on the tensors T; the launches made are what the dummy arguments plan.  Returns the launches' name."""
    planned = [(op.kind, ops.op_kernel_name(op)) for op in _small_case_ops(case)]
    real = _small_case_ops(case, T)
    assert [(op.kind, ops.op_kernel_name(op)) for op in real] == planned, "the real pointers plan something else than the dummies"
    ops.launched = []
    try:
        for op in real:
            ops.small_op_launch(op)
        torch.cuda.synchronize()
        made = list(ops.launched)
    finally:
        ops.launched = None
    assert made == planned, (made, planned)
    return planned[0][1]


def _workspace(case):
    """(the NaN-filled workspace the case's arguments ask for, the allocation it sits in: 1993.0 behind it)"""
    op = _small_case_ops(case)[0]
    nbytes = int(getattr(op.u, ops.L.OP_UNION_FIELD[op.kind]).workspace_bytes)
    nfloat = max(4, (nbytes + 3) // 4)
    slack = torch.full((nfloat + 4096,), float("nan"), device=DEV)
    slack[nfloat:] = 1993.0
    return slack[:nfloat], slack


def _small_pool(case, g):
    from oracle import small_ops_reference as R
    kind, (N, Cc, H, W), mode, strided = case
    st = mode.get("compute", 0)
    fmt = "c8" if st else "f32"
    pad = lambda n: _CT_PAD if n in strided else 0      # noqa: E731
    x = _craft_pool_windows(torch.randn(N, Cc, H, W, generator=g))
    x = _round16(x, st) if st else x
    T = dict(x=_CtTensor(x, fmt, st, pad("x"), g))
    T["y"] = _CtTensor(torch.randn(N, Cc, H // 2, W // 2, generator=g), fmt, st, pad("y"), g)
    if kind == "pool_fwd":
        T["argmax"] = _Guarded(torch.full((N, Cc // 8 if st else Cc, (H // 2) * (W // 2)), 0x5555, dtype=torch.int16))
    else:
        dy = torch.randn(N, Cc, H // 2, W // 2, generator=g)
        pre = torch.randn(N, Cc, H, W, generator=g)
        T["dy"], T["dx"] = _CtTensor(dy, "f32", 0, pad("dy"), g), _CtTensor(pre, "f32", 0, pad("dx"), g)
    b = _Bounds(_small_launch(case, T))
    assert _same_bits(T["x"].buf.cpu(), T["x"].cpu), "x was written"
    got, untouched = T["y"].read()
    if kind == "pool_fwd":
        assert untouched, "y: the channels around the view were written"
        assert _identical64(got, R.maxpool_fwd64(x)), f"y ({b.name}): not the first maximum of every window, bit for bit"
        codes, intact = T["argmax"].read()
        assert intact, "argmax: the memory around it was written"
        if mode.get("argmax"):
            assert torch.equal(codes.long() & 0xffff, R.maxpool_argmax_codes(x)), f"argmax codes ({b.name})"
        else:
            assert torch.equal(codes, T["argmax"].cpu), "argmax was written without being asked for"
        b.worst["y exact"] = 0.0
        return b
    assert untouched and _same_bits(T["y"].buf.cpu(), T["y"].cpu), "the backward wrote y"
    assert _same_bits(T["dy"].buf.cpu(), T["dy"].cpu), "dy was written"
    got, untouched = T["dx"].read()
    assert untouched, "dx: the channels around the view were written"
    routed = R.maxpool_bwd64(x, dy).float()
    want = (pre + routed) if mode.get("acc_dx") else routed          # one IEEE add
    assert torch.equal(got.float(), want), f"dx ({b.name}): max difference {(got.float() - want).abs().max().item():.3e}"
    b.worst["dx exact"] = 0.0
    return b


def _small_conv1x1(case, g):
    from oracle import small_ops_reference as R
    kind, (N, Cin, Cout, H, W), mode, strided = case
    st = mode.get("compute", 0)
    pad = lambda n: _CT_PAD if n in strided else 0      # noqa: E731
    x = torch.randn(N, Cin, H, W, generator=g)
    x = _round16(x, st) if st else x
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * (1.0 / Cin) ** 0.5
    bias, dy = torch.randn(Cout, generator=g), torch.randn(N, Cout, H, W, generator=g)
    ins = dict(w=w.to(DEV), bias=bias.to(DEV), dy=dy.to(DEV))
    T = dict(ins, x=_CtTensor(x, "c8" if st else "f32", st, pad("x"), g))
    T["y"] = _Guarded(torch.randn(N, Cout, H, W, generator=g))
    T["dx"] = _CtTensor(torch.randn(N, Cin, H, W, generator=g), "f32", 0, pad("dx"), g)
    T["dw"], T["dbias"] = _Guarded(torch.randn(Cout, Cin, 1, 1, generator=g)), _Guarded(torch.randn(Cout, generator=g))
    slack = None
    if kind == "c1_wgrad":
        T["workspace"], slack = _workspace(case)
    b = _Bounds(_small_launch(case, T))
    assert _same_bits(T["x"].buf.cpu(), T["x"].cpu), "x was written"
    for n, t in (("w", w), ("bias", bias), ("dy", dy)):
        assert torch.equal(ins[n].cpu(), t), f"{n} was written"
    b.out("y", T["y"], R.conv1x1_fwd64(x, w, bias if mode.get("bias", True) else None) if kind == "c1_fwd" else None, b.fwd)
    got, untouched = T["dx"].read()
    assert untouched, "dx: the channels around the view were written"
    if kind == "c1_dgrad":
        b.fwd("dx", got, R.conv1x1_dx64(dy, w), T["dx"].cpu[:, T["dx"]._sl] if mode.get("acc_dx") else None)
    else:
        assert _same_bits(T["dx"].buf.cpu(), T["dx"].cpu), "dx was written without being asked for"
    wg, acc = kind == "c1_wgrad", mode.get("acc_dw")
    b.out("dW", T["dw"], R.conv1x1_dw64(x, dy).reshape(Cout, Cin, 1, 1) if wg else None, b.param, acc)
    b.out("dbias", T["dbias"], R.conv1x1_dbias64(dy) if wg and mode.get("bias", True) else None, b.param, acc)
    if slack is not None:
        assert bool((slack[T["workspace"].numel():] == 1993.0).all()), "the memory behind the workspace was written"
    return b


def _small_gap(case, g):
    from oracle import small_ops_reference as R
    kind, (N, Cc, H, W), mode, strided = case
    x, dy = torch.randn(N, Cc, H, W, generator=g) + 0.5, torch.randn(N, Cc, generator=g)
    ins = dict(x=x.to(DEV), dy=dy.to(DEV))
    T = dict(ins, y=_Guarded(torch.randn(N, Cc, generator=g)), dx=_Guarded(torch.randn(N, Cc, H, W, generator=g)))
    b = _Bounds(_small_launch(case, T))
    assert torch.equal(ins["x"].cpu(), x) and torch.equal(ins["dy"].cpu(), dy), "an input was written"
    b.out("y", T["y"], R.gap_fwd64(x) if kind == "gap_fwd" else None, b.fwd)
    b.out("dx", T["dx"], R.gap_bwd64(dy, H, W) if kind == "gap_bwd" else None, b.fwd)
    return b


def _small_linear(case, g):
    from oracle import small_ops_reference as R
    kind, (N, In, Out), mode, strided = case
    relu, has_bias = bool(mode.get("relu")), mode.get("bias", True)
    x, w = torch.randn(N, In, generator=g), torch.randn(Out, In, generator=g) * (1.0 / In) ** 0.5
    bias, dy = torch.randn(Out, generator=g) * 0.1, torch.randn(N, Out, generator=g)
    yref = R.linear_fwd64(x, w, bias if has_bias else None, relu)
    fwd = kind == "lin_fwd"
    ins = dict(x=x.to(DEV), w=w.to(DEV), bias=bias.to(DEV), dy=dy.to(DEV))
    T = dict(ins)
    ystored = yref.float()                  # the backward masks on the stored output: exact zeros where the ReLU cut
    T["y"] = _Guarded(torch.randn(N, Out, generator=g) if fwd else ystored)
    T["dx"], T["dw"], T["dbias"] = _Guarded(torch.randn(N, In, generator=g)), _Guarded(torch.randn(Out, In, generator=g)), _Guarded(torch.randn(Out, generator=g))
    slack = None
    if not fwd and relu:
        T["workspace"], slack = _workspace(case)
    b = _Bounds(_small_launch(case, T))
    for n, t in (("x", x), ("w", w), ("bias", bias), ("dy", dy)):
        assert torch.equal(ins[n].cpu(), t), f"{n} was written"
    if fwd:
        b.out("y", T["y"], yref, b.fwd)
        if relu:
            got = T["y"].read()[0]
            pre = R.linear_fwd64(x, w, bias if has_bias else None, False)
            cut = pre < -1e-5 * pre.abs().max().item()
            assert bool(cut.any()) and bool((yref > 0).any()), "the case has no output on each side of the ReLU"
            assert bool((got[cut] == 0).all()), "a negative pre-activation was not stored as exactly 0"
    else:
        assert bool((ystored == 0).any()) or not relu
        b.out("y", T["y"], None, None)
        dx, dw, db = R.linear_bwd64(x, w, ystored, dy, relu)
        acc = mode.get("acc_dw")
        b.out("dx", T["dx"], dx if mode.get("dx", True) else None, b.fwd)
        b.out("dW", T["dw"], dw, b.param, acc)
        b.out("dbias", T["dbias"], db, b.param, acc)
    if fwd:
        for n in ("dx", "dw", "dbias"):
            b.out(n, T[n], None, None)
    if slack is not None:
        assert bool((slack[T["workspace"].numel():] == 1993.0).all()), "the memory behind the workspace was written"
    return b


def _small_head(case, g):
    from oracle import small_ops_reference as R
    kind, (Cin, Cmid, Rr, k), mode, strided = case
    wT, bT = torch.randn(Cin, Cmid, k, k, generator=g) * (1.0 / Cin) ** 0.5, torch.randn(Cmid, generator=g)
    w1, b1 = torch.randn(Rr, Cmid, generator=g) * (1.0 / Cmid) ** 0.5, torch.randn(Rr, generator=g)
    G, gb = torch.randn(Cin, Rr, k, k, generator=g), torch.randn(Rr, generator=g)
    src = dict(wT=wT, bT=bT, w1=w1, b1=b1, G=G, gb=gb)
    ins = {n: t.to(DEV) for n, t in src.items()}
    T = dict(ins)
    for n, shape in (("Wc", (Cin, Rr, k, k)), ("bc", (Rr,)), ("dwT", wT.shape), ("dbT", bT.shape), ("dw1", w1.shape), ("db1", b1.shape)):
        T[n] = _Guarded(torch.randn(*shape, generator=g))
    b = _Bounds(_small_launch(case, T))
    for n, t in src.items():
        assert torch.equal(ins[n].cpu(), t), f"{n} was written"
    has_bT, has_b1 = mode.get("bT", True), mode.get("b1", True)
    comb = kind == "head_combine"
    Wc, bc = R.head_combine64(wT, bT if has_bT else None, w1, b1 if has_b1 else None)
    b.out("Wc", T["Wc"], Wc if comb else None, b.fwd)
    b.out("bc", T["bc"], bc if comb else None, b.fwd)
    refs = dict(zip(("dwT", "dbT", "dw1", "db1"), R.head_expand64(wT, bT if has_bT else None, w1, G, gb)))
    if not mode.get("dbT", True):
        refs["dbT"] = None
    if not mode.get("db1", True):
        refs["db1"] = None
    acc = dict(zip(("dwT", "dbT", "dw1", "db1"), mode.get("acc", (0, 0, 0, 0))))
    for n in ("dwT", "dbT", "dw1", "db1"):
        b.out(n, T[n], None if comb else refs[n], b.param, acc[n])
    return b


_SMALL_RUN = {"maxpool": _small_pool, "conv1x1": _small_conv1x1, "gap": _small_gap, "linear": _small_linear, "head": _small_head}


@pytest.mark.parametrize("case", SMALL_OP_CASES, ids=_small_case_id)
def test_small_op_step_instances_match_fp64(case):
    """Every launch the dispatchers of the max-pool, the 1x1 convolution, GAP, Linear and the fused ConvT + 1x1 head can pick (pool_up.hip,
    c8_ops.hip, head_loss.hip, the reducers of reduce.hip) -- the ones the benchmark's step programs make among them
    (test_step_programs_launch_only_reference_tested_small_op_instances) -- against the plain fp64 references of oracle/small_ops_reference.py
    on the STORED operands: inputs are drawn on the CPU and rounded RNE to the type the mode stores.  Every element of every output is compared:
      max-pool forward, argmax codes, backward      bit for bit (a selection; NaN where NaN, the sign of zero included); the backward in
                                                    accumulate mode against pre-fill + routed gradient formed in fp32: one IEEE add
      fp32 forward and dx outputs                   max error <= 1e-5 x max |ref|       (1x1 y and dx, GAP, Linear y and dx, Wc, bc)
      parameter gradients                           max error <= 1e-4 x max(1, max |ref|)      (1x1 / Linear dW and dbias, dwT, dbT, dw1, db1)
      accumulate                                    against ref + pre-fill, the same bound on the larger of the two scales
    the bounds of the ConvT section above; plain fp32 arithmetic on such inputs is within 1.1e-6 relative.  Every pool input carries the
    windows of _POOL_WINDOWS at both ends.  Every output is pre-filled: what a call was not asked for (dbias, dx, argmax, the other direction's
    outputs), the channels around a view, the canaries around every dense output, the inputs and the floats behind the workspace keep their
    contents bit for bit.  The launches made are exactly what mtbc_op_kernel_name plans for the case's dummy arguments."""
    kind, shape, mode, strided = case
    g = _g(1993 + 7919 * sorted(_SMALL_FAMILY).index(kind) + sum((31 + 2 * i) * v for i, v in enumerate(shape)) + 3 * mode.get("compute", 0) + len(strided))
    b = _SMALL_RUN[_SMALL_FAMILY[kind][0]](case, g)
    print(f"{_small_case_id(case)}: {b.name}: worst error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in b.worst.items()))
    bad = [m for m, v in zip(b.msgs, [v for n, v in b.worst.items() if not n.endswith(" exact")]) if not v <= 1.0]
    assert not bad, "; ".join(bad)


def _reference_tested_small_op_keys():
    """(op kind, key) of every call test_small_op_step_instances_match_fp64 makes, from its case table's argument structs."""
    return {(op.kind, _small_op_key(op)) for case in SMALL_OP_CASES for op in _small_case_ops(case)}


def test_step_programs_launch_only_reference_tested_small_op_instances():
    """Surveys (builds, does not run) the benchmark's four step programs for the coverage key of every max-pool, 1x1, GAP, Linear and fused-head
    op: each must be the key of a call that test_small_op_step_instances_match_fp64 makes.  A plan change -- another kernel or reducer
    instance, a tensor that became a view, a new argument-selected branch -- that no fp64 case reaches fails here; _small_op_key
    (tests/step_programs.py), SMALL_OP_CASES and _reference_tested_small_op_keys are the places to edit.  Every program must hold the
    classification head: GAP and Linear, forward and backward."""
    L = ops.L
    assert_all_tested("small-op", _reference_tested_small_op_keys(), [survey(p) for p in STEP_PROGRAMS],
                      required=(L.OP_GAP_FWD, L.OP_GAP_BWD, L.OP_LINEAR_FWD, L.OP_LINEAR_BWD))


# ------------------------------------------------------------------ the weight-image, weight-view and channel-blocking launches of the step programs, bit for bit
# These kernels (csrc/conv3x3.hip) move or round values and add nothing: every word of every destination is compared with the numpy
# scatter references of oracle/layout_reference.py (checked on their own in tests/test_layout_reference_cpu.py) as integers, no tolerance.
# The one exception is NaN: where the reference holds a NaN pattern the device must hold one too; payload and sign are printed, not compared.
# Every destination sits between two guard regions of _LPAD elements (512 bytes and more), destination and guards pre-filled with a fixed
# non-zero pattern; the guards and the sources must come back unchanged.
from oracle import layout_reference as LR  # noqa: E402

PACK_CASES = LR.PACK_CASES                    # (Cout, Cin)
WVIEW_CASES = LR.WVIEW_CASES                  # (Cout, Cin, off, cnt, mode, k_off, K)
C8_PACK_CASES = LR.C8_PACK_CASES              # (N, C, HW, strided): mtbc_c8_pack and _unpack, both formats
C8_PACK16_CASES = LR.C8_PACK16_CASES          # (N, C, HW, strided): mtbc_c8_pack16
PACK_KINDS = [(0, 0), (1, 0), (2, 1), (2, 2), (3, 1), (3, 2)]          # (kind of mtbc_pack_desc, compute): the four images, the 16-bit ones in both formats
_LPAD = 256
_MARK = {torch.float32: 1993.0, torch.int16: 0x5a5a}


class _LayoutDst:
    """A pre-filled flat destination on the device between two pre-filled guard regions of _LPAD elements."""

    def __init__(self, numel, dtype):
        self.numel, self.dtype = numel, dtype
        self.buf = torch.full((numel + 2 * _LPAD,), _MARK[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[_LPAD:_LPAD + numel]
        assert self.view.data_ptr() % 16 == 0

    def prefill(self):
        """The destination's pre-fill as the numpy array a reference writes into."""
        return np.full(self.numel, _MARK[self.dtype], dtype=np.float32 if self.dtype == torch.float32 else np.uint16)

    def read(self, what):
        got = self.buf.cpu()
        assert bool((got[:_LPAD] == _MARK[self.dtype]).all() and (got[-_LPAD:] == _MARK[self.dtype]).all()), f"{what}: written outside the destination"
        got = got[_LPAD:-_LPAD].numpy()
        return got.view(np.uint32) if self.dtype == torch.float32 else got.view(np.uint16)


class _LayoutSrc:
    """A numpy source uploaded to the device; intact() tells whether the device copy still holds the same words."""

    def __init__(self, vals):
        self.np = np.ascontiguousarray(vals)
        self.t = torch.from_numpy(self.np.view(np.int16) if self.np.dtype == np.uint16 else self.np).to(DEV)

    def intact(self):
        back = self.t.cpu().numpy()
        return np.array_equal(back.view(np.uint32 if back.dtype == np.float32 else np.uint16), self.np.view(np.uint32 if self.np.dtype == np.float32 else np.uint16))


def _same_words(what, got, want, compute=0):
    """got == want as integers; for the 16-bit type of `compute` a NaN pattern of the reference matches any NaN pattern."""
    want = np.ascontiguousarray(want).reshape(-1)
    want = want.view(np.uint32) if want.dtype == np.float32 else want
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ok = np.ones(want.shape, bool)
    if compute:
        nan = LR.is_nan16(want, compute)
        assert bool(LR.is_nan16(got, compute)[nan].all()), f"{what}: the reference holds NaN where the device does not"
        if nan.any():
            print(f"    {what}: {int(nan.sum())} NaN, device patterns {sorted({hex(v) for v in got[nan].tolist()})}, reference {sorted({hex(v) for v in want[nan].tolist()})}")
        ok = ~nan
    bad = np.flatnonzero((got != want) & ok)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} words differ, the first at {int(bad[0])}: {hex(int(got[bad[0]]))} for {hex(int(want[bad[0]]))}"


_PACK_W, _PACK_REF = {}, {}


def _pack_weight(Cout, Cin, compute):
    """The (Cout, Cin, 3, 3) source of a shape: randn with the special values of `compute` scattered in, some in the last row and the last K."""
    key = (Cout, Cin, compute)
    if key not in _PACK_W:
        w = np.random.default_rng(1993 + 131 * Cout + 17 * Cin + compute).standard_normal((Cout, Cin, 3, 3)).astype(np.float32)
        _PACK_W[key] = LR.plant(w, compute, LR.weight_edges(Cout, Cin))
    return _PACK_W[key]


def _pack_ref(Cout, Cin, kind, compute):
    """The reference image of _pack_weight, computed once and shared (read only)."""
    key = (Cout, Cin, kind, compute)
    if key not in _PACK_REF:
        w = _pack_weight(Cout, Cin, compute)
        _PACK_REF[key] = LR.pack_fwd(w) if kind == 0 else LR.pack_dgrad(w) if kind == 1 else LR.pack_lp(w, kind - 2, compute)
        _PACK_REF[key].setflags(write=False)
    return _PACK_REF[key]


def _run_pack_list(what, descs):
    """descs: (Cout, Cin, kind, compute) in list order.  ONE mtbc_conv3x3_pack_many call for a list of more than one descriptor, else the
    single-tensor entry point of the kind; every image against its reference."""
    src = {(Cout, Cin, c): _LayoutSrc(_pack_weight(Cout, Cin, c)) for Cout, Cin, _, c in descs}
    dst = [_LayoutDst(ops.conv3x3_image_elems(Cout, Cin, kind), torch.int16 if kind >= 2 else torch.float32) for Cout, Cin, kind, _ in descs]
    if len(descs) > 1:
        ops.conv3x3_pack_list([(src[Cout, Cin, c].t, kind, c) for Cout, Cin, kind, c in descs], out=[d.view for d in dst])
    else:
        (Cout, Cin, kind, c), lib, L = descs[0], ops.L.load(), ops.L
        w, p = src[Cout, Cin, c].t.data_ptr(), dst[0].view.data_ptr()
        if kind >= 2:
            L.check(lib.mtbc_conv3x3_pack_lp(w, p, Cin, Cout, kind - 2, c, ops._s()), "pack_lp")
        else:
            L.check((lib.mtbc_conv3x3_pack_dgrad if kind else lib.mtbc_conv3x3_pack_fwd)(w, p, Cin, Cout, ops._s()), "pack")
    torch.cuda.synchronize()
    bad = []
    for i, ((Cout, Cin, kind, c), d) in enumerate(zip(descs, dst)):
        name = f"{what}[{i}] {Cout}x{Cin} kind {kind} compute {c}"
        try:
            _same_words(name, d.read(name), _pack_ref(Cout, Cin, kind, c), c if kind >= 2 else 0)
        except AssertionError as e:
            bad.append(str(e))
    assert all(s.intact() for s in src.values()), f"{what}: a source was written"
    assert not bad, f"{len(bad)} of {len(descs)} images wrong:\n  " + "\n  ".join(bad[:8])
    return len(descs)


@pytest.mark.parametrize("path", ["single", "many"])
@pytest.mark.parametrize("Cout,Cin", PACK_CASES, ids=lambda v: str(v))
def test_weight_images_match_the_layout_reference(Cout, Cin, path):
    """The four images of a shape -- fp32 forward and dgrad, 16-bit forward and dgrad in bf16 and in fp16 -- through the single-tensor entry
    points (pack_fwd_kernel, pack_dgrad_kernel, pack_lp_kernel) and as ONE mtbc_conv3x3_pack_many list of the six (pack_many_kernel: the LDS
    transpose, pack_dgrad_elem, pack_lp_unit; the list changes format three times, so it is four launches each with its own format flag)."""
    if path == "many":
        n = _run_pack_list(f"{Cout}x{Cin} many", [(Cout, Cin, k, c) for k, c in PACK_KINDS])
    else:
        n = sum(_run_pack_list(f"{Cout}x{Cin} single", [(Cout, Cin, k, c)]) for k, c in PACK_KINDS)
    print(f"{Cout}x{Cin} {path}: {n} images bit for bit")


def _mixed_pack_list():
    """116 descriptors over the shapes of at most 2048 weights: 100 that mix the fp32 kinds with bf16 images (the first launch ends at the 96-descriptor
    argument batch), then 8 with fp16 images, then 8 with bf16 again: two format breaks.  Repeated descriptors get their own destinations."""
    small = [s for s in PACK_CASES if s[0] * s[1] <= 32 * 64]
    descs = []
    for n, fmt in ((100, 1), (8, 2), (8, 1)):
        for i in range(n):
            Cout, Cin = small[(len(descs) * 5 + 3) % len(small)]
            kind = (2, 0, 3, 1)[i % 4]          # each run starts with a 16-bit image of its format
            descs.append((Cout, Cin, kind, fmt if kind >= 2 else 0))
    return descs


def test_pack_many_over_format_breaks_and_an_argument_batch_boundary():
    descs = _mixed_pack_list()
    assert len(descs) > 96 and {k for _, _, k, _ in descs} == {0, 1, 2, 3}
    fmts = [c for _, _, k, c in descs if k >= 2]
    assert [c for i, c in enumerate(fmts) if i == 0 or fmts[i - 1] != c] == [1, 2, 1]
    n = _run_pack_list("mixed list", descs)
    print(f"mixed list: {n} images bit for bit")


def test_pack_many_of_exactly_two():
    assert _run_pack_list("two", [(7, 13, 0, 0), (17, 33, 3, 2)]) == 2
    assert _run_pack_list("two 16-bit", [(17, 33, 2, 1), (7, 13, 3, 1)]) == 2


# ---- weight views
def _wview_id(case):
    return "-".join(map(str, case))


def _wview_desc(case, w, dst):
    d = ops.L.WViewDesc()
    d.w, d.dst = w.t.data_ptr(), dst.view.data_ptr()
    d.Cout, d.Cin, d.ci_off, d.ci_cnt, d.mode, d.k_off, d.K = case
    return d


def _wview_numel(case):
    Cout, Cin, off, cnt, mode, k_off, K = case
    return (cnt * K if mode else Cout * cnt) * 9


def _wview_weight(case, salt=0):
    Cout, Cin = case[:2]
    w = np.random.default_rng(17 + 131 * Cout + 17 * Cin + salt).standard_normal((Cout, Cin, 3, 3)).astype(np.float32)
    return LR.plant(w, 0, LR.weight_edges(Cout, Cin))


def _wview_want(cases_ws, dst):
    """The destination's pre-fill with the views (case, weight) written into it by the reference, in order."""
    Cout, Cin, off, cnt, mode, k_off, K = cases_ws[0][0]
    want = dst.prefill().reshape((cnt, K, 3, 3) if mode else (Cout, cnt, 3, 3))
    for (Cout, Cin, off, cnt, mode, k_off, K), w in cases_ws:
        LR.weight_view(w, off, cnt, mode, k_off, K, want)
    return want


@pytest.mark.parametrize("case", WVIEW_CASES, ids=_wview_id)
def test_weight_view_matches_the_layout_reference(case):
    """mtbc_conv3x3_weight_view (wview_kernel): the whole destination -- for mode 1 all K of the (cnt, K, 3, 3) tensor, so what lies outside
    [k_off, k_off + Cout) must keep its pre-fill -- against the reference."""
    w, dst = _LayoutSrc(_wview_weight(case)), _LayoutDst(_wview_numel(case), torch.float32)
    ops.L.check(ops.L.load().mtbc_conv3x3_weight_view(w.t.data_ptr(), dst.view.data_ptr(), *case, ops._s()), "weight_view")
    torch.cuda.synchronize()
    _same_words(_wview_id(case), dst.read(_wview_id(case)), _wview_want([(case, w.np)], dst))
    assert w.intact()


# three consumers' views side by side in one (8, 40, 3, 3) destination: K ranges [0, 8), [8, 20), [26, 40); [20, 26) is nobody's
WVIEW_GROUP = [(8, 24, 16, 8, 1, 0, 40), (12, 8, 0, 8, 1, 8, 40), (14, 20, 4, 8, 1, 26, 40)]


def test_weight_view_many_matches_the_layout_reference():
    """mtbc_conv3x3_weight_view_many (wview_many_kernel) over 4 x every case + the group of three = 59 descriptors (more than one argument
    batch of 48), each with its own destination -- except WVIEW_GROUP, which fills disjoint K ranges of ONE destination and leaves a fourth
    range to its pre-fill."""
    L = ops.L
    items = [(case, _LayoutSrc(_wview_weight(case, rep)), _LayoutDst(_wview_numel(case), torch.float32)) for rep in range(2) for case in WVIEW_CASES]
    gdst = _LayoutDst(_wview_numel(WVIEW_GROUP[0]), torch.float32)
    group = [(case, _LayoutSrc(_wview_weight(case, 5)), gdst) for case in WVIEW_GROUP]
    items += group + [(case, _LayoutSrc(_wview_weight(case, rep)), _LayoutDst(_wview_numel(case), torch.float32)) for rep in range(2, 4) for case in WVIEW_CASES]
    assert len(items) > 48
    arr = (L.WViewDesc * len(items))(*[_wview_desc(case, w, dst) for case, w, dst in items])
    L.check(L.load().mtbc_conv3x3_weight_view_many(arr, len(items), ops._s()), "weight_view_many")
    torch.cuda.synchronize()
    bad = []
    for i, (case, w, dst) in enumerate(items):
        name = f"[{i}] {_wview_id(case)}"
        try:
            if dst is gdst:
                want = _wview_want([(c, s.np) for c, s, _ in group], dst)
                assert bool((want[:, 20:26] == _MARK[torch.float32]).all())
            else:
                want = _wview_want([(case, w.np)], dst)
            _same_words(name, dst.read(name), want)
            assert w.intact(), f"{name}: the source was written"
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{len(bad)} of {len(items)} views wrong:\n  " + "\n  ".join(bad[:8])
    print(f"{len(items)} views in one call, bit for bit")


# ---- channel-blocked activations
def _c8_source(N, Cc, HW, strided, compute):
    """(the whole float32 source (N, Cfull, HW), the channel range under test, Cfull)"""
    Cfull, c0 = (40, 8) if strided else (Cc, 0)
    x = np.random.default_rng(5 + 7 * N + 3 * Cc + HW + compute).standard_normal((N, Cfull, HW)).astype(np.float32) * 3
    last = ((N - 1) * Cfull + c0 + Cc - 1) * HW + HW - 1          # the last pixel of the last channel of the range
    return LR.plant(x, compute, [last, c0 * HW]), slice(c0, c0 + Cc), Cfull


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cc,HW,strided", C8_PACK_CASES)
def test_c8_pack_and_unpack_match_the_layout_reference(N, Cc, HW, strided, compute):
    """mtbc_c8_pack (c8_pack_kernel<F16>), dense and on a channel range of a wider tensor (src_batch_stride = 40 HW), then mtbc_c8_unpack
    (c8_unpack_kernel<F16>) of what it wrote: unpack(pack(x)) == round16(x) as floats, bit for bit."""
    L, lib = ops.L, ops.L.load()
    x, rng, Cfull = _c8_source(N, Cc, HW, strided, compute)
    src, y, back = _LayoutSrc(x), _LayoutDst(N * Cc * HW, torch.int16), _LayoutDst(N * Cc * HW, torch.float32)
    L.check(lib.mtbc_c8_pack(src.t.data_ptr() + 4 * rng.start * HW, Cfull * HW, y.view.data_ptr(), N, Cc, HW, compute, ops._s()), "c8_pack")
    L.check(lib.mtbc_c8_unpack(y.view.data_ptr(), back.view.data_ptr(), N, Cc, HW, compute, ops._s()), "c8_unpack")
    torch.cuda.synchronize()
    want = LR.c8_pack(x[:, rng], compute)
    _same_words("pack", y.read("pack"), want, compute)
    h = LR.round16(x[:, rng], compute)
    wide, got = LR.widen16(h, compute).view(np.uint32).reshape(-1), back.read("unpack")
    nan = LR.is_nan16(h, compute).reshape(-1)
    assert bool(np.isnan(got.view(np.float32))[nan].all()) and np.array_equal(got[~nan], wide[~nan]), "unpack(pack(x)) != round16(x)"
    _same_words("unpack against the reference", got[~nan], LR.c8_unpack(want, compute).view(np.uint32).reshape(-1)[~nan])
    assert src.intact()


@pytest.mark.parametrize("N,Cc,HW,strided", C8_PACK16_CASES)
def test_c8_pack16_matches_the_layout_reference(N, Cc, HW, strided):
    """mtbc_c8_pack16 (c8_pack16_kernel) moves 16-bit words whatever they mean: random words, every one compared."""
    L, lib = ops.L, ops.L.load()
    Cfull, c0 = (40, 8) if strided else (Cc, 0)
    x = np.random.default_rng(9 + 7 * N + 3 * Cc + HW).integers(0, 1 << 16, (N, Cfull, HW), dtype=np.uint16)
    src, y = _LayoutSrc(x), _LayoutDst(N * Cc * HW, torch.int16)
    L.check(lib.mtbc_c8_pack16(src.t.data_ptr() + 2 * c0 * HW, Cfull * HW, y.view.data_ptr(), N, Cc, HW, ops._s()), "c8_pack16")
    torch.cuda.synchronize()
    _same_words("pack16", y.read("pack16"), LR.c8_pack16(x[:, c0:c0 + Cc]))
    assert src.intact()


# ---- the guard
_DESC_KIND = {0: ("OP_CONV3_PACK_FWD", 0), 1: ("OP_CONV3_PACK_DGRAD", 1), 2: ("OP_CONV3_PACK_LP", 0), 3: ("OP_CONV3_PACK_LP", 1)}


def _reference_tested_layout_keys():
    """The key of every call the layout tests above make, from their tables."""
    L = ops.L
    keys = set()
    for Cout, Cin in PACK_CASES:
        for k, c in PACK_KINDS:
            for path in ("single", "many"):
                keys.add(_pack_key(getattr(L, _DESC_KIND[k][0]), Cin, Cout, _DESC_KIND[k][1], c, path))
    for case in WVIEW_CASES:
        keys.add(_wview_key(*case, "single"))
    for case in WVIEW_CASES + WVIEW_GROUP:
        keys.add(_wview_key(*case, "many"))
    for N, Cc, HW, strided in C8_PACK_CASES:
        keys.update(_c8_key(L.OP_C8_PACK, N, Cc, HW, c, 40 * HW if strided else Cc * HW) for c in (1, 2))
    for N, Cc, HW, strided in C8_PACK16_CASES:
        keys.add(_c8_key(L.OP_C8_PACK16, N, Cc, HW, 0, 40 * HW if strided else Cc * HW))
    return keys


def test_step_programs_launch_only_reference_tested_layout_ops():
    """Surveys (builds, does not run) the benchmark's four step programs for the coverage key of every weight-image, weight-view and
    channel-blocking op in every program of the step (the views and images sit in the "pack" program): each must be the key of a call that the
    layout tests above make.  _pack_key / _wview_key / _c8_key (tests/step_programs.py), the case tables and _reference_tested_layout_keys are
    the places to edit.  A missing key is named with its op's arguments: (Cin, Cout, dgrad, compute) of an image, (Cout, Cin, off, cnt, mode,
    k_off, K) of a view, (N, C, HW, compute, src_batch_stride) of a channel-blocking op."""
    assert_all_tested("layout", _reference_tested_layout_keys(), [survey(p) for p in STEP_PROGRAMS])


# ---- the loss mix
def test_loss_mix_is_the_written_fp32_expression_and_flags_nan():
    """mtbc_loss_mix, launched in every step: out4 == (alpha * s + (1 - alpha) * c, s, c, flag) with the first element formed in fp32 as
    written (two products and a sum, each rounded), flag 1 for a NaN in either input and 0 for infinities.  (With the sum contracted into an
    fma the second launch below answers 0x3ec4109d for 0x3ec4109e.)"""
    L, lib = ops.L, ops.L.load()
    f = np.float32
    nan, inf = float("nan"), float("inf")
    for s, c, alpha in ((0.7312345, 1.0986123, 0.3), (0.1234567, 2.7182817, 0.9), (3.1415927, 0.5772157, 0.7), (nan, 1.5, 0.5), (0.25, nan, 0.5),
                        (inf, 1.5, 0.5), (0.25, -inf, 0.25)):
        seg, cls = torch.tensor([s], dtype=torch.float32, device=DEV), torch.tensor([c], dtype=torch.float32, device=DEV)
        out = _LayoutDst(4, torch.float32)
        L.check(lib.mtbc_loss_mix(seg.data_ptr(), cls.data_ptr(), alpha, out.view.data_ptr(), ops._s()), "loss_mix")
        torch.cuda.synchronize()
        got = out.read("out4").view(np.float32)
        with np.errstate(invalid="ignore"):
            mix = f(f(alpha) * f(s)) + f((f(1.0) - f(alpha)) * f(c))
        want = np.array([mix, s, c, 1.0 if (s != s or c != c) else 0.0], dtype=np.float32)
        print(f"loss_mix({s}, {c}, {alpha}): device {got.tolist()} ({hex(int(got.view(np.uint32)[0]))}), as written {float(mix)!r} ({hex(int(want.view(np.uint32)[0]))})")
        assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
        ok = ~np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), (s, c, alpha, got.tolist(), want.tolist())


# ---- every op kind of the step programs has a test that answers for it
_THIS = "tests/test_ops_gpu.py"
_LAYOUT_GUARD = (_THIS, "test_step_programs_launch_only_reference_tested_layout_ops")
_SMALL_GUARD = (_THIS, "test_step_programs_launch_only_reference_tested_small_op_instances")
_CONV3_GUARD = (_THIS, "test_step_programs_launch_only_reference_tested_conv3x3_instances")
_INORM_GUARD = (_THIS, "test_step_programs_launch_only_reference_tested_instnorm_instances")
_CONVT_GUARD = (_THIS, "test_step_programs_launch_only_reference_tested_convT_instances")
_STREAMS = (_THIS, "test_program_run_on_two_streams_orders_a_forked_section")
# (the loss mix has ONE key; the guard's key set names test_loss_mix_is_the_written_fp32_expression_and_flags_nan above as the test that makes it)
_LOSS_GUARD = ("tests/test_loss_launches_gpu.py", "test_step_programs_launch_only_reference_tested_loss_instances")
# op kind -> (file, test): the reference test, or the guard that ties every launch of the kind to a reference case
OP_KIND_COVERED_BY = {
    "OP_CONV3_FWD": _CONV3_GUARD, "OP_CONV3_DGRAD": _CONV3_GUARD, "OP_CONV3_WGRAD": _CONV3_GUARD,
    "OP_CONV3_PACK_FWD": _LAYOUT_GUARD, "OP_CONV3_PACK_DGRAD": _LAYOUT_GUARD, "OP_CONV3_PACK_LP": _LAYOUT_GUARD, "OP_CONV3_WVIEW": _LAYOUT_GUARD,
    "OP_C8_PACK": _LAYOUT_GUARD, "OP_C8_PACK16": _LAYOUT_GUARD,
    "OP_IN_FWD": _INORM_GUARD, "OP_IN_BWD": _INORM_GUARD, "OP_IN_DPARAM": _INORM_GUARD,
    "OP_CONVT_FWD": _CONVT_GUARD, "OP_CONVT_DGRAD": _CONVT_GUARD, "OP_CONVT_WGRAD": _CONVT_GUARD,
    "OP_POOL_FWD": _SMALL_GUARD, "OP_POOL_BWD": _SMALL_GUARD, "OP_CONV1_FWD": _SMALL_GUARD, "OP_CONV1_DGRAD": _SMALL_GUARD, "OP_CONV1_WGRAD": _SMALL_GUARD,
    "OP_GAP_FWD": _SMALL_GUARD, "OP_GAP_BWD": _SMALL_GUARD, "OP_LINEAR_FWD": _SMALL_GUARD, "OP_LINEAR_BWD": _SMALL_GUARD,
    "OP_HEAD_COMBINE": _SMALL_GUARD, "OP_HEAD_EXPAND": _SMALL_GUARD,
    "OP_DICE_FWD": _LOSS_GUARD, "OP_DICE_BWD": _LOSS_GUARD, "OP_FOCAL": _LOSS_GUARD, "OP_LOSS_MIX": _LOSS_GUARD, "OP_SOFTMAX": _LOSS_GUARD,
    "OP_OPTIM": ("tests/test_fused_optim_gpu.py", "test_kernel_is_the_host_function_bit_for_bit"), "OP_DICE_COUNTS": (_THIS, "test_dice_counts_exact"),
    "OP_MEMSET": (_THIS, "test_memset_op_zeroes_exactly_its_bytes"),
    "OP_SET_STREAM": _STREAMS, "OP_EVENT_RECORD": _STREAMS, "OP_EVENT_WAIT": _STREAMS,
}


def test_memset_op_zeroes_exactly_its_bytes():
    """MTBC_OP_MEMSET through mtbc_program_run: the bytes asked for become zero, the guards and the tail keep their pre-fill."""
    import ctypes as C
    from multi_task_breast_cancer_amd.engine import _mk
    L = ops.L
    dst = _LayoutDst(300, torch.float32)
    op = _mk(L.OP_MEMSET)
    op.u.memset0.ptr, op.u.memset0.bytes = dst.view.data_ptr(), 4 * 260
    arr, failed = (L.Op * 1)(op), C.c_int32(-1)
    L.check(L.load().mtbc_program_run(arr, 0, 1, ops._s(), C.byref(failed)), "program_run")
    torch.cuda.synchronize()
    got = dst.read("memset").view(np.float32)
    assert not got[:260].any() and bool((got[260:] == _MARK[torch.float32]).all())


def test_every_op_kind_of_the_step_programs_is_claimed_by_a_test():
    """Surveys (builds, does not run) the four step programs for every op kind present: each must have an entry in OP_KIND_COVERED_BY, and the
    test or guard it names must exist in the file it names.  A new op kind in a program without an entry fails here."""
    import os
    L = ops.L
    name_of = {getattr(L, n): n for n in dir(L) if n.startswith("OP_") and isinstance(getattr(L, n), int)}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, (path, test) in OP_KIND_COVERED_BY.items():
        assert name in name_of.values(), f"{name} is no op kind"
        text = open(os.path.join(root, path)).read()
        assert re.search(rf"^def {test}\(", text, re.M), f"{name}: {path} has no {test}"
    assert_op_kinds_claimed([survey(p) for p in STEP_PROGRAMS])
