"""The stem with intensity channels (data.augmentation: the first conv reads ONE fp32 planar segment of 2 .. 5 channels) on the GPU:
the multi-channel stem kernels against the direct kernel (fp32: bit for bit; 16-bit: that value rounded once), the weight gradient
from a channel-blocked dz against the fp32 weight-gradient kernel, the plan that uses them, whole models in the 16-bit modes against
the emulation, and the device-resident dataset feeding a bf16 model."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import augment as AUG  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import engine, ops  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet, MTUNetPlusPlus  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
# (N, Cin, Cout, H, W); 40 x 24: 240 four-pixel groups, the last block is ragged
FP32_SHAPES = [(2, 3, 24, 64, 64), (1, 5, 5, 8, 12), (3, 2, 32, 40, 24), (2, 4, 24, 96, 96)]
C8_SHAPES = [s for s in FP32_SHAPES if s[2] % 8 == 0] + [(1, 5, 8, 256, 256)]
WG_SHAPES = C8_SHAPES + [(2, 3, 24, 128, 128)]          # 128 x 128: 4 bands, 256 x 256: 16 bands
MODES = [(1, True), (1, False), (2, False)]              # (compute, out_fp16)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _operands(N, Cin, Cout, H, W, seed, wscale=0.05):
    g = _g(seed)
    x = (torch.rand(N, Cin, H, W, generator=g) * 255.0).to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * wscale).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    return g, x, w, b


@pytest.mark.parametrize("N,Cin,Cout,H,W", FP32_SHAPES)
def test_fp32_stem_equals_direct_kernel_bitwise(N, Cin, Cout, H, W):
    _, x, w, b = _operands(N, Cin, Cout, H, W, Cin + Cout + H, 0.1)
    a = ops._conv_args([x], w, N, H, W)
    ops._fill_segs(a.in_, [x])
    a.out = x.data_ptr()
    assert ops.conv3x3_kernel_name(a, L.OP_CONV3_FWD) == f"conv3x3_stem_mc_fwd_kernel<{Cin}>"
    assert torch.equal(ops.conv3x3_fwd([x], w, b), ops.conv3x3_fwd([x], w, b, force_direct=True))
    assert torch.equal(ops.conv3x3_fwd([x], w, None), ops.conv3x3_fwd([x], w, None, force_direct=True))


def _check_c8_forward(x, w, b, compute, out_fp16):
    N, Cout = x.shape[0], w.shape[0]
    z32 = ops.conv3x3_fwd([x], w, b, force_direct=True)
    z8, part = ops.conv3x3_stem_fwd_c8(x, w, b, compute, out_fp16=out_fp16, stats=True)
    t = 2 if out_fp16 else compute
    want = ops.C8.pack(z32.clamp(-65504.0, 65504.0) if t == 2 else z32, t)
    assert z8.compute == t and torch.equal(z8.data, want.data)
    assert not torch.isnan(part).any()
    zr = z8.unpack().double()
    tot = part.double().sum(1)
    assert torch.allclose(tot[..., 0].cpu(), zr.sum((2, 3)).cpu(), rtol=1e-5, atol=1e-2)
    assert torch.allclose(tot[..., 1].cpu(), (zr * zr).sum((2, 3)).cpu(), rtol=1e-5, atol=1e-1)
    return z32, z8


@pytest.mark.parametrize("compute,out_fp16", MODES)
@pytest.mark.parametrize("N,Cin,Cout,H,W", C8_SHAPES)
def test_16bit_stem_forward(N, Cin, Cout, H, W, compute, out_fp16):
    """fp32 operands and the direct kernel's fmaf order; the output channel-blocked 16-bit = the fp32 result, clamped for fp16 storage,
    rounded once; InstanceNorm statistics of the stored values (tolerances of test_stem_conv_on_the_16bit_path)."""
    ops.launched = []
    try:
        _, x, w, b = _operands(N, Cin, Cout, H, W, N + Cin + Cout + H + compute)
        _check_c8_forward(x, w, b, compute, out_fp16)
        of16 = "true" if (out_fp16 or compute == 2) else "false"
        assert (L.OP_CONV3_FWD, f"conv3x3_stem_mc_fwd_c8_kernel<{Cin}, {of16}>") in ops.launched
    finally:
        ops.launched = None


def test_16bit_stem_forward_saturates_fp16_storage():
    """bf16 mode storing fp16: |z| beyond 65504 is stored as +-65504, never as inf."""
    _, x, w, b = _operands(2, 3, 24, 40, 24, 77, wscale=40.0)
    z32 = ops.conv3x3_fwd([x], w, b, force_direct=True)
    assert z32.abs().max().item() > 65504.0
    z8, part = ops.conv3x3_stem_fwd_c8(x, w, b, 1, out_fp16=True, stats=True)
    assert z8.compute == 2 and torch.equal(z8.data, ops.C8.pack(z32.clamp(-65504.0, 65504.0), 2).data)
    assert torch.isfinite(part).all()
    zs = z8.unpack()
    assert torch.isfinite(zs).all() and zs.abs().max().item() == 65504.0
    assert bool((zs[z32 > 65504.0] == 65504.0).all()) and bool((zs[z32 < -65504.0] == -65504.0).all())


@pytest.mark.parametrize("compute", [1, 2])
@pytest.mark.parametrize("N,Cin,Cout,H,W", WG_SHAPES)
def test_16bit_stem_weight_gradient(N, Cin, Cout, H, W, compute):
    """dz channel-blocked 16-bit, the input fp32 planar: = the fp32 weight-gradient kernel on the unpacked dz (other summation order)."""
    g, x, w, _ = _operands(N, Cin, Cout, H, W, N + Cin + Cout + H + 3 * compute)
    dz8 = ops.C8.pack(torch.randn(N, Cout, H, W, generator=g).to(DEV), compute)
    dw_ref, _ = ops.conv3x3_wgrad([x], dz8.unpack(), tuple(w.shape))
    ops.launched = []
    try:
        dw, _ = ops.conv3x3_wgrad_c8([x], dz8, tuple(w.shape))
        f16 = "true" if compute == 2 else "false"
        assert ops.launched == [(L.OP_CONV3_WGRAD, f"conv3x3_wgrad_stem_mc_c8_kernel<{Cin}, {f16}> + splitk_reduce")]
    finally:
        ops.launched = None
    err = (dw - dw_ref).abs().max().item()
    print("wgrad", (N, Cin, Cout, H, W), "max err", err, "max |dw|", dw_ref.abs().max().item())
    assert torch.allclose(dw, dw_ref, rtol=1e-4, atol=1e-4 * max(1.0, dw_ref.abs().max().item())), err


def test_16bit_stem_weight_gradient_accumulates():
    g, x, w, _ = _operands(2, 3, 24, 64, 64, 5)
    dz8 = ops.C8.pack(torch.randn(2, 24, 64, 64, generator=g).to(DEV), 1)
    dw, _ = ops.conv3x3_wgrad_c8([x], dz8, tuple(w.shape))
    pre = torch.randn(24, 3, 3, 3, generator=g).to(DEV) * dw.abs().max()
    acc, _ = ops.conv3x3_wgrad_c8([x], dz8, tuple(w.shape), dw=pre.clone(), accumulate=True)
    assert torch.allclose(acc, pre + dw, rtol=1e-5, atol=1e-5 * dw.abs().max().item())


def test_fp32_weight_gradient_with_five_channels():
    """fp32 mode, Cin = 5: the small-Cin kernel (it stopped at 4) against F.conv2d's autograd in float64, direct-wgrad tolerance."""
    N, Cin, Cout, H, W = 3, 5, 24, 40, 24
    g, x, w, _ = _operands(N, Cin, Cout, H, W, 9, 0.1)
    dz = torch.randn(N, Cout, H, W, generator=g)
    wr = w.cpu().double().requires_grad_(True)
    F.conv2d(x.cpu().double(), wr, None, padding=1).backward(dz.double())
    ops.launched = []
    try:
        dw, _ = ops.conv3x3_wgrad([x], dz.to(DEV), tuple(w.shape))
        assert ops.launched == [(L.OP_CONV3_WGRAD, "conv3x3_wgrad_smallcin_kernel + splitk_reduce")]
    finally:
        ops.launched = None
    want = wr.grad.float()
    err = (dw.cpu() - want).abs()
    assert bool((err <= 1e-4 * max(1.0, want.abs().max().item()) + 1e-4 * want.abs()).all()), err.max().item()


def _model(arch, cin=3):
    if arch == "MTnnUNet":
        return MTnnUNet(cin, 1, 3)
    return MTUNetPlusPlus(in_channels=cin, out_channels=1, n_classes=3, deep_supervision=True)


def _batch3(N, size, seed):
    """The image and two intensity channels (brighter, higher contrast), as data.augmentation stacks them."""
    img, mask, label = O.synthetic_batch(N, size, size, seed=seed)
    x = torch.cat([img, (img * 1.3).clamp(0.0, 255.0), ((img - 128.0) * 1.5 + 128.0).clamp(0.0, 255.0)], 1)
    return x, mask, label


def _first_cell_launches(st):
    """(cell, forward instance, weight-gradient instance) of the first conv cell of a compiled step."""
    cell = st.plan.cells[0]
    fwd = next(op for op in st.programs["fwd"].array if op.kind == L.OP_CONV3_FWD and op.tag == cell.tag)
    bwd = st.programs["bwd"]
    wg = next(bwd.array[i] for i in range(bwd.n) if bwd.array[i].kind == L.OP_CONV3_WGRAD and bwd.array[i].tag == cell.tag)
    return cell, ops.conv3x3_kernel_name(fwd.u.conv3, L.OP_CONV3_FWD), ops.conv3x3_kernel_name(wg.u.conv3, L.OP_CONV3_WGRAD)


@pytest.mark.parametrize("arch", ["MTnnUNet", "MTUNetPlusPlus"])
def test_the_plan_uses_the_stem(arch, monkeypatch):
    x, mask, label = _batch3(2, 64, 3)
    for old in (False, True):
        monkeypatch.setattr(engine, "_NO_STEM_MC", old)
        seed_everything(7)
        m = _model(arch).to(DEV)
        m.set_compute("bf16")
        step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5)
        st = step.load_batch(x.to(DEV), mask.to(DEV), label.to(DEV))
        cell, fwd, wg = _first_cell_launches(st)
        assert cell.cin == 3 and cell.H == 64
        if old:
            assert not cell.stem16 and not cell.z16
            assert (fwd, wg) == ("conv3x3_direct_kernel", "conv3x3_wgrad_smallcin_kernel + splitk_reduce")
        else:
            assert cell.stem16 and cell.z16
            assert (fwd, wg) == ("conv3x3_stem_mc_fwd_c8_kernel<3, true>", "conv3x3_wgrad_stem_mc_c8_kernel<3, false> + splitk_reduce")
        step.run(st)
        step.check_nan()


class _stem_mc_emulation:
    """Layered INSIDE O.lowp_conv3x3 (which stores the stem's output in 16 bits for a 1-channel weight only): the same treatment for a
    3x3 / pad-1 conv over 2 .. 5 input channels with Cout % 8 == 0 -- exact fp32 conv, clamped when the bf16 mode stores fp16, stored
    rounded, flagged as a conv-cell output.  Everything else goes to the oracle's patched F.conv2d."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        inner, ctx = F.conv2d, self.ctx
        self._inner = inner

        def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
            H, W = input.shape[-2:]
            if (tuple(weight.shape[-2:]) == (3, 3) and padding in (1, (1, 1)) and stride in (1, (1, 1)) and groups == 1 and ctx.z16 and ctx.stem16
                    and 2 <= weight.shape[1] <= L.STEM_MAX_CIN and weight.shape[0] % 8 == 0 and H >= 8 and W >= 8 and W % 4 == 0
                    and O._z16_plane_ok(H, W)):
                z = torch.conv2d(input, weight, bias, stride, padding, dilation, groups)
                if ctx.zt == torch.float16 and ctx.lp != torch.float16:
                    z = z.clamp(-65504.0, 65504.0)
                out = O._StoreRounded.apply(z, ctx.zt)
                out._mtbc_z16 = True
                return out
            return inner(input, weight, bias, stride, padding, dilation, groups)

        F.conv2d = conv2d
        return self

    def __exit__(self, *exc):
        F.conv2d = self._inner
        return False


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# (arch, dtype, size, N, arm); 128 x 128: cooperative InstanceNorm at level 0; "no_stem_mc": the plan switch, against the oracle's own
# treatment of a multi-channel first conv (exact, fp32 output)
@pytest.mark.parametrize("arch,dtype,size,N,arm", [("MTnnUNet", "bf16", 64, 4, ""), ("MTUNetPlusPlus", "f16", 64, 4, ""),
                                                    ("MTUNetPlusPlus", "bf16", 128, 2, ""), ("MTnnUNet", "bf16", 64, 4, "no_stem_mc")])
def test_whole_model_against_the_emulation(arch, dtype, size, N, arm, monkeypatch):
    """test_16bit_mfma_modes_match_their_emulation's pattern and tolerances with 3 input channels, from weights that 40 fp32-mode steps
    have moved: against the fp64-accumulating emulation, allowed 3 x the distance of the fp32-accumulating one (floors 5e-4 loss, 2e-3
    outputs, 5e-2 per parameter gradient), no tensor exempt.  The first layer's weight gradient is printed: it is what the multi-channel
    weight-gradient kernel computes."""
    if arm == "no_stem_mc":
        monkeypatch.setattr(engine, "_NO_STEM_MC", True)
    seed_everything(1993)
    prod = _model(arch)
    O.seed_everything(1993)
    ref = O.build_oracle_model(arch, 3, 1, 3, True)
    ref.load_state_dict(prod.state_dict())
    prod = prod.to(DEV)
    warm = FusedTrainStep(prod, FusedAdam(prod, lr=1e-3, eps=1e-4), alpha=0.5)
    for s_ in range(40):
        x, mask, label = _batch3(4, size, 100 + s_)
        warm(x.to(DEV), mask.to(DEV), label.to(DEV))
    warm.check_nan()
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in prod.state_dict().items()})
    prod.set_compute(dtype)
    ref64 = copy.deepcopy(ref).double()
    x, mask, label = _batch3(N, size, 21)
    step = FusedTrainStep(prod, FusedAdam(prod, lr=1e-4, eps=1e-4), alpha=0.5)
    st = step.load_batch(x.to(DEV), mask.to(DEV), label.to(DEV))
    cell = st.plan.cells[0]
    assert cell.cin == 3 and cell.stem16 == (arm == "")
    losses = step.run(st).cpu()
    ls = prod.loss_scale
    with O.lowp_conv3x3(dtype, model=[ref, ref64], da16=False) as ctx, (_stem_mc_emulation(ctx) if arm == "" else _nothing()):
        t32 = O.train_step(ref, O.make_adam(ref, 1e-4), x, mask, label, 0.5, True, 3, loss_scale=ls)
        t64 = O.train_step(ref64, O.make_adam(ref64, 1e-4), x.double(), mask.double(), label, 0.5, True, 3, loss_scale=ls)
    assert losses[3].item() == 0.0
    rel = lambda a, b: ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()      # noqa: E731
    assert abs(losses[0].item() - t64[0].item()) < max(3 * abs(t32[0].item() - t64[0].item()), 5e-4)
    assert rel(st.logits.data.view(N, -1), t64[3][0]) < max(3 * rel(t32[3][0], t64[3][0]), 2e-3)
    for got, w32, w64 in zip(st.segs, t32[4], t64[4]):
        assert rel(got.data, w64) < max(3 * rel(w32, w64), 2e-3)
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad = []
    for name in prod._order:
        if name.endswith("conv.bias") or g64[name].grad.norm().item() == 0.0:
            continue
        e_hip, e_cpu = rel(prod._grad_view(name) / ls, g64[name].grad), rel(g32[name].grad, g64[name].grad)
        if name == cell.wname:
            print("first-layer weight gradient", name, "e_hip", e_hip, "e_cpu", e_cpu)
        if not e_hip < max(3 * e_cpu, 5e-2):
            bad.append((name, round(e_hip, 4), round(e_cpu, 4)))
    assert not bad, bad


AUG2 = {"brightness_brighter": True, "contrast_high": True}


def _store(M, H, W, seed):
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def _twin_steps(seed, **kw):
    out = []
    for _ in range(2):
        seed_everything(seed)
        model = MTnnUNet(3, 1, 3).to(DEV)
        model.set_compute("bf16")
        out.append((model, FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5, **kw)))
    return out


def _host_batch(ds, images, masks, labels, index, params):
    """What a caller of `load_batch` assembles for the same rows: mask, image and its intensity channels stacked, transformed together."""
    idx = torch.as_tensor(index, dtype=torch.long)
    im = images[idx]
    planes = [masks[idx].float(), im.float()] + [torch.from_numpy(l.astype("float32"))[im.long()] for l in DD.intensity_luts(AUG2)]
    stack = AUG.flip_rotate(torch.stack(planes, dim=1).to(DEV), torch.as_tensor(params))
    return stack[:, 1:].contiguous(), stack[:, :1].contiguous(), labels[idx].float().view(-1, 1).to(DEV)


def test_device_dataset_feeds_a_bf16_model():
    """test_load_indexed_step_equals_load_batch_step with a 3-channel dataset and a bf16 MTnnUNet(3, 1, 3): the multi-channel stem reads what
    the one-launch batch assembly wrote."""
    images, masks, labels = _store(7, 64, 64, seed=8)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=AUG2)
    assert ds.n_augments == 2
    (ma, sa), (mb, sb) = _twin_steps(31)
    for s, index in enumerate(([6, 0], [3, 5])):
        params = AUG.params_from([37.5, -123.4] if s == 0 else [180.0, 12.0], [1, 0], [0, 1])
        sta = sa.load_indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV), params.to(DEV))
        assert sta.plan.cells[0].stem16 and sta.plan.cells[0].cin == 3
        la = sa.run(sta)
        lb = sb.run(sb.load_batch(*_host_batch(ds, images, masks, labels, index, params)))
        assert torch.equal(la, lb), (s, la.tolist(), lb.tolist())
        assert torch.equal(ma.flat_g, mb.flat_g), s
    assert torch.equal(ma.flat_p, mb.flat_p)
    sa.check_nan()


def test_device_dataset_graph_replay_equals_eager():
    images, masks, labels = _store(7, 64, 64, seed=8)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=AUG2)
    (ma, sa), (mb, sb) = _twin_steps(32)
    sa.graph, sb.graph = True, False
    for s in range(5):                                          # one plan: captured at the third call, replayed after
        index = torch.tensor([(s + 1) % 7, (3 * s) % 7], dtype=torch.int32, device=DEV)
        params = AUG.params_from([10.0 * s, -45.0], [s % 2, 0], [0, 1]).to(DEV)
        la, lb = sa.run(sa.load_indexed(ds, index, params)).clone(), sb.run(sb.load_indexed(ds, index, params)).clone()
        assert torch.equal(la, lb), (s, la.tolist(), lb.tolist())
        assert torch.equal(ma.flat_g, mb.flat_g), s
    assert any(ent[2] is not None for ent in sa._graphs.values())
    assert torch.equal(ma.flat_p, mb.flat_p)
