"""The segmentation criteria of the fused step beside Dice -- BCE, Dice+Focal ("FocalDICE"), Jaccard (experiment_init.py:199-232) -- on the GPU:
the kernels against float64 autograd restatements and closed forms, then one optimisation step of the whole model through the fused step and
through the drop-in loop against the CPU oracle.

The restatements (the MONAI ones from knowledge of MONAI 1.3.0, as oracle.torch_oracle.dice_loss_sigmoid_sq is):
  BCE        torch.nn.functional.binary_cross_entropy_with_logits, mean over all elements
  FocalDICE  DiceFocalLoss(include_background, sigmoid, squared_pred, smooth 1 / 1): the squared-pred Dice term (mean over planes) + the mean over
             all elements of exp(gamma logsigmoid(-x (2t - 1))) * bce, gamma 2
  Jaccard    DiceLoss(include_background, sigmoid, jaccard=True, reduction="sum"): sum over planes of 1 - (2I + 1e-5) / (2 (P + T - I) + 1e-5)"""
import ctypes as C
import math
import os
import socket

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_criterion_segmentation  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedEvalStep, FusedTrainStep  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = [L.SEG_DICE, L.SEG_BCE, L.SEG_FOCALDICE, L.SEG_JACCARD]
NAME = {L.SEG_DICE: "DICE", L.SEG_BCE: "BCE", L.SEG_FOCALDICE: "FocalDICE", L.SEG_JACCARD: "Jaccard"}


# ------------------------------------------------------------------------------------------------ restatements (any float dtype)
def _bce(x, t):
    return F.binary_cross_entropy_with_logits(x, t)


def _focal_dice(x, t, gamma=2.0):
    s = 2.0 * t - 1.0
    focal = torch.exp(gamma * F.logsigmoid(-x * s)) * F.binary_cross_entropy_with_logits(x, t, reduction="none")
    return O.dice_loss_sigmoid_sq(x, t, 1.0, 1.0) + focal.mean()


def _jaccard(x, t, smooth=1e-5):
    p = torch.sigmoid(x)
    dims = tuple(range(2, x.dim()))
    inter, ps, ts = (p * t).sum(dims), p.sum(dims), t.sum(dims)
    return (1.0 - (2.0 * inter + smooth) / (2.0 * (ps + ts - inter) + smooth)).sum()


RESTATED = {L.SEG_DICE: O.dice_loss_sigmoid_sq, L.SEG_BCE: _bce, L.SEG_FOCALDICE: _focal_dice, L.SEG_JACCARD: _jaccard}
BY_NAME = {NAME[k]: f for k, f in RESTATED.items()}


def _close(got, want, rtol, atol, what=""):
    got = got.detach().cpu().double()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, max |want| {want.abs().max().item():.3e}"


def _against_float64(kind, xs, t, weights, gscale):
    """ops.dice_multihead(kind) on float32 device copies against the float64 autograd restatement of the same values: the tolerances of
    test_dice_multihead_matches_oracle (per-head loss 2e-6, total 5e-6, dx rel 1e-4 / abs 1e-9); Jaccard's loss is a SUM of `planes` terms of the
    size of one Dice term, so its two loss bounds are multiplied by the number of planes."""
    planes = t.shape[0] * t.shape[1]
    lscale = planes if kind == L.SEG_JACCARD else 1
    xr = [x.double().requires_grad_(True) for x in xs]
    each = [RESTATED[kind](x, t.double()) for x in xr]
    total = sum(w * e for w, e in zip(weights, each))
    (gscale * total).backward()
    loss, dxs = ops.dice_multihead([x.to(DEV) for x in xs], t.to(DEV), weights, gscale=gscale, kind=kind)
    loss = loss.cpu()
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(d).all()) for d in dxs)
    for i in range(len(xs)):
        err = abs(loss[i].item() - each[i].item())
        print(f"{NAME[kind]} head {i}: loss {loss[i].item():.7f} err {err:.2e}; dx max err {(dxs[i].cpu().double() - xr[i].grad).abs().max().item():.2e}")
        assert err < 2e-6 * lscale, (i, loss[i].item(), each[i].item())
        _close(dxs[i], xr[i].grad, 1e-4, 1e-9, f"{NAME[kind]} dx head {i}")
    assert abs(loss[len(xs)].item() - total.item()) < 5e-6 * lscale, (loss[len(xs)].item(), total.item())


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("kind", KINDS)
def test_multihead_matches_float64(kind):
    g = torch.Generator().manual_seed(9)
    N, H, W = 3, 64, 64
    xs = [torch.randn(N, 1, H, W, generator=g) * 2 for _ in range(4)]
    t = (torch.rand(N, 1, H, W, generator=g) > 0.7).float()
    t[1] = 0                                              # empty mask (class "normal")
    _against_float64(kind, xs, t, [1 / 4, 1 / 3, 1 / 2, 1.0], 0.35)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", [(6, 5), (4, 4)])
def test_scalar_path_and_plane_smaller_than_the_block(kind, H, W):
    """6 x 5: HW % 4 != 0, the scalar loops; 4 x 4: fewer elements than threads (and than one 16-byte round per thread)."""
    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(2, 1, H, W, generator=g) * 2 for _ in range(2)]
    t = (torch.rand(2, 1, H, W, generator=g) > 0.5).float()
    _against_float64(kind, xs, t, [0.5, 1.0], 0.35)


@pytest.mark.parametrize("kind", KINDS)
def test_1024_thread_path(kind):
    """HW = 16384: the 1024-thread blocks, every thread exactly the four rounds in flight."""
    g = torch.Generator().manual_seed(22)
    xs = [torch.randn(1, 1, 128, 128, generator=g) * 2]
    t = (torch.rand(1, 1, 128, 128, generator=g) > 0.7).float()
    _against_float64(kind, xs, t, [1.0], 0.35)


@pytest.mark.parametrize("kind", KINDS)
def test_saturated_logits_stay_finite(kind):
    """Logits of +-30 on both mask values inside a 16 x 16 plane: exp(30) in a naive softplus / a 0 * inf in the focal modulator would show as
    inf / NaN; finiteness is asserted in the helper, the values against float64 within the same tolerances."""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(1, 1, 16, 16, generator=g) * 2
    t = (torch.rand(1, 1, 16, 16, generator=g) > 0.5).float()
    flat = x.view(-1)
    flat[0:64:8] = 30.0
    flat[4:64:8] = -30.0
    assert {(30.0, 0.0), (30.0, 1.0), (-30.0, 0.0), (-30.0, 1.0)} <= set(zip(flat.tolist(), t.view(-1).tolist()))
    _against_float64(kind, [x], t, [1.0], 0.35)


def test_closed_forms_on_zero_logits_and_zero_mask():
    """x = 0, t = 0, HW = 256: p = 1/2.  BCE: softplus(0) = ln 2.  FocalDICE: Dice 1 - 1 / (0.25 HW + 1), focal sigmoid(0)^2 ln 2 = ln 2 / 4.
    Jaccard: I = 0, P = HW / 2, T = 0: each of the N planes gives 1 - 1e-5 / (HW + 1e-5), summed."""
    N = 2
    z = torch.zeros(N, 1, 16, 16, device=DEV)
    want = {L.SEG_BCE: math.log(2.0), L.SEG_FOCALDICE: 1 - 1 / (0.25 * 256 + 1) + 0.25 * math.log(2.0),
            L.SEG_JACCARD: N * (1 - 1e-5 / (256 + 1e-5))}
    for kind, w in want.items():
        l, _ = ops.dice_multihead([z], z.clone(), [1.0], kind=kind)
        assert abs(l[0].item() - w) < 1e-6 * (N if kind == L.SEG_JACCARD else 1), (NAME[kind], l[0].item(), w)


def test_default_kind_is_the_dice_call():
    g = torch.Generator().manual_seed(9)
    xs = [(torch.randn(3, 1, 64, 64, generator=g) * 2).to(DEV) for _ in range(4)]
    t = (torch.rand(3, 1, 64, 64, generator=g) > 0.7).float().to(DEV)
    w = [1 / 4, 1 / 3, 1 / 2, 1.0]
    l0, d0 = ops.dice_multihead(xs, t, w, gscale=0.35)
    l1, d1 = ops.dice_multihead(xs, t, w, gscale=0.35, kind=0)
    l2, d2 = ops.dice_multihead(xs, t, w, 0.35, L.SEG_DICE, (1.0, 1.0), 2.0)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    for a, b, c in zip(d0, d1, d2):
        assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(L.MtbcError):                       # a kind outside the four is refused by the library, not read as Dice
        a = L.DiceArgs()
        a.n_heads, a.N, a.C, a.H, a.W, a.kind = 1, 1, 1, 4, 4, 4
        a.x[0], a.target = xs[0].data_ptr(), t.data_ptr()
        buf = torch.empty(8, device=DEV)
        a.stats = a.loss = buf.data_ptr()
        L.check(L.load().mtbc_dice_fwd(C.byref(a), None), "dice_fwd")


# ------------------------------------------------------------------------------------------------ model level (MTnnUNet, 2 x 1 x 64 x 64, fp32)
ALPHA = 0.35


def _pair(seed=3):
    seed_everything(seed)
    prod = MTnnUNet(1, 1, 3)
    ref = O.build_oracle_model("MTnnUNet", 1, 1, 3, True)
    ref.load_state_dict(prod.state_dict())
    return prod.to(DEV), ref


def _oracle_losses(ref, crit, img, mask, onehot):
    rl, ro = ref(img)
    rseg = sum(crit(o, mask) / (j + 1) for j, o in enumerate(reversed(ro)))
    rcls = sum(O.focal_loss_soft(l, onehot) for l in reversed(rl))
    return ALPHA * rseg + (1 - ALPHA) * rcls, rseg, rcls


def _oracle_step(ref, crit, img, mask, onehot):
    ropt = O.make_adam(ref, 1e-4)                           # torch.optim.Adam(eps=1e-4)
    ropt.zero_grad()
    rtot, rseg, rcls = _oracle_losses(ref, crit, img, mask, onehot)
    rtot.backward()
    ropt.step()
    return rtot.item(), rseg.item(), rcls.item()


def _assert_params(prod, ref, what):
    for (k, a), (_, b) in zip(prod.state_dict().items(), ref.state_dict().items()):
        assert (a.cpu() - b).abs().max().item() < 2.0e-4, (what, k)


@pytest.mark.parametrize("name", ["BCE", "FocalDICE", "Jaccard"])
def test_fused_step_matches_oracle(name):
    """One FusedTrainStep(seg_criterion=name) step against the oracle model + the restated criterion + torch.optim.Adam(eps=1e-4): losses
    within 1e-4, every parameter within 2e-4 (the bounds of test_dropin_loop_with_torch_classification_criteria)."""
    prod, ref = _pair()
    img, mask, label = O.synthetic_batch(2, 64, 64, seed=8)
    onehot = F.one_hot(label.flatten().long(), 3).float()
    step = FusedTrainStep(prod, FusedAdam(prod, lr=1e-4, eps=1e-4), alpha=ALPHA, inversely_weighted=True, seg_criterion=name)
    got = step(img.to(DEV), mask.to(DEV), label.to(DEV)).cpu()
    step.check_nan()
    want = _oracle_step(ref, BY_NAME[name], img, mask, onehot)
    for i in range(3):
        assert abs(got[i].item() - want[i]) < 1e-4, (name, got.tolist(), want)
    _assert_params(prod, ref, name)


@pytest.mark.parametrize("name", ["FocalDICE", "Jaccard"])
def test_dropin_loop_matches_oracle(name):
    """The same step through the factory's module, the reference's aggregation and autograd (training_multitask.py:87-103)."""
    prod, ref = _pair()
    img, mask, label = O.synthetic_batch(2, 64, 64, seed=8)
    onehot = F.one_hot(label.flatten().long(), 3).float()
    seg_c = init_criterion_segmentation(name)
    opt = FusedAdam(prod, lr=1e-4, eps=1e-4)
    opt.zero_grad(set_to_none=True)
    logits, outs = prod(img.to(DEV))
    seg, cls = CR.apply_criterion_multitask_segmentation_classification(seg_c, mask.to(DEV), outs, CR.FocalLoss(alpha=1, gamma=2), onehot.to(DEV), logits, True)
    total = ALPHA * seg + (1 - ALPHA) * cls
    total.backward()
    opt.step()
    want = _oracle_step(ref, BY_NAME[name], img, mask, onehot)
    for g, w in zip((total, seg, cls), want):
        assert abs(g.item() - w) < 1e-4, (name, total.item(), seg.item(), cls.item(), want)
    _assert_params(prod, ref, name)


def test_bce_graph_replay_is_the_eager_step_and_eval_shares_the_plan():
    batches = [O.synthetic_batch(2, 64, 64, seed=30 + s) for s in range(3)]
    res = []
    for graph in (False, True):
        prod, _ = _pair()
        opt = FusedAdam(prod, lr=1e-4, eps=1e-4)
        step = FusedTrainStep(prod, opt, alpha=ALPHA, inversely_weighted=True, seg_criterion="BCE", graph=graph)
        losses = [step(*(t.to(DEV) for t in b)).clone() for b in batches]
        torch.cuda.synchronize()
        step.check_nan()
        if graph:
            assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
        res.append((prod.flat_p.clone(), torch.stack(losses)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # the evaluation step with the same (N, H, W, alpha, weighting, criteria): the training step's compiled plan, the oracle's BCE loss
    n_plans = len(prod._steps)
    ev = FusedEvalStep(prod, alpha=ALPHA, inversely_weighted=True, seg_criterion="BCE")
    img, mask, label = batches[0]
    ev(img.to(DEV), mask.to(DEV), label.to(DEV))
    got = ev.result()
    assert len(prod._steps) == n_plans
    ref = O.build_oracle_model("MTnnUNet", 1, 1, 3, True)
    ref.load_state_dict({k: v.cpu() for k, v in prod.state_dict().items()})
    ref.train(False)
    with torch.no_grad():
        tot, seg, cls = _oracle_losses(ref, _bce, img, mask, F.one_hot(label.flatten().long(), 3).float())
    assert abs(got[4] - seg.item()) < 1e-4 and abs(got[0] - tot.item()) < 1e-4 and abs(got[5] - cls.item()) < 1e-4, (got, tot, seg, cls)
    # another criterion is another plan
    FusedEvalStep(prod, alpha=ALPHA, inversely_weighted=True, seg_criterion="Jaccard")(img.to(DEV), mask.to(DEV), label.to(DEV))
    assert len(prod._steps) == n_plans + 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bce_distributed_single_rank_rccl_equals_local_step():
    """The data-parallel path at world size 1 (real RCCL launches) with a mean criterion: bit for bit the local step."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        res = []
        for distributed in (False, True):
            seed_everything(1993)
            m = MTnnUNet(1, 1, 3).to(DEV)
            step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=ALPHA, distributed=distributed, n_buckets=4, seg_criterion="BCE")
            img, mask, label = O.synthetic_batch(2, 64, 64, seed=4)
            for _ in range(2):
                l = step(img.to(DEV), mask.to(DEV), label.to(DEV))
            torch.cuda.synchronize()
            if distributed:
                assert len(step._st.buckets) >= 2
            res.append((m.flat_p.clone(), l.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    finally:
        dist.destroy_process_group()


def test_refusals():
    m = MTnnUNet(1, 1, 3).to(DEV)
    opt = FusedAdam(m, lr=1e-4, eps=1e-4)
    with pytest.raises(NotImplementedError, match="sum"):             # a sum over the batch is not a mean under data parallelism
        FusedTrainStep(m, opt, alpha=ALPHA, seg_criterion="Jaccard", distributed=True)
    for bad in ("CrossentropyDICE", "GeneralizedDICE", "dice"):
        with pytest.raises(ValueError):
            FusedTrainStep(m, opt, alpha=ALPHA, seg_criterion=bad)
        with pytest.raises(ValueError):
            FusedEvalStep(m, alpha=ALPHA, seg_criterion=bad)
