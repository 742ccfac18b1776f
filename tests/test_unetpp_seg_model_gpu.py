"""The single-task U-Net++ segmentation model (nets.BasicUnetPlusPlus, `architecture: UnetPlusPlus`) on the GPU, 2 x 1 x 64 x 64 throughout
(the smallest input that leaves a 4 x 4 map at level 4): the fp32 step against the float64 oracle of tests/unetpp_seg_oracle.py, the step as
the subgraph of the MTUNetPlusPlus step, fused against drop-in, graph replay, the dynamic loss scale, the never-trained heads without deep
supervision, and the fold loop with the segmentation test phase.  Nothing of the reference pins this model (MONAI is not installed): the
oracle is this repository's restatement.  The 16-bit modes rest on the bit-equality with the multi-task step below and on the launch cases of
tests/test_unetpp_seg_launches_gpu.py; the emulation comparison of tests/test_model_gpu.py is written around class logits and does not take
this model.

(Named to run behind tests/test_coop_safety_gpu.py, as tests/test_mt_btsunet_model_gpu.py is: the graph captures below draw side streams.)"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

from multi_task_breast_cancer_amd import checkpoint as CK  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import inference as I  # noqa: E402
from multi_task_breast_cancer_amd import nets  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import unetpp_seg_oracle as U  # noqa: E402

DEV = torch.device("cuda:0")
TOL = 1e-4           # the project's pinned fp32 bound (tests/test_model_gpu.py)
GRAD_FLOOR = 5e-3    # tests/test_mt_btsunet_model_gpu.py: the floor of the 3x rule where no LeakyReLU sign flipped (5e-2 where one did)
WEIGHT_TOL = 2e-4    # tests/test_model_gpu.py: after one Adam step of lr 1e-4 every weight within 2 x lr of the oracle's
SIX = [f"final_conv_0_{j}.{p}" for j in (1, 2, 3) for p in ("weight", "bias")]


def _model(ds=True, dtype="f32", seed=1993, features=nets.BASIC_UNETPP_FEATURES):
    seed_everything(seed)
    m = nets.BasicUnetPlusPlus(2, 1, 1, features, ds).to(DEV)
    m.set_compute(dtype)
    return m


def _batch(seed, n=2):
    img, mask, label = O.synthetic_batch(n, 64, 64, seed=seed)
    return img.to(DEV), mask.to(DEV), label.to(DEV)


def _forward_and_loss(st):
    """pack -> fwd -> loss of a loaded step: (loss words, the heads' outputs) -- cloned before the backward, which reuses the outputs' memory."""
    for p in ("pack", "fwd", "loss"):
        st.programs[p].run()
    torch.cuda.synchronize()
    return st.plan.loss_out.clone(), [h.data.clone() for h in st.segs]


def _backward(model, st):
    st.programs["bwd"].run()
    torch.cuda.synchronize()
    return {n: model._grad_view(n).clone() for n in model._order if n not in model.untrained}


# ------------------------------------------------------------------------------------------------ against the oracle
def test_fp32_step_matches_the_float64_oracle():
    """Default widths, deep supervision, fp32 mode.  The four heads and the loss words within 1e-4 of the float64 oracle (the fp32 contract);
    every parameter's gradient, relative L2 against the float64 oracle's, within 3 x the float32 oracle run's own distance, floor 5e-3 -- 5e-2
    where a LeakyReLU pre-activation inside the forward rounding band changed sign (counted) --, the rule of
    tests/test_mt_btsunet_model_gpu.py; after one fused Adam step of lr 1e-4 every weight within 2e-4 of the float32 oracle's after torch's.
    The printed distances are profiles/unetpp_seg_parity.txt.  Measured on an MI355X: see that file."""
    torch.set_num_threads(8)
    m = _model()
    m.ensure_flat()
    ref = U.OracleBasicUnetPlusPlus(1, 1, U.FEATURES, True)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    ref64 = copy.deepcopy(ref).double()
    img, mask, _ = O.synthetic_batch(2, 64, 64, seed=66)
    step = T.FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4))
    st = step.load_batch(img.to(DEV), mask.to(DEV))
    words, heads = _forward_and_loss(st)
    # the float64 run, with every conv cell's activation kept for the sign count
    acts64 = {}
    hooks = [mod.register_forward_hook(lambda m_, i, o, name=name: acts64.__setitem__(name, o.detach()))
             for name, mod in ref64.named_modules() if name in st.plan.acts]
    loss64, outs64 = U.train_step(ref64, O.make_adam(ref64, 1e-4), img.double(), mask.double())
    for h in hooks:
        h.remove()
    flips = elements = compared = 0
    worst_flip = 0.0
    for name, want in acts64.items():
        act = st.plan.acts[name]
        if act.in_op is None or not act.planar_valid or tuple(act.data.shape) != tuple(want.shape):
            continue
        f = (act.data.cpu() > 0) != (want > 0)
        flips, elements, compared = flips + int(f.sum()), elements + f.numel(), compared + 1
        if f.any():
            worst_flip = max(worst_flip, want[f].abs().max().item())
    grads = _backward(m, st)
    loss32, outs32 = U.train_step(ref, O.make_adam(ref, 1e-4), img, mask)
    assert len(heads) == 4 == len(outs64)
    e_heads = [(g.cpu().double() - w).abs().max().item() for g, w in zip(heads, outs64)]
    r_heads = [(a.double() - w).abs().max().item() for a, w in zip(outs32, outs64)]
    e_loss = [abs(words[i].item() - loss64.item()) for i in (0, 1)]
    print(f"heads: max |head - f64| {[f'{e:.2e}' for e in e_heads]} (the float32 oracle run: {[f'{e:.2e}' for e in r_heads]})")
    print(f"loss words: |word - f64| {e_loss[0]:.2e} {e_loss[1]:.2e} (the float32 oracle run: {abs(loss32.item() - loss64.item()):.2e}); "
          f"loss {loss64.item():.6f}")
    print(f"LeakyReLU sign flips against the float64 forward: {flips} of {elements} over {compared} activations, largest flipped |value| {worst_flip:.2e}")
    assert max(e_heads) < TOL and max(e_loss) < TOL
    assert words[0].item() == words[1].item() and words[2].item() == 0.0 and words[3].item() == 0.0          # [seg, seg, 0, nan flag]
    assert compared >= 25, compared                      # the activation names do line up with the oracle's modules
    assert flips <= max(8, 3e-6 * elements) and worst_flip < 1e-4, (flips, worst_flip, elements)
    floor = GRAD_FLOOR if flips == 0 else 5e-2
    r32, r64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad, judged = [], 0
    for name in m._order:
        g64 = r64[name].grad
        gn = g64.norm().item()
        if gn / g64.numel() ** 0.5 < 1e-9:               # a conv bias in front of an InstanceNorm: the true gradient is 0
            print(f"grad {name}: |g64| {gn:.2e}, not judged")
            continue
        e = (grads[name].cpu().double() - g64).norm().item() / gn
        e32 = (r32[name].grad.double() - g64).norm().item() / gn
        judged += 1
        print(f"grad {name}: relative distance to float64 {e:.3e}, the float32 oracle run {e32:.3e}")
        if not e <= max(3 * e32, floor):
            bad.append((name, e, e32))
    assert judged >= 100 and not bad, (bad, flips)
    # one fused Adam step (a second model from the same seed: the step above stopped in front of the optimizer)
    m2 = _model()
    T.FusedTrainStep(m2, FusedAdam(m2, lr=1e-4, eps=1e-4))(img.to(DEV), mask.to(DEV))
    worst = max((m2._param_view(n).cpu() - r32[n].detach()).abs().max().item() for n in m2._order)
    moved = max((m2._param_view(n).cpu() - m.state_dict()[n].cpu()).abs().max().item() for n in m2._order)
    print(f"one Adam step: max |weight - float32 oracle's| {worst:.3e} (the step moved a weight by at most {moved:.3e})")
    assert worst <= WEIGHT_TOL and 0 < moved <= 1.01e-4


# ------------------------------------------------------------------------------------------------ against MTUNetPlusPlus
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_seg_only_step_is_the_subgraph_of_the_multitask_step(dtype):
    """Built with features=nets.UNETPP_FEATURES and the same seed, the model's initial weights are MTUNetPlusPlus's trunk bit for bit; with
    alpha = 1 the multi-task step sends a zero gradient into its class logits, adding zeros is exact, and so every head, the segmentation loss
    word and the gradient of every shared parameter equal the segmentation-only step's bit for bit -- those upstream of x_3_0, x_3_1 and
    x_4_0 too, into whose gradients the multi-task plan accumulates a second reader's (the classifier's, here zeros): measured on an MI355X,
    no tensor differs in any of the three modes, so none is excepted."""
    img, mask, label = _batch(21)
    seg = _model(True, dtype, features=nets.UNETPP_FEATURES)
    seed_everything(1993)
    mt = nets.MTUNetPlusPlus(2, 1, 1, 3, deep_supervision=True).to(DEV)
    mt.set_compute(dtype)
    seg.ensure_flat(), mt.ensure_flat()
    assert list(seg._order) == list(mt._order)[:len(seg._order)]
    for n in seg._order:
        assert torch.equal(seg._param_view(n), mt._param_view(n)), n
    st_s = T.FusedTrainStep(seg, FusedAdam(seg, lr=1e-4, eps=1e-4)).load_batch(img, mask)
    ls, heads_s = _forward_and_loss(st_s)
    gs = _backward(seg, st_s)
    st_m = T.FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4), alpha=1.0).load_batch(img, mask, label)
    lm, heads_m = _forward_and_loss(st_m)
    gm = _backward(mt, st_m)
    assert float(gm["classifier.5.weight"].abs().max()) == 0.0             # the zero class-logit gradient
    print(dtype, "loss words", ls.tolist(), lm.tolist())
    assert len(heads_s) == len(heads_m) == 4
    for j, (got, want) in enumerate(zip(heads_s, heads_m)):
        assert torch.equal(got, want), f"{dtype}: head {j + 1} differs by {(got - want).abs().max().item():.3e}"
    assert ls[1].item() == lm[1].item() and ls[0].item() == ls[1].item()
    scale = seg.loss_scale
    diff = [(n, ((gs[n] - gm[n]).norm() / gm[n].norm()).item(), (gm[n].abs().max() / scale).item()) for n in seg._order if not torch.equal(gs[n], gm[n])]
    for row in diff:
        print(dtype, "gradient differs (name, relative L2, |g|max):", row)
    assert not diff, f"{dtype}: {len(diff)} shared parameters' gradients differ, the last in backward order: {diff[0]}"


# ------------------------------------------------------------------------------------------------ fused and drop-in
@pytest.mark.parametrize("ds", [True, False], ids=["ds", "nods"])
def test_fused_step_is_the_drop_in_autograd_step(ds):
    """training_segmentation.py:40-57 on the drop-in surface (model(x), the Dice module, apply_criterion_binary_segmentation, backward, the
    optimizer) against the fused step: one forward program behind both, so the heads are bit-equal; the loss within 1e-6 and every weight
    after the Adam step within 1e-7, the bounds tests/test_seg_nnunet_gpu.py holds nnUNet to."""
    img, mask, _ = _batch(41)
    a = _model(ds, seed=7)
    a.train(True)
    oa = FusedAdam(a, lr=1e-4, eps=1e-4)
    oa.zero_grad(set_to_none=True)
    outs = a(img)
    assert isinstance(outs, list) and len(outs) == (4 if ds else 1) and all(tuple(o.shape) == (2, 1, 64, 64) for o in outs)
    loss = CR.apply_criterion_binary_segmentation(CR.DiceLoss(), mask, outs, True)
    loss.backward()
    assert all((p.grad is None) == (n in a.untrained) for n, p in a.named_parameters())
    oa.step()
    b = _model(ds, seed=7)
    step = T.FusedTrainStep(b, FusedAdam(b, lr=1e-4, eps=1e-4))
    st = step.load_batch(img, mask)
    _, heads = _forward_and_loss(st)
    for x, y in zip(outs, heads):
        assert torch.equal(x.detach(), y)
    words = step.run(st).cpu()
    assert abs(words[0].item() - loss.item()) < 1e-6 and words[0].item() == words[1].item() and words[2].item() == 0.0 and words[3].item() == 0.0
    worst = max((a._param_view(n) - b._param_view(n)).abs().max().item() for n in a._order)
    print("fused against drop-in after one Adam step: max |dparam|", worst)
    assert worst < 1e-7


@pytest.mark.parametrize("name", ["BCE", "FocalDICE", "Jaccard"])
def test_other_seg_criteria_take_the_model(name):
    m = _model()
    before = m.state_dict()["final_conv_0_4.weight"].clone()
    step = T.FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), seg_criterion=name)
    img, mask, _ = _batch(3)
    losses = step(img, mask).cpu()
    assert torch.isfinite(losses).all() and losses[0] == losses[1] and losses[2] == 0 and losses[3] == 0 and losses[0] > 0
    assert not torch.equal(m.state_dict()["final_conv_0_4.weight"], before)


@pytest.mark.parametrize("dtype,opt_cls", [("f16", FusedAdam), ("f32", FusedSGD), ("bf16", FusedAdamW)])
def test_graph_replayed_steps_are_the_eager_steps(dtype, opt_cls):
    res = []
    for graph in (False, True):
        m = _model(True, dtype)
        opt = opt_cls(m, lr=1e-3) if opt_cls is not FusedAdam else FusedAdam(m, lr=1e-3, eps=1e-4)
        step = T.FusedTrainStep(m, opt, graph=graph, metrics=True)
        step.begin_epoch_metrics()
        losses = []
        for s in range(5):
            img, mask, _ = _batch(10 + s)
            losses.append(step(img, mask).clone())
        torch.cuda.synchronize()
        step.check_nan()
        if graph:
            assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
        res.append((m.flat_p.clone(), torch.stack(losses), step.epoch_metrics()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert isinstance(res[0][2], T.SegTrainMetrics) and res[0][2].batches == res[1][2].batches == 5 and np.array_equal(res[0][2].table, res[1][2].table)
    assert res[0][2].loss == res[1][2].loss and res[0][2].dice == res[1][2].dice


def test_dynamic_loss_scale_without_overflow_is_the_static_scale():
    res = []
    for scale in (None, DynamicLossScale(init_scale=65536.0, growth_interval=10 ** 6)):
        m = _model(True, "f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        step = T.FusedTrainStep(m, opt, loss_scale=scale)
        losses = [step(*_batch(30 + s)[:2]).clone() for s in range(3)]
        torch.cuda.synchronize()
        step.check_nan()
        res.append((m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.stack(losses), step))
    for a, b, what in zip(res[0][:4], res[1][:4], ("parameters", "exp_avg", "exp_avg_sq", "losses")):
        assert torch.equal(a, b), f"dynamic against static: {what} differ, max |diff| {(a - b).abs().max().item():.3e}"
    assert res[1][4].scaler.stats() == {"scale": 65536.0, "growth_tracker": 3, "skipped": 0, "t": 3}


# ------------------------------------------------------------------------------------------------ without deep supervision
@pytest.mark.parametrize("kind", [FusedAdam, FusedSGD, FusedAdamW])
def test_never_trained_heads_stay_bit_equal_and_stateless(kind):
    """deep_supervision=False: final_conv_0_1 .. 0_3 (weight and bias) are parameters the forward's result never reads.  After three steps of
    each fused optimizer -- AdamW's decay included -- they hold their initial bits, their .grad is None and the optimizer's state_dict has no
    entry for them; every other tensor has a gradient and the trunk has moved."""
    m = _model(False)
    m.ensure_flat()
    assert sorted(m.untrained) == sorted(SIX)
    initial = {n: m._param_view(n).clone() for n in m._order}
    opt = FusedAdam(m, lr=1e-3, eps=1e-4) if kind is FusedAdam else kind(m, lr=1e-3)
    step = T.FusedTrainStep(m, opt)
    for s in range(3):
        img, mask, _ = _batch(50 + s)
        losses = step(img, mask)
    step.check_nan()
    assert bool(torch.isfinite(losses).all())
    params = dict(m.named_parameters())
    for n in SIX:
        assert torch.equal(m._param_view(n), initial[n]) and torch.equal(params[n].detach(), initial[n]), n
        assert params[n].grad is None, n
    assert all(params[n].grad is not None for n in m._order if n not in m.untrained)
    # every live tensor but the conv biases in front of an InstanceNorm has a gradient that is not zero, and both ends of the trunk have moved
    # (not every tensor: under SGD a norm weight of 1.0 at the 4 x 4 level keeps its bits where lr x gradient is below half an ulp of 1)
    flat = [n for n in m._order if n not in m.untrained and not n.endswith("conv.bias") and float(m._grad_view(n).abs().max()) == 0.0]
    assert not flat, flat
    for n in ("conv_0_0.conv_0.conv.weight", "conv_4_0.convs.conv_1.conv.weight", "upcat_0_4.convs.conv_1.conv.weight", "final_conv_0_4.weight", "final_conv_0_4.bias"):
        assert not torch.equal(m._param_view(n), initial[n]), n
    dead = {i for i, n in enumerate(m._order) if n in m.untrained}
    assert len(dead) == 6 and set(opt.state_dict()["state"]) == set(range(len(m._order))) - dead
    outs = m(_batch(50)[0])
    assert isinstance(outs, list) and len(outs) == 1


# ------------------------------------------------------------------------------------------------ the driver
def test_fit_fold_runs_the_segmentation_driver(tmp_path):
    """trainer.fit_fold for two epochs on 16 synthetic images with the model the factory returns: indexed training with metrics, on-device
    validation, the testing phase (FusedSegTestStep) behind every epoch, the segmentation driver's metrics.csv, and results_segmentation.csv."""
    from multi_task_breast_cancer_amd.experiment_init import init_segmentation_model
    img, mask, label = O.synthetic_batch(16, 64, 64, seed=33)
    ds = DD.DeviceDataset(img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long())
    seed_everything(1993)
    model = init_segmentation_model("UnetPlusPlus", sequences=1, regions=1, deep_supervision=True).to(DEV)
    opt = FusedAdam(model, lr=1e-3, eps=1e-4)
    step = T.FusedTrainStep(model, opt, metrics=True)
    eval_step, test_step = T.FusedEvalStep(model, on_device=True), I.FusedSegTestStep(model)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    run_dir = str(tmp_path / "fold_0")
    train, val, test = EpochIndex(np.arange(10), 4, seed=13, drop_last=False), EpochIndex(np.arange(10, 13), 2, seed=13, drop_last=False), \
        EpochIndex(np.arange(13, 16), 2, seed=13, drop_last=False)
    rows = T.fit_fold(step, eval_step, ds, train, val, scheduler, run_dir, epochs=2, max_patience=5,
                      transforms={"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 217 / 360}, seed=13, plateau=False,
                      test_step=test_step, test_index=test)
    assert len(rows) == 2 and all(len(r) == 7 for r in rows) and [r[0] for r in rows] == [0, 1]
    lines = open(os.path.join(run_dir, "metrics.csv")).read().splitlines()
    assert lines[0] == CK.SEG_METRICS_HEADER and len(lines) == 3
    for line, r in zip(lines[1:], rows):
        assert line == f"{r[0]},{r[1]:.8f},{r[2]:.4f}, {r[3]:.4f},{r[4]:.4f},{r[5]:.4f},{r[6]:.4f}"
        assert all(0.0 <= v <= 1.0 for v in r[2:5]) and r[5] > 0 and r[6] > 0
    got = T.test_one_epoch_indexed(test_step, ds, DD.EpochTables(test, 0, None, device=ds.device))
    assert len(got) == 3 and rows[1][4] == float(np.mean([r["DICE"] for r in got]))
    file = test_step.write_csv(run_dir)
    assert os.path.basename(file) == "results_segmentation.csv" and len(open(file).read().splitlines()) == 4
    ckpt = torch.load(os.path.join(run_dir, "model_best"), map_location="cpu", weights_only=False)
    assert list(ckpt["model_state_dict"]) == list(model.state_dict())
