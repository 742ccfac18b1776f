"""Multi_BTSUNet on the GPU: forward, losses and gradients against the reference's float64 numbers (tests/golden/mt_btsunet_step.npz), the
step equivalences (fused against drop-in, graph replay, dynamic loss scale, a step from a trained state against tests/bts_oracle.py), the
16-bit modes against the oracle under oracle.torch_oracle's emulation, and the test phase and fold loop end to end.

Where this file stands in the suite matters to another one: every graph capture (trainer._capture) draws a side stream from torch's
round-robin pool, and tests/test_coop_safety_gpu.py needs ITS side stream on another hardware queue than the default stream (with four
queues, one pool position in four shares it, and the hog then runs in front of the steps instead of beside them).  The two captures below
moved that position when this file ran in front of it; named as it is, it runs behind."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import inference as I  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import Multi_BTSUNet  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import bts_oracle as B  # noqa: E402

DEV = torch.device("cuda:0")
TOL = 1e-4          # the project's pinned fp32 bound (tests/test_model_gpu.py)
GRAD_FLOOR = 5e-3   # ... and the floor of its 3x rule for gradients where no LeakyReLU sign flipped


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "mt_btsunet_step.npz"))


def _model(cfg, seed=1993, dtype="f32"):
    width, n_classes, ds = B.CONFIGS[cfg]
    seed_everything(seed)
    m = Multi_BTSUNet(1, 1, n_classes, width, ds).to(DEV)
    m.set_compute(dtype)
    return m


def _oracle_of(prod, cfg):
    width, n_classes, ds = B.CONFIGS[cfg]
    ref = B.OracleMultiBTSUNet(1, 1, n_classes, width, ds)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in prod.state_dict().items()})
    return ref


def _fixture_batch(fixture, cfg):
    n_classes = B.CONFIGS[cfg][1]
    label = torch.from_numpy(fixture["label"])
    label = (label == 1).float().view(-1, 1) if n_classes == 2 else label.float().view(-1, 1)
    return torch.from_numpy(fixture["image"]).float(), torch.from_numpy(fixture["mask"]).float(), label


def _batch(cfg, n, seed):
    img, mask, label = O.synthetic_batch(n, 128, 128, seed=seed)
    if B.CONFIGS[cfg][1] == 2:
        label = (label == 1).float()
    return img, mask, label


def _dev(batch):
    return tuple(t.to(DEV) for t in batch)


def _step(m, cfg, opt=None, **kw):
    return T.FusedTrainStep(m, opt or FusedAdam(m, lr=1e-4, eps=1e-4), alpha=B.ALPHA, n_classes=B.CONFIGS[cfg][1], **kw)


def _run_programs(st, names=("pack", "fwd", "loss", "bwd")):
    for p in names:
        st.programs[p].run()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ against the reference's numbers
@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_forward_and_losses_match_the_reference_fixture(fixture, cfg):
    """fp32 logits, heads and the three loss words within 1e-4 of the reference's float64 values (the reference's own float32 run: printed)."""
    width, n_classes, ds = B.CONFIGS[cfg]
    m = _model(cfg)
    img, mask, label = _fixture_batch(fixture, cfg)
    m.train(True)
    with torch.no_grad():
        logits, segs = m(img.to(DEV))
    if ds:
        assert isinstance(logits, list) and len(logits) == 1 and isinstance(segs, list) and len(segs) == 3      # Multi_BTS_UNet.py:172
        logits, heads = logits[0], segs
    else:
        assert isinstance(logits, torch.Tensor) and isinstance(segs, torch.Tensor)                              # :176
        heads = [segs]
    assert tuple(logits.shape) == (2, m.n_classes) and all(tuple(h.shape) == (2, 1, 128, 128) for h in heads)
    e_logits = (logits.cpu().double() - torch.from_numpy(fixture[f"{cfg}.logits"])).abs().max().item()
    e_heads = []
    for i, h in enumerate(heads):
        idx = B.sample_index(h.numel(), 100 + i)
        e_heads.append((h.cpu().double().reshape(-1)[idx] - torch.from_numpy(fixture[f"{cfg}.head{i}"])).abs().max().item())
        # the whole head through its per-sample sums: 16384 elements, each within TOL
        assert (h.cpu().double().sum(dim=(1, 2, 3)) - torch.from_numpy(fixture[f"{cfg}.head{i}_sum"])).abs().max().item() < TOL * 16384
    st = _step(m, cfg).load_batch(*_dev((img, mask, label)))
    _run_programs(st, ("pack", "fwd", "loss"))
    words = st.plan.loss_out.cpu().double()
    e_loss = (words[:3] - torch.from_numpy(fixture[f"{cfg}.losses"])).abs().max().item()
    print(f"{cfg}: |logits - f64| {e_logits:.2e} (reference float32: {float(fixture[cfg + '.logits_ref32']):.2e}), heads {max(e_heads):.2e} "
          f"({float(fixture[cfg + '.head_ref32']):.2e}), loss words {e_loss:.2e} ({float(fixture[cfg + '.loss_ref32']):.2e})")
    assert e_logits < TOL and max(e_heads) < TOL and e_loss < TOL and words[3].item() == 0.0


@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_gradients_match_the_reference_fixture(fixture, cfg):
    """Each recorded gradient within 3x the reference float32 run's own distance to float64 (relative L2 over the recorded positions), floor
    5e-3: the 3x rule and the floor of tests/test_model_gpu.py."""
    m = _model(cfg)
    st = _step(m, cfg).load_batch(*_dev(_fixture_batch(fixture, cfg)))
    _run_programs(st)
    bad = []
    for j, k in enumerate(B.GRAD_TENSORS):
        g64 = torch.from_numpy(fixture[f"{cfg}.grad.{k}"])
        got = m._grad_view(k).cpu().double().reshape(-1)[B.sample_index(m._grad_view(k).numel(), 200 + j)]
        e, e_ref = ((got - g64).norm() / g64.norm()).item(), float(fixture[f"{cfg}.grad_ref32.{k}"])
        print(f"{cfg} {k}: relative distance to float64 {e:.3e}, the reference's float32 run {e_ref:.3e}")
        if not e <= max(3 * e_ref, GRAD_FLOOR):
            bad.append((k, e, e_ref))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ step equivalences
@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_fused_step_is_the_drop_in_autograd_step(cfg):
    """The reference loop on the drop-in surface (model(x), the criteria modules, backward) against the fused step: one forward and one backward
    program behind both, so logits and heads are bit-equal; the loss mix sits in another place (alpha is baked into the loss ops' gradient
    scale there, multiplied by autograd here: one more rounding), so losses within 1e-6 and gradients within 1e-5 relative per tensor."""
    width, n_classes, ds = B.CONFIGS[cfg]
    img, mask, label = _dev(_batch(cfg, 2, 41))
    a = _model(cfg, 7)
    a.train(True)
    logits, outs = a(img)
    seg_c = CR.DiceLoss(include_background=True, sigmoid=True, smooth_dr=1, smooth_nr=1, squared_pred=True)
    if n_classes == 2:
        cls_c, target = torch.nn.BCEWithLogitsLoss(), label
    else:
        cls_c, target = CR.FocalLoss(alpha=1, gamma=2), torch.nn.functional.one_hot(label.flatten().long(), 3).float()
    seg, cls = CR.apply_criterion_multitask_segmentation_classification(seg_c, mask, outs, cls_c, target, logits, True)
    total = B.ALPHA * seg + (1 - B.ALPHA) * cls
    total.backward()
    ga = {n: p.grad.clone() for n, p in a.named_parameters()}
    b = _model(cfg, 7)
    st = _step(b, cfg).load_batch(img, mask, label)
    _run_programs(st)
    la = logits[0] if ds else logits
    assert torch.equal(la, st.logits.data.view(2, -1))
    for x, y in zip(outs if ds else [outs], st.segs):
        assert torch.equal(x, y.data)
    words = st.plan.loss_out.cpu()
    assert abs(words[0].item() - total.item()) < 1e-6 and abs(words[1].item() - seg.item()) < 1e-6 and abs(words[2].item() - cls.item()) < 1e-6
    worst = max(((ga[n] - b._grad_view(n)).norm() / ga[n].norm()).item() for n in b._order)
    print(cfg, "fused against drop-in: worst relative gradient distance", worst)
    assert worst < 1e-5


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replayed_steps_are_the_eager_steps(dtype):
    cfg = "w8_c3_ds"
    res = []
    for graph in (False, True):
        m = _model(cfg, 3, dtype)
        step = _step(m, cfg, FusedAdam(m, lr=1e-3, eps=1e-4), graph=graph, metrics=True)
        step.begin_epoch_metrics()
        losses = [step(*_dev(_batch(cfg, 2, 10 + s))).clone() for s in range(5)]
        torch.cuda.synchronize()
        step.check_nan()
        if graph:
            assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
        res.append((m.flat_p.clone(), torch.stack(losses), step.epoch_metrics()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].batches == res[1][2].batches == 5 and np.array_equal(res[0][2].conf, res[1][2].conf)


def test_dynamic_loss_scale_without_overflow_is_the_static_scale():
    cfg = "w16_c2"
    res = []
    for scale in (None, DynamicLossScale(init_scale=65536.0, growth_interval=10 ** 6)):
        m = _model(cfg, 3, "f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        step = _step(m, cfg, opt, loss_scale=scale)
        losses = [step(*_dev(_batch(cfg, 2, 30 + s))).clone() for s in range(3)]
        torch.cuda.synchronize()
        step.check_nan()
        res.append((m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.stack(losses)))
    for a, b, what in zip(res[0], res[1], ("parameters", "exp_avg", "exp_avg_sq", "losses")):
        assert torch.equal(a, b), f"dynamic against static: {what} differ, max |diff| {(a - b).abs().max().item():.3e}"


def _count_flips(st, ref64, run):
    """LeakyReLU sign flips of the HIP forward against the float64 oracle, over every conv-cell activation (tests/test_model_gpu.py)."""
    acts = {}
    hooks = [mod.register_forward_hook(lambda m_, i, o, name=name: acts.__setitem__(name, o.detach()))
             for name, mod in ref64.named_modules() if name in st.plan.acts and isinstance(mod, B._Cell)]
    out = run()
    for h in hooks:
        h.remove()
    flips = elements = compared = 0
    worst = 0.0
    for name, want in acts.items():
        act = st.plan.acts[name]
        if act.in_op is None or not act.planar_valid:
            continue
        f = (act.data.cpu() > 0) != (want > 0)
        flips, elements, compared = flips + int(f.sum()), elements + f.numel(), compared + 1
        if f.any():
            worst = max(worst, want[f].abs().max().item())
    return out, flips, elements, compared, worst


@pytest.mark.parametrize("cfg,seed", [("w8_c3_ds", 11), ("w16_c2", 12)])
def test_a_step_from_a_trained_state_matches_the_oracle(cfg, seed):
    """Another seed, four fused steps at lr 1e-3 (Adam state, moved weights, the weight images rebuilt), then ONE step on both sides from the
    same weights: logits, heads and losses within 1e-4 of the float32 oracle; every parameter's gradient against the float64 oracle within
    3x the float32 oracle's own distance, floor 5e-3 -- 5e-2 where a LeakyReLU pre-activation inside the forward rounding band changed
    sign (counted, as tests/test_model_gpu.py counts them)."""
    width, n_classes, ds = B.CONFIGS[cfg]
    torch.set_num_threads(8)
    m = _model(cfg, seed)
    step = _step(m, cfg, FusedAdam(m, lr=1e-3, eps=1e-4))
    for s in range(4):
        step(*_dev(_batch(cfg, 2, 100 + s)))
    step.check_nan()
    ref = _oracle_of(m, cfg)
    ref64 = copy.deepcopy(ref).double()
    img, mask, label = _batch(cfg, 3, 77)          # another batch size: another compiled plan
    st = step.load_batch(*_dev((img, mask, label)))
    _run_programs(st)
    words = st.plan.loss_out.cpu()
    total, seg, cls, rl, ro = O.train_step(ref, O.make_adam(ref, 1e-4), img, mask, label, B.ALPHA, True, n_classes)
    (_, flips, elements, compared, worst) = _count_flips(
        st, ref64, lambda: O.train_step(ref64, O.make_adam(ref64, 1e-4), img.double(), mask.double(), label, B.ALPHA, True, n_classes))
    rl = rl[0] if ds else rl
    assert (st.logits.data.view(3, -1).cpu() - rl.detach()).abs().max().item() < TOL
    for got, want in zip(st.segs, ro if ds else [ro]):
        assert (got.data.cpu() - want.detach()).abs().max().item() < TOL
    assert abs(words[0].item() - total.item()) < TOL and abs(words[1].item() - seg.item()) < TOL and abs(words[2].item() - cls.item()) < TOL
    assert words[3].item() == 0.0
    assert compared >= 15, compared
    assert flips <= max(8, 3e-6 * elements) and worst < 1e-4, (flips, worst, elements)
    floor = GRAD_FLOOR if flips == 0 else 5e-2
    r32, r64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad = []
    for name in m._order:
        g64 = r64[name].grad
        gn = g64.norm().item()
        if gn / g64.numel() ** 0.5 < 1e-9:
            continue
        e = (m._grad_view(name).cpu().double() - g64).norm().item() / gn
        e32 = (r32[name].grad.double() - g64).norm().item() / gn
        if not e <= max(3 * e32, floor):
            bad.append((name, e, e32))
    print(cfg, "flips", flips, "of", elements, "worst", worst, "bad", bad)
    assert not bad, (bad, flips)


@pytest.mark.parametrize("kind", [FusedAdam, FusedSGD, FusedAdamW])
def test_the_three_fused_optimizers_step_the_model(kind):
    cfg = "w8_c3_ds"
    m = _model(cfg, 5)
    m.ensure_flat()
    before = m.flat_p.clone()
    opt = FusedAdam(m, lr=1e-3, eps=1e-4) if kind is FusedAdam else kind(m, lr=1e-3)
    step = _step(m, cfg, opt)
    l0 = step(*_dev(_batch(cfg, 2, 50))).clone()
    for s in range(2):
        step(*_dev(_batch(cfg, 2, 50)))
    l2 = step(*_dev(_batch(cfg, 2, 50))).clone()
    step.check_nan()
    assert bool(torch.isfinite(m.flat_p).all())
    # every tensor has a gradient and moves (not every ELEMENT: a row of classifier.1.weight whose ReLU output is zero for the whole batch has
    # a zero gradient, and Adam / SGD leave it where it is)
    still = [n for n in m._order if torch.equal(m._param_view(n), before[m.slots[n].offset:m.slots[n].offset + m.slots[n].numel].view(m.slots[n].shape))]
    assert not still, still
    assert l2[0].item() < l0[0].item(), (l0.tolist(), l2.tolist())                          # the same batch four times: the loss goes down


# ------------------------------------------------------------------------------------------------ 16-bit modes
@pytest.mark.parametrize("cfg,dtype", [("w16_c2", "bf16"), ("w16_c2", "f16"), ("w8_c3_ds", "bf16"), ("w8_c3_ds", "f16")])
def test_16bit_modes_match_their_emulation(cfg, dtype):
    """The bars of tests/test_model_gpu.py::test_16bit_mfma_modes_match_their_emulation: against the fp64-accumulating emulation, 3x the
    distance the fp32-accumulating CPU emulation has from it, every tensor (floors: 5e-4 loss, 2e-3 outputs, 5e-2 gradients), from a state
    that fp32 steps have moved away from the initialisation.  Width 16: every 3x3 conv but the stem on channel-blocked 16-bit operands, the
    up-sampling moves channel-blocked tensors; width 8: the mixed plan (4-channel tensors stay fp32 planes)."""
    width, n_classes, ds = B.CONFIGS[cfg]
    torch.set_num_threads(8)
    m = _model(cfg, 1993)
    warm = _step(m, cfg, FusedAdam(m, lr=1e-3, eps=1e-4))
    for s in range(10):
        warm(*_dev(_batch(cfg, 2, 100 + s)))
    warm.check_nan()
    ref = _oracle_of(m, cfg)
    m.set_compute(dtype)
    ref64 = copy.deepcopy(ref).double()
    ref.lowp = ref64.lowp = dtype
    img, mask, label = _batch(cfg, 2, 21)
    step = _step(m, cfg)
    st = step.load_batch(*_dev((img, mask, label)))
    losses = step.run(st).cpu()
    if dtype != "f32":
        ups = [op for op in st.programs["fwd"].array[:st.programs["fwd"].n] if op.kind == L.OP_UPSAMPLE2_FWD]
        assert len(ups) == 3 and all(op.u.up2.layout == L.LAYOUT_C8 and op.u.up2.type16 == m.compute for op in ups)      # C = 32 / 16 / 8 (64 / 32 / 16): channel-blocked
    ls = m.loss_scale
    with O.lowp_conv3x3(dtype, model=[ref, ref64], da16=False):
        t32 = O.train_step(ref, O.make_adam(ref, 1e-4), img, mask, label, B.ALPHA, True, n_classes, loss_scale=ls)
        t64 = O.train_step(ref64, O.make_adam(ref64, 1e-4), img.double(), mask.double(), label, B.ALPHA, True, n_classes, loss_scale=ls)
    assert losses[3].item() == 0.0
    rel = lambda a, b: ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()      # noqa: E731
    first = lambda t: t[0] if isinstance(t, list) else t      # noqa: E731
    assert abs(losses[0].item() - t64[0].item()) < max(3 * abs(t32[0].item() - t64[0].item()), 5e-4)
    assert rel(st.logits.data.view(2, -1), first(t64[3])) < max(3 * rel(first(t32[3]), first(t64[3])), 2e-3)
    for got, w32, w64 in zip(st.segs, t32[4] if ds else [t32[4]], t64[4] if ds else [t64[4]]):
        assert rel(got.data, w64) < max(3 * rel(w32, w64), 2e-3)
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad = []
    for name in m._order:
        if g64[name].grad.norm().item() == 0.0:
            continue
        e_hip, e_cpu = rel(m._grad_view(name) / ls, g64[name].grad), rel(g32[name].grad, g64[name].grad)
        if not e_hip < max(3 * e_cpu, 5e-2):
            bad.append((name, round(e_hip, 4), round(e_cpu, 4)))
    print(cfg, dtype, "bad", bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ end to end
def _store(M, seed):
    img, mask, label = O.synthetic_batch(M, 128, 128, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def test_test_phase_and_fold_loop_run_end_to_end(tmp_path):
    """FusedTestStep over 16 synthetic images, and fit_fold for two epochs (load_indexed batches, metrics=True, the on-device evaluation
    step, checkpoints): the drivers take the model as they take the other two."""
    cfg = "w8_c3_ds"
    m = _model(cfg, 13)
    images, masks, labels = _store(16, 33)
    ds = DD.DeviceDataset(images, masks, labels)
    opt = FusedAdam(m, lr=1e-3, eps=1e-4)
    step = _step(m, cfg, opt, metrics=True)
    eval_step = T.FusedEvalStep(m, alpha=B.ALPHA, on_device=True)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    rows = T.fit_fold(step, eval_step, ds, EpochIndex(np.arange(12), 4, seed=13), EpochIndex(np.arange(12, 16), 4, seed=13), scheduler,
                      str(tmp_path / "fold_0"), epochs=2, max_patience=5, transforms={"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0},
                      seed=13, plateau=False)
    assert len(rows) == 2 and [r[0] for r in rows] == [0, 1] and all(np.isfinite(np.asarray(r[1:], dtype=np.float64)).all() for r in rows)
    test = I.FusedTestStep(m)
    img, mask, label = O.synthetic_batch(16, 128, 128, seed=33)
    for i in range(0, 16, 4):
        test(img[i:i + 4].to(DEV), mask[i:i + 4].to(DEV), label[i:i + 4].to(DEV))
    seg_rows, cls_rows = test.result()
    assert len(seg_rows) == 16 and len(cls_rows) == 16 and all(0.0 <= r["DICE"] <= 1.0 for r in seg_rows)
    with pytest.raises(ValueError, match="128 x 128"):
        m(torch.zeros(1, 1, 64, 64, device=DEV))
