"""Single-task nnUNet segmentation (BASELINE.json configs[0]) on the GPU: the reference-pinned golden through the drop-in loop and through
the fused step, the model as a subgraph of MTnnUNet, graph replay, the dynamic loss scale, mtbc_seg_step_metrics, the refusals, and the
launch-coverage guard.  N = 2 at 64 x 64 throughout (the smallest plane this model takes)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet, nnUNet  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedEvalStep, FusedTrainStep, SegTrainMetrics, _dice  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import step_programs as SP  # noqa: E402

DEV = torch.device("cuda:0")
TOL = 1e-4          # tests/test_model_gpu.py


def _maxerr(a, b):
    return (a.detach().cpu().float() - b.detach().cpu().float()).abs().max().item()


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "seg_nnunet_step.npz"))


def _model(dtype="f32"):
    seed_everything(1993)
    m = nnUNet(1, 1).to(DEV)
    m.set_compute(dtype)
    return m


def _batch(n, size, seed):
    img, mask, label = O.synthetic_batch(n, size, size, seed=seed)
    return img.to(DEV), mask.to(DEV), label.to(DEV)


def _check_probes(model, g, what):
    params = dict(model.named_parameters())
    for i, k in enumerate(str(p) for p in g["probe_names"]):
        want = g[f"after_{i}"]
        got = params[k].detach().flatten()[:32].cpu().numpy()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        err = np.abs(got - want).max()
        print(f"{what}: {k} max |param - golden| {err:.3e}")
        assert err < 2e-5, (what, k, err)          # one Adam(lr 1e-4) step moves a weight <= 1e-4


# ------------------------------------------------------------------------------------------------ 1
def test_forward_matches_reference_golden(golden_dir):
    g = _golden(golden_dir)
    model = _model()
    model.train(True)
    with torch.no_grad():
        outs = model(torch.from_numpy(g["x"]).to(DEV))
    assert isinstance(outs, list) and len(outs) == 4                               # nnUNet.py:168
    assert all(tuple(o.shape) == (2, 1, 64, 64) for o in outs)
    err = _maxerr(outs[-1], torch.from_numpy(g["out1"]))
    means = [o.double().mean().item() for o in outs]
    print("out1 max err", err, "head means", means, "golden", g["out_means"].tolist())
    assert err < TOL
    for got, want in zip(means, g["out_means"]):
        assert abs(got - float(want)) < TOL


# ------------------------------------------------------------------------------------------------ 2
def _dropin_step(model, x, mask):
    """training_segmentation.py:40-57 verbatim on the drop-in surface."""
    optimizer = FusedAdam(model, lr=1e-4, eps=1e-4)
    criterion = CR.DiceLoss()
    optimizer.zero_grad(set_to_none=True)
    outputs = model(x)
    loss = CR.apply_criterion_binary_segmentation(criterion, mask, outputs, True)
    loss.backward()
    optimizer.step()
    return loss.item()


def test_reference_loop_verbatim_matches_golden_step(golden_dir):
    g = _golden(golden_dir)
    x, mask = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["mask"]).to(DEV)
    a = _model()
    loss_a = _dropin_step(a, x, mask)
    print("drop-in loss", loss_a, "golden", float(g["loss"]))
    assert abs(loss_a - float(g["loss"])) < TOL
    _check_probes(a, g, "drop-in")
    # the same step through FusedTrainStep
    b = _model()
    step = FusedTrainStep(b, FusedAdam(b, lr=1e-4, eps=1e-4), inversely_weighted=True)
    losses = step(x, mask).cpu()
    print("fused loss words", losses.tolist())
    assert abs(losses[0].item() - float(g["loss"])) < TOL
    assert losses[0].item() == losses[1].item() and losses[2].item() == 0.0 and losses[3].item() == 0.0      # [seg, seg, 0, nan_flag], exactly
    _check_probes(b, g, "fused")
    # the drop-in path and the fused path agree as test_dropin_autograd_path_equals_fused_path requires of the multi-task model
    assert abs(losses[0].item() - loss_a) < 1e-6
    for name in a._order:
        assert _maxerr(a._param_view(name), b._param_view(name)) < 1e-7, name


@pytest.mark.parametrize("name", ["BCE", "FocalDICE", "Jaccard"])
def test_other_seg_criteria_take_the_seg_only_plan(name):
    """All four `seg_criterion` kinds work unchanged: the loss words keep their [seg, seg, 0, nan] form and the step moves the weights."""
    m = _model()
    before = m.to(DEV).state_dict()["output1.weight"].clone()
    step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), seg_criterion=name)
    img, mask, _ = _batch(2, 64, 3)
    losses = step(img, mask).cpu()
    assert torch.isfinite(losses).all() and losses[0] == losses[1] and losses[2] == 0 and losses[3] == 0 and losses[0] > 0
    assert not torch.equal(m.state_dict()["output1.weight"], before)


# ------------------------------------------------------------------------------------------------ 3
def _grads_of_one_backward(model, step, batch):
    """pack -> fwd -> loss -> bwd of the fused step without the optimizer: (loss words, {name: gradient}, the heads' outputs)."""
    st = step.load_batch(*batch)
    for p in ("pack", "fwd", "loss"):
        st.programs[p].run()
    heads = [(h.name, h.data.clone()) for h in st.segs]        # before the backward, which reuses the outputs' memory
    st.programs["bwd"].run()
    torch.cuda.synchronize()
    return st.plan.loss_out.clone(), {n: model._grad_view(n).clone() for n in model._order}, heads


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_seg_only_step_is_the_subgraph_of_mtnnunet_bit_for_bit(dtype):
    """MTnnUNet with the same shared weights and alpha = 1.0 sends a zero gradient into its class logits; adding zeros is exact, so the
    segmentation loss word and the gradient of every shared parameter equal the segmentation-only step's bit for bit."""
    img, mask, label = _batch(2, 64, 21)
    seg = _model(dtype)
    seed_everything(1993)
    mt = MTnnUNet(1, 1, 3).to(DEV)
    mt.set_compute(dtype)
    seg.ensure_flat(), mt.ensure_flat()
    for n in seg._order:                        # same seed, same creation order: the trunk is drawn first in both
        assert torch.equal(seg._param_view(n), mt._param_view(n)), n
    ls, gs, heads_s = _grads_of_one_backward(seg, FusedTrainStep(seg, FusedAdam(seg, lr=1e-4, eps=1e-4)), (img, mask))
    lm, gm, heads_m = _grads_of_one_backward(mt, FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4), alpha=1.0), (img, mask, label))
    assert float(gm["classifier.5.weight"].abs().max()) == 0.0             # the zero class-logit gradient
    print(dtype, "loss words", ls.tolist(), lm.tolist())
    assert ls[1].item() == lm[1].item() and ls[0].item() == ls[1].item()
    for (name, got), (_, want) in zip(heads_s, heads_m):                   # (the forward first: a difference there names itself)
        assert torch.equal(got, want), f"{dtype}: forward head {name} differs by {(got - want).abs().max().item():.3e}"
    diff = [(n, (gs[n] - gm[n]).abs().max().item(), gm[n].abs().max().item()) for n in seg._order if not torch.equal(gs[n], gm[n])]
    for row in diff:
        print(dtype, "gradient differs:", row)
    assert not diff, f"{dtype}: {len(diff)} shared parameters' gradients differ, the last in backward order: {diff[0]}"


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype,opt_cls", [("f16", FusedAdam), ("f32", FusedSGD), ("bf16", FusedAdamW)])
def test_graph_replayed_steps_are_the_eager_steps(dtype, opt_cls):
    res = []
    for graph in (False, True):
        m = _model(dtype)
        opt = opt_cls(m, lr=1e-3) if opt_cls is not FusedAdam else FusedAdam(m, lr=1e-3, eps=1e-4)
        step = FusedTrainStep(m, opt, graph=graph, metrics=True)
        step.begin_epoch_metrics()
        losses = []
        for s in range(5):
            img, mask, _ = _batch(2, 64, 10 + s)
            losses.append(step(img, mask).clone())
        torch.cuda.synchronize()
        step.check_nan()
        if graph:
            assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
        res.append((m.flat_p.clone(), torch.stack(losses), step.epoch_metrics()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].batches == res[1][2].batches == 5 and np.array_equal(res[0][2].table, res[1][2].table)
    assert res[0][2].loss == res[1][2].loss and res[0][2].dice == res[1][2].dice


# ------------------------------------------------------------------------------------------------ 5
def test_dynamic_loss_scale_without_overflow_is_the_static_scale():
    res = []
    for scale in (None, DynamicLossScale(init_scale=65536.0, growth_interval=10 ** 6)):
        m = _model("f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        step = FusedTrainStep(m, opt, loss_scale=scale)
        losses = [step(*_batch(2, 64, 30 + s)[:2]).clone() for s in range(3)]
        torch.cuda.synchronize()
        step.check_nan()
        res.append((m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.stack(losses), step))
    for a, b, what in zip(res[0][:4], res[1][:4], ("parameters", "exp_avg", "exp_avg_sq", "losses")):
        assert torch.equal(a, b), f"dynamic against static: {what} differ, max |diff| {(a - b).abs().max().item():.3e}"
    assert res[1][4].scaler.stats() == {"scale": 65536.0, "growth_tracker": 3, "skipped": 0, "t": 3}


# ------------------------------------------------------------------------------------------------ 6
def _restate_row(seg_logits, mask):
    s, g = torch.sigmoid(seg_logits.float()) > 0.5, mask != 0
    return [int((s & g).sum()), int((s & ~g).sum()), int((~s & g).sum()), int(seg_logits.shape[0])]


def _call_seg_step_metrics(x, t, counts, state, capacity, loss_in=None, loss_rows=None, weight=None, empty=False):
    a = L.SegStepMetricsArgs()
    if not empty:
        a.seg_logits, a.mask, a.n_seg, a.N = x.data_ptr(), t.data_ptr(), x.numel(), x.shape[0]
    a.table, a.state, a.capacity = counts.data_ptr(), state.data_ptr(), capacity
    a.loss_in = loss_in.data_ptr() if loss_in is not None else None
    a.loss_rows = loss_rows.data_ptr() if loss_rows is not None else None
    a.shard_weight = weight.data_ptr() if weight is not None else None
    return L.load().mtbc_seg_step_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_seg_step_metrics_rows_cursor_capacity_and_empty_shard():
    g = torch.Generator().manual_seed(5)
    cap = 3
    counts = torch.zeros(cap * 4, dtype=torch.int64, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    rows = torch.zeros(cap, 4, dtype=torch.float64, device=DEV)
    want_rows, want_loss = [], []
    shapes = [(2, 1, 64, 64), (3, 1, 16, 23)]                       # the second: an element count that is no multiple of 4 (the scalar tail)
    for i, shape in enumerate(shapes):
        x = torch.randn(shape, generator=g).to(DEV)
        t = (torch.rand(shape, generator=g) > 0.6).float().to(DEV)
        loss = torch.tensor([0.3 + i, 0.3 + i, 0.0, 0.0], dtype=torch.float32, device=DEV) / 3
        w = torch.tensor([0.75], dtype=torch.float32, device=DEV) if i else None
        assert _call_seg_step_metrics(x, t, counts, state, cap, loss, rows, w) == 0
        want_rows.append(_restate_row(x, t))
        want_loss.append([(0.75 if i else 1.0) * float(v) for v in loss.double().cpu()])
    assert _call_seg_step_metrics(None, None, counts, state, cap, empty=True) == 0           # the empty shard: the cursor only
    assert state.cpu().tolist() == [3, 0]
    x = torch.randn(shapes[0], generator=g).to(DEV)
    t = torch.ones(shapes[0], device=DEV)
    assert _call_seg_step_metrics(x, t, counts, state, cap, None, None) == 0                 # cursor == capacity: dropped and counted
    assert state.cpu().tolist() == [4, 1]
    assert counts.view(cap, 4).cpu().tolist() == want_rows + [[0, 0, 0, 0]]
    assert rows.cpu().tolist() == want_loss + [[0.0] * 4]
    # the training call: loss_in NULL leaves loss_rows alone
    state.zero_(), counts.zero_()
    assert _call_seg_step_metrics(x, t, counts, state, cap, None, None) == 0
    assert counts.view(cap, 4)[0].cpu().tolist() == _restate_row(x, t) and state.cpu().tolist() == [1, 0]
    # refusals
    assert _call_seg_step_metrics(x, t, counts, state, cap, torch.zeros(4, device=DEV), None) == -2          # loss_in without loss_rows
    a = L.SegStepMetricsArgs()
    a.table, a.state, a.capacity, a.N, a.n_seg = counts.data_ptr(), state.data_ptr(), cap, 0, 16
    assert L.load().mtbc_seg_step_metrics(C.byref(a), None) == -1                                            # N == 0 without n_seg == 0


def test_step_metrics_equal_a_restatement_and_the_default_eval_path():
    m = _model()
    batches = [_batch(2, 64, 40 + s)[:2] for s in range(3)]
    default, device, graphed = FusedEvalStep(m), FusedEvalStep(m, on_device=True), FusedEvalStep(m, on_device=True, graph=True, capacity=8)
    want_rows, want_loss = [], []
    for img, mask in batches:
        default(img, mask)
        device(img, mask)
        st = device._compiled(2, 64, 64)
        want_rows.append(_restate_row(st.segs[-1].data, st.mask))          # the step's own outputs (no backward has reused them)
        want_loss.append(st.plan.loss_out.double().cpu().tolist())
    for _ in range(2):                                                      # replay is reached at the third call of a compiled step
        graphed.reset()
        for img, mask in batches:
            graphed(img, mask)
    r_default, r_device, r_graph = default.result(), device.result(), graphed.result()
    print("eval results", r_default, r_device, r_graph)
    assert len(r_default) == 2 and r_default == r_device == r_graph                       # (val_loss, val_dice), training_segmentation.py:88
    assert device._em[:12].view(3, 4).cpu().tolist() == want_rows
    assert device._em_loss[:3].cpu().tolist() == want_loss
    assert all(w[0] == w[1] and w[2] == 0.0 and w[3] == 0.0 for w in want_loss)
    assert r_device[1] == sum(_dice(*map(float, r[:3])) for r in want_rows) / 3
    # the training step appends the same rows for the same weights: lr = 0 keeps them (SGD: p -= 0 * g)
    step = FusedTrainStep(m, FusedSGD(m, lr=0.0), metrics=True, metrics_capacity=8)
    step.begin_epoch_metrics()
    losses = [step(img, mask)[0].item() for img, mask in batches]
    em = step.epoch_metrics()
    assert isinstance(em, SegTrainMetrics) and em.batches == 3 and em.table.tolist() == want_rows
    assert em[1] == r_device[1] and em[0] == sum(float(np.float32(v)) for v in losses) / 3 == r_device[0]
    # capacity: a fourth batch into a three-row table is dropped and counted, and result() refuses
    small = FusedEvalStep(m, on_device=True, capacity=2)
    for img, mask in batches:
        small(img, mask)
    assert small._em_state.cpu().tolist() == [3, 1]
    with pytest.raises(L.MtbcError):
        small.result()


# ------------------------------------------------------------------------------------------------ 7
def test_refusals():
    m = _model()
    opt = FusedAdam(m, lr=1e-4, eps=1e-4)
    for kw in ({"alpha": 0.5}, {"n_classes": 3}, {"cls_criterion": "CE"}, {"focal_weight": torch.ones(3, device=DEV)}):
        with pytest.raises(ValueError):
            FusedTrainStep(m, opt, **kw)
        with pytest.raises(ValueError):
            FusedEvalStep(m, **kw)
    with pytest.raises(NotImplementedError):
        FusedTrainStep(m, opt, distributed=True)
    with pytest.raises(NotImplementedError):
        FusedEvalStep(m, on_device=True, distributed=True)
    FusedTrainStep(m, opt, alpha=1.0)                                      # alpha = 1 is what the step does anyway
    img, mask, label = _batch(2, 64, 1)
    with pytest.raises(ValueError):
        FusedTrainStep(m, opt)(img, mask, label)                           # a class label for a model without a classifier
    with pytest.raises(ValueError):
        FusedEvalStep(m)(img, mask, label)
    mt = MTnnUNet(1, 1, 3).to(DEV)
    with pytest.raises(TypeError):
        FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4))               # alpha stays required for a multi-task model
    with pytest.raises(ValueError):
        FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4), alpha=0.5)(img, mask)       # ... and so does its label


# ------------------------------------------------------------------------------------------------ 8
def _make_model(arch):
    from multi_task_breast_cancer_amd.experiment_init import init_segmentation_model
    return init_segmentation_model(arch, sequences=1, regions=1)


def _surveys():
    """(the MTnnUNet survey, the segmentation-only survey) of the benchmark shape (BASELINE.json configs[2]: bf16, N 64, 256 x 256), each built
    (not run) once per session by tests/step_programs.py."""
    program = next(p for p in SP.STEP_PROGRAMS if p[0] == "MTnnUNet")
    return SP.survey(program), SP.survey(("nnUNet",) + program[1:], build=SP.step_builder(_make_model, inversely_weighted=True))


def test_seg_only_programs_launch_a_subset_of_the_mtnnunet_programs():
    """The set of kernel instances the segmentation-only step programs launch at the benchmark shape is a subset of what the MTnnUNet programs
    launch.  (What the ARGUMENTS select inside an instance -- upsample4 stores dx where MTnnUNet, whose decoder5 output has a second reader,
    accumulates it -- is not an instance; those branches are held to the reference cases, key by key, by the test below.)  This guard is why
    nets._graph_nnunet_parts keeps up5's gradient fp32: as 16-bit planes it selected convT2_dgrad_kernel<1, true, 4>, which no benchmark
    program launches."""
    mt, seg = _surveys()
    for name in ("pack", "fwd", "loss", "bwd"):
        assert 0 < len(seg.kinds[name]) <= len(mt.kinds[name]), name
    have, allowed = SP.kernel_instances(seg), SP.kernel_instances(mt)
    print(len(have), "kernel instances of", len(allowed))
    assert len(have) >= 30, sorted(have)                       # the names did parse into instances
    assert have <= allowed, f"kernel instances of the segmentation-only programs that the MTnnUNet programs do not launch: {sorted(have - allowed)}"
    SP.assert_keys_subset(seg, mt, [f for f in SP.COLLECTORS if f not in SP.NAMED])          # the layout ops have no kernel-name function: their keys, as they are


def test_seg_only_programs_launch_only_reference_tested_instances():
    """No untested launch enters: every coverage key of the segmentation-only step programs at the benchmark shape -- kernel instances AND
    the branches the arguments select, as tests/step_programs.py keys them -- is the key of a call that an element-wise reference test of
    tests/test_ops_gpu.py makes, the sets its own guards hold the MTnnUNet and U-Net++ programs to."""
    SP.assert_only_tested(_surveys()[1], SP.reference_tested_keys(), SP.table_keys())
