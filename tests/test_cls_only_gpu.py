"""Single-task classification (`nnUNetClassifier`, `UNetPlusPlusClassifier`) on the GPU: the reference-pinned fixture through the drop-in loop and
the fused step, the models as subgraphs of the multi-task ones, the softmax op, the loss on probabilities, the never-trained parameters under the
three fused optimizers, graph replay, the dynamic loss scale, mtbc_cls_step_metrics, the testing phase, the refusals and the launch-coverage
guard.  N = 2 or 3 at 64 x 64 (the smallest plane the nnUNet trunk takes) unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd import inference as INF  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet, MTUNetPlusPlus, UNetPlusPlusClassifier, nnUNetClassifier  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from multi_task_breast_cancer_amd.trainer import ClsTrainMetrics, FusedEvalStep, FusedTrainStep  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import step_programs as SP  # noqa: E402
from test_cls_only_cpu import softmax_cases, softmax_references, within  # noqa: E402

DEV = torch.device("cuda:0")
TOL = 1e-4          # tests/test_model_gpu.py: the project's pinned fp32 bound
GRAD_TOL = 2e-5     # tests/test_seg_nnunet_gpu.py: the bound of its golden step
OPT_TOL = 2.5e-4    # tests/test_fused_optim_gpu.py: a further step from an interchanged optimizer state
GRADS = ("classifier.5.weight", "classifier.5.bias", "encoder1.ConvInNormLRelu1.Conv.weight")


def _maxerr(a, b):
    return (a.detach().cpu().float() - b.detach().cpu().float()).abs().max().item()


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_nnunet_step.npz"))


def _model(n_classes=3, dtype="f32", arch=nnUNetClassifier):
    seed_everything(1993)
    m = (arch(1, n_classes) if arch is nnUNetClassifier else arch(2, 1, n_classes)).to(DEV)
    m.set_compute(dtype)
    return m


def _batch(n, seed, binary=False, size=64):
    img, _, label = O.synthetic_batch(n, size, size, seed=seed)
    return img.to(DEV), ((label > 0).float() if binary else label).to(DEV)


def _onehot(label):
    return torch.nn.functional.one_hot(label.flatten().to(torch.int64), num_classes=3).to(torch.float)


def _untouched(model, initial):
    return all(torch.equal(model._param_view(n), initial[n]) for n in model.untrained)


# ------------------------------------------------------------------------------------------------ 1
def test_forward_and_verbatim_driver_step_match_the_fixture(golden_dir):
    g = _golden(golden_dir)
    x, label = torch.from_numpy(g["image"]).to(DEV), torch.from_numpy(g["label"]).to(DEV)
    a = _model()
    a.train(True)
    with torch.no_grad():
        out = a(x)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 3)                 # nnUNet_classifier.py:171: ONE tensor
    print("probabilities max err", _maxerr(out, torch.from_numpy(g["out_3"])))
    assert _maxerr(out, torch.from_numpy(g["out_3"])) < TOL
    initial = {n: a._param_view(n).clone() for n in a._order}
    # training_classification.py:41-58 verbatim on the drop-in surface
    optimizer = FusedAdam(a, lr=1e-4, eps=1e-4)
    classification_criterion = CR.FocalLoss(alpha=1, gamma=2, reduction="mean")
    onehot = _onehot(label)
    optimizer.zero_grad(set_to_none=True)
    pred_class = a(x)
    classification_loss = CR.apply_criterion_classification(classification_criterion, onehot, pred_class, True)
    classification_loss.backward()
    params = dict(a.named_parameters())
    assert sorted(n for n, p in params.items() if p.grad is None) == sorted(str(n) for n in g["grad_none"])
    for name in GRADS:                  # against the same gradients in float64 (against the float32 ones: the test below)
        err = (params[name].grad.cpu().double() - torch.from_numpy(g["grad64_" + name])).abs().max().item()
        print("drop-in gradient against float64", name, err)
        assert err < GRAD_TOL, (name, err)
    optimizer.step()
    print("drop-in loss", classification_loss.item(), "fixture", float(g["step_loss"]))
    assert abs(classification_loss.item() - float(g["step_loss"])) < TOL
    assert _untouched(a, initial) and not torch.equal(a._param_view(GRADS[0]), initial[GRADS[0]])
    assert all(i not in optimizer.state_dict()["state"] for i, n in enumerate(a._order) if n in a.untrained)
    # the same step through FusedTrainStep
    b = _model()
    step = FusedTrainStep(b, FusedAdam(b, lr=1e-4, eps=1e-4), n_classes=3, cls_criterion="Focal")
    st = step.load_batch(x, label)
    for p in ("pack", "fwd", "loss", "bwd"):
        st.programs[p].run()
    for name in GRADS:
        err = (b._grad_view(name).cpu().double() - torch.from_numpy(g["grad64_" + name])).abs().max().item()
        print("fused gradient against float64", name, err)
        assert err < GRAD_TOL, (name, err)
        assert torch.equal(b._grad_view(name), params[name].grad), name          # one backward program behind both surfaces
    losses = step(x, label).cpu()
    print("fused loss words", losses.tolist())
    assert abs(losses[0].item() - float(g["step_loss"])) < TOL
    assert losses[0].item() == losses[2].item() and losses[1].item() == 0.0 and losses[3].item() == 0.0       # [cls, 0, cls, nan_flag], exactly
    assert _untouched(b, initial) and all(p.grad is None for n, p in b.named_parameters() if n in b.untrained)
    for name in a._order:
        assert _maxerr(a._param_view(name), b._param_view(name)) < 1e-7, name
    # the other criteria of the fixture through the evaluation step: CE on the probabilities, BCE on the binary head's logit
    c = _model()
    for crit, key in (("Focal", "loss_focal"), ("CE", "loss_ce")):
        ev = FusedEvalStep(c, n_classes=3, cls_criterion=crit)
        ev(x, label)
        got = ev.result()
        print(crit, got, float(g[key]))
        assert len(got) == 3 and abs(got[0] - float(g[key])) < TOL
    d = _model(2)
    with torch.no_grad():
        logit = d(x)
    assert tuple(logit.shape) == (2, 1) and _maxerr(logit, torch.from_numpy(g["out_2"])) < TOL
    ev = FusedEvalStep(d, n_classes=2)
    ev(x, (label > 0).float())
    assert abs(ev.result()[0] - float(g["loss_bce"])) < TOL


@pytest.mark.parametrize("name", GRADS)
def test_step_gradients_against_the_fixtures_float32_gradients(golden_dir, name):
    """The gradients of the verbatim driver step against the reference's own float32 gradients (torch on the CPU), within 2e-5, the bound
    tests/test_seg_nnunet_gpu.py uses for its golden step.

    Measured on an MI355X, max |difference| (against the fixture's float32 gradient / against its float64 gradient / the fixture's float32
    against its own float64):
        classifier.5.weight                       1.93e-07 / 2.09e-07 / 8.44e-08
        classifier.5.bias                         7.45e-09 / 1.42e-08 / 6.71e-09
        encoder1.ConvInNormLRelu1.Conv.weight     1.17e-06 / 1.22e-06 / 4.73e-07      (|g| up to 1.9e-2)
    The fixture's batch is chosen by the reference's own error (tools/make_cls_fixture.py): with 2 x 2 planes in the bottleneck's InstanceNorm,
    float32 torch's first-layer gradient is between 2e-7 and 5e-4 from the float64 one depending on the draw, and a stored gradient further
    from the truth than this bound would measure torch's rounding, not these kernels."""
    g = _golden(golden_dir)
    x, label = torch.from_numpy(g["image"]).to(DEV), torch.from_numpy(g["label"]).to(DEV)
    m = _model()
    step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), n_classes=3, cls_criterion="Focal")
    st = step.load_batch(x, label)
    for p in ("pack", "fwd", "loss", "bwd"):
        st.programs[p].run()
    got = m._grad_view(name).cpu()
    e32, e64 = _maxerr(got, torch.from_numpy(g["grad_" + name])), (got.double() - torch.from_numpy(g["grad64_" + name])).abs().max().item()
    ref = (torch.from_numpy(g["grad_" + name]).double() - torch.from_numpy(g["grad64_" + name])).abs().max().item()
    print(f"{name}: against the fixture's float32 gradient {e32:.3e}, against its float64 gradient {e64:.3e}; the fixture's float32 against its float64 {ref:.3e}")
    assert e32 < GRAD_TOL, (name, e32)


# ------------------------------------------------------------------------------------------------ 2
def _one_backward(model, step, batch):
    st = step.load_batch(*batch)
    for p in ("pack", "fwd", "loss"):
        st.programs[p].run()
    logits = (st.plan.acts["logits"] if "logits" in st.plan.acts else st.logits).data.clone()
    st.programs["bwd"].run()
    torch.cuda.synchronize()
    return logits, st.plan.loss_out.clone(), {n: model._grad_view(n).clone() for n in model._order if n not in model.untrained}


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("arch,n_classes", [("nnunet", 3), ("nnunet", 2), ("unetpp", 3)])
def test_cls_only_step_is_the_subgraph_of_the_multitask_step(arch, n_classes, dtype):
    """The multi-task model's weights copied into the classifier.  Class logits: bit-equal in every mode (for the 3-class nnUNetClassifier the
    logits in front of its softmax).  Gradients, against the multi-task step with alpha = 0 (whose segmentation heads send zeros back; adding
    zeros is exact): compared for the models whose criterion reads the same logits -- the binary nnUNetClassifier and the UNetPlusPlusClassifier
    (the 3-class nnUNetClassifier's criterion reads probabilities: another function).  Every shared parameter's gradient is required to be
    bit-equal -- the tensors whose gradient the two programs gather from different readers included (decoder5's output: one reader here, two
    there; x_3_1, x_3_0, x_2_0: their decoder-side readers carry zeros there) -- so no tensor falls back to the fp64 comparison."""
    seed_everything(1993)
    if arch == "nnunet":
        mt, cl = MTnnUNet(1, 1, n_classes).to(DEV), nnUNetClassifier(1, n_classes).to(DEV)
    else:
        mt, cl = MTUNetPlusPlus(2, 1, 1, n_classes).to(DEV), UNetPlusPlusClassifier(2, 1, n_classes).to(DEV)
    mt.set_compute(dtype), cl.set_compute(dtype)
    mt.ensure_flat(), cl.ensure_flat()
    for n in cl._order:
        cl._param_view(n).copy_(mt._param_view(n))
    img, label = _batch(2, 21, binary=n_classes == 2)
    mask = torch.zeros(2, 1, 64, 64, device=DEV)
    lm, wm, gm = _one_backward(mt, FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4), alpha=0.0, n_classes=n_classes), (img, mask, label))
    lc, wc, gc = _one_backward(cl, FusedTrainStep(cl, FusedAdam(cl, lr=1e-4, eps=1e-4), n_classes=n_classes), (img, label))
    assert torch.equal(lc, lm), f"{dtype}: class logits differ by {(lc - lm).abs().max().item():.3e}"
    if arch == "nnunet" and n_classes == 3:
        return
    assert wc[2].item() == wm[2].item() == wc[0].item() and wc[1].item() == 0.0
    diff = [(n, (gc[n] - gm[n]).abs().max().item(), gm[n].abs().max().item()) for n in gc if not torch.equal(gc[n], gm[n])]
    for row in diff:
        print(dtype, "gradient differs:", row)
    assert gc and not diff, f"{dtype}: {len(diff)} of {len(gc)} shared parameters' gradients differ, e.g. {diff[0]}"


# ------------------------------------------------------------------------------------------------ 3
def test_softmax_op_on_the_device_is_the_host_function_bit_for_bit():
    for x, dp in softmax_cases():
        p_host, dz_host = ops.softmax_rows_host(x, dp)
        p = ops.softmax_rows(x.to(DEV))
        dz = ops.softmax_rows_bwd(p, dp.to(DEV))
        assert torch.equal(p.cpu().view(torch.int32), p_host.view(torch.int32)), (x, p.cpu(), p_host)
        assert torch.equal(dz.cpu().view(torch.int32), dz_host.view(torch.int32)), (x, dz.cpu(), dz_host)
    a = ops.softmax_args(2, 4, False, x=1 << 20, p=2 << 20)
    assert L.load().mtbc_softmax_rows(C.byref(a), None) == -1                            # C outside 1 .. 3
    a = ops.softmax_args(2, 3, True, p=1 << 20)
    assert L.load().mtbc_softmax_rows(C.byref(a), None) == -2                            # the backward without dp / dz


# ------------------------------------------------------------------------------------------------ 4
def _criterion64(z, onehot, gamma, weight, dtype):
    """criterion(softmax(z), onehot) restated in torch: FocalLoss (criterions.py:14-24; gamma 0 = CrossEntropyLoss without weights) ON PROBABILITIES."""
    z = z.to(dtype).clone().requires_grad_(True)
    p = torch.softmax(z, dim=1)
    ce = torch.nn.functional.cross_entropy(p, onehot.to(dtype), reduction="none", weight=None if weight is None else weight.to(dtype))
    loss = torch.mean((1 - torch.exp(-ce)) ** gamma * ce) if gamma else torch.mean(ce)
    loss.backward()
    return loss.detach(), z.grad


@pytest.mark.parametrize("crit,weighted", [("Focal", False), ("CE", False), ("Focal", True)])
def test_fused_loss_on_probabilities(crit, weighted):
    """The fused 3-class nnUNetClassifier loss and d loss / d logits against float64 torch.  Bound: 8 x the error float32 torch shows on the same
    logits against float64 (floor 1 float32 ulp of the value).  Measured on an MI355X, error of the loss / of the gradient, float32 torch
    then the fused step: Focal 1.72e-08 / 6.21e-09 then 1.72e-08 / 8.69e-09; CE 9.87e-08 / 5.52e-09 then 2.05e-08 / 4.44e-09; Focal with class
    weights 2.26e-09 / 7.14e-10 then 1.34e-08 / 3.01e-09."""
    m = _model()
    w = torch.tensor([0.2, 0.5, 0.3], device=DEV) if weighted else None
    step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), n_classes=3, cls_criterion=crit, focal_weight=w)
    img, label = _batch(3, 17)
    st = step.load_batch(img, label)
    for p in ("pack", "fwd", "loss"):
        st.programs[p].run()
    z = st.plan.acts["logits"].data.view(3, 3).clone()
    st.programs["bwd"].run()          # only its first op matters here: the softmax backward into the logits' gradient
    torch.cuda.synchronize()
    dz = st.plan.acts["logits"].grad.view(3, 3).cpu()
    loss = st.plan.loss_out[0].cpu()
    gamma = 2.0 if crit == "Focal" else 0.0
    onehot, wc = _onehot(label).cpu(), None if w is None else w.cpu()
    l64, g64 = _criterion64(z.cpu(), onehot, gamma, wc, torch.float64)
    l32, g32 = _criterion64(z.cpu(), onehot, gamma, wc, torch.float32)
    e_loss, e_grad = abs(l32.double() - l64).item(), (g32.double() - g64).abs().max().item()
    print(f"{crit} weighted={weighted}: torch float32 error loss {e_loss:.3e} grad {e_grad:.3e}; fused error loss {abs(loss.double() - l64).item():.3e} "
          f"grad {(dz.double() - g64).abs().max().item():.3e}")
    assert within(loss.view(1), l64.view(1), e_loss)
    assert within(dz, g64, e_grad)


# ------------------------------------------------------------------------------------------------ 5
def _torch_opt(kind, params, lr):
    if kind is FusedAdam:
        return torch.optim.Adam(params, lr=lr, eps=1e-4)
    if kind is FusedSGD:
        return torch.optim.SGD(params, lr=lr, momentum=0.9, nesterov=True)
    return torch.optim.AdamW(params, lr=lr)


@pytest.mark.parametrize("kind", [FusedAdam, FusedSGD, FusedAdamW])
def test_never_trained_parameters_stay_bit_equal_and_stateless(kind):
    lr = 1e-3
    a = _model()
    a.ensure_flat()
    initial = {n: a._param_view(n).clone() for n in a._order}
    opt = FusedAdam(a, lr=lr, eps=1e-4) if kind is FusedAdam else kind(a, lr=lr)
    step = FusedTrainStep(a, opt, n_classes=3)
    for s in range(3):
        step(*_batch(2, 50 + s))
    step.check_nan()
    assert _untouched(a, initial)
    assert not torch.equal(a._param_view("decoder5.ConvInNormLRelu1.Conv.weight"), initial["decoder5.ConvInNormLRelu1.Conv.weight"])
    sd = opt.state_dict()
    dead = {i for i, n in enumerate(a._order) if n in a.untrained}
    assert len(dead) == 8 and set(sd["state"]) == set(range(len(a._order))) - dead
    # the state loads into the torch optimizer built on a copy of the model; one further step of each agrees
    b = _model()
    b.load_state_dict(a.state_dict())
    topt = _torch_opt(kind, b.parameters(), lr)
    topt.load_state_dict(sd)
    img, label = _batch(2, 60)
    step(img, label)
    criterion = CR.FocalLoss(alpha=1, gamma=2, reduction="mean")
    topt.zero_grad(set_to_none=True)
    loss = CR.apply_criterion_classification(criterion, _onehot(label), b(img), True)
    loss.backward()
    assert all((p.grad is None) == (n in b.untrained) for n, p in b.named_parameters())
    topt.step()
    worst = max(_maxerr(a._param_view(n), b._param_view(n)) for n in a._order)
    print(kind.__name__, "one further step, fused against torch's optimizer: max |dparam|", worst)
    assert worst < OPT_TOL
    assert _untouched(a, initial) and _untouched(b, initial)
    # ... and the reverse: torch's state into a fresh fused optimizer
    fresh = FusedAdam(b, lr=lr, eps=1e-4) if kind is FusedAdam else kind(b, lr=lr)
    fresh.load_state_dict(topt.state_dict())
    assert set(fresh.state_dict()["state"]) == set(topt.state_dict()["state"]) == set(range(len(a._order))) - dead


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replayed_steps_are_the_eager_steps(dtype):
    res = []
    for graph in (False, True):
        m = _model(3, dtype)
        step = FusedTrainStep(m, FusedAdam(m, lr=1e-3, eps=1e-4), n_classes=3, graph=graph, metrics=True)
        step.begin_epoch_metrics()
        losses = [step(*_batch(2, 10 + s)).clone() for s in range(5)]
        torch.cuda.synchronize()
        step.check_nan()
        if graph:
            assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
        res.append((m.flat_p.clone(), torch.stack(losses), step.epoch_metrics()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert res[0][2].batches == res[1][2].batches == 5 and np.array_equal(res[0][2].conf, res[1][2].conf) and res[0][2][:3] == res[1][2][:3]


def test_dynamic_loss_scale_without_overflow_is_the_static_scale():
    res = []
    for scale in (None, DynamicLossScale(init_scale=65536.0, growth_interval=10 ** 6)):
        m = _model(3, "f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        step = FusedTrainStep(m, opt, n_classes=3, loss_scale=scale)
        losses = [step(*_batch(2, 30 + s)).clone() for s in range(3)]
        torch.cuda.synchronize()
        step.check_nan()
        res.append((m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), torch.stack(losses), step))
    for a, b, what in zip(res[0][:4], res[1][:4], ("parameters", "exp_avg", "exp_avg_sq", "losses")):
        assert torch.equal(a, b), f"dynamic against static: {what} differ, max |diff| {(a - b).abs().max().item():.3e}"
    assert res[1][4].scaler.stats() == {"scale": 65536.0, "growth_tracker": 3, "skipped": 0, "t": 3}


# ------------------------------------------------------------------------------------------------ 7
def _restate_conf(out, target):
    conf = np.zeros((3, 3), dtype=np.int64)
    if out.shape[1] == 1:
        pred, gt = (torch.sigmoid(out[:, 0]) > 0.5).long(), (target[:, 0] != 0).long()
    else:
        pred, gt = out.argmax(dim=1), target.argmax(dim=1)
    for g_, p_ in zip(gt.tolist(), pred.tolist()):
        conf[g_, p_] += 1
    return conf


def _call_cls_step_metrics(out, target, counts, state, capacity, n_logits=3, loss_in=None, loss_rows=None, weight=None):
    a = L.ClsStepMetricsArgs()
    a.n_logits = n_logits
    if out is not None:
        a.cls_out, a.target, a.N, a.n_logits = out.data_ptr(), target.data_ptr(), out.shape[0], out.shape[1]
    a.table, a.conf, a.state, a.capacity = counts.data_ptr(), counts.data_ptr() + capacity * 32, state.data_ptr(), capacity
    a.loss_in = loss_in.data_ptr() if loss_in is not None else None
    a.loss_rows = loss_rows.data_ptr() if loss_rows is not None else None
    a.shard_weight = weight.data_ptr() if weight is not None else None
    return L.load().mtbc_cls_step_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_cls_step_metrics_rows_cursor_capacity_and_empty_shard():
    g = torch.Generator().manual_seed(5)
    cap = 3
    counts = torch.zeros(cap * 4 + 9, dtype=torch.int64, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    rows = torch.zeros(cap, 4, dtype=torch.float64, device=DEV)
    want_conf, want_rows, want_loss = np.zeros((3, 3), dtype=np.int64), [], []
    for i, n in enumerate((7, 300)):                               # the second: more samples than the block has threads
        out = torch.softmax(torch.randn(n, 3, generator=g), dim=1)
        out[0] = 1.0 / 3                                           # equal maxima: the first wins
        target = torch.nn.functional.one_hot(torch.randint(0, 3, (n,), generator=g), 3).float()
        loss = torch.tensor([0.3 + i, 0.0, 0.3 + i, 0.0], dtype=torch.float32, device=DEV) / 3
        w = torch.tensor([0.75], dtype=torch.float32, device=DEV) if i else None
        assert _call_cls_step_metrics(out.to(DEV), target.to(DEV), counts, state, cap, loss_in=loss, loss_rows=rows, weight=w) == 0
        want_conf += _restate_conf(out, target)
        want_rows.append([0, 0, 0, n])
        want_loss.append([(0.75 if i else 1.0) * float(v) for v in loss.double().cpu()])
    assert _call_cls_step_metrics(None, None, counts, state, cap) == 0                        # the empty shard: the cursor only
    assert state.cpu().tolist() == [3, 0]
    out, target = torch.rand(4, 3).to(DEV), torch.eye(3)[[0, 1, 2, 0]].to(DEV)
    assert _call_cls_step_metrics(out, target, counts, state, cap) == 0                       # cursor == capacity: dropped and counted
    assert state.cpu().tolist() == [4, 1]
    assert counts[:cap * 4].view(cap, 4).cpu().tolist() == want_rows + [[0, 0, 0, 0]]
    assert np.array_equal(counts[cap * 4:].view(3, 3).cpu().numpy(), want_conf)
    assert rows.cpu().tolist() == want_loss + [[0.0] * 4]
    # the training call (loss_in NULL) with the binary head
    state.zero_(), counts.zero_()
    out, target = torch.randn(9, 1, generator=g), (torch.rand(9, 1, generator=g) > 0.5).float()
    assert _call_cls_step_metrics(out.to(DEV), target.to(DEV), counts, state, cap) == 0
    assert counts[:4].cpu().tolist() == [0, 0, 0, 9] and state.cpu().tolist() == [1, 0]
    assert np.array_equal(counts[cap * 4:].view(3, 3).cpu().numpy(), _restate_conf(out, target))
    # refusals
    assert _call_cls_step_metrics(out.to(DEV), target.to(DEV), counts, state, cap, loss_in=torch.zeros(4, device=DEV)) == -2      # loss_in without loss_rows
    assert _call_cls_step_metrics(None, None, counts, state, cap, n_logits=4) == -1


@pytest.mark.parametrize("n_classes", [3, 2])
def test_step_metrics_equal_a_restatement_and_the_drivers_tuple(n_classes):
    from sklearn.metrics import accuracy_score, f1_score
    binary = n_classes == 2
    m = _model(n_classes)
    batches = [_batch(3 if s == 1 else 2, 40 + s, binary) for s in range(3)]
    default, device = FusedEvalStep(m, n_classes=n_classes), FusedEvalStep(m, n_classes=n_classes, on_device=True)
    graphed = FusedEvalStep(m, n_classes=n_classes, on_device=True, graph=True, capacity=8)
    conf, want_loss, gts, preds = np.zeros((3, 3), dtype=np.int64), [], [], []
    for img, label in batches:
        default(img, label)
        device(img, label)
        st = device._compiled(img.shape[0], 64, 64)
        out, target = st.logits.data.view(st.N, -1).cpu(), st.onehot.cpu()          # the step's own outputs
        conf += _restate_conf(out, target)
        want_loss.append(st.plan.loss_out.double().cpu().tolist())
        if binary:                                                                   # training_classification.py:136-144
            preds += [(torch.sigmoid(out[i, :]) > .5).double().item() for i in range(out.shape[0])]
            gts += [target[i, :].item() for i in range(out.shape[0])]
        else:                                                                        # :126-132
            preds += [pl.argmax().item() for pl in out]
            gts += [l.argmax().item() for l in target]
    for _ in range(2):
        graphed.reset()
        for img, label in batches:
            graphed(img, label)
    r_default, r_device, r_graph = default.result(), device.result(), graphed.result()
    print("eval results", r_default, r_device, r_graph)
    assert len(r_device) == 3 and r_device == r_graph
    assert np.array_equal(device._em[-9:].view(3, 3).cpu().numpy(), conf) and device._em[:12].view(3, 4).cpu().tolist() == [[0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 2]]
    assert device._em_loss[:3].cpu().tolist() == want_loss and all(w[0] == w[2] and w[1] == 0.0 and w[3] == 0.0 for w in want_loss)
    if binary:
        gt_t, pr_t = torch.Tensor(gts), torch.Tensor(preds)
        tp, tn = torch.sum(torch.logical_and(pr_t, gt_t)).double(), torch.sum(torch.logical_and(torch.logical_not(pr_t), torch.logical_not(gt_t))).double()
        fp, fn = torch.sum(torch.logical_and(pr_t, torch.logical_not(gt_t))).double(), torch.sum(torch.logical_and(torch.logical_not(pr_t), gt_t)).double()
        want_acc, want_f1 = ((tp + tn) / (tp + tn + fp + fn)).item(), ((2 * tp) / (2 * tp + fp + fn)).item()
    else:
        want_acc, want_f1 = accuracy_score(gts, preds), f1_score(y_true=gts, y_pred=preds, labels=[0, 1, 2], average="micro")
    want = (sum(w[0] for w in want_loss) / 3, want_acc, want_f1)
    for got in (r_default, r_device):
        assert all(abs(a - b) <= 1e-12 or (a != a and b != b) for a, b in zip(got, want)), (got, want)
    # the training step appends the same matrix for the same weights: lr = 0 keeps them (SGD: p -= 0 * g)
    step = FusedTrainStep(m, FusedSGD(m, lr=0.0), n_classes=n_classes, metrics=True, metrics_capacity=8)
    step.begin_epoch_metrics()
    for img, label in batches:
        step(img, label)
    em = step.epoch_metrics()
    assert isinstance(em, ClsTrainMetrics) and em.batches == 3 and np.array_equal(em.conf, conf)
    assert all(abs(a - b) <= 1e-12 or (a != a and b != b) for a, b in zip(em[:3], want)), (em[:3], want)
    small = FusedEvalStep(m, n_classes=n_classes, on_device=True, capacity=2)
    for img, label in batches:
        small(img, label)
    assert small._em_state.cpu().tolist() == [3, 1]
    with pytest.raises(L.MtbcError):
        small.result()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("n_classes", [3, 2])
def test_cls_test_step_table_is_the_rule_on_the_outputs(n_classes):
    binary = n_classes == 2
    m = _model(n_classes)
    test = INF.FusedClsTestStep(m, capacity=8)
    want, ids = [], []
    for n, seed in ((2, 70), (1, 71), (3, 72), (1, 73)):             # a batch of one, a last short batch
        img, label = _batch(n, seed, binary)
        test(img, label, patient_id=list(range(100 + len(ids), 100 + len(ids) + n)))
        ids += list(range(100 + len(ids), 100 + len(ids) + n))
        out = m.compiled(n, 64, 64).logits.data.view(n, -1).cpu()    # the read-back outputs of this batch
        for i in range(n):
            if binary:                                               # utils/models.py:489-494
                want.append([int(label[i].item()), int((torch.sigmoid(out[i]) > .5).double()[0].item())])
            else:                                                    # :427-445
                want.append([int(label[i].item()), int(out[i].argmax().item())])
    rows = test.result()
    assert test.table.tolist() == want and [r["patient_id"] for r in rows] == ids
    assert [[r["ground_truth"], r["predicted_label"]] for r in rows] == want
    rep = test.report(rows)
    assert ("Accuracy" in rep) if binary else ("accuracy" in rep and abs(rep["accuracy"] - np.mean([g_ == p_ for g_, p_ in want])) < 1e-12)
    # an eighth image fits, a ninth does not: nothing is written for that batch, it is counted, and result() refuses
    test(*_batch(1, 74, binary))
    assert len(test.result()) == 8
    before = test._rows.clone()
    test(*_batch(1, 75, binary))
    assert torch.equal(test._rows, before) and test._state.cpu().tolist() == [9, 1]
    with pytest.raises(L.MtbcError):
        test.result()
    test.reset()
    assert test._state.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 9
def test_refusals():
    m = _model()
    opt = FusedAdam(m, lr=1e-4, eps=1e-4)
    for kw in ({"alpha": 0.5}, {"seg_criterion": "DICE"}, {"inversely_weighted": False}):
        with pytest.raises(ValueError):
            FusedTrainStep(m, opt, **kw)
        with pytest.raises(ValueError):
            FusedEvalStep(m, **kw)
    with pytest.raises(NotImplementedError):
        FusedTrainStep(m, opt, distributed=True)
    with pytest.raises(NotImplementedError):
        FusedEvalStep(m, on_device=True, distributed=True)
    with pytest.raises(TypeError):
        FusedTrainStep(m, torch.optim.AdamW(m.parameters()))
    img, label = _batch(2, 1)
    mask = torch.zeros(2, 1, 64, 64, device=DEV)
    with pytest.raises(ValueError):
        FusedTrainStep(m, opt)(img, mask, label)                           # a mask for a model without a segmentation head
    with pytest.raises(ValueError):
        FusedTrainStep(m, opt)(img, None)                                  # ... and no label
    mt = MTnnUNet(1, 1, 3).to(DEV)
    with pytest.raises(ValueError, match="both"):
        T.fit_fold(FusedTrainStep(m, opt), FusedEvalStep(mt, alpha=0.5), None, None, None, None, "unused", 1, 1, None, 0, False)
    with pytest.raises(ValueError, match="both"):
        T.fit_fold(FusedTrainStep(mt, FusedAdam(mt, lr=1e-4, eps=1e-4), alpha=0.5), FusedEvalStep(m), None, None, None, None, "unused", 1, 1, None, 0, False)


# ------------------------------------------------------------------------------------------------ 11
_PROGRAMS = {"nnUNetClassifier": "MTnnUNet", "UNetPlusPlusClassifier": "MTUNetPlusPlus"}


def _make_model(arch):
    from multi_task_breast_cancer_amd.experiment_init import init_classification_model
    return init_classification_model(arch, sequences=1, n_classes=3)


def _surveys(arch):
    """(the multi-task survey, the classification-only survey) at the multi-task model's benchmark shape (bf16; nnUNetClassifier 64 x 256^2,
    UNetPlusPlusClassifier 32 x 256^2), each built (not run) once per session by tests/step_programs.py."""
    program = next(p for p in SP.STEP_PROGRAMS if p[0] == _PROGRAMS[arch])
    return SP.survey(program), SP.survey((arch,) + program[1:], build=SP.step_builder(_make_model, n_classes=3))


@pytest.mark.parametrize("arch", list(_PROGRAMS))
def test_cls_only_programs_launch_a_subset_of_the_multitask_programs(arch):
    """The kernel instances the classification-only step programs launch at the benchmark shape are a subset of the multi-task programs'; what
    they add is the softmax op (3-class nnUNetClassifier: one forward and one backward launch of softmax_rows_kernel) and, outside the programs,
    the two metrics kernels this file tests above (train_metrics_samples_kernel through mtbc_cls_step_metrics, cls_test_rows_kernel)."""
    mt, cl = _surveys(arch)
    for name in ("pack", "fwd", "loss", "bwd"):
        assert 0 < len(cl.kinds[name]) <= len(mt.kinds[name]), name
    softmax = [k for name in ("fwd", "bwd") for k in cl.kinds[name] if k == L.OP_SOFTMAX]
    assert len(softmax) == (2 if arch == "nnUNetClassifier" else 0) and L.OP_SOFTMAX not in mt.kinds["fwd"] + mt.kinds["bwd"]
    assert cl.kinds["loss"] == [L.OP_FOCAL, L.OP_LOSS_MIX]
    have, allowed = SP.kernel_instances(cl), SP.kernel_instances(mt)
    print(arch, len(have), "kernel instances of", len(allowed))
    assert len(have) >= 20, sorted(have)
    added = {"softmax_rows_kernel"} if arch == "nnUNetClassifier" else set()          # the one instance the docstring names, for the 3-class nnUNetClassifier only
    assert have - allowed == added, f"kernel instances of the classification-only programs that the multi-task programs do not launch: {sorted(have - allowed)}"
    SP.assert_keys_subset(cl, mt, [f for f in SP.COLLECTORS if f not in SP.NAMED])


def _pool_only_cases():
    """The one argument-selected branch the classification-only programs add to kernel instances the multi-task programs launch: the InstanceNorm
    backward of encoder1 .. encoder4's (conv_0_0 .. conv_3_0's second cell's) output, whose ONLY gradient is the folded max-pool one -- no skip
    connection reads these tensors here, so there is no gradient tensor (dy = NULL beside dy_pool).  It cannot be pinned away short of
    writing and reading a plane of zeros per level, so it gets fp64 cases of its own: the rows of tests/test_ops_gpu.py's INORM_CASES that carry
    pool=True, with dy=None, run by that file's own fp64 test (shapes, references and bounds are its own)."""
    import test_ops_gpu as OPS
    cases = []
    for par in (OPS._NOA, dict(**OPS._AFF, **OPS._DEF)):         # nnUNetClassifier: no affine; UNetPlusPlusClassifier: affine, deferred reductions
        for shape in ((2, 16, 12, 20), (2, 8, 24, 36), (1, 16, 48, 60)):
            cases.append((True, *shape, dict(OPS._BF, **par, dy=None, pool=True)))
        for N, C_, H, W, r in (OPS._T32, OPS._T8):
            cases.append((True, N, C_, H, W, dict(OPS._BF, **par, dy=None, pool=True, reserve_cus=r, rounds=">1")))
    return cases


def _pool_only_ids():
    import test_ops_gpu as OPS
    return [OPS._inorm_case_id(c) for c in _pool_only_cases()]


@pytest.mark.parametrize("case", _pool_only_cases(), ids=_pool_only_ids())
def test_instnorm_backward_with_only_the_folded_pool_gradient_matches_fp64(case):
    import test_ops_gpu as OPS
    OPS.test_instnorm_step_instances_match_fp64(case)


@pytest.mark.parametrize("arch", list(_PROGRAMS))
def test_cls_only_programs_launch_only_reference_tested_instances(arch):
    """Every coverage key of the classification-only step programs at the benchmark shape -- kernel instances AND the branches the arguments
    select, as tests/step_programs.py keys them -- is the key of a call that an element-wise fp64 reference test makes: the tables of
    tests/test_ops_gpu.py, plus the cases of `_pool_only_cases` above."""
    SP.assert_only_tested(_surveys(arch)[1], SP.reference_tested_keys(), SP.table_keys(inorm=_pool_only_cases()))
