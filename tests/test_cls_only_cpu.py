"""The single-task classification baseline (`nnUNetClassifier`, `UNetPlusPlusClassifier`) without a GPU: the softmax row functions compiled for
the host, initial weights and state-dict layout against the reference-pinned fixture, the never-trained parameters' place in the flat buffers, the
factories and the criterion glue, the driver's metric formulas against sklearn, the metrics.csv row and the testing phase's CSV / report code."""
import inspect
import math
import os
import types

import numpy as np
import pytest
import torch

from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd import checkpoint as CK
from multi_task_breast_cancer_amd import criterions as CR
from multi_task_breast_cancer_amd import experiment_init as EI
from multi_task_breast_cancer_amd import inference as INF
from multi_task_breast_cancer_amd import nets, ops
from multi_task_breast_cancer_amd import trainer as T
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD
from test_oracle_goldens import _sha


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_nnunet_step.npz"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


# ------------------------------------------------------------------------------------------------ softmax rows on the host
def softmax_cases():
    """(x, dp) pairs: C = 2 and 3, N = 1, 2 and 7; a row of equal logits, rows with a +-80 and a +-40 spread, a row containing -inf."""
    g = torch.Generator().manual_seed(7)
    out = []
    for C in (2, 3):
        special = [torch.zeros(C) + 1.25, torch.tensor([80.0, -80.0, 0.0][:C]), torch.tensor([0.5, -float("inf"), 1.0][:C]),
                   torch.tensor([-40.0, 40.0, 0.3][:C])]
        for s in special[:3]:
            out.append(s.view(1, C).clone())
        out.append(torch.randn(1, C, generator=g) * 3)
        out.append(torch.stack([special[0], special[1]]))
        out.append(torch.randn(2, C, generator=g) * 3)
        out.append(torch.stack([torch.randn(C, generator=g), special[0], special[1], special[2], torch.randn(C, generator=g) * 10, special[3],
                                torch.randn(C, generator=g) * 0.01]))
    return [(x, torch.randn(x.shape, generator=g)) for x in out]


def softmax_references(cases):
    """Per case (p64, dz64) by torch in float64, and the largest error of torch's own float32 softmax / autograd backward over ALL the cases."""
    refs, e_fwd, e_bwd = [], 0.0, 0.0
    for x, dp in cases:
        xd = x.double().requires_grad_(True)
        pd = torch.softmax(xd, dim=1)
        pd.backward(dp.double())
        xf = x.clone().requires_grad_(True)
        pf = torch.softmax(xf, dim=1)
        pf.backward(dp)
        refs.append((pd.detach(), xd.grad))
        e_fwd = max(e_fwd, (pf.detach().double() - pd.detach()).abs().max().item())
        e_bwd = max(e_bwd, (xf.grad.double() - xd.grad).abs().max().item())
    return refs, e_fwd, e_bwd


def within(got: torch.Tensor, want64: torch.Tensor, e32: float) -> bool:
    """|got - want| <= max(8 x torch's float32 error, 1 float32 ulp of the value), element by element."""
    ulp = torch.from_numpy(np.spacing(np.abs(want64.numpy()).astype(np.float32)).astype(np.float64))
    return bool(((got.double() - want64).abs() <= torch.maximum(torch.full_like(want64, 8 * e32), ulp)).all())


def test_softmax_rows_host_against_float64_torch(lib):
    """Bound: 8 x the largest error torch's own float32 softmax (and its autograd backward) shows against float64 on the same rows, floor 1 float32
    ulp of the value.  Measured on these rows: torch float32 4.61e-08 forward, 7.00e-08 backward; the host row functions 4.61e-08 and 7.00e-08."""
    cases = softmax_cases()
    assert {tuple(x.shape) for x, _ in cases} == {(n, c) for n in (1, 2, 7) for c in (2, 3)}
    refs, e_fwd, e_bwd = softmax_references(cases)
    print(f"torch float32 against float64: forward {e_fwd:.3e}, backward {e_bwd:.3e}")
    assert 0 < e_fwd < 1e-6 and 0 < e_bwd < 1e-6
    worst_f = worst_b = 0.0
    for (x, dp), (p64, dz64) in zip(cases, refs):
        p, dz = ops.softmax_rows_host(x, dp)
        assert torch.equal(p, ops.softmax_rows_host(x))
        worst_f = max(worst_f, (p.double() - p64).abs().max().item())
        worst_b = max(worst_b, (dz.double() - dz64).abs().max().item())
        assert within(p, p64, e_fwd), (x, p, p64)
        assert within(dz, dz64, e_bwd), (x, dz, dz64)
    print(f"mtbc_softmax_rows_host against float64: forward {worst_f:.3e}, backward {worst_b:.3e}")


def test_softmax_rows_host_special_rows_and_refusals(lib):
    p = ops.softmax_rows_host(torch.tensor([[2.0, 2.0], [0.5, -float("inf")]]))
    assert p.tolist() == [[0.5, 0.5], [1.0, 0.0]]
    assert torch.isnan(ops.softmax_rows_host(torch.full((1, 3), -float("inf")))).all()       # as torch
    for shape in ((1, 4), (0, 3)):
        with pytest.raises(Exception, match="bad shape"):
            ops.softmax_rows_host(torch.zeros(shape))


# ------------------------------------------------------------------------------------------------ models against the fixture
@pytest.mark.parametrize("n_classes", [3, 2])
def test_initial_weights_are_the_references(golden, n_classes):
    seed_everything(1993)
    model = nets.nnUNetClassifier(1, n_classes)
    assert _sha(model.state_dict()) == str(golden[f"sha256_init_{n_classes}"])
    assert model.architecture == "nnUNetClassifier" and model.n_classes == (1 if n_classes == 2 else 3) and T.is_cls_only(model)
    assert not T.is_seg_only(model) and not T.is_cls_only(nets.MTnnUNet(1, 1, 3)) and not T.is_cls_only(nets.nnUNet(1, 1))


def test_state_dict_names_and_shapes_are_the_fixtures(golden):
    sd = nets.nnUNetClassifier(1, 3).state_dict()
    assert list(sd) == [str(n) for n in golden["names"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in golden["shapes"]]
    assert "upsample5.weight" in sd and not any(k.startswith(("upsample4", "upsample3", "upsample2", "upsample1", "output")) for k in sd)
    mt = nets.MTnnUNet(1, 1, 3).state_dict()
    assert all(k in mt and mt[k].shape == v.shape for k, v in sd.items())


def test_never_trained_parameters_are_the_fixtures_and_lie_behind_the_live_prefix(golden):
    model = nets.nnUNetClassifier(1, 3)
    assert sorted(model.untrained) == sorted(str(n) for n in golden["grad_none"]) == sorted(nets.NNUNET_CLS_UNTRAINED)
    live = [model.slots[n] for n in model._order if n not in model.untrained]
    dead = [model.slots[n] for n in model._order if n in model.untrained]
    assert [s.offset for s in live] == sorted(s.offset for s in live) and live[0].offset == 0
    assert all(s.offset + s.numel <= model.live_numel for s in live) and all(s.offset >= model.live_numel for s in dead)
    assert model.live_numel % 4 == 0 and model.live_numel < model.flat_numel
    assert max(s.offset + s.numel for s in dead) <= model.flat_numel
    # every other model: the whole buffer is live and the layout is the construction order, as it was
    for other in (nets.MTnnUNet(1, 1, 3), nets.nnUNet(1, 1), nets.MTUNetPlusPlus(), nets.UNetPlusPlusClassifier()):
        offs = [other.slots[n].offset for n in other._order]
        assert other.live_numel == other.flat_numel and not other.untrained and offs == sorted(offs) and offs[0] == 0


def test_unetpp_classifier_names_are_a_subset_of_the_multitask_models():
    sd, mt = nets.UNetPlusPlusClassifier(2, 1, 3).state_dict(), nets.MTUNetPlusPlus(2, 1, 1, 3).state_dict()
    assert all(k in mt and mt[k].shape == v.shape for k, v in sd.items())
    assert {k.split(".")[0] for k in sd} == {"conv_0_0", "conv_1_0", "conv_2_0", "conv_3_0", "conv_4_0", "upcat_3_1", "process_level_3", "classifier"}
    assert [k for k in mt if k in sd] == list(sd)
    assert nets.UNetPlusPlusClassifier(n_classes=2).state_dict()["classifier.5.weight"].shape == (1, 256)
    with pytest.raises(ValueError):
        nets.UNetPlusPlusClassifier(spatial_dims=3)


# ------------------------------------------------------------------------------------------------ factories and glue
CONFIG_DATA = {"classes": ["benign", "malignant", "normal"], "classes_weighted": None}
CONFIG_LOSS = {"classification_criterion": "CE"}


def config_opt(opt):
    return {"opt": opt, "lr": 1e-4, "scheduler": "cosine", "t_max": 20, "patience": 7, "min_lr": 1e-6, "decrease_factor": 0.5}


def test_init_classification_model(tmp_path):
    model = EI.init_classification_model("nnUNetClassifier", sequences=3, n_classes=3, width=48, save_folder=tmp_path / "run")
    assert isinstance(model, nets.nnUNetClassifier) and model.in_channels == 3 and (tmp_path / "run" / "model.txt").exists()
    assert isinstance(EI.init_classification_model("UNetPlusPlusClassifier", sequences=2, n_classes=2), nets.UNetPlusPlusClassifier)
    assert list(inspect.signature(EI.init_classification_model).parameters) == ["architecture", "sequences", "n_classes", "width", "save_folder"]
    for name in ("BTSUNetClassifier", "MTnnUNet", "nnUNet", ""):
        with pytest.raises(ValueError):
            EI.init_classification_model(name)
    with pytest.raises(ValueError):
        EI.init_multitask_model("nnUNetClassifier")


@pytest.mark.parametrize("opt,kind", [("Adam", FusedAdam), ("SGD", FusedSGD), ("AdamW", FusedAdamW)])
def test_load_classification_experiment_artefacts(opt, kind):
    cm = {"architecture": "nnUNetClassifier", "sequences": 1, "width": 48}
    out = EI.load_classification_experiment_artefacts(CONFIG_DATA, cm, config_opt(opt), CONFIG_LOSS, 1, None, fused=True)
    model, optimizer, criterion, sched = out
    assert isinstance(model, nets.nnUNetClassifier) and model.in_channels == 2 and model.n_classes == 3
    assert isinstance(optimizer, kind) and isinstance(criterion, torch.nn.CrossEntropyLoss)
    assert isinstance(sched, torch.optim.lr_scheduler.CosineAnnealingLR)
    assert list(inspect.signature(EI.load_classification_experiment_artefacts).parameters) == [
        "config_data", "config_model", "config_opt", "config_loss", "n_augments", "run_path", "fused"]
    assert optimizer.state_dict()["state"] == {}            # nothing stepped yet


def test_apply_criterion_classification_is_the_references_glue():
    assert list(inspect.signature(CR.apply_criterion_classification).parameters) == ["criterion_class", "label", "predicted_class",
                                                                                     "inversely_weighted"]
    crit = lambda c, t: (c - 1.0).abs().mean()              # noqa: E731  (any criterion: the glue is host arithmetic)
    label = torch.zeros(2, 3)
    assert CR.apply_criterion_classification(crit, label, torch.full((2, 3), 3.0)).item() == 2.0
    preds = [torch.full((2, 3), v) for v in (2.0, 4.0)]
    for iw in (False, True):                                # a list of labels: the same sum either way
        assert CR.apply_criterion_classification(crit, [label], preds, iw).item() == 4.0
    with pytest.raises(SystemExit) as e:
        CR.apply_criterion_classification(crit, label, torch.full((2, 3), float("nan")))
    assert e.value.code == 1


def test_refusals_are_host_logic():
    model = nets.nnUNetClassifier(1, 3)
    opt = FusedAdam(model, lr=1e-4, eps=1e-4)
    with pytest.raises(ValueError, match="alpha"):
        T.FusedTrainStep(model, opt, alpha=0.5)
    with pytest.raises(ValueError, match="seg_criterion"):
        T.FusedTrainStep(model, opt, seg_criterion="DICE")
    with pytest.raises(ValueError, match="inversely_weighted"):
        T.FusedEvalStep(model, inversely_weighted=True)
    with pytest.raises(NotImplementedError):
        T.FusedTrainStep(model, opt, distributed=True)
    with pytest.raises(NotImplementedError):
        T.FusedEvalStep(model, on_device=True, distributed=True)
    with pytest.raises(TypeError):
        T.FusedTrainStep(model, torch.optim.Adam(model.parameters()))
    with pytest.raises(ValueError, match="n_classes"):
        T.FusedTrainStep(model, opt, n_classes=2)
    with pytest.raises(NotImplementedError):
        T.FusedTrainStep(model, opt, cls_criterion="CE", focal_weight=torch.ones(3))
    for alpha in (None, 0.0):
        step = T.FusedTrainStep(model, opt, alpha=alpha, n_classes=3, cls_criterion="CE")
        assert step.cls_only and not step.seg_only and step.alpha == 0.0 and step.cls_gamma == 0.0 and not step.binary
    ev = T.FusedEvalStep(model)
    assert ev.cls_only and ev.alpha == 0.0 and ev.cls_gamma == 2.0
    with pytest.raises(ValueError, match="both"):
        T.fit_fold(step, T.FusedEvalStep(nets.MTnnUNet(1, 1, 3), alpha=0.5), None, None, None, None, "unused", 1, 1, None, 0, False)
    with pytest.raises(ValueError):
        INF.FusedClsTestStep(nets.MTnnUNet(1, 1, 3))


# ------------------------------------------------------------------------------------------------ the driver's metrics
MATRICES = [np.array([[5, 1, 0], [2, 7, 1], [0, 3, 4]]), np.array([[4, 0, 0], [0, 0, 0], [1, 0, 2]]),       # the second: class 1 is empty
            np.array([[0, 3, 0], [0, 0, 2], [1, 0, 0]]), np.array([[9, 0, 0], [0, 0, 0], [0, 0, 0]])]


def labels_of(conf):
    gt, pr = [], []
    for i in range(3):
        for j in range(3):
            gt += [i] * int(conf[i, j])
            pr += [j] * int(conf[i, j])
    return gt, pr


@pytest.mark.parametrize("conf", MATRICES)
def test_three_class_scores_are_sklearns(conf):
    from sklearn.metrics import accuracy_score, f1_score
    gt, pr = labels_of(conf)
    acc, f1 = T.cls_driver_scores(conf.astype(np.float64), binary=False)
    assert abs(acc - accuracy_score(gt, pr)) <= 1e-12
    assert abs(f1 - f1_score(y_true=gt, y_pred=pr, labels=[0, 1, 2], average="micro")) <= 1e-12


@pytest.mark.parametrize("tn,fp,fn,tp", [(3, 1, 2, 5), (4, 0, 0, 0), (0, 0, 3, 0), (0, 2, 0, 6)])
def test_binary_scores_are_the_reference_formulas(tn, fp, fn, tp):
    conf = np.zeros((3, 3))
    conf[0, 0], conf[0, 1], conf[1, 0], conf[1, 1] = tn, fp, fn, tp
    acc, f1 = T.cls_driver_scores(conf, binary=True)
    gt = torch.tensor([0.0] * (tn + fp) + [1.0] * (fn + tp))
    pr = torch.tensor([0.0] * tn + [1.0] * fp + [0.0] * fn + [1.0] * tp)
    t_tp = torch.sum(torch.logical_and(pr, gt)).double()                      # accuracy_from_tensor / f1_score_from_tensor restated
    t_tn = torch.sum(torch.logical_and(torch.logical_not(pr), torch.logical_not(gt))).double()
    t_fp = torch.sum(torch.logical_and(pr, torch.logical_not(gt))).double()
    t_fn = torch.sum(torch.logical_and(torch.logical_not(pr), gt)).double()
    want_acc, want_f1 = ((t_tp + t_tn) / (t_tp + t_tn + t_fp + t_fn)).item(), ((2 * t_tp) / (2 * t_tp + t_fp + t_fn)).item()
    assert abs(acc - want_acc) <= 1e-12
    if math.isnan(want_f1):                                                   # 0 / 0: NaN, as the reference gives
        assert tp == fp == fn == 0 and math.isnan(f1)
    else:
        assert abs(f1 - want_f1) <= 1e-12


def test_binary_scores_of_an_empty_matrix_are_nan():
    acc, f1 = T.cls_driver_scores(np.zeros((3, 3)), binary=True)
    assert math.isnan(acc) and math.isnan(f1)


def test_eval_result_from_counts():
    conf = MATRICES[0]
    table = np.array([[0, 0, 0, 12], [0, 0, 0, 11]])
    rows = np.array([[0.5, 0.0, 0.5, 0.0], [0.25, 0.0, 0.25, 0.0]])
    loss, acc, f1 = T.cls_eval_result_from_counts(table, conf, rows, binary=False)
    assert loss == 0.375 and (acc, f1) == T.cls_driver_scores(conf, False)
    rows[1, 3] = 1.0
    with pytest.raises(SystemExit):
        T.cls_eval_result_from_counts(table, conf, rows, binary=False)


def test_metrics_csv_header_and_row():
    assert CK.CLS_METRICS_HEADER == "epoch,LR,Train_loss,Validation_loss,Train_acc,Train_F1,Validation_acc,Validation_F1"
    epoch, current_lr, avg_train_loss, avg_validation_loss, train_acc, train_f1_score, val_acc, val_f1_score = 3, 1e-4, 0.51234, 1.25, 2 / 3, 0.5, 1.0, 0.0
    want = (f'{epoch},{current_lr:.8f},{avg_train_loss:.4f},{avg_validation_loss:.4f},'          # training_classification.py:263-265
            f'{train_acc:.4f},'
            f'{train_f1_score:.4f},{val_acc:.4f},{val_f1_score:.4f}')
    assert CK.cls_metrics_row(epoch, current_lr, avg_train_loss, avg_validation_loss, train_acc, train_f1_score, val_acc, val_f1_score) == want
    assert want == "3,0.00010000,0.5123,1.2500,0.6667,0.5000,1.0000,0.0000" and len(want.split(",")) == len(CK.CLS_METRICS_HEADER.split(","))


# ------------------------------------------------------------------------------------------------ the testing phase's host code
def test_cls_test_step_csv_and_report(tmp_path):
    table = np.array([[0, 0], [1, 2], [2, 2], [1, 1], [0, 1]])
    rows = INF.cls_rows_from_table(table, ids=[7, 8, 9, 10, 11])
    assert rows[1] == {"patient_id": 8, "ground_truth": 1, "predicted_label": 2}
    assert [r["patient_id"] for r in INF.cls_rows_from_table(table)] == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        INF.cls_rows_from_table(table, ids=[1])
    path = tmp_path / "results.csv"
    INF.write_cls_rows_csv(str(path), rows)
    assert path.read_text() == "patient_id,ground_truth,predicted_label\n7,0,0\n8,1,2\n9,2,2\n10,1,1\n11,0,1\n"
    step = INF.FusedClsTestStep(types.SimpleNamespace(cls_only=True, n_classes=3))
    rep = step.report(rows)
    from sklearn.metrics import accuracy_score, f1_score, precision_score
    gt, pr = table[:, 0], table[:, 1]
    assert abs(rep["accuracy"] - accuracy_score(gt, pr)) <= 1e-12
    assert abs(rep["f1_macro"] - f1_score(gt, pr, labels=[0, 1, 2], average="macro")) <= 1e-12
    assert abs(rep["precision_class_2"] - precision_score(gt, pr, labels=[0, 1, 2], average=None)[2]) <= 1e-12
    binary = INF.FusedClsTestStep(types.SimpleNamespace(cls_only=True, n_classes=1))
    brep = binary.report(INF.cls_rows_from_table(np.array([[0, 0], [1, 1], [1, 0], [0, 1], [1, 1]])))
    assert brep == {"Precision": 2 / 3, "Sensitivity": 2 / 3, "Specificity": 0.5, "Accuracy": 0.6, "F1 score": 2 / 3}
    with pytest.raises(Exception, match="before any batch"):
        step.result()


def test_product_path_has_no_cpu_fallback():
    with pytest.raises(L.MtbcError):
        nets.nnUNetClassifier(1, 3)(torch.zeros(1, 1, 64, 64))
