"""trainer.fit_fold with the classification pair of steps: the epoch loop of training_classification.py:216-271 on a device-resident dataset --
indexed training with metrics, indexed validation, the driver's metrics.csv, a checkpoint on improvement -- and its testing phase afterwards."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import checkpoint as CK  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import inference as I  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import UNetPlusPlusClassifier, nnUNetClassifier  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdamW  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def store(M, H, W, seed):
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


@pytest.mark.parametrize("arch", [nnUNetClassifier, UNetPlusPlusClassifier])
def test_fit_fold_writes_the_classification_drivers_metrics_file(arch, tmp_path):
    images, masks, labels = store(16, 64, 64, seed=33)
    ds = DD.DeviceDataset(images, masks, labels)
    seed_everything(1993)
    model = (arch(1, 3) if arch is nnUNetClassifier else arch(2, 1, 3)).to(DEV)
    model.ensure_flat()
    initial = {n: model._param_view(n).clone() for n in model.untrained}
    opt = FusedAdamW(model, lr=1e-3)                             # the optimizer whose decay would move a never-trained parameter
    step = T.FusedTrainStep(model, opt, n_classes=3, cls_criterion="Focal", metrics=True)
    eval_step = T.FusedEvalStep(model, n_classes=3, cls_criterion="Focal", on_device=True)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    transforms = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}
    run_dir = str(tmp_path / "fold_0")
    train, val, test = EpochIndex(np.arange(10), 4, seed=13, drop_last=False), EpochIndex(np.arange(10, 13), 2, seed=13, drop_last=False), \
        EpochIndex(np.arange(13, 16), 2, seed=13, drop_last=False)
    rows = T.fit_fold(step, eval_step, ds, train, val, scheduler, run_dir, epochs=2, max_patience=5, transforms=transforms, seed=13, plateau=False)
    assert len(rows) == 2 and all(len(r) == 8 for r in rows) and [r[0] for r in rows] == [0, 1]
    assert rows[0][1] == 1e-3 and rows[1][1] < rows[0][1]        # the learning rate at the START of the epoch (:219)
    lines = open(os.path.join(run_dir, "metrics.csv")).read().splitlines()
    assert lines[0] == "epoch,LR,Train_loss,Validation_loss,Train_acc,Train_F1,Validation_acc,Validation_F1" == CK.CLS_METRICS_HEADER and len(lines) == 3
    for line, r in zip(lines[1:], rows):
        assert line == f"{r[0]},{r[1]:.8f},{r[2]:.4f},{r[3]:.4f},{r[4]:.4f},{r[5]:.4f},{r[6]:.4f},{r[7]:.4f}"
        assert r[2] > 0 and r[3] > 0 and all(0.0 <= v <= 1.0 for v in r[4:])
        assert abs(r[4] - r[5]) < 1e-12 and abs(r[6] - r[7]) < 1e-12          # micro F1 over all three labels is the accuracy
    ckpt = torch.load(os.path.join(run_dir, "model_best"), map_location="cpu", weights_only=False)
    assert ckpt["val_loss"] == min(r[3] for r in rows) and list(ckpt["model_state_dict"]) == list(model.state_dict())
    assert all(torch.equal(model._param_view(n), v) for n, v in initial.items())
    # the testing phase, once, after the loop (:284-298): three images in batches of 2 + 1
    test_step = I.FusedClsTestStep(model)
    got = T.test_one_epoch_indexed(test_step, ds, DD.EpochTables(test, 0, None, device=ds.device))
    assert len(got) == 3 and sorted(r["ground_truth"] for r in got) == sorted(labels[13:16].tolist())
    assert all(r["predicted_label"] in (0, 1, 2) for r in got)
    test_step.write_csv(str(tmp_path / "results.csv"), got)
    assert open(tmp_path / "results.csv").read().splitlines()[0] == "patient_id,ground_truth,predicted_label"
    assert abs(test_step.report(got)["accuracy"] - np.mean([r["ground_truth"] == r["predicted_label"] for r in got])) < 1e-12
