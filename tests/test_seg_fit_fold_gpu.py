"""trainer.fit_fold with the segmentation pair of steps: the epoch loop of training_segmentation.py:143-201 on a device-resident dataset --
indexed training with metrics, indexed validation, the testing phase (forward, hole filling, per-image table) after every epoch, and the
driver's metrics.csv."""
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
from multi_task_breast_cancer_amd.nets import MTnnUNet, nnUNet  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")


def store(M, H, W, seed):
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def test_fit_fold_writes_the_segmentation_drivers_metrics_file(tmp_path):
    images, masks, labels = store(16, 64, 64, seed=33)
    ds = DD.DeviceDataset(images, masks, labels)
    seed_everything(1993)
    model = nnUNet(1, 1).to(DEV)
    opt = FusedAdam(model, lr=1e-3, eps=1e-4)
    step = T.FusedTrainStep(model, opt, metrics=True)
    eval_step, test_step = T.FusedEvalStep(model, on_device=True), I.FusedSegTestStep(model)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    d = 217                                                      # the driver's ONE draw np.random.choice(range(0, 360)) of the run (:118)
    transforms = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": d / 360}
    run_dir = str(tmp_path / "fold_0")
    train, val, test = EpochIndex(np.arange(10), 4, seed=13, drop_last=False), EpochIndex(np.arange(10, 13), 2, seed=13, drop_last=False), \
        EpochIndex(np.arange(13, 16), 2, seed=13, drop_last=False)
    rows = T.fit_fold(step, eval_step, ds, train, val, scheduler, run_dir, epochs=2, max_patience=5, transforms=transforms, seed=13,
                      plateau=False, test_step=test_step, test_index=test)
    assert len(rows) == 2 and all(len(r) == 7 for r in rows) and [r[0] for r in rows] == [0, 1]
    assert rows[0][1] < 1e-3 and rows[1][1] < rows[0][1]         # the learning rate AFTER the scheduler step, as the driver writes it (:193)
    lines = open(os.path.join(run_dir, "metrics.csv")).read().splitlines()
    assert lines[0] == "epoch,LR,Train,Validation,Test,Train_loss,Val_loss" == CK.SEG_METRICS_HEADER and len(lines) == 3
    for line, r in zip(lines[1:], rows):
        assert line == f"{r[0]},{r[1]:.8f},{r[2]:.4f}, {r[3]:.4f},{r[4]:.4f},{r[5]:.4f},{r[6]:.4f}"
        assert all(0.0 <= v <= 1.0 for v in r[2:5]) and r[5] > 0 and r[6] > 0
    # the Test column is the mean per-image DICE of the testing phase with the weights the epoch left: run it again by hand
    got = T.test_one_epoch_indexed(test_step, ds, DD.EpochTables(test, 0, None, device=ds.device))
    assert len(got) == 3 and rows[1][4] == float(np.mean([r["DICE"] for r in got]))
    ckpt = torch.load(os.path.join(run_dir, "model_best"), map_location="cpu", weights_only=False)
    assert ckpt["val_loss"] == min(r[6] for r in rows) and list(ckpt["model_state_dict"]) == list(model.state_dict())


def test_fit_fold_refuses_mixed_or_incomplete_segmentation_steps(tmp_path):
    seed_everything(3)
    seg, mt = nnUNet(1, 1).to(DEV), MTnnUNet(1, 1, 3).to(DEV)
    step = T.FusedTrainStep(seg, FusedAdam(seg, lr=1e-3, eps=1e-4), metrics=True)
    with pytest.raises(ValueError):                              # no testing phase given
        T.fit_fold(step, T.FusedEvalStep(seg), None, None, None, None, str(tmp_path / "a"), 1, 1, None, 0, False)
    with pytest.raises(ValueError):                              # a multi-task evaluation step beside a segmentation-only training step
        T.fit_fold(step, T.FusedEvalStep(mt, alpha=0.5), None, None, None, None, str(tmp_path / "b"), 1, 1, None, 0, False,
                   test_step=I.FusedSegTestStep(seg), test_index=EpochIndex(np.arange(2), 2, seed=1))
