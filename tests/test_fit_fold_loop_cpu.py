"""The epoch loop of `trainer.fit_fold` for its three drivers -- multi-task, segmentation, classification -- without a GPU: stand-in steps, the
three epoch functions, `EpochTables` and `save_checkpoint` replaced by scripted versions that record their calls.  What the loop writes
(metrics.csv byte for byte, the log lines), what it returns, which learning rate a row carries, what the scheduler and the checkpoint see, where
it stops, when the testing phase runs, and that every refusal comes before the run directory exists."""
import logging
import os
import re
import sys
import types

import pytest
import torch

from multi_task_breast_cancer_amd import checkpoint as CK
from multi_task_breast_cancer_amd import device_data as DD
from multi_task_breast_cancer_amd import trainer as T

# the scripted epochs: validation improves twice, then not for two epochs -> with max_patience = 1 the loop ends behind epoch 3 of 6
TRAIN_LOSS = [1.5, 1.25, 1.125, 1.0625, 1.0, 0.9]
VAL_LOSS = [0.5, 0.25, 0.375, 0.3125, 0.125, 0.0625]
TRAIN_DICE = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
VAL_DICE = [0.15, 0.25, 0.35, 0.45, 0.55, 0.65]
TRAIN_ACC = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]
TRAIN_F1 = [0.45, 0.5, 0.55, 0.6, 0.65, 0.7]
VAL_ACC = [0.4, 0.45, 0.5, 0.55, 0.6, 0.65]
VAL_F1 = [0.35, 0.4, 0.45, 0.5, 0.55, 0.6]
SEG_VAL = [0.3, 0.2, 0.25, 0.21, 0.1, 0.05]
CLS_VAL = [0.2, 0.05, 0.125, 0.1025, 0.025, 0.0125]
TEST_DICE = [0.5, 0.5625, 0.625, 0.6875, 0.75, 0.8125]          # the mean of the two rows the scripted testing phase returns
EPOCHS, PATIENCE, RAN = 6, 1, 4
LR0 = 0.1
LR_BEFORE = [LR0 * 0.5 ** e for e in range(RAN)]                # halved by the scheduler once per epoch: exact in binary
LR_AFTER = [LR0 * 0.5 ** (e + 1) for e in range(RAN)]

CSV = {
    "multi": "epoch,LR,Train_loss,Validation_loss,Train_dice,Validation_dice,Train_acc,Train_F1,Validation_acc,Validation_F1\n"
             "0,0.10000000,1.5000,0.5000,0.1000, 0.1500,0.5000,0.4500,0.4000,0.3500\n"
             "1,0.05000000,1.2500,0.2500,0.2000, 0.2500,0.5500,0.5000,0.4500,0.4000\n"
             "2,0.02500000,1.1250,0.3750,0.3000, 0.3500,0.6000,0.5500,0.5000,0.4500\n"
             "3,0.01250000,1.0625,0.3125,0.4000, 0.4500,0.6500,0.6000,0.5500,0.5000\n",
    "seg": "epoch,LR,Train,Validation,Test,Train_loss,Val_loss\n"
           "0,0.05000000,0.1000, 0.1500,0.5000,1.5000,0.5000\n"
           "1,0.02500000,0.2000, 0.2500,0.5625,1.2500,0.2500\n"
           "2,0.01250000,0.3000, 0.3500,0.6250,1.1250,0.3750\n"
           "3,0.00625000,0.4000, 0.4500,0.6875,1.0625,0.3125\n",
    "cls": "epoch,LR,Train_loss,Validation_loss,Train_acc,Train_F1,Validation_acc,Validation_F1\n"
           "0,0.10000000,1.5000,0.5000,0.5000,0.4500,0.4000,0.3500\n"
           "1,0.05000000,1.2500,0.2500,0.5500,0.5000,0.4500,0.4000\n"
           "2,0.02500000,1.1250,0.3750,0.6000,0.5500,0.5000,0.4500\n"
           "3,0.01250000,1.0625,0.3125,0.6500,0.6000,0.5500,0.5000\n",
}
FIRST_LOG = {
    "multi": "EPOCH 0 --> || Training loss 1.5000 || Validation loss 0.5000 || Segmentation val loss 0.3000 || Classification val loss 0.2000 "
             "|| Training DICE 0.1000 || Validation DICE  0.1500 || Training ACC 0.5000 || Training F1 0.4500 || Validation ACC 0.4000 "
             "|| Validation F1 0.3500 || Patience: 0 || Epoch time: T|| Best validation performance: 0.5000",
    "seg": "EPOCH 0 --> || Training loss 1.5000 || Validation loss 0.5000 || Training DICE 0.1000 || Validation DICE  0.1500 || Patience: 0 "
           "|| Epoch time: T || LR: 0.05000000",
    "cls": "EPOCH 0 --> || Training loss 1.5000 || Validation loss 0.5000 || Training ACC 0.5000 || Training F1 0.4500 || Validation ACC 0.4000 "
           "|| Validation F1 0.3500 || Patience: 0 || Epoch time: T",
}
LAST_LOG_TAIL = {"multi": "|| Patience: 2 || Epoch time: T|| Best validation performance: 0.2500",
                 "seg": "|| Patience: 2 || Epoch time: T || LR: 0.00625000",
                 "cls": "|| Patience: 2 || Epoch time: T"}
STOP_LOG = "\nValidation loss did not improve over the last 2 epochs. Stopping training"


def expected_rows(task):
    if task == "multi":
        return [(e, LR_BEFORE[e], TRAIN_LOSS[e], VAL_LOSS[e], TRAIN_DICE[e], VAL_DICE[e], TRAIN_ACC[e], TRAIN_F1[e], VAL_ACC[e], VAL_F1[e])
                for e in range(RAN)]
    if task == "seg":
        return [(e, LR_AFTER[e], TRAIN_DICE[e], VAL_DICE[e], TEST_DICE[e], TRAIN_LOSS[e], VAL_LOSS[e]) for e in range(RAN)]
    return [(e, LR_BEFORE[e], TRAIN_LOSS[e], VAL_LOSS[e], TRAIN_ACC[e], TRAIN_F1[e], VAL_ACC[e], VAL_F1[e]) for e in range(RAN)]


def task_attributes(task):
    """What a step of each task carries; the multi-task stand-in has neither attribute, as the stand-ins of older tests."""
    return {"multi": {}, "seg": {"seg_only": True, "cls_only": False}, "cls": {"seg_only": False, "cls_only": True}}[task]


class HalvingScheduler:
    """Records what `step` was given and halves the learning rate, as StepLR(step_size=1, gamma=.5) does."""

    def __init__(self, opt, calls):
        self.opt, self.calls = opt, calls

    def step(self, *args):
        self.calls.append(("scheduler",) + args)
        for g in self.opt.param_groups:
            g["lr"] *= 0.5


class Script:
    """The stand-in steps of one task and the scripted epoch functions; every call lands in `calls` in order."""

    def __init__(self, task, monkeypatch, distributed=False):
        self.task, self.calls, self.epoch = task, [], -1
        self.opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=LR0)
        self.model = object()
        self.step = types.SimpleNamespace(opt=self.opt, model=self.model, scaler=None, distributed=distributed, metrics=True, **task_attributes(task))
        self.eval_step = types.SimpleNamespace(distributed=distributed, **task_attributes(task))
        self.test_step, self.test_index = (object(), "test-index") if task == "seg" else (None, None)
        self.dataset = types.SimpleNamespace(device="cpu")
        monkeypatch.setattr(DD, "EpochTables", self.tables)
        monkeypatch.setattr(CK, "save_checkpoint", self.save)
        monkeypatch.setattr(T, "train_one_epoch_with_metrics", self.train)
        monkeypatch.setattr(T, "validate_one_epoch_indexed", self.validate)
        monkeypatch.setattr(T, "test_one_epoch_indexed", self.test)

    def tables(self, index, epoch, transforms, seed=None, device=None):
        self.calls.append(("tables", index, epoch, transforms, seed, device))
        return ("tables-of", index, epoch)

    def save(self, path, epoch, model, optimizer, val_loss, scaler="not given"):
        self.calls.append(("save", path, epoch, model, optimizer, val_loss, scaler))

    def train(self, step, dataset, tables):
        assert step is self.step and dataset is self.dataset
        self.epoch += 1
        e = self.epoch
        self.calls.append(("train", tables))
        self.opt.step()                         # a scheduler wants the optimizer stepped first
        return {"multi": (TRAIN_LOSS[e], TRAIN_DICE[e], TRAIN_ACC[e], TRAIN_F1[e]), "seg": (TRAIN_LOSS[e], TRAIN_DICE[e]),
                "cls": (TRAIN_LOSS[e], TRAIN_ACC[e], TRAIN_F1[e])}[self.task]

    def validate(self, step, dataset, tables):
        assert step is self.eval_step and dataset is self.dataset
        e = self.epoch
        self.calls.append(("validate", tables))
        return {"multi": (VAL_LOSS[e], VAL_DICE[e], VAL_ACC[e], VAL_F1[e], SEG_VAL[e], CLS_VAL[e]), "seg": (VAL_LOSS[e], VAL_DICE[e]),
                "cls": (VAL_LOSS[e], VAL_ACC[e], VAL_F1[e])}[self.task]

    def test(self, step, dataset, tables):
        assert step is self.test_step and dataset is self.dataset
        self.calls.append(("test", tables))
        return [{"DICE": 0.25 + 0.125 * self.epoch}, {"DICE": 0.75}]

    def fit(self, scheduler, run_dir, plateau, **kw):
        kw.setdefault("test_step", self.test_step)
        kw.setdefault("test_index", self.test_index)
        return T.fit_fold(self.step, self.eval_step, self.dataset, "train-index", "val-index", scheduler, run_dir, EPOCHS, PATIENCE,
                          {"horizontal_flip": .5}, 11, plateau, checkpoint_name="best.pt", **kw)


def expected_calls(task, run_dir, plateau, saves=True):
    """The order of everything the loop does: the validation (and testing) tables once, then per epoch the training tables, training, validation,
    the scheduler, a checkpoint on a new best only, and -- segmentation only -- the testing phase BEHIND the checkpoint decision."""
    out = [("tables", "val-index", 0, None, None, "cpu")]
    if task == "seg":
        out.append(("tables", "test-index", 0, None, None, "cpu"))
    for e in range(RAN):
        out += [("tables", "train-index", e, {"horizontal_flip": .5}, 11, "cpu"), ("train", ("tables-of", "train-index", e)),
                ("validate", ("tables-of", "val-index", 0)), ("scheduler", VAL_LOSS[e]) if plateau else ("scheduler",)]
        if e < 2 and saves:                     # 0.5, then 0.25: the two new bests
            out.append(("save", os.path.join(run_dir, "best.pt"), e, "MODEL", "OPT", VAL_LOSS[e], None))
        if task == "seg":
            out.append(("test", ("tables-of", "test-index", 0)))
    return out


def normalised(script):
    return [tuple("MODEL" if v is script.model else "OPT" if v is script.opt else v for v in c) for c in script.calls]


def messages(caplog):
    return [re.sub(r"Epoch time: [0-9.]+", "Epoch time: T", r.getMessage()) for r in caplog.records if r.name == "root"]


@pytest.mark.parametrize("plateau", [False, True], ids=["steplr", "plateau"])
@pytest.mark.parametrize("task", ["multi", "seg", "cls"])
def test_the_loop_of_each_driver(task, plateau, tmp_path, monkeypatch, caplog):
    s = Script(task, monkeypatch)
    run_dir = str(tmp_path / "run")
    if plateau:
        scheduler = HalvingScheduler(s.opt, s.calls)
    else:
        scheduler = torch.optim.lr_scheduler.StepLR(s.opt, step_size=1, gamma=0.5)
        real = scheduler.step
        scheduler.step = lambda *a: (s.calls.append(("scheduler",) + a), real(*a))[1]
    with caplog.at_level(logging.INFO):
        rows = s.fit(scheduler, run_dir, plateau)
    assert rows == expected_rows(task) and len(rows) == RAN                             # stopped at patience 2 > max_patience 1, not at 6 epochs
    assert [r[1] for r in rows] == (LR_AFTER if task == "seg" else LR_BEFORE)           # which learning rate a row carries
    with open(os.path.join(run_dir, "metrics.csv"), "rb") as f:
        assert f.read() == CSV[task].encode()
    assert sorted(os.listdir(run_dir)) == ["metrics.csv"]
    assert normalised(s) == expected_calls(task, run_dir, plateau)
    assert sum(c[0] == "test" for c in s.calls) == (RAN if task == "seg" else 0)
    log = messages(caplog)
    assert len(log) == RAN + 1 and log[0] == FIRST_LOG[task] and log[RAN - 1].endswith(LAST_LOG_TAIL[task]) and log[RAN] == STOP_LOG


def test_the_loop_runs_every_epoch_when_validation_keeps_improving(tmp_path, monkeypatch):
    monkeypatch.setattr(sys.modules[__name__], "VAL_LOSS", [1.0 / (e + 1) for e in range(EPOCHS)])
    s = Script("cls", monkeypatch)
    rows = s.fit(HalvingScheduler(s.opt, s.calls), str(tmp_path / "run"), False)
    assert [r[0] for r in rows] == list(range(EPOCHS)) and sum(c[0] == "save" for c in s.calls) == EPOCHS


def test_under_data_parallel_only_rank_zero_writes(tmp_path, monkeypatch):
    import torch.distributed as dist
    for rank in (1, 0):
        monkeypatch.setattr(dist, "get_rank", lambda rank=rank: rank)
        s = Script("multi", monkeypatch, distributed=True)
        run_dir = str(tmp_path / f"rank{rank}")
        rows = s.fit(HalvingScheduler(s.opt, s.calls), run_dir, True)
        assert rows == expected_rows("multi")                                           # every rank returns the rows and stops alike
        assert normalised(s) == expected_calls("multi", run_dir, True, saves=rank == 0)
        assert os.listdir(run_dir) == (["metrics.csv"] if rank == 0 else [])


def refused(tmp_path, monkeypatch, match, step_task, eval_task=None, distributed=(False, False), **kw):
    s = Script(step_task, monkeypatch)
    if eval_task is not None:
        s.eval_step = types.SimpleNamespace(distributed=False, **task_attributes(eval_task))
    s.step.distributed = distributed[0]
    if distributed[1] is None:
        del s.eval_step.distributed
    else:
        s.eval_step.distributed = distributed[1]
    run_dir = str(tmp_path / "never")
    with pytest.raises(ValueError, match=match):
        s.fit(HalvingScheduler(s.opt, s.calls), run_dir, False, **kw)
    assert not os.path.exists(run_dir) and s.calls == []


@pytest.mark.parametrize("step_task, eval_task, match", [
    ("cls", "multi", "both be built on a classification-only model"), ("multi", "cls", "both be built on a classification-only model"),
    ("seg", "multi", "both be built on a segmentation-only model"), ("multi", "seg", "both be built on a segmentation-only model"),
    ("cls", "seg", "both be built on a classification-only model"), ("seg", "cls", "both be built on a classification-only model")])
def test_a_mixed_pair_of_steps_is_refused_before_the_run_directory_exists(step_task, eval_task, match, tmp_path, monkeypatch):
    kw = {"test_step": object(), "test_index": "test-index"}
    refused(tmp_path, monkeypatch, match, step_task, eval_task, **kw)


@pytest.mark.parametrize("kw", [{"test_step": None}, {"test_index": None}, {"test_step": None, "test_index": None}], ids=["step", "index", "both"])
def test_segmentation_without_its_testing_phase_is_refused_before_the_run_directory_exists(kw, tmp_path, monkeypatch):
    refused(tmp_path, monkeypatch, "testing phase after every epoch", "seg", **kw)


@pytest.mark.parametrize("eval_distributed", [False, None], ids=["local", "no attribute"])
def test_data_parallel_training_with_a_local_eval_step_is_refused_before_the_run_directory_exists(eval_distributed, tmp_path, monkeypatch):
    refused(tmp_path, monkeypatch, "the training step is data parallel, the evaluation step is not", "multi", distributed=(True, eval_distributed))
