"""The single-task segmentation baseline (`nnUNet2021`, BASELINE.json configs[0]) without a GPU: initial weights and state-dict
layout against the reference-pinned golden, the two factories of experiment_init, and the criterion glue's signature."""
import inspect
import os

import numpy as np
import pytest
import torch

from multi_task_breast_cancer_amd import criterions as CR
from multi_task_breast_cancer_amd import experiment_init as EI
from multi_task_breast_cancer_amd import nets
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.optim import FusedAdam
from oracle import torch_oracle as O
from test_oracle_goldens import _sha

CONFIG_MODEL = {"architecture": "nnUNet", "sequences": 1, "width": 48, "deep_supervision": True}
CONFIG_LOSS = {"function": "DICE"}


def config_opt(scheduler):
    return {"opt": "Adam", "lr": 1e-4, "scheduler": scheduler, "t_max": 20, "patience": 7, "min_lr": 1e-6, "decrease_factor": 0.5}


def test_initial_weights_are_the_references(golden_dir):
    g = np.load(os.path.join(golden_dir, "seg_nnunet_step.npz"))
    seed_everything(1993)
    model = nets.nnUNet(1, 1)
    assert _sha(model.state_dict()) == str(g["sha256_init"])
    assert model.architecture == "nnUNet" and model.n_classes == 0 and model.in_channels == 1


def test_state_dict_names_and_order_are_the_oracles():
    model, ref = nets.nnUNet(2, 1), O.OracleSegNnUNet(2, 1)
    got, want = model.state_dict(), ref.state_dict()
    assert list(got) == list(want)
    assert [tuple(v.shape) for v in got.values()] == [tuple(v.shape) for v in want.values()]
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert not any(k.startswith(("classifier", "process_")) for k in got)
    # the trunk of MTnnUNet is this model: same names, same order, in front of the classification head
    mt = list(nets.MTnnUNet(2, 1, 3).state_dict())
    assert mt[:len(got)] == list(got) and all(k.startswith(("classifier", "process_")) for k in mt[len(got):])


def test_init_segmentation_model(tmp_path):
    model = EI.init_segmentation_model("nnUNet", sequences=3, regions=1, width=48, save_folder=tmp_path / "run", deep_supervision=False)
    assert isinstance(model, nets.nnUNet) and model.in_channels == 3
    assert (tmp_path / "run" / "model.txt").exists()
    assert list(inspect.signature(EI.init_segmentation_model).parameters) == ["architecture", "sequences", "regions", "width", "save_folder",
                                                                               "deep_supervision"]
    for name in ("BTSUNet", "MTnnUNet", "UNet", ""):
        with pytest.raises(ValueError):
            EI.init_segmentation_model(name)
    with pytest.raises(ValueError):                    # and the multi-task factory still refuses this one
        EI.init_multitask_model("nnUNet")


@pytest.mark.parametrize("scheduler", ["plateau", "cosine"])
def test_load_segmentation_experiment_artefacts(scheduler):
    out = EI.load_segmentation_experiment_artefacts(CONFIG_MODEL, config_opt(scheduler), CONFIG_LOSS, 2, None, fused=True)
    assert len(out) == 4
    model, optimizer, criterion, sched = out
    assert isinstance(model, nets.nnUNet) and model.in_channels == 3
    assert isinstance(optimizer, FusedAdam)
    assert optimizer.param_groups[0]["eps"] == 1e-4 and optimizer.param_groups[0]["lr"] == 1e-4
    assert isinstance(criterion, CR.DiceLoss)
    want = torch.optim.lr_scheduler.ReduceLROnPlateau if scheduler == "plateau" else torch.optim.lr_scheduler.CosineAnnealingLR
    assert isinstance(sched, want)
    assert list(inspect.signature(EI.load_segmentation_experiment_artefacts).parameters) == [
        "config_model", "config_opt", "config_loss", "n_augments", "run_path", "fused"]


def test_apply_criterion_binary_segmentation_is_the_references_glue():
    assert list(inspect.signature(CR.apply_criterion_binary_segmentation).parameters) == ["criterion", "ground_truth", "segmentation",
                                                                                          "inversely_weighted"]
    crit = lambda s, t: (s - t).abs().mean()      # noqa: E731  (any criterion: the glue is host arithmetic)
    t = torch.zeros(2, 1, 4, 4)
    heads = [torch.full_like(t, v) for v in (4.0, 3.0, 2.0, 1.0)]      # 1/1 + 2/2 + 3/3 + 4/4 from the LAST head backwards
    assert CR.apply_criterion_binary_segmentation(crit, t, heads, True).item() == 4.0
    assert CR.apply_criterion_binary_segmentation(crit, t, heads, False).item() == 10.0
    assert CR.apply_criterion_binary_segmentation(crit, t, heads[0]).item() == 4.0
    with pytest.raises(SystemExit) as e:
        CR.apply_criterion_binary_segmentation(crit, t, [torch.full_like(t, float("nan"))], True)
    assert e.value.code == 1


def test_product_path_has_no_cpu_fallback():
    from multi_task_breast_cancer_amd import _lib as L
    with pytest.raises(L.MtbcError):
        nets.nnUNet(1, 1)(torch.zeros(1, 1, 64, 64))
