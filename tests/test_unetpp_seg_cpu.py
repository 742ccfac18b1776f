"""The single-task U-Net++ segmentation model (`architecture: UnetPlusPlus`, nets.BasicUnetPlusPlus) without a GPU: the factory, the state-dict
layout and the initial weights against MTUNetPlusPlus's trunk, the constructor's refusals, the never-trained heads' place in the flat buffers,
the oracle wrapper of tests/unetpp_seg_oracle.py against oracle.torch_oracle.OracleMTUNetPlusPlus, and the step programs of the three modes
planned on CPU tensors (nothing is launched)."""
import inspect
import os
import sys

import pytest
import torch

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import experiment_init as EI  # noqa: E402
from multi_task_breast_cancer_amd import inference as INF  # noqa: E402
from multi_task_breast_cancer_amd import nets  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import unetpp_seg_oracle as U  # noqa: E402

WIDTHS = [(32, 32, 64, 128, 256, 32), nets.UNETPP_FEATURES]          # MONAI's default, MTUNetPlusPlus's
SIX = [f"final_conv_0_{j}.{p}" for j in (1, 2, 3) for p in ("weight", "bias")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


# ------------------------------------------------------------------------------------------------ factory
def test_init_segmentation_model_builds_the_model(tmp_path):
    model = EI.init_segmentation_model("UnetPlusPlus", sequences=3, regions=1, width=48, save_folder=tmp_path / "run", deep_supervision=True)
    assert type(model) is nets.BasicUnetPlusPlus and model.architecture == "UnetPlusPlus" and model.n_classes == 0
    assert model.in_channels == 3 and model.deep_supervision and model.features == (32, 32, 64, 128, 256, 32) == nets.BASIC_UNETPP_FEATURES
    assert "conv_0_0" in (tmp_path / "run" / "model.txt").read_text()
    assert model.state_dict()["conv_0_0.conv_0.conv.weight"].shape == (32, 3, 3, 3)
    plain = EI.init_segmentation_model("UnetPlusPlus", sequences=1, regions=2)           # `width` plays no part, deep supervision defaults to off
    assert not plain.deep_supervision and plain.state_dict()["final_conv_0_4.weight"].shape == (2, 32, 1, 1)
    assert EI.init_segmentation_model("UnetPlusPlus", width=7).features == plain.features
    assert T.is_seg_only(model) and not T.is_cls_only(model) and T.task_of(model) is T.SEGMENTATION
    assert list(inspect.signature(EI.init_segmentation_model).parameters) == ["architecture", "sequences", "regions", "width", "save_folder",
                                                                              "deep_supervision"]


def test_every_other_name_stays_refused():
    for name in ("BTSUNet", "UNet", "AttentionUNet", "ResidualUNet", "SwinUNETR", "SegResNet", "MTUNetPlusPlus", "UNetPlusPlusClassifier",
                 "BasicUnetPlusPlus", "unetplusplus", ""):
        with pytest.raises(ValueError, match="'nnUNet' or 'UnetPlusPlus'"):
            EI.init_segmentation_model(name)
    for factory in (EI.init_multitask_model, EI.init_classification_model):
        with pytest.raises(ValueError):
            factory("UnetPlusPlus")


@pytest.mark.parametrize("opt,kind", [("Adam", FusedAdam), ("SGD", FusedSGD), ("AdamW", FusedAdamW)])
def test_load_segmentation_experiment_artefacts_takes_the_name(opt, kind):
    cm = {"architecture": "UnetPlusPlus", "sequences": 1, "width": 48, "deep_supervision": True, "compute_dtype": "bf16"}
    co = {"opt": opt, "lr": 1e-4, "scheduler": "cosine", "t_max": 20, "patience": 7, "min_lr": 1e-6, "decrease_factor": 0.5}
    model, optimizer, criterion, sched = EI.load_segmentation_experiment_artefacts(cm, co, {"function": "DICE"}, 2, None, fused=True)
    assert type(model) is nets.BasicUnetPlusPlus and model.in_channels == 3 and model.deep_supervision and model.compute == 1
    assert isinstance(optimizer, kind) and isinstance(sched, torch.optim.lr_scheduler.CosineAnnealingLR)
    assert optimizer.state_dict()["state"] == {}


# ------------------------------------------------------------------------------------------------ parameters
@pytest.mark.parametrize("features", WIDTHS, ids=["monai", "mt"])
@pytest.mark.parametrize("ds", [True, False])
def test_state_dict_is_the_trunk_of_mtunetplusplus(features, ds):
    sd = nets.BasicUnetPlusPlus(2, 2, 1, features, ds).state_dict()
    mt = list(nets.MTUNetPlusPlus(2, 2, 1, 3, ds).state_dict())
    assert list(sd) == mt[:mt.index("process_level_3.convs.conv_0.conv.weight")]
    assert list(sd)[-8:] == [f"final_conv_0_{j}.{p}" for j in (1, 2, 3, 4) for p in ("weight", "bias")]
    assert len([k for k in sd if k.startswith("upcat_") and k.endswith("deconv.weight")]) == 10
    f = features
    assert sd["conv_4_0.convs.conv_1.conv.weight"].shape == (f[4], f[4], 3, 3) and sd["upcat_0_4.convs.conv_0.conv.weight"].shape == (f[5], 4 * f[0] + f[1], 3, 3)
    assert sd["upcat_3_1.upsample.deconv.weight"].shape == (f[4], f[4] // 2, 2, 2) and sd["upcat_0_1.upsample.deconv.weight"].shape == (f[1], f[1], 2, 2)


@pytest.mark.parametrize("ds", [True, False])
def test_initial_trunk_weights_are_mtunetplusplus_bit_for_bit(ds):
    seed_everything(1993)
    seg = nets.BasicUnetPlusPlus(2, 1, 1, nets.UNETPP_FEATURES, ds).state_dict()
    seed_everything(1993)
    mt = nets.MTUNetPlusPlus(2, 1, 1, 3, ds).state_dict()
    for k, v in seg.items():
        assert torch.equal(v, mt[k]), k


def test_initial_weights_at_the_default_widths_are_the_oracle_wrappers():
    """The product's draw against the restatement's (tests/unetpp_seg_oracle.py): the same names, order and values for the same seed, and the
    hash that file records for ITS draw.  Nothing of the reference pins this model (MONAI is not installed)."""
    seed_everything(1993)
    prod = nets.BasicUnetPlusPlus(deep_supervision=True).state_dict()
    O.seed_everything(1993)
    ref = U.OracleBasicUnetPlusPlus(1, 1, U.FEATURES, True).state_dict()
    assert list(prod) == list(ref) and all(torch.equal(prod[k], ref[k]) for k in ref)
    assert U.sha256_of(prod) == U.sha256_of(ref) == U.INIT_SHA256


def test_constructor_refusals():
    with pytest.raises(ValueError, match="spatial_dims"):
        nets.BasicUnetPlusPlus(spatial_dims=3)
    for bad in ((32, 32, 64, 128, 256), (32, 32, 64, 128, 256, 32, 32), (32, 32, 64, 128, 256, 0), (32, 32, 64, 128, -256, 32),
                (32.0, 32, 64, 128, 256, 32), (32, 32, 64, 128, 256, True), ()):
        with pytest.raises(ValueError, match="six positive integers"):
            nets.BasicUnetPlusPlus(features=bad)
    for bad in ((32, 32, 64, 128, 256, 12), (36, 32, 64, 128, 256, 32), (32, 32, 64, 100, 256, 32), (1, 2, 3, 4, 5, 6)):
        with pytest.raises(ValueError, match="multiple of 8"):
            nets.BasicUnetPlusPlus(features=bad)
    assert nets.BasicUnetPlusPlus(features=[8, 8, 16, 24, 40, 8]).features == (8, 8, 16, 24, 40, 8)


def test_never_trained_heads_lie_behind_the_live_prefix():
    model = nets.BasicUnetPlusPlus(deep_supervision=False)
    assert sorted(model.untrained) == sorted(SIX) == sorted(nets.UNETPP_SEG_UNTRAINED)
    live = [model.slots[n] for n in model._order if n not in model.untrained]
    dead = [model.slots[n] for n in model._order if n in model.untrained]
    assert [s.offset for s in live] == sorted(s.offset for s in live) and live[0].offset == 0
    assert all(s.offset + s.numel <= model.live_numel for s in live) and all(s.offset >= model.live_numel for s in dead)
    assert model.live_numel % 4 == 0 and model.live_numel < model.flat_numel and max(s.offset + s.numel for s in dead) <= model.flat_numel
    assert list(model.state_dict()) == list(nets.BasicUnetPlusPlus(deep_supervision=True).state_dict())          # the names keep their order
    with_ds = nets.BasicUnetPlusPlus(deep_supervision=True)
    offs = [with_ds.slots[n].offset for n in with_ds._order]
    assert not with_ds.untrained and with_ds.live_numel == with_ds.flat_numel and offs == sorted(offs)
    for other in (nets.MTUNetPlusPlus(), nets.MTUNetPlusPlus(deep_supervision=True), nets.UNetPlusPlusClassifier()):       # as they were
        assert not other.untrained and other.live_numel == other.flat_numel


# ------------------------------------------------------------------------------------------------ the oracle wrapper
@pytest.mark.parametrize("ds", [True, False])
def test_oracle_wrapper_heads_are_the_multitask_oracles(ds):
    """For the same weights the wrapper's float32 heads are OracleMTUNetPlusPlus's, bit for bit (the same modules in the same order)."""
    O.seed_everything(5)
    mt = O.OracleMTUNetPlusPlus(1, 1, 3, ds, U.FEATURES)
    seg = U.OracleBasicUnetPlusPlus(1, 1, U.FEATURES, ds)
    assert not any(k.startswith(("process_level_3", "classifier")) for k in seg.state_dict())
    seg.load_state_dict({k: v for k, v in mt.state_dict().items() if k in seg.state_dict()})
    x = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(3)) * 255
    with torch.no_grad():
        _, want = mt(x)
        got = seg(x)
    assert isinstance(got, list) and len(got) == (4 if ds else 1)
    for g, w in zip(got, want if ds else [want]):
        assert torch.equal(g, w)
    mask = (torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(4)) > 0.6).float()
    assert torch.equal(U.seg_loss(got, mask, True), O.multitask_losses(want if ds else [want], mask, [torch.zeros(2, 3)], torch.eye(3)[:2], True)[0])


# ------------------------------------------------------------------------------------------------ step programs on CPU tensors
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("ds", [True, False], ids=["ds", "nods"])
def test_step_programs_build_on_cpu_tensors(lib, dtype, ds):
    """The four programs of a fused step at 2 x 64 x 64, planned on zeroed CPU buffers (tools/step_program_listing.py's way): no classification
    op, no batch pair, one 1x1 head per trained head, and no op that touches a never-trained parameter."""
    torch.manual_seed(1993)
    model = nets.BasicUnetPlusPlus(deep_supervision=ds)
    model.set_compute(dtype)
    model.flat_p = torch.zeros(model.flat_numel, dtype=torch.float32)
    model.flat_g = torch.zeros_like(model.flat_p)
    st = nets.CompiledStep(model, 2, 64, 64, fused_loss={"alpha": 1.0, "inversely_weighted": True})
    assert st.logits is None and st.onehot is None and len(st.segs) == (4 if ds else 1) and st.segs[-1].name == "final_conv_0_4"
    kinds = {name: [p.array[i].kind for i in range(p.n)] for name, p in st.programs.items()}
    assert all(kinds[name] for name in ("pack", "fwd", "loss", "bwd"))
    everything = [k for ks in kinds.values() for k in ks]
    for absent in (L.OP_LINEAR_FWD, L.OP_LINEAR_BWD, L.OP_GAP_FWD, L.OP_GAP_BWD, L.OP_FOCAL, L.OP_SOFTMAX):
        assert absent not in everything
    assert "process_level_3.in" not in st.plan.acts and not any(n.startswith(("process_level_3", "classifier")) for n in st.plan.acts)
    assert kinds["loss"] == [L.OP_DICE_FWD, L.OP_DICE_BWD, L.OP_LOSS_MIX]
    # nothing is written behind the live prefix: every backward op's parameter gradient lies in [0, live_numel)
    ready = {n: model.slots[n].ready_at for n in model._order}
    assert all(ready[n] < 0 for n in model.untrained) and all(ready[n] >= 0 for n in model._order if n not in model.untrained and not n.endswith("conv.bias"))
    with pytest.raises(ValueError, match="alpha"):
        nets.CompiledStep(model, 2, 64, 64, fused_loss={"alpha": 0.5, "inversely_weighted": True})
    for H, W in ((72, 64), (64, 40)):                     # MONAI would replicate-pad inside UpCat: not planned, refused
        with pytest.raises(ValueError, match="multiples of 16"):
            nets.CompiledStep(model, 2, H, W, fused_loss={"alpha": 1.0, "inversely_weighted": True})


def test_existing_unetpp_models_plan_what_they_planned(lib):
    """The widths argument of the shared parameter and graph functions defaults to nets.UNETPP_FEATURES: MTUNetPlusPlus and
    UNetPlusPlusClassifier keep their op counts (tests/golden/step_program_listing.json holds every field of every op)."""
    for ctor, fused, want_segs in ((lambda: nets.MTUNetPlusPlus(2, 1, 1, 3, deep_supervision=True), {"alpha": 0.5, "inversely_weighted": True}, 4),
                                   (lambda: nets.UNetPlusPlusClassifier(2, 1, 3), {"alpha": 0.0, "inversely_weighted": True}, 0)):
        torch.manual_seed(1993)
        model = ctor()
        model.flat_p = torch.zeros(model.flat_numel, dtype=torch.float32)
        model.flat_g = torch.zeros_like(model.flat_p)
        st = nets.CompiledStep(model, 2, 64, 64, fused_loss=fused)
        assert st.logits is not None and len(st.segs) == want_segs and "process_level_3.in" in st.plan.acts


# ------------------------------------------------------------------------------------------------ host-side refusals of the drivers
def test_refusals_are_host_logic():
    model = nets.BasicUnetPlusPlus(deep_supervision=True)
    opt = FusedAdam(model, lr=1e-4, eps=1e-4)
    for kw in ({"alpha": 0.5}, {"n_classes": 3}, {"cls_criterion": "CE"}):
        with pytest.raises(ValueError):
            T.FusedTrainStep(model, opt, **kw)
        with pytest.raises(ValueError):
            T.FusedEvalStep(model, **kw)
    with pytest.raises(NotImplementedError):
        T.FusedTrainStep(model, opt, distributed=True)
    with pytest.raises(NotImplementedError):
        T.FusedEvalStep(model, on_device=True, distributed=True)
    step = T.FusedTrainStep(model, opt, alpha=1.0, seg_criterion="Jaccard")
    assert step.seg_only and not step.cls_only and step.alpha == 1.0
    assert T.step_task(INF.FusedSegTestStep(model)) is not T.CLASSIFICATION
    with pytest.raises(ValueError):
        INF.FusedClsTestStep(model)
    with pytest.raises(L.MtbcError):
        model(torch.zeros(1, 1, 64, 64))                  # no CPU path
