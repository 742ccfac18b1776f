"""Multi_BTSUNet without a GPU: parameter names, order and bit-identical initial weights against the reference's recorded sha256, the factory,
the plain-torch oracle (tests/bts_oracle.py) against the reference's float64 numbers, the refusals, and the C-ABI additions (the nearest 2x
up-sampling op, the batch-shared Linear's workspace query and switch) with the kernel names mtbc_op_kernel_name gives them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
import bts_oracle as B  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "mt_btsunet_step.npz"))


# ------------------------------------------------------------------------------------------------ parameters and factory
@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_state_dict_names_order_and_initial_weights_are_the_references(fixture, cfg):
    from multi_task_breast_cancer_amd.nets import Multi_BTSUNet
    width, n_classes, ds = B.CONFIGS[cfg]
    seed_everything(1993)
    m = Multi_BTSUNet(1, 1, n_classes, width, ds)
    keys = [str(k) for k in fixture[f"{cfg}.keys"]]
    assert list(m.state_dict()) == keys and len(keys) == (33 if ds else 25)
    assert ("output3.0.weight" in keys) == ("output2.1.bias" in keys) == ds
    assert B.state_sha256(m.state_dict()) == str(fixture[f"{cfg}.sha"])
    assert m.n_classes == (1 if n_classes == 2 else n_classes) and tuple(m.state_dict()["classifier.3.weight"].shape) == (m.n_classes, 256)
    assert tuple(m.state_dict()["classifier.1.weight"].shape) == (256, 8 * width * 256)
    # ... and so are the oracle's: same draws, same initialisation pass
    seed_everything(1993)
    ref = B.OracleMultiBTSUNet(1, 1, n_classes, width, ds)
    assert list(ref.state_dict()) == keys and B.state_sha256(ref.state_dict()) == str(fixture[f"{cfg}.sha"])


def test_factory_builds_the_model_and_honours_width_and_deep_supervision():
    from multi_task_breast_cancer_amd import experiment_init as E
    from multi_task_breast_cancer_amd.nets import Multi_BTSUNet
    m = E.init_multitask_model("Multi_BTSUNet", sequences=1, regions=1, n_classes=3, width=8, deep_supervision=True)
    assert isinstance(m, Multi_BTSUNet) and m.architecture == "Multi_BTSUNet" and m.width == 8 and m.deep_supervision and len(m.state_dict()) == 33
    m = E.init_multitask_model("Multi_BTSUNet", sequences=2, regions=1, n_classes=2, width=16, deep_supervision=False)
    assert m.n_classes == 1 and not m.deep_supervision and len(m.state_dict()) == 25
    assert tuple(m.state_dict()["encoder1.ConvInNormLRelu1.Conv.weight"].shape) == (8, 2, 3, 3)
    cfg_model = {"architecture": "Multi_BTSUNet", "sequences": 1, "width": 8, "deep_supervision": True}
    cfg_opt = {"opt": "Adam", "lr": 1e-3, "scheduler": "cosine", "t_max": 20, "patience": 20, "min_lr": 1e-6, "decrease_factor": 0.5}
    model, opt, seg_c, cls_c, sched = E.load_multitask_experiment_artefacts(
        {"classes": ["benign", "malignant", "normal"], "classes_weighted": None}, cfg_model, cfg_opt,
        {"function": "DICE", "classification_criterion": "Focal"}, 0, None)
    assert isinstance(model, Multi_BTSUNet) and model.width == 8 and model.n_classes == 3
    with pytest.raises(ValueError):
        E.init_multitask_model("BTSUNet")
    with pytest.raises(ValueError):
        Multi_BTSUNet(1, 1, 3, width=7)


def test_refusals_other_input_sizes_and_data_parallel():
    from multi_task_breast_cancer_amd import nets, trainer
    from multi_task_breast_cancer_amd.engine import Act
    for size in ((64, 64), (128, 64), (256, 256)):
        with pytest.raises(ValueError, match="128 x 128"):
            nets._graph_multi_btsunet(None, Act("input", torch.empty(1, 1, *size), needs_grad=False))
    m = nets.Multi_BTSUNet(1, 1, 3, 8, True)
    with pytest.raises(NotImplementedError, match="data parallel"):
        trainer.FusedTrainStep(m, None, alpha=0.35, distributed=True)
    with pytest.raises(NotImplementedError, match="data parallel"):
        trainer.FusedEvalStep(m, alpha=0.35, on_device=True, distributed=True)
    assert not getattr(nets.MTnnUNet, "single_device_only", False)


# ------------------------------------------------------------------------------------------------ the oracle against the reference's numbers
@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_oracle_reproduces_the_reference_fixture(fixture, cfg):
    """The oracle in float64 against the reference's float64 run: the same arithmetic in the same library, so 1e-9 (absolute, on O(1)
    values) is rounding-order slack only; gradients 1e-9 relative per tensor."""
    width, n_classes, ds = B.CONFIGS[cfg]
    torch.set_num_threads(8)
    seed_everything(1993)
    ref = B.OracleMultiBTSUNet(1, 1, n_classes, width, ds).double()
    img = torch.from_numpy(fixture["image"]).double()
    mask = torch.from_numpy(fixture["mask"]).double()
    label = torch.from_numpy(fixture["label"])
    label = (label == 1).double().view(-1, 1) if n_classes == 2 else label.view(-1, 1).double()
    total, seg, cls, logits, outs = O.train_step(ref, O.make_adam(ref, 1e-4), img, mask, label, B.ALPHA, True, n_classes)
    heads = outs if isinstance(outs, list) else [outs]
    logits = logits[0] if isinstance(logits, list) else logits
    assert isinstance(outs, list) == ds and len(heads) == (3 if ds else 1)
    assert (logits.detach() - torch.from_numpy(fixture[f"{cfg}.logits"])).abs().max().item() < 1e-9
    want = torch.from_numpy(fixture[f"{cfg}.losses"])
    assert (torch.stack([total, seg, cls]) - want).abs().max().item() < 1e-9
    for i, h in enumerate(heads):
        idx = B.sample_index(h.numel(), 100 + i)
        assert (h.detach().reshape(-1)[idx] - torch.from_numpy(fixture[f"{cfg}.head{i}"])).abs().max().item() < 1e-9, i
        assert (h.detach().sum(dim=(1, 2, 3)) - torch.from_numpy(fixture[f"{cfg}.head{i}_sum"])).abs().max().item() < 1e-6, i
    grads = dict(ref.named_parameters())
    for j, k in enumerate(B.GRAD_TENSORS):
        g64 = torch.from_numpy(fixture[f"{cfg}.grad.{k}"])
        got = grads[k].grad.reshape(-1)[B.sample_index(grads[k].numel(), 200 + j)]
        assert ((got - g64).norm() / g64.norm()).item() < 1e-9, k


# ------------------------------------------------------------------------------------------------ the C-ABI additions
def test_header_exports_enum_and_mirrors_are_consistent(lib, tmp_path):
    src = open(HEADER).read()
    for name in ("mtbc_upsample2_fwd", "mtbc_upsample2_bwd", "mtbc_linear_workspace", "mtbc_linear_wide_enable"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.mtbc_version() == 203 == L.ABI_VERSION
    second = src[src.index("MTBC_OP_SOFTMAX = 37"):]
    second = second[:second.index("};")]
    assert re.search(r"MTBC_OP_UPSAMPLE2_FWD\s*=\s*38", second) and re.search(r"MTBC_OP_UPSAMPLE2_BWD\s*=\s*39", second)
    assert (L.OP_SOFTMAX, L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD) == (37, 38, 39)
    assert L.OP_UNION_FIELD[L.OP_UPSAMPLE2_FWD] == L.OP_UNION_FIELD[L.OP_UPSAMPLE2_BWD] == "up2"
    assert int(re.search(r"#define\s+MTBC_LINEAR_WIDE_MIN_IN\s+(\d+)", src).group(1)) == L.LINEAR_WIDE_MIN_IN >= 4096
    fields = ["N", "C", "H", "W", "x", "x_batch_stride", "y", "y_batch_stride", "layout", "type16", "dy", "dy_batch_stride", "dx", "dx_batch_stride",
              "accumulate_dx"]
    assert [f for f, _ in L.Upsample2Args._fields_] == fields
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(mtbc_upsample2_args));', 'printf("op %zu\\n", sizeof(mtbc_op));',
             'printf("linear %zu\\n", sizeof(mtbc_linear_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbc_upsample2_args, {f}));' for f in fields]
    (tmp_path / "l.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(L.Upsample2Args) and int(got["op"]) == C.sizeof(L.Op) and int(got["linear"]) == C.sizeof(L.LinearArgs)
    for f in fields:
        assert int(got[f]) == getattr(L.Upsample2Args, f).offset, f


def test_upsample2_kernel_names_and_refusals(lib):
    from multi_task_breast_cancer_amd import ops
    F_, B_ = L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD
    name = lambda *a, **k: ops.op_kernel_name(ops.upsample2_case_args(*a, **k))      # noqa: E731
    assert name(F_, 2, 16, 16, 16) == "upsample2_fwd_kernel" and name(B_, 2, 16, 16, 16) == "upsample2_bwd_kernel"
    assert name(B_, 2, 16, 16, 16, acc_dx=True) == "upsample2_bwd_kernel"
    assert name(F_, 1, 5, 3, 5) == "upsample2_fwd_scalar_kernel" and name(B_, 1, 5, 3, 5) == "upsample2_bwd_scalar_kernel"        # W % 4 != 0
    assert name(F_, 2, 8, 8, 8, strides=dict(x=8 * 64 + 2)) == "upsample2_fwd_scalar_kernel"                                     # a stride float4 cannot take
    assert name(F_, 2, 8, 8, 8, strides=dict(y=4 * 8 * 64 + 2)) == "upsample2_fwd_scalar_kernel"
    assert name(B_, 2, 8, 8, 8, strides=dict(dx=8 * 64 + 2)) == "upsample2_bwd_scalar_kernel"
    for c in (1, 2):
        assert name(F_, 2, 8, 4, 4, compute=c) == name(F_, 3, 24, 8, 12, compute=c) == "upsample2_c8_fwd_kernel"      # bf16 and fp16: one kernel
    buf = C.create_string_buffer(512)
    rc = lambda op: lib.mtbc_op_kernel_name(C.byref(op), buf, 512)      # noqa: E731
    assert rc(ops.upsample2_case_args(F_, 2, 12, 4, 4, compute=1)) == -1                   # channel groups of 8
    assert rc(ops.upsample2_case_args(F_, 0, 8, 4, 4)) == -1
    assert rc(ops.upsample2_case_args(F_, 2, 8, 4, 4, compute=1, strides=dict(x=8 * 16 + 4))) == -5      # a pixel's 8 channels would straddle 16 bytes
    op = ops.upsample2_case_args(F_, 2, 8, 4, 4)
    op.u.up2.y = None
    assert rc(op) == -2
    op = ops.upsample2_case_args(B_, 2, 8, 4, 4)
    op.u.up2.dx += 4                                                                        # pointer values count: a misaligned dx takes the scalar kernel
    assert rc(op) == 0 and buf.value == b"upsample2_bwd_scalar_kernel"
    op.u.up2.accumulate_dx = 2
    assert rc(op) == -2
    assert L.OP_UPSAMPLE2_FWD in ops.SMALL_OPS and L.OP_UPSAMPLE2_BWD in ops.SMALL_OPS


_WIDE_F = "linear_wide_fwd_kernel + linear_wide_reduce_kernel"


def test_linear_threshold_from_both_sides_and_the_old_shapes_keep_their_kernels(lib):
    from multi_task_breast_cancer_amd import ops
    import test_abi_cpu as A
    F_, B_ = L.OP_LINEAR_FWD, L.OP_LINEAR_BWD
    T = L.LINEAR_WIDE_MIN_IN
    name = lambda *a, **k: ops.op_kernel_name(ops.linear_case_args(*a, **k))      # noqa: E731
    assert name(F_, 2, T, 32, relu=True) == _WIDE_F
    assert name(F_, 2, T - 4, 32, relu=True) == "linear_fwd_kernel"                        # just below
    assert name(F_, 2, T + 2, 32) == "linear_fwd_kernel"                                    # In % 4 != 0
    assert name(B_, 2, T - 4, 32) == "linear_dx_kernel [Out>=8] + linear_dw_kernel"
    assert name(B_, 2, T, 32) == "linear_wide_dx_kernel + linear_wide_dx_reduce_kernel + linear_dw_kernel"
    assert name(B_, 9, T, 8, relu=True) == "linear_mask_kernel + linear_wide_dx_kernel + linear_dw_kernel [N>=8]"      # Out < 32: one range of outputs, no reduction
    assert name(B_, 2, 8192, 256, dx=False) == "linear_dw_kernel"                           # no input gradient: nothing batch-shared to run
    assert name(B_, 2, 49152, 256, relu=True) == "linear_mask_kernel + linear_wide_dx_kernel + linear_wide_dx_reduce_kernel + linear_dw_kernel"
    op = ops.linear_case_args(F_, 2, T, 32)
    op.u.linear.w += 4                                                                      # rows that are not 16-byte aligned: the per-sample kernel
    assert ops.op_kernel_name(op) == "linear_fwd_kernel"
    # the workspace: what the query says, refused when absent or a float short
    buf = C.create_string_buffer(512)
    rc = lambda op: lib.mtbc_op_kernel_name(C.byref(op), buf, 512)      # noqa: E731
    for kind, shape, kw in ((F_, (2, 8192, 256), {}), (B_, (2, 8192, 256), dict(relu=True)), (B_, (65, 8192, 32), {})):
        op = ops.linear_case_args(kind, *shape, **kw)
        need = lib.mtbc_linear_workspace(C.byref(op.u.linear), int(kind == B_))
        assert op.u.linear.workspace_bytes == need > 0 and rc(op) == 0
        op.u.linear.workspace_bytes -= 4
        assert rc(op) == -3
        assert rc(ops.linear_case_args(kind, *shape, workspace=False, **kw)) == -3
    assert lib.mtbc_linear_workspace(C.byref(ops.linear_case_args(B_, 16, 512, 256, relu=True).u.linear), 1) == 16 * 256 * 4      # as before
    assert lib.mtbc_linear_workspace(C.byref(ops.linear_case_args(B_, 16, 512, 256).u.linear), 1) == 0
    assert lib.mtbc_linear_workspace(C.byref(ops.linear_case_args(F_, 16, 512, 256).u.linear), 0) == 0
    # every Linear row of the frozen selection table (In <= 512) names what it named
    rows = [r for r in A.SMALL_OP_SELECTION if r[0] == "linear"]
    assert len(rows) >= 7
    for helper, kind, shape, mode, want in rows:
        assert shape[1] < T and "wide" not in want
        assert ops.op_kernel_name(ops.linear_case_args(kind, *shape, **mode)) == want
    # the switch: off, a wide shape makes the per-sample launches and asks for their workspace
    assert ops.linear_wide(False) is True
    try:
        assert name(F_, 2, 8192, 256, relu=True) == "linear_fwd_kernel"
        assert name(B_, 16, 8192, 256, relu=True) == "linear_mask_kernel + linear_dx_kernel [Out>=8] + linear_dw_kernel [N>=8]"
        assert lib.mtbc_linear_workspace(C.byref(ops.linear_case_args(B_, 16, 8192, 256, relu=True).u.linear), 1) == 16 * 256 * 4
        assert lib.mtbc_linear_workspace(C.byref(ops.linear_case_args(F_, 16, 8192, 256).u.linear), 0) == 0
    finally:
        assert ops.linear_wide(True) is False
    assert name(F_, 2, 8192, 256, relu=True) == _WIDE_F
