# tests/golden/conv_cell_listing.json was generated from the package of the PARENT commit of the change that made engine.StepPlan.conv_cell,
# _gathered_dgrad and _conv_cell_backward call the 3x3 convolution and InstanceNorm fillers of ops.py -- commit
# c6dc9afccef9c5ccb1b7d2982ec2123117ed25ad, whose emitters wrote every field of those ops by hand -- NOT from the code under test:
#     python tools/step_program_listing.py --package <a copy of that commit's multi_task_breast_cancer_amd> --set cells --short
# The same short form as tests/golden/step_program_listing.json (tests/test_step_program_listing_cpu.py): per configuration and program one
# string per op, the kind and a digest of the op's canonical fields.  The three 16-bit configurations above 64 x 64 whose plan asks the runtime
# for the InstanceNorm team plan are in it twice: `label` from a machine without a device, `label@device` from the same command (CPU tensors
# all the same) on a machine with an MI355X.  A change that means to alter a step program regenerates it from its own tree and says so.
"""The conv-cell branches that the 28 configurations of tests/golden/step_program_listing.json do not reach -- a first conv of 2 .. 5 channels,
the plan switches of engine.py, force_direct plans, 16-bit gathered activation gradients, the bias cells of the single-task U-Net++,
coop_reserve_cus -- are op for op and field for field what the golden listing pins, and the set reaches each of them (the combinations
tools/step_program_listing.py --set cells --combos lists).  Plans on CPU tensors: a device plan alone reaches the deferred InstanceNorm
parameter-gradient reductions (MTBC_OP_IN_DPARAM, defer_dparams and the op's own workspace), and without a device (no `@device` entry
compared) the cooperative kernels above 64 x 64 -- the channel-blocked z, y8 / dz8 and the folded pool at 128 x 128 -- are not reached either."""
import importlib.util
import json
import os

import pytest
import torch

from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd import nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_program_listing", os.path.join(ROOT, "tools", "step_program_listing.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

CONFIGS = T._cells_set()
F_, D_, W_, NF, NB = L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD, L.OP_IN_FWD, L.OP_IN_BWD


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "conv_cell_listing.json")) as f:
        return json.load(f)


_BUILT = {}


def _built(label):
    """label -> ({program: (kind, canonical fields) per op}, the combinations it reaches); each configuration is built once."""
    if label not in _BUILT:
        config = next(c for c in CONFIGS if c[0] == label)
        model, step = T.build(nets, config, "cpu")
        canon = T.Canon(model, step)
        _BUILT[label] = ({name: T.op_lines(L, canon, step.programs[name]) for name in T.PROGRAMS},
                         set().union(*(T.combos(L, step.programs[name], name) for name in T.PROGRAMS)))
    return _BUILT[label]


def test_the_golden_lists_exactly_the_configurations(golden):
    assert sorted(k for k in golden if "@" not in k) == sorted(c[0] for c in CONFIGS)
    assert {k.split("@")[0] for k in golden if "@" in k} <= {c[0] for c in CONFIGS if c[5] > 64 and c[3] != "f32"}
    assert all(sorted(programs) == sorted(T.PROGRAMS) for programs in golden.values())


def test_a_build_leaves_the_plan_switches_as_they_were():
    from multi_task_breast_cancer_amd import engine
    names = sorted({k for c in CONFIGS for k in c[9]})
    assert names == ["_DA16", "_NO_COOP", "_NO_GATHER", "_NO_STEM_MC", "_NO_Z16", "_Z_BF16"]
    before = {k: getattr(engine, k) for k in names}
    _built("da16-bf16")
    assert {k: getattr(engine, k) for k in names} == before


@pytest.mark.parametrize("label", [c[0] for c in CONFIGS])
def test_step_programs_are_the_golden_listing(label, golden):
    listing, _ = _built(label)
    on_device = label + "@device"
    want = golden[on_device if on_device in golden and torch.cuda.is_available() else label]
    for name in T.PROGRAMS:
        lines = listing[name]
        got = T.short(lines)
        for i, (g, w) in enumerate(zip(got, want[name])):
            if g != w:
                print(f"{label} {name} op #{i}: {lines[i][1]}")
                pytest.fail(f"{label} {name}: op #{i} is {g}, the golden has {w} (its fields are printed above)")
        assert len(got) == len(want[name]), f"{label} {name}: {len(got)} ops, the golden has {len(want[name])}"


def _has(label, kind, *flags):
    return any(c[0] == kind and set(flags) <= set(c) for c in _built(label)[1])


def _kinds(label, program):
    return [kind for kind, _ in _built(label)[0][program]]


def test_the_set_reaches_the_first_conv_of_2_to_5_channels():
    for label, cin in (("stem2-f32", 2), ("stem5-f32", 5)):         # fp32: the direct forward's kernels, the small-Cin weight gradient
        assert _has(label, F_, f"cin={cin}", "compute=0", "force_direct=0", "out_layout=0", "packed=False")
        assert _has(label, W_, f"cin={cin}", "compute=0", "operand_layout=0", "force_direct=0")
        assert not _has(label, D_, f"cin={cin}")                    # (the input needs no gradient)
    for label, cin, compute, zt in (("stem3-bf16", 3, 1, 2), ("stem5-f16", 5, 2, 0)):       # stem16: planar fp32 in, channel-blocked z out + statistics
        assert _has(label, F_, f"cin={cin}", f"compute={compute}", "operand_layout=0", "out_layout=1", f"out_type={zt}", "stats=True", "packed=False")
        assert _has(label, W_, f"cin={cin}", f"compute={compute}", "operand_layout=1")
        assert _has(label, NF, "z_layout=1", f"z_type={zt}", "stats=True")


def test_the_set_reaches_no_stem_mc():
    for label, cin in (("stem3-bf16-nostemmc", 3), ("stem5-bf16-nostemmc", 5), ("stem5-f32-nostemmc", 5)):
        assert _has(label, F_, f"cin={cin}", "compute=0", "force_direct=1", "out_layout=0")       # conv3x3_direct_kernel, fp32 z
        assert _has(label, W_, f"cin={cin}", "compute=0", "operand_layout=0", f"force_direct={int(cin > 4)}")      # Cin = 5: the direct weight gradient
        assert not _has(label, F_, "cin>5", "force_direct=1")


def test_the_set_reaches_force_direct_plans():
    for kind in (F_, D_, W_):
        assert _has("direct-f32", kind, "compute=0", "force_direct=1") and not _has("direct-f32", kind, "force_direct=0")
    assert L.OP_CONV3_PACK_FWD in _kinds("direct-f32", "pack")
    # 16-bit: planar operands all the way, 16-bit planes out of the InstanceNorm for nobody (no channel-blocked copies, no 16-bit outputs)
    for kind in (F_, D_, W_):
        assert _has("direct-bf16", kind, "cin>5", "compute=1", "operand_layout=0", "force_direct=1") and not _has("direct-bf16", kind, "operand_layout=1")
    assert not _has("direct-bf16", NF, "out16=1") and not _has("direct-bf16", NB, "out16=1")


def test_the_set_reaches_the_plan_switches():
    # _NO_COOP / _NO_Z16 at 64 x 64: fp32 z, the one-plane kernels, dz as 16-bit planes + the 16-bit pack
    for label in ("nocoop-bf16", "noz16-bf16"):
        assert _has(label, F_, "operand_layout=1", "out_layout=0", "stats=False") and not _has(label, F_, "out_layout=1")
        assert not _has(label, NF, "z_layout=1") and _has(label, NB, "out=dz+dz16", "out16=1") and not _has(label, NB, "out=dz+dz8")
        assert L.OP_C8_PACK16 in _kinds(label, "bwd")
    # ... above 256 x 256: dz in place over dy, fp32, and the fp32 pack behind it; the chunked-statistics workspace forward
    assert _has("nocoop-bf16-512", NB, "out=dz", "out16=0") and L.OP_C8_PACK in _kinds("nocoop-bf16-512", "bwd")
    assert _has("nocoop-bf16-512", NF, "ws=True") and _has("nocoop-f16-128", NB, "out=dz+dz16", "out16=2")
    # _NO_Z16 at 128 x 128: with a device the cooperative kernels on fp32 z (y8 forward); without one the one-plane kernels
    if torch.cuda.is_available():
        assert _has("noz16-f16-128", NF, "z_layout=0", "out16=2", "out=y8") or _has("noz16-f16-128", NF, "z_layout=0", "out16=2", "out=y+y8")
    assert not _has("noz16-f16-128", NF, "z_layout=1")
    # _NO_GATHER: no forward-type op in the backward program, every input gradient by its own cell's dgrad (a skip accumulated beside the
    # 16-bit planes for the transposed convolution)
    assert not _has("nogather-bf16", F_, "in=bwd") and _has("nogather-bf16", D_, "operand_layout=1", "seg_acc=12")
    assert _has("da16-bf16", F_, "in=bwd") and _has("stem3-bf16", F_, "in=bwd", "out_acc=0") and _has("stem3-bf16", F_, "in=bwd", "out_acc=1")
    # _Z_BF16: z in bf16 under a bf16 output (z_type 0 = the output's type), where the default stores fp16 (stem3-bf16 above)
    assert _has("zbf16-bf16", F_, "out_layout=1", "out_type=0") and not _has("zbf16-bf16", F_, "out_type=2")
    assert _has("zbf16-bf16", NF, "z_layout=1", "z_type=0", "out16=1") and not _has("zbf16-bf16", NB, "z_type=2")


def test_the_set_reaches_16_bit_gathered_activation_gradients():
    for label, compute in (("da16-bf16", 1), ("da16-f16-nn", 2), ("da16-bf16-bts-128", 1)):
        assert _has(label, F_, "in=bwd", f"compute={compute}", "operand_layout=1", "out_layout=1", "out_acc=0")        # the gathered dgrad writes grad8
        assert _has(label, NB, "dy=True", "dy_layout=1", "n_extra=0", "out=dz8")
    assert _has("da16-bf16", NB, "dy_layout=1", "n_extra=1") and _has("da16-f16-nn", NB, "dy_layout=1", "n_extra=1")      # + the other readers' fp32 partial
    assert not _has("stem3-bf16", NB, "dy_layout=1")


def test_the_set_reaches_the_bias_cells_of_the_single_task_unetpp():
    for label in ("UnetPlusPlus-f32-ds", "UnetPlusPlus-f32-nods", "UnetPlusPlus-bf16-ds", "UnetPlusPlus-bf16-nods"):
        assert _has(label, F_, "in=fwd", "bias=True") and not _has(label, F_, "in=fwd", "bias=False")
        assert _has(label, NB, "affine=True", "dbias=True") and not _has(label, NB, "dbias=False")
        convs = [text for kind, text in _built(label)[0]["fwd"] if kind == F_]
        for width in (32, 64, 128, 256):
            assert any(f" Cout={width} " in text for text in convs), (label, width)
    ds, nods = (sum(kind == L.OP_CONV1_FWD for kind in _kinds(f"UnetPlusPlus-f32-{s}", "fwd")) for s in ("ds", "nods"))
    assert (ds, nods) == (4, 1)


def test_the_set_reaches_coop_reserve_cus():
    for label in ("reserve64-bf16", "reserve64-bf16-128"):
        assert _has(label, NF, "reserve=64") and _has(label, NB, "reserve=64") and not _has(label, NF, "reserve=0")
    assert _has("stem3-bf16", NF, "reserve=0")


def test_the_set_reaches_a_cell_without_the_channel_blocked_backward():
    """Multi_BTSUNet of width 20: a first cell of 10 channels (channel-blocked operands forward, planar backward), then a conv of 10 input
    channels that no 16-bit image is packed for."""
    assert _has("bts-w20-bf16-128", F_, "in=fwd", "cin>5", "compute=0", "packed=False", "operand_layout=0")
    assert _has("bts-w20-bf16-128", W_, "compute=1", "operand_layout=0") and _has("bts-w20-bf16-128", W_, "compute=1", "operand_layout=1")
    assert _has("bts-w20-bf16-128", D_, "compute=1", "operand_layout=0", "packed=False")
