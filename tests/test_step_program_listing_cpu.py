# tests/golden/step_program_listing.json was generated from the package of the PARENT commit of the change that made engine.StepPlan.maxpool /
# convT / convT_head / conv1x1 / gap / linear call the fillers of ops.py -- commit 93bd3bd01e022b8c9a77b08546afde3503782af1, whose emitters
# wrote every field by hand -- NOT from the code under test:
#     python tools/step_program_listing.py --package <a copy of that commit's multi_task_breast_cancer_amd> --short
# It holds, per configuration and program, one string per op: the kind and a digest of the op's canonical fields (pointers as buffer
# ordinal + byte offset).  A change that means to alter a step program regenerates it from its own tree and says so.
# Planes above 64 x 64 in the 16-bit modes ask the runtime how many InstanceNorm teams can be resident (norm_coop.hip resident_blocks): with no
# device visible the answer is none and the plan takes the one-plane kernels, on an MI355X it takes the cooperative ones.  The six 128 x 128
# configurations this touches are in the golden twice: `label` from a machine without a device, `label@device` from the same command (CPU
# tensors all the same) on a machine with an MI355X; the test compares with the one that fits where it runs.
"""Whole step programs, built on CPU tensors (host-only library queries, nothing launched), are op for op and field for field what the golden
listing pins: tools/step_program_listing.py.  A plan built on CPU tensors differs from a device plan in one known place: the InstanceNorm
parameter-gradient reductions are deferred on a device only."""
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

CONFIGS = T._cpu_set()
SIX = {"pool", "conv1", "gap", "linear", "convT", "head"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "step_program_listing.json")) as f:
        return json.load(f)


_BUILT = {}


def _built(config):
    """label -> ({program: (kind, canonical fields) per op}, the combinations of the six families it reaches); each configuration is built once."""
    if config[0] not in _BUILT:
        model, step = T.build(nets, config, "cpu")
        canon = T.Canon(model, step)
        _BUILT[config[0]] = ({name: T.op_lines(L, canon, step.programs[name]) for name in T.PROGRAMS},
                             set().union(*(T.combos(L, step.programs[name]) for name in T.PROGRAMS)))
    return _BUILT[config[0]]


def _want(golden, label):
    on_device = label + "@device"
    return golden[on_device if on_device in golden and torch.cuda.is_available() else label]


def test_the_golden_lists_exactly_the_configurations(golden):
    assert sorted(k for k in golden if "@" not in k) == sorted(c[0] for c in CONFIGS)
    assert {k.split("@")[0] for k in golden if "@" in k} <= {c[0] for c in CONFIGS if c[5] > 64 and c[3] != "f32"}
    assert all(sorted(programs) == sorted(T.PROGRAMS) for programs in golden.values())


@pytest.mark.parametrize("config", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_step_programs_are_the_golden_listing(config, golden):
    listing, _ = _built(config)
    for name in T.PROGRAMS:
        lines = listing[name]
        got, want = T.short(lines), _want(golden, config[0])[name]
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                print(f"{config[0]} {name} op #{i}: {lines[i][1]}")
                pytest.fail(f"{config[0]} {name}: op #{i} is {g}, the golden has {w} (its fields are printed above)")
        assert len(got) == len(want), f"{config[0]} {name}: {len(got)} ops, the golden has {len(want)}"


def test_the_set_reaches_every_variant_of_the_six_families():
    """Among the configurations: every op kind of the pool, 1x1, GAP, Linear, ConvT and fused-head
    families, channel-blocked and planar, a folded and a launched pool, the rank-1 head and the launched 1x1 backward, the 16-bit ConvT
    backward with and without 16-bit dy."""
    reached = set().union(*(_built(c)[1] for c in CONFIGS))
    print("\n".join(" ".join(str(v) for v in c) for c in sorted(reached)))
    kinds = {k for k, member in L.OP_UNION_FIELD.items() if member in SIX}
    assert kinds <= {c[0] for c in reached}, sorted(kinds - {c[0] for c in reached})
    has = lambda kind, *flags: any(c[0] == kind and set(flags) <= set(c) for c in reached)         # noqa: E731
    for kind, planar, blocked in ((L.OP_CONV1_FWD, "x_layout=0", "x_layout=1"), (L.OP_CONV1_WGRAD, "x_layout=0", "x_layout=1"),
                                  (L.OP_CONV1_DGRAD, "x_layout=0", "x_layout=1"), (L.OP_CONVT_FWD, "y_layout=0", "y_layout=1")):
        assert has(kind, planar) and has(kind, blocked), kind
    # the channel-blocked pool: folded into the InstanceNorm ops wherever the plan has the streaming pass; launched (both directions) only in the
    # 128 x 128 plans of a machine without a device, which fall back to the one-plane InstanceNorm kernels
    assert has(L.OP_POOL_FWD, "layout=0") and has(L.OP_POOL_BWD, "layout=0")
    assert (has(L.OP_POOL_FWD, "layout=1") and has(L.OP_POOL_BWD, "layout=1")) or torch.cuda.is_available()
    assert has(L.OP_IN_FWD, "pool_y8=True", "pool_arg=True") and has(L.OP_IN_BWD, "dy_pool=True") and has(L.OP_IN_BWD, "dy_rank1=True")
    assert has(L.OP_POOL_BWD, "acc_dx=0") and has(L.OP_POOL_BWD, "acc_dx=1")
    for kind in (L.OP_CONVT_WGRAD, L.OP_CONVT_DGRAD):
        assert has(kind, "compute=0") and has(kind, "compute=1", "dy16=0") and has(kind, "compute=1", "dy16=1") and has(kind, "compute=2", "dy16=2"), kind
    assert has(L.OP_CONVT_WGRAD, "x16=1") and has(L.OP_CONVT_WGRAD, "x16=2") and has(L.OP_CONVT_DGRAD, "acc_dx=1")
    assert has(L.OP_LINEAR_FWD, "relu=0") and has(L.OP_LINEAR_FWD, "relu=1", "ws=True") and has(L.OP_LINEAR_BWD, "relu=0") and has(L.OP_LINEAR_BWD, "relu=1")
