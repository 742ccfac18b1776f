"""tests/step_programs.py -- the survey of a step program and the compare-and-report behind the launch-coverage guards of tests/test_ops_gpu.py --
on hand-made programs: the walks that carry state (the ConvT pair, the run of layout ops), the conv3x3, up-sampling and loss keys flag by flag, the session cache and
the failure messages; and the guards of the further models' launch modules (assert_only_tested, assert_rows_needed, table_keys, kernel_instances,
assert_keys_subset, assert_op_kinds_claimed), one test per way each can fail.  mtbc_conv3x3_kernel_name, mtbc_convT_kernel_name and
mtbc_op_kernel_name are host-only, mtbc_instnorm_kernel_name is for one-workgroup launches; no device, no step is built."""
import types

import pytest

import step_programs as SP
from multi_task_breast_cancer_amd import ops
from multi_task_breast_cancer_amd.engine import Program, _mk

L = ops.L
CONVT, LAYOUT, SMALL = "transposed-convolution", "layout", "small-op"


def _convT(kind, N=2, Cin=48, Cout=24, H=8, W=8):
    op = _mk(kind)
    op.u.convT = ops.convT_case_args(kind, N, Cin, Cout, H, W)
    return op


def _pack(kind, Cin=24, Cout=24, dgrad=0, compute=0):
    op = _mk(kind)
    op.u.pack.Cin, op.u.pack.Cout, op.u.pack.dgrad, op.u.pack.compute = Cin, Cout, dgrad, compute
    return op


def _wview(Cout=8, Cin=24, off=16, cnt=8, mode=1, k_off=0, K=40):
    op = _mk(L.OP_CONV3_WVIEW)
    v = op.u.wview
    v.Cout, v.Cin, v.ci_off, v.ci_cnt, v.mode, v.k_off, v.K = Cout, Cin, off, cnt, mode, k_off, K
    return op


def _survey(label, programs, reserve_cus=0, collectors=SP.COLLECTORS, calls=None):
    """The survey of the hand-made step {program name: [op]} under its own cache entry; `calls` receives the arguments of every build."""
    def build(*args):
        if calls is not None:
            calls.append(args)
        step = types.SimpleNamespace(programs=dict({name: Program(oplist, []) for name, oplist in programs.items()}, graph=None))
        return step, None
    return SP.survey(("hand-made", label, 0, 0), reserve_cus, collectors=collectors, build=build)


def _kinds(s, family):
    return sorted(kind for kind, _ in s.seen[family].values())


# ---- the ConvT walk
def test_wgrad_then_dgrad_of_the_same_upconv_is_one_pair():
    wg, dg = _convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)
    s = _survey("pair", {"bwd": [wg, dg]})
    assert s.seen[CONVT] == {("pair", SP._convT_key(wg.u.convT, L.OP_CONVT_WGRAD, dg.u.convT)): ("pair", (2, 48, 24, 8, 8, 2))}
    assert s.kinds == {"bwd": [L.OP_CONVT_WGRAD, L.OP_CONVT_DGRAD], "graph": []}


def test_wgrad_then_dgrad_of_another_upconv_is_two_entries():
    wg, dg = _convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD, Cin=96)
    s = _survey("no pair", {"bwd": [wg, dg]})
    assert s.seen[CONVT] == {("wgrad", SP._convT_key(wg.u.convT, L.OP_CONVT_WGRAD)): ("wgrad", (2, 48, 24, 8, 8, 2)),
                             ("dgrad", SP._convT_key(dg.u.convT, L.OP_CONVT_DGRAD)): ("dgrad", (2, 96, 24, 8, 8, 2))}


def test_wgrad_at_the_end_of_its_program_is_a_wgrad():
    """... also where the next program begins with the DGRAD of the same up-convolution: the runner pairs inside one program only."""
    s = _survey("last op", {"a": [_convT(L.OP_CONVT_FWD), _convT(L.OP_CONVT_WGRAD)], "b": [_convT(L.OP_CONVT_DGRAD)]})
    assert _kinds(s, CONVT) == ["dgrad", "fwd", "wgrad"]


# ---- the layout walk
def test_a_lone_pack_op_is_single():
    s = _survey("lone pack", {"pack": [_convT(L.OP_CONVT_FWD), _pack(L.OP_CONV3_PACK_FWD), _convT(L.OP_CONVT_FWD)]})
    assert s.seen[LAYOUT] == {SP._pack_key(L.OP_CONV3_PACK_FWD, 24, 24, 0, 0, "single"): (L.OP_CONV3_PACK_FWD, (24, 24, 0, 0))}


def test_two_adjacent_pack_ops_are_both_many():
    s = _survey("two packs", {"pack": [_pack(L.OP_CONV3_PACK_FWD), _pack(L.OP_CONV3_PACK_LP, 48, 24, 1, 2)]})
    assert set(s.seen[LAYOUT]) == {SP._pack_key(L.OP_CONV3_PACK_FWD, 24, 24, 0, 0, "many"), SP._pack_key(L.OP_CONV3_PACK_LP, 48, 24, 1, 2, "many")}


def test_a_weight_view_between_two_packs_is_single():
    s = _survey("view between packs", {"pack": [_pack(L.OP_CONV3_PACK_FWD), _wview(), _pack(L.OP_CONV3_PACK_DGRAD, dgrad=1)]})
    assert set(s.seen[LAYOUT]) == {SP._wview_key(8, 24, 16, 8, 1, 0, 40, "single"), SP._pack_key(L.OP_CONV3_PACK_FWD, 24, 24, 0, 0, "single"),
                                   SP._pack_key(L.OP_CONV3_PACK_DGRAD, 24, 24, 1, 0, "single")}
    assert s.seen[LAYOUT][SP._wview_key(8, 24, 16, 8, 1, 0, 40, "single")] == (L.OP_CONV3_WVIEW, (8, 24, 16, 8, 1, 0, 40))


# ---- the conv3x3 key: the full name + the branches the arguments select (hand-made mtbc_conv3x3_args, dummy pointers)
F_, D_, W_ = L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD
_BF = dict(compute=1, c8=True)
_PTR = 77 << 20          # a dummy address for a field the builder left NULL


def _c3(op, N=2, segs=(32,), Cout=32, H=16, W=32, **mode):
    return ops.conv3x3_case_args(op, N, list(segs), Cout, H, W, **mode)


def _flags(op, **kw):
    return SP._conv3_key(_c3(op, **kw), op)[1]


def test_conv3_key_keeps_the_reduction_behind_the_weight_gradient():
    name = lambda **kw: SP._conv3_key(_c3(W_, **kw), W_)[0]                                             # noqa: E731
    assert name(**_BF).endswith("_kernel<false, 0> + splitk_reduce")
    assert name(**_BF, in_kernel_reduce=True).endswith(" + splitk_fixup")
    assert name().endswith(" + splitk_reduce + channel_sums") and name(bias=False).endswith(" + splitk_reduce")
    # one image range on a 16 x 16 map, no dbias, no accumulation: the blocks store straight into dw -- no suffix, another key than with dbias
    direct = dict(_BF, N=1, segs=(64,), Cout=48, H=16, W=16)
    assert " + " not in name(**direct, bias=False) and name(**direct).endswith(" + splitk_reduce")
    assert len({name(**direct, bias=False), name(**direct), name(**direct, bias=False, in_kernel_reduce=True, accumulate_dw=True)}) == 3


@pytest.mark.parametrize("op,flag,without,with_", [
    (F_, "bias", dict(bias=False), dict(bias=True)),
    (F_, "stats", dict(_BF, out_c8=True), dict(_BF, out_c8=True, stats=True)),
    (F_, "out_acc", dict(_BF, bias=False), dict(_BF, bias=False, out_accumulate=True)),
    (F_, "out_partial", dict(_BF, out_c8=True, bias=False, stats=True, norm=0.1), dict(_BF, out_c8=True, bias=False, stats=True, norm=0.1, out_partial=True)),
    (F_, "norm_affine", dict(_BF, out_c8=True, bias=False, stats=True), dict(_BF, out_c8=True, bias=False, stats=True, norm=0.1)),
    (D_, "codes=0,2", dict(_BF, segs=(16, 16), accumulate=[0, 1]), dict(_BF, segs=(16, 16), accumulate=[0, 2])),
    (D_, "codes=3", dict(_BF, segs=(16, 16), accumulate=[0, 0]), dict(_BF, segs=(16, 16), dx_c8=True)),
    (D_, "codes=1", dict(accumulate=[0]), dict(accumulate=[1])),
    (W_, "dbias", dict(_BF, bias=False), dict(_BF, bias=True)),
    (W_, "acc_dw", dict(_BF, bias=False), dict(_BF, bias=False, accumulate_dw=True)),
    (W_, "acc_dw", dict(bias=False), dict(bias=False, accumulate_dw=True)),
    (F_, "segs>1", dict(_BF), dict(_BF, segs=(16, 16))),
    (D_, "segs>1", dict(_BF), dict(_BF, segs=(16, 16))),
    (W_, "segs>1", dict(), dict(segs=(16, 16))),
    (F_, "straddle", dict(_BF, segs=(32, 32)), dict(_BF, segs=(24, 40))),               # a 32-channel chunk of the 16-bit MFMA reads two segments
    (W_, "straddle", dict(_BF, segs=(32, 32)), dict(_BF, segs=(24, 40))),
    (F_, "straddle", dict(segs=(8, 24)), dict(segs=(12, 20))),                          # ... an 8-channel chunk of the fp32 kernels
    (D_, "straddle", dict(_BF, segs=(16, 32)), dict(_BF, segs=(24, 24))),               # a 16-row tile writes two segments
    (F_, "ragged_rows", dict(_BF), dict(_BF, Cout=24)),
    (D_, "ragged_rows", dict(_BF, segs=(48,)), dict(_BF, segs=(40,))),
    (W_, "ragged_rows", dict(), dict(Cout=40)),
    (F_, "ragged_k", dict(_BF, segs=(64,)), dict(_BF, segs=(48,))),
    (F_, "ragged_k", dict(segs=(16,)), dict(segs=(12,))),
    (D_, "ragged_k", dict(_BF, Cout=64), dict(_BF, Cout=48)),
    (F_, "force_direct", dict(), dict(force_direct=True)),
    (D_, "force_direct", dict(), dict(force_direct=True)),
    (W_, "force_direct", dict(), dict(force_direct=True)),
])
def test_conv3_key_flag_follows_the_arguments(op, flag, without, with_):
    a, b = _flags(op, **without), _flags(op, **with_)
    assert flag not in a and flag in b and a != b, (a, b)


def test_conv3_key_norm_plain_and_strided():
    a = _c3(F_, **_BF, out_c8=True, bias=False, stats=True, norm=0.1)
    a.norm_gamma = a.norm_beta = None
    assert "norm_plain" in SP._conv3_key(a, F_)[1] and "norm_affine" not in SP._conv3_key(a, F_)[1]
    for op in (F_, D_, W_):
        a = _c3(op, **_BF, segs=(16, 16))
        dense = SP._conv3_key(a, op)
        a.in_[1].batch_stride += 8 * 16 * 32          # a channel-range view of a wider tensor
        assert "strided" not in dense[1] and SP._conv3_key(a, op)[1] == dense[1] + ("strided",)


@pytest.mark.parametrize("op,fields", [
    (F_, ("dbias", "dw", "dout", "accumulate_dw", "wgrad_sync")),
    (D_, ("bias", "dbias", "dw", "out", "accumulate_dw", "out_accumulate", "stats_partial", "out_partial", "norm_z")),
    (W_, ("bias", "out", "out_accumulate", "stats_partial", "out_partial", "norm_z")),
])
def test_conv3_key_ignores_fields_the_call_does_not_read(op, fields):
    for mode in (_BF, {}):
        want = SP._conv3_key(_c3(op, **mode), op)
        for name in fields:
            a = _c3(op, **mode)
            setattr(a, name, 1 if name.startswith("accumulate") or name == "out_accumulate" else _PTR)
            assert SP._conv3_key(a, op) == want, (op, mode, name)
    # channel-blocked operands: the dispatch never looks at force_direct
    for op in (F_, D_, W_):
        assert _flags(op, **_BF, force_direct=True) == _flags(op, **_BF)


def test_conv3_collector_keys_by_kind_and_arguments_and_names_the_segments():
    wg, fw = _mk(W_), _mk(F_)
    wg.u.conv3, fw.u.conv3 = _c3(W_, **_BF, segs=(16, 16), bias=False), _c3(F_, **_BF, segs=(16, 16), bias=False)
    s = _survey("conv3", {"fwd": [fw], "bwd": [wg, wg]})
    assert s.seen["conv3x3"] == {(F_, SP._conv3_key(fw.u.conv3, F_)): (F_, (2, 32, 32, 16, 32, (16, 16))),
                                 (W_, SP._conv3_key(wg.u.conv3, W_)): (W_, (2, 32, 32, 16, 32, (16, 16)))}
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested("conv3x3", {(F_, SP._conv3_key(fw.u.conv3, F_))}, [s], required=(F_, W_))
    assert "splitk_reduce" in str(e.value) and "segs>1" in str(e.value) and "(2, 32, 32, 16, 32, (16, 16))" in str(e.value)
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested("conv3x3", set(s.seen["conv3x3"]), [s], required=(F_, D_, W_))
    assert f"[{D_}]" in str(e.value)


# ---- the weight-gradient plan key: the full name + the class of the plan mtbc_conv3x3_wgrad_plan reports (host only, dummy pointers)
PLAN = "conv3x3-wgrad-plan"
_WB = dict(compute=1, c8=True, bias=False)


def _plan(N, segs, Cout, H, W, **mode):
    return SP._wgrad_plan_key(ops.conv3x3_case_args(W_, N, list(segs), Cout, H, W, **mode))


@pytest.mark.parametrize("flag,without,with_", [
    # the tile-walking kernels: 32 x 32 channel blocks (bf16, channel-blocked) ...
    ("even", (3, (192, 192), 192, 44, 64, _WB), (8, (48,), 96, 128, 128, _WB)),             # 66 tiles in 14 splits of 5 | 1024 tiles dealt over 168 splits
    ("fixed", (8, (48,), 96, 128, 128, _WB), (3, (192, 192), 192, 44, 64, _WB)),
    ("tiles=1", (4, (96,), 96, 64, 64, _WB), (3, (24,), 24, 20, 48, _WB)),                  # 128 tiles in 64 splits | 30 tiles in 30 splits
    ("tiles=2", (3, (24,), 24, 20, 48, _WB), (4, (96,), 96, 64, 64, _WB)),
    ("tiles>=3", (4, (96,), 96, 64, 64, _WB), (3, (192, 192), 192, 44, 64, _WB)),
    ("ragged", (4, (96,), 96, 64, 64, _WB), (3, (192, 192), 192, 44, 64, _WB)),             # 13 splits of 5 tiles and one of 1
    ("ragged", (32, (840,), 8, 64, 64, _WB), (8, (48,), 96, 128, 128, _WB)),                # dealt evenly: 1024 / 32 | 1024 / 168 = 6 or 7
    ("crosses", (4, (96,), 96, 64, 64, _WB), (3, (192, 192), 192, 44, 64, _WB)),            # 22 tiles an image in shares of 5
    # ... and the fp32 kernel on 8 x 8 maps: a tile is two images
    ("odd_N", (2, (192,), 192, 8, 8, dict(bias=False)), (3, (192,), 192, 8, 8, dict(bias=False))),
    # the wide-block kernel
    ("segs=1", (8, (24, 24, 24), 24, 20, 128, _WB), (8, (192,), 96, 20, 384, _WB)),         # 96 strips fill the block budget: one block per strip
    ("segs>1", (8, (192,), 96, 20, 384, _WB), (8, (24, 24, 24), 24, 20, 128, _WB)),
    ("short_last_seg", (8, (24, 24, 24), 24, 256, 256, _WB), (8, (24, 24, 24), 24, 20, 128, _WB)),       # 5 steps in segments of 2
    ("img8", (3, (24, 24, 48), 24, 20, 128, _WB), (8, (24, 24, 24), 24, 20, 128, _WB)),
    ("steps>=ring", (8, (24, 24, 24), 24, 20, 128, _WB), (8, (24, 24, 24), 24, 256, 256, _WB)),
    ("steps<ring", (8, (24, 24, 24), 24, 256, 256, _WB), (8, (24, 24, 24), 24, 20, 128, _WB)),
    ("ciblocks>1", (3, (32, 32), 32, 20, 128, _WB), (3, (24, 24, 48), 24, 20, 128, _WB)),
    ("ragged_cit", (3, (24, 24, 48), 24, 20, 128, _WB), (3, (24, 24, 24, 24, 48), 24, 20, 128, _WB)),      # 9 input tiles in blocks of 5 and 4
    # the image-tile kernel
    ("images=1", (16, (384,), 384, 16, 16, _WB), (3, (384,), 384, 16, 16, _WB)),
    ("images=2", (3, (384,), 384, 16, 16, _WB), (3, (512,), 512, 16, 16, _WB)),
    ("images>=3", (3, (384,), 384, 16, 16, _WB), (16, (384,), 384, 16, 16, _WB)),           # 16 images in 6 ranges of 3: the last one 1
    ("short_last_range", (3, (384,), 384, 16, 16, _WB), (16, (384,), 384, 16, 16, _WB)),
    ("ciblocks>1", (5, (64,), 40, 16, 16, _WB), (3, (384,), 384, 16, 16, _WB)),
    # the stem, the small-Cin kernel, the direct kernel
    ("bands=1", (3, (1,), 24, 128, 128, _WB), (3, (1,), 24, 20, 48, _WB)),
    ("bands=4", (3, (1,), 24, 20, 48, _WB), (3, (1,), 24, 128, 128, _WB)),
    ("bands=16", (3, (1,), 24, 128, 128, _WB), (2, (1,), 24, 256, 256, _WB)),
    ("bands=4", (3, (1,), 24, 20, 48, dict(bias=False)), (4, (1,), 24, 256, 256, dict(bias=False))),
    ("images>1", (8, (7,), 8, 8, 8, dict(bias=False)), (24, (7,), 8, 8, 8, dict(bias=False))),
    # the reduction
    ("store", (12, (384, 384, 384), 512, 16, 16, dict(compute=1, c8=True)), (12, (384, 384, 384), 512, 16, 16, _WB)),
    ("fixup levels=2", (2, (192,), 192, 32, 32, _WB), (2, (192,), 192, 32, 32, dict(_WB, in_kernel_reduce=True))),
    ("fixup levels=3", (2, (192,), 192, 32, 32, dict(_WB, in_kernel_reduce=True)), (8, (48,), 96, 128, 128, dict(_WB, in_kernel_reduce=True))),
    ("fixup ragged_group", (2, (192,), 192, 32, 32, dict(_WB, in_kernel_reduce=True)), (3, (192, 192), 192, 44, 64, dict(_WB, in_kernel_reduce=True))),      # 16 | 14 leaves in groups of 4
    ("splitk_reduce<4> x2+x1", (8, (48,), 96, 128, 128, _WB), (3, (192, 192), 192, 44, 64, _WB)),          # 14 splits | 168
    ("splitk_reduce<16> x8+x2+x1", (3, (192, 192), 192, 44, 64, _WB), (8, (48,), 96, 128, 128, _WB)),
    ("splitk_reduce<64, 16> x8", (3, (1,), 24, 128, 128, _WB), (32, (1,), 8, 128, 512, _WB)),              # 512 splits of 72 floats
])
def test_wgrad_plan_key_flag_follows_the_arguments(flag, without, with_):
    a, b = _plan(*without[:5], **without[5]), _plan(*with_[:5], **with_[5])
    assert a[0].split("<")[0] == b[0].split("<")[0], (a, b)          # the same kernel family: the class is what differs
    assert flag not in a[1] and flag in b[1], (a, b)


def test_splitk_reduce_phases_are_the_loops_of_the_kernel():
    ph = SP._splitk_reduce_phases
    assert ph(1, 4) == ["x1"] and ph(4, 4) == ["x1"] and ph(5, 4) == ["x2", "x1"] and ph(8, 4) == ["x2"]
    assert ph(28, 4) == ["x2", "x1"] and ph(29, 4) == ["x8", "x2", "x1"] and ph(32, 4) == ["x8"]          # the first round of 8 rows: nsplit > 7 G
    assert ph(112, 16) == ["x2", "x1"] and ph(128, 16) == ["x8"] and ph(168, 16) == ["x8", "x2", "x1"] and ph(512, 64) == ["x8"]


def test_wgrad_plan_key_carries_the_name_and_not_the_argument_flags():
    name, flags = _plan(3, (24, 24, 48), 24, 20, 128, **_WB)
    assert name == "conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce" == SP._conv3_key(_c3(W_, N=3, segs=(24, 24, 48), Cout=24, H=20, W=128, **_WB), W_)[0]
    assert flags == ("segs>1", "short_last_seg", "steps<ring", "ciblocks>1", "splitk_reduce<16> x2+x1")
    # segments, strides and the accumulate flag are _conv3_key's business: the plan reads none of them
    assert _plan(3, (96,), 24, 20, 128, **_WB) == (name, flags) == _plan(3, (24, 24, 48), 24, 20, 128, **_WB, accumulate_dw=True)
    a = ops.conv3x3_case_args(W_, 3, [24, 24, 48], 24, 20, 128, **_WB)
    a.in_[1].batch_stride += 8 * 20 * 128
    assert SP._wgrad_plan_key(a) == (name, flags)


def test_wgrad_plan_key_raises_on_a_kernel_family_it_does_not_know(monkeypatch):
    monkeypatch.setattr(ops, "conv3x3_kernel_name", lambda a, op: "conv3x3_wgrad_new_kernel<1> + splitk_reduce")
    with pytest.raises(AssertionError, match="does not know the kernel family"):
        _plan(3, (24,), 24, 20, 48, **_WB)


def test_wgrad_plan_collector_keys_every_wgrad_op_once_and_the_message_names_program_key_and_shape():
    big, small, fw = _mk(W_), _mk(W_), _mk(F_)
    big.u.conv3, small.u.conv3 = _c3(W_, N=8, segs=(48,), Cout=96, H=128, W=128, **_WB), _c3(W_, N=3, segs=(16, 8), Cout=24, H=20, W=48, **_WB)
    fw.u.conv3 = _c3(F_, **_BF, bias=False)
    s = _survey("wgrad plan", {"fwd": [fw], "bwd": [big, small, small]})
    kb, ks = (W_, SP._wgrad_plan_key(big.u.conv3)), (W_, SP._wgrad_plan_key(small.u.conv3))
    assert s.seen[PLAN] == {kb: (W_, (8, 48, 96, 128, 128, (48,))), ks: (W_, (3, 24, 24, 20, 48, (16, 8)))}
    assert s.launches[PLAN] == {kb: [(8, 48, 96, 128, 128, (48,))], ks: [(3, 24, 24, 20, 48, (16, 8))] * 2}          # every op under exactly one key
    assert kb[1][1][0] == "even" and ks[1][1][:2] == ("fixed", "tiles=1") and kb[1][0] == ks[1][0]          # one kernel instance, two plans
    SP.assert_all_tested(PLAN, {kb, ks}, [s], required=(W_,), answers={kb: "TABLE_A", ks: "TABLE_B"})
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested(PLAN, {ks}, [s], required=(W_,))
    msg = str(e.value)
    assert "('hand-made', 'wgrad plan', 0, 0)" in msg and "'even', 'tiles>=3', 'ragged'" in msg and "(8, 48, 96, 128, 128, (48,))" in msg
    assert "tiles=1" not in msg


def test_wgrad_plan_listing_names_every_launch_and_its_table(capsys):
    wg = _mk(W_)
    wg.u.conv3 = _c3(W_, N=3, segs=(24,), Cout=24, H=20, W=48, **_WB)
    s = _survey("wgrad listing", {"bwd": [wg, wg]})
    key = (W_, SP._wgrad_plan_key(wg.u.conv3))
    SP.assert_all_tested(PLAN, {key}, [s], answers={key: "CONV3_STEP_CASES"})
    out = capsys.readouterr().out
    assert "<- CONV3_STEP_CASES" in out and out.count("at (3, 24, 24, 20, 48, (24,))") == 2


# ---- the nearest 2x up-sampling key: the launch string + the strided tensors + acc_dx (hand-made ops, dummy pointers)
UF_, UB_ = L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD
_UP = (3, 24, 8, 12)          # N, C, H, W of the input: dense x / dx = 2304 elements an image, y / dy = 9216


def _up2(kind, shape=_UP, **kw):
    return SP._small_op_key(ops.upsample2_case_args(kind, *shape, **kw))


def test_up2_key_is_the_launch_string_of_the_dispatcher():
    assert _up2(UF_) == ("upsample2_fwd_kernel", ()) and _up2(UB_) == ("upsample2_bwd_kernel", ())
    assert _up2(UF_, (1, 5, 3, 5)) == ("upsample2_fwd_scalar_kernel", ()) and _up2(UB_, (1, 5, 3, 5)) == ("upsample2_bwd_scalar_kernel", ())
    assert _up2(UF_, compute=1) == _up2(UF_, compute=2) == ("upsample2_c8_fwd_kernel", ())          # one kernel: the type is never looked at


@pytest.mark.parametrize("kind,flag,with_", [
    (UF_, "x_strided", dict(strides=dict(x=2304 + 16 * 96))),
    (UF_, "y_strided", dict(strides=dict(y=9216 + 16 * 384))),
    (UF_, "x_strided", dict(compute=1, strides=dict(x=2304 + 16 * 96))),                 # channel-blocked: strides in 16-bit elements
    (UF_, "y_strided", dict(compute=2, strides=dict(y=9216 + 16 * 384))),
    (UB_, "dy_strided", dict(strides=dict(dy=9216 + 16 * 384))),
    (UB_, "dx_strided", dict(strides=dict(dx=2304 + 16 * 96))),
    (UB_, "acc_dx", dict(acc_dx=True)),
])
def test_up2_key_flag_follows_the_arguments(kind, flag, with_):
    mode = {k: v for k, v in with_.items() if k == "compute"}
    a, b = _up2(kind, **mode), _up2(kind, **with_)
    assert a[0] == b[0] and a[1] == () and b[1] == (flag,), (a, b)


def test_up2_key_holds_every_flag_at_once_and_ignores_fields_the_call_does_not_read():
    assert _up2(UF_, compute=1, strides=dict(x=4608, y=18432)) == ("upsample2_c8_fwd_kernel", ("x_strided", "y_strided"))
    assert _up2(UB_, acc_dx=True, strides=dict(dy=18432, dx=4608)) == ("upsample2_bwd_kernel", ("dy_strided", "dx_strided", "acc_dx"))
    fwd, bwd = ops.upsample2_case_args(UF_, *_UP), ops.upsample2_case_args(UB_, *_UP)
    want_f, want_b = SP._small_op_key(fwd), SP._small_op_key(bwd)
    fwd.u.up2.accumulate_dx, fwd.u.up2.dy_batch_stride, fwd.u.up2.dx_batch_stride = 1, 5, 5        # the forward reads none of the backward's fields
    bwd.u.up2.x_batch_stride, bwd.u.up2.y_batch_stride, bwd.u.up2.layout, bwd.u.up2.type16 = 5, 5, L.LAYOUT_C8, 1        # ... and the reverse
    assert SP._small_op_key(fwd) == want_f and SP._small_op_key(bwd) == want_b


def test_up2_ops_are_surveyed_with_their_shape():
    fwd, bwd = ops.upsample2_case_args(UF_, *_UP, compute=1, strides=dict(y=18432)), ops.upsample2_case_args(UB_, *_UP, acc_dx=True)
    s = _survey("up2", {"fwd": [fwd], "bwd": [bwd, bwd]})
    assert s.seen[SMALL] == {(UF_, ("upsample2_c8_fwd_kernel", ("y_strided",))): (UF_, _UP), (UB_, ("upsample2_bwd_kernel", ("acc_dx",))): (UB_, _UP)}


# ---- the loss key: the launch string + the branches the arguments select (ops of the structs' fillers, dummy pointers)
DF_, DB_, FO_ = L.OP_DICE_FWD, L.OP_DICE_BWD, L.OP_FOCAL
_DICE = (4, 2, 1, 16, 16)          # n_heads, N, C, H, W


def _dice(kind, shape=_DICE, **kw):
    return SP._loss_key(ops.dice_case_args(kind, *shape, **kw))


def _focal(shape=(8, 3), **kw):
    return SP._loss_key(ops.focal_case_args(*shape, **kw))


def _softmax(N, Cc, backward):
    op = _mk(L.OP_SOFTMAX)
    ops.softmax_args(N, Cc, backward, x=1 << 20, p=2 << 20, dp=3 << 20, dz=4 << 20, into=op.u.softmax)
    return op


def _mix():
    op = _mk(L.OP_LOSS_MIX)
    op.u.mix.seg, op.u.mix.cls, op.u.mix.alpha, op.u.mix.out4 = 1 << 20, 2 << 20, 0.5, 3 << 20
    return op


def test_loss_key_is_the_launch_string_and_the_argument_flags():
    assert _dice(DF_) == ("dice_stats_kernel<0> [threads=256 paths=vvvv rounds=0 rest part] + dice_finalize_kernel<0>", ("kind=0", "n_heads=4"))
    assert _dice(DB_, gscale_dev=True, seg_kind=L.SEG_JACCARD, shape=(1, 2, 3, 16, 16)) == \
        ("dice_bwd_kernel<3> [paths=v]", ("kind=3", "n_heads=1", "gscale_dev", "C>1"))
    assert _focal() == ("focal_kernel", ("C=3", "dx", "gamma>=1"))
    assert _focal((300, 1), gamma=0.0, weight=True, gscale_dev=True) == ("focal_kernel [N>256]", ("C=1", "weight", "dx", "gscale_dev", "gamma=0"))
    assert SP._loss_key(_softmax(5, 3, False)) == ("softmax_rows_kernel", ("fwd", "C=3"))
    assert SP._loss_key(_softmax(70, 2, True)) == ("softmax_rows_kernel [N>64]", ("bwd", "C=2"))
    assert SP._loss_key(_mix()) == ("loss_mix_kernel", ())


@pytest.mark.parametrize("make,flag,without,with_", [
    (lambda **kw: _dice(DB_, **kw), "gscale_dev", dict(), dict(gscale_dev=True)),
    (lambda **kw: _dice(DB_, **kw), "kind=2", dict(), dict(seg_kind=L.SEG_FOCALDICE)),
    (lambda **kw: _dice(DF_, **kw), "kind=1", dict(), dict(seg_kind=L.SEG_BCE)),
    (lambda **kw: _dice(DF_, **kw), "n_heads=3", dict(), dict(shape=(3, 2, 1, 16, 16))),
    (lambda **kw: _dice(DF_, **kw), "C>1", dict(), dict(shape=(4, 2, 2, 16, 16))),
    (lambda **kw: _dice(DB_, **kw), "C>1", dict(), dict(shape=(4, 1, 3, 16, 16))),
    (lambda **kw: _focal(**kw), "C=1", dict(gamma=0.0), dict(gamma=0.0, shape=(8, 1))),
    (lambda **kw: _focal(**kw), "weight", dict(), dict(weight=True)),
    (lambda **kw: _focal(**kw), "dx", dict(dx=False), dict()),
    (lambda **kw: _focal(**kw), "gscale_dev", dict(), dict(gscale_dev=True)),
    (lambda **kw: _focal(**kw), "gamma=0", dict(), dict(gamma=0.0)),
    (lambda **kw: _focal(**kw), "0<gamma<1", dict(), dict(gamma=0.5)),
    (lambda **kw: _focal(**kw), "gamma>=1", dict(gamma=0.999), dict(gamma=1.0)),
    (lambda backward=False, Cc=3: SP._loss_key(_softmax(5, Cc, backward)), "bwd", dict(), dict(backward=True)),
    (lambda backward=False, Cc=3: SP._loss_key(_softmax(5, Cc, backward)), "C=2", dict(), dict(Cc=2)),
])
def test_loss_key_flag_follows_the_arguments(make, flag, without, with_):
    a, b = make(**without), make(**with_)
    assert flag not in a[1] and flag in b[1] and a != b, (a, b)


def test_loss_key_ignores_fields_the_call_does_not_read():
    """The forward reads neither gscale_dev nor gscale nor dx; focal_gamma is read by the FocalDICE kind alone, and there as a value; smooth
    and the head weights are values; Focal reads gscale_dev only where it writes a gradient."""
    fwd = ops.dice_case_args(DF_, *_DICE)
    want = SP._loss_key(fwd)
    fwd.u.dice.gscale_dev, fwd.u.dice.gscale = 77 << 20, 3.0
    fwd.u.dice.dx[0] = (78 << 20) + 4                      # misaligned, even
    assert SP._loss_key(fwd) == want
    for kind in (DF_, DB_):
        for seg_kind in (L.SEG_DICE, L.SEG_BCE, L.SEG_FOCALDICE, L.SEG_JACCARD):
            op = ops.dice_case_args(kind, *_DICE, seg_kind=seg_kind, gscale_dev=True)
            want = SP._loss_key(op)
            op.u.dice.focal_gamma, op.u.dice.smooth_nr, op.u.dice.smooth_dr, op.u.dice.gscale = 0.5, 0.25, 0.125, 7.0
            op.u.dice.head_weight[2] = 9.0
            assert SP._loss_key(op) == want, (kind, seg_kind)
    assert _focal(dx=False, gscale_dev=True) == _focal(dx=False)
    assert _focal(alpha=0.25, gscale=3.0) == _focal()


def test_loss_ops_are_surveyed_with_their_shape():
    fwd, bwd = ops.dice_case_args(DF_, *_DICE), ops.dice_case_args(DB_, *_DICE, gscale_dev=True)
    foc, sm = ops.focal_case_args(8, 3, gscale_dev=True), _softmax(8, 3, False)
    s = _survey("loss", {"fwd": [sm], "loss": [fwd, bwd, foc, _mix()], "bwd": [_softmax(8, 3, True)]})
    assert s.seen["loss"] == {(DF_, SP._loss_key(fwd)): (DF_, _DICE), (DB_, SP._loss_key(bwd)): (DB_, _DICE), (FO_, SP._loss_key(foc)): (FO_, (8, 3)),
                              (L.OP_LOSS_MIX, ("loss_mix_kernel", ())): (L.OP_LOSS_MIX, ()),
                              (L.OP_SOFTMAX, ("softmax_rows_kernel", ("fwd", "C=3"))): (L.OP_SOFTMAX, (8, 3)),
                              (L.OP_SOFTMAX, ("softmax_rows_kernel", ("bwd", "C=3"))): (L.OP_SOFTMAX, (8, 3))}
    assert not s.seen[SMALL] and _plain(s.seen)
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested("loss", set(s.seen["loss"]) - {(DB_, SP._loss_key(bwd))}, [s], required=(DF_, DB_, FO_, L.OP_LOSS_MIX))
    assert "dice_bwd_kernel<0>" in str(e.value) and "gscale_dev" in str(e.value) and str(_DICE) in str(e.value)


def test_loss_fillers_fill_what_the_engine_filled_by_hand():
    """ops.dice_case_args / focal_case_args with into= leave in a program op, byte for byte, what engine.StepPlan.fused_losses and _focal_op
    wrote field by field before the fillers existed (restated here)."""
    import ctypes as C

    import torch
    nh, N, C_, H, W = 4, 2, 1, 16, 16
    heads, grads = [torch.empty(8) for _ in range(nh)], [torch.empty(8) for _ in range(nh)]
    mask, stats, loss, gw = (torch.empty(8) for _ in range(4))
    weights = [1.0 / (nh - i) for i in range(nh)]
    ptrs = {"x": heads, "dx": grads, "target": mask, "stats": stats, "loss": loss, "gscale_dev": gw}
    for name, (seg_kind, nr, dr, gamma, _) in L.SEG_CRITERIA.items():
        for kind in (DF_, DB_):
            want = _mk(kind)
            a = want.u.dice
            a.n_heads, a.N, a.C, a.H, a.W, a.smooth_nr, a.smooth_dr = nh, N, C_, H, W, nr, dr
            a.kind, a.focal_gamma = seg_kind, gamma
            for i in range(nh):
                a.x[i] = heads[i].data_ptr()
                a.head_weight[i] = weights[i]
            a.target, a.stats, a.loss = mask.data_ptr(), stats.data_ptr(), loss.data_ptr()
            if kind == DB_:
                for i in range(nh):
                    a.dx[i] = grads[i].data_ptr()
                a.gscale_dev = gw.data_ptr()
                a.gscale = 0.5 * 65536.0
            got = _mk(kind)
            ops.dice_case_args(kind, nh, N, C_, H, W, ptrs=ptrs, seg_kind=seg_kind, weights=weights, smooth=(nr, dr), focal_gamma=gamma,
                               gscale=0.5 * 65536.0, gscale_dev=True, into=got.u.dice)
            assert bytes(got) == bytes(want), (name, kind)
    x, onehot, fl, dx = (torch.empty(8) for _ in range(4))
    for Cc, gamma, fw in ((3, 2.0, None), (3, 0.0, None), (3, 2.0, torch.empty(3)), (1, 0.0, None)):
        want = _mk(FO_)
        a = want.u.focal
        a.N, a.C, a.alpha, a.gamma = N, Cc, 1.0, gamma
        a.x, a.target, a.weight = x.data_ptr(), onehot.data_ptr(), None if fw is None else fw.data_ptr()
        a.loss, a.dx, a.gscale = fl.data_ptr(), dx.data_ptr(), 0.65
        a.gscale_dev = gw.data_ptr()
        got = _mk(FO_)
        ops.focal_case_args(N, Cc, ptrs={"x": x, "target": onehot, "weight": fw, "loss": fl, "dx": dx, "gscale_dev": gw}, alpha=1.0, gamma=gamma,
                            weight=fw is not None, gscale=0.65, gscale_dev=True, into=got.u.focal)
        assert bytes(got) == bytes(want), (Cc, gamma, fw is not None)
    assert C.sizeof(L.Op) == len(bytes(got))


# ---- what a survey keeps, and for how long
def _plain(v):
    if isinstance(v, (tuple, list)):
        return all(_plain(x) for x in v)
    if isinstance(v, dict):
        return all(_plain(k) and _plain(x) for k, x in v.items())
    return v is None or type(v) in (str, int, bool)


def test_a_survey_holds_plain_values_of_every_family():
    gap = ops.gap_case_args(L.OP_GAP_FWD, 2, 8, 4, 4)
    s = _survey("plain", {"fwd": [gap, _convT(L.OP_CONVT_FWD), _pack(L.OP_CONV3_PACK_FWD), gap]})
    assert s.seen[SMALL] == {(L.OP_GAP_FWD, SP._small_op_key(gap)): (L.OP_GAP_FWD, (2, 8, 4, 4))}
    assert set(s.seen) == set(SP.COLLECTORS) and not s.seen["conv3x3"] and not s.seen["InstanceNorm"]
    assert _plain(s.kinds) and _plain(s.seen) and _plain(s.program), s


def test_survey_builds_once_per_program_and_reserve():
    calls, programs = [], {"bwd": [_convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)]}
    first = _survey("cache", programs, calls=calls)
    assert _survey("cache", programs, calls=calls) is first
    assert _survey("cache", programs, collectors={CONVT: SP.collect_convT}, calls=calls) is first
    assert calls == [("hand-made", "cache", 0, 0, 0)]
    other = _survey("cache", programs, reserve_cus=64, calls=calls)
    assert other is not first and other.reserve_cus == 64 and calls[1:] == [("hand-made", "cache", 0, 0, 64)]
    assert _survey("cache", programs, reserve_cus=64, calls=calls) is other and len(calls) == 2


# ---- compare-and-report
def test_report_names_a_missing_key_with_program_kind_key_and_where():
    s = _survey("report: missing", {"bwd": [_convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)]})
    (key, (kind, where)), = s.seen[CONVT].items()
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested(CONVT, set(), [s])
    msg = str(e.value)
    assert "no reference case" in msg
    for part in (str(s.program), f" {kind} ", str(key), str(where)):
        assert part in msg, (part, msg)


def test_report_names_the_program_without_a_required_kind():
    whole = _survey("report: whole", {"fwd": [_convT(L.OP_CONVT_FWD)], "bwd": [_convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)]})
    half = _survey("report: half", {"bwd": [_convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)]})
    tested = set(whole.seen[CONVT])
    with pytest.raises(AssertionError) as e:
        SP.assert_all_tested(CONVT, tested, [whole, half], required=("fwd", "pair"))
    assert str(half.program) in str(e.value) and "fwd" in str(e.value) and str(whole.program) not in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:          # a program without any launch of the family
        SP.assert_all_tested(LAYOUT, set(), [half])
    assert str(half.program) in str(e.value)


def test_report_passes_when_every_key_is_tested():
    whole = _survey("report: whole", {"fwd": [_convT(L.OP_CONVT_FWD)], "bwd": [_convT(L.OP_CONVT_WGRAD), _convT(L.OP_CONVT_DGRAD)]})
    SP.assert_all_tested(CONVT, set(whole.seen[CONVT]) | {("fwd", "another key")}, [whole], required=("fwd", "pair"))


# ---- the guards of a further model's launch module, on a hand-made program with one launch of every family and hand-made tables
_FP = dict(compute=2, out="c8", z="c8", affine=False)          # the fp16 mode without affine parameters: one-workgroup launches at 12 x 20


def _whole(label, without=()):
    """The survey of a hand-made step with a launch of every family but those of `without`."""
    wg, norm = _mk(W_), _mk(L.OP_IN_BWD)
    wg.u.conv3 = _c3(W_, **_WB)
    ops.instnorm_case_args(True, 2, 16, 12, 20, **_FP, into=norm.u.inorm)
    made = {"conv3x3": wg, "InstanceNorm": norm, CONVT: _convT(L.OP_CONVT_FWD), SMALL: ops.gap_case_args(L.OP_GAP_FWD, 2, 8, 4, 4),
            LAYOUT: _pack(L.OP_CONV3_PACK_FWD), "loss": ops.dice_case_args(DF_, *_DICE)}
    s = _survey(label, {"fwd": [op for family, op in made.items() if family not in without]})
    assert all(bool(s.seen[family]) == (family not in without and not (family == PLAN and "conv3x3" in without)) for family in SP.COLLECTORS)
    return s


def _older(s, but=()):
    """{family: the keys the survey saw}, the families of `but` empty: older tables that answer for everything else."""
    return {family: set() if family in but else set(seen) for family, seen in s.seen.items()}


def _rows(**made):
    """{family: {key: [row]}} over every family, as table_keys gives it."""
    return {family: dict(made.get(family, {})) for family in SP.COLLECTORS}


def _only(s, family):
    (key, (kind, where)), = s.seen[family].items()
    return key, kind, where


def test_only_tested_passes_and_names_the_row_that_answers(capsys):
    s = _whole("guard: passes")
    key, kind, where = _only(s, CONVT)
    SP.assert_only_tested(s, _older(s, but=[CONVT]), _rows(**{CONVT: {key: [("fwd", "row A"), ("fwd", "row B")]}}))
    out = capsys.readouterr().out
    assert f"{s.program} {CONVT}: 1 keys, 0 tested by tests/test_ops_gpu.py's tables, 1 by the rows added for this model, 0 missing\n" in out
    assert f"  {kind} {key} at {where}  <- row ('fwd', 'row A')\n" in out
    assert f"{s.program} loss: 1 keys, 1 tested by tests/test_loss_launches_gpu.py's tables, 0 by the rows added for this model, 0 missing\n" in out
    assert out.count("<- tests/test_ops_gpu.py\n") == 5 and out.count("<- tests/test_loss_launches_gpu.py\n") == 1 and "MISSING" not in out


def test_only_tested_names_a_launch_in_no_table_with_family_kind_key_and_where(capsys):
    s = _whole("guard: missing")
    key, kind, where = _only(s, CONVT)
    with pytest.raises(AssertionError) as e:
        SP.assert_only_tested(s, _older(s, but=[CONVT]), _rows())
    assert str(e.value) == f"launches of {s.program} that no reference case makes:\n  {CONVT}: {kind} {key} at {where}"
    assert f"  {kind} {key} at {where}  <- MISSING\n" in capsys.readouterr().out


def test_only_tested_names_a_family_without_a_launch():
    s = _whole("guard: no layout op", without=[LAYOUT])
    with pytest.raises(AssertionError) as e:
        SP.assert_only_tested(s, _older(s), _rows())
    assert str(e.value) == f"{s.program}: no {LAYOUT} launch found"


def test_only_tested_attributes_a_borrowed_key_to_its_file(capsys):
    s = _whole("guard: borrowed")
    key, kind, where = _only(s, SMALL)
    SP.assert_only_tested(s, _older(s, but=[SMALL]), _rows(), borrowed={SMALL: {key}}, borrowed_from="tests/test_of_the_model_gpu.py")
    out = capsys.readouterr().out
    assert f"  {kind} {key} at {where}  <- tests/test_of_the_model_gpu.py\n" in out and "1 by the rows added for this model, 0 missing" in out
    with pytest.raises(AssertionError, match="no reference case"):          # ... and to nothing without it
        SP.assert_only_tested(s, _older(s, but=[SMALL]), _rows())


def test_rows_needed_passes_for_one_row_per_launched_key_no_older_table_makes():
    s = _whole("guard: rows")
    row, view = ("fwd", "row A"), ("a view", 1)
    own = _rows(**{CONVT: {_only(s, CONVT)[0]: [row]}, LAYOUT: {_only(s, LAYOUT)[0]: [view], "a key of the other path": [view]}})
    SP.assert_rows_needed("the tables", [s], _older(s, but=[CONVT, LAYOUT]), own, [[row], [view]])          # one of a row's keys is enough
    with pytest.raises(AssertionError):          # every family, as table_keys gives them
        SP.assert_rows_needed("the tables", [s], _older(s, but=[CONVT, LAYOUT]), {CONVT: own[CONVT]}, [[row]])


def _rows_needed_message(label, keys, tables, older_has=False):
    s = _whole(label)
    with pytest.raises(AssertionError) as e:
        SP.assert_rows_needed("the tables", [s], _older(s, but=[] if older_has else [CONVT]), _rows(**{CONVT: keys(_only(s, CONVT)[0])}), tables)
    assert str(e.value).startswith("rows of the tables that are not needed:\n"), str(e.value)
    return str(e.value)


def test_rows_needed_reports_a_row_whose_key_no_program_launches():
    row, dead = ("fwd", "row A"), ("fwd", "a dead row")
    msg = _rows_needed_message("guard: dead row", lambda key: {key: [row], ("fwd", "another key"): [dead]}, [[row, dead]])
    assert f"{CONVT}: no program launches ('fwd', 'another key') of row {dead}" in msg and "row A" not in msg and "already" not in msg


def test_rows_needed_reports_a_row_whose_key_an_older_table_makes():
    row = ("fwd", "row A")
    msg = _rows_needed_message("guard: older row", lambda key: {key: [row]}, [[row]], older_has=True)
    assert f"{CONVT}: an older table already makes ('fwd', " in msg and f"of row {row}" in msg and "no program launches" not in msg


def test_rows_needed_reports_two_rows_with_one_key():
    rows = [("fwd", "row A"), ("fwd", "row B")]
    msg = _rows_needed_message("guard: double row", lambda key: {key: rows}, [rows])
    assert f"{CONVT}: 2 rows make ('fwd', " in msg and str(rows) in msg
    msg = _rows_needed_message("guard: double row", lambda key: {key: rows[:1] * 2}, [rows[:1] * 2])          # the same row twice
    assert f"{CONVT}: 2 rows make ('fwd', " in msg and "2 rows in the tables, 1 distinct rows that make a key" in msg


def test_rows_needed_reports_a_row_that_makes_no_key():
    row, mute = ("fwd", "row A"), ("fwd", "a row without a key")
    msg = _rows_needed_message("guard: mute row", lambda key: {key: [row]}, [[row, mute]])
    assert f"no key is made by row {mute}" in msg and "2 rows in the tables, 1 distinct rows that make a key" in msg and "row A" not in msg


def test_rows_needed_reports_an_empty_table():
    row = ("fwd", "row A")
    msg = _rows_needed_message("guard: empty table", lambda key: {key: [row]}, [[row], []])
    assert msg.endswith("\n  table 2 of 2 is empty")


def test_table_keys_are_the_key_functions_on_the_rows():
    """Three rows per family against the key functions called directly (the InstanceNorm rows: one-workgroup launches, which the name query
    answers without a device)."""
    import test_ops_gpu as OPS
    conv3 = [(F_, 4, [32, 32], 32, 512, 48, dict(compute=1, c8=True, bias=False, out_accumulate=True)), (D_, 2, [24], 12, 20, 48, dict(accumulate=[0])),
             (W_, 3, [1], 32, 8, 8, dict(bias=False))]
    plans = [(4, [32], 64, 512, 48, _WB), (1, [7], 8, 8, 8, dict(bias=False)), (48, [96], 128, 16, 16, _WB)]
    inorm = [(False, 2, 16, 12, 20, dict(_FP, stats_slots=64, pool=True)), (True, 2, 16, 12, 20, _FP), (True, 2, 3, 12, 20, dict(affine=False, inplace=True))]
    convT = [("fwd", 2, 64, 32, 8, 8, 2, {}, ()), ("dgrad", 2, 48, 24, 8, 8, 2, dict(acc_dx=True), ()), ("pair", 3, 48, 48, 16, 24, 2, {}, ())]
    wview = [(12, 8, 0, 8, 1, 28, 40), (8, 24, 16, 8, 1, 0, 40), (8, 24, 0, 24, 0, 0, 8)]
    own = SP.table_keys(conv3=conv3, wgrad_plan=plans, inorm=inorm, convT=convT, wview=wview)
    assert set(own) == set(SP.COLLECTORS) and not own[SMALL] and not own["loss"]
    assert own["conv3x3"] == {(c[0], SP._conv3_key(_c3(c[0], c[1], c[2], c[3], c[4], c[5], **c[6]), c[0])): [c] for c in conv3}
    assert own[PLAN] == {(W_, _plan(*c[:5], **c[5])): [c] for c in plans}
    assert own["InstanceNorm"] == {(L.OP_IN_BWD if c[0] else L.OP_IN_FWD, SP._instnorm_key(OPS._inorm_args(*c), c[0])): [c] for c in inorm}
    ct = {"fwd": L.OP_CONVT_FWD, "dgrad": L.OP_CONVT_DGRAD}
    assert own[CONVT] == {
        **{(c[0], SP._convT_key(ops.convT_case_args(ct[c[0]], *c[1:7], **c[7]), ct[c[0]])): [c] for c in convT[:2]},
        ("pair", SP._convT_key(ops.convT_case_args(L.OP_CONVT_WGRAD, 3, 48, 48, 16, 24, 2), L.OP_CONVT_WGRAD, ops.convT_case_args(L.OP_CONVT_DGRAD, 3, 48, 48, 16, 24, 2))): [convT[2]]}
    assert own[LAYOUT] == {SP._wview_key(*c, path): [c] for c in wview for path in ("single", "many")}
    assert all(len(keys) == (6 if family == LAYOUT else 3) for family, keys in own.items() if keys)
    assert SP.table_keys() == _rows()


def test_kernel_instances_are_the_launches_of_the_name_strings_without_their_brackets():
    seen = {family: {} for family in SP.COLLECTORS}
    seen["InstanceNorm"] = {(7, ("a<1, 2> [T=8 rounds=1] + b", ("affine",))): (7, (2, 8))}
    seen["conv3x3"] = {(1, ("c<false, 0> + b", ())): (1, ()), (2, ("c<false, 0> + d [threads=64]", ("segs>1",))): (2, ())}
    seen[LAYOUT] = {("fwd", 0, 0, False, False, 0, "single"): (3, ())}          # no name string: not looked at
    assert SP.kernel_instances(SP.Survey(("hand-made",), 0, {}, seen, {})) == {"a<1, 2>", "b", "c<false, 0>", "d"}
    s = _whole("guard: instances")          # ... and on the name queries' own strings: a launch and the reduction behind it
    assert {"conv3x3_wgrad_c8_kernel<false, 0>", "splitk_reduce"} <= SP.kernel_instances(s) and not any("[" in i or "+" in i for i in SP.kernel_instances(s))


def test_keys_subset_names_the_extra_key_and_a_family_without_a_launch():
    whole, part = _whole("guard: whole"), _whole("guard: part", without=[LAYOUT])
    SP.assert_keys_subset(part, whole, [f for f in SP.COLLECTORS if f != LAYOUT])
    SP.assert_keys_subset(whole, whole)
    with pytest.raises(AssertionError) as e:
        SP.assert_keys_subset(whole, part)
    key, kind, where = _only(whole, LAYOUT)
    assert str(e.value) == f"launches of {whole.program} that {part.program} does not make:\n  {LAYOUT}: {kind} {key} at {where}"
    with pytest.raises(AssertionError) as e:
        SP.assert_keys_subset(part, whole)
    assert str(e.value) == f"{part.program}: no {LAYOUT} launch found"


def test_op_kinds_claimed_names_the_unclaimed_and_the_missing_required_kind():
    s = _survey("guard: kinds", {"fwd": [_convT(L.OP_CONVT_FWD), ops.upsample2_case_args(UF_, *_UP)]})
    with pytest.raises(AssertionError) as e:
        SP.assert_op_kinds_claimed([_whole("guard: whole"), s])
    assert str(e.value) == f"op kinds of {s.program} that no test answers for: ['OP_UPSAMPLE2_FWD']"
    SP.assert_op_kinds_claimed([s], claimed_also=("OP_UPSAMPLE2_FWD",), required=(UF_, L.OP_CONVT_FWD))
    with pytest.raises(AssertionError) as e:
        SP.assert_op_kinds_claimed([s], claimed_also=("OP_UPSAMPLE2_FWD",), required=(UF_, UB_))
    assert str(e.value) == f"{s.program}: no op of kind ['OP_UPSAMPLE2_BWD']"
