"""tests/step_programs.py -- the survey of a step program and the compare-and-report behind the launch-coverage guards of tests/test_ops_gpu.py --
on hand-made programs: the walks that carry state (the ConvT pair, the run of layout ops), the session cache and the failure messages.
mtbc_convT_kernel_name and mtbc_op_kernel_name are host-only; no device, no step is built."""
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
