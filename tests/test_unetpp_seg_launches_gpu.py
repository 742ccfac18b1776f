"""The launches of the single-task U-Net++ segmentation step programs (nets.BasicUnetPlusPlus at MONAI's default widths (32, 32, 64, 128, 256, 32),
deep supervision, Adam, alpha 1; bf16 and f32 at 32 x 256 x 256, f16 at 16 x 512 x 512: the benchmark's shapes), each tied to an element-wise fp64
reference case: the tables below hold one row per coverage key (tests/step_programs.py) of those programs that no table of
tests/test_ops_gpu.py makes, run through that file's own fp64 tests -- references, bounds and the made-launches-equal-planned-launches assertion
are theirs --, and the guards compare the surveyed programs with the tables.  The widths are what is new: 32-channel cells with a conv bias
where nnU-Net has none, 64- and 128-channel levels at map sizes the other models give to 48 and 96 channels.  With MTUNetPlusPlus's own widths
the programs launch nothing the multi-task programs do not launch (the second guard).  profiles/unetpp_seg_step_keys.txt is the listing."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

import step_programs as SP  # noqa: E402
from multi_task_breast_cancer_amd import nets, ops  # noqa: E402

L = ops.L
PROGRAMS = [("UnetPlusPlus", "bf16", 32, 256), ("UnetPlusPlus", "f32", 32, 256), ("UnetPlusPlus", "f16", 16, 512)]
NARROW = [("UnetPlusPlus-f24", "bf16", 32, 256), ("UnetPlusPlus-f24", "f32", 32, 256)]          # features=nets.UNETPP_FEATURES
F_, D_, W_ = L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD


def _ops_gpu():
    import test_ops_gpu as OPS
    return OPS


def _make_model(arch):
    from multi_task_breast_cancer_amd.experiment_init import init_segmentation_model
    if arch == "UnetPlusPlus":
        return init_segmentation_model("UnetPlusPlus", sequences=1, regions=1, deep_supervision=True)
    return nets.BasicUnetPlusPlus(2, 1, 1, features=nets.UNETPP_FEATURES, deep_supervision=True)


def _survey(program):
    """The survey of one program of this model, built (not run) once per session through the factory's constructor path."""
    return SP.survey(program, build=SP.step_builder(_make_model, alpha=1.0))


# ------------------------------------------------------------------------------------------------ 3x3 convolution
# (op, N, segs, Cout, H, W, mode) as in CONV3_STEP_CASES of tests/test_ops_gpu.py, and by its shape rule: the key holds neither N nor the map
# size, so each row takes the fewest pixels -- of at least 2 images (3 for a weight gradient) -- at which the dummy-pointer struct has the key
# of the step's launch.  Every cell of this model has a conv bias.  Behind each row: its key, and in brackets the first launch of the step it
# stands for (N x segments -> Cout @ map, programs).
CONV3_CASES = [
    (F_, 4, [32, 32], 32, 512, 48, dict(compute=1, c8=True, bias=False, out_accumulate=True)),          # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0> (out_acc, segs>1)  [32 x 32+32 -> 32 @ 128 x 128 in bf16 and 2 more]
    (F_, 4, [32], 32, 512, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),       # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3> (bias, stats)  [32 x 32 -> 32 @ 128 x 128 in bf16 and 11 more]
    (F_, 4, [32, 32], 32, 512, 48, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),   # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3> (bias, stats, segs>1)  [32 x 32+32 -> 32 @ 128 x 128 in bf16 and 5 more]
    (F_, 64, [32, 32], 32, 20, 512, dict(compute=1, c8=True, bias=False)),                              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0> (segs>1)  [32 x 32+32 -> 32 @ 256 x 256 in bf16 and 2 more]
    (F_, 64, [32], 32, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),      # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3> (bias, stats)  [32 x 32 -> 32 @ 256 x 256 in bf16 and 4 more]
    (F_, 64, [32, 32], 32, 20, 512, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),  # conv3x3_igemm_c8_kernel<2, 0, false, 8, 3> (bias, stats, segs>1)  [32 x 32+32 -> 32 @ 256 x 256 in bf16 and 3 more]
    (F_, 2, [128], 256, 16, 16, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),      # conv3x3_igemm_c8_ring_kernel<2, 1, false, 3, 3> (bias, stats)  [32 x 128 -> 256 @ 16 x 16 in bf16 and 1 more]
    (F_, 2, [1], 32, 8, 8, dict(compute=1, c8=True, out_c8=True, out_fp16=True, stats=True)),           # conv3x3_stem_fwd_c8_kernel<true> (bias, stats, ragged_k)  [32 x 1 -> 32 @ 256 x 256 in bf16 / f16 and 1 more]
    (D_, 24, [64, 64], 64, 20, 48, dict(compute=1, c8=True, accumulate=[0, 2])),                        # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0> (codes=0,2, segs>1)  [32 x 64+64 -> 64 @ 64 x 64 in bf16 and 1 more]
    (D_, 4, [32], 32, 512, 48, dict(compute=1, c8=True, accumulate=[2])),                               # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0> (codes=2)  [32 x 32 -> 32 @ 128 x 128 in bf16 and 2 more]
    (D_, 64, [32], 32, 20, 512, dict(compute=1, c8=True, accumulate=[2])),                              # conv3x3_igemm_c8_kernel<2, 0, false, 8, 0> (codes=2)  [32 x 32 -> 32 @ 256 x 256 in bf16 and 2 more]
    (D_, 2, [64], 128, 20, 32, dict(compute=1, c8=True, accumulate=[0])),                               # conv3x3_igemm_c8_ring_kernel<2, 0, false, 0, 3> (codes=0)  [32 x 64 -> 128 @ 32 x 32 in bf16]
    (D_, 2, [256], 256, 16, 16, dict(compute=1, c8=True, accumulate=[0])),                              # conv3x3_igemm_c8_ring_kernel<2, 1, false, 0, 3> (codes=0)  [32 x 256 -> 256 @ 16 x 16 in bf16 and 1 more]
    (F_, 4, [32, 32], 32, 512, 48, dict()),                                                             # conv3x3_igemm_dma_kernel<2, 0, 2> (bias, segs>1)  [32 x 32+32 -> 32 @ 256 x 256 in f32 and 9 more]
    (F_, 4, [32], 32, 512, 48, dict()),                                                                 # conv3x3_igemm_dma_kernel<2, 0, 2> (bias)  [32 x 32 -> 32 @ 256 x 256 in f32 and 16 more]
    (F_, 2, [1], 32, 8, 8, dict()),                                                                     # conv3x3_stem_fwd_kernel (bias, ragged_k)  [32 x 1 -> 32 @ 256 x 256 in f32]
    (D_, 4, [32], 32, 512, 48, dict(accumulate=[0])),                                                   # conv3x3_igemm_dma_kernel<2, 0, 2> (codes=0)  [32 x 32 -> 32 @ 256 x 256 in f32 and 15 more]
    (D_, 48, [32, 32], 32, 20, 48, dict(accumulate=[1, 0])),                                            # conv3x3_igemm_dma_kernel<2, 0, 2> (codes=0,1, segs>1)  [32 x 32+32 -> 32 @ 128 x 128 in f32 and 1 more]
    (W_, 3, [1], 32, 8, 8, dict(bias=False)),                                                           # conv3x3_wgrad_smallcin_kernel + splitk_reduce (ragged_k)  [32 x 1 -> 32 @ 256 x 256 in f32]
    (F_, 48, [64, 64], 64, 20, 48, dict(compute=2, c8=True, bias=False, out_accumulate=True)),          # conv3x3_igemm_c8_kernel<2, 0, true, 4, 0> (out_acc, segs>1)  [16 x 64+64 -> 64 @ 128 x 128 in f16]
    (F_, 64, [32, 32], 32, 20, 512, dict(compute=2, c8=True, bias=False, out_accumulate=True)),         # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0> (out_acc, segs>1)  [16 x 32+32 -> 32 @ 256 x 256 in f16 and 1 more]
    (F_, 64, [32, 32], 32, 20, 512, dict(compute=2, c8=True, bias=False)),                              # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0> (segs>1)  [16 x 32+32 -> 32 @ 512 x 512 in f16 and 2 more]
    (F_, 64, [32], 32, 20, 512, dict(compute=2, c8=True, out_c8=True, stats=True)),                     # conv3x3_igemm_c8_kernel<2, 0, true, 8, 1> (bias, stats)  [16 x 32 -> 32 @ 512 x 512 in f16 and 9 more]
    (F_, 64, [32, 32], 32, 20, 512, dict(compute=2, c8=True, out_c8=True, stats=True)),                 # conv3x3_igemm_c8_kernel<2, 0, true, 8, 1> (bias, stats, segs>1)  [16 x 32+32 -> 32 @ 512 x 512 in f16 and 6 more]
    (D_, 12, [128, 128], 128, 20, 48, dict(compute=2, c8=True, accumulate=[0, 2])),                     # conv3x3_igemm_c8_kernel<2, 0, true, 4, 0> (codes=0,2, segs>1)  [16 x 128+128 -> 128 @ 64 x 64 in f16]
    (D_, 48, [64], 64, 20, 48, dict(compute=2, c8=True, accumulate=[2])),                               # conv3x3_igemm_c8_kernel<2, 0, true, 4, 0> (codes=2)  [16 x 64 -> 64 @ 128 x 128 in f16]
    (D_, 64, [32], 32, 20, 512, dict(compute=2, c8=True, accumulate=[0])),                              # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0> (codes=0)  [16 x 32 -> 32 @ 512 x 512 in f16 and 9 more]
    (D_, 32, [32, 32], 32, 20, 512, dict(compute=2, c8=True, accumulate=[0, 2])),                       # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0> (codes=0,2, segs>1)  [16 x 32+32 -> 32 @ 512 x 512 in f16 and 2 more]
    (D_, 64, [32], 32, 20, 512, dict(compute=2, c8=True, accumulate=[2])),                              # conv3x3_igemm_c8_kernel<2, 0, true, 8, 0> (codes=2)  [16 x 32 -> 32 @ 512 x 512 in f16 and 4 more]
    (D_, 2, [128], 256, 20, 32, dict(compute=2, c8=True, accumulate=[0])),                              # conv3x3_igemm_c8_ring_kernel<2, 0, true, 0, 3> (codes=0)  [16 x 128 -> 256 @ 32 x 32 in f16]
    (W_, 3, [32, 32, 32, 32, 32], 32, 20, 128, dict(compute=2, c8=True, bias=False)),                   # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs>1)  [16 x 32+32+32+32+32 -> 32 @ 512 x 512 in f16 and 8 more]
    (W_, 3, [64], 64, 20, 128, dict(compute=2, c8=True, bias=False)),                                   # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce  [16 x 64 -> 64 @ 128 x 128 in f16 and 2 more]
    (W_, 3, [1], 32, 8, 8, dict(compute=2, c8=True, bias=False)),                                       # conv3x3_wgrad_stem_c8_kernel<true> + splitk_reduce (ragged_k)  [16 x 1 -> 32 @ 512 x 512 in f16]
]


def _conv3_ids():
    return [_ops_gpu()._conv3_case_id(c) for c in CONV3_CASES]


@pytest.mark.parametrize("case", CONV3_CASES, ids=_conv3_ids())
def test_conv3x3_launches_match_fp64(case):
    _ops_gpu().test_conv3x3_step_instances_match_fp64(case)


# ------------------------------------------------------------------------------------------------ the split plans of the 3x3 weight gradients
# (N, segs, Cout, H, W, mode) as in WGRAD_PLAN_CASES of tests/test_ops_gpu.py, and by its shape rule (of the channel counts and map sizes at
# which the dummy-pointer struct has the plan key, the fewest multiply-adds, then the fewest pixels; one segment): one row per plan key
# (tests/step_programs.py _wgrad_plan_key) of the three programs that no table of that file makes.  Behind each row: its plan key, and in
# brackets the first launch it stands for.
_PB, _PH, _P32 = dict(compute=1, c8=True, bias=False), dict(compute=2, c8=True, bias=False), dict(bias=False)
WGRAD_PLAN_CASES = [
    (4, [32], 64, 512, 48, _PB),     # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (even, tiles=2, splitk_reduce<16> x8)  [32 x 32 -> 64 @ 64 x 64 in bf16]
    (1, [40], 96, 512, 48, _PB),     # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles=2, splitk_reduce<16> x8)  [32 x 64 -> 128 @ 32 x 32 in bf16]
    (2, [192], 128, 96, 48, _PB),    # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<4> x8)  [32 x 128+128 -> 128 @ 32 x 32 in bf16]
    (48, [96], 128, 16, 16, _PB),    # conv3x3_wgrad_c8i_kernel<false, 2, false> + splitk_reduce (images=2, ciblocks>1, splitk_reduce<4> x2)  [32 x 128 -> 256 @ 16 x 16 in bf16]
    (8, [128], 16, 128, 128, _PB),   # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [32 x 32+32+32+32 -> 32 @ 128 x 128 in bf16 and 1 more]
    (16, [64], 32, 128, 128, _PB),   # conv3x3_wgrad_c8w_kernel<false, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, splitk_reduce<16> x8)  [32 x 32+32 -> 32 @ 128 x 128 in bf16 and 1 more]
    (64, [96], 8, 20, 48, _P32),     # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<16> x8+x2+x1)  [32 x 32+32+32+32+32 -> 32 @ 256 x 256 in f32 and 8 more]
    (2, [256], 128, 256, 48, _P32),  # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<4> x2)  [32 x 128+128 -> 128 @ 32 x 32 in f32]
    (8, [8], 8, 512, 48, _P32),      # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, ragged, crosses, splitk_reduce<64, 16> x8+x2+x1)  [32 x 32 -> 32 @ 256 x 256 in f32 and 9 more]
    (4, [192], 64, 96, 48, _P32),    # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x2)  [32 x 64+64+64 -> 64 @ 64 x 64 in f32]
    (4, [96], 128, 96, 48, _PH),     # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x2)  [16 x 128 -> 128 @ 64 x 64 in f16 and 1 more]
    (8, [40], 96, 96, 48, _PH),      # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [16 x 64 -> 128 @ 64 x 64 in f16]
    (1, [192], 256, 96, 48, _PH),    # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<4> x2)  [16 x 256 -> 256 @ 32 x 32 in f16]
    (2, [192], 128, 96, 48, _PH),    # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<4> x8)  [16 x 128+128 -> 128 @ 64 x 64 in f16 and 1 more]
    (24, [192], 8, 20, 128, _PH),    # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs=1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x2)  [16 x 64+64+64 -> 64 @ 128 x 128 in f16]
    (8, [128], 16, 128, 128, _PH),   # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, ciblocks>1, splitk_reduce<16> x8)  [16 x 32+32+32+32 -> 32 @ 256 x 256 in f16 and 2 more]
    (8, [64], 40, 128, 128, _PH),    # conv3x3_wgrad_c8w_kernel<true, 2, false> + splitk_reduce (segs>1, img8, steps>=ring, splitk_reduce<16> x8)  [16 x 64 -> 64 @ 128 x 128 in f16 and 4 more]
]


def _wgrad_plan_ids():
    return [_ops_gpu()._wgrad_plan_case_id(c) for c in WGRAD_PLAN_CASES]


@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=_wgrad_plan_ids())
def test_conv3x3_wgrad_plans_match_fp64(case):
    _ops_gpu().test_conv3x3_wgrad_plan_cases_match_fp64(case)


# ------------------------------------------------------------------------------------------------ transposed convolution
# (kind, N, Cin, Cout, H, W, k, mode, strided) as in CONVT_CASES of tests/test_ops_gpu.py: the fp32 forward through the LDS kernel at KI = 16
# WITH a bias and dense tensors (that table has the instance without a bias, on views)  [32 x 64 -> 32 @ 64 x 64 in f32 and 2 more]
CONVT_CASES = [("fwd", 2, 64, 32, 8, 8, 2, {}, ())]


def _convT_ids():
    return [_ops_gpu()._convT_case_id(c) for c in CONVT_CASES]


@pytest.mark.parametrize("case", CONVT_CASES, ids=_convT_ids())
def test_convT_launches_match_fp64(case):
    _ops_gpu().test_convT_step_instances_match_fp64(case)


# ------------------------------------------------------------------------------------------------ the guards
def _own_keys():
    return SP.table_keys(conv3=CONV3_CASES, wgrad_plan=WGRAD_PLAN_CASES, convT=CONVT_CASES)


@pytest.mark.parametrize("program", PROGRAMS, ids=[p[1] for p in PROGRAMS])
def test_unetpp_seg_programs_launch_only_reference_tested_instances(program):
    """Every coverage key of the step program -- kernel instances AND the branches the arguments select, as tests/step_programs.py keys them --
    is the key of a call that an element-wise reference test makes: the tables of tests/test_ops_gpu.py and tests/test_loss_launches_gpu.py,
    or the rows of this module.  The print-out is profiles/unetpp_seg_step_keys.txt."""
    s = _survey(program)
    assert not any(kind in (L.OP_LINEAR_FWD, L.OP_GAP_FWD, L.OP_FOCAL) for kinds in s.kinds.values() for kind in kinds), "a classification op in a segmentation-only program"
    SP.assert_only_tested(s, SP.reference_tested_keys(), _own_keys())


@pytest.mark.parametrize("program", NARROW, ids=[p[1] for p in NARROW])
def test_narrow_unetpp_seg_programs_launch_a_subset_of_the_multitask_programs(program):
    """With features=nets.UNETPP_FEATURES the program launches no coverage key that the MTUNetPlusPlus program of the same mode and shape (the
    benchmark's, tests/step_programs.py STEP_PROGRAMS) does not launch: taking the classification head away brings no kernel instance and
    no argument branch of its own."""
    mt_program = ("MTUNetPlusPlus",) + program[1:]
    assert mt_program in SP.STEP_PROGRAMS
    SP.assert_keys_subset(_survey(program), SP.survey(mt_program))


def test_unetpp_seg_cases_are_all_needed():
    """Every row of this module's tables makes a key that a surveyed program launches, that no table of tests/test_ops_gpu.py makes and that no
    other row makes: no dead and no double rows, and deleting one fails the first guard."""
    SP.assert_rows_needed("tests/test_unetpp_seg_launches_gpu.py", [_survey(p) for p in PROGRAMS], SP.reference_tested_keys(), _own_keys(),
                          [CONV3_CASES, WGRAD_PLAN_CASES, CONVT_CASES])


def test_every_op_kind_of_the_unetpp_seg_programs_is_claimed():
    """The op kinds of the three programs are among those tests/test_ops_gpu.py's OP_KIND_COVERED_BY claims."""
    SP.assert_op_kinds_claimed([_survey(p) for p in PROGRAMS])
