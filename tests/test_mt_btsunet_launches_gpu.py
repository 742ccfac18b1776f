"""The launches of the Multi_BTSUNet step programs (width 24 of the reference's config.yaml, deep supervision, 3 classes, 128 x 128; bf16 and f16
at N 16, f32 at N 2: the shapes of tools/btsunet_cost.py), each tied to an element-wise fp64 reference case: the tables below hold one row per
coverage key (tests/step_programs.py) of those programs that no table of tests/test_ops_gpu.py makes, run through that file's own fp64 tests --
references, bounds and the made-launches-equal-planned-launches assertion are theirs --, and three guards compare the surveyed programs with
the tables.  The up-sampling and wide-Linear keys are answered by the cases of tests/test_mt_btsunet_ops_gpu.py, by key.
profiles/mt_btsunet_step_keys.txt is the listing."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

import step_programs as SP  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402

L = ops.L
PROGRAMS = [("Multi_BTSUNet-w24", "bf16", 16, 128), ("Multi_BTSUNet-w24", "f16", 16, 128), ("Multi_BTSUNet-w24", "f32", 2, 128)]
F_, D_, W_ = L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD


def _ops_gpu():
    import test_ops_gpu as OPS
    return OPS


def _bts_ops():
    import test_mt_btsunet_ops_gpu as BTS
    return BTS


def _survey(program):
    """The survey of one Multi_BTSUNet program, built (not run) once per session by tests/step_programs.py."""
    return SP.survey(program, build=SP.step_builder(lambda arch: SP.multitask_model("Multi_BTSUNet", width=24), alpha=0.5, inversely_weighted=True))


# ------------------------------------------------------------------------------------------------ 3x3 convolution
# (op, N, segs, Cout, H, W, mode) as in CONV3_STEP_CASES of tests/test_ops_gpu.py, and by its shape rule: the key holds neither N nor the map
# size, so each row takes the fewest pixels -- of at least 2 images (3 for a weight gradient), 20 x 48 where the step's map is that large,
# 20 x 32 under a 32 x 32 map, 16 x 16 for the instances the plan picks by that map size -- at which the dummy-pointer struct has the key of
# the step's launch.  No cell of this model has a conv bias.  In brackets: the launch of the step (N x segments -> Cout @ map, programs).
CONV3_CASES = [
    (F_, 2, [12], 24, 20, 48, dict(bias=False)),                                                                    # conv3x3_direct_kernel (ragged_rows, ragged_k)  [16 x 12 -> 24 @ 128 x 128 in bf16 / f16 / f32]
    (F_, 2, [24], 12, 20, 48, dict(compute=1, c8=True, bias=False)),                                                # conv3x3_igemm_c8_kernel<1, 0, false, 4, 0> (ragged_rows, ragged_k)  [16 x 24 -> 12 @ 128 x 128 in bf16]
    (F_, 2, [48], 48, 20, 32, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),        # conv3x3_igemm_c8_kernel<1, 0, false, 4, 3> (stats, ragged_k)  [16 x 48 -> 48 @ 32 x 32 in bf16]
    (F_, 2, [24], 24, 20, 48, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),        # conv3x3_igemm_c8_kernel<1, 0, false, 4, 3> (stats, ragged_rows, ragged_k)  [16 x 24 -> 24 @ 64 x 64 in bf16]
    (F_, 48, [24], 48, 20, 48, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),       # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3> (stats, ragged_k)  [16 x 24 -> 48 @ 64 x 64 in bf16]
    (F_, 4, [24, 24], 24, 512, 48, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),   # conv3x3_igemm_c8_kernel<2, 0, false, 4, 3> (stats, segs>1, straddle, ragged_rows, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in bf16]
    (F_, 2, [96, 96], 96, 20, 32, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),    # conv3x3_igemm_c8_ring_kernel<3, 0, false, 3, 3> (stats, segs>1)  [16 x 96+96 -> 96 @ 32 x 32 in bf16]
    (F_, 2, [48, 48], 48, 20, 48, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),    # conv3x3_igemm_c8_ring_kernel<3, 0, false, 3, 3> (stats, segs>1, straddle)  [16 x 48+48 -> 48 @ 64 x 64 in bf16]
    (F_, 2, [96], 48, 20, 32, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),        # conv3x3_igemm_c8_ring_kernel<3, 0, false, 3, 3> (stats)  [16 x 96 -> 48 @ 32 x 32 in bf16]
    (F_, 2, [192, 96], 192, 16, 16, dict(compute=1, c8=True, bias=False)),                                          # conv3x3_igemm_c8_ring_kernel<3, 1, false, 0, 3> (segs>1)  [16 x 192+96 -> 192 @ 16 x 16 in bf16]
    (F_, 2, [192, 192], 96, 16, 16, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),  # conv3x3_igemm_c8_ring_kernel<3, 1, false, 3, 3> (stats, segs>1)  [16 x 192+192 -> 96 @ 16 x 16 in bf16]
    (F_, 2, [96], 96, 16, 16, dict(compute=1, c8=True, bias=False, out_c8=True, stats=True, out_fp16=True)),        # conv3x3_igemm_c8_ring_kernel<3, 1, false, 3, 3> (stats)  [16 x 96 -> 96 @ 16 x 16 in bf16]
    (F_, 2, [1], 12, 20, 48, dict(bias=False)),                                                                     # conv3x3_stem_fwd_kernel (ragged_rows, ragged_k)  [16 x 1 -> 12 @ 128 x 128 in bf16 / f16 / f32]
    (D_, 2, [24], 12, 20, 48, dict(accumulate=[0])),                                                                # conv3x3_direct_kernel (codes=0, ragged_rows, ragged_k)  [16 x 24 -> 12 @ 128 x 128 in bf16 / f16 / f32]
    (D_, 48, [48], 24, 20, 48, dict(compute=1, c8=True, accumulate=[0])),                                           # conv3x3_igemm_c8_kernel<2, 0, false, 4, 0> (codes=0, ragged_k)  [16 x 48 -> 24 @ 64 x 64 in bf16]
    (D_, 48, [48, 48], 48, 20, 48, dict(compute=1, c8=True, accumulate=[0, 0])),                                    # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0> (codes=0, segs>1, ragged_k)  [16 x 48+48 -> 48 @ 64 x 64 in bf16]
    (D_, 4, [24, 24], 24, 512, 48, dict(compute=1, c8=True, accumulate=[0, 0])),                                    # conv3x3_igemm_c8_kernel<3, 0, false, 4, 0> (codes=0, segs>1, straddle, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in bf16]
    (D_, 2, [96, 96], 96, 20, 32, dict(compute=1, c8=True, accumulate=[0, 0])),                                     # conv3x3_igemm_c8_ring_kernel<3, 0, false, 0, 3> (codes=0, segs>1)  [16 x 96+96 -> 96 @ 32 x 32 in bf16]
    (W_, 3, [48, 48], 48, 20, 48, dict(compute=1, c8=True, bias=False)),                                            # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (segs>1, straddle)  [16 x 48+48 -> 48 @ 64 x 64 in bf16]
    (W_, 3, [24, 24], 24, 20, 48, dict(compute=1, c8=True, bias=False)),                                            # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (segs>1, straddle, ragged_rows, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in bf16]
    (W_, 3, [192, 192, 192], 192, 16, 16, dict(compute=1, c8=True, bias=False)),                                    # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce (segs>1)  [16 x 192+192+192 -> 192 @ 16 x 16 in bf16]
    (W_, 3, [12], 24, 20, 48, dict(bias=False)),                                                                    # conv3x3_wgrad_direct_kernel + splitk_reduce (ragged_rows, ragged_k)  [16 x 12 -> 24 @ 128 x 128 in bf16 / f16 / f32]
    (W_, 3, [24], 12, 20, 48, dict(compute=1, bias=False)),                                                         # conv3x3_wgrad_lp2_kernel<false> + splitk_reduce (ragged_rows, ragged_k)  [16 x 24 -> 12 @ 128 x 128 in bf16]
    (F_, 2, [24], 12, 20, 48, dict(compute=2, c8=True, bias=False)),                                                # conv3x3_igemm_c8_kernel<1, 0, true, 4, 0> (ragged_rows, ragged_k)  [16 x 24 -> 12 @ 128 x 128 in f16]
    (F_, 2, [48], 48, 20, 32, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                       # conv3x3_igemm_c8_kernel<1, 0, true, 4, 1> (stats, ragged_k)  [16 x 48 -> 48 @ 32 x 32 in f16]
    (F_, 2, [24], 24, 20, 48, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                       # conv3x3_igemm_c8_kernel<1, 0, true, 4, 1> (stats, ragged_rows, ragged_k)  [16 x 24 -> 24 @ 64 x 64 in f16]
    (F_, 48, [24], 48, 20, 48, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                      # conv3x3_igemm_c8_kernel<2, 0, true, 4, 1> (stats, ragged_k)  [16 x 24 -> 48 @ 64 x 64 in f16]
    (F_, 4, [24, 24], 24, 512, 48, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                  # conv3x3_igemm_c8_kernel<2, 0, true, 4, 1> (stats, segs>1, straddle, ragged_rows, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in f16]
    (F_, 2, [96, 96], 96, 20, 32, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                   # conv3x3_igemm_c8_ring_kernel<3, 0, true, 1, 3> (stats, segs>1)  [16 x 96+96 -> 96 @ 32 x 32 in f16]
    (F_, 2, [48, 48], 48, 20, 48, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                   # conv3x3_igemm_c8_ring_kernel<3, 0, true, 1, 3> (stats, segs>1, straddle)  [16 x 48+48 -> 48 @ 64 x 64 in f16]
    (F_, 2, [96], 48, 20, 32, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                       # conv3x3_igemm_c8_ring_kernel<3, 0, true, 1, 3> (stats)  [16 x 96 -> 48 @ 32 x 32 in f16]
    (F_, 2, [192, 96], 192, 16, 16, dict(compute=2, c8=True, bias=False)),                                          # conv3x3_igemm_c8_ring_kernel<3, 1, true, 0, 3> (segs>1)  [16 x 192+96 -> 192 @ 16 x 16 in f16]
    (F_, 2, [192, 192], 96, 16, 16, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                 # conv3x3_igemm_c8_ring_kernel<3, 1, true, 1, 3> (stats, segs>1)  [16 x 192+192 -> 96 @ 16 x 16 in f16]
    (F_, 2, [96], 96, 16, 16, dict(compute=2, c8=True, bias=False, out_c8=True, stats=True)),                       # conv3x3_igemm_c8_ring_kernel<3, 1, true, 1, 3> (stats)  [16 x 96 -> 96 @ 16 x 16 in f16]
    (D_, 48, [48], 24, 20, 48, dict(compute=2, c8=True, accumulate=[0])),                                           # conv3x3_igemm_c8_kernel<2, 0, true, 4, 0> (codes=0, ragged_k)  [16 x 48 -> 24 @ 64 x 64 in f16]
    (D_, 48, [48, 48], 48, 20, 48, dict(compute=2, c8=True, accumulate=[0, 0])),                                    # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0> (codes=0, segs>1, ragged_k)  [16 x 48+48 -> 48 @ 64 x 64 in f16]
    (D_, 4, [24, 24], 24, 512, 48, dict(compute=2, c8=True, accumulate=[0, 0])),                                    # conv3x3_igemm_c8_kernel<3, 0, true, 4, 0> (codes=0, segs>1, straddle, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in f16]
    (D_, 2, [96, 96], 96, 20, 32, dict(compute=2, c8=True, accumulate=[0, 0])),                                     # conv3x3_igemm_c8_ring_kernel<3, 0, true, 0, 3> (codes=0, segs>1)  [16 x 96+96 -> 96 @ 32 x 32 in f16]
    (D_, 2, [48], 96, 20, 32, dict(compute=2, c8=True, accumulate=[0])),                                            # conv3x3_igemm_c8_ring_kernel<3, 0, true, 0, 3> (codes=0)  [16 x 48 -> 96 @ 32 x 32 in f16]
    (D_, 2, [192], 192, 16, 16, dict(compute=2, c8=True, accumulate=[0])),                                          # conv3x3_igemm_c8_ring_kernel<3, 1, true, 0, 3> (codes=0)  [16 x 192 -> 192 @ 16 x 16 in f16]
    (W_, 3, [48, 48], 48, 20, 48, dict(compute=2, c8=True, bias=False)),                                            # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (segs>1, straddle)  [16 x 48+48 -> 48 @ 64 x 64 in f16]
    (W_, 3, [24, 24], 24, 20, 48, dict(compute=2, c8=True, bias=False)),                                            # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (segs>1, straddle, ragged_rows, ragged_k)  [16 x 24+24 -> 24 @ 128 x 128 in f16]
    (W_, 3, [192, 192, 192], 192, 16, 16, dict(compute=2, c8=True, bias=False)),                                    # conv3x3_wgrad_c8i_kernel<true, 3, false> + splitk_reduce (segs>1)  [16 x 192+192+192 -> 192 @ 16 x 16 in f16]
    (W_, 3, [96], 192, 16, 16, dict(compute=2, c8=True, bias=False)),                                               # conv3x3_wgrad_c8i_kernel<true, 3, false> + splitk_reduce  [16 x 96 -> 192 @ 16 x 16 in f16]
    (W_, 3, [24], 12, 20, 48, dict(compute=2, bias=False)),                                                         # conv3x3_wgrad_lp2_kernel<true> + splitk_reduce (ragged_rows, ragged_k)  [16 x 24 -> 12 @ 128 x 128 in f16]
    (F_, 2, [24], 24, 20, 48, dict(bias=False)),                                                                    # conv3x3_igemm_dma_kernel<1, 0, 2> (ragged_rows)  [2 x 24 -> 24 @ 64 x 64 in f32]
    (F_, 2, [24, 24], 24, 20, 48, dict(bias=False)),                                                                # conv3x3_igemm_dma_kernel<1, 0, 2> (segs>1, ragged_rows)  [2 x 24+24 -> 24 @ 128 x 128 in f32]
    (F_, 2, [96, 96], 96, 20, 32, dict(bias=False)),                                                                # conv3x3_igemm_dma_kernel<1, 0, 2> (segs>1)  [2 x 96+96 -> 96 @ 32 x 32 in f32]
    (F_, 2, [24], 48, 20, 48, dict(bias=False)),                                                                    # conv3x3_igemm_dma_kernel<1, 0, 2>  [2 x 24 -> 48 @ 64 x 64 in f32]
    (F_, 2, [192, 192], 96, 16, 16, dict(bias=False)),                                                              # conv3x3_igemm_dma_kernel<1, 1, 2> (segs>1)  [2 x 192+192 -> 96 @ 16 x 16 in f32]
    (F_, 2, [96], 96, 16, 16, dict(bias=False)),                                                                    # conv3x3_igemm_dma_kernel<1, 1, 2>  [2 x 96 -> 96 @ 16 x 16 in f32]
    (D_, 2, [24], 48, 20, 48, dict(accumulate=[0])),                                                                # conv3x3_igemm_dma_kernel<1, 0, 2> (codes=0, ragged_rows)  [2 x 24 -> 48 @ 64 x 64 in f32]
    (D_, 2, [48, 48], 48, 20, 48, dict(accumulate=[0, 0])),                                                         # conv3x3_igemm_dma_kernel<1, 0, 2> (codes=0, segs>1)  [2 x 48+48 -> 48 @ 64 x 64 in f32]
    (D_, 2, [24, 24], 24, 20, 48, dict(accumulate=[0, 0])),                                                         # conv3x3_igemm_dma_kernel<1, 0, 2> (codes=0, segs>1, straddle)  [2 x 24+24 -> 24 @ 128 x 128 in f32]
    (D_, 2, [192, 192, 192], 192, 16, 16, dict(accumulate=[0, 0, 0])),                                              # conv3x3_igemm_dma_kernel<1, 1, 2> (codes=0, segs>1)  [2 x 192+192+192 -> 192 @ 16 x 16 in f32]
    (D_, 2, [192, 192], 96, 16, 16, dict(accumulate=[1, 1])),                                                       # conv3x3_igemm_dma_kernel<1, 1, 2> (codes=1, segs>1)  [2 x 192+192 -> 96 @ 16 x 16 in f32]
    (W_, 3, [96], 48, 20, 32, dict(bias=False)),                                                                    # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce  [2 x 96 -> 48 @ 32 x 32 in f32]
]


def _conv3_ids():
    return [_ops_gpu()._conv3_case_id(c) for c in CONV3_CASES]


@pytest.mark.parametrize("case", CONV3_CASES, ids=_conv3_ids())
def test_conv3x3_launches_match_fp64(case):
    _ops_gpu().test_conv3x3_step_instances_match_fp64(case)


# ------------------------------------------------------------------------------------------------ the split plans of the 3x3 weight gradients
# (N, segs, Cout, H, W, mode) as in WGRAD_PLAN_CASES of tests/test_ops_gpu.py, and by its shape rule (the fewest multiply-adds at which the
# dummy-pointer struct has the plan key): one row per plan key (tests/step_programs.py _wgrad_plan_key) of the three programs that no table of
# that file makes -- at N 16 / 2 on maps of 128 x 128 and below the tile-walking kernels get ONE tile per split behind the many-split
# reductions, which the benchmark's batches never do.  Behind each row: its plan key, and in brackets the first launch it stands for.
_PB, _PH, _P32 = dict(compute=1, c8=True, bias=False), dict(compute=2, c8=True, bias=False), dict(bias=False)
_LB, _LH = dict(compute=1, bias=False), dict(compute=2, bias=False)          # 16-bit MFMA on fp32 planes (a 12-channel neighbour: no channel-blocked tensors)
WGRAD_PLAN_CASES = [
    (32, [8], 8, 96, 48, _LB),        # conv3x3_wgrad_lp2_kernel<false> + splitk_reduce (fixed, tiles>=3, splitk_reduce<64, 16> x8)  [16 x 24 -> 12 @ 128 x 128 in bf16]
    (1, [8], 8, 256, 48, _PB),        # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles=1, splitk_reduce<16> x8)  [16 x 96 -> 48 @ 32 x 32 in bf16 and 2 more]
    (2, [8], 8, 512, 48, _PB),        # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles=1, splitk_reduce<64, 16> x8)  [16 x 48 -> 24 @ 64 x 64 in bf16 and 2 more]
    (8, [8], 192, 96, 48, _PB),       # conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [16 x 48+48 -> 48 @ 64 x 64 in bf16]
    (8, [96], 48, 16, 16, _PB),       # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce (images=1, ciblocks>1, splitk_reduce<4> x2)  [16 x 96 -> 192 @ 16 x 16 in bf16 and 3 more]
    (48, [96], 192, 16, 16, _PB),     # conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce (images=2, ciblocks>1, splitk_reduce<4> x2)  [16 x 192+192+192 -> 192 @ 16 x 16 in bf16]
    (32, [8], 8, 96, 48, _LH),        # conv3x3_wgrad_lp2_kernel<true> + splitk_reduce (fixed, tiles>=3, splitk_reduce<64, 16> x8)  [16 x 24 -> 12 @ 128 x 128 in f16]
    (1, [8], 8, 256, 48, _PH),        # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles=1, splitk_reduce<16> x8)  [16 x 96 -> 48 @ 32 x 32 in f16 and 2 more]
    (2, [8], 8, 512, 48, _PH),        # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles=1, splitk_reduce<64, 16> x8)  [16 x 48 -> 24 @ 64 x 64 in f16 and 2 more]
    (8, [8], 192, 96, 48, _PH),       # conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce (fixed, tiles>=3, splitk_reduce<16> x8)  [16 x 48+48 -> 48 @ 64 x 64 in f16]
    (8, [96], 48, 16, 16, _PH),       # conv3x3_wgrad_c8i_kernel<true, 3, false> + splitk_reduce (images=1, ciblocks>1, splitk_reduce<4> x2)  [16 x 96 -> 192 @ 16 x 16 in f16 and 3 more]
    (48, [96], 192, 16, 16, _PH),     # conv3x3_wgrad_c8i_kernel<true, 3, false> + splitk_reduce (images=2, ciblocks>1, splitk_reduce<4> x2)  [16 x 192+192+192 -> 192 @ 16 x 16 in f16]
    (1, [7], 8, 8, 8, _P32),          # conv3x3_wgrad_direct_kernel + splitk_reduce (splitk_reduce<4> x1)  [2 x 12 -> 24 @ 128 x 128 in f32]
    (8, [7], 8, 8, 8, _P32),          # conv3x3_wgrad_direct_kernel + splitk_reduce (splitk_reduce<4> x2)  [16 x 12 -> 24 @ 128 x 128 in bf16 and 1 more]
    (1, [8], 8, 16, 48, _P32),        # conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce (fixed, tiles=1, splitk_reduce<4> x2)  [2 x 96+96 -> 96 @ 32 x 32 in f32]
    (1, [24], 8, 128, 48, _P32),      # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles=1, splitk_reduce<16> x2)  [2 x 48 -> 24 @ 64 x 64 in f32 and 1 more]
    (1, [24], 8, 16, 48, _P32),       # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles=1, splitk_reduce<4> x2)  [2 x 48 -> 96 @ 32 x 32 in f32]
    (1, [24], 8, 512, 48, _P32),      # conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce (fixed, tiles=1, splitk_reduce<64, 16> x2)  [2 x 24 -> 12 @ 128 x 128 in f32 and 1 more]
    (1, [8], 40, 128, 48, _P32),      # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce (fixed, tiles=1, splitk_reduce<16> x2)  [2 x 48+48 -> 48 @ 64 x 64 in f32]
    (1, [8], 40, 16, 48, _P32),       # conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce (fixed, tiles=1, splitk_reduce<4> x2)  [2 x 96 -> 48 @ 32 x 32 in f32]
    (1, [24], 40, 128, 48, _P32),     # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce (fixed, tiles=1, splitk_reduce<16> x2)  [2 x 24 -> 48 @ 64 x 64 in f32]
    (1, [24], 40, 16, 48, _P32),      # conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce (fixed, tiles=1, splitk_reduce<4> x2)  [2 x 48 -> 48 @ 32 x 32 in f32]
    (1, [8], 8, 12, 8, _P32),         # conv3x3_wgrad_mfma_kernel<1, 2, false> + splitk_reduce (fixed, tiles=1, splitk_reduce<4> x1)  [2 x 192+192+192 -> 192 @ 16 x 16 in f32 and 4 more]
    (16, [1], 8, 32, 512, _P32),      # conv3x3_wgrad_smallcin_kernel + splitk_reduce (bands=4, splitk_reduce<16> x2)  [16 x 1 -> 12 @ 128 x 128 in bf16 and 1 more]
    (2, [1], 8, 32, 512, _P32),       # conv3x3_wgrad_smallcin_kernel + splitk_reduce (bands=4, splitk_reduce<4> x2)  [2 x 1 -> 12 @ 128 x 128 in f32]
]


def _wgrad_plan_ids():
    return [_ops_gpu()._wgrad_plan_case_id(c) for c in WGRAD_PLAN_CASES]


@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=_wgrad_plan_ids())
def test_conv3x3_wgrad_plans_match_fp64(case):
    _ops_gpu().test_conv3x3_wgrad_plan_cases_match_fp64(case)


# ------------------------------------------------------------------------------------------------ InstanceNorm + LeakyReLU
# (backward, N, C, H, W, mode) as in INORM_CASES of tests/test_ops_gpu.py.  Every cell of this model is without affine parameters and without a
# conv bias (slope 0.01): no dgamma / dbeta / dbias_pre, nothing deferred.  The 12-channel cells (no group of 8 channels) and the whole f32
# program run the fp32 kernels of norm.hip, the backward in place over dy; the 128 x 128 planes of the 24-channel cells take a team of 8
# workgroups (2 x 3 items: one round); the rest are the one-workgroup instances at the smallest shapes of INORM_CASES that reach them.
_NOA = dict(affine=False, slope=0.01)
_BF = dict(compute=1, out="c8", z="c8f16", **_NOA)          # the bf16 mode: conv outputs stored as fp16
_FP = dict(compute=2, out="c8", z="c8", **_NOA)             # the fp16 mode
_F32B = dict(**_NOA, inplace=True)
INORM_CASES = [
    (False, 2, 24, 128, 128, dict(compute=1, out="c8", **_NOA, rounds=1)),      # in_fwd_c8_kernel<512, 4, false, true, 0> [T=8 rounds=1]  [16 x 24 @ 128 x 128 in bf16: fp32 z, own statistics]
    (True, 2, 24, 128, 128, dict(_BF, rounds=1)),                               # in_bwd_c8_kernel<512, 4, false, true, 2, 0> [T=8 rounds=1]  [16 x 24 @ 128 x 128 in bf16]
    (False, 2, 16, 12, 20, dict(_FP, stats_slots=16, planar=True)),             # in_apply_fwd_c8_kernel<true, true, true, false> (y)  [16 x 48 @ 32 x 32 in f16]
    (False, 2, 16, 12, 20, dict(_FP, stats_slots=64)),                          # in_apply_fwd_c8_kernel<true, true, true, false>  [16 x 24 @ 64 x 64 in f16]
    (False, 2, 16, 12, 20, dict(_FP, stats_slots=64, pool=True)),               # in_apply_fwd_c8_kernel<true, true, true, true> (pool_y8, pool_arg)  [16 x 48 @ 64 x 64 in f16]
    (False, 2, 16, 12, 20, dict(_FP, stats_slots=256, planar=True)),            # in_stats_finalize_kernel + in_apply_fwd_c8_kernel<true, false, true, false> (y)  [16 x 24 @ 128 x 128 in f16]
    (False, 2, 24, 128, 128, dict(compute=2, out="c8", **_NOA, rounds=1)),      # in_fwd_c8_kernel<512, 4, true, true, 0> [T=8 rounds=1]  [16 x 24 @ 128 x 128 in f16: fp32 z, own statistics]
    (True, 1, 16, 48, 60, dict(_FP, pool=True)),                                # in_bwd_c8_kernel<1024, 4, true, false, 1, 0> (dy_pool)  [16 x 48 @ 64 x 64 in f16]
    (True, 1, 16, 48, 60, _FP),                                                 # in_bwd_c8_kernel<1024, 4, true, false, 1, 0>  [16 x 24 @ 64 x 64 in f16]
    (True, 2, 16, 12, 20, _FP),                                                 # in_bwd_c8_kernel<256, 1, true, false, 1, 0>  [16 x 192 @ 16 x 16 in f16]
    (True, 2, 8, 24, 36, dict(_FP, pool=True)),                                 # in_bwd_c8_kernel<256, 4, true, false, 1, 0> (dy_pool)  [16 x 96 @ 32 x 32 in f16]
    (True, 2, 8, 24, 36, _FP),                                                  # in_bwd_c8_kernel<256, 4, true, false, 1, 0>  [16 x 48 @ 32 x 32 in f16]
    (True, 2, 24, 128, 128, dict(_FP, rounds=1)),                               # in_bwd_c8_kernel<512, 4, true, true, 1, 0> [T=8 rounds=1]  [16 x 24 @ 128 x 128 in f16]
    (False, 1, 3, 120, 136, _NOA),                                              # in_fwd_reg_kernel<16> [threads=256]  [N x 12 @ 128 x 128 in bf16 / f16 / f32]
    (False, 2, 3, 60, 68, _NOA),                                                # in_fwd_reg_kernel<4> [threads=256]  [2 x 24 @ 64 x 64 in f32]
    (False, 2, 3, 28, 36, _NOA),                                                # in_fwd_reg_kernel<4> [threads=64]  [2 x 48 @ 32 x 32 in f32]
    (False, 2, 3, 12, 20, _NOA),                                                # in_fwd_reg_kernel<1> [threads=64]  [2 x 96 @ 16 x 16 in f32]
    (True, 1, 3, 128, 128, _F32B),                                              # in_bwd_reg_kernel<4, true> [threads=1024] (inplace)  [N x 12 @ 128 x 128 in bf16 / f16 / f32]
    (True, 2, 3, 60, 68, _F32B),                                                # in_bwd_reg_kernel<4, true> [threads=256] (inplace)  [2 x 24 @ 64 x 64 in f32]
    (True, 2, 3, 32, 32, _F32B),                                                # in_bwd_reg_kernel<1, true> [threads=256] (inplace)  [2 x 48 @ 32 x 32 in f32]
    (True, 2, 3, 12, 20, _F32B),                                                # in_bwd_reg_kernel<1, true> [threads=64] (inplace)  [2 x 192 @ 16 x 16 in f32]
]


def _inorm_ids():
    return [_ops_gpu()._inorm_case_id(c) for c in INORM_CASES]


@pytest.mark.parametrize("case", INORM_CASES, ids=_inorm_ids())
def test_instnorm_launches_match_fp64(case):
    _ops_gpu().test_instnorm_step_instances_match_fp64(case)


# ------------------------------------------------------------------------------------------------ the weight view
# (Cout, Cin, off, cnt, mode, k_off, K) as in WVIEW_CASES of oracle/layout_reference.py: the transposed view of a WHOLE weight (off = 0,
# cnt = Cin) that ends its consumer's K range (k_off > 0, k_off + Cout = K) -- bottleneck2's weight in process_features_map's gathered dgrad
# [(192, 192, 0, 192, 1, 288, 480)], here with Cout 12 (no multiple of 8) behind 28 channels of somebody else.
WVIEW_CASES = [(12, 8, 0, 8, 1, 28, 40)]


@pytest.mark.parametrize("case", WVIEW_CASES, ids=lambda c: "-".join(map(str, c)))
def test_weight_view_launches_match_the_layout_reference(case):
    """The single launch through tests/test_ops_gpu.py's own test, then the batched launch the step's "pack" program makes
    (mtbc_conv3x3_weight_view_many) over two weights into two destinations: every word of each whole destination against the reference."""
    OPS = _ops_gpu()
    OPS.test_weight_view_matches_the_layout_reference(case)
    items = [(case, OPS._LayoutSrc(OPS._wview_weight(case, salt)), OPS._LayoutDst(OPS._wview_numel(case), torch.float32)) for salt in (1, 2)]
    arr = (L.WViewDesc * len(items))(*[OPS._wview_desc(c, w, dst) for c, w, dst in items])
    L.check(L.load().mtbc_conv3x3_weight_view_many(arr, len(items), ops._s()), "weight_view_many")
    torch.cuda.synchronize()
    for i, (c, w, dst) in enumerate(items):
        name = f"[{i}] {OPS._wview_id(c)}"
        OPS._same_words(name, dst.read(name), OPS._wview_want([(c, w.np)], dst))
        assert w.intact(), f"{name}: the source was written"


# ------------------------------------------------------------------------------------------------ the guards
def _own_keys():
    return SP.table_keys(conv3=CONV3_CASES, wgrad_plan=WGRAD_PLAN_CASES, inorm=INORM_CASES, wview=WVIEW_CASES)


def _borrowed_keys():
    """{"small-op": (op kind, key) of the up-sampling and wide-Linear calls that the fp64 / bit-for-bit cases of tests/test_mt_btsunet_ops_gpu.py make}"""
    OPS, BTS = _ops_gpu(), _bts_ops()
    made = BTS.up2_case_ops() + [op for case in BTS._WIDE_CASES for op in OPS._small_case_ops(case)]
    return {"small-op": {(op.kind, SP._small_op_key(op)) for op in made}}


@pytest.mark.parametrize("program", PROGRAMS, ids=[p[1] for p in PROGRAMS])
def test_mt_btsunet_programs_launch_only_reference_tested_instances(program):
    """Every coverage key of the Multi_BTSUNet step program -- kernel instances AND the branches the arguments select, as
    tests/step_programs.py keys them -- is the key of a call that an element-wise reference test makes: the tables of tests/test_ops_gpu.py
    and tests/test_loss_launches_gpu.py, the rows of this module, and for the up-sampling and the wide Linear the cases of tests/test_mt_btsunet_ops_gpu.py.
    The print-out is profiles/mt_btsunet_step_keys.txt."""
    SP.assert_only_tested(_survey(program), SP.reference_tested_keys(), _own_keys(), _borrowed_keys(), "tests/test_mt_btsunet_ops_gpu.py")


def test_mt_btsunet_cases_are_all_needed():
    """Every row of this module's tables makes a key that a surveyed program launches, that no table of tests/test_ops_gpu.py makes and that no
    other row makes: no dead and no double rows, and deleting one fails the guard above."""
    SP.assert_rows_needed("tests/test_mt_btsunet_launches_gpu.py", [_survey(p) for p in PROGRAMS], SP.reference_tested_keys(), _own_keys(),
                          [CONV3_CASES, WGRAD_PLAN_CASES, INORM_CASES, WVIEW_CASES])


def test_every_op_kind_of_the_mt_btsunet_programs_is_claimed():
    """The op kinds of the three programs are those tests/test_ops_gpu.py's OP_KIND_COVERED_BY claims, plus the two up-sampling kinds, which
    the first guard of this module claims and every program must hold."""
    SP.assert_op_kinds_claimed([_survey(p) for p in PROGRAMS], claimed_also=("OP_UPSAMPLE2_FWD", "OP_UPSAMPLE2_BWD"),
                               required=(L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD))
