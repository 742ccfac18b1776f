"""C-ABI checks that need no GPU: the library loads, exports every symbol include/mtbc.h declares, and the
ctypes mirrors in _lib.py have exactly the C layout (sizes + a few offsets) of the header's structs."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_library_exports_every_declared_symbol(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(mtbc_[A-Za-z0-9_]+)\s*\(", src))
    assert declared == set(L.EXPORTS), declared ^ set(L.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mtbc_version() == 203
    # header, library and binding agree on the layout version (the binding refuses any other library at load time)
    assert int(re.search(r"#define\s+MTBC_VERSION\s+(\d+)", src).group(1)) == lib.mtbc_version() == L.ABI_VERSION
    assert lib.mtbc_arch() == b"gfx950"
    assert lib.mtbc_strerror(0) == b"ok" and b"workspace" in lib.mtbc_strerror(-3)


def test_ctypes_layout_matches_header(tmp_path):
    structs = {"mtbc_seg": L.Seg, "mtbc_conv3x3_args": L.Conv3x3Args, "mtbc_instnorm_args": L.InstNormArgs,
               "mtbc_maxpool_args": L.MaxPoolArgs, "mtbc_convT_args": L.ConvTArgs, "mtbc_conv1x1_args": L.Conv1x1Args,
               "mtbc_gap_args": L.GapArgs, "mtbc_linear_args": L.LinearArgs, "mtbc_dice_args": L.DiceArgs,
               "mtbc_focal_args": L.FocalArgs, "mtbc_op": L.Op,
               "mtbc_pack_desc": L.PackDesc, "mtbc_head_fuse_args": L.HeadFuseArgs, "mtbc_wview_desc": L.WViewDesc,
               "mtbc_wgrad_plan": L.WgradPlan}
    offs = [("mtbc_conv3x3_args", "workspace_bytes", L.Conv3x3Args.workspace_bytes.offset),
            ("mtbc_conv3x3_args", "w_packed", L.Conv3x3Args.w_packed.offset),
            ("mtbc_instnorm_args", "dgamma", L.InstNormArgs.dgamma.offset),
            ("mtbc_convT_args", "accumulate_dw", L.ConvTArgs.accumulate_dw.offset),
            ("mtbc_convT_args", "compute", L.ConvTArgs.compute.offset),
            ("mtbc_convT_args", "y_type", L.ConvTArgs.y_type.offset),
            ("mtbc_conv3x3_args", "compute", L.Conv3x3Args.compute.offset),
            ("mtbc_conv3x3_args", "operand_layout", L.Conv3x3Args.operand_layout.offset),
            ("mtbc_conv3x3_args", "out_accumulate", L.Conv3x3Args.out_accumulate.offset),
            ("mtbc_pack_desc", "kind", L.PackDesc.kind.offset),
            ("mtbc_dice_args", "gscale_dev", L.DiceArgs.gscale_dev.offset),
            ("mtbc_wgrad_plan", "reduce", L.WgradPlan.reduce.offset),
            ("mtbc_wgrad_plan", "reduce_kernel", L.WgradPlan.reduce_kernel.offset),
            ("mtbc_op", "u", L.Op.u.offset)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in structs:
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for s, f, _ in offs:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, typ in structs.items():
        assert int(got[name]) == C.sizeof(typ), (name, got[name], C.sizeof(typ))
    for s, f, off in offs:
        assert int(got[f"{s}.{f}"]) == off, (s, f)


def test_op_kind_enum_in_sync():
    src = open(HEADER).read()
    body = src[src.index("MTBC_OP_CONV3_FWD = 1"):]
    body = body[:body.index("};")]
    names = [n.strip().split("=")[0].strip() for n in body.replace("\n", " ").split(",") if n.strip()]
    want = ["CONV3_FWD", "CONV3_DGRAD", "CONV3_WGRAD", "CONV3_PACK_FWD", "CONV3_PACK_DGRAD", "IN_FWD", "IN_BWD",
            "POOL_FWD", "POOL_BWD", "CONVT_FWD", "CONVT_DGRAD", "CONVT_WGRAD", "CONV1_FWD", "CONV1_DGRAD", "CONV1_WGRAD",
            "GAP_FWD", "GAP_BWD", "LINEAR_FWD", "LINEAR_BWD", "DICE_FWD", "DICE_BWD", "FOCAL", "LOSS_MIX", "OPTIM",
            "MEMSET", "DICE_COUNTS", "CONV3_PACK_LP", "HEAD_COMBINE", "HEAD_EXPAND", "C8_PACK", "C8_PACK16", "CONV3_WVIEW",
            "SET_STREAM", "EVENT_RECORD", "EVENT_WAIT", "IN_DPARAM"]
    assert names == ["MTBC_OP_" + w for w in want]
    for i, w in enumerate(want, start=1):
        assert getattr(L, "OP_" + w) == i


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from multi_task_breast_cancer_amd.nets import MTnnUNet
    from multi_task_breast_cancer_amd.criterions import DiceLoss, FocalLoss
    m = MTnnUNet(1, 1, 3)
    with pytest.raises(L.MtbcError):
        m(torch.rand(1, 1, 64, 64))
    with pytest.raises(L.MtbcError):
        DiceLoss()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(L.MtbcError):
        FocalLoss()(torch.zeros(2, 3), torch.zeros(2, 3))


def test_library_is_loaded_after_torch():
    """_lib.load() must import torch before dlopen: libmtbc_hip.so has to bind to the HIP runtime torch ships, not bring the system one in
    beside it (two runtimes in one process: every launch fails) -- also when the package is imported first, as __graft_entry__.build() does."""
    import subprocess, sys
    code = ("import sys\n"
            "from multi_task_breast_cancer_amd import _lib\n"
            "assert 'torch' not in sys.modules, 'the package import itself stays light'\n"
            "_lib.load()\n"
            "assert 'torch' in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_adam_dynamic_scalars_are_torch_adams_scalar_path(lib):
    """mtbc_optim_dynamic (Adam: kind ADAMW, weight_decay 0) is host arithmetic only (no GPU call): the per-step scalars a replayed (hipGraph) Adam
    launch reads from device memory -- grad_scale, lr / (1 - b1^t), 1 / sqrt(1 - b2^t), and a decay factor of exactly 1 -- with the bias corrections in
    double as torch.optim.Adam's scalar path computes them
    (torch/optim/adam.py: bias_correction1 = 1 - beta1 ** step; step_size = lr / bias_correction1; bias_correction2_sqrt = sqrt(1 - beta2 ** step)),
    the float32 betas / lr of the argument struct widened first.  experiment_init.py:186-187 (Adam, eps 1e-4), training_multitask.py:103."""
    import math
    import numpy as np
    for lr, b1, b2, t, gs in [(1e-4, 0.9, 0.999, 1, 1.0), (3e-4, 0.9, 0.999, 7, 1.0 / 4096.0), (5e-4, 0.8, 0.99, 12345, 0.125), (1e-6, 0.9, 0.999, 2_000_000, 1.0)]:
        a = L.OptimArgs()
        a.kind, a.weight_decay = L.OPT_ADAMW, 0.0
        a.lr, a.beta1, a.beta2, a.eps, a.grad_scale, a.step = lr, b1, b2, 1e-4, gs, t
        out = (C.c_float * 4)()
        assert lib.mtbc_optim_dynamic(C.byref(a), C.byref(out)) == 0
        lr32, b132, b232 = (float(np.float32(v)) for v in (lr, b1, b2))
        want = (np.float32(gs), np.float32(lr32 / (1.0 - math.pow(b132, t))), np.float32(1.0 / math.sqrt(1.0 - math.pow(b232, t))))
        assert tuple(np.float32(v) for v in out[:3]) == want, (lr, b1, b2, t, list(out), want)
        assert out[3] == 1.0
    bad = L.OptimArgs()
    bad.kind, bad.step = L.OPT_ADAMW, 0
    assert lib.mtbc_optim_dynamic(C.byref(bad), C.byref((C.c_float * 4)())) != 0       # t >= 1, as mtbc_optim_step


# (op, N, segs, Cout, H, W, mode) -> the instance mtbc_conv3x3_kernel_name names: the selection of plan_igemm / plan_wgrad made visible.
# mode: compute, c8 (channel-blocked operands), out_c8 / out_fp16 (forward output channel-blocked / stored as fp16), bias, in-kernel reduce
_BF16_O3 = dict(compute=1, c8=True, out_c8=True, out_fp16=True)
_BF16 = dict(compute=1, c8=True)
_F16_O1 = dict(compute=2, c8=True, out_c8=True)
_F16 = dict(compute=2, c8=True)
SELECTION = [
    # configs[1] (U-Net++, bf16, N = 32): forward into fp16-stored outputs, dgrad / gathered-dgrad outputs in fp32 planes
    ("fwd", 32, [24], 24, 256, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>"),
    ("fwd", 32, [48], 48, 128, 128, _BF16_O3, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"),
    ("fwd", 32, [96], 96, 64, 64, _BF16_O3, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"),
    ("fwd", 32, [192], 192, 32, 32, _BF16_O3, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"),
    ("fwd", 32, [384], 384, 16, 16, _BF16_O3, "conv3x3_igemm_c8_ring_kernel<3, 1, false, 3, 3>"),
    ("fwd", 32, [384, 384, 384], 512, 16, 16, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>"),
    ("fwd", 32, [24, 24], 24, 256, 256, _BF16, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>"),
    ("dgrad", 32, [24], 24, 256, 256, _BF16, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 0>"),
    ("dgrad", 32, [48], 48, 128, 128, _BF16, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 0>"),
    ("dgrad", 32, [384, 384, 384], 512, 16, 16, _BF16, "conv3x3_igemm_c8_kernel<3, 1, false, 4, 0>"),
    ("dgrad", 32, [384], 384, 16, 16, _BF16, "conv3x3_igemm_c8_ring_kernel<3, 1, false, 0, 3>"),
    ("wgrad", 32, [24], 24, 256, 256, _BF16, "conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce"),
    ("wgrad", 32, [48, 48], 48, 128, 128, dict(_BF16, bias=False), "conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce"),
    ("wgrad", 32, [48, 48], 48, 128, 128, dict(_BF16, in_kernel_reduce=True), "conv3x3_wgrad_c8w_kernel<false, 3, true> + splitk_fixup"),
    ("wgrad", 32, [384], 384, 16, 16, dict(_BF16, bias=False), "conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce"),
    ("wgrad", 1, [64], 48, 16, 16, dict(_BF16, bias=False), "conv3x3_wgrad_c8i_kernel<false, 3, false>"),         # one split: stored into dw
    ("fwd", 32, [1], 24, 256, 256, _BF16_O3, "conv3x3_stem_fwd_c8_kernel<true>"),
    ("wgrad", 32, [1], 24, 256, 256, dict(_BF16, bias=False), "conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce"),
    # configs[4] (fp16, N = 16, 512 x 512): conv outputs in fp16 channel-blocked (O8 = 1)
    ("fwd", 16, [24], 24, 512, 512, _F16_O1, "conv3x3_igemm_c8_kernel<2, 0, true, 8, 1>"),
    ("fwd", 16, [48], 48, 256, 256, _F16_O1, "conv3x3_igemm_c8_kernel<3, 0, true, 4, 1>"),
    ("fwd", 16, [96, 96], 96, 32, 32, _F16_O1, "conv3x3_igemm_c8_ring_kernel<3, 0, true, 1, 3>"),
    ("dgrad", 16, [24], 24, 512, 512, _F16, "conv3x3_igemm_c8_kernel<2, 0, true, 8, 0>"),
    ("wgrad", 16, [24], 24, 512, 512, dict(_F16, bias=False), "conv3x3_wgrad_c8_kernel<true, 0> + splitk_reduce"),
    # fp32 parity mode (N = 32): the DMA kernels, 2-slot ring
    ("fwd", 32, [24], 24, 256, 256, {}, "conv3x3_igemm_dma_kernel<2, 0, 2>"),
    ("fwd", 32, [48], 48, 128, 128, {}, "conv3x3_igemm_dma_kernel<3, 0, 2>"),
    ("dgrad", 32, [384, 384, 384], 512, 16, 16, {}, "conv3x3_igemm_dma_kernel<3, 1, 2>"),
    ("fwd", 32, [384, 384, 384], 512, 16, 16, {}, "conv3x3_igemm_dma_kernel<2, 1, 2>"),
    ("fwd", 32, [384], 384, 16, 16, {}, "conv3x3_igemm_dma_kernel<1, 1, 2>"),
    ("fwd", 5, [32], 80, 8, 8, {}, "conv3x3_igemm_kernel<1, 2>"),                     # 2 blocks of 4 images: MT lowered to 1
    ("wgrad", 32, [24], 24, 256, 256, {}, "conv3x3_wgrad_mfma_kernel<0, 2, true> + splitk_reduce + channel_sums"),
    ("wgrad", 32, [48], 48, 128, 128, {}, "conv3x3_wgrad_mfma_kernel<0, 3, true> + splitk_reduce + channel_sums"),
    ("wgrad", 32, [96], 96, 64, 64, {}, "conv3x3_wgrad_mfma_kernel<0, 2, false> + splitk_reduce + channel_sums"),
    ("fwd", 32, [1], 24, 256, 256, {}, "conv3x3_stem_fwd_kernel"),
    ("wgrad", 32, [1], 24, 256, 256, {}, "conv3x3_wgrad_smallcin_kernel + splitk_reduce + channel_sums"),
    # 16-bit operands in fp32 planes (the planar-staging kernels)
    ("fwd", 2, [48], 48, 128, 128, dict(compute=1), "conv3x3_igemm_lp_kernel<1, 0, false>"),
    ("wgrad", 2, [48], 48, 128, 128, dict(compute=2), "conv3x3_wgrad_lp2_kernel<true> + splitk_reduce + channel_sums"),
    # edges: ntiles * mblocks just below / at 512 lowers MT (48 channels = 3 tiles; 32 x 8k maps: ntiles = N * k)
    ("fwd", 7, [48], 48, 584, 32, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>"),      # 511 tiles
    ("fwd", 8, [48], 48, 512, 32, _BF16_O3, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"),      # 512
    ("fwd", 7, [48], 48, 128, 128, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>"),     # 448
    ("fwd", 8, [48], 48, 128, 128, _BF16_O3, "conv3x3_igemm_c8_kernel<3, 0, false, 4, 3>"),     # 512
    ("fwd", 7, [48], 48, 584, 32, {}, "conv3x3_igemm_dma_kernel<2, 0, 2>"),
    ("fwd", 8, [48], 48, 512, 32, {}, "conv3x3_igemm_dma_kernel<3, 0, 2>"),
    # t16 * mblocks at 2048 switches to the 8-wave blocks (MT = 2, 256 x 256: t16 = 128 N)
    ("fwd", 15, [32], 32, 256, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>"),
    ("fwd", 16, [32], 32, 256, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>"),
    ("fwd", 16, [32], 32, 240, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 4, 3>"),    # H = 240: t16 = 1920
    ("fwd", 16, [32], 32, 248, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>"),    # H = 248: a ragged 16-row tile, t16 = 2048
    ("fwd", 16, [32], 32, 264, 256, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 0, false, 8, 3>"),    # H not a multiple of 16
    # the ring kernel at ntiles * mb = 256 / 257 (16 x 16 maps: ntiles = N; 48 channels: mb = 1; reads >= 96 channels)
    ("fwd", 256, [96], 48, 16, 16, _BF16_O3, "conv3x3_igemm_c8_ring_kernel<3, 1, false, 3, 3>"),
    ("fwd", 257, [96], 48, 16, 16, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>"),
    ("fwd", 256, [64], 48, 16, 16, _BF16_O3, "conv3x3_igemm_c8_kernel<2, 1, false, 4, 3>"),     # reads < 96 channels: never the ring
    # 8 x 8 maps, N % 4 != 0 (4 images per block)
    ("fwd", 5, [32], 80, 8, 8, _BF16_O3, "conv3x3_igemm_c8_kernel<1, 2, false, 4, 3>"),
    ("dgrad", 6, [64, 64], 320, 8, 8, _F16, "conv3x3_igemm_c8_kernel<1, 2, true, 4, 0>"),
    ("fwd", 33, [320], 320, 8, 8, _F16_O1, "conv3x3_igemm_c8_kernel<1, 2, true, 4, 1>"),
]


@pytest.mark.parametrize("op,N,segs,Cout,H,W,mode,want", SELECTION)
def test_conv3x3_kernel_selection(lib, op, N, segs, Cout, H, W, mode, want):
    """mtbc_conv3x3_kernel_name (host only: the dummy tensor pointers are never dereferenced) names the instance each call launches;
    a change of the selection shows up here, in review."""
    from multi_task_breast_cancer_amd import ops
    kind = {"fwd": L.OP_CONV3_FWD, "dgrad": L.OP_CONV3_DGRAD, "wgrad": L.OP_CONV3_WGRAD}[op]
    assert ops.conv3x3_case_kernel(kind, N, segs, Cout, H, W, **mode) == want


def test_conv3x3_kernel_name_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    buf = C.create_string_buffer(256)
    a = ops.conv3x3_case_args(L.OP_CONV3_FWD, 2, [8], 8, 8, 10, **_BF16)           # channel-blocked operands need W % 4 == 0
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_FWD, buf, 256) == -5
    a = ops.conv3x3_case_args(L.OP_CONV3_FWD, 2, [8], 12, 16, 16, **_BF16_O3)      # channel-blocked output needs Cout % 8 == 0
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_FWD, buf, 256) == -2
    a = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, 2, [48], 48, 32, 32, **_BF16)
    a.workspace_bytes -= 4                                                         # one float short
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_WGRAD, buf, 256) == -3
    a = ops.conv3x3_case_args(L.OP_CONV3_FWD, 2, [48], 48, 32, 32, **_BF16)
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_FWD, buf, 256) == 0
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_PACK_FWD, buf, 256) == -2
    assert lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_FWD, buf, 8) == -2        # shorter than the name
    assert lib.mtbc_conv3x3_kernel_name(None, L.OP_CONV3_FWD, buf, 256) == -2


# (N, segs, Cout, H, W, mode) -> the fields of mtbc_wgrad_plan that the kernel family reads, worked out by hand from plan_wgrad
# (csrc/conv3x3.hip) for one launch of each family; a field not named must be 0 (reduce_kernel: empty)
_F = dict(compute=1, c8=True, bias=False)
WGRAD_PLANS = [
    # 32 x 32 kernel: 2 x 11 tiles x 3 images = 66; 6 x 12 channel blocks -> 1024 / 72 = 14 splits asked (< 16: dealt fixed), 5 tiles each, the last split 1
    (3, [192, 192], 192, 44, 64, _F, "conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce",
     dict(nsplit=14, total_tiles=66, tiles_per_split=5, tiles_x=2, tiles_y=11, coblocks=6, ciblocks=12, reduce=1, reduce_kernel=b"splitk_reduce<4>")),
    # ... 1024 tiles, 3 x 2 channel blocks -> 170 splits asked: 168 (a multiple of 8), dealt evenly
    (8, [48], 96, 128, 128, _F, "conv3x3_wgrad_c8_kernel<false, 0> + splitk_reduce",
     dict(nsplit=168, total_tiles=1024, tiles_per_split=-1, tiles_x=4, tiles_y=32, coblocks=3, ciblocks=2, reduce=1, reduce_kernel=b"splitk_reduce<16>")),
    # ... the in-kernel reduction: 16 tiles, 36 channel blocks -> 28 splits asked, 16 there are; a tree of 2 levels, fan-in 4
    (2, [192], 192, 32, 32, dict(compute=1, c8=True, in_kernel_reduce=True), "conv3x3_wgrad_c8_kernel<false, 0> + splitk_fixup",
     dict(nsplit=16, total_tiles=16, tiles_per_split=1, tiles_x=1, tiles_y=8, coblocks=6, ciblocks=6, reduce=2, fix_levels=2, fix_fanin=4)),
    # wide-block kernel: 12 strips x 8 images = 96 > the budget of 512 / (2 x 3) = 85 blocks: ONE segment of all 5 steps per strip
    (8, [192], 96, 20, 384, _F, "conv3x3_wgrad_c8w_kernel<false, 3, false> + splitk_reduce",
     dict(nsplit=96, total_tiles=96, tiles_per_split=1, tiles_x=12, tiles_y=5, coblocks=2, ciblocks=3, cit=4, segs=1, seg_tiles=5, depth=1, reduce=1,
          reduce_kernel=b"splitk_reduce<16>")),
    # image-tile kernel: 8 x 5 channel blocks -> 256 / 40 = 6 ranges of 3 images, the last one 1
    (16, [384], 384, 16, 16, _F, "conv3x3_wgrad_c8i_kernel<false, 3, false> + splitk_reduce",
     dict(nsplit=6, total_tiles=16, tiles_per_split=3, coblocks=8, ciblocks=5, cit=5, segs=6, seg_tiles=3, geo=1, reduce=1, reduce_kernel=b"splitk_reduce<4>")),
    # ... 16 x 15 channel blocks fill the chip: ONE range of all 12 images, stored straight into dw
    (12, [384, 384, 384], 512, 16, 16, _F, "conv3x3_wgrad_c8i_kernel<false, 2, false>",
     dict(nsplit=1, total_tiles=12, tiles_per_split=12, coblocks=16, ciblocks=15, cit=5, segs=1, seg_tiles=12, geo=1, reduce=0)),
    # the stem: 16 bands per 256 x 256 image
    (2, [1], 24, 256, 256, _F, "conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce", dict(nsplit=32, bands=16, reduce=1, reduce_kernel=b"splitk_reduce<4>")),
    # fp32 MFMA kernel: 2 x 16 tiles x 8 images = 256; 48-channel output blocks, 3 input blocks -> 512 / 3 = 170 splits asked: 2 tiles each, 128 splits
    (8, [96], 48, 64, 64, dict(), "conv3x3_wgrad_mfma_kernel<0, 3, false> + splitk_reduce + channel_sums",
     dict(nsplit=128, total_tiles=256, tiles_per_split=2, tiles_x=2, tiles_y=16, coblocks=1, ciblocks=3, reduce=1, reduce_kernel=b"splitk_reduce<16>")),
    # small-Cin kernel: 4 bands per image from 128 x 128 on
    (4, [1], 24, 256, 256, dict(), "conv3x3_wgrad_smallcin_kernel + splitk_reduce + channel_sums", dict(nsplit=16, bands=4, reduce=1, reduce_kernel=b"splitk_reduce<4>")),
    # direct kernel: at most 16 splits; split s takes images s, s + 16
    (24, [7], 8, 8, 8, dict(bias=False), "conv3x3_wgrad_direct_kernel + splitk_reduce", dict(nsplit=16, images_per_split=2, reduce=1, reduce_kernel=b"splitk_reduce<4>")),
]


@pytest.mark.parametrize("N,segs,Cout,H,W,mode,name,want", WGRAD_PLANS, ids=[f"{r[6].split('<')[0].split(' ')[0]}-{r[0]}x{sum(r[1])}-{r[2]}@{r[3]}x{r[4]}" for r in WGRAD_PLANS])
def test_conv3x3_wgrad_plan_is_the_hand_computed_plan(lib, N, segs, Cout, H, W, mode, name, want):
    """mtbc_conv3x3_wgrad_plan (host only) reports what the launch hands its kernel: against plans worked out by hand, field by field."""
    from multi_task_breast_cancer_amd import ops
    a = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, N, segs, Cout, H, W, **mode)
    assert ops.conv3x3_kernel_name(a, L.OP_CONV3_WGRAD) == name
    plan = ops.conv3x3_wgrad_plan(a)
    got = {f: getattr(plan, f) for f, _ in L.WgradPlan._fields_}
    assert got == dict({f: (b"" if f == "reduce_kernel" else 0) for f in got}, **want)


def test_conv3x3_wgrad_plan_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    plan = L.WgradPlan()
    good = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, 2, [48], 48, 32, 32, **_BF16)
    assert lib.mtbc_conv3x3_wgrad_plan(C.byref(good), C.byref(plan)) == 0 and plan.nsplit > 0
    assert lib.mtbc_conv3x3_wgrad_plan(None, C.byref(plan)) == -2
    assert lib.mtbc_conv3x3_wgrad_plan(C.byref(good), None) == -2
    a = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, 2, [48], 48, 32, 32, **_BF16)
    a.H = 0
    assert lib.mtbc_conv3x3_wgrad_plan(C.byref(a), C.byref(plan)) == -1                # bad shape
    a = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, 2, [48], 48, 32, 32, **_BF16)
    a.workspace_bytes -= 4                                                              # one float short
    assert lib.mtbc_conv3x3_wgrad_plan(C.byref(a), C.byref(plan)) == -3
    for op in (L.OP_CONV3_FWD, L.OP_CONV3_DGRAD):                                       # not a weight gradient's arguments: no dw (and no dout)
        a = ops.conv3x3_case_args(op, 2, [48], 48, 32, 32, **_BF16)
        assert lib.mtbc_conv3x3_wgrad_plan(C.byref(a), C.byref(plan)) == -2
    a = ops.conv3x3_case_args(L.OP_CONV3_WGRAD, 2, [1], 24, 32, 32, **_BF16)           # the stem's weight gradient has no dbias
    assert lib.mtbc_conv3x3_wgrad_plan(C.byref(a), C.byref(plan)) == lib.mtbc_conv3x3_kernel_name(C.byref(a), L.OP_CONV3_WGRAD, C.create_string_buffer(256), 256) == -5


# (backward, N, C, H, W, mode) -> what mtbc_instnorm_kernel_name names: the selection of norm.hip / norm_coop.hip made visible where it needs
# no device (planes up to 64 x 64 with a channel-blocked output, the streaming passes, the fp32 kernels).  mode: ops.instnorm_case_args
_IN_BF = dict(compute=1, out="c8", z="c8f16")
_IN_FP = dict(compute=2, out="c8", z="c8")
NORM_SELECTION = [
    # one workgroup per (image, channel group): block sizes at H*W = 64 / 65, 256 / 257, 1024 / 1025, 4096
    (False, 2, 16, 8, 8, _IN_BF, "in_fwd_c8_kernel<64, 1, false, false, 2>"),
    (False, 2, 16, 5, 13, _IN_BF, "in_fwd_c8_kernel<256, 1, false, false, 2>"),
    (False, 2, 16, 16, 16, _IN_BF, "in_fwd_c8_kernel<256, 1, false, false, 2>"),
    (False, 2, 16, 257, 1, _IN_BF, "in_fwd_c8_kernel<256, 4, false, false, 2>"),
    (False, 2, 16, 32, 32, _IN_BF, "in_fwd_c8_kernel<256, 4, false, false, 2>"),
    (False, 2, 16, 25, 41, _IN_BF, "in_fwd_c8_kernel<1024, 4, false, false, 2>"),
    (False, 2, 16, 64, 64, _IN_BF, "in_fwd_c8_kernel<1024, 4, false, false, 2>"),
    (True, 2, 16, 8, 8, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<64, 1, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 5, 13, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<256, 1, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 16, 16, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<256, 1, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 257, 1, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<256, 4, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 32, 32, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<256, 4, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 25, 41, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<1024, 4, false, false, 2, 1> + in_dparam_kernel"),
    (True, 2, 16, 64, 64, dict(_IN_BF, dy="c8"), "in_bwd_c8_kernel<1024, 4, false, false, 2, 1> + in_dparam_kernel"),
    # var_of: ZC8 = 0 fp32 planar z, 1 channel-blocked of the output's type, 2 channel-blocked fp16 under a bf16 output;
    #         DY8 = 0 fp32 planar dy, 1 channel-blocked, 2 channel-blocked + an fp32 planar partial
    (False, 2, 16, 16, 16, dict(compute=1, out="c8"), "in_fwd_c8_kernel<256, 1, false, false, 0>"),
    (False, 2, 16, 16, 16, dict(compute=1, out="c8", z="c8"), "in_fwd_c8_kernel<256, 1, false, false, 1>"),
    (False, 2, 16, 16, 16, dict(compute=2, out="c8"), "in_fwd_c8_kernel<256, 1, true, false, 0>"),
    (False, 2, 16, 16, 16, _IN_FP, "in_fwd_c8_kernel<256, 1, true, false, 1>"),
    (True, 2, 16, 16, 16, dict(compute=1, out="c8", affine=False), "in_bwd_c8_kernel<256, 1, false, false, 0, 0>"),
    (True, 2, 16, 16, 16, dict(compute=1, out="c8", n_extra=1), "in_bwd_c8_kernel<256, 1, false, false, 0, 0> + in_dparam_kernel"),
    (True, 2, 16, 16, 16, dict(_IN_BF, dy="c8", n_extra=1), "in_bwd_c8_kernel<256, 1, false, false, 2, 2> + in_dparam_kernel"),
    (True, 2, 16, 16, 16, dict(_IN_FP, dy="c8", n_extra=1, defer=True), "in_bwd_c8_kernel<256, 1, true, false, 1, 2>"),
    (True, 2, 16, 16, 16, dict(_IN_FP, dy=None, rank1=True, rank1_grads=True, affine=False, dbias=True),
     "in_bwd_c8_kernel<256, 1, true, false, 1, 0> + in_r1_finalize_kernel + in_dparam_kernel"),
    # the streaming passes: every workgroup finalizes its own channels up to 64 pixel subsets, a finalize launch above
    (False, 2, 16, 64, 64, dict(_IN_BF, stats_slots=64), "in_apply_fwd_c8_kernel<false, true, true, false>"),
    (False, 2, 16, 64, 64, dict(_IN_BF, stats_slots=65), "in_stats_finalize_kernel + in_apply_fwd_c8_kernel<false, false, true, false>"),
    (False, 2, 16, 64, 64, dict(_IN_BF, stats_slots=64, pool=True), "in_apply_fwd_c8_kernel<false, true, true, true>"),
    (False, 2, 16, 64, 64, dict(_IN_BF, stats_slots=65, pool=True, planar16=True), "in_stats_finalize_kernel + in_apply_fwd_c8_kernel<false, false, true, true>"),
    (False, 2, 16, 512, 512, dict(_IN_FP, stats_slots=4096), "in_stats_finalize_kernel + in_apply_fwd_c8_kernel<true, false, true, false>"),
    (False, 2, 16, 64, 64, dict(compute=1, out="c8", z="c8", stats_slots=1), "in_apply_fwd_c8_kernel<false, true, false, false>"),
    (True, 2, 16, 64, 64, dict(_IN_BF, dy="c8", stats_slots=65), "in_bstats_finalize_kernel + in_apply_bwd_c8_kernel<false, true> + in_dparam_kernel"),
    # the fp32 kernels of norm.hip (H*W % 4 == 0 and 16-byte aligned: the register-resident planes)
    (False, 2, 5, 16, 16, {}, "in_fwd_reg_kernel<1> [threads=64]"),
    (False, 2, 5, 32, 32, {}, "in_fwd_reg_kernel<4> [threads=64]"),
    (False, 2, 5, 64, 64, {}, "in_fwd_reg_kernel<4> [threads=256]"),
    (False, 2, 5, 128, 128, {}, "in_fwd_reg_kernel<16> [threads=256]"),
    (False, 2, 5, 256, 256, {}, "in_fwd_reg_kernel<16> [threads=1024]"),
    (False, 2, 5, 256, 256, dict(compute=1, out="p16"), "in_fwd_reg_kernel<16> [threads=1024]"),
    (False, 2, 5, 512, 512, {}, "in_fwd_chunk_stats_kernel + in_fwd_chunk_apply_kernel"),
    (False, 2, 5, 512, 512, dict(chunk_ws=False), "in_fwd_stream_kernel [threads=1024]"),
    (False, 2, 5, 7, 9, {}, "in_fwd_stream_kernel [threads=256]"),
    (True, 2, 5, 16, 16, {}, "in_bwd_reg_kernel<1, true> [threads=64] + in_dparam_kernel"),
    (True, 2, 5, 32, 32, dict(inplace=True), "in_bwd_reg_kernel<1, true> [threads=256] + in_dparam_kernel"),
    (True, 2, 5, 64, 64, dict(affine=False), "in_bwd_reg_kernel<4, true> [threads=256]"),
    (True, 2, 5, 64, 64, dict(affine=False, dbias=True, n_extra=2), "in_bwd_reg_kernel<4, true> [threads=256] + in_dparam_kernel"),
    (True, 2, 5, 128, 128, {}, "in_bwd_reg_kernel<4, true> [threads=1024] + in_dparam_kernel"),
    (True, 2, 5, 128, 256, {}, "in_bwd_reg_kernel<8, true> [threads=1024] + in_dparam_kernel"),
    (True, 2, 5, 256, 256, dict(compute=2, out="p16"), "in_bwd_reg_kernel<16, false> [threads=1024] + in_dparam_kernel"),
    (True, 2, 5, 512, 512, {}, "in_bwd_kernel<true> [threads=1024] + in_dparam_kernel"),
    (True, 2, 5, 7, 9, {}, "in_bwd_kernel<false> [threads=64] + in_dparam_kernel"),
]


@pytest.mark.parametrize("backward,N,Cc,H,W,mode,want", NORM_SELECTION)
def test_instnorm_kernel_selection(lib, backward, N, Cc, H, W, mode, want):
    """mtbc_instnorm_kernel_name (the dummy tensor pointers are never dereferenced) names every launch of a call; a change of the
    selection shows up here, in review."""
    from multi_task_breast_cancer_amd import ops
    assert ops.instnorm_case_kernel(backward, N, Cc, H, W, **mode) == want


def test_instnorm_kernel_name_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    buf = C.create_string_buffer(512)
    name = lambda a, b: lib.mtbc_instnorm_kernel_name(C.byref(a), b, buf, 512)      # noqa: E731
    assert name(ops.instnorm_case_args(False, 2, 12, 16, 16, **_IN_BF), 0) == -2                           # C % 8
    assert name(ops.instnorm_case_args(True, 2, 12, 16, 16, **dict(_IN_BF, dy="c8")), 1) == -5             # ... backward: no team size
    assert name(ops.instnorm_case_args(False, 2, 16, 16, 16, **dict(_IN_BF, planar16=True)), 0) == -5      # y16 beside y8 without stats_partial
    assert name(ops.instnorm_case_args(False, 2, 16, 16, 16, **dict(_IN_BF, planar16=True, stats_slots=4)), 0) == 0
    assert name(ops.instnorm_case_args(True, 2, 16, 16, 16, **dict(_IN_BF, dy="c8", rank1=True, stats_slots=4)), 1) == -5      # rank-1 with stats_partial
    assert name(ops.instnorm_case_args(True, 2, 16, 16, 16, **dict(_IN_BF, dy="c8", pool=True, stats_slots=4)), 1) == -5
    assert name(ops.instnorm_case_args(True, 2, 16, 16, 16, **dict(_IN_BF, dy=None)), 1) == -2             # no gradient at all
    assert name(ops.instnorm_case_args(True, 2, 16, 16, 16, **dict(_IN_BF, dy="c8", affine=False, defer=True)), 1) == -5       # nothing to defer
    assert name(ops.instnorm_case_args(True, 2, 5, 16, 16, **dict(defer=True)), 1) == -5                   # the fp32 kernels do not defer
    assert name(ops.instnorm_case_args(True, 2, 5, 16, 16, **dict(rank1=True)), 1) == -5                   # rank-1 without dz8
    a = ops.instnorm_case_args(True, 2, 16, 16, 16, **dict(_IN_BF, dy="c8"))
    a.workspace_bytes = 2 * 16 * 4 * 4 - 4                                                                 # one float short of N*C*(3 + T)
    assert name(a, 1) == -3
    a = ops.instnorm_case_args(False, 2, 16, 16, 16, **_IN_BF)
    assert name(a, 0) == 0 and buf.value == b"in_fwd_c8_kernel<256, 1, false, false, 2>"
    assert lib.mtbc_instnorm_kernel_name(C.byref(a), 0, buf, 8) == -2                                      # shorter than the name
    assert lib.mtbc_instnorm_kernel_name(None, 0, buf, 512) == -1 and lib.mtbc_instnorm_kernel_name(None, 1, buf, 512) == -1
    import torch
    if not torch.cuda.is_available():          # planes above 64 x 64: the team plan needs the device, as the launch does
        assert name(ops.instnorm_case_args(False, 2, 24, 256, 256, **_IN_BF), 0) == -5


# (op, (N, Cin, Cout, H, W, k), mode, pair) -> what mtbc_convT_kernel_name names: the selection of convt2.hip and of the ConvT entry points of
# pool_up.hip, one row per instance that tests/test_ops_gpu.py::test_convT_step_instances_match_fp64 compares with fp64, and the edges of
# each rule.  mode: ops.convT_case_args; pair: the OP_CONVT_DGRAD of the same problem right behind the weight gradient.
_CT_B16 = dict(compute=1, dy16=True, x16=True)
_CT_F16 = dict(compute=2, dy16=True, x16=True)
_CT_C8B = dict(compute=1, x_c8=True, y_c8=True)
_CT_C8F = dict(compute=2, x_c8=True, y_c8=True)
_RR = " + splitk_reduce + splitk_reduce"          # the bias-gradient partials, then dW
CONVT_SELECTION = [
    # forward on the 16-bit MFMA: MTC = min(3, Cout / 16 rounded up), lowered until 64 x MTC rows of Cin (rounded up to 32) + 16 halves fit 72 KB
    ("fwd", (3, 96, 48, 8, 16, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<3, false>"),
    ("fwd", (2, 56, 40, 16, 16, 2), _CT_C8F, False, "convT2_fwd_lp_c8_kernel<3, true>"),
    ("fwd", (2, 160, 96, 8, 8, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<3, false>"),        # the last Cin with three tiles
    ("fwd", (2, 192, 96, 8, 8, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<2, false>"),
    ("fwd", (3, 40, 24, 8, 16, 2), _CT_C8F, False, "convT2_fwd_lp_c8_kernel<2, true>"),
    ("fwd", (2, 256, 96, 8, 8, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<2, false>"),        # the last Cin with two
    ("fwd", (2, 288, 96, 8, 8, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<1, false>"),
    ("fwd", (1, 384, 192, 8, 8, 2), _CT_C8B, False, "convT2_fwd_lp_c8_kernel<1, false>"),
    ("fwd", (2, 24, 8, 8, 16, 2), _CT_C8F, False, "convT2_fwd_lp_c8_kernel<1, true>"),
    # forward, fp32 x into channel-blocked y, and fp32 into planes: KI = Cin / 4 rounded up to 8 | 12 | 16
    ("fwd", (2, 32, 40, 16, 16, 2), dict(compute=2, y_c8=True), False, "convT2_fwd_c8_kernel<8, true>"),
    ("fwd", (2, 24, 24, 8, 16, 2), dict(compute=1, y_c8=True), False, "convT2_fwd_c8_kernel<8, false>"),
    ("fwd", (3, 48, 48, 8, 16, 2), dict(compute=1, y_c8=True), False, "convT2_fwd_c8_kernel<12, false>"),
    ("fwd", (2, 36, 8, 16, 16, 2), dict(compute=2, y_c8=True), False, "convT2_fwd_c8_kernel<12, true>"),
    ("fwd", (2, 64, 48, 8, 8, 2), dict(compute=1, y_c8=True), False, "convT2_fwd_c8_kernel<16, false>"),
    ("fwd", (2, 52, 24, 16, 16, 2), dict(compute=2, y_c8=True), False, "convT2_fwd_c8_kernel<16, true>"),
    ("fwd", (2, 20, 12, 8, 16, 2), {}, False, "convT2_fwd_lds_kernel<8>"),
    ("fwd", (3, 48, 48, 16, 16, 2), {}, False, "convT2_fwd_lds_kernel<12>"),
    ("fwd", (2, 64, 40, 8, 8, 2), {}, False, "convT2_fwd_lds_kernel<16>"),
    ("fwd", (2, 32, 1, 8, 8, 2), {}, False, "convT2_fwd_lds_kernel<8>"),                        # a k = 2 head on a 32-pixel-multiple map
    ("fwd", (2, 68, 48, 8, 8, 2), {}, False, "convT_fwd_kernel<2>"),                            # Cin above 64
    ("fwd", (2, 64, 52, 8, 8, 2), {}, False, "convT_fwd_kernel<2>"),                            # Cout above 48
    ("fwd", (2, 20, 12, 6, 10, 2), {}, False, "convT_fwd_kernel<2>"),                           # H * W % 32 != 0
    ("fwd", (2, 64, 1, 6, 10, 4), {}, False, "convT_fwd_kernel<4>"),
    ("fwd", (2, 128, 1, 4, 4, 8), {}, False, "convT_fwd_kernel<8>"),
    # dgrad: 16-bit dy keeps the weights in LDS while Cout % 8 == 0 and 48 rows of 4 Cout + 16 halves fit 104 KB (Cout <= 272)
    ("dgrad", (3, 48, 48, 8, 16, 2), dict(compute=1, dy16=True), False, "convT2_dgrad_lds_kernel<1, 4>"),
    ("dgrad", (2, 64, 256, 8, 8, 2), dict(compute=2, dy16=True), False, "convT2_dgrad_lds_kernel<2, 4>"),
    ("dgrad", (2, 64, 272, 8, 8, 2), dict(compute=2, dy16=True), False, "convT2_dgrad_lds_kernel<2, 4>"),          # the last multiple of 8 that fits
    ("dgrad", (2, 64, 280, 8, 8, 2), dict(compute=2, dy16=True), False, "convT2_dgrad_kernel<2, true, 4>"),
    ("dgrad", (2, 48, 320, 8, 8, 2), dict(compute=1, dy16=True), False, "convT2_dgrad_kernel<1, true, 4>"),
    ("dgrad", (2, 40, 100, 8, 16, 2), dict(compute=1, dy16=True), False, "convT2_dgrad_kernel<1, true, 4>"),       # Cout % 8 != 0, D = 4 from 96
    ("dgrad", (2, 40, 20, 8, 16, 2), dict(compute=1, dy16=True), False, "convT2_dgrad_kernel<1, true, 2>"),
    ("dgrad", (3, 24, 12, 8, 8, 2), dict(compute=2, dy16=True), False, "convT2_dgrad_kernel<2, true, 2>"),
    ("dgrad", (2, 48, 24, 8, 16, 2), {}, False, "convT2_dgrad_kernel<0, false, 2>"),
    ("dgrad", (2, 56, 40, 8, 8, 2), dict(compute=1), False, "convT2_dgrad_kernel<1, false, 2>"),
    ("dgrad", (2, 96, 48, 8, 8, 2), dict(compute=2), False, "convT2_dgrad_kernel<2, false, 2>"),
    ("dgrad", (2, 32, 1, 8, 8, 2), {}, False, "convT_dgrad_kernel<2>"),                         # odd Cout
    ("dgrad", (2, 20, 12, 6, 10, 2), {}, False, "convT_dgrad_kernel<2>"),
    ("dgrad", (2, 64, 1, 6, 10, 4), {}, False, "convT_dgrad_kernel<4>"),
    ("dgrad", (2, 128, 1, 4, 4, 8), {}, False, "convT_dgrad_kernel<8>"),
    # wgrad: splits of at least 8 steps of 32 pixels; x and dy as 16-bit planes: two channel tiles per wave when their count is even,
    # a split's tasks on one XCD from 8 splits
    ("wgrad", (1, 48, 48, 16, 16, 2), _CT_B16, False, "convT2_wgrad16_kernel<1, 2, 2> [splits=1]" + _RR),
    ("wgrad", (3, 64, 16, 16, 24, 2), dict(_CT_F16, bias=False), False, "convT2_wgrad16_kernel<2, 2, 2> [splits>1] + splitk_reduce"),
    ("wgrad", (7, 96, 32, 16, 16, 2), _CT_B16, False, "convT2_wgrad16_kernel<1, 2, 2> [splits>1]" + _RR),          # 7 splits
    ("wgrad", (2, 96, 32, 32, 32, 2), _CT_B16, False, "convT2_wgrad16_kernel<1, 2, 2> [xcd splits>1]" + _RR),      # 8
    ("wgrad", (3, 48, 192, 24, 40, 2), _CT_F16, False, "convT2_wgrad16_kernel<2, 2, 2> [xcd splits>1]" + _RR),
    ("wgrad", (2, 40, 24, 8, 16, 2), _CT_B16, False, "convT2_wgrad16_kernel<1, 1, 4> [splits=1]" + _RR),
    ("wgrad", (3, 56, 40, 16, 24, 2), _CT_F16, False, "convT2_wgrad16_kernel<2, 1, 4> [splits>1]" + _RR),
    ("wgrad", (3, 48, 8, 32, 32, 2), _CT_B16, False, "convT2_wgrad16_kernel<1, 1, 4> [xcd splits>1]" + _RR),
    ("wgrad", (3, 64, 24, 24, 40, 2), _CT_F16, False, "convT2_wgrad16_kernel<2, 1, 4> [xcd splits>1]" + _RR),
    ("wgrad", (3, 48, 24, 16, 24, 2), dict(compute=1, dy16=True), False, "convT2_wgrad_kernel<1, true, 2> [splits>1]" + _RR),
    ("wgrad", (2, 96, 48, 8, 16, 2), dict(compute=2, dy16=True), False, "convT2_wgrad_kernel<2, true, 2> [splits=1]" + _RR),
    ("wgrad", (3, 20, 12, 16, 24, 2), {}, False, "convT2_wgrad_kernel<0, false, 2> [splits>1]" + _RR),
    ("wgrad", (2, 48, 48, 8, 16, 2), dict(compute=1), False, "convT2_wgrad_kernel<1, false, 2> [splits=1]" + _RR),
    ("wgrad", (1, 96, 40, 16, 16, 2), dict(compute=2, bias=False), False, "convT2_wgrad_kernel<2, false, 2> [splits=1] + splitk_reduce"),
    ("wgrad", (2, 32, 1, 8, 16, 2), {}, False, "convT2_wgrad_kernel<0, false, 2> [splits=1]" + _RR),               # a k = 2 head: no parity rule on Cout here
    ("wgrad", (2, 32, 1, 8, 12, 2), {}, False, "convT_wgrad_kernel<2> [splits>1] + splitk_reduce + channel_sums"),    # W % 8 != 0
    ("wgrad", (2, 64, 1, 6, 10, 4), {}, False, "convT_wgrad_kernel<4> [splits>1] + splitk_reduce + channel_sums"),
    ("wgrad", (1, 128, 1, 4, 4, 8), dict(bias=False), False, "convT_wgrad_kernel<8> [splits=1] + splitk_reduce"),
    ("wgrad", (2, 128, 1, 4, 4, 8), dict(bias=False), False, "convT_wgrad_kernel<8> [splits>1] + splitk_reduce"),      # a split per image at least
    ("wgrad", (1, 384, 192, 8, 8, 2), _CT_F16, True, "convT2_wgrad16_kernel<2, 2, 2> [splits=1]" + _RR + " + convT2_dgrad_lds_kernel<2, 4>"),
    # the pair: one launch where Cout is 24 (CT = 1), 48 or 96 (CT = 2; 3 or 6 waves), unless it has fewer than 256 workgroups of more than 8 steps
    ("wgrad", (2, 64, 24, 16, 16, 2), _CT_B16, True, "convT2_bwd_fused_kernel<1, 1, 3, false> [splits>1]" + _RR),
    ("wgrad", (3, 40, 24, 16, 24, 2), dict(_CT_B16, acc_dx=True), True, "convT2_bwd_fused_kernel<1, 1, 3, true> [splits>1]" + _RR),
    ("wgrad", (3, 56, 24, 32, 32, 2), _CT_F16, True, "convT2_bwd_fused_kernel<2, 1, 3, false> [splits>1]" + _RR),
    ("wgrad", (1, 48, 24, 16, 16, 2), dict(_CT_F16, acc_dx=True), True, "convT2_bwd_fused_kernel<2, 1, 3, true> [splits=1]" + _RR),
    ("wgrad", (3, 48, 48, 32, 32, 2), _CT_B16, True, "convT2_bwd_fused_kernel<1, 2, 3, false> [splits>1]" + _RR),
    ("wgrad", (2, 96, 48, 32, 32, 2), dict(_CT_B16, acc_dx=True), True, "convT2_bwd_fused_kernel<1, 2, 3, true> [splits>1]" + _RR),
    ("wgrad", (3, 48, 48, 16, 24, 2), _CT_F16, True, "convT2_bwd_fused_kernel<2, 2, 3, false> [splits>1]" + _RR),
    ("wgrad", (2, 96, 48, 8, 16, 2), dict(_CT_F16, acc_dx=True, bias=False), True, "convT2_bwd_fused_kernel<2, 2, 3, true> [splits=1] + splitk_reduce"),
    ("wgrad", (2, 96, 48, 16, 16, 2), dict(_CT_F16, acc_dx=True), True, "convT2_bwd_fused_kernel<2, 2, 3, true> [splits>1]" + _RR),
    ("wgrad", (1, 192, 96, 8, 8, 2), _CT_B16, True, "convT2_bwd_fused_kernel<1, 2, 6, false> [splits=1]" + _RR),
    ("wgrad", (3, 96, 96, 16, 24, 2), dict(_CT_B16, acc_dx=True), True, "convT2_bwd_fused_kernel<1, 2, 6, true> [splits>1]" + _RR),
    ("wgrad", (3, 64, 96, 24, 40, 2), _CT_F16, True, "convT2_bwd_fused_kernel<2, 2, 6, false> [splits>1]" + _RR),
    ("wgrad", (2, 192, 96, 8, 16, 2), dict(_CT_F16, acc_dx=True), True, "convT2_bwd_fused_kernel<2, 2, 6, true> [splits=1]" + _RR),
    ("wgrad", (32, 48, 48, 128, 128, 2), _CT_B16, True, "convT2_bwd_fused_kernel<1, 2, 3, false> [splits>1]" + _RR),                  # the bench: 256 workgroups
    ("wgrad", (32, 192, 96, 32, 32, 2), _CT_B16, True, "convT2_wgrad16_kernel<1, 2, 2> [xcd splits>1]" + _RR + " + convT2_dgrad_lds_kernel<1, 4>"),   # 128 of 32 steps
    ("wgrad", (3, 48, 192, 32, 32, 2), _CT_B16, True, "convT2_wgrad16_kernel<1, 2, 2> [xcd splits>1]" + _RR + " + convT2_dgrad_lds_kernel<1, 4>"),    # 12 waves
    ("wgrad", (2, 64, 320, 8, 16, 2), _CT_B16, True, "convT2_wgrad16_kernel<1, 2, 2> [splits=1]" + _RR + " + convT2_dgrad_kernel<1, true, 4>"),
    ("wgrad", (3, 48, 48, 16, 24, 2), {}, True, "convT2_wgrad_kernel<0, false, 2> [splits>1]" + _RR + " + convT2_dgrad_kernel<0, false, 2>"),
    ("wgrad", (3, 320, 320, 8, 16, 2), dict(compute=1), True, "convT2_wgrad_kernel<1, false, 2> [splits>1]" + _RR + " + convT2_dgrad_kernel<1, false, 2>"),
    ("wgrad", (3, 48, 48, 16, 24, 2), dict(compute=1, dy16=True), True,                               # fp32 x: never fused
     "convT2_wgrad_kernel<1, true, 2> [splits>1]" + _RR + " + convT2_dgrad_lds_kernel<1, 4>"),
]
_CT_OPS = {"fwd": L.OP_CONVT_FWD, "dgrad": L.OP_CONVT_DGRAD, "wgrad": L.OP_CONVT_WGRAD}


@pytest.mark.parametrize("op,shape,mode,pair,want", CONVT_SELECTION)
def test_convT_kernel_selection(lib, op, shape, mode, pair, want):
    """mtbc_convT_kernel_name (host only, no device: the dummy tensor pointers are never dereferenced) names every launch of a call, or of a
    program's WGRAD + DGRAD pair; a change of the selection shows up here, in review."""
    from multi_task_breast_cancer_amd import ops
    assert ops.convT_case_kernel(_CT_OPS[op], *shape, pair=pair, **mode) == want


def test_convT_selection_table_names_every_instance_the_fp64_test_reaches(lib):
    """One row above per distinct launch -- instance and bracketed plan facts -- of tests/test_ops_gpu.py::CONVT_CASES (that table is importable
    without a GPU)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import test_ops_gpu as G
    finally:
        sys.path.pop(0)
    from multi_task_breast_cancer_amd import ops
    named = {part for *_, want in CONVT_SELECTION for part in want.split(" + ")}
    reached = {part for case in G.CONVT_CASES for _, op, a, nxt in G._convT_case_calls(case) for part in ops.convT_kernel_name(a, op, nxt).split(" + ")}
    assert len(reached) >= 50 and not reached - named, sorted(reached - named)


def test_convT_kernel_name_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    F_, D_, W_ = L.OP_CONVT_FWD, L.OP_CONVT_DGRAD, L.OP_CONVT_WGRAD
    buf = C.create_string_buffer(512)
    name = lambda a, op, nxt=None: lib.mtbc_convT_kernel_name(C.byref(a), op, None if nxt is None else C.byref(nxt), buf, 512)      # noqa: E731
    shape = (2, 48, 48, 16, 16, 2)
    a = ops.convT_case_args(D_, *shape, compute=1, dy16=True)
    a.compute = 2                                                                           # 16-bit dy of another type than `compute`
    assert name(a, D_) == -5
    a = ops.convT_case_args(W_, *shape, compute=1, dy16=True)
    a.compute = 0
    assert name(a, W_) == -5
    a = ops.convT_case_args(W_, *shape, compute=1, x16=True)                                # x_type16 without dy_type16
    assert name(a, W_) == -5
    a = ops.convT_case_args(F_, *shape, compute=1, x_c8=True)                               # channel-blocked x with planar y
    assert name(a, F_) == -2
    assert name(ops.convT_case_args(F_, 2, 48, 52, 16, 16, 2, compute=1, y_c8=True), F_) == -5      # channel-blocked y from fp32 x: Cout <= 48
    assert name(ops.convT_case_args(F_, 2, 48, 48, 6, 10, 2, compute=1, x_c8=True, y_c8=True), F_) == -5      # ... H * W % 32
    assert name(ops.convT_case_args(F_, 2, 48, 48, 16, 16, 4, compute=1, y_c8=True), F_) == -5      # ... k = 2 only
    assert name(ops.convT_case_args(W_, *shape, workspace=False), W_) == -3                 # no workspace
    a = ops.convT_case_args(W_, *shape)
    a.workspace_bytes -= 4                                                                  # one float short
    assert name(a, W_) == -3
    wg, dg = ops.convT_case_args(W_, *shape, **_CT_B16), ops.convT_case_args(D_, *shape, **_CT_B16)
    assert name(wg, W_, dg) == 0 and buf.value.startswith(b"convT2_bwd_fused_kernel<1, 2, 3, false>")
    wg.workspace_bytes -= 4                                                                 # the pair leaves the refusal to the weight gradient's call
    assert name(wg, W_, dg) == -3
    a = ops.convT_case_args(F_, *shape)
    assert name(a, F_) == 0 and buf.value == b"convT2_fwd_lds_kernel<12>"
    a.y += 4                                                                                # pointer values count: a misaligned y has no kernel
    assert name(a, F_) == -5
    a = ops.convT_case_args(D_, *shape)
    a.dx += 4                                                                               # ... a misaligned dx takes the generic GEMM
    assert name(a, D_) == 0 and buf.value == b"convT_dgrad_kernel<2>"
    a.dx = None
    assert name(a, D_) == -2
    assert name(ops.convT_case_args(F_, 2, 48, 48, 16, 16, 3), F_) == -5                    # k outside 2, 4, 8
    assert name(ops.convT_case_args(F_, 0, 48, 48, 16, 16, 2), F_) == -1
    a = ops.convT_case_args(F_, *shape)
    assert name(a, L.OP_CONV3_FWD) == -2                                                    # not a ConvT op
    assert lib.mtbc_convT_kernel_name(C.byref(a), F_, None, buf, 8) == -2                   # shorter than the name
    assert lib.mtbc_convT_kernel_name(C.byref(a), F_, None, buf, len(b"convT2_fwd_lds_kernel<12>")) == -2      # no room for the NUL
    assert lib.mtbc_convT_kernel_name(C.byref(a), F_, None, buf, len(b"convT2_fwd_lds_kernel<12>") + 1) == 0
    for op in (F_, D_, W_):
        assert lib.mtbc_convT_kernel_name(None, op, None, buf, 512) == -1                   # NULL args: what the calls return
    assert lib.mtbc_convT_kernel_name(None, W_, C.byref(dg), buf, 512) == -1


# (helper, kind, shape, mode) -> what mtbc_op_kernel_name names: one row per dispatch decision of the max-pool, 1x1, GAP, Linear and fused-head
# calls (pool_up.hip, c8_ops.hip, head_loss.hip) and of the two reducers behind the 1x1 weight gradient (reduce.hip).
_RS = " + c8_rows_sum_kernel"
_PS64, _PS256 = " + plane_sum_k [threads=64] + sum_over_n_k", " + plane_sum_k [threads=256] + sum_over_n_k"
SMALL_OP_SELECTION = [
    ("maxpool", L.OP_POOL_FWD, (3, 16, 16, 16), {}, "maxpool_fwd_kernel"),
    ("maxpool", L.OP_POOL_FWD, (1, 5, 6, 10), {}, "maxpool_fwd_scalar_kernel"),                       # W % 4 != 0
    ("maxpool", L.OP_POOL_FWD, (2, 8, 8, 8), dict(strides=dict(x=8 * 64 + 2)), "maxpool_fwd_scalar_kernel"),      # a batch stride the float4 loads cannot take
    ("maxpool", L.OP_POOL_FWD, (3, 16, 16, 16), dict(compute=1), "maxpool_c8_fwd_kernel<false>"),
    ("maxpool", L.OP_POOL_FWD, (3, 16, 16, 16), dict(compute=2, argmax=True), "maxpool_c8_fwd_kernel<true>"),
    ("maxpool", L.OP_POOL_BWD, (3, 16, 16, 16), {}, "maxpool_bwd_kernel"),
    ("maxpool", L.OP_POOL_BWD, (3, 16, 16, 16), dict(compute=1, acc_dx=True), "maxpool_c8_bwd_kernel<false>"),
    ("maxpool", L.OP_POOL_BWD, (3, 16, 16, 16), dict(compute=2), "maxpool_c8_bwd_kernel<true>"),
    ("conv1x1", L.OP_CONV1_FWD, (2, 16, 10, 32, 36), {}, "conv1x1_fwd_kernel"),
    ("conv1x1", L.OP_CONV1_FWD, (2, 16, 3, 32, 36), dict(compute=1), "conv1x1_c8_fwd_kernel<false>"),
    ("conv1x1", L.OP_CONV1_FWD, (2, 16, 3, 32, 36), dict(compute=2, bias=False), "conv1x1_c8_fwd_kernel<true>"),
    ("conv1x1", L.OP_CONV1_DGRAD, (2, 16, 10, 32, 36), dict(acc_dx=True), "conv1x1_dgrad_kernel"),
    ("conv1x1", L.OP_CONV1_DGRAD, (2, 16, 1, 32, 36), dict(compute=1), "conv1x1_dgrad_kernel"),        # the input gradient never reads x: no channel-blocked form
    ("conv1x1", L.OP_CONV1_WGRAD, (3, 16, 3, 8, 8), dict(bias=False), "conv1x1_wgrad_kernel + splitk_reduce<4>"),
    ("conv1x1", L.OP_CONV1_WGRAD, (32, 16, 3, 8, 8), {}, "conv1x1_wgrad_kernel + splitk_reduce<4>" + _PS64),       # 32 images: still four split lanes
    ("conv1x1", L.OP_CONV1_WGRAD, (33, 16, 3, 8, 8), {}, "conv1x1_wgrad_kernel + splitk_reduce<16>" + _PS64),
    ("conv1x1", L.OP_CONV1_WGRAD, (255, 16, 3, 4, 4), {}, "conv1x1_wgrad_kernel + splitk_reduce<16>" + _PS64),
    ("conv1x1", L.OP_CONV1_WGRAD, (256, 16, 3, 4, 4), {}, "conv1x1_wgrad_kernel + splitk_reduce<64, 16>" + _PS64),
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 1, 63, 64), {}, "conv1x1_wgrad_kernel + splitk_reduce<4>" + _PS64),       # H * W = 4032 < 4096
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 1, 64, 64), {}, "conv1x1_wgrad_kernel + splitk_reduce<4>" + _PS256),
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 3, 64, 64), dict(compute=1), "conv1x1_c8_wgrad_kernel<false> [nblk=1]" + _RS + _RS),
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 3, 89, 92), dict(compute=2, bias=False), "conv1x1_c8_wgrad_kernel<true> [nblk=1]" + _RS),      # 8188 pixels: one block
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 3, 90, 92), dict(compute=2, bias=False), "conv1x1_c8_wgrad_kernel<true> [nblk>1]" + _RS),      # 8280 = 2 chunks of 4140
    ("conv1x1", L.OP_CONV1_WGRAD, (1, 8, 1, 248, 512), dict(compute=1), "conv1x1_c8_wgrad_kernel<false> [nblk>1]" + _RS + _RS),          # 31 blocks
    ("conv1x1", L.OP_CONV1_WGRAD, (1, 8, 1, 256, 512), dict(compute=1), "conv1x1_c8_wgrad_kernel<false> [nblk=32]" + _RS + _RS),         # the cap, first reached
    ("conv1x1", L.OP_CONV1_WGRAD, (1, 8, 1, 512, 512), dict(compute=2), "conv1x1_c8_wgrad_kernel<true> [nblk=32]" + _RS + _RS),
    ("gap", L.OP_GAP_FWD, (3, 5, 5, 7), {}, "gap_fwd_kernel"),
    ("gap", L.OP_GAP_BWD, (3, 5, 5, 7), {}, "gap_bwd_kernel"),
    ("linear", L.OP_LINEAR_FWD, (11, 70, 13), dict(relu=True), "linear_fwd_kernel"),
    ("linear", L.OP_LINEAR_BWD, (11, 70, 13), dict(relu=True), "linear_mask_kernel + linear_dx_kernel [Out>=8] + linear_dw_kernel [N>=8]"),
    ("linear", L.OP_LINEAR_BWD, (7, 70, 7), {}, "linear_dx_kernel + linear_dw_kernel"),
    ("linear", L.OP_LINEAR_BWD, (8, 70, 7), {}, "linear_dx_kernel + linear_dw_kernel [N>=8]"),
    ("linear", L.OP_LINEAR_BWD, (7, 70, 8), {}, "linear_dx_kernel [Out>=8] + linear_dw_kernel"),
    ("linear", L.OP_LINEAR_BWD, (16, 512, 256), dict(relu=True, dx=False), "linear_mask_kernel + linear_dw_kernel [N>=8]"),
    ("linear", L.OP_LINEAR_BWD, (3, 256, 3), dict(dx=False), "linear_dw_kernel"),
    ("head", L.OP_HEAD_COMBINE, (32, 16, 1, 2), {}, "head_combine_kernel"),
    ("head", L.OP_HEAD_EXPAND, (32, 16, 3, 8), dict(bT=False, db1=False), "head_expand_dwT_kernel + head_expand_small_kernel"),
]


@pytest.mark.parametrize("helper,kind,shape,mode,want", SMALL_OP_SELECTION)
def test_small_op_kernel_selection(lib, helper, kind, shape, mode, want):
    """mtbc_op_kernel_name (host only, no device: the dummy tensor pointers are never dereferenced) names every launch of a max-pool, 1x1
    convolution, GAP, Linear or fused-head call; a change of the selection shows up here, in review."""
    from multi_task_breast_cancer_amd import ops
    assert ops.op_kernel_name(getattr(ops, helper + "_case_args")(kind, *shape, **mode)) == want


def test_small_op_selection_table_names_every_launch_the_fp64_test_reaches(lib):
    """One row above per distinct launch -- kernel and bracketed facts -- of tests/test_ops_gpu.py::SMALL_OP_CASES (importable without a GPU)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import test_ops_gpu as G
    finally:
        sys.path.pop(0)
    from multi_task_breast_cancer_amd import ops
    named = {part for *_, want in SMALL_OP_SELECTION for part in want.split(" + ")}
    reached = {part for case in G.SMALL_OP_CASES for op in G._small_case_ops(case) for part in ops.op_kernel_name(op).split(" + ")}
    assert len(reached) >= 30 and not reached - named, sorted(reached - named)
    assert not named - reached, sorted(named - reached)          # ... and the fp64 table reaches every launch that has a name here


def test_small_op_kernel_name_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    buf = C.create_string_buffer(512)
    name = lambda op: lib.mtbc_op_kernel_name(C.byref(op), buf, 512)      # noqa: E731
    P, B = L.OP_POOL_FWD, L.OP_POOL_BWD
    assert name(ops.maxpool_case_args(P, 2, 8, 6, 7)) == -1                                 # odd W
    assert name(ops.maxpool_case_args(P, 0, 8, 6, 8)) == -1
    op = ops.maxpool_case_args(P, 2, 8, 8, 8)
    op.u.pool.y = None
    assert name(op) == -2
    op = ops.maxpool_case_args(P, 2, 8, 8, 8)
    op.u.pool.layout = 2                                                                    # no such layout
    assert name(op) == -2
    assert name(ops.maxpool_case_args(P, 2, 12, 8, 8, compute=1)) == -2                     # channel-blocked: C % 8
    op = ops.maxpool_case_args(P, 2, 8, 8, 8, compute=1)
    op.u.pool.type16 = 3
    assert name(op) == -2
    assert name(ops.maxpool_case_args(P, 2, 8, 8, 8, compute=1, strides=dict(y=8 * 16 + 4))) == -5      # a channel-blocked view starts on 16 bytes
    op = ops.maxpool_case_args(P, 2, 8, 8, 8)
    op.u.pool.x += 4                                                                        # pointer values count: a misaligned x takes the scalar kernel
    assert name(op) == 0 and buf.value == b"maxpool_fwd_scalar_kernel"
    op = ops.maxpool_case_args(B, 2, 8, 8, 8)
    op.u.pool.dx += 4                                                                       # ... the backward has float2 stores only
    assert name(op) == -5
    assert name(ops.maxpool_case_args(B, 2, 8, 8, 8, strides=dict(dx=8 * 64 + 1))) == -5
    op = ops.maxpool_case_args(B, 2, 8, 8, 8)
    op.u.pool.dy = None
    assert name(op) == -2
    F_, D_, W_ = L.OP_CONV1_FWD, L.OP_CONV1_DGRAD, L.OP_CONV1_WGRAD
    assert name(ops.conv1x1_case_args(F_, 2, 16, 3, 5, 6)) == -5                            # H * W % 4
    assert name(ops.conv1x1_case_args(F_, 2, 0, 3, 8, 8)) == -1
    assert name(ops.conv1x1_case_args(F_, 2, 16, 3, 8, 8, strides=dict(x=16 * 64 + 2))) == -5
    assert name(ops.conv1x1_case_args(F_, 2, 16, 9, 8, 8, compute=1)) == -5                 # channel-blocked x: Cout <= 8
    assert name(ops.conv1x1_case_args(F_, 2, 12, 3, 8, 8, compute=1)) == -5                 # ... Cin % 8
    op = ops.conv1x1_case_args(F_, 2, 16, 3, 8, 8)
    op.u.conv1.x_layout = 2
    assert name(op) == -2
    op = ops.conv1x1_case_args(D_, 2, 16, 3, 8, 8)
    op.u.conv1.dx = None
    assert name(op) == -2
    assert name(ops.conv1x1_case_args(D_, 2, 16, 3, 8, 8, strides=dict(dx=16 * 64 + 2))) == -5
    assert name(ops.conv1x1_case_args(W_, 2, 16, 3, 8, 8, workspace=False)) == -3
    for mode in ({}, dict(compute=1)):
        op = ops.conv1x1_case_args(W_, 2, 16, 3, 8, 8, **mode)
        assert name(op) == 0
        op.u.conv1.workspace_bytes -= 4                                                     # one float short
        assert name(op) == -3
    op = ops.conv1x1_case_args(W_, 2, 16, 3, 8, 8)
    op.u.conv1.dw = None
    assert name(op) == -2
    G_, GB = L.OP_GAP_FWD, L.OP_GAP_BWD
    assert name(ops.gap_case_args(G_, 2, 8, 0, 8)) == -1
    op = ops.gap_case_args(GB, 2, 8, 4, 4)
    op.u.gap.dx = None
    assert name(op) == -2
    LF, LB = L.OP_LINEAR_FWD, L.OP_LINEAR_BWD
    assert name(ops.linear_case_args(LF, 2, 0, 3)) == -1
    op = ops.linear_case_args(LF, 2, 8, 3)
    op.u.linear.w = None
    assert name(op) == -2
    assert name(ops.linear_case_args(LB, 4, 8, 3, relu=True, workspace=False)) == -3
    op = ops.linear_case_args(LB, 4, 8, 3, relu=True)
    op.u.linear.workspace_bytes -= 4
    assert name(op) == -3
    op = ops.linear_case_args(LB, 4, 8, 3, relu=True)
    op.u.linear.y = None                                                                    # the mask needs the stored output
    assert name(op) == -2
    assert name(ops.linear_case_args(LB, 4, 8, 3, workspace=False)) == 0                    # no ReLU: no workspace needed
    HC, HE = L.OP_HEAD_COMBINE, L.OP_HEAD_EXPAND
    assert name(ops.head_case_args(HC, 8, 0, 1, 2)) == -1
    op = ops.head_case_args(HC, 8, 4, 1, 2)
    op.u.head.bc = None
    assert name(op) == -2
    op = ops.head_case_args(HE, 8, 4, 1, 2)
    op.u.head.gb = None
    assert name(op) == -2
    assert name(ops.head_case_args(HE, 8, 4, 1, 2, bT=False, b1=False, dbT=False, db1=False)) == 0      # every optional pointer absent
    for kind in range(0, 40):                                                               # every other op kind: not this query's
        if kind not in ops.SMALL_OPS + ops.LOSS_OPS:
            op = ops.gap_case_args(G_, 2, 8, 4, 4)
            op.kind = kind
            assert name(op) == -2, kind
    op = ops.maxpool_case_args(P, 2, 8, 8, 8, compute=2)
    want = b"maxpool_c8_fwd_kernel<true>"
    assert lib.mtbc_op_kernel_name(C.byref(op), buf, len(want)) == -2                       # no room for the NUL
    assert lib.mtbc_op_kernel_name(C.byref(op), buf, len(want) + 1) == 0 and buf.value == want
    assert lib.mtbc_op_kernel_name(C.byref(op), None, 512) == -2
    assert lib.mtbc_op_kernel_name(None, buf, 512) == -2


# (what, arguments, mode) -> what mtbc_op_kernel_name names: one row per dispatch decision of the Dice, Focal, loss-mix and softmax calls
# (head_loss.hip), each boundary from both sides.  Dice: (n_heads, N, C, H, W), mode = keywords of ops.dice_case_args + `poke`: field -> bytes
# added to head 0's dummy address; Focal: (N, C); softmax: (N, C, backward).
_DF, _DB = L.OP_DICE_FWD, L.OP_DICE_BWD
_FIN = " + dice_finalize_kernel"
LOSS_OP_SELECTION = [
    (_DF, (1, 1, 1, 4095, 4), {}, "dice_stats_kernel<0> [threads=256 paths=v rounds>1 rest part]" + _FIN + "<0>"),            # H * W = 16380: the last 256-thread plane
    (_DF, (1, 1, 1, 4096, 4), {}, "dice_stats_kernel<0> [threads=1024 paths=v rounds=1]" + _FIN + "<0>"),                     # 16384; n4 = 4096: one round, nothing else
    (_DF, (1, 1, 1, 4097, 4), {}, "dice_stats_kernel<0> [threads=1024 paths=v rounds=1 rest part]" + _FIN + "<0>"),           # n4 = 4097: thread 0 alone takes a rest trip
    (_DF, (1, 1, 1, 7168, 4), {}, "dice_stats_kernel<0> [threads=1024 paths=v rounds=1 rest]" + _FIN + "<0>"),                # n4 = 7168: three rest trips each
    (_DF, (1, 1, 1, 7169, 4), {}, "dice_stats_kernel<0> [threads=1024 paths=v rounds>1 rest part]" + _FIN + "<0>"),           # n4 = 7169: thread 0 alone takes a second round
    (_DF, (4, 2, 1, 256, 256), {}, "dice_stats_kernel<0> [threads=1024 paths=vvvv rounds>1]" + _FIN + "<0>"),
    (_DF, (2, 1, 1, 2, 4), {}, "dice_stats_kernel<0> [threads=256 paths=vv rounds=0 rest part]" + _FIN + "<0>"),              # fewer float4 than threads
    (_DF, (2, 2, 1, 6, 5), dict(seg_kind=L.SEG_BCE), "dice_stats_kernel<1> [threads=256 paths=ss]" + _FIN + "<1>"),           # H * W % 4 != 0
    (_DF, (3, 2, 1, 16, 16), dict(seg_kind=L.SEG_FOCALDICE, poke=dict(x=4)), "dice_stats_kernel<2> [threads=256 paths=svv rounds=0 rest part]" + _FIN + "<2>"),
    (_DF, (1, 2, 1, 16, 16), dict(seg_kind=L.SEG_JACCARD, poke=dict(target=4)), "dice_stats_kernel<3> [threads=256 paths=s]" + _FIN + "<3>"),
    (_DF, (1, 2, 1, 16, 16), dict(poke=dict(dx=4)), "dice_stats_kernel<0> [threads=256 paths=v rounds=0 rest part]" + _FIN + "<0>"),      # the forward does not read dx
    (_DF, (1, 256, 1, 4, 4), {}, "dice_stats_kernel<0> [threads=256 paths=v rounds=0 rest part]" + _FIN + "<0>"),
    (_DF, (1, 257, 1, 4, 4), {}, "dice_stats_kernel<0> [threads=256 paths=v rounds=0 rest part]" + _FIN + "<0> [planes>256]"),
    (_DF, (1, 129, 2, 4, 4), dict(seg_kind=L.SEG_JACCARD), "dice_stats_kernel<3> [threads=256 paths=v rounds=0 rest part]" + _FIN + "<3> [planes>256]"),
    (_DB, (4, 2, 1, 256, 256), {}, "dice_bwd_kernel<0> [paths=vvvv]"),
    (_DB, (2, 2, 1, 6, 5), dict(seg_kind=L.SEG_BCE), "dice_bwd_kernel<1> [paths=ss]"),
    (_DB, (2, 2, 1, 16, 16), dict(seg_kind=L.SEG_FOCALDICE, poke=dict(dx=4)), "dice_bwd_kernel<2> [paths=sv]"),
    (_DB, (2, 2, 1, 16, 16), dict(seg_kind=L.SEG_JACCARD, poke=dict(x=8)), "dice_bwd_kernel<3> [paths=sv]"),
    (_DB, (1, 16, 1, 512, 512), {}, "dice_bwd_kernel<0> [paths=v]"),                          # 4 194 304 elements: 4096 x 256 threads, one float4 each
    (_DB, (1, 1, 1, 1048577, 4), {}, "dice_bwd_kernel<0> [paths=v loop]"),                    # 4 194 308: one float4 more
    (_DB, (1, 1, 1, 1048575, 1), {}, "dice_bwd_kernel<0> [paths=s]"),                         # the scalar loop: 4096 blocks are not capped
    (_DB, (1, 1, 1, 1048577, 1), {}, "dice_bwd_kernel<0> [paths=s loop]"),
    (_DB, (2, 1, 1, 1048577, 4), dict(poke=dict(dx=4)), "dice_bwd_kernel<0> [paths=sv loop]"),
    (L.OP_FOCAL, (256, 3), {}, "focal_kernel"),
    (L.OP_FOCAL, (257, 3), dict(weight=True, dx=False), "focal_kernel [N>256]"),
    (L.OP_FOCAL, (5, 1), dict(gamma=0.0), "focal_kernel"),
    (L.OP_SOFTMAX, (64, 3, False), {}, "softmax_rows_kernel"),
    (L.OP_SOFTMAX, (65, 3, False), {}, "softmax_rows_kernel [N>64]"),
    (L.OP_SOFTMAX, (64, 2, True), {}, "softmax_rows_kernel"),
    (L.OP_SOFTMAX, (65, 1, True), {}, "softmax_rows_kernel [N>64]"),
    (L.OP_LOSS_MIX, (), {}, "loss_mix_kernel"),
]


def _loss_op(kind, shape, mode):
    """The op of a row of LOSS_OP_SELECTION through its struct's filler (dummy pointers)."""
    from multi_task_breast_cancer_amd import ops
    mode = dict(mode)
    poke = mode.pop("poke", {})
    if kind in (_DF, _DB):
        op = ops.dice_case_args(kind, *shape, **mode)
        for name, nbytes in poke.items():
            if name == "target":
                op.u.dice.target += nbytes
            else:
                getattr(op.u.dice, name)[0] = (getattr(op.u.dice, name)[0] or 0) + nbytes
        return op
    if kind == L.OP_FOCAL:
        return ops.focal_case_args(*shape, **mode)
    op = L.Op()
    op.kind = kind
    if kind == L.OP_SOFTMAX:
        N, Cc, backward = shape
        ops.softmax_args(N, Cc, backward, x=1 << 20, p=2 << 20, dp=3 << 20, dz=4 << 20, into=op.u.softmax)
    else:
        op.u.mix.seg, op.u.mix.cls, op.u.mix.alpha, op.u.mix.out4 = 1 << 20, 2 << 20, 0.5, 3 << 20
    return op


@pytest.mark.parametrize("kind,shape,mode,want", LOSS_OP_SELECTION)
def test_loss_op_kernel_selection(lib, kind, shape, mode, want):
    """mtbc_op_kernel_name (host only: the dummy pointers are never dereferenced) names every launch of a Dice, Focal, loss-mix or softmax
    call and what the arguments -- pointer VALUES included -- select inside it."""
    from multi_task_breast_cancer_amd import ops
    assert ops.op_kernel_name(_loss_op(kind, shape, mode)) == want


def test_loss_op_kernel_name_refuses_what_the_call_refuses(lib):
    from multi_task_breast_cancer_amd import ops
    buf = C.create_string_buffer(512)
    name = lambda op: lib.mtbc_op_kernel_name(C.byref(op), buf, 512)      # noqa: E731
    for kind in (_DF, _DB):
        assert name(ops.dice_case_args(kind, 0, 2, 1, 8, 8)) == -1                          # no head
        op = ops.dice_case_args(kind, 4, 2, 1, 8, 8)
        op.u.dice.n_heads = 5                                                               # more heads than the struct holds
        assert name(op) == -1
        assert name(ops.dice_case_args(kind, 2, 2, 1, 0, 8)) == -1
        op = ops.dice_case_args(kind, 3, 2, 1, 8, 8)
        op.u.dice.x[1] = None                                                               # a NULL head
        assert name(op) == -2
        op = ops.dice_case_args(kind, 3, 2, 1, 8, 8)
        op.u.dice.x[3] = None                                                               # ... behind the last one: not read
        assert name(op) == 0
        op = ops.dice_case_args(kind, 2, 2, 1, 8, 8)
        op.u.dice.kind = 4                                                                  # no such criterion
        assert name(op) == -5
        op = ops.dice_case_args(kind, 2, 2, 1, 8, 8)
        op.u.dice.stats = None
        assert name(op) == -2
    op = ops.dice_case_args(_DF, 2, 2, 1, 8, 8)
    op.u.dice.loss = None
    assert name(op) == -2
    op = ops.dice_case_args(_DB, 2, 2, 1, 8, 8)
    op.u.dice.loss = None                                                                   # the backward writes no loss
    assert name(op) == 0
    op = ops.dice_case_args(_DB, 2, 2, 1, 8, 8)
    op.u.dice.dx[1] = None
    assert name(op) == -2
    op = ops.dice_case_args(_DF, 2, 2, 1, 8, 8)
    assert not op.u.dice.dx[0] and name(op) == 0                                            # the forward needs no dx
    assert name(ops.focal_case_args(0, 3)) == -1 and name(ops.focal_case_args(4, 0)) == -1
    for field in ("x", "target", "loss"):
        op = ops.focal_case_args(4, 3)
        setattr(op.u.focal, field, None)
        assert name(op) == -2, field
    assert name(ops.focal_case_args(4, 3, dx=False)) == 0                                   # weight, dx and gscale_dev are optional
    assert name(_loss_op(L.OP_SOFTMAX, (4, 4, False), {})) == -1                            # C outside 1 .. 3
    assert name(_loss_op(L.OP_SOFTMAX, (0, 3, False), {})) == -1
    op = _loss_op(L.OP_SOFTMAX, (4, 3, True), {})
    op.u.softmax.dp = None
    assert name(op) == -2
    op = _loss_op(L.OP_SOFTMAX, (4, 3, False), {})
    op.u.softmax.dp = op.u.softmax.dz = None                                                # the forward reads neither
    assert name(op) == 0
    op.u.softmax.x = None
    assert name(op) == -2
    for field in ("seg", "cls", "out4"):
        op = _loss_op(L.OP_LOSS_MIX, (), {})
        setattr(op.u.mix, field, None)
        assert name(op) == -2, field


# ---------------------------------------------------------------- one filler, two callers: dummy pointers (the guards) against ptrs= (the launches)
# rows beside the selection tables: the keywords only the eager wrappers of ops.py use
_CASE_EXTRA = [
    ("conv3x3", L.OP_CONV3_FWD, (2, [16, 8], 16, 16, 16), dict(_BF16, out_c8=True, stats=True)),                 # epilogue statistics
    ("conv3x3", L.OP_CONV3_FWD, (2, [16], 16, 16, 16), dict(_F16_O1, bias=False, stats=True, norm=0.1, out_partial=True)),   # the gathered dgrad's norm epilogue
    ("conv3x3", L.OP_CONV3_FWD, (2, [3], 24, 16, 16), dict(_BF16_O3, stats=True)),                               # the stem with statistics
    ("conv3x3", L.OP_CONV3_FWD, (2, [16, 16], 16, 16, 16), dict(_BF16, bias=False, out_accumulate=True)),        # a gathered dgrad added to fp32 planes
    ("conv3x3", L.OP_CONV3_WGRAD, (1, [64], 48, 16, 16), dict(_BF16, bias=False)),                               # one image range: the direct store
    ("conv3x3", L.OP_CONV3_DGRAD, (2, [8, 16], 16, 16, 16), dict(_BF16, accumulate=[0, 0])),
    ("conv3x3", L.OP_CONV3_FWD, (2, [8, 8], 16, 16, 16), dict(packed=False, force_direct=True, bias=False)),
    ("conv3x3", L.OP_CONV3_DGRAD, (2, [8, 16], 16, 16, 16), dict(_BF16, accumulate=[1, 2])),                     # 16-bit planar second segment
    ("conv3x3", L.OP_CONV3_DGRAD, (2, [8, 16], 16, 16, 16), dict(_F16, dx_c8=True)),
    ("conv3x3", L.OP_CONV3_DGRAD, (2, [8, 16], 16, 16, 16), dict(packed=False, force_direct=True, accumulate=())),
    ("conv3x3", L.OP_CONV3_WGRAD, (2, [8, 16], 16, 16, 16), dict(accumulate_dw=True, force_direct=True, bias=False)),
    ("instnorm", True, (2, 16, 16, 16), dict(compute=1, out="c8", z="c8f16", dy="c8", pool=True, rank1=True, rank1_grads=True, rank1_acc=True, acc=True)),
    ("instnorm", False, (2, 16, 16, 16), dict(compute=1, out="c8", planar=True, affine=False, pool=True, pool_arg=False)),
    ("convT", L.OP_CONVT_WGRAD, (2, 16, 8, 8, 8, 4), dict(workspace=False, acc_dw=True)),
    ("convT", L.OP_CONVT_DGRAD, (2, 16, 8, 8, 8, 2), dict(acc_dx=True, strides=dict(dx=2 * 16 * 64, dy=3 * 8 * 256))),
    ("gap", L.OP_GAP_BWD, (2, 8, 4, 4), {}),
    ("linear", L.OP_LINEAR_FWD, (4, 8, 3), dict(bias=False)),
    ("linear", L.OP_LINEAR_BWD, (4, 8, 3), dict(relu=True, acc_dw=True)),
    ("conv1x1", L.OP_CONV1_WGRAD, (2, 16, 3, 8, 8), dict(workspace=False, acc_dw=True)),
    ("head", L.OP_HEAD_EXPAND, (8, 4, 1, 2), dict(acc=(1, 0, 1, 1))),
]


def _case_rows():
    """(family, op, shape, mode, pair) of every row of the four selection tables -- InstanceNorm up to 64 x 64 planes only: larger ones with a
    channel-blocked output ask the device for the team plan --, of tests/test_ops_gpu.py CONV3_STEP_CASES and of _CASE_EXTRA."""
    kinds = {"fwd": L.OP_CONV3_FWD, "dgrad": L.OP_CONV3_DGRAD, "wgrad": L.OP_CONV3_WGRAD}
    rows = [("conv3x3", kinds[op], (N, segs, Cout, H, W), mode, False) for op, N, segs, Cout, H, W, mode, _ in SELECTION]
    rows += [("instnorm", bwd, (N, Cc, H, W), mode, False) for bwd, N, Cc, H, W, mode, _ in NORM_SELECTION if H * W <= 64 * 64]
    rows += [("convT", _CT_OPS[op], shape, mode, pair) for op, shape, mode, pair, _ in CONVT_SELECTION]
    rows += [(helper, kind, shape, mode, False) for helper, kind, shape, mode, _ in SMALL_OP_SELECTION]
    import test_ops_gpu          # (imports without a device) every row of the conv3x3 step-instance table: its modes are the engine's
    rows += [("conv3x3", op, (N, segs, Cout, H, W), mode, False) for op, N, segs, Cout, H, W, mode in test_ops_gpu.CONV3_STEP_CASES]
    return rows + [r + (False,) for r in _CASE_EXTRA]


class _Tensors(dict):
    """ptrs= of a *_case_args builder: a small CPU tensor per field, made when first asked for (only data_ptr() and numel() are read)."""

    def __missing__(self, name):
        import torch
        self[name] = torch.empty(16, dtype=torch.float32)
        return self[name]


def _case_fields(a, prefix=""):
    """{path: value} of a struct; pointers as NULL or not, the active union member of an op."""
    if isinstance(a, L.Op):
        return dict(_case_fields(getattr(a.u, L.OP_UNION_FIELD[a.kind])), kind=a.kind)
    out = {}
    for name, typ in a._fields_:
        v = getattr(a, name)
        if isinstance(v, C.Array):
            for i, e in enumerate(v):
                out.update(_case_fields(e, f"{prefix}{name}[{i}].") if isinstance(e, C.Structure) else {f"{prefix}{name}[{i}]": bool(e)})
        else:
            out[prefix + name] = bool(v) if typ is C.c_void_p else v
    return out


@pytest.mark.parametrize("family", ["conv3x3", "instnorm", "convT", "maxpool", "conv1x1", "gap", "linear", "head"])
def test_case_args_with_tensors_equal_case_args_with_dummies(lib, family):
    """Each *_case_args builder serves the launch-coverage guards (ptrs=None: dummy addresses) and every launch of ops.py (ptrs= tensors).  Both
    must give one struct: every non-pointer field equal -- workspace_bytes follows the tensor handed in and may be larger --, the same pointer
    fields NULL, the same launches named by the family's *_kernel_name (or the same refusal: a weight gradient without its workspace).  Nothing
    is launched."""
    import torch
    from multi_task_breast_cancer_amd import ops
    rows = [r for r in _case_rows() if r[0] == family]
    assert len(rows) >= 3

    def named(f, *args):
        try:
            return f(*args)
        except L.MtbcError as e:
            return str(e)
    for _, op, shape, mode, pair in rows:
        build = getattr(ops, family + "_case_args")
        if family == "conv3x3":
            name = lambda a: ops.conv3x3_kernel_name(a, op)                                             # noqa: E731
        elif family == "instnorm":
            name = lambda a: ops.instnorm_kernel_name(a, op)                                            # noqa: E731
        elif family == "convT":
            name = lambda a, nxt=None: ops.convT_kernel_name(a, op, nxt)                                # noqa: E731
        else:
            name = ops.op_kernel_name
        dummy = build(op, *shape, **mode)
        d = _case_fields(dummy)
        T = _Tensors()
        if family == "conv3x3":
            T["in"] = [torch.empty(16) for _ in shape[1]]
            T["wgrad_sync"] = torch.empty(max(1, d["wgrad_sync_bytes"] // 4), dtype=torch.int32)
        T["workspace"] = torch.empty(d.get("workspace_bytes", 0) // 4 + 8, dtype=torch.float32)      # as the wrappers: at least what is asked for
        real = build(op, *shape, ptrs=T, **mode)
        r = _case_fields(real)
        assert r.pop("workspace_bytes", 0) >= d.pop("workspace_bytes", 0), (family, op, shape, mode)
        assert r == d, (family, op, shape, mode, {k: (d[k], r[k]) for k in d if d[k] != r[k]})
        if pair:
            dg = L.OP_CONVT_DGRAD
            assert named(name, real, ops.convT_case_args(dg, *shape, ptrs=T, **mode)) == named(name, dummy, ops.convT_case_args(dg, *shape, **mode))
        else:
            assert named(name, real) == named(name, dummy), (family, op, shape, mode)
