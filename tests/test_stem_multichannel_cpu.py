"""The stem with intensity channels (data.augmentation: Cin = 2 .. MTBC_STEM_MAX_CIN, one fp32 planar segment), host only: which
kernel instances mtbc_conv3x3_kernel_name names for it, the plan arithmetic behind them (statistics slots, split-K workspace) and what
the library refuses.  The dummy tensor pointers of ops.conv3x3_case_args are never dereferenced."""
import ctypes as C
import os
import re

import pytest

from multi_task_breast_cancer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, WGRAD = L.OP_CONV3_FWD, L.OP_CONV3_WGRAD


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_constant_is_mirrored():
    src = open(os.path.join(ROOT, "include", "mtbc.h")).read()
    assert int(re.search(r"#define\s+MTBC_STEM_MAX_CIN\s+(\d+)", src).group(1)) == L.STEM_MAX_CIN == 5


_BF16_O3 = dict(compute=1, c8=True, out_c8=True, out_fp16=True)
_F16_O1 = dict(compute=2, out_c8=True)
_WG = dict(compute=1, c8=True, bias=False)
SELECTION = [
    # 16-bit forward: <CIN, OF16> -- bf16 mode storing fp16 (configs[1]'s plan) and fp16 mode
    (FWD, 32, [3], 24, 256, 256, _BF16_O3, "conv3x3_stem_mc_fwd_c8_kernel<3, true>"),
    (FWD, 32, [5], 24, 256, 256, _BF16_O3, "conv3x3_stem_mc_fwd_c8_kernel<5, true>"),
    (FWD, 32, [3], 24, 256, 256, _F16_O1, "conv3x3_stem_mc_fwd_c8_kernel<3, true>"),
    (FWD, 32, [5], 24, 256, 256, _F16_O1, "conv3x3_stem_mc_fwd_c8_kernel<5, true>"),
    (FWD, 32, [2], 24, 256, 256, dict(compute=1, out_c8=True), "conv3x3_stem_mc_fwd_c8_kernel<2, false>"),      # MTBC_Z_BF16: stored as bf16
    # fp32 parity mode: <CIN>
    (FWD, 32, [3], 24, 256, 256, {}, "conv3x3_stem_mc_fwd_kernel<3>"),
    (FWD, 32, [5], 24, 256, 256, {}, "conv3x3_stem_mc_fwd_kernel<5>"),
    # weight gradient from the channel-blocked dz: <CIN, F16>
    (WGRAD, 32, [3], 24, 256, 256, _WG, "conv3x3_wgrad_stem_mc_c8_kernel<3, false> + splitk_reduce"),
    (WGRAD, 32, [5], 24, 256, 256, _WG, "conv3x3_wgrad_stem_mc_c8_kernel<5, false> + splitk_reduce"),
    (WGRAD, 16, [4], 24, 512, 512, dict(_WG, compute=2), "conv3x3_wgrad_stem_mc_c8_kernel<4, true> + splitk_reduce"),
    # fp32 weight gradient: the small-Cin kernel up to MTBC_STEM_MAX_CIN (it stopped at 4)
    (WGRAD, 32, [5], 24, 256, 256, {}, "conv3x3_wgrad_smallcin_kernel + splitk_reduce + channel_sums"),
    # the 1-channel stem keeps its four instances
    (FWD, 32, [1], 24, 256, 256, _BF16_O3, "conv3x3_stem_fwd_c8_kernel<true>"),
    (FWD, 32, [1], 24, 256, 256, {}, "conv3x3_stem_fwd_kernel"),
    (WGRAD, 32, [1], 24, 256, 256, _WG, "conv3x3_wgrad_stem_c8_kernel<false> + splitk_reduce"),
    (WGRAD, 32, [1], 24, 256, 256, {}, "conv3x3_wgrad_smallcin_kernel + splitk_reduce + channel_sums"),
]


@pytest.mark.parametrize("op,N,segs,Cout,H,W,mode,want", SELECTION)
def test_kernel_selection(lib, op, N, segs, Cout, H, W, mode, want):
    from multi_task_breast_cancer_amd import ops
    assert ops.conv3x3_case_kernel(op, N, segs, Cout, H, W, **mode) == want


def test_plan_arithmetic(lib):
    from multi_task_breast_cancer_amd import ops
    cdiv = lambda a, b: (a + b - 1) // b      # noqa: E731
    for H, W in ((40, 24), (256, 256)):
        a = ops.conv3x3_case_args(FWD, 2, [3], 24, H, W, **_BF16_O3)
        assert a.operand_layout == L.LAYOUT_PLANAR and a.out_layout == L.LAYOUT_C8
        assert lib.mtbc_conv3x3_stats_slots(C.byref(a)) == cdiv(H * W // 4, 128), (H, W)
    for size, bands in ((64, 1), (128, 4), (256, 16)):
        for N, cin, cout in ((2, 3, 24), (3, 5, 8), (1, 2, 32)):
            a = ops.conv3x3_case_args(WGRAD, N, [cin], cout, size, size, **_WG)
            assert a.operand_layout == L.LAYOUT_C8
            assert lib.mtbc_conv3x3_wgrad_workspace(C.byref(a)) == N * bands * cout * cin * 9 * 4, (size, N, cin, cout)
            assert lib.mtbc_conv3x3_wgrad_sync_bytes(C.byref(a)) == 0


def test_refusals(lib):
    from multi_task_breast_cancer_amd import ops
    buf = C.create_string_buffer(256)
    name = lambda a: lib.mtbc_conv3x3_kernel_name(C.byref(a), FWD, buf, 256)      # noqa: E731
    UNSUPPORTED = -5
    a = ops.conv3x3_case_args(FWD, 2, [5], 24, 64, 64, **_BF16_O3)
    assert name(a) == 0
    # planar fp32 operands into a channel-blocked output: one segment of at most MTBC_STEM_MAX_CIN channels, nothing else
    a = ops.conv3x3_case_args(FWD, 2, [5], 24, 64, 64, **_BF16_O3)
    a.Cin, a.in_[0].channels, a.in_[0].batch_stride = 6, 6, 6 * 64 * 64
    assert name(a) == UNSUPPORTED
    a = ops.conv3x3_case_args(FWD, 2, [3], 24, 64, 64, **_BF16_O3)
    a.n_in, a.in_[0].channels, a.in_[0].batch_stride = 2, 1, 64 * 64
    a.in_[1].ptr, a.in_[1].channels, a.in_[1].batch_stride = 1 << 30, 2, 2 * 64 * 64
    assert name(a) == UNSUPPORTED
    assert name(ops.conv3x3_case_args(FWD, 2, [3], 12, 64, 64, **_BF16_O3)) == UNSUPPORTED      # 16-bit output: Cout % 8 == 0
    assert name(ops.conv3x3_case_args(FWD, 2, [3], 24, 64, 10, **_BF16_O3)) == UNSUPPORTED      # W % 4 == 0
    # the weight gradient from a channel-blocked dz refuses the same shapes
    wname = lambda a: lib.mtbc_conv3x3_kernel_name(C.byref(a), WGRAD, buf, 256)      # noqa: E731
    assert wname(ops.conv3x3_case_args(WGRAD, 2, [3], 24, 64, 64, **_WG)) == 0
    assert wname(ops.conv3x3_case_args(WGRAD, 2, [3], 12, 64, 64, **_WG)) == UNSUPPORTED
    assert wname(ops.conv3x3_case_args(WGRAD, 2, [3], 24, 64, 10, **_WG)) == UNSUPPORTED


def test_plan_switch_is_declared():
    from multi_task_breast_cancer_amd import switches
    assert switches.PLAN_SWITCHES["MTBC_NO_STEM_MC"][0] == "0"
