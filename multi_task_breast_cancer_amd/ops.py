"""Tensor-level wrappers over the per-op C-ABI (one call = one mtbc_* entry point).

Used by the parity tests and as the reference-side binding example of INTEGRATION.md; the training path itself
goes through step programs (engine.py).  Device fp32 tensors only; every wrapper raises on CPU input.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L


def _s() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if t.device.type != "cuda":
            L.require_gpu()
            raise L.MtbcError("device tensors required")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("fp32 contiguous tensors required")


def _p(t):
    return None if t is None else t.data_ptr()


def _fill_segs(arr, tensors: Sequence[torch.Tensor], accumulate: Sequence[int] = ()):
    for i, t in enumerate(tensors):
        arr[i].ptr = t.data_ptr()
        arr[i].batch_stride = t.shape[1] * t.shape[2] * t.shape[3]
        arr[i].channels = t.shape[1]
        arr[i].accumulate = accumulate[i] if i < len(accumulate) else 0


def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(4, (nbytes + 3) // 4), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------ conv3x3
def conv3x3_kernel_name(a: "L.Conv3x3Args", op: int) -> str:
    """The kernel instance (+ weight-gradient reduction) that mtbc_conv3x3_fwd / _dgrad / _wgrad -- op = L.OP_CONV3_FWD / _DGRAD /
    _WGRAD -- would launch for `a`: mtbc_conv3x3_kernel_name, host-only (no launch, no device access); raises what the call would."""
    buf = C.create_string_buffer(256)
    L.check(L.load().mtbc_conv3x3_kernel_name(C.byref(a), op, buf, len(buf)), "conv3x3_kernel_name")
    return buf.value.decode()


def conv3x3_case_args(op: int, N: int, segs: Sequence[int], Cout: int, H: int, W: int, compute: int = 0, c8: bool = False,
                      out_c8: bool = False, out_fp16: bool = False, dx_c8: bool = False, bias: bool = True,
                      in_kernel_reduce: bool = False) -> "L.Conv3x3Args":
    """The argument struct the wrappers below fill for one call (fwd: conv3x3_fwd / conv3x3_fwd_c8 / conv3x3_stem_fwd_c8, dgrad:
    conv3x3_dgrad / conv3x3_dgrad_c8 with the first segment overwritten and the others accumulated, wgrad: conv3x3_wgrad /
    conv3x3_wgrad_c8), its tensor pointers distinct 16-byte aligned dummies that nothing may dereference: for conv3x3_kernel_name.
    c8: operands in MTBC_LAYOUT_C8 (one segment of at most L.STEM_MAX_CIN channels stays fp32 planar: the stem); bias: fwd bias / wgrad dbias."""
    lib = L.load()
    ptr = iter(range(1 << 20, 1 << 30, 1 << 20))
    a = L.Conv3x3Args()
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, sum(segs), Cout, len(segs)
    for i, c in enumerate(segs):
        a.in_[i].ptr, a.in_[i].batch_stride, a.in_[i].channels = next(ptr), c * H * W, c
        if op == L.OP_CONV3_DGRAD:
            a.in_[i].accumulate = 3 if dx_c8 else (1 if i else 0)
    a.w, a.compute = next(ptr), compute
    stem = len(segs) == 1 and segs[0] <= L.STEM_MAX_CIN
    if c8 and not (stem and op == L.OP_CONV3_FWD):
        a.operand_layout = L.LAYOUT_C8
    if op == L.OP_CONV3_FWD:
        a.out, a.bias = next(ptr), (next(ptr) if bias else None)
        if not stem:
            a.w_packed = next(ptr)
        if out_c8:
            a.out_layout = L.LAYOUT_C8
            a.out_type = 2 if out_fp16 else 0
    elif op == L.OP_CONV3_DGRAD:
        a.w_packed, a.dout = next(ptr), next(ptr)
    else:
        a.dout, a.dw, a.dbias = next(ptr), next(ptr), (next(ptr) if bias else None)
        a.workspace, a.workspace_bytes = next(ptr), int(lib.mtbc_conv3x3_wgrad_workspace(C.byref(a)))
        nsync = int(lib.mtbc_conv3x3_wgrad_sync_bytes(C.byref(a))) if in_kernel_reduce else 0
        if nsync:
            a.wgrad_sync, a.wgrad_sync_bytes = next(ptr), nsync
    return a


def conv3x3_case_kernel(op: int, *shape, **mode) -> str:
    """conv3x3_kernel_name of conv3x3_case_args(op, *shape, **mode)."""
    return conv3x3_kernel_name(conv3x3_case_args(op, *shape, **mode), op)


# (op, instance) of every conv3x3 launch -- and (op, launches) of every InstanceNorm call -- made through the wrappers below while this is
# a list (the reference tests record what they ran)
launched: Optional[list] = None


def _note(a, op: int) -> None:
    if launched is not None:
        launched.append((op, conv3x3_kernel_name(a, op)))


def conv3x3_pack(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _chk(w)
    lib = L.load()
    cout, cin = w.shape[0], w.shape[1]
    pf = torch.empty(lib.mtbc_conv3x3_packed_elems(cin, cout), dtype=torch.float32, device=w.device)
    pd = torch.empty(lib.mtbc_conv3x3_packed_dgrad_elems(cin, cout), dtype=torch.float32, device=w.device)
    L.check(lib.mtbc_conv3x3_pack_fwd(w.data_ptr(), pf.data_ptr(), cin, cout, _s()), "pack_fwd")
    L.check(lib.mtbc_conv3x3_pack_dgrad(w.data_ptr(), pd.data_ptr(), cin, cout, _s()), "pack_dgrad")
    return pf, pd


def conv3x3_pack_lp(w: torch.Tensor, compute: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """16-bit operand images (compute 1 = bf16, 2 = fp16) for fwd and dgrad, as int16 tensors."""
    _chk(w)
    lib = L.load()
    cout, cin = w.shape[0], w.shape[1]
    outs = []
    for dgrad in (0, 1):
        t = torch.empty(lib.mtbc_conv3x3_packed_lp_elems(cin, cout, dgrad), dtype=torch.int16, device=w.device)
        L.check(lib.mtbc_conv3x3_pack_lp(w.data_ptr(), t.data_ptr(), cin, cout, dgrad, compute, _s()), "pack_lp")
        outs.append(t)
    return outs[0], outs[1]


def conv3x3_image_elems(cout: int, cin: int, kind: int) -> int:
    """Elements of one weight image of a (cout, cin, 3, 3) weight; kind as in mtbc_pack_desc: 0 fp32 forward, 1 fp32 dgrad (floats),
    2 16-bit forward, 3 16-bit dgrad (16-bit words)."""
    lib = L.load()
    if kind >= 2:
        return lib.mtbc_conv3x3_packed_lp_elems(cin, cout, kind - 2)
    return lib.mtbc_conv3x3_packed_dgrad_elems(cin, cout) if kind else lib.mtbc_conv3x3_packed_elems(cin, cout)


def conv3x3_pack_list(items, out=None):
    """One mtbc_conv3x3_pack_many call over a free list of (w, kind, compute) -- kind as in mtbc_pack_desc, compute read for the 16-bit kinds
    2, 3 -- in list order.  out: the destination tensor of each item (fp32 for kinds 0, 1, int16 for 2, 3), allocated here when None.
    Returns the destinations."""
    lib = L.load()
    descs = (L.PackDesc * len(items))()
    outs = []
    for i, (w, kind, compute) in enumerate(items):
        _chk(w)
        cout, cin = w.shape[0], w.shape[1]
        if out is None:
            t = torch.empty(conv3x3_image_elems(cout, cin, kind), dtype=torch.int16 if kind >= 2 else torch.float32, device=w.device)
        else:
            t = out[i]
            if t.numel() != conv3x3_image_elems(cout, cin, kind) or t.dtype != (torch.int16 if kind >= 2 else torch.float32):
                raise ValueError(f"destination {i}: {t.numel()} x {t.dtype} for a kind {kind} image of {cout} x {cin}")
        d = descs[i]
        d.w, d.packed, d.Cin, d.Cout, d.kind, d.compute = w.data_ptr(), t.data_ptr(), cin, cout, kind, compute
        outs.append(t)
    L.check(lib.mtbc_conv3x3_pack_many(descs, len(descs), _s()), "pack_many")
    return outs


def conv3x3_pack_many(weights, compute: int = 0):
    """All weight images of a list of conv weights in one launch (mtbc_conv3x3_pack_many).  Returns, per weight, the
    (fwd, dgrad) images: fp32 tensors for compute 0, int16 tensors for compute 1 (bf16) / 2 (fp16)."""
    outs = conv3x3_pack_list([(w, (2 + dg if compute else dg), compute) for w in weights for dg in (0, 1)])
    return [(outs[2 * i], outs[2 * i + 1]) for i in range(len(weights))]


def _conv_args(xs, w, N, H, W):
    a = L.Conv3x3Args()
    cin = sum(x.shape[1] for x in xs)
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, cin, w.shape[0], len(xs)
    a.w = w.data_ptr()
    return a


def conv3x3_fwd(xs: Sequence[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                packed: Optional[torch.Tensor] = None, force_direct: bool = False, compute: int = 0) -> torch.Tensor:
    _chk(*xs, w, bias)
    N, _, H, W = xs[0].shape
    a = _conv_args(xs, w, N, H, W)
    _fill_segs(a.in_, xs)
    out = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=w.device)
    a.w_packed, a.bias, a.out, a.force_direct = _p(packed), _p(bias), out.data_ptr(), int(force_direct)
    a.compute = compute
    _note(a, L.OP_CONV3_FWD)
    L.check(L.load().mtbc_conv3x3_fwd(C.byref(a), _s()), "conv3x3_fwd")
    return out


def conv3x3_stem_fwd_c8(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], compute: int, out_fp16: bool = False, stats: bool = False):
    """The stem conv of the 16-bit modes (1 .. L.STEM_MAX_CIN input channels: the image + intensity channels): fp32 operands, the output
    channel-blocked 16-bit (out_layout = C8 with operand_layout = planar) + optional InstanceNorm statistics partials."""
    _chk(x, w, bias)
    if not 1 <= w.shape[1] <= L.STEM_MAX_CIN or x.shape[1] != w.shape[1]:
        raise ValueError(f"the stem takes 1 .. {L.STEM_MAX_CIN} input channels")
    N, _, H, W = x.shape
    a = _conv_args([x], w, N, H, W)
    _fill_segs(a.in_, [x])
    out = torch.empty(N, w.shape[0] // 8, H * W, 8, dtype=torch.int16, device=w.device)
    a.bias, a.out, a.compute, a.out_layout = _p(bias), out.data_ptr(), compute, L.LAYOUT_C8
    if out_fp16:
        a.out_type = 2
    part = None
    if stats:
        slots = L.load().mtbc_conv3x3_stats_slots(C.byref(a))
        if slots <= 0:
            raise L.MtbcError("conv3x3_fwd: no epilogue statistics for this launch")
        part = torch.full((N, slots, w.shape[0], 2), float("nan"), dtype=torch.float32, device=w.device)
        a.stats_partial = part.data_ptr()
    _note(a, L.OP_CONV3_FWD)
    L.check(L.load().mtbc_conv3x3_fwd(C.byref(a), _s()), "conv3x3_fwd(stem c8)")
    z = C8(out, (N, w.shape[0], H, W), 2 if out_fp16 else compute)
    return (z, part) if stats else z


def conv3x3_dgrad(dz: torch.Tensor, w: torch.Tensor, dxs: Sequence[torch.Tensor], accumulate: Sequence[int] = (),
                  packed: Optional[torch.Tensor] = None, force_direct: bool = False, compute: int = 0) -> None:
    _chk(dz, w, *dxs)
    N, _, H, W = dz.shape
    a = _conv_args(dxs, w, N, H, W)
    _fill_segs(a.in_, dxs, accumulate)
    a.w_packed, a.dout, a.force_direct = _p(packed), dz.data_ptr(), int(force_direct)
    a.compute = compute
    _note(a, L.OP_CONV3_DGRAD)
    L.check(L.load().mtbc_conv3x3_dgrad(C.byref(a), _s()), "conv3x3_dgrad")


def conv3x3_wgrad(xs: Sequence[torch.Tensor], dz: torch.Tensor, w_shape, want_bias: bool = False,
                  force_direct: bool = False, dw: Optional[torch.Tensor] = None, accumulate: bool = False,
                  compute: int = 0):
    _chk(*xs, dz)
    N, _, H, W = dz.shape
    dev = dz.device
    if dw is None:
        dw = torch.empty(*w_shape, dtype=torch.float32, device=dev)
    db = torch.empty(w_shape[0], dtype=torch.float32, device=dev) if want_bias else None
    a = L.Conv3x3Args()
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, w_shape[1], w_shape[0], len(xs)
    _fill_segs(a.in_, xs)
    a.dout, a.dw, a.dbias, a.force_direct, a.accumulate_dw = dz.data_ptr(), dw.data_ptr(), _p(db), int(force_direct), int(accumulate)
    a.compute = compute
    nb = L.load().mtbc_conv3x3_wgrad_workspace(C.byref(a))
    ws = _ws(nb, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _note(a, L.OP_CONV3_WGRAD)
    L.check(L.load().mtbc_conv3x3_wgrad(C.byref(a), _s()), "conv3x3_wgrad")
    return dw, db


# ------------------------------------------------------------------ conv3x3 on 16-bit channel-blocked operands
class C8:
    """A tensor in MTBC_LAYOUT_C8: [N][C/8][H*W][8] in bf16 (compute 1) or fp16 (compute 2), held as int16 storage.
    What the 3x3 convolutions' MFMAs read when `operand_layout = 1` (include/mtbc.h)."""

    def __init__(self, data: torch.Tensor, shape, compute: int):
        self.data, self.shape, self.compute = data, tuple(shape), compute

    @staticmethod
    def pack(x: torch.Tensor, compute: int) -> "C8":
        _chk(x)
        N, Cc, H, W = x.shape
        d = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=x.device)
        L.check(L.load().mtbc_c8_pack(x.data_ptr(), Cc * H * W, d.data_ptr(), N, Cc, H * W, compute, _s()), "c8_pack")
        return C8(d, x.shape, compute)

    @staticmethod
    def pack16(x16: torch.Tensor, compute: int) -> "C8":
        """From 16-bit planes (N,C,H,W as int16 storage), mtbc_c8_pack16."""
        N, Cc, H, W = x16.shape
        d = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=x16.device)
        L.check(L.load().mtbc_c8_pack16(x16.data_ptr(), Cc * H * W, d.data_ptr(), N, Cc, H * W, _s()), "c8_pack16")
        return C8(d, x16.shape, compute)

    def unpack(self) -> torch.Tensor:
        N, Cc, H, W = self.shape
        y = torch.empty(N, Cc, H, W, dtype=torch.float32, device=self.data.device)
        L.check(L.load().mtbc_c8_unpack(self.data.data_ptr(), y.data_ptr(), N, Cc, H * W, self.compute, _s()), "c8_unpack")
        return y


def _fill_segs_c8(arr, tensors: Sequence["C8"]):
    for i, t in enumerate(tensors):
        arr[i].ptr = t.data.data_ptr()
        arr[i].batch_stride = t.shape[1] * t.shape[2] * t.shape[3]      # 16-bit elements
        arr[i].channels = t.shape[1]
        arr[i].accumulate = 0


def conv3x3_fwd_c8(xs: Sequence["C8"], w: torch.Tensor, bias: Optional[torch.Tensor], packed: torch.Tensor, out_c8: bool = False,
                   stats: bool = False, norm=None, out_partial: Optional[torch.Tensor] = None, out_fp16: bool = False):
    """z = conv3x3(concat(xs)) with the inputs already in the MFMA's 16-bit channel-blocked layout; z comes back as fp32
    planes, or (out_c8, `out_layout = C8` of the C-ABI) as a channel-blocked 16-bit tensor of the inputs' type."""
    _chk(w, bias)
    N, _, H, W = xs[0].shape
    a = L.Conv3x3Args()
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, sum(x.shape[1] for x in xs), w.shape[0], len(xs)
    _fill_segs_c8(a.in_, xs)
    if out_c8:
        out = torch.empty(N, w.shape[0] // 8, H * W, 8, dtype=torch.int16, device=w.device)
        a.out_layout = L.LAYOUT_C8
        if out_fp16:            # bf16 operands, the output stored as fp16 (out_type of the C-ABI)
            a.out_type = 2
    else:
        out = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=w.device)
    a.w, a.w_packed, a.bias, a.out = w.data_ptr(), packed.data_ptr(), _p(bias), out.data_ptr()
    a.compute, a.operand_layout = xs[0].compute, L.LAYOUT_C8
    part = None
    if norm is not None:    # gathered dgrad + norm-backward reductions: norm = (z8, mean, rstd, gamma, beta, slope) of the output tensor
        z8n, mean, rstd, gamma, beta, slope = norm
        _chk(mean, rstd, gamma, beta, out_partial)
        a.norm_z, a.norm_mean, a.norm_rstd, a.norm_gamma, a.norm_beta, a.norm_slope = z8n.data.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(gamma), _p(beta), slope
        a.out_partial = _p(out_partial)
        stats = True
    if stats:       # InstanceNorm statistics from the epilogue: (partials [N][slots][Cout][2], slots)
        slots = L.load().mtbc_conv3x3_stats_slots(C.byref(a))
        if slots <= 0:
            raise L.MtbcError("conv3x3_fwd: no epilogue statistics for this launch")
        part = torch.full((N, slots, w.shape[0], 2), float("nan"), dtype=torch.float32, device=w.device)
        a.stats_partial = part.data_ptr()
    _note(a, L.OP_CONV3_FWD)
    L.check(L.load().mtbc_conv3x3_fwd(C.byref(a), _s()), "conv3x3_fwd(c8)")
    z = C8(out, (N, w.shape[0], H, W), 2 if out_fp16 else xs[0].compute) if out_c8 else out
    return (z, part) if stats else z


def conv3x3_dgrad_c8(dz: "C8", w: torch.Tensor, dxs: Sequence[torch.Tensor], accumulate: Sequence[int], packed: torch.Tensor) -> None:
    """dx segments (fp32 planar, accumulate honoured; accumulate 2 = the segment is an int16 (N,C,H,W) tensor written as
    16-bit planar values of dz's type) from dz in the 16-bit channel-blocked layout."""
    if any(isinstance(d, C8) for d in dxs):       # accumulate = 3: channel-blocked 16-bit segments (all of them)
        N, _, H, W = dz.shape
        a = L.Conv3x3Args()
        a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, sum(d.shape[1] for d in dxs), w.shape[0], len(dxs)
        a.w = w.data_ptr()
        _fill_segs_c8(a.in_, dxs)
        for i in range(len(dxs)):
            a.in_[i].accumulate = 3
        a.w_packed, a.dout = packed.data_ptr(), dz.data.data_ptr()
        a.compute, a.operand_layout = dz.compute, L.LAYOUT_C8
        _note(a, L.OP_CONV3_DGRAD)
        L.check(L.load().mtbc_conv3x3_dgrad(C.byref(a), _s()), "conv3x3_dgrad(c8 -> c8)")
        return
    _chk(w, *[d for i, d in enumerate(dxs) if not (i < len(accumulate) and accumulate[i] == 2)])
    N, _, H, W = dz.shape
    a = _conv_args(dxs, w, N, H, W)
    _fill_segs(a.in_, dxs, accumulate)
    a.w_packed, a.dout = packed.data_ptr(), dz.data.data_ptr()
    a.compute, a.operand_layout = dz.compute, L.LAYOUT_C8
    _note(a, L.OP_CONV3_DGRAD)
    L.check(L.load().mtbc_conv3x3_dgrad(C.byref(a), _s()), "conv3x3_dgrad(c8)")


_WGRAD_SYNC: dict = {}       # device -> zeroed int32 counters of the in-kernel split-K reduction (every launch leaves them at zero)


def wgrad_sync_buffer(dev, nbytes: int) -> torch.Tensor:
    buf = _WGRAD_SYNC.get(dev)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.zeros(max(4096, (nbytes + 3) // 4), dtype=torch.int32, device=dev)
        _WGRAD_SYNC[dev] = buf
    return buf


def conv3x3_wgrad_c8(xs: Sequence["C8"], dz: "C8", w_shape, want_bias: bool = False, dw: Optional[torch.Tensor] = None,
                     accumulate: bool = False, in_kernel_reduce: bool = True):
    """in_kernel_reduce: the split-K partials are summed inside the launch by the last-arriving block of each group
    (mtbc_conv3x3_args.wgrad_sync); False = the reduction launch behind the kernel (another, equally fixed, summation order)."""
    N, _, H, W = dz.shape
    dev = dz.data.device
    if dw is None:
        dw = torch.empty(*w_shape, dtype=torch.float32, device=dev)
    db = torch.empty(w_shape[0], dtype=torch.float32, device=dev) if want_bias else None
    a = L.Conv3x3Args()
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, w_shape[1], w_shape[0], len(xs)
    if w_shape[1] <= L.STEM_MAX_CIN and isinstance(xs[0], torch.Tensor):      # the stem: ONE fp32 planar input of 1 .. STEM_MAX_CIN channels, channel-blocked dz
        _fill_segs(a.in_, xs)
    else:
        _fill_segs_c8(a.in_, xs)
    a.dout, a.dw, a.dbias, a.accumulate_dw = dz.data.data_ptr(), dw.data_ptr(), _p(db), int(accumulate)
    a.compute, a.operand_layout = dz.compute, L.LAYOUT_C8
    nb = L.load().mtbc_conv3x3_wgrad_workspace(C.byref(a))
    ws = _ws(nb, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    nsync = int(L.load().mtbc_conv3x3_wgrad_sync_bytes(C.byref(a))) if in_kernel_reduce else 0
    if nsync:
        sync = wgrad_sync_buffer(dev, nsync)
        a.wgrad_sync, a.wgrad_sync_bytes = sync.data_ptr(), sync.numel() * 4
    _note(a, L.OP_CONV3_WGRAD)
    L.check(L.load().mtbc_conv3x3_wgrad(C.byref(a), _s()), "conv3x3_wgrad(c8)")
    return dw, db


# ------------------------------------------------------------------ instance norm + leaky relu
def instnorm_kernel_name(a: "L.InstNormArgs", backward: bool) -> str:
    """Every launch mtbc_instnorm_lrelu_fwd / _bwd would make for `a`, joined with " + ": mtbc_instnorm_kernel_name (launches nothing; planes
    above 64 x 64 with y8 / dz8 ask the device for the team plan, as the call does); raises what the call would."""
    buf = C.create_string_buffer(512)
    L.check(L.load().mtbc_instnorm_kernel_name(C.byref(a), 1 if backward else 0, buf, len(buf)), "instnorm_kernel_name")
    return buf.value.decode()


def instnorm_case_args(backward: bool, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, out: str = "f32",
                       z: str = "f32", affine: bool = True, eps: float = 1e-5, slope: float = 0.01, reserve_cus: int = 0, stats_slots: int = 0,
                       planar: bool = False, planar16: bool = False, pool: bool = False, pool_arg: bool = True, chunk_ws: bool = True,
                       dy: Optional[str] = "f32", n_extra: int = 0, rank1: bool = False, rank1_grads: bool = False, rank1_acc: bool = False,
                       dbias: bool = False, acc: bool = False, defer: bool = False, inplace: bool = False) -> "L.InstNormArgs":
    """The argument struct of ONE InstanceNorm + LeakyReLU call, every field the step programs set (engine._conv_cell / _conv_cell_backward).
    ptrs: field name -> tensor (dy_extra0 .. dy_extra3 for the fan-in); None = distinct 16-byte aligned dummies that nothing may dereference
    (for instnorm_kernel_name).  compute: 0 = the fp32 kernels of norm.hip, 1 / 2 = out16_type.  out: "f32" planes, "p16" 16-bit planes
    (y16 / dz16), "c8" channel-blocked (y8 / dz8).  z: "f32" planes, "c8" channel-blocked of the output type, "c8f16" channel-blocked fp16
    under a bf16 output.  Forward: planar / planar16 = fp32 / 16-bit planes beside y8, stats_slots > 0 = statistics from the conv epilogue,
    pool (+ pool_arg) = the pooled output (+ argmax codes), chunk_ws = offer the chunked-statistics workspace.  Backward: dy "f32" / "c8" /
    None, n_extra planar partials, rank1 (+ the head's own gradients, accumulated or not), pool = the routed max-pool gradient, dbias =
    dbias_pre, acc = accumulate_dparams, defer = defer_dparams, inplace = dz over dy (fp32 planes)."""
    dummy = iter(range(1 << 20, 1 << 30, 1 << 20))

    def ptr(name):
        return next(dummy) if ptrs is None else ptrs[name].data_ptr()

    a = L.InstNormArgs()
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.mean, a.rstd = ptr("z"), ptr("mean"), ptr("rstd")
    if affine:
        a.gamma, a.beta = ptr("gamma"), ptr("beta")
    a.out16_type, a.coop_reserve_cus = compute, reserve_cus
    if z != "f32":
        a.z_layout, a.z_type = L.LAYOUT_C8, (2 if z == "c8f16" else 0)
    a.y_batch_stride = a.dy_batch_stride = Cc * H * W
    if stats_slots:
        a.stats_partial, a.stats_slots = ptr("stats_partial"), stats_slots
    if out == "c8":
        a.coop_state = ptr("coop_state")
    if not backward:
        if out == "c8":
            a.y8 = ptr("y8")
            if planar16:
                a.y16 = ptr("y16")
            elif planar:
                a.y = ptr("y")
            if pool:
                a.pool_y8, a.pool_arg = ptr("pool_y8"), (ptr("pool_arg") if pool_arg else None)
        elif out == "p16":
            a.y16 = ptr("y16")
        else:
            a.y = ptr("y")
        nb = L.load().mtbc_instnorm_fwd_workspace(C.byref(a))
        if nb and chunk_ws:
            a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
        return a
    if dy is not None:
        a.dy = ptr("dy")
        a.dy_layout = L.LAYOUT_C8 if dy == "c8" else L.LAYOUT_PLANAR
    a.n_dy_extra = n_extra
    for k_ in range(n_extra):
        a.dy_extra[k_] = ptr(f"dy_extra{k_}")
    if out == "c8":
        a.dz8 = ptr("dz8")
    elif out == "p16":
        a.dz16 = ptr("dz16")
    else:
        a.dz = a.dy if inplace else ptr("dz")
    if rank1:
        a.dy_rank1, a.dy_rank1_w = ptr("dy_rank1"), ptr("dy_rank1_w")
        if rank1_grads:
            a.dy_rank1_dw, a.dy_rank1_db, a.dy_rank1_accumulate = ptr("dy_rank1_dw"), ptr("dy_rank1_db"), int(rank1_acc)
    if pool:
        a.dy_pool, a.dy_pool_arg = ptr("dy_pool"), ptr("dy_pool_arg")
    if affine:
        a.dgamma, a.dbeta = ptr("dgamma"), ptr("dbeta")
    if dbias:
        a.dbias_pre = ptr("dbias_pre")
    a.accumulate_dparams, a.defer_dparams = int(acc), int(defer)
    a.workspace, a.workspace_bytes = ptr("workspace"), (N * (Cc + 1) * 262 * 4 if ptrs is None else ptrs["workspace"].numel() * 4)
    return a


def instnorm_case_kernel(backward: bool, *shape, **mode) -> str:
    """instnorm_kernel_name of instnorm_case_args(backward, *shape, **mode)."""
    return instnorm_kernel_name(instnorm_case_args(backward, *shape, **mode), backward)


def _note_norm(a, backward: bool) -> None:
    if launched is not None:
        launched.append((L.OP_IN_BWD if backward else L.OP_IN_FWD, instnorm_kernel_name(a, backward)))


def instnorm_launch(a: "L.InstNormArgs", backward: bool) -> None:
    """mtbc_instnorm_lrelu_fwd / _bwd on the current stream for an argument struct of instnorm_case_args(ptrs=...)."""
    _note_norm(a, backward)
    lib = L.load()
    L.check((lib.mtbc_instnorm_lrelu_bwd if backward else lib.mtbc_instnorm_lrelu_fwd)(C.byref(a), _s()), "instnorm_bwd" if backward else "instnorm_fwd")


def instnorm_dparam_desc(a: "L.InstNormArgs", part: int):
    """The descriptor (an array of one) that reduces the partials a backward call with defer_dparams left at address `part` (= its workspace),
    as the step programs build it (MTBC_OP_IN_DPARAM, engine._conv_cell_backward)."""
    d = (L.DparamDesc * 1)()
    d[0].part, d[0].dgamma, d[0].dbeta, d[0].dbias_pre = part, a.dgamma, a.dbeta, a.dbias_pre
    d[0].N, d[0].C, d[0].T, d[0].accumulate = a.N, a.C, L.load().mtbc_instnorm_bwd_team(C.byref(a)), a.accumulate_dparams
    return d


def instnorm_dparam_many(d) -> None:
    """mtbc_instnorm_dparam_many over an array of descriptors on the current stream."""
    if launched is not None:
        launched.extend((L.OP_IN_DPARAM, "in_dparam_many_kernel") for _ in d)
    L.check(L.load().mtbc_instnorm_dparam_many(d, len(d), _s()), "instnorm_dparam_many")


def instnorm_lrelu_fwd(z, gamma=None, beta=None, eps=1e-5, slope=0.01, out16: int = 0):
    """out16 = 1 (bf16) / 2 (fp16): the activation comes back as 16-bit planes (int16 storage), y16 of the C-ABI."""
    _chk(z, gamma, beta)
    N, Cc, H, W = z.shape
    y = torch.empty_like(z, dtype=torch.int16 if out16 else torch.float32)
    mean = torch.empty(N * Cc, dtype=torch.float32, device=z.device)
    rstd = torch.empty_like(mean)
    a = L.InstNormArgs()
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.gamma, a.beta, a.y, a.y_batch_stride = z.data_ptr(), _p(gamma), _p(beta), y.data_ptr(), Cc * H * W
    a.mean, a.rstd = mean.data_ptr(), rstd.data_ptr()
    if out16:
        a.y, a.y16, a.out16_type = None, y.data_ptr(), out16
    nb = L.load().mtbc_instnorm_fwd_workspace(C.byref(a))
    if nb:
        ws = _ws(nb, z.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _note_norm(a, False)
    L.check(L.load().mtbc_instnorm_lrelu_fwd(C.byref(a), _s()), "instnorm_fwd")
    return y, mean, rstd


def instnorm_lrelu_bwd(z, dy, mean, rstd, gamma=None, beta=None, eps=1e-5, slope=0.01, inplace=False,
                       dbias_pre=None, dy_extra=(), out16: int = 0):
    _chk(z, dy, mean, rstd, gamma, beta, dbias_pre, *dy_extra)
    N, Cc, H, W = z.shape
    dz = torch.empty_like(z, dtype=torch.int16) if out16 else (dy if inplace else torch.empty_like(z))
    dg = torch.empty(Cc, dtype=torch.float32, device=z.device) if gamma is not None else None
    db = torch.empty(Cc, dtype=torch.float32, device=z.device) if gamma is not None else None
    ws = _ws(N * Cc * 12, z.device)
    a = L.InstNormArgs()
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.gamma, a.beta, a.mean, a.rstd = z.data_ptr(), _p(gamma), _p(beta), mean.data_ptr(), rstd.data_ptr()
    a.dy, a.dy_batch_stride, a.dz, a.dgamma, a.dbeta = dy.data_ptr(), Cc * H * W, dz.data_ptr(), _p(dg), _p(db)
    a.dbias_pre = _p(dbias_pre)
    if out16:
        a.dz, a.dz16, a.out16_type = None, dz.data_ptr(), out16
    a.n_dy_extra = len(dy_extra)
    for k_, t_ in enumerate(dy_extra):
        a.dy_extra[k_] = t_.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _note_norm(a, True)
    L.check(L.load().mtbc_instnorm_lrelu_bwd(C.byref(a), _s()), "instnorm_bwd")
    return dz, dg, db


_coop_states = {}


def coop_state(dev) -> torch.Tensor:
    """The persistent, zero-initialised mailbox block of the cooperative InstanceNorm kernels (one per device here;
    the C-ABI wants one per stream that launches them)."""
    key = str(dev)
    if key not in _coop_states:
        _coop_states[key] = torch.zeros(L.load().mtbc_instnorm_coop_state_bytes() // 4, dtype=torch.int32, device=dev)
    return _coop_states[key]


def instnorm_lrelu_fwd_c8(z, gamma=None, beta=None, eps=1e-5, slope=0.01, compute: Optional[int] = None, want_planar: bool = False,
                          stats: Optional[torch.Tensor] = None, want_pool: bool = False, planar16: bool = False, reserve_cus: int = 0):
    """InstanceNorm + LeakyReLU straight into the 16-bit channel-blocked layout (y8 of the C-ABI).  z: fp32 planes, or a
    C8 tensor (z_layout = C8: the conv output of the 16-bit modes).  planar16 (with stats): the planar copy is an int16
    (N,C,H,W) tensor of the output type (y16 beside y8).  reserve_cus: coop_reserve_cus of the C-ABI."""
    z8 = z if isinstance(z, C8) else None
    if compute is None:         # output type: given, else the type of a channel-blocked z, else bf16
        compute = z8.compute if z8 is not None else 1
    zt = z8.data if z8 is not None else z
    _chk(zt if z8 is None else None, gamma, beta)
    N, Cc, H, W = z.shape
    dev = zt.device
    y8 = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=dev)
    y = torch.empty(N, Cc, H, W, dtype=torch.int16 if planar16 else torch.float32, device=dev) if (want_planar or planar16) else None
    mean = torch.empty(N * Cc, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    a = L.InstNormArgs()
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.gamma, a.beta, a.y, a.y_batch_stride = zt.data_ptr(), _p(gamma), _p(beta), (None if planar16 else _p(y)), Cc * H * W
    if planar16:
        a.y16 = y.data_ptr()
    a.z_layout = L.LAYOUT_C8 if z8 is not None else L.LAYOUT_PLANAR
    if z8 is not None and z8.compute != compute:
        a.z_type = z8.compute           # fp16 z with bf16 outputs
    a.mean, a.rstd = mean.data_ptr(), rstd.data_ptr()
    a.y8, a.out16_type, a.coop_state, a.coop_reserve_cus = y8.data_ptr(), compute, coop_state(dev).data_ptr(), reserve_cus
    if stats is not None:       # [N][slots][C][2] from conv3x3_fwd_c8(stats=True)
        a.stats_partial, a.stats_slots = stats.data_ptr(), stats.shape[1]
    yp8 = parg = None
    if want_pool:               # the streaming pass also writes the activation's 2x2 max-pool + argmax codes (pool_y8 / pool_arg)
        yp8 = torch.empty(N, Cc // 8, (H // 2) * (W // 2), 8, dtype=torch.int16, device=dev)
        parg = torch.empty(N, Cc // 8, (H // 2) * (W // 2), dtype=torch.int16, device=dev)
        a.pool_y8, a.pool_arg = yp8.data_ptr(), parg.data_ptr()
    if not L.load().mtbc_instnorm_c8_supported(C.byref(a), 0):
        raise L.MtbcError("instnorm_fwd: shape not supported with a channel-blocked output")
    _note_norm(a, False)
    L.check(L.load().mtbc_instnorm_lrelu_fwd(C.byref(a), _s()), "instnorm_fwd(c8)")
    if want_pool:
        return C8(y8, z.shape, compute), mean, rstd, y, C8(yp8, (N, Cc, H // 2, W // 2), compute), parg
    return C8(y8, z.shape, compute), mean, rstd, y


def instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma=None, beta=None, eps=1e-5, slope=0.01, dbias_pre=None, compute: Optional[int] = None,
                          dy_extra: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, rank1=None, rank1_grads: bool = False,
                          pool=None, defer_dparams: bool = False, reserve_cus: int = 0):
    """z / dy: fp32 planes or C8 tensors (z_layout / dy_layout = C8); dy_extra (with a C8 dy only): an fp32 planar partial
    gradient added while loading; rank1 = (dyhead (N,1,H,W), w (C)): the rank-1 gradient term of a one-output 1x1 head (dy may
    then be None).  reserve_cus: coop_reserve_cus of the C-ABI."""
    zt = z.data if isinstance(z, C8) else z
    dyt = dy.data if isinstance(dy, C8) else dy
    if compute is None:         # output (and channel-blocked dy) type: given, else dy's, else z's, else bf16
        compute = dy.compute if isinstance(dy, C8) else (z.compute if isinstance(z, C8) else 1)
    _chk(mean, rstd, gamma, beta, dbias_pre, dy_extra)
    N, Cc, H, W = z.shape
    dev = zt.device
    dz8 = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=dev)
    dg = torch.empty(Cc, dtype=torch.float32, device=dev) if gamma is not None else None
    db = torch.empty(Cc, dtype=torch.float32, device=dev) if gamma is not None else None
    ws = _ws(N * (Cc + 1) * 262 * 4, dev)
    a = L.InstNormArgs()
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.gamma, a.beta, a.mean, a.rstd = zt.data_ptr(), _p(gamma), _p(beta), mean.data_ptr(), rstd.data_ptr()
    a.dy, a.dy_batch_stride, a.dgamma, a.dbeta, a.dbias_pre = (dyt.data_ptr() if dyt is not None else None), Cc * H * W, _p(dg), _p(db), _p(dbias_pre)
    if rank1 is not None:
        _chk(*rank1)
        a.dy_rank1, a.dy_rank1_w = rank1[0].data_ptr(), rank1[1].data_ptr()
    if pool is not None:        # (gradient of the 2x2 max-pool of this activation (N,C,H/2,W/2) fp32, argmax codes from maxpool2_fwd_c8)
        _chk(pool[0])
        a.dy_pool, a.dy_pool_arg = pool[0].data_ptr(), pool[1].data_ptr()
    hdw = hdb = None
    if rank1_grads:             # the head's own weight / bias gradient from the same pass
        hdw, hdb = torch.empty(Cc, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        a.dy_rank1_dw, a.dy_rank1_db = hdw.data_ptr(), hdb.data_ptr()
    a.z_layout = L.LAYOUT_C8 if isinstance(z, C8) else L.LAYOUT_PLANAR
    if isinstance(z, C8) and z.compute != compute:
        a.z_type = z.compute
    a.dy_layout = L.LAYOUT_C8 if isinstance(dy, C8) else L.LAYOUT_PLANAR
    if dy_extra is not None:
        a.n_dy_extra = 1
        a.dy_extra[0] = dy_extra.data_ptr()
    a.dz8, a.out16_type, a.coop_state, a.coop_reserve_cus = dz8.data_ptr(), compute, coop_state(dev).data_ptr(), reserve_cus
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if stats is not None:       # {sum g, sum g * xhat} partials from conv3x3_fwd_c8(norm=...)
        a.stats_partial, a.stats_slots = stats.data_ptr(), stats.shape[1]
    if not L.load().mtbc_instnorm_c8_supported(C.byref(a), 1):
        raise L.MtbcError("instnorm_bwd: shape not supported with a channel-blocked output")
    if defer_dparams:           # leave the partials in the workspace, reduce them with the batched entry point afterwards
        a.defer_dparams = 1
    _note_norm(a, True)
    L.check(L.load().mtbc_instnorm_lrelu_bwd(C.byref(a), _s()), "instnorm_bwd(c8)")
    if defer_dparams:
        instnorm_dparam_many(instnorm_dparam_desc(a, ws.data_ptr()))
    if rank1_grads:
        return C8(dz8, z.shape, compute), dg, db, hdw, hdb
    return C8(dz8, z.shape, compute), dg, db


def coop_error(dev) -> int:
    """1 if a cooperative kernel ever gave up polling its mailbox (protocol failure; results are then garbage)."""
    return int(coop_state(dev)[2].item())


# ------------------------------------------------------------------ maxpool
def maxpool2_fwd(x):
    _chk(x)
    N, Cc, H, W = x.shape
    y = torch.empty(N, Cc, H // 2, W // 2, dtype=torch.float32, device=x.device)
    a = L.MaxPoolArgs()
    a.N, a.C, a.H, a.W = N, Cc, H, W
    a.x, a.x_batch_stride, a.y, a.y_batch_stride = x.data_ptr(), Cc * H * W, y.data_ptr(), Cc * H * W // 4
    L.check(L.load().mtbc_maxpool2_fwd(C.byref(a), _s()), "maxpool_fwd")
    return y


def maxpool2_bwd(x, dy, dx=None, accumulate=False):
    _chk(x, dy, dx)
    N, Cc, H, W = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    a = L.MaxPoolArgs()
    a.N, a.C, a.H, a.W = N, Cc, H, W
    a.x, a.x_batch_stride = x.data_ptr(), Cc * H * W
    a.dy, a.dy_batch_stride, a.dx, a.dx_batch_stride = dy.data_ptr(), Cc * H * W // 4, dx.data_ptr(), Cc * H * W
    a.accumulate_dx = int(accumulate)
    L.check(L.load().mtbc_maxpool2_bwd(C.byref(a), _s()), "maxpool_bwd")
    return dx


def maxpool2_fwd_c8(x8: "C8", want_argmax: bool = False):
    """2x2 max-pool of a channel-blocked 16-bit tensor into one (mtbc_maxpool_args.layout = MTBC_LAYOUT_C8); want_argmax: also the
    (N, C/8, H/2*W/2) int16 codes of where each window's maximum sits (mtbc_maxpool_args.argmax)."""
    N, Cc, H, W = x8.shape
    y = torch.empty(N, Cc // 8, (H // 2) * (W // 2), 8, dtype=torch.int16, device=x8.data.device)
    a = L.MaxPoolArgs()
    a.N, a.C, a.H, a.W, a.layout, a.type16 = N, Cc, H, W, L.LAYOUT_C8, x8.compute
    a.x, a.x_batch_stride, a.y, a.y_batch_stride = x8.data.data_ptr(), Cc * H * W, y.data_ptr(), Cc * H * W // 4
    arg = torch.empty(N, Cc // 8, (H // 2) * (W // 2), dtype=torch.int16, device=x8.data.device) if want_argmax else None
    if arg is not None:
        a.argmax = arg.data_ptr()
    L.check(L.load().mtbc_maxpool2_fwd(C.byref(a), _s()), "maxpool_fwd c8")
    out = C8(y, (N, Cc, H // 2, W // 2), x8.compute)
    return (out, arg) if want_argmax else out


def maxpool2_bwd_c8(x8: "C8", dy, dx=None, accumulate=False):
    _chk(dy, dx)
    N, Cc, H, W = x8.shape
    if dx is None:
        dx = torch.empty(N, Cc, H, W, dtype=torch.float32, device=dy.device)
    a = L.MaxPoolArgs()
    a.N, a.C, a.H, a.W, a.layout, a.type16 = N, Cc, H, W, L.LAYOUT_C8, x8.compute
    a.x, a.x_batch_stride = x8.data.data_ptr(), Cc * H * W
    a.dy, a.dy_batch_stride, a.dx, a.dx_batch_stride = dy.data_ptr(), Cc * H * W // 4, dx.data_ptr(), Cc * H * W
    a.accumulate_dx = int(accumulate)
    L.check(L.load().mtbc_maxpool2_bwd(C.byref(a), _s()), "maxpool_bwd c8")
    return dx


# ------------------------------------------------------------------ conv transpose (k == stride)
def convT_kernel_name(a: "L.ConvTArgs", op: int, dgrad_next: Optional["L.ConvTArgs"] = None) -> str:
    """Every launch mtbc_convT_fwd / _dgrad / _wgrad -- op = L.OP_CONVT_FWD / _DGRAD / _WGRAD -- would make for `a`, joined with " + ":
    mtbc_convT_kernel_name, host-only (no launch, no device).  dgrad_next (with L.OP_CONVT_WGRAD): the arguments of the OP_CONVT_DGRAD
    right behind it in a program; the name is then what the program runner makes of the pair.  Raises what the call would."""
    buf = C.create_string_buffer(512)
    nxt = None if dgrad_next is None else C.byref(dgrad_next)
    L.check(L.load().mtbc_convT_kernel_name(C.byref(a), op, nxt, buf, len(buf)), "convT_kernel_name")
    return buf.value.decode()


_CT_DUMMY = {n: (i + 1) << 20 for i, n in enumerate(("x", "w", "bias", "y", "dy", "dx", "dw", "dbias", "workspace"))}


def convT_case_args(op: int, N: int, Cin: int, Cout: int, H: int, W: int, k: int = 2, ptrs: Optional[dict] = None, compute: int = 0,
                    dy16: bool = False, x16: bool = False, x_c8: bool = False, y_c8: bool = False, bias: bool = True,
                    acc_dx: bool = False, acc_dw: bool = False, strides: Optional[dict] = None, workspace: bool = True) -> "L.ConvTArgs":
    """The argument struct of ONE transposed-convolution call as the step programs fill it (engine.StepPlan.convT / convT_head).
    ptrs: field name (x, w, bias, y, dy, dx, dw, dbias, workspace) -> tensor; None = distinct 16-byte aligned dummies that nothing may
    dereference (for convT_kernel_name), the same address for the same field of every call so that a WGRAD and the DGRAD behind it
    describe one problem.  Forward: x_c8 / y_c8 = 16-bit channel-blocked input / output of type `compute`; bias = with a bias.
    Backward: `compute` = the MFMA operand type, dy16 / x16 = dy / x as 16-bit planes of that type, bias = with dbias (weight gradient),
    acc_dx / acc_dw = accumulate.  strides: field name (x, y, dy, dx) -> batch stride in elements of that tensor where the tensor is a
    channel-range view of a wider buffer; dense otherwise.  workspace = False leaves the weight gradient without one."""
    strides = strides or {}

    def ptr(name):
        return _CT_DUMMY[name] if ptrs is None else ptrs[name].data_ptr()

    a = L.ConvTArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k = N, H, W, Cin, Cout, k
    a.w = ptr("w")
    a.x_batch_stride = strides.get("x", Cin * H * W)
    a.y_batch_stride = strides.get("y", Cout * H * k * W * k)
    if op == L.OP_CONVT_FWD:
        a.x, a.y, a.bias = ptr("x"), ptr("y"), (ptr("bias") if bias else None)
        if y_c8:
            a.y_layout, a.y_type = L.LAYOUT_C8, compute
        if x_c8:
            a.x_layout = L.LAYOUT_C8
        return a
    a.compute = compute
    a.dy, a.dy_batch_stride, a.dy_type16 = ptr("dy"), strides.get("dy", Cout * H * k * W * k), (compute if dy16 else 0)
    if op == L.OP_CONVT_DGRAD:
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cin * H * W), int(acc_dx)
        return a
    a.x, a.x_type16 = ptr("x"), (compute if x16 else 0)
    a.dw, a.dbias, a.accumulate_dw = ptr("dw"), (ptr("dbias") if bias else None), int(acc_dw)
    if workspace:
        nb = int(L.load().mtbc_convT_wgrad_workspace(C.byref(a)))
        a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
    return a


def convT_case_kernel(op: int, *shape, pair: bool = False, **mode) -> str:
    """convT_kernel_name of convT_case_args(op, *shape, **mode); pair (with L.OP_CONVT_WGRAD): followed by the L.OP_CONVT_DGRAD of the
    same problem and mode, as engine.StepPlan.convT emits the two."""
    nxt = convT_case_args(L.OP_CONVT_DGRAD, *shape, **mode) if pair else None
    return convT_kernel_name(convT_case_args(op, *shape, **mode), op, nxt)


def convT_note(a: "L.ConvTArgs", op: int, dgrad_next: Optional["L.ConvTArgs"] = None) -> None:
    """Records (op, launches) of a transposed-convolution call -- or of a program's WGRAD + DGRAD pair -- while `launched` is a list."""
    if launched is not None:
        launched.append((op, convT_kernel_name(a, op, dgrad_next)))


def convT_launch(a: "L.ConvTArgs", op: int) -> None:
    """mtbc_convT_fwd / _dgrad / _wgrad on the current stream for an argument struct of convT_case_args(ptrs=...)."""
    convT_note(a, op)
    lib = L.load()
    fn, what = {L.OP_CONVT_FWD: (lib.mtbc_convT_fwd, "convT_fwd"), L.OP_CONVT_DGRAD: (lib.mtbc_convT_dgrad, "convT_dgrad"),
                L.OP_CONVT_WGRAD: (lib.mtbc_convT_wgrad, "convT_wgrad")}[op]
    L.check(fn(C.byref(a), _s()), what)


def _ct_args(x, w, k):
    a = L.ConvTArgs()
    N, Cin, H, W = x.shape
    a.N, a.H, a.W, a.Cin, a.Cout, a.k = N, H, W, Cin, w.shape[1], k
    a.x, a.x_batch_stride, a.w = x.data_ptr(), Cin * H * W, w.data_ptr()
    return a


def convT_fwd(x, w, bias, k):
    _chk(x, w, bias)
    N, Cin, H, W = x.shape
    y = torch.empty(N, w.shape[1], H * k, W * k, dtype=torch.float32, device=x.device)
    a = _ct_args(x, w, k)
    a.bias, a.y, a.y_batch_stride = _p(bias), y.data_ptr(), y[0].numel()
    convT_note(a, L.OP_CONVT_FWD)
    L.check(L.load().mtbc_convT_fwd(C.byref(a), _s()), "convT_fwd")
    return y


def convT_fwd_c8(x, w, bias, k, compute: int) -> "C8":
    """ConvTranspose2d(k = s) forward written straight into the 16-bit channel-blocked layout (y_layout = C8)."""
    _chk(x, w, bias)
    a = _ct_args(x, w, k)
    N, _, H, W = x.shape
    cout = w.shape[1]
    y = torch.empty(N, cout // 8, H * k * W * k, 8, dtype=torch.int16, device=x.device)
    a.bias, a.y, a.y_batch_stride = _p(bias), y.data_ptr(), cout * H * k * W * k
    a.y_layout, a.y_type = L.LAYOUT_C8, compute
    if not L.load().mtbc_convT_fwd_c8_supported(C.byref(a)):
        raise L.MtbcError("convT_fwd: shape not supported with a channel-blocked output")
    convT_note(a, L.OP_CONVT_FWD)
    L.check(L.load().mtbc_convT_fwd(C.byref(a), _s()), "convT_fwd(c8)")
    return C8(y, (N, cout, H * k, W * k), compute)


def convT_fwd_c8_lp(x8: "C8", w, bias, k) -> "C8":
    """ConvTranspose2d(k = s = 2) forward on the 16-bit MFMA, input and output channel-blocked (x_layout = y_layout = C8)."""
    _chk(w, bias)
    N, Cin, H, W = x8.shape
    cout = w.shape[1]
    a = L.ConvTArgs()
    a.N, a.H, a.W, a.Cin, a.Cout, a.k = N, H, W, Cin, cout, k
    a.x, a.x_batch_stride, a.w = x8.data.data_ptr(), Cin * H * W, w.data_ptr()
    y = torch.empty(N, cout // 8, H * k * W * k, 8, dtype=torch.int16, device=w.device)
    a.bias, a.y, a.y_batch_stride = _p(bias), y.data_ptr(), cout * H * k * W * k
    a.y_layout, a.y_type, a.x_layout = L.LAYOUT_C8, x8.compute, L.LAYOUT_C8
    if not L.load().mtbc_convT_fwd_c8_supported(C.byref(a)):
        raise L.MtbcError("convT_fwd: shape not supported with channel-blocked input and output")
    convT_note(a, L.OP_CONVT_FWD)
    L.check(L.load().mtbc_convT_fwd(C.byref(a), _s()), "convT_fwd(c8 -> c8)")
    return C8(y, (N, cout, H * k, W * k), x8.compute)


def convT_dgrad(x, w, dy, k, dx=None, accumulate=False, compute=0, dy16=False):
    """dy16: dy is an int16 (N,Cout,kH,kW) tensor holding 16-bit planar values of the type of `compute`."""
    _chk(x, w, None if dy16 else dy, dx)
    if dx is None:
        dx = torch.empty_like(x)
    a = _ct_args(x, w, k)
    a.compute = compute
    a.dy_type16 = compute if dy16 else 0
    a.dy, a.dy_batch_stride, a.dx, a.dx_batch_stride, a.accumulate_dx = dy.data_ptr(), dy[0].numel(), dx.data_ptr(), x[0].numel(), int(accumulate)
    convT_note(a, L.OP_CONVT_DGRAD)
    L.check(L.load().mtbc_convT_dgrad(C.byref(a), _s()), "convT_dgrad")
    return dx


def convT_wgrad(x, w, dy, k, want_bias=True, compute=0, dy16=False, x16=False):
    """x16 (with dy16): x is an int16 (N,Cin,H,W) tensor of 16-bit planar values of the type of `compute` too."""
    _chk(None if x16 else x, w, None if dy16 else dy)
    dw = torch.empty_like(w)
    db = torch.empty(w.shape[1], dtype=torch.float32, device=x.device) if want_bias else None
    a = _ct_args(x, w, k)
    a.compute = compute
    a.dy_type16 = compute if dy16 else 0
    a.x_type16 = compute if x16 else 0
    a.dy, a.dy_batch_stride, a.dw, a.dbias = dy.data_ptr(), dy[0].numel(), dw.data_ptr(), _p(db)
    ws = _ws(L.load().mtbc_convT_wgrad_workspace(C.byref(a)), x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    convT_note(a, L.OP_CONVT_WGRAD)
    L.check(L.load().mtbc_convT_wgrad(C.byref(a), _s()), "convT_wgrad")
    return dw, db


# ------------------------------------------------------------------ conv1x1
def _c1_args(x, w):
    a = L.Conv1x1Args()
    N, Cin, H, W = x.shape
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, w.shape[0]
    a.x, a.x_batch_stride, a.w = x.data_ptr(), Cin * H * W, w.data_ptr()
    return a


def conv1x1_fwd(x, w, bias):
    _chk(x, w, bias)
    N, _, H, W = x.shape
    y = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=x.device)
    a = _c1_args(x, w)
    a.bias, a.y = _p(bias), y.data_ptr()
    L.check(L.load().mtbc_conv1x1_fwd(C.byref(a), _s()), "conv1x1_fwd")
    return y


def conv1x1_bwd(x, w, dy):
    _chk(x, w, dy)
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device)
    a = _c1_args(x, w)
    a.dy, a.dx, a.dx_batch_stride = dy.data_ptr(), dx.data_ptr(), x[0].numel()
    L.check(L.load().mtbc_conv1x1_dgrad(C.byref(a), _s()), "conv1x1_dgrad")
    a.dw, a.dbias = dw.data_ptr(), db.data_ptr()
    ws = _ws(L.load().mtbc_conv1x1_wgrad_workspace(C.byref(a)), x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    L.check(L.load().mtbc_conv1x1_wgrad(C.byref(a), _s()), "conv1x1_wgrad")
    return dx, dw, db


def conv1x1_fwd_c8(x8: "C8", w, bias):
    """1x1 conv reading the channel-blocked 16-bit activation (mtbc_conv1x1_args.x_layout = MTBC_LAYOUT_C8)."""
    _chk(w, bias)
    N, Cin, H, W = x8.shape
    y = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=w.device)
    a = L.Conv1x1Args()
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, w.shape[0]
    a.x, a.x_batch_stride, a.w, a.x_layout, a.x_type = x8.data.data_ptr(), Cin * H * W, w.data_ptr(), L.LAYOUT_C8, x8.compute
    a.bias, a.y = _p(bias), y.data_ptr()
    L.check(L.load().mtbc_conv1x1_fwd(C.byref(a), _s()), "conv1x1_fwd c8")
    return y


def conv1x1_wgrad_c8(x8: "C8", w, dy, accumulate=False, dw=None, db=None):
    _chk(w, dy)
    N, Cin, H, W = x8.shape
    dw = torch.empty_like(w) if dw is None else dw
    db = torch.empty(w.shape[0], dtype=torch.float32, device=w.device) if db is None else db
    a = L.Conv1x1Args()
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, w.shape[0]
    a.x, a.x_batch_stride, a.w, a.x_layout, a.x_type = x8.data.data_ptr(), Cin * H * W, w.data_ptr(), L.LAYOUT_C8, x8.compute
    a.dy, a.dw, a.dbias, a.accumulate_dw = dy.data_ptr(), dw.data_ptr(), db.data_ptr(), int(accumulate)
    ws = _ws(L.load().mtbc_conv1x1_wgrad_workspace(C.byref(a)), w.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    L.check(L.load().mtbc_conv1x1_wgrad(C.byref(a), _s()), "conv1x1_wgrad c8")
    return dw, db


# ------------------------------------------------------------------ head
def gap_fwd(x):
    _chk(x)
    N, Cc, H, W = x.shape
    y = torch.empty(N, Cc, dtype=torch.float32, device=x.device)
    a = L.GapArgs()
    a.N, a.C, a.H, a.W, a.x, a.y = N, Cc, H, W, x.data_ptr(), y.data_ptr()
    L.check(L.load().mtbc_gap_fwd(C.byref(a), _s()), "gap_fwd")
    return y


def gap_bwd(dy, H, W):
    _chk(dy)
    N, Cc = dy.shape
    dx = torch.empty(N, Cc, H, W, dtype=torch.float32, device=dy.device)
    a = L.GapArgs()
    a.N, a.C, a.H, a.W, a.dy, a.dx = N, Cc, H, W, dy.data_ptr(), dx.data_ptr()
    L.check(L.load().mtbc_gap_bwd(C.byref(a), _s()), "gap_bwd")
    return dx


def linear_fwd(x, w, b, relu=False):
    _chk(x, w, b)
    y = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    a = L.LinearArgs()
    a.N, a.In, a.Out, a.relu = x.shape[0], x.shape[1], w.shape[0], int(relu)
    a.x, a.w, a.bias, a.y = x.data_ptr(), w.data_ptr(), _p(b), y.data_ptr()
    L.check(L.load().mtbc_linear_fwd(C.byref(a), _s()), "linear_fwd")
    return y


def linear_bwd(x, w, y, dy, relu=False):
    _chk(x, w, y, dy)
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device)
    ws = _ws(x.shape[0] * w.shape[0] * 4, x.device)
    a = L.LinearArgs()
    a.N, a.In, a.Out, a.relu = x.shape[0], x.shape[1], w.shape[0], int(relu)
    a.x, a.w, a.y, a.dy = x.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr()
    a.dx, a.dw, a.dbias = dx.data_ptr(), dw.data_ptr(), db.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    L.check(L.load().mtbc_linear_bwd(C.byref(a), _s()), "linear_bwd")
    return dx, dw, db


# ------------------------------------------------------------------ losses / optimiser
def dice_multihead(xs: Sequence[torch.Tensor], target, weights: Sequence[float], gscale: float = 1.0, kind: int = 0,
                   smooth: Optional[Tuple[float, float]] = None, focal_gamma: float = 2.0):
    """returns (loss[n_heads+1], [dx per head]).  kind: L.SEG_DICE (0, the default) | SEG_BCE | SEG_FOCALDICE | SEG_JACCARD; `smooth` = (nr, dr),
    default the reference's for the kind (1 / 1; Jaccard: MONAI's 1e-5 / 1e-5)."""
    _chk(*xs, target)
    nh = len(xs)
    N, Cc, H, W = xs[0].shape
    dev = target.device
    stats = torch.empty(nh * N * Cc * L.SEG_STATS_STRIDE[kind], dtype=torch.float32, device=dev)
    loss = torch.empty(nh + 1, dtype=torch.float32, device=dev)
    dxs = [torch.empty_like(x) for x in xs]
    a = L.DiceArgs()
    nr, dr = smooth if smooth is not None else ((1e-5, 1e-5) if kind == L.SEG_JACCARD else (1.0, 1.0))
    a.n_heads, a.N, a.C, a.H, a.W, a.smooth_nr, a.smooth_dr = nh, N, Cc, H, W, nr, dr
    if kind != L.SEG_DICE:
        a.kind, a.focal_gamma = kind, (focal_gamma if kind == L.SEG_FOCALDICE else 0.0)
    for i in range(nh):
        a.x[i], a.dx[i], a.head_weight[i] = xs[i].data_ptr(), dxs[i].data_ptr(), weights[i]
    a.target, a.stats, a.loss, a.gscale = target.data_ptr(), stats.data_ptr(), loss.data_ptr(), gscale
    L.check(L.load().mtbc_dice_fwd(C.byref(a), _s()), "dice_fwd")
    L.check(L.load().mtbc_dice_bwd(C.byref(a), _s()), "dice_bwd")
    return loss, dxs


def focal(x, t, alpha=1.0, gamma=2.0, weight=None, gscale=1.0):
    _chk(x, t, weight)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    a = L.FocalArgs()
    a.N, a.C, a.alpha, a.gamma = x.shape[0], x.shape[1], alpha, gamma
    a.x, a.target, a.weight, a.loss, a.dx, a.gscale = x.data_ptr(), t.data_ptr(), _p(weight), loss.data_ptr(), dx.data_ptr(), gscale
    L.check(L.load().mtbc_focal_fwd_bwd(C.byref(a), _s()), "focal")
    return loss, dx


def adam_step(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-4, grad_scale=1.0, zero_grad=False):
    """Adam on the shared optimizer launch: the AdamW rule with weight_decay 0 (a decay factor of exactly 1)."""
    optim_step(L.OPT_ADAMW, p, g, m, v, lr=lr, step=step, beta1=beta1, beta2=beta2, eps=eps, weight_decay=0.0, grad_scale=grad_scale, zero_grad=zero_grad)


# ------------------------------------------------------------------ dynamic loss scale (op level; `state` = 16 int32 words on the device = mtbc_loss_scale_state)
def _loss_scale_args(state, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, world=1, beta1=0.9, beta2=0.999, gscale_out=None, g=None):
    if state.device.type != "cuda":
        L.require_gpu()
        raise L.MtbcError("device tensors required")
    if state.dtype != torch.int32 or not state.is_contiguous() or state.numel() * 4 < C.sizeof(L.LossScaleState):
        raise ValueError("loss-scale state: 16 contiguous int32 words on the device")
    a = L.LossScaleArgs()
    a.state = state.data_ptr()
    a.gscale_out = gscale_out.data_ptr() if gscale_out is not None else None
    if g is not None:
        a.g, a.n = g.data_ptr(), g.numel()
    a.growth_factor, a.backoff_factor, a.growth_interval = growth_factor, backoff_factor, growth_interval
    a.inv_world, a.beta1, a.beta2 = 1.0 / world, beta1, beta2
    return a


def loss_scale_begin(state, gscale_out, world=1, beta1=0.9, beta2=0.999):
    """*gscale_out = shard_weight * scale; state.adam = Adam's three scalars of step t + 1 (state.lr, state.scale, 1 / world)."""
    _chk(gscale_out)
    L.check(L.load().mtbc_loss_scale_begin(C.byref(_loss_scale_args(state, world=world, beta1=beta1, beta2=beta2, gscale_out=gscale_out)), _s()), "loss scale begin")


def loss_scale_check(state, g):
    """state.found_inf |= any(g is inf or NaN)."""
    _chk(g)
    L.check(L.load().mtbc_loss_scale_check(C.byref(_loss_scale_args(state, g=g)), _s()), "loss scale check")


def loss_scale_adam(state, p, g, m, v, beta1=0.9, beta2=0.999, eps=1e-4, zero_grad=False, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """Adam with the scalars `loss_scale_begin` left, skipped when state.found_inf is set; then the scale / tracker / t / skipped update."""
    _chk(p, g, m, v)
    ad = optim_args(L.OPT_ADAMW, p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), beta1=beta1, beta2=beta2, eps=eps, weight_decay=0.0,
                    zero_grad=zero_grad)
    a = _loss_scale_args(state, growth_factor, backoff_factor, growth_interval, beta1=beta1, beta2=beta2)
    L.check(L.load().mtbc_loss_scale_optim(C.byref(a), C.byref(ad), _s()), "loss scale adam")


# ------------------------------------------------------------------ fused Adam / SGD (Nesterov) / AdamW (op level)
def optim_args(kind, n, p, g, m, v=None, lr=1e-3, step=1, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.9, weight_decay=0.0, grad_scale=1.0,
               zero_grad=False, nesterov=True, dynamic=None, skip=None, scale_state=None):
    """mtbc_optim_args from ADDRESSES (device pointers for optim_step, host pointers for mtbc_optim_step_host)."""
    a = L.OptimArgs()
    a.kind, a.n, a.p, a.g, a.m, a.v = kind, n, p, g, m, v
    a.lr, a.beta1, a.beta2, a.eps, a.momentum, a.weight_decay, a.grad_scale = lr, beta1, beta2, eps, momentum, weight_decay, grad_scale
    a.step, a.zero_grad, a.nesterov = step, int(zero_grad), int(nesterov)
    a.dynamic, a.skip, a.scale_state = dynamic, skip, scale_state
    return a


def optim_step(kind, p, g, m, v=None, dynamic=None, skip=None, **hyper):
    """One fused SGD (kind = L.OPT_SGD; `m` is the momentum buffer) or AdamW (L.OPT_ADAMW; Adam with weight_decay 0) launch on device tensors; `dynamic`: 4 device floats as
    mtbc_optim_dynamic writes them, `skip`: a device int32 word."""
    _chk(p, g, m, v, dynamic)
    a = optim_args(kind, p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr() if v is not None else None,
                   dynamic=dynamic.data_ptr() if dynamic is not None else None, skip=skip.data_ptr() if skip is not None else None, **hyper)
    L.check(L.load().mtbc_optim_step(C.byref(a), _s()), "optim")


# ------------------------------------------------------------------ fused ConvT + 1x1 head (MTnnUNet deep supervision)
def convT_head_fwd_bwd(x, wT, bT, w1, b1, k, dout):
    """Forward and backward of Conv2d_1x1(ConvTranspose2d_k(x)) through the combined-weight path
    (mtbc_convT_head_combine -> mtbc_convT_* with Cout = R -> mtbc_convT_head_expand).
    Returns (y, dx, dwT, dbT, dw1, db1)."""
    _chk(x, wT, bT, w1, b1, dout)
    lib = L.load()
    cin, cmid, R = wT.shape[0], wT.shape[1], w1.shape[0]
    dev = x.device
    Wc, bc = torch.empty(cin, R, k, k, device=dev), torch.empty(R, device=dev)
    a = L.HeadFuseArgs()
    a.Cin, a.Cmid, a.R, a.k = cin, cmid, R, k
    a.wT, a.bT, a.w1, a.b1 = wT.data_ptr(), bT.data_ptr(), w1.data_ptr(), b1.data_ptr()
    a.Wc, a.bc = Wc.data_ptr(), bc.data_ptr()
    L.check(lib.mtbc_convT_head_combine(C.byref(a), _s()), "head_combine")
    y = convT_fwd(x, Wc, bc, k)
    dx = convT_dgrad(x, Wc, dout, k)
    G, gb = convT_wgrad(x, Wc, dout, k)
    dwT, dbT, dw1, db1 = torch.empty_like(wT), torch.empty_like(bT), torch.empty_like(w1), torch.empty_like(b1)
    a.G, a.gb = G.data_ptr(), gb.data_ptr()
    a.dwT, a.dbT, a.dw1, a.db1 = dwT.data_ptr(), dbT.data_ptr(), dw1.data_ptr(), db1.data_ptr()
    L.check(lib.mtbc_convT_head_expand(C.byref(a), _s()), "head_expand")
    return y, dx, dwT, dbT, dw1, db1


# ------------------------------------------------------------------ the small ops as step-program ops: plan query, argument structs, launch
SMALL_OPS = (L.OP_POOL_FWD, L.OP_POOL_BWD, L.OP_CONV1_FWD, L.OP_CONV1_DGRAD, L.OP_CONV1_WGRAD, L.OP_GAP_FWD, L.OP_GAP_BWD,
             L.OP_LINEAR_FWD, L.OP_LINEAR_BWD, L.OP_HEAD_COMBINE, L.OP_HEAD_EXPAND)


def op_kernel_name(op: "L.Op") -> str:
    """Every launch the call behind a max-pool, 1x1 convolution, GAP, Linear or fused-head op (SMALL_OPS) would make, joined with " + ":
    mtbc_op_kernel_name, host-only (no launch, no device).  Raises what the call would."""
    buf = C.create_string_buffer(512)
    L.check(L.load().mtbc_op_kernel_name(C.byref(op), buf, len(buf)), "op_kernel_name")
    return buf.value.decode()


_SMALL_DUMMY = {n: (i + 1) << 20 for i, n in enumerate(("x", "w", "bias", "y", "dy", "dx", "dw", "dbias", "workspace", "argmax", "wT", "bT", "w1", "b1",
                                                        "Wc", "bc", "G", "gb", "dwT", "dbT", "dw1", "db1"))}


def _small_ptr(ptrs: Optional[dict]):
    return (lambda name: _SMALL_DUMMY[name]) if ptrs is None else (lambda name: ptrs[name].data_ptr())


def _small_op(kind: int) -> "L.Op":
    op = L.Op()
    op.kind = kind
    return op


def maxpool_case_args(kind: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, argmax: bool = False,
                      acc_dx: bool = False, strides: Optional[dict] = None) -> "L.Op":
    """The MTBC_OP_POOL_FWD / _BWD op of ONE 2x2 max-pool call as engine.StepPlan.maxpool fills it.  ptrs: field name (x, y, dy, dx, argmax) ->
    tensor; None = distinct 16-byte aligned dummies that nothing may dereference (for op_kernel_name).  compute: 0 = fp32 planar x / y, 1 / 2 =
    16-bit channel-blocked x / y of that type (layout C8; dy / dx stay fp32 planes); argmax: the forward also writes the codes; acc_dx: the
    backward adds into dx.  strides: field name (x, y, dy, dx) -> batch stride in elements of that tensor where it is a channel-range view of a
    wider buffer; dense otherwise."""
    strides, ptr = strides or {}, _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.pool
    a.N, a.C, a.H, a.W = N, Cc, H, W
    if compute:
        a.layout, a.type16 = L.LAYOUT_C8, compute
    a.x, a.x_batch_stride = ptr("x"), strides.get("x", Cc * H * W)
    a.y, a.y_batch_stride = ptr("y"), strides.get("y", Cc * H * W // 4)      # engine.StepPlan.maxpool's base(): both ops carry x and y
    if kind == L.OP_POOL_FWD:
        a.argmax = ptr("argmax") if argmax else None
    else:
        a.dy, a.dy_batch_stride = ptr("dy"), strides.get("dy", Cc * H * W // 4)
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cc * H * W), int(acc_dx)
    return op


def conv1x1_case_args(kind: int, N: int, Cin: int, Cout: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, bias: bool = True,
                      acc_dx: bool = False, acc_dw: bool = False, strides: Optional[dict] = None, workspace: bool = True) -> "L.Op":
    """The MTBC_OP_CONV1_FWD / _DGRAD / _WGRAD op of ONE 1x1 convolution call as engine.StepPlan.conv1x1 fills it.  ptrs: field name (x, w,
    bias, y, dy, dx, dw, dbias, workspace) -> tensor, None = dummies.  compute: 0 = fp32 planar x, 1 / 2 = 16-bit channel-blocked x of that
    type.  bias: forward with a bias / weight gradient with dbias; acc_dx / acc_dw: accumulate.  strides: x, dx -> batch stride of a view
    (y and dy are always dense).  workspace = False leaves the weight gradient without one."""
    strides, ptr = strides or {}, _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.conv1
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, Cout
    a.x, a.x_batch_stride, a.w = ptr("x"), strides.get("x", Cin * H * W), ptr("w")
    if compute:
        a.x_layout, a.x_type = L.LAYOUT_C8, compute
    if kind == L.OP_CONV1_FWD:
        a.bias, a.y = (ptr("bias") if bias else None), ptr("y")
        return op
    a.dy = ptr("dy")
    if kind == L.OP_CONV1_DGRAD:
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cin * H * W), int(acc_dx)
        return op
    a.dw, a.dbias, a.accumulate_dw = ptr("dw"), (ptr("dbias") if bias else None), int(acc_dw)
    if workspace:
        nb = int(L.load().mtbc_conv1x1_wgrad_workspace(C.byref(a)))
        a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
    return op


def gap_case_args(kind: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None) -> "L.Op":
    """The MTBC_OP_GAP_FWD / _BWD op as engine.StepPlan.gap fills it (x, y / dy, dx; all dense)."""
    ptr = _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.gap
    a.N, a.C, a.H, a.W = N, Cc, H, W
    a.x, a.y = ptr("x"), ptr("y")           # engine.StepPlan.gap's base(): both ops carry x and y
    if kind == L.OP_GAP_BWD:
        a.dy, a.dx = ptr("dy"), ptr("dx")
    return op


def linear_case_args(kind: int, N: int, In: int, Out: int, ptrs: Optional[dict] = None, relu: bool = False, bias: bool = True, dx: bool = True,
                     acc_dw: bool = False, workspace: bool = True) -> "L.Op":
    """The MTBC_OP_LINEAR_FWD / _BWD op as engine.StepPlan.linear fills it.  ptrs: x, w, bias, y, dy, dx, dw, dbias, workspace.  bias: the
    forward's bias (the backward always has dbias, as in the programs); dx = False: no input gradient; workspace: the backward with relu gets
    its N * Out floats (the engine gives one to the ReLU layers only)."""
    ptr = _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.linear
    a.N, a.In, a.Out, a.relu = N, In, Out, int(relu)
    a.x, a.w, a.bias, a.y = ptr("x"), ptr("w"), (ptr("bias") if bias else None), ptr("y")
    if kind == L.OP_LINEAR_BWD:
        a.dy, a.dx = ptr("dy"), (ptr("dx") if dx else None)
        a.dw, a.dbias, a.accumulate_dw = ptr("dw"), ptr("dbias"), int(acc_dw)
        if relu and workspace:
            a.workspace, a.workspace_bytes = ptr("workspace"), (N * Out * 4 if ptrs is None else ptrs["workspace"].numel() * 4)
    return op


def head_case_args(kind: int, Cin: int, Cmid: int, R: int, k: int, ptrs: Optional[dict] = None, bT: bool = True, b1: bool = True,
                   dbT: bool = True, db1: bool = True, acc: Sequence[int] = (0, 0, 0, 0)) -> "L.Op":
    """The MTBC_OP_HEAD_COMBINE / _EXPAND op as engine.StepPlan.convT_head fills it (every pointer in both ops).  ptrs: wT, bT, w1, b1, Wc, bc,
    G, gb, dwT, dbT, dw1, db1.  bT / b1 = False: the layer has no bias; dbT / db1 = False: that gradient is not asked for; acc = (acc_wT,
    acc_bT, acc_w1, acc_b1)."""
    ptr = _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.head
    a.Cin, a.Cmid, a.R, a.k = Cin, Cmid, R, k
    a.wT, a.bT, a.w1, a.b1 = ptr("wT"), (ptr("bT") if bT else None), ptr("w1"), (ptr("b1") if b1 else None)
    a.Wc, a.bc, a.G, a.gb = ptr("Wc"), ptr("bc"), ptr("G"), ptr("gb")
    if kind == L.OP_HEAD_EXPAND:
        a.dwT, a.dbT, a.dw1, a.db1 = ptr("dwT"), (ptr("dbT") if dbT else None), ptr("dw1"), (ptr("db1") if db1 else None)
        a.acc_wT, a.acc_bT, a.acc_w1, a.acc_b1 = (int(v) for v in acc)
    return op


def small_op_launch(op: "L.Op") -> None:
    """The entry point behind a small op (SMALL_OPS) on the current stream, for an op of the *_case_args(ptrs=...) helpers above; records
    (kind, launches) while `launched` is a list."""
    lib = L.load()
    fn = {L.OP_POOL_FWD: lib.mtbc_maxpool2_fwd, L.OP_POOL_BWD: lib.mtbc_maxpool2_bwd, L.OP_CONV1_FWD: lib.mtbc_conv1x1_fwd,
          L.OP_CONV1_DGRAD: lib.mtbc_conv1x1_dgrad, L.OP_CONV1_WGRAD: lib.mtbc_conv1x1_wgrad, L.OP_GAP_FWD: lib.mtbc_gap_fwd,
          L.OP_GAP_BWD: lib.mtbc_gap_bwd, L.OP_LINEAR_FWD: lib.mtbc_linear_fwd, L.OP_LINEAR_BWD: lib.mtbc_linear_bwd,
          L.OP_HEAD_COMBINE: lib.mtbc_convT_head_combine, L.OP_HEAD_EXPAND: lib.mtbc_convT_head_expand}[op.kind]
    if launched is not None:
        launched.append((op.kind, op_kernel_name(op)))
    L.check(fn(C.byref(getattr(op.u, L.OP_UNION_FIELD[op.kind])), _s()), f"small op {op.kind}")
