"""Tensor-level wrappers over the per-op C-ABI (one call = one mtbc_* entry point).

Used by the parity tests and as the reference-side binding example of INTEGRATION.md; the training path itself
goes through step programs (engine.py).  Device fp32 tensors only; every wrapper raises on CPU input.

Each argument struct is filled in ONE function, the family's *_case_args builder: with ptrs=None it carries dummy addresses for the host-only
*_kernel_name queries (the launch-coverage guards of the tests), with ptrs= tensors it is what conv3x3_launch / instnorm_launch /
convT_launch / small_op_launch / loss_op_launch hand the library.  The eager wrappers validate, allocate, call the builder and launch; the
step programs' ops -- the conv cells' 3x3 convolutions and InstanceNorms, pool, 1x1, GAP, Linear, ConvT, fused head, up-sampling, losses -- are
filled by the same builders (engine.StepPlan).
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
    """The address of a tensor or of a C8 tensor's storage; None stays None (a NULL field)."""
    return None if t is None else (t.data if isinstance(t, C8) else t).data_ptr()


def _ptr(ptrs: Optional[dict], dummy):
    """name -> the address a *_case_args builder puts into a pointer field: of ptrs[name] (a tensor, a C8, or None for NULL), or with
    ptrs = None dummy(name), a 16-byte aligned address that nothing may dereference (for the *_kernel_name queries)."""
    return dummy if ptrs is None else (lambda name: _p(ptrs[name]))


def _dummies(*names) -> dict:
    return {n: (i + 1) << 20 for i, n in enumerate(names)}


def _segs(arr, addrs, chans: Sequence[int], HW: int, accumulate: Sequence[int] = ()):
    """The segment array of a conv3x3 call: batch strides in elements of the segment's own type."""
    for i, (addr, c) in enumerate(zip(addrs, chans)):
        arr[i].ptr, arr[i].batch_stride, arr[i].channels = addr, c * HW, c
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


def conv3x3_wgrad_plan(a: "L.Conv3x3Args") -> "L.WgradPlan":
    """The plan numbers mtbc_conv3x3_wgrad would hand its kernel for `a` (splits, tiles per split, row segments, image ranges, bands, the
    reduction behind it): mtbc_conv3x3_wgrad_plan, host-only (no launch, no device access); raises what the call would."""
    plan = L.WgradPlan()
    L.check(L.load().mtbc_conv3x3_wgrad_plan(C.byref(a), C.byref(plan)), "conv3x3_wgrad_plan")
    return plan


_C3_DUMMY = _dummies(*(f"in{i}" for i in range(L.MAX_SEGS)), "w", "w_packed", "bias", "out", "dout", "dw", "dbias", "workspace", "wgrad_sync",
                     "stats_partial", "out_partial", "norm_z", "norm_mean", "norm_rstd", "norm_gamma", "norm_beta")


def conv3x3_case_args(op: int, N: int, segs: Sequence[int], Cout: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0,
                      c8: bool = False, out_c8: bool = False, out_fp16: bool = False, dx_c8: bool = False, bias: bool = True,
                      in_kernel_reduce: bool = False, accumulate: Optional[Sequence[int]] = None, packed: Optional[bool] = None,
                      force_direct: bool = False, accumulate_dw: bool = False, stats: bool = False, norm: Optional[float] = None,
                      out_partial: bool = False, out_accumulate: bool = False, workspace: bool = True,
                      into: Optional["L.Conv3x3Args"] = None) -> "L.Conv3x3Args":
    """The argument struct of ONE 3x3 convolution call (op = L.OP_CONV3_FWD / _DGRAD / _WGRAD), the only place that fills it: the filler
    engine.StepPlan.conv_cell, _gathered_dgrad and _conv_cell_backward call (through conv3x3_case_op).  ptrs: "in" ->
    the segments (tensors, or C8 tensors) and field name -> tensor / C8 / None for NULL; None = distinct 16-byte aligned dummies that nothing
    may dereference (for conv3x3_kernel_name).  c8: operands in MTBC_LAYOUT_C8 (one segment of at most L.STEM_MAX_CIN channels stays fp32
    planar: the stem, whose weight gradient reads it beside a channel-blocked dout); bias: fwd bias / wgrad dbias; packed: with w_packed
    (default: the dgrad and every forward but the stem's); accumulate: the dgrad's per-segment codes 0 .. 3 (default: the first segment
    overwritten, the others accumulated; dx_c8: all 3 = channel-blocked 16-bit segments).  Forward: out_c8 (+ out_fp16) = a channel-blocked
    16-bit output, stats = the InstanceNorm statistics partials of the epilogue, norm = the slope of the norm-backward epilogue of a gathered
    dgrad (norm_z / _mean / _rstd / _gamma / _beta), out_partial = its planar partial, out_accumulate = the result added to fp32 planes (a
    gathered dgrad into a gradient something else has written).  Weight gradient: accumulate_dw, in_kernel_reduce =
    offer the counters of the in-kernel split-K reduction, workspace = False leaves it without a workspace (the step programs point it at
    their shared one).  into: the (zeroed) struct to fill, a step-program op's union member."""
    lib = L.load()
    ptr = _ptr(ptrs, _C3_DUMMY.__getitem__)
    a = L.Conv3x3Args() if into is None else into
    a.N, a.H, a.W, a.Cin, a.Cout, a.n_in = N, H, W, sum(segs), Cout, len(segs)
    if accumulate is None:
        accumulate = [3 if dx_c8 else int(i > 0) for i in range(len(segs))] if op == L.OP_CONV3_DGRAD else ()
    _segs(a.in_, [ptr(f"in{i}") for i in range(len(segs))] if ptrs is None else [_p(t) for t in ptrs["in"]], segs, H * W, accumulate)
    a.w, a.compute, a.force_direct = ptr("w"), compute, int(force_direct)
    stem = len(segs) == 1 and segs[0] <= L.STEM_MAX_CIN
    if c8 and not (stem and op == L.OP_CONV3_FWD):
        a.operand_layout = L.LAYOUT_C8
    if (op != L.OP_CONV3_WGRAD and not (stem and op == L.OP_CONV3_FWD)) if packed is None else packed:
        a.w_packed = ptr("w_packed")
    if op == L.OP_CONV3_FWD:
        a.out, a.bias, a.out_accumulate = ptr("out"), (ptr("bias") if bias else None), int(out_accumulate)
        if out_c8:
            a.out_layout = L.LAYOUT_C8
            a.out_type = 2 if out_fp16 else 0
        if norm is not None:
            a.norm_z, a.norm_mean, a.norm_rstd, a.norm_slope = ptr("norm_z"), ptr("norm_mean"), ptr("norm_rstd"), norm
            a.norm_gamma, a.norm_beta = ptr("norm_gamma"), ptr("norm_beta")
        if out_partial:
            a.out_partial = ptr("out_partial")
        if stats:
            a.stats_partial = ptr("stats_partial")
    elif op == L.OP_CONV3_DGRAD:
        a.dout = ptr("dout")
    else:
        a.dout, a.dw, a.dbias, a.accumulate_dw = ptr("dout"), ptr("dw"), (ptr("dbias") if bias else None), int(accumulate_dw)
        if workspace:
            nb = int(lib.mtbc_conv3x3_wgrad_workspace(C.byref(a)))
            a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
        nsync = int(lib.mtbc_conv3x3_wgrad_sync_bytes(C.byref(a))) if in_kernel_reduce else 0
        if nsync:
            a.wgrad_sync, a.wgrad_sync_bytes = ptr("wgrad_sync"), (nsync if ptrs is None else ptrs["wgrad_sync"].numel() * 4)
    return a


def conv3x3_case_op(op: int, *shape, tag: int = 0, **mode) -> "L.Op":
    """conv3x3_case_args(op, *shape, **mode) as the step-program op of that kind (+ tag), filled in place."""
    o = _small_op(op, tag)
    conv3x3_case_args(op, *shape, into=o.u.conv3, **mode)
    return o


def conv3x3_case_kernel(op: int, *shape, **mode) -> str:
    """conv3x3_kernel_name of conv3x3_case_args(op, *shape, **mode)."""
    return conv3x3_kernel_name(conv3x3_case_args(op, *shape, **mode), op)


# (op, launches) of every call made through the *_launch functions below while this is a list (the reference tests record what they ran)
launched: Optional[list] = None


def conv3x3_launch(a: "L.Conv3x3Args", op: int) -> None:
    """mtbc_conv3x3_fwd / _dgrad / _wgrad on the current stream for an argument struct of conv3x3_case_args(ptrs=...)."""
    if launched is not None:
        launched.append((op, conv3x3_kernel_name(a, op)))
    lib = L.load()
    fn, what = {L.OP_CONV3_FWD: (lib.mtbc_conv3x3_fwd, "conv3x3_fwd"), L.OP_CONV3_DGRAD: (lib.mtbc_conv3x3_dgrad, "conv3x3_dgrad"),
                L.OP_CONV3_WGRAD: (lib.mtbc_conv3x3_wgrad, "conv3x3_wgrad")}[op]
    L.check(fn(C.byref(a), _s()), what)


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


def _conv_args(xs, w, N, H, W):       # (kept for the tests) a forward over planar xs, no bias, no packed weights, `out` left to the caller
    return conv3x3_case_args(L.OP_CONV3_FWD, N, [x.shape[1] for x in xs], w.shape[0], H, W, ptrs={"in": xs, "w": w, "out": None}, bias=False, packed=False)


def _fill_segs(arr, tensors: Sequence[torch.Tensor], accumulate: Sequence[int] = ()):       # (kept for the tests) planar segments
    _segs(arr, [t.data_ptr() for t in tensors], [t.shape[1] for t in tensors], tensors[0].shape[2] * tensors[0].shape[3], accumulate)


def _conv3x3_fwd(N, segs, Cout, H, W, ptrs: dict, stats: bool = False, **mode):
    """One forward launch; stats: with the epilogue's InstanceNorm statistics partials [N][slots][Cout][2], allocated here and returned."""
    case = lambda **kw: conv3x3_case_args(L.OP_CONV3_FWD, N, segs, Cout, H, W, **mode, **kw)      # noqa: E731
    if stats:
        slots = L.load().mtbc_conv3x3_stats_slots(C.byref(case()))
        if slots <= 0:
            raise L.MtbcError("conv3x3_fwd: no epilogue statistics for this launch")
        ptrs["stats_partial"] = torch.full((N, slots, Cout, 2), float("nan"), dtype=torch.float32, device=ptrs["out"].device)
    conv3x3_launch(case(ptrs=ptrs, stats=stats), L.OP_CONV3_FWD)
    return ptrs.get("stats_partial")


def _conv3x3_dgrad(dz, w, dxs, accumulate, packed, **mode) -> None:
    N, _, H, W = dz.shape
    ptrs = {"in": dxs, "w": w, "w_packed": packed, "dout": dz}
    a = conv3x3_case_args(L.OP_CONV3_DGRAD, N, [d.shape[1] for d in dxs], w.shape[0], H, W, ptrs=ptrs, accumulate=accumulate, packed=packed is not None, **mode)
    conv3x3_launch(a, L.OP_CONV3_DGRAD)


def _conv3x3_wgrad(xs, dz, w_shape, want_bias, dw, accumulate, **mode):
    N, _, H, W = dz.shape
    dev = (dz.data if isinstance(dz, C8) else dz).device
    if dw is None:
        dw = torch.empty(*w_shape, dtype=torch.float32, device=dev)
    db = torch.empty(w_shape[0], dtype=torch.float32, device=dev) if want_bias else None
    case = lambda ptrs: conv3x3_case_args(L.OP_CONV3_WGRAD, N, [x.shape[1] for x in xs], w_shape[0], H, W, ptrs=ptrs, bias=want_bias,      # noqa: E731
                                          accumulate_dw=accumulate, **mode)
    want = case(None)           # (dummy pointers) the workspace and the counters this launch asks for
    ptrs = {"in": xs, "w": None, "dout": dz, "dw": dw, "dbias": db, "workspace": _ws(want.workspace_bytes, dev),
            "wgrad_sync": wgrad_sync_buffer(dev, want.wgrad_sync_bytes) if want.wgrad_sync_bytes else None}
    conv3x3_launch(case(ptrs), L.OP_CONV3_WGRAD)
    return dw, db


def conv3x3_fwd(xs: Sequence[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                packed: Optional[torch.Tensor] = None, force_direct: bool = False, compute: int = 0) -> torch.Tensor:
    _chk(*xs, w, bias)
    N, _, H, W = xs[0].shape
    out = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=w.device)
    _conv3x3_fwd(N, [x.shape[1] for x in xs], w.shape[0], H, W, {"in": xs, "w": w, "w_packed": packed, "bias": bias, "out": out},
                 compute=compute, bias=bias is not None, packed=packed is not None, force_direct=force_direct)
    return out


def conv3x3_stem_fwd_c8(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], compute: int, out_fp16: bool = False, stats: bool = False):
    """The stem conv of the 16-bit modes (1 .. L.STEM_MAX_CIN input channels: the image + intensity channels): fp32 operands, the output
    channel-blocked 16-bit (out_layout = C8 with operand_layout = planar) + optional InstanceNorm statistics partials."""
    _chk(x, w, bias)
    if not 1 <= w.shape[1] <= L.STEM_MAX_CIN or x.shape[1] != w.shape[1]:
        raise ValueError(f"the stem takes 1 .. {L.STEM_MAX_CIN} input channels")
    N, _, H, W = x.shape
    out = torch.empty(N, w.shape[0] // 8, H * W, 8, dtype=torch.int16, device=w.device)
    part = _conv3x3_fwd(N, [x.shape[1]], w.shape[0], H, W, {"in": [x], "w": w, "bias": bias, "out": out}, stats,
                        compute=compute, c8=True, out_c8=True, out_fp16=out_fp16, bias=bias is not None)
    z = C8(out, (N, w.shape[0], H, W), 2 if out_fp16 else compute)
    return (z, part) if stats else z


def conv3x3_dgrad(dz: torch.Tensor, w: torch.Tensor, dxs: Sequence[torch.Tensor], accumulate: Sequence[int] = (),
                  packed: Optional[torch.Tensor] = None, force_direct: bool = False, compute: int = 0) -> None:
    _chk(dz, w, *dxs)
    _conv3x3_dgrad(dz, w, dxs, accumulate, packed, force_direct=force_direct, compute=compute)


def conv3x3_wgrad(xs: Sequence[torch.Tensor], dz: torch.Tensor, w_shape, want_bias: bool = False,
                  force_direct: bool = False, dw: Optional[torch.Tensor] = None, accumulate: bool = False,
                  compute: int = 0):
    _chk(*xs, dz)
    return _conv3x3_wgrad(xs, dz, w_shape, want_bias, dw, accumulate, force_direct=force_direct, compute=compute)


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


def conv3x3_fwd_c8(xs: Sequence["C8"], w: torch.Tensor, bias: Optional[torch.Tensor], packed: torch.Tensor, out_c8: bool = False,
                   stats: bool = False, norm=None, out_partial: Optional[torch.Tensor] = None, out_fp16: bool = False):
    """z = conv3x3(concat(xs)) with the inputs already in the MFMA's 16-bit channel-blocked layout; z comes back as fp32
    planes, or (out_c8, `out_layout = C8` of the C-ABI) as a channel-blocked 16-bit tensor of the inputs' type (out_fp16: bf16 operands,
    the output stored as fp16).  stats: also the InstanceNorm statistics partials of the epilogue.  norm = (z8, mean, rstd, gamma, beta,
    slope) of the output tensor: the gathered dgrad + norm-backward reductions (statistics always), out_partial its planar partial."""
    _chk(w, bias)
    N, _, H, W = xs[0].shape
    Cout, compute = w.shape[0], xs[0].compute
    out = torch.empty((N, Cout // 8, H * W, 8) if out_c8 else (N, Cout, H, W), dtype=torch.int16 if out_c8 else torch.float32, device=w.device)
    ptrs = {"in": xs, "w": w, "w_packed": packed, "bias": bias, "out": out}
    mode = dict(compute=compute, c8=True, out_c8=out_c8, out_fp16=out_fp16, bias=bias is not None, packed=True)
    if norm is not None:
        z8n, mean, rstd, gamma, beta, slope = norm
        _chk(mean, rstd, gamma, beta, out_partial)
        ptrs.update(norm_z=z8n, norm_mean=mean, norm_rstd=rstd, norm_gamma=gamma, norm_beta=beta, out_partial=out_partial)
        mode.update(norm=slope, out_partial=out_partial is not None)
        stats = True
    part = _conv3x3_fwd(N, [x.shape[1] for x in xs], Cout, H, W, ptrs, stats, **mode)
    z = C8(out, (N, Cout, H, W), 2 if out_fp16 else compute) if out_c8 else out
    return (z, part) if stats else z


def conv3x3_dgrad_c8(dz: "C8", w: torch.Tensor, dxs: Sequence[torch.Tensor], accumulate: Sequence[int], packed: torch.Tensor) -> None:
    """dx segments (fp32 planar, accumulate honoured; accumulate 2 = the segment is an int16 (N,C,H,W) tensor written as
    16-bit planar values of dz's type) from dz in the 16-bit channel-blocked layout.  C8 segments (all of them): accumulate = 3."""
    if any(isinstance(d, C8) for d in dxs):
        accumulate = [3] * len(dxs)
    else:
        _chk(w, *[d for i, d in enumerate(dxs) if not (i < len(accumulate) and accumulate[i] == 2)])
    _conv3x3_dgrad(dz, w, dxs, accumulate, packed, compute=dz.compute, c8=True)


_WGRAD_SYNC: dict = {}       # device -> zeroed int32 counters of the in-kernel split-K reduction (every launch leaves them at zero)


def wgrad_sync_buffer(dev, nbytes: int) -> torch.Tensor:
    buf = _WGRAD_SYNC.get(dev)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.zeros(max(4096, (nbytes + 3) // 4), dtype=torch.int32, device=dev)
        _WGRAD_SYNC[dev] = buf
    return buf


def conv3x3_wgrad_c8(xs: Sequence["C8"], dz: "C8", w_shape, want_bias: bool = False, dw: Optional[torch.Tensor] = None,
                     accumulate: bool = False, in_kernel_reduce: bool = True):
    """xs: C8 tensors, or the stem's ONE fp32 planar input of 1 .. L.STEM_MAX_CIN channels (dz channel-blocked either way).
    in_kernel_reduce: the split-K partials are summed inside the launch by the last-arriving block of each group
    (mtbc_conv3x3_args.wgrad_sync); False = the reduction launch behind the kernel (another, equally fixed, summation order)."""
    return _conv3x3_wgrad(xs, dz, w_shape, want_bias, dw, accumulate, compute=dz.compute, c8=True, in_kernel_reduce=in_kernel_reduce)


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
                       dbias: bool = False, acc: bool = False, defer: bool = False, inplace: bool = False, workspace: bool = True,
                       into: Optional["L.InstNormArgs"] = None) -> "L.InstNormArgs":
    """The argument struct of ONE InstanceNorm + LeakyReLU call, the filler engine.StepPlan.conv_cell / _conv_cell_backward call (through
    instnorm_case_op).
    ptrs: field name -> tensor, C8 or None for NULL (dy_extra0 .. dy_extra3 for the fan-in); None = distinct 16-byte aligned dummies that nothing may dereference
    (for instnorm_kernel_name).  compute: 0 = the fp32 kernels of norm.hip, 1 / 2 = out16_type.  out: "f32" planes, "p16" 16-bit planes
    (y16 / dz16), "c8" channel-blocked (y8 / dz8).  z: "f32" planes, "c8" channel-blocked of the output type, "c8f16" / "c8bf16" channel-blocked fp16 / bf16
    under an output of the other type.  Forward: planar / planar16 = fp32 / 16-bit planes beside y8, stats_slots > 0 = statistics from the conv epilogue,
    pool (+ pool_arg) = the pooled output (+ argmax codes), chunk_ws = offer the chunked-statistics workspace.  Backward: dy "f32" / "c8" /
    None, n_extra planar partials, rank1 (+ the head's own gradients, accumulated or not), pool = the routed max-pool gradient, dbias =
    dbias_pre, acc = accumulate_dparams, defer = defer_dparams, inplace = dz over dy (fp32 planes; beside dz8 / dz16 the step programs leave
    dy's address in dz all the same, though no kernel reads it there).  workspace = False leaves either direction without a workspace (the
    step programs point it at their shared one).  into: the (zeroed) struct to fill, a step-program op's union member."""
    dummy = iter(range(1 << 20, 1 << 30, 1 << 20))

    def ptr(name):
        return next(dummy) if ptrs is None else _p(ptrs[name])

    a = L.InstNormArgs() if into is None else into
    a.N, a.C, a.H, a.W, a.eps, a.slope = N, Cc, H, W, eps, slope
    a.z, a.mean, a.rstd = ptr("z"), ptr("mean"), ptr("rstd")
    if affine:
        a.gamma, a.beta = ptr("gamma"), ptr("beta")
    a.coop_reserve_cus = reserve_cus
    if out != "f32":        # (the type of the 16-bit output: read with y8 / y16 / dz8 / dz16 only)
        a.out16_type = compute
    if z != "f32":
        a.z_layout, a.z_type = L.LAYOUT_C8, {"c8": 0, "c8bf16": 1, "c8f16": 2}[z]
    if backward:            # (each direction reads its own stride only)
        a.dy_batch_stride = Cc * H * W
    else:
        a.y_batch_stride = Cc * H * W
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
        nb = L.load().mtbc_instnorm_fwd_workspace(C.byref(a)) if workspace else 0
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
    if inplace:
        a.dz = a.dy
    elif out == "f32":
        a.dz = ptr("dz")
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
    if workspace:
        a.workspace, a.workspace_bytes = ptr("workspace"), (N * (Cc + 1) * 262 * 4 if ptrs is None else ptrs["workspace"].numel() * 4)
    return a


def instnorm_case_op(backward: bool, *shape, tag: int = 0, **mode) -> "L.Op":
    """instnorm_case_args(backward, *shape, **mode) as the MTBC_OP_IN_FWD / _BWD op (+ tag), filled in place."""
    o = _small_op(L.OP_IN_BWD if backward else L.OP_IN_FWD, tag)
    instnorm_case_args(backward, *shape, into=o.u.inorm, **mode)
    return o


def instnorm_case_kernel(backward: bool, *shape, **mode) -> str:
    """instnorm_kernel_name of instnorm_case_args(backward, *shape, **mode)."""
    return instnorm_kernel_name(instnorm_case_args(backward, *shape, **mode), backward)


def instnorm_launch(a: "L.InstNormArgs", backward: bool) -> None:
    """mtbc_instnorm_lrelu_fwd / _bwd on the current stream for an argument struct of instnorm_case_args(ptrs=...)."""
    if launched is not None:
        launched.append((L.OP_IN_BWD if backward else L.OP_IN_FWD, instnorm_kernel_name(a, backward)))
    lib = L.load()
    L.check((lib.mtbc_instnorm_lrelu_bwd if backward else lib.mtbc_instnorm_lrelu_fwd)(C.byref(a), _s()), "instnorm_bwd" if backward else "instnorm_fwd")


def instnorm_dparam_desc(a: "L.InstNormArgs", part: int):
    """The descriptor (an array of one) that reduces the partials a backward call with defer_dparams left at address `part` (= its workspace),
    as the step programs build it (MTBC_OP_IN_DPARAM: engine.StepPlan._conv_cell_backward copies it into the op)."""
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
    ptrs = {"z": z, "gamma": gamma, "beta": beta, "y": y, "y16": y, "mean": mean, "rstd": torch.empty_like(mean)}
    mode = dict(compute=out16, out="p16" if out16 else "f32", affine=gamma is not None or beta is not None, eps=eps, slope=slope)
    nb = instnorm_case_args(False, N, Cc, H, W, **mode).workspace_bytes         # (dummy pointers) the chunked-statistics workspace, if wanted
    if nb:
        ptrs["workspace"] = _ws(nb, z.device)
    instnorm_launch(instnorm_case_args(False, N, Cc, H, W, ptrs=ptrs, **mode), False)
    return y, mean, ptrs["rstd"]


def instnorm_lrelu_bwd(z, dy, mean, rstd, gamma=None, beta=None, eps=1e-5, slope=0.01, inplace=False,
                       dbias_pre=None, dy_extra=(), out16: int = 0):
    _chk(z, dy, mean, rstd, gamma, beta, dbias_pre, *dy_extra)
    N, Cc, H, W = z.shape
    inplace = inplace and not out16
    dz = torch.empty_like(z, dtype=torch.int16) if out16 else (dy if inplace else torch.empty_like(z))
    dg = torch.empty(Cc, dtype=torch.float32, device=z.device) if gamma is not None else None
    db = torch.empty(Cc, dtype=torch.float32, device=z.device) if gamma is not None else None
    ptrs = {"z": z, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "dy": dy, "dz": dz, "dz16": dz, "dgamma": dg, "dbeta": db,
            "dbias_pre": dbias_pre, "workspace": _ws(N * Cc * 12, z.device), **{f"dy_extra{k_}": t_ for k_, t_ in enumerate(dy_extra)}}
    a = instnorm_case_args(True, N, Cc, H, W, ptrs=ptrs, compute=out16, out="p16" if out16 else "f32", affine=gamma is not None or beta is not None, eps=eps, slope=slope,
                           n_extra=len(dy_extra), dbias=dbias_pre is not None, inplace=inplace)
    instnorm_launch(a, True)
    return dz, dg, db


_coop_states = {}


def coop_state(dev) -> torch.Tensor:
    """The persistent, zero-initialised mailbox block of the cooperative InstanceNorm kernels (one per device here;
    the C-ABI wants one per stream that launches them)."""
    key = str(dev)
    if key not in _coop_states:
        _coop_states[key] = torch.zeros(L.load().mtbc_instnorm_coop_state_bytes() // 4, dtype=torch.int32, device=dev)
    return _coop_states[key]


def _z_kind(z, compute: int) -> str:
    """instnorm_case_args' `z` of a wrapper's operand: fp32 planes, or a C8 tensor of the output type `compute` or of the other 16-bit type."""
    if not isinstance(z, C8):
        return "f32"
    return "c8" if z.compute == compute else ("c8f16" if z.compute == 2 else "c8bf16")


def instnorm_lrelu_fwd_c8(z, gamma=None, beta=None, eps=1e-5, slope=0.01, compute: Optional[int] = None, want_planar: bool = False,
                          stats: Optional[torch.Tensor] = None, want_pool: bool = False, planar16: bool = False, reserve_cus: int = 0):
    """InstanceNorm + LeakyReLU straight into the 16-bit channel-blocked layout (y8 of the C-ABI).  z: fp32 planes, or a
    C8 tensor (z_layout = C8: the conv output of the 16-bit modes).  planar16 (with stats): the planar copy is an int16
    (N,C,H,W) tensor of the output type (y16 beside y8).  stats: [N][slots][C][2] from conv3x3_fwd_c8(stats=True).  want_pool: the
    streaming pass also writes the activation's 2x2 max-pool + argmax codes (pool_y8 / pool_arg).  reserve_cus: coop_reserve_cus of the C-ABI."""
    z8 = z if isinstance(z, C8) else None
    if compute is None:         # output type: given, else the type of a channel-blocked z, else bf16
        compute = z8.compute if z8 is not None else 1
    _chk(z if z8 is None else None, gamma, beta)
    N, Cc, H, W = z.shape
    dev = (z8.data if z8 is not None else z).device
    y8 = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=dev)
    y = torch.empty(N, Cc, H, W, dtype=torch.int16 if planar16 else torch.float32, device=dev) if (want_planar or planar16) else None
    mean = torch.empty(N * Cc, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    yp8 = parg = None
    if want_pool:
        yp8 = torch.empty(N, Cc // 8, (H // 2) * (W // 2), 8, dtype=torch.int16, device=dev)
        parg = torch.empty(N, Cc // 8, (H // 2) * (W // 2), dtype=torch.int16, device=dev)
    ptrs = {"z": z, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "y8": y8, "y": y, "y16": y, "coop_state": coop_state(dev),
            "stats_partial": stats, "pool_y8": yp8, "pool_arg": parg}
    a = instnorm_case_args(False, N, Cc, H, W, ptrs=ptrs, compute=compute, out="c8", z=_z_kind(z, compute), affine=gamma is not None or beta is not None,
                           eps=eps, slope=slope, reserve_cus=reserve_cus, stats_slots=stats.shape[1] if stats is not None else 0,
                           planar=y is not None, planar16=planar16, pool=want_pool, chunk_ws=False)
    if not L.load().mtbc_instnorm_c8_supported(C.byref(a), 0):
        raise L.MtbcError("instnorm_fwd: shape not supported with a channel-blocked output")
    instnorm_launch(a, False)
    if want_pool:
        return C8(y8, z.shape, compute), mean, rstd, y, C8(yp8, (N, Cc, H // 2, W // 2), compute), parg
    return C8(y8, z.shape, compute), mean, rstd, y


def instnorm_lrelu_bwd_c8(z, dy, mean, rstd, gamma=None, beta=None, eps=1e-5, slope=0.01, dbias_pre=None, compute: Optional[int] = None,
                          dy_extra: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, rank1=None, rank1_grads: bool = False,
                          pool=None, defer_dparams: bool = False, reserve_cus: int = 0):
    """z / dy: fp32 planes or C8 tensors (z_layout / dy_layout = C8); dy_extra (with a C8 dy only): an fp32 planar partial
    gradient added while loading; rank1 = (dyhead (N,1,H,W), w (C)): the rank-1 gradient term of a one-output 1x1 head (dy may
    then be None), rank1_grads: the head's own weight / bias gradient from the same pass.  pool = (gradient of the 2x2 max-pool of this
    activation (N,C,H/2,W/2) fp32, argmax codes from maxpool2_fwd_c8).  stats: {sum g, sum g * xhat} partials from conv3x3_fwd_c8(norm=...).
    defer_dparams: leave the partials in the workspace, reduce them with the batched entry point afterwards.  reserve_cus:
    coop_reserve_cus of the C-ABI."""
    if compute is None:         # output (and channel-blocked dy) type: given, else dy's, else z's, else bf16
        compute = dy.compute if isinstance(dy, C8) else (z.compute if isinstance(z, C8) else 1)
    _chk(mean, rstd, gamma, beta, dbias_pre, dy_extra, *(rank1 or ()), *(pool[:1] if pool is not None else ()))
    N, Cc, H, W = z.shape
    dev = (z.data if isinstance(z, C8) else z).device
    dz8 = torch.empty(N, Cc // 8, H * W, 8, dtype=torch.int16, device=dev)
    dg = torch.empty(Cc, dtype=torch.float32, device=dev) if gamma is not None else None
    db = torch.empty(Cc, dtype=torch.float32, device=dev) if gamma is not None else None
    hdw = hdb = None
    if rank1_grads:
        hdw, hdb = torch.empty(Cc, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    ws = _ws(N * (Cc + 1) * 262 * 4, dev)
    r1, pl = rank1 or (None, None), pool or (None, None)
    ptrs = {"z": z, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "dy": dy, "dy_extra0": dy_extra, "dz8": dz8, "dgamma": dg, "dbeta": db,
            "dbias_pre": dbias_pre, "coop_state": coop_state(dev), "workspace": ws, "stats_partial": stats, "dy_rank1": r1[0], "dy_rank1_w": r1[1],
            "dy_rank1_dw": hdw, "dy_rank1_db": hdb, "dy_pool": pl[0], "dy_pool_arg": pl[1]}
    a = instnorm_case_args(True, N, Cc, H, W, ptrs=ptrs, compute=compute, out="c8", z=_z_kind(z, compute), affine=gamma is not None or beta is not None,
                           eps=eps, slope=slope, reserve_cus=reserve_cus, stats_slots=stats.shape[1] if stats is not None else 0,
                           dy=None if dy is None else ("c8" if isinstance(dy, C8) else "f32"), n_extra=int(dy_extra is not None),
                           rank1=rank1 is not None or rank1_grads, rank1_grads=rank1_grads, pool=pool is not None, dbias=dbias_pre is not None,
                           defer=defer_dparams)
    if not L.load().mtbc_instnorm_c8_supported(C.byref(a), 1):
        raise L.MtbcError("instnorm_bwd: shape not supported with a channel-blocked output")
    instnorm_launch(a, True)
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
    small_op_launch(maxpool_case_args(L.OP_POOL_FWD, N, Cc, H, W, ptrs={"x": x, "y": y}))
    return y


def maxpool2_bwd(x, dy, dx=None, accumulate=False):
    """x: fp32 planes, or a C8 tensor (dy / dx stay fp32 planes)."""
    _chk(None if isinstance(x, C8) else x, dy, dx)
    N, Cc, H, W = x.shape
    if dx is None:
        dx = torch.empty(N, Cc, H, W, dtype=torch.float32, device=dy.device)
    small_op_launch(maxpool_case_args(L.OP_POOL_BWD, N, Cc, H, W, ptrs={"x": x, "y": None, "dy": dy, "dx": dx},
                                      compute=x.compute if isinstance(x, C8) else 0, acc_dx=accumulate))
    return dx


def maxpool2_fwd_c8(x8: "C8", want_argmax: bool = False):
    """2x2 max-pool of a channel-blocked 16-bit tensor into one (mtbc_maxpool_args.layout = MTBC_LAYOUT_C8); want_argmax: also the
    (N, C/8, H/2*W/2) int16 codes of where each window's maximum sits (mtbc_maxpool_args.argmax)."""
    N, Cc, H, W = x8.shape
    y = torch.empty(N, Cc // 8, (H // 2) * (W // 2), 8, dtype=torch.int16, device=x8.data.device)
    arg = torch.empty(N, Cc // 8, (H // 2) * (W // 2), dtype=torch.int16, device=x8.data.device) if want_argmax else None
    small_op_launch(maxpool_case_args(L.OP_POOL_FWD, N, Cc, H, W, ptrs={"x": x8, "y": y, "argmax": arg}, compute=x8.compute, argmax=want_argmax))
    out = C8(y, (N, Cc, H // 2, W // 2), x8.compute)
    return (out, arg) if want_argmax else out


maxpool2_bwd_c8 = maxpool2_bwd


# ------------------------------------------------------------------ conv transpose (k == stride)
def convT_kernel_name(a: "L.ConvTArgs", op: int, dgrad_next: Optional["L.ConvTArgs"] = None) -> str:
    """Every launch mtbc_convT_fwd / _dgrad / _wgrad -- op = L.OP_CONVT_FWD / _DGRAD / _WGRAD -- would make for `a`, joined with " + ":
    mtbc_convT_kernel_name, host-only (no launch, no device).  dgrad_next (with L.OP_CONVT_WGRAD): the arguments of the OP_CONVT_DGRAD
    right behind it in a program; the name is then what the program runner makes of the pair.  Raises what the call would."""
    buf = C.create_string_buffer(512)
    nxt = None if dgrad_next is None else C.byref(dgrad_next)
    L.check(L.load().mtbc_convT_kernel_name(C.byref(a), op, nxt, buf, len(buf)), "convT_kernel_name")
    return buf.value.decode()


_CT_DUMMY = _dummies("x", "w", "bias", "y", "dy", "dx", "dw", "dbias", "workspace")


def convT_case_args(op: int, N: int, Cin: int, Cout: int, H: int, W: int, k: int = 2, ptrs: Optional[dict] = None, compute: int = 0,
                    dy16: bool = False, x16: bool = False, x_c8: bool = False, y_c8: bool = False, bias: bool = True,
                    acc_dx: bool = False, acc_dw: bool = False, strides: Optional[dict] = None, workspace: bool = True) -> "L.ConvTArgs":
    """The argument struct of ONE transposed-convolution call, the filler engine.StepPlan.convT / convT_head call (through convT_case_op).
    ptrs: field name (x, w, bias, y, dy, dx, dw, dbias, workspace) -> tensor, C8 or None for NULL; None = distinct 16-byte aligned dummies that nothing may
    dereference (for convT_kernel_name), the same address for the same field of every call so that a WGRAD and the DGRAD behind it
    describe one problem.  Forward: x_c8 / y_c8 = 16-bit channel-blocked input / output of type `compute`; bias = with a bias.
    Backward: `compute` = the MFMA operand type, dy16 / x16 = dy / x as 16-bit planes of that type, bias = with dbias (weight gradient),
    acc_dx / acc_dw = accumulate.  strides: field name (x, y, dy, dx) -> batch stride in elements of that tensor where the tensor is a
    channel-range view of a wider buffer; dense otherwise.  workspace = False leaves the weight gradient without one.  Carried where
    ptrs names them, though the call reads neither: bias and y by both gradients, x by the DGRAD."""
    strides, ptr = strides or {}, _ptr(ptrs, _CT_DUMMY.__getitem__)
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
    _carry(a, ptrs, "bias", "y")
    if op == L.OP_CONVT_DGRAD:
        _carry(a, ptrs, "x")
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cin * H * W), int(acc_dx)
        return a
    a.x, a.x_type16 = ptr("x"), (compute if x16 else 0)
    a.dw, a.dbias, a.accumulate_dw = ptr("dw"), (ptr("dbias") if bias else None), int(acc_dw)
    if workspace:
        nb = int(L.load().mtbc_convT_wgrad_workspace(C.byref(a)))
        a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
    return a


def convT_case_op(op: int, *shape, **mode) -> "L.Op":
    """convT_case_args(op, *shape, **mode) as the step-program op of that kind, which is what the fillers of the small ops return."""
    o = _small_op(op)
    o.u.convT = convT_case_args(op, *shape, **mode)
    return o


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


def _convT_fwd(x, w, bias, k, compute: int = 0, y_c8: bool = False) -> torch.Tensor:
    N, Cin, H, W = x.shape
    cout, x_c8 = w.shape[1], isinstance(x, C8)
    y = torch.empty((N, cout // 8, H * k * W * k, 8) if y_c8 else (N, cout, H * k, W * k), dtype=torch.int16 if y_c8 else torch.float32, device=w.device)
    a = convT_case_args(L.OP_CONVT_FWD, N, Cin, cout, H, W, k, ptrs={"x": x, "w": w, "bias": bias, "y": y}, compute=compute, x_c8=x_c8, y_c8=y_c8)
    if y_c8 and not L.load().mtbc_convT_fwd_c8_supported(C.byref(a)):
        raise L.MtbcError("convT_fwd: shape not supported with " + ("channel-blocked input and output" if x_c8 else "a channel-blocked output"))
    convT_launch(a, L.OP_CONVT_FWD)
    return y


def convT_fwd(x, w, bias, k):
    _chk(x, w, bias)
    return _convT_fwd(x, w, bias, k)


def convT_fwd_c8(x, w, bias, k, compute: int) -> "C8":
    """ConvTranspose2d(k = s) forward written straight into the 16-bit channel-blocked layout (y_layout = C8)."""
    _chk(x, w, bias)
    return C8(_convT_fwd(x, w, bias, k, compute, True), (x.shape[0], w.shape[1], x.shape[2] * k, x.shape[3] * k), compute)


def convT_fwd_c8_lp(x8: "C8", w, bias, k) -> "C8":
    """ConvTranspose2d(k = s = 2) forward on the 16-bit MFMA, input and output channel-blocked (x_layout = y_layout = C8)."""
    _chk(w, bias)
    return C8(_convT_fwd(x8, w, bias, k, x8.compute, True), (x8.shape[0], w.shape[1], x8.shape[2] * k, x8.shape[3] * k), x8.compute)


def convT_dgrad(x, w, dy, k, dx=None, accumulate=False, compute=0, dy16=False):
    """dy16: dy is an int16 (N,Cout,kH,kW) tensor holding 16-bit planar values of the type of `compute`.  (x gives the shape of dx only.)"""
    _chk(x, w, None if dy16 else dy, dx)
    if dx is None:
        dx = torch.empty_like(x)
    N, Cin, H, W = x.shape
    convT_launch(convT_case_args(L.OP_CONVT_DGRAD, N, Cin, w.shape[1], H, W, k, ptrs={"w": w, "dy": dy, "dx": dx}, compute=compute, dy16=dy16,
                                 acc_dx=accumulate), L.OP_CONVT_DGRAD)
    return dx


def convT_wgrad(x, w, dy, k, want_bias=True, compute=0, dy16=False, x16=False):
    """x16 (with dy16): x is an int16 (N,Cin,H,W) tensor of 16-bit planar values of the type of `compute` too."""
    _chk(None if x16 else x, w, None if dy16 else dy)
    dw = torch.empty_like(w)
    db = torch.empty(w.shape[1], dtype=torch.float32, device=x.device) if want_bias else None
    N, Cin, H, W = x.shape
    case = lambda ptrs: convT_case_args(L.OP_CONVT_WGRAD, N, Cin, w.shape[1], H, W, k, ptrs=ptrs, compute=compute, dy16=dy16, x16=x16, bias=want_bias)      # noqa: E731
    ptrs = {"x": x, "w": w, "dy": dy, "dw": dw, "dbias": db, "workspace": _ws(case(None).workspace_bytes, x.device)}
    convT_launch(case(ptrs), L.OP_CONVT_WGRAD)
    return dw, db


# ------------------------------------------------------------------ conv1x1
def conv1x1_fwd(x, w, bias):
    """x: fp32 planes, or a C8 tensor (mtbc_conv1x1_args.x_layout = MTBC_LAYOUT_C8)."""
    _chk(None if isinstance(x, C8) else x, w, bias)
    N, Cin, H, W = x.shape
    y = torch.empty(N, w.shape[0], H, W, dtype=torch.float32, device=w.device)
    small_op_launch(conv1x1_case_args(L.OP_CONV1_FWD, N, Cin, w.shape[0], H, W, ptrs={"x": x, "w": w, "bias": bias, "y": y},
                                      compute=x.compute if isinstance(x, C8) else 0))
    return y


conv1x1_fwd_c8 = conv1x1_fwd


def conv1x1_wgrad_c8(x8: "C8", w, dy, accumulate=False, dw=None, db=None):
    _chk(w, dy)
    N, Cin, H, W = x8.shape
    dw = torch.empty_like(w) if dw is None else dw
    db = torch.empty(w.shape[0], dtype=torch.float32, device=w.device) if db is None else db
    case = lambda ptrs: conv1x1_case_args(L.OP_CONV1_WGRAD, N, Cin, w.shape[0], H, W, ptrs=ptrs, compute=x8.compute, acc_dw=accumulate)      # noqa: E731
    ptrs = {"x": x8, "w": w, "dy": dy, "dw": dw, "dbias": db, "workspace": _ws(case(None).u.conv1.workspace_bytes, w.device)}
    small_op_launch(case(ptrs))
    return dw, db


# ------------------------------------------------------------------ losses / optimiser
LOSS_OPS = (L.OP_DICE_FWD, L.OP_DICE_BWD, L.OP_FOCAL, L.OP_LOSS_MIX, L.OP_SOFTMAX)      # op_kernel_name covers these beside SMALL_OPS
_LOSS_DUMMY = _dummies("x0", "x1", "x2", "x3", "dx0", "dx1", "dx2", "dx3", "target", "stats", "loss", "gscale_dev", "x", "weight", "dx")
_SEG_DEFAULTS = {kind: (nr, dr, gamma) for kind, nr, dr, gamma, _ in L.SEG_CRITERIA.values()}


def dice_case_args(kind_op: int, n_heads: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None, seg_kind: int = L.SEG_DICE,
                   weights: Optional[Sequence[float]] = None, smooth: Optional[Tuple[float, float]] = None, focal_gamma: Optional[float] = None,
                   gscale: float = 1.0, gscale_dev: bool = False, into: Optional["L.DiceArgs"] = None):
    """The MTBC_OP_DICE_FWD / _BWD op of ONE segmentation-criterion call, the filler engine.StepPlan.fused_losses calls and the only place that
    fills a mtbc_dice_args.  ptrs: x and dx -> a list of n_heads tensors, target, stats, loss, gscale_dev -> a tensor; None = distinct 16-byte
    aligned dummies that nothing may dereference (for op_kernel_name).  seg_kind: L.SEG_*; weights: the heads' weights (default 1);
    smooth = (nr, dr) and focal_gamma default to the criterion's of L.SEG_CRITERIA (focal_gamma is 0 outside FocalDICE whatever is passed).
    Both ops carry x, the weights, target, stats and loss; only the backward carries dx, gscale and -- with gscale_dev -- the address of the
    device word multiplied into the gradient.  `into`: the struct inside a step-program op, returned instead of a new op."""
    op = None
    if into is None:
        op = _small_op(kind_op)
        into = op.u.dice
    a, nr, dr, gamma = into, *_SEG_DEFAULTS[seg_kind]
    if smooth is not None:
        nr, dr = smooth
    if focal_gamma is not None and seg_kind == L.SEG_FOCALDICE:
        gamma = focal_gamma
    a.n_heads, a.N, a.C, a.H, a.W, a.smooth_nr, a.smooth_dr = n_heads, N, Cc, H, W, nr, dr
    a.kind, a.focal_gamma = seg_kind, gamma

    def ptr(name, i=None):
        if ptrs is None:
            return _LOSS_DUMMY[name if i is None else f"{name}{i}"]
        return _p(ptrs[name] if i is None else ptrs[name][i])

    for i in range(n_heads):
        a.x[i] = ptr("x", i)
        a.head_weight[i] = 1.0 if weights is None else weights[i]
    a.target, a.stats, a.loss = ptr("target"), ptr("stats"), ptr("loss")
    if kind_op == L.OP_DICE_BWD:
        for i in range(n_heads):
            a.dx[i] = ptr("dx", i)
        a.gscale_dev = ptr("gscale_dev") if gscale_dev else None
        a.gscale = gscale
    return a if op is None else op


def focal_case_args(N: int, Cc: int, ptrs: Optional[dict] = None, alpha: float = 1.0, gamma: float = 2.0, weight: bool = False, dx: bool = True,
                    gscale: float = 1.0, gscale_dev: bool = False, into: Optional["L.FocalArgs"] = None):
    """The MTBC_OP_FOCAL op of ONE classification-criterion call, the filler engine.StepPlan._focal_op calls and the only place that fills a
    mtbc_focal_args.  ptrs: x, target, loss and -- where the flag of the same name is set -- weight, dx, gscale_dev -> a tensor; None = dummies.
    `into`: the struct inside a step-program op, returned instead of a new op."""
    op = None
    if into is None:
        op = _small_op(L.OP_FOCAL)
        into = op.u.focal
    a, ptr = into, _ptr(ptrs, _LOSS_DUMMY.__getitem__)
    a.N, a.C, a.alpha, a.gamma = N, Cc, alpha, gamma
    a.x, a.target, a.weight = ptr("x"), ptr("target"), (ptr("weight") if weight else None)
    a.loss, a.dx, a.gscale = ptr("loss"), (ptr("dx") if dx else None), gscale
    a.gscale_dev = ptr("gscale_dev") if gscale_dev else None
    return a if op is None else op


def loss_op_launch(op: "L.Op") -> None:
    """The entry point behind a Dice / Focal / softmax op (of dice_case_args, focal_case_args or an op around softmax_args) on the current
    stream; records (kind, launches) while `launched` is a list."""
    lib = L.load()
    fn = {L.OP_DICE_FWD: lib.mtbc_dice_fwd, L.OP_DICE_BWD: lib.mtbc_dice_bwd, L.OP_FOCAL: lib.mtbc_focal_fwd_bwd, L.OP_SOFTMAX: lib.mtbc_softmax_rows}[op.kind]
    if launched is not None:
        launched.append((op.kind, op_kernel_name(op)))
    L.check(fn(C.byref(getattr(op.u, L.OP_UNION_FIELD[op.kind])), _s()), f"loss op {op.kind}")


def dice_multihead(xs: Sequence[torch.Tensor], target, weights: Sequence[float], gscale: float = 1.0, kind: int = 0,
                   smooth: Optional[Tuple[float, float]] = None, focal_gamma: float = 2.0):
    """returns (loss[n_heads+1], [dx per head]).  kind: L.SEG_DICE (0, the default) | SEG_BCE | SEG_FOCALDICE | SEG_JACCARD; `smooth` = (nr, dr),
    default the reference's for the kind (1 / 1; Jaccard: MONAI's 1e-5 / 1e-5; BCE reads neither)."""
    _chk(*xs, target)
    nh = len(xs)
    N, Cc, H, W = xs[0].shape
    dev = target.device
    stats = torch.empty(nh * N * Cc * L.SEG_STATS_STRIDE[kind], dtype=torch.float32, device=dev)
    loss = torch.empty(nh + 1, dtype=torch.float32, device=dev)
    dxs = [torch.empty_like(x) for x in xs]
    ptrs = {"x": list(xs), "dx": dxs, "target": target, "stats": stats, "loss": loss}
    for kind_op in (L.OP_DICE_FWD, L.OP_DICE_BWD):
        loss_op_launch(dice_case_args(kind_op, nh, N, Cc, H, W, ptrs=ptrs, seg_kind=kind, weights=weights, smooth=smooth, focal_gamma=focal_gamma,
                                      gscale=gscale))
    return loss, dxs


def focal(x, t, alpha=1.0, gamma=2.0, weight=None, gscale=1.0):
    _chk(x, t, weight)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    loss_op_launch(focal_case_args(x.shape[0], x.shape[1], ptrs={"x": x, "target": t, "weight": weight, "loss": loss, "dx": dx}, alpha=alpha,
                                   gamma=gamma, weight=weight is not None, gscale=gscale))
    return loss, dx


def softmax_args(N: int, Cc: int, backward: bool, x=None, p=None, dp=None, dz=None, into: Optional["L.SoftmaxArgs"] = None) -> "L.SoftmaxArgs":
    """mtbc_softmax_args of one call, the only place that fills it: x / p / dp / dz are addresses (device ones for mtbc_softmax_rows and the plan op,
    host ones for mtbc_softmax_rows_host).  `into`: the struct inside a step-program op."""
    a = L.SoftmaxArgs() if into is None else into
    a.N, a.C, a.backward = N, Cc, int(bool(backward))
    a.x, a.p, a.dp, a.dz = x, p, dp, dz
    return a


def softmax_rows(x):
    """softmax over the rows of (N, C <= 3) on the device."""
    _chk(x)
    p = torch.empty_like(x)
    L.check(L.load().mtbc_softmax_rows(C.byref(softmax_args(x.shape[0], x.shape[1], False, x=x.data_ptr(), p=p.data_ptr())), _s()), "softmax_rows")
    return p


def softmax_rows_bwd(p, dp):
    """dz = p * (dp - sum p dp) on the device."""
    _chk(p, dp)
    dz = torch.empty_like(p)
    L.check(L.load().mtbc_softmax_rows(C.byref(softmax_args(p.shape[0], p.shape[1], True, p=p.data_ptr(), dp=dp.data_ptr(), dz=dz.data_ptr())), _s()),
            "softmax_rows_bwd")
    return dz


def softmax_rows_host(x, dp=None):
    """The same row functions compiled for the host, on CPU float32 tensors (no GPU call): p, or with `dp` (p, dz)."""
    x = x.detach().to(torch.float32).contiguous()
    if x.device.type != "cpu" or x.dim() != 2:
        raise ValueError("softmax_rows_host takes a CPU (N, C) tensor")
    p = torch.empty_like(x)
    L.check(L.load().mtbc_softmax_rows_host(C.byref(softmax_args(x.shape[0], x.shape[1], False, x=x.data_ptr(), p=p.data_ptr()))), "softmax_rows_host")
    if dp is None:
        return p
    dp = dp.detach().to(torch.float32).contiguous()
    dz = torch.empty_like(p)
    L.check(L.load().mtbc_softmax_rows_host(C.byref(softmax_args(x.shape[0], x.shape[1], True, p=p.data_ptr(), dp=dp.data_ptr(), dz=dz.data_ptr()))),
            "softmax_rows_host")
    return p, dz


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
    cin, cmid, R = wT.shape[0], wT.shape[1], w1.shape[0]
    dev = x.device
    T = {"wT": wT, "bT": bT, "w1": w1, "b1": b1, "Wc": torch.empty(cin, R, k, k, device=dev), "bc": torch.empty(R, device=dev), "G": None, "gb": None}
    small_op_launch(head_case_args(L.OP_HEAD_COMBINE, cin, cmid, R, k, ptrs=T))
    y = convT_fwd(x, T["Wc"], T["bc"], k)
    dx = convT_dgrad(x, T["Wc"], dout, k)
    T["G"], T["gb"] = convT_wgrad(x, T["Wc"], dout, k)
    T.update(dwT=torch.empty_like(wT), dbT=torch.empty_like(bT), dw1=torch.empty_like(w1), db1=torch.empty_like(b1))
    small_op_launch(head_case_args(L.OP_HEAD_EXPAND, cin, cmid, R, k, ptrs=T))
    return y, dx, T["dwT"], T["dbT"], T["dw1"], T["db1"]


# ------------------------------------------------------------------ the small ops as step-program ops: plan query, argument structs, launch
SMALL_OPS = (L.OP_POOL_FWD, L.OP_POOL_BWD, L.OP_CONV1_FWD, L.OP_CONV1_DGRAD, L.OP_CONV1_WGRAD, L.OP_GAP_FWD, L.OP_GAP_BWD,
             L.OP_LINEAR_FWD, L.OP_LINEAR_BWD, L.OP_HEAD_COMBINE, L.OP_HEAD_EXPAND, L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD)


def op_kernel_name(op: "L.Op") -> str:
    """Every launch the call behind a max-pool, 1x1 convolution, GAP, Linear or fused-head op (SMALL_OPS) or behind a Dice, Focal, loss-mix or
    softmax op (LOSS_OPS) would make, joined with " + ": mtbc_op_kernel_name, host-only (no launch, no device).  Raises what the call would."""
    buf = C.create_string_buffer(512)
    L.check(L.load().mtbc_op_kernel_name(C.byref(op), buf, len(buf)), "op_kernel_name")
    return buf.value.decode()


_SMALL_DUMMY = _dummies("x", "w", "bias", "y", "dy", "dx", "dw", "dbias", "workspace", "argmax", "wT", "bT", "w1", "b1", "Wc", "bc", "G", "gb",
                        "dwT", "dbT", "dw1", "db1")


def _small_ptr(ptrs: Optional[dict]):
    return _ptr(ptrs, _SMALL_DUMMY.__getitem__)


def _small_op(kind: int, tag: int = 0) -> "L.Op":
    """A step-program op of `kind` with an all-zero argument struct (the engine knows it as _mk)."""
    op = L.Op()
    op.kind, op.tag = kind, tag
    return op


def _carry(a, ptrs: Optional[dict], *names) -> None:
    """Fields an op does not read but the step programs carry: set where the caller hands the pointer in, NULL where ptrs has no such key
    (and with the dummies of ptrs = None)."""
    for name in names:
        if ptrs is not None and name in ptrs:
            setattr(a, name, _p(ptrs[name]))


def maxpool_case_args(kind: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, argmax: bool = False,
                      acc_dx: bool = False, strides: Optional[dict] = None) -> "L.Op":
    """The MTBC_OP_POOL_FWD / _BWD op of ONE 2x2 max-pool call, the filler engine.StepPlan.maxpool calls.  ptrs: field name (x, y, dy, dx, argmax) ->
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
    a.y, a.y_batch_stride = ptr("y"), strides.get("y", Cc * H * W // 4)      # both ops carry x and y (the backward reads x alone)
    if kind == L.OP_POOL_FWD:
        a.argmax = ptr("argmax") if argmax else None
    else:
        a.dy, a.dy_batch_stride = ptr("dy"), strides.get("dy", Cc * H * W // 4)
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cc * H * W), int(acc_dx)
    return op


def conv1x1_case_args(kind: int, N: int, Cin: int, Cout: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, bias: bool = True,
                      acc_dx: bool = False, acc_dw: bool = False, strides: Optional[dict] = None, workspace: bool = True) -> "L.Op":
    """The MTBC_OP_CONV1_FWD / _DGRAD / _WGRAD op of ONE 1x1 convolution call, the filler engine.StepPlan.conv1x1 calls.  ptrs: field name (x, w,
    bias, y, dy, dx, dw, dbias, workspace) -> tensor, None = dummies.  compute: 0 = fp32 planar x, 1 / 2 = 16-bit channel-blocked x of that
    type.  bias: forward with a bias / weight gradient with dbias; acc_dx / acc_dw: accumulate.  strides: x, dx -> batch stride of a view
    (y and dy are always dense).  workspace = False leaves the weight gradient without one.  Both gradients carry bias and y where ptrs
    names them, though neither call reads them."""
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
    _carry(a, ptrs, "bias", "y")
    if kind == L.OP_CONV1_DGRAD:
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cin * H * W), int(acc_dx)
        return op
    a.dw, a.dbias, a.accumulate_dw = ptr("dw"), (ptr("dbias") if bias else None), int(acc_dw)
    if workspace:
        nb = int(L.load().mtbc_conv1x1_wgrad_workspace(C.byref(a)))
        a.workspace, a.workspace_bytes = ptr("workspace"), (nb if ptrs is None else ptrs["workspace"].numel() * 4)
    return op


def gap_case_args(kind: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None) -> "L.Op":
    """The MTBC_OP_GAP_FWD / _BWD op, the filler engine.StepPlan.gap calls (x, y / dy, dx; all dense)."""
    ptr = _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.gap
    a.N, a.C, a.H, a.W = N, Cc, H, W
    a.x, a.y = ptr("x"), ptr("y")           # both ops carry x and y (the backward reads neither)
    if kind == L.OP_GAP_BWD:
        a.dy, a.dx = ptr("dy"), ptr("dx")
    return op


def linear_case_args(kind: int, N: int, In: int, Out: int, ptrs: Optional[dict] = None, relu: bool = False, bias: bool = True, dx: bool = True,
                     acc_dw: bool = False, workspace: bool = True) -> "L.Op":
    """The MTBC_OP_LINEAR_FWD / _BWD op, the filler engine.StepPlan.linear calls.  ptrs: x, w, bias, y, dy, dx, dw, dbias, workspace.  bias: the
    forward's bias, which the backward carries beside y (it always has dbias, as in the programs); dx = False: no input gradient; workspace: the call gets what
    mtbc_linear_workspace asks for -- N * Out floats for the backward with relu (the engine gives one to the ReLU layers only), the split
    partials of the batch-shared kernels from In = LINEAR_WIDE_MIN_IN on, nothing otherwise.  ptrs without a "workspace" where one is needed:
    one is allocated here, beside ptrs["x"], and kept alive by the op."""
    ptr = _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.linear
    a.N, a.In, a.Out, a.relu = N, In, Out, int(relu)
    a.x, a.w, a.bias, a.y = ptr("x"), ptr("w"), (ptr("bias") if bias else None), ptr("y")
    if kind == L.OP_LINEAR_BWD:
        a.dy, a.dx = ptr("dy"), (ptr("dx") if dx else None)
        a.dw, a.dbias, a.accumulate_dw = ptr("dw"), ptr("dbias"), int(acc_dw)
    nb = int(L.load().mtbc_linear_workspace(C.byref(a), int(kind == L.OP_LINEAR_BWD)))
    if nb and workspace:
        if ptrs is None:
            a.workspace, a.workspace_bytes = ptr("workspace"), nb
        else:
            if "workspace" not in ptrs:
                op.own_workspace = _ws(nb, ptrs["x"].device)
            ws = ptrs["workspace"] if "workspace" in ptrs else op.own_workspace
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return op


def linear_wide(enabled: bool) -> bool:
    """Process-wide A/B switch of the batch-shared Linear kernels (mtbc_linear_wide_enable); returns what it was.  Off, every Linear call makes
    the per-sample launches it made before those kernels existed.  Plans built while it is off keep their (smaller) workspace: rebuild them."""
    return bool(L.load().mtbc_linear_wide_enable(int(bool(enabled))))


def upsample2_case_args(kind: int, N: int, Cc: int, H: int, W: int, ptrs: Optional[dict] = None, compute: int = 0, acc_dx: bool = False,
                        strides: Optional[dict] = None) -> "L.Op":
    """The MTBC_OP_UPSAMPLE2_FWD / _BWD op of ONE nearest 2x up-sampling call, the filler engine.StepPlan.upsample2 calls (H, W: the INPUT's).  ptrs:
    x, y (forward), dy, dx (backward); None = dummies.  compute: 0 = fp32 planes, 1 / 2 = the forward moves 16-bit channel-blocked tensors of
    that type (dy / dx are fp32 planes always).  strides: field name -> batch stride in elements of that tensor; dense otherwise."""
    strides, ptr = strides or {}, _small_ptr(ptrs)
    op = _small_op(kind)
    a = op.u.up2
    a.N, a.C, a.H, a.W = N, Cc, H, W
    if kind == L.OP_UPSAMPLE2_FWD:
        if compute:
            a.layout, a.type16 = L.LAYOUT_C8, compute
        a.x, a.x_batch_stride = ptr("x"), strides.get("x", Cc * H * W)
        a.y, a.y_batch_stride = ptr("y"), strides.get("y", 4 * Cc * H * W)
    else:
        a.dy, a.dy_batch_stride = ptr("dy"), strides.get("dy", 4 * Cc * H * W)
        a.dx, a.dx_batch_stride, a.accumulate_dx = ptr("dx"), strides.get("dx", Cc * H * W), int(acc_dx)
    return op


def upsample2_fwd(x):
    """nn.Upsample(scale_factor=2, mode="nearest") of fp32 planes (N, C, H, W), or of a C8 tensor into a C8 tensor."""
    N, Cc, H, W = x.shape
    if isinstance(x, C8):
        y = torch.empty(N, Cc // 8, 4 * H * W, 8, dtype=torch.int16, device=x.data.device)
        small_op_launch(upsample2_case_args(L.OP_UPSAMPLE2_FWD, N, Cc, H, W, ptrs={"x": x, "y": y}, compute=x.compute))
        return C8(y, (N, Cc, 2 * H, 2 * W), x.compute)
    _chk(x)
    y = torch.empty(N, Cc, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
    small_op_launch(upsample2_case_args(L.OP_UPSAMPLE2_FWD, N, Cc, H, W, ptrs={"x": x, "y": y}))
    return y


def upsample2_bwd(dy, dx=None, accumulate=False):
    """dx (N, C, H, W) (+)= the 2 x 2 window sums of dy (N, C, 2H, 2W)."""
    _chk(dy, dx)
    N, Cc, H2, W2 = dy.shape
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs the dx to add into")
        dx = torch.empty(N, Cc, H2 // 2, W2 // 2, dtype=torch.float32, device=dy.device)
    small_op_launch(upsample2_case_args(L.OP_UPSAMPLE2_BWD, N, Cc, H2 // 2, W2 // 2, ptrs={"dy": dy, "dx": dx}, acc_dx=accumulate))
    return dx


def head_case_args(kind: int, Cin: int, Cmid: int, R: int, k: int, ptrs: Optional[dict] = None, bT: bool = True, b1: bool = True,
                   dbT: bool = True, db1: bool = True, acc: Sequence[int] = (0, 0, 0, 0)) -> "L.Op":
    """The MTBC_OP_HEAD_COMBINE / _EXPAND op, the filler engine.StepPlan.convT_head calls (every pointer in both ops).  ptrs: wT, bT, w1, b1, Wc, bc,
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
          L.OP_HEAD_COMBINE: lib.mtbc_convT_head_combine, L.OP_HEAD_EXPAND: lib.mtbc_convT_head_expand,
          L.OP_UPSAMPLE2_FWD: lib.mtbc_upsample2_fwd, L.OP_UPSAMPLE2_BWD: lib.mtbc_upsample2_bwd}[op.kind]
    if launched is not None:
        launched.append((op.kind, op_kernel_name(op)))
    L.check(fn(C.byref(getattr(op.u, L.OP_UNION_FIELD[op.kind])), _s()), f"small op {op.kind}")
