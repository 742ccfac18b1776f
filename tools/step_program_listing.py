#!/usr/bin/env python
"""Lists whole step programs op by op, host only: kind, tag and every field of the live union member, each pointer written as
(buffer ordinal, byte offset) -- buffer 0 = the flat parameters, 1 = the flat gradients, 2 + i = plan.keep[i] -- so that two builds of the
same plan list the same text whatever the allocator handed out.  Nothing is launched; on --device cpu no GPU is needed.

    python tools/step_program_listing.py [--package DIR] [--set cpu|gpu|cells] [--device cpu|cuda:0] [--short | --summary] [--combos]

--package: the directory of the package to list (default: this tree's); a copy of another commit's package takes this tree's built library
(MTBC_LIB) unless it has its own.  --set cpu: the configurations of tests/golden/step_program_listing.json; gpu: the benchmark's four step
programs and one data-parallel variant; cells: the configurations of tests/golden/conv_cell_listing.json, small plans that reach the branches
of StepPlan.conv_cell and its backward the cpu set does not (several sets: --set cpu --set cells).  --short: JSON {configuration:
{program: ["kind:digest of the canonical fields", ...]}}; --summary: per program the op count and one digest; --combos: the (kind, layout /
flag) combinations of the pool, 1x1, GAP, Linear, ConvT, fused-head, 3x3 convolution and InstanceNorm ops that the set reaches.  A plan on
CPU tensors still depends on whether a device is visible where planes exceed 64 x 64 in the 16-bit
modes (the InstanceNorm team query asks the runtime): the golden holds those configurations from both kinds of machine."""
import argparse
import bisect
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OWN_PACKAGE = os.path.join(os.path.dirname(HERE), "multi_task_breast_cancer_amd")
PROGRAMS = ("pack", "fwd", "loss", "bwd")
FUSED = {"alpha": 0.5, "inversely_weighted": True}


def _cpu_set():
    """(label, class name, constructor arguments, dtype, N, size, fused loss, attributes set on the model, environment)"""
    out = []
    for arch, size in (("MTUNetPlusPlus", 64), ("MTnnUNet", 64), ("Multi_BTSUNet", 128)):
        for dtype in ("f32", "bf16", "f16"):
            for ds in (True, False):
                # MTnnUNet always owns its deep heads (the reference's constructor takes no flag): off = only the last head is trained
                kw, attrs = ({}, {"deep_supervision_outputs": ds}) if arch == "MTnnUNet" else ({"deep_supervision": ds}, {})
                out.append((f"{arch}-{dtype}-{'ds' if ds else 'nods'}-{size}", arch, kw, dtype, 2, size, FUSED, attrs, {}))
    for dtype in ("f32", "bf16"):
        out.append((f"nnUNet-{dtype}-64", "nnUNet", {}, dtype, 2, 64, dict(FUSED, alpha=1.0), {}, {}))
        for arch in ("nnUNetClassifier", "UNetPlusPlusClassifier"):
            out.append((f"{arch}-{dtype}-64", arch, {}, dtype, 2, 64, dict(FUSED, alpha=0.0), {}, {}))
    # 128 x 128: planes of the cooperative InstanceNorm kernels; planned without a device, the one launched channel-blocked pool backward that
    # is the first writer of its dx
    out.append(("MTUNetPlusPlus-bf16-ds-128", "MTUNetPlusPlus", {"deep_supervision": True}, "bf16", 2, 128, FUSED, {}, {}))
    out.append(("MTUNetPlusPlus-bf16-ds-64-noloss", "MTUNetPlusPlus", {"deep_supervision": True}, "bf16", 2, 64, None, {}, {}))
    out.append(("MTnnUNet-bf16-ds-64-nofuse", "MTnnUNet", {}, "bf16", 2, 64, FUSED, {}, {"MTBC_NOFUSE_HEADS": "1"}))
    out.append(("Multi_BTSUNet-bf16-ds-128-nofuse", "Multi_BTSUNet", {"deep_supervision": True}, "bf16", 2, 128, FUSED, {}, {"MTBC_NOFUSE_HEADS": "1"}))
    return out


def _gpu_set():
    shapes = [("MTUNetPlusPlus", "bf16", 32, 256), ("MTUNetPlusPlus", "f16", 16, 512), ("MTnnUNet", "bf16", 64, 256), ("MTUNetPlusPlus", "f32", 32, 256)]
    ctor = {"MTUNetPlusPlus": {"deep_supervision": True}, "MTnnUNet": {}}
    out = [(f"{a}-{d}-{n}x{s}", a, ctor[a], d, n, s, FUSED, {}, {}) for a, d, n, s in shapes]
    out.append(("MTUNetPlusPlus-bf16-32x256-reserve64", "MTUNetPlusPlus", ctor["MTUNetPlusPlus"], "bf16", 32, 256, FUSED, {"coop_reserve_cus": 64}, {}))
    return out


def _cells_set():
    """The cpu set's tuple + the plan switches of engine.py (module attributes, read when a plan is built) that hold for this build."""
    pp = {"deep_supervision": True}
    mc = lambda c, **kw: dict(in_channels=c, out_channels=1, n_classes=3, **kw)         # noqa: E731
    rows = [
        # a first conv of 2 .. 5 channels: fp32, and the multi-channel stem kernels of the 16-bit modes
        ("stem2-f32", "MTUNetPlusPlus*", mc(2), "f32", 64, {}, {}),
        ("stem5-f32", "MTUNetPlusPlus*", mc(5), "f32", 64, {}, {}),
        ("stem3-bf16", "MTUNetPlusPlus*", mc(3, **pp), "bf16", 64, {}, {}),
        ("stem5-f16", "MTnnUNet*", dict(sequences=5, regions=1, n_classes=3), "f16", 64, {}, {}),
        # ... on the launches from before those kernels; Cin = 5: the direct weight gradient
        ("stem3-bf16-nostemmc", "MTUNetPlusPlus*", mc(3, **pp), "bf16", 64, {}, {"_NO_STEM_MC": True}),
        ("stem5-bf16-nostemmc", "MTUNetPlusPlus*", mc(5), "bf16", 64, {}, {"_NO_STEM_MC": True}),
        ("stem5-f32-nostemmc", "MTnnUNet*", dict(sequences=5, regions=1, n_classes=3), "f32", 64, {}, {"_NO_STEM_MC": True}),
        ("direct-f32", "MTUNetPlusPlus*", mc(1, force_direct=True, **pp), "f32", 64, {}, {}),
        # (16-bit modes: only a graph without a transposed convolution can be planned with force_direct)
        ("direct-bf16", "nnUNetClassifier*", dict(sequences=1, n_classes=3, force_direct=True), "bf16", 64, {}, {}),
        ("nocoop-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {}, {"_NO_COOP": True}),
        ("nocoop-f16-128", "MTnnUNet*", dict(sequences=1, regions=1, n_classes=3), "f16", 128, {}, {"_NO_COOP": True}),
        # a plane above 256 x 256 on the one-plane kernels: the channel-blocked dz packed from fp32 planes
        ("nocoop-bf16-512", "MTnnUNet*", dict(sequences=1, regions=1, n_classes=3), "bf16", 512, {}, {"_NO_COOP": True}),
        ("nogather-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {}, {"_NO_GATHER": True}),
        ("noz16-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {}, {"_NO_Z16": True}),
        ("noz16-f16-128", "MTUNetPlusPlus*", mc(1), "f16", 128, {}, {"_NO_Z16": True}),
        ("zbf16-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {}, {"_Z_BF16": True}),
        # 16-bit gathered activation gradients: a channel-blocked dy, and dy_extra where something else wrote the fp32 gradient
        ("da16-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {}, {"_DA16": True}),
        ("da16-f16-nn", "MTnnUNet*", dict(sequences=1, regions=1, n_classes=3), "f16", 64, {}, {"_DA16": True}),
        ("da16-bf16-bts-128", "Multi_BTSUNet", pp, "bf16", 128, {}, {"_DA16": True}),
        # a first cell of 10 channels: channel-blocked operands without the channel-blocked backward, then a conv that is not packed
        ("bts-w20-bf16-128", "Multi_BTSUNet", dict(width=20), "bf16", 128, {}, {}),
        ("reserve64-bf16", "MTUNetPlusPlus*", mc(1, **pp), "bf16", 64, {"coop_reserve_cus": 64}, {}),
        ("reserve64-bf16-128", "MTnnUNet*", dict(sequences=1, regions=1, n_classes=3), "bf16", 128, {"coop_reserve_cus": 64}, {}),
    ]
    # the single-task U-Net++ (MONAI's widths 32 / 32 / 64 / 128 / 256, every conv with a bias), with and without deep supervision
    for dtype in ("f32", "bf16"):
        for ds in (True, False):
            rows.append((f"UnetPlusPlus-{dtype}-{'ds' if ds else 'nods'}", "UnetPlusPlus", {"deep_supervision": ds}, dtype, 64, {}, {}))
    alpha = {"UnetPlusPlus": 1.0, "nnUNetClassifier*": 0.0}          # a segmentation-only and a classification-only model
    return [(label, arch, kw, dtype, 2, size, dict(FUSED, alpha=alpha.get(arch, FUSED["alpha"])), attrs, {}, flags)
            for label, arch, kw, dtype, size, attrs, flags in rows]


SETS = {"cpu": _cpu_set, "gpu": _gpu_set, "cells": _cells_set}
CONSTRUCT = {"MTUNetPlusPlus*": lambda nets, kw: nets.MTUNetPlusPlus(2, **kw), "MTnnUNet*": lambda nets, kw: nets.MTnnUNet(**kw),
             "UnetPlusPlus": lambda nets, kw: nets.BasicUnetPlusPlus(2, **kw), "nnUNetClassifier*": lambda nets, kw: nets.nnUNetClassifier(**kw),
             "MTUNetPlusPlus": lambda nets, kw: nets.MTUNetPlusPlus(2, 1, 1, 3, **kw), "MTnnUNet": lambda nets, kw: nets.MTnnUNet(1, 1, 3),
             "Multi_BTSUNet": lambda nets, kw: nets.Multi_BTSUNet(1, 1, 3, **kw), "nnUNet": lambda nets, kw: nets.nnUNet(1, 1),
             "nnUNetClassifier": lambda nets, kw: nets.nnUNetClassifier(1, 3), "UNetPlusPlusClassifier": lambda nets, kw: nets.UNetPlusPlusClassifier(2, 1, 3)}


def build(nets, config, device):
    """The compiled step of one configuration on zeroed flat buffers: programs and plan, nothing launched."""
    import torch
    label, arch, kw, dtype, N, size, fused, attrs, env, *flags = config
    env = dict({"MTBC_NOFUSE_HEADS": "0"}, **env)          # (the one plan switch read while a graph is built)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    engine = sys.modules[nets.__name__.rsplit(".", 1)[0] + ".engine"]
    flags = flags[0] if flags else {}
    saved_flags = {k: getattr(engine, k) for k in flags}          # (a name the engine does not have is an error)
    for k, v in flags.items():
        setattr(engine, k, v)
    try:
        torch.manual_seed(1993)
        model = CONSTRUCT[arch](nets, kw)
        model.set_compute(dtype)
        for k, v in attrs.items():
            setattr(model, k, v)
        model.flat_p = torch.zeros(model.flat_numel, dtype=torch.float32, device=device)
        model.flat_g = torch.zeros_like(model.flat_p)
        return model, nets.CompiledStep(model, N, size, size, fused_loss=fused)
    finally:
        for k, v in saved_flags.items():
            setattr(engine, k, v)
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


class Canon:
    """Addresses of one compiled step -> (buffer ordinal, byte offset)."""

    def __init__(self, model, step):
        self.spans = []                # (start, end, ordinal), sorted by start
        for i, t in enumerate([model.flat_p, model.flat_g] + list(step.plan.keep)):
            lo = t.data_ptr()
            if t.numel() and self.find(lo) is None:        # (a tensor kept twice, or a view of a buffer kept earlier, resolves through the earlier one)
                bisect.insort(self.spans, (lo, lo + t.numel() * t.element_size(), i))

    def find(self, addr):
        j = bisect.bisect_right(self.spans, (addr, float("inf"), 0)) - 1
        while j >= 0 and self.spans[j][1] <= addr:
            j -= 1
        return self.spans[j] if j >= 0 else None

    def ptr(self, addr):
        if not addr:
            return "0"
        s = self.find(addr)
        if s is None:
            raise ValueError(f"address {addr:#x} lies in no buffer of the plan")
        return f"b{s[2]}+{addr - s[0]}"

    def value(self, typ, v):
        if typ is C.c_void_p:
            return self.ptr(v)
        if isinstance(typ, type) and issubclass(typ, C.Array):
            return "[" + ",".join(self.value(typ._type_, v[i]) for i in range(typ._length_)) + "]"
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            return "{" + self.fields(v) + "}"
        return repr(v)

    def fields(self, struct):
        return " ".join(f"{name}={self.value(typ, getattr(struct, name))}" for name, typ in struct._fields_)


def op_lines(L, canon, program):
    """(kind, canonical text) of every op of a program."""
    out = []
    for i in range(program.n):
        op = program.array[i]
        out.append((op.kind, f"kind={op.kind} tag={op.tag} {canon.fields(getattr(op.u, L.OP_UNION_FIELD[op.kind]))}"))
    return out


def short(lines):
    return [f"{kind}:{hashlib.sha1(text.encode()).hexdigest()[:12]}" for kind, text in lines]


def combos(L, program, name=""):
    """The (kind, layout / flag) combinations of the pool, 1x1, GAP, Linear, ConvT, fused-head, 3x3 convolution and InstanceNorm ops of a
    program (`name`: which of PROGRAMS, listed with the 3x3 convolutions -- a forward-type op of the backward program is a gathered dgrad)."""
    seen = set()
    for i in range(program.n):
        op = program.array[i]
        member = L.OP_UNION_FIELD[op.kind]
        a = getattr(op.u, member)
        if member == "pool":
            f = (f"layout={a.layout}", f"argmax={bool(a.argmax)}", f"acc_dx={a.accumulate_dx}")
        elif member == "conv1":
            f = (f"x_layout={a.x_layout}", f"acc_dx={a.accumulate_dx}", f"acc_dw={a.accumulate_dw}")
        elif member == "convT":
            f = (f"x_layout={a.x_layout}", f"y_layout={a.y_layout}", f"compute={a.compute}", f"dy16={a.dy_type16}", f"x16={a.x_type16}",
                 f"bias={bool(a.bias)}", f"acc_dx={a.accumulate_dx}", f"acc_dw={a.accumulate_dw}")
        elif member == "linear":
            f = (f"relu={a.relu}", f"dx={bool(a.dx)}", f"ws={bool(a.workspace)}", f"acc_dw={a.accumulate_dw}")
        elif member == "head":
            f = (f"acc={a.acc_wT}{a.acc_bT}{a.acc_w1}{a.acc_b1}",)
        elif member == "gap":
            f = ()
        elif member == "inorm":       # (with the pool and the 1x1 head folded into it)
            out = "+".join(n for n in ("y", "y8", "y16", "dz", "dz8", "dz16") if getattr(a, n))
            f = (f"pool_y8={bool(a.pool_y8)}", f"pool_arg={bool(a.pool_arg)}", f"dy_pool={bool(a.dy_pool)}", f"dy_rank1={bool(a.dy_rank1)}",
                 f"z_layout={a.z_layout}", f"z_type={a.z_type}", f"out16={a.out16_type}", f"out={out}", f"stats={a.stats_slots > 0}",
                 f"reserve={a.coop_reserve_cus}", f"affine={bool(a.gamma)}", f"dy={bool(a.dy)}", f"dy_layout={a.dy_layout}",
                 f"n_extra={a.n_dy_extra}", f"dbias={bool(a.dbias_pre)}", f"acc={a.accumulate_dparams}", f"defer={a.defer_dparams}",
                 f"ws={bool(a.workspace)}")
        elif member == "conv3":
            f = (f"in={name}", f"cin={a.Cin}" if a.Cin <= L.STEM_MAX_CIN else "cin>5", f"compute={a.compute}", f"operand_layout={a.operand_layout}",
                 f"out_layout={a.out_layout}", f"out_type={a.out_type}", f"force_direct={a.force_direct}", f"packed={bool(a.w_packed)}",
                 f"bias={bool(a.bias)}", f"stats={bool(a.stats_partial)}", f"out_acc={a.out_accumulate}",
                 "seg_acc=" + "".join(str(c) for c in sorted({a.in_[i].accumulate for i in range(a.n_in)})), f"acc_dw={a.accumulate_dw}")
        else:
            continue
        seen.add((op.kind, member) + f)
    return seen


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package", default=OWN_PACKAGE)
    ap.add_argument("--set", choices=sorted(SETS), action="append")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--short", action="store_true")
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--combos", action="store_true")
    args = ap.parse_args(argv)
    package = os.path.abspath(args.package)
    if not os.path.exists(os.path.join(package, "libmtbc_hip.so")):
        os.environ.setdefault("MTBC_LIB", os.path.join(OWN_PACKAGE, "libmtbc_hip.so"))
    sys.path.insert(0, os.path.dirname(package))
    import importlib
    nets = importlib.import_module(os.path.basename(package) + ".nets")
    L = importlib.import_module(os.path.basename(package) + "._lib")
    result, reached = {}, set()
    for config in [c for name in (args.set or ["cpu"]) for c in SETS[name]()]:
        model, step = build(nets, config, args.device)
        canon = Canon(model, step)
        listing = {name: op_lines(L, canon, step.programs[name]) for name in PROGRAMS}
        for name in PROGRAMS:
            reached |= combos(L, step.programs[name], name)
        if args.short:
            result[config[0]] = {name: short(lines) for name, lines in listing.items()}
        elif args.summary:
            for name, lines in listing.items():
                print(f"{config[0]} {name}: {len(lines)} ops, digest {hashlib.sha1(chr(10).join(t for _, t in lines).encode()).hexdigest()[:16]}")
        elif not args.combos:
            for name, lines in listing.items():
                print(f"== {config[0]} {name}: {len(lines)} ops")
                for i, (_, text) in enumerate(lines):
                    print(f"#{i} {text}")
        del model, step, canon
    if args.short:
        json.dump(result, sys.stdout, indent=0, sort_keys=True)
        print()
    if args.combos:
        for c in sorted(reached):
            print(" ".join(str(v) for v in c))
        print(f"{len(reached)} combinations")


if __name__ == "__main__":
    main()
