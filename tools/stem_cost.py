#!/usr/bin/env python3
"""What the multi-channel stem kernels change for a model that reads intensity channels (profiles/stem_multichannel_cost.txt).

    python tools/stem_cost.py bf16 32 256 3            # dtype, batch, size, input channels (2 .. 5)

Interleaved A/B in one process, four rounds.  A: the plan as it was before the multi-channel stem kernels (engine._NO_STEM_MC, the
MTBC_NO_STEM_MC switch): conv3x3_direct_kernel into an fp32 conv output, the one-plane InstanceNorm, the small-Cin / direct weight
gradient from fp32 dz.  B: conv3x3_stem_mc_fwd_c8_kernel into a 16-bit channel-blocked output + epilogue statistics, the streaming
InstanceNorm, conv3x3_wgrad_stem_mc_c8_kernel from the channel-blocked dz.  Per arm: the first cell's launches alone (conv forward, conv + the
InstanceNorm forward behind it, weight gradient + split-K reduction; HIP events around back-to-back runs of the step's own ops on the
step's own buffers) and ms per step of the whole model."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import _lib as L                               # noqa: E402
from multi_task_breast_cancer_amd import engine, ops                             # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

STEPS, WARMUP, ROUNDS, CALLS = 30, 5, 4, 100
ARMS = (("A: plan before (MTBC_NO_STEM_MC)", True), ("B: multi-channel stem", False))


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def first_cell_ops(st):
    """{label: (program, first op, count, instance name)}: the first conv cell's conv forward alone, with the InstanceNorm forward right behind
    it (which reads what the conv stored), and its weight gradient (+ split-K reduction)."""
    tag = st.plan.cells[0].tag
    fwd, bwd = st.programs["fwd"], st.programs["bwd"]
    i = next(i for i in range(fwd.n) if fwd.array[i].kind == L.OP_CONV3_FWD and fwd.array[i].tag == tag)
    assert fwd.array[i + 1].kind == L.OP_IN_FWD and fwd.array[i + 1].tag == tag
    j = next(j for j in range(bwd.n) if bwd.array[j].kind == L.OP_CONV3_WGRAD and bwd.array[j].tag == tag)
    fname = ops.conv3x3_kernel_name(fwd.array[i].u.conv3, L.OP_CONV3_FWD)
    return {"conv fwd": (fwd, i, 1, fname), "conv + norm fwd": (fwd, i, 2, fname + " + instnorm_lrelu_fwd"),
            "wgrad": (bwd, j, 1, ops.conv3x3_kernel_name(bwd.array[j].u.conv3, L.OP_CONV3_WGRAD))}


def main():
    dtype, N, S, cin = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    dev = torch.device("cuda:0")
    img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    # intensity channels as data.augmentation derives them from the image: brighter, darker, lower and higher contrast
    extra = [(img * 1.3).clamp(0, 255), (img * 0.7).clamp(0, 255), ((img - 128.0) * 0.6 + 128.0).clamp(0, 255), ((img - 128.0) * 1.5 + 128.0).clamp(0, 255)]
    x = torch.cat([img] + extra[:cin - 1], 1).contiguous()
    arms = {}
    for name, old in ARMS:
        engine._NO_STEM_MC = old
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=cin, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        step = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5)
        st = step.load_batch(x, mask, label)
        arms[name] = (step, st)
    engine._NO_STEM_MC = False

    def run(name):
        step, st = arms[name]
        for _ in range(WARMUP):
            step.run(st)
        return events_ms(lambda: step.run(st), STEPS)

    for name in arms:
        run(name)
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}, {cin} input channels: ms per step, HIP events around {STEPS} steps after "
          f"{WARMUP} warm-up, interleaved in one process, {ROUNDS} rounds")
    rows = {name: [] for name in arms}
    for r in range(ROUNDS):
        for name in arms:
            rows[name].append(run(name))
            print(f"round {r + 1} [{name:34s}] {rows[name][-1]:8.3f} ms")
    a, b = (float(np.mean(rows[name])) for name in arms)
    print(f"   mean: A {a:.3f} ms, B {b:.3f} ms ({b - a:+.3f} ms, {100 * (b - a) / a:+.2f} %)")

    print(f"== the first cell's launches alone, us per call (HIP events around {CALLS} back-to-back calls), {ROUNDS} rounds interleaved")
    cells = {name: first_cell_ops(arms[name][1]) for name in arms}
    us = {name: {k: [] for k in cells[name]} for name in arms}
    for r in range(ROUNDS):
        for name in arms:
            for k, (prog, i, n, _) in cells[name].items():
                for _ in range(5):
                    prog.run(i, n)
                us[name][k].append(events_ms(lambda: prog.run(i, n), CALLS) * 1e3)
    for name in arms:
        for k, (_, _, _, inst) in cells[name].items():
            v = us[name][k]
            print(f"[{name:34s}] {k:15s} {np.mean(v):8.2f} us (rounds: {', '.join(f'{t:.2f}' for t in v)})  {inst}")
    cell = arms[ARMS[1][0]][1].plan.cells[0]
    hw = N * S * S
    print(f"   bytes from the shapes: 16-bit forward {hw * (4 * cin + 2 * cell.cout) / 1e6:.1f} MB, forward before {hw * (4 * cin + 4 * cell.cout) / 1e6:.1f} MB "
          f"(+ an fp32 read of z in the norm: {hw * 4 * cell.cout / 1e6:.1f} MB); weight gradient dz {hw * 2 * cell.cout / 1e6:.1f} MB (16-bit) against "
          f"{hw * 4 * cell.cout / 1e6:.1f} MB (fp32), x {hw * 4 * cin / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
