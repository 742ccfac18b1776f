#!/usr/bin/env python3
"""What Multi_BTSUNet's two new ops cost in its training step (profiles/mt_btsunet_cost.txt).

    python tools/btsunet_cost.py bf16 16            # dtype (f32 | bf16 | f16), batch

The model at width 24 with deep supervision on 128 x 128 inputs, FusedTrainStep with FusedAdam.  Interleaved in one process, four rounds,
HIP events:
  * ms per step, A: the per-sample Linear kernels (ops.linear_wide(False), the launches before the batch-shared kernels existed) against
    B: the batch-shared ones -- the same compiled plan, the switch thrown between the runs;
  * the three up-sampling launches of the forward and of the backward program alone, with the bytes they move (from the shapes) per second;
  * the first Linear's forward and backward (mask + dx + dW) alone in both arms, with W's bytes (4 In Out) per second for the forward.
A launch timed back to back re-reads what the previous call left in the chip's last-level cache (W is 50 MB here, the cache 256 MB): these
are rates of the launches, not of HBM; the step times are the end-to-end figure."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import _lib as L                               # noqa: E402
from multi_task_breast_cancer_amd import ops                                     # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

STEPS, WARMUP, ROUNDS, CALLS = 30, 5, 4, 50
ARMS = (("A: per-sample Linear", False), ("B: batch-shared Linear", True))


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def find(prog, kind):
    return [i for i in range(prog.n) if prog.array[i].kind == kind]


def up_bytes(op, backward):
    a = op.u.up2
    n = a.N * a.C * a.H * a.W
    if backward:
        return n * (16 + 4 + (4 if a.accumulate_dx else 0))
    return n * 5 * (2 if a.layout == L.LAYOUT_C8 else 4)


def main():
    dtype, N = sys.argv[1], int(sys.argv[2])
    dev = torch.device("cuda:0")
    img, mask, label = synthetic_batch(N, 128, 128, seed=0, device=dev, rank=0)
    seed_everything(1993)
    model = init_multitask_model("Multi_BTSUNet", sequences=1, regions=1, n_classes=3, width=24, deep_supervision=True).to(dev)
    model.set_compute(dtype)
    step = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.35)
    st = step.load_batch(img, mask, label)          # planned with the batch-shared kernels on: its workspace covers both arms
    fwd, bwd = st.programs["fwd"], st.programs["bwd"]

    def run_steps(wide):
        ops.linear_wide(wide)
        for _ in range(WARMUP):
            step.run(st)
        return events_ms(lambda: step.run(st), STEPS)

    print(f"== Multi_BTSUNet width 24, deep supervision, {dtype}, batch {N}, 128 x 128: ms per step, HIP events around {STEPS} steps after {WARMUP} "
          f"warm-up, interleaved in one process, {ROUNDS} rounds")
    for _, wide in ARMS:
        run_steps(wide)
    rows = {name: [] for name, _ in ARMS}
    for r in range(ROUNDS):
        for name, wide in ARMS:
            rows[name].append(run_steps(wide))
            print(f"round {r + 1} [{name:24s}] {rows[name][-1]:8.3f} ms")
    a, b = (float(np.mean(rows[name])) for name, _ in ARMS)
    print(f"   mean: A {a:.3f} ms, B {b:.3f} ms ({b - a:+.3f} ms, {100 * (b - a) / a:+.2f} %)")
    step.check_nan()

    print(f"== the up-sampling launches alone, us per call (HIP events around {CALLS} back-to-back calls), mean of {ROUNDS} rounds")
    for prog, kind, back in ((fwd, L.OP_UPSAMPLE2_FWD, False), (bwd, L.OP_UPSAMPLE2_BWD, True)):
        for i in find(prog, kind):
            op = prog.array[i]
            for _ in range(5):
                prog.run(i, 1)
            us = float(np.mean([events_ms(lambda: prog.run(i, 1), CALLS) * 1e3 for _ in range(ROUNDS)]))
            u = op.u.up2
            nb = up_bytes(op, back)
            print(f"   {ops.op_kernel_name(op):28s} ({u.N}, {u.C}, {u.H}, {u.W}){' accumulate' if back and u.accumulate_dx else ''}: {us:8.2f} us, "
                  f"{nb / 1e6:7.2f} MB -> {nb / us / 1e6:6.2f} TB/s")

    i = find(fwd, L.OP_LINEAR_FWD)[0]
    j = find(bwd, L.OP_LINEAR_BWD)[-1]            # the backward program runs the layers in reverse: the first Linear's op is the last
    lin = fwd.array[i].u.linear
    assert bwd.array[j].u.linear.In == lin.In
    wbytes = 4 * lin.In * lin.Out
    print(f"== the first Linear alone (N {lin.N}, In {lin.In}, Out {lin.Out}; W {wbytes / 1e6:.1f} MB), us per call (HIP events around {CALLS} back-to-back "
          f"calls), {ROUNDS} rounds interleaved")
    us = {(name, k): [] for name, _ in ARMS for k in ("forward", "backward")}
    names = {}
    for r in range(ROUNDS):
        for name, wide in ARMS:
            ops.linear_wide(wide)
            for k, prog, idx in (("forward", fwd, i), ("backward", bwd, j)):
                names[(name, k)] = ops.op_kernel_name(prog.array[idx])
                for _ in range(3):
                    prog.run(idx, 1)
                us[(name, k)].append(events_ms(lambda: prog.run(idx, 1), CALLS) * 1e3)
    ops.linear_wide(True)
    for (name, k), v in us.items():
        m = float(np.mean(v))
        reads = 1 if name.startswith("B") else lin.N
        note = f"W read {reads} x: {reads * wbytes / m / 1e6:6.2f} TB/s" if k == "forward" else "mask + dx + dW"
        print(f"   [{name:24s}] {k:8s} {m:9.2f} us (rounds: {', '.join(f'{t:.2f}' for t in v)})  {note}  {names[(name, k)]}")
    print(f"   bytes from the shapes: forward and dx each read W once per launch in B ({wbytes / 1e6:.1f} MB) and once per sample in A "
          f"({lin.N * wbytes / 1e6:.1f} MB); dW writes W once in both")


if __name__ == "__main__":
    main()
