#!/usr/bin/env python3
"""What each optimizer of the fused step costs per step on one GPU (profiles/optim_cost.txt).

    python tools/optim_cost.py bf16 32 256            # dtype, batch, size

Interleaved in one process, four rounds: FusedTrainStep with FusedAdam -- the step as it was, launch for launch -- against the step with FusedSGD
and FusedAdamW, each on a twin model and the same batch, ms per step by HIP events around a run of steps.  Then the three optimizer launches
alone over that model's flat buffer: HIP events around back-to-back calls, with the bytes they move per second beside the chip's 6.3 TB/s copy
rate.  From bytes alone: Adam and AdamW read p, g, m, v and write p, m, v (28 B per parameter), SGD reads p, g, buf and writes p, buf (20 B)."""
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
from multi_task_breast_cancer_amd.optim import FusedAdam, FusedAdamW, FusedSGD   # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

STEPS, WARMUP, ROUNDS, CALLS = 30, 5, 4, 200
OPTIMIZERS = {"Adam": lambda m: FusedAdam(m, lr=1e-4, eps=1e-4), "SGD": lambda m: FusedSGD(m, lr=1e-4), "AdamW": lambda m: FusedAdamW(m, lr=1e-4)}
BYTES = {"Adam": 28, "SGD": 20, "AdamW": 28}


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    arms = {}
    for name, make in OPTIMIZERS.items():
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        step = FusedTrainStep(model, make(model), alpha=0.5)
        img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
        st = step.load_batch(img, mask, label)
        arms[name] = (step, st)

    def run(name):
        step, st = arms[name]
        for _ in range(WARMUP):
            step.run(st)
        return events_ms(lambda: step.run(st), STEPS)

    for name in arms:
        run(name)                                                              # the plan, every kernel, the allocator
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}: ms per step, HIP events around {STEPS} steps after {WARMUP} warm-up, "
          f"interleaved in one process, {ROUNDS} rounds; stream-ordered programs (eager)")
    rows = {name: [] for name in arms}
    for r in range(ROUNDS):
        for name in arms:
            rows[name].append(run(name))
            print(f"round {r + 1} [{name:5s}] {rows[name][-1]:8.3f} ms")
    base = float(np.mean(rows["Adam"]))
    spread = float(np.max(rows["Adam"]) - np.min(rows["Adam"]))
    print(f"   mean: Adam  {base:.3f} ms (its own rounds span {spread:.3f} ms)")
    for name in ("SGD", "AdamW"):
        m = float(np.mean(rows[name]))
        print(f"   mean: {name:5s} {m:.3f} ms ({m - base:+.3f} ms, {100 * (m - base) / base:+.2f} % against Adam)")
    for name, (step, _) in arms.items():
        step.check_nan()

    # the optimizer launches alone, over buffers of the model's flat size
    n = arms["Adam"][0].model.flat_numel
    g = torch.Generator().manual_seed(0)
    p, gr = torch.randn(n, generator=g).to(dev), (torch.randn(n, generator=g) * 1e-3).to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    calls = {"Adam": lambda: ops.adam_step(p, gr, m, v, lr=1e-4, step=3, eps=1e-4),
             "SGD": lambda: ops.optim_step(L.OPT_SGD, p, gr, m, lr=1e-4, step=3),
             "AdamW": lambda: ops.optim_step(L.OPT_ADAMW, p, gr, m, v, lr=1e-4, step=3, weight_decay=1e-2)}
    print(f"== the optimizer launches alone: {n} parameters, us per call (HIP events around {CALLS} back-to-back calls after 5)")
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        us = events_ms(fn, CALLS) * 1e3
        print(f"   {name:5s} {us:8.2f} us   {BYTES[name]} B per parameter -> {BYTES[name] * n / us * 1e-6:5.2f} TB/s   [copy rate of the chip: 6.3 TB/s]")


if __name__ == "__main__":
    main()
