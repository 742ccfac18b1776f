#!/usr/bin/env python3
"""What the training-time metrics cost per step on one GPU (profiles/train_metrics_cost.txt).

    python tools/train_metrics_cost.py bf16 32 256            # dtype, batch, size
    python tools/train_metrics_cost.py bf16 32 256 graph      # both arms as hipGraph replays (FusedTrainStep(graph=True)): no host issue time in the figure

Interleaved A/B in one process, four rounds: FusedTrainStep(metrics=False) -- the step as it was, launch for launch -- against
FusedTrainStep(metrics=True) on a twin model and the same batch, ms per step by HIP events around a run of steps; then the two launches of
mtbc_train_metrics alone (HIP events around back-to-back calls on the step's own buffers) with the bytes they read per second beside the
chip's 6.3 TB/s copy rate."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

STEPS, WARMUP, ROUNDS, CALLS = 30, 5, 4, 200


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
    graph = len(sys.argv) > 4 and sys.argv[4] == "graph"
    dev = torch.device("cuda:0")
    arms = {}
    for name, metrics in (("metrics=False", False), ("metrics=True", True)):
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        step = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5, metrics=metrics, metrics_capacity=CALLS + 5, graph=graph)
        img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
        st = step.load_batch(img, mask, label)
        arms[name] = (step, st)

    def run(name):
        step, st = arms[name]
        if step.metrics:
            step.begin_epoch_metrics()
        for _ in range(WARMUP):
            step.run(st)
        return events_ms(lambda: step.run(st), STEPS)

    for name in arms:
        run(name)                                                              # the plan, every kernel, the allocator
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}: ms per step, HIP events around {STEPS} steps after {WARMUP} warm-up, "
          f"interleaved in one process, {ROUNDS} rounds; {'hipGraph replay' if graph else 'stream-ordered programs (eager)'}")
    rows = {name: [] for name in arms}
    for r in range(ROUNDS):
        for name in arms:
            rows[name].append(run(name))
            print(f"round {r + 1} [{name:13s}] {rows[name][-1]:8.3f} ms")
    a, b = (float(np.mean(rows[name])) for name in arms)
    print(f"   mean: metrics=False {a:.3f} ms, metrics=True {b:.3f} ms ({b - a:+.3f} ms, {100 * (b - a) / a:+.2f} %); "
          f"for scale: the dynamic loss scale's three launches cost +0.19 % on the bench shape (profiles/dynamic_loss_scale_cost.txt)")
    step, st = arms["metrics=True"]
    m = step.epoch_metrics()
    print(f"   last epoch of the metrics arm: {m.batches} batches, Dice {m.dice:.4f}, accuracy {m.accuracy:.4f}, F1 {m.f1:.4f}")

    step.begin_epoch_metrics()
    for _ in range(5):
        step._append_metrics(st)
    us = events_ms(lambda: step._append_metrics(st), CALLS) * 1e3
    nbytes = 2 * st.mask.numel() * 4
    print(f"mtbc_train_metrics, both launches: {us:.2f} us per call (HIP events around {CALLS} back-to-back calls), reads {nbytes} bytes = "
          f"{nbytes / us * 1e-6:.2f} TB/s (copy rate of the chip: 6.3 TB/s)")
    assert step.epoch_metrics().batches == CALLS + 5


if __name__ == "__main__":
    main()
