#!/usr/bin/env python3
"""What a validation batch costs on one GPU, default path against the device-side path (profiles/eval_step_cost.txt).

    python tools/eval_cost.py bf16 32 256            # dtype, batch, size
    python tools/eval_cost.py fp32 2 128             # the reference configuration's own batch: bound by launch and issue time

Interleaved in one process, four rounds, three arms on ONE model and the same batch: FusedEvalStep() -- the default path, launch for launch
what it was, the yardstick --, FusedEvalStep(on_device=True) eager and FusedEvalStep(on_device=True, graph=True).  Per arm and round: ms per
batch by HIP events around a run of batches (the input fills included: they are the same in every arm), and beside it the HOST issue time per
batch -- a host clock around the same loop, stopped BEFORE the synchronise: what the CPU spends enqueuing a batch, the figure a latency-bound
shape lives on.  Then the two launches of mtbc_eval_metrics alone, HIP events around back-to-back calls on the step's own buffers.  Every arm
is warmed up first (plans, kernels, the allocator, the captured graph); needs a GPU (no fallback)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import _lib as L                               # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedEvalStep                   # noqa: E402

BATCHES, WARMUP, ROUNDS, CALLS = 50, 5, 4, 200


def timed(fn, reps):
    """(ms per call by HIP events, host ms per call spent issuing)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, host * 1e3 / reps


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    L.require_gpu()
    dev = torch.device("cuda:0")
    seed_everything(1993)
    model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
    model.set_compute(dtype)
    img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    cap = max(BATCHES + WARMUP, CALLS + 5)
    arms = {"default": FusedEvalStep(model, alpha=0.5),
            "on_device": FusedEvalStep(model, alpha=0.5, on_device=True, graph=False, capacity=cap),
            "on_device+graph": FusedEvalStep(model, alpha=0.5, on_device=True, graph=True, capacity=cap)}

    def run(name):
        step = arms[name]
        step.reset()
        for _ in range(WARMUP):
            step(img, mask, label)
        return timed(lambda: step(img, mask, label), BATCHES)

    for name in arms:
        run(name)                                                              # the plan, every kernel, the allocator, the capture
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}: ms per validation batch (HIP events around {BATCHES} batches after {WARMUP} "
          f"warm-up) | host issue ms per batch (host clock around the same loop, before the synchronise); interleaved in one process, {ROUNDS} rounds")
    rows = {name: [] for name in arms}
    for r in range(ROUNDS):
        for name in arms:
            rows[name].append(run(name))
            print(f"round {r + 1} [{name:15s}] {rows[name][-1][0]:8.3f} ms | issue {rows[name][-1][1]:7.3f} ms")
    mean = {name: np.mean(np.array(v), axis=0) for name, v in rows.items()}
    base = mean["default"]
    for name in arms:
        m = mean[name]
        print(f"   mean [{name:15s}] {m[0]:8.3f} ms ({100 * (m[0] - base[0]) / base[0]:+6.2f} % against default) | issue {m[1]:7.3f} ms "
              f"({100 * (m[1] - base[1]) / base[1]:+6.2f} %)")
    res = {name: step.result() for name, step in arms.items()}
    print("   six numbers of the last round: " + "; ".join(f"{name} loss {v[0]:.6f} dice {v[1]:.4f}" for name, v in res.items()))
    assert res["on_device"] == res["on_device+graph"] and res["default"][0] == res["on_device"][0]

    step = arms["on_device"]
    st = step._compiled(N, S, S)
    step.reset()
    for _ in range(5):
        step._append_eval(st)
    us = timed(lambda: step._append_eval(st), CALLS)[0] * 1e3
    nbytes = 2 * st.mask.numel() * 4
    print(f"mtbc_eval_metrics, both launches: {us:.2f} us per call (HIP events around {CALLS} back-to-back calls), reads {nbytes} bytes = "
          f"{nbytes / us * 1e-6:.2f} TB/s (copy rate of the chip: 6.3 TB/s)")
    assert step._em_state.cpu().tolist() == [CALLS + 5, 0]


if __name__ == "__main__":
    main()
