#!/usr/bin/env python3
"""What a classification-only training step costs beside the multi-task step of the same backbone (profiles/cls_only_cost.txt).

    python tools/cls_step_cost.py bf16 64 256            # dtype, batch, size

Two pairs, each interleaved in one process over four rounds: nnUNetClassifier against MTnnUNet and UNetPlusPlusClassifier against
MTUNetPlusPlus (deep supervision on, alpha 0.5), three classes, Focal, fused Adam, eager launches (no graph replay), the batch resident in the
plan's buffers.  ms per step by HIP events on the stream, 10 steps per round after 3 warm-up steps.  Batch and size are the multi-task
model's; the U-Net++ pair runs at half the batch (the benchmark's 32 beside MTnnUNet's 64)."""
import gc
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd.experiment_init import init_classification_model, init_multitask_model, init_optimizer   # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything                                                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch                                                          # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                                                             # noqa: E402

ROUNDS, WARM, REPS = 4, 3, 10


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps          # ms per step


def pair(cls_arch, mt_arch, dtype, N, S, dev):
    img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    seed_everything(1993)
    cl = init_classification_model(cls_arch, sequences=1, n_classes=3).to(dev)
    mt = init_multitask_model(mt_arch, sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
    steps = []
    for model, kw, batch in ((cl, {}, (img, label)), (mt, {"alpha": 0.5, "inversely_weighted": True}, (img, mask, label))):
        model.set_compute(dtype)
        step = FusedTrainStep(model, init_optimizer(model, "Adam", 1e-4), n_classes=3, graph=False, **kw)
        st = step.load_batch(*batch)
        steps.append((step, st))
    runs = [lambda s=s, st=st: s.run(st) for s, st in steps]
    c, m = [], []
    for _ in range(ROUNDS):
        c.append(timed(runs[0], WARM, REPS))
        m.append(timed(runs[1], WARM, REPS))
    for s, _ in steps:
        s.check_nan()
    launches = [sum(st.programs[p].n for p in ("pack", "fwd", "loss", "bwd")) for _, st in steps]
    print(f"-- {cls_arch} against {mt_arch}, {dtype}, batch {N}, {S} x {S}; program ops {launches[0]} against {launches[1]}")
    print(f"   {cls_arch:24s}" + "  ".join(f"{t:8.3f}" for t in c))
    print(f"   {mt_arch:24s}" + "  ".join(f"{t:8.3f}" for t in m))
    print(f"   medians: {np.median(c):.3f} ms against {np.median(m):.3f} ms per step ({np.median(c) / np.median(m):.2f} x)")
    del steps, runs, cl, mt
    gc.collect()
    torch.cuda.empty_cache()


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    print(f"== classification-only step against the multi-task step; ms per step, HIP events, {ROUNDS} interleaved rounds of {REPS} steps after {WARM} warm-up")
    pair("nnUNetClassifier", "MTnnUNet", dtype, N, S, dev)
    pair("UNetPlusPlusClassifier", "MTUNetPlusPlus", dtype, max(1, N // 2), S, dev)


if __name__ == "__main__":
    main()
