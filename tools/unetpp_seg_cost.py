#!/usr/bin/env python3
"""What a single-task U-Net++ segmentation training step costs beside the multi-task step of the same backbone (profiles/unetpp_seg_cost.txt).

    python tools/unetpp_seg_cost.py bf16 32 256            # dtype, batch, size

Two pairs, each interleaved in one process over four rounds: BasicUnetPlusPlus at MONAI's default widths (32, 32, 64, 128, 256, 32) -- what
`architecture: UnetPlusPlus` builds -- against MTUNetPlusPlus, and BasicUnetPlusPlus at MTUNetPlusPlus's own widths (the same trunk without
the classification head) against it.  Deep supervision on, Dice, fused Adam, eager launches (no graph replay), the batch resident in the
plan's buffers; alpha 1 for the segmentation-only model, 0.5 for the multi-task one.  ms per step by HIP events on the stream, 10 steps per
round after 3 warm-up steps."""
import gc
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import nets                                                                                # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model, init_optimizer, init_segmentation_model        # noqa: E402
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


def pair(label, build_seg, dtype, N, S, dev):
    img, mask, cls = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    seed_everything(1993)
    seg = build_seg().to(dev)
    mt = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
    steps = []
    for model, kw, batch in ((seg, {}, (img, mask)), (mt, {"alpha": 0.5, "n_classes": 3}, (img, mask, cls))):
        model.set_compute(dtype)
        step = FusedTrainStep(model, init_optimizer(model, "Adam", 1e-4), inversely_weighted=True, graph=False, **kw)
        st = step.load_batch(*batch)
        steps.append((step, st))
    runs = [lambda s=s, st=st: s.run(st) for s, st in steps]
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(timed(runs[0], WARM, REPS))
        b.append(timed(runs[1], WARM, REPS))
    for s, _ in steps:
        s.check_nan()
    launches = [sum(st.programs[p].n for p in ("pack", "fwd", "loss", "bwd")) for _, st in steps]
    params = [sum(p.numel() for p in m.parameters()) for m in (seg, mt)]
    print(f"-- {label} against MTUNetPlusPlus, {dtype}, batch {N}, {S} x {S}; program ops {launches[0]} against {launches[1]}; "
          f"parameters {params[0]} against {params[1]}")
    print(f"   {label:40s}" + "  ".join(f"{t:8.3f}" for t in a))
    print(f"   {'MTUNetPlusPlus':40s}" + "  ".join(f"{t:8.3f}" for t in b))
    print(f"   medians: {np.median(a):.3f} ms against {np.median(b):.3f} ms per step ({np.median(a) / np.median(b):.2f} x)")
    del steps, runs, seg, mt
    gc.collect()
    torch.cuda.empty_cache()


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    print(f"== segmentation-only U-Net++ step against the multi-task step; ms per step, HIP events, {ROUNDS} interleaved rounds of {REPS} steps after {WARM} warm-up")
    pair("UnetPlusPlus (32, 32, 64, 128, 256, 32)", lambda: init_segmentation_model("UnetPlusPlus", sequences=1, regions=1, deep_supervision=True),
         dtype, N, S, dev)
    pair("UnetPlusPlus (24, 48, 96, 192, 384, 24)", lambda: nets.BasicUnetPlusPlus(2, 1, 1, nets.UNETPP_FEATURES, True), dtype, N, S, dev)


if __name__ == "__main__":
    main()
