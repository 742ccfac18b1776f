#!/usr/bin/env python3
"""What each segmentation criterion of the fused step costs per step on one GPU (profiles/seg_criteria_cost.txt).

    python tools/seg_criteria_cost.py bf16 32 256            # dtype, batch, size

Interleaved in one process, four rounds: FusedTrainStep(seg_criterion="DICE") -- the step as it was, launch for launch -- against the step with
"BCE", "FocalDICE" and "Jaccard", each on a twin model and the same batch, ms per step by HIP events around a run of steps.  Then the two loss
ops alone (mtbc_dice_fwd: statistics + finalize; mtbc_dice_bwd) for every kind on the four heads of that shape: HIP events around back-to-back
calls, with the bytes they move per second beside the chip's 6.3 TB/s copy rate.  The focal term is the one with real arithmetic: five
transcendentals and two divisions per element over 4 x N x H x W elements, in the forward and again in the backward."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import _lib as L                               # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

STEPS, WARMUP, ROUNDS, CALLS = 30, 5, 4, 200
CRITERIA = ("DICE", "BCE", "FocalDICE", "Jaccard")


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
    import ctypes as C
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    arms = {}
    for name in CRITERIA:
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        step = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5, seg_criterion=name)
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
            print(f"round {r + 1} [{name:9s}] {rows[name][-1]:8.3f} ms")
    base = float(np.mean(rows["DICE"]))
    spread = float(np.max(rows["DICE"]) - np.min(rows["DICE"]))
    print(f"   mean: DICE {base:.3f} ms (its own rounds span {spread:.3f} ms)")
    for name in CRITERIA[1:]:
        m = float(np.mean(rows[name]))
        print(f"   mean: {name:9s} {m:.3f} ms ({m - base:+.3f} ms, {100 * (m - base) / base:+.2f} % against DICE)")
    for name, (step, _) in arms.items():
        step.check_nan()

    # the two loss ops alone, four heads of (N, 1, S, S), fp32 logits as the step program hands them over
    g = torch.Generator().manual_seed(0)
    xs = [(torch.randn(N, 1, S, S, generator=g) * 2).to(dev) for _ in range(4)]
    t = (torch.rand(N, 1, S, S, generator=g) > 0.7).float().to(dev)
    dxs = [torch.empty_like(x) for x in xs]
    loss = torch.empty(5, device=dev)
    elems = 4 * N * S * S
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = L.load()
    print(f"== the loss ops alone: 4 heads x {N} x {S} x {S} = {elems} elements, us per call (HIP events around {CALLS} back-to-back calls after 5); "
          f"the Dice forward's budget noted in head_loss.hip was ~40 us before its 16-byte loads")
    for name in CRITERIA:
        kind, nr, dr, gamma, _ = L.SEG_CRITERIA[name]
        stats = torch.empty(4 * N * L.SEG_STATS_STRIDE[kind], device=dev)
        a = L.DiceArgs()
        a.n_heads, a.N, a.C, a.H, a.W, a.smooth_nr, a.smooth_dr, a.kind, a.focal_gamma = 4, N, 1, S, S, nr, dr, kind, gamma
        for i in range(4):
            a.x[i], a.dx[i], a.head_weight[i] = xs[i].data_ptr(), dxs[i].data_ptr(), 1.0 / (4 - i)
        a.target, a.stats, a.loss, a.gscale = t.data_ptr(), stats.data_ptr(), loss.data_ptr(), 0.5

        def fwd():
            L.check(lib.mtbc_dice_fwd(C.byref(a), stream), "dice_fwd")

        def bwd():
            L.check(lib.mtbc_dice_bwd(C.byref(a), stream), "dice_bwd")

        for _ in range(5):
            fwd(); bwd()
        uf, ub = events_ms(fwd, CALLS) * 1e3, events_ms(bwd, CALLS) * 1e3
        bf, bb = 2 * elems * 4, 3 * elems * 4                   # forward reads x and t; backward reads x and t and writes dx
        print(f"   {name:9s} forward {uf:7.2f} us ({bf / uf * 1e-6:5.2f} TB/s)   backward {ub:7.2f} us ({bb / ub * 1e-6:5.2f} TB/s)   "
              f"both {uf + ub:7.2f} us   [copy rate of the chip: 6.3 TB/s]")


if __name__ == "__main__":
    main()
