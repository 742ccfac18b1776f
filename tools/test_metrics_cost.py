#!/usr/bin/env python3
"""What the device-side test evaluation costs on one GPU (profiles/test_metrics_cost.txt).

    python tools/test_metrics_cost.py bf16 32 256            # dtype, batch, size
    python tools/test_metrics_cost.py f16 16 512 --kernels   # only 25 seg_metrics calls, to run under rocprofv3 --kernel-trace --stats

Per batch, HIP events, 20 timed calls after 5 warm-up: the `pack` + `fwd` programs of a U-Net++ (deep supervision) in the given
compute mode, the two launches of `seg_metrics` on that forward's outputs, and FusedTestStep as a whole (wall time); beside them the
route without the kernels: predict() -> .cpu() -> the numpy restatement of tests/test_test_metrics_cpu.py (wall time, once)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_task_breast_cancer_amd import inference as I                         # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us per call


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    seed_everything(1993)
    model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
    model.set_compute(dtype)
    img, mask, label = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    st = model.compiled(N, S, S)
    st.x.data.copy_(img)

    def forward():
        st.programs["pack"].run()
        st.programs["fwd"].run()

    forward()
    logits = st.logits.data.view(N, -1)
    # an untrained model predicts noise; the metric kernels are priced on a prediction that looks like a trained one's as well:
    # the mask's own ellipse, shifted by 9 pixels
    shifted = torch.roll(mask, 9, dims=3) * 8.0 - 4.0
    cases = [("model's own logits", st.segs[-1].data), ("mask shifted by 9 px as the prediction", shifted.contiguous())]

    def metrics(x):
        return lambda: I.seg_metrics(x, mask, logits, 0, True, True)

    if "--kernels" in sys.argv:
        for _, x in cases:
            for _ in range(25):
                metrics(x)()
        torch.cuda.synchronize()
        return
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}; us per batch, HIP events, 20 timed calls after 5 warm-up")
    print(f"forward (pack + fwd programs)                              {timed(forward):10.1f} us")
    for name, x in cases:
        raw = (x > 0).flatten(1).sum(dim=1)
        print(f"seg_metrics, both launches [{name}] {timed(metrics(x)):10.1f} us   (predicted pixels per image {int(raw.min())} .. {int(raw.max())})")
    step = I.FusedTestStep(model, 0, True, True)

    def whole():
        step(img, mask, label)
    t = timed(whole)
    step.reset()
    print(f"FusedTestStep per batch (forward + seg_metrics + bookkeeping)  {t:10.1f} us")
    from test_test_metrics_cpu import table_np
    for name, x in cases[1:] + cases[:1]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        forward()
        xs, ms, lg = x.cpu().numpy(), mask.cpu().numpy(), logits.cpu().numpy()
        t1 = time.perf_counter()
        want = table_np(xs, ms, lg, 0, True, True)
        t2 = time.perf_counter()
        got = I.seg_metrics(x, mask, logits, 0, True, True).cpu().numpy()
        diff = sorted({int(n) for n in (got != want).nonzero()[0]})
        print(f"host route [{name}]: forward + .cpu() {1e3 * (t1 - t0):.1f} ms, numpy table {1e3 * (t2 - t1):.1f} ms; equal to the device table: {not diff}")
        for n in diff:          # the restatement's `x > 0` and the kernels' fp32 `sigmoid(x) > .5` part ways only within ~1e-7 of zero
            import numpy as np
            print(f"   image {n}: device {got[n].tolist()} numpy {want[n].tolist()}; smallest |logit| {np.abs(xs[n]).min():.3e}, "
                  f"{int(((xs[n] > 0) & (xs[n] < 1e-6)).sum())} logits in (0, 1e-6)")


if __name__ == "__main__":
    main()
