#!/usr/bin/env python3
"""What the device-side testing phase of the segmentation driver costs on one GPU (profiles/fill_holes_cost.txt).

    python tools/fill_holes_cost.py bf16 32 256            # dtype, batch, size

Per batch: the `pack` + `fwd` programs of an nnUNet in the given compute mode, then the two routes of the testing phase
(`inference_binary_segmentation`, fill_holes=True) on that forward's last head:
  device   `mtbc_fill_holes` + `mtbc_seg_metrics` on the filled mask, nothing read back (inference.FusedSegTestStep.evaluate_logits)
  host     the route it replaces: read the logits back, scipy.ndimage.binary_fill_holes per image
The two are interleaved in one process over four rounds, each timed by HIP events on the stream (the host route's events bracket its
copy and its scipy loop, so they measure its wall time), 10 calls per round after 3 warm-up calls.  An untrained model predicts noise,
so both routes are also priced on a prediction that looks like a trained model's: the mask's own ellipse as a ring 3 pixels thick."""
import os
import sys

import numpy as np
import torch
from scipy.ndimage import binary_fill_holes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import inference as I                           # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_segmentation_model   # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything                # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch                 # noqa: E402

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
    return a.elapsed_time(b) / reps * 1e3          # us per call


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    seed_everything(1993)
    model = init_segmentation_model("nnUNet", sequences=1, regions=1).to(dev)
    model.set_compute(dtype)
    img, mask, _ = synthetic_batch(N, S, S, seed=0, device=dev, rank=0)
    st = model.compiled(N, S, S)
    st.x.data.copy_(img)

    def forward():
        st.programs["pack"].run()
        st.programs["fwd"].run()

    forward()
    eroded = mask * torch.roll(mask, 3, 2) * torch.roll(mask, -3, 2) * torch.roll(mask, 3, 3) * torch.roll(mask, -3, 3)
    ring = ((mask - eroded) * 8.0 - 4.0).contiguous()
    cases = [("model's own logits", st.segs[-1].data), ("the mask's outline, 3 px, as the prediction", ring)]
    step = I.FusedSegTestStep(model)

    def device(x):
        def run():
            step.evaluate_logits(x, mask)
            step._tables.clear(), step._ids.clear(), step._classes.clear()
        return run

    def host(x):
        def run():
            raw = (torch.sigmoid(x) > .5).cpu().numpy()
            return [binary_fill_holes(m[0]) for m in raw]
        return run

    print(f"== nnUNet {dtype}, batch {N}, {S} x {S}; us per batch, HIP events, {ROUNDS} interleaved rounds of {REPS} calls after {WARM} warm-up")
    fwd = [timed(forward, WARM, REPS) for _ in range(ROUNDS)]
    print(f"forward (pack + fwd programs)                 " + "  ".join(f"{t:10.1f}" for t in fwd))
    for name, x in cases:
        filled = np.stack(host(x)())
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        got = I.fill_holes(x, err, want_logits=False, want_u8=True)[1].cpu().numpy() != 0
        raw = (torch.sigmoid(x) > .5).flatten(1).sum(dim=1)
        print(f"-- {name}: predicted pixels per image {int(raw.min())} .. {int(raw.max())}, filled {int(filled.sum() - raw.sum())} in the batch; "
              f"device == scipy: {bool(np.array_equal(got, filled))}, error word {int(err.item())}")
        d, h = [], []
        for _ in range(ROUNDS):
            d.append(timed(device(x), WARM, REPS))
            h.append(timed(host(x), 1, REPS))
        print("   device: fill_holes + seg_metrics             " + "  ".join(f"{t:10.1f}" for t in d))
        print("   host:   logits -> .cpu() -> scipy per image  " + "  ".join(f"{t:10.1f}" for t in h))
        print(f"   medians: device {np.median(d):.1f} us, host {np.median(h):.1f} us, forward {np.median(fwd):.1f} us")


if __name__ == "__main__":
    main()
