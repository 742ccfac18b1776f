#!/usr/bin/env python3
"""Record tests/golden/adam_steps.npz: what ops.adam_step leaves in p, exp_avg, exp_avg_sq and g, word for word, on the GPU.

    python tools/make_adam_fixture.py [OUT.npz]           # default: tests/golden/adam_steps.npz

The committed file was recorded at commit 10fe25b, the last one at which Adam had a kernel of its own in csrc/head_loss.hip, before
Adam moved onto the shared optimizer launch.  It is the evidence that the shared launch (AdamW, weight_decay 0) writes the words that kernel wrote:
tests/test_fused_optim_cpu.py holds mtbc_optim_step_host to it and tests/test_fused_optim_gpu.py the kernel.  Running this tool at a later commit
records what THAT commit's code computes, not the old kernel: do not regenerate the file to make a failing test pass.

Per size n in SIZES (all tail; tail only past a float4; one float4; body + tail): generator seed 21, p0 and five gradients drawn in that order and
scaled 1e-6, 1e-3, 1, 1e-2, 1e-4; steps t = 1..5 with lr 1e-4, betas (0.9, 0.999), eps 1e-4, grad_scale 0.25, the fifth with zero_grad.  Everything
is stored as the int32 view of the float32 words: n{n}_p0 [n], n{n}_grads [5, n], and n{n}_p / _m / _v / _g [5, n] after each step."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import ops                                     # noqa: E402

SIZES = (1, 3, 4, 1027)
SCALES = (-6, -3, 0, -2, -4)
HYPER = dict(lr=1e-4, eps=1e-4, grad_scale=0.25)


def inputs(n):
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=gen)
    return p0, [torch.randn(n, generator=gen) * 10 ** float(e) for e in SCALES]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "adam_steps.npz")
    dev = torch.device("cuda:0")
    words = lambda x: x.detach().cpu().contiguous().view(torch.int32).numpy().copy()
    rec = {}
    for n in SIZES:
        p0, grads = inputs(n)
        p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        after = {k: [] for k in "pmvg"}
        for t, gr in enumerate(grads, start=1):
            g = gr.to(dev)
            ops.adam_step(p, g, m, v, step=t, zero_grad=(t == len(grads)), **HYPER)
            for k, x in zip("pmvg", (p, m, v, g)):
                after[k].append(words(x))
        rec[f"n{n}_p0"] = words(p0)
        rec[f"n{n}_grads"] = np.stack([words(g) for g in grads])
        for k in "pmvg":
            rec[f"n{n}_{k}"] = np.stack(after[k])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, sizes {SIZES}, {len(SCALES)} steps")


if __name__ == "__main__":
    main()
