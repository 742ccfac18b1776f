#!/usr/bin/env python3
"""What the CLAHE / SOBEL planes cost on one GPU (profiles/spatial_planes_cost.txt).

    python tools/spatial_planes_cost.py bf16 32 256            # dtype, batch, size

Interleaved in one process, four rounds, HIP events:
  assembly   indices -> the filled buffers of a 7-channel step (E = 2 stored planes, K = 4 look-up tables: eight fp32 planes per image with the
             mask), rotated path.  [indexed] one mtbc_batch_assemble_planes launch; [tensors] the tensor-fed route for the same eight planes
             from the package's own functions: a fancy-index gather from an fp32 device-resident copy of the stacked dataset,
             augment.flip_rotate, load_batch.  Beside it the launch alone, back to back, with the bytes it writes per second.
  step       ms per training step of MTUNetPlusPlus with 7, 5 and 1 input channels (the first cell of 7 channels is no stem: direct
             kernels, fp32 conv output), buffers already filled."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import augment as AUG                          # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD                       # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex                # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam                         # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402
from multi_task_breast_cancer_amd.trainer import FusedTrainStep                  # noqa: E402

M = 450                 # curated BUSI
TRANSFORMS = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}
ALL6 = {k: True for k in DD.SPATIAL_KEYS + DD.LUT_KEYS}


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    steps = {}
    for cin in (7, 5, 1):
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=cin, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        steps[cin] = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5)
    parts = [synthetic_batch(50, S, S, seed=s, device=dev, rank=0) for s in range(M // 50)]
    img = torch.cat([p[0] for p in parts]).round()[:, 0].to(torch.uint8).contiguous()
    mask = torch.cat([p[1] for p in parts])[:, 0].to(torch.uint8).contiguous()
    label = torch.cat([p[2] for p in parts]).flatten().long()
    g = torch.Generator(device=dev).manual_seed(7)
    planes = {k: torch.randint(0, 256, img.shape, generator=g, device=dev, dtype=torch.uint8) for k in DD.SPATIAL_KEYS}     # any bytes: the cost does not depend on them
    ds = DD.DeviceDataset(img, mask, label, augmentation=ALL6, spatial_planes=planes)
    luts = torch.from_numpy(DD.intensity_luts({k: True for k in DD.LUT_KEYS}).astype(np.float32)).to(dev)
    # the [tensors] route's fp32 copy: (M, 8, H, W) = mask, image, CLAHE, SOBEL, the four intensity variants
    stack_f = torch.stack([mask.float(), img.float()] + [planes[k].float() for k in DD.SPATIAL_KEYS] + [l[img.long()] for l in luts], dim=1).contiguous()
    label_f = label.float().view(-1, 1)
    tables = DD.EpochTables(EpochIndex(np.arange(M), N, seed=7, drop_last=True), 0, TRANSFORMS)
    nb = len(tables)
    step = steps[7]

    def tensors(i):
        index, params, _, _ = tables.batch(i % nb)
        idx = index.long()
        res = AUG.flip_rotate(stack_f[idx], params)
        step.load_batch(res[:, 1:], res[:, :1], label_f[idx])

    def indexed(i):
        index, params, _, _ = tables.batch(i % nb)
        step.load_indexed(ds, index, params)

    tensors(0), indexed(0)
    print(f"== U-Net++ {dtype}, batch {N}, {S} x {S}, {M} images; all six data.augmentation flags: E = 2 stored planes, K = 4 look-up tables")
    print("-- indices -> filled step buffers, rotated path, us per batch (HIP events around 4 x the epoch's batches)")
    rows = {"tensors": [], "indexed": []}
    for r in range(4):
        for name, fn in (("tensors", tensors), ("indexed", indexed)):
            rows[name].append(events_ms(fn, 4 * nb) * 1e3)
            print(f"round {r + 1} [{name}] {rows[name][-1]:9.1f} us per batch")
    a, b = float(np.mean(rows["tensors"])), float(np.mean(rows["indexed"]))
    print(f"   mean: tensors {a:.1f} us, indexed {b:.1f} us per batch: {a / b:.2f} x")
    st = step._compiled(N, S, S)
    out = (st.x.data, st.mask, st.onehot)
    nbytes = sum(t.numel() * 4 for t in out)
    for name, params in (("rotated path", tables.batch(0)[1]), ("identity path", None)):
        index = tables.batch(0)[0]
        events_ms(lambda i: ds.assemble(index, params, out=out), 5)
        us = events_ms(lambda i: ds.assemble(index, params, out=out), 200) * 1e3
        print(f"mtbc_batch_assemble_planes, {name}: {us:.2f} us per launch (200 back-to-back launches), writes {nbytes} bytes = "
              f"{nbytes / us * 1e-6:.2f} TB/s (copy rate of the chip: 6.3 TB/s)")

    print("-- ms per training step, buffers filled (HIP events around 10 steps)")
    loaded = {}
    for cin, s in steps.items():
        x = torch.rand(N, cin, S, S, device=dev) * 255.0
        b0 = parts[0]
        reps = (N + 49) // 50
        loaded[cin] = s.load_batch(x, b0[1].repeat(reps, 1, 1, 1)[:N], b0[2].repeat(reps, 1)[:N])
        for _ in range(3):
            s.run(loaded[cin])
    rows = {cin: [] for cin in steps}
    for r in range(4):
        for cin, s in steps.items():
            rows[cin].append(events_ms(lambda i: s.run(loaded[cin]), 10))
            print(f"round {r + 1} [{cin} channels] {rows[cin][-1]:8.3f} ms per step")
    m = {cin: float(np.mean(v)) for cin, v in rows.items()}
    print(f"   mean: 7 channels {m[7]:.3f} ms, 5 channels {m[5]:.3f} ms, 1 channel {m[1]:.3f} ms per step: "
          f"7 against 5: {m[7] / m[5]:.3f} x, 7 against 1: {m[7] / m[1]:.3f} x")
    for s in steps.values():
        s.check_nan()


if __name__ == "__main__":
    main()
