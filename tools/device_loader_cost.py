#!/usr/bin/env python3
"""What it costs to go from indices to the step's filled input buffers on one GPU (profiles/device_loader_cost.txt).

    python tools/device_loader_cost.py bf16 32 256            # dtype, batch, size

Interleaved A/B in one process, four rounds, wall time per batch (host clock around a run of batches that ends in a synchronise):
  [tensors]  the route the package had before the device-resident dataset, from its own functions only: a fancy-index gather from an
             fp32 device-resident copy of the dataset, augment.augment_batch (parameters drawn and uploaded per batch), load_batch
  [indexed]  EpochTables once per epoch (timed on its own line), then load_indexed per batch: one mtbc_batch_assemble launch
and the assembly kernel's own time: HIP events around a run of back-to-back launches into the step's buffers, with the bytes it
writes per second beside the chip's 6.3 TB/s copy rate."""
import os
import sys
import time

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


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    dev = torch.device("cuda:0")
    seed_everything(1993)
    model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
    model.set_compute(dtype)
    step = FusedTrainStep(model, FusedAdam(model, lr=1e-4, eps=1e-4), alpha=0.5)
    parts = [synthetic_batch(50, S, S, seed=s, device=dev, rank=0) for s in range(M // 50)]
    img_f = torch.cat([p[0] for p in parts]).round().contiguous()               # the fp32 device-resident copy of the [tensors] route
    mask_f = torch.cat([p[1] for p in parts]).contiguous()
    label_f = torch.cat([p[2] for p in parts]).contiguous()
    ds = DD.DeviceDataset(img_f[:, 0].to(torch.uint8), mask_f[:, 0].to(torch.uint8), label_f.flatten().long())
    ei = EpochIndex(np.arange(M), N, seed=7, drop_last=True)
    nb = len(ei)

    def tensors_epoch(epoch):
        rng = np.random.default_rng(epoch)
        for index in ei.batches(epoch):
            idx = torch.from_numpy(index).to(dev)
            image, mask = AUG.augment_batch(img_f[idx], mask_f[idx], rng)
            step.load_batch(image, mask, label_f[idx])

    def indexed_epoch(epoch, tables=None):
        tables = tables or DD.EpochTables(ei, epoch, TRANSFORMS)
        for b in range(len(tables)):
            index, params, _, _ = tables.batch(b)
            step.load_indexed(ds, index, params)

    def wall(fn, epochs=4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(epochs):
            fn(e)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (epochs * nb) * 1e6

    tensors_epoch(0), indexed_epoch(0)                                           # warm-up: the plan, every kernel, the allocator
    print(f"== U-Net++ {dtype} step buffers, batch {N}, {S} x {S}, {M} images ({nb} batches per epoch, drop_last); "
          f"us per batch from indices to filled buffers, wall time, 4 epochs per figure")
    rows = {"tensors": [], "indexed": []}
    for r in range(4):
        for name, fn in (("tensors", tensors_epoch), ("indexed", indexed_epoch)):
            rows[name].append(wall(fn))
            print(f"round {r + 1} [{name}] {rows[name][-1]:9.1f} us per batch")
    a, b = float(np.mean(rows["tensors"])), float(np.mean(rows["indexed"]))
    print(f"   mean: tensors {a:.1f} us, indexed {b:.1f} us per batch: {a / b:.2f} x")
    t0 = time.perf_counter()
    for e in range(8):
        tables = DD.EpochTables(ei, e, TRANSFORMS)
    torch.cuda.synchronize()
    print(f"   EpochTables (inside the [indexed] figures): {(time.perf_counter() - t0) / 8 * 1e6:.1f} us per epoch = "
          f"{(time.perf_counter() - t0) / 8 / nb * 1e6:.1f} us per batch")
    fixed = lambda e: indexed_epoch(e, tables)                                   # noqa: E731
    print(f"   [indexed] with the epoch's tables already built: {wall(fixed):.1f} us per batch")

    st = step._compiled(N, S, S)
    out = (st.x.data, st.mask, st.onehot)
    nbytes = sum(t.numel() * 4 for t in out)
    for label, params in (("rotated path", tables.batch(0)[1]), ("identity path", None)):
        index = tables.batch(0)[0]
        for _ in range(5):
            ds.assemble(index, params, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 200
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            ds.assemble(index, params, out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        print(f"mtbc_batch_assemble, {label}: {us:.2f} us per launch (HIP events around {reps} back-to-back launches), writes {nbytes} bytes = "
              f"{nbytes / us * 1e-6:.2f} TB/s (copy rate of the chip: 6.3 TB/s)")


if __name__ == "__main__":
    main()
