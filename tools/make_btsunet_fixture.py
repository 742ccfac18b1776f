#!/usr/bin/env python3
"""Writes tests/golden/mt_btsunet_step.npz from the REFERENCE's own Multi_BTS_UNet, FocalLoss and
apply_criterion_multitask_segmentation_classification (needs a checkout of the reference; only the numbers it produces are committed).

usage: tools/make_btsunet_fixture.py /path/to/reference

For each configuration of tests/bts_oracle.py CONFIGS (width 8 / 3 classes / deep supervision: 4-channel tensors, the non-channel-blocked
routes; width 16 / 2 classes / no deep supervision: every channel count a multiple of 8), under the reference's seed_everything(1993):
  sha        sha256 of the initial state_dict (bts_oracle.state_sha256) -- no weights are stored (18 - 38 MB)
  keys       the state_dict's names, in order
  logits     float64 (2, n_logits)
  head{i}    float64 values of head i (deep supervision: output3, output2, output1) at the flat positions bts_oracle.sample_index gives
  head{i}_sum  float64 sum of the whole head per sample
  losses     float64 [total, seg, cls], total = 0.35 seg + 0.65 cls; Dice = oracle.torch_oracle.dice_loss_sigmoid_sq (MONAI is not pinned here),
             classes: the reference's FocalLoss (3 classes) / torch's BCEWithLogitsLoss (2), heads weighted 1 / (j + 1) from the last one
  grad.{name}      float64 gradient of the tensors of bts_oracle.GRAD_TENSORS (sampled the same way when large)
  grad_ref32.{name}  the reference float32 run's own relative distance to those float64 values, over the recorded positions
  logits_ref32, head_ref32, loss_ref32   the float32 run's largest absolute distance to the float64 logits / heads (whole) / loss words
The batch (shared by both configurations): image uint8 (2, 1, 128, 128) raw 0..255 values, mask uint8, label (2,) in {0, 1, 2} (the binary
configuration's target is label == 1)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    from src.models.multitask.Multi_BTS_UNet import Multi_BTS_UNet
    from src.utils.criterions import FocalLoss, apply_criterion_multitask_segmentation_classification
    from src.utils.miscellany import seed_everything
    import bts_oracle as B
    from oracle import torch_oracle as O

    torch.set_num_threads(8)
    img, mask, label = O.synthetic_batch(2, 128, 128, seed=5)
    img = img.round().clamp(0, 255)
    mask = (mask + torch.roll(mask, 1, 0)).clamp(0, 1)      # the generator leaves a "normal" sample's mask empty: every Dice plane carries a lesion here
    assert bool((mask.sum(dim=(1, 2, 3)) > 0).all())
    label = torch.tensor([1, 2])           # one target on each side of the binary head
    out = dict(image=img.to(torch.uint8).numpy(), mask=mask.to(torch.uint8).numpy(), label=label.numpy().astype(np.int64))
    for name, (width, n_classes, ds) in B.CONFIGS.items():
        seed_everything(1993)
        m32 = Multi_BTS_UNet(1, 1, n_classes, width, ds)
        sd = m32.state_dict()
        out[f"{name}.sha"] = np.array(B.state_sha256(sd))
        out[f"{name}.keys"] = np.array(list(sd))
        runs = {}
        for dt in (torch.float32, torch.float64):
            m = Multi_BTS_UNet(1, 1, n_classes, width, ds).to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in sd.items()})
            cls_out, seg_out = m(img.to(dt))
            if n_classes == 2:
                crit, target = torch.nn.BCEWithLogitsLoss(), (label == 1).to(dt).view(-1, 1)
            else:
                crit, target = FocalLoss(), torch.nn.functional.one_hot(label, n_classes).to(dt)
            seg, cls = apply_criterion_multitask_segmentation_classification(O.dice_loss_sigmoid_sq, mask.to(dt), seg_out, crit, target, cls_out,
                                                                              inversely_weighted=True)
            total = B.ALPHA * seg + (1 - B.ALPHA) * cls
            total.backward()
            heads = seg_out if isinstance(seg_out, list) else [seg_out]
            logits = cls_out[0] if isinstance(cls_out, list) else cls_out
            runs[dt] = (logits.detach().double(), [h.detach().double() for h in heads], torch.stack([total, seg, cls]).detach().double(),
                        {k: p.grad.detach().double() for k, p in m.named_parameters()})
        l32, h32, w32, g32 = runs[torch.float32]
        l64, h64, w64, g64 = runs[torch.float64]
        out[f"{name}.logits"] = l64.numpy()
        out[f"{name}.logits_ref32"] = np.array((l32 - l64).abs().max().item())
        out[f"{name}.losses"] = w64.numpy()
        out[f"{name}.loss_ref32"] = np.array((w32 - w64).abs().max().item())
        out[f"{name}.head_ref32"] = np.array(max((a - b).abs().max().item() for a, b in zip(h32, h64)))
        for i, h in enumerate(h64):
            idx = B.sample_index(h.numel(), 100 + i)
            out[f"{name}.head{i}"] = h.reshape(-1)[idx].numpy()
            out[f"{name}.head{i}_sum"] = h.sum(dim=(1, 2, 3)).numpy()
        for j, k in enumerate(B.GRAD_TENSORS):
            idx = B.sample_index(g64[k].numel(), 200 + j)
            a, b = g32[k].reshape(-1)[idx], g64[k].reshape(-1)[idx]
            out[f"{name}.grad.{k}"] = b.numpy()
            out[f"{name}.grad_ref32.{k}"] = np.array(((a - b).norm() / b.norm()).item())
        print(name, "keys", len(sd), "losses", w64.tolist(), "ref32: logits %.2e heads %.2e loss %.2e" %
              (out[f"{name}.logits_ref32"], out[f"{name}.head_ref32"], out[f"{name}.loss_ref32"]),
              {k.split(".")[0]: float(out[f"{name}.grad_ref32.{k}"]) for k in B.GRAD_TENSORS})
    path = os.path.join(ROOT, "tests", "golden", "mt_btsunet_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
