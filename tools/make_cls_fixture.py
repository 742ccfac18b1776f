#!/usr/bin/env python3
"""Write tests/golden/cls_nnunet_step.npz: the single-task classification baseline (`nnUNetClassifier`, src/models/classification/
nnUNet_classifier.py) under the reference's own code, on one seed-fixed 2 x 1 x 64 x 64 batch.

Runs only where the reference checkout exists (MTBC_REFERENCE, default /root/reference): it imports the reference's `nnUNetClassifier`,
`FocalLoss` and `apply_criterion_classification` (torch only) and stores what they compute -- data, nothing of the reference's text:

    names, shapes            the state dict's keys and shapes (n_classes 3)
    sha256_init_3 / _2       sha256 of the initial state dict under seed 1993, n_classes 3 and 2
    image, label, seed       the batch: oracle.torch_oracle.synthetic_batch(2, 64, 64, seed) at the first seed 0, 1, 2, ... that gives two different
                             labels and at which the reference's own float32 gradients (below) are within 2e-6 of its float64 gradients
    out_3, out_2             what the model returns: probabilities (3 classes), the raw logit (binary head)
    loss_focal, loss_ce      FocalLoss(alpha 1, gamma 2) and CrossEntropyLoss on out_3 against the one-hot label
    loss_bce                 BCEWithLogitsLoss on out_2 against the {0, 1} label (label > 0)
    step_loss, grad_*        one verbatim driver step (training_classification.py:41-58) with Focal and Adam(lr 1e-4, eps 1e-4): the loss and
                             the gradients of classifier.5.weight, classifier.5.bias and encoder1.ConvInNormLRelu1.Conv.weight
    grad_none                the names of the parameters whose .grad is None after that step
    grad64_*                 the same three gradients from the same model and batch in float64 (the model cast with .double()): what the float32
                             gradients above are an approximation of

64 x 64 is the smallest input at which the bottleneck's InstanceNorm still has more than one element per plane.  With 2 x 2 planes there, how
well float32 torch reproduces the first layer's gradient depends on the draw: over seeds 0 .. 11 its distance from the float64 gradient of the
same model runs from 2e-7 to 5e-4 (|g| about 3e-2 throughout).  A stored float32 gradient that is itself further from the true gradient than the
bound the tests hold against it (2e-5) measures torch's rounding, not the code under test, so the batch is chosen by the reference's own
error, a tenth of that bound: nothing of this project's arithmetic enters the choice.

    python tools/make_cls_fixture.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MTBC_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cls_nnunet_step.npz")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from src.models.classification.nnUNet_classifier import nnUNetClassifier                         # noqa: E402
from src.utils.criterions import FocalLoss, apply_criterion_classification                       # noqa: E402

from multi_task_breast_cancer_amd.miscellany import seed_everything                               # noqa: E402
from oracle.torch_oracle import synthetic_batch                                                   # noqa: E402

GRADS = ("classifier.5.weight", "classifier.5.bias", "encoder1.ConvInNormLRelu1.Conv.weight")
OWN_ERROR = 2e-6        # the reference's float32 gradients against its float64 gradients: a tenth of the bound the tests hold against the former


def sha(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def own_error(image, label) -> float:
    """max |float32 - float64| over the three gradients, both from the reference's model and criterion at the seed-1993 initial weights."""
    onehot = torch.nn.functional.one_hot(label.flatten().to(torch.int64), num_classes=3).to(torch.float)
    grads = []
    for dtype in (torch.float32, torch.float64):
        seed_everything(1993)
        model = nnUNetClassifier(sequences=1, n_classes=3).to(dtype)
        model.train(True)
        FocalLoss(alpha=1, gamma=2, reduction="mean")(model(image.to(dtype)), onehot.to(dtype)).backward()
        params = dict(model.named_parameters())
        grads.append([params[n].grad.double() for n in GRADS])
    return max((a - b).abs().max().item() for a, b in zip(*grads))


def choose_batch():
    for seed in range(64):
        image, _, label = synthetic_batch(2, 64, 64, seed=seed)
        if label[0].item() == label[1].item():
            continue
        err = own_error(image, label)
        print(f"seed {seed}: labels {label.flatten().tolist()}, the reference's float32 against its float64 gradients {err:.3e}")
        if err < OWN_ERROR:
            return seed, image, label
    raise SystemExit("no batch found")


def main() -> None:
    torch.set_num_threads(1)
    seed, image, label = choose_batch()
    out = {"image": image.numpy(), "label": label.numpy(), "seed": np.array(seed)}

    seed_everything(1993)
    model = nnUNetClassifier(sequences=1, n_classes=3)
    sd = model.state_dict()
    out["names"] = np.array(list(sd))
    out["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    out["sha256_init_3"] = np.array(sha(sd))

    onehot = torch.nn.functional.one_hot(label.flatten().to(torch.int64), num_classes=3).to(torch.float)
    model.train(True)
    with torch.no_grad():
        probs = model(image)
        out["out_3"] = probs.numpy()
        out["loss_focal"] = np.array(FocalLoss(alpha=1, gamma=2, reduction="mean")(probs, onehot).item(), dtype=np.float64)
        out["loss_ce"] = np.array(torch.nn.CrossEntropyLoss(reduction="mean")(probs, onehot).item(), dtype=np.float64)

    # one verbatim driver step (training_classification.py:41-58)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-4, eps=1e-4)
    classification_criterion = FocalLoss(alpha=1, gamma=2, reduction="mean")
    optimizer.zero_grad(set_to_none=True)
    pred_class = model(image)
    classification_loss = apply_criterion_classification(classification_criterion, onehot, pred_class, True)
    classification_loss.backward()
    optimizer.step()
    out["step_loss"] = np.array(classification_loss.item(), dtype=np.float64)
    params = dict(model.named_parameters())
    for name in GRADS:
        out["grad_" + name] = params[name].grad.numpy().copy()
    out["grad_none"] = np.array([n for n, p in params.items() if p.grad is None])

    seed_everything(1993)
    model64 = nnUNetClassifier(sequences=1, n_classes=3).double()
    model64.train(True)
    FocalLoss(alpha=1, gamma=2, reduction="mean")(model64(image.double()), onehot.double()).backward()
    params64 = dict(model64.named_parameters())
    for name in GRADS:
        out["grad64_" + name] = params64[name].grad.numpy().copy()
        print(f"{name}: max |float32 - float64| gradient {np.abs(out['grad_' + name] - out['grad64_' + name]).max():.3e}")

    seed_everything(1993)
    binary = nnUNetClassifier(sequences=1, n_classes=2)
    out["sha256_init_2"] = np.array(sha(binary.state_dict()))
    binary.train(True)
    with torch.no_grad():
        logit = binary(image)
        out["out_2"] = logit.numpy()
        out["loss_bce"] = np.array(torch.nn.BCEWithLogitsLoss()(logit, (label > 0).to(torch.float)).item(), dtype=np.float64)

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; grad is None for {len(out['grad_none'])} parameters")


if __name__ == "__main__":
    main()
