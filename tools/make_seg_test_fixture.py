#!/usr/bin/env python3
"""Write tests/golden/seg_test_metrics.npz: the segmentation driver's testing phase (`inference_binary_segmentation`, src/utils/models.py:39-100,
fill_holes=True) on a dozen hand-made 32 x 32 (prediction logits, mask) pairs, by the reference's own metric code.

Runs only where the reference checkout exists (MTBC_REFERENCE, default /root/reference; numpy / scipy / sklearn are all its
`src.utils.metrics` needs).  Per pair, as the driver does: prediction = sigmoid(logits) > .5, scipy.ndimage.binary_fill_holes of it,
`calculate_metrics(mask, filled, patient_id)` on the (H, W) arrays.  The file holds data only -- the logits, the masks, the filled
predictions and the seven numbers per pair -- and nothing of the reference's text.

    python tools/make_seg_test_fixture.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
from scipy.ndimage import binary_fill_holes

REF = os.environ.get("MTBC_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "seg_test_metrics.npz")
sys.path.insert(0, REF)

from src.utils.metrics import calculate_metrics                                                  # noqa: E402

COLUMNS = ["Haussdorf distance", "DICE", "Sensitivity", "Specificity", "Accuracy", "Jaccard index", "Precision"]
S = 32


def box(y0, x0, y1, x1):
    m = np.zeros((S, S), bool)
    m[y0:y1, x0:x1] = True
    return m


def ring(y0, x0, y1, x1):
    return box(y0, x0, y1, x1) & ~box(y0 + 1, x0 + 1, y1 - 1, x1 - 1)


def diamond(c, r):
    """An outline whose consecutive pixels touch only diagonally: closed for the 4-connected background."""
    y, x = np.mgrid[:S, :S]
    return np.abs(y - c) + np.abs(x - c) == r


def pairs():
    z = np.zeros((S, S), bool)
    disc = box(8, 9, 22, 24)
    open_ring = ring(6, 6, 26, 26)
    open_ring[6, 15] = False                      # a gap in the wall: nothing to fill
    speckle = disc ^ (np.random.default_rng(11).random((S, S)) < 0.05)
    return [                                      # (name, ground truth, raw prediction)
        ("ring_with_hole", box(6, 7, 24, 25), ring(6, 7, 24, 25)),
        ("nested_rings", box(3, 3, 29, 29), ring(3, 3, 29, 29) | ring(8, 8, 24, 24) | ring(13, 13, 19, 19)),
        ("ring_on_border", box(0, 0, 14, 32), ring(0, 0, 14, 32)),
        ("empty_prediction", disc, z),
        ("empty_mask", z, ring(10, 10, 20, 20)),
        ("both_empty", z, z),
        ("all_foreground", disc, ~z),
        ("diagonal_ring", diamond(16, 8) | (np.abs(np.mgrid[:S, :S][0] - 16) + np.abs(np.mgrid[:S, :S][1] - 16) < 8), diamond(16, 8)),
        ("open_ring", box(6, 6, 26, 26), open_ring),
        ("speckled_disc", disc, speckle),
        ("two_rings", box(2, 2, 12, 12) | box(18, 16, 30, 30), ring(2, 2, 12, 12) | ring(18, 16, 30, 30)),
        ("hole_touching_border", box(4, 0, 20, 10), ring(4, 0, 20, 10) & ~box(10, 0, 12, 1)),
    ]


def logits_of(pred: np.ndarray) -> np.ndarray:
    """Logits whose sign is the prediction, magnitudes 0.25 .. 2 in a fixed pattern."""
    y, x = np.mgrid[:S, :S]
    mag = 0.25 * (1 + (7 * y + 3 * x) % 8)
    return np.where(pred, mag, -mag).astype(np.float32)


def main() -> None:
    names, logits, masks, filled, rows = [], [], [], [], []
    for name, gt, pred in pairs():
        x = logits_of(pred)
        raw = (1.0 / (1.0 + np.exp(-x.astype(np.float64))) > .5)
        assert np.array_equal(raw, pred), name
        out = binary_fill_holes(raw.astype(np.uint8)).astype(int)                # utils/models.py:84-87
        m = calculate_metrics(gt.astype(np.uint8), out, name)
        names.append(name)
        logits.append(x)
        masks.append(gt.astype(np.uint8))
        filled.append(out.astype(np.uint8))
        rows.append([float(m[c]) for c in COLUMNS])
    np.savez_compressed(OUT, columns=np.array(COLUMNS), names=np.array(names), logits=np.stack(logits), masks=np.stack(masks),
                        filled=np.stack(filled), metrics=np.array(rows, np.float64))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(names)} pairs")
    for n, r, f, p in zip(names, rows, filled, pairs()):
        print(f"  {n:22s} filled {int(f.sum()) - int(p[2].sum()):4d}  " + " ".join(f"{v:.6g}" for v in r))


if __name__ == "__main__":
    main()
