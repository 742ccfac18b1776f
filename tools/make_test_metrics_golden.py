#!/usr/bin/env python3
"""Write tests/golden/test_metrics.npz: what the reference's own testing-phase metric code gives on a dozen hand-made mask pairs.

Runs only where the reference checkout exists (MTBC_REFERENCE, default /root/reference; numpy / scipy / sklearn are all its
`src.utils.metrics` needs).  The file holds data only -- packed masks, the numbers `calculate_metrics`,
`postprocess_binary_segmentation`, `multiclass_classification_metrics` and `binary_classification_metrics` returned for them,
and the label vectors -- and nothing of the reference's text.

    python tools/make_test_metrics_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = os.environ.get("MTBC_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "test_metrics.npz")
sys.path.insert(0, REF)

from src.utils.images import postprocess_binary_segmentation                                     # noqa: E402
from src.utils.metrics import (binary_classification_metrics, calculate_metrics,                # noqa: E402
                               multiclass_classification_metrics)

COLUMNS = ["Haussdorf distance", "DICE", "Sensitivity", "Specificity", "Accuracy", "Jaccard index", "Precision"]


def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def ring(H, W, cy, cx, r0, r1):
    y, x = np.mgrid[:H, :W]
    d2 = (y - cy) ** 2 + (x - cx) ** 2
    return (d2 >= r0 * r0) & (d2 <= r1 * r1)


def pairs():
    rng = np.random.default_rng(20240607)
    e64 = ellipse(64, 64, 30, 28, 12, 17)
    z64 = np.zeros((64, 64), bool)
    one_a, one_b = z64.copy(), z64.copy()
    one_a[10, 50] = True
    one_b[40, 7] = True
    e4880 = ellipse(48, 80, 20, 45, 9, 21)
    e256 = ellipse(256, 256, 120, 140, 50, 70)
    return [
        ("ellipse_64", e64, ellipse(64, 64, 31, 30, 11, 15)),
        ("shifted_64", e64, np.roll(e64, 9, axis=1)),
        ("speckle_64", e64, e64 ^ (rng.random((64, 64)) < 0.03)),
        ("both_empty_64", z64, z64),
        ("gt_only_64", e64, z64),
        ("seg_only_64", z64, e64),
        ("full_seg_64", e64, np.ones((64, 64), bool)),
        ("single_pixel_64", one_a, one_b),
        ("ellipse_48x80", e4880, ellipse(48, 80, 22, 41, 10, 18)),
        ("speckle_48x80", e4880, e4880 ^ (rng.random((48, 80)) < 0.02)),
        ("shifted_256", e256, np.roll(np.roll(e256, 9, axis=1), -5, axis=0)),
        ("disc_in_ring_256", ellipse(256, 256, 128, 128, 20, 20), ring(256, 256, 128, 128, 40, 44)),
    ]


def metric_row(gt, seg):
    m = calculate_metrics(gt[None, None].astype(np.float32), seg[None, None].astype(np.float32), "p")
    return [float(m[c]) for c in COLUMNS]


def main() -> None:
    out = {"columns": np.array(COLUMNS)}
    names, shapes, rows = [], [], []
    for i, (name, gt, seg) in enumerate(pairs()):
        names.append(name)
        shapes.append(gt.shape)
        out[f"gt_{i:02d}"] = np.packbits(gt.reshape(-1))
        out[f"seg_{i:02d}"] = np.packbits(seg.reshape(-1))
        rows.append(metric_row(gt, seg))
    out["names"], out["shapes"], out["metrics"] = np.array(names), np.array(shapes, np.int32), np.array(rows, np.float64)

    # threshold_postprocessing around the raw pixel count of two pairs: below / equal / above
    th_pair, th_value, th_cleared, th_rows = [], [], [], []
    for i in (0, 8):
        _, gt, seg = pairs()[i]
        count = int(seg.sum())
        for th in (count - 1, count, count + 1):
            post = postprocess_binary_segmentation(seg[None, None].astype(np.float32), th)
            th_pair.append(i)
            th_value.append(th)
            th_cleared.append(bool(post.sum() == 0))
            th_rows.append(metric_row(gt, post[0, 0] > 0))
    out["threshold_pair"], out["threshold_value"] = np.array(th_pair, np.int32), np.array(th_value, np.int32)
    out["threshold_cleared"], out["threshold_metrics"] = np.array(th_cleared), np.array(th_rows, np.float64)

    # label vectors: mixed / class 2 never predicted / class 1 absent from the ground truth
    rng = np.random.default_rng(7)
    gt_a, pr_a = rng.integers(0, 3, 40), rng.integers(0, 3, 40)
    gt_b, pr_b = rng.integers(0, 3, 30), rng.integers(0, 2, 30)
    gt_c, pr_c = rng.integers(0, 2, 25) * 2, rng.integers(0, 3, 25)
    keys = None
    for tag, gt, pr in (("a", gt_a, pr_a), ("b", gt_b, pr_b), ("c", gt_c, pr_c)):
        m = multiclass_classification_metrics(gt, pr)
        keys = list(m) if keys is None else keys
        out[f"labels_{tag}_gt"], out[f"labels_{tag}_pred"] = gt.astype(np.int64), pr.astype(np.int64)
        out[f"labels_{tag}_values"] = np.array([float(m[k]) for k in keys], np.float64)
    out["multiclass_keys"] = np.array(keys)
    gt_d, pr_d = rng.integers(0, 2, 35), rng.integers(0, 2, 35)
    m = binary_classification_metrics(gt_d, pr_d)
    out["labels_bin_gt"], out["labels_bin_pred"] = gt_d.astype(np.int64), pr_d.astype(np.int64)
    out["binary_keys"], out["labels_bin_values"] = np.array(list(m)), np.array([float(v) for v in m.values()], np.float64)

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(names)} pairs")
    for n, r in zip(names, rows):
        print(f"  {n:18s} " + " ".join(f"{v:.6g}" for v in r))


if __name__ == "__main__":
    main()
