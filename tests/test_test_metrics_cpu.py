"""Testing-phase tables without a GPU: the host half of `inference` (metrics_from_table, classification_report, the CSV writer)
against what the reference's own metric code recorded in tests/golden/test_metrics.npz (tools/make_test_metrics_golden.py), the
numpy restatement of the device table that tests/test_test_metrics_gpu.py compares the kernels with, pinned here first, and the
C-ABI of mtbc_seg_metrics."""
import csv
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L            # noqa: E402
from multi_task_breast_cancer_amd import inference as I       # noqa: E402

NORMAL = 2


# ------------------------------------------------------------------------------------------------
# numpy restatement of the device table (the GPU tests import it from here)
# ------------------------------------------------------------------------------------------------
def hd_rows_sq_np(a: np.ndarray, b: np.ndarray) -> int:
    """Square of scipy's directed_hausdorff on two (H, W) boolean images, both directions: rows are points, the squared
    distance of two rows is their Hamming distance (XOR + sum, here as two exact float32 matrix products)."""
    if not a.any() and not b.any():
        return 0
    if a.any() != b.any():
        return -1
    af, bf = a.astype(np.float32), b.astype(np.float32)
    ham = af @ (1 - bf).T + (1 - af) @ bf.T                  # (H, H): ham[i, j] = sum_x a[i, x] != b[j, x]
    return int(max(ham.min(axis=1).max(), ham.min(axis=0).max()))


def _directed_px_sq(a: np.ndarray, b: np.ndarray) -> int:
    """max over the pixels of a of the squared distance to the nearest pixel of b: column scan, then a row minimum."""
    H, W = a.shape
    INF = 1 << 20
    g = np.full((H, W), INF, np.int64)                       # vertical distance to the nearest b pixel of the column
    run = np.full(W, INF, np.int64)
    for y in range(H):
        run = np.where(b[y], 0, np.minimum(run + 1, INF))
        g[y] = run
    run = np.full(W, INF, np.int64)
    for y in range(H - 1, -1, -1):
        run = np.where(b[y], 0, np.minimum(run + 1, INF))
        g[y] = np.minimum(g[y], run)
    dx2 = (np.arange(W)[:, None] - np.arange(W)[None, :]) ** 2
    worst = 0
    for y in np.nonzero(a.any(axis=1))[0]:
        d2 = (dx2 + (g[y] ** 2)[None, :]).min(axis=1)        # for every x of the row
        worst = max(worst, int(d2[a[y]].max()))
    return worst


def hd_px_sq_np(a: np.ndarray, b: np.ndarray) -> int:
    if not a.any() and not b.any():
        return 0
    if a.any() != b.any():
        return -1
    return max(_directed_px_sq(a, b), _directed_px_sq(b, a))


def hd_px_sq_brute(a: np.ndarray, b: np.ndarray) -> int:
    pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
    d2 = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)
    return int(max(d2.min(axis=1).max(), d2.min(axis=0).max()))


def table_np(seg_logits, target, cls_logits=None, pixel_threshold=0, seg_from_class=False, class_from_seg=False) -> np.ndarray:
    """The (N, SEGM_COLS) table of mtbc_seg_metrics, restated: raw mask = logit > 0 (equal to the fp32 `sigmoid > .5` away from 0)."""
    x, t = np.asarray(seg_logits), np.asarray(target)
    N = x.shape[0]
    out = np.zeros((N, L.SEGM_COLS), np.int64)
    for n in range(N):
        raw, gt = x[n, 0] > 0, t[n, 0] != 0
        raw_pixels = int(raw.sum())
        cls_raw = cls_final = -1
        rules = False
        if cls_logits is not None:
            lg = np.asarray(cls_logits)[n].reshape(-1)
            if lg.size == 1:
                cls_raw = cls_final = int(lg[0] > 0)
            else:
                rules = True
                cls_raw = cls_final = int(np.argmax(lg))
        seg = raw
        if pixel_threshold > 0 and raw_pixels <= pixel_threshold:
            seg = np.zeros_like(raw)
        if rules and seg_from_class and cls_raw == NORMAL:
            seg = np.zeros_like(raw)
        if rules and class_from_seg and raw_pixels == 0:
            cls_final = NORMAL
        out[n] = [int((seg & gt).sum()), int((~seg & ~gt).sum()), int((seg & ~gt).sum()), int((~seg & gt).sum()), raw_pixels,
                  hd_rows_sq_np(seg, gt), hd_px_sq_np(seg, gt), cls_raw, cls_final]
    return out


# ------------------------------------------------------------------------------------------------
# fixture
# ------------------------------------------------------------------------------------------------
def load_pairs(golden_dir):
    g = np.load(os.path.join(golden_dir, "test_metrics.npz"))
    pairs = []
    for i, (name, (H, W)) in enumerate(zip(g["names"], g["shapes"])):
        gt = np.unpackbits(g[f"gt_{i:02d}"])[:H * W].reshape(H, W).astype(bool)
        seg = np.unpackbits(g[f"seg_{i:02d}"])[:H * W].reshape(H, W).astype(bool)
        pairs.append((str(name), gt, seg))
    return g, pairs


def logits_of(mask: np.ndarray) -> np.ndarray:
    """(H, W) bool -> (1, 1, H, W) logits whose sign is the mask (any magnitude would do here)."""
    return np.where(mask, 1.0, -1.0).astype(np.float32)[None, None]


def assert_columns_equal(got: dict, want_rows: np.ndarray, columns) -> None:
    for c, name in enumerate(columns):
        assert np.array_equal(got[str(name)], want_rows[:, c], equal_nan=True), (name, got[str(name)], want_rows[:, c])


# ------------------------------------------------------------------------------------------------
# 1 + 2: the formulas and the restated distances against the reference's recorded values, exactly
# ------------------------------------------------------------------------------------------------
def test_metrics_from_table_equals_the_reference_exactly(golden_dir):
    g, pairs = load_pairs(golden_dir)
    assert len(pairs) >= 12 and {"both_empty_64", "gt_only_64", "seg_only_64", "disc_in_ring_256"} <= {n for n, _, _ in pairs}
    table = np.concatenate([table_np(logits_of(seg), gt[None, None].astype(np.float32)) for _, gt, seg in pairs])
    assert table.dtype == np.int64 and (table[:, L.SEGM_TP:L.SEGM_FN + 1].sum(axis=1) == [gt.size for _, gt, _ in pairs]).all()
    got = I.metrics_from_table(table)
    assert all(v.dtype == np.float64 for v in got.values())
    assert list(got) == list(g["columns"]) + ["Hausdorff (pixels)"]
    assert_columns_equal(got, g["metrics"], g["columns"])
    assert np.isnan(g["metrics"]).any() and (g["metrics"][:, 0] > 0).any()          # the fixture does exercise both


def test_restated_row_distance_is_the_references_haussdorf(golden_dir):
    g, pairs = load_pairs(golden_dir)
    for (name, gt, seg), want in zip(pairs, g["metrics"][:, 0]):
        sq = hd_rows_sq_np(seg, gt)
        got = math.nan if sq < 0 else math.sqrt(sq)
        assert (math.isnan(got) and math.isnan(want)) or got == want, (name, sq, want)
        assert hd_rows_sq_np(gt, seg) == sq                                           # symmetric


def test_restated_pixel_distance_equals_brute_force():
    rng = np.random.default_rng(11)
    for H, W, p in [(16, 16, 0.05), (16, 16, 0.5), (48, 80, 0.01), (32, 64, 0.002), (64, 64, 0.3)]:
        for _ in range(3):
            a, b = rng.random((H, W)) < p, rng.random((H, W)) < p
            if not a.any() or not b.any():
                a[0, 0] = b[H - 1, W - 1] = True
            assert hd_px_sq_np(a, b) == hd_px_sq_brute(a, b), (H, W, p)
    y, x = np.mgrid[:128, :128]
    d2 = (y - 64) ** 2 + (x - 64) ** 2
    disc, ring = d2 <= 20 * 20, (d2 >= 40 * 40) & (d2 <= 44 * 44)
    assert hd_px_sq_np(disc, ring) == hd_px_sq_brute(disc, ring) == 1600           # the disc's centre: boundary pixels alone give less
    z = np.zeros((16, 16), bool)
    assert hd_px_sq_np(z, z) == 0 and hd_px_sq_np(z, ~z) == -1 and hd_px_sq_np(~z, z) == -1 and hd_px_sq_np(~z, ~z) == 0


def test_restated_rules_follow_the_recorded_postprocessing(golden_dir):
    g, pairs = load_pairs(golden_dir)
    seen = set()
    for i, th, cleared, want in zip(g["threshold_pair"], g["threshold_value"], g["threshold_cleared"], g["threshold_metrics"]):
        _, gt, seg = pairs[int(i)]
        t = table_np(logits_of(seg), gt[None, None].astype(np.float32), pixel_threshold=int(th))
        assert (t[0, L.SEGM_TP] + t[0, L.SEGM_FP] == 0) == bool(cleared)
        assert t[0, L.SEGM_RAW_PIXELS] == seg.sum()
        assert_columns_equal(I.metrics_from_table(t), want[None], g["columns"])
        seen.add(bool(cleared))
    assert seen == {True, False}
    # the class rules: "normal" clears the mask; an empty RAW mask makes the class "normal", a mask the threshold cleared does not
    _, gt, seg = pairs[0]
    x, m = logits_of(seg), gt[None, None].astype(np.float32)
    normal, benign = np.array([[0.1, 0.2, 0.9]], np.float32), np.array([[0.9, 0.2, 0.1]], np.float32)
    t = table_np(x, m, normal, seg_from_class=True)
    assert t[0, L.SEGM_TP] == 0 and t[0, L.SEGM_FN] == gt.sum() and t[0, L.SEGM_HD_ROWS_SQ] == -1 and list(t[0, -2:]) == [2, 2]
    assert table_np(x, m, normal)[0, L.SEGM_TP] > 0
    t = table_np(x, m, benign, pixel_threshold=int(seg.sum()), class_from_seg=True)
    assert t[0, L.SEGM_TP] == 0 and list(t[0, -2:]) == [0, 0]
    t = table_np(logits_of(np.zeros_like(seg)), m, benign, class_from_seg=True)
    assert list(t[0, -2:]) == [0, 2]
    t = table_np(x, m, np.array([[3.0]], np.float32), seg_from_class=True, class_from_seg=True)       # binary head: no rules
    assert t[0, L.SEGM_TP] > 0 and list(t[0, -2:]) == [1, 1]


# ------------------------------------------------------------------------------------------------
# 3: classification summaries
# ------------------------------------------------------------------------------------------------
def test_classification_report_equals_recorded_sklearn(golden_dir):
    g = np.load(os.path.join(golden_dir, "test_metrics.npz"))
    keys = [str(k) for k in g["multiclass_keys"]]
    assert len(keys) == 19 and keys[-1] == "accuracy"
    for tag in "abc":
        gt, pr = g[f"labels_{tag}_gt"], g[f"labels_{tag}_pred"]
        got = I.classification_report(gt, pr)
        assert list(got) == keys
        for k, want in zip(keys, g[f"labels_{tag}_values"]):
            assert abs(got[k] - want) <= 1e-12, (tag, k, got[k], want)
    assert 2 not in g["labels_b_pred"] and 1 not in g["labels_c_gt"]                  # never predicted / absent from the ground truth
    got = I.classification_report(g["labels_bin_gt"], g["labels_bin_pred"], labels=(0, 1))
    assert list(got) == [str(k) for k in g["binary_keys"]]
    for k, want in zip(got, g["labels_bin_values"]):
        assert abs(got[k] - want) <= 1e-12, (k, got[k], want)


# ------------------------------------------------------------------------------------------------
# 4: C-ABI
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_seg_metrics_names_in_header_binding_and_library(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(mtbc_[A-Za-z0-9_]+)\s*\(", src))
    for name in ("mtbc_seg_metrics", "mtbc_seg_metrics_workspace_size"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name)
    assert "mtbc_seg_metrics_args" in src and hasattr(L, "SegMetricsArgs")
    assert int(re.search(r"#define\s+MTBC_SEGM_COLS\s+(\d+)", src).group(1)) == L.SEGM_COLS
    for name in ("TP", "TN", "FP", "FN", "RAW_PIXELS", "HD_ROWS_SQ", "HD_PX_SQ", "CLS_RAW", "CLS_FINAL"):
        assert int(re.search(rf"#define\s+MTBC_SEGM_{name}\s+(\d+)", src).group(1)) == getattr(L, "SEGM_" + name)
    assert lib.mtbc_version() == 203 and "MTBC_OP_SEG" not in src                    # additive: no new version, no new op kind


def test_seg_metrics_args_layout(tmp_path):
    fields = ["N", "n_cls", "seg_logits", "cls_logits", "pixel_threshold", "normal_class", "out", "workspace", "workspace_bytes"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(mtbc_seg_metrics_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbc_seg_metrics_args, {f}));' for f in fields]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(L.SegMetricsArgs)
    for f in fields:
        assert int(got[f]) == getattr(L.SegMetricsArgs, f).offset, f


def _args(N=2, H=64, W=64, ptr=0x1000):
    a = L.SegMetricsArgs()
    a.N, a.H, a.W, a.n_cls = N, H, W, 3
    a.seg_logits = a.target = a.cls_logits = a.out = a.workspace = ptr           # never dereferenced: every call below is refused first
    a.normal_class = 2
    return a


def test_seg_metrics_workspace_size_and_refusals_need_no_device(lib):
    size = lambda **kw: lib.mtbc_seg_metrics_workspace_size(C.byref(_args(**kw)))          # noqa: E731
    sizes = [size(N=n, H=256, W=256) for n in (1, 2, 5, 32)]
    assert sizes[0] > 0 and sizes == sorted(set(sizes)) and sizes[3] == 32 * sizes[0]
    assert size(N=1, H=512, W=512) >= 4 * 512 * 512 // 8                                   # four bit planes
    assert size(N=1, H=48, W=80) > 0 and size(N=1, H=16, W=16) > 0
    for bad in (dict(W=40), dict(H=528), dict(N=0), dict(H=8), dict(W=520), dict(H=100)):
        a = _args(**bad)
        assert lib.mtbc_seg_metrics_workspace_size(C.byref(a)) == 0, bad
        a.workspace_bytes = 1 << 30
        assert lib.mtbc_seg_metrics(C.byref(a), None) == -1, bad                           # MTBC_E_BADSHAPE
    assert lib.mtbc_seg_metrics(None, None) == -2
    for field in ("seg_logits", "target", "out", "workspace"):
        a = _args()
        a.workspace_bytes = 1 << 30
        setattr(a, field, None)
        assert lib.mtbc_seg_metrics(C.byref(a), None) == -2, field                         # MTBC_E_BADARG
    a = _args()
    a.workspace_bytes = size() - 1
    assert lib.mtbc_seg_metrics(C.byref(a), None) == -3                                    # MTBC_E_WORKSPACE
    a = _args()
    a.workspace_bytes, a.n_cls = 1 << 30, 0
    assert lib.mtbc_seg_metrics(C.byref(a), None) == -2                                    # class logits without columns
    a = _args()
    a.workspace_bytes, a.pixel_threshold = 1 << 30, -1
    assert lib.mtbc_seg_metrics(C.byref(a), None) == -2


# ------------------------------------------------------------------------------------------------
# 5: the two CSV files
# ------------------------------------------------------------------------------------------------
def test_write_result_csvs_columns_and_nan(tmp_path):
    t = np.array([[5, 90, 3, 2, 8, 26, 9, 1, 1], [0, 95, 0, 5, 0, -1, -1, 0, 2], [0, 100, 0, 0, 0, 0, 0, 2, 2]], np.int64)
    cols = I.metrics_from_table(t)
    seg_rows = []
    for i, (pid, cname) in enumerate([(17, "benign"), (4, "malignant"), (230, "normal")]):
        row = {"patient_id": pid, "class": cname}
        row.update({k: float(v[i]) for k, v in cols.items()})
        seg_rows.append(row)
    cls_rows = [{"patient_id": 17, "ground_truth": 0, "predicted_label": 1, "prob_benign": 0.25, "prob_malignant": 1.5, "prob_normal": -2.0},
                {"patient_id": 4, "ground_truth": 1, "predicted_label": 2, "prob_benign": 0.1, "prob_malignant": 0.30000000000000004, "prob_normal": 1e-9}]
    seg_file, cls_file = I.write_result_csvs(str(tmp_path / "fold0"), seg_rows, cls_rows)
    assert os.path.basename(seg_file) == "results_segmentation.csv" and os.path.basename(cls_file) == "results_classification.csv"
    rows = list(csv.reader(open(seg_file, newline="")))
    # the reference's DataFrame columns (utils/models.py:297-298), then the extra distance
    assert rows[0] == ["patient_id", "Haussdorf distance", "DICE", "Sensitivity", "Specificity", "Accuracy", "Jaccard index", "Precision",
                       "class", "Hausdorff (pixels)"]
    assert len(rows) == 4 and all(len(r) == 10 for r in rows)
    back = [[math.nan if v == "" else float(v) for v in r[1:8] + r[9:]] for r in rows[1:]]
    want = [[row[k] for k in rows[0][1:8] + rows[0][9:]] for row in seg_rows]
    assert np.array_equal(np.array(back), np.array(want), equal_nan=True)               # repr round-trips every float, NaN as ''
    assert np.isnan(np.array(back)).sum() == 6 and [r[0] for r in rows[1:]] == ["17", "4", "230"] and rows[2][8] == "malignant"
    rows = list(csv.reader(open(cls_file, newline="")))
    assert rows[0] == ["patient_id", "ground_truth", "predicted_label", "prob_benign", "prob_malignant", "prob_normal"]
    assert rows[2] == ["4", "1", "2", "0.1", "0.30000000000000004", "1e-09"]
    _, cls_file = I.write_result_csvs(str(tmp_path / "binary"), seg_rows, [{k: r[k] for k in list(r)[:3]} for r in cls_rows])
    rows = list(csv.reader(open(cls_file, newline="")))
    assert rows[0] == ["patient_id", "ground_truth", "predicted_label"] and rows[1] == ["17", "0", "1"]     # binary head (:262-266)
