"""Test-time prediction refining and the testing phase's result tables (second half).

`inference_multitask_multiclass_classification_segmentation` (src/utils/models.py:270-400) runs the model twice
over the batch-1 test loader and applies two cross-task rules, each on the RAW prediction of the other task:

  * overlap_seg_based_on_class (:325-332): predicted class == 2 ("normal") -> the predicted mask is cleared;
  * overlap_class_based_on_seg (:366-376): no tumour pixel in sigmoid(last head) > .5 -> the predicted class becomes 2,

after the optional `threshold_postprocessing` (images.py:41-55: a raw mask of at most `threshold` pixels is cleared), and writes
`results_segmentation.csv` (one row per image: metrics.py:26-74) and `results_classification.csv`.

`refine_predictions` / `predict` are the two rules as tensor ops for a whole batch.  `FusedTestStep` is the whole testing
phase on the device: the compiled forward programs, then `seg_metrics` (csrc/seg_metrics.hip) turns the last head's logits,
the mask and the class logits into an exact integer table per image -- confusion counts of the final mask, the raw pixel
count, the reference's row-wise "Haussdorf distance" and the Hausdorff distance of the pixel sets, the class before and after
its rule -- with no host round trip per image or per batch; `metrics_from_table` turns it into the reference's columns and
`write_csv` into its two files.  `classification_report` restates the sklearn summaries of metrics.py:387-458 in numpy.
PNG dumps and the xlsx aggregation are not covered (the reference's own `save_*_results` reads the two CSV files).

`FusedSegTestStep` is the testing phase of the single-task segmentation driver (`inference_binary_segmentation`, src/utils/models.py:39-100,
which training_segmentation.py:179 runs after EVERY epoch): forward, `fill_holes` (csrc/fill_holes.hip =
scipy.ndimage.binary_fill_holes of the predicted mask, the driver's default), then the same `seg_metrics` table without class rules.
"""
from __future__ import annotations

import csv
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L

NORMAL_CLASS = 2
_E_BADSHAPE = -1       # MTBC_E_BADSHAPE

# results_segmentation.csv (utils/models.py:297-298); the pixel-set Hausdorff distance goes last, after the reference's columns
SEG_METRIC_COLUMNS = ("Haussdorf distance", "DICE", "Sensitivity", "Specificity", "Accuracy", "Jaccard index", "Precision")
HAUSDORFF_PIXELS = "Hausdorff (pixels)"
SEG_CSV_COLUMNS = ("patient_id",) + SEG_METRIC_COLUMNS + ("class", HAUSDORFF_PIXELS)
# results_classification.csv (:389-394; the binary head writes the first three, :262-266)
CLS_CSV_COLUMNS = ("patient_id", "ground_truth", "predicted_label", "prob_benign", "prob_malignant", "prob_normal")


def _last(x):
    return x[-1] if isinstance(x, (list, tuple)) else x


def _mean_logits(logits: Union[torch.Tensor, Sequence[torch.Tensor]]) -> torch.Tensor:
    if isinstance(logits, (list, tuple)):                       # deep supervision: average the heads (:327, :358)
        return torch.mean(torch.stack(list(logits), dim=0), dim=0)
    return logits


def refine_predictions(cls_logits, seg_logits, overlap_seg_based_on_class: bool = True,
                       overlap_class_based_on_seg: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cls_logits, seg_logits) as returned by the model -> (binary masks (N,1,H,W) float, class ids (N,) int64)."""
    lg = _mean_logits(cls_logits)
    lg = lg.view(lg.shape[0], -1)
    raw_cls = lg.argmax(dim=1)
    raw_seg = (torch.sigmoid(_last(seg_logits)) > .5).float()
    seg, cls = raw_seg, raw_cls
    if overlap_seg_based_on_class:
        seg = raw_seg * (raw_cls != NORMAL_CLASS).view(-1, 1, 1, 1).to(raw_seg.dtype)
    if overlap_class_based_on_seg:
        empty = raw_seg.flatten(1).sum(dim=1) == 0
        cls = torch.where(empty, torch.full_like(raw_cls, NORMAL_CLASS), raw_cls)
    return seg, cls


@torch.no_grad()
def predict(model, images: torch.Tensor, overlap_seg_based_on_class: bool = True,
            overlap_class_based_on_seg: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One forward pass + refining: (masks, class ids, class probabilities)."""
    logits, segs = model(images)
    seg, cls = refine_predictions(logits, segs, overlap_seg_based_on_class, overlap_class_based_on_seg)
    lg = _mean_logits(logits)
    return seg, cls, torch.softmax(lg.view(lg.shape[0], -1), dim=1)


# ------------------------------------------------------------------------------------------------
# the testing phase: per-image tables on the device
# ------------------------------------------------------------------------------------------------
def seg_metrics(seg_logits: torch.Tensor, target: torch.Tensor, cls_logits: Optional[torch.Tensor] = None,
                pixel_threshold: int = 0, seg_from_class: bool = False, class_from_seg: bool = False) -> torch.Tensor:
    """mtbc_seg_metrics: (N,1,H,W) logits of the last head, (N,1,H,W) mask, optional (N,K) class logits -> int64 (N, SEGM_COLS)
    on the device (columns `_lib.SEGM_*`).  Two launches on the current stream, nothing is read back."""
    import ctypes as C
    if seg_logits.dim() != 4 or seg_logits.shape[1] != 1 or tuple(target.shape) != tuple(seg_logits.shape):
        raise ValueError(f"expected (N,1,H,W) logits and a mask of the same shape, got {tuple(seg_logits.shape)} / {tuple(target.shape)}")
    if seg_logits.device.type != "cuda":
        L.require_gpu()
        raise L.MtbcError("seg_metrics needs device tensors (no CPU path)")
    x, t = seg_logits.contiguous().float(), target.contiguous().float()
    a = L.SegMetricsArgs()
    a.N, a.H, a.W = x.shape[0], x.shape[2], x.shape[3]
    a.seg_logits, a.target = x.data_ptr(), t.data_ptr()
    lg = None
    if cls_logits is not None:
        lg = cls_logits.reshape(x.shape[0], -1).contiguous().float()
        a.n_cls, a.cls_logits = lg.shape[1], lg.data_ptr()
    a.pixel_threshold, a.seg_from_class, a.class_from_seg, a.normal_class = int(pixel_threshold), int(bool(seg_from_class)), int(bool(class_from_seg)), NORMAL_CLASS
    lib = L.load()
    nbytes = lib.mtbc_seg_metrics_workspace_size(C.byref(a))
    if nbytes == 0:
        L.check(_E_BADSHAPE, f"seg_metrics (N, H, W) = ({a.N}, {a.H}, {a.W}): H and W must be multiples of 16 in [16, 512]")
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
    out = torch.empty(x.shape[0], L.SEGM_COLS, dtype=torch.int64, device=x.device)
    a.out, a.workspace, a.workspace_bytes = out.data_ptr(), ws.data_ptr(), nbytes
    L.check(lib.mtbc_seg_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "seg_metrics")
    return out



def fill_holes(seg_logits: torch.Tensor, error: torch.Tensor, want_logits: bool = True, want_u8: bool = False):
    """mtbc_fill_holes: (N,1,H,W) logits of the last head -> (filled_logits (N,1,H,W) float32 of +-1 or None, filled_u8 (N,H,W) uint8 of 255 / 0
    or None): scipy.ndimage.binary_fill_holes(sigmoid(logits) > .5), one workgroup per image, one launch on the current stream.  `error`: a
    device int32 word the kernel sets when its pass bound was reached (never, unless the kernel is broken); the caller reads it when it reads
    its results."""
    import ctypes as C
    if seg_logits.dim() != 4 or seg_logits.shape[1] != 1:
        raise ValueError(f"expected (N,1,H,W) logits, got {tuple(seg_logits.shape)}")
    if seg_logits.device.type != "cuda":
        L.require_gpu()
        raise L.MtbcError("fill_holes needs device tensors (no CPU path)")
    if error.dtype != torch.int32 or error.numel() != 1 or error.device != seg_logits.device:
        raise ValueError("error must be one int32 word on the logits' device")
    if not (want_logits or want_u8):
        raise ValueError("ask for at least one of the two outputs")
    x = seg_logits.contiguous().float()
    N, _, H, W = x.shape
    out_f = torch.empty_like(x) if want_logits else None
    out_u8 = torch.empty(N, H, W, dtype=torch.uint8, device=x.device) if want_u8 else None
    a = L.FillHolesArgs()
    a.N, a.H, a.W, a.seg_logits, a.error = N, H, W, x.data_ptr(), error.data_ptr()
    a.filled_logits = out_f.data_ptr() if want_logits else None
    a.filled_u8 = out_u8.data_ptr() if want_u8 else None
    rc = L.load().mtbc_fill_holes(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, f"fill_holes (N, H, W) = ({N}, {H}, {W}): H and W must be multiples of 16 in [16, 512]" if rc == _E_BADSHAPE else "fill_holes")
    return out_f, out_u8


def metrics_from_table(table) -> Dict[str, np.ndarray]:
    """Integer table (M, SEGM_COLS) -> the reference's per-image columns as float64 arrays, its conventions included
    (metrics.py:175-252): sensitivity / precision NaN when tp == 0; DICE / Jaccard 1 or 0 on an empty ground truth; Hausdorff 0 for
    two empty masks and NaN for exactly one.  The same integers through the same formula, so the values equal the reference's bit
    for bit.  (Specificity of a mask with no background pixel is NaN here; the reference divides by zero and raises.)"""
    t = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table).astype(np.int64).reshape(-1, L.SEGM_COLS)
    tp, tn, fp, fn = (t[:, c].astype(np.float64) for c in (L.SEGM_TP, L.SEGM_TN, L.SEGM_FP, L.SEGM_FN))
    nan = np.full(tp.shape, np.nan)

    def div(num, den, where, other):
        return np.where(where, np.divide(num, den, out=np.zeros_like(num), where=where & (den != 0)), other)

    def root(sq):
        sq = sq.astype(np.float64)
        return np.where(sq < 0, np.nan, np.sqrt(np.maximum(sq, 0.0)))

    gt_empty, seg_empty = (tp + fn) == 0, (tp + fp) == 0
    empty_score = np.where(seg_empty, 1.0, 0.0)
    return {
        "Haussdorf distance": root(t[:, L.SEGM_HD_ROWS_SQ]),
        "DICE": div(2 * tp, 2 * tp + fp + fn, ~gt_empty, empty_score),
        "Sensitivity": div(tp, tp + fn, tp != 0, nan),
        "Specificity": div(tn, tn + fp, (tn + fp) != 0, nan),
        "Accuracy": div(tp + tn, tp + tn + fp + fn, np.ones(tp.shape, bool), nan),
        "Jaccard index": div(tp, tp + fp + fn, ~gt_empty, empty_score),
        "Precision": div(tp, tp + fp, tp != 0, nan),
        HAUSDORFF_PIXELS: root(t[:, L.SEGM_HD_PX_SQ]),
    }


def classification_report(ground_truth, predicted, labels: Sequence[int] = (0, 1, 2)) -> Dict[str, float]:
    """`multiclass_classification_metrics` (metrics.py:407-458: sklearn precision / recall / f1 per class, macro, micro, weighted, and
    accuracy_score) from the confusion counts, a zero denominator giving 0 as sklearn's zero_division default does; with two labels the
    five keys of `binary_classification_metrics` (:387-400, the reference's own NaN conventions; label 1 is the positive class)."""
    gt = np.asarray(ground_truth).astype(np.int64).reshape(-1)
    pr = np.asarray(predicted).astype(np.int64).reshape(-1)
    if gt.shape != pr.shape or gt.size == 0:
        raise ValueError("ground_truth and predicted must be non-empty and of equal length")
    labels = list(labels)

    def safe(num, den):
        num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
        return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)

    if len(labels) == 2:
        neg, pos = labels
        tp, tn = float(np.sum((gt == pos) & (pr == pos))), float(np.sum((gt == neg) & (pr == neg)))
        fp, fn = float(np.sum((gt == neg) & (pr == pos))), float(np.sum((gt == pos) & (pr == neg)))
        return {"Precision": tp / (tp + fp) if tp else math.nan, "Sensitivity": tp / (tp + fn) if tp else math.nan,
                "Specificity": tn / (tn + fp) if tn + fp else math.nan, "Accuracy": (tp + tn) / (tp + tn + fp + fn),
                "F1 score": 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else math.nan}
    tp = np.array([np.sum((gt == c) & (pr == c)) for c in labels], np.float64)
    pred_sum = np.array([np.sum(pr == c) for c in labels], np.float64)
    true_sum = np.array([np.sum(gt == c) for c in labels], np.float64)
    out: Dict[str, float] = {}
    for name, per_class, micro in (("precision", safe(tp, pred_sum), safe(tp.sum(), pred_sum.sum())),
                                   ("recall", safe(tp, true_sum), safe(tp.sum(), true_sum.sum())),
                                   ("f1", safe(2 * tp, pred_sum + true_sum), safe(2 * tp.sum(), pred_sum.sum() + true_sum.sum()))):
        for n, v in enumerate(per_class):
            out[f"{name}_class_{n}"] = float(v)
        out[f"{name}_macro"] = float(per_class.mean())
        out[f"{name}_micro"] = float(micro)
        out[f"{name}_weighted"] = float(safe((per_class * true_sum).sum(), true_sum.sum()))
    out["accuracy"] = float(np.mean(gt == pr))
    return out


def _csv_value(v):
    if isinstance(v, (float, np.floating)):
        return "" if math.isnan(v) else repr(float(v))          # an empty field is how pandas writes (and reads back) NaN
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def write_result_csvs(path: str, segmentation_rows: Sequence[dict], classification_rows: Sequence[dict]) -> Tuple[str, str]:
    """`results_segmentation.csv` and `results_classification.csv` under `path`, the reference's columns in its order."""
    os.makedirs(path, exist_ok=True)
    seg_file, cls_file = os.path.join(path, "results_segmentation.csv"), os.path.join(path, "results_classification.csv")
    cls_cols = [c for c in CLS_CSV_COLUMNS if not classification_rows or c in classification_rows[0]]
    for file, cols, rows in ((seg_file, SEG_CSV_COLUMNS, segmentation_rows), (cls_file, cls_cols, classification_rows)):
        with open(file, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(cols)
            for r in rows:
                w.writerow([_csv_value(r[c]) for c in cols])
    return seg_file, cls_file


class FusedTestStep:
    """The testing phase of a fold (training_multitask.py:296-308 -> utils/models.py:273-397; binary head: :186-270) in batches on the
    device.  Per batch: the compiled `pack` + `fwd` programs of the batch shape, then `seg_metrics` on the last segmentation head and
    the class logits where the programs left them; the (N, SEGM_COLS) integer table, the class logits and the labels stay on the
    device.  `result()` reads everything back once and returns `(segmentation_rows, classification_rows)`, lists of dicts keyed by
    the reference's CSV columns; `write_csv(path)` writes its two files.  The arguments default to the reference's signature
    defaults (config keys `threshold_postprocessing`, `overlap_seg_based_on_class`, `overlap_class_based_on_seg`); the binary head
    (model.n_classes == 1) has no rules in the reference and takes none here."""

    def __init__(self, model, pixel_threshold: int = 0, overlap_seg_based_on_class: bool = False,
                 overlap_class_based_on_seg: bool = False):
        self.model = model
        self.binary = getattr(model, "n_classes", 3) == 1
        if self.binary and (pixel_threshold or overlap_seg_based_on_class or overlap_class_based_on_seg):
            raise ValueError("the binary head's testing phase has no post-processing rules (utils/models.py:186-270)")
        if int(pixel_threshold) < 0:
            raise ValueError("pixel_threshold must be >= 0 (0 = off)")
        self.pixel_threshold = int(pixel_threshold)
        self.seg_from_class, self.class_from_seg = bool(overlap_seg_based_on_class), bool(overlap_class_based_on_seg)
        self.reset()

    def reset(self) -> None:
        self._tables: List[torch.Tensor] = []      # device int64 (N, SEGM_COLS) per batch
        self._logits: List[torch.Tensor] = []      # device float32 (N, K) per batch
        self._labels: List[torch.Tensor] = []      # device int64 (N,) per batch
        self._ids: list = []
        self._classes: list = []
        self._coop_err = None

    @staticmethod
    def _as_list(v, n: int) -> list:
        if isinstance(v, torch.Tensor):
            v = v.reshape(-1).tolist()
        elif isinstance(v, np.ndarray):
            v = v.reshape(-1).tolist()
        elif isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
            v = [v]
        v = list(v)
        if len(v) != n:
            raise ValueError(f"expected {n} values per batch, got {len(v)}")
        return v

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, mask: torch.Tensor, label: torch.Tensor, patient_id=None, class_name=None) -> None:
        N, _, H, W = image.shape
        st = self.model.compiled(N, H, W)
        st.x.data.copy_(image, non_blocking=True)
        self._evaluate(st, mask, label, patient_id, class_name)

    @torch.no_grad()
    def indexed(self, dataset, index, patient_id=None, class_name=None) -> None:
        """`__call__` from a device-resident dataset (device_data.DeviceDataset): one assembly launch (identity transform) straight into the
        plan's input, a mask plane and a float label column of the batch's own."""
        st = self.model.compiled(len(index), dataset.H, dataset.W)
        dev = st.x.data.device
        mask = torch.empty(st.N, 1, st.H, st.W, dtype=torch.float32, device=dev)
        label = torch.empty(st.N, 1, dtype=torch.float32, device=dev)
        dataset.assemble(index, None, n_onehot=0, out=(st.x.data, mask, label))
        self._evaluate(st, mask, label, patient_id, class_name)

    def _evaluate(self, st, mask: torch.Tensor, label: torch.Tensor, patient_id, class_name) -> None:
        """Everything behind the filled input buffer: the programs, the metrics launch, the batch's rows."""
        N, dev = st.N, st.x.data.device
        st.programs["pack"].run()
        st.programs["fwd"].run()
        self._coop_err = self.model.coop_error_word()
        logits = st.logits.data.view(N, -1)
        table = seg_metrics(st.segs[-1].data, mask.to(dev, non_blocking=True), logits, self.pixel_threshold,
                            self.seg_from_class, self.class_from_seg)
        self._tables.append(table)
        self._logits.append(logits.clone())                      # the plan's buffer is rewritten by the next batch of this shape
        self._labels.append(label.to(dev, non_blocking=True).reshape(-1).to(torch.int64))
        first = len(self._ids)
        self._ids += list(range(first, first + N)) if patient_id is None else self._as_list(patient_id, N)
        self._classes += [None] * N if class_name is None else self._as_list(class_name, N)

    def result(self) -> Tuple[List[dict], List[dict]]:
        if not self._tables:
            raise L.MtbcError("FusedTestStep.result() before any batch was evaluated")
        table, logits, labels = torch.cat(self._tables), torch.cat(self._logits), torch.cat(self._labels)
        M, K = logits.shape
        err = self._coop_err
        flat = torch.cat([table.double().flatten(), logits.double().flatten(), labels.double(),
                          (err if err is not None else labels[:1] * 0).double().flatten()]).cpu().numpy()     # the one read-back
        if flat[-1] != 0.0:
            L.raise_coop_timeout()
        table = flat[:M * L.SEGM_COLS].astype(np.int64).reshape(M, L.SEGM_COLS)
        logits = flat[M * L.SEGM_COLS:M * (L.SEGM_COLS + K)].reshape(M, K)
        labels = flat[M * (L.SEGM_COLS + K):M * (L.SEGM_COLS + K + 1)].astype(np.int64)
        self.table = table                                        # the integers behind the rows
        cols = metrics_from_table(table)
        seg_rows, cls_rows = [], []
        for i in range(M):
            row = {"patient_id": self._ids[i]}
            row.update({c: float(cols[c][i]) for c in SEG_METRIC_COLUMNS})
            row["class"] = int(labels[i]) if self._classes[i] is None else self._classes[i]
            row[HAUSDORFF_PIXELS] = float(cols[HAUSDORFF_PIXELS][i])
            seg_rows.append(row)
            crow = {"patient_id": self._ids[i], "ground_truth": int(labels[i]), "predicted_label": int(table[i, L.SEGM_CLS_FINAL])}
            if not self.binary:                                   # the reference's "prob_*" columns hold the mean class LOGITS (:363)
                crow.update({c: float(v) for c, v in zip(CLS_CSV_COLUMNS[3:], logits[i])})
            cls_rows.append(crow)
        return seg_rows, cls_rows

    def write_csv(self, path: str) -> Tuple[str, str]:
        seg_rows, cls_rows = self.result()
        return write_result_csvs(path, seg_rows, cls_rows)


class FusedSegTestStep:
    """The testing phase of the single-task segmentation driver (training_segmentation.py:179, :206 -> `inference_binary_segmentation`,
    utils/models.py:39-100) in batches on the device.  Per batch: the compiled `pack` + `fwd` programs, `fill_holes` on the last head when
    `fill_holes` is true (the driver's default), then `seg_metrics` on the filled mask -- as logits of +-1, whose sigmoid falls on the right side
    of .5 -- with no class logits and no rules.  `result()` reads everything back once and returns the rows of `results_segmentation.csv`
    (the reference's columns through `metrics_from_table`; `class` is the caller's class name); `write_csv(path)` writes that one file;
    `masks_u8()` returns the filled masks as 0 / 255 planes, what `save_binary_segmentation` writes to segs/*.png (with keep_masks=True;
    writing the PNG files is the caller's business).  `__call__` takes the batch; `evaluate_logits` takes the last head's logits directly."""

    def __init__(self, model, fill_holes: bool = True, keep_masks: bool = False):
        self.model, self.fill_holes, self.keep_masks = model, bool(fill_holes), bool(keep_masks)
        self._error = self._scratch = None
        self.reset()

    def reset(self) -> None:
        self._tables: List[torch.Tensor] = []      # device int64 (N, SEGM_COLS) per batch
        self._masks: List[torch.Tensor] = []       # device uint8 (N, H, W) per batch (keep_masks)
        self._ids: list = []
        self._classes: list = []
        self._coop_err = None
        if self._error is not None:
            self._error.zero_()

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, mask: torch.Tensor, patient_id=None, class_name=None) -> None:
        N, _, H, W = image.shape
        st = self.model.compiled(N, H, W)
        st.x.data.copy_(image, non_blocking=True)
        st.programs["pack"].run()
        st.programs["fwd"].run()
        self._coop_err = self.model.coop_error_word()
        self.evaluate_logits(st.segs[-1].data, mask, patient_id, class_name)

    @torch.no_grad()
    def indexed(self, dataset, index) -> None:
        """`__call__` from a device-resident dataset (device_data.DeviceDataset): one assembly launch (identity transform) into the plan's input
        and a mask plane of the batch's own; the labels go to a scratch column nothing reads."""
        st = self.model.compiled(len(index), dataset.H, dataset.W)
        if self._scratch is None or self._scratch.shape[0] != st.N:
            self._scratch = torch.empty(st.N, 1, dtype=torch.float32, device=dataset.device)
        image, mask, _ = dataset.assemble(index, None, n_onehot=0, out=(st.x.data, torch.empty_like(st.segs[-1].data), self._scratch))
        self(image, mask)

    @torch.no_grad()
    def evaluate_logits(self, seg_logits: torch.Tensor, mask: torch.Tensor, patient_id=None, class_name=None) -> None:
        """The two launches behind the forward, on (N,1,H,W) logits of the last head that are already on the device."""
        dev, N = seg_logits.device, seg_logits.shape[0]
        if self._error is None or self._error.device != dev:
            self._error = torch.zeros(1, dtype=torch.int32, device=dev)
        x, u8 = seg_logits, None
        if self.fill_holes:
            x, u8 = fill_holes(seg_logits, self._error, want_logits=True, want_u8=self.keep_masks)
        elif self.keep_masks:
            u8 = (torch.sigmoid(seg_logits[:, 0].float()) > .5).to(torch.uint8) * 255
        self._tables.append(seg_metrics(x, mask.to(dev, non_blocking=True)))
        if u8 is not None:
            self._masks.append(u8)
        first = len(self._ids)
        self._ids += list(range(first, first + N)) if patient_id is None else FusedTestStep._as_list(patient_id, N)
        self._classes += [None] * N if class_name is None else FusedTestStep._as_list(class_name, N)

    def result(self) -> List[dict]:
        if not self._tables:
            raise L.MtbcError("FusedSegTestStep.result() before any batch was evaluated")
        table = torch.cat(self._tables)
        M = table.shape[0]
        err = self._coop_err
        flat = torch.cat([table.flatten(), self._error.to(torch.int64),
                          (err if err is not None else self._error * 0).to(torch.int64).flatten()]).cpu().numpy()     # the one read-back
        if flat[-1] != 0:
            L.raise_coop_timeout()
        if flat[-2] != 0:
            raise L.MtbcError("fill_holes: the pass bound H*W + 1 was reached before the flood was stable: the filled masks are invalid")
        self.table = flat[:M * L.SEGM_COLS].reshape(M, L.SEGM_COLS)          # the integers behind the rows
        cols = metrics_from_table(self.table)
        rows = []
        for i in range(M):
            row = {"patient_id": self._ids[i]}
            row.update({c: float(cols[c][i]) for c in SEG_METRIC_COLUMNS})
            row["class"] = self._classes[i]
            row[HAUSDORFF_PIXELS] = float(cols[HAUSDORFF_PIXELS][i])
            rows.append(row)
        return rows

    def mean_dice(self) -> float:
        """The `Test` column of the driver's metrics.csv: the mean DICE over the test set (training_segmentation.py:179-183)."""
        return float(np.mean([r["DICE"] for r in self.result()]))

    def masks_u8(self) -> List[np.ndarray]:
        """The (filled) predicted masks of every image so far as (H, W) uint8 arrays of 0 / 255, in order (needs keep_masks=True)."""
        if not self.keep_masks:
            raise ValueError("build the FusedSegTestStep with keep_masks=True")
        return [m for batch in self._masks for m in batch.cpu().numpy()]

    def write_csv(self, path: str) -> str:
        """`results_segmentation.csv` under `path`, the reference's columns in its order (utils/models.py:52-53, :97-98)."""
        rows = self.result()
        os.makedirs(path, exist_ok=True)
        file = os.path.join(path, "results_segmentation.csv")
        with open(file, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(SEG_CSV_COLUMNS)
            for r in rows:
                w.writerow([_csv_value(r[c]) for c in SEG_CSV_COLUMNS])
        return file


def cls_rows_from_table(table, ids=None) -> List[dict]:
    """The rows of the classification driver's results.csv (utils/models.py:448-452, :497-501) from the (M, 2) int table
    (ground_truth, predicted_label) `mtbc_cls_test_rows` appended; `ids`: the patient ids (default 0 .. M - 1)."""
    table = np.asarray(table).reshape(-1, 2)
    ids = list(range(len(table))) if ids is None else list(ids)
    if len(ids) != len(table):
        raise ValueError(f"{len(table)} rows but {len(ids)} patient ids")
    return [{"patient_id": i, "ground_truth": int(g), "predicted_label": int(p)} for i, (g, p) in zip(ids, table.tolist())]


def write_cls_rows_csv(path: str, rows: List[dict]) -> None:
    """results.csv as `metrics.to_csv(..., index=False)` writes it: `patient_id,ground_truth,predicted_label`."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["patient_id", "ground_truth", "predicted_label"])
        for r in rows:
            w.writerow([r["patient_id"], r["ground_truth"], r["predicted_label"]])


class FusedClsTestStep:
    """The testing phase of the single-task classification driver (training_classification.py:284-298 -> `inference_multiclass_classification` /
    `inference_binary_classification`, utils/models.py:400-505) in batches on the device.  Per batch: the compiled `pack` + `fwd` programs, then ONE
    launch (`mtbc_cls_test_rows`) that appends (ground_truth, predicted_label) of every image to an int32 table at a device cursor: argmax of the
    model's output against argmax of the one-hot label, or, for the binary head, sigmoid(output) > .5 against the {0, 1} label.  `result()` is one
    read-back and returns the rows of results.csv; `write_csv(path)` writes that file; `report()` gives `multiclass_classification_metrics` (three
    classes) or the five numbers of `binary_classification_metrics` (binary head) through `classification_report`.  `capacity`: images per
    testing phase the table holds (8 bytes each)."""

    cls_only = True

    def __init__(self, model, capacity: int = 65536):
        if not getattr(model, "cls_only", False):
            raise ValueError("FusedClsTestStep takes a classification-only model (nets.nnUNetClassifier, nets.UNetPlusPlusClassifier)")
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1 row")
        self.model, self.capacity = model, int(capacity)
        self.binary = model.n_classes == 1
        self._rows = self._state = self._target = self._scratch = None
        self._coop_err = None
        self._ids: list = []
        self.table = None

    def _buffers(self, dev) -> None:
        if self._rows is None or self._rows.device != dev:
            self._rows = torch.zeros(self.capacity, 2, dtype=torch.int32, device=dev)
            self._state = torch.zeros(2, dtype=torch.int32, device=dev)

    def reset(self) -> None:
        self._ids = []
        self._coop_err = None
        if self._state is not None:
            self._state.zero_()

    def _target_buffer(self, N: int, dev) -> torch.Tensor:
        c = 1 if self.binary else 3
        t = self._target
        if t is None or t.shape != (N, c) or t.device != dev:
            self._target = t = torch.empty(N, c, dtype=torch.float32, device=dev)
        return t

    def _forward_and_append(self, st, target: torch.Tensor, patient_id) -> None:
        st.programs["pack"].run()
        st.programs["fwd"].run()
        self._coop_err = self.model.coop_error_word()
        self.append_outputs(st.logits.data.view(st.N, -1), target, patient_id)

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, label: torch.Tensor, patient_id=None) -> None:
        N, _, H, W = image.shape
        st = self.model.compiled(N, H, W)
        st.x.data.copy_(image, non_blocking=True)
        dev = st.x.data.device
        target = self._target_buffer(N, dev)
        lab = label.to(dev, non_blocking=True).flatten()
        if self.binary:
            target.copy_(lab.view(-1, 1).to(torch.float32))
        else:
            target.zero_()
            target.scatter_(1, lab.to(torch.int64).view(-1, 1), 1.0)
        self._forward_and_append(st, target, patient_id)

    @torch.no_grad()
    def indexed(self, dataset, index, patient_id=None) -> None:
        """`__call__` from a device-resident dataset (device_data.DeviceDataset): one assembly launch (identity transform) into the plan's input
        and this step's target buffer; the mask goes to a scratch plane nothing reads."""
        st = self.model.compiled(len(index), dataset.H, dataset.W)
        dev = st.x.data.device
        target = self._target_buffer(st.N, dev)
        if self._scratch is None or self._scratch.shape != (st.N, 1, st.H, st.W) or self._scratch.device != dev:
            self._scratch = torch.empty(st.N, 1, st.H, st.W, dtype=torch.float32, device=dev)
        dataset.assemble(index, None, n_onehot=0 if self.binary else 3, out=(st.x.data, self._scratch, target))
        self._forward_and_append(st, target, patient_id)

    @torch.no_grad()
    def append_outputs(self, outputs: torch.Tensor, target: torch.Tensor, patient_id=None) -> None:
        """The one launch behind the forward, on (N, n) outputs and (N, n) targets that are already on the device (fp32, contiguous)."""
        import ctypes as C
        N, n = outputs.shape
        if outputs.dtype != torch.float32 or target.dtype != torch.float32 or not outputs.is_contiguous() or not target.is_contiguous() \
                or tuple(target.shape) != (N, n):
            raise ValueError("FusedClsTestStep: outputs and targets must be contiguous fp32 (N, n) tensors of one shape")
        self._buffers(outputs.device)
        a = L.ClsTestRowsArgs()
        a.cls_out, a.target, a.N, a.n_logits = outputs.data_ptr(), target.data_ptr(), N, n
        a.rows, a.state, a.capacity = self._rows.data_ptr(), self._state.data_ptr(), self.capacity
        L.check(L.load().mtbc_cls_test_rows(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cls_test_rows")
        first = len(self._ids)
        self._ids += list(range(first, first + N)) if patient_id is None else FusedTestStep._as_list(patient_id, N)

    def result(self) -> List[dict]:
        if self._state is None or not self._ids:
            raise L.MtbcError("FusedClsTestStep.result() before any batch was evaluated")
        err = self._coop_err
        flat = torch.cat([self._rows.flatten(), self._state, (err if err is not None else self._state[:1] * 0).to(torch.int32).flatten()]).cpu().numpy()
        if flat[-1] != 0:
            L.raise_coop_timeout()
        cursor, dropped = int(flat[-3]), int(flat[-2])
        if dropped or cursor > self.capacity or cursor != len(self._ids):
            raise L.MtbcError(f"classification test rows: {cursor} images since reset() but capacity = {self.capacity} rows ({dropped} batches dropped): "
                              f"build the FusedClsTestStep with a larger capacity")
        self.table = flat[:cursor * 2].reshape(cursor, 2).astype(np.int64)      # the integers behind the rows
        return cls_rows_from_table(self.table, self._ids)

    def write_csv(self, path: str, rows: Optional[List[dict]] = None) -> None:
        write_cls_rows_csv(path, self.result() if rows is None else rows)

    def report(self, rows: Optional[List[dict]] = None) -> Dict[str, float]:
        rows = self.result() if rows is None else rows
        return classification_report([r["ground_truth"] for r in rows], [r["predicted_label"] for r in rows],
                                     labels=(0, 1) if self.binary else (0, 1, 2))
