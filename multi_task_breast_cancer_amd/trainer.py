"""The optimisation step of src/training_multitask.py:87-103 as ONE stream-ordered program, plus the
data-parallel layer the reference does not have: one process per GPU, equal contiguous shards of a
single seeded global permutation, bucketed gradient all-reduce (RCCL over xGMI) overlapped with backward,
1/world folded into the fused Adam.

    zero_grad -> fwd -> Dice(4 heads, 1/(j+1)) + Focal -> alpha-mix -> bwd -> [all-reduce] -> Adam

No host synchronisation happens inside a step: the loss scalars and the NaN flag stay on the device
(`FusedTrainStep.losses`), to be read every k steps (the reference syncs 3+N times per step).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import os

import numpy as np
import torch

from . import _lib as L
from . import checkpoint as CK
from . import switches as _sw
from .criterions import exit_on_nan
from .loss_scale import betas_of
from .optim import FUSED_OPTIMIZERS


# ------------------------------------------------------------------------------------------------
# pure host logic (CPU-testable with gloo)
# ------------------------------------------------------------------------------------------------
@dataclass
class Bucket:
    start: int          # element range [start, end) of the flat gradient buffer
    end: int
    ready_op: int       # backward ops [0, ready_op] must have been issued before this bucket is reduced


def plan_buckets(slots: Sequence[Tuple[int, int, int]], flat_numel: int, n_buckets: int) -> List[Bucket]:
    """slots: (offset, numel, ready_at) per parameter in layout order.  Splits the flat buffer into
    `n_buckets` contiguous ranges of roughly equal size on parameter boundaries and returns them from the END of the
    buffer to its start: parameters are laid out in construction (= forward) order, so that is the order in which the
    backward pass finishes them, and -- unlike a sort by op index -- it is the same on every rank even when ranks
    build different step programs (the short last batch of an epoch): collectives must pair up.  A bucket whose
    `ready_op` lies behind its successor's only waits a little longer.  Ranges tile [0, flat_numel) exactly."""
    if not slots:
        return []
    n_buckets = max(1, min(n_buckets, len(slots)))
    cuts = [0]
    for i, (off, numel, _) in enumerate(slots):
        nxt = slots[i + 1][0] if i + 1 < len(slots) else flat_numel
        left = n_buckets - len(cuts)            # cuts still allowed after this bucket closes
        if left <= 0:
            break
        target = cuts[-1] + (flat_numel - cuts[-1]) / (left + 1)
        if nxt >= target and nxt < flat_numel:
            cuts.append(nxt)
    cuts.append(flat_numel)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b <= a:
            continue
        ready = max((r for off, numel, r in slots if a <= off < b), default=0)
        out.append(Bucket(a, b, ready))
    out.sort(key=lambda bk: -bk.start)
    return out


def plan_segments(buckets: Sequence[Bucket], n_bwd_ops: int) -> List[Tuple[int, int, Tuple[int, ...]]]:
    """Where the data-parallel step cuts its backward program of `n_bwd_ops` ops: (first, count, bucket indices) in issue order -- the ops
    [first, first + count) are issued, then the all-reduces of the named buckets (indices into `buckets`, in that order).  One entry per bucket,
    ending behind its `ready_op` (clamped to the program's end); a bucket whose `ready_op` has been passed already gets an EMPTY range (count 0):
    its all-reduce follows its predecessor's back to back.  Ops behind the last bucket form a closing entry without buckets.  The ranges tile
    [0, n_bwd_ops) in order and every bucket appears exactly once."""
    out, done = [], 0
    for i, b in enumerate(buckets):
        upto = max(done, min(n_bwd_ops, b.ready_op + 1))
        out.append((done, upto - done, (i,)))
        done = upto
    if done < n_bwd_ops or not out:
        out.append((done, n_bwd_ops - done, ()))
    return out


def shard_positions(positions: np.ndarray, rank: int, world: int, global_batch: int, step: int) -> np.ndarray:
    """Batch `step` of a global index list, cut into `world` equal contiguous shards: rank r takes
    rows [r*G/world, (r+1)*G/world) of the global batch, so the union over ranks IS the single-GPU batch."""
    if global_batch % world:
        raise ValueError("global batch must divide evenly across ranks")
    per = global_batch // world
    lo = step * global_batch + rank * per
    return positions[lo:lo + per]


def global_permutation(n: int, seed: int, epoch: int) -> np.ndarray:
    """One seeded permutation of the (oversampled) index list per epoch, identical on every rank."""
    return np.random.Generator(np.random.PCG64(seed * 1_000_003 + epoch)).permutation(n)


def allreduce_buckets(flat_g: torch.Tensor, buckets: Sequence[Bucket], group=None, async_op: bool = False):
    """Sum-all-reduce every bucket of the flat gradient buffer (averaging = grad_scale 1/world in Adam)."""
    import torch.distributed as dist
    works = []
    for b in buckets:
        w = dist.all_reduce(flat_g[b.start:b.end], op=dist.ReduceOp.SUM, group=group, async_op=async_op)
        if async_op:
            works.append(w)
    return works


# ---- training-time metrics (training_multitask.py:105-113) from the integer counts of mtbc_train_metrics: pure functions of (table, conf)
class TrainMetrics(NamedTuple):
    dice: float             # mean over the batches of the per-batch Dice (`training_dice / len(training_loader)`, :111)
    accuracy: float         # accuracy_score over every sample of the epoch (:112)
    f1: float               # f1_score(labels=[0, 1, 2], average='weighted') (:113)
    batches: int
    conf: np.ndarray        # (3, 3) int64, rows = ground truth, cols = prediction
    table: np.ndarray       # (batches, 4) int64: tp, fp, fn, samples of each (global) batch


def _dice(tp: float, fp: float, fn: float) -> float:
    """metrics.py:255-267 on float64 counts: an empty ground truth scores 1 with an empty prediction, else 0."""
    if tp + fn == 0:
        return 1.0 if tp + fp == 0 else 0.0
    return 2 * tp / (2 * tp + fp + fn)


def classification_scores(conf: np.ndarray) -> Tuple[float, float]:
    """(accuracy_score, f1_score(labels=[0, 1, 2], average='weighted')) of a float64 3 x 3 confusion matrix, rows = ground truth
    (training_multitask.py:112-113, :155-156): per-class F1 weighted by support; a class with no support has weight 0, one that is never
    predicted scores 0."""
    total = conf.sum()
    accuracy = float(np.trace(conf) / total) if total else 0.0
    support = conf.sum(axis=1)
    tp = np.diag(conf)
    denom = conf.sum(axis=0) + support
    f1c = np.divide(2 * tp, denom, out=np.zeros_like(tp), where=denom > 0)
    f1w = float((f1c * support).sum() / support.sum()) if support.sum() else 0.0
    return accuracy, f1w


def cls_driver_scores(conf: np.ndarray, binary: bool) -> Tuple[float, float]:
    """(accuracy, F1) as the classification driver computes them (training_classification.py:88-96, :152-160) from a float64 3 x 3 confusion
    matrix, rows = ground truth.  Three classes: sklearn's accuracy_score and f1_score(labels=[0, 1, 2], average='micro') -- precision and recall
    over the summed counts, 0 on an empty matrix.  Binary head: `accuracy_from_tensor` / `f1_score_from_tensor` (metrics.py:270-286) on the
    {0, 1} labels -- (tp + tn) / total and 2 tp / (2 tp + fp + fn), NaN on 0 / 0 as the reference's tensor division gives."""
    conf = np.asarray(conf, dtype=np.float64).reshape(3, 3)
    if binary:
        tn, fp, fn, tp = conf[0, 0], conf[0, 1], conf[1, 0], conf[1, 1]
        total, den = tp + tn + fp + fn, 2 * tp + fp + fn
        return (float((tp + tn) / total) if total else float("nan")), (float(2 * tp / den) if den else float("nan"))
    total, tp = conf.sum(), np.trace(conf)
    accuracy = float(tp / total) if total else 0.0
    precision = tp / conf.sum(axis=0).sum() if total else 0.0
    recall = tp / conf.sum(axis=1).sum() if total else 0.0
    f1 = float(2 * precision * recall / (precision + recall)) if precision + recall else 0.0
    return accuracy, f1


def train_metrics_from_counts(table, conf) -> TrainMetrics:
    """The reference's training-time metrics from the rows the device appended: `table` (batches, 4) = tp, fp, fn, samples per batch,
    `conf` (3, 3).  Dice: the per-batch score of `dice_score_from_tensor`, summed in batch order in float64 and divided by the number of
    batches, as the reference's `training_dice += ...; training_dice / len(training_loader)`."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
    total = 0.0
    for tp, fp, fn, _ in table.tolist():
        total += _dice(float(tp), float(fp), float(fn))
    accuracy, f1w = classification_scores(conf.astype(np.float64))
    return TrainMetrics(total / len(table) if len(table) else 0.0, accuracy, f1w, len(table), conf, table)


# ---- the device metrics table's way to the host, shared by training (mtbc_train_metrics) and validation (mtbc_eval_metrics): one pack, one decode
# the words in which each flavour's refusals speak
_TRAIN = {"kind": "training", "owner": "FusedTrainStep", "cap": "metrics_capacity", "since": "begin_epoch_metrics()", "per_batch": "call run() or run_empty()"}
_EVAL = {"kind": "validation", "owner": "FusedEvalStep", "cap": "capacity", "since": "reset()", "per_batch": "evaluate its shard or call run_empty()"}


def _reduce_packed(table: torch.Tensor, conf: torch.Tensor, state: torch.Tensor, loss_rows: Optional[torch.Tensor] = None,
                   coop_err: Optional[torch.Tensor] = None, distributed: bool = False, group=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """One rank's accumulators -> the int64 host array [table | conf | sum cursor, sum cursor^2, sum dropped] and, with `loss_rows` (validation), a
    fourth word -- the cooperative-kernel error word -- and the float64 host array [loss_rows]: each array with, under `distributed`, ONE
    sum-all-reduce in front of its ONE device-to-host read.  The accumulators themselves are not modified (the sums work on copies)."""
    s = state.to(torch.int64)
    words = [s[0], s[0] * s[0], s[1]]
    losses = None
    if loss_rows is not None:
        words.append(s[0] * 0 if coop_err is None else (coop_err.reshape(-1)[0] != 0).to(torch.int64))
        losses = loss_rows.reshape(-1)
    packed = torch.cat([table.reshape(-1), conf.reshape(-1), torch.stack(words)])
    if distributed:
        import torch.distributed as dist
        if losses is not None:
            losses = losses.clone()
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
        if losses is not None:
            dist.all_reduce(losses, op=dist.ReduceOp.SUM, group=group)
    return packed.cpu().numpy(), None if losses is None else losses.cpu().numpy()


def _decode_packed(packed: np.ndarray, capacity: int, world: int, f: dict) -> Tuple[np.ndarray, np.ndarray]:
    """The int64 array of `_reduce_packed` -> (the appended rows (batches, 4), conf (3, 3)), or MtbcError (and no number) when a batch found the table
    full or the ranks did not see the same number of batches.  Every rank holds the same sums, so every rank raises or none does."""
    c_sum, c_sq, dropped = (int(v) for v in packed[capacity * 4 + 9:capacity * 4 + 12])
    if world * c_sq != c_sum * c_sum:              # Cauchy-Schwarz: equality only when all cursors are equal
        raise L.MtbcError(f"{f['kind']} metrics: the ranks appended different numbers of batches (sum {c_sum} over {world} ranks): every rank must "
                          f"{f['per_batch']} once per global batch; rows of the {f['cap']} = {capacity} table do not line up")
    cursor = c_sum // world
    if dropped != 0 or cursor > capacity:
        raise L.MtbcError(f"{f['kind']} metrics: {cursor} batches since {f['since']} but {f['cap']} = {capacity} rows "
                          f"({dropped} dropped): build the {f['owner']} with a larger {f['cap']}")
    return packed[:cursor * 4].reshape(cursor, 4), packed[capacity * 4:capacity * 4 + 9].reshape(3, 3)


def reduce_train_metrics(table: torch.Tensor, conf: torch.Tensor, state: torch.Tensor, distributed: bool = False, group=None) -> np.ndarray:
    """`_reduce_packed` for training: ONE int64 host array [table | conf | sum cursor, sum cursor^2, sum dropped].  The ranks' shards of global
    batch b all sit in row b, so the summed row holds the GLOBAL batch's tp / fp / fn: the Dice of the union, not a mean of shard Dices."""
    return _reduce_packed(table, conf, state, distributed=distributed, group=group)[0]


def train_metrics_from_packed(packed: np.ndarray, capacity: int, world: int = 1) -> TrainMetrics:
    """`reduce_train_metrics`' array -> TrainMetrics, or the MtbcError of `_decode_packed`."""
    return train_metrics_from_counts(*_decode_packed(packed, capacity, world, _TRAIN))


# ---- the validation epoch (training_multitask.py:119-159) from what mtbc_eval_metrics appended: pure functions of (table, conf, loss_rows)
def eval_result_from_counts(table, conf, loss_rows) -> tuple:
    """The reference's 6-tuple (avg_val_loss, avg_val_dice, val_acc, val_f1, avg_seg_val_loss, avg_cls_val_loss) from one row per (global) batch:
    `table` (batches, 4) = tp, fp, fn, samples, `conf` (3, 3), `loss_rows` (batches, 4) float64 = total, seg, cls, NaN word.  Losses: summed in row
    order in float64 and divided by the number of rows -- `val_loss += total_loss.item()` ... `/ len(val_loader)` (:141-153); Dice: `_dice` per row,
    summed in order, divided likewise (:140, :154).  A non-zero NaN word in any row ends the run as the reference's criterion wrapper does in
    validation too (criterions.py:72-76): log + exit(1)."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
    loss_rows = np.asarray(loss_rows, dtype=np.float64).reshape(-1, 4)
    if len(loss_rows) != len(table):
        raise ValueError(f"{len(table)} count rows but {len(loss_rows)} loss rows")
    total = seg = cls = dice = 0.0
    nan = False
    for (tp, fp, fn, _), (lt, ls, lc, flag) in zip(table.tolist(), loss_rows.tolist()):
        total += lt
        seg += ls
        cls += lc
        dice += _dice(float(tp), float(fp), float(fn))
        nan = nan or flag != 0.0
    if nan:
        exit_on_nan()
    nb = len(table)
    accuracy, f1w = classification_scores(conf.astype(np.float64))
    if nb == 0:
        return 0.0, 0.0, accuracy, f1w, 0.0, 0.0
    return total / nb, dice / nb, accuracy, f1w, seg / nb, cls / nb


def cls_eval_result_from_counts(table, conf, loss_rows, binary: bool) -> tuple:
    """The classification driver's (val_loss, val_acc, val_f1) (training_classification.py:149-162) from one row per batch: the loss words' first
    column summed in row order in float64 and divided by the number of rows, `cls_driver_scores` of the confusion matrix; a NaN word ends the run."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    loss_rows = np.asarray(loss_rows, dtype=np.float64).reshape(-1, 4)
    if len(loss_rows) != len(table):
        raise ValueError(f"{len(table)} count rows but {len(loss_rows)} loss rows")
    total = 0.0
    for lt, _, _, flag in loss_rows.tolist():
        total += lt
        if flag != 0.0:
            exit_on_nan()
    accuracy, f1 = cls_driver_scores(conf, binary)
    return (total / len(table) if len(table) else 0.0), accuracy, f1


def reduce_eval_metrics(table: torch.Tensor, conf: torch.Tensor, state: torch.Tensor, loss_rows: torch.Tensor, coop_err: Optional[torch.Tensor] = None,
                        distributed: bool = False, group=None) -> Tuple[np.ndarray, np.ndarray]:
    """`_reduce_packed` for validation: TWO host arrays, int64 [table | conf | sum cursor, sum cursor^2, sum dropped, sum coop error word] and float64
    [loss_rows].  The ranks' shards of global batch b sit in row b on every rank: the summed integer row is the global batch's counts exactly, the
    summed loss row -- each rank's words carry its share n_local / n_batch -- the global batch's mean losses."""
    return _reduce_packed(table, conf, state, loss_rows, coop_err, distributed=distributed, group=group)


def eval_result_from_packed(packed: np.ndarray, losses: np.ndarray, capacity: int, world: int = 1, cls_only: Optional[bool] = None) -> tuple:
    """`reduce_eval_metrics`' arrays -> the 6-tuple, or MtbcError (and no number) when a cooperative kernel failed on some rank, or by the rule of
    `_decode_packed`.  Every rank holds the same sums, so every rank raises (or exits on a NaN word) or none does.  `cls_only` (the head is
    binary: True / False): the classification driver's 3-tuple of `cls_eval_result_from_counts` instead."""
    if int(packed[capacity * 4 + 12]) != 0:
        L.raise_coop_timeout()
    table, conf = _decode_packed(packed, capacity, world, _EVAL)
    if len(table) == 0:
        raise L.MtbcError("FusedEvalStep.result() before any batch was evaluated")
    if cls_only is not None:
        return cls_eval_result_from_counts(table, conf, np.asarray(losses, dtype=np.float64)[:len(table) * 4].reshape(len(table), 4), cls_only)
    return eval_result_from_counts(table, conf, np.asarray(losses, dtype=np.float64)[:len(table) * 4].reshape(len(table), 4))


# ------------------------------------------------------------------------------------------------
# the fused step (HIP)
# ------------------------------------------------------------------------------------------------
def _check_seg_criterion(name: str, distributed: bool) -> str:
    if name not in L.SEG_CRITERIA:
        raise ValueError(f"unknown segmentation criterion {name!r} ({' | '.join(L.SEG_CRITERIA)}; the other `loss.function` names of the "
                         f"reference are not on HIP)")
    if distributed and L.SEG_CRITERIA[name][4]:
        # the shard-weight mechanism makes the all-reduced gradient that of the global batch for a MEAN over the batch (weight = n_local / n_batch
        # times world, then 1 / world); a SUM over the batch would need the factor 1 / world undone, i.e. a factor that depends on each step's
        # global batch, which the ranks' step programs do not carry
        raise NotImplementedError(f"seg_criterion={name!r} sums over the batch (reduction='sum'): the data-parallel step averages the ranks' gradients, "
                                  f"which is exact for a mean over the batch only -- train it on one device, or use a mean criterion")
    return name


def _check_heads(model, n_classes: int, cls_criterion: str, focal_weight, owner: str) -> tuple:
    """What FusedTrainStep and FusedEvalStep both require of the classification head and its criterion -> (binary, cls_gamma, focal_weight)."""
    if n_classes > 3:       # the confusion matrix is the reference's 3 x 3 (f1_score(labels=[0, 1, 2]), training_multitask.py:155)
        raise NotImplementedError(f"{owner} covers the reference's label set {{0, 1, 2}} (n_classes <= 3)")
    binary = n_classes == 2
    if binary != (getattr(model, "n_classes", n_classes) == 1):
        raise ValueError("n_classes does not match the model's classification head (n_classes == 2 <=> ONE logit)")
    if cls_criterion not in ("Focal", "CE"):
        raise ValueError(f"unknown classification criterion {cls_criterion!r} (Focal | CE; the binary head always takes BCEWithLogits)")
    if cls_criterion == "CE" and focal_weight is not None:
        # torch.nn.CrossEntropyLoss(weight=w) divides by the sum of the samples' weights; FocalLoss (criterions.py:14-24) by N
        raise NotImplementedError("class-weighted CrossEntropyLoss normalises by the weights' sum: use the drop-in loop for it")
    return binary, 2.0 if cls_criterion == "Focal" else 0.0, None if binary else focal_weight


def is_seg_only(model) -> bool:
    """A single-task segmentation model (nets.nnUNet, nets.BasicUnetPlusPlus): no classification head, no class logits anywhere in its plans."""
    return getattr(model, "n_classes", None) == 0


def _check_seg_only(alpha, n_classes, focal_weight, cls_criterion, distributed: bool, owner: str) -> None:
    """What FusedTrainStep and FusedEvalStep refuse of a segmentation-only model (training_segmentation.py has no class label, no mix)."""
    if alpha is not None and float(alpha) != 1.0:
        raise ValueError(f"{owner}: a segmentation-only model has no classification loss to mix: alpha must be 1.0, got {alpha}")
    passed = [k for k, v in (("n_classes", n_classes), ("focal_weight", focal_weight), ("cls_criterion", cls_criterion)) if v is not None]
    if passed:
        raise ValueError(f"{owner}: {', '.join(passed)} given, but the model has no classification head")
    if distributed:
        raise NotImplementedError(f"{owner}: data parallel is not built for segmentation-only models yet")


def _check_single_device(model, distributed: bool, owner: str) -> None:
    """A model whose data-parallel step is not built or tested (nets.Multi_BTSUNet) refuses distributed=True, as the single-task models do."""
    if distributed and getattr(model, "single_device_only", False):
        raise NotImplementedError(f"{owner}: data parallel is not built for {getattr(model, 'architecture', type(model).__name__)} yet")


def is_cls_only(model) -> bool:
    """A single-task classification model (nets.nnUNetClassifier, nets.UNetPlusPlusClassifier): no segmentation head anywhere in its plans."""
    return bool(getattr(model, "cls_only", False))


def _check_cls_only(alpha, inversely_weighted, seg_criterion, distributed: bool, owner: str) -> None:
    """What FusedTrainStep and FusedEvalStep refuse of a classification-only model (training_classification.py has no mask, no mix)."""
    if alpha is not None and float(alpha) != 0.0:
        raise ValueError(f"{owner}: a classification-only model has no segmentation loss to mix: alpha must be None or 0.0, got {alpha}")
    passed = [k for k, v in (("inversely_weighted", inversely_weighted), ("seg_criterion", seg_criterion)) if v is not None]
    if passed:
        raise ValueError(f"{owner}: {', '.join(passed)} given, but the model has no segmentation head")
    if distributed:
        raise NotImplementedError(f"{owner}: data parallel is not built for classification-only models yet")


class ClsTrainMetrics(NamedTuple):
    """`epoch_metrics()` of a classification-only training step: the driver's (loss, acc, f1) first (training_classification.py:98)."""
    loss: float             # mean over the batches of the step's loss
    accuracy: float
    f1: float               # micro over labels [0, 1, 2]; the binary head: 2 tp / (2 tp + fp + fn)
    batches: int
    conf: np.ndarray        # (3, 3) int64, rows = ground truth, cols = prediction


class SegTrainMetrics(NamedTuple):
    """`epoch_metrics()` of a segmentation-only training step: the driver's (loss, dice) first (training_segmentation.py:59-62)."""
    loss: float             # mean over the batches of the step's loss
    dice: float             # mean over the batches of the per-batch Dice
    batches: int
    table: np.ndarray       # (batches, 4) int64: tp, fp, fn, samples of each batch


# ---- the task of a model, decided once: everything the multi-task, the segmentation and the classification driver do differently, as data
@dataclass(frozen=True)
class Task:
    name: str                           # as the refusals say it: "a {name}-only model"
    seg: bool                           # a segmentation head: batches carry a mask, the metrics call fills the Dice rows
    cls: bool                           # a classification head: batches carry a label, the metrics call fills the confusion matrix
    metrics_fn: Tuple[str, str]         # the metrics entry point of _lib (training, validation); L.check is told the name without its prefix
    metrics_args: Tuple[type, type]     # its argument struct (training, validation)
    cls_field: Optional[str]            # that struct's name for the class output
    scores: Callable                    # (float64 confusion matrix, binary) -> (accuracy, F1) as this driver computes them
    epoch_metrics: Callable             # (TrainMetrics, mean loss of the steps, binary) -> what FusedTrainStep.epoch_metrics() returns
    train_fields: Tuple[str, ...]       # the fields of that result behind the loss in the training epoch's tuple
    val_fields: Tuple[str, ...]         # the validation epoch's tuple, out of loss, dice, accuracy, f1, seg_loss, cls_loss
    header: str                         # metrics.csv: its header, the formatter of a row and the row's values, out of epoch, lr, test_dice,
    row: Callable                       # train_loss, train_<train_fields> and val_<val_fields>
    row_fields: Tuple[str, ...]
    log: str                            # the epoch's log line over the same names plus patience, epoch_time and best
    lr_at_start: bool                   # the row's learning rate is read before the epoch (else behind the scheduler step)
    tests_every_epoch: bool             # fit_fold runs a testing phase behind every epoch and writes its mean DICE into the row

    @property
    def single(self) -> bool:
        return not (self.seg and self.cls)

    @property
    def batch_fields(self) -> Tuple[str, ...]:
        """What a batch dict of this driver's loader carries beside the image, in the order the steps take it."""
        return tuple(k for k, has in (("mask", self.seg), ("label", self.cls)) if has)


def _cls_epoch_metrics(m: TrainMetrics, loss: float, binary: bool) -> ClsTrainMetrics:
    accuracy, f1 = cls_driver_scores(m.conf, binary)
    return ClsTrainMetrics(loss, accuracy, f1, m.batches, m.conf)


MULTI_TASK = Task(          # training_multitask.py
    "multi-task", True, True, ("mtbc_train_metrics", "mtbc_eval_metrics"), (L.TrainMetricsArgs, L.EvalMetricsArgs), "cls_logits",
    scores=lambda conf, binary: classification_scores(conf), epoch_metrics=lambda m, loss, binary: m,
    train_fields=("dice", "accuracy", "f1"), val_fields=("loss", "dice", "accuracy", "f1", "seg_loss", "cls_loss"),
    header=CK.METRICS_HEADER, row=CK.metrics_row,
    row_fields=("epoch", "lr", "train_loss", "val_loss", "train_dice", "val_dice", "train_accuracy", "train_f1", "val_accuracy", "val_f1"),
    log="EPOCH {epoch} --> || Training loss {train_loss:.4f} || Validation loss {val_loss:.4f} || Segmentation val loss {val_seg_loss:.4f} "
        "|| Classification val loss {val_cls_loss:.4f} || Training DICE {train_dice:.4f} || Validation DICE  {val_dice:.4f} "
        "|| Training ACC {train_accuracy:.4f} || Training F1 {train_f1:.4f} || Validation ACC {val_accuracy:.4f} || Validation F1 {val_f1:.4f} "
        "|| Patience: {patience} || Epoch time: {epoch_time:.4f}|| Best validation performance: {best:.4f}",
    lr_at_start=True, tests_every_epoch=False)
SEGMENTATION = Task(        # training_segmentation.py: the confusion matrix stays zero, the struct has neither `conf` nor `n_logits`
    "segmentation", True, False, ("mtbc_seg_step_metrics",) * 2, (L.SegStepMetricsArgs,) * 2, None,
    scores=MULTI_TASK.scores, epoch_metrics=lambda m, loss, binary: SegTrainMetrics(loss, m.dice, m.batches, m.table),
    train_fields=("dice",), val_fields=("loss", "dice"), header=CK.SEG_METRICS_HEADER, row=CK.seg_metrics_row,
    row_fields=("epoch", "lr", "train_dice", "val_dice", "test_dice", "train_loss", "val_loss"),
    log="EPOCH {epoch} --> || Training loss {train_loss:.4f} || Validation loss {val_loss:.4f} || Training DICE {train_dice:.4f} "
        "|| Validation DICE  {val_dice:.4f} || Patience: {patience} || Epoch time: {epoch_time:.4f} || LR: {lr:.8f}",
    lr_at_start=False, tests_every_epoch=True)
CLASSIFICATION = Task(      # training_classification.py: the samples launch alone, tp / fp / fn stay zero; the struct reads the model's OUTPUT
    "classification", False, True, ("mtbc_cls_step_metrics",) * 2, (L.ClsStepMetricsArgs,) * 2, "cls_out",
    scores=cls_driver_scores, epoch_metrics=_cls_epoch_metrics,
    train_fields=("accuracy", "f1"), val_fields=("loss", "accuracy", "f1"), header=CK.CLS_METRICS_HEADER, row=CK.cls_metrics_row,
    row_fields=("epoch", "lr", "train_loss", "val_loss", "train_accuracy", "train_f1", "val_accuracy", "val_f1"),
    log="EPOCH {epoch} --> || Training loss {train_loss:.4f} || Validation loss {val_loss:.4f} || Training ACC {train_accuracy:.4f} "
        "|| Training F1 {train_f1:.4f} || Validation ACC {val_accuracy:.4f} || Validation F1 {val_f1:.4f} || Patience: {patience} "
        "|| Epoch time: {epoch_time:.4f}",
    lr_at_start=True, tests_every_epoch=False)


def task_of(model) -> Task:
    return CLASSIFICATION if is_cls_only(model) else SEGMENTATION if is_seg_only(model) else MULTI_TASK


def step_task(step) -> Task:
    """The task of a training, evaluation or test step by its public attributes; an object without them (a stand-in) is multi-task."""
    return CLASSIFICATION if getattr(step, "cls_only", False) else SEGMENTATION if getattr(step, "seg_only", False) else MULTI_TASK


def _resolve_step(model, owner: str, cls_name: str, distributed: bool, alpha, inversely_weighted, n_classes, focal_weight, cls_criterion,
                  seg_criterion, before_criterion: Callable = lambda: None) -> tuple:
    """The prologue FusedTrainStep and FusedEvalStep share -> (task, alpha, inversely_weighted, n_classes, seg_criterion, binary, cls_gamma,
    focal_weight).  None = "not given": alpha is required, n_classes defaults to 3 and cls_criterion to "Focal" for a model with a classification
    head, and not given is all a segmentation-only model accepts; inversely_weighted (default True) and seg_criterion (default "DICE") likewise,
    and not given is all a classification-only model accepts.  `before_criterion`: the caller's own refusals that come in front of the criterion's."""
    task = task_of(model)
    _check_single_device(model, distributed, owner)
    if not task.seg:
        _check_cls_only(alpha, inversely_weighted, seg_criterion, distributed, owner)
        alpha = 0.0
    inversely_weighted = True if inversely_weighted is None else inversely_weighted
    seg_criterion = "DICE" if seg_criterion is None else seg_criterion
    if not task.cls:
        _check_seg_only(alpha, n_classes, focal_weight, cls_criterion, distributed, owner)
        alpha = 1.0
    else:
        if alpha is None:
            raise TypeError(f"{cls_name}: alpha (the weight of the segmentation loss in the mix) is required for a multi-task model")
        n_classes = 3 if n_classes is None else n_classes
        cls_criterion = "Focal" if cls_criterion is None else cls_criterion
    before_criterion()
    # seg_criterion: the reference's `loss.function` (experiment_init.py:199-232) -- "DICE" | "BCE" | "FocalDICE" | "Jaccard", all in the same
    # two loss ops of the step program (mtbc_dice_args.kind); the remaining names are not on HIP (experiment_init.init_criterion_segmentation).
    seg_criterion = _check_seg_criterion(seg_criterion, distributed)
    heads = _check_heads(model, n_classes, cls_criterion, focal_weight, owner) if task.cls else (False, 2.0, None)
    return (task, float(alpha), bool(inversely_weighted), n_classes, seg_criterion) + heads


def _n_onehot(step) -> int:
    """The width of the one-hot class target the batch-assembly launch writes: none for the binary head (the label itself) or without a head."""
    return 0 if step.binary or not step.task.cls else 3


def _fused_loss(step) -> dict:
    """The `fused_loss` settings a step compiles its plan with.  A training and an evaluation step with the same (alpha, weighting, criteria) build
    equal dicts and so share one compiled plan at equal (N, H, W); only a dynamic loss scale adds a key."""
    d = {"alpha": step.alpha, "inversely_weighted": step.iw, "focal_weight": step.focal_weight, "binary": step.binary,
         "cls_gamma": step.cls_gamma, "seg_criterion": step.seg_criterion}
    if getattr(step, "scaler", None) is not None:
        d["loss_scale"] = 1.0
    return d


def _check_in_channels(model, dataset) -> None:
    if model.in_channels != 1 + dataset.n_augments:
        raise ValueError(f"the model reads {model.in_channels} input channels, the dataset gives 1 + {dataset.n_augments}: build the model with "
                         f"sequences + dataset.n_augments (experiment_init.load_multitask_experiment_artefacts(n_augments=...))")


def fill_batch(st, image: torch.Tensor, mask: torch.Tensor, label: Optional[torch.Tensor], binary: bool) -> None:
    """H2D / D2D of training_multitask.py:82-84 into the plan's static buffers; the class target is built on the device: the one-hot rows, or, for
    the binary head, the (N, 1) float label itself (the target of the one-logit criterion).  A segmentation-only plan has no class target and
    takes no label (training_segmentation.py:36-37)."""
    if (st.onehot is None) != (label is None):
        raise ValueError("a class label was given to a segmentation-only model" if label is not None else
                         "this model has a classification head: the batch needs its class labels")
    st.x.data.copy_(image, non_blocking=True)
    if st.mask is not None:                 # a classification-only plan reads no mask (training_classification.py:41)
        st.mask.copy_(mask, non_blocking=True)
    elif mask is not None:
        raise ValueError("a mask was given to a classification-only model")
    if label is None:
        return
    lab = label.to(st.onehot.device, non_blocking=True).flatten()
    if binary:
        st.onehot.copy_(lab.view(-1, 1).to(torch.float32))
    else:
        st.onehot.zero_()
        st.onehot.scatter_(1, lab.to(torch.int64).view(-1, 1), 1.0)


def _target_of(step, st) -> torch.Tensor:
    """The class-target buffer the batch-assembly launch writes: the plan's, or -- a segmentation-only plan has none, the launch always
    writes one -- an (N, 1) scratch of the step's that nothing reads."""
    if st.onehot is not None:
        return st.onehot
    t = step._scratch_target
    if t is None or t.shape[0] != st.N or t.device != st.mask.device:
        step._scratch_target = t = torch.empty(st.N, 1, dtype=torch.float32, device=st.mask.device)
    return t


def _mask_of(step, st) -> torch.Tensor:
    """The mask buffer the batch-assembly launch writes (it refuses a NULL out_mask): the plan's, or -- a classification-only plan has none --
    an (N, 1, H, W) scratch plane of the step's that nothing reads."""
    if st.mask is not None:
        return st.mask
    t = step._scratch_mask
    if t is None or t.shape != (st.N, 1, st.H, st.W) or t.device != st.x.data.device:
        step._scratch_mask = t = torch.empty(st.N, 1, st.H, st.W, dtype=torch.float32, device=st.x.data.device)
    return t


def _capture(body, error_mode: str = "global"):
    """`body`'s launches as ONE hipGraph, captured on a fresh side stream that joins the current one on both sides.  `error_mode`: torch's
    capture_error_mode ("global", its default, for every single-device capture)."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode=error_mode):
        body()
    cur.wait_stream(side)
    return g


def _capture_segment(body):
    """`_capture` for one segment of the data-parallel step.  A process group is alive beside these captures, and its watchdog thread polls events of
    earlier collectives whenever it likes: under the global mode such a call from ANOTHER thread invalidates a capture in flight.  The thread-local mode
    still refuses every unsafe call of the capturing thread itself, which is all a segment body could get wrong."""
    return _capture(body, error_mode="thread_local")


def run_or_replay(owner, st, key, body, capture=_capture) -> None:
    """`body` (a static list of launches on the compiled step `st`) as a hipGraph replay: eager for the first two calls of a compiled step (lazily
    created buffers, kernel attributes), captured at the third, replayed afterwards.  A graph holds addresses: `key` names what it depends on, and
    a changed key drops it.  The entry [key, eager calls, graph] lives ON the compiled step under id(owner) -- a dropped step takes its graph along
    (no address or id() can be reused under a stale graph), and two steps that share a plan keep a graph each -- and is mirrored in
    owner._graphs[id(st)] for tests and tools."""
    ents = st.__dict__.setdefault("_graph_ents", {})
    ent = ents.get(id(owner))
    if ent is None or ent[0] != key:
        ents[id(owner)] = ent = [key, 0, None]
    owner._graphs[id(st)] = ent
    if ent[2] is None and ent[1] >= 2:
        ent[2] = capture(body)
    if ent[2] is not None:
        ent[2].replay()
    else:
        ent[1] += 1
        body()


class SegmentGraphs:
    """The hipGraphs of one compiled step replayed in segments (`run_or_replay_segments`), in issue order: ONE object in the entry's graph slot."""

    def __init__(self, graphs):
        self.graphs = list(graphs)

    def __len__(self) -> int:
        return len(self.graphs)


def run_or_replay_segments(owner, st, key, bodies, between, capture=_capture_segment, quiesce=None) -> None:
    """`run_or_replay` for a step that is a LIST of static bodies with eager work between them (the data-parallel step: the bucket all-reduces stay
    with the host): `between(i)` runs right behind segment i, exactly once per segment per call, whether segment i ran eager or as a replay.  The
    same entry [key, eager calls, graph] in the same two places; the graph slot holds one SegmentGraphs.  Eager for the first two calls; the third
    calls `quiesce()` (nothing of an earlier step may still be in flight on another stream of ours while a capture is open), captures EVERY body --
    a capture executes nothing, so no `between` is due yet -- and then replays like every later call."""
    ents = st.__dict__.setdefault("_graph_ents", {})
    ent = ents.get(id(owner))
    if ent is None or ent[0] != key:
        ents[id(owner)] = ent = [key, 0, None]
    owner._graphs[id(st)] = ent
    if ent[2] is None and ent[1] >= 2:
        if quiesce is not None:
            quiesce()
        ent[2] = SegmentGraphs(capture(body) for body in bodies)
    if ent[2] is not None:
        for i, g in enumerate(ent[2].graphs):
            g.replay()
            between(i)
    else:
        ent[1] += 1
        for i, body in enumerate(bodies):
            body()
            between(i)


class MetricsTable:
    """The device accumulator behind `mtbc_train_metrics` and, with `validation`, `mtbc_eval_metrics`: `counts` int64 [capacity * 4 + 9] --
    one row tp, fp, fn, samples per batch, then the 3 x 3 confusion matrix -- and `state` int32 [2] = cursor, dropped; for validation also
    `loss_rows` float64 [capacity][4] = (weighted) total, seg, cls, NaN word of each batch and `weight` float32 [1], this rank's share of the batch in
    flight (read by the kernel under `distributed` only).  Allocated at first use, once, and never moved: captured graphs hold the addresses."""

    def __init__(self, model, capacity: int, validation: bool = False, distributed: bool = False):
        self.model, self.capacity, self.eval, self.distributed = model, int(capacity), bool(validation), bool(distributed)
        self.words = _EVAL if self.eval else _TRAIN
        self.task = task_of(model)
        self.entry = self.task.metrics_fn[self.eval]     # the metrics call of _lib; L.check is told its name without the prefix
        self.label = self.entry[len("mtbc_"):]
        self.counts = self.state = self.loss_rows = self.weight = None
        self._args = {}             # id(compiled step) -> (the step, its argument struct, the entry point); None -> the empty shard's

    def buffers(self) -> "MetricsTable":
        if self.counts is None:
            dev = next(self.model.parameters()).device
            self.counts = torch.zeros(self.capacity * 4 + 9, dtype=torch.int64, device=dev)
            self.state = torch.zeros(2, dtype=torch.int32, device=dev)
            if self.eval:
                self.loss_rows = torch.zeros(self.capacity, 4, dtype=torch.float64, device=dev)
                self.weight = torch.ones(1, dtype=torch.float32, device=dev)
        return self

    def zero(self) -> None:
        """Rows, confusion matrix and cursor back to zero in stream order (outside any replayed graph: the buffers stay where they are)."""
        for t in (self.counts, self.state, self.loss_rows):
            if t is not None:
                t.zero_()

    def _arguments(self, st, n_logits):
        """The argument struct of one compiled step (st = None: of the empty shard, N = 0), which never changes: outputs and accumulators stay where
        they are.  Behind the loss program the plan's buffers hold fp32 NCHW logits of the last head, the mask, the class output and its target,
        in every compute mode; the struct carries the pair of each head the task has, and `loss_in` stays NULL for training."""
        self.buffers()
        task = self.task
        a = task.metrics_args[self.eval]()
        seg = cls = None
        if st is not None:
            seg = (st.segs[-1].data, st.mask) if task.seg else None
            cls = (st.logits.data, st.onehot) if task.cls else None
            pairs = [p for p in (seg, cls) if p is not None]
            loss_out = (st.plan.loss_out,) if self.eval else ()
            for t in (*(t for p in pairs for t in p), *loss_out):
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise L.MtbcError(f"{self.words['kind']} metrics: the step's outputs are not contiguous fp32 buffers")
            if any(x.numel() != y.numel() for x, y in pairs) or any(t.numel() < 4 for t in loss_out):
                raise L.MtbcError(f"{self.words['kind']} metrics: outputs and targets differ in size")
            a.N = st.N
            if self.eval:
                a.loss_in = st.plan.loss_out.data_ptr()
        if seg is not None:
            a.seg_logits, a.mask, a.n_seg = seg[0].data_ptr(), seg[1].data_ptr(), seg[0].numel()
        if task.cls:
            a.n_logits, a.conf = n_logits if st is None else st.logits.C, self.counts.data_ptr() + self.capacity * 32
            if cls is not None:
                setattr(a, task.cls_field, cls[0].data_ptr())
                a.target = cls[1].data_ptr()
        a.table, a.state, a.capacity = self.counts.data_ptr(), self.state.data_ptr(), self.capacity
        if self.eval:
            a.loss_rows = self.loss_rows.data_ptr()
            a.shard_weight = self.weight.data_ptr() if self.distributed else None
        return a

    def append(self, st, n_logits: int = 0) -> None:
        """The metrics call on the outputs (validation: and the loss words) of the step program that has just run; st = None: the empty shard, which
        only advances the cursor (`n_logits` = the head's width).  Two launches on the current stream, capturable."""
        import ctypes as C
        key = None if st is None else id(st)
        ent = self._args.get(key)
        if ent is None or ent[0] is not st:
            self._args[key] = ent = (st, self._arguments(st, n_logits), getattr(L.load(), self.entry))
        L.check(ent[2](C.byref(ent[1]), C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.label)

    def reduce(self, coop_err: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """`_reduce_packed` of these buffers: under `distributed` one sum-all-reduce per array (row b of the sum is GLOBAL batch b), one read each."""
        cap = self.capacity
        return _reduce_packed(self.counts[:cap * 4], self.counts[cap * 4:], self.state, self.loss_rows, coop_err, distributed=self.distributed)


def _issue_forward(step, st) -> None:
    """What every path of the training step issues in front of its backward program, a static list of launches on the current stream (capturable):
    the dynamic scale's `begin` (the loss ops read the word it writes), pack, forward, losses and -- before the backward, which reuses the
    outputs' memory -- the metrics call, appending at the device cursor."""
    P = st.programs
    if step.scaler is not None:
        step._begin_dynamic(st, fills=False)
    P["pack"].run()
    P["fwd"].run()
    P["loss"].run()
    if step.metrics:
        step._append_metrics(st)


class FusedTrainStep:
    """One optimisation step of training_multitask.py:87-103 as ONE stream-ordered program.  `cls_criterion`: "Focal" (config.yaml's
    default, FocalLoss alpha 1 gamma 2), "CE" (CrossEntropyLoss = gamma 0) -- experiment_init.py:232-262; with n_classes == 2 the model has
    ONE logit and the reference trains it with BCEWithLogitsLoss on the {0, 1} label (`:241-242`, training_multitask.py:83-84 leaves the
    label (N, 1)): the same program with the focal kernel's one-logit form.

    metrics=True: the counts behind the reference's Train_dice / Train_acc / Train_F1 (:105-113) are appended on the device by every step --
    `mtbc_train_metrics`, two small launches between the loss program and the backward program (which reuses the outputs' memory) --
    one table row per batch; `begin_epoch_metrics()` starts an epoch, `epoch_metrics()` reads it back once.

    A segmentation-only model (nets.nnUNet) makes this the step of training_segmentation.py:29-62: no classification argument is taken (alpha,
    if given, must be 1.0), `load_batch(image, mask)` / `load_indexed` fill no class target, the loss words are [seg, seg, 0, nan_flag],
    metrics=True appends through `mtbc_seg_step_metrics`, and `epoch_metrics()` returns SegTrainMetrics, the driver's (loss, dice) first.  Data
    parallel is not built for it.

    A classification-only model (nets.nnUNetClassifier, nets.UNetPlusPlusClassifier) makes it the step of training_classification.py:34-98:
    `n_classes`, `cls_criterion` and `focal_weight` as for a multi-task model, no segmentation argument is taken (alpha, if given, must be 0.0),
    `load_batch(image, label)` / `step(image, label)` take no mask, the criterion reads the model's OUTPUT (the 3-class nnUNetClassifier's
    probabilities), the loss words are [cls, 0, cls, nan_flag], metrics=True appends through `mtbc_cls_step_metrics`, and `epoch_metrics()`
    returns ClsTrainMetrics, the driver's (loss, acc, f1) first.  Parameters the forward never reads are not stepped.  Data parallel is not
    built for it."""

    def __init__(self, model, optimizer, alpha: Optional[float] = None, inversely_weighted: Optional[bool] = None, n_classes: Optional[int] = None,
                 distributed: bool = False, n_buckets: int = 4, focal_weight: Optional[torch.Tensor] = None,
                 cls_criterion: Optional[str] = None, graph: Optional[bool] = None, loss_scale=None, metrics: bool = False,
                 metrics_capacity: int = 4096, seg_criterion: Optional[str] = None):
        # the task of the model, the defaults of the arguments not given and what each task refuses: `_resolve_step`, shared with FusedEvalStep
        (self.task, self.alpha, self.iw, self.n_classes, self.seg_criterion, self.binary, self.cls_gamma, self.focal_weight) = _resolve_step(
            model, "the fused step", "FusedTrainStep", distributed, alpha, inversely_weighted, n_classes, focal_weight, cls_criterion, seg_criterion)
        self.seg_only, self.cls_only = not self.task.cls, not self.task.seg
        # metrics: off = exactly the launches of a step without it.  metrics_capacity: rows (= batches per epoch) of the device table, 32 bytes each;
        # allocated once and never moved, so a captured graph stays valid across epochs.
        self.metrics = bool(metrics)
        self.metrics_capacity = int(metrics_capacity)
        if self.metrics and self.metrics_capacity < 1:
            raise ValueError("metrics_capacity must be at least 1 row")
        self._table = MetricsTable(model, self.metrics_capacity, distributed=distributed) if self.metrics else None
        # graph: replay each compiled step as ONE hipGraph from its third call on (None: the MTBC_GRAPH switch).  The step is a static list of ~380
        # launches with every pointer resolved at plan time -- exactly what a graph holds; what changes from step to step (the batch, the learning
        # rate, Adam's bias corrections, the shard weight) lives in device buffers written BEFORE the replay.  Under data parallel the bucket
        # all-reduces are issued between ranges of the backward program by the host, and they stay there: the step is replayed as a short CHAIN of
        # hipGraphs, one per range (`plan_segments`, `run_or_replay_segments`) plus one for the update, with the event records, the waits and the
        # collectives eager between them -- no collective is captured, no graph depends on the communication stream.  Bit-equal to the eager
        # distributed step (which a step with distributed=True, graph=True used to be: the switch was ignored there).
        self.graph = _sw.flag("MTBC_GRAPH") if graph is None else bool(graph)
        # loss_scale: None = the model's static scale baked into the loss ops (65536 in fp16 mode, 1 otherwise; None + the MTBC_DYN_SCALE switch = "dynamic");
        # "dynamic" or a loss_scale.DynamicLossScale = torch.amp.GradScaler's rule on the device: three more launches per step (begin, found-inf check over
        # the flat gradients, state update behind Adam), an overflowing backward skips the update and halves the scale instead of ending the run.
        if loss_scale is None and _sw.flag("MTBC_DYN_SCALE"):
            loss_scale = "dynamic"
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError(f"unknown loss_scale {loss_scale!r} (None | 'dynamic' | a DynamicLossScale)")
            from .loss_scale import DynamicLossScale
            loss_scale = DynamicLossScale()
        if not isinstance(optimizer, FUSED_OPTIMIZERS):
            # torch's own optimizers do not work on the flat buffers this step fills (no gather of p.grad, no device-side scalars): the drop-in loop is theirs
            raise TypeError(f"FusedTrainStep drives FusedAdam, FusedSGD or FusedAdamW (multi_task_breast_cancer_amd.optim), not {type(optimizer).__name__}: "
                            "build it with experiment_init.init_optimizer(..., fused=True)")
        self.scaler = loss_scale
        if self.scaler is not None:
            self.scaler.attach(optimizer)
        self._graphs = {}
        self._sums_loss = self.task.single and self.metrics
        self._epoch_loss = None         # single-task models, metrics=True: device float64 [sum of the steps' loss, steps] behind epoch_metrics()
        self._scratch_target = None     # segmentation only: where the batch-assembly launch puts the labels nobody reads
        self._scratch_mask = None       # classification only: where it puts the masks nobody reads
        self.model, self.opt = model, optimizer
        self.distributed = distributed
        self.n_buckets = n_buckets
        self.world = 1
        self.comm_stream = None
        if distributed:
            import torch.distributed as dist
            self.world = dist.get_world_size()
            self.comm_stream = torch.cuda.Stream()
            optimizer.grad_scale = 1.0 / self.world
            # the bucket all-reduces run on their own stream under the backward pass: keep CUs free for RCCL's resident
            # kernels so that the cooperative InstanceNorm teams (which need every member resident) never queue behind
            # them.  A property of the step programs this trainer builds (mtbc_instnorm_args.coop_reserve_cus), not of
            # the process.
            if self.world > 1 or "MTBC_COOP_RESERVE_CUS" in os.environ:
                reserve = int(_sw.get("MTBC_COOP_RESERVE_CUS"))
                if getattr(model, "coop_reserve_cus", 0) != reserve:
                    model.coop_reserve_cus = reserve
        self._st = None
        self.losses: Optional[torch.Tensor] = None      # device: [total, seg, cls, nan_flag]

    def _compiled(self, N: int, H: int, W: int):
        st = self.model.compiled(N, H, W, fused_loss=_fused_loss(self))
        if st is not self._st:
            self._st = st
            self.model.grads_as_views()
        if st.buckets is None:          # readiness snapshot of THIS step program (model.slots is plan-time scratch)
            st.buckets = plan_buckets(st.slot_ready, self.model.flat_numel, self.n_buckets)
        return st

    def load_batch(self, image: torch.Tensor, mask: torch.Tensor, label: Optional[torch.Tensor] = None, weight: Optional[float] = None):
        """H2D / D2D of training_multitask.py:82-84 into the plan's static buffers (one-hot on the device).
        `weight` = this rank's share n_local / n_batch of the global batch (EpochIndex.weights) when shards are NOT
        equal -- the short last batch of `DataLoader(drop_last=False)`, BUSI_dataloader.py:146: the local mean-loss
        gradient is then scaled by weight * world on the device, so that the summed, 1/world-averaged gradient is the
        global batch's."""
        N, _, H, W = image.shape
        st = self._compiled(N, H, W)
        if label is None and not self.task.seg:     # (image, label): the batches of a driver without a segmentation head carry no mask
            mask, label = None, mask
        fill_batch(st, image, mask, label, self.binary)
        self._set_shard_weight(st, weight)
        return st

    def _set_shard_weight(self, st, weight: Optional[float]) -> None:
        """The shard weight (and, under a dynamic loss scale, its word of the scaler's state) of the batch just loaded: fills in stream order."""
        w = 1.0 if weight is None else float(weight) * self.world
        if self.scaler is None:
            st.grad_weight.fill_(w)
        else:                       # `begin` writes shard weight x scale into st.grad_weight on the device; the weight has a word of its own in the scaler's state
            self.scaler.ensure(st.grad_weight.device)
            self.scaler.set_shard_weight(w)

    def load_indexed(self, dataset, index, params, weight: Optional[float] = None):
        """`load_batch` from a device-resident dataset (device_data.DeviceDataset): ONE launch gathers rows `index` of the uint8 stores under the
        per-sample flip / rotation `params` (None = identity) straight into the plan's static buffers -- image and its intensity channels, mask,
        class target -- with no intermediate tensor and no host-to-device transfer when `index` / `params` are device tensors (EpochTables.batch).
        In stream order in front of the step and, with graph=True, outside the replayed region, where `load_batch` sits.  `weight` as in `load_batch`."""
        _check_in_channels(self.model, dataset)
        st = self._compiled(len(index), dataset.H, dataset.W)
        dataset.assemble(index, params, n_onehot=_n_onehot(self), out=(st.x.data, _mask_of(self, st), _target_of(self, st)))
        self._set_shard_weight(st, weight)
        return st

    # ---- training-time metrics ----------------------------------------------------------------------------------------------
    def _metrics_table(self) -> MetricsTable:
        if self._table is None:
            raise ValueError("this FusedTrainStep was built with metrics=False")
        return self._table.buffers()

    def _append_metrics(self, st) -> None:
        """`mtbc_train_metrics` on the outputs of the forward that has just run (st = None: the empty shard)."""
        self._metrics_table().append(st, self._st.logits.C if self.task.cls else 0)

    def begin_epoch_metrics(self) -> None:
        """Zero the table, the confusion matrix and the cursor in stream order (outside any replayed graph: the buffers stay where they are)."""
        self._metrics_table().zero()
        if self._epoch_loss is not None:
            self._epoch_loss.zero_()

    def _count_loss(self, losses: torch.Tensor) -> None:
        """Single-task models, metrics=True: the step's loss into the epoch's device sum, in stream order behind the step (outside a replayed graph)."""
        if self._sums_loss:
            if self._epoch_loss is None:
                self._epoch_loss = torch.zeros(2, dtype=torch.float64, device=losses.device)
            self._epoch_loss[0] += losses[0].double()
            self._epoch_loss[1] += 1

    def epoch_metrics(self):
        """The epoch so far as the reference's numbers: under data parallel ONE sum-all-reduce of the table and the confusion matrix (row b of the sum is
        GLOBAL batch b), then ONE device-to-host read.  MtbcError when the table was too small or the ranks' cursors disagree."""
        m = train_metrics_from_packed(self._metrics_table().reduce()[0], self.metrics_capacity, self.world)
        total, steps = (0.0, 0.0) if self._epoch_loss is None else self._epoch_loss.cpu().tolist()      # no sum, no read for a multi-task model
        return self.task.epoch_metrics(m, total / steps if steps else 0.0, self.binary)

    def _apply_update(self, st) -> None:
        """Adam on the (all-reduced) flat gradients: the static path divides the baked loss scale out, the dynamic path checks, skips or applies, and
        moves its scale -- all in stream order."""
        if self.scaler is None:
            self.opt.grad_scale = (1.0 / self.world) / getattr(st, "loss_scale", 1.0)
            self.opt.step(grads_in_flat=True)
        else:
            self.scaler.check(self.model.flat_g)
            self.scaler.apply(self.opt, self.world)

    def _begin_dynamic(self, st, fills: bool = True) -> None:
        sc = self.scaler
        if fills:                   # the learning rate of the day, in stream order, outside a captured graph
            sc.ensure(st.grad_weight.device)
            sc.set_lr(self.opt.param_groups[0]["lr"])
        else:
            sc.begin(st.grad_weight, self.world, betas_of(self.opt))

    def _reduce_all(self) -> None:
        allreduce_buckets(self.model.flat_g, self._st.buckets if self._st is not None and self._st.buckets else
                          plan_buckets([(0, self.model.flat_numel, 0)], self.model.flat_numel, 1))

    def _finish(self, st) -> torch.Tensor:
        """Behind every path of the step, outside any replayed graph: where its loss words and the cooperative kernels' error word are."""
        self.losses = st.plan.loss_out
        self._coop_err = self.model.coop_error_word()      # ONE word per model: every compiled step's kernels set it
        self._count_loss(self.losses)
        return self.losses

    def _run_graph(self, st) -> torch.Tensor:
        """The step as a hipGraph replay (`run_or_replay`), keyed by the optimizer's buffers and dropped when they move."""
        opt = self.opt
        sc = self.scaler
        if sc is None:
            opt.grad_scale = (1.0 / self.world) / getattr(st, "loss_scale", 1.0)
            opt.advance_dynamic()                 # step count, lr, bias corrections, decay factor -> 16 bytes of device memory, in stream order, outside the graph
        else:
            opt._ensure_state()
            self._begin_dynamic(st)               # lr -> the scaler's state; step count, scale and bias corrections are the device's own business

        def body():                               # a linear chain on the capturing stream, the metrics call included: replayed with the step
            _issue_forward(self, st)
            st.programs["bwd"].run()
            if sc is None:
                opt.launch_dynamic()
            else:
                self._apply_update(st)

        key = (id(self), opt.graph_key() if sc is None else (opt.graph_key(dynamic=False), sc.graph_key()), self.metrics)
        run_or_replay(self, st, key, body)
        return self._finish(st)

    def _dp_segments(self, st, update):
        """The data-parallel step as (bodies, between, ranges): `bodies` are its static runs of launches on the compute stream -- the dynamic scale's
        `begin`, pack, forward, losses, metrics and the first backward range; one body per further NON-EMPTY backward range of `plan_segments`; then
        `update` -- and `between(i)` is the host's work behind body i: per bucket that became ready, an event record on the compute stream and, on the
        communication stream, the wait and the all-reduce; behind the last backward range also the join.  A bucket with an empty range rides with
        the range in front of it.  `begin` stands in front, where the eager step has always had it: the loss ops read the word it writes."""
        P = st.programs
        ranges = plan_segments(st.buckets, P["bwd"].n)
        groups = []                     # [first, count, bucket indices]: entry 0 always opens one, an empty range joins its predecessor
        for first, count, bks in ranges:
            if groups and count == 0:
                groups[-1][2].extend(bks)
            else:
                groups.append([first, count, list(bks)])
        events = st.__dict__.get("_dp_events")
        if events is None or len(events) != len(st.buckets):          # one event per bucket, for the life of the compiled step
            events = st.__dict__["_dp_events"] = [torch.cuda.Event() for _ in st.buckets]

        def front():                    # on the compute stream, the metrics call too
            _issue_forward(self, st)
            P["bwd"].run(groups[0][0], groups[0][1])

        def backward_range(first, count):
            return lambda: P["bwd"].run(first, count)

        def between(i):
            if i >= len(groups):        # behind the update: nothing
                return
            cur = torch.cuda.current_stream()
            for k in groups[i][2]:
                events[k].record(cur)
                with torch.cuda.stream(self.comm_stream):
                    self.comm_stream.wait_event(events[k])
                    allreduce_buckets(self.model.flat_g, [st.buckets[k]])
            if i == len(groups) - 1:
                cur.wait_stream(self.comm_stream)

        bodies = [front] + [backward_range(first, count) for first, count, _ in groups[1:]] + [update]
        return bodies, between, tuple((first, count) for first, count, _ in ranges)

    def _run_distributed(self, st) -> torch.Tensor:
        """The data-parallel step: its segments (`_dp_segments`) issued one after the other, or -- graph=True -- replayed as a chain of hipGraphs
        (`run_or_replay_segments`) with the same eager work between them.  What `_run_graph` keeps outside its captured body stays outside here."""
        opt, sc = self.opt, self.scaler
        if not self.graph:
            if sc is not None:
                self._begin_dynamic(st)
            bodies, between, _ = self._dp_segments(st, lambda: self._apply_update(st))
            for i, body in enumerate(bodies):
                body()
                between(i)
        else:
            if sc is None:
                opt.grad_scale = (1.0 / self.world) / getattr(st, "loss_scale", 1.0)
                opt.advance_dynamic()
            else:
                opt._ensure_state()
                self._begin_dynamic(st)
            bodies, between, ranges = self._dp_segments(st, opt.launch_dynamic if sc is None else (lambda: self._apply_update(st)))
            key = (id(self), opt.graph_key() if sc is None else (opt.graph_key(dynamic=False), sc.graph_key()), self.metrics, ranges, len(st.buckets))
            run_or_replay_segments(self, st, key, bodies, between, quiesce=self.comm_stream.synchronize)
        return self._finish(st)

    def run(self, st) -> torch.Tensor:
        """One optimisation step on the batch already resident in the plan's buffers."""
        if self.graph and not self.distributed:
            return self._run_graph(st)
        if self.distributed:
            return self._run_distributed(st)
        if self.scaler is not None:
            self._begin_dynamic(st)
        _issue_forward(self, st)
        st.programs["bwd"].run()
        self._apply_update(st)
        return self._finish(st)

    def run_empty(self) -> None:
        """This rank's shard of the (short, last) global batch is EMPTY: contribute a zero gradient to the same
        collectives the other ranks issue, then apply the same update.  Needs one earlier real step (bucket layout)."""
        if not self.distributed:
            return
        if self._st is None:
            raise L.MtbcError("run_empty() before any real step: the bucket layout is not known yet")
        if self.scaler is not None:
            self._begin_dynamic(self._st)
            self._begin_dynamic(self._st, fills=False)
        if self.metrics:            # row b is global batch b on every rank: the empty shard advances the cursor
            self._append_metrics(None)
        self.model.flat_g.zero_()
        for b in self._st.buckets:
            allreduce_buckets(self.model.flat_g, [b])
        self._apply_update(self._st)

    def __call__(self, image, mask, label=None, weight: Optional[float] = None) -> torch.Tensor:
        return self.run(self.load_batch(image, mask, label, weight))

    def check_nan(self) -> None:
        """The reference's NaN guard (criterions.py:72-76) plus the device-side protocol check of the cooperative
        InstanceNorm kernels, one device->host read when the caller chooses.  NaN -> log + exit(1) like the reference;
        a cooperative-kernel failure (a team member was not resident: results are garbage) raises MtbcError."""
        if self.losses is None:
            return
        err = getattr(self, "_coop_err", None)
        vals = torch.cat([self.losses[3:4].double(), (err if err is not None else self.losses[3:4] * 0).double()]).cpu().tolist()
        if vals[1] != 0.0:
            L.raise_coop_timeout("activations and gradients of this and later steps are invalid. Raise MTBC_COOP_RESERVE_CUS, or set MTBC_NO_COOP=1.",
                                 ", e.g. another stream or process held the CUs")
        if vals[0] != 0.0:
            exit_on_nan()


def dice_score_from_counts(counts: torch.Tensor) -> float:
    """metrics.py:255-267 from {tp, fp, fn} float64 counts (mtbc_dice_counts)."""
    tp, fp, fn = (float(v) for v in counts.tolist())
    return _dice(tp, fp, fn)


def dice_counts(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    import ctypes as C
    out = torch.empty(3, dtype=torch.float64, device=logits.device)
    x, t = logits.contiguous().float(), target.contiguous().float()
    L.check(L.load().mtbc_dice_counts(x.data_ptr(), t.data_ptr(), x.numel(), out.data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dice_counts")
    return out


# ------------------------------------------------------------------------------------------------
# validation / inference epoch
# ------------------------------------------------------------------------------------------------
class FusedEvalStep:
    """Forward + losses + metrics of `validate_one_epoch` (training_multitask.py:119-159) with no host round trip per
    batch: the step program runs pack -> forward -> fused Dice/Focal, `mtbc_dice_counts` gives the batch Dice of
    `process_segmentation_predicted` (:66-71: sigmoid(last head) > .5 against the mask, `dice_score_from_tensor`), and
    the confusion matrix of `processes_classification_predicted` (:34-63) accumulates on the device: multi-class =
    argmax of softmax vs argmax of the one-hot label (:41-51); binary head (n_classes == 2, ONE logit) = sigmoid > .5
    vs the {0,1} label (:53-61), classification loss BCEWithLogits (experiment_init.py:242) = the focal kernel's one-logit form
    inside the same step program.  `cls_criterion` ("Focal" | "CE") is the criterion the run TRAINS with (the reference validates with
    the training criterion, and `scheduler.step(val_loss)` runs on that value, training_multitask.py:234-237): with the same
    (alpha, weighting, criterion) the evaluation step shares the training step's compiled plan at equal (N, H, W).  `result()` reads
    everything back once and returns the reference's 6-tuple
    (avg_val_loss, avg_val_dice, val_acc, val_f1, avg_seg_val_loss, avg_cls_val_loss).

    on_device=True: launches only per batch -- pack -> forward -> losses -> `mtbc_eval_metrics` (two launches), which appends the batch's counts
    AND its loss words as one row at a device cursor, into buffers this step owns (`capacity` rows, allocated once, never moved); `result()` is one
    read of an int64 and a float64 array and pure host arithmetic (`eval_result_from_counts`).
    graph (None: the MTBC_GRAPH switch; needs on_device): that chain replayed as ONE hipGraph from the third call of a compiled step on
    (`run_or_replay`); the fills of the batch and of the weight word stay in front of the replay.
    distributed=True (needs on_device): every rank evaluates ITS shard of each global batch with its share `weight` = n_local / n_batch (a rank
    with an empty shard calls `run_empty()`), `result()` sum-all-reduces the two arrays once and every rank returns the SAME six numbers: the
    integer rows sum to the global batch's counts exactly, the weighted loss rows to its mean losses (the criteria allowed here are means over
    samples, and total is linear in seg and cls).  The step itself issues no collective, so graph=True works under it."""

    def __init__(self, model, alpha: Optional[float] = None, inversely_weighted: Optional[bool] = None, n_classes: Optional[int] = None,
                 focal_weight: Optional[torch.Tensor] = None, cls_criterion: Optional[str] = None, seg_criterion: Optional[str] = None,
                 on_device: bool = False, graph: Optional[bool] = None, distributed: bool = False, capacity: int = 4096):
        # a segmentation-only model (nets.nnUNet): `validate_one_epoch` of training_segmentation.py:65-88 -- no label, no classification argument,
        # the metrics launch is `mtbc_seg_step_metrics`, and `result()` is the driver's (val_loss, val_dice)
        # a classification-only model (nets.nnUNetClassifier / UNetPlusPlusClassifier): `validate_one_epoch` of training_classification.py:101-162 --
        # `step(image, label)`, no segmentation argument, the metrics launch is `mtbc_cls_step_metrics`, `result()` is (val_loss, val_acc, val_f1)
        self._scratch_target = self._scratch_mask = None
        self.model, self.on_device, self.distributed, self.capacity = model, bool(on_device), bool(distributed), int(capacity)

        def on_device_rules():          # behind the task's own refusals, in front of the criterion's
            if self.distributed and not self.on_device:
                raise ValueError("FusedEvalStep(distributed=True) needs on_device=True: the ranks' rows are merged from the device table")
            if graph and not self.on_device:
                raise ValueError("FusedEvalStep(graph=True) needs on_device=True: the default path's per-batch torch ops are not a static launch list")
            if self.on_device and self.capacity < 1:
                raise ValueError("capacity must be at least 1 row")

        # seg_criterion, as `cls_criterion`: the criterion the run trains with
        (self.task, self.alpha, self.iw, self.n_classes, self.seg_criterion, self.binary, self.cls_gamma, self.focal_weight) = _resolve_step(
            model, "FusedEvalStep", "FusedEvalStep", distributed, alpha, inversely_weighted, n_classes, focal_weight, cls_criterion, seg_criterion,
            before_criterion=on_device_rules)
        self.seg_only, self.cls_only = not self.task.cls, not self.task.seg
        self.graph = self.on_device and (_sw.flag("MTBC_GRAPH") if graph is None else bool(graph))
        self.world = 1
        if self.distributed:
            import torch.distributed as dist
            self.world = dist.get_world_size()
        self._graphs = {}
        self._table = MetricsTable(model, self.capacity, validation=True, distributed=self.distributed) if self.on_device else None
        self._coop_err = None
        self.reset()

    # the on_device accumulators under the names tests/test_eval_device_gpu.py and tools/eval_cost.py read them by
    _em = property(lambda self: self._table.counts)
    _em_state = property(lambda self: self._table.state)
    _em_loss = property(lambda self: self._table.loss_rows)

    def reset(self) -> None:
        self._acc = None          # device float64: [sum total, sum seg, sum cls, sum dice, batches]
        self._conf = None         # device int64 (3, 3): rows = ground truth, cols = prediction (f1 is asked for labels 0,1,2)
        if self._table is not None:
            self._table.zero()

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, mask: torch.Tensor, label: Optional[torch.Tensor] = None, weight: Optional[float] = None) -> None:
        """`weight`: this rank's share n_local / n_batch of the global batch (distributed=True; None = 1)."""
        N, _, H, W = image.shape
        st = self._compiled(N, H, W)
        if label is None and not self.task.seg:     # (image, label), as FusedTrainStep.load_batch
            mask, label = None, mask
        fill_batch(st, image, mask, label, self.binary)
        self._evaluate_resident(st, weight)

    def _compiled(self, N: int, H: int, W: int):
        return self.model.compiled(N, H, W, fused_loss=_fused_loss(self))

    @torch.no_grad()
    def indexed(self, dataset, index, weight: Optional[float] = None) -> None:
        """`__call__` from a device-resident dataset (device_data.DeviceDataset): rows `index` go into the plan's buffers in one launch (identity
        transform), then the same step program and the same device accumulators.  `weight` as in `__call__`."""
        _check_in_channels(self.model, dataset)
        st = self._compiled(len(index), dataset.H, dataset.W)
        dataset.assemble(index, None, n_onehot=_n_onehot(self), out=(st.x.data, _mask_of(self, st), _target_of(self, st)))
        self._evaluate_resident(st, weight)

    def _evaluate_resident(self, st, weight: Optional[float]) -> None:
        if self.on_device:
            self._evaluate_on_device(st, weight)
        else:                       # the binary head's target column holds the {0, 1} labels themselves
            self._evaluate(st, st.onehot[:, 0].to(torch.int64) if self.binary else None)

    def _evaluate(self, st, gt_binary: Optional[torch.Tensor]) -> None:
        """Forward + losses + metrics of the batch resident in the plan's buffers; gt_binary = the {0, 1} labels of the binary head."""
        N, dev = st.N, st.plan.loss_out.device
        P = st.programs
        P["pack"].run()
        P["fwd"].run()
        P["loss"].run()
        self._coop_err = self.model.coop_error_word()
        if self._acc is None:
            self._acc = torch.zeros(5, dtype=torch.float64, device=dev)
            self._conf = torch.zeros(3, 3, dtype=torch.int64, device=dev)
        if self.task.seg:
            counts = dice_counts(st.segs[-1].data, st.mask)             # {tp, fp, fn} float64 on the device
            tp, fp, fn = counts[0], counts[1], counts[2]
            empty_gt = (tp + fn) == 0
            self._acc[3] += torch.where(empty_gt, torch.where((tp + fp) == 0, torch.ones_like(tp), torch.zeros_like(tp)),
                                        2 * tp / torch.clamp(2 * tp + fp + fn, min=1.0))          # metrics.py:255-267
        self._acc[:3] += st.plan.loss_out[:3].double()
        self._acc[4] += 1
        if self.task.cls:
            self._count_classes(st, gt_binary)

    def _count_classes(self, st, gt_binary: Optional[torch.Tensor]) -> None:
        logit = st.logits.data.view(st.N, -1)
        if self.binary:
            pred = (torch.sigmoid(logit[:, 0]) > 0.5).to(torch.int64)
            gt = gt_binary
        else:
            pred = logit.argmax(dim=1)
            gt = st.onehot.argmax(dim=1)
        self._conf.view(-1).index_add_(0, gt * 3 + pred, torch.ones_like(gt))

    # ---- on_device=True ------------------------------------------------------------------------------------------------------
    def _append_eval(self, st) -> None:
        """`mtbc_eval_metrics` on the outputs and the loss words of the step program that has just run (st = None: the empty shard)."""
        self._table.append(st, (1 if self.binary else 3) if self.task.cls else 0)

    def _evaluate_on_device(self, st, weight: Optional[float]) -> None:
        """The batch resident in the plan's buffers as launches only: pack -> forward -> losses -> mtbc_eval_metrics, eager or as one graph replay."""
        t = self._table.buffers()
        if self.distributed:        # in stream order in front of the call and outside the replayed region: a replay reads the value of the day
            t.weight.fill_(1.0 if weight is None else float(weight))
        P = st.programs

        def body():
            P["pack"].run(); P["fwd"].run(); P["loss"].run()
            self._append_eval(st)   # a linear chain on the capturing stream, appending at the device cursor

        if not self.graph:
            body()
        else:                       # a step that shares the training step's plan keeps its own graph (the entry sits under id(self))
            key = (id(self), "eval", t.counts.data_ptr(), t.state.data_ptr(), t.loss_rows.data_ptr(), t.weight.data_ptr(), self.capacity, self.distributed)
            run_or_replay(self, st, key, body)
        self._coop_err = self.model.coop_error_word()

    def run_empty(self) -> None:
        """This rank's shard of the (short, last) global batch is EMPTY: only the cursor advances, so that row b stays global batch b on every rank."""
        if not self.on_device:
            return
        self._append_eval(None)

    def result(self):
        if self._acc is None and (self._table is None or self._table.counts is None):
            raise L.MtbcError("FusedEvalStep.result() before any batch was evaluated")
        task = self.task
        if self.on_device:              # the 6-tuple, or the classification driver's 3-tuple; the segmentation driver's pair opens the 6-tuple
            r = eval_result_from_packed(*self._table.reduce(self._coop_err), self.capacity, self.world, cls_only=None if task.seg else self.binary)
            return r[:len(task.val_fields)]
        err = self._coop_err
        if err is not None and int(err.item()) != 0:
            L.raise_coop_timeout()
        acc = self._acc.cpu().tolist()
        nb = max(acc[4], 1.0)
        # multi-task: sklearn accuracy_score / f1_score(labels=[0,1,2], average='weighted') (:155-156); training_classification.py:162: `cls_driver_scores`
        accuracy, f1 = task.scores(self._conf.cpu().numpy().astype(np.float64), self.binary)
        v = {"loss": acc[0] / nb, "dice": acc[3] / nb, "accuracy": accuracy, "f1": f1, "seg_loss": acc[1] / nb, "cls_loss": acc[2] / nb}
        return tuple(v[k] for k in task.val_fields)


def validate_one_epoch(step: FusedEvalStep, loader, device) -> tuple:
    """training_multitask.py:119-159 on the fused evaluation step; `loader` yields the reference's batch dicts."""
    step.reset()
    fields = ("image",) + step_task(step).batch_fields
    for data in loader:
        step(*(data[k].to(device) for k in fields))
    return step.result()


# ------------------------------------------------------------------------------------------------
# epochs from a device-resident dataset (device_data.py, csrc/batch_loader.hip)
# ------------------------------------------------------------------------------------------------
def _check_tables(dataset, tables) -> None:
    if len(tables.batches) and (tables.index_min < 0 or tables.index_max >= len(dataset)):      # host copies kept by EpochTables: no transfer
        raise ValueError(f"epoch tables hold indices in [{tables.index_min}, {tables.index_max}], the dataset has {len(dataset)} rows")


def _train_epoch(step: FusedTrainStep, dataset, tables, lr: Optional[float]) -> tuple:
    """The loop `train_one_epoch` and `train_one_epoch_with_metrics` share: (avg_total, avg_seg, avg_cls) over the batches this rank ran."""
    _check_tables(dataset, tables)
    if lr is not None:
        for group in step.opt.param_groups:
            group["lr"] = float(lr)
    acc = None                    # device float64: [sum total, sum seg, sum cls, sum of the steps' NaN flags]
    ran = 0
    for b in range(len(tables)):
        index, params, n_local, weight = tables.batch(b)
        if n_local == 0:
            step.run_empty()
            continue
        losses = step.run(step.load_indexed(dataset, index, params, weight if step.distributed else None))
        if acc is None:
            acc = torch.zeros(4, dtype=torch.float64, device=losses.device)
        acc += losses[:4].double()
        ran += 1
    if acc is None:
        return 0.0, 0.0, 0.0
    step.check_nan()
    total, seg, cls, nan = acc.cpu().tolist()
    if nan != 0.0 or total != total:
        exit_on_nan()
    return total / ran, seg / ran, cls / ran


def train_one_epoch(step: FusedTrainStep, dataset, tables, lr: Optional[float] = None) -> tuple:
    """The batch loop of training_multitask.py:74-103 on the fused step with no host work per batch: `dataset` is a
    device_data.DeviceDataset, `tables` the epoch's device_data.EpochTables.  Per batch: one assembly launch into the plan's buffers
    (`load_indexed`) and the step; the loss words are summed on the device in float64, read back once at the end of the epoch together
    with ONE `check_nan()` (a NaN in any step's loss ends the run like the reference's guard, criterions.py:72-76).  Nothing is copied
    from host to device inside the loop.  The short last batch of drop_last=False compiles (once) a second plan.  Under data parallel
    each batch carries this rank's share `weight`, and a rank whose shard of the last batch is empty calls `run_empty()`.
    `lr`: written into the optimizer's parameter groups first (the scheduler's value of the epoch).

    Returns (avg_total, avg_seg, avg_cls): means over the batches this rank ran, as `training_loss / len(training_loader)` (:110).
    The reference's training-time Dice, accuracy and F1 (:107-113) come from `train_one_epoch_with_metrics` on a step built with metrics=True."""
    return _train_epoch(step, dataset, tables, lr)


def train_one_epoch_with_metrics(step: FusedTrainStep, dataset, tables, lr: Optional[float] = None) -> tuple:
    """`train_one_epoch` plus the training-time metrics of training_multitask.py:105-113, still with no host read inside the batch loop: the step
    (built with metrics=True) appends each batch's counts on the device; `begin_epoch_metrics()` in front, `epoch_metrics()` behind (one all-reduce
    under data parallel, one read).  Returns the reference's 4-tuple (avg_training_loss, avg_training_dice, training_acc, training_f1) (:116).
    Under data parallel Dice, accuracy and F1 are those of the GLOBAL batches (the same on every rank); the loss is this rank's mean, as above."""
    if not getattr(step, "metrics", False):
        raise ValueError("train_one_epoch_with_metrics needs a FusedTrainStep built with metrics=True")
    step.begin_epoch_metrics()
    total, _, _ = _train_epoch(step, dataset, tables, lr)
    m = step.epoch_metrics()            # (loss, dice) for training_segmentation.py:62, (loss, acc, f1) for training_classification.py:98
    return (total,) + tuple(getattr(m, k) for k in step_task(step).train_fields)


def validate_one_epoch_indexed(step: FusedEvalStep, dataset, tables) -> tuple:
    """`validate_one_epoch` from a device-resident dataset: the batches of `tables` (built without transforms: the identity path), one
    assembly launch each; the reference's 6-tuple, read back once.  With a distributed step (`tables` from a rank-sharded EpochIndex) each batch
    carries this rank's share and an empty shard calls `run_empty()`: every rank returns the global validation set's numbers."""
    _check_tables(dataset, tables)
    if tables.params is not None:
        raise ValueError("validation runs without transforms (training_multitask.py:199-201): build the tables with transforms=None")
    step.reset()
    distributed = getattr(step, "distributed", False)
    for b in range(len(tables)):
        index, _, n_local, weight = tables.batch(b)
        if n_local:
            if distributed:
                step.indexed(dataset, index, weight)
            else:
                step.indexed(dataset, index)
        elif distributed:           # row b is global batch b on every rank
            step.run_empty()
    return step.result()


# ------------------------------------------------------------------------------------------------
# one fold of the reference's training script (training_multitask.py:216-280) on the indexed epochs
# ------------------------------------------------------------------------------------------------
def fit_fold(step: FusedTrainStep, eval_step: FusedEvalStep, dataset, train_index, val_index, scheduler, run_dir: str, epochs: int,
             max_patience: int, transforms: Optional[dict], seed: int, plateau: bool, checkpoint_name: str = "model_best",
             test_step=None, test_index=None) -> List[tuple]:
    """The epoch loop of training_multitask.py:216-280: `train_index` / `val_index` are dataset_index.EpochIndex objects over the rows of
    `dataset` (a device_data.DeviceDataset), `scheduler` a torch scheduler on `step.opt` stepped once per epoch -- with the validation loss
    when `plateau` (:234-237).  Per epoch: the learning rate of the day, the epoch's device tables (`transforms`, `seed`), training with
    metrics, validation, the scheduler, a checkpoint under run_dir/checkpoint_name on a new best validation loss, the patience rule, one row of
    run_dir/metrics.csv under METRICS_HEADER and the reference's log line.  Files are written by rank 0 only under data parallel.
    Returns the rows as tuples (epoch, lr, train_loss, val_loss, train_dice, val_dice, train_acc, train_f1, val_acc, val_f1).

    With the segmentation pair of steps (both built on a nets.nnUNet) this is the epoch loop of training_segmentation.py:143-201 instead:
    `test_step` (an inference.FusedSegTestStep) and `test_index` are required, because that driver runs its testing phase after EVERY epoch
    (:179) and writes its mean DICE into the row; metrics.csv gets the header `epoch,LR,Train,Validation,Test,Train_loss,Val_loss` and the
    row of :192-195 (the learning rate AFTER the scheduler step); the rows returned are (epoch, lr, train_dice, val_dice, test_dice,
    train_loss, val_loss).  Rotation: that driver draws ONE bound d = np.random.choice(range(0, 360)) per run (:118) and rotates by
    U(-d, d): pass transforms={"horizontal_flip": .5, "vertical_flip": .5, "rotation": d / 360}.

    With the classification pair of steps (both built on a nets.nnUNetClassifier / UNetPlusPlusClassifier) it is the epoch loop of
    training_classification.py:216-271: metrics.csv gets the header `epoch,LR,Train_loss,Validation_loss,Train_acc,Train_F1,Validation_acc,
    Validation_F1` and the row of :262-266 (the learning rate at the START of the epoch); the rows returned are (epoch, lr, train_loss, val_loss,
    train_acc, train_f1, val_acc, val_f1).  That driver's testing phase runs once, after the loop (:284-298): `test_one_epoch_indexed` with an
    inference.FusedClsTestStep; `test_step` / `test_index` are not used here."""
    import logging
    import time
    from .device_data import EpochTables
    task, eval_task = step_task(step), step_task(eval_step)
    if task is not eval_task:
        odd = CLASSIFICATION if CLASSIFICATION in (task, eval_task) else SEGMENTATION
        raise ValueError(f"fit_fold: the training and the evaluation step must both be built on a {odd.name}-only model, or neither")
    if task.tests_every_epoch and (test_step is None or test_index is None):
        raise ValueError("fit_fold: the segmentation driver runs its testing phase after every epoch: pass test_step (inference.FusedSegTestStep) "
                         "and test_index")
    if step.distributed and not getattr(eval_step, "distributed", False):
        # every rank must read the SAME val_loss: the scheduler, the checkpoint rule and early stopping below act on it, and a rank that
        # leaves the epoch loop alone leaves the others waiting in a collective
        raise ValueError("fit_fold: the training step is data parallel, the evaluation step is not: build it with "
                         "FusedEvalStep(..., on_device=True, distributed=True) so that every rank sees the same validation numbers")
    writer = True
    if step.distributed:
        import torch.distributed as dist
        writer = dist.get_rank() == 0
    os.makedirs(run_dir, exist_ok=True)
    metrics_path = os.path.join(run_dir, "metrics.csv")
    if writer:
        CK.write_metrics_file(metrics_path, task.header)
    stopper = CK.EarlyStopping(max_patience)
    val_tables = EpochTables(val_index, 0, None, device=dataset.device)        # no shuffle that matters, no transforms (:199-201)
    test_tables = EpochTables(test_index, 0, None, device=dataset.device) if task.tests_every_epoch else None
    train_names = ("train_loss",) + tuple("train_" + k for k in task.train_fields)
    val_names = tuple("val_" + k for k in task.val_fields)
    rows = []
    for epoch in range(int(epochs)):
        v = {"epoch": epoch, "lr": step.opt.param_groups[0]["lr"]}
        t0 = time.perf_counter()
        tables = EpochTables(train_index, epoch, transforms, seed=seed, device=dataset.device)
        v.update(zip(train_names, train_one_epoch_with_metrics(step, dataset, tables), strict=True))
        v.update(zip(val_names, validate_one_epoch_indexed(eval_step, dataset, val_tables), strict=True))
        if plateau:
            scheduler.step(v["val_loss"])
        else:
            scheduler.step()
        if stopper.update(v["val_loss"]) and writer:
            CK.save_checkpoint(os.path.join(run_dir, checkpoint_name), epoch, step.model, step.opt, v["val_loss"], scaler=step.scaler)
        v.update(patience=stopper.patience, epoch_time=time.perf_counter() - t0, best=stopper.best)
        if task.tests_every_epoch:          # behind the checkpoint decision, outside the epoch's time (training_segmentation.py:179)
            v["test_dice"] = float(np.mean([r["DICE"] for r in test_one_epoch_indexed(test_step, dataset, test_tables)]))
        if not task.lr_at_start:
            v["lr"] = step.opt.param_groups[0]["lr"]
        logging.info(task.log.format(**v))
        row = tuple(v[k] for k in task.row_fields)
        rows.append(row)
        if writer:
            CK.write_metrics_file(metrics_path, task.row(*row))
        if stopper.should_stop:
            logging.info(f"\nValidation loss did not improve over the last {stopper.patience} epochs. Stopping training")
            break
    return rows


def test_one_epoch_indexed(test_step, dataset, tables) -> list:
    """The testing phase of the segmentation driver from a device-resident dataset: the batches of `tables` (no transforms) through an
    inference.FusedSegTestStep; the rows of results_segmentation.csv, read back once.  With an inference.FusedClsTestStep: the classification
    driver's testing phase, the (ground_truth, predicted_label) rows of its results.csv.  With an inference.FusedTestStep: the multi-task testing
    phase, its (segmentation_rows, classification_rows)."""
    _check_tables(dataset, tables)
    _check_in_channels(test_step.model, dataset)
    test_step.reset()
    for b in range(len(tables)):
        index, _, n_local, _ = tables.batch(b)
        if n_local:
            test_step.indexed(dataset, index)
    return test_step.result()
