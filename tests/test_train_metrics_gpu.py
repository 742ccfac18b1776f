"""Training-time metrics on the GPU: mtbc_train_metrics against torch on the CPU (exact integers), the cursor, the capacity guard and the
empty shard; FusedTrainStep(metrics=True) eager, as a replayed hipGraph, with the binary head and under a dynamic loss scale, each against
a torch restatement on clones of the step's own forward outputs; the epoch and fold drivers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import checkpoint as CK  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet, MTUNetPlusPlus  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
TRANSFORMS = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}


# ------------------------------------------------------------------------------------------------ the torch restatement (CPU)
def want_row(seg_logits, mask, n):
    """tp, fp, fn of process_segmentation_predicted's mask (training_multitask.py:69) against the ground truth, and the sample count."""
    s, g = torch.sigmoid(seg_logits.cpu().float()) > .5, mask.cpu() != 0
    return [int((s & g).sum()), int((s & ~g).sum()), int((~s & g).sum()), int(n)]


def want_conf(logits, target):
    """processes_classification_predicted (:34-63) as a 3 x 3 count, rows = ground truth."""
    logits, target = logits.cpu().float(), target.cpu().float()
    if logits.shape[1] == 1:
        pred, gt = (torch.sigmoid(logits[:, 0]) > .5).long(), (target[:, 0] != 0).long()
    else:
        pred, gt = torch.softmax(logits, dim=1).argmax(dim=1), target.argmax(dim=1)
        nan = torch.isnan(logits).any(dim=1)                  # softmax spreads a NaN over the row; torch.argmax of the logits picks the (first) NaN
        pred = torch.where(nan, logits.argmax(dim=1), pred)
    conf = torch.zeros(3, 3, dtype=torch.int64)
    conf.view(-1).index_add_(0, gt * 3 + pred, torch.ones_like(gt))
    return conf


class Acc:
    """table [capacity + 1][4] (the extra row is a sentinel behind the table), conf, state -- and the call."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.table = torch.zeros(capacity + 1, 4, dtype=torch.int64, device=DEV)
        self.table[capacity] = -7
        self.conf = torch.zeros(3, 3, dtype=torch.int64, device=DEV)
        self.state = torch.zeros(2, dtype=torch.int32, device=DEV)

    def append(self, seg, mask, logits, target, n_logits=None):
        a = L.TrainMetricsArgs()
        if seg is not None:
            assert seg.dtype == mask.dtype == logits.dtype == target.dtype == torch.float32
            assert seg.numel() == mask.numel() and logits.shape == target.shape
            a.seg_logits, a.mask, a.n_seg = seg.data_ptr(), mask.data_ptr(), seg.numel()
            a.cls_logits, a.target, a.N, a.n_logits = logits.data_ptr(), target.data_ptr(), logits.shape[0], logits.shape[1]
        else:
            a.N, a.n_seg, a.n_logits = 0, 0, n_logits
        a.table, a.conf, a.state, a.capacity = self.table.data_ptr(), self.conf.data_ptr(), self.state.data_ptr(), self.capacity
        L.check(L.load().mtbc_train_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "train_metrics")

    def read(self):
        assert self.table[self.capacity].tolist() == [-7] * 4, "the row behind the table was written"
        return self.table[:self.capacity].cpu(), self.conf.cpu(), self.state.cpu().tolist()


def seg_case(shape, seed, offset=0, empty_mask=False):
    """fp32 logits with exact zeros, +-tiny values and +-0 among them, a {0, 1} mask; offset = 1: 4-byte-offset views of larger buffers."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    x = torch.randn(n + offset, generator=g) * 3
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.4e-45, -1.4e-45, 1e-3, -1e-3, 80.0, -80.0, 200.0, -200.0])
    pos = torch.randperm(n, generator=g)[:4 * len(special)] + offset
    x[pos] = special.repeat(4)                               # against mask 0 and mask 1 alike
    m = (torch.rand(n + offset, generator=g) < .4).float()
    if empty_mask:
        m.zero_()
    x, m = x.to(DEV), m.to(DEV)
    return x[offset:].view(shape), m[offset:].view(shape)


def cls_case(n, n_logits, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, n_logits, generator=g)
    if n_logits == 1:
        logits[:3, 0] = torch.tensor([0.0, 1e-30, -1e-30])
        target = torch.randint(0, 2, (n, 1), generator=g).float()
    else:
        rows = [[2., 2., 1.], [0., 3., 3.], [1., 1., 1.], [float("nan"), 1., float("nan")], [1., float("nan"), 5.], [-1., -2., float("nan")]]
        k = min(n, len(rows))
        logits[:k] = torch.tensor(rows)[:k, :n_logits]
        target = torch.nn.functional.one_hot(torch.randint(0, n_logits, (n,), generator=g), n_logits).float()
    return logits.to(DEV), target.to(DEV)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape,offset,empty_mask,n_logits", [
    ((3, 1, 17, 30), 0, False, 3),       # 1530 pixels: two behind the last whole vector
    ((5, 1, 64, 64), 0, False, 3),       # the vector path, 10 blocks
    ((5, 1, 64, 64), 1, False, 3),       # 4-byte-offset views: the unaligned path
    ((3, 1, 17, 30), 1, True, 1),        # an all-zero mask; the binary head
    ((7, 1, 64, 64), 0, True, 1),
])
def test_kernel_against_torch_exact(shape, offset, empty_mask, n_logits):
    seg, mask = seg_case(shape, seed=3, offset=offset, empty_mask=empty_mask)
    assert seg.data_ptr() % 16 == (4 if offset else 0) and (seg == 0).sum().item() >= 8
    logits, target = (t[:shape[0]].contiguous() for t in cls_case(7, n_logits, seed=4))     # the first rows are the hand-written ones
    acc = Acc(4)
    acc.append(seg, mask, logits, target)
    table, conf, state = acc.read()
    want = want_row(seg, mask, shape[0])
    print("row", table[0].tolist(), "want", want)
    assert table[0].tolist() == want and not table[1:].any()
    assert want[0] + want[2] == int((mask != 0).sum()) and (empty_mask or (want[0] and want[1] and want[2]))
    assert torch.equal(conf, want_conf(logits, target)) and int(conf.sum()) == shape[0]
    assert state == [1, 0]


def test_first_maximum_ties_and_nan_rows():
    logits, target = cls_case(9, 3, seed=5)
    seg, mask = seg_case((9, 1, 8, 8), seed=6)
    acc = Acc(1)
    acc.append(seg, mask, logits, target)
    _, conf, _ = acc.read()
    pred = [0, 1, 0, 0, 1, 2]                                 # the six hand-written rows of cls_case: first maximum, a NaN is the maximum
    gt = target[:6].argmax(dim=1).tolist()
    hand = torch.zeros(3, 3, dtype=torch.int64)
    for g, p in zip(gt, pred):
        hand[g, p] += 1
    assert torch.equal(want_conf(logits[:6], target[:6]), hand)          # the restatement itself, against the rule written out
    assert torch.equal(conf, want_conf(logits, target))


def test_three_calls_fill_three_rows_in_order():
    acc = Acc(5)
    rows, conf_sum = [], torch.zeros(3, 3, dtype=torch.int64)
    for k, shape in enumerate([(3, 1, 17, 30), (5, 1, 64, 64), (2, 1, 16, 16)]):
        seg, mask = seg_case(shape, seed=10 + k)
        logits, target = cls_case(shape[0], 3, seed=20 + k)
        acc.append(seg, mask, logits, target)
        rows.append(want_row(seg, mask, shape[0]))
        conf_sum += want_conf(logits, target)
    table, conf, state = acc.read()
    assert table[:3].tolist() == rows and not table[3:].any()
    assert torch.equal(conf, conf_sum) and state == [3, 0]


def test_capacity_two_with_three_calls_drops_the_third():
    acc = Acc(2)
    rows, conf_sum = [], torch.zeros(3, 3, dtype=torch.int64)
    for k in range(3):
        seg, mask = seg_case((5, 1, 64, 64), seed=30 + k)
        logits, target = cls_case(5, 3, seed=40 + k)
        acc.append(seg, mask, logits, target)
        if k < 2:
            rows.append(want_row(seg, mask, 5))
            conf_sum += want_conf(logits, target)
    table, conf, state = acc.read()                           # also: the sentinel row behind the table is untouched
    assert table.tolist() == rows and state == [3, 1]
    assert torch.equal(conf, conf_sum)                        # the matrix describes the batches that have a row
    with pytest.raises(L.MtbcError, match="metrics_capacity"):
        T.train_metrics_from_packed(T.reduce_train_metrics(acc.table[:2], acc.conf, acc.state), 2)


def test_empty_shard_only_advances_the_cursor():
    acc = Acc(3)
    seg, mask = seg_case((2, 1, 16, 16), seed=50)
    logits, target = cls_case(2, 3, seed=51)
    acc.append(seg, mask, logits, target)
    acc.append(None, None, None, None, n_logits=3)
    acc.append(seg, mask, logits, target)
    table, conf, state = acc.read()
    row = want_row(seg, mask, 2)
    assert table.tolist() == [row, [0, 0, 0, 0], row] and state == [3, 0]
    assert torch.equal(conf, 2 * want_conf(logits, target))
    acc.append(None, None, None, None, n_logits=3)            # behind the table: still only the cursor
    assert acc.read()[2] == [4, 0]


# ------------------------------------------------------------------------------------------------ the step
def build(arch, compute=None, n_classes=3, seed=1993, **kw):
    seed_everything(seed)
    nl = 1 if n_classes == 2 else n_classes
    m = (MTnnUNet(1, 1, nl) if arch == "MTnnUNet" else MTUNetPlusPlus(in_channels=1, out_channels=1, n_classes=nl, deep_supervision=True)).to(DEV)
    if compute:
        m.set_compute(compute)
    opt = FusedAdam(m, lr=1e-3, eps=1e-4)
    return m, opt, T.FusedTrainStep(m, opt, alpha=0.5, n_classes=n_classes, **kw)


def batches(n_steps, n=2, size=64, seed0=70, binary=False):
    out = []
    for s in range(n_steps):
        img, mask, label = O.synthetic_batch(n, size, size, seed=seed0 + s)
        if binary:
            label = (label != 0).float()
        out.append((img.to(DEV), mask.to(DEV), label.to(DEV)))
    return out


def run_with_clones(step, data):
    """Per step: load, run `pack` and `fwd` by hand, clone the outputs the metrics call will see, then the real step (which recomputes the same
    forward: it is deterministic) -> the expected table rows and confusion matrix from the clones."""
    rows, conf = [], torch.zeros(3, 3, dtype=torch.int64)
    for img, mask, label in data:
        st = step.load_batch(img, mask, label)
        st.programs["pack"].run()
        st.programs["fwd"].run()
        seg, logits = st.segs[-1].data.clone(), st.logits.data.clone()
        assert seg.dtype == torch.float32 and logits.dtype == torch.float32 and seg.shape == st.mask.shape     # fp32 NCHW in every compute mode
        step.run(st)
        rows.append(want_row(seg, st.mask, st.N))
        conf += want_conf(logits.view(st.N, -1), st.onehot)
    return rows, conf


def check_metrics(m, rows, conf):
    assert m.table.tolist() == rows and m.batches == len(rows)
    assert torch.equal(torch.from_numpy(m.conf), conf)
    want = T.train_metrics_from_counts(np.array(rows, dtype=np.int64).reshape(-1, 4), conf.numpy())
    training_dice = 0.
    for tp, fp, fn, _ in rows:                                # metrics.py:255-267 on the same integers
        training_dice += (1.0 if tp + fp == 0 else 0.0) if tp + fn == 0 else 2 * float(tp) / (2 * float(tp) + fp + fn)
    assert m.dice == training_dice / len(rows) == want.dice
    assert (m.accuracy, m.f1) == (want.accuracy, want.f1)


@pytest.mark.parametrize("arch,compute", [("MTnnUNet", None), ("MTUNetPlusPlus", None), ("MTUNetPlusPlus", "bf16")])
def test_step_metrics_equal_the_restatement_and_leave_the_step_alone(arch, compute):
    data = batches(3)
    model, _, step = build(arch, compute, metrics=True)
    step.begin_epoch_metrics()
    rows, conf = run_with_clones(step, data)
    m = step.epoch_metrics()
    print(arch, compute, "rows", rows, "conf", conf.tolist(), "dice", m.dice, "acc", m.accuracy, "f1", m.f1)
    check_metrics(m, rows, conf)
    assert sum(r[0] + r[1] for r in rows) > 0 or sum(r[2] for r in rows) > 0
    plain_model, _, plain = build(arch, compute)
    assert plain.metrics is False
    for img, mask, label in data:
        plain(img, mask, label)
    assert torch.equal(model.flat_p, plain_model.flat_p)      # the metrics call reads; the update is bit for bit the one without it
    step.check_nan()
    again = step.epoch_metrics()                              # reading does not consume: the accumulators stay
    assert again.table.tolist() == rows
    with pytest.raises(ValueError):
        plain.epoch_metrics()


def test_graph_replay_appends_at_the_device_cursor():
    data = batches(7, seed0=80)
    eager_model, _, eager = build("MTnnUNet", metrics=True, graph=False)
    graph_model, _, graph = build("MTnnUNet", metrics=True, graph=True)
    for step in (eager, graph):
        step.begin_epoch_metrics()
        for img, mask, label in data[:5]:
            step(img, mask, label)
    ents = [e for e in graph._graphs.values() if e[2] is not None]
    assert len(ents) == 1                                     # captured at the third call, replayed for the fourth and fifth
    captured = ents[0][2]
    me, mg = eager.epoch_metrics(), graph.epoch_metrics()
    assert mg.batches == 5 and mg.table.tolist() == me.table.tolist() and np.array_equal(mg.conf, me.conf)
    assert (mg.dice, mg.accuracy, mg.f1) == (me.dice, me.accuracy, me.f1)
    assert torch.equal(graph_model.flat_p, eager_model.flat_p)
    # second epoch: zeroed outside the replayed region, the SAME graph object appends from row 0
    for step in (eager, graph):
        step.begin_epoch_metrics()
        for img, mask, label in data[5:]:
            step(img, mask, label)
    assert [e[2] for e in graph._graphs.values() if e[2] is not None] == [captured]
    me, mg = eager.epoch_metrics(), graph.epoch_metrics()
    assert mg.batches == 2 and mg.table.tolist() == me.table.tolist() and np.array_equal(mg.conf, me.conf)
    assert int(mg.conf.sum()) == 4 and mg.table[:, 3].tolist() == [2, 2]
    assert torch.equal(graph_model.flat_p, eager_model.flat_p)


def test_binary_head():
    data = batches(3, n=3, seed0=90, binary=True)
    _, _, step = build("MTnnUNet", n_classes=2, metrics=True)
    step.begin_epoch_metrics()
    rows, conf = run_with_clones(step, data)
    m = step.epoch_metrics()
    check_metrics(m, rows, conf)
    assert int(m.conf[2].sum()) == 0 and int(m.conf[:, 2].sum()) == 0 and int(m.conf.sum()) == 9


def test_a_skipped_update_still_counts_its_batch():
    sc = DynamicLossScale(init_scale=2.0 ** 40, growth_interval=10 ** 6)
    model, _, step = build("MTUNetPlusPlus", "f16", metrics=True, loss_scale=sc)
    data = batches(1, seed0=31)
    step.begin_epoch_metrics()
    model.ensure_flat()
    before = model.flat_p.clone()
    rows, conf = run_with_clones(step, data)
    stats = sc.stats()
    assert stats["skipped"] == 1 and stats["t"] == 0 and torch.equal(model.flat_p, before), stats        # the update was skipped ...
    m = step.epoch_metrics()
    check_metrics(m, rows, conf)                              # ... the forward happened: the batch is counted (the reference has no skip)
    assert m.batches == 1 and int(m.conf.sum()) == 2


def test_capacity_overflow_raises_and_names_the_argument():
    _, _, step = build("MTnnUNet", metrics=True, metrics_capacity=2)
    data = batches(3)
    step.begin_epoch_metrics()
    for img, mask, label in data:
        step(img, mask, label)
    with pytest.raises(L.MtbcError, match="metrics_capacity"):
        step.epoch_metrics()
    step.begin_epoch_metrics()
    step(*data[0])
    assert step.epoch_metrics().batches == 1


# ------------------------------------------------------------------------------------------------ the drivers
def store(M, H, W, seed):
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def test_train_one_epoch_with_metrics_over_a_short_last_batch():
    images, masks, labels = store(10, 64, 64, seed=30)
    ds = DD.DeviceDataset(images, masks, labels)
    ei = EpochIndex(np.arange(10), 4, seed=13, drop_last=False)
    model, _, step = build("MTnnUNet", metrics=True)
    plain_model, _, plain = build("MTnnUNet")
    tables = DD.EpochTables(ei, 0, TRANSFORMS)
    got = T.train_one_epoch_with_metrics(step, ds, tables, lr=1e-4)
    want3 = T.train_one_epoch(plain, ds, tables, lr=1e-4)
    assert len(got) == 4 and len(want3) == 3 and got[0] == want3[0]          # train_one_epoch keeps its 3-tuple; the loss is the same number
    assert torch.equal(model.flat_p, plain_model.flat_p)
    m = step.epoch_metrics()                                  # the 4 + 4 + 2 batches: two plans, one set of accumulators
    assert m.batches == 3 and m.table[:, 3].tolist() == [4, 4, 2] and int(m.conf.sum()) == 10
    assert got[1:] == (m.dice, m.accuracy, m.f1)
    assert m.table[:, [0, 2]].sum(axis=1).tolist() == [int(ds.assemble(*tables.batch(b)[:2])[1].sum().item()) for b in range(3)]   # tp + fn = the batch's tumour pixels
    assert np.array_equal(m.conf.sum(axis=1), np.bincount(labels.numpy(), minlength=3))
    with pytest.raises(ValueError):
        T.train_one_epoch_with_metrics(plain, ds, tables)
    got2 = T.train_one_epoch_with_metrics(step, ds, DD.EpochTables(ei, 1, TRANSFORMS))     # a second epoch starts from zero
    assert step.epoch_metrics().batches == 3 and len(got2) == 4


def test_fit_fold_writes_the_reference_metrics_file(tmp_path):
    images, masks, labels = store(14, 64, 64, seed=33)
    ds = DD.DeviceDataset(images, masks, labels)
    model, opt, step = build("MTnnUNet", metrics=True)
    eval_step = T.FusedEvalStep(model, alpha=0.5)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    run_dir = str(tmp_path / "fold_0")
    rows = T.fit_fold(step, eval_step, ds, EpochIndex(np.arange(10), 4, seed=13), EpochIndex(np.arange(10, 14), 4, seed=13), scheduler, run_dir,
                      epochs=2, max_patience=5, transforms=TRANSFORMS, seed=13, plateau=False)
    assert len(rows) == 2 and all(len(r) == 10 for r in rows) and [r[0] for r in rows] == [0, 1]
    assert rows[0][1] == 1e-3 and rows[1][1] < rows[0][1]                    # the learning rate of the day, read before the scheduler moved it
    lines = open(os.path.join(run_dir, "metrics.csv")).read().splitlines()
    assert lines[0] == CK.METRICS_HEADER and len(lines) == 3
    for line, r in zip(lines[1:], rows):
        assert line == CK.metrics_row(*r)
        assert line == (f"{r[0]},{r[1]:.8f},{r[2]:.4f},{r[3]:.4f},{r[4]:.4f}, {r[5]:.4f},{r[6]:.4f},{r[7]:.4f},{r[8]:.4f},{r[9]:.4f}")
        assert all(0.0 <= v <= 1.0 for v in r[4:])
    ckpt = torch.load(os.path.join(run_dir, "model_best"), map_location="cpu", weights_only=False)
    assert ckpt["epoch"] in (0, 1) and ckpt["val_loss"] == min(r[3] for r in rows)
    assert set(ckpt) >= {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler", "val_loss"}
