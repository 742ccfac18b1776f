"""The validation epoch on the device: mtbc_eval_metrics through the C-ABI against a torch / numpy restatement on the host (exact integers, exact
float64 loss rows), FusedEvalStep(on_device=True) against the host function on clones of what the same call computed and against the default path,
the hipGraph replay, the indexed epoch, the capacity guard, two ranks with real kernels, and fit_fold."""
import ctypes as C
import os
import queue as _queue
import socket
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import trainer as T  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet  # noqa: E402
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


def want_loss_row(loss_words, w=1.0):
    """What the kernel stores: w * (double)word, one float64 product per word."""
    return (np.float64(w) * loss_words.cpu().numpy().astype(np.float64)[:4]).tolist()


def close6(got, want):
    """The six numbers of two paths that sum the same float32 loss words in the same order in float64: the three losses bit for bit; Dice, accuracy
    and F1 (the same integers through the same expressions, on the device in one path and on the host in the other) within 1e-12."""
    assert len(got) == len(want) == 6
    assert (got[0], got[4], got[5]) == (want[0], want[4], want[5]), (got, want)
    assert all(abs(got[i] - want[i]) <= 1e-12 for i in (1, 2, 3)), (got, want)


# ------------------------------------------------------------------------------------------------ the kernel, through the C-ABI
class Acc:
    """table [capacity + 1][4], loss_rows [capacity + 1][4] (the extra rows are sentinels behind them), conf, state, a weight word -- and the call."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.table = torch.zeros(capacity + 1, 4, dtype=torch.int64, device=DEV)
        self.table[capacity] = -7
        self.loss_rows = torch.zeros(capacity + 1, 4, dtype=torch.float64, device=DEV)
        self.loss_rows[capacity] = -7.0
        self.conf = torch.zeros(3, 3, dtype=torch.int64, device=DEV)
        self.state = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.weight = torch.ones(1, dtype=torch.float32, device=DEV)

    def append(self, seg, mask, logits, target, loss_in, weight=None, n_logits=None):
        a = L.EvalMetricsArgs()
        if seg is not None:
            assert seg.dtype == mask.dtype == logits.dtype == target.dtype == loss_in.dtype == torch.float32
            assert seg.numel() == mask.numel() and logits.shape == target.shape and loss_in.numel() == 4
            a.seg_logits, a.mask, a.n_seg = seg.data_ptr(), mask.data_ptr(), seg.numel()
            a.cls_logits, a.target, a.N, a.n_logits = logits.data_ptr(), target.data_ptr(), logits.shape[0], logits.shape[1]
            a.loss_in = loss_in.data_ptr()
        else:
            a.N, a.n_seg, a.n_logits = 0, 0, n_logits
        a.table, a.conf, a.state, a.capacity = self.table.data_ptr(), self.conf.data_ptr(), self.state.data_ptr(), self.capacity
        a.loss_rows = self.loss_rows.data_ptr()
        if weight is not None:                                # filled in stream order in front of the call
            self.weight.fill_(weight)
            a.shard_weight = self.weight.data_ptr()
        L.check(L.load().mtbc_eval_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eval_metrics")

    def read(self):
        assert self.table[self.capacity].tolist() == [-7] * 4, "the row behind the table was written"
        assert self.loss_rows[self.capacity].tolist() == [-7.0] * 4, "the row behind the loss rows was written"
        return self.table[:self.capacity].cpu(), self.conf.cpu(), self.loss_rows[:self.capacity].cpu(), self.state.cpu().tolist()


N_SEG, N_CLS = 4099, 5               # 1024 whole 16-byte vectors and three elements behind them; with 4-byte-offset pointers the all-scalar instantiation


def seg_case(seed, offset):
    """fp32 logits with exact zeros (sigmoid = .5, which is NOT > .5), +-tiny values and +-0 among them, a {0, 1} mask."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N_SEG + offset, generator=g) * 3
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1.4e-45, -1.4e-45, 1e-3, -1e-3, 80.0, -80.0, 200.0, -200.0])
    pos = torch.randperm(N_SEG - 3, generator=g)[:4 * len(special)] + offset
    x[pos] = special.repeat(4)
    x[offset + N_SEG - 3:] = torch.tensor([0.0, 2.0, -2.0])  # the three-element tail holds a zero too
    m = (torch.rand(N_SEG + offset, generator=g) < .4).float()
    m[offset + N_SEG - 3:] = 1.0
    x, m = x.to(DEV), m.to(DEV)
    return x[offset:], m[offset:]


def cls_case(n_logits, seed):
    g = torch.Generator().manual_seed(seed)
    if n_logits == 1:
        logits = torch.randn(N_CLS, 1, generator=g)
        logits[:4, 0] = torch.tensor([0.0, 1e-30, -1e-30, float("nan")])        # sigmoid(0) = .5 is not > .5; NaN > .5 is false
        target = torch.tensor([[1.], [1.], [0.], [1.], [0.]])
    else:
        logits = torch.tensor([[2., 2., 1.], [0., 3., 3.], [1., 1., 1.], [float("nan"), 1., float("nan")], [0., 0., -1.]])     # ties, a NaN row
        logits = logits + 0 * torch.randn(N_CLS, 3, generator=g)
        target = torch.nn.functional.one_hot(torch.randint(0, 3, (N_CLS,), generator=g), 3).float()
    return logits.to(DEV), target.to(DEV)


@pytest.mark.parametrize("n_logits", [3, 1])
@pytest.mark.parametrize("offset", [0, 1])
def test_kernel_three_calls_capacity_two(offset, n_logits):
    acc = Acc(2)
    weights = [None, 0.5, None]
    rows, loss_rows, conf_sum = [], [], torch.zeros(3, 3, dtype=torch.int64)
    for k in range(3):
        seg, mask = seg_case(seed=10 + k, offset=offset)
        assert seg.data_ptr() % 16 == (4 if offset else 0) and mask.data_ptr() % 16 == (4 if offset else 0) and seg.numel() == N_SEG
        assert int((seg == 0).sum()) >= 8
        logits, target = cls_case(n_logits, seed=20 + k)
        loss_in = torch.tensor([1.1 + k, 0.3 * (k + 1), 0.7 / (k + 1), 0.0], dtype=torch.float32).to(DEV)
        acc.append(seg, mask, logits, target, loss_in, weight=weights[k])
        if k < 2:
            rows.append(want_row(seg, mask, N_CLS))
            loss_rows.append(want_loss_row(loss_in, 1.0 if weights[k] is None else weights[k]))
            conf_sum += want_conf(logits, target)
    table, conf, lr, state = acc.read()                       # also: the sentinel rows behind the table and the loss rows are untouched
    print("rows", table.tolist(), "want", rows, "loss rows", lr.tolist(), "want", loss_rows)
    assert table.tolist() == rows                             # the third call found the table full: nothing of it anywhere
    assert torch.equal(conf, conf_sum) and int(conf.sum()) == 2 * N_CLS
    assert lr.tolist() == loss_rows and loss_rows[1][0] == 0.5 * float(np.float32(2.1))
    assert state == [3, 1]
    assert all(r[0] and r[1] and r[2] for r in rows)


def test_kernel_empty_shard_only_advances_the_cursor():
    acc = Acc(3)
    seg, mask = seg_case(seed=50, offset=0)
    logits, target = cls_case(3, seed=51)
    loss_in = torch.tensor([0.9, 0.5, 0.4, 0.0], dtype=torch.float32).to(DEV)
    acc.append(seg, mask, logits, target, loss_in)
    acc.append(None, None, None, None, None, n_logits=3)
    acc.append(seg, mask, logits, target, loss_in, weight=0.25)
    table, conf, lr, state = acc.read()
    row = want_row(seg, mask, N_CLS)
    assert table.tolist() == [row, [0, 0, 0, 0], row] and state == [3, 0]
    assert lr.tolist() == [want_loss_row(loss_in), [0.0] * 4, want_loss_row(loss_in, 0.25)]
    assert torch.equal(conf, 2 * want_conf(logits, target))
    acc.append(None, None, None, None, None, n_logits=1)      # behind the table: still only the cursor, and no drop is counted
    assert acc.read()[3] == [4, 0]


# ------------------------------------------------------------------------------------------------ the step, world 1
def build_model(n_classes=3, compute=None, seed=1993):
    seed_everything(seed)
    m = MTnnUNet(1, 1, 1 if n_classes == 2 else n_classes).to(DEV)
    if compute:
        m.set_compute(compute)
    return m


def batches(sizes, size=64, seed0=70, binary=False):
    out = []
    for s, n in enumerate(sizes):
        img, mask, label = O.synthetic_batch(n, size, size, seed=seed0 + s)
        if binary:
            label = (label != 0).float()
        out.append((img.to(DEV), mask.to(DEV), label.to(DEV)))
    return out


def clones_of(step, n, size=64):
    """What the on-device call that has just run read: the loss words, the last head, the mask, the class logits and their target."""
    st = step._compiled(n, size, size)
    return (st.plan.loss_out.clone(), st.segs[-1].data.clone(), st.mask.clone(), st.logits.data.clone().view(n, -1), st.onehot.clone())


def host_result(clones, weights=None):
    rows, loss_rows, conf = [], [], torch.zeros(3, 3, dtype=torch.int64)
    for k, (loss, seg, mask, logits, target) in enumerate(clones):
        rows.append(want_row(seg, mask, logits.shape[0]))
        loss_rows.append(want_loss_row(loss, 1.0 if weights is None else weights[k]))
        conf += want_conf(logits, target)
    return rows, conf.numpy(), loss_rows


@pytest.mark.parametrize("n_classes,compute", [(3, None), (2, None), (3, "bf16")])
def test_on_device_equals_the_host_function_on_its_own_outputs_and_the_default_path(n_classes, compute):
    data = batches([4, 4, 3], binary=n_classes == 2)          # the short last batch compiles a second plan
    model = build_model(n_classes, compute)
    step = T.FusedEvalStep(model, alpha=0.5, n_classes=n_classes, on_device=True)
    assert step.graph is False or os.environ.get("MTBC_GRAPH")
    clones = []
    for img, mask, label in data:
        step(img, mask, label)
        clones.append(clones_of(step, img.shape[0]))
    got = step.result()
    rows, conf, loss_rows = host_result(clones)
    want = T.eval_result_from_counts(rows, conf, loss_rows)
    print(n_classes, compute, "rows", rows, "conf", conf.tolist(), "loss rows", loss_rows, "got", got)
    assert got == want                                        # bit for bit
    assert [r[3] for r in rows] == [4, 4, 3] and int(conf.sum()) == 11
    assert sum(r[0] + r[1] + r[2] for r in rows) > 0 and all(lr[0] > 0 and lr[3] == 0.0 for lr in loss_rows)
    if n_classes == 2:
        assert int(conf[2].sum()) == 0 and int(conf[:, 2].sum()) == 0
    assert step.result() == got                               # reading does not consume
    plain = T.FusedEvalStep(model, alpha=0.5, n_classes=n_classes)
    for img, mask, label in data:
        plain(img, mask, label)
    close6(got, plain.result())
    step.reset()                                              # a second epoch starts from zero in the same buffers
    ptrs = (step._em.data_ptr(), step._em_loss.data_ptr(), step._em_state.data_ptr())
    step(*data[2])
    again = step.result()
    assert again == T.eval_result_from_counts(*host_result([clones_of(step, 3)]))
    assert ptrs == (step._em.data_ptr(), step._em_loss.data_ptr(), step._em_state.data_ptr())


def test_graph_replay_is_bit_equal_to_eager():
    full = batches([4] * 6, seed0=80)
    short = batches([3], seed0=90)[0]
    order = full[:4] + [short] + full[4:]
    model = build_model()
    eager = T.FusedEvalStep(model, alpha=0.5, on_device=True, graph=False)
    graph = T.FusedEvalStep(model, alpha=0.5, on_device=True, graph=True)
    for k, (img, mask, label) in enumerate(order):
        graph(img, mask, label)
        st = graph._compiled(4, 64, 64)
        if k < 2:
            assert graph._graphs[id(st)][2] is None           # eager for the first two calls of the compiled step
        elif k == 2:
            assert graph._graphs[id(st)][2] is not None       # captured at the third
            captured = graph._graphs[id(st)][2]
    assert graph._graphs[id(st)][2] is captured and id(st) not in eager._graphs
    assert graph._graphs[id(graph._compiled(3, 64, 64))][2] is None       # the short shape ran once: eager
    for img, mask, label in order:
        eager(img, mask, label)
    got, want = graph.result(), eager.result()
    print("graph", got, "eager", want)
    assert got == want                                        # bit for bit
    assert graph._em_state.cpu().tolist() == [7, 0] and eager._em_state.cpu().tolist() == [7, 0]
    assert torch.equal(graph._em, eager._em) and torch.equal(graph._em_loss, eager._em_loss)
    assert graph._em[:28].view(7, 4)[:, 3].tolist() == [4, 4, 4, 4, 3, 4, 4]


# ------------------------------------------------------------------------------------------------ the drivers
def store(M, H, W, seed):
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def test_indexed_epoch_with_graph_equals_the_default_step():
    ds = DD.DeviceDataset(*store(11, 64, 64, seed=30))
    tables = DD.EpochTables(EpochIndex(np.arange(11), 4, seed=13), 0, None)
    model = build_model()
    want = T.validate_one_epoch_indexed(T.FusedEvalStep(model, alpha=0.5), ds, tables)
    step = T.FusedEvalStep(model, alpha=0.5, on_device=True, graph=True)
    first = T.validate_one_epoch_indexed(step, ds, tables)    # 4 + 4 + 3: all eager
    second = T.validate_one_epoch_indexed(step, ds, tables)   # the full shape's third call is captured, its fourth replayed
    assert step._graphs[id(step._compiled(4, 64, 64))][2] is not None
    print("default", want, "on device", first, second)
    close6(first, want)
    assert second == first
    assert step._em_state.cpu().tolist() == [3, 0]


def test_capacity_two_with_three_batches_raises():
    model = build_model()
    step = T.FusedEvalStep(model, alpha=0.5, on_device=True, capacity=2)
    data = batches([2, 2, 2])
    for img, mask, label in data:
        step(img, mask, label)
    with pytest.raises(L.MtbcError, match="capacity"):
        step.result()
    step.reset()
    step(*data[0])
    assert len(step.result()) == 6


def test_fit_fold_refuses_a_data_parallel_step_with_a_local_eval_step(tmp_path):
    run_dir = str(tmp_path / "fold_0")
    with pytest.raises(ValueError, match="distributed=True"):
        T.fit_fold(types.SimpleNamespace(distributed=True), types.SimpleNamespace(distributed=False), None, None, None, None, run_dir, epochs=1,
                   max_patience=1, transforms=None, seed=0, plateau=False)
    assert not os.path.exists(run_dir)                        # before anything else happened


def test_fit_fold_two_epochs_equals_the_default_eval_step(tmp_path):
    ds = DD.DeviceDataset(*store(11, 64, 64, seed=33))
    out = []
    for name, kw in (("default", {}), ("device", dict(on_device=True, graph=True))):
        model = build_model(seed=1993)
        opt = FusedAdam(model, lr=1e-3, eps=1e-4)
        step = T.FusedTrainStep(model, opt, alpha=0.5, metrics=True)
        eval_step = T.FusedEvalStep(model, alpha=0.5, **kw)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
        # train 4 + 2, validate 2 + 2 + 1: the full validation shape is captured at its third call (epoch 1) and replayed at its fourth; the
        # (2, 64, 64) plan is shared with the training step's short batch
        rows = T.fit_fold(step, eval_step, ds, EpochIndex(np.arange(6), 4, seed=13), EpochIndex(np.arange(6, 11), 2, seed=13), scheduler,
                          str(tmp_path / name), epochs=2, max_patience=5, transforms=TRANSFORMS, seed=13, plateau=False)
        assert len(rows) == 2
        out.append(rows)
        if kw:
            assert eval_step._graphs[id(eval_step._compiled(2, 64, 64))][2] is not None
    for a, b in zip(*out):
        print("default", a, "device", b)
        assert (a[0], a[1], a[2], a[4], a[6], a[7]) == (b[0], b[1], b[2], b[4], b[6], b[7])      # epoch, lr and the training columns: bit for bit
        assert a[3] == b[3]                                   # val_loss
        assert all(abs(a[i] - b[i]) <= 1e-12 for i in (5, 8, 9))                                 # val_dice, val_acc, val_f1


# ------------------------------------------------------------------------------------------------ two ranks, real kernels
CUTS = [(0, 2, 4), (0, 1, 1)]        # [lo of rank 0, lo of rank 1, end) inside each global batch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model = build_model()
        step = T.FusedEvalStep(model, alpha=0.5, on_device=True, distributed=True)
        clones, weights = [], []
        for b, cut in enumerate(CUTS):
            G = cut[2]
            img, mask, label = O.synthetic_batch(G, 64, 64, seed=7 + b)          # the GLOBAL batch
            lo, hi = cut[rank], cut[rank + 1]
            if hi == lo:
                step.run_empty()
                clones.append(None)
                weights.append(0.0)
                continue
            step(img[lo:hi].to(DEV), mask[lo:hi].to(DEV), label[lo:hi].to(DEV), weight=(hi - lo) / G)
            clones.append(clones_of(step, hi - lo))
            weights.append((hi - lo) / G)
        got = step.result()
        rows, loss_rows, conf = [], [], np.zeros((3, 3), dtype=np.int64)
        for c, w in zip(clones, weights):
            if c is None:
                rows.append([0, 0, 0, 0])
                loss_rows.append([0.0] * 4)
                continue
            r, cf, lr = host_result([c], [w])
            rows.append(r[0])
            loss_rows.append(lr[0])
            conf += cf
        single = None
        if rank == 0:                                         # one process, the default step, the two GLOBAL batches
            plain = T.FusedEvalStep(model, alpha=0.5)
            for b, cut in enumerate(CUTS):
                img, mask, label = O.synthetic_batch(cut[2], 64, 64, seed=7 + b)
                plain(img.to(DEV), mask.to(DEV), label.to(DEV))
            single = plain.result()
        torch.cuda.synchronize()
        q.put((rank, rows, conf, loss_rows, got, single))     # numpy arrays and lists travel by value
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_report_the_global_validation_numbers():
    import time
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got, deadline = [], time.monotonic() + 150
    while len(got) < world and time.monotonic() < deadline:      # ONE attempt: GPU work that did not finish is not run again
        try:
            got.append(q.get(timeout=1))
        except _queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):   # a rank died: its partner would wait for it in a collective
                break
    for p in procs:
        p.join(60 if len(got) == world else 1)
        if p.is_alive():
            p.kill()                      # exactly the processes this test started
            p.join(10)
    assert len(got) == world and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    got.sort(key=lambda t: t[0])
    rows = np.array(got[0][1], dtype=np.int64) + np.array(got[1][1], dtype=np.int64)
    conf = got[0][2] + got[1][2]
    loss_rows = np.array(got[0][3], dtype=np.float64) + np.array(got[1][3], dtype=np.float64)       # two ranks: one commutative add per word
    assert rows[:, 3].tolist() == [4, 1] and got[1][1][1] == [0, 0, 0, 0] and got[1][3][1] == [0.0] * 4 and int(conf.sum()) == 5
    want = T.eval_result_from_counts(rows, conf, loss_rows)
    print("ranks", got[0][4], got[1][4], "host", want, "single process", got[0][5])
    assert got[0][4] == got[1][4] == want                     # both ranks, exactly
    single = got[0][5]
    # shard means and plans of different N round differently: the project's fp32 loss-parity bound
    assert all(abs(want[i] - single[i]) <= 1e-4 for i in range(6)), (want, single)
