"""The device-side validation epoch without a GPU: the declaration, export and binding of mtbc_eval_metrics and the layout of its argument
struct against the C compiler's, the refusals that answer before any launch, the host arithmetic on (table, conf, loss_rows) against a
restatement of the reference's validation loop (training_multitask.py:119-159), `dice_score_from_tensor` (metrics.py:255-267) and sklearn,
the refusals of the packed arrays, and the merge of two ranks' accumulators over gloo."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd import trainer as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")


# ------------------------------------------------------------------------------------------------ declaration, binding, layout
def test_export_is_declared_and_bound():
    src = open(HEADER).read()
    assert re.search(r"\bint\s+mtbc_eval_metrics\s*\(\s*const\s+mtbc_eval_metrics_args\s*\*\s*\w+\s*,\s*void\s*\*", src)
    assert "mtbc_eval_metrics" in L.EXPORTS
    lib = L.load()
    assert hasattr(lib, "mtbc_eval_metrics")
    assert lib.mtbc_eval_metrics.argtypes[0]._type_ is L.EvalMetricsArgs and lib.mtbc_eval_metrics.restype is C.c_int
    assert int(re.search(r"#define\s+MTBC_VERSION\s+(\d+)", src).group(1)) == 203
    assert lib.mtbc_version() == 203 == L.ABI_VERSION              # additive: no existing layout moved
    # the mirror names the header's fields in the header's order
    body = src[src.index("typedef struct {", src.index("validation-epoch metrics")):src.index("} mtbc_eval_metrics_args;")]
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in L.EvalMetricsArgs._fields_], names
    assert names[:11] == [f[0] for f in L.TrainMetricsArgs._fields_]


def test_ctypes_layout_matches_the_compiled_struct(tmp_path):
    fields = [f[0] for f in L.EvalMetricsArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(mtbc_eval_metrics_args));']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(mtbc_eval_metrics_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["sizeof"]) == C.sizeof(L.EvalMetricsArgs) == 104
    for f in fields:
        assert int(got[f]) == getattr(L.EvalMetricsArgs, f).offset, f
    assert L.EvalMetricsArgs.loss_in.offset == 80 and L.EvalMetricsArgs.shard_weight.offset == 96


def test_refusals_answer_before_any_launch():
    """Argument checks are host code: these calls return before a GPU call is made."""
    lib = L.load()
    BADSHAPE, BADARG = -1, -2
    assert lib.mtbc_eval_metrics(None, None) == BADARG                         # a null args pointer
    a = L.EvalMetricsArgs()
    a.n_logits, a.capacity = 3, 1
    assert lib.mtbc_eval_metrics(C.byref(a), None) == BADARG                   # a null table (and conf, state)
    buf = (C.c_int64 * 16)()
    a.conf = a.state = C.addressof(buf)
    assert lib.mtbc_eval_metrics(C.byref(a), None) == BADARG                   # the table alone is null
    a.table = C.addressof(buf)
    for bad in (0, 4):
        a.n_logits = bad
        assert lib.mtbc_eval_metrics(C.byref(a), None) == BADSHAPE, bad
    a.n_logits, a.N, a.n_seg = 3, 0, 64
    assert lib.mtbc_eval_metrics(C.byref(a), None) == BADSHAPE                 # pixels without samples
    data = (C.c_float * 64)()
    a.N, a.n_seg = 2, 64
    a.seg_logits = a.mask = a.cls_logits = a.target = a.loss_in = C.addressof(data)
    a.loss_rows = None
    assert lib.mtbc_eval_metrics(C.byref(a), None) == BADARG                   # N > 0 with a null loss_rows
    a.loss_rows, a.loss_in = C.addressof(buf), None
    assert lib.mtbc_eval_metrics(C.byref(a), None) == BADARG                   # ... or a null loss_in


# ------------------------------------------------------------------------------------------------ the host function
def dice_score_from_tensor(gt: torch.Tensor, seg: torch.Tensor):
    """metrics.py:255-267, restated."""
    gt = gt.double()
    seg = seg.double()
    tp = torch.sum(torch.logical_and(seg, gt)).double()
    fp = torch.sum(torch.logical_and(seg, torch.logical_not(gt))).double()
    fn = torch.sum(torch.logical_and(torch.logical_not(seg), gt)).double()
    if torch.sum(gt) == 0:
        dice = 1 if torch.sum(seg) == 0 else 0
    else:
        dice = 2 * tp / (2 * tp + fp + fn)
    return dice


def counts_row(gt: torch.Tensor, seg: torch.Tensor, n: int):
    g, s = gt.bool(), seg.bool()
    return [int((s & g).sum()), int((s & ~g).sum()), int((~s & g).sum()), n]


def mask_batches(seed: int):
    """Per-batch (samples, ground truth, prediction): random ones, an empty ground truth with and without predictions, an empty prediction."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n, p_gt, p_seg in [(4, .3, .3), (4, .5, .1), (4, .02, .6), (3, .9, .9)]:
        out.append((n, torch.rand(n, 1, 17, 30, generator=g) < p_gt, torch.rand(n, 1, 17, 30, generator=g) < p_seg))
    z = torch.zeros(2, 1, 17, 30, dtype=torch.bool)
    some = torch.rand(2, 1, 17, 30, generator=g) < .2
    out += [(2, z, z), (2, z, some), (2, some, z)]
    return out


def reference_loop(loss_words, dices):
    """training_multitask.py:121-123, :140-153: float64 `+=` of the float32 `.item()`s, then `/ len(val_loader)`."""
    val_loss, seg_val_loss, cls_val_loss, val_dice = 0., 0., 0., 0.
    for (total, seg, cls), d in zip(loss_words, dices):
        val_loss += total.item()
        seg_val_loss += seg.item()
        cls_val_loss += cls.item()
        val_dice += d
    n = len(loss_words)
    return val_loss / n, float(val_dice / n), seg_val_loss / n, cls_val_loss / n


@pytest.mark.filterwarnings("ignore")                   # sklearn warns where a class has no predicted samples (and scores it 0)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_function_equals_the_reference_loop(seed):
    from sklearn.metrics import accuracy_score, f1_score
    batches = mask_batches(seed)
    table = np.array([counts_row(gt, seg, n) for n, gt, seg in batches], dtype=np.int64)
    assert table[4].tolist()[:3] == [0, 0, 0] and table[5, 1] > 0 and table[5, 0] + table[5, 2] == 0
    rng = np.random.default_rng(seed)
    words = torch.from_numpy((rng.random((len(batches), 3)) * 3).astype(np.float32))
    loss_rows = np.zeros((len(batches), 4), dtype=np.float64)
    loss_rows[:, :3] = words.numpy().astype(np.float64)                    # what the kernel stores: 1 * (double)word
    n_all = int(table[:, 3].sum())
    gt, pred = rng.integers(0, 3, n_all), rng.integers(0, 3 if seed else 2, n_all)          # seed 0: class 2 is never predicted
    conf = np.zeros((3, 3), dtype=np.int64)
    for g, p in zip(gt, pred):
        conf[g, p] += 1
    got = T.eval_result_from_counts(table, conf, loss_rows)
    dices = [dice_score_from_tensor(g, s) for _, g, s in batches]
    assert [float(d) for d in dices[4:]] == [1.0, 0.0, 0.0]
    want_loss, want_dice, want_seg, want_cls = reference_loop([tuple(w) for w in words], dices)
    assert len(got) == 6
    assert (got[0], got[4], got[5]) == (want_loss, want_seg, want_cls)     # bit for bit
    assert got[1] == want_dice
    want_acc = accuracy_score(gt.tolist(), pred.tolist())
    want_f1 = f1_score(y_true=gt.tolist(), y_pred=pred.tolist(), labels=[0, 1, 2], average='weighted')
    assert abs(got[2] - want_acc) <= 1e-12 and abs(got[3] - want_f1) <= 1e-12, (got, want_acc, want_f1)


# ------------------------------------------------------------------------------------------------ the packed arrays
def _accumulators(cap, rows, conf, loss_rows, cursor, dropped=0):
    table = torch.zeros(cap, 4, dtype=torch.int64)
    table[:len(rows)] = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    losses = torch.zeros(cap, 4, dtype=torch.float64)
    losses[:len(loss_rows)] = torch.tensor(loss_rows, dtype=torch.float64).reshape(-1, 4)
    return table, torch.tensor(conf, dtype=torch.int64), torch.tensor([cursor, dropped], dtype=torch.int32), losses


def test_packed_arrays_refuse_a_full_table_unequal_cursors_and_a_nan_word():
    cap = 3
    rows, conf = [[5, 1, 2, 4], [0, 0, 0, 4]], [[3, 0, 0], [1, 2, 0], [0, 0, 2]]
    loss_rows = [[0.75, 0.5, 0.25, 0.0], [1.5, 1.0, 0.5, 0.0]]
    table, cf, state, losses = _accumulators(cap, rows, conf, loss_rows, 2)
    packed, lr = T.reduce_eval_metrics(table, cf, state, losses)
    assert packed.dtype == np.int64 and packed.shape == (cap * 4 + 13,) and packed[-4:].tolist() == [2, 4, 0, 0]
    assert lr.dtype == np.float64 and lr.shape == (cap * 4,)
    got = T.eval_result_from_packed(packed, lr, cap)
    assert got == T.eval_result_from_counts(rows, conf, loss_rows)
    assert got[0] == (0.75 + 1.5) / 2 and got[1] == (2 * 5 / (2 * 5 + 1 + 2) + 1.0) / 2 and got[4] == 0.75 and got[5] == 0.375
    # a full table: the fourth batch found no row
    full = T.reduce_eval_metrics(*_accumulators(cap, rows, conf, loss_rows, 4, dropped=1)[:3], losses)
    with pytest.raises(L.MtbcError, match="capacity"):
        T.eval_result_from_packed(*full, cap)
    two = packed.copy()
    two[cap * 4 + 9:cap * 4 + 12] = [2 + 3, 4 + 9, 0]     # what the sum over a rank at cursor 2 and one at cursor 3 looks like
    with pytest.raises(L.MtbcError, match="different numbers of batches"):
        T.eval_result_from_packed(two, lr, cap, world=2)
    err = packed.copy()
    err[-1] = 1                                          # the cooperative-InstanceNorm error word of some rank
    with pytest.raises(L.MtbcError, match="cooperative InstanceNorm"):
        T.eval_result_from_packed(err, lr, cap)
    with pytest.raises(L.MtbcError, match="before any batch"):
        T.eval_result_from_packed(*T.reduce_eval_metrics(*_accumulators(cap, [], conf, [], 0)), cap)
    # a NaN word in any row: the reference's guard, log + exit(1)
    nan = lr.copy()
    nan[1 * 4 + 3] = 1.0
    with pytest.raises(SystemExit) as e:
        T.eval_result_from_packed(packed, nan, cap)
    assert e.value.code == 1


# ------------------------------------------------------------------------------------------------ two ranks over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_accumulators(rank: int, cap: int):
    """What each rank's device would hold after two global batches of 4 and 1 samples cut 2 + 2 and 1 + 0: rank 1's second shard is empty (its
    row stays zero, its cursor advanced).  Loss words are float32 shard means, stored as weight * (double)word."""
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(5, 1, 17, 30, generator=g) < .3
    seg = torch.rand(5, 1, 17, 30, generator=g) < .3
    labels, preds = [0, 1, 2, 2, 1], [0, 2, 2, 1, 1]
    words = torch.rand(2, 2, 3, generator=g, dtype=torch.float32)            # [batch][rank][total, seg, cls]
    cuts = [(0, 2, 4), (4, 5, 5)]
    weights = [(0.5, 0.5), (1.0, 0.0)]
    rows, loss_rows = [], []
    conf = np.zeros((3, 3), dtype=np.int64)
    for b, c in enumerate(cuts):
        lo, hi = c[rank], c[rank + 1]
        if hi == lo:
            rows.append([0, 0, 0, 0])
            loss_rows.append([0.0] * 4)
            continue
        rows.append(counts_row(gt[lo:hi], seg[lo:hi], hi - lo))
        loss_rows.append([weights[b][rank] * float(w) for w in words[b, rank]] + [0.0])
        for gl, pl in zip(labels[lo:hi], preds[lo:hi]):
            conf[gl, pl] += 1
    return rows, conf, loss_rows


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cap = 5
        rows, conf, loss_rows = _rank_accumulators(rank, cap)
        acc = _accumulators(cap, rows, conf.tolist(), loss_rows, 2)
        before = [t.clone() for t in acc]
        got = T.eval_result_from_packed(*T.reduce_eval_metrics(*acc, distributed=True), cap, world)
        assert all(torch.equal(a, b) for a, b in zip(before, acc))           # the accumulators are left as they were
        # the hand-summed rows: for two ranks the float64 sum is one commutative add per word
        r0, c0, l0 = _rank_accumulators(0, cap)
        r1, c1, l1 = _rank_accumulators(1, cap)
        assert r1[1] == [0, 0, 0, 0] and l1[1] == [0.0] * 4
        want = T.eval_result_from_counts(np.array(r0) + np.array(r1), c0 + c1, np.array(l0, dtype=np.float64) + np.array(l1, dtype=np.float64))
        assert got == want, (got, want)
        q.put((rank, got))
    finally:
        dist.destroy_process_group()


def test_two_ranks_merge_into_the_same_six_numbers_over_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    got = sorted(q.get(timeout=5) for _ in range(world))
    assert [g[0] for g in got] == [0, 1] and got[0][1] == got[1][1] and len(got[0][1]) == 6
    assert got[0][1][2] == 3 / 5                        # accuracy over the five samples of both ranks


def test_new_keywords_are_off_by_default_and_checked():
    """The constructor's refusals are host logic; no model is touched."""
    import inspect
    sig = inspect.signature(T.FusedEvalStep.__init__).parameters
    assert (sig["on_device"].default, sig["graph"].default, sig["distributed"].default, sig["capacity"].default) == (False, None, False, 4096)

    class Net:
        n_classes = 3
    step = T.FusedEvalStep(Net(), alpha=0.5)
    assert (step.on_device, step.graph, step.distributed) == (False, False, False)
    with pytest.raises(ValueError, match="on_device"):
        T.FusedEvalStep(Net(), alpha=0.5, graph=True)
    with pytest.raises(ValueError, match="on_device"):
        T.FusedEvalStep(Net(), alpha=0.5, distributed=True)
    with pytest.raises(ValueError, match="capacity"):
        T.FusedEvalStep(Net(), alpha=0.5, on_device=True, capacity=0)
    assert T.FusedEvalStep(Net(), alpha=0.5, on_device=True, graph=True).graph is True
