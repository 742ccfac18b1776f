"""The data-parallel fused step replayed as hipGraph segments (`FusedTrainStep(distributed=True, graph=True)`): one graph per backward range of
`trainer.plan_segments` plus one for the update, the bucket all-reduces eager between them.  Everything here is held against the EAGER distributed
step, bit for bit: at world 1 with real RCCL collectives on the communication stream, and on two ranks that share the one GPU (gloo as transport:
RCCL refuses two ranks on one device).  No reference counterpart: the reference is single-device (experiment_init.py:339-347)."""
import os
import socket

import numpy as np
import pytest
import torch

from multi_task_breast_cancer_amd import trainer as T
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.nets import MTUNetPlusPlus, Multi_BTSUNet, nnUNet
from multi_task_breast_cancer_amd.optim import FusedAdam
from multi_task_breast_cancer_amd.trainer import FusedTrainStep
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def rccl_world_1():
    """ONE world-1 RCCL group for the whole module (the collectives still launch)."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _net(dtype, reserve=None):
    seed_everything(1993)
    m = MTUNetPlusPlus(in_channels=1, out_channels=1, n_classes=3, deep_supervision=True).to(DEV)
    m.set_compute(dtype)
    if reserve is not None:
        m.coop_reserve_cus = reserve
    return m


def _batch(n, size, seed):
    return tuple(t.to(DEV) for t in O.synthetic_batch(n, size, size, seed=seed))


def _segment_graphs(step, st):
    """How many graphs the step's entry on `st` holds (0: nothing captured) -- the entry's graph slot is ONE object."""
    ent = step._graphs.get(id(st))
    if ent is None or ent[2] is None:
        return 0
    assert isinstance(ent[2], T.SegmentGraphs) and st._graph_ents[id(step)] is ent
    return len(ent[2])


def _steps(dtype, batches, n_buckets, graph, lr_change_at=None, reserve=None):
    """Steps of the distributed step over `batches`; after each one (parameters, gradients, loss words) and the number of captured graphs."""
    m = _net(dtype, reserve)
    opt = FusedAdam(m, lr=1e-4, eps=1e-4)
    step = FusedTrainStep(m, opt, alpha=0.5, distributed=True, n_buckets=n_buckets, graph=graph)
    trace, captured = [], []
    for s, b in enumerate(batches):
        if s == lr_change_at:
            opt.param_groups[0]["lr"] = 2.5e-5                      # what a scheduler does between steps
        l = step(*b)
        trace.append((m.flat_p.clone(), m.flat_g.clone(), l.clone()))
        captured.append(_segment_graphs(step, step._st))
    torch.cuda.synchronize()
    step.check_nan()                                                # raises MtbcError on a non-zero cooperative error word
    assert m.coop_error_word() is None or int(m.coop_error_word().item()) == 0
    return trace, captured, step


def _same_traces(eager, graph, what):
    assert len(eager) == len(graph)
    for s, (a, b) in enumerate(zip(eager, graph)):
        for x, y, name in zip(a, b, ("parameters", "gradients", "loss words")):
            assert torch.equal(x, y), f"{what}, step {s + 1}: {name} differ, max |diff| {(x - y).abs().max().item():.3e}"


@pytest.mark.parametrize("n_buckets", [1, 4, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_segment_replay_is_the_eager_distributed_step(rccl_world_1, dtype, n_buckets):
    """Six steps on six batches, the learning rate changed before the fifth: calls 1 and 2 run eager, the third captures, 3 .. 6 are replays; after
    every step parameters, gradients and loss words are those of the eager distributed twin.  The entry holds one graph per non-empty backward
    range plus the update's."""
    batches = [_batch(2, 64, 40 + s) for s in range(6)]
    eager, none, twin = _steps(dtype, batches, n_buckets, graph=False, lr_change_at=4)
    assert none == [0] * 6 and not twin._graphs                     # graph=False never makes an entry
    graph, captured, step = _steps(dtype, batches, n_buckets, graph=True, lr_change_at=4)
    st = step._st
    assert len(st.buckets) == n_buckets
    segs = T.plan_segments(st.buckets, st.programs["bwd"].n)
    assert segs[0][1] > 0                                           # the first range is never empty in this model: it opens the first graph
    expected = sum(1 for _, count, _ in segs if count > 0) + 1
    print(f"{dtype} {n_buckets} buckets: ranges {[(f, c) for f, c, _ in segs]} of {st.programs['bwd'].n} ops, {expected} graphs")
    assert captured == [0, 0] + [expected] * 4, captured
    assert any(e[2] is not None for e in step._graphs.values())
    assert len(st._dp_events) == n_buckets
    _same_traces(eager, graph, f"{dtype}, {n_buckets} buckets")


def test_segment_replay_beside_rccl_at_the_bench_plane_size(rccl_world_1, monkeypatch):
    """The shapes of test_rccl_collectives_beside_the_cooperative_kernels_at_the_bench_plane_size: bf16, 2 x 256 x 256, planned with a reserve of
    64 CUs as an 8-rank trainer plans it, 4 buckets -- the cooperative InstanceNorm launches replayed from graphs beside real RCCL kernels."""
    monkeypatch.setenv("MTBC_COOP_RESERVE_CUS", "64")
    batches = [_batch(2, 256, 60 + s) for s in range(5)]
    eager, _, twin = _steps("bf16", batches, 4, graph=False, reserve=64)
    graph, captured, step = _steps("bf16", batches, 4, graph=True, reserve=64)
    assert twin.model.coop_reserve_cus == 64 == step.model.coop_reserve_cus
    assert step.model.coop_error_word() is not None and int(step.model.coop_error_word().item()) == 0
    assert captured[:2] == [0, 0] and captured[2] > 1 and captured[2:] == [captured[2]] * 3
    _same_traces(eager, graph, "bf16 256 x 256")


def test_segment_replay_with_metrics_and_a_dynamic_scale_skips_and_applies(rccl_world_1):
    """fp16 from a loss scale of 2^40 on one repeated batch, metrics on: the overflowing steps are skipped (sixteen of them, as
    tests/test_loss_scale_gpu.py sees), then updates are applied -- both kinds among the replayed steps 3 .. 20.  Skip count, scale, parameters,
    moments and the metrics table equal the eager distributed run's."""
    batch = _batch(2, 64, 31)
    runs = []
    for graph in (False, True):
        m = _net("f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        sc = DynamicLossScale(init_scale=2.0 ** 40, growth_interval=10 ** 6)
        step = FusedTrainStep(m, opt, alpha=0.35, distributed=True, n_buckets=4, graph=graph, loss_scale=sc, metrics=True, metrics_capacity=32)
        step.begin_epoch_metrics()
        stats = []
        for s in range(20):
            step(*batch)
            stats.append(sc.stats())
        torch.cuda.synchronize()
        step.check_nan()
        assert (_segment_graphs(step, step._st) > 1) == graph
        runs.append(dict(stats=stats, p=m.flat_p.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), metrics=step.epoch_metrics(),
                         counts=step._table.counts.clone(), state=step._table.state.clone()))
    e, g = runs
    print("eager:", e["stats"][-1], "replayed:", g["stats"][-1])
    replayed = g["stats"][2:]                                       # the states behind steps 3 .. 20
    assert replayed[-1]["skipped"] > g["stats"][1]["skipped"], "no replayed step was skipped: the test would show nothing"
    assert replayed[-1]["t"] > g["stats"][1]["t"], "no replayed step was applied: the test would show nothing"
    assert g["stats"] == e["stats"]
    for k in ("p", "m", "v", "counts", "state"):
        assert torch.equal(e[k], g[k]), k
    me, mg = e["metrics"], g["metrics"]
    assert mg.batches == 20 and mg.table.tolist() == me.table.tolist() and np.array_equal(mg.conf, me.conf)
    assert (mg.dice, mg.accuracy, mg.f1) == (me.dice, me.accuracy, me.f1)


def test_refusals_stay_with_graph_on(rccl_world_1):
    with pytest.raises(NotImplementedError, match="data parallel"):
        FusedTrainStep(Multi_BTSUNet(1, 1, 3, 8, True), None, alpha=0.35, distributed=True, graph=True)
    m = nnUNet(1, 1).to(DEV)
    with pytest.raises(NotImplementedError):
        FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), distributed=True, graph=True)


# ------------------------------------------------------------------------------------------------ two ranks on the one GPU
STEPS = 5


def _shard(rank, world, G, cuts):
    if cuts is None:
        per = G // world
        return slice(rank * per, (rank + 1) * per), None            # equal contiguous shards
    return slice(cuts[rank], cuts[rank + 1]), (cuts[rank + 1] - cuts[rank]) / G      # EpochIndex.weights


def _worker(rank, world, port, q, G, cuts, mode):
    """mode "twin": an eager and a replaying distributed step side by side in each rank (the collectives pair up: both ranks issue them in the same
    order), compared after every step where they live; rank 0 reports the verdicts and its first step.  mode "empty": one replaying step; in step 4
    rank 1's shard is empty (`run_empty()`) while rank 0 replays the whole batch; both ranks report their parameters."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sl, weight = _shard(rank, world, G, cuts)
        data = [O.synthetic_batch(G, 64, 64, seed=7 + s) for s in range(STEPS)]              # the GLOBAL batches
        if mode == "twin":
            arms = []
            for graph in (False, True):
                m = _net("fp32")
                arms.append((m, FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5, distributed=True, n_buckets=4, graph=graph)))
            equal, first = [], None
            for s, (img, mask, label) in enumerate(data):
                out = [step(img[sl].to(DEV), mask[sl].to(DEV), label[sl].to(DEV), weight=weight) for _, step in arms]
                torch.cuda.synchronize()
                (me, _), (mg, sg) = arms
                equal.append([bool(torch.equal(me.flat_p, mg.flat_p)), bool(torch.equal(me.flat_g, mg.flat_g)), bool(torch.equal(out[0], out[1]))])
                if s == 0:          # numpy arrays travel by value; CPU tensors would travel as shared-memory handles that die with this process
                    first = (mg.flat_p.cpu().numpy(), mg.flat_g.cpu().numpy(), out[1].cpu().numpy())
            if rank == 0:
                q.put((0, equal, first, _segment_graphs(sg, sg._st), len(arms[0][1]._graphs)))
        else:
            m = _net("fp32")
            step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5, distributed=True, n_buckets=4, graph=True)
            per = G // world
            for s, (img, mask, label) in enumerate(data):
                if s == 3 and rank == 1:
                    step.run_empty()
                elif s == 3:                                        # the whole (short) global batch is rank 0's: weight n_local / n_batch = 1
                    step(img[:per].to(DEV), mask[:per].to(DEV), label[:per].to(DEV), weight=1.0)
                else:
                    step(img[sl].to(DEV), mask[sl].to(DEV), label[sl].to(DEV), weight=weight)
            torch.cuda.synchronize()
            step.check_nan()
            q.put((rank, m.flat_p.cpu().numpy(), _segment_graphs(step, step._st)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _two_ranks(G, cuts, mode, n_results):
    """The spawn / queue / kill pattern of tests/test_dp_gpu.py: two children at a time, exactly the processes started here are reaped."""
    import queue as _queue
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    got = None
    for attempt in range(2):          # a 2-process gloo rendezvous on one box has been seen to stall once
        q, port = ctx.Queue(), _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q, G, cuts, mode)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            got = [q.get(timeout=120) for _ in range(n_results)]
        except _queue.Empty:
            got = None
        for p in procs:
            p.join(60 if got is not None else 1)
            if p.is_alive():
                p.kill()
                p.join(10)
        if got is not None:
            assert all(p.exitcode == 0 for p in procs)
            break
    assert got is not None, "the two-rank run produced no result in two attempts"
    return sorted(got, key=lambda r: r[0])


@pytest.mark.parametrize("G,cuts", [(4, None), (5, (0, 3, 5))])
def test_two_rank_segment_replay_is_the_two_rank_eager_step(G, cuts):
    """Five steps on two ranks, equal and uneven shards: rank 0's parameters, gradients and losses after every step are bit-equal between the replaying
    and the eager distributed step (a two-term sum does not depend on its order); after step 1 the bounds of
    test_two_rank_step_equals_single_rank_global_batch against the single-rank step on the global batch hold."""
    (_, equal, first, n_graphs, eager_entries), = _two_ranks(G, cuts, "twin", 1)
    assert n_graphs > 1 and eager_entries == 0
    assert equal == [[True, True, True]] * STEPS, equal
    p2, g2, l2 = (torch.from_numpy(a) for a in first)
    m = _net("fp32")
    step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5)
    l1 = step(*_batch(G, 64, 7)).cpu()
    p1, g1 = m.flat_p.cpu(), m.flat_g.cpu()
    g2 = g2 / 2
    rel = (g2 - g1).norm().item() / g1.norm().item()
    print(f"G={G} cuts={cuts}: gradient rel {rel:.3e}, parameters max |diff| {(p2 - p1).abs().max().item():.3e}")
    assert rel < 1e-5, rel
    assert (p2 - p1).abs().max().item() < 2e-6
    assert l2[3].item() == 0.0 and abs(l1[0].item()) > 0


def test_an_empty_shard_pairs_its_collectives_with_a_replaying_rank():
    """After three full steps rank 1's shard is empty: `run_empty()` stays eager and issues the same collectives, rank 0 replays; a fifth full step
    follows.  The run finishes and both ranks hold the same parameters, bit for bit."""
    (_, p0, n0), (_, p1, n1) = _two_ranks(4, None, "empty", 2)
    assert n0 > 1 and n1 > 1
    assert np.array_equal(p0, p1) and np.isfinite(p0).all()
