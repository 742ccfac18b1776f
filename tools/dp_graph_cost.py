#!/usr/bin/env python3
"""What the host spends issuing a data-parallel training step, eager against replayed as hipGraph segments (profiles/dp_graph_replay.txt).

    python tools/dp_graph_cost.py bf16 32 256            # dtype, batch, size [, n_buckets = 4]: the bench shape
    python tools/dp_graph_cost.py fp16 16 512

ONE process, ONE rank: a world-1 RCCL group, so that the bucket all-reduces are real RCCL launches on the communication stream (planned with the
cooperative reserve an 8-rank trainer plans with).  Nothing here says anything about 8 GPUs: the scaling curve is the driver's to measure.
Four arms on twin models, interleaved, four rounds of 50 steps after 10 warm-up steps each (plans, kernels, the allocator, the captures):

    eager DP        FusedTrainStep(distributed=True, graph=False): the eager distributed step, launch for launch what it was
    eager DP (A/A)  the same again on a twin: the difference between these two is the spread of this box, the yardstick for every other difference
    segments        FusedTrainStep(distributed=True, graph=True): one hipGraph per backward range + one for the update, collectives eager between
    single graph    FusedTrainStep(graph=True), not distributed: the whole step as ONE hipGraph, no collective -- the floor

Per arm and round: HOST issue time per step (a host clock around the issuing loop, no synchronisation inside, stopped before the synchronise) and
ms per step between synchronisations (the same clock stopped behind it).  Then one more run of the segmented arm with a clock around every graph
launch and around the eager work between the segments (event record, wait, all-reduce call; the join), which splits its host time three ways.
Needs a GPU (no fallback)."""
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_task_breast_cancer_amd import _lib as L                               # noqa: E402
from multi_task_breast_cancer_amd import trainer as T                            # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model, init_optimizer    # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything              # noqa: E402
from multi_task_breast_cancer_amd.synthetic import synthetic_batch               # noqa: E402

STEPS, WARMUP, ROUNDS = 50, 10, 4
RESERVE = "64"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    dtype, N, S = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    n_buckets = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    L.require_gpu()
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    os.environ.setdefault("MTBC_COOP_RESERVE_CUS", RESERVE)      # world 1 plans like world 8
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        run(dtype, N, S, n_buckets, dev)
    finally:
        dist.destroy_process_group()


def run(dtype, N, S, n_buckets, dev):
    batches = [synthetic_batch(N, S, S, seed=s, device=dev) for s in range(2)]
    reserve = int(os.environ["MTBC_COOP_RESERVE_CUS"])
    arms = {}
    for name, kw in (("eager DP", dict(distributed=True, graph=False)), ("eager DP (A/A)", dict(distributed=True, graph=False)),
                     ("segments", dict(distributed=True, graph=True)), ("single graph", dict(distributed=False, graph=True))):
        seed_everything(1993)
        model = init_multitask_model("MTUNetPlusPlus", sequences=1, regions=1, n_classes=3, deep_supervision=True).to(dev)
        model.set_compute(dtype)
        model.coop_reserve_cus = reserve                          # every arm runs the same kernels with the same grids
        step = T.FusedTrainStep(model, init_optimizer(model, "Adam", 1e-4), alpha=0.5, inversely_weighted=True, n_buckets=n_buckets, **kw)
        for i in range(WARMUP):
            step(*batches[i % 2])
        torch.cuda.synchronize()
        step.check_nan()
        arms[name] = (model, step)
    seg = arms["segments"][1]
    st = seg._st
    ent = seg._graphs[id(st)]
    ranges = T.plan_segments(st.buckets, st.programs["bwd"].n)
    assert isinstance(ent[2], T.SegmentGraphs) and not arms["eager DP"][1]._graphs
    print(f"== U-Net++ (deep supervision) {dtype}, batch {N}, {S} x {S}, world-1 RCCL, {len(st.buckets)} buckets, cooperative reserve {reserve} CUs: "
          f"backward of {st.programs['bwd'].n} ops cut into ranges {[(f, c) for f, c, _ in ranges]} -> {len(ent[2])} graphs; "
          f"{ROUNDS} rounds of {STEPS} steps after {WARMUP} warm-up steps per arm, interleaved in one process")
    rows = {name: [] for name in arms}
    for r in range(ROUNDS):
        for name, (model, step) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(STEPS):
                step(*batches[i % 2])
            issue = time.perf_counter() - t0
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            rows[name].append((1e3 * issue / STEPS, 1e3 * total / STEPS))
            print(f"round {r + 1} [{name:14s}] host issue {rows[name][-1][0]:7.3f} ms per step | {rows[name][-1][1]:8.3f} ms per step", flush=True)
    mean = {name: np.mean(np.array(v), axis=0) for name, v in rows.items()}
    base = mean["eager DP"]
    for name in arms:
        m = mean[name]
        print(f"   mean [{name:14s}] host issue {m[0]:7.3f} ms ({m[0] - base[0]:+7.3f} against eager DP) | {m[1]:8.3f} ms per step ({m[1] - base[1]:+7.3f} ms, "
              f"{100 * (m[1] - base[1]) / base[1]:+6.2f} %)")
    spread = abs(mean["eager DP (A/A)"][1] - base[1])
    over = mean["segments"][1] - base[1]
    print(f"   spread between the two identical eager arms: {spread:.3f} ms per step; segments against eager DP: {over:+.3f} ms per step "
          f"({'within' if over <= spread else 'OUTSIDE'} the spread)")
    print(f"   host issue, segments: {mean['segments'][0]:.3f} ms per step against {base[0]:.3f} eager (the bar of this item: <= 1.5 ms at bf16 32 256); "
          f"the single graph, with no collective to issue: {mean['single graph'][0]:.3f} ms")

    pe = arms["eager DP"][0].flat_p
    same = {name: bool(torch.equal(pe, model.flat_p)) for name, (model, _) in arms.items() if name != "eager DP"}
    print(f"   parameters after {WARMUP + ROUNDS * STEPS} steps, bit-identical to eager DP's: {same}")
    assert all(same.values())

    # ---- where the segmented step's host time goes: the replay branch of trainer.run_or_replay_segments with a clock around each part
    acc = {"launch": 0.0, "between": 0.0}
    real = T.run_or_replay_segments

    def clocked(owner, st_, key, bodies, between, **kw):
        e = owner._graphs[id(st_)]
        assert e[0] == key and e[2] is not None
        for i, g in enumerate(e[2].graphs):
            t0 = time.perf_counter()
            g.replay()
            t1 = time.perf_counter()
            between(i)
            acc["launch"] += t1 - t0
            acc["between"] += time.perf_counter() - t1

    T.run_or_replay_segments = clocked
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(STEPS):
            seg(*batches[i % 2])
        issue = time.perf_counter() - t0
        torch.cuda.synchronize()
    finally:
        T.run_or_replay_segments = real
    ms = {k: 1e3 * v / STEPS for k, v in acc.items()}
    print(f"   segments, host time per step with a clock around each part ({STEPS} steps): {1e3 * issue / STEPS:.3f} ms = {ms['launch']:.3f} in {len(ent[2])} "
          f"graph launches + {ms['between']:.3f} in the event / wait / all-reduce calls and the join + {1e3 * issue / STEPS - ms['launch'] - ms['between']:.3f} "
          f"in front of them (the batch fill, the optimizer's four scalar fills, building the segment list)")
    for name, (model, step) in arms.items():
        step.check_nan()


if __name__ == "__main__":
    main()
