"""The device-side dynamic loss scale (loss_scale.DynamicLossScale, mtbc_loss_scale_*), through the C-ABI on the GPU: the found-inf pass, the
skipped / applied Adam launch and the state update at op level, then whole training steps -- without an overflow bit-equal to the static scale,
with one skipped and recovered from -- eager, as a hipGraph replay and under data parallel."""
import ctypes as C
import os
import socket

import pytest
import torch

from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd import ops
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.nets import MTUNetPlusPlus
from multi_task_breast_cancer_amd.optim import FusedAdam
from multi_task_breast_cancer_amd.trainer import FusedTrainStep
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BIG = 2.0 ** 40           # a loss scale under which the first backward overflows an fp16 MFMA operand (asserted below, not assumed)


def _net(dtype):
    seed_everything(1993)
    m = MTUNetPlusPlus(in_channels=1, out_channels=1, n_classes=3, deep_supervision=True).to(DEV)
    m.set_compute(dtype)
    return m


def _state(**fields):
    h = L.LossScaleState()
    h.scale, h.shard_weight = 65536.0, 1.0
    for k, v in fields.items():
        setattr(h, k, v)
    return torch.frombuffer(bytearray(bytes(h)), dtype=torch.int32).clone().to(DEV)


def _read(state):
    return L.LossScaleState.from_buffer_copy(state.cpu().numpy().tobytes())


def _batch(n, size, seed):
    return tuple(t.to(DEV) for t in O.synthetic_batch(n, size, size, seed=seed))


# ------------------------------------------------------------------------------------------------ op level
def test_check_kernel_finds_every_non_finite_value():
    n = MTUNetPlusPlus(in_channels=1, out_channels=1, n_classes=3, deep_supervision=True).flat_numel
    gen = torch.Generator(device="cpu").manual_seed(7)
    g = (torch.randn(n, generator=gen) * 1e3).to(DEV)
    g[1], g[2] = 3.4e38, -1e-45                                   # the largest exponent that is still finite; a subnormal
    state = _state()
    ops.loss_scale_check(state, g)
    assert _read(state).found_inf == 0
    short = g[:n - 3]                                             # not a multiple of 4 long: the last elements go through the scalar tail
    assert short.numel() % 4 != 0
    ops.loss_scale_check(state, short)
    assert _read(state).found_inf == 0
    rnd = int(torch.randint(0, n, (1,), generator=gen))
    for val in (float("inf"), float("-inf"), float("nan")):
        for buf, idx in ((g, 0), (g, n - 1), (g, n - 2), (g, rnd), (short, short.numel() - 1), (short, 0)):
            keep = buf[idx].clone()
            buf[idx] = val
            state = _state()
            ops.loss_scale_check(state, buf)
            assert _read(state).found_inf == 1, (val, idx)
            buf[idx] = keep
        # one element PAST the end of the shorter buffer is not the check's business
        keep = g[n - 3].clone()
        g[n - 3] = val
        state = _state()
        ops.loss_scale_check(state, short)
        assert _read(state).found_inf == 0, val
        g[n - 3] = keep
    # the word is sticky until the update clears it
    g[5] = float("inf")
    state = _state()
    ops.loss_scale_check(state, g)
    g[5] = 0.0
    ops.loss_scale_check(state, g)
    assert _read(state).found_inf == 1


def _ulps(a: float, b: float) -> int:
    ia, ib = (int.from_bytes(bytes(C.c_float(v)), "little") for v in (a, b))
    return abs(ia - ib)


def test_update_applies_adam_or_skips_it():
    """Clear word: the launch is ops.adam_step(grad_scale = (1 / world) / scale, step = t + 1) bit for bit, given the device's bias corrections equal the
    host's (asserted first: both in double, rounded once; 1 ulp allowed, t = 1, 2, 3 must be equal).  Set word: nothing but the scale state moves."""
    n = 1_000_003
    gen = torch.Generator(device="cpu").manual_seed(3)
    p0, g0 = torch.randn(n, generator=gen).to(DEV), (torch.randn(n, generator=gen) * 65536.0).to(DEV)
    m0, v0 = (torch.randn(n, generator=gen) * 0.1).to(DEV), (torch.rand(n, generator=gen) * 0.01).to(DEV)
    lr, b1, b2, eps, scale = 1e-3, 0.9, 0.999, 1e-4, 65536.0
    lib = L.load()
    gscale = torch.zeros(1, device=DEV)
    equal_ts = []
    for world in (1, 2):
        for t in (1, 2, 3, 10, 100, 1000, 12000):
            state = _state(scale=scale, lr=lr, t=t - 1, growth_tracker=6, shard_weight=0.75)
            ops.loss_scale_begin(state, gscale, world=world, beta1=b1, beta2=b2)
            h = _read(state)
            assert gscale.item() == 0.75 * scale
            ad = L.OptimArgs()
            ad.kind, ad.weight_decay = L.OPT_ADAMW, 0.0
            ad.lr, ad.beta1, ad.beta2, ad.eps, ad.grad_scale, ad.step = lr, b1, b2, eps, (1.0 / world) / scale, t
            want = (C.c_float * 4)()
            assert lib.mtbc_optim_dynamic(C.byref(ad), C.byref(want)) == 0
            assert h.adam[0] == want[0], (t, world)
            d = [_ulps(h.adam[i], want[i]) for i in (1, 2)]
            if any(d):
                print(f"t = {t}: device bias corrections differ from the host's by {d} ulp")
            assert max(d) <= 1 and (t > 3 or max(d) == 0), (t, d, list(h.adam), list(want))
            if max(d) == 0 and world == 1:
                equal_ts.append(t)
    assert equal_ts[:3] == [1, 2, 3]
    for t in equal_ts:
        for world in (1, 2):
            state = _state(scale=scale, lr=lr, t=t - 1, growth_tracker=6)
            p, g, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
            ops.loss_scale_begin(state, gscale, world=world, beta1=b1, beta2=b2)
            ops.loss_scale_check(state, g)
            ops.loss_scale_adam(state, p, g, m, v, beta1=b1, beta2=b2, eps=eps, growth_interval=7)
            pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
            ops.adam_step(pr, g0, mr, vr, lr, t, beta1=b1, beta2=b2, eps=eps, grad_scale=(1.0 / world) / scale)
            assert torch.equal(p, pr) and torch.equal(m, mr) and torch.equal(v, vr), (t, world)
            assert torch.equal(g, g0)
            h = _read(state)
            assert (h.scale, h.growth_tracker, h.found_inf, h.t, h.skipped) == (2 * scale, 0, 0, t, 0)     # 6 + 1 = growth_interval: doubled
    # found-inf: parameters and moments bit-unchanged, t stays, the scale halves
    for val in (float("inf"), float("nan")):
        for zero_grad in (False, True):
            state = _state(scale=scale, lr=lr, t=4, growth_tracker=6, skipped=2)
            p, g, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
            g[n - 1] = val
            ops.loss_scale_begin(state, gscale, beta1=b1, beta2=b2)
            ops.loss_scale_check(state, g)
            ops.loss_scale_adam(state, p, g, m, v, beta1=b1, beta2=b2, eps=eps, zero_grad=zero_grad, growth_interval=7)
            assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
            assert bool((g == 0).all()) == zero_grad              # zero_grad behaves as in an applied step
            h = _read(state)
            assert (h.scale, h.growth_tracker, h.found_inf, h.t, h.skipped) == (scale / 2, 0, 0, 4, 3)


# ------------------------------------------------------------------------------------------------ whole steps
def _train(dtype, size, steps, loss_scale, graph=False, static_scale=None, lr_change_at=None, seed0=20, same_batch=False, n=2, snapshots=False):
    m = _net(dtype)
    if static_scale is not None:
        m.loss_scale = float(static_scale)
    opt = FusedAdam(m, lr=1e-3, eps=1e-4)
    step = FusedTrainStep(m, opt, alpha=0.35, graph=graph, loss_scale=loss_scale)
    losses, trace = [], []
    for s in range(steps):
        if lr_change_at is not None and s == lr_change_at:
            opt.param_groups[0]["lr"] = 2.5e-4                    # what a scheduler does between steps
        losses.append(step(*_batch(n, size, seed0 if same_batch else seed0 + s)).clone())
        if snapshots:
            trace.append((step.scaler.stats(), m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
    torch.cuda.synchronize()
    step.check_nan()
    if graph:
        assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
    return {"p": m.flat_p.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "losses": torch.stack(losses),
            "stats": step.scaler.stats() if step.scaler is not None else None, "trace": trace, "step": step, "opt": opt, "model": m}


def _same(a, b, what):
    for k in ("losses", "p", "m", "v"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differ, max |diff| {(a[k] - b[k]).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype,size,init,how", [("f16", 64, 65536.0, "object"), ("f16", 256, 65536.0, "object"), ("bf16", 64, 1.0, "object"),
                                                 ("f16", 64, 65536.0, "switch")])
def test_dynamic_steps_without_overflow_are_the_static_steps(dtype, size, init, how, monkeypatch):
    """Five steps under DynamicLossScale(init_scale = the static scale) against five steps of the static path: multiplying by a power of two is exact, so
    losses, parameters and both moments are bit-equal; nothing was skipped.  `switch`: the MTBC_DYN_SCALE arm (loss_scale=None, DynamicLossScale())."""
    static = _train(dtype, size, 5, None, lr_change_at=3)
    assert static["step"].scaler is None
    if how == "switch":
        monkeypatch.setenv("MTBC_DYN_SCALE", "1")
        dyn = _train(dtype, size, 5, None, lr_change_at=3)
        assert isinstance(dyn["step"].scaler, DynamicLossScale)
    else:
        dyn = _train(dtype, size, 5, DynamicLossScale(init_scale=init, growth_interval=10 ** 6), lr_change_at=3)
    _same(static, dyn, "dynamic against static")
    assert dyn["stats"] == {"scale": init, "growth_tracker": 5, "skipped": 0, "t": 5}
    assert dyn["opt"].applied_steps() == 5 == static["opt"].step_count
    assert float(dyn["opt"].state_dict()["state"][0]["step"]) == 5.0


@pytest.mark.parametrize("dtype,size,init", [("f16", 64, 65536.0), ("bf16", 64, 1.0)])
def test_graph_replayed_dynamic_steps_are_the_eager_dynamic_steps(dtype, size, init):
    """Eight steps (replay is reached at the third), the learning rate changed in between: begin, check, Adam and the state update are part of the captured
    graph, the learning rate reaches them through the scaler's device state."""
    runs = [_train(dtype, size, 8, DynamicLossScale(init_scale=init, growth_interval=3), graph=graph, lr_change_at=5) for graph in (False, True)]
    _same(runs[0], runs[1], "graph replay against eager")
    assert runs[0]["stats"] == runs[1]["stats"]
    st = runs[0]["stats"]
    assert st["t"] + st["skipped"] == 8
    if dtype == "bf16":
        assert st == {"scale": init * 4, "growth_tracker": 2, "skipped": 0, "t": 8}                     # grown twice


def test_overflowing_steps_are_skipped_and_the_first_applied_update_is_the_static_one():
    """fp16 under a loss scale of 2^40: the backward overflows, the step is skipped and the scale halves until the gradients are finite.  While skipping,
    parameters and moments do not move and t stays 0; the first update that IS applied equals the first update of a fresh static run at the settled scale."""
    sc = DynamicLossScale(init_scale=BIG, growth_interval=10 ** 6)
    m = _net("f16")
    opt = FusedAdam(m, lr=1e-3, eps=1e-4)
    step = FusedTrainStep(m, opt, alpha=0.35, loss_scale=sc)
    batch = _batch(2, 64, 31)
    step.load_batch(*batch)
    opt._ensure_state()
    first = settled = None
    prev, clean = sc.stats(), 0
    for s in range(64):
        before = (m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
        step(*batch)
        step.check_nan()                                          # the forward losses stay finite: an overflowing backward is not fatal any more
        st = sc.stats()
        if st["skipped"] > prev["skipped"]:                       # skipped: nothing but the scale state moved
            clean = 0
            assert st["skipped"] == prev["skipped"] + 1 and st["t"] == prev["t"] and st["scale"] == prev["scale"] / 2 and st["growth_tracker"] == 0
            assert torch.equal(m.flat_p, before[0]) and torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2])
            if first is None:
                assert st["t"] == 0 and not opt.exp_avg.any() and not opt.exp_avg_sq.any()
        else:
            clean += 1
            assert st["t"] == prev["t"] + 1 and st["scale"] == prev["scale"]
            if first is None:
                first, settled = (m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()), st["scale"]
        prev = st
        if clean == 4:                                            # skipped has stopped growing, plus three steps
            break
    print("after", s + 1, "steps:", prev, "scale of the first applied update:", settled)
    assert prev["skipped"] >= 1, "2^40 did not overflow: the test would show nothing"
    assert clean == 4 and prev["skipped"] + prev["t"] == s + 1
    for v in (settled, prev["scale"]):
        assert v <= BIG and v == 2.0 ** round(torch.log2(torch.tensor(v, dtype=torch.float64)).item())
    assert bool(torch.isfinite(m.flat_p).all()) and bool(torch.isfinite(opt.exp_avg).all()) and bool(torch.isfinite(opt.exp_avg_sq).all())
    assert float(opt.state_dict()["state"][0]["step"]) == float(prev["t"])     # the device's t, not the number of calls
    ref = _train("f16", 64, 1, None, static_scale=settled, seed0=31, same_batch=True)
    for a, b, what in zip(first, (ref["p"], ref["m"], ref["v"]), ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), f"first applied update against the static run at {settled}: {what} differ"


def test_scale_grows_back_and_graph_replay_keeps_the_same_state():
    """growth_interval = 4 from 2^40: skips down to a scale that works, doubles after four clean steps (and backs off again when that was too much).
    Eager and hipGraph replay go through the same states, step by step."""
    runs = [_train("f16", 64, 48, DynamicLossScale(init_scale=BIG, growth_interval=4), graph=graph, same_batch=True, seed0=31, snapshots=True)
            for graph in (False, True)]
    trace = [t[0] for t in runs[0]["trace"]]
    assert trace[-1]["skipped"] >= 1 and trace[-1]["t"] >= 4
    doubled = 0
    for i in range(1, len(trace)):
        if trace[i]["skipped"] == trace[i - 1]["skipped"] and trace[i - 1]["growth_tracker"] == 3:      # the fourth clean step in a row
            assert trace[i]["scale"] == 2 * trace[i - 1]["scale"] and trace[i]["growth_tracker"] == 0
            doubled += 1
    assert doubled >= 1
    for i, (a, b) in enumerate(zip(runs[0]["trace"], runs[1]["trace"])):
        assert a[0] == b[0], (i, a[0], b[0])
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), i
    _same(runs[0], runs[1], "graph replay against eager, with skips")
    assert bool(torch.isfinite(runs[0]["p"]).all())


# ------------------------------------------------------------------------------------------------ data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_distributed_overflowing_steps_and_run_empty_single_rank_rccl():
    """The data-parallel path at world 1 (real RCCL launches) from an overflowing scale, 1 / 4 / 8 buckets: the same skips as the local run, and
    run_empty() goes through the same begin / check / update path."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        batches = [_batch(2, 64, 70 + s) for s in range(3)]

        def run(distributed, n_buckets, init):
            m = _net("f16")
            sc = DynamicLossScale(init_scale=init, growth_interval=2)
            opt = FusedAdam(m, lr=1e-4, eps=1e-4)
            step = FusedTrainStep(m, opt, alpha=0.5, distributed=distributed, n_buckets=n_buckets, loss_scale=sc)
            for b in batches:
                l = step(*b)
            if distributed:
                step.run_empty()                                  # a zero gradient through the same begin / check / update path
            torch.cuda.synchronize()
            step.check_nan()
            assert m.coop_error_word() is None or int(m.coop_error_word().item()) == 0
            if distributed:
                assert len(step._st.buckets) == n_buckets
            return m.flat_p.clone(), opt.exp_avg.clone(), l.clone(), sc.stats()

        p0, m0, l0, s0 = run(False, 4, BIG)
        # three halvings leave 2^37: any |dz| above 2^-21 still overflows fp16's 65504 there, so all three steps are skipped
        assert s0 == {"scale": BIG / 8, "growth_tracker": 0, "skipped": 3, "t": 0}
        for nb in (1, 4, 8):
            p1, m1, l1, s1 = run(True, nb, BIG)
            # run_empty's zero gradient is finite: that update IS applied (and, with zero moments, moves nothing)
            assert s1 == {"scale": BIG / 8, "growth_tracker": 1, "skipped": 3, "t": 1}, (nb, s1)
            assert torch.equal(l0, l1) and torch.equal(p0, p1) and not m1.any(), nb
    finally:
        dist.destroy_process_group()


def test_distributed_dynamic_step_single_rank_rccl_equals_local_dynamic_step():
    """The data-parallel path (bucketed RCCL all-reduce on the side stream, check and Adam after the streams join) at world 1, for 1 / 4 / 8 buckets:
    bit-equal to the local dynamic step; the cooperative kernels' error word stays 0."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        batches = [_batch(2, 64, 70 + s) for s in range(3)]

        def run(distributed, n_buckets):
            m = _net("f16")
            sc = DynamicLossScale(init_scale=65536.0, growth_interval=2)
            opt = FusedAdam(m, lr=1e-4, eps=1e-4)
            step = FusedTrainStep(m, opt, alpha=0.5, distributed=distributed, n_buckets=n_buckets, loss_scale=sc)
            for b in batches:
                l = step(*b)
            torch.cuda.synchronize()
            step.check_nan()
            assert m.coop_error_word() is None or int(m.coop_error_word().item()) == 0
            return m.flat_p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), l.clone(), sc.stats()

        ref = run(False, 4)
        assert ref[4] == {"scale": 131072.0, "growth_tracker": 1, "skipped": 0, "t": 3}
        for nb in (1, 4, 8):
            got = run(True, nb)
            assert got[4] == ref[4], nb
            for a, b in zip(ref[:4], got[:4]):
                assert torch.equal(a, b), nb
    finally:
        dist.destroy_process_group()


def _worker(rank, world, port, q, steps):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _net("f16")
        sc = DynamicLossScale(init_scale=BIG, growth_interval=3)
        step = FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5, distributed=True, n_buckets=4, loss_scale=sc)
        G = 4
        per = G // world
        for s in range(steps):
            img, mask, label = O.synthetic_batch(G, 64, 64, seed=7 + (s % 2))          # the GLOBAL batch; each rank takes its shard
            sl = slice(rank * per, (rank + 1) * per)
            step(img[sl].to(DEV), mask[sl].to(DEV), label[sl].to(DEV))
        torch.cuda.synchronize()
        step.check_nan()
        st = sc.stats()
        q.put((rank, st, m.flat_p.cpu().numpy()))                 # numpy arrays travel by value
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_on_skips_scale_and_parameters():
    """Two ranks (both on the one visible GPU, gloo as transport) from an overflowing scale: the found-inf pass runs on the all-reduced gradients, so both ranks
    skip the same steps, end at the same scale and hold the same parameters without any collective of its own."""
    import queue as _queue
    import torch.multiprocessing as mp
    world, steps = 2, 40
    ctx = mp.get_context("spawn")
    got = []
    for attempt in range(2):          # a 2-process gloo rendezvous on one box has been seen to stall once
        q, port = ctx.Queue(), _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q, steps)) for r in range(world)]
        for p in procs:
            p.start()
        got = []
        try:
            for _ in range(world):
                got.append(q.get(timeout=240))
        except _queue.Empty:
            got = []
        for p in procs:
            p.join(60 if got else 1)
            if p.is_alive():
                p.kill()              # exactly the processes this test started
                p.join(10)
        if got:
            assert all(p.exitcode == 0 for p in procs)
            break
    assert len(got) == world, "the two-rank run produced no result in two attempts"
    got.sort(key=lambda r: r[0])
    (_, s0, p0), (_, s1, p1) = got
    print("two ranks:", s0, s1)
    assert s0 == s1
    assert s0["skipped"] >= 1 and s0["t"] >= 1 and s0["skipped"] + s0["t"] == steps
    assert (p0 == p1).all()
    assert torch.isfinite(torch.from_numpy(p0)).all()


# ------------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_round_trip_with_the_scaler(tmp_path):
    from multi_task_breast_cancer_amd.checkpoint import load_pretrained_model, save_checkpoint
    a = _train("f16", 64, 3, DynamicLossScale(init_scale=65536.0, growth_interval=2))
    assert a["stats"] == {"scale": 131072.0, "growth_tracker": 1, "skipped": 0, "t": 3}
    new, old = str(tmp_path / "new.pth"), str(tmp_path / "old.pth")
    save_checkpoint(new, 1, a["model"], a["opt"], 0.25, scaler=a["step"].scaler)
    save_checkpoint(old, 1, a["model"], a["opt"], 0.25)
    ck = torch.load(new, weights_only=False)
    assert float(ck["optimizer_state_dict"]["state"][0]["step"]) == 3.0
    assert ck["loss_scaler_state_dict"] == {"scale": 131072.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2, "_growth_tracker": 1}
    assert "loss_scaler_state_dict" not in torch.load(old, weights_only=False)

    def resume(path, scaler):
        m = _net("f16")
        opt = FusedAdam(m, lr=1e-3, eps=1e-4)
        step = FusedTrainStep(m, opt, alpha=0.35, loss_scale=scaler)
        load_pretrained_model(m, path, optimizer=opt, scaler=scaler)
        return m, opt, step

    m, opt, step = resume(new, DynamicLossScale())
    assert step.scaler.stats() == {"scale": 131072.0, "growth_tracker": 1, "skipped": 0, "t": 3}
    assert torch.equal(m.flat_p, a["p"]) and torch.equal(opt.exp_avg, a["m"])
    batch = _batch(2, 64, 99)
    l0, l1 = a["step"](*batch).clone(), step(*batch).clone()
    assert torch.equal(l0, l1) and torch.equal(m.flat_p, a["model"].flat_p) and torch.equal(opt.exp_avg_sq, a["opt"].exp_avg_sq)
    assert step.scaler.stats() == a["step"].scaler.stats() == {"scale": 262144.0, "growth_tracker": 0, "skipped": 0, "t": 4}
    # a file written without a scaler: model and optimizer load as before, the scaler keeps its own scale and takes the optimizer's step count
    m, opt, step = resume(old, DynamicLossScale(init_scale=1024.0))
    assert step.scaler.stats() == {"scale": 1024.0, "growth_tracker": 0, "skipped": 0, "t": 3}
    assert torch.equal(m.flat_p, a["p"])
