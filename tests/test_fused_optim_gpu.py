"""Fused Adam / SGD (Nesterov) / AdamW on the GPU: the kernel against the host function that runs the same element function, bit for bit; Adam
against the words its own kernel wrote before it moved onto the shared launch (tests/golden/adam_steps.npz); whole training
steps under FusedTrainStep against the oracle with torch.optim.SGD / torch.optim.AdamW (experiment_init.py:188-191); hipGraph replay, the dynamic
loss scale, data parallel at world 1 with real RCCL launches, and checkpoint interchange with torch's optimizers in both directions."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd import checkpoint as CK
from multi_task_breast_cancer_amd import ops
from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.nets import MTnnUNet
from multi_task_breast_cancer_amd.optim import FusedAdamW, FusedSGD
from multi_task_breast_cancer_amd.trainer import FusedTrainStep
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = {"SGD": L.OPT_SGD, "AdamW": L.OPT_ADAMW}
# the op-level rules by name -> (kind, the hyper-parameters that tell them apart): Adam is the AdamW rule without decay at the reference's eps
RULES = {"SGD": (L.OPT_SGD, dict(weight_decay=1e-2, eps=1e-8)), "AdamW": (L.OPT_ADAMW, dict(weight_decay=1e-2, eps=1e-8)),
         "Adam": (L.OPT_ADAMW, dict(weight_decay=0.0, eps=1e-4))}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_steps.npz")
BIG = 2.0 ** 40           # a loss scale under which the first fp16 backward overflows (asserted below, not assumed)


def _make(name, model, lr=1e-3):
    return FusedSGD(model, lr=lr, momentum=0.9, nesterov=True) if name == "SGD" else FusedAdamW(model, lr=lr)


def _torch_opt(name, params, lr=1e-3):
    return torch.optim.SGD(params, lr=lr, momentum=0.9, nesterov=True) if name == "SGD" else torch.optim.AdamW(params, lr=lr)


def _state_of(opt):
    return [b.clone() for b in opt._buffers()]


def _batch(n, size, seed):
    return tuple(t.to(DEV) for t in O.synthetic_batch(n, size, size, seed=seed))


# ------------------------------------------------------------------------------------------------ 6. the kernel against the host function
def _host(lib, kind, arrs, dyn=None, skip=None, **hyper):
    p, g, m, v = arrs
    ptr = lambda x: x.ctypes.data if x is not None else None
    a = ops.optim_args(kind, p.size, ptr(p), ptr(g), ptr(m), ptr(v) if kind == L.OPT_ADAMW else None, dynamic=ptr(dyn), skip=ptr(skip), **hyper)
    assert lib.mtbc_optim_step_host(C.byref(a)) == 0


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2_098_179])          # the last: 2048 blocks x 256 threads x 4 + 1027 -- the grid-stride loop and the tail
@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_kernel_is_the_host_function_bit_for_bit(name, n):
    """Four steps with the scalars in the launch arguments and four with `dynamic` set; then a step under a set skip word (nothing but g moves) and one
    under a clear word.  Every buffer is compared as bits after every launch."""
    lib = L.load()
    kind, rule = RULES[name]
    adamw = kind == L.OPT_ADAMW
    gen = torch.Generator().manual_seed(n)
    host = [torch.randn(n, generator=gen), None, torch.zeros(n), torch.zeros(n)]
    grads = [torch.randn(n, generator=gen) * 10 ** float(e) for e in (-6, -3, 0, -2)]
    dev = [host[0].to(DEV), None, host[2].to(DEV), host[3].to(DEV)]
    arrs = [host[0].numpy(), None, host[2].numpy(), host[3].numpy()]      # torch CPU allocations are 64-byte aligned
    dyn_dev = torch.zeros(4, device=DEV)

    def compare(what):
        for k, (d, h) in enumerate(zip(dev, host)):
            assert torch.equal(d.cpu().view(torch.int32), h.view(torch.int32)), (what, "pgmv"[k])

    t = 0
    for use_dyn in (False, True):
        for gr in grads:
            t += 1
            hyper = dict(lr=1e-3 / t, step=t, grad_scale=0.5, zero_grad=(t % 2 == 0), **rule)
            host[1] = gr.clone()
            arrs[1] = host[1].numpy()
            dev[1] = gr.to(DEV)
            if use_dyn:
                out = (C.c_float * 4)()
                assert lib.mtbc_optim_dynamic(C.byref(ops.optim_args(kind, 0, None, None, None, **hyper)), C.byref(out)) == 0
                dyn_host = np.array(list(out), dtype=np.float32)
                dyn_dev.copy_(torch.from_numpy(dyn_host))
                wrong = dict(hyper, lr=1.0, step=1, grad_scale=3.0)          # not read when `dynamic` is set
                _host(lib, kind, arrs, dyn=dyn_host, **wrong)
                ops.optim_step(kind, dev[0], dev[1], dev[2], dev[3] if adamw else None, dynamic=dyn_dev, **wrong)
            else:
                _host(lib, kind, arrs, **hyper)
                ops.optim_step(kind, dev[0], dev[1], dev[2], dev[3] if adamw else None, **hyper)
            compare(f"step {t} dynamic {use_dyn}")
    assert bool(dev[2].any()) and (not adamw or bool(dev[3].any()))
    before = [x.clone() for x in dev]
    for word, zero in ((1, True), (1, False), (0, True)):
        hyper = dict(lr=1e-3, step=9, zero_grad=zero, **rule)
        host[1] = grads[2].clone()
        arrs[1] = host[1].numpy()
        dev[1] = grads[2].to(DEV)
        skip_dev = torch.tensor([word], dtype=torch.int32, device=DEV)
        _host(lib, kind, arrs, skip=np.array([word], dtype=np.uint32), **hyper)
        ops.optim_step(kind, dev[0], dev[1], dev[2], dev[3] if adamw else None, skip=skip_dev, **hyper)
        compare(f"skip word {word} zero_grad {zero}")
        if word:
            assert torch.equal(dev[0], before[0]) and torch.equal(dev[2], before[2]) and torch.equal(dev[3], before[3])
            assert bool((dev[1] == 0).all()) == zero
        else:
            assert not torch.equal(dev[0], before[0]) and not bool(dev[1].any())


def test_misaligned_pointers_are_refused():
    lib = L.load()
    bufs = [torch.zeros(9, device=DEV) for _ in range(4)]
    for kind in KINDS.values():
        for bad in range(4 if kind == L.OPT_ADAMW else 3):
            ptrs = [(b[1:] if i == bad else b[:8]).data_ptr() for i, b in enumerate(bufs)]
            a = ops.optim_args(kind, 8, *ptrs)
            assert lib.mtbc_optim_step(C.byref(a), None) == -5, (kind, bad)          # MTBC_E_UNSUPPORTED, before any launch
    torch.cuda.synchronize()
    assert all(not b.any() for b in bufs)


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2_098_179])
def test_adamw_without_decay_is_fused_adam(n):
    """ops.adam_step against an explicit AdamW launch (weight_decay 0, eps 1e-4) over four steps: torch.equal on every element.  Both are the shared
    kernel today, so this holds the wrapper's arguments to the explicit call's, the grid-stride size included; that the words are the ones Adam's own
    kernel wrote is the next test's statement."""
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10 ** float(e) for e in (-6, -3, 0, -2)]
    pa, ma, va = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pw, mw, vw = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t, gr in enumerate(grads, start=1):
        g = gr.to(DEV)
        ops.adam_step(pa, g, ma, va, lr=1e-4, step=t, eps=1e-4, grad_scale=0.25)
        ops.optim_step(L.OPT_ADAMW, pw, g, mw, vw, lr=1e-4, step=t, eps=1e-4, weight_decay=0.0, grad_scale=0.25)
        for a, w, what in ((pa, pw, "p"), (ma, mw, "exp_avg"), (va, vw, "exp_avg_sq")):
            assert torch.equal(a, w), (t, what)


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_adam_step_reproduces_the_words_recorded_from_adams_own_kernel(n):
    """ops.adam_step -- the shared kernel as AdamW with weight_decay 0 -- against tests/golden/adam_steps.npz (tools/make_adam_fixture.py): p, exp_avg,
    exp_avg_sq and g after each of five launches, recorded at the last commit at which Adam had its own kernel.  Every word is equal: v fused in the
    float4 body, two products and an add on the tail (n = 1 and 3 are all tail); the fifth step clears g.  The grid-stride size is
    test_kernel_is_the_host_function_bit_for_bit[Adam-2098179]'s."""
    z = np.load(GOLDEN)
    dev = lambda words: torch.from_numpy(np.ascontiguousarray(words).view(np.float32).copy()).to(DEV)
    p, m, v = dev(z[f"n{n}_p0"]), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t in range(1, 6):
        g = dev(z[f"n{n}_grads"][t - 1])
        ops.adam_step(p, g, m, v, lr=1e-4, step=t, eps=1e-4, grad_scale=0.25, zero_grad=(t == 5))
        for key, mine in (("p", p), ("m", m), ("v", v), ("g", g)):
            assert np.array_equal(mine.cpu().view(torch.int32).numpy(), z[f"n{n}_{key}"][t - 1]), (n, t, key)
    assert not bool(g.any()) and bool(v.any())


# ------------------------------------------------------------------------------------------------ 7. the whole step against the oracle
@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_fused_step_matches_the_oracle_with_torchs_optimizer(name):
    """MTnnUNet, fp32, one FusedTrainStep with the fused optimizer against O.train_step with torch's over the oracle model, lr 1e-3; the bounds are
    the ones one drop-in step of these optimizers is held to (test_factory_torch_optimizers_step_the_flat_parameters)."""
    seed_everything(4)
    prod = MTnnUNet(1, 1, 3)
    ref = O.build_oracle_model("MTnnUNet", 1, 1, 3, True)
    ref.load_state_dict(prod.state_dict())
    prod = prod.to(DEV)
    opt = _make(name, prod)
    step = FusedTrainStep(prod, opt, alpha=0.5)
    img, mask, label = O.synthetic_batch(2, 64, 64, seed=2)
    losses = step(img.to(DEV), mask.to(DEV), label.to(DEV)).cpu()
    step.check_nan()
    ropt = _torch_opt(name, ref.parameters())
    total = O.train_step(ref, ropt, img, mask, label, 0.5, True, 3)[0]
    assert abs(losses[0].item() - float(total)) < 1e-4
    assert opt.applied_steps() == 1
    for (k, a), (_, b) in zip(prod.state_dict().items(), ref.state_dict().items()):
        d = (a.cpu() - b).abs()
        if name == "SGD":                       # update = lr * (1.9 g): as exact as the gradient
            assert d.max().item() < 5e-5, (name, k, d.max().item())
        else:                                   # AdamW, eps 1e-8, step 1: update = lr * sign(g) -- an element whose gradient is
            assert d.max().item() <= 2.1e-3     # rounding noise may go the other way (2 lr), few do
            assert (d > 1e-4).float().mean().item() < 0.02, (name, k)


def test_torch_optimizers_are_refused_by_name():
    prod = MTnnUNet(1, 1, 3).to(DEV)
    for make in (lambda: torch.optim.SGD(prod.parameters(), lr=1e-3, momentum=0.9, nesterov=True), lambda: torch.optim.AdamW(prod.parameters(), lr=1e-3)):
        with pytest.raises(TypeError, match="FusedSGD"):
            FusedTrainStep(prod, make(), alpha=0.5)


# ------------------------------------------------------------------------------------------------ 8. / 9. graph replay, dynamic loss scale
def _net(dtype):
    seed_everything(1993)
    m = MTnnUNet(1, 1, 3).to(DEV)
    m.set_compute(dtype)
    return m


def _train(name, dtype, size, steps, loss_scale, graph=False, static_scale=None, lr_change_at=None, seed0=20, same_batch=False, n=2):
    m = _net(dtype)
    if static_scale is not None:
        m.loss_scale = float(static_scale)
    opt = _make(name, m)
    step = FusedTrainStep(m, opt, alpha=0.35, graph=graph, loss_scale=loss_scale)
    losses = []
    for s in range(steps):
        if lr_change_at is not None and s == lr_change_at:
            opt.param_groups[0]["lr"] = 2.5e-4                    # what a scheduler does between steps
        losses.append(step(*_batch(n, size, seed0 if same_batch else seed0 + s)).clone())
    torch.cuda.synchronize()
    step.check_nan()
    if graph:
        assert any(e[2] is not None for e in step._graphs.values()), "no step was captured"
    return {"p": m.flat_p.clone(), "state": _state_of(opt), "losses": torch.stack(losses),
            "stats": step.scaler.stats() if step.scaler is not None else None, "step": step, "opt": opt, "model": m}


def _same(a, b, what):
    for k in ("losses", "p"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differ, max |diff| {(a[k] - b[k]).abs().max().item():.3e}"
    assert len(a["state"]) == len(b["state"])
    for i, (x, y) in enumerate(zip(a["state"], b["state"])):
        assert torch.equal(x, y), f"{what}: state buffer {i} differs, max |diff| {(x - y).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_graph_replayed_steps_are_the_eager_steps(name, dtype):
    """Six steps (replay is reached at the third), the learning rate changed at step 4: it reaches the captured launch through the 16 bytes of scalars."""
    runs = [_train(name, dtype, 64, 6, None, graph=graph, lr_change_at=4) for graph in (False, True)]
    _same(runs[0], runs[1], "graph replay against eager")
    assert runs[0]["opt"].applied_steps() == runs[1]["opt"].applied_steps() == 6
    still = _train(name, dtype, 64, 6, None)                      # the change of the learning rate is not a no-op
    assert not torch.equal(still["p"], runs[0]["p"])


@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_dynamic_steps_without_overflow_are_the_static_steps(name):
    """fp16, five steps under DynamicLossScale(init_scale = the static 65536) against the static path: multiplying by a power of two is exact, so losses,
    parameters and the optimizer's state are bit-equal; nothing was skipped.  The learning rate changes on the way (through the scaler's state)."""
    static = _train(name, "f16", 64, 5, None, lr_change_at=3)
    assert static["step"].scaler is None and static["model"].loss_scale == 65536.0
    dyn = _train(name, "f16", 64, 5, DynamicLossScale(init_scale=65536.0, growth_interval=10 ** 6), lr_change_at=3)
    _same(static, dyn, "dynamic against static")
    assert dyn["stats"] == {"scale": 65536.0, "growth_tracker": 5, "skipped": 0, "t": 5}
    assert dyn["opt"].applied_steps() == 5 == static["opt"].step_count


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_overflowing_steps_are_skipped_and_the_first_applied_update_is_the_static_one(name, graph):
    """fp16 under a loss scale of 2^40: the backward overflows (an fp16 value, not a fault), the step is skipped and the scale halves until the gradients
    are finite.  While skipping, parameters and the momentum buffer / the moments do not move and t stays 0; the first update that IS applied equals the
    first update of a fresh static run at the settled scale."""
    sc = DynamicLossScale(init_scale=BIG, growth_interval=10 ** 6)
    m = _net("f16")
    opt = _make(name, m)
    step = FusedTrainStep(m, opt, alpha=0.35, loss_scale=sc, graph=graph)
    batch = _batch(2, 64, 31)
    step.load_batch(*batch)
    opt._ensure_state()
    first = settled = None
    prev, clean = sc.stats(), 0
    for s in range(64):
        before = (m.flat_p.clone(), *_state_of(opt))
        step(*batch)
        step.check_nan()                                          # the forward losses stay finite
        st = sc.stats()
        if st["skipped"] > prev["skipped"]:                       # skipped: nothing but the scale state moved
            clean = 0
            assert st["skipped"] == prev["skipped"] + 1 and st["t"] == prev["t"] and st["scale"] == prev["scale"] / 2 and st["growth_tracker"] == 0
            for a, b in zip((m.flat_p, *opt._buffers()), before):
                assert torch.equal(a, b)
            if first is None:
                assert st["t"] == 0 and not any(bool(b.any()) for b in opt._buffers())
        else:
            clean += 1
            assert st["t"] == prev["t"] + 1 and st["scale"] == prev["scale"]
            if first is None:
                first, settled = (m.flat_p.clone(), *_state_of(opt)), st["scale"]
        prev = st
        if clean == 2:
            break
    print("after", s + 1, "steps:", prev, "scale of the first applied update:", settled)
    assert prev["skipped"] >= 1, "2^40 did not overflow: the test would show nothing"
    assert clean == 2 and prev["skipped"] + prev["t"] == s + 1
    assert opt.applied_steps() == prev["t"]                       # the device's t, not the number of calls
    assert all(bool(torch.isfinite(b).all()) for b in (m.flat_p, *opt._buffers()))
    ref = _train(name, "f16", 64, 1, None, static_scale=settled, seed0=31, same_batch=True)
    for a, b in zip(first, (ref["p"], *ref["state"])):
        assert torch.equal(a, b), f"first applied update against the static run at {settled}"


# ------------------------------------------------------------------------------------------------ 10. data parallel at world 1, real RCCL launches
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_data_parallel_step_with_rccl_collectives_is_the_local_step():
    """World 1 with the nccl backend (the collectives still launch, on the communication stream): distributed=True with 1 / 4 / 8 buckets reproduces
    the local step bit for bit, for both optimizers, two steps in a row.  run_empty() after that applies a zero-gradient update: SGD's buffer is
    multiplied by its momentum and the parameters move along it; AdamW still decays the parameters and its moments."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        batches = [O.synthetic_batch(2, 64, 64, seed=60 + s) for s in range(2)]

        def run(name, distributed, n_buckets):
            seed_everything(1993)
            m = MTnnUNet(1, 1, 3).to(DEV)
            opt = _make(name, m)
            step = FusedTrainStep(m, opt, alpha=0.5, distributed=distributed, n_buckets=n_buckets)
            for img, mask, label in batches:
                l = step(img.to(DEV), mask.to(DEV), label.to(DEV))
            torch.cuda.synchronize()
            step.check_nan()
            return m, opt, l.clone(), step

        for name in ("SGD", "AdamW"):
            m0, opt0, l0, _ = run(name, False, 4)
            for nb in (1, 4, 8):
                m1, opt1, l1, step = run(name, True, nb)
                assert opt1.grad_scale == 1.0 and len(step._st.buckets) == nb
                assert torch.equal(l0, l1) and torch.equal(m0.flat_g, m1.flat_g) and torch.equal(m0.flat_p, m1.flat_p), (name, nb)
                for a, b in zip(opt0._buffers(), opt1._buffers()):
                    assert torch.equal(a, b), (name, nb)
            # the empty shard of a short last batch: the same collectives on a zero gradient, then the same update
            p, state = m1.flat_p.clone(), _state_of(opt1)
            step.run_empty()
            torch.cuda.synchronize()
            assert not bool(m1.flat_g.any())
            if name == "SGD":
                buf = state[0] * 0.9                              # fma(0.9, buf, 0): one rounding, as the product
                assert torch.equal(opt1.momentum_buffer, buf)
                want = p.double() - 1e-3 * 0.9 * buf.double()       # d = momentum buf (g' = 0), p -= lr d
                assert (m1.flat_p.double() - want).abs().max().item() <= 2.0 ** -23 * p.abs().max().item()
                assert not torch.equal(m1.flat_p, p)
            else:
                assert torch.allclose(opt1.exp_avg, state[0] * 0.9, rtol=1e-6, atol=1e-30) and torch.allclose(opt1.exp_avg_sq, state[1] * 0.999, rtol=1e-6, atol=1e-30)
                # p (1 - lr wd) - step * m / denom: the decay alone (1e-5 of p, 80 ulp) moves a parameter unless the other term happens to cancel it
                assert (m1.flat_p != p).float().mean().item() > 0.99
                assert opt1.applied_steps() == 3
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ 11. checkpoint interchange
@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_checkpoint_interchanges_with_torchs_optimizer(name, tmp_path):
    """A checkpoint written here resumes under torch's optimizer on the oracle model and the other way round: the optimizer state is in torch's
    layout (SGD: momentum_buffer; AdamW: step, exp_avg, exp_avg_sq); the next step then agrees within test_checkpoint_interchanges_with_torch_adam's
    bound."""
    lr = 1e-4 if name == "AdamW" else 1e-3
    seed_everything(5)
    prod = MTnnUNet(1, 1, 3).to(DEV)
    opt = _make(name, prod, lr)
    step = FusedTrainStep(prod, opt, alpha=0.5)
    img, mask, label = O.synthetic_batch(2, 64, 64, seed=1)
    step(img.to(DEV), mask.to(DEV), label.to(DEV))
    path = str(tmp_path / "model_fold_0")
    CK.save_checkpoint(path, 3, prod, opt, 0.123)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler", "val_loss"}
    keys = {"momentum_buffer"} if name == "SGD" else {"step", "exp_avg", "exp_avg_sq"}
    assert all(set(s) == keys for s in ck["optimizer_state_dict"]["state"].values())
    # -> into the CPU oracle + torch's optimizer
    ref = O.build_oracle_model("MTnnUNet", 1, 1, 3, True)
    ref.load_state_dict(ck["model_state_dict"])
    ropt = _torch_opt(name, ref.parameters(), lr)
    ropt.load_state_dict(ck["optimizer_state_dict"])
    img2, mask2, label2 = O.synthetic_batch(2, 64, 64, seed=2)
    O.train_step(ref, ropt, img2, mask2, label2, 0.5, True, 3)
    step(img2.to(DEV), mask2.to(DEV), label2.to(DEV))
    worst = max((a.cpu() - b).abs().max().item() for (k, a), (_, b) in zip(prod.state_dict().items(), ref.state_dict().items()))
    print(f"{name}: second step from the restored state, max |dparam| vs the oracle {worst:.3e}")
    for (k, a), (_, b) in zip(prod.state_dict().items(), ref.state_dict().items()):
        assert (a.cpu() - b).abs().max().item() < 2.5e-4, k
    # <- and back: torch's checkpoint into a fresh HIP model and fused optimizer
    torch.save({"epoch": 4, "model_state_dict": ref.state_dict(), "optimizer_state_dict": ropt.state_dict(),
                "scheduler": "scheduler", "val_loss": 0.1}, path)
    seed_everything(99)
    fresh = MTnnUNet(1, 1, 3).to(DEV)
    fopt = _make(name, fresh, 0.5)
    CK.load_pretrained_model(fresh, path, optimizer=fopt)
    assert fopt.param_groups[0]["lr"] == lr
    if name == "AdamW":
        assert fopt.step_count == 2
    for (k, a), (_, b) in zip(fresh.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a.cpu(), b), k
    sd, rsd = fopt.state_dict()["state"], ropt.state_dict()["state"]
    assert set(sd) == set(rsd)
    for i in rsd:
        for key in keys - {"step"}:
            assert torch.equal(sd[i][key].cpu(), rsd[i][key]), (i, key)
    # a third step on both sides from the state torch wrote
    img3, mask3, label3 = O.synthetic_batch(2, 64, 64, seed=3)
    O.train_step(ref, ropt, img3, mask3, label3, 0.5, True, 3)
    FusedTrainStep(fresh, fopt, alpha=0.5)(img3.to(DEV), mask3.to(DEV), label3.to(DEV))
    for (k, a), (_, b) in zip(fresh.state_dict().items(), ref.state_dict().items()):
        assert (a.cpu() - b).abs().max().item() < 2.5e-4, k


# ------------------------------------------------------------------------------------------------ the per-fold loop: load_indexed, metrics, scheduler, checkpoint
@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_fit_fold_drives_the_fused_optimizers(name, tmp_path):
    """trainer.fit_fold over a device-resident dataset (load_indexed), with training metrics and a cosine schedule on the fused optimizer: two epochs move
    the parameters, the learning rate of the day reaches the launch, and model_best carries the optimizer state in torch's layout."""
    from multi_task_breast_cancer_amd import device_data as DD
    from multi_task_breast_cancer_amd import trainer as T
    from multi_task_breast_cancer_amd.dataset_index import EpochIndex
    img, mask, label = O.synthetic_batch(14, 64, 64, seed=33)
    ds = DD.DeviceDataset(img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long())
    seed_everything(1993)
    model = MTnnUNet(1, 1, 3).to(DEV)
    model.ensure_flat()
    p0 = model.flat_p.clone()
    opt = _make(name, model)
    step = FusedTrainStep(model, opt, alpha=0.5, metrics=True)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20, eta_min=1e-5)
    run_dir = str(tmp_path / "fold_0")
    rows = T.fit_fold(step, T.FusedEvalStep(model, alpha=0.5), ds, EpochIndex(np.arange(10), 4, seed=13), EpochIndex(np.arange(10, 14), 4, seed=13),
                      scheduler, run_dir, epochs=2, max_patience=5, transforms={"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0},
                      seed=13, plateau=False)
    assert len(rows) == 2 and rows[0][1] == 1e-3 and rows[1][1] < rows[0][1]
    assert all(np.isfinite(v) for r in rows for v in r) and all(0.0 <= v <= 1.0 for r in rows for v in r[4:])
    assert opt.applied_steps() == 6                              # two epochs of 10 samples in batches of 4 + 4 + 2 (drop_last=False, the reference's loader)
    assert not torch.equal(model.flat_p, p0)
    ckpt = torch.load(os.path.join(run_dir, "model_best"), map_location="cpu", weights_only=False)
    keys = {"momentum_buffer"} if name == "SGD" else {"step", "exp_avg", "exp_avg_sq"}
    assert all(set(s) == keys for s in ckpt["optimizer_state_dict"]["state"].values()) and len(ckpt["optimizer_state_dict"]["state"]) > 0
    ref = O.build_oracle_model("MTnnUNet", 1, 1, 3, True)
    _torch_opt(name, ref.parameters()).load_state_dict(ckpt["optimizer_state_dict"])      # torch takes it


def test_loading_an_sgd_state_keeps_the_devices_count_of_applied_steps():
    """torch.optim.SGD's state carries no step count: a resumed FusedSGD reports at least one applied update, and a count the dynamic loss scale
    already holds stays what it is."""
    model = MTnnUNet(1, 1, 3).to(DEV)
    theirs = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    for q in model.parameters():
        q.grad = torch.ones_like(q)
    theirs.step()
    sd = theirs.state_dict()
    model.zero_grad(set_to_none=True)
    fresh = FusedSGD(model, lr=0.5)
    fresh.load_state_dict(sd)
    assert fresh.applied_steps() == 1 and fresh.param_groups[0]["lr"] == 1e-3
    used = torch.cat([fresh.momentum_buffer[s.offset:s.offset + s.numel] for s in model.slots.values()])
    assert bool((used == 1).all())
    scaled = FusedSGD(model, lr=0.5)
    sc = DynamicLossScale()
    sc.attach(scaled)
    sc.ensure(DEV)
    sc.set_t(5)
    scaled.load_state_dict(sd)
    assert sc.stats()["t"] == 5 == scaled.applied_steps()
