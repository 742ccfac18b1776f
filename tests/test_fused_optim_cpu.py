"""Fused Adam / SGD (Nesterov) / AdamW on a machine without a GPU: the C-ABI additions (exports, the struct's layout against the header through gcc),
the per-step scalars, the update rule -- `mtbc_optim_step_host` runs the same inline element function as the device kernel -- against torch.optim.Adam /
torch.optim.SGD / torch.optim.AdamW (experiment_init.py:186-191), the words Adam's own kernel wrote before it moved onto the shared launch
(tests/golden/adam_steps.npz), and the factory's `fused=True`."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L   # noqa: E402
from multi_task_breast_cancer_amd import ops   # noqa: E402

NEW = ("mtbc_optim_step", "mtbc_optim_dynamic", "mtbc_loss_scale_optim", "mtbc_optim_step_host")
KINDS = {"SGD": L.OPT_SGD, "AdamW": L.OPT_ADAMW, "Adam": L.OPT_ADAMW}
# the hyper-parameters that tell the names apart: Adam is the AdamW rule without decay, at the eps the reference runs it with (experiment_init.py:187)
RULE = {"SGD": dict(weight_decay=1e-2, eps=1e-8), "AdamW": dict(weight_decay=1e-2, eps=1e-8), "Adam": dict(weight_decay=0.0, eps=1e-4)}
GOLDEN = os.path.join(ROOT, "tests", "golden", "adam_steps.npz")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


# ------------------------------------------------------------------------------------------------ 1. exports and layout
def test_optim_symbols_are_declared_bound_and_exported(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(mtbc_[A-Za-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.mtbc_version() == 203 == L.ABI_VERSION           # 203: Adam's own struct and entry points left, Adam is mtbc_optim_args (ADAMW, weight_decay 0)
    assert (L.OPT_SGD, L.OPT_ADAMW) == tuple(int(re.search(rf"#define\s+MTBC_OPT_{k}\s+(\d+)", src).group(1)) for k in ("SGD", "ADAMW"))


def test_optim_args_ctypes_layout_matches_header(tmp_path):
    offs = [("mtbc_optim_args", f, getattr(L.OptimArgs, f).offset) for f, _ in L.OptimArgs._fields_]
    assert {"kind", "dynamic", "skip", "scale_state"} <= {f for _, f, _ in offs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("mtbc_optim_args %zu\\n", sizeof(mtbc_optim_args));']
    for s, f, _ in offs:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["mtbc_optim_args"]) == C.sizeof(L.OptimArgs)
    for s, f, off in offs:
        assert int(got[f"{s}.{f}"]) == off, (s, f)


# ------------------------------------------------------------------------------------------------ 2. the per-step scalars
ROWS = [(1e-4, 0.9, 0.999, 1, 1.0), (3e-4, 0.9, 0.999, 7, 1.0 / 4096.0), (5e-4, 0.8, 0.99, 12345, 0.125), (1e-6, 0.9, 0.999, 2_000_000, 1.0)]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_optim_dynamic_scalars_are_the_double_precision_expressions(lib, wd):
    """{grad_scale, lr / (1 - b1^t), 1 / sqrt(1 - b2^t), 1 - lr wd} for AdamW -- each in double on the float32 members widened first, rounded once, the
    first three as torch.optim.Adam's scalar path and the last as torch's `param.mul_(1 - lr * weight_decay)` -- and {grad_scale, lr, 1, 1} for SGD."""
    f32 = lambda x: float(np.float32(x))
    for lr, b1, b2, t, gs in ROWS:
        a = ops.optim_args(L.OPT_ADAMW, 0, None, None, None, lr=lr, beta1=b1, beta2=b2, eps=1e-4, weight_decay=wd, grad_scale=gs, step=t)
        out = (C.c_float * 4)()
        assert lib.mtbc_optim_dynamic(C.byref(a), C.byref(out)) == 0
        want = (np.float32(gs), np.float32(f32(lr) / (1.0 - math.pow(f32(b1), t))), np.float32(1.0 / math.sqrt(1.0 - math.pow(f32(b2), t))),
                np.float32(1.0 - f32(lr) * f32(wd)))
        assert tuple(np.float32(v) for v in out) == want, (lr, b1, b2, t, list(out), want)
        if wd == 0.0:
            assert out[3] == 1.0                                  # Adam: the decay factor is exactly one
        a.kind = L.OPT_SGD
        assert lib.mtbc_optim_dynamic(C.byref(a), C.byref(out)) == 0
        assert tuple(np.float32(v) for v in out) == (np.float32(gs), np.float32(lr), np.float32(1.0), np.float32(1.0))
    for kind in set(KINDS.values()):
        bad = ops.optim_args(kind, 0, None, None, None, step=0)
        assert lib.mtbc_optim_dynamic(C.byref(bad), C.byref((C.c_float * 4)())) != 0        # t >= 1
    assert lib.mtbc_optim_dynamic(C.byref(ops.optim_args(2, 0, None, None, None)), C.byref((C.c_float * 4)())) != 0   # no such kind


# ------------------------------------------------------------------------------------------------ 3. the rule against torch
def _ptr(x):
    return x.ctypes.data if x is not None else None


def host_step(lib, kind, p, g, m, v=None, **kw):
    """mtbc_optim_step_host on numpy float32 arrays, in place."""
    for x in (p, g, m, v):
        assert x is None or (x.dtype == np.float32 and x.flags.c_contiguous)
    dyn, skip, st = kw.pop("dynamic", None), kw.pop("skip", None), kw.pop("scale_state", None)
    a = ops.optim_args(kind, p.size, _ptr(p), _ptr(g), _ptr(m), _ptr(v), dynamic=_ptr(dyn), skip=_ptr(skip),
                       scale_state=C.addressof(st) if st is not None else None, **kw)
    return lib.mtbc_optim_step_host(C.byref(a))


def aligned(n):
    """n float32 zeros at a 16-byte aligned address (what mtbc_optim_args asks of p, g, m, v; numpy promises less for small arrays)."""
    raw = np.zeros(n + 4, dtype=np.float32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + n]
    assert out.ctypes.data % 16 == 0
    return out


def aligned_copy(x):
    out = aligned(x.size)
    out[:] = x
    return out


def _torch_opt(name, params, lr):
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, nesterov=True, foreach=False)
    if name == "Adam":
        return torch.optim.Adam(params, lr=lr, eps=1e-4, foreach=False)
    return torch.optim.AdamW(params, lr=lr, foreach=False)


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_host_rule_matches_torch(lib, name, n):
    """Four steps on gradients of four magnitudes (test_adam_matches_torch's) against torch's own optimizer in float32 AND its float64 twin on the same
    float32 gradients.  Per step: max |host - t64| <= 2 max |t32 - t64| + 2^-23 max |p| -- twice the reference's own rounding distance plus one ulp at the
    largest parameter; the factor 2 covers torch's different association (reciprocal-multiply against divide in Adam's denominator)."""
    gen = torch.Generator().manual_seed(21)
    lr = 1e-3
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10 ** float(e) for e in (-6, -3, 0, -2)]
    p32, p64 = p0.clone().requires_grad_(True), p0.double().requires_grad_(True)
    o32, o64 = _torch_opt(name, [p32], lr), _torch_opt(name, [p64], lr)
    g0 = o32.param_groups[0]
    p, m, v = aligned_copy(p0.numpy()), aligned(n), (aligned(n) if name != "SGD" else None)
    hyper = dict(lr=lr, momentum=0.9, nesterov=True) if name == "SGD" else \
        dict(lr=lr, beta1=g0["betas"][0], beta2=g0["betas"][1], eps=g0["eps"], weight_decay=g0["weight_decay"])
    worst = 0.0
    for t, gr in enumerate(grads, start=1):
        p32.grad, p64.grad = gr.clone(), gr.double()
        o32.step()
        o64.step()
        g = aligned_copy(gr.numpy())
        assert host_step(lib, KINDS[name], p, g, m, v, step=t, **hyper) == 0
        assert np.array_equal(g, gr.numpy())                      # zero_grad = 0: the gradient stays
        ref = p64.detach().numpy()
        mine = np.abs(p.astype(np.float64) - ref).max()
        theirs = np.abs(p32.detach().numpy().astype(np.float64) - ref).max()
        bound = 2.0 * theirs + 2.0 ** -23 * np.abs(ref).max()
        ratio = mine / bound
        worst = max(worst, ratio)
        print(f"{name} n={n} step {t}: max|host - t64| = {mine:.3e}, max|t32 - t64| = {theirs:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
        assert mine <= bound, (name, n, t, mine, theirs, bound)
    print(f"{name} n={n}: worst ratio to the bound {worst:.3f}")
    # the state too, against the float64 twin's.  The kernel holds momentum and the betas as float32 (mtbc_optim_args), the twin as doubles: half an
    # ulp of 0.9 is 2^-25 / 0.9 of the buffer per step; 1 - b1 and 1 - b2 taken from the float32 betas are off by 2^-25 / 0.1 and 2^-25 / 0.001
    # relative.  On top of that one to three roundings per element and step.
    st64 = o64.state[p64]
    rel = {"momentum_buffer": 4 * 2.0 ** -25 / 0.9 + 4 * 2.0 ** -24, "exp_avg": 2.0 ** -25 / 0.1 + 8 * 2.0 ** -24, "exp_avg_sq": 2.0 ** -25 / 0.001 + 12 * 2.0 ** -24}
    for key, mine in (("momentum_buffer", m),) if name == "SGD" else (("exp_avg", m), ("exp_avg_sq", v)):
        ref = st64[key].numpy()
        assert np.abs(mine.astype(np.float64) - ref).max() <= rel[key] * np.abs(ref).max(), key


# ------------------------------------------------------------------------------------------------ 3b. Adam: the words of the kernel it had to itself
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_host_adam_reproduces_the_words_recorded_from_adams_own_kernel(lib, n):
    """tests/golden/adam_steps.npz (tools/make_adam_fixture.py) holds p, exp_avg, exp_avg_sq and g after each of five ops.adam_step launches, recorded on
    the GPU at the last commit at which Adam had its own kernel.  The shared element function -- AdamW, weight_decay 0 -- gives every one of those words,
    on the tail elements (n = 1 and 3 are all tail) as on the float4 body; the fifth step clears g."""
    z = np.load(GOLDEN)
    f32 = lambda words: aligned_copy(np.ascontiguousarray(words).view(np.float32))
    p, m, v = f32(z[f"n{n}_p0"]), aligned(n), aligned(n)
    grads = z[f"n{n}_grads"]
    assert grads.shape == (5, n) and grads.dtype == np.int32
    for t in range(1, 6):
        g = f32(grads[t - 1])
        assert host_step(lib, L.OPT_ADAMW, p, g, m, v, lr=1e-4, step=t, eps=1e-4, weight_decay=0.0, grad_scale=0.25, zero_grad=(t == 5)) == 0
        for key, mine in (("p", p), ("m", m), ("v", v), ("g", g)):
            assert np.array_equal(mine.view(np.int32), z[f"n{n}_{key}"][t - 1]), (n, t, key)
    assert not g.any() and v.any()


# ------------------------------------------------------------------------------------------------ 4. exact statements on the host path
def _case(n=1027, seed=5):
    rng = np.random.default_rng(seed)
    mk = lambda s=1.0: aligned_copy((rng.standard_normal(n) * s).astype(np.float32))
    return mk(), mk(1e-2), mk(0.1), aligned_copy(np.abs(rng.standard_normal(n) * 1e-3).astype(np.float32))


@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_host_grad_scale_zero_grad_and_skip_are_exact(lib, name):
    kind = KINDS[name]
    hyper = dict(lr=1e-3, step=3, **RULE[name])
    p0, g0, m0, v0 = _case()
    use_v = lambda v: v if name != "SGD" else None
    # grad_scale = 1/8 on 8 g is grad_scale = 1 on g (a power of two: g' is the same float)
    p1, g1, m1, v1 = (aligned_copy(x) for x in (p0, g0 * np.float32(8.0), m0, v0))
    p2, g2, m2, v2 = (aligned_copy(x) for x in (p0, g0, m0, v0))
    assert host_step(lib, kind, p1, g1, m1, use_v(v1), grad_scale=0.125, zero_grad=True, **hyper) == 0
    assert host_step(lib, kind, p2, g2, m2, use_v(v2), **hyper) == 0
    assert np.array_equal(p1, p2) and np.array_equal(m1, m2) and np.array_equal(v1, v2)
    assert not np.array_equal(p1, p0) and not np.array_equal(m1, m0)
    assert not g1.any() and np.array_equal(g2, g0)               # zero_grad clears g, and only then
    # a non-zero skip word: p, m, v bit-unchanged, g cleared
    skip = np.array([1], dtype=np.uint32)
    p3, g3, m3, v3 = (aligned_copy(x) for x in (p0, g0, m0, v0))
    assert host_step(lib, kind, p3, g3, m3, use_v(v3), zero_grad=True, skip=skip, **hyper) == 0
    assert np.array_equal(p3, p0) and np.array_equal(m3, m0) and np.array_equal(v3, v0) and not g3.any()
    g3[:] = g0
    assert host_step(lib, kind, p3, g3, m3, use_v(v3), skip=skip, **hyper) == 0
    assert np.array_equal(p3, p0) and np.array_equal(g3, g0)     # skipped without zero_grad: nothing moves at all
    skip[0] = 0
    assert host_step(lib, kind, p3, g3, m3, use_v(v3), skip=skip, **hyper) == 0
    assert np.array_equal(p3, p2) and np.array_equal(m3, m2)     # a clear word: the plain step


@pytest.mark.parametrize("name", ["SGD", "AdamW", "Adam"])
def test_host_scalars_from_memory_give_the_launch_arguments_bits(lib, name):
    """`dynamic` (4 floats from mtbc_optim_dynamic) and `scale_state` (what mtbc_loss_scale_begin_host leaves) against the plain arguments."""
    kind = KINDS[name]
    hyper = dict(lr=2.5e-4, step=7, grad_scale=1.0 / 4096.0, **RULE[name])
    p0, g0, m0, v0 = _case(259, seed=9)
    g0 = aligned_copy(g0 * np.float32(4096.0))
    use_v = lambda v: v if name != "SGD" else None
    pa, ga, ma, va = (aligned_copy(x) for x in (p0, g0, m0, v0))
    assert host_step(lib, kind, pa, ga, ma, use_v(va), **hyper) == 0
    out = (C.c_float * 4)()
    assert lib.mtbc_optim_dynamic(C.byref(ops.optim_args(kind, 0, None, None, None, **hyper)), C.byref(out)) == 0
    dyn = np.array(list(out), dtype=np.float32)
    pb, gb, mb, vb = (aligned_copy(x) for x in (p0, g0, m0, v0))
    wrong = dict(hyper, lr=1.0, step=1, grad_scale=3.0)          # not read when `dynamic` is set
    assert host_step(lib, kind, pb, gb, mb, use_v(vb), dynamic=dyn, **wrong) == 0
    assert np.array_equal(pa, pb) and np.array_equal(ma, mb) and np.array_equal(va, vb)
    st = L.LossScaleState()
    st.scale, st.lr, st.t, st.shard_weight = 4096.0, hyper["lr"], hyper["step"] - 1, 1.0
    ls = L.LossScaleArgs()
    ls.state, ls.growth_factor, ls.backoff_factor, ls.growth_interval, ls.inv_world, ls.beta1, ls.beta2 = C.addressof(st), 2.0, 0.5, 2000, 1.0, 0.9, 0.999
    assert lib.mtbc_loss_scale_begin_host(C.byref(ls)) == 0
    pc, gc, mc, vc = (aligned_copy(x) for x in (p0, g0, m0, v0))
    assert host_step(lib, kind, pc, gc, mc, use_v(vc), scale_state=st, **wrong) == 0
    assert np.array_equal(pa, pc) and np.array_equal(ma, mc) and np.array_equal(va, vc)


def test_host_refuses_what_the_launch_refuses(lib):
    p, g, m, v = _case(8)
    assert host_step(lib, L.OPT_ADAMW, p, g, m, None) == -2                   # AdamW needs v
    assert host_step(lib, L.OPT_SGD, p, g, m, None) == 0                      # SGD does not
    assert host_step(lib, 2, p, g, m, v) == -5                                # no such kind
    assert host_step(lib, L.OPT_SGD, p, g, m, None, step=0) == -1
    assert host_step(lib, L.OPT_SGD, p[1:], g[1:], m[1:], None) == -5         # 16-byte alignment, as the kernel's float4 body needs


# ------------------------------------------------------------------------------------------------ 5. the factory
def test_factory_fused_keyword():
    from multi_task_breast_cancer_amd.experiment_init import init_optimizer
    from multi_task_breast_cancer_amd.nets import MTnnUNet
    from multi_task_breast_cancer_amd.optim import FusedAdamW, FusedSGD
    model = MTnnUNet(1, 1, 3)
    sgd, adamw, other = (init_optimizer(model, name, 3e-4, fused=True) for name in ("SGD", "AdamW", "RMSprop"))
    assert type(sgd) is FusedSGD and type(adamw) is FusedAdamW and type(other) is FusedSGD
    assert sgd.param_groups[0]["lr"] == 3e-4 and adamw.param_groups[0]["lr"] == 3e-4
    assert other.param_groups[0]["lr"] == 0.001                  # the reference's fallback: SGD at lr 0.001 whatever was asked
    for o in (sgd, other):
        assert o.param_groups[0]["momentum"] == 0.9 and o.param_groups[0]["nesterov"] is True
    for name in ("SGD", "AdamW"):
        assert type(init_optimizer(model, name, 3e-4)).__name__ == name == type(init_optimizer(model, name, 3e-4, fused=False)).__name__
        assert type(init_optimizer(model, name, 3e-4)).__module__.startswith("torch.optim")
    # the hyper-parameters are the installed torch optimizer's own set: the param group loads into one, and torch's loads here
    for ours, make in ((sgd, lambda ps: torch.optim.SGD(ps, lr=1.0, momentum=0.5)), (adamw, lambda ps: torch.optim.AdamW(ps, lr=1.0))):
        theirs = make(model.parameters())
        sd = ours.state_dict()
        assert set(sd["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
        theirs.load_state_dict({"state": {}, "param_groups": sd["param_groups"]})
        want = {k: v for k, v in ours.param_groups[0].items() if k != "params"}
        assert {k: v for k, v in theirs.param_groups[0].items() if k != "params"} == want
        ours.load_state_dict(make(model.parameters()).state_dict())
        assert ours.param_groups[0]["lr"] == 1.0
    assert adamw.param_groups[0]["weight_decay"] == torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"] == 1e-2


def test_host_adamw_second_moment_takes_the_tail_form_from_the_last_multiple_of_four(lib):
    """The kernel's scalar tail (the elements from n & ~3 on) sums v as two float32 products and an add, as the Adam kernel's tail does; the float4 body
    fuses the sum.  The host loop follows the same split: on the tail v is the plain float32 expression bit for bit, for every n down to an all-tail 1."""
    f = np.float32
    for n in (1, 3, 4, 7, 1027):
        p, g, m, v = _case(n, seed=n)
        v0, g0 = v.copy(), g.copy()
        assert host_step(lib, L.OPT_ADAMW, p, g, m, v, lr=1e-3, step=2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=0.5) == 0
        gp = f(0.5) * g0
        want = gp * ((f(1.0) - f(0.999)) * gp) + f(0.999) * v0
        body = n & ~3
        assert np.array_equal(v[body:], want[body:]), n
        assert np.abs(v[:body] - want[:body]).max(initial=0.0) <= 2.0 ** -23 * np.abs(want).max()      # the fused form: within an ulp of it


def test_loss_scale_optim_refuses_a_null_optimizer_as_a_bad_argument(lib):
    st = L.LossScaleState()
    ls = L.LossScaleArgs()
    ls.state, ls.growth_factor, ls.backoff_factor, ls.growth_interval, ls.inv_world, ls.beta1, ls.beta2 = C.addressof(st), 2.0, 0.5, 2000, 1.0, 0.9, 0.999
    assert lib.mtbc_loss_scale_optim(C.byref(ls), None, None) == -2       # MTBC_E_BADARG before any launch, as every other NULL pointer
