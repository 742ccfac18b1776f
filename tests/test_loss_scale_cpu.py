"""The dynamic loss scale's host side, on a machine without a GPU: the C-ABI additions (exports, struct layout against the header through gcc),
the update rule -- `mtbc_loss_scale_update_host` runs the same inline function as the device kernel -- against `torch._amp_update_scale_`, the
state-dict interchange with torch.amp.GradScaler, and the checkpoint key."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L   # noqa: E402

NEW = ("mtbc_loss_scale_begin", "mtbc_loss_scale_check", "mtbc_loss_scale_optim", "mtbc_loss_scale_update_host", "mtbc_loss_scale_begin_host")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_loss_scale_symbols_are_declared_bound_and_exported(lib):
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(mtbc_[A-Za-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.mtbc_version() == 203 == L.ABI_VERSION


def test_loss_scale_ctypes_layout_matches_header(tmp_path):
    structs = {"mtbc_loss_scale_state": L.LossScaleState, "mtbc_loss_scale_args": L.LossScaleArgs}
    offs = [("mtbc_loss_scale_state", f, getattr(L.LossScaleState, f).offset) for f, _ in L.LossScaleState._fields_]
    offs += [("mtbc_loss_scale_args", f, getattr(L.LossScaleArgs, f).offset) for f, _ in L.LossScaleArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for name in structs:
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for s, f, _ in offs:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, typ in structs.items():
        assert int(got[name]) == C.sizeof(typ), (name, got[name], C.sizeof(typ))
    for s, f, off in offs:
        assert int(got[f"{s}.{f}"]) == off, (s, f)
    assert C.sizeof(L.LossScaleState) == 64                      # DynamicLossScale keeps it as 16 int32 words


def _args(st, growth, backoff, interval):
    a = L.LossScaleArgs()
    a.state = C.addressof(st)
    a.growth_factor, a.backoff_factor, a.growth_interval = growth, backoff, interval
    a.inv_world, a.beta1, a.beta2 = 1.0, 0.9, 0.999
    return a


@pytest.mark.parametrize("interval,growth,backoff,init", [(5, 2.0, 0.5, 65536.0), (3, 1.7, 0.3, 1000.0)])
def test_update_rule_is_torch_amp_update_scale(lib, interval, growth, backoff, init):
    """torch.amp.GradScaler.update() is torch._amp_update_scale_: over a random found / not-found sequence the scale and the growth tracker must be
    EQUAL to torch's at every step (factors that are not powers of two included: the product is taken in double and rounded once, as torch does),
    t counts the clean steps and `skipped` the others."""
    rng = random.Random(interval)
    st = L.LossScaleState()
    st.scale = init
    a = _args(st, growth, backoff, interval)
    scale, tracker = torch.full((1,), init, dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    clean = skipped = 0
    for step in range(400):
        found = rng.random() < 0.2
        st.found_inf = 1 if found else 0
        assert lib.mtbc_loss_scale_update_host(C.byref(a)) == 0
        torch._amp_update_scale_(scale, tracker, torch.tensor([1.0 if found else 0.0]), growth, backoff, interval)
        clean, skipped = clean + (not found), skipped + found
        assert st.scale == scale.item() and st.growth_tracker == tracker.item(), (step, st.scale, scale.item(), st.growth_tracker, tracker.item())
        assert st.found_inf == 0 and st.t == clean and st.skipped == skipped
    assert clean > 100 and skipped > 30


def test_update_rule_keeps_a_scale_that_would_grow_to_inf(lib):
    st = L.LossScaleState()
    st.scale = 2.0 ** 127
    a = _args(st, 2.0, 0.5, 1)
    scale, tracker = torch.full((1,), 2.0 ** 127), torch.zeros(1, dtype=torch.int32)
    lib.mtbc_loss_scale_update_host(C.byref(a))
    torch._amp_update_scale_(scale, tracker, torch.zeros(1), 2.0, 0.5, 1)
    assert st.scale == scale.item() == 2.0 ** 127 and st.growth_tracker == tracker.item() == 0 and st.t == 1


def test_begin_scalars_on_the_host_are_mtbc_optim_dynamics(lib):
    """What `begin` leaves for the Adam launch of step t + 1, evaluated by the shared inline function on the host: bit-equal to the first three scalars
    of mtbc_optim_dynamic (the static path's), with grad_scale = (1 / world) / scale."""
    for t in (0, 1, 2, 9, 99, 999, 11999):
        st = L.LossScaleState()
        st.scale, st.lr, st.t, st.shard_weight = 4096.0, 1e-3, t, 1.0
        a = _args(st, 2.0, 0.5, 2000)
        a.inv_world = 0.5
        assert lib.mtbc_loss_scale_begin_host(C.byref(a)) == 0
        ad = L.OptimArgs()
        ad.kind, ad.weight_decay = L.OPT_ADAMW, 0.0
        ad.lr, ad.beta1, ad.beta2, ad.eps, ad.grad_scale, ad.step = 1e-3, 0.9, 0.999, 1e-4, 0.5 / 4096.0, t + 1
        out = (C.c_float * 4)()
        assert lib.mtbc_optim_dynamic(C.byref(ad), C.byref(out)) == 0
        assert list(st.adam) == list(out)[:3], (t, list(st.adam), list(out))
        assert st.t == t


def test_bad_arguments_are_refused(lib):
    st = L.LossScaleState()
    a = _args(st, 2.0, 0.5, 0)
    assert lib.mtbc_loss_scale_update_host(C.byref(a)) != 0        # growth_interval >= 1
    a = _args(st, 2.0, 0.5, 4)
    a.state = None
    assert lib.mtbc_loss_scale_update_host(C.byref(a)) != 0


def test_state_dict_interchanges_with_torch_gradscaler():
    from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale
    ours = DynamicLossScale(init_scale=1024.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
    sd = ours.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    gs = torch.amp.GradScaler("cpu")
    assert set(gs.state_dict()) == set(sd)
    gs.load_state_dict(sd)
    back = gs.state_dict()
    assert back == sd, (back, sd)
    gs2 = torch.amp.GradScaler("cpu", init_scale=8.0, growth_factor=3.0, backoff_factor=0.125, growth_interval=11)
    other = DynamicLossScale()
    other.load_state_dict(gs2.state_dict())
    assert other.state_dict() == gs2.state_dict()
    assert other.stats() == {"scale": 8.0, "growth_tracker": 0, "skipped": 0, "t": 0}
    with pytest.raises(ValueError):
        DynamicLossScale(growth_factor=1.0)
    with pytest.raises(ValueError):
        DynamicLossScale(backoff_factor=1.0)


def test_checkpoint_carries_the_scaler_under_its_own_key(tmp_path):
    from multi_task_breast_cancer_amd.checkpoint import load_pretrained_model, save_checkpoint
    from multi_task_breast_cancer_amd.loss_scale import DynamicLossScale
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sc = DynamicLossScale(init_scale=512.0, growth_interval=9)
    save_checkpoint(str(tmp_path / "with.pth"), 3, model, opt, 0.5, scaler=sc)
    save_checkpoint(str(tmp_path / "without.pth"), 3, model, opt, 0.5)
    ck = torch.load(str(tmp_path / "with.pth"), weights_only=False)
    assert ck["loss_scaler_state_dict"] == sc.state_dict()
    assert set(ck) - {"loss_scaler_state_dict"} == set(torch.load(str(tmp_path / "without.pth"), weights_only=False))
    fresh = DynamicLossScale()
    load_pretrained_model(torch.nn.Linear(3, 2), str(tmp_path / "with.pth"), optimizer=None, scaler=fresh)
    assert fresh.state_dict() == sc.state_dict()
    untouched = DynamicLossScale(init_scale=2.0)
    load_pretrained_model(torch.nn.Linear(3, 2), str(tmp_path / "without.pth"), scaler=untouched)     # an old file: loads as before
    assert untouched.stats()["scale"] == 2.0


def test_trainer_keyword_and_switch_are_declared():
    import inspect
    from multi_task_breast_cancer_amd import switches
    from multi_task_breast_cancer_amd.trainer import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["loss_scale"].default is None
    assert switches.PLAN_SWITCHES["MTBC_DYN_SCALE"][0] == "0"
