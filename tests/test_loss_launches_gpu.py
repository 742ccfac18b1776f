"""The launches of a step's loss program -- the segmentation criterion's forward and backward (OP_DICE_FWD / _BWD, all four kinds), the
classification criterion (OP_FOCAL), the loss mix -- and the softmax pair of the 3-class classifier, held to float64 cases by their ARGUMENTS.

LOSS_CASES holds one row per branch the dispatchers and kernels of csrc/head_loss.hip can take for these ops, each at the smallest shape
at which the branch exists.  A row builds its argument structs with the one filler the engine uses (ops.dice_case_args / focal_case_args /
softmax_args), derives its coverage key with tests/step_programs.py's _loss_key, runs that same struct and compares every output with float64
autograd of the restated criterion on the same float32 inputs.  The guard at the end surveys the benchmark's step programs: a loss launch
whose key no row makes fails it.

Every backward runs with a host factor (gscale) AND a device word (*gscale_dev) that both differ from 1, as the engine always sets them (the
shard weight, and under the dynamic loss scale the scale itself): a kernel that dropped either would be off by that factor.

Bounds, all the project's own:
  Dice family   tests/test_seg_criteria_gpu.py _against_float64: per-head loss 2e-6, total 5e-6 (both x planes for Jaccard's sum); dx relative
                1e-4 plus an absolute 1e-9 that was set at gscale = 0.35 -- dx is linear in gscale * *gscale_dev, so 1e-9 * that / 0.35
  Focal         test_focal_matches_reference_goldens: loss 1e-6; dx relative 1e-4 plus 1e-7 * gscale * *gscale_dev / 0.65
  softmax       tests/test_cls_only_cpu.py `within`: 8 x the error torch's own float32 softmax / backward shows on the same rows, floor 1 ulp"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import ops  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402
from step_programs import STEP_PROGRAMS, _loss_key, assert_all_tested, survey  # noqa: E402
from test_cls_only_cpu import softmax_references, within  # noqa: E402
from test_seg_criteria_gpu import NAME, RESTATED  # noqa: E402

L = ops.L
DEV = torch.device("cuda:0")
KINDS = (L.SEG_DICE, L.SEG_BCE, L.SEG_FOCALDICE, L.SEG_JACCARD)
GSCALE, GDEV = 0.35, 1.75          # alpha * loss_scale of an fp32 step; a shard that weighs 1.75 x its share
GSCALE_F16 = 0.5 * 65536           # alpha 0.5 times the fp16 mode's loss scale

# (n_heads, N, C, H, W), mode, kinds: the branch of csrc/head_loss.hip the row is there for
_DICE_SHAPES = [
    ((4, 2, 1, 128, 128), {}, KINDS),                        # 1024 threads, every thread exactly one unrolled round
    ((3, 2, 1, 128, 128), {}, (L.SEG_DICE,)),                # ... with the three heads of the Multi_BTSUNet programs (tests/test_mt_btsunet_launches_gpu.py)
    ((4, 2, 1, 128, 256), dict(gscale=GSCALE_F16), KINDS),   # more than one round (the 256 x 256 and 512 x 512 programs), the fp16 mode's gscale
    ((1, 1, 1, 512, 512), {}, (L.SEG_DICE,)),                # 16 rounds: the longest per-thread accumulation a program has
    ((2, 2, 1, 128, 160), {}, KINDS),                        # one unrolled round, then one trip of the rest loop for every thread
    ((1, 1, 1, 120, 256), {}, KINDS),                        # n4 = 4096 + 3584: half the block takes a second round, the others three rest trips
    ((2, 2, 1, 96, 96), {}, KINDS),                          # 256 threads: two rounds, then a rest trip
    ((2, 2, 1, 6, 5), {}, KINDS),                            # the scalar loops: H * W % 4 != 0
    ((1, 2, 1, 16, 16), dict(misaligned=True), KINDS),       # ... and by alignment: x[0] and dx[0] start one element into their buffers
    ((1, 2, 3, 16, 16), {}, KINDS),                          # C > 1: planes = N * C
    ((1, 257, 1, 128, 128), {}, KINDS),                      # a finalize thread sums two planes; 4 210 688 elements: the capped backward grid loops
]
# (N, C), gamma, weight
_FOCAL_SHAPES = [((32, 3), 2.0, False), ((300, 3), 2.0, True), ((7, 3), 0.0, False), ((5, 1), 0.0, False), ((300, 1), 0.0, False),
                 ((6, 3), 0.5, False)]
_SOFTMAX_SHAPES = [(5, 3), (70, 3)]

LOSS_CASES = [("dice", shape, dict(mode, kind=kind)) for shape, mode, kinds in _DICE_SHAPES for kind in kinds] + \
             [("focal", shape, dict(gamma=gamma, weight=weight)) for shape, gamma, weight in _FOCAL_SHAPES] + \
             [("softmax", shape, {}) for shape in _SOFTMAX_SHAPES]


def _case_id(case):
    family, shape, mode = case
    what = NAME[mode["kind"]] if family == "dice" else f"gamma{mode['gamma']:g}" + ("-w" if mode["weight"] else "") if family == "focal" else ""
    return "-".join([family, "x".join(map(str, shape))] + ([what] if what else []) + [k for k in ("misaligned",) if mode.get(k)])


def _weights(nh):
    return [1.0 / (nh - i) for i in range(nh)]


def _softmax_op(N, Cc, backward, x=None, p=None, dp=None, dz=None):
    op = ops._small_op(L.OP_SOFTMAX)
    ops.softmax_args(N, Cc, backward, x=x, p=p, dp=dp, dz=dz, into=op.u.softmax)
    return op


def _case_ops(case, ptrs=None):
    """[op] of the calls a row makes, each through its struct's one filler (dummy pointers without ptrs; the misaligned row's dummies start one
    element in, as its tensors do)."""
    family, shape, mode = case
    if family == "dice":
        made = [ops.dice_case_args(k, *shape, ptrs=ptrs, seg_kind=mode["kind"], weights=_weights(shape[0]), gscale=mode.get("gscale", GSCALE),
                                   gscale_dev=True) for k in (L.OP_DICE_FWD, L.OP_DICE_BWD)]
        if mode.get("misaligned") and ptrs is None:
            for op in made:
                op.u.dice.x[0] += 4
            made[1].u.dice.dx[0] += 4
        return made
    if family == "focal":
        return [ops.focal_case_args(*shape, ptrs=ptrs, gamma=mode["gamma"], weight=mode["weight"], gscale=GSCALE, gscale_dev=True)]
    if ptrs is None:
        ptrs = dict(x=1 << 20, p=2 << 20, dp=3 << 20, dz=4 << 20)
    return [_softmax_op(*shape, False, x=ptrs["x"], p=ptrs["p"]), _softmax_op(*shape, True, p=ptrs["p"], dp=ptrs["dp"], dz=ptrs["dz"])]


def _mix_op():
    op = ops._small_op(L.OP_LOSS_MIX)
    op.u.mix.seg, op.u.mix.cls, op.u.mix.alpha, op.u.mix.out4 = 1 << 20, 2 << 20, 0.5, 3 << 20
    return op


def _reference_tested_loss_keys():
    """(op kind, key) of every call the rows of LOSS_CASES make, from their argument structs; the mix has one key, and
    tests/test_ops_gpu.py::test_loss_mix_is_the_written_fp32_expression_and_flags_nan answers for it bit for bit."""
    keys = {(op.kind, _loss_key(op)) for case in LOSS_CASES for op in _case_ops(case)}
    return keys | {(L.OP_LOSS_MIX, _loss_key(_mix_op()))}


class _Out:
    """A device tensor `off` elements into a buffer pre-filled with a mark, 64 elements (256 bytes) of it on each side."""
    PAD, MARK = 64, 1993.0

    def __init__(self, shape, vals=None, off=0):
        n = int(torch.Size(shape).numel())
        flat = torch.full((n + 2 * self.PAD + 4,), self.MARK)
        self.lo = self.PAD + off
        if vals is not None:
            flat[self.lo:self.lo + n] = vals.reshape(-1)
        self.sent, self.n, self.shape = flat.clone(), n, tuple(shape)
        self.buf = flat.to(DEV)
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        assert self.view.data_ptr() % 16 == 4 * off

    def data_ptr(self):
        return self.view.data_ptr()

    def read(self, what):
        got = self.buf.cpu()
        assert bool((got[:self.lo] == self.MARK).all() and (got[self.lo + self.n:] == self.MARK).all()), f"{what}: written outside the tensor"
        return got[self.lo:self.lo + self.n].view(self.shape)

    def intact(self):
        return torch.equal(self.buf.cpu().view(torch.int32), self.sent.view(torch.int32))


def _launch(case, ptrs):
    """Runs the row's structs on the tensors `ptrs`: the real pointers plan what the dummies plan, and the launches made are those."""
    planned = [(op.kind, ops.op_kernel_name(op)) for op in _case_ops(case)]
    real = _case_ops(case, ptrs)
    assert [(op.kind, ops.op_kernel_name(op)) for op in real] == planned, "the real pointers plan something else than the dummies"
    ops.launched = []
    try:
        for op in real:
            ops.loss_op_launch(op)
        torch.cuda.synchronize()
        made = list(ops.launched)
    finally:
        ops.launched = None
    assert made == planned, (made, planned)
    return " + ".join(name for _, name in planned)


def _dx_close(what, got, want, atol):
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
    err = (got - want).abs()
    worst = (err / (atol + 1e-4 * want.abs())).max().item()
    print(f"  {what}: max err {err.max().item():.3e}, max |want| {want.abs().max().item():.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: max err {err.max().item():.3e} (max |want| {want.abs().max().item():.3e}), {worst:.2f} x the bound"


def _run_dice(case):
    _, (nh, N, Cc, H, W), mode = case
    kind, gscale, off = mode["kind"], mode.get("gscale", GSCALE), int(bool(mode.get("misaligned")))
    g = torch.Generator().manual_seed(1993 + 31 * nh + 7 * N + 5 * Cc + 3 * H + W + 101 * kind)
    planes, shape, weights = N * Cc, (N, Cc, H, W), _weights(nh)
    xs = [torch.randn(*shape, generator=g) * 2 for _ in range(nh)]
    t = (torch.rand(*shape, generator=g) > 0.7).float()
    if planes > 1:
        t.view(planes, -1)[1] = 0                             # an empty mask (class "normal")
    # float64 autograd of the restated criterion on the same float32 values
    xr = [x.double().requires_grad_(True) for x in xs]
    each = [RESTATED[kind](x, t.double()) for x in xr]
    total = sum(w * e for w, e in zip(weights, each))
    (gscale * GDEV * total).backward()
    X = [_Out(shape, x, off if i == 0 else 0) for i, x in enumerate(xs)]
    DX = [_Out(shape, None, off if i == 0 else 0) for i in range(nh)]
    T, loss = _Out(shape, t), _Out((nh + 1,))
    stats = torch.full((nh * planes * L.SEG_STATS_STRIDE[kind],), float("nan"), device=DEV)
    gdev = torch.tensor([GDEV], dtype=torch.float32, device=DEV)
    name = _launch(case, {"x": X, "dx": DX, "target": T, "stats": stats, "loss": loss, "gscale_dev": gdev})
    print(f"{_case_id(case)}: {name}")
    assert all(x.intact() for x in X) and T.intact() and gdev.item() == GDEV, "an input was written"
    got = loss.read("loss").double()
    assert bool(torch.isfinite(got).all()), got
    lscale = planes if kind == L.SEG_JACCARD else 1           # Jaccard is a SUM of `planes` terms of the size of one Dice term
    errs = [abs(got[i].item() - each[i].item()) for i in range(nh)] + [abs(got[nh].item() - total.item())]
    print(f"  loss {got.tolist()}: errors per head {[f'{e:.2e}' for e in errs[:nh]]} (bound {2e-6 * lscale:.1e}), total {errs[nh]:.2e} (bound {5e-6 * lscale:.1e})")
    for i in range(nh):
        _dx_close(f"dx head {i}", DX[i].read(f"dx head {i}"), xr[i].grad, 1e-9 * gscale * GDEV / 0.35)
    for i in range(nh):
        assert errs[i] < 2e-6 * lscale, (i, got[i].item(), each[i].item())
    assert errs[nh] < 5e-6 * lscale, (got[nh].item(), total.item())


def _focal_inputs(N, Cc, g):
    """Logits and targets (one-hot rows; for the one-logit head the {0, 1} label itself) with logits of +-30 on both target values.
    Every batch has them where sign and target agree: row 0 of three classes is (30, -30, .) on the target (1, 0, 0), rows 0 and 1 of the
    one-logit head are 30 on 1 and -30 on 0 -- p_t rounds to 1 and 1 - p_t to 0, the end at which the kernel guards pow(0, gamma - 1).
    A logit of 30 AGAINST its target is a sample loss of 30.  The loss bound is an absolute 1e-6 and float32 values between 8 and 16 are
    9.5e-7 apart, so a batch of 5 to 7 samples that held the two disagreeing pairs (a mean above 60 / 7) could not be held to it by any float32
    kernel; the batches of 32 and 300 samples (means below 4, spacing 2.4e-7) carry them too, in rows 2 and 3: all four pairs, p_t down to 0."""
    x = torch.randn(N, Cc, generator=g) * 2
    if Cc == 1:
        t = (torch.rand(N, 1, generator=g) > 0.5).float()
        x[:4, 0], t[:4, 0] = torch.tensor([30.0, -30.0, 30.0, -30.0]), torch.tensor([1.0, 0.0, 0.0, 1.0])
        if N < 32:
            x[2:4, 0] = torch.tensor([1.5, -0.5])
    else:
        label = torch.randint(0, Cc, (N,), generator=g)
        label[:4] = torch.tensor([0, 0, 1, 0])
        t = F.one_hot(label, Cc).float()
        x[0, :2] = torch.tensor([30.0, -30.0])
        if N >= 32:
            x[2:4, 0] = torch.tensor([30.0, -30.0])          # 30 on a 0 of row 2, -30 on the 1 of row 3
    pairs = {(v, tv) for v, tv in zip(x.reshape(-1).tolist(), t.reshape(-1).tolist()) if abs(v) == 30.0}
    assert {(30.0, 1.0), (-30.0, 0.0)} <= pairs and (N < 32 or {(30.0, 0.0), (-30.0, 1.0)} <= pairs), pairs
    return x, t


def _run_focal(case):
    _, (N, Cc), mode = case
    gamma = mode["gamma"]
    g = torch.Generator().manual_seed(1993 + 13 * N + Cc + int(10 * gamma))
    x, t = _focal_inputs(N, Cc, g)
    w = (torch.rand(Cc, generator=g) + 0.5) if mode["weight"] else None
    xr = x.double().requires_grad_(True)
    if Cc == 1:                                               # the binary head: BCEWithLogitsLoss on the label (gamma 0)
        assert gamma == 0.0 and w is None
        want = F.binary_cross_entropy_with_logits(xr, t.double())
    else:
        want = O.focal_loss_soft(xr, t.double(), 1.0, gamma, None if w is None else w.double())
    (GSCALE * GDEV * want).backward()
    X, T, DX, loss = _Out((N, Cc), x), _Out((N, Cc), t), _Out((N, Cc)), _Out((1,))
    W_ = None if w is None else _Out((Cc,), w)
    gdev = torch.tensor([GDEV], dtype=torch.float32, device=DEV)
    name = _launch(case, {"x": X, "target": T, "weight": W_, "loss": loss, "dx": DX, "gscale_dev": gdev})
    assert X.intact() and T.intact() and (W_ is None or W_.intact()) and gdev.item() == GDEV, "an input was written"
    got = loss.read("loss")[0].item()
    print(f"{_case_id(case)}: {name}: loss {got:.7f}, float64 {want.item():.7f}, error {abs(got - want.item()):.2e} (bound 1e-6)")
    _dx_close("dx", DX.read("dx"), xr.grad, 1e-7 * GSCALE * GDEV / 0.65)
    assert got == got and abs(got - want.item()) < 1e-6, (got, want.item())


def _run_softmax(case):
    _, (N, Cc), _ = case
    g = torch.Generator().manual_seed(7 + N)
    x = torch.randn(N, Cc, generator=g) * 3
    special = [torch.zeros(Cc) + 1.25, torch.tensor([80.0, -80.0, 0.0][:Cc]), torch.tensor([0.5, -float("inf"), 1.0][:Cc]), torch.tensor([-40.0, 40.0, 0.3][:Cc])]
    for i, s in enumerate(special):                           # the rows of tests/test_cls_only_cpu.py's cases, at both ends of the batch
        x[i], x[N - 1 - i] = s, s.flip(0)
    dp = torch.randn(N, Cc, generator=g)
    ((p64, dz64),), e_fwd, e_bwd = softmax_references([(x, dp)])
    X, DP, P, DZ = _Out((N, Cc), x), _Out((N, Cc), dp), _Out((N, Cc)), _Out((N, Cc))
    name = _launch(case, dict(x=X.data_ptr(), p=P.data_ptr(), dp=DP.data_ptr(), dz=DZ.data_ptr()))
    assert X.intact() and DP.intact(), "an input was written"
    p, dz = P.read("p"), DZ.read("dz")
    print(f"{_case_id(case)}: {name}: torch float32 against float64 {e_fwd:.3e} / {e_bwd:.3e}; device {(p.double() - p64).abs().max().item():.3e} / "
          f"{(dz.double() - dz64).abs().max().item():.3e}")
    assert 0 < e_fwd < 1e-6 and 0 < e_bwd < 1e-6
    assert within(p, p64, e_fwd), (p, p64)
    assert within(dz, dz64, e_bwd), (dz, dz64)


_RUN = {"dice": _run_dice, "focal": _run_focal, "softmax": _run_softmax}


@pytest.mark.parametrize("case", LOSS_CASES, ids=_case_id)
def test_loss_launches_match_float64(case):
    """One row of LOSS_CASES: the struct of the engine's filler, on real tensors, plans what its dummy-pointer twin (whose key the guard below
    counts) plans; the launches made are those; every output -- the per-head losses and their weighted total, dx of every head; the focal
    loss and dx; p and dz -- is within the module docstring's bounds of float64 autograd on the same float32 inputs; nothing is written
    outside an output, and no input changes."""
    _RUN[case[0]](case)


def test_every_row_makes_a_key_of_its_own_branch():
    """The rows reach the branches they are there for, by their keys' names: both block sizes, every shape of the statistics loop, both paths by
    both causes, the looping finalize and backward grid, both focal and softmax block regimes; all backward keys carry gscale_dev."""
    names = {}
    for case in LOSS_CASES:
        for op in _case_ops(case):
            names.setdefault((case[0],) + tuple(case[1]) + (("misaligned",) if case[2].get("misaligned") else ()), []).append(_loss_key(op))
    stats = lambda *k: names[("dice",) + k][0][0].split(" + ")[0]          # noqa: E731
    assert stats(4, 2, 1, 128, 128).endswith("[threads=1024 paths=vvvv rounds=1]")
    assert stats(4, 2, 1, 128, 256).endswith("[threads=1024 paths=vvvv rounds>1]") and stats(1, 1, 1, 512, 512).endswith("[threads=1024 paths=v rounds>1]")
    assert stats(2, 2, 1, 128, 160).endswith("[threads=1024 paths=vv rounds=1 rest]")
    assert stats(1, 1, 1, 120, 256).endswith("[threads=1024 paths=v rounds>1 rest part]")
    assert stats(2, 2, 1, 96, 96).endswith("[threads=256 paths=vv rounds>1 rest]")
    assert stats(2, 2, 1, 6, 5).endswith("[threads=256 paths=ss]") and stats(1, 2, 1, 16, 16, "misaligned").endswith("[threads=256 paths=s]")
    big = names["dice", 1, 257, 1, 128, 128]
    assert big[0][0].endswith("[planes>256]") and big[1][0].endswith("[paths=v loop]")
    assert all("loop" not in ks[1][0] and "planes>256" not in ks[0][0] for k, ks in names.items() if k[0] == "dice" and k[2] != 257)
    assert names["dice", 1, 2, 1, 16, 16, "misaligned"][1][0].endswith("[paths=s]") and "C>1" in names["dice", 1, 2, 3, 16, 16][0][1]
    for k, ks in names.items():
        if k[0] == "dice":
            assert all("gscale_dev" not in key[1] for key in ks[0::2]) and all("gscale_dev" in key[1] for key in ks[1::2]), (k, ks)
        if k[0] == "focal":
            assert "gscale_dev" in ks[0][1] and "dx" in ks[0][1] and (ks[0][0] == "focal_kernel [N>256]") == (k[1] > 256), (k, ks)
        if k[0] == "softmax":
            assert [key[1][0] for key in ks] == ["fwd", "bwd"] and all((key[0] == "softmax_rows_kernel [N>64]") == (k[1] > 64) for key in ks), (k, ks)


def test_step_programs_launch_only_reference_tested_loss_instances():
    """Surveys (builds, does not run) the benchmark's four step programs, and the first with 64 CUs reserved as under data parallelism, for the
    coverage key of every Dice, Focal, loss-mix and softmax op: each must be the key of a call that a row of LOSS_CASES makes (the mix: of
    the bit test that answers for it).  A plan change -- another block size or loop shape, a head that lost its alignment, another head
    count, class weights, a criterion kind -- that no float64 case reaches fails here; _loss_key (tests/step_programs.py) and LOSS_CASES
    are the places to edit.  Every program must hold the four loss ops."""
    assert_all_tested("loss", _reference_tested_loss_keys(), [survey(p) for p in STEP_PROGRAMS] + [survey(STEP_PROGRAMS[0], 64)],
                      required=(L.OP_DICE_FWD, L.OP_DICE_BWD, L.OP_FOCAL, L.OP_LOSS_MIX))
