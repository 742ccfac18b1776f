"""ConvT k = 2 backward, pair by pair: every OP_CONVT_WGRAD + OP_CONVT_DGRAD pair of the bench plan (U-Net++ MT, B = 32, 256 x 256) timed as two
program ranges (the two launches + split-K reductions) and as ONE range (the fused launch where convt2.hip takes the shape), interleaved in one
process, HIP events around the range.  usage: python tools/convt_pair_cost.py [bf16|f16]   (probes build: MTBC_CT_FUSE_ALL=1 fuses every eligible shape)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multi_task_breast_cancer_amd import _lib as L
from multi_task_breast_cancer_amd.experiment_init import init_multitask_model, init_optimizer
from multi_task_breast_cancer_amd.miscellany import seed_everything
from multi_task_breast_cancer_amd.synthetic import synthetic_batch
from multi_task_breast_cancer_amd.trainer import FusedTrainStep

B, S, DT = 32, 256, sys.argv[1] if len(sys.argv) > 1 else "bf16"
dev = torch.device("cuda:0")
seed_everything(1993)
model = init_multitask_model("MTUNetPlusPlus", 1, 1, 3, deep_supervision=True).to(dev)
model.set_compute(DT)
step = FusedTrainStep(model, init_optimizer(model, "Adam", 1e-4), alpha=0.5)
batch = synthetic_batch(B, S, S, 0, dev)
for _ in range(3):
    step(*batch)
torch.cuda.synchronize()
prog = step._st.programs["bwd"]

def t(first, count, reps=7):
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); prog.run(first, count); e.record(); e.synchronize(); ms.append(s.elapsed_time(e) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0]

tot = [0.0, 0.0]
print(f"{DT}: us, median (min) of 7, HIP events around the program range")
for i in range(prog.n - 1):
    if prog.array[i].kind == L.OP_CONVT_WGRAD and prog.array[i + 1].kind == L.OP_CONVT_DGRAD:
        a, d = prog.array[i].u.convT, prog.array[i + 1].u.convT
        rows = []
        for _ in range(2):             # interleaved: two launches, pair, two launches, pair
            w, dg, pr = t(i, 1), t(i + 1, 1), t(i, 2)
            rows.append((w, dg, pr))
        w = min(r[0][0] for r in rows); dg = min(r[1][0] for r in rows); pr = min(r[2][0] for r in rows)
        tot[0] += w + dg; tot[1] += pr
        print(f"  #{i:3d} {a.Cin:3d}->{a.Cout:3d} @{a.H}x{a.W} x16={a.x_type16} dy16={a.dy_type16} acc_dx={d.accumulate_dx} bias={int(bool(a.dbias))}: "
              f"wgrad {w:6.1f} + dgrad {dg:6.1f} = {w + dg:6.1f}   pair in one range {pr:6.1f}   "
              f"[rounds: {', '.join(f'{r[0][0]:.1f}+{r[1][0]:.1f} vs {r[2][0]:.1f}' for r in rows)}]", flush=True)
print(f"  sum: two launches {tot[0]:.1f} us, one range {tot[1]:.1f} us")
