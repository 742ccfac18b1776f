"""The benchmark's step programs, surveyed once per session for the launch-coverage guards of tests/test_ops_gpu.py
(test_step_programs_launch_only_reference_tested_*): build_step is the one copy of bench.py's constructor path, survey walks the programs of a
built step once and keeps plain values, the collectors and the key functions say per op family what "the same launch" means, and
assert_all_tested compares what a survey saw with what the reference cases make.  No test module: pytest does not collect it.

The launch module of a further model (tests/test_unetpp_seg_launches_gpu.py is the shortest) holds what is the model's alone:
  * PROGRAMS, a make_model(arch) for step_builder, and the case tables: one row per coverage key of the model's programs that no older table
    makes, in the formats of tests/test_ops_gpu.py's tables, with the key and the launch each row stands for in a comment behind it;
  * the thin parametrised wrappers that run the rows through tests/test_ops_gpu.py's own fp64 tests;
  * three calls: assert_only_tested(survey, reference_tested_keys(), table_keys(...)) per program, assert_rows_needed(...) once over the
    tables, assert_op_kinds_claimed(surveys) -- beside them whatever only this model can assert (an op kind that must or must not be there).
kernel_instances and assert_keys_subset serve a model that is a part of an older one and should launch nothing of its own."""
import collections
import functools
import gc
import re

import torch

from multi_task_breast_cancer_amd import ops

L = ops.L
DEV = "cuda:0"

# the benchmark's step programs (bench.py run_mode): (arch, dtype, N, size) of BASELINE.json configs[1], configs[4] (its per-GPU shape),
# configs[2], and the fp32 parity mode
STEP_PROGRAMS = [("MTUNetPlusPlus", "bf16", 32, 256), ("MTUNetPlusPlus", "f16", 16, 512), ("MTnnUNet", "bf16", 64, 256), ("MTUNetPlusPlus", "f32", 32, 256)]


PLAN = "conv3x3-wgrad-plan"
NAMED = ("conv3x3", PLAN, "InstanceNorm", "transposed-convolution", "small-op", "loss")      # the families whose keys carry a kernel-name string


def step_builder(make_model, **step_kwargs):
    """build(arch, dtype, N, size, reserve_cus=0) for survey: builds (does not run) one fused training step of make_model(arch), seeded
    1993, with Adam(1e-4) and step_kwargs: (the compiled step, what must stay referenced beside it)."""
    def build(arch, dtype, N, size, reserve_cus=0):
        from multi_task_breast_cancer_amd.experiment_init import init_optimizer
        from multi_task_breast_cancer_amd.miscellany import seed_everything
        from multi_task_breast_cancer_amd.trainer import FusedTrainStep
        seed_everything(1993)
        model = make_model(arch).to(DEV)
        model.set_compute(dtype)
        model.coop_reserve_cus = reserve_cus          # what a data-parallel FusedTrainStep sets (trainer.py)
        step = FusedTrainStep(model, init_optimizer(model, "Adam", 1e-4), **step_kwargs)
        return step._compiled(N, size, size), (step, model)
    return build


def multitask_model(arch, sequences=1, **kwargs):
    from multi_task_breast_cancer_amd.experiment_init import init_multitask_model
    return init_multitask_model(arch, sequences=sequences, regions=1, n_classes=3, deep_supervision=True, **kwargs)


build_step = step_builder(multitask_model, alpha=0.5, inversely_weighted=True)          # bench.py's constructor path


# ------------------------------------------------------------------ the key functions: the only places that decide what "the same launch" means
_CONV3_KC = 8          # conv3x3.hip:77, KC: input channels per LDS chunk of the fp32 kernels (the 16-bit kernels: LPKC = 32, conv3x3.hip:603)


def _conv3_key(a, op):
    """Coverage key of ONE mtbc_conv3x3_fwd / _dgrad / _wgrad call: the FULL string of mtbc_conv3x3_kernel_name -- the kernel instance and the
    reduction behind a weight gradient: " + splitk_reduce", " + splitk_fixup", " + channel_sums", or nothing (blocks store straight into dw) --
    + the branches the ARGUMENTS select inside those kernels.  The only place that decides what "the same launch" means for the guard below.
    A field the call does not read does not enter its key (line numbers: csrc/conv3x3.hip).  How a weight gradient walks its pixels -- what
    plan_wgrad decides from N and the map size -- is the business of _wgrad_plan_key, a family of its own."""
    L = ops.L
    name = ops.conv3x3_kernel_name(a, op)
    c8 = a.operand_layout == L.LAYOUT_C8
    segs = [a.in_[i] for i in range(a.n_in)]
    chunk = 32 if a.compute in (1, 2) else _CONV3_KC
    f = []
    if op == L.OP_CONV3_FWD:
        # rows = the channels written (Cout); the MFMA reduces over the segmented input (Cin)
        if a.bias:                            # (p.bias: the igemm epilogues 1136 and 1344, the stem and direct kernels; 4160: NULL with norm_z)
            f.append("bias")
        if a.stats_partial:                   # (1037 `p.stats`; 4130 the stem kernels; 4167: refused with planar operands and output)
            f.append("stats")
        if a.out_accumulate:                  # (4112: the output segment's accumulate; 4114: channel-blocked operands only)
            f.append("out_acc")
        if c8 and a.out_partial:              # (3814 p.extra, with norm_z only: 4160)
            f.append("out_partial")
        if c8 and a.norm_z:                   # (3814 p.nz; p.ngamma / p.nbeta: both or neither, 4160)
            f.append("norm_affine" if a.norm_gamma else "norm_plain")
        rows, red, every = a.Cout, a.Cin, chunk
    elif op == L.OP_CONV3_DGRAD:
        # rows = the channels written (the dx segments, Cin); the MFMA reduces over dout (Cout: one segment, no boundary inside)
        f.append("codes=" + ",".join(str(c) for c in sorted({s.accumulate for s in segs})))      # (4214-4223, make_segtable 4209)
        rows, red, every = a.Cin, a.Cout, 16      # (straddle: a boundary of the WRITTEN segments inside a 16-row tile -- one tile writes two segments)
    else:
        # rows = the output channels of dw (Cout), columns = the segmented input (Cin) in blocks of the chunk
        if a.dbias:                           # (4328 want_bias, 4345 BIAS, 4436 the bias row of the reduction, 4447 channel_sums; 4297: the stem refuses it)
            f.append("dbias")
        if a.accumulate_dw:                   # (4274 the reduction launch, 4331, 4339)
            f.append("acc_dw")
        rows, red, every = a.Cout, a.Cin, chunk
    if a.n_in > 1:
        f.append("segs>1")
    acc = 0
    for s in segs[:-1]:                       # fwd / wgrad: one chunk of the reduced / column channels reads two segments
        acc += s.channels
        if acc % every:
            f.append("straddle")
            break
    if rows % 16:
        f.append("ragged_rows")
    if red % chunk:
        f.append("ragged_k")
    if any(s.batch_stride != s.channels * a.H * a.W for s in segs):
        f.append("strided")
    if a.force_direct and not c8:             # (4115, 4169, 4224, plan_wgrad 3980 / 4022: the planar dispatch only)
        f.append("force_direct")
    return name, tuple(f)


_WG_TILE_WALKERS = ("conv3x3_wgrad_c8_kernel", "conv3x3_wgrad_mfma_kernel", "conv3x3_wgrad_lp_kernel", "conv3x3_wgrad_lp2_kernel")
_WG_BANDED = ("conv3x3_wgrad_stem_c8_kernel", "conv3x3_wgrad_stem_mc_c8_kernel", "conv3x3_wgrad_smallcin_kernel")


def _splitk_reduce_phases(nsplit, G):
    """Which of the three row loops of splitk_reduce_k<G, E> some split lane g runs (reduce.hip:25 eight rows in flight per round, :32 pairs,
    :33 the odd tail), walked as the kernel walks them."""
    ph = set()
    for g in range(G):
        k = g
        while k + 7 * G < nsplit:
            ph.add("x8")
            k += 8 * G
        while k + G < nsplit:
            ph.add("x2")
            k += 2 * G
        if k < nsplit:
            ph.add("x1")
    return [n for n in ("x8", "x2", "x1") if n in ph]


def _wgrad_plan_key(a):
    """Plan key of ONE mtbc_conv3x3_wgrad call: the FULL string of mtbc_conv3x3_kernel_name + the class of the plan mtbc_conv3x3_wgrad_plan
    reports -- what plan_wgrad decides from N and the map size, which neither the name nor _conv3_key carries.  The argument flags of
    _conv3_key are NOT repeated here: the two keys are not multiplied with each other.  The only place that turns plan numbers into classes
    (line numbers: csrc/conv3x3.hip unless reduce.hip is named); a kernel family it does not know raises.  Covered now: per kernel family how
    a block walks its share of the pixels (the tile loop's trip count, even or fixed dealing, ragged shares, shares that cross an image
    boundary; the wide-block kernel's row segments, block mapping and ring; the image-tile kernel's ranges; the bands of the stem and
    small-Cin kernels; the direct kernel's image stride) and the reduction behind it (the splitk_reduce_k instance with the row loops it
    runs; the in-kernel tree's depth and a ragged last group)."""
    name = ops.conv3x3_kernel_name(a, L.OP_CONV3_WGRAD)
    p = ops.conv3x3_wgrad_plan(a)
    fam = name.split(" + ")[0].split("<")[0]
    f = []
    if fam in _WG_TILE_WALKERS:
        T, S = p.total_tiles, p.nsplit
        if p.tiles_per_split < 0:             # (2225 / 2226: split s owns [s T / S, (s + 1) T / S); the fp32 and planar 16-bit kernels only deal fixed: 1535, 1755, 1903)
            share = [(s * T // S, (s + 1) * T // S) for s in range(S)]
        else:
            share = [(s * p.tiles_per_split, min(T, (s + 1) * p.tiles_per_split)) for s in range(S)]
        assert share[0][0] == 0 and share[-1][1] == T and all(b < e for b, e in share), (name, T, S, p.tiles_per_split)
        f.append("even" if p.tiles_per_split < 0 else "fixed")
        longest = max(e - b for b, e in share)            # (the tile loop 2283 / 1536 / 1756 / 1904: one trip, two, or a steady state between first and last)
        f.append(f"tiles={longest}" if longest < 3 else "tiles>=3")
        if len({e - b for b, e in share}) > 1:            # (a short last split: `min(p.total_tiles, ...)` 2226; T % S != 0 of the even deal)
            f.append("ragged")
        per_image = p.tiles_x * p.tiles_y                 # (2241-2243: tile -> (tx, ty, n); geo 2 of the planar kernels: a tile IS an image pair)
        if any(b // per_image != (e - 1) // per_image for b, e in share):
            f.append("crosses")
        if p.geo == 2 and fam != "conv3x3_wgrad_c8_kernel" and a.N % 2:      # (plan_wgrad 3988 tn = cdiv(N, 2): the last tile holds one image)
            f.append("odd_N")
    elif fam == "conv3x3_wgrad_c8w_kernel":
        f.append("segs=1" if p.segs == 1 else "segs>1")                       # (2463 / 2473: a block walks the whole strip, or rows [seg * seg_tiles, ...))
        if p.tiles_y % p.seg_tiles:                                           # (2473 nt = min(seg_tiles, tiles_y - ty0))
            f.append("short_last_seg")
        if a.N % 8 == 0:                                                      # (2460 the image-major block mapping; 2669 its partial rows)
            f.append("img8")
        f.append("steps>=ring" if 4 * p.seg_tiles + 2 > 6 + 4 * p.depth else "steps<ring")      # (2447 RING rows; 2521 / 2606 the slot wraps)
        if p.ciblocks > 1:                                                    # (2466 cib, 2549 the bias wave of block 0)
            f.append("ciblocks>1")
        if ((a.Cin + 15) // 16) % p.cit:                                      # (2467 ncit = min(cit, tiles - cit0): a shorter last input-channel block)
            f.append("ragged_cit")
    elif fam == "conv3x3_wgrad_c8i_kernel":
        f.append(f"images={p.seg_tiles}" if p.seg_tiles < 3 else "images>=3")      # (2805 / 2808: no prefetch, one, or both stages in turn)
        if a.N % p.seg_tiles:                                                 # (2734 n_end = min(N, ...))
            f.append("short_last_range")
        if p.ciblocks > 1:                                                    # (2732 cib)
            f.append("ciblocks>1")
    elif fam in _WG_BANDED:
        assert p.bands in (1, 4, 16), (name, p.bands)                         # (3184 / 3378 / 3480 band = b % S; plan_wgrad 3896, 4023)
        f.append(f"bands={p.bands}")
    elif fam == "conv3x3_wgrad_direct_kernel":
        if p.images_per_split > 1:                                            # (3452 `for (n = split; n < N; n += nsplit)`)
            f.append("images>1")
    else:
        raise AssertionError(f"_wgrad_plan_key does not know the kernel family of {name!r}")
    if p.reduce == L.WGRAD_REDUCE_LAUNCH:
        inst = p.reduce_kernel.decode()
        m = re.fullmatch(r"splitk_reduce<(\d+)(?:, (\d+))?>", inst)
        assert m, inst
        f.append(inst + " " + "+".join(_splitk_reduce_phases(p.nsplit, int(m.group(1)))))
    elif p.reduce == L.WGRAD_REDUCE_FIXUP:
        f.append(f"fixup levels={p.fix_levels}")                              # (2115 splitk_fix_plan; 2139 the walk up the tree)
        if p.nsplit % p.fix_fanin:
            f.append("fixup ragged_group")
    else:
        assert p.reduce == L.WGRAD_REDUCE_NONE and p.nsplit == 1, (name, p.reduce, p.nsplit)      # (4331: one split stores into dw)
        f.append("store")
    return name, tuple(f)


def _instnorm_key(a, backward):
    """Coverage key of ONE mtbc_instnorm_lrelu_fwd / _bwd call: the launches mtbc_instnorm_kernel_name plans (kernel instances, block sizes,
    team size T; the number of rounds only as 1 or >1) + the branches the ARGUMENTS select inside those kernels.  The only place that
    decides what "the same launch" means for the guard below."""
    name = re.sub(r"rounds=(\d+)", lambda m: "rounds=1" if m.group(1) == "1" else "rounds>1", ops.instnorm_kernel_name(a, backward))
    c8 = bool(a.dz8 if backward else a.y8)
    f = []
    if a.gamma and a.beta:
        f.append("affine")
    else:
        f += [n for n in ("gamma", "beta") if getattr(a, n)]
    if not backward:
        if a.y16:                             # (beside y8: the 16-bit planes of the streaming pass; without y8: norm.hip in_fwd_reg_kernel `if (p.y16)`, in_cvt4)
            f.append("y16")
        if c8:
            f += [n for n in ("pool_y8", "pool_arg") if getattr(a, n)]
            if a.y and not a.y16:             # (norm_coop.hip fill_coop: `if (p->y16) p->y = nullptr`)
                f.append("y")
        # without y8: `y` is the output itself when y16 is NULL, and no kernel of norm.hip reads pool_y8 / pool_arg (norm.hip fill() copies neither into InP)
        return name, tuple(f)
    if not a.dy:
        f.append("dy=NULL")
    if a.n_dy_extra:
        f.append(f"dy_extra={a.n_dy_extra}")
    if a.dy_rank1:
        f.append("rank1")
        if a.dy_rank1_dw:
            f.append("rank1_dw")
            f += ["rank1_acc"] if a.dy_rank1_accumulate else []       # (read by in_r1_finalize_kernel only)
            f += [] if a.dy_rank1_db else ["rank1_db=NULL"]
    if a.dy_pool:
        f.append("dy_pool")
    f += [n for n in ("dgamma", "dbeta", "dbias_pre") if getattr(a, n)]
    if a.accumulate_dparams and (a.dgamma or a.dbeta or a.dbias_pre) and not a.defer_dparams:
        f.append("acc")                       # (with defer_dparams the flag is read by the MTBC_OP_IN_DPARAM descriptor only: _dparam_key)
    if a.defer_dparams:
        f.append("defer")
    if a.dz16 and not a.dz8:                  # (norm.hip in_bwd_reg_kernel `if (p.dz16)`, in_cvt4; with dz8 norm_coop.hip fill_coop never copies a->dz16 into CoP)
        f.append("dz16")
    # dz in place over dy: only the fp32 kernels of norm.hip write `dz` (norm_coop.hip fill_coop never copies a->dz into CoP; with dz16
    # norm.hip in_bwd_reg_kernel stores through p.dz16 and never through d4)
    if a.dz and a.dz == a.dy and not a.dz8 and not a.dz16:
        f.append("inplace")
    return name, tuple(f)


def _dparam_key(d):
    """Coverage key of one descriptor of mtbc_instnorm_dparam_many (MTBC_OP_IN_DPARAM: the deferred parameter-gradient reduction)."""
    return "in_dparam_many_kernel", tuple([n for n in ("dgamma", "dbeta", "dbias_pre") if getattr(d, n)] + [f"T={d.T}"] + (["acc"] if d.accumulate else []))


def _convT_key(a, op, nxt=None):
    """Coverage key of ONE mtbc_convT_fwd / _dgrad / _wgrad call, or of a program's WGRAD + DGRAD pair (nxt = the DGRAD's arguments): the
    launches mtbc_convT_kernel_name plans + the branches the ARGUMENTS select inside those kernels -- bias / dbias, the accumulate flags,
    which tensors are channel-range views of wider buffers (a batch stride above dense), and Cout = 1 for the generic GEMM kernels (what the
    fused deep-supervision heads launch: a 4-, 16- or 64-row M with one output plane).  The only place that decides what "the same launch" means
    for the guard below."""
    L = ops.L
    name = ops.convT_kernel_name(a, op, nxt)
    plane, up = a.H * a.W, a.H * a.W * a.k * a.k
    dense = dict(x=a.Cin * plane, y=a.Cout * up, dy=a.Cout * up, dx=a.Cin * plane)
    f = []

    def views(s, *names):
        f.extend(f"{n}_strided" for n in names if getattr(s, n + "_batch_stride") != dense[n])

    if op == L.OP_CONVT_FWD:
        f += ["bias"] if a.bias else []
        views(a, "x", "y")
    elif op == L.OP_CONVT_DGRAD:
        f += ["acc_dx"] if a.accumulate_dx else []
        views(a, "dy", "dx")
    else:
        f += ["dbias"] if a.dbias else []
        f += ["acc_dw"] if a.accumulate_dw else []
        views(a, "x", "dy")
        if nxt is not None:
            f += ["acc_dx"] if nxt.accumulate_dx else []
            views(nxt, "dx")
    if re.search(r"\bconvT_(fwd|dgrad|wgrad)_kernel<", name) and a.Cout == 1:
        f.append("Cout=1")
    return name, tuple(f)


def _same_upconv(wg, dg):
    """The DGRAD behind a WGRAD belongs to the same up-convolution (engine.StepPlan.convT emits the two back to back)."""
    return all(getattr(wg, n) == getattr(dg, n) for n in ("N", "H", "W", "Cin", "Cout", "k", "dy", "w"))


def _small_op_key(op):
    """Coverage key of ONE small op (ops.SMALL_OPS): the launches mtbc_op_kernel_name plans + the branches the ARGUMENTS select inside those
    kernels -- which tensors are channel-range views of wider buffers (a batch stride above dense), argmax, bias / dbias, every accumulate
    flag, dx present, and Cout > 8 (a second channel group in the planar 1x1 kernels); for the nearest 2x up-sampling its strided tensors and
    acc_dx.  The only place that decides what "the same launch"
    means for the guard below."""
    L = ops.L
    name, k, f = ops.op_kernel_name(op), op.kind, []

    def views(a, dense, *names):
        f.extend(f"{n}_strided" for n in names if getattr(a, n + "_batch_stride") != dense[n])

    if k in (L.OP_POOL_FWD, L.OP_POOL_BWD):
        a = op.u.pool
        full = a.C * a.H * a.W
        dense = dict(x=full, y=full // 4, dy=full // 4, dx=full)
        if k == L.OP_POOL_FWD:
            views(a, dense, "x", "y")
            f += ["argmax"] if a.argmax else []
        else:
            views(a, dense, "x", "dy", "dx")
            f += ["acc_dx"] if a.accumulate_dx else []
    elif k in (L.OP_CONV1_FWD, L.OP_CONV1_DGRAD, L.OP_CONV1_WGRAD):
        a = op.u.conv1
        dense = dict(x=a.Cin * a.H * a.W, dx=a.Cin * a.H * a.W)
        if k == L.OP_CONV1_FWD:
            views(a, dense, "x")
            f += ["bias"] if a.bias else []
        elif k == L.OP_CONV1_DGRAD:
            views(a, dense, "dx")
            f += ["acc_dx"] if a.accumulate_dx else []
        else:
            views(a, dense, "x")
            f += ["dbias"] if a.dbias else []
            f += ["acc_dw"] if a.accumulate_dw else []
        f += ["Cout>8"] if a.Cout > 8 else []
    elif k == L.OP_LINEAR_FWD:
        f += [n for n in ("relu", "bias") if getattr(op.u.linear, n)]
    elif k == L.OP_LINEAR_BWD:
        a = op.u.linear
        f += [n for n in ("relu", "dx", "dbias") if getattr(a, n)]
        f += ["acc_dw"] if a.accumulate_dw else []
    elif k == L.OP_HEAD_COMBINE:
        f += [n for n in ("bT", "b1") if getattr(op.u.head, n)]
    elif k == L.OP_HEAD_EXPAND:
        f += [n for n in ("bT", "dbT", "db1", "acc_wT", "acc_bT", "acc_w1", "acc_b1") if getattr(op.u.head, n)]
    elif k in (L.OP_UPSAMPLE2_FWD, L.OP_UPSAMPLE2_BWD):
        # (pool_up.hip: the name carries the layout -- upsample2_c8_fwd_kernel moves 16-byte words and never looks at type16, and the backward
        # reads neither layout nor type16: dy / dx are fp32 planes always.  Batch strides in elements of the tensor: 16-bit ones for C8.)
        a = op.u.up2
        full = a.C * a.H * a.W
        dense = dict(x=full, y=4 * full, dy=4 * full, dx=full)
        if k == L.OP_UPSAMPLE2_FWD:
            views(a, dense, "x", "y")
        else:
            views(a, dense, "dy", "dx")
            f += ["acc_dx"] if a.accumulate_dx else []
    else:
        assert k in (L.OP_GAP_FWD, L.OP_GAP_BWD), k          # (GAP: dense tensors, no flag)
    return name, tuple(f)


def _loss_key(op):
    """Coverage key of ONE op of a step's loss program (ops.LOSS_OPS: Dice forward / backward, Focal, the loss mix, the classifier's softmax):
    the launches mtbc_op_kernel_name plans -- block size, per head the 16-byte or the scalar path, the shape of the statistics loop, a looping
    finalize / backward grid / focal block -- + the branches the ARGUMENTS select inside those kernels that the name does not carry.  A field
    the call does not read does not enter its key (head_loss.hip): the Dice forward reads neither gscale nor gscale_dev nor dx, focal_gamma
    is read by the FocalDICE kind only (its value is no branch), smooth_nr / smooth_dr and the head weights are values."""
    L = ops.L
    name, k, f = ops.op_kernel_name(op), op.kind, []
    if k in (L.OP_DICE_FWD, L.OP_DICE_BWD):
        a = op.u.dice
        f += [f"kind={a.kind}", f"n_heads={a.n_heads}"]
        if k == L.OP_DICE_BWD and a.gscale_dev:       # (dice_bwd_kernel: `p.gscale_dev ? *p.gscale_dev : 1.f`)
            f.append("gscale_dev")
        f += ["C>1"] if a.C > 1 else []               # (planes = N * C: a plane index is no image index)
    elif k == L.OP_FOCAL:
        a = op.u.focal                                # (focal_kernel: `p.C == 1`, `p.w ?`, `if (p.dx)`, `p.gscale_dev ?`, gamma == 0 / >= 1)
        f.append(f"C={a.C}")
        f += [n for n in ("weight", "dx") if getattr(a, n)]
        if a.dx and a.gscale_dev:                     # (read only where a gradient is written)
            f.append("gscale_dev")
        f.append("gamma=0" if a.gamma == 0.0 else "0<gamma<1" if a.gamma < 1.0 else "gamma>=1")
    elif k == L.OP_SOFTMAX:
        f += ["bwd" if op.u.softmax.backward else "fwd", f"C={op.u.softmax.C}"]
    else:
        assert k == L.OP_LOSS_MIX, k                  # (no branch on an argument)
    return name, tuple(f)


def _pack_key(kind, Cin, Cout, dgrad, compute, path):
    """Coverage key of one weight-image op from its arguments: what selects a kernel path (kind, format, single or batched) and the branches
    inside it (a ragged last row tile, a ragged last K chunk -- for the fp32 forward image of the batched launch: 16 x 16 patches that
    straddle two row tiles --, one / two / more chunks)."""
    L = ops.L
    if kind == L.OP_CONV3_PACK_LP:
        rows, red = (Cin, Cout) if dgrad else (Cout, Cin)
        return ("lp", int(bool(dgrad)), compute, rows % 16 != 0, red % 32 != 0, min(3, (red + 31) // 32), path)
    if kind == L.OP_CONV3_PACK_FWD:
        return ("fwd", 0, 0, Cout % 16 != 0, (9 * Cin) % 16 != 0, 0, path)
    assert kind == L.OP_CONV3_PACK_DGRAD, kind
    return ("dgrad", 1, 0, Cin % 16 != 0, False, 0, path)


def _wview_key(Cout, Cin, off, cnt, mode, k_off, K, path):
    return (mode, off > 0, off + cnt < Cin, bool(mode) and k_off > 0, bool(mode) and k_off + Cout < K, path)


def _c8_key(kind, N, Cc, HW, compute, stride):
    p16 = kind == ops.L.OP_C8_PACK16
    pieces = N * (Cc // 8) * (HW // 4 if p16 else HW)
    return ("pack16" if p16 else "pack", 0 if p16 else compute, stride != Cc * HW, pieces % 256 != 0)


# ------------------------------------------------------------------ the collectors: (a program's ops, an index) -> None, or
# (ops consumed, kind label, key, where); `where` is the shape or argument tuple a failure message names the op by
def _fields(s, *names):
    return tuple(getattr(s, n) for n in names)


def collect_conv3x3(prog, i):
    op = prog[i]
    if op.kind in (L.OP_CONV3_FWD, L.OP_CONV3_DGRAD, L.OP_CONV3_WGRAD):
        a = op.u.conv3          # where: (N, Cin, Cout, H, W, the segments' channels)
        return 1, op.kind, (op.kind, _conv3_key(a, op.kind)), _fields(a, "N", "Cin", "Cout", "H", "W") + (tuple(a.in_[i].channels for i in range(a.n_in)),)


def collect_wgrad_plan(prog, i):
    """Every OP_CONV3_WGRAD op, keyed by _wgrad_plan_key alone; where as collect_conv3x3's."""
    op = prog[i]
    if op.kind == L.OP_CONV3_WGRAD:
        a = op.u.conv3
        return 1, op.kind, (op.kind, _wgrad_plan_key(a)), _fields(a, "N", "Cin", "Cout", "H", "W") + (tuple(a.in_[i].channels for i in range(a.n_in)),)


def collect_instnorm(prog, i):
    op = prog[i]
    if op.kind in (L.OP_IN_FWD, L.OP_IN_BWD):
        return 1, op.kind, (op.kind, _instnorm_key(op.u.inorm, op.kind == L.OP_IN_BWD)), _fields(op.u.inorm, "N", "C", "H", "W")
    if op.kind == L.OP_IN_DPARAM:
        return 1, op.kind, (op.kind, _dparam_key(op.u.dparam)), _fields(op.u.dparam, "N", "C")


_CONVT_KINDS = {L.OP_CONVT_FWD: "fwd", L.OP_CONVT_DGRAD: "dgrad", L.OP_CONVT_WGRAD: "wgrad"}


def collect_convT(prog, i):
    """kind "pair" = an OP_CONVT_WGRAD with the OP_CONVT_DGRAD of the same problem right behind it in the same program, which is what the
    program runner looks at: one entry for both ops."""
    op = prog[i]
    if op.kind in _CONVT_KINDS:
        a = op.u.convT
        shape = _fields(a, "N", "Cin", "Cout", "H", "W", "k")
        nxt = prog[i + 1] if i + 1 < len(prog) else None
        if op.kind == L.OP_CONVT_WGRAD and nxt is not None and nxt.kind == L.OP_CONVT_DGRAD and _same_upconv(a, nxt.u.convT):
            return 2, "pair", ("pair", _convT_key(a, op.kind, nxt.u.convT)), shape
        return 1, _CONVT_KINDS[op.kind], (_CONVT_KINDS[op.kind], _convT_key(a, op.kind)), shape


_SMALL_SHAPE = {"pool": ("N", "C", "H", "W"), "conv1": ("N", "Cin", "Cout", "H", "W"), "gap": ("N", "C", "H", "W"), "linear": ("N", "In", "Out"),
                "head": ("Cin", "Cmid", "R", "k"), "up2": ("N", "C", "H", "W")}


def collect_small_op(prog, i):
    op = prog[i]
    if op.kind in ops.SMALL_OPS:
        field = L.OP_UNION_FIELD[op.kind]
        return 1, op.kind, (op.kind, _small_op_key(op)), _fields(getattr(op.u, field), *_SMALL_SHAPE[field])


_PACKS = (L.OP_CONV3_PACK_FWD, L.OP_CONV3_PACK_DGRAD, L.OP_CONV3_PACK_LP)


def collect_layout(prog, i):
    """The weight-image, weight-view and channel-blocking ops; where = (Cin, Cout, dgrad, compute) of an image, (Cout, Cin, off, cnt, mode,
    k_off, K) of a view, (N, C, HW, compute, src_batch_stride) of a channel-blocking op.  A pack or view op in a run of more than one inside
    its program goes through the batched launch (mtbc_program_run_ms): path "many"."""
    kind = prog[i].kind

    def in_run(family):          # an op of the same family stands next to op i
        return "many" if (i > 0 and prog[i - 1].kind in family) or (i + 1 < len(prog) and prog[i + 1].kind in family) else "single"

    if kind in _PACKS:
        args = Cin, Cout, dgrad, compute = _fields(prog[i].u.pack, "Cin", "Cout", "dgrad", "compute")
        return 1, kind, _pack_key(kind, Cin, Cout, dgrad, compute if kind == L.OP_CONV3_PACK_LP else 0, in_run(_PACKS)), args
    if kind == L.OP_CONV3_WVIEW:
        args = _fields(prog[i].u.wview, "Cout", "Cin", "ci_off", "ci_cnt", "mode", "k_off", "K")
        return 1, kind, _wview_key(*args, in_run((L.OP_CONV3_WVIEW,))), args
    if kind in (L.OP_C8_PACK, L.OP_C8_PACK16):
        args = _fields(prog[i].u.c8pack, "N", "C", "HW", "compute", "src_batch_stride")
        return 1, kind, _c8_key(kind, *args), args


_LOSS_SHAPE = {"dice": ("n_heads", "N", "C", "H", "W"), "focal": ("N", "C"), "softmax": ("N", "C"), "mix": ()}


def collect_loss(prog, i):
    """The ops of the loss program and the classifier's softmax pair; where = (n_heads, N, C, H, W) of a Dice op, (N, C) of a Focal or softmax
    op, () of the mix."""
    op = prog[i]
    if op.kind in ops.LOSS_OPS:
        field = L.OP_UNION_FIELD[op.kind]
        return 1, op.kind, (op.kind, _loss_key(op)), _fields(getattr(op.u, field), *_LOSS_SHAPE[field])


COLLECTORS = {"conv3x3": collect_conv3x3, "conv3x3-wgrad-plan": collect_wgrad_plan, "InstanceNorm": collect_instnorm, "transposed-convolution": collect_convT, "small-op": collect_small_op,
              "layout": collect_layout, "loss": collect_loss}

# program: (arch, dtype, N, size); kinds: {program name: [op kind]}; seen: {family: {key: (kind label, where) of the first op that has it}};
# launches: {family: {key: [where of every op that has it, in program order]}}
Survey = collections.namedtuple("Survey", "program reserve_cus kinds seen launches")
_SURVEYS = {}


def survey(program, reserve_cus=0, collectors=COLLECTORS, build=build_step):
    """The Survey of one step program, built (not run) once per session: the first call for a (program, reserve_cus) builds the step, hands
    the ops of each of its programs to every collector and keeps plain values only, so that the step and its model can go before the next
    one is built -- the four programs do not fit the device side by side.  Later calls get that result, whatever collectors and build they
    name: the guards all take the defaults; `build` is there for a test to hand in a program of its own."""
    if (program, reserve_cus) in _SURVEYS:
        return _SURVEYS[program, reserve_cus]
    st, keep = build(*program, reserve_cus)
    kinds, seen, p, prog = {}, {family: {} for family in collectors}, None, None
    launches = {family: {} for family in collectors}
    for name, p in st.programs.items():
        prog = [p.array[i] for i in range(getattr(p, "n", 0))]
        kinds[name] = [op.kind for op in prog]
        for family, collect in collectors.items():
            i = 0
            while i < len(prog):
                hit = collect(prog, i)
                if hit:
                    used, kind, key, where = hit
                    seen[family].setdefault(key, (kind, where))
                    launches[family].setdefault(key, []).append(where)
                i += used if hit else 1
    del st, keep, p, prog
    gc.collect()          # a step and its model refer to each other: their tensors go only with a collection
    torch.cuda.empty_cache()
    _SURVEYS[program, reserve_cus] = Survey(program, reserve_cus, kinds, seen, launches)
    return _SURVEYS[program, reserve_cus]


def assert_all_tested(family, tested, surveys, required=(), answers=None):
    """Every key the surveys saw of the family must be in `tested`, and every program must hold a launch of the family and of each kind label
    in `required`.  A missing key is named with its program, kind label and where.  answers: {key: the case table that makes it} -- the
    listing then names, per key, every launch of the program that has it and the table that answers for them."""
    missing, total = [], set()
    for s in surveys:
        seen, prog = s.seen[family], s.program + ((f"reserve {s.reserve_cus}",) if s.reserve_cus else ())
        print(f"{prog}: {len(seen)} keys")
        absent = set(required) - {kind for kind, _ in seen.values()}
        assert seen and not absent, f"{prog}: no {family} launch found" + (f" of kind {sorted(absent, key=repr)}" if absent else "")
        for key, (kind, where) in sorted(seen.items(), key=repr):
            if answers is None:
                print(f"  {kind} {key} at {where}")
            else:
                print(f"  {kind} {key}  <- {answers.get(key, 'MISSING')}")
                for w in s.launches[family][key]:
                    print(f"      at {w}")
            total.add(key)
            if key not in tested:
                missing.append(f"\n  {prog}: {kind} {key} at {where}")
    print(f"{len(total)} distinct keys in the {len(surveys)} programs, {len(tested)} keys tested")
    assert not missing, f"{family} launches of the step programs that no reference case makes:" + "".join(missing)


# ------------------------------------------------------------------ the guards of a further model's launch module (the header says how they go together)
@functools.lru_cache(maxsize=None)
def reference_tested_keys():
    """{family: the keys of the older tables -- tests/test_ops_gpu.py's, for the loss family tests/test_loss_launches_gpu.py's}, the sets the
    benchmark programs' guards hold those programs to.  A function of the case tables: computed once per session, not to be written to."""
    import test_loss_launches_gpu as LOSS
    import test_ops_gpu as OPS
    return {"conv3x3": OPS._reference_tested_conv3x3_keys(), PLAN: OPS._reference_tested_wgrad_plan_keys(), "InstanceNorm": OPS._reference_tested_instnorm_keys(),
            "transposed-convolution": OPS._reference_tested_convT_keys(), "small-op": OPS._reference_tested_small_op_keys(),
            "layout": OPS._reference_tested_layout_keys(), "loss": LOSS._reference_tested_loss_keys()}


def table_keys(conv3=(), wgrad_plan=(), inorm=(), convT=(), wview=()):
    """{family: {key: [row]}} of the calls the rows of a module's tables make, from dummy-pointer structs (nothing is launched).  The tables
    are in the formats of CONV3_STEP_CASES, WGRAD_PLAN_CASES, INORM_CASES and CONVT_CASES of tests/test_ops_gpu.py and of WVIEW_CASES of
    oracle/layout_reference.py; a view row goes through the single and through the batched launch."""
    import test_ops_gpu as OPS
    W_ = L.OP_CONV3_WGRAD
    own = {family: {} for family in COLLECTORS}
    for case in conv3:
        op, N, segs, Cout, H, W, mode = case
        own["conv3x3"].setdefault((op, _conv3_key(ops.conv3x3_case_args(op, N, segs, Cout, H, W, **mode), op)), []).append(case)
    for case in wgrad_plan:
        own[PLAN].setdefault((W_, _wgrad_plan_key(ops.conv3x3_case_args(W_, *case[:5], **case[5]))), []).append(case)
    for case in inorm:
        for op, _, key in OPS._inorm_case_calls(case):
            own["InstanceNorm"].setdefault((op, key), []).append(case)
    for case in convT:
        for kind, op, a, nxt in OPS._convT_case_calls(case):
            own["transposed-convolution"].setdefault((kind, _convT_key(a, op, nxt)), []).append(case)
    for case in wview:
        for path in ("single", "many"):
            own["layout"].setdefault(_wview_key(*case, path), []).append(case)
    return own


def assert_only_tested(survey, older, own, borrowed=None, borrowed_from=None):
    """Every coverage key of the surveyed program is the key of a call that a reference case makes: in older[family] (reference_tested_keys),
    in own[family] (table_keys of the model's rows) or in borrowed[family], the keys of the cases of the test file borrowed_from; and the
    program holds a launch of every family.  Prints per family the counts and every key with its first launch and what answers for it (the
    listings profiles/*_step_keys.txt record); a missing key is named with its family, kind label, key and where."""
    program, borrowed, missing = survey.program, borrowed or {}, []
    for family in COLLECTORS:
        seen, old, rows, lent = survey.seen[family], older[family], own[family], borrowed.get(family, ())
        assert seen, f"{program}: no {family} launch found"
        table = "tests/test_loss_launches_gpu.py" if family == "loss" else "tests/test_ops_gpu.py"
        print(f"{program} {family}: {len(seen)} keys, {sum(k in old for k in seen)} tested by {table}'s tables, "
              f"{sum((k in rows or k in lent) and k not in old for k in seen)} by the rows added for this model, "
              f"{sum(k not in old and k not in rows and k not in lent for k in seen)} missing")
        for key, (kind, where) in sorted(seen.items(), key=repr):
            by = table if key in old else f"row {rows[key][0]}" if key in rows else borrowed_from if key in lent else "MISSING"
            print(f"  {kind} {key} at {where}  <- {by}")
            if by == "MISSING":
                missing.append(f"\n  {family}: {kind} {key} at {where}")
    assert not missing, f"launches of {program} that no reference case makes:" + "".join(missing)


def assert_rows_needed(module, surveys, older, own, tables):
    """Every row of `tables` (the lists own = table_keys(...) was made from) makes a key that a surveyed program launches, that no older table
    makes and that no other row makes: no dead row, no double row, no row without a key and no empty table -- deleting a row fails
    assert_only_tested.  `module` names the tables in the message."""
    assert set(own) == set(COLLECTORS), sorted(set(own) ^ set(COLLECTORS))
    bad, made = [], 0
    for family, keys in own.items():
        launched = set().union(*(s.seen[family] for s in surveys))
        rows = {}
        for key, cases in keys.items():
            for case in cases:
                rows.setdefault(repr(case), []).append(key)
            if len(cases) > 1:
                bad.append(f"\n  {family}: {len(cases)} rows make {key}: {cases}")
        for row, ks in rows.items():
            if not any(k in launched and k not in older[family] for k in ks):
                why = "; ".join(f"{'no program launches' if k not in launched else 'an older table already makes'} {k}" for k in ks)
                bad.append(f"\n  {family}: {why} of row {row}")
        print(f"{family}: {len(rows)} rows, {len(keys)} keys")
        made += len(rows)
    with_key = {repr(case) for keys in own.values() for cases in keys.values() for case in cases}
    bad += [f"\n  table {i + 1} of {len(tables)} is empty" for i, table in enumerate(tables) if not table]
    bad += [f"\n  no key is made by row {case}" for table in tables for case in table if repr(case) not in with_key]
    if sum(len(table) for table in tables) != made:
        bad.append(f"\n  {sum(len(table) for table in tables)} rows in the tables, {made} distinct rows that make a key")
    assert not bad, f"rows of {module} that are not needed:" + "".join(bad)


def kernel_instances(survey):
    """The set of kernel instances a surveyed step's programs launch, from the strings of mtbc_conv3x3_kernel_name / _instnorm_ / _convT_ /
    _op_kernel_name that the keys of the NAMED families keep: launches are joined by " + ", and what stands in brackets behind an instance
    is what the arguments select inside it (common.h, OpChoice), not part of the instance."""
    out = set()
    for family in NAMED:
        for key in survey.seen[family]:
            out |= {re.sub(r"\s*\[[^\]]*\]", "", part).strip() for part in key[1][0].split(" + ")}
    return out


def assert_keys_subset(survey, of, families=COLLECTORS):
    """The surveyed program launches something of every family of `families`, and no coverage key of those that the program of the survey
    `of` does not launch; an extra key is named with its family, kind label, key and where."""
    extra = []
    for family in families:
        seen = survey.seen[family]
        assert seen, f"{survey.program}: no {family} launch found"
        print(f"{survey.program} {family}: {len(seen)} keys, {len(of.seen[family])} in {of.program}")
        for key, (kind, where) in sorted(seen.items(), key=repr):
            if key not in of.seen[family]:
                extra.append(f"\n  {family}: {kind} {key} at {where}")
    assert not extra, f"launches of {survey.program} that {of.program} does not make:" + "".join(extra)


def assert_op_kinds_claimed(surveys, claimed_also=(), required=()):
    """The op kinds of each surveyed program are among those tests/test_ops_gpu.py's OP_KIND_COVERED_BY claims or the names in claimed_also
    (kinds the calling module's own guard answers for), and each program holds every op kind of `required`."""
    import test_ops_gpu as OPS
    name_of = {getattr(L, n): n for n in dir(L) if n.startswith("OP_") and isinstance(getattr(L, n), int)}
    claimed = set(OPS.OP_KIND_COVERED_BY) | set(claimed_also)
    for s in surveys:
        kinds = {kind for oplist in s.kinds.values() for kind in oplist}
        print(f"{s.program}: {sorted(name_of.get(k, str(k)) for k in kinds)}")
        absent = sorted(name_of.get(k, str(k)) for k in set(required) - kinds)
        assert not absent, f"{s.program}: no op of kind {absent}"
        unclaimed = sorted(name_of.get(k, str(k)) for k in kinds if name_of.get(k) not in claimed)
        assert not unclaimed, f"op kinds of {s.program} that no test answers for: {unclaimed}"
