"""CLAHE / SOBEL as stored planes on the GPU: mtbc_batch_assemble_planes word for word against a torch restatement that goes through the
existing augmentation kernel (ONE coordinate function), E = 0 against mtbc_batch_assemble, a dataset with all six `data.augmentation` flags
feeding the fused train / eval / test steps and the epoch drivers, the 7-channel first cell in fp32, bf16 and fp16 against the oracle and
its 16-bit emulation, the programs of a 5-channel model against the listing recorded before this feature, and the launches of the 7-channel
step programs each tied to an element-wise fp64 case."""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path[:0] = [p for p in (os.path.dirname(os.path.abspath(__file__)),) if p not in sys.path]

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import augment as AUG  # noqa: E402
from multi_task_breast_cancer_amd import criterions as CR  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd import inference as I  # noqa: E402
from multi_task_breast_cancer_amd import ops  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.experiment_init import init_criterion_segmentation  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet, MTUNetPlusPlus  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from multi_task_breast_cancer_amd.trainer import (FusedEvalStep, FusedTrainStep, test_one_epoch_indexed, train_one_epoch,  # noqa: E402
                                                  validate_one_epoch, validate_one_epoch_indexed)
from oracle import torch_oracle as O  # noqa: E402
import step_programs as SP  # noqa: E402

test_one_epoch_indexed.__test__ = False          # a driver of the package, not a test of this module

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_programs_5ch.json")
ALL6 = {k: True for k in DD.SPATIAL_KEYS + DD.LUT_KEYS}
LUTS_BY_K = {0: [], 1: ["contrast_high"], 4: list(DD.LUT_KEYS)}
PLANES_BY_E = {1: ["SOBEL"], 2: ["CLAHE", "SOBEL"]}
INDEX = [4, 0, 0, 2, 3, 1, 4, 2, 1, 3, 0, 4]                   # 12 samples: more than one block at both plane sizes
PARAMS = {
    "none": None,
    "flips": ([0.0] * 12, [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0]),
    "90": ([90.0, -90.0, 180.0, 90.0, 270.0, -180.0, 90.0, -90.0, 0.0, 90.0, 180.0, -270.0], [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0]),
    "37": ([37.0, -37.0, 37.5, -123.4, 359.0, 12.0, -300.25, 37.0, 143.0, -37.0, 217.0, 37.0], [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0]),
}


def _params(name):
    return None if PARAMS[name] is None else AUG.params_from(*PARAMS[name])


def _store(M, H, W, seed):
    """uint8 image / mask stores, int64 labels and two more uint8 planes per image (what a caller's CLAHE and Sobel passes leave: any bytes)."""
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    planes = {k: torch.randint(0, 256, (M, H, W), generator=g, dtype=torch.uint8) for k in DD.SPATIAL_KEYS}
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long(), planes


def _restate(images, masks, planes, luts, index, params):
    """cat([mask, image] + extras) of the reference's __getitem__ for rows `index` as fp32 -- the stored planes, then lut[image] -- and ONE joint
    transform through the existing augmentation kernel; plain indexing without parameters.  -> (image stack, mask) on the device."""
    idx = torch.as_tensor(index, dtype=torch.long)
    im = images[idx]
    stack = torch.stack([masks[idx].float(), im.float()] + [p[idx].float() for p in planes]
                        + [torch.from_numpy(l.astype(np.float32))[im.long()] for l in luts], dim=1).to(DEV)
    if params is not None:
        stack = AUG.flip_rotate(stack, params)
    return stack[:, 1:].contiguous(), stack[:, :1].contiguous()


def _target(labels, index, n_onehot):
    lab = labels[torch.as_tensor(index, dtype=torch.long)]
    return F.one_hot(lab, 3).float() if n_onehot else lab.float().view(-1, 1)


def _outputs(N, C_img, H, W, n_onehot, misaligned):
    """(image, mask, target) filled with a sentinel; misaligned: the image is a view 4 bytes off a 16-byte boundary."""
    if misaligned:
        flat = torch.full((N * C_img * H * W + 4,), -7.0, device=DEV)
        assert flat.data_ptr() % 16 == 0
        image = flat[1:1 + N * C_img * H * W].view(N, C_img, H, W)
        assert image.data_ptr() % 16 == 4 and image.is_contiguous()
    else:
        image = torch.full((N, C_img, H, W), -7.0, device=DEV)
    return image, torch.full((N, 1, H, W), -7.0, device=DEV), torch.full((N, n_onehot or 1), -7.0, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. the launch, word for word
# (H, W, misaligned): the vector instance; the scalar instance with a ragged last 4-pixel group (90 % 4 = 2); a vector-shaped call whose
# image output is 4 bytes off 16-byte alignment, which takes the scalar instance
SHAPES = [(12, 20, False), (9, 10, False), (12, 20, True)]


@pytest.mark.parametrize("H,W,misaligned", SHAPES, ids=["vector", "scalar-ragged", "misaligned"])
@pytest.mark.parametrize("K", [0, 1, 4])
@pytest.mark.parametrize("E", [1, 2])
def test_assembly_is_bit_equal_to_the_restatement(E, K, H, W, misaligned):
    images, masks, labels, planes = _store(5, H, W, seed=5 + E + K)
    aug = {k: True for k in PLANES_BY_E[E] + LUTS_BY_K[K]}
    ds = DD.DeviceDataset(images, masks, labels, augmentation=aug, spatial_planes={k: planes[k] for k in PLANES_BY_E[E]})
    luts = DD.intensity_luts({k: True for k in LUTS_BY_K[K]})
    assert (ds.n_planes, ds.n_luts, ds.n_augments) == (E, K, E + K) and ds.channels == DD.channel_names(aug)
    assert tuple(ds.planes.shape) == (E, 5, H, W)
    before = [t.clone() for t in (ds.images, ds.masks, ds.labels, ds.planes, ds.luts)]
    N = len(INDEX)
    for pname in PARAMS:
        params = _params(pname)
        want_image, want_mask = _restate(images, masks, [planes[k] for k in PLANES_BY_E[E]], luts, INDEX, params)
        assert want_image.shape == (N, 1 + E + K, H, W)
        for n_onehot in (0, 3):
            out = _outputs(N, 1 + E + K, H, W, n_onehot, misaligned)
            got = ds.assemble(INDEX, None if params is None else params.to(DEV), n_onehot=n_onehot, out=out)
            assert all(g is o for g, o in zip(got, out))
            what = (pname, n_onehot)
            assert torch.equal(out[0], want_image), what
            assert torch.equal(out[1], want_mask), what
            assert torch.equal(out[2].cpu(), _target(labels, INDEX, n_onehot)), what
        if pname == "37":        # zero fill outside the rotated frame on the stored planes too: the corner of the first sample
            assert out[0][0, :, 0, 0].abs().max().item() == 0.0
    for t, b in zip((ds.images, ds.masks, ds.labels, ds.planes, ds.luts), before):
        assert torch.equal(t, b)
    with pytest.raises(ValueError):          # `out` is checked against 1 + E + K channels
        ds.assemble(INDEX, None, out=_outputs(N, 1 + K, H, W, 3, False))


def _raw_call(ds, index, params, n_onehot, out, planes_entry, E=None, K=None):
    """mtbc_batch_assemble_planes (or, planes_entry False, mtbc_batch_assemble) on a dataset's stores with a device index that nothing validated."""
    a = L.BatchPlanesArgs() if planes_entry else L.BatchArgs()
    a.M, a.N, a.H, a.W, a.n_onehot = ds.M, int(index.numel()), ds.H, ds.W, n_onehot
    a.K = ds.n_luts if K is None else K
    a.images, a.masks, a.labels, a.index = ds.images.data_ptr(), ds.masks.data_ptr(), ds.labels.data_ptr(), index.data_ptr()
    a.params = params.data_ptr() if params is not None else None
    a.luts = ds.luts.data_ptr() if a.K else None
    a.out_image, a.out_mask, a.out_target = (t.data_ptr() for t in out)
    lib, stream = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if planes_entry:
        a.E = ds.n_planes if E is None else E
        a.planes = ds.planes.data_ptr() if a.E else None
        L.check(lib.mtbc_batch_assemble_planes(C.byref(a), stream), "batch_assemble_planes")
    else:
        L.check(lib.mtbc_batch_assemble(C.byref(a), stream), "batch_assemble")
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(12, 20), (9, 10)], ids=["vector", "scalar-ragged"])
@pytest.mark.parametrize("pname", ["none", "37"])
def test_an_index_outside_the_store_writes_zeros(H, W, pname):
    images, masks, labels, planes = _store(5, H, W, seed=11)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=ALL6, spatial_planes=planes)
    raw_index = [4, 5, 0, -1, 2, 2 ** 31 - 1, 3, -2 ** 31, 1, 0, 4, 2]       # M, -1, INT_MAX, INT_MIN among valid rows
    bad = [n for n, i in enumerate(raw_index) if not 0 <= i < 5]
    valid = [i if 0 <= i < 5 else 0 for i in raw_index]
    params = _params(pname)
    want_image, want_mask = _restate(images, masks, [planes[k] for k in DD.SPATIAL_KEYS], DD.intensity_luts({k: True for k in DD.LUT_KEYS}), valid, params)
    want_image[bad], want_mask[bad] = 0.0, 0.0
    index = torch.tensor(raw_index, dtype=torch.int32, device=DEV)
    before = [t.clone() for t in (ds.images, ds.masks, ds.labels, ds.planes, ds.luts)]
    for n_onehot in (0, 3):
        want_target = _target(labels, valid, n_onehot)
        want_target[bad] = 0.0
        out = _outputs(len(raw_index), 7, H, W, n_onehot, False)
        _raw_call(ds, index, None if params is None else params.to(DEV), n_onehot, out, True)
        assert torch.equal(out[0], want_image) and torch.equal(out[1], want_mask) and torch.equal(out[2].cpu(), want_target), n_onehot
    for t, b in zip((ds.images, ds.masks, ds.labels, ds.planes, ds.luts), before):
        assert torch.equal(t, b)


# ------------------------------------------------------------------------------------------------ 2. E == 0 is mtbc_batch_assemble
@pytest.mark.parametrize("H,W,misaligned", SHAPES, ids=["vector", "scalar-ragged", "misaligned"])
@pytest.mark.parametrize("K", [0, 1, 4])
def test_no_planes_is_bit_equal_to_batch_assemble(K, H, W, misaligned):
    images, masks, labels, _ = _store(5, H, W, seed=17 + K)
    ds = DD.DeviceDataset(images, masks, labels, augmentation={k: True for k in LUTS_BY_K[K]})
    assert ds.planes is None and ds.n_planes == 0 and ds.n_augments == K
    index = torch.tensor([4, 0, 7, 2, 3, 1, 4, -3, 1, 3, 0, 4], dtype=torch.int32, device=DEV)       # two rows outside the store
    for pname in PARAMS:
        params = _params(pname)
        params = None if params is None else params.to(DEV)
        for n_onehot in (0, 3):
            old, new = (_outputs(12, 1 + K, H, W, n_onehot, misaligned) for _ in range(2))
            _raw_call(ds, index, params, n_onehot, old, False)
            _raw_call(ds, index, params, n_onehot, new, True)
            for o, n_ in zip(old, new):
                assert torch.equal(o.view(torch.int32), n_.view(torch.int32)), (pname, n_onehot)
            assert not bool((new[0] == -7.0).any()) and not bool((new[1] == -7.0).any()) and not bool((new[2] == -7.0).any())


# ------------------------------------------------------------------------------------------------ 3. the dataset with E = 2, K = 4 at 2 x 64 x 64
def _dataset7(M=6, seed=8):
    images, masks, labels, planes = _store(M, 64, 64, seed=seed)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=ALL6, spatial_planes=planes)
    assert ds.n_augments == 6 and ds.channels == ("image",) + DD.SPATIAL_KEYS + DD.LUT_KEYS
    return ds, labels


def _model7(seed, arch="MTnnUNet"):
    seed_everything(seed)
    m = MTnnUNet(7, 1, 3) if arch == "MTnnUNet" else MTUNetPlusPlus(in_channels=7, out_channels=1, n_classes=3, deep_supervision=True)
    return m.to(DEV)


def _label_column(labels, index):
    return labels[torch.as_tensor(index, dtype=torch.long)].float().view(-1, 1).to(DEV)


def test_load_indexed_step_equals_the_tensor_fed_step():
    ds, labels = _dataset7()
    (ma, sa), (mb, sb) = [(m, FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5)) for m in (_model7(21), _model7(21))]
    assert ma.in_channels == 7 and all(torch.equal(pa, pb) for pa, pb in zip(ma.parameters(), mb.parameters()))
    for s, index in enumerate(([5, 0], [3, 4])):
        params = AUG.params_from([37.5, -123.4] if s == 0 else [180.0, 12.0], [1, 0], [0, 1]).to(DEV)
        image, mask, _ = ds.assemble(index, params)
        sta = sa.load_indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV), params)
        assert sta.plan.cells[0].cin == 7
        la = sa.run(sta)
        lb = sb.run(sb.load_batch(image, mask, _label_column(labels, index)))
        assert torch.equal(la, lb), (s, la.tolist(), lb.tolist())
        assert torch.equal(ma.flat_g, mb.flat_g), s
    assert torch.equal(ma.flat_p, mb.flat_p)
    sa.check_nan()
    with pytest.raises(ValueError):          # a 5-channel dataset into the 7-channel model
        sa.load_indexed(DD.DeviceDataset(ds.images, ds.masks, ds.labels, augmentation={k: True for k in DD.LUT_KEYS}),
                        torch.tensor([0, 1], dtype=torch.int32, device=DEV), None)


def _same_rows(a, b):
    """Lists of CSV rows, equal value for value (an undefined metric is NaN in both)."""
    same = lambda x, y: x == y or (isinstance(x, float) and isinstance(y, float) and x != x and y != y)      # noqa: E731
    return len(a) == len(b) and all(ra.keys() == rb.keys() and all(same(ra[k], rb[k]) for k in ra) for ra, rb in zip(a, b))


def test_eval_and_test_steps_indexed_equal_the_tensor_fed_calls():
    ds, labels = _dataset7()
    model = _model7(24)
    batches = ([5, 0], [3, 4], [1, 2])
    ev_a, ev_b = FusedEvalStep(model, alpha=0.5), FusedEvalStep(model, alpha=0.5)
    te_a, te_b = I.FusedTestStep(model), I.FusedTestStep(model)
    for index in batches:
        image, mask, _ = ds.assemble(index, None)
        ev_a.indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV))
        ev_b(image, mask, _label_column(labels, index))
        te_a.indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV), patient_id=[f"p{i}" for i in index])
        te_b(image, mask, _label_column(labels, index), patient_id=[f"p{i}" for i in index])
    ra, rb = ev_a.result(), ev_b.result()
    assert len(ra) == 6 and ra == rb, (ra, rb)
    (seg_a, cls_a), (seg_b, cls_b) = te_a.result(), te_b.result()
    assert len(seg_a) == 6 and _same_rows(seg_a, seg_b) and _same_rows(cls_a, cls_b)
    assert [r["patient_id"] for r in seg_a] == [f"p{i}" for index in batches for i in index]
    assert [r["ground_truth"] for r in cls_a] == [int(labels[i]) for index in batches for i in index]
    assert np.array_equal(te_a.table, te_b.table)


def test_epoch_drivers_take_the_seven_channel_dataset():
    """EpochTables and the drivers need nothing but n_augments: an indexed training epoch equals the hand-written loop on the assembled tensors, the
    indexed validation epoch equals the tensor-fed one, and test_one_epoch_indexed drives the multi-task testing phase."""
    ds, labels = _dataset7()
    ei = EpochIndex(np.arange(6), 2, seed=13, drop_last=False)
    tf = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}
    (ma, sa), (mb, sb) = [(m, FusedTrainStep(m, FusedAdam(m, lr=1e-4, eps=1e-4), alpha=0.5)) for m in (_model7(22), _model7(22))]
    tables = DD.EpochTables(ei, 0, tf)
    got = train_one_epoch(sa, ds, tables, lr=1e-4)
    acc = torch.zeros(3, dtype=torch.float64)
    for b in range(len(tables)):
        index, params, n, _ = tables.batch(b)
        image, mask, _ = ds.assemble(index, params)
        acc += sb.run(sb.load_batch(image, mask, _label_column(labels, index.cpu())))[:3].double().cpu()
    for g, w in zip(got, (acc / len(tables)).tolist()):
        assert abs(g - w) <= 1e-12 * abs(w), (got, acc)
    assert torch.equal(ma.flat_p, mb.flat_p)
    plain = DD.EpochTables(ei, 0)
    step = FusedEvalStep(ma, alpha=0.5)
    got = validate_one_epoch_indexed(step, ds, plain)
    loader = []
    for b in range(len(plain)):
        index = plain.batch(b)[0]
        image, mask, _ = ds.assemble(index, None)
        loader.append({"image": image, "mask": mask, "label": _label_column(labels, index.cpu())})
    assert got == validate_one_epoch(step, loader, DEV)
    test = I.FusedTestStep(ma)
    seg_rows, cls_rows = test_one_epoch_indexed(test, ds, plain)
    want = I.FusedTestStep(ma)
    for data in loader:
        want(data["image"], data["mask"], data["label"])
    want_seg, want_cls = want.result()
    assert len(seg_rows) == 6 and _same_rows(seg_rows, want_seg) and _same_rows(cls_rows, want_cls) and np.array_equal(test.table, want.table)
    with pytest.raises(ValueError):          # the channel check of the drivers: a 1-channel model on this dataset
        seed_everything(1)
        test_one_epoch_indexed(I.FusedTestStep(MTnnUNet(1, 1, 3).to(DEV)), ds, plain)


# ------------------------------------------------------------------------------------------------ 4. the 7-channel first cell
def _batch7(N, size, seed):
    """The image and six more channels as data.augmentation stacks them: two spatial planes (other bytes) and the four intensity variants."""
    img, mask, label = O.synthetic_batch(N, size, size, seed=seed)
    g = torch.Generator().manual_seed(5000 + seed)
    u8 = img.round().clamp(0, 255)
    extra = [torch.randint(0, 256, img.shape, generator=g).float() for _ in range(2)]
    luts = [torch.from_numpy(l.astype(np.float32))[u8.long()] for l in DD.intensity_luts({k: True for k in DD.LUT_KEYS})]
    return torch.cat([u8] + extra + luts, 1).contiguous(), mask, label


def _first_cell_launches(st):
    cell = st.plan.cells[0]
    fwd = next(op for op in st.programs["fwd"].array if op.kind == L.OP_CONV3_FWD and op.tag == cell.tag)
    bwd = st.programs["bwd"]
    wg = next(bwd.array[i] for i in range(bwd.n) if bwd.array[i].kind == L.OP_CONV3_WGRAD and bwd.array[i].tag == cell.tag)
    return cell, ops.conv3x3_kernel_name(fwd.u.conv3, L.OP_CONV3_FWD), ops.conv3x3_kernel_name(wg.u.conv3, L.OP_CONV3_WGRAD)


@pytest.mark.parametrize("arch", ["MTnnUNet", "MTUNetPlusPlus"])
def test_fp32_seven_channel_step_matches_the_oracle(arch):
    """Loss words, class logits and every segmentation head of one fused step within 1e-4 of oracle/torch_oracle (the project's parity bound); the
    first layer's weight gradient against the drop-in module's autograd on the same batch: every element within 1e-4 of the largest.  (The
    distance to the oracle's fp32 gradient is printed, not bounded: the inputs are 0 .. 255 and the dz of a cell with an InstanceNorm behind it
    sums to zero over a plane, so each element is a small difference of large fp32 sums in either implementation.)"""
    seed_everything(25)
    prod = MTnnUNet(7, 1, 3) if arch == "MTnnUNet" else MTUNetPlusPlus(in_channels=7, out_channels=1, n_classes=3, deep_supervision=True)
    ref = O.build_oracle_model(arch, 7, 1, 3, True)
    ref.load_state_dict(prod.state_dict())
    prod = prod.to(DEV)
    twin = copy.deepcopy(prod)
    x, mask, label = _batch7(2, 64, 12)
    alpha = 0.35
    step = FusedTrainStep(prod, FusedAdam(prod, lr=1e-4, eps=1e-4), alpha=alpha, inversely_weighted=True)
    st = step.load_batch(x.to(DEV), mask.to(DEV), label.to(DEV))
    cell, fwd, wg = _first_cell_launches(st)
    assert cell.cin == 7 and not cell.stem16 and not cell.z16
    assert (fwd, wg) == ("conv3x3_direct_kernel", "conv3x3_wgrad_direct_kernel + splitk_reduce")
    losses = step.run(st).cpu().tolist()
    step.check_nan()
    total, seg, cls, logits, outs = O.train_step(ref, O.make_adam(ref, 1e-4), x, mask, label, alpha, True, 3)
    print("fused", losses[:3], "oracle", [total.item(), seg.item(), cls.item()])
    for g, w in zip(losses[:3], (total, seg, cls)):
        assert abs(g - w.item()) < 1e-4, (losses, total.item(), seg.item(), cls.item())
    assert losses[3] == 0.0
    err = (st.logits.data.view(2, -1).cpu() - logits[0].detach()).abs().max().item()
    print("class logits: max err", err)
    assert err < 1e-4
    assert len(st.segs) == len(outs)
    for i, (got, want) in enumerate(zip(st.segs, outs)):
        err = (got.data.cpu() - want.detach()).abs().max().item()
        print("head", i, "max err", err)
        assert err < 1e-4, i
    # the first layer's weight gradient: fused step, drop-in autograd surface, oracle
    g_fused = prod._grad_view(cell.wname).detach().cpu().clone()
    twin.zero_grad(set_to_none=True)
    tl, to = twin(x.to(DEV))
    onehot = F.one_hot(label.flatten().long(), 3).float().to(DEV)
    dseg, dcls = CR.apply_criterion_multitask_segmentation_classification(init_criterion_segmentation("DICE"), mask.to(DEV), to,
                                                                          CR.FocalLoss(alpha=1, gamma=2), onehot, tl, True)
    (alpha * dseg + (1 - alpha) * dcls).backward()
    g_dropin = dict(twin.named_parameters())[cell.wname].grad.detach().cpu()
    g_oracle = dict(ref.named_parameters())[cell.wname].grad.detach()
    assert g_fused.shape == g_oracle.shape == (g_oracle.shape[0], 7, 3, 3)
    scale = g_oracle.abs().max().item()
    err = (g_fused - g_dropin).abs().max().item()
    print("first-layer weight gradient: max |dw|", scale, "max err vs drop-in", err, "vs the oracle's fp32 gradient", (g_fused - g_oracle).abs().max().item())
    assert err <= 1e-4 * scale, (err, scale)


@pytest.mark.parametrize("arch,dtype,size,N", [("MTnnUNet", "bf16", 64, 4), ("MTUNetPlusPlus", "f16", 64, 4)])
def test_16bit_seven_channel_model_against_the_emulation(arch, dtype, size, N):
    """tests/test_stem_multichannel_gpu.py::test_whole_model_against_the_emulation's comparison and bounds with 7 input channels, on the arm that
    model takes under MTBC_NO_STEM_MC (direct kernel, fp32 conv output, one-plane InstanceNorm -- the oracle's own treatment of a first conv that
    is no multiple of 8 channels wide): from weights that 40 fp32-mode steps have moved, against the fp64-accumulating emulation, allowed 3 x the
    distance of the fp32-accumulating one (floors 5e-4 loss, 2e-3 outputs, 5e-2 per parameter gradient), no tensor exempt."""
    seed_everything(1993)
    prod = MTnnUNet(7, 1, 3) if arch == "MTnnUNet" else MTUNetPlusPlus(in_channels=7, out_channels=1, n_classes=3, deep_supervision=True)
    O.seed_everything(1993)
    ref = O.build_oracle_model(arch, 7, 1, 3, True)
    ref.load_state_dict(prod.state_dict())
    prod = prod.to(DEV)
    warm = FusedTrainStep(prod, FusedAdam(prod, lr=1e-3, eps=1e-4), alpha=0.5)
    for s_ in range(40):
        x, mask, label = _batch7(4, size, 100 + s_)
        warm(x.to(DEV), mask.to(DEV), label.to(DEV))
    warm.check_nan()
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in prod.state_dict().items()})
    prod.set_compute(dtype)
    ref64 = copy.deepcopy(ref).double()
    x, mask, label = _batch7(N, size, 21)
    step = FusedTrainStep(prod, FusedAdam(prod, lr=1e-4, eps=1e-4), alpha=0.5)
    st = step.load_batch(x.to(DEV), mask.to(DEV), label.to(DEV))
    cell, fwd, wg = _first_cell_launches(st)
    assert cell.cin == 7 and not cell.stem16 and not cell.z16 and not cell.c8
    assert (fwd, wg) == ("conv3x3_direct_kernel", "conv3x3_wgrad_direct_kernel + splitk_reduce")
    losses = step.run(st).cpu()
    ls = prod.loss_scale
    with O.lowp_conv3x3(dtype, model=[ref, ref64], da16=False):
        t32 = O.train_step(ref, O.make_adam(ref, 1e-4), x, mask, label, 0.5, True, 3, loss_scale=ls)
        t64 = O.train_step(ref64, O.make_adam(ref64, 1e-4), x.double(), mask.double(), label, 0.5, True, 3, loss_scale=ls)
    assert losses[3].item() == 0.0
    rel = lambda a, b: ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()      # noqa: E731
    print("loss", losses[0].item(), t32[0].item(), t64[0].item())
    assert abs(losses[0].item() - t64[0].item()) < max(3 * abs(t32[0].item() - t64[0].item()), 5e-4)
    assert rel(st.logits.data.view(N, -1), t64[3][0]) < max(3 * rel(t32[3][0], t64[3][0]), 2e-3)
    for got, w32, w64 in zip(st.segs, t32[4], t64[4]):
        assert rel(got.data, w64) < max(3 * rel(w32, w64), 2e-3)
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad = []
    for name in prod._order:
        if name.endswith("conv.bias") or g64[name].grad.norm().item() == 0.0:
            continue
        e_hip, e_cpu = rel(prod._grad_view(name) / ls, g64[name].grad), rel(g32[name].grad, g64[name].grad)
        if name == cell.wname:
            print("first-layer weight gradient", name, "e_hip", e_hip, "e_cpu", e_cpu)
        if not e_hip < max(3 * e_cpu, 5e-2):
            bad.append((name, round(e_hip, 4), round(e_cpu, 4)))
    assert not bad, bad


# ---- the programs of a model with at most 5 channels are what they were: tests/golden/step_programs_5ch.json is the listing of the commit
# before this feature (op kinds per program, coverage keys per family as tests/step_programs.py spells them; the keys of the "loss" family
# were added to it with that family, from the same four loss ops its "kinds" already listed)
FIVE = [(arch, dtype) for arch in ("MTUNetPlusPlus", "MTnnUNet") for dtype in ("f32", "bf16", "f16")]


def _build_with_channels(cin):
    def make_model(arch):
        model = SP.multitask_model(arch.split("-")[0], sequences=cin)
        assert model.in_channels == cin
        return model
    return SP.step_builder(make_model, alpha=0.5, inversely_weighted=True)


def five_channel_listing(arch, dtype):
    """{"kinds": {program name: [op kind]}, "keys": {family: [repr(key)], sorted}} of the 5-channel model's step at 2 x 64 x 64."""
    s = SP.survey((arch + "-5ch", dtype, 2, 64), build=_build_with_channels(5))
    return {"kinds": {name: [int(k) for k in kinds] for name, kinds in s.kinds.items()},
            "keys": {family: sorted(repr(key) for key in seen) for family, seen in s.seen.items()}}


@pytest.mark.parametrize("arch,dtype", FIVE, ids=[f"{a}-{d}" for a, d in FIVE])
def test_five_channel_programs_are_unchanged(arch, dtype):
    with open(GOLDEN) as f:
        want = json.load(f)[f"{arch}-{dtype}"]
    got = five_channel_listing(arch, dtype)
    assert got["kinds"] == want["kinds"]
    for family in want["keys"]:
        assert got["keys"][family] == want["keys"][family], family
    assert set(got["keys"]) == set(want["keys"])


# ------------------------------------------------------------------------------------------------ 5. the launches of the 7-channel step programs
# The benchmark's shapes (tests/step_programs.STEP_PROGRAMS) with a 7-channel model, built and not run.  A first cell of 7 channels is no stem
# (MTBC_STEM_MAX_CIN = 5) and no multiple of 8: the direct forward and weight-gradient kernels on fp32 planes, an fp32 conv output, and in the
# 16-bit modes the channel-group InstanceNorm forward computing its own statistics from that fp32 z (teams at these plane sizes) in front of
# the fp32 backward of norm.hip.  Every coverage key of those programs that no table of tests/test_ops_gpu.py makes has ONE row below, run
# through that file's fp64 tests at its shape rule (the fewest pixels at which the dummy-pointer struct has the key of the step's launch).
PROGRAMS7 = [(arch + "-7ch", dtype, N, size) for arch, dtype, N, size in SP.STEP_PROGRAMS]
F_, W_ = L.OP_CONV3_FWD, L.OP_CONV3_WGRAD
# (op, N, segs, Cout, H, W, mode) as in CONV3_STEP_CASES.  In brackets: the launch of the step.
CONV3_CASES = [
    (F_, 2, [7], 24, 20, 48, dict()),                  # conv3x3_direct_kernel (bias, ragged_rows, ragged_k)  [N x 7 -> 24 in MTUNetPlusPlus bf16 / f16 / f32]
    (F_, 2, [7], 32, 20, 48, dict(bias=False)),        # conv3x3_direct_kernel (ragged_k)  [64 x 7 -> 32 @ 256 x 256 in MTnnUNet bf16]
    (W_, 3, [7], 24, 20, 48, dict(bias=False)),        # conv3x3_wgrad_direct_kernel + splitk_reduce (ragged_rows, ragged_k)  [N x 7 -> 24 in MTUNetPlusPlus bf16 / f16 / f32]
    (W_, 3, [7], 32, 20, 48, dict(bias=False)),        # conv3x3_wgrad_direct_kernel + splitk_reduce (ragged_k)  [64 x 7 -> 32 @ 256 x 256 in MTnnUNet bf16]
]
# (N, segs, Cout, H, W, mode) as in WGRAD_PLAN_CASES of tests/test_ops_gpu.py, and by its shape rule: the plan keys (tests/step_programs.py
# _wgrad_plan_key) of the 7-channel first cell's weight gradient that no table of that file makes -- the direct kernel deals a batch of 16
# images one per split and a larger one two or four (`images>1`).  In brackets: the launch of the step.
WGRAD_PLAN_CASES = [
    (24, [7], 8, 8, 8, dict(bias=False)),              # conv3x3_wgrad_direct_kernel + splitk_reduce (images>1, splitk_reduce<4> x2)  [32 x 7 -> 24 @ 256 x 256 in MTUNetPlusPlus bf16 / f32, 64 x 7 -> 32 in MTnnUNet bf16]
    (8, [7], 8, 8, 8, dict(bias=False)),               # conv3x3_wgrad_direct_kernel + splitk_reduce (splitk_reduce<4> x2)  [16 x 7 -> 24 @ 512 x 512 in MTUNetPlusPlus f16]
]
# (backward, N, C, H, W, mode) as in INORM_CASES.  The team size follows the plane (T = 32 at 256 x 256, 128 at 512 x 512); reserve_cus leaves one
# team resident so that two items take two rounds, as that file's backward team cases do.  The fp32 backward: the largest plane of the register
# kernel (65000 elements) without parameters, the smallest above it (66560) with them.
_AFF, _NOA = dict(affine=True, slope=0.1), dict(affine=False, slope=0.01)
INORM_CASES = [
    (False, 1, 16, 256, 256, dict(compute=1, out="c8", **_AFF, reserve_cus=240, rounds=">1")),      # in_fwd_c8_kernel<512, 4, false, true, 0> [T=32 rounds>1] (affine)  [32 x 24 @ 256 x 256 in MTUNetPlusPlus bf16]
    (False, 1, 16, 256, 256, dict(compute=1, out="c8", **_NOA, reserve_cus=240, rounds=">1")),      # in_fwd_c8_kernel<512, 4, false, true, 0> [T=32 rounds>1]  [64 x 32 @ 256 x 256 in MTnnUNet bf16]
    (False, 1, 16, 512, 512, dict(compute=2, out="c8", **_AFF, reserve_cus=192, rounds=">1")),      # in_fwd_c8_kernel<512, 4, true, true, 0> [T=128 rounds>1] (affine)  [16 x 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (True, 1, 2, 260, 256, dict(**_AFF, dbias=True, inplace=True)),                                # in_bwd_kernel<true> [threads=1024] + in_dparam_kernel (affine, dgamma, dbeta, dbias_pre, inplace)  [16 x 24 @ 512 x 512 in MTUNetPlusPlus f16]
    (True, 1, 2, 250, 260, dict(**_NOA, inplace=True)),                                            # in_bwd_reg_kernel<16, false> [threads=1024] (inplace)  [64 x 32 @ 256 x 256 in MTnnUNet bf16]
]


def _ops_gpu():
    import test_ops_gpu as OPS
    return OPS


@pytest.mark.parametrize("case", CONV3_CASES, ids=lambda c: _ops_gpu()._conv3_case_id(c))
def test_seven_channel_conv3x3_launches_match_fp64(case):
    _ops_gpu().test_conv3x3_step_instances_match_fp64(case)


@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=lambda c: _ops_gpu()._wgrad_plan_case_id(c))
def test_seven_channel_wgrad_plans_match_fp64(case):
    _ops_gpu().test_conv3x3_wgrad_plan_cases_match_fp64(case)


@pytest.mark.parametrize("case", INORM_CASES, ids=lambda c: _ops_gpu()._inorm_case_id(c))
def test_seven_channel_instnorm_launches_match_fp64(case):
    _ops_gpu().test_instnorm_step_instances_match_fp64(case)


def _survey7(program):
    return SP.survey(program, build=_build_with_channels(7))


def _own_keys():
    return SP.table_keys(conv3=CONV3_CASES, wgrad_plan=WGRAD_PLAN_CASES, inorm=INORM_CASES)


@pytest.mark.parametrize("program", PROGRAMS7, ids=["-".join(map(str, p)) for p in PROGRAMS7])
def test_seven_channel_programs_launch_only_reference_tested_instances(program):
    """Every coverage key of the 7-channel step program -- kernel instances AND the branches the arguments select, as tests/step_programs.py
    keys them -- is the key of a call that an element-wise reference test makes: the tables of tests/test_ops_gpu.py and
    tests/test_loss_launches_gpu.py or the rows above."""
    s = _survey7(program)
    assert any(where[1] == 7 for (kind, where) in s.seen["conv3x3"].values()), "no 7-channel conv in the program"
    SP.assert_only_tested(s, SP.reference_tested_keys(), _own_keys())


def test_seven_channel_rows_are_all_needed():
    """Every row above makes a key that a surveyed program launches, that no table of tests/test_ops_gpu.py makes and that no other row makes:
    no dead and no double rows, and deleting one fails the guard above."""
    SP.assert_rows_needed("tests/test_spatial_planes_gpu.py", [_survey7(p) for p in PROGRAMS7], SP.reference_tested_keys(), _own_keys(),
                          [CONV3_CASES, WGRAD_PLAN_CASES, INORM_CASES])
