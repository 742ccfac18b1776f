"""Device-resident dataset on the GPU: mtbc_batch_assemble against torch (identity path, bit-exact), against the existing augmentation
kernel (rotated path, bit-exact: ONE coordinate function) and against the torchvision restatement; `load_indexed` / `indexed` and the
epoch drivers against the tensor-fed `load_batch` / `__call__` / `validate_one_epoch`; extra intensity channels through a model."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import augment as AUG  # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD  # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex  # noqa: E402
from multi_task_breast_cancer_amd.miscellany import seed_everything  # noqa: E402
from multi_task_breast_cancer_amd.nets import MTnnUNet  # noqa: E402
from multi_task_breast_cancer_amd.optim import FusedAdam  # noqa: E402
from multi_task_breast_cancer_amd.trainer import (FusedEvalStep, FusedTrainStep, train_one_epoch, validate_one_epoch,  # noqa: E402
                                                  validate_one_epoch_indexed)
from oracle import torch_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
ALL4 = {"brightness_brighter": True, "brightness_darker": True, "contrast_low": True, "contrast_high": True}
ANGLES = [0.0, 90.0, -90.0, 180.0, 37.5, -123.4, 359.0, 12.0, -300.25]      # test_flip_rotate_matches_torchvision_restatement's
HF = [0, 1, 0, 1, 1, 0, 1, 0, 1]
VF = [0, 0, 1, 1, 0, 1, 1, 0, 0]
TRANSFORMS = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}


def store(M, H, W, seed):
    """uint8 image / mask stores (M, H, W) and int64 labels (M) from the oracle's synthetic batch."""
    img, mask, label = O.synthetic_batch(M, H, W, seed=seed)
    return img[:, 0].round().to(torch.uint8), mask[:, 0].to(torch.uint8), label.flatten().long()


def torch_stack(images, masks, luts, index):
    """cat([mask, image] + extras) as the reference's __getitem__ builds it (BUSI_dataset.py:154), for rows `index`, on the CPU."""
    idx = torch.as_tensor(index, dtype=torch.long)
    im = images[idx]
    planes = [masks[idx].float(), im.float()] + [torch.from_numpy(l.astype(np.float32))[im.long()] for l in luts]
    return torch.stack(planes, dim=1)


@pytest.mark.parametrize("H,W", [(16, 20), (17, 30)])          # the vector path and the scalar path (W % 4 != 0, odd H * W)
@pytest.mark.parametrize("aug", [None, ALL4])                   # K = 0 and K = 4
def test_identity_path_is_bit_exact(H, W, aug):
    images, masks, labels = store(7, H, W, seed=5)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=aug)
    luts = DD.intensity_luts(aug)
    assert ds.n_augments == len(luts) == (4 if aug else 0) and len(ds) == 7 and (ds.H, ds.W) == (H, W)
    index = [6, 0, 0, 3, 5]                                      # repeats; N * H * W / 4 is not a multiple of the block
    want = torch_stack(images, masks, luts, index)
    image, mask, onehot = ds.assemble(index)
    assert image.shape == (5, 1 + len(luts), H, W) and mask.shape == (5, 1, H, W) and onehot.shape == (5, 3)
    assert torch.equal(image[:, 0].cpu(), images[index].float())
    for k, l in enumerate(luts):
        assert torch.equal(image[:, 1 + k].cpu(), torch.from_numpy(l.astype(np.float32))[images[index].long()]), k
    assert torch.equal(image.cpu(), want[:, 1:])
    assert torch.equal(mask.cpu(), masks[index].float()[:, None])
    assert torch.equal(onehot.cpu(), torch.nn.functional.one_hot(labels[index], 3).float())
    # binary head: the float label itself; a device index; preallocated outputs (filled with a sentinel: every element is written)
    out = tuple(torch.full(s, -7.0, device=DEV) for s in ((5, 1 + len(luts), H, W), (5, 1, H, W), (5, 1)))
    got = ds.assemble(torch.tensor(index, dtype=torch.int32, device=DEV), n_onehot=0, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert torch.equal(out[0].cpu(), want[:, 1:]) and torch.equal(out[1].cpu(), want[:, :1])
    assert torch.equal(out[2].cpu(), labels[index].float().view(-1, 1))
    with pytest.raises(ValueError):
        ds.assemble([0, 7])                                      # a host index is validated before it is uploaded


@pytest.mark.parametrize("H,W", [(64, 64), (48, 80), (17, 30)])
@pytest.mark.parametrize("aug", [None, ALL4])
def test_rotated_path_equals_the_augmentation_kernel(H, W, aug):
    """The same source pixel, operation for operation (flip_rotate_src of csrc/common.h): `assemble` is `flip_rotate` of the float stack."""
    images, masks, labels = store(7, H, W, seed=3)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=aug)
    index = [6, 0, 0, 3, 5, 1, 2, 4, 6]
    params = AUG.params_from(ANGLES, HF, VF)
    want = AUG.flip_rotate(torch_stack(images, masks, DD.intensity_luts(aug), index).to(DEV), params)
    image, mask, onehot = ds.assemble(index, params.to(DEV))
    assert torch.equal(mask, want[:, :1])
    assert torch.equal(image, want[:, 1:])
    assert torch.equal(onehot.cpu(), torch.nn.functional.one_hot(labels[index], 3).float())
    if aug:     # zero fill outside the rotated frame on the LUT planes too (a "brighter" plane is 0 out there, not 80): the corner of a 37.5 degree turn
        assert image[4, :, 0, 0].abs().max().item() == 0.0 and DD.intensity_luts(aug)[0][0] == 80


@pytest.mark.parametrize("H,W", [(64, 64), (48, 80)])
def test_rotated_path_matches_torchvision_restatement(H, W):
    images, masks, labels = store(9, H, W, seed=3)
    masks = images & 1                                           # a binary plane that is a function of the image plane: planes that move apart show
    aug = {"contrast_low": True, "contrast_high": True}          # both map 0 to 0, so lut[image plane] holds outside the rotated frame as well
    luts = DD.intensity_luts(aug)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=aug)
    index = list(range(9))
    want = O.tv_flip_rotate(torch_stack(images, masks, luts, index), ANGLES, HF, VF)
    image, mask, _ = ds.assemble(index, AUG.params_from(ANGLES, HF, VF).to(DEV))
    got = torch.cat([mask, image], dim=1).cpu()
    # identical gather except where the source coordinate sits on a .5 tie and the fp32 products round differently (the existing test's cap)
    diff = (got != want).float().mean(dim=(1, 2, 3))
    print("share of differing pixels per image:", diff.tolist())
    assert diff.max().item() < 2e-3, diff
    for i in (0, 3):                                             # angle 0 / 180 with flips: pure index permutations
        assert torch.equal(got[i], want[i]), i
    # planes move together: every plane of a sample comes from the same source pixel
    src = got[:, 1].long()
    assert torch.equal(got[:, 0], (src & 1).float())
    for k, l in enumerate(luts):
        assert torch.equal(got[:, 2 + k], torch.from_numpy(l.astype(np.float32))[src]), k
    assert set(torch.unique(got[:, 0]).tolist()) <= {0.0, 1.0}   # nearest: a binary mask stays binary


def host_batch(images, masks, labels, index, params):
    """What a caller of `load_batch` assembles: fp32 image / mask (the existing augmentation kernel for the transform) and the float label."""
    stack = torch_stack(images, masks, [], index).to(DEV)
    if params is not None:
        stack = AUG.flip_rotate(stack, torch.as_tensor(params))
    return stack[:, 1:].contiguous(), stack[:, :1].contiguous(), labels[torch.as_tensor(index, dtype=torch.long)].float().view(-1, 1).to(DEV)


def twin_steps(seed, compute=None, **kw):
    out = []
    for _ in range(2):
        seed_everything(seed)
        model = MTnnUNet(1, 1, 3).to(DEV)
        if compute:
            model.set_compute(compute)
        opt = FusedAdam(model, lr=1e-4, eps=1e-4)
        out.append((model, FusedTrainStep(model, opt, alpha=0.5, **kw)))
    return out


@pytest.mark.parametrize("compute", [None, "bf16"])
def test_load_indexed_step_equals_load_batch_step(compute):
    images, masks, labels = store(7, 64, 64, seed=8)
    ds = DD.DeviceDataset(images, masks, labels)
    (ma, sa), (mb, sb) = twin_steps(21, compute)
    assert all(torch.equal(pa, pb) for pa, pb in zip(ma.parameters(), mb.parameters()))
    for s, index in enumerate(([6, 0], [3, 5])):
        params = AUG.params_from([37.5, -123.4] if s == 0 else [180.0, 12.0], [1, 0], [0, 1])
        la = sa.run(sa.load_indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV), params.to(DEV)))
        lb = sb.run(sb.load_batch(*host_batch(images, masks, labels, index, params)))
        assert torch.equal(la, lb), (s, la.tolist(), lb.tolist())
    assert torch.equal(ma.flat_p, mb.flat_p)
    sa.check_nan()


def epoch_setup(n_images, G, seed=13):
    images, masks, labels = store(n_images, 64, 64, seed=30)
    ds = DD.DeviceDataset(images, masks, labels)
    ei = EpochIndex(np.arange(n_images), G, seed=seed, drop_last=False)
    return images, masks, labels, ds, ei


def test_train_one_epoch_equals_the_hand_written_loop():
    images, masks, labels, ds, ei = epoch_setup(10, 4)
    (ma, sa), (mb, sb) = twin_steps(22)
    for epoch in range(2):
        got = train_one_epoch(sa, ds, DD.EpochTables(ei, epoch, TRANSFORMS), lr=1e-4)
        host = DD.EpochTables(ei, epoch, TRANSFORMS, device=None)
        assert [n for _, n in host.batches] == [4, 4, 2]
        acc = torch.zeros(3, dtype=torch.float64)
        for b in range(len(host)):
            index, params, n, _ = host.batch(b)
            acc += sb.run(sb.load_batch(*host_batch(images, masks, labels, index.tolist(), params)))[:3].double().cpu()
        want = (acc / len(host)).tolist()
        print("epoch", epoch, "averages", got, want)
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-12 * abs(w), (got, want)
        assert torch.equal(ma.flat_p, mb.flat_p), epoch


def test_train_one_epoch_graph_replay_equals_eager():
    images, masks, labels, ds, ei = epoch_setup(12, 2)
    (ma, sa), (mb, sb) = twin_steps(23)
    sa.graph, sb.graph = True, False
    tables = DD.EpochTables(ei, 0, TRANSFORMS)
    got, want = train_one_epoch(sa, ds, tables), train_one_epoch(sb, ds, tables)
    assert any(ent[2] is not None for ent in sa._graphs.values())             # six steps of one plan: captured at the third, replayed after
    print("graph", got, "eager", want)
    assert torch.equal(ma.flat_p, mb.flat_p)


def test_validate_one_epoch_indexed_equals_validate_one_epoch():
    images, masks, labels, ds, ei = epoch_setup(10, 4)
    seed_everything(24)
    model = MTnnUNet(1, 1, 3).to(DEV)
    step = FusedEvalStep(model, alpha=0.5)
    got = validate_one_epoch_indexed(step, ds, DD.EpochTables(ei, 0))
    host = DD.EpochTables(ei, 0, device=None)
    loader = []
    for b in range(len(host)):
        idx = torch.as_tensor(host.batch(b)[0], dtype=torch.long)
        loader.append({"image": images[idx].float()[:, None], "mask": masks[idx].float()[:, None], "label": labels[idx].float().view(-1, 1)})
    want = validate_one_epoch(step, loader, DEV)
    assert len(got) == 6 and got == want, (got, want)
    with pytest.raises(ValueError):
        validate_one_epoch_indexed(step, ds, DD.EpochTables(ei, 0, TRANSFORMS))


def test_rank_shards_reassemble_the_single_process_batch():
    images, masks, labels = store(10, 17, 30, seed=9)
    ds = DD.DeviceDataset(images, masks, labels, augmentation={"brightness_darker": True})
    mk = lambda rank, world: DD.EpochTables(EpochIndex(np.arange(10), 4, seed=5, rank=rank, world=world, drop_last=False), 1, TRANSFORMS)   # noqa: E731
    one, ranks = mk(0, 1), [mk(0, 2), mk(1, 2)]
    for b in range(len(one)):
        want = ds.assemble(*one.batch(b)[:2])
        parts = [ds.assemble(*t.batch(b)[:2]) for t in ranks]
        for k in range(3):
            assert torch.equal(torch.cat([p[k] for p in parts]), want[k]), (b, k)


def test_extra_channels_through_a_model_match_the_oracle():
    aug = {"brightness_brighter": True, "contrast_high": True}
    images, masks, labels = store(5, 64, 64, seed=12)
    ds = DD.DeviceDataset(images, masks, labels, augmentation=aug)
    assert ds.n_augments == 2
    seed_everything(25)
    prod = MTnnUNet(1 + ds.n_augments, 1, 3)
    ref = O.build_oracle_model("MTnnUNet", 3, 1, 3)
    ref.load_state_dict(prod.state_dict())
    prod = prod.to(DEV)
    step = FusedTrainStep(prod, FusedAdam(prod, lr=1e-4, eps=1e-4), alpha=0.35)
    index, params = [4, 1], AUG.params_from([37.5, 180.0], [1, 0], [0, 1])
    stack = AUG.flip_rotate(torch_stack(images, masks, DD.intensity_luts(aug), index).to(DEV), params).cpu()
    total, seg, cls, _, _ = O.train_step(ref, O.make_adam(ref, 1e-4), stack[:, 1:].contiguous(), stack[:, :1].contiguous(),
                                         labels[index].float().view(-1, 1), 0.35, True, 3)
    losses = step.run(step.load_indexed(ds, torch.tensor(index, dtype=torch.int32, device=DEV), params.to(DEV))).cpu().tolist()
    print("fused", losses[:3], "oracle", [total.item(), seg.item(), cls.item()])
    for g, w in zip(losses[:3], (total, seg, cls)):
        assert abs(g - w.item()) < 1e-4, (losses, total.item(), seg.item(), cls.item())
    assert losses[3] == 0.0
    with pytest.raises(ValueError):                              # a 1-channel dataset into the 3-channel model
        step.load_indexed(DD.DeviceDataset(images, masks, labels), torch.tensor(index, dtype=torch.int32, device=DEV), None)
