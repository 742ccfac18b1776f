"""The dataset on the device: one upload, one HIP launch per batch -- the training-epoch side of SURVEY 8(f) rows N1 / N2.

The reference keeps the whole dataset in RAM as uint8 (BUSI_dataset.py:47-92: curated BUSI is 450 images, 29 MB at 256 x 256) and
builds every item on the CPU with 0 workers (:97-158).  Here the uint8 stores live on the GPU and `mtbc_batch_assemble`
(csrc/batch_loader.hip) goes from a device index array straight to the fp32 buffers a step reads: image (+ the intensity variants
of `data.augmentation` as look-up tables), mask, class target, all under one joint flip / rotation.  The two spatial variants (CLAHE,
SOBEL) are OpenCV filters with no oracle here: the caller computes them once per image and hands them over as uint8 planes
(`spatial_planes`), which are stored next to the images and gathered like them (`mtbc_batch_assemble_planes`).

    ds = DeviceDataset(images_u8, masks_u8, labels, augmentation=config["data"]["augmentation"])
    tables = EpochTables(EpochIndex(train_positions, 32, seed), epoch, transforms={"horizontal_flip": .5, "vertical_flip": .5, "rotation": 1.0})
    train_one_epoch(step, ds, tables)                                       # trainer.py: no host work per batch
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .dataset_index import EpochIndex

# the reference's append order (BUSI_dataset.py:123-139): channel 1 + k of the image is LUT_KEYS-order entry k of those switched on
LUT_KEYS = ("brightness_brighter", "brightness_darker", "contrast_low", "contrast_high")
SPATIAL_KEYS = _SPATIAL_KEYS = ("CLAHE", "SOBEL")        # ... in front of them (:114-122), as stored planes the caller supplies


def channel_names(augmentation: Optional[dict]) -> Tuple[str, ...]:
    """The model-input channels a DeviceDataset emits for `data.augmentation`, in order: "image", then every flag that is on in the
    reference's append order (BUSI_dataset.py:114-139) -- the stored planes CLAHE, SOBEL, then the look-up-table channels."""
    aug = dict(augmentation or {})
    unknown = set(aug) - set(LUT_KEYS) - set(SPATIAL_KEYS)
    if unknown:
        raise ValueError(f"unknown data.augmentation keys {sorted(unknown)}")
    return ("image",) + tuple(k for k in SPATIAL_KEYS + LUT_KEYS if aug.get(k, False))


def _check_spatial_planes(augmentation: Optional[dict], spatial_planes: Optional[dict], shape) -> List:
    """The stored planes of the spatial flags that are on, in SPATIAL_KEYS order; ValueError for a flag without its plane, a plane
    without its flag, an unknown key, a plane that is not uint8 or not of the image store's shape."""
    aug, planes = dict(augmentation or {}), dict(spatial_planes or {})
    unknown = set(planes) - set(SPATIAL_KEYS)
    if unknown:
        raise ValueError(f"unknown spatial_planes keys {sorted(unknown)}: the stored planes are {', '.join(SPATIAL_KEYS)}")
    out = []
    for key in SPATIAL_KEYS:
        on = bool(aug.get(key, False))
        if on and key not in planes:
            raise ValueError(f"data.augmentation.{key} is a spatial OpenCV filter: the device-resident dataset does not compute it, it takes "
                             f"the filtered images as spatial_planes[{key!r}] (uint8, one plane per image)")
        if key in planes and not on:
            raise ValueError(f"spatial_planes[{key!r}] given but data.augmentation.{key} is off: the plane would be ignored")
        if on:
            pl = planes[key] if getattr(planes[key], "is_cuda", False) else _as_numpy(planes[key])
            if str(pl.dtype).split(".")[-1] != "uint8":
                raise ValueError(f"spatial_planes[{key!r}] must be uint8, got {pl.dtype}")
            if tuple(pl.shape) != tuple(shape):
                raise ValueError(f"spatial_planes[{key!r}] must have the image store's shape {tuple(shape)}, got {tuple(pl.shape)}")
            out.append(pl)
    return out


def intensity_luts(augmentation: Optional[dict]) -> np.ndarray:
    """(K, 256) uint8: row k maps a pixel value to the k-th intensity variant `data.augmentation` switches on, in the reference's
    append order.  Each is the reference's expression over every uint8 value (BUSI_dataset.py:123-139):
        brightness_brighter  cv2.add(image, 80)       -- saturating on uint8
        brightness_darker    cv2.subtract(image, 80)  -- saturating on uint8
        contrast_low         np.uint8(np.float64(image) * .02)
        contrast_high        np.uint8(np.clip(np.float64(image) * 1.5, 0, 255))
    CLAHE and SOBEL are spatial OpenCV filters, not functions of the pixel value: not covered (ValueError)."""
    aug = dict(augmentation or {})
    for key in _SPATIAL_KEYS:
        if aug.get(key, False):
            raise ValueError(f"data.augmentation.{key} is a spatial OpenCV filter: the device-resident dataset covers the intensity variants "
                             f"({', '.join(LUT_KEYS)}) only")
    unknown = set(aug) - set(LUT_KEYS) - set(_SPATIAL_KEYS)
    if unknown:
        raise ValueError(f"unknown data.augmentation keys {sorted(unknown)}")
    x = np.arange(256, dtype=np.uint8)
    rows = []
    if aug.get("brightness_brighter", False):
        rows.append(np.clip(x.astype(np.int32) + 80, 0, 255).astype(np.uint8))
    if aug.get("brightness_darker", False):
        rows.append(np.clip(x.astype(np.int32) - 80, 0, 255).astype(np.uint8))
    if aug.get("contrast_low", False):
        rows.append(np.uint8(np.float64(x) * .02))
    if aug.get("contrast_high", False):
        rows.append(np.uint8(np.clip(np.float64(x) * 1.5, 0, 255)))
    return np.stack(rows).astype(np.uint8) if rows else np.zeros((0, 256), dtype=np.uint8)


def _as_numpy(a) -> np.ndarray:
    try:
        import torch
        if isinstance(a, torch.Tensor):
            return a.detach().cpu().numpy()
    except ImportError:         # numpy-only callers
        pass
    return np.asarray(a)


class DeviceDataset:
    """uint8 image / mask stores (M, H, W) and int32 labels (M) on the device, uploaded once.  `assemble` is the kernel call.
    spatial_planes = {"CLAHE": (M, H, W) uint8, "SOBEL": ...}: the filtered images of the spatial flags that are on in `augmentation`,
    computed by the caller, on the host or on the device; exactly the flags that are on, nothing is ignored."""

    def __init__(self, images_u8, masks_u8, labels, augmentation: Optional[dict] = None, device="cuda:0",
                 spatial_planes: Optional[dict] = None):
        names = channel_names(augmentation)
        luts = intensity_luts({k: True for k in names if k in LUT_KEYS})
        on_device = all(getattr(a, "is_cuda", False) for a in (images_u8, masks_u8))
        img, msk, lab = images_u8, masks_u8, labels
        if not on_device:
            img, msk = _as_numpy(images_u8), _as_numpy(masks_u8)
        lab = _as_numpy(labels)
        if str(img.dtype).split(".")[-1] != "uint8" or str(msk.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"image and mask stores must be uint8, got {img.dtype} and {msk.dtype}")
        if len(img.shape) != 3 or tuple(img.shape) != tuple(msk.shape) or 0 in tuple(img.shape):
            raise ValueError(f"image and mask stores must be (M, H, W) of one shape, got {tuple(img.shape)} and {tuple(msk.shape)}")
        M, H, W = (int(v) for v in img.shape)
        if M * H * W >= 2 ** 40 or H * W >= 2 ** 31:
            raise ValueError("store too large")
        if lab.shape != (M,):
            raise ValueError(f"labels must be ({M},), got {lab.shape}")
        if lab.dtype.kind not in "iu":
            if lab.dtype.kind != "f" or not np.array_equal(lab, np.round(lab)):
                raise ValueError(f"labels must be integers, got {lab.dtype}")
        if lab.size and (lab.min() < 0 or lab.max() > 2):
            raise ValueError("labels must be in {0, 1, 2}")
        if int(msk.max()) > 1:
            raise ValueError("mask values must be in {0, 1} (the reference maps 255 to 1 at load time, BUSI_dataset.py:55)")
        planes = _check_spatial_planes(augmentation, spatial_planes, (M, H, W))
        L.require_gpu()
        import torch
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.images = (img if on_device else torch.from_numpy(np.ascontiguousarray(img))).to(self.device).contiguous()
        self.masks = (msk if on_device else torch.from_numpy(np.ascontiguousarray(msk))).to(self.device).contiguous()
        self.labels = torch.from_numpy(lab.astype(np.int32)).to(self.device)
        self.luts = torch.from_numpy(luts).to(self.device)
        self.M, self.H, self.W = M, H, W
        # ONE (E, M, H, W) store, CLAHE before SOBEL: the kernel's channel 1 + e
        self.planes = torch.stack([(pl if getattr(pl, "is_cuda", False) else torch.from_numpy(np.ascontiguousarray(pl))).to(self.device)
                                   for pl in planes]).contiguous() if planes else None
        self.n_planes, self.n_luts = len(planes), int(luts.shape[0])
        self.channels = names
        self.n_augments = self.n_planes + self.n_luts   # what load_multitask_experiment_artefacts(n_augments=...) adds to the model's input layer

    def __len__(self) -> int:
        return self.M

    def upload_index(self, index):
        """Host indices -> validated int32 device array (the kernel's own guard only keeps a bad index from reading outside the stores)."""
        import torch
        idx = _as_numpy(index).astype(np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError("empty index")
        if idx.min() < 0 or idx.max() >= self.M:
            raise ValueError(f"index outside [0, {self.M})")
        return torch.from_numpy(idx.astype(np.int32)).to(self.device)

    def assemble(self, index, params=None, n_onehot: int = 3, out: Optional[Sequence] = None) -> Tuple:
        """index (N) int32 device tensor (a host array is validated against M and uploaded), params (N, 4) device tensor from
        `augment.random_params` or None = identity -> (image (N, 1 + E + K, H, W), mask (N, 1, H, W), target) fp32, written by ONE launch on
        the current stream.  target: one-hot (N, 3) with n_onehot=3, the float label (N, 1) with n_onehot=0 (binary head).
        `out`: that triple preallocated (a step's static buffers)."""
        import torch
        if n_onehot not in (0, 3):
            raise ValueError("n_onehot is 3 (one-hot) or 0 (float label)")
        if not (isinstance(index, torch.Tensor) and index.is_cuda):
            index = self.upload_index(index)
        if index.dtype != torch.int32 or not index.is_contiguous():
            index = index.to(torch.int32).contiguous()
        if index.dim() != 1 or index.numel() == 0 or index.device != self.device:
            raise ValueError("index must be a non-empty 1-d tensor on the dataset's device")
        N = int(index.numel())
        if params is not None:
            if not (isinstance(params, torch.Tensor) and params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()):
                params = torch.as_tensor(params, dtype=torch.float32).to(self.device).contiguous()
            if tuple(params.shape) != (N, 4) or params.device != self.device:
                raise ValueError(f"params must be ({N}, 4) on the dataset's device, got {tuple(params.shape)}")
        C_img = 1 + self.n_augments
        shapes = ((N, C_img, self.H, self.W), (N, 1, self.H, self.W), (N, n_onehot or 1))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        else:
            out = tuple(out)
            if len(out) != 3:
                raise ValueError("out = (image, mask, target)")
            for t, s in zip(out, shapes):
                if tuple(t.shape) != s or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError(f"out buffer {tuple(t.shape)} {t.dtype}: expected contiguous float32 {s} on {self.device}")
        a = L.BatchPlanesArgs() if self.n_planes else L.BatchArgs()
        a.M, a.N, a.H, a.W, a.K, a.n_onehot = self.M, N, self.H, self.W, self.n_luts, n_onehot
        a.images, a.masks, a.labels = self.images.data_ptr(), self.masks.data_ptr(), self.labels.data_ptr()
        a.index = index.data_ptr()
        a.params = params.data_ptr() if params is not None else None
        a.luts = self.luts.data_ptr() if self.n_luts else None
        a.out_image, a.out_mask, a.out_target = (t.data_ptr() for t in out)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.n_planes:       # with stored planes: the entry point that gathers them; without: the call as it always was
            a.E, a.planes = self.n_planes, self.planes.data_ptr()
            L.check(L.load().mtbc_batch_assemble_planes(C.byref(a), stream), "batch_assemble_planes")
        else:
            L.check(L.load().mtbc_batch_assemble(C.byref(a), stream), "batch_assemble")
        return out


class EpochTables:
    """One epoch of one rank as device tables, built in two uploads: `index` (n) int32 = this rank's rows of every batch, batch after
    batch; `params` (n, 4) float32 = their {cos a, sin a, flip_h, flip_v} (None without `transforms`); on the host `batches` =
    [(offset, n_local)] into both and `weights` = EpochIndex.weights(epoch).

    transforms = {"horizontal_flip": p, "vertical_flip": p, "rotation": r}: the reference's RandomHorizontalFlip(p) ->
    RandomVerticalFlip(p) -> RandomRotation(degrees=360 * r) (training_multitask.py:193-197).  The parameters are drawn for the GLOBAL
    epoch order from one generator seeded by (seed, epoch) -- `seed` defaults to the EpochIndex's -- and cut with the bounds that cut
    the indices (EpochIndex.shard_bounds): the union of the ranks' shards is the single-process batch, parameters included.
    device=None keeps numpy arrays (host-side checks, hand-written loops)."""

    def __init__(self, epoch_index: EpochIndex, epoch: int, transforms: Optional[dict] = None, seed: Optional[int] = None,
                 device="cuda:0"):
        ei = epoch_index
        self.epoch = int(epoch)
        G = ei.global_batch
        perm = ei.permutation(self.epoch)[:len(ei) * G]
        gparams = None
        if transforms is not None:
            unknown = set(transforms) - {"horizontal_flip", "vertical_flip", "rotation"}
            if unknown:
                raise ValueError(f"unknown transforms {sorted(unknown)}")
            from .augment import random_params
            rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(ei.seed if seed is None else seed), self.epoch])))
            gparams = random_params(len(perm), rng, float(transforms.get("horizontal_flip", 0.0)), float(transforms.get("vertical_flip", 0.0)),
                                    360.0 * float(transforms.get("rotation", 0.0))).numpy()
        idx_parts, prm_parts = [], []
        self.batches: List[Tuple[int, int]] = []
        off = 0
        for b in range(len(ei)):
            nb = min(G, len(perm) - b * G)
            lo, hi = ei.shard_bounds(nb)
            idx_parts.append(perm[b * G + lo:b * G + hi])
            if gparams is not None:
                prm_parts.append(gparams[b * G + lo:b * G + hi])
            self.batches.append((off, hi - lo))
            off += hi - lo
        self.weights: List[float] = ei.weights(self.epoch)
        index = np.concatenate(idx_parts).astype(np.int32) if idx_parts else np.zeros(0, dtype=np.int32)
        params = np.ascontiguousarray(np.concatenate(prm_parts), dtype=np.float32) if gparams is not None else None
        self.index_min, self.index_max = (int(index.min()), int(index.max())) if index.size else (0, -1)   # host copies: the drivers check them against the store
        self.device = device
        if device is None:
            self.index, self.params = index, params
        else:
            L.require_gpu()
            import torch
            self.index = torch.from_numpy(index).to(device)
            self.params = None if params is None else torch.from_numpy(params).to(device)

    def __len__(self) -> int:
        return len(self.batches)

    def batch(self, b: int):
        """(index, params or None, n_local, weight) of batch b: views into the tables, no copy, no transfer."""
        off, n = self.batches[b]
        return (self.index[off:off + n], None if self.params is None else self.params[off:off + n], n, self.weights[b])
