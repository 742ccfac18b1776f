"""Device-resident dataset, the parts that need no GPU: the intensity look-up tables of `data.augmentation`, the C layout of
mtbc_batch_args, and the host side of the epoch tables (rank shards reassemble the single-process epoch, parameters included)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L   # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD   # noqa: E402
from multi_task_breast_cancer_amd.dataset_index import EpochIndex   # noqa: E402

X = np.arange(256, dtype=np.uint8)
# the reference's expressions (BUSI_dataset.py:123-139) over every uint8 value; cv2.add / cv2.subtract saturate on uint8
LITERAL = {
    "brightness_brighter": np.minimum(X.astype(np.int64) + 80, 255).astype(np.uint8),
    "brightness_darker": np.maximum(X.astype(np.int64) - 80, 0).astype(np.uint8),
    "contrast_low": np.uint8(np.float64(X) * .02),
    "contrast_high": np.uint8(np.clip(np.float64(X) * 1.5, 0, 255)),
}
ORDER = ["brightness_brighter", "brightness_darker", "contrast_low", "contrast_high"]


def test_every_lut_row_is_the_literal_expression():
    luts = DD.intensity_luts({k: True for k in ORDER})
    assert luts.shape == (4, 256) and luts.dtype == np.uint8
    for k, name in enumerate(ORDER):
        assert np.array_equal(luts[k], LITERAL[name]), name
    # spot values: saturation at both ends, truncation of the float products
    assert luts[0][175] == 255 and luts[0][176] == 255 and luts[0][0] == 80
    assert luts[1][80] == 0 and luts[1][79] == 0 and luts[1][255] == 175
    assert luts[2][255] == 5 and luts[2][49] == 0 and luts[2][50] == 1
    assert luts[3][170] == 255 and luts[3][171] == 255 and luts[3][1] == 1 and luts[3][3] == 4


@pytest.mark.parametrize("keys", [["contrast_high", "brightness_brighter"], ["brightness_darker"], ["contrast_low", "brightness_darker", "contrast_high"],
                                  ORDER[::-1]])
def test_lut_row_order_is_the_reference_append_order(keys):
    cfg = {"CLAHE": False, "SOBEL": False, **{k: k in keys for k in ORDER}}
    luts = DD.intensity_luts(cfg)
    want = [k for k in ORDER if k in keys]              # the reference's append order, whatever the dict's order
    assert luts.shape == (len(want), 256)               # = n_augments
    for row, name in zip(luts, want):
        assert np.array_equal(row, LITERAL[name]), name


def test_spatial_filters_raise_and_all_false_is_empty():
    for key in ("CLAHE", "SOBEL"):
        with pytest.raises(ValueError):
            DD.intensity_luts({key: True, "brightness_brighter": True})
    none = DD.intensity_luts({"CLAHE": False, "SOBEL": False, **{k: False for k in ORDER}})
    assert none.shape == (0, 256) and none.dtype == np.uint8
    assert DD.intensity_luts(None).shape == (0, 256)


def test_batch_args_layout_matches_header_and_symbol_is_exported(tmp_path):
    offs = [("n_onehot", L.BatchArgs.n_onehot.offset), ("params", L.BatchArgs.params.offset), ("out_target", L.BatchArgs.out_target.offset)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(mtbc_batch_args));', 'printf("maxluts %d\\n", MTBC_BATCH_MAX_LUTS);']
    for f, _ in offs:
        lines.append(f'printf("{f} %zu\\n", offsetof(mtbc_batch_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(L.BatchArgs)
    assert int(got["maxluts"]) == L.BATCH_MAX_LUTS
    for f, off in offs:
        assert int(got[f]) == off, f
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert "mtbc_batch_assemble" in L.EXPORTS and hasattr(L.load(), "mtbc_batch_assemble")


def test_batch_assemble_refuses_bad_arguments_on_the_host():
    """The argument checks run before any GPU call: shapes first, then pointers and aliasing."""
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()

    def args(**kw):
        a = L.BatchArgs()
        a.M, a.N, a.H, a.W, a.K, a.n_onehot = 4, 2, 8, 8, 0, 3
        a.images, a.masks, a.labels, a.index = 0x10000, 0x20000, 0x30000, 0x40000
        a.out_image, a.out_mask, a.out_target = 0x100000, 0x200000, 0x300000
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    BADSHAPE, BADARG = -1, -2
    for kw in ({"K": 5}, {"K": -1}, {"n_onehot": 2}, {"n_onehot": 1}, {"N": 0}, {"M": 0}, {"H": 0}, {"W": -3}):
        assert lib.mtbc_batch_assemble(C.byref(args(**kw)), None) == BADSHAPE, kw
    for kw in ({"images": None}, {"index": None}, {"out_target": None}, {"K": 2}, {"out_mask": 0x100000}, {"out_image": 0x10000},
               {"out_target": 0x200000 + 16}):
        assert lib.mtbc_batch_assemble(C.byref(args(**kw)), None) == BADARG, kw


def _tables(world, rank, epoch, transforms, seed=None, n=10, G=4):
    ei = EpochIndex(np.arange(100, 100 + n), G, seed=7, rank=rank, world=world, drop_last=False)
    return ei, DD.EpochTables(ei, epoch, transforms=transforms, seed=seed, device=None)


def test_epoch_tables_rank_shards_reassemble_the_single_process_epoch():
    tf = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}
    ei1, one = _tables(1, 0, 3, tf)
    assert one.index.dtype == np.int32 and one.params.dtype == np.float32 and one.params.shape == (10, 4)
    assert [n for _, n in one.batches] == [4, 4, 2] and [o for o, _ in one.batches] == [0, 4, 8]
    assert np.array_equal(one.index, ei1.permutation(3).astype(np.int32))
    assert one.weights == ei1.weights(3) == [1.0, 1.0, 1.0]
    ranks = [_tables(2, r, 3, tf) for r in range(2)]
    idx, prm = [], []
    for b in range(3):
        for ei, t in ranks:
            i, p, n, w = t.batch(b)
            assert n == len(i) == len(p) and w == ei.weights(3)[b]
            idx.append(i)
            prm.append(p)
    assert np.array_equal(np.concatenate(idx), one.index)
    assert np.array_equal(np.concatenate(prm), one.params)            # bit-equal: one draw for the global order, cut like the indices
    for ei, t in ranks:
        assert t.weights == ei.weights(3) == [0.5, 0.5, 0.5]
        assert [n for _, n in t.batches] == [2, 2, 1]
        assert ei.shard_bounds(2) == ei._bounds(2, ei.rank) and ei.shard_bounds(5, 1) == ei._bounds(5, 1)
    # rotation angles are inside the asked range, the flips are 0 / 1, and (cos, sin) is a unit vector
    assert set(np.unique(one.params[:, 2:]).tolist()) <= {0.0, 1.0}
    assert np.allclose(one.params[:, 0] ** 2 + one.params[:, 1] ** 2, 1.0, atol=1e-6)


def test_epoch_tables_epochs_differ_and_repeat():
    tf = {"horizontal_flip": 0.5, "vertical_flip": 0.5, "rotation": 1.0}
    a, b, again = _tables(1, 0, 0, tf)[1], _tables(1, 0, 1, tf)[1], _tables(1, 0, 0, tf)[1]
    assert not np.array_equal(a.index, b.index) and not np.array_equal(a.params, b.params)
    assert np.array_equal(a.index, again.index) and np.array_equal(a.params, again.params)
    other_seed = _tables(1, 0, 0, tf, seed=99)[1]
    assert np.array_equal(a.index, other_seed.index) and not np.array_equal(a.params, other_seed.params)
    # no transforms: the identity path, no parameter table; rotation 0 and flips 0: the identity as parameters
    assert _tables(1, 0, 0, None)[1].params is None
    ident = _tables(1, 0, 0, {"horizontal_flip": 0.0, "vertical_flip": 0.0, "rotation": 0.0})[1].params
    assert np.array_equal(ident, np.tile(np.array([1, 0, 0, 0], dtype=np.float32), (10, 1)))


def test_device_dataset_validates_then_needs_a_gpu():
    import torch
    img = np.zeros((3, 8, 8), dtype=np.uint8)
    lab = np.array([0, 1, 2])
    with pytest.raises(ValueError):
        DD.DeviceDataset(img.astype(np.float32), img, lab)
    with pytest.raises(ValueError):
        DD.DeviceDataset(img, img[:, :4], lab)
    with pytest.raises(ValueError):
        DD.DeviceDataset(img, img + 255, lab)                 # a mask still holding 255
    with pytest.raises(ValueError):
        DD.DeviceDataset(img, img, np.array([0, 1, 3]))
    with pytest.raises(ValueError):
        DD.DeviceDataset(img, img, lab, augmentation={"CLAHE": True})
    if not torch.cuda.is_available():
        with pytest.raises(L.MtbcError):
            DD.DeviceDataset(img, img, lab)
