"""CLAHE / SOBEL as stored planes, the parts that need no GPU: the C layout of mtbc_batch_planes_args against its ctypes mirror, the host-side
refusals of mtbc_batch_assemble_planes, what the DeviceDataset constructor refuses before it asks for a GPU, and the channel order for every
subset of the six `data.augmentation` flags."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtbc.h")

from multi_task_breast_cancer_amd import _lib as L   # noqa: E402
from multi_task_breast_cancer_amd import device_data as DD   # noqa: E402

# the reference's append order (BUSI_dataset.py:114-139), written out
REFERENCE_ORDER = ["CLAHE", "SOBEL", "brightness_brighter", "brightness_darker", "contrast_low", "contrast_high"]
BADSHAPE, BADARG = -1, -2


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_planes_args_layout_matches_header_and_symbol_is_exported(tmp_path):
    fields = ["E", "planes", "params", "out_target"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(mtbc_batch_planes_args));', 'printf("oldsize %zu\\n", sizeof(mtbc_batch_args));',
             'printf("maxplanes %d\\n", MTBC_BATCH_MAX_PLANES);', 'printf("maxluts %d\\n", MTBC_BATCH_MAX_LUTS);', 'printf("version %d\\n", MTBC_VERSION);']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(mtbc_batch_planes_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert got["size"] == C.sizeof(L.BatchPlanesArgs)
    for f in fields:
        assert got[f] == getattr(L.BatchPlanesArgs, f).offset, f
    assert got["maxplanes"] == 2 == L.BATCH_MAX_PLANES
    # what stays: the old struct (six int32, nine pointers), its LUT bound, the ABI version
    assert got["oldsize"] == C.sizeof(L.BatchArgs) == 6 * 4 + 9 * 8
    assert got["maxluts"] == L.BATCH_MAX_LUTS == 4
    assert got["version"] == 203 == L.ABI_VERSION
    # every field of mtbc_batch_args is in the new struct
    assert {n for n, _ in L.BatchArgs._fields_} | {"E", "planes"} == {n for n, _ in L.BatchPlanesArgs._fields_}
    lib = _lib()
    assert "mtbc_batch_assemble_planes" in L.EXPORTS and hasattr(lib, "mtbc_batch_assemble_planes")
    assert lib.mtbc_version() == 203


def _args(**kw):
    """test_batch_assemble_refuses_bad_arguments_on_the_host's dummy arguments, E = 0."""
    a = L.BatchPlanesArgs()
    a.M, a.N, a.H, a.W, a.K, a.n_onehot, a.E = 4, 2, 8, 8, 0, 3, 0
    a.images, a.masks, a.labels, a.index = 0x10000, 0x20000, 0x30000, 0x40000
    a.out_image, a.out_mask, a.out_target = 0x100000, 0x200000, 0x300000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_batch_assemble_planes_refuses_what_batch_assemble_refuses():
    """Every case of test_batch_assemble_refuses_bad_arguments_on_the_host, the same codes, with E = 0 and with E = 2."""
    lib = _lib()
    for extra in ({}, {"E": 2, "planes": 0x50000}):
        for kw in ({"K": 5}, {"K": -1}, {"n_onehot": 2}, {"n_onehot": 1}, {"N": 0}, {"M": 0}, {"H": 0}, {"W": -3}):
            assert lib.mtbc_batch_assemble_planes(C.byref(_args(**extra, **kw)), None) == BADSHAPE, (extra, kw)
        for kw in ({"images": None}, {"index": None}, {"out_target": None}, {"K": 2}, {"out_mask": 0x100000}, {"out_image": 0x10000},
                   {"out_target": 0x200000 + 16}):
            assert lib.mtbc_batch_assemble_planes(C.byref(_args(**extra, **kw)), None) == BADARG, (extra, kw)
    assert lib.mtbc_batch_assemble_planes(None, None) == BADARG


def test_batch_assemble_planes_refuses_bad_planes_on_the_host():
    lib = _lib()
    call = lambda **kw: lib.mtbc_batch_assemble_planes(C.byref(_args(**kw)), None)      # noqa: E731
    for E in (-1, 3, 100):
        assert call(E=E, planes=0x50000) == BADSHAPE, E
    assert call(E=3, planes=None, images=None) == BADSHAPE             # shapes first, then pointers
    for E in (1, 2):
        assert call(E=E, planes=None) == BADARG, E
    # the store is E * M * H * W = E * 256 bytes; out_image 2 * (1 + E) * 64 * 4, out_mask 2 * 64 * 4, out_target 2 * 3 * 4 bytes
    for E in (1, 2):
        store = E * 4 * 64
        assert call(E=E, planes=0x100000) == BADARG                    # on out_image
        assert call(E=E, planes=0x100000 + 2 * (1 + E) * 256 - 1) == BADARG    # its last byte
        assert call(E=E, planes=0x100000 - store + 1) == BADARG        # the store's last byte on its first
        assert call(E=E, planes=0x200000 + 8) == BADARG                # inside out_mask
        assert call(E=E, planes=0x300000 - store + 1) == BADARG        # the store's last byte on out_target's first
        assert call(E=E, planes=0x300000 + 23) == BADARG               # out_target's last byte
    # E = 2: the SECOND plane alone reaches the output (every call of this test is one the host refuses: nothing is launched)
    assert call(E=2, planes=0x100000 - 2 * 256 + 1) == BADARG
    # with E == 0 the pointer is not looked at
    assert call(E=0, planes=0x100000, N=0) == BADSHAPE


IMG = np.zeros((3, 8, 8), dtype=np.uint8)
LAB = np.array([0, 1, 2])


@pytest.mark.parametrize("aug,planes", [
    ({"CLAHE": True}, None),                                             # flag without plane (the existing test's call)
    ({"CLAHE": True}, {}),
    ({"CLAHE": True, "SOBEL": True}, {"CLAHE": IMG}),
    ({"SOBEL": True}, {"CLAHE": IMG}),
    (None, {"CLAHE": IMG}),                                              # plane without flag
    ({"CLAHE": False}, {"CLAHE": IMG}),
    ({"CLAHE": True, "brightness_darker": True}, {"CLAHE": IMG, "SOBEL": IMG}),
    ({"CLAHE": True}, {"CLAHE": IMG.astype(np.float32)}),               # wrong dtype
    ({"SOBEL": True}, {"SOBEL": IMG.astype(np.int8)}),
    ({"CLAHE": True}, {"CLAHE": IMG[:2]}),                               # wrong shape
    ({"SOBEL": True}, {"SOBEL": IMG[:, :, :4]}),
    ({"SOBEL": True}, {"SOBEL": IMG[0]}),
    ({"CLAHE": True}, {"CLAHE": IMG, "LAPLACE": IMG}),                   # unknown keys
    ({"brightness_darker": True}, {"brightness_darker": IMG}),
    ({"CLAHE": True, "GAMMA": True}, {"CLAHE": IMG}),
])
def test_constructor_refuses_before_it_needs_a_gpu(aug, planes, monkeypatch):
    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were validated")
    monkeypatch.setattr(L, "require_gpu", no_gpu)
    with pytest.raises(ValueError):
        DD.DeviceDataset(IMG, IMG, LAB, augmentation=aug, spatial_planes=planes)


def test_valid_planes_reach_the_gpu_check(monkeypatch):
    """The counterpart: valid planes (numpy or torch, host) pass every check, and the next thing the constructor does is ask for the GPU."""
    import torch

    class Reached(Exception):
        pass

    def stop():
        raise Reached()
    monkeypatch.setattr(L, "require_gpu", stop)
    with pytest.raises(Reached):
        DD.DeviceDataset(IMG, IMG, LAB, augmentation={"CLAHE": True, "SOBEL": True, "contrast_low": True},
                         spatial_planes={"SOBEL": torch.from_numpy(IMG), "CLAHE": IMG})
    with pytest.raises(Reached):
        DD.DeviceDataset(IMG, IMG, LAB, augmentation={"CLAHE": False, "contrast_low": True}, spatial_planes={})


def test_intensity_luts_still_refuses_the_spatial_keys():
    for key in DD.SPATIAL_KEYS:
        with pytest.raises(ValueError):
            DD.intensity_luts({key: True})


def test_channel_order_is_the_reference_append_order_for_every_subset():
    seen = 0
    for r in range(len(REFERENCE_ORDER) + 1):
        for on in itertools.combinations(REFERENCE_ORDER, r):
            want = ("image",) + tuple(k for k in REFERENCE_ORDER if k in on)
            # the dict's own order must not matter, nor flags that are present and off
            aug = {k: k in on for k in reversed(REFERENCE_ORDER)}
            assert DD.channel_names(aug) == want, on
            assert DD.channel_names({k: True for k in on}) == want, on
            # the LUT rows behind the names are the intensity_luts rows of the LUT keys alone
            luts = DD.intensity_luts({k: True for k in on if k in DD.LUT_KEYS})
            assert 1 + sum(k in DD.SPATIAL_KEYS for k in on) + len(luts) == len(want)
            seen += 1
    assert seen == 64
    assert DD.channel_names(None) == ("image",)
    assert DD.SPATIAL_KEYS + DD.LUT_KEYS == tuple(REFERENCE_ORDER)
    with pytest.raises(ValueError):
        DD.channel_names({"GAMMA": True})
