"""mtbc_fill_holes on the GPU against its host twin and scipy.ndimage.binary_fill_holes, bit for bit, on the cases of
tests/test_fill_holes_cpu.py and the sizes only the device reaches; FusedSegTestStep against the reference's recorded testing phase
(tests/golden/seg_test_metrics.npz)."""
import csv
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import binary_fill_holes

pytestmark = pytest.mark.gpu

from multi_task_breast_cancer_amd import _lib as L  # noqa: E402
from multi_task_breast_cancer_amd import inference as I  # noqa: E402
from test_fill_holes_cpu import CASES, assert_filled, logits_of, passes_needed, random_mask, run_host, spiral  # noqa: E402
from test_test_metrics_cpu import assert_columns_equal  # noqa: E402

DEV = torch.device("cuda:0")


def run_device(x: np.ndarray):
    """(N, H, W) fp32 logits -> (filled_logits, filled_u8, error word) of mtbc_fill_holes."""
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out_f, out_u8 = I.fill_holes(torch.from_numpy(np.ascontiguousarray(x, np.float32))[:, None].to(DEV), err, want_logits=True, want_u8=True)
    return out_f[:, 0].cpu().numpy(), out_u8.cpu().numpy(), int(err.item())


def check(x: np.ndarray, fg: np.ndarray, name=""):
    out_f, out_u8, err = run_device(x)
    assert err == 0, name
    host_f, host_u8, host_err = run_host(L.load(), x)
    assert host_err == 0
    want = np.stack([binary_fill_holes(m) for m in fg])
    assert_filled(out_f, out_u8, want, name)
    assert np.array_equal(out_f, host_f) and np.array_equal(out_u8, host_u8), name


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_and_scipy(name):
    fg = CASES[name][None]
    check(logits_of(fg), fg, name)


def test_nan_logit_is_not_foreground():
    fg = CASES["ring"].copy()
    x = logits_of(fg)
    x[5, 10] = np.nan
    fg[5, 10] = False
    check(x[None], fg[None])


def test_three_different_images_one_workgroup_each():
    fg = np.stack([CASES[n] for n in ("nested_rings", "all_zero", "diagonal_ring")])
    check(logits_of(fg), fg)
    fg = np.stack([random_mask(64, 64, d, 7 + k) for k, d in enumerate((0.3, 0.5, 0.7))])
    check(logits_of(fg), fg)


def test_128_random_and_the_512_spiral():
    fg = random_mask(128, 128, 0.5, 128)[None]
    check(logits_of(fg), fg, "random 128")
    sp = spiral(512)                                 # the largest LDS footprint, 255 passes of the repeat-until-stable loop
    out_f, out_u8, err = run_device(logits_of(sp[None]))
    assert err == 0
    assert_filled(out_f[0], out_u8[0], binary_fill_holes(sp), "spiral 512")
    assert np.array_equal(out_u8[0] != 0, sp)        # its corridor is open to the border: nothing is a hole
    fg = random_mask(512, 512, 0.55, 512)[None]      # ... and one 512 x 512 mask that does have holes, against the host twin too
    check(logits_of(fg), fg, "random 512")
    assert passes_needed(spiral(64)) == 31           # (the count the docstring of `spiral` states, at the size that is cheap to restate)


def test_single_outputs_and_refusals():
    fg = CASES["ring"][None]
    x = torch.from_numpy(logits_of(fg))[:, None].to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    f, u = I.fill_holes(x, err, want_logits=True, want_u8=False)
    assert u is None and np.array_equal(f[0, 0].cpu().numpy() > 0, binary_fill_holes(fg[0]))
    f, u = I.fill_holes(x, err, want_logits=False, want_u8=True)
    assert f is None and np.array_equal(u[0].cpu().numpy() != 0, binary_fill_holes(fg[0]))
    assert int(err.item()) == 0
    with pytest.raises(L.MtbcError):
        I.fill_holes(torch.zeros(1, 1, 40, 40, device=DEV), err)
    with pytest.raises(L.MtbcError):
        I.fill_holes(torch.zeros(1, 1, 32, 32), torch.zeros(1, dtype=torch.int32))          # CPU tensors: no fallback


# ------------------------------------------------------------------------------------------------ the testing phase
@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "seg_test_metrics.npz"))


def _feed(step, g, batch=5):
    x, t = torch.from_numpy(g["logits"])[:, None].to(DEV), torch.from_numpy(g["masks"].astype(np.float32))[:, None].to(DEV)
    names = [str(n) for n in g["names"]]
    for i in range(0, len(names), batch):            # 5 + 5 + 2: batches of two sizes
        step.evaluate_logits(x[i:i + batch], t[i:i + batch], patient_id=list(range(i, min(i + batch, len(names)))), class_name=names[i:i + batch])
    return names


def test_seg_test_step_equals_the_references_testing_phase(fixture, tmp_path):
    g = fixture
    step = I.FusedSegTestStep(model=None, fill_holes=True, keep_masks=True)
    names = _feed(step, g)
    rows = step.result()
    assert [r["class"] for r in rows] == names and [r["patient_id"] for r in rows] == list(range(len(names)))
    got = {c: np.array([r[c] for r in rows]) for c in I.SEG_METRIC_COLUMNS}
    assert_columns_equal(got, g["metrics"], g["columns"])                     # the reference's seven columns, bit for bit, NaN positions included
    assert np.isnan(g["metrics"]).any() and (g["metrics"][:, 1] == 1.0).sum() >= 5       # the fixture does exercise both
    masks = step.masks_u8()
    assert len(masks) == len(names) and all(m.dtype == np.uint8 and m.shape == (32, 32) for m in masks)
    assert set(np.unique(np.stack(masks))) <= {0, 255}
    assert np.array_equal(np.stack(masks) != 0, g["filled"] != 0)
    assert np.array_equal(g["filled"] != 0, np.stack([binary_fill_holes(x > 0) for x in g["logits"]]))
    assert abs(step.mean_dice() - float(np.mean(g["metrics"][:, 1]))) < 1e-15
    file = step.write_csv(str(tmp_path / "fold_0"))
    assert os.path.basename(file) == "results_segmentation.csv" and os.listdir(tmp_path / "fold_0") == ["results_segmentation.csv"]
    with open(file, newline="") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == I.SEG_CSV_COLUMNS and len(lines) == 1 + len(names)
    assert lines[1][lines[0].index("DICE")] == "1.0" and lines[4][lines[0].index("Sensitivity")] == ""      # NaN as pandas writes it


def test_without_filling_the_step_is_seg_metrics_alone(fixture):
    g = fixture
    step = I.FusedSegTestStep(model=None, fill_holes=False, keep_masks=True)
    _feed(step, g)
    step.result()
    x, t = torch.from_numpy(g["logits"])[:, None].to(DEV), torch.from_numpy(g["masks"].astype(np.float32))[:, None].to(DEV)
    assert np.array_equal(step.table, I.seg_metrics(x, t).cpu().numpy())
    assert np.array_equal(np.stack(step.masks_u8()) != 0, g["logits"] > 0)
    filled = I.FusedSegTestStep(model=None, fill_holes=True)
    _feed(filled, g)
    filled.result()
    assert not np.array_equal(filled.table, step.table)                       # the fixture's holes do change the table
    with pytest.raises(ValueError):
        filled.masks_u8()


def test_seg_test_step_on_the_model():
    """pack + fwd + fill + metrics on a real forward: the rows equal scipy + the table of the same logits."""
    from multi_task_breast_cancer_amd.miscellany import seed_everything
    from multi_task_breast_cancer_amd.nets import nnUNet
    from oracle import torch_oracle as O
    seed_everything(1993)
    m = nnUNet(1, 1).to(DEV)
    img, mask, _ = O.synthetic_batch(2, 64, 64, seed=3)
    step = I.FusedSegTestStep(m, keep_masks=True)
    step(img.to(DEV), mask.to(DEV), class_name=["benign", "malignant"])
    rows = step.result()
    with torch.no_grad():
        logits = m(img.to(DEV))[-1]
    want = np.stack([binary_fill_holes(x) for x in (torch.sigmoid(logits[:, 0]) > .5).cpu().numpy()])
    assert np.array_equal(np.stack(step.masks_u8()) != 0, want)
    t = I.seg_metrics(torch.from_numpy(np.where(want, 1.0, -1.0).astype(np.float32))[:, None].to(DEV), mask.to(DEV)).cpu().numpy()
    assert np.array_equal(step.table, t) and [r["class"] for r in rows] == ["benign", "malignant"]
