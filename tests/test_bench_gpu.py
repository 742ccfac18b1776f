"""bench.py on the GPU: a plain run measures the headline only, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_reports_the_headline_and_dumps_its_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["dtype"] == "bf16" and out["ms_per_step"] > 0
    assert abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]
    for key in ("fp32_parity_mode", "cpu_baseline", "roofline", "roofline_hbm"):     # --full only
        assert key not in out

    files = sorted(os.listdir(tmp_path))
    assert files == ["cls_logits.npy", "grads.npy", "losses.npy", "params.npy", "seg_logits.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 2 ** 20
    got = {f[:-4]: np.load(tmp_path / f) for f in files}
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got["losses"].shape == (4,) and got["losses"][3] == 0.0
    assert abs(float(got["losses"][0]) - out["final_loss"]) < 1e-5
    assert got["cls_logits"].shape == (32, 3) and got["seg_logits"].shape == (32, 1, 256, 256)
    assert got["params"].ndim == 1 and np.abs(got["grads"]).max() > 0
