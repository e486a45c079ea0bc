"""GPU: a plain `bench.py --gpus 1` run end to end -- one JSON line with the contract's fields, nothing of what only --full measures, and
--dump-outputs writing the last timed step's outputs, identical in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_reproducible_dump(tmp_path):
    out = _run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 16 / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]      # 8 + 8 images per Mean-Teacher step
    assert out["dtype"].startswith("bf16x3") and out["config"]["hipgraph"] is True
    assert out["blocks"]["ms_per_step"] == [out["ms_per_step"]]
    assert out["cpu_baseline"] is None and out["f32_math"] is None and out["other_bn_mode"] is None
    files = sorted(os.listdir(tmp_path / "a"))
    assert "step.loss.npy" in files and any(f.startswith("model0.") for f in files) and any(f.startswith("model1.") for f in files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6 + 4096 * len(files)
    for f in files:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    _run(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == files
    diff = [f for f in files if not np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))]
    assert not diff, diff
