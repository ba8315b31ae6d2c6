"""bench.py on the GPU: a plain run times the headline alone and prints the contract's keys; --dump-outputs writes what the last timed
step computed, the same from one run to the next (the inputs come from fixed seeds)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", *extra]
    out = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and out.stdout.rstrip().endswith(lines[0]), out.stdout
    return json.loads(lines[0])


def test_plain_run_and_its_dumped_outputs(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config"):
        assert key in a, key
    assert a["steps"] == 3 and a["warmup"] == 1 and a["n_gpus"] == 1 and a["unit"] == "postage-stamps/s" and a["dtype"] == "f64"
    assert abs(a["value"] - 8 / (a["ms_per_step"] * 1e-3)) < 1e-6 * a["value"]
    for key in ("roofline", "cpu_baseline", "summary", "detail", "farm"):  # (the legs beyond the headline run with --full)
        assert key not in a, key
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "T_sample.npy" in names and "outimage.npy" in names
    total = 0
    for name in names:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), name
        tol = 1e-5 if x.dtype == np.float32 else 1e-10
        assert np.allclose(x, y, rtol=tol, atol=tol * np.abs(x).max()), (name, np.abs(x - y).max())
        total += (tmp_path / "a" / name).stat().st_size
    assert total < 64e6
    assert np.load(tmp_path / "a" / "outimage.npy").shape[0] == 8 and np.abs(np.load(tmp_path / "a" / "T_sample.npy")).max() > 0
