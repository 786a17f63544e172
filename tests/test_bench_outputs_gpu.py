"""bench.py's plain run (no --full) and --dump-outputs: the line holds the headline fields and none of the --full objects,
--steps is the number of timed steps, and the arrays the last timed step returned land as float32 / float64 .npy files
within the 64 MB budget, the same from run to run (seeded inputs).  Small batch (the "plumbing" configuration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_mfma", "roofline_att_bwd", "precision_modes", "extra_workloads", "cpu_baseline")


def _plain_run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--config", "plumbing", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_dumps_the_last_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _plain_run(a, 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert not [k for k in FULL_ONLY if k in d], "a plain run measures only the headline"
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    got = _load(a)
    assert "losses" in got and "logit" in got, sorted(got)
    assert sum(x.nbytes for x in got.values()) <= 64 * 1000 * 1000
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert got["losses"].dtype == np.float64 and got["losses"].shape == (4,)
    assert abs(float(got["losses"].sum()) - d["loss"]) <= 1e-9 * abs(d["loss"])
    assert got["logit"].size == 64 * 5 and np.isfinite(got["logit"]).all()
    # same arguments, same inputs: a second run computes the same arrays
    _plain_run(b, 3)
    again = _load(b)
    assert sorted(again) == sorted(got)
    for k in got:
        assert again[k].shape == got[k].shape, k
        np.testing.assert_allclose(again[k], got[k], rtol=1e-5, atol=1e-6, err_msg=k)
