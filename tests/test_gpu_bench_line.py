"""bench.py's plain and --full result lines on a GPU, at C4's layer dims on a small batch (--rows).

A plain run prints the headline only and takes its dtype label from the dispatch rules; --full adds the profile-pass
figures and derives the label from the launch tags: both must say the same.  --dump-outputs writes the last timed
update's outputs, identical from run to run (seeded inputs, deterministic kernels), so the two runs' files are
compared bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 20_000          # more than one workgroup tile, not a multiple of 256
FULL_ONLY = ("roofline", "update_roofline", "fvp", "alt_arithmetic", "cpu_baseline", "arithmetic", "timing")


def _run(tmp, name, *extra):
    out = tmp / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--rows", str(ROWS), "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_plain_and_full_lines_agree(gpu_available, tmp_path):
    plain, pdir = _run(tmp_path, "plain")
    full, fdir = _run(tmp_path, "full", "--full", "--no-cpu-baseline", "--no-alt")
    for d in (plain, full):
        assert d["metric"] == bench.METRIC and d["unit"] == "updates/s" and d["higher_is_better"] is True
        assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["n_states"] == ROWS
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in plain]
    assert all(k in full for k in FULL_ONLY)
    assert plain["dtype"] == full["dtype"] == "fp32 (f16x3 split)"
    assert plain["last_update"] == full["last_update"]
    P = plain["config"]["num_params"]
    for name in bench.OUTPUT_VECTORS:
        a, b = np.load(pdir / f"{name}.npy"), np.load(fdir / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (P,) and np.isfinite(a).all() and np.any(a != 0)
        np.testing.assert_array_equal(a, b, err_msg=name)
    s = np.load(pdir / "stats.npy")
    assert s.dtype == np.float64 and s.shape == (len(bench.DIGEST_STATS),)
    np.testing.assert_array_equal(s, np.load(fdir / "stats.npy"))
    assert s[bench.DIGEST_STATS.index("cg_iters")] == 10 == plain["last_update"]["cg_iters"]
    assert sorted(os.listdir(pdir)) == sorted(f"{n}.npy" for n in (*bench.OUTPUT_VECTORS, "stats"))
