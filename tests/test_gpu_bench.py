"""A plain `bench.py --gpus 1` run on a GPU (config B, n=64, t=31, as a fresh child process): one
result line with the headline fields, none of the side measurements that --full adds, and
--dump-outputs writing the last timed step's result -- its mpk is g * sum_i a_i0 of the seeded
coefficients (computed here by the CPU oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import dkg_amd
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "B", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dumped_outputs(tmp_path):
    n, t = bench.CONFIGS["B"]
    out, arrs = _run(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "verified shares/s" and out["higher_is_better"] is True and out["dtype"].startswith("u32")
    assert f"n={n},t={t}" in out["metric"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n * (n - 1) / (out["ms_per_step"] / 1e3), rel=1e-6)
    for k in ("roofline", "cpu_baseline", "gpu_vs_cpu", "interp_mode", "sclk_mhz", "checks_serialised_ms"):
        assert k not in out, k  # behind --full
    assert all(a.dtype == np.float32 for a in arrs.values())
    a, _ = dkg_amd.dealer_coefficients(b"\xbe" * 32, 0, 0, n, t)  # bench.py's master seed
    N = t + 1
    secret = sum(int.from_bytes(a[32 * N * i:32 * N * i + 32], "little") for i in range(n)) % bench.L
    assert bytes(arrs["mpk"].astype(np.uint8)) == O.base_mul(secret.to_bytes(32, "little"))
    assert arrs["n_qualified"].tolist() == [n] and arrs["qualified"].tolist() == [1.0] * n
    assert not arrs["complaints2"].any() and not arrs["reconstruct"].any() and not arrs["phase4_error"].any()
