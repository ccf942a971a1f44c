"""bench.py's plain run and --dump-outputs, for every config at a small size: the plain line carries the headline fields and
none of what --full adds, --steps sets the number of timed steps, and two runs with the same arguments write the same
outputs (float32, under the 64 MB limit), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SMALL = {"kalman4": ["--batch", "4096", "--T", "400"], "gsf32": ["--batch", "512", "--T", "100", "--chunk", "50"],
         "bpf4096": ["--batch", "32", "--T", "20"], "kalman64": ["--batch", "512", "--T", "200"]}
FULL5 = {"weights", "means", "covariances", "predicted_means", "predicted_covariances"}
CARRY = {"carry_weights", "carry_means", "carry_covariances"}
NAMES = {"kalman4": FULL5, "gsf32": FULL5 | CARRY, "kalman64": FULL5 | CARRY, "bpf4096": {"mean", "ess", "logz", "resampled"}}


def _run(config, out_dir):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", config,
           "--dump-outputs", str(out_dir)] + SMALL[config]
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-4000:])
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(SMALL))
def test_bench_plain_line_and_dump_outputs(config, tmp_path):
    d = _run(config, tmp_path / "a")
    assert d["metric"] == "filter timesteps/sec (batch x T)" and d["unit"] == "timesteps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not {"finite_frac", "roofline", "cpu_baseline"} & set(d)
    a = _load(tmp_path / "a")
    assert set(a) == NAMES[config]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES
    _run(config, tmp_path / "b")
    b = _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_sample_idx_is_fixed_and_keeps_the_last_index():
    i = bench.sample_idx(10000, 256)
    assert len(i) == 256 and i[-1] == 9999 and np.all(np.diff(i) > 0)
    assert np.array_equal(i, bench.sample_idx(10000, 256))
    assert np.array_equal(bench.sample_idx(20, 256), np.arange(20))
