"""bench.py's command line: a plain run measures the headline only, `--full` adds the rest, and
`--dump-outputs DIR` writes what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default_and_steps_must_be_positive():
  a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
  assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
  a = bench.parse_args(["--full", "--dump-outputs", "out"])
  assert a.full and a.dump_outputs == "out"
  for bad in ("0", "-1"):
    with pytest.raises(SystemExit):
      bench.parse_args(["--steps", bad])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_sample(tmp_path):
  out = tmp_path / "outputs"
  r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                      "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
  assert r.returncode == 0, r.stderr[-3000:]
  lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
  assert len(lines) == 1, r.stdout
  d = json.loads(lines[0])
  assert d["metric"] == "denoiser-calls/sec" and d["unit"] == "calls/s" and d["higher_is_better"] is True
  assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
  assert abs(d["value"] - 1e3 * bench.CALLS_PER_STEP / d["ms_per_step"]) < 0.01 * d["value"]
  assert d["roofline"] is None and d["cpu_baseline"] is None and d["one_degree"] is None
  smp = np.load(out / "sample.npy")
  assert smp.dtype == np.float32
  assert smp.shape == (d["config"]["grid_nodes"], 1, d["config"]["c_out"])
  assert np.isfinite(smp).all() and np.abs(smp).max() > 0
