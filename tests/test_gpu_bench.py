"""bench.py on the device: a plain run reports the headline alone, and `--full` adds its other legs to the line without changing the
timed iterations (same chain, same counters, same dumped outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "roofline_hmc", "cpu_baseline", "gradient_modes_same_iterations", "per_chain_hmc_mode1", "per_chain_hmc_mode1_headline_window")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--burn-in", "30", "--n", "5000", "--p", "10",
           "--trees", "20", "--dump-outputs", str(out_dir), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_full_adds_legs_not_iterations(tmp_path):
    plain = _bench(tmp_path / "plain")
    full = _bench(tmp_path / "full", "--full", "--no-extra-configs", "--target-n", "0", "--mode-iters", "10", "--cpu-iters", "2")
    for k in FULL_ONLY:
        assert k not in plain and k in full, k
    assert "stationarity" not in plain["config"] and "stationarity" in full["config"]
    assert full["cpu_baseline"]["same_chain_as_the_gpu"]["first_iteration_tree_moves_identical"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    for k in ("tree_path", "hmc_mode", "n_leapfrog_timed", "gradient_evals_timed", "tree_updates_timed", "sigma_last"):
        assert plain["config"][k] == full["config"][k], k
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and sorted(os.listdir(tmp_path / "full")) == names
    for name in names:
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)), name
