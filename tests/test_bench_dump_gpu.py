"""bench.py at N = 1: a plain run measures the headline only, `--full` adds the other legs, and `--dump-outputs` writes
the last timed step's outputs from identical seeded inputs run after run (a tiny config, so each run takes seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("pooler_output", "loss", "last_hidden_state_rows", "grad_norms", "grad_sample")


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "hostile", "--batch", "3"]
    r = subprocess.run(cmd + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    dumps = []
    for steps in (3, 1):
        d = tmp_path / f"steps{steps}"
        line = run_bench("--steps", str(steps), "--warmup", "1", "--dump-outputs", str(d))
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "images/sec"
        assert abs(line["value"] - 3 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        for leg in ("roofline", "step_breakdown", "secondary", "optimizer_step", "train_step_with_optimizer",
                    "cpu_baseline", "tolerance", "leg_errors"):
            assert leg not in line, leg
        arrs = {n: np.load(d / f"{n}.npy") for n in DUMPED}
        assert sorted(os.listdir(d)) == sorted(f"{n}.npy" for n in DUMPED)
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["pooler_output"].shape == (3, 144) and arrs["pooler_output"].dtype == np.float32
        assert arrs["loss"].dtype == np.float64 and arrs["grad_norms"].dtype == np.float64
        assert all(np.isfinite(a).all() for a in arrs.values())
        assert np.isclose(arrs["loss"], np.square(arrs["pooler_output"].astype(np.float64)).mean(), rtol=1e-2)
        dumps.append(arrs)
    # same arguments up to --steps: same inputs, so the same outputs up to the split-K atomics' summation order
    for n in DUMPED:
        a, b = dumps[0][n], dumps[1][n]
        assert a.shape == b.shape, n
        assert np.abs(a - b).max() <= 2e-2 * max(np.abs(a).max(), 1e-6), n


def test_full_run_adds_the_other_legs():
    line = run_bench("--steps", "2", "--warmup", "1", "--full", "--kernel-reps", "2", "--cpu-steps", "1",
                     "--train-steps", "2")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert "leg_errors" not in line, line.get("leg_errors")
    for leg in ("roofline", "step_breakdown", "optimizer_step", "train_step_with_optimizer", "cpu_baseline",
                "tolerance"):
        assert leg in line, leg
