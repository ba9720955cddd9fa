"""bench.py command line: result-line fields, --steps, --full and
--dump-outputs (CPU, llama-tiny; the child never opens a GPU)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent
STEPS = 2


def _run_bench(out_dir, *extra):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["PYTHONPATH"] = str(REPO_ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, str(REPO_ROOT / "bench.py"), "--gpus", "1",
           "--steps", str(STEPS), "--warmup", "1", "--model", "llama-tiny",
           "--layers-per-stage", "2", "--seq-len", "32", "--gas", "2",
           "--micro-batch-size", "2", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=REPO_ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    a = tmp_path_factory.mktemp("dump_a")
    b = tmp_path_factory.mktemp("dump_b")
    return (_run_bench(a), a), (_run_bench(b, "--full"), b)


def test_result_line_fields(runs):
    for res, _ in runs:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in res
        assert res["steps"] == STEPS
        assert res["unit"] == "tokens/s" and res["higher_is_better"] is True
        assert res["ms_per_step"] > 0
        tokens_per_step = res["config"]["global_batch"] * res["config"]["seq_len"]
        assert res["value"] == pytest.approx(tokens_per_step / (res["ms_per_step"] / 1e3), rel=1e-2)


def test_dump_outputs_written_and_reproducible(runs):
    (res_a, dir_a), (_, dir_b) = runs
    names = sorted(p.name for p in dir_a.glob("*.npy"))
    assert names == ["grad_moment_sample.npy", "loss.npy", "params_sample.npy", "step_losses.npy"]
    total = 0
    for name in names:
        a, b = np.load(dir_a / name), np.load(dir_b / name)
        assert a.dtype in (np.float32, np.float64)
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)  # same arguments -> same inputs -> same outputs
        total += a.nbytes
    assert total <= 64 * 2**20
    losses = np.load(dir_a / "step_losses.npy")
    assert losses.shape == (STEPS,)  # --steps really sets the timed steps
    assert np.load(dir_a / "loss.npy")[0] == losses[-1]
    assert losses[-1] == pytest.approx(res_a["config"]["last_loss"], abs=1e-4)
    assert np.abs(np.load(dir_a / "grad_moment_sample.npy")).max() > 0
