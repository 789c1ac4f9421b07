"""bench.py's command line: a plain run only times the steps (the roofline sweep and the CPU leg
come with --full), --dump-outputs writes what the last timed step computed, bounded in size and
identical run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("step_preds", "step_log_probas", "step_values", "step_pos", "step_actions", "scalars", "params", "grads")


def _bench(*args, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_dump_outputs_budget_and_sample(tmp_path):
    import bench

    arrays = {"big": th.arange(10000, dtype=th.float32), "ints": th.arange(300, dtype=th.int64),
              "small": th.ones(3, 2)}
    bench.dump_outputs(str(tmp_path / "a"), arrays, budget=8000)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert got["small"].dtype == np.float32 and got["small"].shape == (3, 2)
    assert got["ints"].dtype == np.float64 and np.array_equal(got["ints"], np.arange(300))
    big = got["big"]
    assert big.dtype == np.float32 and 0 < big.size < 10000
    assert sum(a.nbytes for a in got.values()) <= 8000
    assert np.all(np.diff(big) > 0) and np.all(big == np.round(big))  # sorted elements of the original
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=8000)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), big)  # the same sample every run
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), np.arange(10000))  # fits: written whole


def test_steps_must_be_positive():
    r = _bench("--steps", "0", timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(device, tmp_path):
    """Plain run: the headline fields, nothing from the --full legs; two runs with the same arguments
    dump the same outputs."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = _bench("--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["metric"] == "agent-env-steps/sec" and j["dtype"] == "f32" and j["higher_is_better"] is True
        assert j["roofline"] is None and j["cpu_baseline"] is None
        got = {k: np.load(d / f"{k}.npy") for k in OUTPUTS}
        assert sum(os.path.getsize(d / f"{k}.npy") for k in OUTPUTS) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert got["step_pos"].shape == (5, 3, 1024, 2) and got["step_preds"].shape == (5, 3, 1024, 10)
        assert all(np.isfinite(a).all() for a in got.values())
        dumps.append(got)
    for k in OUTPUTS:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
