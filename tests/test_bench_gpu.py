"""bench.py on the GPU: --steps sets the timed minibatches and --dump-outputs writes what the last of them computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dumps_the_outputs_of_the_timed_steps(tmp_path):
    out = tmp_path / "dump"
    env = dict(os.environ, MMG_BENCH_MIN_SECONDS="0.2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "5", "--warmup", "2", "--no-other-configs",
                        "--no-cli", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 5 and d["config"]["timed_minibatches"] == 5 and d["ms_per_step"] > 0
    assert abs(d["ms_per_step"] - 1e3 * d["config"]["timed_seconds"] / 5) < 1e-9
    arrs = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(arrs) == {"params", "grads", "opt_state", "losses"}
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    for name, a in arrs.items():
        assert a.dtype in (np.float32, np.float64) and a.size == d["dump_outputs"]["entries"][name] and np.isfinite(a).all(), name
    assert arrs["params"].size == arrs["grads"].size == arrs["opt_state"].size // 2
    assert arrs["losses"].size == 8 and arrs["losses"][6] >= 1          # n_steps of the last timed minibatch
    assert np.abs(arrs["params"]).max() > 0 and np.abs(arrs["opt_state"]).max() > 0   # trained state, not zeros


@pytest.mark.gpu
def test_full_adds_passes_after_the_same_timed_steps(tmp_path):
    """A plain run and a --full run time the same steps from the same point and dump the same outputs; only the --full line
    carries the window and the roofline, which it measures after them."""
    env = dict(os.environ, MMG_BENCH_MIN_SECONDS="0.2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    lines, dumps = {}, {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-other-configs", "--no-cli", "--no-cpu-baseline"])):
        out = tmp_path / mode
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "5", "--warmup", "2", "--dump-outputs", str(out)] + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (mode, p.stderr[-2000:])
        lines[mode] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        dumps[mode] = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    plain, full = lines["plain"], lines["full"]
    assert plain["full"] is False and full["full"] is True
    assert "value_window" not in plain and "roofline" not in plain and "window" not in plain["config"]
    assert full["value_window"] > 0 and full["config"]["window"]["minibatches"] >= 5 and full["roofline"]["kernels_us"]
    assert plain["config"]["exchange_steps_per_minibatch"] == full["config"]["exchange_steps_per_minibatch"]
    assert set(dumps["plain"]) == set(dumps["full"]) == {"params", "grads", "opt_state", "losses"}
    for name, a in dumps["plain"].items():
        np.testing.assert_allclose(a, dumps["full"][name], rtol=1e-5, atol=1e-7, err_msg=name)
