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
