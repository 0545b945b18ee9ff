"""CPU-only check of tests/wgrad_ref.py, the float64 restatement of k_wgrad's job table that tests/test_hip_wgrad.py gates
the GPU's weight gradients against: on the library's own parameter table, the restated jobs write every parameter float
exactly once (binary messages), or exactly the receiver's blocks that build_jobs writes (continuous messages: only the
receiver is trained, model.py:1313).  A job the restatement skipped or wrote twice would otherwise leave a block ungated."""
import pytest

from multimodalgame_amd import _lib
from tests import wgrad_ref

# (batch, n_classes, feat, H, W, R, V, K, T)
SHAPES = {
    "config2": (64, 30, 512, 256, 32, 64, 100, 500, 10),
    "config3_b512": (512, 30, 512, 256, 32, 64, 100, 500, 10),
    "config4": (64, 30, 512, 1024, 256, 64, 100, 500, 10),
    "config4_R256": (64, 30, 512, 1024, 256, 256, 100, 500, 10),
    "D1000": (256, 1000, 512, 256, 32, 64, 100, 500, 10),
}


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_restated_jobs_write_every_parameter_once(shape, binary):
    B, D, F, H, W, R, V, K, T = SHAPES[shape]
    cfg = _lib.make_config(B, D, F, H, W, R, V, K, T, use_binary=binary, fixed_exchange=not binary)
    table = _lib.param_table(cfg)
    d = wgrad_ref.dims_of(cfg)
    variants = ("fast", "tile", "generic") if binary else (None,)
    for variant in variants:
        jobs = wgrad_ref.build_jobs(d, table, variant)
        cnt = wgrad_ref.coverage(jobs, table, binary)
        for (agent, name), c in cnt.items():
            want = 1 if (binary or (agent == "receiver" and name not in wgrad_ref.RECEIVER_ONLY_BINARY)) else 0
            assert (c == want).all(), "%s %s variant %s: %s.%s written %s times" % (shape, binary, variant, agent, name,
                                                                                  sorted(set(c.reshape(-1).tolist())))
        for j in jobs:
            assert j.nsplit >= 1 and (j.nsplit == 1 or j.kind == "gemm"), j.label


def test_row_split_plan_matches_layout_arithmetic():
    """The split plan restated from layout.h for the shapes the GPU tests name (their docstrings quote these numbers)."""
    def plan(B, T, D=30, H=256, W=32, R=64, binary=True):
        cfg = _lib.make_config(B, D, 512, H, W, R, 100, 500, T, use_binary=binary, fixed_exchange=not binary)
        table = _lib.param_table(cfg)
        jobs = wgrad_ref.build_jobs(wgrad_ref.dims_of(cfg), table)
        return wgrad_ref.param_total(table), {j.label: (j.kind, j.nsplit) for j in jobs}, jobs[0].small_split
    ptotal, p, small = plan(64, 10)                                  # config 2: 640 rows, nothing split
    assert ptotal == 384192 and not small and all(ns == 1 for _, ns in p.values())
    ptotal, p, small = plan(512, 10)                                 # config 3 at 512 samples: 5 120 rows
    assert wgrad_ref.wgrad_nsplit(5120, ptotal) == 2 and not small
    assert p["receiver.rnn.weight_ih[0:192, 0:32]"] == ("gemm", 2)
    assert p["receiver.rnn.bias_ih[0:192, 0:1]"] == ("gemm", 2)      # bias columns as K = 1 GEMMs
    ptotal, p, small = plan(256, 10, D=1000, binary=False)           # config 5 shard: continuous, 2 560 rows
    assert small and p["receiver.rnn.weight_ih[0:192, 0:32]"] == ("gemm", 8)
    assert p["receiver.rnn.bias_hh[0:192, 0:1]"] == ("gemm", 8)
    ptotal, p, small = plan(2048, 3, D=1000, binary=False)           # config 5 at 2 048 samples, T = 3: 6 144 rows
    assert small and p["receiver.rnn.weight_hh[0:192, 0:64]"] == ("gemm", 16)
