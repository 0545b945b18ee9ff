"""Log minibatches (include/mmg.h: run_all_steps == 3; Game.train_step(full_tape=True), mmg_dp_train_step(full_tape=1)).
Every number of a training log comes from one: every sample runs all T steps so that the tape holds the whole conversation,
while the baselines and the update are the training step's.  Until now they were compared with themselves only.

  * against the CPU oracle (run-all, injected uniforms as common.hip_train_case): every per-step array of exchange() through
    common.assert_parity -- bs / br excepted, which mode 3 defines on the live rows only -- and losses, gradients and
    updated parameters through the same gate;
  * against run_all_steps == 1 and the fused step from the same start: messages, stop bits and masks bit-identical to mode 1,
    class logits within the forward gate, and parameters, gradient norms and losses within rounding (rtol 2e-4, atol 2e-6,
    as test_hip_parity.py: test_early_exit_and_fused_step_equal_run_all); the same for mmg_dp_train_step(full_tape=1,
    reduce=0).
Cases: g2 (Adaptive, the register-resident path, where mode 3 has its own tape_all branch), g5_one_active, g3_fixed_c3shard
(Fixed: mode 1 inside) and a many-class binary shape (k_conversation_mc: mode 1 inside)."""
import numpy as np
import pytest

from tests import common
from tests.test_hip_configs import C1, _meta

pytestmark = pytest.mark.gpu

CASES = ["g2_adaptive_c1", "g5_one_active", "g3_fixed_c3shard", "mc_D200"]
PER_STEP = (".s_masks", ".s_feats", ".s_probs", ".sen_feats", ".sen_probs", ".rec_feats", ".rec_probs", ".y")
TRAIN = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")


def _case(name):
    if name == "mc_D200":
        return None, _meta(dict(C1, batch_size=40), 200, 40, 2)
    return name, common.load_golden(name)[1]


def _skip(meta):
    return ("y2.bias", ".bs", ".br")


@pytest.mark.parametrize("name", CASES)
def test_log_minibatch_vs_oracle(name):
    case, meta = _case(name)
    got, eng = common.hip_train_case(case, meta, log_tape=True)
    flips = []
    want = common.oracle_train_case(case, meta, flips=flips)
    assert any(k.endswith(".y") for k in got) and any(".g." in k for k in got)
    common.assert_parity(got, want, flips, eng, "log-" + name, skip=_skip(meta))


@pytest.mark.parametrize("name", CASES)
def test_log_minibatch_equals_run_all_and_fused(name):
    case, meta = _case(name)
    log, _ = common.hip_train_case(case, meta, log_tape=True)
    full, _ = common.hip_train_case(case, meta)                           # run_all_steps == 1
    fused, _ = common.hip_train_case(case, meta, fused=True)
    dp, _ = common.hip_train_case(case, meta, dp_full_tape=True)
    for i in range(meta["n_minibatches"]):
        p = "mb%d." % i
        # the same start (mb0): the conversation's discrete outcome and logits of mode 3 are mode 1's; later minibatches
        # start from parameters that differ by rounding, so only mb0's discrete arrays are required to be identical
        if i == 0:
            for k in ("s_masks", "s_feats", "sen_feats", "rec_feats", "n_steps", "hits"):
                for other, what in ((full, "run-all"), (dp, "dp full_tape")):
                    np.testing.assert_array_equal(log[p + k], other[p + k], err_msg="%s%s vs %s" % (p, k, what))
            for k in ("y", "outp", "dist", "s_probs", "sen_probs", "rec_probs", "logs"):
                if log[p + k].size:
                    np.testing.assert_allclose(log[p + k], full[p + k], rtol=0, atol=1e-4, err_msg=p + k)
                    np.testing.assert_allclose(log[p + k], dp[p + k], rtol=0, atol=1e-4, err_msg=p + k + " dp")
        keys = [k for k in log if k.startswith(p) and (".g." in k or ".p." in k or k.endswith("losses") or "gradnorm" in k)
                and "y2.bias" not in k]                     # y2.bias: see common.compare_packed
        assert keys
        for k in keys:
            for other, what in ((full, "run-all"), (fused, "fused"), (dp, "dp full_tape")):
                np.testing.assert_allclose(log[k], other[k], rtol=2e-4, atol=2e-6, err_msg="%s vs %s" % (k, what))
