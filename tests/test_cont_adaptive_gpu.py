"""Continuous messages with Adaptive stopping (-nouse_binary -model_type Adaptive) on every kernel family, against the CPU oracle.
The stop bit is sampled, samples leave the conversation at different steps, the reference breaks out of exchange() once all have
stopped (fewer executed steps than max_exchange) and `outp` is each sample's logits at its own stop step; only the receiver is
trained, through the NLL.  Every other continuous training case of the suite is Fixed.  tests/cont_adaptive.py holds the shapes and
seeds, tests/test_cont_adaptive_cpu.py shows on the oracle alone that these inputs reach those branches and that every shape
selects its family.

Gate: common.assert_parity with its defaults -- forward quantities 1e-4 absolute (config 4's agents: the six losses against the
float64 oracle, as every C4 case), masks / stop bits / n_steps / hits exact, gradients / parameters / gradient norms atol 1e-4 +
rtol 1e-3, a near-threshold ReLU unit only through the forced re-run.  "phased": forward(run_all) / loss_stats / backward /
clip_step with every per-step array compared; "fused": train_step, compared on what the lean tape keeps.

The rc case found a precision defect: unit 241 of its 256-unit y head is on for all 1 200 (sample, class) pairs of minibatch 0, so
the exact gradient of y1.bias[241] (and of its h-side weights) is w2 sum_b sum_d dy[b, d] = 0.  The wide-receiver tail formed the
softmax as exp(y - lse) with the fast logarithm, rows summed to 1 within ~1e-6 only, the gradient came out -2.7e-8 (oracle 2.5e-9),
RMSprop turned it into a step 2.39e-4 off (tolerance 1.6e-4) and minibatch 1's logits moved by 5.9e-4.  The tail now divides by
the row's own sum: -1.9e-9, the parameter 4.3e-5 off."""
import numpy as np
import pytest

from tests import common, cont_adaptive as ca
from tests.test_option_branches_gpu import FAMILIES, MODE_KW, _names, _pick

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,mode", [(k, m) for k, c in ca.CASES.items() for m in c["modes"]])
def test_continuous_adaptive_vs_oracle(case, mode, monkeypatch):
    c = ca.CASES[case]
    for sw in c["env"]:
        monkeypatch.setenv(sw, "1")
    name, meta, want, flips, params = ca.oracle(case)
    scopes = FAMILIES[c["scopes"]]
    n_mb = meta["n_minibatches"]
    got, eng = common.hip_train_case(name, meta, **MODE_KW[mode])
    label = "contadapt-%s-%s" % (case, mode)
    steps, hits = [int(got["mb%d.n_steps" % i]) for i in range(n_mb)], [int(got["mb%d.hits" % i]) for i in range(n_mb)]
    print(label, "n_steps", steps, "oracle", list(c["n_steps"]), "hits", hits, "losses", np.asarray(got["mb0.losses"]).round(4).tolist())
    if c.get("mc3p"):                               # the pair kernel must be the one that ran: a device whose caps say otherwise fails here
        assert "mc3p 1 wins 1" in eng.plan_text(), eng.plan_text()
    # a target logit tied to the bit in the oracle's own output (generic-tiny, test_only_the_tiny_agents_tie_a_target_logit): the
    # oracle's count is numpy's argsort order there; the library's rule on the oracle's values is the expected count
    tied = [i for i in range(n_mb) if ca.tied_targets(want, meta, name, i)]
    assert tied == ([0, 1] if case == "generic-tiny" else [])
    f64 = common.oracle_losses_f64(name, meta, want, params, eng.param_snapshots) if c.get("f64") else None
    g, w = (_pick(got), _pick(want)) if mode == "fused" else (got, want)
    common.assert_parity(g, w, flips, eng, label, skip=ca.SKIP + tuple("mb%d.hits" % i for i in tied), f64=f64)
    assert steps == list(c["n_steps"])              # (exact in assert_parity already; the table of cont_adaptive.py)
    assert hits == [ca.rule_hits(want, meta, name, i) for i in range(n_mb)]
    names = _names(eng, name, meta, mode)
    print(label, names)
    assert all(n in names for n in scopes["must"]) and not any(n in names for n in scopes["must_not"]), (label, names)
