"""Reach conditions of tests/test_cont_adaptive_gpu.py, on the CPU oracle and the pure kernel selection alone: the inputs of the
continuous + Adaptive GPU cases must take the branches they are meant for -- samples that stop at different steps, a conversation
that breaks early (model.py:866: fewer executed steps than max_exchange), a sample tile that finishes before another one -- and
every shape must select the kernel family it is named after.  Shapes, seeds and predicates: tests/cont_adaptive.py."""
import numpy as np
import pytest

from multimodalgame_amd import _lib
from tests import common, cont_adaptive as ca
from tests.test_generic_instantiations_cpu import SWITCHES

# An MI355X's answers (tests/golden/plans_mi355x.json): the CU count and, per role kernel, the occupancy every recorded shape that
# asked for it was given (c4: persist; c4_r256: rc_bwd, rc_persist; c5_b2048: mc, mc3, mc3p; c1: game, wgrad_opt, wgrad).  No recorded
# shape asks for `split`.
CAPS = [256, -1, 1, 3, 1, 1, 1, 1, 1, 4, 4]
# one float32 spacing below 1: separate_draws moves a close uniform to p -/+ 1e-4 IN float32, which may round towards p by that much
MARGIN = 1e-4 - 6e-8


def test_caps_are_the_recorded_answers():
    from tests.test_plan_cpu import ENTRIES
    assert len(CAPS) == len(_lib.PLAN_CAPS)
    for i, cap in enumerate(_lib.PLAN_CAPS):
        seen = {e["caps"][i] for e in ENTRIES if not e["cu_budget"] and e["caps"][i] != -1}
        assert seen == ({CAPS[i]} if CAPS[i] != -1 else set()), (cap, seen)


@pytest.mark.parametrize("case", ca.ADAPTIVE)
def test_stop_steps_are_spread_and_draws_are_clear(case):
    """Every Adaptive case, every minibatch: at least three distinct stop steps, a sample that stops at step 0 and one at step 2 or
    later, no stop uniform within 1e-4 of its probability, and the executed step counts of the table in cont_adaptive.py."""
    name, meta, want, _, _ = ca.oracle(case)
    steps = []
    for mb in range(meta["n_minibatches"]):
        tstar, n = ca.stop_steps(want, mb)
        hist = np.bincount(tstar, minlength=n).tolist()
        print(case, "minibatch", mb, "steps", n, "t* histogram", hist)
        assert len(set(tstar.tolist())) >= 3 and (tstar == 0).any() and (tstar >= 2).any(), hist
        assert int(tstar.max()) + 1 == n                     # what a single GPU reports: max_b t* + 1 executed steps
        steps.append(n)
    margin = ca.stop_margin(want, meta, name)
    print(case, "smallest |u - p| of a stop draw: %.6e" % margin)
    assert margin >= MARGIN
    assert tuple(steps) == ca.CASES[case]["n_steps"]


def test_recorded_histograms():
    """t* histograms of minibatch 0 as the oracle gives them: fast3 (16 samples over 6 steps) and the two mc3p batches."""
    for case, hist in (("fast3", [10, 3, 1, 1, 0, 1]), ("mc3p-B512", [223, 125, 74, 40, 20, 30]), ("mc3p-B784", [341, 177, 111, 155])):
        _, _, want, _, _ = ca.oracle(case)
        tstar, n = ca.stop_steps(want, 0)
        assert np.bincount(tstar, minlength=n).tolist() == hist, case


def test_fixed_twin_runs_every_step():
    name, meta, want, _, _ = ca.oracle("mc3p-B784-fixed")
    assert meta["fixed_exchange"] and int(want["mb0.n_steps"]) == meta["max_exchange"] == 3 == ca.CASES["mc3p-B784-fixed"]["n_steps"][0]
    assert name not in common.U_OVERRIDES                    # (Fixed: no stop bit decides anything, the seeded uniforms as they are)


@pytest.mark.parametrize("case", ca.BREAKS_EARLY)
def test_conversation_breaks_early(case):
    """n_steps < max_exchange in at least one minibatch: the reference left exchange() early, and a library that reports T fails."""
    _, meta, want, _, _ = ca.oracle(case)
    steps = [int(want["mb%d.n_steps" % mb]) for mb in range(meta["n_minibatches"])]
    assert min(steps) < meta["max_exchange"], steps


def test_a_whole_tile_finishes_before_another():
    """tile: in at least one minibatch the largest t* of one 16-sample tile is below another tile's, so that a tile of the fused
    step is done while others still talk (may_stop)."""
    _, meta, want, _, _ = ca.oracle("tile")
    last = [ca.tile_last_steps(ca.stop_steps(want, mb)[0]) for mb in range(meta["n_minibatches"])]
    print("max t* per tile and minibatch", last)
    assert all(len(v) == 3 for v in last)
    assert any(len(set(v)) > 1 for v in last), last


def test_separate_draws_skips_the_empty_message_probabilities():
    """Continuous messages have no Bernoulli message draws: sen_probs / rec_probs are packed empty, and separate_draws leaves the
    message uniforms as drawn and moves stop uniforms only."""
    name, meta, want, _, _ = ca.oracle("generic-tiny")
    for mb in range(meta["n_minibatches"]):
        assert np.asarray(want["mb%d.sen_probs" % mb]).size == 0 and np.asarray(want["mb%d.rec_probs" % mb]).size == 0
        assert np.asarray(want["mb%d.s_probs" % mb]).size == int(want["mb%d.n_steps" % mb]) * meta["batch"]
        _, _, _, (u_z0, u_s0, u_w0) = common.case_inputs(meta, mb, None)
        _, _, _, (u_z, u_s, u_w) = common.case_inputs(meta, mb, name)
        np.testing.assert_array_equal(u_z, u_z0)
        np.testing.assert_array_equal(u_w, u_w0)
        assert np.abs(u_s - u_s0).max() <= 2e-4
        p = np.asarray(want["mb%d.s_probs" % mb])
        n = p.shape[0]
        np.testing.assert_array_equal(u_s[:n].reshape(p.shape) < p, u_s0[:n].reshape(p.shape) < p)      # the same stop bits


def test_only_the_tiny_agents_tie_a_target_logit():
    """`hits` is compared exactly.  Where the oracle's own log-probabilities tie the target with another class to the bit, its count
    depends on numpy's argsort order among equal keys: the GPU test takes the library's rule on the oracle's values there
    (cont_adaptive.rule_hits).  That happens in generic-tiny alone (5 hidden units in the y head: sample 6 of minibatch 0, sample 5
    of minibatch 1); everywhere else the two counts are the same number."""
    tied = {}
    for case in ca.CASES:
        name, meta, want, _, _ = ca.oracle(case)
        for mb in range(meta["n_minibatches"]):
            t = ca.tied_targets(want, meta, name, mb)
            if t:
                tied[(case, mb)] = t
            else:
                assert ca.rule_hits(want, meta, name, mb) == int(want["mb%d.hits" % mb]), (case, mb)
    assert tied == {("generic-tiny", 0): [6], ("generic-tiny", 1): [5]}, tied
    name, meta, want, _, _ = ca.oracle("generic-tiny")
    assert [ca.rule_hits(want, meta, name, mb) for mb in range(2)] == [3, 5] and [int(want["mb%d.hits" % mb]) for mb in range(2)] == [2, 5]


# ---------------------------------------------------------------------------------------------- the pure selection
def _plan(case, monkeypatch, binary=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in ca.CASES[case]["env"]:
        monkeypatch.setenv(k, "1")
    meta = ca.meta_of(case)
    if binary:
        meta = dict(meta, use_binary=True)
    lines = _lib.plan_for(_lib.make_config(**common.engine_kwargs(meta)), CAPS).splitlines()
    words = [l.replace("|", " ").split() for l in lines]
    val = lambda i, key, off=1: int(words[i][words[i].index(key) + off])
    return dict(family=val(0, "family"), tile_fwd=val(2, "forward"), mc3=val(3, "mc3"), mc3p=val(3, "mc3p"), wins=val(3, "wins"),
                mc_groups=val(4, "groups"), text="\n".join(lines))


WANT_FAMILY = {"fast3": 0, "tile": 2, "generic": 3, "generic-tiny": 3, "persist": 2, "rc": 2}     # (0 fast, 1 mc, 2 tile, 3 generic)


@pytest.mark.parametrize("case", list(ca.CASES))
def test_every_shape_selects_its_family(case, monkeypatch):
    p = _plan(case, monkeypatch)
    print(case, p["text"])
    if case.startswith("mc3"):
        assert p["family"] == 1 and p["mc3"] == 1, p["text"]
        assert p["wins"] == int(bool(ca.CASES[case].get("mc3p"))), p["text"]
        if ca.CASES[case].get("mc3p"):
            assert p["mc3p"] == 1 and p["mc_groups"] == 16, p["text"]
    else:
        assert p["family"] == WANT_FAMILY[case], p["text"]
    if case in ("persist", "rc"):                             # 2 persist/sample, 4 rc persist: what the binary twin of the shape selects
        assert p["tile_fwd"] == {"persist": 2, "rc": 4}[case] == _plan(case, monkeypatch, binary=True)["tile_fwd"], p["text"]


def test_the_two_evaluation_cases_select_their_families(monkeypatch):
    """test_eval_steps_cpu.CASES: c1_cont_B64 runs the register-resident kernels, D130_cont_B17 k_conversation_mc3 (train = False)."""
    from tests.test_eval_steps_cpu import CASES, case_meta
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for name, family, mc3 in (("c1_cont_B64", 0, 0), ("D130_cont_B17", 1, 1)):
        meta = case_meta(CASES[name])
        assert not meta["use_binary"] and not meta["fixed_exchange"]
        lines = _lib.plan_for(_lib.make_config(**common.engine_kwargs(meta)), CAPS).splitlines()
        assert lines[0].startswith("mmg_create: family %d " % family) and (" mc3 %d " % mc3) in lines[3], lines


def test_no_older_training_shape_is_continuous_and_adaptive():
    """The gap this file closes: the shape tables of test_hip_configs.py and test_option_branches_* treat "continuous" as a kind of
    Fixed exchange.  None of them combines use_binary = False with fixed_exchange = False."""
    from tests import test_hip_configs as hc, test_option_branches_cpu as ob
    tables = [hc.C4, hc.C5, hc.C1, ob.C1, ob.C4, ob.TINY, ob.MC3_SHAPE[0]] + [v[0] for v in ob.TRAIN_SHAPES.values()] + [v[0] for v in ob.EVAL_SHAPES.values()]
    assert len(tables) == 7 + len(ob.TRAIN_SHAPES) + len(ob.EVAL_SHAPES)
    for kw in tables:
        assert kw["use_binary"] or kw["fixed_exchange"], kw
    assert not any(kw["use_binary"] or kw["fixed_exchange"] for kw in map(ca.flags_of, ca.ADAPTIVE))
