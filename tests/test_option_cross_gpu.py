"""Crossings of the handle options on the GPU that no feature module runs (shapes, seeds, adapters and oracle runs: tests/option_cross.py;
what the shapes select and what the seeds reach: tests/test_option_cross_cpu.py):

A.  Message flips on every instantiation of k_conversation_fast3 a flipping handle can select -- V = 100 | run-time width, k_prep merged |
    its own launch --, under Adaptive and Fixed exchange, with the flipping handle's k_bwd_conv_fast backward (and the unmerged-statistics
    one), against the Philox masks and tests/flipout_ref.py.
B.  Frozen agents (mmg_set_trainable) together with flips, a sender variant or Gaussian noise: the two setters in either order and with a
    minibatch in between -- the same plan, the same step bit for bit, the wrapped oracle's step with FrozenOptimizer.
C.  The evaluation corruption mask on the run-time-width fast3, on the 512-thread generic kernel and together with flipout_dev.
D.  The run-time-width small-agent kernels at their width and class-count edges.

Tolerances, the project's own: forward quantities 1e-4 absolute, gradients and parameters 1e-4 + 1e-3 |v|, the 2e-5 near-tie band of
tests/test_flipout_gpu.py with at least 3/4 of the rows compared, exact equality wherever a test says bit-identical."""
import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import common, flipout_ref, generic_inst as gi, noise_ref as nr, option_cross as oc, training_controls_ref as ref
from tests.test_plan_cpu import switches  # noqa: F401  (a fixture: exactly the given selection switches set)

pytestmark = pytest.mark.gpu

TAPE_KEYS = ("s", "ps", "z", "pz", "w", "pw", "y", "lp_z", "lp_w")
STEP = [False, True]
STEP_IDS = ["phased", "fused"]


# ------------------------------------------------------------------ helpers
def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _inputs(meta, eng, us=None):
    """((x, target, desc), (u_z, u_s, u_w)) of minibatch 0 on the device; us: other uniforms than the seeded ones."""
    x, target, desc, u = common.case_inputs(meta, 0)
    u = us if us is not None else u
    ud = tuple(_dev(eng, np.ascontiguousarray(a, dtype=np.float32)) for a in (u[0], np.asarray(u[1])[..., 0], u[2]))
    return (_dev(eng, x), _dev(eng, target), _dev(eng, desc)), ud


def _tape(eng, keys=TAPE_KEYS):
    torch.cuda.synchronize()
    eng.check_sync()
    return {k: eng.tape[k].cpu().numpy().copy() for k in keys}


def _scopes(eng, call):
    eng.set_profiling(True)
    call()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _state(eng):
    torch.cuda.synchronize()
    return dict(flat_params=eng.flat_params.clone(), opt_state=eng.opt_state.clone(), flat_grads=eng.flat_grads.clone(),
                losses=eng.tape["losses"].clone(), counter=eng.tape["counter"].clone())


def _assert_same_state(a, b, label, counter=slice(None)):
    for k in ("losses", "flat_grads", "flat_params", "opt_state"):
        if not torch.equal(a[k], b[k]):
            where = torch.nonzero(a[k] != b[k]).reshape(-1)
            assert False, "%s: %s differs in %d of %d places (first %d, last %d), max |difference| %.3e" % (
                label, k, where.numel(), a[k].numel(), int(where[0]), int(where[-1]), float((a[k] - b[k]).abs().max()))
    assert torch.equal(a["counter"][counter], b["counter"][counter]), "%s: counter %s vs %s" % (label, a["counter"].tolist(), b["counter"].tolist())


def _restore(eng, meta):
    """The seeded weights, a zeroed optimizer state, the minibatch / step / frozen-step counters at zero: the state of a fresh handle
    (word 3 of the counter is the handle's own launch epoch and stays)."""
    eng.load_state_dicts(cpu_ref.fill_state_dicts(common.param_shapes(eng), seed=meta["seed_weights"]))
    eng.opt_state.zero_()
    c = eng.tape["counter"]
    c[:3] = 0
    c[4:8] = 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ A. flips on every fast3 instantiation
def _flip_scopes(names, case):
    V, _, sw = case
    conv, bwd = ("k_conversation", "k_bwd_conv") if V == 100 else ("k_conversation_wv", "k_bwd_conv_wv")
    assert conv in names and bwd in names and "k_wgrad" in names, names
    assert ("k_prep+h_x" in names) == ("MMG_NO_MERGE_PREP" in sw), names
    if "MMG_NO_MERGE" in sw:
        assert "k_stats" in names, names
    assert "k_game" not in names and "k_conv_tile" not in names, names
    other = ("k_conversation_wv", "k_bwd_conv_wv") if V == 100 else ("k_conversation", "k_bwd_conv")
    assert not set(other) & set(names), names


def _flip_train_forward(case, switches):
    """A training run-all forward with injected uniforms on a fresh flipping engine of the case: (tape, host uniforms, engine)."""
    V, exchange, sw = case
    switches({k: "1" for k in sw})
    meta = oc.c1_meta(V, exchange)
    eng = common.make_engine(meta)
    eng.set_message_flipout(oc.P_SEN, oc.P_REC)
    assert oc.plan_fields(eng.plan_text())["family"] == 0 and oc.plan_fields(eng.plan_text())["merge_prep"] == int("MMG_NO_MERGE_PREP" not in sw)
    xs, ud = _inputs(meta, eng)
    eng.forward(*xs, *ud, seed=oc.SEED, train=True, run_all=True)
    tp = _tape(eng)
    assert int(eng.tape["counter"][0]) == 1
    return tp, tuple(u.cpu().numpy() for u in ud), eng


@pytest.mark.parametrize("case", oc.FLIP_CASES, ids=oc.flip_id)
def test_flip_positions_are_the_philox_masks(case, switches):
    """The bits that differ from the GPU's own sample u < p are the Philox masks, exactly (no near-tie can interfere), and the
    log-likelihood sums score the flipped bits with the logits' own probabilities."""
    tp, uh, _ = _flip_train_forward(case, switches)
    m_z, m_w = flipout_ref.flip_masks(oc.SEED, 1, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC)
    np.testing.assert_array_equal((tp["z"] != (uh[0] < tp["pz"])).astype(np.float32), m_z)
    np.testing.assert_array_equal((tp["w"] != (uh[2] < tp["pw"])).astype(np.float32), m_w)
    assert 0 < m_z.sum() < m_z.size and 0 < m_w.sum() < m_z.sum()
    assert set(np.unique(tp["z"])) <= {0.0, 1.0} and set(np.unique(tp["w"])) <= {0.0, 1.0}
    for bits, p, lp in ((tp["z"], tp["pz"], tp["lp_z"]), (tp["w"], tp["pw"], tp["lp_w"])):
        b, q = bits.astype(np.float64), p.astype(np.float64)
        want = (b * np.log(q + 1e-8) + (1 - b) * np.log(1 - q + 1e-8)).sum(-1)
        np.testing.assert_allclose(lp.reshape(want.shape), want, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("case", oc.FLIP_CASES, ids=oc.flip_id)
def test_flipping_conversation_matches_the_oracle_wrapper(case, switches):
    tp, uh, _ = _flip_train_forward(case, switches)
    want, u = oc.flip_conversation(case[0], case[1])
    assert (want["z"] != (uh[0] < want["pz"])).any()                    # the oracle's messages are flipped ones
    oc.check_conversation(tp, want, oc.sample_ties(u), "cross/flip conv/" + oc.flip_id(case))


MINIBATCH_CASES = [(c, f) for c in oc.FLIP_CASES for f in STEP if not (f and c == oc.PHASED_ONLY)]


@pytest.mark.parametrize("case,fused", MINIBATCH_CASES, ids=["%s-%s" % (oc.flip_id(c), STEP_IDS[f]) for c, f in MINIBATCH_CASES])
def test_flipping_minibatch_matches_the_oracle(case, fused, switches, monkeypatch):
    """cpu_ref.train_minibatch on the flipped agents against the phased step (every array exchange() returns, the flipped bits exact) and
    the fused step (what training reads); the launches are the case's own.  The MMG_NO_MERGE case is the phased step's: mmg_loss_stats
    launches k_stats and mmg_backward the FLIP handle's backward without statistics and class roles."""
    V, exchange, sw = case
    switches({k: "1" for k in sw})
    meta = oc.c1_meta(V, exchange)
    name = "cross_flip_" + oc.flip_id(case)
    us, want = oc.flip_minibatch(V, exchange)
    n = int(want["mb0.n_steps"])
    assert (np.asarray(want["mb0.sen_feats"]) != (np.asarray(us[0])[:n] < np.asarray(want["mb0.sen_probs"]))).any()
    make = common.make_engine

    def flipping(meta_, tweak=None, **over):
        eng = make(meta_, tweak=tweak, **over)
        eng.set_message_flipout(oc.P_SEN, oc.P_REC)
        return eng
    monkeypatch.setattr(common, "make_engine", flipping)
    monkeypatch.setitem(common.U_OVERRIDES, name, lambda i, u_z, u_s, u_w: us)
    got, eng = common.hip_train_case(name, meta, fused=fused)
    pick = (lambda d: {k: d[k] for k in d if any(t in k for t in oc.FUSED_KEEP)}) if fused else (lambda d: d)
    common.assert_parity(pick(got), pick(want), [], eng, "cross/flip/%s/%s" % (oc.flip_id(case), STEP_IDS[fused]), skip=("y2.bias",),
                         atol=oc.ATOL, rtol=oc.RTOL)
    xs, ud = _inputs(meta, eng, us)
    if fused:
        names = _scopes(eng, lambda: eng.train_step(*xs, *ud))
    else:
        def phased():
            eng.forward(*xs, *ud, train=True, run_all=True)
            eng.loss_stats()
            eng.backward(*xs)
            eng.clip_step()
        names = _scopes(eng, phased)
    _flip_scopes(names, case)


def test_evaluation_under_flipout_dev_on_the_run_time_width(switches):
    """The first wide case: evaluation conversations 0 and 1 under flipout_dev (streams 5 / 6, key eval_seed) -- the tape is
    |round(p) - mask| exactly, conversation 0 follows the oracle wrapper."""
    case = oc.FLIP_CASES[0]
    V, exchange, sw = case
    assert V != 100 and not sw
    switches({})
    meta = oc.c1_meta(V, exchange)
    eng = common.make_engine(meta)
    eng.set_message_flipout(oc.P_SEN, oc.P_REC, dev=True, eval_seed=oc.EVAL_SEED)
    xs, _ = _inputs(meta, eng)
    masks = []
    for c1 in (0, 1):
        names = _scopes(eng, lambda: eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc()))
        assert "k_conversation_wv" in names and "k_conversation" not in names, names
        tp = _tape(eng)
        m_z, m_w = flipout_ref.flip_masks(oc.EVAL_SEED, c1, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC, flipout_ref.EVAL_STREAMS)
        np.testing.assert_array_equal(tp["z"], np.abs(np.round(tp["pz"]) - m_z), err_msg="z, evaluation %d" % c1)
        np.testing.assert_array_equal(tp["w"], np.abs(np.round(tp["pw"]) - m_w), err_msg="w, evaluation %d" % c1)
        masks.append((m_z, m_w))
        oc.check_conversation(tp, oc.flip_eval_conversation(V, c1), oc.round_ties(oc.T, oc.B), "cross/flip eval/%d" % c1)
    assert (masks[0][0] != masks[1][0]).any() and (masks[0][1] != masks[1][1]).any()
    assert int(eng.tape["counter"][0]) == 0                             # evaluations leave the minibatch counter alone


# ------------------------------------------------------------------ B. frozen agents x channel options, in every setter order
def _set_option(eng, option):
    if option == "flip":
        eng.set_message_flipout(oc.P_SEN, oc.P_REC)
    elif option == "variant":
        eng.set_sender_variant(*oc.VARIANT)
    else:
        eng.set_message_noise(nr.SIGMA_SEN, nr.SIGMA_REC)


def _handle(option, meta, order, frozen, us):
    """A fresh handle with the option and the mask set in `order` (oc.ORDERS).  freeze_step_option: the mask, one plain training
    minibatch -- the pending job table goes to the device --, the state of a fresh handle again, then the option."""
    eng = common.make_engine(meta)
    trainable = [a for a in ref.AGENTS if a not in frozen]
    if order == "option_then_freeze":
        _set_option(eng, option)
        eng.set_trainable(trainable)
    else:
        eng.set_trainable(trainable)
        if order == "freeze_step_option":
            xs, ud = _inputs(meta, eng, us)
            eng.train_step(*xs, *ud)
            _restore(eng, meta)
        _set_option(eng, option)
    return eng


def _fresh_plan(eng, text, option, frozen):
    return _lib.plan_for(eng.cfg, _lib.plan_caps(text), (oc.PLAN_FLAG[option] if option else 0) | oc.frozen_flags(frozen))


@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("option,case,mask", oc.FROZEN_CASES)
def test_frozen_agents_under_a_channel_option_in_every_setter_order(option, case, mask, fused, switches):
    switches({k: "1" for k in oc.SWITCHES_OF.get((option, case), ())})
    meta, _, us = oc.option_ref(option, case)
    want, _ = oc.frozen_oracle(option, case, mask)
    frozen = ref.MASKS[mask]
    mode_trains = ref.trained_agents(meta)
    trained = [a for a in mode_trains if a not in frozen]
    label = "cross/frozen/%s-%s/%s/%s" % (option, case, mask, STEP_IDS[fused])
    runs = {}
    for order in oc.ORDERS:
        eng = _handle(option, meta, order, frozen, us)
        plan = eng.plan_text()
        # the plan of the handle is the plan decided from scratch for this option and mask on this device's caps
        assert plan == _fresh_plan(eng, plan, option, frozen), "%s %s" % (label, order)
        assert eng.training_controls()["trainable"] == tuple(a for a in ref.AGENTS if a not in frozen)
        dev_inputs = _inputs(meta, eng, us)
        got, eng, problems = ref.hip_loop(None, meta, [dict(frozen=frozen)], fused=fused, eng=eng, inputs=lambda i: dev_inputs)
        assert not problems, "%s %s\n%s" % (label, order, "\n".join(problems))
        assert eng.plan_text() == plan
        problems = common.compare_packed(ref.pick(got, fused), ref.pick(want, fused), atol=ref.ATOL, rtol=ref.RTOL, skip=oc.skip_of(meta),
                                         label="%s/%s" % (label, order))
        assert not problems, "%s %s\n%s" % (label, order, "\n".join(problems[:30]))
        for a in trained:
            assert "mb0.gradnorm." + a in want and float(got["mb0.gradnorm." + a]) > 0, a
        assert eng.agent_steps() == {a: (1 if a in trained or a not in mode_trains else 0) for a in ref.AGENTS}
        eng.check_sync()
        runs[order] = (plan, _state(eng), eng)
    first = runs[oc.ORDERS[0]]
    for order in oc.ORDERS[1:]:
        assert runs[order][0] == first[0], "%s: plan of %s differs from %s" % (label, order, oc.ORDERS[0])
        # (the handle that ran a minibatch before has launched more: word 3, its own launch epoch, is not compared)
        words = slice(None) if order == "freeze_then_option" else [0, 1, 2, 4, 5, 6, 7]
        _assert_same_state(runs[order][1], first[1], "%s: %s vs %s" % (label, order, oc.ORDERS[0]), counter=words)
    if option == "noise":
        eng = first[2]
        start = common.make_engine(meta)
        if "receiver" in frozen:                                        # continuous messages train the receiver alone: nothing moves ...
            assert torch.equal(eng.flat_params, start.flat_params) and not bool(eng.opt_state.any())
            xs, _ = _inputs(meta, eng, us)                              # ... but the channel is noisy: step 0 of the sender reads no message
            start.forward(*xs, seed=0, train=True, run_all=True)
            n_z, _ = nr.noise_fields(0, 1, *nr.dims(meta))
            diff = _tape(eng, ("z",))["z"][0] - _tape(start, ("z",))["z"][0]
            print("%s: max |z[0] - clean z[0] - sigma n| = %.3e" % (label, np.abs(diff - nr.SIGMA_SEN * n_z[0]).max()))
            np.testing.assert_allclose(diff, nr.SIGMA_SEN * n_z[0], atol=1e-4, rtol=0)
            assert np.abs(nr.SIGMA_SEN * n_z[0]).max() > 0.5
        else:                                                           # the sender's bit is a no-op: the unfrozen handle's step, bit for bit
            _set_option(start, option)
            dev_inputs = _inputs(meta, start, us)
            ref.hip_loop(None, meta, [dict()], fused=fused, eng=start, inputs=lambda i: dev_inputs)
            _assert_same_state(first[1], _state(start), label + ": frozen sender vs unfrozen handle")
            assert start.plan_text() == first[0]


@pytest.mark.parametrize("kernel", ["fast3", "generic"])
def test_clearing_the_flips_while_frozen_is_the_handle_that_only_froze(kernel, switches):
    """mmg_set_message_flipout(None, None) re-selects under the mask in force: the plan and the next fused step of a handle that only
    froze -- from a handle that never stepped and from one whose flipping step put its tables on the device.  (The second found a
    defect: the one-launch step right behind a step of the launch chain took that step's sums of squares and clip coefficients for its
    own -- k_wgrad<OPT> tagged its hand-off pairs with the same launch epoch on both routes, kernels_bwd.h -- the gradients and losses
    identical, the parameters off by up to 1e-5 on every trained agent.)"""
    switches({k: "1" for k in oc.SWITCHES_OF.get(("flip", kernel), ())})
    meta, _, us = oc.option_ref("flip", kernel)
    frozen = ref.MASKS["sender_frozen"]
    trainable = [a for a in ref.AGENTS if a not in frozen]
    only = common.make_engine(meta)
    only.set_trainable(trainable)
    xs, ud = _inputs(meta, only, us)
    only.train_step(*xs, *ud)
    want = _state(only)
    assert only.plan_text() == _fresh_plan(only, only.plan_text(), None, frozen)
    for stepped in (False, True):
        eng = _handle("flip", meta, "option_then_freeze", frozen, us)
        flipping = eng.plan_text()
        if stepped:
            eng.train_step(*xs, *ud)
            _restore(eng, meta)
        eng.set_message_flipout(None, None)
        assert eng.plan_text() == only.plan_text() and (kernel == "generic" or eng.plan_text() != flipping)
        eng.train_step(*xs, *ud)
        _assert_same_state(_state(eng), want, "cleared%s vs only frozen" % (" after a step" if stepped else ""),
                           counter=[0, 1, 2, 4, 5, 6, 7] if stepped else slice(None))
        lo, hi = eng.agent_range["sender"]
        assert not bool(eng.flat_grads[lo:hi].any())
        eng.check_sync()


def test_game_with_flips_freezes_its_sender(switches):
    """Game(flipout_sen=..., flipout_rec=...), then game.freeze("sender"): the engine's controls and plan are those of the handle-level
    cases, exchange() flips at the Philox masks' positions and backpropagates."""
    from multimodalgame_amd import losses
    from tests.test_flipout_gpu import _game
    switches({})
    meta = oc.c1_meta(100)
    game, eng, fl = _game(meta, seed=oc.SEED, autograd=True, flipout_sen=oc.P_SEN, flipout_rec=oc.P_REC)
    game.freeze("sender")
    assert eng.flipout == (oc.P_SEN, oc.P_REC, False)
    ctl = eng.training_controls()
    assert ctl["trainable"] == ("receiver", "baseline_rec", "baseline_sen") and ctl["mask"] == 13
    plan = eng.plan_text()
    assert plan == _fresh_plan(eng, plan, "flip", ("sender",)) and oc.plan_fields(plan)["family"] == 0
    xs, ud = _inputs(meta, eng)
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], uniforms=ud, train=True, break_early=True))
    n = len(out[3])
    uh = tuple(u.cpu().numpy() for u in ud)
    m_z, m_w = flipout_ref.flip_masks(oc.SEED, 1, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC)
    sen_feats, sen_probs = torch.stack(out[1][0]).cpu().numpy(), torch.stack(out[1][1]).detach().cpu().numpy()
    np.testing.assert_array_equal((sen_feats != (uh[0][:n] < sen_probs)).astype(np.float32), m_z[:n])
    rec_feats, rec_probs = torch.stack(out[2][0]).cpu().numpy(), torch.stack(out[2][1]).detach().cpu().numpy()
    np.testing.assert_array_equal((rec_feats != (uh[2][:n] < rec_probs)).astype(np.float32), m_w[:n])
    loss = losses.training_losses(out, xs[1], fl)
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)
    loss["receiver"].backward()
    grads = [p.grad for p in game.modules["receiver"].parameters() if p.grad is not None]
    assert grads and any(float(g.abs().max()) > 0 for g in grads)
    assert eng.plan_text() == plan
    eng.check_sync()


# ------------------------------------------------------------------ C. the corruption mask on the untested sites
def _corrupted_eval(site, scope):
    """An evaluation run-all forward under the mask against the oracle with the sender corrupted: tests/test_corrupt_gpu.py's rule."""
    meta = oc.corrupt_meta(site)
    mask = oc.corrupt_mask(meta["rec_w_dim"])
    eng = common.make_engine(meta)
    xs, _ = _inputs(meta, eng)
    names = _scopes(eng, lambda: eng.forward(*xs, train=False, run_all=True, corrupt_mask=mask))
    assert scope in names, names
    tp = _tape(eng, ("s", "ps", "z", "pz", "w", "pw", "y", "dist"))
    conv, res = oc.corrupt_oracle(site)
    n, nb = conv["s"].shape[:2]
    ok = []
    oc.check_conversation(tp, conv, oc.round_ties(n, nb), "cross/corrupt/" + site, ok_out=ok)
    np.testing.assert_array_equal(tp["z"], np.abs(np.round(tp["pz"]) - mask))       # the message the receiver read, every row
    assert (tp["z"][0][:, mask != 0] != np.round(tp["pz"][0][:, mask != 0])).all()
    # corrupt_ref.eval_batch: the output distribution of the conversation as eval_dev runs it, on the samples no near-tie took away
    want_dist = res["dist"].numpy()
    print("cross/corrupt/%s dist: max |gpu - oracle| = %.3e on %d samples" % (site, np.abs(tp["dist"] - want_dist)[ok[0]].max(), int(ok[0].sum())))
    np.testing.assert_allclose(tp["dist"][ok[0]], want_dist[ok[0]], atol=1e-4, rtol=0)
    assert 4 * int(ok[0].sum()) >= 3 * nb
    return eng, names


def test_corruption_mask_on_the_run_time_width_fast3(switches):
    switches({})
    _, names = _corrupted_eval("fast3_wide", "k_conversation_wv")
    assert "k_conversation" not in names, names


def test_corruption_mask_on_the_512_thread_generic_kernel(switches):
    switches({})
    meta = oc.corrupt_meta("generic_512")
    assert gi.conv_threads(**gi.dims_of(meta)) == 512
    eng, names = _corrupted_eval("generic_512", "k_conversation")
    assert "family 3 " in eng.plan_text().splitlines()[0], eng.plan_text()
    assert not [k for k in names if "tile" in k or "_wv" in k or "_mc" in k], names


def test_corruption_mask_together_with_flipout_dev(switches):
    """k_conversation_fast3's FLIP site: the mask applies after the flip, to the sender's message alone; the second evaluation draws
    other flips under the same mask."""
    switches({})
    meta = oc.corrupt_meta("fast3_flip")
    mask = oc.corrupt_mask()
    eng = common.make_engine(meta)
    eng.set_message_flipout(oc.P_SEN, oc.P_REC, dev=True, eval_seed=oc.EVAL_SEED)
    assert oc.plan_fields(eng.plan_text())["family"] == 0
    xs, _ = _inputs(meta, eng)
    seen = []
    for c1 in (0, 1):
        names = _scopes(eng, lambda: eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc(), corrupt_mask=mask))
        assert "k_conversation" in names and "k_conversation_wv" not in names and "k_conv_tile" not in names, names
        tp = _tape(eng)
        m_z, m_w = flipout_ref.flip_masks(oc.EVAL_SEED, c1, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC, flipout_ref.EVAL_STREAMS)
        np.testing.assert_array_equal(tp["z"], np.abs(np.abs(np.round(tp["pz"]) - m_z) - mask), err_msg="z, evaluation %d" % c1)
        np.testing.assert_array_equal(tp["w"], np.abs(np.round(tp["pw"]) - m_w), err_msg="w, evaluation %d" % c1)
        oc.check_conversation(tp, oc.flip_eval_conversation(100, c1, mask), oc.round_ties(oc.T, oc.B), "cross/corrupt/fast3_flip/%d" % c1)
        seen.append((m_z, tp["z"]))
    assert (seen[0][0] != seen[1][0]).any() and (seen[0][1] != seen[1][1]).any() and mask.any() and seen[0][0].any()
    # no mask outlives its call: the next evaluation flips only
    eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc())
    tp = _tape(eng)
    m_z, _ = flipout_ref.flip_masks(oc.EVAL_SEED, 2, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC, flipout_ref.EVAL_STREAMS)
    np.testing.assert_array_equal(tp["z"], np.abs(np.round(tp["pz"]) - m_z))


# ------------------------------------------------------------------ D. width and class-count edges of the run-time-width kernels
@pytest.mark.parametrize("mode", ["run_all_1", "fused_2"])
@pytest.mark.parametrize("V,n_classes", oc.WIDTH_CASES)
def test_run_time_width_kernels_at_their_edges(V, n_classes, mode, switches):
    """A plain Adaptive handle, two minibatches (the second starts from the updated parameters), dead rows in the first: the phased
    run-all step and the fused step through the project's parity gate at tests/test_wide_desc_gpu.py's tolerances."""
    from tests.test_hip_parity import ATOL, RTOL, _skip_keys
    from tests.test_wide_desc_gpu import MODES, WIDE_SCOPES, _names, _pick
    switches({})
    meta = oc.width_meta(V, n_classes)
    want, flips = oc.width_oracle(V, n_classes)
    masks = want["mb0.s_masks"][:, :, 0]
    assert 0 < masks[1].sum() < masks.shape[1]
    got, eng = common.hip_train_case(None, meta, **MODES[mode])
    label = "cross/width%d-d%d-%s" % (V, n_classes, mode)
    if mode == "run_all_1":
        common.assert_parity(got, want, flips, eng, label, skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    else:
        common.assert_parity(_pick(got), _pick(want), flips, eng, label, skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    names = _names(common.make_engine(meta), meta)
    assert set(WIDE_SCOPES) <= set(names) and "k_wgrad" in names, names
    assert not set(names) & {"k_conversation", "k_bwd_conv", "k_game", "k_conv_tile", "k_bwd_tile"}, names
