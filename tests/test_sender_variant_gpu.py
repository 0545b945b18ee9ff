"""The sender's communication ablations (-sender_mix prod / -ignore_code / -ignore_receiver, model.py:217-218, 208-210, 470-472;
include/mmg.h: mmg_set_sender_variant) on the GPU, against the CPU oracle with the wrapped sender (tests/sender_variant_ref.py).

Shape A: config 1's agents (H 256, W 32, R 64, V 100, K 500), 30 classes, 16 samples, 4 steps, RMSprop.  Shape B: H 40, W 12, R 20,
V 12, K 70, 7 classes, 5 samples, 3 steps, 18 image features, Adam -- the strided loops' tails of the new branches.  Weights seed 5,
data seed 6, uniforms seed 7 (tests/test_sender_variant_cpu.py checks what these seeds reach).  Tolerances: tests/test_hip_parity.py's,
as quoted in tests/test_flipout_gpu.py -- forward 1e-4 absolute, gradients 1e-4 + 1e-3 |v|."""
import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import common, sender_variant_ref as ref

pytestmark = pytest.mark.gpu

SEED = 21
ATOL, RTOL = 1e-4, 1e-3
SETTINGS = sorted(ref.SETTINGS)
TAPE_KEYS = ("s", "ps", "z", "pz", "w", "pw", "y", "lp_z", "lp_w", "a")
DEV = torch.device("cuda:0")
_CACHE = {}


def _once(key, make):
    """One oracle run per key, shared by the tests that need it and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _engine(meta, setting=None, **over):
    eng = common.make_engine(meta, **over)
    if setting is not None:
        eng.set_sender_variant(*setting)
    return eng


def _inputs(meta, eng, uniforms=None):
    x, target, desc, u = common.case_inputs(meta, 0)
    u_z, u_s, u_w = uniforms if uniforms is not None else u
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    uh = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (u_z, np.asarray(u_s).reshape(u_s.shape[0], -1), u_w))
    return (d(x), d(target), d(desc)), tuple(d(a) for a in uh), uh


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


def _log_lik(bits, p):
    b, q = bits.astype(np.float64), p.astype(np.float64)
    return (b * np.log(q + 1e-8) + (1 - b) * np.log(1 - q + 1e-8)).sum(-1)


def _train_conversation(shape, name):
    """(GPU tape, oracle conversation) of one run-all training conversation with injected, separated uniforms."""
    meta, setting = ref.meta(shape), ref.SETTINGS[name]
    u = _once(("u", shape, name), lambda: ref.separated_uniforms(meta, setting, margin=1e-4))
    want = _once(("train", shape, name), lambda: ref.conversation(meta, setting, train=True, uniforms=u))
    eng = _engine(meta, setting)
    xs, ud, _ = _inputs(meta, eng, u)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    return _tape(eng, TAPE_KEYS + ("zr",)), want, eng


# ------------------------------------------------------------------ 1. the training conversation against the wrapped oracle
@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
@pytest.mark.parametrize("name", SETTINGS)
def test_training_conversation_matches_the_wrapped_oracle(name, shape):
    tp, want, _ = _train_conversation(shape, name)
    for k in ("s", "z", "w"):                                           # every draw is 1e-4 away from its probability: bits exact
        np.testing.assert_array_equal(tp[k].reshape(want[k].shape), want[k], err_msg=k)
    for k in ("ps", "pz", "pw", "y", "a"):
        err = np.abs(tp[k].reshape(want[k].shape) - want[k]).max()
        print("%s/%s %s: max |gpu - oracle| = %.3e" % (shape, name, k, err))
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)
    for lp, bits, p in (("lp_z", "z", "pz"), ("lp_w", "w", "pw")):
        w_lp = _log_lik(want[bits], want[p])
        np.testing.assert_allclose(tp[lp].reshape(w_lp.shape), w_lp, atol=1e-4, rtol=1e-5, err_msg=lp)


# ------------------------------------------------------------------ 2. ignore_receiver
@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
@pytest.mark.parametrize("name", ["ignore_receiver", "prod_ignore_receiver"])
def test_ignore_receiver_returns_zeros_and_scores_them(name, shape):
    tp, want, _ = _train_conversation(shape, name)
    assert not tp["w"].any() and tp["w"].size == want["w"].size
    assert not tp["zr"].any()                                           # z_r of t = 0 is first_rec = 0, of t > 0 the zero message
    pw = tp["pw"].astype(np.float64)
    assert (pw > 0.5).any()                                             # zeros are not what sampling gave
    np.testing.assert_allclose(tp["lp_w"].reshape(pw.shape[:-1]), np.log(1 - pw + 1e-8).sum(-1), atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(tp["pw"].reshape(want["pw"].shape), want["pw"], atol=ATOL, rtol=0)


def test_ignore_receiver_does_nothing_to_continuous_messages():
    meta = ref.meta("A", use_binary=False, fixed_exchange=True, entropy_rec=None, entropy_sen=None, entropy_s=None)
    keys = ("z", "w", "y", "outp", "dist", "losses")

    def run(setting):
        eng = _engine(meta, setting)
        xs, _, _ = _inputs(meta, eng)
        eng.forward(*xs, train=False, run_all=True)
        ev = _tape(eng, keys[:5])
        eng.train_step(*xs, seed=SEED)
        return ev, _tape(eng, keys), eng.flat_params.cpu().numpy().copy(), eng.plan_text()
    a, b = run(("sum", False, True)), run(None)
    assert a[3] == b[3]                                                 # the same selection
    for got, want in ((a[0], b[0]), (a[1], b[1])):
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(a[2], b[2])
    assert np.abs(b[0]["w"]).max() > 0


# ------------------------------------------------------------------ 3. one training minibatch against the wrapped oracle
MINIBATCH_CASES = [(name, "A") for name in SETTINGS] + [("prod", "B")]
CODE_TENSORS = ("code_layer.weight", "code_layer.bias", "code_bias")


@pytest.mark.parametrize("name,shape", MINIBATCH_CASES)
def test_training_minibatch_matches_the_wrapped_oracle(name, shape, monkeypatch):
    """cpu_ref.train_minibatch with the wrapped sender against the phased step (every array exchange() returns) and against the
    fused step (what training reads): the six losses, every agent's gradients, gradient norms and updated parameters."""
    meta, setting = ref.meta(shape), ref.SETTINGS[name]
    case = "sender_variant_%s_%s" % (name, shape)
    us = _once(("u", shape, name), lambda: ref.separated_uniforms(meta, setting, margin=1e-4))
    want = _once(("minibatch", shape, name), lambda: ref.train_minibatch(meta, setting, us)[0])
    make = common.make_engine

    def variant(meta_, tweak=None, **over):
        eng = make(meta_, tweak=tweak, **over)
        eng.set_sender_variant(*setting)
        return eng
    monkeypatch.setattr(common, "make_engine", variant)
    monkeypatch.setitem(common.U_OVERRIDES, case, lambda i, u_z, u_s, u_w: us)
    assert int(want["mb0.n_steps"]) > 1
    got, eng = common.hip_train_case(case, meta)
    common.assert_parity(got, want, [], eng, None, skip=("y2.bias",), atol=ATOL, rtol=RTOL)
    keep = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")      # tests/test_hip_parity.py: FUSED_KEEP
    pick = lambda d: {k: d[k] for k in d if any(t in k for t in keep)}
    fused, feng = common.hip_train_case(case, meta, fused=True)
    common.assert_parity(pick(fused), pick(want), [], feng, None, skip=("y2.bias",), atol=ATOL, rtol=RTOL)
    for e in (eng, feng):
        plan = e.plan_text()
        assert "family 3 " in plan.splitlines()[0], plan
    before = cpu_ref.fill_state_dicts(common.param_shapes(eng), seed=meta["seed_weights"])["sender"]
    for e in (eng, feng):
        for k in CODE_TENSORS:
            g, p = e.grads["sender"][k].cpu().numpy(), e.params["sender"][k].cpu().numpy()
            if setting[1]:                                              # ignore_code: exact zeros in, bit-identical parameters out
                assert not g.any(), k
                np.testing.assert_array_equal(p, before[k], err_msg=k)
            else:
                assert g.any() and (p != before[k]).any(), k


# ------------------------------------------------------------------ 4. evaluation
@pytest.mark.parametrize("name", SETTINGS)
def test_evaluation_matches_the_wrapped_oracle(name):
    meta, setting = ref.meta("A", seed_data=ref.EVAL_DATA_SEED[name]), ref.SETTINGS[name]
    T, B, W = 4, 16, 32
    want = _once(("eval", name), lambda: ref.conversation(meta, setting, train=False))
    eng = _engine(meta, setting)
    xs, _, _ = _inputs(meta, eng)
    _, ham = eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc())
    tp = _tape(eng)
    for k in ("ps", "pz", "pw", "y"):
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)
    left_out = total = 0
    prod = np.cumprod(want["ps"], 0)                                    # the stop bit rounds the running product (model.py:423-427)
    for bits, p in (("z", want["pz"]), ("w", want["pw"]), ("s", prod)):
        clear = np.abs(p - 0.5) > 1e-4
        left_out += int((~clear).sum()); total += clear.size
        np.testing.assert_array_equal(tp[bits].reshape(p.shape)[clear], want[bits][clear], err_msg=bits)
    assert left_out == 0 and 100 * left_out <= total                    # (the data seed leaves none out: test_sender_variant_cpu.py)
    ham = ham.cpu().numpy().reshape(-1)
    for which, key in enumerate(("z", "w")):
        prev = np.concatenate([np.zeros_like(tp[key][:1]), tp[key][:-1]])
        np.testing.assert_array_equal(ham[1 + which * T:1 + (which + 1) * T], np.abs(tp[key] - prev).sum((1, 2)).astype(np.int64))
    if setting[2]:
        assert not ham[1 + T:1 + 2 * T].any() and not tp["w"].any() and (tp["pw"] > 0.5).any()
    else:
        assert ham[1 + T:1 + 2 * T].any()


# ------------------------------------------------------------------ 5. selection
@pytest.mark.parametrize("name", SETTINGS)
def test_a_variant_handle_runs_the_generic_family(name):
    meta = ref.meta("A")
    eng = _engine(meta)
    fresh_plan = eng.plan_text()
    xs, _, _ = _inputs(meta, eng)
    assert _scopes(eng, lambda: eng.train_step(*xs, seed=SEED)) == ["k_game", "k_wgrad"]
    eng.set_sender_variant(*ref.SETTINGS[name])
    assert eng.sender_variant == ref.SETTINGS[name]
    names = _scopes(eng, lambda: eng.train_step(*xs, seed=SEED))
    assert "k_conversation" in names and "k_bwd_conv" in names and "k_wgrad" in names, names
    assert not [n for n in names if "game" in n or "tile" in n or "fast" in n or "persist" in n or "_mc" in n or "_rc" in n], names
    assert eng.plan_text() != fresh_plan and "family 3 " in eng.plan_text().splitlines()[0]
    eng.set_sender_variant()                                            # clearing restores the original selection
    assert eng.sender_variant is None and eng.plan_text() == fresh_plan
    assert _scopes(eng, lambda: eng.train_step(*xs, seed=SEED)) == ["k_game", "k_wgrad"]


def test_the_default_setting_leaves_a_handle_as_it_was():
    meta = ref.meta("A")

    def run(touch):
        eng = _engine(meta)
        if touch:
            eng.set_sender_variant("sum", False, False)
        xs, _, _ = _inputs(meta, eng)
        names = _scopes(eng, lambda: eng.train_step(*xs, seed=SEED))
        return _tape(eng, ("tstar", "losses", "z", "pz", "lp_z")), eng.flat_params.cpu().numpy().copy(), names, eng.plan_text()
    a, b = run(True), run(False)
    assert a[2] == b[2] == ["k_game", "k_wgrad"] and a[3] == b[3]
    np.testing.assert_array_equal(a[0]["tstar"], b[0]["tstar"])
    live = np.arange(4)[:, None] <= b[0]["tstar"].reshape(1, -1)        # a training step stores the live (step, sample) rows only
    for k in ("z", "pz", "lp_z"):
        np.testing.assert_array_equal(a[0][k][live], b[0][k][live], err_msg=k)
    np.testing.assert_array_equal(a[0]["losses"], b[0]["losses"])
    np.testing.assert_array_equal(a[1], b[1])


def test_flips_and_a_variant_refuse_each_other_and_mou_is_refused():
    meta = ref.meta("A")
    eng = _engine(meta, ("prod", False, False))
    plan = eng.plan_text()
    with pytest.raises(_lib.MmgError, match="sender variant"):
        eng.set_message_flipout(0.1, None)
    assert eng.plan_text() == plan
    eng.set_message_flipout(None, None)                                 # clearing flips that are not set is no conflict
    other = _engine(meta)
    other.set_message_flipout(0.1, 0.1)
    plan = other.plan_text()
    with pytest.raises(_lib.MmgError, match="message flips"):
        other.set_sender_variant("sum", True, False)
    assert other.plan_text() == plan and getattr(other, "sender_variant", None) is None
    other.set_sender_variant()                                          # the default setting on a flipping handle is no conflict
    assert eng.lib.mmg_set_sender_variant(eng.handle, 2, 0, 0) < 0
    assert b"4H binary layer" in eng.lib.mmg_last_error()
    assert eng.plan_text() == _engine(meta, ("prod", False, False)).plan_text()     # the setting before stays
    with pytest.raises(NotImplementedError, match="4H binary layer"):
        eng.set_sender_variant("mou")
    with pytest.raises(ValueError):
        eng.set_sender_variant("max")


# ------------------------------------------------------------------ 6. module level
def _game(meta, **kw):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = common.flags_from_meta(meta)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", **kw)
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    eng.load_state_dicts(cpu_ref.fill_state_dicts(common.param_shapes(eng), seed=meta["seed_weights"]))
    return game, eng, fl


@pytest.mark.parametrize("name", SETTINGS)
def test_agent_level_entries_return_the_tape_rows_of_exchange(name):
    """Training steps through the engine's agent-level entries with the uniforms of the conversation, then an evaluation
    conversation written with Sender.forward / Receiver.forward of a variant Game: both give the rows exchange() leaves."""
    meta, setting = ref.meta("A"), ref.SETTINGS[name]
    game, eng, fl = _game(meta, seed=SEED, sender_mix=setting[0], ignore_code=setting[1], ignore_receiver=setting[2])
    assert eng.sender_variant == setting
    xs, ud, _ = _inputs(meta, eng)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    tp = {k: eng.tape[k].clone() for k in ("z", "pz", "w", "pw", "s", "ps", "y", "h")}
    h = torch.zeros(16, 64, device=eng.device)
    sp = torch.ones(16, device=eng.device)
    w = None
    for t in range(2):
        z, pz, _ = eng.sender_forward(xs[0], w, t, True, u_z=ud[0][t].contiguous(), seed=SEED)
        s, ps, w, pw, y, _ = eng.receiver_forward(z, xs[2], h, sp, t == 0, t, True, u_s=ud[1][t].contiguous(), u_w=ud[2][t].contiguous(), seed=SEED)
        torch.cuda.synchronize()
        for got, key in ((z, "z"), (pz, "pz"), (w, "w"), (pw, "pw"), (s, "s"), (ps, "ps"), (y, "y")):
            assert torch.equal(got.reshape(tp[key][t].shape), tp[key][t]), (key, t)
        if setting[2]:
            assert not bool(w.any()) and bool((pw > 0.5).any())
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], train=False, break_early=False))
    S, R = game.modules["sender"], game.modules["receiver"]
    S.eval(); R.eval(); S.reset_state(); R.reset_state()
    w = torch.zeros(16, 32, device=eng.device)
    with torch.no_grad():
        for t in range(4):
            z, pz = S(xs[0], w, None, t)
            (s, ps), (w, pw), y = R(z, xs[2])
            assert torch.equal(z, out[1][0][t]) and torch.equal(pz, out[1][1][t]), t
            assert torch.equal(w, out[2][0][t]) and torch.equal(pw, out[2][1][t]) and torch.equal(y, out[3][t]), t
            assert not w.requires_grad
            if setting[2]:
                assert not bool(w.any())


# ------------------------------------------------------------------ 7. autograd
def _reference_losses(fl, out, target):
    from tests.test_autograd_gpu import _reference_losses as f
    return f(fl, out, target)


@pytest.mark.parametrize("name", ["prod", "ignore_code"])
def test_reference_block_gives_the_engine_gradients(name):
    """Pattern 1 of tests/test_autograd_gpu.py under a variant: exchange() with autograd, the reference's losses and backward()
    calls give the sender gradients of the engine's own backward pass on the same minibatch."""
    meta, setting = ref.meta("A"), ref.SETTINGS[name]
    game, eng, fl = _game(meta, seed=SEED, autograd=True, sender_mix=setting[0], ignore_code=setting[1], ignore_receiver=setting[2])
    xs, ud, _ = _inputs(meta, eng)
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], uniforms=ud, train=True, break_early=True))
    assert out[1][1][0].requires_grad and out[1][1][0].grad_fn is not None
    losses = _reference_losses(fl, out, xs[1].cpu())
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)
    losses["sender"].backward()
    got = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in game.modules["sender"].named_parameters()}
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    eng.loss_stats()
    eng.backward(*xs)
    torch.cuda.synchronize()
    for k, g in got.items():
        want = eng.grads["sender"][k].detach().cpu().numpy()
        assert g is not None, k
        np.testing.assert_allclose(g.numpy(), want, atol=ATOL, rtol=RTOL, err_msg=k)
        if setting[1] and k in CODE_TENSORS:
            assert not g.numpy().any() and not want.any(), k
        else:
            assert np.abs(want).max() > 0, k


@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("name", ["prod", "ignore_code"])
def test_sender_call_node_matches_float64_autograd(name, t):
    """One Sender.forward node: a seeded random linear functional of probs and h_x against float64 autograd through the oracle's
    wrapped sender with the same weights (the functional does not read the sampled bits)."""
    meta, setting = ref.meta("A"), ref.SETTINGS[name]
    game, eng, fl = _game(meta, seed=SEED, autograd=True, sender_mix=setting[0], ignore_code=setting[1], ignore_receiver=setting[2])
    x = common.case_inputs(meta, 0)[0]
    rs = np.random.RandomState(5 + t)
    w0 = (rs.rand(16, 32) < 0.5).astype(np.float32)
    c1, c2 = (torch.from_numpy(rs.standard_normal((16, n))) for n in (32, 256))
    S = game.modules["sender"]
    S.train()
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)
    _, probs = S(torch.from_numpy(x).to(DEV), torch.from_numpy(w0).to(DEV), None, t)
    ((c1.float().to(DEV) * probs).sum() + (c2.float().to(DEV) * S.h_x).sum()).backward()
    models, _ = ref.build(meta, setting, rng=cpu_ref.UniformTape(np.zeros((4, 16, 32)), None, None))
    Sm = models["sender"].double()
    Sm.train()
    _, p64 = Sm.forward(torch.from_numpy(x).double(), torch.from_numpy(w0).double(), None, t)
    ((c1 * p64).sum() + (c2 * Sm.h_x).sum()).backward()
    for k, p in Sm.named_parameters():
        g = dict(S.named_parameters())[k].grad.detach().cpu().double().numpy()
        want = p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape))
        np.testing.assert_allclose(g, want, atol=ATOL, rtol=RTOL, err_msg=k)
        if (setting[1] and k in CODE_TENSORS) or (t > 0 and k == "code_bias"):
            assert not g.any(), k
        else:
            assert np.abs(want).max() > 0, k


def test_channel_and_input_gradients_refuse_a_variant():
    meta = ref.meta("A")
    for kw in (dict(channel_grad=True), dict(input_grad=True)):
        with pytest.raises(NotImplementedError):
            _game(meta, autograd=True, sender_mix="prod", **kw)
        game, eng, _ = _game(meta, autograd=True, ignore_code=True)
        xs, ud, _ = _inputs(meta, eng)
        with pytest.raises(NotImplementedError):
            game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], uniforms=ud, train=True, break_early=True, **kw))
    eng = _engine(meta, ("prod", False, False))
    xs, ud, _ = _inputs(meta, eng)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    with pytest.raises(_lib.MmgError, match="sender variant"):
        eng.vjp_channel(4, xs[0], xs[2], dy=torch.zeros(4, 16, 30, device=eng.device))
