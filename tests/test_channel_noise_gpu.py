"""Gaussian message noise on continuous messages (include/mmg.h: mmg_set_message_noise) on the GPU, on both conversation kernels that
serve a noise handle -- the generic k_conversation_noise at 256 and 512 threads and the many-class k_conversation_mc3_noise -- against
the draws restated in float64 numpy and the CPU oracle with wrapped agents (tests/noise_ref.py; shapes, seeds and reach conditions
there and in tests/test_channel_noise_cpu.py).  Sigmas 0.3 (sender) / 0.2 (receiver).

Tolerances, the project's own: forward values 1e-4 absolute; parameters and gradients against the fp32 oracle 1e-4 + 1e-3 |v|
(tests/test_hip_parity.py); a VJP against float64 2e-5 max(1, max|g|) + 1e-3 |g| (tests/test_channel_grad_gpu.py).  Expected error of
the noise itself: about 1e-6 sigma (float32 log, sqrt and the hardware cosine on 24-bit uniforms)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import channel_ref, common, generic_inst as gi, noise_ref as nr

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-4, 1e-3
S1, S2 = nr.SIGMA_SEN, nr.SIGMA_REC
TAPE = ("z", "w", "y", "s", "ps")
FUSED_KEEP = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")      # tests/test_hip_parity.py
OTHER_CONV = ("k_conversation", "k_conversation_wv", "k_conversation_mc", "k_conv_tile", "k_conv_split", "k_conv_persist", "k_conv_rc", "k_game")
PAIR = ("sender", "receiver")


# ------------------------------------------------------------------ helpers
def _engine(meta, noise=(S1, S2), dev=False, **over):
    eng = common.make_engine(meta, **over)
    if noise is not None:
        eng.set_message_noise(noise[0], noise[1], dev=dev, eval_seed=nr.EVAL_SEED)
    return eng


def _name(case):
    return "channel_noise_" + case


def _uniforms(case, meta):
    """Host uniforms (u_z, u_s [T, B, 1], u_w) of minibatch 0: the seeded ones, for an Adaptive case moved 1e-4 away from the stop
    probabilities of the oracle's noisy minibatch (key 0, counter 1)."""
    if case in nr.ADAPTIVE:
        return gi.oracle_minibatch(_name(case), meta, nr.wrap_of(meta))[0]
    return common.case_inputs(meta, 0)[3]


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _inputs(meta, eng, us=None, rows=None):
    x, target, desc, u = common.case_inputs(meta, 0)
    u = us if us is not None else u
    if rows is not None:
        x, target = x[rows], target[rows]
    ud = tuple(_dev(eng, np.ascontiguousarray(a, dtype=np.float32)) for a in (u[0], u[1][..., 0], u[2]))
    return (_dev(eng, x), _dev(eng, target), _dev(eng, desc)), ud


def _tape(eng, keys=TAPE):
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


def _assert_conversation_kernel(names, case):
    assert nr.SCOPES[case] in names, names
    assert not [n for n in names if n in OTHER_CONV or "fast" in n or "tile" in n], names


def _oracle(case, key, c1, streams, train, us=None, mask=None):
    meta = nr.meta_of(case)
    tag = ("noise conv", case, key, c1, streams, train, None if mask is None else tuple(mask.tolist()))
    return gi.once(tag, lambda: nr.conversation(meta, *nr.noise_fields(key, c1, *nr.dims(meta), streams=streams), train=train,
                                                uniforms=us, mask=mask))


def _compare(tp, want, label, u_s=None):
    """Values at 1e-4 absolute; the stop bits exact wherever their draw (training: the uniform; evaluation: 0.5, asserted on the CPU)
    is more than 2e-5 away from the oracle's probability -- the band in which two correct fp32 sums may decide differently."""
    for k in ("z", "w", "y", "ps"):
        got = tp[k].reshape(want[k].shape)
        print("%s %s: max |gpu - oracle| = %.3e" % (label, k, np.abs(got - want[k]).max()))
        np.testing.assert_allclose(got, want[k], atol=ATOL, rtol=0, err_msg="%s %s" % (label, k))
    ok = np.ones(want["s"].shape, bool) if u_s is None else np.abs(np.asarray(u_s).reshape(want["ps"].shape) - want["ps"]) > 2e-5
    assert ok.mean() > 0.9
    np.testing.assert_array_equal(tp["s"].reshape(want["s"].shape)[ok], want["s"][ok], err_msg="%s s" % label)


def _clean_z0(meta, xs, train=True):
    """Step 0 of the sender depends on no message: the clean handle's z[0] is the logit every noise handle adds its draw to."""
    clean = common.make_engine(meta)
    clean.forward(*xs, seed=0, train=train, run_all=True)
    return _tape(clean, ("z",))["z"][0]


# ------------------------------------------------------------------ 1. the run-all training forward
@pytest.mark.parametrize("case", ["G256", "G512", "M", "A"])
def test_training_forward_matches_the_wrapped_oracle(case):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    us = _uniforms(case, meta)
    eng = _engine(meta)
    xs, ud = _inputs(meta, eng, us)
    names = _scopes(eng, lambda: eng.forward(*xs, *ud, seed=0, train=True, run_all=True))
    _assert_conversation_kernel(names, case)
    tp = _tape(eng)
    assert int(eng.tape["counter"][0]) == 1                          # the first minibatch of a handle draws with counter 1
    n_z, n_w = nr.noise_fields(0, 1, T, B, W)
    _compare(tp, _oracle(case, 0, 1, nr.TRAIN_STREAMS, True, us), "train/" + case, u_s=us[1])
    np.testing.assert_allclose(tp["z"][0] - _clean_z0(meta, xs), S1 * n_z[0], atol=ATOL, rtol=0)
    assert np.abs(S1 * n_z[0]).max() > 0.5                            # (the difference is the noise, not rounding)


# ------------------------------------------------------------------ 2. one training minibatch
@pytest.mark.parametrize("case", ["G256", "M", "A", "MA"])
def test_training_minibatch_matches_the_oracle(case, monkeypatch):
    """mmg_train_step against cpu_ref.train_minibatch on the wrapped agents: losses, the receiver's gradients and updated parameters
    through common.assert_parity; continuous mode updates the receiver alone, so the other three agents stay bit-identical."""
    meta = nr.meta_of(case)
    wrap = nr.wrap_of(meta)                                           # common.hip_train_case trains with seed 0, counter 1
    us, want, flips = gi.oracle_minibatch(_name(case), meta, wrap)
    monkeypatch.setitem(common.U_OVERRIDES, _name(case), lambda i, u_z, u_s, u_w: us)
    make = common.make_engine

    def noisy(meta_, tweak=None, **over):
        eng = make(meta_, tweak=tweak, **over)
        eng.set_message_noise(S1, S2)
        return eng
    monkeypatch.setattr(common, "make_engine", noisy)
    if case in nr.ADAPTIVE:
        tstar, n = nr.stop_steps(want)
        assert (tstar == 0).any() and (tstar == n - 1).any()
    got, eng = common.hip_train_case(_name(case), meta, fused=True)
    pick = lambda d: {k: d[k] for k in d if any(t in k for t in FUSED_KEEP)}
    with gi.wrapped_agents(wrap):
        common.assert_parity(pick(got), pick(want), flips, eng, None, skip=nr.SKIP, atol=ATOL, rtol=RTOL)
    start = make(meta)
    moved = False
    for a in ("sender", "baseline_sen", "baseline_rec"):
        for k, v in eng.params[a].items():
            assert torch.equal(v, start.params[a][k]), (a, k)
    for k, v in eng.params["receiver"].items():
        moved = moved or not torch.equal(v, start.params["receiver"][k])
    assert moved
    xs, _ = _inputs(meta, eng)
    names = _scopes(eng, lambda: eng.train_step(*xs, seed=0))
    _assert_conversation_kernel(names, case)
    assert "k_wgrad" in names, names


# ------------------------------------------------------------------ 3. counters
def test_consecutive_minibatches_and_injected_uniforms():
    case = "G256"
    meta = nr.meta_of(case)
    eng = _engine(meta)
    xs, ud = _inputs(meta, eng)
    first = None
    for c1 in (1, 2):
        eng.forward(*xs, seed=5, train=True, run_all=True)
        tp = _tape(eng)
        assert int(eng.tape["counter"][0]) == c1
        want = _oracle(case, 5, c1, nr.TRAIN_STREAMS, True, common.case_inputs(meta, 0)[3])
        for k in ("z", "w", "y", "ps"):                              # (Fixed exchange: no value depends on the stop draws)
            np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg="%s, counter %d" % (k, c1))
        first = first or tp
    assert np.abs(tp["z"][0] - first["z"][0]).max() > 0.1             # another counter, another field
    injected = _engine(meta)
    injected.forward(*xs, *ud, seed=5, train=True, run_all=True)      # injected uniforms do not move the noise
    tp = _tape(injected)
    for k in ("z", "w", "y", "ps"):
        np.testing.assert_array_equal(tp[k], first[k], err_msg=k)


@pytest.mark.parametrize("case,split", [("M", 16), ("G256", 2)])
def test_half_batch_handles_draw_the_global_batch_rows(case, split):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    whole = _engine(meta)
    xs, _ = _inputs(meta, whole)
    whole.forward(*xs, seed=0, train=True, run_all=True)
    full = _tape(whole, ("z", "w"))
    n_z, _ = nr.noise_fields(0, 1, T, B, W)
    z0 = _clean_z0(meta, xs)
    for off, size in ((0, split), (split, B - split)):
        eng = _engine(meta, batch=size, global_batch=B, batch_offset=off)
        rows = slice(off, off + size)
        sx, _ = _inputs(meta, eng, rows=rows)
        names = _scopes(eng, lambda: eng.forward(*sx, seed=0, train=True, run_all=True))
        _assert_conversation_kernel(names, case)
        sh = _tape(eng, ("z", "w"))
        for k in ("z", "w"):
            np.testing.assert_allclose(sh[k], full[k][:, rows], atol=ATOL, rtol=0, err_msg="%s, offset %d" % (k, off))
        np.testing.assert_allclose(sh["z"][0] - z0[rows], S1 * n_z[0][rows], atol=ATOL, rtol=0)


# ------------------------------------------------------------------ 4. evaluation
@pytest.mark.parametrize("case", ["G256", "G512", "M", "A"])
def test_evaluation(case, monkeypatch):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    if nr.SCOPES[case] == "k_conversation_noise":                     # the clean handle of the same family (read when a handle is created)
        monkeypatch.setenv("MMG_NO_FAST", "1")
        monkeypatch.setenv("MMG_NO_TILE", "1")
    eng = _engine(meta, dev=False)
    xs, _ = _inputs(meta, eng)
    clean = common.make_engine(meta)
    clean.forward(*xs, train=False, run_all=True)
    plain = _tape(clean)
    # without noise_dev: the clean handle's tape, bit for bit
    names = _scopes(eng, lambda: eng.forward(*xs, train=False, run_all=True))
    _assert_conversation_kernel(names, case)
    quiet = _tape(eng)
    for k in TAPE:
        np.testing.assert_array_equal(quiet[k], plain[k], err_msg=k)
    # with it: streams 9 / 10, key eval_seed, the host's count of evaluation conversations since the setter call
    eng.set_message_noise(S1, S2, dev=True, eval_seed=nr.EVAL_SEED)
    taken = []
    for c1 in range(3):
        eng.eval_steps(xs[0], xs[1], xs[2], 1, 2, eng.eval_acc())
        tp = _tape(eng)
        _compare(tp, _oracle(case, nr.EVAL_SEED, c1, nr.EVAL_STREAMS, False), "eval %d/%s" % (c1, case))
        taken.append(tp)
    assert np.abs(taken[0]["z"][0] - taken[1]["z"][0]).max() > 0.1 and np.abs(taken[1]["z"][0] - taken[2]["z"][0]).max() > 0.1
    eng.set_message_noise(S1, S2, dev=True, eval_seed=nr.EVAL_SEED)   # the setter resets the count: one call of three conversations
    eng.eval_steps(torch.cat([xs[0]] * 3), torch.cat([xs[1]] * 3), xs[2], 3, 2, eng.eval_acc())
    last = _tape(eng)
    for k in TAPE:
        np.testing.assert_array_equal(last[k], taken[2][k], err_msg=k)
    assert int(eng.tape["counter"][0]) == 0                           # evaluations leave the minibatch counter alone
    # a training minibatch afterwards draws as if no evaluation had run
    eng.forward(*xs, seed=0, train=True, run_all=True)
    n_z, _ = nr.noise_fields(0, 1, T, B, W)
    np.testing.assert_allclose(_tape(eng, ("z",))["z"][0] - plain["z"][0], S1 * n_z[0], atol=ATOL, rtol=0)
    # a corruption mask is applied to the noisy message: |clean + sigma n - m|
    mask = (np.arange(W) % 3 == 0).astype(np.uint8)
    eng.set_message_noise(S1, S2, dev=True, eval_seed=nr.EVAL_SEED)
    eng.forward(*xs, train=False, run_all=True, corrupt_mask=mask)
    tp = _tape(eng)
    e_z, _ = nr.noise_fields(nr.EVAL_SEED, 0, T, B, W, nr.EVAL_STREAMS)
    np.testing.assert_allclose(tp["z"][0], np.abs(plain["z"][0] + S1 * e_z[0] - mask), atol=ATOL, rtol=0)
    want = _oracle(case, nr.EVAL_SEED, 0, nr.EVAL_STREAMS, False, mask=mask)
    for k in ("z", "w", "y", "ps"):
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg="masked " + k)


# ------------------------------------------------------------------ 5. the agent modules
def _game(meta, **kw):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = common.flags_from_meta(meta)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", **kw)
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    return game, eng, fl


def _module_conversation(game, eng, x, desc, T, train):
    """The conversation out of Sender.forward / Receiver.forward calls.  Training: every agent-level call starts a minibatch of its
    own, so the counter is put back in front of each one and the whole conversation draws with counter 1, as exchange()'s did."""
    S, R = game.modules["sender"], game.modules["receiver"]
    S.train(train); R.train(train)
    R.reset_state()
    zs, ws, w_in = [], [], None
    with torch.no_grad():
        for t in range(T):
            if train:
                eng.tape["counter"][0] = 0
            z, _ = S(x, w_in, None, t)
            if train:
                eng.tape["counter"][0] = 0
            _, (w_in, _), _ = R(z, desc)
            zs.append(z.clone()); ws.append(w_in.clone())
    torch.cuda.synchronize()
    return torch.stack(zs).cpu().numpy(), torch.stack(ws).cpu().numpy()


@pytest.mark.parametrize("case", ["G256", "M"])
def test_module_forward_gives_the_messages_of_exchange(case):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    game, eng, fl = _game(meta, seed=9, noise_sen=S1, noise_rec=S2, noise_dev=True)
    assert eng.noise == (S1, S2, True)
    xs, _ = _inputs(meta, eng)
    args = dict(data=xs[0], target=xs[1], desc=xs[2], break_early=False)
    out = game.exchange(dict(args, train=True))
    assert int(eng.tape["counter"][0]) == 1
    z_ex, w_ex = torch.stack(out[1][0]).cpu().numpy(), torch.stack(out[2][0]).cpu().numpy()
    n_z, _ = nr.noise_fields(9, 1, T, B, W)
    np.testing.assert_allclose(z_ex[0] - _clean_z0(meta, xs), S1 * n_z[0], atol=ATOL, rtol=0)      # sen_feats hold the noisy messages
    z_m, w_m = _module_conversation(game, eng, xs[0], xs[2], T, True)
    np.testing.assert_allclose(z_m, z_ex, atol=ATOL, rtol=0)
    np.testing.assert_allclose(w_m, w_ex, atol=ATOL, rtol=0)
    # evaluation under noise_dev: set_noise resets the count, so exchange() and the module loop both run conversation 0
    game.set_noise(S1, S2)
    out = game.exchange(dict(args, train=False))
    z_ex, w_ex = torch.stack(out[1][0]).cpu().numpy(), torch.stack(out[2][0]).cpu().numpy()
    e_z, _ = nr.noise_fields(9, 0, T, B, W, nr.EVAL_STREAMS)         # (the game's seed keys its evaluation draws)
    np.testing.assert_allclose(z_ex[0] - _clean_z0(meta, xs, train=False), S1 * e_z[0], atol=ATOL, rtol=0)
    game.set_noise(S1, S2)
    z_m, w_m = _module_conversation(game, eng, xs[0], xs[2], T, False)
    np.testing.assert_allclose(z_m, z_ex, atol=ATOL, rtol=0)
    np.testing.assert_allclose(w_m, w_ex, atol=ATOL, rtol=0)
    z_2, _ = _module_conversation(game, eng, xs[0], xs[2], T, False)  # the next sender step 0 begins conversation 1
    assert np.abs(z_2[0] - z_m[0]).max() > 0.1


# ------------------------------------------------------------------ 6. gradients
def _grads(game, agents=PAIR):
    return {a: {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
                for k, p in game.modules[a].named_parameters()} for a in agents}


def _zero(game):
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)


def _assert_close(got, want, label):
    """tests/test_channel_grad_gpu.py: atol 2e-5 max(1, max|g|) + rtol 1e-3 |g| per tensor."""
    bad = []
    for a in want:
        for k, w in want[a].items():
            g, w = got[a][k].detach().double().cpu(), w.detach().double().cpu()
            tol = 2e-5 * max(1.0, float(w.abs().max())) + 1e-3 * w.abs()
            err = (g - w).abs()
            print("%s %s.%s max|g| %.4e max err %.3e" % (label, a, k, float(w.abs().max()), float(err.max())))
            if not bool((err <= tol).all()):
                bad.append("%s %s.%s: max err %.3e (max|g| %.3e)" % (label, a, k, float(err.max()), float(w.abs().max())))
    assert not bad, "\n".join(bad)


def _f64_models(meta):
    models = cpu_ref.build_agents(common.flags_from_meta(meta))
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    return models


def _host(meta):
    x, target, desc, _ = common.case_inputs(meta, 0)
    return x, target, desc


@pytest.mark.parametrize("channel", [False, True], ids=["per-agent", "channel"])
@pytest.mark.parametrize("case", ["G256", "M"])
def test_vjp_matches_float64(case, channel):
    """A seeded random linear functional of every differentiable output at every executed step against float64 autograd on the
    GPU's trajectory, the restated noise a constant of the graph."""
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    game, eng, fl = _game(meta, seed=4, autograd=True, channel_grad=channel, noise_sen=S1, noise_rec=S2)
    xs, _ = _inputs(meta, eng)
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], train=True, break_early=False))
    c1 = int(eng.tape["counter"][0])
    n = len(out[3])
    gpu_out = dict(sen=out[1][0], y=out[3], ps=out[0][2], w=out[2][0])
    rs = np.random.RandomState(99)
    coef = {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in lst] for k, lst in gpu_out.items()}
    _zero(game)
    loss = sum((c.float().cuda() * v).sum() for k in gpu_out for c, v in zip(coef[k], gpu_out[k]))
    names = _scopes(eng, loss.backward)
    assert ("k_vjp_channel" in names) == channel and ("k_vjp_sen" in names) != channel, names
    got = _grads(game)
    n_z, n_w = nr.noise_fields(4, c1, T, B, W)
    models = _f64_models(meta)
    x, _, desc = _host(meta)
    ref = nr.f64_outputs(models, fl, x, desc, eng.tape, n, n_z, n_w, channel=channel)
    for k in gpu_out:                                                 # the forward the gradients belong to is the noisy one
        for t in range(n):
            np.testing.assert_allclose(gpu_out[k][t].detach().cpu().numpy().reshape(ref[k][t].shape), ref[k][t].detach().numpy(),
                                       atol=ATOL, rtol=0, err_msg="%s[%d]" % (k, t))
    sum((c * v.view_as(c)).sum() for k in gpu_out for c, v in zip(coef[k], ref[k])).backward()
    want = channel_ref.grads_of(models)
    assert float(want["sender"]["image_layer.weight"].abs().max()) > 1e-2
    _assert_close(got, want, "%s/%s" % (case, "channel" if channel else "per-agent"))


def _nll(out, target):
    return F.nll_loss(F.log_softmax(out[3][-1], dim=1), target)


@pytest.mark.parametrize("case", ["G256", "M"])
def test_loss_on_y_alone_reaches_the_sender_through_the_noisy_channel(case):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    game, eng, fl = _game(meta, seed=4, autograd=True, channel_grad=True, noise_sen=S1, noise_rec=S2)
    xs, _ = _inputs(meta, eng)
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], train=True, break_early=False))
    c1 = int(eng.tape["counter"][0])
    _zero(game)
    _nll(out, xs[1]).backward()
    torch.cuda.synchronize()
    got = _grads(game)
    models = _f64_models(meta)
    x, target, desc = _host(meta)
    y64 = nr.f64_outputs(models, fl, x, desc, eng.tape, len(out[3]), *nr.noise_fields(4, c1, T, B, W), channel=True)["y"]
    F.nll_loss(F.log_softmax(y64[-1], dim=1), torch.from_numpy(target)).backward()
    want = channel_ref.grads_of(models)
    gmax = float(want["sender"]["image_layer.weight"].abs().max())
    assert gmax > 100 * 2e-5 * max(1.0, gmax)                         # the comparison cannot pass by both sides being ~ 0
    _assert_close(got, want, "nll on y/" + case)


def test_three_sgd_steps_move_both_agents():
    meta = nr.meta_of("M")
    game, eng, fl = _game(meta, seed=4, autograd=True, channel_grad=True, noise_sen=S1, noise_rec=S2)
    start = {a: {k: p.detach().clone() for k, p in game.modules[a].named_parameters()} for a in PAIR}
    opts = {a: torch.optim.SGD(game.modules[a].parameters(), lr=1e-2) for a in PAIR}
    xs, _ = _inputs(meta, eng)
    losses = []
    for i in range(3):
        out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], train=True, break_early=False))
        assert int(eng.tape["counter"][0]) == i + 1
        for a in PAIR:
            opts[a].zero_grad()
        loss = _nll(out, xs[1])
        loss.backward()
        for a in PAIR:
            opts[a].step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    now = {a: dict(game.modules[a].named_parameters()) for a in PAIR}
    # (the receiver's message head w is reached only through the sender's next step: it moves because the gradient crosses the channel)
    for a, k in [("sender", k) for k in start["sender"]] + [("receiver", k) for k in ("rnn.weight_ih", "rnn.weight_hh", "y1.weight", "w.weight")]:
        assert not torch.equal(now[a][k].detach(), start[a][k]), "%s.%s has not moved" % (a, k)


# ------------------------------------------------------------------ 7. off is off
@pytest.mark.parametrize("case", ["A", "M"])
def test_cleared_and_never_set_handles_are_the_same(case):
    meta = nr.meta_of(case)
    never = common.make_engine(meta)
    cleared = _engine(meta, dev=True)
    xs, ud = _inputs(meta, never, _uniforms(case, meta))
    noisy_plan = cleared.plan_text()
    assert "message noise" in noisy_plan and "message noise" not in never.plan_text()
    cleared.forward(*xs, train=False, run_all=True)                   # a noisy evaluation in between changes nothing that trains
    cleared.set_message_noise(None, None)
    assert cleared.noise is None and cleared.plan_text() == never.plan_text()
    runs = []
    for eng in (never, cleared):
        names = _scopes(eng, lambda: eng.forward(*xs, *ud, seed=0, train=True, run_all=True))
        tape = _tape(eng)
        names += _scopes(eng, lambda: eng.train_step(*xs, *ud, seed=0))
        torch.cuda.synchronize()
        runs.append((names, tape, eng.tape["losses"].cpu().numpy().copy(), eng.flat_params.cpu().numpy().copy()))
    assert runs[0][0] == runs[1][0] and not [n for n in runs[0][0] if "noise" in n], runs[0][0]
    for k in TAPE:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k], err_msg=k)
    np.testing.assert_array_equal(runs[0][2], runs[1][2])
    np.testing.assert_array_equal(runs[0][3], runs[1][3])
    # new sigmas on a noisy handle select nothing
    cleared.set_message_noise(S1, S2, dev=True)
    assert cleared.plan_text() == noisy_plan
    a = _scopes(cleared, lambda: cleared.train_step(*xs, *ud, seed=0))
    cleared.set_message_noise(0.1, 0.05)
    assert cleared.plan_text() == noisy_plan and cleared.noise == (0.1, 0.05, False)
    b = _scopes(cleared, lambda: cleared.train_step(*xs, *ud, seed=0))
    assert a == b and nr.SCOPES[case] in a, (a, b)
    cleared.set_message_noise(0.0, S2)                                # one clean message: still a noise handle
    assert cleared.plan_text() == noisy_plan
    cleared.forward(*xs, *ud, seed=0, train=True, run_all=True)
    np.testing.assert_allclose(_tape(cleared, ("z",))["z"][0], _clean_z0(meta, xs), atol=ATOL, rtol=0)


# ------------------------------------------------------------------ 8. refusals
def test_refusals_and_the_setting_stays():
    from multimodalgame_amd.engine import Engine
    meta = nr.meta_of("G256")
    eng = _engine(meta)
    lib, f = eng.lib, C.c_float
    for bad in (-0.1, float("nan"), float("inf")):
        for args in ((f(bad), f(0.2)), (f(0.3), f(bad))):
            assert lib.mmg_set_message_noise(eng.handle, args[0], args[1], 0, 0) < 0
            assert b"mmg_set_message_noise" in lib.mmg_last_error() and b"standard deviation" in lib.mmg_last_error()
        with pytest.raises(ValueError):
            eng.set_message_noise(bad, 0.2)
    assert eng.noise == (S1, S2, False) and "message noise" in eng.plan_text()          # the setting before stays
    with pytest.raises(_lib.MmgError, match="mmg_set_sender_variant.*message noise"):
        eng.set_sender_variant("prod")
    eng.set_message_flipout(0.25, 0.25)                               # flips on a continuous handle: kept, and nothing happens
    xs, _ = _inputs(meta, eng)
    eng.forward(*xs, seed=0, train=True, run_all=True)
    n_z, _ = nr.noise_fields(0, 1, *nr.dims(meta))
    np.testing.assert_allclose(_tape(eng, ("z",))["z"][0] - _clean_z0(meta, xs), S1 * n_z[0], atol=ATOL, rtol=0)
    kw = common.engine_kwargs(meta)
    variant = Engine(device="cuda:0", **kw)
    variant.set_sender_variant("prod")
    with pytest.raises(_lib.MmgError, match="mmg_set_message_noise.*sender variant"):
        variant.set_message_noise(S1, S2)
    variant.set_message_noise(None, None)                             # clearing is always allowed
    binary = Engine(device="cuda:0", **dict(kw, use_binary=True))
    with pytest.raises(_lib.MmgError, match="mmg_set_message_noise.*mmg_set_message_flipout"):
        binary.set_message_noise(S1, S2)
    D = kw["n_classes"]
    attn = Engine(device="cuda:0", attn_dim=8, n_words=2 * D, **kw)
    with pytest.raises(_lib.MmgError, match="mmg_set_message_noise.*desc_attn"):
        attn.set_message_noise(S1, S2)
    vattn = Engine(device="cuda:0", vattn=(8, 4, 0), **kw)
    with pytest.raises(_lib.MmgError, match="mmg_set_message_noise.*visual_attn"):
        vattn.set_message_noise(S1, S2)
    assert lib.mmg_set_message_noise(None, f(0.1), f(0.1), 0, 0) < 0
