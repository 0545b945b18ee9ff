"""Visual attention (-visual_attn / -attn_extra_context, model.py:80-86, 114-142, 168-195; include/mmg.h: mmg_vattn_create,
mmg_set_data_context) on the GPU, against the CPU oracle with the wrapped sender (tests/visual_attn_ref.py) and the g13 fixtures of
the reference's own code: training-mode and evaluation conversations, training minibatches (losses, every tensor's gradient, updated
parameters), the agent-level Sender.forward, the refusals.

Shapes (tests/visual_attn_ref.py): A config 1's agents on a 512 x 8 x 8 map, A = 256, a 1000-d context, 16 samples, 4 steps;
B H 40, W 12, R 20, V 12, K 70, C 18, a 2 x 3 map, A = 5, G = 7, 5 samples, 3 steps; C = B without a context; D = B on a 1 x 1 map;
E = B on a 9 x 9 map.  tests/test_visual_attn_cpu.py checks what the seeds reach.  Tolerances: the project's bar -- forward
quantities 1e-4 absolute, gradients and updated parameters 1e-4 + 1e-3 |v|, bits exact (every training draw is 1e-4 away from its probability, no evaluation probability within 1e-4
of 0.5)."""
import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, agents, game as G
from multimodalgame_amd.engine import Engine
from tests import common, visual_attn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 21
ATOL = 1e-4
SHAPES = sorted(ref.SHAPES)
MODES = sorted(ref.MODES)
TAPE_KEYS = ("s", "ps", "z", "pz", "w", "pw", "y", "bs", "br", "vattn_alpha", "vattn_xa", "vattn_hx")
NAMES = {"vattn_alpha": "alpha", "vattn_xa": "x_attn", "vattn_hx": "h_x"}
_CACHE = {}


def _once(key, make):
    """One oracle run per key, shared by the tests that need it and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _vattn(m):
    h, w = m["map_hw"]
    return (m["vattn_dim"], h * w, m["context_dim"])


def _engine(m, seed=None):
    """A visual-attention engine with the seeded weights of the case."""
    eng = Engine(vattn=_vattn(m), **common.engine_kwargs(m))
    eng.load_state_dicts(ref.state_dicts(m, seed=seed))
    return eng


def _inputs(m, eng, uniforms=None, i=0):
    _, target, desc, u = common.case_inputs(m, 0)
    x, g = ref.feature_map(m, i)
    u_z, u_s, u_w = uniforms if uniforms is not None else u
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    uh = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (u_z, np.asarray(u_s).reshape(u_s.shape[0], -1), u_w))
    return (d(x.reshape(x.shape[0], x.shape[1], -1)), d(target), d(desc)), tuple(d(a) for a in uh), d(g)


def _tape(eng, keys=TAPE_KEYS):
    torch.cuda.synchronize()
    eng.check_sync()
    return {NAMES.get(k, k): eng.tape[k].cpu().numpy().copy() for k in keys}


def _scopes(eng, call):
    eng.set_profiling(True)
    call()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _assert_attention_kernels(names):
    """The attention instantiations ran; the plain k_conversation (whose sender reads tape.hx) did not."""
    assert "k_vattn_prep" in names and "k_conversation_vattn" in names, names
    assert "k_conversation" not in names and "k_prep+h_x" not in names, names


def _compare_conversation(tp, want, binary=True, exact=True, train=False, label=""):
    if exact:
        for k in ("s", "z", "w") if binary else ("s",):
            np.testing.assert_array_equal(tp[k].reshape(want[k].shape), want[k], err_msg=k)
    keys = ("ps", "pz", "pw", "y") if binary else ("ps", "z", "w", "y")
    for k in keys + ("alpha", "x_attn", "h_x") + (("bs", "br") if train and binary else ()):
        err = np.abs(tp[k].reshape(want[k].shape) - want[k]).max()
        print("%s %s: max |gpu - oracle| = %.3e" % (label, k, err))
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)


def _check_alpha(alpha, m):
    n = alpha.shape[-1]
    np.testing.assert_allclose(alpha.sum(-1), 1.0, atol=1e-5)
    assert (alpha[0] == np.float32(1.0) / np.float32(n)).all()            # model.py:177-180: exactly 1 / N at t == 0
    if n == 1:
        assert (alpha == 1.0).all()
    elif m["shape"] in "AB":                                              # attention matters (tests/test_visual_attn_cpu.py)
        assert np.abs(alpha[1:] - 1.0 / n).max() > 1e-2


# ------------------------------------------------------------------ 1. the run-all conversation, training and evaluation
@pytest.mark.parametrize("shape", SHAPES)
def test_training_conversation_matches_the_wrapped_oracle(shape):
    m = ref.meta(shape, "adaptive")
    u = _once(("u", shape), lambda: ref.separated_uniforms(m))
    want = _once(("train", shape), lambda: ref.conversation(m, train=True, uniforms=u))
    eng = _engine(m)
    xs, ud, g = _inputs(m, eng, u)
    eng.set_data_context(g)
    names = _scopes(eng, lambda: eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True))
    _assert_attention_kernels(names)
    tp = _tape(eng)
    _compare_conversation(tp, want, train=True, label=shape + "/train")
    _check_alpha(tp["alpha"], m)


@pytest.mark.parametrize("mode", ["continuous", "fixed"])
def test_training_conversation_of_the_other_modes(mode):
    m = ref.meta("B", mode)
    u = _once(("u", "B", mode), lambda: ref.separated_uniforms(m))
    want = _once(("train", "B", mode), lambda: ref.conversation(m, train=True, uniforms=u))
    eng = _engine(m)
    xs, ud, g = _inputs(m, eng, u)
    eng.set_data_context(g)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    _compare_conversation(_tape(eng), want, binary=m["use_binary"], train=True, label="B/" + mode)


def _evaluation(shape, mode="adaptive", **kw):
    m = ref.meta(shape, mode)
    return m, _once(("eval", shape, mode, tuple(sorted(kw.items()))), lambda: ref.conversation(m, train=False, **kw))


def _compare_evaluation(tp, want, label):
    _compare_conversation(tp, want, exact=False, label=label)
    prod = np.cumprod(want["ps"], 0)                                    # the stop bit rounds the running product (model.py:423-427)
    for bits, p in (("z", want["pz"]), ("w", want["pw"]), ("s", prod)):
        assert (np.abs(p - 0.5) > 1e-4).all()                           # (the data seed leaves no bit out: test_visual_attn_cpu.py)
        np.testing.assert_array_equal(tp[bits].reshape(p.shape), want[bits], err_msg=bits)


@pytest.mark.parametrize("shape", SHAPES)
def test_evaluation_matches_the_wrapped_oracle(shape):
    m, want = _evaluation(shape)
    eng = _engine(m)
    xs, _, g = _inputs(m, eng)
    eng.set_data_context(g)
    names = _scopes(eng, lambda: eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc()))
    _assert_attention_kernels(names)
    assert "k_eval_reduce" in names, names
    tp = _tape(eng)
    _compare_evaluation(tp, want, shape + "/eval")
    _check_alpha(tp["alpha"], m)
    eng.forward(*xs, train=False, run_all=True)                         # the same instantiation behind mmg_exchange_forward
    _compare_evaluation(_tape(eng), want, shape + "/eval forward")


@pytest.mark.parametrize("mode", MODES)
def test_evaluation_matches_the_references_own_numbers(mode):
    """g13_visual_attn_<mode>_eval: the reference's Sender on torch, on the presets' shape."""
    z, m = ref.load_golden("g13_visual_attn_%s_eval" % mode)
    eng = _engine(m)
    xs, _, g = _inputs(m, eng)
    eng.set_data_context(g)
    eng.forward(*xs, train=False, run_all=True)
    tp = _tape(eng)
    n = int(z["eval.n_steps"])
    binary = m["use_binary"]
    for k, zk in (("ps", "s_probs"), ("y", "y"), ("alpha", "alpha")) + ((("pz", "sen_probs"), ("pw", "rec_probs")) if binary else
                                                                      (("z", "sen_feats"), ("w", "rec_feats"))):
        want = z["eval." + zk]
        got = tp[k][:n].reshape(want.shape)
        print("%s %s: max |gpu - reference| = %.3e" % (mode, k, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, atol=ATOL, rtol=0, err_msg=k)
    xa = z["eval.x_attn"]
    np.testing.assert_allclose(tp["x_attn"][:n, :, ::8], xa, atol=ATOL, rtol=0)     # (every sample, every 8th channel)
    if binary:
        for k, zk, pk in (("z", "sen_feats", "sen_probs"), ("w", "rec_feats", "rec_probs")):
            assert (np.abs(z["eval." + pk] - 0.5) > 1e-4).all()
            np.testing.assert_array_equal(tp[k][:n].reshape(z["eval." + zk].shape), z["eval." + zk], err_msg=k)


def test_a_transposed_map_is_far_from_what_the_kernels_compute():
    """x is channel-major, [B, C, N] with the locations contiguous (model.py:171-172 transposes a view).  The GPU agrees with the
    oracle in that layout and is far from the oracle reading the same memory as [B, N, C]."""
    m, want = _evaluation("B")
    _, wrong = _evaluation("B", transposed=True)
    eng = _engine(m)
    xs, _, g = _inputs(m, eng)
    eng.set_data_context(g)
    eng.forward(*xs, train=False, run_all=True)
    tp = _tape(eng, ("vattn_xa", "vattn_hx"))
    np.testing.assert_allclose(tp["x_attn"], want["x_attn"], atol=ATOL, rtol=0)
    assert np.abs(tp["x_attn"] - wrong["x_attn"]).max() > 1e-2 and np.abs(tp["h_x"] - wrong["h_x"]).max() > 1e-2


def test_tables_are_formed_again_after_the_parameters_change():
    """HX / HG come from the CURRENT parameters at every forward entry: a second set of weights on the same engine."""
    m, _ = _evaluation("B")
    eng = _engine(m)
    xs, _, g = _inputs(m, eng)
    eng.set_data_context(g)
    eng.forward(*xs, train=False, run_all=True)
    first = _tape(eng, ("vattn_alpha",))["alpha"]
    eng.load_state_dicts(ref.state_dicts(m, seed=11))
    eng.forward(*xs, train=False, run_all=True)
    want = _once(("eval", "B", "seed11"), lambda: ref.conversation(m, train=False, seed=11))
    tp = _tape(eng)
    assert np.abs(tp["alpha"] - first).max() > 1e-2
    for k in ("alpha", "x_attn", "h_x", "pz", "y"):
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)


def test_eval_steps_advances_through_the_maps_and_the_context():
    """mmg_eval_steps with two batches: batch 1 reads ITS map (B * C * N floats further) and ITS rows of the context."""
    m = ref.meta("B")
    eng = _engine(m)
    (x0, target, desc), _, g0 = _inputs(m, eng, i=0)
    (x1, _, _), _, g1 = _inputs(m, eng, i=1)
    eng.set_data_context(torch.cat([g0, g1]), n=2)
    eng.eval_steps(torch.cat([x0, x1]), torch.cat([target, target]), desc, 2, 2, eng.eval_acc())
    want = _once(("eval", "B", "map1"), lambda: ref.conversation(m, train=False, map_i=1))
    tp = _tape(eng)                                                     # (the tape holds the last batch)
    for k in ("alpha", "x_attn", "h_x", "pz", "y"):
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)
    assert np.abs(want["alpha"] - _evaluation("B")[1]["alpha"]).max() > 1e-2


def test_the_same_conversation_twice_is_bit_identical():
    m = ref.meta("A")
    eng = _engine(m)
    xs, ud, g = _inputs(m, eng)
    eng.set_data_context(g)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    a = _tape(eng)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    b = _tape(eng)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------ 2. the modules: Game.exchange, Sender.forward
class _Flags(object):
    desc_attn, sender_mix, flipout_sen, flipout_rec = False, "sum", None, None
    ignore_receiver = ignore_code = visual_attn = bit_flip = False
    s_prob_prod, first_rec = True, 0.0


def _game(m):
    fl = _Flags()
    for k in ("max_exchange", "fixed_exchange", "entropy_s", "entropy_sen", "entropy_rec", "optim_type", "learning_rate", "top_k_train"):
        setattr(fl, k, m[k])
    G_ = m["context_dim"]
    s = agents.Sender("layer4_2", m["img_feat_dim"], m["img_h_dim"], m["rec_w_dim"], m["sender_out_dim"], m["use_binary"],
                      use_attn=True, attn_dim=m["vattn_dim"], attn_extra_context=G_ > 0, attn_context_dim=G_ or 4096)
    r = agents.Receiver(m["sender_out_dim"], m["wv_dim"], m["rec_hidden"], 1, m["rec_w_dim"], 1, m["use_binary"])
    K = m["baseline_hid_dim"]
    mods = (s, r, agents.Baseline(K, m["img_h_dim"], m["rec_w_dim"], 0), agents.Baseline(K, 0, m["rec_w_dim"], m["rec_hidden"]))
    game = G.Game(*mods, flags=fl, seed=SEED)
    sd = ref.state_dicts(m)
    for mod, a in zip(mods, ("sender", "receiver", "baseline_sen", "baseline_rec")):
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in sd[a].items()})
    return game, mods


@pytest.mark.parametrize("shape", ["B", "C"])
def test_exchange_and_sender_forward_through_the_modules(shape):
    """Game.exchange with the 4-D data and exchange_args["data_context"] (shape C: a context that is given is ignored), then the
    agent-level Sender.forward over t = 0..2 behind reset_state()."""
    m, want = _evaluation(shape)
    game, (sender, receiver, bs, br) = _game(m)
    x, g = ref.feature_map(m)
    _, target, desc, _ = common.case_inputs(m, 0)
    ctx = torch.from_numpy(g) if g is not None else torch.randn(m["batch"], 3)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=False,
                data_context=ctx)
    s, sen_w, rec_w, y, _, _ = G.exchange(sender, receiver, bs, br, args)
    T = m["max_exchange"]
    assert len(sender.attn_scores) == T and tuple(sender.attn_scores[1].shape) == (m["batch"], x.shape[2] * x.shape[3])
    for t in range(T):
        np.testing.assert_allclose(sender.attn_scores[t].cpu().numpy(), want["alpha"][t], atol=ATOL, rtol=0)
        np.testing.assert_allclose(y[t].cpu().numpy(), want["y"][t], atol=ATOL, rtol=0)
        np.testing.assert_array_equal(sen_w[0][t].cpu().numpy(), want["z"][t])
    np.testing.assert_allclose(sender.h_x.cpu().numpy(), want["h_x"][T - 1], atol=ATOL, rtol=0)
    assert [k for k in game.engines] == [(m["batch"], m["n_classes"], m["batch"], 0, x.shape[2] * x.shape[3])]
    # the agent-level call: reset_state() invalidates the cached tables; t == 1 first, as a module-level caller may
    sender.eval()
    dev = game.engine.device
    xd, gd = torch.from_numpy(x).to(dev), None if g is None else torch.from_numpy(g).to(dev)
    for order in ((0, 1, 2), (1, 0, 2)):
        sender.reset_state()
        assert sender.attn_scores == []
        for t in order:
            w = torch.from_numpy(want["w"][t - 1]).to(dev) if t else torch.zeros(m["batch"], m["rec_w_dim"], device=dev)
            msg, probs = sender(xd, w, gd, t)
            np.testing.assert_allclose(probs.cpu().numpy(), want["pz"][t], atol=ATOL, rtol=0)
            np.testing.assert_array_equal(msg.cpu().numpy(), want["z"][t])
            np.testing.assert_allclose(sender.h_x.cpu().numpy(), want["h_x"][t], atol=ATOL, rtol=0)
            np.testing.assert_allclose(sender.attn_scores[-1].cpu().numpy(), want["alpha"][t], atol=ATOL, rtol=0)
        assert len(sender.attn_scores) == 3


def test_game_eval_steps_takes_the_maps_and_the_context_of_every_batch():
    """Game.eval_steps over two batches: data [2 B, C, h, w], data_context [2 B, G]; the tape holds the second batch."""
    m = ref.meta("B")
    game, _ = _game(m)
    (x0, g0), (x1, g1) = ref.feature_map(m, 0), ref.feature_map(m, 1)
    _, target, desc, _ = common.case_inputs(m, 0)
    t2 = torch.from_numpy(np.concatenate([target, target]))
    acc = game.eval_accumulator(m["n_classes"], 2)
    eng = game.eval_steps(torch.from_numpy(np.concatenate([x0, x1])), t2, torch.from_numpy(desc), 2, acc,
                          data_context=torch.from_numpy(np.concatenate([g0, g1])))
    want = _once(("eval", "B", "map1"), lambda: ref.conversation(m, train=False, map_i=1))
    tp = _tape(eng, ("vattn_alpha", "y"))
    np.testing.assert_allclose(tp["alpha"], want["alpha"], atol=ATOL, rtol=0)
    np.testing.assert_allclose(tp["y"].reshape(want["y"].shape), want["y"], atol=ATOL, rtol=0)
    assert acc.fetch()["samples"] == 2 * m["batch"]


def test_game_refusals_that_need_a_gpu():
    m = ref.meta("B")
    game, (sender, receiver, bs, br) = _game(m)
    x, g = ref.feature_map(m)
    _, target, desc, _ = common.case_inputs(m, 0)
    base = dict(target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=False)
    with pytest.raises(ValueError, match="data_context"):                                   # a missing context
        game.exchange(dict(base, data=torch.from_numpy(x)))
    with pytest.raises(ValueError, match=r"\[B, 18, h, w\]"):                               # data that is not 4-D
        game.exchange(dict(base, data=torch.from_numpy(x).view(5, -1), data_context=torch.from_numpy(g)))
    with pytest.raises(ValueError, match="channels"):                                       # the wrong C
        game.exchange(dict(base, data=torch.from_numpy(x[:, :17]), data_context=torch.from_numpy(g)))
    with pytest.raises(ValueError, match="data_context must be"):
        game.exchange(dict(base, data=torch.from_numpy(x), data_context=torch.from_numpy(g[:, :5])))
    with pytest.raises(NotImplementedError, match="h \\* w"):                               # outside the supported range
        game.exchange(dict(base, data=torch.zeros(5, 18, 17, 17), data_context=torch.from_numpy(g)))
    with pytest.raises(ValueError, match="data_context"):                                   # training needs the context as well
        game.train_step(torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc))


# ------------------------------------------------------------------ 3. the handle: what it does not offer raises, never the plain sender
def test_handle_refusals():
    m = ref.meta("B")
    eng = _engine(m)
    xs, ud, g = _inputs(m, eng)
    with pytest.raises(_lib.MmgError, match="mmg_set_data_context"):                        # no context yet
        eng.forward(*xs, train=False, run_all=True)
    eng.set_data_context(g)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    for call, word in ((lambda: eng.dp_train_step(*xs, reduce=False), "data-parallel"),
                       (lambda: eng.set_message_flipout(0.1, None), "mmg_set_message_flipout"),
                       (lambda: eng.set_sender_variant("prod"), "mmg_set_sender_variant")):
        with pytest.raises(_lib.MmgError, match="visual_attn") as e:
            call()
        assert word in str(e.value), str(e.value)
    lib = eng.lib
    for rc in (lib.mmg_exchange_vjp(eng.handle, 1, 1, None, None, None, None, None, None, None, None, None),
               lib.mmg_exchange_vjp_channel(eng.handle, 1, None, None, None, None, None, None, None),
               lib.mmg_vjp_input_grads(eng.handle, 0, 1, None, None, None, None),
               lib.mmg_sender_vjp(eng.handle, None, None, 0, None, None, None, None, None, None, None)):
        assert rc < 0 and b"visual_attn" in lib.mmg_last_error(), lib.mmg_last_error()
    with pytest.raises(_lib.MmgError, match="description attention"):
        Engine(vattn=_vattn(m), attn_dim=4, n_words=7, **common.engine_kwargs(m))
    with pytest.raises(_lib.MmgError, match="one GPU"):
        Engine(vattn=_vattn(m), **common.engine_kwargs(m, global_batch=10))
    plain = Engine(**common.engine_kwargs(m))
    with pytest.raises(_lib.MmgError, match="not a visual-attention"):
        plain.set_data_context(g)


def test_the_presets_shape_at_512_samples_is_inside_the_supported_range():
    m = ref.meta("A", batch=512)
    eng = Engine(vattn=(256, 64, 1000), **common.engine_kwargs(m))
    assert eng.tape["vattn_HX"].shape == (512, 64, 256) and "attn_W_g.weight" in eng.params["sender"]
    biggest = max(v.numel() for k, v in eng.tape.items() if k.startswith("vattn_"))
    assert biggest == 512 * 64 * 256                                     # (nothing of size T B N C or T B N A on its tape)


# ------------------------------------------------------------------ 4. training: one minibatch, two minibatches, the same step twice
GTOL = lambda v: 1e-4 + 1e-3 * np.abs(v)
LOSS_KEYS = ("nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen", "loss_bas_rec", "loss_bas_sen")


def _oracle_training(shape, mode, n=1, update=False):
    m = ref.meta(shape, mode)
    def make():
        us = [ref.separated_uniforms(m)] + [common.case_inputs(m, i)[3] for i in range(1, n)]
        res, models = ref.train_minibatches(m, us, update=update)
        grads = [{a: {k: v.numpy().copy() for k, v in r["grads"].get(a, {}).items()} for a in models} for r in res]
        params = {a: {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()} for a, mod in models.items()}
        losses = [{k: float(r[k].detach()) for k in LOSS_KEYS} for r in res]
        return us, grads, params, losses
    return m, _once(("training", shape, mode, n, update), make)


def _grads(eng):
    torch.cuda.synchronize()
    return {a: {k: v.cpu().numpy().copy() for k, v in d.items()} for a, d in eng.grads.items()}


def _assert_close(got, want, label):
    bad = np.abs(got - want) > GTOL(want)
    print("%s: max |gpu - oracle| = %.3e (largest |v| %.3e)" % (label, np.abs(got - want).max() if got.size else 0.0,
                                                                np.abs(want).max() if want.size else 0.0))
    assert not bad.any(), (label, int(bad.sum()), float(np.abs(got - want).max()))


def _phased_minibatch(m, us, i=0):
    eng = _engine(m)
    xs, ud, g = _inputs(m, eng, us, i=i)
    eng.set_data_context(g)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    eng.loss_stats()
    eng.backward(*xs)
    return eng, xs, ud, g


@pytest.mark.parametrize("shape, mode", [("A", "adaptive"), ("A", "fixed"), ("A", "continuous"), ("B", "adaptive"), ("C", "adaptive"),
                                         ("D", "adaptive")])
def test_training_minibatch_gradients_match_the_wrapped_oracle(shape, mode):
    """Every tensor's gradient of one minibatch (forward, statistics, reverse pass, k_wgrad; no update): the attention tensors,
    image_layer (which gets its t == 0 share through x_attn = the mean), baseline_sen.linear1 (whose first H columns read the
    per-step h_x), and everything else.  attn_U.bias: exactly zero; the three attention biases: array_equal."""
    m, (us, grads, _, losses) = _oracle_training(shape, mode)
    eng, xs, ud, g = _phased_minibatch(m, us[0])
    got = _grads(eng)
    binary = m["use_binary"]
    for a in (("receiver", "sender", "baseline_rec", "baseline_sen") if binary else ("receiver",)):
        for k, want in grads[0][a].items():
            if (a, k) == ("sender", "attn_U.bias"):
                continue
            _assert_close(got[a][k].reshape(want.shape), want, "%s/%s %s.%s" % (shape, mode, a, k))
    if binary:
        sg = got["sender"]
        assert not sg["attn_U.bias"].any() and abs(float(grads[0]["sender"]["attn_U.bias"][0])) < 1e-6
        np.testing.assert_array_equal(sg["attn_W_x.bias"], sg["attn_W_w.bias"])
        if m["context_dim"]:
            np.testing.assert_array_equal(sg["attn_W_x.bias"], sg["attn_W_g.bias"])
        if m["map_hw"] == [1, 1]:                                       # alpha == 1: the attention tensors get exact zeros
            for k in ref.vattn_names(m):
                assert not sg[k].any(), k
        else:
            assert np.abs(sg["attn_W_x.weight"]).max() > 1e-4 and np.abs(sg["attn_U.weight"]).max() > 1e-4
        H = m["img_h_dim"]
        assert np.abs(grads[0]["baseline_sen"]["linear1.weight"][:, :H]).max() > 1e-4
    got_l = eng.losses()
    for k in LOSS_KEYS:
        assert abs(got_l[k] - losses[0][k]) <= 1e-4 + 1e-3 * abs(losses[0][k]), (k, got_l[k], losses[0][k])


@pytest.mark.parametrize("mode", ["adaptive", "fixed"])
def test_training_minibatch_against_the_references_own_gradients(mode):
    """g13: the reference's gradients (norm and strided sample of every sender tensor) of the same minibatch.  The fixture's uniforms
    are the seeded ones; the bits agree because no draw lies within fp32 noise of its probability (checked: the sampled messages of
    the tape equal the fixture's)."""
    z, m = ref.load_golden("g13_visual_attn_" + mode)
    u = common.case_inputs(m, 0)[3]
    eng, xs, ud, g = _phased_minibatch(m, u)
    tp = _tape(eng, ("z", "s", "w"))
    n = int(z["mb0.n_steps"])
    live = z["mb0.s_masks"][:n].astype(bool)                            # [n, B, 1]: rows the reference's losses read
    np.testing.assert_array_equal((tp["z"][:n] * live), z["mb0.sen_feats"] * live)
    got = _grads(eng)["sender"]
    for name in ref.vattn_names(m) + ("image_layer.weight", "image_layer.bias"):
        if name == "attn_U.bias":
            continue
        flat = got[name].reshape(-1)
        want = z["mb0.g.sender.%s.sample" % name]
        _assert_close(flat[::max(1, flat.size // 512)], want, "g13 %s %s" % (mode, name))
        norm = float(z["mb0.g.sender.%s.norm" % name])
        assert abs(np.linalg.norm(flat.astype(np.float64)) - norm) <= 1e-4 + 1e-3 * norm, name


@pytest.mark.parametrize("shape", ["A", "B"])
def test_two_consecutive_minibatches_update_like_the_oracle(shape):
    """Two fused train steps (Game-free: Engine.train_step): HX / HG are formed again from the UPDATED parameters in the second, whose
    map and context are another minibatch's.  Updated parameters of all four agents; attn_U.bias bit-identical (RMSprop: A, Adam: B)."""
    m, (us, _, params, _) = _oracle_training(shape, "adaptive", n=2, update=True)
    eng = _engine(m)
    before = eng.params["sender"]["attn_U.bias"].clone()
    for i in range(2):
        xs, ud, g = _inputs(m, eng, us[i], i=i)
        _, target, desc, _ = common.case_inputs(m, i)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
        eng.set_data_context(g)
        names = _scopes(eng, lambda: eng.train_step(xs[0], d(target), d(desc), *ud, seed=SEED))
        assert "k_vattn_bwd" in names and "k_vattn_dwx" in names and "k_conversation_vattn" in names and "k_conversation" not in names, names
    torch.cuda.synchronize()
    assert torch.equal(eng.params["sender"]["attn_U.bias"], before)
    for a, d_ in params.items():
        for k, want in d_.items():
            # (receiver.y2.bias shifts every class logit alike: its gradient is sum_d dy[d] = 0 in exact arithmetic, what either side
            #  holds is rounding noise that RMSprop's first steps normalise to +-lr, and no output depends on it -- the exclusion
            #  __graft_entry__.smoke() and the plain parity tests make)
            if (a, k) in (("sender", "attn_U.bias"), ("receiver", "y2.bias")):
                continue
            _assert_close(eng.params[a][k].cpu().numpy().reshape(want.shape), want, "%s two steps %s.%s" % (shape, a, k))
    moved = np.abs(params["sender"]["attn_W_x.weight"] - ref.state_dicts(m)["sender"]["attn_W_x.weight"]).max()
    assert moved > 1e-5                                                 # the attention tensors trained


def test_the_same_step_twice_gives_the_same_gradients_bit_for_bit():
    m, (us, _, _, _) = _oracle_training("A", "adaptive")
    a = _grads(_phased_minibatch(m, us[0])[0])
    b = _grads(_phased_minibatch(m, us[0])[0])
    for agent in a:
        for k in a[agent]:
            np.testing.assert_array_equal(a[agent][k], b[agent][k], err_msg=agent + "." + k)


def test_early_exit_training_conversation_hides_the_rows_a_sample_never_took():
    """The fused step's forward stops a sample at its own last step: the (step, sample) rows behind it keep what an EARLIER
    conversation left there.  Same gradients as the run-all pass, after a conversation on other data has filled the tape."""
    m, (us, _, _, _) = _oracle_training("B", "adaptive")
    want = _grads(_phased_minibatch(m, us[0])[0])
    eng = _engine(m)
    xs1, ud1, g1 = _inputs(m, eng, None, i=1)
    eng.set_data_context(g1)
    eng.forward(*xs1, *ud1, seed=SEED, train=True, run_all=True)        # stale rows: another map, other uniforms
    xs, ud, g = _inputs(m, eng, us[0])
    eng.set_data_context(g)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=False, minimal=True)
    eng.loss_stats()
    eng.backward(*xs)
    got = _grads(eng)
    tstar = eng.tape["tstar"].cpu().numpy().reshape(-1)
    assert (tstar < m["max_exchange"] - 1).any()                        # some sample did stop early
    for agent in want:
        for k in want[agent]:
            _assert_close(got[agent][k], want[agent][k], "early exit %s.%s" % (agent, k))


def test_game_train_steps_advances_through_the_maps_and_the_context():
    """Game.train_steps over two minibatches by ONE library call (data [2 B, C, h, w], data_context [2 B, G]) ends with the
    parameters of two Game.train_step calls, bit for bit: mmg_train_steps reads minibatch 1's map and ITS rows of the context."""
    m = ref.meta("B")
    (x0, g0), (x1, g1) = ref.feature_map(m, 0), ref.feature_map(m, 1)
    _, target, desc, _ = common.case_inputs(m, 0)
    ends = []
    for one_call in (False, True):
        game, _ = _game(m)
        dev = game.device
        t, d = torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev)
        if one_call:
            game.train_steps(torch.from_numpy(np.concatenate([x0, x1])), torch.cat([t, t]), d, 2,
                             data_context=torch.from_numpy(np.concatenate([g0, g1])))
        else:
            for x, g in ((x0, g0), (x1, g1)):
                game.train_step(torch.from_numpy(x), t, d, data_context=torch.from_numpy(g))
        torch.cuda.synchronize()
        ends.append({a: {k: v.clone() for k, v in dd.items()} for a, dd in game.engine.params.items()})
    start = ref.state_dicts(m)["sender"]["attn_W_g.weight"]
    assert np.abs(ends[0]["sender"]["attn_W_g.weight"].cpu().numpy() - start).max() > 1e-6
    for a in ends[0]:
        for k in ends[0][a]:
            assert torch.equal(ends[0][a][k], ends[1][a][k]), (a, k)


NOISE = (("sender", "attn_U.bias"), ("receiver", "y2.bias"))


def _g13_minibatch(mode):
    """The g13 fixture of a mode, its seeded (raw) uniforms, and the oracle's minibatch WITH the update on the same inputs."""
    z, m = ref.load_golden("g13_visual_attn_" + mode)
    u = common.case_inputs(m, 0)[3]
    def make():
        res, models = ref.train_minibatches(m, [u], update=True)
        params = {a: {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()} for a, mod in models.items()}
        return params, {k: float(res[0][k].detach()) for k in LOSS_KEYS}
    return z, m, u, _once(("g13 update", mode), make)


@pytest.mark.parametrize("mode", MODES)
def test_training_minibatch_with_its_update_per_mode(mode):
    """One fused training step (Engine.train_step: forward, statistics, reverse pass, k_wgrad, clip norm over the gradient buffer,
    optimizer) per mode on the presets' shape, against the oracle run with the update AND against g13, the reference's own numbers:
    the six losses, the updated parameters of all four agents, and -- from the phased calls on a second engine -- every gradient
    g13 holds, the receiver's in continuous mode included.  Continuous mode trains the receiver alone: every tensor of the sender
    and of both baselines is bit-identical to its start.  Excluded from the parameter comparisons, each for a reason that holds
    between the oracle and the reference as well (tests/test_visual_attn_cpu.py): attn_U.bias (a shift of every score of a softmax:
    exact zero here, asserted bit-identical) and receiver.y2.bias (a shift of every class logit: its gradient is sum_d dy = 0, and
    RMSprop turns what rounding leaves into a step of the size of the learning rate on every side)."""
    z, m, u, (want_p, want_l) = _g13_minibatch(mode)
    binary = m["use_binary"]
    eng = _engine(m)
    start = {a: {k: v.clone() for k, v in d.items()} for a, d in eng.params.items()}
    xs, ud, g = _inputs(m, eng, u)
    eng.set_data_context(g)
    names = _scopes(eng, lambda: eng.train_step(*xs, *ud, seed=SEED))
    assert "k_conversation_vattn" in names and "k_conversation" not in names and ("k_vattn_bwd" in names) == binary, names
    assert "k_gradnorm" in names and "k_opt" in names, names
    torch.cuda.synchronize()
    if binary:                                                          # the sampled bits are the reference's: same trajectory
        n = int(z["mb0.n_steps"])
        live = z["mb0.s_masks"][:n].astype(bool)
        np.testing.assert_array_equal(eng.tape["z"].cpu().numpy()[:n] * live, z["mb0.sen_feats"] * live)
    got_l = eng.losses()
    for i, k in enumerate(LOSS_KEYS):
        for want, who in ((want_l[k], "oracle"), (float(z["mb0.losses"][i]), "g13")):
            print("%s %s: gpu %.6f %s %.6f" % (mode, k, got_l[k], who, want))
            assert abs(got_l[k] - want) <= 1e-4 + 1e-3 * abs(want), (k, who, got_l[k], want)
    for a, d in eng.params.items():
        trained = binary or a == "receiver"
        for k, v in d.items():
            if not trained or (a, k) == ("sender", "attn_U.bias"):
                assert torch.equal(v, start[a][k]), (a, k)               # bit-identical
                continue
            if (a, k) in NOISE:
                continue
            got = v.cpu().numpy()
            _assert_close(got.reshape(want_p[a][k].shape), want_p[a][k], "%s updated %s.%s (oracle)" % (mode, a, k))
            key = "mb0.p.%s.%s.sample" % (a, k)
            flat = got.reshape(-1)
            _assert_close(flat[::max(1, flat.size // 512)], z[key], "%s updated %s.%s (g13)" % (mode, a, k))
    moved = ("receiver", "rnn.weight_hh") if not binary else ("sender", "attn_W_x.weight")      # (continuous: w_h only feeds the detached message)
    assert not torch.equal(eng.params[moved[0]][moved[1]], start[moved[0]][moved[1]])
    # every gradient g13 holds, from the phased calls
    eng2, _, _, _ = _phased_minibatch(m, u)
    got_g = _grads(eng2)
    for a in (("receiver", "sender", "baseline_rec", "baseline_sen") if binary else ("receiver",)):
        for k in eng2.params[a]:
            key = "mb0.g.%s.%s.sample" % (a, k)
            if (a, k) in NOISE or key not in z:
                continue
            flat = got_g[a][k].reshape(-1)
            _assert_close(flat[::max(1, flat.size // 512)], z[key], "%s gradient %s.%s (g13)" % (mode, a, k))
    if not binary:
        assert "mb0.g.receiver.rnn.weight_hh.sample" in z and not got_g["sender"]["attn_W_x.weight"].any()
