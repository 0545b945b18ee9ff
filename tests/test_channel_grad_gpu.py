"""Gradients through the messages: exchange(channel_grad=True), the joint sender-receiver HIP VJP (include/mmg.h:
mmg_exchange_vjp_channel, kernels_vjp.h: k_vjp_channel).

1. A seeded random linear functional of every differentiable output at every executed step against float64 autograd of the
   channel graph (tests/channel_ref.py) on the GPU's own discrete trajectory, one case per forward family: continuous messages
   (exact) and binary messages (straight-through).
2. A loss on y alone reaches the sender only with the option.
3. exchange(channel_grad=True) equals the same conversation written out of Sender / Receiver module calls with the messages
   not detached: two independent GPU implementations of one graph.
4. Three SGD steps on nll alone train both agents as the float64 reference does.
5. Safety: second backward, stale tape, world > 1, the option off is bit-identical, n_steps out of range.

Tolerance of 1-3: the project's own for a VJP against float64, atol 2e-5 max(1, max|g|) + rtol 1e-3 |g|.  float32 torch autograd of
the same graph misses float64 by 0.8-1.5 % of it on the CPU (largest absolute error 3.5e-5 against gradients up to 37), while
dropping a cross term misses by 30-50 % of max|g| in the sender's tensors.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import channel_ref, common
from tests.test_autograd_gpu import (AGENTS, C1, FAMILIES, _assert_close, _game, _grads, _inputs, _meta, _reference_losses,
                                     _zero)

pytestmark = pytest.mark.gpu

PAIR = ("sender", "receiver")
DEV = torch.device("cuda:0")
NO_ENTROPY = dict(entropy_rec=None, entropy_sen=None, entropy_s=None)
C1_CONTINUOUS = (dict(C1, batch_size=16, use_binary=False, fixed_exchange=True, max_exchange=4, **NO_ENTROPY), 30, 16)
CASES = {
    "fast_c2": FAMILIES["fast_c2"],                             # binary, Adaptive, T 10, B 16, D 30
    "mc_continuous": FAMILIES["mc_continuous"],                 # continuous, Fixed, T 4, D 100
    "tile": FAMILIES["tile"],                                   # binary, H 128, W 64, T 5
    "odd_generic": FAMILIES["odd_generic"],                     # H 100, W 50, R 128, B 5, D 7, T 3, binary
    "odd_generic_continuous": (dict(FAMILIES["odd_generic"][0], use_binary=False, **NO_ENTROPY),) + FAMILIES["odd_generic"][1:],
}


def _exchange(game, fl, dev_args, channel=True, **kw):
    return game.exchange(dict(dev_args, train=True, break_early=not fl.fixed_exchange, autograd=True, channel_grad=channel, **kw))


def _outputs(out, binary):
    s, sen_w, rec_w, y, bs, br = out
    return dict(sen=sen_w[1] if binary else sen_w[0], y=y, ps=s[2], w=rec_w[1] if binary else rec_w[0], bs=bs, br=br)


def _coefficients(gpu_out, seed=99):
    rs = np.random.RandomState(seed)
    return {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in lst] for k, lst in gpu_out.items()}


def _f64_models(meta):
    models = cpu_ref.build_agents(common.flags_from_meta(meta))
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    return models


# ------------------------------------------------------------------ 1. the joint VJP against float64 autograd
@pytest.mark.parametrize("family", sorted(CASES))
def test_channel_vjp_matches_float64(family):
    kw, n_classes, batch = CASES[family]
    meta = _meta(kw, n_classes, batch)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    x, target, desc, args = _inputs(meta)
    out = _exchange(game, fl, args)
    gpu_out = _outputs(out, fl.use_binary)
    n = len(out[3])
    coef = _coefficients(gpu_out)
    loss = sum((c.float().cuda() * v).sum() for k in gpu_out for c, v in zip(coef[k], gpu_out[k]))
    _zero(game)
    eng.set_profiling(True)
    loss.backward()
    torch.cuda.synchronize()
    names = [name for name, _ in eng.kernel_times()]
    eng.set_profiling(False)
    assert "k_vjp_channel" in names and "k_vjp_rec" not in names and "k_vjp_sen" not in names, names
    got = _grads(game, PAIR)
    if family == "fast_c2":
        assert n >= 2, "the case should run more than one step"
        assert int(out[0][0][n - 1].sum()) < batch, "some sample should have stopped before the last step"
    models = _f64_models(meta)
    ref = channel_ref.f64_outputs(models, fl, x, desc, eng.tape, n, channel=True)
    sum((c * v).sum() for k in gpu_out for c, v in zip(coef[k], ref[k])).backward()
    want = channel_ref.grads_of(models)
    for k, v in want["sender"].items():
        print("%s sender.%s max|g| %.4e max err %.3e" % (family, k, float(v.abs().max()),
                                                          float((got["sender"][k].double().cpu() - v).abs().max())))
    _assert_close(got, want, family, atol=2e-5, scale_atol=True)


# ------------------------------------------------------------------ 2. a loss on y alone
def _nll(out, target):
    from multimodalgame_amd.game import get_rec_outp
    outp, _ = get_rec_outp(out[3], None)
    return F.nll_loss(F.log_softmax(outp, dim=1), target)


def test_loss_on_y_alone_reaches_the_sender():
    kw, n_classes, batch = C1_CONTINUOUS
    meta = _meta(kw, n_classes, batch)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    x, target, desc, args = _inputs(meta)
    _zero(game)
    _nll(_exchange(game, fl, args, channel=False), args["target"]).backward()
    for k, p in game.modules["sender"].named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert float(game.modules["receiver"].rnn.weight_ih.grad.abs().max()) > 0
    _zero(game)
    out = _exchange(game, fl, args)
    _nll(out, args["target"]).backward()
    torch.cuda.synchronize()
    got = _grads(game, PAIR)
    models = _f64_models(meta)
    y64 = channel_ref.f64_outputs(models, fl, x, desc, eng.tape, len(out[3]), channel=True)["y"]
    F.nll_loss(F.log_softmax(y64[-1], dim=1), torch.from_numpy(target)).backward()
    want = channel_ref.grads_of(models)
    gmax = float(want["sender"]["image_layer.weight"].abs().max())
    print("image_layer.weight max|g| %.4e" % gmax)
    assert gmax > 100 * 2e-5 * max(1.0, gmax)                   # the comparison cannot pass by both sides being ~ 0
    _assert_close(got, want, "nll on y", atol=2e-5, scale_atol=True)


# ------------------------------------------------------------------ 3. exchange() == the module-level loop
def _module_loop(game, eng, fl, x, desc, T, uniforms):
    """The conversation out of module calls with the messages NOT detached.  Binary: the straight-through line in torch -- the
    bits plus (p - p.detach()), which is p + (bits - p).detach() with the forward value exactly the bits -- and the exchange's
    uniforms handed to the agent-level forwards."""
    S, Rc = game.modules["sender"], game.modules["receiver"]
    S.train(); Rc.train()
    Rc.reset_state()
    binary = fl.use_binary
    sen_fwd, rec_fwd = eng.sender_forward, eng.receiver_forward
    if binary:
        u_z, u_s, u_w = uniforms
        eng.sender_forward = lambda x_, w_, t, train, **k: sen_fwd(x_, w_, t, train, u_z=u_z[t].contiguous(), **k)
        eng.receiver_forward = lambda z_, d_, h_, sp_, first, t, train, **k: rec_fwd(
            z_, d_, h_, sp_, first, t, train, u_s=u_s[t].contiguous(), u_w=u_w[t].contiguous(), **k)
    try:
        outs = dict(sen=[], y=[], ps=[], w=[], bits=[])
        w_in = None
        for t in range(T):
            z, zp = S(x, w_in, None, t)
            z_in = z.detach() + (zp - zp.detach()) if binary else z
            (s, sp), (w, wp), y = Rc(z_in, desc)
            w_in = w.detach() + (wp - wp.detach()) if binary else w
            outs["sen"].append(zp if binary else z); outs["y"].append(y); outs["ps"].append(sp)
            outs["w"].append(wp if binary else w); outs["bits"].append((z.detach(), w.detach()))
    finally:
        if binary:
            del eng.sender_forward, eng.receiver_forward
    return outs


@pytest.mark.parametrize("binary", [False, True])
def test_exchange_equals_the_module_level_loop(binary):
    kw, n_classes, batch = CASES["odd_generic" if binary else "odd_generic_continuous"]
    meta = _meta(kw, n_classes, batch)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    x, target, desc, args = _inputs(meta)
    out = _exchange(game, fl, args)
    gpu_out = {k: v for k, v in _outputs(out, binary).items() if k in ("sen", "y", "ps", "w")}
    coef = _coefficients(gpu_out)
    _zero(game)
    sum((c.float().cuda() * v).sum() for k in gpu_out for c, v in zip(coef[k], gpu_out[k])).backward()
    torch.cuda.synchronize()
    want = _grads(game, PAIR)
    bits = [(z.clone(), w.clone()) for z, w in zip(out[1][0], out[2][0])]
    _zero(game)
    loop = _module_loop(game, eng, fl, args["data"], args["desc"], len(out[3]), args["uniforms"])
    if binary:
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(bits, loop["bits"]))
    sum((c.float().cuda().view_as(v) * v).sum() for k in gpu_out for c, v in zip(coef[k], loop[k])).backward()
    torch.cuda.synchronize()
    got = _grads(game, PAIR)
    assert float(want["sender"]["code_bias"].abs().max()) > 0
    _assert_close(got, want, "module loop", atol=2e-5, scale_atol=True)


# ------------------------------------------------------------------ 4. three SGD steps on nll alone
def test_three_sgd_steps_train_both_agents():
    kw, n_classes, batch = C1_CONTINUOUS
    meta = _meta(kw, n_classes, batch)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    models = {k: m.double() for k, m in _f64_models(meta).items()}
    start = {k: p.detach().clone() for k, p in game.modules["sender"].named_parameters()}
    opts = {a: torch.optim.SGD(game.modules[a].parameters(), lr=1e-2) for a in PAIR}
    opts64 = {a: torch.optim.SGD(models[a].parameters(), lr=1e-2) for a in PAIR}
    for i in range(3):
        x, target, desc, args = _inputs(meta, i)
        out = _exchange(game, fl, args)
        for a in PAIR:
            opts[a].zero_grad()
            opts64[a].zero_grad()
        _nll(out, args["target"]).backward()
        tape = {k: eng.tape[k].detach().clone() for k in ("z", "w", "vA", "vCd")}      # (the next exchange rewrites it)
        y64 = channel_ref.f64_outputs(models, fl, x, desc, tape, len(out[3]), channel=True)["y"]
        F.nll_loss(F.log_softmax(y64[-1], dim=1), torch.from_numpy(target)).backward()
        for a in PAIR:
            torch.nn.utils.clip_grad_norm_(game.modules[a].parameters(), max_norm=1.)
            opts[a].step()
            torch.nn.utils.clip_grad_norm_(models[a].parameters(), max_norm=1.)
            opts64[a].step()
    torch.cuda.synchronize()
    got = {a: {k: p.detach() for k, p in game.modules[a].named_parameters()} for a in PAIR}
    want = {a: {k: p.detach() for k, p in models[a].named_parameters() if not (a == "receiver" and k == "y2.bias")} for a in PAIR}
    # (y2.bias: its exact gradient is zero -- softmax is shift invariant -- both sides step on rounding noise)
    for k, p in got["sender"].items():
        assert not torch.equal(p, start[k]), "sender.%s has not moved" % k
    _assert_close(got, want, "3 SGD steps")


# ------------------------------------------------------------------ 5. safety and no behaviour change
def _c1(**game_kw):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    _, meta = common.load_golden("g2_adaptive_c1")
    fl = common.flags_from_meta(meta)
    if game_kw:
        sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
        receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
        game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                    Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", **game_kw)
        eng = game.engine_for(meta["batch"], meta["n_classes"])
        shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
        eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    else:
        game, eng = _game(meta, autograd=True)
    _, target, _, args = _inputs(meta, 0)
    return game, eng, fl, torch.from_numpy(target), args


def test_second_backward_stale_tape_and_world_raise():
    game, eng, fl, target, args = _c1()
    loss = _nll(_exchange(game, fl, args), args["target"])
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    loss = _nll(_exchange(game, fl, args), args["target"])
    _exchange(game, fl, args)                                   # rewrites the tape the node above was recorded on
    with pytest.raises(RuntimeError, match="sender-receiver node .* overwritten"):       # (the joint node's own message)
        loss.backward()
    game.world = 2
    with pytest.raises(NotImplementedError):
        _exchange(game, fl, args)
    game.world = 1


def test_option_off_is_bit_identical_and_needs_autograd():
    plain_game, _, fl, target, args = _c1()                     # a Game built without the argument
    off_game, _, _, _, _ = _c1(autograd=True, channel_grad=False)
    runs = []
    for game, kw in ((plain_game, {}), (off_game, {}), (off_game, dict(channel_grad=False))):
        out = game.exchange(dict(args, train=True, break_early=True, **kw))
        _zero(game)
        for l in _reference_losses(fl, out, target).values():
            l.backward()
        flat = [t for grp in out[:3] for lst in grp for t in lst if t is not None] + list(out[3]) + list(out[4]) + list(out[5])
        runs.append((flat, _grads(game, AGENTS)))
    for flat, grads in runs[1:]:
        assert len(flat) == len(runs[0][0]) and all(torch.equal(a.detach(), b.detach()) for a, b in zip(runs[0][0], flat))
        for a in AGENTS:
            for k, g in grads[a].items():
                assert torch.equal(g, runs[0][1][a][k]), (a, k)
    on_game, _, _, _, _ = _c1(autograd=False, channel_grad=True)            # the option without the opt-in: plain tensors
    for kw, grad_mode in ((dict(train=True), True), (dict(train=False, autograd=True), True), (dict(train=True, autograd=True), False)):
        with torch.set_grad_enabled(grad_mode):
            out = on_game.exchange(dict(args, break_early=True, **kw))
        assert not any(t.requires_grad for t in out[3])


def test_n_steps_out_of_range_is_an_error():
    game, eng, fl, target, args = _c1()
    _exchange(game, fl, args)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    for n in (0, fl.max_exchange + 1):
        status = eng.lib.mmg_exchange_vjp_channel(eng.handle, n, ptr(args["data"]), ptr(args["desc"]), None, None, None, None, stream)
        assert status < 0
        assert b"n_steps" in eng.lib.mmg_last_error()
