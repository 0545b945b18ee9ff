"""Autograd through Game.exchange() (opt-in): the four agents' HIP vector-Jacobian products (include/mmg.h: mmg_exchange_vjp).

1. The reference's training block (model.py:1243-1330) written with exchange(autograd=True), cpu_ref's loss helpers and four
   backward() calls gives the gradients of the engine's own fused backward on the same minibatch (Adaptive, Fixed, continuous).
2. A seeded random linear functional of EVERY differentiable output at every executed step -- y_t at non-output steps and rows of
   samples that have already stopped included -- against float64 autograd through cpu_ref's agents with the same weights, on
   the GPU's own discrete trajectory (sampled bits are constants of the graph), one case per forward family.
3. Three minibatches of the reference's loop (autograd, clip_grad_norm_, torch.optim.RMSprop) match three Game.train_step calls.
4. Safety: per-agent backward() == one summed backward(); a second backward raises; a stale tape raises; without the opt-in
   exchange() is unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import common

pytestmark = pytest.mark.gpu

AGENTS = ("receiver", "sender", "baseline_rec", "baseline_sen")
C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01,
          entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6)


def _meta(flags_kw, n_classes, batch, seed_weights=11, seed_data=12, seed_uniforms=13):
    meta = dict(cpu_ref.Flags(**flags_kw).__dict__)
    meta.update(n_classes=n_classes, batch=batch, batch_size=batch, n_minibatches=1, seed_weights=seed_weights,
                seed_data=seed_data, seed_uniforms=seed_uniforms)
    return meta


def _game(meta, autograd=False):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = common.flags_from_meta(meta)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", autograd=autograd)
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    return game, eng


def _inputs(meta, i=0, name=None):
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i, name)
    dev = torch.device("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return x, target, desc, dict(data=d(x), target=d(target), desc=d(desc), uniforms=(d(u_z), d(u_s[..., 0]), d(u_w)))


def _exchange(game, fl, dev_args, autograd=True):
    return game.exchange(dict(dev_args, train=True, break_early=not fl.fixed_exchange, autograd=autograd))


def _reference_losses(fl, out, target):
    """model.py:1248-1305 (cpu_ref.train_minibatch) on CPU copies of exchange()'s lists -- the copies keep the graph."""
    s, sen_w, rec_w, y, bs, br = out
    c = lambda lst: [None if t is None else t.cpu() for t in lst]
    s_masks, s_feats, s_probs = c(s[0]), c(s[1]), c(s[2])
    sen_feats, sen_probs, rec_feats, rec_probs, y, bs, br = c(sen_w[0]), c(sen_w[1]), c(rec_w[0]), c(rec_w[1]), c(y), c(bs), c(br)
    if fl.fixed_exchange:
        binary_s_masks = binary_rec_masks = binary_sen_masks = bas_rec_masks = bas_sen_masks = y_masks = None
    else:
        binary_s_masks, binary_rec_masks, binary_sen_masks = s_masks[:-1], s_masks[1:-1], s_masks[:-1]
        bas_rec_masks = bas_sen_masks = s_masks[:-1]
        y_masks = [torch.min(1 - m1, m2) for m1, m2 in zip(s_masks[1:], s_masks[:-1])]
    outp, _ = cpu_ref.get_rec_outp(y, y_masks)
    dist = F.log_softmax(outp, dim=1)
    nll_loss = F.nll_loss(dist, target)
    logs = dist.detach().gather(1, target.view(-1, 1))
    losses = {"receiver": nll_loss}
    if fl.use_binary:
        loss_rec = nll_loss
        if len(rec_feats[:-1]) > 0:
            loss_rec = loss_rec + cpu_ref.multistep_loss_binary(rec_feats[:-1], rec_probs[:-1], logs, br[:-1], binary_rec_masks,
                                                                fl.entropy_rec)[0]
        if not fl.fixed_exchange:
            loss_rec = loss_rec + cpu_ref.multistep_loss_binary(s_feats, s_probs, logs, br, binary_s_masks, fl.entropy_s)[0]
        losses["receiver"] = loss_rec
        losses["sender"] = cpu_ref.multistep_loss_binary(sen_feats, sen_probs, logs, bs, binary_sen_masks, fl.entropy_sen)[0]
        losses["baseline_rec"] = cpu_ref.multistep_loss_bas(br, logs, bas_rec_masks)
        losses["baseline_sen"] = cpu_ref.multistep_loss_bas(bs, logs, bas_sen_masks)
    return losses


def _grads(game, agents):
    return {a: {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
                for k, p in game.modules[a].named_parameters()} for a in agents}


def _zero(game):
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)


def _assert_close(got, want, label, atol=1e-4, rtol=1e-3, scale_atol=False):
    bad = []
    for a in want:
        for k, w in want[a].items():
            g = got[a][k].detach().double().cpu()
            w = w.detach().double().cpu()
            tol = atol * (max(1.0, float(w.abs().max())) if scale_atol else 1.0) + rtol * w.abs()
            err = (g - w).abs()
            if not bool((err <= tol).all()):
                i = int((err - tol).argmax())
                bad.append("%s %s.%s: max err %.3e at %d (got %.6e want %.6e)" % (label, a, k, float(err.max()), i,
                                                                               float(g.reshape(-1)[i]), float(w.reshape(-1)[i])))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ 1. the reference's training block
@pytest.mark.parametrize("name", ["g2_adaptive_c1", "g3_fixed_c3shard", "g3_continuous"])
def test_reference_block_gives_the_engine_gradients(name):
    _, meta = common.load_golden(name)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    _, target, _, args = _inputs(meta, 0, name)
    out = _exchange(game, fl, args)
    assert out[3][0].requires_grad and out[3][0].grad_fn is not None
    losses = _reference_losses(fl, out, torch.from_numpy(target))
    agents = AGENTS if fl.use_binary else ("receiver",)
    _zero(game)
    for a in agents:                                           # four separate backward() calls, model.py:1309-1328
        losses[a].backward()
    got = _grads(game, agents)
    eng.forward(args["data"], args["target"], args["desc"], *args["uniforms"], train=True, run_all=True)
    eng.loss_stats()
    eng.backward(args["data"], args["target"], args["desc"])
    torch.cuda.synchronize()
    want = {a: {k: v.detach().cpu().clone() for k, v in eng.grads[a].items()} for a in agents}
    _assert_close(got, want, name)


# ------------------------------------------------------------------ 2. general VJP against float64 autograd
def _relu_gpu_mask(pre, gpu_on, eps=1e-4):
    """ReLU mask of the float64 reference; units within eps of the threshold take the side the GPU's own fp32 forward put them
    on (d relu / dx is discontinuous there: both sides are correct)."""
    m = pre > 0
    return torch.where(pre.abs() < eps, gpu_on, m)


def _f64_outputs(models, fl, x, desc, tp, n):
    """The reference's per-agent graphs (model.py:144-238, 303-477, 496-516) in float64 on the GPU's discrete trajectory: the
    sampled / exchanged messages z_t, w_t are the GPU's (constants of the graph, detached as at model.py:807-843)."""
    S, Rc, BS, BR = (models[k].double() for k in ("sender", "receiver", "baseline_sen", "baseline_rec"))
    x64, d64 = torch.from_numpy(x).double(), torch.from_numpy(desc).double()
    B, D, R = x.shape[0], d64.shape[0], fl.rec_hidden
    g = lambda k: tp[k].detach().double().cpu()
    z_gpu, w_gpu = g("z"), g("w")
    vA, vCd = g("vA"), g("vCd")
    out = {k: [] for k in ("sen", "y", "ps", "w", "bs", "br")}
    h = torch.zeros(B, R, dtype=torch.float64)
    for t in range(n):
        h_x = S.image_layer(x64)
        if t == 0:
            h_w = S.code_layer(torch.sigmoid(S.code_bias.view(1, -1))).expand(B, fl.img_h_dim)
        else:
            h_w = S.code_layer(w_gpu[t - 1])
        feats = S.binary_layer(torch.tanh(h_x + h_w))
        out["sen"].append(torch.sigmoid(feats) if fl.use_binary else feats)
        z_t = z_gpu[t]
        h = Rc.rnn(z_t, h)
        out["ps"].append(torch.sigmoid(Rc.s(h)))
        pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, D, R)
        on = _relu_gpu_mask(pre, (vA[t][:, None, :] + vCd[None, :, :]) > 0)
        y = Rc.y2((pre * on).view(B * D, R)).view(B, -1)
        out["y"].append(y)
        dbar = F.softmax(y, dim=1).detach() @ d64
        ws = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(dbar)))
        out["w"].append(torch.sigmoid(ws) if fl.use_binary else ws)
        if fl.use_binary:
            zr = torch.full((B, fl.rec_w_dim), float(fl.first_rec), dtype=torch.float64) if t == 0 else w_gpu[t - 1]
            p1 = BS.linear1(torch.cat([h_x.detach(), zr], 1))
            out["bs"].append(BS.linear2(p1 * _relu_gpu_mask(p1, g("vhid_s")[t] > 0)))
            p1 = BR.linear1(torch.cat([z_t, h.detach()], 1))
            out["br"].append(BR.linear2(p1 * _relu_gpu_mask(p1, g("vhid_r")[t] > 0)))
    return out


FAMILIES = {
    "fast_c2": (dict(C1, batch_size=16), 30, 16),                                            # k_conversation_fast3 / k_game
    "mc_binary": (dict(C1, batch_size=16), 100, 16),                                         # many classes (kernels_mc.h)
    "mc_continuous": (dict(C1, batch_size=16, use_binary=False, fixed_exchange=True, max_exchange=4,
                           entropy_rec=None, entropy_sen=None, entropy_s=None), 100, 16),    # kernels_mc3.h
    "tile": (dict(C1, batch_size=16, img_h_dim=128, rec_w_dim=64, sender_out_dim=64, max_exchange=5), 30, 16),   # kernels_tile.h
    "rc_r256": (dict(C1, batch_size=16, img_h_dim=1024, rec_w_dim=64, sender_out_dim=64, rec_hidden=256, max_exchange=4), 30, 16),
    "odd_generic": (dict(C1, batch_size=5, img_h_dim=100, rec_w_dim=50, sender_out_dim=50, rec_hidden=128, max_exchange=3,
                         fixed_exchange=True), 7, 5),                                    # the reference's default agent sizes
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_vjp_of_a_random_functional_matches_float64(family):
    kw, n_classes, batch = FAMILIES[family]
    meta = _meta(kw, n_classes, batch)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    x, target, desc, args = _inputs(meta)
    s, sen_w, rec_w, y, bs, br = _exchange(game, fl, args)
    n = len(y)
    binary = fl.use_binary
    gpu_out = dict(sen=sen_w[1] if binary else sen_w[0], y=y, ps=s[2], w=rec_w[1] if binary else rec_w[0], bs=bs, br=br)
    rs = np.random.RandomState(99)
    coef = {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in lst] for k, lst in gpu_out.items()}
    loss = sum((c.float().cuda() * v).sum() for k in gpu_out for c, v in zip(coef[k], gpu_out[k]))
    _zero(game)
    loss.backward()
    torch.cuda.synchronize()
    agents = AGENTS if binary else ("receiver", "sender")
    got = _grads(game, agents)
    assert n >= 2 or fl.fixed_exchange, "the case should run more than one step"
    if not fl.fixed_exchange:                                   # rows of samples that stopped before the last step are covered
        assert int(s[0][n - 1].sum()) < batch
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    ref = _f64_outputs(models, fl, x, desc, eng.tape, n)
    loss64 = sum((c * v).sum() for k in gpu_out for c, v in zip(coef[k], ref[k]))
    loss64.backward()
    want = {a: {k: p.grad if p.grad is not None else torch.zeros_like(p) for k, p in models[a].named_parameters()} for a in agents}
    _assert_close(got, want, family, atol=2e-5, scale_atol=True)


# ------------------------------------------------------------------ 3. the reference's loop == Game.train_step
def test_three_minibatches_of_the_reference_loop_match_train_step():
    name = "g2_adaptive_c1"
    _, meta = common.load_golden(name)
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    fused, feng = _game(meta)
    opts = {a: torch.optim.RMSprop(game.modules[a].parameters(), lr=fl.learning_rate) for a in AGENTS}
    for i in range(3):
        _, target, _, args = _inputs(meta, i)
        losses = _reference_losses(fl, _exchange(game, fl, args), torch.from_numpy(target))
        for a in AGENTS:                                        # model.py:1307-1330
            opts[a].zero_grad()
            losses[a].backward()
            torch.nn.utils.clip_grad_norm_(game.modules[a].parameters(), max_norm=1.)
            opts[a].step()
        fused.train_step(args["data"], args["target"], args["desc"], uniforms=args["uniforms"])
    torch.cuda.synchronize()
    got = {a: {k: p.detach() for k, p in game.modules[a].named_parameters()} for a in AGENTS}
    want = {a: {k: v for k, v in feng.params[a].items() if not (a == "receiver" and k == "y2.bias")} for a in AGENTS}
    # (y2.bias: its exact gradient is zero -- softmax is shift invariant -- and both paths step on rounding noise; the parity
    #  tests skip it the same way)
    assert all(bool(torch.equal(p.data, eng.params[a][k])) for a in AGENTS for k, p in game.modules[a].named_parameters())
    _assert_close(got, want, "3 minibatches")


# ------------------------------------------------------------------ 4. safety and no behaviour change
def _c1_game():
    _, meta = common.load_golden("g2_adaptive_c1")
    fl = common.flags_from_meta(meta)
    game, eng = _game(meta, autograd=True)
    _, target, _, args = _inputs(meta, 0)
    return game, eng, fl, torch.from_numpy(target), args


def test_separate_backward_calls_equal_one_summed_backward():
    game, eng, fl, target, args = _c1_game()
    _zero(game)
    for a, l in _reference_losses(fl, _exchange(game, fl, args), target).items():
        l.backward()
    sep = _grads(game, AGENTS)
    _zero(game)
    sum(_reference_losses(fl, _exchange(game, fl, args), target).values()).backward()
    both = _grads(game, AGENTS)
    for a in AGENTS:
        for k in sep[a]:
            assert torch.equal(sep[a][k], both[a][k]), (a, k)


def test_second_backward_and_stale_tape_raise():
    game, eng, fl, target, args = _c1_game()
    losses = _reference_losses(fl, _exchange(game, fl, args), target)
    losses["sender"].backward()
    with pytest.raises(RuntimeError):
        losses["sender"].backward()
    losses = _reference_losses(fl, _exchange(game, fl, args), target)
    _exchange(game, fl, args, autograd=False)                   # rewrites the tape the nodes above were recorded on
    for a in AGENTS:
        with pytest.raises(RuntimeError, match="overwritten"):
            losses[a].backward()
    game.world = 2
    with pytest.raises(NotImplementedError):
        _exchange(game, fl, args)


def test_without_the_opt_in_exchange_is_unchanged():
    game, eng, fl, target, args = _c1_game()
    game.autograd = False
    plain = _exchange(game, fl, args, autograd=False)
    tp = eng.tape
    n = len(plain[3])
    flat = [t for grp in (plain[0], plain[1], plain[2]) for lst in grp for t in lst] + list(plain[3]) + list(plain[4]) + list(plain[5])
    assert all(not t.requires_grad for t in flat if t is not None)
    for key, lst in (("s", plain[0][1]), ("ps", plain[0][2]), ("z", plain[1][0]), ("pz", plain[1][1]), ("w", plain[2][0]),
                     ("pw", plain[2][1]), ("y", plain[3]), ("bs", plain[4]), ("br", plain[5])):
        for t in range(n):
            assert torch.equal(lst[t], tp[key][t]), (key, t)
    for grad_mode, train in ((False, True), (True, False)):     # no_grad() and evaluation: plain tensors even with the opt-in
        with torch.set_grad_enabled(grad_mode):
            out = game.exchange(dict(args, train=train, break_early=True, autograd=True))
        assert not any(t.requires_grad for t in out[3])
    with_graph = _exchange(game, fl, args, autograd=True)
    assert len(with_graph[3]) == n
    for a, b in zip(plain[3] + plain[0][2] + plain[1][1] + plain[2][1] + plain[4] + plain[5],
                    with_graph[3] + with_graph[0][2] + with_graph[1][1] + with_graph[2][1] + with_graph[4] + with_graph[5]):
        assert b.requires_grad and torch.equal(a, b.detach())
