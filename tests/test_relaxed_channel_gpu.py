"""Relaxed messages on the GPU: the Gumbel-sigmoid channel (include/mmg.h: mmg_set_message_relaxation; k_conversation<.., RELAX>,
k_vjp_channel_relax) against the float64 reference of tests/relaxed_ref.py.  Cases, temperatures and seeds: tests/relaxed_cases.py.

1. A hard relaxed conversation is the plain one bit for bit (injected uniforms and Philox); zs / ws match float64.
2. A soft conversation matches float64: z, w, pz, pw, ps, y at 1e-4 absolute (the project's forward bar), the stop bits exactly.
3. The joint VJP against float64 autograd: a seeded random linear functional of (pz, y, ps, pw); one case also d data / d desc.
4. A loss on y alone trains the sender, and differently from the plain straight-through channel.
5. Annealing the temperatures between two exchanges selects nothing anew; the second backward is the new temperatures'.
6. Evaluation is the plain game's, bit for bit (where both run the generic family); exchange + backward twice gives bit-identical
   gradients.
7. Three SGD steps on the NLL (HIP loss kernels) move both agents and lower the minibatch's NLL.
8. The refusals of the ABI, and clearing the setting gives the handle back as it was.

Tolerance of 3-5: the project's bar for a VJP against float64, atol 2e-5 max(1, max|g|) + rtol 1e-3 |g| (test_channel_grad_gpu.py).
Measured on an MI355X, largest |error| over the tensors of a case (its tensor, that tensor's largest |gradient|): odd_soft 2.0e-6
(receiver.y2.weight, 5.0), odd_hard 1.5e-6 (receiver.y2.weight, 5.4), c1_soft 1.4e-5 (receiver.y2.weight, 39.4; the bar there
7.9e-4), w512_hard 1.2e-6 (sender.image_layer.weight, 3.0), d data 1.8e-7, d desc 1.7e-7: every tensor is inside the bar with
the 1 / tau factor, so the bar stands as it is.  The test prints every tensor's figure.
9. The agent-level forwards of a relaxed engine form the same relaxed messages.
"""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import common, relaxed_cases as rc, relaxed_ref
from tests.test_autograd_gpu import _assert_close, _grads, _zero

pytestmark = pytest.mark.gpu

PAIR = rc.PAIR
DEV = torch.device("cuda:0")
# what a training run-all forward of the generic per-sample family writes (conversation, baselines, output selection)
FORWARD_TAPE = ("hx", "Cd", "c", "zr", "a", "z", "pz", "h", "gru", "s", "ps", "y", "dbar", "g", "w", "pw", "mask", "tstar", "lp_z", "ne_z",
                "lp_s", "ne_s", "lp_w", "ne_w", "hid_s", "hid_r", "bs", "br", "outp", "dist", "sm", "logs", "hit")


def _game(case, relax="case", **game_kw):
    """A Game of the case's shape with filled weights; relax: "case" (the case's own), None (the plain channel) or a tuple."""
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    meta = rc.CASES[case][0]
    fl = common.flags_from_meta(meta)
    relax = rc.CASES[case][1] if relax == "case" else relax
    kw = dict(autograd=True, channel_grad=True)
    kw.update(game_kw)
    if relax is not None:
        kw["relax"] = dict(tau_sen=relax[0], tau_rec=relax[1], hard=relax[2])
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", **kw)
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    return game, eng, fl


def _args(case, uniforms=True):
    x, target, desc, (u_z, u_s, u_w) = rc.inputs(case)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = dict(data=d(x), target=d(target), desc=d(desc))
    if uniforms:
        args["uniforms"] = (d(u_z), d(u_s[..., 0]), d(u_w))
    return args


def _exchange(game, fl, args, **kw):
    return game.exchange(dict(args, train=True, break_early=not fl.fixed_exchange, **kw))


def _outputs(out):
    s, sen_w, rec_w, y, bs, br = out
    return dict(sen=sen_w[1], y=y, ps=s[2], w=rec_w[1])


def _coefficients(gpu_out, seed=99):
    rs = np.random.RandomState(seed)
    return {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in lst] for k, lst in gpu_out.items()}


def _functional(outs, coef, cuda):
    return sum(((c.float().cuda() if cuda else c) * v).sum() for k in coef for c, v in zip(coef[k], outs[k]))


def _report(case, got, want):
    worst = (0.0, 0.0)
    for a in want:
        for k, v in want[a].items():
            err = float((got[a][k].double().cpu() - v).abs().max())
            print("%s %s.%s max|g| %.4e max err %.3e" % (case, a, k, float(v.abs().max()), err))
            worst = max(worst, (err, float(v.abs().max())))
    print("%s largest error %.3e (max|g| of that tensor %.4e)" % ((case,) + worst))


def _f64_grads(case, tape, n, relax, make_loss, leaves=()):
    """Float64 autograd of make_loss(outputs) through the relaxed graph on the recorded trajectory."""
    meta = rc.CASES[case][0]
    x, target, desc, u = rc.inputs(case)
    models = rc.f64_models(case)
    x_in, d_in = leaves if leaves else (x, desc)
    out = relaxed_ref.f64_outputs(models, common.flags_from_meta(meta), x_in, d_in, tape, n, relax, u)
    make_loss(out).backward()
    from tests.channel_ref import grads_of
    return grads_of(models)


# ------------------------------------------------------------------ 1. hard forward == the plain forward
@pytest.mark.parametrize("injected", [True, False], ids=["injected", "philox"])
def test_hard_forward_is_the_plain_forward_bit_for_bit(injected):
    case = "odd_hard"
    args = _args(case, uniforms=injected)
    tapes = []
    for relax in ("case", None):
        game, eng, fl = _game(case, relax=relax)
        assert eng.plan_text().startswith("mmg_create: family 3 ")            # both on k_conversation
        with torch.no_grad():
            _exchange(game, fl, args)
        torch.cuda.synchronize()
        tapes.append({k: eng.tape[k].clone() for k in FORWARD_TAPE + ("zs", "ws")})
    hard, plain = tapes
    for k in FORWARD_TAPE:
        assert torch.equal(hard[k], plain[k]), k
    assert set(hard["z"].unique().tolist()) <= {0.0, 1.0} and set(hard["w"].unique().tolist()) <= {0.0, 1.0}
    assert float(plain["zs"].abs().max()) == 0.0 and float(plain["ws"].abs().max()) == 0.0      # only a relaxed handle writes them
    if injected:
        ref = rc.cpu_conversation(case)
        for k in ("zs", "ws"):
            err = float((hard[k].double().cpu() - ref[k]).abs().max())
            print("%s %s max err %.3e" % (case, k, err))
            assert err <= 1e-4, k


# ------------------------------------------------------------------ 2. soft forward against float64
@pytest.mark.parametrize("case", ["odd_soft", "c1_soft"])
def test_soft_forward_matches_float64(case):
    game, eng, fl = _game(case)
    with torch.no_grad():
        out = game.exchange(dict(_args(case), train=True, break_early=False))
    torch.cuda.synchronize()
    ref = rc.cpu_conversation(case)
    for k in ("z", "w", "pz", "pw", "ps", "y", "zs", "ws"):
        err = float((eng.tape[k].double().cpu().reshape(ref[k].shape) - ref[k]).abs().max())
        print("%s %s max err %.3e" % (case, k, err))
        assert err <= 1e-4, k
    assert torch.equal(eng.tape["s"].double().cpu().reshape(ref["s"].shape), ref["s"])
    assert torch.equal(eng.tape["z"], eng.tape["zs"]) and torch.equal(eng.tape["w"], eng.tape["ws"])
    # exchange() hands out the relaxed values, detached
    assert torch.equal(torch.stack(out[1][0]), eng.tape["z"]) and torch.equal(torch.stack(out[2][0]), eng.tape["w"])
    assert float((eng.tape["z"] * (1 - eng.tape["z"])).max()) > 1e-2          # no bits
    if case == "c1_soft":
        n = relaxed_ref.executed_steps(ref["s"])
        with torch.no_grad():
            out = _exchange(game, fl, _args(case))
        assert len(out[3]) == n and 2 <= n < fl.max_exchange


# ------------------------------------------------------------------ 3. the joint VJP against float64 autograd
@pytest.mark.parametrize("case", ["odd_soft", "odd_hard", "c1_soft", "w512_hard"])
def test_relaxed_vjp_matches_float64(case):
    relax = rc.CASES[case][1]
    input_grad = case == "odd_soft"
    game, eng, fl = _game(case, input_grad=input_grad)
    if case == "w512_hard":
        from tests import generic_inst
        assert generic_inst.conv_threads(**generic_inst.dims_of(rc.CASES[case][0])) == 512
    args = _args(case)
    if input_grad:
        args["data"].requires_grad_(True); args["desc"].requires_grad_(True)
    out = _exchange(game, fl, args)
    gpu_out = _outputs(out)
    n = len(out[3])
    assert all(v.requires_grad for lst in gpu_out.values() for v in lst) and not out[1][0][0].requires_grad
    if relax[2]:
        assert set(torch.stack(out[1][0]).unique().tolist()) <= {0.0, 1.0}
    coef = _coefficients(gpu_out)
    _zero(game)
    eng.set_profiling(True)
    _functional(gpu_out, coef, True).backward()
    torch.cuda.synchronize()
    names = [name for name, _ in eng.kernel_times()]
    eng.set_profiling(False)
    assert "k_vjp_channel" in names and "k_vjp_rec" not in names and "k_vjp_sen" not in names, names
    got = _grads(game, PAIR)
    if case == "c1_soft":
        assert 2 <= n < fl.max_exchange, "the case should stop early, behind more than one step"
        assert int(out[0][0][n - 1].sum()) < rc.CASES[case][0]["batch"], "some sample should have stopped before the last step"
    x, _, desc, _ = rc.inputs(case)
    leaves = (torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(desc).double().requires_grad_(True)) if input_grad else ()
    want = _f64_grads(case, eng.tape, n, relax, lambda o: _functional(o, coef, False), leaves)
    if input_grad:
        got["inputs"] = dict(data=args["data"].grad, desc=args["desc"].grad)
        want["inputs"] = dict(data=leaves[0].grad, desc=leaves[1].grad)
        assert float(want["inputs"]["data"].abs().max()) > 0 and float(want["inputs"]["desc"].abs().max()) > 0
    _report(case, got, want)
    _assert_close(got, want, case, atol=2e-5, scale_atol=True)


# ------------------------------------------------------------------ 4. a loss on y alone
def test_loss_on_y_alone_trains_the_sender_unlike_straight_through():
    case = "odd_hard"
    relax = rc.CASES[case][1]
    args = _args(case)
    grads, coef = {}, None
    for key, rx in (("relaxed", "case"), ("straight_through", None)):
        game, eng, fl = _game(case, relax=rx)
        out = _exchange(game, fl, args)
        coef = coef or _coefficients(dict(y=out[3]))            # a seeded linear functional of the class logits, nothing else
        _zero(game)
        _functional(dict(y=out[3]), coef, True).backward()
        torch.cuda.synchronize()
        grads[key] = _grads(game, PAIR)
        if rx is not None:
            want = _f64_grads(case, eng.tape, len(out[3]), relax, lambda o: _functional(o, coef, False))
    for k, v in want["sender"].items():
        gmax = float(v.abs().max())
        assert gmax > 100 * 2e-5 * max(1.0, gmax), k             # every sender tensor, code_bias included: none passes by being ~ 0
        assert float(grads["relaxed"]["sender"][k].abs().max()) > 0, k
    _report(case + " f(y)", grads["relaxed"], want)
    _assert_close(grads["relaxed"], want, "loss on y", atol=2e-5, scale_atol=True)
    # the same bits, the same uniforms: the relaxation's derivative is not the straight-through one
    differs = []
    for k, v in want["sender"].items():
        tol = 2e-5 * max(1.0, float(v.abs().max())) + 1e-3 * v.abs()
        differs.append(bool(((grads["straight_through"]["sender"][k].double().cpu() - v).abs() > tol).any()))
    assert all(differs), differs


# ------------------------------------------------------------------ 5. annealing
def test_annealing_selects_nothing_and_the_backward_follows():
    case = "odd_soft"
    game, eng, fl = _game(case)
    args = _args(case)
    plan = eng.plan_text()
    coef = None
    for relax in (rc.CASES[case][1], (0.4, 2.0, False)):
        game.set_relaxation(*relax)
        assert eng.plan_text() == plan and eng.relaxation == relax
        out = _exchange(game, fl, args)
        gpu_out = _outputs(out)
        coef = coef or _coefficients(gpu_out)
        _zero(game)
        loss = _functional(gpu_out, coef, True)
        game.set_relaxation(3.0, 3.0)                           # a later annealing step does not reach a recorded graph
        loss.backward()
        torch.cuda.synchronize()
        assert eng.relaxation == (3.0, 3.0, False)
        got = _grads(game, PAIR)
        want = _f64_grads(case, eng.tape, len(out[3]), relax, lambda o: _functional(o, coef, False))
        _assert_close(got, want, "tau %s" % (relax,), atol=2e-5, scale_atol=True)
    # one call's own setting: exchange_args["relax"] on a game that holds another
    out = _exchange(game, fl, dict(args, relax=dict(tau_sen=0.4, tau_rec=2.0)))
    _zero(game)
    _functional(_outputs(out), coef, True).backward()
    torch.cuda.synchronize()
    _assert_close(_grads(game, PAIR), want, "exchange_args relax", atol=2e-5, scale_atol=True)
    assert eng.relaxation == (3.0, 3.0, False) and eng.plan_text() == plan


# ------------------------------------------------------------------ 6. evaluation and determinism
@pytest.mark.parametrize("case", ["odd_soft", "w512_hard"])
def test_evaluation_is_the_plain_games_bit_for_bit(case):
    """Shapes at which a plain handle runs the generic per-sample family too (another family rounds differently): the RELAX
    instantiation's evaluation conversation is k_conversation's arithmetic, instruction for instruction."""
    args = _args(case)
    runs = []
    for relax in ("case", None):
        game, eng, fl = _game(case, relax=relax)
        assert eng.plan_text().startswith("mmg_create: family 3 ")
        out = game.exchange(dict(args, train=False, break_early=False))
        flat = [t.clone() for grp in out[:3] for lst in grp for t in lst if t is not None] + [t.clone() for t in out[3]]
        acc = game.eval_accumulator(rc.CASES[case][0]["n_classes"], fl.top_k_train)
        game.eval_steps(args["data"], args["target"], args["desc"], 1, acc)
        torch.cuda.synchronize()
        runs.append((flat, acc.fetch(), {k: eng.tape[k].clone() for k in ("z", "w", "pz", "pw", "y", "s", "ps", "mask")}))
    assert len(runs[0][0]) == len(runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    for k, v in runs[0][1].items():
        assert np.array_equal(np.asarray(v), np.asarray(runs[1][1][k])), k
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k
    assert set(runs[0][2]["z"].unique().tolist()) <= {0.0, 1.0}              # a relaxed pair is deployed discrete


def test_exchange_and_backward_twice_are_bit_identical():
    case = "c1_soft"
    args = _args(case)
    game, eng, fl = _game(case)
    twice, coef = [], None
    for _ in range(2):
        gpu_out = _outputs(_exchange(game, fl, args))
        coef = coef or _coefficients(gpu_out)
        _zero(game)
        _functional(gpu_out, coef, True).backward()
        torch.cuda.synchronize()
        twice.append(_grads(game, PAIR))
    for a in PAIR:
        for k, g in twice[0][a].items():
            assert torch.equal(g, twice[1][a][k]), (a, k)
            assert float(g.abs().max()) > 0, (a, k)


# ------------------------------------------------------------------ 7. three SGD steps through the HIP loss kernels
def test_three_sgd_steps_lower_the_nll():
    from multimodalgame_amd import losses
    case = rc.SGD_CASE
    game, eng, fl = _game(case)
    args = _args(case)
    params = [p for a in PAIR for p in game.modules[a].parameters()]
    start = {a: {k: p.detach().clone() for k, p in game.modules[a].named_parameters()} for a in PAIR}
    opt = torch.optim.SGD(params, lr=rc.SGD_LR)
    nll = []
    for i in range(rc.SGD_STEPS + 1):
        out = _exchange(game, fl, args)
        masks = out[0][0]
        y_masks = [torch.min(1 - m1, m2) for m1, m2 in zip(masks[1:], masks[:-1])]
        loss = losses.reward_and_nll(out[3], y_masks, args["target"])[2]
        nll.append(float(loss.detach()))
        if i < rc.SGD_STEPS:
            opt.zero_grad()
            loss.backward()
            opt.step()
    torch.cuda.synchronize()
    want = rc.cpu_sgd_nll()
    print("NLL per step: GPU %s float64 %s" % (["%.6f" % v for v in nll], ["%.6f" % v for v in want]))
    assert nll[-1] < nll[0]
    for a in PAIR:
        still = {k for k, p in game.modules[a].named_parameters() if torch.equal(p.detach(), start[a][k])}
        # (the NLL does not read the stop head; receiver.y2.bias: softmax is shift invariant, its exact gradient is 0)
        assert still <= ({"s.weight", "s.bias", "y2.bias"} if a == "receiver" else set()), (a, still)


# ------------------------------------------------------------------ 8. refusals and clearing
def test_refusals_name_the_setter_and_clearing_restores_the_handle():
    from multimodalgame_amd import _lib
    from multimodalgame_amd.engine import Engine
    case = "c1_hard"
    meta = rc.CASES[case][0]
    kw = rc.engine_kwargs(case)
    eng = Engine(device="cuda:0", **kw)
    fresh = Engine(device="cuda:0", **kw)
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    for e in (eng, fresh):
        e.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    a = _args(case)
    x, target, desc, u = a["data"], a["target"], a["desc"], a["uniforms"]
    B, W, H, R, D, T = kw["batch"], kw["w_dim"], kw["h_dim"], kw["rec_hidden"], kw["n_classes"], kw["max_exchange"]
    before = eng.plan_text()
    assert before.startswith("mmg_create: family 0 ")
    # the setter's own refusals: the setting before stays
    for tau in ((-1.0, 1.0), (1.0, float("nan")), (0.0, 1.0), (1.0, 0.0)):
        assert eng.lib.mmg_set_message_relaxation(eng.handle, tau[0], tau[1], 0) < 0
        assert b"mmg_set_message_relaxation" in eng.lib.mmg_last_error()
        assert eng.plan_text() == before
    eng.set_message_flipout(p_sen=0.1)
    with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation.*flips"):
        eng.set_message_relaxation(1.0, 1.0)
    eng.set_message_flipout()
    eng.set_sender_variant(mix="prod")
    with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation.*variant"):
        eng.set_message_relaxation(1.0, 1.0)
    eng.set_sender_variant()
    assert eng.plan_text() == before
    cont = Engine(device="cuda:0", **dict(kw, use_binary=False, fixed_exchange=True, entropy_s=None, entropy_sen=None, entropy_rec=None))
    with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation.*binary"):
        cont.set_message_relaxation(1.0, 1.0)
    attn = Engine(device="cuda:0", attn_dim=8, n_words=2 * D, **kw)
    with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation.*desc_attn"):
        attn.set_message_relaxation(1.0, 1.0)
    vattn = Engine(device="cuda:0", vattn=(8, 4, 0), **kw)
    with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation.*visual_attn"):
        vattn.set_message_relaxation(1.0, 1.0)
    del cont, attn, vattn
    # a relaxed handle
    eng.set_message_relaxation(1.0, 2.0, hard=True)
    relaxed = eng.plan_text()
    assert relaxed.startswith("mmg_create: family 3 ") and relaxed != before
    eng.set_message_relaxation(0.5, 0.25)                       # moving the temperatures selects nothing
    assert eng.plan_text() == relaxed
    with pytest.raises(_lib.MmgError, match="relaxed messages"):
        eng.set_message_flipout(p_rec=0.2)
    with pytest.raises(_lib.MmgError, match="relaxed messages"):
        eng.set_sender_variant(ignore_code=True)
    eng.forward(x, target, desc, *u, train=True, run_all=True)
    f = lambda *shape: torch.zeros(*shape, device=DEV)
    refused = {
        "mmg_train_step": lambda: eng.train_step(x, target, desc, *u),
        "mmg_train_steps": lambda: eng.train_steps(x, target, desc, 1),
        "mmg_dp_train_step": lambda: eng.dp_train_step(x, target, desc, *u, reduce=False),
        "mmg_dp_train_steps": lambda: eng.dp_train_steps(x, target, desc, 1, reduce=False),
        "mmg_backward": lambda: eng.backward(x, target, desc),
        "mmg_exchange_vjp": lambda: eng.vjp("sender", T, x, desc, dz=f(T, B, W)),
        "mmg_sender_vjp": lambda: eng.sender_vjp(x, None, 0, f(B, H), f(B, W), dout=f(B, W)),
        "mmg_receiver_vjp": lambda: eng.receiver_vjp(f(B, W), desc, None, f(B, R), f(B, D), f(B, W), f(B, 1), dy=f(B, D)),
        "mmg_baseline_vjp": lambda: eng.baseline_vjp("baseline_rec", None, f(B, W), f(B, R), dscore=f(B, 1)),
    }
    for name, call in refused.items():
        with pytest.raises(_lib.MmgError, match=r"%s is not available.*mmg_set_message_relaxation" % name):
            call()
    for agent in ("receiver", "baseline_rec", "baseline_sen"):
        with pytest.raises(_lib.MmgError, match="mmg_set_message_relaxation"):
            eng.vjp(agent, T, x, desc)
    eng.loss_stats()                                            # as before
    eng.vjp_channel(T, x, desc, dy=f(T, B, D))
    torch.cuda.synchronize()
    # clearing: the plan text of before, and a training step of a fresh plain handle bit for bit
    eng.set_message_relaxation(None, None)
    assert eng.plan_text() == before and eng.relaxation is None
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    eng.opt_state.zero_()
    eng.tape["counter"][:3].copy_(fresh.tape["counter"][:3])
    start = fresh.flat_params.clone()
    for e in (eng, fresh):
        e.train_step(x, target, desc, *u)
    torch.cuda.synchronize()
    n = eng.n_params
    assert torch.equal(eng.flat_params, fresh.flat_params) and torch.equal(eng.flat_grads[:n], fresh.flat_grads[:n])
    assert torch.equal(eng.tape["losses"], fresh.tape["losses"])
    assert not torch.equal(fresh.flat_params, start)


# ------------------------------------------------------------------ 9. the agent-level entries form relaxed messages too
@pytest.mark.parametrize("case", ["odd_soft", "odd_hard"])
def test_agent_level_forwards_form_relaxed_messages(case):
    game, eng, fl = _game(case)
    args = _args(case)
    x, desc, (u_z, u_s, u_w) = args["data"], args["desc"], args["uniforms"]
    eng.forward(x, args["target"], desc, u_z, u_s, u_w, train=True, run_all=True)
    torch.cuda.synchronize()
    tape = {k: eng.tape[k].clone() for k in ("z", "w", "zs", "ws", "pz", "pw", "h")}
    msg, probs, _ = eng.sender_forward(x, None, 0, True, u_z=u_z[0].contiguous())
    h = torch.zeros(x.size(0), fl.rec_hidden, device=DEV)
    _, _, w, w_probs, _, _ = eng.receiver_forward(tape["z"][0].contiguous(), desc, h, torch.ones(x.size(0), device=DEV), True, 0, True,
                                                 u_s=u_s[0].contiguous(), u_w=u_w[0].contiguous())
    msg1, _, _ = eng.sender_forward(x, tape["w"][0].contiguous(), 1, True, u_z=u_z[1].contiguous())
    torch.cuda.synchronize()
    for got, want in ((msg, tape["z"][0]), (probs, tape["pz"][0]), (w, tape["w"][0]), (w_probs, tape["pw"][0]), (msg1, tape["z"][1]),
                      (h, tape["h"][1]), (eng.tape["zs"][1], tape["zs"][1]), (eng.tape["ws"][0], tape["ws"][0])):
        assert float((got - want).abs().max()) <= 1e-5          # (h_x comes from another launch here: not bit for bit)
    hard = rc.CASES[case][1][2]
    assert (set(msg.unique().tolist()) <= {0.0, 1.0}) == hard and (set(w.unique().tolist()) <= {0.0, 1.0}) == hard
