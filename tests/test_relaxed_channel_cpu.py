"""Relaxed messages (include/mmg.h: mmg_set_message_relaxation) without a GPU.

1. The entry is declared, exported and bound; mmg_version() stays 3; "zs" / "ws" are the last entries of the plain tape and every
   entry in front of them sits where the list's own sizes put it (nothing moved); the refusals that need no device.
2. mmg_plan_for with bit 3 selects the generic per-sample family at config 1's shape; without the bit the plan text is the recorded one.
3. Game's argument refusals.
4. The float64 reference (tests/relaxed_ref.py) checks itself on channel_ref.cpu_tape()'s stand-in: soft mode is smooth (finite
   differences == autograd under test_channel_grad_cpu's gradcheck bound), hard mode's forward values are the bits and its gradient
   is soft mode's rule, soft > 0.5 exactly when u < p.
5. What the seeds of tests/test_relaxed_channel_gpu.py reach, asserted here where a search is cheap.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import cpu_ref
from tests import channel_ref, common, relaxed_cases as rc, relaxed_ref
from tests.test_channel_grad_cpu import N_CLASSES, TINY, _zero
from tests.test_plan_cpu import caps_line, entry, plan, switches  # noqa: F401  (switches: a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the entry, the tape, the host-only refusals
def test_entry_is_declared_exported_and_bound():
    from multimodalgame_amd import _lib
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    m = re.search(r"int\s+mmg_set_message_relaxation\s*\(([^)]*)\)", header)
    assert m, "include/mmg.h does not declare mmg_set_message_relaxation"
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["h", "tau_sen", "tau_rec", "hard"]
    assert "#define MMG_VERSION 3" in header
    assert "mmg_set_message_relaxation" in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.mmg_set_message_relaxation.argtypes) == 4
    assert lib.mmg_version() == 3
    assert _lib.PLAN_RELAX == 8


@pytest.mark.parametrize("shape", ["c1", "odd"])
def test_zs_and_ws_are_the_last_tape_entries_and_nothing_moved(shape):
    from multimodalgame_amd import _lib
    kw = dict(batch=16, n_classes=30, feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=100, bas_hidden=500, max_exchange=10)
    if shape == "odd":
        kw.update(batch=5, n_classes=7, h_dim=100, w_dim=50, rec_hidden=128, max_exchange=3)
    cfg = _lib.make_config(**kw)
    table = _lib.tape_table(cfg)
    T, B, W = kw["max_exchange"], kw["batch"], kw["w_dim"]
    assert [e["name"] for e in table[-3:]] == ["vtables", "zs", "ws"]
    assert table[-2]["dims"] == [T, B, W] and table[-1]["dims"] == [T, B, W] and table[-1]["dtype"] == 0
    size = {0: 4, 1: 1, 2: 4, 3: 8}
    o = 0
    for e in table:                                             # every entry starts where the entries in front of it end
        assert e["offset"] == o, e["name"]
        o += (int(np.prod(e["dims"])) * size[e["dtype"]] + 255) & ~255
    assert o == int(_lib.load().mmg_workspace_bytes(C.byref(cfg)))
    # an attention handle keeps its own arrays behind the plain tape, the two new entries included
    attn = _lib.tape_table(cfg, 8, 3 * kw["n_classes"])
    assert [e["name"] for e in attn[:len(table)]] == [e["name"] for e in table] and attn[len(table)]["name"] == "attn_set"
    assert [e["offset"] for e in attn[:len(table)]] == [e["offset"] for e in table]


def test_refusals_that_need_no_device():
    from multimodalgame_amd import _lib
    from multimodalgame_amd.engine import Engine
    lib = _lib.load()
    assert lib.mmg_set_message_relaxation(None, 1.0, 1.0, 0) < 0
    eng = Engine.__new__(Engine)                                # (no handle: the argument checks come first)
    for args in ((1.0, None), (None, 1.0), (0.0, 1.0), (1.0, -0.5), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            eng.set_message_relaxation(*args)
    assert Engine.relaxation is None
    sig = inspect.signature(Engine.set_message_relaxation).parameters
    assert list(sig)[1:] == ["tau_sen", "tau_rec", "hard"] and sig["hard"].default is False


# ------------------------------------------------------------------ 2. the selection
def test_plan_for_selects_the_generic_family(switches):
    from multimodalgame_amd import _lib
    e = entry("c1")
    assert plan(e).splitlines() == e["plan"] + [caps_line(e["caps"])]           # without the bit: the recorded text
    assert e["plan"][0].startswith("mmg_create: family 0 ")
    relaxed = plan(e, flags=_lib.PLAN_RELAX).splitlines()
    variant = plan(e, flags=_lib.PLAN_VARIANT).splitlines()
    assert relaxed[0].startswith("mmg_create: family 3 ") and " game_ok 0 " in relaxed[0]
    assert " tile_ok 0 " in relaxed[1] and " mc 0 fast 0 rc 0 " in relaxed[1]
    assert relaxed == variant                                   # cleared exactly as a sender variant clears
    assert plan(e, flags=_lib.PLAN_RELAX | _lib.PLAN_NO_ROLES).splitlines()[0].startswith("mmg_create: family 3 (0 fast, 1 mc, 2 tile, 3 generic) no_roles 1 ")
    with pytest.raises(_lib.MmgError):
        plan(e, flags=_lib.PLAN_RELAX | _lib.PLAN_FLIPS)
    with pytest.raises(_lib.MmgError):
        plan(e, flags=_lib.PLAN_RELAX | _lib.PLAN_VARIANT)
    # continuous messages: the flag is carried and nothing happens, as for the flips
    cont = dict(rc.engine_kwargs("c1_soft"), use_binary=False, fixed_exchange=True, entropy_s=None, entropy_sen=None, entropy_rec=None)
    assert _lib.plan_for(_lib.make_config(**cont), e["caps"], _lib.PLAN_RELAX) == _lib.plan_for(_lib.make_config(**cont), e["caps"], 0)
    # the 512-thread shape stays in the generic family too
    assert _lib.plan_for(_lib.make_config(**rc.engine_kwargs("w512_hard")), e["caps"], _lib.PLAN_RELAX).startswith("mmg_create: family 3 ")


# ------------------------------------------------------------------ 3. Game's arguments
def _modules(fl):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    return sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0), Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden)


def test_game_argument_refusals():
    from multimodalgame_amd.game import Game, relax_setting
    fl = cpu_ref.Flags(**dict(TINY, use_binary=True))
    relax = dict(tau_sen=1.0, tau_rec=2.0, hard=True)
    ok = dict(flags=fl, device="cpu", autograd=True, channel_grad=True)
    game = Game(*_modules(fl), relax=relax, **ok)
    assert game.relax == (1.0, 2.0, True)
    assert inspect.signature(Game.__init__).parameters["relax"].default is None
    game.set_relaxation(0.5, 0.25)
    assert game.relax == (0.5, 0.25, False)
    game.set_relaxation(None, None)
    assert game.relax is None
    for bad in (dict(tau_sen=1.0), dict(tau_sen=1.0, tau_rec=0.0), dict(tau_sen=-1.0, tau_rec=1.0), dict(tau_sen=float("nan"), tau_rec=1.0),
                dict(tau_sen=1.0, tau_rec=1.0, soft=True)):
        with pytest.raises(ValueError):
            Game(*_modules(fl), relax=bad, **ok)
    with pytest.raises(ValueError):
        game.set_relaxation(1.0, None)
    for kw in (dict(autograd=False, channel_grad=True), dict(autograd=True, channel_grad=False), dict()):
        with pytest.raises(ValueError, match="autograd=True and channel_grad=True"):
            Game(*_modules(fl), flags=fl, device="cpu", relax=relax, **kw)
    with pytest.raises(ValueError, match="binary"):
        Game(*_modules(cpu_ref.Flags(**dict(TINY, use_binary=False))), relax=relax,
             **dict(ok, flags=cpu_ref.Flags(**dict(TINY, use_binary=False))))
    for kw in (dict(flipout_sen=0.1), dict(sender_mix="prod"), dict(ignore_receiver=True)):
        with pytest.raises(NotImplementedError):
            Game(*_modules(fl), relax=relax, **dict(ok, **kw))
    game = Game(*_modules(fl), relax=relax, **ok)
    with pytest.raises(NotImplementedError, match="world > 1"):
        game.set_parallel(0, 2)
    with pytest.raises(NotImplementedError, match="REINFORCE"):
        game.train_step(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 6))
    game.modules["sender"].train()
    with pytest.raises(NotImplementedError, match="relaxed"):            # the module-level autograd nodes
        game.modules["sender"](torch.zeros(3, 8), None, None, 0)
    with pytest.raises(NotImplementedError, match="relaxed"):
        game.modules["receiver"](torch.zeros(3, 4), torch.zeros(3, 6))
    assert relax_setting((1, 2, 0)) == (1.0, 2.0, False) and relax_setting(None) is None


# ------------------------------------------------------------------ 4. the reference checks itself
def _case(seed=11):
    fl = cpu_ref.Flags(**dict(TINY, use_binary=True))
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=seed)
    models = {k: m.double() for k, m in models.items()}
    x, target, desc = cpu_ref.synthetic_batch(fl.batch_size, N_CLASSES, fl.img_feat_dim, fl.wv_dim, seed=seed + 1)
    tp = channel_ref.cpu_tape(models, fl, x, desc, fl.max_exchange, seed=seed + 2)
    u = relaxed_ref.uniforms_of_cpu_tape(fl, fl.batch_size, fl.max_exchange, seed=seed + 2)
    return fl, models, x, target, desc, tp, u


def _functional(outs, seed=99):
    rs = np.random.RandomState(seed)
    keys = ("sen", "y", "ps", "w")
    coef = {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in outs[k]] for k in keys}
    return sum((c * v).sum() for k in keys for c, v in zip(coef[k], outs[k]))


class _Conversation(nn.Module):
    def __init__(self, models, fl, x, desc, tp, u, relax, frozen):
        super().__init__()
        self.agents = nn.ModuleDict(models)
        self.a = (fl, x, desc, tp, fl.max_exchange, relax, u, frozen)

    def forward(self):
        return _functional(relaxed_ref.f64_outputs(dict(self.agents.items()), *self.a))


def test_soft_mode_is_smooth_finite_differences_agree_with_autograd():
    fl, models, x, target, desc, tp, u = _case()
    frozen = {}
    conv = _Conversation(models, fl, x, desc, tp, u, (0.7, 1.5, False), frozen)
    conv()                                                      # records the constants: dbar and the ReLU sides
    names = [k for k, _ in conv.named_parameters() if k.split(".")[1] in channel_ref.CHANNEL_AGENTS]
    assert len(names) == 7 + 15
    params = tuple(p.detach().clone().requires_grad_(True) for k, p in conv.named_parameters() if k in names)

    def fn(*tensors):
        return torch.func.functional_call(conv, dict(zip(names, tensors)), ())

    assert torch.autograd.gradcheck(fn, params, eps=1e-6, atol=1e-6, rtol=1e-4)     # (test_channel_grad_cpu's bound)


def test_hard_mode_forward_is_the_bits_and_its_gradient_is_the_soft_rule():
    fl, models, x, target, desc, tp, u = _case()
    n, relax = fl.max_exchange, (0.7, 1.5, True)
    out = relaxed_ref.f64_outputs(models, fl, x, desc, tp, n, relax, u)
    for t in range(n):
        for msg, bits, soft in ((out["z"][t], tp["z"][t], out["zs"][t]), (out["wm"][t], tp["w"][t], out["ws"][t])):
            assert torch.equal(msg.detach(), bits) and set(bits.unique().tolist()) <= {0.0, 1.0}
            assert float((soft.detach() - bits).abs().max()) > 1e-2            # the relaxation is no copy of the bits
    # the stand-in is the unrelaxed conversation of the same uniforms: a hard relaxed conversation draws the very same bits
    conv = relaxed_ref.conversation(models, fl, x, desc, (u[0], np.zeros((n, fl.batch_size, 1)), u[1]), relax)
    assert torch.equal(conv["z"], tp["z"]) and torch.equal(conv["w"], tp["w"])
    # d message / d logit = soft (1 - soft) / tau: the gradient of the hard graph is that of the soft rule evaluated on the bits'
    # trajectory -- a hand-written surrogate with the same forward value
    _zero(models)
    _functional(out).backward()
    got = channel_ref.grads_of(models)
    _zero(models)
    S, Rc = models["sender"], models["receiver"]
    d64, x64 = torch.as_tensor(desc).double(), torch.as_tensor(x).double()
    B, R = fl.batch_size, fl.rec_hidden
    outs = {k: [] for k in ("sen", "y", "ps", "w")}
    h, w_in = torch.zeros(B, R, dtype=torch.float64), None
    for t in range(n):
        c = torch.sigmoid(S.code_bias.view(1, -1)).expand(B, fl.rec_w_dim) if t == 0 else w_in
        lz = S.binary_layer(torch.tanh(S.image_layer(x64) + S.code_layer(c)))
        zs = relaxed_ref.soft_sample(lz, u[0][t], relax[0]).detach()
        z = tp["z"][t] + (lz - lz.detach()) * zs * (1 - zs) / relax[0]
        h = Rc.rnn(z, h)
        pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, -1, R)
        y = Rc.y2(torch.relu(pre).view(-1, R)).view(B, -1)
        lw = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(torch.softmax(y, 1).detach() @ d64)))
        ws = relaxed_ref.soft_sample(lw, u[1][t], relax[1]).detach()
        w_in = tp["w"][t] + (lw - lw.detach()) * ws * (1 - ws) / relax[1]
        for k, v in (("sen", torch.sigmoid(lz)), ("y", y), ("ps", torch.sigmoid(Rc.s(h))), ("w", torch.sigmoid(lw))):
            outs[k].append(v)
    _functional(outs).backward()
    want = channel_ref.grads_of(models)
    for a in want:
        for k, v in want[a].items():
            assert float(v.abs().max()) > 0, (a, k)
            assert torch.allclose(got[a][k], v, rtol=1e-10, atol=1e-12 * float(v.abs().max())), (a, k)


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_soft_rounds_to_the_bit_on_every_draw(case):
    tp = rc.cpu_conversation(case)
    for soft, bits in ((tp["zs"], tp["bits_z"]), (tp["ws"], tp["bits_w"])):
        assert torch.equal((soft > 0.5).double(), bits)


# ------------------------------------------------------------------ 5. what the GPU tests' seeds reach
@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_the_seeds_reach_what_the_gpu_tests_rely_on(case):
    tp = rc.cpu_conversation(case)
    meta, relax = rc.CASES[case]
    u_s = torch.from_numpy(np.asarray(rc.inputs(case)[3][1])).double().reshape(tp["ps"].shape)
    assert float((u_s - tp["ps"]).abs().min()) >= 1e-4         # no stop bit that fp32 could decide the other way
    assert float((tp["zs"] - tp["bits_z"]).abs().max()) > 1e-2 and float((tp["ws"] - tp["bits_w"]).abs().max()) > 1e-2
    if not meta["fixed_exchange"]:
        n = relaxed_ref.executed_steps(tp["s"])
        mask = torch.cumprod(tp["s"], 0)                        # running stop mask after step t
        print(case, "executed steps", n, "still running after each step", mask.sum((1, 2)).tolist())
        if case.startswith("c1"):
            assert n >= 2 and 0 < float(mask[n - 2].sum()) < meta["batch"]     # some sample stops before the last executed step


def test_three_sgd_steps_decrease_the_nll_in_float64():
    nll = rc.cpu_sgd_nll()
    print("float64 NLL of the minibatch before and after each SGD step:", ["%.6f" % v for v in nll])
    assert len(nll) == 4 and all(b < a for a, b in zip(nll, nll[1:]))
    assert nll[0] - nll[-1] > 1e-3                              # a fall the fp32 run cannot lose to rounding
