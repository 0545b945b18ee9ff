"""Agent modules with the reference's constructor signatures, forward() contracts, side-effect
attributes and state_dict keys (model.py:49-516), backed by the HIP library.

The modules hold ordinary ``nn.Parameter``s so ``state_dict`` / ``load_state_dict`` / ``.cuda()`` /
checkpoints behave as in the reference.  When a :class:`multimodalgame_amd.game.Game` adopts them,
each parameter's storage becomes a view into the engine's flat parameter buffer, which is what the
kernels read and the fused optimizer updates in place.

Without the autograd opt-in, forward() returns plain tensors (no autograd graph): gradients are produced by the hand-written
backward kernels through ``Game.train_step`` -- the counterpart of model.py:1243-1330.

With the opt-in (``Game(..., autograd=True)``), a module in training mode under ``torch.is_grad_enabled()`` returns the same
values, but every call is ONE autograd node whose backward is a HIP vector-Jacobian product of that call alone (include/mmg.h:
mmg_sender_vjp / mmg_receiver_vjp / mmg_baseline_vjp), so a conversation written out of module calls -- the reference's own
exchange() loop, model.py:725-876, or any variation of it -- trains with ``loss.backward()``, ``clip_grad_norm_`` and
``torch.optim``:
  - differentiable outputs: the Sender's probs (binary) or message logits (continuous) and ``sender.h_x``; the Receiver's y,
    s_prob, w_probs (binary) or w logits (continuous), ``receiver.h_z`` and ``receiver.h_w``; the Baselines' score.  The
    sampled bits are non-differentiable outputs.
  - gradients reach the parameters and every floating input that requires grad: the Sender's x and w (at t == 0 the code
    input is sigmoid(code_bias), model.py:196-200), the Receiver's z and previous state (``receiver.h_z`` is the node's output
    and the next call's input: backpropagation through time is torch's own graph), all three Baseline inputs.  softmax(y)
    inside dbar is a constant (model.py:441).  desc is a constant too and a desc that requires grad raises NotImplementedError,
    unless the Game was built with ``input_grad=True``: then the Receiver's node returns d desc of the call as well (include/mmg.h:
    mmg_vjp_input_grads) and torch sums it over the calls.
  - a node reads only its own call's saved inputs and outputs and the parameters, never the engine's tape: exchange(), other
    conversations or eval_forward() in between change nothing.  Parameters that changed between forward and backward raise
    RuntimeError (a library-side update: train_step(s), load_state_dicts, ... -- Engine.param_version; an in-place torch edit:
    torch's own version check).  No double backward; a data-parallel Game (world > 1) raises NotImplementedError.
Each backward returns that call's parameter gradients as fresh tensors; torch accumulates them into ``p.grad`` over the calls.

For the fixed protocol, a training ``Game.exchange()`` with the same opt-in returns outputs with one autograd node per agent
over the whole conversation instead (game.py: _AgentVJP).
"""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import flags as _flags


def xavier_normal(tensor, gain=1.0, generator=None):
    """misc.py:367-385: N(0, gain * sqrt(2 / (fan_in + fan_out)))."""
    fan_out, fan_in = tensor.size(0), tensor.size(1)
    std = gain * math.sqrt(2.0 / (fan_in + fan_out))
    with torch.no_grad():
        return tensor.normal_(0, std, generator=generator)


def _linear_default_(weight, bias, generator=None):
    """torch.nn.Linear.reset_parameters (the Baselines keep the default init, model.py:480-494)."""
    bound = 1.0 / math.sqrt(weight.size(1))
    with torch.no_grad():
        weight.uniform_(-bound, bound, generator=generator)
        if bias is not None:
            bias.uniform_(-bound, bound, generator=generator)


def init_state_dicts(engine, seed=0):
    """Reference initialisation (model.py:90-97, 275-288; Baseline default) for all four agents,
    from one CPU generator so that every rank gets identical weights."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for agent, d in engine.params.items():
        out[agent] = {}
        for name, view in d.items():
            t = torch.zeros(view.shape)
            if agent.startswith("baseline"):
                fan_in = engine.params[agent][name.split(".")[0] + ".weight"].shape[1]
                bound = 1.0 / math.sqrt(fan_in)
                t.uniform_(-bound, bound, generator=g)
            elif t.dim() == 2:
                xavier_normal(t, generator=g)
            elif name == "code_bias":
                t.normal_(generator=g)
            out[agent][name] = t
    return out


class _Agent(nn.Module):
    agent_name = None

    def __init__(self):
        super().__init__()
        self._game = None

    def _bound_game(self, batch_size):
        if self._game is None:
            raise RuntimeError(
                "%s is not attached to a Game: construct multimodalgame_amd.game.Game(sender, receiver, "
                "baseline_sen, baseline_rec, ...) (exchange() does this on first use)" % type(self).__name__)
        return self._game

    def _graph_on(self, game):
        """True when this call records an autograd node (opt-in, training mode, grad mode on)."""
        if not (getattr(game, "autograd", False) and self.training and torch.is_grad_enabled()):
            return False
        if getattr(game, "relax", None):
            raise NotImplementedError("autograd through the agent modules is not available on a game with relaxed messages (the "
                                      "per-call VJPs detach the messages): Game.exchange() carries the gradient through them")
        if game.world > 1:
            raise NotImplementedError("autograd through the agent modules runs on one GPU only (data-parallel training: "
                                      "Game.train_step)")
        return True

    def _spec(self, eng, **kw):
        names = [name for name, _ in self.named_parameters()]
        return dict(kw, eng=eng, agent=self.agent_name, names=names, pver=eng.param_version)


class _CallVJP(torch.autograd.Function):
    """Base of the per-call nodes: forward(ctx, spec, *inputs, *params) runs the engine's forward of one agent call; backward
    runs its HIP VJP (Engine.*_vjp), which overwrites the agent's slice of the gradient buffer, and returns fresh copies of it."""

    @staticmethod
    def _check(ctx):
        saved = ctx.saved_tensors                  # (raises once freed -- a second backward -- or after an in-place edit)
        spec = ctx.spec
        if spec["eng"].param_version != spec["pver"]:
            raise RuntimeError("the %s parameters changed between this forward() and backward() (a train_step, load_state_dicts "
                               "or optimizer update of the library): call backward() before updating them" % spec["agent"])
        return saved

    @staticmethod
    def _param_grads(ctx):
        views = ctx.spec["eng"].grads[ctx.spec["agent"]]
        return tuple(views[name].clone() for name in ctx.spec["names"])


class _SenderCall(_CallVJP):
    """One Sender.forward call.  Outputs: (message bits, probs, h_x) when binary (bits non-differentiable), (logits, h_x) when
    continuous."""

    @staticmethod
    def forward(ctx, spec, x, w, *params):
        eng, t = spec["eng"], spec["t"]
        ctx.spec = spec
        ctx.set_materialize_grads(False)
        msg, probs, h_x = eng.sender_forward(x.contiguous(), None if t == 0 else w.contiguous(), t, True, seed=spec["seed"])
        ctx.save_for_backward(x, None if t == 0 else w, h_x, probs, *params)
        if probs is None:
            return msg, h_x
        ctx.mark_non_differentiable(msg)
        return msg, probs, h_x

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        x, w, h_x, probs = _CallVJP._check(ctx)[:4]
        spec = ctx.spec
        dout, dh_x = (grads[1], grads[2]) if probs is not None else (grads[0], grads[1])
        dx, dw = spec["eng"].sender_vjp(x, w, spec["t"], h_x, probs, dout, dh_x, want_dx=ctx.needs_input_grad[1],
                                        want_dw=ctx.needs_input_grad[2])
        return (None, None if dx is None else dx.view_as(x), None if dw is None else dw.view_as(w)) + _CallVJP._param_grads(ctx)


class _ReceiverCall(_CallVJP):
    """One Receiver.forward call.  Outputs: (s, s_prob, w bits, w_probs, y, h_w, h_new) when binary (s, w non-differentiable),
    (s, s_prob, w logits, y, h_w, h_new) when continuous (s non-differentiable)."""

    @staticmethod
    def forward(ctx, spec, z, h_prev, desc_in, *params):
        # desc_in: the caller's desc tensor under input_grad (None otherwise): the call reads spec["desc"], its fp32 copy
        eng = spec["eng"]
        ctx.spec = spec
        ctx.set_materialize_grads(False)
        B = z.size(0)
        h = torch.zeros(B, eng.cfg.rec_hidden, device=z.device) if h_prev is None else h_prev.clone()   # in: h_prev, out: h_new
        sprod = torch.ones(B, device=z.device)
        s, s_prob, w, w_probs, y, h_w = eng.receiver_forward(z.contiguous(), spec["desc"], h, sprod, h_prev is None, spec["t"],
                                                             True, seed=spec["seed"])
        # (desc too: an in-place edit of it before backward() trips torch's version check, as for the other saved inputs)
        ctx.save_for_backward(z, h_prev, h, y, w_probs, s_prob, spec["desc"], desc_in, *params)
        if w_probs is None:
            ctx.mark_non_differentiable(s)
            return s, s_prob, w, y, h_w, h
        ctx.mark_non_differentiable(s, w)
        return s, s_prob, w, w_probs, y, h_w, h

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        z, h_prev, h_new, y, w_probs, s_prob, desc, desc_in = _CallVJP._check(ctx)[:8]
        if w_probs is None:
            _, dps, dw, dy, dh_w, dh_new = grads
        else:
            _, dps, _, dw, dy, dh_w, dh_new = grads
        spec = ctx.spec
        dz, dh_prev = spec["eng"].receiver_vjp(z, desc, h_prev, h_new, y, w_probs, s_prob, dy, dw, dps, dh_w, dh_new,
                                               want_dz=ctx.needs_input_grad[1], want_dh_prev=ctx.needs_input_grad[2])
        ddesc = None
        if ctx.needs_input_grad[3]:                                       # d desc of this call, from the deltas the VJP left
            ddesc = spec["eng"].input_grads(1, want_ddesc=True, per_call=True, y=y)[1]
            ddesc = ddesc.to(device=desc_in.device, dtype=desc_in.dtype).reshape(desc_in.shape)
        return (None, None if dz is None else dz.view_as(z), dh_prev, ddesc) + _CallVJP._param_grads(ctx)


class _BaselineCall(_CallVJP):
    """One Baseline.forward call.  Output: the score [B, 1]."""

    @staticmethod
    def forward(ctx, spec, x, binary, inp, *params):
        ctx.spec = spec
        ctx.set_materialize_grads(False)
        c = lambda v: None if v is None else v.contiguous()
        score = spec["eng"].baseline_forward(spec["agent"], c(x), c(binary), c(inp))
        ctx.save_for_backward(x, binary, inp, *params)
        return score

    @staticmethod
    @once_differentiable
    def backward(ctx, dscore):
        x, binary, inp = _CallVJP._check(ctx)[:3]
        spec = ctx.spec
        outs = spec["eng"].baseline_vjp(spec["agent"], x, binary, inp, dscore, want=tuple(ctx.needs_input_grad[1:4]))
        outs = tuple(None if g is None else g.view_as(v) for g, v in zip(outs, (x, binary, inp)))
        return (None,) + outs + _CallVJP._param_grads(ctx)


class Sender(_Agent):
    """model.py:49-238 (sender_mix == 'sum').  use_attn=True (the reference's -visual_attn / -attn_dim / -attn_extra_context /
    -attn_context_dim, model.py:80-86, 114-142, 168-191): the sender attends over the locations of a feature map -- forward() then
    takes x [B, feat_dim, h, w] and, with attn_extra_context, the context g [B, attn_context_dim]; the module owns attn_W_x, attn_W_w,
    attn_U (and attn_W_g) under the reference's state_dict names and in its order.  Conversations, evaluation, forward() and
    Game.train_step(s) run the attention kernels; attn_U.bias has an exactly zero gradient and never moves."""
    agent_name = "sender"

    def __init__(self, feature_type, feat_dim, h_dim, w_dim, bin_dim_out, use_binary,
                 use_attn=False, attn_dim=256, attn_extra_context=False, attn_context_dim=4096):
        super().__init__()
        self.feature_type, self.feat_dim, self.h_dim, self.w_dim = feature_type, feat_dim, h_dim, w_dim
        self.bin_dim_out, self.use_binary, self.use_attn = bin_dim_out, use_binary, bool(use_attn)
        self.attn_dim, self.attn_extra_context, self.attn_context_dim = attn_dim, bool(attn_extra_context), attn_context_dim
        self.image_layer = nn.Linear(feat_dim, h_dim)
        self.code_layer = nn.Linear(w_dim, h_dim)
        self.code_bias = nn.Parameter(torch.zeros(bin_dim_out))
        self.binary_layer = nn.Linear(h_dim, bin_dim_out)
        if self.use_attn:                                                 # model.py:80-86
            if not 1 <= int(attn_dim) <= _lib.VATTN_MAX_DIM:
                raise NotImplementedError("attn_dim must be 1..%d (got %s)" % (_lib.VATTN_MAX_DIM, attn_dim))
            if self.attn_extra_context and not 1 <= int(attn_context_dim) <= _lib.VATTN_MAX_CTX:
                raise NotImplementedError("attn_context_dim must be 1..%d (got %s)" % (_lib.VATTN_MAX_CTX, attn_context_dim))
            self.attn_W_x = nn.Linear(feat_dim, attn_dim)
            self.attn_W_w = nn.Linear(w_dim, attn_dim)
            self.attn_U = nn.Linear(attn_dim, 1)
            if self.attn_extra_context:
                self.attn_W_g = nn.Linear(attn_context_dim, attn_dim)
        self.h_x = None
        self.reset_parameters()
        self.reset_state()

    @property
    def vattn(self):
        """(attn_dim, context_dim) of an attention sender -- context_dim 0 without attn_W_g --, None of a plain one."""
        return (int(self.attn_dim), int(self.attn_context_dim) if self.attn_extra_context else 0) if self.use_attn else None

    def reset_parameters(self):                                           # model.py:90-97
        for m in self.modules():
            if isinstance(m, nn.Linear):
                xavier_normal(m.weight.data)
                m.bias.data.zero_()
        self.code_bias.data.normal_()

    def reset_state(self):                                                # model.py:99-112
        self.attn_scores = []
        self._state_gen = getattr(self, "_state_gen", 0) + 1              # (the cached attn_W_x(X) / attn_W_g(g) are stale)

    def _forward_attn(self, x, w, g, t):
        """model.py:168-195 on the attention kernels: attn_W_x(X) and attn_W_g(g) are formed by the first call after reset_state()
        and kept, as the reference caches them -- from THAT call's x and g: a later call with another map needs reset_state()
        first, as in the reference.  A whole conversation on the same engine in between (Game.exchange, eval_forward,
        train_step) replaces the tables and the context; the next call here then forms its own again."""
        game = self._bound_game(x.size(0))
        if getattr(game, "autograd", False) and self.training and torch.is_grad_enabled():
            raise NotImplementedError("autograd through Sender.forward with visual attention is not available (the per-call VJPs "
                                      "do not form the attention)")
        eng = game.vattn_engine_for(x)
        B = x.size(0)
        if getattr(eng, "_vattn_gen", None) != (id(self), self._state_gen):
            eng.set_data_context(game.check_context(g, B))
            eng.vattn_reset_state()
            eng._vattn_gen = (id(self), self._state_gen)
        xm = x.detach().to(eng.device, torch.float32).contiguous().view(B, x.size(1), -1)
        msg, probs, h_x = eng.sender_forward(xm, None if t == 0 else w.contiguous(), t, self.training, seed=game.next_seed())
        self.h_x = h_x                                                    # model.py:195 side effect
        self.attn_scores.append(eng.tape["vattn_alpha"][t].clone())       # model.py:189
        return msg, probs

    def forward(self, x, w, g, t):
        if self.use_attn:
            return self._forward_attn(x, w, g, t)
        game = self._bound_game(x.size(0))
        if self._graph_on(game):
            eng = game.engine_for(x.size(0))
            out = _SenderCall.apply(self._spec(eng, t=t, seed=game.next_seed()), x, None if t == 0 else w,
                                    *self.parameters())
            msg, probs, h_x = out if self.use_binary else (out[0], None, out[1])
            self.h_x = h_x                                                # model.py:195 side effect
            return msg, probs
        msg, probs, h_x = game.engine_for(x.size(0)).sender_forward(
            x.contiguous(), None if t == 0 else w.contiguous(), t, self.training, seed=game.next_seed())
        self.h_x = h_x                                                    # model.py:195 side effect
        return msg, probs


class Receiver(_Agent):
    """model.py:241-477.  desc_attn=True (the reference's -desc_attn / -desc_attn_dim, model.py:267-271, 344-410): the receiver
    attends over the words of every description -- forward() then needs desc_set [n_words, desc_dim] and desc_set_lens, and the
    module owns d_d, d_h and d_attn beside the reference's other layers, under the reference's state_dict names."""
    agent_name = "receiver"

    def __init__(self, z_dim, desc_dim, hid_dim, out_dim, w_dim, s_dim, use_binary, desc_attn=False, desc_attn_dim=64):
        super().__init__()
        if out_dim != 1 or s_dim != 1:
            raise NotImplementedError("rec_out_dim and rec_s_dim must be 1 (the reference's only working setting)")
        self.z_dim, self.desc_dim, self.hid_dim = z_dim, desc_dim, hid_dim
        self.out_dim, self.w_dim, self.s_dim, self.use_binary = out_dim, w_dim, s_dim, use_binary
        self.rnn = nn.GRUCell(z_dim, hid_dim)
        self.w_h = nn.Linear(hid_dim, hid_dim, bias=True)
        self.w_d = nn.Linear(desc_dim, hid_dim, bias=False)
        self.w = nn.Linear(hid_dim, w_dim)
        self.y1 = nn.Linear(hid_dim + desc_dim, hid_dim)
        self.y2 = nn.Linear(hid_dim, out_dim)
        self.s = nn.Linear(hid_dim, s_dim)
        self.desc_attn = bool(desc_attn)
        self.attn_dim = int(desc_attn_dim) if self.desc_attn else 0
        if self.desc_attn:                                                # model.py:267-271
            if not 1 <= self.attn_dim <= _lib.ATTN_MAX_DIM:
                raise NotImplementedError("desc_attn_dim must be 1..%d (got %d)" % (_lib.ATTN_MAX_DIM, self.attn_dim))
            self.d_d = nn.Linear(desc_dim, self.attn_dim)
            self.d_h = nn.Linear(hid_dim, self.attn_dim)
            self.d_attn = nn.Linear(self.attn_dim, 1)
        self.reset_parameters()
        self.reset_state()

    def reset_parameters(self):                                           # model.py:275-288
        for m in self.modules():
            if isinstance(m, nn.Linear):
                xavier_normal(m.weight.data)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.GRUCell):
                for mm in m.parameters():
                    if mm.data.ndimension() == 2:
                        xavier_normal(mm.data)
                    else:
                        mm.data.zero_()

    def reset_state(self):                                                # model.py:290-298
        self.h_z = None
        self.s_prob_prod = None
        self.h_w = None
        self._t = 0

    def initial_state(self, batch_size):                                  # model.py:300-301
        return torch.zeros(batch_size, self.hid_dim, device=self.w.weight.device)

    def forward(self, z, desc, desc_set=None, desc_set_lens=None):
        game = self._bound_game(z.size(0))
        B = z.size(0)
        if self.desc_attn:
            if getattr(game, "autograd", False) and self.training and torch.is_grad_enabled():
                raise NotImplementedError("autograd through Receiver.forward with desc_attn is not available (the per-call VJPs do "
                                          "not form the attention); Game.train_step trains an attention receiver")
            game.set_desc_set(desc_set, desc_set_lens)                    # (an unchanged pair is not uploaded again)
        if self._graph_on(game):
            input_grad = getattr(game, "input_grad", False)
            if desc.requires_grad and not input_grad:
                raise NotImplementedError("gradients with respect to desc need the input_grad opt-in (Game(..., input_grad=True)); "
                                          "without it pass desc.detach() (the reference hands the receiver desc.data, "
                                          "model.py:803-805)")
            eng = game.engine_for(B)
            spec = self._spec(eng, t=min(self._t, game.max_exchange - 1), seed=game.next_seed(),
                              desc=desc.detach().contiguous())
            out = _ReceiverCall.apply(spec, z, self.h_z, desc if input_grad and desc.requires_grad else None, *self.parameters())
            if self.use_binary:
                s, s_prob, w, w_probs, y, h_w, h_z = out
            else:
                (s, s_prob, w, y, h_w, h_z), w_probs = out, None
            self._t += 1
            self.h_z, self.h_w = h_z, h_w                                 # model.py:340, 452 side effects
            return (s, s_prob), (w, w_probs), y
        first = self.h_z is None
        h_z = self.initial_state(B) if first else self.h_z.clone()
        sprod = torch.ones(B, device=z.device) if self.s_prob_prod is None else self.s_prob_prod.view(-1).clone()
        s, s_prob, w, w_probs, y, h_w = game.engine_for(B).receiver_forward(
            z.contiguous(), desc.contiguous(), h_z, sprod, first, min(self._t, game.max_exchange - 1),
            self.training, seed=game.next_seed())
        self._t += 1
        self.h_z, self.h_w = h_z, h_w                                     # model.py:340, 452 side effects
        if not self.training:
            self.s_prob_prod = sprod.view(B, 1)                           # model.py:423-426
        return (s, s_prob), (w, w_probs), y


class Baseline(_Agent):
    """model.py:480-516."""

    def __init__(self, hid_dim, x_dim, binary_dim, inp_dim):
        super().__init__()
        self.x_dim, self.binary_dim, self.inp_dim, self.hid_dim = x_dim, binary_dim, inp_dim, hid_dim
        self.linear1 = nn.Linear(x_dim + binary_dim + inp_dim, hid_dim)
        self.linear2 = nn.Linear(hid_dim, 1)
        self.agent_name = "baseline_sen" if inp_dim == 0 else "baseline_rec"

    def forward(self, x, binary, inp):
        game = self._bound_game(binary.size(0))
        if self._graph_on(game):
            eng = game.engine_for(binary.size(0))
            return _BaselineCall.apply(self._spec(eng), x, binary, inp, *self.parameters())
        return game.engine_for(binary.size(0)).baseline_forward(
            self.agent_name, None if x is None else x.contiguous(), binary.contiguous(),
            None if inp is None else inp.contiguous())
