"""exchange() and the per-minibatch training block of the reference (model.py:725-876, 1240-1339)
on top of the HIP engine, with the reference's calling conventions and return structures."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import commstats
from . import flags as _flags
from . import misc
from .engine import Engine, steps_from_counter


def _input_grad(g, like):
    """A gradient the engine formed (fp32, on its device) in the shape, dtype and device of the input it belongs to."""
    return None if g is None else g.to(device=like.device, dtype=like.dtype).reshape(like.shape)


def relax_setting(relax):
    """dict(tau_sen=..., tau_rec=..., hard=False) (or a (tau_sen, tau_rec, hard) tuple) -> (tau_sen, tau_rec, hard); None stays.
    Raises ValueError for anything but two positive temperatures."""
    if relax is None:
        return None
    if isinstance(relax, dict):
        unknown = sorted(set(relax) - {"tau_sen", "tau_rec", "hard"})
        if unknown or "tau_sen" not in relax or "tau_rec" not in relax:
            raise ValueError("relax = dict(tau_sen=..., tau_rec=..., hard=False) expected, got keys %s" % sorted(relax))
        relax = (relax["tau_sen"], relax["tau_rec"], relax.get("hard", False))
    tau_sen, tau_rec, hard = relax
    if tau_sen is None or tau_rec is None:
        raise ValueError("relax: both temperatures, tau_sen and tau_rec, are needed")
    tau_sen, tau_rec = float(tau_sen), float(tau_rec)
    if not (tau_sen > 0.0 and tau_rec > 0.0):                             # (NaN fails the compare)
        raise ValueError("relax: tau_sen = %r and tau_rec = %r must be positive" % (tau_sen, tau_rec))
    return tau_sen, tau_rec, bool(hard)


class _AgentVJP(torch.autograd.Function):
    """One agent's graph of a training exchange() as ONE autograd node (the reference's four graphs are disjoint: every input
    crossing between agents is detached, model.py:807-811, 826-829, 835-843).  Inputs: a spec (engine, tape generation, steps,
    the forward's x / desc, the tape arrays to hand out), the caller's data and desc tensors under ``input_grad`` (None otherwise,
    and None for an agent that does not read the input: data belongs to the sender, desc to the receiver) and the agent's
    parameters; outputs: the agent's differentiable outputs stacked over the executed steps, [n, B, .] copies of the tape.
    backward runs the agent's HIP VJP (Engine.vjp) and returns copies of its gradient slice -- and, where autograd asks for them,
    d data / d desc, formed right behind the VJP from the deltas it left (Engine.input_grads)."""
    AGENT = None
    KEYS = ()          # Engine.vjp keyword of each output's gradient

    @staticmethod
    def forward(ctx, spec, data, desc, *params):
        ctx.spec = spec
        ctx.set_materialize_grads(False)               # (an unused output: a NULL upstream gradient, i.e. zero)
        ctx.save_for_backward(data, desc, *params)     # a second backward / an in-place update of the parameters raise
        return tuple(t.clone() for t in spec["outs"])

    @staticmethod
    def _input_grads(ctx, saved):
        """(d data, d desc) of the VJP that has just run, None where autograd does not ask."""
        want_dx, want_dd = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_dx or want_dd):
            return None, None
        dx, dd = ctx.spec["eng"].input_grads(ctx.spec["n"], want_dx, want_dd)
        return _input_grad(dx, saved[0]), _input_grad(dd, saved[1])

    @classmethod
    def _backward(cls, ctx, grads):
        saved = ctx.saved_tensors                      # (raises once freed: backward through this node a second time)
        spec = ctx.spec
        eng = spec["eng"]
        if eng.generation != spec["gen"]:
            raise RuntimeError("the exchange tape this %s node was recorded on has been overwritten by a later engine call "
                               "(exchange / train_step / forward): call backward() before the next one" % cls.AGENT)
        eng.vjp(cls.AGENT, spec["n"], spec["x"], spec["desc"],
                **{k: g for k, g in zip(cls.KEYS, grads) if g is not None})
        views = eng.grads[cls.AGENT]
        return (None,) + cls._input_grads(ctx, saved) + tuple(views[name].clone() for name in spec["names"])


class _SenderVJP(_AgentVJP):
    AGENT, KEYS = "sender", ("dz",)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _SenderVJP._backward(ctx, grads)


class _ReceiverVJP(_AgentVJP):
    AGENT, KEYS = "receiver", ("dy", "dps", "dw")

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _ReceiverVJP._backward(ctx, grads)


class _BaselineSenVJP(_AgentVJP):
    AGENT, KEYS = "baseline_sen", ("dbs",)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _BaselineSenVJP._backward(ctx, grads)


class _BaselineRecVJP(_AgentVJP):
    AGENT, KEYS = "baseline_rec", ("dbr",)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _BaselineRecVJP._backward(ctx, grads)


class _ChannelVJP(_AgentVJP):
    """The sender's and the receiver's graphs of a training exchange() as ONE autograd node: the messages crossing between the
    two agents are not detached (``channel_grad``; the reference detaches them, model.py:807-811, 826-829).  Inputs: a spec as
    _AgentVJP's and the sender's, then the receiver's parameters; outputs: what _SenderVJP and _ReceiverVJP hand out together
    (pz | z logits, y, ps, pw | w logits, stacked over the executed steps).  backward runs Engine.vjp_channel ONCE and returns
    copies of both agents' gradient slices; under ``input_grad`` d data and d desc too, with the channel's cross terms.
    spec["relax"]: the relaxation the forward ran with (None: the straight-through channel) -- backward runs under the same one,
    whatever the engine has been set to since (an annealing step between exchange() and backward())."""
    KEYS = ("dz", "dy", "dps", "dw")

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors                      # (raises once freed: backward through this node a second time)
        spec = ctx.spec
        eng = spec["eng"]
        if eng.generation != spec["gen"]:
            raise RuntimeError("the exchange tape this sender-receiver node was recorded on has been overwritten by a later "
                               "engine call (exchange / train_step / forward): call backward() before the next one")
        relax, now = spec.get("relax"), eng.relaxation
        if relax != now:
            eng.set_message_relaxation(*(relax or (None, None)))
        try:
            eng.vjp_channel(spec["n"], spec["x"], spec["desc"], **{k: g for k, g in zip(_ChannelVJP.KEYS, grads) if g is not None})
            return ((None,) + _AgentVJP._input_grads(ctx, saved)
                    + tuple(eng.grads[agent][name].clone() for agent, name in spec["names"]))
        finally:
            if relax != now:
                eng.set_message_relaxation(*(now or (None, None)))


class FlatOptimizer(object):
    """Checkpoint-facing stand-in for the reference's four torch.optim objects (model.py:1110-1142):
    the update itself runs inside libmmg (k_gradnorm/k_opt); this class only converts the agent's slice
    of the flat optimizer state to and from torch.optim's state_dict layout (misc.py:61-62, 89-90): state index i is
    the i-th entry of module.parameters(), so a state_dict saved by torch.optim.RMSprop / Adam built on the reference's
    modules loads here and vice versa (tests/test_cli_gpu.py::test_optimizer_state_roundtrip_with_torch_optim)."""

    def __init__(self, game, agent):
        self.game, self.agent = game, agent

    def _params(self):
        """(name, view into the flat buffer) in torch.optim's numbering: the order of module.parameters(), i.e. of
        named_parameters() -- direct nn.Parameters first (Sender: code_bias is index 0), then the sub-modules in
        registration order -- NOT the engine's flat-buffer order."""
        mod = self.game.modules.get(self.agent)
        if self.game.engine is None:                  # (no engine yet: nothing was trained, the modules still own their parameters)
            return [(name, p.data) for name, p in mod.named_parameters()] if mod is not None else []
        views = self.game.engine.params[self.agent]
        if mod is None:
            return list(views.items())
        return [(name, views[name]) for name, _ in mod.named_parameters()]

    def state_dict(self):
        """torch.optim's layout; "step" is the agent's OWN count of updates (a frozen agent's stands still) and
        param_groups[0]["lr"] the current learning rate.  One more top-level key, "training_controls" -- whether the agent is trainable,
        the learning rate, the entropy weights, the agent's step --, carries Game.freeze / set_hyper through a checkpoint;
        torch.optim ignores it."""
        eng, kind = self.game.engine, self.game.cfg["optim_type"]
        step = self.game.agent_steps()[self.agent]
        n = eng.n_params if eng is not None else 0
        state = {}
        for i, (name, view) in enumerate(self._params()):
            off = view.storage_offset()
            if eng is None or step == 0 or kind == "SGD":
                continue
            if kind == "RMSprop":
                state[i] = {"step": torch.tensor(float(step)),
                            "square_avg": eng.opt_state[off:off + view.numel()].view(view.shape).cpu().clone()}
            else:
                state[i] = {"step": torch.tensor(float(step)),
                            "exp_avg": eng.opt_state[off:off + view.numel()].view(view.shape).cpu().clone(),
                            "exp_avg_sq": eng.opt_state[n + off:n + off + view.numel()].view(view.shape).cpu().clone()}
        group = {"lr": self.game.cfg["learning_rate"], "params": list(range(len(self._params())))}
        if kind == "RMSprop":
            group.update(alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False)
        elif kind == "Adam":
            group.update(betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False)
        return {"state": state, "param_groups": [group], "training_controls": self.game.controls_state(self.agent, step)}

    def load_state_dict(self, sd):
        eng, kind = self.game.engine, self.game.cfg["optim_type"]
        # "training_controls" (state_dict): a checkpoint of this package restores the mask bit, the learning rate and the entropy weights;
        # a torch optimizer's state dict, or a checkpoint from before the controls existed, has no such key and sets nothing new
        controls = sd.get("training_controls")
        if controls is not None:
            self.game.load_controls(self.agent, controls)
        if eng is None:
            return
        # The parameters themselves do not change here, but a pending node of an agent module's forward() was recorded before
        # the optimizer state it is meant to be stepped with: it raises, as for the other library-side updates (Engine.param_version).
        eng.bump_param_version()
        n = eng.n_params
        step = 0
        for i, (name, view) in enumerate(self._params()):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None:
                continue
            off = view.storage_offset()
            step = max(step, int(float(st.get("step", 0))))
            if kind == "RMSprop":
                eng.opt_state[off:off + view.numel()].copy_(st["square_avg"].reshape(-1).to(eng.device))
            elif kind == "Adam":
                eng.opt_state[off:off + view.numel()].copy_(st["exp_avg"].reshape(-1).to(eng.device))
                eng.opt_state[n + off:n + off + view.numel()].copy_(st["exp_avg_sq"].reshape(-1).to(eng.device))
        if step:
            self.game.set_agent_step(self.agent, step)


class EvalAccumulator(object):
    """What one dev evaluation adds up ON THE DEVICE (Game.eval_steps; include/mmg.h: mmg_eval_steps): the library's int64
    accumulator -- hits, the [D, D] confusion counts, the classes seen -- shared by the engines of every batch size, and per
    call the conversation lengths and the per-batch step count / Hamming counts.  fetch() copies everything to the host ONCE.
    profile=True: the accumulator also owns ONE communication profile (include/mmg.h: mmg_eval_steps_profile) that the engines of
    all batch sizes add to; fetch() returns it, parsed into its named blocks (commstats.parse_profile), under "profile".
    codes=cap_rows: the accumulator also owns every sample's packed message bits and (output step, target), in dataset order
    (include/mmg.h: mmg_eval_steps_codes; one more launch per batch) -- cap_rows is the capacity the buffers start with; an
    evaluation that outgrows it gets larger ones (device copies, no host synchronisation).  meaning="data" | "desc": and an [N, F]
    device matrix of what a sample MEANS, the batches' data rows or the desc[target] rows, for pair_hist().  fetch() is unchanged
    by both."""

    def __init__(self, n_classes, top_k, profile=False, codes=None, meaning=None):
        self.n_classes, self.top_k, self.profile = int(n_classes), int(top_k), bool(profile)
        self.acc = None                                # created by the first engine that adds to it
        self.prof, self.prof_dims = None, None         # profile=True: the flat profile and its (D, T, W), likewise
        self.parts = []                                # (B, n, T, binary, lens [n * B] i32, batch [n, 1 + 2 T] i64)
        if meaning not in (None, "data", "desc"):
            raise ValueError("meaning must be None, 'data' or 'desc' (got %r)" % (meaning,))
        if meaning is not None and codes is None:
            raise ValueError("meaning=%r needs codes=cap_rows" % (meaning,))
        if codes is not None and int(codes) < 1:
            raise ValueError("codes: the capacity in rows must be >= 1")
        self.cap_rows = None if codes is None else int(codes)
        self.meaning_kind = meaning
        self.codes, self.meta, self.meaning, self.rows = None, None, None, 0      # codes=cap_rows: created by the first engine, likewise
        self._code_eng = None

    def _room(self, eng, rows, width):
        """Buffers for `rows` more rows of codes (and of a `width`-wide meaning matrix)."""
        if self.codes is None:
            self.cap_rows = max(self.cap_rows, rows)
            self.codes, self.meta = eng.eval_codes(self.cap_rows)
            self._code_eng = eng
        elif tuple(self.codes.shape[1:]) != (_lib.EVAL_CODE_AGENTS, eng.cfg.max_exchange, _lib.code_wp(eng.cfg.w_dim)):
            raise ValueError("the engines of one evaluation must share max_exchange and w_dim")
        if self.meaning_kind and self.meaning is None:
            self.meaning = torch.empty(self.cap_rows, width, dtype=torch.float32, device=self.codes.device)
        if self.rows + rows > self.cap_rows:
            self.cap_rows = max(2 * self.cap_rows, self.rows + rows)
            grown = eng.eval_codes(self.cap_rows) + ((torch.empty(self.cap_rows, width, dtype=torch.float32, device=self.codes.device),)
                                                     if self.meaning is not None else ())
            for new, old in zip(grown, (self.codes, self.meta, self.meaning)):
                new[:self.rows].copy_(old[:self.rows])
            self.codes, self.meta = grown[0], grown[1]
            self.meaning = grown[2] if self.meaning is not None else None

    def add(self, eng, data, target, desc, n, corrupt_mask=None):
        if self.acc is None:
            self.acc = eng.eval_acc()
        if self.profile and self.prof is None:
            self.prof, self.prof_dims = eng.eval_profile(), (eng.cfg.n_classes, eng.cfg.max_exchange, eng.cfg.w_dim)
        kw = dict(prof=self.prof) if self.profile else {}
        rows = int(n) * eng.cfg.batch
        if self.cap_rows is not None:
            flat = data.reshape(data.size(0), -1)
            self._room(eng, rows, flat.size(1) if self.meaning_kind == "data" else desc.size(1))
            kw["codes"] = (self.codes, self.meta, self.rows)
        lens, batch = eng.eval_steps(data, target, desc, n, self.top_k, self.acc, corrupt_mask=corrupt_mask, **kw)
        self.parts.append((eng.cfg.batch, int(n), eng.cfg.max_exchange, bool(eng.cfg.use_binary), lens, batch))
        if self.cap_rows is not None:
            if self.meaning_kind == "data":
                self.meaning[self.rows:self.rows + rows].copy_(flat[:rows])
            elif self.meaning_kind == "desc":          # (a target outside [0, D) is skipped by the histogram: any row does)
                self.meaning[self.rows:self.rows + rows].copy_(desc.index_select(0, target[:rows].clamp(0, desc.size(0) - 1)))
            self.rows += rows

    def pair_hist(self, agent=0, steps=None, bins=64, meaning=None):
        """The pair histogram of the codes collected so far (include/mmg.h: mmg_code_pair_hist; two launches, then ONE copy to the
        host), parsed by commstats.parse_pair_hist: head / used / skipped / pairs and hist [2, M + 1, bins].  agent: 0 / "sender",
        1 / "receiver"; steps: (t0, t1) or None for every step; meaning: an [N, F] float32 device matrix to measure against instead
        of the one the accumulator kept (meaning="data" | "desc")."""
        if self.cap_rows is None:
            raise ValueError("pair_hist needs an accumulator created with codes=cap_rows")
        if self.codes is None or self.rows == 0:
            raise ValueError("pair_hist: nothing has been added yet")
        x = self.meaning if meaning is None else meaning
        if x is None:
            raise ValueError("pair_hist needs a meaning matrix: EvalAccumulator(meaning='data' | 'desc') or meaning=[N, F]")
        agent = {"sender": 0, "receiver": 1}.get(agent, agent)
        T, W = int(self.codes.size(2)), self._code_eng.cfg.w_dim
        t0, t1 = (0, T) if steps is None else (int(steps[0]), int(steps[1]))
        flat = self._code_eng.code_pair_hist(self.codes, self.meta, self.rows, agent, (t0, t1), x, bins)
        return commstats.parse_pair_hist(flat.cpu().numpy(), t1 - t0, W, bins)

    def fetch(self):
        """dict(hits, batches, samples, conf [D, D], seen [D], lens [samples] int64 in dataset order, n [batches],
        sizes [batches], ham_sen / ham_rec [batches] float64 = sum_{t < n} ham[t] / (B n): the reference's per-batch mean
        Hamming distance, model.py:675-691) -- one device -> host copy.  profile=True: and "profile", the parsed communication
        profile (None when nothing was added), which rides in the same copy."""
        D = self.n_classes
        if self.acc is None:
            z = np.zeros(0)
            out = dict(hits=0, batches=0, samples=0, conf=np.zeros((D, D), np.int64), seen=np.zeros(D, np.int64),
                       lens=np.zeros(0, np.int64), n=np.zeros(0, np.int64), sizes=np.zeros(0, np.int64), ham_sen=z, ham_rec=z)
            if self.profile:
                out["profile"] = None
            return out
        lens = torch.cat([p[4] for p in self.parts]).to(torch.int64)           # (one conversion for all batches, not one per batch)
        flat = torch.cat([self.acc] + [p[5].reshape(-1) for p in self.parts] + [lens]
                         + ([self.prof] if self.prof is not None else [])).cpu().numpy()
        prof = None
        if self.prof is not None:
            prof = commstats.parse_profile(flat[flat.size - self.prof.numel():], *self.prof_dims)
            flat = flat[:flat.size - self.prof.numel()]
        H = _lib.EVAL_ACC_HEAD
        out = dict(hits=int(flat[0]), batches=int(flat[1]), samples=int(flat[2]), conf=flat[H:H + D * D].reshape(D, D),
                   seen=flat[H + D * D:H + D * D + D])
        o = H + D * D + D
        ns, sizes, hs, hr = [], [], [], []
        for B, n, T, binary, _, _ in self.parts:
            rows = flat[o:o + n * (1 + 2 * T)].reshape(n, 1 + 2 * T); o += n * (1 + 2 * T)
            ham = rows[:, 1:] if binary else np.ascontiguousarray(rows[:, 1:]).view(np.float64)
            for i in range(n):
                k = int(rows[i, 0])
                ns.append(k); sizes.append(B)
                hs.append(float(ham[i, :k].astype(np.float64).sum()) / (float(B) * k))
                hr.append(float(ham[i, T:T + k].astype(np.float64).sum()) / (float(B) * k))
        out.update(lens=flat[o:], n=np.asarray(ns, np.int64), sizes=np.asarray(sizes, np.int64),
                   ham_sen=np.asarray(hs, np.float64), ham_rec=np.asarray(hr, np.float64))
        if self.profile:
            out["profile"] = prof
        return out


class Game(object):
    """Binds the four agent modules to one flat parameter buffer on the GPU and caches one libmmg
    handle per (batch size, number of classes).

    autograd=True: training exchange() calls return outputs that carry autograd graphs (see exchange()).
    channel_grad=True (with autograd): the sender and the receiver are ONE graph there, gradients cross the channel.
    input_grad=True (with autograd): data and desc are differentiable inputs of exchange() and desc of Receiver.forward().
    flipout_sen / flipout_rec (a probability, None: off) and flipout_dev: the reference's noisy channel (model.py:233-234, 467-468,
    554-568) -- every bit of the sender's / the receiver's message is inverted with that probability right after it is sampled,
    in training conversations always, in evaluation ones under flipout_dev; everything downstream reads the flipped bits
    (Engine.set_message_flipout).  These keyword arguments are separate from `flags`, whose -flipout_* switches stay refused.
    sender_mix ("sum" | "prod"), ignore_code, ignore_receiver: the reference's communication ablations (model.py:217-218, 208-210,
    470-472) -- the sender's hidden layer is tanh(h_x * h_w) / tanh(h_x) instead of tanh(h_x + h_w), and the receiver's binary
    message is replaced by zeros after it was sampled or rounded (Engine.set_sender_variant).  They hold for every entry of every
    engine the game creates, on every rank; plain autograd works with them, channel_grad, input_grad and message flips do not.
    Separate from `flags` as well: -sender_mix, -ignore_code and -ignore_receiver stay refused there.
    relax = dict(tau_sen=..., tau_rec=..., hard=False): relaxed messages, the Gumbel-sigmoid channel with exact gradients
    (Engine.set_message_relaxation) -- the differentiable-channel baseline next to REINFORCE and to the plain straight-through
    estimator of channel_grad.  Training exchange() calls then form every message element as sigmoid((logit + logistic noise) / tau)
    from the uniform its Bernoulli sample draws (hard: the bit forward, the soft value's gradient backward), and the joint
    sender-receiver node differentiates exactly that.  Needs autograd=True, channel_grad=True, binary messages and world == 1;
    set_relaxation() anneals the temperatures between minibatches; exchange_args["relax"] overrides the setting for one call.
    Evaluation conversations stay discrete.  Message flips, sender variants, attention, train_step(s) and the agent modules' own
    autograd nodes are not available with it and raise; bs / br of a relaxed exchange are plain tensors (the baselines are
    REINFORCE machinery: mmg_exchange_vjp refuses a relaxed handle).
    noise_sen / noise_rec (a standard deviation, None: off) and noise_dev: additive Gaussian noise on CONTINUOUS messages, the
    continuous twin of the flips (Engine.set_message_noise) -- the sender's / the receiver's message is logits + sigma * n, in
    training conversations always, in evaluation ones under noise_dev (keyed by the game's seed); the noisy value is what the other
    agent, the message lists of exchange() and every gradient see.  autograd, channel_grad (exact here: the gradient crosses the
    channel unchanged), input_grad and the agent modules' own nodes work with it; set_noise() anneals the sigmas between
    minibatches.  Binary messages raise ValueError, attention and sender variants NotImplementedError.  The setting is NOT stored
    in checkpoints (controls_state() / save()): a resumed run states it again.
    Description attention (model.py:267-271, 344-410) is read from the module: Receiver(..., desc_attn=True, desc_attn_dim=A).  The
    receiver then attends over the words of every description: exchange() takes exchange_args["desc_set"] / ["desc_set_lens"] as
    the reference does, Receiver.forward its desc_set / desc_set_lens arguments, and set_desc_set() states the pair for the entries
    that have no such argument (train_step(s), eval_forward, eval_steps).  Training, evaluation and the agent-level forward run the
    attention kernels; autograd / channel_grad / input_grad, message flips, sender variants and data-parallel training are not
    available with it and raise.  The -desc_attn switch of `flags` stays refused.
    Visual attention (model.py:80-86, 114-142, 168-195) is read from the module as well: Sender(..., use_attn=True, attn_dim=A,
    attn_extra_context=bool, attn_context_dim=G).  exchange_args["data"] is then the feature map [B, feat_dim, h, w] and
    exchange_args["data_context"] the context [B, G] -- required iff the sender has attn_W_g, ignored otherwise, as the reference
    ignores g; eval_forward / eval_steps take data_context=, Sender.forward its g.  Conversations (training-mode ones with both
    baselines included), evaluation, the agent-level forward and train_step(s) (which take data_context= too) run the attention
    kernels, and sender.attn_scores holds the per-step [B, h * w] weights after exchange().  autograd / channel_grad / input_grad,
    message flips, sender variants, description attention together with it and world > 1 raise.  Engines are cached per (batch,
    classes, h * w).  The -visual_attn switch of `flags` stays refused."""

    def __init__(self, sender, receiver, baseline_sen, baseline_rec, flags=None, device=None, seed=0, autograd=False,
                 channel_grad=False, input_grad=False, flipout_sen=None, flipout_rec=None, flipout_dev=False,
                 sender_mix="sum", ignore_code=False, ignore_receiver=False, relax=None, noise_sen=None, noise_rec=None, noise_dev=False):
        fl = flags if flags is not None else _flags.FLAGS
        _flags.check_supported(fl)                    # -desc_attn, -sender_mix prod|mou, -flipout_*, -ignore_*, ... raise
        self.modules = dict(sender=sender, receiver=receiver, baseline_sen=baseline_sen, baseline_rec=baseline_rec)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_exchange = fl.max_exchange
        self.cfg = dict(feat_dim=sender.feat_dim, h_dim=sender.h_dim, w_dim=sender.w_dim, rec_hidden=receiver.hid_dim,
                        wv_dim=receiver.desc_dim, bas_hidden=baseline_sen.hid_dim if baseline_sen is not None else 500,
                        max_exchange=fl.max_exchange, use_binary=bool(sender.use_binary),
                        fixed_exchange=bool(fl.fixed_exchange), s_prob_prod=bool(fl.s_prob_prod),
                        entropy_s=fl.entropy_s, entropy_sen=fl.entropy_sen, entropy_rec=fl.entropy_rec,
                        first_rec=fl.first_rec, optim_type=fl.optim_type, learning_rate=fl.learning_rate,
                        top_k=fl.top_k_train)
        assert sender.bin_dim_out == sender.w_dim == receiver.w_dim == receiver.z_dim, \
            "Both sender and receiver should communicate with same dim vectors for now."     # model.py:1756
        self.seed = seed
        self.autograd = bool(autograd)
        self.channel_grad = bool(channel_grad)
        self.input_grad = bool(input_grad)
        for name, p in (("flipout_sen", flipout_sen), ("flipout_rec", flipout_rec)):
            if p is not None and not 0.0 <= float(p) <= 1.0:             # (NaN fails both compares)
                raise ValueError("%s = %r is not a probability in [0, 1]" % (name, p))
        self.flipout = None if flipout_sen is None and flipout_rec is None else (flipout_sen, flipout_rec, bool(flipout_dev))
        if self.flipout and self.channel_grad:
            raise NotImplementedError("channel_grad with message flips: the straight-through surrogate under a flip is not defined")
        if sender_mix == "mou":
            raise NotImplementedError("sender_mix = 'mou' needs a 4H binary layer (binary_layer [W, 4H], and code_bias_mou under "
                                      "ignore_code): another parameter layout; 'sum' and 'prod' are available")
        if sender_mix not in ("sum", "prod"):
            raise ValueError("sender_mix = %r: 'sum' or 'prod' expected" % (sender_mix,))
        variant = (sender_mix, bool(ignore_code), bool(ignore_receiver))
        self.sender_variant = None if variant == ("sum", False, False) else variant
        if self.sender_variant and self.flipout:
            raise NotImplementedError("a sender variant (sender_mix / ignore_code / ignore_receiver) with message flips: a handle "
                                      "has one or the other")
        self._refuse_variant_graph(self.channel_grad, self.input_grad)
        self.attn_dim = int(getattr(receiver, "attn_dim", 0) or 0)       # Receiver(desc_attn=True, desc_attn_dim=A)
        self._desc_set = None                                            # (desc_set, lens) of the next conversation (set_desc_set)
        if self.attn_dim:
            for name, on in (("autograd", self.autograd), ("channel_grad", self.channel_grad), ("input_grad", self.input_grad),
                             ("message flips (flipout_sen / flipout_rec)", self.flipout),
                             ("a sender variant (sender_mix / ignore_code / ignore_receiver)", self.sender_variant)):
                if on:
                    raise NotImplementedError("desc_attn with %s is not available" % name)
        self.vattn = getattr(sender, "vattn", None)                      # Sender(use_attn=True, ...): (attn_dim, context_dim)
        if self.vattn:
            for name, on in (("autograd", self.autograd), ("channel_grad", self.channel_grad), ("input_grad", self.input_grad),
                             ("message flips (flipout_sen / flipout_rec)", self.flipout),
                             ("a sender variant (sender_mix / ignore_code / ignore_receiver)", self.sender_variant),
                             ("description attention (Receiver(desc_attn=True))", self.attn_dim)):
                if on:
                    raise NotImplementedError("visual attention with %s is not available" % name)
        self._call = 0
        self.rank, self.world, self.group, self._dp = 0, 1, None, {}
        self.relax = relax_setting(relax)
        if self.relax:
            self._check_relax(self.autograd, self.channel_grad)
        self._noise_dev = bool(noise_dev)
        self.noise = self._noise_setting(noise_sen, noise_rec, noise_dev)
        self.trainable = tuple(_lib.AGENTS)           # freeze() / unfreeze(): the agents train_step(s) updates
        self._agent_steps = None      # per-agent optimizer steps restored before any engine exists (load_controls)
        self.engines = {}
        self.engine = None            # the first engine owns the flat buffers
        self.optimizers = None
        for m in self.modules.values():
            if m is not None:
                m._game = self

    # the reference's dict names (model.py:1139-1142)
    def optimizers_dict(self):
        return dict(optimizer_rec=FlatOptimizer(self, "receiver"), optimizer_sen=FlatOptimizer(self, "sender"),
                    optimizer_bas_rec=FlatOptimizer(self, "baseline_rec"), optimizer_bas_sen=FlatOptimizer(self, "baseline_sen"))

    def models_dict(self):
        return dict(receiver=self.modules["receiver"], sender=self.modules["sender"],
                    baseline_rec=self.modules["baseline_rec"], baseline_sen=self.modules["baseline_sen"])

    def next_seed(self):
        return self.seed

    def _refuse_variant_graph(self, channel_grad, input_grad):
        """The joint sender-receiver node and the input gradients do not form the sender variants."""
        if self.sender_variant and (channel_grad or input_grad):
            raise NotImplementedError("%s with a sender variant (sender_mix / ignore_code / ignore_receiver) is not available: "
                                      "plain autograd is" % ("channel_grad" if channel_grad else "input_grad"))

    def _check_relax(self, autograd, channel_grad):
        """What relaxed messages need of the game and of the call."""
        if not (autograd and channel_grad):
            raise ValueError("relaxed messages need autograd=True and channel_grad=True: their gradient crosses the channel "
                             "inside the joint sender-receiver node")
        if not self.cfg["use_binary"]:
            raise ValueError("relaxed messages are for binary messages: continuous ones are the logits, already differentiable")
        if self.world > 1:
            raise NotImplementedError("relaxed messages with world > 1 are not available: autograd through exchange() runs on one GPU")
        for name, on in (("message flips (flipout_sen / flipout_rec)", self.flipout),
                         ("a sender variant (sender_mix / ignore_code / ignore_receiver)", self.sender_variant),
                         ("description attention (Receiver(desc_attn=True))", self.attn_dim),
                         ("visual attention (Sender(use_attn=True))", self.vattn)):
            if on:
                raise NotImplementedError("relaxed messages with %s are not available" % name)

    def _noise_setting(self, sigma_sen, sigma_rec, dev):
        """(sigma_sen, sigma_rec, dev) of Gaussian message noise, or None; raises for what a noise game cannot be."""
        sig = []
        for name, v in (("noise_sen", sigma_sen), ("noise_rec", sigma_rec)):
            v = 0.0 if v is None else float(v)
            if not 0.0 <= v < float("inf"):                                # (NaN fails both compares)
                raise ValueError("%s = %r: a standard deviation is finite and not negative" % (name, v))
            sig.append(v)
        if not (sig[0] > 0.0 or sig[1] > 0.0):
            return None
        if self.cfg["use_binary"]:
            raise ValueError("message noise is for continuous messages (use_binary=False): flipout_sen / flipout_rec are the noisy "
                             "channel of binary ones")
        for name, on in (("a sender variant (sender_mix / ignore_code / ignore_receiver)", self.sender_variant),
                         ("description attention (Receiver(desc_attn=True))", self.attn_dim),
                         ("visual attention (Sender(use_attn=True))", self.vattn)):
            if on:
                raise NotImplementedError("message noise with %s is not available" % name)
        return (sig[0], sig[1], bool(dev))

    def set_noise(self, sigma_sen=None, sigma_rec=None):
        """The standard deviations of the message noise from now on -- what a training loop calls between minibatches to anneal
        them -- for every engine of the game (Engine.set_message_noise: host only, no kernel is re-selected while the game stays
        noisy; the evaluation draws start over from count 0).  None, None (or zeros): back to the clean channel.  noise_dev stays
        what the game was created with."""
        self.noise = self._noise_setting(sigma_sen, sigma_rec, self._noise_dev)
        for eng in self.engines.values():
            self._apply_noise(eng)

    def _apply_noise(self, eng):
        if self.noise:
            eng.set_message_noise(self.noise[0], self.noise[1], dev=self.noise[2], eval_seed=self.seed)
        elif getattr(eng, "noise", None):
            eng.set_message_noise(None, None)

    def _refuse_relaxed_step(self, who):
        if self.relax:
            raise NotImplementedError("%s is the REINFORCE step: a game with relaxed messages trains through exchange() and "
                                      "backward() (set_relaxation(None, None) clears the setting)" % who)

    def set_relaxation(self, tau_sen=None, tau_rec=None, hard=False):
        """The temperatures of the relaxed messages from now on -- what a training loop calls between minibatches to anneal them
        -- for every engine of the game (Engine.set_message_relaxation: host only, no kernel is re-selected while the game
        stays relaxed).  None, None: back to the unrelaxed channel."""
        relax = None if tau_sen is None and tau_rec is None else relax_setting((tau_sen, tau_rec, hard))
        if relax:
            self._check_relax(self.autograd, self.channel_grad)
        self.relax = relax
        for eng in self.engines.values():
            eng.set_message_relaxation(*(relax or (None, None)))

    # ------------------------------------------------------------------ training controls (include/mmg.h: mmg_set_trainable, ...)
    def _check_agents(self, agents):
        self._refuse_relaxed_step("freeze / unfreeze: train_step")
        _lib.agent_mask(agents)                       # (ValueError for a name that is no agent)
        return set(agents)

    def freeze(self, *agents):
        """Stop updating these agents (names as in models_dict()) from the next train_step(s) on, in every engine of the game and
        in those created later: parameters and optimizer state stay bit-identical, the agent still speaks / scores, the other
        agents train as before, Adam's bias correction of a frozen agent stands still.  With world > 1 EVERY rank must make the same
        calls between the same minibatches (the mask is host state of each rank's handle).  A game with relaxed messages refuses:
        its optimizers are torch's."""
        off = self._check_agents(agents)
        self.trainable = tuple(a for a in _lib.AGENTS if a in self.trainable and a not in off)
        for eng in self.engines.values():
            eng.set_trainable(self.trainable)

    def unfreeze(self, *agents):
        """Update these agents again (all four when called without a name); see freeze(), and its note on world > 1."""
        on = self._check_agents(agents or _lib.AGENTS)
        self.trainable = tuple(a for a in _lib.AGENTS if a in self.trainable or a in on)
        for eng in self.engines.values():
            eng.set_trainable(self.trainable)

    def set_hyper(self, learning_rate=None, entropy_s=None, entropy_sen=None, entropy_rec=None):
        """New values of the learning rate and of the entropy weights for every later minibatch of train_step(s) -- what a
        training loop calls between minibatches to anneal them; None keeps a value.  They are kept in game.cfg and hold for every
        engine of the game and for those created later.  An entropy weight the game was created without (None in its flags) stays
        absent: its argument is ignored.  With world > 1 EVERY rank must make the same calls between the same minibatches.  A game
        with relaxed messages refuses: its optimizers and losses are the caller's."""
        self._refuse_relaxed_step("set_hyper: train_step")
        new = {}
        if learning_rate is not None:
            lr = float(learning_rate)
            if not (lr >= 0.0 and lr != float("inf")):                    # (NaN fails the compare)
                raise ValueError("learning_rate = %r: finite and >= 0 expected" % (learning_rate,))
            new["learning_rate"] = lr
        for k, v in (("entropy_s", entropy_s), ("entropy_sen", entropy_sen), ("entropy_rec", entropy_rec)):
            if v is None:
                continue
            v = float(v)
            if v != v or v in (float("inf"), float("-inf")):
                raise ValueError("%s = %r: a finite weight expected" % (k, v))
            if self.cfg[k] is not None:
                new[k] = v
        self.cfg.update(new)
        for eng in self.engines.values():
            if "learning_rate" in new:
                eng.set_learning_rate(new["learning_rate"])
            if any(k.startswith("entropy") for k in new):
                eng.set_entropy(**{k: v for k, v in new.items() if k.startswith("entropy")})

    def agent_steps(self):
        """{agent: optimizer steps that updated it} of the engine that trained last (Engine.agent_steps); zeros before any engine."""
        eng = getattr(self, "_train_engine", None) or self.engine
        if eng is None:
            return dict(self._agent_steps or {a: 0 for a in _lib.AGENTS})
        return steps_from_counter(eng.tape["counter"])

    @staticmethod
    def _write_agent_steps(eng, steps):
        """tape "counter" of one engine from {agent: steps}: the global step is the largest count, the others' difference to it the
        steps they sat out frozen (include/mmg.h: mmg_set_trainable)."""
        c = eng.tape["counter"]
        step = max(int(steps[a]) for a in _lib.AGENTS)
        c[1:3] = step
        sat_out = torch.tensor([step - int(steps[a]) for a in _lib.AGENTS], dtype=c.dtype)
        c[4:8] = sat_out[:c[4:8].numel()]

    def set_agent_step(self, agent, step):
        """Restore one agent's step count (FlatOptimizer.load_state_dict) in every engine; the others keep theirs.  The counts are
        read from the device once per load, not once per optimizer (a training step drops the host copy)."""
        steps = dict(self._agent_steps or self.agent_steps())
        if steps[agent] == int(step) and self._agent_steps is not None:
            return
        steps[agent] = int(step)
        self._agent_steps = steps
        for eng in self.engines.values():
            self._write_agent_steps(eng, steps)

    def controls_state(self, agent, step=None):
        """What FlatOptimizer.state_dict()["training_controls"] holds for `agent`."""
        return dict(trainable=agent in self.trainable, learning_rate=self.cfg["learning_rate"], entropy_s=self.cfg["entropy_s"],
                    entropy_sen=self.cfg["entropy_sen"], entropy_rec=self.cfg["entropy_rec"],
                    step=int(self.agent_steps()[agent] if step is None else step))

    def load_controls(self, agent, controls):
        """The inverse of controls_state(): fields a checkpoint lacks keep their current values.  (A game with relaxed messages has
        no library-side optimizer and can only have saved the defaults: nothing to restore.)"""
        if self.relax:
            return
        if "trainable" in controls and bool(controls["trainable"]) != (agent in self.trainable):
            (self.unfreeze if controls["trainable"] else self.freeze)(agent)
        # (the four optimizers of a checkpoint carry the same game-wide values: the first one sets them, the others find them set)
        new = {k: controls[k] for k in ("learning_rate", "entropy_s", "entropy_sen", "entropy_rec")
               if controls.get(k) is not None and self.cfg[k] is not None and float(controls[k]) != self.cfg[k]}
        if new:
            self.set_hyper(**new)
        if "step" in controls:
            self.set_agent_step(agent, controls["step"])

    def _hand_over_counters(self, eng, last):
        """The Philox minibatch counter, the optimizer step and the agents' frozen steps live in each engine's workspace: they move
        to the engine that trains next ([3]: the engine's own launch epoch, never handed over)."""
        c, lc = eng.tape["counter"], last.tape["counter"]
        c[:3].copy_(lc[:3])
        c[4:8].copy_(lc[4:8])

    def set_parallel(self, rank, world, group=None):
        """Data-parallel training (dist.DataParallel): train_step() then takes THIS rank's rows of the global minibatch --
        [rank * B / world, (rank + 1) * B / world) of the reference's batch (misc.py:257-302 order) -- and every rank ends
        each step with the parameters of the single-process step on the whole batch."""
        if self.attn_dim and int(world) > 1:
            raise NotImplementedError("desc_attn with world > 1 is not available: an attention receiver trains on one GPU")
        if self.vattn and int(world) > 1:
            raise NotImplementedError("visual attention with world > 1 is not available: an attention sender runs on one GPU")
        if self.relax and int(world) > 1:
            raise NotImplementedError("relaxed messages with world > 1 are not available: autograd through exchange() runs on one GPU")
        self.rank, self.world, self.group = int(rank), int(world), group

    def check_map(self, data, n=1):
        """The feature map of an attention sender: [B, feat_dim, h, w] (model.py:169; [n * B, ...]: n batches of eval_steps).
        Returns h * w.  Raises ValueError / NotImplementedError (outside the supported range)."""
        if data.dim() != 4:
            raise ValueError("visual attention needs data [B, %d, h, w], got %s" % (self.cfg["feat_dim"], tuple(data.shape)))
        if data.size(1) != self.cfg["feat_dim"]:
            raise ValueError("visual attention: data has %d channels, the sender's feat_dim is %d" % (data.size(1), self.cfg["feat_dim"]))
        if data.size(1) > _lib.VATTN_MAX_CHANNELS:
            raise NotImplementedError("visual attention: at most %d channels (got %d)" % (_lib.VATTN_MAX_CHANNELS, data.size(1)))
        B, N = data.size(0) // n, data.size(2) * data.size(3)
        if not 1 <= N <= _lib.VATTN_MAX_FEATS or B > _lib.VATTN_MAX_BATCH or B * N * self.vattn[0] > _lib.VATTN_MAX_HX:
            raise NotImplementedError("visual attention: h * w must be 1..%d, batch <= %d and batch * h * w * attn_dim <= %d (got "
                                      "h * w = %d, batch %d, attn_dim %d)" % (_lib.VATTN_MAX_FEATS, _lib.VATTN_MAX_BATCH,
                                                                              _lib.VATTN_MAX_HX, N, B, self.vattn[0]))
        return N

    def check_context(self, context, rows):
        """The context of an attention sender: [rows, attn_context_dim], required iff it has attn_W_g; a sender without it
        ignores what it is given (model.py:127-138) -- None is returned then."""
        if not self.vattn[1]:
            return None
        if context is None:
            raise ValueError("this sender has attn_W_g (attn_extra_context): data_context [B, %d] is required" % self.vattn[1])
        if context.dim() != 2 or tuple(context.shape) != (rows, self.vattn[1]):
            raise ValueError("data_context must be [%d, %d], got %s" % (rows, self.vattn[1], tuple(context.shape)))
        return context

    def vattn_engine_for(self, data, n_classes=None, n=1):
        """The engine of an attention sender for the map `data` ([n * B, C, h, w])."""
        N = self.check_map(data, n)
        return self.engine_for(data.size(0) // n, n_classes, n_feats=N)

    def _vattn_train_engine(self, data, desc, data_context, n=1):
        """The training engine of an attention sender for the maps `data` ([n * B, C, h, w]) with their context stated."""
        n_feats = self.check_map(data, n)
        context = self.check_context(data_context, data.size(0))
        eng = self.engine_for(data.size(0) // n, desc.size(0), n_feats=n_feats)
        eng.set_data_context(context, n=n)
        return eng

    def set_desc_set(self, desc_set, desc_set_lens):
        """The description set of an attention receiver (model.py:1081-1084; misc.desc_set_of builds it from misc.cbow's output):
        desc_set [n_words, wv_dim], the word vectors of all classes concatenated, and desc_set_lens, one positive length per
        class.  It holds for every later entry until the next call; exchange() and Receiver.forward call this with their own
        arguments.  A pair that differs from the last one is uploaded to the engine that serves the call (include/mmg.h:
        mmg_set_desc_set); engines are cached per (batch, classes, words), so changing the lengths creates no new handle."""
        if not self.attn_dim:
            if desc_set is None and desc_set_lens is None:
                return
            raise NotImplementedError("desc_set / desc_set_lens need a Receiver built with desc_attn=True")
        from .engine import check_desc_set
        lens = None if desc_set_lens is None else [int(v) for v in desc_set_lens]
        check_desc_set(desc_set, lens, len(lens or ()), self.cfg["wv_dim"])
        if desc_set.size(0) > _lib.ATTN_MAX_WORDS or len(lens) > _lib.ATTN_MAX_CLASSES:
            raise NotImplementedError("desc_attn: at most %d words and %d classes (got %d, %d)"
                                      % (_lib.ATTN_MAX_WORDS, _lib.ATTN_MAX_CLASSES, desc_set.size(0), len(lens)))
        self._desc_set = (desc_set, lens)

    def _adopt(self, eng):
        """Move the modules' parameters into the engine's flat buffer (values preserved)."""
        for agent, m in self.modules.items():
            if m is None:
                continue
            for name, p in m.named_parameters():
                view = eng.params[agent][name]
                view.copy_(p.data.to(eng.device))
                p.data = view

    def engine_for(self, batch, n_classes=None, global_batch=None, batch_offset=0, n_feats=None):
        given = n_classes
        n_classes = n_classes or getattr(self, "_last_classes", None) or 1
        attn = {}
        if self.attn_dim:
            if self._desc_set is None:
                raise ValueError("desc_attn needs desc_set and desc_set_lens (exchange_args, Receiver.forward or Game.set_desc_set)")
            if batch > _lib.ATTN_MAX_BATCH:
                raise NotImplementedError("desc_attn: batch must be <= %d (got %d)" % (_lib.ATTN_MAX_BATCH, batch))
            if given and given != len(self._desc_set[1]):
                raise ValueError("desc has %d classes, desc_set_lens %d" % (given, len(self._desc_set[1])))
            n_classes = len(self._desc_set[1])
            attn = dict(attn_dim=self.attn_dim, n_words=int(self._desc_set[0].size(0)))
        if self.vattn:
            n_feats = n_feats or getattr(self, "_last_feats", None)
            if not n_feats:
                raise ValueError("visual attention: the engine depends on h * w of the feature map (call with the 4-D data first)")
            self._last_feats = n_feats
            attn = dict(vattn=(self.vattn[0], int(n_feats), self.vattn[1]))
        self._last_classes = n_classes
        key = ((batch, n_classes, global_batch or batch, batch_offset) + ((attn["n_words"],) if "n_words" in attn else ())
               + ((int(n_feats),) if self.vattn else ()))
        if key not in self.engines:
            eng = Engine(device=self.device, share=self.engine, batch=batch, n_classes=n_classes,
                         global_batch=global_batch, batch_offset=batch_offset, **attn, **self.cfg)
            if self.flipout:
                eng.set_message_flipout(self.flipout[0], self.flipout[1], dev=self.flipout[2], eval_seed=self.seed)
            if self.sender_variant:
                eng.set_sender_variant(*self.sender_variant)
            if self.relax:
                eng.set_message_relaxation(*self.relax)
            self._apply_noise(eng)
            if set(self.trainable) != set(_lib.AGENTS):
                eng.set_trainable(self.trainable)
            if self._agent_steps:
                self._write_agent_steps(eng, self._agent_steps)
            if self.engine is None:
                self.engine = eng
                self._adopt(eng)
            self.engines[key] = eng
        if "n_words" in attn:
            self.engines[key].set_desc_set(*self._desc_set)              # (an unchanged pair is not uploaded again)
        return self.engines[key]

    def train_engine_for(self, local_batch, n_classes=None):
        """The engine train_step() uses for `local_batch` samples on this rank (the whole batch on one GPU)."""
        return self.engine_for(local_batch, n_classes, global_batch=local_batch * self.world, batch_offset=self.rank * local_batch)

    # ------------------------------------------------------------------ model.py:725-876
    def exchange(self, exchange_args):
        """model.py:725-876: ``(s, sen_w, rec_w, y, bs, br)`` of per-step tensor lists, copies of the engine's tape.

        Autograd (opt-in): with ``exchange_args["autograd"] = True`` (or ``Game(..., autograd=True)``), ``train`` true and
        ``torch.is_grad_enabled()``, the differentiable outputs carry a ``grad_fn``, one autograd node per agent as in the
        reference: the sender's ``sen_probs[t]`` (binary) / ``sen_feats[t]`` (continuous logits); the receiver's ``y[t]``,
        ``s_probs[t]`` and ``rec_probs[t]`` (binary) / ``rec_feats[t]`` (continuous logits); ``bs[t]`` / ``br[t]`` (binary).
        ``backward()`` on any scalar built from them runs the agents' HIP vector-Jacobian products (include/mmg.h:
        mmg_exchange_vjp) and fills ``p.grad`` of the modules' parameters, so that ``clip_grad_norm_`` and ``torch.optim``
        work as in the reference (model.py:1307-1330).  Constants, as in the reference: the sampled bits, the masks, data,
        desc.  ``sender.h_x``, ``receiver.h_z`` and ``receiver.h_w`` stay plain tensors (no gradient flows into them).
        The nodes read the engine's tape: backward() must run before the next exchange / train_step on the same batch shape
        (a stale tape raises RuntimeError).  Otherwise exchange() returns exactly what it returns without autograd.

        Differentiable channel (opt-in on top of autograd): with ``exchange_args["channel_grad"] = True`` (or
        ``Game(..., channel_grad=True)``) the sender and the receiver are ONE node (_ChannelVJP; include/mmg.h:
        mmg_exchange_vjp_channel): the messages are not detached, so a loss on ``y`` alone trains the sender too.  Continuous
        messages: the exact gradient through the logits.  Binary: the straight-through estimator, z = pz + stopgrad(bits - pz),
        w = pw + stopgrad(bits - pw).  Same outputs, same values, same rules; the baselines keep their own nodes, the stop bit
        stays a constant.  Without autograd being active the option changes nothing.

        Input gradients (opt-in on top of autograd, combines with channel_grad): with ``exchange_args["input_grad"] = True`` (or
        ``Game(..., input_grad=True)``) ``exchange_args["data"]`` and ``exchange_args["desc"]`` are tensor inputs of the nodes:
        where they require grad, backward() also returns d data (from the sender's node) and d desc (from the receiver's; both
        from the joint node under channel_grad) in their own shape, dtype and device (include/mmg.h: mmg_vjp_input_grads), so
        that an encoder in front of ``data`` or an embedding table behind ``desc`` trains with the agents.  softmax(y) inside dbar
        stays a constant (model.py:441); baseline_sen reads h_x detached (model.py:835).  Without the option, or without autograd
        being active, both stay constants and nothing changes.

        Relaxed messages (``Game(..., relax=dict(tau_sen=..., tau_rec=..., hard=...))``, ``set_relaxation()``, or
        ``exchange_args["relax"]`` for this call; on top of autograd and channel_grad, binary messages): a training conversation
        forms its messages as sigmoid((logit + logistic noise) / tau) from the uniforms the Bernoulli samples draw, and the joint
        node's backward is the exact gradient of that forward (include/mmg.h: mmg_set_message_relaxation).  Same return structure:
        the message lists hold the relaxed (soft) or rounded (hard) values, detached -- the gradient through them is inside the
        node --, the probabilities, y and s_probs are the node's outputs; bs / br are plain tensors."""
        data, target, desc = exchange_args["data"], exchange_args.get("target"), exchange_args["desc"]
        train = exchange_args["train"]
        relax = (relax_setting(exchange_args["relax"]) if "relax" in exchange_args else self.relax) if train else None
        if relax:
            self._check_relax(bool(exchange_args.get("autograd", self.autograd)), bool(exchange_args.get("channel_grad", self.channel_grad)))
        break_early = exchange_args.get("break_early", False)
        autograd = bool(exchange_args.get("autograd", self.autograd)) and bool(train) and torch.is_grad_enabled()
        inputs = (data, desc) if autograd and bool(exchange_args.get("input_grad", self.input_grad)) else (None, None)
        if autograd and self.flipout and bool(exchange_args.get("channel_grad", self.channel_grad)):
            raise NotImplementedError("channel_grad with message flips: the straight-through surrogate under a flip is not defined")
        if autograd:
            self._refuse_variant_graph(bool(exchange_args.get("channel_grad", self.channel_grad)),
                                       bool(exchange_args.get("input_grad", self.input_grad)))
        if autograd and self.world > 1:
            raise NotImplementedError("autograd through exchange() runs on one GPU only (data-parallel training: Game.train_step)")
        corrupt_mask = None
        if exchange_args.get("corrupt", False):                          # model.py:813-820 (eval_dev's call, model.py:637-638)
            if train:
                raise NotImplementedError("message corruption of training conversations is outside the accelerated hot path")
            corrupt_mask = misc.build_mask(exchange_args.get("corrupt_region"), self.cfg["w_dim"])
        context = exchange_args.get("data_context")
        if context is not None and not self.vattn:
            raise NotImplementedError("data_context needs a Sender built with use_attn=True (visual attention)")
        if self.vattn:
            if autograd:
                raise NotImplementedError("visual attention with autograd is not available")
            n_feats = self.check_map(data)
            context = self.check_context(context, data.size(0))
        if self.attn_dim:
            if autograd:
                raise NotImplementedError("desc_attn with autograd is not available: Game.train_step trains an attention receiver")
            if exchange_args.get("desc_set") is not None or self._desc_set is None:
                self.set_desc_set(exchange_args.get("desc_set"), exchange_args.get("desc_set_lens"))     # model.py:765-766
        for k, m in self.modules.items():
            if m is not None and (train or k in ("sender", "receiver")):
                m.train(train)
        B = data.size(0)
        eng = self.engine_for(B, desc.size(0), **(dict(n_feats=n_feats) if self.vattn else {}))
        dev = eng.device
        data = data.detach().to(dev, torch.float32).contiguous().view(B, -1)         # (a map stays [B, C, h * w] in memory: read in place)
        desc = desc.detach().to(dev, torch.float32).contiguous()
        target = None if target is None else target.to(dev, torch.int64).contiguous()
        if self.vattn:
            eng.set_data_context(context)
        self._call += 1
        # exchange_args["uniforms"] (training): (u_z [T, B, W], u_s [T, B], u_w [T, B, W]) in place of the Philox stream -- the
        # reference's numpy draws (model.py:227, 420, 460), for tests that replay one conversation on two paths
        u = exchange_args.get("uniforms") if train else None
        u = [None if v is None else torch.as_tensor(v).to(dev, torch.float32).contiguous() for v in (u or (None, None, None))]
        held = getattr(eng, "relaxation", None)
        if train and relax != held:                                     # (this call's own setting: restored behind the forward)
            eng.set_message_relaxation(*(relax or (None, None)))
        try:
            eng.forward(data, target, desc, u[0], u[1], u[2], seed=self.seed, train=train, run_all=True,
                        **({} if corrupt_mask is None else dict(corrupt_mask=corrupt_mask)))
        finally:
            if train and relax != held:
                eng.set_message_relaxation(*(held or (None, None)))
        tp = eng.tape
        T = self.max_exchange
        n = T
        if break_early:                                                   # model.py:866 (one host sync)
            alive = tp["mask"][1:, :, 0].sum(1).tolist()
            for t, a in enumerate(alive):
                if a == 0:
                    n = t + 1
                    break
        binary = self.cfg["use_binary"]
        masks = [tp["mask"][t].clone() for t in range(n + 1)]
        masks[-1].zero_()                                                 # model.py:870
        self.modules["sender"].h_x = tp["hx"]
        if self.vattn:                                                    # model.py:189, 195: the last executed step's h_x, every step's weights
            self.modules["sender"].h_x = tp["vattn_hx"][n - 1].clone()
            self.modules["sender"].attn_scores = [tp["vattn_alpha"][t].clone() for t in range(n)]
        self.modules["receiver"].h_z = tp["h"][n]
        self.modules["receiver"].h_w = tp["g"][n - 1]
        if autograd:
            return self._exchange_graph(eng, data, desc, n, masks, bool(exchange_args.get("channel_grad", self.channel_grad)), inputs,
                                        relax=relax)
        s = (masks, [tp["s"][t].clone() for t in range(n)], [tp["ps"][t].clone() for t in range(n)])
        sen_w = ([tp["z"][t].clone() for t in range(n)], [tp["pz"][t].clone() if binary else None for t in range(n)])
        rec_w = ([tp["w"][t].clone() for t in range(n)], [tp["pw"][t].clone() if binary else None for t in range(n)])
        y = [tp["y"][t].clone() for t in range(n)]
        bs = [tp["bs"][t].clone() for t in range(n)] if train and binary else []
        br = [tp["br"][t].clone() for t in range(n)] if train and binary else []
        return s, sen_w, rec_w, y, bs, br

    def _exchange_graph(self, eng, data, desc, n, masks, channel=False, inputs=(None, None), relax=None):
        """exchange()'s return structure with the four agents' autograd nodes (training, run-all tape of this call).
        channel: the sender and the receiver share one node (_ChannelVJP).  inputs: the caller's (data, desc) tensors under
        input_grad -- tensor inputs of the sender's / the receiver's / the joint node."""
        tp, binary = eng.tape, self.cfg["use_binary"]
        data_in, desc_in = inputs

        def node(fn, agent, outs, data_in=None, desc_in=None):
            mod = self.modules[agent]
            names = [name for name, _ in mod.named_parameters()]
            spec = dict(eng=eng, gen=eng.generation, n=n, x=data, desc=desc, names=names, outs=outs)
            return fn.apply(spec, data_in, desc_in, *[p for _, p in mod.named_parameters()])

        if channel:
            named = [(a, name, p) for a in ("sender", "receiver") for name, p in self.modules[a].named_parameters()]
            spec = dict(eng=eng, gen=eng.generation, n=n, x=data, desc=desc, names=[(a, name) for a, name, _ in named], relax=relax,
                        outs=[tp["pz" if binary else "z"][:n], tp["y"][:n], tp["ps"][:n], tp["pw" if binary else "w"][:n]])
            sen_st, y_st, ps_st, w_st = _ChannelVJP.apply(spec, data_in, desc_in, *[p for _, _, p in named])
            sen = sen_st.unbind(0)
        else:
            sen = node(_SenderVJP, "sender", [tp["pz" if binary else "z"][:n]], data_in=data_in)[0].unbind(0)
            y_st, ps_st, w_st = node(_ReceiverVJP, "receiver", [tp["y"][:n], tp["ps"][:n], tp["pw" if binary else "w"][:n]],
                                     desc_in=desc_in)
        ps, rw, y = ps_st.unbind(0), w_st.unbind(0), list(y_st.unbind(0))
        s = (masks, [tp["s"][t].clone() for t in range(n)], list(ps))
        if binary:
            sen_w = ([tp["z"][t].clone() for t in range(n)], list(sen))
            rec_w = ([tp["w"][t].clone() for t in range(n)], list(rw))
            if relax:                             # (the baselines are REINFORCE machinery: no VJP on a relaxed handle)
                bs, br = [tp["bs"][t].clone() for t in range(n)], [tp["br"][t].clone() for t in range(n)]
            else:
                bs = list(node(_BaselineSenVJP, "baseline_sen", [tp["bs"][:n]])[0].unbind(0))
                br = list(node(_BaselineRecVJP, "baseline_rec", [tp["br"][:n]])[0].unbind(0))
        else:
            sen_w = (list(sen), [None] * n)
            rec_w = (list(rw), [None] * n)
            bs, br = [], []
        return s, sen_w, rec_w, y, bs, br

    def eval_forward(self, data, target, desc, corrupt_mask=None, data_context=None):
        """The eval-mode conversation of exchange() (rounded messages, cumulative-product stop bit, every sample runs all
        max_exchange steps) WITHOUT slicing / cloning the tape into the reference's per-step lists and without any host
        synchronisation: returns the engine, whose tape views (mask, s, ps, z, pz, w, pw, y, ...) stay valid until its next
        forward pass.  eval_dev() reduces them on the device (model.py:640-691).  corrupt_mask: misc.build_mask's [W, 1]
        indicator (or W entries of 0 / 1): the sender's messages are corrupted as under -bit_flip (model.py:813-820)."""
        for k in ("sender", "receiver"):
            if self.modules.get(k) is not None:
                self.modules[k].train(False)
        n, acc = getattr(self, "_eval_into", None) or (1, None)       # (eval_steps: n conversations, each reduced into acc)
        B = data.size(0) // n
        if data_context is not None and not self.vattn:
            raise NotImplementedError("data_context needs a Sender built with use_attn=True (visual attention)")
        if self.vattn:                                                # data: the maps [n * B, C, h, w]; the context [n * B, G]
            eng = self.vattn_engine_for(data, desc.size(0), n=n)
            eng.set_data_context(self.check_context(data_context, data.size(0)), n=n)
            self.modules["sender"].reset_state()
        else:
            eng = self.engine_for(B, desc.size(0))
        dev = eng.device
        data = data.to(dev, torch.float32).contiguous().view(n * B, -1)
        desc = desc.to(dev, torch.float32).contiguous()
        target = None if target is None else target.to(dev, torch.int64).contiguous()
        self._call += 1
        if acc is not None:
            acc.add(eng, data, target, desc, n, corrupt_mask=corrupt_mask)
            return eng
        eng.forward(data, target, desc, seed=self.seed, train=False, run_all=True,
                    **({} if corrupt_mask is None else dict(corrupt_mask=corrupt_mask)))
        return eng

    def eval_accumulator(self, n_classes, top_k, profile=False, codes=None, meaning=None):
        return EvalAccumulator(n_classes, top_k, profile=profile, codes=codes, meaning=meaning)

    def eval_steps(self, data, target, desc, n, acc, corrupt_mask=None, data_context=None):
        """n consecutive dev batches (data [n * B, F], target [n * B], as train_steps lays them out) evaluated by ONE library
        call (include/mmg.h: mmg_eval_steps): each conversation of eval_forward() is followed by the library's reduction launch,
        which adds the batch's top-k hits, confusion counts and classes seen to `acc` (eval_accumulator(); the calls of one
        evaluation share it, whatever their batch size) and writes its conversation lengths, step count and Hamming counts
        (model.py:640-691).  No host synchronisation; acc.fetch() copies the results once.  Returns the engine, whose tape
        holds the last batch.  The conversations go through eval_forward(), the one place an evaluation conversation is
        enqueued: whatever wraps it (a corruption mask handed in by a caller) sees these too."""
        if n < 1:
            raise ValueError("eval_steps: n must be >= 1")
        if target is None:
            raise ValueError("eval_steps: the reductions need the targets")
        self._eval_into = (int(n), acc)
        try:
            return self.eval_forward(data, target, desc, corrupt_mask=corrupt_mask,
                                     **({} if data_context is None else dict(data_context=data_context)))
        finally:
            self._eval_into = None

    # ------------------------------------------------------------------ model.py:1240-1339
    def train_step(self, data, target, desc, uniforms=None, full_tape=False, data_context=None):
        """exchange + masks + losses + four backward/clip/optimizer blocks, fused on the device.
        Nothing is copied to the host; read ``losses()`` when a log line needs them.
        The step keeps only what training reads (include/mmg.h: run_all_steps == 2): per-(step, sample) tape arrays are valid on
        the LIVE rows (t <= tstar[b]) only, in Fixed mode tape["y"] holds the output step only, and in continuous mode
        (-nouse_binary) the arrays a / c / zr / dbar / g / w are NOT written -- code that wants them after a training step
        calls exchange() (run-all) instead.  model.run's sample dump reads live rows of binary runs only
        (flags.default_flags sets -exchange_samples 0 without -use_binary, model.py:1758-1759).

        full_tape=True (the minibatches that write a log block, model.py:1342-1542): the SAME update through the phased calls
        with every sample running all steps of the conversation (run-all), so that the tape holds what the reference's log
        block prints -- the class logits of stopped samples too ("Entropy Receiver Predictions" is a mean over the whole
        batch at every executed step, model.py:880-886) and every row of the sample dump.  Early exit == run-all and
        fused == phased are parity-tested (tests/test_hip_parity.py); the extra launches cost ~30 us once per log_interval."""
        B = data.size(0)
        self._refuse_relaxed_step("train_step")
        if self.vattn:                                # data: the map [B, C, h, w], read in place; data_context: [B, G]
            eng = self._vattn_train_engine(data, desc, data_context)
            data = data.detach().to(eng.device, torch.float32).contiguous().view(B, data.size(1), -1)
        else:
            eng = self.train_engine_for(B, desc.size(0))
        u = uniforms or (None, None, None)
        # the Philox minibatch counter and the optimizer step (Adam bias correction) live in each engine's workspace: hand
        # them over when the batch size / class count -- hence the engine -- changes between steps
        last = getattr(self, "_train_engine", None)
        if last is not None and last is not eng:
            self._hand_over_counters(eng, last)
        self._train_engine = eng
        self._agent_steps = None                      # (the device counts move: set_agent_step reads them again)
        if self.world > 1:
            dp = self._dp.get(id(eng))
            if dp is None:
                from .dist import DataParallel
                dp = self._dp[id(eng)] = DataParallel(eng, group=self.group)
            dp.train_step(data, target, desc, u[0], u[1], u[2], seed=self.seed, full_tape=full_tape)
        elif full_tape:
            eng.forward(data, target, desc, u[0], u[1], u[2], seed=self.seed, train=True, run_all=True, log_tape=True)
            eng.loss_stats()
            eng.backward(data, target, desc)
            eng.clip_step()
        else:
            eng.train_step(data, target, desc, u[0], u[1], u[2], seed=self.seed)
        return eng

    def train_steps(self, data, target, desc, n, data_context=None):
        """n consecutive plain minibatches (no log block) enqueued by ONE library call: data [n * B, F] / target [n * B] in batch
        order (misc.Epoch).  Same updates, same sampling streams as n train_step() calls (tests/test_cli_gpu.py)."""
        B = data.size(0) // n
        self._refuse_relaxed_step("train_steps")
        if self.vattn:
            eng = self._vattn_train_engine(data, desc, data_context, n=n)
            data = data.detach().to(eng.device, torch.float32).contiguous().view(n * B, data.size(1), -1)
        else:
            eng = self.train_engine_for(B, desc.size(0))
        last = getattr(self, "_train_engine", None)
        if last is not None and last is not eng:
            self._hand_over_counters(eng, last)
        self._train_engine = eng
        self._agent_steps = None                      # (the device counts move: set_agent_step reads them again)
        if self.world > 1:
            dp = self._dp.get(id(eng))
            if dp is None:
                from .dist import DataParallel
                dp = self._dp[id(eng)] = DataParallel(eng, group=self.group)
            dp.train_steps(data, target, desc, n, seed=self.seed)
        elif hasattr(eng, "train_steps"):
            eng.train_steps(data, target, desc, n, seed=self.seed)
        else:                                            # (an engine stand-in without the C loop: tests/oracle_engine.py)
            for i in range(n):
                eng.train_step(data[i * B:(i + 1) * B], target[i * B:(i + 1) * B], desc, seed=self.seed)
        return eng

    def counters(self):
        """[minibatch counter (Philox stream), optimizer step] of the engine that trained last (checkpointed by model.py)."""
        eng = getattr(self, "_train_engine", None) or self.engine
        c = eng.tape["counter"].cpu().tolist()
        return [int(c[0]), int(max(c[1], c[2]))]

    def set_counters(self, minibatch, step):
        for eng in self.engines.values():
            eng.tape["counter"][0] = int(minibatch)
            eng.tape["counter"][1:3] = int(step)

    def losses(self, batch, n_classes):
        return self.engine_for(batch, n_classes).losses()


def exchange(sender, receiver, baseline_sen, baseline_rec, exchange_args):
    """Drop-in for model.py:725: same arguments, same returned structure
    ``(s, sen_w, rec_w, y, bs, br)`` of per-step tensor lists."""
    game = getattr(sender, "_game", None)
    if game is None:
        game = Game(sender, receiver, baseline_sen, baseline_rec)
    elif baseline_sen is not None and game.modules.get("baseline_sen") is None:
        game.modules["baseline_sen"], game.modules["baseline_rec"] = baseline_sen, baseline_rec
    return game.exchange(exchange_args)


def get_rec_outp(y, masks):
    """model.py:879-904 (host-side tensor ops on the returned lists; used by callers of exchange())."""
    import torch.nn.functional as F

    def negent(yy):
        probs = F.softmax(yy, dim=1)
        return (torch.log(probs + 1e-8) * probs).sum(1).mean()
    negentropy = [negent(yy) for yy in y]
    if masks is not None:
        batch_size = y[0].size(0)
        inp = torch.cat([yy.view(batch_size, 1, -1) for yy in y], 1)
        mask = torch.cat(masks, 1).view(batch_size, len(masks), 1).expand_as(inp)
        return torch.masked_select(inp, mask.bool()).view(batch_size, -1), negentropy
    return y[-1], negentropy
