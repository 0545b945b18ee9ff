"""Engine: owns the flat parameter / gradient / optimizer-state buffers and the workspace of one
libmmg handle on one GPU, and exposes the phases of the reference's per-minibatch block
(model.py:1240-1339) as methods.  PyTorch is used for device memory and streams only."""
import ctypes as C

import numpy as np
import torch

from . import _lib

_TORCH_DTYPE = {0: torch.float32, 1: torch.uint8, 2: torch.int32, 3: torch.float64}


def check_desc_set(desc_set, lens, n_classes, wv_dim):
    """What an attention receiver needs of (desc_set, lens): [n_words, wv_dim] word vectors and n_classes positive lengths that sum
    to n_words (a class without a word has no softmax segment).  Raises ValueError."""
    if desc_set is None or lens is None:
        raise ValueError("desc_attn needs desc_set and desc_set_lens")
    lens = [int(v) for v in lens]
    if desc_set.dim() != 2 or desc_set.size(1) != wv_dim:
        raise ValueError("desc_set must be [n_words, %d], got %s" % (wv_dim, tuple(desc_set.shape)))
    if len(lens) != n_classes:
        raise ValueError("desc_set_lens has %d entries for %d classes" % (len(lens), n_classes))
    if any(v <= 0 for v in lens):
        raise ValueError("desc_set_lens: every class needs at least one word (zero-length description at class %d)"
                         % [i for i, v in enumerate(lens) if v <= 0][0])
    if sum(lens) != desc_set.size(0):
        raise ValueError("desc_set_lens sum to %d, desc_set has %d words" % (sum(lens), desc_set.size(0)))


def steps_from_counter(counter):
    """{agent: optimizer steps that updated it} of a tape "counter" tensor (Engine.agent_steps; Game reads the counter of whichever
    engine trained last through this).  Words the tensor does not hold read zero: a 4-word counter carries the global count alone."""
    c = counter.cpu().tolist()
    step, sat_out = int(max(c[1], c[2])), c[4:8] + [0] * 4
    return {a: step - int(sat_out[i]) for i, a in enumerate(_lib.AGENTS)}


class Engine(object):
    def __init__(self, device="cuda:0", share=None, attn_dim=0, n_words=0, vattn=None, **cfg_kwargs):
        """share: another Engine whose flat parameter / gradient / optimizer-state buffers this one
        uses too (same model, different batch size or class count).
        attn_dim > 0: a description-attention handle (include/mmg.h: mmg_attn_create) for description sets of n_words words --
        six more receiver tensors, more tape arrays ("alpha", ...); set_desc_set() uploads a set before the first conversation.
        vattn = (attn_dim, n_feats, context_dim): a visual-attention handle (include/mmg.h: mmg_vattn_create) -- x of every entry is
        the [B, C, n_feats] feature map, six (eight with a context) more sender tensors, the tape arrays "vattn_alpha", "vattn_xa",
        "vattn_hx", ...; set_data_context() states the context before a conversation.  Not together with attn_dim."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MmgError("no GPU visible: the exchange path runs on MI355X only (no CPU fallback)")
        self.device = torch.device(device)
        self.cfg = _lib.make_config(**cfg_kwargs)
        self.cfg_kwargs = dict(cfg_kwargs)
        self.use_binary = bool(self.cfg.use_binary)
        self.attn_dim, self.n_words = int(attn_dim), int(n_words) if attn_dim else 0
        attn = (self.attn_dim, self.n_words)
        self._set_key = None
        self.vattn = tuple(int(v) for v in vattn) if vattn and int(vattn[0]) else None
        self._ctx = None
        if self.vattn and self.attn_dim:
            raise _lib.MmgError("visual attention together with description attention is not available")
        lib = self.lib
        if self.vattn:             # the (cfg, attn_dim, n_feats, context_dim) twins in place of the (cfg, attn_dim, n_words) ones
            attn = self.vattn
            count, grad_floats, ws_size, create = (lib.mmg_vattn_param_count, lib.mmg_vattn_grad_floats, lib.mmg_vattn_workspace_bytes,
                                                   lib.mmg_vattn_create)
        else:
            count, grad_floats, ws_size, create = (lib.mmg_attn_param_count, lib.mmg_attn_grad_floats, lib.mmg_attn_workspace_bytes,
                                                   lib.mmg_attn_create)
        n = count(C.byref(self.cfg), *attn)
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        self.n_params = int(n)
        with torch.cuda.device(self.device):
            if share is not None:
                assert share.n_params == self.n_params and share.device == self.device
                self.flat_params, self.flat_grads, self.opt_state = share.flat_params, share.flat_grads, share.opt_state
            else:
                self.flat_params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
                # gradients + the library's tail quad (dependency-error flag; all-reduced WITH the gradients in DP)
                self.flat_grads = torch.zeros(int(grad_floats(C.byref(self.cfg), *attn)), dtype=torch.float32, device=self.device)
                self.opt_state = torch.zeros(2 * self.n_params, dtype=torch.float32, device=self.device)
            ws_bytes = int(ws_size(C.byref(self.cfg), *attn))
            self.workspace = torch.zeros(ws_bytes, dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)
            self.handle = create(C.byref(self.cfg), *attn, self.workspace.data_ptr(), ws_bytes,
                                 self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.opt_state.data_ptr())
        if not self.handle:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        # parameter views: {agent: {state_dict key: tensor view into flat_params}}
        self.param_entries = _lib.param_table(self.cfg, vattn=self.vattn) if self.vattn else _lib.param_table(self.cfg, *attn)
        self.params = {a: {} for a in _lib.AGENTS}
        self.grads = {a: {} for a in _lib.AGENTS}
        for e in self.param_entries:
            numel = e["rows"] * max(e["cols"], 1)
            shape = (e["rows"], e["cols"]) if e["cols"] else (e["rows"],)
            self.params[e["agent"]][e["name"]] = self.flat_params[e["offset"]:e["offset"] + numel].view(shape)
            self.grads[e["agent"]][e["name"]] = self.flat_grads[e["offset"]:e["offset"] + numel].view(shape)
        self.agent_range = {}
        for e in self.param_entries:
            lo, hi = self.agent_range.get(e["agent"], (1 << 62, 0))
            numel = e["rows"] * max(e["cols"], 1)
            self.agent_range[e["agent"]] = (min(lo, e["offset"]), max(hi, e["offset"] + ((numel + 3) // 4) * 4))
        # tape views
        self.tape = {}
        for e in (_lib.tape_table(self.cfg, vattn=self.vattn) if self.vattn else _lib.tape_table(self.cfg, *attn)):
            dt = _TORCH_DTYPE[e["dtype"]]
            numel = 1
            for d in e["dims"]:
                numel *= d
            nbytes = numel * torch.empty((), dtype=dt).element_size()
            self.tape[e["name"]] = self.workspace[e["offset"]:e["offset"] + nbytes].view(dt).view(e["dims"])
        self.stats = self.tape["stats"]
        # bumped by every call that rewrites the forward tape (forward, train_step(s), dp_*, the agent-level forwards): an autograd
        # node of Game.exchange() refuses to run its VJP on a tape that is no longer the one its forward left
        self.generation = 0
        # parameter version, shared by the engines over the same flat buffers: bumped by every call that changes the parameters
        # (or the optimizer state) behind torch's back -- load_state_dicts, clip_step, train_step(s), dp_train_step(s).  A node of
        # an agent module's forward() refuses to run its VJP on parameters that are no longer its forward's.
        self._param_version = share._param_version if share is not None else [0]

    @property
    def param_version(self):
        return self._param_version[0]

    def bump_param_version(self):
        self._param_version[0] += 1

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.mmg_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ptr(t, dtype=None):
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
        if dtype is not None:
            assert t.dtype == dtype, (t.dtype, dtype)
        return C.c_void_p(t.data_ptr())

    def load_state_dicts(self, sd):
        """sd: {agent: {key: array-like}} -> copied into the flat parameter buffer."""
        self.bump_param_version()
        for agent, d in sd.items():
            for k, v in d.items():
                self.params[agent][k].copy_(torch.as_tensor(v, dtype=torch.float32).to(self.device).view_as(self.params[agent][k]))

    def state_dicts(self):
        return {a: {k: v.detach().cpu().clone() for k, v in d.items()} for a, d in self.params.items()}

    # ------------------------------------------------------------------ phases
    def forward(self, x, target, desc, u_z=None, u_s=None, u_w=None, seed=0, train=True, run_all=False, minimal=False, log_tape=False,
                corrupt_mask=None):
        """run_all: every sample runs all T steps (what exchange() returns).  minimal (training only): store just what the
        backward pass reads (include/mmg.h: run_all_steps == 2) -- what the fused mmg_train_step does.  log_tape (training
        only): run_all for the conversation, the baselines on the live rows only (run_all_steps == 3: a log minibatch).
        corrupt_mask (evaluation only): W entries of 0 / 1 (misc.build_mask's [W, 1] indicator does) -- the sender's message of
        every step becomes |z - m| before the receiver reads it (model.py:813-820).  The mask is set for this call only: the
        engine may serve a training step next."""
        f32 = torch.float32
        self.generation += 1
        self._vattn_gen = None        # (a whole conversation replaces the tables and the context an agent-level Sender.forward left)
        if corrupt_mask is not None:
            if train:
                raise NotImplementedError("message corruption applies to evaluation conversations only (model.py:637-638)")
            self.set_message_corruption(corrupt_mask)
        try:
            _lib.check(self.lib.mmg_exchange_forward(
                self.handle, self._ptr(x, f32), self._ptr(target, torch.int64), self._ptr(desc, f32),
                self._ptr(u_z, f32), self._ptr(u_s, f32), self._ptr(u_w, f32), C.c_uint64(seed),
                int(bool(train)), (3 if log_tape and train else 1) if run_all else (2 if minimal and train else 0), self._stream()))
        finally:
            if corrupt_mask is not None:
                self.set_message_corruption(None)

    def set_message_corruption(self, mask):
        """mask: W entries of 0 / 1, or None to clear (include/mmg.h: mmg_set_message_corruption; host only, no GPU work).  While a
        mask is set the training entries raise; forward(corrupt_mask=...) sets and clears it around one call."""
        if mask is None:
            _lib.check(self.lib.mmg_set_message_corruption(self.handle, None, 0))
            return
        a = np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask).reshape(-1)
        key = (a.dtype.str, a.tobytes())
        cached = getattr(self, "_corrupt_buf", None)
        if cached is None or cached[0] != key:                # (eval_dev hands the same mask to every dev batch: convert it once)
            if a.size != self.cfg.w_dim:
                raise ValueError("corruption mask of %d entries for a %d-bit message" % (a.size, self.cfg.w_dim))
            if not ((a == 0) | (a == 1)).all():
                raise ValueError("corruption mask entries must be 0 or 1")
            cached = self._corrupt_buf = (key, (C.c_uint8 * a.size)(*[int(v) for v in a.tolist()]))
        _lib.check(self.lib.mmg_set_message_corruption(self.handle, cached[1], len(cached[1])))

    def set_message_flipout(self, p_sen=None, p_rec=None, dev=False, eval_seed=0):
        """Random flips of the message bits, the reference's -flipout_sen / -flipout_rec / -flipout_dev (model.py:554-568;
        include/mmg.h: mmg_set_message_flipout).  p_sen / p_rec: flip probability of every bit of the sender's / the receiver's
        message, None = that message is not flipped; both None clears the setting.  dev: evaluation conversations flip too (their
        draws are keyed by eval_seed and a count of the evaluation conversations since this call).  Holds for every later
        forward entry of this engine (forward, train_step(s), dp_train_step(s), eval_steps, sender_forward, receiver_forward);
        binary messages only.  Host only: the library re-selects its kernels, no GPU work."""
        _lib.check(self.lib.mmg_set_message_flipout(
            self.handle, int(p_sen is not None), float(p_sen if p_sen is not None else 0.0), int(p_rec is not None),
            float(p_rec if p_rec is not None else 0.0), int(bool(dev)), C.c_uint64(int(eval_seed) & 0xFFFFFFFFFFFFFFFF)))
        self.flipout = None if p_sen is None and p_rec is None else (p_sen, p_rec, bool(dev))

    def set_sender_variant(self, mix="sum", ignore_code=False, ignore_receiver=False):
        """The sender's communication ablations, the reference's -sender_mix prod / -ignore_code / -ignore_receiver
        (model.py:217-218, 208-210, 470-472; include/mmg.h: mmg_set_sender_variant).  mix: "sum" -- tanh(h_x + h_w) -- or "prod" --
        tanh(h_x * h_w); ignore_code: tanh(h_x), and code_layer / code_bias get exact zero gradients; ignore_receiver (binary
        messages only): the receiver's message is replaced by zeros after it was sampled or rounded.  All defaults clears the
        setting.  Holds for every later forward entry of this engine, its backward pass and the sender's VJPs.  Host only: the
        library re-selects its kernels (a variant runs the generic per-sample family), no GPU work.  Not together with message
        flips."""
        if mix == "mou":
            raise NotImplementedError("sender_mix = 'mou' needs a 4H binary layer: another parameter layout")
        if mix not in ("sum", "prod"):
            raise ValueError("mix = %r: 'sum' or 'prod' expected" % (mix,))
        _lib.check(self.lib.mmg_set_sender_variant(self.handle, _lib.MIX[mix], int(bool(ignore_code)), int(bool(ignore_receiver))))
        variant = (mix, bool(ignore_code), bool(ignore_receiver))
        self.sender_variant = None if variant == ("sum", False, False) else variant

    relaxation = None              # (tau_sen, tau_rec, hard) while set_message_relaxation holds

    def set_message_relaxation(self, tau_sen=None, tau_rec=None, hard=False):
        """Relaxed messages, the Gumbel-sigmoid channel (include/mmg.h: mmg_set_message_relaxation): every message element of a
        training conversation is sigmoid((logit + logistic noise) / tau), the noise formed from the very uniform its Bernoulli
        sample draws -- tau_sen for the sender's message, tau_rec for the receiver's; hard: the message is the bit and the soft
        value carries the gradient (straight-through).  The soft values land in tape["zs"] / tape["ws"].  vjp_channel is the
        backward pass of such an engine; the REINFORCE entries and the detached VJPs raise.  None, None clears the setting.
        Host only; the library re-selects its kernels only when the relaxed state changes, so a training loop may call this
        before every minibatch to anneal the temperatures."""
        if (tau_sen is None) != (tau_rec is None):
            raise ValueError("tau_sen and tau_rec: both temperatures, or None, None to clear the setting")
        if tau_sen is None:
            _lib.check(self.lib.mmg_set_message_relaxation(self.handle, 0.0, 0.0, 0))
            self.relaxation = None
            return
        tau_sen, tau_rec = float(tau_sen), float(tau_rec)
        if not (tau_sen > 0.0 and tau_rec > 0.0):                         # (NaN fails the compare)
            raise ValueError("tau_sen = %r, tau_rec = %r: temperatures must be positive" % (tau_sen, tau_rec))
        _lib.check(self.lib.mmg_set_message_relaxation(self.handle, tau_sen, tau_rec, int(bool(hard))))
        self.relaxation = (tau_sen, tau_rec, bool(hard))

    noise = None                   # (sigma_sen, sigma_rec, dev) while set_message_noise holds

    def set_message_noise(self, sigma_sen=None, sigma_rec=None, dev=False, eval_seed=0):
        """Additive Gaussian noise on CONTINUOUS messages, an AWGN channel (include/mmg.h: mmg_set_message_noise): the sender's
        message of step t becomes logits + sigma_sen * n, the receiver's logits + sigma_rec * n, n standard normal from the
        library's Philox streams 7 / 8 (evaluation: 9 / 10).  None or 0 = that message stays clean; both clears the setting.
        dev: evaluation conversations are noisy too (their draws are keyed by eval_seed and a count of the evaluation
        conversations since this call).  The noisy value is the message everything downstream reads, and the gradient crosses it
        unchanged, so forward, train_step(s), dp_train_step(s), eval_steps, sender_forward / receiver_forward and every VJP work
        on such an engine.  Continuous messages only; not together with attention or a sender variant.  Host only; the library
        re-selects its kernels only when the noisy state changes, so a training loop may call this before every minibatch to
        anneal the sigmas."""
        sig = [0.0 if v is None else float(v) for v in (sigma_sen, sigma_rec)]
        for name, v in zip(("sigma_sen", "sigma_rec"), sig):
            if not 0.0 <= v < float("inf"):                                # (NaN fails both compares)
                raise ValueError("%s = %r: a standard deviation is finite and not negative" % (name, v))
        on = sig[0] > 0.0 or sig[1] > 0.0
        _lib.check(self.lib.mmg_set_message_noise(self.handle, sig[0], sig[1], int(bool(dev) and on),
                                                  C.c_uint64(int(eval_seed) & 0xFFFFFFFFFFFFFFFF)))
        self.noise = (sig[0], sig[1], bool(dev)) if on else None

    # ------------------------------------------------------------------ training controls
    def set_trainable(self, agents):
        """The agents the REINFORCE step updates from the next minibatch on (include/mmg.h: mmg_set_trainable): a collection of agent
        names (_lib.AGENTS) or the mask itself; the others are frozen -- parameters and optimizer state bit-identical, their slice of
        the gradient buffer zero, the forward pass and the other agents' updates unchanged.  Host only, no synchronisation."""
        mask = int(agents) if isinstance(agents, int) else _lib.agent_mask([agents] if isinstance(agents, str) else agents)
        _lib.check(self.lib.mmg_set_trainable(self.handle, mask))

    def set_learning_rate(self, lr):
        """The learning rate of every later minibatch (include/mmg.h: mmg_set_learning_rate): finite, >= 0.  Host only."""
        _lib.check(self.lib.mmg_set_learning_rate(self.handle, float(lr)))

    def set_entropy(self, entropy_s=None, entropy_sen=None, entropy_rec=None):
        """New values of the entropy weights of every later minibatch (include/mmg.h: mmg_set_entropy); None keeps a weight's current
        value.  A weight that was None when the engine was created stays absent, whatever is passed.  Host only."""
        cur = self.training_controls()
        vals = [float((cur[k] or 0.0) if v is None else v) for k, v in (("entropy_s", entropy_s), ("entropy_sen", entropy_sen), ("entropy_rec", entropy_rec))]
        _lib.check(self.lib.mmg_set_entropy(self.handle, *vals))

    def training_controls(self):
        """dict(trainable = tuple of agent names, mask, learning_rate, entropy_s, entropy_sen, entropy_rec): what the next minibatch
        trains with (include/mmg.h: mmg_get_training_controls).  An entropy weight the engine was created without reads None."""
        mask, lr, ent = C.c_int(0), C.c_float(0.0), (C.c_float * 3)()
        _lib.check(self.lib.mmg_get_training_controls(self.handle, C.byref(mask), C.byref(lr), ent))
        has = (self.cfg.has_entropy_s, self.cfg.has_entropy_sen, self.cfg.has_entropy_rec)
        out = dict(mask=mask.value, trainable=tuple(a for i, a in enumerate(_lib.AGENTS) if (mask.value >> i) & 1), learning_rate=float(lr.value))
        for k, h, v in zip(("entropy_s", "entropy_sen", "entropy_rec"), has, ent):
            out[k] = float(v) if h else None
        return out

    def agent_steps(self):
        """{agent: optimizer steps that updated it}: the global step count (tape "counter"[1], [2] while a step is not committed yet)
        minus the steps the agent sat out frozen ("counter"[4 + a]).  One device->host copy."""
        return steps_from_counter(self.tape["counter"])

    def set_desc_set(self, desc_set, lens):
        """The description set of an attention engine (include/mmg.h: mmg_set_desc_set): desc_set [n_words, V], the word vectors of
        all classes concatenated; lens: n_classes positive lengths that sum to n_words.  Copied into the workspace (a blocking
        call); an unchanged (tensor, lens) pair is not uploaded again."""
        if not self.attn_dim:
            raise _lib.MmgError("set_desc_set: not an attention engine (Engine(attn_dim=...))")
        lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
        key = (desc_set.data_ptr(), desc_set._version, tuple(desc_set.shape), tuple(lens))
        if key == self._set_key:
            return
        check_desc_set(desc_set, lens, self.cfg.n_classes, self.cfg.wv_dim)
        if desc_set.size(0) != self.n_words:
            raise ValueError("desc_set has %d words, the engine was created for %d" % (desc_set.size(0), self.n_words))
        dset = desc_set.detach().to(self.device, torch.float32).contiguous()
        arr = (C.c_int32 * len(lens))(*lens)
        _lib.check(self.lib.mmg_set_desc_set(self.handle, self._ptr(dset, torch.float32), arr, int(dset.size(0))))
        self._set_key = key

    def set_data_context(self, context, n=1):
        """The data context of a visual-attention engine's next conversations (include/mmg.h: mmg_set_data_context): [n * B, G],
        read in place -- the engine keeps the fp32 device tensor alive.  None clears it.  Host only."""
        if not self.vattn:
            raise _lib.MmgError("set_data_context: not a visual-attention engine (Engine(vattn=...))")
        if context is not None:
            G = self.vattn[2]
            if not G:
                context = None                                            # (a sender without attn_W_g ignores g, model.py:127-138)
            elif context.dim() != 2 or context.size(1) != G or context.size(0) != n * self.cfg.batch:
                raise ValueError("data_context must be [%d, %d], got %s" % (n * self.cfg.batch, G, tuple(context.shape)))
            else:
                context = context.detach().to(self.device, torch.float32).contiguous()
        self._ctx = context
        _lib.check(self.lib.mmg_set_data_context(self.handle, self._ptr(context, torch.float32)))

    def vattn_reset_state(self):
        """Sender.reset_state() for sender_forward (include/mmg.h: mmg_vattn_reset_state): the next call forms attn_W_x(X) / attn_W_g(g)."""
        _lib.check(self.lib.mmg_vattn_reset_state(self.handle))

    def loss_stats(self):
        _lib.check(self.lib.mmg_loss_stats(self.handle, self._stream()))

    def backward(self, x, target, desc):
        _lib.check(self.lib.mmg_backward(self.handle, self._ptr(x, torch.float32), self._ptr(target, torch.int64),
                                         self._ptr(desc, torch.float32), self._stream()))

    def clip_step(self):
        self.bump_param_version()
        _lib.check(self.lib.mmg_clip_step(self.handle, self._stream()))

    def train_step(self, x, target, desc, u_z=None, u_s=None, u_w=None, seed=0):
        f32 = torch.float32
        self.generation += 1
        self._vattn_gen = None
        self.bump_param_version()
        _lib.check(self.lib.mmg_train_step(
            self.handle, self._ptr(x, f32), self._ptr(target, torch.int64), self._ptr(desc, f32),
            self._ptr(u_z, f32), self._ptr(u_s, f32), self._ptr(u_w, f32), C.c_uint64(seed), self._stream()))

    def train_steps(self, x, target, desc, n, seed=0):
        """n consecutive minibatches enqueued by ONE C call: x [n * B, F], target [n * B] = the epoch's samples in batch order
        (include/mmg.h: mmg_train_steps)."""
        B = self.cfg.batch
        assert x.size(0) >= n * B and target.size(0) >= n * B
        self.generation += 1
        self._vattn_gen = None
        self.bump_param_version()
        _lib.check(self.lib.mmg_train_steps(self.handle, self._ptr(x, torch.float32), self._ptr(target, torch.int64), int(n),
                                            self._ptr(desc, torch.float32), C.c_uint64(seed), self._stream()))

    def eval_acc(self):
        """A zeroed accumulator for eval_steps (include/mmg.h: mmg_eval_acc_count int64 -- hits, batches, samples, 0, the
        [D, D] confusion counts, the [D] classes seen).  Engines of the same class count may share one."""
        n = int(self.lib.mmg_eval_acc_count(C.byref(self.cfg)))
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        return torch.zeros(n, dtype=torch.int64, device=self.device)

    def eval_profile(self):
        """A zeroed communication profile for eval_steps(prof=...) (include/mmg.h: mmg_eval_profile_count int64 -- the head,
        steps [D, T], rank [T, D], class_hits [D], class_ranksum [D], msg_sen / msg_rec [T, D, W]; commstats.parse_profile names
        the blocks).  Engines of the same class count, step count and message width may share one."""
        n = int(self.lib.mmg_eval_profile_count(C.byref(self.cfg)))
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        return torch.zeros(n, dtype=torch.int64, device=self.device)

    def eval_codes(self, cap_rows):
        """(codes [cap_rows, 2, T, Wp] uint32-as-int32, meta [cap_rows, 2] int32) device buffers for eval_steps(codes=...)
        (include/mmg.h: mmg_eval_steps_codes; mmg_eval_code_words() words per row).  Not zeroed: every word of a row is written.
        Engines of the same step count and message width may share them (each writes its own rows)."""
        n = int(self.lib.mmg_eval_code_words(C.byref(self.cfg)))
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        T = self.cfg.max_exchange
        codes = torch.empty(int(cap_rows), _lib.EVAL_CODE_AGENTS, T, n // (_lib.EVAL_CODE_AGENTS * T), dtype=torch.int32, device=self.device)
        return codes, torch.empty(int(cap_rows), _lib.EVAL_CODE_META, dtype=torch.int32, device=self.device)

    def code_pair_hist(self, codes, meta, n_rows, agent, steps, meaning, bins):
        """The pair histogram of the first n_rows rows of (codes, meta) (eval_codes(), filled by eval_steps(codes=...)) against the
        cosine distance of the rows of `meaning` [>= n_rows, F] float32 (include/mmg.h: mmg_code_pair_hist): agent 0 the sender's
        codes, 1 the receiver's; steps = (t0, t1) or None for all T; returns the flat int64 device histogram of
        4 + 2 ((t1 - t0) W + 1) bins entries (commstats.parse_pair_hist names its parts).  Two launches on the current stream, no host
        synchronisation."""
        T, W = int(codes.size(2)), self.cfg.w_dim
        assert codes.dtype == torch.int32 and codes.dim() == 4 and codes.size(1) == _lib.EVAL_CODE_AGENTS and codes.size(3) == _lib.code_wp(W)
        assert codes.size(0) >= n_rows and meta.size(0) >= n_rows and meaning.dim() == 2 and meaning.size(0) >= n_rows
        assert meaning.dtype == torch.float32 and meaning.is_cuda and meaning.stride(1) == 1
        t0, t1 = (0, T) if steps is None else (int(steps[0]), int(steps[1]))
        n = int(self.lib.mmg_code_pair_hist_count(max(t1 - t0, 0), W, int(bins)))
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        hist = torch.zeros(n, dtype=torch.int64, device=self.device)
        inv = torch.empty(int(n_rows), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mmg_code_pair_hist(self._ptr(codes, torch.int32), self._ptr(meta, torch.int32), int(n_rows), T, W, int(agent),
                                               t0, t1, C.c_void_p(meaning.data_ptr()), int(meaning.size(1)), int(meaning.stride(0)),
                                               self._ptr(inv, torch.float32), int(bins), self._ptr(hist, torch.int64), self._stream()))
        return hist

    def eval_steps(self, x, target, desc, n, top_k, acc, lens=None, batch=None, corrupt_mask=None, prof=None, codes=None):
        """n consecutive evaluation conversations (x [n * B, F], target [n * B]), each followed by the library's reduction launch
        (include/mmg.h: mmg_eval_steps): hits / confusion counts / classes seen are ADDED to `acc` (eval_acc()); returns
        (lens [n * B] int32: conversation lengths, batch [n, 1 + 2 T] int64: executed steps | Hamming counts of the sender's
        and of the receiver's messages per step -- float64 bits with continuous messages).  No host synchronisation; the
        minibatch counter is untouched; the tape holds the last batch.  corrupt_mask: as forward().
        prof (eval_profile()): the call is mmg_eval_steps_profile -- the same results, and one more launch per batch ADDS the
        batch's communication profile to `prof`.
        codes = (codes, meta, row0) (eval_codes()): the call is mmg_eval_steps_codes, with or without prof -- the same results, and
        one more launch per batch WRITES every sample's packed message bits and (output step, target) at rows row0 + i B + b."""
        B, T = self.cfg.batch, self.cfg.max_exchange
        assert x.size(0) >= n * B and target.size(0) >= n * B
        assert acc.dtype == torch.int64 and acc.numel() == _lib.EVAL_ACC_HEAD + self.cfg.n_classes * (self.cfg.n_classes + 1)
        if prof is not None:
            D, W = self.cfg.n_classes, self.cfg.w_dim
            assert prof.dtype == torch.int64 and prof.is_contiguous() and prof.numel() == _lib.EVAL_PROF_HEAD + 2 * D * T + 2 * D + 2 * T * D * W
        if lens is None:
            lens = torch.empty(n * B, dtype=torch.int32, device=self.device)
        if batch is None:
            batch = torch.empty(n, 1 + 2 * T, dtype=torch.int64, device=self.device)
        assert lens.numel() >= n * B and batch.numel() >= n * (1 + 2 * T)
        self.generation += 1
        self._vattn_gen = None
        if corrupt_mask is not None:
            self.set_message_corruption(corrupt_mask)
        try:
            args = (self.handle, self._ptr(x, torch.float32), self._ptr(target, torch.int64), int(n), self._ptr(desc, torch.float32),
                    int(top_k), self._ptr(acc, torch.int64), self._ptr(lens, torch.int32), self._ptr(batch, torch.int64))
            if codes is not None:
                cd, meta, row0 = codes
                assert cd.size(0) == meta.size(0) and tuple(cd.shape[1:]) == (_lib.EVAL_CODE_AGENTS, T, _lib.code_wp(self.cfg.w_dim))
                _lib.check(self.lib.mmg_eval_steps_codes(*args, self._ptr(prof, torch.int64), self._ptr(cd, torch.int32),
                                                         self._ptr(meta, torch.int32), int(row0), int(cd.size(0)), self._stream()))
            elif prof is None:
                _lib.check(self.lib.mmg_eval_steps(*args, self._stream()))
            else:
                _lib.check(self.lib.mmg_eval_steps_profile(*args, self._ptr(prof, torch.int64), self._stream()))
        finally:
            if corrupt_mask is not None:
                self.set_message_corruption(None)
        return lens, batch

    def set_allreduce(self, fn_address, comm):
        """RCCL's ncclAllReduce by address + a communicator: the data-parallel step then runs inside ONE C call (dp_train_step)."""
        _lib.check(self.lib.mmg_dp_set_allreduce(self.handle, C.c_void_p(fn_address), comm))

    def dp_train_step(self, x, target, desc, u_z=None, u_s=None, u_w=None, seed=0, full_tape=False, reduce=True):
        f32 = torch.float32
        self.generation += 1
        self.bump_param_version()
        _lib.check(self.lib.mmg_dp_train_step(
            self.handle, self._ptr(x, f32), self._ptr(target, torch.int64), self._ptr(desc, f32),
            self._ptr(u_z, f32), self._ptr(u_s, f32), self._ptr(u_w, f32), C.c_uint64(seed), int(bool(full_tape)), int(bool(reduce)),
            self._stream()))

    def dp_train_steps(self, x, target, desc, n, seed=0, reduce=True):
        B = self.cfg.batch
        assert x.size(0) >= n * B and target.size(0) >= n * B
        self.generation += 1
        self.bump_param_version()
        _lib.check(self.lib.mmg_dp_train_steps(self.handle, self._ptr(x, torch.float32), self._ptr(target, torch.int64), int(n),
                                               self._ptr(desc, torch.float32), C.c_uint64(seed), int(bool(reduce)), self._stream()))

    def log_snapshot(self, target, dump=0, losses=True):
        """What the log block of the last minibatch prints, as ONE flat float64 device vector written by one launch
        (include/mmg.h: mmg_log_snapshot)."""
        n = int(self.lib.mmg_log_snapshot_count(C.byref(self.cfg), int(dump), int(bool(losses))))
        out = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.mmg_log_snapshot(self.handle, self._ptr(target, torch.int64) if target is not None else None, int(dump),
                                             int(bool(losses)), C.c_void_p(out.data_ptr()), self._stream()))
        return out[:n]

    def clear_error(self):
        """Clear a recorded in-launch dependency error (drains the stream; the selected kernels stay)."""
        _lib.check(self.lib.mmg_clear_error(self.handle, self._stream()))

    def plan_text(self):
        """What the kernel selection of this handle decided, and the device caps it decided from (include/mmg.h: mmg_plan_text)."""
        buf = C.create_string_buffer(4096)
        _lib.check(self.lib.mmg_plan_text(self.handle, buf, len(buf)))
        return buf.value.decode()

    def degraded(self):
        """0: role launches in use; 1: launches without in-launch waits since mmg_create; 2: ... since a recovery."""
        return int(self.lib.mmg_degraded(self.handle))

    # ------------------------------------------------------------------ agent-level steps
    def sender_forward(self, x, w, t, train, u_z=None, seed=0):
        B, W, H = self.cfg.batch, self.cfg.w_dim, self.cfg.h_dim
        self.generation += 1
        msg = torch.empty(B, W, device=self.device)
        probs = torch.empty(B, W, device=self.device) if self.cfg.use_binary else None
        h_x = torch.empty(B, H, device=self.device)
        _lib.check(self.lib.mmg_sender_forward(self.handle, self._ptr(x), self._ptr(w), int(t), int(bool(train)),
                                               self._ptr(u_z), C.c_uint64(seed), self._ptr(msg), self._ptr(probs),
                                               self._ptr(h_x), self._stream()))
        return msg, probs, h_x

    def receiver_forward(self, z, desc, h_z, s_prob_prod, first, t, train, u_s=None, u_w=None, seed=0):
        B, W, R, D = self.cfg.batch, self.cfg.w_dim, self.cfg.rec_hidden, self.cfg.n_classes
        dev = self.device
        self.generation += 1
        s, s_prob = torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev)
        w = torch.empty(B, W, device=dev)
        w_probs = torch.empty(B, W, device=dev) if self.cfg.use_binary else None
        y, h_w = torch.empty(B, D, device=dev), torch.empty(B, R, device=dev)
        _lib.check(self.lib.mmg_receiver_forward(
            self.handle, self._ptr(z), self._ptr(desc), self._ptr(h_z), self._ptr(s_prob_prod), int(bool(first)),
            int(t), int(bool(train)), self._ptr(u_s), self._ptr(u_w), C.c_uint64(seed), self._ptr(s),
            self._ptr(s_prob), self._ptr(w), self._ptr(w_probs), self._ptr(y), self._ptr(h_w), self._stream()))
        return s, s_prob, w, w_probs, y, h_w

    def baseline_forward(self, which, x, binary, inp):
        rows = binary.shape[0]
        self.generation += 1
        score = torch.empty(rows, 1, device=self.device)
        _lib.check(self.lib.mmg_baseline_forward(self.handle, _lib.AGENTS.index(which), self._ptr(x), self._ptr(binary),
                                                 self._ptr(inp), rows, self._ptr(score), self._stream()))
        return score

    # ------------------------------------------------------------------ vector-Jacobian products
    def vjp(self, agent, n_steps, x, desc, dy=None, dz=None, dw=None, dps=None, dbs=None, dbr=None):
        """Backward pass of ONE agent's graph of the last training run-all forward (include/mmg.h: mmg_exchange_vjp): writes that
        agent's slice of the gradient buffer (self.grads[agent]) from the upstream gradients of its outputs over the n_steps
        executed steps -- dy [n, B, D], dz / dw [n, B, W] (probabilities when binary, logits when continuous), dps / dbs / dbr
        [n, B] or [n, B, 1]; None = zero.  The caller checks that the tape is still the forward's (self.generation)."""
        f32 = torch.float32
        args = self._upstream(n_steps, dy=dy, dz=dz, dw=dw, dps=dps, dbs=dbs, dbr=dbr)
        _lib.check(self.lib.mmg_exchange_vjp(
            self.handle, _lib.AGENTS.index(agent), int(n_steps), self._ptr(x, f32), self._ptr(desc, f32),
            self._ptr(args["dy"]), self._ptr(args["dz"]), self._ptr(args["dw"]), self._ptr(args["dps"]),
            self._ptr(args["dbs"]), self._ptr(args["dbr"]), self._stream()))

    def _upstream(self, n_steps, **named):
        """Upstream gradients of a tape VJP -> fp32 contiguous device copies, checked to hold n_steps x batch rows; None stays."""
        width = dict(dy=self.cfg.n_classes, dz=self.cfg.w_dim, dw=self.cfg.w_dim, dps=1, dbs=1, dbr=1)
        args = {}
        for k, g in named.items():
            if g is not None:
                g = g.to(self.device, torch.float32).contiguous()
                if g.numel() != n_steps * self.cfg.batch * width[k]:
                    raise ValueError("%s: %d entries for %d steps x %d samples x %d" % (k, g.numel(), n_steps, self.cfg.batch, width[k]))
            args[k] = g
        return args

    def vjp_channel(self, n_steps, x, desc, dy=None, dz=None, dw=None, dps=None):
        """Backward pass of the sender's and the receiver's graphs of the last training run-all forward as ONE graph, the
        messages not detached (include/mmg.h: mmg_exchange_vjp_channel): writes self.grads["receiver"] and self.grads["sender"].
        Upstream gradients as in vjp(); None = zero.  The caller checks that the tape is still the forward's."""
        f32 = torch.float32
        args = self._upstream(n_steps, dy=dy, dz=dz, dw=dw, dps=dps)
        _lib.check(self.lib.mmg_exchange_vjp_channel(
            self.handle, int(n_steps), self._ptr(x, f32), self._ptr(desc, f32), self._ptr(args["dy"]), self._ptr(args["dz"]),
            self._ptr(args["dw"]), self._ptr(args["dps"]), self._stream()))

    def input_grads(self, n_steps, want_dx=False, want_ddesc=False, per_call=False, y=None):
        """d data [B, F] and d desc [D, V] of the VJP that ran LAST on this engine and stream (include/mmg.h:
        mmg_vjp_input_grads): vjp("sender") leaves what d data needs, vjp("receiver") what d desc needs, vjp_channel both; with
        per_call, receiver_vjp (y: that call's class logits).  Returns (d data, d desc), None where not wanted.  Writes no
        gradient slice and no tape array a VJP wrote."""
        c = self.cfg
        dx = torch.empty(c.batch, c.feat_dim, device=self.device) if want_dx else None
        dd = torch.empty(c.n_classes, c.wv_dim, device=self.device) if want_ddesc else None
        if per_call and y is not None:
            y = y.detach().to(self.device, torch.float32).contiguous()
            if y.numel() != c.batch * c.n_classes:
                raise ValueError("y: %d entries for %d samples x %d" % (y.numel(), c.batch, c.n_classes))
        if dx is not None or dd is not None:
            _lib.check(self.lib.mmg_vjp_input_grads(self.handle, int(bool(per_call)), int(n_steps), self._ptr(y if per_call else None),
                                                    self._ptr(dx), self._ptr(dd), self._stream()))
        return dx, dd

    # ------------------------------------------------------------------ per-call vector-Jacobian products
    def _vjp_args(self, named):
        """(name, tensor or None, floats per sample) -> device pointers of fp32 contiguous copies, checked to hold B rows."""
        B, out, keep = self.cfg.batch, [], []
        for name, t, width in named:
            if t is not None:
                t = t.detach().to(self.device, torch.float32).contiguous()
                if t.numel() != B * width:
                    raise ValueError("%s: %d entries for %d samples x %d" % (name, t.numel(), B, width))
                keep.append(t)
            out.append(self._ptr(t))
        return out, keep

    def _grad_out(self, want, width):
        return torch.empty(self.cfg.batch, width, device=self.device) if want else None

    def sender_vjp(self, x, w, t, h_x, probs, dout=None, dh_x=None, want_dx=False, want_dw=False):
        """Backward pass of ONE sender_forward call (include/mmg.h: mmg_sender_vjp): writes self.grads["sender"] from the
        upstream gradients of its probs (binary) | message logits (continuous) and of h_x; returns (d x, d w), None where not
        wanted.  None upstream = zero."""
        c = self.cfg
        (px, pw, phx, pp, pdo, pdh), keep = self._vjp_args(
            (("x", x, c.feat_dim), ("w", w if t > 0 else None, c.w_dim), ("h_x", h_x, c.h_dim),
             ("probs", probs if c.use_binary else None, c.w_dim), ("dout", dout, c.w_dim), ("dh_x", dh_x, c.h_dim)))
        dx, dw = self._grad_out(want_dx, c.feat_dim), self._grad_out(want_dw and t > 0, c.w_dim)
        _lib.check(self.lib.mmg_sender_vjp(self.handle, px, pw, int(t), phx, pp, pdo, pdh, self._ptr(dx), self._ptr(dw),
                                           self._stream()))
        return dx, dw

    def receiver_vjp(self, z, desc, h_prev, h_new, y, w_probs, s_prob, dy=None, dw=None, dps=None, dh_w=None, dh_new=None,
                     want_dz=False, want_dh_prev=False):
        """Backward pass of ONE receiver_forward call (include/mmg.h: mmg_receiver_vjp): writes self.grads["receiver"];
        returns (d z, d h_prev), None where not wanted.  h_prev None: the zero state of a first call.  None upstream = zero."""
        c = self.cfg
        R, W, D = c.rec_hidden, c.w_dim, c.n_classes
        desc = desc.detach().to(self.device, torch.float32).contiguous()
        (pz, ph0, ph1, py, ppw, pps, pdy, pdw, pdps, pdhw, pdhn), keep = self._vjp_args(
            (("z", z, W), ("h_prev", h_prev, R), ("h_new", h_new, R), ("y", y, D), ("w_probs", w_probs if c.use_binary else None, W),
             ("s_prob", s_prob, 1), ("dy", dy, D), ("dw", dw, W), ("dps", dps, 1), ("dh_w", dh_w, R), ("dh_new", dh_new, R)))
        dz, dh0 = self._grad_out(want_dz, W), self._grad_out(want_dh_prev and h_prev is not None, R)
        _lib.check(self.lib.mmg_receiver_vjp(self.handle, pz, self._ptr(desc), ph0, ph1, py, ppw, pps, pdy, pdw, pdps, pdhw, pdhn,
                                             self._ptr(dz), self._ptr(dh0), self._stream()))
        return dz, dh0

    def baseline_vjp(self, which, x, binary, inp, dscore=None, want=(False, False, False)):
        """Backward pass of ONE baseline_forward call (include/mmg.h: mmg_baseline_vjp): writes self.grads[which]; returns
        (d x, d binary, d inp), None where not wanted or absent."""
        c = self.cfg
        widths = (c.h_dim, c.w_dim, c.rec_hidden)
        ins = (x, binary, inp)
        (px, pb, pi, pds), keep = self._vjp_args(
            (("x", x, widths[0]), ("binary", binary, widths[1]), ("inp", inp, widths[2]), ("dscore", dscore, 1)))
        outs = [self._grad_out(wnt and v is not None, wd) for wnt, v, wd in zip(want, ins, widths)]
        _lib.check(self.lib.mmg_baseline_vjp(self.handle, _lib.AGENTS.index(which), px, pb, pi, c.batch, pds,
                                             *[self._ptr(o) for o in outs], self._stream()))
        return tuple(outs)

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on):
        _lib.check(self.lib.mmg_set_profiling(self.handle, int(bool(on))))

    def kernel_times(self, max_kernels=512):
        names = C.create_string_buffer(16384)
        ms = (C.c_float * max_kernels)()
        n = self.lib.mmg_get_kernel_times(self.handle, names, 16384, ms, max_kernels)
        if n < 0:
            raise _lib.MmgError(self.lib.mmg_last_error().decode())
        nm = names.value.decode().split(";")[:n]
        return list(zip(nm, [float(ms[i]) for i in range(n)]))

    def check_sync(self):
        """Raise if an in-launch dependency wait (device_utils.h: role_wait) ever hit its spin bound: word 511 of the
        tape array `sync` holds the dependency number + 1.  Synchronises the device; call it off the hot path."""
        code = int(self.tape["sync"][511].item())
        if code:
            raise _lib.MmgError("in-launch dependency %d timed out on the device (workgroup roles out of order?)" % (code - 1))

    # ------------------------------------------------------------------ results
    def losses(self):
        """dict of the six scalars of model.py:1271-1294 plus n_steps / hits (one device->host copy)."""
        v = self.tape["losses"].cpu().tolist()
        self.check_sync()
        keys = ("nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen", "loss_bas_rec", "loss_bas_sen",
                "n_steps", "hits")
        return dict(zip(keys, v))
