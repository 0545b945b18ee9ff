"""Test-side reference of visual attention (-visual_attn / -attn_extra_context, model.py:80-86, 114-142, 168-195): the CPU oracle
(oracle/cpu_ref) with the attention layers on its Sender and the Sender's forward replaced by a restatement of the reference's
attention branch.  The oracle itself is not edited: the wrapper sits on the sender it is handed (the pattern of
tests/desc_attn_ref.py) and keeps the 4-D feature map and the context in its closure -- cpu_ref.exchange hands the sender its `data`
argument (here a [B, C] stand-in that only carries the batch size) and None for the context.

cpu_ref.fill_state_dicts only knows the reference's seven sender tensors; fill_vattn is the seeded filler of the others.
forward_f64 is a float64 numpy restatement of one sender step, independent of torch, for the checks the reference cannot run in
float64 (it builds a FloatTensor at t == 0)."""
import json
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cpu_ref
from tests import common

VATTN_NAMES = ("attn_W_x.weight", "attn_W_x.bias", "attn_W_w.weight", "attn_W_w.bias", "attn_U.weight", "attn_U.bias")
VATTN_CTX_NAMES = ("attn_W_g.weight", "attn_W_g.bias")

# The shapes of tests/test_visual_attn_gpu.py (their reach conditions: tests/test_visual_attn_cpu.py).
#   A: config 1's agents on the presets' map: 512 channels, 8 x 8 locations, A = 256, a 1000-d context; 16 samples, 4 steps.
#   B: small dimensions that are no multiple of a tile, of a wave or of four, a 2 x 3 map (h != w, C != N: a transposed layout or
#      swapped axes cannot pass), a context, Adam.
#   C: shape B without attn_W_g -- six tensors, and a context that is given is ignored.
#   D: shape B on a 1 x 1 map: alpha == 1 at every step.
#   E: shape B on a 9 x 9 map: 81 locations, longer than a wave and odd.
_C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=16, learning_rate=1e-4, entropy_rec=0.01,
           entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
           rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)
_SMALL = dict(_C1, max_exchange=3, batch_size=5, img_feat_dim=18, img_h_dim=40, rec_w_dim=12, sender_out_dim=12, rec_hidden=20,
              wv_dim=12, baseline_hid_dim=70, optim_type="Adam", top_k_train=2, top_k_dev=2)
# shape: (flags, classes, batch, attn_dim, (h, w), context_dim)
SHAPES = {"A": (_C1, 30, 16, 256, (8, 8), 1000),
          "B": (_SMALL, 7, 5, 5, (2, 3), 7),
          "C": (_SMALL, 7, 5, 5, (2, 3), 0),
          "D": (_SMALL, 7, 5, 5, (1, 1), 7),
          "E": (_SMALL, 7, 5, 5, (9, 9), 7)}
MODES = {"adaptive": dict(use_binary=True, fixed_exchange=False), "fixed": dict(use_binary=True, fixed_exchange=True),
         "continuous": dict(use_binary=False, fixed_exchange=True)}
# Data seeds searched on the CPU oracle (tests/test_visual_attn_cpu.py asserts what they reach): no probability of the evaluation
# conversation lies within 1e-4 of 0.5, and at some step t >= 1 the attention weights are more than 1e-2 away from 1 / N.
DATA_SEED = {"A": 27, "B": 7, "C": 7, "D": 27, "E": 9}


def load_golden(name):
    """A g13 fixture as (dict of arrays, meta), the float64 scalars unpacked again (tests/golden/make_golden_visual_attn.py)."""
    z, m = common.load_golden(name)
    out = {k: z[k] for k in z.files if k not in ("scalars", "scalar_keys", "meta")}
    out.update({k: np.float64(v) for k, v in zip(json.loads(str(z["scalar_keys"])), z["scalars"])})
    return out, m


def meta(shape, mode="adaptive", **over):
    """The meta dict (tests/common.py: flags_from_meta, case_inputs) of a shape: weights seed 5, uniforms seed 7."""
    flags, n_classes, batch, attn_dim, hw, ctx = SHAPES[shape]
    m = dict(cpu_ref.Flags(**dict(flags, **MODES[mode])).__dict__)
    m.update(n_classes=n_classes, batch=batch, n_minibatches=1, seed_weights=5, seed_data=DATA_SEED[shape], seed_uniforms=7,
             vattn_dim=attn_dim, map_hw=list(hw), context_dim=ctx, shape=shape)
    m.update(over)
    return m


def feature_map(m, i=0):
    """Seeded map [B, C, h, w] of minibatch i (0.5 N(0, 1), the scale of cpu_ref.synthetic_batch's features) and context [B, G]
    (None without attn_W_g); streams of their own, so that target and desc stay what common.case_inputs gives."""
    h, w = m["map_hw"]
    rs = np.random.RandomState(m["seed_data"] + i + 2000)
    x = (0.5 * rs.standard_normal((m["batch"], m["img_feat_dim"], h, w))).astype(np.float32)
    g = (0.5 * rs.standard_normal((m["batch"], m["context_dim"]))).astype(np.float32) if m["context_dim"] else None
    return x, g


def vattn_names(m):
    return VATTN_NAMES + (VATTN_CTX_NAMES if m["context_dim"] else ())


def fill_vattn(m, seed=None, gain=2.0):
    """{name: float32 ndarray} of the attention tensors in the reference's state_dict order: Xavier-normal 2-D tensors times `gain`,
    N(0, 0.05) biases (cpu_ref.fill_state_dicts' rule), from a stream of their own.  gain: plain Xavier weights give scores so close
    together that alpha stays within 1e-3 of 1 / N and a kernel that ignored the scores would pass; tests/test_visual_attn_cpu.py
    asserts that alpha moves away from uniform."""
    A, C, W, G = m["vattn_dim"], m["img_feat_dim"], m["rec_w_dim"], m["context_dim"]
    shapes = {"attn_W_x.weight": (A, C), "attn_W_x.bias": (A,), "attn_W_w.weight": (A, W), "attn_W_w.bias": (A,),
              "attn_U.weight": (1, A), "attn_U.bias": (1,), "attn_W_g.weight": (A, G), "attn_W_g.bias": (A,)}
    rs = np.random.RandomState((m["seed_weights"] if seed is None else seed) + 777)
    out = {}
    for name in vattn_names(m):
        shape = shapes[name]
        std = gain * math.sqrt(2.0 / (shape[0] + shape[1])) if len(shape) == 2 else 0.05
        out[name] = (rs.standard_normal(shape) * std).astype(np.float32)
    return out


def attention_sender(sender, attn_dim, context_dim, xmap, g, transposed=False):
    """sender gets attn_W_x / attn_W_w / attn_U (/ attn_W_g) (model.py:80-86) and its forward becomes model.py:114-238 with
    use_attn on, over the map `xmap` [B, C, h, w] and the context `g` of its closure.  transposed: read the map as if it were
    [B, h * w, C] in memory -- the layout the reference does NOT have."""
    sender.attn_dim, sender.attn_extra_context = attn_dim, context_dim > 0
    sender.attn_W_x = nn.Linear(sender.feat_dim, attn_dim)
    sender.attn_W_w = nn.Linear(sender.w_dim, attn_dim)
    sender.attn_U = nn.Linear(attn_dim, 1)
    if context_dim:
        sender.attn_W_g = nn.Linear(context_dim, attn_dim)
    plain_forward = sender.forward
    sender.vattn_inputs = [xmap, g]                                       # (train_minibatches swaps in the next minibatch's)
    state = dict(hx=None, hg=None)
    sender.trace = dict(alpha=[], x_attn=[], h_x=[])

    def reset_state():                                                    # model.py:99-112
        state["hx"] = state["hg"] = None
        sender.attn_scores = []
        sender.trace = dict(alpha=[], x_attn=[], h_x=[])

    def forward(x_unused, w, g_unused, t):
        self = sender
        dt = self.attn_W_x.weight.dtype
        x, g = self.vattn_inputs[0].to(dt), self.vattn_inputs[1]
        batch_size, channels, height, width = x.size()                    # model.py:169-172
        n_feats = height * width
        if transposed:
            x = x.contiguous().view(batch_size, n_feats, channels)
        else:
            x = x.view(batch_size, channels, n_feats).transpose(1, 2)
        h_w_attn = self.attn_W_w(w)                                       # model.py:117-121
        h_w_flat = h_w_attn.unsqueeze(1).expand(batch_size, n_feats, attn_dim).contiguous().view(batch_size * n_feats, attn_dim)
        if state["hx"] is None:                                           # model.py:123-125
            state["hx"] = self.attn_W_x(x.contiguous().view(batch_size * n_feats, channels))
        if self.attn_extra_context:                                       # model.py:127-138
            if state["hg"] is None:
                h_g = self.attn_W_g(g.to(dt))
                state["hg"] = h_g.unsqueeze(1).expand(batch_size, n_feats, attn_dim).contiguous().view(batch_size * n_feats, attn_dim)
            inp = torch.tanh(h_w_flat + state["hx"] + state["hg"])
        else:
            inp = torch.tanh(h_w_flat + state["hx"])
        scores_flat = self.attn_U(inp)                                    # model.py:140
        if t == 0:                                                        # model.py:177-183
            attn = torch.ones(batch_size, n_feats, dtype=dt) / n_feats
        else:
            attn = F.softmax(scores_flat.view(batch_size, n_feats), dim=1)
        x_attn = torch.bmm(attn.unsqueeze(1), x).squeeze(1)               # model.py:186
        self.attn_scores.append(attn)                                     # model.py:189
        out = plain_forward(x_attn, w, None, t)                           # model.py:195-238 (the oracle's: h_x = image_layer(x_attn))
        self.trace["alpha"].append(attn.detach().clone()); self.trace["x_attn"].append(x_attn.detach().clone())
        self.trace["h_x"].append(self.h_x.detach().clone())
        return out
    sender.forward, sender.reset_state = forward, reset_state
    reset_state()
    return sender


def build(m, rng=None, seed=None, transposed=False, i=0):
    """The oracle's four agents under the flags of `m`, the sender attending over feature_map(m, i), with the seeded weights:
    cpu_ref.load_filled's for the reference's tensors (loaded BEFORE the attention layers exist: it loads strictly), fill_vattn's
    for the others."""
    fl = common.flags_from_meta(m)
    models = cpu_ref.build_agents(fl, rng=rng)
    cpu_ref.load_filled(models, seed=m["seed_weights"] if seed is None else seed)
    x, g = feature_map(m, i)
    attention_sender(models["sender"], m["vattn_dim"], m["context_dim"], torch.from_numpy(x), None if g is None else torch.from_numpy(g),
                     transposed=transposed)
    sd = models["sender"].state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_vattn(m, seed=seed).items()})
    models["sender"].load_state_dict(sd)
    return models, fl


def state_dicts(m, seed=None):
    """{agent: {name: ndarray}} of the seeded weights of `m`, the attention tensors included (what an engine loads)."""
    models, _ = build(m, seed=seed)
    return {a: {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()} for a, mod in models.items()}


def _inputs(m, i=0):
    _, target, desc, _ = common.case_inputs(m, i)
    stand_in = torch.zeros(m["batch"], m["img_feat_dim"])                 # (the wrapped sender reads the map of its closure)
    return stand_in, torch.from_numpy(target), torch.from_numpy(desc)


def conversation(m, train, uniforms=None, seed=None, transposed=False, map_i=0):
    """Every step of every sample (what the GPU's run-all pass stores) of minibatch 0 of `m`: the exchange's outputs plus the
    sender's attention weights alpha [T, B, N], x_attn [T, B, C] and the per-step h_x [T, B, H]."""
    tape = cpu_ref.UniformTape(*uniforms) if uniforms is not None else None
    models, fl = build(m, rng=tape, seed=seed, transposed=transposed, i=map_i)     # (map_i: another map and context, same target / desc)
    x, target, desc = _inputs(m)
    sen = models["sender"]
    args = dict(data=x, target=target, desc=desc, train=train, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, bs, br = cpu_ref.exchange(sen, models["receiver"], models["baseline_sen"], models["baseline_rec"], args, fl)
    st = lambda v: torch.stack(v).numpy()
    out = dict(s=st(s[1]), ps=st(s[2]), z=st(sen_w[0]), w=st(rec_w[0]), y=st(y), alpha=st(sen.trace["alpha"]),
               x_attn=st(sen.trace["x_attn"]), h_x=st(sen.trace["h_x"]), mask=np.stack([v.numpy() for v in s[0]]))
    if fl.use_binary:
        out.update(pz=st(sen_w[1]), pw=st(rec_w[1]))
        if train:
            out.update(bs=st(bs), br=st(br))
    return out


def eval_case(m, seed=None):
    """cpu_ref.eval_batch of minibatch 0 of `m`, packed as tests/golden/make_golden_visual_attn.py packs the reference's."""
    models, fl = build(m, seed=seed)
    x, target, desc = _inputs(m)
    res = cpu_ref.eval_batch(models, x, target, desc, fl)
    out = {"eval.n_steps": np.int64(res["n_steps"]), "eval.s_masks": cpu_ref._stack(res["s_masks"]).astype(np.uint8)}
    for k in ("s_feats", "s_probs", "sen_feats", "sen_probs", "rec_feats", "rec_probs", "y"):
        out["eval." + k] = cpu_ref._stack(res[k]).astype(np.float32)
    out["eval.outp"], out["eval.dist"] = res["outp"].numpy(), res["dist"].numpy()
    out["eval.hits"] = np.int64(res["hits"])
    n = int(res["n_steps"])
    tr = models["sender"].trace
    out["eval.alpha"] = torch.stack(tr["alpha"][:n]).numpy()
    out["eval.x_attn"] = torch.stack(tr["x_attn"][:n]).numpy()
    return out


def separated_uniforms(m, margin=1e-4):
    """tests/sender_variant_ref.separated_uniforms' method for the attention sender: the seeded uniforms of minibatch 0 with every
    draw within `margin` of its probability moved to p -/+ margin on the side it was on (bits, trajectory and every later
    probability stay; what goes is the coin two correct fp32 implementations toss on a near-tie)."""
    _, _, _, us = common.case_inputs(m, 0)
    us = [np.array(u, copy=True) for u in us]
    tp = conversation(m, train=True, uniforms=us)
    keys = ("pz", "ps", "pw") if m["use_binary"] else (None, "ps", None)
    for key, u in zip(keys, us):
        if key is None:
            continue
        p = np.asarray(tp[key], dtype=np.float64)
        v = u.reshape(p.shape)                                            # a view: edits land in u
        close = np.abs(v - p) < margin
        v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
        np.clip(v, 0.0, 0.99999994, out=v)
    return tuple(us)


def forward_f64(sd, x, g, w, t):
    """One sender step up to h_x in float64 numpy, from the formulas alone: sd the sender's state dict (arrays), x [B, C, h, w],
    g [B, G] or None, w [B, W] the receiver's last message.  Returns (alpha [B, N], x_attn [B, C], h_x [B, H])."""
    f = lambda k: np.asarray(sd[k], np.float64)
    B, C = x.shape[:2]
    X = np.asarray(x, np.float64).reshape(B, C, -1)                       # X[b, c, i]: channel-major
    N = X.shape[2]
    if t == 0:
        alpha = np.full((B, N), 1.0 / N)
    else:
        q = np.asarray(w, np.float64) @ f("attn_W_w.weight").T + f("attn_W_w.bias")
        hx = np.einsum("bci,ac->bia", X, f("attn_W_x.weight")) + f("attn_W_x.bias")
        pre = q[:, None, :] + hx
        if "attn_W_g.weight" in sd and g is not None:
            pre = pre + (np.asarray(g, np.float64) @ f("attn_W_g.weight").T + f("attn_W_g.bias"))[:, None, :]
        beta = np.tanh(pre) @ f("attn_U.weight")[0] + f("attn_U.bias")[0]
        e = np.exp(beta - beta.max(1, keepdims=True))
        alpha = e / e.sum(1, keepdims=True)
    x_attn = np.einsum("bi,bci->bc", alpha, X)
    h_x = x_attn @ f("image_layer.weight").T + f("image_layer.bias")
    return alpha, x_attn, h_x


def train_minibatches(m, uniforms_list, update=True):
    """cpu_ref.train_minibatch of minibatches 0 .. len(uniforms_list) - 1 of `m` on ONE set of agents and optimizers (minibatch i:
    the map and context of feature_map(m, i), target and desc of common.case_inputs(m, i)).  Returns ([res per minibatch], models);
    res["grads"][agent][name] are the gradients autograd left, attn_U.bias's rounding noise included."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms_list[0])
    models, fl = build(m, rng=tape)
    optimizers = cpu_ref.build_optimizers(models, fl)
    out = []
    for i, u in enumerate(uniforms_list):
        if i:
            x, g = feature_map(m, i)
            models["sender"].vattn_inputs = [torch.from_numpy(x), None if g is None else torch.from_numpy(g)]
            tape.__init__(*u)
        stand_in, target, desc = _inputs(m, i)
        out.append(cpu_ref.train_minibatch(models, optimizers, stand_in, target, desc, fl, update=update))
    return out, models


def backward_f64(sd, x, g, w, t, dh_x):
    """The reverse pass through one sender step's attention, written out by hand in float64 numpy from the formulas of the kernels:
    given dL/dh_x [B, H] it returns the gradients of image_layer and of the attention tensors (attn_U.bias: exact zeros).
    tests/test_visual_attn_cpu.py holds it against torch autograd over the literal statement (autograd_f64): they agree to 1e-12
    relative to the largest entry of each tensor."""
    f = lambda k: np.asarray(sd[k], np.float64)
    B, C = x.shape[:2]
    X = np.asarray(x, np.float64).reshape(B, C, -1)
    N = X.shape[2]
    dh = np.asarray(dh_x, np.float64)
    alpha, x_attn, _ = forward_f64(sd, x, g, w, t)
    out = {"image_layer.weight": dh.T @ x_attn, "image_layer.bias": dh.sum(0)}
    ctx = "attn_W_g.weight" in sd and g is not None
    names = VATTN_NAMES + (VATTN_CTX_NAMES if ctx else ())
    for k in names:
        out[k] = np.zeros_like(f(k))
    if t == 0:
        return out
    dxa = dh @ f("image_layer.weight")                                    # [B, C]
    dalpha = np.einsum("bci,bc->bi", X, dxa)
    dbeta = alpha * (dalpha - (alpha * dalpha).sum(1, keepdims=True))
    wv = np.asarray(w, np.float64)
    pre = (wv @ f("attn_W_w.weight").T + f("attn_W_w.bias"))[:, None, :] + np.einsum("bci,ac->bia", X, f("attn_W_x.weight")) + f("attn_W_x.bias")
    if ctx:
        gv = np.asarray(g, np.float64)
        pre = pre + (gv @ f("attn_W_g.weight").T + f("attn_W_g.bias"))[:, None, :]
    th = np.tanh(pre)
    u = dbeta[:, :, None] * f("attn_U.weight")[0] * (1.0 - th * th)       # [B, N, A]
    dq = u.sum(1)                                                         # [B, A]
    out["attn_U.weight"] = np.einsum("bi,bia->a", dbeta, th)[None, :]
    out["attn_W_w.weight"] = dq.T @ wv
    out["attn_W_x.weight"] = np.einsum("bia,bci->ac", u, X)
    out["attn_W_x.bias"] = out["attn_W_w.bias"] = dq.sum(0)
    if ctx:
        out["attn_W_g.weight"], out["attn_W_g.bias"] = dq.T @ gv, dq.sum(0)
    return out


def autograd_f64(sd, x, g, w, t, dh_x):
    """torch autograd in float64 over the literal statement of the step (model.py:114-142, 168-195), loss = sum(h_x * dh_x)."""
    P = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items() if k.startswith(("attn_", "image_layer"))}
    B, C = x.shape[:2]
    X = torch.tensor(np.asarray(x, np.float64)).view(B, C, -1).transpose(1, 2)          # [B, N, C]
    N = X.size(1)
    h = F.linear(torch.tensor(np.asarray(w, np.float64)), P["attn_W_w.weight"], P["attn_W_w.bias"]).unsqueeze(1) \
        + F.linear(X, P["attn_W_x.weight"], P["attn_W_x.bias"])
    if "attn_W_g.weight" in P and g is not None:
        h = h + F.linear(torch.tensor(np.asarray(g, np.float64)), P["attn_W_g.weight"], P["attn_W_g.bias"]).unsqueeze(1)
    beta = F.linear(torch.tanh(h), P["attn_U.weight"], P["attn_U.bias"]).squeeze(2)
    attn = torch.full((B, N), 1.0 / N, dtype=torch.float64) if t == 0 else F.softmax(beta, dim=1)
    h_x = F.linear(torch.bmm(attn.unsqueeze(1), X).squeeze(1), P["image_layer.weight"], P["image_layer.bias"])
    (h_x * torch.tensor(np.asarray(dh_x, np.float64))).sum().backward()
    return {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items()}
