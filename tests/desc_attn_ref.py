"""Test-side reference of description attention (-desc_attn, model.py:267-271, 344-410, 444-445): the CPU oracle (oracle/cpu_ref)
with three more layers on its Receiver and the Receiver's forward replaced by a restatement of the reference's attention branch.
The oracle itself is not edited: the wrapper sits on the receiver it is handed (the pattern of tests/sender_variant_ref.py), which
keeps the description set and the segment lengths in its closure -- cpu_ref.exchange hands the receiver None for both.

cpu_ref.fill_state_dicts only knows the reference's fifteen receiver tensors; fill_attn is the seeded filler of the other six."""
import json
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cpu_ref
from tests import common

ATTN_NAMES = ("d_d.weight", "d_d.bias", "d_h.weight", "d_h.bias", "d_attn.weight", "d_attn.bias")

# The shapes of tests/test_desc_attn_gpu.py (their reach conditions: tests/test_desc_attn_cpu.py).
#   A: config 1's agents, 16 samples, 4 steps, A = 64, 30 classes over 300 words -- more words than a workgroup has threads; one class
#      of ONE word (its alpha is 1 and carries no gradient), one of 70 (a segment longer than a wave), one word row all zeros.
#   B: small dimensions that are no multiple of the workgroup size, of a wave or of a 16-wide tile -- the strided loops' tails --, Adam.
_C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=16, learning_rate=1e-4, entropy_rec=0.01,
           entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
           rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)
LENS_A = [9, 1, 8, 8, 70] + [9] * 4 + [8] * 21
LENS_B = [1, 3, 2, 5, 1, 4, 2]
ZERO_ROW = {"A": 40, "B": 7}            # a word without a GloVe vector: inside the 70-word class (A), inside the 5-word class (B)
SHAPES = {"A": (_C1, LENS_A, 16, 64),
          "B": (dict(_C1, max_exchange=3, batch_size=5, img_feat_dim=18, img_h_dim=40, rec_w_dim=12, sender_out_dim=12, rec_hidden=20,
                     wv_dim=12, baseline_hid_dim=70, optim_type="Adam", top_k_train=2, top_k_dev=2), LENS_B, 5, 10)}
assert sum(LENS_A) == 300 and len(LENS_A) == 30 and min(LENS_A) == 1 and max(LENS_A) == 70
MODES = {"adaptive": dict(use_binary=True, fixed_exchange=False), "fixed": dict(use_binary=True, fixed_exchange=True),
         "continuous": dict(use_binary=False, fixed_exchange=True)}


# Seeds searched on the CPU oracle (tests/test_desc_attn_cpu.py asserts what they reach).  Training minibatch, per (shape, mode): the
# data seed with which no relu pre-activation of the output step lies within 1e-5 of 0 (shape A has 30 720 of them per minibatch) and,
# in Adaptive mode, samples stop early, run to the last step and have t* >= 1.  Evaluation: the data seed with which no probability of
# the conversation lies within 1e-4 of 0.5 (the description set is drawn from the data seed too), for the seeded weights and for the
# second set the stale-tables test loads (SECOND_WEIGHTS).
TRAIN_DATA_SEED = {("A", "adaptive"): 7, ("A", "fixed"): 14, ("A", "continuous"): 19,
                   ("B", "adaptive"): 6, ("B", "fixed"): 6, ("B", "continuous"): 6}
EVAL_DATA_SEED = {"A": 7, "B": 6}
SECOND_WEIGHTS = 11
SECOND_EVAL_DATA_SEED = {"A": 50, "B": 6}


def train_meta(shape, mode):
    return meta(shape, mode, seed_data=TRAIN_DATA_SEED[shape, mode])


def load_golden(name):
    """A g12 fixture as (dict of arrays, meta): common.load_golden with the float64 scalars unpacked again
    (tests/golden/make_golden_desc_attn.py: pack_scalars keeps them as one vector)."""
    z, m = common.load_golden(name)
    out = {k: z[k] for k in z.files if k not in ("scalars", "scalar_keys")}
    out.update({k: np.float64(v) for k, v in zip(json.loads(str(z["scalar_keys"])), z["scalars"])})
    return out, m


def meta(shape, mode="adaptive", **over):
    """The meta dict (tests/common.py: flags_from_meta, case_inputs) of a shape: weights seed 5, data seed 6, uniforms seed 7."""
    flags, lens, batch, attn_dim = SHAPES[shape]
    m = dict(cpu_ref.Flags(**dict(flags, **MODES[mode])).__dict__)
    m.update(n_classes=len(lens), batch=batch, n_minibatches=1, seed_weights=5, seed_data=6, seed_uniforms=7,
             desc_attn_dim=attn_dim, desc_set_lens=list(lens), shape=shape)
    m.update(over)
    return m


def desc_set(m):
    """Seeded word vectors [n_words, V] of the case (0.3 N(0, 1), as cpu_ref.synthetic_batch draws desc) with one all-zero row, and
    the lengths."""
    lens = list(m["desc_set_lens"])
    rs = np.random.RandomState(m["seed_data"] + 1000)
    s = (0.3 * rs.standard_normal((sum(lens), m["wv_dim"]))).astype(np.float32)
    s[ZERO_ROW[m["shape"]]] = 0.0
    return s, lens


def fill_attn(m, seed=None):
    """{name: float32 ndarray} of the six attention tensors: Xavier-normal 2-D tensors, N(0, 0.05) biases (cpu_ref.fill_state_dicts'
    rule), from a stream of their own so that the other tensors keep the values every other test gives them."""
    A, V, R = m["desc_attn_dim"], m["wv_dim"], m["rec_hidden"]
    shapes = {"d_d.weight": (A, V), "d_d.bias": (A,), "d_h.weight": (A, R), "d_h.bias": (A,), "d_attn.weight": (1, A), "d_attn.bias": (1,)}
    rs = np.random.RandomState((m["seed_weights"] if seed is None else seed) + 4242)
    out = {}
    for name in ATTN_NAMES:
        shape = shapes[name]
        std = math.sqrt(2.0 / (shape[0] + shape[1])) if len(shape) == 2 else 0.05
        out[name] = (rs.standard_normal(shape) * std).astype(np.float32)
    return out


def attention_receiver(receiver, attn_dim, dset, lens, swap_y1=False):
    """receiver gets d_d / d_h / d_attn (model.py:267-271) and its forward becomes model.py:333-477 with FLAGS.desc_attn on.
    swap_y1: build the y1 input as [h || description] -- the column order of build_inp, which the attention branch does NOT use."""
    receiver.attn_dim = attn_dim
    receiver.d_d = nn.Linear(receiver.desc_dim, attn_dim)
    receiver.d_h = nn.Linear(receiver.hid_dim, attn_dim)
    receiver.d_attn = nn.Linear(attn_dim, 1)
    lens = [int(v) for v in lens]

    def forward(z, desc, desc_set=None, desc_set_lens=None):
        self = receiver
        desc_set = dset.to(self.d_d.weight.dtype)
        batch_size = z.size(0)
        if self.h_z is None:                                          # model.py:336-337
            self.h_z = self.initial_state(batch_size).to(z.dtype)
        self.h_z = self.rnn(z, self.h_z)                              # model.py:340
        nwords = desc_set.size(0)
        desc_set_broadcast = desc_set.unsqueeze(0).expand(batch_size, nwords, self.desc_dim)       # model.py:348-349
        dd = self.d_d(desc_set)                                       # model.py:352
        dd_flat = dd.unsqueeze(0).expand(batch_size, nwords, self.attn_dim).contiguous().view(batch_size * nwords, self.attn_dim)
        dh = self.d_h(self.h_z)                                       # model.py:359
        dh_flat = dh.unsqueeze(1).expand(batch_size, nwords, self.attn_dim).contiguous().view(batch_size * nwords, self.attn_dim)
        d_attn = self.d_attn(torch.tanh(dd_flat + dh_flat)).view(batch_size, nwords)               # model.py:366-367
        cumlen, scores = 0, []
        for ndesc in lens:                                            # model.py:370-378
            scores.append(F.softmax(d_attn[:, cumlen:cumlen + ndesc], dim=1))
            cumlen += ndesc
        self.d_attn_scores = d_attn_scores = torch.cat(scores, 1)     # model.py:379-380
        desc_set_weighted = desc_set_broadcast * d_attn_scores.unsqueeze(2).expand_as(desc_set_broadcast)    # model.py:383-385
        cumlen, weighted_desc = 0, []
        for ndesc in lens:                                            # model.py:388-396
            weighted_desc.append(desc_set_weighted[:, cumlen:cumlen + ndesc, :].sum(1, keepdim=True))
            cumlen += ndesc
        weighted_desc = torch.cat(weighted_desc, 1)                   # model.py:397: B x D x WV
        nclasses = weighted_desc.size(1)
        weighted_desc = weighted_desc.view(batch_size * nclasses, self.desc_dim)                   # model.py:401-402
        h_z_flat = self.h_z.unsqueeze(1).expand(batch_size, nclasses, self.hid_dim).contiguous().view(batch_size * nclasses, self.hid_dim)
        parts = [h_z_flat, weighted_desc] if swap_y1 else [weighted_desc, h_z_flat]                # model.py:409-410: description FIRST
        inp_with_desc = torch.cat(parts, 1)

        s_prob = torch.sigmoid(self.s(self.h_z))                      # model.py:414-415
        if self.training:                                             # model.py:416-420
            prob_ = s_prob.detach().cpu().numpy()
            s_binary = torch.from_numpy((self.rng.rand("s", *prob_.shape) < prob_).astype(prob_.dtype))
        else:                                                         # model.py:421-427
            if self.s_prob_prod is None or not self.flags.s_prob_prod:
                self.s_prob_prod = s_prob
            else:
                self.s_prob_prod = self.s_prob_prod * s_prob
            s_binary = torch.round(self.s_prob_prod).detach()
        y = self.y1(inp_with_desc).clamp(min=0)                       # model.py:432
        y = self.y2(y).view(batch_size, -1)                           # model.py:433
        n_desc = y.size(1)
        y_scores = F.softmax(y, dim=1).detach()                       # model.py:441
        y_broadcast = y_scores.unsqueeze(2).expand(batch_size, n_desc, self.desc_dim)
        wd_inp = weighted_desc.view(batch_size, nclasses, self.desc_dim)                           # model.py:444-445
        wd_inp = (y_broadcast * wd_inp).sum(1)                        # model.py:449
        self.dbar = wd_inp.detach()
        self.h_w = torch.tanh(self.w_h(self.h_z) + self.w_d(wd_inp))  # model.py:452
        w_scores = self.w(self.h_w)                                   # model.py:454
        if self.use_binary:
            w_probs = torch.sigmoid(w_scores)                         # model.py:456
            if self.training:                                         # model.py:457-460
                probs_ = w_probs.detach().cpu().numpy()
                w_feats = torch.from_numpy((self.rng.rand("w", *probs_.shape) < probs_).astype(probs_.dtype))
            else:
                w_feats = torch.round(w_probs).detach()               # model.py:462
        else:
            w_feats, w_probs = w_scores, None                         # model.py:474-475
        return (s_binary, s_prob), (w_feats, w_probs), y
    receiver.forward = forward
    return receiver


def build(m, rng=None, swap_y1=False, seed=None):
    """The oracle's four agents under the flags of `m`, the receiver attending over desc_set(m), with the seeded weights:
    cpu_ref.load_filled's for the reference's tensors (loaded BEFORE the attention layers exist: it loads strictly), fill_attn's
    for the six.  seed: another weight seed than the meta's."""
    fl = common.flags_from_meta(m)
    models = cpu_ref.build_agents(fl, rng=rng)
    cpu_ref.load_filled(models, seed=m["seed_weights"] if seed is None else seed)
    dset, lens = desc_set(m)
    attention_receiver(models["receiver"], m["desc_attn_dim"], torch.from_numpy(dset), lens, swap_y1=swap_y1)
    sd = models["receiver"].state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_attn(m, seed=seed).items()})
    models["receiver"].load_state_dict(sd)
    return models, fl


def _inputs(m):
    x, target, desc, _ = common.case_inputs(m, 0)
    return torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc)


def conversation(m, train, uniforms=None, swap_y1=False, seed=None):
    """Every step of every sample (what the GPU's run-all pass stores) of minibatch 0 of `m`: the exchange's outputs plus the
    receiver's attention weights alpha [T, B, NW], dbar [T, B, V] and the y1 pre-activations [T, B, D, R]."""
    tape = cpu_ref.UniformTape(*uniforms) if uniforms is not None else None
    models, fl = build(m, rng=tape, swap_y1=swap_y1, seed=seed)
    x, target, desc = _inputs(m)
    rec = models["receiver"]
    alpha, dbar, pre = [], [], []
    plain = rec.forward

    def forward(*a, **k):
        out = plain(*a, **k)
        alpha.append(rec.d_attn_scores.detach().clone()); dbar.append(rec.dbar.clone())
        return out
    rec.forward = forward
    hook = rec.y1.register_forward_hook(lambda mod, inp, o: pre.append(o.detach().view(x.size(0), len(m["desc_set_lens"]), -1).clone()))
    args = dict(data=x, target=target, desc=desc, train=train, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], rec, models["baseline_sen"], models["baseline_rec"], args, fl)
    hook.remove()
    st = lambda v: torch.stack(v).numpy()
    out = dict(s=st(s[1]), ps=st(s[2]), z=st(sen_w[0]), w=st(rec_w[0]), y=st(y), alpha=st(alpha), dbar=st(dbar), pre=st(pre),
               mask=np.stack([v.numpy() for v in s[0]]))
    if fl.use_binary:
        out.update(pz=st(sen_w[1]), pw=st(rec_w[1]))
    return out


def eval_case(m, seed=None):
    """cpu_ref.eval_batch of minibatch 0 of `m`, packed as tests/golden/make_golden_desc_attn.py packs the reference's."""
    models, fl = build(m, seed=seed)
    x, target, desc = _inputs(m)
    res = cpu_ref.eval_batch(models, x, target, desc, fl)
    out = {"eval.n_steps": np.int64(res["n_steps"]), "eval.s_masks": cpu_ref._stack(res["s_masks"]).astype(np.uint8)}
    for k in ("s_feats", "s_probs", "sen_feats", "sen_probs", "rec_feats", "rec_probs", "y"):
        out["eval." + k] = cpu_ref._stack(res[k]).astype(np.float32)
    out["eval.outp"], out["eval.dist"] = res["outp"].numpy(), res["dist"].numpy()
    out["eval.hits"] = np.int64(res["hits"])
    return out


def train_minibatch(m, uniforms, update=True, y2_bias=None, swap_y1=False):
    """cpu_ref.train_minibatch of minibatch 0 of `m`, packed as common.oracle_train_case packs it.  Returns (packed, res, models)."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms)
    models, fl = build(m, rng=tape, swap_y1=swap_y1)
    optimizers = cpu_ref.build_optimizers(models, fl)
    x, target, desc = _inputs(m)
    res = cpu_ref.train_minibatch(models, optimizers, x, target, desc, fl, update=update)
    if y2_bias is not None:
        with torch.no_grad():
            models["receiver"].y2.bias.copy_(torch.as_tensor(np.asarray(y2_bias, np.float32)).view_as(models["receiver"].y2.bias))
    return cpu_ref.pack_train(res, models, prefix="mb0."), res, models


def separated_uniforms(m, margin=1e-4):
    """tests/sender_variant_ref.separated_uniforms' method for the attention receiver: the seeded uniforms of minibatch 0 with every
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
        v = u.reshape(p.shape)                                        # a view: edits land in u
        close = np.abs(v - p) < margin
        v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
        np.clip(v, 0.0, 0.99999994, out=v)
    return tuple(us)
