"""Test-side reference of the sender's communication ablations (-sender_mix prod / -ignore_code / -ignore_receiver, model.py:217-218,
208-210, 470-472): the CPU oracle (oracle/cpu_ref) with the Sender's forward replaced by a restatement of model.py:195-221 for the
three cases, and cpu_ref.Flags(ignore_receiver=True), which the oracle's Receiver already implements.  The oracle itself is not
edited: the wrapper sits on the forward method of the sender it is handed (the pattern of tests/flipout_ref.py).

A setting is a tuple (mix, ignore_code, ignore_receiver), mix "sum" or "prod"."""
import numpy as np
import torch

from oracle import cpu_ref
from tests import common

SUM = ("sum", False, False)
SETTINGS = {"prod": ("prod", False, False), "ignore_code": ("sum", True, False), "ignore_receiver": ("sum", False, True),
            "prod_ignore_receiver": ("prod", False, True)}


# The shapes of tests/test_sender_variant_gpu.py (their reach conditions: tests/test_sender_variant_cpu.py).  A: config 1's agents,
# RMSprop.  B: small dimensions that are no multiple of the workgroup size or of a 16-wide tile -- the strided loops' tails --, Adam.
_C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=16, learning_rate=1e-4, entropy_rec=0.01,
           entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
           rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)
SHAPES = {"A": (_C1, 30, 16),
          "B": (dict(_C1, max_exchange=3, batch_size=5, img_feat_dim=18, img_h_dim=40, rec_w_dim=12, sender_out_dim=12, rec_hidden=20,
                     wv_dim=12, baseline_hid_dim=70, optim_type="Adam", top_k_train=2, top_k_dev=2), 7, 5)}
# data seeds of the evaluation comparison on shape A, per setting: the oracle's conversation has no probability within 1e-4 of 0.5
EVAL_DATA_SEED = {"ignore_code": 8, "ignore_receiver": 22, "prod": 254, "prod_ignore_receiver": 274}


def meta(shape, **over):
    """The meta dict (tests/common.py: flags_from_meta, case_inputs) of a shape: weights seed 5, data seed 6, uniforms seed 7."""
    flags, n_classes, batch = SHAPES[shape]
    m = dict(cpu_ref.Flags(**flags).__dict__)
    m.update(n_classes=n_classes, batch=batch, n_minibatches=1, seed_weights=5, seed_data=6, seed_uniforms=7)
    m.update(over)
    return m


def variant_sender(sender, mix, ignore_code):
    """sender.forward becomes model.py:195-238 with FLAGS.sender_mix = mix and FLAGS.ignore_code = ignore_code."""
    assert mix in ("sum", "prod")

    def forward(x, w, g, t):
        self = sender
        self.h_x = h_x = self.image_layer(x)                          # model.py:195
        if t == 0:                                                    # model.py:196-200
            first_code = torch.sigmoid(self.code_bias.view(1, -1))
            h_w = self.code_layer(first_code).expand(x.size(0), self.h_dim)
        else:
            h_w = self.code_layer(w)                                  # model.py:207
        if ignore_code:
            features = self.binary_layer(torch.tanh(h_x))             # model.py:208-210 (h_w is computed and dropped)
        elif mix == "sum":
            features = self.binary_layer(torch.tanh(h_x + h_w))       # model.py:216
        else:
            features = self.binary_layer(torch.tanh(h_x * h_w))       # model.py:218
        if self.use_binary:
            probs = torch.sigmoid(features)                           # model.py:223
            if self.training:                                         # model.py:224-227
                probs_ = probs.detach().cpu().numpy()
                binary = torch.from_numpy((self.rng.rand("z", *probs_.shape) < probs_).astype(probs_.dtype))
            else:
                binary = torch.round(probs).detach()                  # model.py:229
            return binary, probs
        return features, None                                         # model.py:238
    sender.forward = forward
    return sender


def flags_of(meta, setting):
    fl = common.flags_from_meta(meta)
    fl.ignore_receiver = bool(setting[2])
    return fl


def build(meta, setting, rng=None):
    """The oracle's four agents with the seeded weights of `meta` under `setting`."""
    fl = flags_of(meta, setting)
    models = cpu_ref.build_agents(fl, rng=rng)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    variant_sender(models["sender"], setting[0], setting[1])
    return models, fl


def _inputs(meta):
    x, target, desc, _ = common.case_inputs(meta, 0)
    return torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc)


def conversation(meta, setting, train, uniforms=None):
    """Every step of every sample (what the GPU's run-all pass stores) of minibatch 0 of `meta` under `setting`."""
    tape = cpu_ref.UniformTape(*uniforms) if uniforms is not None else None
    models, fl = build(meta, setting, rng=tape)
    x, target, desc = _inputs(meta)
    args = dict(data=x, target=target, desc=desc, train=train, break_early=False)
    hidden = []                                                       # the sender's hidden layer a_t: what binary_layer is handed
    hook = models["sender"].binary_layer.register_forward_pre_hook(lambda mod, inp: hidden.append(inp[0].detach().clone()))
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], models["baseline_sen"], models["baseline_rec"], args, fl)
    hook.remove()
    st = lambda v: torch.stack(v).numpy()
    return dict(s=st(s[1]), ps=st(s[2]), z=st(sen_w[0]), pz=st(sen_w[1]), w=st(rec_w[0]), pw=st(rec_w[1]), y=st(y), a=st(hidden))


def eval_case(meta, setting):
    """cpu_ref.eval_batch of minibatch 0 of `meta` under `setting`, packed as tests/golden/make_golden_sender_variants.py packs the
    reference's evaluation conversation."""
    models, fl = build(meta, setting)
    x, target, desc = _inputs(meta)
    res = cpu_ref.eval_batch(models, x, target, desc, fl)
    out = {"eval.n_steps": np.int64(res["n_steps"]), "eval.s_masks": cpu_ref._stack(res["s_masks"]).astype(np.uint8)}
    for k in ("s_feats", "s_probs", "sen_feats", "sen_probs", "rec_feats", "rec_probs", "y"):
        out["eval." + k] = cpu_ref._stack(res[k]).astype(np.float32)
    out["eval.outp"], out["eval.dist"] = res["outp"].numpy(), res["dist"].numpy()
    out["eval.hits"] = np.int64(res["hits"])
    return out


def train_minibatch(meta, setting, uniforms, update=True, y2_bias=None):
    """cpu_ref.train_minibatch of minibatch 0 of `meta` under `setting`, packed as common.oracle_train_case packs it (y2_bias: as
    there -- the value the receiver's y2.bias takes after the update, whose own step is rounding noise).  Returns (packed, res,
    models): under ignore_code the models' code_layer / code_bias .grad stay None."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms)
    models, fl = build(meta, setting, rng=tape)
    optimizers = cpu_ref.build_optimizers(models, fl)
    x, target, desc = _inputs(meta)
    res = cpu_ref.train_minibatch(models, optimizers, x, target, desc, fl, update=update)
    if y2_bias is not None:
        with torch.no_grad():
            models["receiver"].y2.bias.copy_(torch.as_tensor(np.asarray(y2_bias, np.float32)).view_as(models["receiver"].y2.bias))
    return cpu_ref.pack_train(res, models, prefix="mb0."), res, models


def separated_uniforms(meta, setting, margin=1e-4):
    """common.separate_draws restated for the wrapped sender: the seeded uniforms of minibatch 0 with every draw that lies within
    `margin` of its probability moved to p -/+ margin on the side it was on -- the sampled bits, hence the trajectory and every
    later probability, stay what they were; what goes is the coin two correct fp32 implementations toss on a near-tie.  The
    conversation runs all steps here (break_early off), so that the run-all pass of the GPU is covered too."""
    _, _, _, us = common.case_inputs(meta, 0)
    us = [np.array(u, copy=True) for u in us]
    tp = conversation(meta, setting, train=True, uniforms=us)
    for key, u in zip(("pz", "ps", "pw"), us):
        p = np.asarray(tp[key], dtype=np.float64)
        v = u.reshape(p.shape)                                        # a view: edits land in u
        close = np.abs(v - p) < margin
        v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
        np.clip(v, 0.0, 0.99999994, out=v)
    return tuple(us)
