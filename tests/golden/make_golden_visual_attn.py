#!/usr/bin/env python
"""Generate the g13 fixtures of visual attention (-visual_attn -attn_dim 256 -attn_extra_context -attn_context_dim 1000) by running
the REFERENCE's own code.

Same rules as tests/golden/make_golden.py, whose loader, substitutions and harness this reuses: run in the build container only,
the reference is read and executed in memory, and only NUMBERS are written out.  Two more semantics-restoring substitutions, both
`len`-truthiness restorations for lines only the attention branch runs (the cached attn_W_x(X) / attn_W_g(g) are tensors now:
`not tensor` raises for more than one element): `if not self.h_x_attn_flat:` and `if not self.h_g_flat:` become `is None` tests.
make_golden.set_flags hard-sets visual_attn = False and build_ref_models builds a plain sender; both are overridden here for the
duration of a case (the pattern of make_golden_desc_attn.py), exchange() gets the 4-D map in place of the harness's [B, C] features
plus exchange_args["data_context"] (what run() sets at model.py:1231-1232), and the attention tensors come from
tests/visual_attn_ref.fill_vattn.  Inputs are regenerated from seeds by the tests (tests/visual_attn_ref.feature_map).

  g13_visual_attn_<mode>        config-1 agents (H 256, W 32, R 64, V 100, K 500), a 512 x 8 x 8 map, A = 256, a 1000-d context,
                                30 classes, 16 samples, 4 steps; modes: adaptive, fixed, continuous (-nouse_binary).  One training
                                minibatch (keys mb0.*, packed as make_golden.run_train_case packs it) plus the sender's per-step
                                attention weights mb0.alpha [T, B, N] and mb0.x_attn [T, B, C / 8] (every sample, every 8th channel)
  g13_visual_attn_<mode>_eval   one evaluation conversation of the same agents on the same inputs (keys eval.*, with eval.alpha and
                                eval.x_attn, the latter every 8th channel of every sample) -- a file of its own, so that each stays within the size of the g12 fixtures

usage: python tests/golden/make_golden_visual_attn.py --ref REFERENCE_DIR [--out tests/golden]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets oracle.PORTABLE_FP_ENV before torch loads)
from make_golden_desc_attn import pack_scalars  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import cpu_ref  # noqa: E402
from tests import visual_attn_ref as var  # noqa: E402

XA_STRIDE = 8
SEEDS = dict(weights=5, data=var.DATA_SEED["A"], uniforms=7)         # tests/test_visual_attn_cpu.py checks what these seeds reach


def load_reference(ref_dir):
    plain = mg._sub
    pairs = (("if not self.h_x_attn_flat:", "if self.h_x_attn_flat is None:"), ("if not self.h_g_flat:", "if self.h_g_flat is None:"))

    def _sub(src, old, new, count=1):
        src = plain(src, old, new, count)
        for a, b in pairs:
            if a in src:
                src = plain(src, a, b)
        return src
    mg._sub = _sub
    try:
        return mg.load_reference(ref_dir)
    finally:
        mg._sub = plain


def flags_for(meta):
    return mg.make_flags(**{k: v for k, v in meta.items() if k in cpu_ref.Flags().__dict__})


class attention(object):
    """For the duration of a case: the attention flags behind set_flags, an attention sender out of build_ref_models, the map and
    the context in every exchange() call, a weight filler that knows the attention tensors, and hooks that record what the
    reference's sender computes per step (x_attn is image_layer's input, h_x its output; alpha is sender.attn_scores)."""

    def __init__(self, ref, meta):
        self.ref, self.meta = ref, meta
        x, g = var.feature_map(meta)
        self.x, self.g = torch.from_numpy(x), None if g is None else torch.from_numpy(g)
        self.x_attn, self.h_x, self.sender = [], [], None

    def __enter__(self):
        ref, meta = self.ref, self.meta
        self.saved = (mg.set_flags, mg.build_ref_models, ref.exchange, cpu_ref.load_filled)
        plain_flags, _, plain_exchange, _ = self.saved

        def set_flags(FLAGS, fl):
            plain_flags(FLAGS, fl)
            FLAGS.visual_attn, FLAGS.attn_dim = True, meta["vattn_dim"]
            FLAGS.attn_extra_context, FLAGS.attn_context_dim = meta["context_dim"] > 0, max(meta["context_dim"], 1)

        def build_ref_models(ref_, FLAGS):
            models = self.saved[1](ref_, FLAGS)
            models["sender"] = ref_.Sender(feature_type=FLAGS.img_feat, feat_dim=FLAGS.img_feat_dim, h_dim=FLAGS.img_h_dim,
                                           w_dim=FLAGS.rec_w_dim, bin_dim_out=FLAGS.sender_out_dim, use_binary=FLAGS.use_binary,
                                           use_attn=True, attn_dim=FLAGS.attn_dim, attn_extra_context=FLAGS.attn_extra_context,
                                           attn_context_dim=FLAGS.attn_context_dim)                  # model.py:1014-1023
            self.sender = models["sender"]
            self.sender.image_layer.register_forward_hook(
                lambda mod, inp, out: (self.x_attn.append(inp[0].detach().clone()), self.h_x.append(out.detach().clone())) and None)
            return models

        def exchange(sender, receiver, baseline_sen, baseline_rec, exchange_args):
            args = dict(exchange_args, data=self.x)
            if self.g is not None:
                args["data_context"] = self.g                                                        # model.py:1231-1232
            del self.x_attn[:], self.h_x[:]
            return plain_exchange(sender, receiver, baseline_sen, baseline_rec, args)

        def load_filled(models, seed=0, bias_scale=0.05):
            shapes = {a: {k: tuple(v.shape) for k, v in m.state_dict().items()} for a, m in models.items()}
            filled = cpu_ref.fill_state_dicts(shapes, seed, bias_scale)
            filled["sender"].update(var.fill_vattn(meta, seed=seed))
            for a, m in models.items():
                m.load_state_dict({k: torch.from_numpy(v) for k, v in filled[a].items()})
            return filled
        mg.set_flags, mg.build_ref_models, ref.exchange, cpu_ref.load_filled = set_flags, build_ref_models, exchange, load_filled
        return self

    def __exit__(self, *exc):
        mg.set_flags, mg.build_ref_models, self.ref.exchange, cpu_ref.load_filled = self.saved

    def trace(self, prefix, n):
        st = lambda v: torch.stack([t.detach() for t in v[:n]]).numpy().astype(np.float32)
        # (x_attn of EVERY sample and step, every XA_STRIDE-th channel; h_x not at all: in full they alone would be larger than a whole
        #  g12 fixture; tests/test_visual_attn_cpu.py holds the wrapped oracle, which keeps all of them, against these)
        return {prefix + "alpha": st(self.sender.attn_scores), prefix + "x_attn": np.ascontiguousarray(st(self.x_attn)[:, :, ::XA_STRIDE])}


def ref_eval(ref, FLAGS, fl, meta, att):
    """The per-batch body of eval_dev (model.py:620-668) on the seeded weights and minibatch 0's inputs."""
    models = mg.build_ref_models(ref, FLAGS)
    cpu_ref.load_filled(models, seed=SEEDS["weights"])
    x, target, desc = cpu_ref.synthetic_batch(meta["batch"], meta["n_classes"], fl.img_feat_dim, fl.wv_dim, seed=SEEDS["data"])
    exchange_args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc),
                         train=False, break_early=not fl.fixed_exchange, corrupt=False, corrupt_region=None)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = ref.exchange(models["sender"], models["receiver"], None, None, exchange_args)
        s_masks, s_feats, s_probs = s
        y_masks = None if fl.fixed_exchange else [torch.min(1 - m1, m2) for m1, m2 in zip(s_masks[1:], s_masks[:-1])]
        outp, _ = ref.get_rec_outp(y, y_masks)
        dist = F.log_softmax(outp, dim=1)
    top_k_ind = dist.numpy().argsort()[:, -fl.top_k_dev:]                     # model.py:658
    out = {"eval.n_steps": np.int64(len(y)), "eval.s_masks": mg._stack(s_masks).astype(np.uint8)}
    for k, v in (("s_feats", s_feats), ("s_probs", s_probs), ("sen_feats", sen_w[0]), ("sen_probs", sen_w[1]),
                 ("rec_feats", rec_w[0]), ("rec_probs", rec_w[1]), ("y", y)):
        out["eval." + k] = mg._stack(v).astype(np.float32)
    out["eval.outp"], out["eval.dist"] = outp.numpy(), dist.numpy()
    out["eval.hits"] = np.int64((top_k_ind == target.reshape(-1, 1)).sum())
    tr = att.trace("eval.", len(y))
    out["eval.alpha"], out["eval.x_attn"] = tr["eval.alpha"], tr["eval.x_attn"]
    return out


def case(ref, FLAGS, mode):
    meta = var.meta("A", mode)
    fl = flags_for(meta)
    with attention(ref, meta) as att:
        train = mg.run_train_case(ref, FLAGS, fl, meta["n_classes"], meta["batch"], SEEDS, n_minibatches=1)
        train.update(att.trace("mb0.", int(train["mb0.n_steps"])))
        mg.set_flags(FLAGS, fl)
        evaluation = ref_eval(ref, FLAGS, fl, meta, att)
    train["meta"] = evaluation["meta"] = np.array(json.dumps(meta))
    return train, evaluation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref, FLAGS = load_reference(args.ref)
    for mode in var.MODES:
        for suffix, d in zip(("", "_eval"), case(ref, FLAGS, mode)):
            path = os.path.join(args.out, "g13_visual_attn_%s%s.npz" % (mode, suffix))
            np.savez_compressed(path, **pack_scalars(d))
            print("%-44s %7.1f KB  %d arrays" % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(d)))


if __name__ == "__main__":
    main()
