#!/usr/bin/env python
"""Generate the g12 fixtures of description attention (-desc_attn -desc_attn_dim 64) by running the REFERENCE's own code.

Same rules as tests/golden/make_golden.py, whose loader, substitutions and harness this reuses: run in the build container only,
the reference is read and executed in memory, and only NUMBERS are written out.  make_golden.set_flags hard-sets desc_attn = False;
it is overridden here right behind it (the pattern of make_golden_sender_variants.py).  The harness hands exchange() no description
set and its weight filler only knows the plain receiver's tensors, so both are wrapped for the duration of a case: exchange() gets
exchange_args["desc_set"] / ["desc_set_lens"] (what run() sets at model.py:1235-1236), and the six attention tensors come from
tests/desc_attn_ref.fill_attn.  The reference's attention branch runs as it stands on torch 2.10.

  g12_desc_attn_<mode>        config-1 agents (H 256, W 32, R 64, V 100, K 500), 30 classes over 300 words (tests/desc_attn_ref:
                              LENS_A, one all-zero word row), 16 samples, 4 steps; modes: adaptive, fixed, continuous (-nouse_binary).
                              One training minibatch (keys mb0.*, packed as make_golden.run_train_case packs it)
  g12_desc_attn_<mode>_eval   one evaluation conversation of the same agents on the same inputs (keys eval.*) -- a file of its own,
                              so that each stays within the size of the g11 fixtures

usage: python tests/golden/make_golden_desc_attn.py --ref REFERENCE_DIR [--out tests/golden]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets oracle.PORTABLE_FP_ENV before torch loads)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import cpu_ref  # noqa: E402
from tests import desc_attn_ref as dar  # noqa: E402

SEEDS = dict(weights=5, data=6, uniforms=7)          # tests/test_desc_attn_cpu.py checks what these seeds reach


def load_reference(ref_dir):
    """make_golden.load_reference with one more semantics-restoring substitution, for a line only the attention branch runs:
    PyTorch 0.1.12's sum(1) keeps the dimension (model.py:395 comments the result as B x 1 x WV, and model.py:397 concatenates the
    classes along it) -- the same restoration make_golden applies to model.py:911."""
    plain = mg._sub
    line = "cbow = desc_set_weighted[:, start:end, :].sum(1)"

    def _sub(src, old, new, count=1):
        src = plain(src, old, new, count)
        return plain(src, line, line[:-1] + ", keepdim=True)") if line in src else src
    mg._sub = _sub
    try:
        return mg.load_reference(ref_dir)
    finally:
        mg._sub = plain


def flags_for(meta):
    return mg.make_flags(**{k: v for k, v in meta.items() if k in cpu_ref.Flags().__dict__})


class attention(object):
    """For the duration of a case: FLAGS.desc_attn behind set_flags, the description set in every exchange() call, and a weight
    filler that knows the six attention tensors."""

    def __init__(self, ref, meta):
        self.ref, self.meta = ref, meta
        dset, self.lens = dar.desc_set(meta)
        self.dset = torch.from_numpy(dset)

    def __enter__(self):
        ref, meta = self.ref, self.meta
        self.saved = (mg.set_flags, ref.exchange, cpu_ref.load_filled)
        plain_flags, plain_exchange, plain_filled = self.saved

        def set_flags(FLAGS, fl):
            plain_flags(FLAGS, fl)
            FLAGS.desc_attn, FLAGS.desc_attn_dim = True, meta["desc_attn_dim"]

        def exchange(sender, receiver, baseline_sen, baseline_rec, exchange_args):
            return plain_exchange(sender, receiver, baseline_sen, baseline_rec,
                                  dict(exchange_args, desc_set=self.dset, desc_set_lens=self.lens))     # model.py:1235-1236

        def load_filled(models, seed=0, bias_scale=0.05):
            shapes = {a: {k: tuple(v.shape) for k, v in m.state_dict().items()} for a, m in models.items()}
            filled = cpu_ref.fill_state_dicts(shapes, seed, bias_scale)
            filled["receiver"].update(dar.fill_attn(meta, seed=seed))
            for a, m in models.items():
                m.load_state_dict({k: torch.from_numpy(v) for k, v in filled[a].items()})
            return filled
        mg.set_flags, ref.exchange, cpu_ref.load_filled = set_flags, exchange, load_filled
        return self

    def __exit__(self, *exc):
        mg.set_flags, self.ref.exchange, cpu_ref.load_filled = self.saved


def ref_eval(ref, FLAGS, fl, meta):
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
    return out


def case(ref, FLAGS, mode):
    meta = dar.meta("A", mode)
    fl = flags_for(meta)
    with attention(ref, meta):
        train = mg.run_train_case(ref, FLAGS, fl, meta["n_classes"], meta["batch"], SEEDS, n_minibatches=1)
        mg.set_flags(FLAGS, fl)
        evaluation = ref_eval(ref, FLAGS, fl, meta)
    train["meta"] = evaluation["meta"] = np.array(json.dumps(meta))
    return train, evaluation


def pack_scalars(d):
    """The float64 scalars of a packed case (gradient norms, parameter sums, ...: every one of them a zip member of its own, 250 bytes
    of headers around 8 bytes of data) as ONE vector "scalars" beside their keys "scalar_keys" (JSON): the six more tensors of an
    attention receiver would otherwise carry the file past the g11 fixtures' size.  tests/desc_attn_ref.load_golden unpacks them."""
    keys = sorted(k for k, v in d.items() if isinstance(v, np.float64) or (isinstance(v, np.ndarray) and v.ndim == 0 and v.dtype == np.float64))
    out = {k: v for k, v in d.items() if k not in keys}
    out["scalars"] = np.array([float(d[k]) for k in keys], np.float64)
    out["scalar_keys"] = np.array(json.dumps(keys))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref, FLAGS = load_reference(args.ref)
    for mode in dar.MODES:
        for suffix, d in zip(("", "_eval"), case(ref, FLAGS, mode)):
            path = os.path.join(args.out, "g12_desc_attn_%s%s.npz" % (mode, suffix))
            np.savez_compressed(path, **pack_scalars(d))
            print("%-44s %7.1f KB  %d arrays" % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(d)))


if __name__ == "__main__":
    main()
