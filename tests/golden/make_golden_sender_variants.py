#!/usr/bin/env python
"""Generate the g11 fixtures of the sender's communication ablations (-sender_mix prod, -ignore_code, -ignore_receiver) by running
the REFERENCE's own code.

Same rules as tests/golden/make_golden.py, whose loader, substitutions and harness this reuses: run in the build container
only, the reference is read and executed in memory, and only NUMBERS are written out.  make_golden.set_flags hard-sets
sender_mix = "sum" and ignore_code = False; the two are overridden here right behind it.  (model.py:471's
Variable(..., volatile=...) runs as it stands on torch 2.10 -- volatile is ignored with a warning --, so no further substitution.)

  g11_sender_variant_<setting>   config-1 agents (H 256, W 32, R 64, V 100, K 500), 30 classes, 16 samples, 4 steps, Adaptive,
                                 binary, config 1's entropy weights; settings: prod, ignore_code, ignore_receiver,
                                 prod_ignore_receiver.  One training minibatch (keys mb0.*, packed as
                                 make_golden.run_train_case packs it)
  g11_sender_variant_<setting>_eval   one evaluation conversation of the same agents on the same inputs (keys eval.*) -- a file of
                                 its own, so that each stays within the size of the g3_tiny_* fixtures

usage: python tests/golden/make_golden_sender_variants.py --ref REFERENCE_DIR [--out tests/golden]
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

SHAPE = dict(mg.C1, batch_size=16, max_exchange=4)
N_CLASSES, BATCH = 30, 16
SEEDS = dict(weights=5, data=6, uniforms=7)          # tests/test_sender_variant_cpu.py checks what these seeds reach
SETTINGS = {"prod": ("prod", False, False), "ignore_code": ("sum", True, False), "ignore_receiver": ("sum", False, True),
            "prod_ignore_receiver": ("prod", False, True)}


def flags_for(setting):
    return mg.make_flags(use_binary=True, fixed_exchange=False, ignore_receiver=setting[2], **SHAPE)


def with_variant(setting):
    """make_golden.set_flags followed by the two switches it pins."""
    plain = mg.set_flags

    def set_flags(FLAGS, fl):
        plain(FLAGS, fl)
        FLAGS.sender_mix, FLAGS.ignore_code = setting[0], setting[1]
    return plain, set_flags


def ref_eval(ref, FLAGS, fl):
    """The per-batch body of eval_dev (model.py:620-668) on the seeded weights and minibatch 0's inputs."""
    models = mg.build_ref_models(ref, FLAGS)
    cpu_ref.load_filled(models, seed=SEEDS["weights"])
    x, target, desc = cpu_ref.synthetic_batch(BATCH, N_CLASSES, fl.img_feat_dim, fl.wv_dim, seed=SEEDS["data"])
    exchange_args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc),
                         desc_set=None, desc_set_lens=None, train=False, break_early=True, corrupt=False, corrupt_region=None)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = ref.exchange(models["sender"], models["receiver"], None, None, exchange_args)
        s_masks, s_feats, s_probs = s
        y_masks = [torch.min(1 - m1, m2) for m1, m2 in zip(s_masks[1:], s_masks[:-1])]
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


def case(ref, FLAGS, setting):
    fl = flags_for(setting)
    plain, mg.set_flags = with_variant(setting)
    try:
        train = mg.run_train_case(ref, FLAGS, fl, N_CLASSES, BATCH, SEEDS, n_minibatches=1)
        mg.set_flags(FLAGS, fl)
        evaluation = ref_eval(ref, FLAGS, fl)
    finally:
        mg.set_flags = plain
    meta = json.loads(str(mg.flags_to_meta(fl, N_CLASSES, BATCH, SEEDS, 1)))
    meta.update(sender_mix=setting[0], ignore_code=setting[1])
    train["meta"] = evaluation["meta"] = np.array(json.dumps(meta))
    return train, evaluation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref, FLAGS = mg.load_reference(args.ref)
    for name, setting in SETTINGS.items():
        for suffix, d in zip(("", "_eval"), case(ref, FLAGS, setting)):
            path = os.path.join(args.out, "g11_sender_variant_%s%s.npz" % (name, suffix))
            np.savez_compressed(path, **d)
            print("%-44s %7.1f KB  %d arrays" % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(d)))


if __name__ == "__main__":
    main()
