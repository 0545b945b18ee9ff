#!/usr/bin/env python
"""Generate the g9 fixtures of message corruption (-bit_flip -corrupt_region) by running the REFERENCE's own code.

Same rules as tests/golden/make_golden.py, whose loader, substitutions and harness this reuses: run in the build container
only, the reference is read and executed in memory, and only NUMBERS are written out.

  g9_eval_corrupt_c1          the g4 weights and inputs (Adaptive binary, config-1 agents, 50 samples) through the
                              reference's exchange(train=False, corrupt=True, corrupt_region=REGION_C1), get_rec_outp and
                              the top-k of eval_dev (model.py:637-668, 813-820)
  g9_eval_corrupt_continuous  a small -nouse_binary case (Fixed, 4 steps): the abs applies to every message entry
  g9_build_mask               region strings -> the reference's build_mask (misc.py:388-402) output, or its IndexError

usage: python tests/golden/make_golden_corrupt.py [--ref /root/reference] [--out tests/golden]
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

REGION_C1 = "0,-1,-2:3,10:14"        # bit 0, bit W-1 by a negative index, a mixed-sign range (30, 31, 0, 1, 2), a plain range
REGION_CONT = "1:4,-3"
CONT = dict(mg.C1, batch_size=16, max_exchange=4, entropy_rec=None, entropy_sen=None, entropy_s=None)
# (region, W): in-range pieces of every form, negative single positions, mixed-sign and empty ranges, repeats, and the pieces
# outside [-W, W) that the reference rejects
MASK_CASES = [("0:3,5", 8), ("-1", 4), ("0:2,4,6:8", 9), ("-2:3", 32), ("30:32", 32), ("-32", 32), ("5:5", 32),
              ("3:1,7", 8), ("0,0,1", 4), ("-3:-1", 8), ("0:256", 256), ("-256,255", 256), ("31:33", 64),
              ("30:40", 32), ("32", 32), ("-33", 32), ("-40:-30", 32), ("0:9", 8)]


def ref_eval(ref, FLAGS, fl, models, x, target, desc, region, n_classes):
    exchange_args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc),
                         desc_set=None, desc_set_lens=None, train=False, break_early=not fl.fixed_exchange,
                         corrupt=True, corrupt_region=region)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = ref.exchange(models["sender"], models["receiver"], None, None, exchange_args)
        s_masks, s_feats, s_probs = s
        y_masks = None if fl.fixed_exchange else [torch.min(1 - m1, m2) for m1, m2 in zip(s_masks[1:], s_masks[:-1])]
        outp, _ = ref.get_rec_outp(y, y_masks)
        dist = F.log_softmax(outp, dim=1)
    top_k_ind = dist.numpy().argsort()[:, -fl.top_k_dev:]                     # model.py:658
    out = {}
    out["n_steps"] = np.int64(len(y))
    out["s_masks"] = mg._stack(s_masks).astype(np.uint8)
    out["s_feats"], out["s_probs"] = mg._stack(s_feats), mg._stack(s_probs)
    out["sen_feats"] = mg._stack(sen_w[0])
    if fl.use_binary:
        out["sen_probs"], out["rec_probs"] = mg._stack(sen_w[1]), mg._stack(rec_w[1])
    out["rec_feats"] = mg._stack(rec_w[0])
    out["y"] = mg._stack(y)
    out["outp"], out["dist"] = outp.numpy(), dist.numpy()
    out["top_k_ind"] = top_k_ind.astype(np.int64)
    out["hits"] = np.int64((top_k_ind == target.reshape(-1, 1)).sum())
    out["conversation_lengths"] = torch.cat(s_feats, 1).float().sum(1).numpy()
    out["mask"] = ref_mask(region, fl.rec_w_dim)
    out["region"] = np.array(region)
    return out


def ref_mask(region, size):
    import misc                                   # the reference's misc.py (make_golden.load_reference put it on the path)
    return misc.build_mask(region, size).numpy().reshape(-1).astype(np.uint8)


def case_c1(ref, FLAGS):
    fl = mg.make_flags(use_binary=True, fixed_exchange=False, **mg.C1)
    mg.set_flags(FLAGS, fl)
    models = mg.build_ref_models(ref, FLAGS)
    cpu_ref.load_filled(models, seed=3)
    with torch.no_grad():
        models["receiver"].s.bias.fill_(1.2)      # as g4_eval_c1
    x, target, desc = cpu_ref.synthetic_batch(50, 30, 512, 100, seed=77)
    out = ref_eval(ref, FLAGS, fl, models, x, target, desc, REGION_C1, 30)
    out["meta"] = mg.flags_to_meta(fl, 30, 50, dict(weights=3, data=77, uniforms=0), 0)
    return out


def case_continuous(ref, FLAGS):
    fl = mg.make_flags(use_binary=False, fixed_exchange=True, **CONT)
    mg.set_flags(FLAGS, fl)
    models = mg.build_ref_models(ref, FLAGS)
    cpu_ref.load_filled(models, seed=9)
    x, target, desc = cpu_ref.synthetic_batch(16, 40, 512, 100, seed=91)
    out = ref_eval(ref, FLAGS, fl, models, x, target, desc, REGION_CONT, 40)
    out["meta"] = mg.flags_to_meta(fl, 40, 16, dict(weights=9, data=91, uniforms=0), 0)
    return out


def case_masks():
    table = []
    for region, size in MASK_CASES:
        try:
            table.append([region, size, ref_mask(region, size).tolist()])
        except IndexError:
            table.append([region, size, "IndexError"])
    return dict(table=np.array(json.dumps(table)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref, FLAGS = mg.load_reference(args.ref)

    def save(name, d):
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-28s %7.1f KB  %d arrays" % (name, os.path.getsize(path) / 1024.0, len(d)))

    save("g9_eval_corrupt_c1", case_c1(ref, FLAGS))
    save("g9_eval_corrupt_continuous", case_continuous(ref, FLAGS))
    save("g9_build_mask", case_masks())


if __name__ == "__main__":
    main()
