#!/usr/bin/env python
"""Generate the g10 fixtures of wide class descriptions (-wv_dim 300, and a tiny 50-d case) by running the REFERENCE's own code.

Same rules as tests/golden/make_golden.py, whose loader, substitutions and harness this reuses: run in the build container
only, the reference is read and executed in memory, and only NUMBERS are written out (inputs by seed, recorded outputs).

  g10_wide_desc_adaptive    config 1's agents, Adaptive binary step at V = 300 (one minibatch: exchange, losses, four updates)
  g10_wide_desc_fixed       the same agents, Fixed exchange, V = 300
  g10_wide_desc_continuous  -nouse_binary, Fixed, 4 steps, 40 classes, V = 300
  g10_wide_desc_tiny50      tiny agents with unaligned dimensions at V = 50 (a real GloVe width that is not a multiple of 4)

usage: python tests/golden/make_golden_wide.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets oracle.PORTABLE_FP_ENV before torch loads)

import numpy as np  # noqa: E402

C1W = dict(mg.C1, wv_dim=300)
CONTW = dict(C1W, batch_size=16, max_exchange=4, entropy_rec=None, entropy_sen=None, entropy_s=None)
TINY50 = dict(mg.TINY, wv_dim=50)

# name -> (flags, classes, batch, seeds)
CASES = {
    "g10_wide_desc_adaptive": (dict(use_binary=True, fixed_exchange=False, **C1W), 30, 64, dict(weights=20, data=2001, uniforms=30)),
    "g10_wide_desc_fixed": (dict(use_binary=True, fixed_exchange=True, **C1W), 30, 32, dict(weights=21, data=2002, uniforms=31)),
    "g10_wide_desc_continuous": (dict(use_binary=False, fixed_exchange=True, **CONTW), 40, 16, dict(weights=22, data=2003, uniforms=32)),
    "g10_wide_desc_tiny50": (dict(use_binary=True, fixed_exchange=False, max_exchange=5, batch_size=8, learning_rate=1e-2,
                                  top_k_train=2, **TINY50), 5, 8, dict(weights=23, data=2004, uniforms=33)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref, FLAGS = mg.load_reference(args.ref)
    for name, (kw, n_classes, batch, seeds) in CASES.items():
        fl = mg.make_flags(**kw)
        d = mg.run_train_case(ref, FLAGS, fl, n_classes, batch, seeds, n_minibatches=1)
        d["meta"] = mg.flags_to_meta(fl, n_classes, batch, seeds, 1)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **d)
        print("%-28s %7.1f KB  %d arrays" % (name, os.path.getsize(path) / 1024.0, len(d)))


if __name__ == "__main__":
    main()
