"""What Gaussian message noise costs per training minibatch.

  python scripts/noise_cost.py --chain generic|mc3 [--noise] [--repo CHECKOUT] [--windows 5] [--calls 20] [--batches 16]

One process times ONE handle and prints one JSON line; a session starts several processes per variant, the variants alternating.
  generic  config 1's shape with continuous messages (batch 64, T = 10, 30 classes, Adaptive stopping), the handle forced onto the
           generic per-sample chain: MMG_NO_FAST=1 MMG_NO_TILE=1 while it is created (the switches are read at mmg_create)
  mc3      config 5's 256-sample shard (1000 classes, T = 10, Fixed, continuous) on the one-tile many-class chain: MMG_NO_MC3P=1
--noise: sigmas 0.3 / 0.2 (a noise handle selects those chains by itself; the switches are set all the same).  Without it: the clean
continuous handle on the same family, the yardstick.  --repo: import the package from another checkout (the parent commit's clean
handle).  µs per minibatch: mmg_train_steps over `batches` fresh minibatches per call, host clock around `calls` calls ending in a
device synchronise, `windows` windows after a warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = dict(feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=100, bas_hidden=500, max_exchange=10, use_binary=False,
          learning_rate=1e-4, top_k=6)
CHAINS = {"generic": (dict(C1, batch=64, n_classes=30, fixed_exchange=False), ("MMG_NO_FAST", "MMG_NO_TILE"), "family 3 "),
          "mc3": (dict(C1, batch=256, n_classes=1000, fixed_exchange=True), ("MMG_NO_MC3P",), "family 1 ")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chain", choices=sorted(CHAINS), required=True)
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--repo", default=REPO)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", type=int, default=16)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from multimodalgame_amd.engine import Engine
    from oracle import cpu_ref
    kw, env, family = CHAINS[args.chain]
    for k in env:
        os.environ[k] = "1"
    try:
        eng = Engine(device="cuda:0", **kw)
        if args.noise:
            eng.set_message_noise(0.3, 0.2)
    finally:
        for k in env:
            os.environ.pop(k, None)
    plan = eng.plan_text()
    assert family in plan.splitlines()[0] and " mc3p 0 " in plan, plan
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=0))
    n, B = args.batches, kw["batch"]
    x, target, desc = cpu_ref.synthetic_batch(n * B, kw["n_classes"], kw["feat_dim"], kw["wv_dim"], seed=7)
    dev = eng.device
    data, tgt, dsc = torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc[:kw["n_classes"]]).to(dev)

    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            eng.train_steps(data, tgt, dsc, n, seed=3)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (args.calls * n)
    window()                                              # warm-up: code objects, the first launches
    us = [window() for _ in range(args.windows)]
    eng.set_profiling(True)
    eng.train_step(data[:B], tgt[:B], dsc, seed=3)
    torch.cuda.synchronize()
    kernels = [name for name, _ in eng.kernel_times()]
    eng.set_profiling(False)
    eng.check_sync()
    print(json.dumps(dict(chain=args.chain, noise=bool(args.noise), repo=os.path.relpath(os.path.abspath(args.repo), REPO),
                          us_per_minibatch=[round(v, 2) for v in us], median=round(float(np.median(us)), 2), kernels=kernels)), flush=True)


if __name__ == "__main__":
    main()
