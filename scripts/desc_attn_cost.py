"""What description attention costs per training minibatch.

  python scripts/desc_attn_cost.py [--windows 5] [--calls 20] [--batches 46] [--out profiles/desc_attn_cost.txt]

Config-2 shape (config 1's agents, binary, Adaptive, 30 classes, batch 64, T = 10), seed-0 weights, one process:
  plain   a plain handle forced onto the generic per-sample family (MMG_NO_FAST=1 MMG_NO_TILE=1 while it is created: the
          switches are read at mmg_create) -- the "generic sum" yardstick of the sender ablations
  attn    an attention handle (desc_attn_dim 64) over a seeded description set of 300 words in 30 classes of 1 to 70 words
(a) µs per minibatch: mmg_train_steps over `batches` fresh minibatches per call, host clock around `calls` calls ending in a
    device synchronise, `windows` windows per kind after a warm-up, the two kinds alternating; median and min-max of the windows.
(b) kernel times of single steps (HIP events around each launch, Engine.kernel_times), medians of 8 steps, profiling off in (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import cpu_ref  # noqa: E402

FLAGS = dict(use_binary=True, fixed_exchange=False, max_exchange=10, batch_size=64, learning_rate=1e-4, entropy_rec=0.01,
             entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64,
             wv_dim=100, baseline_hid_dim=500, top_k_train=6)
LENS = [9, 1, 8, 8, 70] + [9] * 4 + [8] * 21           # 300 words, 30 classes
ATTN_DIM, N_CLASSES, BATCH = 64, 30, 64


def build(attn):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**FLAGS)
    torch.manual_seed(0)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, True)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, True, desc_attn=attn, desc_attn_dim=ATTN_DIM)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0")
    if attn:
        rs = np.random.RandomState(1006)
        game.set_desc_set(torch.from_numpy((0.3 * rs.standard_normal((sum(LENS), fl.wv_dim))).astype(np.float32)), LENS)
    else:
        os.environ["MMG_NO_FAST"] = os.environ["MMG_NO_TILE"] = "1"
    try:
        eng = game.train_engine_for(BATCH, N_CLASSES)
    finally:
        os.environ.pop("MMG_NO_FAST", None); os.environ.pop("MMG_NO_TILE", None)
    assert "family 3 " in eng.plan_text().splitlines()[0], eng.plan_text()
    return game, eng


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", type=int, default=46)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "desc_attn_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.batches
    x, target, desc = cpu_ref.synthetic_batch(n * BATCH, N_CLASSES, FLAGS["img_feat_dim"], FLAGS["wv_dim"], seed=7)
    data, tgt, dsc = torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc[:N_CLASSES]).to(dev)
    kinds = {"plain": build(False), "attn": build(True)}

    def window(game):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            game.train_steps(data, tgt, dsc, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (args.calls * n)
    for game, _ in kinds.values():                       # warm-up: code objects, the first launches
        window(game)
    us = {k: [] for k in kinds}
    for _ in range(args.windows):
        for k, (game, _) in kinds.items():
            us[k].append(window(game))
    res = dict(windows=args.windows, minibatches_per_window=args.calls * n)
    for k, v in us.items():
        res[k + "_us_per_minibatch"] = float(np.median(v)); res[k + "_min"] = float(min(v)); res[k + "_max"] = float(max(v))
    for k, (game, eng) in kinds.items():
        per = {}
        for _ in range(8):
            torch.cuda.synchronize()
            eng.set_profiling(True)
            game.train_step(data[:BATCH], tgt[:BATCH], dsc)
            torch.cuda.synchronize()
            for name, ms in eng.kernel_times():
                per.setdefault(name, []).append(ms * 1e3)
            eng.set_profiling(False)
        res[k + "_kernels_us"] = {name: round(float(np.median(v)) * (len(v) // 8), 1) for name, v in per.items()}
    lines = ["description attention, cost per training minibatch (scripts/desc_attn_cost.py), MI355X, config-2 shape"]
    lines += ["%-28s %s" % (k, ("%.1f" % v) if isinstance(v, float) else v) for k, v in res.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
