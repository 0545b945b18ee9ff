"""What visual attention costs per training minibatch and per evaluation conversation.

  python scripts/visual_attn_cost.py [--windows 5] [--calls 20] [--batches 16] [--out profiles/visual_attn_cost.txt]

Config-2 shape (config 1's agents, binary, Adaptive, 30 classes, batch 64, T = 10), seed-0 weights, one process:
  plain   a plain handle forced onto the generic per-sample family (MMG_NO_FAST=1 MMG_NO_TILE=1 while it is created: the
          switches are read at mmg_create) -- the "generic sum" yardstick of the sender ablations; x is [B, 512]
  vattn   a visual-attention handle: x is the 512 x 8 x 8 map, attn_dim 256, a 1000-d context
(a) us per training minibatch (mmg_train_steps) and per evaluation conversation (mmg_eval_steps) over `batches` fresh batches per
    call, host clock around `calls` calls ending in a device synchronise, `windows` windows per kind after a warm-up, the two
    kinds alternating; median and min-max of the windows.
(b) kernel times of single training steps and evaluation conversations (HIP events around each launch, Engine.kernel_times),
    medians of 8, profiling off in (a)."""
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
ATTN_DIM, HW, CTX, N_CLASSES, BATCH = 256, (8, 8), 1000, 30, 64


def build(vattn):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**FLAGS)
    torch.manual_seed(0)
    sender = Sender("layer4_2" if vattn else "avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, True,
                    use_attn=vattn, attn_dim=ATTN_DIM, attn_extra_context=vattn, attn_context_dim=CTX)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, True)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0")
    if not vattn:
        os.environ["MMG_NO_FAST"] = os.environ["MMG_NO_TILE"] = "1"
    try:
        eng = game.engine_for(BATCH, N_CLASSES, **(dict(n_feats=HW[0] * HW[1]) if vattn else {}))
    finally:
        os.environ.pop("MMG_NO_FAST", None); os.environ.pop("MMG_NO_TILE", None)
    assert "family 3 " in eng.plan_text().splitlines()[0], eng.plan_text()
    return game, eng


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "visual_attn_cost.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.batches
    x, target, desc = cpu_ref.synthetic_batch(n * BATCH, N_CLASSES, FLAGS["img_feat_dim"], FLAGS["wv_dim"], seed=7)
    tgt, dsc = torch.from_numpy(target).to(dev), torch.from_numpy(desc[:N_CLASSES]).to(dev)
    gen = torch.Generator().manual_seed(7)
    data = {"plain": torch.from_numpy(x).to(dev),
            "vattn": (0.5 * torch.randn(n * BATCH, FLAGS["img_feat_dim"], *HW, generator=gen)).to(dev)}
    ctx = {"plain": None, "vattn": (0.5 * torch.randn(n * BATCH, CTX, generator=gen)).to(dev)}
    kinds = {"plain": build(False), "vattn": build(True)}
    accs = {k: game.eval_accumulator(N_CLASSES, 6) for k, (game, _) in kinds.items()}

    def window(k, train):
        game = kinds[k][0]
        kw = {} if ctx[k] is None else dict(data_context=ctx[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            if train:
                game.train_steps(data[k], tgt, dsc, n, **kw)
            else:
                game.eval_steps(data[k], tgt, dsc, n, accs[k], **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (args.calls * n)
    res = dict(windows=args.windows, batches_per_window=args.calls * n)
    for train, what in ((True, "train_minibatch"), (False, "eval_conversation")):
        for k in kinds:                                  # warm-up: code objects, the first launches
            window(k, train)
        us = {k: [] for k in kinds}
        for _ in range(args.windows):
            for k in kinds:
                us[k].append(window(k, train))
        for k, v in us.items():
            res["%s_us_per_%s" % (k, what)] = float(np.median(v))
            res["%s_%s_min" % (k, what)] = float(min(v)); res["%s_%s_max" % (k, what)] = float(max(v))
    for k, (game, eng) in kinds.items():
        xb = data[k][:BATCH].contiguous().view(BATCH, FLAGS["img_feat_dim"], -1) if k == "vattn" else data[k][:BATCH]
        if k == "vattn":
            eng.set_data_context(ctx[k][:BATCH])
        for train in (False, True):
            per = {}
            for _ in range(8):
                torch.cuda.synchronize()
                eng.set_profiling(True)
                if train:
                    eng.train_step(xb, tgt[:BATCH], dsc, seed=0)
                else:
                    eng.forward(xb, tgt[:BATCH], dsc, seed=0, train=False, run_all=True)
                torch.cuda.synchronize()
                for name, ms in eng.kernel_times():
                    per.setdefault(name, []).append(ms * 1e3)
                eng.set_profiling(False)
            res["%s_%s_kernels_us" % (k, "train_step" if train else "eval")] = {
                name: round(float(np.median(v)) * (len(v) // 8), 1) for name, v in per.items()}
    lines = ["visual attention, cost per training minibatch / evaluation conversation (scripts/visual_attn_cost.py), MI355X, config-2 shape"]
    lines += ["%-36s %s" % (k, ("%.1f" % v) if isinstance(v, float) else v) for k, v in res.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
