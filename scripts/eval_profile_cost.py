"""Times model.eval_dev over the 3 000-sample synthetic dev set (config 2's agents, -batch_size_dev 50: 60 dev batches), plain, with
the communication profile, with every sample's codes collected (one more launch per batch, no pair launches) or with topsim= (the
codes, then two pair launches per agent, image-level meaning, 64 bins, and the host's topsim()), every call between device
synchronisations.

  python scripts/eval_profile_cost.py [--root TREE] [--profile | --mode plain|profile|codes|topsim] [--calls N] [--warmup W] [--label L]

--root: the tree whose multimodalgame_amd is imported (default: this one; another checkout, built, for an A/B in one session:
start the variants in turn, several rounds, one process each).  Prints one JSON line: label, median / min / max in ms."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--profile", action="store_true")
ap.add_argument("--mode", default=None, choices=("plain", "profile", "codes", "topsim"))
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
mode = args.mode or ("profile" if args.profile else "plain")
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from multimodalgame_amd import flags as _flags, misc, model  # noqa: E402
from multimodalgame_amd.agents import Baseline, Receiver, Sender  # noqa: E402
from multimodalgame_amd.game import Game  # noqa: E402

tmp = tempfile.mkdtemp(prefix="mmg_evalcost_")
try:
    paths = misc.write_synthetic_dataset(os.path.join(tmp, "data"), n_classes=30, per_class=100, feat_dim=512, wv_dim=100)
    argv = ["model.py", "-experiment_name", "evalcost", "-log_path", os.path.join(tmp, "logs"), "-model_type", "Adaptive",
            "-batch_size", "64", "-max_exchange", "10", "-rec_w_dim", "32", "-sender_out_dim", "32", "-img_h_dim", "256",
            "-rec_hidden", "64", "-use_binary", "-top_k_train", "6"] + [a for k, v in paths.items() for a in ("-" + k, v)]
    _flags.define_flags()
    _flags.FLAGS.Reset()
    _flags.FLAGS(argv)
    _flags.default_flags(argv)
    F = _flags.FLAGS
    os.makedirs(F.log_path, exist_ok=True)
    torch.manual_seed(F.seed)
    device = torch.device("cuda:0")
    sender = Sender(F.img_feat, F.img_feat_dim, F.img_h_dim, F.rec_w_dim, F.sender_out_dim, F.use_binary, False, 0, False, 0)
    receiver = Receiver(F.sender_out_dim, F.wv_dim, F.rec_hidden, F.rec_out_dim, F.rec_w_dim, F.rec_s_dim, F.use_binary)
    game = Game(sender, receiver, Baseline(F.baseline_hid_dim, F.img_h_dim, F.rec_w_dim, 0),
                Baseline(F.baseline_hid_dim, 0, F.rec_w_dim, F.rec_hidden), device=device, seed=F.seed)
    desc, map_labels = model._desc_matrix(F.descr_dev, F.glove_path, F.wv_dim)
    desc = desc.to(device)
    if mode == "codes":                            # the codes alone: eval_dev's accumulator with codes=, no pair launches
        real = game.eval_accumulator
        game.eval_accumulator = lambda n_cls, top_k, **k: real(n_cls, top_k, codes=4096, **k)
    times, acc = [], None
    for i in range(args.warmup + args.calls):
        kw = dict(profile={}) if mode == "profile" else dict(topsim=dict(meaning="data", bins=64)) if mode == "topsim" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc, _ = model.eval_dev(F.dev_file, F.batch_size_dev, 0, F.shuffle_dev, F.top_k_dev, game, desc, map_labels, F.conf_mat, device, **kw)
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    out = dict(label=args.label or mode, calls=len(times), median_ms=float(np.median(times)),
               min_ms=float(min(times)), max_ms=float(max(times)), accuracy=acc,
               package=os.path.relpath(os.path.dirname(model.__file__)))
    if mode == "profile":
        out["profile_samples"] = int(kw["profile"]["head"][1])
    if mode == "topsim":
        ts = kw["topsim"]
        out.update(pairs=ts["sender"]["n_pairs"], spearman_sender=ts["sender"]["spearman"], spearman_receiver=ts["receiver"]["spearman"])
    print(json.dumps(out))
finally:
    _flags.FLAGS.Reset()
    shutil.rmtree(tmp, ignore_errors=True)
