"""Time the joint sender-receiver VJP of exchange(channel_grad=True) (include/mmg.h: mmg_exchange_vjp_channel).

  python scripts/channel_vjp_time.py [--reps 40] [--warmup 5] [--out profiles/channel_vjp.txt]

Config-1 agents (binary, H 256, W 32, R 64, V 100, 30 classes), B 64, all T = 10 steps, seed-0 weights.  The loss is
nll(y[-1]) + sum_t mean(sen_probs_t): it touches both agents' outputs, so that the detached path runs both of its VJPs.  Medians:
  (a) k_vjp_rec + k_vjp_sen of the two detached VJPs (HIP events around each launch, Engine.kernel_times)
  (b) k_vjp_channel, the same way
  (c) wall time of one backward() through exchange(channel_grad=True), host clock, synchronised at both ends
  (d) wall time of the backward() of the same gradient through the module-level loop (straight-through line in torch)
and the wall time of forward + backward of both routes.  (c) and (d) alternate in one process, profiling off."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import cpu_ref  # noqa: E402

KW = dict(use_binary=True, fixed_exchange=False, max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01,
          entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6, batch_size=64)
N_CLASSES, BATCH = 30, 64


def build():
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**KW)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", autograd=True)
    eng = game.engine_for(BATCH, N_CLASSES)
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=0))
    return fl, game, eng


def loss_of(sen, y, target):
    return F.nll_loss(F.log_softmax(y[-1], dim=1), target) + sum(p.mean() for p in sen)


def exchange_loss(game, data, desc, target, channel):
    out = game.exchange(dict(data=data, target=target, desc=desc, train=True, break_early=False, channel_grad=channel))
    return loss_of(out[1][1], out[3], target)


def module_loss(game, fl, data, desc, target):
    S, Rc = game.modules["sender"], game.modules["receiver"]
    S.train(); Rc.train()
    Rc.reset_state()
    sen, y, w_in = [], [], None
    for t in range(fl.max_exchange):
        z, zp = S(data, w_in, None, t)
        (_, _), (w, wp), outp = Rc(z.detach() + (zp - zp.detach()), desc)
        w_in = w.detach() + (wp - wp.detach())
        sen.append(zp); y.append(outp)
    return loss_of(sen, y, target)


def zero(game):
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)


def timed_backward(make_loss, game):
    """(forward + backward ms, backward ms), host clock, synchronised."""
    zero(game)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = make_loss()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3


def kernel_ms(game, eng, make_loss, names):
    zero(game)
    loss = make_loss()
    torch.cuda.synchronize()
    eng.set_profiling(True)
    loss.backward()
    torch.cuda.synchronize()
    times = eng.kernel_times()
    eng.set_profiling(False)
    return {n: sum(ms for k, ms in times if k == n) for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "channel_vjp.txt"))
    args = ap.parse_args()
    fl, game, eng = build()
    dev = torch.device("cuda:0")
    x, target, desc = cpu_ref.synthetic_batch(BATCH, N_CLASSES, fl.img_feat_dim, fl.wv_dim, seed=7)
    data, dsc, tgt = torch.from_numpy(x).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(target).to(dev)
    routes = dict(detached=lambda: exchange_loss(game, data, dsc, tgt, False),
                  channel=lambda: exchange_loss(game, data, dsc, tgt, True),
                  module_loop=lambda: module_loss(game, fl, data, dsc, tgt))
    for _ in range(args.warmup):
        for fn in routes.values():
            timed_backward(fn, game)
    kern = dict(detached=("k_vjp_rec", "k_vjp_sen"), channel=("k_vjp_channel",))
    per_kernel = {r: {n: [] for n in names} for r, names in kern.items()}
    wall = {r: ([], []) for r in routes}
    for _ in range(args.reps):                                     # the routes alternate: all see the same machine state
        for r, names in kern.items():
            for n, ms in kernel_ms(game, eng, routes[r], names).items():
                per_kernel[r][n].append(ms)
        for r, fn in routes.items():
            both, bwd = timed_backward(fn, game)
            wall[r][0].append(both); wall[r][1].append(bwd)
    med = lambda v: float(np.median(v))
    res = dict(config="config-1 agents, binary straight-through, B 64, T 10, 30 classes, seed-0 weights", reps=args.reps,
               warmup=args.warmup,
               a_k_vjp_rec_ms=med(per_kernel["detached"]["k_vjp_rec"]), a_k_vjp_sen_ms=med(per_kernel["detached"]["k_vjp_sen"]),
               b_k_vjp_channel_ms=med(per_kernel["channel"]["k_vjp_channel"]),
               c_backward_exchange_channel_ms=med(wall["channel"][1]), d_backward_module_loop_ms=med(wall["module_loop"][1]),
               backward_exchange_detached_ms=med(wall["detached"][1]),
               fwd_bwd_exchange_channel_ms=med(wall["channel"][0]), fwd_bwd_module_loop_ms=med(wall["module_loop"][0]),
               fwd_bwd_exchange_detached_ms=med(wall["detached"][0]))
    res["a_ms"] = res["a_k_vjp_rec_ms"] + res["a_k_vjp_sen_ms"]
    res["b_over_a"] = res["b_k_vjp_channel_ms"] / res["a_ms"]
    res["d_over_c"] = res["d_backward_module_loop_ms"] / res["c_backward_exchange_channel_ms"]
    lines = ["channel VJP timing (scripts/channel_vjp_time.py): medians of %d repetitions after %d warm-up rounds, MI355X" % (args.reps, args.warmup)]
    lines += ["%-34s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v) for k, v in res.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
