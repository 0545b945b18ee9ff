"""Time the input gradients of exchange(input_grad=True) (include/mmg.h: mmg_vjp_input_grads; kernels_vjp.h: k_vjp_ddesc).

  python scripts/input_grad_time.py [--reps 40] [--warmup 5] [--out profiles/input_grad.txt]

Two shapes, seed-0 weights, channel_grad on, all T = 10 steps, loss nll(y[-1]):
  c1   config-1 agents (binary, H 256, W 32, R 64, V 100), 30 classes, B 64
  c5   config 5's 256-sample shard (continuous, Fixed, same agents), 1000 classes, B 256
Medians per shape:
  (a) wall time of one backward() without and with input_grad (data and desc require grad), host clock, synchronised at both
      ends, the two alternating in one process, profiling off
  (b) the launches mmg_vjp_input_grads adds (HIP events around each, Engine.kernel_times): k_vjp_nn (d data = dhx . W_image and
      q = dgpre . W_d) and k_vjp_ddesc
  (c) k_vjp_ddesc alone against torch forming the same two products in fp32 from the same tape arrays,
      softmax(y).T @ q + vdC @ W_y1[:, R:] (torch.cuda events around the three torch launches, TF32 off)
No plain-loop variant of k_vjp_ddesc exists to time against: (c) is the only comparison."""
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

AGENTS = dict(learning_rate=1e-4, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
              baseline_hid_dim=500, top_k_train=6, max_exchange=10)
SHAPES = {
    "c1": (dict(AGENTS, use_binary=True, fixed_exchange=False, entropy_rec=0.01, entropy_sen=0.01, entropy_s=0.08), 30, 64),
    "c5": (dict(AGENTS, use_binary=False, fixed_exchange=True), 1000, 256),
}


def build(kw, n_classes, batch):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**dict(kw, batch_size=batch))
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", autograd=True,
                channel_grad=True)
    eng = game.engine_for(batch, n_classes)
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=0))
    return fl, game, eng


def make_loss(game, data, desc, target, input_grad):
    out = game.exchange(dict(data=data, target=target, desc=desc, train=True, break_early=False, input_grad=input_grad))
    return F.nll_loss(F.log_softmax(out[3][-1], dim=1), target)


def zero(game, *leaves):
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)
    for t in leaves:
        t.grad = None


def timed_backward(game, data, desc, target, input_grad):
    zero(game, data, desc)
    loss = make_loss(game, data, desc, target, input_grad)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_ms(game, eng, data, desc, target):
    zero(game, data, desc)
    loss = make_loss(game, data, desc, target, True)
    torch.cuda.synchronize()
    eng.set_profiling(True)
    loss.backward()
    torch.cuda.synchronize()
    times = eng.kernel_times()
    eng.set_profiling(False)
    first = [i for i, (k, _) in enumerate(times) if k in ("k_vjp_nn", "k_vjp_nn_plain")][0]     # (the entry runs behind the VJP)
    return {n: sum(ms for k, ms in times[first:] if k == n) for n in ("k_vjp_nn", "k_vjp_ddesc")}


def torch_ddesc_ms(eng, n):
    """torch forming d desc from the tape the last backward() left: softmax(y).T @ vdq + vdC @ W_y1[:, R:], fp32."""
    tp, R = eng.tape, eng.cfg.rec_hidden
    rows = n * eng.cfg.batch
    y, q = tp["y"].view(-1, eng.cfg.n_classes)[:rows], tp["vdq"].view(-1, eng.cfg.wv_dim)[:rows]
    w = eng.params["receiver"]["y1.weight"][:, R:]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = torch.addmm(tp["vdC"] @ w, torch.softmax(y, dim=1).t(), q)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def run_shape(name, reps, warmup):
    kw, n_classes, batch = SHAPES[name]
    fl, game, eng = build(kw, n_classes, batch)
    dev = torch.device("cuda:0")
    x, target, desc = cpu_ref.synthetic_batch(batch, n_classes, fl.img_feat_dim, fl.wv_dim, seed=7)
    data = torch.from_numpy(x).to(dev).requires_grad_(True)
    dsc = torch.from_numpy(desc).to(dev).requires_grad_(True)
    tgt = torch.from_numpy(target).to(dev)
    for _ in range(warmup):
        for on in (False, True):
            timed_backward(game, data, dsc, tgt, on)
        torch_ddesc_ms(eng, fl.max_exchange)
    wall = {False: [], True: []}
    kern = {"k_vjp_nn": [], "k_vjp_ddesc": []}
    tor = []
    err = 0.0
    for _ in range(reps):
        for on in (False, True):
            wall[on].append(timed_backward(game, data, dsc, tgt, on))
        for k, ms in kernel_ms(game, eng, data, dsc, tgt).items():
            kern[k].append(ms)
        ms, ref = torch_ddesc_ms(eng, fl.max_exchange)
        tor.append(ms)
        err = max(err, float((ref - dsc.grad).abs().max()))
    med = lambda v: float(np.median(v))
    return {"%s_shape" % name: "B %d, D %d, T %d, %s" % (batch, n_classes, fl.max_exchange, "binary" if fl.use_binary else "continuous"),
            "%s_backward_ms" % name: med(wall[False]), "%s_backward_input_grad_ms" % name: med(wall[True]),
            "%s_k_vjp_nn_ms" % name: med(kern["k_vjp_nn"]), "%s_k_vjp_ddesc_ms" % name: med(kern["k_vjp_ddesc"]),
            "%s_torch_ddesc_ms" % name: med(tor), "%s_ddesc_max_abs_diff_to_torch" % name: err}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "input_grad.txt"))
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    res = dict(reps=args.reps, warmup=args.warmup)
    for name in ("c1", "c5"):
        res.update(run_shape(name, args.reps, args.warmup))
    lines = ["input-gradient timing (scripts/input_grad_time.py): medians of %d repetitions after %d warm-up rounds, MI355X"
             % (args.reps, args.warmup)]
    lines += ["%-34s %s" % (k, ("%.4f" % v if v >= 1e-3 else "%.3e" % v) if isinstance(v, float) else v) for k, v in res.items()]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
