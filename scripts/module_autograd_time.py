"""Time the module-level autograd loop: the reference's exchange() body written with agent-module calls (model.py:788-876), its
losses (oracle/cpu_ref helpers on CPU copies, model.py:1248-1305) and four backward() calls (model.py:1309-1328) -- against the
same loop over the same parameters in plain PyTorch on the GPU.

  python scripts/module_autograd_time.py [--configs c2,c5shard] [--iters 20] [--warmup 3] [--losses cpu|device|cpu,device]

c2: configs[1] (Adaptive, binary, 30 classes, batch 64, max_exchange 10).  c5shard: one GPU's shard of configs[4] (Fixed,
continuous, 1000 classes, 256 samples).  Prints one JSON line per config: wall ms per minibatch (forward + losses + backward,
host time included, synchronised at the end of every minibatch) for the HIP modules and for plain PyTorch.

--losses cpu (the default): the losses are oracle/cpu_ref's on CPU copies, as above.  --losses device: multimodalgame_amd.losses on
the device (no copies).  --losses cpu,device measures both routes in one invocation: per config the two routes alternate in
--rounds rounds of --iters minibatches each, and the line carries every round's time and the median per route
(hip_ms_<route>); plain PyTorch is timed with the cpu route only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import cpu_ref  # noqa: E402

BASE = dict(img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100, baseline_hid_dim=500,
            max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01, entropy_s=0.08)
CONFIGS = {
    "c2": (dict(BASE, use_binary=True, fixed_exchange=False), 30, 64),
    "c5shard": (dict(BASE, use_binary=False, fixed_exchange=True, entropy_rec=None, entropy_sen=None, entropy_s=None), 1000, 256),
}


# ------------------------------------------------------------------ plain PyTorch agents over cpu_ref's parameters
class PlainSender(nn.Module):
    def __init__(self, ref):
        super().__init__()
        self.ref, self.w_dim, self.use_binary = ref, ref.w_dim, ref.use_binary

    def forward(self, x, w, g, t):
        S = self.ref
        self.h_x = h_x = S.image_layer(x)
        h_w = S.code_layer(torch.sigmoid(S.code_bias.view(1, -1))).expand(x.size(0), S.h_dim) if t == 0 else S.code_layer(w)
        feats = S.binary_layer(torch.tanh(h_x + h_w))
        if not self.use_binary:
            return feats, None
        probs = torch.sigmoid(feats)
        return (torch.rand_like(probs) < probs).float(), probs


class PlainReceiver(nn.Module):
    def __init__(self, ref):
        super().__init__()
        self.ref, self.use_binary = ref, ref.use_binary
        self.h_z = None

    def reset_state(self):
        self.h_z = None

    def forward(self, z, desc):
        Rc = self.ref
        B, D = z.size(0), desc.size(0)
        if self.h_z is None:
            self.h_z = torch.zeros(B, Rc.hid_dim, device=z.device)
        self.h_z = h = Rc.rnn(z, self.h_z)
        s_prob = torch.sigmoid(Rc.s(h))
        s = (torch.rand_like(s_prob) < s_prob).float()
        inp = torch.cat([h.repeat_interleave(D, 0), desc.repeat(B, 1)], 1)
        y = Rc.y2(Rc.y1(inp).clamp(min=0)).view(B, -1)
        dbar = F.softmax(y, dim=1).detach() @ desc
        self.h_w = torch.tanh(Rc.w_h(h) + Rc.w_d(dbar))
        ws = Rc.w(self.h_w)
        if not self.use_binary:
            return (s, s_prob), (ws, None), y
        wp = torch.sigmoid(ws)
        return (s, s_prob), ((torch.rand_like(wp) < wp).float(), wp), y


# ------------------------------------------------------------------ the loop
def module_exchange(agents, fl, data, desc, break_early):
    """model.py:788-876 with module calls; .detach() where the reference takes .data."""
    sender, receiver, baseline_sen, baseline_rec = agents
    B = data.size(0)
    stop_mask = [torch.ones(B, 1, dtype=torch.uint8, device=data.device)]
    s_feat, s_prob_l, sen_feats, sen_probs, rec_feats, rec_probs, y, bs, br = [], [], [], [], [], [], [], [], []
    w_binary = torch.full((B, sender.w_dim), float(fl.first_rec), device=data.device)
    receiver.reset_state()
    for t in range(fl.max_exchange):
        z_r = w_binary
        z_binary, z_probs = sender(data, z_r.detach(), None, t)
        (s_binary, s_prob), (w_binary, w_probs), outp = receiver(z_binary.detach(), desc)
        if fl.use_binary:
            bs.append(baseline_sen(sender.h_x.detach(), z_r.detach(), None))
            br.append(baseline_rec(None, z_binary.detach(), receiver.h_z.detach()))
        stop_mask.append(torch.min(stop_mask[-1], s_binary.byte()))
        s_feat.append(s_binary)
        s_prob_l.append(s_prob)
        sen_feats.append(z_binary)
        sen_probs.append(z_probs)
        rec_feats.append(w_binary)
        rec_probs.append(w_probs)
        y.append(outp.view(B, -1))
        if break_early and stop_mask[-1].float().sum().item() == 0:
            break
    stop_mask[-1].fill_(0)
    return (stop_mask, s_feat, s_prob_l), (sen_feats, sen_probs), (rec_feats, rec_probs), y, bs, br


def losses(fl, out, target):
    """model.py:1248-1305 (cpu_ref's helpers) on CPU copies that keep the graph."""
    s, sen_w, rec_w, y, bs, br = out
    c = lambda lst: [None if t is None else t.cpu() for t in lst]
    s_masks, s_feats, s_probs = c(s[0]), c(s[1]), c(s[2])
    sen_feats, sen_probs, rec_feats, rec_probs, y, bs, br = c(sen_w[0]), c(sen_w[1]), c(rec_w[0]), c(rec_w[1]), c(y), c(bs), c(br)
    if fl.fixed_exchange:
        m_s = m_rec = m_sen = m_bas = y_masks = None
    else:
        m_s, m_rec, m_sen, m_bas = s_masks[:-1], s_masks[1:-1], s_masks[:-1], s_masks[:-1]
        y_masks = [torch.min(1 - m1, m2) for m1, m2 in zip(s_masks[1:], s_masks[:-1])]
    outp, _ = cpu_ref.get_rec_outp(y, y_masks)
    dist = F.log_softmax(outp, dim=1)
    nll = F.nll_loss(dist, target)
    logs = dist.detach().gather(1, target.view(-1, 1))
    if not fl.use_binary:
        return {"receiver": nll}
    loss_rec = nll
    if len(rec_feats[:-1]) > 0:
        loss_rec = loss_rec + cpu_ref.multistep_loss_binary(rec_feats[:-1], rec_probs[:-1], logs, br[:-1], m_rec, fl.entropy_rec)[0]
    if not fl.fixed_exchange:
        loss_rec = loss_rec + cpu_ref.multistep_loss_binary(s_feats, s_probs, logs, br, m_s, fl.entropy_s)[0]
    return {"receiver": loss_rec,
            "sender": cpu_ref.multistep_loss_binary(sen_feats, sen_probs, logs, bs, m_sen, fl.entropy_sen)[0],
            "baseline_rec": cpu_ref.multistep_loss_bas(br, logs, m_bas),
            "baseline_sen": cpu_ref.multistep_loss_bas(bs, logs, m_bas)}


def device_losses(fl, out, target):
    """model.py:1248-1305 on the device: multimodalgame_amd.losses.training_losses, nothing is copied to the host."""
    from multimodalgame_amd.losses import training_losses
    return training_losses(out, target, fl)


def minibatch(agents, params, fl, data, desc, target, route="cpu"):
    for p in params:
        p.grad = None
    ls = (device_losses if route == "device" else losses)(fl, module_exchange(agents, fl, data, desc, not fl.fixed_exchange), target)
    for k in ("receiver", "sender", "baseline_rec", "baseline_sen"):
        if k in ls:
            ls[k].backward()
    torch.cuda.synchronize()


def time_loop(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) * 1e3 / iters


def run(name, iters, warmup, which, routes=("cpu",), rounds=1):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    kw, n_classes, batch = CONFIGS[name]
    fl = cpu_ref.Flags(**kw)
    dev = torch.device("cuda:0")
    x, target, desc = cpu_ref.synthetic_batch(batch, n_classes, fl.img_feat_dim, fl.wv_dim, seed=7)
    data, dsc, tgt = torch.from_numpy(x).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(target)
    res = dict(config=name, batch=batch, n_classes=n_classes, iters=iters)
    ref = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(ref, seed=3)
    if which in ("both", "hip"):
        sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
        receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
        bsen, brec = Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0), Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden)
        game = Game(sender, receiver, bsen, brec, flags=fl, device="cuda:0", autograd=True)
        eng = game.engine_for(batch, n_classes)
        eng.load_state_dicts({a: {k: v.detach() for k, v in m.state_dict().items()} for a, m in ref.items()})
        agents = (sender, receiver, bsen, brec)
        for m in agents:
            m.train()
        params = [p for m in agents for p in m.parameters()]
        tgts = {"cpu": tgt, "device": tgt.to(dev)}
        if routes == ("cpu",) and rounds == 1:
            res["hip_ms"] = time_loop(lambda: minibatch(agents, params, fl, data, dsc, tgt), iters, warmup)
        else:
            per = {r: [] for r in routes}
            for i in range(rounds):                                  # the routes alternate: both see the same machine state
                for r in routes:
                    per[r].append(time_loop(lambda: minibatch(agents, params, fl, data, dsc, tgts[r], r), iters, warmup if i == 0 else 1))
            res["rounds"] = rounds
            for r in routes:
                res["hip_ms_%s_rounds" % r] = per[r]
                res["hip_ms_%s" % r] = float(np.median(per[r]))
            res["hip_ms"] = res["hip_ms_%s" % routes[0]]
    if which in ("both", "torch"):
        plain = {k: m.to(dev) for k, m in ref.items()}
        agents = (PlainSender(plain["sender"]), PlainReceiver(plain["receiver"]), plain["baseline_sen"], plain["baseline_rec"])
        params = [p for m in plain.values() for p in m.parameters()]
        res["torch_ms"] = time_loop(lambda: minibatch(agents, params, fl, data, dsc, tgt), iters, warmup)
    if "hip_ms" in res and "torch_ms" in res:
        res["speedup"] = res["torch_ms"] / res["hip_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="c2,c5shard")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--which", choices=("both", "hip", "torch"), default="both")
    ap.add_argument("--losses", default="cpu", help="cpu, device or cpu,device (both routes, alternating)")
    ap.add_argument("--rounds", type=int, default=1, help="alternating rounds per route with --losses cpu,device")
    args = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    routes = tuple(args.losses.split(","))
    if not routes or any(r not in ("cpu", "device") for r in routes):
        ap.error("--losses takes cpu, device or cpu,device")
    for name in args.configs.split(","):
        print(json.dumps(run(name, args.iters, args.warmup, args.which, routes, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
