"""Float64 reference of one training conversation with or without gradients through the channel (test side only).

f64_outputs is the loop of tests/test_autograd_gpu.py::_f64_outputs -- cpu_ref's agents in double on a recorded discrete
trajectory, ReLU sides taken from the recorded forward where a pre-activation is within 1e-4 of zero -- with one more argument:

  channel=False   the reference's graph: every message crossing between the agents is a constant (model.py:807-811, 826-829).
  channel=True    continuous messages: the receiver reads the sender's logits feats_t and the sender's step t + 1 reads the
                  receiver's logits ws_t, both WITH their graph.  Binary messages: the bits are the recorded ones and
                  z = pz + (z_bits - pz).detach(), w = pw + (w_bits - pw).detach() (straight-through).
The baselines' inputs, softmax(y) inside dbar, the stop bits, data and desc stay constants in both.

The trajectory (`tp`) is the engine's tape after a VJP has run (z, w, vA, vCd, vhid_s, vhid_r) or cpu_tape()'s stand-in, which
needs no GPU.  frozen: a dict that records the constants of the graph (dbar, the ReLU sides) on the first call and replays them
on later ones, so that a finite-difference check perturbs the parameters of exactly the differentiated function.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

CHANNEL_AGENTS = ("sender", "receiver")


def relu_mask(pre, rec_on, eps=1e-4):
    """ReLU mask of the float64 reference; units within eps of the threshold take the side the recorded forward put them on
    (d relu / dx is discontinuous there: both sides are correct)."""
    return torch.where(pre.abs() < eps, rec_on, pre > 0)


def _double(module):
    return module if next(module.parameters()).dtype == torch.float64 else module.double()


def _frozen(frozen, key, make):
    if frozen is None:
        return make()
    if key not in frozen:
        frozen[key] = make().detach()
    return frozen[key]


def f64_outputs(models, fl, x, desc, tp, n, channel=False, frozen=None):
    S, Rc, BS, BR = (_double(models[k]) for k in ("sender", "receiver", "baseline_sen", "baseline_rec"))
    x64 = torch.as_tensor(x).double()
    d64 = torch.as_tensor(desc).double()
    B, D, R = x64.shape[0], d64.shape[0], fl.rec_hidden
    binary = fl.use_binary
    g = lambda k: tp[k].detach().double().cpu()
    z_rec, w_rec = g("z"), g("w")
    vA, vCd = g("vA"), g("vCd")
    out = {k: [] for k in ("sen", "y", "ps", "w", "bs", "br")}
    h = torch.zeros(B, R, dtype=torch.float64)
    w_in = None                                                 # the sender's code input of step t: w_{t-1}
    for t in range(n):
        h_x = S.image_layer(x64)
        if t == 0:
            h_w = S.code_layer(torch.sigmoid(S.code_bias.view(1, -1))).expand(B, fl.img_h_dim)
        else:
            h_w = S.code_layer(w_in)
        feats = S.binary_layer(torch.tanh(h_x + h_w))
        if binary:
            pz = torch.sigmoid(feats)
            out["sen"].append(pz)
            z_t = pz + (z_rec[t] - pz).detach() if channel else z_rec[t]
        else:
            out["sen"].append(feats)
            z_t = feats if channel else z_rec[t]
        h = Rc.rnn(z_t, h)
        out["ps"].append(torch.sigmoid(Rc.s(h)))
        pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, D, R)
        on = _frozen(frozen, ("on", t), lambda: relu_mask(pre, (vA[t][:, None, :] + vCd[None, :, :]) > 0).double())
        y = Rc.y2((pre * on).view(B * D, R)).view(B, -1)
        out["y"].append(y)
        dbar = _frozen(frozen, ("dbar", t), lambda: F.softmax(y, dim=1).detach() @ d64)
        ws = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(dbar)))
        if binary:
            pw = torch.sigmoid(ws)
            out["w"].append(pw)
            w_in = pw + (w_rec[t] - pw).detach() if channel else w_rec[t]
        else:
            out["w"].append(ws)
            w_in = ws if channel else w_rec[t]
        if binary:                                              # the baselines read constants (model.py:835-843)
            zr = torch.full((B, fl.rec_w_dim), float(fl.first_rec), dtype=torch.float64) if t == 0 else w_rec[t - 1]
            p1 = BS.linear1(torch.cat([h_x.detach(), zr], 1))
            out["bs"].append(BS.linear2(p1 * relu_mask(p1, g("vhid_s")[t] > 0)))
            p1 = BR.linear1(torch.cat([z_rec[t], h.detach()], 1))
            out["br"].append(BR.linear2(p1 * relu_mask(p1, g("vhid_r")[t] > 0)))
    return out


def cpu_tape(models, fl, x, desc, n, seed=0):
    """A stand-in for the engine's tape that needs no GPU: the conversation through cpu_ref's layers in float64 without a
    graph, bits sampled from seeded uniforms (binary) or the logits themselves (continuous)."""
    S, Rc, BS, BR = (_double(models[k]) for k in ("sender", "receiver", "baseline_sen", "baseline_rec"))
    x64, d64 = torch.as_tensor(x).double(), torch.as_tensor(desc).double()
    B, R, W = x64.shape[0], fl.rec_hidden, fl.rec_w_dim
    rs = np.random.RandomState(seed)
    tp = {k: [] for k in ("z", "w", "vA", "vhid_s", "vhid_r")}
    with torch.no_grad():
        Wy1, by1 = Rc.y1.weight, Rc.y1.bias
        tp_vCd = d64 @ Wy1[:, R:].t() + by1
        h = torch.zeros(B, R, dtype=torch.float64)
        h_x = S.image_layer(x64)
        w_in = None
        for t in range(n):
            c = torch.sigmoid(S.code_bias.view(1, -1)).expand(B, W) if t == 0 else w_in
            feats = S.binary_layer(torch.tanh(h_x + S.code_layer(c)))
            z = (torch.from_numpy(rs.rand(B, W)) < torch.sigmoid(feats)).double() if fl.use_binary else feats
            zr = torch.full((B, W), float(fl.first_rec), dtype=torch.float64) if t == 0 else w_in
            h = Rc.rnn(z, h)
            pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, -1, R)
            y = Rc.y2(torch.relu(pre).view(-1, R)).view(B, -1)
            ws = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(F.softmax(y, dim=1) @ d64)))
            w_in = (torch.from_numpy(rs.rand(B, W)) < torch.sigmoid(ws)).double() if fl.use_binary else ws
            tp["z"].append(z); tp["w"].append(w_in); tp["vA"].append(h @ Wy1[:, :R].t())
            tp["vhid_s"].append(torch.relu(BS.linear1(torch.cat([h_x, zr], 1))))
            tp["vhid_r"].append(torch.relu(BR.linear1(torch.cat([z, h], 1))))
    tp = {k: torch.stack(v) for k, v in tp.items()}
    tp["vCd"] = tp_vCd
    return tp


def grads_of(models, agents=CHANNEL_AGENTS):
    return {a: {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in models[a].named_parameters()}
            for a in agents}
