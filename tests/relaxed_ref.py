"""Float64 reference of one training conversation with relaxed messages (include/mmg.h: mmg_set_message_relaxation); test side only.

f64_outputs is tests/channel_ref.py::f64_outputs for binary messages with one more argument, relax = (tau_sen, tau_rec, hard).  Per
message element, with lz the float64 logit and u the recorded uniform of its Bernoulli draw:

    u'   = min(max(u, 2^-24), 1 - 2^-24)
    soft = sigmoid((lz + log(1 - u') - log(u')) / tau)
    hard == 0:  message = soft
    hard == 1:  message = soft + (bit - soft).detach(), the bits taken from the tape

The reference forms soft from its OWN logits; the stop bits (they decide only how many steps a conversation runs) and, in hard mode,
the message bits come from the tape.  ReLU units within 1e-4 of zero take the side of the recorded forward where the tape has one
(vA, vCd: left by a VJP), as in channel_ref.  softmax(y) inside dbar, data and desc are constants.  The baselines are not part of the
relaxed graph (they are REINFORCE machinery): no bs / br here.

conversation() is the stand-in for the engine's tape that needs no GPU: the same loop without a graph, the bits and the stop bits
drawn from the uniforms.  uniforms_of_cpu_tape() replays the draws channel_ref.cpu_tape() samples its bits from, so that its
stand-in is the hard relaxed conversation of exactly those uniforms.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests.channel_ref import _double, _frozen, relu_mask

U_MIN = 2.0 ** -24


def soft_sample(logit, u, tau):
    uc = torch.clamp(torch.as_tensor(u).double(), U_MIN, 1.0 - U_MIN)
    return torch.sigmoid((logit + torch.log(1.0 - uc) - torch.log(uc)) / tau)


def uniforms_of_cpu_tape(fl, batch, n, seed=0):
    """(u_z, u_w) [n, B, W] float64: the draws of channel_ref.cpu_tape(..., seed), in its order (z, then w, per step)."""
    rs = np.random.RandomState(seed)
    u_z, u_w = [], []
    for _ in range(n):
        u_z.append(rs.rand(batch, fl.rec_w_dim))
        u_w.append(rs.rand(batch, fl.rec_w_dim))
    return np.stack(u_z), np.stack(u_w)


def f64_outputs(models, fl, x, desc, tp, n, relax, uniforms, frozen=None):
    """uniforms: (u_z [T, B, W], u_w [T, B, W]) (a third entry in between, u_s, is accepted and ignored).  Returns per-step lists:
    sen / w (the probabilities pz / pw), y, ps, zs / ws (the soft values), z / wm (the messages with their graph)."""
    assert fl.use_binary, "relaxed messages are for binary messages"
    tau_sen, tau_rec, hard = relax
    u_z, u_w = uniforms[0], uniforms[-1]
    S, Rc = _double(models["sender"]), _double(models["receiver"])
    x64, d64 = torch.as_tensor(x).double(), torch.as_tensor(desc).double()
    B, D, R = x64.shape[0], d64.shape[0], fl.rec_hidden
    g = lambda k: tp[k].detach().double().cpu()
    z_rec, w_rec = (g("z"), g("w")) if hard else (None, None)
    sides = (g("vA"), g("vCd")) if "vA" in tp and "vCd" in tp else None
    out = {k: [] for k in ("sen", "y", "ps", "w", "zs", "ws", "z", "wm")}
    h = torch.zeros(B, R, dtype=torch.float64)
    w_in = None
    for t in range(n):
        h_x = S.image_layer(x64)
        if t == 0:
            h_w = S.code_layer(torch.sigmoid(S.code_bias.view(1, -1))).expand(B, fl.img_h_dim)
        else:
            h_w = S.code_layer(w_in)
        feats = S.binary_layer(torch.tanh(h_x + h_w))
        out["sen"].append(torch.sigmoid(feats))
        zs = soft_sample(feats, u_z[t], tau_sen)
        z_t = zs + (z_rec[t] - zs).detach() if hard else zs
        out["zs"].append(zs); out["z"].append(z_t)
        h = Rc.rnn(z_t, h)
        out["ps"].append(torch.sigmoid(Rc.s(h)))
        pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, D, R)
        rec_on = (sides[0][t][:, None, :] + sides[1][None, :, :]) > 0 if sides is not None else pre > 0
        on = _frozen(frozen, ("on", t), lambda: relu_mask(pre, rec_on).double())
        y = Rc.y2((pre * on).view(B * D, R)).view(B, -1)
        out["y"].append(y)
        dbar = _frozen(frozen, ("dbar", t), lambda: F.softmax(y, dim=1).detach() @ d64)
        lw = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(dbar)))
        out["w"].append(torch.sigmoid(lw))
        ws = soft_sample(lw, u_w[t], tau_rec)
        w_in = ws + (w_rec[t] - ws).detach() if hard else ws
        out["ws"].append(ws); out["wm"].append(w_in)
    return out


def conversation(models, fl, x, desc, uniforms, relax, n=None):
    """The relaxed training conversation in float64 without a graph, every sample through all n steps (the engine's run-all tape):
    dict of stacked [n, ...] tensors z, w (the messages), zs, ws, pz, pw, ps, s (stop bits: u_s < ps), y, bits_z, bits_w, vA and
    vCd [D, R].  uniforms: (u_z, u_s, u_w) as tests/common.py::case_inputs hands them out."""
    tau_sen, tau_rec, hard = relax
    u_z, u_s, u_w = (torch.as_tensor(np.asarray(u)).double() for u in uniforms)
    S, Rc = _double(models["sender"]), _double(models["receiver"])
    x64, d64 = torch.as_tensor(x).double(), torch.as_tensor(desc).double()
    B, R = x64.shape[0], fl.rec_hidden
    n = fl.max_exchange if n is None else n
    tp = {k: [] for k in ("z", "w", "zs", "ws", "pz", "pw", "ps", "s", "y", "bits_z", "bits_w", "vA")}
    with torch.no_grad():
        Wy1, by1 = Rc.y1.weight, Rc.y1.bias
        vCd = d64 @ Wy1[:, R:].t() + by1
        h = torch.zeros(B, R, dtype=torch.float64)
        h_x = S.image_layer(x64)
        w_in = None
        for t in range(n):
            c = torch.sigmoid(S.code_bias.view(1, -1)).expand(B, fl.rec_w_dim) if t == 0 else w_in
            lz = S.binary_layer(torch.tanh(h_x + S.code_layer(c)))
            pz, zs = torch.sigmoid(lz), soft_sample(lz, u_z[t], tau_sen)
            bz = (u_z[t] < pz).double()
            z = bz if hard else zs
            h = Rc.rnn(z, h)
            ps = torch.sigmoid(Rc.s(h))
            pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, -1, R)
            y = Rc.y2(torch.relu(pre).view(-1, R)).view(B, -1)
            lw = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(F.softmax(y, dim=1) @ d64)))
            pw, ws = torch.sigmoid(lw), soft_sample(lw, u_w[t], tau_rec)
            bw = (u_w[t] < pw).double()
            w_in = bw if hard else ws
            for k, v in (("z", z), ("w", w_in), ("zs", zs), ("ws", ws), ("pz", pz), ("pw", pw), ("ps", ps),
                         ("s", (u_s[t].view(B, 1) < ps).double()), ("y", y), ("bits_z", bz), ("bits_w", bw), ("vA", h @ Wy1[:, :R].t())):
                tp[k].append(v)
    tp = {k: torch.stack(v) for k, v in tp.items()}
    tp["vCd"] = vCd
    return tp


def executed_steps(s):
    """break_early (model.py:866): the conversation ends behind the first step after which no sample is still running."""
    alive = torch.ones(s.shape[1], 1, dtype=torch.float64)
    for t in range(s.shape[0]):
        alive = torch.min(alive, s[t].double())
        if float(alive.sum()) == 0:
            return t + 1
    return s.shape[0]


def output_nll(y, s, target):
    """The minibatch NLL of the reference (model.py:1261-1274) from the per-step class logits [n, B, D] and the stop bits [n, B, 1]:
    a sample's output step is the first one whose running stop mask falls to zero, else the last."""
    n, B = y.shape[0], y.shape[1]
    alive = torch.ones(B, dtype=torch.bool)
    tstar = torch.full((B,), n - 1, dtype=torch.int64)
    for t in range(n):
        stop = alive & (s[t].reshape(B) == 0)
        tstar[stop] = t
        alive = alive & ~stop
    outp = y[tstar, torch.arange(B)]
    return F.nll_loss(F.log_softmax(outp, dim=1), torch.as_tensor(target))
