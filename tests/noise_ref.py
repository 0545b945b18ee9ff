"""Test-side reference of Gaussian message noise on continuous messages (include/mmg.h: mmg_set_message_noise): the library's normal
draws restated in float64 numpy over the Philox rounds of tests/philox_ref.py, and the CPU oracle (oracle/cpu_ref) with the Sender's
and the Receiver's returned messages replaced by message + sigma * n[t].  The oracle itself is not edited: the wrappers sit on the
forward methods of the agents they are handed (the pattern of tests/flipout_ref.py).  No GPU import here.

Shapes of tests/test_channel_noise_{cpu,gpu}.py (CASES), all with continuous messages:
    G256  the odd-sized shape of the generic per-sample family (H 100, W 50, R 128, 7 classes, 5 samples, T 3): k_conversation_noise<256>,
          every strided `n < W` loop has a tail
    G512  tests/generic_inst.py's W512 shape (H 260, W 253: H * W >= 65 536, five samples): k_conversation_noise<512>
    M     config 1's agents, Fixed, 100 classes, 32 samples, T 4: two tiles of k_conversation_mc3_noise
    A     config 1's agents, Adaptive stopping, 30 classes, 16 samples, T 4: k_conversation_noise<256> with sampled stop bits
    MA    M with Adaptive stopping (the training minibatch on k_conversation_mc3_noise with samples that stop early)
The data seeds of A were searched on the CPU oracle; tests/test_channel_noise_cpu.py asserts what they reach."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import channel_ref, common, generic_inst as gi, philox_ref

TRAIN_STREAMS, EVAL_STREAMS = (7, 8), (9, 10)
SIGMA_SEN, SIGMA_REC = 0.3, 0.2
EVAL_SEED = 77
NO_ENTROPY = dict(entropy_rec=None, entropy_sen=None, entropy_s=None)
C1 = dict(learning_rate=1e-4, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6, use_binary=False, **NO_ENTROPY)
ODD = dict(C1, img_h_dim=100, rec_w_dim=50, sender_out_dim=50, rec_hidden=128)
SKIP = ("y2.bias", ".bs", ".br")        # as every continuous case: the baselines are not trained, y2.bias walks (common.compare_packed)


def _meta(flags_kw, n_classes, batch, seed_weights=11, seed_data=12, seed_uniforms=13):
    meta = dict(cpu_ref.Flags(**flags_kw).__dict__)
    meta.update(n_classes=n_classes, batch=batch, batch_size=batch, n_minibatches=1, seed_weights=seed_weights,
                seed_data=seed_data, seed_uniforms=seed_uniforms)
    return meta


# searched (12.. upwards): samples stop at the first step and samples run to the last one (test_channel_noise_cpu.py)
A_SEED_DATA, MA_SEED_DATA = 12, 22
CASES = {
    "G256": lambda: _meta(dict(ODD, fixed_exchange=True, max_exchange=3), 7, 5),
    "G512": lambda: gi.plain_meta("W512", "continuous", seed=gi.SEEDS["plain", "continuous"]),
    "M": lambda: _meta(dict(C1, fixed_exchange=True, max_exchange=4), 100, 32),
    "A": lambda: _meta(dict(C1, fixed_exchange=False, max_exchange=4), 30, 16, seed_data=A_SEED_DATA),
    "MA": lambda: _meta(dict(C1, fixed_exchange=False, max_exchange=4), 100, 32, seed_data=MA_SEED_DATA),
}
# the conversation kernel's profiling scope per case (a noise handle), and what a handle of that shape must not run
SCOPES = {"G256": "k_conversation_noise", "G512": "k_conversation_noise", "M": "k_conversation_mc3_noise", "A": "k_conversation_noise",
          "MA": "k_conversation_mc3_noise"}
ADAPTIVE = ("A", "MA")


def meta_of(case):
    return CASES[case]()


def dims(meta):
    return meta["max_exchange"], meta["batch"], meta["rec_w_dim"]


# ------------------------------------------------------------------ the draws
def philox_pair(key, e, c1, stream):
    """The first two output words of the Philox4x32-10 block with counter (e, c1, stream, 0) and the 64-bit key: the rounds of
    tests/philox_ref.philox_uniform, which keeps the first word only."""
    e = np.asarray(e, np.uint32)
    x0, x1 = e.copy(), np.full_like(e, c1, dtype=np.uint32)
    x2, x3 = np.full_like(e, stream, dtype=np.uint32), np.zeros_like(e, dtype=np.uint32)
    k0, k1 = np.uint32(key & 0xFFFFFFFF), np.uint32((key >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = philox_ref.M0 * x0.astype(np.uint64)
            p1 = philox_ref.M1 * x2.astype(np.uint64)
            y0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ x1 ^ k0
            y1 = p1.astype(np.uint32)
            y2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ x3 ^ k1
            y3 = p0.astype(np.uint32)
            x0, x1, x2, x3 = y0, y1, y2, y3
            k0, k1 = np.uint32(k0 + philox_ref.W0), np.uint32(k1 + philox_ref.W1)
    return x0, x1


def philox_normal(key, e, c1, stream):
    """(n, x0, x1): the Box-Muller normal of the block's first two words in float64 -- u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1],
    u2 = (x1 >> 8) 2^-24 in [0, 1), n = sqrt(-2 ln u1) cos(2 pi u2) -- and the words themselves."""
    x0, x1 = philox_pair(key, e, c1, stream)
    u1 = ((x0 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (x1 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2), x0, x1


def noise_fields(key, c1, T, B_global, W, streams=TRAIN_STREAMS, batch_offset=0, batch=None):
    """(n_z, n_w) [T, batch, W] float64: n[t, b, j] = philox_normal(key, e, c1, stream)[0] at the element index of the Bernoulli
    streams, e = (t * B_global + batch_offset + b) * W + j."""
    batch = B_global - batch_offset if batch is None else batch
    t = np.arange(T)[:, None, None]; b = (batch_offset + np.arange(batch))[None, :, None]; j = np.arange(W)[None, None, :]
    e = ((t * B_global + b) * W + j).astype(np.uint32)
    return philox_normal(key, e, c1, streams[0])[0], philox_normal(key, e, c1, streams[1])[0]


# ------------------------------------------------------------------ the oracle's agents behind the channel
def noise_agents(models, n_z, n_w, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC):
    """Make models["sender"] return (z + sigma_sen n_z[t], probs) and models["receiver"] (s, (w + sigma_rec n_w[t], probs), y).
    The sender is told t; the receiver wrapper counts its calls since the last reset_state() (exchange() resets both agents
    before a conversation)."""
    sender, receiver = models["sender"], models["receiver"]
    nz, nw = torch.as_tensor(np.asarray(n_z, np.float64)), torch.as_tensor(np.asarray(n_w, np.float64))
    s_forward, r_forward, r_reset = sender.forward, receiver.forward, receiver.reset_state
    state = {"t": 0}

    def sen(x, w, g, t):
        z, p = s_forward(x, w, g, t)
        return z + (sigma_sen * nz[t]).to(z.dtype), p

    def rec(*args, **kw):
        s, (w, pw), y = r_forward(*args, **kw)
        t = state["t"]; state["t"] += 1
        return s, (w + (sigma_rec * nw[t]).to(w.dtype), pw), y

    def reset():
        state["t"] = 0
        return r_reset()
    sender.forward, receiver.forward, receiver.reset_state = sen, rec, reset
    return models


def wrap_of(meta, key=0, c1=1, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC, streams=TRAIN_STREAMS):
    """The wrapper of gi.wrapped_agents for the noise minibatch `c1` draws under `key` (common.hip_train_case trains with seed 0,
    and the first minibatch of a handle draws with counter 1)."""
    T, B, W = dims(meta)
    n_z, n_w = noise_fields(key, c1, T, B, W, streams)
    return lambda models: noise_agents(models, n_z, n_w, sigma_sen, sigma_rec)


def build(meta, n_z, n_w, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC, rng=None):
    """The oracle's four agents with the seeded weights of `meta`, wrapped."""
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl, rng=rng)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    return noise_agents(models, n_z, n_w, sigma_sen, sigma_rec), fl


def conversation(meta, n_z, n_w, train, uniforms=None, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC, mask=None, i=0):
    """Every step of every sample (what the GPU's run-all pass stores) of minibatch `i` of `meta` over the noisy channel.  mask: a
    [W] corruption mask applied to what the sender returned, |z - m| (model.py:813-820), as exchange() applies it."""
    tape = cpu_ref.UniformTape(*uniforms) if uniforms is not None else None
    models, fl = build(meta, n_z, n_w, sigma_sen, sigma_rec, rng=tape)
    if mask is not None:
        s_forward, m = models["sender"].forward, torch.as_tensor(np.asarray(mask, np.float32)).view(1, -1)

        def corrupted(x, w, g, t):
            z, p = s_forward(x, w, g, t)
            return (z - m).abs(), p
        models["sender"].forward = corrupted
    x, target, desc, _ = common.case_inputs(meta, i)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=train, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], models["baseline_sen"], models["baseline_rec"], args, fl)
    st = lambda v: torch.stack(v).numpy()
    return dict(s=st(s[1]).reshape(len(y), -1), ps=st(s[2]).reshape(len(y), -1), z=st(sen_w[0]), w=st(rec_w[0]), y=st(y))


def train_minibatch(meta, n_z, n_w, uniforms, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC):
    """cpu_ref.train_minibatch of minibatch 0 of `meta` on wrapped agents, packed as common.oracle_train_case packs it."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms)
    models, fl = build(meta, n_z, n_w, sigma_sen, sigma_rec, rng=tape)
    optimizers = cpu_ref.build_optimizers(models, fl)
    x, target, desc, _ = common.case_inputs(meta, 0)
    res = cpu_ref.train_minibatch(models, optimizers, torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc), fl)
    return cpu_ref.pack_train(res, models, prefix="mb0."), res


def separated_uniforms(meta, n_z, n_w, margin=1e-4):
    """common.separate_draws restated for wrapped agents: the seeded uniforms of minibatch 0 with every stop draw (the only
    Bernoulli draws of continuous mode) that lies within `margin` of its probability moved to p -/+ margin on the side it was
    on -- the sampled bits, hence the trajectory and every later probability, stay what they were."""
    _, _, _, us = common.case_inputs(meta, 0)
    us = [np.array(u, copy=True) for u in us]
    packed, _ = train_minibatch(meta, n_z, n_w, us)
    n = int(packed["mb0.n_steps"])
    for key, u in zip(("sen_probs", "s_probs", "rec_probs"), us):
        p = np.asarray(packed["mb0." + key], dtype=np.float64)
        if not p.size:
            continue
        v = u[:n].reshape(p.shape)                                    # a view: edits land in u
        close = np.abs(v - p) < margin
        v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
        np.clip(v, 0.0, 0.99999994, out=v)
    return tuple(us)


def stop_steps(packed):
    """(t* per sample, executed steps n) of the packed minibatch: the first step whose running-minimum mask is 0."""
    n = int(packed["mb0.n_steps"])
    masks = np.asarray(packed["mb0.s_masks"]).reshape(n + 1, -1)
    stopped = masks[1:] == 0
    assert stopped.any(0).all()
    return stopped.argmax(0), n


# ------------------------------------------------------------------ float64, for the VJP comparisons
def f64_outputs(models, fl, x, desc, tp, n, n_z, n_w, sigma_sen=SIGMA_SEN, sigma_rec=SIGMA_REC, channel=False):
    """tests/channel_ref.f64_outputs for continuous messages over the noisy channel: the differentiable outputs "sen" / "w" are the
    noisy messages logits + sigma * n[t], the noise a constant of the graph.  channel=False: every message crossing between the
    agents is the recorded (noisy) one, a constant; channel=True: it crosses with its graph, d message / d logits = 1."""
    assert not fl.use_binary
    S, Rc = (channel_ref._double(models[k]) for k in ("sender", "receiver"))
    x64, d64 = torch.as_tensor(x).double(), torch.as_tensor(desc).double()
    B, D, R = x64.shape[0], d64.shape[0], fl.rec_hidden
    g = lambda k: tp[k].detach().double().cpu()
    z_rec, w_rec, vA, vCd = g("z"), g("w"), g("vA"), g("vCd")
    nz, nw = torch.as_tensor(np.asarray(n_z, np.float64)), torch.as_tensor(np.asarray(n_w, np.float64))
    out = {k: [] for k in ("sen", "y", "ps", "w")}
    h = torch.zeros(B, R, dtype=torch.float64)
    w_in = None
    for t in range(n):
        h_x = S.image_layer(x64)
        h_w = S.code_layer(torch.sigmoid(S.code_bias.view(1, -1))).expand(B, fl.img_h_dim) if t == 0 else S.code_layer(w_in)
        z = S.binary_layer(torch.tanh(h_x + h_w)) + sigma_sen * nz[t]
        out["sen"].append(z)
        h = Rc.rnn(z if channel else z_rec[t], h)
        out["ps"].append(torch.sigmoid(Rc.s(h)))
        pre = Rc.y1(cpu_ref.build_inp(h, d64)).view(B, D, R)
        on = channel_ref.relu_mask(pre, (vA[t][:, None, :] + vCd[None, :, :]) > 0).double()
        y = Rc.y2((pre * on).view(B * D, R)).view(B, -1)
        out["y"].append(y)
        dbar = F.softmax(y, dim=1).detach() @ d64
        w = Rc.w(torch.tanh(Rc.w_h(h) + Rc.w_d(dbar))) + sigma_rec * nw[t]
        out["w"].append(w)
        w_in = w if channel else w_rec[t]
    return out
