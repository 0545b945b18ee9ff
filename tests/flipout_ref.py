"""Test-side reference of random message flips (-flipout_sen / -flipout_rec / -flipout_dev, model.py:233-234, 467-468, 554-568):
the CPU oracle (oracle/cpu_ref) with the Sender's and the Receiver's returned bits replaced by |bits - m|, m the flip masks the
library draws (include/mmg.h: mmg_set_message_flipout) restated with tests/philox_ref.  The oracle itself is not edited: the
wrappers sit on the forward methods of the agents they are handed (the pattern of tests/corrupt_ref.py)."""
import numpy as np
import torch

from oracle import cpu_ref
from tests import common, philox_ref

TRAIN_STREAMS, EVAL_STREAMS = (3, 4), (5, 6)


def flip_masks(key, c1, T, B_global, W, p_sen, p_rec, streams=TRAIN_STREAMS, batch_offset=0, batch=None):
    """(m_z, m_w) [T, batch, W] float32 0 / 1: m[t, b, j] = 1 iff philox_uniform(key, e, c1, stream) < p in float32, e the element
    index of the Bernoulli streams 0 / 2, (t * B_global + batch_offset + b) * W + j.  p None: that message is not flipped."""
    batch = B_global - batch_offset if batch is None else batch
    t = np.arange(T)[:, None, None]; b = (batch_offset + np.arange(batch))[None, :, None]; j = np.arange(W)[None, None, :]
    e = ((t * B_global + b) * W + j).astype(np.uint32)

    def one(p, stream):
        if p is None:
            return np.zeros(e.shape, np.float32)
        return (philox_ref.philox_uniform(key, e, c1, stream) < np.float32(p)).astype(np.float32)
    return one(p_sen, streams[0]), one(p_rec, streams[1])


def flip_agents(models, m_z, m_w):
    """Make models["sender"] return (|z - m_z[t]|, probs) and models["receiver"] (s, (|w - m_w[t]|, probs), y): what the
    reference's modules return under -flipout_sen / -flipout_rec.  The sender is told t; the receiver wrapper counts its calls
    since the last reset_state() (exchange() resets both agents before a conversation).  Probabilities stay the agents' own."""
    sender, receiver = models["sender"], models["receiver"]
    mz, mw = torch.as_tensor(np.asarray(m_z, np.float32)), torch.as_tensor(np.asarray(m_w, np.float32))
    s_forward, r_forward, r_reset = sender.forward, receiver.forward, receiver.reset_state
    state = {"t": 0}

    def sen(x, w, g, t):
        z, p = s_forward(x, w, g, t)
        return (z - mz[t].to(z.dtype)).abs(), p

    def rec(*args, **kw):
        s, (w, pw), y = r_forward(*args, **kw)
        t = state["t"]; state["t"] += 1
        return s, ((w - mw[t].to(w.dtype)).abs(), pw), y

    def reset():
        state["t"] = 0
        return r_reset()
    sender.forward, receiver.forward, receiver.reset_state = sen, rec, reset
    return models


def build(meta, m_z, m_w, rng=None):
    """The oracle's four agents with the seeded weights of `meta`, wrapped."""
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl, rng=rng)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    return flip_agents(models, m_z, m_w), fl


def conversation(meta, m_z, m_w, train, uniforms=None):
    """Every step of every sample (what the GPU's run-all pass stores) of minibatch 0 of `meta` with flipped messages."""
    tape = cpu_ref.UniformTape(*uniforms) if uniforms is not None else None
    models, fl = build(meta, m_z, m_w, rng=tape)
    x, target, desc, _ = common.case_inputs(meta, 0)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=train, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], models["baseline_sen"], models["baseline_rec"], args, fl)
    st = lambda v: torch.stack(v).numpy()
    return dict(s=st(s[1]), ps=st(s[2]), z=st(sen_w[0]), pz=st(sen_w[1]), w=st(rec_w[0]), pw=st(rec_w[1]), y=st(y))


def train_minibatch(meta, m_z, m_w, uniforms):
    """cpu_ref.train_minibatch of minibatch 0 of `meta` on wrapped agents, packed as common.oracle_train_case packs it."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms)
    models, fl = build(meta, m_z, m_w, rng=tape)
    optimizers = cpu_ref.build_optimizers(models, fl)
    x, target, desc, _ = common.case_inputs(meta, 0)
    res = cpu_ref.train_minibatch(models, optimizers, torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc), fl)
    return cpu_ref.pack_train(res, models, prefix="mb0."), res


def separated_uniforms(meta, m_z, m_w, margin=1e-4):
    """common.separate_draws restated for wrapped agents: the seeded uniforms of minibatch 0 with every draw that lies within
    `margin` of its probability moved to p -/+ margin on the side it was on -- the sampled bits, hence the trajectory and every
    later probability, stay what they were; what goes is the coin two correct fp32 implementations toss on a near-tie."""
    _, _, _, us = common.case_inputs(meta, 0)
    us = [np.array(u, copy=True) for u in us]
    packed, _ = train_minibatch(meta, m_z, m_w, us)
    n = int(packed["mb0.n_steps"])
    for key, u in zip(("sen_probs", "s_probs", "rec_probs"), us):
        p = np.asarray(packed["mb0." + key], dtype=np.float64)
        v = u[:n].reshape(p.shape)                                    # a view: edits land in u
        close = np.abs(v - p) < margin
        v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
        np.clip(v, 0.0, 0.99999994, out=v)
    return tuple(us)
