"""TEST INFRASTRUCTURE for the training controls (include/mmg.h: mmg_set_trainable, mmg_set_learning_rate, mmg_set_entropy): the
reference loop under a schedule of controls, on the CPU oracle and on the engine.

Oracle side: cpu_ref.train_minibatch with an `optimizers` dict in which a frozen agent's entry is FrozenOptimizer -- zero_grad()
passes through, step() does nothing (train_minibatch's _update calls only those two) -- i.e. model.py:1307-1330 with
optimizer.step() of a frozen agent not called.  New learning rates go into the optimizers' param_groups, new entropy weights into
the flags object, between minibatches.

A schedule is a list with one dict per minibatch: frozen (agent names), lr, entropy (dict of entropy_s / entropy_sen /
entropy_rec); a key that is missing keeps what the minibatch before had."""
import numpy as np
import torch

from oracle import cpu_ref
from tests import common

AGENTS = ("receiver", "sender", "baseline_rec", "baseline_sen")
OPT_KEY = dict(receiver="optimizer_rec", sender="optimizer_sen", baseline_rec="optimizer_bas_rec", baseline_sen="optimizer_bas_sen")
ATOL, RTOL = 1e-4, 1e-3          # common.assert_parity's: what the families' oracle tests (test_hip_parity / test_hip_configs) gate with
# what a fused step guarantees on the tape (tests/test_hip_parity.py: FUSED_KEEP)
FUSED_KEEP = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")
SKIP = (".p.receiver.y2.bias",)  # an exact-zero gradient whose rounding noise the optimizers turn into steps (common.compare_packed)

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01,
          entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6)
# tests/test_autograd_gpu.py::FAMILIES -- one shape per kernel family: (flags, classes, batch)
FAMILIES = {
    "fast_c2": (dict(C1, batch_size=16), 30, 16),
    "mc_binary": (dict(C1, batch_size=16), 100, 16),
    "mc_continuous": (dict(C1, batch_size=16, use_binary=False, fixed_exchange=True, max_exchange=4,
                           entropy_rec=None, entropy_sen=None, entropy_s=None), 100, 16),
    "tile": (dict(C1, batch_size=16, img_h_dim=128, rec_w_dim=64, sender_out_dim=64, max_exchange=5), 30, 16),
    "rc_r256": (dict(C1, batch_size=16, img_h_dim=1024, rec_w_dim=64, sender_out_dim=64, rec_hidden=256, max_exchange=4), 30, 16),
    "odd_generic": (dict(C1, batch_size=5, img_h_dim=100, rec_w_dim=50, sender_out_dim=50, rec_hidden=128, max_exchange=3,
                         fixed_exchange=True), 7, 5),
}
MASKS = {"sender_frozen": ("sender",), "receiver_frozen": ("receiver",), "baselines_frozen": ("baseline_rec", "baseline_sen")}


class FrozenOptimizer(object):
    """A frozen agent's optimizer in the oracle loop: its gradients are cleared and formed as ever, its step is not taken."""

    def __init__(self, opt):
        self.opt = opt

    def zero_grad(self, *a, **kw):
        return self.opt.zero_grad(*a, **kw)

    def step(self, *a, **kw):
        return None


def family_meta(family, n_minibatches=1, **flags_over):
    kw, n_classes, batch = FAMILIES[family]
    meta = dict(cpu_ref.Flags(**dict(kw, **flags_over)).__dict__)
    meta.update(n_classes=n_classes, batch=batch, batch_size=batch, n_minibatches=n_minibatches, seed_weights=11, seed_data=12,
                seed_uniforms=13)
    return meta


def trained_agents(meta):
    return AGENTS if meta["use_binary"] else ("receiver",)


def resolve(schedule, meta):
    """The schedule with every key stated: [(frozen tuple, lr, {entropy_*: value})] per minibatch."""
    cur = dict(frozen=(), lr=meta["learning_rate"], entropy={k: meta[k] for k in ("entropy_s", "entropy_sen", "entropy_rec")})
    out = []
    for ctl in schedule:
        cur = dict(frozen=tuple(ctl.get("frozen", cur["frozen"])), lr=ctl.get("lr", cur["lr"]),
                   entropy=dict(cur["entropy"], **ctl.get("entropy", {})))
        out.append(cur)
    return out


def oracle_loop(name, meta, schedule, snapshots=None):
    """The reference loop under `schedule` -> packed dict ("mb<i>." prefixes, cpu_ref.pack_train).  A frozen agent's gradients are
    left out of the packed result (the library leaves zeros there; its parameters are compared bit for bit with their values
    before the step instead).  snapshots: a list that receives, per minibatch, (params and optimizer state before, after)."""
    fl = common.flags_from_meta(meta)
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape()
    models = cpu_ref.build_agents(fl, rng=tape)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    optimizers = cpu_ref.build_optimizers(models, fl)

    def snap():
        return {a: dict(params={k: v.detach().clone() for k, v in models[a].state_dict().items()},
                        state=[{k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizers[OPT_KEY[a]].state.get(p, {}).items()}
                               for p in models[a].parameters()]) for a in AGENTS}
    out = {}
    for i, ctl in enumerate(resolve(schedule, meta)):
        for opt in optimizers.values():
            for group in opt.param_groups:
                group["lr"] = ctl["lr"]
        for k, v in ctl["entropy"].items():
            setattr(fl, k, v)
        opts = {OPT_KEY[a]: FrozenOptimizer(optimizers[OPT_KEY[a]]) if a in ctl["frozen"] else optimizers[OPT_KEY[a]] for a in AGENTS}
        x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i, name)
        tape.u = {"z": u_z, "s": u_s, "w": u_w}
        tape.t = {"z": 0, "s": 0, "w": 0}
        before = snap() if snapshots is not None else None
        res = cpu_ref.train_minibatch(models, opts, torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc), fl)
        if snapshots is not None:
            snapshots.append((before, snap()))
        for a in ctl["frozen"]:
            res["grads"].pop(a, None)
        out.update(cpu_ref.pack_train(res, models, prefix="mb%d." % i))
    return out


def wrapped_oracle_minibatch(wref, m, uniforms, frozen):
    """Minibatch 0 of an attention case on the oracle with its wrapped agent (wref: tests/desc_attn_ref or tests/visual_attn_ref --
    their train_minibatch[es], with FrozenOptimizer in the frozen agents' places), packed as oracle_loop packs it."""
    torch.manual_seed(0)
    tape = cpu_ref.UniformTape(*uniforms)
    models, fl = wref.build(m, rng=tape)
    optimizers = cpu_ref.build_optimizers(models, fl)
    opts = {OPT_KEY[a]: FrozenOptimizer(optimizers[OPT_KEY[a]]) if a in frozen else optimizers[OPT_KEY[a]] for a in AGENTS}
    x, target, desc = wref._inputs(m)
    res = cpu_ref.train_minibatch(models, opts, x, target, desc, fl)
    for a in frozen:
        res["grads"].pop(a, None)
    return cpu_ref.pack_train(res, models, prefix="mb0.")


def losses_f64(name, meta, schedule, want, snaps_oracle, params_gpu):
    """common.oracle_losses_f64 for a loop under `schedule` (each minibatch with ITS entropy weights): the six losses in float64 on
    the discrete trajectory of the fp32 oracle run `want`, from the parameters the GPU held before minibatch i and from those the
    oracle held -- they differ by the two implementations' own update noise, which RMSprop and Adam turn into steps of the size
    of the learning rate.  Returns {"mb<i>.losses": (exact at the GPU's parameters, exact at the oracle's)} for
    common.compare_packed(f64=...): each implementation against the exact value of its own forward pass."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    keys6 = ("nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen", "loss_bas_rec", "loss_bas_sen")
    try:
        out = {}
        for i, ctl in enumerate(resolve(schedule, meta)):
            fl = common.flags_from_meta(meta)
            for k, v in ctl["entropy"].items():
                setattr(fl, k, v)
            x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i, name)
            u = {"z": np.array(u_z, np.float64), "s": np.array(u_s, np.float64), "w": np.array(u_w, np.float64)}
            if fl.use_binary:
                for kind, key in (("z", "sen_feats"), ("s", "s_feats"), ("w", "rec_feats")):
                    bits = np.asarray(want["mb%d.%s" % (i, key)])
                    n = bits.shape[0]
                    u[kind][:n] = np.where(bits.reshape(u[kind][:n].shape) != 0, 0.0, 1.0)
            both = []
            for params in ((params_gpu[i], snaps_oracle[i][0]) if i > 0 else (snaps_oracle[i][0],)):
                tape = cpu_ref.UniformTape()
                models = cpu_ref.build_agents(fl, rng=tape)
                for a, m in models.items():
                    m.double()
                    src = params[a]["params"] if "params" in params[a] else params[a]
                    m.load_state_dict({k: torch.as_tensor(v).double() for k, v in src.items()})
                tape.u = {k: v.copy() for k, v in u.items()}
                tape.t = {"z": 0, "s": 0, "w": 0}
                res = cpu_ref.train_minibatch(models, cpu_ref.build_optimizers(models, fl), torch.from_numpy(x).double(),
                                              torch.from_numpy(target), torch.from_numpy(desc).double(), fl, update=False)
                assert int(res["n_steps"]) == int(want["mb%d.n_steps" % i]), "the float64 re-run left the fp32 run's trajectory"
                both.append(np.array([float(res[k].detach()) for k in keys6], np.float64))
            out["mb%d.losses" % i] = (both[0], both[-1])
        return out
    finally:
        torch.set_default_dtype(old)


def separate(name, meta, schedule, margin=1e-4):
    """common.separate_draws for a loop under `schedule`: the oracle runs once on the seeded uniforms, every uniform within
    `margin` of its probability moves to the margin on the side it was on -- no bit, hence no later probability, changes -- and
    the adjusted arrays become the inputs of case `name`."""
    common.U_OVERRIDES.pop(name, None)
    packed = oracle_loop(name, meta, schedule)
    adjusted = []
    for i in range(len(schedule)):
        _, _, _, us = common.case_inputs(meta, i, None)
        us = [np.array(u, copy=True) for u in us]
        n = int(packed["mb%d.n_steps" % i])
        for key, u in zip(("sen_probs", "s_probs", "rec_probs"), us):
            p = np.asarray(packed["mb%d.%s" % (i, key)], dtype=np.float64)
            if not p.size:
                continue
            v = u[:n].reshape(p.shape)
            close = np.abs(v - p) < margin
            v[close] = np.where(v[close] < p[close], p[close] - margin, p[close] + margin).astype(v.dtype)
            np.clip(v, 0.0, 0.99999994, out=v)
        adjusted.append(tuple(us))
    common.U_OVERRIDES[name] = lambda i, u_z, u_s, u_w: adjusted[i]
    return adjusted


# ----------------------------------------------------------------------------------------------
# engine side (GPU tests)
# ----------------------------------------------------------------------------------------------
def device_inputs(meta, i, name, dev, lo=0, n=None):
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i, name)
    n = meta["batch"] if n is None else n
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (d(x[lo:lo + n]), d(target[lo:lo + n]), d(desc)), (d(u_z[:, lo:lo + n]), d(u_s[:, lo:lo + n, 0]), d(u_w[:, lo:lo + n]))


def apply_controls(eng, ctl, meta):
    eng.set_trainable([a for a in AGENTS if a not in ctl["frozen"]])
    eng.set_learning_rate(ctl["lr"])
    eng.set_entropy(**{k: v for k, v in ctl["entropy"].items() if v is not None})


def frozen_problems(eng, frozen, before, label):
    """A frozen agent after a step: parameters and optimizer state bit-identical to `before` (flat_params, opt_state clones), its
    slice of the gradient buffer all zeros."""
    n, problems = eng.n_params, []
    for a in frozen:
        lo, hi = eng.agent_range[a]
        if not torch.equal(eng.flat_params[lo:hi], before[0][lo:hi]):
            problems.append("%s: parameters of the frozen %s moved" % (label, a))
        if not (torch.equal(eng.opt_state[lo:hi], before[1][lo:hi]) and torch.equal(eng.opt_state[n + lo:n + hi], before[1][n + lo:n + hi])):
            problems.append("%s: optimizer state of the frozen %s moved" % (label, a))
        if bool(eng.flat_grads[lo:hi].any()):
            problems.append("%s: gradient slice of the frozen %s is not zero" % (label, a))
    return problems


def hip_loop(name, meta, schedule, fused=True, eng=None, inputs=None):
    """The same loop through the C-ABI: mmg_train_step (fused) or forward / loss_stats / backward / clip_step (phased), the controls
    set before each minibatch.  eng / inputs: another engine than common.make_engine's (an attention handle) and its device inputs
    ((x, target, desc), (u_z, u_s, u_w)) of minibatch i.  Returns (packed dict, engine, problems of the frozen agents)."""
    fl = common.flags_from_meta(meta)
    eng = eng or common.make_engine(meta)
    out, problems = {}, []
    eng.param_snapshots = []                                    # the parameters every minibatch starts from (losses_f64)
    for i, ctl in enumerate(resolve(schedule, meta)):
        apply_controls(eng, ctl, meta)
        (xd, td, dd), u = inputs(i) if inputs is not None else device_inputs(meta, i, name, eng.device)
        before = (eng.flat_params.clone(), eng.opt_state.clone())
        eng.param_snapshots.append({a: {k: v.detach().cpu().clone() for k, v in eng.params[a].items()} for a in AGENTS})
        if fused:
            eng.train_step(xd, td, dd, *u)
        else:
            eng.forward(xd, td, dd, *u, train=True, run_all=True)
            eng.loss_stats()
            eng.backward(xd, td, dd)
        res = common.engine_result(eng, fl)
        grads, norms = {}, {}
        for a in trained_agents(meta):
            if a in ctl["frozen"]:
                continue
            grads[a] = {k: v.detach().cpu().clone() for k, v in eng.grads[a].items()}
            lo, hi = eng.agent_range[a]
            norms[a] = float(eng.flat_grads[lo:hi].double().norm())
        res["grads"], res["grad_norms"] = grads, norms
        if not fused:
            eng.clip_step()
        torch.cuda.synchronize()
        problems += frozen_problems(eng, [a for a in ctl["frozen"] if a in trained_agents(meta)], before, "mb%d" % i)
        models = {a: common._SD({k: v.detach().cpu() for k, v in eng.params[a].items()}) for a in AGENTS}
        out.update(cpu_ref.pack_train(res, models, prefix="mb%d." % i))
    return out, eng, problems


def pick(packed, fused):
    return {k: v for k, v in packed.items() if any(t in k for t in FUSED_KEEP)} if fused else packed
