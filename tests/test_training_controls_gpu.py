"""Training controls on the GPU (include/mmg.h: mmg_set_trainable, mmg_set_learning_rate, mmg_set_entropy): frozen agents and
retuned values on a live handle, against the reference loop with optimizer.step() of a frozen agent not called
(tests/training_controls_ref.py).

1. One step per kernel family and mask (sender frozen, receiver frozen, both baselines frozen; fused and phased): the trained
   agents match the oracle, the frozen ones are bit-identical with a zero gradient slice.
2. A five-minibatch schedule of masks, learning rates and entropy weights through mmg_train_step, under RMSprop and under Adam
   (whose bias correction counts each agent's own updates).
3. mmg_train_steps reads the controls of the moment: two calls with set_trainable in between == four train_step calls, bit for bit.
4. The data-parallel step with the sender frozen: two gloo ranks on one GPU == the single-process step; the frozen slice of the
   reduced gradient is zero on both ranks.
5. Freezing changes nothing of the forward pass.
6. Refusals and defaults.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import common, training_controls_ref as ref
from tests.test_plan_cpu import switches  # noqa: F401  (a fixture: every selection switch of the environment unset)

pytestmark = pytest.mark.gpu

_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _separated(name, meta, schedule, snapshots=None):
    """The case's uniforms with every draw at least 1e-4 from its probability (ref.separate), and the oracle's run on them."""
    def make():
        adjusted, snaps = ref.separate(name, meta, schedule), []
        return adjusted, ref.oracle_loop(name, meta, schedule, snapshots=snaps), snaps
    adjusted, want, snaps = _once(("oracle", name), make)
    common.U_OVERRIDES[name] = lambda i, u_z, u_s, u_w: adjusted[i]
    if snapshots is not None:
        snapshots.extend(snaps)
    return want


def _skip(meta):
    # continuous messages train the receiver only (model.py:1313): no baseline scores on the tape
    return ref.SKIP + (() if meta["use_binary"] else (".bs", ".br"))


# ------------------------------------------------------------------ 1. one step per family and mask
CASES = [(f, m) for f in sorted(ref.FAMILIES) for m in sorted(ref.MASKS) if ref.FAMILIES[f][0].get("use_binary", True) or m == "receiver_frozen"]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "phased"])
@pytest.mark.parametrize("family,mask", CASES)
def test_one_step_with_frozen_agents_matches_the_oracle(family, mask, fused):
    meta = ref.family_meta(family)
    name = "tc_%s_%s" % (family, mask)
    schedule = [dict(frozen=ref.MASKS[mask])]
    want = _separated(name, meta, schedule)
    got, eng, frozen_problems = ref.hip_loop(name, meta, schedule, fused=fused)
    assert not frozen_problems, "\n".join(frozen_problems)
    problems = common.compare_packed(ref.pick(got, fused), ref.pick(want, fused), atol=ref.ATOL, rtol=ref.RTOL, skip=_skip(meta),
                                     label="controls/%s/%s/%s" % (family, mask, "fused" if fused else "phased"))
    assert not problems, "\n".join(problems[:30])
    trained = [a for a in ref.trained_agents(meta) if a not in ref.MASKS[mask]]
    for a in trained:                                           # the others did train
        assert "mb0.gradnorm." + a in want and float(got["mb0.gradnorm." + a]) > 0
    if not meta["use_binary"]:                                  # continuous messages, receiver frozen: no parameter changes at all
        fresh = common.make_engine(meta)
        assert torch.equal(eng.flat_params, fresh.flat_params) and not bool(eng.opt_state.any())
    assert eng.agent_steps() == {a: (1 if a in trained or a not in ref.trained_agents(meta) else 0) for a in ref.AGENTS}
    eng.check_sync()


# ... and the two attention handles: shape B of tests/desc_attn_ref.py (the receiver's k_attn_dE / k_attn_dDD / fixed-row jobs) and the
# smallest shape of tests/test_visual_attn_gpu.py (the sender's k_vattn_bwd / k_vattn_dwx, the k_gradnorm + k_opt route of its fused step)
def _attention_case(kind):
    if kind == "desc_attn":
        from tests import desc_attn_ref as wref, test_desc_attn_gpu as t
        m = wref.train_meta("B", "adaptive")
        inputs = lambda eng, us: t._inputs(m, eng, us)
        skip = (".p.receiver.y2.bias", ".p.receiver.d_attn.bias")        # exact-zero gradients (tests/test_desc_attn_gpu.py)
        return wref, m, inputs, t._engine, skip, t.ATOL, t.RTOL
    from tests import visual_attn_ref as wref, test_visual_attn_gpu as t
    m = wref.meta("D")                                                    # a 1 x 1 map, 5 samples, attn_dim 5: the smallest of its SHAPES

    def inputs(eng, us):
        xs, ud, g = t._inputs(m, eng, us)
        eng.set_data_context(g)
        return xs, ud
    skip = (".p.receiver.y2.bias", ".p.sender.attn_U.bias")              # (tests/test_visual_attn_gpu.py: NOISE)
    return wref, m, inputs, t._engine, skip, t.ATOL, 1e-3                 # (its loss and gradient gates: 1e-4 + 1e-3 |want|)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "phased"])
@pytest.mark.parametrize("mask", sorted(ref.MASKS))
@pytest.mark.parametrize("kind", ["desc_attn", "visual_attn"])
def test_one_step_with_frozen_agents_on_the_attention_handles(kind, mask, fused):
    wref, m, inputs, engine, skip, atol, rtol = _attention_case(kind)
    us = _once(("u", kind), lambda: wref.separated_uniforms(m))
    want = _once(("attn oracle", kind, mask), lambda: ref.wrapped_oracle_minibatch(wref, m, us, ref.MASKS[mask]))
    eng = engine(m)
    dev_inputs = inputs(eng, us)
    got, eng, frozen_problems = ref.hip_loop(None, m, [dict(frozen=ref.MASKS[mask])], fused=fused, eng=eng, inputs=lambda i: dev_inputs)
    assert not frozen_problems, "\n".join(frozen_problems)
    problems = common.compare_packed(ref.pick(got, fused), ref.pick(want, fused), atol=atol, rtol=rtol, skip=skip,
                                     label="controls/%s/%s/%s" % (kind, mask, "fused" if fused else "phased"))
    assert not problems, "\n".join(problems[:30])
    trained = [a for a in ref.AGENTS if a not in ref.MASKS[mask]]
    for a in trained:
        assert float(got["mb0.gradnorm." + a]) > 0
    assert eng.agent_steps() == {a: int(a in trained) for a in ref.AGENTS}
    eng.check_sync()


# ------------------------------------------------------------------ 2. a schedule
def _schedule(meta):
    lr = meta["learning_rate"]
    return [dict(),                                                                   # all agents trained
            dict(frozen=("sender",), lr=lr / 2),                                      # sender frozen, lr halved
            dict(entropy=dict(entropy_s=0.02, entropy_sen=0.03, entropy_rec=0.002)),  # new entropy weights
            dict(frozen=("receiver",)),                                               # receiver frozen, sender unfrozen
            dict(frozen=(), lr=lr)]                                                   # all trained, lr restored


@pytest.mark.parametrize("family,optim", [("fast_c2", "RMSprop"), ("odd_generic", "Adam")])
def test_schedule_of_masks_rates_and_entropy_weights_matches_the_oracle(family, optim):
    """The sender sits out minibatches 2 and 3, the receiver minibatch 4.  Adam: with ONE global step count the sender's bias
    correction of minibatches 4 and 5 (its second and third update) would be that of steps 4 and 5, the receiver's of
    minibatch 5 (its fourth) that of step 5 -- parameters off by more than the tolerance."""
    meta = ref.family_meta(family, n_minibatches=5, optim_type=optim)
    name = "tc_schedule_%s" % family
    schedule, snaps = _schedule(meta), []
    want = _separated(name, meta, schedule, snapshots=snaps)
    got, eng, frozen_problems = ref.hip_loop(name, meta, schedule, fused=True)
    assert not frozen_problems, "\n".join(frozen_problems)
    # the six losses of the later minibatches: each side against float64 at ITS OWN parameters (common.oracle_losses_f64's gate --
    # both optimizers turn rounding-level gradients into steps of the size of the learning rate, Adam's first step on every element)
    f64 = ref.losses_f64(name, meta, schedule, want, snaps, eng.param_snapshots)
    problems = common.compare_packed(ref.pick(got, True), ref.pick(want, True), atol=ref.ATOL, rtol=ref.RTOL, skip=_skip(meta),
                                     shift_invariant=True, label="controls/schedule/" + family, f64=f64)
    assert not problems, "\n".join(problems[:30])
    assert eng.agent_steps() == dict(receiver=4, sender=3, baseline_rec=5, baseline_sen=5)
    counter = eng.tape["counter"].cpu().tolist()
    assert counter[0] == 5 and max(counter[1:3]) == 5 and counter[4:8] == [1, 2, 0, 0]
    ctl = eng.training_controls()
    assert ctl["trainable"] == ref.AGENTS and ctl["learning_rate"] == np.float32(meta["learning_rate"])
    assert (ctl["entropy_s"], ctl["entropy_sen"], ctl["entropy_rec"]) == tuple(float(np.float32(v)) for v in (0.02, 0.03, 0.002))
    eng.check_sync()


# ------------------------------------------------------------------ 3. mmg_train_steps
def test_train_steps_reads_the_controls_of_the_moment():
    meta = ref.family_meta("fast_c2", n_minibatches=4)
    dev = torch.device("cuda:0")
    xs, ts = [], []
    for i in range(4):
        (xd, td, dd), _ = ref.device_inputs(meta, i, None, dev)
        xs.append(xd); ts.append(td)
    x, t = torch.cat(xs).contiguous(), torch.cat(ts).contiguous()
    B = meta["batch"]
    a, b = common.make_engine(meta), common.make_engine(meta)
    a.train_steps(x[:2 * B], t[:2 * B], dd, 2, seed=77)
    a.set_trainable(["receiver", "baseline_rec", "baseline_sen"])
    a.set_learning_rate(meta["learning_rate"] / 2)
    a.train_steps(x[2 * B:], t[2 * B:], dd, 2, seed=77)
    for i in range(4):
        if i == 2:
            b.set_trainable(["receiver", "baseline_rec", "baseline_sen"])
            b.set_learning_rate(meta["learning_rate"] / 2)
        b.train_step(xs[i], ts[i], dd, seed=77)
    torch.cuda.synchronize()
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(a.opt_state, b.opt_state)
    assert torch.equal(a.tape["counter"], b.tape["counter"]) and a.tape["counter"].cpu().tolist()[4:8] == [0, 2, 0, 0]
    assert torch.equal(a.tape["losses"], b.tape["losses"])
    lo, hi = a.agent_range["sender"]
    assert not bool(a.flat_grads[lo:hi].any())
    fresh = common.make_engine(meta)
    assert not torch.equal(a.flat_params[lo:hi], fresh.flat_params[lo:hi])     # (the sender did train in the first call)
    a.check_sync()


# ------------------------------------------------------------------ 4. data parallel
DP_NAME = "g2_adaptive_c1"


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _dp_run(eng, dp, meta, lo, n):
    eng.set_trainable(["receiver", "baseline_rec", "baseline_sen"])
    for i in range(2):
        (xd, td, dd), u = ref.device_inputs(meta, i, DP_NAME, eng.device, lo, n)
        (dp or eng).train_step(xd, td, dd, *u, seed=1234)
    torch.cuda.synchronize()
    out = {"%s.%s" % (a, k): v.cpu().numpy() for a, d in eng.params.items() for k, v in d.items()}
    out["losses"] = eng.tape["losses"].cpu().numpy()
    slo, shi = eng.agent_range["sender"]
    out["frozen_grad_slice"] = eng.flat_grads[slo:shi].cpu().numpy()
    return out


def _dp_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from multimodalgame_amd.dist import DataParallel, shard_range
    meta = common.load_golden(DP_NAME)[1]
    lo, n = shard_range(meta["batch"], rank, world)
    eng = common.make_engine(meta, batch=n, global_batch=meta["batch"], batch_offset=lo)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **_dp_run(eng, DataParallel(eng), meta, lo, n))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_the_sender_frozen_equal_single_process(tmp_path):
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    meta = common.load_golden(DP_NAME)[1]
    eng = common.make_engine(meta)
    before = {k: v.cpu().numpy().copy() for k, v in eng.params["sender"].items()}
    want = _dp_run(eng, None, meta, 0, meta["batch"])
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for k, v in want.items():
        np.testing.assert_array_equal(r0[k], r1[k], err_msg="ranks diverged: " + k)
        if k == "receiver.y2.bias":
            continue
        np.testing.assert_allclose(r0[k], v, rtol=2e-4, atol=2e-6, err_msg=k)      # tests/test_hip_dp.py's tolerance
    for r in (r0, r1):
        assert not r["frozen_grad_slice"].any()
        for k, v in before.items():
            np.testing.assert_array_equal(r["sender." + k], v, err_msg=k)


# ------------------------------------------------------------------ 5. the forward pass
def test_freezing_the_sender_leaves_the_forward_pass_alone():
    meta = ref.family_meta("fast_c2")
    a, b = common.make_engine(meta), common.make_engine(meta)
    b.set_trainable(["receiver", "baseline_rec", "baseline_sen"])
    (xd, td, dd), u = ref.device_inputs(meta, 0, None, a.device)
    for eng in (a, b):
        eng.train_step(xd, td, dd, *u)
    torch.cuda.synchronize()
    for k in ("z", "w", "mask", "y", "losses"):
        assert torch.equal(a.tape[k], b.tape[k]), k
    assert torch.equal(a.tape["counter"][:4], b.tape["counter"][:4])          # minibatch counter, Philox stream, launch epoch
    # the other agents' gradients: bit for bit.  Their updates: the clip norm adds the blocks' sums of squares in the order of the
    # job table in use, and the table without the sender's jobs numbers the blocks differently -- a re-ordered fp32 sum of n <= 2048
    # non-negative partials moves by at most n * 2^-24 < 1.3e-4 relative, the clip coefficient 1 / norm by half of that: the step
    # each element takes agrees to rtol 1e-4
    start = common.make_engine(meta).flat_params
    for agent in ("receiver", "baseline_rec", "baseline_sen"):
        lo, hi = a.agent_range[agent]
        assert torch.equal(a.flat_grads[lo:hi], b.flat_grads[lo:hi]), agent
        step_a, step_b = a.flat_params[lo:hi] - start[lo:hi], b.flat_params[lo:hi] - start[lo:hi]
        assert bool(step_a.any()) and torch.allclose(step_a, step_b, rtol=1e-4, atol=1e-9), agent


def test_the_plan_of_a_mask_is_the_fresh_plan_for_that_mask(switches):
    """BASELINE config 3 at 512 samples: k_wgrad walks its 1 336 GEMM tiles with a stride of 856 resident workgroups.  With the receiver
    alone in training the table is another one (other tiles, other row splits, another walk) -- nothing of the plan before may survive
    mmg_set_trainable: after every
    call the handle's plan is what mmg_plan_for decides from scratch for that mask on this device's caps, and the first plan again
    once everybody trains.  One step under the small table: the closing block runs once, the forward pass is the unfrozen handle's."""
    from multimodalgame_amd import _lib
    from multimodalgame_amd.engine import Engine
    from tests.test_plan_cpu import SHAPES
    kw = SHAPES["c3_b512"]
    eng, plain = Engine(**kw), Engine(**kw)
    first = eng.plan_text()
    caps = _lib.plan_caps(first)
    fresh = lambda frozen: _lib.plan_for(eng.cfg, caps, _lib.agent_mask(frozen) << _lib.PLAN_FROZEN_SHIFT)
    assert " wgrad_stride 856 (gemm tiles 1336) " in first and first == fresh(())
    others = ("sender", "baseline_rec", "baseline_sen")
    eng.set_trainable(["receiver"])
    small = eng.plan_text()
    assert small == fresh(others) and " wgrad_stride 856 " not in small and " (gemm tiles 1336) " not in small
    eng.set_trainable(["receiver", "sender"])                    # through a second mask, then back
    assert eng.plan_text() == fresh(("baseline_rec", "baseline_sen"))
    eng.set_trainable(_lib.AGENTS)
    assert eng.plan_text() == first
    eng.set_trainable(["receiver"])
    assert eng.plan_text() == small
    from oracle import cpu_ref
    filled = cpu_ref.fill_state_dicts(common.param_shapes(eng), seed=11)
    eng.load_state_dicts(filled)
    plain.load_state_dicts(filled)                               # (its own buffers: the same seeded weights)
    x, target, desc = cpu_ref.synthetic_batch(kw["batch"], kw["n_classes"], kw["feat_dim"], kw["wv_dim"], seed=12)
    d = lambda a: torch.from_numpy(a).to(eng.device)
    before = eng.flat_params.clone()
    for e in (eng, plain):
        e.train_step(d(x), d(target), d(desc), seed=5)
    torch.cuda.synchronize()
    eng.check_sync()
    assert torch.equal(eng.tape["losses"], plain.tape["losses"]) and torch.equal(eng.tape["totals"], plain.tape["totals"])
    assert float(eng.tape["totals"][2]) == 1.0                  # minibatches counted by the closing block: once
    for a in others:
        lo, hi = eng.agent_range[a]
        assert torch.equal(eng.flat_params[lo:hi], before[lo:hi]) and not bool(eng.flat_grads[lo:hi].any()), a
    # the receiver's gradients: the same products, but the small table splits the 5 120 (step, sample) rows of a job over more
    # workgroups (host_jobs.h: plan_jobs), i.e. another order of an fp32 sum -- a part in 10^4 of the largest entry bounds it amply
    lo, hi = eng.agent_range["receiver"]
    got, want = eng.flat_grads[lo:hi], plain.flat_grads[lo:hi]
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()) and float(want.abs().max()) > 0
    assert not torch.equal(eng.flat_params[lo:hi], before[lo:hi])


# ------------------------------------------------------------------ 6. refusals and defaults
def test_refusals_and_defaults():
    from multimodalgame_amd import _lib
    meta = ref.family_meta("fast_c2")
    eng = common.make_engine(meta)
    f32 = lambda v: float(np.float32(v))
    default = dict(mask=15, trainable=_lib.AGENTS, learning_rate=f32(meta["learning_rate"]), entropy_s=f32(meta["entropy_s"]),
                   entropy_sen=f32(meta["entropy_sen"]), entropy_rec=f32(meta["entropy_rec"]))
    assert eng.training_controls() == default                   # the create-time values
    for mask in (16, -1, 0x2f):
        with pytest.raises(_lib.MmgError, match="bits outside the four agents"):
            eng.set_trainable(mask)
    for lr in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(_lib.MmgError, match="finite and >= 0"):
            eng.set_learning_rate(lr)
    with pytest.raises(_lib.MmgError, match="must be finite"):
        eng.set_entropy(entropy_sen=float("nan"))
    assert eng.training_controls() == default                   # a refused call changes nothing
    # a weight the handle was created without stays absent
    cont = common.make_engine(ref.family_meta("mc_continuous"))
    cont.set_entropy(entropy_s=0.5, entropy_sen=0.5, entropy_rec=0.5)
    cont.set_trainable(["sender"])                              # bits of agents the mode never trains: accepted
    ctl = cont.training_controls()
    assert (ctl["entropy_s"], ctl["entropy_sen"], ctl["entropy_rec"]) == (None, None, None) and ctl["trainable"] == ("sender",)
    # a handle that never calls the new entries: what two such handles always did
    other = common.make_engine(meta)
    for i in range(3):
        (xd, td, dd), u = ref.device_inputs(meta, i, None, eng.device)
        eng.train_step(xd, td, dd, *u)
        other.train_step(xd, td, dd, *u)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_params, other.flat_params) and torch.equal(eng.opt_state, other.opt_state)
    assert eng.tape["counter"].cpu().tolist()[4:8] == [0, 0, 0, 0] and eng.agent_steps() == {a: 3 for a in _lib.AGENTS}


def test_a_relaxed_game_refuses_and_a_plain_game_reaches_every_engine():
    from tests.test_autograd_gpu import _game
    meta = ref.family_meta("odd_generic")
    game, eng = _game(meta)
    game.freeze("sender")
    game.set_hyper(learning_rate=3e-5, entropy_s=0.5)           # (odd_generic is Fixed: entropy_s is set and unused)
    assert eng.training_controls()["trainable"] == ("receiver", "baseline_rec", "baseline_sen")
    later = game.engine_for(3, meta["n_classes"])               # an engine created later
    for e in (eng, later):
        ctl = e.training_controls()
        assert ctl["mask"] == 13 and ctl["learning_rate"] == float(np.float32(3e-5)) and ctl["entropy_s"] == 0.5
    sd = game.optimizers_dict()["optimizer_sen"].state_dict()
    assert sd["param_groups"][0]["lr"] == 3e-5 and sd["training_controls"]["trainable"] is False
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = common.flags_from_meta(meta)
    relaxed = Game(Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, True),
                   Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, True),
                   Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0), Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden),
                   flags=fl, device="cuda:0", autograd=True, channel_grad=True, relax=dict(tau_sen=1.0, tau_rec=1.0))
    for call in (lambda: relaxed.freeze("sender"), lambda: relaxed.set_hyper(learning_rate=1e-3)):
        with pytest.raises(NotImplementedError, match="REINFORCE step: a game with relaxed messages"):
            call()
