"""Reach conditions of tests/test_option_branches_gpu.py, checked on the CPU oracle alone: the inputs of those GPU cases must
actually take the branches they are meant for -- a green GPU test must not be green because its input never got there.

  * reward scaling: weight = (L - beta) / max(1, std(L - beta)) per (stream, step) (model.py:912-916).  With the seeded weights
    the sample std stays below 1 everywhere, so max() always returns 1; scaling receiver.y2.weight spreads the log-likelihoods
    L and puts steps of ONE minibatch on both sides of 1.
  * options: the oracle itself must tell entropy_rec from entropy_sen, first_rec 0.5 from 0 and entropy_rec None from 0.03 at
    the GPU tests' gate -- otherwise a kernel that mixed them up would pass.
  * eval stop decisions: round(running product of p_t) (s_prob_prod) against round(p_t); receiver.s.weight x 30 spreads p_t so
    that the two arms stop different samples at different steps, with no decision value near 0.5.

The shapes, seeds and tweaks of the GPU cases are defined HERE (TRAIN_SHAPES, EVAL_SHAPES) and imported by the GPU file."""
import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import common

ATOL, RTOL = 1e-4, 1e-3                  # the GPU gate (common.assert_parity)

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01,
          entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6)
C4 = dict(C1, img_h_dim=1024, rec_w_dim=256, sender_out_dim=256, max_exchange=4)
TINY = dict(use_binary=True, fixed_exchange=False, max_exchange=5, learning_rate=1e-4, img_feat_dim=16, img_h_dim=8, rec_w_dim=6,
            sender_out_dim=6, rec_hidden=5, wv_dim=7, baseline_hid_dim=9, top_k_train=2)

# the two option sets of the GPU training cases
SCALED_OPTS = dict(entropy_s=0.05, entropy_rec=0.03, entropy_sen=0.005)                 # all three distinct, + a y2.weight tweak
FIRST_OPTS = dict(first_rec=0.5, entropy_s=0.05, entropy_rec=None, entropy_sen=0.005, top_k_train=1)


def scale(key, factor):
    """tweak (common.apply_tweak): receiver.<key> *= factor, in place on the float32 arrays (exact: a power of two or not, both
    sides multiply the same float32 numbers by the same float32 factor)."""
    def tweak(sd):
        sd["receiver"][key] *= np.float32(factor)
    return tweak


Y2X8, Y2X30, SX30 = scale("y2.weight", 8), scale("y2.weight", 30), scale("s.weight", 30)


def make_meta(flags_kw, n_classes, batch, n_mb, seeds=(5, 6, 7)):
    fl = cpu_ref.Flags(**dict(flags_kw, batch_size=batch))
    meta = dict(fl.__dict__)
    meta.update(n_classes=n_classes, batch=batch, n_minibatches=n_mb, seed_weights=seeds[0], seed_data=seeds[1], seed_uniforms=seeds[2])
    return meta


# shape id -> (flags, classes, batch, seeds (weights, data, uniforms), y2.weight factor of the scaled case).  The kernel families
# of the GPU file that share a shape share its oracle run.  Seeds / factors: the first ones at which the oracle alone meets the
# reach condition below.  Every case runs on uniforms moved 1e-4 away from their probabilities (common.separate_draws: the
# 256-bit agents draw 16 000 Bernoulli bits per minibatch, some uniform always lies within 1e-5 of its probability).
TRAIN_SHAPES = {
    "c1": (C1, 30, 16, (5, 6, 7), 8),                                                   # game, fast3, fast3-unmerged, tile, generic, phased-dp
    "c1-fixed": (dict(C1, fixed_exchange=True, max_exchange=4), 30, 16, (5, 6, 7), 4),               # (x 8: every step at 1.7-1.9)
    "tiny": (TINY, 5, 8, (5, 6, 7), 4),                                                 # (x 8: 0.92 .. 2.30)
    "c4": (C4, 30, 16, (5, 6, 7), 4),                                                   # persist (x 8: 1.29 .. 2.05)
    "c4-R256": (dict(C4, rec_hidden=256), 30, 16, (5, 6, 7), 4),                        # rc (x 8: 1.46 .. 2.76)
    "c1-D200": (C1, 200, 16, (5, 6, 7), 8),                                             # mc-binary
}
MC3_SHAPE = (dict(C1, use_binary=False, fixed_exchange=True, max_exchange=4, entropy_s=None, entropy_sen=None, entropy_rec=None), 200, 16, (5, 6, 7))
TOPK1_SEEDS = (1, 6, 7)
N_MB = 2


def train_meta(shape, case, n_mb=N_MB):
    """case: "scaled" | "first" | "topk1" | "x30" -> (meta, tweak)."""
    if shape == "mc3":
        kw, D, B, seeds = MC3_SHAPE
        assert case == "first"
        return make_meta(dict(kw, first_rec=0.5, top_k_train=1), D, B, n_mb, seeds), None
    kw, D, B, seeds, factor = TRAIN_SHAPES[shape]
    if case == "scaled":
        return make_meta(dict(kw, **SCALED_OPTS), D, B, n_mb, seeds), scale("y2.weight", factor)
    if case == "first":
        return make_meta(dict(kw, **FIRST_OPTS), D, B, n_mb, seeds), None
    if case == "topk1":                         # (its own seeds: the ones above leave no top-1 hit in either minibatch)
        return make_meta(dict(kw, top_k_train=1), D, B, n_mb, TOPK1_SEEDS), None
    if case == "x30":
        return make_meta(dict(kw, **SCALED_OPTS), D, B, n_mb, seeds), Y2X30
    raise KeyError(case)


# eval shapes: id -> (flags, classes, batch, seeds (weights, data)); s.weight x 30 on all of them
EVAL_SHAPES = {
    "c1": (C1, 30, 32, (8, 26)),                                                        # fast3, tile, generic, eval_steps
    "c4": (C4, 30, 32, (2, 26)),                                                        # persist
    "c4-R256": (dict(C4, rec_hidden=256), 30, 32, (2, 26)),                             # rc, with and without the one-launch roles
    "c1-D200": (C1, 200, 32, (5, 36)),                                                  # mc-binary
}


def eval_meta(shape, s_prob_prod):
    kw, D, B, seeds = EVAL_SHAPES[shape]
    return make_meta(dict(kw, s_prob_prod=bool(s_prob_prod)), D, B, 1, seeds + (0,))


# ----------------------------------------------------------------------------------------------
# oracle runs, cached per session (the GPU file imports these)
# ----------------------------------------------------------------------------------------------
_TRAIN_CACHE, _EVAL_CACHE = {}, {}


def case_name(shape, case, n_mb=N_MB):
    return "optbranch-%s-%s-%d" % (shape, case, n_mb)


def oracle_train(shape, case, n_mb=N_MB):
    """(name, meta, tweak, want, flips, params_before) of a training case; the returned objects are shared -- leave them
    unchanged.  `name` is the key under which the case's separated uniforms are registered (common.U_OVERRIDES): hand it to
    hip_train_case / case_inputs."""
    key = (shape, case, n_mb)
    if key not in _TRAIN_CACHE:
        meta, tweak = train_meta(shape, case, n_mb)
        name = case_name(shape, case, n_mb)
        if meta["use_binary"]:
            common.separate_draws(name, meta, tweak=tweak)
        flips, params = [], []
        want = common.oracle_train_case(name, meta, flips=flips, params_before=params, tweak=tweak)
        _TRAIN_CACHE[key] = (name, meta, tweak, want, flips, params)
    return _TRAIN_CACHE[key]


def oracle_eval(shape, s_prob_prod, top_k=6):
    """(meta, inputs (x, target, desc), cpu_ref.eval_batch's result) with s.weight x 30."""
    key = (shape, bool(s_prob_prod), top_k)
    if key not in _EVAL_CACHE:
        meta = eval_meta(shape, s_prob_prod)
        fl = common.flags_from_meta(meta)
        torch.manual_seed(0)
        models = cpu_ref.build_agents(fl)
        filled = cpu_ref.load_filled(models, seed=meta["seed_weights"])
        common.apply_tweak(models, filled, SX30)
        x, target, desc = cpu_ref.synthetic_batch(meta["batch"], meta["n_classes"], fl.img_feat_dim, fl.wv_dim, seed=meta["seed_data"])
        res = cpu_ref.eval_batch(models, torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc), fl, top_k=top_k)
        _EVAL_CACHE[key] = (meta, (x, target, desc), res)
    return _EVAL_CACHE[key]


# ----------------------------------------------------------------------------------------------
# what the reach conditions measure
# ----------------------------------------------------------------------------------------------
def reward_stds(want, meta, mb=0):
    """{(stream, step): sample std (ddof = 1) of L - beta over the live rows} of minibatch `mb`, for every (stream, step) with
    more than one live row -- from the oracle's own logs / br / bs / s_masks, paired as train_minibatch pairs them
    (cpu_ref.train_minibatch: s and sen use s_masks[:-1]; rec uses br[:-1] with s_masks[1:-1]; Fixed: no masks, no s stream)."""
    p = "mb%d." % mb
    n = int(want[p + "n_steps"])
    logs = np.asarray(want[p + "logs"], np.float64).reshape(-1)
    br, bs = np.asarray(want[p + "br"], np.float64), np.asarray(want[p + "bs"], np.float64)
    masks = np.asarray(want[p + "s_masks"]).reshape(n + 1, -1) != 0
    fixed = bool(meta["fixed_exchange"])
    out = {}
    streams = [("rec", br, 1, n - 1), ("sen", bs, 0, n)] + ([] if fixed else [("s", br, 0, n)])
    for name, beta, moff, steps in streams:
        for t in range(steps):
            live = np.ones_like(masks[0]) if fixed else masks[t + moff]
            if live.sum() > 1:
                out[(name, t)] = float(np.std((logs - beta[t].reshape(-1))[live], ddof=1))
    return out


def stop_decisions(res, s_prob_prod):
    """(decision values [n, B], live [n, B]) of an eval_batch result: the running product of p_t (s_prob_prod) or p_t itself is
    what round() turns into the stop bit (model.py:421-427); a row is live at step t while its mask is still 1."""
    p = np.stack([t.numpy().reshape(-1) for t in res["s_probs"]]).astype(np.float64)
    val = np.cumprod(p, 0) if s_prob_prod else p
    live = np.stack([m.numpy().reshape(-1) for m in res["s_masks"]])[:p.shape[0]] != 0
    return val, live


TIE = 1e-5          # |p - 0.5| below which round(p) of a message bit may differ between two correct fp32 implementations: 25 x the
                    # largest |p_HIP - p_oracle| the parity suite has recorded at config 4 (4.2e-7, profiles/r06_parity_maxerr.json)
MIN_GAP = 2e-4      # logits are compared at 1e-4: a target logit further than 2e-4 from every other one keeps its rank


def first_tie(res):
    """Per sample: the first executed step at which one of its message probabilities (sender or receiver) lies within TIE of
    0.5; n_steps where none does.  From that step on the sample's bits, and everything downstream, are not pinned."""
    n = res["n_steps"]
    near = np.zeros((n, res["sen_probs"][0].shape[0]), bool)
    for k in ("sen_probs", "rec_probs"):
        near |= (np.abs(np.stack([t.numpy() for t in res[k]]).astype(np.float64) - 0.5) < TIE).any(2)
    return np.where(near.any(0), near.argmax(0), n)


def hit_stable(res, target, top_k):
    """Per sample: hit = #{d: y[d] > y[target]} < top_k comes out the same when every other logit moves by MIN_GAP either way."""
    y = res["outp"].numpy().astype(np.float64)
    yt = y[np.arange(len(target)), target][:, None]
    other = np.ones_like(y, bool)
    other[np.arange(len(target)), target] = False
    k = min(top_k, y.shape[1])
    return (((y > yt + MIN_GAP) & other).sum(1) < k) == (((y > yt - MIN_GAP) & other).sum(1) < k)


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(TRAIN_SHAPES))
def test_scaled_rewards_put_stds_on_both_sides_of_one(shape):
    name, meta, tweak, want, _, _ = oracle_train(shape, "scaled")
    sd = reward_stds(want, meta, 0)
    print(shape, {k: round(v, 3) for k, v in sorted(sd.items())})
    assert any(v > 1.1 for v in sd.values()), "no (stream, step) with std > 1.1: the sd > 1 arm of max(1, std) is not reached"
    assert any(v < 0.9 for v in sd.values()), "no (stream, step) with std < 0.9: the denom = 1 arm is not reached"
    # no Bernoulli draw within rounding distance of its probability: the GPU run follows the same trajectory
    assert common.sampling_margin(want, meta, name) > 5e-5


@pytest.mark.parametrize("shape", sorted(TRAIN_SHAPES) + ["mc3"])
def test_first_message_case_has_clear_draws(shape):
    name, meta, tweak, want, _, _ = oracle_train(shape, "first")
    if meta["use_binary"]:
        assert common.sampling_margin(want, meta, name) > 5e-5


def test_config1_scaled_case_has_the_stds_of_the_issue():
    """(L - br, L - bs) per step of minibatch 0 at config 1's shape with y2.weight x 8: (1.87, 2.01), (1.32, 1.46),
    (0.88, 1.11), (0.19, 0.60) -- the figures DESIGN.md quotes."""
    name, meta, tweak, want, _, _ = oracle_train("c1", "scaled")
    sd = reward_stds(want, meta, 0)
    got = [(sd[("s", t)], sd[("sen", t)]) for t in range(4)]
    np.testing.assert_allclose(got, [(1.87, 2.01), (1.32, 1.46), (0.88, 1.11), (0.19, 0.60)], rtol=0, atol=6e-3)


def test_unscaled_weights_never_reach_std_above_one():
    """The gap this file closes: with the seeded weights as they are, every (stream, step) of the same case has std < 1."""
    meta, _ = train_meta("c1", "scaled", 1)
    want = common.oracle_train_case(None, meta)
    sd = reward_stds(want, meta, 0)
    assert sd and max(sd.values()) < 1.0, sd


def test_y2_times_30_keeps_every_live_step_above_one():
    """The cancellation case (s5[2] - n * mean^2 with mean(L) ~ -20): every (stream, step) with n > 1 has std > 1."""
    name, meta, tweak, want, _, _ = oracle_train("c1", "x30")
    for mb in range(meta["n_minibatches"]):
        sd = reward_stds(want, meta, mb)
        print(mb, "mean L %.2f" % float(np.mean(want["mb%d.logs" % mb])), {k: round(v, 2) for k, v in sorted(sd.items())})
        assert sd and min(sd.values()) > 1.0, sd
    assert float(np.mean(want["mb0.logs"])) < -10.0
    assert common.sampling_margin(want, meta, name) > 5e-5


def _separates(kw_a, kw_b, tweak=None):
    kw, D, B, seeds, _ = TRAIN_SHAPES["c1"]
    a = common.oracle_train_case(None, make_meta(dict(kw, **kw_a), D, B, 1, seeds), tweak=tweak)
    b = common.oracle_train_case(None, make_meta(dict(kw, **kw_b), D, B, 1, seeds), tweak=tweak)
    problems = common.compare_packed(a, b, atol=ATOL, rtol=RTOL, skip=("y2.bias",), shift_invariant=True)
    print(len(problems), problems[:6])
    return problems


def test_oracle_separates_entropy_rec_from_entropy_sen():
    problems = _separates(SCALED_OPTS, dict(SCALED_OPTS, entropy_rec=SCALED_OPTS["entropy_sen"], entropy_sen=SCALED_OPTS["entropy_rec"]), Y2X8)
    assert any("losses" in p for p in problems) and any(".g.receiver" in p for p in problems) and any(".g.sender" in p for p in problems), problems


def test_oracle_separates_first_rec():
    problems = _separates(FIRST_OPTS, dict(FIRST_OPTS, first_rec=0.0))
    assert any(p.split(" ")[0].endswith((".bs", ".sen_probs", ".y")) for p in problems), problems


def test_oracle_separates_entropy_rec_none():
    problems = _separates(FIRST_OPTS, dict(FIRST_OPTS, entropy_rec=0.03))
    assert any("losses" in p for p in problems) and any(".g.receiver" in p for p in problems), problems


def test_oracle_separates_top_k_1():
    name, meta, _, want, _, _ = oracle_train("c1", "topk1")
    hits1 = [int(want["mb%d.hits" % i]) for i in range(N_MB)]
    dist = np.asarray(want["mb0.dist"])
    x, target, desc, _ = common.case_inputs(meta, 0, name)
    assert hits1[0] == int((dist.argmax(1) == target).sum())
    top6 = int((np.argsort(dist, 1)[:, -6:] == target[:, None]).sum())
    print("hits top-1", hits1, "top-6 of minibatch 0", top6)
    assert min(hits1) >= 1, "a kernel that never counts a hit would pass"
    assert top6 > hits1[0], "top_k = 1 and top_k = 6 count the same hits on this input"


@pytest.mark.parametrize("shape", sorted(EVAL_SHAPES))
def test_eval_stop_decisions_differ_between_the_arms(shape):
    """Margin >= 1e-3 of every decision value (live rows -- and stopped ones: they keep computing in the run-all evaluation pass
    and the reference's conversation length sums their stop bits too, model.py:671); >= 25 % of the samples get another
    conversation length under the other arm; >= 3 distinct lengths without the product.  Samples with a message bit on a tie
    (first_tie; the 256-bit agents always have a few among their 65 000 probabilities) do not count towards either figure: the
    GPU test pins them up to the tie only."""
    res, clean = {}, None
    for spp in (True, False):
        meta, (x, target, desc), r = oracle_eval(shape, spp)
        val, live = stop_decisions(r, spp)
        margin = float(np.abs(val - 0.5)[live].min())
        ft = first_tie(r)
        ok = ft == r["n_steps"]
        print(shape, "s_prob_prod", spp, "steps", r["n_steps"], "margin live %.2e all %.2e" % (margin, float(np.abs(val - 0.5).min())),
              "tie-free samples %d of %d" % (int(ok.sum()), len(ok)), "stable hits %d" % int(hit_stable(r, target, 6).sum()),
              "lengths", sorted(set(np.asarray(r["conversation_lengths"])[ok].tolist())))
        assert margin >= 1e-3
        assert float(np.abs(val - 0.5).min()) >= 1e-3
        assert ok.mean() >= 0.75
        if shape.startswith("c1"):
            assert ok.all()                     # the 32-bit agents: seeds without a single tie
        assert hit_stable(r, target, 6)[ok].all()
        res[spp] = r
        clean = ok if clean is None else clean & ok
    la, lb = np.asarray(res[True]["conversation_lengths"]), np.asarray(res[False]["conversation_lengths"])
    print(shape, "tie-free samples with another length: %d of %d" % (int(((la != lb) & clean).sum()), len(la)))
    assert ((la != lb) & clean).mean() >= 0.25
    assert len(set(lb[clean].tolist())) >= 3


def test_make_config_carries_the_options():
    base = dict(batch=16, n_classes=30, feat_dim=512, h_dim=256, w_dim=32, rec_hidden=64, wv_dim=100, bas_hidden=500, max_exchange=10)
    c = _lib.make_config(first_rec=0.5, s_prob_prod=False, entropy_s=0.05, entropy_sen=0.005, entropy_rec=None, top_k=1, **base)
    assert c.first_rec == 0.5 and c.s_prob_prod == 0 and c.top_k == 1
    assert (c.has_entropy_s, c.has_entropy_sen, c.has_entropy_rec) == (1, 1, 0)
    assert c.entropy_s == np.float32(0.05) and c.entropy_sen == np.float32(0.005) and c.entropy_rec == 0.0
    for none in ("entropy_s", "entropy_sen", "entropy_rec"):
        kw = dict(entropy_s=0.05, entropy_sen=0.005, entropy_rec=0.03)
        kw[none] = None
        c = _lib.make_config(**dict(base, **kw))
        assert [c.has_entropy_s, c.has_entropy_sen, c.has_entropy_rec] == [int(k != none) for k in ("entropy_s", "entropy_sen", "entropy_rec")]
        assert [c.entropy_s, c.entropy_sen, c.entropy_rec] == [np.float32(kw[k] or 0.0) for k in ("entropy_s", "entropy_sen", "entropy_rec")]
    d = _lib.make_config(**base)
    assert d.first_rec == 0.0 and d.s_prob_prod == 1 and d.top_k == 6
    # ... and through the helper the GPU tests build their engines with
    meta, _ = train_meta("c1", "first")
    c = _lib.make_config(**common.engine_kwargs(meta))
    assert c.first_rec == 0.5 and c.top_k == 1 and c.has_entropy_rec == 0 and c.has_entropy_s == 1 and c.has_entropy_sen == 1
    assert _lib.make_config(**common.engine_kwargs(eval_meta("c1", False))).s_prob_prod == 0
    assert _lib.make_config(**common.engine_kwargs(eval_meta("c1", True))).s_prob_prod == 1


def test_tweak_default_is_bit_identical_and_both_sides_get_the_same_edit():
    meta, _ = train_meta("tiny", "scaled", 1)
    a = common.oracle_train_case(None, meta)
    b = common.oracle_train_case(None, meta, tweak=lambda sd: None)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl, rng=cpu_ref.UniformTape())
    filled = cpu_ref.load_filled(models, seed=meta["seed_weights"])
    before = filled["receiver"]["y2.weight"].copy()
    common.apply_tweak(models, filled, Y2X8)
    np.testing.assert_array_equal(models["receiver"].y2.weight.detach().numpy(), before * np.float32(8))
    shapes = {a_: {k: tuple(v.shape) for k, v in m.state_dict().items()} for a_, m in models.items()}
    eng_side = cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"])
    Y2X8(eng_side)                                                  # what common.make_engine loads
    for a_, m in models.items():
        for k, v in m.state_dict().items():
            np.testing.assert_array_equal(v.numpy(), eng_side[a_][k], err_msg="%s.%s" % (a_, k))
