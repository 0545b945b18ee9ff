"""The scalar options of mmg_config and the data-dependent branch of the reward scaling, per kernel family, against the CPU
oracle.  Every other GPU case keeps first_rec at 0, s_prob_prod on, entropy_rec == entropy_sen and top_k at 2 or 6, and its
seeded weights keep std(L - beta) below 1, where max(1, std) returns 1: a kernel could read the wrong option, or compute the
wrong variance, and stay green.  tests/test_option_branches_cpu.py defines the shapes, seeds and weight tweaks used here and
shows, on the oracle alone, that these inputs reach those branches.

Gate: common.assert_parity, the project's own -- forward quantities 1e-4 absolute (the six losses of the cases with config 4's
256-bit agents against the float64 oracle, as test_hip_configs.py gates them), bits / masks / counts / hits exact, gradients /
parameters / gradient norms atol 1e-4 + rtol 1e-3, a near-threshold ReLU unit excused only through the forced re-run.  Two
minibatches per case: the update made from the first one is checked through the second."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import common
from tests import test_option_branches_cpu as ob

pytestmark = pytest.mark.gpu

KEEP_TRAIN = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")      # what the fused step leaves (live rows only)

# family -> shape (test_option_branches_cpu.TRAIN_SHAPES), switches read at mmg_create, modes (fused: mmg_train_step; phased:
# forward run-all / loss_stats / backward / clip_step, every per-step array compared; dp: one mmg_dp_train_step(full_tape = 1,
# reduce = 0)), and the timing scopes of the launches (csrc/mmg.hip: Scope) that must / must not appear in a profiled
# minibatch of the same mode.  Scope names, not kernel names: "k_game" holds k_game_fast; "k_conversation" holds
# k_conversation_fast3 (register-resident: k_prep rides in its launch, so no "k_prep+h_x" scope) or the generic k_conversation
# (with "k_prep+h_x" and "k_dC"); "k_bwd_conv" likewise k_bwd_conv_fast / k_bwd_conv; "k_conv_persist" + "k_bwd_tile" hold
# k_conv_persist + k_bwd_sample; "k_conv_rc" + "k_bwd_tile" hold k_rc_persist + k_rc_bwd; "k_conversation_mc" holds
# k_conversation_mc (binary) / k_conversation_mc3 (continuous).
FAMILIES = {
    "game": dict(shape="c1", env=(), modes=("fused",), must=("k_game", "k_wgrad"), must_not=("k_conversation", "k_stats")),
    "fast3": dict(shape="c1", env=("MMG_NO_GAME",), modes=("fused",), must=("k_conversation", "k_bwd_conv"),
                  must_not=("k_game", "k_stats", "k_prep+h_x", "k_dC", "k_conv_tile")),
    "fast3-unmerged": dict(shape="c1", env=("MMG_NO_MERGE",), modes=("phased",), must=("k_conversation", "k_stats", "k_bwd_conv", "k_dC"),
                           must_not=("k_game", "k_prep+h_x", "k_conv_tile", "k_bas_stats")),
    "fixed": dict(shape="c1-fixed", env=(), modes=("fused", "phased"), must=("k_conversation", "k_bwd_conv"),
                  must_not=("k_game", "k_prep+h_x", "k_conv_tile")),
    "tile": dict(shape="c1", env=("MMG_NO_FAST",), modes=("phased", "fused"), must=("k_conv_tile", "k_bwd_tile"),
                 must_not=("k_game", "k_conversation", "k_bwd_conv")),
    "generic": dict(shape="c1", env=("MMG_NO_FAST", "MMG_NO_TILE"), modes=("phased", "fused"),
                    must=("k_prep+h_x", "k_conversation", "k_bwd_conv", "k_dC"), must_not=("k_game", "k_conv_tile", "k_bwd_tile")),
    "generic-tiny": dict(shape="tiny", env=(), modes=("phased", "fused"), must=("k_prep+h_x", "k_conversation", "k_bwd_conv", "k_dC"),
                         must_not=("k_game", "k_conv_tile", "k_bwd_tile")),
    "persist": dict(shape="c4", env=(), modes=("phased", "fused"), must=("k_conv_persist", "k_bwd_tile"), must_not=("k_conv_rc", "k_conversation")),
    "rc": dict(shape="c4-R256", env=(), modes=("phased", "fused"), must=("k_conv_rc", "k_bwd_tile"), must_not=("k_conv_persist", "k_conversation")),
    "mc-binary": dict(shape="c1-D200", env=(), modes=("phased", "fused"), must=("k_conversation_mc", "k_bwd_conv"), must_not=("k_conv_tile", "k_game")),
    "mc3": dict(shape="mc3", env=(), modes=("phased", "fused"), must=("k_conversation_mc", "k_bwd_mc"), must_not=("k_conv_tile", "k_bwd_conv")),
    "phased-dp": dict(shape="c1", env=(), modes=("dp",), must=("k_conversation", "k_bas_stats", "k_bwd_conv", "k_gradnorm", "k_opt"),
                      must_not=("k_game", "k_prep+h_x")),
}
MODE_KW = {"fused": dict(fused=True), "phased": dict(), "dp": dict(dp_full_tape=True)}


def _pick(d):
    return {k: d[k] for k in d if any(t in k for t in KEEP_TRAIN)}


def _names(eng, name, meta, mode):
    """Timing scopes of one more minibatch of the case, run the way `mode` runs it."""
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, 0, name)
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(x), t(target), t(desc), t(u_z), t(u_s[..., 0]), t(u_w))
    eng.set_profiling(True)
    if mode == "fused":
        eng.train_step(*args)
    elif mode == "dp":
        eng.dp_train_step(*args, full_tape=True, reduce=False)
    else:
        eng.forward(*args, train=True, run_all=True)
        eng.loss_stats()
        eng.backward(*args[:3])
        eng.clip_step()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _train(family, case, monkeypatch, skip_extra=()):
    """One training case through every mode of the family against the (cached) oracle run of its shape."""
    f = FAMILIES[family]
    for sw in f["env"]:
        monkeypatch.setenv(sw, "1")
    name, meta, tweak, want, flips, params = ob.oracle_train(f["shape"], case)
    binary = bool(meta["use_binary"])
    skip = (("y2.bias",) if binary else ("y2.bias", ".bs", ".br")) + tuple(skip_extra)
    results = {}
    for mode in f["modes"]:
        got, eng = common.hip_train_case(name, meta, tweak=tweak, **MODE_KW[mode])
        label = "optbranch-%s-%s-%s" % (family, case, mode)
        # config 4's 256-bit agents (|loss| ~ 600) and the y2.weight x 30 cases (baseline losses ~ 300, one fp32 ulp = 3e-5): the
        # six losses are gated against the float64 oracle from each side's own parameters; GATE records it (float64_gate)
        f64 = common.oracle_losses_f64(name, meta, want, params, eng.param_snapshots, tweak=tweak) if f["shape"].startswith("c4") or case == "x30" else None
        g, w, sk = got, want, skip
        if mode == "fused":
            g, w = _pick(got), _pick(want)
        elif mode == "dp":                              # the log minibatch: the conversation on every row, the baselines on the live rows only
            sk = skip + (".bs", ".br")
        print(label, "losses", np.asarray(got["mb0.losses"]).round(4).tolist(), "hits", [int(got["mb%d.hits" % i]) for i in range(meta["n_minibatches"])])
        common.assert_parity(g, w, flips, eng, label, skip=sk, f64=f64)
        names = _names(eng, name, meta, mode)
        print(label, names)
        assert all(n in names for n in f["must"]) and not any(n in names for n in f["must_not"]), (label, names)
        results[mode] = got
    return results, want, meta


@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "mc3"])
def test_scaled_rewards_vs_oracle(family, monkeypatch):
    """receiver.y2.weight scaled so that the per-(stream, step) std of L - beta lies on both sides of 1 within minibatch 0
    (config 1's shape, x 8: (L - br, L - bs) = (1.87, 2.01), (1.32, 1.46), (0.88, 1.11), (0.19, 0.60); the other shapes and
    their factors: test_option_branches_cpu.TRAIN_SHAPES), and three distinct entropy weights: entropy_s 0.05, entropy_rec 0.03,
    entropy_sen 0.005.  A wrong variance, a dropped sd > 1 select or a swapped lambda moves the losses and gradients far beyond
    the gate (the oracle itself: test_oracle_separates_entropy_rec_from_entropy_sen)."""
    _train(family, "scaled", monkeypatch)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_first_message_vs_oracle(family, monkeypatch):
    """first_rec = 0.5 (the receiver's message before step 0: the sender's code layer and the sender baseline of step 0 read
    it), entropy_rec = None with the other two set and distinct (has_entropy_* per stream), top_k_train = 1.  mc3: continuous
    messages have no REINFORCE losses -- first_rec and top_k are the options that apply."""
    _train(family, "first", monkeypatch)


def test_top_k_1_hits_vs_oracle(monkeypatch):
    """top_k_train = 1 alone at the game shape: `above < top_k` degenerates to "the target is the argmax".  Seeds with at least
    one hit per minibatch (test_oracle_separates_top_k_1); hits are exact in assert_parity."""
    results, want, meta = _train("game", "topk1", monkeypatch)
    for i in range(meta["n_minibatches"]):
        assert int(results["fused"]["mb%d.hits" % i]) == int(want["mb%d.hits" % i]) >= 1


@pytest.mark.parametrize("family", ["game", "generic"])
def test_y2_times_30_cancellation_vs_oracle(family, monkeypatch):
    """One case per coefficient implementation (game: coef_compute behind the (value, epoch) pair table; generic:
    loss_coefficients) with receiver.y2.weight x 30: every live (stream, step) has std > 1, up to about 7, and mean(L) is about
    -15 (test_y2_times_30_keeps_every_live_step_above_one), so the variance s5[2] - n * mean^2 loses two to three digits to
    cancellation.  The baseline losses are means of (L - beta)^2 ~ 300 here, where one fp32 ulp is 3.1e-5: under the absolute
    gate minibatch 1's losses came out 1.37e-4 (game) and 1.22e-4 (generic) from the fp32 oracle, every other forward quantity
    within 1.2e-5 -- so the six losses of this case are gated as config 4's are, |GPU - f64| <= |fp32 oracle - f64| + 1e-4
    (common.oracle_losses_f64 with the tweak); everything else keeps 1e-4 absolute."""
    _train(family, "x30", monkeypatch)


def test_tied_target_logit_counts_as_the_rule_says(monkeypatch):
    """Classes 2k and 2k + 1 get identical description rows, so every target logit ties with its twin's TO THE BIT (same
    arithmetic on the same numbers).  The library's rule is hit = #{d: y[d] > y[target]} < top_k (strict: a tied class is not
    "above"); with top_k = 3 and pairs of equal logits that is "the target's pair is among the best two pairs", while a rule
    with >= would need the pair to be the best one.  The expected count is formed from the GPU's own selected logits by that
    rule.  The oracle's count is NOT the contract here: it takes the last top_k indices of numpy's argsort (model.py:1333),
    whose order among equal keys is unspecified (introsort, not stable), and torch's CPU GEMM need not even give the twins
    bit-equal logits (its row blocking treats them differently) -- so `hits` is left out of the comparison with the oracle and
    everything else goes through the gate."""
    real = cpu_ref.synthetic_batch

    def twins(*a, **kw):
        x, target, desc = real(*a, **kw)
        desc = desc.copy()
        desc[1::2] = desc[0:2 * (len(desc) // 2):2]
        return x, target, desc
    monkeypatch.setattr(cpu_ref, "synthetic_batch", twins)
    kw, _, B, seeds, _ = ob.TRAIN_SHAPES["c1"]
    D, k = 6, 3
    name, meta = "optbranch-tied", ob.make_meta(dict(kw, top_k_train=k), D, B, 2, seeds)
    common.separate_draws(name, meta)
    flips = []
    want = common.oracle_train_case(name, meta, flips=flips)
    got, eng = common.hip_train_case(name, meta, fused=True)
    common.assert_parity(_pick(got), _pick(want), flips, eng, "optbranch-tied", skip=("y2.bias", "hits"))
    differs = 0
    for i in range(meta["n_minibatches"]):
        _, target, _, _ = common.case_inputs(meta, i, name)
        y = np.asarray(got["mb%d.outp" % i])
        np.testing.assert_array_equal(y[:, 0::2], y[:, 1::2])               # the premise: twins tie to the bit on the GPU
        yt = y[np.arange(B), target][:, None]
        strict = int(((y > yt).sum(1) < k).sum())
        other = np.ones_like(y, bool)
        other[np.arange(B), target] = False
        loose = int(((((y >= yt) & other).sum(1)) < k).sum())
        print("minibatch", i, "hits", int(got["mb%d.hits" % i]), "rule", strict, "with >=", loose, "oracle", int(want["mb%d.hits" % i]))
        assert int(got["mb%d.hits" % i]) == strict
        differs += int(strict != loose)
    assert differs, "the two rules count the same on this input: the tie decides nothing"
    assert "k_game" in _names(eng, name, meta, "fused")


# ----------------------------------------------------------------------------------------------
# evaluation pass: s_prob_prod off
# ----------------------------------------------------------------------------------------------
EVAL_FAMILIES = {
    "fast3": dict(shape="c1", env=(), must=("k_conversation",), must_not=("k_prep+h_x", "k_conv_tile")),
    "tile": dict(shape="c1", env=("MMG_NO_FAST",), must=("k_conv_tile",), must_not=("k_conversation",)),
    "generic": dict(shape="c1", env=("MMG_NO_FAST", "MMG_NO_TILE"), must=("k_prep+h_x", "k_conversation"), must_not=("k_conv_tile",)),
    "persist": dict(shape="c4", env=(), must=("k_conv_persist",), must_not=("k_conv_rc", "k_conversation")),
    "rc": dict(shape="c4-R256", env=(), must=("k_conv_rc",), must_not=("k_conv_persist", "k_conversation")),                  # k_rc_persist (kernels_rc.h: its role of the stop decision)
    "rc-steps": dict(shape="c4-R256", env=("MMG_NO_RC_PERSIST",), must=("k_conv_rc",), must_not=("k_conv_persist", "k_conversation")),   # k_rc_heads per step
    "mc-binary": dict(shape="c1-D200", env=(), must=("k_conversation_mc",), must_not=("k_conv_tile", "k_conversation")),
}


def _eval_arm(shape, spp):
    """GPU evaluation pass of one arm (run-all, as eval_dev runs it) against cpu_ref.eval_batch: (conversation lengths of the GPU,
    the tie-free samples, scopes of the launch)."""
    meta, (x, target, desc), r = ob.oracle_eval(shape, spp)
    eng = common.make_engine(meta, tweak=ob.SX30)
    assert int(eng.cfg.s_prob_prod) == int(spp)
    dev = eng.device
    eng.set_profiling(True)
    eng.forward(torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev), train=False, run_all=True)
    torch.cuda.synchronize()
    eng.check_sync()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    tp = {k: v.cpu().numpy() for k, v in eng.tape.items() if k in ("mask", "s", "z", "w", "y", "dist", "hit")}
    n, B = r["n_steps"], meta["batch"]
    ft = ob.first_tie(r)                                   # per sample: its first step with a message bit on a tie (n: none)
    ok = ft == n
    stack = lambda key: np.stack([t.numpy() for t in r[key]])
    want = dict(s=stack("s_feats"), z=stack("sen_feats"), w=stack("rec_feats"), mask=stack("s_masks"), y=stack("y"))
    alive = tp["mask"][1:, :, 0].sum(1)
    if ok.all():
        assert int(np.argmax(alive == 0)) + 1 == n if (alive == 0).any() else n == meta["max_exchange"]
    # tie-free samples: every executed step, exactly
    for key in ("s", "z", "w"):
        np.testing.assert_array_equal(tp[key][:n][:, ok], want[key][:, ok], err_msg=key)
    np.testing.assert_array_equal(tp["mask"][:n][:, ok], want["mask"][:n][:, ok], err_msg="mask")
    np.testing.assert_allclose(tp["y"][:n][:, ok], want["y"][:, ok], rtol=0, atol=1e-4, err_msg="y")
    np.testing.assert_allclose(tp["dist"][ok], r["dist"].numpy()[ok], rtol=0, atol=1e-4, err_msg="dist at the selected step")
    lens = tp["s"][:n, :, 0].sum(0)
    np.testing.assert_array_equal(lens[ok], np.asarray(r["conversation_lengths"])[ok], err_msg="conversation lengths")
    want_hit = (r["top_k_ind"].numpy() == target.reshape(-1, 1)).any(1)
    np.testing.assert_array_equal((tp["hit"].reshape(-1) != 0)[ok], want_hit[ok], err_msg="hits")
    if ok.all():
        assert int(tp["hit"].sum()) == int(r["hits"])
    # the others: pinned up to their first tie (the sender's message of that step included when its own bits are clear)
    for b in np.nonzero(~ok)[0]:
        t0 = int(ft[b])
        for key in ("s", "z", "w"):
            np.testing.assert_array_equal(tp[key][:t0, b], want[key][:t0, b], err_msg="%s of sample %d before its tie at step %d" % (key, b, t0))
    print(shape, "s_prob_prod", spp, "steps", n, "tie-free", int(ok.sum()), "lengths", lens.astype(int).tolist(), names)
    return lens, ok, names


@pytest.mark.parametrize("family", list(EVAL_FAMILIES))
def test_eval_without_the_running_product_vs_oracle(family, monkeypatch):
    """eng.forward(train = False) with s_prob_prod off -- the stop bit is round(p_t), not round(prod p) -- and, on the same
    weights and inputs, with it on, both against cpu_ref.eval_batch: stop bits, masks, message bits, conversation lengths and
    per-sample hits exact, logits of every step and the log-probabilities at the selected step within 1e-4.  receiver.s.weight
    x 30 spreads p_t: no decision value within 1e-3 of 0.5, a quarter of the samples and more get another length under the
    other arm (test_eval_stop_decisions_differ_between_the_arms).  The 256-bit agents always have a few message probabilities
    within 1e-5 of 0.5 among their 65 000: those samples are pinned up to that step only and count towards no figure.
    B = 32, T = 10 (config 1's agents) / T = 4 (config 4's)."""
    f = EVAL_FAMILIES[family]
    for sw in f["env"]:
        monkeypatch.setenv(sw, "1")
    lens, oks = {}, {}
    for spp in (True, False):
        lens[spp], oks[spp], names = _eval_arm(f["shape"], spp)
        assert all(n in names for n in f["must"]) and not any(n in names for n in f["must_not"]), names
    clean = oks[True] & oks[False]
    assert ((lens[True] != lens[False]) & clean).mean() >= 0.25, "the two arms should differ on this input"


def test_eval_steps_without_the_running_product_vs_oracle():
    """mmg_eval_steps (k_eval_reduce behind k_conversation_fast3) with s_prob_prod off: conversation lengths, hits and the
    executed step count exact against cpu_ref.eval_batch."""
    meta, (x, target, desc), r = ob.oracle_eval("c1", False)
    assert (ob.first_tie(r) == r["n_steps"]).all()
    eng = common.make_engine(meta, tweak=ob.SX30)
    dev = eng.device
    acc = eng.eval_acc()
    eng.set_profiling(True)
    lens, batch = eng.eval_steps(torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev), 1, 6, acc)
    torch.cuda.synchronize()
    eng.check_sync()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    print(names, lens.cpu().tolist(), acc[:4].cpu().tolist(), batch[0, 0].item())
    assert "k_eval_reduce" in names and "k_conversation" in names and "k_prep+h_x" not in names, names
    np.testing.assert_array_equal(lens.cpu().numpy(), np.asarray(r["conversation_lengths"]).astype(np.int32))
    assert int(acc[0]) == int(r["hits"]) and int(acc[2]) == meta["batch"]
    assert int(batch[0, 0]) == int(r["n_steps"])
    meta_on, _, r_on = ob.oracle_eval("c1", True)
    assert np.asarray(r_on["conversation_lengths"]).tolist() != np.asarray(r["conversation_lengths"]).tolist()
