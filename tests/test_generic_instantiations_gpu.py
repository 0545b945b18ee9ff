"""The generic per-sample family's 512-thread conversation kernels (k_conversation<512>, its flip and variant instantiations,
k_conversation_attn<512>, k_conversation_vattn<512>), its large-batch reverse pass (k_bwd_conv<MANY = true>, plain and with a sender
variant) and the ragged edges of gemm_kmajor_tile's float4 branch (k_vattn_prep), each against the feature's own wrapped CPU oracle.

Shapes, the two selection rules as predicates, seeds: tests/generic_inst.py (tests/test_generic_instantiations_cpu.py asserts what
the shapes select and what the seeds reach).  Every case compares what the feature's own module compares for a training minibatch --
the tape of the training conversation (bits exact, probabilities within tolerance), the six losses, every gradient tensor, the
parameters after the update -- with that module's tolerances: forward 1e-4 absolute, gradients and parameters 1e-4 + 1e-3 |v|.

The profiling scopes do not tell 256 from 512 threads or MANY from not: the predicates say which instantiation a shape selects, the
scopes and the plan's family that the generic kernels ran.  A plain handle of the small shape at 513 samples would take the sample
tiles (its dimensions are multiples of four); MMG_NO_TILE=1, read when the handle is created, keeps it on the generic family."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import common, desc_attn_ref as da, flipout_ref, generic_inst as gi, sender_variant_ref as sv, visual_attn_ref as va
from tests import test_desc_attn_gpu as tda, test_visual_attn_gpu as tv

pytestmark = pytest.mark.gpu

SEED = 21
ATOL, RTOL = gi.ATOL, gi.RTOL
FUSED_KEEP = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")      # tests/test_hip_parity.py
STEP = [False, True]
STEP_IDS = ["phased", "fused"]


def _skip_keys(m):
    # y2.bias: a shift of every class logit, its update is rounding noise; continuous mode runs no baselines (tests/test_hip_parity.py)
    return ("y2.bias",) if m["use_binary"] else ("y2.bias", ".bs", ".br")


def _scopes(eng, call):
    eng.set_profiling(True)
    call()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _assert_generic(names, eng, extra=()):
    for k in ("k_bwd_conv", "k_wgrad") + tuple(extra):
        assert k in names, names
    assert [n for n in names if n.startswith("k_conversation")], names
    assert not [n for n in names if "game" in n or "tile" in n or "fast" in n or "persist" in n or "_mc" in n or "_rc" in n or "_wv" in n], names
    assert "family 3 " in eng.plan_text().splitlines()[0], eng.plan_text()


def _device_inputs(m, eng):
    x, target, desc, _ = common.case_inputs(m, 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    return d(x), d(target), d(desc)


def _train_case(name, m, wrap, setup, fused, monkeypatch):
    """One training minibatch of a plain, flipping or variant handle (common.hip_train_case: the phased step keeps every array
    exchange() returns, the fused step what training reads) against the oracle on the wrapped agents, through common.assert_parity."""
    us, want, flips = gi.oracle_minibatch(name, m, wrap)
    monkeypatch.setitem(common.U_OVERRIDES, name, lambda i, u_z, u_s, u_w: us)
    make = common.make_engine

    def make_engine(meta_, tweak=None, **over):
        eng = make(meta_, tweak=tweak, **over)
        if setup is not None:
            setup(eng)
        return eng
    monkeypatch.setattr(common, "make_engine", make_engine)
    if m["use_binary"] and not m["fixed_exchange"]:                     # rows of both kinds: stopped early (dead later), and never stopped
        tstar, n = gi.stop_steps(want)
        assert n == m["max_exchange"] and (tstar < n - 1).any() and (tstar == n - 1).any()
    got, eng = common.hip_train_case(name, m, fused=fused)
    pick = (lambda d: {k: d[k] for k in d if any(t in k for t in FUSED_KEEP)}) if fused else (lambda d: d)
    with gi.wrapped_agents(wrap):
        common.assert_parity(pick(got), pick(want), flips, eng, None, skip=_skip_keys(m), atol=ATOL, rtol=RTOL)
    xs = _device_inputs(m, eng)
    _assert_generic(_scopes(eng, lambda: eng.train_step(*xs, seed=SEED)), eng)
    return eng


# ------------------------------------------------------------------ 1. the control: a plain handle at W512
@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("mode", gi.MODES)
def test_plain_handle_at_512_threads(mode, fused, monkeypatch):
    """k_conversation<512> at dimensions that are no multiple of four (its GU = 8 row-pass tails), k_bwd_conv<false>."""
    m = gi.plain_meta("W512", mode, seed=gi.SEEDS["plain", mode])
    assert gi.conv_threads(**gi.dims_of(m)) == 512 and not gi.bwd_many(**gi.dims_of(m))
    _train_case("generic_plain_W512_" + mode, m, None, None, fused, monkeypatch)


# ------------------------------------------------------------------ 2. message flips at W512
@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
def test_flipping_handle_at_512_threads(fused, monkeypatch):
    """k_conversation<512, true>: sender and receiver flips, binary Adaptive; the oracle trained on the flipped messages."""
    m = gi.plain_meta("W512", seed=gi.SEEDS["flip"])
    assert gi.conv_threads(**gi.dims_of(m)) == 512
    us, want, _ = gi.oracle_minibatch("generic_flip_W512", m, gi.flip_wrap(m))
    n = int(want["mb0.n_steps"])
    assert (np.asarray(want["mb0.sen_feats"]) != (np.asarray(us[0])[:n] < np.asarray(want["mb0.sen_probs"]))).any()
    eng = _train_case("generic_flip_W512", m, gi.flip_wrap(m), lambda e: e.set_message_flipout(gi.P_SEN, gi.P_REC), fused, monkeypatch)
    assert eng.flipout == (gi.P_SEN, gi.P_REC, False)


def test_flipping_evaluation_at_512_threads():
    """An evaluation conversation under flipout_dev (streams 5 / 6): every row and every bit against the oracle wrapper (the data
    seed keeps every one of the 7 605 probabilities gi.EVAL_MARGIN away from 0.5: tests/generic_inst.py)."""
    m = gi.plain_meta("W512", seed=gi.EVAL_SEEDS["flip"])
    T, B, W = m["max_exchange"], m["batch"], m["rec_w_dim"]
    eng = common.make_engine(m)
    eng.set_message_flipout(gi.P_SEN, gi.P_REC, dev=True, eval_seed=gi.EVAL_SEED)
    xs = _device_inputs(m, eng)
    names = _scopes(eng, lambda: eng.eval_steps(xs[0], xs[1], xs[2], 1, 2, eng.eval_acc()))
    assert "k_conversation" in names and "k_eval_reduce" in names, names
    torch.cuda.synchronize()
    eng.check_sync()
    tp = {k: eng.tape[k].cpu().numpy().copy() for k in ("s", "ps", "z", "pz", "w", "pw", "y")}
    m_z, m_w = flipout_ref.flip_masks(gi.EVAL_SEED, 0, T, B, W, gi.P_SEN, gi.P_REC, flipout_ref.EVAL_STREAMS)
    assert m_z.any() and m_w.any()
    want = gi.once(("flip eval",), lambda: flipout_ref.conversation(m, m_z, m_w, train=False))
    for k in ("ps", "pz", "pw", "y"):
        print("flip eval %s: max |gpu - oracle| = %.3e" % (k, np.abs(tp[k].reshape(want[k].shape) - want[k]).max()))
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)
    prod = np.cumprod(want["ps"], 0)                                    # the stop bit rounds the running product (model.py:423-427)
    for bits, p in (("z", want["pz"]), ("w", want["pw"]), ("s", prod)):
        assert (np.abs(p - 0.5) > gi.EVAL_MARGIN).all()
        np.testing.assert_array_equal(tp[bits].reshape(p.shape), want[bits], err_msg=bits)
    np.testing.assert_array_equal(tp["z"], np.abs(np.round(tp["pz"]) - m_z))
    np.testing.assert_array_equal(tp["w"], np.abs(np.round(tp["pw"]) - m_w))


# ------------------------------------------------------------------ 3. sender variants at W512
@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("name", gi.VARIANTS_W512)
def test_variant_handle_at_512_threads(name, fused, monkeypatch):
    """k_conversation<512, false, true> with k_bwd_conv<false, SV_PROD / SV_IGNORE_CODE> (ignore_receiver alone: the plain one)."""
    setting = sv.SETTINGS[name]
    m = gi.plain_meta("W512", setting=setting, seed=gi.SEEDS["variant", name])
    assert gi.conv_threads(**gi.dims_of(m)) == 512
    eng = _train_case("generic_variant_W512_" + name, m, gi.variant_wrap(setting), lambda e: e.set_sender_variant(*setting), fused, monkeypatch)
    assert eng.sender_variant == setting
    if setting[2]:
        assert not eng.tape["w"].any()


# ------------------------------------------------------------------ 4. description attention at W512
def _compare_free_conversation(tp, want, binary, keys, label):
    """An evaluation conversation: values within ATOL, every bit exact (the seed keeps every probability gi.EVAL_MARGIN away from
    0.5, the stop probabilities of continuous messages 1e-4: tests/generic_inst.py)."""
    for k in (("ps", "pz", "pw", "y") if binary else ("ps", "z", "w", "y")) + keys:
        print("%s %s: max |gpu - oracle| = %.3e" % (label, k, np.abs(tp[k].reshape(want[k].shape) - want[k]).max()))
        np.testing.assert_allclose(tp[k].reshape(want[k].shape), want[k], atol=ATOL, rtol=0, err_msg=k)
    prod = np.cumprod(want["ps"], 0)
    for bits, p in ((("z", want["pz"]), ("w", want["pw"])) if binary else ()) + (("s", prod),):
        assert (np.abs(p - 0.5) > (gi.EVAL_MARGIN if binary else 1e-4)).all()
        np.testing.assert_array_equal(tp[bits].reshape(p.shape), want[bits], err_msg=bits)


@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("mode", gi.MODES)
def test_description_attention_at_512_threads(mode, fused):
    """k_conversation_attn<512>: the attention arrays sit behind the 4 * NT reduction area in LDS.  tests/test_desc_attn_gpu.py's
    comparison of a training minibatch, and the tape of its training conversation (alpha and dbar included) after the phased step."""
    m = gi.desc_meta(mode, seed=gi.SEEDS["desc", mode])
    assert gi.conv_threads(**gi.dims_of(m)) == 512 and m["desc_attn_dim"] == 10 and m["desc_set_lens"] == da.LENS_B
    us, res, models, flips = gi.attention_minibatch(da, m)
    assert not flips["pos"]
    want = gi.once(("desc packed", mode), lambda: cpu_ref.pack_train(res, models, prefix="mb0."))
    got, eng, before, names = tda._hip_minibatch(m, us, fused)
    _assert_generic(names, eng, ("k_attn_prep",))
    pick = (lambda d: {k: d[k] for k in d if any(t in k for t in FUSED_KEEP)}) if fused else (lambda d: d)
    skip = (".p.receiver.y2.bias", ".p.receiver.d_attn.bias") + (() if m["use_binary"] else ("mb0.bs", "mb0.br"))
    problems = common.compare_packed(pick(got), pick(want), atol=ATOL, rtol=RTOL, skip=skip)
    assert not problems, "\n".join(problems[:30])
    assert not eng.grads["receiver"]["d_attn.bias"].any() and torch.equal(eng.params["receiver"]["d_attn.bias"], before["d_attn.bias"])
    for name in ("d_d.weight", "d_h.weight", "d_attn.weight"):
        assert float(got["mb0.g.receiver.%s.norm" % name]) > 0, name
    if not fused:
        conv = gi.once(("desc conversation", mode), lambda: da.conversation(m, train=True, uniforms=us))
        tda._compare_conversation(tda._tape(eng), conv, binary=m["use_binary"], label="W512/" + mode)


@pytest.mark.parametrize("mode", ["adaptive", "continuous"])
def test_description_attention_evaluation_at_512_threads(mode):
    """(Fixed mode's evaluation conversation is Adaptive's: the same kernel arguments but for the masks.)"""
    m = gi.desc_meta(mode, seed=gi.EVAL_SEEDS["desc", mode])
    want = gi.once(("desc eval", mode), lambda: da.conversation(m, train=False))
    eng = tda._engine(m)
    xs, _ = tda._inputs(m, eng)
    names = _scopes(eng, lambda: eng.eval_steps(xs[0], xs[1], xs[2], 1, 2, eng.eval_acc()))
    assert "k_attn_prep" in names and "k_conversation" in names and "k_eval_reduce" in names, names
    _compare_free_conversation(tda._tape(eng), want, m["use_binary"], ("dbar", "alpha"), "W512 eval/" + mode)


# ------------------------------------------------------------------ 5. visual attention at W512;  8. at KM80 / KM272
def _vattn_minibatch(m, label):
    """tests/test_visual_attn_gpu.py's comparisons of one training minibatch: the tape of the training conversation (alpha, x_attn
    and h_x included), every gradient tensor and the six losses from the phased calls, the updated parameters from the fused step."""
    us, res, models, flips = gi.attention_minibatch(va, m)
    assert not flips["pos"]
    binary = m["use_binary"]
    eng, xs, ud, g = tv._phased_minibatch(m, us)
    conv = gi.once(("vattn conversation", label), lambda: va.conversation(m, train=True, uniforms=us))
    tp = tv._tape(eng)
    tv._compare_conversation(tp, conv, binary=binary, train=True, label=label)
    n_loc = tp["alpha"].shape[-1]
    assert (tp["alpha"][0] == np.float32(1.0) / np.float32(n_loc)).all() and np.abs(tp["alpha"][1:] - 1.0 / n_loc).max() > 1e-2
    got = tv._grads(eng)
    for a in (("receiver", "sender", "baseline_rec", "baseline_sen") if binary else ("receiver",)):
        for k, v in res["grads"][a].items():
            if (a, k) == ("sender", "attn_U.bias"):
                continue
            tv._assert_close(got[a][k].reshape(tuple(v.shape)), v.numpy(), "%s gradient %s.%s" % (label, a, k))
    if binary:
        sg = got["sender"]
        assert not sg["attn_U.bias"].any()
        np.testing.assert_array_equal(sg["attn_W_x.bias"], sg["attn_W_w.bias"])
        np.testing.assert_array_equal(sg["attn_W_x.bias"], sg["attn_W_g.bias"])
        assert np.abs(sg["attn_W_x.weight"]).max() > 1e-4 and np.abs(sg["attn_U.weight"]).max() > 1e-4
    losses = {k: float(res[k].detach()) for k in tv.LOSS_KEYS}
    got_l = eng.losses()
    for k in tv.LOSS_KEYS:
        assert abs(got_l[k] - losses[k]) <= 1e-4 + 1e-3 * abs(losses[k]), ("phased", k, got_l[k], losses[k])
    feng = tv._engine(m)
    start = {a: {k: v.clone() for k, v in d.items()} for a, d in feng.params.items()}
    xs, ud, g = tv._inputs(m, feng, us)
    feng.set_data_context(g)
    names = _scopes(feng, lambda: feng.train_step(*xs, *ud, seed=SEED))
    _assert_generic(names, feng, ("k_vattn_prep", "k_conversation_vattn") + (("k_vattn_bwd", "k_vattn_dwx") if binary else ()))
    assert "k_conversation" not in names, names
    got_l = feng.losses()
    for k in tv.LOSS_KEYS:
        assert abs(got_l[k] - losses[k]) <= 1e-4 + 1e-3 * abs(losses[k]), ("fused", k, got_l[k], losses[k])
    for a, d in feng.params.items():
        for k, v in d.items():
            if not (binary or a == "receiver") or (a, k) == ("sender", "attn_U.bias"):
                assert torch.equal(v, start[a][k]), (a, k)               # bit-identical
            elif (a, k) not in tv.NOISE:
                w = models[a].state_dict()[k].detach().numpy()
                tv._assert_close(v.cpu().numpy().reshape(w.shape), w, "%s updated %s.%s" % (label, a, k))
    moved = ("receiver", "rnn.weight_hh") if not binary else ("sender", "attn_W_x.weight")
    assert not torch.equal(feng.params[moved[0]][moved[1]], start[moved[0]][moved[1]])


@pytest.mark.parametrize("mode", gi.MODES)
def test_visual_attention_at_512_threads(mode):
    """k_conversation_vattn<512> with the context (C = 18, A = 5, a 2 x 3 map, G = 7)."""
    m = gi.vattn_meta("W512", mode, seed=gi.SEEDS["vattn", mode])
    assert gi.conv_threads(**gi.dims_of(m)) == 512
    assert (m["img_feat_dim"], m["vattn_dim"], m["map_hw"], m["context_dim"]) == (18, 5, [2, 3], 7)
    _vattn_minibatch(m, "vattn W512/" + mode)


@pytest.mark.parametrize("kind", sorted(gi.KM))
def test_kmajor_gemm_float4_branch_at_ragged_edges(kind):
    """gemm_kmajor_tile's float4 branch (C % 16 == 0) with a partial last pass, idle waves and both output-tile edges ragged: the
    HX / HG tables k_vattn_prep leaves on the tape against a float64 product of the same map and weights, then a training minibatch."""
    m = gi.vattn_meta(kind, seed=gi.SEEDS[kind, "adaptive"])
    C, A, (h, w), B = m["img_feat_dim"], m["vattn_dim"], m["map_hw"], m["batch"]
    assert C == gi.KM[kind] and C % 16 == 0 and (A, h * w, B) == (20, 5, 5) and gi.conv_threads(**gi.dims_of(m)) == 256
    eng = tv._engine(m)
    xs, _, g = tv._inputs(m, eng)
    eng.set_data_context(g)
    names = _scopes(eng, lambda: eng.forward(*xs, train=False, run_all=True))
    assert "k_vattn_prep" in names, names
    tp = tv._tape(eng, ("vattn_HX", "vattn_HG"))
    sd = va.state_dicts(m)["sender"]
    f = lambda k: np.asarray(sd[k], np.float64)
    x, ctx = va.feature_map(m)
    X = np.asarray(x, np.float64).reshape(B, C, h * w)
    hx = np.einsum("bci,ac->bia", X, f("attn_W_x.weight")) + f("attn_W_x.bias")
    hg = np.asarray(ctx, np.float64) @ f("attn_W_g.weight").T + f("attn_W_g.bias")
    for got, want, k in ((tp["vattn_HX"], hx, "HX"), (tp["vattn_HG"], hg, "HG")):
        print("%s %s: max |gpu - float64| = %.3e (largest |v| %.3e)" % (kind, k, np.abs(got.reshape(want.shape) - want).max(), np.abs(want).max()))
        np.testing.assert_allclose(got.reshape(want.shape), want, atol=ATOL, rtol=0, err_msg=k)
    assert np.abs(hx).max() > 0.5                                        # (a dropped chunk of 16 channels is far outside ATOL)
    _vattn_minibatch(m, "vattn " + kind)


# ------------------------------------------------------------------ 6. a plain handle at B513;  7. sender variants at B513
@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("mode", ["adaptive", "continuous"])
@pytest.mark.parametrize("T", [3, 4])
def test_plain_handle_at_513_samples(T, mode, fused, monkeypatch):
    """k_bwd_conv<true> (TU = 2, gemv_rows<2>); T = 4: T * B = 2052 rows also cross k_wgrad's 2048-row split.  Adaptive: samples
    that stopped early leave dead rows behind."""
    monkeypatch.setenv("MMG_NO_TILE", "1")
    m = gi.plain_meta("B513", mode, T, seed=gi.SEEDS["b513", T, mode])
    assert gi.bwd_many(**gi.dims_of(m)) and gi.conv_threads(**gi.dims_of(m)) == 256 and (T < 4 or T * m["batch"] > 2048)
    _train_case("generic_plain_B513_T%d_%s" % (T, mode), m, None, None, fused, monkeypatch)


@pytest.mark.parametrize("fused", STEP, ids=STEP_IDS)
@pytest.mark.parametrize("name", gi.VARIANTS_B513)
def test_variant_handle_at_513_samples(name, fused, monkeypatch):
    """k_bwd_conv<true, SV_PROD>, k_bwd_conv<true, SV_IGNORE_CODE>; ignore_receiver alone takes the plain k_bwd_conv<true> (the
    tape holds the zeros)."""
    setting = sv.SETTINGS[name]
    m = gi.plain_meta("B513", "adaptive", 3, setting=setting, seed=gi.SEEDS["b513", name])
    assert gi.bwd_many(**gi.dims_of(m))
    eng = _train_case("generic_variant_B513_" + name, m, gi.variant_wrap(setting), lambda e: e.set_sender_variant(*setting), fused, monkeypatch)
    assert eng.sender_variant == setting
