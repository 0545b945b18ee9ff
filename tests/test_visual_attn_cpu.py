"""Visual attention without a GPU: the wrapped oracle (tests/visual_attn_ref.py) against the g13 fixtures the reference's own code
produced, the float64 restatement against the wrapped oracle, the layout twins of the ABI, the module, the refusals with their
messages, and the conditions the GPU comparisons rely on (so that none of them can pass vacuously)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, agents, flags as F, game as G, misc
from oracle import PORTABLE_FP_ENV
from tests import common, visual_attn_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(ref.MODES)
SHAPES = sorted(ref.SHAPES)
C1 = (64, 30, 512, 256, 32, 64, 100, 500, 10)


# ------------------------------------------------------------------ the wrapped oracle against the reference's own numbers
@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """The three modes' training-mode conversation (the fixture's uniforms) and evaluation conversation from the wrapped oracle,
    in one child process under oracle.PORTABLE_FP_ENV (the environment the fixtures were generated in; it has to be in place
    before torch loads)."""
    out = str(tmp_path_factory.mktemp("visual_attn") / "oracle.npz")
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, torch; torch.set_num_threads(1); "
            "from tests import common, visual_attn_ref as ref; d = {}\n"
            "for mode in ref.MODES:\n"
            "    z, meta = ref.load_golden('g13_visual_attn_' + mode)\n"
            "    u = common.case_inputs(meta, 0)[3]\n"
            "    tp = ref.conversation(meta, train=True, uniforms=u)\n"
            "    packed = {'train.' + k: v for k, v in tp.items()}\n"
            "    packed.update(ref.eval_case(meta))\n"
            "    d.update({mode + '/' + k: v for k, v in packed.items()})\n"
            "np.savez(%r, **d)" % (REPO, out))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + ["-c", code], env=dict(os.environ, **PORTABLE_FP_ENV), cwd=REPO,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("mode", MODES)
def test_wrapped_oracle_matches_the_reference(mode, oracle_runs):
    """tests/test_oracle_golden.py's tolerances for g2 / g3 (atol 2e-6, rtol 2e-5), on the evaluation conversation and on every
    executed step of the training-mode conversation: messages, probabilities, logits, both baselines' scores, alpha, x_attn."""
    got = {k[len(mode) + 1:]: v for k, v in oracle_runs.items() if k.startswith(mode + "/")}
    z, meta = ref.load_golden("g13_visual_attn_%s_eval" % mode)
    assert (meta["vattn_dim"], meta["map_hw"], meta["context_dim"], meta["img_feat_dim"]) == (256, [8, 8], 1000, 512)
    n = int(z["eval.n_steps"])
    ev = {k: v for k, v in got.items() if k.startswith("eval.")}
    ev["eval.x_attn"] = ev["eval.x_attn"][:, :, ::8]
    assert z["eval.x_attn"].shape == (n, 16, 64)                          # every sample, every 8th channel
    problems = common.compare_packed(ev, z, atol=2e-6, rtol=2e-5, ulps=1)
    assert not problems, "\n".join(problems[:20])
    assert n > 1 and z["eval.alpha"].shape == (n, 16, 64)
    z, meta = ref.load_golden("g13_visual_attn_" + mode)
    n = int(z["mb0.n_steps"])
    binary = meta["use_binary"]
    pairs = [("s", "s_feats"), ("ps", "s_probs"), ("z", "sen_feats"), ("w", "rec_feats"), ("y", "y"), ("alpha", "alpha")]
    pairs += [("pz", "sen_probs"), ("pw", "rec_probs"), ("bs", "bs"), ("br", "br")] if binary else []
    for k, zk in pairs:
        want = z["mb0." + zk]
        np.testing.assert_allclose(got["train." + k][:n].reshape(want.shape), want, atol=2e-6, rtol=2e-5, err_msg=k)
    xa = z["mb0.x_attn"]
    np.testing.assert_allclose(got["train.x_attn"][:n, :, ::8], xa, atol=2e-6, rtol=2e-5)


def test_fixtures_record_what_they_claim():
    for mode in MODES:
        z, meta = ref.load_golden("g13_visual_attn_" + mode)
        e, _ = ref.load_golden("g13_visual_attn_%s_eval" % mode)
        for f in ("g13_visual_attn_" + mode, "g13_visual_attn_%s_eval" % mode):
            assert os.path.getsize(os.path.join(common.GOLDEN_DIR, f + ".npz")) <= 200 * 1024, f
        assert int(z["mb0.n_steps"]) >= 2 and int(e["eval.n_steps"]) > 1
        assert meta["use_binary"] == ref.MODES[mode]["use_binary"] and meta["fixed_exchange"] == ref.MODES[mode]["fixed_exchange"]
        n = z["mb0.alpha"].shape[-1]
        assert (z["mb0.alpha"][0] == np.float32(1.0) / np.float32(n)).all() and (e["eval.alpha"][0] == np.float32(1.0) / np.float32(n)).all()
        assert np.abs(z["mb0.alpha"][1:] - 1.0 / n).max() > 1e-2 and np.abs(e["eval.alpha"][1:] - 1.0 / n).max() > 1e-2
        if not meta["use_binary"]:
            continue
        names = ref.vattn_names(meta)                                     # the reference trained the attention tensors ...
        assert len(names) == 8
        for name in names:
            assert "mb0.g.sender.%s.norm" % name in z and "mb0.p.sender.%s.sample" % name in z
        for name in ("attn_W_x.weight", "attn_W_w.weight", "attn_W_g.weight", "attn_U.weight"):
            assert float(z["mb0.g.sender.%s.norm" % name]) > 1e-8, (mode, name)
        # ... except attn_U.bias, a shift of every score of a softmax: what the reference's autograd leaves there is rounding noise;
        assert float(z["mb0.g.sender.attn_U.bias.norm"]) < 1e-6
        # and the three biases that add into the same pre-activation share one gradient
        gb = [z["mb0.g.sender.attn_W_%s.bias.sample" % k] for k in "xwg"]
        np.testing.assert_allclose(gb[0], gb[1], atol=1e-6, rtol=0)
        np.testing.assert_allclose(gb[0], gb[2], atol=1e-6, rtol=0)


@pytest.mark.parametrize("shape", ["B", "C", "E"])
def test_float64_restatement_matches_the_wrapped_oracle(shape):
    """forward_f64 (numpy, from the formulas alone) against the oracle's sender, step by step, within fp32 rounding (1e-5)."""
    m = ref.meta(shape)
    tp = ref.conversation(m, train=False)
    sd = ref.state_dicts(m)["sender"]
    x, g = ref.feature_map(m)
    for t in range(m["max_exchange"]):
        w = tp["w"][t - 1] if t else np.zeros((m["batch"], m["rec_w_dim"]), np.float32)
        alpha, x_attn, h_x = ref.forward_f64(sd, x, g, w, t)
        for got, want in ((alpha, tp["alpha"][t]), (x_attn, tp["x_attn"][t]), (h_x, tp["h_x"][t])):
            np.testing.assert_allclose(got, want, atol=1e-5, rtol=0)


@pytest.mark.parametrize("shape", ["B", "C", "D"])
def test_hand_written_backward_matches_autograd_in_float64(shape):
    """backward_f64 (the kernels' formulas: dx_attn, dalpha, dbeta, u, dq, and the eight gradients) against torch autograd over the
    literal statement, both in float64: 1e-12 relative to each tensor's largest entry.  attn_U.bias: exact zeros by hand, rounding
    noise (< 1e-12) from autograd; the three biases share one gradient; at t == 0 only image_layer gets one."""
    m = ref.meta(shape)
    sd = ref.state_dicts(m)["sender"]
    x, g = ref.feature_map(m)
    rs = np.random.RandomState(3)
    w = (rs.rand(m["batch"], m["rec_w_dim"]) > 0.5).astype(np.float32)
    dh = rs.standard_normal((m["batch"], m["img_h_dim"]))
    for t in (0, 1, 2):
        hand, auto = ref.backward_f64(sd, x, g, w, t, dh), ref.autograd_f64(sd, x, g, w, t, dh)
        assert set(hand) == set(auto)
        for k in hand:
            if k == "attn_U.bias":
                assert not hand[k].any() and np.abs(auto[k]).max() < 1e-12
                continue
            scale = np.abs(auto[k]).max()
            assert np.abs(hand[k] - auto[k]).max() <= 1e-12 * max(scale, 1e-30), (k, t)
            live = t > 0 and m["map_hw"] != [1, 1]
            assert (scale > 1e-6) == (live or k.startswith("image_layer")), (k, t, scale)
        np.testing.assert_array_equal(hand["attn_W_x.bias"], hand["attn_W_w.bias"])


def test_oracle_training_reproduces_the_references_gradients():
    """tests/visual_attn_ref.train_minibatches (what the GPU gradients are held against) against g13: the norm and the strided
    sample of every sender tensor's gradient, within the oracle <-> golden bar (atol 2e-6, rtol 2e-5)."""
    z, m = ref.load_golden("g13_visual_attn_fixed")
    res, _ = ref.train_minibatches(m, [common.case_inputs(m, 0)[3]], update=False)
    grads = res[0]["grads"]["sender"]
    for name in ref.vattn_names(m) + ("image_layer.weight", "binary_layer.weight"):
        flat = grads[name].numpy().reshape(-1)
        np.testing.assert_allclose(flat[::max(1, flat.size // 512)], z["mb0.g.sender.%s.sample" % name], atol=2e-6, rtol=2e-5, err_msg=name)


@pytest.mark.parametrize("mode", MODES)
def test_oracle_minibatch_with_its_update_reproduces_the_reference(mode):
    """The oracle's minibatch WITH the update (what the GPU's updated parameters are held against) against g13: the six losses and
    the strided sample of every updated tensor, within the oracle <-> golden bar.  Two tensors are left out, and this is where the
    reason is measured: attn_U.bias and receiver.y2.bias have gradients that vanish in exact arithmetic (a shift of every score of
    a softmax / of every class logit), the optimizers step on what rounding leaves, and the ORACLE and the REFERENCE -- the same
    formulas on the same library -- already disagree on them by more than the bar."""
    z, m = ref.load_golden("g13_visual_attn_" + mode)
    res, models = ref.train_minibatches(m, [common.case_inputs(m, 0)[3]], update=True)
    keys = ("nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen", "loss_bas_rec", "loss_bas_sen")
    np.testing.assert_allclose([float(res[0][k].detach()) for k in keys], z["mb0.losses"], atol=2e-6, rtol=2e-5)
    agents_ = ("receiver", "sender", "baseline_rec", "baseline_sen") if m["use_binary"] else ("receiver",)
    seen = 0
    for a in agents_:
        for k, v in models[a].state_dict().items():
            flat = v.numpy().reshape(-1)
            err = np.abs(flat[::max(1, flat.size // 512)] - z["mb0.p.%s.%s.sample" % (a, k)]).max()
            if (a, k) in (("sender", "attn_U.bias"), ("receiver", "y2.bias")):
                assert err < 1e-3                                         # (a step of the size of the learning rate at the most)
                continue
            assert err <= 2e-6 + 2e-5 * np.abs(flat).max(), (a, k, err)
            seen += 1
    assert seen == (15 + 15 + 4 + 4 - 2 if m["use_binary"] else 14)       # receiver 15, sender 7 + 8, the baselines 4 each


# ------------------------------------------------------------------ what the GPU comparisons rely on
@pytest.mark.parametrize("shape", SHAPES)
def test_evaluation_seeds_leave_no_bit_out_and_attention_matters(shape):
    m = ref.meta(shape)
    tp = ref.conversation(m, train=False)
    prod = np.cumprod(tp["ps"], 0)
    for p in (tp["pz"], tp["pw"], prod):
        assert (np.abs(p - 0.5) > 1e-4).all()
    n = tp["alpha"].shape[-1]
    assert n == m["map_hw"][0] * m["map_hw"][1]
    np.testing.assert_allclose(tp["alpha"].sum(-1), 1.0, atol=1e-6)
    assert (tp["alpha"][0] == np.float32(1.0) / np.float32(n)).all()
    if n == 1:
        assert (tp["alpha"] == 1.0).all()
    else:                                                                 # otherwise a kernel that ignores the scores passes
        assert np.abs(tp["alpha"][1:] - 1.0 / n).max() > 1e-2


@pytest.mark.parametrize("shape", ["A", "B"])
def test_separated_uniforms_keep_the_trajectory_and_the_margin(shape):
    m = ref.meta(shape)
    u0 = common.case_inputs(m, 0)[3]
    u = ref.separated_uniforms(m)
    a, b = ref.conversation(m, train=True, uniforms=u0), ref.conversation(m, train=True, uniforms=u)
    for k in ("s", "z", "w"):
        np.testing.assert_array_equal(a[k], b[k])
    for k, uu in zip(("pz", "ps", "pw"), u):
        assert (np.abs(np.asarray(uu).reshape(b[k].shape) - b[k]) >= 1e-4 - 1e-7).all()
    n = b["alpha"].shape[-1]
    assert np.abs(b["alpha"][1:] - 1.0 / n).max() > 1e-2                  # attention matters in the training conversation too


def test_a_transposed_map_is_far_outside_the_tolerance():
    """x is channel-major: reading the same memory as [B, N, C] moves x_attn and h_x by more than 1e-2 (2 x 3 map, C = 18)."""
    m = ref.meta("B")
    right, wrong = ref.conversation(m, train=False), ref.conversation(m, train=False, transposed=True)
    assert np.abs(right["x_attn"] - wrong["x_attn"]).max() > 1e-2 and np.abs(right["h_x"] - wrong["h_x"]).max() > 1e-2
    x, _ = ref.feature_map(m)                                             # t == 0: x_attn is the mean over the LOCATIONS
    np.testing.assert_allclose(right["x_attn"][0], x.reshape(5, 18, 6).mean(-1), atol=1e-6)


# ------------------------------------------------------------------ the ABI: twins, the tensors, the supported range
def _cfg(batch, n_classes, F_, H, W, R, V, K, T, **over):
    kw = dict(batch=batch, n_classes=n_classes, feat_dim=F_, h_dim=H, w_dim=W, rec_hidden=R, wv_dim=V, bas_hidden=K, max_exchange=T,
              use_binary=True, fixed_exchange=False, s_prob_prod=True, entropy_s=0.08, entropy_sen=0.01, entropy_rec=0.01,
              first_rec=0.0, optim_type="RMSprop", learning_rate=1e-4, top_k=6)
    kw.update(over)
    return _lib.make_config(**kw)


def test_twins_with_attn_dim_zero_equal_the_plain_queries():
    lib = _lib.load()
    assert lib.mmg_version() == 3
    for dims in (C1, (5, 7, 18, 40, 12, 20, 12, 70, 3)):
        cfg = _cfg(*dims)
        for n_feats, ctx in ((0, 0), (64, 1000)):
            assert lib.mmg_vattn_param_count(C.byref(cfg), 0, n_feats, ctx) == lib.mmg_param_count(C.byref(cfg))
            assert lib.mmg_vattn_grad_floats(C.byref(cfg), 0, n_feats, ctx) == lib.mmg_grad_floats(C.byref(cfg))
            assert lib.mmg_vattn_workspace_bytes(C.byref(cfg), 0, n_feats, ctx) == lib.mmg_workspace_bytes(C.byref(cfg))
            assert _lib.param_table(cfg, vattn=(0, n_feats, ctx)) == _lib.param_table(cfg)
            assert _lib.tape_table(cfg, vattn=(0, n_feats, ctx)) == _lib.tape_table(cfg)
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    for sym in ("mmg_vattn_param_count", "mmg_vattn_param_table", "mmg_vattn_grad_floats", "mmg_vattn_workspace_bytes",
                "mmg_vattn_tape_table", "mmg_vattn_create", "mmg_set_data_context", "mmg_vattn_reset_state"):
        assert sym in _lib.SYMBOLS and sym + "(" in header and hasattr(lib, sym)


@pytest.mark.parametrize("ctx", [0, 1000])
def test_the_attention_tensors_lie_inside_the_senders_range(ctx):
    cfg = _cfg(*C1)
    plain, table = _lib.param_table(cfg), _lib.param_table(cfg, vattn=(256, 64, ctx))
    names = [e["name"] for e in table if e["agent"] == "sender"]
    want = list(ref.VATTN_NAMES) + (list(ref.VATTN_CTX_NAMES) if ctx else [])
    assert names[:7] == [e["name"] for e in plain if e["agent"] == "sender"] and names[7:] == want       # model.py:80-86 order
    shapes = {e["name"]: (e["rows"], e["cols"]) for e in table if e["agent"] == "sender"}
    assert shapes["attn_W_x.weight"] == (256, 512) and shapes["attn_W_w.weight"] == (256, 32) and shapes["attn_U.weight"] == (1, 256)
    assert shapes["attn_U.bias"] == (1, 0) and (not ctx or shapes["attn_W_g.weight"] == (256, 1000))
    offs = [e["offset"] for e in table]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs)
    extra = sum(((e["rows"] * max(e["cols"], 1) + 3) // 4) * 4 for e in table if e["name"] in want and e["agent"] == "sender")
    for a, b in zip(plain, [e for e in table if not (e["agent"] == "sender" and e["name"] in want)]):
        moved = extra if a["agent"].startswith("baseline") else 0        # the receiver and the sender's seven stay, the others move up
        assert (a["name"], a["agent"], a["rows"], a["cols"]) == (b["name"], b["agent"], b["rows"], b["cols"]) and b["offset"] == a["offset"] + moved
    assert _lib.load().mmg_vattn_param_count(C.byref(cfg), 256, 64, ctx) == _lib.load().mmg_param_count(C.byref(cfg)) + extra
    tape = {e["name"]: e["dims"] for e in _lib.tape_table(cfg, vattn=(256, 64, ctx))}
    assert tape["vattn_HX"] == [64, 64, 256] and tape["vattn_alpha"] == [10, 64, 64] and tape["vattn_xa"] == [10, 64, 512]
    assert tape["vattn_hx"] == [10, 64, 256] and tape["vattn_HG"] == [64, 256]
    assert [e for e in _lib.tape_table(cfg)] == _lib.tape_table(cfg, vattn=(256, 64, ctx))[:len(_lib.tape_table(cfg))]


@pytest.mark.parametrize("vattn, dims, word", [((257, 64, 0), C1, "attn_dim"), ((-1, 64, 0), C1, "attn_dim"), ((256, 0, 0), C1, "n_feats"),
                                               ((256, 257, 0), C1, "n_feats"), ((256, 64, 4097), C1, "context_dim"),
                                               ((256, 64, -1), C1, "context_dim"), ((256, 64, 0), (513,) + C1[1:], "batch must be"),
                                               ((256, 64, 0), C1[:2] + (4097,) + C1[3:], "feat_dim")])
def test_outside_the_supported_range_is_an_error_with_a_message(vattn, dims, word):
    lib = _lib.load()
    cfg = _cfg(*dims)
    for fn in (lib.mmg_vattn_param_count, lib.mmg_vattn_grad_floats, lib.mmg_vattn_workspace_bytes):
        assert fn(C.byref(cfg), *vattn) < 0
        msg = lib.mmg_last_error().decode()
        assert "visual_attn" in msg and __import__("re").search(word, msg), msg
    with pytest.raises(_lib.MmgError, match="visual_attn"):
        _lib.param_table(cfg, vattn=vattn)


def test_the_edges_of_the_supported_range_are_accepted():
    lib = _lib.load()
    # (the presets' shape at 512 samples; the smallest; the largest of every bound at once: batch * n_feats * attn_dim == 2^25 there)
    for vattn, dims in (((256, 64, 1000), (512,) + C1[1:]), ((1, 1, 0), C1), ((256, 256, 4096), (512, 30, 4096) + C1[3:])):
        assert vattn[0] * vattn[1] * dims[0] <= _lib.VATTN_MAX_HX
        assert lib.mmg_vattn_param_count(C.byref(_cfg(*dims)), *vattn) > 0, lib.mmg_last_error()
    assert lib.mmg_vattn_param_count(C.byref(_cfg(*C1, global_batch=128)), 256, 64, 0) < 0 and b"one GPU" in lib.mmg_last_error()
    assert (_lib.VATTN_MAX_DIM, _lib.VATTN_MAX_FEATS, _lib.VATTN_MAX_CTX, _lib.VATTN_MAX_BATCH) == (256, 256, 4096, 512)


# ------------------------------------------------------------------ Python: the module, the refusals
def _agents(use_attn=True, ctx=True, use_binary=True, desc_attn=False):
    s = agents.Sender("layer4_2", 512, 256, 32, 32, use_binary, use_attn=use_attn, attn_dim=256, attn_extra_context=ctx,
                      attn_context_dim=1000)
    r = agents.Receiver(32, 100, 64, 1, 32, 1, use_binary, desc_attn=desc_attn)
    return s, r, agents.Baseline(500, 256, 32, 0), agents.Baseline(500, 0, 32, 64)


class _Flags(object):
    desc_attn, sender_mix, flipout_sen, flipout_rec = False, "sum", None, None
    ignore_receiver = ignore_code = visual_attn = bit_flip = False
    max_exchange, fixed_exchange, s_prob_prod = 4, False, True
    entropy_s = entropy_sen = entropy_rec = None
    first_rec, optim_type, learning_rate, top_k_train = 0.0, "RMSprop", 1e-4, 6


def test_sender_module_owns_the_tensors_under_the_reference_names_and_order():
    """state_dict order behind binary_layer.* as the reference's (model.py:80-86): attn_W_x, attn_W_w, attn_U, then attn_W_g."""
    torch.manual_seed(3)
    s = _agents()[0]
    names = list(s.state_dict().keys())
    assert names[-8:] == list(ref.VATTN_NAMES + ref.VATTN_CTX_NAMES) and len(names) == 15
    assert names[-10:-8] == ["binary_layer.weight", "binary_layer.bias"]
    assert tuple(s.attn_W_x.weight.shape) == (256, 512) and tuple(s.attn_W_w.weight.shape) == (256, 32)
    assert tuple(s.attn_U.weight.shape) == (1, 256) and tuple(s.attn_W_g.weight.shape) == (256, 1000)
    for lin in (s.attn_W_x, s.attn_W_w, s.attn_U, s.attn_W_g):           # model.py:90-95: Xavier-normal weights, zero biases
        assert not lin.bias.any()
        std, want = float(lin.weight.detach().std()), (2.0 / sum(lin.weight.shape)) ** 0.5
        assert 0.6 * want < std < 1.5 * want
    assert s.vattn == (256, 1000) and s.attn_scores == []
    six = _agents(ctx=False)[0]
    assert list(six.state_dict().keys())[-6:] == list(ref.VATTN_NAMES) and len(six.state_dict()) == 13 and six.vattn == (256, 0)
    plain = _agents(use_attn=False)[0]
    assert len(plain.state_dict()) == 7 and plain.vattn is None
    with pytest.raises(NotImplementedError, match="attn_dim"):
        agents.Sender("layer4_2", 512, 256, 32, 32, True, use_attn=True, attn_dim=257)
    with pytest.raises(NotImplementedError, match="attn_context_dim"):
        agents.Sender("layer4_2", 512, 256, 32, 32, True, use_attn=True, attn_extra_context=True, attn_context_dim=5000)


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(4)
    s = _agents()[0]
    path = str(tmp_path / "sender.pt")
    misc.torch_save(path, dict(step=3), dict(sender=s), {})
    t = _agents()[0]
    assert not torch.equal(t.attn_W_x.weight, s.attn_W_x.weight)
    assert misc.torch_load(path, dict(sender=t), {}) == dict(step=3)
    sd = t.state_dict()
    assert list(sd.keys()) == list(s.state_dict().keys())
    for k, v in s.state_dict().items():
        assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("kw, word", [(dict(autograd=True), "autograd"), (dict(autograd=True, channel_grad=True), "autograd"),
                                      (dict(input_grad=True), "input_grad"), (dict(channel_grad=True), "channel_grad"),
                                      (dict(flipout_sen=0.1), "flips"), (dict(flipout_rec=0.1), "flips"),
                                      (dict(sender_mix="prod"), "sender variant"), (dict(ignore_receiver=True), "sender variant")])
def test_game_refuses_what_attention_does_not_combine_with(kw, word):
    with pytest.raises(NotImplementedError, match="visual attention") as e:
        G.Game(*_agents(), flags=_Flags(), device="cpu", **kw)
    assert word in str(e.value)
    G.Game(*_agents(use_attn=False), flags=_Flags(), device="cpu", **kw)        # (the plain game takes every one of them)


def test_game_refuses_the_rest_with_a_message():
    with pytest.raises(NotImplementedError, match="visual attention with description attention"):
        G.Game(*_agents(desc_attn=True), flags=_Flags(), device="cpu")
    g = G.Game(*_agents(), flags=_Flags(), device="cpu")
    assert g.vattn == (256, 1000)
    with pytest.raises(NotImplementedError, match="visual attention.*world > 1"):
        g.set_parallel(0, 2)
    fl = _Flags()
    fl.visual_attn = True                                                 # the switch stays refused, and names the library option
    with pytest.raises(NotImplementedError, match="-visual_attn"):
        G.Game(*_agents(), flags=fl, device="cpu")
    entry = [u for u in F.UNSUPPORTED if u[0] == "visual_attn"][0]
    assert "use_attn=True" in entry[2] and "data_context" in entry[2] and "model.py:114" in entry[2]
    x, ctx, desc, target = torch.zeros(4, 512, 8, 8), torch.zeros(4, 1000), torch.zeros(30, 100), torch.zeros(4, dtype=torch.int64)
    for data, context, err, word in ((x.view(4, 512, 64), ctx, ValueError, r"\[B, 512, h, w\]"), (x[:, :500], ctx, ValueError, "channels"),
                                     (x, None, ValueError, "data_context"), (x, ctx[:, :999], ValueError, "data_context must be"),
                                     (torch.zeros(4, 512, 17, 17), ctx, NotImplementedError, "h \\* w must be"),
                                     (torch.zeros(600, 512, 1, 1), torch.zeros(600, 1000), NotImplementedError, "batch <= 512")):
        with pytest.raises(err, match=word):
            g.exchange(dict(data=data, target=target, desc=desc, train=False, data_context=context))
    for call in (lambda: g.train_step(x, target, desc), lambda: g.train_steps(x, target, desc, 1),
                 lambda: g.train_step(x.view(4, -1), target, desc, data_context=ctx)):      # training checks its inputs the same way
        with pytest.raises(ValueError, match=r"data_context|\[B, 512, h, w\]"):
            call()
    with pytest.raises(NotImplementedError, match="autograd"):
        g.exchange(dict(data=x, target=target, desc=desc, train=True, data_context=ctx, autograd=True))
    plain = G.Game(*_agents(use_attn=False), flags=_Flags(), device="cpu")
    with pytest.raises(NotImplementedError, match="use_attn=True"):
        plain.exchange(dict(data=torch.zeros(4, 512), target=target, desc=desc, train=False, data_context=ctx))
    six = G.Game(*_agents(ctx=False), flags=_Flags(), device="cpu")
    assert six.check_context(torch.zeros(4, 3), 4) is None                # a sender without attn_W_g ignores what it is given
