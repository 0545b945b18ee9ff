"""Gaussian message noise on continuous messages (include/mmg.h: mmg_set_message_noise), what needs no GPU:

1. tests/noise_ref.philox_normal, the restatement of the library's draws: moments, range, the four streams.
2. The oracle wrapper (noise_ref.noise_agents): sigma 0 is cpu_ref.exchange, sigma > 0 adds sigma * n[0] to the first message and
   moves every later logit.
3. The reach conditions of tests/test_channel_noise_gpu.py's cases, asserted on the oracle: the Adaptive case stops early and late,
   no stop draw within 1e-4 of its probability, no evaluation stop-probability product within 1e-4 of 0.5.
4. Game's arguments on device="cpu".
5. mmg_plan_for with the noise bit: the generic family at config 1's shape, mc3 kept and mc3p cleared at the many-class shapes,
   and the recorded text without the bit."""
import inspect

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import common, noise_ref as nr
from tests.test_channel_grad_cpu import TINY
from tests.test_plan_cpu import SHAPES, caps_line, entry, plan, switches  # noqa: F401  (switches: a fixture)


# ------------------------------------------------------------------ 1. the draws
def test_philox_normal_moments_range_and_streams():
    e = np.arange(100000, dtype=np.uint32)
    n, x0, _ = nr.philox_normal(21, e, 1, 7)
    # six and about four standard errors of the two statistics over 100 000 draws (0.0032 and 0.0045)
    assert abs(n.mean()) < 0.02 and 0.98 < n.var() < 1.02, (n.mean(), n.var())
    assert np.abs(n).max() <= 5.78                                   # sqrt(-2 ln 2^-24) = 5.768
    u1 = ((x0 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    assert u1.min() > 0.0 and u1.max() <= 1.0
    fields = [nr.philox_normal(21, e, 1, s)[0] for s in nr.TRAIN_STREAMS + nr.EVAL_STREAMS]
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.abs(fields[i] - fields[j]).max() > 1.0 and abs(np.corrcoef(fields[i], fields[j])[0, 1]) < 0.02
    # the first word is the one philox_uniform keeps
    from tests import philox_ref
    np.testing.assert_array_equal((x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), philox_ref.philox_uniform(21, e, 1, 7))
    # the extreme words: u1 = 2^-24 gives the largest |n|, u1 = 1 gives 0
    assert np.sqrt(-2.0 * np.log(2.0 ** -24)) < 5.78


def test_noise_fields_index_the_global_batch():
    n_z, n_w = nr.noise_fields(5, 3, 3, 8, 6)
    for off in (0, 4):
        s_z, s_w = nr.noise_fields(5, 3, 3, 8, 6, batch_offset=off, batch=4)
        np.testing.assert_array_equal(s_z, n_z[:, off:off + 4])
        np.testing.assert_array_equal(s_w, n_w[:, off:off + 4])
    assert (n_z != n_w).all()
    assert (nr.noise_fields(5, 4, 3, 8, 6)[0] != n_z).all()           # another minibatch counter: another field


# ------------------------------------------------------------------ 2. the wrapper
def _plain_conversation(meta, train):
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    x, target, desc, _ = common.case_inputs(meta, 0)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=train, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], models["baseline_sen"], models["baseline_rec"], args, fl)
    st = lambda v: torch.stack(v).numpy()
    return dict(ps=st(s[2]).reshape(len(y), -1), z=st(sen_w[0]), w=st(rec_w[0]), y=st(y))


def test_wrapper_adds_sigma_n_to_the_messages():
    meta = nr.meta_of("G256")
    T, B, W = nr.dims(meta)
    n_z, n_w = nr.noise_fields(21, 1, T, B, W)
    clean = _plain_conversation(meta, train=False)
    zero = nr.conversation(meta, n_z, n_w, train=False, sigma_sen=0.0, sigma_rec=0.0)
    for k in clean:
        np.testing.assert_array_equal(zero[k], clean[k], err_msg=k)
    noisy = nr.conversation(meta, n_z, n_w, train=False)
    np.testing.assert_allclose(noisy["z"][0], clean["z"][0] + nr.SIGMA_SEN * n_z[0], atol=1e-6, rtol=0)
    # the receiver's first message is formed from the noisy z_0: its own logits moved, and its noise sits on top of them
    assert np.abs(noisy["w"][0] - nr.SIGMA_REC * n_w[0] - clean["w"][0]).max() > 1e-3
    for t in range(1, T):
        assert np.abs(noisy["z"][t] - nr.SIGMA_SEN * n_z[t] - clean["z"][t]).max() > 1e-3, t
    only_rec = nr.conversation(meta, n_z, n_w, train=False, sigma_sen=0.0)
    np.testing.assert_array_equal(only_rec["z"][0], clean["z"][0])
    np.testing.assert_allclose(only_rec["w"][0], clean["w"][0] + nr.SIGMA_REC * n_w[0], atol=1e-6, rtol=0)
    masked = nr.conversation(meta, n_z, n_w, train=False, mask=(np.arange(W) % 3 == 0))
    np.testing.assert_allclose(masked["z"][0], np.abs(clean["z"][0] + nr.SIGMA_SEN * n_z[0] - (np.arange(W) % 3 == 0)), atol=1e-6, rtol=0)


# ------------------------------------------------------------------ 3. reach conditions of the GPU cases
_ADAPTIVE = {}


def adaptive_minibatch(case):
    """(separated uniforms, packed oracle minibatch) of an Adaptive case under the training noise of seed 0, counter 1."""
    if case not in _ADAPTIVE:
        meta = nr.meta_of(case)
        n_z, n_w = nr.noise_fields(0, 1, *nr.dims(meta))
        us = nr.separated_uniforms(meta, n_z, n_w)
        _ADAPTIVE[case] = (us, nr.train_minibatch(meta, n_z, n_w, us)[0])
    return _ADAPTIVE[case]


@pytest.mark.parametrize("case", nr.ADAPTIVE)
def test_adaptive_cases_stop_early_and_late_and_their_draws_are_separated(case):
    meta = nr.meta_of(case)
    us, packed = adaptive_minibatch(case)
    tstar, n = nr.stop_steps(packed)
    assert n == meta["max_exchange"] == 4
    assert (tstar == 0).any() and (tstar == n - 1).any() and len(set(tstar.tolist())) >= 3, tstar
    p = np.asarray(packed["mb0.s_probs"], np.float64)
    assert np.abs(np.asarray(us[1])[:n].reshape(p.shape) - p).min() >= 1e-4 - 1e-7
    assert not np.asarray(packed["mb0.sen_probs"]).size               # continuous mode: the stop bits are the only draws


@pytest.mark.parametrize("case", sorted(nr.CASES))
def test_shapes_and_evaluation_margins(case):
    meta = nr.meta_of(case)
    T, B, W = nr.dims(meta)
    assert not meta["use_binary"]
    from tests import generic_inst as gi
    threads = gi.conv_threads(**gi.dims_of(meta))
    assert threads == (512 if case == "G512" else 256)
    if case == "G256":                                                # every strided loop has a tail, rows are not 16-byte aligned
        assert (meta["img_h_dim"], W, meta["rec_hidden"], meta["n_classes"], B, T) == (100, 50, 128, 7, 5, 3) and W % 4
    if case in ("M", "MA"):
        assert meta["n_classes"] == 100 and B == 32 and T == 4 and meta["fixed_exchange"] == (case == "M")      # two sample tiles of mc3
    if case == "A":
        assert meta["n_classes"] == 30 and B == 16 and T == 4 and not meta["fixed_exchange"]
    for c1 in range(3):                                               # the three evaluation conversations the GPU tests run
        n_z, n_w = nr.noise_fields(nr.EVAL_SEED, c1, T, B, W, nr.EVAL_STREAMS)
        conv = nr.conversation(meta, n_z, n_w, train=False)
        prod = np.cumprod(conv["ps"], 0) if meta["s_prob_prod"] else conv["ps"]
        assert np.abs(prod - 0.5).min() > 1e-4, (case, c1)


# ------------------------------------------------------------------ 4. Game's arguments
def _modules(fl):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    return sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0), Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden)


def test_game_arguments():
    from multimodalgame_amd.game import Game
    cont = cpu_ref.Flags(**dict(TINY, use_binary=False))
    ok = dict(flags=cont, device="cpu")
    params = inspect.signature(Game.__init__).parameters
    assert params["noise_sen"].default is None and params["noise_rec"].default is None and params["noise_dev"].default is False
    game = Game(*_modules(cont), noise_sen=0.3, noise_rec=0.2, noise_dev=True, **ok)
    assert game.noise == (0.3, 0.2, True)
    for kw in (dict(autograd=True), dict(autograd=True, channel_grad=True), dict(autograd=True, channel_grad=True, input_grad=True)):
        assert Game(*_modules(cont), noise_sen=0.3, **dict(ok, **kw)).noise == (0.3, 0.0, False)
    assert Game(*_modules(cont), **ok).noise is None
    assert Game(*_modules(cont), noise_sen=0.0, noise_rec=None, **ok).noise is None
    game.set_noise(0.1, None)
    assert game.noise == (0.1, 0.0, True)
    game.set_noise(None, None)
    assert game.noise is None
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="standard deviation"):
            Game(*_modules(cont), noise_sen=bad, **ok)
        with pytest.raises(ValueError, match="standard deviation"):
            Game(*_modules(cont), noise_rec=bad, **ok)
        with pytest.raises(ValueError, match="standard deviation"):
            game.set_noise(0.1, bad)
    binary = cpu_ref.Flags(**dict(TINY, use_binary=True))
    with pytest.raises(ValueError, match="continuous"):
        Game(*_modules(binary), flags=binary, device="cpu", noise_sen=0.3)
    assert Game(*_modules(binary), flags=binary, device="cpu", noise_sen=None, noise_rec=0.0).noise is None
    for kw in (dict(sender_mix="prod"), dict(ignore_code=True)):
        with pytest.raises(NotImplementedError, match="sender variant"):
            Game(*_modules(cont), noise_rec=0.2, **dict(ok, **kw))


def test_game_refuses_noise_with_attention():
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = cpu_ref.Flags(**dict(TINY, use_binary=False))
    _, _, bs, br = _modules(fl)
    attn_rec = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary, desc_attn=True, desc_attn_dim=8)
    with pytest.raises(NotImplementedError, match="description attention"):
        Game(_modules(fl)[0], attn_rec, bs, br, flags=fl, device="cpu", noise_sen=0.3)
    attn_sen = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary, use_attn=True, attn_dim=8)
    with pytest.raises(NotImplementedError, match="visual attention"):
        Game(attn_sen, _modules(fl)[1], bs, br, flags=fl, device="cpu", noise_rec=0.3)


# ------------------------------------------------------------------ 5. the selection
def test_plan_for_with_the_noise_bit(switches):
    from multimodalgame_amd import _lib
    assert _lib.PLAN_NOISE & (15 << _lib.PLAN_FROZEN_SHIFT | _lib.PLAN_NO_ROLES | _lib.PLAN_FLIPS | _lib.PLAN_VARIANT | _lib.PLAN_RELAX) == 0
    e = entry("c1")
    cont = dict(SHAPES["c1"], use_binary=False, fixed_exchange=True, entropy_s=None, entropy_sen=None, entropy_rec=None)
    clean = _lib.plan_for(_lib.make_config(**cont), e["caps"], 0).splitlines()
    noisy = _lib.plan_for(_lib.make_config(**cont), e["caps"], _lib.PLAN_NOISE).splitlines()
    assert clean[0].startswith("mmg_create: family 0 ")               # the register-resident conversation without the bit
    assert noisy[0].startswith("mmg_create: family 3 ") and " game_ok 0 " in noisy[0]
    assert " tile_ok 0 " in noisy[1] and " mc 0 " in noisy[1] and " rc 0 " in noisy[1] and " rc_persist 0 " in noisy[1]
    assert " mc3 0 mc3p 0 wins 0 " in noisy[3]
    assert len(noisy) == len(clean) + 1 and "k_conversation_noise serves the conversation" in noisy[-2]
    assert _lib.plan_caps("\n".join(noisy)) == e["caps"]              # the caps stay the last line
    # the many-class continuous shapes keep k_conversation_mc3 and lose the pair kernel
    for shape in ("mc_continuous", "c5", "c5_b2048"):
        m = entry(shape)
        assert not SHAPES[shape]["use_binary"]
        base = plan(m).splitlines()
        assert base == m["plan"] + [caps_line(m["caps"])]             # without the bit: the recorded text
        assert base[0].startswith("mmg_create: family 1 ") and " mc3 1 " in base[3]
        got = plan(m, flags=_lib.PLAN_NOISE).splitlines()
        if " mc3p 1 " in base[3] and shape == "c5_b2048":
            assert " wins 1 " in base[3]                              # the pair kernel would have served this batch
        assert got[0].startswith("mmg_create: family 1 ") and " mc3 1 mc3p 0 wins 0 " in got[3], got
        assert "k_conversation_mc3_noise serves the conversation" in got[-2]
    # a device without room for mc3: the generic family, never k_conversation_mc
    m = entry("mc_continuous")
    caps = list(m["caps"]); caps[_lib.PLAN_CAPS.index("mc3")] = 0
    got = plan(m, caps=caps, flags=_lib.PLAN_NOISE).splitlines()
    assert got[0].startswith("mmg_create: family 3 ") and " mc 0 " in got[1]
    # binary messages: the bit is carried and nothing happens (the setter refuses such a handle)
    assert plan(e, flags=_lib.PLAN_NOISE) == plan(e)
    # every recorded entry: the bit clear gives the recorded text (tests/test_plan_cpu.py), with a frozen agent too
    assert plan(e, flags=_lib.agent_mask(["receiver"]) << _lib.PLAN_FROZEN_SHIFT) != plan(e)
    with pytest.raises(_lib.MmgError, match="sender variant"):
        _lib.plan_for(_lib.make_config(**cont), e["caps"], _lib.PLAN_NOISE | _lib.PLAN_VARIANT)
    assert _lib.plan_for(_lib.make_config(**cont), e["caps"], _lib.PLAN_NOISE | _lib.PLAN_NO_ROLES).startswith(
        "mmg_create: family 3 (0 fast, 1 mc, 2 tile, 3 generic) no_roles 1 ")


def test_the_symbol_is_declared_and_exported():
    from multimodalgame_amd import _lib
    assert "mmg_set_message_noise" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "mmg_set_message_noise")
