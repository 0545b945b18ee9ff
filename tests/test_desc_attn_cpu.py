"""Description attention without a GPU: the wrapped oracle (tests/desc_attn_ref.py) against the g12 fixtures the reference's own code
produced, the layout twins of the ABI, the refusals with their messages, and the conditions the GPU comparisons rely on (so that
none of them can pass vacuously)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, agents, flags as F, game as G, misc
from multimodalgame_amd.engine import check_desc_set
from oracle import PORTABLE_FP_ENV
from tests import common, desc_attn_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(ref.MODES)
C1 = (64, 30, 512, 256, 32, 64, 100, 500, 10)


# ------------------------------------------------------------------ the wrapped oracle against the reference's own numbers
@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """The three modes' training minibatch and evaluation conversation from the wrapped oracle, in one child process under
    oracle.PORTABLE_FP_ENV (the environment the fixtures were generated in; it has to be in place before torch loads)."""
    out = str(tmp_path_factory.mktemp("desc_attn") / "oracle.npz")
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, torch; torch.set_num_threads(1); "
            "from tests import common, desc_attn_ref as ref; d = {}\n"
            "for mode in ref.MODES:\n"
            "    z, meta = ref.load_golden('g12_desc_attn_' + mode)\n"
            "    u = common.case_inputs(meta, 0)[3]\n"
            "    packed = ref.train_minibatch(meta, u, y2_bias=z['mb0.p.receiver.y2.bias.sample'])[0]\n"
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
    """tests/test_oracle_golden.py's tolerances for g2 / g3."""
    got = {k[len(mode) + 1:]: v for k, v in oracle_runs.items() if k.startswith(mode + "/")}
    for fixture in ("g12_desc_attn_" + mode, "g12_desc_attn_%s_eval" % mode):
        z, meta = ref.load_golden(fixture)
        assert meta["desc_attn_dim"] == 64 and meta["desc_set_lens"] == ref.LENS_A
        problems = common.compare_packed(got, z, atol=2e-6, rtol=2e-5, ulps=1)
        assert not problems, "\n".join(problems[:20])
        assert len(z) > 10


def test_fixtures_record_what_they_claim():
    limit = max(os.path.getsize(os.path.join(common.GOLDEN_DIR, f)) for f in os.listdir(common.GOLDEN_DIR) if f.startswith("g11_"))
    for mode in MODES:
        z, meta = ref.load_golden("g12_desc_attn_" + mode)
        e, _ = ref.load_golden("g12_desc_attn_%s_eval" % mode)
        for f in ("g12_desc_attn_" + mode, "g12_desc_attn_%s_eval" % mode):
            assert os.path.getsize(os.path.join(common.GOLDEN_DIR, f + ".npz")) <= limit, f
        assert int(z["mb0.n_steps"]) == 4 and int(e["eval.n_steps"]) > 1
        for name in ref.ATTN_NAMES:                                      # the reference trained the six tensors
            assert "mb0.g.receiver.%s.norm" % name in z and "mb0.p.receiver.%s.sample" % name in z
        for name in ("d_d.weight", "d_h.weight", "d_attn.weight"):
            assert float(z["mb0.g.receiver.%s.norm" % name]) > 1e-6, (mode, name)
        # a shift inside every softmax segment: what the reference's autograd leaves there is rounding noise
        assert float(z["mb0.g.receiver.d_attn.bias.norm"]) < 1e-7
        assert meta["use_binary"] == ref.MODES[mode]["use_binary"] and meta["fixed_exchange"] == ref.MODES[mode]["fixed_exchange"]


# ------------------------------------------------------------------ the ABI: twins, the six tensors, the supported range
def _cfg(*dims, **kw):
    return _lib.make_config(*dims, **kw)


def test_twins_with_attn_dim_zero_equal_the_plain_queries():
    lib = _lib.load()
    for dims, kw in ((C1, dict(fixed_exchange=False)), ((5, 7, 18, 40, 12, 20, 12, 70, 3), dict(optim_type="Adam")),
                     ((64, 30, 512, 1024, 256, 64, 100, 500, 10), dict(use_binary=False))):
        cfg = _cfg(*dims, **kw)
        for n_words in (0, 300):                                         # (ignored without attention)
            assert lib.mmg_attn_param_count(C.byref(cfg), 0, n_words) == lib.mmg_param_count(C.byref(cfg))
            assert lib.mmg_attn_grad_floats(C.byref(cfg), 0, n_words) == lib.mmg_grad_floats(C.byref(cfg))
            assert lib.mmg_attn_workspace_bytes(C.byref(cfg), 0, n_words) == lib.mmg_workspace_bytes(C.byref(cfg))
            assert _lib.param_table(cfg, 0, n_words) == _lib.param_table(cfg)
            assert _lib.tape_table(cfg, 0, n_words) == _lib.tape_table(cfg)
    assert lib.mmg_version() == 3
    for sym in ("mmg_attn_param_count", "mmg_attn_param_table", "mmg_attn_grad_floats", "mmg_attn_workspace_bytes",
                "mmg_attn_tape_table", "mmg_attn_create", "mmg_set_desc_set"):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym)


def test_the_six_tensors_lie_inside_the_receivers_range():
    cfg = _cfg(*C1, fixed_exchange=False)
    plain, tab = _lib.param_table(cfg), _lib.param_table(cfg, 64, 300)
    assert sum(e["rows"] * max(e["cols"], 1) for e in tab) == 384180 + 64 * 100 + 64 + 64 * 64 + 64 + 64 + 1
    rec = [e for e in tab if e["agent"] == "receiver"]
    assert [e["name"] for e in rec[:15]] == [e["name"] for e in plain if e["agent"] == "receiver"]
    assert [(e["name"], e["rows"], e["cols"]) for e in rec[15:]] == [
        ("d_d.weight", 64, 100), ("d_d.bias", 64, 0), ("d_h.weight", 64, 64), ("d_h.bias", 64, 0), ("d_attn.weight", 1, 64), ("d_attn.bias", 1, 0)]
    # one contiguous range per agent, the receiver's first: its clip norm and optimizer cover the six with no special case
    end, order = 0, []
    for e in tab:
        assert e["offset"] == end and e["offset"] % 4 == 0, e
        end = e["offset"] + (e["rows"] * max(e["cols"], 1) + 3) // 4 * 4
        if not order or order[-1] != e["agent"]:
            order.append(e["agent"])
    assert order == ["receiver", "sender", "baseline_rec", "baseline_sen"]
    assert _lib.load().mmg_attn_param_count(C.byref(cfg), 64, 300) == end
    # the plain tensors keep their order and shapes; the other agents' move up by the six tensors' padded size
    shift = sum((e["rows"] * max(e["cols"], 1) + 3) // 4 * 4 for e in rec[15:])
    for a, b in zip(plain, [e for e in tab if e["name"] not in ref.ATTN_NAMES]):
        assert (a["name"], a["agent"], a["rows"], a["cols"]) == (b["name"], b["agent"], b["rows"], b["cols"])
        assert b["offset"] == a["offset"] + (0 if a["agent"] == "receiver" else shift)
    # the tape: the plain arrays at their offsets, the attention arrays behind them
    tp, ta = _lib.tape_table(cfg), _lib.tape_table(cfg, 64, 300)
    assert ta[:len(tp)] == tp
    extra = {e["name"]: e["dims"] for e in ta[len(tp):]}
    assert extra["alpha"] == [10, 64, 300] and extra["attn_set"] == [300, 100] and extra["attn_DD"] == [300, 64] and extra["attn_E"] == [300, 64]
    assert not set(extra) & {e["name"] for e in tp}
    # nothing of size B * D * V or B * NW * V
    assert max(int(np.prod(d)) for d in extra.values()) == 10 * 64 * 300


@pytest.mark.parametrize("attn_dim, n_words, dims, word", [
    (129, 300, C1, "attn_dim"), (-1, 300, C1, "attn_dim"), (64, 2049, C1, "n_words"), (64, 29, C1, "n_words"),
    (64, 300, (513,) + C1[1:], "batch"), (64, 300, (64, 129) + C1[2:], "n_classes")])
def test_outside_the_supported_range_is_an_error_with_a_message(attn_dim, n_words, dims, word):
    lib = _lib.load()
    cfg = _cfg(*dims)
    for fn in (lib.mmg_attn_param_count, lib.mmg_attn_grad_floats, lib.mmg_attn_workspace_bytes):
        assert fn(C.byref(cfg), attn_dim, n_words) < 0
        msg = lib.mmg_last_error().decode()
        assert "desc_attn" in msg and word in msg, msg
    assert lib.mmg_attn_param_table(C.byref(cfg), attn_dim, n_words, None, 0) < 0
    assert lib.mmg_attn_tape_table(C.byref(cfg), attn_dim, n_words, None, 0) < 0
    assert not lib.mmg_attn_create(C.byref(cfg), attn_dim, n_words, None, 0, None, None, None)


def test_the_edges_of_the_supported_range_are_accepted():
    lib = _lib.load()
    for attn_dim, n_words, dims in ((1, 30, C1), (128, 2048, (512, 128) + C1[2:])):
        assert lib.mmg_attn_param_count(C.byref(_cfg(*dims)), attn_dim, n_words) > 0, lib.mmg_last_error()
    cfg = _cfg(16, 30, 512, 256, 32, 64, 100, 500, 4, global_batch=32)
    assert lib.mmg_attn_param_count(C.byref(cfg), 64, 300) < 0 and b"one GPU" in lib.mmg_last_error()


# ------------------------------------------------------------------ Python: the module, the refusals, the lens
def _agents(desc_attn=True, attn_dim=64, use_binary=True):
    s = agents.Sender("avgpool_512", 512, 256, 32, 32, use_binary)
    r = agents.Receiver(32, 100, 64, 1, 32, 1, use_binary, desc_attn=desc_attn, desc_attn_dim=attn_dim)
    return s, r, agents.Baseline(500, 256, 32, 0), agents.Baseline(500, 0, 32, 64)


class _Flags(object):
    desc_attn, sender_mix, flipout_sen, flipout_rec = False, "sum", None, None
    ignore_receiver = ignore_code = visual_attn = bit_flip = False
    max_exchange, fixed_exchange, s_prob_prod = 4, False, True
    entropy_s = entropy_sen = entropy_rec = None
    first_rec, optim_type, learning_rate, top_k_train = 0.0, "RMSprop", 1e-4, 6


def test_receiver_module_owns_the_six_tensors_under_the_reference_names():
    torch.manual_seed(3)
    r = _agents()[1]
    names = [n for n, _ in r.named_parameters()]
    assert names[-6:] == list(ref.ATTN_NAMES) and len(names) == 21       # model.py:267-271: behind the other layers
    assert tuple(r.d_d.weight.shape) == (64, 100) and tuple(r.d_h.weight.shape) == (64, 64) and tuple(r.d_attn.weight.shape) == (1, 64)
    for lin in (r.d_d, r.d_h, r.d_attn):                                  # model.py:275-280: Xavier-normal weights, zero biases
        assert not lin.bias.any()
        std = float(lin.weight.detach().std())
        want = (2.0 / sum(lin.weight.shape)) ** 0.5
        assert 0.6 * want < std < 1.5 * want
    plain = _agents(desc_attn=False)[1]
    assert len(list(plain.named_parameters())) == 15 and plain.attn_dim == 0
    with pytest.raises(NotImplementedError, match="desc_attn_dim"):
        _agents(attn_dim=129)


@pytest.mark.parametrize("kw, word", [(dict(autograd=True), "autograd"), (dict(autograd=True, channel_grad=True), "autograd"),
                                      (dict(input_grad=True), "input_grad"), (dict(channel_grad=True), "channel_grad"),
                                      (dict(flipout_sen=0.1), "flips"), (dict(flipout_rec=0.1), "flips"),
                                      (dict(sender_mix="prod"), "sender variant"), (dict(ignore_receiver=True), "sender variant")])
def test_game_refuses_what_attention_does_not_combine_with(kw, word):
    with pytest.raises(NotImplementedError, match="desc_attn") as e:
        G.Game(*_agents(), flags=_Flags(), device="cpu", **kw)
    assert word in str(e.value)
    G.Game(*_agents(desc_attn=False), flags=_Flags(), device="cpu", **kw)       # (the plain game takes every one of them)


def test_game_refuses_world_and_the_switch_and_a_plain_receiver_refuses_a_set():
    g = G.Game(*_agents(), flags=_Flags(), device="cpu")
    assert g.attn_dim == 64
    with pytest.raises(NotImplementedError, match="desc_attn.*world > 1"):
        g.set_parallel(0, 2)
    fl = _Flags()
    fl.desc_attn = True
    with pytest.raises(NotImplementedError, match="-desc_attn"):
        G.Game(*_agents(), flags=fl, device="cpu")
    entry = [u for u in F.UNSUPPORTED if u[0] == "desc_attn"][0]
    assert "desc_attn=True" in entry[2] and "model.py:344" in entry[2]
    plain = G.Game(*_agents(desc_attn=False), flags=_Flags(), device="cpu")
    with pytest.raises(NotImplementedError, match="desc_attn=True"):
        plain.set_desc_set(torch.zeros(3, 100), [1, 2])
    with pytest.raises(ValueError, match="desc_set"):                         # no set yet: a message, not the plain receiver
        g.engine_for(16, 30)


@pytest.mark.parametrize("lens, word", [([1, 0, 2], "at least one word"), ([1, 1, 2], "sum to 4"), ([3], "1 entries for 3 classes"),
                                        ([1, -1, 3], "at least one word")])
def test_bad_lens_are_rejected(lens, word):
    with pytest.raises(ValueError, match=word):
        check_desc_set(torch.zeros(3, 100), lens, 3, 100)
    g = G.Game(*_agents(), flags=_Flags(), device="cpu")
    with pytest.raises(ValueError):
        g.set_desc_set(torch.zeros(3, 100), lens if len(lens) == 3 else [1, 1, 2])
    with pytest.raises(ValueError, match=r"\[n_words, 100\]"):
        g.set_desc_set(torch.zeros(3, 99), [1, 1, 1])
    with pytest.raises(ValueError, match="desc_set and desc_set_lens"):
        g.set_desc_set(None, None)
    with pytest.raises(NotImplementedError, match="2048 words"):
        g.set_desc_set(torch.zeros(2049, 100), [2049])
    g.set_desc_set(torch.zeros(3, 100), [1, 1, 1])


def test_desc_set_of_restates_the_references_concatenation():
    """model.py:1081-1084 over misc.cbow's output: the 'set' rows in key order, the token counts (missing words included)."""
    word_dict = {w: {"emb": None if w == "zzz" else torch.full((4,), float(i + 1))} for i, w in enumerate(("a", "b", "c", "zzz"))}
    descr = {7: {"desc": ["a", "zzz", "b"]}, 3: {"desc": ["c"]}, 9: {"desc": ["b", "b"]}}
    descr = misc.cbow(descr, word_dict)
    dset, lens = misc.desc_set_of(descr)
    assert lens == [3, 1, 2] and tuple(dset.shape) == (6, 4)
    want = torch.cat([descr[i]["set"].view(-1, 4) for i in descr.keys()], 0)                          # model.py:1081-1082
    assert torch.equal(dset, want) and not dset[1].any() and float(dset[3, 0]) == 3.0
    check_desc_set(dset, lens, 3, 4)


# ------------------------------------------------------------------ what the GPU comparisons rely on, with their seeds
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_reach_of_the_training_cases(shape, mode):
    """Adaptive: at least one sample stops before the last step and one runs to it, and one has t* >= 1, so the query path carries
    gradient.  Every mode: no relu pre-activation of the output step lies within 1e-5 of 0; every segment's alpha sums to 1, a
    one-word class has alpha == 1, the all-zero word row is still attended over."""
    m = ref.train_meta(shape, mode)
    T, lens = m["max_exchange"], m["desc_set_lens"]
    tp = ref.conversation(m, train=True, uniforms=ref.separated_uniforms(m))
    stopped = tp["mask"][1:T + 1, :, 0] == 0
    tstar = np.where(stopped.any(0), stopped.argmax(0), T - 1) if mode == "adaptive" else np.full(m["batch"], T - 1)
    if mode == "adaptive":
        assert (tstar < T - 1).any() and (tstar == T - 1).any() and (tstar >= 1).any(), tstar
    pre = np.stack([tp["pre"][tstar[b], b] for b in range(m["batch"])])
    assert np.abs(pre).min() > 1e-5
    seg = np.concatenate([[0], np.cumsum(lens)])
    for d, n in enumerate(lens):
        np.testing.assert_allclose(tp["alpha"][:, :, seg[d]:seg[d + 1]].sum(-1), 1.0, atol=1e-6)
        if n == 1:
            assert (tp["alpha"][:, :, seg[d]] == 1.0).all()
    assert 1 in lens and (shape != "A" or (max(lens) > 64 and sum(lens) > 256))
    dset, _ = ref.desc_set(m)
    assert not dset[ref.ZERO_ROW[shape]].any() and (tp["alpha"][:, :, ref.ZERO_ROW[shape]] > 0).all()


@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_separated_uniforms_keep_the_trajectory_and_the_margin(shape):
    m = ref.train_meta(shape, "adaptive")
    u0 = common.case_inputs(m, 0)[3]
    u = ref.separated_uniforms(m, margin=1e-4)
    a, b = ref.conversation(m, True, u0), ref.conversation(m, True, u)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for key, uu in zip(("pz", "ps", "pw"), u):
        assert np.abs(uu.reshape(b[key].shape) - b[key]).min() >= 1e-4 - 1e-7, key


@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_evaluation_seeds_leave_no_bit_out(shape):
    """The evaluation comparisons on the GPU leave out no bit: with these seeds the oracle has no probability within 1e-4 of 0.5,
    for the seeded weights and for the second set the stale-tables test loads."""
    for seed, data in ((None, ref.EVAL_DATA_SEED[shape]), (ref.SECOND_WEIGHTS, ref.SECOND_EVAL_DATA_SEED[shape])):
        tp = ref.conversation(ref.meta(shape, seed_data=data), train=False, seed=seed)
        prod = np.cumprod(tp["ps"], 0)                                   # model.py:423-427: the stop bit rounds the running product
        for p in (tp["pz"], tp["pw"], prod):
            assert np.abs(p - 0.5).min() > 1e-4, (shape, seed)


def test_swapping_the_two_blocks_of_y1_changes_the_logits():
    """The column-order test on the GPU compares against BOTH orders: they have to differ by far more than the tolerance."""
    m = ref.meta("A", seed_data=ref.EVAL_DATA_SEED["A"])
    a, b = ref.conversation(m, train=False), ref.conversation(m, train=False, swap_y1=True)
    assert np.abs(a["y"][0] - b["y"][0]).max() > 1e-2
