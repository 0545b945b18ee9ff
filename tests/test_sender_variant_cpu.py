"""The sender's communication ablations without a GPU: the wrapped oracle (tests/sender_variant_ref.py) against the g11 fixtures the
reference's own code produced, the conditions the GPU comparisons rely on (so that none of them can pass vacuously), the kernel
selection of a variant handle through mmg_plan_for, and the validation of Game(..., sender_mix=, ignore_code=, ignore_receiver=)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, flags as F
from oracle import PORTABLE_FP_ENV
from tests import common, sender_variant_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = sorted(ref.SETTINGS)


# ------------------------------------------------------------------ the wrapped oracle against the reference's own numbers
@pytest.fixture(scope="module")
def oracle_runs(tmp_path_factory):
    """The four settings' training minibatch and evaluation conversation from the wrapped oracle, in one child process under
    oracle.PORTABLE_FP_ENV (the environment the fixtures were generated in; it has to be in place before torch loads)."""
    out = str(tmp_path_factory.mktemp("sender_variant") / "oracle.npz")
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, torch; torch.set_num_threads(1); "
            "from tests import common, sender_variant_ref as ref; d = {}\n"
            "for name, setting in ref.SETTINGS.items():\n"
            "    z, meta = common.load_golden('g11_sender_variant_' + name)\n"
            "    u = common.case_inputs(meta, 0)[3]\n"
            "    packed = ref.train_minibatch(meta, setting, u, y2_bias=z['mb0.p.receiver.y2.bias.sample'])[0]\n"
            "    packed.update(ref.eval_case(meta, setting))\n"
            "    d.update({name + '/' + k: v for k, v in packed.items()})\n"
            "np.savez(%r, **d)" % (REPO, out))
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + ["-c", code], env=dict(os.environ, **PORTABLE_FP_ENV), cwd=REPO,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", SETTINGS)
def test_wrapped_oracle_matches_the_reference(name, oracle_runs):
    """tests/test_oracle_golden.py's tolerances for g2 / g3."""
    got = {k[len(name) + 1:]: v for k, v in oracle_runs.items() if k.startswith(name + "/")}
    for fixture in ("g11_sender_variant_" + name, "g11_sender_variant_%s_eval" % name):
        z, meta = common.load_golden(fixture)
        assert (meta["sender_mix"], meta["ignore_code"], meta["ignore_receiver"]) == ref.SETTINGS[name]
        problems = common.compare_packed(got, z, atol=2e-6, rtol=2e-5, ulps=1)
        assert not problems, "\n".join(problems[:20])
        assert len(z.files) > 10


def test_fixtures_record_what_they_claim():
    limit = max(os.path.getsize(os.path.join(common.GOLDEN_DIR, "g3_tiny_%s.npz" % k)) for k in ("sgd", "adam"))
    for name, setting in ref.SETTINGS.items():
        z, meta = common.load_golden("g11_sender_variant_" + name)
        e, _ = common.load_golden("g11_sender_variant_%s_eval" % name)
        for f in ("g11_sender_variant_" + name, "g11_sender_variant_%s_eval" % name):
            assert os.path.getsize(os.path.join(common.GOLDEN_DIR, f + ".npz")) <= limit, f
        assert int(z["mb0.n_steps"]) > 1 and int(e["eval.n_steps"]) > 1
        grads = [k for k in z.files if ".g.sender." in k]
        assert any("image_layer.weight" in k for k in grads)
        # the reference leaves .grad of the three tensors None under -ignore_code: pack_train then has no entry for them
        has_code = any("code_layer" in k or "code_bias" in k for k in grads)
        assert has_code == (not setting[1]), name
        if setting[2]:                                                  # the returned message is zeros although the logits say otherwise
            assert not z["mb0.rec_feats"].any() and not e["eval.rec_feats"].any()
            assert (z["mb0.rec_probs"] > 0.5).any() and (e["eval.rec_probs"] > 0.5).any()
        else:
            assert z["mb0.rec_feats"].any() and e["eval.rec_feats"].any()


# ------------------------------------------------------------------ what the GPU comparisons rely on, with their seeds
@pytest.mark.parametrize("shape", sorted(ref.SHAPES))
def test_every_setting_changes_the_sender_and_ignore_receiver_hides_set_bits(shape):
    meta = ref.meta(shape)
    u = common.case_inputs(meta, 0)[3]
    plain = ref.conversation(meta, ref.SUM, train=True, uniforms=u)
    for name, setting in ref.SETTINGS.items():
        got = ref.conversation(meta, setting, train=True, uniforms=ref.separated_uniforms(meta, setting))
        assert np.abs(got["pz"] - plain["pz"]).max() > 1e-3, (shape, name)
        if setting[2]:
            assert (got["pw"] > 0.5).any() and not got["w"].any(), (shape, name)
            if setting[0] == "sum":
                np.testing.assert_array_equal(got["pz"][0], plain["pz"][0])     # step 0 has seen no message yet
        else:
            assert got["w"].any(), (shape, name)
    a = ref.conversation(meta, ("prod", True, False), train=True, uniforms=u)
    b = ref.conversation(meta, ("sum", True, False), train=True, uniforms=u)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)              # prod + ignore_code == sum + ignore_code


def test_separated_uniforms_keep_the_trajectory_and_the_margin():
    meta = ref.meta("A")
    for name, setting in ref.SETTINGS.items():
        u0 = common.case_inputs(meta, 0)[3]
        u = ref.separated_uniforms(meta, setting, margin=1e-4)
        a, b = ref.conversation(meta, setting, True, u0), ref.conversation(meta, setting, True, u)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (name, k))
        for key, uu in zip(("pz", "ps", "pw"), u):
            assert np.abs(uu.reshape(b[key].shape) - b[key]).min() >= 1e-4 - 1e-7, (name, key)


@pytest.mark.parametrize("name", SETTINGS)
def test_evaluation_seeds_leave_no_bit_out(name):
    """The evaluation comparison on the GPU leaves out bits with |p - 0.5| <= 1e-4; with these data seeds the oracle has none."""
    meta = ref.meta("A", seed_data=ref.EVAL_DATA_SEED[name])
    tp = ref.conversation(meta, ref.SETTINGS[name], train=False)
    prod = np.cumprod(tp["ps"], 0)                                       # model.py:423-427: the stop bit rounds the running product
    for p in (tp["pz"], tp["pw"], prod):
        assert np.abs(p - 0.5).min() > 1e-4
    if ref.SETTINGS[name][2]:
        assert (tp["pw"] > 0.5).any() and not tp["w"].any()


def test_ignore_code_leaves_the_three_gradients_none():
    meta = ref.meta("A")
    u = common.case_inputs(meta, 0)[3]
    for mix in ("sum", "prod"):
        _, res, models = ref.train_minibatch(meta, (mix, True, False), u, update=False)
        s = models["sender"]
        assert s.code_layer.weight.grad is None and s.code_layer.bias.grad is None and s.code_bias.grad is None
        assert s.image_layer.weight.grad is not None and float(s.image_layer.weight.grad.abs().max()) > 0
        assert set(res["grads"]["sender"]) == {"image_layer.weight", "image_layer.bias", "binary_layer.weight", "binary_layer.bias"}
    _, _, models = ref.train_minibatch(meta, ("prod", False, False), u, update=False)
    assert float(models["sender"].code_bias.grad.abs().max()) > 0


# ------------------------------------------------------------------ selection
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "plans_mi355x.json")))
SWITCHES = ("MMG_NO_FAST", "MMG_NO_MERGE", "MMG_NO_MERGE_PREP", "MMG_NO_PERSIST_LL", "MMG_NO_RSAMPLE", "MMG_NO_RMSG", "MMG_NO_FUSED_S",
            "MMG_NO_MC", "MMG_NO_RC", "MMG_NO_TILE", "MMG_TILE", "MMG_NO_SPLIT", "MMG_NO_PERSIST", "MMG_NO_RC_BWD", "MMG_NO_RC_PERSIST",
            "MMG_NO_MC3P", "MMG_NO_GAME", "MMG_NO_WGRAD_OPT", "MMG_NO_ROLES", "HSA_CU_MASK", "ROC_GLOBAL_CU_MASK")


def _entry(shape):
    return [e for e in GOLDEN["entries"] if e["shape"] == shape and e["setting"] == "default"][0]


def _plan(e, flags):
    return _lib.plan_for(_lib.make_config(cu_budget=e["cu_budget"], **GOLDEN["shapes"][e["shape"]]), e["caps"], flags)


def _field(text, line, name):
    words = text.splitlines()[line].split()
    return int(words[words.index(name) + 1])


@pytest.mark.parametrize("shape", ["c2", "c4"])
def test_plan_of_a_variant_handle_is_the_generic_family(shape, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    e = _entry(shape)
    plain = _plan(e, 0)
    assert plain.splitlines()[:5] == e["plan"]                           # without the bit: the golden text, unchanged
    assert _field(plain, 0, "family") != 3
    text = _plan(e, _lib.PLAN_VARIANT)
    assert _field(text, 0, "family") == 3 and _field(text, 0, "game_ok") == 0
    for name in ("tile_ok", "tile_persist", "split", "mc", "fast", "rc", "rc_persist", "rc_bwd"):
        assert _field(text, 1, name) == 0, name
    assert _field(text, 3, "merge_prep") == 0 and _field(text, 3, "fwd_basehx") == 0
    assert "class roles 0 " in text.splitlines()[4]
    with pytest.raises(_lib.MmgError, match="flips"):
        _plan(e, _lib.PLAN_VARIANT | _lib.PLAN_FLIPS)


# ------------------------------------------------------------------ the interface
def test_lib_declares_the_entry():
    assert "mmg_set_sender_variant" in _lib.SYMBOLS and _lib.MIX == {"sum": 0, "prod": 1}
    src = open(os.path.join(REPO, "include", "mmg.h")).read()
    assert "int mmg_set_sender_variant(mmg_handle* h, int mix, int ignore_code, int ignore_receiver);" in src
    assert "enum { MMG_MIX_SUM = 0, MMG_MIX_PROD = 1 };" in src and "#define MMG_VERSION 3" in src
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        fn = lib.mmg_set_sender_variant
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int]
        assert fn(None, 1, 0, 0) < 0                                     # NULL handle: an error, not a crash
        assert b"NULL handle" in lib.mmg_last_error()
        assert lib.mmg_version() == 3


@pytest.mark.parametrize("argv,option", [(["-sender_mix", "prod"], "sender_mix=\"prod\""), (["-sender_mix", "mou"], "4H binary layer"),
                                         (["-ignore_code"], "ignore_code=True"), (["-ignore_receiver"], "ignore_receiver=True")])
def test_command_line_switches_stay_refused_and_name_the_option(argv, option):
    F.define_flags(); F.FLAGS.Reset()
    try:
        F.FLAGS(["model.py"] + argv)
        with pytest.raises(NotImplementedError) as e:
            F.check_supported()
        assert argv[0][1:] in str(e.value) and option in str(e.value) and "Game(" in str(e.value)
    finally:
        F.FLAGS.Reset()


def test_game_options_are_validated_before_any_engine_exists():
    from multimodalgame_amd.game import Game

    class Fl(object):
        desc_attn, sender_mix, flipout_sen, flipout_rec = False, "sum", None, None
        ignore_receiver = ignore_code = visual_attn = bit_flip = False
        max_exchange, fixed_exchange, s_prob_prod = 4, False, True
        entropy_s = entropy_sen = entropy_rec = None
        first_rec, optim_type, learning_rate, top_k_train = 0.0, "RMSprop", 1e-4, 6

    class Ag(object):
        feat_dim, h_dim, w_dim, hid_dim, desc_dim, use_binary, bin_dim_out, z_dim = 512, 256, 32, 64, 100, True, 32, 32
    make = lambda **kw: Game(Ag(), Ag(), None, None, flags=Fl(), device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="4H binary layer"):
        make(sender_mix="mou")
    for bad in ("product", "", None, 1):
        with pytest.raises(ValueError):
            make(sender_mix=bad)
    for variant in (dict(sender_mix="prod"), dict(ignore_code=True), dict(ignore_receiver=True)):
        with pytest.raises(NotImplementedError):
            make(flipout_sen=0.1, **variant)
        with pytest.raises(NotImplementedError):
            make(flipout_rec=0.1, **variant)
        with pytest.raises(NotImplementedError, match="channel_grad"):
            make(autograd=True, channel_grad=True, **variant)
        with pytest.raises(NotImplementedError, match="input_grad"):
            make(autograd=True, input_grad=True, **variant)
    assert make().sender_variant is None and make(sender_mix="sum").sender_variant is None
    assert make(sender_mix="prod", ignore_receiver=True, autograd=True).sender_variant == ("prod", False, True)
    assert make(ignore_code=1).sender_variant == ("sum", True, False)
    assert make(channel_grad=True, input_grad=True, autograd=True).sender_variant is None      # without a variant: as before
