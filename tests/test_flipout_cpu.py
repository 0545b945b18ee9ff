"""Random message flips without a GPU: the oracle wrapper's self-checks (tests/flipout_ref.py), the ctypes declaration of the new
entry, and the command line's -flipout_sen, which stays refused (the capability is Game(..., flipout_sen=P))."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, flags as F
from tests import common, flipout_ref

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=16, learning_rate=1e-4, entropy_rec=0.01,
          entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
          rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)


def _meta():
    from oracle import cpu_ref
    meta = dict(cpu_ref.Flags(**C1).__dict__)
    meta.update(n_classes=30, batch=16, n_minibatches=1, seed_weights=5, seed_data=6, seed_uniforms=7)
    return meta


@pytest.fixture(scope="module")
def plain():
    meta = _meta()
    zero = np.zeros((4, 16, 32), np.float32)
    return meta, flipout_ref.conversation(meta, zero, zero, train=False)


def test_p0_is_the_identity(plain):
    meta, want = plain
    m_z, m_w = flipout_ref.flip_masks(3, 0, 4, 16, 32, 0.0, 0.0, flipout_ref.EVAL_STREAMS)
    assert not m_z.any() and not m_w.any()
    got = flipout_ref.conversation(meta, m_z, m_w, train=False)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_p1_inverts_every_bit_and_leaves_the_probabilities(plain):
    meta, want = plain
    m_z, m_w = flipout_ref.flip_masks(3, 0, 4, 16, 32, 1.0, 1.0, flipout_ref.EVAL_STREAMS)
    assert m_z.all() and m_w.all()
    got = flipout_ref.conversation(meta, m_z, m_w, train=False)
    # step 0 of the sender has seen no flipped message yet: its probabilities are the plain run's, its bits the inverse
    np.testing.assert_array_equal(got["pz"][0], want["pz"][0])
    np.testing.assert_array_equal(got["z"][0], 1.0 - want["z"][0])
    for t in range(4):                                                # every returned bit is the inverse of its own rounded probability
        np.testing.assert_array_equal(got["z"][t], 1.0 - np.round(got["pz"][t]))
        np.testing.assert_array_equal(got["w"][t], 1.0 - np.round(got["pw"][t]))


def test_mask_rates_indices_and_shards():
    m_z, m_w = flipout_ref.flip_masks(11, 2, 10, 50, 32, 0.1, None)
    assert not m_w.any()
    assert abs(float(m_z.mean()) - 0.1) < 0.01
    a, _ = flipout_ref.flip_masks(11, 2, 10, 50, 32, 0.1, None, batch_offset=20, batch=10)
    np.testing.assert_array_equal(a, m_z[:, 20:30])                     # a data-parallel shard draws the global batch's rows
    b, _ = flipout_ref.flip_masks(11, 3, 10, 50, 32, 0.1, None)
    assert (b != m_z).any()                                             # another minibatch counter, other masks


def test_receiver_wrapper_counts_steps_per_conversation(plain):
    """The receiver wrapper applies m_w[t] at its t-th call after reset_state(): a second conversation on the same agents
    starts at t = 0 again."""
    meta, _ = plain
    m_z, m_w = flipout_ref.flip_masks(5, 0, 4, 16, 32, 0.25, 0.25, flipout_ref.EVAL_STREAMS)
    from oracle import cpu_ref
    models, fl = flipout_ref.build(meta, m_z, m_w)
    x, target, desc, _ = common.case_inputs(meta, 0)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=False, break_early=False)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            _, sen_w, rec_w, _, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], None, None, args, fl)
        runs.append((torch.stack(sen_w[0]).numpy(), torch.stack(rec_w[0]).numpy(), torch.stack(rec_w[1]).numpy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(np.abs(runs[0][1] - np.round(runs[0][2])), m_w)


def test_lib_declares_the_entry():
    assert "mmg_set_message_flipout" in _lib.SYMBOLS
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmg.h")).read()
    assert "int mmg_set_message_flipout(mmg_handle* h, int has_sen, float p_sen, int has_rec, float p_rec, int flipout_dev, uint64_t eval_seed);" in src
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        fn = lib.mmg_set_message_flipout
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_uint64]
        assert fn(None, 1, 0.5, 0, 0.0, 0, 0) < 0                       # NULL handle: an error, not a crash
        assert b"NULL handle" in lib.mmg_last_error()


def test_command_line_flipout_stays_refused():
    F.define_flags(); F.FLAGS.Reset()
    try:
        F.FLAGS(["model.py", "-flipout_sen", "0.1"])
        with pytest.raises(NotImplementedError) as e:
            F.check_supported()
        assert "flipout_sen" in str(e.value) and "Game(" in str(e.value)
    finally:
        F.FLAGS.Reset()


def test_game_option_is_validated_before_any_engine_exists():
    from multimodalgame_amd.game import Game

    class Fl(object):
        desc_attn, sender_mix, flipout_sen, flipout_rec = False, "sum", None, None
        ignore_receiver = ignore_code = visual_attn = bit_flip = False
        max_exchange, fixed_exchange, s_prob_prod = 4, False, True
        entropy_s = entropy_sen = entropy_rec = None
        first_rec, optim_type, learning_rate, top_k_train = 0.0, "RMSprop", 1e-4, 6

    class Ag(object):
        feat_dim, h_dim, w_dim, hid_dim, desc_dim, use_binary, bin_dim_out, z_dim = 512, 256, 32, 64, 100, True, 32, 32
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Game(Ag(), Ag(), None, None, flags=Fl(), device="cpu", flipout_sen=bad)
    with pytest.raises(NotImplementedError):
        Game(Ag(), Ag(), None, None, flags=Fl(), device="cpu", flipout_rec=0.1, channel_grad=True)
    g = Game(Ag(), Ag(), None, None, flags=Fl(), device="cpu", flipout_sen=0.1, flipout_dev=True)
    assert g.flipout == (0.1, None, True)
