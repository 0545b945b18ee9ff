"""Message corruption (-bit_flip -corrupt_region, model.py:813-820) on the GPU: every conversation kernel an evaluation pass
can select, against the CPU oracle with the Sender's output corrupted (tests/corrupt_ref.py); the g9 fixtures of the reference
through Game.exchange and eval_dev; no mask outliving its call; the CLI's -eval_only -bit_flip."""
import ctypes
import os

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, misc
from oracle import cpu_ref
from tests import common, corrupt_ref

pytestmark = pytest.mark.gpu

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, batch_size=50, learning_rate=1e-4, entropy_rec=0.01,
          entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
          rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)
C4 = dict(C1, batch_size=32, img_h_dim=1024, rec_w_dim=256, sender_out_dim=256)
C5 = dict(C1, use_binary=False, fixed_exchange=True, batch_size=128, entropy_rec=None, entropy_sen=None, entropy_s=None)
REGION_32 = "0,-1,-2:3,10:14"                                 # bit 0, bit W-1, a mixed-sign range (30, 31, 0, 1, 2)
REGION_256 = "0:3,37,100:104,-2:2,200:203,-1"                 # bits in the first and the last 32-bit word of the mask
REGION_G9 = "0,-1,-2:3,10:14"                                 # tests/golden/make_golden_corrupt.py: REGION_C1


def _meta(flags_kw, n_classes, batch, seed_weights=5, seed_data=6):
    meta = dict(cpu_ref.Flags(**flags_kw).__dict__)
    meta.update(n_classes=n_classes, batch=batch, n_minibatches=1, seed_weights=seed_weights, seed_data=seed_data, seed_uniforms=7)
    return meta


def _oracle(meta, mask):
    """Every step of every sample (what the GPU's run-all evaluation pass stores), the sender corrupted by `mask`."""
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    corrupt_ref.corrupt_sender(models["sender"], mask)
    x, target, desc, _ = common.case_inputs(meta, 0)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=False, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], None, None, args, fl)
    st = lambda v: torch.stack(v).numpy()
    out = dict(s=st(s[1]), ps=st(s[2]), z=st(sen_w[0]), w=st(rec_w[0]), y=st(y))
    if fl.use_binary:
        out.update(pz=st(sen_w[1]), pw=st(rec_w[1]))
    return out


def _gpu(meta, mask):
    eng = common.make_engine(meta)
    x, target, desc, _ = common.case_inputs(meta, 0)
    dev = eng.device
    eng.set_profiling(True)
    eng.forward(torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev), train=False,
                run_all=True, corrupt_mask=mask)
    torch.cuda.synchronize()
    eng.check_sync()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    got = {k: v.cpu().numpy().copy() for k, v in eng.tape.items() if k in ("s", "ps", "z", "pz", "w", "pw", "y")}
    return got, names, eng


def _check(meta, region, kernel):
    """The GPU's corrupted evaluation pass against the oracle wrapper.  Binary: rounding a sigmoid output near 0.5 may differ
    between two correct fp32 summation orders and then changes everything downstream, so each sample is followed up to its
    first such near-tie (test_hip_configs.py: test_wide_receiver_eval_pass_agrees_with_generic_kernels): probabilities within
    1e-4, bits exact, and the message the receiver read is exactly |round(pz) - m|.  Continuous: every message entry within
    1e-4, and none negative (the abs applies to all of them)."""
    W = meta["rec_w_dim"]
    mask = misc.build_mask(region, W).view(-1)
    got, names, _ = _gpu(meta, mask)
    assert kernel in names, names
    want = _oracle(meta, mask)
    T, B = got["s"].shape[0], got["s"].shape[1]
    m = mask.numpy()
    if not meta["use_binary"]:
        np.testing.assert_allclose(got["z"], want["z"], atol=1e-4, rtol=1e-4)
        assert (got["z"] >= 0).all()
        np.testing.assert_allclose(got["y"] - got["y"].mean(-1, keepdims=True), want["y"] - want["y"].mean(-1, keepdims=True), atol=1e-4)
        np.testing.assert_array_equal(got["s"], want["s"])
        return
    ok = np.ones(B, bool)
    checked = 0
    for t in range(T):
        np.testing.assert_allclose(got["pz"][t][ok], want["pz"][t][ok], atol=1e-4, err_msg="pz[%d]" % t)
        ok &= ~(np.abs(want["pz"][t] - 0.5) < 2e-5).any(1)
        np.testing.assert_array_equal(got["z"][t][ok], want["z"][t][ok], err_msg="z[%d]" % t)
        np.testing.assert_array_equal(got["z"][t][ok], np.abs(np.round(got["pz"][t][ok]) - m), err_msg="z[%d] != |round(pz) - m|" % t)
        np.testing.assert_allclose(got["ps"][t][ok], want["ps"][t][ok], atol=1e-4, err_msg="ps[%d]" % t)
        ok &= ~(np.abs(want["ps"][t].reshape(B, -1) - 0.5) < 2e-5).any(1)
        np.testing.assert_array_equal(got["s"][t][ok], want["s"][t][ok], err_msg="s[%d]" % t)
        np.testing.assert_allclose(got["y"][t][ok] - got["y"][t][ok].mean(-1, keepdims=True),
                                   want["y"][t][ok] - want["y"][t][ok].mean(-1, keepdims=True), atol=1e-4, err_msg="y[%d]" % t)
        np.testing.assert_allclose(got["pw"][t][ok], want["pw"][t][ok], atol=1e-4, err_msg="pw[%d]" % t)
        ok &= ~(np.abs(want["pw"][t] - 0.5) < 2e-5).any(1)
        np.testing.assert_array_equal(got["w"][t][ok], want["w"][t][ok], err_msg="w[%d]" % t)
        checked += int(ok.sum())
    assert checked >= T * B // 2, "too few tie-free (step, sample) rows were compared: %d" % checked
    # the mask did something the receiver saw: the corrupted bits are the inverted rounded probabilities
    assert (got["z"][0][:, m != 0] != np.round(got["pz"][0][:, m != 0])).all()


# ------------------------------------------------------------------ one case per conversation kernel of an evaluation pass
def test_fast3_config1_agents():
    """k_conversation_fast3 (the register-resident agents of configs 1-3; profiling scope k_conversation, shared with the
    generic kernel: the shape pins the path)."""
    _check(_meta(C1, 30, 50), REGION_32, "k_conversation")


def test_generic_kernel(monkeypatch):
    """MMG_NO_FAST=1 + MMG_NO_TILE=1: the generic per-sample k_conversation at the same shape."""
    monkeypatch.setenv("MMG_NO_FAST", "1")
    monkeypatch.setenv("MMG_NO_TILE", "1")
    _check(_meta(C1, 30, 50), REGION_32, "k_conversation")


def test_no_fast_takes_the_whole_conversation_tile(monkeypatch):
    """MMG_NO_FAST=1 alone: the sample tiles, at 32-bit messages one k_conv_tile launch for the whole conversation
    (conv_tile_body forms the message)."""
    monkeypatch.setenv("MMG_NO_FAST", "1")
    _check(_meta(C1, 30, 50), REGION_32, "k_conv_tile")


@pytest.mark.parametrize("switch", [None, "MMG_NO_PERSIST_LL", "MMG_NO_FUSED_S", "MMG_NO_RMSG", "MMG_NO_RSAMPLE", "MMG_NO_PERSIST"])
def test_config4_tile_variants(switch, monkeypatch):
    """Config 4's 256-bit agents on the sample tiles.  None: k_conv_persist with fused sender roles handing (value, epoch)
    pairs to per-sample receiver roles (sb_role); MMG_NO_PERSIST_LL: the same roles with payload + counter; MMG_NO_FUSED_S:
    split sender roles (s2_role); MMG_NO_RMSG / MMG_NO_RSAMPLE: per-sample / per-tile receiver roles behind s2_role;
    MMG_NO_PERSIST: per-step launches, the message formed by k_send_s2 and read by k_conv_tile."""
    if switch:
        monkeypatch.setenv(switch, "1")
    _check(_meta(C4, 30, 32), REGION_256, "k_conv_tile" if switch == "MMG_NO_PERSIST" else "k_conv_persist")


@pytest.mark.parametrize("switch", [None, "MMG_NO_RC_PERSIST"])
def test_config4_rec_hidden_256(switch, monkeypatch):
    """rec_hidden 256: k_rc_persist's sender roles (rc_s2_role); MMG_NO_RC_PERSIST: k_send_s2 + the per-step k_rc_* launches."""
    if switch:
        monkeypatch.setenv(switch, "1")
    _check(_meta(dict(C4, rec_hidden=256), 30, 32), REGION_256, "k_conv_rc")


@pytest.mark.parametrize("kernels", ["mc3", "tile-split", "tile"])
def test_config5_continuous(kernels, monkeypatch):
    """Config 5's flavour (1000 classes, continuous messages): k_conversation_mc3 by default; MMG_TILE=1 the sample tiles with
    class helpers (k_conv_split); + MMG_NO_SPLIT=1 the whole conversation in k_conv_tile (conv_tile_body forms the message)."""
    if kernels.startswith("tile"):
        monkeypatch.setenv("MMG_TILE", "1")
    if kernels == "tile":
        monkeypatch.setenv("MMG_NO_SPLIT", "1")
    _check(_meta(C5, 1000, 128), REGION_32, {"mc3": "k_conversation_mc", "tile-split": "k_conv_split", "tile": "k_conv_tile"}[kernels])


def test_many_class_binary():
    """k_conversation_mc (binary messages, more classes than the register-resident kernels hold; continuous messages at this
    shape select k_conversation_mc3, so the binary many-class case is what drives this kernel)."""
    _check(_meta(C1, 200, 40), REGION_32, "k_conversation_mc")


# ------------------------------------------------------------------ the reference's fixtures through Game
def _game(meta):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    fl = common.flags_from_meta(meta)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0")
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    eng.params["receiver"]["s.bias"].fill_(1.2)                   # as g4_eval_c1 / g9_eval_corrupt_c1
    return game


def _exchange(game, x, target, desc, corrupt):
    from multimodalgame_amd.game import get_rec_outp
    dev = torch.device("cuda:0")
    args = dict(data=torch.from_numpy(x).to(dev), target=torch.from_numpy(target).to(dev), desc=torch.from_numpy(desc).to(dev),
                train=False, break_early=True, corrupt=corrupt, corrupt_region=REGION_G9 if corrupt else None)
    s, sen_w, rec_w, y, _, _ = game.exchange(args)
    y_masks = [torch.min(1 - m1, m2) for m1, m2 in zip(s[0][1:], s[0][:-1])]
    outp, _ = get_rec_outp(y, y_masks)
    dist = torch.nn.functional.log_softmax(outp, dim=1)
    st = lambda v: torch.stack(v).cpu().numpy()
    return dict(n_steps=len(y), s_masks=st(s[0]), s_feats=st(s[1]), sen_feats=st(sen_w[0]), sen_probs=st(sen_w[1]),
                rec_feats=st(rec_w[0]), y=st(y), dist=dist.cpu().numpy())


def test_g9_through_game_exchange():
    z, meta = common.load_golden("g9_eval_corrupt_c1")
    game = _game(meta)
    x, target, desc = cpu_ref.synthetic_batch(meta["batch"], meta["n_classes"], 512, 100, seed=meta["seed_data"])
    plain = _exchange(game, x, target, desc, False)
    got = _exchange(game, x, target, desc, True)
    assert got["n_steps"] == int(z["n_steps"])
    n = got["n_steps"]
    np.testing.assert_array_equal(got["s_masks"].astype(np.uint8), z["s_masks"])
    np.testing.assert_array_equal(got["s_feats"], z["s_feats"])
    np.testing.assert_array_equal(got["sen_feats"], z["sen_feats"])
    np.testing.assert_array_equal(got["rec_feats"], z["rec_feats"])
    np.testing.assert_allclose(got["y"], z["y"], atol=1e-4)
    np.testing.assert_allclose(got["dist"], z["dist"], atol=1e-4)
    k = z["top_k_ind"].shape[1]
    got_hit = (np.argsort(-got["dist"], axis=1, kind="stable")[:, :k] == target.reshape(-1, 1)).any(1)
    np.testing.assert_array_equal(got_hit, (z["top_k_ind"] == target.reshape(-1, 1)).any(1))
    assert int(got_hit.sum()) == int(z["hits"])
    # the Sender's probabilities are not corrupted: at step 0 they are the uncorrupted run's, bit for bit
    np.testing.assert_array_equal(got["sen_probs"][0], plain["sen_probs"][0])
    np.testing.assert_allclose(got["sen_probs"][:n], z["sen_probs"], atol=1e-4)
    with pytest.raises(NotImplementedError):
        game.exchange(dict(data=torch.from_numpy(x).cuda(), target=torch.from_numpy(target).cuda(), desc=torch.from_numpy(desc).cuda(),
                           train=True, corrupt=True, corrupt_region=REGION_G9))


def _with_flags(argv):
    from multimodalgame_amd import flags as _flags
    _flags.define_flags(); _flags.FLAGS.Reset()
    _flags.FLAGS(argv)
    _flags.default_flags(argv)
    return _flags.FLAGS


def test_g9_through_eval_dev(tmp_path, monkeypatch):
    """model.eval_dev under -bit_flip -corrupt_region: the accuracy of the reference's corrupted conversation on the g9 batch."""
    from multimodalgame_amd import flags as _flags, model
    z, meta = common.load_golden("g9_eval_corrupt_c1")
    try:
        F = _with_flags(["model.py", "-model_type", "Adaptive", "-max_exchange", "10", "-rec_w_dim", "32", "-sender_out_dim", "32",
                         "-img_h_dim", "256", "-rec_hidden", "64", "-wv_dim", "100", "-use_binary", "-top_k_dev", "6",
                         "-log_path", str(tmp_path), "-bit_flip", "-corrupt_region", REGION_G9])
        F.img_feat_dim = 512
        game = _game(meta)
        B = meta["batch"]
        x, target, desc = cpu_ref.synthetic_batch(B, meta["n_classes"], 512, 100, seed=meta["seed_data"])
        dev = torch.device("cuda:0")

        def fake_load_hdf5(dev_file, batch_size, epoch, shuffle, truncate_final_batch=False, map_labels=int, feats=(), device=None, **kw):
            yield {"target": torch.from_numpy(target).to(dev), "avgpool_512": torch.from_numpy(x).to(dev)}
        monkeypatch.setattr(model, "load_hdf5", fake_load_hdf5)
        acc, extra = model.eval_dev("dev", B, 0, False, 6, game, torch.from_numpy(desc).to(dev), int, str(tmp_path / "c.txt"), dev)
        assert acc == pytest.approx(int(z["hits"]) / float(B), abs=1e-12)
        assert float(extra["conversation_lengths_mean"]) == pytest.approx(float(z["conversation_lengths"].mean()), abs=1e-6)    # (fixture: float32)
    finally:
        _flags.FLAGS.Reset()


# ------------------------------------------------------------------ no mask outlives its call
def test_mask_does_not_leak_into_later_calls():
    meta = _meta(C1, 30, 50)
    x, target, desc, _ = common.case_inputs(meta, 0)
    mask = misc.build_mask(REGION_32, 32)

    def run(corrupt_first):
        eng = common.make_engine(meta)
        dev = eng.device
        xd, td, dd = torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev)
        if corrupt_first:
            eng.forward(xd, td, dd, train=False, run_all=True, corrupt_mask=mask)
        eng.forward(xd, td, dd, train=False, run_all=True)
        tape = {k: v.cpu().numpy().copy() for k, v in eng.tape.items() if k in ("s", "ps", "z", "pz", "w", "pw", "y", "dist")}
        eng.train_step(xd, td, dd, seed=3)
        torch.cuda.synchronize()
        eng.check_sync()
        return tape, eng.flat_params.cpu().numpy().copy(), eng.tape["losses"].cpu().numpy().copy()
    tape_a, params_a, losses_a = run(True)
    tape_b, params_b, losses_b = run(False)
    for k in tape_b:
        np.testing.assert_array_equal(tape_a[k], tape_b[k], err_msg=k)
    np.testing.assert_array_equal(params_a, params_b)
    np.testing.assert_array_equal(losses_a, losses_b)


def test_training_entries_refuse_while_a_mask_is_set():
    meta = _meta(C1, 30, 50)
    x, target, desc, _ = common.case_inputs(meta, 0)
    eng = common.make_engine(meta)
    dev = eng.device
    xd, td, dd = torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev)
    before = eng.flat_params.cpu().numpy().copy()
    eng.set_message_corruption(misc.build_mask(REGION_32, 32))
    for call in (lambda: eng.train_step(xd, td, dd, seed=1), lambda: eng.forward(xd, td, dd, train=True, run_all=True),
                 lambda: eng.train_steps(xd, td, dd, 1, seed=1), lambda: eng.dp_train_step(xd, td, dd, seed=1, reduce=False),
                 lambda: eng.dp_train_steps(xd, td, dd, 1, seed=1, reduce=False)):
        with pytest.raises(_lib.MmgError, match="corruption mask is set"):
            call()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eng.flat_params.cpu().numpy(), before)
    with pytest.raises(NotImplementedError):
        eng.forward(xd, td, dd, train=True, corrupt_mask=misc.build_mask(REGION_32, 32))
    # a mask of the wrong length, or with an entry other than 0 / 1, is refused and leaves the mask set before in place
    assert eng.lib.mmg_set_message_corruption(eng.handle, (ctypes.c_uint8 * 31)(), 31) < 0
    assert eng.lib.mmg_set_message_corruption(eng.handle, (ctypes.c_uint8 * 32)(*([2] + [0] * 31)), 32) < 0
    with pytest.raises(_lib.MmgError, match="corruption mask is set"):
        eng.train_step(xd, td, dd, seed=1)
    eng.set_message_corruption(None)
    eng.train_step(xd, td, dd, seed=1)
    torch.cuda.synchronize()
    assert not np.array_equal(eng.flat_params.cpu().numpy(), before)


# ------------------------------------------------------------------ the command line
def test_cli_eval_only_with_bit_flip(tmp_path, monkeypatch):
    """-eval_only -bit_flip -corrupt_region on -synthetic_data writes the CSV line; its accuracy is eval_dev's through
    Game.eval_forward with the same mask handed over explicitly."""
    from multimodalgame_amd import flags as _flags, model
    from multimodalgame_amd.game import Game
    tmp = str(tmp_path)
    base = ["model.py", "-experiment_name", "bf", "-model_type", "Adaptive", "-max_exchange", "6", "-batch_size", "32",
            "-rec_w_dim", "32", "-sender_out_dim", "32", "-img_h_dim", "256", "-rec_hidden", "64", "-use_binary",
            "-max_epoch", "1", "-top_k_dev", "6", "-top_k_train", "6", "-wv_dim", "100", "-log_path", os.path.join(tmp, "logs"),
            "-synthetic_data", os.path.join(tmp, "data"), "-log_interval", "5", "-save_after", "4", "-save_interval", "4"]
    seen = {}
    real_eval_dev = model.eval_dev

    def spy(*a, **kw):
        seen["args"], seen["kw"] = a, kw
        return real_eval_dev(*a, **kw)
    try:
        _flags.define_flags(); _flags.FLAGS.Reset()
        model.main(base + ["-max_steps", "5"])
        _flags.FLAGS.Reset()
        monkeypatch.setattr(model, "eval_dev", spy)
        model.main(base + ["-eval_only", "-checkpoint", os.path.join(tmp, "logs", "bf.pt"), "-bit_flip", "-corrupt_region", "0:8,-1"])
        csv = open(_flags.FLAGS.eval_csv_file).read().splitlines()
        assert len(csv) == 2
        acc_cli = float(csv[1].split(",")[5])
        # the same dev pass with -nobit_flip, the mask handed to Game.eval_forward explicitly
        game = seen["args"][5]
        mask = misc.build_mask("0:8,-1", 32)
        _flags.FLAGS.bit_flip = False
        plain = Game.eval_forward
        monkeypatch.setattr(Game, "eval_forward", lambda self, d, t, ds, corrupt_mask=None: plain(self, d, t, ds, corrupt_mask=mask))
        acc_game, _ = real_eval_dev(*seen["args"], **seen["kw"])
        assert acc_cli == pytest.approx(acc_game, abs=1e-12)
        monkeypatch.setattr(Game, "eval_forward", plain)
        acc_plain, _ = real_eval_dev(*seen["args"], **seen["kw"])
        assert np.isfinite(acc_plain)
    finally:
        _flags.FLAGS.Reset()
