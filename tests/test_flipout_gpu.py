"""Random message flips (the noisy channel of -flipout_sen / -flipout_rec / -flipout_dev, model.py:233-234, 467-468, 554-568;
include/mmg.h: mmg_set_message_flipout) on the GPU, on both conversation kernels that serve a flipping handle -- the
register-resident k_conversation_fast3 chain and the generic k_conversation -- against the flip masks restated with
tests/philox_ref and against the CPU oracle with wrapped agents (tests/flipout_ref.py).

All cases use config 1's agents (H 256, W 32, R 64, V 100, K 500) with 30 classes, weights seed 5, data seed 6."""
import ctypes as C

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from tests import common, flipout_ref

pytestmark = pytest.mark.gpu

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=16, learning_rate=1e-4, entropy_rec=0.01,
          entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
          rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)
W = 32
P_SEN, P_REC = 0.25, 0.05
SEED, EVAL_SEED = 21, 77
KERNELS = ["fast3", "generic"]
ATOL, RTOL = 1e-4, 1e-3          # tests/test_hip_parity.py, g2_adaptive_c1: forward 1e-4 absolute, gradients 1e-4 + 1e-3 |v|
TAPE_KEYS = ("s", "ps", "z", "pz", "w", "pw", "y", "lp_z", "lp_w")


def _meta(batch=16, T=4):
    from oracle import cpu_ref
    meta = dict(cpu_ref.Flags(**dict(C1, max_exchange=T, batch_size=batch)).__dict__)
    meta.update(n_classes=30, batch=batch, n_minibatches=1, seed_weights=5, seed_data=6, seed_uniforms=7)
    return meta


def _select(kernel, monkeypatch):
    """The environment switches are read when a handle is created."""
    if kernel == "generic":
        monkeypatch.setenv("MMG_NO_FAST", "1")
        monkeypatch.setenv("MMG_NO_TILE", "1")


def _inputs(meta, eng, i=0):
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    u = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (u_z, u_s[..., 0], u_w))
    return (d(x), d(target), d(desc)), tuple(d(a) for a in u), u


def _tape(eng, keys=TAPE_KEYS):
    torch.cuda.synchronize()
    eng.check_sync()
    return {k: eng.tape[k].cpu().numpy().copy() for k in keys}


def _scopes(eng, call):
    eng.set_profiling(True)
    call()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _train_forward(meta, p_sen, p_rec, seed=SEED, **over):
    """A training run-all forward with injected uniforms on a fresh flipping engine: (tape, host uniforms, engine)."""
    eng = common.make_engine(meta, **over)
    eng.set_message_flipout(p_sen, p_rec)
    xs, ud, uh = _inputs(meta, eng)
    eng.forward(*xs, *ud, seed=seed, train=True, run_all=True)
    tp = _tape(eng)
    assert int(eng.tape["counter"][0]) == 1                         # the first minibatch of a handle draws with counter 1
    return tp, uh, eng


def _own_flips(tp, uh):
    """Which bits of the GPU's tape differ from the GPU's own sample u < p: exact, no near-tie can interfere."""
    return (tp["z"] != (uh[0] < tp["pz"])).astype(np.float32), (tp["w"] != (uh[2] < tp["pw"])).astype(np.float32)


# ------------------------------------------------------------------ 1. flip positions, exact
@pytest.mark.parametrize("kernel", KERNELS)
def test_flip_positions_are_the_philox_masks(kernel, monkeypatch):
    _select(kernel, monkeypatch)
    meta = _meta()
    tp, uh, eng = _train_forward(meta, P_SEN, P_REC)
    m_z, m_w = flipout_ref.flip_masks(SEED, 1, 4, 16, W, P_SEN, P_REC)
    f_z, f_w = _own_flips(tp, uh)
    np.testing.assert_array_equal(f_z, m_z)
    np.testing.assert_array_equal(f_w, m_w)
    assert 0 < m_z.sum() < m_z.size and 0 < m_w.sum() < m_z.sum()
    assert set(np.unique(tp["z"])) <= {0.0, 1.0} and set(np.unique(tp["w"])) <= {0.0, 1.0}
    # the log-likelihood sums score the returned (flipped) bits, the probabilities are the logits' own (model.py:908-910)
    for bits, p, lp in ((tp["z"], tp["pz"], tp["lp_z"]), (tp["w"], tp["pw"], tp["lp_w"])):
        b, q = bits.astype(np.float64), p.astype(np.float64)
        want = (b * np.log(q + 1e-8) + (1 - b) * np.log(1 - q + 1e-8)).sum(-1)
        np.testing.assert_allclose(lp.reshape(want.shape), want, atol=1e-4, rtol=1e-5)
    xs, _, _ = _inputs(meta, eng)
    names = _scopes(eng, lambda: eng.train_step(*xs, seed=SEED))
    assert "k_game" not in names and "k_conversation" in names and "k_wgrad" in names, names


# ------------------------------------------------------------------ 2. p = 1 and p = 0
@pytest.mark.parametrize("kernel", KERNELS)
def test_p1_inverts_every_sample(kernel, monkeypatch):
    _select(kernel, monkeypatch)
    tp, uh, _ = _train_forward(_meta(), 1.0, 1.0)
    f_z, f_w = _own_flips(tp, uh)
    assert f_z.all() and f_w.all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_p0_is_the_unflipped_step_bit_for_bit(kernel, monkeypatch):
    """p = 0.0 set (not absent): the flipping kernels with masks that never flip -- the same launches and draws as a handle
    without flips that MMG_NO_GAME=1 keeps off the one-launch step."""
    _select(kernel, monkeypatch)
    meta = _meta()

    def run(flip):
        eng = common.make_engine(meta)
        if flip:
            eng.set_message_flipout(0.0, 0.0)
        xs, _, _ = _inputs(meta, eng)
        names = _scopes(eng, lambda: eng.train_step(*xs, seed=SEED))
        return _tape(eng, TAPE_KEYS + ("losses",)), eng.flat_params.cpu().numpy().copy(), names
    tape_a, params_a, names_a = run(True)
    monkeypatch.setenv("MMG_NO_GAME", "1")
    tape_b, params_b, names_b = run(False)
    assert names_a == names_b and "k_game" not in names_a, (names_a, names_b)
    for k in tape_b:
        np.testing.assert_array_equal(tape_a[k], tape_b[k], err_msg=k)
    np.testing.assert_array_equal(params_a, params_b)


# ------------------------------------------------------------------ 3. the conversation against the oracle wrapper
def _check(got, want, ties, label):
    """tests/test_corrupt_gpu.py's rule: every sample is followed up to its first near-tie -- a probability within 2e-5 of the
    threshold its bit is decided at (0.5 when rounding, the uniform when sampling), where two correct fp32 summation orders
    may decide differently and everything downstream then differs --, probabilities within 1e-4, bits exact."""
    T, B = got["s"].shape[0], got["s"].shape[1]
    ok = np.ones(B, bool)
    checked = 0
    for t in range(T):
        np.testing.assert_allclose(got["pz"][t][ok], want["pz"][t][ok], atol=1e-4, err_msg="%s pz[%d]" % (label, t))
        ok &= ~(np.abs(want["pz"][t] - ties[0][t]) < 2e-5).any(1)
        np.testing.assert_array_equal(got["z"][t][ok], want["z"][t][ok], err_msg="%s z[%d]" % (label, t))
        np.testing.assert_allclose(got["ps"][t][ok], want["ps"][t][ok], atol=1e-4, err_msg="%s ps[%d]" % (label, t))
        ok &= ~(np.abs(want["ps"][t].reshape(B, -1) - ties[1][t].reshape(B, -1)) < 2e-5).any(1)
        np.testing.assert_array_equal(got["s"][t][ok], want["s"][t][ok], err_msg="%s s[%d]" % (label, t))
        np.testing.assert_allclose(got["y"][t][ok] - got["y"][t][ok].mean(-1, keepdims=True),
                                   want["y"][t][ok] - want["y"][t][ok].mean(-1, keepdims=True), atol=1e-4, err_msg="%s y[%d]" % (label, t))
        np.testing.assert_allclose(got["pw"][t][ok], want["pw"][t][ok], atol=1e-4, err_msg="%s pw[%d]" % (label, t))
        ok &= ~(np.abs(want["pw"][t] - ties[2][t]) < 2e-5).any(1)
        np.testing.assert_array_equal(got["w"][t][ok], want["w"][t][ok], err_msg="%s w[%d]" % (label, t))
        checked += int(ok.sum())
    assert 4 * checked >= 3 * T * B, "%s: too few tie-free (step, sample) rows were compared: %d of %d" % (label, checked, T * B)


SHAPES = [(16, 4, P_SEN, P_REC), (50, 10, 0.1, 0.1)]
_ORACLE = {}


def _oracle(key, make):
    """One oracle run per (mode, shape), shared by the two kernels' cases and left unchanged."""
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


@pytest.mark.parametrize("batch,T,p_sen,p_rec", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_training_conversation_matches_the_oracle_wrapper(kernel, batch, T, p_sen, p_rec, monkeypatch):
    _select(kernel, monkeypatch)
    meta = _meta(batch, T)
    tp, uh, _ = _train_forward(meta, p_sen, p_rec)
    m_z, m_w = flipout_ref.flip_masks(SEED, 1, T, batch, W, p_sen, p_rec)
    _, _, _, u = common.case_inputs(meta, 0)
    want = _oracle(("train", batch, T), lambda: flipout_ref.conversation(meta, m_z, m_w, train=True, uniforms=u))
    assert (want["z"] != (uh[0] < want["pz"])).any()                  # the oracle's messages are flipped ones
    _check(tp, want, (uh[0], uh[1], uh[2]), "train/%s" % kernel)


@pytest.mark.parametrize("batch,T,p_sen,p_rec", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_evaluation_under_flipout_dev(kernel, batch, T, p_sen, p_rec, monkeypatch):
    """An evaluation conversation under flipout_dev against the oracle wrapper (streams 5 / 6, key = eval_seed, counter = the
    evaluation conversations since the setter call); k_eval_reduce counts Hamming distances on the flipped tape; the next
    conversation draws other masks; a training step afterwards draws what it would have drawn without the evaluations."""
    _select(kernel, monkeypatch)
    meta = _meta(batch, T)
    eng = common.make_engine(meta)
    eng.set_message_flipout(p_sen, p_rec, dev=True, eval_seed=EVAL_SEED)
    xs, _, _ = _inputs(meta, eng)
    half = np.float32(0.5)
    masks = []
    for c1 in (0, 1):
        _, ham = eng.eval_steps(xs[0], xs[1], xs[2], 1, 6, eng.eval_acc())
        tp = _tape(eng)
        m_z, m_w = flipout_ref.flip_masks(EVAL_SEED, c1, T, batch, W, p_sen, p_rec, flipout_ref.EVAL_STREAMS)
        np.testing.assert_array_equal(tp["z"], np.abs(np.round(tp["pz"]) - m_z), err_msg="z, evaluation %d" % c1)
        np.testing.assert_array_equal(tp["w"], np.abs(np.round(tp["pw"]) - m_w), err_msg="w, evaluation %d" % c1)
        masks.append((m_z, m_w))
        ham = ham.cpu().numpy().reshape(-1)
        for which, key in enumerate(("z", "w")):
            prev = np.concatenate([np.zeros_like(tp[key][:1]), tp[key][:-1]])
            np.testing.assert_array_equal(ham[1 + which * T:1 + (which + 1) * T], np.abs(tp[key] - prev).sum((1, 2)).astype(np.int64))
        if c1 == 0:
            want = _oracle(("eval", batch, T), lambda: flipout_ref.conversation(meta, m_z, m_w, train=False))
            _check(tp, want, ([half] * T, [np.full((batch, 1), half)] * T, [half] * T), "eval/%s" % kernel)
    assert (masks[0][0] != masks[1][0]).any() and (masks[0][1] != masks[1][1]).any()
    assert int(eng.tape["counter"][0]) == 0                           # evaluations leave the minibatch counter alone
    eng.train_step(*xs, seed=SEED)
    after = _tape(eng, ("z", "pz", "tstar", "losses"))
    params = eng.flat_params.cpu().numpy().copy()
    fresh = common.make_engine(meta)
    fresh.set_message_flipout(p_sen, p_rec, dev=True, eval_seed=EVAL_SEED)
    fresh.train_step(*xs, seed=SEED)
    plain = _tape(fresh, ("z", "pz", "tstar", "losses"))
    np.testing.assert_array_equal(after["tstar"], plain["tstar"])
    live = np.arange(T)[:, None] <= plain["tstar"].reshape(1, -1)      # a training step stores the live (step, sample) rows only
    for k in ("z", "pz"):
        np.testing.assert_array_equal(after[k][live], plain[k][live], err_msg=k)
    np.testing.assert_array_equal(after["losses"], plain["losses"])
    np.testing.assert_array_equal(params, fresh.flat_params.cpu().numpy())


def test_evaluation_without_flipout_dev_does_not_flip():
    meta = _meta()
    eng = common.make_engine(meta)
    eng.set_message_flipout(1.0, 1.0, dev=False)
    xs, _, _ = _inputs(meta, eng)
    eng.forward(*xs, train=False, run_all=True)
    tp = _tape(eng)
    np.testing.assert_array_equal(tp["z"], np.round(tp["pz"]))
    np.testing.assert_array_equal(tp["w"], np.round(tp["pw"]))


# ------------------------------------------------------------------ 4. one training minibatch against the oracle
@pytest.mark.parametrize("kernel", KERNELS)
def test_training_minibatch_matches_the_oracle(kernel, monkeypatch):
    """cpu_ref.train_minibatch on wrapped agents against the phased step (every array exchange() returns, the flipped bits
    exact) and against the fused step (what training reads) -- losses, gradients and updated parameters at the tolerances of
    tests/test_hip_parity.py for g2_adaptive_c1: flips add no arithmetic.  The injected uniforms keep every draw 1e-4 away from
    its probability (flipout_ref.separated_uniforms: common.separate_draws for wrapped agents)."""
    _select(kernel, monkeypatch)
    meta = _meta()
    name = "flipout_c1"
    m_z, m_w = flipout_ref.flip_masks(0, 1, 4, 16, W, P_SEN, P_REC)       # hip_train_case trains with seed 0, counter 1

    def oracle():
        u = flipout_ref.separated_uniforms(meta, m_z, m_w)
        return u, flipout_ref.train_minibatch(meta, m_z, m_w, u)[0]
    us, want = _oracle(("minibatch",), oracle)
    make = common.make_engine

    def flipping(meta_, tweak=None, **over):
        eng = make(meta_, tweak=tweak, **over)
        eng.set_message_flipout(P_SEN, P_REC)
        return eng
    monkeypatch.setattr(common, "make_engine", flipping)
    monkeypatch.setitem(common.U_OVERRIDES, name, lambda i, u_z, u_s, u_w: us)
    n = int(want["mb0.n_steps"])
    flipped = np.asarray(want["mb0.sen_feats"]) != (np.asarray(us[0])[:n] < np.asarray(want["mb0.sen_probs"]))
    assert flipped.any()                                              # the oracle trained on flipped messages
    got, eng = common.hip_train_case(name, meta)
    common.assert_parity(got, want, [], eng, None, skip=("y2.bias",), atol=ATOL, rtol=RTOL)
    keep = ("losses", "n_steps", "hits", "logs", "outp", "dist", ".g.", ".p.", "gradnorm")      # tests/test_hip_parity.py: FUSED_KEEP
    pick = lambda d: {k: d[k] for k in d if any(t in k for t in keep)}
    fused, eng = common.hip_train_case(name, meta, fused=True)
    common.assert_parity(pick(fused), pick(want), [], eng, None, skip=("y2.bias",), atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------ 5. plumbing
def test_train_steps_equals_two_train_step_calls():
    meta = _meta()

    def run(loop):
        eng = common.make_engine(meta)
        eng.set_message_flipout(P_SEN, P_REC)
        a, b = _inputs(meta, eng, 0)[0], _inputs(meta, eng, 1)[0]
        if loop:
            eng.train_steps(torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]), a[2], 2, seed=SEED)
        else:
            eng.train_step(*a, seed=SEED)
            eng.train_step(b[0], b[1], a[2], seed=SEED)
        return _tape(eng, TAPE_KEYS + ("losses",)), eng.flat_params.cpu().numpy().copy()
    tape_a, params_a = run(True)
    tape_b, params_b = run(False)
    for k in tape_b:
        np.testing.assert_array_equal(tape_a[k], tape_b[k], err_msg=k)
    np.testing.assert_array_equal(params_a, params_b)


def test_data_parallel_shards_draw_the_global_batch_rows():
    meta = _meta()
    tp, uh, _ = _train_forward(meta, P_SEN, P_REC)
    f_z, f_w = _own_flips(tp, uh)
    m_z, m_w = flipout_ref.flip_masks(SEED, 1, 4, 16, W, P_SEN, P_REC)
    for off in (0, 8):
        eng = common.make_engine(meta, batch=8, global_batch=16, batch_offset=off)
        eng.set_message_flipout(P_SEN, P_REC)
        xs, ud, _ = _inputs(meta, eng)
        rows = slice(off, off + 8)
        eng.dp_train_step(xs[0][rows].contiguous(), xs[1][rows].contiguous(), xs[2], ud[0][:, rows].contiguous(),
                          ud[1][:, rows].contiguous(), ud[2][:, rows].contiguous(), seed=SEED, full_tape=True, reduce=False)
        sh = _tape(eng)
        s_z, s_w = _own_flips(sh, tuple(u[:, rows] for u in uh))
        for got, single, ref in ((s_z, f_z, m_z), (s_w, f_w, m_w)):
            np.testing.assert_array_equal(got, single[:, rows], err_msg="offset %d" % off)
            np.testing.assert_array_equal(got, ref[:, rows], err_msg="offset %d" % off)


def test_clearing_restores_the_one_launch_step():
    meta = _meta()
    eng = common.make_engine(meta)
    xs, _, _ = _inputs(meta, eng)
    eng.set_message_flipout(P_SEN, P_REC, dev=True, eval_seed=EVAL_SEED)
    eng.forward(*xs, train=False, run_all=True)                       # a flipping evaluation in between changes nothing that trains
    eng.set_message_flipout(None, None)
    names = _scopes(eng, lambda: eng.train_step(*xs, seed=SEED))
    assert names == ["k_game", "k_wgrad"], names
    fresh = common.make_engine(meta)
    fresh.train_step(*xs, seed=SEED)
    a, b = _tape(eng, TAPE_KEYS + ("losses", "tstar")), _tape(fresh, TAPE_KEYS + ("losses", "tstar"))
    np.testing.assert_array_equal(a["tstar"], b["tstar"])
    live = np.arange(4)[:, None] <= b["tstar"].reshape(1, -1)         # a training step stores the live (step, sample) rows only
    for k in ("s", "ps", "z", "pz", "y", "lp_z"):
        np.testing.assert_array_equal(a[k][live], b[k][live], err_msg=k)
    np.testing.assert_array_equal(a["losses"], b["losses"])
    np.testing.assert_array_equal(eng.flat_params.cpu().numpy(), fresh.flat_params.cpu().numpy())


def test_bad_probabilities_are_refused_and_the_setting_stays():
    meta = _meta()
    eng = common.make_engine(meta)
    eng.set_message_flipout(P_SEN, None)
    for bad in (-0.1, 1.5, float("nan")):
        assert eng.lib.mmg_set_message_flipout(eng.handle, 1, C.c_float(bad), 0, C.c_float(0.0), 0, 0) < 0
        assert b"p_sen" in eng.lib.mmg_last_error()
        assert eng.lib.mmg_set_message_flipout(eng.handle, 1, C.c_float(0.5), 1, C.c_float(bad), 0, 0) < 0
        with pytest.raises(_lib.MmgError):
            eng.set_message_flipout(0.5, bad)
    xs, ud, uh = _inputs(meta, eng)
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    f_z, f_w = _own_flips(_tape(eng), uh)
    m_z, _ = flipout_ref.flip_masks(SEED, 1, 4, 16, W, P_SEN, None)
    np.testing.assert_array_equal(f_z, m_z)
    assert not f_w.any()


def _game(meta, **kw):
    from multimodalgame_amd.agents import Baseline, Receiver, Sender
    from multimodalgame_amd.game import Game
    from oracle import cpu_ref
    fl = common.flags_from_meta(meta)
    sender = Sender("avgpool_512", fl.img_feat_dim, fl.img_h_dim, fl.rec_w_dim, fl.sender_out_dim, fl.use_binary)
    receiver = Receiver(fl.sender_out_dim, fl.wv_dim, fl.rec_hidden, 1, fl.rec_w_dim, 1, fl.use_binary)
    game = Game(sender, receiver, Baseline(fl.baseline_hid_dim, fl.img_h_dim, fl.rec_w_dim, 0),
                Baseline(fl.baseline_hid_dim, 0, fl.rec_w_dim, fl.rec_hidden), flags=fl, device="cuda:0", **kw)
    eng = game.engine_for(meta["batch"], meta["n_classes"])
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    return game, eng, fl


def test_game_option_flips_and_backpropagates():
    """Game(flipout_sen=...) through exchange(train=True) with autograd: the returned sen_feats are the flipped bits, and the
    sender's gradient of the losses module's REINFORCE loss on them is the one the library's own backward pass forms from the
    flipped tape of the same minibatch."""
    from multimodalgame_amd import losses
    meta = _meta()
    game, eng, fl = _game(meta, seed=SEED, autograd=True, flipout_sen=P_SEN, flipout_rec=P_REC)
    assert eng.flipout == (P_SEN, P_REC, False)
    xs, ud, uh = _inputs(meta, eng)
    out = game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], uniforms=ud, train=True, break_early=True))
    n = len(out[3])
    sen_feats = torch.stack(out[1][0]).cpu().numpy()
    sen_probs = torch.stack(out[1][1]).detach().cpu().numpy()
    m_z, m_w = flipout_ref.flip_masks(SEED, 1, 4, 16, W, P_SEN, P_REC)
    np.testing.assert_array_equal((sen_feats != (uh[0][:n] < sen_probs)).astype(np.float32), m_z[:n])
    rec_feats = torch.stack(out[2][0]).cpu().numpy()
    np.testing.assert_array_equal((rec_feats != (uh[2][:n] < torch.stack(out[2][1]).detach().cpu().numpy())).astype(np.float32), m_w[:n])
    loss = losses.training_losses(out, xs[1], fl)
    for m in game.modules.values():
        m.zero_grad(set_to_none=True)
    loss["sender"].backward()
    got = {k: p.grad.detach().cpu().clone() for k, p in game.modules["sender"].named_parameters()}
    assert any(float(g.abs().max()) > 0 for g in got.values())
    game.set_counters(0, 0)                                           # the same minibatch again: the same flip masks
    eng.forward(*xs, *ud, seed=SEED, train=True, run_all=True)
    eng.loss_stats()
    eng.backward(*xs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eng.tape["z"][:n].cpu().numpy(), sen_feats)
    for k, g in got.items():
        want = eng.grads["sender"][k].detach().cpu()
        np.testing.assert_allclose(g.numpy(), want.numpy(), atol=ATOL, rtol=RTOL, err_msg=k)


def test_channel_grad_with_flips_raises():
    meta = _meta()
    with pytest.raises(NotImplementedError):
        _game(meta, autograd=True, channel_grad=True, flipout_sen=P_SEN)
    game, eng, _ = _game(meta, autograd=True, flipout_sen=P_SEN)
    xs, ud, _ = _inputs(meta, eng)
    with pytest.raises(NotImplementedError):
        game.exchange(dict(data=xs[0], target=xs[1], desc=xs[2], uniforms=ud, train=True, break_early=True, channel_grad=True))


def test_module_forward_flips_at_the_agent_level_entries():
    """The agent-level entries run k_conversation through its step window: one Sender / Receiver step of a flipping engine
    flips its own sample at the masks' positions of that step, as the reference's modules do."""
    meta = _meta()
    eng = common.make_engine(meta)
    eng.set_message_flipout(P_SEN, P_REC)
    xs, ud, uh = _inputs(meta, eng)
    m_z, m_w = flipout_ref.flip_masks(SEED, 1, 4, 16, W, P_SEN, P_REC)
    z0, pz0, _ = eng.sender_forward(xs[0], None, 0, True, u_z=ud[0][0].contiguous(), seed=SEED)
    torch.cuda.synchronize()
    assert int(eng.tape["counter"][0]) == 1
    np.testing.assert_array_equal((z0.cpu().numpy() != (uh[0][0] < pz0.cpu().numpy())).astype(np.float32), m_z[0])
    eng.tape["counter"][0] = 0                                        # the receiver's step of the same minibatch
    h = torch.zeros(16, 64, device=eng.device)
    sp = torch.ones(16, device=eng.device)
    _, _, w0, pw0, _, _ = eng.receiver_forward(z0, xs[2], h, sp, True, 0, True, u_s=ud[1][0].contiguous(), u_w=ud[2][0].contiguous(), seed=SEED)
    torch.cuda.synchronize()
    np.testing.assert_array_equal((w0.cpu().numpy() != (uh[2][0] < pw0.cpu().numpy())).astype(np.float32), m_w[0])
    # evaluation under flipout_dev: a sender step 0 begins a conversation (the next evaluation count), the receiver's step joins it
    eng.set_message_flipout(P_SEN, P_REC, dev=True, eval_seed=EVAL_SEED)
    for c1 in (0, 1):
        e_z, e_w = flipout_ref.flip_masks(EVAL_SEED, c1, 4, 16, W, P_SEN, P_REC, flipout_ref.EVAL_STREAMS)
        z0, pz0, _ = eng.sender_forward(xs[0], None, 0, False)
        _, _, w0, pw0, _, _ = eng.receiver_forward(z0, xs[2], torch.zeros(16, 64, device=eng.device), sp, True, 0, False)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(z0.cpu().numpy(), np.abs(np.round(pz0.cpu().numpy()) - e_z[0]))
        np.testing.assert_array_equal(w0.cpu().numpy(), np.abs(np.round(pw0.cpu().numpy()) - e_w[0]))
