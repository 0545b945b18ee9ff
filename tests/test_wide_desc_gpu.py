"""Wide class descriptions on the GPU: -wv_dim 200 / 300 / 512 (and 50, the GloVe width that is not a multiple of 4).

Every case runs through the C-ABI (common.hip_train_case) or through Game and is gated by the project's own parity gate
(common.assert_parity): class logits, probabilities, rewards, baseline scores and the six losses within 1e-4
absolute of the CPU oracle, sampled bits / masks / step counts / hits exact, gradients and post-update parameters within
1e-4 + 1e-3 |v| -- the tolerances tests/test_hip_parity.py applies at V = 100, unchanged (a V-deep fp32 dot product of O(0.1)
terms carries ~V * 6e-8 * |term|^2 of rounding, 1e-6 at V = 512: two orders below the gate, so no wider bound is claimed).
The autograd cases keep the tolerances of tests/test_autograd_gpu.py / test_module_autograd_gpu.py (they are those tests'
bodies, run at V = 300).

Which kernels serve which V (DESIGN.md "Shapes"): the small agents (H 256, W 32, R 64, D <= 32, T <= 16) with V a multiple of 4
run the register-resident conversation and reverse kernels at any V <= 512 (profiling scopes k_conversation_wv / k_bwd_conv_wv;
V = 100 keeps k_game / k_conversation / k_bwd_conv); the many-class, sample-tile and wide-receiver kernels are not selected
beyond their audited widths and such shapes run the per-sample kernels (scopes k_conversation / k_bwd_conv)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import common
from tests import test_autograd_gpu as ta
from tests import test_hip_configs as thc
from tests import test_hip_dp as tdp
from tests import test_module_autograd_gpu as tma
from tests.test_hip_parity import ATOL, FUSED_KEEP, RTOL, _skip_keys

pytestmark = pytest.mark.gpu

C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, learning_rate=1e-4, entropy_rec=0.01, entropy_sen=0.01,
          entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
          baseline_hid_dim=500, top_k_train=6)
FLAVOURS = {
    "adaptive": dict(),
    "fixed": dict(fixed_exchange=True),
    "continuous": dict(use_binary=False, fixed_exchange=True, max_exchange=4, entropy_rec=None, entropy_sen=None, entropy_s=None),
}
GENERIC_SCOPES = ("k_conversation", "k_bwd_conv")
WIDE_SCOPES = ("k_conversation_wv", "k_bwd_conv_wv")
_CACHE = {}


def _c1_meta(V, flavour, batch=32, n_mb=2):
    kw = dict(C1, wv_dim=V, batch_size=batch)
    kw.update(FLAVOURS[flavour])
    return thc._meta(kw, 30, batch, n_mb, seeds=(41, 42 + V, 43))


def _oracle(meta, key):
    if key not in _CACHE:
        flips = []
        _CACHE[key] = (common.oracle_train_case(None, meta, flips=flips), flips)
    return _CACHE[key]


def _pick(d):
    return {k: d[k] for k in (d.keys() if hasattr(d, "keys") else d.files) if any(t in k for t in FUSED_KEEP)}


# mmg_exchange_forward's run_all_steps: 1 = exchange() (every row), 0 = early exit, 2 = the fused training step, 3 = log tape
MODES = {"run_all_1": dict(), "run_all_0": dict(early_exit=True), "fused_2": dict(fused=True), "log_tape_3": dict(log_tape=True)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("V", [200, 300, 512])
def test_config1_agents_vs_oracle(V, flavour, mode):
    """Config 1's agents, two minibatches (the second starts from the updated parameters), early stopping on in the Adaptive
    flavour (dead rows exist: asserted).  The phased calls with every run_all_steps mode and the fused mmg_train_step."""
    meta = _c1_meta(V, flavour)
    want, flips = _oracle(meta, (V, flavour))
    if flavour == "adaptive":
        masks = want["mb0.s_masks"][:, :, 0]
        assert 0 < masks[1].sum() < masks.shape[1]
    got, eng = common.hip_train_case(None, meta, **MODES[mode])
    if mode == "run_all_1":
        common.assert_parity(got, want, flips, eng, "wide%d-%s-%s" % (V, flavour, mode), skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    else:
        common.assert_parity(_pick(got), _pick(want), flips, eng, "wide%d-%s-%s" % (V, flavour, mode), skip=_skip_keys(meta),
                             atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["g10_wide_desc_adaptive", "g10_wide_desc_fixed", "g10_wide_desc_continuous", "g10_wide_desc_tiny50"])
def test_golden_wide_cases(name, fused):
    """The reference's own run at V = 300 (and tiny agents at V = 50): forward quantities against the fixture, everything
    against this host's oracle."""
    z, meta = common.load_golden(name)
    got, eng = common.hip_train_case(name, meta, fused=fused)
    flips = []
    want = common.oracle_train_case(name, meta, flips=flips)
    if fused:
        got, want, z = _pick(got), _pick(want), _pick(z)
    common.assert_parity(got, want, flips, eng, name + ("/fused" if fused else ""), skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    gold = {k: v for k, v in (z.items() if isinstance(z, dict) else ((k, z[k]) for k in z.files)) if not common.is_grad_key(k) and k != "meta"}
    pg = common.compare_packed(got, gold, atol=ATOL, rtol=RTOL, skip=_skip_keys(meta), shift_invariant=True, label=name + "/golden")
    assert not pg, "forward mismatch vs golden (atol 1e-4):\n" + "\n".join(pg[:25])


@pytest.mark.parametrize("V", [200, 300, 512])
def test_eval_pass_vs_oracle(V):
    """Evaluation mode (rounded bits, cumulative stop product) at config 1's agents: bits exact, logits / log-probabilities
    within 1e-4, identical top-k sets wherever the k-th and (k+1)-th differ by more than the tolerance."""
    meta = _c1_meta(V, "adaptive", batch=50)
    fl = common.flags_from_meta(meta)
    eng = common.make_engine(meta)
    eng.params["receiver"]["s.bias"].fill_(1.2)
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    with torch.no_grad():
        models["receiver"].s.bias.fill_(1.2)
    x, target, desc = cpu_ref.synthetic_batch(50, 30, 512, V, seed=meta["seed_data"])
    res = cpu_ref.eval_batch(models, torch.from_numpy(x), torch.from_numpy(target), torch.from_numpy(desc), fl)
    dev = eng.device
    eng.set_profiling(True)
    eng.forward(torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev), train=False, run_all=True)
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    assert "k_conversation_wv" in names and "k_conversation" not in names, names
    n = res["n_steps"]
    tp = {k: v.cpu().numpy() for k, v in eng.tape.items() if k in ("mask", "s", "z", "w", "y", "dist", "hit")}
    np.testing.assert_array_equal(tp["s"][:n], torch.stack(res["s_feats"]).numpy())
    np.testing.assert_array_equal(tp["z"][:n], torch.stack(res["sen_feats"]).numpy())
    np.testing.assert_array_equal(tp["w"][:n], torch.stack(res["rec_feats"]).numpy())
    np.testing.assert_array_equal(tp["mask"][:n], torch.stack(res["s_masks"]).numpy()[:n])
    np.testing.assert_allclose(tp["y"][:n], torch.stack(res["y"]).numpy(), atol=ATOL)
    want_dist = res["dist"].numpy()
    np.testing.assert_allclose(tp["dist"], want_dist, atol=ATOL)
    assert int(tp["hit"].sum()) == int(res["hits"])
    k = res["top_k_ind"].shape[1]
    order = np.argsort(-want_dist, axis=1, kind="stable")
    gap = np.take_along_axis(want_dist, order[:, k - 1:k], 1) - np.take_along_axis(want_dist, order[:, k:k + 1], 1)
    got_top = np.argsort(-tp["dist"], axis=1, kind="stable")[:, :k]
    for b in np.nonzero(gap.reshape(-1) > ATOL)[0]:
        assert set(got_top[b].tolist()) == set(res["top_k_ind"].numpy()[b].tolist()), b


ODD = dict(C1, img_h_dim=100, rec_w_dim=50, sender_out_dim=50, rec_hidden=128, max_exchange=3, baseline_hid_dim=90)


@pytest.mark.parametrize("V", [50, 300, 512])
@pytest.mark.parametrize("fused", [False, True])
def test_unaligned_dims_generic_path(V, fused):
    """The reference's default agent sizes (H 100, W 50, R 128: nothing a multiple of 16) on the per-sample kernels."""
    meta = thc._meta(dict(ODD, wv_dim=V, batch_size=7), 7, 7, 2, seeds=(51, 52 + V, 53))
    want, flips = _oracle(meta, ("odd", V))
    got, eng = common.hip_train_case(None, meta, fused=fused)
    if fused:
        got, want = _pick(got), _pick(want)
    common.assert_parity(got, want, flips, eng, "odd%d" % V, skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    names = _names(eng, meta)
    assert set(names) & set(GENERIC_SCOPES) and not set(names) & set(WIDE_SCOPES), names


@pytest.mark.parametrize("fused", [False, True])
def test_generic_kernels_at_the_cap(fused, monkeypatch):
    """MMG_NO_FAST=1 at config 1's agents and V = 512: the per-sample kernels (their LDS plans grow with V) at the cap, parity
    against the oracle, not only the path."""
    monkeypatch.setenv("MMG_NO_FAST", "1")
    meta = _c1_meta(512, "adaptive")
    want, flips = _oracle(meta, (512, "adaptive"))
    got, eng = common.hip_train_case(None, meta, fused=fused)
    if fused:
        got, want = _pick(got), _pick(want)
    common.assert_parity(got, want, flips, eng, "generic512" + ("/fused" if fused else ""), skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    names = _names(eng, meta)
    assert set(GENERIC_SCOPES) <= set(names) and not set(names) & set(WIDE_SCOPES) and "k_conv_tile" not in names, names


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("V", [100, 300])
def test_small_agents_with_another_rec_hidden_stay_off_the_register_resident_kernels(V, fused):
    """H 256, W 32, D 30 with rec_hidden 128: every register-resident kernel is instantiated for R = 64 only, so this shape
    runs the per-sample kernels at V = 100 (as before) and at V = 300 -- never the k_game / _wv launches.  Parity against the oracle on the path that is selected."""
    meta = thc._meta(dict(C1, wv_dim=V, rec_hidden=128, batch_size=32), 30, 32, 2, seeds=(81, 82 + V, 83))
    want, flips = _oracle(meta, ("r128", V))
    got, eng = common.hip_train_case(None, meta, fused=fused)
    if fused:
        got, want = _pick(got), _pick(want)
    common.assert_parity(got, want, flips, eng, "r128-v%d" % V + ("/fused" if fused else ""), skip=_skip_keys(meta), atol=ATOL, rtol=RTOL)
    names = _names(eng, meta)
    assert "k_game" not in names and not set(names) & set(WIDE_SCOPES), names
    # the per-sample kernels at both widths (k_prep, k_stats and k_dC as launches of their own: the register-resident chain
    # carries them as roles of its two launches)
    assert set(GENERIC_SCOPES) <= set(names) and {"k_prep+h_x", "k_stats", "k_dC"} <= set(names), names


def test_many_classes_continuous_at_v300():
    """D = 1000, continuous messages, V = 300: the many-class kernels keep V = 100; correct on the path that is selected."""
    meta = thc._meta(dict(thc.C5, wv_dim=300, batch_size=24, max_exchange=4), 1000, 24, 2, seeds=(61, 62, 63))
    thc._compare(meta, skip=_skip_keys(meta), label="wide300-c5")
    names = _names(common.make_engine(meta), meta)
    assert "k_conversation_mc" not in names, names


@pytest.mark.parametrize("R", [64, 256])
def test_config4_shape_at_v300(R):
    """W 256, H 1024 (config 4's agents) at V = 300, rec_hidden 64 and 256: the sample-tile / wide-receiver kernels are not
    selected beyond V = 256; the losses are gated against the float64 oracle as in tests/test_hip_configs.py (label config4)."""
    meta = thc._meta(dict(thc.C4, wv_dim=300, rec_hidden=R, batch_size=16, max_exchange=4), 30, 16, 2, seeds=(71, 72, 73))
    thc._compare(meta, skip=("y2.bias",), label="config4-wide300-r%d" % R)
    names = _names(common.make_engine(meta), meta)
    assert "k_conv_tile" not in names and "k_conv_rc" not in names and "k_conv_persist" not in names, names


def _names(eng, meta, i=0):
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, i, None)
    dev = eng.device
    shapes = {a: {k: tuple(v.shape) for k, v in d.items()} for a, d in eng.params.items()}
    eng.load_state_dicts(cpu_ref.fill_state_dicts(shapes, seed=meta["seed_weights"]))
    eng.set_profiling(True)
    eng.train_step(torch.from_numpy(x).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(desc).to(dev), seed=1)
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
@pytest.mark.parametrize("V", [200, 300])
def test_path_wide_v_runs_register_resident_kernels(V, flavour):
    """A config-1-agents training minibatch at V = 200 / 300 holds no launch of the per-sample generic kernels."""
    meta = _c1_meta(V, flavour, batch=64, n_mb=1)
    names = _names(common.make_engine(meta), meta)
    assert not set(names) & set(GENERIC_SCOPES), names
    assert set(WIDE_SCOPES) <= set(names) and "k_wgrad" in names, names
    assert "k_conv_tile" not in names and "k_bwd_tile" not in names and "k_game" not in names, names


def test_path_v100_is_unchanged():
    meta = _c1_meta(100, "adaptive", batch=64, n_mb=1)
    assert _names(common.make_engine(meta), meta) == ["k_game", "k_wgrad"]


def test_path_generic_fallback_switch(monkeypatch):
    """MMG_NO_FAST=1 (the switch the timings of the generic path at V = 300 use) selects the per-sample kernels."""
    monkeypatch.setenv("MMG_NO_FAST", "1")
    meta = _c1_meta(300, "adaptive", batch=64, n_mb=1)
    names = _names(common.make_engine(meta), meta)
    assert set(GENERIC_SCOPES) <= set(names) and not set(names) & set(WIDE_SCOPES), names


def test_create_refuses_beyond_the_cap():
    from multimodalgame_amd.engine import Engine
    meta = _c1_meta(516, "adaptive")
    with pytest.raises(Exception, match="wv_dim must be <= 512"):
        Engine(**common.engine_kwargs(meta))


# ------------------------------------------------------------------ Game
def test_game_train_step_matches_engine_and_oracle():
    """Game.train_step at V = 300 (config 1's agents): the engine it builds takes the steps hip_train_case takes."""
    meta = _c1_meta(300, "adaptive")
    want, flips = _oracle(meta, (300, "adaptive"))
    game, eng = ta._game(meta)
    assert eng.cfg.wv_dim == 300
    for i in range(meta["n_minibatches"]):
        _, _, _, args = ta._inputs(meta, i)
        game.train_step(args["data"], args["target"], args["desc"], uniforms=args["uniforms"])
    torch.cuda.synchronize()
    # the oracle's packed parameters after the last minibatch are strided samples (cpu_ref.pack_train): the same samples here
    last = "mb%d.p." % (meta["n_minibatches"] - 1)
    got, ref = {a: {} for a in ta.AGENTS}, {a: {} for a in ta.AGENTS}
    for a in ta.AGENTS:
        for k, v in eng.params[a].items():
            if a == "receiver" and k == "y2.bias":
                continue                                   # (common.compare_packed: its exact gradient is zero)
            flat = v.detach().cpu().reshape(-1)
            got[a][k] = flat[::max(1, flat.numel() // 512)]
            ref[a][k] = torch.from_numpy(np.asarray(want[last + "%s.%s.sample" % (a, k)]))
    assert tuple(got["receiver"]["w_d.weight"].shape) == tuple(ref["receiver"]["w_d.weight"].shape)
    ta._assert_close(got, ref, "game-wide300", atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------ autograd
def test_exchange_vjp_reference_block_at_v300():
    ta.test_reference_block_gives_the_engine_gradients("g10_wide_desc_adaptive")


@pytest.mark.parametrize("family", ["fast", "continuous", "odd"])
def test_exchange_vjp_random_functional_at_v300(family, monkeypatch):
    kw = {"fast": dict(ta.C1, batch_size=16, wv_dim=300),
          "continuous": dict(ta.C1, batch_size=16, wv_dim=300, use_binary=False, fixed_exchange=True, max_exchange=4,
                             entropy_rec=None, entropy_sen=None, entropy_s=None),
          "odd": dict(ta.C1, batch_size=5, img_h_dim=100, rec_w_dim=50, sender_out_dim=50, rec_hidden=128, max_exchange=3,
                      fixed_exchange=True, wv_dim=300)}[family]
    batch = kw["batch_size"]
    monkeypatch.setitem(ta.FAMILIES, "wide300_" + family, (kw, 7 if family == "odd" else 30, batch))
    ta.test_vjp_of_a_random_functional_matches_float64("wide300_" + family)


@pytest.mark.parametrize("case", ["adaptive", "continuous_wired"])
def test_module_vjps_at_v300(case, monkeypatch):
    kw, n_classes, batch, T, wire = tma.CASES["c1_adaptive" if case == "adaptive" else "continuous_wired"]
    monkeypatch.setitem(tma.CASES, "wide300_" + case, (dict(kw, wv_dim=300), n_classes, batch, T, wire))
    tma.test_module_loop_functional_matches_float64("wide300_" + case)


# ------------------------------------------------------------------ data parallel, command line
@pytest.mark.parametrize("philox", [False, True])
def test_two_ranks_on_one_gpu_at_v300(philox, tmp_path):
    tdp.test_two_ranks_on_one_gpu_equal_single_process("g10_wide_desc_adaptive", philox, tmp_path)


def test_command_line_runs_at_wv_dim_300(tmp_path):
    from multimodalgame_amd import flags, model
    from tests.test_cli_gpu import _argv
    tmp = str(tmp_path)
    argv = _argv(tmp, "wide", ["-max_steps", "21"])
    argv[argv.index("-wv_dim") + 1] = "300"
    flags.define_flags(); flags.FLAGS.Reset()
    try:
        model.main(argv)
    finally:
        flags.FLAGS.Reset()
    assert os.path.exists(os.path.join(tmp, "data", "glove.synthetic.300d.txt"))
    log = open(os.path.join(tmp, "logs", "wide.log")).read()
    for pat in (r"Epoch: 0 Step: 20 Batch: 20 Training Accuracy: ", r"Development Accuracy: ", r"Checkpointing\."):
        assert re.search(pat, log), pat
    ck = torch.load(os.path.join(tmp, "logs", "wide.pt"), weights_only=False)
    assert tuple(ck["models"]["receiver"]["w_d.weight"].shape) == (64, 300)
    assert tuple(ck["models"]["receiver"]["y1.weight"].shape) == (64, 364)
