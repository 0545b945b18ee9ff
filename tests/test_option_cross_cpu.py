"""What tests/test_option_cross_gpu.py relies on, without a GPU: every shape of tests/option_cross.py selects what the GPU test says it
runs (the library's pure selection, mmg_plan_for, on the caps an MI355X gave: tests/golden/plans_mi355x.json), and the inputs reach
their branches on the CPU oracle -- flipped bits, stopped and running samples, frozen parameters that stay, and enough tie-free rows
for every conversation comparison, judged on the oracle's probabilities alone -- so that no GPU comparison passes vacuously."""
import numpy as np
import pytest

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import common, flipout_ref, generic_inst as gi, noise_ref as nr, option_cross as oc, training_controls_ref as tc
from tests.test_plan_cpu import switches  # noqa: F401  (a fixture: every selection switch of the environment unset)


def _plan(meta, shape, flags=0):
    return _lib.plan_for(_lib.make_config(**common.engine_kwargs(meta)), oc.caps_of(shape), flags)


# ------------------------------------------------------------------ what the shapes select
@pytest.mark.parametrize("case", oc.FLIP_CASES, ids=oc.flip_id)
def test_flip_cases_select_their_fast3_instantiation(case, switches):
    """host_select.h: plan_launches picks the FLIP instantiation from V (100 | run-time width) and merge_prep; a flipping handle never
    takes the one-launch step (game_ok), MMG_NO_MERGE leaves the backward without class roles and the forward without basehx roles."""
    V, exchange, sw = case
    meta = oc.c1_meta(V, exchange)
    switches({})
    plain = oc.plan_fields(_plan(meta, oc.flip_shape(case)))
    assert plain["family"] == 0 and plain["game_ok"] == int(V == 100 and exchange == "adaptive")
    switches({k: "1" for k in sw})
    f = oc.plan_fields(_plan(meta, oc.flip_shape(case), _lib.PLAN_FLIPS))
    assert f["family"] == 0 and f["game_ok"] == 0
    assert f["merge_prep"] == int("MMG_NO_MERGE_PREP" not in sw)
    merged = "MMG_NO_MERGE" not in sw
    assert (f["class_roles"], f["fwd_basehx"]) == ((oc.D, 1) if merged else (0, 0))
    assert meta["fixed_exchange"] == (exchange == "fixed") and meta["wv_dim"] == V and (meta["batch"], meta["max_exchange"]) == (oc.B, oc.T)
    assert case == oc.PHASED_ONLY or merged


def test_the_flip_cases_are_the_instantiations_the_flipout_module_does_not_run():
    """tests/test_flipout_gpu.py: V = 100, Adaptive, default switches -- the merged V = 100 instantiation alone."""
    from tests import test_flipout_gpu as tfl
    assert tfl.C1["wv_dim"] == 100 and not tfl.C1["fixed_exchange"]
    assert (100, "adaptive", ()) not in oc.FLIP_CASES
    assert {(c[0] == 100, "MMG_NO_MERGE_PREP" not in c[2]) for c in oc.FLIP_CASES if c[1] == "adaptive"} == {(True, True), (True, False), (False, True), (False, False)}
    assert {c[0] for c in oc.FLIP_CASES if c[1] == "fixed"} == {100, 200}


@pytest.mark.parametrize("option,case,mask", oc.FROZEN_CASES)
def test_frozen_cases_select_their_family_and_accept_the_mask(option, case, mask, switches):
    switches({k: "1" for k in oc.SWITCHES_OF.get((option, case), ())})
    meta = oc.option_meta(option, case)
    shape = "mc_continuous" if (option, case) == ("noise", "M") else "c1"
    flag, frozen = oc.PLAN_FLAG[option], tc.MASKS[mask]
    free = _plan(meta, shape, flag)
    text = _plan(meta, shape, flag | oc.frozen_flags(frozen))
    family = {("flip", "fast3"): 0, ("flip", "generic"): 3, ("variant", "A"): 3, ("noise", "G256"): 3, ("noise", "M"): 1}[option, case]
    assert oc.plan_fields(free)["family"] == family and oc.plan_fields(text)["family"] == family
    assert oc.plan_fields(text)["game_ok"] == 0
    tiles = lambda t: int(t.splitlines()[0].split("(gemm tiles ")[1].split(")")[0])
    if meta["use_binary"] or "receiver" in frozen:
        assert tiles(text) < tiles(free)                                # the frozen agents' jobs leave the table
    else:
        assert text == free                                             # continuous messages train the receiver alone: the sender's bit is a no-op
    if option == "noise":
        assert ("k_conversation_mc3_noise" if case == "M" else "k_conversation_noise") + " serves the conversation" in text
        assert nr.SCOPES[case] == ("k_conversation_mc3_noise" if case == "M" else "k_conversation_noise")


def test_corruption_sites_select_their_kernels(switches):
    switches({})
    assert oc.plan_fields(_plan(oc.corrupt_meta("fast3_wide"), "c1_wv200"))["family"] == 0 and oc.corrupt_meta("fast3_wide")["wv_dim"] == 200
    assert oc.plan_fields(_plan(oc.corrupt_meta("fast3_flip"), "c1", _lib.PLAN_FLIPS))["family"] == 0 and oc.corrupt_meta("fast3_flip")["wv_dim"] == 100
    m = oc.corrupt_meta("generic_512")
    assert gi.conv_threads(**gi.dims_of(m)) == 512 and oc.plan_fields(_plan(m, "c1"))["family"] == 3
    for site in oc.CORRUPT_SEEDS:
        mask = oc.corrupt_mask(oc.corrupt_meta(site)["rec_w_dim"])
        assert mask[0] == 1 and mask[1] == 0 and mask[-1] == int((mask.size - 1) % 3 == 0) and 0 < mask.sum() < mask.size


@pytest.mark.parametrize("V,n_classes", oc.WIDTH_CASES)
def test_width_edges_select_the_run_time_width_kernels(V, n_classes, switches):
    """layout.h: fast_wide_v takes every multiple of 4 from 4 to 512 but 100; the small agents hold at most 32 classes."""
    switches({})
    meta = oc.width_meta(V, n_classes)
    f = oc.plan_fields(_plan(meta, "c1_wv200"))
    assert f["family"] == 0 and f["game_ok"] == 0 and f["merge_prep"] == 1 and f["class_roles"] == n_classes
    assert V % 4 == 0 and V != 100 and 4 <= V <= 512 and n_classes <= 32


def test_width_edges_are_the_edges(switches):
    switches({})
    vs = sorted({v for v, _ in oc.WIDTH_CASES})
    assert vs[0] == 4 and vs[0] < 16                                    # below one 16-column tile
    assert 16 < 20 < 4 * 16                                             # tiles, but fewer than the four waves
    assert 104 == 100 + 4                                               # the first width past the V = 100 instantiation
    assert 508 == 512 - 4 and 508 % 16 == 12                            # the largest width whose last tile is partial
    assert {d for _, d in oc.WIDTH_CASES} == {2, 30, 32}
    # one step past either end leaves the family: V = 0 mod 4 only, at most 32 classes
    assert oc.plan_fields(_plan(oc.c1_meta(102), "c1_wv200"))["family"] != 0
    assert oc.plan_fields(_plan(oc.c1_meta(104, n_classes=33), "c1_wv200"))["family"] != 0


# ------------------------------------------------------------------ what the inputs reach on the oracle
def _flipped(bits, probs, u):
    return np.asarray(bits) != (np.asarray(u).reshape(np.asarray(probs).shape) < np.asarray(probs))


@pytest.mark.parametrize("V,exchange", sorted({c[:2] for c in oc.FLIP_CASES}))
def test_flip_oracles_reach_their_branches(V, exchange):
    want, u = oc.flip_conversation(V, exchange)
    m_z, m_w = flipout_ref.flip_masks(oc.SEED, 1, oc.T, oc.B, oc.W, oc.P_SEN, oc.P_REC)
    np.testing.assert_array_equal(_flipped(want["z"], want["pz"], u[0]), m_z != 0)
    np.testing.assert_array_equal(_flipped(want["w"], want["pw"], u[2]), m_w != 0)
    assert 0 < m_w.sum() < m_z.sum() < m_z.size
    assert oc.check_conversation(None, want, oc.sample_ties(u), "") >= 0.75
    us, packed = oc.flip_minibatch(V, exchange)
    n = int(packed["mb0.n_steps"])
    assert _flipped(packed["mb0.sen_feats"], packed["mb0.sen_probs"], us[0][:n]).any()
    assert _flipped(packed["mb0.rec_feats"], packed["mb0.rec_probs"], us[2][:n]).any()
    for key, uu in zip(("sen_probs", "s_probs", "rec_probs"), us):
        p = np.asarray(packed["mb0." + key])
        assert (np.abs(np.asarray(uu)[:n].reshape(p.shape) - p) >= 1e-4 - 1e-7).all(), key
    masks = np.asarray(packed["mb0.s_masks"]).reshape(n + 1, -1)
    if exchange == "adaptive":
        assert n == oc.T and 0 < masks[1].sum() < oc.B                  # after step 1: stopped samples and running ones
    else:
        assert n == oc.T


def test_flip_evaluation_oracle_keeps_its_rows():
    V = oc.FLIP_CASES[0][0]
    convs = [oc.flip_eval_conversation(V, c1) for c1 in (0, 1)]
    for c in convs:
        assert oc.check_conversation(None, c, oc.round_ties(oc.T, oc.B), "") >= 0.75
    assert (convs[0]["z"] != convs[1]["z"]).any()


@pytest.mark.parametrize("option,case,mask", oc.FROZEN_CASES)
def test_frozen_oracles_leave_the_frozen_parameters_alone(option, case, mask):
    meta, _, us = oc.option_ref(option, case)
    want, after = oc.frozen_oracle(option, case, mask)
    start = cpu_ref.fill_state_dicts({a: {k: v.shape for k, v in d.items()} for a, d in after.items()}, seed=meta["seed_weights"])
    trained = tc.trained_agents(meta)
    for a in tc.AGENTS:
        moved = False
        for k, v in start[a].items():
            same = np.array_equal(after[a][k], np.asarray(v, np.float32).reshape(after[a][k].shape))
            moved = moved or not same
            if a in tc.MASKS[mask] or a not in trained:
                assert same, (a, k)
        assert moved == (a in trained and a not in tc.MASKS[mask]), a
        assert ("mb0.gradnorm." + a in want) == (a in trained and a not in tc.MASKS[mask]), a
    if option == "flip":
        n = int(want["mb0.n_steps"])
        assert _flipped(want["mb0.sen_feats"], want["mb0.sen_probs"], us[0][:n]).any()
        masks = np.asarray(want["mb0.s_masks"]).reshape(n + 1, -1)
        assert 0 < masks[1].sum() < meta["batch"]
    if option == "noise":
        assert np.abs(nr.SIGMA_SEN * nr.noise_fields(0, 1, *nr.dims(meta))[0][0]).max() > 0.5


@pytest.mark.parametrize("site", sorted(oc.CORRUPT_SEEDS))
def test_corruption_oracles_keep_their_rows(site):
    meta = oc.corrupt_meta(site)
    mask = oc.corrupt_mask(meta["rec_w_dim"])
    if site == "fast3_flip":
        convs = [oc.flip_eval_conversation(100, c1, mask) for c1 in (0, 1)]
        assert (convs[0]["z"] != convs[1]["z"]).any()
    else:
        conv, res = oc.corrupt_oracle(site)
        convs = [conv]
        n = int(res["n_steps"])
        np.testing.assert_array_equal(np.stack([t.numpy() for t in res["sen_feats"]]), conv["z"][:n])      # eval_batch: the same conversation, cut short
        # the receiver read the inverted rounded probabilities at the masked bits
        assert (conv["z"][0][:, mask != 0] != np.round(conv["pz"][0][:, mask != 0])).all()
        assert (conv["z"][0][:, mask == 0] == np.round(conv["pz"][0][:, mask == 0])).all()
    for c in convs:
        assert oc.check_conversation(None, c, oc.round_ties(*c["s"].shape[:2]), "") >= 0.75


@pytest.mark.parametrize("V,n_classes", oc.WIDTH_CASES)
def test_width_oracles_have_dead_rows(V, n_classes):
    want, _ = oc.width_oracle(V, n_classes)
    masks = want["mb0.s_masks"][:, :, 0]
    assert int(want["mb0.n_steps"]) == oc.T and 0 < masks[1].sum() < masks.shape[1]
