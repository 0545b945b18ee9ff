"""mmg_eval_steps_profile / k_eval_profile (include/mmg.h, csrc/kernels_eval.h) without a GPU: the two entry points exist and
the accumulator's size is what the parsers lay out; the numpy restatement (tests/eval_profile_ref.py) keeps the invariants that
tie it to k_eval_reduce's numbers on the oracle's tapes, and those tapes reach what the GPU tests rely on (several output steps,
ranks that move between step 0 and the output step); model.eval_dev(profile=...) through its torch form on the oracle-backed
engine equals the sum of the restatement over the dev batches; commstats.summarise against brute-force passes over the
per-sample tape."""
import ctypes as C
import os

import numpy as np
import pytest

from multimodalgame_amd import _lib, commstats
from tests import common
from tests import eval_profile_ref as ref
from tests.test_eval_steps_cpu import CASES, case_meta, np_eval_reduce

INVARIANT_CASES = ["tiny_ragged", "tiny_all_stop", "tiny_never_stop", "tiny_T1", "tiny_fixed", "tiny_continuous", "c1_B64", "D130_B17"]
ORACLE_GPU_CASES = ["tiny_ragged", "tiny_never_stop", "tiny_W70"]       # the GPU compares these with the oracle's own conversation


def _profile(name):
    c, meta, target, tape = ref.oracle_case(name)
    p = ref.np_eval_profile(tape, target, c["top_k"], meta["fixed_exchange"], bool(meta["use_binary"]))
    return c, meta, target, tape, p


def test_library_exports_profile_entry_points():
    lib = _lib.load()
    assert lib.mmg_eval_steps_profile is not None and lib.mmg_eval_profile_count is not None     # (AttributeError: the symbol is missing)
    assert "mmg_eval_steps_profile" in _lib.SYMBOLS and "mmg_eval_profile_count" in _lib.SYMBOLS
    header = open(os.path.join(os.path.dirname(common.GOLDEN_DIR), "..", "include", "mmg.h")).read()
    assert "int64_t mmg_eval_profile_count(const mmg_config* cfg);" in header
    assert "int mmg_eval_steps_profile(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k," in header
    assert "int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof, void* stream);" in header
    assert "#define MMG_VERSION 3" in header and lib.mmg_version() == 3
    assert _lib.EVAL_PROF_HEAD == ref.HEAD == commstats.HEAD == 4


def test_profile_count_matches_both_parsers():
    """mmg_eval_profile_count = 4 + 2 D T + 2 D + 2 T D W for three configs, and both parsers -- the tests' and the product's --
    cut a flat array of that size into the same named blocks."""
    lib = _lib.load()
    for name in ("tiny_ragged", "c1_B64", "tiny_W70"):
        c = ref.PROFILE_CASES[name]
        meta = case_meta(c)
        cfg = _lib.make_config(**common.engine_kwargs(meta))
        D, T, W = c["n_classes"], meta["max_exchange"], meta["rec_w_dim"]
        n = int(lib.mmg_eval_profile_count(C.byref(cfg)))
        assert n == 4 + 2 * D * T + 2 * D + 2 * T * D * W == ref.profile_count(D, T, W) == commstats.profile_count(D, T, W)
        flat = np.arange(n, dtype=np.int64)
        mine, theirs = ref.parse(flat, D, T, W), commstats.parse_profile(flat, D, T, W)
        ref.assert_profile_equal(theirs, mine, name)
        assert mine["steps"].shape == (D, T) and mine["rank"].shape == (T, D) and mine["msg_rec"].shape == (T, D, W)
        assert mine["steps"][0, 0] == 4 and mine["rank"][0, 0] == 4 + D * T and mine["class_hits"][0] == 4 + 2 * D * T
        assert mine["class_ranksum"][0] == 4 + 2 * D * T + D and mine["msg_sen"][0, 0, 0] == 4 + 2 * D * T + 2 * D
        assert mine["msg_rec"][-1, -1, -1] == n - 1
    bad = _lib.make_config(**common.engine_kwargs(case_meta(dict(CASES["tiny_ragged"], n_classes=0))))
    assert lib.mmg_eval_profile_count(C.byref(bad)) < 0
    with pytest.raises(ValueError):
        commstats.parse_profile(np.zeros(5, np.int64), 3, 4, 6)


@pytest.mark.parametrize("name", INVARIANT_CASES)
def test_restatement_invariants_on_the_oracle_tape(name):
    c, meta, target, tape, p = _profile(name)
    r = np_eval_reduce(tape, target, c["top_k"], meta["fixed_exchange"])
    D, T, B = c["n_classes"], meta["max_exchange"], c["batch"]
    k = min(c["top_k"], D)
    assert p["head"].tolist() == [1, B, 0, 0]
    assert p["steps"].sum() == p["head"][1]
    assert (p["rank"].sum(1) == p["head"][1]).all()
    assert p["rank"][T - 1, :k].sum() == p["class_hits"].sum() == r["hits"]
    np.testing.assert_array_equal(p["steps"].sum(1), r["conf"].sum(1))
    live = p["steps"][:, ::-1].cumsum(1)[:, ::-1].T                           # [T, D]: sum_{l >= t} steps[c, l]
    for m in ("msg_sen", "msg_rec"):
        assert (p[m] <= live[:, :, None]).all() and (p[m] >= 0).all()
    assert p["class_ranksum"].sum() == p["ranks"][T - 1].sum() == (np.arange(D) * p["rank"][T - 1]).sum()
    if name in ("tiny_fixed", "tiny_never_stop"):
        assert p["steps"][:, :T - 1].sum() == 0 and p["steps"][:, T - 1].sum() == B
    if name == "tiny_continuous":
        assert not p["msg_sen"].any() and not p["msg_rec"].any()
        assert np.abs(tape["z"]).sum() > 0                                    # (the messages themselves are not zero)
    else:
        assert p["msg_sen"][0].sum() > 0 and p["msg_rec"][0].sum() > 0
    if name == "tiny_all_stop":
        assert (p["rank"] == p["rank"][0]).all() and p["steps"][:, 0].sum() == B
        assert not p["msg_sen"][1:].any() and not p["msg_rec"][1:].any()      # only step 0 is live


def test_cases_reach_what_the_gpu_tests_rely_on():
    """A profile that is constant over the steps cannot pass: the oracle's conversations spread their output steps and move the
    rank of the target between step 0 and the output step."""
    c, meta, target, tape, p = _profile("c1_B64")
    T = meta["max_exchange"]
    assert p["steps"].sum(0).tolist() == [0, 1, 41, 21, 1] + [0] * (T - 5)
    assert int((p["steps"].sum(1) > 0).sum()) == 27
    assert int((p["ranks"][0] != p["ranks"][T - 1]).sum()) == 53
    c, meta, target, tape, p = _profile("D130_B17")
    assert int((p["ranks"][0] != p["ranks"][meta["max_exchange"] - 1]).sum()) == 13
    for name in ("tiny_ragged", "tiny_topk_ge_D", "tiny_W70"):
        c, meta, target, tape, p = _profile(name)
        assert p["steps"].sum(0).tolist() == [0, 4, 1, 0] and int((p["steps"].sum(1) > 0).sum()) == 2, name
    c, meta, target, tape, p = _profile("tiny_W70")
    assert int((p["ranks"][0] != p["ranks"][3]).sum()) == 1
    assert tape["z"].shape[2] == 70 and p["msg_sen"][0].sum() > 150 and p["steps"].sum() * 70 == 350


@pytest.mark.parametrize("name", ORACLE_GPU_CASES)
def test_oracle_compared_cases_are_far_from_every_tie(name):
    """The three cases the GPU compares with the ORACLE's conversation: the target's logit is far from every other logit at
    every step that forms a rank, and every stop probability is more than 1e-4 away from 0.5 (two correct fp32 implementations
    agree to ~1e-5), so steps, rank and class_hits cannot differ between the oracle and a correct kernel."""
    c, meta, target, tape, p = _profile(name)
    gap = ref.target_gap(tape, target, p)
    margin = float(np.abs(ref.oracle_stop_probs(name) - 0.5).min())
    print(name, "logit gap %.3e stop margin %.3e" % (gap, margin))
    assert gap > 8e-3 and margin > 1e-4


def test_eval_dev_profile_through_the_torch_form(tmp_path, monkeypatch):
    """model.eval_dev(profile=...) on the oracle-backed engine (no eval_steps: the torch form) over two dev batches, the second
    one short: the sum of the restatement over the batches; return value and confusion matrix file as without a profile."""
    from multimodalgame_amd import flags as _flags, game as _game
    from tests import oracle_engine
    from tests.test_eval_steps_cpu import oracle_tape
    monkeypatch.setattr(_game, "Engine", oracle_engine.OracleEngine)
    try:
        game, run, batches, desc, meta, z = ref.g8_game(tmp_path, "cpu", monkeypatch)
        prof = {"stale": 1}
        acc_p, extra_p = run("with.txt", profile=prof)
        acc, extra = run("without.txt")
        assert acc_p == acc and extra_p == extra
        assert open(str(tmp_path / "with.txt")).read() == open(str(tmp_path / "without.txt")).read()
        want = ref.add_profiles([ref.np_eval_profile(oracle_tape(dict(meta, batch=len(x)), x, t, desc, float(z["s_bias"])), t, 2, False)
                                 for x, t in batches])
        assert "stale" not in prof and prof["batches"] == 2 and prof["samples"] == sum(len(x) for x, _ in batches)
        ref.assert_profile_equal(prof, want, "eval_dev")
        assert len(batches[1][0]) < len(batches[0][0]) and want["head"].tolist() == [2, prof["samples"], 0, 0]
        assert acc == pytest.approx(float(z["accuracy"]), abs=1e-12)
    finally:
        _flags.FLAGS.Reset()


def test_tape_profile_equals_the_restatement():
    """commstats.tape_profile (the torch form's per-batch reduction) against the tests' restatement, with two targets outside
    [0, D) and on continuous messages."""
    for name in ("c1_B64", "tiny_continuous", "tiny_fixed"):
        c, meta, target, tape, _ = _profile(name)
        target = target.copy()
        target[1], target[3] = c["n_classes"], -1
        fixed, binary = meta["fixed_exchange"], bool(meta["use_binary"])
        want = ref.np_eval_profile(tape, target, c["top_k"], fixed, binary)
        got = commstats.parse_profile(commstats.tape_profile(tape["mask"], tape["z"], tape["w"], tape["y"], target, c["top_k"], fixed, binary),
                                      c["n_classes"], meta["max_exchange"], tape["z"].shape[2])
        ref.assert_profile_equal(got, want, name)
        assert got["invalid"] == 2 and got["samples"] == c["batch"] - 2


def test_summarise_against_brute_force():
    c, meta, target, tape, p = _profile("c1_B64")
    D, T, B, W, k = c["n_classes"], meta["max_exchange"], c["batch"], tape["z"].shape[2], c["top_k"]
    r = np_eval_reduce(tape, target, k, False)
    s = commstats.summarise(p, k)
    ranks, tsel = p["ranks"], p["tsel"]
    assert s["acc_by_step"][T - 1] == pytest.approx(r["hits"] / float(B), abs=1e-15)
    np.testing.assert_allclose(s["acc_by_step"], (ranks < k).mean(1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(commstats.summarise(p, 1)["acc_by_step"], (ranks < 1).mean(1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(s["mrr_by_step"], (1.0 / (ranks + 1)).mean(1), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(s["step_counts"], np.bincount(tsel, minlength=T))
    assert s["mean_steps"] == pytest.approx((tsel + 1).mean(), abs=1e-14)
    assert abs(s["mrr_by_step"][0] - s["mrr_by_step"][T - 1]) > 1e-3, "the case should move the ranks over the steps"
    for cls in range(D):
        sel = target == cls
        if not sel.any():
            assert np.isnan(s["class_acc"][cls]) and np.isnan(s["class_mean_rank"][cls]) and np.isnan(s["class_steps"][cls])
            assert np.isnan(s["code_sen"][:, cls]).all()
            continue
        assert s["class_count"][cls] == sel.sum()
        assert s["class_acc"][cls] == pytest.approx(r["hit"][sel].mean(), abs=1e-15)
        assert s["class_mean_rank"][cls] == pytest.approx(ranks[T - 1, sel].mean(), abs=1e-13)
        assert s["class_steps"][cls] == pytest.approx((tsel[sel] + 1).mean(), abs=1e-13)
    assert np.isnan(s["class_acc"]).sum() == D - 27
    # code means and I(bit; class) from the per-sample (bit, class) pairs of the live samples
    for key, msg in (("sen", tape["z"]), ("rec", tape["w"])):
        for t in range(T):
            live = tsel >= t
            if not live.any():
                assert np.isnan(s["mi_" + key][t]).all() and np.isnan(s["code_" + key][t]).all()
                continue
            for cls in np.unique(target[live]):
                np.testing.assert_allclose(s["code_" + key][t, cls], msg[t, live & (target == cls)].astype(np.float64).mean(0), rtol=0, atol=1e-13)
            for j in range(W):
                joint = np.zeros((2, D))
                np.add.at(joint, (msg[t, live, j].astype(np.int64), target[live]), 1.0)
                joint /= joint.sum()
                pb, pc = joint.sum(1, keepdims=True), joint.sum(0, keepdims=True)
                nz = joint > 0
                mi = float((joint[nz] * np.log2(joint[nz] / (pb * pc)[nz])).sum())
                assert s["mi_" + key][t, j] == pytest.approx(mi, abs=1e-12), (key, t, j)
    assert np.isnan(s["mi_sen"][5:]).all() and not np.isnan(s["mi_sen"][:5]).any()       # output steps 1 .. 4: nothing is live at t >= 5
    assert s["mi_sen"][:5].max() > 0.1
    empty = commstats.summarise(commstats.parse_profile(np.zeros(commstats.profile_count(3, 4, 6), np.int64), 3, 4, 6), 2)
    assert np.isnan(empty["acc_by_step"]).all() and np.isnan(empty["mi_rec"]).all() and np.isnan(empty["mean_steps"])
