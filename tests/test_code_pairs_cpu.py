"""The pairwise code analysis without a GPU (include/mmg.h: mmg_eval_steps_codes, mmg_code_pair_hist; commstats.py): the four
symbols are declared, exported and bound and the size queries are what the parsers lay out; commstats.pack_codes on the oracle's
tapes (bit order, dead steps, padding); commstats.pair_hist_np against the brute-force loops of tests/pairs_ref.py; the edge-pair
conditions the GPU tests rest on, for the very seeds and shapes they use; commstats.topsim against scipy on the expanded pairs and
against brute-force counts; model.eval_dev(topsim=...) through its torch form on the oracle-backed engine."""
import ctypes as C
import os

import numpy as np
import pytest

from multimodalgame_amd import _lib, commstats
from tests import common
from tests import eval_profile_ref as ref
from tests import pairs_ref as pr
from tests.test_eval_steps_cpu import CASES, case_meta


def test_library_exports_the_entry_points():
    lib = _lib.load()
    for name in ("mmg_eval_code_words", "mmg_eval_steps_codes", "mmg_code_pair_hist_count", "mmg_code_pair_hist"):
        assert getattr(lib, name) is not None and name in _lib.SYMBOLS              # (AttributeError: the symbol is missing)
        assert getattr(lib, name).argtypes is not None, name
    header = open(os.path.join(os.path.dirname(common.GOLDEN_DIR), "..", "include", "mmg.h")).read()
    assert "int64_t mmg_eval_code_words(const mmg_config* cfg);" in header
    assert "int mmg_eval_steps_codes(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k," in header
    assert "uint32_t* d_codes, int32_t* d_meta, int64_t row0, int64_t cap_rows, void* stream);" in header
    assert "int64_t mmg_code_pair_hist_count(int n_sel_steps, int w_dim, int n_bins);" in header
    assert "int mmg_code_pair_hist(const uint32_t* d_codes, const int32_t* d_meta, int64_t n_rows, int T, int W," in header
    assert "binary_vectors.py" in header.split("mmg_eval_code_words")[0][-3000:]
    assert "#define MMG_VERSION 3" in header and lib.mmg_version() == 3
    assert _lib.PAIR_HIST_HEAD == commstats.PAIR_HEAD == 4 and _lib.EVAL_CODE_BITS == commstats.CODE_BITS == 32
    assert (_lib.EVAL_CODE_AGENTS, _lib.EVAL_CODE_META, _lib.EVAL_CODE_SENDER, _lib.EVAL_CODE_RECEIVER) == (2, 2, 0, 1)


def test_size_queries():
    lib = _lib.load()
    for name in ("tiny_ragged", "c1_B64", "tiny_W70"):
        c = ref.PROFILE_CASES[name]
        meta = case_meta(c)
        cfg = _lib.make_config(**common.engine_kwargs(meta))
        T, W = meta["max_exchange"], meta["rec_w_dim"]
        assert int(lib.mmg_eval_code_words(C.byref(cfg))) == 2 * T * ((W + 31) // 32) == commstats.code_words(T, W)
    assert commstats.code_words(10, 32) == 20 and commstats.code_words(4, 70) == 24 and _lib.code_wp(70) == 3 and _lib.code_wp(64) == 2
    bad = _lib.make_config(**common.engine_kwargs(case_meta(dict(CASES["tiny_ragged"], n_classes=0))))
    assert lib.mmg_eval_code_words(C.byref(bad)) < 0
    cont = _lib.make_config(**common.engine_kwargs(case_meta(CASES["tiny_continuous"])))
    assert lib.mmg_eval_code_words(C.byref(cont)) < 0 and b"continuous" in lib.mmg_last_error()
    for steps, W, K in ((1, 6, 16), (10, 32, 64), (10, 256, 64), (3, 70, 1), (64, 256, 511)):
        assert int(lib.mmg_code_pair_hist_count(steps, W, K)) == 4 + 2 * (steps * W + 1) * K == commstats.pair_hist_count(steps, W, K)
    assert int(lib.mmg_code_pair_hist_count(10, 32, 64)) == 41092
    for steps, W, K in ((0, 6, 16), (1, 0, 16), (1, 6, 0), (1, 6, 1025), (64, 256, 512), (-1, 6, 16)):
        assert lib.mmg_code_pair_hist_count(steps, W, K) < 0, (steps, W, K)         # (64 * 256 + 1) * 2 * 512 > 2^24
        assert lib.mmg_last_error().startswith(b"mmg_code_pair_hist_count")
    flat = np.arange(commstats.pair_hist_count(2, 6, 4), dtype=np.int64)
    p = commstats.parse_pair_hist(flat, 2, 6, 4)
    assert p["hist"].shape == (2, 13, 4) and p["hist"][0, 0, 0] == 4 and p["hist"][1, 0, 0] == 4 + 13 * 4 and p["hist"][1, 12, 3] == flat.size - 1
    assert (p["used"], p["skipped"], p["pairs"]) == (0, 1, 2)
    with pytest.raises(ValueError):
        commstats.parse_pair_hist(flat[:-1], 2, 6, 4)


@pytest.mark.parametrize("name", ["tiny_ragged", "tiny_fixed", "tiny_W70", "c1_B64"])
def test_pack_codes_on_the_oracle_tape(name):
    """Bit (j & 31) of word (j >> 5) is message bit j; steps behind the output step and the padding bits are zero; meta holds the
    output step np_eval_reduce derives and the target, -1 outside [0, D)."""
    c, meta, target, tape = ref.oracle_case(name)
    D, fixed = c["n_classes"], bool(meta["fixed_exchange"])
    target = target.copy()
    target[1] = D
    if len(target) > 3:
        target[3] = -1
    codes, cm = commstats.pack_codes(tape["mask"], tape["z"], tape["w"], target, fixed, D)
    T, B, W = tape["z"].shape
    Wp = (W + 31) // 32
    tsel = np.asarray(ref.np_eval_profile(tape, np.where((target >= 0) & (target < D), target, 0), c["top_k"], fixed)["tsel"])
    assert codes.shape == (B, 2, T, Wp) and codes.dtype == np.uint32 and cm.shape == (B, 2) and cm.dtype == np.int32
    np.testing.assert_array_equal(cm[:, 0], tsel)
    np.testing.assert_array_equal(cm[:, 1], np.where((target >= 0) & (target < D), target, -1))
    assert cm[1, 1] == -1
    for a, key in enumerate(("z", "w")):
        for b in range(B):
            for t in range(T):
                for j in range(Wp * 32):
                    bit = (int(codes[b, a, t, j >> 5]) >> (j & 31)) & 1
                    want = int(j < W and t <= tsel[b] and np.rint(tape[key][t, b, j]) == 1)
                    assert bit == want, (key, b, t, j)
    assert codes.any() and (fixed or (tsel < T - 1).any()), "the case should have dead steps and set bits"
    only_neg = commstats.pack_codes(tape["mask"], tape["z"], tape["w"], target, fixed)[1]
    assert only_neg[1, 1] == D                                                      # (without n_classes only negative targets are cut)


@pytest.mark.parametrize("name", list(pr.EXACT_CASES))
def test_exact_cases_have_no_edge_pair_and_the_restatement_equals_brute_force(name):
    c = pr.EXACT_CASES[name]
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    flat, edges = pr.brute_pair_hist(codes, meta, x, c["agent"], t0, t1, c["K"], c["W"])
    assert edges.sum() == 0, "an exact case must keep every pair away from the bin edges (a condition on the inputs)"
    got = pr.case_reference(c)
    np.testing.assert_array_equal(got, flat)
    used = c["N"] - len(c["skip"])
    assert got[:4].tolist() == [used, len(c["skip"]), used * (used - 1) // 2, 0] and got[4:].sum() == used * (used - 1) // 2
    blocked = commstats.pair_hist_np(codes, meta, x, c["agent"], t0, t1, c["K"], W=c["W"], block=7)
    np.testing.assert_array_equal(blocked, flat)                                    # (the row blocks are an implementation detail)


def test_the_cases_cover_what_the_kernel_branches_on():
    """Diagonal-only, ragged and off-diagonal tiles; one word, a full word, a ragged third word, eight words; both agents; the whole
    range, step 0 alone and an inner range; K = 1, 16, 64; F = 1, 6, 18, 64; skipped rows; one class; a row stride; the histogram
    that fits the default 48 KB of dynamic LDS, the one that needs the raised limit, the one that fits no workgroup; code words that
    fit LDS and code words that do not."""
    cs = list(pr.EXACT_CASES.values())
    assert {c["N"] for c in cs} >= {1, 2, 64, 65, 130} and {c["W"] for c in cs} >= {6, 32, 70, 256}
    assert {c["T"] for c in cs} >= {1, 10} and {c["agent"] for c in cs} == {0, 1}
    assert {c["K"] for c in cs} >= {1, 16, 64} and {c["F"] for c in cs} >= {1, 6, 18, 64}
    assert any(c["steps"] == (0, 1) and c["T"] > 1 for c in cs) and any(c["steps"] and c["steps"][0] > 0 and c["steps"][1] < c["T"] for c in cs)
    assert any(c["skip"] for c in cs) and any(c["single"] for c in cs) and any(c["ld"] and c["ld"] > c["F"] for c in cs)
    slots = lambda c: 2 * (((c["steps"] or (0, c["T"]))[1] - (c["steps"] or (0, c["T"]))[0]) * c["W"] + 1) * c["K"]
    assert slots(pr.EXACT_CASES["class_global_route"]) * 4 > 160 * 1024 and slots(pr.EXACT_CASES["class_lds_route"]) * 4 < 40 * 1024
    assert slots(pr.EXACT_CASES["class_global_route"]) == 2 * 2561 * 64
    assert 48 * 1024 < slots(pr.EXACT_CASES["class_lds_large"]) * 4 < 140 * 1024
    words = lambda c: 128 * ((((c["steps"] or (0, c["T"]))[1] - (c["steps"] or (0, c["T"]))[0]) * ((c["W"] + 31) // 32)) | 1) * 4
    assert words(pr.EXACT_CASES["class_codes_global"]) > 160 * 1024 and slots(pr.EXACT_CASES["class_codes_global"]) * 4 < 140 * 1024
    assert words(pr.EXACT_CASES["class_global_route"]) < 48 * 1024
    single = commstats.parse_pair_hist(pr.case_reference(pr.EXACT_CASES["class_single"]), 1, 32, 16)
    assert single["hist"][0].sum() == 0 and single["hist"][1].sum() == single["pairs"] > 0


def test_bounded_case_has_few_edge_pairs():
    c = pr.BOUNDED_CASE
    assert (c["F"], c["K"], c["N"]) == (512, 64, 97)
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    flat, edges = pr.brute_pair_hist(codes, meta, x, c["agent"], t0, t1, c["K"], c["W"])
    share = edges.sum() / float(flat[2])
    print("edge pairs %d of %d: %.4f" % (edges.sum(), flat[2], share))
    assert 0 < share <= pr.BOUNDED_MAX_EDGE_SHARE
    np.testing.assert_array_equal(pr.case_reference(c), flat)
    h = commstats.parse_pair_hist(flat, t1 - t0, c["W"], c["K"])["hist"]
    assert pr.assert_bounded(h, h, edges) == 0
    moved = h.copy()                                                                # one pair moved across an edge it is not close to
    p, hh, q = [int(v[0]) for v in np.nonzero((h > 0) & (np.arange(c["K"])[None, None, :] < c["K"] - 1) & (edges[:, :, 1:] == 0))]
    moved[p, hh, q] -= 1; moved[p, hh, q + 1] += 1
    with pytest.raises(AssertionError):
        pr.assert_bounded(moved, h, edges)


def test_topsim_against_scipy_and_brute_force():
    from scipy import stats
    rng = np.random.RandomState(0)
    M1, K = 40, 16
    # a joint histogram with a trend, ties in both marginals and empty rows / columns
    hh, qq = np.meshgrid(np.arange(M1), np.arange(K), indexing="ij")
    lam = 3.0 * np.exp(-((hh / float(M1) - qq / float(K)) ** 2) * 6.0)
    H = np.stack([rng.poisson(lam), rng.poisson(lam * 0.3 * (hh < 25))]).astype(np.int64)
    H[:, 7] = 0; H[:, :, 3] = 0
    t = commstats.topsim(dict(hist=H))
    h, q = pr.expand_pairs(H[0] + H[1])
    assert t["n_pairs"] == len(h) == H.sum()
    assert t["spearman"] == pytest.approx(stats.spearmanr(h, q)[0], abs=1e-12)
    assert t["pearson"] == pytest.approx(stats.pearsonr(h, (q + 0.5) * 2.0 / K)[0], abs=1e-12)
    assert 0.2 < t["spearman"] < 0.99
    hd, _ = pr.expand_pairs(H[0]); hs, _ = pr.expand_pairs(H[1])
    assert t["hamming_diff"] == pytest.approx(hd.mean(), abs=1e-12) and t["hamming_same"] == pytest.approx(hs.mean(), abs=1e-12)
    brute = ((hd[:, None] > hs[None, :]).sum() + 0.5 * (hd[:, None] == hs[None, :]).sum()) / float(len(hd) * len(hs))
    assert t["separation"] == pytest.approx(brute, abs=1e-12) and t["separation"] > 0.5
    assert t["collisions"] == H[0, 0].sum()
    assert commstats.topsim(H) == t                                                 # (the array itself does too)
    # the nan rules: an empty plane, zero variance, nothing at all
    one = commstats.topsim(np.stack([H[0], np.zeros_like(H[0])]))
    assert np.isnan(one["separation"]) and np.isnan(one["hamming_same"]) and not np.isnan(one["spearman"]) and not np.isnan(one["hamming_diff"])
    flat_q = np.zeros((2, 5, 4), np.int64); flat_q[0, :, 2] = 3; flat_q[1, 1, 2] = 2
    f = commstats.topsim(flat_q)
    assert np.isnan(f["spearman"]) and np.isnan(f["pearson"]) and f["n_pairs"] == 17 and not np.isnan(f["separation"]) and f["collisions"] == 3
    e = commstats.topsim(np.zeros((2, 5, 4), np.int64))
    assert e["n_pairs"] == 0 and e["collisions"] == 0 and all(np.isnan(e[k]) for k in ("spearman", "pearson", "hamming_same", "hamming_diff", "separation"))
    with pytest.raises(ValueError):
        commstats.topsim(np.zeros((3, 5, 4)))


def test_eval_dev_topsim_through_the_torch_form(tmp_path, monkeypatch):
    """model.eval_dev(topsim=...) on the oracle-backed engine (no eval_steps: the torch form) over two dev batches, the second one
    short: the histograms are pair_hist_np of pack_codes of the oracle's tapes; return value and confusion matrix as without."""
    from multimodalgame_amd import flags as _flags, game as _game
    from tests import oracle_engine
    from tests.test_eval_steps_cpu import oracle_tape
    monkeypatch.setattr(_game, "Engine", oracle_engine.OracleEngine)
    try:
        game, run, batches, desc, meta, z = ref.g8_game(tmp_path, "cpu", monkeypatch)
        D, T, W = int(z["n_classes"]), meta["max_exchange"], meta["rec_w_dim"]
        ts = dict(meaning="data", bins=16, steps=(0, 2), stale=1)
        acc_t, extra_t = run("with.txt", topsim=ts)
        acc, extra = run("without.txt")
        assert acc_t == acc and extra_t == extra
        assert open(str(tmp_path / "with.txt")).read() == open(str(tmp_path / "without.txt")).read()
        packed = [commstats.pack_codes(*[oracle_tape(dict(meta, batch=len(x)), x, t, desc, float(z["s_bias"]))[k] for k in ("mask", "z", "w")], t, False, D)
                  for x, t in batches]
        codes, cm = np.concatenate([p[0] for p in packed]), np.concatenate([p[1] for p in packed])
        data = np.concatenate([x for x, _ in batches])
        n = len(data)
        assert "stale" not in ts and ts["meaning"] == "data" and ts["bins"] == 16
        for a, agent in enumerate(("sender", "receiver")):
            want = commstats.parse_pair_hist(commstats.pair_hist_np(codes, cm, data, a, 0, 2, 16, W=W), 2, W, 16)
            np.testing.assert_array_equal(ts["hist"][agent]["hist"], want["hist"])
            assert ts["hist"][agent]["head"].tolist() == [n, 0, n * (n - 1) // 2, 0]
            assert ts[agent] == pytest.approx(commstats.topsim(want), nan_ok=True) and ts[agent]["n_pairs"] == n * (n - 1) // 2
        ts2 = dict(meaning="desc")                                                  # the class-level measure, every step, 64 bins
        run("desc.txt", topsim=ts2)
        want = commstats.pair_hist_np(codes, cm, desc[cm[:, 1]], 0, 0, T, 64, W=W)
        np.testing.assert_array_equal(ts2["hist"]["sender"]["hist"].reshape(-1), want[4:])
        assert ts2["bins"] == 64 and ts2["steps"] is None
        with pytest.raises(ValueError):
            run("bad.txt", topsim=dict(meaning="words"))
    finally:
        _flags.FLAGS.Reset()


def test_end_to_end_case_is_exact_and_mixes_output_steps(tmp_path, monkeypatch):
    """The inputs of the GPU's end-to-end case (tests/pairs_ref.py: e2e_batches on the g8 game): no pair of class descriptions is
    within the fp32 error of one of the 15 inner bin edges, so the class-level histogram is an exact case; and with receiver.s.weight
    x 30 the oracle's conversations end at several output steps."""
    from multimodalgame_amd import flags as _flags, game as _game, model
    from tests import oracle_engine
    import torch
    monkeypatch.setattr(_game, "Engine", oracle_engine.OracleEngine)
    try:
        game, run, batches, desc, meta, z = ref.g8_game(tmp_path, "cpu", monkeypatch)
        D, fl = int(z["n_classes"]), common.flags_from_meta(meta)
        dist, tol = pr.class_edge_distance(desc, pr.E2E_BINS)
        print("class-level cosines: nearest edge at %.3e, tolerance %.3e" % (dist, tol))
        assert dist > tol
        many = pr.e2e_batches(D, fl.img_feat_dim, fl.wv_dim)
        assert [len(x) for x, _ in many] == [32, 32, 6]

        def fake_load_hdf5(*a, **kw):
            for x, t in many:
                yield {"target": torch.from_numpy(t), "avgpool_512": torch.from_numpy(x)}
        monkeypatch.setattr(model, "load_hdf5", fake_load_hdf5)
        game.engine_for(32, D).params["receiver"]["s.weight"].mul_(pr.E2E_S_SCALE)
        prof, ts = {}, dict(meaning="desc", bins=pr.E2E_BINS)
        model.eval_dev("dev", 32, 0, False, 2, game, torch.from_numpy(desc), int, str(tmp_path / "e2e.txt"), torch.device("cpu"), profile=prof, topsim=ts)
        steps = prof["steps"].sum(0)
        print("output steps", steps.tolist())
        assert (steps > 0).sum() >= 2 and steps.sum() == 70
        assert ts["hist"]["sender"]["head"].tolist() == [70, 0, 70 * 69 // 2, 0]
    finally:
        _flags.FLAGS.Reset()


def test_accumulator_keywords():
    from multimodalgame_amd.game import EvalAccumulator
    with pytest.raises(ValueError):
        EvalAccumulator(3, 2, meaning="data")                                       # a meaning matrix needs the codes
    with pytest.raises(ValueError):
        EvalAccumulator(3, 2, codes=8, meaning="words")
    with pytest.raises(ValueError):
        EvalAccumulator(3, 2, codes=0)
    with pytest.raises(ValueError):
        EvalAccumulator(3, 2).pair_hist()
    with pytest.raises(ValueError):
        EvalAccumulator(3, 2, codes=8, meaning="data").pair_hist()                  # nothing added yet
    acc = EvalAccumulator(3, 2, codes=8)
    assert sorted(acc.fetch()) == sorted(EvalAccumulator(3, 2).fetch())             # fetch() is unchanged
