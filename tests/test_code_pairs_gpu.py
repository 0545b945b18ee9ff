"""mmg_eval_steps_codes and mmg_code_pair_hist on the GPU (include/mmg.h; csrc/kernels_eval.h: k_eval_codes; csrc/kernels_pairs.h:
k_pair_norms, k_pair_hist).

The pair histogram runs on synthetic codes (tests/pairs_ref.py).  EXACT cases -- tests/test_code_pairs_cpu.py asserts that no pair
of theirs is within the fp32 error of a bin edge -- must equal commstats.pair_hist_np (float64 cosine) entry for entry, head included;
the one BOUNDED case (F = 512) must keep the Hamming marginals and may move only its edge pairs across their own edge.  The codes of
real conversations must equal commstats.pack_codes of the GPU's own tape exactly, with acc / lens / batch / prof byte-equal to what
mmg_eval_steps_profile leaves.  eval_dev(topsim=...) gives the same histograms through the library form and the torch form."""
import ctypes as C

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib, commstats
from multimodalgame_amd.game import EvalAccumulator
from oracle import cpu_ref
from tests import common
from tests import eval_profile_ref as ref
from tests import pairs_ref as pr
from tests.test_eval_steps_cpu import CASES, case_meta

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev_codes(codes, meta):
    return torch.from_numpy(np.array(codes).view(np.int32)).to(DEV), torch.from_numpy(np.array(meta)).to(DEV)      # (copies: the cases are read-only)


def _dev_meaning(x, ld=None):
    """The meaning matrix on the device with row stride ld (the padding columns hold NaN: they must never be read)."""
    N, F = x.shape
    buf = torch.full((N, ld or F), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :F] = torch.from_numpy(np.array(x)).to(DEV)
    return buf


def _pair_hist(codes_d, meta_d, n_rows, T, W, agent, t0, t1, x_d, F, K, hist=None, row_off=0):
    """One mmg_code_pair_hist call through ctypes -> (status, flat device histogram, inv)."""
    lib = _lib.load()
    n = int(lib.mmg_code_pair_hist_count(t1 - t0, W, K))
    assert n == commstats.pair_hist_count(t1 - t0, W, K)
    if hist is None:
        hist = torch.zeros(n, dtype=torch.int64, device=DEV)
    inv = torch.full((max(n_rows, 1),), float("nan"), dtype=torch.float32, device=DEV)
    cd, mt, xx = codes_d[row_off:], meta_d[row_off:], x_d[row_off:]
    st = lib.mmg_code_pair_hist(_p(cd), _p(mt), n_rows, T, W, agent, t0, t1, _p(xx), F, x_d.stride(0), _p(inv), K, _p(hist), _stream())
    return st, hist, inv


def _run_case(c):
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    cd, mt = _dev_codes(codes, meta)
    st, hist, inv = _pair_hist(cd, mt, c["N"], c["T"], c["W"], c["agent"], t0, t1, _dev_meaning(x, c["ld"]), c["F"], c["K"])
    assert st == 0, _lib.load().mmg_last_error()
    torch.cuda.synchronize()
    return hist.cpu().numpy(), inv.cpu().numpy(), x


@pytest.mark.parametrize("name", list(pr.EXACT_CASES))
def test_pair_hist_exact_cases_equal_the_float64_restatement(name):
    c = pr.EXACT_CASES[name]
    got, inv, x = _run_case(c)
    want = pr.case_reference(c)
    t0, t1 = pr.case_inputs(c)[3:]
    g = commstats.parse_pair_hist(got, t1 - t0, c["W"], c["K"])
    print(name, "head", g["head"].tolist(), "planes", g["hist"][0].sum(), g["hist"][1].sum())
    np.testing.assert_array_equal(got, want)
    used = c["N"] - len(c["skip"])
    assert g["head"].tolist() == [used, len(c["skip"]), used * (used - 1) // 2, 0] and g["hist"].sum() == g["pairs"]
    if c["single"]:
        assert g["hist"][0].sum() == 0 and g["hist"][1].sum() == g["pairs"]
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    np.testing.assert_allclose(inv, 1.0 / norm, rtol=(c["F"] + 4) * 2.0 ** -24, atol=0)


def test_pair_hist_bounded_case_moves_edge_pairs_only():
    c = pr.BOUNDED_CASE
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    _, edges = pr.brute_pair_hist(codes, meta, x, c["agent"], t0, t1, c["K"], c["W"])
    got = commstats.parse_pair_hist(_run_case(c)[0], t1 - t0, c["W"], c["K"])
    want = commstats.parse_pair_hist(pr.case_reference(c), t1 - t0, c["W"], c["K"])
    np.testing.assert_array_equal(got["head"], want["head"])
    moved = pr.assert_bounded(got["hist"], want["hist"], edges)
    print("bounded: edge pairs", int(edges.sum()), "of", got["pairs"], "cumulative counts moved", moved)


def test_pair_hist_clamps_identical_opposite_and_zero_rows():
    """Identical rows (c = 1 +- ulp) fall into bin 0, opposite rows (u = K) into bin K - 1, a zero row has c = 0 exactly: bin K / 2."""
    T, W, K, F = 1, 6, 16, 18
    codes, meta = pr.synthetic_codes(5, T, W, seed=11)
    x = pr.features(5, F, 11)
    x[1] = x[0]; x[2] = -x[0]; x[3] = 0.0
    x[4] = x[0] * 3.0                                                # a positive multiple: c = 1 up to rounding
    cd, mt = _dev_codes(codes, meta)
    st, hist, inv = _pair_hist(cd, mt, 5, T, W, 0, 0, 1, _dev_meaning(x), F, K)
    assert st == 0
    torch.cuda.synchronize()
    got = commstats.parse_pair_hist(hist.cpu().numpy(), 1, W, K)["hist"].sum((0, 1))
    # pairs: (0,1) (0,4) (1,4) identical -> bin 0; (0,2) (1,2) (2,4) opposite -> bin K - 1; four pairs with the zero row -> bin K / 2
    want = np.zeros(K, np.int64); want[0], want[K - 1], want[K // 2] = 3, 3, 4
    np.testing.assert_array_equal(got, want)
    assert inv.cpu().numpy()[3] == 0.0
    np.testing.assert_array_equal(hist.cpu().numpy(), commstats.pair_hist_np(codes, meta, x, 0, 0, 1, K, W=W))


def test_two_calls_add_into_one_histogram():
    """Rows [0, 64) and rows [64, 130) of one case into ONE histogram: the sum of the two restatements, heads included."""
    c = pr.EXACT_CASES["class_N130_ld"]
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    cd, mt = _dev_codes(codes, meta)
    xd = _dev_meaning(x, c["ld"])
    args = (c["T"], c["W"], c["agent"], t0, t1, xd, c["F"], c["K"])
    st, hist, _ = _pair_hist(cd, mt, 64, *args)
    st2, hist, _ = _pair_hist(cd, mt, 66, *args, hist=hist, row_off=64)
    assert st == 0 and st2 == 0
    torch.cuda.synchronize()
    want = (commstats.pair_hist_np(codes[:64], meta[:64], x[:64], c["agent"], t0, t1, c["K"], W=c["W"])
            + commstats.pair_hist_np(codes[64:], meta[64:], x[64:], c["agent"], t0, t1, c["K"], W=c["W"]))
    np.testing.assert_array_equal(hist.cpu().numpy(), want)
    st, again, _ = _pair_hist(cd, mt, 64, *args)                      # the same call into a second zeroed histogram: the same integers
    st2, again, _ = _pair_hist(cd, mt, 66, *args, hist=again, row_off=64)
    torch.cuda.synchronize()
    assert torch.equal(again, hist)


def test_pair_hist_refusals_enqueue_nothing():
    c = pr.EXACT_CASES["feat_N65_F6_K16"]
    codes, meta, x, t0, t1 = pr.case_inputs(c)
    cd, mt = _dev_codes(codes, meta)
    xd = _dev_meaning(x)
    lib = _lib.load()
    n = int(lib.mmg_code_pair_hist_count(1, 6, 16))
    hist = torch.zeros(n, dtype=torch.int64, device=DEV)
    inv = torch.zeros(65, dtype=torch.float32, device=DEV)
    good = dict(codes=_p(cd), meta=_p(mt), n_rows=65, T=1, W=6, agent=0, t0=0, t1=1, x=_p(xd), F=6, ld=6, inv=_p(inv), K=16, hist=_p(hist))
    order = ("codes", "meta", "n_rows", "T", "W", "agent", "t0", "t1", "x", "F", "ld", "inv", "K", "hist")
    bad = [dict(codes=None), dict(meta=None), dict(x=None), dict(inv=None), dict(hist=None), dict(n_rows=0), dict(n_rows=65537),
           dict(F=0), dict(F=4097), dict(K=0), dict(K=1025), dict(agent=2), dict(agent=-1), dict(t0=-1), dict(t0=1), dict(t1=2),
           dict(ld=5), dict(T=0), dict(W=0), dict(T=64, W=1 << 20, t1=64, K=1)]
    for b in bad:
        a = dict(good, **b)
        assert lib.mmg_code_pair_hist(*[a[k] for k in order], _stream()) < 0, b
        assert lib.mmg_last_error().startswith(b"mmg_code_pair_hist"), (b, lib.mmg_last_error())
    torch.cuda.synchronize()
    assert not hist.any() and not inv.any(), "a refused call enqueues nothing"
    assert lib.mmg_code_pair_hist_count(0, 6, 16) < 0 and lib.mmg_code_pair_hist_count(1, 6, 1025) < 0
    assert lib.mmg_code_pair_hist_count(64, 256, 1024) < 0 and b"2^24" in lib.mmg_last_error()
    assert lib.mmg_code_pair_hist(*[good[k] for k in order], _stream()) == 0
    torch.cuda.synchronize()
    assert int(hist[2]) == 65 * 64 // 2


# ---------------------------------------------------------------------------------------------
# mmg_eval_steps_codes on real conversations
# ---------------------------------------------------------------------------------------------
CODE_CASES = dict(ref.PROFILE_CASES)
CODE_CASES["tiny_D2"] = dict(CASES["tiny_ragged"], n_classes=2)
CODE_CASES["tiny_B1"] = dict(CASES["tiny_ragged"], batch=1)
CODE_CASES["c1_B64_sx30"] = dict(CASES["c1_B64"], s_scale=30.0)                # receiver.s.weight x 30 spreads the stop probabilities
CODE_CASE_NAMES = ["tiny_ragged", "tiny_fixed", "tiny_W70", "tiny_D2", "tiny_B1", "c1_B64", "c1_B64_sx30", "D130_B17"]


def _case_inputs(name):
    c = CODE_CASES[name]
    meta = case_meta(c)
    x, target, desc = cpu_ref.synthetic_batch(c["batch"], c["n_classes"], meta["img_feat_dim"], meta["wv_dim"], seed=c["seed_data"])
    return c, meta, x, target, desc


def _engine(meta, s_bias=None, batch=None, s_scale=None):
    eng = common.make_engine(meta, **({} if batch is None else dict(batch=batch)))
    if s_bias is not None:
        eng.params["receiver"]["s.bias"].fill_(float(s_bias))
    if s_scale is not None:
        eng.params["receiver"]["s.weight"].mul_(float(s_scale))
    return eng


def _tape(eng):
    tp, B, T = eng.tape, eng.cfg.batch, eng.cfg.max_exchange
    return dict(mask=tp["mask"].view(T + 1, B).clone(), z=tp["z"].view(T, B, -1).clone(), w=tp["w"].view(T, B, -1).clone())


def _dev(eng, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrays]


def _want_codes(tape, target, fixed, D):
    return commstats.pack_codes(tape["mask"].cpu().numpy(), tape["z"].cpu().numpy(), tape["w"].cpu().numpy(), target, fixed, D)


def _u32(codes):
    return codes.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("with_prof", [False, True])
@pytest.mark.parametrize("name", CODE_CASE_NAMES)
def test_codes_equal_pack_codes_of_the_gpu_tape(name, with_prof):
    c, meta, x, target, desc = _case_inputs(name)
    D, T, k, B = c["n_classes"], meta["max_exchange"], c["top_k"], c["batch"]
    fixed = bool(meta["fixed_exchange"])
    eng = _engine(meta, c["s_bias"], s_scale=c.get("s_scale"))
    xd, td, dd = _dev(eng, x, target, desc)
    acc0, prof0 = eng.eval_acc(), eng.eval_profile()
    lens0, rows0 = eng.eval_steps(xd, td, dd, 1, k, acc0, prof=prof0)           # mmg_eval_steps_profile: what must not move
    acc, prof = eng.eval_acc(), eng.eval_profile()
    codes, cmeta = eng.eval_codes(B + 2)
    codes.fill_(-1); cmeta.fill_(-7)                                             # (every word of a written row is written; the others stay)
    lens, rows = eng.eval_steps(xd, td, dd, 1, k, acc, codes=(codes, cmeta, 1), **(dict(prof=prof) if with_prof else {}))
    tape = _tape(eng)
    torch.cuda.synchronize()
    eng.check_sync()
    assert torch.equal(acc, acc0) and torch.equal(lens, lens0) and torch.equal(rows, rows0)
    assert torch.equal(prof, prof0) if with_prof else not prof.any()
    want, want_meta = _want_codes(tape, target, fixed, D)
    got, got_meta = _u32(codes), cmeta.cpu().numpy()
    print(name, "tsel", np.bincount(got_meta[1:B + 1, 0], minlength=T).tolist(), "bits", int(np.unpackbits(got[1:B + 1].view(np.uint8)).sum()))
    np.testing.assert_array_equal(got_meta[1:B + 1], want_meta)
    np.testing.assert_array_equal(got[1:B + 1], want)
    assert (got[0] == 0xFFFFFFFF).all() and (got[B + 1] == 0xFFFFFFFF).all() and (got_meta[[0, B + 1]] == -7).all()
    assert want.any() and int(eng.tape["counter"][0]) == 0
    if name.startswith("c1_B64"):
        assert len(np.unique(want_meta[:, 0])) >= 2, "the case should mix output steps"
    if fixed:
        assert (want_meta[:, 0] == T - 1).all()


def test_three_batches_two_engines_fill_one_buffer_with_bad_targets_and_a_mask():
    """n = 3 batches of 5 in one call, then a batch of 3 from a second engine through row0 = 15: one buffer in dataset order.  Two
    targets lie outside [0, D); the last call runs under a corruption mask and packs the sender's bits as the receiver saw them."""
    c, meta, _, _, desc = _case_inputs("tiny_ragged")
    D, T, k, W = c["n_classes"], meta["max_exchange"], c["top_k"], meta["rec_w_dim"]
    xs, ts = zip(*[cpu_ref.synthetic_batch(b, D, meta["img_feat_dim"], meta["wv_dim"], seed=c["seed_data"] + i)[:2]
                   for i, b in enumerate((5, 5, 5, 3))])
    ts = [t.copy() for t in ts]
    ts[1][2], ts[3][0] = D, -1
    eng5, eng3 = _engine(meta, c["s_bias"]), _engine(meta, c["s_bias"], batch=3)
    codes, cmeta = eng5.eval_codes(18)
    acc = eng5.eval_acc()
    wants = []
    xd, td, dd = _dev(eng5, np.concatenate(xs[:3]), np.concatenate(ts[:3]), desc)
    for i in range(3):                                                            # the tapes of the three batches, one by one
        eng5.eval_steps(xd[5 * i:5 * i + 5], td[5 * i:5 * i + 5], dd, 1, k, eng5.eval_acc())
        wants.append(_want_codes(_tape(eng5), ts[i], False, D))
    eng5.eval_steps(xd, td, dd, 3, k, acc, codes=(codes, cmeta, 0))
    x3, t3 = _dev(eng3, xs[3], ts[3])
    mask = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.float32).view(-1, 1)
    eng3.eval_steps(x3, t3, dd, 1, k, acc, codes=(codes, cmeta, 15), corrupt_mask=mask)
    wants.append(_want_codes(_tape(eng3), ts[3], False, D))
    eng3.eval_steps(x3, t3, dd, 1, k, eng3.eval_acc())
    clean = _want_codes(_tape(eng3), ts[3], False, D)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(codes), np.concatenate([w[0] for w in wants]))
    np.testing.assert_array_equal(cmeta.cpu().numpy(), np.concatenate([w[1] for w in wants]))
    assert cmeta.cpu().numpy()[[7, 15], 1].tolist() == [-1, -1] and int(acc[2]) == 18
    assert not np.array_equal(wants[3][0][:, 0], clean[0][:, 0]), "the mask should change the sender's bits that are packed"
    # ... and through the accumulator, which owns the buffers, the row count and the class-level meaning matrix
    dacc = EvalAccumulator(D, k, codes=4, meaning="desc")                         # (starts too small: it grows)
    dacc.add(eng5, xd, td, dd, 3)
    dacc.add(eng3, x3, t3, dd, 1)
    torch.cuda.synchronize()
    assert dacc.rows == 18 and "profile" not in dacc.fetch()
    np.testing.assert_array_equal(_u32(dacc.codes[:15]), _u32(codes[:15]))
    h = dacc.pair_hist(agent="receiver", steps=(0, 2), bins=16)
    cd_h, mt_h = _u32(dacc.codes[:18]), dacc.meta[:18].cpu().numpy()
    np.testing.assert_array_equal(dacc.meaning[:18].cpu().numpy(), desc[np.clip(np.concatenate(ts), 0, D - 1)])
    want = commstats.pair_hist_np(cd_h, mt_h, dacc.meaning[:18].cpu().numpy(), 1, 0, 2, 16, W=W)
    np.testing.assert_array_equal(np.concatenate([h["head"], h["hist"].reshape(-1)]), want)
    assert h["used"] == 16 and h["skipped"] == 2 and h["pairs"] == 120


def test_codes_refusals():
    c, meta, x, target, desc = _case_inputs("tiny_ragged")
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)
    acc = eng.eval_acc()
    lens, rows = eng.eval_steps(xd, td, dd, 1, 2, acc)
    before = acc.clone()
    codes, cmeta = eng.eval_codes(5)
    codes.fill_(-1)
    lib = eng.lib
    args = [eng.handle, _p(xd), _p(td), 1, _p(dd), 2, _p(acc), _p(lens), _p(rows), None, _p(codes), _p(cmeta), 0, 5, eng._stream()]
    for i, v in ((10, None), (11, None), (12, -1), (13, 4), (12, 1), (1, None), (2, None), (4, None), (6, None), (7, None), (8, None), (5, 0)):
        a = list(args)
        a[i] = v
        assert lib.mmg_eval_steps_codes(*a) < 0, (i, v)
    a = list(args); a[3], a[13] = 2, 9                                           # two batches need ten rows
    assert lib.mmg_eval_steps_codes(*a) < 0 and b"do not fit" in lib.mmg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(acc, before) and (codes == -1).all(), "a refused call enqueues nothing"
    assert lib.mmg_eval_steps_codes(*args) == 0                                  # cap_rows exactly enough
    c2, meta2, x2, target2, desc2 = ref.case_inputs("tiny_continuous")
    cont = _engine(meta2)
    assert int(lib.mmg_eval_code_words(C.byref(cont.cfg))) < 0
    x2d, t2d, d2d = _dev(cont, x2, target2, desc2)
    acc2 = cont.eval_acc()
    l2, r2 = cont.eval_steps(x2d, t2d, d2d, 1, 2, acc2)
    a = [cont.handle, _p(x2d), _p(t2d), 1, _p(d2d), 2, _p(acc2), _p(l2), _p(r2), None, _p(codes), _p(cmeta), 0, 5, cont._stream()]
    assert lib.mmg_eval_steps_codes(*a) < 0 and b"continuous" in lib.mmg_last_error()
    with pytest.raises(_lib.MmgError):
        cont.eval_codes(5)
    torch.cuda.synchronize()


def test_codes_kernel_runs_under_the_new_entry_only():
    c, meta, x, target, desc = ref.case_inputs("tiny_ragged")
    eng = _engine(meta, c["s_bias"])
    xd, td, dd = _dev(eng, x, target, desc)

    def names(n, **kw):
        eng.set_profiling(True)
        eng.eval_steps(torch.cat([xd] * n), torch.cat([td] * n), dd, n, c["top_k"], eng.eval_acc(), **kw)
        torch.cuda.synchronize()
        out = [name for name, _ in eng.kernel_times()]
        eng.set_profiling(False)
        return out
    plain = names(1)
    assert "k_eval_codes" not in plain and plain[-1] == "k_eval_reduce", plain
    prof = names(1, prof=eng.eval_profile())
    assert prof == plain + ["k_eval_profile"], prof
    codes, cmeta = eng.eval_codes(10)
    assert names(2, codes=(codes, cmeta, 0)) == (plain + ["k_eval_codes"]) * 2
    assert names(2, codes=(codes, cmeta, 0), prof=eng.eval_profile()) == (plain + ["k_eval_profile", "k_eval_codes"]) * 2


def test_visual_attention_handle():
    from tests import test_visual_attn_gpu as vg, visual_attn_ref as vref
    m = vref.meta("B")
    eng = vg._engine(m)
    (xd, td, dd), _, g = vg._inputs(m, eng)
    eng.set_data_context(g)
    codes, cmeta = eng.eval_codes(eng.cfg.batch)
    eng.eval_steps(xd, td, dd, 1, 2, eng.eval_acc(), codes=(codes, cmeta, 0))
    tape = _tape(eng)
    torch.cuda.synchronize()
    want, want_meta = _want_codes(tape, td.cpu().numpy(), bool(common.flags_from_meta(m).fixed_exchange), eng.cfg.n_classes)
    np.testing.assert_array_equal(_u32(codes), want)
    np.testing.assert_array_equal(cmeta.cpu().numpy(), want_meta)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_eval_dev_topsim_library_form_equals_torch_form(tmp_path, monkeypatch):
    """model.eval_dev(topsim=...) over 70 samples in batches of 32 with a final 6, class-level meaning (an exact case: 15 distinct
    cosines, which tests/test_code_pairs_cpu.py asserts to be far from every edge): the library form (k_eval_codes per batch, two pair
    launches per agent) gives the histograms of the torch form on the same engine (MMG_EVAL_TORCH=1), and return value and confusion
    matrix are those of a run without topsim."""
    from multimodalgame_amd import flags as _flags, model
    try:
        game, run, batches, desc, meta, z = ref.g8_game(tmp_path, DEV, monkeypatch)
        D, fl = int(z["n_classes"]), common.flags_from_meta(meta)
        many = pr.e2e_batches(D, fl.img_feat_dim, fl.wv_dim)
        tdev = torch.device(DEV)

        def fake_load_hdf5(*a, **kw):
            for x, t in many:
                yield {"target": torch.from_numpy(t).to(tdev), "avgpool_512": torch.from_numpy(x).to(tdev)}
        monkeypatch.setattr(model, "load_hdf5", fake_load_hdf5)
        run = lambda path, **kw: model.eval_dev("dev", 32, 0, False, 2, game, torch.from_numpy(desc).to(tdev), int, str(tmp_path / path), tdev, **kw)
        game.engine_for(32, D).params["receiver"]["s.weight"].mul_(pr.E2E_S_SCALE)   # (one parameter buffer: every batch size sees it)
        ts_lib, ts_py = dict(meaning="desc", bins=pr.E2E_BINS), dict(meaning="desc", bins=pr.E2E_BINS)
        plain = run("plain.txt")
        prof = {}
        lib_out = run("lib.txt", topsim=ts_lib, profile=prof)                      # (together with the profile: three launches per batch)
        assert (prof["steps"].sum(0) > 0).sum() >= 2, "the scaled stop weights should mix the output steps: %s" % prof["steps"].sum(0).tolist()
        monkeypatch.setenv("MMG_EVAL_TORCH", "1")
        py_out = run("py.txt", topsim=ts_py)
        assert lib_out == plain and lib_out[0] == pytest.approx(py_out[0], abs=1e-12)
        assert open(str(tmp_path / "lib.txt")).read() == open(str(tmp_path / "plain.txt")).read() == open(str(tmp_path / "py.txt")).read()
        for agent in ("sender", "receiver"):
            hl, hp = ts_lib["hist"][agent], ts_py["hist"][agent]
            np.testing.assert_array_equal(hl["head"], hp["head"])
            np.testing.assert_array_equal(hl["hist"], hp["hist"])
            assert hl["head"].tolist() == [70, 0, 70 * 69 // 2, 0]
            assert ts_lib[agent] == pytest.approx(ts_py[agent], nan_ok=True)
            assert ts_lib[agent]["n_pairs"] == 70 * 69 // 2
        print("topsim", {k: ts_lib["sender"][k] for k in ("spearman", "separation", "collisions")})
    finally:
        _flags.FLAGS.Reset()
