"""mmg_eval_steps / k_eval_reduce (include/mmg.h, csrc/kernels_eval.h) without a GPU: the two entry points exist, the accumulator
layout is what the Python side parses, and a numpy restatement of the reduction -- kept here, used by the GPU tests too -- fed
with the oracle's eval tape reproduces the reference's numbers of the g8 and g4 fixtures.  Also: every shape the GPU tests run
has clear gaps at the top-k boundary and at the argmax in the oracle's logits, so that "strictly more than top_k - 1 logits
above the target's" (the kernel) and torch.topk / argsort (the torch form, the reference) cannot disagree on any sample."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from multimodalgame_amd import _lib
from oracle import cpu_ref
from tests import common, corrupt_ref

TINY = dict(use_binary=True, fixed_exchange=False, max_exchange=4, batch_size=5, learning_rate=1e-4, img_feat_dim=16, img_h_dim=8,
            rec_w_dim=6, sender_out_dim=6, rec_hidden=5, wv_dim=7, baseline_hid_dim=9, top_k_train=2, top_k_dev=2)
C1 = dict(use_binary=True, fixed_exchange=False, max_exchange=10, batch_size=64, learning_rate=1e-4, entropy_rec=0.01,
          entropy_sen=0.01, entropy_s=0.08, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32,
          rec_hidden=64, wv_dim=100, baseline_hid_dim=500, top_k_train=6, top_k_dev=6)

# The shapes of tests/test_eval_steps_gpu.py that no fixture covers: flags, classes, batch, top_k, receiver s.bias (None: the
# filled one), seeds.  Smallest shapes at which k_eval_reduce can still go wrong: a ragged batch below one wave's worth of
# sample workgroups, everyone stopping at step 1 (n = 1), nobody stopping (n = T, tsel = T - 1), T = 1, Fixed mode, top_k >= D,
# more classes than a wave has lanes (130, and 1000 on k_conversation_mc), continuous messages, config 1's shape at B = 64, and
# continuous messages with Adaptive stopping on the register-resident kernels (c1_cont_B64) and on k_conversation_mc3 with
# train = False (D130_cont_B17): s.bias 1.2 spreads their output steps over 7 and 4 values.
# (The stop bit s = 1 KEEPS a sample talking -- the mask is the running minimum of s, model.py:852 -- so the strongly negative
# s.bias is the one that ends every conversation at step 1 and the strongly positive one never stops.)
CASES = {
    "tiny_ragged": dict(flags=TINY, n_classes=3, batch=5, top_k=2, s_bias=0.6, seed_weights=13, seed_data=12),
    "tiny_all_stop": dict(flags=TINY, n_classes=3, batch=5, top_k=2, s_bias=-8.0, seed_weights=13, seed_data=12),
    "tiny_never_stop": dict(flags=TINY, n_classes=3, batch=5, top_k=2, s_bias=8.0, seed_weights=13, seed_data=12),
    "tiny_T1": dict(flags=dict(TINY, max_exchange=1), n_classes=3, batch=5, top_k=2, s_bias=None, seed_weights=13, seed_data=12),
    "tiny_fixed": dict(flags=dict(TINY, fixed_exchange=True), n_classes=3, batch=5, top_k=2, s_bias=None, seed_weights=13, seed_data=12),
    "tiny_topk_ge_D": dict(flags=TINY, n_classes=3, batch=5, top_k=5, s_bias=0.6, seed_weights=13, seed_data=12),
    "tiny_continuous": dict(flags=dict(TINY, use_binary=False), n_classes=3, batch=5, top_k=2, s_bias=None, seed_weights=13, seed_data=12),
    "c1_B64": dict(flags=C1, n_classes=30, batch=64, top_k=6, s_bias=1.2, seed_weights=5, seed_data=6),
    "D130_B17": dict(flags=C1, n_classes=130, batch=17, top_k=6, s_bias=1.2, seed_weights=5, seed_data=6),
    "D1000_B16": dict(flags=C1, n_classes=1000, batch=16, top_k=6, s_bias=1.2, seed_weights=5, seed_data=6),
    "c1_cont_B64": dict(flags=dict(C1, use_binary=False), n_classes=30, batch=64, top_k=6, s_bias=1.2, seed_weights=5, seed_data=6),
    "D130_cont_B17": dict(flags=dict(C1, use_binary=False), n_classes=130, batch=17, top_k=6, s_bias=1.2, seed_weights=5, seed_data=6),
}
MIN_GAP = 1e-4


def case_meta(c):
    meta = dict(cpu_ref.Flags(**c["flags"]).__dict__)
    meta.update(n_classes=c["n_classes"], batch=c["batch"], n_minibatches=1, seed_weights=c["seed_weights"],
                seed_data=c["seed_data"], seed_uniforms=0)
    return meta


def oracle_tape(meta, x, target, desc, s_bias=None, corrupt=None):
    """The run-all eval tape of the CPU oracle, laid out as the engine's: mask [T + 1, B] (running minimum of the stop bits),
    s [T, B], z / w [T, B, W], y [T, B, D]."""
    fl = common.flags_from_meta(meta)
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    if s_bias is not None:
        with torch.no_grad():
            models["receiver"].s.bias.fill_(float(s_bias))
    if corrupt is not None:
        corrupt_ref.corrupt_sender(models["sender"], corrupt)
    args = dict(data=torch.from_numpy(x), target=torch.from_numpy(target), desc=torch.from_numpy(desc), train=False, break_early=False)
    with torch.no_grad():
        s, sen_w, rec_w, y, _, _ = cpu_ref.exchange(models["sender"], models["receiver"], None, None, args, fl)
    B = x.shape[0]
    st = lambda v: torch.stack([t.float().view(B, -1) for t in v]).numpy()
    tape = dict(mask=st(s[0])[:, :, 0].astype(np.uint8), s=st(s[1])[:, :, 0], z=st(sen_w[0]), w=st(rec_w[0]), y=st(y))
    tape["mask"][-1] = np.minimum(tape["mask"][-2], tape["s"][-1].astype(np.uint8))      # (exchange() forces the last mask to 0)
    return tape


def np_eval_reduce(tape, target, top_k, fixed):
    """What k_eval_reduce leaves for ONE batch (csrc/kernels_eval.h), restated in numpy."""
    mask, s, y = tape["mask"].astype(np.int64), tape["s"], tape["y"]
    T, B, D = y.shape
    if fixed:
        n, tsel = T, np.full(B, T - 1)
    else:
        dead = np.nonzero(mask[1:].sum(1) == 0)[0]
        n = int(dead[0]) + 1 if len(dead) else T
        tsel = mask[1:n].sum(0)
    sel = y[tsel, np.arange(B)]
    above = (sel > sel[np.arange(B), target][:, None]).sum(1)
    hit = above < min(top_k, D)
    pred = sel.argmax(1)                                  # (numpy: the first maximum)
    conf, seen = np.zeros((D, D), np.int64), np.zeros(D, np.int64)
    np.add.at(conf, (target, pred), 1)
    np.add.at(seen, target, 1)
    np.add.at(seen, pred, 1)
    ham = lambda m: np.abs(m.astype(np.float64) - np.concatenate([np.zeros_like(m[:1]), m[:-1]]).astype(np.float64)).sum((1, 2))
    return dict(n=n, tsel=tsel, sel=sel, hit=hit, hits=int(hit.sum()), pred=pred, conf=conf, seen=seen,
                lens=(s[:n] != 0).sum(0).astype(np.int64), ham_sen=ham(tape["z"]), ham_rec=ham(tape["w"]))


def gaps(sel, top_k):
    """Per sample: the gap between the top_k-th and the next logit (inf when top_k >= D), and between the two largest."""
    srt = -np.sort(-sel.astype(np.float64), axis=1)
    D = sel.shape[1]
    k = min(top_k, D)
    return (srt[:, k - 1] - srt[:, k]) if k < D else np.full(len(sel), np.inf), srt[:, 0] - srt[:, 1]


def test_library_exports_eval_entry_points():
    lib = _lib.load()
    assert lib.mmg_eval_steps is not None and lib.mmg_eval_acc_count is not None      # (AttributeError: the symbol is missing)
    assert "mmg_eval_steps" in _lib.SYMBOLS and "mmg_eval_acc_count" in _lib.SYMBOLS
    header = open(os.path.join(os.path.dirname(common.GOLDEN_DIR), "..", "include", "mmg.h")).read()
    assert "int64_t mmg_eval_acc_count(const mmg_config* cfg);" in header
    assert "int mmg_eval_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k," in header
    assert "#define MMG_VERSION 3" in header and lib.mmg_version() == 3


def test_accumulator_layout_matches_python_side():
    """mmg_eval_acc_count = 4 + D * D + D, and EvalAccumulator.fetch() parses [hits, batches, samples, 0 | conf | seen] followed
    by the per-batch rows [n | ham_sen[T] | ham_rec[T]] and the lengths -- checked on CPU tensors filled from the numpy
    restatement (binary counts and the float64 bits of continuous sums)."""
    from multimodalgame_amd.game import EvalAccumulator
    lib = _lib.load()
    for D in (2, 3, 30, 130, 1000):
        cfg = _lib.make_config(**common.engine_kwargs(case_meta(dict(CASES["tiny_ragged"], n_classes=D))))
        assert lib.mmg_eval_acc_count(C.byref(cfg)) == _lib.EVAL_ACC_HEAD + D * D + D
    bad = _lib.make_config(**common.engine_kwargs(case_meta(dict(CASES["tiny_ragged"], n_classes=0))))
    assert lib.mmg_eval_acc_count(C.byref(bad)) < 0
    for name in ("tiny_ragged", "tiny_continuous"):
        c = CASES[name]
        meta = case_meta(c)
        x, target, desc = cpu_ref.synthetic_batch(c["batch"], c["n_classes"], meta["img_feat_dim"], meta["wv_dim"], seed=c["seed_data"])
        r = np_eval_reduce(oracle_tape(meta, x, target, desc, c["s_bias"]), target, c["top_k"], meta["fixed_exchange"])
        D, B, T, binary = c["n_classes"], c["batch"], meta["max_exchange"], bool(meta["use_binary"])
        acc = EvalAccumulator(D, c["top_k"])
        acc.acc = torch.from_numpy(np.concatenate([[r["hits"], 1, B, 0], r["conf"].reshape(-1), r["seen"]]).astype(np.int64))
        ham = np.concatenate([r["ham_sen"], r["ham_rec"]])
        row = np.concatenate([[r["n"]], ham.astype(np.int64) if binary else ham.view(np.int64)])
        acc.parts.append((B, 1, T, binary, torch.from_numpy(r["lens"].astype(np.int32)), torch.from_numpy(row.reshape(1, -1))))
        got = acc.fetch()
        assert (got["hits"], got["batches"], got["samples"]) == (r["hits"], 1, B)
        np.testing.assert_array_equal(got["conf"], r["conf"])
        np.testing.assert_array_equal(got["seen"], r["seen"])
        np.testing.assert_array_equal(got["lens"], r["lens"])
        assert got["n"].tolist() == [r["n"]] and got["sizes"].tolist() == [B]
        assert got["ham_sen"][0] == r["ham_sen"][:r["n"]].sum() / (float(B) * r["n"])
        assert got["ham_rec"][0] == r["ham_rec"][:r["n"]].sum() / (float(B) * r["n"])
    empty = EvalAccumulator(3, 2).fetch()
    assert empty["hits"] == 0 and empty["conf"].shape == (3, 3) and empty["lens"].size == 0


def test_numpy_restatement_reproduces_g8_eval_dev():
    """The reference's eval_dev on two dev batches, the second one short (tests/golden/make_golden_host.py): accuracy with the
    nominal batch size in the denominator, conversation lengths, Hamming means, sklearn's confusion matrix."""
    z, meta = common.load_golden("g8_eval_dev")
    B, D = int(z["batch"]), int(z["n_classes"])
    sizes = [int(v) for v in z["sizes"]]
    x0, _, desc = cpu_ref.synthetic_batch(sizes[0], D, meta["img_feat_dim"], meta["wv_dim"], seed=int(z["seed_data"]))
    x1, _, _ = cpu_ref.synthetic_batch(sizes[1], D, meta["img_feat_dim"], meta["wv_dim"], seed=int(z["seed_data"]) + 1)
    hits, conf, seen, lens, hs, hr = 0, 0, 0, [], [], []
    for x, t in ((x0, z["target0"]), (x1, z["target1"])):
        r = np_eval_reduce(oracle_tape(dict(meta, batch=len(x)), x, t.astype(np.int64), desc, float(z["s_bias"])), t.astype(np.int64), 2, False)
        k_gap, a_gap = gaps(r["sel"], 2)
        assert k_gap.min() > MIN_GAP and a_gap.min() > MIN_GAP
        hits, conf, seen = hits + r["hits"], conf + r["conf"], seen + r["seen"]
        lens.append(r["lens"])
        hs.append(r["ham_sen"][:r["n"]].sum() / (len(x) * r["n"])); hr.append(r["ham_rec"][:r["n"]].sum() / (len(x) * r["n"]))
    assert hits / (2.0 * B) == pytest.approx(float(z["accuracy"]), abs=1e-12)
    cl = np.concatenate(lens).astype(np.float64)
    assert cl.mean() == pytest.approx(float(z["conversation_lengths_mean"]), abs=1e-9)
    assert cl.std() == pytest.approx(float(z["conversation_lengths_std"]), abs=1e-9)
    assert np.mean(hs) == pytest.approx(float(z["hamming_sen_mean"]), abs=1e-6)
    assert np.mean(hr) == pytest.approx(float(z["hamming_rec_mean"]), abs=1e-6)
    occ = np.nonzero(seen > 0)[0]
    np.testing.assert_array_equal(conf[np.ix_(occ, occ)], z["conf_mat"])


def test_numpy_restatement_reproduces_g4_eval_c1():
    """Config 1's agents, early break at step 4 of 10: step count, per-sample hits, conversation lengths and the confusion
    counts of the reference's own log-probabilities."""
    z, meta = common.load_golden("g4_eval_c1")
    x, target, desc = cpu_ref.synthetic_batch(meta["batch"], meta["n_classes"], 512, 100, seed=meta["seed_data"])
    r = np_eval_reduce(oracle_tape(meta, x, target, desc, 1.2), target, 6, False)
    assert r["n"] == int(z["n_steps"]) and r["hits"] == int(z["hits"])
    np.testing.assert_array_equal(r["hit"], (z["top_k_ind"] == target.reshape(-1, 1)).any(1))
    np.testing.assert_array_equal(r["lens"], z["conversation_lengths"].astype(np.int64))
    want = np.zeros_like(r["conf"])
    np.add.at(want, (target, z["dist"].argmax(1)), 1)
    np.testing.assert_array_equal(r["conf"], want)
    assert r["hits"] / float(meta["batch"]) == pytest.approx(int(z["hits"]) / float(meta["batch"]), abs=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_cases_have_clear_gaps(name):
    """Every sample of every GPU case: the oracle's logits at the output step are more than 1e-4 apart at the top-k boundary and
    at the argmax (two correct fp32 implementations agree to ~1e-5 there), so no sample needs to be excluded."""
    c = CASES[name]
    meta = case_meta(c)
    x, target, desc = cpu_ref.synthetic_batch(c["batch"], c["n_classes"], meta["img_feat_dim"], meta["wv_dim"], seed=c["seed_data"])
    r = np_eval_reduce(oracle_tape(meta, x, target, desc, c["s_bias"]), target, c["top_k"], meta["fixed_exchange"])
    k_gap, a_gap = gaps(r["sel"], c["top_k"])
    assert k_gap.min() > MIN_GAP and a_gap.min() > MIN_GAP, (float(k_gap.min()), float(a_gap.min()))
    T = meta["max_exchange"]
    if name == "tiny_all_stop":
        assert r["n"] == 1
    if name in ("tiny_never_stop", "tiny_fixed"):
        assert r["n"] == T and (r["tsel"] == T - 1).all()
    if name == "tiny_ragged":
        assert 1 < r["n"] <= T and len(set(r["tsel"].tolist())) > 1, "the ragged case should select different output steps"
    if name == "tiny_topk_ge_D":
        assert r["hits"] == c["batch"]
    if name in ("c1_cont_B64", "D130_cont_B17"):
        assert not meta["use_binary"] and not meta["fixed_exchange"]
        assert 2 < r["n"] <= T and len(set(r["tsel"].tolist())) >= 3, "continuous + Adaptive: the output steps should spread over three values and more"
