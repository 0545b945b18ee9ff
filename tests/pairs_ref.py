"""The pair histogram of a dev evaluation's codes (include/mmg.h: mmg_code_pair_hist; csrc/kernels_pairs.h) restated as brute-force
loops over the pairs in float64, the edge-pair bookkeeping that says where an fp32 cosine may land in another bin than the float64
one, synthetic codes, and the cases the CPU and the GPU tests share.

The one floating quantity is c = cos(x_i, x_j).  For unit-normalised fp32 rows, any summation order and fp32 inverse norms
  |c_gpu - c_f64| <= delta_c = 2 (F + 8) 2^-24
(the dot product contributes F u sum |a_k b_k| <= F u, the two norms F u / 2 + 2 u each, the final products 2 u; u = 2^-24).  With
u_f64 = (1 - c_f64) K / 2, a pair is an EDGE PAIR of edge e in 1 .. K - 1 iff |u_f64 - e| < delta_c K / 2: only such a pair may be
counted on the other side of e.  The clamped edges 0 and K are harmless.  EXACT cases have no edge pair (a condition on the inputs,
asserted on the CPU for the very seeds and shapes the GPU runs): the GPU histogram equals the float64 one entry for entry.  The
BOUNDED case has a few: its Hamming marginals are exact and every cumulative count over q may differ by no more than the edge pairs
of that (p, h, e)."""
import functools

import numpy as np

from multimodalgame_amd import commstats


def delta_c(F):
    return 2.0 * (F + 8) * 2.0 ** -24


def synthetic_codes(N, T, W, seed, n_classes=5, skip=(), single_class=False):
    """(codes [N, 2, T, Wp] uint32, meta [N, 2] int32): random bits at the live steps t <= tsel, zero behind them and in the padding
    bits; tsel uniform over the steps, targets uniform over the classes, -1 at the rows of `skip`."""
    rng = np.random.RandomState(seed)
    Wp = (W + 31) // 32
    tsel = rng.randint(0, T, N)
    bits = rng.randint(0, 2, (N, 2, T, Wp * 32)).astype(np.uint64)
    bits[..., W:] = 0
    bits *= (np.arange(T)[None, :] <= tsel[:, None]).astype(np.uint64)[:, None, :, None]
    codes = (bits.reshape(N, 2, T, Wp, 32) << np.arange(32, dtype=np.uint64)).sum(4).astype(np.uint32)
    target = np.zeros(N, np.int64) if single_class else rng.randint(0, n_classes, N)
    target[list(skip)] = -1
    return codes, np.stack([tsel, target], 1).astype(np.int32)


def features(N, F, seed):
    """|N(0, 1)| features, fp32."""
    return np.abs(np.random.RandomState(seed).randn(N, F)).astype(np.float32)


def class_meaning(meta, F, seed, n_classes=5):
    """desc[target] rows of a random |N(0, 1)| description matrix (rows of skipped samples: class 0)."""
    desc = features(n_classes, F, seed + 1000)
    return desc[np.clip(meta[:, 1], 0, n_classes - 1)]


def _pairs(codes, meta, meaning, agent, t0, t1):
    """Brute-force loops: yields (p, h, c_f64) of every unordered pair of used rows."""
    used = [i for i in range(len(meta)) if meta[i, 1] >= 0]
    x = np.asarray(meaning, np.float64)
    norm = np.sqrt((x * x).sum(1))
    sel = np.asarray(codes)[:, agent, t0:t1].reshape(len(meta), -1)
    for a, i in enumerate(used):
        for j in used[a + 1:]:
            h = sum(bin(int(u) ^ int(v)).count("1") for u, v in zip(sel[i], sel[j]))
            c = float(np.dot(x[i], x[j]) / (norm[i] * norm[j])) if norm[i] > 0 and norm[j] > 0 else 0.0
            yield int(meta[i, 1] == meta[j, 1]), h, c


def brute_pair_hist(codes, meta, meaning, agent, t0, t1, K, W):
    """(flat histogram, edge pairs [2, M + 1, K + 1]) by loops over the pairs; edges[p, h, e] counts the pairs of (p, h) within
    delta_c K / 2 of edge e, e = 1 .. K - 1."""
    M = (t1 - t0) * W
    F = np.asarray(meaning).shape[1]
    n_used = int((meta[:, 1] >= 0).sum())
    flat = np.zeros(commstats.pair_hist_count(t1 - t0, W, K), np.int64)
    flat[:3] = (n_used, len(meta) - n_used, n_used * (n_used - 1) // 2)
    hist = flat[4:].reshape(2, M + 1, K)
    edges = np.zeros((2, M + 1, K + 1), np.int64)
    tol = delta_c(F) * K / 2.0
    for p, h, c in _pairs(codes, meta, meaning, agent, t0, t1):
        u = (1.0 - c) * K / 2.0
        hist[p, h, min(K - 1, max(0, int(np.floor(u))))] += 1
        e = int(np.rint(u))
        if 1 <= e <= K - 1 and abs(u - e) < tol:
            edges[p, h, e] += 1
    return flat, edges


def assert_bounded(got_hist, ref_hist, edges):
    """got may differ from ref only by moving edge pairs across their own edge: equal Hamming marginals, and every cumulative count
    over q within the edge pairs of that (p, h, e)."""
    got_hist, ref_hist = np.asarray(got_hist), np.asarray(ref_hist)
    np.testing.assert_array_equal(got_hist.sum(2), ref_hist.sum(2), err_msg="Hamming marginals")
    K = got_hist.shape[2]
    cg, cr = got_hist.cumsum(2), ref_hist.cumsum(2)                    # cum[p, h, e - 1] = pairs below edge e
    diff = np.abs(cg - cr)[:, :, :K - 1]
    bad = diff > edges[:, :, 1:K]
    assert not bad.any(), "pairs moved across an edge they are not close to: %s" % (np.argwhere(bad)[:5].tolist(),)
    return int(diff.sum())


# name -> N, T, W, F, K, agent, steps (None: all), meaning ("feat": |N(0,1)| features, "class": desc[target] of 5 classes), seed,
# skip (rows with target -1), ld (row stride of the meaning matrix on the GPU; None: F), single (one class only)
def _case(N, T, W, F, K, agent=0, steps=None, meaning="class", seed=0, skip=(), ld=None, single=False):
    return dict(N=N, T=T, W=W, F=F, K=K, agent=agent, steps=steps, meaning=meaning, seed=seed, skip=tuple(skip), ld=ld, single=single)


EXACT_CASES = {
    # the three feature cases: no pair within delta_c K / 2 of an edge (tests/test_code_pairs_cpu.py asserts it)
    "feat_N65_F6_K16": _case(65, 1, 6, 6, 16, meaning="feat", seed=0),
    "feat_N64_F64_K16": _case(64, 10, 32, 64, 16, agent=1, steps=(3, 7), meaning="feat", seed=0),
    "feat_N130_F18_K64": _case(130, 10, 70, 18, 64, steps=(0, 1), meaning="feat", seed=2, skip=(5, 64, 129)),
    # class-level meanings: 15 distinct cosines, far from every edge
    "class_N1": _case(1, 1, 6, 6, 16),
    "class_N2": _case(2, 10, 32, 1, 1, agent=1),
    "class_N64_K1": _case(64, 1, 32, 18, 1, seed=3),
    "class_N65_W70": _case(65, 10, 70, 64, 64, agent=1, steps=(2, 9), seed=4, skip=(0, 63, 64)),
    "class_N130_ld": _case(130, 10, 6, 18, 16, seed=5, ld=24, skip=(7,)),
    "class_single": _case(65, 1, 32, 6, 16, seed=6, single=True),
    "class_N65_F1": _case(65, 10, 6, 1, 64, steps=(0, 1), seed=7),
    # 2 (M + 1) K counters do not fit the workgroup's LDS (W = 256, T = 10, K = 64: 1.3 MB): global atomics ...
    "class_global_route": _case(65, 10, 256, 6, 64, seed=8, skip=(3,)),
    # ... beside the same rows on the LDS route (step 0 alone, 16 bins: 33 KB of counters) ...
    "class_lds_route": _case(65, 10, 256, 6, 16, steps=(0, 1), seed=8, skip=(3,)),
    # ... a histogram beyond the 48 KB a launch gets by default, still in LDS (three steps of W = 32 at 64 bins: 50 KB) ...
    "class_lds_large": _case(65, 10, 32, 6, 64, steps=(0, 3), seed=9, skip=(11,)),
    # ... and code words that do not fit LDS (40 steps x 8 words x 128 rows = 160 KB): read from global memory, the histogram in LDS
    "class_codes_global": _case(65, 40, 256, 6, 1, agent=1, seed=10),
}
BOUNDED_CASE = _case(97, 10, 32, 512, 64, meaning="feat", seed=1)
BOUNDED_MAX_EDGE_SHARE = 0.02


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = dict(key)
    codes, meta = synthetic_codes(c["N"], c["T"], c["W"], c["seed"], skip=c["skip"], single_class=c["single"])
    x = features(c["N"], c["F"], c["seed"]) if c["meaning"] == "feat" else class_meaning(meta, c["F"], c["seed"])
    for a in (codes, meta, x):
        a.setflags(write=False)
    return codes, meta, x


def case_inputs(c):
    """(codes, meta, meaning, t0, t1) of a case -- computed once per process and left unchanged."""
    codes, meta, x = _inputs(tuple(sorted(c.items())))
    t0, t1 = (0, c["T"]) if c["steps"] is None else c["steps"]
    return codes, meta, x, t0, t1


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = dict(key)
    codes, meta, x, t0, t1 = case_inputs(c)
    flat = commstats.pair_hist_np(codes, meta, x, c["agent"], t0, t1, c["K"], W=c["W"])
    flat.setflags(write=False)
    return flat


def case_reference(c):
    """commstats.pair_hist_np of a case (float64 cosine), shared by the tests that need it."""
    return _reference(tuple(sorted(c.items())))


def expand_pairs(hist2d):
    """(h, q) of every pair of a joint histogram [M + 1, K], one entry per pair."""
    h, q = np.nonzero(hist2d)
    cnt = hist2d[h, q].astype(np.int64)
    return np.repeat(h, cnt), np.repeat(q, cnt)


# the end-to-end case of both test files: model.eval_dev(topsim=...) on the g8 game (tests/eval_profile_ref.py: g8_game), 70 samples in
# batches of 32 with a final 6, class-level meaning, 16 bins, receiver.s.weight x 30 so that the output steps differ
E2E_SIZES, E2E_BINS, E2E_S_SCALE = (32, 32, 6), 16, 30.0


def e2e_batches(D, feat_dim, wv_dim):
    from oracle import cpu_ref
    rng = np.random.RandomState(3)
    return [(cpu_ref.synthetic_batch(b, D, feat_dim, wv_dim, seed=40 + i)[0], rng.randint(0, D, b).astype(np.int64))
            for i, b in enumerate(E2E_SIZES)]


def class_edge_distance(desc, K):
    """(smallest distance of u_f64 = (1 - cos) K / 2 from an inner bin edge over all pairs of rows of desc, the edge-pair tolerance
    delta_c K / 2): a class-level meaning is an exact case iff the first exceeds the second."""
    d = np.asarray(desc, np.float64)
    dn = d / np.sqrt((d * d).sum(1, keepdims=True))
    u = (1.0 - dn @ dn.T) * K / 2.0
    e = np.rint(u)
    inner = (e >= 1) & (e <= K - 1)
    return (float(np.abs(u - e)[inner].min()) if inner.any() else float("inf")), delta_c(d.shape[1]) * K / 2.0
