"""k_wgrad and the clip + optimizer step against float64 restatements of the same operations, fed with the GPU's own
operands (tests/wgrad_ref.py), per job of the weight-gradient table and per minibatch.

The parity tests compare whole minibatches with the fp32 CPU oracle at atol 1e-4 + rtol 1e-3, which end-to-end drift
(ReLU masks, RMSprop) requires.  That gate cannot see one (step, sample) row dropped or summed twice: at 5 120 rows one row
moves an entry by ~2e-4 of its value.  Here trajectory noise is taken out -- the reference reads the very tape k_wgrad read
-- so each entry is gated at fp32 rounding:

    (a) |got - ref64| <= n_chain * 2^-24 * sum_r |a_r b_r| + 1e-30

n_chain bounds the number of dependent fp32 roundings on the way of any one product into its output element
(kernels_bwd.h: k_wgrad).  With it the bound is the standard worst-case bound of a floating-point sum (every product is
rounded at most n_chain times, each time by a relative 2^-24), so it cannot flake:
  * GEMM jobs: rows in chunks of 64; wave w multiplies rows 16w..16w+15 of each chunk by four mfma_f32_16x16x4, i.e. 16
    accumulations per chunk into the same accumulator (counted as 4 dependent adds per MFMA, whatever its internal order);
    ceil(ceil(rows / 64) / nsplit) chunks per row slice; the four waves' tiles are added as (w0 + w1) + (w2 + w3): +2; the
    last slice to arrive adds nsplit partial tiles in slice order: +nsplit; the product itself: +1; the virtual operand of the
    baselines (d score * linear2.weight formed in fp32): +1.
        n_chain = 16 * ceil(ceil(rows / 64) / nsplit) + 2 + nsplit + 1 (+1)
  * column jobs: a thread accumulates every 64th row (float4 path, alternating two accumulators) or every 256 / P-th row in four
    accumulators (scalar path), then (a0 + a1) + (a2 + a3), a butterfly of <= 6 shuffles, <= 64 row groups added in order, the
    scale factor and the product (fma / virtual): bounded by ceil(rows / 64) + 64 + 12.
  * the code_bias job of the register-resident path (one workgroup): u[h] = sum_b dpre[0, b, h] in four accumulators
    (ceil(B / 4) + 2), then 32 fmas per lane (H = 256) and a group-of-8 DPP sum (+3), the scale and slack: ceil(B / 4) + 2 +
    max(32, H / 8) + 3 + 2, against sum_h |W_c[h, j]| sum_b |dpre[0, b, h]|.
rows is T * B for (step, sample)-row jobs (the live-row list, where used, only shortens the chain).

    (b) negative controls on the same data: the gate must FAIL against the reference with one live row left out, and -- after
        an earlier run-all minibatch wrote every row -- with one dead row's stale operands (that minibatch's tape) added.  The
        row is the one whose products stand out most against the bound (a row with all-zero products is invisible to any
        gate; jobs whose every row product is zero -- e.g. s.weight in Fixed mode -- are listed and must be exactly zero).
    (c) post-update parameters and optimizer state in float64 from the parameters / state before the step and the GPU's own
        gradients (per-agent clip_grad_norm(1) + torch.optim.RMSprop / Adam / SGD, oracle/cpu_ref.py), within 2 fp32 ulps of
        the parameter + 16 * 2^-24 + eps of the step (+ lr * 2^-20); eps = 1e-5 bounds the relative error of the GPU's fp32
        gradient norm when the clip is active.  k_wgrad<OPT> publishes its per-agent squared norms (tape coefll); they are
        checked against the float64 norms of the gradients within 1e-5.  Continuous mode: only the receiver moves, every
        other parameter and state entry is bit-identical.
    (d) shapes with row-split jobs: two engines with the same state and the same minibatch give bitwise-equal gradients (the
        slices are added in slice order whoever arrives last).  One run each; nothing is repeated.

Shapes (layout.h: wgrad_nsplit(TB, ptotal) = TB >= 4096 ? min(TB / 2048, 16) : 1, capped at 12000 / (ptotal / 512 + 64);
wgrad_job_nsplit raises jobs of <= 64 output tiles to min(TB / 320, 16) when TB > 2048 and mmg_create's table has <= 256
GEMM tiles without it; the bias columns run as K = 1 GEMMs when wgrad_nsplit > 1 or that small split is on):
  g2 fused / phased      T B = 640, ptotal 384 192: no split, fused -> k_game + k_wgrad<true> with the live-row list
  C1 B = 10 / 50         T B = 100 / 500: ragged 16-row tiles, baseline_sen's hx operand through row % B at B = 10, 50
  C1 Adaptive B = 256    T B = 2 560 > 2 048: no live-row list (dead rows zeroed by the backward kernels), wgrad_nsplit = 1,
                         gemm tiles > 256 -> no small split; a log minibatch (run-all) first, then two fused ones
  config 3 B = 512 Fixed T B = 5 120: wgrad_nsplit = 5120 / 2048 = 2 (cap 12000 / (750 + 64) = 14), bias_as_gemm
  C5 shard B = 256       T B = 2 560, continuous: receiver jobs only, 21 gemm tiles <= 256 -> small split, 2560 / 320 = 8
  C5 B = 2 048, T = 3    T B = 6 144: wgrad_nsplit = 3, small split min(6144 / 320, 16) = 16 on the receiver's jobs
  C4 / C4 at R = 256     tile / wide-receiver paths: code_bias from u0 (k_dhx), thousands of output tiles
  C1 D = 200, B = 40     many-class binary (k_conversation_mc, generic backward): dC / Py2 over 200 class rows, code_bias
                         from dc0
Walked tiles (wgrad_stride > 0, occupancy-dependent; 256 CUs): config 3 at B = 512 (856 workgroups walk 1 336 tiles) and
C4 (672 walk 3 848); see WGRAD_STRIDE below, checked against the engine's own plan text."""
import numpy as np
import pytest
import torch

from tests import common, wgrad_ref
from tests.test_hip_configs import C1, C4, C5, _meta

pytestmark = pytest.mark.gpu

TAPE_NAMES = ("dgi", "dgh", "z", "h", "dA", "hstar", "dC", "descc", "Py2", "dysum", "dgpre", "dbar", "dlw", "g", "dls", "dhx",
              "dpre", "c", "dsig", "u0", "dc0", "dlz", "a", "dbr", "hid_r", "dbs", "hid_s", "hx", "zr", "tstar")

# mmg_create's choice of walked GEMM tiles per shape on a 256-CU MI355X, the "wgrad_stride <s> (gemm tiles <n>)" of
# Engine.plan_text() -- g2, C1 at B = 10 / 50 / 256 and D = 200: 0 (760 tiles); config 3 at B = 512: 856 (1 336); C5 shard:
# 0 (504); C5 at B = 2 048: 0 (984); C4: 672 (3 848); C4 at R = 256: 0 (5 120, more than 6 tiles per slot).  A shape not
# listed walks no tiles.  _case asserts the value against the engine it runs.
WGRAD_STRIDE = {"c3-b512-fused": 856, "c3-b512-runall": 856, "c4-R64": 672}


def _plan_field(eng, name):
    words = eng.plan_text().split()
    return int(words[words.index(name) + 1])

REPORT = {}         # shape label -> worst |got - ref| / bound over its jobs (printed by the test)


def _fetch(eng):
    torch.cuda.synchronize()
    eng.check_sync()
    tape = {k: eng.tape[k].detach().cpu().numpy().copy() for k in TAPE_NAMES}
    grads = {a: {k: v.detach().cpu().numpy().copy() for k, v in d.items()} for a, d in eng.grads.items()}
    return tape, grads


def _state(eng):
    params = {a: {k: v.detach().cpu().numpy().copy() for k, v in d.items()} for a, d in eng.params.items()}
    st = eng.opt_state.detach().cpu().numpy().copy()
    n = eng.n_params
    state = {}
    for e in eng.param_entries:
        numel = e["rows"] * max(e["cols"], 1)
        shape = (e["rows"], e["cols"]) if e["cols"] else (e["rows"],)
        o = e["offset"]
        state.setdefault(e["agent"], {})[e["name"]] = (st[o:o + numel].reshape(shape), st[n + o:n + o + numel].reshape(shape))
    return params, state


def _run(eng, mode, x, target, desc, u):
    dev = eng.device
    xd, td, dd = (torch.from_numpy(v).to(dev) for v in (x, target, desc))
    uz, us, uw = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (u[0], u[1][..., 0], u[2]))
    eng.set_profiling(True)
    if mode == "fused":
        eng.train_step(xd, td, dd, uz, us, uw)
    else:          # "runall": exchange() tape (run_all_steps = 1); "log": a log minibatch (run_all_steps = 3, Game.train_step(full_tape))
        eng.forward(xd, td, dd, uz, us, uw, train=True, run_all=True, log_tape=(mode == "log"))
        eng.loss_stats()
        eng.backward(xd, td, dd)
        eng.clip_step()
    torch.cuda.synchronize()
    names = [n for n, _ in eng.kernel_times()]
    eng.set_profiling(False)
    return names


def _row_scores(Aabs, Babs, w):
    """Per row r: max over (n, k) of |A[r, n]| |Bm[r, k]| w[n, k] (in blocks of rows: [rows, N, K] would not fit)."""
    out = np.empty(Aabs.shape[0])
    step = max(1, (1 << 22) // max(1, w.size))
    for r0 in range(0, Aabs.shape[0], step):
        a, b = Aabs[r0:r0 + step], Babs[r0:r0 + step]
        out[r0:r0 + step] = (a[:, :, None] * b[:, None, :] * w[None]).reshape(a.shape[0], -1).max(1)
    return out


def _gate(jobs, d, env, live, grads, label, stale=None):
    """(a) + (b) for one minibatch.  Returns the worst ratio |got - ref| / bound."""
    TB = d["T"] * d["B"]
    worst, silent, dead_seen = 0.0, [], []
    for j in jobs:
        got = wgrad_ref.region_of(j, grads)
        ref, aps = wgrad_ref.evaluate(j, env, live)
        nc = wgrad_ref.n_chain(j, d, TB)
        bound = nc * wgrad_ref.U32 * aps + 1e-30
        err = np.abs(got - ref)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        i = int(np.argmax(err / bound))
        assert ratio <= 1.0, "%s: %s exceeds its rounding bound: |got - ref| %.3e > %.3e (n_chain %d, got %.6e, ref %.6e)" % (
            label, j.label, err.flat[i], bound.flat[i], nc, got.flat[i], ref.flat[i])
        if j.rows != "tb":
            continue
        # (b) one live row left out: the row whose products stand out most against the bound
        A, Bm, scale, Babs = j.ops(env)
        w = (np.ones(A.shape[1]) if scale is None else np.abs(scale))[:, None] / bound
        rowmax = _row_scores(np.abs(A), np.abs(Bm) if Babs is None else Babs, w)
        rowmax[~live] = -1.0
        if rowmax.max() <= 0.0:
            assert np.all(got == 0.0) and np.all(ref == 0.0), "%s: %s has no non-zero row product but a non-zero gradient" % (label, j.label)
            silent.append(j.label)
            continue
        r = int(rowmax.argmax())
        ref2, aps2 = wgrad_ref.evaluate(j, env, live, drop_row=r)
        assert np.any(np.abs(got - ref2) > nc * wgrad_ref.U32 * aps2 + 1e-30), \
            "%s: %s -- the gate does not see live row %d left out" % (label, j.label, r)
        if stale is None or live.all():
            continue
        # (b) one dead row's stale operands (an earlier run-all minibatch wrote them) added
        sA, sB, _, _ = j.ops(stale)
        score = _row_scores(np.abs(sA), np.abs(sB), w)
        score[live] = -1.0
        if score.max() <= 0.0:
            continue                                   # the earlier minibatch left this job's dead rows zero as well
        r2 = int(score.argmax())
        ref3, aps3 = wgrad_ref.evaluate(j, env, live, extra_rows=(sA[r2:r2 + 1], sB[r2:r2 + 1]))
        assert np.any(np.abs(got - ref3) > nc * wgrad_ref.U32 * aps3 + 1e-30), \
            "%s: %s -- the gate does not see dead row %d's stale operands summed in" % (label, j.label, r2)
        dead_seen.append(j.label)
    return worst, silent, dead_seen


def _check_update(eng, d, before, grads, after, names, label, step, meta):
    """(c): the post-update parameters / optimizer state from the GPU's own gradients."""
    params0, state0 = before
    params1, state1 = after
    agents = ("receiver", "sender", "baseline_rec", "baseline_sen") if d["binary"] else ("receiver",)
    lr = float(meta["learning_rate"])
    newp, news, norms = wgrad_ref.clip_and_step(params0, state0, grads, agents, meta["optim_type"], lr, step)
    eps = 1e-5
    for a in agents:
        clipped = norms[a] + 1e-6 > 1.0
        for k, p in newp[a].items():
            got = params1[a][k].astype(np.float64)
            dp = np.abs(p - params0[a][k])
            tol = 2 * np.spacing(np.abs(p).astype(np.float32)).astype(np.float64) + (16 * wgrad_ref.U32 + (eps if clipped else 0)) * dp + lr * 2.0 ** -20
            bad = np.abs(got - p) > tol
            assert not bad.any(), "%s: %s.%s updated parameter off by %.3e (tol %.3e)" % (
                label, a, k, float(np.abs(got - p)[bad].max()), float(tol[bad].min()))
            s = news[a][k][0]
            gs = state1[a][k][0].astype(np.float64)
            tol_s = (32 * wgrad_ref.U32 + (2 * eps if clipped else 0)) * np.abs(s) + 1e-37
            bad = np.abs(gs - s) > tol_s
            assert not bad.any(), "%s: %s.%s optimizer state off by %.3e" % (label, a, k, float(np.abs(gs - s)[bad].max()))
    if "k_opt" not in names and "k_gradnorm" not in names:          # k_wgrad<OPT>: the norm roles' published squared norms
        co = eng.tape["coefll"].detach().cpu().numpy()
        for i, a in enumerate(("receiver", "sender", "baseline_rec", "baseline_sen")):
            if a in norms:
                tot = float(co[2 * (4 * 64 + i)])
                assert abs(tot - norms[a] ** 2) <= eps * norms[a] ** 2, "%s: %s squared norm %.8e vs %.8e" % (label, a, tot, norms[a] ** 2)
    if not d["binary"]:
        for a in ("sender", "baseline_rec", "baseline_sen"):
            for k in params0[a]:
                assert np.array_equal(params1[a][k], params0[a][k]), (label, a, k)
                assert np.array_equal(state1[a][k][0], state0[a][k][0]) and np.array_equal(state1[a][k][1], state0[a][k][1]), (label, a, k)


def _variant(d, names):
    if wgrad_ref.fast_shape(d):
        return "fast"
    return "tile" if "k_bwd_tile" in names else "generic"


def _case(label, meta, modes, variant, expect_names=None, twin=False, name=None, over=None):
    """Runs the minibatches `modes` on one engine; every one through (a) (b) (c).  twin: (d) on the first minibatch."""
    eng = common.make_engine(meta, **(over or {}))
    assert _plan_field(eng, "wgrad_stride") == WGRAD_STRIDE.get(label, 0), (label, eng.plan_text())
    d = wgrad_ref.dims_of(eng.cfg)
    table = eng.param_entries
    jobs = wgrad_ref.build_jobs(d, table, variant)
    splits = sorted({j.nsplit for j in jobs})
    stale, worst, silent_all, dead_all = None, 0.0, set(), set()
    for i, mode in enumerate(modes):
        x, target, desc, u = common.case_inputs(meta, i, name)
        before = _state(eng)
        if twin and i == 0:
            eng2 = common.make_engine(meta, **(over or {}))
            _run(eng2, mode, x, target, desc, u)
        names = _run(eng, mode, x, target, desc, u)
        if twin and i == 0:
            assert max(splits) > 1, (label, splits)
            assert torch.equal(eng.flat_grads, eng2.flat_grads), "%s: row-split gradients differ between two identical runs" % label
            del eng2
        tape, grads = _fetch(eng)
        after = _state(eng)
        if d["binary"]:
            assert _variant(d, names) == variant, (label, variant, names)
        if mode == "fused" and expect_names is not None:
            assert names == expect_names, (label, names)
        live = wgrad_ref.live_rows(d, tape["tstar"])
        env = wgrad_ref.make_env(d, tape, x, desc, before[0])
        w, silent, dead = _gate(jobs, d, env, live, grads, "%s mb%d (%s)" % (label, i, mode), stale=stale)
        worst = max(worst, w)
        silent_all.update(silent)
        dead_all.update(dead)
        _check_update(eng, d, before, grads, after, names, "%s mb%d" % (label, i), i + 1, meta)
        if mode != "fused":
            stale = wgrad_ref.make_env(d, tape, x, desc, before[0])
    if stale is not None and not d["fixed"]:
        # every (step, sample)-row job with a non-zero product must have failed the dead-row control at least once
        tb_jobs = {j.label for j in jobs if j.rows == "tb"} - silent_all
        assert tb_jobs <= dead_all, "%s: no dead-row control for %s" % (label, sorted(tb_jobs - dead_all))
    REPORT[label] = worst
    print("\n%s: code_bias variant %s, row slices %s, small split %s, walked tiles %s, worst |got - ref| / bound %.3f, "
          "jobs without a non-zero row product: %s" % (label, variant, splits, jobs[0].small_split, WGRAD_STRIDE.get(label, 0),
                                                        worst, sorted(silent_all) or "none"))
    return eng


G2 = "g2_adaptive_c1"


def test_wgrad_config2_fused():
    _, meta = common.load_golden(G2)
    _case("g2-fused", meta, ["runall", "fused", "fused"], "fast", expect_names=["k_game", "k_wgrad"], name=G2)


def test_wgrad_config2_phased_run_all():
    _, meta = common.load_golden(G2)
    _case("g2-phased", meta, ["runall", "runall"], "fast", name=G2)


@pytest.mark.parametrize("batch", [10, 50])
def test_wgrad_ragged_batches_fused(batch):
    _case("c1-b%d" % batch, _meta(dict(C1, batch_size=batch), 30, batch, 3), ["runall", "fused", "fused"], "fast")


def test_wgrad_adaptive_without_row_list_after_log_minibatch():
    """T B = 2 560 > 2 048: k_wgrad walks all rows and relies on the backward kernels zeroing the dead ones.  The log
    minibatch (Game.train_step(full_tape=True): run_all_steps = 3) writes every row first; the two fused minibatches after it
    must not sum any of those stale rows (the dead-row control shows the gate would see one)."""
    _case("c1-b256-log-then-fused", _meta(dict(C1, batch_size=256), 30, 256, 3), ["log", "fused", "fused"], "fast")


@pytest.mark.parametrize("mode", ["fused", "runall"])
def test_wgrad_config3_fixed_b512_row_split(mode):
    kw = dict(use_binary=True, fixed_exchange=True, max_exchange=10, batch_size=512, learning_rate=1e-4, entropy_rec=0.01,
              entropy_sen=0.01, img_feat_dim=512, img_h_dim=256, rec_w_dim=32, sender_out_dim=32, rec_hidden=64, wv_dim=100,
              baseline_hid_dim=500, top_k_train=6)
    _case("c3-b512-" + mode, _meta(kw, 30, 512, 2), [mode, mode], "fast", twin=True)


def test_wgrad_config5_shard_small_split():
    _case("c5-b256", _meta(dict(C5, batch_size=256), 1000, 256, 2), ["fused", "fused"], "fast", twin=True)


def test_wgrad_config5_b2048_t3():
    _case("c5-b2048-t3", _meta(dict(C5, batch_size=2048, max_exchange=3), 1000, 2048, 1), ["fused"], "fast", twin=True)


@pytest.mark.parametrize("R", [64, 256])
def test_wgrad_config4_tile_paths(R):
    _case("c4-R%d" % R, _meta(dict(C4, rec_hidden=R, batch_size=64), 30, 64, 3), ["runall", "fused", "fused"], "tile")


def test_wgrad_many_class_binary():
    _case("c1-D200-b40", _meta(dict(C1, batch_size=40), 200, 40, 3), ["runall", "fused", "fused"], "generic")
