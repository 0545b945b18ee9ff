"""k_wgrad's prologue (job lookup, live-row list through registers, job record by value) and tail (early parameter / state
requests, agent index from the job record) at the shapes where that code takes another path.

Gates exactly as tests/test_hip_wgrad.py applies them: (a) every job of the weight-gradient table against float64 fed with the
GPU's own operands, within n_chain * 2^-24 * sum |a b| (with the left-out-row control (b) that comes with it), and (c) the
post-update parameters / optimizer state from the GPU's own gradients.  Nothing here is looser; the helpers are imported.

What the cases are for (kernels_bwd.h: k_wgrad, "prologue"):
  * the live-row list is read by a compile-time number of clamped loads per thread -- 3 up to T B = 768, 8 up to 2 048 -- and
    written to LDS only after the first operand chunk was requested.  With B >= 64 that chunk is rows 0..63 of the list
    whatever the list holds, so the number of live rows decides what is left for the chunks behind the barrier:
        64 live rows    exactly one chunk, nothing behind it          65      one row in chunk 1
        128 / 129       the chunk boundary                            640     ten chunks, the prefetch ring wraps
    The count is designed through the stop uniforms (tests/common.py: u_s = 0.0 continues, 0.999999 stops) and asserted from
    tape["tstar"] before anything is gated.
  * B = 16 / 48 (T B = 160 / 480): threads beyond the list clamp to its last entry; B < 64, so chunk 0 is fetched behind the
    barrier too.
  * B = 200 (T B = 2 000, 1 792 < T B <= 2 048): the eight-load variant and its clamped tail.
  * a Fixed-exchange shard (config 3, B = 64): k_wgrad<true> with every row live, behind the role launches instead of k_game.
  * a VJP weight-gradient call: no live-row list at all (rmap == NULL), compared as tests/test_autograd_gpu.py compares."""
import numpy as np
import pytest
import torch

from tests import common, wgrad_ref
from tests import test_autograd_gpu as ag
from tests.test_hip_configs import C1, _meta
from tests.test_hip_wgrad import _check_update, _fetch, _gate, _run, _state, _variant

pytestmark = pytest.mark.gpu

G2 = "g2_adaptive_c1"          # config-2 dimensions, B = 64, T = 10
G3 = "g3_fixed_c3shard"        # config 3's shard, B = 64, Fixed


def _stops(T, B, live):
    """u_s [T, B, 1] under which exactly `live` (step, sample) rows are live: every sample is live at t = 0; sample b goes on to
    step t + 1 iff u_s[t, b] = 0.0.  The rows are handed out step by step, samples in order."""
    assert B <= live <= T * B
    tstar = np.zeros(B, int)
    left = live - B
    for t in range(1, T):
        n = min(B, left)
        tstar[:n] = t
        left -= n
    assert left == 0
    u_s = np.full((T, B, 1), 0.0, np.float32)
    for b in range(B):
        u_s[tstar[b]:, b, 0] = 0.999999
    return u_s, tstar


def _one_minibatch(label, meta, name, modes, live_count=None, expect_names=None):
    """`modes` minibatches on one engine, each through (a) (b) (c); live_count: the designed number of live rows of the fused ones."""
    eng = common.make_engine(meta)
    d = wgrad_ref.dims_of(eng.cfg)
    jobs = None
    worst = 0.0
    for i, mode in enumerate(modes):
        x, target, desc, u = common.case_inputs(meta, i, name)
        if live_count is not None and mode == "fused":
            u_s, want_tstar = _stops(d["T"], d["B"], live_count)
            u = (u[0], u_s, u[2])
        before = _state(eng)
        names = _run(eng, mode, x, target, desc, u)
        tape, grads = _fetch(eng)
        after = _state(eng)
        if jobs is None:
            jobs = wgrad_ref.build_jobs(d, eng.param_entries, _variant(d, names))
        live = wgrad_ref.live_rows(d, tape["tstar"])
        if live_count is not None and mode == "fused":
            assert int(live.sum()) == live_count, "%s: %d live rows, designed %d (tstar %s)" % (label, int(live.sum()), live_count, tape["tstar"])
            assert np.array_equal(np.asarray(tape["tstar"]).reshape(-1), want_tstar), (label, tape["tstar"])
        if mode == "fused" and expect_names is not None:
            assert names == expect_names, (label, names)
        env = wgrad_ref.make_env(d, tape, x, desc, before[0])
        w, _, _ = _gate(jobs, d, env, live, grads, "%s mb%d (%s)" % (label, i, mode))
        worst = max(worst, w)
        _check_update(eng, d, before, grads, after, names, "%s mb%d" % (label, i), i + 1, meta)
    print("\n%s: worst |got - ref| / bound %.3f" % (label, worst))


@pytest.mark.parametrize("live", [64, 65, 128, 129, 640])
def test_wgrad_fused_config2_designed_live_rows(live):
    _, meta = common.load_golden(G2)
    _one_minibatch("g2-live%d" % live, meta, G2, ["fused"], live_count=live, expect_names=["k_game", "k_wgrad"])


@pytest.mark.parametrize("batch", [16, 48])
def test_wgrad_fused_short_list_below_one_chunk_per_step(batch):
    _one_minibatch("c1-b%d" % batch, _meta(dict(C1, batch_size=batch), 30, batch, 2), None, ["fused", "fused"])


def test_wgrad_fused_long_list_eight_loads():
    _one_minibatch("c1-b200", _meta(dict(C1, batch_size=200), 30, 200, 1), None, ["fused"])


def test_wgrad_fused_fixed_shard_all_rows_live():
    _, meta = common.load_golden(G3)
    _one_minibatch("g3-fixed-shard", meta, G3, ["fused"])


def test_wgrad_vjp_call_without_row_list():
    """exchange() backward: four k_wgrad launches over the VJP job tables (no live-row list, no spare block), against the engine's
    own run-all backward -- the comparison of test_autograd_gpu.test_reference_block_gives_the_engine_gradients."""
    _, meta = common.load_golden(G2)
    fl = common.flags_from_meta(meta)
    game, eng = ag._game(meta, autograd=True)
    _, target, _, args = ag._inputs(meta, 0, G2)
    out = ag._exchange(game, fl, args)
    losses = ag._reference_losses(fl, out, torch.from_numpy(target))
    ag._zero(game)
    for a in ag.AGENTS:
        losses[a].backward()
    got = ag._grads(game, ag.AGENTS)
    eng.forward(args["data"], args["target"], args["desc"], *args["uniforms"], train=True, run_all=True)
    eng.loss_stats()
    eng.backward(args["data"], args["target"], args["desc"])
    torch.cuda.synchronize()
    want = {a: {k: v.detach().cpu().clone() for k, v in eng.grads[a].items()} for a in ag.AGENTS}
    ag._assert_close(got, want, "vjp-g2")
