"""k_game_fast's baseline roles against the launches the window arithmetic never touched.

Each case takes ONE training step on an engine that runs k_game_fast (its baseline roles build their row lists from a reciprocal
of the slot count and carry the sample index in the list entry: csrc/game_windows.h) and one on an engine created with
MMG_NO_ROLES=1 (k_baselines3 and k_stats: no windows, no slots), from the same parameters, inputs, seed and counters, and
compares what the baseline roles and the statistics chain behind them produce, over the LIVE (step, sample) rows (t <= t*; the
other rows are never written by either path):

  bit-equal (they are on the commit before the reciprocal too, in every case below): tape["tstar"]; the receiver baseline's
  hidden tape tape["hid_r"] and scores tape["br"] (the same MFMA fragments over the same rows, the same per-block partial sums
  added in the same order); tape["losses"][6:] (executed steps, hits).
  rtol = atol = 2e-5, the tolerance of test_hip_safety.py::test_no_roles_path_matches_the_role_launches: the sender baseline's
  hidden tape tape["hid_s"] and scores tape["bs"] (its h_x part, basehx, is accumulated by a different kernel on each path: the
  two differ by up to 1.7e-6 and 7.2e-7 on that commit), and tape["losses"][:6] (reduced in a different order: up to 7.6e-6).

Cases: B = 5 / 37 / 64, T = 2 / 10 / 15, D = 30 / 7 (k_game_fast<32>); nobody stops (B = 64, T = 10: 640 live rows = 40 windows,
every role pipelines two or three); everybody stops at step 0 (live rows = B: one partial window, and the forward loop's first
step is its only one); mixed stopping; a cu_budget that keeps the fused launch with fewer baseline roles (a slot count that is
no power of two); injected uniforms.  The stop head's bit is 1 = "go on" (model.py:852: the mask is the running minimum of the
bits), so a bias of +20 keeps every conversation running and -20 ends every one at step 0; each case asserts the live rows it is
meant to produce."""
import os
import re

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _meta(B=64, T=10, D=30):
    _, meta = common.load_golden("g2_adaptive_c1")
    meta = dict(meta)
    meta["batch"], meta["max_exchange"], meta["n_classes"] = B, T, D
    return meta


def _stop_bias(v):
    def tweak(sd):
        sd["receiver"]["s.bias"][...] = v
    return tweak


def _engines(meta, tweak=None, **over):
    eng = common.make_engine(meta, tweak, **over)
    os.environ["MMG_NO_ROLES"] = "1"
    try:
        ref = common.make_engine(meta, tweak, **over)
    finally:
        del os.environ["MMG_NO_ROLES"]
    assert eng.degraded() == 0 and ref.degraded() == 1
    return eng, ref


def _slots(eng):
    m = re.search(r"game_ok (\d) game_nbas (\d+)", eng.plan_text())
    npb = (eng.cfg.bas_hidden + 63) // 64
    per = 2 * npb // (2 if npb % 2 == 0 else 1)                       # baseline roles per window slot (host_select.h)
    return (int(m.group(2)) // per) if int(m.group(1)) else 0


def _step_and_compare(meta, eng, ref, uniforms=False, seed=11):
    x, target, desc, (u_z, u_s, u_w) = common.case_inputs(meta, 0)
    dev = eng.device
    xd, td, dd = [torch.from_numpy(a).to(dev) for a in (x, target, desc)]
    u = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u_z, u_s[..., 0], u_w)] if uniforms else []
    for e in (eng, ref):
        e.set_profiling(True)
        e.train_step(xd, td, dd, *u, seed=seed)
    torch.cuda.synchronize()
    eng.check_sync(); ref.check_sync()
    assert "k_game" in [n for n, _ in eng.kernel_times()]
    names = [n for n, _ in ref.kernel_times()]
    assert "k_game" not in names and "k_opt" in names, names
    a, b = [{k: e.tape[k].cpu() for k in ("tstar", "hid_r", "hid_s", "br", "bs", "losses")} for e in (eng, ref)]
    T, B = int(meta["max_exchange"]), int(meta["batch"])
    tstar = a["tstar"].long()
    live = torch.arange(T).view(T, 1) <= tstar.view(1, B)             # [T, B]
    figures = {"tstar": float((a["tstar"] != b["tstar"]).sum())}
    for k in ("hid_r", "hid_s", "br", "bs"):
        figures[k] = float((a[k][live] - b[k][live]).abs().max())
    figures["losses[6:]"] = float((a["losses"][6:] - b["losses"][6:]).abs().max())
    figures["losses[:6]"] = float((a["losses"][:6] - b["losses"][:6]).abs().max())
    print("live rows %d, slots %d; largest differences: %s" % (int(live.sum()), _slots(eng), figures))
    assert torch.equal(a["tstar"], b["tstar"])
    for k in ("hid_r", "br"):
        assert torch.equal(a[k][live], b[k][live]), k
    for k in ("hid_s", "bs"):
        torch.testing.assert_close(a[k][live], b[k][live], rtol=TOL, atol=TOL)
    assert torch.equal(a["losses"][6:], b["losses"][6:])
    torch.testing.assert_close(a["losses"][:6], b["losses"][:6], rtol=TOL, atol=TOL)
    return tstar, int(live.sum())


@pytest.mark.parametrize("B,T,D", [(5, 10, 30), (37, 10, 30), (64, 2, 30), (64, 15, 30), (64, 10, 7)],
                         ids=["B5", "B37", "T2", "T15", "D7"])
def test_shapes(B, T, D):
    meta = _meta(B, T, D)
    _step_and_compare(meta, *_engines(meta))


def test_mixed_stopping():
    meta = _meta()
    tstar, rows = _step_and_compare(meta, *_engines(meta))
    assert int(tstar.min()) < int(tstar.max()) and 64 < rows < 640


def test_nobody_stops():
    meta = _meta()
    eng, ref = _engines(meta, _stop_bias(20.0))
    tstar, rows = _step_and_compare(meta, eng, ref)
    slots = _slots(eng)
    assert rows == 640 and int(tstar.min()) == 9                     # 40 windows
    assert 40 // slots >= 2 and -(-40 // slots) <= 3, slots          # every role: two or three of them


def test_everybody_stops_at_step_0():
    meta = _meta()
    tstar, rows = _step_and_compare(meta, *_engines(meta, _stop_bias(-20.0)))
    assert rows == 64 and int(tstar.max()) == 0


def test_partial_last_window_when_everybody_stops():
    meta = _meta(B=37)
    tstar, rows = _step_and_compare(meta, *_engines(meta, _stop_bias(-20.0)))
    assert rows == 37 and int(tstar.max()) == 0                      # two full windows and five rows of a third


def test_fewer_baseline_roles_under_a_cu_budget():
    meta = _meta()
    full = _slots(common.make_engine(meta))
    for cu in (208, 192, 176, 224, 240):
        eng, ref = _engines(meta, _stop_bias(20.0), cu_budget=cu)
        slots = _slots(eng)
        if 0 < slots < full and slots & (slots - 1):
            break
    else:
        pytest.skip("no cu_budget of 176..240 keeps k_game_fast with a slot count below %d that is no power of two" % full)
    tstar, rows = _step_and_compare(meta, eng, ref)
    assert rows == 640


def test_injected_uniforms():
    meta = _meta()
    tstar, rows = _step_and_compare(meta, *_engines(meta), uniforms=True)
    assert int(tstar.min()) < int(tstar.max())
