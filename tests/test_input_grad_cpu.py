"""Input gradients (d data, d desc): what exists without a GPU.

1. The entry point is declared, exported and bound (include/mmg.h, _lib.SYMBOLS, libmmg.so), the ABI version stays 3, and the
   Python opt-in exists and is off by default.
2. The tape table lists the two new arrays (vsm, vdq) and stays consistent (tests/test_abi.py's checks).
3. The float64 reference (tests/channel_ref.py::f64_outputs) propagates to float64 leaves x and desc, and what it returns is the
   derivative of the function it computes: central finite differences with the `frozen` constants (dbar and the ReLU sides
   recorded on the first call), channel off and on with continuous messages, channel off with binary ones.  This is the
   reference's self-check: it runs test-side code only, so it is the one test here that does not need the feature.  Without
   `frozen`, d desc gains the term through dbar = softmax(y).detach() . desc and d x stays put.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import channel_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(batch_size=3, img_feat_dim=8, img_h_dim=6, rec_w_dim=4, sender_out_dim=4, rec_hidden=5, wv_dim=6,
            baseline_hid_dim=7, max_exchange=3, fixed_exchange=True)
N_CLASSES = 3


# ------------------------------------------------------------------ 1. the boundary
def test_input_grads_entry_is_declared_exported_and_bound():
    from multimodalgame_amd import _lib
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    m = re.search(r"int\s+mmg_vjp_input_grads\s*\(([^)]*)\)", header)
    assert m, "include/mmg.h does not declare mmg_vjp_input_grads"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 7
    assert "mmg_vjp_input_grads" in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.mmg_vjp_input_grads.argtypes) == 7
    assert lib.mmg_version() == 3
    # a NULL handle is an error of its own, before anything touches a device
    assert lib.mmg_vjp_input_grads(None, 0, 1, None, None, None, None) < 0
    assert b"NULL handle" in lib.mmg_last_error()


def test_input_grad_is_an_option_of_the_opt_in():
    from multimodalgame_amd import agents, game
    from multimodalgame_amd.engine import Engine
    sig = inspect.signature(game.Game.__init__).parameters
    assert sig["input_grad"].default is False and sig["autograd"].default is False and sig["channel_grad"].default is False
    assert callable(Engine.input_grads)
    for fn in (game._SenderVJP, game._ReceiverVJP, game._ChannelVJP):          # (spec, data, desc, *params)
        assert list(inspect.signature(fn.forward).parameters)[1:4] == ["spec", "data", "desc"]
    assert "desc_in" in inspect.signature(agents._ReceiverCall.forward).parameters


# ------------------------------------------------------------------ 2. the tape table
def test_tape_table_lists_the_new_arrays_and_stays_consistent():
    from multimodalgame_amd import _lib
    B, D, V, T = 64, 30, 100, 10
    cfg = _lib.make_config(B, D, 512, 256, 32, 64, V, 500, T, fixed_exchange=False)
    tab = _lib.tape_table(cfg)
    names = [e["name"] for e in tab]
    assert len(set(names)) == len(names)
    by = {e["name"]: e for e in tab}
    assert list(by["vsm"]["dims"][:3]) == [T, B, 2] and by["vsm"]["dtype"] == 0
    assert list(by["vdq"]["dims"][:3]) == [T, B, V] and by["vdq"]["dtype"] == 0
    for k in ("vdhx", "vdC", "vdgpre", "y"):                   # what the entry reads besides them
        assert k in by
    end = 0
    for e in tab:
        assert e["offset"] >= end and e["offset"] % 256 == 0
        end = e["offset"]
    assert _lib.load().mmg_workspace_bytes(C.byref(cfg)) > end
    order = sorted(tab, key=lambda e: e["offset"])
    for a, b in zip(order, order[1:]):                         # no array overlaps the next one
        numel = int(np.prod([int(d) for d in a["dims"]]))
        assert a["offset"] + numel * (4, 1, 4, 8)[a["dtype"]] <= b["offset"], (a["name"], b["name"])


# ------------------------------------------------------------------ 3. the float64 reference checks itself
def _case(use_binary, seed=11):
    fl = cpu_ref.Flags(**dict(TINY, use_binary=use_binary))
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=seed)
    models = {k: m.double() for k, m in models.items()}
    x, target, desc = cpu_ref.synthetic_batch(fl.batch_size, N_CLASSES, fl.img_feat_dim, fl.wv_dim, seed=seed + 1)
    tp = channel_ref.cpu_tape(models, fl, x, desc, fl.max_exchange, seed=seed + 2)
    return fl, models, torch.from_numpy(x).double(), torch.from_numpy(desc).double(), tp


def _functional(outs, seed=99):
    """A random linear functional of the sender's and the receiver's outputs.  The baselines' scores stay out: they read h_x and
    the GRU state DETACHED (model.py:835-843), so their dependence on x is cut on purpose and differences would see it."""
    rs = np.random.RandomState(seed)
    keys = [k for k in ("sen", "y", "ps", "w") if outs[k]]
    coef = {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in outs[k]] for k in keys}
    return sum((c * v).sum() for k in keys for c, v in zip(coef[k], outs[k]))


# (binary messages with the channel on are the straight-through estimator: the forward value of z = pz + (bits - pz).detach() is
# the constant bits, so differences of the function see no channel at all -- not a derivative, by construction)
@pytest.mark.parametrize("use_binary,channel", [(False, False), (False, True), (True, False)])
def test_reference_input_gradients_match_finite_differences(use_binary, channel):
    fl, models, x, desc, tp = _case(use_binary)
    n = fl.max_exchange
    frozen = {}
    f = lambda xx, dd: _functional(channel_ref.f64_outputs(models, fl, xx, dd, tp, n, channel=channel, frozen=frozen))
    f(x, desc)                                                  # records the constants: dbar and the ReLU sides
    xl, dl = x.clone().requires_grad_(True), desc.clone().requires_grad_(True)
    gx, gd = torch.autograd.grad(f(xl, dl), (xl, dl))
    assert float(gx.abs().max()) > 0 and float(gd.abs().max()) > 0
    eps = 1e-6
    with torch.no_grad():
        for leaf, g, other in ((x, gx, "x"), (desc, gd, "desc")):
            fd = torch.zeros_like(leaf)
            for i in range(leaf.numel()):
                hi, lo = leaf.clone(), leaf.clone()
                hi.view(-1)[i] += eps
                lo.view(-1)[i] -= eps
                fd.view(-1)[i] = (f(hi, desc) - f(lo, desc) if other == "x" else f(x, hi) - f(x, lo)) / (2 * eps)
            err = float((fd - g).abs().max())
            print("%s channel=%s d %s: max|g| %.3e max |fd - g| %.3e" % ("binary" if use_binary else "continuous", channel, other,
                                                                         float(g.abs().max()), err))
            # central differences in float64: truncation ~ eps^2 f''' and rounding ~ 1e-16 |f| / eps, both far below 1e-6 max|g|
            assert err <= 1e-6 * max(1.0, float(g.abs().max()))
    # without the frozen constants desc also enters through dbar = softmax(y).detach() . desc; x does not
    xl2, dl2 = x.clone().requires_grad_(True), desc.clone().requires_grad_(True)
    gx2, gd2 = torch.autograd.grad(_functional(channel_ref.f64_outputs(models, fl, xl2, dl2, tp, n, channel=channel)), (xl2, dl2))
    assert float((gd2 - gd).abs().max()) > 1e-6 * float(gd.abs().max())
    assert float((gx2 - gx).abs().max()) <= 1e-9 * max(1.0, float(gx.abs().max()))
