"""The float64 reference of the differentiable channel (tests/channel_ref.py) checks itself; no GPU.

1. channel=False gives the per-agent gradients of the existing detached construction (tests/test_autograd_gpu.py::_f64_outputs)
   on one binary case.
2. torch.autograd.gradcheck in float64 on the continuous channel graph at tiny dims: nothing on the path between the agents is
   detached by accident.
3. Under a loss on y alone the sender's gradient is identically zero with channel=False and non-zero in every sender tensor,
   code_bias included, with channel=True (continuous and binary straight-through).
The entry point and the Python layer exist without a GPU (declared, exported, bound; the option is off by default).
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import cpu_ref
from tests import channel_ref
from tests.test_autograd_gpu import _f64_outputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(batch_size=3, img_feat_dim=8, img_h_dim=6, rec_w_dim=4, sender_out_dim=4, rec_hidden=5, wv_dim=6,
            baseline_hid_dim=7, max_exchange=3, fixed_exchange=True)
N_CLASSES = 3


def _case(use_binary, seed=11):
    fl = cpu_ref.Flags(**dict(TINY, use_binary=use_binary))
    models = cpu_ref.build_agents(fl)
    cpu_ref.load_filled(models, seed=seed)
    models = {k: m.double() for k, m in models.items()}
    x, target, desc = cpu_ref.synthetic_batch(fl.batch_size, N_CLASSES, fl.img_feat_dim, fl.wv_dim, seed=seed + 1)
    tp = channel_ref.cpu_tape(models, fl, x, desc, fl.max_exchange, seed=seed + 2)
    return fl, models, x, target, desc, tp


def _functional(outs, seed=99):
    rs = np.random.RandomState(seed)
    keys = [k for k in ("sen", "y", "ps", "w", "bs", "br") if outs[k]]
    coef = {k: [torch.from_numpy(rs.standard_normal(tuple(v.shape))) for v in outs[k]] for k in keys}
    return sum((c * v).sum() for k in keys for c, v in zip(coef[k], outs[k]))


def _zero(models):
    for m in models.values():
        m.zero_grad(set_to_none=True)


def test_channel_off_is_the_detached_construction():
    fl, models, x, target, desc, tp = _case(True)
    n = fl.max_exchange
    agents = ("sender", "receiver", "baseline_sen", "baseline_rec")
    _zero(models)
    _functional(channel_ref.f64_outputs(models, fl, x, desc, tp, n, channel=False)).backward()
    got = channel_ref.grads_of(models, agents)
    _zero(models)
    _functional(_f64_outputs(models, fl, x, desc, tp, n)).backward()
    want = channel_ref.grads_of(models, agents)
    for a in agents:
        for k in want[a]:
            assert torch.equal(got[a][k], want[a][k]), (a, k)
        assert any(float(v.abs().max()) > 0 for v in want[a].values()), a


class _Conversation(nn.Module):
    def __init__(self, models, fl, x, desc, tp, frozen):
        super().__init__()
        self.agents = nn.ModuleDict(models)
        self.fl, self.x, self.desc, self.tp, self.frozen = fl, x, desc, tp, frozen

    def forward(self):
        return _functional(channel_ref.f64_outputs(dict(self.agents.items()), self.fl, self.x, self.desc, self.tp,
                                                   self.fl.max_exchange, channel=True, frozen=self.frozen))


def test_gradcheck_of_the_continuous_channel_graph():
    fl, models, x, target, desc, tp = _case(False)
    frozen = {}
    conv = _Conversation(models, fl, x, desc, tp, frozen)
    conv()                                                      # records the constants: dbar and the ReLU sides
    names = [k for k, _ in conv.named_parameters() if k.split(".")[1] in channel_ref.CHANNEL_AGENTS]
    assert len(names) == 7 + 15
    params = tuple(p.detach().clone().requires_grad_(True) for k, p in conv.named_parameters() if k in names)

    def fn(*tensors):
        return torch.func.functional_call(conv, dict(zip(names, tensors)), ())

    assert torch.autograd.gradcheck(fn, params, eps=1e-6, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("use_binary", [False, True])
def test_loss_on_y_alone_reaches_the_sender_only_through_the_channel(use_binary):
    fl, models, x, target, desc, tp = _case(use_binary)
    n = fl.max_exchange
    for channel in (False, True):
        _zero(models)
        y = channel_ref.f64_outputs(models, fl, x, desc, tp, n, channel=channel)["y"]
        torch.nn.functional.nll_loss(torch.log_softmax(y[-1], dim=1), torch.from_numpy(target)).backward()
        g = channel_ref.grads_of(models)
        assert float(g["receiver"]["rnn.weight_ih"].abs().max()) > 0
        for k, v in g["sender"].items():
            if channel:
                assert float(v.abs().max()) > 0, k
            else:
                assert float(v.abs().max()) == 0, k
    assert "code_bias" in g["sender"]


def test_channel_entry_is_declared_exported_and_bound():
    from multimodalgame_amd import _lib
    header = open(os.path.join(REPO, "include", "mmg.h")).read()
    m = re.search(r"int\s+mmg_exchange_vjp_channel\s*\(([^)]*)\)", header)
    assert m, "include/mmg.h does not declare mmg_exchange_vjp_channel"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 9
    assert "mmg_exchange_vjp_channel" in _lib.SYMBOLS
    lib = _lib.load()
    assert len(lib.mmg_exchange_vjp_channel.argtypes) == 9
    assert lib.mmg_version() == 3


def test_channel_grad_is_an_option_of_the_opt_in():
    from multimodalgame_amd import game
    from multimodalgame_amd.engine import Engine
    sig = inspect.signature(game.Game.__init__).parameters
    assert sig["channel_grad"].default is False and sig["autograd"].default is False
    assert callable(Engine.vjp_channel)
    assert issubclass(game._ChannelVJP, torch.autograd.Function)
