"""The cases of tests/test_relaxed_channel_{cpu,gpu}.py: shapes, temperatures, seeds, and their float64 runs on the CPU
(tests/relaxed_ref.py), computed once per process and shared.

    odd      B 5, H 100, W 50, R 128, D 7, T 3, Fixed: no multiple of a wave; a plain handle runs k_conversation here too
    c1       config 1's agents at B 16, D 30, T 10, Adaptive: early stops, rows with t >= n
    w512     tests/generic_inst.py's H 260 / W 253 shape (T 3, B 5): the 512-thread instantiation, unaligned weight rows
The data / uniform seeds were searched on the CPU: tests/test_relaxed_channel_cpu.py asserts what they reach (every stop-bit draw
1e-4 away from its float64 probability, early stops at c1, a falling NLL over the SGD steps).
"""
import numpy as np
import torch

from oracle import cpu_ref
from tests import common, generic_inst, relaxed_ref
from tests.test_autograd_gpu import FAMILIES, _meta

_ODD = _meta(*FAMILIES["odd_generic"])
_C1 = _meta(*FAMILIES["fast_c2"])
_W512 = generic_inst.plain_meta("W512", "adaptive")

# case -> (meta, (tau_sen, tau_rec, hard))
CASES = {
    "odd_soft": (_ODD, (0.8, 1.25, False)),
    "odd_hard": (_ODD, (0.8, 1.25, True)),
    "c1_soft": (_C1, (0.7, 1.5, False)),
    "c1_hard": (_C1, (1.0, 1.0, True)),
    "w512_hard": (_W512, (0.9, 1.1, True)),
}
SGD_CASE, SGD_LR, SGD_STEPS = "c1_hard", 0.5, 3
PAIR = ("sender", "receiver")
_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def engine_kwargs(case):
    return common.engine_kwargs(CASES[case][0])


def inputs(case):
    """x, target, desc, (u_z, u_s, u_w) of the case's minibatch (numpy)."""
    return common.case_inputs(CASES[case][0], 0)


def f64_models(case):
    meta = CASES[case][0]
    models = cpu_ref.build_agents(common.flags_from_meta(meta))
    cpu_ref.load_filled(models, seed=meta["seed_weights"])
    return {k: m.double() for k, m in models.items()}


def cpu_conversation(case):
    """The case's relaxed conversation in float64 (relaxed_ref.conversation), every sample through all T steps."""
    def make():
        meta, relax = CASES[case]
        x, _, desc, u = inputs(case)
        return relaxed_ref.conversation(f64_models(case), common.flags_from_meta(meta), x, desc, u, relax)
    return once(("conversation", case), make)


def cpu_sgd_nll():
    """SGD_STEPS steps of plain SGD on the NLL of ONE minibatch of SGD_CASE in float64, the gradient through the relaxed messages:
    the NLL before the first step and after each one (the same uniforms every time)."""
    def make():
        meta, relax = CASES[SGD_CASE]
        fl = common.flags_from_meta(meta)
        x, target, desc, u = inputs(SGD_CASE)
        models = f64_models(SGD_CASE)
        opt = torch.optim.SGD([p for a in PAIR for p in models[a].parameters()], lr=SGD_LR)
        nll = []
        for i in range(SGD_STEPS + 1):
            tp = relaxed_ref.conversation(models, fl, x, desc, u, relax)
            n = relaxed_ref.executed_steps(tp["s"])
            out = relaxed_ref.f64_outputs(models, fl, x, desc, tp, n, relax, u)
            loss = relaxed_ref.output_nll(torch.stack(out["y"]), tp["s"][:n], target)
            nll.append(float(loss.detach()))
            if i < SGD_STEPS:
                opt.zero_grad()
                loss.backward()
                opt.step()
        return nll
    return once("sgd", make)


def to_numpy(t):
    return np.asarray(t.detach().cpu())
