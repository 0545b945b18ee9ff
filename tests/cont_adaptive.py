"""Continuous messages WITH Adaptive stopping (-nouse_binary -model_type Adaptive): shapes, seeds and predicates shared by
tests/test_cont_adaptive_cpu.py (the reach conditions, on the oracle alone) and tests/test_cont_adaptive_gpu.py (the kernels).

The reference treats `use_binary` and `fixed_exchange` as two independent flags: with continuous messages only the receiver is
trained, through the NLL (model.py:1297-1305), but the stop bit is still SAMPLED, the conversation ends as soon as every sample
has stopped (model.py:866) and `outp` is each sample's logits at its own stop step.  Every other training case of the suite with
use_binary = False also sets fixed_exchange = True.  No GPU import here."""
import numpy as np

from tests import common
from tests.test_hip_configs import C1, C4
from tests.test_option_branches_cpu import TINY, make_meta

SEEDS = (5, 6, 7)                       # (weights, data, uniforms) of every case
BASES = {"c1": C1, "tiny": TINY, "c4": C4, "c4-R256": dict(C4, rec_hidden=256)}

# case id -> base flags, classes D, batch B, max_exchange T, minibatches, environment switches read at mmg_create, modes, the key in
# test_option_branches_gpu.FAMILIES whose timing scopes the case must / must not show, float64 gate of the six losses (config 4's
# 256-bit agents, as every C4 case), `fixed` (the Fixed twin), and the oracle's executed steps per minibatch as measured on the CPU
# (test_cont_adaptive_cpu.py asserts them).
#   B = 40: three sample tiles, the last one ragged (8 samples).        D = 33: mc_per = 4 -- members 9..15 own no class, member 8 one.
#   D = 1024: mc_per = 64 = CAP -- every class slice full, the last class-per-thread slot of the output softmax too; B = 17: a second
#   tile with a single sample.      B = 512: 32 tiles = 16 pairs, one round of k_conversation_mc3p, and the first tile count above 16
#   for k_bwd_mc1 (tpg = 2).        B = 784: 49 tiles = 25 pairs over two rounds, the last pair's second slot empty; k_bwd_mc1 with
#   tpg = 4 and groups 13..15 empty.  Its Fixed twin tells an odd-pair fault from an Adaptive one.
CASES = {
    "fast3": dict(base="c1", D=30, B=16, T=10, n_mb=2, env=(), modes=("phased", "fused"), scopes="fixed", n_steps=(6, 8)),
    "tile": dict(base="c1", D=30, B=40, T=10, n_mb=2, env=("MMG_NO_FAST",), modes=("phased", "fused"), scopes="tile", n_steps=(5, 10)),
    "generic": dict(base="c1", D=30, B=40, T=10, n_mb=2, env=("MMG_NO_FAST", "MMG_NO_TILE"), modes=("phased", "fused"), scopes="generic", n_steps=(5, 10)),
    "generic-tiny": dict(base="tiny", D=5, B=8, T=5, n_mb=2, env=(), modes=("phased", "fused"), scopes="generic-tiny", n_steps=(3, 3)),
    "persist": dict(base="c4", D=30, B=40, T=10, n_mb=2, env=(), modes=("phased", "fused"), scopes="persist", f64=True, n_steps=(10, 9)),
    "rc": dict(base="c4-R256", D=30, B=40, T=10, n_mb=2, env=(), modes=("phased", "fused"), scopes="rc", f64=True, n_steps=(5, 5)),
    "mc3-D200": dict(base="c1", D=200, B=40, T=10, n_mb=2, env=(), modes=("phased", "fused"), scopes="mc3", n_steps=(5, 10)),
    "mc3-D33": dict(base="c1", D=33, B=20, T=10, n_mb=2, env=(), modes=("phased", "fused"), scopes="mc3", n_steps=(6, 7)),
    "mc3-D1024": dict(base="c1", D=1024, B=17, T=6, n_mb=2, env=(), modes=("phased", "fused"), scopes="mc3", n_steps=(6, 6)),
    "mc3p-B512": dict(base="c1", D=40, B=512, T=6, n_mb=1, env=(), modes=("fused",), scopes="mc3", mc3p=True, n_steps=(6,)),
    "mc3p-B784": dict(base="c1", D=40, B=784, T=4, n_mb=1, env=(), modes=("fused",), scopes="mc3", mc3p=True, n_steps=(4,)),
    "mc3p-B784-fixed": dict(base="c1", D=40, B=784, T=3, n_mb=1, env=(), modes=("fused",), scopes="mc3", mc3p=True, fixed=True, n_steps=(3,)),
}
ADAPTIVE = [k for k, c in CASES.items() if not c.get("fixed")]
BREAKS_EARLY = ("fast3", "tile", "generic", "generic-tiny", "persist", "rc", "mc3-D200", "mc3-D33")     # n_steps < T in a minibatch
SKIP = ("y2.bias", ".bs", ".br")        # as every continuous case: the baselines are not trained, y2.bias walks (common.compare_packed)


def flags_of(case):
    c = CASES[case]
    return dict(BASES[c["base"]], use_binary=False, fixed_exchange=bool(c.get("fixed")), max_exchange=c["T"])


def meta_of(case):
    c = CASES[case]
    return make_meta(flags_of(case), c["D"], c["B"], c["n_mb"], SEEDS)


def name_of(case):
    """The key of the case's separated uniforms (common.U_OVERRIDES).  Cases with the same shape share it, and the oracle run."""
    c = CASES[case]
    return "contadapt-%s-D%d-B%d-T%d%s" % (c["base"], c["D"], c["B"], c["T"], "-fixed" if c.get("fixed") else "")


_CACHE = {}


def oracle(case):
    """(name, meta, want, flips, params_before) of a case, cached per session under its shape; leave the objects unchanged.  The
    stop bits are sampled, so an Adaptive case runs on uniforms moved 1e-4 away from their probabilities (common.separate_draws;
    the message probabilities of continuous mode are empty and are skipped there)."""
    name, meta = name_of(case), meta_of(case)
    if name not in _CACHE:
        if not meta["fixed_exchange"]:
            common.separate_draws(name, meta)
        flips, params = [], []
        want = common.oracle_train_case(name, meta, flips=flips, params_before=params)
        _CACHE[name] = (name, meta, want, flips, params)
    return _CACHE[name]


def stop_steps(want, mb):
    """(t* per sample, executed steps n) of minibatch `mb`: t* is the first step whose running-minimum mask is 0 (the last mask
    is forced to 0, model.py:870, so every sample has one)."""
    n = int(want["mb%d.n_steps" % mb])
    masks = np.asarray(want["mb%d.s_masks" % mb]).reshape(n + 1, -1)
    stopped = masks[1:] == 0
    assert stopped.any(0).all()
    return stopped.argmax(0), n


def stop_margin(want, meta, name):
    """Smallest |u - p| over the stop draws of the executed steps (the only Bernoulli draws of continuous mode)."""
    return common.sampling_margin(want, meta, name)


def tile_last_steps(tstar, tile=16):
    """max t* per 16-sample tile: the step after which a tile of the fused step has nothing left to do."""
    return [int(tstar[i:i + tile].max()) for i in range(0, len(tstar), tile)]


def tied_targets(want, meta, name, mb):
    """Samples of minibatch `mb` whose target log-probability equals another class's TO THE BIT in the oracle's own `dist` (tiny
    agents: every ReLU unit of the y head off for two classes leaves both logits at y2.bias).  The oracle's hit count takes the last
    top_k indices of numpy's argsort there (model.py:1333), whose order among equal keys is unspecified; the library's rule is
    hit = #{d: y[d] > y[target]} < top_k (tests/test_option_branches_gpu.py: test_tied_target_logit_counts_as_the_rule_says)."""
    _, target, _, _ = common.case_inputs(meta, mb, name)
    d = np.asarray(want["mb%d.dist" % mb])
    other = np.ones_like(d, bool)
    other[np.arange(len(target)), target] = False
    return np.nonzero(((d == d[np.arange(len(target)), target][:, None]) & other).any(1))[0].tolist()


def rule_hits(want, meta, name, mb):
    """The library's hit rule applied to the ORACLE's log-probabilities: #{b: #{d: dist[b, d] > dist[b, target]} < top_k}."""
    _, target, _, _ = common.case_inputs(meta, mb, name)
    d = np.asarray(want["mb%d.dist" % mb])
    return int(((d > d[np.arange(len(target)), target][:, None]).sum(1) < min(meta["top_k_train"], d.shape[1])).sum())
