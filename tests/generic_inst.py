"""Shapes, selection predicates and oracle runs of tests/test_generic_instantiations_{cpu,gpu}.py: the generic per-sample family's
512-thread conversation kernels and its large-batch (MANY) reverse pass, which every handle with message flips, a sender variant,
description attention or visual attention runs and which no shape of those features' own test modules selects.

The two rules of multimodalgame_amd/csrc/host_select.h (shape_pass: conv_threads; plan_launches: bwd_conv_fn), restated:
    conv_threads = 512  when  B <= 256 and (H * W >= 65536 or D * (R + V) >= 65536),  else 256
    k_bwd_conv<MANY = true, ...>  when  B > 512
The shapes are the smallest that meet a rule, derived from the feature modules' small shape (T 3, B 5, F 18, H 40, W 12, R 20, V 12,
K 70, 7 classes, Adam):
    W512   H = 260, W = sender_out_dim = 253 (H * W = 65 780; W is no multiple of four: unaligned weight rows, the row passes' tails)
    B513   B = 513 at T = 3 and T = 4 (T * B = 2052 rows: beyond the 2048 rows k_wgrad's live-row list holds)
    KM80 / KM272 (visual attention)  C = 80 / 272 channels = 5 / 17 sixteen-channel chunks of gemm_kmajor_tile's float4 branch:
           an idle wave and a two-chunk pass / a full pass and a one-chunk pass; A = 20, a 1 x 5 map, B = 5: M = 25 output rows, both
           output-tile edges ragged, a 16-row tile spans several samples.
The data seeds were searched on the CPU oracle; tests/test_generic_instantiations_cpu.py asserts what they reach."""
import contextlib

import numpy as np
import torch

from oracle import cpu_ref
from tests import common, desc_attn_ref as da, flipout_ref, sender_variant_ref as sv, visual_attn_ref as va

ATOL, RTOL = 1e-4, 1e-3                  # the feature modules' own: forward 1e-4 absolute, gradients and parameters 1e-4 + 1e-3 |v|
W512 = dict(img_h_dim=260, rec_w_dim=253, sender_out_dim=253)
B513 = 513
KM = {"KM80": 80, "KM272": 272}
KM_OVER = dict(vattn_dim=20, map_hw=[1, 5])
P_SEN, P_REC, EVAL_SEED = 0.25, 0.05, 77
MODES = ("adaptive", "fixed", "continuous")
MODE_FLAGS = {"adaptive": dict(use_binary=True, fixed_exchange=False), "fixed": dict(use_binary=True, fixed_exchange=True),
              "continuous": dict(use_binary=False, fixed_exchange=True)}
VARIANTS_W512 = ("prod", "ignore_code", "ignore_receiver", "prod_ignore_receiver")
VARIANTS_B513 = ("prod", "ignore_code", "ignore_receiver")


# ------------------------------------------------------------------ the two selection rules
def dims_of(m):
    return dict(B=m["batch"], H=m["img_h_dim"], W=m["rec_w_dim"], D=m["n_classes"], R=m["rec_hidden"], V=m["wv_dim"])


def conv_threads(B, H, W, D, R, V):
    return 512 if B <= 256 and (H * W >= 65536 or D * (R + V) >= 65536) else 256


def bwd_many(B, **_):
    return B > 512


# ------------------------------------------------------------------ data seeds (searched on the CPU oracle)
# W512 and KM cases: no ReLU unit of the y head's output step or of a baseline's live rows within common.RELU_EPS of zero, adaptive
# cases with samples that stop early and samples that run to the last step, attention weights more than 1e-2 away from uniform at
# some t >= 1, evaluation conversations without a probability within 1e-4 of 0.5.  B513 cases have ~3 x 10^5 ReLU units per
# minibatch: no seed leaves none of them near its threshold, so the near-threshold units of the oracle's own run are pinned (N_NEAR,
# asserted on the CPU) and the GPU comparison goes through common.assert_parity, which exempts nothing: a unit out of that set that
# the GPU put on the other side is forced to the GPU's side in a re-run of the oracle, and every entry must then agree.
SEEDS = {("plain", "adaptive"): 6, ("plain", "fixed"): 6, ("plain", "continuous"): 6, "flip": 6,
         ("variant", "prod"): 6, ("variant", "ignore_code"): 6, ("variant", "ignore_receiver"): 6, ("variant", "prod_ignore_receiver"): 6,
         ("desc", "adaptive"): 7, ("desc", "fixed"): 7, ("desc", "continuous"): 6,
         ("vattn", "adaptive"): 8, ("vattn", "fixed"): 8, ("vattn", "continuous"): 6, ("KM80", "adaptive"): 6, ("KM272", "adaptive"): 6,
         ("b513", 3, "adaptive"): 6, ("b513", 3, "continuous"): 6, ("b513", 4, "adaptive"): 6, ("b513", 4, "continuous"): 6,
         ("b513", "prod"): 6, ("b513", "ignore_code"): 6, ("b513", "ignore_receiver"): 6}
# near-threshold units (common.RELU_EPS) of the oracle's own run per B513 case: (T, mode) of the plain handle, (variant,) at T = 3
N_NEAR = {(3, "adaptive"): 45, (3, "continuous"): 17, (4, "adaptive"): 50, (4, "continuous"): 19,
          ("prod",): 39, ("ignore_code",): 44, ("ignore_receiver",): 48}
# Evaluation conversations round every probability.  Continuous messages: no stop probability within 1e-4 of 0.5.  Binary messages
# of W = 253 bits: 7 605 probabilities per conversation, about ten of them within 1e-4 of 0.5 whatever the seed (6..149 searched);
# the seeds below keep every probability more than EVAL_MARGIN away from 0.5, twice the band in which tests/test_flipout_gpu.py
# lets two correct fp32 summation orders decide differently (2e-5).  The GPU tests compare every bit of every row.
EVAL_SEEDS = {"flip": 148, ("desc", "adaptive"): 37, ("desc", "continuous"): 6}
EVAL_MARGIN = 4e-5


def plain_meta(kind, mode="adaptive", T=3, setting=None, seed=None):
    """The small shape at W512 or B513 for a plain, flipping or variant handle (sender_variant_ref's meta: weights 5, uniforms 7)."""
    over = dict(MODE_FLAGS[mode])
    if kind == "W512":
        over.update(W512)
    else:
        over.update(batch=B513, batch_size=B513, max_exchange=T)
    if setting is not None and setting[2]:
        over.update(ignore_receiver=True)
    m = sv.meta("B", **over)
    if seed is not None:
        m["seed_data"] = seed
    return m


def desc_meta(mode, seed=None, **over):
    return da.meta("B", mode, **dict(W512, **over), **({} if seed is None else dict(seed_data=seed)))


def vattn_meta(kind, mode="adaptive", seed=None):
    over = dict(W512) if kind == "W512" else dict(KM_OVER, img_feat_dim=KM[kind])
    if seed is not None:
        over.update(seed_data=seed)
    return va.meta("B", mode, **over)


# ------------------------------------------------------------------ the oracle with wrapped agents, through tests/common.py
@contextlib.contextmanager
def wrapped_agents(wrap):
    """cpu_ref.build_agents hands out agents with `wrap(models)` applied (None: the plain ones) while the block runs: what
    common.separate_draws, common.oracle_train_case and the forced re-runs of common.assert_parity then train."""
    if wrap is None:
        yield
        return
    plain = cpu_ref.build_agents

    def build(flags, rng=None):
        models = plain(flags, rng=rng)
        wrap(models)
        return models
    cpu_ref.build_agents = build
    try:
        yield
    finally:
        cpu_ref.build_agents = plain


def variant_wrap(setting):
    return None if setting is None else (lambda models: sv.variant_sender(models["sender"], setting[0], setting[1]))


def flip_wrap(m):
    T, B, W = m["max_exchange"], m["batch"], m["rec_w_dim"]
    m_z, m_w = flipout_ref.flip_masks(0, 1, T, B, W, P_SEN, P_REC)        # common.hip_train_case trains with seed 0, counter 1
    return lambda models: flipout_ref.flip_agents(models, m_z, m_w)


_CACHE = {}


def once(key, make):
    """One oracle run per key, shared by the tests that need it and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_minibatch(name, m, wrap=None):
    """(separated uniforms, packed oracle minibatch, near-threshold ReLU units) of the case `name`: common.separate_draws (every draw
    1e-4 away from its probability, the trajectory unchanged) and common.oracle_train_case on the wrapped agents."""
    def make():
        with wrapped_agents(wrap):
            us = common.separate_draws(name, m, margin=1e-4)[0]
            try:
                flips = []
                want = common.oracle_train_case(name, m, flips=flips)
            finally:
                common.U_OVERRIDES.pop(name, None)
        return us, want, flips
    return once(("minibatch", name), make)


def attention_minibatch(ref, m, update=True):
    """(separated uniforms, res, models, near-threshold ReLU units) of minibatch 0 of `m` with the wrapped agents of `ref`
    (desc_attn_ref / visual_attn_ref: their build loads the attention tensors, which common.oracle_train_case cannot)."""
    def make():
        us = ref.separated_uniforms(m)
        torch.manual_seed(0)
        models, fl = ref.build(m, rng=cpu_ref.UniformTape(*us))
        optimizers = cpu_ref.build_optimizers(models, fl)
        y1_out, bas_out = [], {"bas_rec": [], "bas_sen": []}
        keep = lambda store: (lambda mod, inp, o: store.append(o.detach().clone()))
        hooks = [models["receiver"].y1.register_forward_hook(keep(y1_out)),
                 models["baseline_rec"].linear1.register_forward_hook(keep(bas_out["bas_rec"])),
                 models["baseline_sen"].linear1.register_forward_hook(keep(bas_out["bas_sen"]))]
        x, target, desc = ref._inputs(m)
        res = cpu_ref.train_minibatch(models, optimizers, x, target, desc, fl, update=update)
        for h in hooks:
            h.remove()
        flips = common._relu_flips(res, y1_out, bas_out, m["n_classes"], binary=bool(fl.use_binary), fixed=bool(fl.fixed_exchange))
        return us, res, models, flips
    return once(("attention", ref.__name__, update, tuple(sorted((k, str(v)) for k, v in m.items()))), make)


def stop_steps(want):
    """Per sample, the step it stopped at (n - 1: it ran to the last executed step) from the packed masks of a minibatch."""
    masks = np.asarray(want["mb0.s_masks"]).reshape(int(want["mb0.n_steps"]) + 1, -1)
    n = masks.shape[0] - 1
    stopped = masks[1:n + 1] == 0
    return np.where(stopped.any(0), stopped.argmax(0), n - 1), n
