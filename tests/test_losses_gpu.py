"""The differentiable loss functions of multimodalgame_amd.losses (HIP forward / VJP kernels, csrc/kernels_loss.h) against
oracle.cpu_ref's functions on float64 copies of the same fp32 inputs -- the reference contributes no rounding.

Tolerances are the project's, not this file's: losses 1e-4 absolute; gradients atol 1e-4 scaled by
max(1, |want|_max) and rtol 1e-3, as _assert_close of tests/test_autograd_gpu.py.

1. forward and gradients of each function over the shapes at which the kernels take another path (rows: 1, 2, one more than one /
   two row chunks; row widths below, at and above a wave pass and a 16-byte lane; 1 and 10 steps; masks None and Adaptive-shaped
   with a step of zero, of exactly one and of exactly two active rows; entropy penalty None / 0.08; saturated probabilities);
2. both sides of the std guard of model.py:912-915 (reach conditions asserted on the float64 reference);
3. upstream gradients through every output alone and through a random functional of all of them;
4. non-contiguous inputs and unbind views of one tensor;
5. retain_graph, bit-identical repeats, double backward raises;
6. the reference's training block -- exchange(autograd) + losses.training_losses + four backward() -- equals the engine's fused
   gradients; 7. ... without a host synchronisation.

multistep_loss_bas and a step WITHOUT active rows: the reference multiplies the MSE of an empty selection (NaN in current torch,
an indexing error in the reference's torch) by the step's weight 0; the kernels define that step's contribution as 0, like
multistep_loss_binary's ``mask_sums == 0`` branch does, so the float64 reference is cpu_ref.multistep_loss_bas on the same lists
with the empty steps left out (their weight is 0), and the gradient of an empty step must be exactly 0."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import common

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodalgame_amd", "csrc",
                         "kernels_loss.h")).read()
CHUNK = int(re.search(r"#define MMG_LOSS_ROWS (\d+)", _HDR).group(1))
BATCHES = sorted({1, 2, 65, CHUNK + 1, 2 * CHUNK + 1})
LOSS_ATOL = 1e-4


def _close(got, want, label, atol=1e-4, rtol=1e-3):
    """_assert_close of tests/test_autograd_gpu.py with scale_atol, on one pair of tensors."""
    g, w = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    if w.numel() == 0:
        return
    tol = atol * max(1.0, float(w.abs().max())) + rtol * w.abs()
    err = (g - w).abs()
    assert bool(torch.isfinite(g).all()), label + ": non-finite gradient"
    assert bool((err <= tol).all()), "%s: max err %.3e at %d (got %.6e want %.6e)" % (
        label, float(err.max()), int((err - tol).argmax()), float(g[int((err - tol).argmax())]), float(w[int((err - tol).argmax())]))


def _loss_close(got, want, label):
    g, w = float(got.detach()), float(want.detach())
    print("%s: got %.8f want %.8f" % (label, g, w))
    assert abs(g - w) <= LOSS_ATOL, "%s: got %.8f want %.8f" % (label, g, w)


def _lengths(rs, n, B):
    """Adaptive conversations: sample b is active at steps 0 .. L_b - 1.  n >= 4 and B >= 2: the last step has no active row, the
    one before exactly one (sample 0), the one before that exactly two (samples 0 and 1)."""
    if n < 4:
        return np.full(B, n, dtype=np.int64)
    L = rs.randint(1, n - 2, size=B)                     # 1 .. n - 3
    L[0] = n - 1
    if B > 1:
        L[1] = n - 2
    return L


def _stop_masks(L, n):
    """[n, B, 1] uint8: the masks multistep_loss_* get in Adaptive mode (s_masks[:-1]: all ones first, then a running minimum)."""
    t = np.arange(n)[:, None]
    return (t < L[None, :]).astype(np.uint8)[:, :, None]


def _y_masks(L, n):
    """[n, B, 1] uint8: y_masks of model.py:1261 -- exactly one step per sample, its last active one."""
    t = np.arange(n)[:, None]
    return (t == (L[None, :] - 1)).astype(np.uint8)[:, :, None]


def _dev_list(a, requires_grad=False):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(requires_grad) for x in a]


def _ref_list(a, requires_grad=False):
    return [torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(requires_grad) for x in a]


def _g(t):
    """Gradient of a float64 reference leaf; a leaf the reference's graph does not reach (a step without an active row) has 0."""
    return t.grad if t.grad is not None else torch.zeros_like(t)


def _mask_lists(m):
    if m is None:
        return None, None
    return [torch.from_numpy(x.copy()).to(DEV) for x in m], [torch.from_numpy(x.copy()) for x in m]


# ------------------------------------------------------------------ binary REINFORCE loss
def _binary_case(seed, n, B, W, masked, spread=1.0):
    rs = np.random.RandomState(seed)
    prob = (1.0 / (1.0 + np.exp(-2.0 * rs.standard_normal((n, B, W))))).astype(np.float32)
    feat = (rs.random_sample((n, B, W)) < prob).astype(np.float32)
    sat = rs.random_sample((n, B, W)) < 0.06                  # saturated probabilities, bits consistent with them
    hi = rs.random_sample((n, B, W)) < 0.5
    prob[sat & hi], feat[sat & hi] = 1.0, 1.0
    prob[sat & ~hi], feat[sat & ~hi] = 0.0, 0.0
    logs = (-np.abs(rs.standard_normal((B, 1))) - 0.1).astype(np.float32)
    scores = (logs[None] - spread * rs.standard_normal((n, B, 1))).astype(np.float32)
    L = _lengths(rs, n, B)
    m = _stop_masks(L, n) if masked else None
    return feat, prob, logs, scores, m


def _binary_both(case, penalty, from_lists=None):
    """(loss, entropies, probs) on the device and in float64 on the CPU."""
    from multimodalgame_amd import losses
    feat, prob, logs, scores, m = case
    md, mr = _mask_lists(m)
    pd = from_lists if from_lists is not None else _dev_list(prob, True)
    got = losses.multistep_loss_binary(_dev_list(feat), pd, torch.from_numpy(logs).to(DEV), _dev_list(scores), md, penalty)
    pr = _ref_list(prob, True)
    want = cpu_ref.multistep_loss_binary(_ref_list(feat), pr, torch.from_numpy(logs).double(), _ref_list(scores), mr, penalty)
    return (got[0], got[1], pd), (want[0].sum(), [e.sum() for e in want[1]], pr)


def _functional(rs, loss, ents, a=None, b=None):
    a = rs.standard_normal() if a is None else a
    b = rs.standard_normal(len(ents)) if b is None else b
    return a * loss + sum(float(bt) * e for bt, e in zip(b, ents)), a, b


def _check_binary(case, penalty, label, rs):
    (gl, ge, gp), (wl, we, wp) = _binary_both(case, penalty)
    assert gl.dim() == 0 and len(ge) == len(we) and gl.device.type == torch.device(DEV).type
    _loss_close(gl, wl, label + " loss")
    for t, (g, w) in enumerate(zip(ge, we)):
        _loss_close(g, w, "%s entropy[%d]" % (label, t))
    fg, a, b = _functional(rs, gl, ge)
    fw, _, _ = _functional(rs, wl, we, a, b)
    fg.backward()
    if fw.requires_grad:
        fw.backward()
    for t, (g, w) in enumerate(zip(gp, wp)):
        _close(g.grad, _g(w), "%s dprob[%d]" % (label, t))


@pytest.mark.parametrize("n", [1, 10])
@pytest.mark.parametrize("W", [1, 32, 33])
@pytest.mark.parametrize("B", BATCHES)
def test_binary_loss_and_gradient(B, W, n):
    rs = np.random.RandomState(1000 * B + 10 * W + n)
    for masked in (False, True):
        case = _binary_case(7 + B + W + n, n, B, W, masked)
        if masked and n >= 4 and B >= 2:                     # the mask shapes the issue asks for were built
            act = case[4].reshape(n, B).sum(1)
            assert act[-1] == 0 and act[-2] == 1 and act[-3] == 2 and act[0] == B
        for penalty in (None, 0.08):
            _check_binary(case, penalty, "B%d W%d n%d %s pen=%s" % (B, W, n, "masks" if masked else "nomask", penalty), rs)


def test_calculate_loss_binary_single_step():
    from multimodalgame_amd import losses
    feat, prob, logs, scores, _ = _binary_case(5, 1, CHUNK + 1, 33, False)
    p = torch.from_numpy(prob[0]).to(DEV).requires_grad_(True)
    loss, ne = losses.calculate_loss_binary(torch.from_numpy(feat[0]).to(DEV), p, torch.from_numpy(logs).to(DEV),
                                            torch.from_numpy(scores[0]).to(DEV), 0.08)
    p64 = torch.from_numpy(prob[0]).double().requires_grad_(True)
    wl, wne = cpu_ref.calculate_loss_binary(torch.from_numpy(feat[0]).double(), p64, torch.from_numpy(logs).double(),
                                            torch.from_numpy(scores[0]).double(), 0.08)
    _loss_close(loss, wl, "calculate_loss_binary loss")
    _loss_close(ne, wne, "calculate_loss_binary negentropy")
    loss.backward(); wl.backward()
    _close(p.grad, p64.grad, "calculate_loss_binary dprob")


@pytest.mark.parametrize("spread, side", [(3.0, "scaled"), (0.1, "unscaled")])
def test_both_sides_of_the_std_guard(spread, side):
    for masked in (False, True):
        n, B = (10, 65) if masked else (2, 65)
        case = _binary_case(31, n, B, 32, masked, spread=spread)
        feat, prob, logs, scores, m = case
        w = torch.from_numpy(logs).double()[None] - torch.from_numpy(scores).double()        # [n, B, 1]
        stds = []
        for t in range(n):
            rows = w[t][torch.from_numpy(m[t]).bool()] if masked else w[t].reshape(-1)
            if rows.numel() > 1:
                stds.append(float(torch.std(rows)))
        if side == "scaled":                              # reach: some step divides by its std ...
            assert len([s for s in stds if s > 1.0]) >= 2, stds
        else:                                             # ... and here every step keeps the divisor 1
            assert stds and all(s < 1.0 for s in stds), stds
        _check_binary(case, 0.08, "std guard %s %s" % (side, "masks" if masked else "nomask"), np.random.RandomState(3))


def test_binary_upstream_gradients_alone():
    case = _binary_case(11, 10, CHUNK + 1, 33, True)
    for which in ("loss", "entropies"):
        (gl, ge, gp), (wl, we, wp) = _binary_both(case, 0.08)
        if which == "loss":
            gl.backward(); wl.backward()
        else:
            sum(ge).backward(); sum(we).backward()
        for t, (g, w) in enumerate(zip(gp, wp)):
            assert g.grad is not None
            _close(g.grad, _g(w), "binary d%s dprob[%d]" % (which, t))


# ------------------------------------------------------------------ baseline MSE
def _bas_both(n, B, masked, seed):
    from multimodalgame_amd import losses
    rs = np.random.RandomState(seed)
    logs = (-np.abs(rs.standard_normal((B, 1)))).astype(np.float32)
    scores = rs.standard_normal((n, B, 1)).astype(np.float32)
    m = _stop_masks(_lengths(rs, n, B), n) if masked else None
    md, mr = _mask_lists(m)
    sd = _dev_list(scores, True)
    got = losses.multistep_loss_bas(sd, torch.from_numpy(logs).to(DEV), md)
    sr = _ref_list(scores, True)
    keep = [t for t in range(n) if m is None or m[t].sum() > 0]          # (see the module docstring: empty steps weigh 0)
    want = cpu_ref.multistep_loss_bas([sr[t] for t in keep], torch.from_numpy(logs).double(), None if m is None else [mr[t] for t in keep])
    return got, sd, want, sr, keep


@pytest.mark.parametrize("n", [1, 10])
@pytest.mark.parametrize("B", BATCHES)
def test_bas_loss_and_gradient(B, n):
    for masked in (False, True):
        got, sd, want, sr, keep = _bas_both(n, B, masked, 17 + B + n)
        label = "bas B%d n%d %s" % (B, n, "masks" if masked else "nomask")
        assert got.dim() == 0
        _loss_close(got, want, label)
        (1.7 * got).backward(); (1.7 * want).backward()
        for t in range(n):
            if t in keep:
                _close(sd[t].grad, sr[t].grad, "%s dscores[%d]" % (label, t))
            else:
                assert float(sd[t].grad.abs().max()) == 0.0


def test_calculate_loss_bas_single_step():
    from multimodalgame_amd import losses
    rs = np.random.RandomState(2)
    s, l = rs.standard_normal((2 * CHUNK + 1, 1)).astype(np.float32), rs.standard_normal((2 * CHUNK + 1, 1)).astype(np.float32)
    sd = torch.from_numpy(s).to(DEV).requires_grad_(True)
    got = losses.calculate_loss_bas(sd, torch.from_numpy(l).to(DEV))
    s64 = torch.from_numpy(s).double().requires_grad_(True)
    want = F.mse_loss(s64, torch.from_numpy(l).double())
    _loss_close(got, want, "calculate_loss_bas")
    got.backward(); want.backward()
    _close(sd.grad, s64.grad, "calculate_loss_bas dscores")


# ------------------------------------------------------------------ output selection + NLL
def _rec_case(seed, n, B, D, masked):
    rs = np.random.RandomState(seed)
    y = (3.0 * rs.standard_normal((n, B, D))).astype(np.float32)
    target = rs.randint(0, D, size=B).astype(np.int64)
    m = _y_masks(_lengths(rs, n, B), n) if masked else None
    return y, target, m


def _rec_ref(y, target, m):
    yr = _ref_list(y, True)
    outp, ne = cpu_ref.get_rec_outp(yr, None if m is None else [torch.from_numpy(x.copy()) for x in m])
    dist = F.log_softmax(outp, dim=1)
    tg = torch.from_numpy(target)
    return outp, ne, F.nll_loss(dist, tg), dist.detach().gather(1, tg.view(-1, 1)), yr


def _rec_dev(y, target, m, ys=None):
    from multimodalgame_amd import losses
    yd = ys if ys is not None else _dev_list(y, True)
    md, _ = _mask_lists(m)
    outp, ne, nll, logs = losses.reward_and_nll(yd, md, torch.from_numpy(target).to(DEV))
    return outp, ne, nll, logs, yd


def _rec_functional(outp, ne, nll, coef, parts=("outp", "negent", "nll")):
    f = 0.0
    if "outp" in parts:
        f = f + (coef["outp"].to(outp) * outp).sum()
    if "negent" in parts:
        f = f + sum(float(c) * e for c, e in zip(coef["negent"], ne))
    if "nll" in parts:
        f = f + float(coef["nll"]) * nll
    return f


def _check_rec(case, label, parts=("outp", "negent", "nll"), ys=None, leaves=None):
    y, target, m = case
    n, B, D = y.shape
    go, gne, gnll, glogs, yd = _rec_dev(y, target, m, ys)
    wo, wne, wnll, wlogs, yr = _rec_ref(y, target, m)
    assert go.shape == (B, D) and glogs.shape == (B, 1) and not glogs.requires_grad and gnll.dim() == 0 and len(gne) == n
    assert float((go.detach().double().cpu() - wo.detach()).abs().max()) == 0.0, label + ": outp is a selection of y"
    for t in range(n):
        _loss_close(gne[t], wne[t], "%s negentropy[%d]" % (label, t))
    _loss_close(gnll, wnll, label + " nll")
    assert float((glogs.double().cpu() - wlogs).abs().max()) <= LOSS_ATOL, label + " logs"
    rs = np.random.RandomState(5)
    coef = dict(outp=torch.from_numpy(rs.standard_normal((B, D))), negent=rs.standard_normal(n), nll=rs.standard_normal())
    _rec_functional(go, gne, gnll, coef, parts).backward()
    _rec_functional(wo, wne, wnll, coef, parts).backward()
    got = leaves() if leaves is not None else [t.grad for t in yd]
    for t in range(n):
        assert got[t] is not None
        _close(got[t], _g(yr[t]), "%s dy[%d] via %s" % (label, t, "+".join(parts)))


@pytest.mark.parametrize("n", [1, 10])
@pytest.mark.parametrize("B, D", [(b, d) for b in BATCHES for d in (1, 30, 33)] + [(3, 1000)])
def test_rec_outp_nll_and_gradient(B, D, n):
    for masked in (False, True):
        case = _rec_case(3 + B + D + n, n, B, D, masked)
        if masked and n >= 4 and B >= 2:
            sel = case[2].reshape(n, B)
            assert (sel.sum(0) == 1).all() and sel[-1].sum() == 0 and sel[-2].sum() == 1 and sel[-3].sum() == 1
        _check_rec(case, "rec B%d D%d n%d %s" % (B, D, n, "masks" if masked else "nomask"))


def test_get_rec_outp_without_a_target():
    from multimodalgame_amd import losses
    y, target, m = _rec_case(9, 10, CHUNK + 1, 30, True)
    yd = _dev_list(y, True)
    outp, ne = losses.get_rec_outp(yd, _mask_lists(m)[0])
    wo, wne, _, _, yr = _rec_ref(y, target, m)
    assert float((outp.detach().double().cpu() - wo.detach()).abs().max()) == 0.0 and len(ne) == 10
    (outp.sum() + 2.0 * sum(ne)).backward(); (wo.sum() + 2.0 * sum(wne)).backward()
    for t in range(10):
        _close(yd[t].grad, _g(yr[t]), "get_rec_outp dy[%d]" % t)
    last, _ = losses.get_rec_outp(_dev_list(y), None)              # masks None: the last step (model.py:904)
    assert torch.equal(last.cpu(), torch.from_numpy(y[-1]))
    ll = losses.loglikelihood(F.log_softmax(outp.detach(), dim=1), torch.from_numpy(target).to(DEV).view(-1, 1))
    assert ll.shape == (CHUNK + 1, 1)


@pytest.mark.parametrize("parts", [("negent",), ("outp",), ("nll",), ("outp", "negent", "nll")])
def test_rec_upstream_gradients(parts):
    _check_rec(_rec_case(21, 10, CHUNK + 1, 33, True), "rec upstream", parts=parts)


# ------------------------------------------------------------------ 4. views
def test_non_contiguous_inputs_and_unbind_views():
    from multimodalgame_amd import losses
    n, B, W, D = 10, CHUNK + 1, 33, 30
    case = _binary_case(41, n, B, W, True)
    feat, prob, logs, scores, m = case
    # (a) every list entry a non-contiguous view: every second column of a twice as wide tensor / a transposed tensor
    wide = [torch.zeros(B, 2 * W, device=DEV) for _ in range(n)]
    for t in range(n):
        wide[t][:, ::2] = torch.from_numpy(prob[t]).to(DEV)
    leaves = [w.requires_grad_(True) for w in wide]
    views = [w[:, ::2] for w in leaves]
    assert not views[0].is_contiguous()
    (gl, ge, _), (wl, we, wp) = _binary_both(case, 0.08, from_lists=views)
    _loss_close(gl, wl, "non-contiguous binary loss")
    (gl + sum(ge)).backward(); (wl + sum(we)).backward()
    for t in range(n):
        _close(leaves[t].grad[:, ::2], _g(wp[t]), "non-contiguous dprob[%d]" % t)
        assert float(leaves[t].grad[:, 1::2].abs().max()) == 0.0
    rcase = _rec_case(42, n, B, D, True)
    yT = [torch.from_numpy(np.ascontiguousarray(rcase[0][t].T)).to(DEV).requires_grad_(True) for t in range(n)]      # [D, B] leaves
    _check_rec(rcase, "transposed y", ys=[v.t() for v in yT], leaves=lambda: [v.grad.t() for v in yT])
    # (b) the unbind views of ONE tensor (what exchange(autograd) returns): used in place, gradients reach the stacked leaf
    P = torch.from_numpy(prob).to(DEV).requires_grad_(True)
    (gl, ge, _), (wl, we, wp) = _binary_both(case, 0.08, from_lists=list(P.unbind(0)))
    _loss_close(gl, wl, "unbind binary loss")
    (gl + sum(ge)).backward(); (wl + sum(we)).backward()
    _close(P.grad, torch.stack([_g(w) for w in wp]), "unbind dprob")
    Y = torch.from_numpy(rcase[0]).to(DEV).requires_grad_(True)
    _check_rec(rcase, "unbind y", ys=list(Y.unbind(0)), leaves=lambda: list(Y.grad.unbind(0)))
    S = torch.from_numpy(scores).to(DEV).requires_grad_(True)
    md, mr = _mask_lists(m)
    got = losses.multistep_loss_bas(list(S.unbind(0)), torch.from_numpy(logs).to(DEV), md)
    keep = [t for t in range(n) if m[t].sum() > 0]
    sr = _ref_list(scores, True)
    want = cpu_ref.multistep_loss_bas([sr[t] for t in keep], torch.from_numpy(logs).double(), [mr[t] for t in keep])
    _loss_close(got, want, "unbind bas loss")
    got.backward(); want.backward()
    _close(S.grad, torch.stack([_g(s) for s in sr]), "unbind dscores")


# ------------------------------------------------------------------ 5. backward twice, determinism
def _all_three(seed=51):
    from multimodalgame_amd import losses
    n, B, W, D = 10, 2 * CHUNK + 1, 33, 33
    feat, prob, logs, scores, m = _binary_case(seed, n, B, W, True)
    y, target, ym = _rec_case(seed + 1, n, B, D, True)
    pd, sd, yd = _dev_list(prob, True), _dev_list(scores, True), _dev_list(y, True)
    md = _mask_lists(m)[0]
    lb, ents = losses.multistep_loss_binary(_dev_list(feat), pd, torch.from_numpy(logs).to(DEV), _dev_list(scores), md, 0.08)
    ls = losses.multistep_loss_bas(sd, torch.from_numpy(logs).to(DEV), md)
    outp, ne, nll, lg = losses.reward_and_nll(yd, _mask_lists(ym)[0], torch.from_numpy(target).to(DEV))
    total = lb + 0.5 * sum(ents) + ls + nll + 0.25 * sum(ne) + (outp * outp).sum()
    outs = [lb, ls, nll, outp, lg] + list(ents) + list(ne)
    return total, outs, pd + sd + yd


def _grads_of(leaves):
    return [t.grad.clone() for t in leaves]


def test_retain_graph_repeats_and_double_backward():
    total, outs, leaves = _all_three()
    total.backward(retain_graph=True)
    first = _grads_of(leaves)
    for t in leaves:
        t.grad = None
    total.backward()                                            # the second pass reads the saved inputs and the save array only
    for a, b in zip(first, _grads_of(leaves)):
        assert torch.equal(a, b)
    total2, outs2, leaves2 = _all_three()                       # two fresh calls: bit-identical outputs and gradients
    total2.backward()
    for a, b in zip(outs, outs2):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(first, _grads_of(leaves2)):
        assert torch.equal(a, b)
    total3, _, leaves3 = _all_three()
    g = torch.autograd.grad(total3, leaves3[0], create_graph=True)[0]
    with pytest.raises(RuntimeError):                           # once_differentiable
        g.sum().backward()


# ------------------------------------------------------------------ 6. / 7. the reference's training block
def _block(name, sync_mode=None):
    from multimodalgame_amd import losses
    from tests import test_autograd_gpu as ag
    _, meta = common.load_golden(name)
    fl = common.flags_from_meta(meta)
    game, eng = ag._game(meta, autograd=True)
    _, target, _, args = ag._inputs(meta, 0, name)
    agents = ag.AGENTS if fl.use_binary else ("receiver",)
    out = ag._exchange(game, fl, args)           # (Adaptive: exchange()'s own break_early test is the reference's one host sync, model.py:866)
    ag._zero(game)
    torch.cuda.synchronize()
    if sync_mode is not None:
        torch.cuda.set_sync_debug_mode(sync_mode)
    try:
        ls = losses.training_losses(out, args["target"], fl)
        assert set(agents) <= set(ls) and all(ls[a].is_cuda for a in agents)
        assert (len(ls) == 10) if fl.use_binary else (set(ls) == {"receiver"})
        for a in agents:                                        # four separate backward() calls, model.py:1309-1328
            ls[a].backward()
    finally:
        if sync_mode is not None:
            torch.cuda.set_sync_debug_mode("default")
    got = ag._grads(game, agents)
    eng.forward(args["data"], args["target"], args["desc"], *args["uniforms"], train=True, run_all=True)
    eng.loss_stats()
    eng.backward(args["data"], args["target"], args["desc"])
    torch.cuda.synchronize()
    want = {a: {k: v.detach().cpu().clone() for k, v in eng.grads[a].items()} for a in agents}
    ag._assert_close(got, want, name)
    if fl.use_binary:                                           # the logged scalars are the engine's (tape "losses")
        logged = eng.losses()
        for k in ("nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen", "loss_bas_rec", "loss_bas_sen"):
            if k in logged:
                assert abs(float(ls[k]) - float(logged[k])) <= LOSS_ATOL, (k, float(ls[k]), logged[k])


@pytest.mark.parametrize("name", ["g2_adaptive_c1", "g3_fixed_c3shard", "g3_continuous"])
def test_reference_block_on_device_losses_gives_the_engine_gradients(name):
    _block(name)


def _sync_debug_works():
    """True when this torch build raises on a synchronising call under set_sync_debug_mode("error")."""
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception:
        return False
    try:
        probe.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("name", ["g2_adaptive_c1", "g3_fixed_c3shard"])
def test_losses_and_backward_do_not_synchronise_with_the_host(name):
    if not _sync_debug_works():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag synchronising calls in this torch build on ROCm")
    _block(name, sync_mode="error")
