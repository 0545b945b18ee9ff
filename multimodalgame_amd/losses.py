"""The reference's loss functions (model.py:571-577, 879-988) on the device, differentiable: each one is ONE autograd node over the
HIP forward / vector-Jacobian kernels of include/mmg.h (mmg_loss_binary_*, mmg_loss_bas_*, mmg_rec_outp_*; csrc/kernels_loss.h).

Same names, signatures and return structures as the reference: arguments are lists of per-step ``[B, .]`` tensors as exchange()
returns them, masks are lists of uint8 ``[B, 1]`` tensors or ``None``, ``entropy_penalty`` is a float or ``None``.  Gradients
reach ``binary_probs``, ``baseline_scores`` (in the ``*_bas`` functions) and ``y`` -- exactly where the reference's do; the sampled
bits, ``logs``, the scores inside the REINFORCE weight, masks and targets are constants (the reference detaches them).

Everything stays on the device: the lists are stacked there (consecutive ``unbind`` views of one tensor are used in place), no
tensor is copied to the host and nothing synchronises with it.  There is no CPU fallback: CPU tensors, ``None`` probabilities
(continuous messages have no REINFORCE loss) and lists of different lengths raise ``ValueError``.  Double backward raises.

Besides the six reference names: ``reward_and_nll`` (model.py:1264-1275 as one node) and ``training_losses`` (model.py:1248-1305)."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["loglikelihood", "get_rec_outp", "calculate_loss_binary", "multistep_loss_binary", "calculate_loss_bas",
           "multistep_loss_bas", "reward_and_nll", "training_losses"]


# ------------------------------------------------------------------ argument plumbing
def _same_length(n, **lists):
    """Every list of one call (None and stacked masks aside) holds n steps; checked before anything else is looked at."""
    for name, lst in lists.items():
        if lst is None or torch.is_tensor(lst):
            continue
        if not isinstance(lst, (list, tuple)):
            raise ValueError("%s must be a list of per-step tensors" % name)
        if len(lst) != n:
            raise ValueError("%s has %d steps, %d expected: the lists of one call must have the same length" % (name, len(lst), n))


def _tensor_list(lst, name, n=None):
    if torch.is_tensor(lst) or not isinstance(lst, (list, tuple)):
        raise ValueError("%s must be a list of per-step tensors" % name)
    if len(lst) == 0:
        raise ValueError("%s is empty" % name)
    _same_length(len(lst) if n is None else n, **{name: lst})
    for t in lst:
        if t is None:
            raise ValueError("%s holds None (continuous messages carry no probabilities: there is no REINFORCE loss for them, "
                             "model.py:1277)" % name)
        _device_tensor(t, name)
    return list(lst)


def _device_tensor(t, name):
    if not torch.is_tensor(t):
        raise ValueError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s is a CPU tensor: the loss functions run on the GPU only (there is no CPU fallback)" % name)
    return t


def _stacked(tensors, dtype=torch.float32):
    """[n, ...] contiguous stack of per-step tensors.  The consecutive unbind(0) views of one contiguous tensor are used in place."""
    first = tensors[0]
    step = first.numel()
    if first.dtype == dtype and all(t.dtype == dtype and t.shape == first.shape and t.is_contiguous()
                                    and t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
                                    and t.storage_offset() == first.storage_offset() + i * step for i, t in enumerate(tensors)):
        shape = (len(tensors),) + tuple(first.shape)
        stride = (step,) + tuple(first.stride())
        return first.detach().as_strided(shape, stride, first.storage_offset())
    if any(t.shape != first.shape for t in tensors):
        raise ValueError("the tensors of one list must have the same shape")
    return torch.stack([t.detach().to(dtype) for t in tensors]).contiguous()


def _masks(masks, n, batch):
    """None, a list of n [B, 1] masks or an already stacked [n, B, 1] tensor -> contiguous uint8 [n, B] or None."""
    if masks is None:
        return None
    if torch.is_tensor(masks):
        m = _device_tensor(masks, "masks")
        if m.size(0) != n:
            raise ValueError("masks has %d steps, %d expected" % (m.size(0), n))
        m = m.detach().to(torch.uint8)
    else:
        m = _stacked(_tensor_list(masks, "masks", n), torch.uint8)
    if m.numel() != n * batch:
        raise ValueError("a mask must hold one entry per sample")
    return m.reshape(n, batch).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _grad(g, numel):
    """An upstream gradient as a contiguous fp32 array (None = zero, a NULL pointer)."""
    if g is None:
        return None
    g = g.detach().to(torch.float32).contiguous()
    assert g.numel() == numel
    return g


# ------------------------------------------------------------------ the three autograd nodes
class _BinaryLoss(torch.autograd.Function):
    """multistep_loss_binary (model.py:907-968): (loss [1], negentropy [n]) of the stacked inputs; d / d binary_probs only."""

    @staticmethod
    def forward(ctx, feat, logs, scores, mask, penalty, *probs):
        lib = _lib.load()
        prob = _stacked(probs)
        n, B, W = prob.shape
        dev = prob.device
        loss = torch.empty(1, device=dev)
        negent = torch.empty(n, device=dev)
        save = torch.empty(int(lib.mmg_loss_save_doubles(n)), dtype=torch.float64, device=dev)
        has_ent, lam = int(penalty is not None), float(penalty or 0.0)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_loss_binary_forward(_ptr(feat), _ptr(prob), _ptr(logs), _ptr(scores), _ptr(mask), n, B, W, has_ent, lam,
                                                   _ptr(loss), _ptr(negent), _ptr(save), _stream(dev)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(feat, prob, logs, scores, mask, save)
        ctx.penalty = (has_ent, lam)
        return loss, negent

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, dnegent):
        feat, prob, logs, scores, mask, save = ctx.saved_tensors
        lib = _lib.load()
        n, B, W = prob.shape
        dev = prob.device
        dloss, dnegent = _grad(dloss, 1), _grad(dnegent, n)
        dprob = torch.empty_like(prob)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_loss_binary_vjp(_ptr(feat), _ptr(prob), _ptr(logs), _ptr(scores), _ptr(mask), _ptr(save), _ptr(dloss),
                                               _ptr(dnegent), n, B, W, ctx.penalty[0], ctx.penalty[1], _ptr(dprob), _stream(dev)))
        return (None,) * 5 + tuple(dprob.unbind(0))


class _BasLoss(torch.autograd.Function):
    """multistep_loss_bas (model.py:971-988): loss [1] of the stacked scores; d / d baseline_scores only."""

    @staticmethod
    def forward(ctx, logs, mask, *scores):
        lib = _lib.load()
        sc = _stacked(scores)
        n, B = sc.size(0), sc[0].numel()
        dev = sc.device
        loss = torch.empty(1, device=dev)
        save = torch.empty(int(lib.mmg_loss_save_doubles(n)), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_loss_bas_forward(_ptr(sc), _ptr(logs), _ptr(mask), n, B, _ptr(loss), _ptr(save), _stream(dev)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(sc, logs, mask, save)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        sc, logs, mask, save = ctx.saved_tensors
        lib = _lib.load()
        n, B = sc.size(0), sc[0].numel()
        dev = sc.device
        dloss = _grad(dloss, 1)
        dsc = torch.empty_like(sc)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_loss_bas_vjp(_ptr(sc), _ptr(logs), _ptr(mask), _ptr(save), _ptr(dloss), n, B, _ptr(dsc), _stream(dev)))
        return (None, None) + tuple(dsc.unbind(0))


class _RecOutp(torch.autograd.Function):
    """get_rec_outp (model.py:879-904) and, with a target, log_softmax / nll_loss / the reward (model.py:1264-1275): outputs
    (outp [B, D], negentropy [n]) or (outp, negentropy, nll [1], logs [B, 1]); logs is not differentiable (model.py:1274)."""

    @staticmethod
    def forward(ctx, mask, target, *ys):
        lib = _lib.load()
        y = _stacked(ys)
        n, B, D = y.shape
        dev = y.device
        outp = torch.empty(B, D, device=dev)
        negent = torch.empty(n, device=dev)
        save = torch.empty(int(lib.mmg_loss_save_doubles(n)), dtype=torch.float64, device=dev)
        nll = logs = None
        if target is not None:
            nll, logs = torch.empty(1, device=dev), torch.empty(B, 1, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_rec_outp_forward(_ptr(y), _ptr(mask), _ptr(target), n, B, D, _ptr(outp), _ptr(negent), _ptr(logs),
                                                _ptr(nll), _ptr(save), _stream(dev)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y, mask, target)
        if target is None:
            return outp, negent
        ctx.mark_non_differentiable(logs)
        return outp, negent, nll, logs

    @staticmethod
    @once_differentiable
    def backward(ctx, doutp, dnegent, dnll=None, dlogs=None):
        y, mask, target = ctx.saved_tensors
        lib = _lib.load()
        n, B, D = y.shape
        dev = y.device
        doutp, dnegent, dnll = _grad(doutp, B * D), _grad(dnegent, n), _grad(dnll, 1)
        dy = torch.empty_like(y)
        with torch.cuda.device(dev):
            _lib.check(lib.mmg_rec_outp_vjp(_ptr(y), _ptr(mask), _ptr(target), _ptr(doutp), _ptr(dnll), _ptr(dnegent), n, B, D, _ptr(dy),
                                            _stream(dev)))
        return (None, None) + tuple(dy.unbind(0))


# ------------------------------------------------------------------ the reference's functions
def _binary(binary_features, binary_probs, logs, baseline_scores, masks, entropy_penalty):
    if not isinstance(binary_probs, (list, tuple)):
        raise ValueError("binary_probs must be a list of per-step tensors")
    _same_length(len(binary_probs), binary_features=binary_features, baseline_scores=baseline_scores, masks=masks)
    probs = _tensor_list(binary_probs, "binary_probs")
    n = len(probs)
    feats = _tensor_list(binary_features, "binary_features", n)
    scores = _tensor_list(baseline_scores, "baseline_scores", n)
    _device_tensor(logs, "logs")
    if probs[0].dim() != 2:
        raise ValueError("binary_probs must hold [B, W] tensors")
    B = probs[0].size(0)
    if logs.numel() != B or scores[0].numel() != B or feats[0].shape != probs[0].shape:
        raise ValueError("binary_features / binary_probs [B, W], logs [B, 1] and baseline_scores [B, 1] must agree in B and W")
    mask = _masks(masks, n, B)
    loss, negent = _BinaryLoss.apply(_stacked(feats), logs.detach().to(torch.float32).contiguous(), _stacked(scores), mask,
                                     entropy_penalty, *probs)
    return loss.view(()), negent


def calculate_loss_binary(binary_features, binary_probs, logs, baseline_scores, entropy_penalty):
    """model.py:907-927: ``(loss, negentropy)`` of one step (both 0-dim)."""
    if binary_probs is None:
        raise ValueError("binary_probs is None (continuous messages carry no probabilities)")
    for t, name in ((binary_probs, "binary_probs"), (binary_features, "binary_features"), (baseline_scores, "baseline_scores")):
        _device_tensor(t, name)
    loss, negent = _binary([binary_features], [binary_probs], logs, [baseline_scores], None, entropy_penalty)
    return loss, negent[0]


def multistep_loss_binary(binary_features, binary_probs, logs, baseline_scores, masks, entropy_penalty):
    """model.py:930-968: ``(loss, entropies)``; entropies is the list of the steps' negentropies (0 for a step without an active
    row).  All lists must have the same length (the reference's map() would pad with None)."""
    loss, negent = _binary(binary_features, binary_probs, logs, baseline_scores, masks, entropy_penalty)
    return loss, list(negent.unbind(0))


def _bas(baseline_scores, logs, masks):
    if not isinstance(baseline_scores, (list, tuple)):
        raise ValueError("baseline_scores must be a list of per-step tensors")
    _same_length(len(baseline_scores), masks=masks)
    scores = _tensor_list(baseline_scores, "baseline_scores")
    _device_tensor(logs, "logs")
    n, B = len(scores), scores[0].numel()
    if logs.numel() != B:
        raise ValueError("baseline_scores [B, 1] and logs [B, 1] must agree in B")
    return _BasLoss.apply(logs.detach().to(torch.float32).contiguous(), _masks(masks, n, B), *scores).view(())


def calculate_loss_bas(baseline_scores, logs):
    """model.py:971-973: MSE of one step's scores against the (constant) rewards."""
    _device_tensor(baseline_scores, "baseline_scores")
    return _bas([baseline_scores], logs, None)


def multistep_loss_bas(baseline_scores, logs, masks):
    """model.py:976-988.  A step without an active row contributes 0 (its weight n_t / N is 0; the reference's indexing of an
    empty selection is undefined there)."""
    return _bas(baseline_scores, logs, masks)


def loglikelihood(log_prob, target):
    """model.py:571-577: ``log_prob.gather(1, target)`` -- [N, 1] for target [N, 1].  One device gather, differentiable in
    log_prob; the training block's reward comes out of ``reward_and_nll`` without it."""
    _device_tensor(log_prob, "log_prob")
    _device_tensor(target, "target")
    return log_prob.gather(1, target.view(log_prob.size(0), -1))


def _rec_outp(y, masks, target):
    if not isinstance(y, (list, tuple)):
        raise ValueError("y must be a list of per-step tensors")
    _same_length(len(y), masks=masks)
    ys = _tensor_list(y, "y")
    if ys[0].dim() != 2:
        raise ValueError("y must hold [B, D] tensors")
    n, B = len(ys), ys[0].size(0)
    if target is not None:
        _device_tensor(target, "target")
        if target.numel() != B:
            raise ValueError("target must hold one class per sample")
        target = target.detach().to(torch.int64).reshape(B).contiguous()
    return _RecOutp.apply(_masks(masks, n, B), target, *ys)


def get_rec_outp(y, masks):
    """model.py:879-904: ``(outp, negentropy)``: the class logits of every sample's output step -- the first step whose mask is
    set; the last step without masks and for a row no mask selects (the reference's masked_select is undefined there) -- and the
    list of the steps' mean prediction negentropies."""
    outp, negent = _rec_outp(y, masks, None)
    return outp, list(negent.unbind(0))


def reward_and_nll(y, y_masks, target):
    """model.py:1264-1275 as one node: ``(outp, negentropy, nll, logs)`` with outp [B, D], negentropy the list of get_rec_outp, nll
    = F.nll_loss(F.log_softmax(outp), target) (0-dim) and logs [B, 1] = the log-likelihood of the target, detached."""
    outp, negent, nll, logs = _rec_outp(y, y_masks, target)
    return outp, list(negent.unbind(0)), nll.view(()), logs


def training_losses(exchange_out, target, flags):
    """Mask derivation and loss totals of the training block (model.py:1248-1305) from exchange()'s return value.

    Binary messages: {"receiver", "sender", "baseline_rec", "baseline_sen"} -- the four losses to call backward() on
    (model.py:1309-1328) -- plus the six logged scalars "nll_loss", "loss_binary_s", "loss_binary_rec", "loss_binary_sen",
    "loss_bas_rec", "loss_bas_sen" (detached).  Continuous messages: {"receiver"} only (model.py:1313)."""
    s, sen_w, rec_w, y, bs, br = exchange_out
    s_masks, s_feats, s_probs = s
    sen_feats, sen_probs = sen_w
    rec_feats, rec_probs = rec_w
    n = len(y)
    if flags.fixed_exchange:                                         # model.py:1248-1254
        m_all = m_rec = y_masks = None
    else:                                                            # model.py:1255-1262, on the stacked stop masks
        m = _stacked(_tensor_list(s_masks, "s_masks", n + 1), torch.uint8)
        m_all, m_rec = m[:-1], m[1:-1]
        y_masks = torch.min(1 - m[1:], m[:-1])
    outp, _, nll, logs = reward_and_nll(y, y_masks, target)
    if not flags.use_binary:
        return {"receiver": nll}
    zero = torch.zeros((), device=nll.device)
    loss_binary_s = loss_binary_rec = zero
    if not flags.fixed_exchange:                                     # model.py:1278-1280
        loss_binary_s, _ = multistep_loss_binary(s_feats, s_probs, logs, br, m_all, flags.entropy_s)
    if n > 1:                                                        # model.py:1284-1289
        loss_binary_rec, _ = multistep_loss_binary(rec_feats[:-1], rec_probs[:-1], logs, br[:-1], m_rec, flags.entropy_rec)
    loss_binary_sen, _ = multistep_loss_binary(sen_feats, sen_probs, logs, bs, m_all, flags.entropy_sen)
    loss_bas_rec = multistep_loss_bas(br, logs, m_all)
    loss_bas_sen = multistep_loss_bas(bs, logs, m_all)
    loss_rec = nll + loss_binary_rec                                 # model.py:1296-1305
    if not flags.fixed_exchange:
        loss_rec = loss_rec + loss_binary_s
    out = {"receiver": loss_rec, "sender": loss_binary_sen, "baseline_rec": loss_bas_rec, "baseline_sen": loss_bas_sen}
    for k, v in (("nll_loss", nll), ("loss_binary_s", loss_binary_s), ("loss_binary_rec", loss_binary_rec),
                 ("loss_binary_sen", loss_binary_sen), ("loss_bas_rec", loss_bas_rec), ("loss_bas_sen", loss_bas_sen)):
        out[k] = v.detach()
    return out
