"""The communication profile of a dev evaluation on the host: the layout of the library's integer accumulator
(include/mmg.h: mmg_eval_steps_profile; csrc/kernels_eval.h: k_eval_profile), the same reduction restated on a tape for the torch
form of model.eval_dev, and summarise(), which turns the counts into what the reference's -binary_only dump is analysed for
(binary_vectors.py:24-46): accuracy against conversation length, conversation length per class, per-class message codes and
the information a message bit carries about the class.  Pure numpy, no GPU.

Definitions (one batch of an evaluation conversation, T steps, B samples, D classes, W message bits):
  tsel[b]    the sample's output step: Fixed mode T - 1, else #{t in 1..n-1 : mask[t, b] = 1}, n the batch's executed step count
  live       sample b is live at step t iff t <= tsel[b]
  rank_t[b]  #{d : y[min(t, tsel[b]), b, d] > y[min(t, tsel[b]), b, target[b]]}: the rank of the target had every conversation
             been cut after t + 1 steps (strict > on the fp32 logits)

Flat layout (int64, profile_count(D, T, W) = 4 + 2 D T + 2 D + 2 T D W entries):
  head [4]            [0] batches | [1] samples with a valid target | [2] samples with a target outside [0, D) | [3] 0
  steps [D, T]        samples of class c whose output step is l
  rank [T, D]         samples with rank_t = r
  class_hits [D]      samples of class c with rank_{T-1} < min(top_k, D)
  class_ranksum [D]   sum over the samples of class c of rank_{T-1}
  msg_sen [T, D, W]   samples of class c, live at t, whose sender bit j is set at step t
  msg_rec [T, D, W]   the same over the receiver's messages
A sample whose target is outside [0, D) counts in head[2] only.  Continuous messages leave msg_sen / msg_rec zero."""
import numpy as np

HEAD = 4
BLOCKS = ("steps", "rank", "class_hits", "class_ranksum", "msg_sen", "msg_rec")


def profile_count(D, T, W):
    return HEAD + 2 * D * T + 2 * D + 2 * T * D * W


def parse_profile(flat, D, T, W):
    """The named blocks of a flat profile (views of `flat` where it is a contiguous int64 array), and head / batches /
    samples / invalid."""
    flat = np.asarray(flat, np.int64).reshape(-1)
    if flat.size != profile_count(D, T, W):
        raise ValueError("a profile of D = %d, T = %d, W = %d has %d entries, not %d" % (D, T, W, profile_count(D, T, W), flat.size))
    out = dict(head=flat[:HEAD], batches=int(flat[0]), samples=int(flat[1]), invalid=int(flat[2]))
    o = HEAD
    for name, shape in (("steps", (D, T)), ("rank", (T, D)), ("class_hits", (D,)), ("class_ranksum", (D,)),
                        ("msg_sen", (T, D, W)), ("msg_rec", (T, D, W))):
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


def tape_profile(mask, z, w, y, target, top_k, fixed, binary):
    """The flat profile of ONE batch from its run-all eval tape: mask [T + 1, B], z / w [T, B, W], y [T, B, D] (numpy arrays),
    target [B] -- what k_eval_profile adds for that batch, restated for the torch form of model.eval_dev."""
    mask, y, target = np.asarray(mask).astype(np.int64), np.asarray(y), np.asarray(target).astype(np.int64).reshape(-1)
    T, B, D = y.shape
    W = np.asarray(z).shape[2]
    if fixed:
        tsel = np.full(B, T - 1, np.int64)
    else:
        dead = np.nonzero(mask[1:].sum(1) == 0)[0]
        n = int(dead[0]) + 1 if len(dead) else T
        tsel = mask[1:n].sum(0)
    p = parse_profile(np.zeros(profile_count(D, T, W), np.int64), D, T, W)
    valid = (target >= 0) & (target < D)
    p["head"][:3] = (1, int(valid.sum()), int((~valid).sum()))
    kk = min(int(top_k), D)
    for b in np.nonzero(valid)[0]:
        c, ts = int(target[b]), int(tsel[b])
        p["steps"][c, ts] += 1
        for t in range(T):
            row = y[min(t, ts), b]
            r = int((row > row[c]).sum())
            p["rank"][t, r] += 1
        p["class_hits"][c] += int(r < kk)                      # (r: rank_{T-1})
        p["class_ranksum"][c] += r
        if binary:
            for name, m in (("msg_sen", z), ("msg_rec", w)):
                p[name][:ts + 1, c] += np.rint(np.asarray(m)[:ts + 1, b]) == 1
    return np.concatenate([p["head"]] + [p[k].reshape(-1) for k in BLOCKS])


def _entropy_bits(p):
    """H(p) of a Bernoulli probability in bits, 0 log 0 = 0."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -(np.where(p > 0, p * np.log2(p), 0.0) + np.where(p < 1, (1 - p) * np.log2(1 - p), 0.0))
    return h


def summarise(profile, top_k):
    """profile: parse_profile()'s dict (EvalAccumulator.fetch()["profile"], the dict model.eval_dev(profile=...) fills).
    With N = head[1] (the samples with a valid target), n_c = sum_l steps[c, l] and live[t, c] = sum_{l >= t} steps[c, l]
    (the samples of class c that are live at step t), all in float64 and NaN where the denominator is zero:
      acc_by_step [T]      sum_{r < min(top_k, D)} rank[t, r] / N: the top-k accuracy had every conversation been cut after t + 1
                           steps; acc_by_step[T - 1] is the evaluation's top-k accuracy over the valid samples (any top_k: it
                           is formed from the rank histogram, not from class_hits)
      mrr_by_step [T]      sum_r rank[t, r] / (r + 1) / N: the mean reciprocal rank of the target
      step_counts [T]      sum_c steps[c, l]: samples whose output step is l;  step_dist = step_counts / N
      mean_steps           sum_l (l + 1) step_counts[l] / N: the mean number of exchange steps up to the output step
      class_count [D]      n_c
      class_steps [D]      sum_l (l + 1) steps[c, l] / n_c: the same mean per class
      class_acc [D]        class_hits[c] / n_c, with the top_k OF THE EVALUATION that filled the profile
      class_mean_rank [D]  class_ranksum[c] / n_c
      live [T, D]          live[t, c]
      code_sen, code_rec [T, D, W]   msg_*[t, c, j] / live[t, c]: the mean message of class c at step t over its live samples
      mi_sen, mi_rec [T, W]          I(bit; class) in bits over the samples live at t: with N_t = sum_c live[t, c],
                           p(c) = live[t, c] / N_t, q_c = code[t, c, j] and q = sum_c msg[t, c, j] / N_t,
                           I = H(q) - sum_c p(c) H(q_c),  H(p) = -p log2 p - (1 - p) log2(1 - p),  0 log 0 = 0
                           (NaN where no sample is live at t; 0 for continuous messages, whose blocks are zero)."""
    steps, rank = np.asarray(profile["steps"], np.float64), np.asarray(profile["rank"], np.float64)
    D, T = steps.shape
    N = float(profile["head"][1])
    k = min(int(top_k), D)
    with np.errstate(divide="ignore", invalid="ignore"):
        nan_div = lambda a, b: np.where(np.asarray(b) > 0, np.asarray(a, np.float64) / np.where(np.asarray(b) > 0, b, 1), np.nan)
        n_c = steps.sum(1)
        step_counts = steps.sum(0)
        live = steps[:, ::-1].cumsum(1)[:, ::-1].T                      # [T, D]
        out = dict(acc_by_step=nan_div(rank[:, :k].sum(1), N), mrr_by_step=nan_div((rank / (np.arange(D) + 1.0)).sum(1), N),
                   step_counts=step_counts.astype(np.int64), step_dist=nan_div(step_counts, N),
                   mean_steps=float(nan_div((step_counts * (np.arange(T) + 1.0)).sum(), N)),
                   class_count=n_c.astype(np.int64), class_steps=nan_div((steps * (np.arange(T) + 1.0)).sum(1), n_c),
                   class_acc=nan_div(profile["class_hits"], n_c), class_mean_rank=nan_div(profile["class_ranksum"], n_c),
                   live=live.astype(np.int64))
        N_t = live.sum(1)                                               # [T]
        p_c = nan_div(live, N_t[:, None])                               # [T, D]
        for name in ("sen", "rec"):
            msg = np.asarray(profile["msg_" + name], np.float64)       # [T, D, W]
            code = nan_div(msg, live[:, :, None])
            q = nan_div(msg.sum(1), N_t[:, None])                       # [T, W]
            cond = np.where(live[:, :, None] > 0, p_c[:, :, None] * _entropy_bits(np.nan_to_num(code)), 0.0).sum(1)
            out["code_" + name] = code
            out["mi_" + name] = np.where(N_t[:, None] > 0, _entropy_bits(np.nan_to_num(q)) - cond, np.nan)
    return out
