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
A sample whose target is outside [0, D) counts in head[2] only.  Continuous messages leave msg_sen / msg_rec zero.

The second half of the module is the PAIRWISE analysis (mmg_eval_steps_codes, mmg_code_pair_hist): pack_codes, pair_hist_np and
topsim() -- topographic similarity, class separation, collisions; its layouts stand in front of it."""
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


# ---------------------------------------------------------------------------------------------
# Pairwise code analysis (include/mmg.h: mmg_eval_steps_codes, mmg_code_pair_hist; csrc/kernels_eval.h: k_eval_codes,
# csrc/kernels_pairs.h): every sample's own code, the joint histogram of (same class?, Hamming distance of two codes, cosine
# distance of two meanings) over all unordered pairs of samples, and what is read off it -- topographic similarity, class
# separation, collisions.  The codes are the bits the -binary_only dump stores per sample and step (binary_vectors.py:101-126).
#
#   codes [rows, 2, T, Wp] uint32   agent 0 the sender's z, 1 the receiver's w; Wp = (W + 31) // 32; bit (j & 31) of word (j >> 5)
#                                   is set iff rint(msg[t, b, j]) == 1 and t <= tsel[b]; dead steps and padding bits are zero
#   meta [rows, 2] int32            tsel[b] | target[b], or -1 for a target outside [0, D)
#   flat histogram, int64, pair_hist_count() = 4 + 2 (M + 1) K entries, M = (t1 - t0) W selected bits, K bins:
#     head [4]            [0] rows used | [1] rows skipped (meta target -1) | [2] pairs counted = used (used - 1) / 2 | [3] 0
#     hist [2, M + 1, K]  hist[p, h, q]: pairs i < j of used rows with p = (target_i == target_j), Hamming distance h over the
#                         selected steps, and q = min(K - 1, max(0, floor((1 - cos(x_i, x_j)) K / 2))); a zero row has cos = 0
# ---------------------------------------------------------------------------------------------
CODE_BITS = 32
PAIR_HEAD = 4


def code_words(T, W):
    """uint32 words of one sample's row of codes: 2 agents x T steps x ceil(W / 32)."""
    return 2 * int(T) * ((int(W) + CODE_BITS - 1) // CODE_BITS)


def pack_codes(mask, z, w, target, fixed, n_classes=None):
    """(codes [B, 2, T, Wp] uint32, meta [B, 2] int32) of ONE batch from its run-all eval tape: mask [T + 1, B], z / w [T, B, W],
    target [B] -- what k_eval_codes writes for that batch.  n_classes: targets outside [0, n_classes) become -1 (None: negative
    targets only)."""
    mask, target = np.asarray(mask).astype(np.int64), np.asarray(target).astype(np.int64).reshape(-1)
    z, w = np.asarray(z), np.asarray(w)
    T, B, W = z.shape
    if fixed:
        tsel = np.full(B, T - 1, np.int64)
    else:
        dead = np.nonzero(mask[1:].sum(1) == 0)[0]
        n = int(dead[0]) + 1 if len(dead) else T
        tsel = mask[1:n].sum(0)
    Wp = (W + CODE_BITS - 1) // CODE_BITS
    live = np.arange(T)[:, None] <= tsel[None, :]                               # [T, B]
    codes = np.zeros((B, 2, T, Wp), np.uint32)
    shifts = np.arange(CODE_BITS, dtype=np.uint64)
    for a, msg in enumerate((z, w)):
        bits = np.zeros((T, B, Wp * CODE_BITS), np.uint64)
        bits[:, :, :W] = (np.rint(msg) == 1) & live[:, :, None]
        words = (bits.reshape(T, B, Wp, CODE_BITS) << shifts).sum(3)            # [T, B, Wp]
        codes[:, a] = words.transpose(1, 0, 2).astype(np.uint32)
    valid = (target >= 0) & ((target < n_classes) if n_classes is not None else True)
    meta = np.stack([tsel, np.where(valid, target, -1)], 1).astype(np.int32)
    return codes, meta


def pair_hist_count(n_sel_steps, W, bins):
    return PAIR_HEAD + 2 * (int(n_sel_steps) * int(W) + 1) * int(bins)


def parse_pair_hist(flat, n_sel_steps, W, bins):
    """The parts of a flat pair histogram: head, used / skipped / pairs, hist [2, M + 1, K] (a view of `flat` where it is a
    contiguous int64 array; plane 0 the pairs of different classes, plane 1 those of the same class)."""
    flat = np.asarray(flat, np.int64).reshape(-1)
    M, K = int(n_sel_steps) * int(W), int(bins)
    if flat.size != pair_hist_count(n_sel_steps, W, bins):
        raise ValueError("a pair histogram of %d selected bits and %d bins has %d entries, not %d"
                         % (M, K, pair_hist_count(n_sel_steps, W, bins), flat.size))
    return dict(head=flat[:PAIR_HEAD], used=int(flat[0]), skipped=int(flat[1]), pairs=int(flat[2]),
                hist=flat[PAIR_HEAD:].reshape(2, M + 1, K))


def _code_bits(words):
    """[n, nw] uint32 -> [n, 32 nw] float64 of 0 / 1 (the bit order does not matter for a Hamming distance)."""
    words = np.ascontiguousarray(words)
    words = np.ascontiguousarray(words.view(np.uint32) if words.dtype == np.int32 else words, dtype="<u4")     # (int32: torch's view of the words)
    return np.unpackbits(words.view(np.uint8), axis=1).astype(np.float64)


def pair_hist_np(codes, meta, meaning, agent, t0, t1, bins, W=None, block=512):
    """mmg_code_pair_hist restated: the flat histogram of codes [N, 2, T, Wp] / meta [N, 2] against the cosine distance of the
    rows of meaning [N, F], with the cosine in float64 (c = dot(x_i, x_j) * (inv_i * inv_j), inv = 1 / sqrt(sum x^2), 0 for a zero
    row).  W: the message width (default 32 Wp: then M counts the padding bits too).  Rows are walked in blocks of `block`."""
    codes, meta = np.asarray(codes), np.asarray(meta)
    N, _, T, Wp = codes.shape
    W = Wp * CODE_BITS if W is None else int(W)
    if not (agent in (0, 1) and 0 <= t0 < t1 <= T and bins >= 1):
        raise ValueError("agent must be 0 or 1, 0 <= t0 < t1 <= T, bins >= 1")
    M, K = (t1 - t0) * W, int(bins)
    tgt = meta[:, 1].astype(np.int64)
    used = np.nonzero(tgt >= 0)[0]
    n = len(used)
    flat = np.zeros(pair_hist_count(t1 - t0, W, K), np.int64)
    flat[:3] = (n, N - n, n * (n - 1) // 2)
    x = np.asarray(meaning, np.float64)[used]
    ss = (x * x).sum(1)
    inv = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)
    bits = _code_bits(codes[used, agent, t0:t1].reshape(n, -1))
    ones = bits.sum(1)
    tg = tgt[used]
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        c = (x[i0:i1] @ x[i0:].T) * (inv[i0:i1, None] * inv[None, i0:])
        q = np.clip(np.floor((1.0 - c) * (0.5 * K)), 0, K - 1).astype(np.int64)
        h = np.rint(ones[i0:i1, None] + ones[None, i0:] - 2.0 * (bits[i0:i1] @ bits[i0:].T)).astype(np.int64)
        p = (tg[i0:i1, None] == tg[None, i0:]).astype(np.int64)
        keep = np.arange(i1 - i0)[:, None] < np.arange(n - i0)[None, :]          # i < j
        slot = ((p * (M + 1) + h) * K + q)[keep]
        flat[PAIR_HEAD:] += np.bincount(slot, minlength=2 * (M + 1) * K)
    return flat


def _midranks(counts):
    """Mid-ranks (1-based) of the values of a marginal histogram."""
    counts = np.asarray(counts, np.float64)
    return np.cumsum(counts) - counts + (counts + 1.0) / 2.0


def _weighted_pearson(J, a, b):
    """Pearson correlation of the row scores a and column scores b under the joint counts J; nan without variance."""
    n = J.sum()
    if n <= 0:
        return float("nan")
    ra, rb = J.sum(1), J.sum(0)
    da, db = a - (ra * a).sum() / n, b - (rb * b).sum() / n
    va, vb = (ra * da * da).sum(), (rb * db * db).sum()
    if not (va > 0 and vb > 0):
        return float("nan")
    return float((J * da[:, None] * db[None, :]).sum() / np.sqrt(va * vb))


def topsim(hist):
    """What is read off a pair histogram (parse_pair_hist()'s dict, or its hist [2, M + 1, K]): dict of
      n_pairs        the pairs counted
      spearman       topographic similarity: the mid-rank Spearman correlation of (h, q) over all pairs -- Pearson over the
                     mid-ranks of the two marginals, weighted by the joint counts (= scipy.stats.spearmanr on the expanded pairs)
      pearson        h against the bin centres (q + 1/2) 2 / K of the cosine distance
      hamming_same, hamming_diff    mean Hamming distance of the same-class / different-class pairs
      separation     P(h_diff > h_same) + 1/2 P(h_diff == h_same) for a random different-class and a random same-class pair
      collisions     different-class pairs with identical codes (h == 0)
    each nan where undefined (an empty plane, zero variance)."""
    H = np.asarray(hist["hist"] if isinstance(hist, dict) else hist, np.float64)
    if H.ndim != 3 or H.shape[0] != 2:
        raise ValueError("a pair histogram is [2, M + 1, K]")
    _, M1, K = H.shape
    J = H[0] + H[1]
    hs = np.arange(M1, dtype=np.float64)
    diff, same = H[0].sum(1), H[1].sum(1)
    nd, ns = diff.sum(), same.sum()
    nan = float("nan")
    sep = nan
    if nd > 0 and ns > 0:
        below = np.cumsum(same) - same                                           # same-class pairs with a smaller h
        sep = float((diff * (below + 0.5 * same)).sum() / (nd * ns))
    return dict(n_pairs=int(round(J.sum())),
                spearman=_weighted_pearson(J, _midranks(J.sum(1)), _midranks(J.sum(0))),
                pearson=_weighted_pearson(J, hs, (np.arange(K) + 0.5) * (2.0 / K)),
                hamming_same=float((same * hs).sum() / ns) if ns > 0 else nan,
                hamming_diff=float((diff * hs).sum() / nd) if nd > 0 else nan,
                separation=sep, collisions=int(round(H[0, 0].sum())))
