// kernels_eval.h -- the per-batch reductions of a dev evaluation (model.py:640-691) on the device: k_eval_reduce runs once
// behind every evaluation conversation of mmg_eval_steps, on the same stream, reads the run-all eval tape (mask, s, z, w, y)
// and the targets, and leaves INTEGERS only -- nothing floating is accumulated across samples, so the results do not depend
// on the order in which workgroups or waves arrive and are bit-reproducible.  (The one exception, continuous messages, is
// reduced in a fixed order: see "Hamming" below.)
//
// Accumulator (int64, caller-owned and caller-zeroed, shared by every batch -- of any batch size -- of one evaluation;
// mmg_eval_acc_count() entries, integer atomics):
//   [0] hits     samples whose target is among the top_k classes of the selected logits            model.py:657-668
//   [1] batches  k_eval_reduce launches added so far
//   [2] samples  samples added so far
//   [3] (zero)
//   [4, 4 + D*D)            conf[target * D + pred]: pred = argmax of the selected logits, lowest index on ties   model.py:700-709
//   [4 + D*D, 4 + D*D + D)  seen[c]: occurrences of class c as a target or as a prediction (the confusion matrix the host
//                           writes holds the classes that occur, as sklearn's does)
// Per batch, written (not accumulated) by this launch:
//   len[b] int32            conversation length sum_{t < n} s[t, b]                                 model.py:671-672
//   batch[0] int64          n: the steps the reference's exchange() executes for this batch         model.py:866
//   batch[1 + t]            ham_sen[t] = sum_b sum_j |z[t, b, j] - z[t-1, b, j]|, z[-1] = 0, every t < T   model.py:675-691
//   batch[1 + T + t]        ham_rec[t], the same over w
//     binary messages: int64 counts.  Continuous messages (use_binary == 0): the slot holds the BITS of the float64 sum.
//     Layout of that sum: ONE workgroup owns a (message, step) slot, so there is a single slot per batch and step and no
//     second pass over slots: every thread adds its elements (index tid, tid + 256, ...) in ascending order in float64, the
//     64 lanes of a wave are added by a fixed butterfly, the four wave sums in the order ((0 + 1) + (2 + 3)).
//
// The selected logits of sample b are y[tsel[b], b, :] with tsel[b] = #{t in 1..n-1 : mask[t, b] = 1} (the masks are a running
// minimum that starts at 1; model.py:870, 1261, 879-904), in Fixed mode n = T and tsel = T - 1.  A hit is
// #{d : y[d] > y[target]} < min(top_k, D) on the logits (log-softmax is monotone).  A target outside [0, D) counts as a
// sample, never as a hit, and touches neither conf nor seen.
//
// grid = eval_sample_blocks(B) + 2 T workgroups of 256 threads: sample workgroups (one wave per sample, lanes over the classes
// and over the steps; every one of them derives n from the masks itself) and one workgroup per (message, step) Hamming slot.
// No workgroup waits for another one: the launch is the same with and without the role launches (fail-soft, mmg.hip).
#pragma once

namespace mmg {

#define MMG_EVAL_ACC_HEAD 4
__host__ __device__ inline int64_t eval_acc_count(int D) { return MMG_EVAL_ACC_HEAD + (int64_t)D * D + D; }
__host__ __device__ inline int eval_sample_blocks(int B) { const int n = (B + MMG_BLOCK / 64 - 1) / (MMG_BLOCK / 64); return n > 256 ? 256 : n; }

template <class V> __device__ __forceinline__ V eval_wave_sum(V v) {          // fixed butterfly: every lane gets the total
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void eval_add(int64_t* p, int v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

__global__ __launch_bounds__(MMG_BLOCK) void k_eval_reduce(Dims dm, Tape tp, const int64_t* __restrict__ target, int top_k,
                                                           int64_t* __restrict__ acc, int32_t* __restrict__ len,
                                                           int64_t* __restrict__ batch, int n_sample_blocks) {
    __shared__ int s_alive[64];                        // [t]: some sample is alive after step t (T <= 64)
    __shared__ double s_sum[MMG_BLOCK / 64];
    __shared__ long long s_cnt[MMG_BLOCK / 64];
    const int T = dm.T, B = dm.B, D = dm.D, W = dm.W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x;
    if (blk >= n_sample_blocks) {
        // ---- one (message, step) Hamming slot
        const int slot = blk - n_sample_blocks, which = slot / T, t = slot % T;
        if (which > 1) return;
        const size_t BW = (size_t)B * W;
        const float* cur = (which ? tp.w : tp.z) + (size_t)t * BW;
        const float* prev = t > 0 ? cur - BW : cur;    // (t == 0: the zero message, prev is not read)
        if (dm.use_binary) {
            long long cnt = 0;
            for (size_t i = tid; i < BW; i += MMG_BLOCK) cnt += lrintf(fabsf(cur[i] - (t > 0 ? prev[i] : 0.f)));
            cnt = eval_wave_sum(cnt);
            if (lane == 0) s_cnt[wave] = cnt;
            __syncthreads();
            if (tid == 0) batch[1 + which * T + t] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        } else {
            double sum = 0.0;
            for (size_t i = tid; i < BW; i += MMG_BLOCK) sum += (double)fabsf(cur[i] - (t > 0 ? prev[i] : 0.f));
            sum = eval_wave_sum(sum);
            if (lane == 0) s_sum[wave] = sum;
            __syncthreads();
            if (tid == 0) batch[1 + which * T + t] = __builtin_bit_cast(int64_t, (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
        }
        return;
    }
    // ---- sample workgroups: n of the batch first (every workgroup for itself: T * B mask bytes)
    if (tid < 64) s_alive[tid] = 0;
    __syncthreads();
    if (!dm.fixed)
        for (int i = tid; i < T * B; i += MMG_BLOCK)
            if (tp.mask[(size_t)B + i]) s_alive[i / B] = 1;      // (every writer stores the same value)
    __syncthreads();
    int n = T;
    if (!dm.fixed)
        for (int t = T - 1; t >= 0; --t)
            if (s_alive[t] == 0) n = t + 1;                      // the FIRST step after which nobody is alive (model.py:866)
    if (blk == 0 && tid == 0) {
        batch[0] = n;
        eval_add(acc + 1, 1);
        eval_add(acc + 2, B);
    }
    const int kk = top_k < D ? top_k : D;
    int hits = 0;
    for (int b = blk * (MMG_BLOCK / 64) + wave; b < B; b += n_sample_blocks * (MMG_BLOCK / 64)) {
        // lanes over the steps (T <= 64): conversation length and the output step
        const int stop = (lane < n && tp.s[(size_t)lane * B + b] != 0.f) ? 1 : 0;
        const int live = (lane >= 1 && lane < n && tp.mask[(size_t)lane * B + b] != 0) ? 1 : 0;
        const int ln = eval_wave_sum(stop);
        const int tsel = dm.fixed ? T - 1 : eval_wave_sum(live);
        if (lane == 0) len[b] = ln;
        // lanes over the classes: rank of the target and the first maximum
        const float* yr = tp.y + ((size_t)tsel * B + b) * D;
        const int64_t tg = target[b];
        const bool valid = tg >= 0 && tg < D;
        const float yt = valid ? yr[tg] : 0.f;
        int above = 0, arg = 0x7fffffff;
        float best = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float v = yr[d];
            above += v > yt ? 1 : 0;
            if (arg == 0x7fffffff || v > best) { best = v; arg = d; }
        }
        above = eval_wave_sum(above);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
        }
        if (lane == 0 && valid) {
            hits += above < kk ? 1 : 0;
            eval_add(acc + MMG_EVAL_ACC_HEAD + tg * D + arg, 1);
            eval_add(acc + MMG_EVAL_ACC_HEAD + (int64_t)D * D + tg, 1);
            eval_add(acc + MMG_EVAL_ACC_HEAD + (int64_t)D * D + arg, 1);
        }
    }
    if (lane == 0 && hits) eval_add(acc, hits);
}

// ---------------------------------------------------------------------------------------------
// k_eval_profile -- the communication profile of a dev evaluation: what the reference's -binary_only dump stores per sample and
// step (the rank of the target, the stop bit, both messages; binary_vectors.py:24-46, 89-141) and what its notebook and the
// paper's figures derive from that dump (accuracy against conversation length, conversation length per class, per-class message
// codes), reduced on the device into INTEGER counts.  One launch behind k_eval_reduce of mmg_eval_steps_profile, on the same
// stream; it reads only the plain tape arrays mask, z, w, y and the targets, so it serves every handle kind.
//
// Per sample b: tsel[b] and n as k_eval_reduce derives them; c = target[b]; the sample is LIVE at step t iff t <= tsel[b];
//   rank_t[b] = #{d : y[min(t, tsel[b]), b, d] > y[min(t, tsel[b]), b, c]}   for t = 0 .. T - 1
// (the rank of the target had every conversation been cut after t + 1 steps; a sample that stopped earlier keeps its own answer;
// strict > on the fp32 logits, so rank_{T-1} is the rank k_eval_reduce's hit is formed from).
//
// Accumulator prof (int64, caller-owned and caller-zeroed, shared by every batch -- of any batch size -- of one evaluation;
// eval_profile_count() entries, integer atomics only):
//   head [4]                [0] batches added, [1] samples with a valid target, [2] samples with a target outside [0, D), [3] 0
//   steps [D, T]            samples of class c whose output step is l
//   rank [T, D]             samples with rank_t[b] = r
//   class_hits [D]          samples of class c with rank_{T-1}[b] < min(top_k, D)
//   class_ranksum [D]       sum over the samples of class c of rank_{T-1}[b]
//   msg_sen [T, D, W]       samples of class c, live at t, with lrintf(z[t, b, j]) == 1
//   msg_rec [T, D, W]       the same over w
// A sample with a target outside [0, D) counts in head[2] only.  Continuous messages (use_binary == 0): msg_sen / msg_rec are
// not touched.  The denominator of the code book -- the samples of class c live at t -- is sum_{l >= t} steps[c, l].
//
// grid = eval_sample_blocks(B) workgroups of 256 threads, a wave per sample: lanes over the steps for tsel, lanes over the classes
// for each of the tsel + 1 distinct ranks (lane t keeps rank_t, so the T adds into rank[] are one atomic per lane), lanes over the
// W bits of every live step for the code book.  No LDS beyond the step flags, no workgroup waits for another one.
// ---------------------------------------------------------------------------------------------
#define MMG_EVAL_PROF_HEAD 4
__host__ __device__ inline int64_t eval_profile_count(int D, int T, int W) {
    return MMG_EVAL_PROF_HEAD + 2 * (int64_t)D * T + 2 * (int64_t)D + 2 * (int64_t)T * D * W;
}

__global__ __launch_bounds__(MMG_BLOCK) void k_eval_profile(Dims dm, Tape tp, const int64_t* __restrict__ target, int top_k,
                                                            int64_t* __restrict__ prof, int n_sample_blocks) {
    __shared__ int s_alive[64];                        // [t]: some sample is alive after step t (T <= 64)
    const int T = dm.T, B = dm.B, D = dm.D, W = dm.W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x;
    if (blk >= n_sample_blocks) return;
    // ---- n of the batch, as k_eval_reduce forms it
    if (tid < 64) s_alive[tid] = 0;
    __syncthreads();
    if (!dm.fixed)
        for (int i = tid; i < T * B; i += MMG_BLOCK)
            if (tp.mask[(size_t)B + i]) s_alive[i / B] = 1;
    __syncthreads();
    int n = T;
    if (!dm.fixed)
        for (int t = T - 1; t >= 0; --t)
            if (s_alive[t] == 0) n = t + 1;
    if (blk == 0 && tid == 0) eval_add(prof, 1);
    int64_t* p_steps = prof + MMG_EVAL_PROF_HEAD;
    int64_t* p_rank = p_steps + (int64_t)D * T;
    int64_t* p_hits = p_rank + (int64_t)T * D;
    int64_t* p_rsum = p_hits + D;
    int64_t* p_sen = p_rsum + D;
    int64_t* p_rec = p_sen + (int64_t)T * D * W;
    const int kk = top_k < D ? top_k : D;
    int n_valid = 0, n_invalid = 0;
    for (int b = blk * (MMG_BLOCK / 64) + wave; b < B; b += n_sample_blocks * (MMG_BLOCK / 64)) {
        const int64_t tg = target[b];
        if (!(tg >= 0 && tg < D)) { ++n_invalid; continue; }       // (wave-uniform)
        ++n_valid;
        // lanes over the steps (T <= 64): the output step
        const int live = (lane >= 1 && lane < n && tp.mask[(size_t)lane * B + b] != 0) ? 1 : 0;
        const int tsel = dm.fixed ? T - 1 : eval_wave_sum(live);
        // lanes over the classes, once per live step: lane t keeps rank_t, the lanes behind the output step keep its rank
        int mine = 0, above = 0;
        for (int t = 0; t <= tsel; ++t) {
            const float* yr = tp.y + ((size_t)t * B + b) * D;
            const float yt = yr[tg];
            above = 0;
            for (int d = lane; d < D; d += 64) above += yr[d] > yt ? 1 : 0;
            above = eval_wave_sum(above);
            if (lane == t) mine = above;
        }
        if (lane > tsel) mine = above;                               // (above: rank_{tsel} = rank_{T-1}, on every lane)
        if (lane < T) eval_add(p_rank + (int64_t)lane * D + mine, 1);
        if (lane == 0) {
            eval_add(p_steps + tg * T + tsel, 1);
            if (above < kk) eval_add(p_hits + tg, 1);
            if (above) eval_add(p_rsum + tg, above);
        }
        // lanes over the bits of every live step: the per-class code book
        if (dm.use_binary)
            for (int t = 0; t <= tsel; ++t) {
                const size_t row = ((size_t)t * B + b) * W;
                const int64_t slot = ((int64_t)t * D + tg) * W;
                for (int j = lane; j < W; j += 64) {
                    if (lrintf(tp.z[row + j]) == 1) eval_add(p_sen + slot + j, 1);
                    if (lrintf(tp.w[row + j]) == 1) eval_add(p_rec + slot + j, 1);
                }
            }
    }
    if (lane == 0 && n_valid) eval_add(prof + 1, n_valid);
    if (lane == 0 && n_invalid) eval_add(prof + 2, n_invalid);
}

// ---------------------------------------------------------------------------------------------
// k_eval_codes -- every sample's own code of a dev evaluation: the bits of both agents' messages the -binary_only dump stores per
// sample and step (binary_vectors.py:101-126), packed 32 to a word, for the pairwise analysis of kernels_pairs.h (which needs every
// sample's code, not the per-class sums of k_eval_profile).  One launch behind k_eval_reduce (and k_eval_profile) of
// mmg_eval_steps_codes, on the same stream; it reads only the plain tape arrays mask, z, w and the targets, so it serves every
// handle kind, and a corruption mask or flipout_dev flips are packed as the receiver saw them.  Binary messages only.
//
// Per sample b, WRITTEN (not accumulated) at row = the launch's first row + b; n and tsel[b] as k_eval_reduce derives them:
//   codes[row][agent][t][k] uint32, agent 0 = the sender's z, 1 = the receiver's w, t < T, k < Wp = eval_code_wp(W):
//                           bit (j & 31) of word (j >> 5) is set iff lrintf(msg[t, b, j]) == 1 and t <= tsel[b]; the steps behind
//                           the output step and the padding bits of the last word are zero.  EVERY word of the row is written.
//   meta[row][2] int32      tsel[b] | target[b], or -1 for a target outside [0, D)
//
// grid = eval_sample_blocks(B) workgroups of 256 threads, a wave per sample: lanes over the steps for tsel, then lanes over 64 bits
// of a message at a time -- the wave's ballot IS the two code words.  No LDS beyond the step flags, no atomics, no workgroup waits
// for another one.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int eval_code_wp(int W) { return (W + 31) / 32; }
__host__ __device__ inline int64_t eval_code_words(int T, int W) { return 2 * (int64_t)T * eval_code_wp(W); }

__global__ __launch_bounds__(MMG_BLOCK) void k_eval_codes(Dims dm, Tape tp, const int64_t* __restrict__ target,
                                                          uint32_t* __restrict__ codes, int32_t* __restrict__ meta,
                                                          int n_sample_blocks) {
    __shared__ int s_alive[64];                        // [t]: some sample is alive after step t (T <= 64)
    const int T = dm.T, B = dm.B, D = dm.D, W = dm.W, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x;
    if (blk >= n_sample_blocks) return;
    // ---- n of the batch, as k_eval_reduce forms it
    if (tid < 64) s_alive[tid] = 0;
    __syncthreads();
    if (!dm.fixed)
        for (int i = tid; i < T * B; i += MMG_BLOCK)
            if (tp.mask[(size_t)B + i]) s_alive[i / B] = 1;
    __syncthreads();
    int n = T;
    if (!dm.fixed)
        for (int t = T - 1; t >= 0; --t)
            if (s_alive[t] == 0) n = t + 1;
    const int Wp = eval_code_wp(W);
    for (int b = blk * (MMG_BLOCK / 64) + wave; b < B; b += n_sample_blocks * (MMG_BLOCK / 64)) {
        const int live = (lane >= 1 && lane < n && tp.mask[(size_t)lane * B + b] != 0) ? 1 : 0;
        const int tsel = dm.fixed ? T - 1 : eval_wave_sum(live);
        if (lane == 0) {
            const int64_t tg = target[b];
            meta[(size_t)b * 2] = tsel;
            meta[(size_t)b * 2 + 1] = (tg >= 0 && tg < D) ? (int32_t)tg : -1;
        }
        uint32_t* out = codes + (size_t)b * (2 * T * Wp);
        for (int a = 0; a < 2; ++a) {
            const float* msg = a ? tp.w : tp.z;
            for (int t = 0; t < T; ++t)
                for (int k0 = 0; k0 < Wp; k0 += 2) {                   // (wave-uniform loops: the ballot sees all 64 lanes)
                    const int j = k0 * 32 + lane;
                    const bool bit = t <= tsel && j < W && lrintf(msg[((size_t)t * B + b) * W + j]) == 1;
                    const unsigned long long word = __ballot(bit);
                    if (lane == 0) out[((size_t)a * T + t) * Wp + k0] = (uint32_t)word;
                    if (lane == 1 && k0 + 1 < Wp) out[((size_t)a * T + t) * Wp + k0 + 1] = (uint32_t)(word >> 32);
                }
        }
    }
}

}  // namespace mmg
