// kernels_loss.h -- the reference's loss functions as forward / vector-Jacobian kernels over ARBITRARY tensors (no mmg_config, no
// tape): what stats_pairs / loss_coefficients (kernels_bwd.h) compute for the fixed mmg_train_step configuration, reachable as
// functions.  include/mmg.h: mmg_loss_binary_*, mmg_loss_bas_*, mmg_rec_outp_*.
//
//   binary REINFORCE loss   calculate_loss_binary / multistep_loss_binary   model.py:907-968
//   baseline MSE            calculate_loss_bas / multistep_loss_bas         model.py:971-988
//   output selection + NLL  get_rec_outp, log_softmax, nll_loss, loglikelihood   model.py:879-904, 1264-1275, 571-577
//
// All data fp32; every sum over rows or over the elements of a row is formed in float64 in an order that depends on the shapes
// alone: no float atomics, no dependence on the number of compute units or on which workgroup arrives first, bit-identical from
// run to run.
//
// Geometry of a forward: grid (slots, n_steps).  The B rows of a step are cut into chunks of MMG_LOSS_ROWS rows; workgroup
// (slot, t) walks the chunks slot, slot + slots, ... of step t in ascending order (slots = min(chunks, MMG_LOSS_SLOTS)), one wave
// per row (wave w of the workgroup takes rows 8 w .. 8 w + 7 of the chunk in ascending order, its 64 lanes stride over the row
// and are added by dpp_wave_sum_d's fixed tree), and leaves its partial sums -- waves added in the order 0, 1, 2, 3 -- in the
// caller's save array.  A SECOND launch of one workgroup (k_loss_finish / k_rec_outp_finish) adds the slots of every step in
// ascending order and forms the scalars: no counter to zero, so no hipMemset and nothing to re-arm, and no in-launch wait.
// The VJPs are one elementwise launch each: they recompute what they need from the saved inputs and read the per-step
// coefficients from the save array.
//
// Save array (float64, mmg_loss_save_doubles(n) entries, caller-owned):
//   head[t][4]      n_t (active rows) | den_t (the std guard, model.py:912-915) | c_t / n_t | c_t       (0 where n_t == 0)
//   part[t][slot][MMG_LOSS_PART]   the partial sums of workgroup (slot, t)
#pragma once

namespace mmg {

#define MMG_LOSS_ROWS 32           // rows of one chunk: 4 waves x 8 rows
#define MMG_LOSS_SLOTS 64          // partial-sum slots per step
#define MMG_LOSS_HEAD 4
#define MMG_LOSS_PART 5
#define MMG_LOSS_MAX_STEPS 1024    // per-step terms of the finishing workgroup live in LDS

__host__ __device__ inline int64_t loss_save_doubles(int n) { return (int64_t)n * (MMG_LOSS_HEAD + MMG_LOSS_SLOTS * MMG_LOSS_PART); }
__host__ __device__ inline int loss_slots(int B) { const int c = (B + MMG_LOSS_ROWS - 1) / MMG_LOSS_ROWS; return c > MMG_LOSS_SLOTS ? MMG_LOSS_SLOTS : c; }
__device__ __forceinline__ double* loss_part(double* save, int n, int t, int slot) {
    return save + (size_t)n * MMG_LOSS_HEAD + ((size_t)t * MMG_LOSS_SLOTS + slot) * MMG_LOSS_PART;
}

// the four wave-uniform partial-sum vectors of a workgroup, added in wave order by thread 0 and stored to the slot
template <int K>
__device__ __forceinline__ void loss_store_part(const double (&acc)[K], double* dst) {
    __shared__ double s_part[MMG_BLOCK / 64][MMG_LOSS_PART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < K; ++k) s_part[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < MMG_LOSS_PART; ++k) {
            double v = 0.0;
            if (k < K) for (int w = 0; w < MMG_BLOCK / 64; ++w) v += s_part[w][k];
            dst[k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// (a) binary REINFORCE loss.  part = { n, sum r, sum r^2, sum r * lp, sum ne } over the active rows, r = logs - scores.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MMG_BLOCK) void k_loss_binary_part(const float* __restrict__ feat, const float* __restrict__ prob,
                                                                const float* __restrict__ logs, const float* __restrict__ scores,
                                                                const uint8_t* __restrict__ mask, int n, int B, int W,
                                                                double* __restrict__ save) {
    const int t = blockIdx.y, slot = blockIdx.x, nslot = gridDim.x;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nchunk = (B + MMG_LOSS_ROWS - 1) / MMG_LOSS_ROWS;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ch = slot; ch < nchunk; ch += nslot) {
        for (int i = 0; i < MMG_LOSS_ROWS / (MMG_BLOCK / 64); ++i) {
            const int b = ch * MMG_LOSS_ROWS + wave * (MMG_LOSS_ROWS / (MMG_BLOCK / 64)) + i;      // wave-uniform
            if (b >= B) break;
            if (mask && !mask[(size_t)t * B + b]) continue;
            const size_t row = ((size_t)t * B + b) * W;
            double lp = 0.0, ne = 0.0;
            for (int j = lane; j < W; j += 64) {
                const float p = prob[row + j], z = feat[row + j];
                const float la = logf(p + MMG_EPS), lb = logf((1.0f - p) + MMG_EPS);
                lp += (double)(z * la) + (double)((1.0f - z) * lb);
                ne += (double)(p * la) + (double)((1.0f - p) * lb);
            }
            lp = dpp_wave_sum_d(lp); ne = dpp_wave_sum_d(ne);
            const double r = (double)logs[b] - (double)scores[(size_t)t * B + b];
            acc[0] += 1.0; acc[1] += r; acc[2] += r * r; acc[3] += r * lp; acc[4] += ne;
        }
    }
    loss_store_part(acc, loss_part(save, n, t, slot));
}

// (b) baseline MSE.  part = { n, sum (scores - logs)^2 }.  A row is one float: lane i < 32 of wave 0 takes row i of every chunk of
// the workgroup in ascending chunk order, the lanes are added by the fixed tree; the other waves only join the barrier.
__global__ __launch_bounds__(MMG_BLOCK) void k_loss_bas_part(const float* __restrict__ scores, const float* __restrict__ logs,
                                                             const uint8_t* __restrict__ mask, int n, int B, double* __restrict__ save) {
    const int t = blockIdx.y, slot = blockIdx.x, nslot = gridDim.x, tid = threadIdx.x;
    const int nchunk = (B + MMG_LOSS_ROWS - 1) / MMG_LOSS_ROWS;
    double cnt = 0.0, sq = 0.0;
    if (tid < MMG_LOSS_ROWS) {
        for (int ch = slot; ch < nchunk; ch += nslot) {
            const int b = ch * MMG_LOSS_ROWS + tid;
            if (b < B && (!mask || mask[(size_t)t * B + b])) {
                const double d = (double)scores[(size_t)t * B + b] - (double)logs[b];
                cnt += 1.0; sq += d * d;
            }
        }
    }
    double acc[2] = {0.0, 0.0};
    if (tid < 64) { acc[0] = dpp_wave_sum_d(cnt); acc[1] = dpp_wave_sum_d(sq); }
    loss_store_part(acc, loss_part(save, n, t, slot));
}

// Second launch of (a) and (b): one workgroup.  Thread t adds the slots of step t in ascending order and forms the step's term;
// thread 0 then adds the steps in ascending order.  BINARY: term_t = -(sum r lp) / (den_t n_t) + lambda ne_t; else sum sq / n_t.
template <bool BINARY>
__global__ __launch_bounds__(MMG_BLOCK) void k_loss_finish(double* __restrict__ save, int n, int B, int has_mask, int has_entropy,
                                                           float lambda, float* __restrict__ loss, float* __restrict__ negent) {
    __shared__ double s_term[MMG_LOSS_MAX_STEPS], s_cnt[MMG_LOSS_MAX_STEPS];
    const int nslot = loss_slots(B);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        double s[MMG_LOSS_PART];
        for (int k = 0; k < MMG_LOSS_PART; ++k) s[k] = 0.0;
        for (int slot = 0; slot < nslot; ++slot) {
            const double* p = loss_part(save, n, t, slot);
            for (int k = 0; k < MMG_LOSS_PART; ++k) s[k] += p[k];
        }
        const double nt = s[0];
        double den = 1.0, term = 0.0, ne = 0.0;
        if (BINARY) {
            if (nt > 1.0) {                                  // unbiased std over the active rows, model.py:914-915
                const double var = (s[2] - s[1] * s[1] / nt) / (nt - 1.0);
                den = fmax(1.0, sqrt(fmax(var, 0.0)));
            }
            if (nt > 0.0) {
                ne = s[4] / nt;
                term = -(s[3] / den) / nt + (has_entropy ? (double)lambda * ne : 0.0);
            }
            negent[t] = (float)ne;
        } else if (nt > 0.0) term = s[1] / nt;
        s_term[t] = term; s_cnt[t] = nt;
        save[(size_t)t * MMG_LOSS_HEAD + 0] = nt;
        save[(size_t)t * MMG_LOSS_HEAD + 1] = den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double N = 0.0, total = 0.0;
        for (int t = 0; t < n; ++t) N += s_cnt[t];
        for (int t = 0; t < n; ++t) {
            // c_t = n_t / N with masks (model.py:960-961), 1 / n without (model.py:967); N == 0: NaN as in the reference
            const double nt = s_cnt[t], ct = has_mask ? nt / N : 1.0 / (double)n;
            if (nt > 0.0) total += ct * s_term[t];
            save[(size_t)t * MMG_LOSS_HEAD + 2] = nt > 0.0 ? ct / nt : 0.0;
            save[(size_t)t * MMG_LOSS_HEAD + 3] = nt > 0.0 ? ct : 0.0;
        }
        loss[0] = (N > 0.0) ? (float)total : __builtin_nanf("");
    }
}

// VJP of (a): dprob[t, b, j] = dloss (c_t / n_t) (-w dlp + lambda e') + dnegent[t] e' / n_t on the active rows, 0 elsewhere.
__global__ __launch_bounds__(MMG_BLOCK) void k_loss_binary_vjp(const float* __restrict__ feat, const float* __restrict__ prob,
                                                               const float* __restrict__ logs, const float* __restrict__ scores,
                                                               const uint8_t* __restrict__ mask, const double* __restrict__ save,
                                                               const float* __restrict__ dloss, const float* __restrict__ dnegent,
                                                               int n, int B, int W, int has_entropy, float lambda,
                                                               float* __restrict__ dprob) {
    const size_t total = (size_t)n * B * W, stride = (size_t)gridDim.x * blockDim.x;
    const double dl = dloss ? (double)dloss[0] : 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t rowi = i / W;                          // t * B + b
        const int t = (int)(rowi / B), b = (int)(rowi - (size_t)t * B);
        float out = 0.f;
        const double nt = save[(size_t)t * MMG_LOSS_HEAD];
        if ((!mask || mask[rowi]) && nt > 0.0) {
            const double den = save[(size_t)t * MMG_LOSS_HEAD + 1], ctnt = save[(size_t)t * MMG_LOSS_HEAD + 2];
            const double w = ((double)logs[b] - (double)scores[rowi]) / den;
            const float p = prob[i], z = feat[i];
            const float pa = p + MMG_EPS, qa = (1.0f - p) + MMG_EPS;
            const double dlp = (double)(z / pa) - (double)((1.0f - z) / qa);
            const double e = ((double)logf(pa) + (double)(p / pa)) - ((double)logf(qa) + (double)((1.0f - p) / qa));
            const double ce = (has_entropy ? dl * ctnt * (double)lambda : 0.0) + (dnegent ? (double)dnegent[t] / nt : 0.0);
            out = (float)(-dl * ctnt * w * dlp + ce * e);
        }
        dprob[i] = out;
    }
}

// VJP of (b): dscores[t, b] = dloss 2 (c_t / n_t) (scores - logs) on the active rows, 0 elsewhere.
__global__ __launch_bounds__(MMG_BLOCK) void k_loss_bas_vjp(const float* __restrict__ scores, const float* __restrict__ logs,
                                                            const uint8_t* __restrict__ mask, const double* __restrict__ save,
                                                            const float* __restrict__ dloss, int n, int B, float* __restrict__ dscores) {
    const size_t total = (size_t)n * B, stride = (size_t)gridDim.x * blockDim.x;
    const double dl = dloss ? (double)dloss[0] : 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
        float out = 0.f;
        if (!mask || mask[i])
            out = (float)(dl * 2.0 * save[(size_t)t * MMG_LOSS_HEAD + 2] * ((double)scores[i] - (double)logs[b]));
        dscores[i] = out;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// (c) output selection + NLL.  A wave owns row (t, b) of y [n, B, D].
// ------------------------------------------------------------------------------------------------------------------------
// f(value, index) over the row, lane-strided; 16 bytes per lane where the row allows (D % 4 == 0 and a 16-byte aligned base: every
// row of a contiguous y then is).  A lane meets its elements in ascending index order on either path.
template <class F>
__device__ __forceinline__ void loss_row_each(const float* __restrict__ row, int D, int lane, F f) {
    if (((D & 3) == 0) && ((((uintptr_t)row) & 15) == 0)) {
        for (int k4 = lane; k4 < (D >> 2); k4 += 64) {
            const float4 v = reinterpret_cast<const float4*>(row)[k4];
            f(v.x, 4 * k4); f(v.y, 4 * k4 + 1); f(v.z, 4 * k4 + 2); f(v.w, 4 * k4 + 3);
        }
    } else {
        for (int k = lane; k < D; k += 64) f(row[k], k);
    }
}
// the output step t*_b of sample b: the first step whose mask is set; the last step without masks or when no step is set (the
// reference's masked_select is undefined for such a row, model.py:896-900)
__device__ __forceinline__ int loss_tsel(const uint8_t* __restrict__ ymask, int n, int B, int b) {
    if (ymask)
        for (int t = 0; t < n; ++t)
            if (ymask[(size_t)t * B + b]) return t;
    return n - 1;
}
// max and sum_d exp(y_d - max) of a row (wave-uniform results)
__device__ __forceinline__ void loss_row_softmax(const float* __restrict__ row, int D, int lane, float& m, double& S) {
    float mx = -INFINITY;
    loss_row_each(row, D, lane, [&](float v, int) { mx = fmaxf(mx, v); });
    mx = dpp_wave_max(mx);
    double s = 0.0;
    loss_row_each(row, D, lane, [&](float v, int) { s += (double)expf(v - mx); });
    m = mx; S = dpp_wave_sum_d(s);
}

// part = { sum over the chunk rows of sum_d pi log(pi + eps), sum of logs[b] over the rows selected at this step }
__global__ __launch_bounds__(MMG_BLOCK) void k_rec_outp_part(const float* __restrict__ y, const uint8_t* __restrict__ ymask,
                                                             const int64_t* __restrict__ target, int n, int B, int D,
                                                             float* __restrict__ outp, float* __restrict__ logs,
                                                             double* __restrict__ save) {
    const int t = blockIdx.y, slot = blockIdx.x, nslot = gridDim.x;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nchunk = (B + MMG_LOSS_ROWS - 1) / MMG_LOSS_ROWS;
    double acc[2] = {0.0, 0.0};
    for (int ch = slot; ch < nchunk; ch += nslot) {
        for (int i = 0; i < MMG_LOSS_ROWS / (MMG_BLOCK / 64); ++i) {
            const int b = ch * MMG_LOSS_ROWS + wave * (MMG_LOSS_ROWS / (MMG_BLOCK / 64)) + i;      // wave-uniform
            if (b >= B) break;
            const float* row = y + ((size_t)t * B + b) * D;
            float m; double S;
            loss_row_softmax(row, D, lane, m, S);
            const float inv = (float)(1.0 / S);
            double ne = 0.0;
            loss_row_each(row, D, lane, [&](float v, int) { const float pi = expf(v - m) * inv; ne += (double)(pi * logf(pi + MMG_EPS)); });
            acc[0] += dpp_wave_sum_d(ne);
            if (t == loss_tsel(ymask, n, B, b)) {
                float* o = outp + (size_t)b * D;
                for (int k = lane; k < D; k += 64) o[k] = row[k];
                if (target) {
                    const int64_t tg = target[b];
                    // a target outside [0, D) is never dereferenced: its reward is NaN (the reference's gather raises)
                    const float lg = (tg >= 0 && tg < D) ? (float)((double)(row[tg] - m) - log(S)) : __builtin_nanf("");
                    if (lane == 0) logs[b] = lg;
                    acc[1] += (double)lg;
                }
            }
        }
    }
    loss_store_part(acc, loss_part(save, n, t, slot));
}

// one workgroup: negent[t] = (1 / B) sum of the step's slots; nll = -(1 / B) sum over steps and slots, both in ascending order
__global__ __launch_bounds__(MMG_BLOCK) void k_rec_outp_finish(const double* __restrict__ save, int n, int B, float* __restrict__ negent,
                                                               float* __restrict__ nll) {
    const int nslot = loss_slots(B);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        double s = 0.0;
        for (int slot = 0; slot < nslot; ++slot) s += loss_part(const_cast<double*>(save), n, t, slot)[0];
        negent[t] = (float)(s / (double)B);
    }
    if (threadIdx.x == 0 && nll) {
        double s = 0.0;
        for (int t = 0; t < n; ++t)
            for (int slot = 0; slot < nslot; ++slot) s += loss_part(const_cast<double*>(save), n, t, slot)[1];
        nll[0] = (float)(-s / (double)B);
    }
}

// dy[t, b, k] = [t == t*_b] (doutp[b, k] + dnll (pi_k - [k == target_b]) / B) + dnegent[t] pi_k (f'_k - sum_d pi_d f'_d) / B,
// f'_k = log(pi_k + eps) + pi_k / (pi_k + eps).  Rows are walked wave by wave with a grid stride.
__global__ __launch_bounds__(MMG_BLOCK) void k_rec_outp_vjp(const float* __restrict__ y, const uint8_t* __restrict__ ymask,
                                                            const int64_t* __restrict__ target, const float* __restrict__ doutp,
                                                            const float* __restrict__ dnll, const float* __restrict__ dnegent,
                                                            int n, int B, int D, float* __restrict__ dy) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t rows = (size_t)n * B, wpb = MMG_BLOCK / 64;
    for (size_t r = (size_t)blockIdx.x * wpb + wave; r < rows; r += (size_t)gridDim.x * wpb) {
        const int t = (int)(r / B), b = (int)(r - (size_t)t * B);
        const float* row = y + r * D;
        float* out = dy + r * D;
        const bool sel = t == loss_tsel(ymask, n, B, b);
        const bool want_ne = dnegent != nullptr, want_nll = sel && dnll && target;
        const float* go = (sel && doutp) ? doutp + (size_t)b * D : nullptr;
        if (!want_ne && !want_nll) {
            for (int k = lane; k < D; k += 64) out[k] = go ? go[k] : 0.f;
            continue;
        }
        float m; double S;
        loss_row_softmax(row, D, lane, m, S);
        const float inv = (float)(1.0 / S);
        double dot = 0.0;
        if (want_ne) {
            loss_row_each(row, D, lane, [&](float v, int) {
                const float pi = expf(v - m) * inv;
                dot += (double)(pi * (logf(pi + MMG_EPS) + pi / (pi + MMG_EPS)));
            });
            dot = dpp_wave_sum_d(dot);
        }
        const float gn = want_ne ? dnegent[t] / (float)B : 0.f, gl = want_nll ? dnll[0] / (float)B : 0.f;
        const int64_t tg = want_nll ? target[b] : -1;
        const float fdot = (float)dot;
        for (int k = lane; k < D; k += 64) {
            const float pi = expf(row[k] - m) * inv;
            float v = go ? go[k] : 0.f;
            if (want_nll) v += gl * (pi - ((int64_t)k == tg ? 1.f : 0.f));
            if (want_ne) v += gn * pi * ((logf(pi + MMG_EPS) + pi / (pi + MMG_EPS)) - fdot);
            out[k] = v;
        }
    }
}

}  // namespace mmg
