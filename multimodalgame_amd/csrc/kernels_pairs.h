// kernels_pairs.h -- the pairwise code analysis of a dev evaluation: the joint histogram of (same class?, Hamming distance of two
// samples' codes, cosine distance of their meanings) over ALL unordered pairs of samples, from which the host forms topographic
// similarity (the rank correlation of the two distances), class separation and code collisions (commstats.topsim).  O(N^2) in the
// dev set, so it runs on the device; handle-free like kernels_loss.h -- the arithmetic depends on no mmg_config.
//
// Inputs: codes [n_rows][2][T][Wp] uint32 and meta [n_rows][2] int32 as k_eval_codes (kernels_eval.h) leaves them -- what the codes
// stand for: binary_vectors.py:101-126 -- and a meaning matrix x [n_rows, F] fp32 with row stride ld: the image features give the
// image-level measure, desc[target] the class-level one.  Finite inputs are the caller's duty.
//
// k_pair_norms: inv[i] = 1 / sqrt(sum_k x_ik^2) in fp32, 0 for a zero row; adds head[0] = rows used, head[1] = rows skipped (meta
// target -1).  A wave per row.
//
// k_pair_hist: with M = (t1 - t0) * W and K bins, for every unordered pair i < j of used rows ONE integer is added to
//   hist[p][h][q],  p = (target_i == target_j),  h = sum_{t0 <= t < t1} sum_k popc(code_i[agent][t][k] ^ code_j[agent][t][k]),
//   c = dot(x_i, x_j) * (inv_i * inv_j),  u = (1 - c) * (0.5 K),  q = min(K - 1, max(0, floor(u)))      (fp32, each op rounded once)
// (identical rows give c = 1 +- ulp and opposite rows u = K: the clamps; a zero row gives c = 0), and head[2] += the pairs counted.
// The array is int64, caller-zeroed, 4 + 2 (M + 1) K entries (pair_hist_count); integers only are added, so the result does not
// depend on the order in which workgroups arrive.
//
// One workgroup owns one 64 x 64 tile of the upper triangle of the pair matrix (grid linearised over the tile pairs bi <= bj; a
// diagonal tile counts i < j only; rows beyond n_rows and skipped rows count nothing).  The Gram tile runs on the matrix cores
// (mfma16: v_mfma_f32_16x16x4_f32, as k_vjp_ddesc uses it): each of the four waves owns 16 x 64 of the tile, four accumulator
// tiles; both operands are staged through LDS in chunks of MMG_PAIR_KC columns (an F that is no multiple of the chunk is padded with
// zeros).  A lane feeds k = 16 g + 4 q + u to k-slot q of MFMA step u of group g -- a permutation of the columns that is the same
// for both operands, so the lane's four steps read ONE 16-byte LDS word per operand row.  The selected code words of the tile's 128
// rows (contiguous in a row: [t0, t1) x Wp) sit in LDS where they fit, else they are read from global memory.  Counts go into a
// workgroup-private LDS histogram of 32-bit counters where 2 (M + 1) K of them fit beside the operands (a tile adds at most 4096 to
// a slot), flushed with one 64-bit atomic per non-zero slot; otherwise straight to global 64-bit atomics.  Both routes give
// identical integers.  No workgroup waits for another one.
#pragma once
#include "device_utils.h"

namespace mmg {

#define MMG_PAIR_HEAD 4
#define MMG_PAIR_TILE 64
#define MMG_PAIR_KC 32                        // columns of the meaning matrix per LDS chunk
#define MMG_PAIR_LDK (MMG_PAIR_KC + 4)        // row stride of the staged operands (floats; rows stay 16-byte aligned)
// dynamic LDS a launch may take -- the code words, then the histogram: what a workgroup's 160 KB leave beside the 19 456 static bytes
// (operand chunks, classes, inverse norms).  Measured ("Pairwise code analysis"): a histogram of a few thousand slots on
// the global route is an order of magnitude slower than in LDS (its atomics pile up on few addresses), so everything that fits stays
// in LDS; only tens of thousands of slots spread the global atomics enough.  (-DMMG_PAIR_DYN_BYTES=...: for that A/B.)
#ifndef MMG_PAIR_DYN_BYTES
#define MMG_PAIR_DYN_BYTES (160 * 1024 - 19456)
#endif
#define MMG_PAIR_MAX_ROWS 65536
#define MMG_PAIR_MAX_F 4096
#define MMG_PAIR_MAX_BINS 1024
#define MMG_PAIR_MAX_SLOTS (1 << 24)

__host__ __device__ inline int64_t pair_hist_slots(int64_t M, int K) { return 2 * (M + 1) * (int64_t)K; }
__host__ __device__ inline int64_t pair_hist_count(int64_t M, int K) { return MMG_PAIR_HEAD + pair_hist_slots(M, K); }
// dynamic LDS layout of k_pair_hist: [code words: 128 rows x cstride, if they fit] [histogram: slots uint32, if it fits behind them]
__host__ __device__ inline int pair_code_stride(int nw) { return nw | 1; }      // (odd: the 16 rows a wave reads fall into 16 banks)
__host__ __device__ inline bool pair_codes_in_lds(int nw) { return (int64_t)2 * MMG_PAIR_TILE * pair_code_stride(nw) * 4 <= MMG_PAIR_DYN_BYTES; }
__host__ __device__ inline int64_t pair_code_lds_bytes(int nw) { return pair_codes_in_lds(nw) ? (int64_t)2 * MMG_PAIR_TILE * pair_code_stride(nw) * 4 : 0; }
__host__ __device__ inline bool pair_hist_in_lds(int nw, int64_t slots) { return pair_code_lds_bytes(nw) + slots * 4 <= MMG_PAIR_DYN_BYTES; }

__device__ __forceinline__ void pair_add(int64_t* p, unsigned long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), v); }

__global__ __launch_bounds__(MMG_BLOCK) void k_pair_norms(const float* __restrict__ x, int64_t ld, int F, const int32_t* __restrict__ meta,
                                                          int n_rows, float* __restrict__ inv, int64_t* __restrict__ head) {
    __shared__ int s_used[MMG_BLOCK / 64], s_skip[MMG_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * (MMG_BLOCK / 64) + wave;
    int used = 0, skip = 0;
    if (row < n_rows) {
        const float* xr = x + (size_t)row * ld;
        float s = 0.f;
        for (int k = lane; k < F; k += 64) s = fmaf(xr[k], xr[k], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) inv[row] = s > 0.f ? 1.f / sqrtf(s) : 0.f;
        used = meta[(size_t)row * 2 + 1] >= 0 ? 1 : 0;
        skip = 1 - used;
    }
    if (lane == 0) { s_used[wave] = used; s_skip[wave] = skip; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int u = (s_used[0] + s_used[1]) + (s_used[2] + s_used[3]), k = (s_skip[0] + s_skip[1]) + (s_skip[2] + s_skip[3]);
        if (u) pair_add(head, (unsigned long long)u);
        if (k) pair_add(head + 1, (unsigned long long)k);
    }
}

// Hamming distances of the lane's 4 x 4 pairs: rows a[r] (r < 4) against rows b[j] (j < 4), nw words each
__device__ __forceinline__ void pair_hamming(const uint32_t* (&a)[4], const uint32_t* (&b)[4], int nw, int (&h)[4][4]) {
    for (int w = 0; w < nw; ++w) {
        uint32_t av[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { av[r] = a[r][w]; bv[r] = b[r][w]; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[j][r] += __popc(av[r] ^ bv[j]);
    }
}

struct PairArgs {
    const uint32_t* codes;     // [n_rows][2][T][Wp]
    const int32_t* meta;       // [n_rows][2]
    const float* x;            // [n_rows, F], row stride ld
    const float* inv;          // [n_rows]
    int64_t* hist;             // [4 + 2 (M + 1) K]
    int64_t ld;
    int64_t row_words;         // 2 T Wp
    int64_t sel0;              // (agent T + t0) Wp: the first selected word of a row
    int n_rows, F, nw, M, K, n_tiles;
    int codes_lds, hist_lds;   // the routes the host chose (pair_codes_in_lds, pair_hist_in_lds)
};

__global__ __launch_bounds__(MMG_BLOCK) void k_pair_hist(PairArgs ar) {
    __shared__ __attribute__((aligned(16))) float s_a[MMG_PAIR_TILE][MMG_PAIR_LDK];
    __shared__ __attribute__((aligned(16))) float s_b[MMG_PAIR_TILE][MMG_PAIR_LDK];
    __shared__ float s_inv[2 * MMG_PAIR_TILE];
    __shared__ int s_tgt[2 * MMG_PAIR_TILE];              // the row's class; -1: the row counts nothing
    extern __shared__ uint32_t s_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int n = ar.n_rows, F = ar.F, nw = ar.nw, K = ar.K;
    // ---- the tile pair bi <= bj of this workgroup: p = bj (bj + 1) / 2 + bi
    const int p = blockIdx.x;
    int bj = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);       // (p < 2^20: the float is exact up to the root's rounding)
    while ((bj + 1) * (bj + 2) / 2 <= p) ++bj;
    while (bj * (bj + 1) / 2 > p) --bj;
    const int bi = p - bj * (bj + 1) / 2;
    const int I0 = bi * MMG_PAIR_TILE, J0 = bj * MMG_PAIR_TILE;
    const int cstride = pair_code_stride(nw);
    uint32_t* s_codes = s_dyn;
    uint32_t* s_hist = s_dyn + (ar.codes_lds ? 2 * MMG_PAIR_TILE * cstride : 0);
    const int slots = 2 * (ar.M + 1) * K;
    // ---- rows of the tile: classes, inverse norms, code words; the private histogram starts at zero
    if (tid < 2 * MMG_PAIR_TILE) {
        const int g = (tid < MMG_PAIR_TILE ? I0 : J0 - MMG_PAIR_TILE) + tid;
        s_tgt[tid] = g < n ? ar.meta[(size_t)g * 2 + 1] : -1;
        s_inv[tid] = g < n ? ar.inv[g] : 0.f;
    }
    if (ar.codes_lds)
        for (int e = tid; e < 2 * MMG_PAIR_TILE * nw; e += MMG_BLOCK) {
            const int r = e / nw, w = e - r * nw;
            const int g = min((r < MMG_PAIR_TILE ? I0 : J0 - MMG_PAIR_TILE) + r, n - 1);       // (clamped rows: read, never counted)
            s_codes[r * cstride + w] = ar.codes[(size_t)g * ar.row_words + ar.sel0 + w];
        }
    if (ar.hist_lds)
        for (int e = tid; e < slots; e += MMG_BLOCK) s_hist[e] = 0u;
    // ---- the Gram tile: rows I0 + 16 wave + .. against columns J0 + 16 j + .., chunks of MMG_PAIR_KC columns of x through LDS
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < F; k0 += MMG_PAIR_KC) {
        __syncthreads();                                   // the previous chunk has been read
        for (int e = tid; e < MMG_PAIR_TILE * MMG_PAIR_KC; e += MMG_BLOCK) {
            const int r = e / MMG_PAIR_KC, k = e - r * MMG_PAIR_KC;
            const bool kok = k0 + k < F;
            const int kc = kok ? k0 + k : 0;
            const float va = ar.x[(size_t)min(I0 + r, n - 1) * ar.ld + kc], vb = ar.x[(size_t)min(J0 + r, n - 1) * ar.ld + kc];
            s_a[r][k] = (kok && I0 + r < n) ? va : 0.f;
            s_b[r][k] = (kok && J0 + r < n) ? vb : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < MMG_PAIR_KC / 16; ++g) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&s_a[16 * wave + i][16 * g + 4 * q]);
            f32x4 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const f32x4*>(&s_b[16 * j + i][16 * g + 4 * q]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[j] = mfma16(a.x, b[j].x, acc[j]); acc[j] = mfma16(a.y, b[j].y, acc[j]);
                acc[j] = mfma16(a.z, b[j].z, acc[j]); acc[j] = mfma16(a.w, b[j].w, acc[j]);
            }
        }
    }
    __syncthreads();                                       // s_tgt, s_inv, s_codes, s_hist are in place (F >= 1: also behind the loop's barriers)
    // ---- the lane's 16 pairs: accumulator tile j, register r = row 16 wave + 4 q + r of the I block, column 16 j + i of the J block
    int h[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[j][r] = 0;
    if (ar.codes_lds) {
        const uint32_t* ca[4];
        const uint32_t* cb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ca[r] = s_codes + (16 * wave + 4 * q + r) * cstride;
            cb[r] = s_codes + (MMG_PAIR_TILE + 16 * r + i) * cstride;
        }
        pair_hamming(ca, cb, nw, h);
    } else {
        const uint32_t* ca[4];
        const uint32_t* cb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ca[r] = ar.codes + (size_t)min(I0 + 16 * wave + 4 * q + r, n - 1) * ar.row_words + ar.sel0;
            cb[r] = ar.codes + (size_t)min(J0 + 16 * r + i, n - 1) * ar.row_words + ar.sel0;
        }
        pair_hamming(ca, cb, nw, h);
    }
    const float halfK = 0.5f * (float)K;
    int counted = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = 16 * wave + 4 * q + r, lj = 16 * j + i;
            const int ti = s_tgt[li], tj = s_tgt[MMG_PAIR_TILE + lj];
            if (ti < 0 || tj < 0 || (bi == bj && li >= lj)) continue;
            const float c = __fmul_rn(acc[j][r], __fmul_rn(s_inv[li], s_inv[MMG_PAIR_TILE + lj]));
            const float u = __fmul_rn(__fsub_rn(1.f, c), halfK);
            const int qb = (int)fminf(fmaxf(floorf(u), 0.f), (float)(K - 1));          // (a NaN lands in bin 0: never out of bounds)
            const int slot = ((ti == tj ? 1 : 0) * (ar.M + 1) + min(h[j][r], ar.M)) * K + qb;     // (min: codes with padding bits set stay in bounds)
            if (ar.hist_lds) atomicAdd(&s_hist[slot], 1u);
            else pair_add(ar.hist + MMG_PAIR_HEAD + slot, 1ull);
            ++counted;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) counted += __shfl_xor(counted, o, 64);
    if (lane == 0 && counted) pair_add(ar.hist + 2, (unsigned long long)counted);
    if (ar.hist_lds) {
        __syncthreads();
        for (int e = tid; e < slots; e += MMG_BLOCK) {
            const uint32_t v = s_hist[e];
            if (v) pair_add(ar.hist + MMG_PAIR_HEAD + e, (unsigned long long)v);
        }
    }
}

}  // namespace mmg
