// bwd_sample_parts.h -- the receiver's reverse-time pass of ONE sample per workgroup with W_hh^T in registers, written once
// for the kernels that run it: k_bwd_conv_fast (kernels_fast.h), the second half of k_game_fast (kernels_game.h) and
// k_bwd_sample (kernels_tile.h).
// Copies that remain, to be changed TOGETHER with the pieces here:
//   * k_bwd_mc2 (kernels_mc.h) keeps every line it had -- the fragment loads (load_whhT_y1T), the gru / h staging (stage_gru_h),
//     W_y1h^T dA (y1hT_dA) and the two-barrier recurrence with its cell backward, minus the dhin term.  Converted, config 5 timed
//     a median of 724.3 us per minibatch against 723.2 .. 723.6 of the copy (three alternating runs each): outside the copy's own
//     spread, the bar this header was held to.  load_whhT_y1T, stage_gru_h and recurrence_two_barrier so have ONE caller, k_bwd_sample.
//   * recurrence_one_barrier spells the cell backward (gru_cell_bwd) out: the cell backward exists three times in csrc.
// Measurements: profiles/bwd_parts_isa_digest.txt, profiles/bwd_parts_ab.txt, profiles/bwd_parts_bench_ab.txt (scripts/bwd_ab.py).
//
// Plain function templates over raw pointers (global and LDS), register arrays and scalars: a kernel fetches its operands
// where it keeps them (global tape, LDS slots of a forward half) and calls the pieces; what differs between the kernels stays
// at the call sites.  Common lane mapping: 256 threads, R = 64 units, K4 = 4 lanes per unit -- thread tid works on output
// unit k4 = tid / K4 and reduction slice p4 = tid % K4 of the R-wide transposed products; (wv, fi, fq) = (tid >> 6,
// lane & 15, lane >> 4) are the wave and the MFMA fragment coordinates of the sweeps.  Every contract below says which
// thread holds what and which barrier, if any, the piece ends on.  Expressions are kept in the order the kernels had them:
// the results are bit-identical.
#pragma once
#include "device_utils.h"
#include "layout.h"

namespace mmg {

// hardware log (v_log_f32, ~1 ulp; kernels_fast.h: fsigmoid, ftanh)
__device__ __forceinline__ float flog(float x) { return __logf(x); }

// d loss / d logit of one Bernoulli unit (kernels_bwd.h: bit_seed) with hardware rcp / log
__device__ __forceinline__ float bit_seed_fast(float q, float p, float wh, float ce) {
    const float pe = p + MMG_EPS, qe = 1.f - p + MMG_EPS;
    const float rp = __builtin_amdgcn_rcpf(pe), rq = __builtin_amdgcn_rcpf(qe);
    float dLdp = -wh * (q * rp - (1.f - q) * rq);
    if (ce != 0.f) dLdp += ce * (flog(pe) + p * rp - flog(qe) - (1.f - p) * rq);
    return dLdp * p * (1.f - p);
}

// ---------------------------------------------------------------------------------------------
// 1. GRU cell backward of unit k.  gr: the step's four gate rows [r | u | n | W_hn h + b_hn] (4 R floats, LDS), hprev: h_{t-1}
// (R floats, LDS).  Every thread computes all of its unit's gate gradients; which lane stores which is the caller's business.
// dgi = (drp, dup, dnp), dgh = (drp, dup, dnp * rr).  No barrier.
// (recurrence_one_barrier below spells the same six lines out: as a call they moved k_game_fast's SGPR spill code -- 164 / 38
//  v_readlane / v_writelane instead of 160 / 43 -- and that kernel is held to the resources it had.  Change both together.)
// ---------------------------------------------------------------------------------------------
struct CellGrad { float drp, dup, dnp, rr, uu; };

template <int R>
__device__ __forceinline__ CellGrad gru_cell_bwd(float dh, const float* gr, const float* hprev, int k) {
    const float rr = gr[k], uu = gr[R + k], nn = gr[2 * R + k], ghn = gr[3 * R + k];
    const float hp = hprev[k];
    const float dn = dh * (1.f - uu), du = dh * (hp - nn);
    const float dnp = dn * (1.f - nn * nn), dup = du * uu * (1.f - uu);
    const float drp = dnp * ghn * rr * (1.f - rr);
    return {drp, dup, dnp, rr, uu};
}

// ---------------------------------------------------------------------------------------------
// 2. (W_hh^T dgh)[k4]: thread (k4, p4) holds whhT[i] = W_hh[p4 * 3R/K4 + i][k4] and reads its slice of dgh (3 R floats, LDS,
// 16-byte aligned) as float4s into four independent FMA chains; the K4-lane sum leaves the result in ALL lanes of the unit.
// The caller has put a barrier between the stores to dgh and this call.  No barrier.
// ---------------------------------------------------------------------------------------------
template <int R, int K4>
__device__ __forceinline__ float whhT_dgh(const float (&whhT)[3 * R / K4], const float* dgh, int p4) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < 3 * R / K4; i += 4) {
        const float4 dv = *reinterpret_cast<const float4*>(dgh + p4 * (3 * R / K4) + i);
        a0 = fmaf(whhT[i], dv.x, a0); a1 = fmaf(whhT[i + 1], dv.y, a1);
        a2 = fmaf(whhT[i + 2], dv.z, a2); a3 = fmaf(whhT[i + 3], dv.w, a3);
    }
    return dpp_group_sum<K4>((a0 + a1) + (a2 + a3));
}

// ---------------------------------------------------------------------------------------------
// 3a. The recurrence of k_bwd_conv_fast / k_game_fast: two phases and ONE barrier per step.  The carried dh of unit k4 lives in a
// register of each of the unit's four lanes (the 4-lane sum leaves W_hh^T dgh in all of them: no LDS hop, no barrier before the
// next cell backward), and the gate gradients are double-buffered in s_dgh[2][3 R]: a wave that runs ahead writes the OTHER
// buffer and stops at the next step's barrier, which the slowest wave reaches only after it has read this one.
// What step t adds to dh besides the recurrence: cf[t] dhin[t] + cf[TMAX + t] H2[t] + w_s[k4] dls[t], and dAy at t*.
// Lane p4 < 3 of a unit stores the p4-th gate gradient (selects, then ONE predicated region: three divergent branches each with
// their own stores split the phase).  dgi / dgh: the global [T, B, 3 R] tapes.  The caller's barrier has made every LDS operand
// visible; ends WITHOUT a barrier (the last W_hh^T dgh only reads).  stamp(16 + 2 t) / stamp(16 + 2 t + 1): timing build.
// ---------------------------------------------------------------------------------------------
template <int R, int K4, int TMAX, class Stamp>
__device__ __forceinline__ void recurrence_one_barrier(const float (&whhT)[3 * R / K4], const float* t_gru, const float* t_h, const float* s_cf,
                                                       const float* s_dhin, const float* s_H2, const float* s_dls, const float* s_dAy, float wsk,
                                                       float* s_dgh, float* dgi, float* dgh, int B, int b, int tstar, int k4, int p4, Stamp stamp) {
    static_assert(K4 == 4, "four lanes per unit share the stores");
    auto step_in = [&](int t) {
        float v = fmaf(s_cf[t], s_dhin[t * R + k4], s_cf[TMAX + t] * s_H2[t * R + k4]) + wsk * s_dls[t];
        if (t == tstar) v += s_dAy[k4];
        return v;
    };
    float dh_c = 0.f;
    for (int t = tstar; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        float* const dgb = s_dgh + (t & 1) * 3 * R;
        stamp(16 + 2 * t);
        // ===== GRU cell backward
        const float dh = dh_c + step_in(t);
        const float* gr = t_gru + t * 4 * R;
        const float rr = gr[k4], uu = gr[R + k4], nn = gr[2 * R + k4], ghn = gr[3 * R + k4];
        {
            const float hp = t_h[t * R + k4];
            const float dn = dh * (1.f - uu), du = dh * (hp - nn);
            const float dnp = dn * (1.f - nn * nn), dup = du * uu * (1.f - uu);
            const float drp = dnp * ghn * rr * (1.f - rr);
            float* gi = dgi + row * 3 * R; float* gh = dgh + row * 3 * R;
            const float vi = (p4 == 0) ? drp : (p4 == 1) ? dup : dnp;
            const float vh = (p4 == 2) ? dnp * rr : vi;
            const int idx = p4 * R + k4;
            if (p4 < 3) { gi[idx] = vi; gh[idx] = vh; dgb[idx] = vh; }
        }
        __syncthreads(); stamp(16 + 2 * t + 1);
        // ===== dh_{t-1} = dh * u + W_hh^T dgh
        dh_c = __fmul_rn(dh, uu) + whhT_dgh<R, K4>(whhT, dgb, p4);
    }
}

// ---------------------------------------------------------------------------------------------
// 3b. The recurrence of k_bwd_sample: [cell backward] barrier [W_hh^T dgh] barrier, the carried dh in s_dh (R floats, zeroed by
// the caller).  Step t adds s_dhin[t * R + k4] (k_bwd_pre's message terms) and, at t*, s_dAy[k4].  The caller's barrier has made
// t_gru, t_h, s_dhin, s_dAy and s_dh visible; ends on a barrier.
// ---------------------------------------------------------------------------------------------
template <int R, int K4>
__device__ __forceinline__ void recurrence_two_barrier(const float (&whhT)[3 * R / K4], const float* t_gru, const float* t_h, const float* s_dhin,
                                                       const float* s_dAy, float* s_dh, float* s_dgh, float* dgi, float* dgh, int B, int b,
                                                       int tstar, int k4, int p4) {
    for (int t = tstar; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        const float din = s_dhin[t * R + k4] + ((t == tstar) ? s_dAy[k4] : 0.f);
        {
            const CellGrad c = gru_cell_bwd<R>(s_dh[k4] + din, t_gru + t * 4 * R, t_h + t * R, k4);
            float* gi = dgi + row * 3 * R; float* gh = dgh + row * 3 * R;
            if (p4 == 0)      { gi[k4] = c.drp; gh[k4] = c.drp; s_dgh[k4] = c.drp; }
            else if (p4 == 1) { gi[R + k4] = c.dup; gh[R + k4] = c.dup; s_dgh[R + k4] = c.dup; }
            else if (p4 == 2) { gi[2 * R + k4] = c.dnp; gh[2 * R + k4] = c.dnp * c.rr; s_dgh[2 * R + k4] = c.dnp * c.rr; }
        }
        __syncthreads();
        {
            const float acc = whhT_dgh<R, K4>(whhT, s_dgh, p4);
            if (p4 == 0) s_dh[k4] = __fmul_rn(s_dh[k4] + din, t_gru[t * 4 * R + R + k4]) + acc;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// 4. s_dAy = W_y1h^T dA (enters dh at the output step only): thread (k4, p4) holds y1T[i] = y1[p4 * R/K4 + i][k4]; lane p4 == 0
// writes s_dAy[k4].  The caller's barrier has made s_dA visible.  No barrier.
// ---------------------------------------------------------------------------------------------
template <int R, int K4>
__device__ __forceinline__ void y1hT_dA(const float (&y1T)[R / K4], const float* s_dA, float* s_dAy, int k4, int p4) {
    float accy = 0.f;
#pragma unroll
    for (int i = 0; i < R / K4; ++i) accy = fmaf(y1T[i], s_dA[p4 * (R / K4) + i], accy);
    accy = dpp_group_sum<K4>(accy);
    if (p4 == 0) s_dAy[k4] = accy;
}

// ---------------------------------------------------------------------------------------------
// 5. The output step t* (model.py:1264-1275).
// output_seed: wave 0 holds dy_mine = the NLL seed of class `lane` (zero beyond Dr) and stores dy, s_dy[32] and dysum[b]; wave 1
// copies h* = hstar_src (R floats, LDS) to hstar.  No barrier.
// output_dA: thread tid < R holds a = A*[tid] and acc = sum_d [a + Cd[d][tid] > 0] dy_d, summed by the caller from s_dy and the Cd
// column where the kernel keeps it; dA = w2 acc; stores s_dA, dA and A*.  No barrier.
// WT: dy and A* go out as device-scope write-through stores (the class roles of the same launch read them after a counter moves).
// ---------------------------------------------------------------------------------------------
template <bool WT>
__device__ __forceinline__ void store_maybe_wt(float* p, float v) {
    if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

template <int R, bool WT>
__device__ __forceinline__ void output_seed(float dy_mine, const float* hstar_src, float* s_dy, float* dy, float* dysum, float* hstar, int Dr, int b, int tid) {
    const int lane = tid & 63;
    if (tid < 64) {
        if (lane < Dr) store_maybe_wt<WT>(&dy[(size_t)b * Dr + lane], dy_mine);
        if (lane < 32) s_dy[lane] = dy_mine;
        const float dsum = dpp_wave_sum(dy_mine);
        if (lane == 0) dysum[b] = dsum;
    } else if (tid < 64 + R) {
        hstar[(size_t)b * R + tid - 64] = hstar_src[tid - 64];
    }
}

template <int R, bool WT>
__device__ __forceinline__ void output_dA(float a, float acc, float w2_mine, float* s_dA, float* dA, float* Astar, int b, int tid) {
    const float v = acc * w2_mine;
    s_dA[tid] = v; dA[(size_t)b * R + tid] = v;
    store_maybe_wt<WT>(&Astar[(size_t)b * R + tid], a);
}

// The whole step for the kernels that hold y1[:, :R]'s row fragment (y1r[i] = y1[k4][p4 * R/K4 + i]) and the Cd columns
// (cdcol[d] = Cd[d][tid], tid < R) in registers: output_seed, A* = y1h . h* through s_A, barrier, output_dA.  t_h: the staged
// h rows, visible.  Ends after output_dA, WITHOUT a barrier.
template <int R, int K4, int D, bool WT>
__device__ __forceinline__ void output_step(float dy_mine, const float (&y1r)[R / K4], const float (&cdcol)[D], float w2_mine, const float* t_h, float* s_dy,
                                            float* s_A, float* s_dA, float* dy, float* dysum, float* hstar, float* dA, float* Astar, int Dr, int b,
                                            int tstar, int tid, int k4, int p4) {
    const float* hs = t_h + (tstar + 1) * R;
    output_seed<R, WT>(dy_mine, hs, s_dy, dy, dysum, hstar, Dr, b, tid);
    {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < R / K4; ++i) acc = fmaf(y1r[i], hs[p4 * (R / K4) + i], acc);
        acc = dpp_group_sum<K4>(acc);
        if (p4 == 0) s_A[k4] = acc;
    }
    __syncthreads();
    if (tid < R) {
        const float a = s_A[tid];
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) acc += (a + cdcol[d] > 0.f) ? s_dy[d] : 0.f;
        output_dA<R, WT>(a, acc, w2_mine, s_dA, dA, Astar, b, tid);
    }
}

// ---------------------------------------------------------------------------------------------
// 6. k_bwd_sample: the two transposed register fragments from the parameter buffer (whh: W_hh [3 R, R]; y1w: y1
// [R, R + V]) and this sample's GRU tape and h rows for ALL steps into LDS in one round trip (steps clamped to t*, not guarded:
// t_gru [TMAX][4 R], t_h [TMAX + 1][R]).  No barrier.
// ---------------------------------------------------------------------------------------------
template <int R, int V, int K4>
__device__ __forceinline__ void load_whhT_y1T(const float* __restrict__ whh, const float* __restrict__ y1w, float (&whhT)[3 * R / K4], float (&y1T)[R / K4],
                                              int k4, int p4) {
#pragma unroll
    for (int i = 0; i < 3 * R / K4; ++i) whhT[i] = whh[(size_t)(p4 * (3 * R / K4) + i) * R + k4];
#pragma unroll
    for (int i = 0; i < R / K4; ++i) y1T[i] = y1w[(size_t)(p4 * (R / K4) + i) * (R + V) + k4];
}

template <int R, int NT, int TMAX>
__device__ __forceinline__ void stage_gru_h(const float* gru, const float* h, float* t_gru, float* t_h, int B, int T, int b, int tstar, int tid) {
    constexpr int NU_ = TMAX * 4 * R / NT, NH_ = ((TMAX + 1) * R + NT - 1) / NT;
    float ru_[NU_], rh_[NH_];
    const int Tm1 = T - 1;
#pragma unroll
    for (int u = 0; u < NU_; ++u) { const int i = tid + NT * u, t = min(i / (4 * R), min(tstar, Tm1)), j = i % (4 * R); ru_[u] = gru[((size_t)t * B + b) * 4 * R + j]; }
#pragma unroll
    for (int u = 0; u < NH_; ++u) { const int i = tid + NT * u, t = min(i / R, min(tstar + 1, T)), j = i % R; rh_[u] = h[((size_t)t * B + b) * R + j]; }
#pragma unroll
    for (int u = 0; u < NU_; ++u) t_gru[tid + NT * u] = ru_[u];
#pragma unroll
    for (int u = 0; u < NH_; ++u) { const int i = tid + NT * u; if (i < (TMAX + 1) * R) t_h[i] = rh_[u]; }
}

// ---------------------------------------------------------------------------------------------
// 7. k_bwd_conv_fast / k_game_fast: everything that does not depend on the carried dh, for ALL steps of the sample at once, on the
// two seed BASES.  A Bernoulli seed is linear in its two loss coefficients (App. A.4):
//   seed = wh S1 + ce S2,   S1 = -(q / pe - (1 - q) / qe) p (1 - p),   S2 = (log pe + p / pe - log qe - (1 - p) / qe) p (1 - p)
// and so is everything downstream of it: dgpre = (dlw W_w)(1 - g^2), the sender's dpre = (dlz W_b)(1 - a^2) and dgpre W_h run as
// [16 steps, K] x [K, N] products on the matrix cores (v_mfma_f32_16x16x4_f32) BEFORE the batch statistics are needed; after the
// wait a step's gradients are two multiply-adds of its bases with (wh_t, ce_t).
// ---------------------------------------------------------------------------------------------
// The 30 float4 of tape.wrep (kernels_fwd.h: prep_repack) -> the five transposed fragments.  The caller issues the loads into q,
// in the order it wants them back.
__device__ __forceinline__ void unpack_wrep(const float4 (&q)[MMG_REPACK_F4], float (&whhT)[48], float (&y1T)[16], float (&wwF)[8], float (&whF)[16], float (&wbF)[4][8]) {
    static_assert(MMG_REPACK_F4 == 30, "layout of tape.wrep");
    auto put = [](float* dst, const float4& v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w; };
#pragma unroll
    for (int j = 0; j < 12; ++j) put(whhT + 4 * j, q[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) put(y1T + 4 * j, q[12 + j]);
#pragma unroll
    for (int j = 0; j < 2; ++j) put(wwF + 4 * j, q[16 + j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) put(whF + 4 * j, q[18 + j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) put(&wbF[j >> 1][4 * (j & 1)], q[22 + j]);
}

__device__ __forceinline__ void seed_basis(float q, float pr, float& S1, float& S2) {
    const float pe = pr + MMG_EPS, qe = 1.f - pr + MMG_EPS;
    const float rp = __builtin_amdgcn_rcpf(pe), rq = __builtin_amdgcn_rcpf(qe), pq = pr * (1.f - pr);
    S1 = -(q * rp - (1.f - q) * rq) * pq;
    S2 = (flog(pe) + pr * rp - flog(qe) - (1.f - pr) * rq) * pq;
}

// The seed bases of element i = tid + NT u of the [TMAX][W] message tiles (receiver: t_w, t_pw; sender: t_z, t_pz; LDS, visible):
// kept in registers (s1w .. s2z) for the tape stores and written to s_sbas [4][TMAX][SW] (w1 | w2 | z1 | z2, rows padded) as the
// A operands of sweep_seed.  The receiver's message is active while m_{t+1} == 1 (t < t*), the sender's for t <= t*; neither
// without binary messages.  No barrier: the caller puts one before sweep_seed.
template <int W, int NT, int TMAX, int SW>
__device__ __forceinline__ void seed_bases(const float* t_w, const float* t_pw, const float* t_z, const float* t_pz, float* s_sbas, bool binary, int tstar,
                                           int tid, float (&s1w)[TMAX * W / NT], float (&s2w)[TMAX * W / NT], float (&s1z)[TMAX * W / NT],
                                           float (&s2z)[TMAX * W / NT]) {
#pragma unroll
    for (int u = 0; u < TMAX * W / NT; ++u) {
        const int i = tid + NT * u, t = i / W;
        float a1, a2, b1, b2;
        seed_basis(t_w[i], t_pw[i], a1, a2);
        seed_basis(t_z[i], t_pz[i], b1, b2);
        if (!(binary && t < tstar)) { a1 = 0.f; a2 = 0.f; }
        if (!(binary && t <= tstar)) { b1 = 0.f; b2 = 0.f; }
        s1w[u] = a1; s2w[u] = a2; s1z[u] = b1; s2z[u] = b2;
        const int j = i - t * W;
        s_sbas[t * SW + j] = a1; s_sbas[(TMAX + t) * SW + j] = a2; s_sbas[(2 * TMAX + t) * SW + j] = b1; s_sbas[(3 * TMAX + t) * SW + j] = b2;
    }
}

// First sweep: g1 | g2 = (bases of dlw) W_w scaled by (1 - g^2) for unit 16 wv + fi, p1 | p2[nt] = (bases of dlz) binary_layer scaled
// by (1 - a^2) for column 64 wv + 16 nt + fi; a lane's D fragment holds rows t = 4 fq + r.  B fragments: lane (fi, fq) holds
// Wm[4 ks + fq][n0 + fi] per k-step ks (wwF, wbF).  t_g [TMAX][R], t_a [TMAX][H]: LDS, visible.  No barrier.
template <int W, int R, int H, int TMAX, int SW>
__device__ __forceinline__ void sweep_seed(const float* s_sbas, const float (&wwF)[W / 4], const float (&wbF)[4][W / 4], const float* t_g, const float* t_a,
                                           int wv, int fi, int fq, f32x4& g1, f32x4& g2, f32x4 (&p1)[4], f32x4 (&p2)[4]) {
    g1 = f32x4{0.f, 0.f, 0.f, 0.f}; g2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { p1[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; p2[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int ks = 0; ks < W / 4; ++ks) {
        const int o = fi * SW + 4 * ks + fq;
        const float aw1 = s_sbas[o], aw2 = s_sbas[TMAX * SW + o], az1 = s_sbas[2 * TMAX * SW + o], az2 = s_sbas[3 * TMAX * SW + o];
        g1 = mfma16(aw1, wwF[ks], g1); g2 = mfma16(aw2, wwF[ks], g2);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { p1[nt] = mfma16(az1, wbF[nt][ks], p1[nt]); p2[nt] = mfma16(az2, wbF[nt][ks], p2[nt]); }
    }
    const int unit = 16 * wv + fi;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float g = t_g[(4 * fq + r) * R + unit];
        g1[r] *= (1.f - g * g); g2[r] *= (1.f - g * g);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = t_a[(4 * fq + r) * H + 64 * wv + 16 * nt + fi];
            p1[nt][r] *= (1.f - a * a); p2[nt][r] *= (1.f - a * a);
        }
}

// Second sweep: s_dhin | s_H2 [TMAX][R] = (s_G1 | s_G2 [TMAX][SR], the dgpre bases the caller stored and put a barrier behind) W_h,
// the two bases of the message terms of dh.  No barrier: the caller puts one before the recurrence.
template <int R, int SR>
__device__ __forceinline__ void sweep_wh(const float* s_G1, const float* s_G2, const float (&whF)[R / 4], float* s_dhin, float* s_H2, int wv, int fi, int fq) {
    f32x4 h1 = {0.f, 0.f, 0.f, 0.f}, h2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < R / 4; ++ks) {
        h1 = mfma16(s_G1[fi * SR + 4 * ks + fq], whF[ks], h1);
        h2 = mfma16(s_G2[fi * SR + 4 * ks + fq], whF[ks], h2);
    }
    const int unit = 16 * wv + fi;
#pragma unroll
    for (int r = 0; r < 4; ++r) { s_dhin[(4 * fq + r) * R + unit] = h1[r]; s_H2[(4 * fq + r) * R + unit] = h2[r]; }
}

// Per-step scalars of the three streams (model.py:908-922), thread tid < TMAX for step tid: s_cf [4][TMAX] = (wh, ce) of the
// receiver's and of the sender's message, wh = (L - baseline) cw; s_dls = the stop bit's seed (none with a fixed number of steps);
// live steps also store dls and the baselines' MSE seeds dbs, dbr (model.py:971-988).  cw, ce [3][T] and cb [T]: the loss
// coefficients (coef_compute), visible; rbs, rbr, rs, rps: this step's baseline scores, stop bit and its probability.
// No barrier: the caller puts one before the tape stores and the recurrence.
template <int TMAX>
__device__ __forceinline__ void step_scalars(const float* cw, const float* ce, const float* cb, float L, float rbs, float rbr, float rs, float rps,
                                             bool binary, bool fixed, float* s_cf, float* s_dls, float* dls_out, float* dbs, float* dbr, int B, int T,
                                             int b, int tstar, int tid) {
    if (tid < TMAX) {
        const int t = min(tid, T - 1);
        const bool on = binary && tid <= tstar;
        s_cf[tid] = on ? (L - rbr) * cw[T + t] : 0.f;          s_cf[TMAX + tid] = on ? ce[T + t] : 0.f;          // receiver message
        s_cf[2 * TMAX + tid] = on ? (L - rbs) * cw[2 * T + t] : 0.f; s_cf[3 * TMAX + tid] = on ? ce[2 * T + t] : 0.f;   // sender message
        float dls = 0.f;
        if (on && !fixed) dls = bit_seed_fast(rs, rps, (L - rbr) * cw[t], ce[t]);
        s_dls[tid] = dls;
        if (tid <= tstar) {
            const size_t row = (size_t)tid * B + b;
            dls_out[row] = dls;
            dbs[row] = binary ? cb[t] * (rbs - L) : 0.f;
            dbr[row] = binary ? cb[t] * (rbr - L) : 0.f;
        }
    }
}

// The gradient tapes of the live steps: bases x coefficients (stores only; the recurrence does not wait for them).  dlw, dlz
// [T, B, W] from the register bases of seed_bases, dgpre [T, B, R] and dpre [T, B, H] from sweep_seed's fragments, and
// dhx [B, H] = the column sums of dpre over the live steps.  s_cf: step_scalars', visible.  No barrier.
template <int W, int R, int H, int NT, int TMAX>
__device__ __forceinline__ void store_grad_tapes(const float* s_cf, const float (&s1w)[TMAX * W / NT], const float (&s2w)[TMAX * W / NT],
                                                 const float (&s1z)[TMAX * W / NT], const float (&s2z)[TMAX * W / NT], const f32x4& g1, const f32x4& g2,
                                                 const f32x4 (&p1)[4], const f32x4 (&p2)[4], float* dlw, float* dlz, float* dgpre, float* dpre, float* dhx,
                                                 int B, int b, int tstar, int tid, int wv, int fi, int fq) {
    const float* c1r = s_cf, *c2r = s_cf + TMAX, *c1z = s_cf + 2 * TMAX, *c2z = s_cf + 3 * TMAX;
#pragma unroll
    for (int u = 0; u < TMAX * W / NT; ++u) {
        const int i = tid + NT * u, t = i / W, j = i - t * W;
        if (t <= tstar) {
            const size_t row = (size_t)t * B + b;
            dlw[row * W + j] = fmaf(c1r[t], s1w[u], c2r[t] * s2w[u]);
            dlz[row * W + j] = fmaf(c1z[t], s1z[u], c2z[t] * s2z[u]);
        }
    }
    const int unit = 16 * wv + fi;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = 4 * fq + r;
        if (t <= tstar) dgpre[((size_t)t * B + b) * R + unit] = fmaf(c1r[t], g1[r], c2r[t] * g2[r]);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int hcol = 64 * wv + 16 * nt + fi;
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 4 * fq + r;
            if (t <= tstar) {
                const float v = fmaf(c1z[t], p1[nt][r], c2z[t] * p2[nt][r]);
                dpre[((size_t)t * B + b) * H + hcol] = v;
                part += v;
            }
        }
        part += __shfl_xor(part, 16); part += __shfl_xor(part, 32);       // the four row groups of the column
        if (fq == 0) dhx[(size_t)b * H + hcol] = part;
    }
}

}  // namespace mmg
