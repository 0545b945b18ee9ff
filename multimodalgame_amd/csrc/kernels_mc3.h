// kernels_mc3.h -- k_conversation_mc3: the many-class conversation of kernels_mc.h for CONTINUOUS messages (-nouse_binary: BASELINE
// config 5), re-cut the way kernels_fast3.h re-cut the 30-class kernel:
//   * 256 threads, one wave per SIMD; the per-sample agent phases are k_conversation_fast3's (code_layer | binary_layer | GRU cell |
//     heads on h | message), phases written as [LDS loads] [branch-free arithmetic] [stores];
//   * the description mixture is folded onto the classes: W_d (softmax(y) . desc) = softmax(y) . Dd, Dd = desc W_d^T [D, R] (k_prep).
//     A member's slice of the mixture is then e_k [16, 64] x Dd_k [64, R = 64] -- ONE 16-column MFMA tile per wave instead of seven
//     over V = 100 -- the all-to-all payload shrinks from V + 2 to R + 2 floats per (slice, sample), and the sample's combine step
//     yields w_d dbar directly (no dbar phase, no w_d phase).  dbar itself is never formed: in continuous mode w_d, w_h and w get no
//     gradient (every message input is detached, model.py:810, 1297-1305);
//   * W_hh (and code_layer) parked in LDS as per-lane spill slots; the hidden-side GRU product of the NEXT step runs between the
//     publication of A and the poll for the tile's rows, i.e. inside the first hand-off's wait.
// Hand-offs: the payload itself, as (value, epoch) pairs -- one aligned 8-byte write-through store / agent-scope load each
// (device_utils.h: st_ll), epoch = (minibatch counter, step).  A consumer loads the pairs it needs and loads again while any carries
// another epoch: one trip through memory once the data has landed.  k_conversation_mc's protocol (write-through payload, wait for
// the stores to complete, one counter increment per member; poll the counter, then agent-scope loads of the payload) is three
// dependent trips, ~1.5 us more per hand-off, two hand-offs per step.  The buffers are reused every step: a member's step t + 1
// rows go out only after it has passed the second hand-off of step t, i.e. after every member has read the step-t rows.
// ONE counter hand-off remains, after the last step: a slice owner's write-through stores of the selected logits (tape.outp) must
// have completed before the sample's owner reads them.
// Same tape contract and sampling streams as k_conversation_mc; binary messages with many classes stay on k_conversation_mc (their
// w_d gradient needs dbar).
#pragma once
#include "device_utils.h"
#include "kernels_fast3.h"
#include "kernels_mc.h"
#include "layout.h"

namespace mmg {

#define MMG_MC3_LDP 68                              // floats per (slice, sample) row of the partial buffer: R mixture terms | m | s | pad

// The y head of one (sample row, class, r-quarter): sum_j w2[j] max(A[j], -Cd[j]) over the quarter's 16 hidden units, as two
// chains over the even / the odd units kept in ONE packed accumulator (v_pk_fma_f32: half the FMA issue slots of the scalar
// form; the same products in the same order, so the sum is bit for bit that of p0 + p1 of rounds 3-5).
__device__ __forceinline__ float yhead16(const float4& a0, const float4& a1, const float4& a2, const float4& a3,
                                         const float (&ncd)[16], const float (&w2e)[16]) {
    f32x2 acc = {0.f, 0.f};
#define MMG_YH(ax, ay, j) acc = __builtin_elementwise_fma(f32x2{w2e[j], w2e[j + 1]}, f32x2{fmax_nn(ax, ncd[j]), fmax_nn(ay, ncd[j + 1])}, acc)
    MMG_YH(a0.x, a0.y, 0); MMG_YH(a0.z, a0.w, 2); MMG_YH(a1.x, a1.y, 4); MMG_YH(a1.z, a1.w, 6);
    MMG_YH(a2.x, a2.y, 8); MMG_YH(a2.z, a2.w, 10); MMG_YH(a3.x, a3.y, 12); MMG_YH(a3.z, a3.w, 14);
#undef MMG_YH
    return acc.x + acc.y;
}
// ... for the 16 rows of a tile: rows are fetched one ahead of their use (LDS latency under the previous row's 30 VALU slots; at
// one wave per SIMD nothing else hides it), two rows in flight keep the register footprint at 32 floats
template <int TM, int LDA, int LDY>
__device__ __forceinline__ void yhead_tile(const float* s_At, float* s_y, int e4, int cls, float cyv, const float (&ncd)[16], const float (&w2e)[16]) {
    const float* ar_ = s_At + 16 * e4;
    float4 c0 = *reinterpret_cast<const float4*>(ar_), c1 = *reinterpret_cast<const float4*>(ar_ + 4);
    float4 c2 = *reinterpret_cast<const float4*>(ar_ + 8), c3 = *reinterpret_cast<const float4*>(ar_ + 12);
#pragma unroll 2
    for (int i = 0; i < TM; ++i) {
        const float* nx = s_At + min(i + 1, TM - 1) * LDA + 16 * e4;
        const float4 n0 = *reinterpret_cast<const float4*>(nx), n1 = *reinterpret_cast<const float4*>(nx + 4);
        const float4 n2 = *reinterpret_cast<const float4*>(nx + 8), n3 = *reinterpret_cast<const float4*>(nx + 12);
        const float tot = dpp_group_sum<4>(yhead16(c0, c1, c2, c3, ncd, w2e));
        if (e4 == 0) s_y[i * LDY + cls] = tot + cyv;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
}

struct Mc3Lds {
    static constexpr int R = 64, W = 32, H = 256, TM = 16, LDA = R + 4, LDY = 64 + 4;
    static constexpr int a = 0;                          // [H]
    static constexpr int z = a + H;                      // [W]
    static constexpr int w = z + W;                      // [W]    the message the sender reads next
    static constexpr int h = w + W;                      // [2][R] state before / after the step
    static constexpr int Aown = h + 2 * R;               // [LDA]
    static constexpr int gh = Aown + LDA;                // [R]    w_h h + b_h
    static constexpr int g = gh + R;                     // [R]
    static constexpr int At = g + R;                     // [TM][LDA]
    static constexpr int y = At + TM * LDA;              // [TM][LDY]
    static constexpr int e = y + TM * LDY;               // [TM][LDY]
    static constexpr int P = e + TM * LDY;               // [TM][LDP]
    static constexpr int in = P + TM * MMG_MC3_LDP;      // [TM][LDP]  the 16 slices' partials of this sample
    static constexpr int ms = in + TM * MMG_MC3_LDP;     // m[16] | s[16]
    static constexpr int small = ms + 32;                // us[16] | mask[17] | red[16] | pad
    static constexpr int park = small + 64;              // [20][256] float4: W_hh (12) | code_layer (8)
    // the sample's tape, staged per step and flushed after the conversation (a hand-off signal waits for the member's
    // outstanding stores: only the hand-off payload is outstanding then)
    static constexpr int TMAX = 16;
    static constexpr int t_gru = park + 20 * 256 * 4;    // [TMAX][4 R]
    static constexpr int t_h = t_gru + TMAX * 4 * R;     // [TMAX + 1][R]
    static constexpr int t_z = t_h + (TMAX + 1) * R;     // [TMAX][W]
    static constexpr int t_sp = t_z + TMAX * W;          // s[16] | ps[16]
    static constexpr int t_a = t_sp + 32;                // [TMAX][H]      (not lean)
    static constexpr int t_g = t_a + TMAX * H;           // [TMAX][R]      (not lean)
    static constexpr int t_w = t_g + TMAX * R;           // [TMAX + 1][W]  (not lean): slot 0 = first_rec, slot t + 1 = w_t
    static constexpr int total = t_w + (TMAX + 1) * W;
};
__host__ __device__ inline int mc3_lds_bytes() { return Mc3Lds::total * 4; }

// k_conversation_mc3 and, for a handle with Gaussian message noise, k_conversation_mc3_noise: one text (conversation_mc3_body.h), two kernels
#define MMG_MC3_NOISE 0
#include "conversation_mc3_body.h"
#undef MMG_MC3_NOISE
#define MMG_MC3_NOISE 1
#include "conversation_mc3_body.h"
#undef MMG_MC3_NOISE

}  // namespace mmg
