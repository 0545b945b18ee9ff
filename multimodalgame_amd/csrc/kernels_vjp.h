// kernels_vjp.h -- vector-Jacobian products of one training exchange (mmg_exchange_vjp): the backward pass of each agent's own
// autograd graph for ANY scalar built from exchange()'s outputs, not only the reference's losses (model.py:1243-1330).
//
// One generic path serves every forward path.  The VJP reads only what every training run-all forward leaves and exchange()
// itself hands out -- h_x, the GRU states h, the messages z / w, the probabilities pz / pw / ps and the class logits y -- and forms
// everything else (gate activations, h_w, dbar, the sender's hidden layer, the baselines' hidden units, Cd) from the parameters,
// in fp32, into tape arrays of its own (v*).  The paths' tapes differ (k_conversation_fast3 keeps softmax rows instead of dbar,
// the live-row paths leave dead rows stale); the VJP depends on none of that.  Rows of steps t >= n_steps carry zero deltas.
//
// The weight gradients are then the existing k_wgrad<false> over four job tables of their own (one per agent, all T * B rows,
// built at mmg_create).  Every sum below runs in a fixed order inside one thread: results are deterministic.
//
// The per-call VJPs of the agent modules' forward() (mmg_sender_vjp / mmg_receiver_vjp / mmg_baseline_vjp) run the same step
// math (vjp_rec_step, vjp_sen_step, vjp_bas_hidden) on ONE call: the call's inputs and outputs come from the caller's buffers,
// the recurrent carry from d h_new and back out as d h_prev, and the input gradients (d z, d w, d x, the baselines' inputs) are
// formed too.  Their deltas land in the first B rows of the same v* arrays; the operands that the exchange tables read from the
// tape (z, h, h_x) are copied to vcz / vch0 / vch1 / vchx; k_wgrad<false> then runs over four per-call tables of B rows.
//
// Inputs crossing between agents are constants, as in the reference (model.py:807-811, 826-829, 835-843): the sender's and the
// receiver's messages, data, desc and softmax(y) (dbar = softmax(y).detach() . desc, model.py:441-452).  The one exception is
// k_vjp_channel (mmg_exchange_vjp_channel, an option the reference does not have): the sender and the receiver as one graph
// with the gradient crossing the channel through the messages, over the same step functions, tape rows and job tables.
// data and desc are constants of every kernel above; mmg_vjp_input_grads forms their gradients afterwards, from the deltas a VJP
// left in the v* arrays (k_vjp_ddesc, at the end of this file).
#pragma once
#include "device_utils.h"
#include "kernels_tile.h"
#include "layout.h"

namespace mmg {

struct VjpIn {
    const float* dy;     // [n, B, D]   d loss / d y_t                                        (receiver)
    const float* dz;     // [n, B, W]   d loss / d sen_probs_t (binary) | d sen_feats_t (continuous logits)
    const float* dw;     // [n, B, W]   d loss / d rec_probs_t (binary) | d rec_feats_t (continuous logits)
    const float* dps;    // [n, B]      d loss / d s_probs_t
    const float* dbs;    // [n, B]      d loss / d bs_t
    const float* dbr;    // [n, B]      d loss / d br_t
    int n;               // executed steps: upstream gradients exist for t < n only
    int sv;              // k_vjp_sen: the handle's sender variant (SV_* bits, layout.h; 0: the plain sender); sits in what was padding
    float tau_z, tau_w;  // k_vjp_channel_relax: the temperatures of the relaxed messages (mmg_set_message_relaxation); nothing else reads them
};

__device__ __forceinline__ float vjp_block_reduce(float v, float* s_red, bool is_max) {
    // fixed-order reduction over the 256 threads (deterministic): every thread gets the result
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MMG_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_red[threadIdx.x] = is_max ? fmaxf(s_red[threadIdx.x], s_red[threadIdx.x + s])
                                                              : s_red[threadIdx.x] + s_red[threadIdx.x + s];
        __syncthreads();
    }
    const float r = s_red[0];
    __syncthreads();
    return r;
}

// Cd = desc . W_y1[:, R:]^T + b_y1 and a copy of desc inside the workspace (the B operand of the y1.weight[:, R:] job).
// One workgroup per class.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_cd(Dims dm, Params P, Tape tp, const float* __restrict__ desc) {
    const int d = blockIdx.x, R = dm.R, V = dm.V;
    const float* Wy1 = P.p[R_Y1_W];
    for (int v = threadIdx.x; v < V; v += MMG_BLOCK) tp.vdesc[(size_t)d * V + v] = desc[(size_t)d * V + v];
    for (int r = threadIdx.x; r < R; r += MMG_BLOCK) {
        float acc = P.p[R_Y1_B][r];
        for (int v = 0; v < V; ++v) acc = fmaf(Wy1[(size_t)r * (R + V) + R + v], desc[(size_t)d * V + v], acc);
        tp.vCd[(size_t)d * R + r] = acc;
    }
}

// dynamic LDS floats of k_vjp_rec / k_vjp_rec_call
__host__ __device__ inline int vjp_rec_smem_floats(const Dims& d) { return 14 * d.R + 3 * d.W + d.V + 2 * d.D + MMG_BLOCK; }

// One (step, sample) row of the receiver VJP: where the step's forward values and upstream gradients live (row pointers, NULL =
// zero), and the row of the v* arrays it writes.  k_vjp_rec points into the exchange tape, k_vjp_rec_call into the caller's buffers.
struct RecRow {
    const float *h0, *h1, *z, *y, *pw, *ps;    // GRU state before (NULL = zero state) / after the step, message in, y, w / s probs
    const float *dy, *dw, *dps, *dhw;          // d y, d w_probs | d w logits, d s_prob, d h_w
    size_t row;
    // RELAX only (k_vjp_channel_relax): the gradient arriving at the relaxed message w_t, its soft value of the forward pass, tau_rec
    const float *dwm, *wsoft;
    float tau;
};

// The receiver's step backward (model.py:340-474), shared by the exchange and the per-call VJP.  On entry s_car (LDS, R floats)
// holds d h_{t+1} from later uses of the state; on exit it holds d h_t.  Writes the row's deltas the weight-gradient jobs reduce
// (vdgi, vdgh, vdgpre, vdlw, vdls, vdA, vdys) and the recomputed operands (vA, vg, vdbar, the softmax statistics vsm).
// RELAX (relaxed messages, k_vjp_channel_relax): the message gradient io.dwm crosses into the logits with the relaxed sample's own
// derivative ws (1 - ws) / tau, beside the upstream gradient on the probabilities with pw (1 - pw).  A compile-time switch: every
// other caller keeps the code it had.
template <bool RELAX = false>
__device__ __forceinline__ void vjp_rec_step(const Dims& dm, const Params& P, const Tape& tp, float* smem, const RecRow& io) {
    const int D = dm.D, W = dm.W, R = dm.R, V = dm.V;
    const int tid = threadIdx.x;
    float* s_h0 = smem;            float* s_h1 = s_h0 + R;       float* s_r = s_h1 + R;      float* s_u = s_r + R;
    float* s_n = s_u + R;          float* s_ghn = s_n + R;       float* s_g = s_ghn + R;     float* s_dgp = s_g + R;
    float* s_dA = s_dgp + R;       float* s_car = s_dA + R;      float* s_dgh = s_car + R;   /* 3R */
    float* s_z = s_dgh + 3 * R;    float* s_dlw = s_z + W;       float* s_pw = s_dlw + W;
    float* s_dbar = s_pw + W;      float* s_p = s_dbar + V;      float* s_dy = s_p + D;      float* s_red = s_dy + D;
    const float *Wih = P.p[R_WIH], *Whh = P.p[R_WHH], *bih = P.p[R_BIH], *bhh = P.p[R_BHH];
    const float *Wh = P.p[R_WH_W], *bh = P.p[R_WH_B], *Wd = P.p[R_WD_W], *Ww = P.p[R_W_W];
    const float *Wy1 = P.p[R_Y1_W], *w2 = P.p[R_Y2_W], *ws = P.p[R_S_W];
    const bool bin = dm.use_binary;
    const size_t row = io.row;
    __syncthreads();
    for (int i = tid; i < R; i += MMG_BLOCK) { s_h0[i] = io.h0 ? io.h0[i] : 0.f; s_h1[i] = io.h1[i]; }
    for (int j = tid; j < W; j += MMG_BLOCK) { s_z[j] = io.z[j]; s_pw[j] = bin ? io.pw[j] : 0.f; }
    for (int d = tid; d < D; d += MMG_BLOCK) {
        s_p[d] = io.y[d];
        s_dy[d] = io.dy ? io.dy[d] : 0.f;
    }
    // softmax(y_t) . desc (model.py:441-449), a constant of the graph
    float m = -INFINITY;
    for (int d = tid; d < D; d += MMG_BLOCK) m = fmaxf(m, s_p[d]);
    m = vjp_block_reduce(m, s_red, true);
    float sum = 0.f;
    for (int d = tid; d < D; d += MMG_BLOCK) sum += expf(s_p[d] - m);
    sum = vjp_block_reduce(sum, s_red, false);
    float dys = 0.f;
    for (int d = tid; d < D; d += MMG_BLOCK) dys += s_dy[d];
    dys = vjp_block_reduce(dys, s_red, false);                // (ends with a barrier: s_p is complete below)
    for (int d = tid; d < D; d += MMG_BLOCK) s_p[d] = expf(s_p[d] - m) / sum;
    __syncthreads();
    for (int v = tid; v < V; v += MMG_BLOCK) {
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(s_p[d], tp.vdesc[(size_t)d * V + v], acc);
        s_dbar[v] = acc;
        tp.vdbar[row * V + v] = acc;
    }
    if (tid == 0) {
        tp.vdys[row] = dys;
        tp.vsm[row * 2] = m; tp.vsm[row * 2 + 1] = 1.f / sum;  // the row's softmax statistics (k_vjp_ddesc re-forms softmax(y_t))
    }
    // GRU gates of the step (model.py:340): r, u, n and W_hn h + b_hn
    for (int i = tid; i < R; i += MMG_BLOCK) {
        float gr = bih[i] + bhh[i], gu = bih[R + i] + bhh[R + i], gin = bih[2 * R + i], ghn = bhh[2 * R + i];
        for (int k = 0; k < W; ++k) {
            const float zk = s_z[k];
            gr = fmaf(Wih[(size_t)i * W + k], zk, gr);
            gu = fmaf(Wih[(size_t)(R + i) * W + k], zk, gu);
            gin = fmaf(Wih[(size_t)(2 * R + i) * W + k], zk, gin);
        }
        for (int k = 0; k < R; ++k) {
            const float hk = s_h0[k];
            gr = fmaf(Whh[(size_t)i * R + k], hk, gr);
            gu = fmaf(Whh[(size_t)(R + i) * R + k], hk, gu);
            ghn = fmaf(Whh[(size_t)(2 * R + i) * R + k], hk, ghn);
        }
        const float r = sigmoidf_(gr), u = sigmoidf_(gu);
        s_r[i] = r; s_u[i] = u; s_ghn[i] = ghn; s_n[i] = tanhf(gin + r * ghn);
    }
    __syncthreads();                                          // s_dbar complete
    // h_w = tanh(w_h h_{t+1} + w_d dbar) (model.py:452) and A_t = W_y1[:, :R] h_{t+1}
    for (int i = tid; i < R; i += MMG_BLOCK) {
        float gp = bh[i], a = 0.f;
        for (int k = 0; k < R; ++k) {
            gp = fmaf(Wh[(size_t)i * R + k], s_h1[k], gp);
            a = fmaf(Wy1[(size_t)i * (R + V) + k], s_h1[k], a);
        }
        for (int v = 0; v < V; ++v) gp = fmaf(Wd[(size_t)i * V + v], s_dbar[v], gp);
        const float g = tanhf(gp);
        s_g[i] = g;
        tp.vg[row * R + i] = g;
        tp.vA[row * R + i] = a;
        // dA_t[r] = w2[r] sum_d dy_t[d] 1[A_t[r] + Cd[d, r] > 0]   (model.py:432-433)
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += (a + tp.vCd[(size_t)d * R + i] > 0.f) ? s_dy[d] : 0.f;
        s_dA[i] = w2[i] * acc;
        tp.vdA[row * R + i] = s_dA[i];
    }
    // message seeds: sigmoid' of the receiver's message probabilities (model.py:456) or the logits' gradient directly (:474)
    for (int j = tid; j < W; j += MMG_BLOCK) {
        float dl = 0.f;
        if (io.dw) {
            const float gw = io.dw[j];
            dl = bin ? gw * s_pw[j] * (1.f - s_pw[j]) : gw;
        }
        if (RELAX) { const float sw = io.wsoft[j]; dl += io.dwm[j] * (sw * (1.f - sw) / io.tau); }
        s_dlw[j] = dl;
        tp.vdlw[row * W + j] = dl;
    }
    float dls = 0.f;
    if (io.dps) { const float ps = io.ps[0]; dls = io.dps[0] * ps * (1.f - ps); }
    if (tid == 0) tp.vdls[row] = dls;
    __syncthreads();
    for (int i = tid; i < R; i += MMG_BLOCK) {
        float dg = io.dhw ? io.dhw[i] : 0.f;                  // (d h_w from a use of receiver.h_w: per-call VJP only)
        for (int j = 0; j < W; ++j) dg = fmaf(Ww[(size_t)j * R + i], s_dlw[j], dg);
        const float g = s_g[i], dgp = dg * (1.f - g * g);
        s_dgp[i] = dgp;
        tp.vdgpre[row * R + i] = dgp;
    }
    __syncthreads();
    // d h_{t+1}: recurrence + w_h + s + the y head; then the GRU cell backward
    for (int i = tid; i < R; i += MMG_BLOCK) {
        float dh = s_car[i] + dls * ws[i];
        for (int k = 0; k < R; ++k) {
            dh = fmaf(Wh[(size_t)k * R + i], s_dgp[k], dh);
            dh = fmaf(Wy1[(size_t)k * (R + V) + i], s_dA[k], dh);
        }
        const float r = s_r[i], u = s_u[i], nn = s_n[i];
        const float dnp = dh * (1.f - u) * (1.f - nn * nn);
        const float dup = dh * (s_h0[i] - nn) * u * (1.f - u);
        const float drp = dnp * s_ghn[i] * r * (1.f - r);
        float* dgi = tp.vdgi + row * 3 * R;
        float* dgh = tp.vdgh + row * 3 * R;
        dgi[i] = drp; dgi[R + i] = dup; dgi[2 * R + i] = dnp;
        dgh[i] = drp; dgh[R + i] = dup; dgh[2 * R + i] = dnp * r;
        s_dgh[i] = drp; s_dgh[R + i] = dup; s_dgh[2 * R + i] = dnp * r;
        s_car[i] = dh * u;                                    // (own entry: read above by this thread only)
    }
    __syncthreads();
    for (int i = tid; i < R; i += MMG_BLOCK) {
        float c = s_car[i];
        for (int k = 0; k < 3 * R; ++k) c = fmaf(Whh[(size_t)k * R + i], s_dgh[k], c);
        s_car[i] = c;
    }
}

// Receiver (model.py:303-477): one workgroup per sample, reverse time from t = T - 1.  Seeds at every step come from the upstream
// gradients (dls = dps ps (1 - ps), dlw = dpw pw (1 - pw) or dw, dA_t from dy_t); backprop through time over the GRU state.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_rec(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, B = dm.B, D = dm.D, W = dm.W, R = dm.R, T = dm.T;
    float* s_car = smem + 9 * R;                              // (vjp_rec_step's carry slot)
    for (int i = threadIdx.x; i < R; i += MMG_BLOCK) s_car[i] = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        const bool live = t < in.n;
        RecRow io;
        io.h0 = tp.h + row * R; io.h1 = tp.h + row * R + (size_t)B * R; io.z = tp.z + row * W; io.y = tp.y + row * D;
        io.pw = tp.pw + row * W; io.ps = tp.ps + row;
        io.dy = (live && in.dy) ? in.dy + row * D : nullptr;
        io.dw = (live && in.dw) ? in.dw + row * W : nullptr;
        io.dps = (live && in.dps) ? in.dps + row : nullptr;
        io.dhw = nullptr;
        io.row = row;
        vjp_rec_step(dm, P, tp, smem, io);
    }
}

// The caller-side buffers of one receiver call (mmg_receiver_vjp): the call's inputs, outputs and upstream gradients, [B, .] each.
struct RecCall {
    const float *z, *h_prev, *h_new, *y, *w_probs, *s_prob;
    const float *dy, *dw, *dps, *dh_w, *dh_new;
    float *dz, *dh_prev;
    int dz_tiles;              // d z is formed by k_vjp_nn (MFMA) after this kernel, from vdgi
};

// Receiver, one call: one workgroup per sample, vjp_rec_step on row b with the carry taken from d h_new and returned as d h_prev,
// plus d z = W_ih^T dgi (here when the shape keeps it off the MFMA tiles, else k_vjp_nn).  Copies the operands of its weight-gradient jobs (z, h_prev, h_new) in front of the job tables.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_rec_call(Dims dm, Params P, Tape tp, RecCall c) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, D = dm.D, W = dm.W, R = dm.R, tid = threadIdx.x;
    float* s_car = smem + 9 * R;
    for (int i = tid; i < R; i += MMG_BLOCK) {
        s_car[i] = c.dh_new ? c.dh_new[(size_t)b * R + i] : 0.f;
        tp.vch0[(size_t)b * R + i] = c.h_prev ? c.h_prev[(size_t)b * R + i] : 0.f;
        tp.vch1[(size_t)b * R + i] = c.h_new[(size_t)b * R + i];
    }
    for (int j = tid; j < W; j += MMG_BLOCK) tp.vcz[(size_t)b * W + j] = c.z[(size_t)b * W + j];
    RecRow io;
    io.h0 = c.h_prev ? c.h_prev + (size_t)b * R : nullptr; io.h1 = c.h_new + (size_t)b * R; io.z = c.z + (size_t)b * W;
    io.y = c.y + (size_t)b * D; io.pw = c.w_probs ? c.w_probs + (size_t)b * W : nullptr; io.ps = c.s_prob ? c.s_prob + b : nullptr;
    io.dy = c.dy ? c.dy + (size_t)b * D : nullptr;
    io.dw = c.dw ? c.dw + (size_t)b * W : nullptr;
    io.dps = c.dps ? c.dps + b : nullptr;
    io.dhw = c.dh_w ? c.dh_w + (size_t)b * R : nullptr;
    io.row = b;
    vjp_rec_step(dm, P, tp, smem, io);
    __syncthreads();                                          // s_car and this row of vdgi complete
    if (c.dh_prev)
        for (int i = tid; i < R; i += MMG_BLOCK) c.dh_prev[(size_t)b * R + i] = s_car[i];
    if (c.dz && !c.dz_tiles) {
        const float* Wih = P.p[R_WIH];
        const float* dgi = tp.vdgi + (size_t)b * 3 * R;
        for (int k = tid; k < W; k += MMG_BLOCK) {
            float acc = 0.f;
            for (int i = 0; i < 3 * R; ++i) acc = fmaf(Wih[(size_t)i * W + k], dgi[i], acc);
            c.dz[(size_t)b * W + k] = acc;
        }
    }
}

// Class side of the receiver: dC[d, r] = w2[r] sum_{t < n, b} dy_t[b, d] 1[A_t[b, r] + Cd[d, r] > 0] (-> y1.weight[:, R:], y1.bias)
// and Py2[d, r] = sum_{t < n, b} dy_t[b, d] relu(A_t[b, r] + Cd[d, r]) (-> y2.weight).  One workgroup per class.  The per-call VJP
// runs it with n = 1 over the call's B rows.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_class(Dims dm, Params P, Tape tp, VjpIn in) {
    const int d = blockIdx.x, B = dm.B, D = dm.D, R = dm.R;
    for (int r = threadIdx.x; r < R; r += MMG_BLOCK) {
        const float cd = tp.vCd[(size_t)d * R + r];
        float dc = 0.f, py = 0.f;
        if (in.dy)
            for (int row = 0; row < in.n * B; ++row) {
                const float g = in.dy[(size_t)row * D + d];
                const float pre = tp.vA[(size_t)row * R + r] + cd;
                if (pre > 0.f) { dc += g; py = fmaf(g, pre, py); }
            }
        tp.vdC[(size_t)d * R + r] = P.p[R_Y2_W][r] * dc;
        tp.vPy2[(size_t)d * R + r] = py;
    }
}

__host__ __device__ inline int vjp_sen_smem_floats(const Dims& d) { return 4 * d.H + 2 * d.W; }

// The sender's step backward (model.py:195-238), shared by the exchange and the per-call VJP.  s_hx (LDS) holds h_x of the sample;
// c: the code input w_{t-1} (NULL: sigmoid(code_bias), t = 0), pz: the message probabilities (binary), dz: d probs | d logits
// (NULL = zero).  Adds d pre of the step to s_dhx and leaves it in s_dpre.
// VAR (a handle with a sender variant; sv: SV_* bits, wave-uniform): with a = tanh(h_x * h_w) (SV_PROD, model.py:217-218) the step adds
// d h_x = dpre * h_w to s_dhx and leaves d h_w = dpre * h_x in s_dpre / vdpre -- the operand of code_layer's jobs and of W_c^T .
// (code_bias, d w) --; with a = tanh(h_x) (SV_IGNORE_CODE, model.py:208-210) d h_x = dpre and d h_w = 0 exactly.  A compile-time
// switch: the callers without a variant (k_vjp_channel among them) keep the code they had.
// RELAX (relaxed messages, k_vjp_channel_relax): dzm is the gradient arriving at the relaxed message z_t and zsoft its soft value of the
// forward pass; it crosses into the logits as zs (1 - zs) / tau, beside dz pz (1 - pz).  Likewise a compile-time switch.
template <bool VAR = false, bool RELAX = false>
__device__ __forceinline__ void vjp_sen_step(const Dims& dm, const Params& P, const Tape& tp, float* smem, const float* c,
                                             const float* pz, const float* dz, size_t row, int sv = 0, const float* dzm = nullptr,
                                             const float* zsoft = nullptr, float tau = 1.f) {
    const int H = dm.H, W = dm.W, tid = threadIdx.x;
    float* s_hx = smem;  float* s_a = s_hx + H;  float* s_dpre = s_a + H;  float* s_dhx = s_dpre + H;
    float* s_c = s_dhx + H;  float* s_dlz = s_c + W;
    const float *Wc = P.p[S_CODE_W], *bc = P.p[S_CODE_B], *cb = P.p[S_CODE_BIAS], *Wb = P.p[S_BIN_W];
    const bool bin = dm.use_binary;
    __syncthreads();
    for (int j = tid; j < W; j += MMG_BLOCK) {
        const float cj = c ? c[j] : sigmoidf_(cb[j]);
        s_c[j] = cj;
        tp.vc[row * W + j] = cj;
        float dl = 0.f;
        if (dz) {
            const float g = dz[j];
            if (bin) { const float p = pz[j]; dl = g * p * (1.f - p); } else dl = g;
        }
        if (RELAX) { const float sz = zsoft[j]; dl += dzm[j] * (sz * (1.f - sz) / tau); }
        s_dlz[j] = dl;
        tp.vdlz[row * W + j] = dl;
    }
    __syncthreads();
    for (int h = tid; h < H; h += MMG_BLOCK) {
        float pre = s_hx[h] + bc[h];
        float fx = 1.f, fw = 1.f;                             // VAR: d h_x = dpre * fx, d h_w = dpre * fw
        if (VAR && (sv & SV_IGNORE_CODE)) {
            pre = s_hx[h]; fw = 0.f;
        } else if (VAR && (sv & SV_PROD)) {
            float hw = bc[h];
            for (int j = 0; j < W; ++j) hw = fmaf(Wc[(size_t)h * W + j], s_c[j], hw);
            pre = s_hx[h] * hw; fx = hw; fw = s_hx[h];
        } else {
            for (int j = 0; j < W; ++j) pre = fmaf(Wc[(size_t)h * W + j], s_c[j], pre);
        }
        const float a = tanhf(pre);
        s_a[h] = a;
        tp.va[row * H + h] = a;
        float da = 0.f;
        for (int j = 0; j < W; ++j) da = fmaf(Wb[(size_t)j * H + h], s_dlz[j], da);
        const float dp = da * (1.f - a * a);
        const float dw = VAR ? dp * fw : dp;
        s_dpre[h] = dw;
        tp.vdpre[row * H + h] = dw;
        s_dhx[h] += VAR ? dp * fx : dp;
    }
}

// Sender (model.py:144-238): one workgroup per sample.  dlz = dpz pz (1 - pz) (binary) or dz (continuous logits), dpre =
// (W_b^T dlz)(1 - a^2), dhx = sum_t dpre, and at t = 0 the code_bias path W_c^T dpre_0 (model.py:196-200).
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_sen(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, B = dm.B, H = dm.H, W = dm.W, T = dm.T, tid = threadIdx.x;
    float* s_hx = smem;  float* s_dpre = s_hx + 2 * H;  float* s_dhx = s_dpre + H;
    const float *Wc = P.p[S_CODE_W], *cb = P.p[S_CODE_BIAS];
    if (b == 0)
        for (int j = tid; j < W; j += MMG_BLOCK) { const float s = sigmoidf_(cb[j]); tp.vdsig[j] = s * (1.f - s); }
    for (int h = tid; h < H; h += MMG_BLOCK) { s_hx[h] = tp.hx[(size_t)b * H + h]; s_dhx[h] = 0.f; }
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)t * B + b;
        const bool live = t < in.n;
        const float* c = t == 0 ? nullptr : tp.w + (row - B) * W;                 // (the receiver's previous message)
        const float* dz = (live && in.dz) ? in.dz + row * W : nullptr;
        if (in.sv) vjp_sen_step<true>(dm, P, tp, smem, c, tp.pz + row * W, dz, row, in.sv);
        else vjp_sen_step(dm, P, tp, smem, c, tp.pz + row * W, dz, row);
        if (t == 0) {
            __syncthreads();
            for (int j = tid; j < W; j += MMG_BLOCK) {
                float acc = 0.f;
                for (int h = 0; h < H; ++h) acc = fmaf(Wc[(size_t)h * W + j], s_dpre[h], acc);
                tp.vdc0[(size_t)b * W + j] = acc;
            }
        }
    }
    __syncthreads();
    for (int h = tid; h < H; h += MMG_BLOCK) tp.vdhx[(size_t)b * H + h] = s_dhx[h];
}

// dynamic LDS floats of k_vjp_channel: the receiver's and the sender's step areas, then the two message-gradient rows
__host__ __device__ inline int vjp_channel_smem_floats(const Dims& d) {
    return vjp_rec_smem_floats(d) + vjp_sen_smem_floats(d) + 2 * d.W;
}

// Sender and receiver as ONE graph (mmg_exchange_vjp_channel): the messages are NOT detached, so the gradient of the receiver's
// GRU input z_t flows into the sender's step t and the gradient of the sender's code input w_{t-1} into the receiver's step
// t - 1.  One workgroup per sample, one reverse-time loop running both agents' steps (vjp_rec_step, vjp_sen_step):
//   s_dw = dw_up[t] + q_{t+1}      -> receiver step t   (q_{t+1} = W_c^T dpre_{t+1}, the cross term of the sender's step t + 1)
//   s_dz = dz_up[t] + W_ih^T dgi_t -> sender step t
// Continuous messages: both rows are logit gradients, exact.  Binary: they are d loss / d probabilities and the steps' own
// p (1 - p) factor applies -- the straight-through estimator z = pz + stopgrad(bits - pz), w = pw + stopgrad(bits - pw).
// Rows of steps t >= n get zero deltas: both carries start at zero and the cross terms are linear in the upstream gradients.
// Writes the rows the receiver's and the sender's job tables reduce; the stop bit, softmax(y) inside dbar, data and desc stay
// constants.
// RELAX (a handle with relaxed messages, mmg_set_message_relaxation): the messages are the relaxed samples (or their bits, hard), whose
// soft values the forward pass left in tape.zs / tape.ws.  The cross terms and the upstream gradients no longer share one factor:
//   dlz_t = dz_up[t] pz (1 - pz) + (W_ih^T dgi_t) zs (1 - zs) / tau_sen;   dlw_t = dw_up[t] pw (1 - pw) + q_{t+1} ws (1 - ws) / tau_rec
// so s_dw / s_dz carry the cross terms alone and the steps read the upstream rows themselves.
template <bool RELAX>
__device__ __forceinline__ void vjp_channel_body(const Dims& dm, const Params& P, const Tape& tp, const VjpIn& in, float* smem) {
    const int b = blockIdx.x, B = dm.B, D = dm.D, H = dm.H, W = dm.W, R = dm.R, T = dm.T, tid = threadIdx.x;
    float* rsm = smem;                                        // vjp_rec_step's area
    float* ssm = rsm + vjp_rec_smem_floats(dm);               // vjp_sen_step's area
    float* s_dw = ssm + vjp_sen_smem_floats(dm);
    float* s_dz = s_dw + W;
    float* s_car = rsm + 9 * R;                               // (vjp_rec_step's carry slot)
    float* s_hx = ssm;  float* s_dpre = s_hx + 2 * H;  float* s_dhx = s_dpre + H;
    const float *Wih = P.p[R_WIH], *Wc = P.p[S_CODE_W], *cb = P.p[S_CODE_BIAS];
    if (b == 0)
        for (int j = tid; j < W; j += MMG_BLOCK) { const float s = sigmoidf_(cb[j]); tp.vdsig[j] = s * (1.f - s); }
    for (int i = tid; i < R; i += MMG_BLOCK) s_car[i] = 0.f;
    for (int h = tid; h < H; h += MMG_BLOCK) { s_hx[h] = tp.hx[(size_t)b * H + h]; s_dhx[h] = 0.f; }
    for (int j = tid; j < W; j += MMG_BLOCK)
        s_dw[j] = (!RELAX && T - 1 < in.n && in.dw) ? in.dw[((size_t)(T - 1) * B + b) * W + j] : 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        const bool live = t < in.n;
        RecRow io;
        io.h0 = tp.h + row * R; io.h1 = tp.h + row * R + (size_t)B * R; io.z = tp.z + row * W; io.y = tp.y + row * D;
        io.pw = tp.pw + row * W; io.ps = tp.ps + row;
        io.dy = (live && in.dy) ? in.dy + row * D : nullptr;
        io.dw = s_dw;
        if (RELAX) { io.dw = (live && in.dw) ? in.dw + row * W : nullptr; io.dwm = s_dw; io.wsoft = tp.ws + row * W; io.tau = in.tau_w; }
        io.dps = (live && in.dps) ? in.dps + row : nullptr;
        io.dhw = nullptr;
        io.row = row;
        vjp_rec_step<RELAX>(dm, P, tp, rsm, io);
        __syncthreads();                                      // this row of vdgi complete
        const float* dgi = tp.vdgi + row * 3 * R;
        for (int k = tid; k < W; k += MMG_BLOCK) {            // d z_t = W_ih^T dgi_t
            float acc = 0.f;
            for (int i = 0; i < 3 * R; ++i) acc = fmaf(Wih[(size_t)i * W + k], dgi[i], acc);
            s_dz[k] = acc + ((!RELAX && live && in.dz) ? in.dz[row * W + k] : 0.f);
        }
        if (RELAX) vjp_sen_step<false, true>(dm, P, tp, ssm, t == 0 ? nullptr : tp.w + (row - B) * W, tp.pz + row * W,
                                             (live && in.dz) ? in.dz + row * W : nullptr, row, 0, s_dz, tp.zs + row * W, in.tau_z);
        else vjp_sen_step(dm, P, tp, ssm, t == 0 ? nullptr : tp.w + (row - B) * W, tp.pz + row * W, s_dz, row);
        __syncthreads();                                      // s_dpre complete
        for (int j = tid; j < W; j += MMG_BLOCK) {            // d w_{t-1} = W_c^T dpre_t (t = 0: the code_bias path)
            float acc = 0.f;
            for (int h = 0; h < H; ++h) acc = fmaf(Wc[(size_t)h * W + j], s_dpre[h], acc);
            if (t == 0) tp.vdc0[(size_t)b * W + j] = acc;
            else s_dw[j] = acc + ((!RELAX && t - 1 < in.n && in.dw) ? in.dw[(row - B) * W + j] : 0.f);
        }
    }
    __syncthreads();
    for (int h = tid; h < H; h += MMG_BLOCK) tp.vdhx[(size_t)b * H + h] = s_dhx[h];
}

__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_channel(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    vjp_channel_body<false>(dm, P, tp, in, smem);
}

// ... of a handle with relaxed messages (mmg_set_message_relaxation): the two-factor rule above
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_channel_relax(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    vjp_channel_body<true>(dm, P, tp, in, smem);
}

// The caller-side buffers of one sender call (mmg_sender_vjp), [B, .] each.  w: the code input (t > 0).
struct SenCall {
    const float *w, *h_x, *probs, *dout, *dh_x;
    float *dx, *dw;
    int t;
    int q_tiles, dx_tiles;     // W_c^T dpre / d x are formed by k_vjp_nn (MFMA) after this kernel, from vdpre / vdhx
    int sv;                    // the handle's sender variant (SV_* bits, layout.h; 0: the plain sender); sits in what was padding
};

// Sender, one call: one workgroup per sample.  vjp_sen_step on row b, then W_c^T dpre -> the code_bias path (t = 0) or d w (t > 0),
// d h_x = dpre + the upstream gradient of sender.h_x (-> image_layer) and d x = W_img^T d h_x.  The two products run here only
// when the shape keeps them off the MFMA tiles (q_tiles / dx_tiles: k_vjp_nn).
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_sen_call(Dims dm, Params P, Tape tp, const float* __restrict__ x, SenCall c) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, H = dm.H, W = dm.W, F = dm.F, tid = threadIdx.x;
    float* s_hx = smem;  float* s_dpre = s_hx + 2 * H;  float* s_dhx = s_dpre + H;
    const float *Wc = P.p[S_CODE_W], *cb = P.p[S_CODE_BIAS], *Wi = P.p[S_IMG_W];
    if (b == 0)
        for (int j = tid; j < W; j += MMG_BLOCK) { const float s = sigmoidf_(cb[j]); tp.vdsig[j] = s * (1.f - s); }
    for (int h = tid; h < H; h += MMG_BLOCK) { s_hx[h] = c.h_x[(size_t)b * H + h]; s_dhx[h] = 0.f; }
    if (c.sv) vjp_sen_step<true>(dm, P, tp, smem, c.t == 0 ? nullptr : c.w + (size_t)b * W, c.probs ? c.probs + (size_t)b * W : nullptr,
                                 c.dout ? c.dout + (size_t)b * W : nullptr, b, c.sv);
    else vjp_sen_step(dm, P, tp, smem, c.t == 0 ? nullptr : c.w + (size_t)b * W, c.probs ? c.probs + (size_t)b * W : nullptr,
                      c.dout ? c.dout + (size_t)b * W : nullptr, b);
    __syncthreads();
    for (int j = tid; j < W; j += MMG_BLOCK) {
        if (c.q_tiles) {                                      // (k_vjp_nn writes vdc0 at t = 0 and d w after)
            if (c.t > 0) tp.vdc0[(size_t)b * W + j] = 0.f;
            continue;
        }
        float acc = 0.f;
        for (int h = 0; h < H; ++h) acc = fmaf(Wc[(size_t)h * W + j], s_dpre[h], acc);
        tp.vdc0[(size_t)b * W + j] = c.t == 0 ? acc : 0.f;
        if (c.t > 0 && c.dw) c.dw[(size_t)b * W + j] = acc;
    }
    for (int h = tid; h < H; h += MMG_BLOCK) {
        const float dh = s_dhx[h] + (c.dh_x ? c.dh_x[(size_t)b * H + h] : 0.f);
        s_dhx[h] = dh;
        tp.vdhx[(size_t)b * H + h] = dh;
    }
    if (c.dx && !c.dx_tiles) {
        __syncthreads();
        for (int f = tid; f < F; f += MMG_BLOCK) {
            float acc = 0.f;
            for (int h = 0; h < H; ++h) acc = fmaf(Wi[(size_t)h * F + f], s_dhx[h], acc);
            c.dx[(size_t)b * F + f] = acc;
        }
    }
}

// relu(linear1(in)) of one baseline row (model.py:513), in: the row's nin inputs in LDS.  Shared by both baseline VJPs.
__device__ __forceinline__ void vjp_bas_hidden(int K, int nin, const float* W1, const float* b1, const float* in, float* hid) {
    for (int k = threadIdx.x; k < K; k += MMG_BLOCK) {
        float acc = b1[k];
        for (int i = 0; i < nin; ++i) acc = fmaf(W1[(size_t)k * nin + i], in[i], acc);
        hid[k] = fmaxf(acc, 0.f);
    }
}

// Baselines (model.py:496-516): one workgroup per (step, sample) row.  The hidden units relu(linear1([..])) of the row and the
// upstream score gradient (zero for t >= n) -- the virtual-operand jobs of k_wgrad form d hidden = dscore * w2 * 1[hidden > 0].
// which: MMG agent index (2 = baseline_rec: [z_t || h_{t+1}], 3 = baseline_sen: [h_x || z_r,t], z_r,0 = first_rec).
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_bas(Dims dm, Params P, Tape tp, VjpIn in, int which) {
    extern __shared__ float smem[];
    const int row = blockIdx.x, B = dm.B, H = dm.H, W = dm.W, R = dm.R, K = dm.K;
    const int t = row / B, b = row - t * B;
    const bool rec = which == 2;
    const int nin = rec ? W + R : H + W;
    for (int i = threadIdx.x; i < nin; i += MMG_BLOCK) {
        float v;
        if (rec) v = i < W ? tp.z[(size_t)row * W + i] : tp.h[((size_t)row + B) * R + (i - W)];
        else if (i < H) v = tp.hx[(size_t)b * H + i];
        else {
            v = (t == 0) ? dm.first_rec : tp.w[((size_t)row - B) * W + (i - H)];
            tp.vzr[(size_t)row * W + (i - H)] = v;
        }
        smem[i] = v;
    }
    __syncthreads();
    vjp_bas_hidden(K, nin, P.p[rec ? BR_L1_W : BS_L1_W], P.p[rec ? BR_L1_B : BS_L1_B], smem,
                   (rec ? tp.vhid_r : tp.vhid_s) + (size_t)row * K);
    if (threadIdx.x == 0) {
        const float* up = rec ? in.dbr : in.dbs;
        (rec ? tp.vdbr : tp.vdbs)[row] = (t < in.n && up) ? up[row] : 0.f;
    }
}

// The caller-side buffers of one baseline call (mmg_baseline_vjp), [B, .] each: baseline_rec reads (binary, inp), baseline_sen
// (x, binary).
struct BasCall {
    const float *x, *binary, *inp, *dscore;
    float *dx, *dbinary, *dinp;
    int tiles;                 // the input gradients are formed by k_vjp_nn (MFMA) from d hidden (vcdh) after this kernel
};

__host__ __device__ inline int vjp_bas_call_smem_floats(const Dims& d, int which) {
    return (which == 2 ? d.W + d.R : d.H + d.W) + d.K;
}

// Baseline, one call: one workgroup per sample.  The hidden units (vjp_bas_hidden) and d score of the row for the weight-gradient
// jobs, copies of the inputs in front of the job tables, and the input gradients W1^T (dscore * w2 * 1[hidden > 0]) -- here, or
// (tiles) d hidden into vcdh for k_vjp_nn.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_bas_call(Dims dm, Params P, Tape tp, BasCall c, int which) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, H = dm.H, W = dm.W, R = dm.R, K = dm.K, tid = threadIdx.x;
    const bool rec = which == 2;
    const int n1 = rec ? W : H, nin = rec ? W + R : H + W;
    const float* in1 = rec ? c.binary : c.x;                  // the two inputs in linear1's column order
    const float* in2 = rec ? c.inp : c.binary;
    float* cp1 = rec ? tp.vcz : tp.vchx;
    float* cp2 = rec ? tp.vch1 : tp.vcz;
    float* s_dhid = smem + nin;
    for (int i = tid; i < nin; i += MMG_BLOCK) {
        float v;
        if (i < n1) { v = in1[(size_t)b * n1 + i]; cp1[(size_t)b * n1 + i] = v; }
        else { v = in2[(size_t)b * (nin - n1) + (i - n1)]; cp2[(size_t)b * (nin - n1) + (i - n1)] = v; }
        smem[i] = v;
    }
    __syncthreads();
    const float* W1 = P.p[rec ? BR_L1_W : BS_L1_W];
    const float* w2 = P.p[rec ? BR_L2_W : BS_L2_W];
    float* hid = (rec ? tp.vhid_r : tp.vhid_s) + (size_t)b * K;
    vjp_bas_hidden(K, nin, W1, P.p[rec ? BR_L1_B : BS_L1_B], smem, hid);
    const float ds = c.dscore ? c.dscore[b] : 0.f;
    if (tid == 0) (rec ? tp.vdbr : tp.vdbs)[b] = ds;
    float* dout1 = rec ? c.dbinary : c.dx;
    float* dout2 = rec ? c.dinp : c.dbinary;
    if (!dout1 && !dout2) return;
    if (c.tiles) {
        for (int k = tid; k < K; k += MMG_BLOCK) tp.vcdh[(size_t)b * K + k] = hid[k] > 0.f ? ds * w2[k] : 0.f;
        return;
    }
    for (int k = tid; k < K; k += MMG_BLOCK) s_dhid[k] = hid[k] > 0.f ? ds * w2[k] : 0.f;   // (hid[k]: this thread's own store)
    __syncthreads();
    for (int i = tid; i < nin; i += MMG_BLOCK) {
        float* dst = i < n1 ? dout1 : dout2;
        if (!dst) continue;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(W1[(size_t)k * nin + i], s_dhid[k], acc);
        if (i < n1) dst[(size_t)b * n1 + i] = acc;
        else dst[(size_t)b * (nin - n1) + (i - n1)] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// The per-call-only products on the matrix cores: C[b, n] = sum_k A[b, k] Bm[k, n] over the B rows of one call, Bm a PyTorch
// [out, in] weight read "NN" (n contiguous) -- d z = dgi . W_ih, d x = d h_x . W_img, dpre . W_c, d hidden . W1[:, cols].
// One workgroup per 16-sample tile (blockIdx.x) and product (blockIdx.y: up to two products per launch); the A rows are staged
// in LDS, zero-padded, and tgemm_nn_raw (kernels_tile.h) runs the fp32 MFMA tiles.  The k-parts are added in a fixed order:
// deterministic.  Host: vjp_nn_fits decides per product (N, ldb multiples of 4, Bm 16-byte aligned, LDS within 64 KiB); a
// product that does not fit stays in its per-sample kernel.
// ---------------------------------------------------------------------------------------------
struct NnProd { const float* A; const float* Bm; float* C; int lda, ldb, ldc, N, K; };

__host__ __device__ inline int vjp_nn_smem_floats(int N, int K) { return MMG_TM * ld16(K) + tile_raw_floats_nn(N, MMG_BLOCK / 64); }

__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_nn(int B, NnProd p0, NnProd p1) {
    extern __shared__ float smem[];
    const NnProd p = blockIdx.y ? p1 : p0;
    const int b0 = blockIdx.x * MMG_TM, nw = MMG_BLOCK / 64, wave = threadIdx.x >> 6;
    const int lda = ld16(p.K);
    float* sA = smem;
    float* raw = smem + MMG_TM * lda;
    for (int e = threadIdx.x; e < MMG_TM * lda; e += MMG_BLOCK) {
        const int m = e / lda, k = e - m * lda;
        sA[e] = (b0 + m < B && k < p.K) ? p.A[(size_t)(b0 + m) * p.lda + k] : 0.f;
    }
    __syncthreads();
    tgemm_nn_raw(sA, lda, p.Bm, p.ldb, p.N, p.K, raw, wave, nw);
    __syncthreads();
    const int ldr = ld16(p.N), kparts = tile_kparts((p.N + 63) >> 6, nw);
    for (int e = threadIdx.x; e < MMG_TM * p.N; e += MMG_BLOCK) {
        const int m = e / p.N, n = e - m * p.N;
        if (b0 + m < B) p.C[(size_t)(b0 + m) * p.ldc + n] = raw_sum(raw, ldr, kparts, m, n);
    }
}

// The same product for a shape vjp_nn_fits turns down (N or ldb no multiple of 4, the LDS plan beyond 64 KiB): one thread per
// output element, k in order.  Only mmg_vjp_input_grads needs it -- the per-call kernels form such a product themselves.
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_nn_plain(int rows, NnProd p) {
    const size_t total = (size_t)rows * p.N;
    for (size_t e = (size_t)blockIdx.x * MMG_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * MMG_BLOCK) {
        const size_t m = e / p.N;
        const int n = (int)(e - m * p.N);
        float acc = 0.f;
        for (int k = 0; k < p.K; ++k) acc = fmaf(p.A[m * p.lda + k], p.Bm[(size_t)k * p.ldb + n], acc);
        p.C[m * p.ldc + n] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Input gradients (mmg_vjp_input_grads): the game's two inputs, data and desc, as differentiable inputs of the graphs above.
//   d data[b, :] = vdhx[b, :] . W_image                     data enters through image_layer only (model.py:195; baseline_sen reads
//                                                            h_x detached, model.py:835)                                  -> k_vjp_nn
//   d desc[d, :] = sum_r vdC[d, r] W_y1[r, R:]               through Cd (model.py:432 over build_inp)
//                + sum_{t < n, b} pi_t[b, d] q_t[b, :]       through dbar = pi_t . desc (model.py:442-452), pi_t = softmax(y_t) a
//                                                            constant (model.py:441), q_t = vdgpre_t . W_d (vdq, k_vjp_nn)
// k_vjp_ddesc forms d desc: a [D x rows] . [rows x V] product over the rows = n * B executed (step, sample) rows plus the K = R
// product of the Cd term, in fp32 on the matrix cores (v_mfma_f32_16x16x4_f32: bit for bit an fmaf chain in k order).
// One workgroup owns one output tile, 16 classes x MMG_DDESC_VT columns of desc; its four waves split the rows in groups of 16
// (group g -> wave g & 3) and the k-steps of the Cd term the same way, four accumulator tiles per wave.  Lane (i = l & 15,
// q = l >> 4) holds A[class i][k = q] and B[k = q][column i] of a k-step of four rows.  The Pi^T operand never exists in memory:
// a lane forms its element exp(y - m) * inv from the row statistics vjp_rec_step left in vsm -- every element feeds exactly one
// lane (the wave owns the row, the lane the class), so a round trip through LDS would only add a barrier per group.  Loads are
// branch-free (indices clamped, the A element zeroed instead) and those of a whole group are in flight together.  The waves'
// partial tiles meet in LDS and are added in wave order: no atomics, no cross-workgroup traffic, bit-identical from run to run.
// D, V and rows need not be multiples of anything; rows of steps t >= n are never read, so they contribute exactly zero.
// ---------------------------------------------------------------------------------------------
#define MMG_DDESC_VT 64

__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_ddesc(Dims dm, Params P, Tape tp, const float* __restrict__ y, int rows,
                                                         float* __restrict__ ddesc) {
    __shared__ float s_part[MMG_BLOCK / 64][16][MMG_DDESC_VT + 4];
    const int D = dm.D, V = dm.V, R = dm.R;
    const int d0 = blockIdx.x * 16, v0 = blockIdx.y * MMG_DDESC_VT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = MMG_BLOCK / 64, i = lane & 15, q = lane >> 4;
    const bool dok = d0 + i < D;
    const int dc = min(d0 + i, D - 1);
    int vc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vc[j] = min(v0 + 16 * j + i, V - 1);        // (clamped columns: computed, never written)
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // sum over the executed (step, sample) rows of pi[row, d] q[row, v]
    const float* sm = tp.vsm;
    const float* dq = tp.vdq;
    const int ngroups = (rows + 15) >> 4;
    for (int g = wave; g < ngroups; g += nw) {
        float yv[4], mx[4], inv[4], b[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rc = min(g * 16 + u * 4 + q, rows - 1);
            yv[u] = y[(size_t)rc * D + dc]; mx[u] = sm[(size_t)rc * 2]; inv[u] = sm[(size_t)rc * 2 + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[u][j] = dq[(size_t)rc * V + vc[j]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float a = (dok && g * 16 + u * 4 + q < rows) ? expf(yv[u] - mx[u]) * inv[u] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma16(a, b[u][j], acc[j]);
        }
    }
    // + sum_r vdC[d, r] W_y1[r, R + v]
    const float* Wy1 = P.p[R_Y1_W];
    const int cgroups = (R + 15) >> 4;
    for (int g = wave; g < cgroups; g += nw) {
        float av[4], b[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rc = min(g * 16 + u * 4 + q, R - 1);
            av[u] = tp.vdC[(size_t)dc * R + rc];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[u][j] = Wy1[(size_t)rc * (R + V) + R + vc[j]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float a = (dok && g * 16 + u * 4 + q < R) ? av[u] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma16(a, b[u][j], acc[j]);
        }
    }
    // accumulator tile j: column i, rows 4 q + r in register r
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_part[wave][q * 4 + r][16 * j + i] = acc[j][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * MMG_DDESC_VT; e += MMG_BLOCK) {
        const int m = e / MMG_DDESC_VT, n = e - m * MMG_DDESC_VT;
        if (d0 + m < D && v0 + n < V) {
            float v = s_part[0][m][n];
            for (int w = 1; w < nw; ++w) v += s_part[w][m][n];
            ddesc[(size_t)(d0 + m) * V + v0 + n] = v;
        }
    }
}

}  // namespace mmg
