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
// Inputs crossing between agents are constants, as in the reference (model.py:807-811, 826-829, 835-843): the sender's and the
// receiver's messages, data, desc and softmax(y) (dbar = softmax(y).detach() . desc, model.py:441-452).
#pragma once
#include "device_utils.h"
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

// dynamic LDS floats of k_vjp_rec
__host__ __device__ inline int vjp_rec_smem_floats(const Dims& d) { return 14 * d.R + 3 * d.W + d.V + 2 * d.D + MMG_BLOCK; }

// Receiver (model.py:303-477): one workgroup per sample, reverse time from t = T - 1.  Seeds at every step come from the upstream
// gradients (dls = dps ps (1 - ps), dlw = dpw pw (1 - pw) or dw, dA_t from dy_t); backprop through time over the GRU state.
// Writes the per-row deltas the weight-gradient jobs reduce (vdgi, vdgh, vdgpre, vdlw, vdls, vdA, vdys) and the recomputed
// operands (vA, vg, vdbar).
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_rec(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, B = dm.B, D = dm.D, W = dm.W, R = dm.R, V = dm.V, T = dm.T;
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
    for (int i = tid; i < R; i += MMG_BLOCK) s_car[i] = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        const bool live = t < in.n;
        __syncthreads();
        for (int i = tid; i < R; i += MMG_BLOCK) { s_h0[i] = tp.h[row * R + i]; s_h1[i] = tp.h[row * R + (size_t)B * R + i]; }
        for (int j = tid; j < W; j += MMG_BLOCK) { s_z[j] = tp.z[row * W + j]; s_pw[j] = bin ? tp.pw[row * W + j] : 0.f; }
        for (int d = tid; d < D; d += MMG_BLOCK) {
            s_p[d] = tp.y[row * D + d];
            s_dy[d] = (live && in.dy) ? in.dy[row * D + d] : 0.f;
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
        if (tid == 0) tp.vdys[row] = dys;
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
            if (live && in.dw) {
                const float gw = in.dw[row * W + j];
                dl = bin ? gw * s_pw[j] * (1.f - s_pw[j]) : gw;
            }
            s_dlw[j] = dl;
            tp.vdlw[row * W + j] = dl;
        }
        float dls = 0.f;
        if (live && in.dps) { const float ps = tp.ps[row]; dls = in.dps[row] * ps * (1.f - ps); }
        if (tid == 0) tp.vdls[row] = dls;
        __syncthreads();
        for (int i = tid; i < R; i += MMG_BLOCK) {
            float dg = 0.f;
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
}

// Class side of the receiver: dC[d, r] = w2[r] sum_{t < n, b} dy_t[b, d] 1[A_t[b, r] + Cd[d, r] > 0] (-> y1.weight[:, R:], y1.bias)
// and Py2[d, r] = sum_{t < n, b} dy_t[b, d] relu(A_t[b, r] + Cd[d, r]) (-> y2.weight).  One workgroup per class.
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

// Sender (model.py:144-238): one workgroup per sample.  dlz = dpz pz (1 - pz) (binary) or dz (continuous logits), dpre =
// (W_b^T dlz)(1 - a^2), dhx = sum_t dpre, and at t = 0 the code_bias path W_c^T dpre_0 (model.py:196-200).
__global__ __launch_bounds__(MMG_BLOCK) void k_vjp_sen(Dims dm, Params P, Tape tp, VjpIn in) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, B = dm.B, H = dm.H, W = dm.W, T = dm.T, tid = threadIdx.x;
    float* s_hx = smem;  float* s_a = s_hx + H;  float* s_dpre = s_a + H;  float* s_dhx = s_dpre + H;
    float* s_c = s_dhx + H;  float* s_dlz = s_c + W;
    const float *Wc = P.p[S_CODE_W], *bc = P.p[S_CODE_B], *cb = P.p[S_CODE_BIAS], *Wb = P.p[S_BIN_W];
    const bool bin = dm.use_binary;
    if (b == 0)
        for (int j = tid; j < W; j += MMG_BLOCK) { const float s = sigmoidf_(cb[j]); tp.vdsig[j] = s * (1.f - s); }
    for (int h = tid; h < H; h += MMG_BLOCK) { s_hx[h] = tp.hx[(size_t)b * H + h]; s_dhx[h] = 0.f; }
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)t * B + b;
        const bool live = t < in.n;
        __syncthreads();
        for (int j = tid; j < W; j += MMG_BLOCK) {
            const float c = (t == 0) ? sigmoidf_(cb[j]) : tp.w[(row - B) * W + j];    // the receiver's previous message
            s_c[j] = c;
            tp.vc[row * W + j] = c;
            float dl = 0.f;
            if (live && in.dz) {
                const float g = in.dz[row * W + j];
                if (bin) { const float p = tp.pz[row * W + j]; dl = g * p * (1.f - p); } else dl = g;
            }
            s_dlz[j] = dl;
            tp.vdlz[row * W + j] = dl;
        }
        __syncthreads();
        for (int h = tid; h < H; h += MMG_BLOCK) {
            float pre = s_hx[h] + bc[h];
            for (int j = 0; j < W; ++j) pre = fmaf(Wc[(size_t)h * W + j], s_c[j], pre);
            const float a = tanhf(pre);
            s_a[h] = a;
            tp.va[row * H + h] = a;
            float da = 0.f;
            for (int j = 0; j < W; ++j) da = fmaf(Wb[(size_t)j * H + h], s_dlz[j], da);
            const float dp = da * (1.f - a * a);
            s_dpre[h] = dp;
            tp.vdpre[row * H + h] = dp;
            s_dhx[h] += dp;
        }
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
    const float* W1 = P.p[rec ? BR_L1_W : BS_L1_W];
    const float* b1 = P.p[rec ? BR_L1_B : BS_L1_B];
    float* hid = rec ? tp.vhid_r : tp.vhid_s;
    for (int k = threadIdx.x; k < K; k += MMG_BLOCK) {
        float acc = b1[k];
        for (int i = 0; i < nin; ++i) acc = fmaf(W1[(size_t)k * nin + i], smem[i], acc);
        hid[(size_t)row * K + k] = fmaxf(acc, 0.f);
    }
    if (threadIdx.x == 0) {
        const float* up = rec ? in.dbr : in.dbs;
        (rec ? tp.vdbr : tp.vdbs)[row] = (t < in.n && up) ? up[row] : 0.f;
    }
}

}  // namespace mmg
