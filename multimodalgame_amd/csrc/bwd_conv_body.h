// bwd_conv_body.h -- the text of k_bwd_conv.  NOT a header of its own: kernels_bwd.h includes it twice, with MMG_BWD_ATTN 0 for
// k_bwd_conv<MANY, VAR> -- token for token the kernel every plain handle has always run, so its instantiations keep their symbols, arguments
// and code -- and with MMG_BWD_ATTN 1 for k_bwd_conv_attn, the instantiation of an attention handle.  With dpre[d, :] = dy[d] w_y2 1[pre[d] > 0]
// at t* and dgpre at every t < t* (softmax(y) inside dbar is detached, alpha is not: model.py:441-449):
//   dalpha[j] = E[j] . dpre[class j]  (t = t*)   +   softmax(y)[class j] (G[j] . dgpre)  (t < t*)
//   dscore    = alpha * (dalpha - sum over the segment of alpha dalpha)
//   u[j, a]   = dscore[j] v[a] (1 - tanh^2(DD[j, a] + dh[a]));  ddh = sum_j u;  dh_z += d_h.weight^T ddh
// The tapes dscore / attn_ddh / attn_dv feed k_attn_dDD and k_wgrad's jobs; pre[d] is recomputed from alpha and E (nothing per sample x class x unit
// is stored).
#if MMG_BWD_ATTN
__global__ __launch_bounds__(MMG_BLOCK, 1) void k_bwd_conv_attn(Dims dm, Params P, Tape tp, const int64_t* __restrict__ target, AttnArgs at) {
    constexpr bool MANY = false;
    constexpr int VAR = 0;
#else
template <bool MANY, int VAR = 0>
__global__ __launch_bounds__(MMG_BLOCK, MANY ? (VAR ? 3 : 4) : 1) void k_bwd_conv(Dims dm, Params P, Tape tp, const int64_t* __restrict__ target) {
#endif
    constexpr int TU = MANY ? 2 : 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int B = dm.B, H = dm.H, W = dm.W, R = dm.R, V = dm.V, D = dm.D, T = dm.T;
    auto p4 = [](int n) { return (n + 3) & ~3; };
    float* p = smem;
    LossCoef lc; lc.cw = p; p += 3 * T; lc.ce = p; p += 3 * T; lc.cb = p; p += T;
    p = smem + ((7 * T + 3) & ~3);
    float* s_dhx = p; p += p4(H);   float* s_da = p; p += p4(H);   float* s_dpre = p; p += p4(H);
    float* s_dlz = p; p += p4(W);   float* s_dlw = p; p += p4(W);  float* s_dc0 = p; p += p4(W);
    float* s_dh = p; p += p4(R);    float* s_dhn = p; p += p4(R);  float* s_dg = p; p += p4(R);
    float* s_A = p; p += p4(R);     float* s_dA = p; p += p4(R);   float* s_hs = p; p += p4(R);
    float* s_dgi = p; p += p4(3 * R); float* s_dgh = p; p += p4(3 * R);
    float* s_dy = p; p += p4(D);
    float* s_red = p; p += 4 * MMG_BLOCK;
    float* s_misc = p;
    float* s_hw = s_misc + 32;                                    // SV_PROD only (bwd_smem_floats(d, true)): h_w of the step, recomputed
#if MMG_BWD_ATTN
    // (bwd_attn_smem_floats) alpha of the step | dalpha, then dscore | d_h(h) of the step | ddh | softmax(y) of the step
    float* s_al = s_misc + 32;
    float* s_ds = s_al + p4(at.NW);
    float* s_dhv = s_ds + p4(at.NW);
    float* s_ddh = s_dhv + p4(at.A);
    float* s_pi = s_ddh + p4(at.A);
#endif
    constexpr bool prod = VAR == SV_PROD, no_code = (VAR & SV_IGNORE_CODE) != 0;

    loss_coefficients(dm, tp.stats, lc, nullptr, nullptr);        // logged losses: spare block of k_wgrad

    const bool binary = dm.use_binary != 0;
    const int tstar = tp.tstar[b];
    const float L = tp.logs[b];
    const float* cw_s = lc.cw, *cw_r = lc.cw + T, *cw_z = lc.cw + 2 * T;
    const float* ce_s = lc.ce, *ce_r = lc.ce + T, *ce_z = lc.ce + 2 * T;

    for (int i = tid; i < R; i += nt) s_dh[i] = 0.f;
    for (int i = tid; i < H; i += nt) s_dhx[i] = 0.f;
    __syncthreads();

    // ---------------- zero the gradient tapes of steps this sample never took ----------------
    for (int t = tstar + 1; t < T; ++t) {
        const size_t row = (size_t)t * B + b;
        for (int i = tid; i < W; i += nt) { tp.dlz[row * W + i] = 0.f; tp.dlw[row * W + i] = 0.f; }
        for (int i = tid; i < H; i += nt) tp.dpre[row * H + i] = 0.f;
        for (int i = tid; i < R; i += nt) tp.dgpre[row * R + i] = 0.f;
        for (int i = tid; i < 3 * R; i += nt) { tp.dgi[row * 3 * R + i] = 0.f; tp.dgh[row * 3 * R + i] = 0.f; }
        if (tid == 0) { tp.dls[row] = 0.f; tp.dbs[row] = 0.f; tp.dbr[row] = 0.f; }
#if MMG_BWD_ATTN
        for (int a = tid; a < at.A; a += nt) { at.tp.attn_ddh[row * at.A + a] = 0.f; at.tp.attn_dv[row * at.A + a] = 0.f; }
#endif
    }

    // ---------------- reverse time ----------------
    for (int t = tstar; t >= 0; --t) {
        const size_t row = (size_t)t * B + b;
        const float* hn = tp.h + ((size_t)(t + 1) * B + b) * R;    // h after step t
        const float* hp = tp.h + ((size_t)t * B + b) * R;          // h before step t

        // ---- receiver message head (stream 1: active while m_{t+1} == 1) ----
        const bool act_next = binary && (t < tstar);
        if (act_next) {
            const float wh = (L - tp.br[row]) * cw_r[t];
            for (int j = tid; j < W; j += nt) {
                const float v = bit_seed(tp.w[row * W + j], tp.pw[row * W + j], wh, ce_r[t]);
                s_dlw[j] = v; tp.dlw[row * W + j] = v;
            }
            __syncthreads();
            gemv_t<TU>(P.p[R_W_W], R, W, R, s_dlw, s_dg, s_red, false);            // dg = W_w^T dlw
            for (int i = tid; i < R; i += nt) {
                const float g = tp.g[row * R + i];
                const float v = s_dg[i] * (1.f - g * g);
                s_dg[i] = v; tp.dgpre[row * R + i] = v;
            }
            __syncthreads();
            gemv_t<TU>(P.p[R_WH_W], R, R, R, s_dg, s_dh, s_red, true);             // dh += W_h^T dgpre
        } else {
            for (int j = tid; j < W; j += nt) tp.dlw[row * W + j] = 0.f;
            for (int i = tid; i < R; i += nt) tp.dgpre[row * R + i] = 0.f;
        }
        // ---- stop head (stream 0, Adaptive only) ----
        if (binary && !dm.fixed) {
            const float wh = (L - tp.br[row]) * cw_s[t];
            const float dls = bit_seed(tp.s[row], tp.ps[row], wh, ce_s[t]);
            if (tid == 0) tp.dls[row] = dls;
            const float* ws = P.p[R_S_W];
            for (int i = tid; i < R; i += nt) s_dh[i] += ws[i] * dls;
        } else if (tid == 0) {
            tp.dls[row] = 0.f;
        }
        __syncthreads();
        // ---- class logits at the output step (NLL, model.py:1271) ----
        if (t == tstar) {
            const int tgt = (int)target[b];
            float dsum = 0.f;
            for (int d = tid; d < D; d += nt) {
                const float v = (tp.sm[(size_t)b * D + d] - (d == tgt ? 1.f : 0.f)) / (float)dm.Bg;
                s_dy[d] = v; tp.dy[(size_t)b * D + d] = v; dsum += v;
            }
            dsum = block_sum(dsum, s_misc);
            if (tid == 0) tp.dysum[b] = dsum;
#if MMG_BWD_ATTN
            // softmax(outp) as the forward pass left it (expf of the log-softmax) sums to 1 + O(1e-7), so sum_d dy is that over B, not 0 -- and with
            // attention many y1 units are on for EVERY class (the description moves pre[d] far less than the state does), where dA = w_y2 sum_d dy
            // vanishes exactly: their y1.bias gradient would be that residue, which RMSprop's first step turns into 1e-4.  Renormalised to first order,
            // sm / sum sm:  dy[d] -= sm[d] dsum.  (A thread corrects the entries it wrote.)
            for (int d = tid; d < D; d += nt) { const float v = s_dy[d] - tp.sm[(size_t)b * D + d] * dsum; s_dy[d] = v; tp.dy[(size_t)b * D + d] = v; }
#endif
            for (int i = tid; i < R; i += nt) { const float v = hn[i]; s_hs[i] = v; tp.hstar[(size_t)b * R + i] = v; }
            __syncthreads();
#if MMG_BWD_ATTN
            gemv_rows<4>(P.p[R_Y1_W] + V, R + V, R, R, s_hs, [&](int n, float acc) { s_A[n] = acc; });      // h is the SECOND column block (model.py:409-410)
#else
            gemv_rows<(MANY ? 2 : 4)>(P.p[R_Y1_W], R + V, R, R, s_hs, [&](int n, float acc) { s_A[n] = acc; });
#endif
            __syncthreads();
            const float* w2 = P.p[R_Y2_W];
#if MMG_BWD_ATTN
            {
                // a wave per class: pre[d] again from alpha and E, dpre[d] in registers (a lane owns units lane, lane + 64, ...: R <= 256),
                // dalpha[j] = E[j] . dpre[d] for the words of d; dA = w_y2 sum_{d on} dy[d], the sum in float64: sum_d dy[d] = 0, so a unit that is on for
                // every class -- the description moves pre[d] far less than the state does -- has dA = 0 up to what the summation leaves, and dA feeds
                // y1.bias (whose first RMSprop step magnifies an error of 1e-8 to 1e-4) and the BPTT; the waves' partials meet in s_red, 128 units at a time
                const int NW = at.NW, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
                const int* seg = at.tp.attn_seg;
                const float* E = at.tp.attn_E; const float* b1 = P.p[R_Y1_B];
                const float* al = at.tp.alpha + row * NW;
                for (int j = tid; j < NW; j += nt) s_al[j] = al[j];
                __syncthreads();
                double dAp[4] = {0., 0., 0., 0.};
                for (int d = wave; d < D; d += nw) {
                    const int j0 = seg[d], j1 = seg[d + 1];
                    const float dyd = s_dy[d];
                    float dp[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = lane + 64 * k;
                        dp[k] = 0.f;
                        if (r < R) {
                            float pre = s_A[r] + b1[r];
                            for (int j = j0; j < j1; ++j) pre = fmaf(s_al[j], E[(size_t)j * R + r], pre);
                            dp[k] = pre > 0.f ? dyd * w2[r] : 0.f;
                            dAp[k] += pre > 0.f ? (double)dyd : 0.;
                        }
                    }
                    for (int j = j0; j < j1; ++j) {
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const int r = lane + 64 * k; if (r < R) acc = fmaf(E[(size_t)j * R + r], dp[k], acc); }
                        acc = wave_sum(acc);
                        if (lane == 0) s_ds[j] = acc;
                    }
                }
                double* s_redd = reinterpret_cast<double*>(s_red);      // 4 * MMG_BLOCK floats = nw waves x 128 doubles
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    __syncthreads();
#pragma unroll
                    for (int k = 2 * half; k < 2 * half + 2; ++k) s_redd[wave * 128 + lane + 64 * (k - 2 * half)] = dAp[k];
                    __syncthreads();
                    const int i = 128 * half + tid;
                    if (tid < 128 && i < R) {
                        double v = 0.;
                        for (int w = 0; w < nw; ++w) v += s_redd[w * 128 + tid];
                        const float va = (float)v * w2[i];
                        s_dA[i] = va; tp.dA[(size_t)b * R + i] = va; tp.Astar[(size_t)b * R + i] = s_A[i];
                    }
                }
            }
#else
            for (int i = tid; i < R; i += nt) {
                const float a = s_A[i];
                float acc = 0.f;
                for (int d = 0; d < D; d += 8) {                               // 8 class rows of Cd in flight, same add order
                    float cv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) cv[u] = tp.Cd[(size_t)min(d + u, D - 1) * R + i];
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += (d + u < D && a + cv[u] > 0.f) ? s_dy[min(d + u, D - 1)] : 0.f;
                }
                const float v = acc * w2[i];
                s_dA[i] = v; tp.dA[(size_t)b * R + i] = v; tp.Astar[(size_t)b * R + i] = a;
            }
#endif
            __syncthreads();
#if MMG_BWD_ATTN
            gemv_t<TU>(P.p[R_Y1_W] + V, R + V, R, R, s_dA, s_dh, s_red, true);     // dh += W_y1h^T dA
#else
            gemv_t<TU>(P.p[R_Y1_W], R + V, R, R, s_dA, s_dh, s_red, true);         // dh += W_y1h^T dA
#endif
        }
#if MMG_BWD_ATTN
        {
            const int NW = at.NW, A = at.A, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
            const int* seg = at.tp.attn_seg;
            if (t == tstar || act_next) {
                if (t != tstar) {
                    const float* al = at.tp.alpha + row * NW;
                    for (int j = tid; j < NW; j += nt) { s_al[j] = al[j]; s_ds[j] = 0.f; }
                }
                for (int a = tid; a < A; a += nt) s_dhv[a] = at.tp.attn_dh[row * A + a];
                if (act_next) {
                    // the query path: dlw -> g -> w_d -> dbar -> alpha; softmax(y) is a constant there (model.py:441)
                    float mx = -3.4e38f;
                    for (int d = tid; d < D; d += nt) mx = fmaxf(mx, tp.y[row * D + d]);
                    mx = block_max(mx, s_misc + 8);
                    float se = 0.f;
                    for (int d = tid; d < D; d += nt) { const float e = expf(tp.y[row * D + d] - mx); s_pi[d] = e; se += e; }
                    se = block_sum(se, s_misc + 16);
                    const float inv = 1.f / se;
                    const float* Gt = at.tp.attn_G; const int* cls = at.tp.attn_cls;
                    const int grp = tid >> 4, gl = tid & 15, ngrp = nt >> 4;
                    for (int j0 = 0; j0 < NW; j0 += ngrp) {          // 16 lanes per word (uniform trip count for the DPP sum)
                        const int j = min(j0 + grp, NW - 1);
                        float acc = 0.f;
                        for (int r = gl; r < R; r += 16) acc = fmaf(Gt[(size_t)j * R + r], s_dg[r], acc);
                        acc = dpp_group_sum<16>(acc);
                        if (gl == 0 && j0 + grp < NW) s_ds[j] += s_pi[cls[j]] * inv * acc;
                    }
                }
                __syncthreads();
                // dscore = alpha (dalpha - sum over the segment of alpha dalpha): a wave per class
                for (int d = wave; d < D; d += nw) {
                    const int j0 = seg[d], j1 = seg[d + 1];
                    float sm = 0.f;
                    for (int j = j0 + lane; j < j1; j += 64) sm = fmaf(s_al[j], s_ds[j], sm);
                    sm = wave_sum(sm);
                    for (int j = j0 + lane; j < j1; j += 64) { const float v = s_al[j] * (s_ds[j] - sm); s_ds[j] = v; at.tp.dscore[row * NW + j] = v; }
                }
                __syncthreads();
                {   // ddh = sum_j u[j, :], dv = sum_j dscore[j] tanh(DD[j] + dh): `parts` word slices per unit, added in slice order
                    const float* DDt = at.tp.attn_DD; const float* va = at.P.p[A_DA_W];
                    const int parts = nt / A, part = tid / A, a = tid - part * A;
                    if (part < parts) {
                        float u = 0.f, dv = 0.f;
                        const float dha = s_dhv[a];
                        for (int j = part; j < NW; j += parts) {
                            const float th = tanhf(DDt[(size_t)j * A + a] + dha), ds = s_ds[j];
                            u = fmaf(ds, 1.f - th * th, u); dv = fmaf(ds, th, dv);
                        }
                        s_red[part * A + a] = u * va[a]; s_red[2 * MMG_BLOCK + part * A + a] = dv;
                    }
                    __syncthreads();
                    if (tid < A) {
                        float u = 0.f, dv = 0.f;
                        for (int q = 0; q < parts; ++q) { u += s_red[q * A + tid]; dv += s_red[2 * MMG_BLOCK + q * A + tid]; }
                        s_ddh[tid] = u; at.tp.attn_ddh[row * A + tid] = u; at.tp.attn_dv[row * A + tid] = dv;
                    }
                    __syncthreads();
                }
                gemv_t<TU>(at.P.p[A_DH_W], R, A, R, s_ddh, s_dh, s_red, true);    // dh += d_h.weight^T ddh, beside W_y1h^T dA and W_h^T dgpre
            } else {
                for (int j = tid; j < NW; j += nt) at.tp.dscore[row * NW + j] = 0.f;
                for (int a = tid; a < A; a += nt) { at.tp.attn_ddh[row * A + a] = 0.f; at.tp.attn_dv[row * A + a] = 0.f; }
            }
        }
#endif
        // ---- GRU cell backward ----
        {
            const float* gr = tp.gru + row * 4 * R;
            for (int i = tid; i < R; i += nt) {
                const float rr = gr[i], uu = gr[R + i], nn = gr[2 * R + i], ghn = gr[3 * R + i];
                const float dh = s_dh[i];
                const float dn = dh * (1.f - uu), du = dh * (hp[i] - nn);
                const float dnp = dn * (1.f - nn * nn), dup = du * uu * (1.f - uu);
                const float drp = dnp * ghn * rr * (1.f - rr);
                s_dgi[i] = drp; s_dgi[R + i] = dup; s_dgi[2 * R + i] = dnp;
                s_dgh[i] = drp; s_dgh[R + i] = dup; s_dgh[2 * R + i] = dnp * rr;
                s_dhn[i] = dh * uu;
            }
            __syncthreads();
            for (int i = tid; i < 3 * R; i += nt) { tp.dgi[row * 3 * R + i] = s_dgi[i]; tp.dgh[row * 3 * R + i] = s_dgh[i]; }
            gemv_t<TU>(P.p[R_WHH], R, 3 * R, R, s_dgh, s_dhn, s_red, true);        // dh_{t-1} += W_hh^T dgh
            for (int i = tid; i < R; i += nt) s_dh[i] = s_dhn[i];
            __syncthreads();
        }
        // ---- sender (stream 2) ----
        if (binary) {
            const float wh = (L - tp.bs[row]) * cw_z[t];
            for (int j = tid; j < W; j += nt) {
                const float v = bit_seed(tp.z[row * W + j], tp.pz[row * W + j], wh, ce_z[t]);
                s_dlz[j] = v; tp.dlz[row * W + j] = v;
                if (VAR && prod && t > 0) s_dc0[j] = tp.c[row * W + j];        // the step's code input (s_dc0 is free until t = 0)
            }
            __syncthreads();
            // VAR: h_w = W_c c_t + b_c again (t = 0: tp.hw0), beside the product below -- no barrier of its own: gemv_t ends with one
            if (VAR && prod && t > 0) gemv_rows<(MANY ? 2 : 4)>(P.p[S_CODE_W], W, H, W, s_dc0, [&](int n, float acc) { s_hw[n] = acc; });
            gemv_t<TU>(P.p[S_BIN_W], H, W, H, s_dlz, s_da, s_red, false);          // da = W_b^T dlz
            for (int i = tid; i < H; i += nt) {
                const float a = tp.a[row * H + i];
                const float v = s_da[i] * (1.f - a * a);
                if (VAR && prod) {                                             // a = tanh(h_x * h_w), model.py:217-218
                    const float hw = (t == 0) ? tp.hw0[i] : s_hw[i] + P.p[S_CODE_B][i];
                    const float dhw = v * tp.hx[(size_t)b * H + i];
                    s_dpre[i] = dhw; tp.dpre[row * H + i] = dhw; s_dhx[i] += v * hw;
                } else if (VAR && no_code) {                                   // a = tanh(h_x), model.py:208-210: nothing reaches code_layer / code_bias
                    s_dpre[i] = 0.f; tp.dpre[row * H + i] = 0.f; s_dhx[i] += v;
                } else {
                    s_dpre[i] = v; tp.dpre[row * H + i] = v; s_dhx[i] += v;
                }
            }
            __syncthreads();
            if (t == 0) {                                                      // code_bias path (model.py:199)
                gemv_t<TU>(P.p[S_CODE_W], W, H, W, s_dpre, s_dc0, s_red, false);
                for (int j = tid; j < W; j += nt) tp.dc0[(size_t)b * W + j] = s_dc0[j];
            }
            // ---- baselines (MSE, model.py:971-988) ----
            const float dbs = lc.cb[t] * (tp.bs[row] - L), dbr = lc.cb[t] * (tp.br[row] - L);
            // d hidden = dbeta * w2 * 1[hidden > 0] is formed on the fly by k_wgrad (virtual operand)
            if (tid == 0) { tp.dbs[row] = dbs; tp.dbr[row] = dbr; }
        } else {
            for (int i = tid; i < W; i += nt) tp.dlz[row * W + i] = 0.f;
            for (int i = tid; i < H; i += nt) tp.dpre[row * H + i] = 0.f;
            if (tid == 0) { tp.dbs[row] = 0.f; tp.dbr[row] = 0.f; }
        }
        __syncthreads();
    }
    for (int i = tid; i < H; i += nt) tp.dhx[(size_t)b * H + i] = s_dhx[i];
    if (!binary) for (int j = tid; j < W; j += nt) tp.dc0[(size_t)b * W + j] = 0.f;
}
