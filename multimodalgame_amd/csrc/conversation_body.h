// conversation_body.h -- the text of k_conversation.  NOT a header of its own: kernels_fwd.h includes it four times, with MMG_CONV_ATTN 0 for
// k_conversation<NT, FLIP, VAR, RELAX> -- token for token the kernel every plain handle has always run, so its instantiations keep their symbols,
// arguments and code -- and with MMG_CONV_ATTN 1 for k_conversation_attn<NT>, the instantiation of an attention handle (mmg_attn_create;
// model.py:344-410, 444-445): the receiver attends over the words of every description with its GRU state as the query.  `at` carries the
// extra parameters, the description set and the per-word tables k_attn_prep formed (DD, E).  Per step, behind the GRU update:
//   dh = d_h(h);  score[j] = d_attn(tanh(DD[j] + dh));  alpha = softmax of score inside each class's segment
//   pre[d] = y1.weight[:, V:] h + b_y1 + sum_{j in d} alpha[j] E[j]   -- the attention branch puts the description FIRST (model.py:409-410)
//   dbar = sum_j softmax(y)[class j] alpha[j] set[j]                  -- model.py:441-449 over the weighted descriptions
// Nothing per (sample, class, V) or per (sample, word, V) is formed: everything behind alpha is linear in the set.
// A third inclusion, with MMG_CONV_VATTN 1, is k_conversation_vattn<NT>, the instantiation of a visual-attention handle (mmg_vattn_create;
// model.py:114-142, 168-195): the SENDER attends over the N locations of the feature map x [B, C, N] (channel-major, read in place) with
// the receiver's last message as the query.  `va` carries the extra parameters and what k_vattn_prep formed per conversation (HX, HG).
// Per step, in front of the tanh site:
//   t == 0: alpha = 1 / N;   t >= 1: q = attn_W_w(w);  beta[i] = attn_U(tanh(q + HX[i] + HG));  alpha = softmax_i beta
//   x_attn = sum_i alpha[i] x[:, i];   h_x = image_layer(x_attn)        -- h_x is per STEP here (tape: vattn_hx), tape.hx is not read
// A fourth inclusion, with MMG_CONV_NOISE 1, is k_conversation_noise<NT>, the instantiation of a continuous handle with Gaussian message noise
// (mmg_set_message_noise): noise_msg at both message sites of the continuous branch, in front of corrupt_msg.  A kernel of its own name, so
// that k_conversation<NT, FLIP, VAR, RELAX> keeps its symbols as well as its code.
#if MMG_CONV_VATTN
template <int NT>
__global__ __launch_bounds__(NT) void k_conversation_vattn(Dims dm, Params P, Tape tp, ConvArgs ar, VattnArgs va) {
    constexpr bool FLIP = false, VAR = false, RELAX = false, NOISE = false;
#elif MMG_CONV_ATTN
template <int NT>
__global__ __launch_bounds__(NT) void k_conversation_attn(Dims dm, Params P, Tape tp, ConvArgs ar, AttnArgs at) {
    constexpr bool FLIP = false, VAR = false, RELAX = false, NOISE = false;
#elif MMG_CONV_NOISE
template <int NT>
__global__ __launch_bounds__(NT) void k_conversation_noise(Dims dm, Params P, Tape tp, ConvArgs ar) {
    constexpr bool FLIP = false, VAR = false, RELAX = false, NOISE = true;
#else
template <int NT, bool FLIP = false, bool VAR = false, bool RELAX = false>
__global__ __launch_bounds__(NT) void k_conversation(Dims dm, Params P, Tape tp, ConvArgs ar) {
    constexpr bool NOISE = false;
#endif
    constexpr int GU = NT == 512 ? 8 : 4;               // row passes per load batch of gemv_rows
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int B = dm.B, H = dm.H, W = dm.W, R = dm.R, V = dm.V, D = dm.D, T = dm.T;
    ConvSmem s;
    {
        float* p = smem;
        s.hx = p; p += pad4(H);  s.a = p; p += pad4(H);
        s.c = p; p += pad4(W);   s.z = p; p += pad4(W);  s.w = p; p += pad4(W);
        s.lp = p; p += pad4(W);  s.ne = p; p += pad4(W);
        s.h = p; p += pad4(R);   s.hn = p; p += pad4(R); s.A = p; p += pad4(R);
        s.g = p; p += pad4(R);   s.g2 = p; p += pad4(R);
        s.gi = p; p += pad4(3 * R); s.gh = p; p += pad4(3 * R);
        s.y = p; p += pad4(D);   s.yout = p; p += pad4(D);
        s.dbar = p; p += pad4(V);
        s.red = p; p += 4 * NT;
        s.misc = p;
    }
    float* s_ne = s.ne;
#if MMG_CONV_ATTN
    // (conv_attn_smem_floats) the step's attention weights | softmax(y)[class j] alpha[j] | d_h(h)
    float* s_alpha = s.misc + 32;
    float* s_coef = s_alpha + pad4(at.NW);
    float* s_dhv = s_coef + pad4(at.NW);
#endif
#if MMG_CONV_VATTN
    // (conv_vattn_smem_floats) the step's scores / attention weights | q + HG | x_attn
    float* s_val = s.misc + 32;
    float* s_vq = s_val + pad4(va.N);
    float* s_vxa = s_vq + pad4(va.A);
#endif

    const bool do_sen = ar.phases & 1, do_rec = ar.phases & 2;
    const bool binary = dm.use_binary != 0;
    const bool train = ar.train != 0;

    // ---- conversation state ----
#if !MMG_CONV_VATTN
    if (do_sen) for (int i = tid; i < H; i += nt) s.hx[i] = tp.hx[(size_t)b * H + i];
#endif
    if (do_rec) {
        for (int i = tid; i < R; i += nt)
            s.h[i] = ar.h_state ? ar.h_state[(size_t)b * R + i] : (ar.t_begin == 0 ? 0.f : tp.h[((size_t)ar.t_begin * B + b) * R + i]);
        if (ar.t_begin == 0 && !ar.h_state) for (int i = tid; i < R; i += nt) tp.h[(size_t)b * R + i] = 0.f;
    }
    for (int j = tid; j < W; j += nt) {
        float wv = dm.first_rec;                                   // model.py:786
        if (ar.t_begin > 0) wv = ar.w_in ? ar.w_in[(size_t)b * W + j] : tp.w[((size_t)(ar.t_begin - 1) * B + b) * W + j];
        s.w[j] = wv;
    }
    if (tid == 0) {
        s.misc[0] = 1.f;                                           // running stop mask m_t
        s.misc[1] = -1.f;                                          // t* (not yet known)
        s.misc[2] = (ar.sprod_state && !ar.sprod_first) ? ar.sprod_state[b] : 1.f;   // running prod of p_s
        if (ar.t_begin == 0 && do_rec) tp.mask[b] = 1;             // stop_mask[0] = ones   model.py:775
    }
    __syncthreads();

    const uint32_t mb_counter = tp.counter[0];
    const uint32_t gb = (uint32_t)(dm.boff + b);                   // index inside the GLOBAL minibatch

    int t = ar.t_begin;
    for (; t < ar.t_end; ++t) {
        const size_t row = (size_t)t * B + b;
        // ================= Sender (model.py:193-238) =================
        if (do_sen) {
            // code input: sigmoid(code_bias) at t == 0 (hw0 precomputed), else the receiver's last message
            for (int j = tid; j < W; j += nt) {
                const float cv = s.w[j];
                s.c[j] = cv;
                tp.zr[row * W + j] = cv;                           // z_r fed to baseline_sen (model.py:836)
                tp.c[row * W + j] = (t == 0) ? sigmoidf_(P.p[S_CODE_BIAS][j]) : cv;
            }
            __syncthreads();
#if MMG_CONV_VATTN
            {
                const int A = va.A, N = va.N, C = dm.F;
                const float* xb = ar.x + (size_t)b * C * N;                // x[b, c, i]: locations contiguous (model.py:171-172 transposes a VIEW)
                if (t == 0) {
                    for (int i = tid; i < N; i += nt) s_val[i] = va.inv_n;  // model.py:177-180 (attention_func's scores are computed and dropped)
                } else {
                    gemv_rows<GU>(va.P.p[VA_WW_W], W, A, W, s.c, [&](int n, float acc) { s_vq[n] = acc; });
                    __syncthreads();
                    {
                        const float* bw = va.P.p[VA_WW_B];
                        const float* hg = va.tp.vattn_HG + (size_t)b * A;
                        for (int a = tid; a < A; a += nt) s_vq[a] += bw[a];
                        __syncthreads();
                        // beta[i] = attn_U(tanh((q + HX[i]) + HG)) (model.py:136-140): 16 lanes per location
                        const float* ua = va.P.p[VA_U_W];
                        const float cu = va.P.p[VA_U_B][0];
                        const bool ctx = va.G > 0;
                        const int grp = tid >> 4, gl = tid & 15, ngrp = nt >> 4;
                        for (int i0 = 0; i0 < N; i0 += ngrp) {              // (uniform trip count: every lane takes part in the DPP sum)
                            const int i = min(i0 + grp, N - 1);
                            const float* hxr = va.tp.vattn_HX + ((size_t)b * N + i) * A;
                            float acc = 0.f;
                            for (int a = gl; a < A; a += 16) {
                                float pre = s_vq[a] + hxr[a];
                                if (ctx) pre += hg[a];
                                acc = fmaf(ua[a], tanhf(pre), acc);
                            }
                            acc = dpp_group_sum<16>(acc);
                            if (gl == 0 && i0 + grp < N) s_val[i] = acc + cu;
                        }
                    }
                    __syncthreads();
                    float mx = -3.4e38f;                                    // softmax over the locations (model.py:182-183)
                    for (int i = tid; i < N; i += nt) mx = fmaxf(mx, s_val[i]);
                    mx = block_max(mx, s.misc + 8);
                    float se = 0.f;
                    for (int i = tid; i < N; i += nt) { const float e = expf(s_val[i] - mx); s_val[i] = e; se += e; }
                    se = block_sum(se, s.misc + 16);
                    const float inv = 1.f / se;
                    for (int i = tid; i < N; i += nt) s_val[i] *= inv;
                }
                __syncthreads();
                for (int i = tid; i < N; i += nt) va.tp.vattn_alpha[row * N + i] = s_val[i];
                // x_attn[c] = sum_i alpha[i] x[c, i] (model.py:186): a row of x per channel
                gemv_rows<GU>(xb, N, C, N, s_val, [&](int n, float acc) { s_vxa[n] = acc; va.tp.vattn_xa[row * C + n] = acc; });
                __syncthreads();
                gemv_rows<GU>(P.p[S_IMG_W], C, H, C, s_vxa, [&](int n, float acc) { s.hx[n] = acc; });     // model.py:195
                __syncthreads();
                {
                    const float* bi = P.p[S_IMG_B];
                    for (int i = tid; i < H; i += nt) { const float v = s.hx[i] + bi[i]; s.hx[i] = v; va.tp.vattn_hx[row * H + i] = v; }
                }
                __syncthreads();
            }
#endif
            const bool no_code = VAR && (ar.sender_var & SV_IGNORE_CODE);     // model.py:208-210: h_w is not used (the reference computes and drops it)
            if (t > 0 && !no_code) {
                // (epilogues only park the sums in LDS: a bias / uniform load inside them would be one dependent
                //  global round trip per row pass, executed by a single lane of each group)
                gemv_rows<GU>(P.p[S_CODE_W], W, H, W, s.c, [&](int n, float acc) { s.a[n] = acc; });
                __syncthreads();
            }
            const float* bc = P.p[S_CODE_B];
            for (int i = tid; i < H; i += nt) {
                float av;
                if (VAR && no_code) {
                    av = tanhf(s.hx[i]);                           // model.py:208-210
                } else {
                    const float hw = (t == 0) ? tp.hw0[i] : s.a[i] + bc[i];
                    av = (VAR && (ar.sender_var & SV_PROD)) ? tanhf(s.hx[i] * hw)      // model.py:217-218
                                                            : tanhf(s.hx[i] + hw);     // model.py:216
                }
                s.a[i] = av;
                tp.a[row * H + i] = av;
            }
            __syncthreads();
            {
                const float* bb = P.p[S_BIN_B];
                const float* uz = ar.u_z ? ar.u_z + row * W : nullptr;
                gemv_rows<GU>(P.p[S_BIN_W], H, W, H, s.a, [&](int n, float acc) { s.z[n] = acc; });
                __syncthreads();
                for (int n = tid; n < W; n += nt) {
                    const float lz = s.z[n] + bb[n];
                    float zz = lz, lpv = 0.f, nev = 0.f;
                    if (binary) {
                        const float p = sigmoidf_(lz);             // model.py:223
                        if (train) {
                            const float u = uz ? uz[n] : philox_uniform(ar.seed, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, 0u);
                            zz = (u < p) ? 1.f : 0.f;              // model.py:227
                            if (RELAX) {                           // mmg_set_message_relaxation: the same draw as logistic noise
                                const float soft = relax_soft(lz, u, ar.relax_tau_z);
                                tp.zs[row * W + n] = soft;
                                if (!ar.relax_hard) zz = soft;
                            }
                        } else {
                            zz = rintf(p);                         // model.py:229 (torch.round = half-to-even)
                        }
                        if (FLIP) zz = flip_msg(ar, false, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, zz);   // model.py:233-234
                        tp.pz[row * W + n] = p;
                        const float l1 = logf(p + MMG_EPS), l0 = logf(1.f - p + MMG_EPS);
                        lpv = zz * l1 + (1.f - zz) * l0;           // model.py:908-910
                        nev = p * l1 + (1.f - p) * l0;             // model.py:919-922
                    }
                    if (NOISE && !binary) zz = noise_msg(ar, false, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, zz);   // the channel sits inside the agent: before the mask
                    zz = corrupt_msg(ar, n, zz);                   // model.py:813-820 (evaluation only)
                    s.z[n] = zz; s.lp[n] = lpv; s_ne[n] = nev;
                    tp.z[row * W + n] = zz;
                }
            }
            __syncthreads();
            if (binary) {
                float lpv = 0.f, nev = 0.f;
                for (int j = tid; j < W; j += nt) { lpv += s.lp[j]; nev += s_ne[j]; }
                lpv = block_sum(lpv, s.misc + 8);
                nev = block_sum(nev, s.misc + 16);
                if (tid == 0) { tp.lp_z[row] = lpv; tp.ne_z[row] = nev; }
            }
        } else {
            // receiver-only call: the message comes from the tape slot of this step
            for (int j = tid; j < W; j += nt) s.z[j] = tp.z[row * W + j];
            __syncthreads();
        }
        if (!do_rec) continue;

        // ================= Receiver (model.py:333-342, 411-477) =================
        {   // GRUCell (model.py:340); gate order r, z(u), n
            const float* bih = P.p[R_BIH]; const float* bhh = P.p[R_BHH];
            gemv_rows<GU>(P.p[R_WIH], W, 3 * R, W, s.z, [&](int n, float acc) { s.gi[n] = acc; });
            gemv_rows<GU>(P.p[R_WHH], R, 3 * R, R, s.h, [&](int n, float acc) { s.gh[n] = acc; });
            __syncthreads();
            for (int i = tid; i < 3 * R; i += nt) { s.gi[i] += bih[i]; s.gh[i] += bhh[i]; }
        }
        __syncthreads();
        for (int i = tid; i < R; i += nt) {
            const float rr = sigmoidf_(s.gi[i] + s.gh[i]);
            const float uu = sigmoidf_(s.gi[R + i] + s.gh[R + i]);
            const float ghn = s.gh[2 * R + i];
            const float nn = tanhf(s.gi[2 * R + i] + rr * ghn);
            const float hv = nn + uu * (s.h[i] - nn);
            s.hn[i] = hv;
            float* gr = tp.gru + row * 4 * R;
            gr[i] = rr; gr[R + i] = uu; gr[2 * R + i] = nn; gr[3 * R + i] = ghn;
            tp.h[((size_t)(t + 1) * B + b) * R + i] = hv;
        }
        __syncthreads();
        {   // stop head (model.py:414-427) and the h-half of y1 (Appendix A.2)
            const float bsv = P.p[R_S_B][0];
            gemv_rows<GU>(P.p[R_S_W], R, 1, R, s.hn, [&](int n, float acc) {
                const float p = sigmoidf_(acc + bsv);
                float sv;
                if (train) {
                    const float u = ar.u_s ? ar.u_s[row] : philox_uniform(ar.seed, (uint32_t)(t * dm.Bg + gb), mb_counter, 1u);
                    sv = (u < p) ? 1.f : 0.f;                      // model.py:420
                } else {
                    const float prod = dm.s_prob_prod ? s.misc[2] * p : p;   // model.py:423-426 (misc[2] == 1 on a fresh conversation)
                    s.misc[2] = prod;
                    sv = rintf(prod);                              // model.py:427
                }
                tp.s[row] = sv; tp.ps[row] = p;
                const float l1 = logf(p + MMG_EPS), l0 = logf(1.f - p + MMG_EPS);
                tp.lp_s[row] = sv * l1 + (1.f - sv) * l0;
                tp.ne_s[row] = p * l1 + (1.f - p) * l0;
                s.misc[3] = sv;
            });
#if MMG_CONV_ATTN
            gemv_rows<GU>(P.p[R_Y1_W] + V, R + V, R, R, s.hn, [&](int n, float acc) { s.A[n] = acc; });      // h is the SECOND column block (model.py:409-410)
            gemv_rows<GU>(at.P.p[A_DH_W], R, at.A, R, s.hn, [&](int n, float acc) { s_dhv[n] = acc; });
#else
            gemv_rows<GU>(P.p[R_Y1_W], R + V, R, R, s.hn, [&](int n, float acc) { s.A[n] = acc; });
#endif
        }
        __syncthreads();
#if MMG_CONV_ATTN
        {
            const int A = at.A, NW = at.NW;
            const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
            const int* seg = at.tp.attn_seg;
            {   // dh = d_h(h) (model.py:359)
                const float* bh = at.P.p[A_DH_B];
                for (int a = tid; a < A; a += nt) { const float v = s_dhv[a] + bh[a]; s_dhv[a] = v; at.tp.attn_dh[row * A + a] = v; }
            }
            __syncthreads();
            {   // score[j] = d_attn(tanh(DD[j] + dh)) (model.py:366): 16 lanes per word
                const float* va = at.P.p[A_DA_W];
                const float ca = at.P.p[A_DA_B][0];
                const int grp = tid >> 4, gl = tid & 15, ngrp = nt >> 4;
                for (int j0 = 0; j0 < NW; j0 += ngrp) {            // (uniform trip count: every lane takes part in the DPP sum)
                    const int j = min(j0 + grp, NW - 1);
                    const float* ddr = at.tp.attn_DD + (size_t)j * A;
                    float acc = 0.f;
                    for (int a = gl; a < A; a += 16) acc = fmaf(va[a], tanhf(ddr[a] + s_dhv[a]), acc);
                    acc = dpp_group_sum<16>(acc);
                    if (gl == 0 && j0 + grp < NW) s_alpha[j] = acc + ca;
                }
            }
            __syncthreads();
            // softmax inside each class's segment (model.py:370-380): a wave per class, a lane owns the same words in all three passes
            for (int d = wave; d < D; d += nw) {
                const int j0 = seg[d], j1 = seg[d + 1];
                float mx = -3.4e38f;
                for (int j = j0 + lane; j < j1; j += 64) mx = fmaxf(mx, s_alpha[j]);
                mx = wave_max(mx);
                float se = 0.f;
                for (int j = j0 + lane; j < j1; j += 64) { const float e = expf(s_alpha[j] - mx); s_alpha[j] = e; se += e; }
                se = wave_sum(se);
                const float inv = 1.f / se;
                for (int j = j0 + lane; j < j1; j += 64) { const float al = s_alpha[j] * inv; s_alpha[j] = al; at.tp.alpha[row * NW + j] = al; }
            }
            __syncthreads();
            {   // y[d] = y2(relu(y1([wdesc[d] || h]))), wdesc[d] = sum_{j in d} alpha[j] set[j] folded into E (model.py:383-410, 432-433)
                const float* w2 = P.p[R_Y2_W]; const float* b1 = P.p[R_Y1_B];
                const float b2 = P.p[R_Y2_B][0];
                const float* E = at.tp.attn_E;
                for (int d = wave; d < D; d += nw) {
                    const int j0 = seg[d], j1 = seg[d + 1];
                    float acc = 0.f;
                    for (int r = lane; r < R; r += 64) {
                        float pre = s.A[r] + b1[r];
                        for (int j = j0; j < j1; ++j) pre = fmaf(s_alpha[j], E[(size_t)j * R + r], pre);
                        acc = fmaf(w2[r], fmaxf(pre, 0.f), acc);
                    }
                    acc = wave_sum(acc);
                    if (lane == 0) { const float yv = acc + b2; s.y[d] = yv; tp.y[row * D + d] = yv; }
                }
            }
        }
#else
        {   // y[d] = b_y2 + sum_r w_y2[r] * relu(A[r] + Cd[d,r])      (model.py:432-433)
            const float* w2 = P.p[R_Y2_W];
            const float b2 = P.p[R_Y2_B][0];
            const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
            const bool vec = (R & 3) == 0;
            const int items = vec ? (R >> 2) : R;
            int G = 1; while (G < 64 && G < items) G <<= 1;
            const int rpw = 64 / G, sub = lane / G, gl = lane - sub * G;
            constexpr int U = 4;                                    // class passes loaded together (cf. gemv_rows)
            const int stride = nw * rpw;
            for (int d0 = wave * rpw + sub; d0 < D + sub; d0 += stride * U) {
                float acc[U];
                const float* crow[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { acc[u] = 0.f; crow[u] = tp.Cd + (size_t)min(d0 + u * stride, D - 1) * R; }
                if (vec) {
                    for (int k = gl; k < items; k += G) {
                        float4 cv[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) cv[u] = reinterpret_cast<const float4*>(crow[u])[k];
                        const float4 av = reinterpret_cast<const float4*>(s.A)[k];
                        const float4 wv = reinterpret_cast<const float4*>(w2)[k];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            acc[u] = fmaf(wv.x, fmax_nn(av.x + cv[u].x, 0.f), acc[u]); acc[u] = fmaf(wv.y, fmax_nn(av.y + cv[u].y, 0.f), acc[u]);
                            acc[u] = fmaf(wv.z, fmax_nn(av.z + cv[u].z, 0.f), acc[u]); acc[u] = fmaf(wv.w, fmax_nn(av.w + cv[u].w, 0.f), acc[u]);
                        }
                    }
                } else {
                    for (int k = gl; k < items; k += G) {
                        float cv[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) cv[u] = crow[u][k];
#pragma unroll
                        for (int u = 0; u < U; ++u) acc[u] = fmaf(w2[k], fmax_nn(s.A[k] + cv[u], 0.f), acc[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int d = d0 + u * stride;
                    const float r = group_sum(acc[u], G);
                    if (gl == 0 && d < D) { const float yv = r + b2; s.y[d] = yv; tp.y[row * D + d] = yv; }
                }
            }
        }
#endif
        __syncthreads();
        {   // stop-mask bookkeeping (model.py:852) -- uniform decision for the whole workgroup
            const float m_t = s.misc[0], sv = s.misc[3];
            const float m_next = fminf(m_t, sv);
            const bool first_stop = (m_next == 0.f) && (s.misc[1] < 0.f);
            const bool last = (t == T - 1);
            if (first_stop || (last && s.misc[1] < 0.f)) {
                for (int d = tid; d < D; d += nt) s.yout[d] = s.y[d];   // the output step (model.py:1261-1264)
            }
            __syncthreads();
            if (tid == 0) {
                tp.mask[(size_t)(t + 1) * B + b] = (uint8_t)(m_next != 0.f);
                if (first_stop || (last && s.misc[1] < 0.f)) s.misc[1] = (float)t;
                s.misc[0] = m_next;
            }
            __syncthreads();
            // a sample whose conversation has ended contributes nothing further to any loss (its
            // query w_t is never read: the receiver-message stream is active only while m_{t+1} == 1)
            if (!ar.run_all && !dm.fixed && train && m_next == 0.f) { ++t; break; }
        }
        // softmax(y) (detached, model.py:441) and the description mixture (model.py:442-449)
        float mx = -3.4e38f;
        for (int d = tid; d < D; d += nt) mx = fmaxf(mx, s.y[d]);
        mx = block_max(mx, s.misc + 8);
        float se = 0.f;
        for (int d = tid; d < D; d += nt) { const float e = expf(s.y[d] - mx); s.y[d] = e; se += e; }
        se = block_sum(se, s.misc + 16);
        const float inv = 1.f / se;
        for (int d = tid; d < D; d += nt) s.y[d] *= inv;
        __syncthreads();
#if MMG_CONV_ATTN
        {                                       // model.py:444-449 over the weighted descriptions: alpha keeps its graph, softmax(y) does not
            const int* cls = at.tp.attn_cls;
            for (int j = tid; j < at.NW; j += nt) s_coef[j] = s.y[cls[j]] * s_alpha[j];
            __syncthreads();
            gemv_t(at.tp.attn_set, V, at.NW, V, s_coef, s.dbar, s.red, false);
        }
#else
        gemv_t(ar.desc, V, D, V, s.y, s.dbar, s.red, false);
#endif
        for (int v = tid; v < V; v += nt) tp.dbar[row * V + v] = s.dbar[v];
        {   // h_w = tanh(w_h(h) + w_d(dbar))   (model.py:452)
            gemv_rows<GU>(P.p[R_WH_W], R, R, R, s.hn, [&](int n, float acc) { s.g[n] = acc; });
            gemv_rows<GU>(P.p[R_WD_W], V, R, V, s.dbar, [&](int n, float acc) { s.g2[n] = acc; });
        }
        __syncthreads();
        for (int i = tid; i < R; i += nt) {
            const float gv = tanhf((s.g[i] + P.p[R_WH_B][i]) + s.g2[i]);
            s.g[i] = gv;
            tp.g[row * R + i] = gv;
            s.h[i] = s.hn[i];                                       // advance the GRU state
        }
        __syncthreads();
        {   // receiver message (model.py:454-475)
            const float* bw = P.p[R_W_B];
            const float* uw = ar.u_w ? ar.u_w + row * W : nullptr;
            gemv_rows<GU>(P.p[R_W_W], R, W, R, s.g, [&](int n, float acc) { s.w[n] = acc; });
            __syncthreads();
            for (int n = tid; n < W; n += nt) {
                const float lw = s.w[n] + bw[n];
                float wv = lw, lpv = 0.f, nev = 0.f;
                if (binary) {
                    const float p = sigmoidf_(lw);
                    if (train) {
                        const float u = uw ? uw[n] : philox_uniform(ar.seed, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, 2u);
                        wv = (u < p) ? 1.f : 0.f;                  // model.py:460
                        if (RELAX) {
                            const float soft = relax_soft(lw, u, ar.relax_tau_w);
                            tp.ws[row * W + n] = soft;
                            if (!ar.relax_hard) wv = soft;
                        }
                    } else {
                        wv = rintf(p);                             // model.py:462
                    }
                    if (FLIP) wv = flip_msg(ar, true, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, wv);       // model.py:467-468
                    if (VAR && (ar.sender_var & SV_IGNORE_REC)) wv = 0.f;                                          // model.py:470-472 (the draw above is still consumed)
                    tp.pw[row * W + n] = p;
                    const float l1 = logf(p + MMG_EPS), l0 = logf(1.f - p + MMG_EPS);
                    lpv = wv * l1 + (1.f - wv) * l0;
                    nev = p * l1 + (1.f - p) * l0;
                }
                if (NOISE && !binary) wv = noise_msg(ar, true, (uint32_t)((t * dm.Bg + gb) * W + n), mb_counter, wv);
                s.w[n] = wv; s.lp[n] = lpv; s_ne[n] = nev;
                tp.w[row * W + n] = wv;
            }
        }
        __syncthreads();
        if (binary) {
            float lpv = 0.f, nev = 0.f;
            for (int j = tid; j < W; j += nt) { lpv += s.lp[j]; nev += s_ne[j]; }
            lpv = block_sum(lpv, s.misc + 8);
            nev = block_sum(nev, s.misc + 16);
            if (tid == 0) { tp.lp_w[row] = lpv; tp.ne_w[row] = nev; }
        }
        __syncthreads();
    }
    if (!do_rec) return;

    // ---- agent-level state hand-back ----
    if (ar.h_state) for (int i = tid; i < R; i += nt) ar.h_state[(size_t)b * R + i] = s.h[i];
    if (ar.sprod_state && tid == 0) ar.sprod_state[b] = s.misc[2];
    if (ar.t_end != T && s.misc[1] < 0.f) return;     // partial window without an output step
    if (ar.t_begin != 0) return;

    // ---- output selection, log-softmax, reward, top-k (model.py:1264-1275, 1333-1339) ----
    const int tstar = dm.fixed ? (T - 1) : (int)s.misc[1];
    if (dm.fixed) {
        __syncthreads();
        for (int d = tid; d < D; d += nt) s.yout[d] = tp.y[((size_t)(T - 1) * B + b) * D + d];
        __syncthreads();
    }
    if (tid == 0) tp.tstar[b] = tstar;
    float mx = -3.4e38f;
    for (int d = tid; d < D; d += nt) mx = fmaxf(mx, s.yout[d]);
    mx = block_max(mx, s.misc + 8);
    float se = 0.f;
    for (int d = tid; d < D; d += nt) se += expf(s.yout[d] - mx);
    se = block_sum(se, s.misc + 16);
    const float lse = mx + logf(se);
    const int tgt = ar.target ? (int)ar.target[b] : -1;
    const float dt = (tgt >= 0) ? (s.yout[tgt] - lse) : 0.f;
    float above = 0.f;
    for (int d = tid; d < D; d += nt) {
        const float o = s.yout[d], ld = o - lse;
        tp.outp[(size_t)b * D + d] = o;
        tp.dist[(size_t)b * D + d] = ld;
        tp.sm[(size_t)b * D + d] = expf(ld);
        if (tgt >= 0 && ld > dt) above += 1.f;
    }
    above = block_sum(above, s.misc + 8);
    if (tid == 0) {
        tp.logs[b] = dt;
        tp.hit[b] = (tgt >= 0 && above < (float)dm.top_k) ? 1 : 0;
    }
}
