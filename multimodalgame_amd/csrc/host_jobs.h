// host_jobs.h -- host side of mmg.hip: k_wgrad's job tables (kernels_bwd.h: JobTable).  Included by mmg.hip only.
#pragma once

static_assert(sizeof(JobTable) <= MMG_TABLE_BYTES, "the job table does not fit its tape slot (tape.tables)");
static_assert(sizeof(JobTable) <= MMG_VJP_TABLE_BYTES, "a VJP job table does not fit its tape slot");

// Appends jobs to a table and closes it.  split_rows: the row count of the (step, sample) jobs that reduce over the live-row list
// and may split their rows over workgroups (0: no such job -- the VJP tables).
struct JobBuilder {
    JobTable& jt;
    int split_rows;
    long long ptotal;
    bool small_split, bias_as_gemm;
    const float* ones;
    int tiles = 0, ng = 0, cblocks = 0, nc = 0;
    // frozen agents (mmg_set_trainable): a job whose destination lies in a frozen agent's slice of the gradient buffer is not entered --
    // the caller still gets a record to fill in (off_g / off_c), which no table holds
    int frozen = 0;
    const float* grads = nullptr;
    const int64_t* agent_begin = nullptr;
    GemmJob off_g;
    ColJob off_c;
    JobBuilder(JobTable& jt_, int split_rows_, long long ptotal_, bool small_split_, bool bias_as_gemm_, const float* ones_)
        : jt(jt_), split_rows(split_rows_), ptotal(ptotal_), small_split(small_split_), bias_as_gemm(bias_as_gemm_), ones(ones_) {
        memset(&jt, 0, sizeof(jt));
    }
    void freeze(int frozen_, const float* grads_, const int64_t* agent_begin_) { frozen = frozen_; grads = grads_; agent_begin = agent_begin_; }
    bool off(const float* dst) const {
        if (!frozen) return false;
        const int64_t at = dst - grads;
        int a = 0;
        for (int k = 1; k < 4; ++k) if (at >= agent_begin[k]) a = k;
        return (frozen >> a) & 1;
    }
    GemmJob& gemm(const float* A, int lda, const float* Bm, int ldb, int bmod, int bsrc, float* C, int ldc, int rows, int N, int Kk) {
        const bool skip = off(C);
        GemmJob& g = skip ? off_g : jt.g[ng++];
        g.A = A; g.Bm = Bm; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.rows = rows; g.N = N; g.K = Kk;
        g.bmod = bmod; g.bsrc = bsrc; g.tile_begin = tiles; g.tiles_k = (Kk + 31) / 32;     // 16 x 32 outputs per block
        g.vhid = nullptr; g.vw2 = nullptr; g.compact = (rows == split_rows) ? 1 : 0;
        g.nsplit = (rows != split_rows) ? 1 : small_split ? wgrad_job_nsplit(rows, ptotal, ((N + 15) / 16) * ((Kk + 31) / 32))
                                                          : wgrad_nsplit(rows, ptotal);
        if (!skip) tiles += ((N + 15) / 16) * g.tiles_k * g.nsplit;
        return g;
    }
    // a job whose rows are NOT (step, sample) rows whatever their count (the words of a description set): never compact, never split
    GemmJob& gemm_fixed(const float* A, int lda, const float* Bm, int ldb, float* C, int ldc, int rows, int N, int Kk) {
        const int keep = split_rows;
        split_rows = -1;
        GemmJob& g = gemm(A, lda, Bm, ldb, 0, SRC_STATIC, C, ldc, rows, N, Kk);
        split_rows = keep;
        return g;
    }
    // dW = (dbeta * w2 * relu'(hid))^T . input  with the first factor formed on the fly
    void gemm_virt(const float* dbeta, const float* hid, const float* w2, const float* Bm, int ldb, int bmod,
                   float* C, int ldc, int rows, int N, int Kk) {
        GemmJob& g = gemm(dbeta, N, Bm, ldb, bmod, SRC_STATIC, C, ldc, rows, N, Kk);
        g.vhid = hid; g.vw2 = w2;
    }
    ColJob& col(const float* src, int ld, int rows, int cols, float* dst, const float* scale) {
        const bool skip = off(dst);
        ColJob& c = skip ? off_c : jt.c[nc++];
        c.src = src; c.dst = dst; c.scale = scale; c.ld = ld; c.rows = rows; c.cols = cols; c.blk_begin = cblocks;
        c.vbeta = nullptr; c.vw2 = nullptr; c.wrow = nullptr; c.compact = (rows == split_rows) ? 1 : 0; c.special = 0;
        if (!skip) cblocks += (cols + 15) / 16;
        return c;
    }
    // bias gradient = column sums of a (step, sample)-row tape.  With thousands of rows the 16-column blocks of a column job
    // are a handful of latency-bound workgroups: run it through the row-split GEMM pipeline instead, as delta^T . ones (K = 1)
    void bias(const float* src, int ld, int rows, int cols, float* dst) {       // plain column sums over the (step, sample) rows
        if (bias_as_gemm) gemm(src, ld, ones, 0, 0, SRC_STATIC, dst, 1, rows, cols, 1);
        else col(src, ld, rows, cols, dst, nullptr);
    }
    // block totals, the special block, the lane-parallel copies of the jobs' first blocks; `where` names the table in the message
    int finish(const char* where) {
        if (ng > MMG_MAX_GEMM || nc > MMG_MAX_COL) return fail("job table overflow");
        jt.n_gemm = ng; jt.n_col = nc; jt.gemm_tiles = tiles; jt.gemm_blocks = tiles; jt.col_blocks = cblocks;
        jt.n_wblocks = tiles + cblocks;
        jt.special_block = -1; jt.special_job = -1;
        for (int c = 0; c < nc; ++c) if (jt.c[c].special) { jt.special_job = c; jt.special_block = tiles + jt.c[c].blk_begin; }
        for (int k = 0; k < 64; ++k) {
            jt.g_begin[k] = k < ng ? jt.g[k].tile_begin : 0x7fffffff;
            jt.c_begin[k] = k < nc ? jt.c[k].blk_begin : 0x7fffffff;
        }
        if (jt.n_wblocks > MMG_MAX_WBLOCKS) return fail("too many weight-gradient tiles%s (%d)", where, jt.n_wblocks);   // (k_wgrad addresses 16384 workgroups)
        return 0;
    }
};

// ---------------------------------------------------------------------------------------------
// job table: every parameter tensor's gradient is produced by exactly one GEMM / column-sum job
// (two for the matrices whose input is a concatenation: y1, both baselines' linear1).
// code_bias: which kernels leave the sender's code_bias operands behind (host_select.h: the family -- FAM_TILE / FAM_FAST / the others).
// ---------------------------------------------------------------------------------------------
enum CodeBiasJob { CODE_BIAS_TILE, CODE_BIAS_FAST, CODE_BIAS_GENERIC };

static int build_jobs(mmg_handle* h, CodeBiasJob code_bias, bool small_split) {
    JobTable& jt = h->jt;
    const Dims& d = h->dm;
    const Tape& tp = h->tp;
    const Params& G = h->G;
    const int B = d.B, T = d.T, H = d.H, W = d.W, R = d.R, V = d.V, K = d.K, D = d.D, F = d.F;
    const int TB = T * B;
    JobBuilder jb(jt, TB, h->pl.total, small_split, wgrad_nsplit(TB, h->pl.total) > 1 || (small_split && TB > 2048), tp.ones);
    jb.freeze(frozen_agents(h), h->grads, h->pl.agent_begin);
    const Params& P = h->P;
    const bool bin = d.use_binary;
    // ---- receiver ----
    jb.gemm(tp.dgi, 3 * R, tp.z, W, 0, SRC_STATIC, G.p[R_WIH], W, TB, 3 * R, W);          // rnn.weight_ih
    jb.gemm(tp.dgh, 3 * R, tp.h, R, 0, SRC_STATIC, G.p[R_WHH], R, TB, 3 * R, R);          // rnn.weight_hh (h before the step)
    jb.bias(tp.dgi, 3 * R, TB, 3 * R, G.p[R_BIH]);
    jb.bias(tp.dgh, 3 * R, TB, 3 * R, G.p[R_BHH]);
    if (h->attn_dim) {
        // description attention (model.py:409-410 puts the description FIRST): y1.weight[:, :V] = dE^T . set, y1.weight[:, V:] = dA^T . h*;
        // the three extra layers: d_d from dDD over the words, d_h and d_attn.weight from the (step, sample) tapes of k_bwd_conv_attn.
        // d_attn.bias has NO job: a shift inside a softmax segment -- its gradient is exactly zero, the buffer keeps mmg_attn_create's zero
        const AttnTape& atp = h->at.tp; const AttnParams& AG = h->AG;
        const int A = h->attn_dim, NW = h->n_words;
        jb.gemm_fixed(atp.attn_dE, R, atp.attn_set, V, G.p[R_Y1_W], R + V, NW, R, V);
        jb.gemm(tp.dA, R, tp.hstar, R, 0, SRC_STATIC, G.p[R_Y1_W] + V, R + V, B, R, R);
        jb.gemm_fixed(atp.attn_dDD, A, atp.attn_set, V, AG.p[A_DD_W], V, NW, A, V);
        jb.col(atp.attn_dDD, A, NW, A, AG.p[A_DD_B], nullptr).compact = 0;
        jb.gemm(atp.attn_ddh, A, tp.h + (size_t)B * R, R, 0, SRC_STATIC, AG.p[A_DH_W], R, TB, A, R);   // d_h (h after the step)
        jb.bias(atp.attn_ddh, A, TB, A, AG.p[A_DH_B]);
        jb.bias(atp.attn_dv, A, TB, A, AG.p[A_DA_W]);
    } else {
    jb.gemm(tp.dA, R, tp.hstar, R, 0, SRC_STATIC, G.p[R_Y1_W], R + V, B, R, R);           // y1.weight[:, :R]
    jb.gemm(tp.dC, R, tp.descc, V, 0, SRC_STATIC, G.p[R_Y1_W] + R, R + V, D, R, V);      // y1.weight[:, R:]
    }
    if (h->attn_dim) jb.col(tp.dA, R, B, R, G.p[R_Y1_B], nullptr).compact = 0;             // y1.bias = sum_b dA (sum_d first, where it cancels: bwd_conv_body.h)
    else jb.col(tp.dC, R, D, R, G.p[R_Y1_B], nullptr);
    jb.col(tp.Py2, R, D, R, G.p[R_Y2_W], nullptr);
    jb.col(tp.dysum, 1, B, 1, G.p[R_Y2_B], nullptr);
    if (bin) {
        jb.gemm(tp.dgpre, R, tp.h + (size_t)B * R, R, 0, SRC_STATIC, G.p[R_WH_W], R, TB, R, R);   // w_h (h after the step)
        jb.bias(tp.dgpre, R, TB, R, G.p[R_WH_B]);
        jb.gemm(tp.dgpre, R, tp.dbar, V, 0, SRC_STATIC, G.p[R_WD_W], V, TB, R, V);        // w_d
        jb.gemm(tp.dlw, W, tp.g, R, 0, SRC_STATIC, G.p[R_W_W], R, TB, W, R);              // w
        jb.bias(tp.dlw, W, TB, W, G.p[R_W_B]);
        jb.col(tp.h + (size_t)B * R, R, TB, R, G.p[R_S_W], nullptr).wrow = tp.dls;        // s.weight = dls^T . h_after
        jb.col(tp.dls, 1, TB, 1, G.p[R_S_B], nullptr);
        // ---- sender ----
        if (h->vd.A) {
            // visual attention: h_x is per step -- image_layer's input is the step's x_attn, its delta the step's dpre (at t == 0 too, where
            // x_attn is the mean over the locations); the attention tensors from the (step, sample) tapes of k_vattn_bwd.  attn_W_x.weight has
            // no job (k_vattn_dwx: its operand is channel-major), attn_U.bias none at all: its gradient is exactly zero, the buffer keeps
            // mmg_vattn_create's zero.  The three biases add into one pre-activation: the same column sums, three times the same reduction
            const VattnTape& vtp = h->va.tp; const VattnParams& VG = h->VG;
            const int A = h->vd.A, Gc = h->vd.G;
            jb.gemm(tp.dpre, H, vtp.vattn_xa, F, 0, SRC_STATIC, G.p[S_IMG_W], F, TB, H, F);
            jb.gemm(vtp.vattn_dq, A, tp.zr, W, 0, SRC_STATIC, VG.p[VA_WW_W], W, TB, A, W);
            if (Gc > 0) jb.gemm(vtp.vattn_dq, A, vtp.vattn_g, Gc, B, SRC_STATIC, VG.p[VA_WG_W], Gc, TB, A, Gc);
            jb.bias(vtp.vattn_dq, A, TB, A, VG.p[VA_WX_B]);
            jb.bias(vtp.vattn_dq, A, TB, A, VG.p[VA_WW_B]);
            if (Gc > 0) jb.bias(vtp.vattn_dq, A, TB, A, VG.p[VA_WG_B]);
            jb.bias(vtp.vattn_dv, A, TB, A, VG.p[VA_U_W]);
        } else
        jb.gemm(tp.dhx, H, nullptr, F, 0, SRC_X, G.p[S_IMG_W], F, B, H, F);               // image_layer (sum over steps first)
        jb.col(tp.dhx, H, B, H, G.p[S_IMG_B], nullptr);
        jb.gemm(tp.dpre, H, tp.c, W, 0, SRC_STATIC, G.p[S_CODE_W], W, TB, H, W);          // code_layer
        jb.bias(tp.dpre, H, TB, H, G.p[S_CODE_B]);
        if (code_bias == CODE_BIAS_TILE) {
            // code_bias: dsig[j] * sum_h code_layer.weight[h, j] * u0[h], u0 = sum_b dpre[t = 0, b, :] (k_dhx): a row-weighted
            // column sum over the weight matrix itself
            ColJob& c = jb.col(P.p[S_CODE_W], W, H, W, G.p[S_CODE_BIAS], tp.dsig);
            c.wrow = tp.u0; c.compact = 0;
        } else if (code_bias == CODE_BIAS_FAST) {
            // code_bias: dsig[j] * sum_h code_layer.weight[h, j] * (sum_b dpre[t = 0, b, h]) -- one workgroup of k_wgrad;
            // the register-resident backward kernel then needs no per-sample W_c^T dpre_0 product at its tail
            ColJob& c = jb.col(tp.dpre, H, B, 1, G.p[S_CODE_BIAS], tp.dsig);
            c.special = 1; c.wrow = P.p[S_CODE_W]; c.compact = 0; c.cols = W;
        } else {
            jb.col(tp.dc0, W, B, W, G.p[S_CODE_BIAS], tp.dsig);                           // code_bias
        }
        jb.gemm(tp.dlz, W, tp.a, H, 0, SRC_STATIC, G.p[S_BIN_W], H, TB, W, H);            // binary_layer
        jb.bias(tp.dlz, W, TB, W, G.p[S_BIN_B]);
        // ---- baseline_rec: input [z || h_after] ----
        jb.gemm_virt(tp.dbr, tp.hid_r, P.p[BR_L2_W], tp.z, W, 0, G.p[BR_L1_W], W + R, TB, K, W);
        jb.gemm_virt(tp.dbr, tp.hid_r, P.p[BR_L2_W], tp.h + (size_t)B * R, R, 0, G.p[BR_L1_W] + W, W + R, TB, K, R);
        ColJob& r1 = jb.col(tp.hid_r, K, TB, K, G.p[BR_L1_B], nullptr);
        r1.vbeta = tp.dbr; r1.vw2 = P.p[BR_L2_W];
        jb.col(tp.hid_r, K, TB, K, G.p[BR_L2_W], nullptr).wrow = tp.dbr;
        jb.col(tp.dbr, 1, TB, 1, G.p[BR_L2_B], nullptr);
        // ---- baseline_sen: input [h_x || z_r] ----
        if (h->vd.A) jb.gemm_virt(tp.dbs, tp.hid_s, P.p[BS_L2_W], h->va.tp.vattn_hx, H, 0, G.p[BS_L1_W], H + W, TB, K, H);   // (the step's h_x)
        else jb.gemm_virt(tp.dbs, tp.hid_s, P.p[BS_L2_W], tp.hx, H, B, G.p[BS_L1_W], H + W, TB, K, H);
        jb.gemm_virt(tp.dbs, tp.hid_s, P.p[BS_L2_W], tp.zr, W, 0, G.p[BS_L1_W] + H, H + W, TB, K, W);
        ColJob& s1 = jb.col(tp.hid_s, K, TB, K, G.p[BS_L1_B], nullptr);
        s1.vbeta = tp.dbs; s1.vw2 = P.p[BS_L2_W];
        jb.col(tp.hid_s, K, TB, K, G.p[BS_L2_W], nullptr).wrow = tp.dbs;
        jb.col(tp.dbs, 1, TB, 1, G.p[BS_L2_B], nullptr);
    }
    if (jb.finish("")) return -1;
    const int tiles = jt.gemm_tiles, ng = jt.n_gemm, nc = jt.n_col;
    h->sel.wgrad_small_split = small_split;
    h->sel.any_split = false;
    for (int g = 0; g < ng; ++g) h->sel.any_split = h->sel.any_split || jt.g[g].nsplit > 1;
    {
        auto agent_of = [&](const float* dst) {
            const int64_t off = dst - h->grads;
            int a = 0;
            for (int k = 1; k < 4; ++k) if (off >= h->pl.agent_begin[k]) a = k;
            return (signed char)a;
        };
        for (int g = 0; g < ng; ++g) {
            const int end = (g + 1 < ng) ? jt.g[g + 1].tile_begin : tiles;
            for (int t = jt.g[g].tile_begin; t < end; ++t) jt.wblock_agent[t] = agent_of(jt.g[g].C);
        }
        for (int c = 0; c < nc; ++c) {
            const int end = (c + 1 < nc) ? jt.c[c + 1].blk_begin : jt.col_blocks;
            for (int bk = jt.c[c].blk_begin; bk < end; ++bk) jt.wblock_agent[tiles + bk] = agent_of(jt.c[c].dst);
        }
    }
    // ---- gradient-norm plan: MMG_GN_BLOCKS chunks, each inside one agent ----
    const ParamLayout& pl = h->pl;
    int nb[4];
    int left = MMG_GN_BLOCKS - 4;
    for (int a = 0; a < 4; ++a) {
        const double frac = (double)(pl.agent_begin[a + 1] - pl.agent_begin[a]) / (double)pl.total;
        nb[a] = 1 + (int)(frac * left);
    }
    int blk = 0;
    for (int a = 0; a < 4; ++a) {
        const int64_t b0 = pl.agent_begin[a], b1 = pl.agent_begin[a + 1];
        const int64_t quads = (b1 - b0) / 4;
        for (int k = 0; k < nb[a]; ++k) {
            jt.np.begin[blk] = b0 + 4 * (quads * k / nb[a]);
            jt.np.end[blk] = b0 + 4 * (quads * (k + 1) / nb[a]);
            jt.np.agent[blk] = a;
            ++blk;
        }
    }
    for (; blk < MMG_GN_BLOCKS; ++blk) { jt.np.begin[blk] = jt.np.end[blk] = 0; jt.np.agent[blk] = -1; }
    return 0;
}

// Which split plan the job table of this handle uses (Selection::wgrad_small_split, any_split), and the table itself (h->jt):
// jobs with few output tiles split their rows further only when the whole table leaves the chip idle otherwise (continuous
// mode: the receiver's dozen small matrices; measured at config 5, 256 samples: k_wgrad 32 -> 22 us.  With a full table --
// config 3 at 512 samples, 1 660 tiles -- the extra tiles made it slower: 104 -> 205 us)
static int plan_jobs(mmg_handle* h, CodeBiasJob code_bias) {
    if (build_jobs(h, code_bias, false)) return -1;
    if (h->jt.gemm_tiles > 256 || h->dm.T * h->dm.B <= 2048) return 0;
    if (build_jobs(h, code_bias, true) == 0) return 0;
    return build_jobs(h, code_bias, false);              // (the finer split overflows k_wgrad's 16384 workgroups)
}

// ---------------------------------------------------------------------------------------------
// Job tables of mmg_exchange_vjp (kernels_vjp.h): one per agent, each writing only that agent's gradient slice.  Same job kinds as
// build_jobs, but every (step, sample) job reduces over ALL T * B rows (rows of steps t >= n_steps carry zero deltas), no row
// splits, no live-row list, no special block.  They depend on the shape only: built and uploaded once, at mmg_create.
// percall: the tables of the per-call VJPs (mmg_sender_vjp / _receiver_vjp / _baseline_vjp) -- the same jobs over the B rows of
// one call, with the operands the exchange reads from the tape taken from the call's copies (vcz, vch0, vch1, vchx).
// ---------------------------------------------------------------------------------------------
static int build_vjp_job_table(mmg_handle* h, int agent, bool percall, JobTable& jt) {
    const Dims& d = h->dm;
    const Tape& tp = h->tp;
    const Params &G = h->G, &P = h->P;
    const int B = d.B, H = d.H, W = d.W, R = d.R, V = d.V, K = d.K, D = d.D, F = d.F;
    const int TB = percall ? B : d.T * B;
    JobBuilder jb(jt, 0, h->pl.total, false, false, tp.ones);
    const float* h_before = percall ? tp.vch0 : tp.h;
    const float* h_after = percall ? tp.vch1 : tp.h + (size_t)B * R;
    const float* z_in = percall ? tp.vcz : tp.z;
    if (agent == MMG_AGENT_RECEIVER) {
        jb.gemm(tp.vdgi, 3 * R, z_in, W, 0, SRC_STATIC, G.p[R_WIH], W, TB, 3 * R, W);              // rnn.weight_ih
        jb.gemm(tp.vdgh, 3 * R, h_before, R, 0, SRC_STATIC, G.p[R_WHH], R, TB, 3 * R, R);          // rnn.weight_hh (h before the step)
        jb.bias(tp.vdgi, 3 * R, TB, 3 * R, G.p[R_BIH]);
        jb.bias(tp.vdgh, 3 * R, TB, 3 * R, G.p[R_BHH]);
        jb.gemm(tp.vdA, R, h_after, R, 0, SRC_STATIC, G.p[R_Y1_W], R + V, TB, R, R);               // y1.weight[:, :R]: dA_t over T * B rows
        jb.gemm(tp.vdC, R, tp.vdesc, V, 0, SRC_STATIC, G.p[R_Y1_W] + R, R + V, D, R, V);          // y1.weight[:, R:]
        jb.col(tp.vdC, R, D, R, G.p[R_Y1_B], nullptr);
        jb.col(tp.vPy2, R, D, R, G.p[R_Y2_W], nullptr);
        jb.col(tp.vdys, 1, TB, 1, G.p[R_Y2_B], nullptr);
        jb.gemm(tp.vdgpre, R, h_after, R, 0, SRC_STATIC, G.p[R_WH_W], R, TB, R, R);               // w_h
        jb.bias(tp.vdgpre, R, TB, R, G.p[R_WH_B]);
        jb.gemm(tp.vdgpre, R, tp.vdbar, V, 0, SRC_STATIC, G.p[R_WD_W], V, TB, R, V);              // w_d
        jb.gemm(tp.vdlw, W, tp.vg, R, 0, SRC_STATIC, G.p[R_W_W], R, TB, W, R);                    // w
        jb.bias(tp.vdlw, W, TB, W, G.p[R_W_B]);
        jb.col(h_after, R, TB, R, G.p[R_S_W], nullptr).wrow = tp.vdls;                            // s.weight = dls^T . h_after
        jb.col(tp.vdls, 1, TB, 1, G.p[R_S_B], nullptr);
    } else if (agent == MMG_AGENT_SENDER) {
        jb.gemm(tp.vdhx, H, nullptr, F, 0, SRC_X, G.p[S_IMG_W], F, B, H, F);                       // image_layer (sum over steps first)
        jb.col(tp.vdhx, H, B, H, G.p[S_IMG_B], nullptr);
        jb.gemm(tp.vdpre, H, tp.vc, W, 0, SRC_STATIC, G.p[S_CODE_W], W, TB, H, W);                 // code_layer (t = 0: sigmoid(code_bias))
        jb.bias(tp.vdpre, H, TB, H, G.p[S_CODE_B]);
        jb.col(tp.vdc0, W, B, W, G.p[S_CODE_BIAS], tp.vdsig);                                      // code_bias
        jb.gemm(tp.vdlz, W, tp.va, H, 0, SRC_STATIC, G.p[S_BIN_W], H, TB, W, H);                   // binary_layer
        jb.bias(tp.vdlz, W, TB, W, G.p[S_BIN_B]);
    } else if (agent == MMG_AGENT_BASELINE_REC) {                                                // input [z || h_after]
        jb.gemm_virt(tp.vdbr, tp.vhid_r, P.p[BR_L2_W], z_in, W, 0, G.p[BR_L1_W], W + R, TB, K, W);
        jb.gemm_virt(tp.vdbr, tp.vhid_r, P.p[BR_L2_W], h_after, R, 0, G.p[BR_L1_W] + W, W + R, TB, K, R);
        ColJob& c1 = jb.col(tp.vhid_r, K, TB, K, G.p[BR_L1_B], nullptr);
        c1.vbeta = tp.vdbr; c1.vw2 = P.p[BR_L2_W];
        jb.col(tp.vhid_r, K, TB, K, G.p[BR_L2_W], nullptr).wrow = tp.vdbr;
        jb.col(tp.vdbr, 1, TB, 1, G.p[BR_L2_B], nullptr);
    } else {                                                                                    // input [h_x || z_r]
        jb.gemm_virt(tp.vdbs, tp.vhid_s, P.p[BS_L2_W], percall ? tp.vchx : tp.hx, H, B, G.p[BS_L1_W], H + W, TB, K, H);
        jb.gemm_virt(tp.vdbs, tp.vhid_s, P.p[BS_L2_W], percall ? tp.vcz : tp.vzr, W, 0, G.p[BS_L1_W] + H, H + W, TB, K, W);
        ColJob& c1 = jb.col(tp.vhid_s, K, TB, K, G.p[BS_L1_B], nullptr);
        c1.vbeta = tp.vdbs; c1.vw2 = P.p[BS_L2_W];
        jb.col(tp.vhid_s, K, TB, K, G.p[BS_L2_W], nullptr).wrow = tp.vdbs;
        jb.col(tp.vdbs, 1, TB, 1, G.p[BS_L2_B], nullptr);
    }
    if (jb.finish((" in the VJP of agent " + std::to_string(agent)).c_str())) return -1;
    for (int k = 0; k < jt.n_wblocks; ++k) jt.wblock_agent[k] = (signed char)agent;
    for (int k = 0; k < MMG_GN_BLOCKS; ++k) { jt.np.begin[k] = jt.np.end[k] = 0; jt.np.agent[k] = -1; }
    return 0;
}

static int upload_vjp_tables(mmg_handle* h) {
    std::vector<JobTable> tabs(8);
    for (int a = 0; a < 8; ++a) {
        if (build_vjp_job_table(h, a % 4, a >= 4, tabs[a])) return -1;
        WgHead& hd = h->vjp_hd[a];
        hd.gemm_tiles = tabs[a].gemm_tiles; hd.n_wblocks = tabs[a].n_wblocks; hd.special_block = -1; hd.special_job = -1;
    }
    for (int a = 0; a < 8; ++a)
        HIP_OK(hipMemcpy(h->tp.vtables + (size_t)a * MMG_VJP_TABLE_BYTES, &tabs[a], sizeof(JobTable), hipMemcpyHostToDevice));
    return 0;
}
