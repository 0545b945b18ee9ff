// host_select.h -- host side of mmg.hip: launch geometry shared by the selection and the launches, the path predicates and
// select_paths.  Included by mmg.hip only (after host_launch.h and host_jobs.h).
#pragma once

// ---------------------------------------------------------------------------------------------
// Launch geometry: role / tile counts that select_paths proves co-resident and the launches use as their grids.  (The kernels
// find their roles from the counts they are handed; what they compute themselves stays in the kernel headers.)
// ---------------------------------------------------------------------------------------------
inline int sample_tiles(int B) { return (B + MMG_TM - 1) / MMG_TM; }
inline int stat_roles(int T) { return (5 * T + 2 + 3) / 4; }          // statistics roles: one (stream, step) pair per wave
inline int bas_roles(const Dims& d) { return ((d.T * d.B + 15) / 16) * 2 * ((d.K + 63) / 64); }     // baseline roles: 16 live rows x 64 hidden units each
inline int basehx_tiles(const Dims& d) { return ((d.B + 15) / 16) * ((d.K + 15) / 16); }
// basehx tiles for k_baselines4 ride along a conversation launch as trailing workgroups (training minibatches of <= 64 samples)
inline bool basehx_rides(const Dims& d, int nchunk, int train, int run_all, bool merge_roles) {
    return nchunk == 1 && train && d.use_binary && !run_all && d.B <= 64 && !(d.H & 3) && merge_roles;
}
// roles per sample tile of the wide receiver's one-launch conversation (k_rc_persist)
inline int rc_roles_per_tile(const Dims& d) {
    const int nj = d.R / 16, njw = d.W / 16;
    return (nj > njw ? nj : njw) + njw + (d.H + 63) / 64 + 1;
}

// register-resident kernels exist for the agent shape of BASELINE configs 1-3
static bool fast_shape(const mmg_handle* h) {
    const Dims& d = h->dm;
    if (h->sel.tile_ok && h->sel.tile_force) return false;
    return h->sel.use_fast && d.H == 256 && d.W == 32 && d.R == 64 && (d.V == 100 || fast_wide_v(d.V)) && d.D <= 32 && d.T <= 16;   // (D = 30: own instantiation, other D <= 32: capacity 32; V = 100 likewise, other V % 4 == 0: at run time)
}
// every other shape: sample tiles on the matrix cores (kernels_tile.h); the per-sample generic kernels remain for
// dimensions whose tile does not fit the LDS and for the agent-level entry points
// the small agents with many classes (32 < D <= 1024): register-resident conversation with class slices (kernels_mc.h) up to 2 048
// samples per GPU (measured at D = 1000: 2 048 samples 1 064 us per minibatch against 1 113 on the sample tiles, 4 096 samples
// 2 090 against 1 242 -- from 256 tiles on, the tiles fill the chip and a workgroup per sample is 16 waves of it;
// MMG_TILE=1 forces the tiles)
static bool mc_path(const mmg_handle* h) { return h->sel.mc_ok && !(h->sel.tile_ok && h->sel.tile_force) && (h->dm.B <= 2048 || !h->sel.tile_ok); }
static bool tile_path(const mmg_handle* h) { return h->sel.tile_ok && !fast_shape(h) && !mc_path(h); }
// continuous many-class path: the two-launch backward of kernels_mc.h
static bool mc_bwd(const mmg_handle* h) { return mc_path(h) && !h->dm.use_binary; }
// single-GPU minibatch: the statistics run as extra roles of the backward launch (no all-reduce in between)
static bool merge_stats(const mmg_handle* h) {
    if (mc_bwd(h)) return h->sel.merge_roles;            // (sum of rewards / hits only: one extra workgroup of k_bwd_mc2)
    return fast_shape(h) && h->dm.use_binary && h->fwd.scores_in_parts && h->sel.merge_roles;
}

// ---------------------------------------------------------------------------------------------
// Path selection: which kernels serve this handle's shape on this device.  Runs at mmg_create and again when the library
// falls back to launches WITHOUT in-launch waits (h->no_roles: after a timed-out dependency, for a CU budget / CU mask that
// cannot hold the role launches, or MMG_NO_ROLES=1).  Environment switches are read here only -- never on the per-minibatch path.
// ---------------------------------------------------------------------------------------------
static int select_paths(mmg_handle* h) {
    const mmg_config& cfg = h->cfg;
    const Dims& d = h->dm;
    const bool no_roles = h->no_roles;
    h->sel = Selection();
    Selection& s = h->sel;
    s.use_fast = !getenv("MMG_NO_FAST"); s.merge_roles = !getenv("MMG_NO_MERGE") && !no_roles;
    s.sw_merge_prep = !getenv("MMG_NO_MERGE_PREP") && !no_roles;
    s.sw_merge_bas = s.merge_roles;
    s.persist_ll = !getenv("MMG_NO_PERSIST_LL") && persist_ll_shape(cfg.batch, cfg.h_dim, cfg.w_dim, cfg.rec_hidden, cfg.wv_dim, cfg.n_classes, cfg.max_exchange);
    s.sw_rsample = !getenv("MMG_NO_RSAMPLE"); s.sw_rmsg = !getenv("MMG_NO_RMSG"); s.sw_fused_s = !getenv("MMG_NO_FUSED_S");
    s.mc_ok = s.use_fast && mc_shape(d.H, d.W, d.R, d.V, d.D, d.T) && !getenv("MMG_NO_MC") && !no_roles;
    s.mc_per = (((d.D + 15) / 16) + 3) & ~3;
    s.mc_xcd = 1;                                   // a tile's 16 workgroups on one XCD (measured at config 5, 256 samples: 192 us per minibatch against 201); cleared below on a device without room for it
    int n_cu = 0;
    {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu <= 0) return fail("cannot query the device (multiProcessorCount)");
        // caller-supplied budget (mmg_config.cu_budget): a process that shares the GPU, or runs under a CU mask, states how many
        // compute units it can count on -- every co-residency budget below is sized from it
        if (cfg.cu_budget > 0 && cfg.cu_budget < n_cu) n_cu = cfg.cu_budget;
    }
    // co-resident workgroups a role launch may hold: occupancy of the kernel at its LDS size x compute units, minus a margin
    // of 1/16 of the chip (256 CUs -> 240, the value the role launches were tuned with).  A partitioned device (CPX), a
    // smaller SKU or a masked process simply gets a smaller budget and, where the roles do not fit, the per-step / generic launches.
    auto budget_of = [&](const void* fn, int threads, int smem) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, (size_t)smem) != hipSuccess || nb < 1) return 0;
        const int total = nb * n_cu;
        return total - (total + 15) / 16;
    };
    // raises a kernel's dynamic LDS limit; e keeps the first error (reported once, below)
    hipError_t e = hipSuccess;
    auto raise_lds = [&](const void* fn, int bytes) {
        if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    };
    s.n_cu = n_cu;
    // few samples and large sender matrices or class tables: 512-thread variant of the generic conversation kernel
    s.conv_threads = (d.B <= 256 && ((int64_t)d.H * d.W >= 65536 || (int64_t)d.D * (d.R + d.V) >= 65536)) ? 512 : 256;
    s.conv_smem = conv_smem_floats(d, s.conv_threads) * 4;
    s.conv_smem_agent = conv_smem_floats(d, MMG_BLOCK) * 4;
    s.bwd_smem = bwd_smem_floats(d) * 4;
    s.prep_smem = ((d.V > d.W ? d.V : d.W) + 16) * 4;
    // hundreds of classes: 8 per class block of k_prep (weight rows in registers across them); few classes: one per block (latency)
    s.prep_cpb = (d.D >= 256 && d.R <= 64 && d.V <= 128 && !(d.V & 3) && 2 * d.R <= MMG_BLOCK) ? 2 : 1;
    if (s.prep_cpb > 1 && (int)(s.prep_cpb * (d.V + d.R) * 4) > s.prep_smem) s.prep_smem = s.prep_cpb * (d.V + d.R) * 4;
    if (s.conv_smem > 160 * 1024 || s.bwd_smem > 160 * 1024) return fail("dimensions need more than 160 KB of LDS per sample");
    {
        const int tiles = sample_tiles(d.B);
        // few tiles and a large sender MLP: one step's sender products as chip-wide launches of their own
        s.tile_ext = tiles < 64 && (int64_t)d.H * d.W >= 65536;
        // one tile per CU up to 256 tiles: 16 waves hide the LDS / L2 latency of the tile's phases; beyond that several
        // smaller workgroups share a CU.  Fewer waves also mean smaller split-K staging areas.
        const int nts[2] = {512, 256};                            // (a 1024-thread variant spilled at 128 registers per lane: deleted)
        for (int k = (tiles <= 512 ? 0 : 1); k < 2; ++k) {
            s.tile_nt = nts[k];
            s.tile_smem = tile_lds(d, s.tile_nt / 64, !s.tile_ext).total * 4;
            if (s.tile_smem <= 160 * 1024) break;
        }
        if (!s.tile_ext && d.H > s.tile_nt) {                      // the in-kernel sender keeps the tile's h_x in 16 registers per thread
            s.tile_ext = true;
            s.tile_smem = tile_lds(d, s.tile_nt / 64, false).total * 4;
        }
        // 16-byte aligned weight rows (float4 fragments): every BASELINE shape; odd dimensions take the per-sample kernels
        const bool aligned = !(d.H & 3) && !(d.W & 3) && !(d.R & 3) && !(d.V & 3);
        s.rc_fwd = aligned && s.tile_ext && s.tile_smem > 160 * 1024 && rc_shape(d.B, d.H, d.W, d.R, d.V, d.D) && !getenv("MMG_NO_RC");
        // (the sample tiles keep a [16, V] mixture tile and V-wide split-K staging in LDS: audited and tested up to V = 256, the
        //  limit before MMG_MAX_WV; wider descriptions take the register-resident small agents or the per-sample kernels)
        s.tile_ok = aligned && d.V <= 256 && (s.tile_smem <= 160 * 1024 || s.rc_fwd) && !getenv("MMG_NO_TILE");
        s.tile_force = getenv("MMG_TILE") != nullptr;
        // many classes, small agents, fewer than 64 tiles: a workgroup per SAMPLE fills the chip (256 samples = 256 CUs) and
        // beats 16 tiles + class helpers (measured at D = 1000, B = 256: 557 us against 1 010 us per minibatch; B = 2048:
        // 2 091 against 1 189) -- the tile kernels take over from 1024 samples (MMG_TILE=1: always)
        if (s.tile_ok && !s.tile_force && !s.tile_ext && d.D * MMG_TM > 8 * 512 && d.B < 1024) s.tile_ok = false;
        // many classes and fewer sample tiles than CUs: class helpers (k_conv_split)
        s.split_nh = split_helpers(d.B);
        s.split_per = (((d.D + s.split_nh) / (s.split_nh + 1)) + 3) & ~3;
        s.tile_split = s.tile_ok && !s.tile_ext && d.D * MMG_TM > 8 * 512 && s.split_nh >= 1 && tiles * (1 + s.split_nh) <= 224 &&
                       !getenv("MMG_NO_SPLIT") && !no_roles;
        if (s.tile_split) {
            const int a = tile_lds(d, 512 / 64, true, s.split_per).total * 4, b = helper_lds(d, 512 / 64, s.split_per).total * 4;
            s.split_smem = a > b ? a : b;
            if (s.split_smem > 160 * 1024) s.tile_split = false;
            else raise_lds((const void*)k_conv_split<512>, s.split_smem);
            if (s.tile_split && e == hipSuccess) {
                s.split_budget = budget_of((const void*)k_conv_split<512>, 512, s.split_smem);
                if (tiles * (1 + s.split_nh) > s.split_budget) s.tile_split = false;     // not all co-resident here: k_conv_tile instead
            }
        }
        // per-step sender products as ROLES of one persistent launch when all of them fit on the chip together
        s.persist_ns1 = d.H / 64; s.persist_ns2 = d.W / 32;
        // (receiver shape of the register-resident kernels: per-sample receiver roles, and batches too large for one launch of
        //  co-resident roles run as consecutive launches over sample ranges)
        const bool rs_capable = d.R == 64 && d.V == 100 && d.D <= 32 && d.T <= 16 && s.sw_rsample;
        s.tile_persist = s.tile_ok && s.tile_ext && !(d.H % 64) && !(d.W % 32) && tiles <= 64 &&
                         MMG_TM * d.W <= 8 * 512 && !getenv("MMG_NO_PERSIST") && !no_roles;
        s.rs_capable = rs_capable;
        if (s.tile_persist) {
            const int a = tile_lds(d, 512 / 64, false).total * 4, b = srole_lds(d, 512 / 64).total * 4;
            s.persist_smem = a > b ? a : b;
            if (s.persist_smem > 160 * 1024) s.tile_persist = false;
            else {
                raise_lds((const void*)k_conv_persist<512, true>, s.persist_smem);
                raise_lds((const void*)k_conv_persist<512, false>, s.persist_smem);
                raise_lds((const void*)k_conv_persist<512, true, true>, s.persist_smem);
            }
            if (s.tile_persist && e == hipSuccess) {
                s.resident_budget = rs_capable ? budget_of((const void*)k_conv_persist<512, true>, 512, s.persist_smem)
                                               : budget_of((const void*)k_conv_persist<512, false>, 512, s.persist_smem);
                // tile roles: every tile's roles in one launch; per-sample receiver roles: at least ONE whole tile per launch
                const bool fits = rs_capable ? (MMG_TM + d.H / 64 + d.W / 16 <= s.resident_budget || MMG_TM + s.persist_ns1 + s.persist_ns2 <= s.resident_budget)
                                             : tiles * (1 + s.persist_ns1 + s.persist_ns2) <= s.resident_budget;
                if (!fits) s.tile_persist = false;                                       // per-step launches instead (no co-residency needed)
            }
        }
        s.tile_bwd_smem = bwd_tile_lds(d, 512 / 64).total * 4;
        s.send_bwd_smem = (MMG_TM * ld16(d.W) + 7 * 64 + 16 + tile_raw_floats_nn(64, MMG_BLOCK / 64)) * 4;
        if (s.tile_bwd_smem > 160 * 1024 || d.W > 256 || d.R > 256) s.tile_ok = false;     // (k_bwd_tile keeps a step's GRU tape in 4 registers per thread per 32 hidden units)
        const int pre_smem = bwd_pre_lds_floats(d) * 4, pre_send_smem = pre_smem > s.send_bwd_smem ? pre_smem : s.send_bwd_smem;
        if (s.tile_ok && s.tile_bwd_smem > 48 * 1024) {
            raise_lds((const void*)k_bwd_tile<512, 2>, s.tile_bwd_smem);
            raise_lds((const void*)k_bwd_tile<512, 4>, s.tile_bwd_smem);
            raise_lds((const void*)k_bwd_tile<512, 8>, s.tile_bwd_smem);
        }
        if (s.tile_ok && pre_smem > 48 * 1024) {
            raise_lds((const void*)k_bwd_pre<8>, pre_smem);
            raise_lds((const void*)k_bwd_pre<16>, pre_smem);
        }
        if (s.tile_ok && s.send_bwd_smem > 48 * 1024) raise_lds((const void*)k_send_bwd, s.send_bwd_smem);
        if (s.tile_ok && pre_send_smem > 48 * 1024) {
            raise_lds((const void*)k_bwd_pre_send<8>, pre_send_smem);
            raise_lds((const void*)k_bwd_pre_send<16>, pre_send_smem);
        }
        if (!s.tile_ok) s.rc_fwd = false;
        if (s.rc_fwd && e == hipSuccess)
            s.rc_bwd = tiles <= 64 && tiles * (d.R / 16) <= budget_of((const void*)k_rc_bwd, 256, 0) && !getenv("MMG_NO_RC_BWD") && !no_roles;
        if (s.rc_fwd && e == hipSuccess) {
            s.rc_budget = budget_of((const void*)k_rc_persist, 256, 0);
            // (up to two consecutive launches over tile ranges; beyond that the per-step launches over the whole batch win:
            //  profiles/r04_rc_batch_sweep.log)
            const int ct = s.rc_budget / rc_roles_per_tile(d);
            s.rc_persist = !(d.H & 15) && d.H <= 1024 && tiles <= 15 && ct >= 1 && (tiles + ct - 1) / ct <= 2 && !getenv("MMG_NO_RC_PERSIST") && !no_roles;
        }
        if (s.tile_ok && s.tile_smem > 48 * 1024 && !s.rc_fwd) {
            raise_lds((const void*)k_conv_tile<256>, s.tile_smem);
            raise_lds((const void*)k_conv_tile<512>, s.tile_smem);
        }
    }
    if (s.mc_ok) {
        // k_conversation_mc's 16 workgroups per tile spin on each other: with the per-XCD mapping a tile's members are 16 of 128
        // consecutive ids, so in-order dispatch needs 128 of them resident (16 with consecutive ids); below that the tile /
        // generic kernels run instead -- never a timed-out wait on a partitioned or masked device
        const int mc_budget = budget_of((const void*)(k_conversation_mc<256, 32, 64, 100, 64>), 512, 0);
        if (mc_budget < 128) s.mc_xcd = 0;
        if (mc_budget < 16) s.mc_ok = false;
        s.mc3_ok = s.mc_ok && !d.use_binary;
        if (s.mc3_ok) {
            raise_lds((const void*)(k_conversation_mc3<256, 32, 64, 100, 64>), mc3_lds_bytes());
            const int b3 = budget_of((const void*)(k_conversation_mc3<256, 32, 64, 100, 64>), 256, mc3_lds_bytes());
            if (b3 < (s.mc_xcd ? 128 : 16)) s.mc3_ok = false;
            // two tiles per workgroup (kernels_mc3p.h): from 512 samples on, where the one-tile kernel needs several rounds of workgroups
            if (s.mc3_ok && s.mc_xcd && mc3p_shape(d.B, d.T, d.D) && !getenv("MMG_NO_MC3P")) {
                raise_lds((const void*)(k_conversation_mc3p<256, 32, 64, 100, 64>), mc3p_lds_bytes(d.T));
                s.mc3p_ok = e == hipSuccess && budget_of((const void*)(k_conversation_mc3p<256, 32, 64, 100, 64>), 256, mc3p_lds_bytes(d.T)) >= 128;
            }
        }
    }
    raise_lds((const void*)(k_conversation_fast3<256, 32, 64, 100, false>), fast3_lds_bytes());
    raise_lds((const void*)(k_conversation_fast3<256, 32, 64, 100, true>), fast3_lds_bytes());
    if (fast_wide_v(d.V)) {
        raise_lds((const void*)(k_conversation_fast3<256, 32, 64, 0, false>), fast3_lds_bytes());
        raise_lds((const void*)(k_conversation_fast3<256, 32, 64, 0, true>), fast3_lds_bytes());
    }
    {
        const bool shape = s.use_fast && s.merge_roles && s.sw_merge_prep && s.sw_merge_bas && d.H == 256 && d.W == 32 && d.R == 64 && d.V == 100 &&
                           d.D <= 32 && d.T <= 15 && d.B <= 64 && d.use_binary && !d.fixed && (d.K + 63) / 64 <= 8 && d.K <= 512 &&
                           !(s.tile_ok && s.tile_force) && s.prep_cpb == 1 && s.prep_smem <= game_lds_bytes() && !getenv("MMG_NO_GAME") && !no_roles;
        if (shape && e == hipSuccess) {
            const void* fn = (const void*)game_fast_fn(d.D);
            raise_lds(fn, game_lds_bytes());
            if (e == hipSuccess) {
                // every spinning role must be resident together with the sample roles (the sample roles wait for the statistics roles,
                // those for the baseline roles): B + n_stats + n_bas + D workgroups inside the co-residency budget of this device
                const int budget = budget_of(fn, 256, game_lds_bytes());
                const int npb_ = (d.K + 63) / 64;
                s.game_bas_ub = !(npb_ & 1) ? 2 : 1;
                const int n_stats = stat_roles(d.T), per = 2 * npb_ / s.game_bas_ub;
                int nb = ((budget - d.B - n_stats - d.D) / per) * per;
                const int want = ((d.T * d.B + 15) / 16) * per;
                if (nb > want) nb = want;
                if (nb >= per && prep_blocks(d, s.prep_cpb, true) + d.B <= n_cu) { s.game_ok = true; s.game_nbas = nb; }
            }
        }
    }
#ifdef MMG_DEBUG_CREATE                                  // (compile with -DMMG_DEBUG_CREATE: what select_paths decided)
    fprintf(stderr, "mmg_create: game_ok %d game_nbas %d\n", (int)s.game_ok, s.game_nbas);
    fprintf(stderr, "mmg_create: tile_ok %d tile_nt %d tile_smem %d tile_ext %d tile_persist %d persist_smem %d resident_budget %d tile_bwd_smem %d bwd_pre %d send_bwd %d split %d mc %d fast %d rc %d rc_persist %d rc_budget %d rc_bwd %d\n",
            (int)s.tile_ok, s.tile_nt, s.tile_smem, (int)s.tile_ext, (int)s.tile_persist, s.persist_smem, s.resident_budget, s.tile_bwd_smem,
            bwd_pre_lds_floats(d) * 4, s.send_bwd_smem, (int)s.tile_split, (int)s.mc_ok, (int)s.use_fast, (int)s.rc_fwd, (int)s.rc_persist, s.rc_budget, (int)s.rc_bwd);
#endif
    if (s.conv_smem > 48 * 1024) {
        raise_lds((const void*)k_conversation<256>, s.conv_smem);
        raise_lds((const void*)k_conversation<512>, s.conv_smem);
    }
    if (s.bwd_smem > 48 * 1024) {
        raise_lds((const void*)k_bwd_conv<false>, s.bwd_smem);
        raise_lds((const void*)k_bwd_conv<true>, s.bwd_smem);
    }
    if (e != hipSuccess) return fail("device init failed: %s", hipGetErrorString(e));
    if (plan_jobs(h, tile_path(h) ? CODE_BIAS_TILE : fast_shape(h) ? CODE_BIAS_FAST : CODE_BIAS_GENERIC)) return -1;
    {
        // the optimizer inside k_wgrad: its blocks spin on the norm role of the same launch, so ALL of them must be resident together
        int nb = 0;
        s.wgrad_opt_ok = !s.any_split && d.use_binary && h->d_err != nullptr && !getenv("MMG_NO_WGRAD_OPT") && !no_roles &&
                         hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_wgrad<true>, MMG_BLOCK, 0) == hipSuccess &&
                         h->jt.n_wblocks + 5 <= nb * n_cu - 8;
        int nb2 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, (const void*)k_wgrad<false>, MMG_BLOCK, 0) == hipSuccess) {
            const int others = h->jt.n_wblocks + 1 - h->jt.gemm_tiles;
            const int slots = ((nb2 * n_cu - others) / 8) * 8;
            // (measured, round 5: 1 336 tiles on 856 slots 289 -> 281 us per minibatch, 3 848 on 672 219 -> 217; 5 120 on 552 388 -> 396 --
            //  beyond ~6 tiles per workgroup the static split loses more to its ragged last round than the walk saves;
            //  a balanced stride (tiles / rounds) gave the gain away again: as many workgroups as are resident)
            if (h->jt.gemm_tiles > slots && slots >= 64 && h->jt.gemm_tiles <= 6 * slots) s.wgrad_stride = slots;
        }
#ifdef MMG_DEBUG_CREATE
        fprintf(stderr, "mmg_create: wgrad_stride %d (gemm tiles %d)\n", s.wgrad_stride, h->jt.gemm_tiles);
        fprintf(stderr, "mmg_create: wgrad_opt_ok %d (blocks %d, resident %d x %d)\n", (int)s.wgrad_opt_ok, h->jt.n_wblocks + 5, nb, n_cu);
#endif
    }
    if (no_roles) {
        // nothing that spins on another workgroup of its own launch: per-step / per-phase launches only
        //   (MMG_NO_MERGE + MMG_NO_MERGE_PREP + MMG_NO_GAME + MMG_NO_WGRAD_OPT + MMG_NO_PERSIST + MMG_NO_SPLIT + MMG_NO_MC + MMG_NO_RC_PERSIST + MMG_NO_RC_BWD)
        if (s.game_ok || s.wgrad_opt_ok || s.tile_persist || s.tile_split || s.mc_ok || s.rc_persist || s.rc_bwd || s.merge_roles || s.sw_merge_prep)
            return fail("internal: a role launch survived the no-roles selection");
    }
    return 0;
}
