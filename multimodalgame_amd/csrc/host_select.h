// host_select.h -- host side of mmg.hip: select_paths decides, once per handle (and again for the no-roles fall-back), which kernels serve its shape
// on this device: capability flags and budgets, then the family (select_family) and the launch plan (plan_launches: every launch of a minibatch with
// its variant and grid).  The decision is a pure function of the config, the environment switches, the handle's flags and a dozen numbers the device
// reports (shape_pass, decide); read_switches and probe_device fetch those inputs and hold every access to the environment and to the runtime.
// plan_text prints the result (mmg_plan_text; mmg_plan_for: the same for caller-supplied device numbers, no GPU needed).  Included by mmg.hip only.
#pragma once

// ---------------------------------------------------------------------------------------------
// Launch geometry: role / tile counts that select_paths proves co-resident and the plan hands to the launches as their grids.  (The kernels
// find their roles from the counts they are handed; what they compute themselves stays in the kernel headers.)
// ---------------------------------------------------------------------------------------------
inline int sample_tiles(int B) { return (B + MMG_TM - 1) / MMG_TM; }
inline int stat_roles(int T) { return (5 * T + 2 + 3) / 4; }          // statistics roles: one (stream, step) pair per wave
inline int bas_roles(const Dims& d) { return ((d.T * d.B + 15) / 16) * 2 * ((d.K + 63) / 64); }     // baseline roles: 16 live rows x 64 hidden units each
inline int basehx_tiles(const Dims& d) { return ((d.B + 15) / 16) * ((d.K + 15) / 16); }
// roles per sample tile of the wide receiver's one-launch conversation (k_rc_persist)
inline int rc_roles_per_tile(const Dims& d) {
    const int nj = d.R / 16, njw = d.W / 16;
    return (nj > njw ? nj : njw) + njw + (d.H + 63) / 64 + 1;
}

// continuous many-class family: the two-launch backward of kernels_mc.h
static bool mc_bwd(const mmg_handle* h) { return h->sel.family == FAM_MC && !h->dm.use_binary; }
// single-GPU minibatch: the statistics run as extra roles of the backward launch (no all-reduce in between)
static bool merge_stats(const mmg_handle* h) {
    if (mc_bwd(h)) return h->sel.merge_roles;            // (sum of rewards / hits only: one extra workgroup of k_bwd_mc2)
    return h->sel.family == FAM_FAST && h->dm.use_binary && h->fwd.scores_in_parts && h->sel.merge_roles;
}

// The family.  FAM_FAST (fast_shape): register-resident kernels exist for the agent shape of BASELINE configs 1-3.  Every other shape: sample tiles on
// the matrix cores (kernels_tile.h); the per-sample generic kernels remain for dimensions whose tile does not fit the LDS and for the agent-level entry
// points.  The small agents with many classes (32 < D <= 1024): register-resident conversation with class slices (kernels_mc.h) up to 2 048 samples per
// GPU (measured at D = 1000: 2 048 samples 1 064 us per minibatch against 1 113 on the sample tiles, 4 096 samples 2 090 against 1 242 -- from 256 tiles
// on, the tiles fill the chip and a workgroup per sample is 16 waves of it; MMG_TILE=1 forces the tiles)
static Family select_family(const Selection& s, const Dims& d) {
    const bool forced = s.tile_ok && s.tile_force;
    // (D = 30: own instantiation, other D <= 32: capacity 32; V = 100 likewise, other V % 4 == 0: at run time)
    const bool fast = !forced && s.use_fast && !s.noise && d.H == 256 && d.W == 32 && d.R == 64 && (d.V == 100 || fast_wide_v(d.V)) && d.D <= 32 && d.T <= 16;
    const bool mc = s.mc_ok && !forced && (d.B <= 2048 || !s.tile_ok);
    return (s.tile_ok && !fast && !mc) ? FAM_TILE : mc ? FAM_MC : fast ? FAM_FAST : FAM_GENERIC;
}

// The launch plan (host_launch.h: LaunchPlan): which launches a minibatch of this handle enqueues and at what grid.  Everything here depends on
// Dims, the switches and the budgets select_paths has just measured -- nothing on a call's arguments.
static void plan_launches(mmg_handle* h) {
    const Dims& d = h->dm;
    Selection& s = h->sel;
    LaunchPlan& p = s.plan;
    const Family fam = s.family;
    const int tiles = sample_tiles(d.B), TB = d.T * d.B;
    p.tiles = tiles;
    p.n_stats = stat_roles(d.T);
    p.n_bas = bas_roles(d);
    p.basehx_tiles = basehx_tiles(d);
    p.nprep_hx = prep_blocks(d, s.prep_cpb, true);
    // ---- forward, sample tiles (the order of the outcomes is the fall-through order) ----
    p.conv_tile_fn = s.tile_nt == 512 ? k_conv_tile<512> : k_conv_tile<256>;
    p.skip_ok = !d.fixed;
    p.s1_grid = tiles * ((d.H + 15) / 16);
    p.s2_grid = tiles * ((d.W + 15) / 16);
    p.rc_nj = d.R / 16;
    p.rc_njw = d.W / 16;
    // all roles of a launch must be co-resident (`budget` workgroups, occupancy query above): as many whole tiles per launch
    // as fit, the batch in consecutive launches (the conversations of different samples are independent)
    auto chunks = [&](int per_tile, int budget) {
        const int ct = budget / per_tile > 1 ? budget / per_tile : 1;
        p.chunk_roles = per_tile;
        p.n_chunk = (tiles + ct - 1) / ct;
        p.chunk_tiles = (tiles + p.n_chunk - 1) / p.n_chunk;
        p.basehx_rides = p.n_chunk == 1 && d.use_binary && d.B <= 64 && !(d.H & 3) && s.merge_roles;   // training minibatches of <= 64 samples
    };
    if (s.tile_split) p.tile_fwd = TF_SPLIT;
    else if (!s.tile_ext) p.tile_fwd = TF_WHOLE;
    else {
        p.tile_fwd = !s.rc_fwd ? TF_STEP : s.rc_persist ? TF_RC_PERSIST : TF_RC_STEP;
        if (s.tile_persist) {
            p.ns1 = s.persist_ns1;
            p.ns2 = s.persist_ns2;
            // receiver shape of the register-resident kernels: one receiver role per SAMPLE (rs_role) beside the tiles' sender roles
            int rs = s.rs_capable ? 1 : 0;
            if (rs && d.W == 256 && s.sw_rmsg) rs = 2;          // ... which also form the receiver's message
            if (rs == 2 && d.H % 64 == 0 && d.H / 64 <= 16 && s.sw_fused_s) { rs = 3; p.ns1 = d.H / 64; p.ns2 = d.W / 16; }   // fused sender roles (sa_role / sb_role)
            const int per_tile = MMG_TM + p.ns1 + p.ns2, ct = s.resident_budget / per_tile > 1 ? s.resident_budget / per_tile : 1;
            // (measured with config 4's agents: 256 samples in 4 launches 471 us against 858 us as per-step launches; 1024 samples
            //  in 13 launches 1 723 against 1 544 -- beyond six launches the per-step GEMM launches over the whole batch win)
            if (rs && (tiles + ct - 1) / ct <= 6 && per_tile <= s.resident_budget) {
                p.tile_fwd = TF_PERSIST_SAMPLE;
                p.rsample = rs;
                p.persist_fn = (rs == 3 && s.persist_ll) ? k_conv_persist<512, true, true> : k_conv_persist<512, true>;
                chunks(per_tile, s.resident_budget);
            } else if (!rs && tiles * (1 + p.ns1 + p.ns2) <= s.resident_budget) {
                p.tile_fwd = TF_PERSIST_TILE;
                p.persist_fn = k_conv_persist<512, false>;
                p.chunk_roles = 1 + p.ns1 + p.ns2;
            }
        }
        // wide receiver, all roles co-resident: one launch for the whole conversation (kernels_rc.h: k_rc_persist)
        if (p.tile_fwd == TF_RC_PERSIST) chunks(rc_roles_per_tile(d), s.rc_budget);
    }
    {   // ---- forward, many classes ----
        const int ntile = p.mc_ntile = (d.B + 15) / 16, per16 = s.n_cu / 16 > 0 ? s.n_cu / 16 : 1, per128 = s.n_cu / 128 > 0 ? s.n_cu / 128 : 1;
        p.mc_grid = s.mc_xcd ? ((ntile + 7) / 8) * 128 : ntile * 16;     // (mc_xcd assumes the 8 XCDs of an unpartitioned MI355X; select_paths clears it otherwise)
        // the pair kernel (kernels_mc3p.h) when it needs fewer rounds: a round of 16 pairs takes ~1.55x a round of 16 single tiles (measured,
        // scripts/mc3p_ab.py: 768 samples = 24 pairs = two rounds lose to three rounds of single tiles, every other multiple of 256 from 512 on wins)
        const int npair = (ntile + 1) / 2, mc3p_rounds = (npair + s.n_cu / 16 - 1) / per16, mc3_rounds = (ntile * 16 + s.n_cu - 1) / s.n_cu;
        p.mc3p_wins = s.mc3_ok && s.mc3p_ok && 31 * mc3p_rounds < 20 * mc3_rounds;
        // 128 consecutive workgroups = 8 pairs of tiles x 16 members; one workgroup per CU: the launch is persistent
        p.mc3p_grid = 128 * ((npair + 7) / 8 > s.n_cu / 128 ? per128 : (npair + 7) / 8);
    }
    // ---- forward, register-resident / generic ----
    // k_prep's blocks run as leading roles of k_conversation_fast3's launch -- when every prep and sample role has a CU of its own
    // (the launch holds ONE workgroup per CU: with 512 samples the 531 prep roles would be two more rounds of workgroups ahead of
    // the conversations: 318 us per minibatch against 306 with k_prep as its own launch)
    p.merge_prep = s.sw_merge_prep && fam == FAM_FAST && s.prep_smem <= fast3_lds_bytes() && p.nprep_hx + d.B <= s.n_cu;
    p.fwd_basehx = fam == FAM_FAST && d.use_binary && s.merge_roles;
    const bool wide = fam == FAM_FAST && d.V != 100;
    p.fast_fn = wide ? (p.merge_prep ? k_conversation_fast3<256, 32, 64, 0, true> : k_conversation_fast3<256, 32, 64, 0, false>)
                     : (p.merge_prep ? k_conversation_fast3<256, 32, 64, 100, true> : k_conversation_fast3<256, 32, 64, 100, false>);
    p.fast_smem = fast3_lds_bytes();
    p.conv_fn = s.conv_threads == 512 ? k_conversation<512> : k_conversation<256>;
    p.agent_fn = k_conversation<256>;
    if (s.flip) {                                // message flips: the FLIP instantiations (select_paths has cleared every other conversation kernel)
        p.fast_fn = wide ? (p.merge_prep ? k_conversation_fast3<256, 32, 64, 0, true, true> : k_conversation_fast3<256, 32, 64, 0, false, true>)
                         : (p.merge_prep ? k_conversation_fast3<256, 32, 64, 100, true, true> : k_conversation_fast3<256, 32, 64, 100, false, true>);
        p.fast_smem = fast3_flip_lds_bytes();
        p.conv_fn = s.conv_threads == 512 ? k_conversation<512, true> : k_conversation<256, true>;
        p.agent_fn = k_conversation<256, true>;
    }
    if (s.attn) {                                // description attention: the ATTN instantiations (shape_pass has cleared every other family)
        p.conv_attn_fn = s.conv_threads == 512 ? k_conversation_attn<512> : k_conversation_attn<256>;
        p.agent_attn_fn = k_conversation_attn<256>;
    }
    if (s.vattn) {                               // visual attention: the VATTN instantiations (shape_pass has cleared every other family)
        p.conv_vattn_fn = s.conv_threads == 512 ? k_conversation_vattn<512> : k_conversation_vattn<256>;
        p.agent_vattn_fn = k_conversation_vattn<256>;
    }
    if (s.variant) {                             // a sender variant: the VAR instantiations (shape_pass has cleared every other conversation kernel)
        p.conv_fn = s.conv_threads == 512 ? k_conversation<512, false, true> : k_conversation<256, false, true>;
        p.agent_fn = k_conversation<256, false, true>;
    }
    if (s.relax) {                               // relaxed messages: the RELAX instantiations (shape_pass has cleared every other conversation kernel)
        p.conv_fn = s.conv_threads == 512 ? k_conversation<512, false, false, true> : k_conversation<256, false, false, true>;
        p.agent_fn = k_conversation<256, false, false, true>;
    }
    if (s.noise) {                               // Gaussian message noise: the NOISE instantiations (shape_pass has cleared every other conversation kernel but mc3)
        p.conv_fn = s.conv_threads == 512 ? k_conversation_noise<512> : k_conversation_noise<256>;
        p.agent_fn = k_conversation_noise<256>;
    }
    p.conv_name = s.vattn ? "k_conversation_vattn" : s.noise ? "k_conversation_noise" : wide ? "k_conversation_wv" : "k_conversation";     // (the profiling scope says which sender ran)
    p.bwd_name = wide ? "k_bwd_conv_wv" : "k_bwd_conv";
    // ---- baselines (training minibatch that did not run all rows) ----
    // Fused step: the baselines' live-row pass (k_baselines3's body) as workgroup roles of the backward launch, beside the sample
    // roles' statistics-independent prologue (kernels_fast.h) -- one launch less.  (The sample and statistics roles of that launch
    // sit ahead of these producers and spin: only with CUs to spare.  Adaptive conversations only: Fixed mode keeps all 640 rows
    // live and the backward kernel holds ONE workgroup per CU -- measured at config 3: 101.3 us per minibatch with the roles
    // against 94.6 with k_baselines3 as its own launch; config 2: 66.0 against 72.1.)  Phased step: as roles of mmg_loss_stats'
    // launch, beside the statistics roles that consume their scores (k_bas_stats) -- one launch less before the statistics all-reduce
    const bool bas_roles_ok = p.fwd_basehx && d.B <= 64 && (d.K + 63) / 64 <= 8 && s.sw_merge_bas;
    p.bas_defer_ok = bas_roles_ok && !d.fixed && s.n_cu >= 2 * (d.B + p.n_stats);
    p.bas_pending_ok = bas_roles_ok && s.n_cu >= 2 * p.n_stats;
    // any message / state width on the tiles: basehx as a GEMM launch, then one MFMA pass over the live rows (kernels_tile.h); register-resident agents:
    // k_baselines3 over the live (step, sample) rows; else every row (grid.z = 2 baselines x 2 step ranges: 128 workgroups at config 1 instead of 64)
    p.bas_kernel = (fam == FAM_TILE && d.B <= 64 && !(d.H & 3)) ? BAS_TILE4 : (p.fwd_basehx && d.B <= 64) ? BAS_LIVE3 : BAS_ALL2;
    p.bas2_z = 2 * (d.T >= 4 ? 2 : 1);
    // ---- backward ----
    p.n_rowblk = sample_tiles(TB);
    p.n_hbands = (d.H + 63) / 64;
    p.dhx_blk = (d.B * (d.H / 4) + MMG_BLOCK - 1) / MMG_BLOCK;
    p.dhx_grid = p.dhx_blk + (d.H / 4 + 63) / 64;
    if (fam == FAM_TILE) {
        p.row_map = TB <= 2048;   // k_wgrad keeps the live-row list in LDS (2048 entries)
        p.zero_dead = !p.row_map && !d.fixed;
        // the sender's backward rides in the same launch as k_bwd_pre (independent latency chains side by side) while the row
        // blocks are few: it then walks all T * B rows instead of the live-row list (MMG_NO_MERGE=1: separate launches)
        p.merged_send = d.use_binary && s.merge_roles && TB <= 2048;
        const bool rc = s.rc_fwd && s.rc_bwd;
        // wide receiver whose reverse-time loop runs as roles (k_rc_bwd adds the partials): four column bands per (step, tile)
        p.pre_bands = (p.merged_send && rc && d.R == 256) ? 4 : 1;
        p.n_pre = d.T * tiles * p.pre_bands;
        p.pre_smem = bwd_pre_lds_floats(d) * 4;
        if (p.merged_send && s.send_bwd_smem > p.pre_smem) p.pre_smem = s.send_bwd_smem;
        if (p.merged_send) p.pre_send_fn = d.R <= 128 ? k_bwd_pre_send<8> : k_bwd_pre_send<16>;
        else if (d.use_binary) p.pre_fn = d.R <= 128 ? k_bwd_pre<8> : k_bwd_pre<16>;
        // receiver shape of the register-resident kernels: one workgroup per sample; else the tile's recurrence with 2 / 4 / 8
        // tape registers per thread, or the wide receiver's reverse-time loop as roles over 16-unit slices (kernels_rc.h)
        p.bwd_rec = s.rs_capable ? BR_SAMPLE : (d.R > 128 && rc) ? BR_RC : BR_TILE;
        p.bwd_tile_fn = d.R <= 64 ? k_bwd_tile<512, 2> : d.R <= 128 ? k_bwd_tile<512, 4> : k_bwd_tile<512, 8>;
        p.send_own = !p.merged_send;
        p.dhx_own = !(p.bwd_rec == BR_SAMPLE && p.merged_send);     // (k_bwd_sample carries k_dhx's blocks when the sender's backward already ran)
        const int RL = d.R < MMG_BLOCK ? d.R : MMG_BLOCK, CPB = MMG_BLOCK / RL;
        p.dc = DC_TILE;
        p.dc_grid = (d.D + CPB - 1) / CPB;
        p.dc_slices = dc_slices(d.B);
    } else if (mc_bwd(h)) {
        // one sample tile per workgroup up to 16 groups (measured at 256 samples: 4 groups 26 us, 8: 15, 16: 10)
        p.mc_ngroup = p.mc_ntile > 16 ? 16 : p.mc_ntile;
        p.mc_nred = (2 * d.D * d.R / 4 + MMG_BLOCK - 1) / MMG_BLOCK;
    } else {
        const bool fast = fam == FAM_FAST, merge_dc = fast && s.merge_roles;
        p.row_map = merge_dc && TB <= 2048;   // class role 0 lists the live (step, sample) rows for k_wgrad
        p.zero_dead = !p.row_map;
        // k_conversation_fast3 stores softmax rows, not dbar = softmax(y) . desc: trailing workgroups form it (16 rows each); class roles: k_dC's work inside the launch
        p.n_dbar = (fast && d.use_binary) ? (TB + 15) / 16 : 0;
        p.n_class = merge_dc ? d.D : 0;
        if (fast) {
            p.bwd_fast_stats_fn = bwd_conv_fast_fn<true, true>(d.D, d.V);
            p.bwd_fast_fn = merge_dc ? bwd_conv_fast_fn<false, true>(d.D, d.V) : bwd_conv_fast_fn<false, false>(d.D, d.V);
        }
        p.bwd_conv_fn = d.B > 512 ? k_bwd_conv<true> : k_bwd_conv<false>;
        // (a sender variant: the reverse step of tanh(h_x) / tanh(h_x * h_w); ignore_receiver alone needs none -- the tape holds the zeros)
        if (s.variant & SV_IGNORE_CODE) p.bwd_conv_fn = d.B > 512 ? k_bwd_conv<true, SV_IGNORE_CODE> : k_bwd_conv<false, SV_IGNORE_CODE>;
        else if (s.variant & SV_PROD) p.bwd_conv_fn = d.B > 512 ? k_bwd_conv<true, SV_PROD> : k_bwd_conv<false, SV_PROD>;
        p.dc = (merge_dc || s.attn) ? DC_NONE : DC_PLAIN;     // (attention: k_attn_dE forms Py2 beside dE, y1.bias comes from dA)
    }
}

// ---------------------------------------------------------------------------------------------
// Path selection: which kernels serve this handle's shape on this device.  Runs at mmg_create, when mmg_set_message_flipout / mmg_set_sender_variant / mmg_set_message_relaxation / mmg_set_message_noise change the
// routing, and again when the library falls back to launches WITHOUT in-launch waits (h->no_roles: after a timed-out dependency, for a CU
// budget / CU mask that cannot hold the role launches, or MMG_NO_ROLES=1).  Four steps, in this order:
//   read_switches   the environment, once per selection -- never on the per-minibatch path, and nowhere else in the library
//   shape_pass      pure: LDS sizes, thread counts, every decision the shape and the switches settle alone, and which occupancies are needed (ask)
//   probe_device    the only code that talks to the HIP runtime: CU count, the LDS raises, one occupancy per role kernel that was asked for (caps)
//   decide          pure: budgets from the caps, capability flags, family, job table, k_wgrad's walk, launch plan, the no-roles invariant
// mmg_plan_for runs the two pure passes on caller-supplied caps; plan_text prints what a selection decided.
// ---------------------------------------------------------------------------------------------
enum Switch { SW_NO_FAST, SW_NO_MERGE, SW_NO_MERGE_PREP, SW_NO_PERSIST_LL, SW_NO_RSAMPLE, SW_NO_RMSG, SW_NO_FUSED_S, SW_NO_MC, SW_NO_RC, SW_NO_TILE,
              SW_TILE, SW_NO_SPLIT, SW_NO_PERSIST, SW_NO_RC_BWD, SW_NO_RC_PERSIST, SW_NO_MC3P, SW_NO_GAME, SW_NO_WGRAD_OPT, SW_NO_ROLES,
              SW_HSA_CU_MASK, SW_ROC_GLOBAL_CU_MASK, SW_COUNT };
struct Switches {
    bool set[SW_COUNT];
    bool operator[](Switch k) const { return set[k]; }
    // a process whose compute units are masked still sees the whole chip in the device properties: the occupancy budgets would promise
    // co-residency the dispatcher cannot deliver
    bool roles_off() const { return set[SW_NO_ROLES] || set[SW_HSA_CU_MASK] || set[SW_ROC_GLOBAL_CU_MASK]; }
};
static Switches read_switches() {
    static const char* const name[SW_COUNT] = {
        "MMG_NO_FAST", "MMG_NO_MERGE", "MMG_NO_MERGE_PREP", "MMG_NO_PERSIST_LL", "MMG_NO_RSAMPLE", "MMG_NO_RMSG", "MMG_NO_FUSED_S", "MMG_NO_MC", "MMG_NO_RC",
        "MMG_NO_TILE", "MMG_TILE", "MMG_NO_SPLIT", "MMG_NO_PERSIST", "MMG_NO_RC_BWD", "MMG_NO_RC_PERSIST", "MMG_NO_MC3P", "MMG_NO_GAME", "MMG_NO_WGRAD_OPT",
        "MMG_NO_ROLES", "HSA_CU_MASK", "ROC_GLOBAL_CU_MASK"};
    Switches w;
    for (int k = 0; k < SW_COUNT; ++k) w.set[k] = getenv(name[k]) != nullptr;
    return w;
}

// Pure.  Everything Dims, the switches and the handle's flags (no_roles; flips: message flips are set; variant: the SV_* bits of
// mmg_set_sender_variant; relax: relaxed messages are set; noise: Gaussian message noise is set; err_word: the pinned error word exists)
// settle alone.  A capability that also needs a co-residency budget (tile_split, tile_persist, mc_ok) leaves here as a CANDIDATE: its
// preconditions hold and s.ask names the occupancy it waits for; decide() confirms or clears it.
static int shape_pass(const mmg_config& cfg, const Dims& d, const Switches& w, bool no_roles, bool flips, int variant, bool relax, bool noise, bool err_word,
                      Selection& s, int attn_dim = 0, int n_words = 0, VattnDims vd = VattnDims()) {
    s = Selection();
    // visual attention: the generic per-sample family with the sender's VATTN instantiation; every other family is cleared below
    s.vattn = vd.A > 0;
    if (s.vattn && (flips || variant || attn_dim > 0)) return fail("visual attention with message flips, a sender variant or description attention");
    // description attention: the generic per-sample family in its ATTN instantiations; every other family is cleared below (use_fast, tile_ok)
    s.attn = attn_dim > 0;
    if (s.attn && (flips || variant)) return fail("desc_attn with message flips or a sender variant");
    // message flips on binary messages (continuous ones are not flipped: the setting is kept and nothing happens)
    s.flip = flips && d.use_binary;
    // a sender variant (ignore_receiver on binary messages only, like the flips): the generic per-sample kernels form it -- the register-resident
    // family with the one-launch step, the many-class kernels, the sample tiles and the wide receiver do not, so all of them are cleared here
    s.variant = variant & (d.use_binary ? (SV_PROD | SV_IGNORE_CODE | SV_IGNORE_REC) : (SV_PROD | SV_IGNORE_CODE));
    if (s.variant && s.flip) return fail("message flips and a sender variant on one handle");
    // relaxed messages (binary only): the generic per-sample kernels form them, so like a variant the setting clears the register-resident,
    // many-class, sample-tile and wide-receiver conversations
    s.relax = relax && d.use_binary;
    if (s.relax && (s.flip || s.variant || s.attn || s.vattn)) return fail("relaxed messages with message flips, a sender variant or attention");
    // Gaussian noise on continuous messages (binary ones take none: the setter refuses them): k_conversation_noise forms it and, for the small
    // agents with many classes, k_conversation_mc3_noise -- the register-resident conversation, the sample tiles, the wide receiver and the pair
    // kernel (mc3p) do not, so they are cleared below and in select_family; mc stays a candidate and decide() keeps it only with mc3
    s.noise = noise && !d.use_binary;
    if (s.noise && (s.variant || s.attn || s.vattn)) return fail("message noise with a sender variant or attention");
    s.use_fast = !w[SW_NO_FAST] && !s.variant && !s.relax && !s.attn && !s.vattn; s.merge_roles = !w[SW_NO_MERGE] && !no_roles;
    s.sw_merge_prep = !w[SW_NO_MERGE_PREP] && !no_roles;
    s.sw_merge_bas = s.merge_roles;
    s.persist_ll = !w[SW_NO_PERSIST_LL] && persist_ll_shape(cfg.batch, cfg.h_dim, cfg.w_dim, cfg.rec_hidden, cfg.wv_dim, cfg.n_classes, cfg.max_exchange);
    s.sw_rsample = !w[SW_NO_RSAMPLE]; s.sw_rmsg = !w[SW_NO_RMSG]; s.sw_fused_s = !w[SW_NO_FUSED_S];
    s.mc_ok = s.use_fast && mc_shape(d.H, d.W, d.R, d.V, d.D, d.T) && !w[SW_NO_MC] && !no_roles && !s.flip;
    s.mc_per = (((d.D + 15) / 16) + 3) & ~3;
    s.mc_xcd = 1;                                   // a tile's 16 workgroups on one XCD (measured at config 5, 256 samples: 192 us per minibatch against 201); cleared by decide() on a device without room for it
    // few samples and large sender matrices or class tables: 512-thread variant of the generic conversation kernel
    s.conv_threads = (d.B <= 256 && ((int64_t)d.H * d.W >= 65536 || (int64_t)d.D * (d.R + d.V) >= 65536)) ? 512 : 256;
    s.conv_smem = conv_smem_floats(d, s.conv_threads) * 4;
    s.conv_smem_agent = conv_smem_floats(d, MMG_BLOCK) * 4;
    s.bwd_smem = bwd_smem_floats(d, (s.variant & (SV_PROD | SV_IGNORE_CODE)) == SV_PROD) * 4;
    if (s.attn) {
        s.conv_smem = conv_attn_smem_floats(d, s.conv_threads, attn_dim, n_words) * 4;
        s.conv_smem_agent = conv_attn_smem_floats(d, MMG_BLOCK, attn_dim, n_words) * 4;
        s.bwd_smem = bwd_attn_smem_floats(d, attn_dim, n_words) * 4;
    }
    if (s.vattn) {
        s.conv_smem = conv_vattn_smem_floats(d, s.conv_threads, vd.A, vd.N) * 4;
        s.conv_smem_agent = conv_vattn_smem_floats(d, MMG_BLOCK, vd.A, vd.N) * 4;
        s.vattn_bwd_smem = vattn_bwd_smem_floats(d, vd.A, vd.N) * 4;
    }
    s.prep_smem = ((d.V > d.W ? d.V : d.W) + 16) * 4;
    // hundreds of classes: 8 per class block of k_prep (weight rows in registers across them); few classes: one per block (latency)
    s.prep_cpb = (d.D >= 256 && d.R <= 64 && d.V <= 128 && !(d.V & 3) && 2 * d.R <= MMG_BLOCK) ? 2 : 1;
    if (s.prep_cpb > 1 && (int)(s.prep_cpb * (d.V + d.R) * 4) > s.prep_smem) s.prep_smem = s.prep_cpb * (d.V + d.R) * 4;
    if (s.conv_smem > 160 * 1024 || s.bwd_smem > 160 * 1024 || s.vattn_bwd_smem > 160 * 1024) return fail("dimensions need more than 160 KB of LDS per sample");
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
    s.rc_fwd = aligned && s.tile_ext && s.tile_smem > 160 * 1024 && rc_shape(d.B, d.H, d.W, d.R, d.V, d.D) && !w[SW_NO_RC];
    // (the sample tiles keep a [16, V] mixture tile and V-wide split-K staging in LDS: audited and tested up to V = 256, the
    //  limit before MMG_MAX_WV; wider descriptions take the register-resident small agents or the per-sample kernels)
    // (message flips: k_conversation_fast3 and k_conversation form them, the sample tiles and the wide receiver do not)
    s.tile_ok = aligned && d.V <= 256 && (s.tile_smem <= 160 * 1024 || s.rc_fwd) && !w[SW_NO_TILE] && !s.flip && !s.variant && !s.relax && !s.attn && !s.vattn && !s.noise;
    s.tile_force = w[SW_TILE];
    // many classes, small agents, fewer than 64 tiles: a workgroup per SAMPLE fills the chip (256 samples = 256 CUs) and
    // beats 16 tiles + class helpers (measured at D = 1000, B = 256: 557 us against 1 010 us per minibatch; B = 2048:
    // 2 091 against 1 189) -- the tile kernels take over from 1024 samples (MMG_TILE=1: always)
    if (s.tile_ok && !s.tile_force && !s.tile_ext && d.D * MMG_TM > 8 * 512 && d.B < 1024) s.tile_ok = false;
    // many classes and fewer sample tiles than CUs: class helpers (k_conv_split)
    s.split_nh = split_helpers(d.B);
    s.split_per = (((d.D + s.split_nh) / (s.split_nh + 1)) + 3) & ~3;
    s.tile_split = s.tile_ok && !s.tile_ext && d.D * MMG_TM > 8 * 512 && s.split_nh >= 1 && tiles * (1 + s.split_nh) <= 224 && !w[SW_NO_SPLIT] && !no_roles;
    if (s.tile_split) {
        const int a = tile_lds(d, 512 / 64, true, s.split_per).total * 4, b = helper_lds(d, 512 / 64, s.split_per).total * 4;
        s.split_smem = a > b ? a : b;
        if (s.split_smem > 160 * 1024) s.tile_split = false;
    }
    // per-step sender products as ROLES of one persistent launch when all of them fit on the chip together
    s.persist_ns1 = d.H / 64; s.persist_ns2 = d.W / 32;
    // (receiver shape of the register-resident kernels: per-sample receiver roles, and batches too large for one launch of
    //  co-resident roles run as consecutive launches over sample ranges)
    s.rs_capable = d.R == 64 && d.V == 100 && d.D <= 32 && d.T <= 16 && s.sw_rsample;
    s.tile_persist = s.tile_ok && s.tile_ext && !(d.H % 64) && !(d.W % 32) && tiles <= 64 && MMG_TM * d.W <= 8 * 512 && !w[SW_NO_PERSIST] && !no_roles;
    if (s.tile_persist) {
        const int a = tile_lds(d, 512 / 64, false).total * 4, b = srole_lds(d, 512 / 64).total * 4;
        s.persist_smem = a > b ? a : b;
        if (s.persist_smem > 160 * 1024) s.tile_persist = false;
    }
    s.tile_bwd_smem = bwd_tile_lds(d, 512 / 64).total * 4;
    s.send_bwd_smem = (MMG_TM * ld16(d.W) + 7 * 64 + 16 + tile_raw_floats_nn(64, MMG_BLOCK / 64)) * 4;
    if (s.tile_bwd_smem > 160 * 1024 || d.W > 256 || d.R > 256) s.tile_ok = false;     // (k_bwd_tile keeps a step's GRU tape in 4 registers per thread per 32 hidden units)
    if (!s.tile_ok) s.rc_fwd = false;
    // the occupancies decide() will read, each under the preconditions of the capability it sizes
    bool* ask = s.ask;
    ask[MMG_CAP_SPLIT] = s.tile_split;
    ask[MMG_CAP_PERSIST] = s.tile_persist;
    ask[MMG_CAP_RC_BWD] = s.rc_fwd && tiles <= 64;
    ask[MMG_CAP_RC_PERSIST] = s.rc_fwd;
    ask[MMG_CAP_MC] = s.mc_ok;
    ask[MMG_CAP_MC3] = s.mc_ok && !d.use_binary;
    // two tiles per workgroup (kernels_mc3p.h): from 512 samples on, where the one-tile kernel needs several rounds of workgroups
    ask[MMG_CAP_MC3P] = ask[MMG_CAP_MC3] && mc3p_shape(d.B, d.T, d.D) && !w[SW_NO_MC3P] && !s.noise;
    // fused step of the small Adaptive agents (kernels_game.h)
    ask[MMG_CAP_GAME] = s.use_fast && s.merge_roles && s.sw_merge_prep && s.sw_merge_bas && d.H == 256 && d.W == 32 && d.R == 64 && d.V == 100 &&
                        d.D <= 32 && d.T <= 15 && d.B <= 64 && d.use_binary && !d.fixed && (d.K + 63) / 64 <= 8 && d.K <= 512 &&
                        !(s.tile_ok && s.tile_force) && s.prep_cpb == 1 && s.prep_smem <= game_lds_bytes() && !w[SW_NO_GAME] && !no_roles && !s.flip;
    // the optimizer inside k_wgrad (decide() also wants a job table without row splits)
    ask[MMG_CAP_WGRAD_OPT] = d.use_binary && err_word && !w[SW_NO_WGRAD_OPT] && !no_roles;
    ask[MMG_CAP_WGRAD] = true;
    return 0;
}

// The device's answers (Selection::caps, indexed by MMG_CAP_*): the CU count and, for every role kernel shape_pass asked about, the workgroups
// of it that one CU holds at its thread count and LDS size (0: the query failed; -1: not asked).  Raises the dynamic LDS limits on the way,
// each before the query that depends on it.
static int probe_device(const mmg_config& cfg, const Dims& d, Selection& s) {
    int n_cu = 0, dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
    if (n_cu <= 0) return fail("cannot query the device (multiProcessorCount)");
    // caller-supplied budget (mmg_config.cu_budget): a process that shares the GPU, or runs under a CU mask, states how many
    // compute units it can count on -- every co-residency budget of decide() is sized from it
    if (cfg.cu_budget > 0 && cfg.cu_budget < n_cu) n_cu = cfg.cu_budget;
    for (int k = 0; k < MMG_PLAN_CAPS; ++k) s.caps[k] = -1;
    s.caps[MMG_CAP_N_CU] = n_cu;
    // raises the dynamic LDS limit of the kernels named after `bytes`; e keeps the first error (reported once, below)
    hipError_t e = hipSuccess;
    auto raise_lds = [&](int bytes, auto... fns) {
        for (const void* fn : {(const void*)fns...}) if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    };
    auto occupancy = [&](int cap, auto fn, int threads, int smem) {
        int nb = 0;
        if (s.ask[cap] && e == hipSuccess)
            s.caps[cap] = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, threads, (size_t)smem) == hipSuccess && nb > 0 ? nb : 0;
    };
    if (s.ask[MMG_CAP_SPLIT]) raise_lds(s.split_smem, k_conv_split<512>);
    occupancy(MMG_CAP_SPLIT, k_conv_split<512>, 512, s.split_smem);
    if (s.ask[MMG_CAP_PERSIST]) raise_lds(s.persist_smem, k_conv_persist<512, true>, k_conv_persist<512, false>, k_conv_persist<512, true, true>);
    if (s.rs_capable) occupancy(MMG_CAP_PERSIST, k_conv_persist<512, true>, 512, s.persist_smem);
    else occupancy(MMG_CAP_PERSIST, k_conv_persist<512, false>, 512, s.persist_smem);
    const int pre_smem = bwd_pre_lds_floats(d) * 4, pre_send_smem = pre_smem > s.send_bwd_smem ? pre_smem : s.send_bwd_smem;
    if (s.tile_ok && s.tile_bwd_smem > 48 * 1024) raise_lds(s.tile_bwd_smem, k_bwd_tile<512, 2>, k_bwd_tile<512, 4>, k_bwd_tile<512, 8>);
    if (s.tile_ok && pre_smem > 48 * 1024) raise_lds(pre_smem, k_bwd_pre<8>, k_bwd_pre<16>);
    if (s.tile_ok && s.send_bwd_smem > 48 * 1024) raise_lds(s.send_bwd_smem, k_send_bwd);
    if (s.tile_ok && pre_send_smem > 48 * 1024) raise_lds(pre_send_smem, k_bwd_pre_send<8>, k_bwd_pre_send<16>);
    occupancy(MMG_CAP_RC_BWD, k_rc_bwd, 256, 0);
    occupancy(MMG_CAP_RC_PERSIST, k_rc_persist, 256, 0);
    if (s.tile_ok && s.tile_smem > 48 * 1024 && !s.rc_fwd) raise_lds(s.tile_smem, k_conv_tile<256>, k_conv_tile<512>);
    occupancy(MMG_CAP_MC, k_conversation_mc<256, 32, 64, 100, 64>, 512, 0);
    if (s.ask[MMG_CAP_MC3]) raise_lds(mc3_lds_bytes(), k_conversation_mc3<256, 32, 64, 100, 64>);
    if (s.ask[MMG_CAP_MC3] && s.noise) raise_lds(mc3_lds_bytes(), k_conversation_mc3_noise<256, 32, 64, 100, 64>);
    occupancy(MMG_CAP_MC3, s.noise ? k_conversation_mc3_noise<256, 32, 64, 100, 64> : k_conversation_mc3<256, 32, 64, 100, 64>, 256, mc3_lds_bytes());
    if (s.ask[MMG_CAP_MC3P]) raise_lds(mc3p_lds_bytes(d.T), k_conversation_mc3p<256, 32, 64, 100, 64>);
    occupancy(MMG_CAP_MC3P, k_conversation_mc3p<256, 32, 64, 100, 64>, 256, mc3p_lds_bytes(d.T));
    raise_lds(fast3_lds_bytes(), k_conversation_fast3<256, 32, 64, 100, false>, k_conversation_fast3<256, 32, 64, 100, true>);
    if (fast_wide_v(d.V)) raise_lds(fast3_lds_bytes(), k_conversation_fast3<256, 32, 64, 0, false>, k_conversation_fast3<256, 32, 64, 0, true>);
    if (s.flip) {
        raise_lds(fast3_flip_lds_bytes(), k_conversation_fast3<256, 32, 64, 100, false, true>, k_conversation_fast3<256, 32, 64, 100, true, true>);
        if (fast_wide_v(d.V)) raise_lds(fast3_flip_lds_bytes(), k_conversation_fast3<256, 32, 64, 0, false, true>, k_conversation_fast3<256, 32, 64, 0, true, true>);
    }
    if (s.ask[MMG_CAP_GAME]) raise_lds(game_lds_bytes(), game_fast_fn(d.D));
    occupancy(MMG_CAP_GAME, game_fast_fn(d.D), 256, game_lds_bytes());
    if (s.conv_smem > 48 * 1024) raise_lds(s.conv_smem, k_conversation<256>, k_conversation<512>);
    if (s.conv_smem > 48 * 1024 && s.flip) raise_lds(s.conv_smem, k_conversation<256, true>, k_conversation<512, true>);
    if (s.conv_smem > 48 * 1024 && s.variant) raise_lds(s.conv_smem, k_conversation<256, false, true>, k_conversation<512, false, true>);
    if (s.conv_smem > 48 * 1024 && s.relax) raise_lds(s.conv_smem, k_conversation<256, false, false, true>, k_conversation<512, false, false, true>);
    if (s.conv_smem > 48 * 1024 && s.noise) raise_lds(s.conv_smem, k_conversation_noise<256>, k_conversation_noise<512>);
    if (s.conv_smem > 48 * 1024 && s.attn) raise_lds(s.conv_smem, k_conversation_attn<256>, k_conversation_attn<512>);
    if (s.bwd_smem > 48 * 1024 && s.attn) raise_lds(s.bwd_smem, k_bwd_conv_attn);
    if (s.conv_smem > 48 * 1024 && s.vattn) raise_lds(s.conv_smem, k_conversation_vattn<256>, k_conversation_vattn<512>);
    if (s.vattn_bwd_smem > 48 * 1024) raise_lds(s.vattn_bwd_smem, k_vattn_bwd);
    if (s.bwd_smem > 48 * 1024) raise_lds(s.bwd_smem, k_bwd_conv<false>, k_bwd_conv<true>);
    if (s.bwd_smem > 48 * 1024 && (s.variant & SV_IGNORE_CODE)) raise_lds(s.bwd_smem, k_bwd_conv<false, SV_IGNORE_CODE>, k_bwd_conv<true, SV_IGNORE_CODE>);
    else if (s.bwd_smem > 48 * 1024 && (s.variant & SV_PROD)) raise_lds(s.bwd_smem, k_bwd_conv<false, SV_PROD>, k_bwd_conv<true, SV_PROD>);
    if (e != hipSuccess) return fail("device init failed: %s", hipGetErrorString(e));
    occupancy(MMG_CAP_WGRAD_OPT, k_wgrad<true>, MMG_BLOCK, 0);
    occupancy(MMG_CAP_WGRAD, k_wgrad<false>, MMG_BLOCK, 0);
    return 0;
}

// Pure.  From shape_pass's candidates and the caps: the co-residency budgets, the capabilities they confirm, the family, the job table,
// k_wgrad's walk, the launch plan.  Reads h->cfg / dm / no_roles / sel and the buffer ADDRESSES the job table is built from; no HIP call.
static int decide(mmg_handle* h, const Switches& w) {
    const Dims& d = h->dm; const bool no_roles = h->no_roles;
    Selection& s = h->sel;
    const int n_cu = s.n_cu = s.caps[MMG_CAP_N_CU], tiles = sample_tiles(d.B);
    // co-resident workgroups a role launch may hold: occupancy of the kernel at its LDS size x compute units, minus a margin
    // of 1/16 of the chip (256 CUs -> 240, the value the role launches were tuned with).  A partitioned device (CPX), a
    // smaller SKU or a masked process simply gets a smaller budget and, where the roles do not fit, the per-step / generic launches.
    auto budget_of = [&](int cap) {
        if (s.caps[cap] < 1) return 0;
        const int total = s.caps[cap] * n_cu;
        return total - (total + 15) / 16;
    };
    if (s.tile_split) {
        s.split_budget = budget_of(MMG_CAP_SPLIT);
        if (tiles * (1 + s.split_nh) > s.split_budget) s.tile_split = false;     // not all co-resident here: k_conv_tile instead
    }
    if (s.tile_persist) {
        s.resident_budget = budget_of(MMG_CAP_PERSIST);
        // tile roles: every tile's roles in one launch; per-sample receiver roles: at least ONE whole tile per launch
        const bool fits = s.rs_capable ? (MMG_TM + d.H / 64 + d.W / 16 <= s.resident_budget || MMG_TM + s.persist_ns1 + s.persist_ns2 <= s.resident_budget)
                                       : tiles * (1 + s.persist_ns1 + s.persist_ns2) <= s.resident_budget;
        if (!fits) s.tile_persist = false;                                       // per-step launches instead (no co-residency needed)
    }
    if (s.rc_fwd) {
        s.rc_bwd = tiles <= 64 && tiles * (d.R / 16) <= budget_of(MMG_CAP_RC_BWD) && !w[SW_NO_RC_BWD] && !no_roles;
        s.rc_budget = budget_of(MMG_CAP_RC_PERSIST);
        // (up to two consecutive launches over tile ranges; beyond that the per-step launches over the whole batch win:
        //  profiles/r04_rc_batch_sweep.log)
        const int ct = s.rc_budget / rc_roles_per_tile(d);
        s.rc_persist = !(d.H & 15) && d.H <= 1024 && tiles <= 15 && ct >= 1 && (tiles + ct - 1) / ct <= 2 && !w[SW_NO_RC_PERSIST] && !no_roles;
    }
    if (s.mc_ok) {
        // k_conversation_mc's 16 workgroups per tile spin on each other: with the per-XCD mapping a tile's members are 16 of 128
        // consecutive ids, so in-order dispatch needs 128 of them resident (16 with consecutive ids); below that the tile /
        // generic kernels run instead -- never a timed-out wait on a partitioned or masked device
        const int mc_budget = budget_of(MMG_CAP_MC);
        if (mc_budget < 128) s.mc_xcd = 0;
        if (mc_budget < 16) s.mc_ok = false;
        s.mc3_ok = s.mc_ok && !d.use_binary && budget_of(MMG_CAP_MC3) >= (s.mc_xcd ? 128 : 16);
        s.mc3p_ok = s.mc3_ok && s.mc_xcd && s.ask[MMG_CAP_MC3P] && budget_of(MMG_CAP_MC3P) >= 128;
        if (s.noise && !s.mc3_ok) s.mc_ok = false;       // (k_conversation_mc forms no noise: the generic family instead)
    }
    if (s.ask[MMG_CAP_GAME]) {
        // every spinning role must be resident together with the sample roles (the sample roles wait for the statistics roles,
        // those for the baseline roles): B + n_stats + n_bas + D workgroups inside the co-residency budget of this device
        const int budget = budget_of(MMG_CAP_GAME);
        const int npb_ = (d.K + 63) / 64;
        s.game_bas_ub = !(npb_ & 1) ? 2 : 1;
        const int n_stats = stat_roles(d.T), per = 2 * npb_ / s.game_bas_ub;
        int nb = ((budget - d.B - n_stats - d.D) / per) * per;
        const int want = ((d.T * d.B + 15) / 16) * per;
        if (nb > want) nb = want;
        if (nb >= per && prep_blocks(d, s.prep_cpb, true) + d.B <= n_cu) { s.game_ok = true; s.game_nbas = nb; }
    }
    s.family = select_family(s, d);
    if (plan_jobs(h, s.family == FAM_TILE ? CODE_BIAS_TILE : s.family == FAM_FAST ? CODE_BIAS_FAST : CODE_BIAS_GENERIC)) return -1;
    {
        // the optimizer inside k_wgrad: its blocks spin on the norm role of the same launch, so ALL of them must be resident together
        s.wgrad_resident = (!s.any_split && s.ask[MMG_CAP_WGRAD_OPT] && s.caps[MMG_CAP_WGRAD_OPT] > 0) ? s.caps[MMG_CAP_WGRAD_OPT] : 0;
        s.wgrad_opt_ok = s.wgrad_resident > 0 && h->jt.n_wblocks + 5 <= s.wgrad_resident * n_cu - 8;
        if (s.vattn) s.wgrad_opt_ok = false;      // (attn_W_x.weight comes from k_vattn_dwx, not from a job: the norm is taken over d_grads, k_gradnorm + k_opt)
        const int nb2 = s.caps[MMG_CAP_WGRAD] > 0 ? s.caps[MMG_CAP_WGRAD] : 0;
        const int others = h->jt.n_wblocks + 1 - h->jt.gemm_tiles;
        const int slots = ((nb2 * n_cu - others) / 8) * 8;
        // (measured, round 5: 1 336 tiles on 856 slots 289 -> 281 us per minibatch, 3 848 on 672 219 -> 217; 5 120 on 552 388 -> 396 --
        //  beyond ~6 tiles per workgroup the static split loses more to its ragged last round than the walk saves;
        //  a balanced stride (tiles / rounds) gave the gain away again: as many workgroups as are resident)
        s.wgrad_stride = (h->jt.gemm_tiles > slots && slots >= 64 && h->jt.gemm_tiles <= 6 * slots) ? slots : 0;
    }
    plan_launches(h);
    if (no_roles) {
        // nothing that spins on another workgroup of its own launch: per-step / per-phase launches only
        //   (MMG_NO_MERGE + MMG_NO_MERGE_PREP + MMG_NO_GAME + MMG_NO_WGRAD_OPT + MMG_NO_PERSIST + MMG_NO_SPLIT + MMG_NO_MC + MMG_NO_RC_PERSIST + MMG_NO_RC_BWD) -- in the switches and in every role launch of the plan
        const LaunchPlan& p = s.plan; const TileFwd tf = p.tile_fwd;
        if (s.game_ok || s.wgrad_opt_ok || s.tile_persist || s.tile_split || s.mc_ok || s.rc_persist || s.rc_bwd || s.merge_roles || s.sw_merge_prep ||
            s.family == FAM_MC || tf == TF_SPLIT || tf == TF_PERSIST_SAMPLE || tf == TF_PERSIST_TILE || tf == TF_RC_PERSIST || p.basehx_rides ||
            p.merge_prep || p.fwd_basehx || p.bas_defer_ok || p.bas_pending_ok || p.merged_send || p.bwd_rec == BR_RC || p.n_class)
            return fail("internal: a role launch survived the no-roles selection");
    }
    return 0;
}

static int shape_pass(mmg_handle* h, const Switches& w) {
    h->no_roles = h->no_roles || w.roles_off();
    return shape_pass(h->cfg, h->dm, w, h->no_roles, h->flip_sen || h->flip_rec, h->sender_var, h->relax_tau_sen > 0.f,
                      h->noise_sigma_sen > 0.f || h->noise_sigma_rec > 0.f, h->d_err != nullptr, h->sel, h->attn_dim, h->n_words, h->vd);
}
static int select_paths(mmg_handle* h) {
    const Switches w = read_switches();
    if (shape_pass(h, w) || probe_device(h->cfg, h->dm, h->sel)) return -1;
    // (the tables mmg_set_trainable kept belong to the selection before; the callers upload h->jt themselves, after draining the device)
    for (auto& mp : h->mask_plans) mp.valid = false;
    if (decide(h, w)) return -1;
    if (h->jt_src) {                                      // a table that still waits for its upload: the one just decided takes its place
        if (keep_mask_plan(h)) return -1;
        h->jt_src = h->mask_plans[frozen_agents(h)].pinned;
    }
    return 0;
}
// The selection again for another set of frozen agents (mmg_set_trainable), from the caps the device gave at the last select_paths: exactly
// what mmg_plan_for does -- shape_pass starts from an empty Selection, so nothing of the plan before survives --, and no HIP call.
static int reselect_from_caps(mmg_handle* h) {
    const Switches w = read_switches();
    int32_t caps[MMG_PLAN_CAPS];
    memcpy(caps, h->sel.caps, sizeof(caps));
    if (shape_pass(h, w)) return -1;
    memcpy(h->sel.caps, caps, sizeof(caps));
    return decide(h, w);
}

// What a selection decided (mmg_plan_text / mmg_plan_for): family and k_wgrad's plan | capabilities, LDS sizes and budgets | the sample tiles'
// forward | many classes, register-resident forward, baselines | backward | the caps the decisions were taken from.
static int plan_text(const mmg_handle* h, char* out, int out_bytes) {
    const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    if (!out || out_bytes <= 0) return fail("plan text: no output buffer");
    int n = 0;
    auto line = [&](const char* fmt, auto... a) { if (n < out_bytes) n += snprintf(out + n, (size_t)(out_bytes - n), fmt, a...); };
    line("mmg_create: family %d (0 fast, 1 mc, 2 tile, 3 generic) no_roles %d n_cu %d game_ok %d game_nbas %d wgrad_stride %d (gemm tiles %d) wgrad_opt_ok %d (blocks %d, resident %d x %d)\n",
         (int)s.family, (int)h->no_roles, s.n_cu, (int)s.game_ok, s.game_nbas, s.wgrad_stride, h->jt.gemm_tiles, (int)s.wgrad_opt_ok, h->jt.n_wblocks + 5, s.wgrad_resident, s.n_cu);
    line("mmg_create: tile_ok %d tile_nt %d tile_smem %d tile_ext %d tile_persist %d persist_smem %d resident_budget %d tile_bwd_smem %d bwd_pre %d send_bwd %d split %d mc %d fast %d rc %d rc_persist %d rc_budget %d rc_bwd %d\n",
         (int)s.tile_ok, s.tile_nt, s.tile_smem, (int)s.tile_ext, (int)s.tile_persist, s.persist_smem, s.resident_budget, s.tile_bwd_smem,
         bwd_pre_lds_floats(h->dm) * 4, s.send_bwd_smem, (int)s.tile_split, (int)s.mc_ok, (int)s.use_fast, (int)s.rc_fwd, (int)s.rc_persist, s.rc_budget, (int)s.rc_bwd);
    line("mmg_create: tile forward %d (0 split, 1 whole, 2 persist/sample, 3 persist/tile, 4 rc persist, 5 rc step, 6 step) rsample %d ns1 %d ns2 %d roles per tile %d tiles per launch %d launches %d basehx rides %d skip %d\n",
         (int)p.tile_fwd, p.rsample, p.ns1, p.ns2, p.chunk_roles, p.chunk_tiles, p.n_chunk, (int)p.basehx_rides, (int)p.skip_ok);
    line("mmg_create: mc grid %d xcd %d mc3 %d mc3p %d wins %d grid %d | merge_prep %d nprep %d fwd_basehx %d | baselines: defer %d pending %d kernel %d (0 tile4, 1 live3, 2 all2)\n",
         p.mc_grid, s.mc_xcd, (int)s.mc3_ok, (int)s.mc3p_ok, (int)p.mc3p_wins, p.mc3p_grid, (int)p.merge_prep, p.nprep_hx, (int)p.fwd_basehx, (int)p.bas_defer_ok, (int)p.bas_pending_ok, (int)p.bas_kernel);
    line("mmg_create: backward: row_map %d zero_dead %d merged_send %d pre_bands %d receiver %d (0 sample, 1 tile, 2 rc) n_dbar %d class roles %d k_dC %d (0 none, 1 tile, 2 plain) mc groups %d\n",
         (int)p.row_map, (int)p.zero_dead, (int)p.merged_send, p.pre_bands, (int)p.bwd_rec, p.n_dbar, p.n_class, (int)p.dc, p.mc_ngroup);
    if (s.noise) line("mmg_create: message noise: %s serves the conversation, k_conversation_noise the agent-level entries\n",
                      s.family == FAM_MC ? "k_conversation_mc3_noise" : "k_conversation_noise");
    const int32_t* c = s.caps;
    line("mmg_create: caps n_cu %d split %d persist %d rc_bwd %d rc_persist %d mc %d mc3 %d mc3p %d game %d wgrad_opt %d wgrad %d\n",
         c[MMG_CAP_N_CU], c[MMG_CAP_SPLIT], c[MMG_CAP_PERSIST], c[MMG_CAP_RC_BWD], c[MMG_CAP_RC_PERSIST], c[MMG_CAP_MC], c[MMG_CAP_MC3], c[MMG_CAP_MC3P],
         c[MMG_CAP_GAME], c[MMG_CAP_WGRAD_OPT], c[MMG_CAP_WGRAD]);
    if (n >= out_bytes) return fail("plan text: %d bytes needed, the buffer holds %d", n + 1, out_bytes);
    return 0;
}
