// host_launch.h -- host side of mmg.hip: the handle with its Selection (the device caps it was decided from included) and LaunchPlan, the timing
// scope of a launch and the launch helpers that more than one entry point uses.  Included by mmg.hip only (after the kernels and fail() / HIP_OK).
#pragma once

struct KernelTimer { std::string name; hipEvent_t t0, t1; };

// The D == 30 instantiations of the register-resident kernels (D = 30: own instantiation, other D <= 32: capacity 32): each
// family picks its function once, selection and launch share the choice.
static auto game_fast_fn(int D) { return D == 30 ? k_game_fast<30> : k_game_fast<32>; }
static auto bwd_sample_fn(int D) { return D == 30 ? k_bwd_sample<64, 100, 30> : k_bwd_sample<64, 100, 32>; }
// V == 100 has its own instantiation as well; every other width runs the V = 0 one (layout.h: fast_wide_v)
template <bool STATS, bool DC> static auto bwd_conv_fast_fn(int D, int V) {
    if (V != 100) return k_bwd_conv_fast<256, 32, 64, 0, 32, STATS, DC>;
    return D == 30 ? k_bwd_conv_fast<256, 32, 64, 100, 30, STATS, DC> : k_bwd_conv_fast<256, 32, 64, 100, 32, STATS, DC>;
}

// Which kernel family serves the handle (host_select.h: select_family): the register-resident kernels of the small agents (the
// former fast_shape) | the same agents with many classes (kernels_mc*.h) | sample tiles on the matrix cores | the per-sample kernels
enum Family { FAM_FAST, FAM_MC, FAM_TILE, FAM_GENERIC };
// How far a forward pass runs and what it keeps (the ABI's run_all_steps 0 / 1 / 2 / 3, mapped at the entry points: tape_mode)
enum TapeMode { TAPE_TO_STOP, TAPE_ALL, TAPE_MINIMAL, TAPE_LOG };
static TapeMode tape_mode(int v) { return v == 0 ? TAPE_TO_STOP : v == 2 ? TAPE_MINIMAL : v == 3 ? TAPE_LOG : TAPE_ALL; }
// The sample tiles' forward, in fall-through order: class helpers | one workgroup per tile | one launch of co-resident roles
// (per-sample or per-tile receiver roles) | the wide receiver as one role launch / per step | per-step launches
enum TileFwd { TF_SPLIT, TF_WHOLE, TF_PERSIST_SAMPLE, TF_PERSIST_TILE, TF_RC_PERSIST, TF_RC_STEP, TF_STEP };
enum BasKernel { BAS_TILE4, BAS_LIVE3, BAS_ALL2 };          // standalone baselines: k_baselines4 (after k_gemm_nt unless basehx rode along) / 3 / 2
enum BwdRec { BR_SAMPLE, BR_TILE, BR_RC };                  // the tiles' receiver BPTT: k_bwd_sample / k_bwd_tile<512, 2|4|8> / k_rc_bwd
enum DcKernel { DC_NONE, DC_TILE, DC_PLAIN };               // the class-side reduction left after the backward launch: none (class roles) / k_dC_tile / k_dC

// The launch plan of a handle: every decision the per-minibatch launches need, taken ONCE by select_paths (host_select.h: plan_launches) from Dims, the switches and the
// device's budgets.  The launch code of mmg.hip reads it and tests nothing else; the per-call inputs (train, tape mode, defer_bas, the corruption mask, ForwardState) join it at the call.
struct LaunchPlan {
    int tiles = 0, n_stats = 0, n_bas = 0, basehx_tiles = 0, nprep_hx = 0;      // sample tiles, statistics / baseline roles, basehx tiles, k_prep's blocks incl. h_x
    TileFwd tile_fwd = TF_STEP;
    decltype(&k_conv_tile<512>) conv_tile_fn = nullptr;
    decltype(&k_conv_persist<512, true>) persist_fn = nullptr;
    int rsample = 0, ns1 = 0, ns2 = 0;          // k_conv_persist: receiver-role level 0-3, sender roles per tile
    int chunk_roles = 0, chunk_tiles = 0, n_chunk = 0;   // the chunked role launches (k_conv_persist with sample roles, k_rc_persist): roles per tile, tiles per launch, launches
    bool basehx_rides = false;                  // ... whose single launch may carry the basehx tiles (at the call: train && !run_all)
    bool skip_ok = false;                       // per-step launches may skip finished tiles (at the call: train && !run_all)
    int s1_grid = 0, s2_grid = 0, rc_nj = 0, rc_njw = 0;
    int mc_ntile = 0, mc_grid = 0, mc3p_grid = 0;
    bool mc3p_wins = false;                     // the pair kernel needs fewer rounds (at the call: lean)
    bool merge_prep = false, fwd_basehx = false;         // k_prep's blocks / the basehx tiles as roles of the conversation launch (basehx at the call: train && !all rows)
    decltype(&k_conversation_fast3<256, 32, 64, 100, false>) fast_fn = nullptr;
    decltype(&k_conversation<256>) conv_fn = nullptr, agent_fn = nullptr;   // whole conversation / the agent-level entries' step window (k_conversation<256>)
    decltype(&k_conversation_attn<256>) conv_attn_fn = nullptr, agent_attn_fn = nullptr;   // ... of an attention handle (the receiver's entries; the sender's run agent_fn)
    decltype(&k_conversation_vattn<256>) conv_vattn_fn = nullptr, agent_vattn_fn = nullptr;   // ... of a visual-attention handle (the sender's entries; the receiver's run agent_fn)
    int fast_smem = 0;                          // dynamic LDS of fast_fn
    const char *conv_name = "k_conversation", *bwd_name = "k_bwd_conv";
    bool bas_defer_ok = false, bas_pending_ok = false;   // roles of the backward launch (fused step) / of k_bas_stats (phased step)
    BasKernel bas_kernel = BAS_ALL2;
    int bas2_z = 0;
    bool row_map = false, zero_dead = false;    // k_wgrad walks the live-row list (conv_done: always); dead rows zeroed instead
    bool merged_send = false, send_own = false, dhx_own = false;
    int pre_bands = 1, pre_smem = 0, n_pre = 0, n_rowblk = 0, n_hbands = 0, dhx_blk = 0, dhx_grid = 0;
    decltype(&k_bwd_pre<8>) pre_fn = nullptr;
    decltype(&k_bwd_pre_send<8>) pre_send_fn = nullptr;
    BwdRec bwd_rec = BR_TILE;
    decltype(&k_bwd_tile<512, 2>) bwd_tile_fn = nullptr;
    int mc_ngroup = 0, mc_nred = 0, dc_grid = 0, dc_slices = 1;
    decltype(bwd_conv_fast_fn<true, true>(0, 0)) bwd_fast_fn = nullptr, bwd_fast_stats_fn = nullptr;
    decltype(&k_bwd_conv<false>) bwd_conv_fn = nullptr;
    int n_dbar = 0, n_class = 0;                // k_bwd_conv_fast: dbar tiles, class roles without the statistics
    DcKernel dc = DC_NONE;
};

// What select_paths decided (host_select.h): which kernels serve this handle's shape on this device, their LDS sizes, the co-residency budgets, the
// family and the launch plan.  Filled in three steps -- shape_pass (pure: everything up to the candidates that wait for a budget, and `ask`),
// probe_device (`caps`), decide (pure: the rest) -- and printed by plan_text.  Constant until the next selection (mmg_create; error_gate after a
// timed-out dependency; mmg_set_message_flipout / mmg_set_sender_variant / mmg_set_message_relaxation / mmg_set_message_noise when the routing changes).
struct Selection {
    int conv_smem = 0, conv_smem_agent = 0, conv_threads = 0, bwd_smem = 0, prep_smem = 0, prep_cpb = 1;
    int vattn_bwd_smem = 0;      // dynamic LDS of k_vattn_bwd (a visual-attention handle)
    bool sw_merge_bas = false;   // (= merge_roles) the baselines' forward pass rides in the backward / statistics launch; off: its own launch
    bool sw_merge_prep = false;  // k_prep's blocks as roles of k_conversation_fast3's launch (MMG_NO_MERGE_PREP=1: a launch of their own)
    bool game_ok = false;        // fused step of the small Adaptive agents: conversation + statistics + baselines + backward in ONE launch (kernels_game.h); MMG_NO_GAME=1: off
    int game_bas_ub = 1;         // ... 64-unit blocks of a baseline per role: 2 when the block count is even
    int game_nbas = 0;           // ... its baseline roles (a multiple of 2 * ceil(K / 64), sized by the co-residency budget)
    int wgrad_stride = 0;        // > 0: k_wgrad's GEMM tiles are walked by this many resident workgroups (more tiles than slots); 0: one workgroup per tile
    bool wgrad_opt_ok = false;   // the clip + optimizer step can run inside k_wgrad's launch (k_wgrad<true>: every block co-resident, no row splits); MMG_NO_WGRAD_OPT=1: off
    bool flip = false;           // message flips are set on a binary handle (mmg_set_message_flipout): k_conversation_fast3<FLIP> / k_conversation<FLIP> serve it, nothing else
    bool attn = false;           // an attention handle (mmg_attn_create): the generic per-sample family with k_conversation_attn / k_bwd_conv_attn serves it, nothing else
    bool vattn = false;          // a visual-attention handle (mmg_vattn_create): the generic per-sample family with k_conversation_vattn serves it, nothing else
    bool relax = false;          // relaxed messages are set (mmg_set_message_relaxation): the generic per-sample family with k_conversation<NT, false, false, RELAX>
                                 // serves the handle, nothing else; its backward pass is mmg_exchange_vjp_channel (k_vjp_channel_relax) only
    bool noise = false;          // Gaussian message noise is set on a continuous handle (mmg_set_message_noise): k_conversation_noise<NT> and, where the shape has it,
                                 // k_conversation_mc3_noise serve it, nothing else; every backward / VJP kernel reads the noisy messages from the tape
    int variant = 0;             // the sender variant in effect (mmg_set_sender_variant; SV_* bits, SV_IGNORE_REC on a binary handle only): != 0: the generic
                                 // per-sample family with k_conversation<NT, false, VAR> / k_bwd_conv<MANY, VAR> serves the handle, nothing else
    bool use_fast = false;       // debugging switches, read once at mmg_create: MMG_NO_FAST=1 forces the generic kernels,
    bool merge_roles = false;    // MMG_NO_MERGE=1 keeps k_stats / k_dC / basehx as separate launches / in-kernel work
    // sample-tile MFMA path (kernels_tile.h): every shape the register-resident kernels do not cover
    bool tile_ok = false;        // its LDS plan fits (MMG_NO_TILE=1: never use it)
    bool rc_bwd = false;         // ... and the reverse-time loop of its backward as co-resident roles over 16-unit slices (k_rc_bwd); MMG_NO_RC_BWD=1: k_bwd_tile's loop
    bool rc_persist = false;     // ... as ONE launch of co-resident roles (k_rc_persist) when they all fit on the device; MMG_NO_RC_PERSIST=1: per-step launches
    int rc_budget = 0;
    bool rc_fwd = false;         // wide receiver (kernels_rc.h): the tile's receiver step as three chip-wide launches over 16-unit slices -- the
                                 // one-workgroup-per-tile forward does not fit its LDS plan (R > 128 with a 256-bit message); MMG_NO_RC=1: off
    bool tile_force = false;     // MMG_TILE=1: use it even where the register-resident kernels apply (cross-checks)
    bool tile_ext = false;       // the sender MLP of a step runs as its own chip-wide launches (k_send_s1 / k_send_s2)
    int tile_nt = 0, tile_smem = 0;   // threads per tile workgroup, dynamic LDS bytes
    int tile_bwd_smem = 0, send_bwd_smem = 0;
    bool tile_persist = false;   // the whole conversation as one launch of co-resident roles (k_conv_persist)
    bool tile_split = false;     // many classes: idle CUs as class helpers of the sample tiles (k_conv_split)
    int split_nh = 0, split_per = 0, split_smem = 0;
    int persist_ns1 = 0, persist_ns2 = 0, persist_smem = 0;
    // debugging switches of the launch paths (environment, read ONCE at mmg_create -- never on the per-minibatch path)
    bool sw_rsample = false, sw_rmsg = false, sw_fused_s = false, rs_capable = false;
    bool persist_ll = false;     // k_conv_persist's fused sender roles hand over (value, epoch) pairs in per-step slots (tape.pll_*); MMG_NO_PERSIST_LL=1: counters
    bool mc_ok = false;          // many-class register-resident conversation (kernels_mc.h); MMG_NO_MC=1: off
    bool mc3p_ok = false;        // ... for batches of several rounds of workgroups: two sample tiles per workgroup, pipelined (kernels_mc3p.h); MMG_NO_MC3P=1: off
    bool mc3_ok = false;         // continuous messages: the one-wave-per-SIMD many-class kernel (kernels_mc3.h); binary messages: k_conversation_mc
    bool any_split = false;      // some k_wgrad job splits its rows over workgroups (the last slice to arrive adds the partial tiles)
    bool wgrad_small_split = false;   // jobs with few output tiles split their (step, sample) rows further (layout.h: wgrad_job_nsplit)
    int mc_per = 0, mc_xcd = 0;  // classes per member of a tile; mc_xcd: a tile's 16 workgroups on one XCD
    // workgroups of 512 threads that are guaranteed to be resident together on this device (occupancy query at mmg_create,
    // minus a margin): the role launches (k_conv_persist / k_conv_split / k_conversation_mc) spin on each other, so a launch
    // may never hold more roles than this
    int resident_budget = 0, split_budget = 0, n_cu = 0;
    // the selection's device inputs (host_select.h): which occupancies the shape needs, what the device answered (indexed by MMG_CAP_*; 0: query
    // failed, -1: not asked), and k_wgrad<true>'s workgroups per CU where the in-launch optimizer was a candidate (else 0)
    bool ask[MMG_PLAN_CAPS] = {};
    int32_t caps[MMG_PLAN_CAPS] = {};
    int wgrad_resident = 0;
    Family family = FAM_GENERIC;
    LaunchPlan plan;
};

// What the last forward pass left for the later phases of the same minibatch (mmg_loss_stats / mmg_backward may be separate ABI
// calls).  Reset where a forward pass starts (exchange_forward_impl); the fused step (k_game_fast) states all of it.
struct ForwardState {
    bool scores_in_parts = false;   // the last forward left baseline scores as partials (k_baselines2)
    bool bas_deferred = false;      // the fused step's forward left the baselines to the backward launch (k_bwd_conv_fast: baseline roles)
    bool bas_pending = false;       // phased step: the forward pass left the baselines to mmg_loss_stats (k_bas_stats: one launch for both)
    bool basehx_ready = false;      // this forward pass formed tape.basehx inside the conversation launch
};

// What mmg_set_trainable decided for one set of frozen agents: the selection (k_wgrad's plan follows the job table) and the job table in
// pinned host memory, uploaded on the stream of the next minibatch.  valid: built since the last full selection (select_paths)
struct MaskPlan { bool valid = false; Selection sel; JobTable* pinned = nullptr; };

struct mmg_handle {
    mmg_config cfg = {};
    Dims dm = {};
    ParamLayout pl = {};
    TapeLayout tl = {};
    Params P = {}, G = {};
    Tape tp = {};
    float *params = nullptr, *grads = nullptr, *opt_state = nullptr;
    void* ws = nullptr;
    JobTable* d_jt = nullptr;
    JobTable jt = {};
    Selection sel;
    ForwardState fwd;
    bool profiling = false;
    std::vector<KernelTimer> timers;
    size_t timers_used = 0;
    uint32_t* h_err = nullptr;   // pinned host copy of sync[MMG_SYNC_ERR], written by k_opt of every step (posted store to mapped host memory)
    uint32_t* d_err = nullptr;   // its device-side address
    bool xcd_rule_ok = false;    // probed at mmg_create (k_xcc_probe): workgroup i of a launch runs on XCD i % 8 -- a hand-off between workgroups of one XCD may stay in its L2
    // fail-soft (round 6): no_roles = only launches without in-launch waits are selected (select_paths).  Set at mmg_create by
    // MMG_NO_ROLES=1 / a CU mask in the environment, or by recover() after a timed-out dependency (degraded)
    bool no_roles = false, degraded = false;
    int recoveries = 0;          // recover() calls so far (bounded: a wait that keeps timing out without roles is a real fault)
    uint32_t last_code = 0u;     // the dependency word of the last recovery
    // data-parallel step inside the library (mmg_dp_set_allreduce): RCCL's ncclAllReduce by address + the caller's communicator
    void* ar_fn = nullptr; void* ar_comm = nullptr;
    // mmg_set_message_corruption: the mask every evaluation conversation applies to the sender's messages (model.py:813-820);
    // while it is set, the training entries refuse to run
    bool corrupt_on = false;
    uint32_t corrupt[MMG_BLOCK / 32] = {};
    // mmg_set_message_flipout: random flips of the message bits (model.py:554-568).  Host state; flip_args copies it into the launch
    // arguments of every forward entry.  flip_evals: evaluation conversations enqueued since the setter call (their Philox counter)
    bool flip_sen = false, flip_rec = false, flip_dev = false;
    float flip_p_sen = 0.f, flip_p_rec = 0.f;
    uint64_t flip_eval_seed = 0;
    uint32_t flip_evals = 0;
    // mmg_set_message_noise: additive Gaussian noise on continuous messages (both sigmas 0: not set).  Host state; noise_args copies it into the
    // launch arguments of every forward entry.  noise_evals: evaluation conversations enqueued since the setter call (their Philox counter)
    float noise_sigma_sen = 0.f, noise_sigma_rec = 0.f;
    bool noise_dev = false;
    uint64_t noise_eval_seed = 0;
    uint32_t noise_evals = 0;
    // mmg_set_sender_variant: SV_* bits as the caller set them (layout.h).  Host state; what is in effect on this handle is sel.variant, which the
    // forward entries copy into ConvArgs::sender_var and the backward / sender-VJP launches pass as sv
    int sender_var = 0;
    // mmg_set_message_relaxation: the temperatures of the sender's / the receiver's relaxed message (both 0: not set) and the rounding.  Host
    // state; the forward entries copy it into ConvArgs, mmg_exchange_vjp_channel into VjpIn
    float relax_tau_sen = 0.f, relax_tau_rec = 0.f;
    bool relax_hard = false;
    // mmg_set_trainable: MMG_AGENT_* bits of the agents the training entries update (the others are frozen).  Host state; the optimizer
    // launches get it as OptArgs::trainable (mmg.hip: opt_trainable).  The learning rate and the entropy weights of mmg_set_learning_rate /
    // mmg_set_entropy live where mmg_create put them: cfg.learning_rate, cfg.entropy_* and their copies in dm
    int train_mask = 15;
    // ... and its job tables: k_wgrad's table holds the jobs of the agents in training only (host_jobs.h), one per set of frozen agents,
    // built at mmg_set_trainable and kept.  jt_src != NULL: the table in use is not on the device yet (apply_pending uploads it on the
    // stream of the next minibatch); zero_pending: agents whose gradient slice has to be cleared once -- nothing writes it while they are frozen
    MaskPlan mask_plans[16];
    std::vector<JobTable*> retired_tables;   // pinned tables a later selection replaced: never rewritten (an upload may still read them), freed with the handle
    const JobTable* jt_src = nullptr;
    int zero_pending = 0;
    // mmg_attn_create: desc_attn_dim (0: a plain handle) and the words of the description set; `at` is what the ATTN instantiations get
    // on top of the plain kernels' arguments (the six tensors inside the flat buffer, the attention arrays behind the plain tape), AG
    // the six gradient tensors; set_ready: mmg_set_desc_set has uploaded a set
    int attn_dim = 0, n_words = 0;
    AttnArgs at = {};
    AttnParams AG = {};
    bool set_ready = false;
    // mmg_vattn_create: the sender's attn_dim (0: a plain handle), the locations of the map, context_dim; `va` is what the VATTN
    // instantiations get on top of the plain kernels' arguments; d_ctx: the data context of the next conversation (mmg_set_data_context)
    VattnDims vd = VattnDims();
    VattnArgs va = {};
    const float* d_ctx = nullptr;
    VattnParams VG = {};         // the visual-attention tensors' gradients
    const float* bwd_x = nullptr;     // x of the backward call in flight (the attention's reverse pass reads the map)
    const float* ctx_cur = nullptr;   // the context rows the last forward entry read (the backward pass reads the same)
    bool vattn_stale = true;     // mmg_sender_forward forms HX / HG before its launch (mmg_vattn_reset_state; a whole conversation ran)
    WgHead vjp_hd[8] = {};       // launch geometry of k_wgrad over the VJP job tables (tape.vtables: exchange 0-3, per-call 4-7)
    ~mmg_handle() {
        for (auto& t : timers) { hipEventDestroy(t.t0); hipEventDestroy(t.t1); }
        if (h_err) hipHostFree(h_err);
        for (auto& mp : mask_plans) if (mp.pinned) hipHostFree(mp.pinned);
        for (JobTable* t : retired_tables) hipHostFree(t);
    }
};

// mmg_set_trainable on the device side.  OptArgs::trainable: bits 0-3 = the agents this step updates -- the caller's mask inside what the
// mode trains (continuous messages: the receiver alone, model.py:1313) --, bits 4-7 = the agents the mode trains and the caller froze.
static int opt_trainable(const mmg_handle* h) {
    const int mode = h->cfg.use_binary ? 15 : 1;
    return (mode & h->train_mask) | ((mode & ~h->train_mask) << 4);
}
static int frozen_agents(const mmg_handle* h) { return opt_trainable(h) >> 4; }
// The table in use into pinned memory of its own, kept with the selection it belongs to.  A buffer that held another table is retired, not
// rewritten: an upload enqueued from it may not have run yet.
static int keep_mask_plan(mmg_handle* h) {
    MaskPlan& mp = h->mask_plans[frozen_agents(h)];
    if (mp.pinned) h->retired_tables.push_back(mp.pinned);
    mp.pinned = nullptr; mp.valid = false;
    if (hipHostMalloc(reinterpret_cast<void**>(&mp.pinned), sizeof(JobTable), hipHostMallocDefault) != hipSuccess) { mp.pinned = nullptr; return fail("no pinned host memory for a job table"); }
    memcpy(mp.pinned, &h->jt, sizeof(JobTable));
    mp.sel = h->sel; mp.valid = true;
    return 0;
}
static bool is_frozen(const mmg_handle* h, int agent) { return (frozen_agents(h) >> agent) & 1; }

// ---------------------------------------------------------------------------------------------
// launch helper with optional HIP-event timing on the launch stream
// ---------------------------------------------------------------------------------------------
struct Scope {
    mmg_handle* h; hipStream_t st; KernelTimer* kt;
    Scope(mmg_handle* h_, hipStream_t st_, const char* name) : h(h_), st(st_), kt(nullptr) {
        if (!h->profiling) return;
        if (h->timers_used == h->timers.size()) {
            KernelTimer t; hipEventCreate(&t.t0); hipEventCreate(&t.t1); h->timers.push_back(t);
        }
        kt = &h->timers[h->timers_used++];
        kt->name = name;
        hipEventRecord(kt->t0, st);
    }
    ~Scope() { if (kt) hipEventRecord(kt->t1, st); }
};

static int launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

static int launch_gemm_nt(mmg_handle* h, hipStream_t st, const char* name, const float* X, int ldx, const float* Wm, int ldw,
                          const float* bias, float* out, int ldo, int M, int N, int K) {
    Scope sc(h, st, name);
    const int tiles = ((M + 15) / 16) * ((N + 15) / 16);
    hipLaunchKernelGGL(k_gemm_nt, dim3(tiles), dim3(MMG_BLOCK), 0, st, X, ldx, Wm, ldw, bias, out, ldo, M, N, K);
    return launch_check(name);
}

// x != NULL: also computes h_x = image_layer(x) in the same launch
static int launch_prep(mmg_handle* h, hipStream_t st, const float* desc, const float* x, int bump_mb) {
    Scope sc(h, st, x ? "k_prep+h_x" : "k_prep");
    const int cpb = h->sel.prep_cpb;
    hipLaunchKernelGGL(k_prep, dim3(prep_blocks(h->dm, cpb, x != nullptr)), dim3(MMG_BLOCK), h->sel.prep_smem, st, h->dm, h->P, h->tp, desc, x, cpb, bump_mb);
    return launch_check("k_prep");
}

// k_wgrad over one job table.  live_rows: the (step, sample) jobs reduce over the live-row list (tape.rmap) instead of all rows.
// stride > 0: that many resident workgroups walk the GEMM tiles.  closing: the spare block behind the tiles and column blocks
// (logged losses, running totals, gradient tail); opt != NULL: k_wgrad<true>, the clip + optimizer step inside the launch.
static int launch_wgrad(mmg_handle* h, hipStream_t st, const JobTable* djt, const WgHead& hd, const float* d_x, const float* d_desc,
                        bool live_rows, int stride, bool closing, const WgOpt* opt) {
    Scope sc(h, st, "k_wgrad");
    WgOpt wo;
    memset(&wo, 0, sizeof(wo));
    if (opt) wo = *opt;
    int grid = (stride > 0 ? stride - hd.gemm_tiles : 0) + hd.n_wblocks + (closing ? 1 : 0);
    if (opt) grid = hd.n_wblocks + 1 + 4;                // tiles + column blocks | spare / closing block | four norm roles
    hipLaunchKernelGGL(opt ? k_wgrad<true> : k_wgrad<false>, dim3(grid), dim3(MMG_BLOCK), 0, st,
                       djt, d_x, d_desc, h->tp.gnpart, h->dm, (const double*)h->tp.stats, h->tp.losses, h->tp.totals,
                       (const int*)(live_rows ? h->tp.rmap : nullptr), (const int*)(live_rows ? h->tp.rcount : nullptr), h->tp.wpart,
                       reinterpret_cast<uint32_t*>(h->tp.wcnt), (const uint32_t*)h->tp.sync, h->grads + h->pl.total, wo, opt ? 0 : stride, hd
#ifdef MMG_TIMING
                       , h->tp.dbg2
#endif
                       );
    return launch_check("k_wgrad");
}

// The weight gradients of a VJP: k_wgrad over job table `slot` of tape.vtables (0-3: exchange, 4-7: per call, agent = slot % 4) --
// its tiles and column blocks only (no spare block: the logged losses, running totals and gradient tail stay untouched), no
// live-row list.  Writes only the agent's slice of the gradient buffer.
static int launch_vjp_wgrad(mmg_handle* h, hipStream_t st, int slot, const float* d_x, const float* d_desc) {
    h->zero_pending |= frozen_agents(h);                 // (a VJP writes its agent's slice whatever the mask: cleared before the next training step)
    const JobTable* djt = reinterpret_cast<const JobTable*>(h->tp.vtables + (size_t)slot * MMG_VJP_TABLE_BYTES);
    return launch_wgrad(h, st, djt, h->vjp_hd[slot], d_x, d_desc, false, 0, false, nullptr);
}

// The class side of the receiver's VJPs: k_vjp_cd forms Cd before the per-sample kernel, k_vjp_class reduces over it afterwards.
static int launch_vjp_cd(mmg_handle* h, hipStream_t st, const float* d_desc) {
    Scope sc(h, st, "k_vjp_cd");
    hipLaunchKernelGGL(k_vjp_cd, dim3(h->dm.D), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, d_desc);
    return launch_check("k_vjp_cd");
}
static int launch_vjp_class(mmg_handle* h, hipStream_t st, const VjpIn& in) {
    Scope sc(h, st, "k_vjp_class");
    hipLaunchKernelGGL(k_vjp_class, dim3(h->dm.D), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, in);
    return launch_check("k_vjp_class");
}

// dynamic LDS of a VJP kernel in bytes; the kernels run under the default limit
static int vjp_lds_ok(size_t smem, const char* who, const char* why) {
    if (smem > 65536) return fail("the %s VJP needs %zu bytes of LDS%s", who, smem, why);
    return 0;
}
