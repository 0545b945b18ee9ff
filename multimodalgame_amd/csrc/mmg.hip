// mmg.hip -- C-ABI (include/mmg.h) of the MI355X-native exchange path.  Host side: layout queries,
// job-table construction, kernel launches on the caller's stream.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mmg.h"
#include "layout.h"
#include "device_utils.h"
#include "kernels_fwd.h"
#include "kernels_bwd.h"
#include "bwd_sample_parts.h"
#include "kernels_fast.h"
#include "kernels_fast3.h"
#include "kernels_game.h"
#include "kernels_tile.h"
#include "kernels_mc.h"
#include "kernels_mc3.h"
#include "kernels_mc3p.h"
#include "kernels_rc.h"
#include "kernels_vjp.h"
#include "kernels_eval.h"
#include "kernels_loss.h"
#include "kernels_pairs.h"
#ifdef MMG_ROLE_DIAG
#include "diag_kernels.h"
#endif

using namespace mmg;

static thread_local char g_err[512] = "";
static int fail(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return -1;
}
#define HIP_OK(expr)                                                                      \
    do { hipError_t e_ = (expr);                                                          \
         if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

#include "host_launch.h"       // the handle with its Selection and LaunchPlan, Scope, launch helpers shared between entry points
#include "host_jobs.h"         // k_wgrad's job tables
#include "host_select.h"       // launch geometry, select_paths: capabilities, family, launch plan

// ---------------------------------------------------------------------------------------------
// Fail-soft (round 6).  An in-launch dependency wait that hits its spin bound (fewer compute units than the launch's roles
// need: a shared or CU-masked GPU) sets sync[MMG_SYNC_ERR] on the device; k_opt / the norm role of THAT minibatch leave
// parameters and optimizer state untouched and post the word to a pinned host word (no synchronisation).  The reference has
// no such failure mode (model.py:1218-1330 simply keeps training), so the library recovers instead of failing the run:
// the next call that STARTS a minibatch (mmg_train_step[s], mmg_exchange_forward(train), mmg_dp_train_step) drains the
// stream once, clears both words, re-selects the kernels WITHOUT in-launch waits (select_paths with no_roles: per-step /
// per-phase launches, what MMG_NO_ROLES=1 selects up front), uploads the job table of that path and continues.  The call
// returns 1 (ok, with a warning in mmg_last_error()).  Entry points in the MIDDLE of a phased minibatch do nothing: that
// minibatch's update is skipped on the device anyway and the next minibatch start recovers.  Data parallel: the flag travels
// in the all-reduced gradient tail, every rank skips the same update and every rank posts a word (its own code or 1001).
// ---------------------------------------------------------------------------------------------
#define MMG_MAX_RECOVERIES 8
static int clear_error_words(mmg_handle* h, hipStream_t st) {
    HIP_OK(hipStreamSynchronize(st));                    // rare path: nothing of this handle is in flight afterwards
    const uint32_t zero = 0u;
    HIP_OK(hipMemcpy(h->tp.sync + MMG_SYNC_ERR, &zero, sizeof(zero), hipMemcpyHostToDevice));
    if (h->h_err) *(volatile uint32_t*)h->h_err = 0u;
    return 0;
}
// step_start: this call begins a minibatch.  0 = nothing to report, 1 = recovered (warning text in g_err), < 0 = error
static int error_gate(mmg_handle* h, hipStream_t st, bool step_start) {
    if (!h->h_err) return 0;
    const uint32_t code = *(volatile uint32_t*)h->h_err;
    if (code == 0u || !step_start) return 0;
    if (h->recoveries >= MMG_MAX_RECOVERIES)
        return fail("in-launch dependency %u timed out on the device again after %d recoveries (the launches in use hold no in-launch "
                    "waits: device fault?)", code - 1u, h->recoveries);
    if (clear_error_words(h, st)) return -1;
    const bool was_roles = !h->no_roles;
    if (was_roles) {
        h->no_roles = true;
        if (select_paths(h)) return -1;
        HIP_OK(hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice));
        h->degraded = true;
    }
    ++h->recoveries; h->last_code = code;
    if (code == MMG_SYNC_ERR_REMOTE)
        fail("warning: another rank of the data-parallel job reported a timed-out in-launch dependency; every rank skipped that "
             "optimizer update%s", was_roles ? " and continues on the launches without in-launch waits" : "");
    else
        fail("warning: in-launch dependency %u timed out on the device (fewer compute units available than the launch's workgroup "
             "roles need?); the optimizer update of that minibatch was skipped%s", code - 1u,
             was_roles ? " and training continues on the launches without in-launch waits (MMG_NO_ROLES=1 selects them up front)" : "");
    return 1;
}
// The gate of every entry that trains: refused while a corruption mask is set (the training conversations are not corrupted) ...
static int begin_minibatch(const mmg_handle* h, const char* who) {
    if (!h) return fail("NULL handle");
    if (h->corrupt_on) return fail("%s: a message corruption mask is set (evaluation only; mmg_set_message_corruption(h, NULL, 0) clears it)", who);
    return 0;
}
// ... and each of its n minibatches starts at error_gate.  < 0: error; 1: ok, some minibatch recovered (warning in g_err); 0: ok
template <class Step> static int run_minibatches(mmg_handle* h, int64_t n, void* stream, Step step) {
    int warn = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int w = error_gate(h, (hipStream_t)stream, true);
        if (w < 0 || step(i)) return -1;
        warn |= w;
    }
    return warn;
}

extern "C" int mmg_clear_error(mmg_handle* h, void* stream) {
    if (!h) return fail("NULL handle");
    return clear_error_words(h, (hipStream_t)stream);
}
extern "C" int mmg_degraded(const mmg_handle* h) { return (h && h->no_roles) ? (h->degraded ? 2 : 1) : 0; }

extern "C" const char* mmg_last_error(void) { return g_err; }
extern "C" int mmg_version(void) { return MMG_VERSION; }

static int validate(const mmg_config* c) {
    if (!c) return fail("config is NULL");
    if (c->batch <= 0 || c->n_classes <= 0 || c->feat_dim <= 0 || c->h_dim <= 0 || c->w_dim <= 0 ||
        c->rec_hidden <= 0 || c->wv_dim <= 0 || c->bas_hidden <= 0 || c->max_exchange <= 0)
        return fail("all dimensions must be positive");
    if (c->max_exchange > 64) return fail("max_exchange must be <= 64");
    if (c->w_dim > MMG_BLOCK || c->rec_hidden > MMG_BLOCK)
        return fail("w_dim and rec_hidden must be <= %d (got %d, %d)", MMG_BLOCK, c->w_dim, c->rec_hidden);
    if (c->wv_dim > MMG_MAX_WV) return fail("wv_dim must be <= %d (got %d)", MMG_MAX_WV, c->wv_dim);
    if (c->optim_type < 0 || c->optim_type > 2) return fail("unknown optim_type %d", c->optim_type);
    if (c->global_batch > 0 && c->global_batch < c->batch) return fail("global_batch < batch");
    return 0;
}

// Description attention (mmg_attn_*): attn_dim == 0 is the plain handle; otherwise the supported range, an error beyond it
static int validate_attn(const mmg_config* c, int attn_dim, int n_words) {
    if (validate(c)) return -1;
    if (attn_dim == 0) return 0;
    if (attn_dim < 0 || attn_dim > MMG_MAX_ATTN) return fail("desc_attn: attn_dim must be 1..%d (got %d)", MMG_MAX_ATTN, attn_dim);
    if (c->n_classes > MMG_ATTN_MAX_CLASSES) return fail("desc_attn: n_classes must be <= %d (got %d)", MMG_ATTN_MAX_CLASSES, c->n_classes);
    if (n_words < c->n_classes || n_words > MMG_MAX_WORDS)
        return fail("desc_attn: n_words must be n_classes..%d, every description holding a word (got %d for %d classes)", MMG_MAX_WORDS, n_words, c->n_classes);
    if (c->batch > MMG_ATTN_MAX_BATCH) return fail("desc_attn: batch must be <= %d (got %d)", MMG_ATTN_MAX_BATCH, c->batch);
    if (c->global_batch > 0 && c->global_batch != c->batch) return fail("desc_attn runs on one GPU (global_batch %d != batch %d)", c->global_batch, c->batch);
    return 0;
}

// Visual attention (mmg_vattn_*): attn_dim == 0 is the plain handle; otherwise the supported range, an error beyond it
static int validate_vattn(const mmg_config* c, VattnDims v) {
    if (validate(c)) return -1;
    if (v.A == 0) return 0;
    if (v.A < 0 || v.A > MMG_VATTN_MAX_DIM) return fail("visual_attn: attn_dim must be 1..%d (got %d)", MMG_VATTN_MAX_DIM, v.A);
    if (v.N < 1 || v.N > MMG_VATTN_MAX_FEATS) return fail("visual_attn: n_feats (h * w of the map) must be 1..%d (got %d)", MMG_VATTN_MAX_FEATS, v.N);
    if (c->feat_dim > MMG_VATTN_MAX_CHANNELS)
        return fail("visual_attn: feat_dim (the channels of the map) must be <= %d (got %d)", MMG_VATTN_MAX_CHANNELS, c->feat_dim);
    if (v.G < 0 || v.G > MMG_VATTN_MAX_CTX) return fail("visual_attn: context_dim must be 0..%d (got %d)", MMG_VATTN_MAX_CTX, v.G);
    if (c->batch > MMG_VATTN_MAX_BATCH) return fail("visual_attn: batch must be <= %d (got %d)", MMG_VATTN_MAX_BATCH, c->batch);
    if ((int64_t)c->batch * v.N * v.A > MMG_VATTN_MAX_HX)
        return fail("visual_attn: batch * n_feats * attn_dim must be <= %lld (got %lld)", (long long)MMG_VATTN_MAX_HX, (long long)c->batch * v.N * v.A);
    if (c->global_batch > 0 && c->global_batch != c->batch) return fail("visual_attn runs on one GPU (global_batch %d != batch %d)", c->global_batch, c->batch);
    return 0;
}
static int validate_any(const mmg_config* c, int attn_dim, int n_words, VattnDims v) {
    return v.A ? validate_vattn(c, v) : validate_attn(c, attn_dim, n_words);
}

static int64_t param_count_impl(const mmg_config* cfg, int attn_dim, int n_words, VattnDims vd) {
    if (validate_any(cfg, attn_dim, n_words, vd)) return -1;
    return param_layout(*cfg, attn_dim, vd).total;
}
extern "C" int64_t mmg_attn_param_count(const mmg_config* cfg, int attn_dim, int n_words) { return param_count_impl(cfg, attn_dim, n_words, VattnDims()); }
extern "C" int64_t mmg_vattn_param_count(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim) {
    return param_count_impl(cfg, 0, 0, VattnDims{attn_dim, n_feats, context_dim});
}
extern "C" int64_t mmg_param_count(const mmg_config* cfg) { return mmg_attn_param_count(cfg, 0, 0); }

static int param_table_impl(const mmg_config* cfg, int attn_dim, int n_words, VattnDims vd, mmg_param_entry* out, int max_entries) {
    if (validate_any(cfg, attn_dim, n_words, vd)) return -1;
    ParamLayout L = param_layout(*cfg, attn_dim, vd);
    const int n = P_COUNT + (attn_dim > 0 ? (int)A_COUNT : 0) + L.v_n;
    if (out) {
        if (max_entries < n) return fail("need room for %d entries", n);
        int k = 0;
        auto put = [&](const char* name, int agent, int rows, int cols, int64_t off) {
            memset(&out[k], 0, sizeof(out[k]));
            strncpy(out[k].name, name, sizeof(out[k].name) - 1);
            out[k].agent = agent; out[k].rows = rows; out[k].cols = cols; out[k].offset = off;
            ++k;
        };
        for (int i = 0; i < P_COUNT; ++i) {
            if (i == S_IMG_W && attn_dim > 0)           // the attention tensors close the receiver's range
                for (int a = 0; a < A_COUNT; ++a) put(L.a_name[a], MMG_AGENT_RECEIVER, L.a_rows[a], L.a_cols[a], L.a_off[a]);
            if (i == BR_L1_W)                           // the visual-attention tensors close the sender's range
                for (int a = 0; a < L.v_n; ++a) put(L.v_name[a], MMG_AGENT_SENDER, L.v_rows[a], L.v_cols[a], L.v_off[a]);
            put(L.name[i], L.agent[i], L.rows[i], L.cols[i], L.off[i]);
        }
    }
    return n;
}
extern "C" int mmg_attn_param_table(const mmg_config* cfg, int attn_dim, int n_words, mmg_param_entry* out, int max_entries) {
    return param_table_impl(cfg, attn_dim, n_words, VattnDims(), out, max_entries);
}
extern "C" int mmg_vattn_param_table(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, mmg_param_entry* out, int max_entries) {
    return param_table_impl(cfg, 0, 0, VattnDims{attn_dim, n_feats, context_dim}, out, max_entries);
}
extern "C" int mmg_param_table(const mmg_config* cfg, mmg_param_entry* out, int max_entries) { return mmg_attn_param_table(cfg, 0, 0, out, max_entries); }

extern "C" int64_t mmg_attn_grad_floats(const mmg_config* cfg, int attn_dim, int n_words) {
    if (validate_attn(cfg, attn_dim, n_words)) return -1;
    return param_layout(*cfg, attn_dim).total + MMG_GRAD_TAIL;
}
extern "C" int64_t mmg_vattn_grad_floats(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim) {
    const int64_t n = mmg_vattn_param_count(cfg, attn_dim, n_feats, context_dim);
    return n < 0 ? -1 : n + MMG_GRAD_TAIL;
}
extern "C" int64_t mmg_grad_floats(const mmg_config* cfg) { return mmg_attn_grad_floats(cfg, 0, 0); }

extern "C" int64_t mmg_attn_workspace_bytes(const mmg_config* cfg, int attn_dim, int n_words) {
    if (validate_attn(cfg, attn_dim, n_words)) return -1;
    return tape_layout(*cfg, attn_dim, n_words).total;
}
extern "C" int64_t mmg_vattn_workspace_bytes(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim) {
    const VattnDims vd{attn_dim, n_feats, context_dim};
    if (validate_vattn(cfg, vd)) return -1;
    return tape_layout(*cfg, 0, 0, vd).total;
}
extern "C" int64_t mmg_workspace_bytes(const mmg_config* cfg) { return mmg_attn_workspace_bytes(cfg, 0, 0); }

static int tape_table_impl(const mmg_config* cfg, int attn_dim, int n_words, VattnDims vd, mmg_tape_entry* out, int max_entries) {
    if (validate_any(cfg, attn_dim, n_words, vd)) return -1;
    TapeLayout L = tape_layout(*cfg, attn_dim, n_words, vd);
    if (out) {
        if (max_entries < L.n) return fail("need room for %d entries", L.n);
        memcpy(out, L.e, sizeof(mmg_tape_entry) * L.n);
    }
    return L.n;
}
extern "C" int mmg_attn_tape_table(const mmg_config* cfg, int attn_dim, int n_words, mmg_tape_entry* out, int max_entries) {
    return tape_table_impl(cfg, attn_dim, n_words, VattnDims(), out, max_entries);
}
extern "C" int mmg_vattn_tape_table(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, mmg_tape_entry* out, int max_entries) {
    return tape_table_impl(cfg, 0, 0, VattnDims{attn_dim, n_feats, context_dim}, out, max_entries);
}
extern "C" int mmg_tape_table(const mmg_config* cfg, mmg_tape_entry* out, int max_entries) { return mmg_attn_tape_table(cfg, 0, 0, out, max_entries); }

// A handle with its layouts and the addresses inside the caller's buffers (no GPU call)
static mmg_handle* new_handle(const mmg_config& cfg, void* ws, float* params, float* grads, float* opt_state, int attn_dim = 0, int n_words = 0,
                              VattnDims vd = VattnDims()) {
    mmg_handle* h = new mmg_handle();
    h->cfg = cfg;
    if (h->cfg.global_batch <= 0) h->cfg.global_batch = h->cfg.batch;
    h->dm = make_dims(h->cfg);
    h->attn_dim = attn_dim; h->n_words = attn_dim > 0 ? n_words : 0;
    h->vd = vd.A > 0 ? vd : VattnDims();
    h->pl = param_layout(h->cfg, attn_dim, h->vd);
    h->tl = tape_layout(h->cfg, attn_dim, n_words, h->vd);
    h->ws = ws; h->params = params; h->grads = grads; h->opt_state = opt_state;
    h->P = resolve_params(h->pl, params);
    h->G = resolve_params(h->pl, grads);
    h->tp = resolve_tape(h->tl, ws);
    h->at.A = h->attn_dim; h->at.NW = h->n_words;
    h->at.P = resolve_attn_params(h->pl, params);
    h->AG = resolve_attn_params(h->pl, grads);
    h->at.tp = resolve_attn_tape(h->tl, ws);
    h->va.A = h->vd.A; h->va.N = h->vd.N; h->va.G = h->vd.G; h->va.inv_n = h->vd.N > 0 ? 1.0f / (float)h->vd.N : 0.f;
    h->va.P = resolve_vattn_params(h->pl, params);
    h->va.tp = resolve_vattn_tape(h->tl, ws);
    h->VG = resolve_vattn_params(h->pl, grads);
    h->d_jt = reinterpret_cast<JobTable*>(h->tp.tables);
    return h;
}

static mmg_handle* create_impl(const mmg_config* cfg, int attn_dim, int n_words, VattnDims vd, void* d_workspace, int64_t workspace_bytes,
                               float* d_params, float* d_grads, float* d_opt_state) {
    if (validate_any(cfg, attn_dim, n_words, vd)) return nullptr;
    if (!d_workspace || !d_params || !d_grads || !d_opt_state) { fail("NULL device buffer"); return nullptr; }
    mmg_handle* h = new_handle(*cfg, d_workspace, d_params, d_grads, d_opt_state, attn_dim, n_words, vd);
    if (workspace_bytes < h->tl.total) { fail("workspace too small: %lld < %lld", (long long)workspace_bytes, (long long)h->tl.total); delete h; return nullptr; }
    if (hipHostMalloc((void**)&h->h_err, sizeof(uint32_t), hipHostMallocMapped) == hipSuccess) {
        *h->h_err = 0u;
        if (hipHostGetDevicePointer((void**)&h->d_err, h->h_err, 0) != hipSuccess) h->d_err = nullptr;
    } else h->h_err = nullptr;
    if (select_paths(h)) { delete h; return nullptr; }       // (also sets h->no_roles for MMG_NO_ROLES=1 / a CU mask in the environment)
    {
        // does this device place workgroup i of a launch on XCD i % 8 (8 distinct XCDs)?  The XCD-aware launches only PREFER that
        // placement; the many-class conversation may additionally keep its hand-off pairs inside the XCD's L2 when it holds.
        if (h->sel.mc_ok && h->sel.mc_xcd) {
            const int n = 2048;
            uint32_t* d_probe = reinterpret_cast<uint32_t*>(h->tp.tables);      // (the job-table slot: uploaded below)
            if (hipMemset(d_probe, 0xff, n * sizeof(uint32_t)) == hipSuccess) {
                hipLaunchKernelGGL(k_xcc_probe, dim3(n), dim3(64), 0, 0, d_probe);
                std::vector<uint32_t> got(n);
                if (hipMemcpy(got.data(), d_probe, n * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess) {
                    bool ok = true;
                    for (int i = 0; i < n && ok; ++i) ok = got[i] < 8u && got[i] == got[i & 7];
                    for (int a = 0; a < 8 && ok; ++a) for (int b = a + 1; b < 8 && ok; ++b) ok = got[a] != got[b];
                    h->xcd_rule_ok = ok;
                }
            }
        }
        hipError_t e = hipMemset(d_workspace, 0, h->tl.total);
        if (e == hipSuccess) e = hipMemset(d_grads, 0, sizeof(float) * (h->pl.total + MMG_GRAD_TAIL));
        if (e != hipSuccess) { fail("device init failed: %s", hipGetErrorString(e)); delete h; return nullptr; }
    }
    hipError_t e = hipSuccess;
    {
        std::vector<float> one(256, 1.0f);
        e = hipMemcpy(h->tp.ones, one.data(), sizeof(float) * one.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { fail("constant upload failed: %s", hipGetErrorString(e)); delete h; return nullptr; }
    }
    e = hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice);
    if (e != hipSuccess) { fail("job table upload failed: %s", hipGetErrorString(e)); delete h; return nullptr; }
    if (upload_vjp_tables(h)) { delete h; return nullptr; }
    return h;
}

extern "C" mmg_handle* mmg_attn_create(const mmg_config* cfg, int attn_dim, int n_words, void* d_workspace, int64_t workspace_bytes,
                                       float* d_params, float* d_grads, float* d_opt_state) {
    return create_impl(cfg, attn_dim, n_words, VattnDims(), d_workspace, workspace_bytes, d_params, d_grads, d_opt_state);
}
extern "C" mmg_handle* mmg_vattn_create(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, void* d_workspace, int64_t workspace_bytes,
                                        float* d_params, float* d_grads, float* d_opt_state) {
    return create_impl(cfg, 0, 0, VattnDims{attn_dim, n_feats, context_dim}, d_workspace, workspace_bytes, d_params, d_grads, d_opt_state);
}

// The data context g [B, G] of a visual-attention handle's next conversations (DEVICE memory, read in place by k_vattn_prep; the
// multi-minibatch entries advance through it by B * G per minibatch).  Host state only.  NULL clears it.
extern "C" int mmg_set_data_context(mmg_handle* h, const float* d_context) {
    if (!h) return fail("NULL handle");
    if (!h->vd.A) return fail("mmg_set_data_context: not a visual-attention handle (mmg_vattn_create with attn_dim > 0)");
    h->d_ctx = d_context;
    return 0;
}

// Sender.reset_state() for the agent-level entry: the next mmg_sender_forward forms HX / HG again, whatever its t.  Host state only.
extern "C" int mmg_vattn_reset_state(mmg_handle* h) {
    if (!h) return fail("NULL handle");
    if (!h->vd.A) return fail("mmg_vattn_reset_state: not a visual-attention handle (mmg_vattn_create with attn_dim > 0)");
    h->vattn_stale = true;
    return 0;
}

extern "C" mmg_handle* mmg_create(const mmg_config* cfg, void* d_workspace, int64_t workspace_bytes,
                                  float* d_params, float* d_grads, float* d_opt_state) {
    return mmg_attn_create(cfg, 0, 0, d_workspace, workspace_bytes, d_params, d_grads, d_opt_state);
}

// The description set of an attention handle: the word vectors go into the workspace (the GEMM operand of the per-word tables and of
// the y1 / d_d weight-gradient jobs), the segment table is built here from the lengths.  Blocking copies: a rare call, and nothing of
// the handle may be in flight while the set changes.
extern "C" int mmg_set_desc_set(mmg_handle* h, const float* d_set, const int32_t* lens, int n_words) {
    if (!h) return fail("NULL handle");
    if (!h->attn_dim) return fail("mmg_set_desc_set: not an attention handle (mmg_attn_create with attn_dim > 0)");
    if (!d_set || !lens) return fail("mmg_set_desc_set: set / lens must not be NULL");
    if (n_words != h->n_words) return fail("mmg_set_desc_set: %d words for a handle created for %d", n_words, h->n_words);
    const int D = h->dm.D;
    std::vector<int32_t> seg(D + 1), cls(n_words);
    int64_t o = 0;
    for (int d = 0; d < D; ++d) {
        if (lens[d] <= 0) return fail("mmg_set_desc_set: description %d has %d words (every class needs at least one: its softmax is over its own words)", d, (int)lens[d]);
        seg[d] = (int32_t)o;
        if (o + lens[d] > n_words) return fail("mmg_set_desc_set: the %d lengths sum to more than n_words = %d", D, n_words);
        for (int j = 0; j < lens[d]; ++j) cls[o + j] = d;
        o += lens[d];
    }
    if (o != n_words) return fail("mmg_set_desc_set: the %d lengths sum to %lld, n_words is %d", D, (long long)o, n_words);
    seg[D] = n_words;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h->at.tp.attn_set, d_set, sizeof(float) * (size_t)n_words * h->dm.V, hipMemcpyDeviceToDevice));
    HIP_OK(hipMemcpy(h->at.tp.attn_seg, seg.data(), sizeof(int32_t) * seg.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(h->at.tp.attn_cls, cls.data(), sizeof(int32_t) * cls.size(), hipMemcpyHostToDevice));
    h->set_ready = true;
    return 0;
}

// Gates of an attention handle: what it does not offer raises (never the plain receiver instead) ...
static int refuse_attn(const mmg_handle* h, const char* who) {
    if (h && h->attn_dim) return fail("%s is not available on a description-attention handle (desc_attn)", who);
    if (h && h->vd.A) return fail("%s is not available on a visual-attention handle (visual_attn)", who);
    return 0;
}
// ... and a conversation of a sender with attn_W_g needs the context
static int vattn_ready(const mmg_handle* h, const char* who) {
    if (h->vd.A && h->vd.G > 0 && !h->d_ctx) return fail("%s: visual_attn with a context needs the data context first (mmg_set_data_context)", who);
    return 0;
}
// x of minibatch i of a multi-minibatch entry: B * F features, times the locations of the map on a visual-attention handle
static size_t x_stride(const mmg_handle* h) { return (size_t)h->dm.B * h->dm.F * (h->vd.A ? h->vd.N : 1); }
static int launch_vattn_prep(mmg_handle* h, hipStream_t st, const float* d_x, const float* d_ctx) {
    Scope sc(h, st, "k_vattn_prep");
    VattnArgs va = h->va; va.ctx = d_ctx;
    const int tiles = vattn_prep_tiles(h->dm.B * va.N, va.A) + (va.G > 0 ? vattn_prep_tiles(h->dm.B, va.A) : 0);
    hipLaunchKernelGGL(k_vattn_prep, dim3(tiles), dim3(MMG_BLOCK), 0, st, h->dm, d_x, va);
    return launch_check("k_vattn_prep");
}
// ... and a conversation needs the description set
static int attn_ready(const mmg_handle* h, const char* who) {
    if (h->attn_dim && !h->set_ready) return fail("%s: desc_attn needs the description set first (mmg_set_desc_set)", who);
    return 0;
}
static int launch_attn_prep(mmg_handle* h, hipStream_t st) {
    Scope sc(h, st, "k_attn_prep");
    const int tiles = attn_prep_tiles(h->n_words, h->attn_dim) + 2 * attn_prep_tiles(h->n_words, h->dm.R);
    hipLaunchKernelGGL(k_attn_prep, dim3(tiles), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->at);
    return launch_check("k_attn_prep");
}

extern "C" void mmg_destroy(mmg_handle* h) { delete h; }      // (~mmg_handle releases the events and the pinned error word)

extern "C" int mmg_plan_text(const mmg_handle* h, char* out, int out_bytes) {
    if (!h) return fail("NULL handle");
    return plan_text(h, out, out_bytes);
}

// The pure passes of select_paths on a handle that owns nothing: the job table is built from addresses only, so the buffers
// are stand-in addresses that nothing dereferences.
extern "C" int mmg_plan_for(const mmg_config* cfg, const int32_t* caps, int n_caps, int flags, char* out, int out_bytes) {
    if (validate(cfg)) return -1;
    if (!caps || n_caps != MMG_PLAN_CAPS) return fail("mmg_plan_for: %d caps expected (MMG_CAP_*)", MMG_PLAN_CAPS);
    if (caps[MMG_CAP_N_CU] <= 0) return fail("mmg_plan_for: caps[MMG_CAP_N_CU] must be positive");
    float* const base = reinterpret_cast<float*>(uintptr_t(1) << 40);
    const std::unique_ptr<mmg_handle> owner(new_handle(*cfg, base, base, base, base));
    mmg_handle* h = owner.get();
    h->d_err = reinterpret_cast<uint32_t*>(base);           // (as a created handle has one; h_err stays NULL: nothing to release)
    h->no_roles = (flags & 1) != 0; h->flip_sen = (flags & 2) != 0; h->sender_var = (flags & 4) ? SV_PROD : 0;
    if (flags & 8) h->relax_tau_sen = h->relax_tau_rec = 1.f;
    if (flags & 256) h->noise_sigma_sen = h->noise_sigma_rec = 1.f;      // bit 8: Gaussian message noise (mmg_set_message_noise)
    h->train_mask = 15 & ~(flags >> 4);                     // bits 4-7: frozen agents (mmg_set_trainable's mask, inverted)
    const Switches w = read_switches();
    if (shape_pass(h, w)) return -1;
    memcpy(h->sel.caps, caps, sizeof(h->sel.caps));
    if (cfg->cu_budget > 0 && cfg->cu_budget < caps[MMG_CAP_N_CU]) h->sel.caps[MMG_CAP_N_CU] = cfg->cu_budget;
    if (decide(h, w)) return -1;
    return plan_text(h, out, out_bytes);
}

// The index arithmetic of k_game_fast's baseline roles (game_windows.h), as the kernel calls it, over a whole range at once.
static int game_window_args(const char* who, int nslots, int n) {
    if (nslots < 1 || nslots > GAME_WIN_MAX_SLOTS) return fail("%s: nslots must be 1..%d", who, GAME_WIN_MAX_SLOTS);
    if (n < 0 || n > GAME_WIN_PER_SLOT * nslots + 1) return fail("%s: n must be 0..%d * nslots + 1", who, GAME_WIN_PER_SLOT);
    return 0;
}
extern "C" int mmg_game_window_split(int nslots, int n, int32_t* kw, int32_t* slot) {
    if (game_window_args("mmg_game_window_split", nslots, n)) return -1;
    if (!kw || !slot) return fail("mmg_game_window_split: NULL output");
    const GameWinDiv d = game_win_div(nslots);
    for (int w = 0; w < n; ++w) { int k, s; game_win_split(d, w, k, s); kw[w] = k; slot[w] = s; }
    return 0;
}
extern "C" int mmg_game_window_counts(int nslots, int slot, int n, int32_t* count) {
    if (game_window_args("mmg_game_window_counts", nslots, n)) return -1;
    if (slot < 0 || slot >= nslots || !count) return fail("mmg_game_window_counts: slot must be 0..nslots - 1, count not NULL");
    const GameWinDiv d = game_win_div(nslots);
    for (int nw = 0; nw < n; ++nw) count[nw] = game_win_count(d, nw, slot);
    return 0;
}

extern "C" int mmg_set_profiling(mmg_handle* h, int enabled) {
    if (!h) return fail("NULL handle");
    h->profiling = enabled != 0; h->timers_used = 0;
    return 0;
}

extern "C" int mmg_get_kernel_times(mmg_handle* h, char* names, int names_bytes, float* ms, int max_kernels) {
    if (!h) return fail("NULL handle");
    int n = 0; std::string all;
    for (size_t i = 0; i < h->timers_used && n < max_kernels; ++i, ++n) {
        hipEventSynchronize(h->timers[i].t1);
        float t = 0.f; hipEventElapsedTime(&t, h->timers[i].t0, h->timers[i].t1);
        ms[n] = t;
        all += h->timers[i].name; all += ";";
    }
    if (names && names_bytes > 0) { strncpy(names, all.c_str(), names_bytes - 1); names[names_bytes - 1] = 0; }
    h->timers_used = 0;
    return n;
}

extern "C" int64_t mmg_log_snapshot_count(const mmg_config* cfg, int dump, int with_losses) {
    if (validate(cfg)) return -1;
    const int k = dump < cfg->batch ? (dump > 0 ? dump : 0) : cfg->batch;
    return log_snapshot_count(cfg->max_exchange, cfg->batch, cfg->w_dim, k, with_losses != 0);
}

extern "C" int mmg_log_snapshot(mmg_handle* h, const int64_t* d_target, int dump, int with_losses, double* d_out, void* stream) {
    if (!h) return fail("NULL handle");
    if (!d_out) return fail("out must not be NULL");
    const int k = dump < h->dm.B ? (dump > 0 ? dump : 0) : h->dm.B;
    if (!with_losses && k == 0) return 0;
    Scope sc(h, (hipStream_t)stream, "k_log_snapshot");
    hipLaunchKernelGGL(k_log_snapshot, dim3(h->dm.T + 2), dim3(MMG_BLOCK), 0, (hipStream_t)stream, h->dm, h->tp, d_target, k, with_losses ? 1 : 0, d_out);
    return launch_check("k_log_snapshot");
}

static int launch_baselines_fused(mmg_handle* h, hipStream_t st) {
    const Dims& d = h->dm; const Tape& tp = h->tp; const Params& P = h->P;
    const int rows = d.T * d.B;
    BasArgs rec, sen;
    memset(&rec, 0, sizeof(rec)); memset(&sen, 0, sizeof(sen));
    rec.rows = rows; rec.x1 = tp.z; rec.ld1 = d.W; rec.k1 = d.W;
    rec.x2 = tp.h + (size_t)d.B * d.R; rec.ld2 = d.R; rec.k2 = d.R;
    rec.W1 = P.p[BR_L1_W]; rec.ldw = d.W + d.R; rec.col0 = 0; rec.b1 = P.p[BR_L1_B];
    rec.W2 = P.p[BR_L2_W]; rec.b2 = P.p[BR_L2_B]; rec.hid = tp.hid_r; rec.score = tp.br;
    sen.rows = rows; sen.x1 = tp.hx; sen.ld1 = d.H; sen.k1 = d.H; sen.mod1 = d.B;      // h_x is per sample, not per step
    if (h->sel.vattn) { sen.x1 = h->va.tp.vattn_hx; sen.mod1 = 0; }                    // (visual attention: per step, model.py:832-836)
    sen.x2 = tp.zr; sen.ld2 = d.W; sen.k2 = d.W;
    sen.W1 = P.p[BS_L1_W]; sen.ldw = d.H + d.W; sen.col0 = 0; sen.b1 = P.p[BS_L1_B];
    sen.W2 = P.p[BS_L2_W]; sen.b2 = P.p[BS_L2_B]; sen.hid = tp.hid_s; sen.score = tp.bs;
    Scope sc(h, st, "k_baselines");
    hipLaunchKernelGGL(k_baselines, dim3((rows + 15) / 16, 2), dim3(MMG_BLOCK), 0, st, d.K, rec, sen);
    return launch_check("k_baselines");
}

// The whole-conversation launch arguments every forward starts from (the fused step included)
static ConvArgs conv_args(const mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc, const float* d_u_z,
                          const float* d_u_s, const float* d_u_w, uint64_t seed, int train, int run_all) {
    ConvArgs ar; memset(&ar, 0, sizeof(ar));
    ar.x = d_x; ar.target = d_target; ar.desc = d_desc; ar.u_z = d_u_z; ar.u_s = d_u_s; ar.u_w = d_u_w; ar.seed = seed;
    ar.train = train; ar.run_all = run_all; ar.t_begin = 0; ar.t_end = h->dm.T; ar.phases = 3; ar.sprod_first = 1;
    return ar;
}

// Message flips of this call (mmg_set_message_flipout), by value: training conversations always, evaluation ones under flipout_dev.
// new_conv: the call enqueues a whole evaluation conversation (it takes the next evaluation count); the agent-level entries draw
// with the count of the conversation the last mmg_sender_forward(t = 0) began.
static void flip_args(mmg_handle* h, ConvArgs& ar, uint64_t seed, int train, bool new_conv) {
    if (!h->sel.flip || (!train && !h->flip_dev)) return;
    ar.flip_on = (h->flip_sen ? 1 : 0) | (h->flip_rec ? 2 : 0) | (train ? 0 : 4);
    ar.flip_pz = h->flip_p_sen; ar.flip_pw = h->flip_p_rec;
    ar.flip_key = train ? seed : h->flip_eval_seed;
    if (!train) ar.flip_c1 = new_conv ? h->flip_evals++ : (h->flip_evals ? h->flip_evals - 1u : 0u);
}

// Gaussian message noise of this call (mmg_set_message_noise), by value and in the flip fields (kernels_fwd.h: ConvArgs; a handle's flips
// act on binary messages and its noise on continuous ones, so one of the two fills them): training conversations always, evaluation ones
// under noise_dev.  new_conv as for flip_args.
static void noise_args(mmg_handle* h, ConvArgs& ar, uint64_t seed, int train, bool new_conv) {
    if (!h->sel.noise || (!train && !h->noise_dev)) return;
    ar.flip_on = (h->noise_sigma_sen > 0.f ? 1 : 0) | (h->noise_sigma_rec > 0.f ? 2 : 0) | (train ? 0 : 4);
    ar.flip_pz = h->noise_sigma_sen; ar.flip_pw = h->noise_sigma_rec;
    ar.flip_key = train ? seed : h->noise_eval_seed;
    if (!train) ar.flip_c1 = new_conv ? h->noise_evals++ : (h->noise_evals ? h->noise_evals - 1u : 0u);
}

// Relaxed messages of this call (mmg_set_message_relaxation), by value; only the RELAX instantiations read them, in training conversations
static void relax_args(const mmg_handle* h, ConvArgs& ar) {
    if (!h->sel.relax) return;
    ar.relax_tau_z = h->relax_tau_sen; ar.relax_tau_w = h->relax_tau_rec; ar.relax_hard = h->relax_hard ? 1 : 0;
}
// ... and what such a handle does not train with: REINFORCE seeds and detached graphs
static int refuse_relax(const mmg_handle* h, const char* who) {
    if (h && h->sel.relax)
        return fail("%s is not available while messages are relaxed (mmg_set_message_relaxation): such a handle trains through "
                    "mmg_exchange_vjp_channel; mmg_set_message_relaxation(h, 0, 0, 0) clears the setting", who);
    return 0;
}

// FAM_TILE: one of the plan's seven outcomes (host_select.h: plan_launches).  The outcome is known BEFORE a timing scope opens.
static int launch_conv_tile(mmg_handle* h, hipStream_t st, ConvArgs ar) {
    const Dims& d = h->dm; const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    const int tiles = p.tiles, free_run = (ar.train && !ar.run_all) ? 1 : 0;
    const int bt = (p.basehx_rides && free_run) ? p.basehx_tiles : 0; const int skip = (p.skip_ok && free_run) ? 1 : 0;   // bt: basehx tiles for k_baselines4 as trailing workgroups
    ar.ns1 = p.ns1; ar.ns2 = p.ns2; ar.rsample = p.rsample;
    switch (p.tile_fwd) {
    case TF_SPLIT: {
        Scope sc(h, st, "k_conv_split");
        ar.nhelp = s.split_nh; ar.per = s.split_per;
        hipLaunchKernelGGL(k_conv_split<512>, dim3(tiles * (1 + ar.nhelp)), dim3(512), s.split_smem, st, h->dm, h->P, h->tp, ar, tiles);
        return launch_check("k_conv_split");
    }
    case TF_WHOLE: {
        Scope sc(h, st, "k_conv_tile");
        hipLaunchKernelGGL(p.conv_tile_fn, dim3(tiles), dim3(s.tile_nt), s.tile_smem, st, h->dm, h->P, h->tp, ar);
        return launch_check("k_conv_tile");
    }
    case TF_PERSIST_SAMPLE: case TF_PERSIST_TILE: {
        Scope sc(h, st, "k_conv_persist");
        ar.phases = 2; ar.persist = 1;
        const int span = p.chunk_tiles * MMG_TM;
        if (p.tile_fwd == TF_PERSIST_TILE)               // every tile's roles in one launch
            hipLaunchKernelGGL(p.persist_fn, dim3(tiles * p.chunk_roles), dim3(512), s.persist_smem, st, h->dm, h->P, h->tp, ar, tiles);
        else for (int c = 0; c < p.n_chunk && c * span < d.B; ++c) {      // per-sample receiver roles: consecutive launches over sample ranges
            ar.b_begin = c * span; ar.b_count = std::min(d.B - ar.b_begin, span);
            hipLaunchKernelGGL(p.persist_fn, dim3(ar.b_count + sample_tiles(ar.b_count) * (ar.ns1 + ar.ns2) + bt), dim3(512), s.persist_smem, st, h->dm, h->P, h->tp, ar, tiles);
        }
        h->fwd.basehx_ready = bt > 0;
        return launch_check("k_conv_persist");
    }
    case TF_RC_PERSIST: case TF_RC_STEP: {
        Scope sc(h, st, "k_conv_rc");
        ar.phases = 2;
        if (p.tile_fwd == TF_RC_PERSIST) {               // all roles co-resident: up to two consecutive launches over tile ranges
            for (int t0 = 0; t0 < tiles; t0 += p.chunk_tiles) {
                const int nt = std::min(tiles - t0, p.chunk_tiles);
                hipLaunchKernelGGL(k_rc_persist, dim3(nt * p.chunk_roles + bt), dim3(256), 0, st, h->dm, h->P, h->tp, ar, nt, t0);
            }
            h->fwd.basehx_ready = bt > 0;
            return launch_check("k_rc_persist");
        }
        for (int t = 0; t < d.T; ++t) {                  // the receiver step of a tile as three launches over 16-unit / 16-bit slices
            hipLaunchKernelGGL(k_send_s1, dim3(p.s1_grid), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, t, skip);
            hipLaunchKernelGGL(k_send_s2, dim3(p.s2_grid), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, ar, t, skip);
            hipLaunchKernelGGL(k_rc_gru, dim3(tiles * p.rc_nj), dim3(256), 0, st, h->dm, h->P, h->tp, ar, t, skip);
            hipLaunchKernelGGL(k_rc_heads, dim3(tiles * p.rc_nj), dim3(256), 0, st, h->dm, h->P, h->tp, ar, t, skip);
            hipLaunchKernelGGL(k_rc_query, dim3(tiles * p.rc_njw), dim3(256), 0, st, h->dm, h->P, h->tp, ar, t, skip);
        }
        hipLaunchKernelGGL(k_rc_tail, dim3(tiles), dim3(256), 0, st, h->dm, h->P, h->tp, ar);
        return launch_check("k_conv_rc");
    }
    case TF_STEP:                                        // per-step launches: no co-residency needed (any device, any batch)
        for (int t = 0; t < d.T; ++t) {
            { Scope sc(h, st, "k_send_s1"); hipLaunchKernelGGL(k_send_s1, dim3(p.s1_grid), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, t, skip); }
            { Scope sc(h, st, "k_send_s2"); hipLaunchKernelGGL(k_send_s2, dim3(p.s2_grid), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, ar, t, skip); }
            ar.phases = 2; ar.t_begin = t; ar.t_end = t + 1;
            { Scope sc(h, st, "k_conv_tile"); hipLaunchKernelGGL(p.conv_tile_fn, dim3(tiles), dim3(s.tile_nt), s.tile_smem, st, h->dm, h->P, h->tp, ar); }
            if (launch_check("k_conv_tile (step)")) return -1;
        }
    }
    return 0;
}

// FAM_MC.  lean: the training-minimal continuous pass, the only one the pair kernel serves
static int launch_conv_mc(mmg_handle* h, hipStream_t st, ConvArgs ar) {
    const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    Scope sc(h, st, s.noise ? "k_conversation_mc3_noise" : "k_conversation_mc");
    ar.per = s.mc_per; ar.l2_handoff = (s.mc_xcd && h->xcd_rule_ok) ? 1 : 0;
    if (p.mc3p_wins && ar.lean)      // two sample tiles per workgroup, half a step apart (kernels_mc3p.h)
        hipLaunchKernelGGL((k_conversation_mc3p<256, 32, 64, 100, 64>), dim3(p.mc3p_grid), dim3(256), mc3p_lds_bytes(h->dm.T), st, h->dm, h->P, h->tp, ar, p.mc_ntile, ar.y_last_only);
    else if (s.noise)                // (decide() keeps the family for a noise handle only with mc3)
        hipLaunchKernelGGL((k_conversation_mc3_noise<256, 32, 64, 100, 64>), dim3(p.mc_grid), dim3(256), mc3_lds_bytes(), st, h->dm, h->P, h->tp, ar, p.mc_ntile, s.mc_xcd, ar.y_last_only);
    else if (s.mc3_ok)
        hipLaunchKernelGGL((k_conversation_mc3<256, 32, 64, 100, 64>), dim3(p.mc_grid), dim3(256), mc3_lds_bytes(), st, h->dm, h->P, h->tp, ar, p.mc_ntile, s.mc_xcd, ar.y_last_only);
    else
        hipLaunchKernelGGL((k_conversation_mc<256, 32, 64, 100, 64>), dim3(p.mc_grid), dim3(512), 0, st, h->dm, h->P, h->tp, ar, p.mc_ntile, s.mc_xcd, ar.y_last_only);
    return launch_check("k_conversation_mc");
}

// FAM_FAST (k_conversation_fast3 with its optional prep / basehx roles) and FAM_GENERIC (k_conversation)
static int launch_conv_sample(mmg_handle* h, hipStream_t st, ConvArgs ar, bool base_ready) {
    const Dims& d = h->dm; const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    Scope sc(h, st, p.conv_name);
    if (s.family == FAM_FAST) {
        ar.nprep = p.merge_prep ? p.nprep_hx : 0; ar.prep_cpb = s.prep_cpb; ar.nbase = base_ready ? p.basehx_tiles : 0;
        hipLaunchKernelGGL(p.fast_fn, dim3(d.B + ar.nbase + (p.merge_prep ? ar.nprep + 1 : 0)), dim3(256), p.fast_smem, st, h->dm, h->P, h->tp, ar);
    } else if (s.attn)
        hipLaunchKernelGGL(p.conv_attn_fn, dim3(d.B), dim3(s.conv_threads), s.conv_smem, st, h->dm, h->P, h->tp, ar, h->at);
    else if (s.vattn)
        hipLaunchKernelGGL(p.conv_vattn_fn, dim3(d.B), dim3(s.conv_threads), s.conv_smem, st, h->dm, h->P, h->tp, ar, h->va);
    else
        hipLaunchKernelGGL(p.conv_fn, dim3(d.B), dim3(s.conv_threads), s.conv_smem, st, h->dm, h->P, h->tp, ar);
    return launch_check("k_conversation");
}

// The baselines of a training forward.  all_rows (exchange()): every row, scores materialised directly; else over the live rows --
// left to the backward launch (fused step) or to k_bas_stats (phased step) where the plan allows, or the plan's standalone kernel
static int launch_baselines(mmg_handle* h, hipStream_t st, bool all_rows, bool defer_bas, bool base_ready) {
    const Dims& d = h->dm; const LaunchPlan& p = h->sel.plan;
    if (all_rows || h->sel.vattn) return launch_baselines_fused(h, st);    // (visual attention: the live-row kernels hoist h_x over the steps)
    h->fwd.scores_in_parts = true;
    if (base_ready && defer_bas && p.bas_defer_ok) { h->fwd.bas_deferred = true; return 0; }
    if (base_ready && !defer_bas && p.bas_pending_ok) { h->fwd.bas_pending = true; return 0; }
    Scope sc(h, st, "k_baselines");
    if (p.bas_kernel == BAS_TILE4 && !h->fwd.basehx_ready)     // basehx did not ride along the conversation: a GEMM launch first
        hipLaunchKernelGGL(k_gemm_nt, dim3(p.basehx_tiles), dim3(MMG_BLOCK), 0, st, (const float*)h->tp.hx, d.H, (const float*)h->P.p[BS_L1_W], d.H + d.W, (const float*)nullptr, h->tp.basehx, d.K, d.B, d.K, d.H);
    if (p.bas_kernel == BAS_ALL2)
        hipLaunchKernelGGL(k_baselines2, dim3((d.B + 15) / 16, (d.K + 63) / 64, p.bas2_z), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, 1, base_ready ? 1 : 0);
    else
        hipLaunchKernelGGL(p.bas_kernel == BAS_TILE4 ? k_baselines4 : k_baselines3, dim3((d.T * d.B + 15) / 16, (d.K + 63) / 64, 2), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp);
    return launch_check("k_baselines");
}

// defer_bas (the fused step's forward): the baselines may ride in the backward launch
static int exchange_forward_impl(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc, const float* d_u_z,
                                 const float* d_u_s, const float* d_u_w, uint64_t seed, int train, TapeMode mode, void* stream, bool defer_bas = false,
                                 int64_t mb = 0) {
    if (!d_x || !d_desc) return fail("x / desc must not be NULL");
    if (attn_ready(h, "exchange") || vattn_ready(h, "exchange")) return -1;
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->dm; const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    // (visual attention: x is the [B, C, N] map -- no h_x tiles in k_prep, the conversation forms h_x per step; mb: the minibatch of a
    //  multi-minibatch entry, whose rows of the context are read)
    if (!p.merge_prep && launch_prep(h, st, d_desc, s.vattn ? nullptr : d_x, train ? 1 : 0)) return -1;
    if (s.attn && launch_attn_prep(h, st)) return -1;
    h->ctx_cur = (s.vattn && h->vd.G > 0) ? h->d_ctx + (size_t)mb * d.B * h->vd.G : nullptr;
    if (s.vattn && launch_vattn_prep(h, st, d_x, h->ctx_cur)) return -1;
    h->vattn_stale = true;                         // (the tables are this conversation's: an agent-level call forms its own)
    if (h->corrupt_on && train) return fail("a message corruption mask is set: training conversations are not corrupted (mmg_set_message_corruption(h, NULL, 0) clears it)");
    // TAPE_LOG (the minibatches whose log block reads the whole tape): the CONVERSATION runs every sample through all steps, everything else
    // is the training step's -- the baselines over the live rows only, in the statistics / backward launch (the log block prints no baseline score;
    // the all-rows baselines launch of TAPE_ALL costs 55 us at config 2).  Register-resident agents of a training pass only: other paths take it as TAPE_ALL.
    const bool bas = train && d.use_binary, tape_all = mode == TAPE_LOG && bas && s.family == FAM_FAST;
    const bool all_rows = mode == TAPE_ALL || (mode == TAPE_LOG && !tape_all);
    ConvArgs ar = conv_args(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, train, (all_rows || tape_all) ? 1 : 0);
    // TAPE_MINIMAL: as TAPE_TO_STOP, and the class logits y[t] of the steps before the output step are not kept
    ar.y_last_only = (mode == TAPE_MINIMAL && d.fixed) ? 1 : 0;
    ar.lean = (mode == TAPE_MINIMAL && !d.use_binary) ? 1 : 0;
    if (h->corrupt_on) { ar.corrupt_on = 1; memcpy(ar.corrupt, h->corrupt, sizeof(ar.corrupt)); }
    flip_args(h, ar, seed, train, true);
    noise_args(h, ar, seed, train, true);
    ar.sender_var = s.variant;
    relax_args(h, ar);
    h->fwd = ForwardState();
    const bool base_ready = p.fwd_basehx && bas && !all_rows;
    switch (s.family) {
    case FAM_TILE: if (launch_conv_tile(h, st, ar)) return -1; break;
    case FAM_MC: if (launch_conv_mc(h, st, ar)) return -1; break;
    default: if (launch_conv_sample(h, st, ar, base_ready)) return -1;
    }
    return bas ? launch_baselines(h, st, all_rows, defer_bas, base_ready) : 0;
}

extern "C" int mmg_exchange_forward(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                                    const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed,
                                    int train, int run_all_steps, void* stream) {
    if (!h) return fail("NULL handle");
    auto fwd = [&](int64_t) { return exchange_forward_impl(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, train, tape_mode(run_all_steps), stream); };
    if (!train) return fwd(0);
    if (begin_minibatch(h, "mmg_exchange_forward(train = 1)")) return -1;
    return run_minibatches(h, 1, stream, fwd);             // a training forward pass starts a minibatch
}

// ---------------------------------------------------------------------------------------------
// mmg_eval_steps: n consecutive dev batches of eval_dev (model.py:620-691) enqueued by ONE call -- the eval-mode conversation
// (train = 0, run-all: no Philox draw, the minibatch counter stays) and behind each one k_eval_reduce (kernels_eval.h), which
// adds the batch's hits / confusion matrix / classes seen to the caller's accumulator and writes its conversation lengths,
// step count and Hamming counts.  Not a minibatch start: no error gate, and nothing here waits inside a launch.
// mmg_eval_steps_profile: the same call with one more reduction launch per batch, k_eval_profile, which adds the batch's
// communication profile (per-step ranks, output steps per class, the per-class code book) to a second accumulator.
// ---------------------------------------------------------------------------------------------
extern "C" int64_t mmg_eval_acc_count(const mmg_config* cfg) {
    if (validate(cfg)) return -1;
    return eval_acc_count(cfg->n_classes);
}

extern "C" int64_t mmg_eval_profile_count(const mmg_config* cfg) {
    if (validate(cfg)) return -1;
    return eval_profile_count(cfg->n_classes, cfg->max_exchange, cfg->w_dim);
}

extern "C" int64_t mmg_eval_code_words(const mmg_config* cfg) {
    if (validate(cfg)) return -1;
    if (!cfg->use_binary) return fail("mmg_eval_code_words: continuous messages (use_binary == 0) have no bits to pack");
    return eval_code_words(cfg->max_exchange, cfg->w_dim);
}

// d_prof != NULL (mmg_eval_steps_profile): one k_eval_profile launch behind every k_eval_reduce; d_codes != NULL (mmg_eval_steps_codes):
// one k_eval_codes launch behind those, which writes rows [row0 + i B, row0 + (i + 1) B) of d_codes / d_meta; both NULL: the launches
// of mmg_eval_steps alone
static int eval_steps_impl(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                           int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof, void* stream,
                           uint32_t* d_codes = nullptr, int32_t* d_meta = nullptr, int64_t row0 = 0) {
    if (!h) return fail("NULL handle");
    if (!d_x || !d_target || !d_desc || !d_acc || !d_len || !d_batch) return fail("mmg_eval_steps: x / target / desc / acc / len / batch must not be NULL");
    if (top_k < 1) return fail("mmg_eval_steps: top_k must be >= 1 (got %d)", top_k);
    if (n < 0) return fail("mmg_eval_steps: n must be >= 0");
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->dm;
    const int nsb = eval_sample_blocks(d.B);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t* tgt = d_target + (size_t)i * d.B;
        if (exchange_forward_impl(h, d_x + (size_t)i * x_stride(h), tgt, d_desc, nullptr, nullptr, nullptr, 0, 0, TAPE_ALL, stream, false, i)) return -1;
        {
            Scope sc(h, st, "k_eval_reduce");
            hipLaunchKernelGGL(k_eval_reduce, dim3(nsb + 2 * d.T), dim3(MMG_BLOCK), 0, st, h->dm, h->tp, tgt, top_k, d_acc,
                               d_len + (size_t)i * d.B, d_batch + (size_t)i * (1 + 2 * d.T), nsb);
            if (launch_check("k_eval_reduce")) return -1;
        }
        if (d_prof) {
            Scope sc(h, st, "k_eval_profile");
            hipLaunchKernelGGL(k_eval_profile, dim3(nsb), dim3(MMG_BLOCK), 0, st, h->dm, h->tp, tgt, top_k, d_prof, nsb);
            if (launch_check("k_eval_profile")) return -1;
        }
        if (d_codes) {
            const size_t row = (size_t)row0 + (size_t)i * d.B;
            Scope sc(h, st, "k_eval_codes");
            hipLaunchKernelGGL(k_eval_codes, dim3(nsb), dim3(MMG_BLOCK), 0, st, h->dm, h->tp, tgt,
                               d_codes + row * (size_t)eval_code_words(d.T, d.W), d_meta + row * 2, nsb);
            if (launch_check("k_eval_codes")) return -1;
        }
    }
    return 0;
}

extern "C" int mmg_eval_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                              int64_t* d_acc, int32_t* d_len, int64_t* d_batch, void* stream) {
    return eval_steps_impl(h, d_x, d_target, n, d_desc, top_k, d_acc, d_len, d_batch, nullptr, stream);
}

extern "C" int mmg_eval_steps_profile(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                                      int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof, void* stream) {
    if (!d_prof) return fail("mmg_eval_steps_profile: prof must not be NULL (mmg_eval_steps is the entry without a profile)");
    return eval_steps_impl(h, d_x, d_target, n, d_desc, top_k, d_acc, d_len, d_batch, d_prof, stream);
}

extern "C" int mmg_eval_steps_codes(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                                    int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof, uint32_t* d_codes, int32_t* d_meta,
                                    int64_t row0, int64_t cap_rows, void* stream) {
    if (!h) return fail("NULL handle");
    if (!h->dm.use_binary) return fail("mmg_eval_steps_codes: continuous messages (use_binary == 0) have no bits to pack");
    if (!d_codes || !d_meta) return fail("mmg_eval_steps_codes: codes / meta must not be NULL (mmg_eval_steps[_profile] are the entries without codes)");
    if (row0 < 0) return fail("mmg_eval_steps_codes: row0 must be >= 0 (got %lld)", (long long)row0);
    if (n > 0 && (n > (INT64_MAX - row0) / h->dm.B || row0 + n * h->dm.B > cap_rows))
        return fail("mmg_eval_steps_codes: rows [%lld, %lld + %lld * %d) do not fit the %lld rows of codes / meta", (long long)row0,
                    (long long)row0, (long long)n, h->dm.B, (long long)cap_rows);
    return eval_steps_impl(h, d_x, d_target, n, d_desc, top_k, d_acc, d_len, d_batch, d_prof, stream, d_codes, d_meta, row0);
}

// The evaluation mask of -bit_flip (include/mmg.h): host state only; exchange_forward_impl copies it into the launch arguments.
extern "C" int mmg_set_message_corruption(mmg_handle* h, const uint8_t* mask, int n) {
    if (!h) return fail("NULL handle");
    if (!mask) {
        h->corrupt_on = false;
        memset(h->corrupt, 0, sizeof(h->corrupt));
        return 0;
    }
    if (n != h->dm.W) return fail("mmg_set_message_corruption: the mask has %d entries, the message %d bits", n, h->dm.W);
    uint32_t words[MMG_BLOCK / 32] = {};
    for (int j = 0; j < n; ++j) {
        if (mask[j] > 1) return fail("mmg_set_message_corruption: mask[%d] = %d (0 or 1 expected)", j, (int)mask[j]);
        words[j >> 5] |= (uint32_t)mask[j] << (j & 31);
    }
    memcpy(h->corrupt, words, sizeof(words));
    h->corrupt_on = true;
    return 0;
}

// Random message flips (include/mmg.h): host state; re-runs the selection, since a flipping handle is served by k_conversation_fast3 /
// k_conversation only (host_select.h).  The job table goes to the device again only where the family changed it.
extern "C" int mmg_set_message_flipout(mmg_handle* h, int has_sen, float p_sen, int has_rec, float p_rec, int flipout_dev, uint64_t eval_seed) {
    if (!h) return fail("NULL handle");
    if ((has_sen || has_rec) && refuse_attn(h, "mmg_set_message_flipout")) return -1;
    if (has_sen && !(p_sen >= 0.f && p_sen <= 1.f)) return fail("mmg_set_message_flipout: p_sen = %g is not a probability in [0, 1]", (double)p_sen);
    if (has_rec && !(p_rec >= 0.f && p_rec <= 1.f)) return fail("mmg_set_message_flipout: p_rec = %g is not a probability in [0, 1]", (double)p_rec);
    const bool o_sen = h->flip_sen, o_rec = h->flip_rec, o_dev = h->flip_dev; const float o_ps = h->flip_p_sen, o_pr = h->flip_p_rec;
    const uint64_t o_seed = h->flip_eval_seed; const uint32_t o_evals = h->flip_evals;
    auto set = [&](bool sen, float ps, bool rec, float pr, bool dev, uint64_t sd, uint32_t ev) {
        h->flip_sen = sen; h->flip_p_sen = sen ? ps : 0.f; h->flip_rec = rec; h->flip_p_rec = rec ? pr : 0.f;
        h->flip_dev = dev && (sen || rec); h->flip_eval_seed = sd; h->flip_evals = ev;
    };
    if ((has_sen || has_rec) && h->sender_var)
        return fail("mmg_set_message_flipout: the handle has a sender variant (mmg_set_sender_variant); flips and a variant do not combine");
    if ((has_sen || has_rec) && h->relax_tau_sen > 0.f)
        return fail("mmg_set_message_flipout: the handle has relaxed messages (mmg_set_message_relaxation); a flip of a relaxed message is not defined");
    set(has_sen != 0, p_sen, has_rec != 0, p_rec, flipout_dev != 0, eval_seed, 0u);
    if (((h->flip_sen || h->flip_rec) && h->dm.use_binary) == h->sel.flip) return 0;        // same routing: nothing to select
    const JobTable old = h->jt;
    if (select_paths(h)) {
        const std::string why = g_err;
        set(o_sen, o_ps, o_rec, o_pr, o_dev, o_seed, o_evals);
        select_paths(h);
        return fail("mmg_set_message_flipout: %s", why.c_str());
    }
    if (memcmp(&old, &h->jt, sizeof(JobTable)) != 0) {
        HIP_OK(hipDeviceSynchronize());                  // (rare: nothing may read the old table while the new one lands)
        HIP_OK(hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice));
    }
    return 0;
}

// The sender's communication ablations (include/mmg.h): host state; re-runs the selection, since a variant handle is served by the generic
// per-sample family only (host_select.h).  The job table goes to the device again only where the family changed it.
extern "C" int mmg_set_sender_variant(mmg_handle* h, int mix, int ignore_code, int ignore_receiver) {
    if (!h) return fail("NULL handle");
    if (mix != MMG_MIX_SUM && mix != MMG_MIX_PROD)
        return fail("mmg_set_sender_variant: mix = %d is not MMG_MIX_SUM or MMG_MIX_PROD (-sender_mix mou needs a 4H binary layer, another parameter layout)", mix);
    const int want = (mix == MMG_MIX_PROD ? SV_PROD : 0) | (ignore_code ? SV_IGNORE_CODE : 0) | (ignore_receiver ? SV_IGNORE_REC : 0);
    if (want && refuse_attn(h, "mmg_set_sender_variant")) return -1;
    if (want && (h->flip_sen || h->flip_rec))
        return fail("mmg_set_sender_variant: the handle has message flips (mmg_set_message_flipout); flips and a variant do not combine");
    if (want && (h->noise_sigma_sen > 0.f || h->noise_sigma_rec > 0.f))
        return fail("mmg_set_sender_variant: the handle has message noise (mmg_set_message_noise); noise and a variant do not combine");
    if (want && h->relax_tau_sen > 0.f)
        return fail("mmg_set_sender_variant: the handle has relaxed messages (mmg_set_message_relaxation); the joint VJP does not form the variants");
    const int old_var = h->sender_var;
    h->sender_var = want;
    const int eff = want & (h->dm.use_binary ? (SV_PROD | SV_IGNORE_CODE | SV_IGNORE_REC) : (SV_PROD | SV_IGNORE_CODE));
    if (eff == h->sel.variant) return 0;                 // same routing and the same kernels: nothing to select
    const JobTable old = h->jt;
    if (select_paths(h)) {
        const std::string why = g_err;
        h->sender_var = old_var;
        select_paths(h);
        return fail("mmg_set_sender_variant: %s", why.c_str());
    }
    if (memcmp(&old, &h->jt, sizeof(JobTable)) != 0) {
        HIP_OK(hipDeviceSynchronize());                  // (rare: nothing may read the old table while the new one lands)
        HIP_OK(hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice));
    }
    return 0;
}

// Relaxed messages (include/mmg.h): host state; re-runs the selection only when the relaxed state itself changes, since a relaxed handle is served
// by the generic per-sample family only (host_select.h) -- a call that only moves the temperatures selects nothing.
extern "C" int mmg_set_message_relaxation(mmg_handle* h, float tau_sen, float tau_rec, int hard) {
    if (!h) return fail("NULL handle");
    if (!(tau_sen >= 0.f) || !(tau_rec >= 0.f))          // (NaN fails both compares)
        return fail("mmg_set_message_relaxation: tau_sen = %g, tau_rec = %g: temperatures must be positive (both 0 clears the setting)", (double)tau_sen, (double)tau_rec);
    if ((tau_sen == 0.f) != (tau_rec == 0.f))
        return fail("mmg_set_message_relaxation: tau_sen = %g, tau_rec = %g: both positive, or both 0 to clear the setting", (double)tau_sen, (double)tau_rec);
    const bool on = tau_sen > 0.f;
    if (on) {
        if (!h->dm.use_binary) return fail("mmg_set_message_relaxation: binary messages only (use_binary = 0: the messages are the logits, already differentiable)");
        if (h->flip_sen || h->flip_rec) return fail("mmg_set_message_relaxation: the handle has message flips (mmg_set_message_flipout)");
        if (h->sender_var) return fail("mmg_set_message_relaxation: the handle has a sender variant (mmg_set_sender_variant)");
        if (refuse_attn(h, "mmg_set_message_relaxation")) return -1;
    }
    const float o_sen = h->relax_tau_sen, o_rec = h->relax_tau_rec; const bool o_hard = h->relax_hard;
    h->relax_tau_sen = tau_sen; h->relax_tau_rec = tau_rec; h->relax_hard = on && hard != 0;
    if (on == h->sel.relax) return 0;                    // same routing: nothing to select
    const JobTable old = h->jt;
    if (select_paths(h)) {
        const std::string why = g_err;
        h->relax_tau_sen = o_sen; h->relax_tau_rec = o_rec; h->relax_hard = o_hard;
        select_paths(h);
        return fail("mmg_set_message_relaxation: %s", why.c_str());
    }
    if (memcmp(&old, &h->jt, sizeof(JobTable)) != 0) {
        HIP_OK(hipDeviceSynchronize());                  // (rare: nothing may read the old table while the new one lands)
        HIP_OK(hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice));
    }
    return 0;
}

// Gaussian message noise (include/mmg.h): host state; re-runs the selection only when the noisy state itself changes, since a noise handle is
// served by k_conversation_noise / k_conversation_mc3_noise only (host_select.h) -- a call that only moves the sigmas selects nothing.
extern "C" int mmg_set_message_noise(mmg_handle* h, float sigma_sen, float sigma_rec, int noise_dev, uint64_t eval_seed) {
    if (!h) return fail("NULL handle");
    if (!(sigma_sen >= 0.f) || !(sigma_rec >= 0.f) || std::isinf(sigma_sen) || std::isinf(sigma_rec))          // (NaN fails the compares)
        return fail("mmg_set_message_noise: sigma_sen = %g, sigma_rec = %g: a standard deviation is finite and not negative (both 0 clears the setting)",
                    (double)sigma_sen, (double)sigma_rec);
    const bool on = sigma_sen > 0.f || sigma_rec > 0.f;
    if (on) {
        if (h->dm.use_binary)
            return fail("mmg_set_message_noise: continuous messages only (use_binary = 1: mmg_set_message_flipout is the noisy channel of binary messages)");
        if (refuse_attn(h, "mmg_set_message_noise")) return -1;
        if (h->sender_var) return fail("mmg_set_message_noise: the handle has a sender variant (mmg_set_sender_variant); noise and a variant do not combine");
    }
    const float o_sen = h->noise_sigma_sen, o_rec = h->noise_sigma_rec; const bool o_dev = h->noise_dev;
    const uint64_t o_seed = h->noise_eval_seed; const uint32_t o_evals = h->noise_evals;
    h->noise_sigma_sen = sigma_sen; h->noise_sigma_rec = sigma_rec; h->noise_dev = on && noise_dev != 0;
    h->noise_eval_seed = eval_seed; h->noise_evals = 0u;
    if (on == h->sel.noise) return 0;                    // same routing: nothing to select
    const JobTable old = h->jt;
    if (select_paths(h)) {
        const std::string why = g_err;
        h->noise_sigma_sen = o_sen; h->noise_sigma_rec = o_rec; h->noise_dev = o_dev; h->noise_eval_seed = o_seed; h->noise_evals = o_evals;
        select_paths(h);
        return fail("mmg_set_message_noise: %s", why.c_str());
    }
    if (memcmp(&old, &h->jt, sizeof(JobTable)) != 0) {
        HIP_OK(hipDeviceSynchronize());                  // (rare: nothing may read the old table while the new one lands)
        HIP_OK(hipMemcpy(h->d_jt, &h->jt, sizeof(JobTable), hipMemcpyHostToDevice));
    }
    return 0;
}

// Training controls (include/mmg.h): host state, read where the next minibatch's launches are enqueued -- the mask, the learning rate and
// the entropy weights travel as kernel arguments (OptArgs, Dims).  No kernel is re-selected and nothing synchronises.  (The values are
// checked before the handle: a bad value reads the same with or without one.)
extern "C" int mmg_set_trainable(mmg_handle* h, int mask) {
    if (mask & ~15) return fail("mmg_set_trainable: mask 0x%x has bits outside the four agents (MMG_AGENT_RECEIVER .. MMG_AGENT_BASELINE_SEN: 0x0 .. 0xf)", (unsigned)mask);
    if (!h) return fail("NULL handle");
    const int old_mask = h->train_mask, old_frozen = frozen_agents(h);
    h->train_mask = mask;
    const int frozen = frozen_agents(h);
    if (frozen == old_frozen) return 0;
    // the job table of this set of frozen agents and what follows it -- row splits, k_wgrad's walk, whether the optimizer fits inside
    // its launch --: decided once (host_select.h: reselect_from_caps, pure), kept, and uploaded on the stream of the next minibatch
    MaskPlan& mp = h->mask_plans[frozen];
    if (mp.valid) {
        h->sel = mp.sel;
        memcpy(&h->jt, mp.pinned, sizeof(JobTable));
    } else if (reselect_from_caps(h) || keep_mask_plan(h)) {
        const std::string why = g_err;
        h->train_mask = old_mask;
        reselect_from_caps(h);
        return fail("mmg_set_trainable: %s", why.c_str());
    }
    h->jt_src = mp.pinned;
    h->zero_pending |= frozen & ~old_frozen;
    return 0;
}
extern "C" int mmg_set_learning_rate(mmg_handle* h, float lr) {
    if (!(lr >= 0.f) || !(lr <= 3.4028235e38f))          // (NaN fails both compares)
        return fail("mmg_set_learning_rate: lr = %g: the learning rate must be finite and >= 0", (double)lr);
    if (!h) return fail("NULL handle");
    h->cfg.learning_rate = lr;
    return 0;
}
extern "C" int mmg_set_entropy(mmg_handle* h, float entropy_s, float entropy_sen, float entropy_rec) {
    const float v[3] = {entropy_s, entropy_sen, entropy_rec};
    for (int k = 0; k < 3; ++k)
        if (!(v[k] >= -3.4028235e38f && v[k] <= 3.4028235e38f))
            return fail("mmg_set_entropy: entropy_s = %g, entropy_sen = %g, entropy_rec = %g: the weights must be finite", (double)entropy_s, (double)entropy_sen, (double)entropy_rec);
    if (!h) return fail("NULL handle");
    // a weight that was None at mmg_create stays absent (has_entropy_* selected the kernels' terms): its argument is ignored
    if (h->cfg.has_entropy_s) h->cfg.entropy_s = h->dm.es = entropy_s;
    if (h->cfg.has_entropy_sen) h->cfg.entropy_sen = h->dm.esen = entropy_sen;
    if (h->cfg.has_entropy_rec) h->cfg.entropy_rec = h->dm.erec = entropy_rec;
    return 0;
}
extern "C" int mmg_get_training_controls(const mmg_handle* h, int* mask, float* lr, float* entropy3) {
    if (!h) return fail("NULL handle");
    if (mask) *mask = h->train_mask;
    if (lr) *lr = h->cfg.learning_rate;
    if (entropy3) { entropy3[0] = h->cfg.entropy_s; entropy3[1] = h->cfg.entropy_sen; entropy3[2] = h->cfg.entropy_rec; }
    return 0;
}

extern "C" int mmg_loss_stats(mmg_handle* h, void* stream) {
    if (!h) return fail("NULL handle");
    hipStream_t st = (hipStream_t)stream;
    if (h->fwd.bas_pending) {
        Scope sc(h, st, "k_bas_stats");
        const LaunchPlan& p = h->sel.plan;
        hipLaunchKernelGGL(k_bas_stats, dim3(p.n_stats + p.n_bas), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, p.n_stats);
        h->fwd.bas_pending = false;
        return launch_check("k_bas_stats");
    }
    Scope sc(h, st, "k_stats");
    hipLaunchKernelGGL(k_stats, dim3(5 * h->dm.T + 2), dim3(64), 0, st, h->dm, h->P, h->tp, h->fwd.scores_in_parts ? 1 : 0);
    return launch_check("k_stats");
}

// FAM_TILE: the dh-independent part of the receiver's BPTT (seeds, dgpre, dhin) for all (step, sample) rows -- with the sender's
// backward in the same launch where the plan merged them --, the recurrence, then what is left of the sender's backward
static int launch_bwd_tile(mmg_handle* h, hipStream_t st, const int64_t* d_target) {
    const Dims& d = h->dm; const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    const int zd = p.zero_dead ? 1 : 0, map = p.row_map ? 1 : 0;
    {
        Scope sc(h, st, "k_bwd_tile");
        if (p.pre_send_fn) hipLaunchKernelGGL(p.pre_send_fn, dim3(p.n_pre + p.n_rowblk * p.n_hbands), dim3(MMG_BLOCK), p.pre_smem, st, h->dm, h->P, h->tp, zd, p.n_pre, p.n_hbands, p.pre_bands);
        else if (p.pre_fn) hipLaunchKernelGGL(p.pre_fn, dim3(p.n_pre), dim3(MMG_BLOCK), p.pre_smem, st, h->dm, h->P, h->tp, zd);
        switch (p.bwd_rec) {
        case BR_SAMPLE:                                  // one workgroup per sample (+ one for the live-row list) (+ k_dhx's blocks)
            hipLaunchKernelGGL(bwd_sample_fn(d.D), dim3(d.B + 1 + (p.dhx_own ? 0 : p.dhx_grid)), dim3(256), 0, st, h->dm, h->P, h->tp, d_target, zd, map, p.dhx_blk);
            break;
        case BR_TILE:
            hipLaunchKernelGGL(p.bwd_tile_fn, dim3(p.tiles), dim3(512), s.tile_bwd_smem, st, h->dm, h->P, h->tp, d_target, zd, map);
            break;
        case BR_RC:                                      // the output-step prelude and the reverse-time loop as roles over 16-unit slices
            if (!d.use_binary) hipMemsetAsync(h->tp.rcflags, 0, 64 * 64 * sizeof(uint32_t), st);   // (binary mode: zeroed by k_bwd_pre)
            hipLaunchKernelGGL(k_rc_bwd, dim3(p.tiles * p.rc_nj), dim3(256), 0, st, h->dm, h->P, h->tp, d_target, zd, p.pre_bands, p.row_map ? 3 : 1);
        }
        if (launch_check("k_bwd_tile")) return -1;
    }
    if (d.use_binary && !is_frozen(h, MMG_AGENT_SENDER)) {                  // (the sender's reverse pass feeds the sender's jobs alone)
        Scope sc(h, st, "k_send_bwd");
        if (p.send_own)
            hipLaunchKernelGGL(k_send_bwd, dim3(p.n_rowblk, p.n_hbands), dim3(MMG_BLOCK), s.send_bwd_smem, st, h->dm, h->P, h->tp, (const int*)(p.row_map ? h->tp.rmap : nullptr), (const int*)(p.row_map ? h->tp.rcount : nullptr));
        if (p.dhx_own) hipLaunchKernelGGL(k_dhx, dim3(p.dhx_grid), dim3(MMG_BLOCK), 0, st, h->dm, h->tp, p.dhx_blk);
        if (launch_check("k_send_bwd")) return -1;
    }
    return 0;
}

// FAM_MC, continuous messages: the two launches of kernels_mc.h (with_stats: one extra workgroup of k_bwd_mc2)
static int launch_bwd_mc(mmg_handle* h, hipStream_t st, const int64_t* d_target, bool with_stats) {
    const Dims& d = h->dm; const LaunchPlan& p = h->sel.plan;
    Scope sc(h, st, "k_bwd_mc");
    hipLaunchKernelGGL((k_bwd_mc1<64, 64>), dim3(16 * p.mc_ngroup), dim3(512), 0, st, h->dm, h->P, h->tp, d_target, h->sel.mc_per, p.mc_ntile, p.mc_ngroup);
    hipLaunchKernelGGL((k_bwd_mc2<64, 100>), dim3(d.B + p.mc_nred + (with_stats ? 1 : 0)), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, p.mc_ngroup, p.mc_nred, with_stats ? 1 : 0);
    return launch_check("k_bwd_mc");
}

// FAM_FAST (sample roles + statistics / class / dbar / deferred baseline roles) and the per-sample k_bwd_conv of every other shape
static int launch_bwd_sample(mmg_handle* h, hipStream_t st, const int64_t* d_target, bool with_stats) {
    const Dims& d = h->dm; const Selection& s = h->sel; const LaunchPlan& p = s.plan;
    if (s.attn) {
        // the reverse pass, then the two reductions that are no GEMM over (step, sample) rows: dE | Py2 per class, dDD per word
        { Scope sc(h, st, "k_bwd_conv"); hipLaunchKernelGGL(k_bwd_conv_attn, dim3(d.B), dim3(MMG_BLOCK), s.bwd_smem, st, h->dm, h->P, h->tp, d_target, h->at); }
        if (is_frozen(h, MMG_AGENT_RECEIVER)) return launch_check("k_bwd_conv_attn");      // (both feed the receiver's jobs alone)
        { Scope sc(h, st, "k_attn_dE"); hipLaunchKernelGGL(k_attn_dE, dim3(d.D), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, h->at); }
        { Scope sc(h, st, "k_attn_dDD"); hipLaunchKernelGGL(k_attn_dDD, dim3(h->n_words), dim3(MMG_BLOCK), 0, st, h->dm, h->tp, h->at); }
        return launch_check("k_bwd_conv_attn");
    }
    if (s.vattn) {
        // the plain reverse pass (it leaves dh_x of every step in tape.dpre), then the attention's: k_vattn_bwd per sample, k_vattn_dwx per
        // output tile of attn_W_x.weight.  Continuous messages train the receiver alone: nothing more
        { Scope sc(h, st, "k_bwd_conv"); hipLaunchKernelGGL(p.bwd_conv_fn, dim3(d.B), dim3(MMG_BLOCK), s.bwd_smem, st, h->dm, h->P, h->tp, d_target); }
        if (launch_check("k_bwd_conv")) return -1;
        if (!d.use_binary || is_frozen(h, MMG_AGENT_SENDER)) return 0;      // (the attention's reverse pass: the sender's tensors alone)
        VattnArgs va = h->va; va.ctx = h->ctx_cur;
        const size_t smem = (size_t)s.vattn_bwd_smem;           // (sized by shape_pass, its limit raised by probe_device)
        { Scope sc(h, st, "k_vattn_bwd"); hipLaunchKernelGGL(k_vattn_bwd, dim3(d.B), dim3(MMG_BLOCK), smem, st, h->dm, h->P, h->tp, h->bwd_x, va); }
        { Scope sc(h, st, "k_vattn_dwx"); hipLaunchKernelGGL(k_vattn_dwx, dim3(((va.A + 15) / 16) * ((d.F + 15) / 16)), dim3(MMG_BLOCK), 0, st, h->dm, h->bwd_x, va, h->VG.p[VA_WX_W]); }
        return launch_check("k_vattn_bwd");
    }
    Scope sc(h, st, p.bwd_name);
    if (s.family == FAM_FAST) {      // (a 512-thread variant of this kernel measured slower: 31.8 vs 28.8 us -- it is not issue-bound)
        const int n_stats = with_stats ? p.n_stats : 0, n_bas = (with_stats && h->fwd.bas_deferred) ? p.n_bas : 0, n_class = with_stats ? d.D : p.n_class;
        hipLaunchKernelGGL(with_stats ? p.bwd_fast_stats_fn : p.bwd_fast_fn, dim3(n_stats + d.B + n_class + p.n_dbar + n_bas), dim3(256), 0, st, h->dm, h->P, h->tp, d_target, n_stats, p.zero_dead ? 1 : 0, p.n_dbar, n_bas);
    } else
        hipLaunchKernelGGL(p.bwd_conv_fn, dim3(d.B), dim3(MMG_BLOCK), s.bwd_smem, st, h->dm, h->P, h->tp, d_target);
    return launch_check("k_bwd_conv");
}

// What mmg_set_trainable left for the stream of the next minibatch: the job table of the agents in training goes to the device, and the
// gradient slice of a newly frozen agent is cleared ONCE -- no job, and none of the launches below, writes it while the agent stays frozen
// (a data-parallel caller all-reduces the whole buffer).  Stream-ordered behind the minibatch before, which read the table before.
static int apply_pending(mmg_handle* h, hipStream_t st) {
    if (h->jt_src) {
        HIP_OK(hipMemcpyAsync(h->d_jt, h->jt_src, sizeof(JobTable), hipMemcpyHostToDevice, st));
        h->jt_src = nullptr;
    }
    const int zero = h->zero_pending & frozen_agents(h);
    h->zero_pending = 0;
    for (int a = 0; a < 4; ++a)
        if ((zero >> a) & 1)
            HIP_OK(hipMemsetAsync(h->grads + h->pl.agent_begin[a], 0, sizeof(float) * (size_t)(h->pl.agent_begin[a + 1] - h->pl.agent_begin[a]), st));
    return 0;
}

// with_opt: this step's k_wgrad carries the optimizer (no k_opt launch).  conv_done: the fused step -- k_game_fast ran the forward and the
// reverse pass (its first class role listed the live rows), so no k_prep committed the minibatch counter / launch epoch: the optimizer does
static int backward_impl(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc, hipStream_t st, bool with_stats,
                         bool with_opt = false, bool conv_done = false) {
    const LaunchPlan& p = h->sel.plan;
    h->bwd_x = d_x;
    if (apply_pending(h, st)) return -1;
    if (!conv_done) {
        if (h->sel.family == FAM_TILE ? launch_bwd_tile(h, st, d_target) : mc_bwd(h) ? launch_bwd_mc(h, st, d_target, with_stats)
                                                                                     : launch_bwd_sample(h, st, d_target, with_stats)) return -1;
        if (p.dc != DC_NONE && !is_frozen(h, MMG_AGENT_RECEIVER)) {         // (dC feeds the receiver's y1 jobs alone)
            Scope sc(h, st, "k_dC");
            if (p.dc == DC_PLAIN) hipLaunchKernelGGL(k_dC, dim3(h->dm.D), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp);
            else hipLaunchKernelGGL(k_dC_tile, dim3(p.dc_grid, p.dc_slices), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, p.dc_slices, 0);
            if (p.dc == DC_TILE && p.dc_slices > 1) hipLaunchKernelGGL(k_dC_tile, dim3(p.dc_grid, 1), dim3(MMG_BLOCK), 0, st, h->dm, h->P, h->tp, p.dc_slices, 1);
            if (launch_check("k_dC")) return -1;
        }
    }
    WgHead hd;
    hd.gemm_tiles = h->jt.gemm_tiles; hd.n_wblocks = h->jt.n_wblocks; hd.special_block = h->jt.special_block; hd.special_job = h->jt.special_job;
    WgOpt wo = {};
    if (with_opt) {
        wo.oa.optim_type = h->cfg.optim_type; wo.oa.trainable = opt_trainable(h); wo.oa.lr = h->cfg.learning_rate;
        wo.oa.from_wgrad = 1; wo.oa.bump_step = 1; wo.oa.bump_mb = conv_done ? 1 : 0;
        for (int a = 0; a < 5; ++a) wo.oa.agent_begin[a] = h->pl.agent_begin[a];
        wo.oa.total = h->pl.total; wo.params = h->params; wo.state = h->opt_state; wo.grads = h->grads; wo.gnll = h->tp.gnll; wo.coefll = h->tp.coefll;
        wo.counter = h->tp.counter; wo.err_host = h->d_err;
    }
    return launch_wgrad(h, st, h->d_jt, hd, d_x, d_desc, conv_done || p.row_map, h->sel.wgrad_stride, true, with_opt ? &wo : nullptr);
}

extern "C" int mmg_backward(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc, void* stream) {
    if (!h) return fail("NULL handle");
    if (!d_x || !d_target || !d_desc) return fail("x / target / desc must not be NULL");
    if (refuse_relax(h, "mmg_backward")) return -1;
    if (h->fwd.bas_pending) return fail("mmg_loss_stats must run between mmg_exchange_forward(train) and mmg_backward (it carries the baselines' forward pass)");
    // continuous messages: the statistics are this rank's sum of rewards and hit count only, nothing a gradient depends on
    // (model.py:1297-1305) -- the call forms them itself (as a workgroup of the backward launch where the path has one, else as
    // k_stats) and no mmg_loss_stats / statistics all-reduce is needed; they reach the other ranks in the gradient tail
    const bool own_stats = mc_bwd(h) && h->sel.merge_roles;
    if (!h->dm.use_binary && !own_stats && mmg_loss_stats(h, stream)) return -1;
    return backward_impl(h, d_x, d_target, d_desc, (hipStream_t)stream, own_stats);
}

// game_step (the fused step, see backward_impl): k_opt commits the minibatch counter / launch epoch
static int clip_step_impl(mmg_handle* h, hipStream_t st, bool from_wgrad, bool game_step = false) {
    // from_wgrad: use the squared-norm partials k_wgrad left behind (valid only if d_grads has not been
    // modified since mmg_backward, i.e. single GPU); otherwise recompute them from d_grads.
    float* part = h->tp.gnpart + (from_wgrad ? 0 : MMG_MAX_WBLOCKS);
    if (apply_pending(h, st)) return -1;
    if (!from_wgrad) {
        Scope sc(h, st, "k_gradnorm");
        hipLaunchKernelGGL(k_gradnorm, dim3(MMG_GN_BLOCKS), dim3(MMG_BLOCK), 0, st, (const JobTable*)h->d_jt,
                           (const float*)h->grads, part, h->tp.counter, (const float*)(h->grads + h->pl.total), h->tp.losses,
                           h->tp.totals, h->dm.use_binary ? 0 : h->dm.Bg);
        if (launch_check("k_gradnorm")) return -1;
    }
    OptArgs oa;
    oa.optim_type = h->cfg.optim_type; oa.trainable = opt_trainable(h); oa.lr = h->cfg.learning_rate;
    oa.from_wgrad = from_wgrad ? 1 : 0; oa.bump_step = from_wgrad ? 1 : 0; oa.bump_mb = game_step ? 1 : 0;
    for (int a = 0; a < 5; ++a) oa.agent_begin[a] = h->pl.agent_begin[a];
    oa.total = h->pl.total;
    int blocks = (int)((oa.total / 4 + MMG_BLOCK - 1) / MMG_BLOCK);
    if (blocks > 1024) blocks = 1024;
    {
        Scope sc(h, st, "k_opt");
        hipLaunchKernelGGL(k_opt, dim3(blocks), dim3(MMG_BLOCK), 0, st, (const JobTable*)h->d_jt, oa, h->params,
                           (const float*)h->grads, h->opt_state, (const float*)part, (const uint32_t*)h->tp.counter, (const uint32_t*)h->tp.sync, h->d_err,
                           (const float*)(from_wgrad ? nullptr : h->grads + h->pl.total), h->tp.losses);
        if (launch_check("k_opt")) return -1;
    }
    return 0;
}

extern "C" int mmg_clip_step(mmg_handle* h, void* stream) {
    if (!h) return fail("NULL handle");
    return clip_step_impl(h, (hipStream_t)stream, false);
}

static int train_step_impl(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                           const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed, void* stream, int64_t mb = 0) {
    if (h->sel.game_ok) {
        // the small Adaptive agents: conversation, baselines, statistics and the reverse pass in ONE launch (kernels_game.h), then
        // k_wgrad and k_opt -- three launches per minibatch
        hipStream_t st = (hipStream_t)stream;
        const Dims& d = h->dm; const LaunchPlan& p = h->sel.plan;
        if (!d_x || !d_desc) return fail("x / desc must not be NULL");
        if ((d_u_z || d_u_s || d_u_w) && !(d_u_z && d_u_s && d_u_w)) return fail("injected uniforms: all three streams or none");
        ConvArgs ar = conv_args(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, 1, 0);
        ar.nprep = p.nprep_hx; ar.prep_cpb = h->sel.prep_cpb; ar.nbase = p.basehx_tiles;
        GameArgs ga; ga.n_stats = p.n_stats; ga.n_bas = h->sel.game_nbas; ga.bas_ub = h->sel.game_bas_ub;
        h->fwd = ForwardState();                        // (this launch is the forward pass: no baselines left over)
        h->fwd.basehx_ready = true; h->fwd.scores_in_parts = true;
        {
            Scope sc(h, st, "k_game");
            const int grid = d.B + ar.nprep + ar.nbase + ga.n_stats + ga.n_bas + d.D;
            hipLaunchKernelGGL(game_fast_fn(d.D), dim3(grid), dim3(256), game_lds_bytes(), st, h->dm, h->P, h->tp, ar, ga);
            if (launch_check("k_game_fast")) return -1;
        }
        if (backward_impl(h, d_x, d_target, d_desc, st, true, h->sel.wgrad_opt_ok, true)) return -1;
        return h->sel.wgrad_opt_ok ? 0 : clip_step_impl(h, st, true, true);
    }
    if (exchange_forward_impl(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, 1, TAPE_MINIMAL, stream, true, mb)) return -1;
    const bool merged = merge_stats(h);
    if (h->fwd.bas_deferred && !merged) return fail("internal: deferred baselines without the merged backward launch");
    if (!merged && mmg_loss_stats(h, stream)) return -1;
    if (backward_impl(h, d_x, d_target, d_desc, (hipStream_t)stream, merged, h->sel.wgrad_opt_ok)) return -1;
    // (visual attention: one gradient tensor is no job of k_wgrad, so the norms are taken over d_grads -- the phased step's k_gradnorm + k_opt)
    return h->sel.wgrad_opt_ok ? 0 : clip_step_impl(h, (hipStream_t)stream, !h->sel.vattn);
}

extern "C" int mmg_train_step(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                              const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed, void* stream) {
    if (begin_minibatch(h, "mmg_train_step") || refuse_relax(h, "mmg_train_step")) return -1;
    if (h->cfg.global_batch != h->cfg.batch) return fail("mmg_train_step is single-GPU; with several ranks: mmg_dp_train_step, or all-reduce between the phases");
    if (!d_target) return fail("target must not be NULL");
    return run_minibatches(h, 1, stream, [&](int64_t) { return train_step_impl(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, stream); });
}

// n consecutive minibatches of the epoch loop (model.py:1218-1240) enqueued from C: minibatch i reads rows [i * B, (i + 1) * B)
// of d_x [n * B, F] / d_target [n * B] -- the batch-ordered gather of the epoch (misc.py:257-302) the caller laid out once.  The
// sampling streams advance with the device-side minibatch counter exactly as under n mmg_train_step calls.
extern "C" int mmg_train_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc,
                               uint64_t seed, void* stream) {
    if (begin_minibatch(h, "mmg_train_steps") || refuse_relax(h, "mmg_train_steps")) return -1;
    if (h->cfg.global_batch != h->cfg.batch) return fail("mmg_train_steps is single-GPU; with several ranks: mmg_dp_train_steps");
    if (!d_x || !d_target || !d_desc || n < 0) return fail("x / target / desc must not be NULL, n >= 0");
    return run_minibatches(h, n, stream, [&](int64_t i) {
        return train_step_impl(h, d_x + (size_t)i * x_stride(h), d_target + (size_t)i * h->dm.B, d_desc, nullptr, nullptr, nullptr, seed, stream, i);
    });
}

// ---------------------------------------------------------------------------------------------
// The data-parallel minibatch (SURVEY 8e option A; couplings model.py:912-915, 947-961, 1310) in ONE call: forward + batch
// statistics | all-reduce of the f64 statistics (binary messages only) | backward | ONE all-reduce of the flat gradient buffer
// incl. its tail quad | norm of the REDUCED gradient + optimizer.  The collectives are RCCL's ncclAllReduce, called through the
// address the caller hands over (the library does not link RCCL) on the caller's communicator and on THIS stream; `reduce` = 0
// skips them (one rank).  What python did in four ctypes calls + two per step (50 us of host time against 77 us of device time).
// ---------------------------------------------------------------------------------------------
typedef int (*mmg_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
extern "C" int mmg_dp_set_allreduce(mmg_handle* h, void* nccl_all_reduce, void* comm) {
    if (!h) return fail("NULL handle");
    h->ar_fn = nccl_all_reduce; h->ar_comm = comm;
    return 0;
}
static int dp_step_impl(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                        const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed, int full_tape, int reduce, void* stream) {
    if (refuse_attn(h, "the data-parallel step")) return -1;
    hipStream_t st = (hipStream_t)stream;
    mmg_allreduce_fn ar = (mmg_allreduce_fn)h->ar_fn;
    if (reduce && !ar) return fail("mmg_dp_train_step: no collective set (mmg_dp_set_allreduce)");
    if (exchange_forward_impl(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, 1, full_tape ? TAPE_LOG : TAPE_MINIMAL, stream)) return -1;
    if (h->dm.use_binary) {
        if (mmg_loss_stats(h, stream)) return -1;
        if (reduce) {
            const int rc = ar(h->tp.stats, h->tp.stats, (size_t)stat_count(h->dm.T), 8 /* ncclFloat64 */, 0 /* ncclSum */, h->ar_comm, st);
            if (rc) return fail("ncclAllReduce (statistics) failed: %d", rc);
        }
    }
    if (mmg_backward(h, d_x, d_target, d_desc, stream)) return -1;
    if (reduce) {
        const int rc = ar(h->grads, h->grads, (size_t)(h->pl.total + MMG_GRAD_TAIL), 7 /* ncclFloat32 */, 0, h->ar_comm, st);
        if (rc) return fail("ncclAllReduce (gradients) failed: %d", rc);
    }
    return clip_step_impl(h, st, false);
}
extern "C" int mmg_dp_train_step(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                                 const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed, int full_tape, int reduce, void* stream) {
    if (begin_minibatch(h, "mmg_dp_train_step") || refuse_relax(h, "mmg_dp_train_step")) return -1;
    if (!d_x || !d_target || !d_desc) return fail("x / target / desc must not be NULL");
    return run_minibatches(h, 1, stream, [&](int64_t) { return dp_step_impl(h, d_x, d_target, d_desc, d_u_z, d_u_s, d_u_w, seed, full_tape, reduce, stream); });
}
extern "C" int mmg_dp_train_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc,
                                  uint64_t seed, int reduce, void* stream) {
    if (begin_minibatch(h, "mmg_dp_train_steps") || refuse_relax(h, "mmg_dp_train_steps")) return -1;
    if (!d_x || !d_target || !d_desc || n < 0) return fail("x / target / desc must not be NULL, n >= 0");
    return run_minibatches(h, n, stream, [&](int64_t i) {
        return dp_step_impl(h, d_x + (size_t)i * h->dm.B * h->dm.F, d_target + (size_t)i * h->dm.B, d_desc, nullptr, nullptr, nullptr, seed, 0, reduce, stream);
    });
}

// ---------------------------------------------------------------------------------------------
// Host helper of the epoch loop (misc.py:270-271 `random.seed(11 + epoch); random.shuffle(order)`): Fisher-Yates exactly as
// CPython's random.shuffle draws it -- j = _randbelow(i + 1) for i = n-1 .. 1 with _randbelow(m) = rejection sampling of
// getrandbits(bit_length(m)) = genrand_uint32() >> (32 - k) -- continuing the Mersenne-Twister state the caller read with
// random.getstate().  The Python loop costs ~0.4 us per sample (1.2 ms per 3000-sample epoch, a third of the epoch's device
// time at config 2); this is ~10 ns per sample.  The caller verifies it against random.shuffle once per process.
// ---------------------------------------------------------------------------------------------
extern "C" int mmg_host_shuffle(const uint32_t* mt_state, int pos, int64_t n, int64_t* perm) {
    if (!mt_state || !perm || n < 0 || pos < 0 || pos > 624) return fail("mmg_host_shuffle: bad arguments");
    if (n > 0x7fffffffLL) return fail("mmg_host_shuffle: more than 2^31 - 1 elements");
    uint32_t mt[624];
    memcpy(mt, mt_state, sizeof(mt));
    int mti = pos;
    auto next = [&]() -> uint32_t {
        if (mti >= 624) {
            const uint32_t UP = 0x80000000u, LO = 0x7fffffffu, MA = 0x9908b0dfu;
            int kk = 0;
            for (; kk < 624 - 397; ++kk) { const uint32_t y = (mt[kk] & UP) | (mt[kk + 1] & LO); mt[kk] = mt[kk + 397] ^ (y >> 1) ^ ((y & 1u) ? MA : 0u); }
            for (; kk < 623; ++kk) { const uint32_t y = (mt[kk] & UP) | (mt[kk + 1] & LO); mt[kk] = mt[kk + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? MA : 0u); }
            const uint32_t y = (mt[623] & UP) | (mt[0] & LO);
            mt[623] = mt[396] ^ (y >> 1) ^ ((y & 1u) ? MA : 0u);
            mti = 0;
        }
        uint32_t y = mt[mti++];
        y ^= (y >> 11); y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= (y >> 18);
        return y;
    };
    for (int64_t i = n - 1; i >= 1; --i) {
        const uint32_t m = (uint32_t)(i + 1);
        const int k = 32 - __builtin_clz(m);                           // bit_length(i + 1)
        uint32_t r = next() >> (32 - k);
        while (r >= m) r = next() >> (32 - k);
        const int64_t t = perm[i]; perm[i] = perm[r]; perm[r] = t;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// agent-level entry points (one exchange step, forward only)
// ---------------------------------------------------------------------------------------------
extern "C" int mmg_sender_forward(mmg_handle* h, const float* d_x, const float* d_w, int t, int train,
                                  const float* d_u_z, uint64_t seed, float* d_message, float* d_probs, float* d_h_x,
                                  void* stream) {
    if (!h) return fail("NULL handle");
    if (!d_x || !d_message) return fail("x / message must not be NULL");
    if (t < 0 || t >= h->dm.T) return fail("t out of range");
    if (t > 0 && !d_w) return fail("w must not be NULL for t > 0");
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->dm;
    // k_prep needs a description matrix only for Cd (unused here); reuse the tape's zero-initialised Cd as a
    // dummy source so that hw0 / dsig are refreshed from the current parameters.
    {
        Scope sc(h, st, "k_prep(sender)");
        Dims d1 = h->dm; d1.D = 0;
        hipLaunchKernelGGL(k_prep, dim3((d1.H + 63) / 64), dim3(MMG_BLOCK), h->sel.prep_smem, st, d1, h->P, h->tp, (const float*)nullptr,
                           (const float*)nullptr, 1, train ? 1 : 0);
        if (launch_check("k_prep")) return -1;
    }
    // visual attention: HX / HG are formed by the first call after mmg_vattn_reset_state (or after any whole conversation on the handle)
    // and kept for the later calls, as the reference caches them from reset_state() on (model.py:107-108, 123-133); the step's h_x
    // comes out of the conversation kernel
    if (h->sel.vattn) {
        if (vattn_ready(h, "mmg_sender_forward")) return -1;
        if (h->vattn_stale && launch_vattn_prep(h, st, d_x, h->vd.G > 0 ? h->d_ctx : nullptr)) return -1;
        h->vattn_stale = false;
    } else if (launch_gemm_nt(h, st, "k_gemm_nt(h_x)", d_x, d.F, h->P.p[S_IMG_W], d.F, h->P.p[S_IMG_B], h->tp.hx, d.H, d.B, d.H, d.F)) return -1;
    ConvArgs ar;
    memset(&ar, 0, sizeof(ar));
    ar.x = d_x; ar.u_z = d_u_z ? d_u_z - (size_t)t * d.B * d.W : nullptr; ar.seed = seed; ar.train = train; ar.run_all = 1;
    ar.t_begin = t; ar.t_end = t + 1; ar.phases = 1; ar.w_in = d_w;
    flip_args(h, ar, seed, train, false);
    noise_args(h, ar, seed, train, false);
    ar.sender_var = h->sel.variant;
    relax_args(h, ar);
    if (ar.flip_on & 4 && t == 0) ar.flip_c1 = h->sel.noise ? h->noise_evals++ : h->flip_evals++;      // (an evaluation conversation begins at the sender's step 0)
    if (h->sel.vattn) hipLaunchKernelGGL(h->sel.plan.agent_vattn_fn, dim3(d.B), dim3(MMG_BLOCK), h->sel.conv_smem_agent, st, h->dm, h->P, h->tp, ar, h->va);
    else hipLaunchKernelGGL(h->sel.plan.agent_fn, dim3(d.B), dim3(MMG_BLOCK), h->sel.conv_smem_agent, st, h->dm, h->P, h->tp, ar);
    if (launch_check("k_conversation(sender)")) return -1;
    const size_t off = (size_t)t * d.B * d.W;
    HIP_OK(hipMemcpyAsync(d_message, h->tp.z + off, sizeof(float) * d.B * d.W, hipMemcpyDeviceToDevice, st));
    if (d_probs && d.use_binary) HIP_OK(hipMemcpyAsync(d_probs, h->tp.pz + off, sizeof(float) * d.B * d.W, hipMemcpyDeviceToDevice, st));
    if (d_h_x) HIP_OK(hipMemcpyAsync(d_h_x, h->sel.vattn ? h->va.tp.vattn_hx + (size_t)t * d.B * d.H : h->tp.hx, sizeof(float) * d.B * d.H, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int mmg_receiver_forward(mmg_handle* h, const float* d_z, const float* d_desc, float* d_h_z,
                                    float* d_s_prob_prod, int first, int t, int train,
                                    const float* d_u_s, const float* d_u_w, uint64_t seed,
                                    float* d_s, float* d_s_prob, float* d_w, float* d_w_probs, float* d_y,
                                    float* d_h_w, void* stream) {
    if (!h) return fail("NULL handle");
    if (!d_z || !d_desc || !d_h_z) return fail("z / desc / h_z must not be NULL");
    if (attn_ready(h, "mmg_receiver_forward")) return -1;
    if (t < 0 || t >= h->dm.T) return fail("t out of range");
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->dm;
    const size_t offW = (size_t)t * d.B * d.W, offB = (size_t)t * d.B;
    HIP_OK(hipMemcpyAsync(h->tp.z + offW, d_z, sizeof(float) * d.B * d.W, hipMemcpyDeviceToDevice, st));
    if (launch_prep(h, st, d_desc, nullptr, train ? 1 : 0)) return -1;
    if (h->sel.attn && launch_attn_prep(h, st)) return -1;
    ConvArgs ar;
    memset(&ar, 0, sizeof(ar));
    ar.desc = d_desc; ar.seed = seed; ar.train = train; ar.run_all = 1;
    ar.u_s = d_u_s ? d_u_s - offB : nullptr; ar.u_w = d_u_w ? d_u_w - offW : nullptr;
    ar.t_begin = t; ar.t_end = t + 1; ar.phases = 2; ar.h_state = d_h_z; ar.sprod_state = d_s_prob_prod; ar.sprod_first = first;
    flip_args(h, ar, seed, train, false);
    noise_args(h, ar, seed, train, false);
    ar.sender_var = h->sel.variant;
    relax_args(h, ar);
    if (h->sel.attn) hipLaunchKernelGGL(h->sel.plan.agent_attn_fn, dim3(d.B), dim3(MMG_BLOCK), h->sel.conv_smem_agent, st, h->dm, h->P, h->tp, ar, h->at);
    else hipLaunchKernelGGL(h->sel.plan.agent_fn, dim3(d.B), dim3(MMG_BLOCK), h->sel.conv_smem_agent, st, h->dm, h->P, h->tp, ar);
    if (launch_check("k_conversation(receiver)")) return -1;
    if (d_s) HIP_OK(hipMemcpyAsync(d_s, h->tp.s + offB, sizeof(float) * d.B, hipMemcpyDeviceToDevice, st));
    if (d_s_prob) HIP_OK(hipMemcpyAsync(d_s_prob, h->tp.ps + offB, sizeof(float) * d.B, hipMemcpyDeviceToDevice, st));
    if (d_w) HIP_OK(hipMemcpyAsync(d_w, h->tp.w + offW, sizeof(float) * d.B * d.W, hipMemcpyDeviceToDevice, st));
    if (d_w_probs && d.use_binary) HIP_OK(hipMemcpyAsync(d_w_probs, h->tp.pw + offW, sizeof(float) * d.B * d.W, hipMemcpyDeviceToDevice, st));
    if (d_y) HIP_OK(hipMemcpyAsync(d_y, h->tp.y + (size_t)t * d.B * d.D, sizeof(float) * d.B * d.D, hipMemcpyDeviceToDevice, st));
    if (d_h_w) HIP_OK(hipMemcpyAsync(d_h_w, h->tp.g + (size_t)t * d.B * d.R, sizeof(float) * d.B * d.R, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int mmg_baseline_forward(mmg_handle* h, int which, const float* d_x, const float* d_binary,
                                    const float* d_inp, int rows, float* d_score, void* stream) {
    if (!h) return fail("NULL handle");
    if (!d_binary || !d_score || rows <= 0) return fail("binary / score must not be NULL, rows > 0");
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->dm; const Params& P = h->P;
    BasArgs rec, sen;
    memset(&rec, 0, sizeof(rec)); memset(&sen, 0, sizeof(sen));
    if (which == MMG_AGENT_BASELINE_REC) {
        if (!d_inp) return fail("baseline_rec needs inp (receiver hidden state)");
        rec.rows = rows; rec.x1 = d_binary; rec.ld1 = d.W; rec.k1 = d.W; rec.x2 = d_inp; rec.ld2 = d.R; rec.k2 = d.R;
        rec.W1 = P.p[BR_L1_W]; rec.ldw = d.W + d.R; rec.b1 = P.p[BR_L1_B]; rec.W2 = P.p[BR_L2_W]; rec.b2 = P.p[BR_L2_B];
        rec.score = d_score;
    } else if (which == MMG_AGENT_BASELINE_SEN) {
        if (!d_x) return fail("baseline_sen needs x (sender.h_x)");
        sen.rows = rows; sen.x1 = d_x; sen.ld1 = d.H; sen.k1 = d.H; sen.x2 = d_binary; sen.ld2 = d.W; sen.k2 = d.W;
        sen.W1 = P.p[BS_L1_W]; sen.ldw = d.H + d.W; sen.b1 = P.p[BS_L1_B]; sen.W2 = P.p[BS_L2_W]; sen.b2 = P.p[BS_L2_B];
        sen.score = d_score;
    } else {
        return fail("which must be MMG_AGENT_BASELINE_REC or MMG_AGENT_BASELINE_SEN");
    }
    hipLaunchKernelGGL(k_baselines, dim3((rows + 15) / 16, 2), dim3(MMG_BLOCK), 0, st, d.K, rec, sen);
    return launch_check("k_baselines(agent)");
}

// ---------------------------------------------------------------------------------------------
// mmg_exchange_vjp: the backward pass of ONE agent's autograd graph of the last training exchange (kernels_vjp.h).  Reads the
// run-all tape of mmg_exchange_forward(train = 1, run_all_steps = 1); writes only that agent's slice of the gradient buffer.
// ---------------------------------------------------------------------------------------------
extern "C" int mmg_exchange_vjp(mmg_handle* h, int agent, int n_steps, const float* d_x, const float* d_desc, const float* d_dy,
                                const float* d_dz, const float* d_dw, const float* d_dps, const float* d_dbs, const float* d_dbr,
                                void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_exchange_vjp") || refuse_relax(h, "mmg_exchange_vjp")) return -1;
    const Dims& d = h->dm;
    if (agent < 0 || agent > 3) return fail("unknown agent %d", agent);
    if (n_steps < 1 || n_steps > d.T) return fail("n_steps must be in [1, %d] (got %d)", d.T, n_steps);
    if (agent >= MMG_AGENT_BASELINE_REC && !d.use_binary) return fail("baseline scores exist in binary training only (model.py:834-843)");
    hipStream_t st = (hipStream_t)stream;
    VjpIn in;
    in.dy = d_dy; in.dz = d_dz; in.dw = d_dw; in.dps = d_dps; in.dbs = d_dbs; in.dbr = d_dbr; in.n = n_steps; in.sv = h->sel.variant;
    in.tau_z = in.tau_w = 0.f;
    if (agent == MMG_AGENT_RECEIVER) {
        if (!d_desc) return fail("desc must not be NULL");
        const size_t smem = sizeof(float) * (size_t)vjp_rec_smem_floats(d);
        if (vjp_lds_ok(smem, "receiver", " (too many classes)") || launch_vjp_cd(h, st, d_desc)) return -1;
        {
            Scope sc(h, st, "k_vjp_rec");
            hipLaunchKernelGGL(k_vjp_rec, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, in);
            if (launch_check("k_vjp_rec")) return -1;
        }
        if (launch_vjp_class(h, st, in)) return -1;
    } else if (agent == MMG_AGENT_SENDER) {
        if (!d_x) return fail("x must not be NULL");
        const size_t smem = sizeof(float) * (size_t)vjp_sen_smem_floats(d);
        if (vjp_lds_ok(smem, "sender", " (h_dim too large)")) return -1;
        Scope sc(h, st, "k_vjp_sen");
        hipLaunchKernelGGL(k_vjp_sen, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, in);
        if (launch_check("k_vjp_sen")) return -1;
    } else {
        const size_t smem = sizeof(float) * (size_t)(agent == MMG_AGENT_BASELINE_REC ? d.W + d.R : d.H + d.W);
        if (vjp_lds_ok(smem, "baseline", "")) return -1;
        Scope sc(h, st, "k_vjp_bas");
        hipLaunchKernelGGL(k_vjp_bas, dim3(d.T * d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, in, agent);
        if (launch_check("k_vjp_bas")) return -1;
    }
    return launch_vjp_wgrad(h, st, agent, d_x, d_desc);
}

// mmg_exchange_vjp_channel: the sender's and the receiver's graphs of the last training exchange as ONE graph, the messages not
// detached (kernels_vjp.h: k_vjp_channel).  Same tape, same job tables; writes exactly the two agents' slices.
extern "C" int mmg_exchange_vjp_channel(mmg_handle* h, int n_steps, const float* d_x, const float* d_desc, const float* d_dy,
                                        const float* d_dz, const float* d_dw, const float* d_dps, void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_exchange_vjp_channel")) return -1;
    const Dims& d = h->dm;
    if (n_steps < 1 || n_steps > d.T) return fail("n_steps must be in [1, %d] (got %d)", d.T, n_steps);
    if (!d_x || !d_desc) return fail("x / desc must not be NULL");
    if (h->sel.variant) return fail("mmg_exchange_vjp_channel: not available on a handle with a sender variant (mmg_set_sender_variant)");
    hipStream_t st = (hipStream_t)stream;
    VjpIn in;
    in.dy = d_dy; in.dz = d_dz; in.dw = d_dw; in.dps = d_dps; in.dbs = nullptr; in.dbr = nullptr; in.n = n_steps; in.sv = 0;
    in.tau_z = h->relax_tau_sen; in.tau_w = h->relax_tau_rec;
    const size_t smem = sizeof(float) * (size_t)vjp_channel_smem_floats(d);
    if (vjp_lds_ok(smem, "channel", " (too many classes or h_dim too large)") || launch_vjp_cd(h, st, d_desc)) return -1;
    {
        Scope sc(h, st, "k_vjp_channel");
        hipLaunchKernelGGL(h->sel.relax ? k_vjp_channel_relax : k_vjp_channel, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, in);
        if (launch_check("k_vjp_channel")) return -1;
    }
    if (launch_vjp_class(h, st, in)) return -1;
    if (launch_vjp_wgrad(h, st, MMG_AGENT_RECEIVER, d_x, d_desc)) return -1;
    return launch_vjp_wgrad(h, st, MMG_AGENT_SENDER, d_x, d_desc);
}

// Can a per-call product run on the MFMA tiles of k_vjp_nn?  tgemm_nn_raw reads Bm rows as float4 (16-byte aligned rows, N a
// multiple of 4) and k_vjp_nn stages a [16, K] A tile plus the raw accumulators in LDS.
static bool vjp_nn_fits(const NnProd& p) {
    return p.N >= 4 && p.N % 4 == 0 && p.ldb % 4 == 0 && ((uintptr_t)p.Bm & 15) == 0 &&
           sizeof(float) * (size_t)vjp_nn_smem_floats(p.N, p.K) <= 65536;
}

// Up to two products in one launch (B / 16 tiles each).  np == 0: nothing.
static int launch_vjp_nn(mmg_handle* h, hipStream_t st, int np, const NnProd& p0, const NnProd& p1) {
    if (np == 0) return 0;
    const NnProd& q = np > 1 ? p1 : p0;
    const int f0 = vjp_nn_smem_floats(p0.N, p0.K), f1 = vjp_nn_smem_floats(q.N, q.K);
    const size_t smem = sizeof(float) * (size_t)(f0 > f1 ? f0 : f1);
    Scope sc(h, st, "k_vjp_nn");
    hipLaunchKernelGGL(k_vjp_nn, dim3(sample_tiles(h->dm.B), np), dim3(MMG_BLOCK), smem, st, h->dm.B, p0, q);
    return launch_check("k_vjp_nn");
}

static NnProd nn_prod(const float* A, int lda, const float* Bm, int ldb, float* C, int ldc, int N, int K) {
    NnProd p;
    p.A = A; p.Bm = Bm; p.C = C; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.N = N; p.K = K;
    return p;
}

// One NN product over `rows` rows: the MFMA tiles of k_vjp_nn where the shape fits them, else one thread per output element.
static int launch_vjp_nn_rows(mmg_handle* h, hipStream_t st, int rows, const NnProd& p) {
    if (vjp_nn_fits(p)) {
        Scope sc(h, st, "k_vjp_nn");
        hipLaunchKernelGGL(k_vjp_nn, dim3(sample_tiles(rows), 1), dim3(MMG_BLOCK), sizeof(float) * (size_t)vjp_nn_smem_floats(p.N, p.K),
                           st, rows, p, p);
        return launch_check("k_vjp_nn");
    }
    const size_t blocks = ((size_t)rows * p.N + MMG_BLOCK - 1) / MMG_BLOCK;
    Scope sc(h, st, "k_vjp_nn_plain");
    hipLaunchKernelGGL(k_vjp_nn_plain, dim3((int)(blocks > 65536 ? 65536 : blocks)), dim3(MMG_BLOCK), 0, st, rows, p);
    return launch_check("k_vjp_nn_plain");
}

// mmg_vjp_input_grads: d data and d desc from the deltas the VJP call just before it left in the v* arrays (kernels_vjp.h:
// k_vjp_ddesc).  Reads the tape and the parameters; writes vdq and the caller's two outputs, nothing else.
extern "C" int mmg_vjp_input_grads(mmg_handle* h, int per_call, int n_steps, const float* d_y, float* d_ddx, float* d_ddesc,
                                   void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_vjp_input_grads")) return -1;
    const Dims& d = h->dm;
    if (n_steps < 1 || n_steps > d.T) return fail("n_steps must be in [1, %d] (got %d)", d.T, n_steps);
    if (per_call && d_ddesc && !d_y) return fail("y of the call must not be NULL (per_call)");
    hipStream_t st = (hipStream_t)stream;
    if (d_ddx) {                                               // d data = dhx . W_image
        const NnProd px = nn_prod(h->tp.vdhx, d.H, h->P.p[S_IMG_W], d.F, d_ddx, d.F, d.F, d.H);
        if (launch_vjp_nn_rows(h, st, d.B, px)) return -1;
    }
    if (d_ddesc) {
        const int rows = per_call ? d.B : n_steps * d.B;       // the executed (step, sample) rows | the call's rows
        const NnProd pq = nn_prod(h->tp.vdgpre, d.R, h->P.p[R_WD_W], d.V, h->tp.vdq, d.V, d.V, d.R);   // q = dgpre . W_d
        if (launch_vjp_nn_rows(h, st, rows, pq)) return -1;
        Scope sc(h, st, "k_vjp_ddesc");
        hipLaunchKernelGGL(k_vjp_ddesc, dim3((d.D + 15) / 16, (d.V + MMG_DDESC_VT - 1) / MMG_DDESC_VT), dim3(MMG_BLOCK), 0, st, d, h->P,
                           h->tp, per_call ? d_y : (const float*)h->tp.y, rows, d_ddesc);
        if (launch_check("k_vjp_ddesc")) return -1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The per-call VJPs of the agent modules' forward() (kernels_vjp.h: k_vjp_sen_call / k_vjp_rec_call / k_vjp_bas_call): the
// backward pass of ONE mmg_sender_forward / mmg_receiver_forward / mmg_baseline_forward call from the caller's copies of its
// inputs and outputs -- never the tape of a forward.  Each writes only its agent's slice of the gradient buffer.
// ---------------------------------------------------------------------------------------------
extern "C" int mmg_sender_vjp(mmg_handle* h, const float* d_x, const float* d_w, int t, const float* d_h_x, const float* d_probs,
                              const float* d_dout, const float* d_dh_x, float* d_dx, float* d_dw, void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_sender_vjp") || refuse_relax(h, "mmg_sender_vjp")) return -1;
    const Dims& d = h->dm;
    if (!d_x || !d_h_x) return fail("x / h_x must not be NULL");
    if (t < 0 || t >= d.T) return fail("t out of range");
    if (t > 0 && !d_w) return fail("w must not be NULL for t > 0");
    if (d.use_binary && d_dout && !d_probs) return fail("probs must not be NULL when d probs is given (binary messages)");
    const size_t smem = sizeof(float) * (size_t)vjp_sen_smem_floats(d);
    if (vjp_lds_ok(smem, "sender", " (h_dim too large)")) return -1;
    hipStream_t st = (hipStream_t)stream;
    SenCall c;
    c.w = d_w; c.h_x = d_h_x; c.probs = d.use_binary ? d_probs : nullptr; c.dout = d_dout; c.dh_x = d_dh_x;
    c.dx = d_dx; c.dw = d_dw; c.t = t; c.sv = h->sel.variant;
    // W_c^T dpre (-> vdc0 at t = 0, d w after) and d x = W_img^T d h_x on the MFMA tiles where the shape allows
    NnProd pr[2];
    int np = 0;
    float* q_out = t == 0 ? h->tp.vdc0 : d_dw;
    const NnProd pq = nn_prod(h->tp.vdpre, d.H, h->P.p[S_CODE_W], d.W, q_out, d.W, d.W, d.H);
    const NnProd px = nn_prod(h->tp.vdhx, d.H, h->P.p[S_IMG_W], d.F, d_dx, d.F, d.F, d.H);
    c.q_tiles = vjp_nn_fits(pq) ? 1 : 0;
    c.dx_tiles = vjp_nn_fits(px) ? 1 : 0;
    if (c.q_tiles && q_out) pr[np++] = pq;
    if (c.dx_tiles && d_dx) pr[np++] = px;
    {
        Scope sc(h, st, "k_vjp_sen_call");
        hipLaunchKernelGGL(k_vjp_sen_call, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, d_x, c);
        if (launch_check("k_vjp_sen_call")) return -1;
    }
    if (launch_vjp_nn(h, st, np, pr[0], pr[1])) return -1;
    return launch_vjp_wgrad(h, st, 4 + MMG_AGENT_SENDER, d_x, nullptr);
}

extern "C" int mmg_receiver_vjp(mmg_handle* h, const float* d_z, const float* d_desc, const float* d_h_prev, const float* d_h_new,
                                const float* d_y, const float* d_w_probs, const float* d_s_prob, const float* d_dy,
                                const float* d_dw, const float* d_dps, const float* d_dh_w, const float* d_dh_new,
                                float* d_dz, float* d_dh_prev, void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_receiver_vjp") || refuse_relax(h, "mmg_receiver_vjp")) return -1;
    const Dims& d = h->dm;
    if (!d_z || !d_desc || !d_h_new || !d_y) return fail("z / desc / h_new / y must not be NULL");
    if (d.use_binary && d_dw && !d_w_probs) return fail("w_probs must not be NULL when d w_probs is given (binary messages)");
    if (d_dps && !d_s_prob) return fail("s_prob must not be NULL when d s_prob is given");
    const size_t smem = sizeof(float) * (size_t)vjp_rec_smem_floats(d);
    if (vjp_lds_ok(smem, "receiver", " (too many classes)")) return -1;
    hipStream_t st = (hipStream_t)stream;
    RecCall c;
    c.z = d_z; c.h_prev = d_h_prev; c.h_new = d_h_new; c.y = d_y; c.w_probs = d.use_binary ? d_w_probs : nullptr; c.s_prob = d_s_prob;
    c.dy = d_dy; c.dw = d_dw; c.dps = d_dps; c.dh_w = d_dh_w; c.dh_new = d_dh_new; c.dz = d_dz; c.dh_prev = d_dh_prev;
    const NnProd pz = nn_prod(h->tp.vdgi, 3 * d.R, h->P.p[R_WIH], d.W, d_dz, d.W, d.W, 3 * d.R);      // d z = dgi . W_ih
    c.dz_tiles = vjp_nn_fits(pz) ? 1 : 0;
    VjpIn in;
    memset(&in, 0, sizeof(in));
    in.dy = d_dy; in.n = 1;                                    // k_vjp_class over the call's B rows
    if (launch_vjp_cd(h, st, d_desc)) return -1;
    {
        Scope sc(h, st, "k_vjp_rec_call");
        hipLaunchKernelGGL(k_vjp_rec_call, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, c);
        if (launch_check("k_vjp_rec_call")) return -1;
    }
    if (launch_vjp_nn(h, st, (c.dz_tiles && d_dz) ? 1 : 0, pz, pz)) return -1;
    if (launch_vjp_class(h, st, in)) return -1;
    return launch_vjp_wgrad(h, st, 4 + MMG_AGENT_RECEIVER, nullptr, d_desc);
}

extern "C" int mmg_baseline_vjp(mmg_handle* h, int which, const float* d_x, const float* d_binary, const float* d_inp, int rows,
                                const float* d_dscore, float* d_dx, float* d_dbinary, float* d_dinp, void* stream) {
    if (!h) return fail("NULL handle");
    if (refuse_attn(h, "mmg_baseline_vjp") || refuse_relax(h, "mmg_baseline_vjp")) return -1;
    const Dims& d = h->dm;
    if (which != MMG_AGENT_BASELINE_REC && which != MMG_AGENT_BASELINE_SEN)
        return fail("which must be MMG_AGENT_BASELINE_REC or MMG_AGENT_BASELINE_SEN");
    if (rows != d.B) return fail("rows must equal the handle's batch (%d, got %d)", d.B, rows);
    if (!d_binary) return fail("binary must not be NULL");
    if (which == MMG_AGENT_BASELINE_REC && !d_inp) return fail("baseline_rec needs inp (receiver hidden state)");
    if (which == MMG_AGENT_BASELINE_SEN && !d_x) return fail("baseline_sen needs x (sender.h_x)");
    const size_t smem = sizeof(float) * (size_t)vjp_bas_call_smem_floats(d, which);
    if (vjp_lds_ok(smem, "baseline", "")) return -1;
    hipStream_t st = (hipStream_t)stream;
    BasCall c;
    c.x = d_x; c.binary = d_binary; c.inp = d_inp; c.dscore = d_dscore; c.dx = d_dx; c.dbinary = d_dbinary; c.dinp = d_dinp;
    // the input gradients d hidden . W1[:, columns of the input] on the MFMA tiles where both column ranges allow
    const bool rec = which == MMG_AGENT_BASELINE_REC;
    const int n1 = rec ? d.W : d.H, nin = rec ? d.W + d.R : d.H + d.W;
    const float* W1 = h->P.p[rec ? BR_L1_W : BS_L1_W];
    float* out1 = rec ? d_dbinary : d_dx;
    float* out2 = rec ? d_dinp : d_dbinary;
    const NnProd p1 = nn_prod(h->tp.vcdh, d.K, W1, nin, out1, n1, n1, d.K);
    const NnProd p2 = nn_prod(h->tp.vcdh, d.K, W1 + n1, nin, out2, nin - n1, nin - n1, d.K);
    NnProd pr[2];
    int np = 0;
    c.tiles = (out1 || out2) && vjp_nn_fits(p1) && vjp_nn_fits(p2) ? 1 : 0;
    if (c.tiles && out1) pr[np++] = p1;
    if (c.tiles && out2) pr[np++] = p2;
    {
        Scope sc(h, st, "k_vjp_bas_call");
        hipLaunchKernelGGL(k_vjp_bas_call, dim3(d.B), dim3(MMG_BLOCK), smem, st, d, h->P, h->tp, c, which);
        if (launch_check("k_vjp_bas_call")) return -1;
    }
    if (launch_vjp_nn(h, st, np, pr[0], pr[1])) return -1;
    return launch_vjp_wgrad(h, st, 4 + which, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// The loss functions (kernels_loss.h): handle-free -- the arithmetic depends on no mmg_config -- on the calling thread's current
// device.  Forward: the partial-sum launch over (slots, steps) and the one-workgroup finishing launch; VJP: one launch.
// ---------------------------------------------------------------------------------------------
static int loss_shape_ok(const char* who, int n, int B, int inner) {
    if (n < 1 || B < 1 || inner < 1) return fail("%s: n_steps, batch and the row width must be positive (got %d, %d, %d)", who, n, B, inner);
    if (n > MMG_LOSS_MAX_STEPS) return fail("%s: n_steps must be <= %d (got %d)", who, MMG_LOSS_MAX_STEPS, n);
    return 0;
}
static int loss_flat_grid(size_t items) {
    const size_t g = (items + MMG_BLOCK - 1) / MMG_BLOCK;
    return (int)(g > 65536 ? 65536 : g);                 // the kernels walk the rest with a grid stride
}

extern "C" int64_t mmg_loss_save_doubles(int n_steps) {
    if (n_steps < 1 || n_steps > MMG_LOSS_MAX_STEPS) { fail("mmg_loss_save_doubles: n_steps must be in 1..%d (got %d)", MMG_LOSS_MAX_STEPS, n_steps); return -1; }
    return loss_save_doubles(n_steps);
}

extern "C" int mmg_loss_binary_forward(const float* d_feat, const float* d_prob, const float* d_logs, const float* d_scores,
                                       const uint8_t* d_mask, int n_steps, int batch, int width, int has_entropy,
                                       float entropy_penalty, float* d_loss, float* d_negent, double* d_save, void* stream) {
    if (loss_shape_ok("mmg_loss_binary_forward", n_steps, batch, width)) return -1;
    if (!d_feat || !d_prob || !d_logs || !d_scores || !d_loss || !d_negent || !d_save)
        return fail("mmg_loss_binary_forward: feat / prob / logs / scores / loss / negent / save must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_loss_binary_part, dim3(loss_slots(batch), n_steps), dim3(MMG_BLOCK), 0, st, d_feat, d_prob, d_logs, d_scores,
                       d_mask, n_steps, batch, width, d_save);
    hipLaunchKernelGGL(k_loss_finish<true>, dim3(1), dim3(MMG_BLOCK), 0, st, d_save, n_steps, batch, d_mask ? 1 : 0,
                       has_entropy ? 1 : 0, entropy_penalty, d_loss, d_negent);
    return launch_check("k_loss_binary");
}

extern "C" int mmg_loss_binary_vjp(const float* d_feat, const float* d_prob, const float* d_logs, const float* d_scores,
                                   const uint8_t* d_mask, const double* d_save, const float* d_dloss, const float* d_dnegent,
                                   int n_steps, int batch, int width, int has_entropy, float entropy_penalty, float* d_dprob,
                                   void* stream) {
    if (loss_shape_ok("mmg_loss_binary_vjp", n_steps, batch, width)) return -1;
    if (!d_feat || !d_prob || !d_logs || !d_scores || !d_save || !d_dprob)
        return fail("mmg_loss_binary_vjp: feat / prob / logs / scores / save / dprob must not be NULL");
    hipLaunchKernelGGL(k_loss_binary_vjp, dim3(loss_flat_grid((size_t)n_steps * batch * width)), dim3(MMG_BLOCK), 0, (hipStream_t)stream,
                       d_feat, d_prob, d_logs, d_scores, d_mask, d_save, d_dloss, d_dnegent, n_steps, batch, width,
                       has_entropy ? 1 : 0, entropy_penalty, d_dprob);
    return launch_check("k_loss_binary_vjp");
}

extern "C" int mmg_loss_bas_forward(const float* d_scores, const float* d_logs, const uint8_t* d_mask, int n_steps, int batch,
                                    float* d_loss, double* d_save, void* stream) {
    if (loss_shape_ok("mmg_loss_bas_forward", n_steps, batch, 1)) return -1;
    if (!d_scores || !d_logs || !d_loss || !d_save) return fail("mmg_loss_bas_forward: scores / logs / loss / save must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_loss_bas_part, dim3(loss_slots(batch), n_steps), dim3(MMG_BLOCK), 0, st, d_scores, d_logs, d_mask, n_steps,
                       batch, d_save);
    hipLaunchKernelGGL(k_loss_finish<false>, dim3(1), dim3(MMG_BLOCK), 0, st, d_save, n_steps, batch, d_mask ? 1 : 0, 0, 0.f, d_loss,
                       (float*)nullptr);
    return launch_check("k_loss_bas");
}

extern "C" int mmg_loss_bas_vjp(const float* d_scores, const float* d_logs, const uint8_t* d_mask, const double* d_save,
                                const float* d_dloss, int n_steps, int batch, float* d_dscores, void* stream) {
    if (loss_shape_ok("mmg_loss_bas_vjp", n_steps, batch, 1)) return -1;
    if (!d_scores || !d_logs || !d_save || !d_dscores) return fail("mmg_loss_bas_vjp: scores / logs / save / dscores must not be NULL");
    hipLaunchKernelGGL(k_loss_bas_vjp, dim3(loss_flat_grid((size_t)n_steps * batch)), dim3(MMG_BLOCK), 0, (hipStream_t)stream, d_scores,
                       d_logs, d_mask, d_save, d_dloss, n_steps, batch, d_dscores);
    return launch_check("k_loss_bas_vjp");
}

extern "C" int mmg_rec_outp_forward(const float* d_y, const uint8_t* d_ymask, const int64_t* d_target, int n_steps, int batch,
                                    int n_classes, float* d_outp, float* d_negent, float* d_logs, float* d_nll, double* d_save,
                                    void* stream) {
    if (loss_shape_ok("mmg_rec_outp_forward", n_steps, batch, n_classes)) return -1;
    if (!d_y || !d_outp || !d_negent || !d_save) return fail("mmg_rec_outp_forward: y / outp / negent / save must not be NULL");
    if (d_target && (!d_logs || !d_nll)) return fail("mmg_rec_outp_forward: with a target, logs and nll must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rec_outp_part, dim3(loss_slots(batch), n_steps), dim3(MMG_BLOCK), 0, st, d_y, d_ymask, d_target, n_steps, batch,
                       n_classes, d_outp, d_logs, d_save);
    hipLaunchKernelGGL(k_rec_outp_finish, dim3(1), dim3(MMG_BLOCK), 0, st, (const double*)d_save, n_steps, batch, d_negent,
                       d_target ? d_nll : (float*)nullptr);
    return launch_check("k_rec_outp");
}

extern "C" int mmg_rec_outp_vjp(const float* d_y, const uint8_t* d_ymask, const int64_t* d_target, const float* d_doutp,
                                const float* d_dnll, const float* d_dnegent, int n_steps, int batch, int n_classes, float* d_dy,
                                void* stream) {
    if (loss_shape_ok("mmg_rec_outp_vjp", n_steps, batch, n_classes)) return -1;
    if (!d_y || !d_dy) return fail("mmg_rec_outp_vjp: y / dy must not be NULL");
    const size_t blocks = ((size_t)n_steps * batch + MMG_BLOCK / 64 - 1) / (MMG_BLOCK / 64);
    hipLaunchKernelGGL(k_rec_outp_vjp, dim3((int)(blocks > 65536 ? 65536 : blocks)), dim3(MMG_BLOCK), 0, (hipStream_t)stream, d_y, d_ymask,
                       d_target, d_doutp, d_dnll, d_dnegent, n_steps, batch, n_classes, d_dy);
    return launch_check("k_rec_outp_vjp");
}

// ---------------------------------------------------------------------------------------------
// The pairwise code analysis (kernels_pairs.h): handle-free, on the calling thread's current device.  Two launches: the inverse
// norms of the meaning rows (and the row counts of the head), then one workgroup per 64 x 64 tile of the upper triangle.
// ---------------------------------------------------------------------------------------------
static int pair_shape_ok(const char* who, int64_t M, int W, int K) {
    if (M < 1 || W < 1) return fail("%s: the selected steps and w_dim must be positive (got %lld, %d)", who, (long long)M, W);
    if (K < 1 || K > MMG_PAIR_MAX_BINS) return fail("%s: n_bins must be in 1..%d (got %d)", who, MMG_PAIR_MAX_BINS, K);
    if (M > MMG_PAIR_MAX_SLOTS || pair_hist_slots(M, K) > MMG_PAIR_MAX_SLOTS)
        return fail("%s: 2 (M + 1) n_bins must be <= 2^24 (M = %lld selected bits, %d bins)", who, (long long)M, K);
    return 0;
}

extern "C" int64_t mmg_code_pair_hist_count(int n_sel_steps, int w_dim, int n_bins) {
    if (n_sel_steps < 1 || w_dim < 1) { fail("mmg_code_pair_hist_count: n_sel_steps and w_dim must be positive (got %d, %d)", n_sel_steps, w_dim); return -1; }
    const int64_t M = (int64_t)n_sel_steps * w_dim;
    if (pair_shape_ok("mmg_code_pair_hist_count", M, w_dim, n_bins)) return -1;
    return pair_hist_count(M, n_bins);
}

extern "C" int mmg_code_pair_hist(const uint32_t* d_codes, const int32_t* d_meta, int64_t n_rows, int T, int W, int agent, int t0, int t1,
                                  const float* d_meaning, int F, int64_t ld, float* d_inv, int n_bins, int64_t* d_hist, void* stream) {
    const char* who = "mmg_code_pair_hist";
    if (!d_codes || !d_meta || !d_meaning || !d_inv || !d_hist) return fail("%s: codes / meta / meaning / inv / hist must not be NULL", who);
    if (n_rows < 1 || n_rows > MMG_PAIR_MAX_ROWS) return fail("%s: n_rows must be in 1..%d (got %lld)", who, MMG_PAIR_MAX_ROWS, (long long)n_rows);
    if (F < 1 || F > MMG_PAIR_MAX_F) return fail("%s: F must be in 1..%d (got %d)", who, MMG_PAIR_MAX_F, F);
    if (ld < F) return fail("%s: the row stride ld must be >= F (got %lld < %d)", who, (long long)ld, F);
    if (agent != 0 && agent != 1) return fail("%s: agent must be 0 (sender) or 1 (receiver) (got %d)", who, agent);
    if (T < 1 || W < 1) return fail("%s: T and W must be positive (got %d, %d)", who, T, W);
    if (!(0 <= t0 && t0 < t1 && t1 <= T)) return fail("%s: the steps must satisfy 0 <= t0 < t1 <= T (got %d, %d, T = %d)", who, t0, t1, T);
    const int64_t M = (int64_t)(t1 - t0) * W;
    if (pair_shape_ok(who, M, W, n_bins)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int Wp = eval_code_wp(W);
    PairArgs ar;
    ar.codes = d_codes; ar.meta = d_meta; ar.x = d_meaning; ar.inv = d_inv; ar.hist = d_hist;
    ar.ld = ld; ar.row_words = eval_code_words(T, W); ar.sel0 = ((int64_t)agent * T + t0) * Wp;
    ar.n_rows = (int)n_rows; ar.F = F; ar.nw = (t1 - t0) * Wp; ar.M = (int)M; ar.K = n_bins;
    ar.n_tiles = (int)((n_rows + MMG_PAIR_TILE - 1) / MMG_PAIR_TILE);
    ar.codes_lds = pair_codes_in_lds(ar.nw) ? 1 : 0;
    ar.hist_lds = pair_hist_in_lds(ar.nw, pair_hist_slots(M, n_bins)) ? 1 : 0;
    const size_t dyn = (size_t)pair_code_lds_bytes(ar.nw) + (ar.hist_lds ? (size_t)pair_hist_slots(M, n_bins) * 4 : 0);
    hipLaunchKernelGGL(k_pair_norms, dim3((unsigned)((n_rows + MMG_BLOCK / 64 - 1) / (MMG_BLOCK / 64))), dim3(MMG_BLOCK), 0, st, d_meaning, ld, F,
                       d_meta, (int)n_rows, d_inv, d_hist);
    if (launch_check("k_pair_norms")) return -1;
    if (dyn > 48 * 1024) HIP_OK(hipFuncSetAttribute((const void*)k_pair_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(k_pair_hist, dim3((unsigned)((int64_t)ar.n_tiles * (ar.n_tiles + 1) / 2)), dim3(MMG_BLOCK), dyn, st, ar);
    return launch_check("k_pair_hist");
}
