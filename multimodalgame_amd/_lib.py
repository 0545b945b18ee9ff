"""ctypes binding of libmmg.so (include/mmg.h).  The product path has NO fallback: if the HIP
library is missing or a call fails, an exception is raised."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmg.so")

MMG_OPT = {"RMSprop": 0, "Adam": 1, "SGD": 2}
AGENTS = ("receiver", "sender", "baseline_rec", "baseline_sen")      # MMG_AGENT_* order


class MmgConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "global_batch", "batch_offset", "n_classes", "feat_dim", "h_dim", "w_dim", "rec_hidden",
        "wv_dim", "bas_hidden", "max_exchange", "use_binary", "fixed_exchange", "s_prob_prod",
        "has_entropy_s", "has_entropy_sen", "has_entropy_rec")] + [
        ("entropy_s", C.c_float), ("entropy_sen", C.c_float), ("entropy_rec", C.c_float),
        ("first_rec", C.c_float), ("optim_type", C.c_int32), ("learning_rate", C.c_float), ("top_k", C.c_int32),
        ("cu_budget", C.c_int32)]


class ParamEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("agent", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("offset", C.c_int64)]


class TapeEntry(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("dtype", C.c_int32), ("ndim", C.c_int32), ("dims", C.c_int64 * 4),
                ("offset", C.c_int64)]


class MmgError(RuntimeError):
    pass


class MmgWarning(RuntimeWarning):
    """A training call returned 1: the library recovered from a timed-out in-launch dependency (include/mmg.h: fail-soft)."""


_lib = None

# every symbol include/mmg.h declares (tests check that the library exports all of them)
SYMBOLS = ["mmg_last_error", "mmg_version", "mmg_param_count", "mmg_grad_floats", "mmg_param_table", "mmg_workspace_bytes",
           "mmg_tape_table", "mmg_create", "mmg_destroy", "mmg_exchange_forward", "mmg_loss_stats",
           "mmg_backward", "mmg_clip_step", "mmg_train_step", "mmg_sender_forward", "mmg_receiver_forward",
           "mmg_baseline_forward", "mmg_set_profiling", "mmg_get_kernel_times", "mmg_host_shuffle", "mmg_train_steps",
           "mmg_dp_set_allreduce", "mmg_dp_train_step", "mmg_dp_train_steps", "mmg_clear_error", "mmg_degraded",
           "mmg_log_snapshot_count", "mmg_log_snapshot", "mmg_set_message_corruption", "mmg_exchange_vjp",
           "mmg_sender_vjp", "mmg_receiver_vjp", "mmg_baseline_vjp", "mmg_eval_acc_count", "mmg_eval_steps",
           "mmg_loss_save_doubles", "mmg_loss_binary_forward", "mmg_loss_binary_vjp", "mmg_loss_bas_forward", "mmg_loss_bas_vjp",
           "mmg_rec_outp_forward", "mmg_rec_outp_vjp", "mmg_exchange_vjp_channel", "mmg_vjp_input_grads", "mmg_set_message_flipout",
           "mmg_plan_text", "mmg_plan_for", "mmg_set_sender_variant", "mmg_attn_param_count", "mmg_attn_grad_floats",
           "mmg_attn_param_table", "mmg_attn_workspace_bytes", "mmg_attn_tape_table", "mmg_attn_create", "mmg_set_desc_set",
           "mmg_vattn_param_count", "mmg_vattn_grad_floats", "mmg_vattn_param_table", "mmg_vattn_workspace_bytes",
           "mmg_vattn_tape_table", "mmg_vattn_create", "mmg_set_data_context", "mmg_vattn_reset_state", "mmg_set_message_relaxation",
           "mmg_set_trainable", "mmg_set_learning_rate", "mmg_set_entropy", "mmg_get_training_controls", "mmg_set_message_noise",
           "mmg_game_window_split", "mmg_game_window_counts", "mmg_eval_profile_count", "mmg_eval_steps_profile",
           "mmg_eval_code_words", "mmg_eval_steps_codes", "mmg_code_pair_hist_count", "mmg_code_pair_hist"]

# description attention (include/mmg.h: mmg_attn_create): the supported range
ATTN_MAX_DIM, ATTN_MAX_WORDS, ATTN_MAX_CLASSES, ATTN_MAX_BATCH = 128, 2048, 128, 512
# visual attention (include/mmg.h: mmg_vattn_create): attn_dim, locations of the map, context_dim, batch, batch * locations * attn_dim
VATTN_MAX_DIM, VATTN_MAX_FEATS, VATTN_MAX_CTX, VATTN_MAX_BATCH, VATTN_MAX_HX = 256, 256, 4096, 512, 1 << 25
VATTN_MAX_CHANNELS = 4096      # feat_dim of the map

# the caps of mmg_plan_for / the last line of mmg_plan_text (include/mmg.h: MMG_CAP_*): the CU count, then one occupancy per role kernel
PLAN_CAPS = ("n_cu", "split", "persist", "rc_bwd", "rc_persist", "mc", "mc3", "mc3p", "game", "wgrad_opt", "wgrad")
PLAN_NO_ROLES, PLAN_FLIPS, PLAN_VARIANT, PLAN_RELAX = 1, 2, 4, 8        # flags of mmg_plan_for
PLAN_FROZEN_SHIFT = 4                   # ... and agent_mask(frozen agents) << PLAN_FROZEN_SHIFT: the plan with those agents frozen
PLAN_NOISE = 256                        # ... and Gaussian message noise is set (bits 4-7 are the frozen agents')
MIX = {"sum": 0, "prod": 1}             # mmg_set_sender_variant's mix (include/mmg.h: MMG_MIX_SUM, MMG_MIX_PROD)

# the accumulator of mmg_eval_steps (include/mmg.h): EVAL_ACC_HEAD scalars -- hits, batches, samples, 0 -- then conf [D, D], seen [D]
EVAL_ACC_HEAD = 4
# the accumulator of mmg_eval_steps_profile: EVAL_PROF_HEAD scalars -- batches, samples with a valid target, samples without, 0 --
# then steps [D, T], rank [T, D], class_hits [D], class_ranksum [D], msg_sen [T, D, W], msg_rec [T, D, W]
EVAL_PROF_HEAD = 4
# the per-sample codes of mmg_eval_steps_codes: codes [rows, EVAL_CODE_AGENTS, T, code_wp(W)] uint32 (agent 0 the sender, 1 the
# receiver; EVAL_CODE_BITS message bits to a word), meta [rows, EVAL_CODE_META] int32 (output step, target or -1)
EVAL_CODE_AGENTS, EVAL_CODE_BITS, EVAL_CODE_META = 2, 32, 2
EVAL_CODE_SENDER, EVAL_CODE_RECEIVER = 0, 1
# the histogram of mmg_code_pair_hist: PAIR_HIST_HEAD scalars -- rows used, rows skipped, pairs counted, 0 -- then hist [2, M + 1, bins];
# its limits: rows, columns of the meaning matrix, bins, 2 (M + 1) bins
PAIR_HIST_HEAD = 4
PAIR_MAX_ROWS, PAIR_MAX_F, PAIR_MAX_BINS, PAIR_MAX_SLOTS = 65536, 4096, 1024, 1 << 24


def code_wp(w_dim):
    """Words of a packed W-bit message."""
    return (int(w_dim) + EVAL_CODE_BITS - 1) // EVAL_CODE_BITS


def load():
    """Load libmmg.so; raises MmgError when it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MmgError("HIP library %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                       "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, fp = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_void_p
    cfgp = C.POINTER(MmgConfig)
    lib.mmg_last_error.restype = C.c_char_p
    lib.mmg_version.restype = i32
    lib.mmg_param_count.restype = i64; lib.mmg_param_count.argtypes = [cfgp]
    lib.mmg_grad_floats.restype = i64; lib.mmg_grad_floats.argtypes = [cfgp]
    lib.mmg_param_table.restype = i32; lib.mmg_param_table.argtypes = [cfgp, C.POINTER(ParamEntry), i32]
    lib.mmg_workspace_bytes.restype = i64; lib.mmg_workspace_bytes.argtypes = [cfgp]
    lib.mmg_tape_table.restype = i32; lib.mmg_tape_table.argtypes = [cfgp, C.POINTER(TapeEntry), i32]
    lib.mmg_create.restype = vp; lib.mmg_create.argtypes = [cfgp, vp, i64, fp, fp, fp]
    lib.mmg_destroy.restype = None; lib.mmg_destroy.argtypes = [vp]
    lib.mmg_attn_param_count.restype = i64; lib.mmg_attn_param_count.argtypes = [cfgp, i32, i32]
    lib.mmg_attn_grad_floats.restype = i64; lib.mmg_attn_grad_floats.argtypes = [cfgp, i32, i32]
    lib.mmg_attn_param_table.restype = i32; lib.mmg_attn_param_table.argtypes = [cfgp, i32, i32, C.POINTER(ParamEntry), i32]
    lib.mmg_attn_workspace_bytes.restype = i64; lib.mmg_attn_workspace_bytes.argtypes = [cfgp, i32, i32]
    lib.mmg_attn_tape_table.restype = i32; lib.mmg_attn_tape_table.argtypes = [cfgp, i32, i32, C.POINTER(TapeEntry), i32]
    lib.mmg_attn_create.restype = vp; lib.mmg_attn_create.argtypes = [cfgp, i32, i32, vp, i64, fp, fp, fp]
    lib.mmg_set_desc_set.restype = i32; lib.mmg_set_desc_set.argtypes = [vp, fp, C.POINTER(C.c_int32), i32]
    lib.mmg_vattn_param_count.restype = i64; lib.mmg_vattn_param_count.argtypes = [cfgp, i32, i32, i32]
    lib.mmg_vattn_grad_floats.restype = i64; lib.mmg_vattn_grad_floats.argtypes = [cfgp, i32, i32, i32]
    lib.mmg_vattn_param_table.restype = i32; lib.mmg_vattn_param_table.argtypes = [cfgp, i32, i32, i32, C.POINTER(ParamEntry), i32]
    lib.mmg_vattn_workspace_bytes.restype = i64; lib.mmg_vattn_workspace_bytes.argtypes = [cfgp, i32, i32, i32]
    lib.mmg_vattn_tape_table.restype = i32; lib.mmg_vattn_tape_table.argtypes = [cfgp, i32, i32, i32, C.POINTER(TapeEntry), i32]
    lib.mmg_vattn_create.restype = vp; lib.mmg_vattn_create.argtypes = [cfgp, i32, i32, i32, vp, i64, fp, fp, fp]
    lib.mmg_set_data_context.restype = i32; lib.mmg_set_data_context.argtypes = [vp, fp]
    lib.mmg_vattn_reset_state.restype = i32; lib.mmg_vattn_reset_state.argtypes = [vp]
    lib.mmg_exchange_forward.restype = i32
    lib.mmg_exchange_forward.argtypes = [vp, fp, vp, fp, fp, fp, fp, u64, i32, i32, vp]
    lib.mmg_loss_stats.restype = i32; lib.mmg_loss_stats.argtypes = [vp, vp]
    lib.mmg_backward.restype = i32; lib.mmg_backward.argtypes = [vp, fp, vp, fp, vp]
    lib.mmg_clip_step.restype = i32; lib.mmg_clip_step.argtypes = [vp, vp]
    lib.mmg_train_step.restype = i32; lib.mmg_train_step.argtypes = [vp, fp, vp, fp, fp, fp, fp, u64, vp]
    lib.mmg_train_steps.restype = i32; lib.mmg_train_steps.argtypes = [vp, fp, vp, i64, fp, u64, vp]
    lib.mmg_eval_acc_count.restype = i64; lib.mmg_eval_acc_count.argtypes = [cfgp]
    lib.mmg_eval_steps.restype = i32; lib.mmg_eval_steps.argtypes = [vp, fp, vp, i64, fp, i32, vp, vp, vp, vp]
    lib.mmg_eval_profile_count.restype = i64; lib.mmg_eval_profile_count.argtypes = [cfgp]
    lib.mmg_eval_steps_profile.restype = i32; lib.mmg_eval_steps_profile.argtypes = [vp, fp, vp, i64, fp, i32, vp, vp, vp, vp, vp]
    lib.mmg_eval_code_words.restype = i64; lib.mmg_eval_code_words.argtypes = [cfgp]
    lib.mmg_eval_steps_codes.restype = i32
    lib.mmg_eval_steps_codes.argtypes = [vp, fp, vp, i64, fp, i32, vp, vp, vp, vp, vp, vp, i64, i64, vp]
    lib.mmg_code_pair_hist_count.restype = i64; lib.mmg_code_pair_hist_count.argtypes = [i32, i32, i32]
    lib.mmg_code_pair_hist.restype = i32
    lib.mmg_code_pair_hist.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, fp, i32, i64, fp, i32, vp, vp]
    lib.mmg_set_message_corruption.restype = i32; lib.mmg_set_message_corruption.argtypes = [vp, vp, i32]
    lib.mmg_set_message_flipout.restype = i32; lib.mmg_set_message_flipout.argtypes = [vp, i32, C.c_float, i32, C.c_float, i32, u64]
    lib.mmg_set_sender_variant.restype = i32; lib.mmg_set_sender_variant.argtypes = [vp, i32, i32, i32]
    lib.mmg_set_message_relaxation.restype = i32; lib.mmg_set_message_relaxation.argtypes = [vp, C.c_float, C.c_float, i32]
    lib.mmg_set_message_noise.restype = i32; lib.mmg_set_message_noise.argtypes = [vp, C.c_float, C.c_float, i32, u64]
    lib.mmg_set_trainable.restype = i32; lib.mmg_set_trainable.argtypes = [vp, i32]
    lib.mmg_set_learning_rate.restype = i32; lib.mmg_set_learning_rate.argtypes = [vp, C.c_float]
    lib.mmg_set_entropy.restype = i32; lib.mmg_set_entropy.argtypes = [vp, C.c_float, C.c_float, C.c_float]
    lib.mmg_get_training_controls.restype = i32
    lib.mmg_get_training_controls.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mmg_exchange_vjp.restype = i32; lib.mmg_exchange_vjp.argtypes = [vp, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.mmg_exchange_vjp_channel.restype = i32; lib.mmg_exchange_vjp_channel.argtypes = [vp, i32, fp, fp, fp, fp, fp, fp, vp]
    lib.mmg_vjp_input_grads.restype = i32; lib.mmg_vjp_input_grads.argtypes = [vp, i32, i32, fp, fp, fp, vp]
    lib.mmg_sender_vjp.restype = i32; lib.mmg_sender_vjp.argtypes = [vp, fp, fp, i32, fp, fp, fp, fp, fp, fp, vp]
    lib.mmg_receiver_vjp.restype = i32
    lib.mmg_receiver_vjp.argtypes = [vp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.mmg_baseline_vjp.restype = i32; lib.mmg_baseline_vjp.argtypes = [vp, i32, fp, fp, fp, i32, fp, fp, fp, fp, vp]
    # the loss functions (handle-free): pointers, then sizes; see include/mmg.h
    f32 = C.c_float
    lib.mmg_loss_save_doubles.restype = i64; lib.mmg_loss_save_doubles.argtypes = [i32]
    lib.mmg_loss_binary_forward.restype = i32
    lib.mmg_loss_binary_forward.argtypes = [fp, fp, fp, fp, vp, i32, i32, i32, i32, f32, fp, fp, vp, vp]
    lib.mmg_loss_binary_vjp.restype = i32
    lib.mmg_loss_binary_vjp.argtypes = [fp, fp, fp, fp, vp, vp, fp, fp, i32, i32, i32, i32, f32, fp, vp]
    lib.mmg_loss_bas_forward.restype = i32; lib.mmg_loss_bas_forward.argtypes = [fp, fp, vp, i32, i32, fp, vp, vp]
    lib.mmg_loss_bas_vjp.restype = i32; lib.mmg_loss_bas_vjp.argtypes = [fp, fp, vp, vp, fp, i32, i32, fp, vp]
    lib.mmg_rec_outp_forward.restype = i32; lib.mmg_rec_outp_forward.argtypes = [fp, vp, vp, i32, i32, i32, fp, fp, fp, fp, vp, vp]
    lib.mmg_rec_outp_vjp.restype = i32; lib.mmg_rec_outp_vjp.argtypes = [fp, vp, vp, fp, fp, fp, i32, i32, i32, fp, vp]
    lib.mmg_dp_set_allreduce.restype = i32; lib.mmg_dp_set_allreduce.argtypes = [vp, vp, vp]
    lib.mmg_dp_train_step.restype = i32; lib.mmg_dp_train_step.argtypes = [vp, fp, vp, fp, fp, fp, fp, u64, i32, i32, vp]
    lib.mmg_dp_train_steps.restype = i32; lib.mmg_dp_train_steps.argtypes = [vp, fp, vp, i64, fp, u64, i32, vp]
    lib.mmg_clear_error.restype = i32; lib.mmg_clear_error.argtypes = [vp, vp]
    lib.mmg_degraded.restype = i32; lib.mmg_degraded.argtypes = [vp]
    lib.mmg_plan_text.restype = i32; lib.mmg_plan_text.argtypes = [vp, C.c_char_p, i32]
    lib.mmg_plan_for.restype = i32; lib.mmg_plan_for.argtypes = [cfgp, C.POINTER(C.c_int32), i32, i32, C.c_char_p, i32]
    lib.mmg_game_window_split.restype = i32; lib.mmg_game_window_split.argtypes = [i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mmg_game_window_counts.restype = i32; lib.mmg_game_window_counts.argtypes = [i32, i32, i32, C.POINTER(C.c_int32)]
    lib.mmg_log_snapshot_count.restype = i64; lib.mmg_log_snapshot_count.argtypes = [cfgp, i32, i32]
    lib.mmg_log_snapshot.restype = i32; lib.mmg_log_snapshot.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.mmg_sender_forward.restype = i32
    lib.mmg_sender_forward.argtypes = [vp, fp, fp, i32, i32, fp, u64, fp, fp, fp, vp]
    lib.mmg_receiver_forward.restype = i32
    lib.mmg_receiver_forward.argtypes = [vp, fp, fp, fp, fp, i32, i32, i32, fp, fp, u64, fp, fp, fp, fp, fp, fp, vp]
    lib.mmg_baseline_forward.restype = i32; lib.mmg_baseline_forward.argtypes = [vp, i32, fp, fp, fp, i32, fp, vp]
    lib.mmg_host_shuffle.restype = i32; lib.mmg_host_shuffle.argtypes = [vp, i32, i64, vp]
    lib.mmg_set_profiling.restype = i32; lib.mmg_set_profiling.argtypes = [vp, i32]
    lib.mmg_get_kernel_times.restype = i32
    lib.mmg_get_kernel_times.argtypes = [vp, C.c_char_p, i32, C.POINTER(C.c_float), i32]
    _lib = lib
    return lib


def check(status):
    """0 = ok; 1 = ok with a warning (the library recovered from a timed-out in-launch dependency and continues on the launches
    without in-launch waits: reported once per event as MmgWarning); negative = error."""
    if status == 0:
        return
    if status > 0:
        import warnings
        warnings.warn(MmgWarning(load().mmg_last_error().decode()), stacklevel=3)
        return
    raise MmgError(load().mmg_last_error().decode())


def make_config(batch, n_classes, feat_dim, h_dim, w_dim, rec_hidden, wv_dim, bas_hidden, max_exchange,
                use_binary=True, fixed_exchange=True, s_prob_prod=True, entropy_s=None, entropy_sen=None,
                entropy_rec=None, first_rec=0.0, optim_type="RMSprop", learning_rate=1e-4, top_k=6,
                global_batch=None, batch_offset=0, cu_budget=0):
    """cu_budget: compute units this process can count on (0 = the whole device; include/mmg.h)."""
    c = MmgConfig()
    c.batch, c.global_batch, c.batch_offset = batch, global_batch or batch, batch_offset
    c.n_classes, c.feat_dim, c.h_dim, c.w_dim = n_classes, feat_dim, h_dim, w_dim
    c.rec_hidden, c.wv_dim, c.bas_hidden, c.max_exchange = rec_hidden, wv_dim, bas_hidden, max_exchange
    c.use_binary, c.fixed_exchange, c.s_prob_prod = int(bool(use_binary)), int(bool(fixed_exchange)), int(bool(s_prob_prod))
    c.has_entropy_s, c.has_entropy_sen, c.has_entropy_rec = [int(v is not None) for v in (entropy_s, entropy_sen, entropy_rec)]
    c.entropy_s, c.entropy_sen, c.entropy_rec = [float(v or 0.0) for v in (entropy_s, entropy_sen, entropy_rec)]
    c.first_rec, c.optim_type, c.learning_rate, c.top_k = float(first_rec), MMG_OPT[optim_type], float(learning_rate), int(top_k)
    c.cu_budget = int(cu_budget or 0)
    return c


def param_table(cfg, attn_dim=0, n_words=0, vattn=None):
    """The flat buffer's tensors; attn_dim > 0: of an attention handle (include/mmg.h: mmg_attn_param_table); vattn = (attn_dim,
    n_feats, context_dim): of a visual-attention handle (mmg_vattn_param_table)."""
    lib = load()
    fn, dims = (lib.mmg_vattn_param_table, tuple(vattn)) if vattn else (lib.mmg_attn_param_table, (attn_dim, n_words))
    n = fn(C.byref(cfg), *dims, None, 0)
    if n < 0:
        raise MmgError(lib.mmg_last_error().decode())
    arr = (ParamEntry * n)()
    check(0 if fn(C.byref(cfg), *dims, arr, n) == n else -1)
    return [dict(name=e.name.decode(), agent=AGENTS[e.agent], rows=e.rows, cols=e.cols, offset=e.offset) for e in arr]


def tape_table(cfg, attn_dim=0, n_words=0, vattn=None):
    lib = load()
    fn, dims = (lib.mmg_vattn_tape_table, tuple(vattn)) if vattn else (lib.mmg_attn_tape_table, (attn_dim, n_words))
    n = fn(C.byref(cfg), *dims, None, 0)
    if n < 0:
        raise MmgError(lib.mmg_last_error().decode())
    arr = (TapeEntry * n)()
    check(0 if fn(C.byref(cfg), *dims, arr, n) == n else -1)
    return [dict(name=e.name.decode(), dtype=e.dtype, dims=[int(e.dims[i]) for i in range(e.ndim)], offset=e.offset)
            for e in arr]


def agent_mask(agents):
    """MMG_AGENT_* bits of a collection of agent names (mmg_set_trainable's mask); raises ValueError for a name that is no agent."""
    mask = 0
    for a in agents:
        if a not in AGENTS:
            raise ValueError("%r is no agent: one of %s" % (a, ", ".join(AGENTS)))
        mask |= 1 << AGENTS.index(a)
    return mask


def plan_for(cfg, caps, flags=0):
    """The kernel selection of `cfg` on a device with these caps (PLAN_CAPS order), as mmg_plan_text prints it.  Host only."""
    buf = C.create_string_buffer(4096)
    arr = (C.c_int32 * len(caps))(*caps)
    check(load().mmg_plan_for(C.byref(cfg), arr, len(caps), flags, buf, len(buf)))
    return buf.value.decode()


def game_window_split(nslots, n):
    """(w / nslots, w % nslots) for w = 0 .. n - 1 as k_game_fast's baseline roles form them (game_windows.h).  Host only.
    This entry and mmg_game_window_counts exist for tests/test_game_windows_cpu.py alone: they expose a detail of one kernel, no
    caller should build on them, and they go when the kernel stops cutting its rows into slot windows."""
    import numpy as np
    kw, slot = np.empty(n, np.int32), np.empty(n, np.int32)
    i32p = C.POINTER(C.c_int32)
    check(load().mmg_game_window_split(nslots, n, kw.ctypes.data_as(i32p), slot.ctypes.data_as(i32p)))
    return kw, slot


def game_window_counts(nslots, slot, n):
    """Windows of `slot` in a minibatch of nw windows, nw = 0 .. n - 1, as the kernel forms them.  Host only."""
    import numpy as np
    count = np.empty(n, np.int32)
    check(load().mmg_game_window_counts(nslots, slot, n, count.ctypes.data_as(C.POINTER(C.c_int32))))
    return count


def plan_caps(text):
    """The caps a plan text ends with, in PLAN_CAPS order."""
    words = text.strip().splitlines()[-1].split()
    assert words[:2] == ["mmg_create:", "caps"] and tuple(words[2::2]) == PLAN_CAPS, text
    return [int(v) for v in words[3::2]]
