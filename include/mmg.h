/*
 * mmg.h -- C-ABI of the MI355X-native REINFORCE exchange path (libmmg.so).
 *
 * The reference (nyu-dl/MultimodalGame) has no FFI: its hot path is reached through the
 * Python objects of model.py.  This header is the boundary a maintainer would bind (ctypes,
 * see INTEGRATION.md) to replace exactly these reference call sites:
 *
 *   mmg_exchange_forward   <- exchange()                    model.py:725-876  (called at 1240, 640)
 *                             + output selection / NLL      model.py:879-904, 1264-1275
 *   mmg_loss_stats         <- mask derivation + the batch statistics of
 *                             multistep_loss_binary/_bas    model.py:1248-1262, 907-988
 *   mmg_backward           <- the four loss.backward()      model.py:1309, 1316, 1322, 1328
 *   mmg_clip_step          <- clip_grad_norm + optimizer    model.py:1310-1311, 1317-1318, 1323-1324, 1329-1330
 *   mmg_train_step         <- the whole per-minibatch block model.py:1240-1339 (single GPU)
 *   mmg_train_steps        <- n iterations of the epoch loop's body, model.py:1218-1240 (batches of misc.py:257-302)
 *   mmg_eval_steps         <- n iterations of eval_dev's loop body: exchange(train = False) + the per-batch
 *                             accuracy / confusion / length / Hamming arithmetic   model.py:620-691
 *   mmg_eval_steps_profile <- the same, plus per batch the counts behind the -binary_only dump's analysis (rank of the target,
 *                             stop step and both messages per sample and step)    binary_vectors.py:24-46, 89-141
 *   mmg_eval_steps_codes   <- the same, plus per sample the packed bits of both messages (the dump's "BinaryVec" records of
 *                             both agents)                                           binary_vectors.py:101-126
 *   mmg_code_pair_hist     <- the pairwise analysis of such a dump: Hamming against meaning distance over all pairs of samples
 *   mmg_dp_train_step[s]   <- the same block on one rank of a data-parallel job (statistics + gradient
 *                             all-reduce; couplings model.py:912-915, 947-961, 1310)
 *   mmg_sender_forward     <- Sender.forward                model.py:144-238 (sender_mix=sum; the attention branch on a handle of mmg_vattn_create)
 *   mmg_receiver_forward   <- Receiver.forward              model.py:303-477 (the desc_attn branch on a handle of mmg_attn_create)
 *   mmg_baseline_forward   <- Baseline.forward              model.py:496-516
 *   mmg_exchange_vjp       <- loss.backward() of ONE agent's graph for any loss built from exchange()'s outputs
 *                             (model.py:1309, 1316, 1322, 1328; graphs split at model.py:807-811, 826-829, 835-843)
 *   mmg_exchange_vjp_channel <- (no call site: the reference detaches the messages, model.py:807-811, 826-829) backward()
 *                             through the sender and the receiver as ONE graph, gradients crossing the channel
 *   mmg_sender_vjp         <- backward() through ONE Sender.forward call      model.py:193-238
 *   mmg_receiver_vjp       <- backward() through ONE Receiver.forward call    model.py:333-474
 *   mmg_baseline_vjp       <- backward() through ONE Baseline.forward call    model.py:496-516
 *   mmg_loss_binary_forward / _vjp <- multistep_loss_binary and its backward  model.py:907-968
 *   mmg_loss_bas_forward / _vjp    <- multistep_loss_bas and its backward     model.py:971-988
 *   mmg_rec_outp_forward / _vjp    <- get_rec_outp + log_softmax + nll_loss + loglikelihood and their backward
 *                                                                             model.py:879-904, 1264-1275, 571-577
 *
 * Conventions
 *   - plain pointers and sizes; every pointer named d_* is DEVICE memory owned by the caller
 *     (torch tensors' data_ptr()).  The library never allocates device memory: the caller hands
 *     it one workspace of mmg_workspace_bytes() bytes at mmg_create().
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*, 0 = null stream) and is
 *     asynchronous w.r.t. the host; no host synchronisation happens inside any call.
 *   - return value: 0 = ok, negative = error (message via mmg_last_error()), 1 = ok with a warning in
 *     mmg_last_error() (training entry points only: the library recovered from a timed-out in-launch
 *     dependency, see mmg_clear_error); nothing throws across the ABI.  One handle per device per process; not thread-safe (the reference is
 *     single-threaded).
 *   - all floating-point data is fp32, row-major, PyTorch [out,in] weight layout; masks are
 *     uint8; targets int64 (as the reference's LongTensor).
 */
#ifndef MMG_H_
#define MMG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMG_VERSION 3
#define MMG_GRAD_TAIL 4       /* floats behind the gradients in d_grads, owned by the library (see mmg_grad_floats) */

enum { MMG_OPT_RMSPROP = 0, MMG_OPT_ADAM = 1, MMG_OPT_SGD = 2 };          /* model.py:1725 */
enum { MMG_AGENT_RECEIVER = 0, MMG_AGENT_SENDER = 1, MMG_AGENT_BASELINE_REC = 2, MMG_AGENT_BASELINE_SEN = 3 };

/* Frozen copy of the gflags the hot path reads (model.py:1639-1741). */
typedef struct mmg_config {
    int32_t batch;            /* B: samples handled by THIS process (-batch_size / world_size)      */
    int32_t global_batch;     /* samples of the whole minibatch over all ranks (== batch if 1 GPU)   */
    int32_t batch_offset;     /* index of this rank's first sample inside the global minibatch       */
    int32_t n_classes;        /* D: rows of the description matrix                                   */
    int32_t feat_dim;         /* F: -img_feat_dim                                                    */
    int32_t h_dim;            /* H: -img_h_dim                                                       */
    int32_t w_dim;            /* W: -rec_w_dim == -sender_out_dim (model.py:1756)                    */
    int32_t rec_hidden;       /* R: -rec_hidden                                                      */
    int32_t wv_dim;           /* V: -wv_dim                                                          */
    int32_t bas_hidden;       /* K: -baseline_hid_dim                                                */
    int32_t max_exchange;     /* T: -max_exchange                                                    */
    int32_t use_binary;       /* -use_binary                                                         */
    int32_t fixed_exchange;   /* -fixed_exchange                                                     */
    int32_t s_prob_prod;      /* -s_prob_prod (eval-mode stop bit, model.py:423-427)                 */
    int32_t has_entropy_s, has_entropy_sen, has_entropy_rec;   /* flag is not None (model.py:925)    */
    float   entropy_s, entropy_sen, entropy_rec;               /* model.py:1730-1732                 */
    float   first_rec;        /* -first_rec (model.py:786)                                           */
    int32_t optim_type;       /* MMG_OPT_*                                                           */
    float   learning_rate;    /* -learning_rate                                                      */
    int32_t top_k;            /* -top_k_train                                                        */
    int32_t cu_budget;        /* compute units this process can count on (0 = the whole device).  The persistent
                                 "role" launches need their workgroups co-resident; their budgets are sized from this
                                 number, and a budget they do not fit selects launches without in-launch waits up front.
                                 Set it when the GPU is shared or the process runs under a CU mask (no reference
                                 counterpart: additive)                                                              */
} mmg_config;

/* One parameter tensor inside the flat parameter / gradient / optimizer-state buffers. */
typedef struct mmg_param_entry {
    char    name[48];         /* state_dict key, e.g. "rnn.weight_ih" (SURVEY.md §8 b)               */
    int32_t agent;            /* MMG_AGENT_*                                                         */
    int32_t rows, cols;       /* cols == 0 for 1-D tensors                                           */
    int64_t offset;           /* in floats from the start of the flat buffer (16-byte aligned)       */
} mmg_param_entry;

/* One named array inside the workspace ("tape"): everything exchange() returns plus what the
 * backward pass re-reads. */
typedef struct mmg_tape_entry {
    char    name[32];
    int32_t dtype;            /* 0 = f32, 1 = u8, 2 = i32, 3 = f64                                   */
    int32_t ndim;
    int64_t dims[4];
    int64_t offset;           /* bytes from the start of the workspace                               */
} mmg_tape_entry;

typedef struct mmg_handle mmg_handle;

const char* mmg_last_error(void);
int     mmg_version(void);

/* Layout queries (host only, no GPU needed). */
int64_t mmg_param_count(const mmg_config* cfg);                                   /* floats incl. padding */
/* Floats the caller allocates for d_grads: mmg_param_count() + MMG_GRAD_TAIL.  The tail quad is written by mmg_backward:
 * [0] = 1.0 if an in-launch dependency wait of this minibatch timed out on this rank (stale gradients), else 0.0.  A
 * data-parallel caller all-reduces (sum) ALL mmg_grad_floats() floats, so the flag reaches every rank with the gradients
 * and mmg_clip_step skips the update on all ranks alike (the reference has no counterpart: model.py:1307-1330 is
 * single-process); [1], [2] = this rank's sum of rewards (log-likelihood of the target, model.py:1274) and top-k hit count,
 * from which mmg_clip_step rewrites the logged NLL / hits of the GLOBAL minibatch in continuous mode (use_binary == 0), where
 * the shards couple through nothing else and no statistics all-reduce is needed; [3] = 0. */
int64_t mmg_grad_floats(const mmg_config* cfg);
int     mmg_param_table(const mmg_config* cfg, mmg_param_entry* out, int max_entries);   /* returns count */
int64_t mmg_workspace_bytes(const mmg_config* cfg);
int     mmg_tape_table(const mmg_config* cfg, mmg_tape_entry* out, int max_entries);     /* returns count */

/* d_params: flat fp32 buffer of mmg_param_count() floats; d_grads: mmg_grad_floats() floats.  d_opt_state: 2x mmg_param_count()
 * (RMSprop square_avg | unused; Adam exp_avg | exp_avg_sq; SGD unused), zero-initialised by the
 * caller.  d_workspace: mmg_workspace_bytes() bytes, 256-byte aligned. */
mmg_handle* mmg_create(const mmg_config* cfg, void* d_workspace, int64_t workspace_bytes,
                       float* d_params, float* d_grads, float* d_opt_state);
void    mmg_destroy(mmg_handle* h);

/* Runs the T-step conversation of one minibatch (model.py:725-876) and the output selection /
 * log-softmax / NLL reward (model.py:879-904, 1264-1275).
 *   d_x [B,F] f32, d_target [B] i64 (may be NULL when train==0 and no accuracy is wanted),
 *   d_desc [D,V] f32.
 *   Sampling (train==1): if d_u_z/d_u_s/d_u_w ([T,B,W],[T,B],[T,B,W] f32 uniforms, the reference's
 *   np.random.rand draws in its call order) are non-NULL they are consumed; otherwise the in-kernel
 *   Philox4x32-10 generator keyed by (seed, the handle's device-side minibatch counter) is used.
 *   train==0: messages are round(p), stop bit round(prod p_s) (model.py:229, 423-427, 462).
 *   run_all_steps==1: every sample runs all T steps (what exchange() returns to Python);
 *   ==0: a sample stops computing once its own conversation has ended (its later steps are masked
 *   out of every loss, so training results are identical); per-(step, sample) arrays -- messages,
 *   baseline scores and hiddens, gradient tapes -- are then defined on the LIVE rows only
 *   (t <= the sample's own last step); the others keep whatever an earlier call left there.
 *   ==2: as 0, and only what the training step itself reads is guaranteed to be stored: in Fixed mode the class logits "y"
 *   are kept for the output step (T-1) only -- the losses read nothing else of them (model.py:885-904, 1264-1275) -- and in
 *   continuous mode (only the receiver is trained, model.py:1313) the sender-side and message arrays (a, c, zr, dbar, g, w)
 *   may be left unwritten.  This is what mmg_train_step runs.
 *   ==3 (train == 1): every sample runs all T steps, as with 1 -- messages, probabilities, stop bits, masks and class logits
 *   of every (step, sample) are on the tape -- but the baselines are the training step's: their scores "bs" / "br" are defined
 *   on the live rows only.  For the minibatches whose log block prints the whole conversation (model.py:1342-1518), which
 *   prints no baseline score.
 * Results land in the workspace arrays listed by mmg_tape_table(). */
int mmg_exchange_forward(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                         const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed,
                         int train, int run_all_steps, void* stream);

/* Message corruption of evaluation conversations (-bit_flip -corrupt_region; the reference's eval_dev passes it to exchange(),
 * model.py:637-638).  mask: host array of n == w_dim entries, each 0 or 1 (misc.py:388-402: build_mask(corrupt_region, W));
 * NULL clears it.  Host only: no GPU work, the mask travels with every later launch as a kernel argument.  While it is set:
 *   - mmg_exchange_forward(train = 0) replaces the sender's message of every step by z <- |z - m| (model.py:813-820), m
 *     broadcast over the batch, before the receiver reads it: the tape's "z" holds the corrupted message, "pz" (the sender's
 *     probabilities) does not change.  Binary messages: the masked bits are inverted.  Continuous messages (use_binary == 0,
 *     z = the raw binary_layer output): EVERY entry becomes |z| and the masked ones |z - 1| -- the abs applies to all entries;
 *   - the training entries (mmg_exchange_forward(train = 1), mmg_train_step[s], mmg_dp_train_step[s]) return an error instead
 *     of running: the reference never corrupts a training conversation (model.py:1240).
 * Returns 0, or negative for n != w_dim or an entry other than 0 / 1 (the mask set before stays). */
int mmg_set_message_corruption(mmg_handle* h, const uint8_t* mask, int n);

/* Random message flips, the noisy channel of -flipout_sen / -flipout_rec / -flipout_dev (model.py:233-234, 467-468, 554-568).
 * has_sen / has_rec: the sender's / the receiver's message flips with probability p_sen / p_rec in [0, 1]; both zero clears the
 * setting.  Binary messages only (use_binary == 0: accepted, nothing happens -- the reference does not flip continuous messages).
 * While it is set, every later forward entry (mmg_exchange_forward, mmg_train_step[s], mmg_dp_train_step[s], mmg_eval_steps,
 * mmg_sender_forward, mmg_receiver_forward) replaces a message bit, right after it was sampled (training) or rounded
 * (evaluation), by |bit - m| with m = 1 iff a uniform draw lies below the probability (a float32 compare: p = 0 never flips,
 * p = 1 always).  Training conversations always flip; evaluation conversations only with flipout_dev != 0.  The flipped bit is
 * what everything downstream reads: the other agent, both baselines, the tape arrays "z" / "w" / "zr", the log-likelihood
 * sums "lp_z" / "lp_w" (model.py:908-910 scores the returned bits), the backward pass and mmg_eval_steps' Hamming counts;
 * "pz" / "pw" and the entropy terms stay functions of the logits.  A mask of mmg_set_message_corruption is applied after the flip.
 * Draws: philox_uniform(key, e, c1, stream) at the element index of the Bernoulli draws, e = (t * B_global + batch_offset + b) * W
 * + j, so a data-parallel shard draws what the single-GPU batch draws.
 *   training:   streams 3 (sender) / 4 (receiver), key = the call's seed, c1 = the minibatch counter of the Bernoulli draws --
 *               also when d_u_z / d_u_s / d_u_w are injected;
 *   evaluation: streams 5 / 6, key = eval_seed, c1 = the number of evaluation conversations enqueued on this handle since this
 *               call (counted on the host; the device-side minibatch counter stays untouched).  The agent-level entries draw
 *               with the count of the conversation the last mmg_sender_forward(t = 0, train = 0) began.
 * Kernels: a flipping handle runs the register-resident k_conversation_fast3 chain (configs 1-3's agents; mmg_train_step then
 * launches k_conversation_fast3 + k_bwd_conv_fast + k_wgrad instead of the one-launch k_game_fast) or the generic per-sample
 * kernels (every other shape: the many-class, sample-tile and wide-receiver kernels do not flip).  The call re-runs the kernel
 * selection and does no other GPU work; clearing restores the original selection.
 * Returns 0, or negative for a probability outside [0, 1] or NaN (the setting before stays). */
int mmg_set_message_flipout(mmg_handle* h, int has_sen, float p_sen, int has_rec, float p_rec, int flipout_dev, uint64_t eval_seed);

/* The sender's communication ablations, -sender_mix prod / -ignore_code / -ignore_receiver (model.py:217-218, 208-210, 470-472).
 * With h_x = image_layer(x) and h_w = code_layer(c_t), c_0 = sigmoid(code_bias), c_t = w_{t-1}:
 *   mix = MMG_MIX_SUM   a_t = tanh(h_x + h_w)   (the default)
 *   mix = MMG_MIX_PROD  a_t = tanh(h_x * h_w), at t = 0 too; backward: dpre = (W_b^T dlz)(1 - a_t^2), d h_x = dpre * h_w, d h_w = dpre * h_x
 *   ignore_code         a_t = tanh(h_x) with either mix (prod + ignore_code == sum + ignore_code); code_layer.weight, code_layer.bias and
 *                       code_bias get exact ZERO gradients.  (The reference leaves their .grad None and its optimizers skip them; here
 *                       the update sees zeros: the parameters stay bit-identical, RMSprop's square average of the three tensors decays.)
 *   ignore_receiver     binary messages only (use_binary == 0: accepted, nothing happens).  The receiver's message is replaced by zeros
 *                       AFTER it was sampled (training) or rounded (evaluation); the uniform draw is still consumed, so no Philox stream
 *                       and no injected uniform shifts.  Everything downstream reads the zeros: the sender's code input of t > 0 (h_w =
 *                       code_layer.bias), baseline_sen's z_r, the tape arrays "w" / "zr", "lp_w" (= sum_j log(1 - pw_j + 1e-8)), the
 *                       REINFORCE seed of the receiver's message stream (q = 0) and mmg_eval_steps' Hamming counts; "pw" and "ne_w" stay
 *                       functions of the logits.
 * All three at their defaults clears the setting.  While it is set it holds for every forward entry (mmg_exchange_forward,
 * mmg_train_step[s], mmg_dp_train_step[s], mmg_eval_steps, mmg_sender_forward, mmg_receiver_forward), for the backward pass and for
 * mmg_exchange_vjp / mmg_sender_vjp; mmg_exchange_vjp_channel refuses such a handle.  No tensor changes shape: parameter buffer,
 * checkpoints and mmg_config stay as they are.
 * Kernels: a variant handle runs the generic per-sample family -- k_conversation -> baselines and statistics launches -> k_bwd_conv ->
 * k_wgrad -- in instantiations of their own (the backward one recomputes h_w of a step from the tape's code input); the register-resident,
 * many-class, sample-tile and wide-receiver kernels do not form the variants.  The call re-runs the kernel selection and does no other
 * GPU work; clearing restores the original selection.  A handle has message flips or a sender variant, not both (this bounds the
 * kernel instantiations): whichever setter comes second returns negative.
 * Returns 0, or negative: any other mix (-sender_mix mou needs a [W, 4H] binary layer and, with -ignore_code, one more parameter --
 * another parameter layout), or flips are set; the setting before stays. */
enum { MMG_MIX_SUM = 0, MMG_MIX_PROD = 1 };
int mmg_set_sender_variant(mmg_handle* h, int mix, int ignore_code, int ignore_receiver);

/* Relaxed messages: the Gumbel-sigmoid (binary concrete) channel with exact gradients, the differentiable-channel baseline next to
 * REINFORCE and to the plain straight-through estimator of mmg_exchange_vjp_channel.  Binary messages only; the reference has no
 * such option.  Per message element of a TRAINING conversation, with lz the logit, p = sigmoid(lz) and u the uniform draw the
 * Bernoulli sample of that element uses today (same Philox key, index, counter and stream, or the injected u_z / u_w):
 *   u'   = min(max(u, 2^-24), 1 - 2^-24)
 *   soft = sigmoid((lz + log(1 - u') - log(u')) / tau)      tau = tau_sen for the sender's z, tau_rec for the receiver's w
 *   bit  = (u < p) ? 1 : 0                                  exactly the unrelaxed compare (model.py:227 / 460)
 *   hard == 0:  message = soft
 *   hard == 1:  message = bit;  backward: message = soft + stopgrad(bit - soft)
 * The sign of the noise makes soft > 0.5 exactly when u < p, up to rounding: a hard relaxed conversation draws the very bits an
 * unrelaxed one draws from the same uniforms.  Everything downstream reads the message: the other agent, both baselines, the tape
 * arrays "z" / "w" / "zr".  "lp_z" / "lp_w" keep their formula applied to the message value -- with hard == 0 they are NO
 * log-likelihoods.  "pz", "pw", the entropy terms, the stop bit and the masks are unchanged, and so is every evaluation conversation
 * (train == 0 rounds the probabilities: a relaxed pair is deployed discrete).  The soft values go to two tape arrays of their own,
 * "zs" and "ws" [T, B, W], the last entries of mmg_tape_table; only a relaxed handle writes them.
 * Backward: mmg_exchange_vjp_channel only.  The gradient arriving at a message crosses into the logits as soft (1 - soft) / tau --
 * the exact derivative of what the forward pass computed --, upstream gradients on the probabilities keep p (1 - p):
 *   dlz_t = dz_up[t] pz (1 - pz) + (W_ih^T dgi_t)     zs (1 - zs) / tau_sen
 *   dlw_t = dw_up[t] pw (1 - pw) + (W_c^T dpre_{t+1}) ws (1 - ws) / tau_rec
 * with zs / ws read from the tape (never drawn again: injected uniform buffers may be gone).  The stop bits, softmax(y) inside dbar,
 * the baselines' inputs, data and desc stay constants; mmg_vjp_input_grads right behind it works unchanged.
 * While it is set: mmg_exchange_forward(train = 1), mmg_sender_forward and mmg_receiver_forward form relaxed messages;
 * mmg_exchange_forward(train = 0), mmg_eval_steps and mmg_loss_stats run as before; mmg_train_step[s], mmg_dp_train_step[s],
 * mmg_backward, mmg_exchange_vjp and the three per-call VJPs return negative with this entry's name in the message (REINFORCE seeds
 * and detached graphs are not what such a handle trains with).
 * Kernels: a relaxed handle runs the generic per-sample conversation in an instantiation of its own (k_conversation<NT, .., RELAX>;
 * the register-resident, many-class, sample-tile and wide-receiver conversations do not relax) and k_vjp_channel_relax.  Host only: the
 * kernel selection is re-run only when the relaxed STATE changes, so the call may precede every minibatch to anneal the temperatures.
 * tau_sen == 0 && tau_rec == 0 clears the setting and restores the original selection.
 * Returns 0, or negative (the setting before stays): a tau that is negative or NaN; exactly one tau being zero; use_binary == 0; a
 * handle with message flips or a sender variant (their setters refuse a relaxed handle likewise); an attention handle. */
int mmg_set_message_relaxation(mmg_handle* h, float tau_sen, float tau_rec, int hard);

/* Gaussian message noise: an additive white Gaussian noise channel for CONTINUOUS messages (use_binary == 0), the continuous twin of
 * mmg_set_message_flipout; the reference has no such option.  With lz_t / lw_t the logits the conversation forms today (in continuous
 * mode they are the messages), the sender's message of step t becomes z_t = lz_t + sigma_sen * n_z[t, b, j] and the receiver's
 * w_t = lw_t + sigma_rec * n_w[t, b, j], n standard normal.  The noisy value IS the message: the receiver's GRU, the sender's code
 * input of step t + 1, the tape arrays "z" / "w" / "zr", the backward pass, every VJP and mmg_eval_steps read it.  The constant
 * first_rec in front of step 0 is no message and takes no noise.  The noise is added where the message is formed; a mask of
 * mmg_set_message_corruption is applied after it (|z + sigma n - m|).  Training conversations always take the noise; evaluation
 * conversations only with noise_dev != 0.  A sigma of 0 leaves that message clean; both 0 clears the setting.
 * Draws: one Philox4x32-10 block per element, counter (e, c1, stream, 0), 64-bit key, as the Bernoulli draws build it; its first two
 * output words x0, x1 give u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1], u2 = (x1 >> 8) 2^-24 in [0, 1) and n = sqrt(-2 ln u1) cos(2 pi u2),
 * so |n| <= 5.77.  e = (t * B_global + batch_offset + b) * W + j is the element index of the Bernoulli draws: a data-parallel shard
 * draws what the single-GPU batch draws.
 *   training:   streams 7 (sender) / 8 (receiver), key = the call's seed, c1 = the minibatch counter of the Bernoulli draws -- also
 *               when d_u_z / d_u_s / d_u_w are injected;
 *   evaluation: streams 9 / 10, key = eval_seed, c1 = the number of evaluation conversations enqueued on this handle since this call
 *               (counted on the host; the device-side minibatch counter stays untouched).  The agent-level entries draw with the
 *               count of the conversation the last mmg_sender_forward(t = 0, train = 0) began.
 * Gradients: d z / d lz = 1, so every backward entry works unchanged on the tape's noisy messages -- the REINFORCE step (continuous
 * mode updates the receiver alone), mmg_exchange_vjp, mmg_exchange_vjp_channel (exact here, no surrogate: the gradient crosses the
 * channel unchanged), the per-call VJPs and mmg_vjp_input_grads.  mmg_dp_train_step[s], mmg_eval_steps, the corruption mask and the
 * training controls work on a noise handle.  A flip setting on the same (continuous) handle keeps doing nothing.
 * Kernels: a noise handle runs k_conversation_noise (the generic per-sample family: -> k_bwd_conv -> k_dC -> k_wgrad; the agent-level
 * entries too) or, for the small agents with many classes, k_conversation_mc3_noise with that family's backward; the register-resident,
 * pair (mc3p), sample-tile and wide-receiver conversations form no noise.  Host only: the kernel selection is re-run only when the
 * noisy STATE changes, so the call may precede every minibatch to anneal the sigmas; it resets the evaluation count.  Clearing
 * restores the original selection.
 * Returns 0, or negative (the setting before stays): a sigma that is negative, infinite or NaN; use_binary == 1
 * (mmg_set_message_flipout is the binary counterpart); an attention handle; a handle with a sender variant (mmg_set_sender_variant
 * refuses a noise handle likewise). */
int mmg_set_message_noise(mmg_handle* h, float sigma_sen, float sigma_rec, int noise_dev, uint64_t eval_seed);

/* Training controls of a live handle: which agents the REINFORCE step updates, and the values of the learning rate and of the entropy
 * weights (model.py:1307-1330 with optimizer.step() of a frozen agent not called; the reference has no such switches).  The calls
 * enqueue nothing and synchronise nothing, and the kernel family of the handle stays.  mmg_set_learning_rate and mmg_set_entropy change
 * host state alone.  mmg_set_trainable also re-plans k_wgrad for the new set of frozen agents (below): its job table, row splits, its
 * walk over the tiles, and whether the clip + optimizer step fits inside its launch (k_wgrad<true>) or runs as k_opt behind it -- the first
 * call for a set allocates pinned host memory for its table.  Each call takes effect at the next minibatch that is enqueued -- of
 * mmg_train_step[s], mmg_dp_train_step[s] and of the phased mmg_backward / mmg_clip_step, on plain, attention and visual-attention
 * handles alike -- and may come between the minibatches of a run.
 *   mmg_set_trainable: bit MMG_AGENT_* of mask set = that agent is updated; the default is all four.  Bits of agents the mode never
 *     trains (continuous messages: the sender and both baselines) are accepted and ignored; a mask without any trained agent is allowed
 *     (the step changes no parameter); bits outside the four are an error.  A frozen agent:
 *       - its parameters and its optimizer state (square_avg | exp_avg, exp_avg_sq) stay bit-identical, and the update neither reads nor
 *         writes them;
 *       - its slice of d_grads holds ZEROS behind mmg_backward and behind every training step (mmg_dp_train_step all-reduces the
 *         whole buffer): its weight-gradient jobs are not in the table k_wgrad runs -- one table per set of frozen agents, built at
 *         this call, kept, and uploaded on the stream of the next minibatch --, the launches that only feed them are not made, and
 *         the slice is cleared once;
 *       - the forward pass, the losses, the statistics, the logged values and the other agents' gradients and updates are what they
 *         are without the mask: a frozen baseline still scores, a frozen sender still speaks; the minibatch counter and the Philox
 *         stream advance as ever;
 *       - Adam's bias correction counts an agent's OWN updates, as four torch.optim.Adam objects would: tape "counter"[4 + a] holds the
 *         committed steps agent a sat out frozen, its step count is counter[1] - counter[4 + a].  With nothing ever frozen the four
 *         words stay zero and every count is the global one.
 *   mmg_set_learning_rate: finite lr >= 0, an error otherwise.
 *   mmg_set_entropy: new values for the weights the handle was created with (has_entropy_*).  A weight that was absent at mmg_create
 *     stays absent and its argument is ignored (the has_* flags never change); a non-finite value is an error.
 *   mmg_get_training_controls: the mask as set, the current learning rate and entropy3 = {entropy_s, entropy_sen, entropy_rec}; each
 *     pointer may be NULL.
 * Each returns 0, or negative (the settings before stay). */
int mmg_set_trainable(mmg_handle* h, int mask);
int mmg_set_learning_rate(mmg_handle* h, float lr);
int mmg_set_entropy(mmg_handle* h, float entropy_s, float entropy_sen, float entropy_rec);
int mmg_get_training_controls(const mmg_handle* h, int* mask, float* lr, float* entropy3);

/* Description attention, the reference's -desc_attn (model.py:267-271, 344-410, 444-445): the receiver's class description is no
 * fixed bag-of-words mean but, per sample and step, an attention over the WORDS of each description with the GRU state as the query.
 * With set [n_words, V] = the word vectors of all classes concatenated (a word without a vector is a row of zeros and is still
 * attended over), lens[D] > 0 the words per class, A = attn_dim and h = h_z after the GRU update:
 *   score[b, j] = d_attn(tanh(d_d(set[j]) + d_h(h[b])));   alpha = softmax of score inside each class's segment
 *   wdesc[b, d] = sum_{j in d} alpha[b, j] set[j];         y[b, d] = y2(relu(y1([wdesc[b, d] || h[b]])))   -- the description FIRST:
 *                 y1.weight[:, :V] multiplies the description and y1.weight[:, V:] the state, the opposite of the plain receiver
 *   dbar[b]     = sum_d softmax(y)[b, d].detach() wdesc[b, d]: alpha keeps its graph there, so the receiver's message stream trains
 *                 d_d / d_h / d_attn and h at every step before the output step, the class logits at the output step
 * desc [D, V] is still an argument of every entry and is NOT read by an attention receiver.
 * The twins below take (cfg, attn_dim, n_words); with attn_dim == 0 each returns exactly what its plain twin returns.  attn_dim > 0:
 *   - six more receiver tensors under the reference's state_dict names, BEHIND its fifteen and inside its contiguous range (clip norm,
 *     optimizer state and checkpoints cover them like the others; the other agents' tensors move up): d_d.weight [A, V], d_d.bias [A],
 *     d_h.weight [A, R], d_h.bias [A], d_attn.weight [1, A], d_attn.bias [1].  d_attn.bias shifts every score of a softmax segment
 *     alike: its gradient is EXACTLY zero here (the reference's autograd leaves rounding noise there, which RMSprop turns into steps
 *     of the size of the learning rate) -- it stays bit-identical under every optimizer;
 *   - more workspace arrays behind the plain ones, among them "alpha" [T, B, n_words];
 *   - supported: attn_dim 1..128, n_classes <= n_words <= 2048, n_classes <= 128, batch <= 512, one GPU (global_batch == batch);
 *     anything else is an error.
 * mmg_set_desc_set uploads the set (d_set: DEVICE memory, copied into the workspace) and the segment table (lens: HOST memory, D
 * entries, each > 0, summing to n_words == the handle's); a blocking call, required before the first conversation, repeatable.  The
 * per-word tables (set . d_d.weight^T + d_d.bias, set . y1.weight[:, :V]^T, set . w_d.weight^T) are rebuilt from the current
 * parameters by every forward entry, like the per-class tables of the plain receiver.
 * Kernels: the generic per-sample family in instantiations of its own -- k_attn_prep -> k_conversation_attn -> baselines and
 * statistics launches -> k_bwd_conv_attn -> k_attn_dE, k_attn_dDD -> k_wgrad -- for training, evaluation and the agent-level entry
 * alike; no entry runs the plain receiver on such a handle.  Not offered, each an error: mmg_set_message_flipout /
 * mmg_set_sender_variant with anything set, mmg_dp_train_step[s], mmg_exchange_vjp[_channel], mmg_vjp_input_grads and the per-call
 * VJPs. */
int64_t mmg_attn_param_count(const mmg_config* cfg, int attn_dim, int n_words);
int64_t mmg_attn_grad_floats(const mmg_config* cfg, int attn_dim, int n_words);
int     mmg_attn_param_table(const mmg_config* cfg, int attn_dim, int n_words, mmg_param_entry* out, int max_entries);
int64_t mmg_attn_workspace_bytes(const mmg_config* cfg, int attn_dim, int n_words);
int     mmg_attn_tape_table(const mmg_config* cfg, int attn_dim, int n_words, mmg_tape_entry* out, int max_entries);
mmg_handle* mmg_attn_create(const mmg_config* cfg, int attn_dim, int n_words, void* d_workspace, int64_t workspace_bytes,
                            float* d_params, float* d_grads, float* d_opt_state);
int     mmg_set_desc_set(mmg_handle* h, const float* d_set, const int32_t* lens, int n_words);

/* Visual attention, the reference's -visual_attn / -attn_extra_context (model.py:80-86, 114-142, 168-195): the SENDER attends over the
 * N = h * w locations of a feature map with the receiver's last message as the query.  On such a handle x of every entry is the map
 * [B, C, N] as the caller holds it -- C == feat_dim channels, the locations contiguous (the reference's x.view(B, C, N).transpose(1, 2)
 * is a view) -- read in place, never transposed.  With A = attn_dim, X[b, i] = x[b, :, i], g [B, G] the optional context:
 *   per conversation: HX[b, i] = attn_W_x(X[b, i]);  HG[b] = attn_W_g(g[b])                               (cached by the reference)
 *   step 0:           alpha = 1 / N (the scores are computed and dropped)
 *   step t >= 1:      beta[b, i] = attn_U(tanh(attn_W_w(w_{t-1}[b]) + HX[b, i] (+ HG[b])));  alpha = softmax_i beta
 *   every step:       x_attn = sum_i alpha[b, i] X[b, i];  h_x = image_layer(x_attn) -- h_x is per STEP, and baseline_sen reads the step's
 * The twins below take (cfg, attn_dim, n_feats, context_dim); with attn_dim == 0 each returns exactly what its plain twin returns.
 * attn_dim > 0:
 *   - six more sender tensors under the reference's state_dict names, BEHIND its seven and inside its contiguous range (the other
 *     agents' tensors move up): attn_W_x.weight [A, C], attn_W_x.bias [A], attn_W_w.weight [A, W], attn_W_w.bias [A], attn_U.weight
 *     [1, A], attn_U.bias [1]; with context_dim = G > 0 two more: attn_W_g.weight [A, G], attn_W_g.bias [A];
 *     attn_U.bias shifts every score of a softmax alike: its gradient is EXACTLY zero here (the reference's autograd leaves rounding
 *     noise there, which RMSprop turns into steps of the size of the learning rate) -- it stays bit-identical under every optimizer;
 *     the three other biases add into one pre-activation and get one gradient, bit for bit;
 *   - more workspace arrays behind the plain ones: "vattn_HX" [B, N, A], "vattn_HG" [B, A], "vattn_alpha" [T, B, N], "vattn_xa"
 *     [T, B, C] (x_attn), "vattn_hx" [T, B, H] (the step's h_x; "hx" is not written), the reverse pass's "vattn_dq" / "vattn_dv"
 *     [T, B, A] and "vattn_dHX" [B, N, A]; nothing of size T B N C or T B N A exists;
 *   - supported: attn_dim 1..256, n_feats 1..256, feat_dim <= 4096, context_dim 0..4096, batch <= 512, batch * n_feats * attn_dim <= 2^25, one GPU
 *     (global_batch == batch); anything else is an error.
 * mmg_set_data_context states the context (DEVICE memory [B, G], or [n * B, G] for mmg_eval_steps, which advances through it as it
 * advances through d_x -- by B * C * N floats per batch there -- and so does mmg_train_steps); it is read in place by every later forward entry, so it must stay valid;
 * required before a conversation iff context_dim > 0.  Host state only.
 * Kernels: k_vattn_prep (HX on the matrix cores with a K-major A operand, HG) -> k_conversation_vattn, the generic per-sample
 * conversation compiled once more -> k_baselines over the per-step h_x -> statistics -> k_bwd_conv (it leaves dh_x of every step) ->
 * k_vattn_bwd (per sample: dx_attn, dalpha, dbeta, the tapes dq / dv, dHX summed over the steps in order) -> k_vattn_dwx
 * (attn_W_x.weight = dHX^T X, X channel-major) -> k_wgrad (the other tensors; image_layer from the per-step x_attn, baseline_sen from the
 * per-step h_x) -> k_gradnorm + k_opt.  Fixed-order reductions, no float atomics.  Served: mmg_exchange_forward (train = 0 / 1, every
 * tape mode), mmg_eval_steps, mmg_loss_stats, mmg_backward, mmg_clip_step, mmg_train_step[s], mmg_sender_forward (HX / HG are formed
 * by the first call after mmg_vattn_reset_state and kept), mmg_receiver_forward, mmg_baseline_forward.  Not offered, each an error:
 * mmg_set_message_flipout / mmg_set_sender_variant with anything set, description attention together with it, mmg_dp_train_step[s],
 * mmg_exchange_vjp[_channel], mmg_vjp_input_grads and the per-call VJPs.  No entry runs the plain sender on such a handle. */
int64_t mmg_vattn_param_count(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim);
int64_t mmg_vattn_grad_floats(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim);
int     mmg_vattn_param_table(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, mmg_param_entry* out, int max_entries);
int64_t mmg_vattn_workspace_bytes(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim);
int     mmg_vattn_tape_table(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, mmg_tape_entry* out, int max_entries);
mmg_handle* mmg_vattn_create(const mmg_config* cfg, int attn_dim, int n_feats, int context_dim, void* d_workspace, int64_t workspace_bytes,
                             float* d_params, float* d_grads, float* d_opt_state);
int     mmg_set_data_context(mmg_handle* h, const float* d_context);
/* Sender.reset_state() (model.py:99-112) for mmg_sender_forward: the next call forms HX / HG from its x, the context and the current
 * parameters, whatever its t; later calls reuse them.  A new handle, and a handle on which a whole conversation ran, is in that state. */
int     mmg_vattn_reset_state(mmg_handle* h);

/* Dev evaluation inside the library (eval_dev's loop body, model.py:620-691): n consecutive evaluation conversations, each
 * followed on the same stream by ONE reduction launch (k_eval_reduce) that leaves what the reference computes per dev batch
 * on the host -- as integers, so the results do not depend on any summation order and are bit-reproducible.
 *   d_x [n * B, F] f32, d_target [n * B] i64: batch i reads rows [i * B, (i + 1) * B), as mmg_train_steps lays them out.
 *   Each conversation is mmg_exchange_forward(train = 0, run_all_steps = 1): rounded messages, no Philox draw, the minibatch
 *   counter is not touched (a training call afterwards draws what it would have drawn without the evaluation); a mask set by
 *   mmg_set_message_corruption applies.  The tape of the LAST batch stays valid (the dev sample dump reads it, model.py:1463-1518).
 *   top_k: -top_k_dev (model.py:657-658).
 * Step count of a batch (model.py:866): n_b = the first t + 1 with sum_b mask[t + 1, b] == 0, else T; Fixed mode: T.  Output step
 * of a sample (model.py:870, 1261, 879-904): tsel[b] = #{t in 1..n_b - 1 : mask[t, b] = 1}; Fixed mode: T - 1.  With
 * y = the class logits of that step: hit iff #{d : y[d] > y[target]} < min(top_k, D) (model.py:657-668: membership in the
 * top_k of the log-softmax, which is monotone in y); prediction = argmax y, lowest index on ties (model.py:700).
 *   d_acc: mmg_eval_acc_count() int64, ZEROED BY THE CALLER before the first batch of an evaluation and added to atomically:
 *     [0] hits | [1] batches added | [2] samples added | [3] 0 |
 *     [4, 4 + D * D) confusion counts conf[target * D + prediction] (model.py:709) |
 *     [4 + D * D, 4 + D * D + D) seen[c] = times class c occurred as target or as prediction (sklearn's confusion_matrix keeps
 *     the classes that occur).
 *     Handles of different batch sizes (the short final dev batch) may share one accumulator.  A target outside [0, D) counts as
 *     a sample only.
 *   d_len [n * B] i32, written: conversation length sum_{t < n_b} s[t, b] of every sample, in dataset order (model.py:671-672).
 *   d_batch [n, 1 + 2 T] i64, written, per batch: [0] n_b | [1 + t] ham_sen[t] = sum_b sum_j |z[t, b, j] - z[t - 1, b, j]| with
 *     z[-1] = 0 | [1 + T + t] ham_rec[t], the same over the receiver's messages w -- for EVERY t < T; the reference's statistic of
 *     the batch is sum_{t < n_b} ham[t] / (B n_b) (model.py:675-691), formed by the caller in float64.  Binary messages: int64
 *     counts.  Continuous messages (use_binary == 0): the int64 slot holds the bits of the float64 sum, reduced in a fixed
 *     order by the one workgroup that owns the slot (per-thread partial sums in index order, a fixed tree over the workgroup;
 *     there is one slot per batch and step, so no second pass over slots): bit-identical from run to run.
 * No host synchronisation; returns 0, or negative for a NULL pointer, top_k < 1 or n < 0. */
int64_t mmg_eval_acc_count(const mmg_config* cfg);
int mmg_eval_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                   int64_t* d_acc, int32_t* d_len, int64_t* d_batch, void* stream);

/* The communication profile of a dev evaluation: mmg_eval_steps with the same arguments and the same results in d_acc / d_len /
 * d_batch, plus ONE more reduction launch per batch (k_eval_profile, behind k_eval_reduce on the same stream) that adds integer
 * counts to d_prof.  It stands for the reference's -binary_only dump (binary_vectors.py:24-46: per sample and step the rank of the
 * target, :92-99, the stop bit and mask, :129-132, and both agents' messages, :101-126) and for what is derived from that file:
 * accuracy against conversation length, conversation length per class, per-class message codes.  The conversations are those of
 * mmg_eval_steps (model.py:620-640: train = 0, every sample runs all steps), so a corruption mask, flipout_dev flips and noise_dev
 * noise are counted as the receiver saw them.
 * Per sample b, with n_b and tsel[b] as above and c = d_target[b]: the sample is LIVE at step t iff t <= tsel[b], and
 *   rank_t[b] = #{d : y[min(t, tsel[b]), b, d] > y[min(t, tsel[b]), b, c]},  t = 0 .. T - 1
 * -- the rank of the target had every conversation been cut after t + 1 steps (a sample that stopped earlier keeps its own
 * answer); strict > on the fp32 logits, so rank_{T-1} is the rank mmg_eval_steps' hit is formed from.
 *   d_prof: mmg_eval_profile_count() = 4 + 2 D T + 2 D + 2 T D W int64, ZEROED BY THE CALLER before the first batch of an evaluation
 *   and added to atomically (integers only: bit-reproducible); handles of different batch sizes may share one.  In this order:
 *     head [4]            [0] batches added | [1] samples with a valid target | [2] samples with a target outside [0, D) | [3] 0
 *     steps [D, T]        samples of class c whose output step is l
 *     rank [T, D]         samples with rank_t[b] = r
 *     class_hits [D]      samples of class c with rank_{T-1}[b] < min(top_k, D)
 *     class_ranksum [D]   sum over the samples of class c of rank_{T-1}[b]
 *     msg_sen [T, D, W]   samples of class c, live at t, with lrintf(z[t, b, j]) == 1 (the sender's messages)
 *     msg_rec [T, D, W]   the same over the receiver's messages w
 *   A target outside [0, D) counts in head[2] only.  msg_sen / msg_rec are the per-class code book; their denominator, the samples
 *   of class c that are live at t, is sum_{l >= t} steps[c, l].  Continuous messages (use_binary == 0): both message blocks are
 *   left untouched.
 * No host synchronisation, the minibatch counter is not touched, the tape of the last batch stays valid.  Returns 0, or negative
 * for what mmg_eval_steps refuses and for d_prof == NULL (mmg_eval_steps is the entry without a profile).
 * mmg_eval_profile_count: host only; negative for a config the library refuses. */
int64_t mmg_eval_profile_count(const mmg_config* cfg);
int mmg_eval_steps_profile(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                           int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof, void* stream);

/* Every sample's own code of a dev evaluation: mmg_eval_steps (d_prof == NULL) or mmg_eval_steps_profile (d_prof != NULL) with the
 * same arguments and the same results in d_acc / d_len / d_batch / d_prof, plus ONE more launch per batch (k_eval_codes, behind
 * k_eval_reduce and k_eval_profile on the same stream) that WRITES -- nothing is accumulated -- the bits of both agents' messages,
 * packed 32 to a word: what the reference's -binary_only dump stores per sample and step (binary_vectors.py:101-126: the
 * "BinaryVec" field of the agent "S" and agent "R" records).  The per-class sums of the profile cannot answer questions about PAIRS of samples (mmg_code_pair_hist below); these
 * can.  The kernel reads the plain tape (mask, z, w) and the targets only: it serves every handle kind, and a corruption mask or
 * flipout_dev flips are packed as the receiver saw them.  Binary messages only.
 * Per sample b of batch i, at row = row0 + i * B + b (so handles of several batch sizes -- the short final dev batch -- fill one
 * caller-owned buffer in dataset order), with n_b and tsel[b] as above, Wp = (W + 31) / 32:
 *   d_codes[row][agent][t][k] uint32, agent 0 = the sender's z, 1 = the receiver's w, t < T, k < Wp: bit (j & 31) of word (j >> 5)
 *     is set iff lrintf(msg[t, b, j]) == 1 and t <= tsel[b].  The steps behind the output step and the padding bits of the last
 *     word are zero; every word of the row is written, so the buffer need not be zeroed.  mmg_eval_code_words() = 2 T Wp per row.
 *   d_meta[row][2] int32: tsel[b] | d_target[b], or -1 for a target outside [0, D).
 * No host synchronisation, the minibatch counter is not touched, the tape of the last batch stays valid.  Returns 0, or negative
 * for what mmg_eval_steps refuses, a handle with continuous messages (use_binary == 0: there are no bits), d_codes or d_meta NULL,
 * row0 < 0 and row0 + n * B > cap_rows (the rows the two buffers hold).
 * mmg_eval_code_words: host only; negative for a config the library refuses and for continuous messages. */
int64_t mmg_eval_code_words(const mmg_config* cfg);
int mmg_eval_steps_codes(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc, int top_k,
                         int64_t* d_acc, int32_t* d_len, int64_t* d_batch, int64_t* d_prof /* may be NULL */,
                         uint32_t* d_codes, int32_t* d_meta, int64_t row0, int64_t cap_rows, void* stream);

/* The pair histogram of a set of codes: for every unordered pair i < j of the rows with a valid target, the Hamming distance of
 * the two codes against the cosine distance of the two rows of a "meaning" matrix, split by whether the two rows share a class.
 * From it the host forms topographic similarity (the rank correlation of the two distances over all pairs), class separation and
 * the count of code collisions (multimodalgame_amd/commstats.py: topsim) -- the second-order analysis the -binary_only dump
 * (binary_vectors.py:24-46) is collected for, O(n_rows^2), on the device.  Handle-free, on the calling thread's current device.
 *   d_codes [n_rows][2][T][Wp], d_meta [n_rows][2]: as mmg_eval_steps_codes leaves them (padding bits zero).  agent: 0 the sender's
 *   codes, 1 the receiver's; the steps t0 <= t < t1 are compared.  M = (t1 - t0) * W, K = n_bins.
 *   d_meaning [n_rows, F] f32 with row stride ld >= F (floats): ANY matrix -- the image features give the image-level measure,
 *   desc[target] the class-level one.  Its entries must be FINITE: that is the caller's duty (a NaN distance is counted in bin 0).
 *   d_inv [n_rows] f32: work space; left holding inv[i] = 1 / sqrt(sum_k x_ik^2) in fp32, 0 for a zero row.
 *   d_hist: mmg_code_pair_hist_count() = 4 + 2 (M + 1) K int64, ZEROED BY THE CALLER, integers only are added (bit-reproducible):
 *     head [4]                  [0] rows used | [1] rows skipped (meta target -1) | [2] pairs counted = used (used - 1) / 2 | [3] 0
 *     hist [2][M + 1][K]        hist[p][h][q] = pairs with p = (target_i == target_j),
 *                               h = sum_{t0 <= t < t1} sum_k popc(code_i[agent][t][k] ^ code_j[agent][t][k]), and q the bin of
 *                               c = dot(x_i, x_j) * (inv_i * inv_j),  u = (1.f - c) * (0.5f * K),  q = min(K - 1, max(0, (int)floorf(u)))
 *                               in fp32: identical rows (c = 1 +- ulp) fall into bin 0, opposite rows (u = K) into bin K - 1, a zero
 *                               row has c = 0.
 *   Calls on disjoint row sets may add into one histogram (their heads add up too).
 * Returns 0, or negative with a message for: a NULL pointer; n_rows outside 1..65536; F outside 1..4096; ld < F; n_bins outside
 * 1..1024; agent not 0 or 1; T or W < 1; not 0 <= t0 < t1 <= T; 2 (M + 1) K > 2^24.  No host synchronisation.
 * mmg_code_pair_hist_count: host only; M = n_sel_steps * w_dim; negative for the same shape refusals. */
int64_t mmg_code_pair_hist_count(int n_sel_steps, int w_dim, int n_bins);
int mmg_code_pair_hist(const uint32_t* d_codes, const int32_t* d_meta, int64_t n_rows, int T, int W,
                       int agent, int t0, int t1, const float* d_meaning, int F, int64_t ld,
                       float* d_inv /* [n_rows] work */, int n_bins, int64_t* d_hist, void* stream);

/* Per-rank partial sums of every batch statistic the losses need (counts, sums and squared sums
 * of reward-minus-baseline per stream and step, ...) into the f64 tape array "stats".  With more
 * than one rank the caller all-reduces (sum) that array between this call and mmg_backward
 * (model.py:912-915, 947-961: the REINFORCE weights are normalised by statistics of the WHOLE minibatch).
 * Continuous mode (use_binary == 0; model.py:1297-1305: loss = NLL mean) has no such coupling: the call and the
 * all-reduce may be skipped, mmg_backward forms the two logged sums itself (see mmg_grad_floats).
 * Binary mode: the call is REQUIRED between mmg_exchange_forward(train, run_all_steps != 1) and mmg_backward -- on the
 * register-resident path it also carries the baselines' forward pass over the live rows (model.py:835-843; one launch for the
 * baselines and the statistics that consume their scores); mmg_backward fails if it was skipped. */
int mmg_loss_stats(mmg_handle* h, void* stream);

/* Gradient of the four losses (model.py:1296-1305) w.r.t. all parameters into d_grads (the whole
 * flat buffer is overwritten).  Also writes the six loss scalars into the tape array "losses". */
int mmg_backward(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc, void* stream);

/* Per-agent clip_grad_norm(max_norm=1) + optimizer update on the flat buffers.  In continuous mode
 * (use_binary==0) only the receiver is updated (model.py:1313).  Skips the update when the dependency-error flag of this
 * rank or -- through the tail quad of d_grads -- of any rank is set; the next call that starts a minibatch recovers
 * (mmg_clear_error).
 * Non-finite guard: when the gradient norm of ANY agent is not finite, tape "losses"[0] (the NLL) is set to NaN in the same
 * step.  (The class-logit ReLU is v_max_f32, which reads a NaN pre-activation as "unit off" where torch's relu propagates
 * it: without the guard a NaN in receiver.y1.weight[:, :R] or in the GRU leaves a plausible NLL = log D while every loss of
 * the reference is NaN.  The reference's NLL is non-finite => this one is, in the same step; it is finite whenever all six
 * losses of the reference are.) */
int mmg_clip_step(mmg_handle* h, void* stream);

/* forward(train, run_all_steps = 2) + stats + backward + clip_step for a single-GPU minibatch; nothing returns to the
 * host.  Equivalent to the four calls above in sequence.  Launches per minibatch depend on the shape: 2 for the agents of
 * BASELINE configs 1-2 (k_game_fast: conversation, k_prep's blocks, baselines, statistics and the reverse pass as roles of
 * one launch; k_wgrad<OPT>: weight gradients + clip + optimizer), 4 for config 3's shard (k_conversation_fast3, k_baselines3,
 * k_bwd_conv_fast, k_wgrad<OPT>; + k_prep with more samples than CUs, + k_opt with row splits), 6 for config 5's
 * shard (k_prep, k_conversation_mc, k_bwd_mc1, k_bwd_mc2, k_wgrad, k_opt), 9 for config 4 (k_prep,
 * k_conv_persist, k_baselines4, k_stats, k_bwd_pre_send, k_bwd_sample, k_dC_tile, k_wgrad, k_opt), 10 for
 * config 4 with rec_hidden 256 (k_prep, k_rc_persist, k_gemm_nt, k_baselines4, k_stats, k_bwd_pre_send, k_rc_bwd, k_dC_tile,
 * k_wgrad, k_opt). */
int mmg_train_step(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                   const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed, void* stream);

/* n consecutive minibatches of the epoch loop (model.py:1218-1240) enqueued by ONE call: minibatch i reads rows
 * [i * B, (i + 1) * B) of d_x [n * B, F] / d_target [n * B] -- the epoch's samples laid out in the reference's batch order
 * (misc.py:257-302: random.seed(11 + epoch) shuffle, consecutive slices, indices sorted inside a batch), which the caller
 * gathers once per epoch.  Philox sampling only (the device-side minibatch counter advances as under n mmg_train_step
 * calls: bit-identical results).  The caller runs the minibatches that write a log block / evaluate / checkpoint itself. */
int mmg_train_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc,
                    uint64_t seed, void* stream);

/* Data-parallel minibatch in ONE call (one rank; batch < global_batch): forward + mmg_loss_stats | all-reduce(sum) of the
 * f64 "stats" array (binary messages only) | mmg_backward | ONE all-reduce of all mmg_grad_floats() floats of d_grads |
 * mmg_clip_step on the reduced gradient.  The collectives are RCCL's
 *     ncclAllReduce(sendbuff, recvbuff, count, datatype, op, comm, stream)
 * called through the ADDRESS the caller registers (libmmg does not link RCCL) on the caller's communicator, in place, on
 * `stream`.  reduce == 0 skips both (a one-rank job).  full_tape != 0: every sample runs all steps (run_all_steps = 3: the
 * minibatches whose log block reads the whole tape; baseline scores on the live rows only), same update.  mmg_dp_train_steps: n minibatches laid out as for
 * mmg_train_steps (this rank's B rows of each).
 * Continuous messages with Adaptive stopping: losses[6] (executed steps) and the running totals are formed from THIS rank's samples
 * -- max_b t* + 1 steps, sum_b (t* + 1) sample-steps -- because only sums travel to the other ranks; on one GPU they are the
 * reference's (model.py:866).  Continuous messages with Fixed exchange: max_exchange steps and max_exchange * global_batch sample-steps on every rank. */
int mmg_dp_set_allreduce(mmg_handle* h, void* nccl_all_reduce, void* comm);
int mmg_dp_train_step(mmg_handle* h, const float* d_x, const int64_t* d_target, const float* d_desc,
                      const float* d_u_z, const float* d_u_s, const float* d_u_w, uint64_t seed,
                      int full_tape, int reduce, void* stream);
int mmg_dp_train_steps(mmg_handle* h, const float* d_x, const int64_t* d_target, int64_t n, const float* d_desc,
                       uint64_t seed, int reduce, void* stream);

/* Fail-soft.  The persistent launches hold workgroup "roles" that wait on each other inside one launch; every wait is
 * bounded.  A wait that expires (fewer compute units than mmg_create assumed: shared or CU-masked GPU) makes that minibatch's
 * optimizer update a no-op on every rank, and the NEXT call that starts a minibatch (mmg_train_step[s],
 * mmg_exchange_forward(train), mmg_dp_train_step[s]) recovers by itself: it drains `stream`, clears the error words,
 * re-selects the kernels WITHOUT in-launch waits for the rest of the handle's life (what MMG_NO_ROLES=1, a CU mask in the
 * environment or a too-small cu_budget select up front), and returns 1 with the warning in mmg_last_error().  The reference
 * has no such failure mode (model.py:1218-1330 keeps training) -- neither has the caller of this library.
 *   mmg_clear_error: the same clearing on request, without changing the selected kernels (drains `stream`).
 *   mmg_degraded:    0 = role launches in use, 1 = launches without in-launch waits selected at mmg_create,
 *                    2 = ... selected by a recovery. */
int mmg_clear_error(mmg_handle* h, void* stream);
int mmg_degraded(const mmg_handle* h);

/* What the kernel selection decided (host only, additive).  The selection is a pure function of the config, the MMG_* / CU-mask
 * environment switches, two handle flags and the "caps": MMG_PLAN_CAPS int32 values the device reports -- the CU count (after
 * cu_budget) and, per role kernel, the workgroups of it one CU holds (0: the query failed, -1: not asked for this shape):
 * k_conv_split | k_conv_persist (the variant the shape uses) | k_rc_bwd | k_rc_persist | k_conversation_mc | _mc3 | _mc3p |
 * k_game_fast | k_wgrad with the optimizer inside | k_wgrad.
 *   mmg_plan_text: the selection of this handle as text: five lines of decisions (family and k_wgrad's plan; capabilities, LDS
 *                  sizes and budgets; the sample tiles' forward; many-class / register-resident forward and baselines; backward),
 *                  then one line with the caps it probed, in MMG_CAP_* order.
 *   mmg_plan_for:  the same text for a config and caller-supplied caps (n_caps == MMG_PLAN_CAPS), under the environment of the
 *                  call: no handle, no buffers, no GPU.  flags: bit 0 = no in-launch waits (what MMG_NO_ROLES=1 or a recovery
 *                  selects), bit 1 = message flips are set, bit 2 = a sender variant is set, bit 3 = messages are relaxed, bits 4-7 = bit 4 + MMG_AGENT_* set: that agent is frozen (mmg_set_trainable; its jobs leave k_wgrad's table: "gemm tiles", "blocks"), bit 8 = Gaussian message noise is set (the text then has one more line, in front of the caps).  cfg->cu_budget lowers caps[MMG_CAP_N_CU] as it lowers the device's.
 * Both return 0, or negative (out too small: about 2 KB are needed; a config the library refuses). */
enum { MMG_CAP_N_CU = 0, MMG_CAP_SPLIT, MMG_CAP_PERSIST, MMG_CAP_RC_BWD, MMG_CAP_RC_PERSIST, MMG_CAP_MC, MMG_CAP_MC3, MMG_CAP_MC3P,
       MMG_CAP_GAME, MMG_CAP_WGRAD_OPT, MMG_CAP_WGRAD, MMG_PLAN_CAPS };
int mmg_plan_text(const mmg_handle* h, char* out, int out_bytes);
int mmg_plan_for(const mmg_config* cfg, const int32_t* caps, int n_caps, int flags, char* out, int out_bytes);

/* The window arithmetic of k_game_fast's baseline roles (host only, additive; for tests).  The live rows of a minibatch are cut
 * into windows of 16; window w is the (w / nslots)-th window of slot w % nslots.  The kernel takes both from a reciprocal of
 * nslots (1..64) instead of dividing; these run the kernel's own inline functions over a range:
 *   mmg_game_window_split:  kw[w] = w / nslots and slot[w] = w % nslots as the kernel forms them, w = 0 .. n - 1;
 *   mmg_game_window_counts: count[nw] = windows of `slot` in a minibatch of nw windows, nw = 0 .. n - 1.
 * n <= 64 * nslots + 1.  Both return 0, or negative (an argument out of range). */
int mmg_game_window_split(int nslots, int n, int32_t* kw, int32_t* slot);
int mmg_game_window_counts(int nslots, int slot, int n, int32_t* count);

/* Agent-level entry points (one exchange step), mirroring the reference modules.  Forward only: their backward pass is
 * mmg_sender_vjp / mmg_receiver_vjp / mmg_baseline_vjp below, from the caller's copies of the call's inputs and outputs.
 *   sender:   x[B,F], w[B,W] (ignored when t==0), t -> message[B,W], probs[B,W] (NULL if continuous),
 *             h_x[B,H]                                                   model.py:193-238
 *   receiver: z[B,W], desc[D,V], h_z[B,R] in/out (zeros for a fresh conversation), s_prob_prod[B]
 *             in/out (eval; `first` != 0 restarts the product) -> s[B], s_prob[B], w[B,W],
 *             w_probs[B,W], y[B,D], h_w[B,R]                             model.py:333-342, 411-477
 *   baseline: which = MMG_AGENT_BASELINE_REC/SEN; x[B,x_dim] or NULL, binary[B,W], inp[B,R] or NULL
 *             -> score[B]                                                model.py:496-516
 * Uniform pointers as in mmg_exchange_forward (NULL + train==1 -> Philox with `seed`, step t). */
int mmg_sender_forward(mmg_handle* h, const float* d_x, const float* d_w, int t, int train,
                       const float* d_u_z, uint64_t seed,
                       float* d_message, float* d_probs, float* d_h_x, void* stream);
int mmg_receiver_forward(mmg_handle* h, const float* d_z, const float* d_desc, float* d_h_z,
                         float* d_s_prob_prod, int first, int t, int train,
                         const float* d_u_s, const float* d_u_w, uint64_t seed,
                         float* d_s, float* d_s_prob, float* d_w, float* d_w_probs, float* d_y,
                         float* d_h_w, void* stream);
int mmg_baseline_forward(mmg_handle* h, int which, const float* d_x, const float* d_binary,
                         const float* d_inp, int rows, float* d_score, void* stream);

/* Vector-Jacobian product of ONE agent's graph of the last training exchange: the backward pass autograd runs for
 * loss.backward() at model.py:1309 (receiver), 1316 (sender), 1322 (baseline_rec), 1328 (baseline_sen), but for ANY loss -- the
 * caller hands in d loss / d output of the agent's differentiable outputs.  The four graphs are disjoint as in the reference
 * (every input crossing between agents is detached, model.py:807-811, 826-829, 835-843), so each call is independent.
 * Reads the tape of mmg_exchange_forward(train = 1, run_all_steps = 1) -- the caller makes sure nothing rewrote it since -- and
 * writes ONLY `agent`'s slice of the gradient buffer (every tensor of the agent, overwritten, not accumulated).
 *   agent:   MMG_AGENT_*; the baselines exist with binary messages only
 *   n_steps: executed steps n (1..max_exchange); every upstream array holds n rows [n, B, .]; steps >= n get zero gradient
 *   d_x[B,F] (sender), d_desc[D,V] (receiver): the inputs of that forward call
 *   upstream gradients, each NULL = zero:
 *     d_dy[n,B,D]   receiver: class logits y_t                                      model.py:433
 *     d_dz[n,B,W]   sender:   sen_probs_t (binary) | sen_feats_t = logits (continuous) model.py:223, 238
 *     d_dw[n,B,W]   receiver: rec_probs_t (binary) | rec_feats_t = logits (continuous) model.py:456, 474
 *     d_dps[n,B]    receiver: s_probs_t                                              model.py:414-415
 *     d_dbs[n,B]    baseline_sen scores bs_t                                         model.py:835
 *     d_dbr[n,B]    baseline_rec scores br_t                                         model.py:842
 * Not differentiated (constants, as in the reference): sampled bits, masks, data, desc, h_x, h_z and softmax(y) inside dbar
 * (model.py:441).  The gradients of data and desc are formed on request by mmg_vjp_input_grads, called right after.  fp32,
 * deterministic (no float atomics); enqueued on `stream`. */
int mmg_exchange_vjp(mmg_handle* h, int agent, int n_steps, const float* d_x, const float* d_desc, const float* d_dy,
                     const float* d_dz, const float* d_dw, const float* d_dps, const float* d_dbs, const float* d_dbr,
                     void* stream);

/* Vector-Jacobian product of the sender's and the receiver's graphs of the last training exchange as ONE graph: the messages
 * crossing between the two agents are NOT detached.  This departs from the reference on purpose (model.py:807-811 hands the
 * receiver z.data, model.py:826-829 hands the sender w.data): it is the differentiable-channel baseline next to REINFORCE.
 *   continuous messages (use_binary == 0): the receiver reads the sender's logits z_t and the sender's step t + 1 reads the
 *     receiver's logits w_t with their graph -- the exact gradient;
 *   binary messages: the straight-through estimator, z_t = pz_t + stopgrad(bits_t - pz_t), w_t = pw_t + stopgrad(bits_t - pw_t):
 *     the forward values are the sampled bits of the tape, the backward pass treats d z_t / d pz_t and d w_t / d pw_t as 1.
 * One reverse-time launch runs both agents' steps (kernels_vjp.h: k_vjp_channel); the gradient of the receiver's GRU input flows
 * into the sender's step t, the gradient of the sender's code input into the receiver's step t - 1 (t = 0: code_bias).
 * Arguments as mmg_exchange_vjp (same tape, NULL upstream = zero, 1 <= n_steps <= max_exchange; d_x and d_desc must not be
 * NULL); writes ONLY the receiver's and the sender's slices of the gradient buffer (overwritten, not accumulated).  Constants as
 * before: the stop bits and masks, softmax(y) inside dbar, data, desc, first_rec and every input of the baselines (their
 * graphs stay separate: mmg_exchange_vjp); d data and d desc on request: mmg_vjp_input_grads, called right after.  fp32, deterministic (no float atomics); enqueued on `stream`. */
int mmg_exchange_vjp_channel(mmg_handle* h, int n_steps, const float* d_x, const float* d_desc, const float* d_dy,
                             const float* d_dz, const float* d_dw, const float* d_dps, void* stream);

/* Vector-Jacobian products of ONE agent-level forward call (mmg_sender_forward / mmg_receiver_forward / mmg_baseline_forward with
 * train = 1): the backward pass of that call alone, for a conversation the caller writes out of module calls.  Every array is
 * [B, .] (B = the handle's batch) and is the caller's copy of the call's inputs and outputs: the tape is never read, so any
 * forward, exchange or other VJP in between changes nothing.  The parameters must be the forward's.
 *   upstream gradients d_d*: NULL = zero.  Input-gradient outputs (d_dx, d_dw, d_dz, d_dh_prev, d_dbinary, d_dinp): NULL = not
 *   wanted; otherwise overwritten.  The weight gradients OVERWRITE the agent's slice of the gradient buffer (as mmg_exchange_vjp).
 *   sender:   x[B,F], w[B,W] (the code input; ignored when t == 0: sigmoid(code_bias) then, model.py:196-200), h_x[B,H] and
 *             probs[B,W] (binary; NULL if continuous) of the call; d_dout: d probs (binary) | d message logits (continuous),
 *             d_dh_x: d sender.h_x  ->  d_dx[B,F], d_dw[B,W] (t > 0)
 *   receiver: z[B,W], desc[D,V], h_prev[B,R] (NULL: the zero state of a first call), h_new[B,R] (= receiver.h_z after the
 *             call), y[B,D], w_probs[B,W] (binary), s_prob[B]; upstream d_dy[B,D], d_dw[B,W] (w_probs | w logits), d_dps[B],
 *             d_dh_w[B,R] (receiver.h_w), d_dh_new[B,R]  ->  d_dz[B,W], d_dh_prev[B,R] (the carry for the previous call's node).
 *             softmax(y) inside dbar and desc are constants (model.py:441).
 *   baseline: which = MMG_AGENT_BASELINE_REC/SEN; x[B,H] (sen) / binary[B,W] / inp[B,R] (rec) as in mmg_baseline_forward,
 *             rows == B; d_dscore[B]  ->  d_dx, d_dbinary, d_dinp.
 * fp32, deterministic (fixed summation order, no float atomics); enqueued on `stream`, no host synchronisation. */
int mmg_sender_vjp(mmg_handle* h, const float* d_x, const float* d_w, int t, const float* d_h_x, const float* d_probs,
                   const float* d_dout, const float* d_dh_x, float* d_dx, float* d_dw, void* stream);
int mmg_receiver_vjp(mmg_handle* h, const float* d_z, const float* d_desc, const float* d_h_prev, const float* d_h_new,
                     const float* d_y, const float* d_w_probs, const float* d_s_prob, const float* d_dy, const float* d_dw,
                     const float* d_dps, const float* d_dh_w, const float* d_dh_new, float* d_dz, float* d_dh_prev, void* stream);
int mmg_baseline_vjp(mmg_handle* h, int which, const float* d_x, const float* d_binary, const float* d_inp, int rows,
                     const float* d_dscore, float* d_dx, float* d_dbinary, float* d_dinp, void* stream);

/* Gradients with respect to the two inputs of the game, the image features data (x) and the class descriptions desc, which every
 * VJP above treats as constants.  Formed from the deltas that the VJP call IMMEDIATELY BEFORE this one, on the same handle and
 * stream, left in the workspace -- call order contract: mmg_exchange_vjp(sender) -> d_ddx; mmg_exchange_vjp(receiver) -> d_ddesc;
 * mmg_exchange_vjp_channel -> both (the deltas then hold the cross terms of the channel); with per_call != 0, mmg_receiver_vjp ->
 * d_ddesc over the call's B rows, with d_y the y[B,D] handed to that call (and mmg_sender_vjp -> d_ddx, which that call can
 * also return itself).  Asking for the gradient of an agent whose VJP did not run last reads stale deltas.
 *   d data[b, :] = (sum_{t < n} d pre_t[b, :]) . image_layer.weight: data enters through image_layer only (model.py:195);
 *                  baseline_sen reads h_x detached (model.py:835)
 *   d desc[d, :] = sum_r dCd[d, r] y1.weight[r, R:]                    through the class side of y1 (model.py:432 over build_inp)
 *                + sum_{t < n, b} softmax(y_t)[b, d] (w_d.weight^T d gpre_t[b, :])   through dbar (model.py:442-452)
 *   softmax(y) inside dbar stays a constant, as in the reference (model.py:441).  Sums run over the n_steps executed steps (per_call:
 *   the one call; n_steps is only range-checked); steps >= n_steps contribute exactly zero.
 *   d_ddx[B,F], d_ddesc[D,V]: NULL = not wanted; otherwise overwritten.  d_y: per_call only (the exchange VJPs read the tape's y).
 * Touches nothing else: the gradient buffer and every tape array the VJPs write stay bit-identical (its own scratch: vdq).
 * Errors: a NULL handle, n_steps outside 1..max_exchange, per_call with d_ddesc but without d_y.  fp32 on the matrix cores, a fixed
 * summation order, no float atomics: bit-identical from run to run; enqueued on `stream`, no host synchronisation. */
int mmg_vjp_input_grads(mmg_handle* h, int per_call, int n_steps, const float* d_y, float* d_ddx, float* d_ddesc, void* stream);

/* The loss functions of the training block as forward / vector-Jacobian launches over the CALLER'S tensors: handle-free (the
 * arithmetic depends on no mmg_config), on the calling thread's current device, enqueued on `stream`; no host synchronisation, no
 * hipMemset, at most 2 launches per forward and 1 per VJP.  Every array is fp32 and contiguous: per-step arrays are the reference's
 * lists stacked over the n_steps steps, [n_steps, batch, .]; d_mask / d_ymask [n_steps, batch] uint8 (NULL = the reference's
 * masks = None); d_target [batch] int64.  n_steps <= 1024 (an error beyond, never a truncation).  Sums over rows and row elements
 * are formed in float64 in an order fixed by the shapes (no float atomics): bit-identical from run to run.
 *   d_save: mmg_loss_save_doubles(n_steps) float64 of scratch the forward writes and the matching VJP reads (per step: active rows
 *   n_t, the std guard den_t, c_t / n_t, c_t; then partial sums) -- caller-owned like everything else, no initialisation needed.
 * With A_t = the rows of step t whose mask is set (all rows without masks), n_t = |A_t|, N = sum_t n_t, c_t = n_t / N with masks
 * (model.py:960-961) and 1 / n_steps without (model.py:967), eps = 1e-8; a step with n_t == 0 contributes 0; N == 0 gives NaN.
 *
 * mmg_loss_binary_forward <- multistep_loss_binary / calculate_loss_binary            model.py:930-968, 907-927
 *   feat, prob [n, B, W] (the sampled bits and their probabilities), logs [B], scores [n, B]; feat, logs and scores are constants
 *   (the reference detaches them).  lp = sum_j z log(p + eps) + (1 - z) log((1 - p) + eps); w = (logs - scores) / den_t, den_t =
 *   max(1, unbiased std over A_t of logs - scores) when n_t > 1, else 1 (model.py:912-915); ne_t = mean over A_t of
 *   sum_j p log(p + eps) + (1 - p) log((1 - p) + eps).  loss[1] = sum_t c_t (mean over A_t of -w lp + (has_entropy ?
 *   entropy_penalty ne_t : 0)); negent[n] = ne_t (the returned `entropies`).
 * mmg_loss_binary_vjp: d_dloss [1], d_dnegent [n] (either NULL = zero) -> d_dprob [n, B, W], overwritten in full (0 off A_t).
 *
 * mmg_loss_bas_forward <- multistep_loss_bas / calculate_loss_bas                      model.py:971-988
 *   loss[1] = sum_t c_t mean over A_t of (scores - logs)^2; logs is a constant (model.py:972).
 * mmg_loss_bas_vjp: d_dloss [1] (NULL = zero) -> d_dscores [n, B], overwritten in full.
 *
 * mmg_rec_outp_forward <- get_rec_outp, log_softmax, nll_loss, loglikelihood          model.py:879-904, 1264-1275, 571-577
 *   y [n, B, D] -> outp [B, D] = y[t*_b, b, :], t*_b = the first step whose ymask is set; the LAST step when ymask is NULL and
 *   for a row without a set step (the reference's masked_select is undefined there, model.py:896-900); negent [n] = mean over ALL
 *   rows of sum_d pi log(pi + eps), pi = softmax(y[t, b, :]) (model.py:880-886).  With d_target: logs [B] =
 *   log_softmax(outp)[b, target_b] (model.py:1274) and nll [1] = -mean_b logs (model.py:1271); a target outside [0, D) is not
 *   dereferenced, its logs entry and the nll are NaN.  d_target NULL: d_logs / d_nll are not touched.
 * mmg_rec_outp_vjp: d_doutp [B, D], d_dnll [1], d_dnegent [n] (each NULL = zero) -> d_dy [n, B, D], overwritten in full; reads
 *   no save array (t*_b and the softmax are recomputed from y and ymask). */
int64_t mmg_loss_save_doubles(int n_steps);                                       /* host only; -1 outside 1..1024 */
int mmg_loss_binary_forward(const float* d_feat, const float* d_prob, const float* d_logs, const float* d_scores,
                            const uint8_t* d_mask, int n_steps, int batch, int width, int has_entropy, float entropy_penalty,
                            float* d_loss, float* d_negent, double* d_save, void* stream);
int mmg_loss_binary_vjp(const float* d_feat, const float* d_prob, const float* d_logs, const float* d_scores,
                        const uint8_t* d_mask, const double* d_save, const float* d_dloss, const float* d_dnegent,
                        int n_steps, int batch, int width, int has_entropy, float entropy_penalty, float* d_dprob, void* stream);
int mmg_loss_bas_forward(const float* d_scores, const float* d_logs, const uint8_t* d_mask, int n_steps, int batch,
                         float* d_loss, double* d_save, void* stream);
int mmg_loss_bas_vjp(const float* d_scores, const float* d_logs, const uint8_t* d_mask, const double* d_save,
                     const float* d_dloss, int n_steps, int batch, float* d_dscores, void* stream);
int mmg_rec_outp_forward(const float* d_y, const uint8_t* d_ymask, const int64_t* d_target, int n_steps, int batch, int n_classes,
                         float* d_outp, float* d_negent, float* d_logs, float* d_nll, double* d_save, void* stream);
int mmg_rec_outp_vjp(const float* d_y, const uint8_t* d_ymask, const int64_t* d_target, const float* d_doutp, const float* d_dnll,
                     const float* d_dnegent, int n_steps, int batch, int n_classes, float* d_dy, void* stream);

/* The log block of a minibatch (model.py:1342-1461) gathered on the device: ONE launch writes one flat float64 vector the
 * caller copies to the host (asynchronously) and formats.  Layout (mmg_log_snapshot_count() doubles):
 *   with_losses != 0:  the tape's losses[8] | running top-k hit count totals[1] | the batch statistics "stats" |
 *                      ent[T]: mean over the WHOLE batch of sum_d softmax(y_t) log(softmax(y_t) + 1e-8) at every step ("Entropy
 *                      Receiver Predictions", model.py:880-886 -- meaningful on the tape of a run_all_steps = 1 minibatch) |
 *                      argmax[B] of the selected log-probabilities | target[B]                    ("Predictions", model.py:1379)
 *   dump = k > 0:      what the sample dump of the first k samples prints at every step (model.py:1411-1461): live samples
 *                      after each step [T] | sender probs, receiver probs, sender bits, receiver bits [T, k, W] each | stop
 *                      probabilities [T, k] | stop masks after each step [T, k]
 * Call it after the minibatch whose block is to be logged, on the same stream. */
int64_t mmg_log_snapshot_count(const mmg_config* cfg, int dump, int with_losses);
int mmg_log_snapshot(mmg_handle* h, const int64_t* d_target, int dump, int with_losses, double* d_out, void* stream);

/* Host-only helper of the epoch loop (no GPU work): shuffles perm[0..n) in place exactly as CPython's
 * `random.shuffle` would from the Mersenne-Twister state (624 words + position, `random.getstate()[1]`) -- the batch order of
 * misc.py:270-271 (`random.seed(11 + epoch); random.shuffle(order)`) without the per-sample interpreter loop. */
int mmg_host_shuffle(const uint32_t* mt_state, int pos, int64_t n, int64_t* perm);

/* Test/bench hooks: per-kernel timing of the most recent mmg_train_step measured with HIP events on
 * the launch stream (enable before the step; read after a stream sync). */
int mmg_set_profiling(mmg_handle* h, int enabled);
int mmg_get_kernel_times(mmg_handle* h, char* names, int names_bytes, float* ms, int max_kernels);

#ifdef __cplusplus
}
#endif
#endif /* MMG_H_ */
