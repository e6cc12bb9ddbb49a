/*
 * ocppo.h — C-ABI of libocppo_hip.so, the MI355X (gfx950) kernels behind the OC-CleanRL PPO
 * actor-learner hot path.
 *
 * The reference (BluemlJ/oc_cleanrl) is pure Python; there is no FFI to mirror. Each entry point
 * below replaces one stock-PyTorch op sequence of `cleanrl/ppo_atari_oc.py` (and its DP twin
 * `cleanrl/ppo_atari_multigpu.py`); the replaced lines are cited per function. A caller binds the
 * library with ctypes and passes torch `data_ptr()`s.
 *
 * Conventions (all functions):
 *   - every pointer is a caller-owned DEVICE pointer unless stated otherwise; nothing allocates;
 *   - `stream` is a hipStream_t (NULL = legacy default stream); every launch is asynchronous and
 *     graph-capturable (no host sync, no hipMalloc, no memcpy to host inside);
 *   - the return value is 0 on success, otherwise an OCPPO_E_* code; ocppo_last_error() returns
 *     a thread-local message for the last failure. Nothing throws or aborts across the ABI;
 *   - results are deterministic: fixed-order reductions, no floating-point atomics;
 *   - scalar hyper-parameters are passed as double, exactly as the reference's Python floats,
 *     and rounded to f32 inside the library exactly where PyTorch rounds them.
 *   - all buffers are step-major: element (t, n) of a [T, N] rollout array is at t*N + n
 *     (ppo_atari_oc.py:452-459, flattened at :550-555).
 */
#ifndef OCPPO_H
#define OCPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCPPO_ABI_VERSION 44

/* status codes */
#define OCPPO_OK 0
#define OCPPO_E_INVALID 1   /* bad argument (null pointer, size, dtype) */
#define OCPPO_E_LAUNCH 2    /* hipGetLastError() after a launch */
#define OCPPO_E_WORKSPACE 3 /* workspace missing or too small */

/* element types used by the obs storage / frame arguments */
#define OCPPO_F32 0
#define OCPPO_BF16 1
#define OCPPO_U8 2

/* net_flags of the rollout store / reset / channels-last gather */
#define OCPPO_NET_CHANNELS_LAST 1
#define OCPPO_NET_SCALE_255 2

/* layout of the `stats` output of ocppo_ppo_loss_fwd_bwd (all f32) */
#define OCPPO_STAT_LOSS 0          /* loss = pg - ent_coef*entropy + vf_coef*v_loss   :599-602 */
#define OCPPO_STAT_PG_LOSS 1       /* pg_loss                                        :581-583 */
#define OCPPO_STAT_V_LOSS 2        /* v_loss                                         :585-597 */
#define OCPPO_STAT_ENTROPY 3       /* entropy_loss = mean(entropy)                   :599     */
#define OCPPO_STAT_OLD_APPROX_KL 4 /* mean(-logratio)                                :573     */
#define OCPPO_STAT_APPROX_KL 5     /* mean((ratio-1) - logratio)                     :574     */
#define OCPPO_STAT_CLIPFRAC 6      /* mean(|ratio-1| > clip_coef)                    :575     */
#define OCPPO_STAT_ADV_MEAN 7      /* minibatch advantage mean used by the norm      :577-579 */
#define OCPPO_STAT_ADV_STD 8       /* minibatch advantage std (unbiased)             :577-579 */
#define OCPPO_NUM_STATS 9

typedef void* ocppo_stream_t; /* hipStream_t */
/* A deferred finish (ocppo_heads_loss_rows, ocppo_relu_bias_wgrad_rows): a plain host record of
 * device pointers and sizes, run later by ocppo_sum_splits_finish / ocppo_sum_splits_db_finish /
 * ocppo_deferred_finish_run. */
typedef struct ocppo_deferred_finish {
  uint64_t opaque[64];
} ocppo_deferred_finish_t;

#if defined(__GNUC__) || defined(__clang__)
#define OCPPO_API __attribute__((visibility("default")))
#else
#define OCPPO_API
#endif

OCPPO_API int ocppo_abi_version(void);
OCPPO_API const char* ocppo_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * GAE — replaces the reverse Python loop of ppo_atari_oc.py:533-547 (identical in ppo.py:218-231
 * and ppo_atari_multigpu.py:288-301); 9 ATen launches per step → one kernel per rollout.
 *   rewards, values, dones : [T, N] f32;   next_value, next_done : [N] f32
 *   advantages, returns    : [T, N] f32 outputs (returns = advantages + values)
 * f32 arithmetic in the reference's exact op order (no FMA contraction), so the result is
 * bit-identical to the PyTorch loop:  delta = (r + (f32(gamma)*nv)*nnt) - v;
 *                                     A = delta + (f32(gamma*lambda)*nnt)*A'
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_gae(ocppo_stream_t stream, const float* rewards, const float* values, const float* dones,
              const float* next_value, const float* next_done, int64_t T, int64_t N, double gamma,
              double gae_lambda, float* advantages, float* returns);
/* GAE that also writes each sample's record (OcppoSampleRecord: log-prob, advantage, value,
 * action) in batch order for ocppo_minibatch_prepare_records; advantages / returns as ocppo_gae,
 * bit for bit. logprobs [T, N] f32 16-B aligned, actions [T, N] int64 in [0, 2^31), records
 * [T*N] 16-B aligned. */
OCPPO_API int ocppo_gae_records(ocppo_stream_t stream, const float* rewards, const float* values,
                                const float* dones, const float* next_value,
                                const float* next_done, int64_t T, int64_t N, double gamma,
                                double gae_lambda, float* advantages, float* returns,
                                const float* logprobs, const int64_t* actions, void* records);

/* ---------------------------------------------------------------------------------------------
 * Minibatch advantage statistics — the (mean, unbiased std) pair of ppo_atari_oc.py:577-579 for
 * `num_mb` minibatches at once. Minibatch k holds b_advantages[perm[k*M + i]], i < M.
 *   perm : [num_mb*M] int64 (the np.random.shuffle'd b_inds of :561, all epochs concatenated)
 *   out  : [num_mb, 2] f32 = {mean, std}
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_minibatch_adv_stats(ocppo_stream_t stream, const float* b_advantages, const int64_t* perm,
                              int64_t M, int64_t num_mb, float* out);

/* Minibatch prepare: the statistics above AND the per-sample records of every minibatch gathered
 * into minibatch order, mb_*[k*M + i] = b_*[perm[k*M + i]] (SoA), so that each
 * ocppo_ppo_loss_fwd_bwd launch can take the already-gathered arrays (mb_inds = NULL) instead of
 * five scattered loads per element (ppo_atari_oc.py:569-593 index b_* by mb_inds). One launch:
 * gather blocks over all num_mb*M elements on a chip-filling grid beside one statistics block
 * per minibatch (bitwise the figures of ocppo_minibatch_adv_stats).
 * adv_stats : [num_mb, 2] or NULL (statistics skipped). */
OCPPO_API int ocppo_minibatch_prepare(ocppo_stream_t stream, const int64_t* perm, int64_t M,
                                      int64_t num_mb, const int64_t* b_actions,
                                      const float* b_logprobs, const float* b_advantages,
                                      const float* b_returns, const float* b_values,
                                      int64_t* mb_actions, float* mb_logprobs,
                                      float* mb_advantages, float* mb_returns, float* mb_values,
                                      float* adv_stats);

/* ---------------------------------------------------------------------------------------------
 * The same, from 16-B per-sample records (OcppoSampleRecord, written by ocppo_gae_records): one
 * 16-B gather per sample instead of five scattered 4-8 B ones (the batch arrays of
 * ppo_atari_oc.py:550-555 are the records' fields; the return is advantage + value, GAE's own f32
 * add); outputs and statistics bitwise those of ocppo_minibatch_prepare. records: 16-B aligned,
 * [B]; actions in [0, 2^31). From 2^20 samples (num_mb x M) on, the statistics are taken by a
 * second launch from the gathered advantages (contiguous reads; same values, same order). 
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  float logprob, advantage, value;
  int32_t action;
} OcppoSampleRecord;
OCPPO_API int ocppo_minibatch_prepare_records(ocppo_stream_t stream, const int64_t* perm,
                                              int64_t M, int64_t num_mb, const void* records,
                                              int64_t* mb_actions, float* mb_logprobs,
                                              float* mb_advantages, float* mb_returns,
                                              float* mb_values, float* adv_stats);

/* ---------------------------------------------------------------------------------------------
 * Fused PPO minibatch loss, forward AND backward — replaces ppo_atari_oc.py:566-602 from the
 * network's raw outputs onward (Categorical log-softmax / log_prob / entropy of
 * architectures/ppo.py:89-95, ratio, KL stats, clipfrac, advantage norm, clipped surrogate,
 * clipped value loss, entropy bonus) plus the autograd backward of that graph down to the
 * network outputs.
 *   logits    : [M, A] f32 raw actor outputs;  new_value : [M] f32 critic outputs
 *   mb_inds   : [M] int64 indices into the b_* batch arrays, or NULL (inputs already gathered,
 *               b_*[i] is element i)
 *   b_actions : int64 [B]; b_logprobs, b_advantages, b_returns, b_values : f32 [B]
 *   adv_stats : [2] f32 {mean, std} from ocppo_minibatch_adv_stats, or NULL to compute them
 *               here (then workspace must be given); ignored when norm_adv == 0
 *   dlogits   : [M, A] f32 = dLoss/dlogits;  dvalue : [M] f32 = dLoss/dnew_value
 *   stats     : [OCPPO_NUM_STATS] f32 (layout above)
 *   workspace : device scratch of ocppo_ppo_loss_workspace_bytes(M, A) bytes; it must be zeroed
 *               once after allocation and then never touched by the caller (its ticket word is
 *               reset by the kernel itself, so the call can be replayed from a graph).
 * Gradient rules follow autograd exactly: torch.max splits the gradient 1/2-1/2 on ties, clamp
 * passes it at the bounds.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_ppo_loss_workspace_bytes(int64_t M, int64_t A);
OCPPO_API int ocppo_ppo_loss_fwd_bwd(ocppo_stream_t stream, const float* logits, const float* new_value,
                           int64_t M, int64_t A, const int64_t* mb_inds, const int64_t* b_actions,
                           const float* b_logprobs, const float* b_advantages,
                           const float* b_returns, const float* b_values, const float* adv_stats,
                           double clip_coef, double ent_coef, double vf_coef, int norm_adv,
                           int clip_vloss, float* dlogits, float* dvalue, float* stats,
                           void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Gradient clipping + Adam over ONE flat buffer — replaces
 * `nn.utils.clip_grad_norm_(agent.parameters(), max_grad_norm); optimizer.step()` of
 * ppo_atari_oc.py:608-610 (torch.optim.Adam(lr, eps=1e-5), betas (0.9, 0.999)) and the
 * `grads / world_size` of ppo_atari_multigpu.py:369-374 (grad_scale = 1/world_size).
 *   params, grads, exp_avg, exp_avg_sq : [P] f32, 16-byte aligned; every parameter tensor of the
 *                                        agent is a view into `params` (grads likewise)
 *   lr       : device f32 scalar (annealed in place, graph-replay safe)
 *   scalars  : device f32[OCPPO_OPT_NUM_SCALARS], zero-initialised; the step count lives here and
 *              total_norm (the value clip_grad_norm_ returns) is reported here
 *   max_norm : <= 0 disables clipping
 * Math per element, f32: g = (g*grad_scale)*clip; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 * p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)  (ATen's fused-Adam formula).
 * ocppo_clip_adam_step, ocppo_clip_adam_step_exact and ocppo_clip_radam_step (below) are one norm
 * launch and one step kernel: they share the argument checks (betas in [0, 1), all four buffers
 * 16-byte aligned, the workspace), the clip, the scalars' layout and the vectorised body with its
 * P % 4 tail, and differ in the step scalars and the per-element update alone.
 * ------------------------------------------------------------------------------------------- */
#define OCPPO_OPT_STEP 0
#define OCPPO_OPT_TOTAL_NORM 1
#define OCPPO_OPT_CLIP_COEF 2
#define OCPPO_OPT_STEP_SIZE 3
#define OCPPO_OPT_BC2_SQRT 4
#define OCPPO_OPT_NUM_SCALARS 8
OCPPO_API size_t ocppo_clip_adam_workspace_bytes(int64_t P);
/* n_planes (0..8) plane jobs: the new values of the row-major [plane_rows[j], plane_cols[j]]
 * weight at params + plane_offset[j] (offset % 4 == 0, cols % 4 == 0) are also written as the
 * three exact bf16 pieces ocppo_split_planes writes for it (trans as plane_trans[j]), piece p at
 * plane_dst[j] + p * rows * cols: the next update's GEMMs read them without a split launch. */
OCPPO_API int ocppo_clip_adam_step(ocppo_stream_t stream, float* params, const float* grads,
                                   float* exp_avg, float* exp_avg_sq, int64_t P, const float* lr,
                                   double beta1, double beta2, double eps, double grad_scale,
                                   double max_norm, float* scalars, void* workspace,
                                   size_t workspace_bytes, int n_planes,
                                   const int64_t* plane_offset, const int64_t* plane_rows,
                                   const int64_t* plane_cols, const int* plane_trans,
                                   void* const* plane_dst);

/* ---------------------------------------------------------------------------------------------
 * Rollout action head — replaces Categorical(logits).sample() / log_prob / entropy of
 * architectures/ppo.py:91-95 and the storage writes of ppo_atari_oc.py:506-510.
 * torch's sampler (Categorical.sample → multinomial(probs, 1, True)) draws q ~ Exp(1) of shape
 * [N, A] and returns argmax(probs / q); `noise` must be that q (e.g. from
 * torch.empty(N, A).exponential_() on the same generator), so actions are bit-identical.
 *   logits : [N, A] f32; noise : [N, A] f32
 *   action_out : [N] int64 (e.g. &actions[t*N]);  logprob_out : [N] f32 (&logprobs[t*N])
 *   entropy_out : [N] f32 or NULL
 *   value_in / value_out : critic output [N] copied into &values[t*N] (both NULL to skip)
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_categorical_sample(ocppo_stream_t stream, const float* logits, float* noise,
                             const int64_t* philox_state, int64_t philox_offset,
                             int64_t philox_stride, int64_t N, int64_t A, int64_t* action_out,
                             float* logprob_out, float* entropy_out, const float* value_in,
                             float* value_out);

/* The sampling entries' Exp(1) values (ocppo_categorical_sample, ocppo_policy_head_sample,
 * ocppo_policy_head_env_step) come from one of two places:
 *   philox_state == NULL : noise [N, A] is read (any source);
 *   philox_state != NULL : the kernel draws them itself, bit for bit the values
 *     torch.empty(N, A, device=...).exponential_() returns on the CUDA/HIP generator whose
 *     (seed, philox offset) is (philox_state[0], philox_state[1] + philox_offset) -- the stream
 *     Categorical.sample() consumes per step in the reference (architectures/ppo.py:92-94 via
 *     torch.multinomial's Exp(1) path; ppo_atari_oc.py:505-506) -- with philox_stride = torch's
 *     grid stride for N*A elements (ocppo_torch_exponential_geometry); noise, when non-NULL,
 *     receives them. philox_state is device memory [2] (graph-capturable: a replay reads the
 *     generator state of that replay). */

/* torch's launch geometry of exponential_ over `numel` elements (ATen DistributionTemplates.h
 * calc_execution_policy): the grid stride (256 * grid, grid <= cus * max_threads_per_cu / 256) and
 * the generator's philox-offset increment per draw. Host only. */
OCPPO_API int ocppo_torch_exponential_geometry(int64_t numel, int64_t cus, int64_t max_threads_per_cu,
                                               int64_t* stride, int64_t* offset_increment);

/* out[numel] = torch.empty(numel).exponential_() at generator (philox_state[0], philox_state[1] +
 * philox_offset), grid stride philox_stride (the reference stream of the sampling entries,
 * on its own: tests, and callers that need the draws as a tensor). */
OCPPO_API int ocppo_philox_exponential(ocppo_stream_t stream, float* out, int64_t numel,
                                       const int64_t* philox_state, int64_t philox_offset,
                                       int64_t philox_stride);
/* `steps` such draws back to back, as `steps` successive exponential_ calls of one shape make
 * them: out[t * numel + i] = element i of the draw at philox offset philox_offset + t * increment
 * (increment from ocppo_torch_exponential_geometry). One launch for a whole rollout's
 * Categorical.sample draws (the reference's per-step stream, ppo_atari_oc.py:505-506). */
OCPPO_API int ocppo_philox_exponential_steps(ocppo_stream_t stream, float* out, int64_t numel,
                                             int64_t steps, const int64_t* philox_state,
                                             int64_t philox_offset, int64_t increment,
                                             int64_t philox_stride);

/* Fused rollout policy head: logits = hidden @ w_actor^T + b_actor, value = hidden . w_critic +
 * b_critic, then the sampler above — replaces the actor/critic Linear layers AND the sampler of
 * architectures/ppo.py:89-95 for one rollout step (PPObj / PPODefault, shared hidden layer).
 *   hidden : [N, H] f32 (decoder output);  w_actor : [A, H];  b_actor : [A];  w_critic : [H];
 *   b_critic : [1];  noise : [N, A] Exp(1) (or drawn: philox_*, above);  value_out : [N];
 *   entropy_out, logits_out ([N, A]) may be NULL.
 * Logits differ from a GEMM's only by f32 summation order; actions are bit-exact w.r.t. the
 * sampler applied to the logits this kernel computes (returned in logits_out). */
OCPPO_API int ocppo_policy_head_sample(ocppo_stream_t stream, const float* hidden, int64_t N,
                                       int64_t H, const float* w_actor, const float* b_actor,
                                       const float* w_critic, const float* b_critic,
                                       float* noise, const int64_t* philox_state,
                                       int64_t philox_offset, int64_t philox_stride, int64_t A,
                                       int64_t* action_out, float* logprob_out,
                                       float* entropy_out, float* value_out, float* logits_out);

/* log_prob(action) and entropy() of Categorical(logits) for given actions (architectures/ppo.py
 * :92-95 with `action` passed) and the matching backward. */
OCPPO_API int ocppo_categorical_logprob_entropy(ocppo_stream_t stream, const float* logits,
                                      const int64_t* actions, int64_t N, int64_t A,
                                      float* logprob_out, float* entropy_out);
OCPPO_API int ocppo_categorical_logprob_entropy_bwd(ocppo_stream_t stream, const float* logits,
                                          const int64_t* actions, const float* grad_logprob,
                                          const float* grad_entropy, int64_t N, int64_t A,
                                          float* dlogits);

/* ---------------------------------------------------------------------------------------------
 * Rollout store — replaces ppo_atari_oc.py:502-503 and :512-514 (host float32 conversion,
 * pageable H2D copies and `obs[step] = next_obs`) with one device pass per env step that also
 * performs the frame stacking the reference does in N env subprocesses.
 *   frame      : [N, D] newest frame per env, dtype frame_dtype (OCPPO_F32 object vectors of
 *                OCAtari obj mode, D = F; or OCPPO_U8 grayscale 84x84 pixels, D = 7056)
 *   reward     : [N] f32;  done : [N] f32 (0/1)
 *   prev_obs   : [N, W, D] stacked obs of the previous step, dtype obs_dtype (rollout slot t)
 *   obs_out    : [N, W, D] new stacked obs, dtype obs_dtype (rollout slot t+1)
 *   net_obs    : f32 copy of obs_out for the network forward (may be NULL when net_layout = 0)
 *   reward_out : [N] f32 (&rewards[t*N]);  done_out : [N] f32 (&dones[(t+1)*N]); either may be NULL
 *   net_flags  : bit 0 (OCPPO_NET_CHANNELS_LAST): net_obs in channels-last order [N, D, W] (the
 *                NHWC input of a channels_last NatureCNN, 16-B aligned; MIOpen's NHWC
 *                convolutions then need no transpose), else [N, W, D] like obs_out;
 *                bit 1 (OCPPO_NET_SCALE_255): net_obs = value / 255 as ATen computes it
 *                (x * (1.0f / 255.0f)) -- the NatureCNN's NormalizeImg (architectures/common.py:19-22)
 *                folded into the store
 *   reset_prev : [N, W-1, D] frame_dtype or NULL: the older W-1 frames of the observation the env
 *                itself returned on a done (read for done rows only)
 * Stacking: obs_out[n] = prev_obs[n][1:] ++ frame[n]; on done[n] the older W-1 slots are
 * reset_prev[n] when given (a host env whose reset stack holds distinct frames: the reference's
 * NoopResetEnv/FireResetEnv step after reset, EpisodicLifeEnv signals done on a life loss without
 * resetting the stack, ppo_atari_oc.py:278-282), else frame[n] (the gymnasium FrameStack reset
 * fill). Conversion to bf16 is round-to-nearest-even and exact for the integer-valued obs of both
 * modes (|x| <= 256).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_rollout_store(ocppo_stream_t stream, const void* frame, int frame_dtype,
                        const float* reward, const float* done, int64_t N, int64_t W, int64_t D,
                        const void* prev_obs, void* obs_out, int obs_dtype, float* net_obs,
                        float* reward_out, float* done_out, int net_flags, const void* reset_prev);

/* Fill a whole stacked-obs slot from one frame per env (env reset, ppo_atari_oc.py:464-465);
 * net_flags as in ocppo_rollout_store. */
OCPPO_API int ocppo_obs_reset(ocppo_stream_t stream, const void* frame, int frame_dtype, int64_t N,
                    int64_t W, int64_t D, void* obs_out, int obs_dtype, float* net_obs,
                    int net_flags);

/* ---------------------------------------------------------------------------------------------
 * Frame-encoding cache of the rollout forward (PPObj, architectures/ppo.py:60-84, whose encoder
 * is applied to each stacked frame on its own). `agent.get_action_and_value(next_obs)` at
 * ppo_atari_oc.py:506 re-encodes all W stacked frames every step although W-1 of them were
 * encoded at the previous steps under the same weights; with this entry point the caller encodes
 * only the newest frame and shifts the cache like the frame stack (same reset fill as
 * ocppo_rollout_store):
 *   enc[n, w, :] = done[n] != 0 || w == W-1 ? fresh[n, :] : enc[n, w+1, :]   (in place)
 * enc [N, W, E] f32, fresh [N, E] f32 with row stride ld_fresh (>= E), done [N] f32 or NULL.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_frame_cache_shift(ocppo_stream_t stream, float* enc, const float* fresh,
                            int64_t ld_fresh, const float* done, int64_t N, int64_t W, int64_t E);

/* ---------------------------------------------------------------------------------------------
 * Rollout-batch Linear(+ReLU): y[M, N] = act(x[M, K] @ w[N, K]^T + b[N]) in f32 on the matrix
 * cores (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation; summation order differs
 * from the BLAS library's). Replaces the nn.Linear(+nn.ReLU) layers of architectures/ppo.py:60-84
 * (PPObj) and the NatureCNN head :36-46 in the rollout forward of ppo_atari_oc.py:506, :534
 * (no autograd: the rollout runs under torch.no_grad()), where M is the number of envs (or envs x
 * frames) and the library's large tiles leave the chip idle.
 *   x : row stride ldx (>= K); w : nn.Linear weight, row-major [N, K]; b : [N] or NULL;
 *   y : row stride ldy (>= N); relu : 0 = identity, 1 = max(., 0) after the bias.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_linear_act(ocppo_stream_t stream, const float* x, int64_t ldx, const float* w,
                     const float* b, float* y, int64_t ldy, int64_t M, int64_t N, int64_t K,
                     int relu);

/* ---------------------------------------------------------------------------------------------
 * Linear(+ReLU) backward, elementwise part, in one pass — replaces the threshold_backward + bias
 * `sum(0)` pair autograd runs inside `loss.backward()` (ppo_atari_oc.py:605) for every
 * nn.Linear -> nn.ReLU of architectures/ppo.py:60-84 / :44-46:
 *   gp[r, n] = out[r, n] <= 0 ? 0 : g[r, n]   (out = the layer's ReLU output; out == NULL: no
 *                                             ReLU, gp unused and may be NULL)
 *   db[n]    = sum_r gp[r, n]                 (deterministic fixed-order reduction)
 * g/out/gp [R, N] f32 row-major, 16-B aligned, N % 4 == 0, N <= 16384; workspace 256-B aligned,
 * >= ocppo_relu_bias_grad_workspace_bytes(R, N), ZEROED before its first use (its tickets re-arm).
 * ------------------------------------------------------------------------------------------- */
/* Forward epilogue of a bias-less convolution / GEMM in NHWC / row-major layout, in place:
 *   y[r, n] = act(y[r, n] + b[n])   (act = ReLU when relu != 0; torch's conv + bias then ReLU,
 *                                    one f32 rounding for the add, architectures/ppo.py:20-31)
 * y [R, N] f32, b [N] f32, both 16-B aligned, N % 4 == 0. */
OCPPO_API int ocppo_bias_act(ocppo_stream_t stream, float* y, const float* b, int64_t R, int64_t N,
                   int relu);
/* The same epilogue with the output in NCHW order (the rollout's last NatureCNN convolution, whose
 * nn.Flatten reads NCHW, architectures/ppo.py:20-31): out[b, c, p] = act(y[b, p, c] + bias[c]),
 * y [B, P, C] NHWC f32 (P = H*W), out [B, C, P] f32 (not aliasing y), P * (C + 1) <= 12288. */
OCPPO_API int ocppo_bias_act_nchw(ocppo_stream_t stream, const float* y, const float* b, int64_t B,
                                  int64_t P, int64_t C, int relu, float* out);

/* ---------------------------------------------------------------------------------------------
 * Update-phase f32 GEMM on the bf16 matrix cores — replaces the f32 GEMMs (addmm /
 * _addmm_activation forward, g'W dX, split-K g'^T x dW) of the Linear layers that
 * `agent.get_action_and_value(b_obs[mb])` and `loss.backward()` run (ppo_atari_oc.py:566-606
 * through architectures/ppo.py:60-84):
 *   C_s[m, n] = act( sum_{k in K_s} A(m, k) B(n, k) + bias[n] )     s = 0 .. splits-1
 *   A(m, k) = a[m*sam + k*sak], B(n, k) = b[n*sbn + k*sbk], C_s[m, n] = c[s*split_c + m*ldc + n]
 *   K_s = steps [s*nk/splits, (s+1)*nk/splits) of the nk = K/32 steps of 32 (even partition)
 * Each f32 operand is split exactly into three bf16 pieces (x = x0 + x1 + x2) and the six piece
 * products down to 2^-24 of |a b| are accumulated in f32 (one accumulator per output with tile
 * bit 4 and the mixed tiles, the shipped forms; the small terms in a second one otherwise):
 * f32-level accuracy (tests/test_gemm_gpu.py: error vs f64 at or below
 * hipBLASLt's f32 GEMM) at 6 bf16 MFMAs per f32 multiply-add.
 * One of (sam, sak) and one of (sbn, sbk) must be 1 (the other a multiple of 4, >= the extent it
 * strides over); a, b 16-B aligned; K % 32 == 0, K / 32 >= splits; M, N multiples of the tile (tile 0: 128 x 128,
 * 1: 64 x 128, 2: 128 x 64, 3: 64 x 64 rows x columns); bias (NULL: none) and relu only with
 * splits == 1. Mask epilogue (mask != NULL; the dX product of the layer above a Linear+ReLU,
 * whose input `mask` [M, N] (row stride ldm) is that ReLU's output): C = mask > 0 ? acc : 0
 * (threshold_backward) and dbp[tm, n] = sum of C over row tile tm (tile rows each) — that layer's
 * bias-gradient partials, [M / tile rows, N], for ocppo_sum_splits_db; splits == 1, no bias/relu.
 * ReLU bitmask (mbits: (M / tile rows) x (N / tile columns) x threads per workgroup (256, or 512
 * for the 8-wave shapes) 64-bit words): a forward with relu writes, per tile and thread, one word
 * of !(output <= 0) bits in the MFMA fragment order (mbits_out); the mask
 * epilogue of a later dX over the same [M, N] with the same tile reads them (mbits_in, mask may
 * then be NULL) instead of the f32 mask. tile: bits 0-2 the tile shape (0: 128 x 128, 1: 64 x
 * 128, 2: 128 x 64, 3: 64 x 64 with 4 waves; 4-7: 8-wave forms), bit 3 loads two K steps ahead,
 * bit 4 one accumulator for all six products. tile 56 (bit 5: mixed tiles; splits == 1): rows
 * [0, mbig) in 128 x 128 tiles dispatched first, rows [mbig, M) in 64 x 128 tiles — mbig chosen
 * by the library (one 128 x 128 tile per CU when the output holds 257..384 of them, else all of
 * M) when mbig is -1; mbig >= 0 imposes the split (a multiple of 128, (mbig / 128)(N / 128) a
 * multiple of 8; experiments and tests); mbig must be -1 for every other tile. M, N multiples of
 * 64 x 128, and dbp rows / mbits words counted as for 64 x 128 (a 128-row tile's dbp partial sits in the first of its two rows, the second is written as zeros).
 * Pre-split B (b_planes != NULL; b is then ignored and may be NULL): the three bf16 pieces of
 * B(n, k) at b_planes[p * bp_stride + n * bp_ld + k] (p = 0, 1, 2; ocppo_split_planes wrote them
 * from the f32 B, so the result is bitwise that of the f32 B): staged by copy, no split in the
 * K loop. Needs sak == 1, bp_ld % 8 == 0, 16-B aligned planes, tile 24..27, 56, 57 or 58.
 * relu | OCPPO_X6_MBITS_ROWS (with relu and mbits_out): mbits_out is row-major instead,
 * (M x N / 32) 32-bit words, bit n % 32 of word [m][n / 32] = !(C[m, n] <= 0) — for a consumer
 * that walks the output by rows (ocppo_frames_scatter_relu's mbits).
 * Tiles 57-60 (the pipelined family): 256 x 128, 128 x 256 (8 waves), 128 x 128 (4 waves) and
 * 128 x 128 (8 waves) with two LDS stages and one barrier per K step (the next step's operand
 * split in the MFMAs' shadow); one workgroup per CU.
 * Deterministic (fixed MFMA order, no atomics).
 * ------------------------------------------------------------------------------------------- */
#define OCPPO_X6_MBITS_ROWS 2
OCPPO_API int ocppo_gemm_x6(ocppo_stream_t stream, const float* a, int64_t sam, int64_t sak,
                            const float* b, int64_t sbn, int64_t sbk, float* c, int64_t ldc,
                            int64_t M, int64_t N, int64_t K, int64_t splits, int64_t split_c,
                            const float* bias, int relu, const float* mask, int64_t ldm,
                            float* dbp, uint64_t* mbits_out, const uint64_t* mbits_in,
                            int tile, int mbig, const void* b_planes, int64_t bp_ld,
                            int64_t bp_stride, void* sk_workspace, size_t sk_workspace_bytes);

/* Bytes of the stream-K workspace of a pipelined tile (57, 58; 0 for every other tile). With
 * sk_workspace != NULL ocppo_gemm_x6 runs a pipelined product (tiles 57 / 58: 256 x 128 /
 * 128 x 256, two LDS stages, one workgroup per CU) as a persistent stream-K launch: the tiles are
 * dealt to the 8 XCDs, each XCD's CUs share its tiles' K steps in equal contiguous ranges, and a
 * tile split between two workgroups is finished by the one holding its first K steps, after the
 * later parts' partial accumulators arrive through the workspace (same XCD, so its L2) — every
 * CU busy to the end at any tile count. splits == 1; the workspace must be 256-B aligned and
 * zero before the first launch (its flags return to zero after every launch). Same products in
 * the same order within a part; the parts are added in K order: deterministic. */
OCPPO_API size_t ocppo_gemm_x6_sk_workspace_bytes(int tile);

/* ---------------------------------------------------------------------------------------------
 * ocppo_gemm_x6 with one operand's rows read through a row table (the update's decoder on the
 * Flatten of the stacked frame encodings, architectures/ppo.py:77-80, without materialising the
 * [M, W * E] input of ppo_atari_oc.py:566's b_obs[mb_inds] forward):
 *   mode 1: A(m, k) = a[gidx[m * gw + k / gseg] * sam + k % gseg]   (sak == 1, K == gw * gseg,
 *           every split's K range inside one segment: gseg % (K / splits) == 0)
 *   mode 2: B(n, k) = b[gidx[k * gw + n / gseg] * sbk + n % gseg]   (sbn == 1, N == gw * gseg,
 *           gseg % 128 == 0, K / splits <= 1024; A m-contiguous, as a weight gradient's g'^T)
 * gidx int32 (mode 1: [M, gw], mode 2: [K, gw]; e.g. ocppo_frames_expand_index). The 128 x 128
 * tile (variant 24), M % 128 == N % 128 == 0, (K / 32) % splits == 0; bias / ReLU only with
 * splits == 1; b_planes (mode 1) as ocppo_gemm_x6's. Bitwise ocppo_gemm_x6 on the gathered
 * operand written out.
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * The dX product of a layer above a Linear+ReLU whose input needs no gradient, with that lower
 * layer's whole backward in the epilogue (the PPObj encoder's second layer above the first,
 * ppo_atari_oc.py:605 through architectures/ppo.py:60-84): with C = A B as ocppo_gemm_x6 (A = g'
 * [M, K] k-contiguous, B(n, k) = W[k, n] n-contiguous: dX = g' W), gp = mask > 0 ? C : 0 (mask
 * [M, N] = the lower layer's ReLU output, row stride ldm) is never stored; instead
 *   db[n] = sum_m gp[m, n],   dw[n, k1] = sum_m gp[m, n] x[m, k1]   (x [M, K1], K1 <= 16)
 * are formed as per-row-tile records in `records` (>= (M / tile rows) * ceil(N / 256) * 256 *
 * (K1 padded to 4 / 8 / 12 / 16, + 1) floats) and finished later from *finish (as
 * ocppo_relu_bias_wgrad_rows': ocppo_sum_splits_db_finish or ocppo_deferred_finish_run).
 * tile 27 (64 x 64) or 24 (128 x 128); M, N multiples of the tile, K % 32 == 0. Deterministic.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_gemm_x6_wgrad(ocppo_stream_t stream, const float* a, int64_t sam, int64_t sak,
                                  const float* b, int64_t sbn, int64_t sbk, int64_t M, int64_t N,
                                  int64_t K, const float* mask, int64_t ldm, const float* x,
                                  int64_t ldx, int64_t K1, float* dw, float* db, float* records,
                                  int64_t records_floats, int tile,
                                  ocppo_deferred_finish_t* finish);
OCPPO_API int ocppo_gemm_x6_gather(ocppo_stream_t stream, const float* a, int64_t sam, int64_t sak,
                                   const float* b, int64_t sbn, int64_t sbk, float* c, int64_t ldc,
                                   int64_t M, int64_t N, int64_t K, int64_t splits,
                                   int64_t split_c, const float* bias, int relu,
                                   const void* b_planes, const int32_t* gidx, int64_t gw,
                                   int64_t gseg, int mode);

/* ---------------------------------------------------------------------------------------------
 * NHWC convolution (no padding, square stride) as an implicit GEMM on ocppo_gemm_x6's exact
 * three-piece bf16 products (the NatureCNN trunk, cleanrl/architectures/ppo.py:20-31: replaces
 * the convolution forward / backward cuDNN (MIOpen) runs for nn.Conv2d at ppo_atari_oc.py:506
 * and :566-606; deterministic: no atomics, split-K partials summed in split order). No im2col
 * buffer: the convolution rows r = (b, qy, qx) over [B, qh, qw] read element k of their kernel
 * window at x[b sb + qy ys + qx xs + (k / gseg) segs + k % gseg], geom = {qh, qw, sb, ys, xs,
 * segs, gseg} (floats; a segment = one kernel row's KW x C taps, contiguous in NHWC; all strides
 * multiples of 4, x and w 16-B aligned, B qh qw < 2^24).
 *   mode 0 (forward; and each stride class of the data gradient, over the zero-padded output
 *          gradient with the flipped weight): c[row(r) + n] = act(sum_k x(r, k) w[n ldw + k] +
 *          bias[n]) for r < M = B qh qw, n < N, k < K; gseg % 32 == 0; splits > 1 (no bias,
 *          ReLU or out_geom, ldc == N): K-split partials [splits, M, N] in c instead; row(r) =
 *          r ldc, or b sb' + qy ys' + qx xs' + off' with out_geom = {sb', ys', xs', off', cw,
 *          cs, cy, cx}, column n then at row(r) + (c / cs) cy + (c % cs) cx + n % cw, c = n / cw
 *          (all stride classes of a data gradient in one product: they read the same rows).
 *   mode 1 (weight gradient): out[m, n] = sum_r w[r ldw + m] x(r, n) (w = the output gradient
 *          [rows, ldw], m < M = Cout, n < N = KH KW C, r < K = B qh qw); c = split partials
 *          [splits, M, N], then summed in split order (f64, one rounding) into out; qh qw <= 1024.
 * mask (mode 0, or null; needs dbp, no bias / ReLU): the layer below's ReLU backward in the
 * epilogue, c = mask > 0 ? acc : 0 with mask in c's layout, and each row tile's column sums of c
 * in dbp [M / tile rows, N] (that layer's bias-gradient partials).
 * pad (mode 0, or null): {ph, pw, ih, iw, C}: x is the UNPADDED [B, ih, iw, C] tensor that the
 * rows index as if zero-padded by ph rows / pw columns on each side (the data gradient's padded
 * output gradient, never materialised; geom's qh, qw, gseg as for the padded one; tile 2, 3,
 * 5 or 6).
 * tile: 0 = 128 x 32, 2 = 128 x 64, 3 = 64 x 64, 5 = 128 x 128, 6 = 32 x 64 (mode 0); 1 =
 * 32 x 128, 3, 4 =
 * 64 x 128, 5 (mode 1); M, N multiples of it; K % 32 == 0, K / 32 >= splits.
 * tile 7 (mode 0, ABI 27): few rows (the rollout's batch) -- a 32-row tile per workgroup with its
 * K steps split over 8 waves and summed in wave order; N = 32 or 64, 32 | M, splits 1, no
 * out_geom / pad / mask; the same x6 products per K step, grouped differently over K (not the
 * other tiles' bits). w_planes (mode 0, else null; 16-B aligned, K % 8 == 0): w's three bf16
 * pieces [3, N, K] (ocppo_split_planes of w), read instead of splitting w in every workgroup
 * (the same pieces: the same bits). mbits_rows (ABI 28; mode 0 with relu, splits 1, no out_geom /
 * pad / mask, ldc == N, 32 | N, tiles 0, 2, 3, 5, 6; else null): the output's ReLU mask as a
 * row-major bitmask u32 [M, N / 32], bit n % 32 of word m N / 32 + n / 32 = !(c[m, n] <= 0) --
 * read by ocppo_relu_bias_grad_bits instead of the f32 output.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_conv_x6(ocppo_stream_t stream, int mode, const float* x, const int64_t* geom,
                            const float* w, int64_t ldw, float* c, int64_t ldc, int64_t M,
                            int64_t N, int64_t K, int64_t splits, const float* bias, int relu,
                            const int64_t* out_geom, int tile, float* out, const int64_t* pad,
                            const float* mask, float* dbp, const uint16_t* w_planes,
                            uint32_t* mbits_rows);

/* ---------------------------------------------------------------------------------------------
 * The first NatureCNN convolution straight from the rollout's u8 frame stacks (ppo_atari_oc.py:566
 * `b_obs[mb_inds]` -> NormalizeImg -> Conv2d, architectures/ppo.py:17-21), without the f32
 * minibatch copy: sample b's stack is row idx[b] of src u8 [rows, C, H, W] (NCHW); taps k = (c,
 * ky, kx) in nn.Conv2d's weight order (w [N, ldw] row-major, k-contiguous). The bytes are exact
 * bf16 operands; the products are divided by `divisor` (255.0: NormalizeImg's x / 255).
 *   mode 0: c[r, n] = act(sum_k u(r, k) w[n, k] / divisor + bias[n]), r < M = B OH OW (c [M, N])
 *   mode 1: out[m, n] = sum_r w[r ldw + m] u(r, n) / divisor (w = the output gradient [K, ldw],
 *           N = C KH KW taps, K = B OH OW rows); c = split partials [splits, M, N], summed in
 *           split order in f64 and divided once.
 * KW, W, stride multiples of 4; no padding; tile 0 / 2 (mode 0), 1 / 4 (mode 1) as ocppo_conv_x6's.
 * tile 7 (mode 0, ABI 25): each image's stack staged in LDS once, bitwise tile 0's output; needs
 * C = 4, 8 x 8 taps, stride 4, N = 32, 16 | OH OW, src 16-B aligned, 16 | C H W, 2 C H W <= 64 KB
 * (NatureCNN's first layer on 4 x 84 x 84 stacks); M a whole number of images, splits 1.
 * tile 8 (mode 1, ABI 25): the weight gradient with each image's stack staged in LDS once; needs
 * 4 x 84 x 84 stacks, 8 x 8 taps, stride 4, M = 32, K a whole number of images, a 16-B aligned
 * src; runs splits / 4 workgroups, each writing 4 partials into c [splits, M, N] (summed in
 * order in f64 and divided once, as the tile loop's); not the tile loop's summation order.
 * mbits (ABI 26, tiles 7 and 8 only, else null; 16-B aligned u32 [M] / [K]): tile 7 (with relu)
 * writes the output's ReLU mask, bit n of word r = c[r, n] > 0; tile 8 reads it and takes w as
 * the UNMASKED output gradient, zeroing it where the bit is clear (relu_bias_grad's ReLU
 * backward, ppo_atari_oc.py:603's loss.backward through nn.ReLU; the same products as on the
 * masked gradient). dbp / db (tile 8, both or neither): dbp workspace [splits, 32], db [32] the
 * (masked) gradient's per-channel sums = the layer's bias gradient (summed in order in f64).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_conv_x6_u8(ocppo_stream_t stream, int mode, const uint8_t* src,
                               const int64_t* idx, int64_t C, int64_t H, int64_t W, int64_t KH,
                               int64_t KW, int64_t stride, const float* w, int64_t ldw, float* c,
                               int64_t M, int64_t N, int64_t K, int64_t splits, const float* bias,
                               int relu, float divisor, int tile, float* out, uint32_t* mbits,
                               float* dbp, float* db);

/* ---------------------------------------------------------------------------------------------
 * The exact three-piece bf16 split ocppo_gemm_x6 forms in its K loop, done once per matrix: the
 * update's Linear weights (architectures/ppo.py:60-84) as the B operand of the forward (W [N, K],
 * trans 0) and of dX (W^T, trans 1), after every optimizer step (ppo_atari_oc.py:606) instead of
 * once per row tile and K step. Job i: src[i] f32 [rows, cols] (row stride ld) -> dst[i] three
 * dense bf16 planes [R', C'] (R' x C' = rows x cols, or cols x rows transposed), plane stride
 * R' C' elements; C' % 8 == 0, dst 16-B aligned; 1 <= n <= 8 jobs, one launch.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_split_planes(ocppo_stream_t stream, int n, const float* const* src,
                                 const int64_t* ld, const int64_t* rows, const int64_t* cols,
                                 const int* trans, void* const* dst);

/* ---------------------------------------------------------------------------------------------
 * Split-K combine of a weight gradient — replaces ATen's `sum(0)` after the batched (split-K)
 * weight-gradient GEMM dW = g'^T x the build runs inside `loss.backward()` (ppo_atari_oc.py:605)
 * for the Linear layers of architectures/ppo.py:60-84:
 *   out[i] = part[0*n + i] + part[1*n + i] + ... + part[(S-1)*n + i]   (left fold, split order,
 *            in double, rounded once to float)
 * part [S, n] f32, out [n] f32 (e.g. the parameter's view in the flat grad buffer); both 16-B
 * aligned, n % 4 == 0, S in {1, 2, 4, 8, 16}. Deterministic.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_sum_splits(ocppo_stream_t stream, const float* part, int64_t S, int64_t n,
                     float* out);
/* Split-K combine of a forward product with its epilogue — the decoder forward of the update
 * (architectures/ppo.py:77-80 inside ppo_atari_oc.py:566) as ocppo_gemm_x6 K splits:
 *   out[m, n] = act(sum_s part[s, m, n] + bias[n])   (part [S, M, N], out [M, N] f32 row-major;
 * the splits added in split order in double, rounded once, then + bias, then ReLU if relu —
 * torch._addmm_activation's order). bias [N] or NULL; 16-B aligned; N % 4 == 0. */
OCPPO_API int ocppo_sum_splits_act(ocppo_stream_t stream, const float* part, int64_t S, int64_t M,
                                   int64_t N, const float* bias, int relu, float* out);
OCPPO_API size_t ocppo_relu_bias_grad_workspace_bytes(int64_t R, int64_t N);
OCPPO_API int ocppo_relu_bias_grad(ocppo_stream_t stream, const float* g, const float* out,
                         float* gp, float* db, int64_t R, int64_t N, void* workspace,
                         size_t workspace_bytes);
/* ocppo_relu_bias_grad with the ReLU mask read from a row-major bitmask (ABI 28): gp[r, n] =
 * bit(r, n) ? g[r, n] : 0 with bit(r, n) = bit n % 32 of mbits[r N / 32 + n / 32] (the forward
 * epilogue's ocppo_conv_x6 mbits_rows: the same rule as out <= 0 -> 0), db = sum_r gp[r, n].
 * R >= 1, 32 | N <= 16384; g / gp 16-B aligned; workspace as ocppo_relu_bias_grad's. */
OCPPO_API int ocppo_relu_bias_grad_bits(ocppo_stream_t stream, const float* g,
                                        const uint32_t* mbits, float* gp, float* db, int64_t R,
                                        int64_t N, void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * First-layer backward in ONE pass — replaces threshold_backward + the split-K weight-gradient
 * GEMM + the bias sum autograd runs inside `loss.backward()` (ppo_atari_oc.py:605) for a
 * Linear(+ReLU) layer whose input needs no gradient and has K <= 16 features (the PPObj
 * encoder's first layer on the object frames, architectures/ppo.py:60-84):
 *   gp[r, n] = out[r, n] <= 0 ? 0 : g[r, n]   (g itself when out == NULL; gp is not written)
 *   db[n]    = sum_r gp[r, n]
 *   dw[n, k] = sum_r gp[r, n] * x[r, k]        (dw [N, K] row-major, nn.Linear.weight layout)
 * g/out [R, N] f32 row-major 16-B aligned, N % 4 == 0, N <= 16384; x [R, K] f32, row stride ldx;
 * 1 <= K <= 16. Workspace 256-B aligned, >= ocppo_relu_bias_wgrad_workspace_bytes(R, N, K),
 * ZEROED before its first use (tickets re-arm). Deterministic (fixed-order sums, f32 fma).
 * ------------------------------------------------------------------------------------------- */
/* Deferred form: gp as above, db left as per-chunk column partials partials[chunks, N]
 * (chunks = ocppo_relu_bias_grad_chunks(R, N)), summed later in chunk order by
 * ocppo_sum_splits_db in the launch that combines the layer's split-K weight gradient: no
 * cross-workgroup hand-off inside this launch. */
OCPPO_API int64_t ocppo_relu_bias_grad_chunks(int64_t R, int64_t N);
OCPPO_API int ocppo_relu_bias_grad_partial(ocppo_stream_t stream, const float* g, const float* out,
                                           float* gp, float* partials, int64_t R, int64_t N);
/* ocppo_sum_splits (out = sum of the S split-K blocks) + db[j] = sum_c db_partials[c, j] (a fixed
 * order) in one launch, both folds in double, rounded once; n, N multiples of 4, all pointers
 * 16-B aligned. */
OCPPO_API int ocppo_sum_splits_db(ocppo_stream_t stream, const float* part, int64_t S, int64_t n,
                                  float* out, const float* db_partials, int64_t chunks, int64_t N,
                                  float* db);
OCPPO_API size_t ocppo_relu_bias_wgrad_workspace_bytes(int64_t R, int64_t N, int64_t K);
OCPPO_API int ocppo_relu_bias_wgrad(ocppo_stream_t stream, const float* g, const float* out,
                          const float* x, int64_t ldx, float* dw, float* db, int64_t R,
                          int64_t N, int64_t K, void* workspace, size_t workspace_bytes);
/* Deferred form: the rows launch only; the finish (the tree over the row-range records that
 * writes dw and db) goes into *finish (R >= 1), to ride in the split-K combine the backward runs
 * next (ocppo_sum_splits_db_finish = ocppo_sum_splits_db, bitwise, plus the finish workgroups in
 * the same launch) or alone (ocppo_deferred_finish_run). Same results as ocppo_relu_bias_wgrad,
 * bitwise; run once, before anything reads dw / db or reuses the workspace. */
OCPPO_API int ocppo_relu_bias_wgrad_rows(ocppo_stream_t stream, const float* g, const float* out,
                                         const float* x, int64_t ldx, float* dw, float* db,
                                         int64_t R, int64_t N, int64_t K, void* workspace,
                                         size_t workspace_bytes, ocppo_deferred_finish_t* finish);
OCPPO_API int ocppo_sum_splits_db_finish(ocppo_stream_t stream, const float* part, int64_t S,
                                         int64_t n, float* out, const float* db_partials,
                                         int64_t chunks, int64_t N, float* db,
                                         const ocppo_deferred_finish_t* finish);

/* ---------------------------------------------------------------------------------------------
 * Policy heads + decoder ReLU backward in ONE pass — replaces, inside `loss.backward()`
 * (ppo_atari_oc.py:605), the actor / critic heads' dX, dW and db (architectures/ppo.py:81-84)
 * and the ReLU-backward + bias grad of the decoder layer feeding them. With
 * c[m] = (dlogits[m, 0..A), dvalue[m]) and W = [wa; wc] ([A+1, H]):
 *   dh[m, j] = sum_k c[m, k] W[k, j];  gp[m, j] = relu && h[m, j] <= 0 ? 0 : dh[m, j]
 *   db_h[j]  = sum_m gp[m, j]   (skipped when db_h == NULL)
 *   dwa[a, j] = sum_m dlogits[m, a] h[m, j];  dwc[j] = sum_m dvalue[m] h[m, j]
 *   dba[a] = sum_m dlogits[m, a];  dbc[0] = sum_m dvalue[m]
 * h / gp [M, H] f32 row-major 16-B aligned, H % 4 == 0, H <= 16384; dlogits [M, A] and dvalue
 * [M] contiguous, 1 <= A <= 7; wa [A, H], wc [H]. wc, dvalue, dwc and dbc may all be NULL: one
 * head only (K = A rows of W; e.g. the DQN Q head of dqn_atari_oc.py:378-392). Workspace 256-B
 * aligned, >=
 * ocppo_heads_bwd_workspace_bytes(M, H, A), ZEROED before first use. Deterministic.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_heads_bwd_workspace_bytes(int64_t M, int64_t H, int64_t A);
OCPPO_API int ocppo_heads_bwd(ocppo_stream_t stream, const float* h, const float* dlogits,
                    const float* dvalue, const float* wa, const float* wc, float* gp,
                    float* db_h, float* dwa, float* dwc, float* dba, float* dbc, int64_t M,
                    int64_t H, int64_t A, int relu, void* workspace, size_t workspace_bytes);

/* Two rollout Linear(+ReLU) layers in one launch (the PPObj encoder's first two layers on the
 * newest frame of every env, architectures/ppo.py:60-84, under torch.no_grad()):
 *   y[M, N2] = act2(act1(x[M, K1] @ w1[N1, K1]^T + b1) @ w2[N2, N1]^T + b2)
 * K1 <= 64, N1 % 16 == 0 and N1 <= 512; x row stride ldx (>= K1), y row stride ldy (>= N2);
 * w2 16-B aligned; b1 / b2 may be NULL. Same f32-MFMA arithmetic as ocppo_linear_act per layer. */
OCPPO_API int ocppo_linear2_act(ocppo_stream_t stream, const float* x, int64_t ldx, const float* w1,
                      const float* b1, const float* w2, const float* b2, float* y, int64_t ldy,
                      int64_t M, int64_t N1, int64_t N2, int64_t K1, int relu1, int relu2);

/* ---------------------------------------------------------------------------------------------
 * Frame-deduplicated PPObj minibatch encoder — replaces the per-slot encoder work inside
 * `agent.get_action_and_value(b_obs[mb_inds], ...)` of ppo_atari_oc.py:566 for the PPObj network
 * (architectures/ppo.py:60-84: Linear on the last dim of every stacked frame). Slot k of the
 * stored obs[t, n] ([T+1, N, W, F], step-major) is env n's frame of step max(t-(W-1)+k, r), r the
 * latest reset in (t-(W-1), t] (dones[r, n] = 1); its timeline id is u = (s+W-1)*N + n.
 *   frames_gather : x_out[c, :] = f32(frame uniq[c]) for the C (padded: id -1 -> zeros) distinct
 *                   frames of one minibatch;
 *   frames_expand : h_out[i, k, :] = enc[pos_of[u(perm[i], k)], :]  ([M, W, E], the decoder input);
 *   frames_scatter: denc[c, :] = sum of dh[i, k, :] over the uses of frame uniq[c] by the samples
 *                   of minibatch `mb` (inv[b] = position of sample b in the epoch permutation;
 *                   sample b belongs to minibatch inv[b] / M), fixed order -> deterministic.
 * W <= 16; dones [T+1, N] f32 with row r = "obs[r] starts an episode".
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_frames_gather(ocppo_stream_t stream, const void* obs, int obs_dtype, int64_t T,
                        int64_t N, int64_t W, int64_t F, const int32_t* uniq, int64_t C,
                        float* x_out);
OCPPO_API int ocppo_frames_expand(ocppo_stream_t stream, const float* enc, int64_t C, int64_t E,
                        const int32_t* pos_of, const int64_t* perm, int64_t M, const float* dones,
                        int64_t T, int64_t N, int64_t W, float* h_out);
/* frames_expand's source rows only: idx[i, k] = pos_of[u(perm[i], k)] ([M, W] int32), the row
 * table ocppo_gemm_x6's gathered operands read (the decoder's input never materialised). */
OCPPO_API int ocppo_frames_expand_index(ocppo_stream_t stream, const int32_t* pos_of,
                                        const int64_t* perm, int64_t M, const float* dones,
                                        int64_t T, int64_t N, int64_t W, int32_t* idx);
OCPPO_API int ocppo_frames_scatter(ocppo_stream_t stream, const float* dh, int64_t M, int64_t E,
                         const int32_t* uniq, int64_t C, const int32_t* inv, int64_t mb,
                         const float* dones, int64_t T, int64_t N, int64_t W, float* denc_out);
/* frames_scatter with the encoder's last ReLU backward fused in (the update's `loss.backward()`
 * through architectures/ppo.py:60-84's last Linear->ReLU, ppo_atari_oc.py:605):
 *   gp_out[c, :] = out[c, :] <= 0 ? 0 : denc[c, :]   (out = that layer's ReLU output [C, E];
 *                                                     NULL: no mask, gp_out = denc)
 *   dbp[g, :] = sum of gp_out rows of chunk g (ocppo_frames_scatter_chunks(C) chunks of 16 frames,
 *               summed later in chunk order by ocppo_sum_splits_db); NULL: not written.
 * mbits (NULL: none): the mask as the row-major ReLU bitmask ocppo_gemm_x6 wrote for `out`
 * (relu | OCPPO_X6_MBITS_ROWS, [C][E / 32] words, E % 32 == 0) instead of reading out (then
 * ignored): 1 bit instead of 4 B per element, the same gp_out.
 * E % 4 == 0, dh / out / gp_out / dbp 16-B aligned. Same per-frame sums as frames_scatter. */
OCPPO_API int64_t ocppo_frames_scatter_chunks(int64_t C);
OCPPO_API int ocppo_frames_scatter_relu(ocppo_stream_t stream, const float* dh, int64_t M,
                                        int64_t E, const int32_t* uniq, int64_t C,
                                        const int32_t* inv, int64_t mb, const float* dones,
                                        int64_t T, int64_t N, int64_t W, const float* out,
                                        const uint32_t* mbits, float* gp_out, float* dbp);
/* frames_gather + the encoder's first Linear(+ReLU) in one pass (the update's first encoder layer
 * over the distinct frames, architectures/ppo.py:60-84 on b_obs[mb_inds], ppo_atari_oc.py:566) (F <= 16, N1 % 4 == 0,
 * N1 <= 1024): x_out [C, F] = the gathered frames (as frames_gather),
 * h_out [C, N1] = act(x W^T + b)
 * (w [N1, F], b [N1] or NULL; products summed over f in order, then + b, then ReLU if relu).  idx_out (NULL: none): also ocppo_frames_expand_index(pos_of, perm, M, dones, T, N, W) into
 * idx_out [M, W], made by extra workgroups of the same launch (the row table the update's gathered
 * decoder reads; one launch instead of two). */
OCPPO_API int ocppo_frames_gather_linear(ocppo_stream_t stream, const void* obs, int obs_dtype,
                                         int64_t T, int64_t N, int64_t W, int64_t F,
                                         const int32_t* uniq, int64_t C, const float* w,
                                         const float* b, int64_t N1, int relu, float* x_out,
                                         float* h_out, const int32_t* pos_of,
                                         const int64_t* perm, int64_t M, const float* dones,
                                         int32_t* idx_out);

/* ---------------------------------------------------------------------------------------------
 * Minibatch gather — replaces `b_obs[mb_inds]` of ppo_atari_oc.py:566-567:
 *   dst[i, :] = f32(src[idx[i], :]),  src [B, R] of dtype src_dtype, dst [M, R] f32.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_gather_rows(ocppo_stream_t stream, const void* src, int src_dtype, const int64_t* idx,
                      int64_t M, int64_t R, float* dst);

/* The same gather into channels-last rows (the NHWC input of a channels_last NatureCNN):
 *   dst[i, p, c] = f32(src[idx[i], c, p]) (/ 255 with OCPPO_NET_SCALE_255 in net_flags, as in
 *   ocppo_rollout_store),  src [B, C, P] (C stacked frames of P pixels), dst [M, P, C] f32,
 *   16-B aligned. */
OCPPO_API int ocppo_gather_rows_cl(ocppo_stream_t stream, const void* src, int src_dtype,
                         const int64_t* idx, int64_t M, int64_t C, int64_t P, float* dst,
                         int net_flags);

/* ---------------------------------------------------------------------------------------------
 * Reward normalisation of SB3 VecNormalize(norm_obs=False, norm_reward=True) as wrapped at
 * ppo_atari_oc.py:414 (stable-baselines3 2.0.0, not in the reference tree), on device in f64:
 *   ret = ret*gamma + r;  rms.update(ret) (batch mean/var over N, Chan merge);
 *   r' = clip(r / sqrt(rms.var + epsilon), -clip, clip);  ret[done] = 0
 *   ret_state : [N] f64;  rms_state : [3] f64 = {mean, var, count} (init {0, 1, 1e-4})
 *   reward_out : [N] f32 (may alias nothing; typically &rewards[t*N])
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_vecnorm_reward(ocppo_stream_t stream, const float* reward, const float* done, int64_t N,
                         double gamma, double epsilon, double clip_reward, double* ret_state,
                         double* rms_state, float* reward_out);

/* Rollout store and VecNormalize reward normalisation in ONE launch (one workgroup normalises the
 * N rewards, the others store): ocppo_rollout_store (reward_out unused) + ocppo_vecnorm_reward.
 * reward_out (normalised, typically &rewards[t*N]) must not alias reward. */
OCPPO_API int ocppo_rollout_store_vecnorm(ocppo_stream_t stream, const void* frame, int frame_dtype,
                                          const float* reward, const float* done, int64_t N,
                                          int64_t W, int64_t D, const void* prev_obs, void* obs_out,
                                          int obs_dtype, float* net_obs, float* done_out,
                                          double gamma, double epsilon, double clip_reward,
                                          double* ret_state, double* rms_state, float* reward_out, int net_flags,
                                          const void* reset_prev);

/* ---------------------------------------------------------------------------------------------
 * DQN (config 5, dqn_atari_oc.py) — HBM replay buffer with stable-baselines3 2.0.0
 * ReplayBuffer(optimize_memory_usage=True, handle_timeout_termination=False) semantics
 * (:317-325 add at :369, sample at :377), epsilon-greedy (:345-350) and the fused TD target +
 * MSE loss forward/backward (:378-382). Replay layout: obs [size, E, D] (storage dtype),
 * actions [size, E] i64, rewards/dones [size, E] f32, state = device i64 {pos, full} (zeroed).
 * Sampling law = SB3's (indices in [0, pos) or (randint(1, size) + pos) % size once full, env
 * index uniform); random bits from a counter-based stream (device counter, +1 per call), not numpy.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_replay_workspace_bytes(void);
OCPPO_API int ocppo_replay_add(ocppo_stream_t stream, const void* obs, const void* next_obs,
                               int obs_dtype, const int64_t* actions, const float* rewards,
                               const float* dones, int64_t E, int64_t D, int64_t* state,
                               int64_t size, void* rb_obs, int rb_dtype, int64_t* rb_actions,
                               float* rb_rewards, float* rb_dones, void* workspace);
/* obs_out / next_obs_out : [B, D] f32; indices_out : [B, 2] {slot, env} or NULL */
OCPPO_API int ocppo_replay_sample(ocppo_stream_t stream, uint64_t seed, int64_t* counter,
                                  const int64_t* state, int64_t size, int64_t E, int64_t D,
                                  const void* rb_obs, int rb_dtype, const int64_t* rb_actions,
                                  const float* rb_rewards, const float* rb_dones, int64_t B,
                                  float* obs_out, float* next_obs_out, int64_t* actions_out,
                                  float* rewards_out, float* dones_out, int64_t* indices_out);
/* global step t = *step + step_offset (step : device i64, so a captured chunk of env steps
 * reads one counter advanced once per chunk); epsilon_out : device f32 or NULL */
/* the Q head (q = hidden Wq^T + bq, hidden [E, H] H a multiple of 256 <= 1024, wq [A, H], A <= 8)
 * and ocppo_epsilon_greedy on it in one launch (same coin, argmax rule and random action);
 * q_out [E, A] or NULL */
OCPPO_API int ocppo_q_head_epsilon_greedy(ocppo_stream_t stream, const float* hidden, int64_t E,
                                          int64_t H, const float* wq, const float* bq, int64_t A,
                                          uint64_t seed, const int64_t* step, int64_t step_offset,
                                          double start_e, double end_e, double duration,
                                          int64_t* actions, float* epsilon_out, float* q_out);
/* One acting step of the DQN loop (dqn_atari_oc.py:345-372) in ONE launch, for the object-frame
 * synthetic env (ocppo_synth_env_step's, seed env_seed, step id *env_step_base + env_step_offset)
 * and E <= 64 envs: ocppo_q_head_epsilon_greedy's actions (actions, epsilon_out), the env step on
 * them (frame [E, D] f32, env_reward / env_done [E], ep_state [E, 5] or NULL), the frame-stack
 * store of ocppo_rollout_store (prev_obs -> obs_out [E, W, D] in obs_dtype, net_obs f32 or NULL,
 * done_out; reward_out = the reward, or with vecnorm != 0 ocppo_rollout_store_vecnorm's normalised
 * reward and (ret_state, rms_state) update) and ocppo_replay_add of (prev_obs, obs_out, actions,
 * reward_out, done_out) into a replay of obs_dtype (rb_obs [rb_size, E, W * D], rb_state {pos,
 * full}). advance != 0 then adds advance to *step and *env_step_base (both read before: the
 * last env step of a captured chunk moves the chunk's counters, replacing two launches). Every
 * output is bitwise the four launches'. */
OCPPO_API int ocppo_dqn_act_step(
    ocppo_stream_t stream, const float* hidden, int64_t E, int64_t H, const float* wq,
    const float* bq, int64_t A, uint64_t seed, int64_t* step, int64_t step_offset,
    double start_e, double end_e, double duration, int64_t* actions, float* epsilon_out,
    uint64_t env_seed, int64_t* env_step_base, int64_t env_step_offset, int64_t D,
    float* frame, float* env_reward, float* env_done, float* ep_state, int64_t W,
    const void* prev_obs, void* obs_out, int obs_dtype, float* net_obs, float* done_out,
    float* reward_out, int vecnorm, double vn_gamma, double vn_epsilon, double vn_clip,
    double* ret_state, double* rms_state, int64_t* rb_state, int64_t rb_size, void* rb_obs,
    int64_t* rb_actions, float* rb_rewards, float* rb_dones, int64_t advance);
OCPPO_API int ocppo_epsilon_greedy(ocppo_stream_t stream, const float* q, int64_t E, int64_t A,
                                   uint64_t seed, const int64_t* step, int64_t step_offset,
                                   double start_e, double end_e, double duration,
                                   int64_t* actions, float* epsilon_out);
/* q, q_next : [B, A] f32 (q_network(obs), target_network(next_obs)); dq : [B, A] = d loss / d q;
 * stats : [2] = {td_loss, mean(old_val)} (losses/td_loss, losses/q_values of :385-386)
 *   td = r + (f32(gamma) * max_a q_next) * (1 - d);  old = q[b, a_b];  loss = mean((td - old)^2) */
OCPPO_API int ocppo_td_loss_fwd_bwd(ocppo_stream_t stream, const float* q, const float* q_next,
                                    const int64_t* actions, const float* rewards,
                                    const float* dones, int64_t B, int64_t A, double gamma,
                                    float* dq, float* stats);

/* ---------------------------------------------------------------------------------------------
 * C51 (cleanrl/c51_atari_oc.py, QNetwork_C51 of architectures/dqn.py:36-72). The network emits
 * [rows, A * N] logits, N atoms per action; `atoms` [N] f32 is the module's registered buffer
 * (torch.linspace(v_min, v_max, N): its spacing atoms[1] - atoms[0] is read from the buffer, for
 * linspace(-10, 10, 51) that is 0.39999962, not 0.4). 2 <= N <= 128, 1 <= A <= 18.
 *
 * ocppo_c51_loss_fwd_bwd: the train step's loss block :339-359 and its backward w.r.t. the online
 * logits as ONE launch (one workgroup, no float atomics, no workspace, bitwise repeatable,
 * graph-replay safe: every output is fully rewritten).
 *   logits      : [B, A * N] q_network on observations;  logits_next : target_network on
 *                 next_observations;  actions : [B] i64;  rewards, dones : [B] f32
 *   next action = first argmax_a sum_k softmax(logits_next[b, a])_k * atoms_k, p' its pmf
 *   next_atoms  = r + (f32(gamma) * atoms) * (1 - d); tz = clamp(next_atoms, v_min, v_max);
 *                 b = (tz - v_min) / delta_z; l = floor(b), u = ceil(b) clamped to [0, N - 1];
 *                 target[l] += (u + (l == u) - b) * p' for every source atom in ascending order,
 *                 then target[u] += (b - l) * p' likewise (index_add_'s CPU order)
 *   p = softmax(logits[b, a_b]);  loss = mean_b(-sum_k target_k * log(clamp(p_k, 1e-5, 1 - 1e-5)))
 *   dlogits     : [B, A * N] = d loss / d logits (through the clamp: zero where p is outside
 *                 [1e-5, 1 - 1e-5]; through the softmax; scaled by 1 / B); rows of the actions
 *                 not taken are written as zeros
 *   stats       : [2] = {losses/loss, losses/q_values = mean_b sum_k p_k * atoms_k}
 *   target_pmfs : [B, N] or NULL;  next_action : [B] i64 or NULL
 *
 * ocppo_c51_epsilon_greedy: q[e, a] = sum_k softmax(logits[e, a])_k * atoms_k (get_action) and
 * ocppo_epsilon_greedy's choice on it in one launch (same coin, random action and first-maximum
 * rule; same arguments).  q_out : [E, A] or NULL.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_c51_loss_fwd_bwd(ocppo_stream_t stream, const float* logits,
                                     const float* logits_next, const float* atoms,
                                     const int64_t* actions, const float* rewards,
                                     const float* dones, int64_t B, int64_t A, int64_t N,
                                     double gamma, double v_min, double v_max, float* dlogits,
                                     float* stats, float* target_pmfs, int64_t* next_action);
OCPPO_API int ocppo_c51_epsilon_greedy(ocppo_stream_t stream, const float* logits,
                                       const float* atoms, int64_t E, int64_t A, int64_t N,
                                       uint64_t seed, const int64_t* step, int64_t step_offset,
                                       double start_e, double end_e, double duration,
                                       int64_t* actions, float* epsilon_out, float* q_out);

/* ---------------------------------------------------------------------------------------------
 * Rainbow (cleanrl/rainbow_atari_oc.py; ABI 30), part 1: the prioritized n-step replay
 * (SumSegmentTree :338-369 + PrioritizedReplayBuffer :395-499) with all of its state in HBM, for
 * num_envs == 1 as the script asserts (:513). The reference walks a numpy sum tree in Python, one
 * host step per sampled element and per updated priority, and copies loss_per_sample to the host
 * on every train step (:704); these entries read and write device memory only, allocate nothing,
 * and replay from a hipGraph. The MinSegmentTree (:373-392) is written and never read in the
 * reference (min() has no caller), so it does not exist here.
 *   rb_obs, rb_next_obs : [capacity, D] in rb_dtype (both rows are stored, as :446-447: the
 *                 n-step next observation is not the next slot's)
 *   rb_actions i64, rb_rewards f32, rb_dones f32 (0 / 1) : [capacity]
 *   tree        : f32 [2 * capacity - 1], root 0, children of i at 2i + 1 and 2i + 2, the leaf of
 *                 slot k at k + capacity - 1; capacity >= 2, any value
 *   state       : i64 [8] = {pos, size, max_priority (f32 in the low 4 bytes; initialise to
 *                 1.0f), n-step ring fill, n-step ring head, 0, 0, 0}
 *   ring_*      : the deque(maxlen=n_step) of :420: ring_obs / ring_next_obs [n_step, D] in
 *                 rb_dtype, ring_actions i64, ring_rewards f32, ring_dones f32 [n_step]; n_step <= 8
 *   workspace   : ocppo_per_workspace_bytes() bytes, zeroed once
 *
 * ocppo_per_add (:435-460 with _get_n_step_info :422-433), one launch: pushes (obs, action,
 * reward, next_obs, done) of the single env into the ring; with fewer than n_step entries nothing
 * else is written. Otherwise the row at pos receives the first entry's obs and action, the
 * n-step reward sum_i gamma_pows[i] * r_i accumulated term by term in f64 up to and including the
 * first done entry (the loop passes float64 reward arrays) and rounded to f32 on the store, and
 * the next obs and done of the first done entry, or else of the last; its leaf becomes
 * max_priority ** alpha and its ancestors are recomputed; pos and size advance; a done row
 * clears the ring (so the n - 1 starts at the end of an episode are dropped, as in the
 * reference). gamma_pows is HOST memory: the n_step values gamma ** i formed in Python.
 *
 * ocppo_per_update_priorities (:492-499), one launch: p = |loss_per_sample| + f32(eps);
 * max_priority = max(max_priority, max p); leaf[indices[i]] = p_i ** alpha (of a repeated index
 * the last occurrence, the reference's order); then every ancestor of a touched leaf is
 * recomputed as f32(left + right), level by level from the deepest, which is what the
 * reference's sequential updates leave. B <= 1024; an index outside [0, capacity) is ignored.
 *
 * ocppo_per_sample (:462-490), two launches (indices + weights, row gather): segment =
 * total / B in f32; upperbound_i uniform in [segment * i, segment * (i + 1)) in f64 from the
 * counter-based stream of (seed, counter[0]), or upperbounds_in[i] when given; index =
 * retrieve(upperbound) (:359-369) in f64 against the f32 nodes; probs = the leaf; weights =
 * (size * probs / total) ** -beta divided by the batch maximum, with beta = min(1, beta0 +
 * (step[0] + step_offset) * (1 - beta0) / total_timesteps) (:611-614; beta0 when step is NULL).
 * counter[0] advances by one.
 *   obs_out, next_obs_out : [B, D] f32;  actions_out i64, rewards_out, dones_out, weights_out
 *   f32, indices_out i64 : [B];  probs_out f32 [B], upperbounds_out f64 [B], beta_out f32 [1]
 *   or NULL.  B <= 1024.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_per_workspace_bytes(void);
OCPPO_API int ocppo_per_add(ocppo_stream_t stream, const void* obs, const void* next_obs,
                            int obs_dtype, const int64_t* action, const float* reward,
                            const float* done, int64_t D, int64_t n_step,
                            const double* gamma_pows, double alpha, int64_t* state,
                            int64_t capacity, void* rb_obs, void* rb_next_obs, int rb_dtype,
                            int64_t* rb_actions, float* rb_rewards, float* rb_dones, float* tree,
                            void* ring_obs, void* ring_next_obs, int64_t* ring_actions,
                            float* ring_rewards, float* ring_dones, void* workspace);
OCPPO_API int ocppo_per_update_priorities(ocppo_stream_t stream, const int64_t* indices,
                                          const float* loss_per_sample, int64_t B, double eps,
                                          double alpha, int64_t* state, int64_t capacity,
                                          float* tree);
OCPPO_API int ocppo_per_sample(ocppo_stream_t stream, uint64_t seed, int64_t* counter,
                               const int64_t* state, const int64_t* step, int64_t step_offset,
                               double beta0, double total_timesteps, int64_t capacity, int64_t D,
                               const void* rb_obs, const void* rb_next_obs, int rb_dtype,
                               const int64_t* rb_actions, const float* rb_rewards,
                               const float* rb_dones, const float* tree, int64_t B,
                               const double* upperbounds_in, float* obs_out, float* next_obs_out,
                               int64_t* actions_out, float* rewards_out, float* dones_out,
                               int64_t* indices_out, float* weights_out, float* probs_out,
                               double* upperbounds_out, float* beta_out);

/* ---------------------------------------------------------------------------------------------
 * Rainbow, part 2: the train step's loss block :655-701 and its backward as ONE launch, and the
 * acting step :617-620. The networks (NoisyDuelingDistributionalNetwork, :283-327, and
 * architectures/rainbow.py's NoisyDuelingDistributionalPPObj) end in
 *   q_atoms = value + advantage - advantage.mean(dim=1, keepdim=True); softmax(q_atoms, dim=2)
 * so these entries take the RAW head outputs value [rows, N] and advantage [rows, A * N] and form
 * the dueling combine and the softmax themselves. support [N] is the registered buffer.
 * 2 <= N <= 128, 1 <= A <= 18.
 *
 * ocppo_rainbow_loss_fwd_bwd (one workgroup, no float atomics, no workspace, bitwise repeatable,
 * graph-replay safe: every output is fully rewritten):
 *   value, advantage                     : q_network on observations
 *   value/advantage_next_online          : q_network on next_observations (double Q, :664-667)
 *   value/advantage_next_target          : target_network on next_observations (:657)
 *   actions [B] i64; rewards, dones, weights [B] f32
 *   gamma_n     : args.gamma ** args.n_step, formed by the host (:672)
 *   best action = first argmax_a of the ONLINE net's expected value; p' = the TARGET net's pmf
 *                 at that action (:667-669)
 *   next_atoms  = r + (f32(gamma_n) * support) * (1 - d); tz = clamp(next_atoms, v_min, v_max);
 *                 b = (tz - v_min) / f32(delta_z), delta_z = (v_max - v_min) / (N - 1) as the
 *                 modules' __init__ forms it (NOT the buffer's spacing); l = floor(b), u =
 *                 ceil(b), clamped to [0, N - 1]; target[l] += (u + (l == b) - b) * p' for every
 *                 source atom in ascending order, then target[u] += (b - l) * p' likewise
 *                 (:678-692, index_add_'s CPU order)
 *   p = the online pmf of the taken action; loss_per_sample_b = -sum_k target_k *
 *                 log(clamp(p_k, 1e-5, 1 - 1e-5)); loss = mean_b(loss_per_sample_b * weights_b)
 *   dvalue [B, N], dadvantage [B, A * N] : d loss / d (value, advantage) through the clamp mask,
 *                 the softmax and the dueling combine; rows of actions not taken receive the
 *                 -1 / A share only; every element is written
 *   loss_per_sample [B] (the new priorities, :704-705)
 *   stats       : [2] = {losses/td_loss, losses/q_values = mean_b sum_k p_k * support_k} (:708-713)
 *   target_pmfs : [B, N] or NULL;  best_actions : [B] i64 or NULL
 *
 * ocppo_rainbow_greedy (:617-620): actions[e] = first argmax_a sum_k q_dist[e, a, k] * support_k,
 * one wave per env, no epsilon.  q_out : [E, A] or NULL.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_rainbow_loss_fwd_bwd(
    ocppo_stream_t stream, const float* value, const float* advantage,
    const float* value_next_online, const float* advantage_next_online,
    const float* value_next_target, const float* advantage_next_target, const float* support,
    const int64_t* actions, const float* rewards, const float* dones, const float* weights,
    int64_t B, int64_t A, int64_t N, double gamma_n, double v_min, double v_max, float* dvalue,
    float* dadvantage, float* loss_per_sample, float* stats, float* target_pmfs,
    int64_t* best_actions);
OCPPO_API int ocppo_rainbow_greedy(ocppo_stream_t stream, const float* value,
                                   const float* advantage, const float* support, int64_t E,
                                   int64_t A, int64_t N, int64_t* actions, float* q_out);

/* ---------------------------------------------------------------------------------------------
 * Synthetic device-resident env (benchmark / test harness; ALE and OCAtari are not available).
 * Not a reference component. Counter-based hashing of (seed, env, step) gives reproducible
 * frames: object mode x~U{0..159}, y~U{0..209}, w,h~U{1..16} per 4-feature object; pixel mode
 * 84x84 u8 with ~90% zeros; reward = +-1 w.p. 0.005 each; done w.p. 1/3500 (Pong-v5 episode
 * lengths). `actions` shift the first object's y so the env reacts to the policy.
 *   frame_out : [N, D] (f32 for obj, u8 for pixels); reward_out, done_out : [N] f32
 *   step_base : device int64 read at run time (graph replays advance it), the hashed step id is
 *               step_base[0] + step_offset
 *   ep_state  : [N, 5] f32 = {running return, running length, finished-episode return sum,
 *               finished-episode length sum, finished-episode count}, updated in place (may be
 *               NULL); the RecordEpisodeStatistics counters behind ppo_atari_oc.py:516-529
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_synth_env_step(ocppo_stream_t stream, uint64_t seed, const int64_t* step_base,
                         int64_t step_offset, const int64_t* actions, int64_t N, int64_t D, int pixel_mode,
                         void* frame_out, float* reward_out, float* done_out, float* ep_state);

/* The rollout policy head (ocppo_policy_head_sample, one wave per env) with the synthetic env's
 * object-frame step fused behind it: the wave that sampled env n's action writes env n's next
 * frame / reward / done / episode counters exactly as ocppo_synth_env_step(pixel_mode 0) would
 * from action_out -- one launch for architectures/ppo.py:89-95 + the env step of
 * ppo_atari_oc.py:506-511. Entropy and logits are not produced.
 *   N <= 3072 (<= 2048 when H > 512), H in {256, 512, 768, 1024}, A <= 7, D <= 4096; hidden and
 *   the head weights 16-B aligned (else OCPPO_ERR_INVALID: use the two launches). */
OCPPO_API int ocppo_policy_head_env_step(ocppo_stream_t stream, const float* hidden, int64_t N,
                                         int64_t H, const float* w_actor, const float* b_actor,
                                         const float* w_critic, const float* b_critic,
                                         float* noise, const int64_t* philox_state,
                                         int64_t philox_offset, int64_t philox_stride,
                                         int64_t A, int64_t* action_out,
                                         float* logprob_out, float* value_out, uint64_t seed,
                                         const int64_t* step_base, int64_t step_offset, int64_t D,
                                         float* frame_out, float* reward_out, float* done_out,
                                         float* ep_state);

/* ---------------------------------------------------------------------------------------------
 * Policy heads forward + fused PPO loss + heads backward in one pass over the decoder output
 * (ppo_atari_oc.py:566-605 from h = relu(z) on; architectures/ppo.py:81-84):
 *   logits = h Wa^T + ba, value = h Wc^T + bc; the loss of ocppo_ppo_loss_fwd_bwd on the prepared
 *   (minibatch-order, contiguous) records mb_* [M] with adv_stats [2] (required when norm_adv);
 *   c = (d loss / d logits, d loss / d value);  gp [M, H] = (h <= 0 ? 0 : c W), W = [Wa; Wc];
 *   db_h [H] = sum_m gp (the decoder bias grad, may be NULL); dwa [A, H], dwc [H], dba [A],
 *   dbc [1] the heads' grads; stats [9] as ocppo_ppo_loss_fwd_bwd; dlogits [M, A] / dvalue [M]
 *   optional (both NULL or both set).
 * H in {64, 128, 256, 512} (else OCPPO_E_INVALID), 1 <= A <= 7; h, gp, Wa, Wc 16-B aligned. Two
 * launches: a fixed grid of at most 512 workgroups, each owning a contiguous row range and writing
 * ONE partial record, then a fixed-shape tree over the records: deterministic; workspace =
 * ocppo_heads_loss_workspace_bytes(M, H, A), needs no zeroing.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_heads_loss_workspace_bytes(int64_t M, int64_t H, int64_t A);
OCPPO_API int ocppo_heads_loss_fwd_bwd(ocppo_stream_t stream, const float* h, int64_t M, int64_t H,
                                       const float* w_actor, const float* b_actor,
                                       const float* w_critic, const float* b_critic, int64_t A,
                                       const int64_t* mb_actions, const float* mb_logprobs,
                                       const float* mb_advantages, const float* mb_returns,
                                       const float* mb_values, const float* adv_stats,
                                       double clip_coef, double ent_coef, double vf_coef,
                                       int norm_adv, int clip_vloss, float* gp, float* db_h,
                                       float* dwa, float* dwc, float* dba, float* dbc,
                                       float* stats, float* dlogits, float* dvalue,
                                       void* workspace, size_t workspace_bytes);
/* Deferred form: ocppo_heads_loss_rows launches the rows kernel only and writes the finish (the
 * tree over the records, which writes db_h, dwa, dwc, dba, dbc and stats) into *finish, a plain
 * host record; the caller runs it later on the same stream, before anything reads those outputs
 * and before the workspace is reused: folded into the split-K combine the backward runs next
 * (ocppo_sum_splits_finish = ocppo_sum_splits, bitwise, plus the finish workgroups in the same
 * launch) or alone (ocppo_deferred_finish_run). Same results as ocppo_heads_loss_fwd_bwd, bitwise.
 * The record holds device pointers only; it may be copied and run once per rows launch. */
OCPPO_API int ocppo_heads_loss_rows(ocppo_stream_t stream, const float* h, int64_t M, int64_t H,
                                    const float* w_actor, const float* b_actor,
                                    const float* w_critic, const float* b_critic, int64_t A,
                                    const int64_t* mb_actions, const float* mb_logprobs,
                                    const float* mb_advantages, const float* mb_returns,
                                    const float* mb_values, const float* adv_stats,
                                    double clip_coef, double ent_coef, double vf_coef,
                                    int norm_adv, int clip_vloss, float* gp, float* db_h,
                                    float* dwa, float* dwc, float* dba, float* dbc, float* stats,
                                    float* dlogits, float* dvalue, void* workspace,
                                    size_t workspace_bytes, ocppo_deferred_finish_t* finish);
OCPPO_API int ocppo_sum_splits_finish(ocppo_stream_t stream, const float* part, int64_t S,
                                      int64_t n, float* out, const ocppo_deferred_finish_t* finish);
OCPPO_API int ocppo_deferred_finish_run(ocppo_stream_t stream,
                                        const ocppo_deferred_finish_t* finish);

/* ---------------------------------------------------------------------------------------------
 * Rollout fusions of the PPObj frame-encoding cache path (ppo_atari_oc.py:502-514 + :506 with
 * architectures/ppo.py:60-95): per env step the launches are [store of step t-1 + the first two
 * encoder layers of the newest frame] -> middle encoder layers -> [last encoder layer + cache
 * shift] -> decoder -> fused policy head.
 *
 * ocppo_linear_cache_shift: fresh = act(x W^T + b) (as ocppo_linear_act, x [M, K], W [N, K]) is
 *   not stored; instead enc [M, W, N] (the frame-encoding cache) is shifted with it:
 *   enc[m, w] = done[m] != 0 || w == W-1 ? fresh[m] : enc[m, w+1]  (ocppo_frame_cache_shift's rule;
 *   done [M] f32 or NULL).
 * ocppo_store_linear2: ocppo_rollout_store (vecnorm = 0; reward_out = the raw reward row) or
 *   ocppo_rollout_store_vecnorm (vecnorm = 1) of frame [N, D] f32 into obs_out / net_obs /
 *   reward_out / done_out, AND y [N, N2] (row stride ldy) = relu(relu(f W1^T + b1) W2^T + b2) of
 *   the newest frames f = frame seen through obs_dtype (OCPPO_F32 or OCPPO_BF16 round trip), as
 *   ocppo_linear2_act (D <= 64, N1 % 16 == 0, N1 <= 512, W2 16-B aligned), in one launch.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_linear_cache_shift(ocppo_stream_t stream, const float* x, int64_t ldx,
                                       const float* w, const float* b, float* enc,
                                       const float* done, int64_t M, int64_t N, int64_t K,
                                       int64_t W, int relu);
/* Ring form of the frame-encoding cache (no shift): the W physical slots of enc [M, W, N] hold the
 * W logical frames (oldest .. newest) rotated by a per-step offset r, logical slot w at physical
 * (w + r) mod W.
 * ocppo_linear_cache_ring: fresh = act(x W^T + b) overwrites physical slot `slot` only (the
 *   oldest frame's: at rollout step t the newest frame goes to slot (t - 1) mod W), or every
 *   slot of env m when done[m] != 0 (a reset fills the stack with the new frame). No old slot is
 *   read. done [M] f32 or NULL.
 * ocppo_linear_act_ring: ocppo_linear_act whose x rows are W = K / seg segments of seg floats
 *   stored rotated: logical segment s at physical segment (s + rot) mod W (seg a power of two >= 32,
 *   K % seg == 0, x / w 16-B aligned, ldx % 4 == 0). Products and summation order are those of
 *   the logical layout: the decoder (architectures/ppo.py:74-78: Flatten + Linear over the W
 *   frame encodings) on the ring gives bit for bit what it gives on the shifted cache. */
OCPPO_API int ocppo_linear_cache_ring(ocppo_stream_t stream, const float* x, int64_t ldx,
                                      const float* w, const float* b, float* enc,
                                      const float* done, int64_t M, int64_t N, int64_t K,
                                      int64_t W, int64_t slot, int relu);
OCPPO_API int ocppo_linear_act_ring(ocppo_stream_t stream, const float* x, int64_t ldx,
                                    const float* w, const float* b, float* y, int64_t ldy,
                                    int64_t M, int64_t N, int64_t K, int64_t seg, int64_t rot,
                                    int relu);
/* ---------------------------------------------------------------------------------------------
 * NHWC Conv2d (no padding, no dilation, groups 1) + bias + optional ReLU for the rollout
 * forward of the NatureCNN trunk (architectures/ppo.py:20-31 at ppo_atari_oc.py:506):
 *   y[b, oy, ox, co] = act(bias[co] + sum_{ky,kx,ci} x[b, oy*s+ky, ox*s+kx, ci] w[co, ky, kx, ci])
 * x [B, H, W, Cin] f32 (a channels_last NCHW tensor's memory), w [Cout, KH, KW, Cin] (a
 * channels_last conv weight's memory), bias [Cout] or NULL, y [B, OH, OW, Cout] f32, OH =
 * (H - KH) / s + 1. Cin a power of two >= 4, KH*KW*Cin % 16 == 0, x / w 16-B aligned.
 * Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_conv2d_act(ocppo_stream_t stream, const float* x, int64_t B, int64_t H,
                               int64_t W, int64_t Cin, const float* w, const float* b,
                               int64_t Cout, int64_t KH, int64_t KW, int64_t stride, float* y,
                               int relu);
OCPPO_API int ocppo_store_linear2(ocppo_stream_t stream, const float* frame, const float* reward,
                                  const float* done, int64_t N, int64_t W, int64_t D,
                                  const void* prev_obs, void* obs_out, int obs_dtype,
                                  float* net_obs, float* reward_out, float* done_out, int vecnorm,
                                  double gamma, double epsilon, double clip_reward,
                                  double* ret_state, double* rms_state, const float* w1,
                                  const float* b1, const float* w2, const float* b2, float* y,
                                  int64_t ldy, int64_t N1, int64_t N2);
/* ocppo_policy_head_env_step (noise read, H = 256 or 512, object frames) followed by
 * ocppo_store_linear2 of the frames / rewards / dones it produced, in ONE launch: the rollout's
 * [head + env step of step t-1, store into slot t, first two encoder layers of step t]. Every
 * workgroup that needs env row n's action and frame recomputes them (the head is A+1 dots of H
 * per row); one owner workgroup per 16 rows writes action_out / logprob_out / value_out, the env
 * outputs frame_out [N, D] / env_reward_out / env_done_out [N] / ep_state [N, 5] (in place; read
 * by the owner alone) and the store's outputs. No buffer is both read and written by different
 * workgroups. Every output is bitwise what the two calls give. N <= 4096. */
OCPPO_API int ocppo_head_env_store_linear2(
    ocppo_stream_t stream, const float* hidden, int64_t H, const float* w_actor,
    const float* b_actor, const float* w_critic, const float* b_critic, const float* noise,
    int64_t A, int64_t* action_out, float* logprob_out, float* value_out, uint64_t seed,
    const int64_t* step_base, int64_t step_offset, float* frame_out, float* env_reward_out,
    float* env_done_out, float* ep_state, int64_t N, int64_t W, int64_t D, const void* prev_obs,
    void* obs_out, int obs_dtype, float* net_obs, float* reward_out, float* done_out, int vecnorm,
    double gamma, double epsilon, double clip_reward, double* ret_state, double* rms_state,
    const float* w1, const float* b1, const float* w2, const float* b2, float* y, int64_t ldy,
    int64_t N1, int64_t N2);

/* ---------------------------------------------------------------------------------------------
 * CartPole-v1 vector env (config 1: cleanrl/ppo.py:81-91, 162 -- SyncVectorEnv of
 * RecordEpisodeStatistics(gym.make("CartPole-v1"))), device-resident. gymnasium 0.28.1
 * cartpole.py dynamics in f64 (Euler, same constants and op order), reward 1 per step,
 * TimeLimit 500, same-step auto-reset (obs of a done env = its reset obs), obs = f32(state).
 * Reset states ~ U(-0.05, 0.05)^4 from a counter-based stream of (seed, env, episode index).
 *   actions  : [N] i64 (0 = push left, 1 = push right), or NULL = reset every env
 *   state    : [N, 4] f64 (x, x_dot, theta, theta_dot), in/out
 *   counters : [N, 2] i64 = {elapsed steps, episodes started}, in/out (zero-initialised)
 *   obs_out  : [N, 4] f32;  reward_out, done_out : [N] f32 (may be NULL on reset)
 *   ep_state : [N, 5] f32 RecordEpisodeStatistics counters as in ocppo_synth_env_step, or NULL
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_cartpole_step(ocppo_stream_t stream, uint64_t seed, const int64_t* actions,
                                  int64_t N, double* state, int64_t* counters, float* obs_out,
                                  float* reward_out, float* done_out, float* ep_state);

/* ---------------------------------------------------------------------------------------------
 * Object-set transformer blocks (cleanrl/ppo_atari_oc_transformer.py:215-277: PPOAgent's
 * torch.nn.TransformerEncoderLayer stack, post-norm, batch_first). The two pieces of a block
 * that are not a Linear; all f32, deterministic (no atomics), graph-capturable.
 *
 * ocppo_mha_fwd: masked multi-head self-attention over short sequences, the math path of
 * nn.MultiheadAttention (torch/nn/functional.py multi_head_attention_forward: q, k, v =
 * in-proj output split in in_proj_weight's row order, heads = column groups of dh = E / heads;
 * scaled_dot_product_attention: softmax(q k^T / sqrt(dh) + mask) v with -inf at the keys a
 * key_padding_mask excludes; heads concatenated for out_proj).
 *   qkv       : [B, S, 3E] (q | k | v)
 *   key_valid : [B, S] u8, non-zero = key takes part (the complement of src_key_padding_mask),
 *               or NULL = every key. Excluded keys get weight exactly 0. A sample with no valid
 *               key is OUTSIDE THE CONTRACT (torch yields NaN rows there; this kernel's output
 *               for such a sample is unspecified but finite-or-NaN, never a fault).
 *   out       : [B, S, E]; every query row is computed, excluded ("padded") rows included
 *   lse       : [B, heads, S] log-sum-exp of each query's scaled scores over the valid keys
 * Contract: 1 <= S <= 64, dh = E / heads in {8, 16, 32, 64}, E <= 512, B * heads < 2^31; anything
 * else returns OCPPO_E_INVALID before any launch.
 *
 * ocppo_mha_bwd: its backward. Probabilities are recomputed from qkv and lse; the softmax
 * backward is dS = P (dP - D) with D = sum_d dout * out per query. Writes EVERY element of
 * dqkv [B, S, 3E]; dK and dV rows of excluded keys are exactly 0.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_mha_fwd(ocppo_stream_t stream, const float* qkv, const uint8_t* key_valid,
                            int64_t B, int64_t S, int64_t E, int64_t heads, float* out,
                            float* lse);
OCPPO_API int ocppo_mha_bwd(ocppo_stream_t stream, const float* qkv, const uint8_t* key_valid,
                            const float* out, const float* lse, const float* dout, int64_t B,
                            int64_t S, int64_t E, int64_t heads, float* dqkv);

/* ---------------------------------------------------------------------------------------------
 * Counter-based dropout for the fused encoder block (ABI 33). No mask tensor exists: every launch
 * regenerates its mask from
 *   rng   : device i64 [2] = (seed, offset), read by the kernel (a replayed graph reads the state
 *           of that replay); ocppo_philox_advance does rng[1] += 1 (one thread)
 *   site  : host integer in [0, 256); the agent uses 4 * layer + {0 attention probabilities,
 *           1 dropout1, 2 the FFN's inner dropout, 3 dropout2}
 *   thr   : host u32 = min((uint64)(p * 2^32), 2^32 - 1); keep iff word >= thr (integer compare)
 *   scale : 1 / (1 - p), computed in double on the host, passed as f32 (>= 1, finite)
 * The 32-bit word of an element is a component of Philox4x32-10 with
 *   counter = (lo32 blk, hi32 blk, lo32 sub, hi32 sub), key = (lo32 seed, hi32 seed),
 *   sub = offset * 256 + site (mod 2^64), and
 *   elementwise tensors : flat index e -> blk = e >> 2, component e & 3
 *   attention probabilities of (sample b, head h, query i, key j), j the absolute key index :
 *                         blk = ((b * heads + h) * 64 + i) * 16 + (j >> 2), component j & 3
 * This is a stream of this library, not torch's dropout stream.
 *
 * ocppo_dropout: y[e] = keep(e) ? x[e] * scale : 0 for e < n; out of place (x != y); its backward
 *   is the same call on dy. 16-byte accesses when x and y are 16-B aligned, element by element
 *   otherwise and for the last n % 4 elements -- the same words either way. n = 0 launches nothing.
 * ocppo_mha_dropout_fwd / _bwd: ocppo_mha_fwd / _bwd (same contract, same lse) with dropout on
 *   the attention probabilities: softmax over all valid keys, then out_i = sum_j m_ij P_ij V_j with
 *   m_ij = keep_ij * scale. A query row whose keys are all dropped yields zeros. Backward:
 *   dP_ij = m_ij (dO_i . V_j), D_i = dO_i . O_i, dS_ij = P_ij (dP_ij - D_i),
 *   dV_j = sum_i m_ij P_ij dO_i; every element of dqkv written, excluded keys' dK / dV exactly 0.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_dropout(ocppo_stream_t stream, const float* x, const int64_t* rng,
                            int64_t site, uint32_t thr, float scale, int64_t n, float* y);
OCPPO_API int ocppo_philox_advance(ocppo_stream_t stream, int64_t* rng);
OCPPO_API int ocppo_mha_dropout_fwd(ocppo_stream_t stream, const float* qkv,
                                    const uint8_t* key_valid, const int64_t* rng, int64_t site,
                                    uint32_t thr, float scale, int64_t B, int64_t S, int64_t E,
                                    int64_t heads, float* out, float* lse);
OCPPO_API int ocppo_mha_dropout_bwd(ocppo_stream_t stream, const float* qkv,
                                    const uint8_t* key_valid, const float* out, const float* lse,
                                    const float* dout, const int64_t* rng, int64_t site,
                                    uint32_t thr, float scale, int64_t B, int64_t S, int64_t E,
                                    int64_t heads, float* dqkv);

/* ---------------------------------------------------------------------------------------------
 * ocppo_add_layernorm_fwd: y = LayerNorm(x + res) * gamma + beta over the last dimension (the
 * `self.norm1(x + self._sa_block(...))` / `self.norm2(x + self._ff_block(x))` of
 * torch/nn/modules/transformer.py TransformerEncoderLayer.forward, norm_first = False). Biased
 * variance taken about the mean in a second pass, as torch's layer_norm; rstd = 1 / sqrt(var + eps).
 *   x, res, y : [R, E];  gamma, beta : [E];  mean, rstd : [R] (written);  1 <= E <= 512
 *
 * ocppo_add_layernorm_bwd: its backward. x + res is RECOMPUTED from the two inputs (not saved).
 *   dx : [R, E], the one gradient that flows to both addends
 *   dgamma, dbeta : [E]; per-workgroup partials of a grid that depends on (R, E) only are
 *   written to the workspace (ocppo_add_layernorm_workspace_bytes(R, E)) and summed in
 *   workgroup order by a second launch of the same call.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_add_layernorm_fwd(ocppo_stream_t stream, const float* x, const float* res,
                                      const float* gamma, const float* beta, int64_t R, int64_t E,
                                      double eps, float* y, float* mean, float* rstd);
OCPPO_API size_t ocppo_add_layernorm_workspace_bytes(int64_t R, int64_t E);
OCPPO_API int ocppo_add_layernorm_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                      const float* res, const float* gamma, const float* mean,
                                      const float* rstd, int64_t R, int64_t E, float* dx,
                                      float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * The recurrent PPO agent's LSTM (cleanrl/ppo_atari_lstm.py:140-158, Agent.get_states: one
 * single-layer nn.LSTM call per time step with the incoming state multiplied by 1 - done), ABI 34.
 * All f32; gate order i | f | g | o; w_ih [4H, I], w_hh [4H, H], b_ih, b_hh [4H] as nn.LSTM stores
 * them. One step, for every environment b on its own:
 *   h_in = (1 - done[t, b]) * h,   c_in = (1 - done[t, b]) * c
 *   z = pre[t, b] + h_in w_hh^T + b_hh;   i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_g)
 *   c = f * c_in + i * g,   h = o * tanh(c)
 * Contract: H in {32, 64, 128}, T >= 1, B (N) >= 1, I >= 1, B < 2^31; a negative size, another H
 * or a null required pointer returns OCPPO_E_INVALID before any launch; T = 0 or B = 0 (N = 0)
 * launches nothing. One launch per call, no atomics, no waiting between workgroups (a workgroup
 * owns whole environments for the whole call); an environment's arithmetic runs in an order fixed
 * by H alone, so its results do not depend on B or on the other rows. Graph-capturable.
 *
 * ocppo_lstm_seq_fwd: the recurrence over a whole sequence.
 *   pre   : [T, B, 4H] the input projection x w_ih^T + b_ih (one GEMM outside)
 *   done  : [T, B];  h0, c0 : [B, H];  w_hh 16-byte aligned
 *   h_out : [T, B, H];  hT, cT : [B, H] the state after step T - 1
 *   c_out [T, B, H], gates [T, B, 4H] (the ACTIVATED gates), h_in [T, B, H] (the masked state each
 *   step consumed): what the backward needs; each may be NULL (inference).
 *   Only rows t < T, b < B of an output are written.
 *
 * ocppo_lstm_seq_bwd: its backward through time, t = T - 1 .. 0, carrying (dh, dc).
 *   dh_out : [T, B, H] the gradient at h_out;  gates, c_out, c0, done, w_hh as above
 *   dgates : [T, B, 4H] the gradient at the pre-activations z (= d pre; d w_hh = dgates^T h_in and
 *            d b_hh = its column sum are GEMM-shaped and left to the caller)
 *   What flows from step t to step t - 1 is multiplied by 1 - done[t]. The initial state and the
 *   final state carry no gradient (the script passes a detached clone and drops the final state).
 *
 * ocppo_lstm_step: one step for the rollout, both products inside: x [N, I], done [N];
 *   h, c [N, H] updated in place. z = (x w_ih^T + h_in w_hh^T) + (b_ih + b_hh).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_lstm_seq_fwd(ocppo_stream_t stream, const float* pre, const float* w_hh,
                                 const float* b_hh, const float* done, const float* h0,
                                 const float* c0, int64_t T, int64_t B, int64_t H, float* h_out,
                                 float* c_out, float* gates, float* h_in, float* hT, float* cT);
OCPPO_API int ocppo_lstm_seq_bwd(ocppo_stream_t stream, const float* dh_out, const float* gates,
                                 const float* c_out, const float* c0, const float* done,
                                 const float* w_hh, int64_t T, int64_t B, int64_t H,
                                 float* dgates);
OCPPO_API int ocppo_lstm_step(ocppo_stream_t stream, const float* x, const float* w_ih,
                              const float* b_ih, const float* w_hh, const float* b_hh,
                              const float* done, int64_t N, int64_t I, int64_t H, float* h,
                              float* c);

/* ---------------------------------------------------------------------------------------------
 * PQN (cleanrl/pqn_atari_envpool.py) on the device rollout, ABI 35. All f32. A negative size, a
 * size outside a contract below or a null required pointer returns OCPPO_E_INVALID before any
 * launch; a zero row / env / sample count launches nothing and returns OCPPO_OK. No atomics:
 * every result is the same run to run. Graph-capturable.
 *
 * ocppo_q_lambda: the Q(lambda) targets of :248-261, bitwise the script's f32 loop (same ops, same
 * order, no FMA contraction; gamma, q_lambda and 1 - q_lambda rounded to f32 once):
 *   t = T-1 : returns[t] = rewards[t] + (gamma * max_a next_q) * (1 - next_done)
 *   t < T-1 : returns[t] = rewards[t] + (gamma * (q_lambda * returns[t+1]
 *                                                 + (1 - q_lambda) * values[t+1])) * (1 - dones[t+1])
 *   rewards, values, dones, returns : [T, N];  next_q : [N, A];  next_done : [N];  A >= 1
 *
 * ocppo_ln_relu_fwd: y = relu(LayerNorm(x) * gamma + beta) over the last dimension of [R, E] rows,
 * 1 <= E <= 1024 (relu = 0: no ReLU). mean, rstd [R] are written. The row is centred before the
 * variance is taken (sum of squared deviations / E, never E[x^2] - mean^2), and re-centred once so
 * that a common offset of the row costs no precision; rstd = 1 / sqrt(var + eps).
 * ocppo_ln_relu_bwd: dx [R, E], dgamma, dbeta [E] from dy, x, y (the ReLU mask is y > 0; y may be
 * NULL with relu = 0), mean and rstd. Per-workgroup partials of dgamma / dbeta (a grid that
 * depends on R only) go to the workspace (ocppo_ln_relu_workspace_bytes(R, E)) with plain stores
 * and are summed in workgroup order by a second launch of the same call.
 *
 * ocppo_pqn_act: q = hidden wq^T + bq for hidden [N, H], wq [A, H]; values[n] = max_a q[n, a] at
 * the LOWEST index among equal maxima (torch.argmax on the CPU), actions[n] = that index or, with
 * probability epsilon, a uniform random action: exactly ocppo_epsilon_greedy's schedule, coin and
 * random action for the same (seed, *step + step_offset). epsilon_out [1] and q_out [N, A] may be
 * NULL. Contract: 1 <= A <= 18, H a multiple of 4 in [4, 1024], hidden and wq 16-byte aligned
 * (ocppo_q_head_epsilon_greedy's, widened), duration > 0.
 *
 * ocppo_pqn_loss_fwd_bwd: F.mse_loss(returns, q[b, actions[b]]) of :276-277 and its gradient:
 *   stats[0] = mean((returns - q_a)^2), stats[1] = mean(q_a);  dq [M, A] = (2 / M)(q_a - returns)
 *   in the taken column, exact zeros elsewhere. One workgroup, a fixed summation order.
 *   1 <= A <= 18; an action outside [0, A) is clamped into it (no out-of-range read).
 *
 * ocppo_clip_radam_step: ocppo_clip_adam_step's clip (same norm kernel, grad_scale, flat buffers,
 * scalars and workspace: ocppo_clip_adam_workspace_bytes) followed by torch.optim.RAdam's step
 * (no weight decay). rho_t and the rectification come from the device step count in double:
 * with beta2 = 0.999 steps 1-5 are un-rectified (p -= lr * m / (1 - b1^t)), step 6 is the first
 * rectified one. scalars[OCPPO_OPT_RECT] reports the rectification term (0: un-rectified).
 * n_planes must be 0 (plane jobs are ocppo_clip_adam_step's). The launches, checks and kernel body
 * are ocppo_clip_adam_step's; the rectification scalars and the element update are its own.
 * ------------------------------------------------------------------------------------------- */
#define OCPPO_OPT_RECT 5
OCPPO_API int ocppo_q_lambda(ocppo_stream_t stream, const float* rewards, const float* values,
                             const float* dones, const float* next_q, const float* next_done,
                             int64_t T, int64_t N, int64_t A, double gamma, double q_lambda,
                             float* returns);
OCPPO_API int ocppo_ln_relu_fwd(ocppo_stream_t stream, const float* x, const float* gamma,
                                const float* beta, int64_t R, int64_t E, double eps, int relu,
                                float* y, float* mean, float* rstd);
OCPPO_API size_t ocppo_ln_relu_workspace_bytes(int64_t R, int64_t E);
OCPPO_API int ocppo_ln_relu_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                const float* y, const float* gamma, const float* mean,
                                const float* rstd, int64_t R, int64_t E, int relu, float* dx,
                                float* dgamma, float* dbeta, void* workspace,
                                size_t workspace_bytes);
OCPPO_API int ocppo_pqn_act(ocppo_stream_t stream, const float* hidden, int64_t N, int64_t H,
                            const float* wq, const float* bq, int64_t A, uint64_t seed,
                            const int64_t* step, int64_t step_offset, double start_e,
                            double end_e, double duration, int64_t* actions, float* values,
                            float* epsilon_out, float* q_out);
OCPPO_API int ocppo_pqn_loss_fwd_bwd(ocppo_stream_t stream, const float* q, const int64_t* actions,
                                     const float* returns, int64_t M, int64_t A, float* dq,
                                     float* stats);
OCPPO_API int ocppo_clip_radam_step(ocppo_stream_t stream, float* params, const float* grads,
                                    float* exp_avg, float* exp_avg_sq, int64_t P, const float* lr,
                                    double beta1, double beta2, double eps, double grad_scale,
                                    double max_norm, float* scalars, void* workspace,
                                    size_t workspace_bytes, int n_planes);

/* ---------------------------------------------------------------------------------------------
 * Discrete SAC (cleanrl/sac_atari.py) on the DQN loop, ABI 36. All f32, [B, A] row-major,
 * 1 <= A <= 18. A negative B / E, an A outside the range or a null required pointer returns
 * OCPPO_E_INVALID before any launch; B = 0 (E = 0) launches nothing and returns OCPPO_OK. One
 * workgroup per loss launch, no atomics, a fixed summation order (the sums over the batch run in
 * f64: a reported mean is the f32 nearest to the sum of its f32 terms). Graph-capturable; `alpha` is a
 * device scalar, so no launch here needs a value from the host between train steps.
 * probs are Categorical(logits=l).probs in torch.distributions' op order, log_pi is
 * F.log_softmax(l) (:165-169).
 *
 * The critic launch (:283-302):
 *   y_b  = rewards_b + ((1 - dones_b) * gamma) * sum_j p'_bj * (min(q1t_bj, q2t_bj) - alpha * logp'_bj)
 *          with p', logp' from next_logits and q1t / q2t the two target critics on the next obs
 *   stats = {qf1_loss, qf2_loss, mean_b q1[b, a_b], mean_b q2[b, a_b]},
 *          qf_loss = mean_b (q[b, a_b] - y_b)^2
 *   dq1, dq2 [B, A] = (2 / B)(q[b, a_b] - y_b) in the taken column, exact zeros elsewhere
 *   y_out [B] may be NULL. An action outside [0, A) is clamped into it (no out-of-range read).
 *
 * The actor / temperature launch (:309-328), q1 / q2 the online critics AFTER the critic step:
 *   g_bj = alpha * logp_bj - min(q1_bj, q2_bj);   actor_loss = mean_bj p_bj g_bj
 *   dlogits_bk = p_bk (g_bk - sum_j p_bj g_bj) / (B A)
 *   alpha_loss = mean_bj p_bj * (-exp(log_alpha) * (logp_bj + target_entropy))
 *   autotune != 0: one torch.optim.Adam (single-tensor) step on *log_alpha with the gradient
 *   exp(log_alpha) * (-mean_bj p_bj (logp_bj + target_entropy)), bias correction from
 *   *adam_step + 1 (which is written back), then *alpha = exp(*log_alpha). autotune == 0: alpha,
 *   log_alpha and the Adam state are not touched (the state pointers may be NULL), alpha_loss = 0.
 *   stats = {actor_loss, alpha_loss, alpha after the launch, mean_b policy entropy}
 *
 * The acting launch (:248-252), t = *step + step_offset: t < learning_starts gives a uniform
 * action in [0, A); otherwise one draw of Categorical(logits[e]) by the exponential race
 * argmax_j p_j / e_j (first maximum), e_j ~ Exp(1) in double. Both from the library's counter
 * stream (splitmix64 / unit53) under the SAC key, keyed by (seed, t, e, j). logits [E, A].
 *
 * ocppo_clip_adam_step_exact: ocppo_clip_adam_step (same norm pass, clip, flat buffers, scalars
 * and workspace; no plane jobs) with torch.optim.Adam's scalars taken as torch takes them, from
 * doubles: lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - beta1 and 1 - beta2 are formed in double and
 * rounded to f32 once, and the element update is lerp_ / mul_().addcmul_() / addcdiv_() in torch's
 * op order. ocppo_clip_adam_step forms them in f32, which a parameter that starts at zero shows
 * whole (up to 6e-7 of the step from 1 - 0.9^t alone); its results are unchanged. It runs
 * ocppo_clip_adam_step's vectorised kernel body, so params, grads, exp_avg and exp_avg_sq must all
 * be 16-byte aligned (earlier only grads had to be).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_clip_adam_step_exact(ocppo_stream_t stream, float* params, const float* grads,
                                         float* exp_avg, float* exp_avg_sq, int64_t P,
                                         const float* lr, double beta1, double beta2, double eps,
                                         double grad_scale, double max_norm, float* scalars,
                                         void* workspace, size_t workspace_bytes);
OCPPO_API int ocppo_sac_critic_loss_fwd_bwd(ocppo_stream_t stream, const float* next_logits,
                                            const float* q1_next_target,
                                            const float* q2_next_target, const float* q1,
                                            const float* q2, const int64_t* actions,
                                            const float* rewards, const float* dones, int64_t B,
                                            int64_t A, double gamma, const float* alpha,
                                            float* dq1, float* dq2, float* stats, float* y_out);
OCPPO_API int ocppo_sac_actor_alpha_fwd_bwd(ocppo_stream_t stream, const float* logits,
                                            const float* q1, const float* q2, int64_t B,
                                            int64_t A, float* alpha, float* log_alpha,
                                            double target_entropy, float* exp_avg,
                                            float* exp_avg_sq, int64_t* adam_step, double lr,
                                            double beta1, double beta2, double eps, int autotune,
                                            float* dlogits, float* stats);
OCPPO_API int ocppo_sac_act(ocppo_stream_t stream, const float* logits, int64_t E, int64_t A,
                            uint64_t seed, const int64_t* step, int64_t step_offset,
                            int64_t learning_starts, int64_t* actions);

/* -------------------------------------------------------------------------------------------
 * Random Network Distillation (cleanrl/ppo_rnd_envpool.py) beyond PPO (ABI 37). Every entry is
 * capture-safe (device scalars only), deterministic (no atomics; sums in an order the shapes fix)
 * and checks its arguments before any launch.
 *
 * Running statistics (gym's RunningMeanStd, all f64): state [2C + 1] = mean [C], var [C], count,
 * starting at zeros, ones, 1e-4. ocppo_rms_update merges the per-column batch mean and population
 * variance of x [R, C] (dtype OCPPO_F32 / BF16 / U8, rows row_stride elements apart: a frame of a
 * stacked observation) with batch count R:
 *   delta = bm - mean; tot = count + R; mean' = mean + delta * R / tot;
 *   var' = (var * count + bv * R + delta^2 * count * R / tot) / tot; count' = tot.
 * The column sums are carried as hi + lo pairs, so bm and bv are within an ulp of exact. Two
 * launches (partials over column blocks x row chunks, then the merge).
 * ocppo_rnd_normalize: out [R, C] f32 = f32(clip((f64(x) - mean_c) / sqrt(var_c), -5, 5)).
 *
 * ocppo_rnd_error: out[r] = sum_j (target[r, j] - pred[r, j])^2 / 2 (:373), rows [R, D].
 *
 * ocppo_rnd_reward_norm (:390-400): the RewardForwardFilter over curiosity [T, N] walked along the
 * env axis as the script does: for n = 0 .. N-1: rewems[t] = rewems[t] * f32(int_gamma) +
 * curiosity[t, n] (f32, two roundings), filtered[n, t] = rewems[t] (written when filtered is
 * given); rewems [T] persists (zeros at first). The mean and population variance of the N * T
 * filtered values (f64, pairs) are merged into state [3] = {mean, var, count} with batch count N
 * (the script's len() of a 2-D array), then curiosity /= f32(sqrt(var')) in place. Two launches.
 *
 * ocppo_rnd_gae (:406-442): both scans in one launch, each op for op ocppo_gae's arithmetic and so
 * bitwise the script's f32 loop: extrinsic over rewards / ext_values / dones with gamma, intrinsic
 * over curiosity / int_values with int_gamma and nonterminal 1; returns = advantages + values;
 * advantages = (int_adv * f32(int_coef)) + (ext_adv * f32(ext_coef)). All arrays [T, N] f32, the
 * next_* rows [N].
 *
 * ocppo_rnd_aux_loss_fwd_bwd (:463-472, :509): with d = pred - target [M, D], row loss
 * f_r = mean_j d^2, mask_r = unit53(splitmix64(h + r + 1)) < update_proportion where
 * h = splitmix64(splitmix64(seed ^ key) + *counter) (the library's counter stream, not torch.rand),
 * c = max(sum mask, 1):  dpred = d * f32(2 / (D c)) on kept rows, d * 0 elsewhere;
 * dv_int = (v_int - ret_int) * f32(vf_coef / M); stats [3] = {0.5 mean (v_int - ret_int)^2,
 * sum_r mask_r f_r / c, sum mask} (batch sums in f64). *counter advances by one (on the device, in
 * the second of its two launches). update_proportion outside [0, 1] is refused.
 * ocppo_rnd_mask writes the same mask [M] as f32 0 / 1 for *counter, which it leaves alone.
 *
 * Workspaces: ocppo_*_workspace_bytes, 8-byte aligned, no initial contents needed.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_rms_update_workspace_bytes(int64_t R, int64_t C);
OCPPO_API int ocppo_rms_update(ocppo_stream_t stream, const void* x, int dtype, int64_t R,
                               int64_t C, int64_t row_stride, double* state, void* workspace,
                               size_t workspace_bytes);
OCPPO_API int ocppo_rnd_normalize(ocppo_stream_t stream, const void* x, int dtype, int64_t R,
                                  int64_t C, int64_t row_stride, const double* state, float* out);
OCPPO_API int ocppo_rnd_error(ocppo_stream_t stream, const float* pred, const float* target,
                              int64_t R, int64_t D, float* out);
OCPPO_API size_t ocppo_rnd_reward_norm_workspace_bytes(int64_t T);
OCPPO_API int ocppo_rnd_reward_norm(ocppo_stream_t stream, float* curiosity, float* rewems,
                                    double* state, int64_t T, int64_t N, double int_gamma,
                                    void* workspace, size_t workspace_bytes, float* filtered);
OCPPO_API int ocppo_rnd_gae(ocppo_stream_t stream, const float* rewards, const float* ext_values,
                            const float* dones, const float* next_ext_value,
                            const float* next_done, const float* curiosity,
                            const float* int_values, const float* next_int_value, int64_t T,
                            int64_t N, double gamma, double int_gamma, double gae_lambda,
                            double int_coef, double ext_coef, float* ext_advantages,
                            float* ext_returns, float* int_advantages, float* int_returns,
                            float* advantages);
OCPPO_API size_t ocppo_rnd_aux_loss_workspace_bytes(int64_t M);
OCPPO_API int ocppo_rnd_aux_loss_fwd_bwd(ocppo_stream_t stream, const float* pred,
                                         const float* target, const float* v_int,
                                         const float* ret_int, int64_t M, int64_t D,
                                         uint64_t seed, int64_t* counter,
                                         double update_proportion, double vf_coef, float* dpred,
                                         float* dv_int, float* stats, void* workspace,
                                         size_t workspace_bytes);
OCPPO_API int ocppo_rnd_mask(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                             int64_t M, double update_proportion, float* out);

/* -------------------------------------------------------------------------------------------
 * Phasic Policy Gradient (cleanrl/ppg_procgen.py) beyond PPO (ABI 38). Every entry is capture-safe,
 * deterministic (no atomics; sums in an order the sizes fix) and checks its arguments before any
 * launch.
 *
 * ocppo_ppg_aux_loss_fwd_bwd (:449-461), rows [M], 1 <= A <= 18: per row both logit rows are
 * normalised as Categorical(logits=..) normalises them (the loss and rollout kernels' routine):
 *   kl_r = sum_j p_old_j (ln_old_j - ln_new_j)   (a term with p_old_j == 0 counts 0, one with
 *          p_new_j == 0 and p_old_j != 0 counts +inf: torch.distributions.kl's masks)
 *   dlogits = (p_new - p_old) * f32(beta_clone / M)   (d (beta_clone mean kl) / d new_logits)
 *   dvalue = (new_value - returns) * f32(1 / M); daux = (new_aux_value - returns) * f32(1 / M)
 *   stats [3] = {mean kl_r, 0.5 mean (new_aux_value - returns)^2, 0.5 mean (new_value - returns)^2}
 * (row sums in f64). A row whose old and new logits are bit-equal gives kl_r == 0 and a zero
 * dlogits row exactly. Two launches; workspace ocppo_ppg_aux_loss_workspace_bytes(M), 8-byte
 * aligned, no initial contents needed.
 *
 * ocppo_ppg_aux_gather (:443-453): one launch writes the auxiliary minibatch of the env columns
 * cols [k] (int64, device) of aux_obs [T, R, D] (obs_dtype OCPPO_F32 / BF16 / U8), aux_pi [T, R, A]
 * f32 and aux_returns [T, R] f32, flattened t-major: output row t k + c holds column cols[c] of
 * step t; out_obs [T k, D] f32 (the exact conversion ocppo_gather_rows makes), out_pi [T k, A],
 * out_returns [T k]. 16-byte stores where D (A) % 4 == 0 and the pointers are aligned. A column
 * index outside [0, R) is never dereferenced: it is clamped into the range.
 *
 * ocppo_clip_adam_step_seg: ocppo_clip_adam_step (same arithmetic, same scalars and workspace, no
 * plane jobs) over a buffer of two segments, the head [0, split) and the tail [split, P) (split and
 * P multiples of 4), each with its own step count, as torch.optim.Adam keeps one per parameter and
 * skips a parameter whose grad is None. The head takes part in every step; its count is
 * scalars[OCPPO_OPT_STEP]. tail_active = 0: the clip norm runs over the head's gradients alone and
 * nothing of the tail -- parameters, both moments, scalars[OCPPO_OPT_TAIL_STEP] -- is written or
 * read; scalars[OCPPO_OPT_TAIL_SKIPPED] counts these steps. tail_active = 1: the norm runs over
 * the whole buffer and the tail's step scalars are formed from its own count,
 * OCPPO_OPT_STEP - OCPPO_OPT_TAIL_SKIPPED, which scalars[OCPPO_OPT_TAIL_STEP] then reports.
 * ------------------------------------------------------------------------------------------- */
#define OCPPO_OPT_TAIL_SKIPPED 6
#define OCPPO_OPT_TAIL_STEP 7
OCPPO_API size_t ocppo_ppg_aux_loss_workspace_bytes(int64_t M);
OCPPO_API int ocppo_ppg_aux_loss_fwd_bwd(ocppo_stream_t stream, const float* new_logits,
                                         const float* new_value, const float* new_aux_value,
                                         const float* old_logits, const float* returns, int64_t M,
                                         int64_t A, double beta_clone, float* dlogits,
                                         float* dvalue, float* daux, float* stats,
                                         void* workspace, size_t workspace_bytes);
OCPPO_API int ocppo_ppg_aux_gather(ocppo_stream_t stream, const void* aux_obs, int obs_dtype,
                                   const float* aux_pi, const float* aux_returns,
                                   const int64_t* cols, int64_t T, int64_t R, int64_t k, int64_t D,
                                   int64_t A, float* out_obs, float* out_pi, float* out_returns);
OCPPO_API int ocppo_clip_adam_step_seg(ocppo_stream_t stream, float* params, const float* grads,
                                       float* exp_avg, float* exp_avg_sq, int64_t P, int64_t split,
                                       int tail_active, const float* lr, double beta1,
                                       double beta2, double eps, double grad_scale,
                                       double max_norm, float* scalars, void* workspace,
                                       size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * The recurrent PQN learner (cleanrl/pqn_atari_envpool_lstm.py): where the LSTM and the Q head
 * meet, ABI 39. All f32, no atomics, no waiting between workgroups, the same result run to run,
 * graph-capturable. A negative size, a size outside a contract below or a null required pointer
 * returns OCPPO_E_INVALID before any launch; a zero row / env count launches nothing and returns
 * OCPPO_OK.
 *
 * ocppo_pqn_lstm_act: the rollout step (:261-267) in one launch: ocppo_lstm_step's state update
 * of every environment (x [N, I], w_ih [4H, I], w_hh [4H, H], b_ih, b_hh [4H], done [N],
 * h, c [N, H]), then ocppo_pqn_act on the new h (wq [A, H], bq [A], the same seed / step /
 * step_offset / schedule arguments) inside the workgroup that owns the environment. Both halves
 * are the device functions of those two entries: h and c are bitwise what ocppo_lstm_step writes,
 * and actions, values [N], epsilon_out [1] and q_out [N, A] bitwise what ocppo_pqn_act returns on
 * that h. commit = 1 updates h / c in place; commit = 0 leaves them untouched and writes only
 * q_out / values (/ actions, epsilon_out when given): the bootstrap of :287, whose state is
 * dropped. actions may be NULL with commit = 0; epsilon_out and q_out may be NULL.
 * Contract: H in {32, 64, 128}, 1 <= A <= 18, I >= 1, N >= 1 (N < 2^31), wq 16-byte aligned,
 * duration > 0. An environment's results do not depend on N or on the other rows.
 *
 * ocppo_pqn_head_loss_fwd_bwd: the update's Q head, the MSE loss on the taken action and the
 * head's backward (:318-325) in one call, one dot product per row (h [M, H], wq [A, H], bq [A],
 * actions [M] int64, returns [M]):
 *   q_a[m] = h[m] . wq[a_m] + bq[a_m]
 *   stats [2] = {mean((returns - q_a)^2), mean(q_a)};   g_m = f32(2 / M) * (q_a[m] - returns[m])
 *   dh[m] = g_m * wq[a_m]  [M, H]  (f32 products, element by element)
 *   dwq[a] = sum_{m: a_m = a} g_m * h[m]  [A, H];   dbq[a] = sum_{m: a_m = a} g_m  [A]
 * Every sum (over H, over the rows, over the workgroups' partials) is accumulated in f64 from exact
 * f32 x f32 products and rounded to f32 once; g_m above, dh's factor, is f32 arithmetic on the
 * rounded q_a, while dwq / dbq sum the f64 (2 / M)(q_a - returns) of the unrounded q_a.
 * dwq / dbq are overwritten; rows of actions nobody took are exact zeros. An action outside [0, A)
 * is clamped into it, as in ocppo_pqn_loss_fwd_bwd. Two launches of the one call: per-workgroup
 * partials (a grid that depends on M and H only) go to the workspace with plain stores and are
 * summed in workgroup order. The workspace (ocppo_pqn_head_loss_workspace_bytes(M, H, A), 16-byte
 * aligned, no initial contents needed; too small or NULL: OCPPO_E_WORKSPACE) starts with q_a [M],
 * which the call leaves there for the caller.
 * Contract: H a multiple of 4 in [4, 1024], 1 <= A <= 18, M >= 1 (M < 2^31); h, wq and dh 16-byte
 * aligned.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_pqn_lstm_act(ocppo_stream_t stream, const float* x, const float* w_ih,
                                 const float* b_ih, const float* w_hh, const float* b_hh,
                                 const float* done, int64_t N, int64_t I, int64_t H, float* h,
                                 float* c, int commit, const float* wq, const float* bq, int64_t A,
                                 uint64_t seed, const int64_t* step, int64_t step_offset,
                                 double start_e, double end_e, double duration, int64_t* actions,
                                 float* values, float* epsilon_out, float* q_out);
OCPPO_API size_t ocppo_pqn_head_loss_workspace_bytes(int64_t M, int64_t H, int64_t A);
OCPPO_API int ocppo_pqn_head_loss_fwd_bwd(ocppo_stream_t stream, const float* h, const float* wq,
                                          const float* bq, const int64_t* actions,
                                          const float* returns, int64_t M, int64_t H, int64_t A,
                                          float* dh, float* dwq, float* dbq, float* stats,
                                          void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * The QDagger learner (cleanrl/qdagger_dqn_atari_impalacnn.py) on the DQN loop, ABI 40. All f32,
 * one workgroup each, no atomics, sums in a fixed order (wave shuffles and LDS): the same result
 * run to run; graph-capturable. Bad sizes and null required pointers return OCPPO_E_INVALID
 * before any launch.
 *
 * ocppo_qdagger_loss_fwd_bwd: the loss of :303-315 / :412-424 and d loss / d q in one launch.
 * q, q_next, q_teacher [B, A] (student(obs), target(next_obs), teacher(obs)), actions [B] int64,
 * rewards, dones [B]; T = temperature, c = *distill_coeff (NULL: 1.0, the offline phase):
 *   y_b     = r_b + (f32(gamma) * max_a q_next[b, a]) * (1 - d_b)
 *   q_loss  = mean_b (y_b - q[b, a_b])^2
 *   t = q_teacher / T,  s = q / T
 *   distill = sum_b sum_a -softmax(t)[b, a] * (log_softmax(s)[b, a] - log_softmax(t)[b, a])
 *   loss    = q_loss + c * distill
 *   dq[b, a] = f32(2 / B) (q[b, a_b] - y_b) [a == a_b]
 *              + ((softmax(s)[b, a] * sum_a' softmax(t)[b, a'] - softmax(t)[b, a]) * c) / T
 * distill is a SUM over the batch, as in the script: its kl_divergence_with_logits returns a
 * scalar, so the torch.mean around it does nothing. The teacher's softmax sum in dq is taken as
 * (sum_a' e_a') / Z = 1, so a student row equal to the teacher's has a zero distillation gradient
 * and dq is then the TD gradient's bits. The TD half is ocppo_td_loss_fwd_bwd's device code: with
 * c = 0, dq, stats[1] and stats[3] are bitwise that call's dq, stats[0] and stats[1].
 *   stats [5] = {loss, q_loss, distill, mean_b q[b, a_b], c}
 * Contract: B >= 1, 1 <= A <= 1024, temperature > 0.
 *
 * ocppo_qdagger_episode_push: the deque(maxlen=10) of episodic returns (:365, :390) and the
 * coefficient of :408-411, once per env step, from the env's raw reward [E] and done [E] (f32,
 * done != 0 ends an episode). Envs are visited in ascending index order:
 *   run_ret[e] += reward[e] (f32);  on done: ring[head] = run_ret[e], head = (head + 1) % 10,
 *   count = min(count + 1, 10), run_ret[e] = 0
 *   coeff_out[0] = count < 10 ? 1 : f32(max(1 - mean(ring) / teacher_mean, 0))
 * with the mean summed in f64 from the oldest return to the newest. run_ret [E] f32, ring [10]
 * f32, ring_state [2] int64 = {head, count} (all zero at the start).
 * Contract: E >= 1, teacher_mean finite and not 0.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_qdagger_loss_fwd_bwd(ocppo_stream_t stream, const float* q,
                                         const float* q_next, const float* q_teacher,
                                         const int64_t* actions, const float* rewards,
                                         const float* dones, int64_t B, int64_t A, double gamma,
                                         double temperature, const float* distill_coeff,
                                         float* dq, float* stats);
OCPPO_API int ocppo_qdagger_episode_push(ocppo_stream_t stream, const float* reward,
                                         const float* done, int64_t E, float* run_ret,
                                         float* ring, int64_t* ring_state, double teacher_mean,
                                         float* coeff_out);

/* ---------------------------------------------------------------------------------------------
 * Continuous-action PPO / RPO (cleanrl/ppo_continuous_action.py, rpo_continuous_action.py): a
 * diagonal-Gaussian policy of A <= 64 action dimensions. f32 unless stated, no atomics (every
 * cross-row sum is two fixed-order stages), graph-capturable.
 *
 * ocppo_gauss_head_sample (:134-141): mean, z [N, A], logstd [A], value_in [N] ->
 *   action = z * exp(logstd) + mean (two roundings, as torch.normal), logprob [N] = the row sum of
 *   Normal.log_prob in column order, value = value_in.
 * ocppo_gauss_ppo_loss_fwd_bwd (:265-300 from the network outputs on, with the backward, one
 *   launch): mean [M, A], logstd [A], new_value [M], the minibatch's actions [M, A], old
 *   log-probs, advantages, returns, old values [M], adv_stats [2] (mean, unbiased std; norm_adv)
 *   -> dmean [M, A], dvalue [M], dlogstd [A] (summed over rows, the entropy bonus included), stats
 *   [OCPPO_NUM_STATS]. Ties of both max() as ocppo_ppo_loss_fwd_bwd. rpo_alpha > 0: mean[m, a] +=
 *   u in [-alpha, alpha) from the library's Philox stream keyed by (seed, rpo_counter[0], mb, m,
 *   a), rpo_counter a device int64 the caller advances; rpo_alpha == 0 is bitwise the launch
 *   without it. ocppo_rpo_noise writes the same draws [M, A].
 * ocppo_env_normalize (:96-100: NormalizeObservation, clip +-10, NormalizeReward(gamma), clip
 *   +-10) on N envs' raw step outputs, per-env statistics norm_state [N, 2D + 5] f64 = {obs mean
 *   [D], obs var [D], obs count, return accumulator, return mean, var, count} (initially 0, 1,
 *   1e-4, 0, 0, 1, 1e-4). obs [N, D]: the returned observation (the reset one of a done env);
 *   final_obs [N, D]: the terminal one, normalised first for done envs (two updates), NULL with
 *   both flag arrays NULL; reward [N] or NULL (a reset); terminated / truncated [N] (!= 0) or
 *   NULL; ret = ret * gamma * (1 - terminated) + reward. A flag of 0 copies that output through.
 * ocppo_pendulum_step: Pendulum-v1 (gymnasium 0.28.1 dynamics, f64) behind ClipAction and
 *   TimeLimit(200), same-step auto-reset. actions [N] f32 or NULL = reset; state [N, 2] f64;
 *   counters [N, 2] i64 {elapsed, episodes}; obs_out [N, 3]; final_obs_out [N, 3] or NULL;
 *   reward_out / done_out [N]; ep_state [N, 5] on the raw reward or NULL; reset states from
 *   ocppo_cartpole_step's stream. norm_state != NULL: the outputs pass through
 *   ocppo_env_normalize's chain in the same launch, bitwise the two launches.
 * Contract: 1 <= A <= 64, M >= 1, D >= 1, N <= 2^20, 0 <= gamma <= 1.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_gauss_head_sample(ocppo_stream_t stream, const float* mean,
                                      const float* logstd, const float* z, const float* value_in,
                                      int64_t N, int64_t A, float* action, float* logprob,
                                      float* value);
OCPPO_API int ocppo_gauss_ppo_loss_fwd_bwd(
    ocppo_stream_t stream, const float* mean, const float* logstd, const float* new_value,
    int64_t M, int64_t A, const float* actions, const float* logprobs, const float* advantages,
    const float* returns, const float* values, const float* adv_stats, double clip_coef,
    double ent_coef, double vf_coef, int norm_adv, int clip_vloss, uint64_t seed,
    const int64_t* rpo_counter, int64_t mb, double rpo_alpha, float* dmean, float* dvalue,
    float* dlogstd, float* stats);
OCPPO_API int ocppo_rpo_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* rpo_counter,
                              int64_t mb, int64_t M, int64_t A, double rpo_alpha, float* out);
OCPPO_API int ocppo_env_normalize(ocppo_stream_t stream, const float* obs, const float* final_obs,
                                  const float* reward, const float* terminated,
                                  const float* truncated, int64_t N, int64_t D, double* norm_state,
                                  int norm_obs, int norm_reward, double gamma, float* obs_out,
                                  float* reward_out);
OCPPO_API int ocppo_pendulum_step(ocppo_stream_t stream, uint64_t seed, const float* actions,
                                  int64_t N, double* state, int64_t* counters, float* obs_out,
                                  float* final_obs_out, float* reward_out, float* done_out,
                                  float* ep_state, double* norm_state, int norm_obs,
                                  int norm_reward, double gamma);

/* ---------------------------------------------------------------------------------------------
 * TD3 / DDPG (cleanrl/td3_continuous_action.py, ddpg_continuous_action.py), ABI 42: a
 * deterministic policy over float-vector actions, 1 <= A <= 64. All f32 unless stated, no atomics
 * (the batch sums are f64 in a fixed order: bitwise repeatable), graph-capturable, one launch each
 * (the sample: two). scale / bias / low / high are device arrays [A].
 *
 * ocppo_cont_replay_add / _sample: SB3 ReplayBuffer(optimize_memory_usage=False,
 *   handle_timeout_termination=False): rb_obs, rb_next_obs [size, E, D], rb_actions [size, E, A],
 *   rb_rewards, rb_dones [size, E], state = device int64 {pos, full}. add stores final_obs in the
 *   rows whose done != 0 (final_obs and done both NULL: none) and terminated (NULL: 0) as the done
 *   flag; carry != 0: obs <- next_obs afterwards. sample draws B (row, env) pairs uniformly over
 *   the filled rows from the stream keyed by (seed, counter[0], b), writes obs_act [B, D + A] =
 *   cat(obs, action), the observation columns of next_obs_act [B, D + A] (its action columns are
 *   left for ocppo_td3_target_actions), rewards_out, dones_out [B], indices_out [B, 2] or NULL,
 *   then counter[0] += 1.
 * ocppo_td3_act (:205-211) at global step t = step[0] + step_offset: t < learning_starts: uniform
 *   in [low, high) per dimension; else clip(tanh(hidden W^T + b) * scale + bias + (scale *
 *   exploration_noise) * z, low, high), hidden [E, H], w_mu [A, H], z a Box-Muller normal in f32.
 *   Draws: Philox4x32-10 keyed by (seed, t, e, a). ocppo_td3_noise writes them: mode 0 z, mode 1
 *   the uniform phase's u in [0, 1), both [rows, A] at t = counter[0] + offset; mode 2 the target
 *   stream's z at sample counter counter[0] + offset.
 * ocppo_td3_target_actions (:239-245): mu [B, A] (the target actor's output before tanh) ->
 *   next_obs_act[:, D:] = clamp(tanh(mu) * scale + bias + clamp(z * policy_noise, +-noise_clip) *
 *   scale, low0, high0); policy_noise == 0 (DDPG, :216): no stream, no clamp.
 * ocppo_td3_critic_loss_fwd_bwd (:248-255): y = r + ((1 - d) * gamma) * min(q1t, q2t), dq = (2 /
 *   B)(q - y), stats [4] = {qf1_loss, qf2_loss, mean q1, mean q2}; q2_next_target, q2, dq2 all
 *   NULL: the single critic of ddpg_continuous_action.py:218-221. y_out [B] or NULL.
 * ocppo_td3_policy_actions_fwd / _bwd (:263): xa [B, D + A] = obs_act with its action columns
 *   replaced by tanh(mu) * scale + bias, tanh_out [B, A]; dmu = (dxa[:, D:] * scale) * (1 -
 *   tanh^2).
 * ocppo_polyak (:269-274): targets[k][i] = tau * params[k][i] + (1 - tau) * targets[k][i] for
 *   1 <= n_pairs <= 4 flat buffers of numels[k] elements (host arrays): two rounded products and
 *   one rounded add.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_cont_replay_add(ocppo_stream_t stream, float* obs, const float* next_obs,
                                    const float* final_obs, const float* done,
                                    const float* actions, const float* rewards,
                                    const float* terminated, int64_t E, int64_t D, int64_t A,
                                    int64_t* state, int64_t size, float* rb_obs,
                                    float* rb_next_obs, float* rb_actions, float* rb_rewards,
                                    float* rb_dones, int carry);
OCPPO_API int ocppo_cont_replay_sample(ocppo_stream_t stream, uint64_t seed, int64_t* counter,
                                       const int64_t* state, int64_t size, int64_t E, int64_t D,
                                       int64_t A, const float* rb_obs, const float* rb_next_obs,
                                       const float* rb_actions, const float* rb_rewards,
                                       const float* rb_dones, int64_t B, float* obs_act,
                                       float* next_obs_act, float* rewards_out, float* dones_out,
                                       int64_t* indices_out);
OCPPO_API int ocppo_td3_act(ocppo_stream_t stream, const float* hidden, int64_t E, int64_t H,
                            const float* w_mu, const float* b_mu, int64_t A,
                            const float* action_scale, const float* action_bias, const float* low,
                            const float* high, uint64_t seed, const int64_t* step,
                            int64_t step_offset, int64_t learning_starts,
                            double exploration_noise, float* actions);
OCPPO_API int ocppo_td3_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                              int64_t offset, int64_t rows, int64_t A, int mode, float* out);
OCPPO_API int ocppo_td3_target_actions(ocppo_stream_t stream, const float* mu, int64_t B,
                                       int64_t D, int64_t A, const float* action_scale,
                                       const float* action_bias, uint64_t seed,
                                       const int64_t* counter, double policy_noise,
                                       double noise_clip, double low0, double high0,
                                       float* next_obs_act);
OCPPO_API int ocppo_td3_critic_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_next_target,
                                            const float* q2_next_target, const float* q1,
                                            const float* q2, const float* rewards,
                                            const float* dones, int64_t B, double gamma,
                                            float* dq1, float* dq2, float* stats, float* y_out);
OCPPO_API int ocppo_td3_policy_actions_fwd(ocppo_stream_t stream, const float* mu,
                                           const float* obs_act, int64_t B, int64_t D, int64_t A,
                                           const float* action_scale, const float* action_bias,
                                           float* xa, float* tanh_out);
OCPPO_API int ocppo_td3_policy_actions_bwd(ocppo_stream_t stream, const float* dxa,
                                           const float* tanh_in, int64_t B, int64_t D, int64_t A,
                                           const float* action_scale, float* dmu);
OCPPO_API int ocppo_polyak(ocppo_stream_t stream, int n_pairs, const float* const* params,
                           float* const* targets, const int64_t* numels, double tau);

/* ---------------------------------------------------------------------------------------------
 * Continuous SAC (cleanrl/sac_continuous_action.py), ABI 43: a tanh-squashed Gaussian policy over
 * float-vector actions, 1 <= A <= 64, on the TD3 block's replay and ocppo_polyak. All f32 unless
 * stated, no atomics (the batch sums are f64 in a fixed order: bitwise repeatable),
 * graph-capturable, one launch each. scale / bias / low / high are device arrays [A]; alpha is a
 * device f32 scalar.
 *
 * Draws: Philox4x32-10 and the TD3 block's Box-Muller; counter words 0, 1 = row * 64 + a, word 2 =
 *   the low 32 bits of the global step (acting) or of the replay's sample counter (updates), word 3
 *   = the draw index (acting 0; updates: 0 the target's draw, 1 + 2 i the policy's draw of
 *   iteration i, 2 + 2 i the temperature's), one key for acting and one for updates.
 *   ocppo_csac_noise writes them: mode 0 the acting z, mode 1 the uniform phase's u in [0, 1), both
 *   [rows, A] at t = counter[0] + offset; mode 2 the update stream's z of `draw` at sample counter
 *   counter[0] + offset.
 * ocppo_csac_act (:233-237) at global step t = step[0] + step_offset: t < learning_starts: uniform
 *   in [low, high) per dimension; else mean = hidden W_mean^T + b_mean, r = hidden W_logstd^T +
 *   b_logstd (hidden [E, H], H a multiple of 64, ocppo_td3_act's summation order), log_std = -5 +
 *   3.5 (tanh(r) + 1), action = tanh(mean + exp(log_std) z) * scale + bias.
 * ocppo_csac_sample_fwd (get_action, :138-150) from the heads' outputs mean, r [B, A] with the
 *   update stream's z of `draw` at counter[0]: xa[:, D:] = tanh(x) * scale + bias, x = mean +
 *   exp(log_std) z, into xa [B, D + A] (obs_act != NULL: its observation columns are copied into
 *   xa, which is another buffer; NULL: left as they are); log_prob [B] = sum_a (-z^2 / 2 - log_std -
 *   log sqrt(2 pi) - log(scale (1 - y^2) + 1e-6)), y = tanh(x), 1 - y^2 formed as 4 e / (1 + e)^2, e
 *   = exp(-2 |x|) (accurate at any x, where 1 - y * y from the rounded y is not), summed in column
 *   order; y_out,
 *   z_out, log_std_out [B, A] for the backward, or all three NULL. xa NULL: log_prob alone. z_in
 *   [B, A] != NULL: the draws are read from it (counter may then be NULL).
 * ocppo_csac_sample_bwd: dxa [B, D + A] (its action columns are read), dlogp [B], the forward's
 *   mean, r and outputs -> dmean, dr
 *   [B, A]. The (x - mean)^2 / (2 sigma^2) term has zero gradient under the reparameterisation and
 *   is not formed.
 * ocppo_csac_critic_loss_fwd_bwd (:264-275): y = r + ((1 - d) * gamma) * (min(q1t, q2t) - alpha *
 *   next_log_prob), dq = (2 / B)(q - y), stats [4] = {qf1_loss, qf2_loss, mean q1, mean q2}; y_out
 *   [B] or NULL. With alpha = 0 and q2 = q1 bitwise ocppo_td3_critic_loss_fwd_bwd's twin form.
 * ocppo_csac_actor_loss_fwd_bwd (:287-290): loss [1] = mean(alpha * log_prob - min(q1_pi, q2_pi)),
 *   dlogp [B] = (1 / B) * alpha, dq1 / dq2 [B]: -(1 / B) to the smaller input and, where q1_pi ==
 *   q2_pi, half of it to each (torch.min's backward).
 * ocppo_csac_alpha_step (:296-304): loss [1] = mean(-exp(log_alpha) * (log_prob + target_entropy)),
 *   torch.optim.Adam's step on log_alpha (exp_avg, exp_avg_sq [1] f32, adam_step [1] int64; the
 *   step scalars formed in double) and alpha = exp(log_alpha).
 * ------------------------------------------------------------------------------------------- */
OCPPO_API int ocppo_csac_act(ocppo_stream_t stream, const float* hidden, int64_t E, int64_t H,
                             const float* w_mean, const float* b_mean, const float* w_logstd,
                             const float* b_logstd, int64_t A, const float* action_scale,
                             const float* action_bias, const float* low, const float* high,
                             uint64_t seed, const int64_t* step, int64_t step_offset,
                             int64_t learning_starts, float* actions);
OCPPO_API int ocppo_csac_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                               int64_t offset, int64_t rows, int64_t A, int mode, int64_t draw,
                               float* out);
OCPPO_API int ocppo_csac_sample_fwd(ocppo_stream_t stream, const float* mean, const float* r,
                                    int64_t B, int64_t D, int64_t A, const float* action_scale,
                                    const float* action_bias, uint64_t seed,
                                    const int64_t* counter, int64_t draw, const float* z_in,
                                    const float* obs_act, float* xa, float* log_prob,
                                    float* y_out, float* z_out, float* log_std_out);
OCPPO_API int ocppo_csac_sample_bwd(ocppo_stream_t stream, const float* dxa, const float* dlogp,
                                    const float* mean, const float* r, const float* y,
                                    const float* z, const float* log_std, int64_t B, int64_t D,
                                    int64_t A, const float* action_scale, float* dmean,
                                    float* dr);
OCPPO_API int ocppo_csac_critic_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_next_target,
                                             const float* q2_next_target, const float* q1,
                                             const float* q2, const float* rewards,
                                             const float* dones, const float* next_log_prob,
                                             const float* alpha, int64_t B, double gamma,
                                             float* dq1, float* dq2, float* stats, float* y_out);
OCPPO_API int ocppo_csac_actor_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_pi,
                                            const float* q2_pi, const float* log_prob,
                                            const float* alpha, int64_t B, float* dq1, float* dq2,
                                            float* dlogp, float* loss);
OCPPO_API int ocppo_csac_alpha_step(ocppo_stream_t stream, const float* log_prob, int64_t B,
                                    float* alpha, float* log_alpha, double target_entropy,
                                    float* exp_avg, float* exp_avg_sq, int64_t* adam_step,
                                    double lr, double beta1, double beta2, double eps,
                                    float* loss);

/* ---------------------------------------------------------------------------------------------
 * MaDi's masker (architectures/madi.py MaskerNet with three layers; cleanrl/ppo_atari_madi.py:441,
 * :502), fused per image tile (ABI 44): y = x * sigmoid(conv3(relu(conv2(relu(conv1(x / 255)))))),
 * every frame of a stack on its own, 3x3 zero-padded convolutions 1 -> F -> F -> 1, F 16 or 32.
 *   src      : the frame stacks [rows, W, H, H], u8 or f32 (src_dtype OCPPO_U8 / OCPPO_F32)
 *   idx      : [B] int64 rows of src (an index outside [0, rows) is clamped into it, never
 *              dereferenced), or NULL: rows 0 .. B - 1
 *   w1 [F,1,3,3] b1 [F] w2 [F,F,3,3] b2 [F] w3 [1,F,3,3] b3 [1] : f32, contiguous
 *   out / g  : the masked stacks [B, W, H, H] f32 / their gradient, memory [B][W][H][H]
 *              (channels_last 0) or [B][H][H][W] (channels_last 1)
 * ocppo_madi_mask_fwd: one launch; the F-channel activations stay in LDS. The middle layer runs on
 *   v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation).
 * ocppo_madi_mask_bwd: dw1 .. db3 (shapes of w1 .. b3), the activations recomputed per tile; two
 *   launches, per-workgroup partial rows added in index order (no atomics: two calls on the same
 *   inputs are bitwise equal). workspace: ocppo_madi_workspace_bytes(F) = 256 rows of
 *   (9 F + F + 9 F F + F + 9 F + 1) floats, whatever the number of frames; 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
OCPPO_API size_t ocppo_madi_workspace_bytes(int64_t F);
OCPPO_API int ocppo_madi_mask_fwd(ocppo_stream_t stream, const void* src, int src_dtype,
                                  const int64_t* idx, int64_t rows, int64_t B, int64_t W,
                                  int64_t H, int64_t F, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* w3,
                                  const float* b3, int channels_last, float* out);
OCPPO_API int ocppo_madi_mask_bwd(ocppo_stream_t stream, const void* src, int src_dtype,
                                  const int64_t* idx, int64_t rows, int64_t B, int64_t W,
                                  int64_t H, int64_t F, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* w3,
                                  const float* b3, int channels_last, const float* g, float* dw1,
                                  float* db1, float* dw2, float* db2, float* dw3, float* db3,
                                  void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* OCPPO_H */
