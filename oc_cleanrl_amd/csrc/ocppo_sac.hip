// Discrete Soft Actor-Critic (cleanrl/sac_atari.py) on the DQN loop: the acting step (:248-252), the
// twin soft-Q target + the two MSE losses with their gradients (:283-302), and the policy loss,
// the temperature loss and the temperature's Adam step (:309-328), one launch each. alpha lives
// on the device: the actor launch writes exp(log_alpha) and the next critic launch reads it, so
// the train step needs no host round trip and stays inside the chunk's hipGraph.
// Row arithmetic in f32 (the acting draw's noise and the sums over the batch in f64), one workgroup
// per loss, no atomics: thread t takes rows t, t + 256, ... in order, then block_sum's fixed order.
#include "ocppo_common.h"
#include "ocppo_categorical.h"
#include "ocppo_rng.h"

namespace ocppo {

constexpr int kSacMaxA = 18;     // ops.C51_MAX_ACTIONS (the full ALE action set)
constexpr int kSacThreads = 256;  // the loss kernels' one workgroup
// the acting stream's key: h_t = splitmix64(splitmix64(seed ^ key) + t), env e's hash
// h_e = splitmix64(h_t + e + 1); the random phase's action is h_e % A, the sampling phase's
// noise is e_j = -log(1 - unit53(splitmix64(h_e + j + 1)))
constexpr uint64_t kSacActKey = 0x5AC0D15C2E7E5EEDull;

// One row of Categorical(logits): probs as torch.distributions forms them (categorical_row) and
// log_pi = F.log_softmax(logits) in its own op order, (l - max) - log(sum exp(l - max)).
__device__ __forceinline__ void sac_row(const float* __restrict__ logits, int64_t b, int A,
                                        float (&p)[kSacMaxA], float (&logp)[kSacMaxA]) {
  float l[kSacMaxA], ln[kSacMaxA], lse;
#pragma unroll
  for (int j = 0; j < kSacMaxA; ++j) l[j] = j < A ? logits[b * A + j] : 0.f;
  categorical_row<kSacMaxA>(l, A, lse, ln, p);
  float m = l[0];
#pragma unroll
  for (int j = 1; j < kSacMaxA; ++j)
    if (j < A) m = fmaxf(m, l[j]);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kSacMaxA; ++j)
    if (j < A) s += expf(l[j] - m);
  const float ls = logf(s);
#pragma unroll
  for (int j = 0; j < kSacMaxA; ++j) logp[j] = j < A ? (l[j] - m) - ls : 0.f;
}

// ---- critic: soft target + twin MSE ----------------------------------------------------------------
//   v_b = sum_j p'_bj * (min(q1t_bj, q2t_bj) - alpha * logp'_bj)
//   y_b = r_b + ((1 - d_b) * gamma) * v_b
//   qf{1,2}_loss = mean_b (q{1,2}[b, a_b] - y_b)^2;  dq = (2 / B)(q[b, a_b] - y_b) at a_b, else 0
__global__ __launch_bounds__(kSacThreads) void sac_critic_kernel(
    const float* __restrict__ next_logits, const float* __restrict__ q1t,
    const float* __restrict__ q2t, const float* __restrict__ q1, const float* __restrict__ q2,
    const int64_t* __restrict__ actions, const float* __restrict__ rewards,
    const float* __restrict__ dones, int64_t B, int A, float gamma, const float* __restrict__ alpha_p,
    float norm, float* __restrict__ dq1, float* __restrict__ dq2, float* __restrict__ stats,
    float* __restrict__ y_out) {
  __shared__ double scratch[kSacThreads / kWave];
  const float alpha = alpha_p[0];
  // the batch sums run in f64 (a mean of Q values near zero cancels): each result is the f32
  // nearest to the sum of the f32 terms
  double se1 = 0.0, se2 = 0.0, sq1 = 0.0, sq2 = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += kSacThreads) {
    float p[kSacMaxA], logp[kSacMaxA];
    sac_row(next_logits, b, A, p, logp);
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < kSacMaxA; ++j)
      if (j < A) v += p[j] * (fminf(q1t[b * A + j], q2t[b * A + j]) - alpha * logp[j]);
    const float y = rewards[b] + ((1.0f - dones[b]) * gamma) * v;
    if (y_out) y_out[b] = y;
    int64_t a = actions[b];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);  // an action outside [0, A) reads no memory
    const float o1 = q1[b * A + a], o2 = q2[b * A + a];
    const float d1 = o1 - y, d2 = o2 - y;
    se1 += d1 * d1;
    se2 += d2 * d2;
    sq1 += o1;
    sq2 += o2;
    const float g1 = d1 * norm, g2 = d2 * norm;
    for (int j = 0; j < A; ++j) {
      dq1[b * A + j] = j == a ? g1 : 0.f;
      dq2[b * A + j] = j == a ? g2 : 0.f;
    }
  }
  se1 = block_sum(se1, scratch);
  se2 = block_sum(se2, scratch);
  sq1 = block_sum(sq1, scratch);
  sq2 = block_sum(sq2, scratch);
  if (threadIdx.x == 0) {
    const double fb = static_cast<double>(B);
    stats[0] = static_cast<float>(se1 / fb);  // losses/qf1_loss
    stats[1] = static_cast<float>(se2 / fb);  // losses/qf2_loss
    stats[2] = static_cast<float>(sq1 / fb);  // losses/qf1_values
    stats[3] = static_cast<float>(sq2 / fb);  // losses/qf2_values
  }
}

// ---- actor + temperature -----------------------------------------------------------------------------
//   g_bj = alpha * logp_bj - min(q1_bj, q2_bj);  s_b = sum_j p_bj g_bj
//   actor_loss = sum_b s_b / (B A);  dlogits_bk = p_bk (g_bk - s_b) / (B A)
// (d/dl_k of sum_j p_j g_j = p_k (g_k - s) + alpha sum_j p_j (delta_jk - p_k) = p_k (g_k - s): the
// alpha * p * dlogp terms sum to zero)
//   alpha_loss = sum_bj p_bj * (-exp(log_alpha) * (logp_bj + target_entropy)) / (B A)
// autotune: torch.optim.Adam's single-tensor step on log_alpha with
//   grad = exp(log_alpha) * (-sum_bj p_bj (logp_bj + target_entropy) / (B A))
// then alpha = exp(log_alpha).
struct SacAdam {
  float* exp_avg;
  float* exp_avg_sq;
  int64_t* step;
  double lr, beta1, beta2, eps;
};

__global__ __launch_bounds__(kSacThreads) void sac_actor_kernel(
    const float* __restrict__ logits, const float* __restrict__ q1, const float* __restrict__ q2,
    int64_t B, int A, float* alpha_p, float* log_alpha_p, float target_entropy, SacAdam ad,
    int autotune, float* __restrict__ dlogits, float* __restrict__ stats) {
  __shared__ double scratch[kSacThreads / kWave];
  const float alpha = alpha_p[0];
  const float log_alpha = log_alpha_p[0];
  const float ea = expf(log_alpha);
  const float inv = 1.0f / (static_cast<float>(B) * static_cast<float>(A));
  const double n = static_cast<double>(B) * static_cast<double>(A);
  double sl = 0.0, sal = 0.0, st = 0.0, sh = 0.0;  // batch sums in f64, as the critic's
  for (int64_t b = threadIdx.x; b < B; b += kSacThreads) {
    float p[kSacMaxA], logp[kSacMaxA], g[kSacMaxA];
    sac_row(logits, b, A, p, logp);
    // the four reported sums (and through `st` the temperature's gradient) take the row's softmax
    // in f64 from the logits: the policy loss is a sum whose terms alpha * logp and min q cancel,
    // and f32 p and logp (a few 1e-7 each) leave up to 1e-6 of it. The gradient below keeps the
    // f32 p and logp of the reference.
    double lmax = logits[b * A], ssum = 0.0;
    for (int j = 1; j < A; ++j) lmax = fmax(lmax, static_cast<double>(logits[b * A + j]));
    for (int j = 0; j < A; ++j) ssum += exp(static_cast<double>(logits[b * A + j]) - lmax);
    const double lsum = log(ssum);
#pragma unroll
    for (int j = 0; j < kSacMaxA; ++j)
      if (j < A) {
        const float mq = fminf(q1[b * A + j], q2[b * A + j]);
        g[j] = alpha * logp[j] - mq;
        const double ld = (static_cast<double>(logits[b * A + j]) - lmax) - lsum;
        const double pd = exp(ld);
        const double lt = ld + static_cast<double>(target_entropy);
        sl += pd * (static_cast<double>(alpha) * ld - static_cast<double>(mq));
        sal += pd * (-static_cast<double>(ea) * lt);
        st += pd * lt;
        sh += pd * ld;
      }
    // p_k (g_k - sum_j p_j g_j) as p_k sum_j p_j (g_k - g_j): equal when sum_j p_j = 1, and free
    // of the cancellation g_k - s that turns the rounding of the p's sum into the whole result
    // where p_k is near 1
#pragma unroll
    for (int k = 0; k < kSacMaxA; ++k)
      if (k < A) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kSacMaxA; ++j)
          if (j < A) acc += p[j] * (g[k] - g[j]);
        dlogits[b * A + k] = (p[k] * acc) * inv;
      }
  }
  sl = block_sum(sl, scratch);
  sal = block_sum(sal, scratch);
  st = block_sum(st, scratch);
  sh = block_sum(sh, scratch);
  if (threadIdx.x != 0) return;
  float alpha_new = alpha;
  if (autotune) {
    const float grad = ea * (-static_cast<float>(st / n));
    const int64_t t = ad.step[0] + 1;
    float m = ad.exp_avg[0], v = ad.exp_avg_sq[0];
    m = m + static_cast<float>(1.0 - ad.beta1) * (grad - m);  // lerp_(grad, 1 - beta1)
    v = v * static_cast<float>(ad.beta2) +
        (static_cast<float>(1.0 - ad.beta2) * grad) * grad;   // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const double bc1 = 1.0 - pow(ad.beta1, static_cast<double>(t));
    const double bc2 = 1.0 - pow(ad.beta2, static_cast<double>(t));
    const float step_size = static_cast<float>(ad.lr / bc1);
    const float denom = sqrtf(v) / static_cast<float>(sqrt(bc2)) + static_cast<float>(ad.eps);
    const float la = log_alpha + ((-step_size) * m) / denom;  // addcdiv_(m, denom, -step_size)
    ad.exp_avg[0] = m;
    ad.exp_avg_sq[0] = v;
    ad.step[0] = t;
    log_alpha_p[0] = la;
    alpha_new = expf(la);
    alpha_p[0] = alpha_new;
  }
  stats[0] = static_cast<float>(sl / n);                    // losses/actor_loss
  stats[1] = autotune ? static_cast<float>(sal / n) : 0.f;  // losses/alpha_loss
  stats[2] = alpha_new;  // losses/alpha (after the update, as the script logs)
  stats[3] = static_cast<float>(-sh / static_cast<double>(B));  // mean policy entropy
}

// ---- acting ------------------------------------------------------------------------------------------
// t < learning_starts: uniform in [0, A). Otherwise one draw of Categorical(logits) by the
// exponential race: argmax_j p_j / e_j (first maximum; a NaN counts as the maximum), e_j ~ Exp(1).
__global__ __launch_bounds__(256) void sac_act_kernel(
    const float* __restrict__ logits, int64_t E, int A, uint64_t seed,
    const int64_t* __restrict__ step, int64_t step_offset, int64_t learning_starts,
    int64_t* __restrict__ actions) {
  const int64_t t = step[0] + step_offset;
  const uint64_t ht = splitmix64(splitmix64(seed ^ kSacActKey) + static_cast<uint64_t>(t));
  const bool random = t < learning_starts;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < E;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint64_t he = splitmix64(ht + static_cast<uint64_t>(e) + 1);
    if (random) {
      actions[e] = static_cast<int64_t>(he % static_cast<uint64_t>(A));
      continue;
    }
    float p[kSacMaxA], logp[kSacMaxA];
    sac_row(logits, e, A, p, logp);
    int best = 0;
    double bv = 0.0;
    for (int j = 0; j < A; ++j) {
      const double ej = -log(1.0 - unit53(splitmix64(he + static_cast<uint64_t>(j) + 1)));
      double pj = 0.0;
#pragma unroll
      for (int k = 0; k < kSacMaxA; ++k)
        if (k == j) pj = static_cast<double>(p[k]);
      const double r = pj / ej;
      if (j == 0 || r > bv || (r != r && bv == bv)) {
        bv = r;
        best = j;
      }
    }
    actions[e] = best;
  }
}

static int sac_sizes(const char* who, int64_t B, int64_t A) {
  OCPPO_REQUIRE(A >= 1 && A <= kSacMaxA && B >= 0,
                "%s: bad sizes B=%lld A=%lld (B >= 0, 1 <= A <= %d)", who, (long long)B,
                (long long)A, kSacMaxA);
  return OCPPO_OK;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_sac_critic_loss_fwd_bwd(
    ocppo_stream_t stream, const float* next_logits, const float* q1_next_target,
    const float* q2_next_target, const float* q1, const float* q2, const int64_t* actions,
    const float* rewards, const float* dones, int64_t B, int64_t A, double gamma,
    const float* alpha, float* dq1, float* dq2, float* stats, float* y_out) {
  if (int rc = sac_sizes("ocppo_sac_critic_loss_fwd_bwd", B, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(next_logits && q1_next_target && q2_next_target && q1 && q2 && actions &&
                    rewards && dones && alpha && dq1 && dq2 && stats,
                "ocppo_sac_critic_loss_fwd_bwd: null pointer");
  clear_stale_error();
  // mse_loss backward: norm = 2 / numel (computed in double by ATen, applied in f32)
  const float norm = static_cast<float>(2.0 / static_cast<double>(B));
  hipLaunchKernelGGL(sac_critic_kernel, dim3(1), dim3(kSacThreads), 0, as_stream(stream),
                     next_logits, q1_next_target, q2_next_target, q1, q2, actions, rewards, dones,
                     B, (int)A, static_cast<float>(gamma), alpha, norm, dq1, dq2, stats, y_out);
  return check_launch("ocppo_sac_critic_loss_fwd_bwd");
}

extern "C" int ocppo_sac_actor_alpha_fwd_bwd(
    ocppo_stream_t stream, const float* logits, const float* q1, const float* q2, int64_t B,
    int64_t A, float* alpha, float* log_alpha, double target_entropy, float* exp_avg,
    float* exp_avg_sq, int64_t* adam_step, double lr, double beta1, double beta2, double eps,
    int autotune, float* dlogits, float* stats) {
  if (int rc = sac_sizes("ocppo_sac_actor_alpha_fwd_bwd", B, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(logits && q1 && q2 && alpha && log_alpha && dlogits && stats &&
                    (!autotune || (exp_avg && exp_avg_sq && adam_step)),
                "ocppo_sac_actor_alpha_fwd_bwd: null pointer");
  OCPPO_REQUIRE(!autotune || (lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 &&
                              eps >= 0),
                "ocppo_sac_actor_alpha_fwd_bwd: bad Adam constants");
  clear_stale_error();
  const SacAdam ad{exp_avg, exp_avg_sq, adam_step, lr, beta1, beta2, eps};
  hipLaunchKernelGGL(sac_actor_kernel, dim3(1), dim3(kSacThreads), 0, as_stream(stream), logits,
                     q1, q2, B, (int)A, alpha, log_alpha, static_cast<float>(target_entropy), ad,
                     autotune ? 1 : 0, dlogits, stats);
  return check_launch("ocppo_sac_actor_alpha_fwd_bwd");
}

extern "C" int ocppo_sac_act(ocppo_stream_t stream, const float* logits, int64_t E, int64_t A,
                             uint64_t seed, const int64_t* step, int64_t step_offset,
                             int64_t learning_starts, int64_t* actions) {
  if (int rc = sac_sizes("ocppo_sac_act", E, A)) return rc;
  if (E == 0) return OCPPO_OK;
  OCPPO_REQUIRE(logits && step && actions, "ocppo_sac_act: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(sac_act_kernel, dim3(grid_for(E, 256)), dim3(256), 0, as_stream(stream),
                     logits, E, (int)A, seed, step, step_offset, learning_starts, actions);
  return check_launch("ocppo_sac_act");
}
