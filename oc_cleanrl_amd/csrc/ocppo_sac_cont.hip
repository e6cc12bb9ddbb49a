// Continuous SAC (cleanrl/sac_continuous_action.py): a tanh-squashed Gaussian policy over
// float-vector actions of A <= 64 dimensions, on ocppo_td3.hip's replay and soft update.
// Everything around the three MLPs' GEMMs that TD3 does not already have:
//   csac_act                  both heads + both acting phases (:233-237), the branch on the device
//   csac_sample_fwd / _bwd    get_action (:138-150) from the heads' outputs: the reparameterised
//                             draw, the squash, the action into the critics' input, log_prob
//   csac_critic_loss_fwd_bwd  min - alpha * logp', TD target, both MSEs, dq1 / dq2 (:264-275)
//   csac_actor_loss_fwd_bwd   mean(alpha * logp - min(q1, q2)) and its gradients (:287-290)
//   csac_alpha_step           alpha_loss, log_alpha's Adam step, alpha = exp(log_alpha) (:296-304)
// ocppo_td3.hip's conventions: f32 row arithmetic in torch's op order (no contraction), batch sums
// in f64 in a fixed order (thread t takes rows t, t + 256, ..., then block_sum), no atomics, int64
// row offsets, plain vector stores.
//
// Streams (counter-based Philox4x32-10, ocppo_contq.h's Box-Muller). The 128-bit counter is
//   words 0, 1   row * 64 + a (row: the env e or the batch row b)
//   word 2       the low 32 bits of the global step t (acting) or of the replay's sample counter
//   word 3       the draw index: 0 acting; in an update 0 = the target's draw (:265), 1 + 2 i = the
//                policy's draw of iteration i (:286), 2 + 2 i = the temperature's fresh draw (:298)
// under key seed ^ kCsacActKey (acting: word 0 -> the uniform phase's u, words 0, 1 -> z) or
// seed ^ kCsacUpdateKey (updates), so no two draws of a step coincide.
//
// min's gradient (csac_actor_loss): torch.min(a, b)'s backward gives the whole gradient to the
// smaller input and, where a == b, half to each (checked against autograd on the CPU by
// tests/test_sac_continuous_cpu.py).
#include "ocppo_contq.h"

namespace ocppo {

constexpr uint64_t kCsacActKey = 0x5AC0C7A1D3E2F481ull;
constexpr uint64_t kCsacUpdateKey = 0x5AC0D9B7E6A3C215ull;
constexpr float kLogStdMin = -5.0f;                      // LOG_STD_MIN (:102)
constexpr float kLogStdHalfRange = 3.5f;                 // 0.5 * (LOG_STD_MAX - LOG_STD_MIN) (:134)
constexpr float kHalfLog2Pi = 0.91893853320467274178f;   // math.log(math.sqrt(2 * math.pi))
constexpr float kSquashEps = 1e-6f;                      // :147

__device__ __forceinline__ uint4 csac_words(uint64_t key, int64_t ctr, int64_t draw, int64_t row,
                                            int a) {
  const uint64_t sub = (static_cast<uint64_t>(draw) << 32) |
                       (static_cast<uint64_t>(ctr) & 0xFFFFFFFFull);
  return philox_block(key, sub, static_cast<uint64_t>(row) * 64 + static_cast<uint64_t>(a));
}

__device__ __forceinline__ float csac_z(uint64_t key, int64_t ctr, int64_t draw, int64_t row,
                                        int a) {
  const uint4 w = csac_words(key, ctr, draw, row, a);
  return box_muller(w.x, w.y);
}

// 1 - tanh(x)^2 as 4 e / (1 + e)^2 with e = exp(-2 |x|): the same number to f32 rounding at any x,
// where 1 - y * y from the rounded y = tanh(x) is decided by y's last bit once |x| passes ~3 (and
// is 0 past |x| ~ 9, which makes log_prob's squash term the constant log(1e-6) there)
__device__ __forceinline__ float one_minus_tanh2(float x) {
  const float e = expf(-2.0f * fabsf(x));
  const float q = 1.0f + e;
  return (4.0f * e) / (q * q);
}

// log_std = LOG_STD_MIN + 0.5 (LOG_STD_MAX - LOG_STD_MIN) (tanh(r) + 1) (:133-134)
__device__ __forceinline__ float csac_log_std(float tanh_r) {
  return kLogStdMin + kLogStdHalfRange * (tanh_r + 1.0f);
}

// ---- acting ------------------------------------------------------------------------------------------
// One wave per env, as td3_act: head[a] = sum_j h[e, j] w[a, j] + b[a] with lane l adding j = l,
// l + 64, ... in order and the lanes combined by wave_sum's butterfly (td3.act_mu's order), for
// fc_mean and then fc_logstd.
__global__ __launch_bounds__(kWave) void csac_act_kernel(
    const float* __restrict__ hidden, int64_t E, int64_t H, const float* __restrict__ w_mean,
    const float* __restrict__ b_mean, const float* __restrict__ w_ls,
    const float* __restrict__ b_ls, int A, const float* __restrict__ scale,
    const float* __restrict__ abias, const float* __restrict__ low, const float* __restrict__ high,
    uint64_t seed, const int64_t* __restrict__ step, int64_t step_offset, int64_t learning_starts,
    float* __restrict__ actions) {
  const int64_t t = step[0] + step_offset;
  const bool random = t < learning_starts;
  const int lane = threadIdx.x;
  for (int64_t e = blockIdx.x; e < E; e += gridDim.x) {
    float mean = 0.f, r = 0.f;
    if (!random) {
      for (int a = 0; a < A; ++a) {
        float am = 0.f, ar = 0.f;
        for (int64_t j = lane; j < H; j += kWave) {
          const float h = hidden[e * H + j];
          am += h * w_mean[a * H + j];
          ar += h * w_ls[a * H + j];
        }
        am = wave_sum(am);
        ar = wave_sum(ar);
        if (lane == a) {
          mean = am + b_mean[a];
          r = ar + b_ls[a];
        }
      }
    }
    if (lane >= A) continue;
    const uint4 w = csac_words(seed ^ kCsacActKey, t, 0, e, lane);
    float v;
    if (random) {
      const float lo = low[lane], hi = high[lane];
      v = lo + (hi - lo) * unit24(w.x);
      if (v >= hi) v = nextafterf(hi, lo);  // the last product may round up to the bound
    } else {
      const float x = mean + expf(csac_log_std(tanhf(r))) * box_muller(w.x, w.y);
      v = tanhf(x) * scale[lane] + abias[lane];
    }
    actions[e * A + lane] = v;
  }
}

// mode 0: the acting stream's z [E, A]; 1: its uniform u; 2: the update stream's z [B, A] of `draw`
__global__ __launch_bounds__(kTd3Threads) void csac_draws_kernel(
    uint64_t seed, const int64_t* __restrict__ counter, int64_t offset, int64_t R, int A, int mode,
    int64_t draw, float* __restrict__ out) {
  const int64_t c = counter[0] + offset;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < R * A;
       g += stride) {
    const int64_t r = g / A;
    const int a = static_cast<int>(g - r * A);
    if (mode == 2) {
      out[g] = csac_z(seed ^ kCsacUpdateKey, c, draw, r, a);
    } else {
      const uint4 x = csac_words(seed ^ kCsacActKey, c, 0, r, a);
      out[g] = mode == 1 ? unit24(x.x) : box_muller(x.x, x.y);
    }
  }
}

// ---- get_action (:138-150) from the heads' outputs ----------------------------------------------------
// One thread per row; per column a, in order:
//   log_std = -5 + 3.5 (tanh(r) + 1);  x = mean + exp(log_std) z;  y = tanh(x)
//   xa[b, D + a] = y * scale + bias
//   log_prob_b += ((-(z z) 0.5 - log_std) - log sqrt(2 pi)) - log(scale (1 - y^2) + 1e-6)
// with 1 - y^2 = one_minus_tanh2(x).
// Normal.log_prob's (x - mean)^2 / (2 sigma^2) is z^2 / 2 under the reparameterisation and its
// log(sigma) is log_std. z_in != null: the draws are read from it, not from the stream. obs_act != null: xa's observation columns are copied from it. xa, y_out /
// z_out / ls_out null: not written (the forward-only mode: log_prob alone).
__global__ __launch_bounds__(kTd3Threads) void csac_sample_fwd_kernel(
    const float* __restrict__ mean, const float* __restrict__ r, int64_t B, int64_t D, int A,
    const float* __restrict__ scale, const float* __restrict__ abias, uint64_t seed,
    const int64_t* __restrict__ counter, int64_t draw, const float* __restrict__ z_in,
    const float* __restrict__ obs_act, float* __restrict__ xa, float* __restrict__ logp,
    float* __restrict__ y_out, float* __restrict__ z_out, float* __restrict__ ls_out) {
  const int64_t ctr = z_in ? 0 : counter[0];
  const int64_t W = D + A;
  const uint64_t key = seed ^ kCsacUpdateKey;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; b < B;
       b += stride) {
    if (xa && obs_act)
      for (int64_t c = 0; c < D; ++c) xa[b * W + c] = obs_act[b * W + c];
    float lp = 0.f;
    for (int a = 0; a < A; ++a) {
      const int64_t g = b * A + a;
      const float z = z_in ? z_in[g] : csac_z(key, ctr, draw, b, a);
      const float ls = csac_log_std(tanhf(r[g]));
      const float x = mean[g] + expf(ls) * z;
      const float y = tanhf(x);
      if (xa) xa[b * W + D + a] = y * scale[a] + abias[a];
      const float u = scale[a] * one_minus_tanh2(x) + kSquashEps;
      const float term = ((-(z * z) * 0.5f - ls) - kHalfLog2Pi) - logf(u);
      lp += term;
      if (y_out) {
        y_out[g] = y;
        z_out[g] = z;
        ls_out[g] = ls;
      }
    }
    logp[b] = lp;
  }
}

// One thread per element. With x = mean + exp(log_std) z, s2 = one_minus_tanh2(x) and u = scale s2 +
// 1e-6 (the forward's values):
//   gy = dxa * scale + ((dlogp / u) * scale) * (2 y)      mul's backward + log's, mul's, pow's
//   gx = gy * s2                                          tanh's backward
//   dmean = gx;   dlog_std = (gx * z) * exp(log_std) - dlogp
//   dr = (dlog_std * 3.5) * (1 - t * t), t = tanh(r)
// every operation rounded on its own, so that sac_continuous.SquashTorch's backward, the same
// expressions in torch ops, is bitwise this kernel.
// The (x - mean)^2 / (2 sigma^2) term of Normal.log_prob contributes exactly zero to both (autograd
// forms it as a cancelling pair).
__global__ __launch_bounds__(kTd3Threads) void csac_sample_bwd_kernel(
    const float* __restrict__ dxa, const float* __restrict__ dlogp,
    const float* __restrict__ mean, const float* __restrict__ r, const float* __restrict__ y_in, const float* __restrict__ z_in,
    const float* __restrict__ ls_in, int64_t B, int64_t D, int A, const float* __restrict__ scale,
    float* __restrict__ dmean, float* __restrict__ dr) {
  const int64_t W = D + A;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < B * A;
       g += stride) {
    const int64_t b = g / A;
    const int a = static_cast<int>(g - b * A);
    const float y = y_in[g], sc = scale[a], dl = dlogp[b];
    const float z = z_in[g], sigma = expf(ls_in[g]);
    const float s2 = one_minus_tanh2(mean[g] + sigma * z);
    const float u = sc * s2 + kSquashEps;
    const float gy = dxa[b * W + D + a] * sc + ((dl / u) * sc) * (2.0f * y);
    const float gx = gy * s2;
    dmean[g] = gx;
    const float dls = (gx * z) * sigma - dl;
    const float t = tanhf(r[g]);
    dr[g] = (dls * kLogStdHalfRange) * (1.0f - t * t);
  }
}

// ---- critic (:264-275) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTd3Threads) void csac_critic_kernel(
    const float* __restrict__ q1t, const float* __restrict__ q2t, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ rewards,
    const float* __restrict__ dones, const float* __restrict__ logp,
    const float* __restrict__ alpha, int64_t B, float gamma, float norm, float* __restrict__ dq1,
    float* __restrict__ dq2, float* __restrict__ stats, float* __restrict__ y_out) {
  __shared__ double scratch[kTd3Threads / kWave];
  critic_loss_rows<true>(q1t, q2t, q1, q2, rewards, dones, logp, alpha[0], B, gamma, norm, dq1, dq2,
                         stats, y_out, scratch);
}

// ---- actor loss (:287-290) --------------------------------------------------------------------------------
//   actor_loss = mean_b (alpha * logp_b - min(q1_b, q2_b))
//   dlogp_b = (1 / B) * alpha;  dq = -(1 / B) to the smaller input, -(1 / B) / 2 to each where equal
__global__ __launch_bounds__(kTd3Threads) void csac_actor_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ logp,
    const float* __restrict__ alpha_p, int64_t B, float* __restrict__ dq1, float* __restrict__ dq2,
    float* __restrict__ dlogp, float* __restrict__ loss) {
  __shared__ double scratch[kTd3Threads / kWave];
  const float alpha = alpha_p[0];
  const float inv = 1.0f / static_cast<float>(B);
  const float dl = inv * alpha;
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += kTd3Threads) {
    const float a = q1[b], c = q2[b];
    s += static_cast<double>(alpha * logp[b] - fminf(a, c));
    const float g = a == c ? -inv / 2.0f : -inv;
    dq1[b] = a > c ? 0.f : g;
    dq2[b] = a < c ? 0.f : g;
    dlogp[b] = dl;
  }
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) loss[0] = static_cast<float>(s / static_cast<double>(B));
}

// ---- temperature (:296-304) -------------------------------------------------------------------------------
//   alpha_loss = mean_b (-exp(log_alpha) * (logp_b + target_entropy))
//   grad = -exp(log_alpha) * mean_b (logp_b + target_entropy), then torch.optim.Adam's
//   single-tensor step on log_alpha with its step scalars formed in double (as
//   ocppo_clip_adam_step_exact), then alpha = exp(log_alpha).
struct CsacAdam {
  float* exp_avg;
  float* exp_avg_sq;
  int64_t* step;
  double lr, beta1, beta2, eps;
};

__global__ __launch_bounds__(kTd3Threads) void csac_alpha_kernel(
    const float* __restrict__ logp, int64_t B, float* alpha_p, float* log_alpha_p,
    float target_entropy, CsacAdam ad, float* __restrict__ loss) {
  __shared__ double scratch[kTd3Threads / kWave];
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += kTd3Threads)
    s += static_cast<double>(logp[b] + target_entropy);
  s = block_sum(s, scratch);
  if (threadIdx.x != 0) return;
  const float log_alpha = log_alpha_p[0];
  const float ea = expf(log_alpha);
  const double mean = s / static_cast<double>(B);
  loss[0] = static_cast<float>(-static_cast<double>(ea) * mean);
  const float grad = -ea * static_cast<float>(mean);
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
  alpha_p[0] = expf(la);
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_csac_act(ocppo_stream_t stream, const float* hidden, int64_t E, int64_t H,
                              const float* w_mean, const float* b_mean, const float* w_logstd,
                              const float* b_logstd, int64_t A, const float* action_scale,
                              const float* action_bias, const float* low, const float* high,
                              uint64_t seed, const int64_t* step, int64_t step_offset,
                              int64_t learning_starts, float* actions) {
  if (int rc = td3_sizes("ocppo_csac_act", E, H, A)) return rc;
  OCPPO_REQUIRE(H % kWave == 0, "ocppo_csac_act: H=%lld is not a multiple of %d", (long long)H,
                kWave);
  if (E == 0) return OCPPO_OK;
  OCPPO_REQUIRE(hidden && w_mean && b_mean && w_logstd && b_logstd && action_scale &&
                    action_bias && low && high && step && actions,
                "ocppo_csac_act: null pointer");
  clear_stale_error();
  const int64_t g = E < 4096 ? E : 4096;
  hipLaunchKernelGGL(csac_act_kernel, dim3(g), dim3(kWave), 0, as_stream(stream), hidden, E, H,
                     w_mean, b_mean, w_logstd, b_logstd, (int)A, action_scale, action_bias, low,
                     high, seed, step, step_offset, learning_starts, actions);
  return check_launch("ocppo_csac_act");
}

extern "C" int ocppo_csac_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                                int64_t offset, int64_t rows, int64_t A, int mode, int64_t draw,
                                float* out) {
  if (int rc = td3_sizes("ocppo_csac_noise", rows, 1, A)) return rc;
  OCPPO_REQUIRE(mode >= 0 && mode <= 2, "ocppo_csac_noise: mode %d (0 acting z, 1 acting u, 2 "
                "update z)", mode);
  OCPPO_REQUIRE(draw >= 0 && draw <= 0xFFFFFFFFll, "ocppo_csac_noise: draw index %lld",
                (long long)draw);
  if (rows == 0) return OCPPO_OK;
  OCPPO_REQUIRE(counter && out, "ocppo_csac_noise: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(csac_draws_kernel, dim3(grid_for(rows * A, kTd3Threads)), dim3(kTd3Threads),
                     0, as_stream(stream), seed, counter, offset, rows, (int)A, mode, draw, out);
  return check_launch("ocppo_csac_noise");
}

extern "C" int ocppo_csac_sample_fwd(ocppo_stream_t stream, const float* mean, const float* r,
                                     int64_t B, int64_t D, int64_t A, const float* action_scale,
                                     const float* action_bias, uint64_t seed,
                                     const int64_t* counter, int64_t draw, const float* z_in,
                                     const float* obs_act, float* xa, float* log_prob,
                                     float* y_out, float* z_out, float* log_std_out) {
  if (int rc = td3_sizes("ocppo_csac_sample_fwd", B, D, A)) return rc;
  OCPPO_REQUIRE(draw >= 0 && draw <= 0xFFFFFFFFll, "ocppo_csac_sample_fwd: draw index %lld",
                (long long)draw);
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(mean && r && action_scale && action_bias && (counter || z_in) && log_prob,
                "ocppo_csac_sample_fwd: null pointer (counter may be null only with z_in)");
  OCPPO_REQUIRE((y_out == nullptr) == (z_out == nullptr) && (y_out == nullptr) == (log_std_out == nullptr),
                "ocppo_csac_sample_fwd: y_out, z_out and log_std_out come together");
  OCPPO_REQUIRE(obs_act == nullptr || (xa != nullptr && xa != obs_act),
                "ocppo_csac_sample_fwd: obs_act is copied into another buffer xa");
  clear_stale_error();
  hipLaunchKernelGGL(csac_sample_fwd_kernel, dim3(grid_for(B, kTd3Threads)), dim3(kTd3Threads), 0,
                     as_stream(stream), mean, r, B, D, (int)A, action_scale, action_bias, seed,
                     counter, draw, z_in, obs_act, xa, log_prob, y_out, z_out, log_std_out);
  return check_launch("ocppo_csac_sample_fwd");
}

extern "C" int ocppo_csac_sample_bwd(ocppo_stream_t stream, const float* dxa, const float* dlogp,
                                     const float* mean, const float* r, const float* y,
                                     const float* z, const float* log_std, int64_t B, int64_t D,
                                     int64_t A, const float* action_scale, float* dmean,
                                     float* dr) {
  if (int rc = td3_sizes("ocppo_csac_sample_bwd", B, D, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dxa && dlogp && mean && r && y && z && log_std && action_scale && dmean && dr,
                "ocppo_csac_sample_bwd: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(csac_sample_bwd_kernel, dim3(grid_for(B * A, kTd3Threads)),
                     dim3(kTd3Threads), 0, as_stream(stream), dxa, dlogp, mean, r, y, z, log_std, B, D,
                     (int)A, action_scale, dmean, dr);
  return check_launch("ocppo_csac_sample_bwd");
}

extern "C" int ocppo_csac_critic_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_next_target,
                                              const float* q2_next_target, const float* q1,
                                              const float* q2, const float* rewards,
                                              const float* dones, const float* next_log_prob,
                                              const float* alpha, int64_t B, double gamma,
                                              float* dq1, float* dq2, float* stats, float* y_out) {
  OCPPO_REQUIRE(B >= 0, "ocppo_csac_critic_loss_fwd_bwd: bad size B=%lld", (long long)B);
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(q1_next_target && q2_next_target && q1 && q2 && rewards && dones &&
                    next_log_prob && alpha && dq1 && dq2 && stats,
                "ocppo_csac_critic_loss_fwd_bwd: null pointer");
  clear_stale_error();
  const float norm = static_cast<float>(2.0 / static_cast<double>(B));  // mse_loss's backward
  hipLaunchKernelGGL(csac_critic_kernel, dim3(1), dim3(kTd3Threads), 0, as_stream(stream),
                     q1_next_target, q2_next_target, q1, q2, rewards, dones, next_log_prob, alpha,
                     B, static_cast<float>(gamma), norm, dq1, dq2, stats, y_out);
  return check_launch("ocppo_csac_critic_loss_fwd_bwd");
}

extern "C" int ocppo_csac_actor_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_pi,
                                             const float* q2_pi, const float* log_prob,
                                             const float* alpha, int64_t B, float* dq1, float* dq2,
                                             float* dlogp, float* loss) {
  OCPPO_REQUIRE(B >= 0, "ocppo_csac_actor_loss_fwd_bwd: bad size B=%lld", (long long)B);
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(q1_pi && q2_pi && log_prob && alpha && dq1 && dq2 && dlogp && loss,
                "ocppo_csac_actor_loss_fwd_bwd: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(csac_actor_kernel, dim3(1), dim3(kTd3Threads), 0, as_stream(stream), q1_pi,
                     q2_pi, log_prob, alpha, B, dq1, dq2, dlogp, loss);
  return check_launch("ocppo_csac_actor_loss_fwd_bwd");
}

extern "C" int ocppo_csac_alpha_step(ocppo_stream_t stream, const float* log_prob, int64_t B,
                                     float* alpha, float* log_alpha, double target_entropy,
                                     float* exp_avg, float* exp_avg_sq, int64_t* adam_step,
                                     double lr, double beta1, double beta2, double eps,
                                     float* loss) {
  OCPPO_REQUIRE(B >= 1, "ocppo_csac_alpha_step: bad size B=%lld", (long long)B);
  OCPPO_REQUIRE(log_prob && alpha && log_alpha && exp_avg && exp_avg_sq && adam_step && loss,
                "ocppo_csac_alpha_step: null pointer");
  OCPPO_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0,
                "ocppo_csac_alpha_step: bad Adam hyper-parameters");
  clear_stale_error();
  const CsacAdam ad{exp_avg, exp_avg_sq, adam_step, lr, beta1, beta2, eps};
  hipLaunchKernelGGL(csac_alpha_kernel, dim3(1), dim3(kTd3Threads), 0, as_stream(stream), log_prob,
                     B, alpha, log_alpha, static_cast<float>(target_entropy), ad, loss);
  return check_launch("ocppo_csac_alpha_step");
}
