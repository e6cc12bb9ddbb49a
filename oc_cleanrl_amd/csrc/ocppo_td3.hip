// TD3 and DDPG (cleanrl/td3_continuous_action.py, ddpg_continuous_action.py): a deterministic
// policy over float-vector actions of A <= 64 dimensions. Everything around the three MLPs' GEMMs:
//   cont_replay_add / sample   SB3 ReplayBuffer(optimize_memory_usage=False) in HBM with float
//                              actions; the sample writes the critics' concatenated inputs
//   td3_act                    fc_mu + both acting phases (:205-211), the branch on the device
//   td3_target_actions         the smoothed target action (:239-245) into next_obs_act
//   td3_critic_loss_fwd_bwd    min, TD target, both MSEs and their gradients (:248-255)
//   td3_policy_actions_fwd/bwd tanh * scale + bias into the critic's input, and its backward
//   polyak                     t = tau * p + (1 - tau) * t over several flat buffers (:269-274)
// f32 row arithmetic in torch's op order (the library is built with -ffp-contract=off), batch sums
// in f64 in a fixed order (thread t takes rows t, t + 256, ..., then block_sum), no atomics, int64
// row offsets, plain vector stores. The stream conversions and the critic loss's rows are
// ocppo_contq.h's, shared with ocppo_sac_cont.hip.
//
// Streams (all counter-based, so a captured graph draws fresh numbers on every replay):
//   replay sample   h = splitmix64(splitmix64(seed ^ kContReplayKey) + counter * 0x100000001B3 +
//                   b); row = h % (full ? size : max(pos, 1)), env = splitmix64(h) % E (SB3's
//                   law without the memory-optimised variant's offset, so ocppo_replay_sample's
//                   draw is not shared)
//   acting          Philox4x32-10, key seed ^ kTd3ActKey, counter (e * 64 + a, global step t):
//                   word 0 -> the uniform phase's u in [0, 1), words 0 and 1 -> Box-Muller's z
//   target noise    Philox4x32-10, key seed ^ kTd3TargetKey, counter (b * 64 + a, sample counter)
#include "ocppo_contq.h"
#include "ocppo_rng.h"

namespace ocppo {

constexpr int kPolyakMaxPairs = 4;
constexpr uint64_t kContReplayKey = 0x7D3C0A7B5E91F2A3ull;
constexpr uint64_t kTd3ActKey = 0x7D3AC7E5B1F00D42ull;
constexpr uint64_t kTd3TargetKey = 0x7D37A26E7C11A9B5ull;

__device__ __forceinline__ uint4 act_words(uint64_t seed, int64_t t, int64_t e, int a) {
  return philox_block(seed ^ kTd3ActKey, static_cast<uint64_t>(t),
                      static_cast<uint64_t>(e) * 64 + static_cast<uint64_t>(a));
}

__device__ __forceinline__ float target_z(uint64_t seed, int64_t counter, int64_t b, int a) {
  const uint4 r = philox_block(seed ^ kTd3TargetKey, static_cast<uint64_t>(counter),
                               static_cast<uint64_t>(b) * 64 + static_cast<uint64_t>(a));
  return box_muller(r.x, r.y);
}

// ---- replay ------------------------------------------------------------------------------------------
// One workgroup: every thread reads {pos, full} before the barrier, thread 0 advances them after it.
// carry: obs <- next_obs once stored (the script's `obs = next_obs`, :233).
__global__ __launch_bounds__(kTd3Threads) void cont_replay_add_kernel(
    float* __restrict__ obs, const float* __restrict__ next_obs,
    const float* __restrict__ final_obs, const float* __restrict__ done,
    const float* __restrict__ actions, const float* __restrict__ rewards,
    const float* __restrict__ terminated, int64_t E, int64_t D, int64_t A, int64_t* state,
    int64_t size, float* __restrict__ rb_obs, float* __restrict__ rb_next,
    float* __restrict__ rb_act, float* __restrict__ rb_rew, float* __restrict__ rb_done, int carry) {
  int64_t pos = state[0];
  if (pos < 0 || pos >= size) pos = 0;  // a corrupt state writes inside the buffer
  const int64_t full = state[1];
  for (int64_t g = threadIdx.x; g < E * D; g += kTd3Threads) {
    const int64_t e = g / D;
    const bool fin = final_obs != nullptr && done != nullptr && done[e] != 0.f;
    const float nx = next_obs[g];
    rb_obs[pos * E * D + g] = obs[g];
    rb_next[pos * E * D + g] = fin ? final_obs[g] : nx;
    if (carry) obs[g] = nx;
  }
  for (int64_t g = threadIdx.x; g < E * A; g += kTd3Threads) rb_act[pos * E * A + g] = actions[g];
  for (int64_t g = threadIdx.x; g < E; g += kTd3Threads) {
    rb_rew[pos * E + g] = rewards[g];
    rb_done[pos * E + g] = terminated ? terminated[g] : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t p1 = pos + 1;
    state[0] = p1 == size ? 0 : p1;
    state[1] = (p1 == size || full != 0) ? 1 : 0;
  }
}

__device__ __forceinline__ void cont_sample_index(uint64_t seed, int64_t ctr, int64_t b,
                                                  int64_t pos, int64_t full, int64_t size,
                                                  int64_t E, int64_t& i, int64_t& e) {
  const uint64_t h = splitmix64(splitmix64(seed ^ kContReplayKey) +
                                static_cast<uint64_t>(ctr) * 0x100000001B3ull +
                                static_cast<uint64_t>(b));
  const int64_t upper = full ? size : (pos > 0 ? (pos < size ? pos : size) : 1);
  i = static_cast<int64_t>(h % static_cast<uint64_t>(upper));
  e = static_cast<int64_t>(splitmix64(h) % static_cast<uint64_t>(E));
}

// One thread per element of obs_act [B, D + A]; the row's indices are recomputed per thread.
__global__ __launch_bounds__(kTd3Threads) void cont_replay_sample_kernel(
    uint64_t seed, const int64_t* __restrict__ counter, const int64_t* __restrict__ state,
    int64_t size, int64_t E, int64_t D, int64_t A, const float* __restrict__ rb_obs,
    const float* __restrict__ rb_next, const float* __restrict__ rb_act,
    const float* __restrict__ rb_rew, const float* __restrict__ rb_done, int64_t B,
    float* __restrict__ obs_act, float* __restrict__ next_obs_act, float* __restrict__ rew_out,
    float* __restrict__ done_out, int64_t* __restrict__ idx_out) {
  const int64_t pos = state[0], full = state[1], ctr = counter[0];
  const int64_t W = D + A, total = B * W;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total;
       g += stride) {
    const int64_t b = g / W, c = g - b * W;
    int64_t i, e;
    cont_sample_index(seed, ctr, b, pos, full, size, E, i, e);
    const int64_t row = i * E + e;
    if (c < D) {
      obs_act[g] = rb_obs[row * D + c];
      next_obs_act[g] = rb_next[row * D + c];
    } else {
      obs_act[g] = rb_act[row * A + (c - D)];  // next_obs_act's action columns: td3_target_actions
    }
    if (c == 0) {
      rew_out[b] = rb_rew[row];
      done_out[b] = rb_done[row];
      if (idx_out) {
        idx_out[2 * b] = i;
        idx_out[2 * b + 1] = e;
      }
    }
  }
}

__global__ void td3_counter_add_kernel(int64_t* counter, int64_t n) { counter[0] += n; }

// ---- acting ------------------------------------------------------------------------------------------
// One wave per env. mu[a] = sum_j h[e, j] w[a, j] + b[a] with lane l adding j = l, l + 64, ... in
// order and the lanes combined by wave_sum's butterfly (td3.act_mu restates that order in torch).
__global__ __launch_bounds__(kWave) void td3_act_kernel(
    const float* __restrict__ hidden, int64_t E, int64_t H, const float* __restrict__ w,
    const float* __restrict__ bias_mu, int A, const float* __restrict__ scale,
    const float* __restrict__ abias, const float* __restrict__ low, const float* __restrict__ high,
    uint64_t seed, const int64_t* __restrict__ step, int64_t step_offset, int64_t learning_starts,
    float noise, float* __restrict__ actions) {
  const int64_t t = step[0] + step_offset;
  const bool random = t < learning_starts;
  const int lane = threadIdx.x;
  for (int64_t e = blockIdx.x; e < E; e += gridDim.x) {
    float mu = 0.f;
    if (!random) {
      for (int a = 0; a < A; ++a) {
        float acc = 0.f;
        for (int64_t j = lane; j < H; j += kWave) acc += hidden[e * H + j] * w[a * H + j];
        acc = wave_sum(acc);
        if (lane == a) mu = acc + bias_mu[a];
      }
    }
    if (lane >= A) continue;
    const uint4 r = act_words(seed, t, e, lane);
    const float lo = low[lane], hi = high[lane];
    float v;
    if (random) {
      v = lo + (hi - lo) * unit24(r.x);
      if (v >= hi) v = nextafterf(hi, lo);  // the last product may round up to the bound
    } else {
      const float act = tanhf(mu) * scale[lane] + abias[lane];
      v = clamp_f(act + (scale[lane] * noise) * box_muller(r.x, r.y), lo, hi);
    }
    actions[e * A + lane] = v;
  }
}

// mode 0: the acting stream's z [E, A]; 1: its uniform u; 2: the target stream's z [B, A]
__global__ __launch_bounds__(kTd3Threads) void td3_draws_kernel(
    uint64_t seed, const int64_t* __restrict__ counter, int64_t offset, int64_t R, int A, int mode,
    float* __restrict__ out) {
  const int64_t c = counter[0] + offset;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < R * A;
       g += stride) {
    const int64_t r = g / A;
    const int a = static_cast<int>(g - r * A);
    if (mode == 2) {
      out[g] = target_z(seed, c, r, a);
    } else {
      const uint4 x = act_words(seed, c, r, a);
      out[g] = mode == 1 ? unit24(x.x) : box_muller(x.x, x.y);
    }
  }
}

// ---- the smoothed target action (:239-245) --------------------------------------------------------
__global__ __launch_bounds__(kTd3Threads) void td3_target_actions_kernel(
    const float* __restrict__ mu, int64_t B, int64_t D, int A, const float* __restrict__ scale,
    const float* __restrict__ abias, uint64_t seed, const int64_t* __restrict__ counter,
    float policy_noise, float noise_clip, float low0, float high0,
    float* __restrict__ next_obs_act) {
  const bool noisy = policy_noise != 0.f;
  const int64_t ctr = noisy ? counter[0] : 0;
  const int64_t W = D + A;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < B * A;
       g += stride) {
    const int64_t b = g / A;
    const int a = static_cast<int>(g - b * A);
    float v = tanhf(mu[g]) * scale[a] + abias[a];
    if (noisy) {
      const float n = clamp_f(target_z(seed, ctr, b, a) * policy_noise, -noise_clip, noise_clip);
      v = clamp_f(v + n * scale[a], low0, high0);
    }
    next_obs_act[b * W + D + a] = v;
  }
}

// ---- critic: TD target + MSE(s) (:248-255) ----------------------------------------------------------
//   y_b = r_b + ((1 - d_b) * gamma) * min(q1t_b, q2t_b);  qf_loss = mean (q - y)^2
//   dq = (2 / B) (q - y), mse_loss's backward. q2 / q2t / dq2 null: DDPG's single critic.
__global__ __launch_bounds__(kTd3Threads) void td3_critic_kernel(
    const float* __restrict__ q1t, const float* __restrict__ q2t, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ rewards,
    const float* __restrict__ dones, int64_t B, float gamma, float norm, float* __restrict__ dq1,
    float* __restrict__ dq2, float* __restrict__ stats, float* __restrict__ y_out) {
  __shared__ double scratch[kTd3Threads / kWave];
  critic_loss_rows<false>(q1t, q2t, q1, q2, rewards, dones, nullptr, 0.f, B, gamma, norm, dq1, dq2,
                          stats, y_out, scratch);
}

// ---- the actor loss's action (:263) -------------------------------------------------------------------
__global__ __launch_bounds__(kTd3Threads) void td3_policy_fwd_kernel(
    const float* __restrict__ mu, const float* __restrict__ obs_act, int64_t B, int64_t D, int A,
    const float* __restrict__ scale, const float* __restrict__ abias, float* __restrict__ xa,
    float* __restrict__ tanh_out) {
  const int64_t W = D + A;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < B * W;
       g += stride) {
    const int64_t b = g / W, c = g - b * W;
    if (c < D) {
      xa[g] = obs_act[g];
    } else {
      const int a = static_cast<int>(c - D);
      const float t = tanhf(mu[b * A + a]);
      tanh_out[b * A + a] = t;
      xa[g] = t * scale[a] + abias[a];
    }
  }
}

// d mu = (dxa * scale) * (1 - tanh^2): autograd's mul backward, then tanh_backward, whose
// 1 - t * t ATen's device kernel contracts into one fma (written out here: this library is built
// without contraction)
__global__ __launch_bounds__(kTd3Threads) void td3_policy_bwd_kernel(
    const float* __restrict__ dxa, const float* __restrict__ tanh_in, int64_t B, int64_t D, int A,
    const float* __restrict__ scale, float* __restrict__ dmu) {
  const int64_t W = D + A;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < B * A;
       g += stride) {
    const int64_t b = g / A;
    const int a = static_cast<int>(g - b * A);
    const float t = tanh_in[g];
    dmu[g] = (dxa[b * W + D + a] * scale[a]) * fmaf(-t, t, 1.0f);
  }
}

// ---- soft target update (:269-274) ------------------------------------------------------------------
struct PolyakArgs {
  const float* p[kPolyakMaxPairs];
  float* t[kPolyakMaxPairs];
  int64_t end[kPolyakMaxPairs];  // running totals of the pairs' lengths
  int n;
};

__global__ __launch_bounds__(kTd3Threads) void polyak_kernel(PolyakArgs P, float tau, float keep) {
  const int64_t total = P.end[P.n - 1];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total;
       g += stride) {
    int k = 0;
#pragma unroll
    for (int q = 0; q < kPolyakMaxPairs - 1; ++q)
      if (q < P.n - 1 && g >= P.end[q]) k = q + 1;
    const float* src = P.p[0];
    float* dst = P.t[0];
    int64_t base = 0;
#pragma unroll
    for (int q = 1; q < kPolyakMaxPairs; ++q)
      if (k == q) {
        src = P.p[q];
        dst = P.t[q];
        base = P.end[q - 1];
      }
    const int64_t i = g - base;
    const float a = tau * src[i];
    const float b = keep * dst[i];
    dst[i] = a + b;
  }
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_cont_replay_add(ocppo_stream_t stream, float* obs, const float* next_obs,
                                     const float* final_obs, const float* done,
                                     const float* actions, const float* rewards,
                                     const float* terminated, int64_t E, int64_t D, int64_t A,
                                     int64_t* state, int64_t size, float* rb_obs,
                                     float* rb_next_obs, float* rb_actions, float* rb_rewards,
                                     float* rb_dones, int carry) {
  if (int rc = td3_sizes("ocppo_cont_replay_add", E, D, A)) return rc;
  OCPPO_REQUIRE(E >= 1 && size >= 1, "ocppo_cont_replay_add: bad sizes E=%lld size=%lld",
                (long long)E, (long long)size);
  OCPPO_REQUIRE(obs && next_obs && actions && rewards && state && rb_obs && rb_next_obs &&
                    rb_actions && rb_rewards && rb_dones,
                "ocppo_cont_replay_add: null pointer");
  OCPPO_REQUIRE((final_obs == nullptr) == (done == nullptr),
                "ocppo_cont_replay_add: final_obs and done come together");
  OCPPO_REQUIRE(obs != next_obs, "ocppo_cont_replay_add: obs and next_obs must not alias");
  clear_stale_error();
  hipLaunchKernelGGL(cont_replay_add_kernel, dim3(1), dim3(kTd3Threads), 0, as_stream(stream), obs,
                     next_obs, final_obs, done, actions, rewards, terminated, E, D, A, state, size,
                     rb_obs, rb_next_obs, rb_actions, rb_rewards, rb_dones, carry ? 1 : 0);
  return check_launch("ocppo_cont_replay_add");
}

extern "C" int ocppo_cont_replay_sample(ocppo_stream_t stream, uint64_t seed, int64_t* counter,
                                        const int64_t* state, int64_t size, int64_t E, int64_t D,
                                        int64_t A, const float* rb_obs, const float* rb_next_obs,
                                        const float* rb_actions, const float* rb_rewards,
                                        const float* rb_dones, int64_t B, float* obs_act,
                                        float* next_obs_act, float* rewards_out, float* dones_out,
                                        int64_t* indices_out) {
  if (int rc = td3_sizes("ocppo_cont_replay_sample", B, D, A)) return rc;
  OCPPO_REQUIRE(E >= 1 && size >= 1 && B >= 1, "ocppo_cont_replay_sample: bad sizes");
  OCPPO_REQUIRE(counter && state && rb_obs && rb_next_obs && rb_actions && rb_rewards &&
                    rb_dones && obs_act && next_obs_act && rewards_out && dones_out,
                "ocppo_cont_replay_sample: null pointer");
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(cont_replay_sample_kernel, dim3(grid_for(B * (D + A), kTd3Threads)),
                     dim3(kTd3Threads), 0, s, seed, counter, state, size, E, D, A, rb_obs,
                     rb_next_obs, rb_actions, rb_rewards, rb_dones, B, obs_act, next_obs_act,
                     rewards_out, dones_out, indices_out);
  if (int rc = check_launch("ocppo_cont_replay_sample")) return rc;
  hipLaunchKernelGGL(td3_counter_add_kernel, dim3(1), dim3(1), 0, s, counter, int64_t(1));
  return check_launch("ocppo_cont_replay_sample/counter");
}

extern "C" int ocppo_td3_act(ocppo_stream_t stream, const float* hidden, int64_t E, int64_t H,
                             const float* w_mu, const float* b_mu, int64_t A,
                             const float* action_scale, const float* action_bias,
                             const float* low, const float* high, uint64_t seed,
                             const int64_t* step, int64_t step_offset, int64_t learning_starts,
                             double exploration_noise, float* actions) {
  if (int rc = td3_sizes("ocppo_td3_act", E, H, A)) return rc;
  if (E == 0) return OCPPO_OK;
  OCPPO_REQUIRE(hidden && w_mu && b_mu && action_scale && action_bias && low && high && step &&
                    actions,
                "ocppo_td3_act: null pointer");
  clear_stale_error();
  const int64_t g = E < 4096 ? E : 4096;
  hipLaunchKernelGGL(td3_act_kernel, dim3(g), dim3(kWave), 0, as_stream(stream), hidden, E, H,
                     w_mu, b_mu, (int)A, action_scale, action_bias, low, high, seed, step,
                     step_offset, learning_starts, static_cast<float>(exploration_noise), actions);
  return check_launch("ocppo_td3_act");
}

extern "C" int ocppo_td3_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                               int64_t offset, int64_t rows, int64_t A, int mode, float* out) {
  if (int rc = td3_sizes("ocppo_td3_noise", rows, 1, A)) return rc;
  OCPPO_REQUIRE(mode >= 0 && mode <= 2, "ocppo_td3_noise: mode %d (0 acting z, 1 acting u, 2 "
                "target z)", mode);
  if (rows == 0) return OCPPO_OK;
  OCPPO_REQUIRE(counter && out, "ocppo_td3_noise: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(td3_draws_kernel, dim3(grid_for(rows * A, kTd3Threads)), dim3(kTd3Threads), 0,
                     as_stream(stream), seed, counter, offset, rows, (int)A, mode, out);
  return check_launch("ocppo_td3_noise");
}

extern "C" int ocppo_td3_target_actions(ocppo_stream_t stream, const float* mu, int64_t B,
                                        int64_t D, int64_t A, const float* action_scale,
                                        const float* action_bias, uint64_t seed,
                                        const int64_t* counter, double policy_noise,
                                        double noise_clip, double low0, double high0,
                                        float* next_obs_act) {
  if (int rc = td3_sizes("ocppo_td3_target_actions", B, D, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(mu && action_scale && action_bias && next_obs_act,
                "ocppo_td3_target_actions: null pointer");
  OCPPO_REQUIRE(policy_noise == 0.0 || counter,
                "ocppo_td3_target_actions: policy_noise != 0 needs the device counter");
  OCPPO_REQUIRE(noise_clip >= 0.0 && low0 <= high0, "ocppo_td3_target_actions: bad bounds");
  clear_stale_error();
  hipLaunchKernelGGL(td3_target_actions_kernel, dim3(grid_for(B * A, kTd3Threads)),
                     dim3(kTd3Threads), 0, as_stream(stream), mu, B, D, (int)A, action_scale,
                     action_bias, seed, counter, static_cast<float>(policy_noise),
                     static_cast<float>(noise_clip), static_cast<float>(low0),
                     static_cast<float>(high0), next_obs_act);
  return check_launch("ocppo_td3_target_actions");
}

extern "C" int ocppo_td3_critic_loss_fwd_bwd(ocppo_stream_t stream, const float* q1_next_target,
                                             const float* q2_next_target, const float* q1,
                                             const float* q2, const float* rewards,
                                             const float* dones, int64_t B, double gamma,
                                             float* dq1, float* dq2, float* stats, float* y_out) {
  OCPPO_REQUIRE(B >= 0, "ocppo_td3_critic_loss_fwd_bwd: bad size B=%lld", (long long)B);
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(q1_next_target && q1 && rewards && dones && dq1 && stats,
                "ocppo_td3_critic_loss_fwd_bwd: null pointer");
  OCPPO_REQUIRE((q2 == nullptr) == (q2_next_target == nullptr) && (q2 == nullptr) == (dq2 == nullptr),
                "ocppo_td3_critic_loss_fwd_bwd: q2, its target and dq2 come together");
  clear_stale_error();
  // mse_loss backward: norm = 2 / numel (computed in double by ATen, applied in f32)
  const float norm = static_cast<float>(2.0 / static_cast<double>(B));
  hipLaunchKernelGGL(td3_critic_kernel, dim3(1), dim3(kTd3Threads), 0, as_stream(stream),
                     q1_next_target, q2_next_target, q1, q2, rewards, dones, B,
                     static_cast<float>(gamma), norm, dq1, dq2, stats, y_out);
  return check_launch("ocppo_td3_critic_loss_fwd_bwd");
}

extern "C" int ocppo_td3_policy_actions_fwd(ocppo_stream_t stream, const float* mu,
                                            const float* obs_act, int64_t B, int64_t D, int64_t A,
                                            const float* action_scale, const float* action_bias,
                                            float* xa, float* tanh_out) {
  if (int rc = td3_sizes("ocppo_td3_policy_actions_fwd", B, D, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(mu && obs_act && action_scale && action_bias && xa && tanh_out,
                "ocppo_td3_policy_actions_fwd: null pointer");
  OCPPO_REQUIRE(xa != obs_act, "ocppo_td3_policy_actions_fwd: xa is a copy, not obs_act itself");
  clear_stale_error();
  hipLaunchKernelGGL(td3_policy_fwd_kernel, dim3(grid_for(B * (D + A), kTd3Threads)),
                     dim3(kTd3Threads), 0, as_stream(stream), mu, obs_act, B, D, (int)A,
                     action_scale, action_bias, xa, tanh_out);
  return check_launch("ocppo_td3_policy_actions_fwd");
}

extern "C" int ocppo_td3_policy_actions_bwd(ocppo_stream_t stream, const float* dxa,
                                            const float* tanh_in, int64_t B, int64_t D, int64_t A,
                                            const float* action_scale, float* dmu) {
  if (int rc = td3_sizes("ocppo_td3_policy_actions_bwd", B, D, A)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dxa && tanh_in && action_scale && dmu,
                "ocppo_td3_policy_actions_bwd: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(td3_policy_bwd_kernel, dim3(grid_for(B * A, kTd3Threads)), dim3(kTd3Threads),
                     0, as_stream(stream), dxa, tanh_in, B, D, (int)A, action_scale, dmu);
  return check_launch("ocppo_td3_policy_actions_bwd");
}

extern "C" int ocppo_polyak(ocppo_stream_t stream, int n_pairs, const float* const* params,
                            float* const* targets, const int64_t* numels, double tau) {
  OCPPO_REQUIRE(n_pairs >= 1 && n_pairs <= kPolyakMaxPairs && params && targets && numels,
                "ocppo_polyak: 1..%d (parameter, target) pairs", kPolyakMaxPairs);
  PolyakArgs P{};
  int64_t total = 0;
  for (int k = 0; k < n_pairs; ++k) {
    OCPPO_REQUIRE(numels[k] >= 0 && (numels[k] == 0 || (params[k] && targets[k])),
                  "ocppo_polyak: pair %d: null pointer or negative length", k);
    OCPPO_REQUIRE(params[k] != targets[k] || numels[k] == 0,
                  "ocppo_polyak: pair %d: the target is the parameter buffer itself", k);
    total += numels[k];
    P.p[k] = params[k];
    P.t[k] = targets[k];
    P.end[k] = total;
  }
  P.n = n_pairs;
  if (total == 0) return OCPPO_OK;
  clear_stale_error();
  hipLaunchKernelGGL(polyak_kernel, dim3(grid_for(total, kTd3Threads)), dim3(kTd3Threads), 0,
                     as_stream(stream), P, static_cast<float>(tau), static_cast<float>(1.0 - tau));
  return check_launch("ocppo_polyak");
}
