// Device code shared by the off-policy continuous-action learners (ocppo_td3.hip: TD3 / DDPG,
// ocppo_sac_cont.hip: continuous SAC): the counter streams' conversions and the twin-critic loss.
#pragma once

#include "ocppo_common.h"
#include "ocppo_philox.h"

namespace ocppo {

constexpr int kTd3MaxA = 64;  // ops.GAUSS_MAX_ACTIONS
constexpr int kTd3Threads = 256;
constexpr float kInv24 = 5.9604644775390625e-08f;  // 2^-24

// top 24 bits of a Philox word as a uniform in [0, 1)
__device__ __forceinline__ float unit24(uint32_t w) { return static_cast<float>(w >> 8) * kInv24; }

// Box-Muller in f32: u1 in (0, 1] (so the logarithm is finite), u2 in [0, 1)
__device__ __forceinline__ float box_muller(uint32_t w0, uint32_t w1) {
  const float u1 = (static_cast<float>(w0 >> 8) + 1.0f) * kInv24;
  const float u2 = unit24(w1);
  const float r = sqrtf(-2.0f * logf(u1));
  return r * cosf(6.2831855f * u2);
}

// torch.clamp's value for a non-NaN input (a NaN stays a NaN)
__device__ __forceinline__ float clamp_f(float v, float lo, float hi) {
  return v != v ? v : fminf(fmaxf(v, lo), hi);
}

// ---- critic: TD target + MSE(s) ----------------------------------------------------------------------
//   y_b = r_b + ((1 - d_b) * gamma) * m_b;  qf_loss = mean (q - y)^2;  dq = (2 / B) (q - y), mse_loss's
//   backward. m_b = min(q1t_b, q2t_b) (q2 / q2t / dq2 null: q1t_b, DDPG's single critic); kEntropy
//   (continuous SAC, always twin): m_b = min(q1t_b, q2t_b) - alpha * logp_b. One workgroup of
//   kTd3Threads; thread t takes rows t, t + 256, ..., the four sums are f64 through block_sum.
template <bool kEntropy>
__device__ __forceinline__ void critic_loss_rows(
    const float* __restrict__ q1t, const float* __restrict__ q2t, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ rewards,
    const float* __restrict__ dones, const float* __restrict__ logp, float alpha, int64_t B,
    float gamma, float norm, float* __restrict__ dq1, float* __restrict__ dq2,
    float* __restrict__ stats, float* __restrict__ y_out, double* scratch) {
  const bool twin = q2 != nullptr;
  double se1 = 0.0, se2 = 0.0, sq1 = 0.0, sq2 = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += kTd3Threads) {
    float m = twin ? fminf(q1t[b], q2t[b]) : q1t[b];
    if (kEntropy) m = m - alpha * logp[b];
    const float y = rewards[b] + ((1.0f - dones[b]) * gamma) * m;
    if (y_out) y_out[b] = y;
    const float o1 = q1[b], d1 = o1 - y;
    se1 += static_cast<double>(d1 * d1);
    sq1 += o1;
    dq1[b] = norm * d1;
    if (twin) {
      const float o2 = q2[b], d2 = o2 - y;
      se2 += static_cast<double>(d2 * d2);
      sq2 += o2;
      dq2[b] = norm * d2;
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

static int td3_sizes(const char* who, int64_t B, int64_t D, int64_t A) {
  OCPPO_REQUIRE(B >= 0 && D >= 1 && A >= 1 && A <= kTd3MaxA,
                "%s: bad sizes B=%lld D=%lld A=%lld (D >= 1, 1 <= A <= %d)", who, (long long)B,
                (long long)D, (long long)A, kTd3MaxA);
  return OCPPO_OK;
}

}  // namespace ocppo
