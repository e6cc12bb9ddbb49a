// Device functions shared by the continuous-action kernels (ocppo_contppo.hip): the wrapper chain
// of cleanrl/ppo_continuous_action.py:96-100 on one env's raw step outputs, and the RPO noise
// stream of cleanrl/rpo_continuous_action.py.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ocppo_philox.h"

namespace ocppo {

// ---- NormalizeObservation / clip / NormalizeReward / clip, one env --------------------------------
// Per-env f64 state [2D + 5] = {obs mean [D], obs var [D], obs count, return accumulator,
// return mean, return var, return count}: every wrapped sub-env of the script's SyncVectorEnv owns
// its statistics. Initial values: mean 0, var 1, count 1e-4, accumulator 0.
__host__ __device__ inline int64_t cont_norm_state_size(int64_t D) { return 2 * D + 5; }

constexpr double kContNormEps = 1e-8;   // the wrappers' epsilon
constexpr double kContNormClip = 10.0;  // TransformObservation / TransformReward clip

// gym's update_mean_var_count_from_moments for a batch of ONE sample (batch_var 0, batch_count 1),
// in its operation order; the caller advances the count.
__device__ __forceinline__ void rms_update_one(double& mean, double& var, double count, double x) {
  const double delta = x - mean;
  const double tot = count + 1.0;
  const double new_mean = mean + delta * 1.0 / tot;
  const double m_a = var * count;
  const double m2 = m_a + 0.0 + delta * delta * count * 1.0 / tot;
  mean = new_mean;
  var = m2 / tot;
}

__device__ __forceinline__ double clip_pm(double v, double c) {
  return v < -c ? -c : (v > c ? c : v);
}

struct ContNorm {
  double* state;   // [N, 2D + 5]; null: no normalisation at all
  int norm_obs;    // NormalizeObservation + clip
  int norm_reward; // NormalizeReward + clip
  double gamma;
};

// One env's step (or reset, has_reward false) through the chain. obs: the D raw values the env
// returned (the reset observation when done); final_obs: the raw terminal observation, read only
// when done: it is normalised first (its output dropped: the script never reads final_observation),
// then the reset observation, so the statistics see two updates on that step.
__device__ __forceinline__ void cont_norm_env(const ContNorm& cn, int64_t n, int64_t D,
                                              const float* obs, const float* final_obs, bool done,
                                              bool terminated, bool has_reward, float reward,
                                              float* obs_out, float* reward_out) {
  double* st = cn.state ? cn.state + n * cont_norm_state_size(D) : nullptr;
  if (st && cn.norm_obs) {
    double count = st[2 * D];
    if (done) {
      for (int64_t d = 0; d < D; ++d)
        rms_update_one(st[d], st[D + d], count, static_cast<double>(final_obs[d]));
      count += 1.0;
    }
    for (int64_t d = 0; d < D; ++d) {
      const double x = static_cast<double>(obs[d]);
      double mean = st[d], var = st[D + d];
      rms_update_one(mean, var, count, x);
      st[d] = mean;
      st[D + d] = var;
      obs_out[d] = static_cast<float>(clip_pm((x - mean) / sqrt(var + kContNormEps), kContNormClip));
    }
    st[2 * D] = count + 1.0;
  } else {
    for (int64_t d = 0; d < D; ++d) obs_out[d] = obs[d];
  }
  if (!has_reward) return;
  if (st && cn.norm_reward) {
    double* rs = st + 2 * D + 1;  // {accumulator, mean, var, count}
    const double r = static_cast<double>(reward);
    const double ret = rs[0] * cn.gamma * (1.0 - (terminated ? 1.0 : 0.0)) + r;
    rs[0] = ret;
    double mean = rs[1], var = rs[2];
    rms_update_one(mean, var, rs[3], ret);
    rs[1] = mean;
    rs[2] = var;
    rs[3] = rs[3] + 1.0;
    reward_out[0] = static_cast<float>(clip_pm(r / sqrt(var + kContNormEps), kContNormClip));
  } else {
    reward_out[0] = reward;
  }
}

// ---- RPO noise -------------------------------------------------------------------------------------
// uniform in [-alpha, alpha) for element (m, a) of minibatch `mb` at update counter `counter`:
// word 0 of the Philox4x32-10 block with key seed ^ kRpoKey and counter (m * 64 + a, counter << 32
// | mb); its top 24 bits give u in [-1, 1 - 2^-23] (exact), times alpha (one rounding).
constexpr uint64_t kRpoKey = 0x3C6EF372FE94F82Bull;

__device__ __forceinline__ float rpo_noise(uint64_t seed, int64_t counter, int64_t mb, int64_t m,
                                           int a, float alpha) {
  const uint64_t sub = (static_cast<uint64_t>(counter) << 32) | (static_cast<uint64_t>(mb) & 0xFFFFFFFFull);
  const uint4 r = philox_block(seed ^ kRpoKey, sub, static_cast<uint64_t>(m) * 64 + static_cast<uint64_t>(a));
  const float u = static_cast<float>(r.x >> 8) * 1.1920928955078125e-07f - 1.0f;  // 2^-23
  return u * alpha;
}

}  // namespace ocppo
