// The TD target + MSE row code of dqn_atari_oc.py:378-382, shared by td_loss_kernel
// (ocppo_dqn.hip) and qdagger_loss_kernel (ocppo_qdagger.hip): one thread owns a row, the batch
// sums run in block_sum's fixed order, so both kernels produce the same bits from the same rows.
#pragma once

#include "ocppo_common.h"

namespace ocppo {

// Row b: target_max = max_a q_next;  td = r + (gamma * target_max) * (1 - d);  old = q[b, a_b].
// Adds (td - old)^2 to `se` and old to `sq`, returns d loss / d q[b, a_b] = (old - td) * norm
// (mse_loss_backward w.r.t. its `target` argument, norm = f32(2 / B)) and the row's action in `a`.
__device__ __forceinline__ float td_row(const float* __restrict__ q,
                                        const float* __restrict__ q_next,
                                        const int64_t* __restrict__ actions,
                                        const float* __restrict__ rewards,
                                        const float* __restrict__ dones, int64_t b, int A,
                                        float gamma, float norm, int64_t& a, float& se,
                                        float& sq) {
  float m = q_next[b * A];
  for (int j = 1; j < A; ++j) m = fmaxf(m, q_next[b * A + j]);
  const float td = rewards[b] + (gamma * m) * (1.0f - dones[b]);
  a = actions[b];
  const float old = q[b * A + a];
  const float diff = td - old;
  se += diff * diff;
  sq += old;
  return (old - td) * norm;
}

// The per-thread sums of td_row over the workgroup: {mean (td - old)^2, mean old}, valid in every
// thread. `scratch` holds blockDim.x / 64 floats.
__device__ __forceinline__ void td_reduce(float se, float sq, int64_t B, float* scratch,
                                          float& td_loss, float& q_mean) {
  se = block_sum(se, scratch);
  sq = block_sum(sq, scratch);
  td_loss = se / static_cast<float>(B);  // losses/td_loss
  q_mean = sq / static_cast<float>(B);   // losses/q_values (old_val.mean())
}

// mse_loss backward's norm = 2 / numel (computed in double by ATen, applied in f32)
inline float td_norm(int64_t B) { return static_cast<float>(2.0 / static_cast<double>(B)); }

}  // namespace ocppo
