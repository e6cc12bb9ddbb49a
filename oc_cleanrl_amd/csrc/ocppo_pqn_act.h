// PQN's acting step for one environment as a device function: ocppo_pqn_act's kernel body
// (ocppo_pqn.hip) and the second half of ocppo_pqn_lstm_act's (ocppo_pqn_lstm.hip) are this one
// piece of code, so both write the same bits.
//
// One wave per environment: the A <= 18 dot products of the hidden row, each lane over the float4
// chunks lane, lane + 64, ... of the row and the butterfly over the lanes (every lane ends with
// every Q value), then the first maximum (torch.argmax's choice on the CPU; a NaN counts as the
// maximum, as there) and EpsGreedy's coin and random action (ocppo_rng.h: ocppo_epsilon_greedy's).
#pragma once
#include "ocppo_common.h"
#include "ocppo_rng.h"

namespace ocppo {

constexpr int kPqnMaxA = 18;
constexpr int kPqnMaxH = 1024;

// All 64 lanes of a wave call it for environment n. hrow: the environment's H hidden values,
// 16-B aligned, in global memory or LDS. actions, eps_out and q_out may be null.
__device__ __forceinline__ void pqn_act_row(const float* hrow, int64_t n, int H,
                                            const float* __restrict__ wq,
                                            const float* __restrict__ bq, int A,
                                            const EpsGreedy& eg, int lane,
                                            int64_t* __restrict__ actions,
                                            float* __restrict__ values,
                                            float* __restrict__ eps_out,
                                            float* __restrict__ q_out) {
  constexpr int kCh = kPqnMaxH / 4 / kWave;  // float4 chunks per lane
  const int H4 = H / 4;
  float4 x[kCh];
#pragma unroll
  for (int c = 0; c < kCh; ++c) {
    const int i = lane + c * kWave;
    x[c] = i < H4 ? reinterpret_cast<const float4*>(hrow)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  int best = 0;
  float bqv = 0.f;
  for (int j = 0; j < A; ++j) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < kCh; ++c) {
      const int i = lane + c * kWave;
      if (i < H4) {
        const float4 w = reinterpret_cast<const float4*>(wq + static_cast<int64_t>(j) * H)[i];
        acc += x[c].x * w.x + x[c].y * w.y + x[c].z * w.z + x[c].w * w.w;
      }
    }
    const float q = wave_sum(acc) + bq[j];
    if (j == 0 || q > bqv || (q != q && bqv == bqv)) {
      bqv = q;
      best = j;
    }
    if (q_out && lane == 0) q_out[n * A + j] = q;
  }
  if (lane == 0) {
    values[n] = bqv;
    if (actions) actions[n] = eg.explore ? eg.random_action(n, A) : static_cast<int64_t>(best);
    if (eps_out && n == 0) eps_out[0] = static_cast<float>(eg.eps);
  }
}

}  // namespace ocppo
