// Wave routines shared by the distributional learners (ocppo_c51.hip, ocppo_rainbow.hip): one wave
// owns one softmax over N <= 128 atoms, lane k holds atoms k and k + 64, and the max / sum /
// expected value are wave butterflies with a fixed order, so every result is bitwise repeatable.
#pragma once

#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kC51MaxAtoms = 128;
constexpr int kC51MaxActions = 18;
constexpr int kC51LossWaves = 16;  // the loss kernels' single workgroup: 1024 threads
constexpr int kC51Batch = 6;       // softmaxes a wave reduces side by side (independent chains)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// softmax over the N atoms of G rows held in registers (x0 / x1: this lane's atoms `lane` and
// `lane + 64`, -inf past N) and each row's expected value q = sum_k p_k * z_k (torch.softmax(dim=2);
// (pmfs * atoms).sum(2)). Called by a whole wave; p0 / p1 are 0 past N, q is the same in every
// lane. The G chains are independent, so their butterflies overlap.
template <int G>
__device__ __forceinline__ void softmax_q_regs(float (&x0)[G], float (&x1)[G], bool h0, bool h1,
                                               float z0, float z1, float (&p0)[G], float (&p1)[G],
                                               float (&q)[G]) {
  float m[G], s[G];
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = wave_max(fmaxf(x0[g], x1[g]));
#pragma unroll
  for (int g = 0; g < G; ++g) {
    x0[g] = h0 ? expf(x0[g] - m[g]) : 0.f;
    x1[g] = h1 ? expf(x1[g] - m[g]) : 0.f;
    s[g] = x0[g] + x1[g];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) s[g] = wave_sum(s[g]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    p0[g] = x0[g] / s[g];
    p1[g] = x1[g] / s[g];
    q[g] = p0[g] * z0 + p1[g] * z1;
  }
#pragma unroll
  for (int g = 0; g < G; ++g) q[g] = wave_sum(q[g]);
}

// softmax_q_regs over up to G consecutive [N] rows starting at `rows` (`valid` of them exist; the
// others repeat the last one and are ignored by the caller).
template <int G>
__device__ __forceinline__ void c51_softmax_q(const float* __restrict__ rows, int valid, int N,
                                              int lane, float z0, float z1, float (&p0)[G],
                                              float (&p1)[G], float (&q)[G]) {
  const bool h0 = lane < N, h1 = lane + kWave < N;
  float x0[G], x1[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* row = rows + static_cast<int64_t>(g < valid ? g : valid - 1) * N;
    x0[g] = h0 ? row[lane] : -INFINITY;
    x1[g] = h1 ? row[lane + kWave] : -INFINITY;
  }
  softmax_q_regs<G>(x0, x1, h0, h1, z0, z1, p0, p1, q);
}

// torch.argmax's update rule on a running best (first maximum; a NaN beats every number)
__device__ __forceinline__ bool c51_better(float v, float best) {
  return v > best || (v != v && best == best);
}

}  // namespace ocppo
