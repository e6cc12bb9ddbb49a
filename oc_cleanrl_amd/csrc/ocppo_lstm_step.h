// The rollout's single LSTM step as a device function: ocppo_lstm_step's kernel body
// (ocppo_lstm.hip) and the first half of ocppo_pqn_lstm_act's (ocppo_pqn_lstm.hip) are this one
// piece of code, so both write the same bits.
//
// Both products are done here, so weights stream: a workgroup of 4H threads owns kStepEnvs
// environments, stages their x rows (then their masked h rows) in LDS in chunks of kStepChunk
// columns, and 16-lane groups walk one weight row each with coalesced 64-byte reads; a row's
// partials are combined by a fixed xor butterfly (8, 4, 2, 1). A row's arithmetic does not depend
// on N or on the other rows of its workgroup (rows past N are zeros that nothing reads back).
#pragma once
#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kStepEnvs = 4;
constexpr int kStepChunk = 512;
constexpr int kStepPasses = 16;  // weight rows per 16-lane group: 4H threads = H / 4 groups

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// acc[p][r] += sum_k tile[r][k] * wrow_p[k] for this thread's 16-lane group: rows p * GROUPS + grp
template <int GROUPS>
__device__ __forceinline__ void step_accumulate(float (&acc)[kStepPasses][kStepEnvs],
                                                const float (*tile)[kStepChunk],
                                                const float* __restrict__ wmat, int64_t ld,
                                                int64_t k0, int kc, int grp, int gl) {
  // k outside, the group's 16 rows inside: 16 independent weight loads in flight per k
  const float* __restrict__ wr = wmat + static_cast<int64_t>(grp) * ld + k0;
  const int64_t pstride = static_cast<int64_t>(GROUPS) * ld;
#pragma unroll 2
  for (int k = gl; k < kc; k += 16) {
    float xv[kStepEnvs], wv[kStepPasses];
#pragma unroll
    for (int p = 0; p < kStepPasses; ++p) wv[p] = wr[p * pstride + k];
#pragma unroll
    for (int r = 0; r < kStepEnvs; ++r) xv[r] = tile[r][k];
#pragma unroll
    for (int p = 0; p < kStepPasses; ++p)
#pragma unroll
      for (int r = 0; r < kStepEnvs; ++r) acc[p][r] = fmaf(xv[r], wv[p], acc[p][r]);
  }
}

// One step for the workgroup's kStepEnvs environments n0 .. n0 + kStepEnvs - 1 (4H threads, all
// of them call it). commit: c / h are updated in place. STASH: the new h rows are also left in
// s_x[r][0 .. H) (valid after the caller's next __syncthreads()). s_x must be 16-B aligned when
// the caller reads it back as float4.
template <int H, bool STASH>
__device__ __forceinline__ void lstm_step_rows(
    const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ done, int64_t N, int64_t I, float* h, float* c, bool commit,
    int64_t n0, float (*s_x)[kStepChunk], float (*s_g)[4 * H]) {
  constexpr int NT = 4 * H, GROUPS = NT / 16, PASSES = kStepPasses, R = kStepEnvs;
  static_assert(GROUPS * PASSES == 4 * H, "every weight row has one group and pass");
  const int tid = threadIdx.x, grp = tid / 16, gl = tid % 16;
  float acc[PASSES][R];
#pragma unroll
  for (int p = 0; p < PASSES; ++p)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[p][r] = 0.f;
  for (int64_t k0 = 0; k0 < I; k0 += kStepChunk) {
    const int kc = static_cast<int>(I - k0 < kStepChunk ? I - k0 : kStepChunk);
    __syncthreads();  // the previous chunk's readers are done with the tile
    for (int idx = tid; idx < R * kc; idx += NT) {
      const int r = idx / kc, k = idx % kc;
      s_x[r][k] = n0 + r < N ? x[(n0 + r) * I + k0 + k] : 0.f;
    }
    __syncthreads();
    step_accumulate<GROUPS>(acc, s_x, w_ih, I, k0, kc, grp, gl);
  }
  __syncthreads();
  for (int idx = tid; idx < R * H; idx += NT) {  // the masked state (H <= kStepChunk)
    const int r = idx / H, k = idx % H;
    s_x[r][k] = n0 + r < N ? (1.f - done[n0 + r]) * h[(n0 + r) * H + k] : 0.f;
  }
  __syncthreads();
  step_accumulate<GROUPS>(acc, s_x, w_hh, H, 0, H, grp, gl);
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int j = p * GROUPS + grp;
    const float bias = b_ih[j] + b_hh[j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v = acc[p][r];
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 16);
      if (gl == 0) {
        const float z = v + bias;
        s_g[r][j] = (j / H == 2) ? tanhf(z) : sigmoid_f(z);
      }
    }
  }
  __syncthreads();  // also: every read of h (and of the s_x tile) above is done before the writes
  for (int idx = tid; idx < R * H; idx += NT) {
    const int r = idx / H, u = idx % H;
    const int64_t n = n0 + r;
    if (n < N) {
      const float c_in = (1.f - done[n]) * c[n * H + u];
      const float cn = s_g[r][H + u] * c_in + s_g[r][u] * s_g[r][2 * H + u];
      const float hn = s_g[r][3 * H + u] * tanhf(cn);
      if (commit) {
        c[n * H + u] = cn;
        h[n * H + u] = hn;
      }
      if (STASH) s_x[r][u] = hn;
    }
  }
}

inline int lstm_check(const char* who, int64_t T, int64_t B, int64_t H) {
  OCPPO_REQUIRE(T >= 0 && B >= 0, "%s: negative size T=%lld B=%lld", who, (long long)T,
                (long long)B);
  OCPPO_REQUIRE(H == 32 || H == 64 || H == 128, "%s: hidden size %lld not in {32, 64, 128}", who,
                (long long)H);
  OCPPO_REQUIRE(B <= INT32_MAX, "%s: B = %lld exceeds the grid", who, (long long)B);
  return OCPPO_OK;
}

#define OCPPO_LSTM_DISPATCH(HV, CALL)                  \
  switch (HV) {                                        \
    case 32: { constexpr int HH = 32; CALL; break; }   \
    case 64: { constexpr int HH = 64; CALL; break; }   \
    default: { constexpr int HH = 128; CALL; break; }  \
  }

}  // namespace ocppo
