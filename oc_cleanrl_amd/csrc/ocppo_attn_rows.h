// Row helpers of the rows-in-lanes attention walks (ocppo_attn.hip, ocppo_oct_trunk.hip): a lane
// holds one query (or key) row of DH floats in registers and reads the other operand's row from
// memory as float4s (16-byte aligned).
#pragma once

#include "ocppo_common.h"

namespace ocppo {

// sum_d a[d] * row[d]: four interleaved FMA chains, combined (0 + 1) + (2 + 3). Every score and
// every dP of the attention kernels goes through here with the register operand first.
template <int DH>
__device__ __forceinline__ float dot_row(const float (&a)[DH], const float* __restrict__ row) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * c);
    s0 = fmaf(a[4 * c + 0], r.x, s0);
    s1 = fmaf(a[4 * c + 1], r.y, s1);
    s2 = fmaf(a[4 * c + 2], r.z, s2);
    s3 = fmaf(a[4 * c + 3], r.w, s3);
  }
  return (s0 + s1) + (s2 + s3);
}

template <int DH>
__device__ __forceinline__ void axpy_row(float (&acc)[DH], float a, const float* __restrict__ row) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * c);
    acc[4 * c + 0] = fmaf(a, r.x, acc[4 * c + 0]);
    acc[4 * c + 1] = fmaf(a, r.y, acc[4 * c + 1]);
    acc[4 * c + 2] = fmaf(a, r.z, acc[4 * c + 2]);
    acc[4 * c + 3] = fmaf(a, r.w, acc[4 * c + 3]);
  }
}

template <int DH>
__device__ __forceinline__ void load_row(float (&v)[DH], const float* __restrict__ src) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(src + 4 * c);
    v[4 * c + 0] = r.x; v[4 * c + 1] = r.y; v[4 * c + 2] = r.z; v[4 * c + 3] = r.w;
  }
}

template <int DH>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float (&v)[DH], float mul) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c)
    *reinterpret_cast<float4*>(dst + 4 * c) = make_float4(
        v[4 * c + 0] * mul, v[4 * c + 1] * mul, v[4 * c + 2] * mul, v[4 * c + 3] * mul);
}

}  // namespace ocppo
