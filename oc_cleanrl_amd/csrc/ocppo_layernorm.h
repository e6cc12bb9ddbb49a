// LayerNorm over the last dimension of [R, E] rows with its backward, once, for the two entries
// that use it: ocppo_add_layernorm_* (ocppo_attn.hip: LayerNorm(x + res), the post-norm step of an
// encoder block) and ocppo_ln_relu_* (ocppo_pqn.hip: relu(LayerNorm(x)) after a Linear layer).
//
// One wave per row; lane l holds columns l, l + 64, ... (PL per lane, E <= 64 PL). The backward
// writes dx per row and keeps dgamma / dbeta in registers over the rows of its wave; the waves of
// a workgroup are combined through LDS in wave order into part[workgroup][2][E], and a finish
// launch sums the partials in workgroup order. No atomics: every sum runs in an order fixed by
// the shapes alone.
#pragma once
#include "ocppo_common.h"

namespace ocppo {

constexpr int kLnWaves = 4;       // rows in flight per workgroup
constexpr int kLnMaxParts = 128;  // workgroups of the backward = dgamma / dbeta partials

// The three places where the two LayerNorms differ
struct LnAddResidual {
  static constexpr bool kRes = true;        // the row is x + res
  static constexpr bool kRecentre = false;  // centred in one step: d = z - sum(z) / E
  static constexpr bool kRelu = false;
};
struct LnRelu {
  static constexpr bool kRes = false;
  // Centred in two steps so that a large common offset costs nothing: d = z - mu0 with mu0 a first
  // estimate of the mean (the plain sum / E in the forward, the saved mean in the backward), then
  // c = sum(d) / E and d -= c. d is then the deviation from the mean to f32 precision of the
  // DEVIATIONS, and the variance is sum(d^2) / E about it (never E[x^2] - mean^2).
  static constexpr bool kRecentre = true;
  static constexpr bool kRelu = true;  // with the launch's relu flag: y = relu(y), dy masked by y > 0
};

template <class K>
__device__ __forceinline__ float ln_at(const float* __restrict__ x, const float* __restrict__ res,
                                       int64_t i) {
  if constexpr (K::kRes) return x[i] + res[i];
  else return x[i];
}

template <class K, int PL>
__device__ __forceinline__ void ln_load(float (&z)[PL], const float* __restrict__ x,
                                        const float* __restrict__ res, int64_t r, int lane, int E) {
#pragma unroll
  for (int k = 0; k < PL; ++k) {
    const int e = lane + k * kWave;
    z[k] = e < E ? ln_at<K>(x, res, r * E + e) : 0.f;
  }
}

// d -= mu0 (and, kRecentre, the mean c of what is left, which is returned); lanes past E hold 0
template <class K, int PL>
__device__ __forceinline__ float ln_center(float (&d)[PL], int lane, int E, float mu0,
                                           float inv_e) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < PL; ++k) {
    d[k] = lane + k * kWave < E ? d[k] - mu0 : 0.f;
    s += d[k];
  }
  if constexpr (!K::kRecentre) return 0.f;
  const float c = wave_sum(s) * inv_e;
#pragma unroll
  for (int k = 0; k < PL; ++k) d[k] = lane + k * kWave < E ? d[k] - c : 0.f;
  return c;
}

template <class K, int PL>
__global__ __launch_bounds__(kLnWaves* kWave) void layernorm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
    const float* __restrict__ beta, int64_t R, int E, float eps, int relu, float* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const float inv_e = 1.0f / static_cast<float>(E);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kLnWaves + wv; r < R;
       r += static_cast<int64_t>(gridDim.x) * kLnWaves) {
    float d[PL];
    ln_load<K, PL>(d, x, res, r, lane, E);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PL; ++k) s += d[k];
    const float mu0 = wave_sum(s) * inv_e;
    const float c = ln_center<K, PL>(d, lane, E, mu0, inv_e);
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < PL; ++k) sq += d[k] * d[k];
    const float rs = 1.0f / sqrtf(wave_sum(sq) * inv_e + eps);
#pragma unroll
    for (int k = 0; k < PL; ++k) {
      const int e = lane + k * kWave;
      if (e < E) {
        const float v = (d[k] * rs) * gamma[e] + beta[e];
        if constexpr (K::kRelu) y[r * E + e] = relu ? relu_f(v) : v;
        else y[r * E + e] = v;
      }
    }
    if (lane == 0) {
      if constexpr (K::kRecentre) mean[r] = mu0 + c;
      else mean[r] = mu0;
      rstd[r] = rs;
    }
  }
}

// dx per row, and this workgroup's dgamma / dbeta partial: rows blockIdx * 4 + wave, stepping by
// the grid, summed per wave in row order, then waves 0..3 in order -> part[blockIdx][2][E]
template <class K, int PL>
__global__ __launch_bounds__(kLnWaves* kWave) void layernorm_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ res,
    const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, int64_t R, int E, int relu, float* __restrict__ dx,
    float* __restrict__ part) {
  __shared__ float s_g[kLnWaves][PL * kWave], s_b[kLnWaves][PL * kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const float inv_e = 1.0f / static_cast<float>(E);
  float gm[PL], dg[PL], db[PL];
#pragma unroll
  for (int k = 0; k < PL; ++k) {
    const int e = lane + k * kWave;
    gm[k] = e < E ? gamma[e] : 0.f;
    dg[k] = db[k] = 0.f;
  }
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kLnWaves + wv; r < R;
       r += static_cast<int64_t>(gridDim.x) * kLnWaves) {
    const float mu = mean[r], rs = rstd[r];
    float xh[PL], g[PL];
    if constexpr (K::kRecentre) {  // needs the whole row first; one step is taken with dy's loads
      ln_load<K, PL>(xh, x, res, r, lane, E);
      ln_center<K, PL>(xh, lane, E, mu, inv_e);
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < PL; ++k) {
      const int e = lane + k * kWave;
      const bool in = e < E;
      float d = 0.f;
      if (in) {
        d = dy[r * E + e];
        if constexpr (K::kRelu)
          if (relu && !(y[r * E + e] > 0.f)) d = 0.f;
      }
      if constexpr (K::kRecentre) xh[k] = xh[k] * rs;
      else xh[k] = in ? (ln_at<K>(x, res, r * E + e) - mu) * rs : 0.f;
      g[k] = d * gm[k];
      s1 += g[k];
      s2 += g[k] * xh[k];
      dg[k] += d * xh[k];
      db[k] += d;
    }
    const float c1 = wave_sum(s1) * inv_e, c2 = wave_sum(s2) * inv_e;
#pragma unroll
    for (int k = 0; k < PL; ++k) {
      const int e = lane + k * kWave;
      if (e < E) dx[r * E + e] = rs * ((g[k] - c1) - xh[k] * c2);
    }
  }
#pragma unroll
  for (int k = 0; k < PL; ++k) {
    s_g[wv][lane + k * kWave] = dg[k];
    s_b[wv][lane + k * kWave] = db[k];
  }
  __syncthreads();
  float* pg = part + static_cast<int64_t>(blockIdx.x) * 2 * E;
  for (int e = threadIdx.x; e < E; e += kLnWaves * kWave) {
    float a = s_g[0][e], c = s_b[0][e];
    for (int w = 1; w < kLnWaves; ++w) {
      a += s_g[w][e];
      c += s_b[w][e];
    }
    pg[e] = a;
    pg[E + e] = c;
  }
}

// dgamma / dbeta = the partials summed in workgroup order (static: one copy per including file)
static __global__ __launch_bounds__(256) void layernorm_finish_kernel(
    const float* __restrict__ part, int nb, int E, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * E) return;
  float a = 0.f;
  for (int p = 0; p < nb; ++p) a += part[static_cast<int64_t>(p) * 2 * E + t];
  if (t < E) dgamma[t] = a;
  else dbeta[t - E] = a;
}

// workgroups of the backward for R rows (its grid, and the partials the finish sums)
inline int ln_parts(int64_t R) {
  const int64_t nb = ceil_div(R, kLnWaves);
  return static_cast<int>(nb < kLnMaxParts ? (nb > 0 ? nb : 1) : kLnMaxParts);
}

inline size_t ln_workspace_bytes(int64_t R, int64_t E) {
  return static_cast<size_t>(ln_parts(R)) * 2 * static_cast<size_t>(E) * sizeof(float);
}

// The backward's two launches on `part` (ln_workspace_bytes(R, E), checked by the caller)
template <class K, int PL>
inline int ln_bwd_launch(const char* who, const char* who_finish, hipStream_t s, const float* dy,
                         const float* x, const float* res, const float* y, const float* gamma,
                         const float* mean, const float* rstd, int64_t R, int64_t E, int relu,
                         float* dx, float* dgamma, float* dbeta, float* part) {
  const int nb = ln_parts(R);
  hipLaunchKernelGGL((layernorm_bwd_kernel<K, PL>), dim3(nb), dim3(kLnWaves * kWave), 0, s, dy, x,
                     res, y, gamma, mean, rstd, R, (int)E, relu, dx, part);
  if (int rc = check_launch(who)) return rc;
  hipLaunchKernelGGL(layernorm_finish_kernel, dim3(static_cast<unsigned>(ceil_div(2 * E, 256))),
                     dim3(256), 0, s, part, nb, (int)E, dgamma, dbeta);
  return check_launch(who_finish);
}

}  // namespace ocppo
