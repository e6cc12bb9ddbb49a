// LayerNorm over [C, H, W] + ReLU with its backward: the three wide LayerNorms of
// pqn_atari_envpool.py's pixel QNetwork (:119-131; rows of 32*20*20, 64*9*9 and 64*7*7 floats),
// which ocppo_layernorm.h's one-wave-per-row kernels cannot hold. f32, wave64, no atomics: every
// sum runs in an order fixed by the shapes alone.
//
// Work split. One workgroup of 256 threads takes one row of E = C*HW floats at a time, rows
// blockIdx, blockIdx + gridDim, ... The WHOLE row stays in registers between the passes over it:
// thread t holds PT / 4 float4s at memory index 4 (t + 256 k) (PT floats at t + 256 k on the
// scalar path: E % 4 != 0 or a misaligned pointer), PT in {4, 16, 32, 64} for E <= 1024 .. 16384.
// The forward reads x once and writes y once; the backward reads dy, x, y once each and writes
// dx once. A row-wide sum is ocppo_common.h's block_sum: lanes by butterfly, then the four waves
// through LDS in wave order.
//
// Arithmetic: ocppo_layernorm.h's LnRelu scheme. d = x - mu0 with mu0 the plain mean (forward) or
// the saved mean (backward), c = mean(d), d -= c; variance = mean(d^2). ReLU mask: y > 0.
//
// Parameters. gamma / beta are always in the module's [C, H, W] order: parameter index
// j = c HW + p. The activation's memory index m is j (NCHW) or p C + c (channels-last, what
// ops.conv_x6 writes). A thread needs the parameters of ITS memory indices, once per workgroup,
// and keeps them in registers over its rows. Channels-last: reading parameter j(m) straight from
// global memory would be one cache line per lane (stride HW), ~E line requests per array against
// E / 32 for the row itself; instead the workgroup reads the array in parameter order (coalesced),
// parks it in LDS with the channel stride padded to an odd number of floats (so that lanes on
// consecutive channels fall on different banks) and each thread picks its own from there.
//
// dgamma / dbeta. A backward workgroup sums its rows' contributions per column in row order --
// in LDS cells that only the owning thread touches (two floats per column: 128 KB of the CU's
// 160 KB at E = 16384), or not at all when it has a single row (R <= the partial count: the
// update's case), where the row's terms are the partial -- and stores one partial [2][E] in
// MEMORY order with plain stores. The finish launch reads the partials coalesced, eight ordered
// segments of workgroups per column in flight at once, sums each segment in workgroup order and
// the segments in order, and writes dgamma / dbeta through the index map in [C, H, W] order.
// The partial count is min(R, OCPPO_LN_CHW_MAX_PARTS = 256): a function of R alone, so a result
// does not depend on the device. 256 and not ocppo_layernorm.h's 128: there a workgroup holds
// four rows of <= 1024 floats and 128 workgroups of small rows keep enough loads in flight; here
// a workgroup is one row of up to 64 KB at one wave per SIMD, the update's minibatch is 256 rows,
// and 256 partials put one row on each of the chip's 256 CUs, where 128 would leave half of them
// idle for twice as long. The price is the partials' traffic (2 E floats per workgroup, written
// once and read once: as much again as dy and x), which the 256 MB last-level cache absorbs.
#include "ocppo_common.h"

namespace ocppo {

constexpr int kChwThreads = 256;
constexpr int kChwMaxE = OCPPO_LN_CHW_MAX_E;
constexpr int kChwMaxParts = OCPPO_LN_CHW_MAX_PARTS;
constexpr int kChwFwdGrid = 1024;   // forward workgroups: rows beyond that by grid stride
constexpr int kChwFinSegs = 8;      // finish: ordered segments of partials summed side by side
constexpr int kChwFinCols = 64;     // finish: columns per workgroup (one wave wide)

// (q, r) = divmod(n, d), stepped by a constant without dividing again
struct DivMod {
  unsigned q, r;
};
__device__ __forceinline__ DivMod divmod(unsigned n, unsigned d) { return {n / d, n % d}; }
__device__ __forceinline__ void advance(DivMod& a, DivMod step, unsigned d) {
  a.q += step.q;
  a.r += step.r;
  if (a.r >= d) {
    a.r -= d;
    ++a.q;
  }
}

// memory index of register k of this thread
template <bool VEC>
__device__ __forceinline__ int chw_index(int k) {
  if constexpr (VEC) return 4 * (static_cast<int>(threadIdx.x) + kChwThreads * (k / 4)) + (k & 3);
  else return static_cast<int>(threadIdx.x) + kChwThreads * k;
}

// One row (or a parameter array in memory order) into registers; indices past E hold 0
template <int PT, bool VEC>
__device__ __forceinline__ void chw_load(float (&v)[PT], const float* __restrict__ p, int E) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < PT; k += 4) {
      const int m = chw_index<true>(k);
      const float4 q = m < E ? *reinterpret_cast<const float4*>(p + m) : make_float4(0, 0, 0, 0);
      v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      const int m = chw_index<false>(k);
      v[k] = m < E ? p[m] : 0.f;
    }
  }
}

template <int PT, bool VEC>
__device__ __forceinline__ void chw_store(float* __restrict__ p, const float (&v)[PT], int E) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < PT; k += 4) {
      const int m = chw_index<true>(k);
      if (m < E) *reinterpret_cast<float4*>(p + m) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      const int m = chw_index<false>(k);
      if (m < E) p[m] = v[k];
    }
  }
}

// This thread's parameters: g[k] = src[j(chw_index(k))]. cl: through `stage` (C * (HW | 1) floats
// of LDS), see the file comment; every thread of the workgroup calls it.
template <int PT, bool VEC>
__device__ __forceinline__ void chw_load_param(float (&g)[PT], const float* __restrict__ src,
                                               float* stage, int E, int C, int HW, int cl) {
  if (!cl) {
    chw_load<PT, VEC>(g, src, E);
    return;
  }
  const unsigned hw = HW, hwp = HW | 1, c = C;
  // parameter order, coalesced: j = t + 256 k = ch * HW + pos -> stage[ch * hwp + pos]
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    const int j = static_cast<int>(threadIdx.x) + kChwThreads * k;
    g[k] = j < E ? src[j] : 0.f;
  }
  DivMod a = divmod(threadIdx.x, hw);
  const DivMod step = divmod(kChwThreads, hw);
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    if (static_cast<int>(threadIdx.x) + kChwThreads * k < E) stage[a.q * hwp + a.r] = g[k];
    advance(a, step, hw);
  }
  __syncthreads();
  // memory order: m = pos * C + ch
  if constexpr (VEC) {
    DivMod b = divmod(4 * threadIdx.x, c);
    const DivMod bstep = divmod(4 * kChwThreads, c), one = {0u, 1u};
#pragma unroll
    for (int k = 0; k < PT; k += 4) {
      DivMod e = b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[k + i] = chw_index<true>(k + i) < E ? stage[e.r * hwp + e.q] : 0.f;
        advance(e, one, c);
      }
      advance(b, bstep, c);
    }
  } else {
    DivMod b = divmod(threadIdx.x, c);
    const DivMod bstep = divmod(kChwThreads, c);
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      g[k] = chw_index<false>(k) < E ? stage[b.r * hwp + b.q] : 0.f;
      advance(b, bstep, c);
    }
  }
  __syncthreads();  // the stage is free again
}

// d -= mu0, then the mean c of what is left (returned); indices past E stay 0
template <int PT, bool VEC>
__device__ __forceinline__ float chw_center(float (&d)[PT], int E, float mu0, float inv_e,
                                            float* red) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    d[k] = chw_index<VEC>(k) < E ? d[k] - mu0 : 0.f;
    s += d[k];
  }
  const float c = block_sum(s, red) * inv_e;
#pragma unroll
  for (int k = 0; k < PT; ++k) d[k] = chw_index<VEC>(k) < E ? d[k] - c : 0.f;
  return c;
}

template <int PT, bool VEC>
__global__ __launch_bounds__(kChwThreads) void ln_chw_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    int64_t R, int E, int C, int HW, int cl, float eps, int relu, float* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd) {
  extern __shared__ float stage[];
  __shared__ float red[kChwThreads / kWave];
  const float inv_e = 1.0f / static_cast<float>(E);
  float gm[PT], bt[PT];
  chw_load_param<PT, VEC>(gm, gamma, stage, E, C, HW, cl);
  chw_load_param<PT, VEC>(bt, beta, stage, E, C, HW, cl);
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    float d[PT];
    chw_load<PT, VEC>(d, x + r * E, E);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PT; ++k) s += d[k];
    const float mu0 = block_sum(s, red) * inv_e;
    const float c = chw_center<PT, VEC>(d, E, mu0, inv_e, red);
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < PT; ++k) sq += d[k] * d[k];
    const float rs = 1.0f / sqrtf(block_sum(sq, red) * inv_e + eps);
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      const float v = (d[k] * rs) * gm[k] + bt[k];
      d[k] = relu ? relu_f(v) : v;
    }
    chw_store<PT, VEC>(y + r * E, d, E);
    if (threadIdx.x == 0) {
      mean[r] = mu0 + c;
      rstd[r] = rs;
    }
  }
}

// dx per row, and this workgroup's dgamma / dbeta partial part[blockIdx][2][E] in memory order.
// MULTI: the workgroup may have several rows; their terms are summed in row order in LDS cells
// acc[2][PT * 256] private to a thread (the parameter stage's bytes, free by then).
template <int PT, bool VEC, bool MULTI>
__global__ __launch_bounds__(kChwThreads) void ln_chw_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, int64_t R, int E, int C, int HW, int cl, int relu,
    float* __restrict__ dx, float* __restrict__ part) {
  extern __shared__ float stage[];
  __shared__ float red[kChwThreads / kWave];
  const float inv_e = 1.0f / static_cast<float>(E);
  float gm[PT];
  chw_load_param<PT, VEC>(gm, gamma, stage, E, C, HW, cl);
  float* acc_g = stage + threadIdx.x;
  float* acc_b = acc_g + PT * kChwThreads;
  float* pg = part + static_cast<int64_t>(blockIdx.x) * 2 * E;
  bool first = true;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const float mu = mean[r], rs = rstd[r];
    float xh[PT], g[PT];
    chw_load<PT, VEC>(xh, x + r * E, E);
    chw_load<PT, VEC>(g, dy + r * E, E);
    if (relu) {  // dy masked by y > 0
      float yv[PT];
      chw_load<PT, VEC>(yv, y + r * E, E);
#pragma unroll
      for (int k = 0; k < PT; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
    }
    chw_center<PT, VEC>(xh, E, mu, inv_e, red);
    float s1 = 0.f, s2 = 0.f;
    float tg[PT];  // this row's dgamma terms; g holds dbeta's until it is scaled by gamma
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      xh[k] = xh[k] * rs;
      tg[k] = g[k] * xh[k];
    }
    if constexpr (MULTI) {
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        acc_g[k * kChwThreads] = first ? tg[k] : acc_g[k * kChwThreads] + tg[k];
        acc_b[k * kChwThreads] = first ? g[k] : acc_b[k * kChwThreads] + g[k];
      }
      first = false;
    } else {
      chw_store<PT, VEC>(pg, tg, E);
      chw_store<PT, VEC>(pg + E, g, E);
    }
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      g[k] = g[k] * gm[k];
      s1 += g[k];
      s2 += g[k] * xh[k];
    }
    const float c1 = block_sum(s1, red) * inv_e, c2 = block_sum(s2, red) * inv_e;
#pragma unroll
    for (int k = 0; k < PT; ++k) g[k] = rs * ((g[k] - c1) - xh[k] * c2);
    chw_store<PT, VEC>(dx + r * E, g, E);
  }
  if constexpr (MULTI) {
    float t[PT];
#pragma unroll
    for (int k = 0; k < PT; ++k) t[k] = acc_g[k * kChwThreads];
    chw_store<PT, VEC>(pg, t, E);
#pragma unroll
    for (int k = 0; k < PT; ++k) t[k] = acc_b[k * kChwThreads];
    chw_store<PT, VEC>(pg + E, t, E);
  }
}

// dgamma / dbeta from nb partials [2][E] in memory order. Thread (seg, lane): column
// blockIdx * 64 + lane of the 2 E, partials [seg * per, (seg + 1) * per) in workgroup order; the
// eight segment sums are added in segment order and stored at the column's parameter index.
__global__ __launch_bounds__(kChwFinSegs* kChwFinCols) void ln_chw_finish_kernel(
    const float* __restrict__ part, int nb, int E, int C, int HW, int cl,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float s_sum[kChwFinSegs][kChwFinCols];
  const int lane = threadIdx.x & (kChwFinCols - 1), seg = threadIdx.x / kChwFinCols;
  const int t = blockIdx.x * kChwFinCols + lane;
  const int per = (nb + kChwFinSegs - 1) / kChwFinSegs;
  const int p0 = seg * per, p1 = min(nb, p0 + per);
  float a = 0.f;
  if (t < 2 * E) {
    const float* src = part + t;
    const int64_t stride = 2 * static_cast<int64_t>(E);
    int p = p0;
    for (; p + 8 <= p1; p += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[(p + i) * stride];
#pragma unroll
      for (int i = 0; i < 8; ++i) a += v[i];
    }
    for (; p < p1; ++p) a += src[p * stride];
  }
  s_sum[seg][lane] = a;
  __syncthreads();
  if (seg != 0 || t >= 2 * E) return;
  for (int s = 1; s < kChwFinSegs; ++s) a += s_sum[s][lane];
  const int m = t < E ? t : t - E;
  const int j = cl ? (m % C) * HW + m / C : m;
  (t < E ? dgamma : dbeta)[j] = a;
}

inline int chw_parts(int64_t R) {
  return static_cast<int>(R < kChwMaxParts ? (R > 0 ? R : 1) : kChwMaxParts);
}

// LDS floats of the channels-last parameter stage (0: the index map is the identity)
inline size_t chw_stage_floats(int64_t C, int64_t HW, int cl) {
  return cl ? static_cast<size_t>(C) * static_cast<size_t>(HW | 1) : 0;
}

inline bool chw_vec(int64_t E, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = static_cast<uintptr_t>(E) & 3;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p) & 15;
  return bits == 0;
}

// More than 64 KB of dynamic LDS (the CU has 160 KB) is asked for per kernel, before its launch
template <class K>
inline void chw_allow_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

}  // namespace ocppo

using namespace ocppo;

// registers per thread: 4, 16, 32 or 64 floats of the row
#define OCPPO_CHW_DISPATCH(E, CALL)                      \
  if ((E) <= 1024) { constexpr int PT = 4; CALL; }       \
  else if ((E) <= 4096) { constexpr int PT = 16; CALL; } \
  else if ((E) <= 8192) { constexpr int PT = 32; CALL; } \
  else { constexpr int PT = 64; CALL; }

static int chw_check(const char* who, int64_t R, int64_t C, int64_t HW) {
  OCPPO_REQUIRE(R >= 0 && R <= INT32_MAX && C >= 1 && HW >= 1 && C <= kChwMaxE &&
                    HW <= kChwMaxE && C * HW <= kChwMaxE,
                "%s: bad sizes R=%lld C=%lld HW=%lld (R >= 0, C, HW >= 1, C HW <= %d)", who,
                (long long)R, (long long)C, (long long)HW, kChwMaxE);
  return OCPPO_OK;
}

extern "C" int ocppo_ln_chw_relu_fwd(ocppo_stream_t stream, const float* x, const float* gamma,
                                     const float* beta, int64_t R, int64_t C, int64_t HW,
                                     int channels_last, double eps, int relu, float* y,
                                     float* mean, float* rstd) {
  if (int rc = chw_check("ocppo_ln_chw_relu_fwd", R, C, HW)) return rc;
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && gamma && beta && y && mean && rstd, "ocppo_ln_chw_relu_fwd: null pointer");
  const int64_t E = C * HW;
  const int cl = channels_last && C > 1 && HW > 1;
  const bool vec = chw_vec(E, {x, gamma, beta, y});
  const size_t lds = chw_stage_floats(C, HW, cl) * sizeof(float);
  const dim3 grid(static_cast<unsigned>(R < kChwFwdGrid ? R : kChwFwdGrid));
  clear_stale_error();
#define OCPPO_CHW_FWD(V)                                                                       \
  {                                                                                            \
    auto kernel = ln_chw_fwd_kernel<PT, V>;                                                    \
    chw_allow_lds(kernel, lds);                                                                \
    hipLaunchKernelGGL(kernel, grid, dim3(kChwThreads), lds, as_stream(stream), x, gamma, beta, \
                       R, (int)E, (int)C, (int)HW, cl, static_cast<float>(eps), relu ? 1 : 0,  \
                       y, mean, rstd);                                                         \
  }
  if (vec) { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_FWD(true)); }
  else { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_FWD(false)); }
#undef OCPPO_CHW_FWD
  return check_launch("ocppo_ln_chw_relu_fwd");
}

extern "C" size_t ocppo_ln_chw_workspace_bytes(int64_t R, int64_t E) {
  if (R < 0 || E < 1 || E > kChwMaxE) return 0;
  return static_cast<size_t>(chw_parts(R)) * 2 * static_cast<size_t>(E) * sizeof(float);
}

extern "C" int ocppo_ln_chw_relu_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                     const float* y, const float* gamma, const float* mean,
                                     const float* rstd, int64_t R, int64_t C, int64_t HW,
                                     int channels_last, int relu, float* dx, float* dgamma,
                                     float* dbeta, void* workspace, size_t workspace_bytes) {
  if (int rc = chw_check("ocppo_ln_chw_relu_bwd", R, C, HW)) return rc;
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dy && x && (y || !relu) && gamma && mean && rstd && dx && dgamma && dbeta,
                "ocppo_ln_chw_relu_bwd: null pointer");
  const int64_t E = C * HW;
  const size_t need = ocppo_ln_chw_workspace_bytes(R, E);
  if (!workspace || workspace_bytes < need)
    return fail(OCPPO_E_WORKSPACE, "ocppo_ln_chw_relu_bwd: workspace of %zu bytes, need %zu",
                workspace_bytes, need);
  const int cl = channels_last && C > 1 && HW > 1;
  // the workspace's rows are 2 E floats apart: with E % 4 == 0 they keep its alignment
  const bool vec = chw_vec(E, {dy, x, y, gamma, dx, workspace});
  const int nb = chw_parts(R);
  const bool multi = R > nb;
  float* part = static_cast<float*>(workspace);
  hipStream_t s = as_stream(stream);
  clear_stale_error();
#define OCPPO_CHW_BWD(V, M)                                                                     \
  {                                                                                             \
    size_t lds = chw_stage_floats(C, HW, cl) * sizeof(float);                                   \
    const size_t acc = (M) ? size_t(2) * PT * kChwThreads * sizeof(float) : 0;                  \
    lds = lds > acc ? lds : acc;                                                                \
    auto kernel = ln_chw_bwd_kernel<PT, V, M>;                                                  \
    chw_allow_lds(kernel, lds);                                                                 \
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(kChwThreads), lds, s, dy, x, y, gamma, mean, rstd, \
                       R, (int)E, (int)C, (int)HW, cl, relu ? 1 : 0, dx, part);                 \
  }
  if (vec && multi) { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_BWD(true, true)); }
  else if (vec) { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_BWD(true, false)); }
  else if (multi) { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_BWD(false, true)); }
  else { OCPPO_CHW_DISPATCH(E, OCPPO_CHW_BWD(false, false)); }
#undef OCPPO_CHW_BWD
  if (int rc = check_launch("ocppo_ln_chw_relu_bwd")) return rc;
  hipLaunchKernelGGL(ln_chw_finish_kernel,
                     dim3(static_cast<unsigned>(ceil_div(2 * E, kChwFinCols))),
                     dim3(kChwFinSegs * kChwFinCols), 0, s, part, nb, (int)E, (int)C, (int)HW, cl,
                     dgamma, dbeta);
  return check_launch("ocppo_ln_chw_relu_bwd (finish)");
}
#undef OCPPO_CHW_DISPATCH
