// The first two steps of SimpleViT's patch embedding (cleanrl/ppo_atari_vit.py through
// vit_pytorch: Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)') -> LayerNorm(C p^2)) read
// straight from the rollout's u8 frame stacks through the minibatch's row indices, with the
// LayerNorm's parameter gradients. In torch that is a u8 -> f32 conversion, a permuting copy and a
// LayerNorm: three passes over B x C x 84 x 84 floats; here the pixels are read once as bytes and
// the only f32 traffic is y (and dy in the backward).
//
// Geometry: H = 84, patch p in {12, 14, 21} (a template parameter: every division by p is by a
// constant), 1 <= C <= 8. E = C p^2 columns per token, Tw = 84 / p tokens per patch row, T = Tw^2.
// Column e = (p1 p + p2) C + c is pixel (c, h p + p1, w p + p2) of token (h, w).
//
// Work unit = (output row, patch row h): the C slabs of p x 84 bytes that hold its Tw tokens are
// contiguous in the source, staged to LDS with 4-byte loads (<= 14 KB).
// Forward: wave w of the 256-thread workgroup takes tokens w, w + 4, ... of the unit; lane l owns
// the patch pixels q = l + 64 k (<= 7 of them, LDS offsets kept in registers) and walks the C
// channels of each. The pixels are integers, so the first sum is an exact u32 sum and
// mu0 = float(sum) / E is correctly rounded: a constant patch has d = x - mu0 = 0 exactly and
// y = beta. Then ocppo_ln_relu_fwd's scheme: c = mean(d), d -= c, var = mean(d^2),
// rstd = 1 / sqrt(var + eps); mean = mu0 + c. Values stay on the 0-255 scale, as the reference's.
// Backward (dgamma, dbeta; pixels need no gradient): thread t owns columns t + 256 k (<= 14) and
// sums g x^ and g over the tokens of its workgroup's units in order, x^ = (x - mean) rstd from the
// staged bytes; min(units, 256) workgroups -- a function of R and p alone -- store one partial
// [2][E] each with plain stores, and a second launch adds them in workgroup order. No atomics.
#include "ocppo_common.h"

namespace ocppo {

constexpr int kVpH = 84;
constexpr int kVpThreads = 256;
constexpr int kVpMaxC = 8;
constexpr int kVpMaxParts = 256;
constexpr int kVpMaxE = kVpMaxC * 21 * 21;                             // 3528
constexpr int kVpMaxK = (kVpMaxE + kVpThreads - 1) / kVpThreads;       // 14 columns per thread
constexpr int kVpMaxBytes = kVpMaxC * 21 * kVpH;                       // a unit's pixels

// source row of output row rr: idx[rr] clamped into [0, rows) (never dereferenced outside), or rr
__device__ __forceinline__ int64_t vp_src_row(const int64_t* __restrict__ idx, int64_t rr,
                                              int64_t rows) {
  int64_t n = idx ? idx[rr] : rr;
  n = n < 0 ? 0 : n;
  return n >= rows ? rows - 1 : n;
}

// the unit's C slabs of P x 84 bytes -> s_px[(c P + p1) 84 + column]
template <int P>
__device__ __forceinline__ void vp_stage(uint32_t* s_px, const uint8_t* __restrict__ src,
                                         int64_t n, int C, int h) {
  constexpr int SLAB = P * kVpH / 4;  // words per channel
  for (int i = threadIdx.x; i < C * SLAB; i += kVpThreads) {
    const int c = i / SLAB, rem = i - c * SLAB;
    const uint8_t* p = src + ((n * C + c) * kVpH + h * P) * kVpH;
    s_px[i] = reinterpret_cast<const uint32_t*>(p)[rem];
  }
}

template <int P>
__global__ __launch_bounds__(kVpThreads) void vit_patch_ln_fwd_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ idx, int64_t rows, int64_t R,
    int C, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd) {
  constexpr int TW = kVpH / P, PP = P * P, NK = (PP + kWave - 1) / kWave;
  __shared__ uint32_t s_px32[kVpMaxBytes / 4];
  const uint8_t* s_px = reinterpret_cast<const uint8_t*>(s_px32);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int E = C * PP, slab = P * kVpH;
  const float fe = static_cast<float>(E);
  int off[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int q = lane + kWave * k, p1 = q / P;
    off[k] = p1 * kVpH + (q - p1 * P);
  }
  for (int64_t unit = blockIdx.x; unit < R * TW; unit += gridDim.x) {
    const int64_t rr = unit / TW;
    const int h = static_cast<int>(unit - rr * TW);
    __syncthreads();  // the previous unit's pixels are read
    vp_stage<P>(s_px32, src, vp_src_row(idx, rr, rows), C, h);
    __syncthreads();
    for (int w = wv; w < TW; w += kVpThreads / kWave) {
      const int64_t tok = (rr * TW + h) * TW + w;
      const uint8_t* px = s_px + w * P;
      uint32_t isum = 0;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (lane + kWave * k < PP)
          for (int c = 0; c < C; ++c) isum += px[c * slab + off[k]];
      const float mu0 = static_cast<float>(wave_sum(isum)) / fe;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (lane + kWave * k < PP)
          for (int c = 0; c < C; ++c) s += static_cast<float>(px[c * slab + off[k]]) - mu0;
      const float cc = wave_sum(s) / fe;
      float sq = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (lane + kWave * k < PP)
          for (int c = 0; c < C; ++c) {
            const float d = (static_cast<float>(px[c * slab + off[k]]) - mu0) - cc;
            sq += d * d;
          }
      const float rs = 1.0f / sqrtf(wave_sum(sq) / fe + eps);
      float* yt = y + tok * E;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int q = lane + kWave * k;
        if (q < PP)
          for (int c = 0; c < C; ++c) {
            const int e = q * C + c;
            const float d = (static_cast<float>(px[c * slab + off[k]]) - mu0) - cc;
            yt[e] = (d * rs) * gamma[e] + beta[e];
          }
      }
      if (lane == 0) {
        mean[tok] = mu0 + cc;
        rstd[tok] = rs;
      }
    }
  }
}

template <int P>
__global__ __launch_bounds__(kVpThreads) void vit_patch_ln_bwd_kernel(
    const float* __restrict__ dy, const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
    int64_t rows, int64_t R, int C, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part) {
  constexpr int TW = kVpH / P, PP = P * P;
  __shared__ uint32_t s_px32[kVpMaxBytes / 4];
  const uint8_t* s_px = reinterpret_cast<const uint8_t*>(s_px32);
  const int E = C * PP;
  int off[kVpMaxK];
  float ag[kVpMaxK], ab[kVpMaxK];
#pragma unroll
  for (int k = 0; k < kVpMaxK; ++k) {
    const int e = static_cast<int>(threadIdx.x) + kVpThreads * k;
    const int q = e / C, c = e - q * C, p1 = q / P;
    off[k] = (c * P + p1) * kVpH + (q - p1 * P);
    ag[k] = 0.f;
    ab[k] = 0.f;
  }
  for (int64_t unit = blockIdx.x; unit < R * TW; unit += gridDim.x) {
    const int64_t rr = unit / TW;
    const int h = static_cast<int>(unit - rr * TW);
    __syncthreads();
    vp_stage<P>(s_px32, src, vp_src_row(idx, rr, rows), C, h);
    __syncthreads();
    for (int w = 0; w < TW; ++w) {
      const int64_t tok = (rr * TW + h) * TW + w;
      const float mu = mean[tok], rs = rstd[tok];
      const float* g = dy + tok * E;
#pragma unroll
      for (int k = 0; k < kVpMaxK; ++k) {
        const int e = static_cast<int>(threadIdx.x) + kVpThreads * k;
        if (e < E) {
          const float gv = g[e];
          const float xh = (static_cast<float>(s_px[off[k] + w * P]) - mu) * rs;
          ag[k] += gv * xh;
          ab[k] += gv;
        }
      }
    }
  }
  float* pg = part + static_cast<int64_t>(blockIdx.x) * 2 * E;
#pragma unroll
  for (int k = 0; k < kVpMaxK; ++k) {
    const int e = static_cast<int>(threadIdx.x) + kVpThreads * k;
    if (e < E) {
      pg[e] = ag[k];
      pg[E + e] = ab[k];
    }
  }
}

// column t of the 2 E: the nb partials in workgroup order
__global__ __launch_bounds__(kVpThreads) void vit_patch_ln_finish_kernel(
    const float* __restrict__ part, int nb, int E, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  const int t = blockIdx.x * kVpThreads + threadIdx.x;
  if (t >= 2 * E) return;
  float a = 0.f;
  for (int p = 0; p < nb; ++p) a += part[static_cast<int64_t>(p) * 2 * E + t];
  (t < E ? dgamma : dbeta)[t < E ? t : t - E] = a;
}

static int vp_check(const char* who, int64_t rows, int64_t R, int64_t C, int64_t H, int64_t p) {
  OCPPO_REQUIRE(rows >= 1 && R >= 0 && R <= (int64_t(1) << 24) && rows <= (int64_t(1) << 31) &&
                    C >= 1 && C <= kVpMaxC && H == kVpH && (p == 12 || p == 14 || p == 21),
                "%s: bad sizes rows=%lld R=%lld C=%lld H=%lld p=%lld (H = 84, p in {12, 14, 21}, "
                "1 <= C <= %d)",
                who, (long long)rows, (long long)R, (long long)C, (long long)H, (long long)p,
                kVpMaxC);
  return OCPPO_OK;
}

inline int vp_parts(int64_t R, int64_t p) {
  const int64_t units = R * (kVpH / p);
  return static_cast<int>(units < kVpMaxParts ? (units > 0 ? units : 1) : kVpMaxParts);
}

}  // namespace ocppo

using namespace ocppo;

#define OCPPO_VP_DISPATCH(PV, CALL)                  \
  switch (PV) {                                      \
    case 12: { constexpr int P = 12; CALL; break; }  \
    case 14: { constexpr int P = 14; CALL; break; }  \
    default: { constexpr int P = 21; CALL; break; }  \
  }

extern "C" int ocppo_vit_patch_ln_fwd(ocppo_stream_t stream, const uint8_t* src,
                                      const int64_t* idx, int64_t rows, int64_t R, int64_t C,
                                      int64_t H, int64_t patch, const float* gamma,
                                      const float* beta, double eps, float* y, float* mean,
                                      float* rstd) {
  const char* who = "ocppo_vit_patch_ln_fwd";
  if (int rc = vp_check(who, rows, R, C, H, patch)) return rc;
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(src && gamma && beta && y && mean && rstd, "%s: null pointer", who);
  OCPPO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0, "%s: src not 4-B aligned", who);
  const int64_t units = R * (kVpH / patch);
  const dim3 grid(static_cast<unsigned>(units < 4096 ? units : 4096));
  clear_stale_error();
  OCPPO_VP_DISPATCH(patch, hipLaunchKernelGGL(vit_patch_ln_fwd_kernel<P>, grid, dim3(kVpThreads),
                                              0, as_stream(stream), src, idx, rows, R, (int)C,
                                              gamma, beta, static_cast<float>(eps), y, mean,
                                              rstd));
  return check_launch(who);
}

extern "C" size_t ocppo_vit_patch_workspace_bytes(int64_t R, int64_t C, int64_t patch) {
  if (R < 0 || C < 1 || C > kVpMaxC || !(patch == 12 || patch == 14 || patch == 21)) return 0;
  return static_cast<size_t>(vp_parts(R, patch)) * 2 * static_cast<size_t>(C * patch * patch) *
         sizeof(float);
}

extern "C" int ocppo_vit_patch_ln_bwd(ocppo_stream_t stream, const float* dy, const uint8_t* src,
                                      const int64_t* idx, int64_t rows, int64_t R, int64_t C,
                                      int64_t H, int64_t patch, const float* mean,
                                      const float* rstd, float* dgamma, float* dbeta,
                                      void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_vit_patch_ln_bwd";
  if (int rc = vp_check(who, rows, R, C, H, patch)) return rc;
  OCPPO_REQUIRE(R >= 1, "%s: R = 0 has no gradient", who);
  OCPPO_REQUIRE(dy && src && mean && rstd && dgamma && dbeta, "%s: null pointer", who);
  OCPPO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0, "%s: src not 4-B aligned", who);
  const size_t need = ocppo_vit_patch_workspace_bytes(R, C, patch);
  if (!workspace || workspace_bytes < need)
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes,
                need);
  const int nb = vp_parts(R, patch);
  const int E = static_cast<int>(C * patch * patch);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  OCPPO_VP_DISPATCH(patch, hipLaunchKernelGGL(vit_patch_ln_bwd_kernel<P>, dim3(nb),
                                              dim3(kVpThreads), 0, s, dy, src, idx, rows, R,
                                              (int)C, mean, rstd, part));
  if (int rc = check_launch(who)) return rc;
  hipLaunchKernelGGL(vit_patch_ln_finish_kernel,
                     dim3(static_cast<unsigned>(ceil_div(2 * E, kVpThreads))), dim3(kVpThreads), 0,
                     s, part, nb, E, dgamma, dbeta);
  return check_launch("ocppo_vit_patch_ln_bwd (finish)");
}
#undef OCPPO_VP_DISPATCH
