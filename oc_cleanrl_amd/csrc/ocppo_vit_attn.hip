// Unmasked multi-head attention at the pixel ViT's shape (cleanrl/ppo_atari_vit.py: SimpleViT,
// S = 49 patch tokens, 8 heads of dh = 64) on v_mfma_f32_16x16x4_f32, with its backward.
//
// csrc/ocppo_attn.hip keeps a query row per lane on the scalar FMA path, which suits S = 6..32
// objects at dh = 16. Here a head's score tile is 64 x 64 (77 % full at S = 49) and each of the
// five products of forward + backward is a 64 x 64 x 64 GEMM, so the head goes to the matrix core.
//
// Work split: one 256-thread workgroup per (sample, head); wave w owns rows 16 w .. 16 w + 15 of
// every product it makes. All f32 (exact f32 products, f32 accumulation), no atomics, every sum
// in an order fixed by the shapes: two runs are bitwise equal.
//
// LDS: 64 x 64 tiles of row stride kLd = 68 floats, rows S .. 63 zero-filled, staged with 16-byte
// accesses. An MFMA operand is read in one of two forms, both conflict-free at stride 68:
//   row form (A = T, or B = T^T: contraction along a tile row): lane (r = lane & 15, g = lane >> 4)
//     reads the float4 T[16 m + r][16 t + 4 g ..]; the four k-steps of chunk t take its four
//     components, i.e. k-step c of chunk t contracts the columns {16 t + 4 g + c}. Both operands
//     of a product use the same assignment, so the product is the plain one with the terms of a
//     sum taken in that fixed order. Banks: 68 r + 4 g covers 4 r + 4 g + 64 n, 16 distinct
//     16-byte slots per quarter wave.
//   column form (A = T^T, or B = T: contraction down a tile column): the scalars
//     T[16 t + 4 g + c][16 m + r], banks 16 g + r + const: 64 distinct.
// The accumulator of a 16 x 16 tile holds D[4 g + i][r] in component i.
//
// Forward: tiles Q, K, V (51 KB, three workgroups per CU). scores = Q K^T in four accumulators
// per wave; padded key columns are set to -inf BEFORE the row maximum (a zero-filled K row alone
// would give score 0, not weight 0); the row maximum and sum run over the in-lane tiles and then
// over the 16 lanes of a quarter wave by butterfly. The normalised P goes to the wave's own Q
// rows (dead once its scores exist; no other wave reads them) to become the A operand of P V.
//
// Backward: tiles Q, K, V, dO (68 KB, two workgroups per CU). P is recomputed from qkv and lse by
// the forward's own product (same operands, same order), dP = dO V^T beside it; P and
// dS = P (dP - D) stay in registers. V is dead then: P is written over it for dV = P^T dO, then
// dS over it for dQ = dS K and dK = dS^T Q. D_i = dO_i . O_i: four lanes per row, butterfly.
// Padded rows and columns of P and dS are exactly 0, so they add nothing to dK / dV.
#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kVaThreads = 256;
constexpr int kVaMaxS = 64;
constexpr int kVaLd = kVaMaxS + 4;          // row stride of every tile, floats
constexpr int kVaTile = kVaMaxS * kVaLd;    // floats per tile
constexpr int kVaMaxI = 512;

typedef float va_x4 __attribute__((ext_vector_type(4)));

// rows [0, S) x DH floats of one head at `src` (row stride `stride` floats) -> tile; rows S .. 63
// are zero-filled
template <int DH>
__device__ __forceinline__ void va_stage(float* tile, const float* __restrict__ src, int S,
                                         int64_t stride) {
  constexpr int V = DH / 4;
  for (int idx = threadIdx.x; idx < kVaMaxS * V; idx += kVaThreads) {
    const int r = idx / V, c = idx % V;
    const float4 v = r < S ? *reinterpret_cast<const float4*>(src + r * stride + 4 * c)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(tile + r * kVaLd + 4 * c) = v;
  }
}

// acc[n] += A[rows 16 w ..][.] B[rows 16 n ..][.]^T over KD contraction columns, both in row form
template <int KD>
__device__ __forceinline__ void va_row_row(va_x4 (&acc)[4], const float* a_tile,
                                           const float* b_tile, int w, int r, int g) {
#pragma unroll
  for (int t = 0; t < KD / 16; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(a_tile + (16 * w + r) * kVaLd + 16 * t + 4 * g);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float4 b = *reinterpret_cast<const float4*>(b_tile + (16 * n + r) * kVaLd + 16 * t + 4 * g);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[n], 0, 0, 0);
    }
  }
}

// acc[n] += A[rows 16 w ..][.] B[.][cols 16 n ..] over the 64 contraction indices: A in row form,
// B in column form; NT = DH / 16 output tiles
template <int NT>
__device__ __forceinline__ void va_row_col(va_x4 (&acc)[NT], const float* a_tile,
                                           const float* b_tile, int w, int r, int g) {
#pragma unroll
  for (int t = 0; t < kVaMaxS / 16; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(a_tile + (16 * w + r) * kVaLd + 16 * t + 4 * g);
    const float* bp = b_tile + (16 * t + 4 * g) * kVaLd + r;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bp[16 * n], acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bp[kVaLd + 16 * n], acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bp[2 * kVaLd + 16 * n], acc[n], 0, 0, 0);
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bp[3 * kVaLd + 16 * n], acc[n], 0, 0, 0);
    }
  }
}

// acc[n] += A[.][cols 16 w ..]^T B[.][cols 16 n ..] over the 64 contraction indices: both in
// column form
template <int NT>
__device__ __forceinline__ void va_col_col(va_x4 (&acc)[NT], const float* a_tile,
                                           const float* b_tile, int w, int r, int g) {
#pragma unroll
  for (int t = 0; t < kVaMaxS / 16; ++t) {
    const float* ap = a_tile + (16 * t + 4 * g) * kVaLd + 16 * w + r;
    const float* bp = b_tile + (16 * t + 4 * g) * kVaLd + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a = ap[c * kVaLd];
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[c * kVaLd + 16 * n], acc[n], 0, 0, 0);
    }
  }
}

// the wave's 16 x 64 accumulator rows -> rows 16 w .. of a tile
__device__ __forceinline__ void va_put(float* tile, const va_x4 (&v)[4], int w, int r, int g) {
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[(16 * w + 4 * g + i) * kVaLd + 16 * n + r] = v[n][i];
}

// rows 16 w .. of a [S, DH] head slice at dst (row stride `stride`), times mul
template <int NT>
__device__ __forceinline__ void va_store(float* __restrict__ dst, int64_t stride,
                                         const va_x4 (&v)[NT], float mul, int S, int w, int r,
                                         int g) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 16 * w + 4 * g + i;
    if (row < S) {
#pragma unroll
      for (int n = 0; n < NT; ++n) dst[row * stride + 16 * n + r] = v[n][i] * mul;
    }
  }
}

// maximum / sum over the 16 lanes of a quarter wave (the lanes that share accumulator rows)
__device__ __forceinline__ float va_max16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float va_sum16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

template <int DH>
__global__ __launch_bounds__(kVaThreads) void vit_attn_fwd_kernel(
    const float* __restrict__ qkv, int S, int I, int heads, float scale, float* __restrict__ out,
    float* __restrict__ lse) {
  extern __shared__ float4 s_va4[];
  float* s_q = reinterpret_cast<float*>(s_va4);  // Q, then the waves' P rows
  float* s_k = s_q + kVaTile;
  float* s_v = s_k + kVaTile;
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t stride = 3 * static_cast<int64_t>(I);
  const float* base = qkv + b * S * stride + h * DH;
  va_stage<DH>(s_q, base, S, stride);
  va_stage<DH>(s_k, base + I, S, stride);
  va_stage<DH>(s_v, base + 2 * I, S, stride);
  __syncthreads();

  va_x4 sc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) sc[n] = va_x4{0.f, 0.f, 0.f, 0.f};
  va_row_row<DH>(sc, s_q, s_k, w, r, g);
  float inv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float m = -INFINITY;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      sc[n][i] = 16 * n + r < S ? sc[n][i] * scale : -INFINITY;
      m = fmaxf(m, sc[n][i]);
    }
    m = va_max16(m);  // finite: key 0 is always real
    float l = 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      sc[n][i] = expf(sc[n][i] - m);  // exactly 0 at a padded key
      l += sc[n][i];
    }
    l = va_sum16(l);
    inv[i] = 1.0f / l;
    const int row = 16 * w + 4 * g + i;
    if (r == 0 && row < S) lse[(b * heads + h) * S + row] = m + logf(l);
  }
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) sc[n][i] *= inv[i];
  __syncthreads();  // this wave's Q rows are read; they take its P rows now
  va_put(s_q, sc, w, r, g);
  __syncthreads();

  constexpr int NT = DH / 16;
  va_x4 o[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = va_x4{0.f, 0.f, 0.f, 0.f};
  va_row_col<NT>(o, s_q, s_v, w, r, g);
  va_store<NT>(out + b * S * I + h * DH, I, o, 1.0f, S, w, r, g);
}

template <int DH>
__global__ __launch_bounds__(kVaThreads) void vit_attn_bwd_kernel(
    const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ lse,
    const float* __restrict__ dout, int S, int I, int heads, float scale,
    float* __restrict__ dqkv) {
  extern __shared__ float4 s_va4[];
  float* s_q = reinterpret_cast<float*>(s_va4);
  float* s_k = s_q + kVaTile;
  float* s_v = s_k + kVaTile;  // V, then P, then dS
  float* s_do = s_v + kVaTile;
  __shared__ float s_d[kVaMaxS];
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int64_t stride = 3 * static_cast<int64_t>(I);
  const float* base = qkv + b * S * stride + h * DH;
  const float* go = dout + b * S * I + h * DH;
  va_stage<DH>(s_q, base, S, stride);
  va_stage<DH>(s_k, base + I, S, stride);
  va_stage<DH>(s_v, base + 2 * I, S, stride);
  va_stage<DH>(s_do, go, S, I);
  {  // D of row 16 w + lane / 4: lane & 3 takes DH / 4 consecutive columns
    const int row = 16 * w + (lane >> 2), c0 = (lane & 3) * (DH / 4);
    float d = 0.f;
    if (row < S) {
      const float* po = out + b * S * I + h * DH + static_cast<int64_t>(row) * I + c0;
      const float* pg = go + static_cast<int64_t>(row) * I + c0;
#pragma unroll
      for (int c = 0; c < DH / 16; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(po + 4 * c);
        const float4 e = *reinterpret_cast<const float4*>(pg + 4 * c);
        d = fmaf(a.x, e.x, d);
        d = fmaf(a.y, e.y, d);
        d = fmaf(a.z, e.z, d);
        d = fmaf(a.w, e.w, d);
      }
    }
    d += __shfl_xor(d, 1, kWave);
    d += __shfl_xor(d, 2, kWave);
    if ((lane & 3) == 0) s_d[row] = d;
  }
  __syncthreads();

  va_x4 p[4], ds[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    p[n] = va_x4{0.f, 0.f, 0.f, 0.f};
    ds[n] = va_x4{0.f, 0.f, 0.f, 0.f};
  }
  va_row_row<DH>(p, s_q, s_k, w, r, g);    // the forward's scores, bit for bit
  va_row_row<DH>(ds, s_do, s_v, w, r, g);  // dP
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 16 * w + 4 * g + i;
    const float ls = row < S ? lse[(b * heads + h) * S + row] : 0.f;
    const float d = s_d[row];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const bool real = row < S && 16 * n + r < S;
      p[n][i] = real ? expf(p[n][i] * scale - ls) : 0.f;
      ds[n][i] = real ? p[n][i] * (ds[n][i] - d) : 0.f;
    }
  }
  __syncthreads();  // every wave is through with V
  va_put(s_v, p, w, r, g);
  __syncthreads();

  constexpr int NT = DH / 16;
  float* gq = dqkv + b * S * stride + h * DH;
  {
    va_x4 dv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dv[n] = va_x4{0.f, 0.f, 0.f, 0.f};
    va_col_col<NT>(dv, s_v, s_do, w, r, g);  // P^T dO
    va_store<NT>(gq + 2 * I, stride, dv, 1.0f, S, w, r, g);
  }
  __syncthreads();  // every wave is through with P
  va_put(s_v, ds, w, r, g);
  __syncthreads();
  {
    va_x4 dq[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dq[n] = va_x4{0.f, 0.f, 0.f, 0.f};
    va_row_col<NT>(dq, s_v, s_k, w, r, g);  // dS K
    va_store<NT>(gq, stride, dq, scale, S, w, r, g);
  }
  {
    va_x4 dk[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) dk[n] = va_x4{0.f, 0.f, 0.f, 0.f};
    va_col_col<NT>(dk, s_v, s_q, w, r, g);  // dS^T Q
    va_store<NT>(gq + I, stride, dk, scale, S, w, r, g);
  }
}

inline bool va_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int va_check(const char* who, int64_t B, int64_t S, int64_t I, int64_t heads) {
  OCPPO_REQUIRE(B >= 1 && S >= 1 && S <= kVaMaxS && heads >= 1 && I >= 1 && I <= kVaMaxI &&
                    I % heads == 0 && (I / heads == 32 || I / heads == 64) &&
                    B * heads < (int64_t(1) << 31),
                "%s: bad sizes B=%lld S=%lld I=%lld heads=%lld (1 <= S <= %d, I / heads in "
                "{32, 64}, I <= %d, B * heads < 2^31)",
                who, (long long)B, (long long)S, (long long)I, (long long)heads, kVaMaxS, kVaMaxI);
  return OCPPO_OK;
}

// More than 64 KB of dynamic LDS (the CU has 160 KB) is asked for per kernel, before its launch
template <class K>
inline void va_allow_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_vit_attn_fwd(ocppo_stream_t stream, const float* qkv, int64_t B, int64_t S,
                                  int64_t I, int64_t heads, float* out, float* lse) {
  const char* who = "ocppo_vit_attn_fwd";
  if (int rc = va_check(who, B, S, I, heads)) return rc;
  OCPPO_REQUIRE(qkv && out && lse, "%s: null pointer", who);
  OCPPO_REQUIRE(va_aligned16(qkv) && va_aligned16(out), "%s: qkv / out not 16-B aligned", who);
  const int dh = static_cast<int>(I / heads);
  const float scale = static_cast<float>(1.0 / sqrt(static_cast<double>(dh)));
  const size_t lds = 3 * static_cast<size_t>(kVaTile) * sizeof(float);
  const dim3 grid(static_cast<unsigned>(B * heads));
  clear_stale_error();
  if (dh == 32)
    hipLaunchKernelGGL(vit_attn_fwd_kernel<32>, grid, dim3(kVaThreads), lds, as_stream(stream),
                       qkv, (int)S, (int)I, (int)heads, scale, out, lse);
  else
    hipLaunchKernelGGL(vit_attn_fwd_kernel<64>, grid, dim3(kVaThreads), lds, as_stream(stream),
                       qkv, (int)S, (int)I, (int)heads, scale, out, lse);
  return check_launch(who);
}

extern "C" int ocppo_vit_attn_bwd(ocppo_stream_t stream, const float* qkv, const float* out,
                                  const float* lse, const float* dout, int64_t B, int64_t S,
                                  int64_t I, int64_t heads, float* dqkv) {
  const char* who = "ocppo_vit_attn_bwd";
  if (int rc = va_check(who, B, S, I, heads)) return rc;
  OCPPO_REQUIRE(qkv && out && lse && dout && dqkv, "%s: null pointer", who);
  OCPPO_REQUIRE(va_aligned16(qkv) && va_aligned16(out) && va_aligned16(dout) && va_aligned16(dqkv),
                "%s: qkv / out / dout / dqkv not 16-B aligned", who);
  const int dh = static_cast<int>(I / heads);
  const float scale = static_cast<float>(1.0 / sqrt(static_cast<double>(dh)));
  const size_t lds = 4 * static_cast<size_t>(kVaTile) * sizeof(float);
  const dim3 grid(static_cast<unsigned>(B * heads));
  clear_stale_error();
  if (dh == 32) {
    va_allow_lds(vit_attn_bwd_kernel<32>, lds);
    hipLaunchKernelGGL(vit_attn_bwd_kernel<32>, grid, dim3(kVaThreads), lds, as_stream(stream),
                       qkv, out, lse, dout, (int)S, (int)I, (int)heads, scale, dqkv);
  } else {
    va_allow_lds(vit_attn_bwd_kernel<64>, lds);
    hipLaunchKernelGGL(vit_attn_bwd_kernel<64>, grid, dim3(kVaThreads), lds, as_stream(stream),
                       qkv, out, lse, dout, (int)S, (int)I, (int)heads, scale, dqkv);
  }
  return check_launch(who);
}
