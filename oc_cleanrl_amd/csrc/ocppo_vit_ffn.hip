// The feed-forward half of a SimpleViT block (cleanrl/ppo_atari_vit.py through vit_pytorch:
// FeedForward = LayerNorm -> Linear -> GELU -> Linear, plus the block's residual add) as ONE launch
// forward and one (+ a finish) backward, on v_mfma_f32_16x16x4_f32:
//   y = x + W2 gelu(W1 u + b1) + b2,  u = LN(x)        x, y [rows, D]; W1 [H, D]; W2 [D, H]
// D and H are multiples of 32 in [32, 128] (template parameters). All f32 (exact f32 products, f32
// accumulation), exact GELU (erff), no atomics, every sum in an order fixed by (rows, D, H): two
// runs are bitwise equal.
//
// Work split: workgroups (256 threads forward, 512 backward) walk 64-row tiles (tile = blockIdx + k gridDim). In every
// product of an activation tile with a weight, wave w owns the OUTPUT COLUMN tiles n = w and w + 4
// (forward; n = w alone in the backward; 16 columns each; those < N / 16 exist) for all four 16-row tiles, so its B operand is a slice of
// the weight that it keeps in registers across the tiles (2 x K / 16 float4 per lane: 64 VGPRs per
// matrix at 128 x 128) and the A operand is the activation tile in LDS. The weights never sit in
// LDS: two of them at a padded stride plus one tile would not fit the CU's 160 KB. The forward
// holds both slices for the life of the workgroup; the backward, whose registers go to the
// weight-gradient accumulators, reads a slice from global memory (L2) before the product that
// uses it: 16 to 64 loads per lane against 256 MFMAs.
//
// LDS tiles are 64 rows at a row stride of width + 4 floats. The A operand is read in
// ocppo_vit_attn.hip's row form (lane (r = lane & 15, g = lane >> 4) reads the float4
// T[16 m + r][16 t + 4 g ..]; k-step c of chunk t contracts the columns 16 t + 4 g + c, and the B
// registers hold the weight under the same assignment), conflict-free at a stride that is 4 mod 32.
// The accumulator of a 16 x 16 tile holds D[4 g + i][r] in component i.
//
// LayerNorm: wave w normalises rows 16 w .. 16 w + 15 of the tile straight from global memory, a
// row at a time with lane l on columns l and l + 64: mean, re-centre once, variance = mean of the
// squared deviations, rstd = 1 / sqrt(var + eps) (ocppo_ln_relu_fwd's scheme; the divisions by D
// are true divisions, so a constant row has deviation exactly 0 and u == beta bitwise).
//
// Forward (tiles u [64 x D], h [64 x H]: 67,584 B at 128 x 128): u -> z = u W1^T + b1 in
// registers -> h = gelu(z) to LDS -> y = h W2^T + b2 + x stored from the accumulators.
//
// Backward (tiles x^, u, dy [64 x D] and dz [64 x H]: 135,168 B) recomputes u, z, h per tile:
//   z (as the forward) -> h and gelu'(z) in the accumulator layout, which IS the column form of an
//   MFMA operand over the tile's rows: dW2 += dy^T h takes h from the registers it was made in;
//   dh = dy W2 (W2's column slice) -> dz = dh gelu'(z) in place -> db1's tile sum ->
//   dW1 += dz^T u, again from registers; dz to LDS; du = dz W1 (W1's column slice);
//   du over the dead u tile; then per row dx = dy + rstd ((g - mean g) - x^ mean(g x^)), g = du gamma.
// The backward runs 512 threads, wave w owning column tile w alone, so dW1 / dW2 stay in 2 x 32
// accumulator VGPRs per lane across all the tiles of the workgroup. The four column
// sums (db1, db2, dgamma, dbeta) are two-level: a balanced tree over the rows of a tile in f32 (a sum
// of identical rows is exact), then f64 over the workgroup's tiles. Each workgroup stores one
// partial (dW1, dW2 f32; column sums f64, db2 / dgamma / dbeta per wave) with plain stores;
// min(tiles, 128) workgroups -- a function of rows alone -- and a finish launch adds the partials in
// workgroup (then wave) order in f64.
#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kFfThreads = 256;     // forward: 4 waves, two column tiles each
constexpr int kFfBwdThreads = 512;  // backward: 8 waves, one column tile each
constexpr int kFfBwdWaves = kFfBwdThreads / 64;
constexpr int kFfRows = 64;        // rows per tile
constexpr int kFfMaxParts = 128;   // workgroups of the backward = partials the finish adds
constexpr int kFfMaxFwdGrid = 512;
constexpr float kFfInvSqrt2 = 0.70710678118654752440f;
constexpr float kFfInvSqrt2Pi = 0.39894228040143267794f;

typedef float ff_x4 __attribute__((ext_vector_type(4)));

// h = gelu(z) = 0.5 z (1 + erf(z / sqrt 2)) and gelu'(z) = Phi(z) + z phi(z) from one erff; z^2
// overflowing gives exp(-inf) = 0, never inf * 0
__device__ __forceinline__ float ff_gelu(float z, float* dg) {
  const float e = 1.0f + erff(z * kFfInvSqrt2);
  if (dg) *dg = 0.5f * e + z * (expf(-0.5f * (z * z)) * kFfInvSqrt2Pi);
  return (0.5f * z) * e;
}

// Everything is unrolled, and left alone the scheduler lifts a whole product's LDS reads ahead
// of its MFMAs, and interleaves the erff / expf expansions of all of a wave's elements: hundreds
// of live VGPRs, and scratch. A fence per k-chunk and per element keeps that bounded.
__device__ __forceinline__ void ff_fence() { __builtin_amdgcn_sched_barrier(0); }

template <int NJ>
__device__ __forceinline__ void ff_zero(ff_x4 (&a)[4][NJ]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int j = 0; j < NJ; ++j) a[m][j] = ff_x4{0.f, 0.f, 0.f, 0.f};
}

// B slice of a product a W^T (output columns = W's rows): W [16 NT, 16 KT], rows 16 n + r
template <int KT, int NT, int NJ>
__device__ __forceinline__ void ff_load_rows(ff_x4 (&b)[NJ][KT], const float* __restrict__ W, int w,
                                             int r, int g) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = w + (8 / NJ) * j;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      b[j][t] = ff_x4{0.f, 0.f, 0.f, 0.f};
      if (n < NT) {
        const float4 v = *reinterpret_cast<const float4*>(W + (16 * n + r) * (16 * KT) + 16 * t + 4 * g);
        b[j][t] = ff_x4{v.x, v.y, v.z, v.w};
      }
    }
  }
}

// B slice of a product a W (output columns = W's columns): W [16 KT, 16 NT], columns 16 n + r
template <int KT, int NT, int NJ>
__device__ __forceinline__ void ff_load_cols(ff_x4 (&b)[NJ][KT], const float* __restrict__ W, int w,
                                             int r, int g) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = w + (8 / NJ) * j;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      b[j][t] = ff_x4{0.f, 0.f, 0.f, 0.f};
      if (n < NT) {
        const float* p = W + (16 * t + 4 * g) * (16 * NT) + 16 * n + r;
        b[j][t] = ff_x4{p[0], p[16 * NT], p[2 * 16 * NT], p[3 * 16 * NT]};
      }
    }
  }
}

// acc[m][j] += tile rows 16 m .. (row form, stride 16 KT + 4) times the wave's B slice
template <int KT, int NT, int NJ>
__device__ __forceinline__ void ff_prod(ff_x4 (&acc)[4][NJ], const float* tile,
                                        const ff_x4 (&b)[NJ][KT], int w, int r, int g) {
  constexpr int LD = 16 * KT + 4;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 a = *reinterpret_cast<const float4*>(tile + (16 * m + r) * LD + 16 * t + 4 * g);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (w + (8 / NJ) * j < NT) {
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[j][t][0], acc[m][j], 0, 0, 0);
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[j][t][1], acc[m][j], 0, 0, 0);
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[j][t][2], acc[m][j], 0, 0, 0);
          acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[j][t][3], acc[m][j], 0, 0, 0);
        }
      }
    }
    ff_fence();
  }
}

// the wave's accumulator columns -> a tile of row stride LD (banks 16 g + 4 i + r: 64 distinct)
template <int LD, int NT, int NJ>
__device__ __forceinline__ void ff_put(float* tile, const ff_x4 (&v)[4][NJ], int w, int r, int g) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = w + (8 / NJ) * j;
    if (n < NT) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(16 * m + 4 * g + i) * LD + 16 * n + r] = v[m][j][i];
    }
  }
}

// ((a0 + a1) + (a2 + a3)): the balanced tree of the column sums
__device__ __forceinline__ float ff_tree4(float a0, float a1, float a2, float a3) {
  return (a0 + a1) + (a2 + a3);
}

template <int D, int H>
__global__ __launch_bounds__(kFfThreads) void vit_ffn_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, int64_t rows, float eps, float* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd) {
  constexpr int DT = D / 16, HT = H / 16, LDD = D + 4, LDH = H + 4;
  extern __shared__ float4 s_ff4[];
  float* s_u = reinterpret_cast<float*>(s_ff4);
  float* s_h = s_u + kFfRows * LDD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  ff_x4 w1[2][DT], w2[2][HT];
  ff_load_rows<DT, HT, 2>(w1, W1, w, r, g);
  ff_load_rows<HT, DT, 2>(w2, W2, w, r, g);
  float bz[2], by[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = w + 4 * j;
    bz[j] = n < HT ? b1[16 * n + r] : 0.f;
    by[j] = n < DT ? b2[16 * n + r] : 0.f;
  }
  const bool in0 = lane < D, in1 = lane + 64 < D;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float e0 = in0 ? beta[lane] : 0.f, e1 = in1 ? beta[lane + 64] : 0.f;
  const float fd = static_cast<float>(D);
  const int64_t tiles = (rows + kFfRows - 1) / kFfRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kFfRows;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int lr = 16 * w + i;
      const int64_t row = row0 + lr;
      const bool real = row < rows;
      float d0 = real && in0 ? x[row * D + lane] : 0.f;
      float d1 = real && in1 ? x[row * D + lane + 64] : 0.f;
      const float mu0 = wave_sum(d0 + d1) / fd;
      d0 = in0 ? d0 - mu0 : 0.f;
      d1 = in1 ? d1 - mu0 : 0.f;
      const float c = wave_sum(d0 + d1) / fd;
      d0 = in0 ? d0 - c : 0.f;
      d1 = in1 ? d1 - c : 0.f;
      const float rs = 1.0f / sqrtf(wave_sum(d0 * d0 + d1 * d1) / fd + eps);
      if (in0) s_u[lr * LDD + lane] = real ? (d0 * rs) * g0 + e0 : 0.f;
      if (in1) s_u[lr * LDD + lane + 64] = real ? (d1 * rs) * g1 + e1 : 0.f;
      if (mean && real && lane == 0) {
        mean[row] = mu0 + c;
        rstd[row] = rs;
      }
    }
    __syncthreads();  // u is whole; every wave is through with the previous tile's h
    ff_x4 acc[4][2];
    ff_zero(acc);
    ff_prod<DT, HT, 2>(acc, s_u, w1, w, r, g);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[m][j][i] = ff_gelu(acc[m][j][i] + bz[j], nullptr);
          ff_fence();
        }
    ff_put<LDH, HT, 2>(s_h, acc, w, r, g);
    __syncthreads();  // h is whole; every wave is through with u
    ff_zero(acc);
    ff_prod<HT, DT, 2>(acc, s_h, w2, w, r, g);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = w + 4 * j;
      if (n < DT) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int64_t row = row0 + 16 * m + 4 * g + i;
            if (row < rows) {
              const int64_t o = row * D + 16 * n + r;
              y[o] = (acc[m][j][i] + by[j]) + x[o];
            }
          }
      }
    }
  }
}

// byte offsets inside one workgroup's partial: dW1 [H D] f32, dW2 [D H] f32, then f64: db1 [H],
// and per wave w of 8 (db2, dgamma, dbeta) [3][D] at H + 3 D w
__host__ __device__ inline size_t ff_part_bytes(int64_t D, int64_t H) {
  return static_cast<size_t>(2 * D * H) * sizeof(float) +
         static_cast<size_t>(H + 3 * kFfBwdWaves * D) * sizeof(double);
}

template <int D, int H>
__global__ __launch_bounds__(kFfBwdThreads) void vit_ffn_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, int64_t rows, float* __restrict__ dx,
    unsigned char* __restrict__ part) {
  constexpr int DT = D / 16, HT = H / 16, LDD = D + 4, LDH = H + 4;
  constexpr int RW = kFfRows / kFfBwdWaves;  // rows of a tile per wave in the row passes
  extern __shared__ float4 s_ff4[];
  float* s_xh = reinterpret_cast<float*>(s_ff4);  // x^
  float* s_u = s_xh + kFfRows * LDD;              // u, then du
  float* s_dy = s_u + kFfRows * LDD;
  float* s_dz = s_dy + kFfRows * LDD;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  ff_x4 gw1[DT], gw2[DT];  // dW1 rows 16 w .., dW2 columns 16 w .. (w < HT)
#pragma unroll
  for (int m = 0; m < DT; ++m) gw1[m] = gw2[m] = ff_x4{0.f, 0.f, 0.f, 0.f};
  const float bz = w < HT ? b1[16 * w + r] : 0.f;
  const bool in0 = lane < D, in1 = lane + 64 < D;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float e0 = in0 ? beta[lane] : 0.f, e1 = in1 ? beta[lane + 64] : 0.f;
  const float fd = static_cast<float>(D);
  double sb1 = 0.0;  // db1 of column 16 w + r (every g holds it)
  double sb2[2] = {0.0, 0.0}, sg[2] = {0.0, 0.0}, sb[2] = {0.0, 0.0};  // columns lane, lane + 64
  const int64_t tiles = (rows + kFfRows - 1) / kFfRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * kFfRows;
    // The weight slices are this tile's transients: opaque copies of the pointers keep their loads
    // from being lifted out of the tile loop, where 96 VGPRs of them would sit beside the
    // accumulators for good.
    const float* W1t = W1;
    const float* W2t = W2;
    asm volatile("" : "+s"(W1t), "+s"(W2t));
    __syncthreads();  // every wave is through with the previous tile's du, x^ and dy
#pragma unroll 4
    for (int i = 0; i < RW; ++i) {
      const int lr = RW * w + i;
      const int64_t row = row0 + lr;
      const bool real = row < rows;
      const float mu = real ? mean[row] : 0.f, rs = real ? rstd[row] : 0.f;
      float d0 = real && in0 ? x[row * D + lane] - mu : 0.f;
      float d1 = real && in1 ? x[row * D + lane + 64] - mu : 0.f;
      const float c = wave_sum(d0 + d1) / fd;
      d0 = in0 ? (d0 - c) * rs : 0.f;
      d1 = in1 ? (d1 - c) * rs : 0.f;
      if (in0) {
        s_xh[lr * LDD + lane] = d0;
        s_u[lr * LDD + lane] = real ? d0 * g0 + e0 : 0.f;
        s_dy[lr * LDD + lane] = real ? dy[row * D + lane] : 0.f;
      }
      if (in1) {
        s_xh[lr * LDD + lane + 64] = d1;
        s_u[lr * LDD + lane + 64] = real ? d1 * g1 + e1 : 0.f;
        s_dy[lr * LDD + lane + 64] = real ? dy[row * D + lane + 64] : 0.f;
      }
    }
    __syncthreads();

    ff_x4 hz[4][1], dz[4][1];
    ff_zero(hz);
    {
      ff_x4 w1[1][DT];
      ff_load_rows<DT, HT, 1>(w1, W1t, w, r, g);  // z = u W1^T
      ff_prod<DT, HT, 1>(hz, s_u, w1, w, r, g);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float dg;
        hz[m][0][i] = ff_gelu(hz[m][0][i] + bz, &dg);
        dz[m][0][i] = dg;
        ff_fence();
      }
    // dW2[16 m + .][16 w + .] += dy^T h: A = dy^T in column form from LDS, B = h as it stands
    if (w < HT) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* ap = s_dy + (16 * t + 4 * g + c) * LDD + r;
#pragma unroll
          for (int m = 0; m < DT; ++m)
            gw2[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * m], hz[t][0][c], gw2[m], 0, 0, 0);
          ff_fence();
        }
    }
    ff_zero(hz);  // h is used up; hz takes dh
    {
      ff_x4 w2c[1][DT];
      ff_load_cols<DT, HT, 1>(w2c, W2t, w, r, g);  // dh = dy W2
      ff_prod<DT, HT, 1>(hz, s_dy, w2c, w, r, g);
    }
    {
      float s4[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dz[m][0][i] *= hz[m][0][i];
        s4[m] = ff_tree4(dz[m][0][0], dz[m][0][1], dz[m][0][2], dz[m][0][3]);
      }
      float s = ff_tree4(s4[0], s4[1], s4[2], s4[3]);  // rows 4 g + i of the four row tiles
      s += __shfl_xor(s, 16, kWave);
      s += __shfl_xor(s, 32, kWave);
      sb1 += static_cast<double>(s);
    }
    ff_put<LDH, HT, 1>(s_dz, dz, w, r, g);
    // dW1[16 w + .][16 m + .] += dz^T u: A = dz as it stands, B = u in column form from LDS
    if (w < HT) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* bp = s_u + (16 * t + 4 * g + c) * LDD + r;
#pragma unroll
          for (int m = 0; m < DT; ++m)
            gw1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[t][0][c], bp[16 * m], gw1[m], 0, 0, 0);
          ff_fence();
        }
    }
    __syncthreads();  // dz is whole; every wave is through with u
    {
      ff_x4 w1c[1][HT];
      ff_load_cols<HT, DT, 1>(w1c, W1t, w, r, g);  // du = dz W1
      ff_zero(hz);
      ff_prod<HT, DT, 1>(hz, s_dz, w1c, w, r, g);
    }
    ff_put<LDD, DT, 1>(s_u, hz, w, r, g);
    __syncthreads();  // du is whole

    float tb2[2][RW / 4], tg[2][RW / 4], tb[2][RW / 4];
#pragma unroll
    for (int q = 0; q < RW / 4; ++q) {
      float vb2[2][4], vg[2][4], vb[2][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int lr = RW * w + 4 * q + p;
        const int64_t row = row0 + lr;
        const bool real = row < rows;
        const float rs = real ? rstd[row] : 0.f;
        const float u0 = in0 ? s_u[lr * LDD + lane] : 0.f, u1 = in1 ? s_u[lr * LDD + lane + 64] : 0.f;
        const float h0 = in0 ? s_xh[lr * LDD + lane] : 0.f, h1 = in1 ? s_xh[lr * LDD + lane + 64] : 0.f;
        const float y0 = in0 ? s_dy[lr * LDD + lane] : 0.f, y1 = in1 ? s_dy[lr * LDD + lane + 64] : 0.f;
        const float a0 = u0 * g0, a1 = u1 * g1;
        const float c1 = wave_sum(a0 + a1) / fd;
        const float c2 = wave_sum(a0 * h0 + a1 * h1) / fd;
        if (real && in0) dx[row * D + lane] = y0 + rs * ((a0 - c1) - h0 * c2);
        if (real && in1) dx[row * D + lane + 64] = y1 + rs * ((a1 - c1) - h1 * c2);
        vb2[0][p] = y0, vb2[1][p] = y1;
        vg[0][p] = u0 * h0, vg[1][p] = u1 * h1;
        vb[0][p] = u0, vb[1][p] = u1;
      }
      ff_fence();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        tb2[k][q] = ff_tree4(vb2[k][0], vb2[k][1], vb2[k][2], vb2[k][3]);
        tg[k][q] = ff_tree4(vg[k][0], vg[k][1], vg[k][2], vg[k][3]);
        tb[k][q] = ff_tree4(vb[k][0], vb[k][1], vb[k][2], vb[k][3]);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      static_assert(RW == 8, "the tile sum of a wave's rows is a tree over two groups of four");
      sb2[k] += static_cast<double>(tb2[k][0] + tb2[k][1]);
      sg[k] += static_cast<double>(tg[k][0] + tg[k][1]);
      sb[k] += static_cast<double>(tb[k][0] + tb[k][1]);
    }
  }

  unsigned char* mine = part + static_cast<size_t>(blockIdx.x) * ff_part_bytes(D, H);
  float* p1 = reinterpret_cast<float*>(mine);
  float* p2 = p1 + D * H;
  double* cs = reinterpret_cast<double*>(p2 + D * H);
  if (w < HT) {
#pragma unroll
    for (int m = 0; m < DT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p1[(16 * w + 4 * g + i) * D + 16 * m + r] = gw1[m][i];
        p2[(16 * m + 4 * g + i) * H + 16 * w + r] = gw2[m][i];
      }
    if (g == 0) cs[16 * w + r] = sb1;
  }
  double* cw = cs + H + 3 * D * w;
  if (in0) cw[lane] = sb2[0], cw[D + lane] = sg[0], cw[2 * D + lane] = sb[0];
  if (in1) cw[lane + 64] = sb2[1], cw[D + lane + 64] = sg[1], cw[2 * D + lane + 64] = sb[1];
}

// one output element per thread: the nwg partials in workgroup (then wave) order, in f64
__global__ __launch_bounds__(kFfThreads) void vit_ffn_finish_kernel(
    const unsigned char* __restrict__ part, int nwg, int D, int H, float* __restrict__ dW1,
    float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int t = blockIdx.x * kFfThreads + threadIdx.x;
  const int HD = H * D;
  if (t >= 2 * HD + H + 3 * D) return;
  const size_t stride = ff_part_bytes(D, H);
  double a = 0.0;
  if (t < 2 * HD) {
    for (int p = 0; p < nwg; ++p)
      a += static_cast<double>(reinterpret_cast<const float*>(part + p * stride)[t]);
    (t < HD ? dW1 : dW2)[t < HD ? t : t - HD] = static_cast<float>(a);
    return;
  }
  const int c = t - 2 * HD;
  const size_t cs0 = static_cast<size_t>(2 * HD) * sizeof(float);
  if (c < H) {
    for (int p = 0; p < nwg; ++p)
      a += reinterpret_cast<const double*>(part + p * stride + cs0)[c];
    db1[c] = static_cast<float>(a);
    return;
  }
  const int k = (c - H) / D, e = (c - H) % D;  // k: 0 db2, 1 dgamma, 2 dbeta
  for (int p = 0; p < nwg; ++p)
    for (int w = 0; w < kFfBwdWaves; ++w)
      a += reinterpret_cast<const double*>(part + p * stride + cs0)[H + (3 * w + k) * D + e];
  (k == 0 ? db2 : k == 1 ? dgamma : dbeta)[e] = static_cast<float>(a);
}

inline bool ff_dim_ok(int64_t v) { return v >= 32 && v <= 128 && v % 32 == 0; }
inline bool ff_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int ff_check(const char* who, int64_t rows, int64_t D, int64_t H) {
  OCPPO_REQUIRE(rows >= 0 && rows < (int64_t(1) << 40) && ff_dim_ok(D) && ff_dim_ok(H),
                "%s: bad sizes rows=%lld D=%lld H=%lld (D and H multiples of 32 in [32, 128])", who,
                (long long)rows, (long long)D, (long long)H);
  return OCPPO_OK;
}

inline int ff_parts(int64_t rows) {
  const int64_t tiles = ceil_div(rows, kFfRows);
  return static_cast<int>(tiles < kFfMaxParts ? (tiles > 0 ? tiles : 1) : kFfMaxParts);
}

// More than 64 KB of dynamic LDS (the CU has 160 KB) is asked for per kernel, before its launch
template <class K>
inline void ff_allow_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

template <int D, int H>
static void ff_launch_fwd(dim3 grid, hipStream_t s, const float* x, const float* gamma,
                          const float* beta, const float* W1, const float* b1, const float* W2,
                          const float* b2, int64_t rows, float eps, float* y, float* mean,
                          float* rstd) {
  const size_t lds = static_cast<size_t>(kFfRows) * (D + 4 + H + 4) * sizeof(float);
  ff_allow_lds(vit_ffn_fwd_kernel<D, H>, lds);
  hipLaunchKernelGGL((vit_ffn_fwd_kernel<D, H>), grid, dim3(kFfThreads), lds, s, x, gamma, beta,
                     W1, b1, W2, b2, rows, eps, y, mean, rstd);
}

template <int D, int H>
static void ff_launch_bwd(dim3 grid, hipStream_t s, const float* dy, const float* x,
                          const float* mean, const float* rstd, const float* gamma,
                          const float* beta, const float* W1, const float* b1, const float* W2,
                          int64_t rows, float* dx, unsigned char* part) {
  const size_t lds = static_cast<size_t>(kFfRows) * (3 * (D + 4) + H + 4) * sizeof(float);
  ff_allow_lds(vit_ffn_bwd_kernel<D, H>, lds);
  hipLaunchKernelGGL((vit_ffn_bwd_kernel<D, H>), grid, dim3(kFfBwdThreads), lds, s, dy, x, mean, rstd,
                     gamma, beta, W1, b1, W2, rows, dx, part);
}

}  // namespace ocppo

using namespace ocppo;

#define OCPPO_FF_CASE(DV, HV, FN, ...) \
  case (DV / 32) * 8 + HV / 32: FN<DV, HV>(__VA_ARGS__); break;
#define OCPPO_FF_ROW(DV, FN, ...)                                           \
  OCPPO_FF_CASE(DV, 32, FN, __VA_ARGS__) OCPPO_FF_CASE(DV, 64, FN, __VA_ARGS__) \
  OCPPO_FF_CASE(DV, 96, FN, __VA_ARGS__) OCPPO_FF_CASE(DV, 128, FN, __VA_ARGS__)
#define OCPPO_FF_DISPATCH(DV, HV, FN, ...)                                  \
  switch ((DV / 32) * 8 + HV / 32) {                                        \
    OCPPO_FF_ROW(32, FN, __VA_ARGS__) OCPPO_FF_ROW(64, FN, __VA_ARGS__)     \
    OCPPO_FF_ROW(96, FN, __VA_ARGS__) OCPPO_FF_ROW(128, FN, __VA_ARGS__)    \
  }

extern "C" int ocppo_vit_ffn_fwd(ocppo_stream_t stream, const float* x, const float* gamma,
                                 const float* beta, const float* W1, const float* b1,
                                 const float* W2, const float* b2, int64_t rows, int64_t D,
                                 int64_t H, double eps, float* y, float* mean, float* rstd) {
  const char* who = "ocppo_vit_ffn_fwd";
  if (int rc = ff_check(who, rows, D, H)) return rc;
  if (rows == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && gamma && beta && W1 && b1 && W2 && b2 && y, "%s: null pointer", who);
  OCPPO_REQUIRE((mean == nullptr) == (rstd == nullptr), "%s: mean and rstd go together", who);
  OCPPO_REQUIRE(ff_aligned16(W1) && ff_aligned16(W2), "%s: W1 / W2 not 16-B aligned", who);
  const int64_t tiles = ceil_div(rows, kFfRows);
  const dim3 grid(static_cast<unsigned>(tiles < kFfMaxFwdGrid ? tiles : kFfMaxFwdGrid));
  clear_stale_error();
  OCPPO_FF_DISPATCH(D, H, ff_launch_fwd, grid, as_stream(stream), x, gamma, beta, W1, b1, W2, b2,
                    rows, static_cast<float>(eps), y, mean, rstd);
  return check_launch(who);
}

extern "C" size_t ocppo_vit_ffn_workspace_bytes(int64_t rows, int64_t D, int64_t H) {
  if (rows < 0 || !ff_dim_ok(D) || !ff_dim_ok(H)) return 0;
  return static_cast<size_t>(ff_parts(rows)) * ff_part_bytes(D, H);
}

extern "C" int ocppo_vit_ffn_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                 const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, const float* W1, const float* b1,
                                 const float* W2, int64_t rows, int64_t D, int64_t H, float* dx,
                                 float* dgamma, float* dbeta, float* dW1, float* db1, float* dW2,
                                 float* db2, void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_vit_ffn_bwd";
  if (int rc = ff_check(who, rows, D, H)) return rc;
  if (rows == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dy && x && mean && rstd && gamma && beta && W1 && b1 && W2 && dx && dgamma &&
                    dbeta && dW1 && db1 && dW2 && db2,
                "%s: null pointer", who);
  OCPPO_REQUIRE(ff_aligned16(W1) && ff_aligned16(W2), "%s: W1 / W2 not 16-B aligned", who);
  const size_t need = ocppo_vit_ffn_workspace_bytes(rows, D, H);
  if (!workspace || workspace_bytes < need)
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes,
                need);
  OCPPO_REQUIRE(ff_aligned16(workspace), "%s: workspace not 16-B aligned", who);
  const int nwg = ff_parts(rows);
  unsigned char* part = static_cast<unsigned char*>(workspace);
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  OCPPO_FF_DISPATCH(D, H, ff_launch_bwd, dim3(nwg), s, dy, x, mean, rstd, gamma, beta, W1, b1, W2,
                    rows, dx, part);
  if (int rc = check_launch(who)) return rc;
  const int outs = static_cast<int>(2 * D * H + H + 3 * D);
  hipLaunchKernelGGL(vit_ffn_finish_kernel, dim3(static_cast<unsigned>(ceil_div(outs, kFfThreads))),
                     dim3(kFfThreads), 0, s, part, nwg, (int)D, (int)H, dW1, db1, dW2, db2, dgamma,
                     dbeta);
  return check_launch("ocppo_vit_ffn_bwd (finish)");
}
#undef OCPPO_FF_DISPATCH
#undef OCPPO_FF_ROW
#undef OCPPO_FF_CASE
