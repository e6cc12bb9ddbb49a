// The attention half of a SimpleViT block (cleanrl/ppo_atari_vit.py through vit_pytorch:
// Attention = LayerNorm -> to_qkv -> softmax attention per head -> to_out, plus the block's
// residual add) as ONE launch forward and a fused backward, on v_mfma_f32_16x16x4_f32:
//   u = LN(x);  qkv = u Wqkv^T;  O_h = softmax(q_h k_h^T / 8) v_h;  y = x + concat_h(O_h) Wout^T
// x, y [B S, D] sample-major (S <= 64 tokens per sample), Wqkv [3 I, D] (rows q | k | v, each
// head-major), Wout [D, I], I = 64 heads, no biases. D is a multiple of 32 in [32, 128] (template
// parameter); heads <= 8 and S are runtime values. All f32 (exact f32 products, f32 accumulation),
// no atomics, every sum in an order fixed by (B, S, D, heads): two runs are bitwise equal. qkv, the
// attention output and their gradients never leave the chip.
//
// Tile forms are those of ocppo_vit_attn.hip and ocppo_vit_ffn.hip, restated here: 64 x 64 tiles
// at a row stride of 68 floats and 64 x D tiles at stride D + 4, rows S .. 63 zero; an operand that
// contracts along a tile row is one float4 per lane (row form: lane (r = lane & 15, g = lane >> 4)
// reads T[16 m + r][16 t + 4 g ..], k-step c of chunk t contracts column 16 t + 4 g + c on both
// operands), one that contracts down a column is four scalars (column form:
// T[16 t + 4 g + c][16 m + r]); both are conflict-free at a stride that is 4 mod 32. A weight
// operand is a slice read from global memory (L2) into registers just before its product. The
// accumulator of a 16 x 16 tile holds D[4 g + i][r] in component i.
//
// Forward: one 256-thread workgroup per sample (grid-stride beyond 2048). LayerNorm (a wave per
// row, ocppo_ln_relu_fwd's scheme with true divisions by D: a constant row gives u == beta bitwise)
// into the u tile, which stays for all heads. Per head: q, k, v = u W^T (wave w owns output columns
// 16 w .. of all four row tiles) to three tiles; scores, softmax (padded key columns -inf before the
// row maximum) and P V as vit_attn_fwd_kernel, wave w owning rows 16 w ..: P, then O, overwrite the
// wave's own Q rows; y += O_h Wout_h^T accumulates over the heads in registers (wave w owns
// output column tiles w and w + 4). y + x is stored once. Saved: mean, rstd [B S], lse [B, heads, S].
//
// Backward: head-owning 512-thread workgroups (h, p), p < P = min(B, max(256 / heads, 1)), walk
// samples p, p + P, ...; the weight-gradient accumulators of the head (dWqkv_h [192, D] and
// dWout_h [D, 64]: 64 registers per lane at D = 128) stay in registers over all its samples. Per
// sample u, q, k, v, dO = dy Wout_h are recomputed into tiles (u by the forward's own operations,
// so the scores are the forward's bit for bit), P = exp(s - lse) divided by its own row sum (lse is
// rounded at the size of the row maximum: a saturated row would carry that as a common factor),
// dP = dO V^T beside it; the row sums of P and of P dP (= dO . O, the softmax backward's row term)
// run over the two waves that share a row, through LDS in a fixed order. O = P V (for dWout_h += dy^T O) and dV = P^T dO read P from its own
// tile; O overwrites the dead V tile, dS the P tile; dQ, dK, dV then overwrite Q, K, V to be the A
// operands of dWqkv_h += [dQ; dK; dV]^T u and du_h = dQ Wq_h + dK Wk_h + dV Wv_h, which goes to the
// head's slab of the workspace. Every __syncthreads() is reached by all 512 threads: the sample
// loop's trip count and every guarded product depend on the workgroup and the wave alone.
//
// Two finish launches: "rows" adds the heads' du slabs in head order, runs the LayerNorm backward
// and the residual (dx = dy + LN'(du)) and leaves dgamma / dbeta partials (a balanced tree over the
// 16 rows of a wave in f32, then f64 over tiles); "sum" adds the weight-gradient partials in
// workgroup order and the column partials in workgroup, then wave, order, both in f64.
#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kAbFwdThreads = 256;
constexpr int kAbBwdThreads = 512;
constexpr int kAbRows = 64;               // rows of every tile: the token limit
constexpr int kAbDh = 64;                 // head width
constexpr int kAbLd = kAbDh + 4;          // row stride of a 64 x 64 tile
constexpr int kAbTile = kAbRows * kAbLd;  // floats per 64 x 64 tile
constexpr int kAbMaxHeads = 8;
constexpr int kAbMaxFwdGrid = 2048;
constexpr int kAbPartTarget = 256;   // heads * P is about this many workgroups (the CU count)
constexpr int kAbMaxRowParts = 256;  // workgroups of the rows finish
constexpr int kAbRowWaves = kAbFwdThreads / 64;
constexpr float kAbScale = 0.125f;   // 1 / sqrt(64)

typedef float ab_x4 __attribute__((ext_vector_type(4)));

// bounds the scheduler's lifting of LDS reads ahead of the MFMAs (as ff_fence)
__device__ __forceinline__ void ab_fence() { __builtin_amdgcn_sched_barrier(0); }

template <int N>
__device__ __forceinline__ void ab_zero(ab_x4 (&a)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) a[n] = ab_x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ ab_x4 ab_mfma4(const float4 a, const ab_x4 b, ab_x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], acc, 0, 0, 0);
  return acc;
}

// B slice of a product a W^T: 16 rows of W at `rows` (row stride ld), contraction columns 16 KT
template <int KT>
__device__ __forceinline__ void ab_load_rows(ab_x4 (&b)[KT], const float* __restrict__ rows, int ld,
                                             int r, int g) {
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const float4 v = *reinterpret_cast<const float4*>(rows + r * ld + 16 * t + 4 * g);
    b[t] = ab_x4{v.x, v.y, v.z, v.w};
  }
}

// B slice of a product a W: 16 columns of W at `cols` (row stride ld), contraction rows 16 KT
template <int KT>
__device__ __forceinline__ void ab_load_cols(ab_x4 (&b)[KT], const float* __restrict__ cols, int ld,
                                             int r, int g) {
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const float* p = cols + (16 * t + 4 * g) * ld + r;
    b[t] = ab_x4{p[0], p[ld], p[2 * ld], p[3 * ld]};
  }
}

// acc[m] += rows 16 m .. of `tile` (row form, stride LD) times the B slice, m < MR
template <int KT, int MR, int LD>
__device__ __forceinline__ void ab_prod(ab_x4 (&acc)[MR], const float* tile, const ab_x4 (&b)[KT],
                                        int r, int g) {
#pragma unroll
  for (int t = 0; t < KT; ++t) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const float4 a = *reinterpret_cast<const float4*>(tile + (16 * m + r) * LD + 16 * t + 4 * g);
      acc[m] = ab_mfma4(a, b[t], acc[m]);
    }
    ab_fence();
  }
}

// acc[m] (rows 16 m .. of the tile at `dst`, whose first column is the wave's) -> LDS
template <int MR, int LD>
__device__ __forceinline__ void ab_put_rows(float* dst, const ab_x4 (&v)[MR], int r, int g) {
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(16 * m + 4 * g + i) * LD + r] = v[m][i];
}

// v[n] (columns 16 n .. of the 16 rows at `dst`) -> LDS, stride 68
template <int NT>
__device__ __forceinline__ void ab_put_cols(float* dst, const ab_x4 (&v)[NT], int r, int g) {
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[(4 * g + i) * kAbLd + 16 * n + r] = v[n][i];
}

// The three products of 64 x 64 tiles (stride 68), 64 contraction indices, NT output column tiles.
// a / b point at the wave's first row (row form) or first column (column form).
template <int NT>
__device__ __forceinline__ void ab_row_row(ab_x4 (&acc)[NT], const float* a, const float* b, int r,
                                           int g) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float4 av = *reinterpret_cast<const float4*>(a + r * kAbLd + 16 * t + 4 * g);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float4 bv = *reinterpret_cast<const float4*>(b + (16 * n + r) * kAbLd + 16 * t + 4 * g);
      acc[n] = ab_mfma4(av, ab_x4{bv.x, bv.y, bv.z, bv.w}, acc[n]);
    }
    ab_fence();
  }
}

template <int NT>
__device__ __forceinline__ void ab_row_col(ab_x4 (&acc)[NT], const float* a, const float* b, int r,
                                           int g) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float4 av = *reinterpret_cast<const float4*>(a + r * kAbLd + 16 * t + 4 * g);
    const float* bp = b + (16 * t + 4 * g) * kAbLd + r;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      acc[n] = ab_mfma4(av, ab_x4{bp[16 * n], bp[kAbLd + 16 * n], bp[2 * kAbLd + 16 * n],
                                  bp[3 * kAbLd + 16 * n]}, acc[n]);
    ab_fence();
  }
}

template <int NT>
__device__ __forceinline__ void ab_col_col(ab_x4 (&acc)[NT], const float* a, const float* b, int r,
                                           int g) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float* ap = a + (16 * t + 4 * g) * kAbLd + r;
    const float* bp = b + (16 * t + 4 * g) * kAbLd + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float av = ap[c * kAbLd];
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[c * kAbLd + 16 * n], acc[n], 0, 0, 0);
    }
    ab_fence();
  }
}

// maximum / sum over the 16 lanes that share accumulator rows
__device__ __forceinline__ float ab_max16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float ab_sum16(float v) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__device__ __forceinline__ float ab_tree4(float a0, float a1, float a2, float a3) {
  return (a0 + a1) + (a2 + a3);
}

template <int D>
__global__ __launch_bounds__(kAbFwdThreads) void vit_attn_block_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ Wqkv, const float* __restrict__ Wout, int64_t B, int S, int heads,
    float eps, float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ lse) {
  constexpr int DT = D / 16, LDD = D + 4;
  extern __shared__ float4 s_ab4[];
  float* s_u = reinterpret_cast<float*>(s_ab4);
  float* s_q = s_u + kAbRows * LDD;  // Q, then the waves' P rows, then their O rows
  float* s_k = s_q + kAbTile;
  float* s_v = s_k + kAbTile;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int I = kAbDh * heads;
  const bool in0 = lane < D, in1 = lane + 64 < D;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float e0 = in0 ? beta[lane] : 0.f, e1 = in1 ? beta[lane + 64] : 0.f;
  const float fd = static_cast<float>(D);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t row0 = b * S;
    __syncthreads();  // every wave is through with the previous sample's u
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int lr = 16 * w + i;
      const int64_t row = row0 + lr;
      const bool real = lr < S;
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
    ab_x4 ya[2][4];  // y columns 16 (w + 4 j) .., rows 16 m ..
    ab_zero(ya[0]);
    ab_zero(ya[1]);
    for (int h = 0; h < heads; ++h) {
      __syncthreads();  // u is whole; every wave is through with the previous head's tiles
#pragma unroll
      for (int sel = 0; sel < 3; ++sel) {
        ab_x4 bw[DT], acc[4];
        ab_load_rows<DT>(bw, Wqkv + (static_cast<int64_t>(sel) * I + kAbDh * h + 16 * w) * D, D, r, g);
        ab_zero(acc);
        ab_prod<DT, 4, LDD>(acc, s_u, bw, r, g);
        ab_put_rows<4, kAbLd>(s_q + sel * kAbTile + 16 * w, acc, r, g);
      }
      __syncthreads();  // Q, K, V are whole
      float* mine = s_q + 16 * w * kAbLd;  // this wave's rows: no other wave reads them until O
      ab_x4 sc[4];
      ab_zero(sc);
      ab_row_row<4>(sc, mine, s_k, r, g);
      float inv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float m = -INFINITY;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          sc[n][i] = 16 * n + r < S ? sc[n][i] * kAbScale : -INFINITY;
          m = fmaxf(m, sc[n][i]);
        }
        m = ab_max16(m);  // finite: key 0 is always real
        float l = 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          sc[n][i] = expf(sc[n][i] - m);  // exactly 0 at a padded key
          l += sc[n][i];
        }
        l = ab_sum16(l);
        inv[i] = 1.0f / l;
        const int row = 16 * w + 4 * g + i;
        if (lse && r == 0 && row < S) lse[(b * heads + h) * S + row] = m + logf(l);
      }
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[n][i] *= inv[i];
      ab_put_cols<4>(mine, sc, r, g);  // P over the wave's own Q rows
      ab_x4 o[4];
      ab_zero(o);
      ab_row_col<4>(o, mine, s_v, r, g);
      ab_put_cols<4>(mine, o, r, g);  // O over its P rows (o holds every read of them)
      __syncthreads();                // O is whole
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = w + 4 * j;
        if (n < DT) {
          ab_x4 bo[4];
          ab_load_rows<4>(bo, Wout + static_cast<int64_t>(16 * n) * I + kAbDh * h, I, r, g);
          ab_prod<4, 4, kAbLd>(ya[j], s_q, bo, r, g);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = w + 4 * j;
      if (n < DT) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int lr = 16 * m + 4 * g + i;
            if (lr < S) {
              const int64_t o = (row0 + lr) * D + 16 * n + r;
              y[o] = ya[j][m][i] + x[o];
            }
          }
      }
    }
  }
}

// floats of one backward workgroup's weight-gradient partial: dWqkv_h [3][64][D], dWout_h [D][64]
__host__ __device__ inline int64_t ab_part_floats(int64_t D) { return 4 * kAbDh * D; }

template <int D>
__global__ __launch_bounds__(kAbBwdThreads) void vit_attn_block_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ rstd,
    const float* __restrict__ lse, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ Wqkv, const float* __restrict__ Wout, int64_t B, int S, int heads,
    int P, float* __restrict__ slabs, float* __restrict__ wpart) {
  constexpr int DT = D / 16, LDD = D + 4, HN = DT / 2;
  extern __shared__ float4 s_ab4[];
  float* s_u = reinterpret_cast<float*>(s_ab4);
  float* s_dy = s_u + kAbRows * LDD;
  float* s_q = s_dy + kAbRows * LDD;  // Q, then dQ
  float* s_k = s_q + kAbTile;         // K, then dK
  float* s_v = s_k + kAbTile;         // V, then O, then dV
  float* s_do = s_v + kAbTile;
  float* s_p = s_do + kAbTile;        // P, then dS
  __shared__ float s_d[4][kAbRows];  // per column half: sum_j P dP, then sum_j P
  const int h = blockIdx.x % heads, p0 = blockIdx.x / heads;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m4 = w & 3, hf = w >> 2;  // a 16-wide tile index and a half, per product below
  const int I = kAbDh * heads;
  const int64_t R = B * S;
  const bool in0 = lane < D, in1 = lane + 64 < D;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float e0 = in0 ? beta[lane] : 0.f, e1 = in1 ? beta[lane + 64] : 0.f;
  const float fd = static_cast<float>(D);
  ab_x4 gw[3][HN], go[HN];  // dWqkv_h rows 16 m4 .. of q | k | v, dWout_h columns 16 m4 ..
  ab_zero(gw[0]);
  ab_zero(gw[1]);
  ab_zero(gw[2]);
  ab_zero(go);
  for (int64_t b = p0; b < B; b += P) {
    const int64_t row0 = b * S;
    // The weight slices are per-sample transients: opaque copies of the pointers keep their loads
    // inside the sample loop, off the registers that hold the accumulators.
    const float* Wh = Wqkv + static_cast<int64_t>(kAbDh) * h * D;  // + sel I D: the head's rows
    const float* Wo = Wout + kAbDh * h;                            // the head's columns
    asm volatile("" : "+s"(Wh), "+s"(Wo));
    // So are the lane's tile addresses: left loop-invariant they are all computed ahead of the loop
    // and held (about 100 registers, and scratch at D = 96 and 128).
    int r = lane & 15, g = lane >> 4;
    asm volatile("" : "+v"(r), "+v"(g));
    __syncthreads();  // every wave is through with the previous sample's tiles
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
      const int lr = 8 * w + i;
      const int64_t row = row0 + lr;
      const bool real = lr < S;
      // the forward's own operations in its order (first mean, re-centre, the saved rstd): u, and
      // with it q, k and the scores, come out bit for bit as the forward had them
      const float rs = real ? rstd[row] : 0.f;
      float d0 = real && in0 ? x[row * D + lane] : 0.f;
      float d1 = real && in1 ? x[row * D + lane + 64] : 0.f;
      const float mu0 = wave_sum(d0 + d1) / fd;
      d0 = in0 ? d0 - mu0 : 0.f;
      d1 = in1 ? d1 - mu0 : 0.f;
      const float c = wave_sum(d0 + d1) / fd;
      d0 = in0 ? d0 - c : 0.f;
      d1 = in1 ? d1 - c : 0.f;
      if (in0) {
        s_u[lr * LDD + lane] = real ? (d0 * rs) * g0 + e0 : 0.f;
        s_dy[lr * LDD + lane] = real ? dy[row * D + lane] : 0.f;
      }
      if (in1) {
        s_u[lr * LDD + lane + 64] = real ? (d1 * rs) * g1 + e1 : 0.f;
        s_dy[lr * LDD + lane + 64] = real ? dy[row * D + lane + 64] : 0.f;
      }
    }
    __syncthreads();  // u and dy are whole

    // q, k, v = u W^T and dO = dy Wout_h: output columns 16 m4 .., rows 32 hf .. 32 hf + 31
    {
      ab_x4 bw[DT], acc[2];
#pragma unroll
      for (int sel = 0; sel < 3; ++sel) {
        ab_load_rows<DT>(bw, Wh + (static_cast<int64_t>(sel) * I + 16 * m4) * D, D, r, g);
        ab_zero(acc);
        ab_prod<DT, 2, LDD>(acc, s_u + 32 * hf * LDD, bw, r, g);
        ab_put_rows<2, kAbLd>(s_q + sel * kAbTile + 32 * hf * kAbLd + 16 * m4, acc, r, g);
      }
      ab_load_cols<DT>(bw, Wo + 16 * m4, I, r, g);
      ab_zero(acc);
      ab_prod<DT, 2, LDD>(acc, s_dy + 32 * hf * LDD, bw, r, g);
      ab_put_rows<2, kAbLd>(s_do + 32 * hf * kAbLd + 16 * m4, acc, r, g);
    }
    __syncthreads();  // Q, K, V, dO are whole

    // the attention core: rows 16 m4 .., columns 32 hf .. 32 hf + 31 of every 64 x 64 product
    const int rt = 16 * m4 * kAbLd, ct = 32 * hf;
    ab_x4 pp[2], ds[2];
    ab_zero(pp);
    ab_zero(ds);
    ab_row_row<2>(pp, s_q + rt, s_k + ct * kAbLd, r, g);   // the forward's scores
    ab_row_row<2>(ds, s_do + rt, s_v + ct * kAbLd, r, g);  // dP
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * m4 + 4 * g + i;
      const float ls = row < S ? lse[(b * heads + h) * S + row] : 0.f;
      float part = 0.f, z = 0.f;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const bool real = row < S && ct + 16 * n + r < S;
        pp[n][i] = real ? expf(pp[n][i] * kAbScale - ls) : 0.f;
        part += pp[n][i] * ds[n][i];
        z += pp[n][i];
      }
      part = ab_sum16(part);
      z = ab_sum16(z);
      if (r == 0) s_d[hf][row] = part, s_d[2 + hf][row] = z;
    }
    __syncthreads();  // both halves of the row sums are there
    // lse = m + log l is rounded at the size of m: at a saturated head that is a factor of
    // 1 +- 1e-4 on the whole row of exp(s - lse). The row's own sum takes it out again.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * m4 + 4 * g + i;
      const float iz = row < S ? 1.0f / (s_d[2][row] + s_d[3][row]) : 0.f;
      const float d = (s_d[0][row] + s_d[1][row]) * iz;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        pp[n][i] *= iz;
        ds[n][i] = pp[n][i] * (ds[n][i] - d);  // 0 where P is 0
      }
    }
    ab_put_cols<2>(s_p + rt + ct, pp, r, g);
    __syncthreads();  // P is whole
    ab_x4 o[2], dv[2];
    ab_zero(o);
    ab_zero(dv);
    ab_row_col<2>(o, s_p + rt, s_v + ct, r, g);          // O = P V
    ab_col_col<2>(dv, s_p + 16 * m4, s_do + ct, r, g);   // dV = P^T dO
    __syncthreads();  // every wave is through with P and V
    ab_put_cols<2>(s_v + rt + ct, o, r, g);
    ab_put_cols<2>(s_p + rt + ct, ds, r, g);
    __syncthreads();  // O and dS are whole

    // dWout_h[16 (hf HN + j) + .][16 m4 + .] += dy^T O: both in column form
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 16 * t + 4 * g + c;
        const float bv = s_v[k * kAbLd + 16 * m4 + r];
#pragma unroll
        for (int j = 0; j < HN; ++j)
          go[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_dy[k * LDD + 16 * (hf * HN + j) + r], bv,
                                                       go[j], 0, 0, 0);
        ab_fence();
      }
    }
    ab_x4 dq[2], dk[2];
    ab_zero(dq);
    ab_zero(dk);
    ab_row_col<2>(dq, s_p + rt, s_k + ct, r, g);      // dQ = dS K
    ab_col_col<2>(dk, s_p + 16 * m4, s_q + ct, r, g);  // dK = dS^T Q
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dq[n][i] *= kAbScale;
        dk[n][i] *= kAbScale;
      }
    __syncthreads();  // every wave is through with Q, K, O and dS
    ab_put_cols<2>(s_q + rt + ct, dq, r, g);
    ab_put_cols<2>(s_k + rt + ct, dk, r, g);
    ab_put_cols<2>(s_v + rt + ct, dv, r, g);
    __syncthreads();  // dQ, dK, dV are whole

    // dWqkv_h[sel][16 m4 + .][16 (hf HN + j) + .] += [dQ; dK; dV]^T u: both in column form
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 16 * t + 4 * g + c;
        const float a0 = s_q[k * kAbLd + 16 * m4 + r], a1 = s_k[k * kAbLd + 16 * m4 + r],
                    a2 = s_v[k * kAbLd + 16 * m4 + r];
#pragma unroll
        for (int j = 0; j < HN; ++j) {
          const float bv = s_u[k * LDD + 16 * (hf * HN + j) + r];
          gw[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, gw[0][j], 0, 0, 0);
          gw[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, gw[1][j], 0, 0, 0);
          gw[2][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bv, gw[2][j], 0, 0, 0);
        }
        ab_fence();
      }
    }
    // du_h = dQ Wq_h + dK Wk_h + dV Wv_h: columns 16 (m4 + 4 j) .., rows 32 hf ..; to the slab
    float* slab = slabs + (static_cast<int64_t>(h) * R + row0) * D;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = m4 + 4 * j;
      if (n < DT) {
        ab_x4 acc[2];
        ab_zero(acc);
#pragma unroll
        for (int sel = 0; sel < 3; ++sel) {
          ab_x4 bc[4];
          ab_load_cols<4>(bc, Wh + static_cast<int64_t>(sel) * I * D + 16 * n, D, r, g);
          ab_prod<4, 2, kAbLd>(acc, s_q + sel * kAbTile + 32 * hf * kAbLd, bc, r, g);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int lr = 32 * hf + 16 * m + 4 * g + i;
            if (lr < S) slab[static_cast<int64_t>(lr) * D + 16 * n + r] = acc[m][i];
          }
      }
    }
  }

  const int r = lane & 15, g = lane >> 4;
  float* mine = wpart + static_cast<int64_t>(blockIdx.x) * ab_part_floats(D);
#pragma unroll
  for (int j = 0; j < HN; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = 16 * (hf * HN + j);
#pragma unroll
      for (int sel = 0; sel < 3; ++sel)
        mine[(sel * kAbDh + 16 * m4 + 4 * g + i) * D + col + r] = gw[sel][j][i];
      mine[3 * kAbDh * D + (col + 4 * g + i) * kAbDh + 16 * m4 + r] = go[j][i];
    }
}

// First finish launch. Per row: du = the heads' slabs in head order, the LayerNorm backward and the
// residual; per wave: dgamma / dbeta partials [2][D] f64 at cpart[(workgroup 4 + wave) 2 D].
__global__ __launch_bounds__(kAbFwdThreads) void vit_attn_block_rows_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ slabs, int64_t R, int D, int heads, float* __restrict__ dx,
    double* __restrict__ cpart) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool in0 = lane < D, in1 = lane + 64 < D;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float fd = static_cast<float>(D);
  double sg[2] = {0.0, 0.0}, sb[2] = {0.0, 0.0};  // columns lane, lane + 64
  const int64_t tiles = (R + kAbRows - 1) / kAbRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    float tg[2][4], tb[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float vg[2][4], vb[2][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int64_t row = tile * kAbRows + 16 * w + 4 * q + p;
        const bool real = row < R;
        const bool r0 = real && in0, r1 = real && in1;
        const float mu = real ? mean[row] : 0.f, rs = real ? rstd[row] : 0.f;
        float h0 = r0 ? x[row * D + lane] - mu : 0.f;
        float h1 = r1 ? x[row * D + lane + 64] - mu : 0.f;
        const float c = wave_sum(h0 + h1) / fd;
        h0 = r0 ? (h0 - c) * rs : 0.f;
        h1 = r1 ? (h1 - c) * rs : 0.f;
        float u0 = 0.f, u1 = 0.f;
        for (int hh = 0; hh < heads; ++hh) {
          const float* s = slabs + (static_cast<int64_t>(hh) * R + row) * D;
          u0 += r0 ? s[lane] : 0.f;
          u1 += r1 ? s[lane + 64] : 0.f;
        }
        const float a0 = u0 * g0, a1 = u1 * g1;
        const float c1 = wave_sum(a0 + a1) / fd;
        const float c2 = wave_sum(a0 * h0 + a1 * h1) / fd;
        if (r0) dx[row * D + lane] = dy[row * D + lane] + rs * ((a0 - c1) - h0 * c2);
        if (r1) dx[row * D + lane + 64] = dy[row * D + lane + 64] + rs * ((a1 - c1) - h1 * c2);
        vg[0][p] = u0 * h0, vg[1][p] = u1 * h1;
        vb[0][p] = u0, vb[1][p] = u1;
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        tg[k][q] = ab_tree4(vg[k][0], vg[k][1], vg[k][2], vg[k][3]);
        tb[k][q] = ab_tree4(vb[k][0], vb[k][1], vb[k][2], vb[k][3]);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      sg[k] += static_cast<double>(ab_tree4(tg[k][0], tg[k][1], tg[k][2], tg[k][3]));
      sb[k] += static_cast<double>(ab_tree4(tb[k][0], tb[k][1], tb[k][2], tb[k][3]));
    }
  }
  double* cw = cpart + (static_cast<int64_t>(blockIdx.x) * kAbRowWaves + w) * 2 * D;
  if (in0) cw[lane] = sg[0], cw[D + lane] = sb[0];
  if (in1) cw[lane + 64] = sg[1], cw[D + lane + 64] = sb[1];
}

// Second finish launch, one output element per thread: the P weight-gradient partials of its head
// in workgroup order, the column partials in workgroup, then wave, order; in f64.
__global__ __launch_bounds__(kAbFwdThreads) void vit_attn_block_sum_kernel(
    const float* __restrict__ wpart, const double* __restrict__ cpart, int P, int nrow, int D,
    int heads, float* __restrict__ dWqkv, float* __restrict__ dWout, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  const int t = blockIdx.x * kAbFwdThreads + threadIdx.x;
  const int I = kAbDh * heads, ID = I * D;
  if (t >= 4 * ID + 2 * D) return;
  const int64_t stride = ab_part_floats(D);
  double a = 0.0;
  if (t < 4 * ID) {
    int h, off;
    if (t < 3 * ID) {
      const int row = t / D, sel = row / I, rem = row % I;  // row of Wqkv
      h = rem / kAbDh;
      off = (sel * kAbDh + rem % kAbDh) * D + t % D;
    } else {
      const int e = t - 3 * ID, d = e / I, col = e % I;  // element [d][col] of Wout
      h = col / kAbDh;
      off = 3 * kAbDh * D + d * kAbDh + col % kAbDh;
    }
    for (int p = 0; p < P; ++p)
      a += static_cast<double>(wpart[(static_cast<int64_t>(p) * heads + h) * stride + off]);
    (t < 3 * ID ? dWqkv : dWout)[t < 3 * ID ? t : t - 3 * ID] = static_cast<float>(a);
    return;
  }
  const int c = t - 4 * ID;  // [0, D): dgamma, [D, 2 D): dbeta
  for (int q = 0; q < nrow * kAbRowWaves; ++q) a += cpart[static_cast<int64_t>(q) * 2 * D + c];
  (c < D ? dgamma : dbeta)[c < D ? c : c - D] = static_cast<float>(a);
}

inline bool ab_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool ab_sizes_ok(int64_t B, int64_t S, int64_t D, int64_t heads) {
  return B >= 0 && B < (int64_t(1) << 31) && S >= 1 && S <= kAbRows && D >= 32 && D <= 128 &&
         D % 32 == 0 && heads >= 1 && heads <= kAbMaxHeads;
}

static int ab_check(const char* who, int64_t B, int64_t S, int64_t D, int64_t heads) {
  OCPPO_REQUIRE(ab_sizes_ok(B, S, D, heads),
                "%s: bad sizes B=%lld S=%lld D=%lld heads=%lld (1 <= S <= 64, D a multiple of 32 "
                "in [32, 128], 1 <= heads <= 8)",
                who, (long long)B, (long long)S, (long long)D, (long long)heads);
  return OCPPO_OK;
}

// workgroups per head of the backward: a function of B and heads alone
inline int ab_parts(int64_t B, int64_t heads) {
  const int64_t cap = kAbPartTarget / heads;
  return static_cast<int>(B < cap ? (B > 0 ? B : 1) : cap);
}

inline int ab_row_parts(int64_t R) {
  const int64_t tiles = ceil_div(R, kAbRows);
  return static_cast<int>(tiles < kAbMaxRowParts ? (tiles > 0 ? tiles : 1) : kAbMaxRowParts);
}

// workspace: the du slabs [heads, B S, D] f32, the weight partials [P heads][256 D] f32, the column
// partials [row workgroups][4][2][D] f64
inline size_t ab_slab_bytes(int64_t B, int64_t S, int64_t D, int64_t heads) {
  return static_cast<size_t>(heads * B * S * D) * sizeof(float);
}
inline size_t ab_wpart_bytes(int64_t B, int64_t D, int64_t heads) {
  return static_cast<size_t>(ab_parts(B, heads) * heads * ab_part_floats(D)) * sizeof(float);
}

// More than 64 KB of dynamic LDS (the CU has 160 KB) is asked for per kernel, before its launch
template <class K>
inline void ab_allow_lds(K kernel, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

template <int D>
static void ab_launch_fwd(dim3 grid, hipStream_t s, const float* x, const float* gamma,
                          const float* beta, const float* Wqkv, const float* Wout, int64_t B, int S,
                          int heads, float eps, float* y, float* mean, float* rstd, float* lse) {
  const size_t lds = (static_cast<size_t>(kAbRows) * (D + 4) + 3 * kAbTile) * sizeof(float);
  ab_allow_lds(vit_attn_block_fwd_kernel<D>, lds);
  hipLaunchKernelGGL((vit_attn_block_fwd_kernel<D>), grid, dim3(kAbFwdThreads), lds, s, x, gamma,
                     beta, Wqkv, Wout, B, S, heads, eps, y, mean, rstd, lse);
}

template <int D>
static void ab_launch_bwd(dim3 grid, hipStream_t s, const float* dy, const float* x,
                          const float* rstd, const float* lse,
                          const float* gamma, const float* beta, const float* Wqkv,
                          const float* Wout, int64_t B, int S, int heads, int P, float* slabs,
                          float* wpart) {
  const size_t lds = (2 * static_cast<size_t>(kAbRows) * (D + 4) + 5 * kAbTile) * sizeof(float);
  ab_allow_lds(vit_attn_block_bwd_kernel<D>, lds);
  hipLaunchKernelGGL((vit_attn_block_bwd_kernel<D>), grid, dim3(kAbBwdThreads), lds, s, dy, x, rstd,
                     lse, gamma, beta, Wqkv, Wout, B, S, heads, P, slabs, wpart);
}

}  // namespace ocppo

using namespace ocppo;

#define OCPPO_AB_DISPATCH(DV, FN, ...)        \
  switch (DV) {                               \
    case 32: FN<32>(__VA_ARGS__); break;      \
    case 64: FN<64>(__VA_ARGS__); break;      \
    case 96: FN<96>(__VA_ARGS__); break;      \
    case 128: FN<128>(__VA_ARGS__); break;    \
  }

extern "C" int ocppo_vit_attn_block_fwd(ocppo_stream_t stream, const float* x, const float* gamma,
                                        const float* beta, const float* Wqkv, const float* Wout,
                                        int64_t B, int64_t S, int64_t D, int64_t heads, double eps,
                                        float* y, float* mean, float* rstd, float* lse) {
  const char* who = "ocppo_vit_attn_block_fwd";
  if (int rc = ab_check(who, B, S, D, heads)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && gamma && beta && Wqkv && Wout && y, "%s: null pointer", who);
  OCPPO_REQUIRE((mean == nullptr) == (rstd == nullptr) && (mean == nullptr) == (lse == nullptr),
                "%s: mean, rstd and lse go together", who);
  OCPPO_REQUIRE(ab_aligned16(Wqkv) && ab_aligned16(Wout), "%s: Wqkv / Wout not 16-B aligned", who);
  const dim3 grid(static_cast<unsigned>(B < kAbMaxFwdGrid ? B : kAbMaxFwdGrid));
  clear_stale_error();
  OCPPO_AB_DISPATCH(D, ab_launch_fwd, grid, as_stream(stream), x, gamma, beta, Wqkv, Wout, B,
                    (int)S, (int)heads, static_cast<float>(eps), y, mean, rstd, lse);
  return check_launch(who);
}

extern "C" size_t ocppo_vit_attn_block_workspace_bytes(int64_t B, int64_t S, int64_t D,
                                                       int64_t heads) {
  if (!ab_sizes_ok(B, S, D, heads)) return 0;
  return ab_slab_bytes(B, S, D, heads) + ab_wpart_bytes(B, D, heads) +
         static_cast<size_t>(ab_row_parts(B * S)) * kAbRowWaves * 2 * D * sizeof(double);
}

extern "C" int ocppo_vit_attn_block_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                        const float* mean, const float* rstd, const float* lse,
                                        const float* gamma, const float* beta, const float* Wqkv,
                                        const float* Wout, int64_t B, int64_t S, int64_t D,
                                        int64_t heads, float* dx, float* dgamma, float* dbeta,
                                        float* dWqkv, float* dWout, void* workspace,
                                        size_t workspace_bytes) {
  const char* who = "ocppo_vit_attn_block_bwd";
  if (int rc = ab_check(who, B, S, D, heads)) return rc;
  if (B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dy && x && mean && rstd && lse && gamma && beta && Wqkv && Wout && dx && dgamma &&
                    dbeta && dWqkv && dWout,
                "%s: null pointer", who);
  OCPPO_REQUIRE(ab_aligned16(Wqkv) && ab_aligned16(Wout), "%s: Wqkv / Wout not 16-B aligned", who);
  const size_t need = ocppo_vit_attn_block_workspace_bytes(B, S, D, heads);
  if (!workspace || workspace_bytes < need)
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes,
                need);
  OCPPO_REQUIRE(ab_aligned16(workspace), "%s: workspace not 16-B aligned", who);
  const int P = ab_parts(B, heads), nrow = ab_row_parts(B * S);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* slabs = reinterpret_cast<float*>(ws);
  float* wpart = reinterpret_cast<float*>(ws + ab_slab_bytes(B, S, D, heads));
  double* cpart = reinterpret_cast<double*>(ws + ab_slab_bytes(B, S, D, heads) +
                                            ab_wpart_bytes(B, D, heads));
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  OCPPO_AB_DISPATCH(D, ab_launch_bwd, dim3(static_cast<unsigned>(P * heads)), s, dy, x, rstd,
                    lse, gamma, beta, Wqkv, Wout, B, (int)S, (int)heads, P, slabs, wpart);
  if (int rc = check_launch(who)) return rc;
  hipLaunchKernelGGL(vit_attn_block_rows_kernel, dim3(static_cast<unsigned>(nrow)),
                     dim3(kAbFwdThreads), 0, s, dy, x, mean, rstd, gamma, slabs, B * S, (int)D,
                     (int)heads, dx, cpart);
  if (int rc = check_launch("ocppo_vit_attn_block_bwd (rows)")) return rc;
  const int64_t outs = 4 * kAbDh * heads * D + 2 * D;
  hipLaunchKernelGGL(vit_attn_block_sum_kernel,
                     dim3(static_cast<unsigned>(ceil_div(outs, kAbFwdThreads))), dim3(kAbFwdThreads),
                     0, s, wpart, cpart, P, nrow, (int)D, (int)heads, dWqkv, dWout, dgamma, dbeta);
  return check_launch("ocppo_vit_attn_block_bwd (sum)");
}
#undef OCPPO_AB_DISPATCH
