// MaDi's masker (architectures/madi.py MaskerNet, three layers) fused per image tile:
//
//   y = x * sigmoid(conv3(relu(conv2(relu(conv1(x / 255))))))   per 84 x 84 frame of a stack,
//   conv1 3x3 1->F, conv2 3x3 F->F, conv3 3x3 F->1, all zero-padded, F in {16, 32}.
//
//   ocppo_madi_mask_fwd : gather (optional int64 row index over u8 / f32 stacks) + x / 255 + the
//                         three convolutions + sigmoid + multiply, one launch; the f32 masked
//                         stacks are written in the trunk's layout (NCHW or channels_last).
//   ocppo_madi_mask_bwd : the six parameter gradients for g = dL/dy in that layout; every tile's
//                         activations are recomputed from the same rows. Two launches: the tile
//                         pass (per-workgroup partial sums) and a fixed-order finish.
//
// Tile design. A workgroup (256 threads, 4 waves) loops over tiles with the weights resident in
// LDS. For a tile it holds x on a 20 x 20 region, a1 = relu(conv1) on 18 x 18 x F and a2 =
// relu(conv2) on 16 x 16 x F, channel-last rows of F + 4 floats (16 lanes that differ in the
// position hit 16 distinct bank quads). conv2 is an implicit GEMM [256 pixels] x [9 F] x [F] on
// v_mfma_f32_16x16x4_f32: one 16-pixel row of the a2 region is one M tile, a wave owns 4 rows x
// F / 16 column tiles. An activation at a position outside the image is zero at every layer (zero
// padding applies per layer), so both stores force it.
//   forward : the 16 x 16 a2 region gives a 14 x 14 output tile (84 = 6 x 14).
//   backward: the same 16 x 16 a2 region gives z3 / dz3 on 14 x 14, dz2 on 12 x 12 and dz1 on the
//             10 x 10 pixels the tile owns; each image pixel is owned by one tile, so every sum
//             over pixels counts it once. dW2 [F][F][9] (M = out channel, N = in channel, K =
//             owned pixels) and da1 (M = in channel, N = owned pixels, K = 9 F) run on the MFMA,
//             the small sums (dW1, db1, db2, dW3, db3) on the VALU; all of them accumulate in
//             registers over the workgroup's tiles and leave as one partial row per workgroup.
// No floating-point atomics: tiles go to workgroups by a fixed stride, the finish adds the
// workgroups' rows in index order.
#include "ocppo_common.h"

namespace ocppo {

typedef float madi_x4 __attribute__((ext_vector_type(4)));

constexpr int kMadiThreads = 256;
constexpr int kMadiT = 14;    // forward output tile edge
constexpr int kMadiTB = 10;   // backward owned tile edge
constexpr int kMadiR2 = 16;   // a2 region edge
constexpr int kMadiR1 = 18;   // a1 region edge
constexpr int kMadiRX = 20;   // x region edge
constexpr int kMadiGrid = 256;  // workgroups at most (one per CU); the workspace's row count

__host__ __device__ constexpr int madi_params(int F) { return 9 * F + F + 9 * F * F + F + 9 * F + 1; }

template <int F>
struct MadiLds {
  static constexpr int LD = F + 4;
  float a1[kMadiR1 * kMadiR1 * LD];
  float a2[kMadiR2 * kMadiR2 * LD];
  float w2[9 * F * LD];  // [tap][out channel][in channel]
  float w1[9 * F];       // [tap][channel]
  float w3[9 * F];       // [tap][channel]
  float b1[F];
  float b2[F];
  float xn[kMadiRX * kMadiRX];  // x / 255, zero outside the image
  float xr[kMadiRX * kMadiRX];  // x
};

struct MadiSrc {
  const void* src;
  const int64_t* idx;
  int64_t rows, B, W, H;
  int channels_last;
};

__device__ __forceinline__ int64_t madi_out_offset(const MadiSrc& s, int64_t b, int64_t w,
                                                   int64_t y, int64_t x) {
  return s.channels_last ? ((b * s.H + y) * s.H + x) * s.W + w : ((b * s.W + w) * s.H + y) * s.H + x;
}

template <int F>
__device__ __forceinline__ void madi_load_weights(MadiLds<F>& L, const float* __restrict__ w1,
                                                  const float* __restrict__ b1,
                                                  const float* __restrict__ w2,
                                                  const float* __restrict__ b2,
                                                  const float* __restrict__ w3) {
  constexpr int LD = MadiLds<F>::LD;
  for (int i = threadIdx.x; i < 9 * F; i += kMadiThreads) {
    const int c = i / 9, tap = i - c * 9;
    L.w1[tap * F + c] = w1[i];
    L.w3[tap * F + c] = w3[i];
  }
  for (int i = threadIdx.x; i < F; i += kMadiThreads) {
    L.b1[i] = b1[i];
    L.b2[i] = b2[i];
  }
  for (int i = threadIdx.x; i < 9 * F * F; i += kMadiThreads) {
    const int n = i / (9 * F), r = i - n * 9 * F;
    const int c = r / 9, tap = r - c * 9;
    L.w2[(tap * F + n) * LD + c] = w2[i];
  }
}

// x, a1 and a2 of the tile whose a2 region starts at image position (ay, ax) of frame f.
template <int F, int SDT>
__device__ __forceinline__ void madi_tile_activations(MadiLds<F>& L, const MadiSrc& s, int64_t f,
                                                      int ay, int ax) {
  constexpr int LD = MadiLds<F>::LD;
  const int H = static_cast<int>(s.H);
  const int64_t b = f / s.W, w = f - b * s.W;
  int64_t row = s.idx ? s.idx[b] : b;
  row = row < 0 ? 0 : (row >= s.rows ? s.rows - 1 : row);  // never dereferenced out of range
  const int64_t base = (row * s.W + w) * s.H * s.H;
  for (int i = threadIdx.x; i < kMadiRX * kMadiRX; i += kMadiThreads) {
    const int yy = ay - 2 + i / kMadiRX, xx = ax - 2 + i % kMadiRX;
    float v = 0.f;
    if (yy >= 0 && yy < H && xx >= 0 && xx < H)
      v = Elem<SDT>::load(static_cast<const typename Elem<SDT>::T*>(s.src),
                          base + static_cast<int64_t>(yy) * H + xx);
    L.xr[i] = v;
    L.xn[i] = v / 255.0f;
  }
  __syncthreads();
  // layer 1 (VALU): four channels of one position per item
  constexpr int Q = F / 4;
  for (int item = threadIdx.x; item < kMadiR1 * kMadiR1 * Q; item += kMadiThreads) {
    const int p = item / Q, q = item - p * Q;
    const int i = p / kMadiR1, j = p - i * kMadiR1;
    const int yy = ay - 1 + i, xx = ax - 1 + j;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (yy >= 0 && yy < H && xx >= 0 && xx < H) {
      acc = *reinterpret_cast<const float4*>(&L.b1[4 * q]);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float xv = L.xn[(i + tap / 3) * kMadiRX + j + tap % 3];
        const float4 wv = *reinterpret_cast<const float4*>(&L.w1[tap * F + 4 * q]);
        acc.x = fmaf(wv.x, xv, acc.x);
        acc.y = fmaf(wv.y, xv, acc.y);
        acc.z = fmaf(wv.z, xv, acc.z);
        acc.w = fmaf(wv.w, xv, acc.w);
      }
      acc = relu_f4(acc);
    }
    *reinterpret_cast<float4*>(&L.a1[p * LD + 4 * q]) = acc;
  }
  __syncthreads();
  // layer 2 (MFMA): wave wv owns region rows 4 wv .. 4 wv + 3, all F / 16 channel tiles
  constexpr int NT = F / 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  madi_x4 acc[4][NT];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = madi_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap - dy * 3;
    const float* ap = &L.a1[((wv * 4 + dy) * kMadiR1 + c16 + dx) * LD + g];
    const float* bp = &L.w2[(tap * F + c16) * LD + g];
#pragma unroll 4
    for (int k = 0; k < F; k += 4) {
      float a[4], bb[NT];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) a[mi] = ap[mi * kMadiR1 * LD + k];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) bb[ni] = bp[ni * 16 * LD + k];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
    }
  }
  // D: row (pixel column of the region row) = 4 g + r, column (channel) = c16
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = wv * 4 + mi;
    const int yy = ay + m;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int n = ni * 16 + c16;
      const float bv = L.b2[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 4 * g + r, xx = ax + c;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < H;
        L.a2[(m * kMadiR2 + c) * LD + n] = in ? relu_f(acc[mi][ni][r] + bv) : 0.f;
      }
    }
  }
  __syncthreads();
}

// z3 at the a2-region position (u, v), 1 <= u, v <= 14
template <int F>
__device__ __forceinline__ float madi_z3(const MadiLds<F>& L, int u, int v, float b3) {
  constexpr int LD = MadiLds<F>::LD;
  float z = b3;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const float* ap = &L.a2[((u - 1 + tap / 3) * kMadiR2 + v - 1 + tap % 3) * LD];
    const float* wp = &L.w3[tap * F];
#pragma unroll
    for (int c = 0; c < F; c += 4) {
      const float4 av = *reinterpret_cast<const float4*>(ap + c);
      const float4 wv = *reinterpret_cast<const float4*>(wp + c);
      z = fmaf(av.x, wv.x, z);
      z = fmaf(av.y, wv.y, z);
      z = fmaf(av.z, wv.z, z);
      z = fmaf(av.w, wv.w, z);
    }
  }
  return z;
}

__device__ __forceinline__ float madi_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

template <int F, int SDT>
__global__ __launch_bounds__(kMadiThreads) void madi_fwd_kernel(
    MadiSrc s, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) MadiLds<F> L;
  madi_load_weights<F>(L, w1, b1, w2, b2, w3);
  const float b3v = b3[0];
  const int H = static_cast<int>(s.H);
  const int nt = (H + kMadiT - 1) / kMadiT;
  const int64_t tiles = s.B * s.W * nt * nt;
  __syncthreads();
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t f = t / (nt * nt);
    const int r = static_cast<int>(t - f * nt * nt);
    const int oy = (r / nt) * kMadiT, ox = (r % nt) * kMadiT;
    madi_tile_activations<F, SDT>(L, s, f, oy - 1, ox - 1);
    const int p = threadIdx.x;
    if (p < kMadiT * kMadiT) {
      const int py = p / kMadiT, px = p - py * kMadiT;
      const int yy = oy + py, xx = ox + px;
      if (yy < H && xx < H) {
        const float z = madi_z3<F>(L, py + 1, px + 1, b3v);
        const int64_t b = f / s.W, w = f - b * s.W;
        out[madi_out_offset(s, b, w, yy, xx)] =
            L.xr[(py + 3) * kMadiRX + px + 3] * madi_sigmoid(z);
      }
    }
    __syncthreads();
  }
}

template <int F>
struct MadiBwdLds {
  float dz1[kMadiTB * kMadiTB * (F + 1)];
  float dz3[kMadiT * kMadiT];
};

// Partial row of a workgroup: dW1 [F][9], db1 [F], dW2 [F][F][9], db2 [F], dW3 [F][9], db3.
template <int F, int SDT>
__global__ __launch_bounds__(kMadiThreads) void madi_bwd_kernel(
    MadiSrc s, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, const float* __restrict__ gout, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) MadiLds<F> L;
  __shared__ MadiBwdLds<F> Lb;
  constexpr int LD = MadiLds<F>::LD;
  constexpr int LZ = F + 1;
  constexpr int NT = F / 16;
  constexpr int NP = kMadiTB * kMadiTB;       // owned pixels per tile
  constexpr int W2T = NT * NT * 9;            // dW2 accumulator tiles
  constexpr int W2PER = (W2T + 3) / 4;        // ... per wave
  constexpr int PT = (NP + 15) / 16;          // pixel tiles of the da1 product
  constexpr int PTPER = (PT + 3) / 4;         // ... per wave
  madi_load_weights<F>(L, w1, b1, w2, b2, w3);
  const float b3v = b3[0];
  const int H = static_cast<int>(s.H);
  const int nt = (H + kMadiTB - 1) / kMadiTB;
  const int64_t tiles = s.B * s.W * nt * nt;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  // the VALU sums run in f64 (exact products): a bias gradient is a sum with cancellation
  double sA[2] = {0.0, 0.0};  // dW3 / db3 items tid, tid + 256
  double sB = 0.0;            // db2 item tid
  double sC[2] = {0.0, 0.0};  // dW1 / db1 items tid, tid + 256
  madi_x4 dw2[W2PER];
#pragma unroll
  for (int i = 0; i < W2PER; ++i) dw2[i] = madi_x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t f = t / (nt * nt);
    const int r = static_cast<int>(t - f * nt * nt);
    const int oy = (r / nt) * kMadiTB, ox = (r % nt) * kMadiTB;  // first owned pixel
    const int ay = oy - 3, ax = ox - 3;
    madi_tile_activations<F, SDT>(L, s, f, ay, ax);
    // dz3 = g x s (1 - s) on the 14 x 14 positions (a2 region 1 .. 14), zero outside the image
    if (tid < kMadiT * kMadiT) {
      const int py = tid / kMadiT, px = tid - py * kMadiT;
      const int yy = ay + 1 + py, xx = ax + 1 + px;
      float d = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < H) {
        const float sg = madi_sigmoid(madi_z3<F>(L, py + 1, px + 1, b3v));
        const int64_t b = f / s.W, w = f - b * s.W;
        d = gout[madi_out_offset(s, b, w, yy, xx)] * L.xr[(py + 3) * kMadiRX + px + 3] *
            (sg * (1.0f - sg));
      }
      Lb.dz3[tid] = d;
    }
    __syncthreads();
    // dW3 [c][tap] = sum over owned pixels dz3 a2[pixel + tap - 1][c]; db3 = sum dz3
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int item = tid + k * kMadiThreads;
      if (item < 9 * F) {
        const int tap = item / F, c = item - tap * F;
        const int dy = tap / 3, dx = tap - dy * 3;
        double a = sA[k];
#pragma unroll 1
        for (int iy = 0; iy < kMadiTB; ++iy)
#pragma unroll 5
          for (int ix = 0; ix < kMadiTB; ++ix)
            a = fma(static_cast<double>(Lb.dz3[(2 + iy) * kMadiT + 2 + ix]),
                    static_cast<double>(L.a2[((2 + iy + dy) * kMadiR2 + 2 + ix + dx) * LD + c]), a);
        sA[k] = a;
      } else if (item == 9 * F) {
        double a = sA[k];
#pragma unroll 1
        for (int iy = 0; iy < kMadiTB; ++iy)
#pragma unroll 5
          for (int ix = 0; ix < kMadiTB; ++ix)
            a += static_cast<double>(Lb.dz3[(2 + iy) * kMadiT + 2 + ix]);
        sA[k] = a;
      }
    }
    __syncthreads();
    // dz2 = da2 [a2 > 0] in place over a2 on the 12 x 12 positions 2 .. 13 (a2 is zero outside
    // the image, so dz2 is)
    for (int item = tid; item < 12 * 12 * (F / 4); item += kMadiThreads) {
      const int p = item / (F / 4), q = item - p * (F / 4);
      const int jy = p / 12, jx = p - jy * 12;
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float z = Lb.dz3[(2 + jy - tap / 3) * kMadiT + 2 + jx - tap % 3];
        const float4 wq = *reinterpret_cast<const float4*>(&L.w3[tap * F + 4 * q]);
        d.x = fmaf(wq.x, z, d.x);
        d.y = fmaf(wq.y, z, d.y);
        d.z = fmaf(wq.z, z, d.z);
        d.w = fmaf(wq.w, z, d.w);
      }
      float4* ap = reinterpret_cast<float4*>(&L.a2[((2 + jy) * kMadiR2 + 2 + jx) * LD + 4 * q]);
      const float4 a = *ap;
      *ap = make_float4(a.x > 0.f ? d.x : 0.f, a.y > 0.f ? d.y : 0.f, a.z > 0.f ? d.z : 0.f,
                        a.w > 0.f ? d.w : 0.f);
    }
    __syncthreads();
    // db2 [n] = sum over owned pixels dz2
    if (tid < F) {
      double a = sB;
#pragma unroll 1
      for (int iy = 0; iy < kMadiTB; ++iy)
#pragma unroll 5
        for (int ix = 0; ix < kMadiTB; ++ix)
          a += static_cast<double>(L.a2[((3 + iy) * kMadiR2 + 3 + ix) * LD + tid]);
      sB = a;
    }
    // dW2 [n][c][tap] += sum over owned pixels dz2[p][n] a1[p + tap - 1][c]: tile (pair, tap),
    // A[row n][k pixel], B[k pixel][col c]
#pragma unroll
    for (int i = 0; i < W2PER; ++i) {
      const int tile = wv + 4 * i;
      if (tile < W2T) {
        const int pair = tile / 9, tap = tile - pair * 9;
        const int ntile = pair / NT, ctile = pair - ntile * NT;
        const int dy = tap / 3, dx = tap - dy * 3;
        madi_x4 acc = dw2[i];
#pragma unroll 5
        for (int p0 = 0; p0 < NP; p0 += 4) {
          const int p = p0 + g;  // NP % 4 == 0
          const int py = p / kMadiTB, px = p - py * kMadiTB;
          const float a = L.a2[((3 + py) * kMadiR2 + 3 + px) * LD + ntile * 16 + c16];
          const float bb = L.a1[((3 + py + dy) * kMadiR1 + 3 + px + dx) * LD + ctile * 16 + c16];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc, 0, 0, 0);
        }
        dw2[i] = acc;
      }
    }
    // da1 [c][pixel] = sum over (tap, n) w2[n][c][tap] dz2[pixel - (tap - 1)][n]; dz1 = da1
    // [a1 > 0]: A[row c][k n], B[k n][col pixel]
#pragma unroll
    for (int i = 0; i < PTPER; ++i) {
      const int ptile = wv + 4 * i;
      if (ptile < PT) {
        const int praw = ptile * 16 + c16;
        const int p = praw < NP ? praw : NP - 1;
        const int py = p / kMadiTB, px = p - py * kMadiTB;
        madi_x4 acc[NT];
#pragma unroll
        for (int ci = 0; ci < NT; ++ci) acc[ci] = madi_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3, dx = tap - dy * 3;
          const float* bp = &L.a2[((4 + py - dy) * kMadiR2 + 4 + px - dx) * LD + g];
          const float* ap = &L.w2[(tap * F + g) * LD + c16];
#pragma unroll 4
          for (int k = 0; k < F; k += 4) {
            const float bb = bp[k];
#pragma unroll
            for (int ci = 0; ci < NT; ++ci)
              acc[ci] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * LD + ci * 16], bb, acc[ci], 0,
                                                             0, 0);
          }
        }
        if (praw < NP) {
#pragma unroll
          for (int ci = 0; ci < NT; ++ci)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int c = ci * 16 + 4 * g + rr;
              const float a = L.a1[((4 + py) * kMadiR1 + 4 + px) * LD + c];
              Lb.dz1[p * LZ + c] = a > 0.f ? acc[ci][rr] : 0.f;
            }
        }
      }
    }
    __syncthreads();
    // dW1 [c][tap] = sum over owned pixels dz1[p][c] xn[p + tap - 1]; db1 [c] = sum dz1[p][c]
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int item = tid + k * kMadiThreads;
      if (item < 9 * F) {
        const int tap = item / F, c = item - tap * F;
        const int dy = tap / 3, dx = tap - dy * 3;
        double a = sC[k];
#pragma unroll 1
        for (int iy = 0; iy < kMadiTB; ++iy)
#pragma unroll 5
          for (int ix = 0; ix < kMadiTB; ++ix)
            a = fma(static_cast<double>(Lb.dz1[(iy * kMadiTB + ix) * LZ + c]),
                    static_cast<double>(L.xn[(4 + iy + dy) * kMadiRX + 4 + ix + dx]), a);
        sC[k] = a;
      } else if (item < 10 * F) {
        const int c = item - 9 * F;
        double a = sC[k];
#pragma unroll 4
        for (int p = 0; p < NP; ++p) a += static_cast<double>(Lb.dz1[p * LZ + c]);
        sC[k] = a;
      }
    }
    __syncthreads();
  }
  // the workgroup's partial row
  float* o = ws + static_cast<int64_t>(blockIdx.x) * madi_params(F);
  float* o_dw1 = o;
  float* o_db1 = o + 9 * F;
  float* o_dw2 = o + 10 * F;
  float* o_db2 = o_dw2 + 9 * F * F;
  float* o_dw3 = o_db2 + F;
  float* o_db3 = o_dw3 + 9 * F;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int item = tid + k * kMadiThreads;
    if (item < 9 * F) {
      const int tap = item / F, c = item - tap * F;
      o_dw3[c * 9 + tap] = static_cast<float>(sA[k]);
      o_dw1[c * 9 + tap] = static_cast<float>(sC[k]);
    } else if (item == 9 * F) {
      o_db3[0] = static_cast<float>(sA[k]);
    }
    if (item >= 9 * F && item < 10 * F) o_db1[item - 9 * F] = static_cast<float>(sC[k]);
  }
  if (tid < F) o_db2[tid] = static_cast<float>(sB);
#pragma unroll
  for (int i = 0; i < W2PER; ++i) {
    const int tile = wv + 4 * i;
    if (tile < W2T) {
      const int pair = tile / 9, tap = tile - pair * 9;
      const int ntile = pair / NT, ctile = pair - ntile * NT;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int n = ntile * 16 + 4 * g + rr, c = ctile * 16 + c16;
        o_dw2[(n * F + c) * 9 + tap] = dw2[i][rr];
      }
    }
  }
}

// out[i] = partial rows 0 .. nparts - 1 of parameter i, added in that order
__global__ __launch_bounds__(256) void madi_bwd_finish_kernel(
    const float* __restrict__ ws, int nparts, int F, float* __restrict__ dw1,
    float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2,
    float* __restrict__ dw3, float* __restrict__ db3) {
  const int P = madi_params(F);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float a = 0.f;
  for (int k = 0; k < nparts; ++k) a += ws[static_cast<int64_t>(k) * P + i];
  int j = i;
  if (j < 9 * F) { dw1[j] = a; return; }
  j -= 9 * F;
  if (j < F) { db1[j] = a; return; }
  j -= F;
  if (j < 9 * F * F) { dw2[j] = a; return; }
  j -= 9 * F * F;
  if (j < F) { db2[j] = a; return; }
  j -= F;
  if (j < 9 * F) { dw3[j] = a; return; }
  db3[0] = a;
}

static int64_t madi_tiles(int64_t B, int64_t W, int64_t H, int T) {
  const int64_t nt = ceil_div(H, T);
  return B * W * nt * nt;
}

static int madi_check(const char* who, const void* src, int src_dtype, int64_t rows, int64_t B,
                      int64_t W, int64_t H, int64_t F, const float* w1, const float* b1,
                      const float* w2, const float* b2, const float* w3, const float* b3) {
  OCPPO_REQUIRE(src_dtype == OCPPO_U8 || src_dtype == OCPPO_F32,
                "%s: dtype %d is not OCPPO_U8 / OCPPO_F32", who, src_dtype);
  OCPPO_REQUIRE(F == 16 || F == 32, "%s: F=%lld filters (16 or 32)", who, (long long)F);
  OCPPO_REQUIRE(rows >= 1 && B >= 1 && W >= 1 && H >= 1 && H <= 32768 && W <= 65536 &&
                    B <= (int64_t(1) << 40) / (W * H * H) && rows <= (int64_t(1) << 40) / (W * H * H),
                "%s: bad sizes rows=%lld B=%lld W=%lld H=%lld", who, (long long)rows, (long long)B,
                (long long)W, (long long)H);
  OCPPO_REQUIRE(src && w1 && b1 && w2 && b2 && w3 && b3, "%s: null pointer", who);
  return OCPPO_OK;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_madi_workspace_bytes(int64_t F) {
  if (F != 16 && F != 32) return 0;
  return static_cast<size_t>(kMadiGrid) * madi_params(static_cast<int>(F)) * sizeof(float);
}

extern "C" int ocppo_madi_mask_fwd(ocppo_stream_t stream, const void* src, int src_dtype,
                                   const int64_t* idx, int64_t rows, int64_t B, int64_t W,
                                   int64_t H, int64_t F, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const float* w3,
                                   const float* b3, int channels_last, float* out) {
  if (int rc = madi_check("ocppo_madi_mask_fwd", src, src_dtype, rows, B, W, H, F, w1, b1, w2, b2,
                          w3, b3))
    return rc;
  OCPPO_REQUIRE(out, "ocppo_madi_mask_fwd: null pointer");
  const MadiSrc s{src, idx, rows, B, W, H, channels_last ? 1 : 0};
  const int64_t tiles = madi_tiles(B, W, H, kMadiT);
  const unsigned grid = static_cast<unsigned>(tiles < 2 * kMadiGrid ? tiles : 2 * kMadiGrid);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
#define OCPPO_MADI_FWD(FF, DT)                                                                    \
  hipLaunchKernelGGL((madi_fwd_kernel<FF, DT>), dim3(grid), dim3(kMadiThreads), 0, st, s, w1, b1, \
                     w2, b2, w3, b3, out)
  if (F == 32 && src_dtype == OCPPO_U8) OCPPO_MADI_FWD(32, OCPPO_U8);
  else if (F == 32) OCPPO_MADI_FWD(32, OCPPO_F32);
  else if (src_dtype == OCPPO_U8) OCPPO_MADI_FWD(16, OCPPO_U8);
  else OCPPO_MADI_FWD(16, OCPPO_F32);
#undef OCPPO_MADI_FWD
  return check_launch("ocppo_madi_mask_fwd");
}

extern "C" int ocppo_madi_mask_bwd(ocppo_stream_t stream, const void* src, int src_dtype,
                                   const int64_t* idx, int64_t rows, int64_t B, int64_t W,
                                   int64_t H, int64_t F, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const float* w3,
                                   const float* b3, int channels_last, const float* g,
                                   float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                   float* db3, void* workspace, size_t workspace_bytes) {
  if (int rc = madi_check("ocppo_madi_mask_bwd", src, src_dtype, rows, B, W, H, F, w1, b1, w2, b2,
                          w3, b3))
    return rc;
  OCPPO_REQUIRE(g && dw1 && db1 && dw2 && db2 && dw3 && db3, "ocppo_madi_mask_bwd: null pointer");
  if (!workspace || workspace_bytes < ocppo_madi_workspace_bytes(F) ||
      reinterpret_cast<uintptr_t>(workspace) % 4)
    return fail(OCPPO_E_WORKSPACE, "ocppo_madi_mask_bwd: workspace of %zu bytes needed",
                ocppo_madi_workspace_bytes(F));
  const MadiSrc s{src, idx, rows, B, W, H, channels_last ? 1 : 0};
  const int64_t tiles = madi_tiles(B, W, H, kMadiTB);
  const unsigned grid = static_cast<unsigned>(tiles < kMadiGrid ? tiles : kMadiGrid);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
#define OCPPO_MADI_BWD(FF, DT)                                                                    \
  hipLaunchKernelGGL((madi_bwd_kernel<FF, DT>), dim3(grid), dim3(kMadiThreads), 0, st, s, w1, b1, \
                     w2, b2, w3, b3, g, ws)
  if (F == 32 && src_dtype == OCPPO_U8) OCPPO_MADI_BWD(32, OCPPO_U8);
  else if (F == 32) OCPPO_MADI_BWD(32, OCPPO_F32);
  else if (src_dtype == OCPPO_U8) OCPPO_MADI_BWD(16, OCPPO_U8);
  else OCPPO_MADI_BWD(16, OCPPO_F32);
#undef OCPPO_MADI_BWD
  if (int rc = check_launch("ocppo_madi_mask_bwd")) return rc;
  const int P = madi_params(static_cast<int>(F));
  hipLaunchKernelGGL(madi_bwd_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, st, ws,
                     static_cast<int>(grid), static_cast<int>(F), dw1, db1, dw2, db2, dw3, db3);
  return check_launch("ocppo_madi_mask_bwd (finish)");
}
