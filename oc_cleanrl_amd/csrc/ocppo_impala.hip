// The IMPALA tower's ConvSequence (qdagger_dqn_atari_impalacnn.py:126-160, ppg_procgen.py:124-165)
// as two fused units, forward and backward, on NHWC f32 activations:
//
//   ocppo_impala_resblock_fwd / _bwd  : y = x + conv1(relu(conv0(relu(x)) + b0)) + b1, both 3x3
//                                       zero-padded, C -> C, C in {16, 32}
//   ocppo_impala_conv_pool_fwd / _bwd : p = max_pool2d(conv(scale x) + b, 3, stride 2, padding 1),
//                                       3x3 zero-padded, Cin <= 4 or in {16, 32}, Cout in {16, 32}
//
// Tile design. A workgroup (256 threads, 4 waves) loops over the tiles of all images with its
// weights resident in LDS as [tap][k / 4][n][4]: the 64 lanes of a B-operand read hit 64
// consecutive words, so the blocks need no padding. Activations sit in LDS regions with channel-last
// rows of C + 4 floats. Every convolution, forward or transposed, is one routine: an implicit GEMM
// [region pixels] x [9 K] x [N] on v_mfma_f32_16x16x4_f32 where a 16-pixel region row is an M
// tile and a wave owns 4 rows x N / 16 column tiles. It comes in two geometries:
//   outer: an 18 x 18 input region gives a 16 x 16 output region
//   inner: a 16 x 16 input region gives the 14 x 14 pixels a tile owns (rows and columns 14, 15
//          are clamped duplicates that nobody stores)
// The data gradient of a convolution is the same routine on the weights staged transposed with the
// taps reversed. Positions outside the image are forced to zero (-inf before the pool) after every
// layer: padding applies per layer.
//   resblock fwd : relu(x) on 18 x 18 -> outer conv0 -> mid on 16 x 16 -> inner conv1 + skip from
//                  the staged x. The mid activation goes to HBM only when the backward wants it.
//   resblock bwd : dy on 18 x 18 and the saved mid on 16 x 16; dW1 (MFMA: M = out channel, N = in
//                  channel, K = the 196 owned pixels, one accumulator tile per tap), outer
//                  transposed conv1 -> d(mid) masked in place over mid, x on 16 x 16 over the dy
//                  region, dW0, inner transposed conv0 -> dx = dy + [x > 0] da.
//   conv + pool  : fwd: outer conv on the 18 x 18 input region, the 16 x 16 (15 used) conv region
//                  is pooled in LDS to 7 x 7 outputs with the window position of the maximum (first
//                  in row-major order on ties) as one byte. bwd: a tile owns 14 x 14 conv positions;
//                  dz on their 16 x 16 region is gathered from the <= 4 pooled outputs whose window
//                  holds a position (fixed order), then dW / db / inner transposed conv -> dx.
// No floating-point atomics: tiles go to workgroups by a fixed stride, a workgroup's weight and
// bias gradients accumulate in registers (biases in f64) over its tiles and leave as one partial
// row; the finish launch adds the rows in index order.
#include "ocppo_common.h"

namespace ocppo {

typedef float imp_x4 __attribute__((ext_vector_type(4)));

constexpr int kImpThreads = 256;
constexpr int kImpT = 14;     // edge of the pixels a tile owns
constexpr int kImpR1 = 16;    // inner region edge
constexpr int kImpR0 = 18;    // outer region edge
constexpr int kImpTP = 7;     // pooled outputs per tile edge (2 * 7 + 1 conv rows)
constexpr int kImpNP = kImpT * kImpT;
constexpr int kImpGrid = 256;  // workgroups at most (one per CU); the workspace's row count

// ---- staging ----------------------------------------------------------------------------------
// nn.Conv2d weights [co][ci][3][3] into LDS as [tap][k / 4][n][4].
//   TRANS false: k = ci (ck_real of them), n = co                       (forward)
//   TRANS true : k = co, n = ci (cn_real of them), taps reversed        (data gradient)
// Rows / columns past the real count are zero.
template <int CK, int CN, bool TRANS>
__device__ __forceinline__ void imp_stage_w(float* __restrict__ dst, const float* __restrict__ w,
                                            int ck_real, int cn_real) {
  for (int i = threadIdx.x; i < 9 * CK * CN; i += kImpThreads) {
    const int tap = i / (CK * CN), r = i - tap * (CK * CN);
    const int kb = r / (CN * 4), r2 = r - kb * (CN * 4);
    const int n = r2 >> 2, k = kb * 4 + (r2 & 3);
    float v = 0.f;
    if (k < ck_real && n < cn_real)
      v = TRANS ? w[(k * cn_real + n) * 9 + 8 - tap] : w[(n * ck_real + k) * 9 + tap];
    dst[i] = v;
  }
}

// Region of RH x RW positions from image position (y0, x0) of image b (NHWC, creal channels),
// times scale, zero outside the image and in channels creal .. C - 1.
template <int C>
__device__ __forceinline__ void imp_load_region(float* __restrict__ dst, int RW, int RH,
                                                const float* __restrict__ src, int creal,
                                                int64_t b, int y0, int x0, int H, int W,
                                                float scale) {
  constexpr int LD = C + 4, Q = C / 4;
  for (int item = threadIdx.x; item < RH * RW * Q; item += kImpThreads) {
    const int p = item / Q, q = item - p * Q;
    const int py = p / RW;
    const int yy = y0 + py, xx = x0 + p - py * RW;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const float* s = src + ((b * H + yy) * W + xx) * creal + 4 * q;
      if (creal == C) {
        v = *reinterpret_cast<const float4*>(s);
      } else {
        const int left = creal - 4 * q;
        if (left > 0) v.x = s[0];
        if (left > 1) v.y = s[1];
        if (left > 2) v.z = s[2];
        if (left > 3) v.w = s[3];
      }
      v = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    }
    *reinterpret_cast<float4*>(&dst[p * LD + 4 * q]) = v;
  }
}

// ---- the convolution routine --------------------------------------------------------------------
// acc[mi][ni] = output row min(4 wave + mi, MAXI), channels 16 ni .. 16 ni + 15 of the 3x3
// convolution of the region `in` (RIN = MAXI + 3 wide, rows of CK + 4 floats) with the staged
// weights: output (m, c) reads in (m + 0..2, c + 0..2). D: column c = 4 g + r, channel c16.
template <int CK, int CN, int RIN, int MAXI, bool RELU_IN>
__device__ __forceinline__ void imp_conv(const float* __restrict__ in, const float* __restrict__ w,
                                         imp_x4 (&acc)[4][CN / 16]) {
  static_assert(RIN == MAXI + 3, "region width");
  constexpr int LD = CK + 4, NT = CN / 16, KB = CK / 4;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int cc = c16 < MAXI ? c16 : MAXI;
  int base[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = wv * 4 + mi;
    base[mi] = ((m < MAXI ? m : MAXI) * RIN + cc) * LD + g;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = imp_x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3, dx = tap - dy * 3;
    const float* ap = in + (dy * RIN + dx) * LD;
    const float* bp = w + (tap * KB * CN + c16) * 4 + g;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float a[4], bb[NT];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        a[mi] = ap[base[mi] + kb * 4];
        if (RELU_IN) a[mi] = relu_f(a[mi]);
      }
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) bb[ni] = bp[(kb * CN + ni * 16) * 4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
    }
  }
}

// ---- weight gradient ------------------------------------------------------------------------------
// dW [m][n][tap] += sum over the 196 owned pixels p of z[p][m] act[p + tap - 1][n]. z: region ZW
// wide, the owned pixels from (ZOFF, ZOFF); act: 16 wide region whose (1, 1) is the first owned
// pixel. The CM / 16 x ceil(CN / 16) channel tile pairs are dealt to the 4 waves; the waves of a
// pair share its 9 taps. z is zero at owned positions outside the image.
template <int CM, int CN>
struct ImpDw {
  static constexpr int NTN = CN < 16 ? 1 : CN / 16;
  static constexpr int PAIRS = (CM / 16) * NTN;
  static constexpr int WPP = 4 / PAIRS;             // waves per pair
  static constexpr int NACC = (9 + WPP - 1) / WPP;  // taps per wave
  static_assert(PAIRS == 1 || PAIRS == 2 || PAIRS == 4, "channel tile pairs");
};

template <int CM, int CN, int ZW, int ZOFF, bool RELU_ACT>
__device__ __forceinline__ void imp_dw(const float* __restrict__ z, const float* __restrict__ act,
                                       imp_x4 (&acc)[ImpDw<CM, CN>::NACC]) {
  using D = ImpDw<CM, CN>;
  constexpr int LDZ = CM + 4, LDA = CN + 4;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int pair = wv / D::WPP, sub = wv - pair * D::WPP;
  const int mt = pair / D::NTN, nt = pair - mt * D::NTN;
  const int cn = CN < 16 ? (c16 < CN ? c16 : CN - 1) : nt * 16 + c16;  // columns >= CN: unused
#pragma unroll 1
  for (int p0 = 0; p0 < kImpNP; p0 += 4) {
    const int p = p0 + g;  // kImpNP % 4 == 0
    const int py = p / kImpT, px = p - py * kImpT;
    const float a = z[((ZOFF + py) * ZW + ZOFF + px) * LDZ + mt * 16 + c16];
    const float* bp = act + (py * kImpR1 + px) * LDA + cn;
#pragma unroll
    for (int i = 0; i < D::NACC; ++i) {
      const int tap = sub + i * D::WPP;
      if (tap < 9) {
        const int dy = tap / 3, dx = tap - dy * 3;
        float bb = bp[(dy * kImpR1 + dx) * LDA];
        if (RELU_ACT) bb = relu_f(bb);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bb, acc[i], 0, 0, 0);
      }
    }
  }
}

// o[(m * cn_real + n) * 9 + tap] of the wave's accumulators (D: row m = 4 g + r, column n = c16)
template <int CM, int CN>
__device__ __forceinline__ void imp_dw_store(float* __restrict__ o, int cn_real,
                                             const imp_x4 (&acc)[ImpDw<CM, CN>::NACC]) {
  using D = ImpDw<CM, CN>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int pair = wv / D::WPP, sub = wv - pair * D::WPP;
  const int mt = pair / D::NTN, nt = pair - mt * D::NTN;
  const int n = nt * 16 + c16;
#pragma unroll
  for (int i = 0; i < D::NACC; ++i) {
    const int tap = sub + i * D::WPP;
    if (tap < 9 && n < cn_real) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[((mt * 16 + 4 * g + r) * cn_real + n) * 9 + tap] = acc[i][r];
    }
  }
}

// Bias gradient: thread (group, channel) adds the owned pixels group, group + G, ... in f64.
template <int C, int ZW, int ZOFF>
__device__ __forceinline__ double imp_db(const float* __restrict__ z, double a) {
  constexpr int G = kImpThreads / C, LD = C + 4;
  const int c = threadIdx.x % C, grp = threadIdx.x / C;
  for (int p = grp; p < kImpNP; p += G) {
    const int py = p / kImpT, px = p - py * kImpT;
    a += static_cast<double>(z[((ZOFF + py) * ZW + ZOFF + px) * LD + c]);
  }
  return a;
}

// The groups' sums of a channel in group order; scratch: kImpThreads doubles.
template <int C>
__device__ __forceinline__ void imp_db_store(float* __restrict__ o, double a, double* scratch) {
  constexpr int G = kImpThreads / C;
  __syncthreads();
  scratch[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < C) {
    double s = 0.0;
    for (int k = 0; k < G; ++k) s += scratch[k * C + threadIdx.x];
    o[threadIdx.x] = static_cast<float>(s);
  }
}

struct ImpTile {
  int64_t b;
  int oy, ox;
};

__device__ __forceinline__ ImpTile imp_tile(int64_t t, int nty, int ntx, int T) {
  const int64_t b = t / (nty * ntx);
  const int r = static_cast<int>(t - b * nty * ntx);
  return ImpTile{b, (r / ntx) * T, (r % ntx) * T};
}

// ---- residual block ---------------------------------------------------------------------------------
template <int C>
struct ImpResLds {
  static constexpr int LD = C + 4;
  float r0[kImpR0 * kImpR0 * LD];  // fwd: x; bwd: dy, then x on 16 x 16
  float r1[kImpR1 * kImpR1 * LD];  // fwd: mid; bwd: mid, then d(mid) in place
  float wa[9 * C * C];             // fwd: w0; bwd: w1 transposed
  float wb[9 * C * C];             // fwd: w1; bwd: w0 transposed
  float ba[C];
  float bb[C];
};

template <int C>
__global__ __launch_bounds__(kImpThreads) void imp_res_fwd_kernel(
    const float* __restrict__ x, int64_t B, int H, int W, const float* __restrict__ w0,
    const float* __restrict__ b0, const float* __restrict__ w1, const float* __restrict__ b1,
    float* __restrict__ y, float* __restrict__ mid) {
  __shared__ __attribute__((aligned(16))) ImpResLds<C> L;
  constexpr int LD = C + 4, NT = C / 16;
  imp_stage_w<C, C, false>(L.wa, w0, C, C);
  imp_stage_w<C, C, false>(L.wb, w1, C, C);
  for (int i = threadIdx.x; i < C; i += kImpThreads) {
    L.ba[i] = b0[i];
    L.bb[i] = b1[i];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
  const int nty = (H + kImpT - 1) / kImpT, ntx = (W + kImpT - 1) / kImpT;
  const int64_t tiles = B * nty * ntx;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const ImpTile tl = imp_tile(t, nty, ntx, kImpT);
    imp_load_region<C>(L.r0, kImpR0, kImpR0, x, C, tl.b, tl.oy - 2, tl.ox - 2, H, W, 1.0f);
    __syncthreads();
    imp_x4 acc[4][NT];
    imp_conv<C, C, kImpR0, 15, true>(L.r0, L.wa, acc);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = wv * 4 + mi, yy = tl.oy - 1 + m;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = ni * 16 + c16;
        const float bv = L.ba[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 4 * g + r, xx = tl.ox - 1 + c;
          const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const float v = in ? relu_f(acc[mi][ni][r] + bv) : 0.f;
          L.r1[(m * kImpR1 + c) * LD + n] = v;
          if (mid && in && m >= 1 && m <= kImpT && c >= 1 && c <= kImpT)
            mid[((tl.b * H + yy) * W + xx) * C + n] = v;
        }
      }
    }
    __syncthreads();
    imp_conv<C, C, kImpR1, 13, false>(L.r1, L.wb, acc);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = wv * 4 + mi, yy = tl.oy + m;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = ni * 16 + c16;
        const float bv = L.bb[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 4 * g + r, xx = tl.ox + c;
          if (m < kImpT && c < kImpT && yy < H && xx < W)
            y[((tl.b * H + yy) * W + xx) * C + n] =
                (acc[mi][ni][r] + bv) + L.r0[((m + 2) * kImpR0 + c + 2) * LD + n];
        }
      }
    }
    __syncthreads();
  }
}

// Partial row of a workgroup: dW0 [C][C][9], db0 [C], dW1 [C][C][9], db1 [C].
__host__ __device__ constexpr int imp_res_params(int C) { return 2 * (9 * C * C + C); }

template <int C>
__global__ __launch_bounds__(kImpThreads) void imp_res_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mid,
    int64_t B, int H, int W, const float* __restrict__ w0, const float* __restrict__ w1,
    float* __restrict__ dx, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) ImpResLds<C> L;
  constexpr int LD = C + 4, NT = C / 16;
  constexpr int NACC = ImpDw<C, C>::NACC;
  imp_stage_w<C, C, true>(L.wa, w1, C, C);
  imp_stage_w<C, C, true>(L.wb, w0, C, C);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
  const int nty = (H + kImpT - 1) / kImpT, ntx = (W + kImpT - 1) / kImpT;
  const int64_t tiles = B * nty * ntx;
  imp_x4 dw0[NACC], dw1[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) dw0[i] = dw1[i] = imp_x4{0.f, 0.f, 0.f, 0.f};
  double db0 = 0.0, db1 = 0.0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const ImpTile tl = imp_tile(t, nty, ntx, kImpT);
    imp_load_region<C>(L.r0, kImpR0, kImpR0, dy, C, tl.b, tl.oy - 2, tl.ox - 2, H, W, 1.0f);
    imp_load_region<C>(L.r1, kImpR1, kImpR1, mid, C, tl.b, tl.oy - 1, tl.ox - 1, H, W, 1.0f);
    __syncthreads();
    // second convolution: dW1 = dy x mid, db1 = sum dy, d(mid) = [mid > 0] conv1^T(dy)
    imp_dw<C, C, kImpR0, 2, false>(L.r0, L.r1, dw1);
    db1 = imp_db<C, kImpR0, 2>(L.r0, db1);
    imp_x4 acc[4][NT];
    imp_conv<C, C, kImpR0, 15, false>(L.r0, L.wa, acc);
    __syncthreads();  // every read of mid and dy is done
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = ((wv * 4 + mi) * kImpR1 + 4 * g + r) * LD + ni * 16 + c16;
          L.r1[i] = L.r1[i] > 0.f ? acc[mi][ni][r] : 0.f;  // mid is zero outside the image
        }
    imp_load_region<C>(L.r0, kImpR1, kImpR1, x, C, tl.b, tl.oy - 1, tl.ox - 1, H, W, 1.0f);
    __syncthreads();
    // first convolution: dW0 = d(mid) x relu(x), db0 = sum d(mid), dx = dy + [x > 0] conv0^T
    imp_dw<C, C, kImpR1, 1, true>(L.r1, L.r0, dw0);
    db0 = imp_db<C, kImpR1, 1>(L.r1, db0);
    imp_conv<C, C, kImpR1, 13, false>(L.r1, L.wb, acc);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = wv * 4 + mi, yy = tl.oy + m;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = ni * 16 + c16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 4 * g + r, xx = tl.ox + c;
          if (m < kImpT && c < kImpT && yy < H && xx < W) {
            const int64_t o = ((tl.b * H + yy) * W + xx) * C + n;
            const float xv = L.r0[((m + 1) * kImpR1 + c + 1) * LD + n];
            dx[o] = dy[o] + (xv > 0.f ? acc[mi][ni][r] : 0.f);
          }
        }
      }
    }
    __syncthreads();
  }
  float* o = ws + static_cast<int64_t>(blockIdx.x) * imp_res_params(C);
  imp_dw_store<C, C>(o, C, dw0);
  imp_dw_store<C, C>(o + 9 * C * C + C, C, dw1);
  double* scratch = reinterpret_cast<double*>(L.r0);
  imp_db_store<C>(o + 9 * C * C, db0, scratch);
  imp_db_store<C>(o + 2 * 9 * C * C + C, db1, scratch);
}

// ---- convolution + max-pool -----------------------------------------------------------------------
template <int CI, int CO>
struct ImpCpLds {
  static constexpr int LDI = CI + 4, LDO = CO + 4;
  static constexpr int CNP = CI < 16 ? 16 : CI;  // dx columns, padded to an MFMA tile
  float in[kImpR0 * kImpR0 * LDI];  // fwd: scale x on 18 x 18; bwd: on 16 x 16
  float z[kImpR1 * kImpR1 * LDO];   // fwd: conv + b (-inf outside the image); bwd: dz
  float w[9 * CO * CNP];            // fwd: [tap][ci / 4][co][4]; bwd: transposed, for dx
  float b[CO];
};

template <int CI, int CO>
__global__ __launch_bounds__(kImpThreads) void imp_cp_fwd_kernel(
    const float* __restrict__ x, int64_t B, int H, int W, int cin, const float* __restrict__ w,
    const float* __restrict__ bias, float scale, float* __restrict__ out,
    uint8_t* __restrict__ arg) {
  __shared__ __attribute__((aligned(16))) ImpCpLds<CI, CO> L;
  constexpr int LDO = CO + 4, NT = CO / 16;
  imp_stage_w<CI, CO, false>(L.w, w, cin, CO);
  for (int i = threadIdx.x; i < CO; i += kImpThreads) L.b[i] = bias[i];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
  const int HO = (H + 1) / 2, WO = (W + 1) / 2;
  const int nty = (HO + kImpTP - 1) / kImpTP, ntx = (WO + kImpTP - 1) / kImpTP;
  const int64_t tiles = B * nty * ntx;
  const float ninf = -__builtin_huge_valf();
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const ImpTile tl = imp_tile(t, nty, ntx, kImpTP);  // first pooled output of the tile
    imp_load_region<CI>(L.in, kImpR0, kImpR0, x, cin, tl.b, 2 * tl.oy - 2, 2 * tl.ox - 2, H, W,
                        scale);
    __syncthreads();
    imp_x4 acc[4][NT];
    imp_conv<CI, CO, kImpR0, 15, false>(L.in, L.w, acc);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = wv * 4 + mi, yy = 2 * tl.oy - 1 + m;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = ni * 16 + c16;
        const float bv = L.b[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 4 * g + r, xx = 2 * tl.ox - 1 + c;
          const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
          L.z[(m * kImpR1 + c) * LDO + n] = in ? acc[mi][ni][r] + bv : ninf;
        }
      }
    }
    __syncthreads();
    // pooled output (py, px) of the tile: conv region rows 2 py .. 2 py + 2
    for (int item = threadIdx.x; item < kImpTP * kImpTP * CO; item += kImpThreads) {
      const int pp = item / CO, n = item - pp * CO;
      const int py = pp / kImpTP, px = pp - py * kImpTP;
      const int gy = tl.oy + py, gx = tl.ox + px;
      if (gy < HO && gx < WO) {
        float best = ninf;
        int idx = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const float v = L.z[((2 * py + j / 3) * kImpR1 + 2 * px + j % 3) * LDO + n];
          if (v > best || v != v) {
            best = v;
            idx = j;
          }
        }
        const int64_t o = ((tl.b * HO + gy) * WO + gx) * CO + n;
        out[o] = best;
        if (arg) arg[o] = static_cast<uint8_t>(idx);
      }
    }
    __syncthreads();
  }
}

// Partial row of a workgroup: dW [CO][cin][9], db [CO].
template <int CI, int CO>
__global__ __launch_bounds__(kImpThreads) void imp_cp_bwd_kernel(
    const float* __restrict__ dp, const uint8_t* __restrict__ arg, const float* __restrict__ x,
    int64_t B, int H, int W, int cin, const float* __restrict__ w, float scale,
    float* __restrict__ dx, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) ImpCpLds<CI, CO> L;
  constexpr int LDO = CO + 4, CNP = ImpCpLds<CI, CO>::CNP, NTX = CNP / 16;
  constexpr int NACC = ImpDw<CO, CI>::NACC;
  if (dx) imp_stage_w<CO, CNP, true>(L.w, w, CO, cin);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
  const int HO = (H + 1) / 2, WO = (W + 1) / 2;
  const int nty = (H + kImpT - 1) / kImpT, ntx = (W + kImpT - 1) / kImpT;
  const int64_t tiles = B * nty * ntx;
  imp_x4 dw[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) dw[i] = imp_x4{0.f, 0.f, 0.f, 0.f};
  double db = 0.0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const ImpTile tl = imp_tile(t, nty, ntx, kImpT);  // first owned conv position
    imp_load_region<CI>(L.in, kImpR1, kImpR1, x, cin, tl.b, tl.oy - 1, tl.ox - 1, H, W, scale);
    // dz at a conv position: dp of every pooled output whose maximum it is, in (py, px) order
    for (int item = threadIdx.x; item < kImpR1 * kImpR1 * CO; item += kImpThreads) {
      const int pos = item / CO, n = item - pos * CO;
      const int m = pos / kImpR1, c = pos - m * kImpR1;
      const int yy = tl.oy - 1 + m, xx = tl.ox - 1 + c;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const int npy = (yy & 1) ? 2 : 1, npx = (xx & 1) ? 2 : 1;
        for (int iy = 0; iy < npy; ++iy) {
          const int py = (yy >> 1) + iy;
          if (py >= HO) continue;
          const int wy = yy - (2 * py - 1);
          for (int ix = 0; ix < npx; ++ix) {
            const int px = (xx >> 1) + ix;
            if (px >= WO) continue;
            const int wx = xx - (2 * px - 1);
            const int64_t o = ((tl.b * HO + py) * WO + px) * CO + n;
            if (arg[o] == wy * 3 + wx) v += dp[o];
          }
        }
      }
      L.z[pos * LDO + n] = v;
    }
    __syncthreads();
    imp_dw<CO, CI, kImpR1, 1, false>(L.z, L.in, dw);
    db = imp_db<CO, kImpR1, 1>(L.z, db);
    if (dx) {
      imp_x4 acc[4][NTX];
      imp_conv<CO, CNP, kImpR1, 13, false>(L.z, L.w, acc);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int m = wv * 4 + mi, yy = tl.oy + m;
#pragma unroll
        for (int ni = 0; ni < NTX; ++ni) {
          const int n = ni * 16 + c16;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 4 * g + r, xx = tl.ox + c;
            if (m < kImpT && c < kImpT && yy < H && xx < W && n < cin)
              dx[((tl.b * H + yy) * W + xx) * cin + n] = acc[mi][ni][r] * scale;
          }
        }
      }
    }
    __syncthreads();
  }
  float* o = ws + static_cast<int64_t>(blockIdx.x) * (9 * CO * cin + CO);
  imp_dw_store<CO, CI>(o, cin, dw);
  imp_db_store<CO>(o + 9 * CO * cin, db, reinterpret_cast<double*>(L.in));
}

// Parameter i of the concatenated row = partial rows 0 .. nparts - 1 added in that order; the
// row is up to four tensors one after another.
struct ImpOut {
  float* p[4];
  int n[4];
};

__global__ __launch_bounds__(256) void imp_finish_kernel(const float* __restrict__ ws, int nparts,
                                                         int P, ImpOut out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float a = 0.f;
  for (int k = 0; k < nparts; ++k) a += ws[static_cast<int64_t>(k) * P + i];
  int j = i;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (j < out.n[s]) {
      out.p[s][j] = a;
      return;
    }
    j -= out.n[s];
  }
}

static int imp_check(const char* who, int64_t B, int64_t H, int64_t W, int64_t cin, int64_t cout) {
  OCPPO_REQUIRE(cout == 16 || cout == 32, "%s: %lld output channels (16 or 32)", who,
                (long long)cout);
  OCPPO_REQUIRE((cin >= 1 && cin <= 4) || cin == 16 || cin == 32,
                "%s: %lld input channels (1 .. 4, 16 or 32)", who, (long long)cin);
  OCPPO_REQUIRE(B >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 &&
                    B <= (int64_t(1) << 40) / (H * W * 32),
                "%s: bad sizes B=%lld H=%lld W=%lld", who, (long long)B, (long long)H,
                (long long)W);
  return OCPPO_OK;
}

static bool imp_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static unsigned imp_grid(int64_t B, int64_t H, int64_t W, int T) {
  const int64_t tiles = B * ceil_div(H, T) * ceil_div(W, T);
  return static_cast<unsigned>(tiles < kImpGrid ? tiles : kImpGrid);
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_impala_workspace_bytes(int64_t cin, int64_t cout, int resblock) {
  if (cout != 16 && cout != 32) return 0;
  if (resblock)
    return cin == cout ? static_cast<size_t>(kImpGrid) * imp_res_params(static_cast<int>(cout)) *
                             sizeof(float)
                       : 0;
  if (!((cin >= 1 && cin <= 4) || cin == 16 || cin == 32)) return 0;
  return static_cast<size_t>(kImpGrid) * (9 * cout * cin + cout) * sizeof(float);
}

extern "C" int ocppo_impala_resblock_fwd(ocppo_stream_t stream, const float* x, int64_t B,
                                         int64_t H, int64_t W, int64_t C, const float* w0,
                                         const float* b0, const float* w1, const float* b1,
                                         float* y, float* mid) {
  if (int rc = imp_check("ocppo_impala_resblock_fwd", B, H, W, C, C)) return rc;
  OCPPO_REQUIRE(C == 16 || C == 32, "ocppo_impala_resblock_fwd: C=%lld (16 or 32)", (long long)C);
  OCPPO_REQUIRE(x && w0 && b0 && w1 && b1 && y, "ocppo_impala_resblock_fwd: null pointer");
  OCPPO_REQUIRE(imp_aligned(x), "ocppo_impala_resblock_fwd: x must be 16-byte aligned");
  const unsigned grid = imp_grid(B, H, W, kImpT);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  const int h = static_cast<int>(H), w = static_cast<int>(W);
  if (C == 32)
    hipLaunchKernelGGL((imp_res_fwd_kernel<32>), dim3(grid), dim3(kImpThreads), 0, st, x, B, h, w,
                       w0, b0, w1, b1, y, mid);
  else
    hipLaunchKernelGGL((imp_res_fwd_kernel<16>), dim3(grid), dim3(kImpThreads), 0, st, x, B, h, w,
                       w0, b0, w1, b1, y, mid);
  return check_launch("ocppo_impala_resblock_fwd");
}

extern "C" int ocppo_impala_resblock_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                         const float* mid, int64_t B, int64_t H, int64_t W,
                                         int64_t C, const float* w0, const float* w1, float* dx,
                                         float* dw0, float* db0, float* dw1, float* db1,
                                         void* workspace, size_t workspace_bytes) {
  if (int rc = imp_check("ocppo_impala_resblock_bwd", B, H, W, C, C)) return rc;
  OCPPO_REQUIRE(C == 16 || C == 32, "ocppo_impala_resblock_bwd: C=%lld (16 or 32)", (long long)C);
  OCPPO_REQUIRE(dy && x && mid && w0 && w1 && dx && dw0 && db0 && dw1 && db1,
                "ocppo_impala_resblock_bwd: null pointer");
  OCPPO_REQUIRE(imp_aligned(dy) && imp_aligned(x) && imp_aligned(mid),
                "ocppo_impala_resblock_bwd: dy, x and mid must be 16-byte aligned");
  if (!workspace || workspace_bytes < ocppo_impala_workspace_bytes(C, C, 1) ||
      reinterpret_cast<uintptr_t>(workspace) % 4)
    return fail(OCPPO_E_WORKSPACE, "ocppo_impala_resblock_bwd: workspace of %zu bytes needed",
                ocppo_impala_workspace_bytes(C, C, 1));
  const unsigned grid = imp_grid(B, H, W, kImpT);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  const int h = static_cast<int>(H), w = static_cast<int>(W);
  if (C == 32)
    hipLaunchKernelGGL((imp_res_bwd_kernel<32>), dim3(grid), dim3(kImpThreads), 0, st, dy, x, mid,
                       B, h, w, w0, w1, dx, ws);
  else
    hipLaunchKernelGGL((imp_res_bwd_kernel<16>), dim3(grid), dim3(kImpThreads), 0, st, dy, x, mid,
                       B, h, w, w0, w1, dx, ws);
  if (int rc = check_launch("ocppo_impala_resblock_bwd")) return rc;
  const int c = static_cast<int>(C), P = imp_res_params(c);
  const ImpOut out{{dw0, db0, dw1, db1}, {9 * c * c, c, 9 * c * c, c}};
  hipLaunchKernelGGL(imp_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, st, ws,
                     static_cast<int>(grid), P, out);
  return check_launch("ocppo_impala_resblock_bwd (finish)");
}

#define OCPPO_IMP_CP_DISPATCH(LAUNCH)            \
  do {                                           \
    if (cin <= 4 && cout == 16) LAUNCH(4, 16);   \
    else if (cin <= 4) LAUNCH(4, 32);            \
    else if (cin == 16 && cout == 16) LAUNCH(16, 16); \
    else if (cin == 16) LAUNCH(16, 32);          \
    else if (cout == 16) LAUNCH(32, 16);         \
    else LAUNCH(32, 32);                         \
  } while (0)

extern "C" int ocppo_impala_conv_pool_fwd(ocppo_stream_t stream, const float* x, int64_t B,
                                          int64_t H, int64_t W, int64_t cin, int64_t cout,
                                          const float* w, const float* b, float scale, float* out,
                                          uint8_t* arg) {
  if (int rc = imp_check("ocppo_impala_conv_pool_fwd", B, H, W, cin, cout)) return rc;
  OCPPO_REQUIRE(x && w && b && out, "ocppo_impala_conv_pool_fwd: null pointer");
  OCPPO_REQUIRE(imp_aligned(x), "ocppo_impala_conv_pool_fwd: x must be 16-byte aligned");
  OCPPO_REQUIRE(scale > 0.f && scale <= 3.0e38f, "ocppo_impala_conv_pool_fwd: scale must be > 0");
  const unsigned grid = imp_grid(B, (H + 1) / 2, (W + 1) / 2, kImpTP);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  const int h = static_cast<int>(H), wd = static_cast<int>(W), ci = static_cast<int>(cin);
#define OCPPO_IMP_CP_FWD(CI, CO)                                                                  \
  hipLaunchKernelGGL((imp_cp_fwd_kernel<CI, CO>), dim3(grid), dim3(kImpThreads), 0, st, x, B, h, \
                     wd, ci, w, b, scale, out, arg)
  OCPPO_IMP_CP_DISPATCH(OCPPO_IMP_CP_FWD);
#undef OCPPO_IMP_CP_FWD
  return check_launch("ocppo_impala_conv_pool_fwd");
}

extern "C" int ocppo_impala_conv_pool_bwd(ocppo_stream_t stream, const float* dp,
                                          const uint8_t* arg, const float* x, int64_t B, int64_t H,
                                          int64_t W, int64_t cin, int64_t cout, const float* w,
                                          float scale, float* dx, float* dw, float* db,
                                          void* workspace, size_t workspace_bytes) {
  if (int rc = imp_check("ocppo_impala_conv_pool_bwd", B, H, W, cin, cout)) return rc;
  OCPPO_REQUIRE(dp && arg && x && w && dw && db, "ocppo_impala_conv_pool_bwd: null pointer");
  OCPPO_REQUIRE(imp_aligned(x), "ocppo_impala_conv_pool_bwd: x must be 16-byte aligned");
  OCPPO_REQUIRE(scale > 0.f && scale <= 3.0e38f, "ocppo_impala_conv_pool_bwd: scale must be > 0");
  if (!workspace || workspace_bytes < ocppo_impala_workspace_bytes(cin, cout, 0) ||
      reinterpret_cast<uintptr_t>(workspace) % 4)
    return fail(OCPPO_E_WORKSPACE, "ocppo_impala_conv_pool_bwd: workspace of %zu bytes needed",
                ocppo_impala_workspace_bytes(cin, cout, 0));
  const unsigned grid = imp_grid(B, H, W, kImpT);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  const int h = static_cast<int>(H), wd = static_cast<int>(W), ci = static_cast<int>(cin);
#define OCPPO_IMP_CP_BWD(CI, CO)                                                                   \
  hipLaunchKernelGGL((imp_cp_bwd_kernel<CI, CO>), dim3(grid), dim3(kImpThreads), 0, st, dp, arg, x, \
                     B, h, wd, ci, w, scale, dx, ws)
  OCPPO_IMP_CP_DISPATCH(OCPPO_IMP_CP_BWD);
#undef OCPPO_IMP_CP_BWD
  if (int rc = check_launch("ocppo_impala_conv_pool_bwd")) return rc;
  const int co = static_cast<int>(cout), P = 9 * co * ci + co;
  const ImpOut out{{dw, db, nullptr, nullptr}, {9 * co * ci, co, 0, 0}};
  hipLaunchKernelGGL(imp_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, st, ws,
                     static_cast<int>(grid), P, out);
  return check_launch("ocppo_impala_conv_pool_bwd (finish)");
}
