// The pixel RND body (cleanrl/ppo_rnd_envpool.py:193-219): Conv2d(1, 32, 8, 4), Conv2d(32, 64, 4, 2),
// Conv2d(64, 64, 3, 1), each followed by LeakyReLU(0.01), then nn.Flatten, on the normalised newest
// 84 x 84 frame. Forward of one or two networks in one launch; backward of one network (weight and
// bias gradients only: the frame needs no gradient) in three.
//
// Everything is an implicit GEMM on v_mfma_f32_16x16x4_f32 whose A operand is gathered from LDS and
// whose B operand is read straight from torch's [Cout][Cin][KH][KW] weight memory (there is no
// derived weight copy): lane (i = lane & 15, g = lane >> 4) supplies A[i][4 kb + g] and
// B[4 kb + g][i] of k-step kb, and holds D[4 g + r][i], r = 0 .. 3. Activations sit in LDS
// channel-major ([channel][pixel]), so the M index (a pixel) is the fast one of an A gather and a
// lane's four D rows are one 16-byte LDS store.
//
// Forward, one workgroup (4 waves) per image. The loader normalises the u8 frame into LDS once with
// ocppo_rnd_normalize's arithmetic; every network runs from that copy:
//   layer 1: M = 400 pixels (25 tiles), N = 32, K = 64;  wave = (N tile, M tile parity), 13 tiles
//   layer 2: M = 81 -> 96 (6 tiles),    N = 64, K = 512; wave = N tile, 6 M tiles
//   layer 3: M = 49 -> 64 (4 tiles),    N = 64, K = 576; wave = N tile, 4 M tiles
// Rows past the last pixel gather the last pixel (finite data) and are not stored as results. The
// B values of the next eight k-steps are fetched while the current eight multiply.
// LDS: a1 [32][400] 51,200 B + frame 28,224 B; a2 [64][96] 24,576 B lies over the frame with one
// network (the frame is dead after layer 1): 79,424 B, two workgroups per CU; with two networks the
// frame has to survive the first one, a2 gets its own region: 104,000 B, one workgroup per CU (the
// two-network call is the rollout's, with fewer images than CUs).
//
// Backward. Stage A, one workgroup per image, the data-gradient chain in LDS:
//   dz3 = dout * leaky'(a3), zero-padded by 2 into [64][11 x 11];
//   dz2 = conv3^T(dz3) * leaky'(a2): M = 81, N = 64, K = (co, ky, kx) = 576, zero-padded by 1 into
//         [64][11 x 11];
//   dz1 = conv2^T(dz2) * leaky'(a1): the stride-2 transposed convolution split by output parity
//         (y & 1, x & 1): a pixel of one parity meets only the 2 x 2 taps of that parity, so each
//         class is M = 100 -> 112, N = 32, K = (co, u, v) = 256 with no multiplication by an
//         inserted zero. wave = (N tile, two parity classes).
// dz1 / dz2 / dz3 go to the workspace. Stage B, grid (chunks of OCPPO_RND_BODY_CHUNK images, 9
// parts): dW_l = dz_l^T im2col(a_{l-1}) with M = output channel, N = a 16-wide slice of K, the
// MFMA's k the pixels. Parts 0-3 own 128 columns of dW2 each (8 input channels), parts 4-7 144
// columns of dW3 (16 input channels), part 8 dW1 (its operand re-normalised from the u8 frames).
// A part stages per image only what it reads, sums one image's products in a fresh accumulator and
// adds that to the chunk's (two-level: no f32 chain is longer than one image's pixels plus the
// chunk's images), all in registers, and stores the chunk's once, plainly; bias gradients are f64
// sums over a fixed split of the pixels. The finish launch adds the chunks' partial rows in chunk
// order. No atomics anywhere.
#include "ocppo_common.h"

namespace ocppo {

typedef float rb_x4 __attribute__((ext_vector_type(4)));

constexpr int kRbThreads = 256;
constexpr int kRbFrame = 84 * 84;
constexpr int kRbA1 = 32 * 400, kRbA2 = 64 * 81, kRbA3 = 64 * 49;
constexpr int kRbLd2 = 96;     // LDS pixel stride of a2
constexpr int kRbPad = 121;    // 11 x 11: a zero-padded dz plane
constexpr int kRbChunk = OCPPO_RND_BODY_CHUNK;
// a chunk's partial row: dW1 [32][64], db1 [32], dW2 [64][512], db2 [64], dW3 [64][576], db3 [64]
constexpr int kRbOffB1 = 2048, kRbOffW2 = 2080, kRbOffB2 = kRbOffW2 + 32768;
constexpr int kRbOffW3 = kRbOffB2 + 64, kRbOffB3 = kRbOffW3 + 36864, kRbParams = kRbOffB3 + 64;

__device__ __forceinline__ float rb_leaky(float v) { return v > 0.f ? v : v * 0.01f; }
// gradient through LeakyReLU at output a (sign(a) = sign(pre-activation); 0 takes the slope)
__device__ __forceinline__ float rb_dleaky(float a, float gr) { return a > 0.f ? gr : gr * 0.01f; }

// ---- the GEMM operands of every layer: A = in[base(pixel) + koff(k)], B = w[waddr(k, n)] --------
struct RbL1 {  // frame [84 x 84] -> 20 x 20, k = (ky, kx) of 8 x 8, stride 4
  static constexpr int K = 64, NPIX = 400;
  __device__ static int base(int p) { const int oy = p / 20; return 336 * oy + 4 * (p - 20 * oy); }
  __device__ static int koff(int k) { return (k >> 3) * 84 + (k & 7); }
  __device__ int waddr(int k, int n) const { return n * K + k; }
};
struct RbL2 {  // a1 [c][20 x 20] -> 9 x 9, k = (c, ky, kx) of 4 x 4, stride 2
  static constexpr int K = 512, NPIX = 81;
  __device__ static int base(int p) { const int oy = p / 9; return 40 * oy + 2 * (p - 9 * oy); }
  __device__ static int koff(int k) { return (k >> 4) * 400 + ((k >> 2) & 3) * 20 + (k & 3); }
  __device__ int waddr(int k, int n) const { return n * K + k; }
};
struct RbL3 {  // a2 [c][96] (9 x 9) -> 7 x 7, k = (c, ky, kx) of 3 x 3
  static constexpr int K = 576, NPIX = 49;
  __device__ static int base(int p) { const int oy = p / 7; return 9 * oy + (p - 7 * oy); }
  __device__ static int koff(int k) {
    const int c = k / 9, t = k - 9 * c, ty = t / 3;
    return c * kRbLd2 + ty * 9 + (t - 3 * ty);
  }
  __device__ int waddr(int k, int n) const { return n * K + k; }
};
struct RbT3 {  // dz3 padded by 2 [co][11 x 11] -> da2 9 x 9, k = (co, ky, kx), n = c
  static constexpr int K = 576, NPIX = 81;
  __device__ static int base(int p) { const int y = p / 9; return (y + 2) * 11 + (p - 9 * y) + 2; }
  __device__ static int koff(int k) {
    const int co = k / 9, t = k - 9 * co, ty = t / 3;
    return co * kRbPad - ty * 11 - (t - 3 * ty);
  }
  __device__ int waddr(int k, int n) const { return (k / 9) * 576 + n * 9 + k % 9; }
};
struct RbT2 {  // dz2 padded by 1 [co][11 x 11] -> da1 pixels (2 a + py, 2 b + px), k = (co, u, v)
  static constexpr int K = 256, NPIX = 100;
  int py, px;
  __device__ static int base(int q) { const int a = q / 10; return (a + 1) * 11 + (q - 10 * a) + 1; }
  __device__ static int koff(int k) { return (k >> 2) * kRbPad - ((k >> 1) & 1) * 11 - (k & 1); }
  __device__ int waddr(int k, int n) const {
    return ((k >> 2) * 32 + n) * 16 + (py + 2 * ((k >> 1) & 1)) * 4 + px + 2 * (k & 1);
  }
};

// acc[mi] = M tile mt0 + mi * mts (16 pixels; past NPIX: the last pixel again), columns n's tile
template <class L, int MT>
__device__ __forceinline__ void rb_gemm(const L l, const float* __restrict__ in,
                                        const float* __restrict__ w, int n, int mt0, int mts,
                                        rb_x4 (&acc)[MT]) {
  constexpr int U = 8, KB = L::K / 4;
  static_assert(KB % U == 0, "k-steps per prefetch block");
  const int lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
  int base[MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const int p = (mt0 + mi * mts) * 16 + i16;
    base[mi] = L::base(p < L::NPIX ? p : L::NPIX - 1);
    acc[mi] = rb_x4{0.f, 0.f, 0.f, 0.f};
  }
  float b[U], bn[U];
#pragma unroll
  for (int u = 0; u < U; ++u) b[u] = w[l.waddr(4 * u + g, n)];
#pragma unroll 1
  for (int kb = 0; kb < KB; kb += U) {
    const bool more = kb + U < KB;
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) bn[u] = w[l.waddr(4 * (kb + U + u) + g, n)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ko = L::koff(4 * (kb + u) + g);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(in[base[mi] + ko], b[u], acc[mi], 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) b[u] = bn[u];
    }
  }
}

// The frame of image r normalised into LDS: f32(clip((f64(x) - mean) / sqrt(var), -5, 5)), a NaN
// kept (ocppo_rnd_normalize's arithmetic). An index outside [0, src_rows) reads nothing and gives a
// NaN frame, which every output of the image then shows.
__device__ __forceinline__ void rb_load_frame(float* __restrict__ fr,
                                              const uint8_t* __restrict__ frames,
                                              int64_t src_rows, int64_t row_stride,
                                              const int64_t* __restrict__ idx, int64_t r,
                                              const double* __restrict__ state) {
  const int64_t row = idx ? idx[r] : r;
  const bool ok = row >= 0 && row < src_rows;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(frames + (ok ? row : 0) * row_stride);
  for (int i = threadIdx.x; i < kRbFrame / 4; i += kRbThreads) {
    const uint32_t x = src[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * i + k;
      double v = (static_cast<double>(static_cast<float>((x >> (8 * k)) & 0xFFu)) - state[c]) /
                 sqrt(state[kRbFrame + c]);
      v = v != v ? v : fmin(fmax(v, -5.0), 5.0);
      fr[c] = ok ? static_cast<float>(v) : __builtin_nanf("");
    }
  }
}

struct RbNet {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};

// ---- forward ------------------------------------------------------------------------------------
template <int NETS>
__global__ __launch_bounds__(kRbThreads) void rb_fwd_kernel(
    const uint8_t* __restrict__ frames, int64_t src_rows, int64_t row_stride,
    const int64_t* __restrict__ idx, const double* __restrict__ state, RbNet net0, RbNet net1,
    float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ a1s,
    float* __restrict__ a2s) {
  __shared__ __attribute__((aligned(16))) float lds[kRbA1 + kRbFrame + (NETS - 1) * 64 * kRbLd2];
  float* a1 = lds;
  float* fr = lds + kRbA1;
  float* a2 = NETS == 1 ? fr : fr + kRbFrame;
  const int64_t r = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i16 = lane & 15, g = lane >> 4;
  rb_load_frame(fr, frames, src_rows, row_stride, idx, r, state);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < NETS; ++s) {
    const RbNet net = s ? net1 : net0;
    float* out = s ? out1 : out0;
    {
      rb_x4 acc[13];
      const int ch = (wv & 1) * 16 + i16;
      rb_gemm<RbL1, 13>(RbL1{}, fr, net.w1, ch, wv >> 1, 2, acc);
      const float bv = net.b1[ch];
#pragma unroll
      for (int mi = 0; mi < 13; ++mi) {
        const int mt = (wv >> 1) + 2 * mi;
        if (mt < 25)
          *reinterpret_cast<float4*>(&a1[ch * 400 + 16 * mt + 4 * g]) =
              make_float4(rb_leaky(acc[mi][0] + bv), rb_leaky(acc[mi][1] + bv),
                          rb_leaky(acc[mi][2] + bv), rb_leaky(acc[mi][3] + bv));
      }
    }
    __syncthreads();  // a1 is whole; with one network a2 may now overwrite the frame
    if (a1s && s == 0) {
      float4* o = reinterpret_cast<float4*>(a1s + r * kRbA1);
      for (int i = threadIdx.x; i < kRbA1 / 4; i += kRbThreads)
        o[i] = reinterpret_cast<const float4*>(a1)[i];
    }
    {
      rb_x4 acc[6];
      const int ch = wv * 16 + i16;
      rb_gemm<RbL2, 6>(RbL2{}, a1, net.w2, ch, 0, 1, acc);
      const float bv = net.b2[ch];
#pragma unroll
      for (int mi = 0; mi < 6; ++mi)  // rows 81 .. 95 hold copies of pixel 80: never read
        *reinterpret_cast<float4*>(&a2[ch * kRbLd2 + 16 * mi + 4 * g]) =
            make_float4(rb_leaky(acc[mi][0] + bv), rb_leaky(acc[mi][1] + bv),
                        rb_leaky(acc[mi][2] + bv), rb_leaky(acc[mi][3] + bv));
    }
    __syncthreads();
    if (a2s && s == 0) {
      for (int i = threadIdx.x; i < kRbA2; i += kRbThreads) {
        const int c = i / 81;
        a2s[r * kRbA2 + i] = a2[c * kRbLd2 + (i - 81 * c)];
      }
    }
    {
      rb_x4 acc[4];
      const int ch = wv * 16 + i16;
      rb_gemm<RbL3, 4>(RbL3{}, a2, net.w3, ch, 0, 1, acc);
      const float bv = net.b3[ch];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = 16 * mi + 4 * g + q;
          if (p < 49) out[r * kRbA3 + ch * 49 + p] = rb_leaky(acc[mi][q] + bv);
        }
    }
    // the next network writes a1 (last read before the barrier above) and, after its own
    // barrier, a2: every wave has left this network's layer 3 by then
  }
}

// ---- backward, stage A: dz3, dz2, dz1 of one image ----------------------------------------------
__global__ __launch_bounds__(kRbThreads) void rb_bwd_data_kernel(
    const float* __restrict__ dout, const float* __restrict__ a1, const float* __restrict__ a2,
    const float* __restrict__ a3, const float* __restrict__ w2, const float* __restrict__ w3,
    float* __restrict__ dz1, float* __restrict__ dz2, float* __restrict__ dz3) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 64 * kRbPad];
  float* z3p = lds;
  float* z2p = lds + 64 * kRbPad;
  const int64_t r = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i16 = lane & 15, g = lane >> 4;
  for (int i = threadIdx.x; i < 2 * 64 * kRbPad; i += kRbThreads) lds[i] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < kRbA3; i += kRbThreads) {
    const int c = i / 49, p = i - 49 * c, y = p / 7;
    const float v = rb_dleaky(a3[r * kRbA3 + i], dout[r * kRbA3 + i]);
    dz3[r * kRbA3 + i] = v;
    z3p[c * kRbPad + (y + 2) * 11 + (p - 7 * y) + 2] = v;
  }
  __syncthreads();
  {
    rb_x4 acc[6];
    const int ch = wv * 16 + i16;
    rb_gemm<RbT3, 6>(RbT3{}, z3p, w3, ch, 0, 1, acc);
#pragma unroll
    for (int mi = 0; mi < 6; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = 16 * mi + 4 * g + q;
        if (p < 81) {
          const int64_t o = r * kRbA2 + ch * 81 + p;
          const float v = rb_dleaky(a2[o], acc[mi][q]);
          const int y = p / 9;
          dz2[o] = v;
          z2p[ch * kRbPad + (y + 1) * 11 + (p - 9 * y) + 1] = v;
        }
      }
  }
  __syncthreads();
  const int ch = (wv & 1) * 16 + i16;
#pragma unroll 1
  for (int pp = 0; pp < 2; ++pp) {
    const int par = 2 * (wv >> 1) + pp, py = par >> 1, px = par & 1;
    rb_x4 acc[7];
    rb_gemm<RbT2, 7>(RbT2{py, px}, z2p, w2, ch, 0, 1, acc);
#pragma unroll
    for (int mi = 0; mi < 7; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = 16 * mi + 4 * g + q;
        if (p < 100) {
          const int a = p / 10;
          const int64_t o = r * kRbA1 + ch * 400 + (2 * a + py) * 20 + 2 * (p - 10 * a) + px;
          dz1[o] = rb_dleaky(a1[o], acc[mi][q]);
        }
      }
  }
}

// ---- backward, stage B: the weight and bias gradients of a chunk of images --------------------
// dz rows [C][P] of image r into LDS as [C][LD], LD >= P a multiple of 4, zero past P
template <int C, int P, int LD>
__device__ __forceinline__ void rb_stage_dz(float* __restrict__ z, const float* __restrict__ src) {
  for (int i = threadIdx.x; i < C * LD; i += kRbThreads) {
    const int n = i / LD, p = i - LD * n;
    z[i] = p < P ? src[n * P + p] : 0.f;
  }
}

// f64 sum of channel tid % C over pixels tid / C, + G, ... (G = 256 / C groups)
template <int C, int P, int LD>
__device__ __forceinline__ double rb_db(const float* __restrict__ z, double a) {
  constexpr int G = kRbThreads / C;
  const int n = threadIdx.x % C;
  for (int p = threadIdx.x / C; p < P; p += G) a += static_cast<double>(z[n * LD + p]);
  return a;
}

// the groups' sums of a channel added in group order; scratch: 256 doubles
template <int C>
__device__ __forceinline__ void rb_db_store(float* __restrict__ o, double a, double* scratch) {
  __syncthreads();
  scratch[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < C) {
    double s = 0.0;
    for (int k = 0; k < kRbThreads / C; ++k) s += scratch[k * C + threadIdx.x];
    o[threadIdx.x] = static_cast<float>(s);
  }
}

__global__ __launch_bounds__(kRbThreads) void rb_bwd_w_kernel(
    const uint8_t* __restrict__ frames, int64_t src_rows, int64_t row_stride,
    const int64_t* __restrict__ idx, const double* __restrict__ state,
    const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ dz1,
    const float* __restrict__ dz2, const float* __restrict__ dz3, int64_t R,
    float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float lds[kRbA1 + kRbFrame];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, i16 = lane & 15, g = lane >> 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kRbChunk;
  const int64_t r1 = r0 + kRbChunk < R ? r0 + kRbChunk : R;
  const int pt = blockIdx.y;
  float* o = part + static_cast<int64_t>(blockIdx.x) * kRbParams;
  double db = 0.0;
  if (pt < 4) {  // dW2 columns 128 pt .. + 127: input channels 8 pt .. + 7
    constexpr int LD = 84;
    float* z = lds;            // [64][84]
    float* act = lds + 64 * LD;  // [8][400]
    rb_x4 acc[4][2];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt][0] = acc[nt][1] = rb_x4{0.f, 0.f, 0.f, 0.f};
    const int ko0 = RbL2::koff(32 * wv + i16), ko1 = RbL2::koff(32 * wv + 16 + i16);
    for (int64_t r = r0; r < r1; ++r) {
      __syncthreads();
      rb_stage_dz<64, 81, LD>(z, dz2 + r * kRbA2);
      const float4* s4 = reinterpret_cast<const float4*>(a1 + r * kRbA1 + pt * 3200);
      for (int i = threadIdx.x; i < 800; i += kRbThreads) reinterpret_cast<float4*>(act)[i] = s4[i];
      __syncthreads();
      rb_x4 im[4][2];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) im[nt][0] = im[nt][1] = rb_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 3
      for (int s = 0; s < LD / 4; ++s) {
        const int p = 4 * s + g, bb = RbL2::base(p < 81 ? p : 80);
        const float b0 = act[bb + ko0], b1 = act[bb + ko1];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float a = z[(nt * 16 + i16) * LD + p];
          im[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, im[nt][0], 0, 0, 0);
          im[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, im[nt][1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        acc[nt][0] += im[nt][0];
        acc[nt][1] += im[nt][1];
      }
      if (pt == 0) db = rb_db<64, 81, LD>(z, db);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[kRbOffW2 + (nt * 16 + 4 * g + q) * 512 + 128 * pt + 32 * wv + 16 * j + i16] =
              acc[nt][j][q];
    if (pt == 0) rb_db_store<64>(o + kRbOffB2, db, reinterpret_cast<double*>(lds));
  } else if (pt < 8) {  // dW3 columns 144 (pt - 4) .. + 143: input channels 16 (pt - 4) .. + 15
    constexpr int LD = 52;
    const int q4 = pt - 4;
    float* z = lds;              // [64][52]
    float* act = lds + 64 * LD;  // [16][96]
    rb_x4 acc[9];
    int ko[9];
#pragma unroll
    for (int kt = 0; kt < 9; ++kt) {
      acc[kt] = rb_x4{0.f, 0.f, 0.f, 0.f};
      ko[kt] = RbL3::koff(16 * kt + i16);
    }
    for (int64_t r = r0; r < r1; ++r) {
      __syncthreads();
      rb_stage_dz<64, 49, LD>(z, dz3 + r * kRbA3);
      for (int i = threadIdx.x; i < 16 * 81; i += kRbThreads) {
        const int c = i / 81;
        act[c * kRbLd2 + (i - 81 * c)] = a2[r * kRbA2 + q4 * 16 * 81 + i];
      }
      __syncthreads();
      rb_x4 im[9];
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) im[kt] = rb_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int s = 0; s < LD / 4; ++s) {
        const int p = 4 * s + g, bb = RbL3::base(p < 49 ? p : 48);
        const float a = z[(wv * 16 + i16) * LD + p];
#pragma unroll
        for (int kt = 0; kt < 9; ++kt)
          im[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, act[bb + ko[kt]], im[kt], 0, 0, 0);
      }
#pragma unroll
      for (int kt = 0; kt < 9; ++kt) acc[kt] += im[kt];
      if (pt == 4) db = rb_db<64, 49, LD>(z, db);
    }
#pragma unroll
    for (int kt = 0; kt < 9; ++kt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        o[kRbOffW3 + (wv * 16 + 4 * g + q) * 576 + 144 * q4 + 16 * kt + i16] = acc[kt][q];
    if (pt == 4) rb_db_store<64>(o + kRbOffB3, db, reinterpret_cast<double*>(lds));
  } else {  // dW1, its operand the frame normalised again
    float* z = lds;           // [32][400]
    float* fr = lds + kRbA1;  // [84 x 84]
    rb_x4 acc[2];
    acc[0] = acc[1] = rb_x4{0.f, 0.f, 0.f, 0.f};
    const int ko = RbL1::koff(16 * wv + i16);
    for (int64_t r = r0; r < r1; ++r) {
      __syncthreads();
      const float4* s4 = reinterpret_cast<const float4*>(dz1 + r * kRbA1);
      for (int i = threadIdx.x; i < kRbA1 / 4; i += kRbThreads)
        reinterpret_cast<float4*>(z)[i] = s4[i];
      rb_load_frame(fr, frames, src_rows, row_stride, idx, r, state);
      __syncthreads();
      rb_x4 im[2];
      im[0] = im[1] = rb_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int s = 0; s < 100; ++s) {
        const int p = 4 * s + g;
        const float b = fr[RbL1::base(p) + ko];
        im[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(z[i16 * 400 + p], b, im[0], 0, 0, 0);
        im[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(z[(16 + i16) * 400 + p], b, im[1], 0, 0, 0);
      }
      acc[0] += im[0];
      acc[1] += im[1];
      db = rb_db<32, 400, 400>(z, db);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int q = 0; q < 4; ++q) o[(nt * 16 + 4 * g + q) * 64 + 16 * wv + i16] = acc[nt][q];
    rb_db_store<32>(o + kRbOffB1, db, reinterpret_cast<double*>(lds));
  }
}

struct RbOut {
  float* p[6];
};

// parameter i of the row = the chunks' partials added in chunk order
__global__ __launch_bounds__(256) void rb_finish_kernel(const float* __restrict__ part,
                                                        int nchunks, RbOut out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= kRbParams) return;
  float a = 0.f;
  for (int k = 0; k < nchunks; ++k) a += part[static_cast<int64_t>(k) * kRbParams + i];
  constexpr int off[7] = {0, kRbOffB1, kRbOffW2, kRbOffB2, kRbOffW3, kRbOffB3, kRbParams};
#pragma unroll
  for (int s = 0; s < 6; ++s)
    if (i >= off[s] && i < off[s + 1]) out.p[s][i - off[s]] = a;
}

constexpr int64_t kRbMaxR = int64_t(1) << 20;

static int rb_check(const char* who, const void* frames, int64_t src_rows, int64_t row_stride,
                    int64_t R, int64_t H, int64_t W, int64_t c1, int64_t c2, int64_t c3,
                    const double* state) {
  OCPPO_REQUIRE(H == 84 && W == 84 && c1 == 32 && c2 == 64 && c3 == 64,
                "%s: geometry %lld x %lld, channels %lld / %lld / %lld (84 x 84, 32 / 64 / 64 only)",
                who, (long long)H, (long long)W, (long long)c1, (long long)c2, (long long)c3);
  OCPPO_REQUIRE(R >= 1 && R <= kRbMaxR && src_rows >= 1, "%s: bad sizes R=%lld src_rows=%lld", who,
                (long long)R, (long long)src_rows);
  OCPPO_REQUIRE(frames && state, "%s: null pointer", who);
  OCPPO_REQUIRE(row_stride >= kRbFrame && row_stride % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(frames) % 4 == 0,
                "%s: frame rows must be 4-byte aligned and at least %d bytes apart", who, kRbFrame);
  return OCPPO_OK;
}

static bool rb_al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_rnd_body_fwd(ocppo_stream_t stream, const uint8_t* frames, int64_t src_rows,
                                  int64_t row_stride, const int64_t* idx, int64_t R, int64_t H,
                                  int64_t W, int64_t c1, int64_t c2, int64_t c3,
                                  const double* state, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* w3,
                                  const float* b3, const float* tw1, const float* tb1,
                                  const float* tw2, const float* tb2, const float* tw3,
                                  const float* tb3, float* out, float* tout, float* a1, float* a2) {
  if (int rc = rb_check("ocppo_rnd_body_fwd", frames, src_rows, row_stride, R, H, W, c1, c2, c3,
                        state))
    return rc;
  OCPPO_REQUIRE(w1 && b1 && w2 && b2 && w3 && b3 && out, "ocppo_rnd_body_fwd: null pointer");
  const bool two = tw1 || tb1 || tw2 || tb2 || tw3 || tb3 || tout;
  OCPPO_REQUIRE(!two || (tw1 && tb1 && tw2 && tb2 && tw3 && tb3 && tout),
                "ocppo_rnd_body_fwd: the second network needs all six parameters and its output");
  OCPPO_REQUIRE((a1 == nullptr) == (a2 == nullptr) && rb_al16(a1),
                "ocppo_rnd_body_fwd: a1 and a2 come together, a1 16-byte aligned");
  const RbNet n0{w1, b1, w2, b2, w3, b3}, n1{tw1, tb1, tw2, tb2, tw3, tb3};
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  const dim3 grid(static_cast<unsigned>(R));
  if (two)
    hipLaunchKernelGGL(rb_fwd_kernel<2>, grid, dim3(kRbThreads), 0, st, frames, src_rows,
                       row_stride, idx, state, n0, n1, out, tout, a1, a2);
  else
    hipLaunchKernelGGL(rb_fwd_kernel<1>, grid, dim3(kRbThreads), 0, st, frames, src_rows,
                       row_stride, idx, state, n0, n1, out, tout, a1, a2);
  return check_launch("ocppo_rnd_body_fwd");
}

extern "C" size_t ocppo_rnd_body_workspace_bytes(int64_t R) {
  if (R < 1 || R > kRbMaxR) return 0;
  return static_cast<size_t>(R * (kRbA1 + kRbA2 + kRbA3) + ceil_div(R, kRbChunk) * kRbParams) *
         sizeof(float);
}

extern "C" int ocppo_rnd_body_bwd(ocppo_stream_t stream, const uint8_t* frames, int64_t src_rows,
                                  int64_t row_stride, const int64_t* idx, int64_t R, int64_t H,
                                  int64_t W, int64_t c1, int64_t c2, int64_t c3,
                                  const double* state, const float* a1, const float* a2,
                                  const float* a3, const float* w2, const float* w3,
                                  const float* dout, float* dw1, float* db1, float* dw2,
                                  float* db2, float* dw3, float* db3, void* workspace,
                                  size_t workspace_bytes) {
  if (int rc = rb_check("ocppo_rnd_body_bwd", frames, src_rows, row_stride, R, H, W, c1, c2, c3,
                        state))
    return rc;
  OCPPO_REQUIRE(a1 && a2 && a3 && w2 && w3 && dout && dw1 && db1 && dw2 && db2 && dw3 && db3,
                "ocppo_rnd_body_bwd: null pointer");
  OCPPO_REQUIRE(rb_al16(a1), "ocppo_rnd_body_bwd: a1 must be 16-byte aligned");
  if (!workspace || workspace_bytes < ocppo_rnd_body_workspace_bytes(R) || !rb_al16(workspace))
    return fail(OCPPO_E_WORKSPACE, "ocppo_rnd_body_bwd: workspace of %zu bytes needed",
                ocppo_rnd_body_workspace_bytes(R));
  float* dz1 = static_cast<float*>(workspace);
  float* dz2 = dz1 + R * kRbA1;
  float* dz3 = dz2 + R * kRbA2;
  float* part = dz3 + R * kRbA3;
  const int nchunks = static_cast<int>(ceil_div(R, kRbChunk));
  hipStream_t st = as_stream(stream);
  clear_stale_error();
  hipLaunchKernelGGL(rb_bwd_data_kernel, dim3(static_cast<unsigned>(R)), dim3(kRbThreads), 0, st,
                     dout, a1, a2, a3, w2, w3, dz1, dz2, dz3);
  if (int rc = check_launch("ocppo_rnd_body_bwd (data)")) return rc;
  hipLaunchKernelGGL(rb_bwd_w_kernel, dim3(nchunks, 9), dim3(kRbThreads), 0, st, frames, src_rows,
                     row_stride, idx, state, a1, a2, dz1, dz2, dz3, R, part);
  if (int rc = check_launch("ocppo_rnd_body_bwd (weights)")) return rc;
  const RbOut o{{dw1, db1, dw2, db2, dw3, db3}};
  hipLaunchKernelGGL(rb_finish_kernel, dim3((kRbParams + 255) / 256), dim3(256), 0, st, part,
                     nchunks, o);
  return check_launch("ocppo_rnd_body_bwd (finish)");
}
