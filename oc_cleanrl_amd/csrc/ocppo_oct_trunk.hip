// The whole inference forward of the object-set transformer agent's trunk
// (cleanrl/ppo_atari_oc_transformer.py:215-277, oc_cleanrl_amd/transformer.py) as ONE launch:
//   valid[s] = any(x[b, s, :num_obj] != 0)                                  (masking)
//   h = x W_enc^T + b_enc
//   per block (post-norm, dim_feedforward == E, ReLU):
//     q|k|v = h W_in^T + b_in;  a = per-head softmax(q k^T / sqrt(dh)) v over the valid keys
//     h = LN1(h + a W_out^T + b_out);  h = LN2(h + W_2 relu(W_1 h + b_1) + b_2)
//   masking: h = relu(h W_p^T + b_p) per post layer;  hidden = pool(h, valid)
// x [B, S, F] -> hidden [B, E]. Forward only, f32 (exact f32 products, f32 accumulation), no
// dropout, no atomics, no exchange between workgroups: attention mixes tokens only inside one
// sample, so a group of whole samples goes through the entire depth in one workgroup and the
// activations never leave the chip.
//
// Work split: a 512-thread workgroup (8 waves) owns G = max(1, ROWS / S) whole samples, ROWS in
// {16, 32, 64} token rows chosen per launch (oct_tile_rows). Rows of the tile beyond G * S and
// samples past B are zeros on the way in, ride through the products of their 16-row tile (every
// product here is row-wise: nothing crosses rows), are skipped by attention, LayerNorm and pooling
// and are never written out.
//
// LDS: the token tile h [ROWS, E] (row stride E + 4) and a scratch tile [ROWS, 3E] (row stride
// 3E + 4) that holds in turn the staged input rows, q|k|v, the attention output (over q), the
// FFN's hidden and every other post layer's output; + valid [ROWS]. 64 rows at E = 128:
// 133,376 B of the CU's 160 KB. Both strides are 4 mod 32 at E a multiple of 32, the row form of
// ocppo_vit_ffn.hip: conflict-free MFMA A-operand reads.
//
// Linears (v_mfma_f32_16x16x4_f32, the operand idiom of ocppo_vit_ffn.hip): wave w owns the
// output column tiles n = w, w + 8, ... (16 columns each) for all the row tiles. Its B operand is
// the 16 rows of the weight in their native [out, in] layout, read once per workgroup from global
// memory (L2) as K / 16 float4 per lane, ALL in flight at once, and the next column tile's slice is
// requested before the current one's MFMAs: a Linear costs about one L2 round trip per wave, not
// one per k-chunk. The [., E] weights are 16-byte aligned (the contract). The encoder Linear, whose
// K = F has any residue (F = 11), takes scalar weight loads with a clamped column index instead.
// Bias, ReLU and the residual add are epilogues on the accumulators; LayerNorm (biased variance
// about the mean, the module's eps) runs in place on the token tile, a wave per row.
//
// Attention stays rows-in-lanes on the VALU (ocppo_attn.hip's walk and the reasons given there),
// but a lane owns one (token row, head) pair of the tile, so 64 rows x 8 heads fill the 512 lanes
// at S = 8 where a wave per (sample, head) would leave 56 of 64 idle. The lane holds its query row
// in registers and walks the keys of its sample in LDS; lanes of one (sample, head) read the same
// K / V row (a broadcast), but a wave spans 64 / S samples of one head, whose K / V rows lie
// S * LDQ floats apart: per read 64 / S distinct addresses, not one. S * LDQ is 4 S mod 32 banks,
// 0 at S = 8 and 16: those addresses share their banks and the read is serialised 64 / S ways
// (conflicts the wave per (sample, head) form would not have; the price of the filled lanes).
// Excluded keys are skipped: the exact weight 0. The output overwrites the lane's own q slot,
// which nobody else reads.
//
// Parameter pointers travel by value in the kernel argument (OctParams: blocks <= 8, post layers
// <= 4): there is no device-side table that a captured graph could find stale.
#include <math.h>

#include "ocppo_attn_rows.h"
#include "ocppo_common.h"

namespace ocppo {

constexpr int kOctThreads = 512;
constexpr int kOctWaves = kOctThreads / kWave;
constexpr int kOctMaxE = 128, kOctMaxS = 64, kOctMaxF = 64, kOctMaxRows = 64;
constexpr int kOctMaxBlocks = OCPPO_OCT_MAX_BLOCKS, kOctMaxPost = OCPPO_OCT_MAX_POST;
constexpr int kOctKT = kOctMaxE / 16;      // k-chunks of a weight slice held in registers
constexpr int kOctLayerPtrs = 12;          // pointers per block in the host array

typedef float oct_x4 __attribute__((ext_vector_type(4)));

// The host array of ocppo_oct_trunk_fwd as it stands: encoder weight, bias; 12 pointers per block
// (in_proj w, b, out_proj w, b, norm1 w, b, linear1 w, b, linear2 w, b, norm2 w, b); weight, bias
// per post layer. eps: norm1, norm2 per block.
constexpr int kOctMaxPtrs = 2 + kOctLayerPtrs * kOctMaxBlocks + 2 * kOctMaxPost;
struct OctParams {
  const float* p[kOctMaxPtrs];
  float eps[2 * kOctMaxBlocks];
};

// Left alone the scheduler lifts a whole product's LDS reads ahead of its MFMAs (ocppo_vit_ffn.hip)
__device__ __forceinline__ void oct_fence() { __builtin_amdgcn_sched_barrier(0); }

// acc[m] += rows 16 m .. of the A tile (row form, stride lda) times the B slice b, chunks t < KT.
// Lane (r, g) holds A[16 m + r][16 t + 4 g + c] and W[16 n + r][16 t + 4 g + c] for k-step c.
template <int NKT>
__device__ __forceinline__ void oct_mma(oct_x4 (&acc)[4], const float* A, int lda, int KT, int mt,
                                        const oct_x4 (&b)[NKT], int r, int g) {
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = oct_x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (t < KT) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (m < mt) {
          const float4 a = *reinterpret_cast<const float4*>(A + (16 * m + r) * lda + 16 * t + 4 * g);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[t][0], acc[m], 0, 0, 0);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[t][1], acc[m], 0, 0, 0);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[t][2], acc[m], 0, 0, 0);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[t][3], acc[m], 0, 0, 0);
        }
      }
    }
    oct_fence();
  }
}

// The epilogue of column tile n: the accumulator of row tile m holds D[16 m + 4 g + i][16 n + r] in
// component i. `residual` adds what out holds (each element is read and written by the same lane).
__device__ __forceinline__ void oct_store(const oct_x4 (&acc)[4], float bv, float* out, int ldo,
                                          int mt, int n, bool relu, bool residual, int r, int g) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (m < mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float* o = out + (16 * m + 4 * g + i) * ldo + 16 * n + r;
        float v = acc[m][i] + bv;
        if (relu) v = relu_f(v);
        if (residual) v = *o + v;
        *o = v;
      }
    }
  }
}

// The B slice of output columns 16 n + r of an [.., E] weight: row `wrow` as E / 16 float4 per lane
__device__ __forceinline__ void oct_load_slice(oct_x4 (&b)[kOctKT], const float* __restrict__ wrow,
                                               int KT, int g) {
#pragma unroll
  for (int t = 0; t < kOctKT; ++t) {
    b[t] = oct_x4{0.f, 0.f, 0.f, 0.f};
    if (t < KT) {
      const float4 v = *reinterpret_cast<const float4*>(wrow + 16 * t + 4 * g);
      b[t] = oct_x4{v.x, v.y, v.z, v.w};
    }
  }
}

// out[0 .. 16 mt, 0 .. 16 NT) = epilogue(A[.., 0 .. 16 KT) W^T + bias): A an LDS tile of row stride
// lda, W [16 NT, 16 KT] row-major in global memory and 16-byte aligned, out an LDS tile of row
// stride ldo. Every wave of the workgroup calls it; the caller synchronises around it.
__device__ __forceinline__ void oct_linear(const float* A, int lda, int KT,
                                           const float* __restrict__ W,
                                           const float* __restrict__ bias, int NT, int mt,
                                           float* out, int ldo, bool relu, bool residual,
                                           int w, int r, int g) {
  const int K = 16 * KT;
  oct_x4 b[kOctKT];
  if (w < NT) oct_load_slice(b, W + (16 * w + r) * K, KT, g);
  for (int n = w; n < NT; n += kOctWaves) {
    oct_x4 bn[kOctKT];
    const bool more = n + kOctWaves < NT;
    if (more) oct_load_slice(bn, W + (16 * (n + kOctWaves) + r) * K, KT, g);
    const float bv = bias[16 * n + r];
    oct_x4 acc[4];
    oct_mma<kOctKT>(acc, A, lda, KT, mt, b, r, g);
    oct_store(acc, bv, out, ldo, mt, n, relu, residual, r, g);
    if (more) {
#pragma unroll
      for (int t = 0; t < kOctKT; ++t) b[t] = bn[t];
    }
  }
}

// The encoder Linear, out = A W^T + bias with W [16 NT, K], 1 <= K <= 64 of any residue and any
// 4-byte alignment: scalar weight loads. Past K the column index is clamped to the row's last
// column instead of zero-filled: those products meet the zero columns K .. 16 KT of the A tile, so
// a finite weight adds exactly 0. A non-finite one gives inf * 0 = NaN, but the value read is
// W[n][K - 1], a weight of the same output column: that column is already non-finite through its
// real product with column K - 1 (no per-lane masks to keep: the loads are unconditional).
__device__ __forceinline__ void oct_encoder(const float* A, int lda, int KT,
                                            const float* __restrict__ W, int K,
                                            const float* __restrict__ bias, int NT, int mt,
                                            float* out, int ldo, int w, int r, int g) {
  constexpr int NKT = kOctMaxF / 16;
  for (int n = w; n < NT; n += kOctWaves) {
    const float* wrow = W + (16 * n + r) * K;
    oct_x4 b[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      b[t] = oct_x4{0.f, 0.f, 0.f, 0.f};
      if (t < KT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = 16 * t + 4 * g + c;
          b[t][c] = wrow[k < K - 1 ? k : K - 1];
        }
      }
    }
    oct_x4 acc[4];
    oct_mma<NKT>(acc, A, lda, KT, mt, b, r, g);
    oct_store(acc, bias[16 * n + r], out, ldo, mt, n, false, false, r, g);
  }
}

// LayerNorm in place on rows 0 .. nrows of the token tile: wave w takes rows w, w + 8, ..., lane l
// the columns l and l + 64 (E <= 128). Biased variance about the mean.
__device__ __forceinline__ void oct_layernorm(float* h, int ld, int E, int nrows,
                                              const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, int w,
                                              int lane) {
  const bool in0 = lane < E, in1 = lane + 64 < E;
  const float g0 = in0 ? gamma[lane] : 0.f, g1 = in1 ? gamma[lane + 64] : 0.f;
  const float e0 = in0 ? beta[lane] : 0.f, e1 = in1 ? beta[lane + 64] : 0.f;
  const float fe = static_cast<float>(E);
  for (int row = w; row < nrows; row += kOctWaves) {
    float* p = h + row * ld;
    float d0 = in0 ? p[lane] : 0.f, d1 = in1 ? p[lane + 64] : 0.f;
    const float mu = wave_sum(d0 + d1) / fe;
    d0 = in0 ? d0 - mu : 0.f;
    d1 = in1 ? d1 - mu : 0.f;
    const float rs = 1.0f / sqrtf(wave_sum(d0 * d0 + d1 * d1) / fe + eps);
    if (in0) p[lane] = (d0 * rs) * g0 + e0;
    if (in1) p[lane + 64] = (d1 * rs) * g1 + e1;
  }
}

// a = softmax(q k^T * scale) v per (token row, head) of rows 0 .. nrows of the q|k|v tile, the keys
// those of the row's own sample with valid != 0; a overwrites q.
template <int DH>
__device__ __forceinline__ void oct_attention(float* qkv, int ldq, int E, int S, int nrows,
                                              int heads, const float* valid, float scale,
                                              int tid) {
  for (int task = tid; task < nrows * heads; task += kOctThreads) {
    const int h = task / nrows, i = task - h * nrows;
    const int s0 = (i / S) * S;  // first row of the sample
    float* qrow = qkv + i * ldq + h * DH;
    const float* kb = qkv + s0 * ldq + E + h * DH;
    const float* vb = kb + E;
    const float* ok = valid + s0;
    float q[DH];
    load_row<DH>(q, qrow);
    float m = -INFINITY;
    for (int j = 0; j < S; ++j)
      if (ok[j] != 0.f) m = fmaxf(m, dot_row<DH>(q, kb + j * ldq) * scale);
    float l = 0.f, acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = 0.f;
    for (int j = 0; j < S; ++j) {
      if (ok[j] != 0.f) {
        const float p = expf(dot_row<DH>(q, kb + j * ldq) * scale - m);
        l += p;
        axpy_row<DH>(acc, p, vb + j * ldq);
      }
    }
#pragma unroll
    for (int c = 0; c < DH / 4; ++c)
      *reinterpret_cast<float4*>(qrow + 4 * c) = make_float4(
          acc[4 * c + 0] / l, acc[4 * c + 1] / l, acc[4 * c + 2] / l, acc[4 * c + 3] / l);
  }
}

// torch.max over a dimension propagates NaN
__device__ __forceinline__ float oct_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int DH>
__global__ __launch_bounds__(kOctThreads) void oct_trunk_kernel(
    const float* __restrict__ x, const OctParams P, int64_t B, int S, int F, int E,
    int blocks, int post, int mode, int rows, float* __restrict__ hidden) {
  extern __shared__ float4 s_oct4[];
  // 1 / sqrt(dh), a constant of the instantiation (folded at compile time), not a scalar to keep
  const float scale = static_cast<float>(1.0 / __builtin_sqrt(static_cast<double>(DH)));
  // mode: num_obj | masking << 8 | pooling << 9 (one scalar to keep instead of three)
  const int num_obj = mode & 255, pooling = mode >> 9;
  const bool masking = (mode >> 8) & 1;
  const int ET = E / 16, FP = (F + 15) & ~15, LD = E + 4;
  const int LDQ = (3 * E > FP ? 3 * E : FP) + 4;
  float* s_h = reinterpret_cast<float*>(s_oct4);  // [rows, LD]
  float* s_q = s_h + rows * LD;                   // [rows, LDQ]
  float* s_valid = s_q + rows * LDQ;              // [rows]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int G = rows >= S ? rows / S : 1;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * G;
  const int nb = B - b0 < G ? static_cast<int>(B - b0) : G;  // samples of this workgroup that exist
  const int nrows = nb * S;          // their token rows (<= rows: the host gives rows >= S)
  const int mt = (nrows + 15) / 16;  // row tiles the products run over

  // the input rows, zero beyond the real ones and in the columns F .. FP
  const float* xg = x + b0 * S * F;
  for (int idx = tid; idx < rows * FP; idx += kOctThreads) {
    const int row = idx / FP, c = idx - row * FP;
    s_q[row * LDQ + c] = row < nrows && c < F ? xg[row * F + c] : 0.f;
  }
  __syncthreads();
  for (int row = tid; row < rows; row += kOctThreads) {
    bool v = !masking;
    if (masking)
      for (int c = 0; c < num_obj; ++c) v = v || s_q[row * LDQ + c] != 0.f;
    s_valid[row] = v ? 1.f : 0.f;  // first read by the attention step, barriers later
  }

  // The depth as one loop of steps, so that the Linear, the attention walk and the LayerNorm exist
  // once each in the code: seven per block (in-proj, attention, out-proj
  // + residual, LN1, linear1 + ReLU, linear2 + residual, LN2), then the post layers, which
  // alternate between the two tiles. Every branch below is uniform over the workgroup.
  oct_encoder(s_q, LDQ, FP / 16, P.p[0], F, P.p[1], ET, mt, s_h, LD, w, r, g);
  __syncthreads();
  const int nsteps = 7 * blocks + (masking ? post : 0);
#pragma unroll 1
  for (int st = 0; st < nsteps; ++st) {
    const int l = st / 7, ph = st < 7 * blocks ? st % 7 : 7;
    const int base = 2 + kOctLayerPtrs * l;  // the block's pointers
    if (ph == 1) {
      oct_attention<DH>(s_q, LDQ, E, S, nrows, E / DH, s_valid, scale, tid);
    } else if (ph == 3 || ph == 6) {
      oct_layernorm(s_h, LD, E, nrows, P.p[base + (ph == 3 ? 4 : 10)],
                    P.p[base + (ph == 3 ? 5 : 11)], P.eps[2 * l + (ph == 6)], w, lane);
    } else {
      // a Linear: from the token tile to the scratch tile or back
      const bool post_step = ph == 7;
      const bool from_h = post_step ? ((st - 7 * blocks) & 1) == 0 : (ph == 0 || ph == 4);
      const int wi = post_step ? 2 + kOctLayerPtrs * blocks + 2 * (st - 7 * blocks)
                               : base + (ph == 0 ? 0 : ph == 2 ? 2 : ph == 4 ? 6 : 8);
      const float* A = from_h ? s_h : s_q;
      float* out = from_h ? s_q : s_h;
      oct_linear(A, from_h ? LD : LDQ, ET, P.p[wi], P.p[wi + 1], ph == 0 ? 3 * ET : ET, mt, out,
                 from_h ? LDQ : LD, ph == 4 || post_step, ph == 2 || ph == 5, w, r, g);
    }
    __syncthreads();
  }

  // an odd number of post layers leaves the tokens in the scratch tile
  const bool in_q = masking && (post & 1);
  const float* cur = in_q ? s_q : s_h;
  const int ldc = in_q ? LDQ : LD;

  // pooling with the reference's quirks: masked max multiplies the rows by the mask first, masked
  // mean sums ALL rows and divides by the valid count
  for (int idx = tid; idx < nb * E; idx += kOctThreads) {
    const int s = idx / E, c = idx - s * E;
    const float* t = cur + s * S * ldc + c;
    const float* ok = s_valid + s * S;
    float v;
    if (pooling == OCPPO_OCT_POOL_FIRST) {
      v = t[0];
    } else if (pooling == OCPPO_OCT_POOL_MAX) {
      v = masking ? t[0] * ok[0] : t[0];
      for (int j = 1; j < S; ++j) v = oct_max(v, masking ? t[j * ldc] * ok[j] : t[j * ldc]);
    } else {
      float sum = 0.f, cnt = 0.f;
      for (int j = 0; j < S; ++j) {
        sum += t[j * ldc];
        cnt += ok[j];
      }
      v = sum / (masking ? cnt : static_cast<float>(S));
    }
    hidden[(b0 + s) * E + c] = v;
  }
}

// Token rows per workgroup: a tile must hold a whole sample (rows >= S). Among the tiles that do,
// the smallest one that still leaves at most kOctSmallTileGroups workgroups: small batches spread
// over many CUs (80 rows: five 16-row workgroups, not two 64-row ones), large ones stop re-reading
// the weights per 16 rows (DESIGN.md 13 has the measurements).
constexpr int64_t kOctSmallTileGroups = 256;

inline int oct_tile_rows(int64_t B, int64_t S) {
  for (int rows = 16; rows < kOctMaxRows; rows *= 2) {
    if (rows < S) continue;
    if (ceil_div(B, rows / S) <= kOctSmallTileGroups) return rows;
  }
  return kOctMaxRows;
}

inline size_t oct_lds_bytes(int rows, int64_t E, int64_t F) {
  const int64_t FP = (F + 15) & ~int64_t(15);
  const int64_t LDQ = (3 * E > FP ? 3 * E : FP) + 4;
  return static_cast<size_t>(rows * (E + 4 + LDQ) + rows) * sizeof(float);
}

template <int DH>
static void oct_launch(dim3 grid, size_t lds, hipStream_t s, const float* x, const OctParams& P,
                       int64_t B, int S, int F, int E, int blocks, int post,
                       int mode, int rows, float* hidden) {
  // more than 64 KB of dynamic LDS (the CU has 160 KB) is asked for per kernel, before its launch
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(oct_trunk_kernel<DH>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  hipLaunchKernelGGL((oct_trunk_kernel<DH>), grid, dim3(kOctThreads), lds, s, x, P, B, S, F, E,
                     blocks, post, mode, rows, hidden);
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_oct_trunk_fwd(ocppo_stream_t stream, const float* x,
                                   const float* const* params, const double* eps, int64_t B,
                                   int64_t S, int64_t F, int64_t E, int64_t heads, int64_t blocks,
                                   int64_t post, int64_t num_obj, int masking, int pooling,
                                   int64_t tile_rows, float* hidden) {
  const char* who = "ocppo_oct_trunk_fwd";
  OCPPO_REQUIRE(B >= 1 && S >= 1 && S <= kOctMaxS && F >= 1 && F <= kOctMaxF && E >= 16 &&
                    E <= kOctMaxE && E % 16 == 0 && heads >= 1 && E % heads == 0,
                "%s: bad sizes B=%lld S=%lld F=%lld E=%lld heads=%lld (B >= 1, 1 <= S <= %d, "
                "1 <= F <= %d, E a multiple of 16 in [16, %d], heads | E)", who, (long long)B,
                (long long)S, (long long)F, (long long)E, (long long)heads, kOctMaxS, kOctMaxF,
                kOctMaxE);
  const int64_t dh = E / heads;
  OCPPO_REQUIRE(dh == 8 || dh == 16 || dh == 32 || dh == 64,
                "%s: head dim %lld not in {8, 16, 32, 64}", who, (long long)dh);
  OCPPO_REQUIRE(blocks >= 0 && blocks <= kOctMaxBlocks && post >= 0 && post <= kOctMaxPost,
                "%s: blocks=%lld post=%lld (blocks <= %d, post layers <= %d)", who,
                (long long)blocks, (long long)post, kOctMaxBlocks, kOctMaxPost);
  OCPPO_REQUIRE(num_obj >= 1 && num_obj <= F, "%s: num_obj=%lld not in [1, F]", who,
                (long long)num_obj);
  OCPPO_REQUIRE(pooling == OCPPO_OCT_POOL_MAX || pooling == OCPPO_OCT_POOL_MEAN ||
                    pooling == OCPPO_OCT_POOL_FIRST, "%s: pooling %d", who, pooling);
  OCPPO_REQUIRE(tile_rows == 0 ||
                    ((tile_rows == 16 || tile_rows == 32 || tile_rows == 64) && tile_rows >= S),
                "%s: tile_rows=%lld (0, or 16 / 32 / 64 and >= S)", who, (long long)tile_rows);
  OCPPO_REQUIRE(x && params && hidden && (eps || blocks == 0), "%s: null pointer", who);
  const int64_t np = 2 + kOctLayerPtrs * blocks + 2 * post;
  for (int64_t i = 0; i < np; ++i)
    OCPPO_REQUIRE(params[i] != nullptr, "%s: null parameter pointer %lld", who, (long long)i);
  OctParams P = {};
  for (int64_t i = 0; i < np; ++i) P.p[i] = params[i];
  for (int64_t i = 2; i < np; i += 2) {  // the [., E] weights: even slots but the LayerNorms'
    const int64_t k = i < 2 + kOctLayerPtrs * blocks ? (i - 2) % kOctLayerPtrs : 0;
    OCPPO_REQUIRE(k == 4 || k == 10 || (reinterpret_cast<uintptr_t>(params[i]) & 15) == 0,
                  "%s: weight %lld not 16-B aligned", who, (long long)i);
  }
  for (int64_t i = 0; i < 2 * blocks; ++i) P.eps[i] = static_cast<float>(eps[i]);
  const int rows = tile_rows ? static_cast<int>(tile_rows) : oct_tile_rows(B, S);
  const int64_t groups = ceil_div(B, rows / S);
  OCPPO_REQUIRE(groups <= INT32_MAX, "%s: %lld workgroups exceed the grid", who,
                (long long)groups);
  const size_t lds = oct_lds_bytes(rows, E, F);
  const dim3 grid(static_cast<unsigned>(groups));
  const int mode = static_cast<int>(num_obj) | (masking != 0) << 8 | pooling << 9;
  clear_stale_error();
#define OCPPO_OCT_CASE(DHV)                                                                       \
  case DHV:                                                                                       \
    oct_launch<DHV>(grid, lds, as_stream(stream), x, P, B, (int)S, (int)F, (int)E,                \
                    (int)blocks, (int)post, mode, rows, hidden);                                  \
    break;
  switch (dh) {
    OCPPO_OCT_CASE(8)
    OCPPO_OCT_CASE(16)
    OCPPO_OCT_CASE(32)
    OCPPO_OCT_CASE(64)
  }
#undef OCPPO_OCT_CASE
  return check_launch(who);
}

extern "C" int64_t ocppo_oct_trunk_tile_rows(int64_t B, int64_t S) {
  if (B < 1 || S < 1 || S > kOctMaxS) return 0;
  return oct_tile_rows(B, S);
}
