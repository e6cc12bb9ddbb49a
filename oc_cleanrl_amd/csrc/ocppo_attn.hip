// The two non-Linear pieces of a post-norm transformer encoder block, for the object-set PPO agent
// of cleanrl/ppo_atari_oc_transformer.py:215-277 (torch.nn.TransformerEncoderLayer, batch_first):
// masked multi-head self-attention over short sequences (S <= 64 objects, head dim 8..64) and the
// residual add + LayerNorm that follows each half of the block; each with its backward.
//
// Attention, rows in lanes: one wave owns one (sample, head) problem. The head's K and V rows sit
// in LDS (row stride dh + 4 floats, so the per-lane row writes of the backward spread over the
// banks); lane i holds query row i in registers and walks the keys, every lane reading the same
// K / V row as one LDS broadcast. The score row is never stored: pass 1 takes its maximum, pass 2
// recomputes each score, exponentiates and accumulates p * V_j. Excluded keys are skipped (a
// wave-uniform branch on the ballot of key_valid), which is the exact weight 0 that -inf gives.
// The backward runs the same walk for dQ, then swaps roles: the lanes' Q and dO rows replace K and
// V in LDS and lane j, holding K_j and V_j, walks the queries for dK_j and dV_j -- a sum in query
// order inside one lane, so no atomics and no cross-lane order to fix. Both walks form a score
// with the same dot product (same operand pairs, same order), so the recomputed probabilities of
// the two phases are the same bits.
//
// Why not v_mfma_f32_16x16x4f32: at the agent's shapes (S = 6..32 objects, dh = 16) a 16 x 16
// tile is mostly padding, the softmax between the two products needs the score tile moved from the
// MFMA's column-per-lane layout to a row-wise one through LDS, and the whole problem is ~S^2 dh
// FMAs per lane-row -- launch-bound, not FLOP-bound.
//
// Dropout (the DROP instantiations, and ocppo_dropout for the three elementwise sites of a layer):
// the mask is a function of counters, regenerated wherever it is needed and never stored. A
// launch reads the generator state rng = (seed, offset) from device memory (a replayed hipGraph
// reads the state of that replay) and takes a host `site`; element -> (Philox block, component)
// is fixed per layout (DropRng below); keep iff word >= thr, an integer compare.
// The p = 0 instantiations carry none of this and are the kernels as they were.
#include <math.h>

#include "ocppo_common.h"
#include "ocppo_layernorm.h"
#include "ocppo_philox.h"

namespace ocppo {

constexpr int kAttnMaxS = 64;
// residual add + LayerNorm: ocppo_layernorm.h's kernels at E <= 512, 8 columns per lane for every E
constexpr int kLnMaxE = 512;
constexpr int kLnPerLane = kLnMaxE / kWave;

// sum_d a[d] * row[d]: four interleaved FMA chains, combined (0 + 1) + (2 + 3). Every score and
// every dP of this file goes through here with the register operand first.
template <int DH>
__device__ __forceinline__ float dot_row(const float (&a)[DH], const float* __restrict__ row) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * c);
    s0 = fmaf(a[4 * c + 0], r.x, s0);
    s1 = fmaf(a[4 * c + 1], r.y, s1);
    s2 = fmaf(a[4 * c + 2], r.z, s2);
    s3 = fmaf(a[4 * c + 3], r.w, s3);
  }
  return (s0 + s1) + (s2 + s3);
}

template <int DH>
__device__ __forceinline__ void axpy_row(float (&acc)[DH], float a, const float* __restrict__ row) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(row + 4 * c);
    acc[4 * c + 0] = fmaf(a, r.x, acc[4 * c + 0]);
    acc[4 * c + 1] = fmaf(a, r.y, acc[4 * c + 1]);
    acc[4 * c + 2] = fmaf(a, r.z, acc[4 * c + 2]);
    acc[4 * c + 3] = fmaf(a, r.w, acc[4 * c + 3]);
  }
}

template <int DH>
__device__ __forceinline__ void load_row(float (&v)[DH], const float* __restrict__ src) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 r = *reinterpret_cast<const float4*>(src + 4 * c);
    v[4 * c + 0] = r.x; v[4 * c + 1] = r.y; v[4 * c + 2] = r.z; v[4 * c + 3] = r.w;
  }
}

template <int DH>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const float (&v)[DH], float mul) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c)
    *reinterpret_cast<float4*>(dst + 4 * c) = make_float4(
        v[4 * c + 0] * mul, v[4 * c + 1] * mul, v[4 * c + 2] * mul, v[4 * c + 3] * mul);
}

// S rows of DH floats at `src` (row stride `stride` floats) -> an LDS tile of row stride DH + 4
template <int DH>
__device__ __forceinline__ void stage_tile(float* tile, const float* __restrict__ src, int S,
                                           int64_t stride, int lane) {
  constexpr int V = DH / 4, LD = DH + 4;
  for (int idx = lane; idx < S * V; idx += kWave) {
    const int r = idx / V, c = idx % V;
    *reinterpret_cast<float4*>(tile + r * LD + 4 * c) =
        *reinterpret_cast<const float4*>(src + r * stride + 4 * c);
  }
}

// The dropout stream of one launch: Philox4x32-10 keyed by the seed, subsequence offset * 256 +
// site. Elementwise tensors: flat element e -> block e >> 2, component e & 3. Attention
// probabilities of (sample b, head h, query i, key j): block ((b * H + h) * 64 + i) * 16 + (j >> 2),
// component j & 3 -- independent of S, four consecutive keys of a query row per block.
struct DropRng {
  uint64_t seed, sub;
  uint32_t thr;
  float scale;  // 1 / (1 - p)
};

__device__ __forceinline__ DropRng drop_rng(const int64_t* __restrict__ rng, uint32_t site,
                                            uint32_t thr, float scale) {
  return {static_cast<uint64_t>(rng[0]), static_cast<uint64_t>(rng[1]) * 256u + site, thr, scale};
}

__device__ __forceinline__ uint32_t word_of(const uint4& w, int comp) {
  return comp == 0 ? w.x : comp == 1 ? w.y : comp == 2 ? w.z : w.w;
}

// first Philox block of query row i of problem bh = b * H + h
__device__ __forceinline__ uint64_t attn_row_block(uint32_t bh, int i) {
  return (static_cast<uint64_t>(bh) * kAttnMaxS + static_cast<uint64_t>(i)) * (kAttnMaxS / 4);
}

__device__ __forceinline__ uint64_t key_mask(const uint8_t* __restrict__ key_valid, int64_t b,
                                             int S, int lane) {
  const bool kv = lane < S && (key_valid == nullptr || key_valid[b * S + lane] != 0);
  return __ballot(kv);
}

template <int DH, bool DROP>
__global__ __launch_bounds__(kWave) void mha_fwd_kernel(
    const float* __restrict__ qkv, const uint8_t* __restrict__ key_valid, int S, int E, int heads,
    float scale, float* __restrict__ out, float* __restrict__ lse,
    const int64_t* __restrict__ rng, uint32_t site, uint32_t thr, float dscale) {
  constexpr int LD = DH + 4;
  extern __shared__ float4 s_dyn4[];
  float* s_k = reinterpret_cast<float*>(s_dyn4);
  float* s_v = s_k + S * LD;
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const int64_t ld = 3 * static_cast<int64_t>(E);
  const float* base = qkv + b * S * ld + h * DH;
  stage_tile<DH>(s_k, base + E, S, ld, lane);
  stage_tile<DH>(s_v, base + 2 * E, S, ld, lane);
  const uint64_t vmask = key_mask(key_valid, b, S, lane);
  __syncthreads();
  if (lane >= S) return;
  float q[DH];
  load_row<DH>(q, base + lane * ld);
  float m = -INFINITY;
  for (int j = 0; j < S; ++j) {
    if (!((vmask >> j) & 1)) continue;  // wave-uniform
    m = fmaxf(m, dot_row<DH>(q, s_k + j * LD) * scale);
  }
  float l = 0.f, acc[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
  if constexpr (DROP) {
    // the denominator runs over every valid key, the accumulation over the kept ones (x dscale);
    // one Philox block per four keys of this lane's query row, skipped when all four are excluded
    const DropRng dr = drop_rng(rng, site, thr, dscale);
    const uint64_t blk0 = attn_row_block(blockIdx.x, lane);
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    for (int j = 0; j < S; ++j) {
      if ((j & 3) == 0 && ((vmask >> j) & 0xF)) w = philox_block(dr.seed, dr.sub, blk0 + (j >> 2));
      if (!((vmask >> j) & 1)) continue;
      const float p = expf(dot_row<DH>(q, s_k + j * LD) * scale - m);
      l += p;
      const float pm = word_of(w, j & 3) >= dr.thr ? p * dr.scale : 0.f;
      axpy_row<DH>(acc, pm, s_v + j * LD);
    }
  } else {
    for (int j = 0; j < S; ++j) {
      if (!((vmask >> j) & 1)) continue;
      const float p = expf(dot_row<DH>(q, s_k + j * LD) * scale - m);
      l += p;
      axpy_row<DH>(acc, p, s_v + j * LD);
    }
  }
  float* o = out + (b * S + lane) * E + h * DH;
#pragma unroll
  for (int c = 0; c < DH / 4; ++c)
    *reinterpret_cast<float4*>(o + 4 * c) = make_float4(
        acc[4 * c + 0] / l, acc[4 * c + 1] / l, acc[4 * c + 2] / l, acc[4 * c + 3] / l);
  lse[(b * heads + h) * S + lane] = m + logf(l);
}

// With dropout, m_ij = keep_ij * dscale: dP_ij = m_ij (dO_i . V_j), D_i = dO_i . O_i (still
// sum_j P_ij dP_ij), dS_ij = P_ij (dP_ij - D_i), dV_j = sum_i m_ij P_ij dO_i.
template <int DH, bool DROP>
__global__ __launch_bounds__(kWave) void mha_bwd_kernel(
    const float* __restrict__ qkv, const uint8_t* __restrict__ key_valid,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout,
    int S, int E, int heads, float scale, float* __restrict__ dqkv,
    const int64_t* __restrict__ rng, uint32_t site, uint32_t thr, float dscale) {
  constexpr int LD = DH + 4;
  extern __shared__ float4 s_dyn4[];
  float* s_a = reinterpret_cast<float*>(s_dyn4);  // K rows, then Q rows
  float* s_b = s_a + S * LD;                      // V rows, then dO rows
  float* s_lse = s_b + S * LD;                    // [kAttnMaxS]
  float* s_dd = s_lse + kAttnMaxS;                // [kAttnMaxS] D_i = sum_d dO * O
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const int64_t ld = 3 * static_cast<int64_t>(E);
  const float* base = qkv + b * S * ld + h * DH;
  float* dbase = dqkv + b * S * ld + h * DH;
  stage_tile<DH>(s_a, base + E, S, ld, lane);
  stage_tile<DH>(s_b, base + 2 * E, S, ld, lane);
  const uint64_t vmask = key_mask(key_valid, b, S, lane);
  __syncthreads();
  const bool row = lane < S;
  DropRng dr = {0, 0, 0u, 1.f};
  if constexpr (DROP) dr = drop_rng(rng, site, thr, dscale);
  {
    // phase A: lane = query i -> dQ_i
    float q[DH], g_o[DH];
    float lse_i = 0.f, dd = 0.f;
    if (row) {
      load_row<DH>(q, base + lane * ld);
      load_row<DH>(g_o, dout + (b * S + lane) * E + h * DH);
      dd = dot_row<DH>(g_o, out + (b * S + lane) * E + h * DH);
      lse_i = lse[(b * heads + h) * S + lane];
      float dq[DH];
#pragma unroll
      for (int d = 0; d < DH; ++d) dq[d] = 0.f;
      if constexpr (DROP) {
        const uint64_t blk0 = attn_row_block(blockIdx.x, lane);
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        for (int j = 0; j < S; ++j) {
          if ((j & 3) == 0 && ((vmask >> j) & 0xF))
            w = philox_block(dr.seed, dr.sub, blk0 + (j >> 2));
          if (!((vmask >> j) & 1)) continue;  // wave-uniform
          const float p = expf(dot_row<DH>(q, s_a + j * LD) * scale - lse_i);
          const float mk = word_of(w, j & 3) >= dr.thr ? dr.scale : 0.f;
          const float ds = p * (mk * dot_row<DH>(g_o, s_b + j * LD) - dd);
          axpy_row<DH>(dq, ds, s_a + j * LD);
        }
      } else {
        for (int j = 0; j < S; ++j) {
          if (!((vmask >> j) & 1)) continue;  // wave-uniform
          const float p = expf(dot_row<DH>(q, s_a + j * LD) * scale - lse_i);
          const float ds = p * (dot_row<DH>(g_o, s_b + j * LD) - dd);
          axpy_row<DH>(dq, ds, s_a + j * LD);
        }
      }
      store_row<DH>(dbase + lane * ld, dq, scale);
    }
    __syncthreads();  // every lane is done with K and V
    if (row) {
      store_row<DH>(s_a + lane * LD, q, 1.f);
      store_row<DH>(s_b + lane * LD, g_o, 1.f);
      s_lse[lane] = lse_i;
      s_dd[lane] = dd;
    }
    __syncthreads();
  }
  if (!row) return;
  // phase B: lane = key j -> dK_j, dV_j (queries in order 0..S-1)
  float dk[DH], dv[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) dk[d] = dv[d] = 0.f;
  if ((vmask >> lane) & 1) {
    float k[DH], v[DH];
    load_row<DH>(k, base + E + lane * ld);
    load_row<DH>(v, base + 2 * E + lane * ld);
    if constexpr (DROP) {
      // word (i, j): lane j's component of block j >> 2 of query row i, once per query
      const uint64_t blk0 = attn_row_block(blockIdx.x, 0) + (lane >> 2);
      for (int i = 0; i < S; ++i) {
        const uint4 w = philox_block(dr.seed, dr.sub, blk0 + i * (kAttnMaxS / 4));
        const float mk = word_of(w, lane & 3) >= dr.thr ? dr.scale : 0.f;
        const float p = expf(dot_row<DH>(k, s_a + i * LD) * scale - s_lse[i]);
        const float ds = p * (mk * dot_row<DH>(v, s_b + i * LD) - s_dd[i]);
        axpy_row<DH>(dk, ds, s_a + i * LD);
        axpy_row<DH>(dv, mk * p, s_b + i * LD);
      }
    } else {
      for (int i = 0; i < S; ++i) {
        const float p = expf(dot_row<DH>(k, s_a + i * LD) * scale - s_lse[i]);
        const float ds = p * (dot_row<DH>(v, s_b + i * LD) - s_dd[i]);
        axpy_row<DH>(dk, ds, s_a + i * LD);
        axpy_row<DH>(dv, p, s_b + i * LD);
      }
    }
  }
  store_row<DH>(dbase + E + lane * ld, dk, scale);
  store_row<DH>(dbase + 2 * E + lane * ld, dv, 1.f);
}

// ---- elementwise dropout ------------------------------------------------------------------------
// y = keep ? x * scale : 0, one Philox block per thread = four consecutive elements. VEC: both
// pointers 16-B aligned, the full blocks move as float4; the last partial block, and every block
// when a pointer is not aligned, goes element by element (the same words either way).
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ rng, uint32_t site, uint32_t thr,
    float scale, int64_t n, float* __restrict__ y) {
  const DropRng dr = drop_rng(rng, site, thr, scale);
  const int64_t nblk = (n + 3) >> 2;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < nblk;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const uint4 w = philox_block(dr.seed, dr.sub, static_cast<uint64_t>(t));
    const int64_t e = t << 2;
    if (VEC && e + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(x + e);
      *reinterpret_cast<float4*>(y + e) = make_float4(
          w.x >= dr.thr ? v.x * dr.scale : 0.f, w.y >= dr.thr ? v.y * dr.scale : 0.f,
          w.z >= dr.thr ? v.z * dr.scale : 0.f, w.w >= dr.thr ? v.w * dr.scale : 0.f);
    } else {
      for (int c = 0; c < 4 && e + c < n; ++c)
        y[e + c] = word_of(w, c) >= dr.thr ? x[e + c] * dr.scale : 0.f;
    }
  }
}

// the generator moves on by one draw: every site of the next forward reads a new subsequence
__global__ void philox_advance_kernel(int64_t* __restrict__ rng) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rng[1] += 1;
}

inline int mha_check(const char* who, int64_t B, int64_t S, int64_t E, int64_t heads) {
  OCPPO_REQUIRE(B >= 1 && S >= 1 && S <= kAttnMaxS && E >= 1 && E <= 512 && heads >= 1 &&
                    E % heads == 0,
                "%s: bad sizes B=%lld S=%lld E=%lld heads=%lld (B >= 1, 1 <= S <= %d, E <= 512, "
                "heads | E)", who, (long long)B, (long long)S, (long long)E, (long long)heads,
                kAttnMaxS);
  const int64_t dh = E / heads;
  OCPPO_REQUIRE(dh == 8 || dh == 16 || dh == 32 || dh == 64,
                "%s: head dim %lld not in {8, 16, 32, 64}", who, (long long)dh);
  OCPPO_REQUIRE(B * heads <= INT32_MAX, "%s: B * heads = %lld exceeds the grid", who,
                (long long)(B * heads));
  return OCPPO_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ocppo

using namespace ocppo;

#define OCPPO_MHA_DISPATCH(DHV, CALL) \
  switch (DHV) {                      \
    case 8: { constexpr int DH = 8; CALL; break; }   \
    case 16: { constexpr int DH = 16; CALL; break; } \
    case 32: { constexpr int DH = 32; CALL; break; } \
    default: { constexpr int DH = 64; CALL; break; } \
  }

// dropout arguments shared by the three entries that draw a mask
inline int drop_check(const char* who, const int64_t* rng, int64_t site, float scale) {
  OCPPO_REQUIRE(rng != nullptr, "%s: null rng", who);
  OCPPO_REQUIRE(site >= 0 && site < 256, "%s: site %lld not in [0, 256)", who, (long long)site);
  OCPPO_REQUIRE(scale >= 1.f && scale < INFINITY, "%s: scale %g is not 1 / (1 - p), 0 <= p < 1",
                who, (double)scale);
  return OCPPO_OK;
}

template <bool DROP>
static int mha_fwd_launch(const char* who, ocppo_stream_t stream, const float* qkv,
                          const uint8_t* key_valid, const int64_t* rng, int64_t site, uint32_t thr,
                          float dscale, int64_t B, int64_t S, int64_t E, int64_t heads, float* out,
                          float* lse) {
  if (int rc = mha_check(who, B, S, E, heads)) return rc;
  OCPPO_REQUIRE(qkv && out && lse, "%s: null pointer", who);
  OCPPO_REQUIRE(aligned16(qkv) && aligned16(out), "%s: qkv / out not 16-B aligned", who);
  if (DROP)
    if (int rc = drop_check(who, rng, site, dscale)) return rc;
  const int dh = static_cast<int>(E / heads);
  const float scale = static_cast<float>(1.0 / sqrt(static_cast<double>(dh)));
  const size_t lds = 2 * static_cast<size_t>(S) * (dh + 4) * sizeof(float);
  clear_stale_error();
  OCPPO_MHA_DISPATCH(dh, hipLaunchKernelGGL((mha_fwd_kernel<DH, DROP>),
                                            dim3(static_cast<unsigned>(B * heads)), dim3(kWave),
                                            lds, as_stream(stream), qkv, key_valid, (int)S, (int)E,
                                            (int)heads, scale, out, lse, rng,
                                            static_cast<uint32_t>(site), thr, dscale));
  return check_launch(who);
}

template <bool DROP>
static int mha_bwd_launch(const char* who, ocppo_stream_t stream, const float* qkv,
                          const uint8_t* key_valid, const float* out, const float* lse,
                          const float* dout, const int64_t* rng, int64_t site, uint32_t thr,
                          float dscale, int64_t B, int64_t S, int64_t E, int64_t heads,
                          float* dqkv) {
  if (int rc = mha_check(who, B, S, E, heads)) return rc;
  OCPPO_REQUIRE(qkv && out && lse && dout && dqkv, "%s: null pointer", who);
  OCPPO_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv),
                "%s: qkv / out / dout / dqkv not 16-B aligned", who);
  if (DROP)
    if (int rc = drop_check(who, rng, site, dscale)) return rc;
  const int dh = static_cast<int>(E / heads);
  const float scale = static_cast<float>(1.0 / sqrt(static_cast<double>(dh)));
  const size_t lds = (2 * static_cast<size_t>(S) * (dh + 4) + 2 * kAttnMaxS) * sizeof(float);
  clear_stale_error();
  OCPPO_MHA_DISPATCH(dh, hipLaunchKernelGGL((mha_bwd_kernel<DH, DROP>),
                                            dim3(static_cast<unsigned>(B * heads)), dim3(kWave),
                                            lds, as_stream(stream), qkv, key_valid, out, lse, dout,
                                            (int)S, (int)E, (int)heads, scale, dqkv, rng,
                                            static_cast<uint32_t>(site), thr, dscale));
  return check_launch(who);
}

extern "C" int ocppo_mha_fwd(ocppo_stream_t stream, const float* qkv, const uint8_t* key_valid,
                             int64_t B, int64_t S, int64_t E, int64_t heads, float* out,
                             float* lse) {
  return mha_fwd_launch<false>("ocppo_mha_fwd", stream, qkv, key_valid, nullptr, 0, 0u, 1.f, B, S,
                               E, heads, out, lse);
}

extern "C" int ocppo_mha_bwd(ocppo_stream_t stream, const float* qkv, const uint8_t* key_valid,
                             const float* out, const float* lse, const float* dout, int64_t B,
                             int64_t S, int64_t E, int64_t heads, float* dqkv) {
  return mha_bwd_launch<false>("ocppo_mha_bwd", stream, qkv, key_valid, out, lse, dout, nullptr, 0,
                               0u, 1.f, B, S, E, heads, dqkv);
}

extern "C" int ocppo_mha_dropout_fwd(ocppo_stream_t stream, const float* qkv,
                                     const uint8_t* key_valid, const int64_t* rng, int64_t site,
                                     uint32_t thr, float scale, int64_t B, int64_t S, int64_t E,
                                     int64_t heads, float* out, float* lse) {
  return mha_fwd_launch<true>("ocppo_mha_dropout_fwd", stream, qkv, key_valid, rng, site, thr,
                              scale, B, S, E, heads, out, lse);
}

extern "C" int ocppo_mha_dropout_bwd(ocppo_stream_t stream, const float* qkv,
                                     const uint8_t* key_valid, const float* out, const float* lse,
                                     const float* dout, const int64_t* rng, int64_t site,
                                     uint32_t thr, float scale, int64_t B, int64_t S, int64_t E,
                                     int64_t heads, float* dqkv) {
  return mha_bwd_launch<true>("ocppo_mha_dropout_bwd", stream, qkv, key_valid, out, lse, dout, rng,
                              site, thr, scale, B, S, E, heads, dqkv);
}

extern "C" int ocppo_dropout(ocppo_stream_t stream, const float* x, const int64_t* rng,
                             int64_t site, uint32_t thr, float scale, int64_t n, float* y) {
  OCPPO_REQUIRE(n >= 0, "ocppo_dropout: n = %lld < 0", (long long)n);
  if (int rc = drop_check("ocppo_dropout", rng, site, scale)) return rc;
  if (n == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && y, "ocppo_dropout: null pointer");
  OCPPO_REQUIRE(x != y, "ocppo_dropout: out of place only");
  const int grid = grid_for(ceil_div(n, 4), 256);
  clear_stale_error();
  if (aligned16(x) && aligned16(y))
    hipLaunchKernelGGL(dropout_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), x, rng,
                       static_cast<uint32_t>(site), thr, scale, n, y);
  else
    hipLaunchKernelGGL(dropout_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), x, rng,
                       static_cast<uint32_t>(site), thr, scale, n, y);
  return check_launch("ocppo_dropout");
}

extern "C" int ocppo_philox_advance(ocppo_stream_t stream, int64_t* rng) {
  OCPPO_REQUIRE(rng != nullptr, "ocppo_philox_advance: null rng");
  clear_stale_error();
  hipLaunchKernelGGL(philox_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), rng);
  return check_launch("ocppo_philox_advance");
}

extern "C" int ocppo_add_layernorm_fwd(ocppo_stream_t stream, const float* x, const float* res,
                                       const float* gamma, const float* beta, int64_t R,
                                       int64_t E, double eps, float* y, float* mean,
                                       float* rstd) {
  OCPPO_REQUIRE(R >= 0 && R <= INT32_MAX && E >= 1 && E <= kLnMaxE,
                "ocppo_add_layernorm_fwd: bad sizes R=%lld E=%lld (R >= 0, 1 <= E <= %d)",
                (long long)R, (long long)E, kLnMaxE);
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && res && gamma && beta && y && mean && rstd,
                "ocppo_add_layernorm_fwd: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL((layernorm_fwd_kernel<LnAddResidual, kLnPerLane>),
                     dim3(grid_for(R, kLnWaves)), dim3(kLnWaves * kWave), 0, as_stream(stream), x,
                     res, gamma, beta, R, (int)E, static_cast<float>(eps), 0, y, mean, rstd);
  return check_launch("ocppo_add_layernorm_fwd");
}

extern "C" size_t ocppo_add_layernorm_workspace_bytes(int64_t R, int64_t E) {
  if (R < 0 || E < 1 || E > kLnMaxE) return 0;
  return ln_workspace_bytes(R, E);
}

extern "C" int ocppo_add_layernorm_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                       const float* res, const float* gamma, const float* mean,
                                       const float* rstd, int64_t R, int64_t E, float* dx,
                                       float* dgamma, float* dbeta, void* workspace,
                                       size_t workspace_bytes) {
  OCPPO_REQUIRE(R >= 1 && R <= INT32_MAX && E >= 1 && E <= kLnMaxE,
                "ocppo_add_layernorm_bwd: bad sizes R=%lld E=%lld (R >= 1, 1 <= E <= %d)",
                (long long)R, (long long)E, kLnMaxE);
  OCPPO_REQUIRE(dy && x && res && gamma && mean && rstd && dx && dgamma && dbeta,
                "ocppo_add_layernorm_bwd: null pointer");
  if (!workspace || workspace_bytes < ocppo_add_layernorm_workspace_bytes(R, E))
    return fail(OCPPO_E_WORKSPACE, "ocppo_add_layernorm_bwd: workspace of %zu bytes, need %zu",
                workspace_bytes, ocppo_add_layernorm_workspace_bytes(R, E));
  clear_stale_error();
  return ln_bwd_launch<LnAddResidual, kLnPerLane>(
      "ocppo_add_layernorm_bwd", "ocppo_add_layernorm_bwd (finish)", as_stream(stream), dy, x, res,
      nullptr, gamma, mean, rstd, R, E, 0, dx, dgamma, dbeta, static_cast<float*>(workspace));
}
