// Fused NoisyLinear heads of the Rainbow network (cleanrl/rainbow_atari_oc.py:239-279,
// architectures/rainbow.py:12-52): y = act(x (mu + sigma * eps)^T + (bmu + bsigma * beps)) and its
// backward, for few rows (M <= 128: acting at M = 1, the train batch at M = 32) against many
// weights (3136 -> 512 twice per network), one or two layers ("groups") per launch.
//
// The torch path writes the combined [N, K] weight, reads it back in the Linear, and autograd
// saves it and reads it again; here w = mu + sigma * eps exists only in registers (one f32
// multiply and one f32 add, -ffp-contract=off: torch's bits), so each pass streams mu, sigma and
// eps once. At these M the weight stream is the bound, not the MFMAs, and the split follows that.
//
// Forward (noisy_fwd_kernel): a workgroup owns one 16-column output tile of one group and one
//   slice of K, for ALL row tiles (acc[MT] in registers, MT = ceil(M / 16) rounded to 1/2/4/8), so
//   a weight element is loaded by exactly one wave. Its 4 waves take consecutive spans of 2 groups
//   of 32 k: per group a wave loads its 16 x 32 slices of mu, sigma and eps as whole 128-B lines
//   (lane = one 16-B piece, 8 lines per instruction: ocppo_linear.hip's staged form), combines
//   them in registers, and passes w through a wave-private LDS image to get the MFMA B fragments;
//   the x fragments (L2-resident, M x K f32) are loaded directly. All loads of a span are issued
//   before its MFMAs (v_mfma_f32_16x16x4_f32, two accumulator chains per row tile).
//   K split: 512 output columns are 32 tiles per head, so the slices go over the grid's y, not
//   over a workgroup's <= 8 waves: KS = ceil(K / 256) slices (13 at K = 3136: 832 workgroups for
//   the two first layers). KS depends on K alone, so a layer's bits do not depend on what it
//   shares a launch with. Waves combine through LDS in wave order; slices store their partial
//   fragments to the workspace and the last-arriving block of a tile (one ticket per tile, which
//   it re-arms for the next replay) adds them in slice order and runs the epilogue
//   (acc + bias, then ReLU). No float atomics.
//
// Backward (noisy_bwd_kernel): ONE pass for dmu, dsigma, dbmu, dbsigma and dx. A wave owns a strip
//   of 32 k columns (one 128-B line of every weight row) over a block of n rows (16 or 64); the 4
//   waves of a workgroup own 4 adjacent strips of the same n block and share the masked g block
//   (g * (y > 0), M x 64) in LDS. The wave keeps its x strip (M x 32) in registers as MFMA B
//   fragments for the whole block. Per 16-row n tile it
//     - loads mu / sigma / eps as whole lines (as the forward) and forms w,
//     - dmu tile [16 n x 32 k] = g^T x: M / 4 MFMA steps on two accumulators; the tile goes through
//       the wave's LDS image back to line layout, dmu and dsigma = dmu * eps (eps still in
//       registers, the f32 product of the stored dmu) are stored as 16-B pieces of whole lines,
//     - dx[:, strip] += g w: w through the same LDS image as B fragments, g from the shared block.
//   Why not the strip across ALL of N (no dx reduction at all): K = 3136 is 98 strips, 98 waves
//   for 256 CUs. Splitting N as well gives 98 x 16 waves at the pixel shape and costs one partial
//   dx [M, K] per n block (6.4 MB against 64 MB of weight traffic at M = 32), which the
//   last-arriving block of a 128-column strip group adds in block order: value head's blocks
//   first, then the advantage head's, so with a shared x the result is dx_value + dx_advantage.
//   The bias gradients are column sums of the LDS g block in row order (strip group 0 only).
//
// Both directions: f32, deterministic (fixed orders everywhere, tickets only elect the block that
// does the ordered sum), no host sync, capture-safe (the tickets are cleared by their last user).
#include "ocppo_common.h"

namespace ocppo {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kNzWaves = 4;         // waves per workgroup, both directions
constexpr int kNzRow = 36;          // floats per row of a wave's 16 x 32 LDS image (+4: 16-B reads)
constexpr int kNzSpan = 2;          // forward: groups of 32 k per wave
constexpr int kNzMaxM = 128;
constexpr int kNzTicketBytes = 16384;  // head of each workspace: 4096 tickets

__device__ __forceinline__ void wave_lds_fence() {
  // a wave's LDS operations execute in order; this only keeps the compiler from moving them
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ float4 ld4(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// mu + sigma * eps per element: one multiply, one add (no fma: torch's combine)
__device__ __forceinline__ float4 noisy_w(float4 m, float4 s, float4 e) {
  return make_float4(m.x + s.x * e.x, m.y + s.y * e.y, m.z + s.z * e.z, m.w + s.w * e.w);
}

// Cross-block hand-off (ocppo_common.h's handoff_combine form): partials are written with
// agent-scope (write-through) stores and drained with s_waitcnt vmcnt(0) before the block's ONE
// relaxed agent-scope ticket atomic; the elected block reads them with agent-scope loads. No
// release / acquire fence, so no block writes back or invalidates the L2's other lines.
__device__ __forceinline__ void st_agent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The last-arriving block of `expected` blocks on one ticket: true in every thread of that block.
// The elected block re-arms the ticket.
__device__ __forceinline__ bool arrive_last(unsigned* ticket, unsigned expected, int* s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_flag = prev == expected - 1;
    if (*s_flag) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return *s_flag != 0;
}

// ---- forward -------------------------------------------------------------------------------
struct NzFwdGroup {
  const float *x, *mu, *sigma, *eps, *bmu, *bsigma, *beps;
  float* y;
  int N, tile0;  // first column tile of this group in the grid's x
};
struct NzFwdArgs {
  NzFwdGroup g[2];
  int groups, M, K, tiles, KS, relu;
  floatx4* part;      // [KS][tiles][MT][64] fragments
  unsigned* tickets;  // [tiles]
};

template <int MT>
__global__ __launch_bounds__(64 * kNzWaves) void noisy_fwd_kernel(NzFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float stage[kNzWaves][16 * kNzRow];
  __shared__ floatx4 red[kNzWaves - 1][MT][64];
  __shared__ int s_flag;
  const int tile = blockIdx.x, slice = blockIdx.y;
  const bool second = a.groups > 1 && tile >= a.g[1].tile0;
  const NzFwdGroup G = second ? a.g[1] : a.g[0];
  const int col0 = (tile - G.tile0) * 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int piece = lane & 7, lsub = lane >> 3;
  const int M = a.M, K = a.K, N = G.N;
  float* st = stage[wv];

  // this wave's span: groups [grp0, grp0 + kNzSpan) of 32 k; everything is loaded before the MFMAs
  const int grp0 = (slice * kNzWaves + wv) * kNzSpan;
  float4 wb[kNzSpan][2], xa[kNzSpan][MT][2];
#pragma unroll
  for (int s = 0; s < kNzSpan; ++s) {
    const int k0 = (grp0 + s) * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = col0 + i * 8 + lsub, kk = k0 + piece * 4;
      const bool ok = n < N && kk < K;
      const int64_t off = static_cast<int64_t>(ok ? n : 0) * K + (ok ? kk : 0);
      wb[s][i] = noisy_w(ld4(G.mu + off, ok), ld4(G.sigma + off, ok), ld4(G.eps + off, ok));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = mt * 16 + c16, kk = k0 + q * 16 + 4 * g;
        const bool ok = m < M && kk < K;
        xa[s][mt][q] = ld4(G.x + static_cast<int64_t>(ok ? m : 0) * K + (ok ? kk : 0), ok);
      }
  }
  floatx4 acc[MT][2];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    acc[mt][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    acc[mt][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int s = 0; s < kNzSpan; ++s) {
    if ((grp0 + s) * 32 < K) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < 2; ++i)
        *reinterpret_cast<float4*>(&st[(i * 8 + lsub) * kNzRow + piece * 4]) = wb[s][i];
      wave_lds_fence();
      float4 fb[2];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        fb[q] = *reinterpret_cast<const float4*>(&st[c16 * kNzRow + q * 16 + 4 * g]);
      wave_lds_fence();
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float4 fa = xa[s][mt][q];
          floatx4& c = acc[mt][q];
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.x, fb[q].x, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.y, fb[q].y, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.z, fb[q].z, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.w, fb[q].w, c, 0, 0, 0);
        }
    }
  }
  floatx4 sum[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) sum[mt] = acc[mt][0] + acc[mt][1];
  // waves in wave order
  if (wv > 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) red[wv - 1][mt][lane] = sum[mt];
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int w = 0; w < kNzWaves - 1; ++w)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) sum[mt] += red[w][mt][lane];
  }
  if (a.KS > 1) {  // slices in slice order, by the last block to arrive on this tile
    if (wv == 0) {
      float* p = reinterpret_cast<float*>(
          a.part + (static_cast<int64_t>(slice) * a.tiles + tile) * MT * 64 + lane);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_agent(p + mt * 256 + r, sum[mt][r]);
    }
    if (!arrive_last(a.tickets + tile, a.KS, &s_flag)) return;
    if (wv == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) sum[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < a.KS; ++s) {
        const float* p = reinterpret_cast<const float*>(
            a.part + (static_cast<int64_t>(s) * a.tiles + tile) * MT * 64 + lane);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) sum[mt][r] += ld_agent(p + mt * 256 + r);
      }
    }
  }
  if (wv != 0) return;
  // C layout of the 16x16 MFMA: column lane & 15, rows 4 * (lane >> 4) + r
  const int col = col0 + c16;
  if (col >= N) return;
  const float bias = G.bmu[col] + G.bsigma[col] * G.beps[col];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + 4 * g + r;
      if (m < M) {
        float v = sum[mt][r] + bias;
        if (a.relu) v = relu_f(v);
        G.y[static_cast<int64_t>(m) * N + col] = v;
      }
    }
}

static int nz_mt(int64_t M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8; }
static int nz_ks(int64_t K) {
  return static_cast<int>(ceil_div(ceil_div(K, 32), kNzWaves * kNzSpan));
}

// ---- backward ------------------------------------------------------------------------------
struct NzBwdGroup {
  const float *x, *g, *y, *mu, *sigma, *eps, *beps;
  float *dmu, *dsigma, *dbmu, *dbsigma, *dx;
  int N, blk0;  // first n block of this group in the grid's y
};
struct NzBwdArgs {
  NzBwdGroup g[2];
  int groups, M, K, nbt, nblk, relu, shared_x;
  float* part;        // [nblk][M][K]
  unsigned* tickets;  // [strip groups]
};

template <int MT, bool DX>
__global__ __launch_bounds__(64 * kNzWaves) void noisy_bwd_kernel(NzBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float nz_smem[];
  __shared__ int s_flag;
  const int blk = blockIdx.y;
  const bool second = a.groups > 1 && blk >= a.g[1].blk0;
  const NzBwdGroup G = second ? a.g[1] : a.g[0];
  const int nbw = a.nbt * 16, ldg = nbw + 4;
  float* gs = nz_smem;                                  // [MT * 16][ldg]: g * (y > 0), zero padded
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* wl = nz_smem + MT * 16 * ldg + wv * 16 * kNzRow;  // this wave's [16][kNzRow] image
  const int g = lane >> 4, c16 = lane & 15;
  const int piece = lane & 7, lsub = lane >> 3;
  const int M = a.M, K = a.K, N = G.N;
  const int n0 = (blk - G.blk0) * nbw;
  const int k0 = (blockIdx.x * kNzWaves + wv) * 32;

  for (int i = threadIdx.x; i < MT * 16 * nbw; i += 64 * kNzWaves) {
    const int m = i / nbw, nn = i - m * nbw, n = n0 + nn;
    float v = 0.f;
    if (m < M && n < N) {
      v = G.g[static_cast<int64_t>(m) * N + n];
      if (a.relu && !(G.y[static_cast<int64_t>(m) * N + n] > 0.f)) v = 0.f;
    }
    gs[m * ldg + nn] = v;
  }
  __syncthreads();
  if (blockIdx.x == 0 && static_cast<int>(threadIdx.x) < nbw && n0 + static_cast<int>(threadIdx.x) < N) {
    float s = 0.f;  // rows in order
    for (int m = 0; m < M; ++m) s += gs[m * ldg + threadIdx.x];
    G.dbmu[n0 + threadIdx.x] = s;
    G.dbsigma[n0 + threadIdx.x] = s * G.beps[n0 + threadIdx.x];
  }

  floatx4 accx[MT][2];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    accx[mt][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    accx[mt][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  if (k0 < K) {  // wave-uniform: this wave has a strip
    // x strip as B fragments of the dmu product: step s, half h: x[4 s + g][k0 + 16 h + c16]
    float xb[MT * 4][2];
#pragma unroll
    for (int s = 0; s < MT * 4; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int m = 4 * s + g, k = k0 + 16 * h + c16;
        xb[s][h] = (m < M && k < K) ? G.x[static_cast<int64_t>(m) * K + k] : 0.f;
      }
    const int kk = k0 + piece * 4;
    for (int nt = 0; nt < a.nbt && n0 + nt * 16 < N; ++nt) {
      float4 ep[2], wq[2];
      bool ok[2];
      int64_t off[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int n = n0 + nt * 16 + i * 8 + lsub;
        ok[i] = n < N && kk < K;
        off[i] = static_cast<int64_t>(ok[i] ? n : 0) * K + (ok[i] ? kk : 0);
        ep[i] = ld4(G.eps + off[i], ok[i]);
        if (DX) wq[i] = noisy_w(ld4(G.mu + off[i], ok[i]), ld4(G.sigma + off[i], ok[i]), ep[i]);
      }
      // dmu tile: rows n (A = g^T from LDS), columns k (B = the x strip), reduction over m
      floatx4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < MT * 4; ++s) {
        const float ga = gs[(4 * s + g) * ldg + nt * 16 + c16];
        d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, xb[s][0], d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, xb[s][1], d1, 0, 0, 0);
      }
      // C layout (column k = lane & 15, rows n = 4 g + r) -> line layout through the LDS image
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        wl[(4 * g + r) * kNzRow + c16] = d0[r];
        wl[(4 * g + r) * kNzRow + 16 + c16] = d1[r];
      }
      wave_lds_fence();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float4 d = *reinterpret_cast<const float4*>(&wl[(i * 8 + lsub) * kNzRow + piece * 4]);
        if (ok[i]) {
          *reinterpret_cast<float4*>(G.dmu + off[i]) = d;
          *reinterpret_cast<float4*>(G.dsigma + off[i]) =
              make_float4(d.x * ep[i].x, d.y * ep[i].y, d.z * ep[i].z, d.w * ep[i].w);
        }
      }
      wave_lds_fence();
      if (DX) {  // dx[:, strip] += g w: w back through the image as B fragments (rows n = 4 g + j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          *reinterpret_cast<float4*>(&wl[(i * 8 + lsub) * kNzRow + piece * 4]) = wq[i];
        wave_lds_fence();
        float bw[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bw[j][0] = wl[(4 * g + j) * kNzRow + c16];
          bw[j][1] = wl[(4 * g + j) * kNzRow + 16 + c16];
        }
        wave_lds_fence();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const float4 ga = *reinterpret_cast<const float4*>(&gs[(mt * 16 + c16) * ldg + nt * 16 + 4 * g]);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            floatx4& c = accx[mt][h];
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(ga.x, bw[0][h], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(ga.y, bw[1][h], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(ga.z, bw[2][h], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(ga.w, bw[3][h], c, 0, 0, 0);
          }
        }
      }
    }
    if (DX) {  // this n block's partial dx[:, strip]
      float* p = a.part + static_cast<int64_t>(blk) * M * K;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mt * 16 + 4 * g + r, k = k0 + 16 * h + c16;
            if (m < M && k < K) st_agent(p + static_cast<int64_t>(m) * K + k, accx[mt][h][r]);
          }
    }
  }
  if (!DX) return;
  if (!arrive_last(a.tickets + blockIdx.x, gridDim.y, &s_flag)) return;
  // n blocks in block order over this strip group's 128 columns (K % 4 == 0: whole float4s)
  const int kg0 = blockIdx.x * kNzWaves * 32;
  const int kw = (K - kg0 < kNzWaves * 32 ? K - kg0 : kNzWaves * 32) / 4;  // float4s per row
  const int64_t MK = static_cast<int64_t>(M) * K;
  for (int gi = 0; gi < (a.shared_x ? 1 : a.groups); ++gi) {
    const int b0 = a.shared_x ? 0 : a.g[gi].blk0;
    const int b1 = a.shared_x || gi + 1 == a.groups ? a.nblk : a.g[gi + 1].blk0;
    float* dx = a.g[gi].dx;
    for (int i = threadIdx.x; i < M * kw; i += 64 * kNzWaves) {
      const int m = i / kw, k = kg0 + 4 * (i - m * kw);
      const int64_t o = static_cast<int64_t>(m) * K + k;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int b = b0; b < b1; ++b) {
        const float* v = a.part + b * MK + o;
        s.x += ld_agent(v); s.y += ld_agent(v + 1); s.z += ld_agent(v + 2); s.w += ld_agent(v + 3);
      }
      *reinterpret_cast<float4*>(dx + o) = s;
    }
  }
}

// n tiles per block: 4 (64 rows share one g block and one partial dx) once that still gives the
// grid a workgroup per CU, else 1
static int nz_nbt(int64_t K, int64_t ntot) {
  return ceil_div(K, kNzWaves * 32) * ceil_div(ntot, 64) >= 256 ? 4 : 1;
}

static bool nz_al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static int nz_check(const char* who, const ocppo_noisy_layer_t* L, int64_t groups, int64_t M,
                    int64_t K) {
  OCPPO_REQUIRE(L != nullptr && (groups == 1 || groups == 2), "%s: 1 or 2 layer groups", who);
  OCPPO_REQUIRE(M >= 1 && M <= kNzMaxM && K >= 4 && K % 4 == 0 && K <= (1 << 19),
                "%s: bad sizes M=%lld K=%lld (1 <= M <= 128, K %% 4 == 0)", who, (long long)M,
                (long long)K);
  for (int i = 0; i < groups; ++i) {
    OCPPO_REQUIRE(L[i].N >= 1 && L[i].N <= (1 << 20) && L[i].N * K <= INT32_MAX,
                  "%s: group %d: bad N=%lld", who, i, (long long)L[i].N);
    OCPPO_REQUIRE(L[i].x && L[i].mu && L[i].sigma && L[i].eps && L[i].beps,
                  "%s: group %d: null pointer", who, i);
    OCPPO_REQUIRE(nz_al16(L[i].x) && nz_al16(L[i].mu) && nz_al16(L[i].sigma) && nz_al16(L[i].eps),
                  "%s: group %d: x, mu, sigma and eps must be 16-byte aligned", who, i);
  }
  return OCPPO_OK;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_noisy_linear_workspace_bytes(int64_t M, int64_t K, int64_t N0, int64_t N1,
                                                     int backward) {
  if (M < 1 || M > kNzMaxM || K < 4 || K % 4 != 0 || N0 < 1 || N1 < 0) return 0;
  if (!backward) {
    const int64_t tiles = ceil_div(N0, 16) + ceil_div(N1, 16);
    if (tiles * 4 > kNzTicketBytes) return 0;
    const int ks = nz_ks(K);
    return kNzTicketBytes + (ks > 1 ? ks * tiles * nz_mt(M) * 64 * sizeof(floatx4) : 0);
  }
  if (ceil_div(K, kNzWaves * 32) * 4 > kNzTicketBytes) return 0;
  const int nbw = 16 * nz_nbt(K, N0 + N1);
  const int64_t nblk = ceil_div(N0, nbw) + ceil_div(N1, nbw);
  return kNzTicketBytes + nblk * M * K * sizeof(float);
}

extern "C" int ocppo_noisy_linear_fwd(ocppo_stream_t stream, const ocppo_noisy_layer_t* layers,
                                      int64_t groups, int64_t M, int64_t K, int relu,
                                      void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_noisy_linear_fwd";
  if (int rc = nz_check(who, layers, groups, M, K)) return rc;
  NzFwdArgs a;
  a.groups = (int)groups; a.M = (int)M; a.K = (int)K; a.relu = relu; a.KS = nz_ks(K);
  int tiles = 0;
  for (int i = 0; i < 2; ++i) {
    const ocppo_noisy_layer_t& L = layers[i < groups ? i : 0];
    OCPPO_REQUIRE(L.bmu && L.bsigma && L.y, "%s: group %d: null pointer", who, i);
    a.g[i] = NzFwdGroup{L.x, L.mu, L.sigma, L.eps, L.bmu, L.bsigma, L.beps, L.y, (int)L.N, tiles};
    if (i < groups) tiles += (int)ceil_div(L.N, 16);
  }
  a.tiles = tiles;
  const size_t need = ocppo_noisy_linear_workspace_bytes(M, K, layers[0].N,
                                                         groups > 1 ? layers[1].N : 0, 0);
  if (need == 0) return fail(OCPPO_E_INVALID, "%s: too many column tiles", who);
  if (!workspace || workspace_bytes < need || !nz_al16(workspace))
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes needed (zeroed once)", who, need);
  a.tickets = static_cast<unsigned*>(workspace);
  a.part = reinterpret_cast<floatx4*>(static_cast<char*>(workspace) + kNzTicketBytes);
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  const dim3 grid(tiles, a.KS), block(64 * kNzWaves);
  switch (nz_mt(M)) {
    case 1: hipLaunchKernelGGL(noisy_fwd_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(noisy_fwd_kernel<2>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(noisy_fwd_kernel<4>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(noisy_fwd_kernel<8>, grid, block, 0, s, a); break;
  }
  return check_launch(who);
}

template <bool DX>
static void nz_launch_bwd(hipStream_t s, int mt, dim3 grid, size_t lds, const NzBwdArgs& a) {
  const dim3 block(64 * kNzWaves);
  switch (mt) {
    case 1: hipLaunchKernelGGL((noisy_bwd_kernel<1, DX>), grid, block, lds, s, a); break;
    case 2: hipLaunchKernelGGL((noisy_bwd_kernel<2, DX>), grid, block, lds, s, a); break;
    case 4: hipLaunchKernelGGL((noisy_bwd_kernel<4, DX>), grid, block, lds, s, a); break;
    default: hipLaunchKernelGGL((noisy_bwd_kernel<8, DX>), grid, block, lds, s, a); break;
  }
}

extern "C" int ocppo_noisy_linear_bwd(ocppo_stream_t stream, const ocppo_noisy_layer_t* layers,
                                      int64_t groups, int64_t M, int64_t K, int relu,
                                      int shared_x, void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_noisy_linear_bwd";
  if (int rc = nz_check(who, layers, groups, M, K)) return rc;
  const bool dx = layers[0].dx != nullptr;
  NzBwdArgs a;
  a.groups = (int)groups; a.M = (int)M; a.K = (int)K; a.relu = relu;
  a.shared_x = shared_x || groups == 1;
  a.nbt = nz_nbt(K, layers[0].N + (groups > 1 ? layers[1].N : 0));
  int nblk = 0;
  for (int i = 0; i < 2; ++i) {
    const ocppo_noisy_layer_t& L = layers[i < groups ? i : 0];
    OCPPO_REQUIRE(L.g && L.dmu && L.dsigma && L.dbmu && L.dbsigma && (!relu || L.y),
                  "%s: group %d: null pointer", who, i);
    OCPPO_REQUIRE(nz_al16(L.dmu) && nz_al16(L.dsigma), "%s: group %d: dmu and dsigma must be "
                  "16-byte aligned", who, i);
    OCPPO_REQUIRE((L.dx != nullptr) == dx && (!dx || nz_al16(L.dx)) &&
                      (!shared_x || (L.x == layers[0].x && L.dx == layers[0].dx)),
                  "%s: group %d: dx for all groups or none, 16-byte aligned; one x and one dx "
                  "when x is shared", who, i);
    a.g[i] = NzBwdGroup{L.x, L.g, L.y, L.mu, L.sigma, L.eps, L.beps, L.dmu, L.dsigma, L.dbmu,
                        L.dbsigma, L.dx, (int)L.N, nblk};
    if (i < groups) nblk += (int)ceil_div(L.N, 16 * a.nbt);
  }
  a.nblk = nblk;
  const size_t need = ocppo_noisy_linear_workspace_bytes(M, K, layers[0].N,
                                                         groups > 1 ? layers[1].N : 0, 1);
  OCPPO_REQUIRE(need != 0 && nblk <= 65535, "%s: too large", who);
  if (dx && (!workspace || workspace_bytes < need || !nz_al16(workspace)))
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes needed (zeroed once)", who, need);
  a.tickets = static_cast<unsigned*>(workspace);
  a.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + kNzTicketBytes);
  const int mt = nz_mt(M);
  const size_t lds = sizeof(float) * (mt * 16 * (a.nbt * 16 + 4) + kNzWaves * 16 * kNzRow);
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)ceil_div(K, kNzWaves * 32), nblk);
  if (dx)
    nz_launch_bwd<true>(s, mt, grid, lds, a);
  else
    nz_launch_bwd<false>(s, mt, grid, lds, a);
  return check_launch(who);
}
