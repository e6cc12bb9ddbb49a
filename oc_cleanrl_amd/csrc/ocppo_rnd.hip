// Random Network Distillation (cleanrl/ppo_rnd_envpool.py) beyond PPO: the running statistics of the
// newest frame (gym's RunningMeanStd, :302-303, :333, :444) and the normalisation by them
// (:365-370, :449-454), the curiosity reward (:373), the reward filter + its running variance +
// the division (:390-400), both GAE scans and the combined advantage (:406-442), and the
// intrinsic value loss + masked forward loss with their gradients (:463-472, :509).
//
// Precision. The running statistics are f64 on the device. Every sum that feeds them (sum x, sum
// x^2 per column; x is f32 / bf16 / u8, so x and x^2 are exact in f64) is carried as an unevaluated
// pair hi + lo (TwoSum), so a column's batch mean and population variance come out within an ulp
// of the exact ones whatever the cancellation in E[x^2] - E[x]^2; the merge into the state is then
// the law's own f64 operations in its order. Sums over a batch of losses are f64. Everything
// elementwise that the script does in f32 is f32 op for op (the library builds with
// -ffp-contract=off). No atomics: every sum's order is fixed by the shapes.
//
// Launches. A kernel that hands data to another one does so across a launch boundary: the old
// running count (read by every column's merge, written by one) and the old reward state are
// copied into the workspace by the first launch and read from there by the second.
#include "ocppo_common.h"
#include "ocppo_rng.h"

namespace ocppo {

// the update mask's key: h = splitmix64(splitmix64(seed ^ key) + counter); row r is kept when
// unit53(splitmix64(h + r + 1)) < update_proportion
constexpr uint64_t kRndMaskKey = 0x52E4D0A5C3B17F29ull;
constexpr int kRndThreads = 256;
constexpr int kRndWsHeader = 8;  // doubles in front of a workspace's partials

// ---- hi + lo pairs -----------------------------------------------------------------------------------
struct dd {
  double hi, lo;
};
__device__ __forceinline__ dd dd_norm(double s, double e) {
  const double hi = s + e;
  return dd{hi, e - (hi - s)};
}
__device__ __forceinline__ dd dd_add_d(dd a, double b) {
  const double s = a.hi + b, bb = s - a.hi;
  const double e = (a.hi - (s - bb)) + (b - bb);
  return dd_norm(s, e + a.lo);
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
  const double s = a.hi + b.hi, bb = s - a.hi;
  const double e = (a.hi - (s - bb)) + (b.hi - bb);
  return dd_norm(s, e + (a.lo + b.lo));
}
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
  const double p = a.hi * b.hi;
  const double e = fma(a.hi, b.hi, -p);
  return dd_norm(p, e + (a.hi * b.lo + a.lo * b.hi));
}
__device__ __forceinline__ dd dd_div_d(dd a, double n) {
  const double q1 = a.hi / n;
  const double p = q1 * n;
  const double e = fma(q1, n, -p);
  const double r = ((a.hi - p) - e) + a.lo;
  return dd_norm(q1, r / n);
}
// (mean, population variance) of n values from their sum and sum of squares
__device__ __forceinline__ void dd_moments(dd s, dd q, double n, double& mean, double& var) {
  const dd m = dd_div_d(s, n);
  const dd m2 = dd_mul(m, m);
  const dd v = dd_add(dd_div_d(q, n), dd{-m2.hi, -m2.lo});
  mean = m.hi;
  var = v.hi > 0.0 ? v.hi : 0.0;
}

// gym's RunningMeanStd.update_from_moments, op for op in f64
__device__ __forceinline__ void rms_merge(double mean, double var, double count, double bm,
                                          double bv, double bc, double& nmean, double& nvar,
                                          double& ncount) {
  const double delta = bm - mean;
  const double tot = count + bc;
  nmean = mean + delta * bc / tot;
  const double m_a = var * count;
  const double m_b = bv * bc;
  const double m2 = m_a + m_b + delta * delta * count * bc / tot;
  nvar = m2 / tot;
  ncount = tot;
}

// The sum over the 256 threads' pairs that share a column: threads are (ry, cx) = (tid >> cwl,
// tid & (CW - 1)), a tree over ry in a fixed order; the result is in the threads with ry == 0.
__device__ __forceinline__ void dd_tree(dd& s, dd& q, double (*sh)[kRndThreads], int cwl) {
  const int tid = threadIdx.x, ry = tid >> cwl;
  sh[0][tid] = s.hi;
  sh[1][tid] = s.lo;
  sh[2][tid] = q.hi;
  sh[3][tid] = q.lo;
  for (int st = (kRndThreads >> cwl) / 2; st >= 1; st >>= 1) {
    __syncthreads();
    if (ry < st) {
      const int o = tid + (st << cwl);
      s = dd_add(s, dd{sh[0][o], sh[1][o]});
      q = dd_add(q, dd{sh[2][o], sh[3][o]});
      sh[0][tid] = s.hi;
      sh[1][tid] = s.lo;
      sh[2][tid] = q.hi;
      sh[3][tid] = q.lo;
    }
  }
}

// ---- 1. running statistics ----------------------------------------------------------------------
// grid (column blocks of CW = 2^cwl columns, row chunks): per (chunk, column) the pairs of sum x
// and sum x^2 -> ws[header + (chunk * C + c) * 4 ..]; block (0, 0) keeps the old count in ws[0]
template <int DT>
__global__ __launch_bounds__(kRndThreads) void rms_partial_kernel(
    const void* __restrict__ x, int64_t R, int64_t C, int64_t ld, int cwl, int64_t rpc,
    const double* __restrict__ state, double* __restrict__ ws) {
  __shared__ double sh[4][kRndThreads];
  const int tid = threadIdx.x, cx = tid & ((1 << cwl) - 1), ry = tid >> cwl;
  const int RY = kRndThreads >> cwl;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) << cwl) + cx;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpc;
  const int64_t r1 = r0 + rpc < R ? r0 + rpc : R;
  const typename Elem<DT>::T* p = static_cast<const typename Elem<DT>::T*>(x);
  dd s{0.0, 0.0}, q{0.0, 0.0};
  if (c < C)
    for (int64_t r = r0 + ry; r < r1; r += RY) {
      const double v = static_cast<double>(Elem<DT>::load(p, r * ld + c));
      s = dd_add_d(s, v);
      q = dd_add_d(q, v * v);
    }
  dd_tree(s, q, sh, cwl);
  if (ry == 0 && c < C) {
    double* o = ws + kRndWsHeader + (static_cast<int64_t>(blockIdx.y) * C + c) * 4;
    o[0] = s.hi;
    o[1] = s.lo;
    o[2] = q.hi;
    o[3] = q.lo;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) ws[0] = state[2 * C];
}

__global__ __launch_bounds__(kRndThreads) void rms_finish_kernel(const double* __restrict__ ws,
                                                                 int64_t chunks, int64_t R,
                                                                 int64_t C,
                                                                 double* __restrict__ state) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kRndThreads + threadIdx.x;
  if (c >= C) return;
  dd s{0.0, 0.0}, q{0.0, 0.0};
  for (int64_t k = 0; k < chunks; ++k) {
    const double* o = ws + kRndWsHeader + (k * C + c) * 4;
    s = dd_add(s, dd{o[0], o[1]});
    q = dd_add(q, dd{o[2], o[3]});
  }
  double bm, bv, nm, nv, nc;
  dd_moments(s, q, static_cast<double>(R), bm, bv);
  rms_merge(state[c], state[C + c], ws[0], bm, bv, static_cast<double>(R), nm, nv, nc);
  state[c] = nm;
  state[C + c] = nv;
  if (c == 0) state[2 * C] = nc;
}

// ---- 2. normalisation ------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kRndThreads) void rnd_normalize_kernel(
    const void* __restrict__ x, int64_t R, int64_t C, int64_t ld, int cwl, int64_t rpc,
    const double* __restrict__ state, float* __restrict__ out) {
  const int tid = threadIdx.x, cx = tid & ((1 << cwl) - 1), ry = tid >> cwl;
  const int RY = kRndThreads >> cwl;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) << cwl) + cx;
  if (c >= C) return;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rpc;
  const int64_t r1 = r0 + rpc < R ? r0 + rpc : R;
  const typename Elem<DT>::T* p = static_cast<const typename Elem<DT>::T*>(x);
  const double mean = state[c], sd = sqrt(state[C + c]);
  for (int64_t r = r0 + ry; r < r1; r += RY) {
    double v = (static_cast<double>(Elem<DT>::load(p, r * ld + c)) - mean) / sd;
    v = v != v ? v : fmin(fmax(v, -5.0), 5.0);  // clip keeps a NaN
    out[r * C + c] = static_cast<float>(v);
  }
}

// ---- 3. curiosity -------------------------------------------------------------------------------------
// one wave per row: d = t - p in f32 (the script's op), d^2 exact in f64, one rounding of the sum
__global__ __launch_bounds__(kRndThreads) void rnd_error_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ target,
                                                                int64_t R, int64_t D,
                                                                float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wpb = kRndThreads / kWave;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * wpb + threadIdx.x / kWave; r < R;
       r += static_cast<int64_t>(gridDim.x) * wpb) {
    double acc = 0.0;
    for (int64_t j = lane; j < D; j += kWave) {
      const float d = target[r * D + j] - pred[r * D + j];
      acc += static_cast<double>(d) * static_cast<double>(d);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[r] = static_cast<float>(acc) / 2.0f;
  }
}

// ---- 4. reward filter + running variance + division -----------------------------------------
// thread t walks the envs: rewems[t] = rewems[t] * g + cur[t, n], n = 0 .. N-1 (the script's
// RewardForwardFilter over curiosity_rewards.T), the filtered values' sum and sum of squares as
// pairs per block -> ws; block 0 keeps the old state in ws[0..2]
__global__ __launch_bounds__(kRndThreads) void rnd_filter_kernel(
    const float* __restrict__ cur, float* __restrict__ rewems, int64_t T, int64_t N, float g,
    const double* __restrict__ state, double* __restrict__ ws, float* __restrict__ filtered) {
  __shared__ double sh[4][kRndThreads];
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kRndThreads + threadIdx.x;
  dd s{0.0, 0.0}, q{0.0, 0.0};
  if (t < T) {
    float rw = rewems[t];
    for (int64_t n = 0; n < N; ++n) {
      const float m = rw * g;
      rw = m + cur[t * N + n];
      const double v = static_cast<double>(rw);
      s = dd_add_d(s, v);
      q = dd_add_d(q, v * v);
      if (filtered) filtered[n * T + t] = rw;
    }
    rewems[t] = rw;
  }
  dd_tree(s, q, sh, 0);
  if (threadIdx.x == 0) {
    double* o = ws + kRndWsHeader + static_cast<int64_t>(blockIdx.x) * 4;
    o[0] = s.hi;
    o[1] = s.lo;
    o[2] = q.hi;
    o[3] = q.lo;
    if (blockIdx.x == 0) {
      ws[0] = state[0];
      ws[1] = state[1];
      ws[2] = state[2];
    }
  }
}

__global__ __launch_bounds__(kRndThreads) void rnd_reward_finish_kernel(
    float* __restrict__ cur, int64_t T, int64_t N, int64_t nblk, const double* __restrict__ ws,
    double* __restrict__ state) {
  __shared__ float s_sd;
  if (threadIdx.x == 0) {
    dd s{0.0, 0.0}, q{0.0, 0.0};
    for (int64_t k = 0; k < nblk; ++k) {
      const double* o = ws + kRndWsHeader + k * 4;
      s = dd_add(s, dd{o[0], o[1]});
      q = dd_add(q, dd{o[2], o[3]});
    }
    double bm, bv, nm, nv, nc;
    dd_moments(s, q, static_cast<double>(T) * static_cast<double>(N), bm, bv);
    // update_from_moments(mean, std^2, count = len() of the [N, T] array = N)
    rms_merge(ws[0], ws[1], ws[2], bm, bv, static_cast<double>(N), nm, nv, nc);
    s_sd = static_cast<float>(sqrt(nv));
    if (blockIdx.x == 0) {
      state[0] = nm;
      state[1] = nv;
      state[2] = nc;
    }
  }
  __syncthreads();
  const float sd = s_sd;
  const int64_t n = T * N;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kRndThreads + threadIdx.x; e < n;
       e += static_cast<int64_t>(gridDim.x) * kRndThreads)
    cur[e] = cur[e] / sd;
}

// ---- 5. both GAE scans ----------------------------------------------------------------------------
// one thread per env, the two recurrences side by side (two independent chains of two dependent
// f32 ops per step), U rows of operands loaded per batch; op for op ocppo_gae's arithmetic (the
// intrinsic scan with nonterminal 1: x * 1.0f is x), then the combined advantage
// (ia * f32(int_coef)) + (ea * f32(ext_coef)).
struct RndGaeArgs {
  const float *rew, *ev, *don, *next_ev, *next_done, *cur, *iv, *next_iv;
  float *eadv, *eret, *iadv, *iret, *adv;
  float g, gl, ig, igl, ic, ec;
};

template <int U>
__global__ __launch_bounds__(kWave) void rnd_gae_kernel(RndGaeArgs a, int T, int64_t N) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float elast = 0.f, ilast = 0.f;
  float cev = a.next_ev[n], cd = a.next_done[n], civ = a.next_iv[n];
  for (int t_hi = T; t_hi > 0; t_hi -= U) {
    const int rows = t_hi < U ? t_hi : U;
    float r[U], v[U], d[U], c[U], w[U];
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (k < rows) {
        const size_t gi = static_cast<size_t>(t_hi - 1 - k) * N + n;
        r[k] = a.rew[gi];
        v[k] = a.ev[gi];
        d[k] = a.don[gi];
        c[k] = a.cur[gi];
        w[k] = a.iv[gi];
      }
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (k < rows) {
        const float nnt = 1.0f - cd;
        float ed = r[k] + (a.g * cev) * nnt;
        ed = ed - v[k];
        elast = ed + (a.gl * nnt) * elast;
        float id = c[k] + (a.ig * civ) * 1.0f;
        id = id - w[k];
        ilast = id + (a.igl * 1.0f) * ilast;
        cev = v[k];
        cd = d[k];
        civ = w[k];
        r[k] = elast;
        c[k] = ilast;
      }
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (k < rows) {
        const size_t gi = static_cast<size_t>(t_hi - 1 - k) * N + n;
        a.eadv[gi] = r[k];
        a.eret[gi] = r[k] + v[k];
        a.iadv[gi] = c[k];
        a.iret[gi] = c[k] + w[k];
        a.adv[gi] = c[k] * a.ic + r[k] * a.ec;
      }
  }
}

// ---- 6. intrinsic value loss + masked forward loss ------------------------------------------------
__device__ __forceinline__ uint64_t rnd_mask_hash(uint64_t seed, int64_t counter) {
  return splitmix64(splitmix64(seed ^ kRndMaskKey) + static_cast<uint64_t>(counter));
}
__device__ __forceinline__ bool rnd_mask_row(uint64_t h, int64_t r, double prop) {
  return unit53(splitmix64(h + static_cast<uint64_t>(r) + 1)) < prop;
}

__global__ __launch_bounds__(kRndThreads) void rnd_mask_kernel(uint64_t seed,
                                                               const int64_t* __restrict__ counter,
                                                               int64_t M, double prop,
                                                               float* __restrict__ out) {
  const uint64_t h = rnd_mask_hash(seed, counter[0]);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kRndThreads + threadIdx.x; r < M;
       r += static_cast<int64_t>(gridDim.x) * kRndThreads)
    out[r] = rnd_mask_row(h, r, prop) ? 1.0f : 0.0f;
}

// Every block counts the kept rows itself (the mask depends on seed, counter and row only), then
// one wave per row: d = p - t, the row's mean d^2, dpred = d * (2 / (D * max(count, 1))) on kept
// rows and d * 0 on the others; lane 0 takes the row's value error. Per wave the f64 partials
// {sum (v - ret)^2, sum kept mean d^2} -> ws[header + (block * 4 + wave) * 2 ..]; ws[1] = count.
__global__ __launch_bounds__(kRndThreads) void rnd_aux_kernel(
    const float* __restrict__ pred, const float* __restrict__ target,
    const float* __restrict__ v_int, const float* __restrict__ ret_int, int64_t M, int64_t D,
    uint64_t seed, const int64_t* __restrict__ counter, double prop, float vscale,
    float* __restrict__ dpred, float* __restrict__ dv_int, double* __restrict__ ws) {
  __shared__ double scratch[kRndThreads / kWave];
  const uint64_t h = rnd_mask_hash(seed, counter[0]);
  double cnt = 0.0;
  for (int64_t r = threadIdx.x; r < M; r += kRndThreads) cnt += rnd_mask_row(h, r, prop) ? 1.0 : 0.0;
  cnt = block_sum(cnt, scratch);
  const float pscale =
      static_cast<float>(2.0 / (static_cast<double>(D) * (cnt > 1.0 ? cnt : 1.0)));
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int64_t wpb = kRndThreads / kWave;
  double vl = 0.0, fl = 0.0;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * wpb + wid; r < M;
       r += static_cast<int64_t>(gridDim.x) * wpb) {
    const bool keep = rnd_mask_row(h, r, prop);
    const float sc = keep ? pscale : 0.0f;
    double acc = 0.0;
    for (int64_t j = lane; j < D; j += kWave) {
      const float d = pred[r * D + j] - target[r * D + j];
      acc += static_cast<double>(d) * static_cast<double>(d);
      dpred[r * D + j] = d * sc;
    }
    acc = wave_sum(acc);
    if (keep) fl += acc / static_cast<double>(D);
    if (lane == 0) {
      const float dv = v_int[r] - ret_int[r];
      vl += static_cast<double>(dv) * static_cast<double>(dv);
      dv_int[r] = dv * vscale;
    }
  }
  if (lane == 0) {
    double* o = ws + kRndWsHeader + (static_cast<int64_t>(blockIdx.x) * wpb + wid) * 2;
    o[0] = vl;
    o[1] = fl;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ws[1] = cnt;
}

// stats = {0.5 mean (v - ret)^2, sum kept row losses / max(count, 1), count}; the counter advances
__global__ __launch_bounds__(kRndThreads) void rnd_aux_finish_kernel(const double* __restrict__ ws,
                                                                     int64_t nparts, int64_t M,
                                                                     float* __restrict__ stats,
                                                                     int64_t* __restrict__ counter) {
  __shared__ double scratch[kRndThreads / kWave];
  double vl = 0.0, fl = 0.0;
  for (int64_t k = threadIdx.x; k < nparts; k += kRndThreads) {
    vl += ws[kRndWsHeader + k * 2];
    fl += ws[kRndWsHeader + k * 2 + 1];
  }
  vl = block_sum(vl, scratch);
  fl = block_sum(fl, scratch);
  if (threadIdx.x == 0) {
    const double cnt = ws[1];
    stats[0] = static_cast<float>(0.5 * vl / static_cast<double>(M));
    stats[1] = static_cast<float>(fl / (cnt > 1.0 ? cnt : 1.0));
    stats[2] = static_cast<float>(cnt);
    counter[0] = counter[0] + 1;
  }
}

// ---- host side -------------------------------------------------------------------------------------------
constexpr int64_t kRmsMaxChunks = 128;
constexpr int64_t kRndMaxCols = int64_t{1} << 20;

struct RmsGeom {
  int cwl;           // log2 of the column block
  int64_t rpc;       // rows per chunk
  int64_t chunks, colblocks;
};

static RmsGeom rms_geom(int64_t R, int64_t C) {
  RmsGeom g;
  g.cwl = 0;
  while ((1 << g.cwl) < 64 && (int64_t{1} << g.cwl) < C) ++g.cwl;
  const int64_t ry = kRndThreads >> g.cwl;
  g.rpc = ry * 16;
  g.chunks = ceil_div(R, g.rpc);
  if (g.chunks > kRmsMaxChunks) {
    g.rpc = ceil_div(R, kRmsMaxChunks);
    g.chunks = ceil_div(R, g.rpc);
  }
  g.colblocks = ceil_div(C, int64_t{1} << g.cwl);
  return g;
}

static int rms_sizes(const char* who, int64_t R, int64_t C, int64_t ld, int dtype) {
  OCPPO_REQUIRE(R >= 1 && C >= 1 && C <= kRndMaxCols && ld >= C,
                "%s: bad sizes R=%lld C=%lld row_stride=%lld (R >= 1, 1 <= C <= %lld, "
                "row_stride >= C)",
                who, (long long)R, (long long)C, (long long)ld, (long long)kRndMaxCols);
  OCPPO_REQUIRE(dtype == OCPPO_F32 || dtype == OCPPO_BF16 || dtype == OCPPO_U8,
                "%s: dtype %d is not OCPPO_F32 / OCPPO_BF16 / OCPPO_U8", who, dtype);
  return OCPPO_OK;
}

static int64_t aux_grid(int64_t M) {
  const int64_t g = ceil_div(M, kRndThreads / kWave);
  return g < 1024 ? g : 1024;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_rms_update_workspace_bytes(int64_t R, int64_t C) {
  if (R < 1 || C < 1 || C > kRndMaxCols) return 0;
  const RmsGeom g = rms_geom(R, C);
  return static_cast<size_t>(kRndWsHeader + g.chunks * C * 4) * sizeof(double);
}

extern "C" int ocppo_rms_update(ocppo_stream_t stream, const void* x, int dtype, int64_t R,
                                int64_t C, int64_t row_stride, double* state, void* workspace,
                                size_t workspace_bytes) {
  if (int rc = rms_sizes("ocppo_rms_update", R, C, row_stride, dtype)) return rc;
  OCPPO_REQUIRE(x && state && workspace, "ocppo_rms_update: null pointer");
  if (workspace_bytes < ocppo_rms_update_workspace_bytes(R, C) ||
      reinterpret_cast<uintptr_t>(workspace) % 8)
    return fail(OCPPO_E_WORKSPACE, "ocppo_rms_update: workspace of %zu bytes (8-B aligned) needed",
                ocppo_rms_update_workspace_bytes(R, C));
  const RmsGeom g = rms_geom(R, C);
  double* ws = static_cast<double*>(workspace);
  hipStream_t s = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(g.colblocks), static_cast<unsigned>(g.chunks));
  clear_stale_error();
#define OCPPO_RMS_PARTIAL(DT)                                                                     \
  hipLaunchKernelGGL(rms_partial_kernel<DT>, grid, dim3(kRndThreads), 0, s, x, R, C, row_stride, \
                     g.cwl, g.rpc, state, ws)
  if (dtype == OCPPO_F32) OCPPO_RMS_PARTIAL(OCPPO_F32);
  else if (dtype == OCPPO_BF16) OCPPO_RMS_PARTIAL(OCPPO_BF16);
  else OCPPO_RMS_PARTIAL(OCPPO_U8);
#undef OCPPO_RMS_PARTIAL
  if (int rc = check_launch("ocppo_rms_update")) return rc;
  hipLaunchKernelGGL(rms_finish_kernel, dim3(ceil_div(C, kRndThreads)), dim3(kRndThreads), 0, s,
                     ws, g.chunks, R, C, state);
  return check_launch("ocppo_rms_update (finish)");
}

extern "C" int ocppo_rnd_normalize(ocppo_stream_t stream, const void* x, int dtype, int64_t R,
                                   int64_t C, int64_t row_stride, const double* state,
                                   float* out) {
  if (int rc = rms_sizes("ocppo_rnd_normalize", R, C, row_stride, dtype)) return rc;
  OCPPO_REQUIRE(x && state && out, "ocppo_rnd_normalize: null pointer");
  const RmsGeom g = rms_geom(R, C);
  hipStream_t s = as_stream(stream);
  const dim3 grid(static_cast<unsigned>(g.colblocks), static_cast<unsigned>(g.chunks));
  clear_stale_error();
#define OCPPO_RND_NORMALIZE(DT)                                                                   \
  hipLaunchKernelGGL(rnd_normalize_kernel<DT>, grid, dim3(kRndThreads), 0, s, x, R, C,           \
                     row_stride, g.cwl, g.rpc, state, out)
  if (dtype == OCPPO_F32) OCPPO_RND_NORMALIZE(OCPPO_F32);
  else if (dtype == OCPPO_BF16) OCPPO_RND_NORMALIZE(OCPPO_BF16);
  else OCPPO_RND_NORMALIZE(OCPPO_U8);
#undef OCPPO_RND_NORMALIZE
  return check_launch("ocppo_rnd_normalize");
}

extern "C" int ocppo_rnd_error(ocppo_stream_t stream, const float* pred, const float* target,
                               int64_t R, int64_t D, float* out) {
  OCPPO_REQUIRE(R >= 0 && D >= 1, "ocppo_rnd_error: bad sizes R=%lld D=%lld (R >= 0, D >= 1)",
                (long long)R, (long long)D);
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(pred && target && out, "ocppo_rnd_error: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(rnd_error_kernel, dim3(grid_for(R * kWave, kRndThreads)), dim3(kRndThreads),
                     0, as_stream(stream), pred, target, R, D, out);
  return check_launch("ocppo_rnd_error");
}

extern "C" size_t ocppo_rnd_reward_norm_workspace_bytes(int64_t T) {
  if (T < 1) return 0;
  return static_cast<size_t>(kRndWsHeader + ceil_div(T, kRndThreads) * 4) * sizeof(double);
}

extern "C" int ocppo_rnd_reward_norm(ocppo_stream_t stream, float* curiosity, float* rewems,
                                     double* state, int64_t T, int64_t N, double int_gamma,
                                     void* workspace, size_t workspace_bytes, float* filtered) {
  OCPPO_REQUIRE(T >= 1 && N >= 1 && T <= INT32_MAX && N <= INT32_MAX,
                "ocppo_rnd_reward_norm: bad sizes T=%lld N=%lld", (long long)T, (long long)N);
  OCPPO_REQUIRE(curiosity && rewems && state && workspace,
                "ocppo_rnd_reward_norm: null pointer");
  if (workspace_bytes < ocppo_rnd_reward_norm_workspace_bytes(T) ||
      reinterpret_cast<uintptr_t>(workspace) % 8)
    return fail(OCPPO_E_WORKSPACE,
                "ocppo_rnd_reward_norm: workspace of %zu bytes (8-B aligned) needed",
                ocppo_rnd_reward_norm_workspace_bytes(T));
  double* ws = static_cast<double*>(workspace);
  const int64_t nblk = ceil_div(T, kRndThreads);
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  // numpy keeps `rewems * gamma` in f32: the Python float rounds to f32(gamma)
  hipLaunchKernelGGL(rnd_filter_kernel, dim3(static_cast<unsigned>(nblk)), dim3(kRndThreads), 0, s,
                     curiosity, rewems, T, N, static_cast<float>(int_gamma), state, ws, filtered);
  if (int rc = check_launch("ocppo_rnd_reward_norm")) return rc;
  hipLaunchKernelGGL(rnd_reward_finish_kernel, dim3(grid_for(T * N, kRndThreads)),
                     dim3(kRndThreads), 0, s, curiosity, T, N, nblk, ws, state);
  return check_launch("ocppo_rnd_reward_norm (finish)");
}

extern "C" int ocppo_rnd_gae(ocppo_stream_t stream, const float* rewards, const float* ext_values,
                             const float* dones, const float* next_ext_value,
                             const float* next_done, const float* curiosity,
                             const float* int_values, const float* next_int_value, int64_t T,
                             int64_t N, double gamma, double int_gamma, double gae_lambda,
                             double int_coef, double ext_coef, float* ext_advantages,
                             float* ext_returns, float* int_advantages, float* int_returns,
                             float* advantages) {
  OCPPO_REQUIRE(T >= 0 && N >= 0 && T <= INT32_MAX, "ocppo_rnd_gae: bad sizes T=%lld N=%lld",
                (long long)T, (long long)N);
  if (T == 0 || N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(rewards && ext_values && dones && next_ext_value && next_done && curiosity &&
                    int_values && next_int_value && ext_advantages && ext_returns &&
                    int_advantages && int_returns && advantages,
                "ocppo_rnd_gae: null pointer");
  // the Python floats' products are taken in double, then rounded to f32 by the tensor op
  RndGaeArgs a{rewards, ext_values, dones, next_ext_value, next_done, curiosity, int_values,
               next_int_value, ext_advantages, ext_returns, int_advantages, int_returns,
               advantages, static_cast<float>(gamma), static_cast<float>(gamma * gae_lambda),
               static_cast<float>(int_gamma), static_cast<float>(int_gamma * gae_lambda * 1.0),
               static_cast<float>(int_coef), static_cast<float>(ext_coef)};
  clear_stale_error();
  hipLaunchKernelGGL(rnd_gae_kernel<8>, dim3(static_cast<unsigned>(ceil_div(N, kWave))),
                     dim3(kWave), 0, as_stream(stream), a, static_cast<int>(T), N);
  return check_launch("ocppo_rnd_gae");
}

extern "C" size_t ocppo_rnd_aux_loss_workspace_bytes(int64_t M) {
  if (M < 1) return 0;
  return static_cast<size_t>(kRndWsHeader + aux_grid(M) * (kRndThreads / kWave) * 2) *
         sizeof(double);
}

static int rnd_prop(const char* who, double p) {
  OCPPO_REQUIRE(p >= 0.0 && p <= 1.0, "%s: update_proportion %g outside [0, 1]", who, p);
  return OCPPO_OK;
}

extern "C" int ocppo_rnd_aux_loss_fwd_bwd(ocppo_stream_t stream, const float* pred,
                                          const float* target, const float* v_int,
                                          const float* ret_int, int64_t M, int64_t D,
                                          uint64_t seed, int64_t* counter,
                                          double update_proportion, double vf_coef, float* dpred,
                                          float* dv_int, float* stats, void* workspace,
                                          size_t workspace_bytes) {
  OCPPO_REQUIRE(M >= 1 && D >= 1, "ocppo_rnd_aux_loss_fwd_bwd: bad sizes M=%lld D=%lld",
                (long long)M, (long long)D);
  if (int rc = rnd_prop("ocppo_rnd_aux_loss_fwd_bwd", update_proportion)) return rc;
  OCPPO_REQUIRE(pred && target && v_int && ret_int && counter && dpred && dv_int && stats &&
                    workspace,
                "ocppo_rnd_aux_loss_fwd_bwd: null pointer");
  if (workspace_bytes < ocppo_rnd_aux_loss_workspace_bytes(M) ||
      reinterpret_cast<uintptr_t>(workspace) % 8)
    return fail(OCPPO_E_WORKSPACE,
                "ocppo_rnd_aux_loss_fwd_bwd: workspace of %zu bytes (8-B aligned) needed",
                ocppo_rnd_aux_loss_workspace_bytes(M));
  double* ws = static_cast<double*>(workspace);
  const int64_t grid = aux_grid(M);
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  hipLaunchKernelGGL(rnd_aux_kernel, dim3(static_cast<unsigned>(grid)), dim3(kRndThreads), 0, s,
                     pred, target, v_int, ret_int, M, D, seed, counter, update_proportion,
                     static_cast<float>(vf_coef / static_cast<double>(M)), dpred, dv_int, ws);
  if (int rc = check_launch("ocppo_rnd_aux_loss_fwd_bwd")) return rc;
  hipLaunchKernelGGL(rnd_aux_finish_kernel, dim3(1), dim3(kRndThreads), 0, s, ws,
                     grid * (kRndThreads / kWave), M, stats, counter);
  return check_launch("ocppo_rnd_aux_loss_fwd_bwd (finish)");
}

extern "C" int ocppo_rnd_mask(ocppo_stream_t stream, uint64_t seed, const int64_t* counter,
                              int64_t M, double update_proportion, float* out) {
  OCPPO_REQUIRE(M >= 0, "ocppo_rnd_mask: bad size M=%lld", (long long)M);
  if (int rc = rnd_prop("ocppo_rnd_mask", update_proportion)) return rc;
  if (M == 0) return OCPPO_OK;
  OCPPO_REQUIRE(counter && out, "ocppo_rnd_mask: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(rnd_mask_kernel, dim3(grid_for(M, kRndThreads)), dim3(kRndThreads), 0,
                     as_stream(stream), seed, counter, M, update_proportion, out);
  return check_launch("ocppo_rnd_mask");
}
