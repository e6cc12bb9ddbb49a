// Wave routines shared by the distributional learners (ocppo_c51.hip, ocppo_rainbow.hip): one wave
// owns one softmax over N <= 128 atoms, lane k holds atoms k and k + 64, and the max / sum /
// expected value are wave butterflies with a fixed order, so every result is bitwise repeatable.
#pragma once

#include <math.h>

#include "ocppo_common.h"

namespace ocppo {

constexpr int kC51MaxAtoms = 128;
constexpr int kC51MaxActions = 18;
constexpr int kC51LossWaves = 16;  // the loss kernels' single workgroup: 1024 threads
constexpr int kC51Batch = 6;       // softmaxes a wave reduces side by side (independent chains)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// softmax over the N atoms of G rows held in registers (x0 / x1: this lane's atoms `lane` and
// `lane + 64`, -inf past N) and each row's expected value q = sum_k p_k * z_k (torch.softmax(dim=2);
// (pmfs * atoms).sum(2)). Called by a whole wave; p0 / p1 are 0 past N, q is the same in every
// lane. The G chains are independent, so their butterflies overlap.
template <int G>
__device__ __forceinline__ void softmax_q_regs(float (&x0)[G], float (&x1)[G], bool h0, bool h1,
                                               float z0, float z1, float (&p0)[G], float (&p1)[G],
                                               float (&q)[G]) {
  float m[G], s[G];
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = wave_max(fmaxf(x0[g], x1[g]));
#pragma unroll
  for (int g = 0; g < G; ++g) {
    x0[g] = h0 ? expf(x0[g] - m[g]) : 0.f;
    x1[g] = h1 ? expf(x1[g] - m[g]) : 0.f;
    s[g] = x0[g] + x1[g];
  }
#pragma unroll
  for (int g = 0; g < G; ++g) s[g] = wave_sum(s[g]);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    p0[g] = x0[g] / s[g];
    p1[g] = x1[g] / s[g];
    q[g] = p0[g] * z0 + p1[g] * z1;
  }
#pragma unroll
  for (int g = 0; g < G; ++g) q[g] = wave_sum(q[g]);
}

// softmax_q_regs over up to G consecutive [N] rows starting at `rows` (`valid` of them exist; the
// others repeat the last one and are ignored by the caller).
template <int G>
__device__ __forceinline__ void c51_softmax_q(const float* __restrict__ rows, int valid, int N,
                                              int lane, float z0, float z1, float (&p0)[G],
                                              float (&p1)[G], float (&q)[G]) {
  const bool h0 = lane < N, h1 = lane + kWave < N;
  float x0[G], x1[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* row = rows + static_cast<int64_t>(g < valid ? g : valid - 1) * N;
    x0[g] = h0 ? row[lane] : -INFINITY;
    x1[g] = h1 ? row[lane + kWave] : -INFINITY;
  }
  softmax_q_regs<G>(x0, x1, h0, h1, z0, z1, p0, p1, q);
}

// torch.argmax's update rule on a running best (first maximum; a NaN beats every number)
__device__ __forceinline__ bool c51_better(float v, float best) {
  return v > best || (v != v && best == best);
}

// argmax_a of the expected value over A actions' softmaxes, kC51Batch of them side by side, and
// the pmf of that action at this lane's two atoms. `load(j0, valid, p0, p1, q)` fills the batch of
// actions j0 .. j0 + valid - 1 (c51_softmax_q / duel_softmax_q's outputs). `q_row`, when given, is
// the [A] row that receives every action's expected value.
struct Greedy {
  int best;
  float p0, p1;
};
template <typename Load>
__device__ __forceinline__ Greedy greedy_scan(int A, int lane, float* __restrict__ q_row,
                                              Load load) {
  Greedy r{0, 0.f, 0.f};
  float bq = 0.f;
  for (int j0 = 0; j0 < A; j0 += kC51Batch) {
    float p0[kC51Batch], p1[kC51Batch], q[kC51Batch];
    const int valid = A - j0 < kC51Batch ? A - j0 : kC51Batch;
    load(j0, valid, p0, p1, q);
#pragma unroll
    for (int g = 0; g < kC51Batch; ++g)
      if (g < valid) {
        if (j0 + g == 0 || c51_better(q[g], bq)) {
          bq = q[g];
          r.best = j0 + g;
          r.p0 = p0[g];
          r.p1 = p1[g];
        }
        if (q_row && lane == 0) q_row[j0 + g] = q[g];
      }
  }
  return r;
}

// a stored action outside [0, A) reads the nearest row instead of past the buffer
__device__ __forceinline__ int64_t clamp_action(int64_t a, int A) {
  return a < 0 ? 0 : (a >= A ? A - 1 : a);
}

// ---- the categorical projection of one loss workgroup (c51_atari_oc.py:339-352,
// rainbow_atari_oc.py:672-692) -------------------------------------------------------------------
//   next_atoms = r + (f32(gamma) * z) * (1 - d); tz = clamp(next_atoms, v_min, v_max);
//   b = (tz - v_min) / delta_z; l = floor(b), u = ceil(b), both clamped to [0, N - 1];
//   d_m_l = (u + eq - b) * p', d_m_u = (b - l) * p', where eq is (l == u) in C51's text and
//   (l == b) in Rainbow's (kEqIsLU); target[l] += d_m_l then target[u] += d_m_u, each in
//   ascending source-atom order (index_add_ on the CPU): every lane GATHERS its own target atoms
//   from the wave's LDS copy of (l, u, d_m_l, d_m_u), so the order is fixed and no float atomic is
//   needed.
// delta_z is the caller's: atoms[1] - atoms[0] in C51, the host's (v_max - v_min) / (N - 1) in
// Rainbow. Neither routine holds a barrier: the kernel puts one __syncthreads() between
// proj_terms and proj_gather and one after the sample (the wave's rows are rewritten by its next
// sample), both outside `if (active)`, where every wave reaches them with the same trip count.
// 16-B aligned: the gather reads four source atoms per LDS load (ds_read_b128)
struct alignas(16) ProjScratch {  // per wave, per source atom
  int l[kC51LossWaves][kC51MaxAtoms];
  int u[kC51LossWaves][kC51MaxAtoms];
  float dml[kC51LossWaves][kC51MaxAtoms];
  float dmu[kC51LossWaves][kC51MaxAtoms];
};

// the wave's per-source-atom terms from the next state's pmf p0 / p1; nd = 1 - done
template <bool kEqIsLU>
__device__ __forceinline__ void proj_terms(ProjScratch& s, int wv, int lane, int N, float z0,
                                           float z1, float p0, float p1, float r, float nd,
                                           float gamma, float v_min, float v_max, float delta_z) {
  const float n1 = static_cast<float>(N - 1);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + h * kWave;
    if (k < N) {
      const float z = h ? z1 : z0, p = h ? p1 : p0;
      const float na = r + (gamma * z) * nd;
      const float tz = fminf(fmaxf(na, v_min), v_max);
      const float bj = (tz - v_min) / delta_z;
      const float l = fminf(fmaxf(floorf(bj), 0.f), n1);
      const float u = fminf(fmaxf(ceilf(bj), 0.f), n1);
      s.l[wv][k] = static_cast<int>(l);
      s.u[wv][k] = static_cast<int>(u);
      s.dml[wv][k] = (u + (l == (kEqIsLU ? u : bj) ? 1.0f : 0.0f) - bj) * p;
      s.dmu[wv][k] = (bj - l) * p;
    }
  }
}

// this lane's two target atoms, gathered in ascending source-atom order (lower neighbours, then
// upper); `target_row`, when given, is the [N] row that receives them
__device__ __forceinline__ void proj_gather(const ProjScratch& s, int wv, int lane, int N,
                                            float* __restrict__ target_row, float& t0, float& t1) {
  t0 = 0.f;
  t1 = 0.f;
  for (int j = 0; j < N; ++j) {
    const int l = s.l[wv][j];
    const float v = s.dml[wv][j];
    if (l == lane) t0 += v;
    if (l == lane + kWave) t1 += v;
  }
  for (int j = 0; j < N; ++j) {
    const int u = s.u[wv][j];
    const float v = s.dmu[wv][j];
    if (u == lane) t0 += v;
    if (u == lane + kWave) t1 += v;
  }
  if (target_row) {
    if (lane < N) target_row[lane] = t0;
    if (lane + kWave < N) target_row[lane + kWave] = t1;
  }
}

// The clamped cross entropy of one row against the target atoms t0 / t1 and its backward through
// the softmax (c51_atari_oc.py:355-359, rainbow_atari_oc.py:695-701), p0 / p1 the online pmf:
//   c = clamp(p, 1e-5, 1 - 1e-5); loss_b = -sum_k target_k * log(c_k);
//   g_k = in range ? (scale * target_k) / c_k : 0, scale = -(1 / B) times the sample's weight;
//   d_k = (g_k - sum_j g_j p_j) * p_k = d loss / d logit_k
// Called by a whole wave; loss_b is the same in every lane.
struct CeBwd {
  float loss_b, d0, d1;
};
__device__ __forceinline__ CeBwd ce_softmax_bwd(float t0, float t1, float p0, float p1, bool h0,
                                                bool h1, float scale) {
  const float lo = 1e-5f, hi = static_cast<float>(1.0 - 1e-5);
  const float c0 = fminf(fmaxf(p0, lo), hi), c1 = fminf(fmaxf(p1, lo), hi);
  const float e0 = h0 ? t0 * logf(c0) : 0.f, e1 = h1 ? t1 * logf(c1) : 0.f;
  CeBwd r;
  r.loss_b = -wave_sum(e0 + e1);
  const float g0 = (h0 && p0 >= lo && p0 <= hi) ? (scale * t0) / c0 : 0.f;
  const float g1 = (h1 && p1 >= lo && p1 <= hi) ? (scale * t1) / c1 : 0.f;
  const float sg = wave_sum(g0 * p0 + g1 * p1);
  r.d0 = (g0 - sg) * p0;
  r.d1 = (g1 - sg) * p1;
  return r;
}

// stats = {sum_b loss / B, sum_b q / B}: each wave's partial (ascending sample order) through
// LDS, then the waves in order by thread 0, which rewrites both (graph-replay safe). TQ is the
// type the q sum runs in. Holds a barrier: every thread of the workgroup calls it.
template <typename TQ>
__device__ __forceinline__ void loss_stats(float acc_loss, TQ acc_q,
                                           float (&s_loss)[kC51LossWaves],
                                           TQ (&s_q)[kC51LossWaves], int lane, int wv, int64_t B,
                                           float* __restrict__ stats) {
  if (lane == 0) {
    s_loss[wv] = acc_loss;
    s_q[wv] = acc_q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sl = s_loss[0];
    TQ sq = s_q[0];
    for (int w = 1; w < kC51LossWaves; ++w) {
      sl += s_loss[w];
      sq += s_q[w];
    }
    stats[0] = sl / static_cast<float>(B);                   // losses/loss, losses/td_loss
    stats[1] = static_cast<float>(sq / static_cast<TQ>(B));  // losses/q_values
  }
}

}  // namespace ocppo
