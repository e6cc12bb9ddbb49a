// Rainbow path of cleanrl/rainbow_atari_oc.py: the train step's loss block (:655-701) with its
// backward as one launch, and the acting step's greedy choice (:617-620).
//
// The network (NoisyDuelingDistributionalNetwork / ...PPObj.forward) ends in
//   q_atoms = value + advantage - advantage.mean(dim=1, keepdim=True); q_dist = softmax(q_atoms, 2)
// so both kernels read the RAW head outputs value [rows, N] and advantage [rows, A * N] and form
// the dueling combine and the softmax themselves. One wave owns one (sample, action) softmax as in
// ocppo_c51.hip (ocppo_distributional.h): lane k holds atoms k and k + 64 (N <= 128), reductions
// are wave butterflies with a fixed order, so every result is bitwise repeatable. The file is
// compiled with -ffp-contract=off like the rest of the library: next_atoms and the projected
// index b keep the reference's per-op f32 rounding, which floor / ceil depend on.
#include <math.h>

#include "ocppo_common.h"
#include "ocppo_distributional.h"

namespace ocppo {

// advantage.mean(dim=1) at this lane's two atoms: the A rows summed in ascending order, / A
__device__ __forceinline__ void duel_mean(const float* __restrict__ adv, int A, int N, int lane,
                                          bool h0, bool h1, float& m0, float& m1) {
  float s0 = 0.f, s1 = 0.f;
  for (int j = 0; j < A; ++j) {
    if (h0) s0 += adv[j * N + lane];
    if (h1) s1 += adv[j * N + lane + kWave];
  }
  m0 = s0 / static_cast<float>(A);
  m1 = s1 / static_cast<float>(A);
}

// softmax and expected value of the dueling rows j0 .. j0 + valid - 1 (the others repeat the last)
template <int G>
__device__ __forceinline__ void duel_softmax_q(const float* __restrict__ adv, float v0, float v1,
                                               float m0, float m1, int j0, int valid, int N,
                                               int lane, bool h0, bool h1, float z0, float z1,
                                               float (&p0)[G], float (&p1)[G], float (&q)[G]) {
  float x0[G], x1[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* row = adv + static_cast<int64_t>(j0 + (g < valid ? g : valid - 1)) * N;
    x0[g] = h0 ? (v0 + row[lane]) - m0 : -INFINITY;
    x1[g] = h1 ? (v1 + row[lane + kWave]) - m1 : -INFINITY;
  }
  softmax_q_regs<G>(x0, x1, h0, h1, z0, z1, p0, p1, q);
}

// argmax_a of the expected value of (value, advantage) row `r` (first maximum)
__device__ __forceinline__ int duel_greedy(const float* __restrict__ value,
                                           const float* __restrict__ advantage, int64_t r, int A,
                                           int N, int lane, bool h0, bool h1, float z0, float z1,
                                           float* __restrict__ q_out) {
  const float* adv = advantage + r * A * N;
  const float v0 = h0 ? value[r * N + lane] : 0.f, v1 = h1 ? value[r * N + lane + kWave] : 0.f;
  float m0, m1;
  duel_mean(adv, A, N, lane, h0, h1, m0, m1);
  return greedy_scan(A, lane, q_out ? q_out + r * A : nullptr,
                     [&](int j0, int valid, auto& p0, auto& p1, auto& q) {
    duel_softmax_q<kC51Batch>(adv, v0, v1, m0, m1, j0, valid, N, lane, h0, h1, z0, z1, p0, p1, q);
  }).best;
}

// Fused Rainbow train-step loss (rainbow_atari_oc.py:655-701), forward and d loss / d (value,
// advantage) of the online forward on `obs`, as ONE workgroup: wave w takes samples w, w + 16, ...
//   double Q (:657-669): best = argmax_a sum_k softmax(duel(value_no, adv_no)[b, a])_k z_k of the
//     ONLINE net on next_obs (first maximum); p' = softmax(duel(value_nt, adv_nt)[b, best]) of
//     the TARGET net on next_obs
//   projection (:672-692, not C51's text): gamma ** n_step, the HOST's delta_z =
//     (v_max - v_min) / (N - 1) rounded to f32, and the (l == b) rule (ocppo_distributional.h:
//     proj_terms / proj_gather)
//   online side (:695-701): p = softmax(duel(value, adv)[b, a_b]); loss_b, the clamped cross
//     entropy (an output: the new priorities), and its backward with scale -((1 / B) * w_b)
//     (ce_softmax_bwd); loss = mean_b loss_b * w_b; dvalue[b, k] = d_k;
//     dadvantage[b, a, k] = (a == a_b ? d_k : 0) + (-d_k / A): every element is written
//   stats = {loss, mean_b sum_k p_k z_k} (:708-713, loss_stats); the second one's sums run in f64
__global__ __launch_bounds__(kC51LossWaves* kWave) void rainbow_loss_kernel(
    const float* __restrict__ value, const float* __restrict__ adv,
    const float* __restrict__ value_no, const float* __restrict__ adv_no,
    const float* __restrict__ value_nt, const float* __restrict__ adv_nt,
    const float* __restrict__ support, const int64_t* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ dones,
    const float* __restrict__ weights, int64_t B, int A, int N, float gamma_n, float v_min,
    float v_max, float delta_z, float inv_b, float* __restrict__ dvalue, float* __restrict__ dadv,
    float* __restrict__ loss_per_sample, float* __restrict__ stats,
    float* __restrict__ target_out, int64_t* __restrict__ best_out) {
  __shared__ ProjScratch s_proj;
  __shared__ float s_loss[kC51LossWaves];
  __shared__ double s_q[kC51LossWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool h0 = lane < N, h1 = lane + kWave < N;
  const float z0 = h0 ? support[lane] : 0.f, z1 = h1 ? support[lane + kWave] : 0.f;
  const float fa = static_cast<float>(A);
  float acc_loss = 0.f;
  double acc_q = 0.0;
  for (int64_t b0 = 0; b0 < B; b0 += kC51LossWaves) {  // same trip count in every wave
    const int64_t b = b0 + wv;
    const bool active = b < B;  // wave-uniform
    if (active) {
      const int best = duel_greedy(value_no, adv_no, b, A, N, lane, h0, h1, z0, z1, nullptr);
      if (best_out && lane == 0) best_out[b] = best;
      // the target net's pmf at that action
      const float* at = adv_nt + b * A * N;
      const float v0 = h0 ? value_nt[b * N + lane] : 0.f;
      const float v1 = h1 ? value_nt[b * N + lane + kWave] : 0.f;
      float m0, m1, tp0[1], tp1[1], tq[1];
      duel_mean(at, A, N, lane, h0, h1, m0, m1);
      duel_softmax_q<1>(at, v0, v1, m0, m1, best, 1, N, lane, h0, h1, z0, z1, tp0, tp1, tq);
      proj_terms<false>(s_proj, wv, lane, N, z0, z1, tp0[0], tp1[0], rewards[b], 1.0f - dones[b],
                        gamma_n, v_min, v_max, delta_z);
    }
    __syncthreads();
    if (active) {
      float t0, t1;
      proj_gather(s_proj, wv, lane, N, target_out ? target_out + b * N : nullptr, t0, t1);
      // online side: the taken action's pmf
      const int64_t a = clamp_action(actions[b], A);
      const float* ao = adv + b * A * N;
      const float v0 = h0 ? value[b * N + lane] : 0.f;
      const float v1 = h1 ? value[b * N + lane + kWave] : 0.f;
      float m0, m1, p0[1], p1[1], q[1];
      duel_mean(ao, A, N, lane, h0, h1, m0, m1);
      duel_softmax_q<1>(ao, v0, v1, m0, m1, static_cast<int>(a), 1, N, lane, h0, h1, z0, z1, p0,
                        p1, q);
      const float w = weights[b];
      const CeBwd ce = ce_softmax_bwd(t0, t1, p0[0], p1[0], h0, h1, -(inv_b * w));
      if (lane == 0) loss_per_sample[b] = ce.loss_b;
      acc_loss += ce.loss_b * w;
      // the logged q_values is a small difference of large terms (the support is symmetric):
      // its sums run in f64 over the f32 pmf, so only the pmf's own rounding is left in it
      acc_q += wave_sum(static_cast<double>(p0[0]) * z0 + static_cast<double>(p1[0]) * z1);
      const float sh0 = -(ce.d0 / fa), sh1 = -(ce.d1 / fa);  // the mean's share, every action row
      if (h0) dvalue[b * N + lane] = ce.d0;
      if (h1) dvalue[b * N + lane + kWave] = ce.d1;
      for (int j = 0; j < A; ++j) {
        float* out = dadv + (b * A + j) * N;
        if (h0) out[lane] = j == a ? ce.d0 + sh0 : sh0;
        if (h1) out[lane + kWave] = j == a ? ce.d1 + sh1 : sh1;
      }
    }
    __syncthreads();  // the wave's LDS rows are rewritten by its next sample
  }
  loss_stats(acc_loss, acc_q, s_loss, s_q, lane, wv, B, stats);
}

// The acting step (:617-620): q_dist = q_network(obs); argmax_a sum_k q_dist * support. One wave
// per env; no epsilon (the noisy heads explore).
__global__ __launch_bounds__(256) void rainbow_greedy_kernel(
    const float* __restrict__ value, const float* __restrict__ adv,
    const float* __restrict__ support, int64_t E, int A, int N, int64_t* __restrict__ actions,
    float* __restrict__ q_out) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  if (e >= E) return;  // wave-uniform
  const bool h0 = lane < N, h1 = lane + kWave < N;
  const float z0 = h0 ? support[lane] : 0.f, z1 = h1 ? support[lane + kWave] : 0.f;
  const int best = duel_greedy(value, adv, e, A, N, lane, h0, h1, z0, z1, q_out);
  if (lane == 0) actions[e] = best;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_rainbow_loss_fwd_bwd(
    ocppo_stream_t stream, const float* value, const float* advantage, const float* value_next_online,
    const float* advantage_next_online, const float* value_next_target,
    const float* advantage_next_target, const float* support, const int64_t* actions,
    const float* rewards, const float* dones, const float* weights, int64_t B, int64_t A,
    int64_t N, double gamma_n, double v_min, double v_max, float* dvalue, float* dadvantage,
    float* loss_per_sample, float* stats, float* target_pmfs, int64_t* best_actions) {
  OCPPO_REQUIRE(B >= 1 && B <= INT32_MAX && A >= 1 && A <= kC51MaxActions && N >= 2 &&
                    N <= kC51MaxAtoms,
                "ocppo_rainbow_loss_fwd_bwd: bad sizes B=%lld A=%lld N=%lld (B >= 1, 1 <= A <= %d, "
                "2 <= N <= %d)", (long long)B, (long long)A, (long long)N, kC51MaxActions,
                kC51MaxAtoms);
  OCPPO_REQUIRE(value && advantage && value_next_online && advantage_next_online &&
                    value_next_target && advantage_next_target && support && actions && rewards &&
                    dones && weights && dvalue && dadvantage && loss_per_sample && stats,
                "ocppo_rainbow_loss_fwd_bwd: null pointer");
  clear_stale_error();
  // mean's backward: grad / numel, formed in f32; delta_z as the modules' __init__ forms it
  const float inv_b = 1.0f / static_cast<float>(B);
  const double delta_z = (v_max - v_min) / static_cast<double>(N - 1);
  hipLaunchKernelGGL(rainbow_loss_kernel, dim3(1), dim3(kC51LossWaves * kWave), 0,
                     as_stream(stream), value, advantage, value_next_online, advantage_next_online,
                     value_next_target, advantage_next_target, support, actions, rewards, dones,
                     weights, B, (int)A, (int)N, static_cast<float>(gamma_n),
                     static_cast<float>(v_min), static_cast<float>(v_max),
                     static_cast<float>(delta_z), inv_b, dvalue, dadvantage, loss_per_sample, stats,
                     target_pmfs, best_actions);
  return check_launch("ocppo_rainbow_loss_fwd_bwd");
}

extern "C" int ocppo_rainbow_greedy(ocppo_stream_t stream, const float* value,
                                    const float* advantage, const float* support, int64_t E,
                                    int64_t A, int64_t N, int64_t* actions, float* q_out) {
  OCPPO_REQUIRE(E >= 1 && E <= INT32_MAX && A >= 1 && A <= kC51MaxActions && N >= 2 &&
                    N <= kC51MaxAtoms,
                "ocppo_rainbow_greedy: bad sizes E=%lld A=%lld N=%lld (E >= 1, 1 <= A <= %d, "
                "2 <= N <= %d)", (long long)E, (long long)A, (long long)N, kC51MaxActions,
                kC51MaxAtoms);
  OCPPO_REQUIRE(value && advantage && support && actions, "ocppo_rainbow_greedy: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(rainbow_greedy_kernel, dim3(static_cast<unsigned>(ceil_div(E, 4))), dim3(256),
                     0, as_stream(stream), value, advantage, support, E, (int)A, (int)N, actions,
                     q_out);
  return check_launch("ocppo_rainbow_greedy");
}
