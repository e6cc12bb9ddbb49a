// C51 (categorical DQN) path of cleanrl/c51_atari_oc.py: the fused categorical projection + cross
// entropy loss, forward and backward (:339-359), and the acting step's expected-value
// epsilon-greedy choice (:303-308 with QNetwork_C51.get_action, architectures/dqn.py:57-64).
//
// Both kernels read the network's [rows, A * N] logits (N atoms per action) and the registered
// `atoms` buffer [N]. One wave owns one (sample, action) softmax: lane k holds atoms k and k + 64
// (N <= 128), the max / sum / expected value are wave butterflies with a fixed order, so every
// result is bitwise repeatable. The file is compiled with -ffp-contract=off like the rest of the
// library: next_atoms = r + (gamma * z) * (1 - d) keeps the reference's per-op f32 rounding, which
// floor / ceil of the projected index b depend on.
#include <math.h>

#include "ocppo_common.h"
#include "ocppo_distributional.h"
#include "ocppo_rng.h"

namespace ocppo {

// Fused C51 train-step loss (c51_atari_oc.py:339-359), forward and d loss / d logits, as ONE
// workgroup (B is the minibatch, 32 in the reference): wave w takes samples w, w + 16, ...
//   target side: argmax_a sum_k softmax(logits_next[b, a])_k z_k (first maximum), its pmf p',
//     projected onto the support with delta_z = z[1] - z[0] and the (l == u) rule
//     (ocppo_distributional.h: proj_terms / proj_gather)
//   online side: p = softmax(logits[b, a_b]); the clamped cross entropy against the target and
//     its backward with scale -(1 / B) (ce_softmax_bwd);
//     dlogits[b, a_b, k] = d_k, zeros for the other actions
//   stats = {mean_b loss_b, mean_b sum_k p_k z_k} (loss_stats, both sums in f32)
__global__ __launch_bounds__(kC51LossWaves* kWave) void c51_loss_kernel(
    const float* __restrict__ logits, const float* __restrict__ logits_next,
    const float* __restrict__ atoms, const int64_t* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ dones, int64_t B, int A, int N,
    float gamma, float v_min, float v_max, float inv_b, float* __restrict__ dlogits,
    float* __restrict__ stats, float* __restrict__ target_out, int64_t* __restrict__ next_action) {
  __shared__ ProjScratch s_proj;
  __shared__ float s_loss[kC51LossWaves], s_q[kC51LossWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool h0 = lane < N, h1 = lane + kWave < N;
  const float z0 = h0 ? atoms[lane] : 0.f, z1 = h1 ? atoms[lane + kWave] : 0.f;
  const float delta_z = atoms[1] - atoms[0];
  float acc_loss = 0.f, acc_q = 0.f;
  for (int64_t b0 = 0; b0 < B; b0 += kC51LossWaves) {  // same trip count in every wave
    const int64_t b = b0 + wv;
    const bool active = b < B;  // wave-uniform
    if (active) {
      // greedy next action of the target net and its pmf
      const float* next = logits_next + b * A * N;
      const Greedy gr = greedy_scan(A, lane, nullptr, [&](int j0, int valid, auto& p0, auto& p1,
                                                          auto& q) {
        c51_softmax_q<kC51Batch>(next + static_cast<int64_t>(j0) * N, valid, N, lane, z0, z1, p0,
                                 p1, q);
      });
      if (next_action && lane == 0) next_action[b] = gr.best;
      proj_terms<true>(s_proj, wv, lane, N, z0, z1, gr.p0, gr.p1, rewards[b], 1.0f - dones[b],
                       gamma, v_min, v_max, delta_z);
    }
    __syncthreads();
    if (active) {
      float t0, t1;
      proj_gather(s_proj, wv, lane, N, target_out ? target_out + b * N : nullptr, t0, t1);
      // online side: the taken action's pmf
      const int64_t a = clamp_action(actions[b], A);
      float p0[1], p1[1], q[1];
      c51_softmax_q<1>(logits + (b * A + a) * N, 1, N, lane, z0, z1, p0, p1, q);
      const CeBwd ce = ce_softmax_bwd(t0, t1, p0[0], p1[0], h0, h1, -inv_b);
      acc_loss += ce.loss_b;
      acc_q += q[0];
      for (int j = 0; j < A; ++j) {
        float* out = dlogits + (b * A + j) * N;
        if (h0) out[lane] = j == a ? ce.d0 : 0.f;
        if (h1) out[lane + kWave] = j == a ? ce.d1 : 0.f;
      }
    }
    __syncthreads();  // the wave's LDS rows are rewritten by its next sample
  }
  loss_stats(acc_loss, acc_q, s_loss, s_q, lane, wv, B, stats);
}

// Expected Q per action + epsilon_greedy_kernel's choice on it (the same EpsGreedy, the same
// first-maximum rule), one wave per env.
__global__ __launch_bounds__(256) void c51_epsilon_greedy_kernel(
    const float* __restrict__ logits, const float* __restrict__ atoms, int64_t E, int A, int N,
    uint64_t seed, const int64_t* __restrict__ step, int64_t step_offset, double start_e,
    double end_e, double duration, int64_t* __restrict__ actions, float* __restrict__ eps_out,
    float* __restrict__ q_out) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  if (e >= E) return;  // wave-uniform
  const float z0 = lane < N ? atoms[lane] : 0.f, z1 = lane + kWave < N ? atoms[lane + kWave] : 0.f;
  const EpsGreedy eg(seed, step[0] + step_offset, start_e, end_e, duration);
  const float* rows = logits + e * A * N;
  const Greedy gr = greedy_scan(A, lane, q_out ? q_out + e * A : nullptr,
                                [&](int j0, int valid, auto& p0, auto& p1, auto& q) {
    c51_softmax_q<kC51Batch>(rows + static_cast<int64_t>(j0) * N, valid, N, lane, z0, z1, p0, p1,
                             q);
  });
  const int64_t a = eg.explore ? eg.random_action(e, A) : gr.best;
  if (lane == 0) actions[e] = a;
  if (eps_out && e == 0 && lane == 0) eps_out[0] = static_cast<float>(eg.eps);
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_c51_loss_fwd_bwd(ocppo_stream_t stream, const float* logits,
                                      const float* logits_next, const float* atoms,
                                      const int64_t* actions, const float* rewards,
                                      const float* dones, int64_t B, int64_t A, int64_t N,
                                      double gamma, double v_min, double v_max, float* dlogits,
                                      float* stats, float* target_pmfs, int64_t* next_action) {
  OCPPO_REQUIRE(B >= 1 && B <= INT32_MAX && A >= 1 && A <= kC51MaxActions && N >= 2 &&
                    N <= kC51MaxAtoms,
                "ocppo_c51_loss_fwd_bwd: bad sizes B=%lld A=%lld N=%lld (B >= 1, 1 <= A <= %d, "
                "2 <= N <= %d)", (long long)B, (long long)A, (long long)N, kC51MaxActions,
                kC51MaxAtoms);
  OCPPO_REQUIRE(logits && logits_next && atoms && actions && rewards && dones && dlogits && stats,
                "ocppo_c51_loss_fwd_bwd: null pointer");
  clear_stale_error();
  // mean's backward: grad / numel, formed in f32
  const float inv_b = 1.0f / static_cast<float>(B);
  hipLaunchKernelGGL(c51_loss_kernel, dim3(1), dim3(kC51LossWaves * kWave), 0, as_stream(stream),
                     logits, logits_next, atoms, actions, rewards, dones, B, (int)A, (int)N,
                     static_cast<float>(gamma), static_cast<float>(v_min),
                     static_cast<float>(v_max), inv_b, dlogits, stats, target_pmfs, next_action);
  return check_launch("ocppo_c51_loss_fwd_bwd");
}

extern "C" int ocppo_c51_epsilon_greedy(ocppo_stream_t stream, const float* logits,
                                        const float* atoms, int64_t E, int64_t A, int64_t N,
                                        uint64_t seed, const int64_t* step, int64_t step_offset,
                                        double start_e, double end_e, double duration,
                                        int64_t* actions, float* epsilon_out, float* q_out) {
  OCPPO_REQUIRE(E >= 1 && E <= INT32_MAX && A >= 1 && A <= kC51MaxActions && N >= 2 &&
                    N <= kC51MaxAtoms && duration > 0,
                "ocppo_c51_epsilon_greedy: bad sizes E=%lld A=%lld N=%lld (E >= 1, 1 <= A <= %d, "
                "2 <= N <= %d, duration > 0)", (long long)E, (long long)A, (long long)N,
                kC51MaxActions, kC51MaxAtoms);
  OCPPO_REQUIRE(logits && atoms && step && actions, "ocppo_c51_epsilon_greedy: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(c51_epsilon_greedy_kernel, dim3(static_cast<unsigned>(ceil_div(E, 4))),
                     dim3(256), 0, as_stream(stream), logits, atoms, E, (int)A, (int)N, seed, step,
                     step_offset, start_e, end_e, duration, actions, epsilon_out, q_out);
  return check_launch("ocppo_c51_epsilon_greedy");
}
