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

namespace ocppo {

// the splitmix64 finaliser of ocppo_dqn.hip (epsilon_greedy_kernel's coin and random action)
__device__ __forceinline__ uint64_t c51_mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Fused C51 train-step loss (c51_atari_oc.py:339-359), forward and d loss / d logits, as ONE
// workgroup (B is the minibatch, 32 in the reference): wave w takes samples w, w + 16, ...
//   target side: argmax_a sum_k softmax(logits_next[b, a])_k z_k (first maximum), its pmf p';
//     next_atoms = r + (f32(gamma) * z) * (1 - d); tz = clamp(next_atoms, v_min, v_max);
//     b = (tz - v_min) / (z[1] - z[0]); l = floor(b), u = ceil(b), both clamped to [0, N - 1];
//     d_m_l = (u + (l == u) - b) * p', d_m_u = (b - l) * p'; target[l] += d_m_l then
//     target[u] += d_m_u, each in ascending source-atom order (index_add_ on the CPU): every
//     lane GATHERS its own target atoms from the wave's LDS copy of (l, u, d_m_l, d_m_u), so
//     the order is fixed and no float atomic is needed
//   online side: p = softmax(logits[b, a_b]); c = clamp(p, 1e-5, 1 - 1e-5);
//     loss_b = -sum_k target_k * log(c_k); g_k = in range ? (-(1 / B) * target_k) / c_k : 0;
//     dlogits[b, a_b, k] = (g_k - sum_j g_j p_j) * p_k, zeros for the other actions
//   stats = {mean_b loss_b, mean_b sum_k p_k z_k}: per wave in ascending sample order, then the
//     waves in order by thread 0, which rewrites both (graph-replay safe)
__global__ __launch_bounds__(kC51LossWaves* kWave) void c51_loss_kernel(
    const float* __restrict__ logits, const float* __restrict__ logits_next,
    const float* __restrict__ atoms, const int64_t* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ dones, int64_t B, int A, int N,
    float gamma, float v_min, float v_max, float inv_b, float* __restrict__ dlogits,
    float* __restrict__ stats, float* __restrict__ target_out, int64_t* __restrict__ next_action) {
  __shared__ int s_l[kC51LossWaves][kC51MaxAtoms];
  __shared__ int s_u[kC51LossWaves][kC51MaxAtoms];
  __shared__ float s_dml[kC51LossWaves][kC51MaxAtoms];
  __shared__ float s_dmu[kC51LossWaves][kC51MaxAtoms];
  __shared__ float s_part[2][kC51LossWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool h0 = lane < N, h1 = lane + kWave < N;
  const float z0 = h0 ? atoms[lane] : 0.f, z1 = h1 ? atoms[lane + kWave] : 0.f;
  const float delta_z = atoms[1] - atoms[0];
  const float n1 = static_cast<float>(N - 1);
  const float lo = 1e-5f, hi = static_cast<float>(1.0 - 1e-5);
  float acc_loss = 0.f, acc_q = 0.f;
  for (int64_t b0 = 0; b0 < B; b0 += kC51LossWaves) {  // same trip count in every wave
    const int64_t b = b0 + wv;
    const bool active = b < B;  // wave-uniform
    float t_p0 = 0.f, t_p1 = 0.f;
    if (active) {
      // greedy next action of the target net and its pmf
      int best = 0;
      float bq = 0.f;
      for (int j0 = 0; j0 < A; j0 += kC51Batch) {
        float p0[kC51Batch], p1[kC51Batch], q[kC51Batch];
        const int valid = A - j0 < kC51Batch ? A - j0 : kC51Batch;
        c51_softmax_q<kC51Batch>(logits_next + (b * A + j0) * N, valid, N, lane, z0, z1, p0, p1,
                                 q);
#pragma unroll
        for (int g = 0; g < kC51Batch; ++g)
          if (g < valid && (j0 + g == 0 || c51_better(q[g], bq))) {
            bq = q[g];
            best = j0 + g;
            t_p0 = p0[g];
            t_p1 = p1[g];
          }
      }
      if (next_action && lane == 0) next_action[b] = best;
      // the projection's per-source-atom terms
      const float r = rewards[b], nd = 1.0f - dones[b];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + h * kWave;
        if (k < N) {
          const float z = h ? z1 : z0, p = h ? t_p1 : t_p0;
          const float na = r + (gamma * z) * nd;
          const float tz = fminf(fmaxf(na, v_min), v_max);
          const float bj = (tz - v_min) / delta_z;
          const float l = fminf(fmaxf(floorf(bj), 0.f), n1);
          const float u = fminf(fmaxf(ceilf(bj), 0.f), n1);
          s_l[wv][k] = static_cast<int>(l);
          s_u[wv][k] = static_cast<int>(u);
          s_dml[wv][k] = (u + (l == u ? 1.0f : 0.0f) - bj) * p;
          s_dmu[wv][k] = (bj - l) * p;
        }
      }
    }
    __syncthreads();
    if (active) {
      float t0 = 0.f, t1 = 0.f;
      for (int j = 0; j < N; ++j) {
        const int l = s_l[wv][j];
        const float v = s_dml[wv][j];
        if (l == lane) t0 += v;
        if (l == lane + kWave) t1 += v;
      }
      for (int j = 0; j < N; ++j) {
        const int u = s_u[wv][j];
        const float v = s_dmu[wv][j];
        if (u == lane) t0 += v;
        if (u == lane + kWave) t1 += v;
      }
      if (target_out) {
        if (h0) target_out[b * N + lane] = t0;
        if (h1) target_out[b * N + lane + kWave] = t1;
      }
      // online side: the taken action's pmf (an action outside [0, A) reads the nearest row
      // instead of past the buffer)
      int64_t a = actions[b];
      a = a < 0 ? 0 : (a >= A ? A - 1 : a);
      float p0[1], p1[1], q[1];
      c51_softmax_q<1>(logits + (b * A + a) * N, 1, N, lane, z0, z1, p0, p1, q);
      const float c0 = fminf(fmaxf(p0[0], lo), hi), c1 = fminf(fmaxf(p1[0], lo), hi);
      const float e0 = h0 ? t0 * logf(c0) : 0.f, e1 = h1 ? t1 * logf(c1) : 0.f;
      acc_loss += -wave_sum(e0 + e1);
      acc_q += q[0];
      const float g0 = (h0 && p0[0] >= lo && p0[0] <= hi) ? ((-inv_b) * t0) / c0 : 0.f;
      const float g1 = (h1 && p1[0] >= lo && p1[0] <= hi) ? ((-inv_b) * t1) / c1 : 0.f;
      const float sg = wave_sum(g0 * p0[0] + g1 * p1[0]);
      const float d0 = (g0 - sg) * p0[0], d1 = (g1 - sg) * p1[0];
      for (int j = 0; j < A; ++j) {
        float* out = dlogits + (b * A + j) * N;
        if (h0) out[lane] = j == a ? d0 : 0.f;
        if (h1) out[lane + kWave] = j == a ? d1 : 0.f;
      }
    }
    __syncthreads();  // the wave's LDS rows are rewritten by its next sample
  }
  if (lane == 0) {
    s_part[0][wv] = acc_loss;
    s_part[1][wv] = acc_q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sl = s_part[0][0], sq = s_part[1][0];
    for (int w = 1; w < kC51LossWaves; ++w) {
      sl += s_part[0][w];
      sq += s_part[1][w];
    }
    stats[0] = sl / static_cast<float>(B);  // losses/loss
    stats[1] = sq / static_cast<float>(B);  // losses/q_values
  }
}

// Expected Q per action + epsilon_greedy_kernel's choice on it (same coin, same random action,
// same first-maximum rule), one wave per env.
__global__ __launch_bounds__(256) void c51_epsilon_greedy_kernel(
    const float* __restrict__ logits, const float* __restrict__ atoms, int64_t E, int A, int N,
    uint64_t seed, const int64_t* __restrict__ step, int64_t step_offset, double start_e,
    double end_e, double duration, int64_t* __restrict__ actions, float* __restrict__ eps_out,
    float* __restrict__ q_out) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  if (e >= E) return;  // wave-uniform
  const float z0 = lane < N ? atoms[lane] : 0.f, z1 = lane + kWave < N ? atoms[lane + kWave] : 0.f;
  const int64_t t = step[0] + step_offset;
  const double slope = (end_e - start_e) / duration;
  double eps = slope * static_cast<double>(t) + start_e;
  eps = eps > end_e ? eps : end_e;
  const uint64_t h = c51_mix64(c51_mix64(seed ^ 0xA0761D6478BD642Full) + static_cast<uint64_t>(t));
  const double coin = static_cast<double>(h >> 11) * (1.0 / 9007199254740992.0);  // [0, 1)
  int best = 0;
  float bq = 0.f;
  for (int j0 = 0; j0 < A; j0 += kC51Batch) {
    float p0[kC51Batch], p1[kC51Batch], q[kC51Batch];
    const int valid = A - j0 < kC51Batch ? A - j0 : kC51Batch;
    c51_softmax_q<kC51Batch>(logits + (e * A + j0) * N, valid, N, lane, z0, z1, p0, p1, q);
#pragma unroll
    for (int g = 0; g < kC51Batch; ++g)
      if (g < valid) {
        if (j0 + g == 0 || c51_better(q[g], bq)) {
          bq = q[g];
          best = j0 + g;
        }
        if (q_out && lane == 0) q_out[e * A + j0 + g] = q[g];
      }
  }
  int64_t a = best;
  if (coin < eps)
    a = static_cast<int64_t>(c51_mix64(h + static_cast<uint64_t>(e) + 1) % static_cast<uint64_t>(A));
  if (lane == 0) actions[e] = a;
  if (eps_out && e == 0 && lane == 0) eps_out[0] = static_cast<float>(eps);
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
