// QDagger (cleanrl/qdagger_dqn_atari_impalacnn.py) on the DQN loop: the TD + distillation loss of
// :303-315 / :412-424 with its backward w.r.t. the student's Q values in one launch, and the
// script's deque(maxlen=10) of episodic returns with the distillation coefficient of :408-411 on
// the device (so the online chunk stays one hipGraph).
//
// The distillation term is the script's kl_divergence_with_logits: a SUM over the batch and the
// actions (it returns a scalar, so the torch.mean around it does nothing); it is kept as a sum.
#include "ocppo_common.h"
#include "ocppo_td.h"

namespace ocppo {

// One workgroup, one thread per row (as td_loss_kernel). The TD half is ocppo_td.h's td_row /
// td_reduce: with coeff = 0 dq, stats[1] and stats[3] are td_loss_kernel's bits.
// Row b, t = q_teacher / T, s = q / T:
//   p_t = softmax(t), p_s = softmax(s), ls_* = log_softmax (x - max - log(sum exp(x - max)))
//   distill_b = sum_a -p_t * (ls_s - ls_t)
//   d (c * distill) / d q[b, a] = ((p_s * sum_a' p_t - p_t) * c) / T, with the teacher's softmax
//   sum taken as (sum_a' e_t) / Z_t = 1: equal rows give exactly zero.
__global__ __launch_bounds__(1024) void qdagger_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ q_next,
    const float* __restrict__ q_teacher, const int64_t* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ dones, int64_t B, int A,
    float gamma, float norm, float temperature, const float* __restrict__ coeff_ptr,
    float* __restrict__ dq, float* __restrict__ stats) {
  __shared__ float scratch[16];
  const float c = coeff_ptr ? coeff_ptr[0] : 1.0f;
  float se = 0.f, sq = 0.f, sd = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
    int64_t a;
    const float g = td_row(q, q_next, actions, rewards, dones, b, A, gamma, norm, a, se, sq);
    const float* qs = q + b * A;
    const float* qt = q_teacher + b * A;
    float ms = qs[0] / temperature, mt = qt[0] / temperature;
    for (int j = 1; j < A; ++j) {
      ms = fmaxf(ms, qs[j] / temperature);
      mt = fmaxf(mt, qt[j] / temperature);
    }
    float zs = 0.f, zt = 0.f;
    for (int j = 0; j < A; ++j) {
      zs += expf(qs[j] / temperature - ms);
      zt += expf(qt[j] / temperature - mt);
    }
    const float lzs = logf(zs), lzt = logf(zt);
    float row = 0.f;
    for (int j = 0; j < A; ++j) {
      const float xs = qs[j] / temperature - ms, xt = qt[j] / temperature - mt;
      const float ps = expf(xs) / zs, pt = expf(xt) / zt;
      row += -pt * ((xs - lzs) - (xt - lzt));
      const float term = ((ps - pt) * c) / temperature;
      const float tdv = j == a ? g : 0.f;
      dq[b * A + j] = term == 0.f ? tdv : tdv + term;
    }
    sd += row;
  }
  float td_loss, q_mean;
  td_reduce(se, sq, B, scratch, td_loss, q_mean);
  sd = block_sum(sd, scratch);
  if (threadIdx.x == 0) {
    stats[0] = td_loss + c * sd;  // loss
    stats[1] = td_loss;           // q_loss
    stats[2] = sd;                // distill_loss
    stats[3] = q_mean;            // mean q(s, a)
    stats[4] = c;                 // the coefficient used
  }
}

constexpr int kRing = 10;  // deque(maxlen=10)

// One wave. Envs in chunks of 64: every lane updates its env's running return, then lane 0 pushes
// the chunk's finished returns into the ring in ascending env order.
__global__ __launch_bounds__(64) void qdagger_episode_push_kernel(
    const float* __restrict__ reward, const float* __restrict__ done, int64_t E,
    float* __restrict__ run_ret, float* __restrict__ ring, int64_t* __restrict__ state,
    double teacher_mean, float* __restrict__ coeff_out) {
  __shared__ float s_ret[kWave];
  __shared__ int s_done[kWave];
  int64_t head = state[0], count = state[1];  // only lane 0's copy is used
  if (head < 0 || head >= kRing) head = 0;    // never index outside the ring
  for (int64_t base = 0; base < E; base += kWave) {
    const int64_t e = base + threadIdx.x;
    int d = 0;
    float r = 0.f;
    if (e < E) {
      r = run_ret[e] + reward[e];
      d = done[e] != 0.f;
      run_ret[e] = d ? 0.f : r;
    }
    s_ret[threadIdx.x] = r;
    s_done[threadIdx.x] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 0; k < kWave; ++k)
        if (s_done[k]) {
          ring[head] = s_ret[k];
          head = head + 1 == kRing ? 0 : head + 1;
          count = count < kRing ? count + 1 : kRing;
        }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state[0] = head;
    state[1] = count;
    float coeff = 1.0f;
    if (count >= kRing) {
      double sum = 0.0;  // oldest (at head, the ring is full) to newest
      for (int k = 0; k < kRing; ++k) {
        const int64_t i = head + k;
        sum += static_cast<double>(ring[i >= kRing ? i - kRing : i]);
      }
      const double v = 1.0 - (sum / static_cast<double>(kRing)) / teacher_mean;
      coeff = static_cast<float>(v > 0.0 ? v : 0.0);
    }
    coeff_out[0] = coeff;
  }
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_qdagger_loss_fwd_bwd(ocppo_stream_t stream, const float* q,
                                          const float* q_next, const float* q_teacher,
                                          const int64_t* actions, const float* rewards,
                                          const float* dones, int64_t B, int64_t A, double gamma,
                                          double temperature, const float* distill_coeff,
                                          float* dq, float* stats) {
  OCPPO_REQUIRE(B >= 1 && A >= 1 && A <= 1024 && temperature > 0,
                "ocppo_qdagger_loss_fwd_bwd: bad sizes B=%lld A=%lld temperature=%g (B >= 1, "
                "1 <= A <= 1024, temperature > 0)", (long long)B, (long long)A, temperature);
  OCPPO_REQUIRE(q && q_next && q_teacher && actions && rewards && dones && dq && stats,
                "ocppo_qdagger_loss_fwd_bwd: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(qdagger_loss_kernel, dim3(1), dim3(256), 0, as_stream(stream), q, q_next,
                     q_teacher, actions, rewards, dones, B, (int)A, static_cast<float>(gamma),
                     td_norm(B), static_cast<float>(temperature), distill_coeff, dq, stats);
  return check_launch("ocppo_qdagger_loss_fwd_bwd");
}

extern "C" int ocppo_qdagger_episode_push(ocppo_stream_t stream, const float* reward,
                                          const float* done, int64_t E, float* run_ret,
                                          float* ring, int64_t* ring_state, double teacher_mean,
                                          float* coeff_out) {
  OCPPO_REQUIRE(E >= 1, "ocppo_qdagger_episode_push: bad sizes E=%lld", (long long)E);
  OCPPO_REQUIRE(teacher_mean != 0 && teacher_mean - teacher_mean == 0,
                "ocppo_qdagger_episode_push: teacher_mean must be finite and not 0");
  OCPPO_REQUIRE(reward && done && run_ret && ring && ring_state && coeff_out,
                "ocppo_qdagger_episode_push: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(qdagger_episode_push_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                     reward, done, E, run_ret, ring, ring_state, teacher_mean, coeff_out);
  return check_launch("ocppo_qdagger_episode_push");
}
