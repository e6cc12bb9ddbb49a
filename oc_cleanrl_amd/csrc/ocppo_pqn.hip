// PQN (cleanrl/pqn_atari_envpool.py) on the device rollout: the Q(lambda) reverse scan (:248-261),
// LayerNorm + ReLU after a Linear layer with its backward (the `Linear -> LayerNorm -> ReLU` of
// QNetwork, :117-135), the Q head with the greedy value and the epsilon-greedy action written into
// the rollout rows (:224-232), and the MSE loss on the taken action's Q value (:276-277). All f32,
// wave64, no atomics: every sum runs in an order fixed by the shapes alone.
#include "ocppo_common.h"
#include "ocppo_layernorm.h"
#include "ocppo_pqn_act.h"
#include "ocppo_rng.h"

namespace ocppo {

// LayerNorm + ReLU: ocppo_layernorm.h's kernels with the two-step centring, E <= 1024
constexpr int kLnrMaxE = 1024;

// ---- Q(lambda) -----------------------------------------------------------------------------------
// One thread per environment walks t = T-1 .. 0 (consecutive lanes = consecutive envs of a time
// row). The script's ops one by one, f32 without contraction:
//   t = T-1: ret = r + (g * max_a next_q) * (1 - next_done)
//   t < T-1: ret = r + (g * (lam * ret' + oml * v')) * (1 - d')     (v', d' = row t + 1)
__global__ __launch_bounds__(256) void q_lambda_kernel(
    const float* __restrict__ rew, const float* __restrict__ val, const float* __restrict__ don,
    const float* __restrict__ next_q, const float* __restrict__ next_done, int T, int64_t N, int A,
    float g, float lam, float oml, float* __restrict__ ret) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float m = next_q[n * A];  // torch.max: the maximum, a NaN if there is one
  for (int j = 1; j < A; ++j) {
    const float v = next_q[n * A + j];
    if (v > m || v != v) m = v;
  }
  size_t gi = static_cast<size_t>(T - 1) * N + n;
  float last = rew[gi] + (g * m) * (1.0f - next_done[n]);
  ret[gi] = last;
  for (int t = T - 2; t >= 0; --t) {
    const float nnt = 1.0f - don[gi];
    const float nv = val[gi];
    gi -= N;
    const float mix = lam * last + oml * nv;
    last = rew[gi] + (g * mix) * nnt;
    ret[gi] = last;
  }
}

// ---- Q head + greedy value + epsilon-greedy action ----------------------------------------------
// One wave per environment runs ocppo_pqn_act.h's pqn_act_row (shared with ocppo_pqn_lstm_act).
__global__ __launch_bounds__(256) void pqn_act_kernel(
    const float* __restrict__ hidden, int64_t N, int H, const float* __restrict__ wq,
    const float* __restrict__ bq, int A, uint64_t seed, const int64_t* __restrict__ step,
    int64_t step_offset, double start_e, double end_e, double duration,
    int64_t* __restrict__ actions, float* __restrict__ values, float* __restrict__ eps_out,
    float* __restrict__ q_out) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * 4 + wv;
  if (n >= N) return;  // wave-uniform
  const EpsGreedy eg(seed, step[0] + step_offset, start_e, end_e, duration);
  pqn_act_row(hidden + n * H, n, H, wq, bq, A, eg, lane, actions, values, eps_out, q_out);
}

// ---- MSE on the taken action's Q value ----------------------------------------------------------
// old = q[b, a_b];  loss = mean((G_b - old)^2);  dq[b, j] = j == a_b ? (old - G_b) * (2 / M) : 0
// (F.mse_loss(b_returns[mb], old_val) and its backward w.r.t. old_val). One workgroup: thread t
// takes rows t, t + 1024, ... in order, then block_sum's fixed order. An action outside [0, A)
// reads no memory: it is clamped to the range.
__global__ __launch_bounds__(1024) void pqn_loss_kernel(const float* __restrict__ q,
                                                        const int64_t* __restrict__ actions,
                                                        const float* __restrict__ returns,
                                                        int64_t M, int A, float norm,
                                                        float* __restrict__ dq,
                                                        float* __restrict__ stats) {
  __shared__ float scratch[16];
  float se = 0.f, sq = 0.f;
  for (int64_t b = threadIdx.x; b < M; b += blockDim.x) {
    int64_t a = actions[b];
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    const float old = q[b * A + a];
    const float diff = returns[b] - old;
    se += diff * diff;
    sq += old;
    const float gq = (old - returns[b]) * norm;
    for (int j = 0; j < A; ++j) dq[b * A + j] = j == a ? gq : 0.f;
  }
  se = block_sum(se, scratch);
  sq = block_sum(sq, scratch);
  if (threadIdx.x == 0) {
    stats[0] = se / static_cast<float>(M);  // losses/td_loss
    stats[1] = sq / static_cast<float>(M);  // losses/q_values (old_val.mean())
  }
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_q_lambda(ocppo_stream_t stream, const float* rewards, const float* values,
                              const float* dones, const float* next_q, const float* next_done,
                              int64_t T, int64_t N, int64_t A, double gamma, double q_lambda,
                              float* returns) {
  OCPPO_REQUIRE(T >= 0 && N >= 0 && T <= INT32_MAX && A >= 1 && A <= INT32_MAX,
                "ocppo_q_lambda: bad sizes T=%lld N=%lld A=%lld (T, N >= 0, A >= 1)", (long long)T,
                (long long)N, (long long)A);
  if (T == 0 || N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(rewards && values && dones && next_q && next_done && returns,
                "ocppo_q_lambda: null pointer");
  // torch rounds a Python scalar that multiplies an f32 tensor to f32 once: gamma, q_lambda and
  // 1 - q_lambda (the difference taken in double, as Python takes it)
  const float g = static_cast<float>(gamma), lam = static_cast<float>(q_lambda);
  const float oml = static_cast<float>(1.0 - q_lambda);
  clear_stale_error();
  hipLaunchKernelGGL(q_lambda_kernel, dim3(static_cast<unsigned>(ceil_div(N, 256))), dim3(256), 0,
                     as_stream(stream), rewards, values, dones, next_q, next_done, (int)T, N,
                     (int)A, g, lam, oml, returns);
  return check_launch("ocppo_q_lambda");
}

static int lnr_check(const char* who, int64_t R, int64_t E) {
  OCPPO_REQUIRE(R >= 0 && R <= INT32_MAX && E >= 1 && E <= kLnrMaxE,
                "%s: bad sizes R=%lld E=%lld (R >= 0, 1 <= E <= %d)", who, (long long)R,
                (long long)E, kLnrMaxE);
  return OCPPO_OK;
}

// columns per lane: 2, 8 or 16 at E <= 128, <= 512 and above
#define OCPPO_LNR_DISPATCH(E, CALL)                   \
  if ((E) <= 128) { constexpr int PL = 2; CALL; }     \
  else if ((E) <= 512) { constexpr int PL = 8; CALL; } \
  else { constexpr int PL = 16; CALL; }

extern "C" int ocppo_ln_relu_fwd(ocppo_stream_t stream, const float* x, const float* gamma,
                                 const float* beta, int64_t R, int64_t E, double eps, int relu,
                                 float* y, float* mean, float* rstd) {
  if (int rc = lnr_check("ocppo_ln_relu_fwd", R, E)) return rc;
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(x && gamma && beta && y && mean && rstd, "ocppo_ln_relu_fwd: null pointer");
  clear_stale_error();
  OCPPO_LNR_DISPATCH(E, hipLaunchKernelGGL((layernorm_fwd_kernel<LnRelu, PL>),
                                           dim3(grid_for(R, kLnWaves)), dim3(kLnWaves * kWave), 0,
                                           as_stream(stream), x, nullptr, gamma, beta, R, (int)E,
                                           static_cast<float>(eps), relu ? 1 : 0, y, mean, rstd));
  return check_launch("ocppo_ln_relu_fwd");
}

extern "C" size_t ocppo_ln_relu_workspace_bytes(int64_t R, int64_t E) {
  if (R < 0 || E < 1 || E > kLnrMaxE) return 0;
  return ln_workspace_bytes(R, E);
}

extern "C" int ocppo_ln_relu_bwd(ocppo_stream_t stream, const float* dy, const float* x,
                                 const float* y, const float* gamma, const float* mean,
                                 const float* rstd, int64_t R, int64_t E, int relu, float* dx,
                                 float* dgamma, float* dbeta, void* workspace,
                                 size_t workspace_bytes) {
  if (int rc = lnr_check("ocppo_ln_relu_bwd", R, E)) return rc;
  if (R == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dy && x && (y || !relu) && gamma && mean && rstd && dx && dgamma && dbeta,
                "ocppo_ln_relu_bwd: null pointer");
  if (!workspace || workspace_bytes < ocppo_ln_relu_workspace_bytes(R, E))
    return fail(OCPPO_E_WORKSPACE, "ocppo_ln_relu_bwd: workspace of %zu bytes, need %zu",
                workspace_bytes, ocppo_ln_relu_workspace_bytes(R, E));
  clear_stale_error();
  OCPPO_LNR_DISPATCH(E, return (ln_bwd_launch<LnRelu, PL>(
                            "ocppo_ln_relu_bwd", "ocppo_ln_relu_bwd (finish)", as_stream(stream),
                            dy, x, nullptr, y, gamma, mean, rstd, R, E, relu ? 1 : 0, dx, dgamma,
                            dbeta, static_cast<float*>(workspace))));
}
#undef OCPPO_LNR_DISPATCH

extern "C" int ocppo_pqn_act(ocppo_stream_t stream, const float* hidden, int64_t N, int64_t H,
                             const float* wq, const float* bq, int64_t A, uint64_t seed,
                             const int64_t* step, int64_t step_offset, double start_e,
                             double end_e, double duration, int64_t* actions, float* values,
                             float* epsilon_out, float* q_out) {
  OCPPO_REQUIRE(N >= 0 && N <= INT32_MAX && A >= 1 && A <= kPqnMaxA && H >= 4 && H % 4 == 0 &&
                    H <= kPqnMaxH && duration > 0,
                "ocppo_pqn_act: bad sizes N=%lld H=%lld A=%lld (N >= 0, 1 <= A <= %d, H a "
                "multiple of 4 in [4, %d], duration > 0)", (long long)N, (long long)H,
                (long long)A, kPqnMaxA, kPqnMaxH);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(hidden && wq && bq && step && actions && values, "ocppo_pqn_act: null pointer");
  OCPPO_REQUIRE(((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(wq)) & 15) == 0,
                "ocppo_pqn_act: hidden and wq must be 16-B aligned");
  clear_stale_error();
  hipLaunchKernelGGL(pqn_act_kernel, dim3(static_cast<unsigned>(ceil_div(N, 4))), dim3(256), 0,
                     as_stream(stream), hidden, N, (int)H, wq, bq, (int)A, seed, step, step_offset,
                     start_e, end_e, duration, actions, values, epsilon_out, q_out);
  return check_launch("ocppo_pqn_act");
}

extern "C" int ocppo_pqn_loss_fwd_bwd(ocppo_stream_t stream, const float* q,
                                      const int64_t* actions, const float* returns, int64_t M,
                                      int64_t A, float* dq, float* stats) {
  OCPPO_REQUIRE(M >= 0 && A >= 1 && A <= kPqnMaxA,
                "ocppo_pqn_loss_fwd_bwd: bad sizes M=%lld A=%lld (M >= 0, 1 <= A <= %d)",
                (long long)M, (long long)A, kPqnMaxA);
  if (M == 0) return OCPPO_OK;
  OCPPO_REQUIRE(q && actions && returns && dq && stats, "ocppo_pqn_loss_fwd_bwd: null pointer");
  clear_stale_error();
  // mse_loss backward: norm = 2 / numel (computed in double by ATen, applied in f32)
  const float norm = static_cast<float>(2.0 / static_cast<double>(M));
  hipLaunchKernelGGL(pqn_loss_kernel, dim3(1), dim3(1024), 0, as_stream(stream), q, actions,
                     returns, M, (int)A, norm, dq, stats);
  return check_launch("ocppo_pqn_loss_fwd_bwd");
}
