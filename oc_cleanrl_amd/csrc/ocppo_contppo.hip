// Continuous-action PPO / RPO (cleanrl/ppo_continuous_action.py, rpo_continuous_action.py): the
// diagonal-Gaussian head's sample, the fused minibatch loss with its backward, the wrapper chain
// of :96-100 on raw env outputs, and Pendulum-v1 as a device-resident vector env.
//
// The action width A is at most 64 = one wave: the loss gives action column a to lane a, so a
// row's log-prob is one butterfly and d loss / d logstd[a] is one register per lane. Every
// cross-row sum is two fixed-order stages (a wave's rows in order, then the waves in order): no
// atomics, results bitwise repeatable. All row offsets are int64. f32 arithmetic keeps torch's
// per-op rounding (-ffp-contract=off).
#include "ocppo_common.h"
#include "ocppo_contenv.h"
#include "ocppo_rng.h"

namespace ocppo {

constexpr int kGaussMaxA = 64;
// math.log(math.sqrt(2 * math.pi)) and 0.5 + 0.5 * math.log(2 * math.pi) (torch's Normal), as the
// f32 scalars torch's ops take them
constexpr float kLogSqrt2Pi = 0.91893853320467267f;
constexpr float kEntropyConst = 1.4189385332046727f;

// Normal(mu, sigma).log_prob(x) for one element as torch writes it: var = sigma ** 2,
// -((x - mu) ** 2) / (2 * var) - log(sigma) - log(sqrt(2 pi))
__device__ __forceinline__ float gauss_logprob(float x, float mu, float two_var, float log_sigma) {
  const float d = x - mu;
  return (-(d * d)) / two_var - log_sigma - kLogSqrt2Pi;
}

// ---- sample ------------------------------------------------------------------------------------------
// One thread per row; the A per-column constants sit in LDS. The row's log-prob is summed in
// column order.
__global__ __launch_bounds__(256) void gauss_head_sample_kernel(
    const float* __restrict__ mean, const float* __restrict__ logstd, const float* __restrict__ z,
    const float* __restrict__ value_in, int64_t N, int A, float* __restrict__ action,
    float* __restrict__ logprob, float* __restrict__ value) {
  __shared__ float s_sigma[kGaussMaxA], s_two_var[kGaussMaxA], s_log_sigma[kGaussMaxA];
  if (threadIdx.x < A) {
    const float sg = expf(logstd[threadIdx.x]);
    s_sigma[threadIdx.x] = sg;
    s_two_var[threadIdx.x] = 2.0f * (sg * sg);
    s_log_sigma[threadIdx.x] = logf(sg);
  }
  __syncthreads();
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; n < N;
       n += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t row = n * A;
    float lp = 0.f;
    for (int a = 0; a < A; ++a) {
      const float mu = mean[row + a];
      const float x = z[row + a] * s_sigma[a] + mu;  // torch.normal: two roundings, no FMA
      action[row + a] = x;
      const float e = gauss_logprob(x, mu, s_two_var[a], s_log_sigma[a]);
      lp = a == 0 ? e : lp + e;
    }
    logprob[n] = lp;
    value[n] = value_in[n];
  }
}

// ---- fused loss ------------------------------------------------------------------------------------
constexpr int kGaussLossThreads = 1024;
constexpr int kGaussLossWaves = kGaussLossThreads / kWave;
constexpr int kGaussParts = 6;  // pg, v, (unused), old_kl, kl, clipfrac: ocppo_loss.hip's order

struct GaussLossParams {
  const float* mean;
  const float* logstd;
  const float* new_value;
  const float* actions;
  const float* old_lp;
  const float* adv;
  const float* ret;
  const float* val;
  const float* adv_stats;
  float* dmean;
  float* dvalue;
  float* dlogstd;
  float* stats;
  int64_t M;
  int A;
  int norm_adv, clip_vloss;
  float clip, clip_lo, clip_hi, ent_coef, vf_coef, g_pg, g_h, g_v, inv_m;
  uint64_t seed;          // RPO
  const int64_t* counter;
  int64_t mb;
  float alpha;
};

// One workgroup: wave w takes rows w, w + 16, ...; lane a owns action column a. The scalar part of
// a row (ratio, surrogate, value loss and their backward) is ocppo_ppo_loss_fwd_bwd's, ties of the
// two max() included (the gradient splits 1/2 - 1/2; clamp passes it at the bounds).
__global__ __launch_bounds__(kGaussLossThreads) void gauss_ppo_loss_kernel(GaussLossParams P) {
  __shared__ float s_part[kGaussLossWaves][kGaussParts];
  __shared__ float s_dls[kGaussLossWaves][kGaussMaxA];
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const int A = P.A;
  const bool on = lane < A;
  const float ls = on ? P.logstd[lane] : 0.f;
  const float sigma = expf(ls);
  const float var = sigma * sigma;
  const float two_var = 2.0f * var;
  const float log_sigma = logf(sigma);
  // Normal.entropy() = 0.5 + 0.5 log(2 pi) + log(sigma), summed over the columns. The policy's
  // sigma does not depend on the state, so this is every row's entropy and their mean as well
  // (reported as it is: summing M copies would only add rounding)
  const float H = wave_sum(on ? kEntropyConst + log_sigma : 0.f);
  // d log_prob / d sigma through var = sigma ** 2 and log(sigma) is row-dependent; the entropy's
  // is g_h / sigma per row; both reach logstd through exp's backward (* sigma)
  const float adv_mean = P.norm_adv ? P.adv_stats[0] : 0.f;
  const float adv_den = P.norm_adv ? P.adv_stats[1] + 1e-8f : 1.f;
  const bool rpo = P.alpha > 0.f;
  const int64_t counter = rpo ? P.counter[0] : 0;
  float part[kGaussParts] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float dls = 0.f;
  for (int64_t m = wid; m < P.M; m += kGaussLossWaves) {
    const int64_t e = m * A + lane;
    float mu = on ? P.mean[e] : 0.f;
    if (rpo && on) mu = mu + rpo_noise(P.seed, counter, P.mb, m, lane, P.alpha);
    const float x = on ? P.actions[e] : 0.f;
    const float d = x - mu;
    const float t = d * d;
    const float new_lp = wave_sum(on ? (-t) / two_var - log_sigma - kLogSqrt2Pi : 0.f);
    const float old_lp = P.old_lp[m], adv = P.adv[m], R = P.ret[m], v_old = P.val[m];
    const float v = P.new_value[m];

    const float logratio = new_lp - old_lp;
    const float ratio = expf(logratio);
    part[3] += -logratio;
    part[4] += (ratio - 1.0f) - logratio;
    part[5] += fabsf(ratio - 1.0f) > P.clip ? 1.f : 0.f;
    float advn = adv;
    if (P.norm_adv) advn = (adv - adv_mean) / adv_den;
    const float nadv = -advn;
    const float pg1 = nadv * ratio;
    const float rc = fminf(fmaxf(ratio, P.clip_lo), P.clip_hi);
    const float pg2 = nadv * rc;
    part[0] += fmaxf(pg1, pg2);
    const float du = v - R;
    const float vu = du * du;
    float dv;
    if (P.clip_vloss) {
      const float dvv = v - v_old;
      const float dvc = fminf(fmaxf(dvv, -P.clip), P.clip);
      const float vcl = v_old + dvc;
      const float dc = vcl - R;
      const float vc = dc * dc;
      part[1] += fmaxf(vu, vc);
      const float gu = vu > vc ? P.g_v : (vu == vc ? P.g_v / 2.f : 0.f);
      const float gc = vc > vu ? P.g_v : (vu == vc ? P.g_v / 2.f : 0.f);
      const float tu = gu * (2.0f * du);
      float tc = gc * (2.0f * dc);
      tc = (dvv >= -P.clip && dvv <= P.clip) ? tc : 0.f;
      dv = tu + tc;
    } else {
      part[1] += vu;
      dv = P.g_v * (2.0f * du);
    }
    const float g1 = pg1 > pg2 ? P.g_pg : (pg1 == pg2 ? P.g_pg / 2.f : 0.f);
    const float g2 = pg2 > pg1 ? P.g_pg : (pg1 == pg2 ? P.g_pg / 2.f : 0.f);
    const float dr1 = g1 * nadv;
    const float dr2 = (ratio >= P.clip_lo && ratio <= P.clip_hi) ? g2 * nadv : 0.f;
    const float g_lp = (dr1 + dr2) * ratio;  // d loss / d new_logprob, the same for every column

    if (on) {
      P.dmean[e] = g_lp * ((2.0f * d) / two_var);
      // d/d sigma of -t / (2 var) - log(sigma): t / (2 var)^2 * 2 * (2 sigma) - 1 / sigma
      const float dsig = g_lp * ((t / (two_var * two_var)) * 2.0f * (2.0f * sigma) - 1.0f / sigma) +
                         P.g_h / sigma;
      dls += dsig * sigma;
    }
    if (lane == 0) P.dvalue[m] = dv;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kGaussParts; ++k) s_part[wid][k] = part[k];
  }
  s_dls[wid][lane] = dls;
  __syncthreads();
  if (threadIdx.x < A) {
    float s = s_dls[0][threadIdx.x];
    for (int w = 1; w < kGaussLossWaves; ++w) s += s_dls[w][threadIdx.x];
    P.dlogstd[threadIdx.x] = s;
  }
  if (threadIdx.x == 0) {
    float s[kGaussParts];
#pragma unroll
    for (int k = 0; k < kGaussParts; ++k) {
      s[k] = s_part[0][k];
      for (int w = 1; w < kGaussLossWaves; ++w) s[k] += s_part[w][k];
    }
    const float pg_loss = s[0] * P.inv_m;
    const float v_loss = 0.5f * (s[1] * P.inv_m);
    const float ent = H;
    P.stats[OCPPO_STAT_LOSS] = (pg_loss - P.ent_coef * ent) + v_loss * P.vf_coef;
    P.stats[OCPPO_STAT_PG_LOSS] = pg_loss;
    P.stats[OCPPO_STAT_V_LOSS] = v_loss;
    P.stats[OCPPO_STAT_ENTROPY] = ent;
    P.stats[OCPPO_STAT_OLD_APPROX_KL] = s[3] * P.inv_m;
    P.stats[OCPPO_STAT_APPROX_KL] = s[4] * P.inv_m;
    P.stats[OCPPO_STAT_CLIPFRAC] = s[5] * P.inv_m;
    P.stats[OCPPO_STAT_ADV_MEAN] = P.norm_adv ? P.adv_stats[0] : 0.f;
    P.stats[OCPPO_STAT_ADV_STD] = P.norm_adv ? P.adv_stats[1] : 0.f;
  }
}

__global__ __launch_bounds__(256) void rpo_noise_kernel(uint64_t seed,
                                                        const int64_t* __restrict__ counter,
                                                        int64_t mb, int64_t M, int A, float alpha,
                                                        float* __restrict__ out) {
  const int64_t total = M * A;
  const int64_t c = counter[0];
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t m = i / A;
    out[i] = rpo_noise(seed, c, mb, m, static_cast<int>(i - m * A), alpha);
  }
}

// ---- wrapper chain on raw env outputs ----------------------------------------------------------------
__global__ __launch_bounds__(256) void env_normalize_kernel(
    const float* __restrict__ obs, const float* __restrict__ final_obs,
    const float* __restrict__ reward, const float* __restrict__ terminated,
    const float* __restrict__ truncated, int64_t N, int64_t D, ContNorm cn,
    float* __restrict__ obs_out, float* __restrict__ reward_out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const bool term = terminated && terminated[n] != 0.f;
  const bool done = term || (truncated && truncated[n] != 0.f);
  cont_norm_env(cn, n, D, obs + n * D, final_obs ? final_obs + n * D : nullptr,
                done && final_obs != nullptr, term, reward != nullptr, reward ? reward[n] : 0.f,
                obs_out + n * D, reward_out ? reward_out + n : nullptr);
}

// ---- Pendulum-v1 ---------------------------------------------------------------------------------------
namespace pendulum {
constexpr double kMaxSpeed = 8.0;
constexpr double kMaxTorque = 2.0;
constexpr double kDt = 0.05;
constexpr double kG = 10.0;
constexpr double kM = 1.0;
constexpr double kL = 1.0;
constexpr double kPi = 3.141592653589793;
constexpr int64_t kMaxSteps = 200;
}  // namespace pendulum

// theta ~ U(-pi, pi), theta_dot ~ U(-1, 1) as numpy computes low + (high - low) * u, from
// cartpole_reset_state's stream of (seed, env, episode)
__device__ __forceinline__ void pendulum_reset_state(uint64_t seed, int64_t n, int64_t episode,
                                                     double* st) {
  const uint64_t key = env_reset_key(seed, n, episode);
  const double hi[2] = {pendulum::kPi, 1.0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double u = unit53(splitmix64(key + static_cast<uint64_t>(i)));
    st[i] = -hi[i] + (hi[i] - -hi[i]) * u;
  }
}

__device__ __forceinline__ void pendulum_obs(const double* st, float* o) {
  o[0] = static_cast<float>(cos(st[0]));
  o[1] = static_cast<float>(sin(st[0]));
  o[2] = static_cast<float>(st[1]);
}

// One thread per env, the state in HBM between launches (ocppo_cartpole_step's structure). With
// cn.state set the wrapper chain runs on the thread's raw outputs before they are stored: bitwise
// the raw launch followed by env_normalize_kernel.
__global__ __launch_bounds__(256) void pendulum_step_kernel(
    uint64_t seed, const float* __restrict__ actions, int64_t N, double* __restrict__ state,
    int64_t* __restrict__ counters, float* __restrict__ obs_out, float* __restrict__ final_obs_out,
    float* __restrict__ reward_out, float* __restrict__ done_out, float* __restrict__ ep,
    ContNorm cn) {
  using namespace pendulum;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double st[2] = {state[2 * n], state[2 * n + 1]};
  int64_t elapsed = counters[2 * n];
  const int64_t episode = counters[2 * n + 1];
  float o[3], fo[3] = {0.f, 0.f, 0.f};
  if (actions == nullptr) {  // env.reset()
    pendulum_reset_state(seed, n, episode, st);
    counters[2 * n] = 0;
    counters[2 * n + 1] = episode + 1;
    state[2 * n] = st[0];
    state[2 * n + 1] = st[1];
    pendulum_obs(st, o);
    cont_norm_env(cn, n, 3, o, fo, false, false, false, 0.f, obs_out + 3 * n, nullptr);
    if (final_obs_out)
      for (int i = 0; i < 3; ++i) final_obs_out[3 * n + i] = o[i];
    if (reward_out) reward_out[n] = 0.f;
    if (done_out) done_out[n] = 0.f;
    return;
  }
  // pendulum.py step() behind ClipAction; Python evaluates left to right, no FMA
  const double th = st[0], thdot = st[1];
  double u = static_cast<double>(actions[n]);
  u = u < -kMaxTorque ? -kMaxTorque : (u > kMaxTorque ? kMaxTorque : u);
  double an = fmod(th + kPi, 2.0 * kPi);  // angle_normalize: Python's %, the divisor's sign
  if (an < 0.0) an += 2.0 * kPi;
  an = an - kPi;
  const double costs = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u);
  double newthdot = thdot + (3.0 * kG / (2.0 * kL) * sin(th) + 3.0 / (kM * (kL * kL)) * u) * kDt;
  newthdot = newthdot < -kMaxSpeed ? -kMaxSpeed : (newthdot > kMaxSpeed ? kMaxSpeed : newthdot);
  st[0] = th + newthdot * kDt;
  st[1] = newthdot;
  elapsed += 1;
  const bool done = elapsed >= kMaxSteps;  // TimeLimit(200): truncation, never termination
  const float r = static_cast<float>(-costs);
  if (ep) {  // RecordEpisodeStatistics on the raw reward
    float* e = ep + n * 5;
    const float run_ret = e[0] + r, run_len = e[1] + 1.f;
    if (done) {
      e[2] += run_ret;
      e[3] += run_len;
      e[4] += 1.f;
      e[0] = 0.f;
      e[1] = 0.f;
    } else {
      e[0] = run_ret;
      e[1] = run_len;
    }
  }
  pendulum_obs(st, fo);  // the terminal observation when done
  if (done) {            // SyncVectorEnv's same-step auto-reset
    pendulum_reset_state(seed, n, episode, st);
    elapsed = 0;
    counters[2 * n + 1] = episode + 1;
  }
  counters[2 * n] = elapsed;
  state[2 * n] = st[0];
  state[2 * n + 1] = st[1];
  pendulum_obs(st, o);
  cont_norm_env(cn, n, 3, o, fo, done, false, true, r, obs_out + 3 * n, reward_out + n);
  if (final_obs_out)
    for (int i = 0; i < 3; ++i) final_obs_out[3 * n + i] = fo[i];
  done_out[n] = done ? 1.f : 0.f;
}

static int check_norm(const char* who, const double* norm_state, double gamma) {
  OCPPO_REQUIRE(!norm_state || (gamma >= 0.0 && gamma <= 1.0), "%s: gamma must be in [0, 1]", who);
  return OCPPO_OK;
}

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_gauss_head_sample(ocppo_stream_t stream, const float* mean,
                                       const float* logstd, const float* z, const float* value_in,
                                       int64_t N, int64_t A, float* action, float* logprob,
                                       float* value) {
  OCPPO_REQUIRE(N >= 0 && A >= 1, "ocppo_gauss_head_sample: bad sizes N=%lld A=%lld", (long long)N,
                (long long)A);
  OCPPO_REQUIRE(A <= kGaussMaxA, "ocppo_gauss_head_sample: A <= 64 required, got %lld",
                (long long)A);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(mean && logstd && z && value_in && action && logprob && value,
                "ocppo_gauss_head_sample: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(gauss_head_sample_kernel, dim3(grid_for(N, 256)), dim3(256), 0,
                     as_stream(stream), mean, logstd, z, value_in, N, static_cast<int>(A), action,
                     logprob, value);
  return check_launch("ocppo_gauss_head_sample");
}

extern "C" int ocppo_gauss_ppo_loss_fwd_bwd(
    ocppo_stream_t stream, const float* mean, const float* logstd, const float* new_value,
    int64_t M, int64_t A, const float* actions, const float* logprobs, const float* advantages,
    const float* returns, const float* values, const float* adv_stats, double clip_coef,
    double ent_coef, double vf_coef, int norm_adv, int clip_vloss, uint64_t seed,
    const int64_t* rpo_counter, int64_t mb, double rpo_alpha, float* dmean, float* dvalue,
    float* dlogstd, float* stats) {
  OCPPO_REQUIRE(M >= 1 && A >= 1, "ocppo_gauss_ppo_loss_fwd_bwd: bad sizes M=%lld A=%lld",
                (long long)M, (long long)A);
  OCPPO_REQUIRE(A <= kGaussMaxA, "ocppo_gauss_ppo_loss_fwd_bwd: A <= 64 required, got %lld",
                (long long)A);
  OCPPO_REQUIRE(rpo_alpha >= 0.0 && mb >= 0, "ocppo_gauss_ppo_loss_fwd_bwd: rpo_alpha and the "
                "minibatch index must not be negative");
  OCPPO_REQUIRE(mean && logstd && new_value && actions && logprobs && advantages && returns &&
                    values && dmean && dvalue && dlogstd && stats,
                "ocppo_gauss_ppo_loss_fwd_bwd: null pointer");
  OCPPO_REQUIRE(!norm_adv || adv_stats, "ocppo_gauss_ppo_loss_fwd_bwd: norm_adv needs adv_stats");
  OCPPO_REQUIRE(rpo_alpha == 0.0 || rpo_counter,
                "ocppo_gauss_ppo_loss_fwd_bwd: rpo_alpha > 0 needs the device counter");
  GaussLossParams P;
  P.mean = mean; P.logstd = logstd; P.new_value = new_value; P.actions = actions;
  P.old_lp = logprobs; P.adv = advantages; P.ret = returns; P.val = values;
  P.adv_stats = adv_stats; P.dmean = dmean; P.dvalue = dvalue; P.dlogstd = dlogstd;
  P.stats = stats; P.M = M; P.A = static_cast<int>(A);
  P.norm_adv = norm_adv ? 1 : 0;
  P.clip_vloss = clip_vloss ? 1 : 0;
  P.clip = static_cast<float>(clip_coef);
  P.clip_lo = static_cast<float>(1.0 - clip_coef);
  P.clip_hi = static_cast<float>(1.0 + clip_coef);
  P.ent_coef = static_cast<float>(ent_coef);
  P.vf_coef = static_cast<float>(vf_coef);
  const float fm = static_cast<float>(M);
  P.g_pg = 1.0f / fm;  // the upstream grads of ocppo_ppo_loss_fwd_bwd (mean() backward)
  P.g_h = (-1.0f * P.ent_coef) / fm;
  P.g_v = (P.vf_coef * 0.5f) / fm;
  P.inv_m = 1.0f / fm;
  P.seed = seed; P.counter = rpo_counter; P.mb = mb;
  P.alpha = static_cast<float>(rpo_alpha);
  clear_stale_error();
  hipLaunchKernelGGL(gauss_ppo_loss_kernel, dim3(1), dim3(kGaussLossThreads), 0, as_stream(stream),
                     P);
  return check_launch("ocppo_gauss_ppo_loss_fwd_bwd");
}

extern "C" int ocppo_rpo_noise(ocppo_stream_t stream, uint64_t seed, const int64_t* rpo_counter,
                               int64_t mb, int64_t M, int64_t A, double rpo_alpha, float* out) {
  OCPPO_REQUIRE(M >= 0 && A >= 1 && A <= kGaussMaxA && mb >= 0 && rpo_alpha >= 0.0,
                "ocppo_rpo_noise: bad arguments M=%lld A=%lld mb=%lld", (long long)M, (long long)A,
                (long long)mb);
  if (M == 0) return OCPPO_OK;
  OCPPO_REQUIRE(rpo_counter && out, "ocppo_rpo_noise: null pointer");
  clear_stale_error();
  hipLaunchKernelGGL(rpo_noise_kernel, dim3(grid_for(M * A, 256)), dim3(256), 0, as_stream(stream),
                     seed, rpo_counter, mb, M, static_cast<int>(A), static_cast<float>(rpo_alpha),
                     out);
  return check_launch("ocppo_rpo_noise");
}

extern "C" int ocppo_env_normalize(ocppo_stream_t stream, const float* obs, const float* final_obs,
                                   const float* reward, const float* terminated,
                                   const float* truncated, int64_t N, int64_t D, double* norm_state,
                                   int norm_obs, int norm_reward, double gamma, float* obs_out,
                                   float* reward_out) {
  OCPPO_REQUIRE(N >= 0 && D >= 1, "ocppo_env_normalize: bad sizes N=%lld D=%lld", (long long)N,
                (long long)D);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(N <= 256 * 4096, "ocppo_env_normalize: N <= 1048576 required");
  OCPPO_REQUIRE(obs && obs_out && norm_state, "ocppo_env_normalize: null pointer");
  OCPPO_REQUIRE(!reward || reward_out, "ocppo_env_normalize: a reward needs reward_out");
  OCPPO_REQUIRE(final_obs || !(terminated || truncated),
                "ocppo_env_normalize: done flags need the terminal observations");
  if (int rc = check_norm("ocppo_env_normalize", norm_state, gamma)) return rc;
  const ContNorm cn{norm_state, norm_obs ? 1 : 0, norm_reward ? 1 : 0, gamma};
  clear_stale_error();
  hipLaunchKernelGGL(env_normalize_kernel, dim3(grid_for(N, 256)), dim3(256), 0, as_stream(stream),
                     obs, final_obs, reward, terminated, truncated, N, D, cn, obs_out, reward_out);
  return check_launch("ocppo_env_normalize");
}

extern "C" int ocppo_pendulum_step(ocppo_stream_t stream, uint64_t seed, const float* actions,
                                   int64_t N, double* state, int64_t* counters, float* obs_out,
                                   float* final_obs_out, float* reward_out, float* done_out,
                                   float* ep_state, double* norm_state, int norm_obs,
                                   int norm_reward, double gamma) {
  OCPPO_REQUIRE(N >= 0, "ocppo_pendulum_step: bad size N=%lld", (long long)N);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(state && counters && obs_out, "ocppo_pendulum_step: null pointer");
  OCPPO_REQUIRE(actions == nullptr || (reward_out && done_out),
                "ocppo_pendulum_step: a step needs reward_out and done_out");
  if (int rc = check_norm("ocppo_pendulum_step", norm_state, gamma)) return rc;
  const ContNorm cn{norm_state, norm_obs ? 1 : 0, norm_reward ? 1 : 0, gamma};
  clear_stale_error();
  // the grid covers every env: grid_for caps at 4096 blocks, so N is bounded here
  OCPPO_REQUIRE(N <= 256 * 4096, "ocppo_pendulum_step: N <= 1048576 required");
  hipLaunchKernelGGL(pendulum_step_kernel, dim3(grid_for(N, 256)), dim3(256), 0, as_stream(stream),
                     seed, actions, N, state, counters, obs_out, final_obs_out, reward_out,
                     done_out, ep_state, cn);
  return check_launch("ocppo_pendulum_step");
}
