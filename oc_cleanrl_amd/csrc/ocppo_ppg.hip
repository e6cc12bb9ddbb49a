// Phasic Policy Gradient's auxiliary phase (cleanrl/ppg_procgen.py:420-477) beyond PPO:
//
//   ocppo_ppg_aux_gather       : one launch writes an auxiliary minibatch -- whole env columns
//                                cols [k] of aux_obs [T, R, D] / aux_pi [T, R, A] / aux_returns
//                                [T, R] -- flattened t-major ([T k, ...], the script's flatten01 of
//                                aux_*[:, ind], :443-453), the observations converted from their
//                                storage dtype to the f32 the trunk reads.
//   ocppo_ppg_aux_loss_fwd_bwd : KL(old policy || new policy) + the two value regressions with
//                                their three gradients (:449-461), two launches (row pass, finish).
//
// Both are capture-safe (no host scalars read back), deterministic (no atomics; the sums run in an
// order the sizes fix) and check their arguments before any launch.
#include "ocppo_categorical.h"
#include "ocppo_common.h"

namespace ocppo {

constexpr int kPpgThreads = kWave;      // one wave per workgroup: 64 rows per wave and per block
constexpr int kPpgMaxBlocks = 1024;     // rows beyond 64 * 1024 are grid-strided
constexpr int kPpgMaxActions = 18;
constexpr int kPpgWsHeader = 8;         // doubles in front of the workspace's partials

// One thread per row. Both logit rows go through categorical_row, the normalisation the loss and
// rollout kernels use, so a row whose old and new logits are bit-equal has p_new == p_old and
// ln_new == ln_old bit for bit: kl_r == 0 and an all-zero dlogits row exactly.
//   kl_r = sum_j p_old (ln_old - ln_new), with torch.distributions.kl's two masks: a term whose
//   p_old is 0 counts 0, a term whose p_new is 0 (p_old not) counts +inf
//   dlogits = (p_new - p_old) * f32(beta / M); dvalue = (v - R) * f32(1 / M); daux likewise
// Per block the f64 partials {sum kl_r, sum (aux - R)^2, sum (v - R)^2} -> ws[header + 3 block ..].
template <int AMAX>
__global__ __launch_bounds__(kPpgThreads) void ppg_aux_loss_kernel(
    const float* __restrict__ new_logits, const float* __restrict__ new_value,
    const float* __restrict__ new_aux, const float* __restrict__ old_logits,
    const float* __restrict__ returns, int64_t M, int A, float kscale, float vscale,
    float* __restrict__ dlogits, float* __restrict__ dvalue, float* __restrict__ daux,
    double* __restrict__ ws) {
  double kl = 0.0, al = 0.0, vl = 0.0;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kPpgThreads + threadIdx.x; r < M;
       r += static_cast<int64_t>(gridDim.x) * kPpgThreads) {
    float ln_[AMAX], lo_[AMAX], lnn[AMAX], lno[AMAX], pn[AMAX], po[AMAX], lse;
#pragma unroll
    for (int j = 0; j < AMAX; ++j) {
      ln_[j] = j < A ? new_logits[r * A + j] : 0.f;
      lo_[j] = j < A ? old_logits[r * A + j] : 0.f;
    }
    categorical_row<AMAX>(ln_, A, lse, lnn, pn);
    categorical_row<AMAX>(lo_, A, lse, lno, po);
    float k = 0.f;
#pragma unroll
    for (int j = 0; j < AMAX; ++j)
      if (j < A) {
        float t = po[j] * (lno[j] - lnn[j]);
        if (pn[j] == 0.f) t = INFINITY;
        if (po[j] == 0.f) t = 0.f;
        k += t;
        dlogits[r * A + j] = (pn[j] - po[j]) * kscale;
      }
    kl += static_cast<double>(k);
    const float ret = returns[r];
    const float dv = new_value[r] - ret, da = new_aux[r] - ret;
    vl += static_cast<double>(dv) * static_cast<double>(dv);
    al += static_cast<double>(da) * static_cast<double>(da);
    dvalue[r] = dv * vscale;
    daux[r] = da * vscale;
  }
  kl = wave_sum(kl);
  al = wave_sum(al);
  vl = wave_sum(vl);
  if (threadIdx.x == 0) {
    double* o = ws + kPpgWsHeader + static_cast<int64_t>(blockIdx.x) * 3;
    o[0] = kl;
    o[1] = al;
    o[2] = vl;
  }
}

// stats = {mean kl_r, 0.5 mean (aux - R)^2, 0.5 mean (v - R)^2}: the blocks' partials b, b + 256, ..
// in thread b, then the fixed block sum
__global__ __launch_bounds__(256) void ppg_aux_finish_kernel(const double* __restrict__ ws,
                                                             int nparts, int64_t M,
                                                             float* __restrict__ stats) {
  __shared__ double scratch[256 / kWave];
  double kl = 0.0, al = 0.0, vl = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) {
    kl += ws[kPpgWsHeader + k * 3];
    al += ws[kPpgWsHeader + k * 3 + 1];
    vl += ws[kPpgWsHeader + k * 3 + 2];
  }
  kl = block_sum(kl, scratch);
  al = block_sum(al, scratch);
  vl = block_sum(vl, scratch);
  if (threadIdx.x == 0) {
    const double m = static_cast<double>(M);
    stats[0] = static_cast<float>(kl / m);
    stats[1] = static_cast<float>(0.5 * al / m);
    stats[2] = static_cast<float>(0.5 * vl / m);
  }
}

static int64_t ppg_aux_grid(int64_t M) {
  const int64_t g = ceil_div(M, kPpgThreads);
  return g < kPpgMaxBlocks ? g : kPpgMaxBlocks;
}

// A column index outside [0, R) is never dereferenced: it reads column 0 or R - 1 (the clamp of
// clamp_action); the host wrapper refuses such an index where it can see it.
__device__ __forceinline__ int64_t clamp_col(int64_t c, int64_t R) {
  return c < 0 ? 0 : (c >= R ? R - 1 : c);
}

// The flat work list: T k (D / VEC) observation groups, then T k (A / PV) logit groups, then T k
// returns. Output row = t k + c reads column cols[c] of step t.
template <int SDT, int VEC, int PV>
__global__ __launch_bounds__(256) void ppg_aux_gather_kernel(
    const void* __restrict__ obs, const float* __restrict__ pi, const float* __restrict__ ret,
    const int64_t* __restrict__ cols, int64_t T, int64_t R, int64_t k, int64_t D, int64_t A,
    float* __restrict__ out_obs, float* __restrict__ out_pi, float* __restrict__ out_ret) {
  const int64_t rows = T * k;
  const int64_t DG = D / VEC, AG = A / PV;
  const int64_t n_obs = rows * DG, n_pi = rows * AG;
  const int64_t total = n_obs + n_pi + rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total;
       g += stride) {
    if (g < n_obs) {
      const int64_t row = g / DG, e = (g - row * DG) * VEC;
      const int64_t t = row / k, c = row - t * k;
      const int64_t col = clamp_col(cols[c], R);
      float v[VEC];
      VecIO<SDT, VEC>::load(obs, (t * R + col) * D + e, v);
      VecIO<OCPPO_F32, VEC>::store(out_obs, row * D + e, v);
    } else if (g < n_obs + n_pi) {
      const int64_t q = g - n_obs;
      const int64_t row = q / AG, e = (q - row * AG) * PV;
      const int64_t t = row / k, c = row - t * k;
      const int64_t col = clamp_col(cols[c], R);
      float v[PV];
      VecIO<OCPPO_F32, PV>::load(pi, (t * R + col) * A + e, v);
      VecIO<OCPPO_F32, PV>::store(out_pi, row * A + e, v);
    } else {
      const int64_t row = g - n_obs - n_pi;
      const int64_t t = row / k, c = row - t * k;
      out_ret[row] = ret[t * R + clamp_col(cols[c], R)];
    }
  }
}

template <int SDT, int VEC, int PV>
static int launch_ppg_gather(hipStream_t s, const void* obs, const float* pi, const float* ret,
                             const int64_t* cols, int64_t T, int64_t R, int64_t k, int64_t D,
                             int64_t A, float* out_obs, float* out_pi, float* out_ret) {
  const int64_t rows = T * k;
  const int64_t total = rows * (D / VEC) + rows * (A / PV) + rows;
  hipLaunchKernelGGL((ppg_aux_gather_kernel<SDT, VEC, PV>), dim3(grid_for(total, 256)), dim3(256),
                     0, s, obs, pi, ret, cols, T, R, k, D, A, out_obs, out_pi, out_ret);
  return check_launch("ocppo_ppg_aux_gather");
}

template <int SDT>
static int launch_ppg_gather_dt(hipStream_t s, bool v4, bool p4, const void* obs, const float* pi,
                                const float* ret, const int64_t* cols, int64_t T, int64_t R,
                                int64_t k, int64_t D, int64_t A, float* out_obs, float* out_pi,
                                float* out_ret) {
#define OCPPO_PPG_GATHER(V, P) \
  return launch_ppg_gather<SDT, V, P>(s, obs, pi, ret, cols, T, R, k, D, A, out_obs, out_pi, out_ret)
  if (v4 && p4) OCPPO_PPG_GATHER(4, 4);
  if (v4) OCPPO_PPG_GATHER(4, 1);
  if (p4) OCPPO_PPG_GATHER(1, 4);
  OCPPO_PPG_GATHER(1, 1);
#undef OCPPO_PPG_GATHER
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_ppg_aux_loss_workspace_bytes(int64_t M) {
  if (M < 1) return 0;
  return static_cast<size_t>(kPpgWsHeader + ppg_aux_grid(M) * 3) * sizeof(double);
}

extern "C" int ocppo_ppg_aux_loss_fwd_bwd(ocppo_stream_t stream, const float* new_logits,
                                          const float* new_value, const float* new_aux_value,
                                          const float* old_logits, const float* returns,
                                          int64_t M, int64_t A, double beta_clone, float* dlogits,
                                          float* dvalue, float* daux, float* stats,
                                          void* workspace, size_t workspace_bytes) {
  OCPPO_REQUIRE(M >= 1 && A >= 1 && A <= kPpgMaxActions,
                "ocppo_ppg_aux_loss_fwd_bwd: bad sizes M=%lld A=%lld (M >= 1, 1 <= A <= %d)",
                (long long)M, (long long)A, kPpgMaxActions);
  OCPPO_REQUIRE(new_logits && new_value && new_aux_value && old_logits && returns && dlogits &&
                    dvalue && daux && stats && workspace,
                "ocppo_ppg_aux_loss_fwd_bwd: null pointer");
  if (workspace_bytes < ocppo_ppg_aux_loss_workspace_bytes(M) ||
      reinterpret_cast<uintptr_t>(workspace) % 8)
    return fail(OCPPO_E_WORKSPACE,
                "ocppo_ppg_aux_loss_fwd_bwd: workspace of %zu bytes (8-B aligned) needed",
                ocppo_ppg_aux_loss_workspace_bytes(M));
  double* ws = static_cast<double*>(workspace);
  const int64_t grid = ppg_aux_grid(M);
  const float kscale = static_cast<float>(beta_clone / static_cast<double>(M));
  const float vscale = static_cast<float>(1.0 / static_cast<double>(M));
  hipStream_t s = as_stream(stream);
  clear_stale_error();
#define OCPPO_PPG_AUX(AM)                                                                        \
  hipLaunchKernelGGL(ppg_aux_loss_kernel<AM>, dim3(static_cast<unsigned>(grid)),                 \
                     dim3(kPpgThreads), 0, s, new_logits, new_value, new_aux_value, old_logits,  \
                     returns, M, static_cast<int>(A), kscale, vscale, dlogits, dvalue, daux, ws)
  if (A <= 8) OCPPO_PPG_AUX(8);
  else OCPPO_PPG_AUX(kPpgMaxActions);
#undef OCPPO_PPG_AUX
  if (int rc = check_launch("ocppo_ppg_aux_loss_fwd_bwd")) return rc;
  hipLaunchKernelGGL(ppg_aux_finish_kernel, dim3(1), dim3(256), 0, s, ws, static_cast<int>(grid),
                     M, stats);
  return check_launch("ocppo_ppg_aux_loss_fwd_bwd (finish)");
}

extern "C" int ocppo_ppg_aux_gather(ocppo_stream_t stream, const void* aux_obs, int obs_dtype,
                                    const float* aux_pi, const float* aux_returns,
                                    const int64_t* cols, int64_t T, int64_t R, int64_t k,
                                    int64_t D, int64_t A, float* out_obs, float* out_pi,
                                    float* out_returns) {
  OCPPO_REQUIRE(T >= 1 && R >= 1 && k >= 1 && D >= 1 && A >= 1 && T <= INT32_MAX &&
                    R <= INT32_MAX && k <= INT32_MAX && D <= INT32_MAX && A <= INT32_MAX,
                "ocppo_ppg_aux_gather: bad sizes T=%lld R=%lld k=%lld D=%lld A=%lld",
                (long long)T, (long long)R, (long long)k, (long long)D, (long long)A);
  OCPPO_REQUIRE(obs_dtype == OCPPO_F32 || obs_dtype == OCPPO_BF16 || obs_dtype == OCPPO_U8,
                "ocppo_ppg_aux_gather: dtype %d is not OCPPO_F32 / OCPPO_BF16 / OCPPO_U8",
                obs_dtype);
  OCPPO_REQUIRE(aux_obs && aux_pi && aux_returns && cols && out_obs && out_pi && out_returns,
                "ocppo_ppg_aux_gather: null pointer");
  // 16-byte stores (and 16 / 8 / 4-byte loads of four elements) where the row length and the
  // pointers allow, element by element otherwise
  const size_t esz = obs_dtype == OCPPO_F32 ? 4 : obs_dtype == OCPPO_BF16 ? 2 : 1;
  const bool v4 = D % 4 == 0 && reinterpret_cast<uintptr_t>(aux_obs) % (4 * esz) == 0 &&
                  reinterpret_cast<uintptr_t>(out_obs) % 16 == 0;
  const bool p4 = A % 4 == 0 && reinterpret_cast<uintptr_t>(aux_pi) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out_pi) % 16 == 0;
  hipStream_t s = as_stream(stream);
  clear_stale_error();
  if (obs_dtype == OCPPO_F32)
    return launch_ppg_gather_dt<OCPPO_F32>(s, v4, p4, aux_obs, aux_pi, aux_returns, cols, T, R, k,
                                           D, A, out_obs, out_pi, out_returns);
  if (obs_dtype == OCPPO_BF16)
    return launch_ppg_gather_dt<OCPPO_BF16>(s, v4, p4, aux_obs, aux_pi, aux_returns, cols, T, R,
                                            k, D, A, out_obs, out_pi, out_returns);
  return launch_ppg_gather_dt<OCPPO_U8>(s, v4, p4, aux_obs, aux_pi, aux_returns, cols, T, R, k, D,
                                        A, out_obs, out_pi, out_returns);
}
