// The recurrence of the LSTM PPO agent of cleanrl/ppo_atari_lstm.py:140-158 (Agent.get_states: one
// nn.LSTM call per time step, because the per-step `done` reset rules out a whole-sequence LSTM):
// a whole sequence forward in one launch, its BPTT in one launch, and the rollout's single step.
// f32 throughout; gate order i | f | g | o, W_ih [4H, I], W_hh [4H, H] as nn.LSTM stores them.
//
// Geometry (sequence kernels): ONE WORKGROUP PER ENVIRONMENT, 4H threads, alive for the whole
// sequence. Environments are independent, so there is no barrier, flag or atomic between
// workgroups and no co-residency assumption; a grid larger than the chip simply runs in turns.
//
// Where W_hh lives: in registers, across the workgroup. At H = 128 the matrix is 256 KiB, more
// than a CU's 160 KiB of LDS, but 512 threads x 128 registers hold it exactly (8 waves, two per
// SIMD, each within the 256-register budget of that occupancy). It is read from L2 once per
// workgroup, not once per step. Forward: thread j holds ROW j (gate column j of h W_hh^T); the
// masked state h_in sits in LDS and every lane reads the same 16 bytes as one broadcast.
// Backward: thread (q, k) = q * H + k holds the H entries W_hh[q * H .. q * H + H - 1][k] of
// COLUMN k; it sums its quarter of dh_in[k] = sum_j dgates[j] W_hh[j][k] from the dgates in LDS,
// and the four quarters are combined as (q0 + q1) + (q2 + q3).
//
// Summation order: every dot product of these kernels is four interleaved FMA chains over the
// reduction index (element e goes to chain e mod 4, ascending), combined (0 + 1) + (2 + 3). The
// order depends on H alone -- not on B, T, the workgroup or the launch -- so an environment's
// results are the same bits alone and as any row of any batch, and two runs agree bitwise.
//
// The step kernel (rollout, no saved tensors) has both products to do, so weights stream: its
// body is ocppo_lstm_step.h's lstm_step_rows, shared with ocppo_pqn_lstm_act.
#include <math.h>

#include "ocppo_common.h"
#include "ocppo_lstm_step.h"

namespace ocppo {

// sum_e a[e] * v[e], v in LDS (16-B aligned, the same address in every lane: a broadcast)
template <int H>
__device__ __forceinline__ float dot_lds(const float (&a)[H], const float* v) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int e = 0; e < H / 4; ++e) {
    const float4 r = *reinterpret_cast<const float4*>(v + 4 * e);
    s0 = fmaf(a[4 * e + 0], r.x, s0);
    s1 = fmaf(a[4 * e + 1], r.y, s1);
    s2 = fmaf(a[4 * e + 2], r.z, s2);
    s3 = fmaf(a[4 * e + 3], r.w, s3);
  }
  return (s0 + s1) + (s2 + s3);
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_seq_fwd_kernel(
    const float* __restrict__ pre, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ done, const float* __restrict__ h0, const float* __restrict__ c0,
    int64_t T, int64_t B, float* __restrict__ h_out, float* __restrict__ c_out,
    float* __restrict__ gates, float* __restrict__ h_in, float* __restrict__ hT,
    float* __restrict__ cT) {
  constexpr int G = 4 * H;
  __shared__ __align__(16) float s_h[H];
  __shared__ float s_g[G];
  const int j = threadIdx.x;
  const int64_t b = blockIdx.x;
  float w[H];
#pragma unroll
  for (int e = 0; e < H / 4; ++e) {
    const float4 r = *reinterpret_cast<const float4*>(w_hh + static_cast<int64_t>(j) * H + 4 * e);
    w[4 * e + 0] = r.x; w[4 * e + 1] = r.y; w[4 * e + 2] = r.z; w[4 * e + 3] = r.w;
  }
  const float bj = b_hh[j];
  const bool unit = j < H;  // threads 0..H-1 also own hidden unit j's state
  float h = 0.f, c = 0.f;
  if (unit) {
    h = h0[b * H + j];
    c = c0[b * H + j];
  }
  float pre_n = pre[b * G + j];
  float d_n = done[b];
  for (int64_t t = 0; t < T; ++t) {
    const int64_t row = t * B + b;
    const float pre_t = pre_n;
    const float m = 1.f - d_n;
    if (t + 1 < T) {  // next step's operands: in flight while this step computes
      pre_n = pre[(row + B) * G + j];
      d_n = done[row + B];
    }
    float c_in = 0.f;
    if (unit) {
      const float hm = m * h;
      c_in = m * c;
      s_h[j] = hm;
      if (h_in != nullptr) h_in[row * H + j] = hm;
    }
    __syncthreads();
    const float z = (pre_t + dot_lds<H>(w, s_h)) + bj;
    const float a = (j / H == 2) ? tanhf(z) : sigmoid_f(z);
    s_g[j] = a;
    if (gates != nullptr) gates[row * G + j] = a;
    __syncthreads();
    if (unit) {
      const float gi = s_g[j], gf = s_g[H + j], gg = s_g[2 * H + j], go = s_g[3 * H + j];
      c = gf * c_in + gi * gg;
      h = go * tanhf(c);
      h_out[row * H + j] = h;
      if (c_out != nullptr) c_out[row * H + j] = c;
    }
  }
  if (unit) {
    hT[b * H + j] = h;
    cT[b * H + j] = c;
  }
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_seq_bwd_kernel(
    const float* __restrict__ dh_out, const float* __restrict__ gates,
    const float* __restrict__ c_out, const float* __restrict__ c0, const float* __restrict__ done,
    const float* __restrict__ w_hh, int64_t T, int64_t B, float* __restrict__ dgates) {
  constexpr int G = 4 * H;
  __shared__ __align__(16) float s_dg[G];
  __shared__ float s_part[G];
  const int tid = threadIdx.x;
  const int q = tid / H, k = tid % H;
  const int64_t b = blockIdx.x;
  float w[H];  // W_hh[q * H + e][k]: consecutive k in consecutive lanes
#pragma unroll
  for (int e = 0; e < H; ++e) w[e] = w_hh[(static_cast<int64_t>(q) * H + e) * H + k];
  const bool unit = tid < H;
  float dh_c = 0.f, dc_c = 0.f;  // what steps t+1.. send back to step t's h and c
  // step t's operands, loaded one step ahead
  float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f, ct = 0.f, dh_o = 0.f, d_t = 0.f;
  if (unit) {
    const int64_t row = (T - 1) * B + b;
    gi = gates[row * G + tid]; gf = gates[row * G + H + tid];
    gg = gates[row * G + 2 * H + tid]; go = gates[row * G + 3 * H + tid];
    ct = c_out[row * H + tid];
    dh_o = dh_out[row * H + tid];
    d_t = done[row];
  }
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t row = t * B + b;
    float m = 0.f;
    if (unit) {
      const float i_ = gi, f_ = gf, g_ = gg, o_ = go, c_t = ct, dho = dh_o;
      m = 1.f - d_t;
      const float c_prev = t > 0 ? c_out[(row - B) * H + tid] : c0[b * H + tid];
      if (t > 0) {
        const int64_t r1 = row - B;
        gi = gates[r1 * G + tid]; gf = gates[r1 * G + H + tid];
        gg = gates[r1 * G + 2 * H + tid]; go = gates[r1 * G + 3 * H + tid];
        dh_o = dh_out[r1 * H + tid];
        d_t = done[r1];
        ct = c_prev;
      }
      const float c_in = m * c_prev;
      const float dh = dho + dh_c;
      const float tc = tanhf(c_t);
      const float d_o = dh * tc;
      const float dc = dc_c + (dh * o_) * (1.f - tc * tc);
      const float dzi = (dc * g_) * (i_ * (1.f - i_));
      const float dzf = (dc * c_in) * (f_ * (1.f - f_));
      const float dzg = (dc * i_) * (1.f - g_ * g_);
      const float dzo = d_o * (o_ * (1.f - o_));
      s_dg[tid] = dzi; s_dg[H + tid] = dzf; s_dg[2 * H + tid] = dzg; s_dg[3 * H + tid] = dzo;
      dgates[row * G + tid] = dzi; dgates[row * G + H + tid] = dzf;
      dgates[row * G + 2 * H + tid] = dzg; dgates[row * G + 3 * H + tid] = dzo;
      dc_c = (dc * f_) * m;
    }
    __syncthreads();
    s_part[tid] = dot_lds<H>(w, s_dg + q * H);
    __syncthreads();
    if (unit)
      dh_c = ((s_part[tid] + s_part[H + tid]) + (s_part[2 * H + tid] + s_part[3 * H + tid])) * m;
  }
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_step_kernel(
    const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ done, int64_t N, int64_t I, float* __restrict__ h,
    float* __restrict__ c) {
  __shared__ float s_x[kStepEnvs][kStepChunk];
  __shared__ float s_g[kStepEnvs][4 * H];
  lstm_step_rows<H, false>(x, w_ih, b_ih, w_hh, b_hh, done, N, I, h, c, true,
                           static_cast<int64_t>(blockIdx.x) * kStepEnvs, s_x, s_g);
}

inline bool lstm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_lstm_seq_fwd(ocppo_stream_t stream, const float* pre, const float* w_hh,
                                  const float* b_hh, const float* done, const float* h0,
                                  const float* c0, int64_t T, int64_t B, int64_t H, float* h_out,
                                  float* c_out, float* gates, float* h_in, float* hT, float* cT) {
  const char* who = "ocppo_lstm_seq_fwd";
  if (int rc = lstm_check(who, T, B, H)) return rc;
  if (T == 0 || B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(pre && w_hh && b_hh && done && h0 && c0 && h_out && hT && cT, "%s: null pointer",
                who);
  OCPPO_REQUIRE(lstm_aligned16(w_hh), "%s: w_hh not 16-B aligned", who);
  clear_stale_error();
  OCPPO_LSTM_DISPATCH(H, hipLaunchKernelGGL(lstm_seq_fwd_kernel<HH>,
                                            dim3(static_cast<unsigned>(B)), dim3(4 * HH), 0,
                                            as_stream(stream), pre, w_hh, b_hh, done, h0, c0, T,
                                            B, h_out, c_out, gates, h_in, hT, cT));
  return check_launch(who);
}

extern "C" int ocppo_lstm_seq_bwd(ocppo_stream_t stream, const float* dh_out, const float* gates,
                                  const float* c_out, const float* c0, const float* done,
                                  const float* w_hh, int64_t T, int64_t B, int64_t H,
                                  float* dgates) {
  const char* who = "ocppo_lstm_seq_bwd";
  if (int rc = lstm_check(who, T, B, H)) return rc;
  if (T == 0 || B == 0) return OCPPO_OK;
  OCPPO_REQUIRE(dh_out && gates && c_out && c0 && done && w_hh && dgates, "%s: null pointer",
                who);
  clear_stale_error();
  OCPPO_LSTM_DISPATCH(H, hipLaunchKernelGGL(lstm_seq_bwd_kernel<HH>,
                                            dim3(static_cast<unsigned>(B)), dim3(4 * HH), 0,
                                            as_stream(stream), dh_out, gates, c_out, c0, done,
                                            w_hh, T, B, dgates));
  return check_launch(who);
}

extern "C" int ocppo_lstm_step(ocppo_stream_t stream, const float* x, const float* w_ih,
                               const float* b_ih, const float* w_hh, const float* b_hh,
                               const float* done, int64_t N, int64_t I, int64_t H, float* h,
                               float* c) {
  const char* who = "ocppo_lstm_step";
  if (int rc = lstm_check(who, 1, N, H)) return rc;
  OCPPO_REQUIRE(I >= 0, "%s: negative size I=%lld", who, (long long)I);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(I >= 1, "%s: I = 0 with N = %lld rows", who, (long long)N);
  OCPPO_REQUIRE(x && w_ih && b_ih && w_hh && b_hh && done && h && c, "%s: null pointer", who);
  const unsigned grid = static_cast<unsigned>(ceil_div(N, kStepEnvs));
  clear_stale_error();
  OCPPO_LSTM_DISPATCH(H, hipLaunchKernelGGL(lstm_step_kernel<HH>, dim3(grid), dim3(4 * HH), 0,
                                            as_stream(stream), x, w_ih, b_ih, w_hh, b_hh, done,
                                            N, I, h, c));
  return check_launch(who);
}
