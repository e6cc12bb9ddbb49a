// The recurrent PQN learner (cleanrl/pqn_atari_envpool_lstm.py): the two places where the LSTM
// and the Q head meet, each as one call. f32 tensors, wave64, no atomics, no waiting between
// workgroups: every sum runs in an order fixed by the shapes alone.
//
// ocppo_pqn_lstm_act -- the rollout step (:261-267) in one launch. A workgroup of 4H threads owns
// kStepEnvs environments: it runs ocppo_lstm_step's body (ocppo_lstm_step.h: lstm_step_rows) with
// the new h rows left in LDS, then its waves run ocppo_pqn_act's body (ocppo_pqn_act.h:
// pqn_act_row) on those rows, one wave per environment. Nothing of either kernel's arithmetic is
// restated here, so h / c are ocppo_lstm_step's bits and q / values / actions ocppo_pqn_act's.
// commit = 0 skips the stores of h / c: the bootstrap of :287, whose state is dropped.
//
// ocppo_pqn_head_loss_fwd_bwd -- the update's Q head, MSE loss on the taken action and the head's
// backward (:318-325). Only the taken column carries gradient, so a row costs ONE dot product.
// Launch 1, grid (ceil(M / kHlRows), ceil(H / kHlCols)): a wave per row computes
// q_a = h[m] . wq[a_m] + bq[a_m] (float4 chunks lane, lane + 64, ..., the lanes' butterfly) and
// g_m, and writes its column tile of dh[m] = g_m * wq[a_m]; then thread k of the workgroup owns
// column k of its tile and adds g_m * h[m][k] into its private LDS cell [a_m][k], rows ascending.
// The workgroup's [A, tile] sums, its per-action sums of g and its sums of (G - q_a)^2 and q_a go
// to the workspace with plain stores. Launch 2 sums the workgroups' partials in workgroup order.
// Rows of dwq / dbq of actions nobody took are sums of +0: exact zeros.
// Precision: inputs and outputs are f32; every SUM of this call (the dot product over H, the sums
// over the rows, the workgroups' partials) is accumulated in f64 from exact f32 x f32 products and
// rounded to f32 once (as ocppo_ppg_aux_loss_fwd_bwd's row sums are), so q_a, stats, dwq and dbq
// are the nearest f32 to the exact result in all but double-rounding cases. dh's factor g_m is
// ocppo_pqn_loss_fwd_bwd's f32 arithmetic on that q_a, so dh[m] == g_m * wq[a_m] holds in f32.
#include "ocppo_common.h"
#include "ocppo_lstm_step.h"
#include "ocppo_pqn_act.h"
#include "ocppo_rng.h"

namespace ocppo {

template <int H>
__global__ __launch_bounds__(4 * H) void pqn_lstm_act_kernel(
    const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    const float* __restrict__ done, int64_t N, int64_t I, float* h, float* c, int commit,
    const float* __restrict__ wq, const float* __restrict__ bq, int A, uint64_t seed,
    const int64_t* __restrict__ step, int64_t step_offset, double start_e, double end_e,
    double duration, int64_t* __restrict__ actions, float* __restrict__ values,
    float* __restrict__ eps_out, float* __restrict__ q_out) {
  __shared__ __align__(16) float s_x[kStepEnvs][kStepChunk];
  __shared__ float s_g[kStepEnvs][4 * H];
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kStepEnvs;
  lstm_step_rows<H, true>(x, w_ih, b_ih, w_hh, b_hh, done, N, I, h, c, commit != 0, n0, s_x, s_g);
  __syncthreads();  // the new h rows are in s_x[r][0 .. H)
  constexpr int kWaves = 4 * H / kWave;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const EpsGreedy eg(seed, step[0] + step_offset, start_e, end_e, duration);
  for (int r = wv; r < kStepEnvs; r += kWaves) {  // wave-uniform
    const int64_t n = n0 + r;
    if (n < N) pqn_act_row(s_x[r], n, H, wq, bq, A, eg, lane, actions, values, eps_out, q_out);
  }
}

// ---- Q head + MSE on the taken action + head backward -------------------------------------------
constexpr int kHlRows = 32;    // rows per workgroup: the grid depends on M (and H) only
constexpr int kHlCols = 256;   // columns per workgroup = threads
constexpr int kHlMaxH = 1024;

struct HeadLossWs {
  double* part_dw;  // [nb, A, H]
  double* part_db;  // [nb, A]
  double* part_st;  // [nb, 2]
  float* qa;        // [M] q_a per row (left there for the caller): the workspace's first floats
};

inline int64_t hl_blocks(int64_t M) { return ceil_div(M, kHlRows); }
inline int64_t hl_qa_floats(int64_t M) { return ceil_div(M, 4) * 4; }
inline size_t hl_workspace_bytes(int64_t M, int64_t H, int64_t A) {
  const int64_t bytes = hl_qa_floats(M) * 4 + hl_blocks(M) * (A * H + A + 2) * 8;
  return static_cast<size_t>(ceil_div(bytes, 16) * 16);
}
inline HeadLossWs hl_carve(void* ws, int64_t M, int64_t H, int64_t A) {
  HeadLossWs w;
  const int64_t nb = hl_blocks(M);
  w.qa = static_cast<float*>(ws);
  w.part_dw = reinterpret_cast<double*>(w.qa + hl_qa_floats(M));  // 16-B aligned
  w.part_db = w.part_dw + nb * A * H;
  w.part_st = w.part_db + nb * A;
  return w;
}

__global__ __launch_bounds__(kHlCols) void pqn_head_loss_rows_kernel(
    const float* __restrict__ h, const float* __restrict__ wq, const float* __restrict__ bq,
    const int64_t* __restrict__ actions, const float* __restrict__ returns, int64_t M, int H,
    int A, float norm, double norm64, float* __restrict__ dh, HeadLossWs ws) {
  __shared__ double s_g64[kHlRows], s_q[kHlRows], s_se[kHlRows];
  __shared__ int s_a[kHlRows];
  __shared__ double s_dw[kPqnMaxA][kHlCols];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int64_t bx = blockIdx.x, m0 = bx * kHlRows;
  const int by = blockIdx.y;
  const int rows = static_cast<int>(M - m0 < kHlRows ? M - m0 : kHlRows);
  const int H4 = H / 4;
  for (int a = 0; a < A; ++a) s_dw[a][tid] = 0.0;  // this thread's own cells
  for (int r = wv; r < rows; r += kHlCols / kWave) {  // wave-uniform
    const int64_t m = m0 + r;
    int64_t a64 = actions[m];
    a64 = a64 < 0 ? 0 : (a64 >= A ? A - 1 : a64);
    const int a = static_cast<int>(a64);
    const float4* __restrict__ hrow = reinterpret_cast<const float4*>(h + m * H);
    const float4* __restrict__ wrow = reinterpret_cast<const float4*>(wq + static_cast<int64_t>(a) * H);
    double acc = 0.0;  // exact products of f32 pairs, summed in f64
    for (int i = lane; i < H4; i += kWave) {
      const float4 xv = hrow[i], w = wrow[i];
      acc += static_cast<double>(xv.x) * w.x + static_cast<double>(xv.y) * w.y +
             static_cast<double>(xv.z) * w.z + static_cast<double>(xv.w) * w.w;
    }
    const double q64 = wave_sum(acc) + static_cast<double>(bq[a]);
    const float q = static_cast<float>(q64);  // q_a: the f64 sum rounded once
    const float ret = returns[m];
    const double diff = static_cast<double>(ret) - q64;
    const float gm = (q - ret) * norm;  // ocppo_pqn_loss_fwd_bwd's f32 ops on q_a: dh's factor
    const int i = by * (kHlCols / 4) + lane;  // this workgroup's column tile of dh
    if (i < H4) {
      const float4 w = wrow[i];
      reinterpret_cast<float4*>(dh + m * H)[i] = make_float4(gm * w.x, gm * w.y, gm * w.z, gm * w.w);
    }
    if (lane == 0) {
      s_g64[r] = (q64 - ret) * norm64;  // the weight and bias sums' factor
      s_a[r] = a;
      s_q[r] = q64;
      s_se[r] = diff * diff;
      if (by == 0) ws.qa[m] = q;
    }
  }
  __syncthreads();
  const int k = by * kHlCols + tid;
  if (k < H) {
    for (int r = 0; r < rows; ++r) s_dw[s_a[r]][tid] += s_g64[r] * h[(m0 + r) * H + k];
    for (int a = 0; a < A; ++a) ws.part_dw[(bx * A + a) * H + k] = s_dw[a][tid];
  }
  if (by != 0) return;
  if (tid < A) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r)
      if (s_a[r] == tid) s += s_g64[r];
    ws.part_db[bx * A + tid] = s;
  } else if (tid == kWave) {
    double se = 0.0, sq = 0.0;
    for (int r = 0; r < rows; ++r) {
      se += s_se[r];
      sq += s_q[r];
    }
    ws.part_st[bx * 2] = se;
    ws.part_st[bx * 2 + 1] = sq;
  }
}

__global__ __launch_bounds__(256) void pqn_head_loss_finish_kernel(
    HeadLossWs ws, int64_t nb, int64_t M, int H, int A, float* __restrict__ dwq,
    float* __restrict__ dbq, float* __restrict__ stats) {
  const int64_t AH = static_cast<int64_t>(A) * H;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= AH + A + 2) return;
  const double* __restrict__ p;
  int64_t stride;
  if (e < AH) {
    p = ws.part_dw + e;
    stride = AH;
  } else if (e < AH + A) {
    p = ws.part_db + (e - AH);
    stride = A;
  } else {
    p = ws.part_st + (e - AH - A);
    stride = 2;
  }
  double s = 0.0;
  for (int64_t b = 0; b < nb; ++b) s += p[b * stride];
  if (e < AH) {
    dwq[e] = static_cast<float>(s);
  } else if (e < AH + A) {
    dbq[e - AH] = static_cast<float>(s);
  } else {
    stats[e - AH - A] = static_cast<float>(s / static_cast<double>(M));  // td_loss, mean q_a
  }
}

inline bool pl_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ocppo

using namespace ocppo;

extern "C" int ocppo_pqn_lstm_act(ocppo_stream_t stream, const float* x, const float* w_ih,
                                  const float* b_ih, const float* w_hh, const float* b_hh,
                                  const float* done, int64_t N, int64_t I, int64_t H, float* h,
                                  float* c, int commit, const float* wq, const float* bq,
                                  int64_t A, uint64_t seed, const int64_t* step,
                                  int64_t step_offset, double start_e, double end_e,
                                  double duration, int64_t* actions, float* values,
                                  float* epsilon_out, float* q_out) {
  const char* who = "ocppo_pqn_lstm_act";
  if (int rc = lstm_check(who, 1, N, H)) return rc;
  OCPPO_REQUIRE(I >= 0 && A >= 1 && A <= kPqnMaxA && duration > 0,
                "%s: bad sizes I=%lld A=%lld (I >= 0, 1 <= A <= %d, duration > 0)", who,
                (long long)I, (long long)A, kPqnMaxA);
  if (N == 0) return OCPPO_OK;
  OCPPO_REQUIRE(I >= 1, "%s: I = 0 with N = %lld rows", who, (long long)N);
  OCPPO_REQUIRE(x && w_ih && b_ih && w_hh && b_hh && done && h && c && wq && bq && step && values &&
                    (actions || !commit),
                "%s: null pointer", who);
  OCPPO_REQUIRE(pl_aligned16(wq), "%s: wq must be 16-B aligned", who);
  const unsigned grid = static_cast<unsigned>(ceil_div(N, kStepEnvs));
  clear_stale_error();
  OCPPO_LSTM_DISPATCH(H, hipLaunchKernelGGL(pqn_lstm_act_kernel<HH>, dim3(grid), dim3(4 * HH), 0,
                                            as_stream(stream), x, w_ih, b_ih, w_hh, b_hh, done, N,
                                            I, h, c, commit, wq, bq, (int)A, seed, step,
                                            step_offset, start_e, end_e, duration, actions,
                                            values, epsilon_out, q_out));
  return check_launch(who);
}

static int hl_check(const char* who, int64_t M, int64_t H, int64_t A) {
  OCPPO_REQUIRE(M >= 0 && M <= INT32_MAX && A >= 1 && A <= kPqnMaxA && H >= 4 && H % 4 == 0 &&
                    H <= kHlMaxH,
                "%s: bad sizes M=%lld H=%lld A=%lld (M >= 0, 1 <= A <= %d, H a multiple of 4 in "
                "[4, %d])", who, (long long)M, (long long)H, (long long)A, kPqnMaxA, kHlMaxH);
  return OCPPO_OK;
}

extern "C" size_t ocppo_pqn_head_loss_workspace_bytes(int64_t M, int64_t H, int64_t A) {
  if (M < 0 || M > INT32_MAX || A < 1 || A > kPqnMaxA || H < 4 || H % 4 || H > kHlMaxH) return 0;
  return hl_workspace_bytes(M, H, A);
}

extern "C" int ocppo_pqn_head_loss_fwd_bwd(ocppo_stream_t stream, const float* h, const float* wq,
                                           const float* bq, const int64_t* actions,
                                           const float* returns, int64_t M, int64_t H, int64_t A,
                                           float* dh, float* dwq, float* dbq, float* stats,
                                           void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_pqn_head_loss_fwd_bwd";
  if (int rc = hl_check(who, M, H, A)) return rc;
  if (M == 0) return OCPPO_OK;
  OCPPO_REQUIRE(h && wq && bq && actions && returns && dh && dwq && dbq && stats,
                "%s: null pointer", who);
  OCPPO_REQUIRE(pl_aligned16(h) && pl_aligned16(wq) && pl_aligned16(dh),
                "%s: h, wq and dh must be 16-B aligned", who);
  if (!workspace || !pl_aligned16(workspace) || workspace_bytes < hl_workspace_bytes(M, H, A))
    return fail(OCPPO_E_WORKSPACE, "%s: workspace of %zu bytes, need %zu (16-B aligned)", who,
                workspace_bytes, hl_workspace_bytes(M, H, A));
  const HeadLossWs ws = hl_carve(workspace, M, H, A);
  const int64_t nb = hl_blocks(M);
  // mse_loss backward: norm = 2 / numel (computed in double by ATen, applied in f32)
  const float norm = static_cast<float>(2.0 / static_cast<double>(M));
  clear_stale_error();
  hipLaunchKernelGGL(pqn_head_loss_rows_kernel,
                     dim3(static_cast<unsigned>(nb), static_cast<unsigned>(ceil_div(H, kHlCols))),
                     dim3(kHlCols), 0, as_stream(stream), h, wq, bq, actions, returns, M, (int)H,
                     (int)A, norm, 2.0 / static_cast<double>(M), dh, ws);
  if (int rc = check_launch(who)) return rc;
  hipLaunchKernelGGL(pqn_head_loss_finish_kernel,
                     dim3(static_cast<unsigned>(ceil_div(A * H + A + 2, 256))), dim3(256), 0,
                     as_stream(stream), ws, nb, M, (int)H, (int)A, dwq, dbq, stats);
  return check_launch("ocppo_pqn_head_loss_fwd_bwd (finish)");
}
