// Gradient-norm clipping + Adam over ONE flat parameter / gradient / moment buffer
// (replaces `nn.utils.clip_grad_norm_(agent.parameters(), max_grad_norm); optimizer.step()` of
// cleanrl/ppo_atari_oc.py:608-610 with torch.optim.Adam(eps=1e-5), and the `/ world_size` of the
// DP all-reduce, ppo_atari_multigpu.py:369-374).
//
//   norm kernel : grid-strided partial sums of (g * grad_scale)^2 per workgroup (16-B loads),
//                 one plain store per workgroup; workgroup 0 also advances the step counter
//                 (the only writer of it; the step kernel, next on the stream, only reads it)
//   step kernel : every workgroup first combines the <= 1024 partials itself, in a fixed order
//                 (the same fixed-order sum in every workgroup, so every one derives the same
//                 total_norm, clip = min(max_norm / (total_norm + 1e-6), 1), step_size =
//                 lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)), then
//                 g = (g * grad_scale) * clip;  m = beta1*m + (1-beta1)*g;
//                 v = beta2*v + (1-beta2)*g*g;  p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
//                 (the formula of ATen's fused Adam), 16-B vectors, 28 B of HBM per parameter.
// No ticket and no last-arriver hand-off: the kernel boundary orders the partials (round 3's
// ticketed form spent ~7 us of its 11 per minibatch in the 256-way fan-in and the dependent
// combine at config 2).
//
// The same two launches serve ocppo_clip_adam_step_exact (torch.optim.Adam's scalars, from
// doubles) and ocppo_clip_radam_step (torch.optim.RAdam): one norm kernel, one step kernel
// (flat_step_kernel) instantiated with the rule that supplies the step scalars and the
// per-element update, one host helper (flat_step) behind the three entries.
// ocppo_clip_adam_step_seg (a head and a tail segment with a step count each, the tail optional
// per step) runs the same norm kernel over the active length and flat_step_seg_kernel, the same
// loop with the rule's scalars taken once per segment.
#include "ocppo_common.h"
#include "ocppo_x6split.h"

namespace ocppo {

// Weight planes written by the step (ocppo_clip_adam_step's plane jobs): the new values of a
// row-major [R, C] weight at flat offset off (float4 units) as the three exact bf16 pieces
// ocppo_split_planes writes for it -- plane p at dst + p R C (bf16 units), [R, C] or, trans,
// [C, R] -- so the next minibatch's GEMMs read them without a split launch
constexpr int kAdamPlaneJobs = 8;
struct AdamPlanes {
  int n;
  int64_t off4[kAdamPlaneJobs];
  int64_t len4[kAdamPlaneJobs];
  int rows[kAdamPlaneJobs];
  int cols[kAdamPlaneJobs];
  int trans[kAdamPlaneJobs];
  uint16_t* dst[kAdamPlaneJobs];
};

__device__ __forceinline__ void adam_planes_store(const AdamPlanes& pl, int64_t i, float4 v) {
  for (int j = 0; j < pl.n; ++j) {
    const int64_t q = i - pl.off4[j];
    if (q >= 0 && q < pl.len4[j]) {
      uint32_t a0, a1, a2, b0, b1, b2;
      x6_split2(x6f2{v.x, v.y}, a0, a1, a2);
      x6_split2(x6f2{v.z, v.w}, b0, b1, b2);
      const int64_t ps = 4 * pl.len4[j];  // elements per plane
      if (!pl.trans[j]) {
        uint2* d = reinterpret_cast<uint2*>(pl.dst[j]);
        d[q] = uint2{a0, b0};
        d[ps / 4 + q] = uint2{a1, b1};
        d[ps / 2 + q] = uint2{a2, b2};
      } else {  // element (r, c .. c + 3) -> plane rows c .. c + 3, column r
        const int64_t e = 4 * q;
        const int64_t r = e / pl.cols[j], c = e - r * pl.cols[j];
        const int64_t R = pl.rows[j];
        uint16_t* d = pl.dst[j] + c * R + r;
        const uint32_t w[3][2] = {{a0, b0}, {a1, b1}, {a2, b2}};
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          uint16_t* dp = d + p * ps;
          dp[0] = static_cast<uint16_t>(w[p][0]);
          dp[R] = static_cast<uint16_t>(w[p][0] >> 16);
          dp[2 * R] = static_cast<uint16_t>(w[p][1]);
          dp[3 * R] = static_cast<uint16_t>(w[p][1] >> 16);
        }
      }
      return;
    }
  }
}

constexpr int kOptThreads = 256;
constexpr int kOptBlocks = 1024;  // grid-stride cap for the norm pass (4 workgroups per CU), at
                                  // most 1024 partials for every adam workgroup to combine

// scalars layout (f32): see include/ocppo.h OCPPO_OPT_*
enum { S_STEP = 0, S_TOTAL_NORM = 1, S_CLIP = 2, S_STEP_SIZE = 3, S_BC2_SQRT = 4, S_RECT = 5 };

__global__ __launch_bounds__(kOptThreads) void grad_norm_kernel(
    const float* __restrict__ g, int64_t P, float grad_scale, float* __restrict__ scalars,
    float* __restrict__ partials) {
  __shared__ float red[kOptThreads / kWave];
  float acc = 0.f;
  const int64_t P4 = P / 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kOptThreads;
  // kNormU grid-strided float4 loads in flight per thread, then accumulated in index order
  constexpr int kNormU = 4;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kOptThreads + threadIdx.x; i0 < P4;
       i0 += kNormU * stride) {
    float4 x[kNormU];
#pragma unroll
    for (int u = 0; u < kNormU; ++u) {
      const int64_t i = i0 + u * stride;
      x[u] = i < P4 ? reinterpret_cast<const float4*>(g)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kNormU; ++u) {
      const float a = x[u].x * grad_scale, b = x[u].y * grad_scale, c = x[u].z * grad_scale,
                  d = x[u].w * grad_scale;
      acc += a * a + b * b + c * c + d * d;
    }
  }
  if (blockIdx.x == 0)
    for (int64_t i = 4 * P4 + threadIdx.x; i < P; i += kOptThreads) {
      const float a = g[i] * grad_scale;
      acc += a * a;
    }
  const float w = wave_sum(acc);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) red[wid] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = red[0];
    for (int k = 1; k < kOptThreads / kWave; ++k) s += red[k];
    partials[blockIdx.x] = s;
    if (blockIdx.x == 0) scalars[S_STEP] = scalars[S_STEP] + 1.f;
  }
}

// The norm kernel's partials -> total_norm and the clip coefficient, in every workgroup alike
// (fixed order: the partials t, t + 256, ... in thread t, the wave sums, then the 4 waves in order
// by thread 0, the only thread whose return value is meaningful)
struct NormClip {
  float total, clip;
};
__device__ __forceinline__ NormClip norm_clip(const float* __restrict__ partials, int nb,
                                              float max_norm) {
  __shared__ float red[kOptThreads / kWave];
  float t = 0.f;
  for (int b = threadIdx.x; b < nb; b += kOptThreads) t += partials[b];
  const float tw = wave_sum(t);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  if (lane == 0) red[wid] = tw;
  __syncthreads();
  NormClip nc{0.f, 1.f};
  if (threadIdx.x == 0) {
    float s = red[0];
    for (int k = 1; k < kOptThreads / kWave; ++k) s += red[k];
    nc.total = sqrtf(s);
    if (max_norm > 0.f) {
      nc.clip = max_norm / (nc.total + 1e-6f);
      nc.clip = nc.clip < 1.f ? nc.clip : 1.f;
    }
  }
  return nc;
}

// ---- the three update rules -----------------------------------------------------------------------
// A rule is what flat_step_kernel does not share: Scalars (what an element's update needs beside
// the element; thread 0 of every workgroup builds them once from the clip, the device step count
// t, lr and the betas), report (its figures in `scalars`) and elem (one element, g already scaled
// and clipped). kPlanes: the step also serves AdamPlanes jobs; kMaxBlocks: the step's grid cap.

// ATen's fused Adam with every scalar formed in f32 (the PPO learners' step; plane jobs)
struct AdamRule {
  static constexpr int kMaxBlocks = 256 * 8;
  static constexpr bool kPlanes = true;
  struct Scalars {
    float clip, b1, b2, step_size, bc2_sqrt;
  };
  static __device__ Scalars scalars(NormClip nc, float step, float lr, double b1d, double b2d) {
    const float b1 = static_cast<float>(b1d), b2 = static_cast<float>(b2d);
    return Scalars{nc.clip, b1, b2, lr / (1.f - powf(b1, step)), sqrtf(1.f - powf(b2, step))};
  }
  static __device__ void report(const Scalars& sc, float* __restrict__ scalars) {
    scalars[S_STEP_SIZE] = sc.step_size;
    scalars[S_BC2_SQRT] = sc.bc2_sqrt;
  }
  static __device__ __forceinline__ void elem(float& p, float g, float& m, float& v,
                                              const Scalars& sc, float eps) {
    m = sc.b1 * m + (1.f - sc.b1) * g;
    v = sc.b2 * v + (1.f - sc.b2) * g * g;
    const float denom = sqrtf(v) / sc.bc2_sqrt + eps;
    p = p - sc.step_size * m / denom;
  }
};

// torch.optim.Adam with torch's scalars (the discrete SAC learner's optimizers). AdamRule forms
// 1 - beta^t, 1 - beta1 and 1 - beta2 in f32: one rounding of 1 - 0.9^t is up to 6e-7 of the step
// size and 1 - 0.999f is 1.3e-5 off 0.001, which a parameter that starts at zero (a bias) shows
// whole. torch takes them from Python doubles: step_size = lr / (1 - beta1^t), bc2_sqrt =
// sqrt(1 - beta2^t), the lerp weight 1 - beta1 and addcmul's 1 - beta2, each rounded to f32 once.
struct AdamExactRule {
  static constexpr int kMaxBlocks = 256 * 8;
  static constexpr bool kPlanes = false;
  struct Scalars {
    float clip, omb1, omb2, b2, step_size, bc2_sqrt;
  };
  static __device__ Scalars scalars(NormClip nc, float stepf, float lr, double b1, double b2) {
    const double step = static_cast<double>(stepf);
    return Scalars{nc.clip,
                   static_cast<float>(1.0 - b1),
                   static_cast<float>(1.0 - b2),
                   static_cast<float>(b2),
                   static_cast<float>(static_cast<double>(lr) / (1.0 - pow(b1, step))),
                   static_cast<float>(sqrt(1.0 - pow(b2, step)))};
  }
  static __device__ void report(const Scalars& sc, float* __restrict__ scalars) {
    scalars[S_STEP_SIZE] = sc.step_size;
    scalars[S_BC2_SQRT] = sc.bc2_sqrt;
  }
  static __device__ __forceinline__ void elem(float& p, float g, float& m, float& v,
                                              const Scalars& sc, float eps) {
    m = m + sc.omb1 * (g - m);          // exp_avg.lerp_(grad, 1 - beta1)
    v = v * sc.b2 + (sc.omb2 * g) * g;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / sc.bc2_sqrt + eps;
    p = p + ((-sc.step_size) * m) / denom;  // param.addcdiv_(exp_avg, denom, value=-step_size)
  }
};

// torch.optim.RAdam, no weight decay: `optim.RAdam(q_network.parameters(), lr)` after
// `clip_grad_norm_(.., 10.0)` of cleanrl/pqn_atari_envpool.py:194, 282-283. From the device step
// count t, in double as torch's Python scalars are:
//   bc1 = 1 - b1^t, bc2 = 1 - b2^t, rho_inf = 2 / (1 - b2) - 1, rho_t = rho_inf - 2 t b2^t / bc2
//   rho_t > 5 : rect = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
//               p -= (m / bc1) * lr * (sqrt(bc2) / (sqrt(v) + eps)) * rect
//   else      : p -= (m / bc1) * lr
// with m += (1 - b1) (g - m), v = b2 v + (1 - b2) g g per element, 1 - beta taken in double and
// rounded once (1.f - 0.999f is 1.3e-5 off 0.001).
struct RAdamRule {
  // every workgroup resident at once: the double-precision scalars are paid once, not per round
  static constexpr int kMaxBlocks = kOptBlocks;
  static constexpr bool kPlanes = false;
  struct Scalars {
    float clip, bc1, lr, adapt, rect, omb1, omb2, b2;  // adapt = sqrt(bc2); rect = 0: un-rectified
  };
  static __device__ Scalars scalars(NormClip nc, float stepf, float lr, double b1, double b2) {
    const double step = static_cast<double>(stepf);
    const double b2t = pow(b2, step);
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - b2t;
    const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
    const double rho_t = rho_inf - 2.0 * step * b2t / bc2;
    double rect = 0.0;
    if (rho_t > 5.0)
      rect = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf /
                  ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
    return Scalars{nc.clip, static_cast<float>(bc1), lr, static_cast<float>(sqrt(bc2)),
                   static_cast<float>(rect), static_cast<float>(1.0 - b1),
                   static_cast<float>(1.0 - b2), static_cast<float>(b2)};
  }
  static __device__ void report(const Scalars& sc, float* __restrict__ scalars) {
    scalars[S_STEP_SIZE] = sc.lr / sc.bc1;
    scalars[S_BC2_SQRT] = sc.adapt;
    scalars[S_RECT] = sc.rect;
  }
  static __device__ __forceinline__ void elem(float& p, float g, float& m, float& v,
                                              const Scalars& sc, float eps) {
    m = m + sc.omb1 * (g - m);
    v = sc.b2 * v + sc.omb2 * g * g;
    float upd = (m / sc.bc1) * sc.lr;
    if (sc.rect > 0.f) upd = upd * (sc.adapt / (sqrtf(v) + eps)) * sc.rect;
    p = p - upd;
  }
};

// The step of every rule: 16-B vectors, 28 B of HBM per parameter, a grid-stride loop with the
// next group's loads issued before this group's arithmetic is waited for, the P % 4 tail in
// workgroup 0.
template <class Rule>
__global__ __launch_bounds__(kOptThreads) void flat_step_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, int64_t P, float grad_scale, double b1, double b2, float eps,
    float max_norm, const float* __restrict__ lr, const float* __restrict__ partials, int nb,
    float* __restrict__ scalars, AdamPlanes planes) {
  __shared__ typename Rule::Scalars sc_lds;
  // the first element group's loads are issued before the scalars are combined: their latency
  // hides the partials' combine (at config 2 every thread has about one group)
  const int64_t P4 = P / 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kOptThreads;
  int64_t i = static_cast<int64_t>(blockIdx.x) * kOptThreads + threadIdx.x;
  float4 pp{}, gg{}, mm{}, vv{};
  if (i < P4) {
    pp = reinterpret_cast<float4*>(p)[i];
    gg = reinterpret_cast<const float4*>(g)[i];
    mm = reinterpret_cast<float4*>(m)[i];
    vv = reinterpret_cast<float4*>(v)[i];
  }
  const NormClip nc = norm_clip(partials, nb, max_norm);
  if (threadIdx.x == 0) {
    sc_lds = Rule::scalars(nc, scalars[S_STEP], lr[0], b1, b2);
    if (blockIdx.x == 0) {  // the reported figures (read after the step; S_STEP is the norm pass's)
      scalars[S_TOTAL_NORM] = nc.total;
      scalars[S_CLIP] = nc.clip;
      Rule::report(sc_lds, scalars);
    }
  }
  __syncthreads();
  const typename Rule::Scalars sc = sc_lds;
  for (; i < P4; i += stride) {
    Rule::elem(pp.x, (gg.x * grad_scale) * sc.clip, mm.x, vv.x, sc, eps);
    Rule::elem(pp.y, (gg.y * grad_scale) * sc.clip, mm.y, vv.y, sc, eps);
    Rule::elem(pp.z, (gg.z * grad_scale) * sc.clip, mm.z, vv.z, sc, eps);
    Rule::elem(pp.w, (gg.w * grad_scale) * sc.clip, mm.w, vv.w, sc, eps);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (Rule::kPlanes)
      if (planes.n) adam_planes_store(planes, i, pp);
    if (i + stride < P4) {
      pp = reinterpret_cast<float4*>(p)[i + stride];
      gg = reinterpret_cast<const float4*>(g)[i + stride];
      mm = reinterpret_cast<float4*>(m)[i + stride];
      vv = reinterpret_cast<float4*>(v)[i + stride];
    }
  }
  if (blockIdx.x == 0)
    for (int64_t j = 4 * P4 + threadIdx.x; j < P; j += kOptThreads)
      Rule::elem(p[j], (g[j] * grad_scale) * sc.clip, m[j], v[j], sc, eps);
}

// The step over a buffer of two segments, a head [0, split) and a tail [split, P), each with its
// own step count (ocppo_clip_adam_step_seg): the same loop, Rule::scalars once per segment from that
// segment's count and Rule::elem with the scalars of the segment an element group lies in (split
// and P are multiples of 4, so no group straddles). The head's count is the norm pass's S_STEP. The
// tail's is S_STEP - S_TAIL_SKIPPED: a step that leaves the tail out adds one to S_TAIL_SKIPPED
// (workgroup 0, which is the only one to read it in that launch) and touches nothing else of the
// tail -- the loop ends at split; a step that takes it in reads both counts, written by earlier
// launches only, and reports the tail's in S_TAIL_STEP.
enum { S_TAIL_SKIPPED = 6, S_TAIL_STEP = 7 };

template <class Rule>
__global__ __launch_bounds__(kOptThreads) void flat_step_seg_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, int64_t P, int64_t split, int tail_active, float grad_scale, double b1,
    double b2, float eps, float max_norm, const float* __restrict__ lr,
    const float* __restrict__ partials, int nb, float* __restrict__ scalars) {
  __shared__ typename Rule::Scalars sc_lds[2];
  const int64_t P4 = (tail_active ? P : split) / 4, split4 = split / 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kOptThreads;
  int64_t i = static_cast<int64_t>(blockIdx.x) * kOptThreads + threadIdx.x;
  float4 pp{}, gg{}, mm{}, vv{};
  if (i < P4) {
    pp = reinterpret_cast<float4*>(p)[i];
    gg = reinterpret_cast<const float4*>(g)[i];
    mm = reinterpret_cast<float4*>(m)[i];
    vv = reinterpret_cast<float4*>(v)[i];
  }
  const NormClip nc = norm_clip(partials, nb, max_norm);
  if (threadIdx.x == 0) {
    const float step = scalars[S_STEP];
    sc_lds[0] = Rule::scalars(nc, step, lr[0], b1, b2);
    float tail_step = 1.f;  // unused when the tail is left out
    if (tail_active) tail_step = step - scalars[S_TAIL_SKIPPED];
    sc_lds[1] = Rule::scalars(nc, tail_step, lr[0], b1, b2);
    if (blockIdx.x == 0) {
      scalars[S_TOTAL_NORM] = nc.total;
      scalars[S_CLIP] = nc.clip;
      Rule::report(sc_lds[0], scalars);
      if (tail_active) scalars[S_TAIL_STEP] = tail_step;
      else scalars[S_TAIL_SKIPPED] = scalars[S_TAIL_SKIPPED] + 1.f;
    }
  }
  __syncthreads();
  const typename Rule::Scalars sh = sc_lds[0], st = sc_lds[1];
  for (; i < P4; i += stride) {
    const typename Rule::Scalars& sc = i >= split4 ? st : sh;
    Rule::elem(pp.x, (gg.x * grad_scale) * sc.clip, mm.x, vv.x, sc, eps);
    Rule::elem(pp.y, (gg.y * grad_scale) * sc.clip, mm.y, vv.y, sc, eps);
    Rule::elem(pp.z, (gg.z * grad_scale) * sc.clip, mm.z, vv.z, sc, eps);
    Rule::elem(pp.w, (gg.w * grad_scale) * sc.clip, mm.w, vv.w, sc, eps);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (i + stride < P4) {
      pp = reinterpret_cast<float4*>(p)[i + stride];
      gg = reinterpret_cast<const float4*>(g)[i + stride];
      mm = reinterpret_cast<float4*>(m)[i + stride];
      vv = reinterpret_cast<float4*>(v)[i + stride];
    }
  }
}

constexpr size_t kOptWorkspaceBytes = 256 + kOptBlocks * sizeof(float);

// What the three entries share once their own size and plane arguments are through: the checks,
// the norm pass (which advances the step count) and the rule's step
template <class Rule>
static int flat_step(const char* who, ocppo_stream_t stream, float* params, const float* grads,
                     float* exp_avg, float* exp_avg_sq, int64_t P, const float* lr, double beta1,
                     double beta2, double eps, double grad_scale, double max_norm, float* scalars,
                     void* workspace, size_t workspace_bytes, const AdamPlanes& planes) {
  OCPPO_REQUIRE(params && grads && exp_avg && exp_avg_sq && lr && scalars, "%s: null pointer", who);
  OCPPO_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1,
                "%s: betas (%g, %g) must be in [0, 1)", who, beta1, beta2);
  if (!workspace || workspace_bytes < kOptWorkspaceBytes)
    return fail(OCPPO_E_WORKSPACE, "%s: workspace needs %zu bytes, got %zu", who,
                kOptWorkspaceBytes, workspace_bytes);
  OCPPO_REQUIRE((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) |
                 reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) %
                        16 == 0,
                "%s: buffers must be 16-byte aligned", who);
  float* partials = reinterpret_cast<float*>(static_cast<char*>(workspace) + 256);
  const int64_t groups = ceil_div(P / 4 > 0 ? P / 4 : 1, kOptThreads);
  const int64_t nb = groups < kOptBlocks ? groups : kOptBlocks;
  const int64_t na = groups < Rule::kMaxBlocks ? groups : Rule::kMaxBlocks;
  char what[96];
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(grad_norm_kernel, dim3(static_cast<unsigned>(nb)), dim3(kOptThreads), 0, s,
                     grads, P, static_cast<float>(grad_scale), scalars, partials);
  snprintf(what, sizeof(what), "%s/norm", who);
  if (int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(flat_step_kernel<Rule>, dim3(static_cast<unsigned>(na)), dim3(kOptThreads), 0,
                     s, params, grads, exp_avg, exp_avg_sq, P, static_cast<float>(grad_scale),
                     beta1, beta2, static_cast<float>(eps), static_cast<float>(max_norm), lr,
                     partials, static_cast<int>(nb), scalars, planes);
  snprintf(what, sizeof(what), "%s/step", who);
  return check_launch(what);
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_clip_adam_workspace_bytes(int64_t P) {
  (void)P;
  return kOptWorkspaceBytes;
}

extern "C" int ocppo_clip_adam_step(ocppo_stream_t stream, float* params, const float* grads,
                                    float* exp_avg, float* exp_avg_sq, int64_t P, const float* lr,
                                    double beta1, double beta2, double eps, double grad_scale,
                                    double max_norm, float* scalars, void* workspace,
                                    size_t workspace_bytes, int n_planes,
                                    const int64_t* plane_offset, const int64_t* plane_rows,
                                    const int64_t* plane_cols, const int* plane_trans,
                                    void* const* plane_dst) {
  OCPPO_REQUIRE(P > 0, "ocppo_clip_adam_step: bad size P=%lld", (long long)P);
  AdamPlanes planes{};
  OCPPO_REQUIRE(n_planes >= 0 && n_planes <= kAdamPlaneJobs &&
                    (n_planes == 0 ||
                     (plane_offset && plane_rows && plane_cols && plane_trans && plane_dst)),
                "ocppo_clip_adam_step: n_planes=%d (0..%d) and its arrays", n_planes,
                kAdamPlaneJobs);
  planes.n = n_planes;
  for (int j = 0; j < n_planes; ++j) {
    const int64_t R = plane_rows[j], C = plane_cols[j];
    OCPPO_REQUIRE(plane_offset[j] >= 0 && plane_offset[j] % 4 == 0 && R >= 1 && C >= 4 &&
                      C % 4 == 0 && R <= INT32_MAX && C <= INT32_MAX &&
                      (plane_trans[j] ? R : C) % 8 == 0 && plane_offset[j] + R * C <= P &&
                      plane_dst[j] && reinterpret_cast<uintptr_t>(plane_dst[j]) % 16 == 0,
                  "ocppo_clip_adam_step: plane job %d (offset %lld, %lld x %lld, trans %d): "
                  "offset %% 4, cols %% 4, plane rows %% 8, inside P, 16-B aligned planes", j,
                  (long long)plane_offset[j], (long long)R, (long long)C, plane_trans[j]);
    planes.off4[j] = plane_offset[j] / 4;
    planes.len4[j] = R * C / 4;
    planes.rows[j] = static_cast<int>(R);
    planes.cols[j] = static_cast<int>(C);
    planes.trans[j] = plane_trans[j] ? 1 : 0;
    planes.dst[j] = static_cast<uint16_t*>(plane_dst[j]);
  }
  return flat_step<AdamRule>("ocppo_clip_adam_step", stream, params, grads, exp_avg, exp_avg_sq, P,
                             lr, beta1, beta2, eps, grad_scale, max_norm, scalars, workspace,
                             workspace_bytes, planes);
}

extern "C" int ocppo_clip_adam_step_exact(ocppo_stream_t stream, float* params,
                                          const float* grads, float* exp_avg, float* exp_avg_sq,
                                          int64_t P, const float* lr, double beta1, double beta2,
                                          double eps, double grad_scale, double max_norm,
                                          float* scalars, void* workspace,
                                          size_t workspace_bytes) {
  OCPPO_REQUIRE(P > 0, "ocppo_clip_adam_step_exact: bad size P=%lld", (long long)P);
  return flat_step<AdamExactRule>("ocppo_clip_adam_step_exact", stream, params, grads, exp_avg,
                                  exp_avg_sq, P, lr, beta1, beta2, eps, grad_scale, max_norm,
                                  scalars, workspace, workspace_bytes, AdamPlanes{});
}

extern "C" int ocppo_clip_adam_step_seg(ocppo_stream_t stream, float* params, const float* grads,
                                        float* exp_avg, float* exp_avg_sq, int64_t P,
                                        int64_t split, int tail_active, const float* lr,
                                        double beta1, double beta2, double eps,
                                        double grad_scale, double max_norm, float* scalars,
                                        void* workspace, size_t workspace_bytes) {
  const char* who = "ocppo_clip_adam_step_seg";
  OCPPO_REQUIRE(P > 0 && split > 0 && split < P && P % 4 == 0 && split % 4 == 0,
                "%s: bad sizes P=%lld split=%lld (0 < split < P, both multiples of 4)", who,
                (long long)P, (long long)split);
  OCPPO_REQUIRE(tail_active == 0 || tail_active == 1, "%s: tail_active=%d is not 0 / 1", who,
                tail_active);
  OCPPO_REQUIRE(params && grads && exp_avg && exp_avg_sq && lr && scalars, "%s: null pointer", who);
  OCPPO_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1,
                "%s: betas (%g, %g) must be in [0, 1)", who, beta1, beta2);
  if (!workspace || workspace_bytes < kOptWorkspaceBytes)
    return fail(OCPPO_E_WORKSPACE, "%s: workspace needs %zu bytes, got %zu", who,
                kOptWorkspaceBytes, workspace_bytes);
  OCPPO_REQUIRE((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) |
                 reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) %
                        16 == 0,
                "%s: buffers must be 16-byte aligned", who);
  float* partials = reinterpret_cast<float*>(static_cast<char*>(workspace) + 256);
  // the grids of ocppo_clip_adam_step over the whole buffer, whichever segments take part: the
  // norm pass over the active length alone then sums, thread by thread, what the whole-buffer
  // pass sums when the left-out gradients are zero (bitwise the same total)
  const int64_t groups = ceil_div(P / 4, kOptThreads);
  const int64_t nb = groups < kOptBlocks ? groups : kOptBlocks;
  const int64_t na = groups < AdamRule::kMaxBlocks ? groups : AdamRule::kMaxBlocks;
  const int64_t active = tail_active ? P : split;
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(grad_norm_kernel, dim3(static_cast<unsigned>(nb)), dim3(kOptThreads), 0, s,
                     grads, active, static_cast<float>(grad_scale), scalars, partials);
  if (int rc = check_launch("ocppo_clip_adam_step_seg/norm")) return rc;
  hipLaunchKernelGGL(flat_step_seg_kernel<AdamRule>, dim3(static_cast<unsigned>(na)),
                     dim3(kOptThreads), 0, s, params, grads, exp_avg, exp_avg_sq, P, split,
                     tail_active, static_cast<float>(grad_scale), beta1, beta2,
                     static_cast<float>(eps), static_cast<float>(max_norm), lr, partials,
                     static_cast<int>(nb), scalars);
  return check_launch("ocppo_clip_adam_step_seg/step");
}

extern "C" int ocppo_clip_radam_step(ocppo_stream_t stream, float* params, const float* grads,
                                     float* exp_avg, float* exp_avg_sq, int64_t P,
                                     const float* lr, double beta1, double beta2, double eps,
                                     double grad_scale, double max_norm, float* scalars,
                                     void* workspace, size_t workspace_bytes, int n_planes) {
  OCPPO_REQUIRE(P >= 0, "ocppo_clip_radam_step: bad size P=%lld", (long long)P);
  OCPPO_REQUIRE(n_planes == 0, "ocppo_clip_radam_step: n_planes=%d: plane jobs are "
                "ocppo_clip_adam_step's, this step writes none", n_planes);
  if (P == 0) return OCPPO_OK;
  return flat_step<RAdamRule>("ocppo_clip_radam_step", stream, params, grads, exp_avg, exp_avg_sq,
                              P, lr, beta1, beta2, eps, grad_scale, max_norm, scalars, workspace,
                              workspace_bytes, AdamPlanes{});
}

