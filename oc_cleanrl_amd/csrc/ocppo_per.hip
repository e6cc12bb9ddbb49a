// Prioritized n-step replay of cleanrl/rainbow_atari_oc.py (:338-499: SumSegmentTree +
// PrioritizedReplayBuffer) with every piece of state in HBM, for num_envs == 1 as the reference
// asserts (:513). The reference keeps the buffer on the host: a numpy sum tree walked by Python
// loops, one host step per sampled element and per updated priority, and a device -> host copy of
// the per-sample loss on every train step. Here add / sample / update_priorities are launches
// that read and write device state only, so a train chunk replays from a hipGraph.
//
// State:
//   rb_obs, rb_next_obs [capacity, D] in the replay's storage dtype (u8 pixels / bf16 objects:
//     exact); the reference stores both rows too (the n-step next observation is not the next
//     slot's); rb_actions i64, rb_rewards f32, rb_dones f32 (0 / 1), [capacity] each
//   tree f32 [2 * capacity - 1] in the reference's layout: root 0, children of i are 2i + 1 and
//     2i + 2, the leaf of slot k is k + capacity - 1; capacity is any value >= 2, so leaves sit at
//     two depths when it is not a power of two
//   state i64 [8]: {pos, size, max_priority (an f32 in the low half), ring fill, ring head}
//   the n-step ring (deque(maxlen=n_step), n_step <= 8): ring_obs / ring_next_obs [n_step, D] in
//     the storage dtype, ring_actions i64, ring_rewards f32, ring_dones f32 [n_step]
//   counter i64: draws made, the counter of the splitmix64 stream (ocppo_dqn.hip's)
//
// The reference's MinSegmentTree is written on every update and never read (min() has no caller;
// the importance weights are normalised by the batch maximum), so it is not built.
#include <math.h>

#include "ocppo_common.h"
#include "ocppo_rng.h"

namespace ocppo {

constexpr int kPerMaxNStep = 8;
constexpr int kPerMaxBatch = 1024;
enum { kPerPos = 0, kPerSize = 1, kPerMaxPrio = 2, kPerFill = 3, kPerHead = 4 };

struct PerPows {
  double g[kPerMaxNStep];  // gamma ** i, formed by the host
};

// depth of tree node t (root 0): floor(log2(t + 1))
__device__ __forceinline__ int node_depth(int64_t t) {
  return 63 - __clzll(static_cast<unsigned long long>(t + 1));
}

// SumSegmentTree.update (:351-354) of one leaf by one wave: lane j owns the ancestor j + 1 levels
// up; the siblings on the path are loaded side by side, then the sums run leaf to root.
__device__ __forceinline__ void tree_set_leaf(float* __restrict__ tree, int64_t leaf, float v,
                                              int lane) {
  const int depth = node_depth(leaf);
  // the path node whose sibling this lane loads: `lane` levels above the leaf (1-based heap ids)
  const uint64_t node1 = static_cast<uint64_t>(leaf + 1) >> lane;
  float sib = 0.f;
  if (lane < depth) sib = tree[static_cast<int64_t>(node1 ^ 1ull) - 1];
  if (lane == 0) tree[leaf] = v;
  float cur = v;
  for (int j = 0; j < depth; ++j) {
    cur = cur + __shfl(sib, j, kWave);  // f32(left + right): the sum commutes
    if (lane == 0) tree[static_cast<int64_t>(static_cast<uint64_t>(leaf + 1) >> (j + 1)) - 1] = cur;
  }
}

// PrioritizedReplayBuffer.add (:435-460 with _get_n_step_info :422-433). Every workgroup reads
// the state and copies its share of the rows; the last one to arrive writes the scalars, the tree
// and the new state (graph-replay safe: the ticket re-arms itself).
template <int SDT, int ODT>
__global__ __launch_bounds__(256) void per_add_kernel(
    const void* __restrict__ obs, const void* __restrict__ next_obs,
    const int64_t* __restrict__ action, const float* __restrict__ reward,
    const float* __restrict__ done, int64_t D, int n_step, PerPows pows, float alpha,
    int64_t* state, int64_t capacity, void* __restrict__ rb_obs, void* __restrict__ rb_next,
    int64_t* __restrict__ rb_act, float* __restrict__ rb_rew, float* __restrict__ rb_done,
    float* __restrict__ tree, void* __restrict__ ring_obs, void* __restrict__ ring_next,
    int64_t* __restrict__ ring_act, float* __restrict__ ring_rew, float* __restrict__ ring_done,
    unsigned* ticket) {
  using ST = typename Elem<SDT>::T;
  using OT = typename Elem<ODT>::T;
  __shared__ int s_last;
  const int64_t pos = __hip_atomic_load(&state[kPerPos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int fill = static_cast<int>(
      __hip_atomic_load(&state[kPerFill], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  int head = static_cast<int>(
      __hip_atomic_load(&state[kPerHead], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  fill = fill < 0 ? 0 : (fill > n_step ? n_step : fill);  // a corrupt state cannot index past the ring
  head = head < 0 ? 0 : head % n_step;
  // deque.append: a full ring drops its oldest entry
  int slot;
  if (fill == n_step) {
    slot = head;
    head = (head + 1) % n_step;
  } else {
    slot = (head + fill) % n_step;
    ++fill;
  }
  const bool emit = fill == n_step && pos >= 0 && pos < capacity;
  // _get_n_step_info: the first done entry, else the last; the new entry's scalars come from the
  // arguments, the older ones from the ring (no thread reads what this launch writes)
  const float new_r = reward[0], new_d = done[0];
  double acc = 0.0;
  int last = (head + fill - 1) % n_step;
  float out_done = 0.f;
  if (emit) {
    out_done = last == slot ? new_d : ring_done[last];
    for (int i = 0; i < n_step; ++i) {
      const int s = (head + i) % n_step;
      const float r = s == slot ? new_r : ring_rew[s];
      const float d = s == slot ? new_d : ring_done[s];
      acc += pows.g[i] * static_cast<double>(r);
      if (d != 0.f) {
        last = s;
        out_done = 1.f;
        break;
      }
    }
  }
  const int first = head;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < D;
       g += stride) {
    const float o = Elem<ODT>::roundtrip(Elem<SDT>::load(static_cast<const ST*>(obs), g));
    const float no = Elem<ODT>::roundtrip(Elem<SDT>::load(static_cast<const ST*>(next_obs), g));
    if (emit) {
      const float fo = first == slot ? o : Elem<ODT>::load(static_cast<const OT*>(ring_obs), first * D + g);
      const float ln = last == slot ? no : Elem<ODT>::load(static_cast<const OT*>(ring_next), last * D + g);
      Elem<ODT>::store(static_cast<OT*>(rb_obs), pos * D + g, fo);
      Elem<ODT>::store(static_cast<OT*>(rb_next), pos * D + g, ln);
    }
    Elem<ODT>::store(static_cast<OT*>(ring_obs), slot * D + g, o);
    Elem<ODT>::store(static_cast<OT*>(ring_next), slot * D + g, no);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last || threadIdx.x >= kWave) return;
  const int lane = threadIdx.x;
  if (emit) {
    const float maxp = reinterpret_cast<const float*>(state + kPerMaxPrio)[0];
    tree_set_leaf(tree, pos + capacity - 1, powf(maxp, alpha), lane);
  }
  if (lane == 0) {
    const int64_t new_a = action[0];
    if (emit) {
      rb_act[pos] = first == slot ? new_a : ring_act[first];
      rb_rew[pos] = static_cast<float>(acc);
      rb_done[pos] = out_done;
      const int64_t size = state[kPerSize];
      __hip_atomic_store(&state[kPerPos], (pos + 1) % capacity, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      state[kPerSize] = size + 1 < capacity ? size + 1 : capacity;
    }
    ring_act[slot] = new_a;
    ring_rew[slot] = new_r;
    ring_done[slot] = new_d;
    if (emit && out_done != 0.f) {  // n_step_buffer.clear()
      fill = 0;
      head = 0;
    }
    __hip_atomic_store(&state[kPerFill], static_cast<int64_t>(fill), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&state[kPerHead], static_cast<int64_t>(head), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// PrioritizedReplayBuffer.update_priorities (:492-499) as ONE workgroup, thread i owns batch
// element i. The tree the reference's sequential updates leave is a pure function of the final
// leaves (each inner node is f32(left + right) of its final children), so: write the leaves (of a
// repeated index the LAST occurrence, the reference's order), then recompute the touched
// ancestors level by level, deepest first, with a barrier between levels. Threads that share an
// ancestor store the same value. No float atomic.
__global__ __launch_bounds__(kPerMaxBatch) void per_update_kernel(
    const int64_t* __restrict__ indices, const float* __restrict__ loss, int B, float eps,
    float alpha, int64_t* state, int64_t capacity, float* tree) {
  __shared__ int64_t s_idx[kPerMaxBatch];
  __shared__ float s_red[kPerMaxBatch / kWave];
  const int i = threadIdx.x, lane = i & (kWave - 1), wv = i / kWave;
  const bool have = i < B;
  int64_t idx = have ? indices[i] : -1;
  if (idx < 0 || idx >= capacity) idx = -1;  // never a store outside the tree
  const float p = have ? fabsf(loss[i]) + eps : 0.f;
  s_idx[i] = idx;
  float m = p;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
  if (lane == 0) s_red[wv] = m;
  __syncthreads();
  if (i == 0) {
    float* maxp = reinterpret_cast<float*>(state + kPerMaxPrio);
    float mm = maxp[0];
    for (int w = 0; w < static_cast<int>(blockDim.x) / kWave; ++w) mm = fmaxf(mm, s_red[w]);
    maxp[0] = mm;
  }
  const int64_t leaf = idx + capacity - 1;
  int depth = 0;
  if (idx >= 0) {
    bool later = false;
    for (int j = i + 1; j < B; ++j) later |= s_idx[j] == idx;
    if (!later) tree[leaf] = powf(p, alpha);
    depth = node_depth(leaf);
  }
  const int deepest = node_depth(2 * capacity - 2);
  for (int d = deepest - 1; d >= 0; --d) {
    __syncthreads();  // the level below is complete (and visible: one workgroup, one CU)
    if (idx >= 0 && depth > d) {
      const int64_t node = static_cast<int64_t>(static_cast<uint64_t>(leaf + 1) >> (depth - d)) - 1;
      const float l = __hip_atomic_load(&tree[2 * node + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const float r = __hip_atomic_load(&tree[2 * node + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_store(&tree[node], l + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

// PrioritizedReplayBuffer.sample (:462-490), indices and weights: ONE workgroup, thread i owns
// sample i.
//   segment = f32(total) / f32(B); a = segment * i, b = segment * (i + 1) (f32, as numpy keeps
//   np.float32 / int and np.float32 * int); upperbound = a + (b - a) * u in f64
//   (np.random.uniform), u in [0, 1) from the counter-based stream; retrieve (:359-369) in f64
//   against the f32 nodes; probs = leaf; weights = (f32(size) * probs / total) ** f32(-beta)
//   divided by the batch maximum; beta = min(1, beta0 + t * (1 - beta0) / total_timesteps) in
//   f64 from the device step counter (:611-614).
__global__ __launch_bounds__(kPerMaxBatch) void per_sample_kernel(
    uint64_t seed, int64_t* counter, const int64_t* __restrict__ state,
    const int64_t* __restrict__ step, int64_t step_offset, double beta0, double total_timesteps,
    int64_t capacity, const float* __restrict__ tree, const int64_t* __restrict__ rb_act,
    const float* __restrict__ rb_rew, const float* __restrict__ rb_done, int B,
    const double* __restrict__ ub_in, int64_t* __restrict__ act_out, float* __restrict__ rew_out,
    float* __restrict__ done_out, int64_t* __restrict__ idx_out, float* __restrict__ w_out,
    float* __restrict__ probs_out, double* __restrict__ ub_out, float* __restrict__ beta_out) {
  __shared__ float s_red[kPerMaxBatch / kWave];
  const int i = threadIdx.x, lane = i & (kWave - 1), wv = i / kWave;
  const bool have = i < B;
  const int64_t ctr = counter[0];
  const float total = tree[0];
  const int64_t tree_size = 2 * capacity - 1;
  double beta = beta0;
  if (step) {
    const double t = static_cast<double>(step[0] + step_offset);
    beta = beta0 + t * (1.0 - beta0) / total_timesteps;
  }
  beta = beta < 1.0 ? beta : 1.0;
  float w = 0.f;
  if (have) {
    const float segment = total / static_cast<float>(B);
    const float a = segment * static_cast<float>(i), b = segment * static_cast<float>(i + 1);
    double ub;
    if (ub_in) {
      ub = ub_in[i];
    } else {
      const uint64_t h = splitmix64(splitmix64(seed ^ 0x2545F4914F6CDD1Dull) +
                                   static_cast<uint64_t>(ctr) * 0x100000001B3ull +
                                   static_cast<uint64_t>(i));
      const double u = unit53(h);
      ub = static_cast<double>(a) + (static_cast<double>(b) - static_cast<double>(a)) * u;
    }
    if (ub_out) ub_out[i] = ub;
    int64_t node = 0;
    double v = ub;
    while (node * 2 + 1 < tree_size) {
      const int64_t left = node * 2 + 1;
      const double tl = static_cast<double>(tree[left]);
      if (v <= tl) {
        node = left;
      } else {
        v -= tl;
        node = left + 1;
      }
    }
    const int64_t idx = node - (capacity - 1);  // in [0, capacity) by construction
    const float prob = tree[node];
    idx_out[i] = idx;
    act_out[i] = rb_act[idx];
    rew_out[i] = rb_rew[idx];
    done_out[i] = rb_done[idx];
    if (probs_out) probs_out[i] = prob;
    const float size = static_cast<float>(state[kPerSize]);
    w = powf(size * prob / total, static_cast<float>(-beta));
  }
  float m = have ? w : -INFINITY;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
  if (lane == 0) s_red[wv] = m;
  __syncthreads();  // every thread has read the counter
  float mm = s_red[0];
  for (int k = 1; k < static_cast<int>(blockDim.x) / kWave; ++k) mm = fmaxf(mm, s_red[k]);
  if (have) w_out[i] = w / mm;
  if (i == 0) {
    counter[0] = ctr + 1;
    if (beta_out) beta_out[0] = static_cast<float>(beta);
  }
}

// the rows of the sampled indices as f32 (the second launch of a sample: spread over workgroups)
template <int ODT>
__global__ __launch_bounds__(256) void per_gather_kernel(
    const int64_t* __restrict__ idx, int64_t B, int64_t D, int64_t capacity,
    const void* __restrict__ rb_obs, const void* __restrict__ rb_next, float* __restrict__ obs_out,
    float* __restrict__ next_out) {
  using OT = typename Elem<ODT>::T;
  const int64_t total = B * D;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < total;
       g += stride) {
    const int64_t b = g / D, k = g - b * D;
    int64_t i = idx[b];
    i = i < 0 ? 0 : (i >= capacity ? capacity - 1 : i);
    obs_out[g] = Elem<ODT>::load(static_cast<const OT*>(rb_obs), i * D + k);
    next_out[g] = Elem<ODT>::load(static_cast<const OT*>(rb_next), i * D + k);
  }
}

}  // namespace ocppo

using namespace ocppo;

extern "C" size_t ocppo_per_workspace_bytes(void) { return 256; }

static bool per_dtype_ok(int d) { return d == OCPPO_F32 || d == OCPPO_BF16 || d == OCPPO_U8; }

extern "C" int ocppo_per_add(ocppo_stream_t stream, const void* obs, const void* next_obs,
                             int obs_dtype, const int64_t* action, const float* reward,
                             const float* done, int64_t D, int64_t n_step,
                             const double* gamma_pows, double alpha, int64_t* state,
                             int64_t capacity, void* rb_obs, void* rb_next_obs, int rb_dtype,
                             int64_t* rb_actions, float* rb_rewards, float* rb_dones, float* tree,
                             void* ring_obs, void* ring_next_obs, int64_t* ring_actions,
                             float* ring_rewards, float* ring_dones, void* workspace) {
  OCPPO_REQUIRE(D >= 1 && capacity >= 2 && n_step >= 1 && n_step <= kPerMaxNStep,
                "ocppo_per_add: bad sizes D=%lld capacity=%lld n_step=%lld (capacity >= 2, 1 <= "
                "n_step <= %d)", (long long)D, (long long)capacity, (long long)n_step,
                kPerMaxNStep);
  OCPPO_REQUIRE(obs && next_obs && action && reward && done && gamma_pows && state && rb_obs &&
                    rb_next_obs && rb_actions && rb_rewards && rb_dones && tree && ring_obs &&
                    ring_next_obs && ring_actions && ring_rewards && ring_dones && workspace,
                "ocppo_per_add: null pointer");
  OCPPO_REQUIRE(per_dtype_ok(obs_dtype) && per_dtype_ok(rb_dtype), "ocppo_per_add: bad dtypes");
  PerPows pows{};
  for (int i = 0; i < n_step; ++i) pows.g[i] = gamma_pows[i];
  int64_t g = ceil_div(D, 256);
  g = g < 64 ? g : 64;
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  unsigned* ticket = static_cast<unsigned*>(workspace);
#define OCPPO_PADD(S, O)                                                                          \
  if (obs_dtype == S && rb_dtype == O) {                                                          \
    hipLaunchKernelGGL((per_add_kernel<S, O>), dim3(g), dim3(256), 0, s, obs, next_obs, action,   \
                       reward, done, D, (int)n_step, pows, static_cast<float>(alpha), state,      \
                       capacity, rb_obs, rb_next_obs, rb_actions, rb_rewards, rb_dones, tree,     \
                       ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, ticket);  \
    return check_launch("ocppo_per_add");                                                         \
  }
  OCPPO_PADD(OCPPO_F32, OCPPO_F32)
  OCPPO_PADD(OCPPO_F32, OCPPO_BF16)
  OCPPO_PADD(OCPPO_F32, OCPPO_U8)
  OCPPO_PADD(OCPPO_U8, OCPPO_F32)
  OCPPO_PADD(OCPPO_U8, OCPPO_BF16)
  OCPPO_PADD(OCPPO_U8, OCPPO_U8)
  OCPPO_PADD(OCPPO_BF16, OCPPO_F32)
  OCPPO_PADD(OCPPO_BF16, OCPPO_BF16)
  OCPPO_PADD(OCPPO_BF16, OCPPO_U8)
#undef OCPPO_PADD
  return fail(OCPPO_E_INVALID, "ocppo_per_add: unsupported dtype pair");
}

extern "C" int ocppo_per_update_priorities(ocppo_stream_t stream, const int64_t* indices,
                                           const float* loss_per_sample, int64_t B, double eps,
                                           double alpha, int64_t* state, int64_t capacity,
                                           float* tree) {
  OCPPO_REQUIRE(B >= 1 && B <= kPerMaxBatch && capacity >= 2,
                "ocppo_per_update_priorities: bad sizes B=%lld capacity=%lld (1 <= B <= %d, "
                "capacity >= 2)", (long long)B, (long long)capacity, kPerMaxBatch);
  OCPPO_REQUIRE(indices && loss_per_sample && state && tree,
                "ocppo_per_update_priorities: null pointer");
  clear_stale_error();
  const int block = static_cast<int>(ceil_div(B, kWave)) * kWave;
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(block), 0, as_stream(stream), indices,
                     loss_per_sample, (int)B, static_cast<float>(eps), static_cast<float>(alpha),
                     state, capacity, tree);
  return check_launch("ocppo_per_update_priorities");
}

extern "C" int ocppo_per_sample(ocppo_stream_t stream, uint64_t seed, int64_t* counter,
                                const int64_t* state, const int64_t* step, int64_t step_offset,
                                double beta0, double total_timesteps, int64_t capacity, int64_t D,
                                const void* rb_obs, const void* rb_next_obs, int rb_dtype,
                                const int64_t* rb_actions, const float* rb_rewards,
                                const float* rb_dones, const float* tree, int64_t B,
                                const double* upperbounds_in, float* obs_out, float* next_obs_out,
                                int64_t* actions_out, float* rewards_out, float* dones_out,
                                int64_t* indices_out, float* weights_out, float* probs_out,
                                double* upperbounds_out, float* beta_out) {
  OCPPO_REQUIRE(B >= 1 && B <= kPerMaxBatch && D >= 1 && capacity >= 2 && total_timesteps > 0,
                "ocppo_per_sample: bad sizes B=%lld D=%lld capacity=%lld (1 <= B <= %d, capacity "
                ">= 2, total_timesteps > 0)", (long long)B, (long long)D, (long long)capacity,
                kPerMaxBatch);
  OCPPO_REQUIRE(counter && state && rb_obs && rb_next_obs && rb_actions && rb_rewards &&
                    rb_dones && tree && obs_out && next_obs_out && actions_out && rewards_out &&
                    dones_out && indices_out && weights_out,
                "ocppo_per_sample: null pointer");
  OCPPO_REQUIRE(per_dtype_ok(rb_dtype), "ocppo_per_sample: bad dtype %d", rb_dtype);
  clear_stale_error();
  hipStream_t s = as_stream(stream);
  const int block = static_cast<int>(ceil_div(B, kWave)) * kWave;
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(block), 0, s, seed, counter, state, step,
                     step_offset, beta0, total_timesteps, capacity, tree, rb_actions, rb_rewards,
                     rb_dones, (int)B, upperbounds_in, actions_out, rewards_out, dones_out,
                     indices_out, weights_out, probs_out, upperbounds_out, beta_out);
  if (int rc = check_launch("ocppo_per_sample")) return rc;
  int64_t g = ceil_div(B * D, 256);
  g = g < 4096 ? g : 4096;
#define OCPPO_PGATHER(O)                                                                     \
  hipLaunchKernelGGL(per_gather_kernel<O>, dim3(g), dim3(256), 0, s, indices_out, B, D,      \
                     capacity, rb_obs, rb_next_obs, obs_out, next_obs_out)
  if (rb_dtype == OCPPO_F32)
    OCPPO_PGATHER(OCPPO_F32);
  else if (rb_dtype == OCPPO_BF16)
    OCPPO_PGATHER(OCPPO_BF16);
  else
    OCPPO_PGATHER(OCPPO_U8);
#undef OCPPO_PGATHER
  return check_launch("ocppo_per_sample/gather");
}
