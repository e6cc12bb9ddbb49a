// Counter-based random numbers of the library: the splitmix64 finaliser every stream here is built
// on (replay sampling, the prioritized replay's stratified draws, the synthetic env, CartPole's
// reset), its 53-bit uniform, and the epsilon-greedy decision of the value-based learners. Each
// stream's key constant stays with its user.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ocppo {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the top 53 bits as a double in [0, 1) (exact multiple of 2^-53)
__device__ __forceinline__ double unit53(uint64_t h) {
  return static_cast<double>(h >> 11) * (1.0 / 9007199254740992.0);
}

// The classic-control envs' reset stream: the key of env n's episode; draw i of that reset is
// unit53(splitmix64(key + i)) (CartPole's four state values, Pendulum's two).
__device__ __forceinline__ uint64_t env_reset_key(uint64_t seed, int64_t n, int64_t episode) {
  return splitmix64(splitmix64(seed) + static_cast<uint64_t>(n) * 0x100000001B3ull) ^
         splitmix64(static_cast<uint64_t>(episode) + 0x632BE59BD9B4E019ull);
}

// epsilon-greedy (dqn_atari_oc.py:345-350, c51_atari_oc.py:303-308): epsilon = max(slope * t +
// start_e, end_e) with slope = (end_e - start_e) / duration (linear_schedule, :230-232, all in
// double), ONE coin per global step t for all envs (the reference's `random.random() < epsilon`
// decides for the whole vector), and env e's random action uniform in [0, A).
// The constructor is the step's part: it depends on kernel arguments and the step counter only, so
// it is wave-uniform and a kernel that loops over envs builds it once, before the loop.
// random_action(e, A) is the env's part.
constexpr uint64_t kEpsGreedyKey = 0xA0761D6478BD642Full;

struct EpsGreedy {
  double eps;
  uint64_t h;    // the step's hash: the coin, and the base of the envs' random actions
  bool explore;  // coin < eps

  __device__ __forceinline__ EpsGreedy(uint64_t seed, int64_t t, double start_e, double end_e,
                                       double duration) {
    const double slope = (end_e - start_e) / duration;
    eps = slope * static_cast<double>(t) + start_e;
    eps = eps > end_e ? eps : end_e;
    h = splitmix64(splitmix64(seed ^ kEpsGreedyKey) + static_cast<uint64_t>(t));
    explore = unit53(h) < eps;
  }
  __device__ __forceinline__ int64_t random_action(int64_t e, int A) const {
    return static_cast<int64_t>(splitmix64(h + static_cast<uint64_t>(e) + 1) %
                                static_cast<uint64_t>(A));
  }
};

}  // namespace ocppo
