// The Mava wrapper stack every environment runs under, once for the five env kernels (coordsum / lbf / rware / connector / mpe .hip):
// RecordEpisodeMetrics (wrappers/episode_metrics.py:60-112), the AutoResetWrapper's key handling (wrappers/auto_reset_wrapper.py:74), the
// per-agent reward / discount broadcast of the env wrappers, and the one-thread-per-env launch shape.  Dynamics, generators and
// observation functions stay in the env files.  The `lane` / `nlanes` arguments serve CoordSum, which runs one wave per env: its lanes
// share the per-agent stores and lane 0 alone writes the per-env scalars; the thread-per-env kernels leave them at their defaults.
#pragma once
#include "common.hpp"

namespace magpo {

// ---- PRNG keys ------------------------------------------------------------------------------------------------------------------
// a, b = jax.random.split(key)
__device__ __forceinline__ void split_key(uint32_t k0, uint32_t k1, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1) {
  threefry2x32(k0, k1, 0u, 0u, a0, a1);
  threefry2x32(k0, k1, 0u, 1u, b0, b1);
}
// a, _ = jax.random.split(key): the auto-reset branch's `key, _ = split(state.key)` (auto_reset_wrapper.py:74)
__device__ __forceinline__ void split_key_first(uint32_t k0, uint32_t k1, uint32_t& a0, uint32_t& a1) { threefry2x32(k0, k1, 0u, 0u, a0, a1); }

// ---- RecordEpisodeMetrics -------------------------------------------------------------------------------------------------------
struct EpisodeMetrics {   // RecordEpisodeMetricsState, the tail of every env's state struct
  uint32_t* metrics_key;  // [N][2] (kept, never consumed)
  float* run_ret; int* run_len; float* ep_ret; int* ep_len;   // [N] running / last finished episode's return and length
};

// RecordEpisodeMetrics.reset: key, reset_key = split(env key) (episode_metrics.py:62); stores the state, returns reset_key in (r0, r1)
__device__ __forceinline__ void metrics_reset(const EpisodeMetrics& m, long n, uint32_t e0, uint32_t e1, uint32_t& r0, uint32_t& r1,
                                              bool writer = true) {
  uint32_t m0, m1;
  split_key(e0, e1, m0, m1, r0, r1);
  if (writer) {
    m.metrics_key[2 * n] = m0; m.metrics_key[2 * n + 1] = m1;
    m.run_ret[n] = 0.f; m.run_len[n] = 0; m.ep_ret[n] = 0.f; m.ep_len[n] = 0;
  }
}

struct StepOut {
  float* reward;          // [N][A]
  float* discount;        // [N][A] or NULL: timestep.discount
  unsigned char* done;    // [N]    timestep.last()
  float* obs; long ldo;   // [N][A][ldo] next observation (the reset observation after an auto-reset); ldo = floats between rows
  int* obs_step;          // [N]    observation.step_count
  unsigned char* mask;    // [N][A][K] action mask, NULL for envs without illegal actions
  float* m_ep_ret; int* m_ep_len; unsigned char* m_term;   // [N] extras["episode_metrics"]
  // extras["real_next_obs"] (auto_reset_wrapper.py:52-83), both NULL unless a <env>_step_real_obs entry point passes them: the observation
  // and action mask of the stepped state BEFORE any auto-reset, in the layout of obs (row stride ldo) / mask; equal to them on steps
  // without an episode end.  Written by the CoordSum and LBF kernels only.
  float* real_obs = nullptr;
  unsigned char* real_mask = nullptr;
};

// RecordEpisodeMetrics.step (episode_metrics.py:79-112); mean_reward = the mean over agents of the step's rewards, formed by the caller
__device__ __forceinline__ void metrics_step(const EpisodeMetrics& m, const StepOut& o, long n, float mean_reward, bool done) {
  const float new_ret = m.run_ret[n] + mean_reward;
  const int new_len = m.run_len[n] + 1;
  const float ep_ret = done ? new_ret : m.ep_ret[n];
  const int ep_len = done ? new_len : m.ep_len[n];
  m.run_ret[n] = done ? 0.f : new_ret;
  m.run_len[n] = done ? 0 : new_len;
  m.ep_ret[n] = ep_ret;
  m.ep_len[n] = ep_len;
  o.m_ep_ret[n] = ep_ret;
  o.m_ep_len[n] = ep_len;
  o.m_term[n] = done ? 1 : 0;
}

// the mean over agents of one reward repeated for every agent, as episode_metrics.py:91 forms it: a sum in agent order / A in fp32
__device__ __forceinline__ float team_mean(float reward, int A) {
  float msum = 0.f;
  for (int a = 0; a < A; ++a) msum += reward;
  return __fdiv_rn(msum, (float)A);
}

// ---- timestep outputs -----------------------------------------------------------------------------------------------------------
// A is taken as a long: the kernels already hold n * (long)A for their own row addresses, and with an int A the compiler forms the
// helper's product afresh behind the loop guard (as an unsigned one it cannot merge), which costs the step kernels two VGPRs
// discount 0 on termination and 1 otherwise for every agent, and timestep.last()
__device__ __forceinline__ void write_discount_done(const StepOut& o, long n, long A, bool terminated, bool done, int lane = 0, int nlanes = 1) {
  if (o.discount) for (int a = lane; a < A; a += nlanes) o.discount[n * A + a] = terminated ? 0.f : 1.f;
  if (lane == 0) o.done[n] = done ? 1 : 0;
}
// envs with one team reward: the scalar repeated for every agent, then the above
__device__ __forceinline__ void write_team_outputs(const StepOut& o, long n, long A, float reward, bool terminated, bool done, int lane = 0,
                                                   int nlanes = 1) {
  for (int a = lane; a < A; a += nlanes) o.reward[n * A + a] = reward;
  write_discount_done(o, n, A, terminated, done, lane, nlanes);
}

// ---- one thread per env ---------------------------------------------------------------------------------------------------------
constexpr int ENV_BLOCK = 64;
// the thread's env in n; false past the end of the batch
__device__ __forceinline__ bool env_index(int N, long& n) {
  n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  return n < N;
}
inline dim3 env_grid(int N, int block = ENV_BLOCK) { return dim3((N + block - 1) / block); }

// What an entry point returns before it launches, after the env's own config check: MAGPO_OK for an empty batch, MAGPO_EINVAL with
// `stride_error` set when the action rows are narrower than the team (entry points that pass no message do not check), ENV_LAUNCH to go on.
constexpr int ENV_LAUNCH = 1;
inline int env_args(int N, int A = 0, int act_stride = 0, const char* stride_error = nullptr) {
  if (N <= 0) return MAGPO_OK;
  if (stride_error && act_stride < A) { set_error(stride_error); return MAGPO_EINVAL; }
  return ENV_LAUNCH;
}

}  // namespace magpo
