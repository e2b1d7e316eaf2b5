// CoordSum environment + Mava wrapper stack as one HIP kernel per call (gfx950).
//
// Replaces, for a batch of envs, the reference's vmap(env.step) over
//   RecordEpisodeMetrics (wrappers/episode_metrics.py:60-112) -> AutoResetWrapper
//   (wrappers/auto_reset_wrapper.py:60-101) -> AgentIDWrapper (wrappers/observation.py:42-54)
//   -> CoordSumWrapper (wrappers/matrax.py:117-142) -> CoordSum (coordsum/env.py:55-139).
// Integer work, HBM-bound: one wave per env so the 4*T_lim-byte record row is read coalesced; the
// per-action histogram is K wave ballots; JAX's clamped out-of-range gather / dynamic_update_slice
// (record row min(target, K-1)) is reproduced explicitly.  Auto-reset branches per env
// (the reference evaluates reset for every env every step under vmap(cond)).
#include "env_wrappers.hpp"

namespace magpo {

struct CoordSumState {
  int* step_count;       // [N]
  int* target;           // [N][TLIM+1]
  int* record;           // [N][K][TLIM]
  uint32_t* key;         // [N][2]   CoordSum State.key
  EpisodeMetrics m;
};
struct CoordSumCfg { int N, A, K, TLIM, maxval; };

// jax.random.randint(key, (n,), 0, span) element i (see oracle/prng.py:randint)
__device__ __forceinline__ int randint_elem(uint32_t ka0, uint32_t ka1, uint32_t kb0, uint32_t kb1, uint32_t i, uint32_t span) {
  const uint32_t hi = random_bits32(ka0, ka1, i), lo = random_bits32(kb0, kb1, i);
  uint32_t mult = 65536u % span;
  mult = (mult * mult) % span;
  return (int)(((hi % span) * mult + (lo % span)) % span);
}

// CoordSum.reset for one env by one wave: fills target / record / step_count / key; returns target[0] on lane 0.
__device__ __forceinline__ int core_reset(const CoordSumState& s, const CoordSumCfg& c, long n, uint32_t k0, uint32_t k1, int lane) {
  uint32_t nk0, nk1, t0, t1, a0, a1, b0, b1;
  split_key(k0, k1, nk0, nk1, t0, t1);   // key, target_key
  split_key(t0, t1, a0, a1, b0, b1);     // randint: k1, k2 = split(target_key)
  const uint32_t span = c.maxval > 0 ? (uint32_t)c.maxval : 1u;
  int first = 0;
  for (int i = lane; i <= c.TLIM; i += 64) {
    int v = randint_elem(a0, a1, b0, b1, (uint32_t)i, span);
    s.target[n * (c.TLIM + 1) + i] = v;
    if (i == 0) first = v;
  }
  int* rec = s.record + n * (long)c.K * c.TLIM;
  for (int i = lane; i < c.K * c.TLIM; i += 64) rec[i] = -1;
  if (lane == 0) {
    s.step_count[n] = 0;
    s.key[2 * n] = nk0;
    s.key[2 * n + 1] = nk1;
  }
  return __shfl(first, 0, 64);
}

__device__ __forceinline__ void write_obs_rows(float* __restrict__ obs, long n, const CoordSumCfg& c, int target_val, int lane) {
  const int F = c.A + 1;
  float* o = obs + n * (long)c.A * F;
  for (int i = lane; i < c.A * F; i += 64) {
    int a = i / F, f = i - a * F;
    o[i] = f < c.A ? (f == a ? 1.f : 0.f) : (float)target_val;
  }
}
__device__ __forceinline__ void write_obs(float* __restrict__ obs, int* __restrict__ obs_step, long n, const CoordSumCfg& c,
                                          int target_val, int step, int lane) {
  write_obs_rows(obs, n, c, target_val, lane);
  if (lane == 0) obs_step[n] = step;
}

__global__ __launch_bounds__(256) void k_coordsum_reset(CoordSumState s, CoordSumCfg c, const uint32_t* __restrict__ env_keys,
                                                        float* __restrict__ obs, int* __restrict__ obs_step) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= c.N) return;
  uint32_t r0, r1;
  metrics_reset(s.m, n, env_keys[2 * n], env_keys[2 * n + 1], r0, r1, lane == 0);
  const int tv = core_reset(s, c, n, r0, r1, lane);
  write_obs(obs, obs_step, n, c, tv, 0, lane);
}

__global__ __launch_bounds__(256) void k_coordsum_step(CoordSumState s, CoordSumCfg c, const int* __restrict__ actions,
                                                       int act_stride, StepOut o, int auto_reset) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= c.N) return;
  const int t = s.step_count[n];
  const int* tgt = s.target + n * (c.TLIM + 1);
  const int g = tgt[min(t, c.TLIM)];
  int av = 0;
  for (int a = lane; a < c.A; a += 64) av += actions[n * act_stride + a];
  const int asum = (int)wave_sum((float)av);  // exact: |sum| < 2^24
  const int a0 = actions[n * act_stride];
  const int row = min(g, c.K - 1);
  int* rec = s.record + (n * c.K + row) * (long)c.TLIM;
  // histogram of the valid entries of the row: lane b owns bin b.  bincount(length=time_limit)
  // drops values >= time_limit (coordsum/env.py:92-97), so only min(K, T_lim) bins exist.
  const int nbins = min(c.K, c.TLIM);
  int cnt = 0;
  for (int base = 0; base < c.TLIM; base += 64) {
    const int i = base + lane;
    const int v = i < c.TLIM ? rec[i] : -1;
    for (int b = 0; b < nbins; ++b) {
      const unsigned long long m = __ballot(v == b);
      if (lane == b) cnt += __popcll(m);
    }
  }
  // argmax with first-max tie-break (bins >= K are empty; an empty row gives guess 0)
  int keyv = lane < nbins ? cnt * 64 + (63 - lane) : -1;
  for (int off = 32; off > 0; off >>= 1) keyv = max(keyv, __shfl_xor(keyv, off, 64));
  const int guess = 63 - (keyv & 63);
  const bool sum_match = asum == g;
  const float reward = sum_match ? (guess == a0 ? 1.0f : 2.0f) : 0.0f;
  if (lane == 0) rec[min(t, c.TLIM - 1)] = a0;
  const int steps = t + 1;
  const bool done = steps >= c.TLIM;
  int obs_target = tgt[min(steps, c.TLIM)];
  int obs_step = steps;
  if (lane == 0) s.step_count[n] = steps;
  if (o.real_obs) write_obs_rows(o.real_obs, n, c, obs_target, lane);   // extras["real_next_obs"]: the stepped state's observation
  if (done && auto_reset) {
    uint32_t k0 = s.key[2 * n], k1 = s.key[2 * n + 1], nk0, nk1;
    split_key_first(k0, k1, nk0, nk1);
    obs_target = core_reset(s, c, n, nk0, nk1, lane);
    obs_step = 0;
  }
  write_team_outputs(o, n, c.A, reward, done, done, lane, 64);   // termination() at the time limit (coordsum/env.py:121-129)
  write_obs(o.obs, o.obs_step, n, c, obs_target, obs_step, lane);
  if (lane == 0) metrics_step(s.m, o, n, reward, done);   // the mean over agents of identical rewards == reward
}

}  // namespace magpo

using namespace magpo;

static int check_cfg(int N, int A, int K, int TLIM) {
  if (N < 0 || A < 1 || K < 1 || K > 64 || TLIM < 1) {
    set_error("coordsum: need A >= 1, 1 <= K <= 64, time_limit >= 1");
    return MAGPO_EINVAL;
  }
  return MAGPO_OK;
}

extern "C" int magpo_coordsum_reset(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                                    float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                                    int maxval, const uint32_t* env_keys, float* obs, int* obs_step, hipStream_t st) {
  if (int e = check_cfg(N, A, K, TLIM)) return e;
  if (int e = env_args(N); e != ENV_LAUNCH) return e;
  CoordSumState s{step_count, target, record, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  CoordSumCfg c{N, A, K, TLIM, maxval};
  hipLaunchKernelGGL(k_coordsum_reset, dim3((N + 3) / 4), dim3(256), 0, st, s, c, env_keys, obs, obs_step);
  return check_launch("magpo_coordsum_reset");
}

extern "C" int magpo_coordsum_step(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                                   float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                                   int maxval, const int* actions, int act_stride, float* reward, float* discount,
                                   unsigned char* done, float* obs, int* obs_step, float* m_ep_ret, int* m_ep_len, unsigned char* m_term,
                                   int auto_reset, hipStream_t st) {
  if (int e = check_cfg(N, A, K, TLIM)) return e;
  if (int e = env_args(N); e != ENV_LAUNCH) return e;
  CoordSumState s{step_count, target, record, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  CoordSumCfg c{N, A, K, TLIM, maxval};
  StepOut o{reward, discount, done, obs, A + 1, obs_step, nullptr, m_ep_ret, m_ep_len, m_term};   // dense rows
  hipLaunchKernelGGL(k_coordsum_step, dim3((N + 3) / 4), dim3(256), 0, st, s, c, actions, act_stride, o, auto_reset);
  return check_launch("magpo_coordsum_step");
}

// magpo_coordsum_step + extras["real_next_obs"]: the same kernel with StepOut::real_obs set
extern "C" int magpo_coordsum_step_real_obs(int* step_count, int* target, int* record, uint32_t* key, uint32_t* metrics_key,
                                            float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int K, int TLIM,
                                            int maxval, const int* actions, int act_stride, float* reward, float* discount,
                                            unsigned char* done, float* obs, int* obs_step, float* m_ep_ret, int* m_ep_len,
                                            unsigned char* m_term, int auto_reset, float* real_obs, hipStream_t st) {
  if (int e = check_cfg(N, A, K, TLIM)) return e;
  if (int e = env_args(N); e != ENV_LAUNCH) return e;
  CoordSumState s{step_count, target, record, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  CoordSumCfg c{N, A, K, TLIM, maxval};
  StepOut o{reward, discount, done, obs, A + 1, obs_step, nullptr, m_ep_ret, m_ep_len, m_term, real_obs, nullptr};
  hipLaunchKernelGGL(k_coordsum_step, dim3((N + 3) / 4), dim3(256), 0, st, s, c, actions, act_stride, o, auto_reset);
  return check_launch("magpo_coordsum_step_real_obs");
}

// ---- input classes of the networks' first layers (csrc/classtab.hip) for wrapped CoordSum observations -----------------
// A token's observation is [one-hot agent id | target] (observation.py:42-54, matrax.py:117-134) and its position the env step
// count, so the first layers see only A*maxval (actor), A*maxval*npos (encoder) and (K+1)*npos (decoder) distinct inputs.
namespace magpo {
__global__ void k_coordsum_classes(const float* __restrict__ obs, int F, const int* __restrict__ prev, const int* __restrict__ pos,
                                   int A, int maxval, int npos, int* __restrict__ cls_enc, int* __restrict__ cls_dec, long R) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* o = obs + r * F;
  int ag = 0;
  for (int a = 1; a < A; ++a) ag = o[a] != 0.f ? a : ag;
  int g = (int)o[A];
  g = g < 0 ? 0 : (g >= maxval ? maxval - 1 : g);
  int p = pos ? pos[r] : 0;
  p = p < 0 ? 0 : (p >= npos ? npos - 1 : p);
  cls_enc[r] = (ag * maxval + g) * npos + p;
  if (cls_dec) cls_dec[r] = prev[r] * npos + p;
}
// the distinct rows themselves, in class order: obs_tab [A*maxval*npos][F], pos_tab, and for the decoder prev_tab / pos_tab
__global__ void k_coordsum_class_rows(int A, int maxval, int npos, int K, float* __restrict__ obs_tab, int* __restrict__ pos_enc,
                                      int* __restrict__ prev_dec, int* __restrict__ pos_dec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int F = A + 1, Ce = A * maxval * npos, Cd = (K + 1) * npos;
  if (i < Ce) {
    const int p = i % npos, ag_g = i / npos, g = ag_g % maxval, ag = ag_g / maxval;
    for (int a = 0; a < A; ++a) obs_tab[(long)i * F + a] = a == ag ? 1.f : 0.f;
    obs_tab[(long)i * F + A] = (float)g;
    pos_enc[i] = p;
  }
  if (i < Cd) { prev_dec[i] = i / npos; pos_dec[i] = i % npos; }
}
}  // namespace magpo

extern "C" int magpo_coordsum_classes(const float* obs, int F, const int* prev, const int* pos, int A, int maxval, int npos,
                                      int* cls_enc, int* cls_dec, long R, hipStream_t st) {
  if (F != A + 1) { magpo::set_error("coordsum_classes: observations must be [one-hot agent id | target] (F = A + 1)"); return MAGPO_EINVAL; }
  hipLaunchKernelGGL(magpo::k_coordsum_classes, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, obs, F, prev, pos, A, maxval, npos,
                     cls_enc, cls_dec, R);
  return magpo::check_launch("magpo_coordsum_classes");
}

extern "C" int magpo_coordsum_class_rows(int A, int maxval, int npos, int K, float* obs_tab, int* pos_enc, int* prev_dec, int* pos_dec,
                                         hipStream_t st) {
  const int Ce = A * maxval * npos, Cd = (K + 1) * npos, n = Ce > Cd ? Ce : Cd;
  hipLaunchKernelGGL(magpo::k_coordsum_class_rows, dim3((n + 255) / 256), dim3(256), 0, st, A, maxval, npos, K, obs_tab, pos_enc, prev_dec, pos_dec);
  return magpo::check_launch("magpo_coordsum_class_rows");
}
