// MPE simple_spread (discrete actions) + Mava wrappers (MPEWrapper / JaxMarlWrapper, jaxmarl.py:169-243,424-455; AgentID, AutoReset,
// RecordEpisodeMetrics; mava/utils/make_env.py:138-170) for gfx950.
// UNPINNED DYNAMICS: the environment (JaxMARL MPE_simple_spread_v3) is third-party and absent from the reference tree; this kernel and
// tests/mpe_ref.py restate it from memory (every rule is listed in that module's docstring) and are bit-exact with each other.  The
// wrapper rules (key splits, per-agent rewards, discount 1 - done, the observed step counter) are pinned by the reference tree.
//
// Rules, in the order the step applies them:
//   * action a of agent i (mp_decode): 0 no-op, 1 / 2 = -x / +x, 3 / 4 = -y / +y, times accel 5; anything outside 0..4 is a no-op.
//   * contact force on agent i from agent j != i: 100 * (p_i - p_j) / |p_i - p_j| * softplus(-(|p_i - p_j| - 0.3) / k) * k, k = 1e-3,
//     summed over j in index order, then the action force added.  Landmarks neither collide nor move.
//   * p += v * dt, then v *= 1 - damping, then v += F / m * dt (dt 0.1, damping 0.25, m 1, no speed cap).
//   * reward of agent i on the post-step state: local_ratio * (-#{j != i : |p_i - p_j| < 0.3}) + (1 - local_ratio) * sum over landmarks
//     in index order of -min_agents |p_a - p_l|.
//   * the inner step counter is tested BEFORE its increment: done iff inner_step >= time_limit, so an episode lasts time_limit + 1
//     steps.  On done the inner env resets itself from key_reset = split(step_key)[1] (the eval env continues from that state); the
//     train env's auto-reset then overwrites it.
// Numerics: fp32 with no contraction (the pragma below), correctly rounded division and square root (mp_sqrt); the soft-plus is evaluated in
// fp64 as max(x, 0) + log1p(exp(-|x|)) and rounded once to fp32 (JaxMARL's fp32 logaddexp may differ from it by less than an ulp).
// One thread per env; its agents' positions, velocities and forces live in LDS ([6 A][64] floats per block, thread-minor so that a
// wave's accesses hit 64 distinct banks), which keeps the runtime-indexed entity loops out of scratch.
#include "env_wrappers.hpp"

#pragma clang fp contract(off)

namespace magpo {

constexpr int MP_NACT = 5, MP_MAXA = 32, MP_MAXL = 32, MP_BLK = 64;
constexpr float MP_RAD = 0.15f, MP_ACCEL = 5.f, MP_DT = 0.1f, MP_DAMP = 0.25f, MP_CONTACT = 100.f, MP_MARGIN = 1e-3f;

struct MpState {
  float* pos;                             // [N][A+L][2]  agents, then landmarks
  float* vel;                             // [N][A][2]
  int* inner_step;                        // [N] SimpleMPE State.step
  int* step_count;                        // [N] JaxMarlState.step (the wrapper's counter)
  uint32_t* key;                          // [N][2]
  EpisodeMetrics m;
};
struct MpCfg { int N, A, L, TLIM; float local_ratio; };

// per-thread LDS rows: positions [2A], velocities [2A], forces [2A] of the env's agents
struct MpLds {
  float* base; int A;
  __device__ float& p(int k) const { return base[k * MP_BLK]; }
  __device__ float& v(int k) const { return base[(k + 2 * A) * MP_BLK]; }
  __device__ float& f(int k) const { return base[(k + 4 * A) * MP_BLK]; }
};

// jax.random.uniform(key, ..., minval, maxval) element i (oracle/prng.py:bits_to_uniform)
__device__ __forceinline__ float mp_uniform(uint32_t k0, uint32_t k1, uint32_t i, float lo, float hi) {
  return fmaxf(lo, uniform01_from_bits(random_bits32(k0, k1, i)) * (hi - lo) + lo);
}

// SimpleMPE.reset: key_a, key_l = split(key); agents uniform in [-1, 1), landmarks in [-0.9, 0.9); velocities 0
__device__ void mp_inner_reset(const MpCfg& c, const MpState& s, long n, const MpLds& m, uint32_t k0, uint32_t k1) {
  const int A = c.A, L = c.L;
  uint32_t a0, a1, l0, l1;
  split_key(k0, k1, a0, a1, l0, l1);
  float* pos = s.pos + n * (long)(A + L) * 2;
  float* vel = s.vel + n * (long)A * 2;
  for (int k = 0; k < 2 * A; ++k) {
    const float x = mp_uniform(a0, a1, (uint32_t)k, -1.f, 1.f);
    pos[k] = x; m.p(k) = x;
    vel[k] = 0.f; m.v(k) = 0.f;
  }
  for (int k = 0; k < 2 * L; ++k) pos[2 * A + k] = mp_uniform(l0, l1, (uint32_t)k, -0.9f, 0.9f);
  s.inner_step[n] = 0;
}

// the wrapper's reset (JaxMarlWrapper.reset): key, reset_key = split(key); the inner reset on reset_key; the counter starts at 0
__device__ void mp_wrapper_reset(const MpCfg& c, const MpState& s, long n, const MpLds& m, uint32_t k0, uint32_t k1) {
  uint32_t nk0, nk1, r0, r1;
  split_key(k0, k1, nk0, nk1, r0, r1);
  mp_inner_reset(c, s, n, m, r0, r1);
  s.key[2 * n] = nk0; s.key[2 * n + 1] = nk1;
  s.step_count[n] = 0;
}

// discrete action -> acceleration (SimpleMPE._decode_discrete_action); the one place a continuous-action variant would change
__device__ __forceinline__ void mp_decode(int a, float& ux, float& uy) {
  ux = 0.f; uy = 0.f;
  if (a < 1 || a >= MP_NACT) return;
  const float u = (a % 2 == 0 ? 1.f : -1.f) * MP_ACCEL;
  if (a <= 2) ux = u; else uy = u;
}

// soft-plus, fp64 and rounded once (see the header)
__device__ __forceinline__ float mp_softplus(float x) {
  const double d = (double)x;
  return (float)(fmax(d, 0.0) + log1p(exp(-fabs(d))));
}

// correctly rounded fp32 square root (v_sqrt_f32, what sqrtf and __fsqrt_rn compile to here, is within 1 ulp): the neighbour of the
// approximation is taken when x lies beyond the square of the midpoint to it; midpoints and their squares are exact in fp64
__device__ __forceinline__ float mp_sqrt(float x) {
  if (!(x > 0.f)) return __builtin_sqrtf(x);
  const float s = __builtin_sqrtf(x);
  const float lo = __uint_as_float(__float_as_uint(s) - 1u), hi = __uint_as_float(__float_as_uint(s) + 1u);
  const double ml = 0.5 * ((double)lo + (double)s), mh = 0.5 * ((double)s + (double)hi), xd = (double)x;
  if (xd < ml * ml) return lo;
  if (xd > mh * mh) return hi;
  return s;
}

__device__ __forceinline__ float mp_dist(float dx, float dy) { return mp_sqrt(dx * dx + dy * dy); }

// observation rows [A][ldo] = [one-hot id | vel, pos, landmarks - pos, other agents - pos (index order, self skipped), comm (zeros)]
__device__ void mp_observe(const MpCfg& c, const MpState& s, long n, const MpLds& m, float* __restrict__ obs, long ldo) {
  const int A = c.A, L = c.L;
  const float* land = s.pos + n * (long)(A + L) * 2 + 2 * A;
  for (int a = 0; a < A; ++a) {
    float* o = obs + a * ldo;
    for (int i = 0; i < A; ++i) o[i] = i == a ? 1.f : 0.f;
    o += A;
    const float px = m.p(2 * a), py = m.p(2 * a + 1);
    o[0] = m.v(2 * a); o[1] = m.v(2 * a + 1); o[2] = px; o[3] = py;
    int j = 4;
    for (int l = 0; l < L; ++l, j += 2) { o[j] = land[2 * l] - px; o[j + 1] = land[2 * l + 1] - py; }
    for (int b = 0; b < A; ++b) {
      if (b == a) continue;
      o[j] = m.p(2 * b) - px; o[j + 1] = m.p(2 * b + 1) - py;
      j += 2;
    }
    for (int k = 0; k < 2 * (A - 1); ++k) o[j + k] = 0.f;
  }
}

__global__ __launch_bounds__(MP_BLK) void k_mpe_reset(MpState s, MpCfg c, const uint32_t* __restrict__ env_keys, float* __restrict__ obs, long ldo,
                                                      int* __restrict__ obs_step) {
  extern __shared__ float mp_lds[];
  long n;
  if (!env_index(c.N, n)) return;
  const MpLds m{mp_lds + threadIdx.x, c.A};
  uint32_t r0, r1;
  metrics_reset(s.m, n, env_keys[2 * n], env_keys[2 * n + 1], r0, r1);
  mp_wrapper_reset(c, s, n, m, r0, r1);
  mp_observe(c, s, n, m, obs + n * (long)c.A * ldo, ldo);
  obs_step[n] = 0;
}

__global__ __launch_bounds__(MP_BLK) void k_mpe_step(MpState s, MpCfg c, const int* __restrict__ actions, int act_stride, StepOut o, int auto_reset) {
  extern __shared__ float mp_lds[];
  long n;
  if (!env_index(c.N, n)) return;
  const MpLds m{mp_lds + threadIdx.x, c.A};
  const int A = c.A, L = c.L;
  float* pos = s.pos + n * (long)(A + L) * 2;
  float* vel = s.vel + n * (long)A * 2;
  const float* land = pos + 2 * A;
  for (int k = 0; k < 2 * A; ++k) { m.p(k) = pos[k]; m.v(k) = vel[k]; }
  // JaxMarlWrapper.step: key, step_key = split(state.key)
  uint32_t k0, k1, sk0, sk1;
  split_key(s.key[2 * n], s.key[2 * n + 1], k0, k1, sk0, sk1);
  s.key[2 * n] = k0; s.key[2 * n + 1] = k1;
  // world step on the pre-step positions
  const float dmin = MP_RAD + MP_RAD;
  for (int i = 0; i < A; ++i) {
    const float px = m.p(2 * i), py = m.p(2 * i + 1);
    float fx = 0.f, fy = 0.f;
    for (int j = 0; j < A; ++j) {
      if (j == i) continue;
      const float dx = px - m.p(2 * j), dy = py - m.p(2 * j + 1);
      const float dist = mp_dist(dx, dy);
      const float pen = mp_softplus(__fdiv_rn(-(dist - dmin), MP_MARGIN)) * MP_MARGIN;
      fx = fx + __fdiv_rn(MP_CONTACT * dx, dist) * pen;
      fy = fy + __fdiv_rn(MP_CONTACT * dy, dist) * pen;
    }
    float ux, uy;
    mp_decode(actions[n * act_stride + i], ux, uy);
    m.f(2 * i) = fx + ux; m.f(2 * i + 1) = fy + uy;
  }
  for (int k = 0; k < 2 * A; ++k) {
    const float v = m.v(k);
    m.p(k) = m.p(k) + v * MP_DT;
    m.v(k) = v * (1.f - MP_DAMP) + m.f(k) * MP_DT;
  }
  // rewards on the post-step state
  float global = 0.f;
  for (int l = 0; l < L; ++l) {
    const float lx = land[2 * l], ly = land[2 * l + 1];
    float best = INFINITY;
    for (int a = 0; a < A; ++a) best = fminf(best, mp_dist(m.p(2 * a) - lx, m.p(2 * a + 1) - ly));
    global = global + (-best);
  }
  const float lr = c.local_ratio, glr = 1.f - c.local_ratio;
  float msum = 0.f;   // episode_metrics.py:91: mean over agents of the per-agent rewards, as a sum in agent order / A in fp32
  for (int i = 0; i < A; ++i) {
    int coll = 0;
    for (int j = 0; j < A; ++j)
      if (j != i) coll += mp_dist(m.p(2 * i) - m.p(2 * j), m.p(2 * i + 1) - m.p(2 * j + 1)) < dmin ? 1 : 0;
    const float r = (float)(-coll) * lr + global * glr;
    o.reward[n * A + i] = r;
    msum = msum + r;
  }
  for (int k = 0; k < 2 * A; ++k) { pos[k] = m.p(k); vel[k] = m.v(k); }
  const int inner = s.inner_step[n];
  const bool done = inner >= c.TLIM;   // tested before the increment: time_limit + 1 steps
  s.inner_step[n] = inner + 1;
  const int wstep = s.step_count[n];
  s.step_count[n] = wstep + 1;
  int obs_step = wstep;                // observation.step_count: the wrapper's counter before its increment (jaxmarl.py:231,241)
  if (done) {
    if (auto_reset) {
      uint32_t a0, a1;
      split_key_first(k0, k1, a0, a1);
      mp_wrapper_reset(c, s, n, m, a0, a1);
      obs_step = 0;
    } else {
      uint32_t r0, r1;
      threefry2x32(sk0, sk1, 0u, 1u, r0, r1);  // MultiAgentEnv.step: key, key_reset = split(step_key); reset on done
      mp_inner_reset(c, s, n, m, r0, r1);
    }
  }
  mp_observe(c, s, n, m, o.obs + n * (long)A * o.ldo, o.ldo);
  o.obs_step[n] = obs_step;
  write_discount_done(o, n, A, done, done);
  metrics_step(s.m, o, n, __fdiv_rn(msum, (float)A), done);
}

}  // namespace magpo

using namespace magpo;

static int mp_cfg(MpCfg& c, int N, int A, int L, int TLIM, float local_ratio, long ldo) {
  c = MpCfg{N, A, L, TLIM, local_ratio};
  if (A < 1 || A > MP_MAXA || L < 1 || L > MP_MAXL || TLIM < 1) {
    set_error("mpe: 1 <= num_agents <= 32, 1 <= num_landmarks <= 32, time_limit >= 1");
    return MAGPO_EINVAL;
  }
  if (ldo < 5 * (long)A + 2 * L) { set_error("mpe: observation rows narrower than 5 num_agents + 2 num_landmarks floats"); return MAGPO_EINVAL; }
  return MAGPO_OK;
}

static size_t mp_lds_bytes(int A) { return (size_t)6 * A * MP_BLK * sizeof(float); }   // 48 KiB at 32 agents

extern "C" int magpo_mpe_reset(float* pos, float* vel, int* inner_step, int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret,
                               int* run_len, float* ep_ret, int* ep_len, int N, int A, int L, int time_limit, float local_ratio,
                               const uint32_t* env_keys, float* obs, long ldo, int* obs_step, hipStream_t st) {
  MpCfg c;
  if (int e = mp_cfg(c, N, A, L, time_limit, local_ratio, ldo)) return e;
  if (int e = env_args(N); e != ENV_LAUNCH) return e;
  MpState s{pos, vel, inner_step, step_count, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  hipLaunchKernelGGL(k_mpe_reset, env_grid(N, MP_BLK), dim3(MP_BLK), mp_lds_bytes(A), st, s, c, env_keys, obs, ldo, obs_step);
  return check_launch("magpo_mpe_reset");
}

extern "C" int magpo_mpe_step(float* pos, float* vel, int* inner_step, int* step_count, uint32_t* key, uint32_t* metrics_key, float* run_ret,
                              int* run_len, float* ep_ret, int* ep_len, int N, int A, int L, int time_limit, float local_ratio, const int* actions,
                              int act_stride, float* reward, float* discount, unsigned char* done, float* obs, long ldo, int* obs_step,
                              float* m_ep_ret, int* m_ep_len, unsigned char* m_term, int auto_reset, hipStream_t st) {
  MpCfg c;
  if (int e = mp_cfg(c, N, A, L, time_limit, local_ratio, ldo)) return e;
  if (int e = env_args(N, A, act_stride, "mpe: act_stride < num_agents"); e != ENV_LAUNCH) return e;
  MpState s{pos, vel, inner_step, step_count, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  StepOut o{reward, discount, done, obs, ldo, obs_step, nullptr, m_ep_ret, m_ep_len, m_term};
  hipLaunchKernelGGL(k_mpe_step, env_grid(N, MP_BLK), dim3(MP_BLK), mp_lds_bytes(A), st, s, c, actions, act_stride, o, auto_reset);
  return check_launch("magpo_mpe_step");
}
