// VectorConnector env + Mava wrappers (VectorConnectorWrapper: the 54-feature vector view, aggregated reward; AgentID, AutoReset,
// RecordEpisodeMetrics; mava/wrappers/jumanji.py:223-241,346-455, mava/utils/make_env.py:64-75,90-135) for gfx950.
// UNPINNED DYNAMICS: the environment (jumanji Connector-v2 and its RandomWalkGenerator) is third-party and absent from the reference
// tree; this kernel and tests/connector_ref.py restate it from memory (every rule and the one documented choice are listed in that
// module's docstring) and are bit-exact with each other.  The observation rules of the wrapper are pinned by the reference tree.
//
// Grid values: agent i has path 3i+1, position 3i+2, target 3i+3; empty is 0.  Rules, in the order the step applies them:
//   * actions NOOP, UP, RIGHT, DOWN, LEFT = (0,0), (-1,0), (0,1), (1,0), (0,-1); anything outside 0..4 is NOOP.  A move is valid if
//     the agent is not connected (position == target) and the new cell is on the grid and EMPTY or its own target.
//   * all agents move at once on the old grid; agents entering one (EMPTY) cell: the highest id wins (jumanji merges the per-agent
//     grids by max) and the others stay where they are (its collision correction).  A winner leaves its path value behind.
//   * per-agent reward 0.1 * newly_connected + (-0.03) * not_connected_before, summed over agents in id order (aggregate_rewards)
//     and repeated for every agent.
//   * mask after the step: NOOP always, a direction iff its move is valid.  Termination (discount 0) when every agent is connected
//     or has no legal direction, or step_count >= time_limit.
//   * generator: key, board_key = split(key); key', step_key = split(board_key); starts = choice(key', G*G, (A,), replace=False);
//     while some agent has an EMPTY neighbour: cur, step_key = split(step_key), keys = split(cur, A), agent i draws a neighbour
//     [up, right, down, left] with choice(keys[i], 4, (), p=EMPTY) and the moves resolve as in a step.  Final cells become targets;
//     the board is rebuilt with the heads on the starts, then the targets on the final cells (an agent that never moved starts
//     connected: its target value owns the cell).
// One thread per env working in place on the env's grid in HBM ([N][G*G] int32, G <= 16).  A step reads a few cells per agent and
// the two 5 x 5 windows of every agent's view: a small latency-bound stream next to the acting kernel.
#include "env_wrappers.hpp"

namespace magpo {

constexpr int CN_NACT = 5, CN_MAXA = 32, CN_MAXG = 16, CN_FOV = 2, CN_NF = 4 + 2 * (2 * CN_FOV + 1) * (2 * CN_FOV + 1);
__constant__ int CN_DR[5] = {0, -1, 0, 1, 0};
__constant__ int CN_DC[5] = {0, 0, 1, 0, -1};

struct CnState {
  int* grid;                          // [N][G*G]
  int* start; int* target; int* pos;  // [N][A][2] (row, col)
  int* step_count;                    // [N]
  uint32_t* key;                      // [N][2]
  EpisodeMetrics m;
};
struct CnCfg { int N, A, G, TLIM; };

// is_valid_position: on the grid and EMPTY or the agent's own target (the caller checks "not connected")
__device__ __forceinline__ bool cn_open(const CnCfg& c, const int* __restrict__ g, int a, int r, int q) {
  if (r < 0 || r >= c.G || q < 0 || q >= c.G) return false;
  const int v = g[r * c.G + q];
  return v == 0 || v == 3 * a + 3;
}

// Simultaneous move of every agent whose cand[a] >= 0 (a flat cell the agent may enter, checked on the old grid): of several agents
// entering one cell the highest id wins; winners leave their path value and take the cell, the others stay.
__device__ __forceinline__ void cn_resolve(const CnCfg& c, int* __restrict__ g, int* __restrict__ pos, const int* cand) {
  for (int a = 0; a < c.A; ++a) {
    if (cand[a] < 0) continue;
    bool win = true;
    for (int b = a + 1; b < c.A; ++b) win &= cand[b] != cand[a];
    if (!win) continue;
    g[pos[2 * a] * c.G + pos[2 * a + 1]] = 3 * a + 1;
    g[cand[a]] = 3 * a + 2;
    pos[2 * a] = cand[a] / c.G;
    pos[2 * a + 1] = cand[a] % c.G;
  }
}

// jax.random.choice(key, n, (num,), replace=False) without p = permutation(key, n)[:num]: for n < 1626 one round (key, sub = split(key);
// stable sort of 0..n-1 by random_bits(sub, n)), so the prefix is the num smallest (bits, index) pairs in order.  num <= CN_MAXA.
__device__ __forceinline__ void cn_perm_prefix(uint32_t k0, uint32_t k1, int n, int num, int* __restrict__ out) {
  uint32_t s0, s1;
  threefry2x32(k0, k1, 0u, 1u, s0, s1);
  uint32_t bb[CN_MAXA];
  int filled = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t b = random_bits32(s0, s1, (uint32_t)i);
    int p = filled;                          // behind every entry with bits <= b (earlier indices win ties)
    for (int a = filled - 1; a >= 0; --a) if (b < bb[a]) p = a;
    if (p >= num) continue;
    const int last = filled < num ? filled : num - 1;
    for (int a = last; a > p; --a) { bb[a] = bb[a - 1]; out[a] = out[a - 1]; }
    bb[p] = b; out[p] = i;
    if (filled < num) ++filled;
  }
}

// RandomWalkGenerator.__call__ (tests/connector_ref.py:_generate); writes the whole env state
__device__ void cn_generate(const CnCfg& c, const CnState& s, long n, uint32_t k0, uint32_t k1) {
  const int A = c.A, G = c.G, GG = G * G;
  int* g = s.grid + n * GG;
  int* pos = s.pos + n * A * 2;
  uint32_t ks0, ks1, b0, b1, st0, st1, kk0, kk1;
  split_key(k0, k1, ks0, ks1, b0, b1);      // key (kept by the state), board_key = split(key)
  split_key(b0, b1, kk0, kk1, st0, st1);    // key, step_key = split(board_key)
  for (int i = 0; i < GG; ++i) g[i] = 0;
  int starts[CN_MAXA], cand[CN_MAXA];
  cn_perm_prefix(kk0, kk1, GG, A, starts);
  for (int a = 0; a < A; ++a) {
    g[starts[a]] = 3 * a + 2;
    pos[2 * a] = starts[a] / G;
    pos[2 * a + 1] = starts[a] % G;
  }
  for (;;) {   // every round with a free neighbour moves at least one agent: at most G*G - A rounds
    bool any = false;
    unsigned freem[CN_MAXA];
    for (int a = 0; a < A; ++a) {
      unsigned m = 0;
      for (int d = 0; d < 4; ++d) {
        const int r = pos[2 * a] + CN_DR[d + 1], q = pos[2 * a + 1] + CN_DC[d + 1];
        if (r >= 0 && r < G && q >= 0 && q < G && g[r * G + q] == 0) m |= 1u << d;
      }
      freem[a] = m;
      any |= m != 0;
    }
    if (!any) break;
    uint32_t c0, c1, n0, n1;
    split_key(st0, st1, c0, c1, n0, n1);   // cur, step_key = split(step_key)
    st0 = n0; st1 = n1;
    for (int a = 0; a < A; ++a) {
      uint32_t a0, a1;
      threefry2x32(c0, c1, 0u, (uint32_t)a, a0, a1);   // keys = split(cur, A)
      const unsigned long long m[4] = {freem[a], 0ull, 0ull, 0ull};
      const int d = choice_mask_cumsum(m, a0, a1);      // an all-zero mask draws neighbour 0, which is then off the grid or taken: no move
      cand[a] = (freem[a] >> d) & 1u ? (pos[2 * a] + CN_DR[d + 1]) * G + pos[2 * a + 1] + CN_DC[d + 1] : -1;
    }
    cn_resolve(c, g, pos, cand);
  }
  int* start = s.start + n * A * 2; int* target = s.target + n * A * 2;
  for (int i = 0; i < GG; ++i) g[i] = 0;
  for (int a = 0; a < A; ++a) {
    target[2 * a] = pos[2 * a]; target[2 * a + 1] = pos[2 * a + 1];
    start[2 * a] = starts[a] / G; start[2 * a + 1] = starts[a] % G;
    g[starts[a]] = 3 * a + 2;
  }
  for (int a = 0; a < A; ++a) {
    g[target[2 * a] * G + target[2 * a + 1]] = 3 * a + 3;
    pos[2 * a] = start[2 * a]; pos[2 * a + 1] = start[2 * a + 1];
  }
  s.step_count[n] = 0;
  s.key[2 * n] = ks0; s.key[2 * n + 1] = ks1;
}

__device__ __forceinline__ bool cn_connected(const int* pos, const int* target, int a) {
  return pos[2 * a] == target[2 * a] && pos[2 * a + 1] == target[2 * a + 1];
}

// observation [A][ldo] f32 = [one-hot id | my_pos / G^2, my_target / G^2, blockers 5x5, targets 5x5] (VectorConnectorWrapper), the
// action mask [A][5] u8; returns whether every agent is connected or blocked
__device__ bool cn_observe(const CnCfg& c, const CnState& s, long n, float* __restrict__ obs, long ldo, unsigned char* __restrict__ mask) {
  const int A = c.A, G = c.G;
  const int* g = s.grid + n * G * G;
  const int* pos = s.pos + n * A * 2; const int* target = s.target + n * A * 2;
  const float size = (float)(G * G);
  bool finished = true;
  for (int a = 0; a < A; ++a) {
    float* o = obs + a * ldo;
    for (int i = 0; i < A; ++i) o[i] = i == a ? 1.f : 0.f;
    o += A;
    // _get_location: the one cell holding the value, (0, 0) when it is on no cell (a connected agent's target; a never-moved head)
    const int pr0 = pos[2 * a], pc0 = pos[2 * a + 1], tr0 = target[2 * a], tc0 = target[2 * a + 1];
    const bool hp = g[pr0 * G + pc0] == 3 * a + 2, ht = g[tr0 * G + tc0] == 3 * a + 3;
    const int pr = hp ? pr0 : 0, pc = hp ? pc0 : 0, tr = ht ? tr0 : 0, tc = ht ? tc0 : 0;
    o[0] = __fdiv_rn((float)pr, size); o[1] = __fdiv_rn((float)pc, size);
    o[2] = __fdiv_rn((float)tr, size); o[3] = __fdiv_rn((float)tc, size);
    int j = 4;
    for (int dr = -CN_FOV; dr <= CN_FOV; ++dr)
      for (int dc = -CN_FOV; dc <= CN_FOV; ++dc) {
        const int rr = pr + dr, cc = pc + dc;
        float blk = 1.f, tgt = 1.f;   // jnp.pad(..., constant_values=True)
        if (rr >= 0 && rr < G && cc >= 0 && cc < G) {
          const int v = g[rr * G + cc], m3 = v % 3;
          blk = m3 == 2 ? 1.f : (m3 == 1 ? -1.f : 0.f);
          tgt = v == 3 * a + 3 ? 1.f : ((m3 == 0 && v != 0) ? -1.f : 0.f);
        }
        o[j] = blk;
        o[j + (2 * CN_FOV + 1) * (2 * CN_FOV + 1)] = tgt;
        ++j;
      }
    const bool conn = cn_connected(pos, target, a);
    unsigned char* m = mask + a * CN_NACT;
    m[0] = 1;
    bool any = false;
    for (int d = 1; d < CN_NACT; ++d) {
      const bool ok = !conn && cn_open(c, g, a, pr0 + CN_DR[d], pc0 + CN_DC[d]);
      m[d] = ok ? 1 : 0;
      any |= ok;
    }
    finished &= conn || !any;
  }
  return finished;
}

__global__ __launch_bounds__(64) void k_connector_reset(CnState s, CnCfg c, const uint32_t* __restrict__ env_keys, float* __restrict__ obs, long ldo,
                                                        int* __restrict__ obs_step, unsigned char* __restrict__ mask) {
  long n;
  if (!env_index(c.N, n)) return;
  uint32_t r0, r1;
  metrics_reset(s.m, n, env_keys[2 * n], env_keys[2 * n + 1], r0, r1);
  cn_generate(c, s, n, r0, r1);
  cn_observe(c, s, n, obs + n * (long)c.A * ldo, ldo, mask + n * (long)c.A * CN_NACT);
  obs_step[n] = 0;
}

__global__ __launch_bounds__(64) void k_connector_step(CnState s, CnCfg c, const int* __restrict__ actions, int act_stride, StepOut o, int auto_reset) {
  long n;
  if (!env_index(c.N, n)) return;
  const int A = c.A, G = c.G;
  int* g = s.grid + n * G * G;
  int* pos = s.pos + n * A * 2; const int* target = s.target + n * A * 2;
  int cand[CN_MAXA];
  unsigned long long was = 0;   // bit a: agent a connected before the step
  for (int a = 0; a < A; ++a) {
    const bool conn = cn_connected(pos, target, a);
    was |= (unsigned long long)conn << a;
    const int k = actions[n * act_stride + a];
    cand[a] = -1;
    if (!conn && k >= 1 && k < CN_NACT) {
      const int r = pos[2 * a] + CN_DR[k], q = pos[2 * a + 1] + CN_DC[k];
      if (cn_open(c, g, a, r, q)) cand[a] = r * G + q;
    }
  }
  cn_resolve(c, g, pos, cand);
  float reward = 0.f;   // aggregate_rewards: the per-agent DenseRewardFn values summed in agent order
  for (int a = 0; a < A; ++a) {
    const float before = (was >> a) & 1ull ? 0.f : 1.f;
    const float newly = (before != 0.f && cn_connected(pos, target, a)) ? 1.f : 0.f;
    reward = __fadd_rn(reward, __fadd_rn(__fmul_rn(0.1f, newly), __fmul_rn(-0.03f, before)));
  }
  const int steps = s.step_count[n] + 1;
  s.step_count[n] = steps;
  float* ob = o.obs + n * (long)A * o.ldo;
  unsigned char* mk = o.mask + n * (long)A * CN_NACT;
  const bool finished = cn_observe(c, s, n, ob, o.ldo, mk);
  const bool done = finished || steps >= c.TLIM;
  int obs_step = steps;
  if (done && auto_reset) {
    uint32_t nk0, nk1;
    split_key_first(s.key[2 * n], s.key[2 * n + 1], nk0, nk1);
    cn_generate(c, s, n, nk0, nk1);
    cn_observe(c, s, n, ob, o.ldo, mk);
    obs_step = 0;
  }
  o.obs_step[n] = obs_step;
  write_team_outputs(o, n, A, reward, done, done);   // all connected / blocked or horizon: termination
  metrics_step(s.m, o, n, team_mean(reward, A), done);
}

}  // namespace magpo

using namespace magpo;

static int cn_cfg(CnCfg& c, int N, int A, int G, int TLIM, long ldo) {
  c = CnCfg{N, A, G, TLIM};
  if (A < 1 || A > CN_MAXA || G < 2 || G > CN_MAXG || A > G * G || TLIM < 1) {
    set_error("connector: 1 <= num_agents <= 32, 2 <= grid_size <= 16, num_agents <= grid_size^2, time_limit >= 1");
    return MAGPO_EINVAL;
  }
  if (ldo < A + CN_NF) { set_error("connector: observation rows narrower than num_agents + 54 floats"); return MAGPO_EINVAL; }
  return MAGPO_OK;
}

extern "C" int magpo_connector_reset(int* grid, int* agent_start, int* agent_target, int* agent_pos, int* step_count, uint32_t* key,
                                     uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int grid_size,
                                     int time_limit, const uint32_t* env_keys, float* obs, long ldo, int* obs_step, unsigned char* mask,
                                     hipStream_t st) {
  CnCfg c;
  if (int e = cn_cfg(c, N, A, grid_size, time_limit, ldo)) return e;
  if (int e = env_args(N); e != ENV_LAUNCH) return e;
  CnState s{grid, agent_start, agent_target, agent_pos, step_count, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  hipLaunchKernelGGL(k_connector_reset, env_grid(N), dim3(ENV_BLOCK), 0, st, s, c, env_keys, obs, ldo, obs_step, mask);
  return check_launch("magpo_connector_reset");
}

extern "C" int magpo_connector_step(int* grid, int* agent_start, int* agent_target, int* agent_pos, int* step_count, uint32_t* key,
                                    uint32_t* metrics_key, float* run_ret, int* run_len, float* ep_ret, int* ep_len, int N, int A, int grid_size,
                                    int time_limit, const int* actions, int act_stride, float* reward, float* discount, unsigned char* done,
                                    float* obs, long ldo, int* obs_step, unsigned char* mask, float* m_ep_ret, int* m_ep_len,
                                    unsigned char* m_term, int auto_reset, hipStream_t st) {
  CnCfg c;
  if (int e = cn_cfg(c, N, A, grid_size, time_limit, ldo)) return e;
  if (int e = env_args(N, A, act_stride, "connector: act_stride < num_agents"); e != ENV_LAUNCH) return e;
  CnState s{grid, agent_start, agent_target, agent_pos, step_count, key, {metrics_key, run_ret, run_len, ep_ret, ep_len}};
  StepOut o{reward, discount, done, obs, ldo, obs_step, mask, m_ep_ret, m_ep_len, m_term};
  hipLaunchKernelGGL(k_connector_step, env_grid(N), dim3(ENV_BLOCK), 0, st, s, c, actions, act_stride, o, auto_reset);
  return check_launch("magpo_connector_step");
}
