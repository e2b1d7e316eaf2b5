// Off-policy half of the recurrent Q-learning system (gfx950): eps-greedy masked sampling, the device-resident trajectory ring
// (add + windowed gather), the double-Q TD loss with its backward, and the target-network update.
//
// Reference: mava/systems/q_learning/anakin/rec_iql.py:210-236 (eps-greedy acting), :238-278 (the stored transition), :330-401 (update_q),
// mava/networks/distributions.py:94-138 (MaskedEpsGreedyDistribution).  UNPINNED: flashbax's trajectory buffer, tfp's
// Categorical(probs).sample and optax's incremental_update / periodic_update are not part of the reference tree; these kernels and
// tests/iql_ref.py restate them and agree bit for bit with each other.
// No atomics; every reduction has a fixed order; everything that changes from env step to env step (the key, the env-step counter, the ring
// cursor) is read from device memory, so a captured rollout replays with static arguments.
#include <cstdio>

#include "common.hpp"
#include "qselect.hpp"

namespace magpo {

// ---- eps-greedy sampling: one thread per (env, agent) row -------------------------------------------------------------------------
struct EpsGreedyArgs {
  const float* q; long ld; const unsigned char* mask;   // Q rows [R][ld], K valid columns; mask [R][K] u8 or NULL
  uint32_t k0, k1; const uint32_t* key_dev;              // key_dev (device, 2 words) overrides k0 / k1
  const int* t; float eps_min, eps_decay;                // env-step counter (device) or NULL = eps 0
  int* action; int* greedy;                              // [R]; greedy nullable
  long R; int K;
};
__global__ void k_eps_greedy(EpsGreedyArgs a) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.R) return;
  // eps = max(eps_min, 1 - (t / eps_decay) * (1 - eps_min)), every operation rounded to fp32 (rec_iql.py:216-218)
  float eps = 0.f;
  if (a.t) eps = fmaxf(a.eps_min, __fsub_rn(1.f, __fmul_rn(__fdiv_rn((float)a.t[0], a.eps_decay), __fsub_rn(1.f, a.eps_min))));
  const uint32_t k0 = a.key_dev ? a.key_dev[0] : a.k0, k1 = a.key_dev ? a.key_dev[1] : a.k1;
  const float* q = a.q + r * a.ld;
  const unsigned char* m = a.mask ? a.mask + r * a.K : nullptr;
  int navail = 0;
  for (int k = 0; k < a.K; ++k) navail += (!m || m[k]) ? 1 : 0;
  const int g = masked_argmax(q, m, a.K);
  const float uni = __fdiv_rn(1.f, (float)navail), keep = __fsub_rn(1.f, eps);
  float best = -INFINITY;
  int arg = 0;
  for (int k = 0; k < a.K; ++k) {
    // probs = eps * mask / n_avail + (1 - eps) * onehot(greedy) (distributions.py:134-136), no contraction
    const float p = __fadd_rn(__fmul_rn(eps, (!m || m[k]) ? uni : 0.f), __fmul_rn(keep, k == g ? 1.f : 0.f));
    if (!(p > 0.f)) continue;   // log(0) = -inf never wins against the greedy action's finite value
    const float lp = (float)log((double)p);   // correctly rounded, like the gumbel
    const float v = gumbel_exact_from_bits(random_bits32(k0, k1, (uint32_t)(r * a.K + k))) + lp;
    if (v > best) { best = v; arg = k; }
  }
  a.action[r] = arg;
  if (a.greedy) a.greedy[r] = g;
}

// ---- trajectory ring: one time ring [N][S] per field ------------------------------------------------------------------------------
struct Ring {
  float* obs; unsigned char* mask; int* action; float* reward;    // [N][S][A][F], [N][S][A][K] (nullable), [N][S][A], [N][S][A]
  unsigned char* terminal; unsigned char* tot;                    // [N][S]
  float* next_obs; unsigned char* next_mask;                      // [N][S][A][F], [N][S][A][K] (nullable)
  int N, S, A, F, K;
};
struct RingStep {   // one env step of the group, as the acting step and the env kernel leave it
  const float* obs; long ldo; const unsigned char* mask; const int* action; const float* reward;
  const unsigned char* terminal; const unsigned char* tot; const float* next_obs; long ldn; const unsigned char* next_mask;
};
// one block per env; the slot is read from the device cursor, which k_ring_advance moves afterwards (a launch of its own: a block of
// this kernel must not see the cursor another block has already moved)
__global__ __launch_bounds__(64) void k_replay_add(Ring g, RingStep s, const int* __restrict__ cursor) {
  const long n = blockIdx.x;
  const int A = g.A, F = g.F, K = g.K;
  int c = cursor[0];
  c = c < 0 ? 0 : (c >= g.S ? g.S - 1 : c);   // (a corrupt cursor must not send the stores out of the ring)
  const long slot = n * g.S + c;
  for (int i = threadIdx.x; i < A * F; i += 64) {
    const int ag = i / F, f = i - ag * F;
    g.obs[slot * A * F + i] = s.obs[(n * A + ag) * s.ldo + f];
    g.next_obs[slot * A * F + i] = s.next_obs[(n * A + ag) * s.ldn + f];
  }
  if (g.mask)
    for (int i = threadIdx.x; i < A * K; i += 64) {
      g.mask[slot * A * K + i] = s.mask[n * A * K + i];
      g.next_mask[slot * A * K + i] = s.next_mask[n * A * K + i];
    }
  for (int i = threadIdx.x; i < A; i += 64) {
    g.action[slot * A + i] = s.action[n * A + i];
    g.reward[slot * A + i] = s.reward[n * A + i];
  }
  if (threadIdx.x == 0) {
    g.terminal[slot] = s.terminal[n] ? 1 : 0;
    g.tot[slot] = s.tot[n] ? 1 : 0;
  }
}
__global__ void k_ring_advance(int* __restrict__ cursor, int* __restrict__ filled, int S) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int c = cursor[0] + 1, f = filled[0] + 1;
  cursor[0] = (c >= S || c < 0) ? 0 : c;
  filled[0] = f > S ? S : f;
}

struct GatherOut {
  float* obs; long ldo; unsigned char* tot; int* action; float* reward;   // rows (b, t, agent), t < L - 1; tot [B][L-1]
  float* next_obs; long ldn; unsigned char* next_mask; unsigned char* next_tot; unsigned char* next_terminal;
};
// flat over max(rows * F, rows * K, rows): element i serves the obs / next_obs copy, and, while in range, one mask byte, one row's
// scalars and one (sequence, step) pair's flags
__global__ void k_replay_gather(Ring g, const int* __restrict__ env_idx, const int* __restrict__ start, int B, int L, GatherOut o) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int A = g.A, F = g.F, K = g.K, T = L - 1;
  const long rows = (long)B * T * A;
  auto slot_of = [&](long bt, int dt) -> long {   // ring slot of step t + dt of window b
    const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
    int n = env_idx[b], s0 = start[b];
    n = n < 0 ? 0 : (n >= g.N ? g.N - 1 : n);     // indices come from device memory: clamp, never read outside the ring
    s0 = ((s0 % g.S) + g.S) % g.S;
    return (long)n * g.S + (s0 + t + dt) % g.S;
  };
  if (i < rows * F) {
    const long r = i / F;
    const int f = (int)(i - r * F), ag = (int)(r % A);
    const long src = (slot_of(r / A, 0) * A + ag) * F + f;
    o.obs[r * o.ldo + f] = g.obs[src];
    o.next_obs[r * o.ldn + f] = g.next_obs[src];
  }
  if (g.next_mask && i < rows * K) {
    const long r = i / K;
    const int k = (int)(i - r * K), ag = (int)(r % A);
    o.next_mask[i] = g.next_mask[(slot_of(r / A, 0) * A + ag) * K + k];
  }
  if (i < rows) {
    const long src = slot_of(i / A, 0) * A + i % A;
    o.action[i] = g.action[src];
    o.reward[i] = g.reward[src];
  }
  if (i < (long)B * T) {
    const long s0 = slot_of(i, 0), s1 = slot_of(i, 1);
    o.tot[i] = g.tot[s0];
    o.next_tot[i] = g.tot[s1];
    o.next_terminal[i] = g.terminal[s1];
  }
}

// all L stored steps of every window (rec_qmix.py:377-395 unrolls over data_full.obs): flat over max(rows * F, rows * K, rows) like
// k_replay_gather, rows = B L A
struct GatherSeqOut {
  float* obs; long ldo; unsigned char* mask; unsigned char* tot; int* action; float* reward;
};
__global__ void k_replay_gather_seq(Ring g, const int* __restrict__ env_idx, const int* __restrict__ start, int B, int L, GatherSeqOut o) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int A = g.A, F = g.F, K = g.K, T = L - 1;
  const long rows = (long)B * L * A;
  auto slot_of = [&](int b, int t) -> long {   // ring slot of step t of window b
    int n = env_idx[b], s0 = start[b];
    n = n < 0 ? 0 : (n >= g.N ? g.N - 1 : n);     // indices come from device memory: clamp, never read outside the ring
    s0 = ((s0 % g.S) + g.S) % g.S;
    return (long)n * g.S + (s0 + t) % g.S;
  };
  if (i < rows * F) {
    const long r = i / F, bt = r / A;
    const int f = (int)(i - r * F), ag = (int)(r - bt * A);
    o.obs[r * o.ldo + f] = g.obs[(slot_of((int)(bt / L), (int)(bt % L)) * A + ag) * F + f];
  }
  if (g.mask && i < rows * K) {
    const long r = i / K, bt = r / A;
    const int k = (int)(i - r * K), ag = (int)(r - bt * A);
    o.mask[i] = g.mask[(slot_of((int)(bt / L), (int)(bt % L)) * A + ag) * K + k];
  }
  if (i < (long)B * L) o.tot[i] = g.tot[slot_of((int)(i / L), (int)(i % L))];
  if (i < (long)B * T * A) {
    const long bt = i / A;
    o.action[i] = g.action[slot_of((int)(bt / T), (int)(bt % T)) * A + i % A];
  }
  if (i < (long)B * T) o.reward[i] = g.reward[slot_of((int)(i / T), (int)(i % T)) * A];   // (every agent column holds the team reward)
}

// jnp.mean(reward, axis=-1) of one env step (rec_qmix.py:287), stored in every agent column: sequential fp32 sum over the agents, then / A
__global__ void k_team_reward(const float* __restrict__ reward, float* __restrict__ out, int N, int A) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int a = 0; a < A; ++a) s = __fadd_rn(s, reward[(long)n * A + a]);
  s = __fdiv_rn(s, (float)A);
  for (int a = 0; a < A; ++a) out[(long)n * A + a] = s;
}

// ---- double-Q TD loss (rec_iql.py:366-377, :299-328): 16 lanes per row, 4 gradient columns per lane ------------------------------------
struct TdArgs {
  const float* q; const float* qn_online; const float* qn_target; long ld;
  const int* action; const unsigned char* next_mask; const float* reward; const unsigned char* next_terminal;
  float* dq; long lddq; double* part; long R; int K, A; float gamma, two_inv_R;
};
__global__ __launch_bounds__(256) void k_q_td_loss(TdArgs a) {
  __shared__ double sh[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, c4 = 4 * l16;
  double acc[3] = {0.0, 0.0, 0.0};   // (the scalars are means of signed terms: summed in double from the first term on)
  const long nrow4 = (a.R + 3) / 4;
  for (long base = (long)blockIdx.x * 4 + wave; base < nrow4; base += (long)gridDim.x * 4) {
    const long r = base * 4 + (lane >> 4);
    if (r >= a.R) continue;
    // (the 16 lanes of a row form the same scalars from the same loads: no exchange between lanes is needed)
    const int na = masked_argmax(a.qn_online + r * a.ld, a.next_mask ? a.next_mask + r * a.K : nullptr, a.K);
    int act = a.action[r];
    act = act < 0 ? 0 : (act >= a.K ? a.K - 1 : act);   // (a gather with an out-of-range index clamps)
    const float term = a.next_terminal[r / a.A] ? 1.f : 0.f;
    const float target = __fadd_rn(a.reward[r], __fmul_rn(__fmul_rn(__fsub_rn(1.f, term), a.gamma), a.qn_target[r * a.ld + na]));
    const float qs = a.q[r * a.ld + act];
    const float err = __fsub_rn(qs, target);
    const float gq = __fmul_rn(a.two_inv_R, err);
    if (c4 + 3 < a.lddq) {   // lddq is a multiple of 4: a whole float4 or nothing; columns up to min(lddq, 64)
      float4 og;
      og.x = c4 == act ? gq : 0.f; og.y = c4 + 1 == act ? gq : 0.f; og.z = c4 + 2 == act ? gq : 0.f; og.w = c4 + 3 == act ? gq : 0.f;
      *reinterpret_cast<float4*>(a.dq + r * a.lddq + c4) = og;
    }
    if (l16 == 0) { acc[0] += (double)err * (double)err; acc[1] += (double)qs; acc[2] += (double)target; }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double w = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if (lane == 0) sh[q][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) a.part[8 * blockIdx.x + threadIdx.x] = (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}
// out: [q_loss, mean_q, mean_target]
__global__ void k_q_td_final(const double* __restrict__ part, int nb, double inv_R, float* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  double s[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) s[q] = wave_sum_strided(part, nb, 8, q);
  if (threadIdx.x != 0) return;
  out[0] = (float)(s[0] * inv_R); out[1] = (float)(s[1] * inv_R); out[2] = (float)(s[2] * inv_R);
}

// ---- target network ---------------------------------------------------------------------------------------------------------------
__global__ void k_target_update(const float* __restrict__ online, float* __restrict__ target, long n, int mode, float tau,
                                const int* __restrict__ t_train, int period) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode == 0) {   // optax.incremental_update: tau * new + (1 - tau) * old, two products and one sum, none contracted
    target[i] = __fadd_rn(__fmul_rn(tau, online[i]), __fmul_rn(__fsub_rn(1.f, tau), target[i]));
  } else if (t_train[0] % period == 0) {   // optax.periodic_update
    target[i] = online[i];
  }
}

}  // namespace magpo

using namespace magpo;

extern "C" int magpo_eps_greedy_sample(const float* q, long ld, const unsigned char* mask, uint32_t k0, uint32_t k1,
                                       const uint32_t* key_dev, const int* t_dev, float eps_min, float eps_decay, int* action,
                                       int* greedy, long R, int K, hipStream_t st) {
  if (R < 0 || K < 1 || K > 32 || ld < K || !q || !action) {
    set_error("eps_greedy_sample: need R >= 0, 1 <= K <= 32, ld >= K, q and action not NULL");
    return MAGPO_EINVAL;
  }
  if (R * K >= (1L << 32)) { set_error("eps_greedy_sample: R*K must be < 2^32"); return MAGPO_EINVAL; }
  if (t_dev && (!(eps_decay > 0.f) || !(eps_min >= 0.f) || !(eps_min <= 1.f))) {
    set_error("eps_greedy_sample: need eps_decay > 0 and 0 <= eps_min <= 1");
    return MAGPO_EINVAL;
  }
  if (R == 0) return MAGPO_OK;
  EpsGreedyArgs a{q, ld, mask, k0, k1, key_dev, t_dev, eps_min, eps_decay, action, greedy, R, K};
  hipLaunchKernelGGL(k_eps_greedy, dim3((unsigned)((R + 127) / 128)), dim3(128), 0, st, a);
  return check_launch("magpo_eps_greedy_sample");
}

static int ring_check(const char* who, const Ring& g) {
  static thread_local char msg[160];
  const char* bad = nullptr;
  if (g.N < 1 || g.S < 1 || g.A < 1 || g.F < 1 || g.K < 1) bad = "need N, buffer_size, A, F, K >= 1";
  else if (!g.obs || !g.action || !g.reward || !g.terminal || !g.tot || !g.next_obs) bad = "a ring field is NULL";
  else if ((g.mask == nullptr) != (g.next_mask == nullptr)) bad = "mask and next_mask rings must both be given or both be NULL";
  if (!bad) return MAGPO_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, bad);
  set_error(msg);
  return MAGPO_EINVAL;
}

extern "C" int magpo_replay_add(float* r_obs, unsigned char* r_mask, int* r_action, float* r_reward, unsigned char* r_terminal,
                                unsigned char* r_tot, float* r_next_obs, unsigned char* r_next_mask, int* cursor, int* filled,
                                int N, int S, int A, int F, int K, const float* obs, long ldo, const unsigned char* mask,
                                const int* action, const float* reward, const unsigned char* terminal, const unsigned char* tot,
                                const float* next_obs, long ldn, const unsigned char* next_mask, hipStream_t st) {
  Ring g{r_obs, r_mask, r_action, r_reward, r_terminal, r_tot, r_next_obs, r_next_mask, N, S, A, F, K};
  if (int e = ring_check("replay_add", g)) return e;
  if (!cursor || !filled || !obs || !action || !reward || !terminal || !tot || !next_obs || ldo < F || ldn < F) {
    set_error("replay_add: cursor, filled and the step's fields must not be NULL, and row strides must be >= F");
    return MAGPO_EINVAL;
  }
  if (r_mask && (!mask || !next_mask)) { set_error("replay_add: the ring stores masks but the step has none"); return MAGPO_EINVAL; }
  RingStep s{obs, ldo, mask, action, reward, terminal, tot, next_obs, ldn, next_mask};
  hipLaunchKernelGGL(k_replay_add, dim3((unsigned)N), dim3(64), 0, st, g, s, (const int*)cursor);
  hipLaunchKernelGGL(k_ring_advance, dim3(1), dim3(1), 0, st, cursor, filled, S);
  return check_launch("magpo_replay_add");
}

extern "C" int magpo_replay_gather(const float* r_obs, const unsigned char* r_mask, const int* r_action, const float* r_reward,
                                   const unsigned char* r_terminal, const unsigned char* r_tot, const float* r_next_obs,
                                   const unsigned char* r_next_mask, int N, int S, int A, int F, int K, const int* env_idx,
                                   const int* start, int B, int L, float* o_obs, long ldo, unsigned char* o_tot, int* o_action,
                                   float* o_reward, float* o_next_obs, long ldn, unsigned char* o_next_mask,
                                   unsigned char* o_next_tot, unsigned char* o_next_terminal, hipStream_t st) {
  Ring g{const_cast<float*>(r_obs), const_cast<unsigned char*>(r_mask), const_cast<int*>(r_action), const_cast<float*>(r_reward),
         const_cast<unsigned char*>(r_terminal), const_cast<unsigned char*>(r_tot), const_cast<float*>(r_next_obs),
         const_cast<unsigned char*>(r_next_mask), N, S, A, F, K};
  if (int e = ring_check("replay_gather", g)) return e;
  if (B < 1 || L < 2 || L > S) { set_error("replay_gather: need B >= 1 and 2 <= L <= buffer_size"); return MAGPO_EINVAL; }
  if (!env_idx || !start || !o_obs || !o_tot || !o_action || !o_reward || !o_next_obs || !o_next_tot || !o_next_terminal || ldo < F || ldn < F
      || (r_next_mask && !o_next_mask)) {
    set_error("replay_gather: indices and outputs must not be NULL (next_mask where the ring has one), and row strides must be >= F");
    return MAGPO_EINVAL;
  }
  GatherOut o{o_obs, ldo, o_tot, o_action, o_reward, o_next_obs, ldn, o_next_mask, o_next_tot, o_next_terminal};
  const long rows = (long)B * (L - 1) * A, n = rows * (F > K ? F : K);
  hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, env_idx, start, B, L, o);
  return check_launch("magpo_replay_gather");
}

extern "C" int magpo_replay_gather_seq(const float* r_obs, const unsigned char* r_mask, const int* r_action, const float* r_reward,
                                       const unsigned char* r_terminal, const unsigned char* r_tot, const float* r_next_obs,
                                       const unsigned char* r_next_mask, int N, int S, int A, int F, int K, const int* env_idx,
                                       const int* start, int B, int L, float* o_obs, long ldo, unsigned char* o_mask,
                                       unsigned char* o_tot, int* o_action, float* o_reward, hipStream_t st) {
  Ring g{const_cast<float*>(r_obs), const_cast<unsigned char*>(r_mask), const_cast<int*>(r_action), const_cast<float*>(r_reward),
         const_cast<unsigned char*>(r_terminal), const_cast<unsigned char*>(r_tot), const_cast<float*>(r_next_obs),
         const_cast<unsigned char*>(r_next_mask), N, S, A, F, K};
  if (int e = ring_check("replay_gather_seq", g)) return e;
  if (B < 1 || L < 2 || L > S) { set_error("replay_gather_seq: need B >= 1 and 2 <= L <= buffer_size"); return MAGPO_EINVAL; }
  if (!env_idx || !start || !o_obs || !o_tot || !o_action || !o_reward || ldo < F || (r_mask && !o_mask)) {
    set_error("replay_gather_seq: indices and outputs must not be NULL (mask where the ring has one), and the row stride must be >= F");
    return MAGPO_EINVAL;
  }
  GatherSeqOut o{o_obs, ldo, o_mask, o_tot, o_action, o_reward};
  const long rows = (long)B * L * A, n = rows * (F > K ? F : K);
  hipLaunchKernelGGL(k_replay_gather_seq, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, env_idx, start, B, L, o);
  return check_launch("magpo_replay_gather_seq");
}

extern "C" int magpo_team_reward(const float* reward, float* out, int N, int A, hipStream_t st) {
  if (N < 1 || A < 1 || !reward || !out) { set_error("team_reward: need N, A >= 1, reward and out not NULL"); return MAGPO_EINVAL; }
  hipLaunchKernelGGL(k_team_reward, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, st, reward, out, N, A);
  return check_launch("magpo_team_reward");
}

// workspace: >= 8 * 1024 doubles (as magpo_ppo_loss_fwd_bwd)
extern "C" int magpo_q_td_loss(const float* q_online, const float* q_online_next, const float* q_target_next, long ld,
                               const int* action, const unsigned char* next_mask, const float* reward,
                               const unsigned char* next_terminal, float gamma, float* dq, long lddq, double* workspace,
                               float* loss_out, long R, int K, int A, hipStream_t st) {
  if (R < 1 || K < 1 || K > 32 || A < 1 || R % A || K > ld || K > lddq || (lddq & 3)) {
    set_error("q_td_loss: need R >= 1 a multiple of A >= 1, 1 <= K <= 32, K <= strides, gradient stride a multiple of 4");
    return MAGPO_EINVAL;
  }
  if (!q_online || !q_online_next || !q_target_next || !action || !reward || !next_terminal || !dq || !workspace || !loss_out) {
    set_error("q_td_loss: only next_mask may be NULL");
    return MAGPO_EINVAL;
  }
  int nb = (int)((R + 15) / 16);
  if (nb > 1024) nb = 1024;
  TdArgs a{q_online, q_online_next, q_target_next, ld, action, next_mask, reward, next_terminal, dq, lddq, workspace, R, K, A, gamma,
           2.0f / (float)R};
  hipLaunchKernelGGL(k_q_td_loss, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_q_td_final, dim3(1), dim3(64), 0, st, workspace, nb, 1.0 / (double)R, loss_out);
  return check_launch("magpo_q_td_loss");
}

extern "C" int magpo_target_update(const float* online, float* target, long n, int mode, float tau, const int* t_train,
                                   int update_period, hipStream_t st) {
  if (n < 0 || !online || !target || (mode != 0 && mode != 1)) {
    set_error("target_update: need n >= 0, online and target not NULL, mode 0 (incremental) or 1 (periodic)");
    return MAGPO_EINVAL;
  }
  if (mode == 1 && (!t_train || update_period < 1)) {
    set_error("target_update: the periodic mode needs the device counter t_train and update_period >= 1");
    return MAGPO_EINVAL;
  }
  if (n == 0) return MAGPO_OK;
  hipLaunchKernelGGL(k_target_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, online, target, n, mode, tau, t_train, update_period);
  return check_launch("magpo_target_update");
}
