// Stateless retention over independent teams on fp32 MFMA for gfx950: the memoryless Sable (ff_sable).
//
// Reference semantics: SimpleRetention.__call__ with memory_config.type == "ff_sable" (mava/networks/retention.py:79-84, 94-99) on a zero
// hidden state: a team of A consecutive token rows is one sequence,
//   r_i = sum_j M_ij (q_i . k_j) v_j ,   M_ij = [j <= i] when masked, else 1
// with no decay matrix, no xi and no carried state.  Nothing but the operands is read and nothing but r (or dq | dk | dv) is written:
// there is no state buffer and no workspace.
//
// One wave per 32-token tile of floor(32 / A) whole teams; a workgroup is four independent waves (they share one 32-entry table of where
// the tokens of a tile sit, see tr_build_tab).  Every product runs on
// v_mfma_f32_32x32x2_f32 and the block-diagonal (+ causal) mask is applied to the accumulator in registers:
//   P^T = K Q^T     A / B operands are the lanes' own rows of k / q (lane = row, the two lane halves alternate float4 groups of the
//                   feature axis -- both operands use the same feature order, which a dot product does not care about);
//                   the result has its column i on the lane and its rows j in the 16 registers
//   r   = (P^T)^T V the masked accumulator IS the next A operand (register s of lane half h is row j(s, h) = 4 h + (s & 3) + 8 (s >> 2)),
//                   the B operand V[j(s, h)][c] is one coalesced dword load per step: no LDS and no transpose.
// The backward builds P (lane = j), dP (lane = j) and dP^T (lane = i) the same way -- three products instead of one transposed copy --
// so that dv = P^T dr, dk = dP^T q and dq = (dP^T)^T k all sum over the register (row) index of their accumulator.
#include "common.hpp"

namespace magpo {

// row of accumulator register s in lane half h (cdna MFMA 32x32 C/D layout)
__device__ __forceinline__ int tr_acc_row(int s, int h) { return (s & 3) + 8 * (s >> 2) + 4 * h; }

// Where the tokens of a tile sit.  The products over tokens visit the tile rows in the fixed order S = 0, 4, 8, 12, 1, 5, 9, 13, ... (rows
// 16 g + c + 4 t at position 16 g + 4 c + t: the k order of the chunk kernels' 16x16x4 products, retention32.hpp: mma16), and a team's sum has to
// take its agents in that same order whatever the team's place in the tile.  So agent a of the tile's team t sits at row S[rank(a) * tpt + t],
// rank(a) = the position of a among the agents < A in the order S: along S the rows of one team then follow each other as the agents of a
// lone team at rows 0 .. A - 1 do.  tab[row] = (t << 8) | a, or -1 for a row no token sits at; the same for every tile of a launch.
__device__ __forceinline__ int tr_seq(int m) { return 16 * (m >> 4) + ((m >> 2) & 3) + 4 * (m & 3); }   // S[m]; an involution: position of row m
__device__ __forceinline__ void tr_build_tab(int* __restrict__ tab, int A) {
  if (threadIdx.x < 32) {
    const int tpt = 32 / A, n = tr_seq(threadIdx.x), rank = n / tpt, t = n - rank * tpt;
    int a = -1, seen = 0;
    for (int m = 0; m < 32; ++m) {
      const int cand = tr_seq(m);
      if (cand < A) {
        if (seen == rank) a = cand;
        ++seen;
      }
    }
    tab[threadIdx.x] = (rank < A && a >= 0) ? ((t << 8) | a) : -1;
  }
  __syncthreads();
}
// row offset (t A + a) inside the tile's block of rows, or -1: the token must exist (team t among the tile's nt teams)
__device__ __forceinline__ int tr_off(int e, int A, int nt) { return (e >= 0 && (e >> 8) < nt) ? (e >> 8) * A + (e & 255) : -1; }

// features f .. f+3 of the token at row offset off (off < 0 and features >= hs read as zero; the load itself is clamped to row 0 / feature 0)
template <bool VEC>
__device__ __forceinline__ float4 tr_row4(const float* __restrict__ base, long ld, int off, int f, int hs) {
  const bool ok = off >= 0;
  const float* rp = base + (long)(ok ? off : 0) * ld;
  if (VEC) {   // hs % 4 == 0, 16-B aligned rows
    const bool in = ok && f < hs;
    const float4 v = *reinterpret_cast<const float4*>(rp + (in ? f : 0));
    return in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float x[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = ok && f + e < hs;
    const float t = rp[in ? f + e : 0];
    x[e] = in ? t : 0.f;
  }
  return make_float4(x[0], x[1], x[2], x[3]);
}
// element c of the token at row offset off, zero outside
__device__ __forceinline__ float tr_col(const float* __restrict__ base, long ld, int off, int c, int hs) {
  const bool in = off >= 0 && c < hs;
  const float t = base[(long)(in ? off : 0) * ld + (in ? c : 0)];
  return in ? t : 0.f;
}
struct TrFrag { float4 v[8]; };
template <bool VEC>
__device__ __forceinline__ void tr_load_frag(TrFrag& f, const float* __restrict__ base, long ld, int off, int h, int hs, int U) {
#pragma unroll
  for (int u = 0; u < 8; ++u) f.v[u] = u < U ? tr_row4<VEC>(base, ld, off, 8 * u + 4 * h, hs) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// acc += X Y^T over the feature axis: both operands row-per-lane fragments in the same feature order.  The order of the steps -- features
// 16 g + c + {0, 4, 8, 12} for c = 0..3, g = 0..3, two per instruction -- is the k order of the chunk kernels' 16x16x4 products
// (retention32.hpp: mma16), so that on equal inputs the two families add the same products in the same order.
__device__ __forceinline__ void tr_mma_rr(f32x16& acc, const TrFrag& a, const TrFrag& b, int U) {
#define TR_STEP(u, c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[u].c, b.v[u].c, acc, 0, 0, 0)
#pragma unroll
  for (int g = 0; g < 4; ++g)
    if (2 * g < U) {   // (fragment 2 g + 1 is zero when the head ends inside this group)
      TR_STEP(2 * g, x); TR_STEP(2 * g + 1, x);
      TR_STEP(2 * g, y); TR_STEP(2 * g + 1, y);
      TR_STEP(2 * g, z); TR_STEP(2 * g + 1, z);
      TR_STEP(2 * g, w); TR_STEP(2 * g + 1, w);
    }
#undef TR_STEP
}
// out[n][c] = sum_m X[m][n] B[m][c] for c = 32 cb + lane: X is an accumulator (column n on the lane, rows m in the registers); offs[s] = row
// offset of the token at this lane half's row of register s
__device__ __forceinline__ f32x16 tr_mma_xt(const f32x16& x, const float* __restrict__ b, long ldb, const int (&offs)[16], int c, int hs) {
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
  for (int n = 0; n < 16; ++n) {   // tile rows in the order S: 16 g + c + {0, 4 | 8, 12}
    const int s = ((n >> 1) & 3) + 4 * (2 * (n >> 3) + (n & 1));
    o = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s], tr_col(b, ldb, offs[s], c, hs), o, 0, 0, 0);
  }
  return o;
}

struct TeamTile {
  long row0;   // first token row (0 for a tile beyond the last team: its clamped loads then stay inside the buffers)
  int nt;      // teams in the tile
};
__device__ __forceinline__ TeamTile tr_tile(long nteams, int A) {
  const int tpt = 32 / A;
  const long team0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * tpt;
  long nt = nteams - team0;
  nt = nt < 0 ? 0 : (nt > tpt ? tpt : nt);
  TeamTile t;
  t.nt = (int)nt;
  t.row0 = nt ? team0 * A : 0;
  return t;
}
// (team, agent) entries of this lane's own row and of its 16 register rows; pair (i, j) is inside the product when both tokens exist, belong to
// one team, j is among the first ntok agents and -- masked -- not behind i
struct TrRows { int mine, reg[16]; };
__device__ __forceinline__ void tr_rows(TrRows& r, const int* __restrict__ tab, int lr, int h, int nt) {
  const int e = tab[lr];
  r.mine = (e >= 0 && (e >> 8) < nt) ? e : -1;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int x = tab[tr_acc_row(s, h)];
    r.reg[s] = (x >= 0 && (x >> 8) < nt) ? x : -1;
  }
}
__device__ __forceinline__ bool tr_on(int ei, int ej, int ntok, int masked) {
  return ei >= 0 && ej >= 0 && (ei >> 8) == (ej >> 8) && (ej & 255) < ntok && !(masked && (ej & 255) > (ei & 255));
}

struct TeamFwdArgs {
  const float* q; const float* k; const float* v; long ldq, ldk, ldv;
  float* r; long ldr;
  long nteams; int A, ntok, ret_from, masked, hs;
  const float* gp; long ldg; const float* gamma; const float* beta; int gs;   // EPI only
};

template <bool VEC, bool EPI>
__global__ __launch_bounds__(256) void k_team_ret_fwd(TeamFwdArgs a) {
  __shared__ int tab[32];
  const int lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
  const TeamTile t = tr_tile(a.nteams, a.A);
  const int A = a.A, hs = a.hs, U = (hs + 7) >> 3;
  tr_build_tab(tab, A);
  TrRows rw;
  tr_rows(rw, tab, lr, h, t.nt);
  const int myoff = (rw.mine & 255) < a.ntok ? tr_off(rw.mine, A, t.nt) : -1;
  int offs[16];   // rows of agents >= ntok are not part of the call: never stored, and their v rows (not written yet while acting) never read
#pragma unroll
  for (int s = 0; s < 16; ++s) offs[s] = (rw.reg[s] & 255) < a.ntok ? tr_off(rw.reg[s], A, t.nt) : -1;
  const float* qb = a.q + t.row0 * a.ldq;
  const float* kb = a.k + t.row0 * a.ldk;
  const float* vb = a.v + t.row0 * a.ldv;
  f32x16 pt;   // P^T: lane = query row i, registers = key rows j
#pragma unroll
  for (int i = 0; i < 16; ++i) pt[i] = 0.f;
  {
    TrFrag kf, qf;
    tr_load_frag<VEC>(kf, kb, a.ldk, myoff, h, hs, U);
    tr_load_frag<VEC>(qf, qb, a.ldq, myoff, h, hs, U);
    tr_mma_rr(pt, kf, qf, U);
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) pt[s] = tr_on(rw.mine, rw.reg[s], a.ntok, a.masked) ? pt[s] : 0.f;
  if (!EPI) {
    const int ncb = (hs + 31) >> 5;
    for (int cb = 0; cb < ncb; ++cb) {
      const int c = 32 * cb + lr;
      const f32x16 o = tr_mma_xt(pt, vb, a.ldv, offs, c, hs);
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int ai = rw.reg[s] & 255;
        if (offs[s] >= 0 && ai >= a.ret_from && ai < a.ntok && c < hs) a.r[(t.row0 + offs[s]) * a.ldr + c] = o[s];
      }
    }
  } else {
    // fused retention epilogue (retention.py:289-294), as magpo_retention_recurrent's: u = swish(gpre) * GroupNorm(ret) on rows of hs
    // channels in groups of gs; the tile goes through LDS once so that a row's channels lie on the lanes
    __shared__ float ot[4][32][64 + LDP];
    float (*o_t)[64 + LDP] = ot[threadIdx.x >> 6];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const f32x16 o = tr_mma_xt(pt, vb, a.ldv, offs, 32 * cb + lr, hs);   // columns >= hs: zero
#pragma unroll
      for (int s = 0; s < 16; ++s) o_t[tr_acc_row(s, h)][32 * cb + lr] = o[s];
    }
    __syncthreads();
    for (int i = 0; i < 32; ++i) {
      const int e = tab[i], off = tr_off(e, A, t.nt), ai = e & 255;
      if (off < 0 || ai < a.ret_from || ai >= a.ntok) continue;
      const float x = o_t[i][lane];
      float s1 = x, s2 = x * x;
      for (int o = a.gs >> 1; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
      const float mu = s1 / (float)a.gs, m2 = s2 / (float)a.gs;
      const float rstd = rsqrtf(fmaxf(m2 - mu * mu, 0.f) + 1e-6f);
      if (lane < hs) {
        const float rn = (x - mu) * rstd * a.gamma[lane] + a.beta[lane];
        a.r[(t.row0 + off) * a.ldr + lane] = swishf_(a.gp[(t.row0 + off) * a.ldg + lane]) * rn;
      }
    }
  }
}

struct TeamBwdArgs {
  const float* q; const float* k; const float* v; long ldq, ldk, ldv;
  const float* dr; long lddr;
  float* dq; float* dk; float* dv; long lddq, lddk, lddv;
  long nteams; int A, masked, hs;
};

// the tokens of an accumulator's register rows, columns c < hs (column c on the lane), to out
__device__ __forceinline__ void tr_store(float* __restrict__ out, long ld, const f32x16& o, const int (&offs)[16], int c, int hs) {
#pragma unroll
  for (int s = 0; s < 16; ++s)
    if (offs[s] >= 0 && c < hs) out[(long)offs[s] * ld + c] = o[s];
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_team_ret_bwd(TeamBwdArgs a) {
  __shared__ int tab[32];
  const int lane = threadIdx.x & 63, lr = lane & 31, h = lane >> 5;
  const TeamTile t = tr_tile(a.nteams, a.A);
  const int A = a.A, hs = a.hs, U = (hs + 7) >> 3;
  tr_build_tab(tab, A);
  TrRows rw;
  tr_rows(rw, tab, lr, h, t.nt);
  const int myoff = tr_off(rw.mine, A, t.nt);
  int offs[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) offs[s] = tr_off(rw.reg[s], A, t.nt);
  const float* qb = a.q + t.row0 * a.ldq;
  const float* kb = a.k + t.row0 * a.ldk;
  const float* vb = a.v + t.row0 * a.ldv;
  const float* db = a.dr + t.row0 * a.lddr;
  f32x16 p, dp, dpt;   // P, dP: lane = key row j, registers = query rows i;  dP^T: lane = i, registers = j
#pragma unroll
  for (int i = 0; i < 16; ++i) { p[i] = 0.f; dp[i] = 0.f; dpt[i] = 0.f; }
  {
    TrFrag qf, kf;
    tr_load_frag<VEC>(qf, qb, a.ldq, myoff, h, hs, U);
    tr_load_frag<VEC>(kf, kb, a.ldk, myoff, h, hs, U);
    tr_mma_rr(p, qf, kf, U);        // Q K^T
  }
  {
    TrFrag df, vf;
    tr_load_frag<VEC>(df, db, a.lddr, myoff, h, hs, U);
    tr_load_frag<VEC>(vf, vb, a.ldv, myoff, h, hs, U);
    tr_mma_rr(dp, df, vf, U);       // dR V^T
    tr_mma_rr(dpt, vf, df, U);      // V dR^T
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const bool on_p = tr_on(rw.reg[s], rw.mine, A, a.masked);   // (i, j) = (register row, lane)
    const bool on_t = tr_on(rw.mine, rw.reg[s], A, a.masked);   // (i, j) = (lane, register row)
    p[s] = on_p ? p[s] : 0.f;
    dp[s] = on_p ? dp[s] : 0.f;
    dpt[s] = on_t ? dpt[s] : 0.f;
  }
  const int ncb = (hs + 31) >> 5;
  for (int cb = 0; cb < ncb; ++cb) {
    const int c = 32 * cb + lr;
    tr_store(a.dv + t.row0 * a.lddv, a.lddv, tr_mma_xt(p, db, a.lddr, offs, c, hs), offs, c, hs);     // dv = P^T dR
    tr_store(a.dk + t.row0 * a.lddk, a.lddk, tr_mma_xt(dp, qb, a.ldq, offs, c, hs), offs, c, hs);     // dk = dP^T Q
    tr_store(a.dq + t.row0 * a.lddq, a.lddq, tr_mma_xt(dpt, kb, a.ldk, offs, c, hs), offs, c, hs);    // dq = dP K
  }
}

}  // namespace magpo

using namespace magpo;

static bool tr_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int tr_check_shape(const char* what, long nteams, int A, int hs) {
  if (nteams < 0 || A < 1 || A > 32 || hs < 1 || hs > 64) {
    set_error(what);
    return MAGPO_EINVAL;
  }
  const long tiles = (nteams + 32 / A - 1) / (32 / A);
  if ((tiles + 3) / 4 > 0x7fffffffL) { set_error("team_retention: too many teams for one launch"); return MAGPO_EINVAL; }
  return MAGPO_OK;
}

extern "C" int magpo_team_retention_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* r, long ldr,
                                        long nteams, int A, int ntok, int ret_from, int masked, int hs, const float* gp, long ldg,
                                        const float* gamma, const float* beta, int gs, hipStream_t st) {
  if (!q || !k || !v || !r) { set_error("team_retention_fwd: q, k, v and r must not be null"); return MAGPO_EINVAL; }
  if (int e = tr_check_shape("team_retention_fwd: need nteams >= 0, 1 <= A <= 32, 1 <= hs <= 64", nteams, A, hs)) return e;
  if (ntok < 1 || ntok > A || ret_from < 0 || ret_from >= ntok) { set_error("team_retention_fwd: need 1 <= ntok <= A, 0 <= ret_from < ntok"); return MAGPO_EINVAL; }
  if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldr & 3)) { set_error("team_retention_fwd: row strides must be multiples of 4 floats"); return MAGPO_EINVAL; }
  if (gp) {
    if (!gamma || !beta) { set_error("team_retention_fwd: the fused epilogue needs gamma and beta"); return MAGPO_EINVAL; }
    if ((ldg & 3) || gs < 1 || gs > hs || (gs & (gs - 1)) || hs % gs) { set_error("team_retention_fwd: bad gate stride / group size"); return MAGPO_EINVAL; }
  }
  if (nteams == 0) return MAGPO_OK;
  TeamFwdArgs a{q, k, v, ldq, ldk, ldv, r, ldr, nteams, A, ntok, ret_from, masked ? 1 : 0, hs, gp, ldg, gamma, beta, gs};
  const long tiles = (nteams + 32 / A - 1) / (32 / A);
  const dim3 grid((unsigned)((tiles + 3) / 4));
  const bool vec = !(hs & 3) && tr_aligned(q) && tr_aligned(k);
  if (gp) {
    if (vec) hipLaunchKernelGGL((k_team_ret_fwd<true, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_team_ret_fwd<false, true>), grid, dim3(256), 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_team_ret_fwd<true, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_team_ret_fwd<false, false>), grid, dim3(256), 0, st, a);
  }
  return check_launch("magpo_team_retention_fwd");
}

extern "C" int magpo_team_retention_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* dr, long lddr,
                                        float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, long nteams, int A, int masked,
                                        int hs, hipStream_t st) {
  if (!q || !k || !v || !dr || !dq || !dk || !dv) { set_error("team_retention_bwd: q, k, v, dr, dq, dk and dv must not be null"); return MAGPO_EINVAL; }
  if (int e = tr_check_shape("team_retention_bwd: need nteams >= 0, 1 <= A <= 32, 1 <= hs <= 64", nteams, A, hs)) return e;
  if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (lddr & 3) || (lddq & 3) || (lddk & 3) || (lddv & 3)) {
    set_error("team_retention_bwd: row strides must be multiples of 4 floats");
    return MAGPO_EINVAL;
  }
  if (nteams == 0) return MAGPO_OK;
  TeamBwdArgs a{q, k, v, ldq, ldk, ldv, dr, lddr, dq, dk, dv, lddq, lddk, lddv, nteams, A, masked ? 1 : 0, hs};
  const long tiles = (nteams + 32 / A - 1) / (32 / A);
  const dim3 grid((unsigned)((tiles + 3) / 4));
  if (!(hs & 3) && tr_aligned(q) && tr_aligned(k) && tr_aligned(v) && tr_aligned(dr)) hipLaunchKernelGGL(k_team_ret_bwd<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_team_ret_bwd<false>, grid, dim3(256), 0, st, a);
  return check_launch("magpo_team_retention_bwd");
}
