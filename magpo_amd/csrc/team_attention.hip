// Softmax attention over independent teams for gfx950: the Multi-Agent Transformer (mat).
//
// Reference semantics: SelfAttention.__call__ between the projections (mava/networks/attention.py:50-77): a team of A consecutive token
// rows is one sequence and every head of hs channels (head n at columns n hs .. n hs + hs - 1 of the q / k / v / y rows) is its own problem,
//   P_ij = softmax_j((q_i . k_j) / sqrt(hs) + mask_ij) ,  y_i = sum_j P_ij v_j ,  mask_ij = 0 for j <= i (or everywhere, unmasked), -inf else.
// q, k and v are separate pointers with their own row strides (the cross-attention takes q from another tensor than k / v).
//
// One thread per (team, query row), floor(64 / A) whole teams per 64-thread workgroup, blockIdx.y = head.  A team has at most 32 rows of at
// most 64 channels, so a row's whole problem is a few thousand multiply-adds; they run on the vector ALU in fp64, and every output is rounded
// to fp32 once.  (The first version of these kernels ran the products on team_retention.hip's fp32-MFMA tile.  Its error against fp64 was
// 1 - 3 x that of an fp32 evaluation on the CPU, above the factor 2 the kernels are held to in about one comparison in ten, and a fp32
// score of magnitude 60 carries 4e-6 into every weight.  With these kernels the acting step of the 8-agent, two-block network takes
// 2.8 ms at 16 384 envs against 3.8 ms for ff_sable's chain on the MFMA retention tile: DESIGN 4t.)  The k / v rows of a team are read
// by all of its threads at the same time (one request per team and wave) and stay in L1 for the whole loop.
//
// Forward: scores to LDS (one column of 32 doubles per thread), row maximum subtracted, masked pairs never enter a sum (an exact 0 weight),
// y = (sum_j e_j v_j) / sum_j e_j, and lse_i = max_i + log(sum_j e_j) per row and head.
// Backward: recomputes P from q, k and lse -- e_ij = exp(s_ij - lse_i) needs no maximum pass, and P_ij = e_ij / sum_j e_ij takes the fp32
// rounding of lse out again (a one-agent team has P = 1 and dq = dk = 0 exactly) -- then dP = dy v^T, D_i = sum_j P_ij dP_ij
// (= rowsum(dy o y)), dS = P o (dP - D), dq_i = sum_j dS_ij k_j / sqrt(hs) by the thread of row i; P and dS go through LDS ([A][A] per
// team, never to memory) and the thread of row j then sums dv_j = sum_i P_ij dy_i and dk_j = sum_i dS_ij q_i / sqrt(hs).  No atomics:
// equal inputs give equal bits.
#include "common.hpp"

namespace magpo {

constexpr int TA_THREADS = 64;   // threads (= query rows) per workgroup
constexpr int TA_MAXA = 32;      // rows of a team

template <bool VEC> __device__ __forceinline__ float4 ta_ld4(const float* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <int HS, bool VEC> __device__ __forceinline__ void ta_load_row(float (&x)[HS], const float* __restrict__ p) {
#pragma unroll
  for (int c = 0; c < HS; c += 4) {
    const float4 t = ta_ld4<VEC>(p + c);
    x[c] = t.x; x[c + 1] = t.y; x[c + 2] = t.z; x[c + 3] = t.w;
  }
}
// a . b over HS channels in fp64, b a row in memory
template <int HS, bool VEC> __device__ __forceinline__ double ta_dot(const float (&a)[HS], const float* __restrict__ b) {
  double s0 = 0., s1 = 0.;
#pragma unroll
  for (int c = 0; c < HS; c += 4) {
    const float4 t = ta_ld4<VEC>(b + c);
    s0 += (double)a[c] * (double)t.x;
    s1 += (double)a[c + 1] * (double)t.y;
    s0 += (double)a[c + 2] * (double)t.z;
    s1 += (double)a[c + 3] * (double)t.w;
  }
  return s0 + s1;
}
// acc += w * b over HS channels, b a row in memory
template <int HS, bool VEC> __device__ __forceinline__ void ta_axpy(double (&acc)[HS], double w, const float* __restrict__ b) {
#pragma unroll
  for (int c = 0; c < HS; c += 4) {
    const float4 t = ta_ld4<VEC>(b + c);
    acc[c] += w * (double)t.x; acc[c + 1] += w * (double)t.y; acc[c + 2] += w * (double)t.z; acc[c + 3] += w * (double)t.w;
  }
}
template <int HS> __device__ __forceinline__ void ta_store_row(float* __restrict__ p, const double (&acc)[HS], double f) {
#pragma unroll
  for (int c = 0; c < HS; ++c) p[c] = (float)(acc[c] * f);
}

// the thread's (team, row): tl = team inside the workgroup, i = row; ok = the team exists
struct TaRow { long row0; int tl, i; bool ok; };
__device__ __forceinline__ TaRow ta_row(long nteams, int A) {
  const int tpb = TA_THREADS / A;
  TaRow r;
  r.tl = threadIdx.x / A;
  r.i = threadIdx.x - r.tl * A;
  const long team = (long)blockIdx.x * tpb + r.tl;
  r.ok = r.tl < tpb && team < nteams;
  r.row0 = r.ok ? team * A : 0;
  return r;
}

struct AttnFwdArgs {
  const float* q; const float* k; const float* v; long ldq, ldk, ldv;
  float* y; long ldy; float* lse;
  long nteams; int A, ntok, ret_from, masked, nh; double scale;
};

template <int HS, bool VEC>
__global__ __launch_bounds__(TA_THREADS) void k_team_attn_fwd(AttnFwdArgs a) {
  __shared__ double sc[TA_MAXA][TA_THREADS];   // column tid: the scores, then the weights, of the thread's row
  const int tid = threadIdx.x, c0 = blockIdx.y * HS;
  const TaRow r = ta_row(a.nteams, a.A);
  if (!r.ok || r.i < a.ret_from || r.i >= a.ntok) return;   // (no barrier below)
  const int n = a.masked ? r.i + 1 : a.ntok;                // keys j < n: the first ntok rows, masked: not behind i
  float q[HS];
  ta_load_row<HS, VEC>(q, a.q + (r.row0 + r.i) * a.ldq + c0);
  double m = -INFINITY;
  for (int j = 0; j < n; ++j) {
    const double s = ta_dot<HS, VEC>(q, a.k + (r.row0 + j) * a.ldk + c0) * a.scale;
    sc[j][tid] = s;
    m = fmax(m, s);
  }
  double l = 0.;
  for (int j = 0; j < n; ++j) {
    const double e = exp(sc[j][tid] - m);
    sc[j][tid] = e;
    l += e;
  }
  double acc[HS];
#pragma unroll
  for (int c = 0; c < HS; ++c) acc[c] = 0.;
  for (int j = 0; j < n; ++j) ta_axpy<HS, VEC>(acc, sc[j][tid], a.v + (r.row0 + j) * a.ldv + c0);
  ta_store_row<HS>(a.y + (r.row0 + r.i) * a.ldy + c0, acc, 1.0 / l);
  a.lse[(r.row0 + r.i) * a.nh + blockIdx.y] = (float)(m + log(l));
}

struct AttnBwdArgs {
  const float* q; const float* k; const float* v; long ldq, ldk, ldv;
  const float* lse; const float* dy; long lddy;
  float* dq; float* dk; float* dv; long lddq, lddk, lddv;
  long nteams; int A, masked, nh; double scale;
};

template <int HS, bool VEC>
__global__ __launch_bounds__(TA_THREADS) void k_team_attn_bwd(AttnBwdArgs a) {
  __shared__ double sP[TA_MAXA][TA_THREADS + 1];   // [j][tid of row i]: P_ij
  __shared__ double sS[TA_MAXA][TA_THREADS + 1];   // [j][tid of row i]: dP_ij, then dS_ij
  const int tid = threadIdx.x, c0 = blockIdx.y * HS, A = a.A;
  const TaRow r = ta_row(a.nteams, A);
  const int n = a.masked ? r.i + 1 : A;
  double acc[HS];
  if (r.ok) {   // as query row i
    float q[HS], dy[HS];
    ta_load_row<HS, VEC>(q, a.q + (r.row0 + r.i) * a.ldq + c0);
    ta_load_row<HS, VEC>(dy, a.dy + (r.row0 + r.i) * a.lddy + c0);
    const double lse = (double)a.lse[(r.row0 + r.i) * a.nh + blockIdx.y];
    double l = 0.;
    for (int j = 0; j < n; ++j) {
      const double e = exp(ta_dot<HS, VEC>(q, a.k + (r.row0 + j) * a.ldk + c0) * a.scale - lse);
      sP[j][tid] = e;
      l += e;
    }
    double D = 0.;
    for (int j = 0; j < n; ++j) {
      const double p = sP[j][tid] / l, dp = ta_dot<HS, VEC>(dy, a.v + (r.row0 + j) * a.ldv + c0);
      sP[j][tid] = p;
      sS[j][tid] = dp;
      D += p * dp;
    }
#pragma unroll
    for (int c = 0; c < HS; ++c) acc[c] = 0.;
    for (int j = 0; j < n; ++j) {
      const double ds = sP[j][tid] * (sS[j][tid] - D);
      sS[j][tid] = ds;
      ta_axpy<HS, VEC>(acc, ds, a.k + (r.row0 + j) * a.ldk + c0);
    }
    ta_store_row<HS>(a.dq + (r.row0 + r.i) * a.lddq + c0, acc, a.scale);
    for (int j = n; j < A; ++j) { sP[j][tid] = 0.; sS[j][tid] = 0.; }   // masked pairs: an exact 0
  }
  __syncthreads();
  if (!r.ok) return;
  const int t0 = r.tl * A, j = r.i;   // as key row j: column sums over the team's query rows
#pragma unroll
  for (int c = 0; c < HS; ++c) acc[c] = 0.;
  for (int i = 0; i < A; ++i) ta_axpy<HS, VEC>(acc, sP[j][t0 + i], a.dy + (r.row0 + i) * a.lddy + c0);
  ta_store_row<HS>(a.dv + (r.row0 + j) * a.lddv + c0, acc, 1.0);
#pragma unroll
  for (int c = 0; c < HS; ++c) acc[c] = 0.;
  for (int i = 0; i < A; ++i) ta_axpy<HS, VEC>(acc, sS[j][t0 + i], a.q + (r.row0 + i) * a.ldq + c0);
  ta_store_row<HS>(a.dk + (r.row0 + j) * a.lddk + c0, acc, a.scale);
}

}  // namespace magpo

using namespace magpo;

static bool ta_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static long ta_blocks(long nteams, int A) { return (nteams + TA_THREADS / A - 1) / (TA_THREADS / A); }

static int ta_check_shape(const char* what, long nteams, int A, int hs, int nh) {
  if (nteams < 0 || A < 1 || A > TA_MAXA || (hs != 16 && hs != 32 && hs != 64) || nh < 1 || nh > 64) {
    set_error(what);
    return MAGPO_EINVAL;
  }
  if (ta_blocks(nteams, A) > 0x7fffffffL) { set_error("team_attention: too many teams for one launch"); return MAGPO_EINVAL; }
  return MAGPO_OK;
}
// a row stride: a multiple of 4 floats that holds the nh heads
static bool ta_bad_ld(long ld, int hs, int nh) { return (ld & 3) || ld < (long)hs * nh; }

#define TA_LAUNCH(K_, vec, ...)                                                                              \
  {                                                                                                          \
    if (hs == 16) { if (vec) hipLaunchKernelGGL((K_<16, true>), __VA_ARGS__); else hipLaunchKernelGGL((K_<16, false>), __VA_ARGS__); }      \
    else if (hs == 32) { if (vec) hipLaunchKernelGGL((K_<32, true>), __VA_ARGS__); else hipLaunchKernelGGL((K_<32, false>), __VA_ARGS__); } \
    else { if (vec) hipLaunchKernelGGL((K_<64, true>), __VA_ARGS__); else hipLaunchKernelGGL((K_<64, false>), __VA_ARGS__); }               \
  }

extern "C" int magpo_team_attention_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* y, long ldy,
                                        float* lse, long nteams, int A, int ntok, int ret_from, int masked, int hs, int nh, hipStream_t st) {
  if (!q || !k || !v || !y || !lse) { set_error("team_attention_fwd: q, k, v, y and lse must not be null"); return MAGPO_EINVAL; }
  if (int e = ta_check_shape("team_attention_fwd: need nteams >= 0, 1 <= A <= 32, hs in {16, 32, 64}, 1 <= nh <= 64", nteams, A, hs, nh)) return e;
  if (ntok < 1 || ntok > A || ret_from < 0 || ret_from >= ntok) { set_error("team_attention_fwd: need 1 <= ntok <= A, 0 <= ret_from < ntok"); return MAGPO_EINVAL; }
  if (ta_bad_ld(ldq, hs, nh) || ta_bad_ld(ldk, hs, nh) || ta_bad_ld(ldv, hs, nh) || ta_bad_ld(ldy, hs, nh)) {
    set_error("team_attention_fwd: row strides must be multiples of 4 floats and hold nh * hs floats");
    return MAGPO_EINVAL;
  }
  if (nteams == 0) return MAGPO_OK;
  AttnFwdArgs a{q, k, v, ldq, ldk, ldv, y, ldy, lse, nteams, A, ntok, ret_from, masked ? 1 : 0, nh, 1.0 / sqrt((double)hs)};
  const dim3 grid((unsigned)ta_blocks(nteams, A), (unsigned)nh);
  const bool vec = ta_aligned(q) && ta_aligned(k) && ta_aligned(v);
  TA_LAUNCH(k_team_attn_fwd, vec, grid, dim3(TA_THREADS), 0, st, a)
  return check_launch("magpo_team_attention_fwd");
}

extern "C" int magpo_team_attention_bwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* lse,
                                        const float* dy, long lddy, float* dq, long lddq, float* dk, long lddk, float* dv, long lddv,
                                        long nteams, int A, int masked, int hs, int nh, hipStream_t st) {
  if (!q || !k || !v || !lse || !dy || !dq || !dk || !dv) {
    set_error("team_attention_bwd: q, k, v, lse, dy, dq, dk and dv must not be null");
    return MAGPO_EINVAL;
  }
  if (int e = ta_check_shape("team_attention_bwd: need nteams >= 0, 1 <= A <= 32, hs in {16, 32, 64}, 1 <= nh <= 64", nteams, A, hs, nh)) return e;
  if (ta_bad_ld(ldq, hs, nh) || ta_bad_ld(ldk, hs, nh) || ta_bad_ld(ldv, hs, nh) || ta_bad_ld(lddy, hs, nh) || ta_bad_ld(lddq, hs, nh) ||
      ta_bad_ld(lddk, hs, nh) || ta_bad_ld(lddv, hs, nh)) {
    set_error("team_attention_bwd: row strides must be multiples of 4 floats and hold nh * hs floats");
    return MAGPO_EINVAL;
  }
  if (nteams == 0) return MAGPO_OK;
  AttnBwdArgs a{q, k, v, ldq, ldk, ldv, lse, dy, lddy, dq, dk, dv, lddq, lddk, lddv, nteams, A, masked ? 1 : 0, nh, 1.0 / sqrt((double)hs)};
  const dim3 grid((unsigned)ta_blocks(nteams, A), (unsigned)nh);
  const bool vec = ta_aligned(q) && ta_aligned(k) && ta_aligned(v) && ta_aligned(dy);
  TA_LAUNCH(k_team_attn_bwd, vec, grid, dim3(TA_THREADS), 0, st, a)
  return check_launch("magpo_team_attention_bwd");
}
