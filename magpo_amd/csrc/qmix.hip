// QMIX monotonic mixing network (gfx950): forward, backward and TD loss of rec_qmix.
//
// Reference: QMixingNetwork, mava/networks/base.py:276-343; MLPTorso, torsos.py:24-47; rec_qmix.py:358-367, :413 (loss).
// For one row (b, t) with agent values q[A] and global state s[G]:
//   x = LayerNorm(s) * scale + bias (flax: rstd = rsqrt(max(E[s^2] - E[s]^2, 0) + 1e-6)), or x = s
//   w1 = |Dense(A E)(relu(Dense(64)(x)))|, b1 = Dense(E)(x), hidden = elu(q . w1 + b1)
//   w2 = |Dense(E)(relu(Dense(64)(x)))|,   b2 = Dense(1)(relu(Dense(E)(x))), q_tot = hidden . w2 + b2
//
// The mixer is launch-bound (about 0.2 GFLOP per epoch), so each direction is ONE launch.  A workgroup of 256 threads owns a tile of
// RT = 16 rows whose activations live in LDS; the weights (up to ~260 KB) are streamed from L2 once per tile, one output column per thread
// with the 16 row accumulators in registers (fp32 FMA).  The global state is never materialised: a row's state is read straight from the A
// observation rows of its team (the layout of magpo_global_state).  The backward recomputes the two hypernetwork outputs from the saved
// 64-wide hiddens, and leaves every parameter gradient as per-workgroup slabs [grid][P] in the layout of the parameter buffer, folded by
// magpo_reduce_slabs in a fixed order: no atomics, two runs give the same bits.
#include "common.hpp"
#include "qselect.hpp"

namespace magpo {

constexpr int QM_RT = 16;     // rows per tile
constexpr int QM_HH = 64;     // hypernetwork hidden width
constexpr int QM_NPAR = 16;   // parameter entries
// entry order of the offset table (floats from the start of the parameter / gradient buffer)
enum { P_W1A = 0, P_W1AB, P_W1B, P_W1BB, P_B1W, P_B1B, P_W2A, P_W2AB, P_W2B, P_W2BB, P_B2A, P_B2AB, P_B2W, P_B2B, P_LNS, P_LNB };

struct MixDims { int A, E, G, F_raw, id_cols, norm, Tm, Ts, t_off, qmode, K; };
struct MixOffs { long o[QM_NPAR]; };

__host__ __device__ inline int qm_round4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int qm_save_floats(int E, int G) { return 2 * QM_HH + 2 * E + qm_round4(G) + 4; }
__host__ __device__ inline int qm_entry_size(const MixDims& d, int i) {
  switch (i) {
    case P_W1A: case P_W2A: return d.G * QM_HH;
    case P_W1AB: case P_W2AB: return QM_HH;
    case P_W1B: return QM_HH * d.A * d.E;
    case P_W1BB: return d.A * d.E;
    case P_B1W: case P_B2A: return d.G * d.E;
    case P_B1B: case P_W2BB: case P_B2AB: case P_B2W: return d.E;
    case P_W2B: return QM_HH * d.E;
    case P_B2B: return 1;
    default: return d.G;   // layer_norm scale / bias
  }
}
// LDS floats of a tile: x | h1 | h2 | b1 (bwd: d pre-activation) | hb | dhb | w1 | w2 | hidden | q | dq | dq_tot
__host__ __device__ inline int qm_lds_floats(const MixDims& d) {
  return QM_RT * (qm_round4(d.G) + 2 * QM_HH + 5 * d.E + d.A * d.E + 2 * qm_round4(d.A) + 1);
}

// observation-row group (team) that mixer row r reads: row r = (sequence, step) with Tm steps per sequence, taken from sequences of Ts
// stored steps starting at step t_off
__device__ __forceinline__ long qm_src_group(const MixDims& d, long r) {
  const long s = r / d.Tm;
  return s * d.Ts + (r - s * d.Tm) + d.t_off;
}

struct Tile {
  float *x, *h1, *h2, *b1, *hb, *dhb, *w1, *w2, *q, *dq, *hid, *dqt;
  int G4, AE, A4;
};
__device__ __forceinline__ Tile qm_tile(float* sm, const MixDims& d) {
  Tile t;
  t.G4 = qm_round4(d.G); t.AE = d.A * d.E; t.A4 = qm_round4(d.A);
  float* p = sm;
  t.x = p; p += QM_RT * t.G4;
  t.h1 = p; p += QM_RT * QM_HH;
  t.h2 = p; p += QM_RT * QM_HH;
  t.b1 = p; p += QM_RT * d.E;
  t.hb = p; p += QM_RT * d.E;
  t.dhb = p; p += QM_RT * d.E;
  t.w1 = p; p += QM_RT * t.AE;
  t.w2 = p; p += QM_RT * d.E;
  t.hid = p; p += QM_RT * d.E;
  t.q = p; p += QM_RT * t.A4;
  t.dq = p; p += QM_RT * t.A4;
  t.dqt = p;
  return t;
}

// out[r] = sum_k xs[r][k] W[k ld + col], k < KIN: one output column per thread, weights streamed (coalesced across the threads' columns)
__device__ __forceinline__ void qm_col(const float* __restrict__ xs, int ldx, int KIN, const float* __restrict__ W, int ld, float (&acc)[QM_RT]) {
#pragma unroll
  for (int r = 0; r < QM_RT; ++r) acc[r] = 0.f;
  for (int k = 0; k < KIN; ++k) {
    const float w = W[(long)k * ld];
#pragma unroll
    for (int r = 0; r < QM_RT; ++r) acc[r] = fmaf(xs[r * ldx + k], w, acc[r]);
  }
}

// the two hypernetwork outputs of a tile, signed (before |.|): w1 [RT][A E] from h1, w2 [RT][E] from h2
__device__ __forceinline__ void qm_hyper_out(const Tile& t, const MixDims& d, const float* __restrict__ par, const MixOffs& of) {
  float acc[QM_RT];
  for (int c = threadIdx.x; c < t.AE + d.E; c += 256) {
    const bool first = c < t.AE;
    const int cc = first ? c : c - t.AE, ld = first ? t.AE : d.E;
    qm_col(first ? t.h1 : t.h2, QM_HH, QM_HH, par + of.o[first ? P_W1B : P_W2B] + cc, ld, acc);
    const float b = par[of.o[first ? P_W1BB : P_W2BB] + cc];
    float* dst = first ? t.w1 : t.w2;
#pragma unroll
    for (int r = 0; r < QM_RT; ++r) dst[r * ld + cc] = acc[r] + b;
  }
}

struct MixFwdArgs {
  MixDims d; MixOffs of; const float* par;
  const float* obs; long ldo; const float* q; const float* qo; long ldq; const int* index; const unsigned char* mask;
  float* q_tot; float* q_used; float* save; long R;
};

extern __shared__ __align__(16) float qm_smem[];

__global__ __launch_bounds__(256) void k_qmix_fwd(MixFwdArgs a) {
  const MixDims& d = a.d;
  const Tile t = qm_tile(qm_smem, d);
  const int tid = threadIdx.x, A = d.A, E = d.E, G = d.G, SV = qm_save_floats(E, G);
  const long row0 = (long)blockIdx.x * QM_RT;
  const float* par = a.par;
  // ---- the global state of the tile's rows, read from the team's observation rows
  for (int i = tid; i < QM_RT * G; i += 256) {
    const int r = i / G, g = i - r * G;
    const long row = row0 + r;
    float v = 0.f;
    if (row < a.R) {
      const int ag = g / d.F_raw, f = g - ag * d.F_raw;
      v = a.obs[(qm_src_group(d, row) * A + ag) * a.ldo + d.id_cols + f];
    }
    t.x[r * t.G4 + g] = v;
  }
  // ---- the agents' values: given, or selected from 64-wide Q rows
  for (int i = tid; i < QM_RT * A; i += 256) {
    const int r = i / A, ag = i - r * A;
    const long row = row0 + r;
    float v = 0.f;
    if (row < a.R) {
      if (d.qmode == 0) {
        v = a.q[row * A + ag];
      } else {
        const long src = qm_src_group(d, row) * A + ag;
        int k;
        if (d.qmode == 1) {
          k = a.index[row * A + ag];
          k = k < 0 ? 0 : (k >= d.K ? d.K - 1 : k);   // (a gather with an out-of-range index clamps)
        } else {
          k = masked_argmax(a.qo + src * a.ldq, a.mask ? a.mask + src * d.K : nullptr, d.K);
        }
        v = a.q[src * a.ldq + k];
      }
      if (a.q_used) a.q_used[row * A + ag] = v;
    }
    t.q[r * t.A4 + ag] = v;
  }
  __syncthreads();
  // ---- LayerNorm over the state: 16 lanes per row
  if (d.norm) {
    const int r = tid >> 4, l = tid & 15;
    float s = 0.f, s2 = 0.f;
    for (int g = l; g < G; g += 16) { const float v = t.x[r * t.G4 + g]; s += v; s2 = fmaf(v, v, s2); }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); s2 += __shfl_xor(s2, o, 64); }
    const float mean = s / (float)G;
    const float var = fmaxf(s2 / (float)G - mean * mean, 0.f);
    const float rstd = 1.0f / sqrtf(var + 1e-6f);
    const long row = row0 + r;
    for (int g = l; g < G; g += 16) {
      const float xh = (t.x[r * t.G4 + g] - mean) * rstd;
      if (a.save && row < a.R) a.save[row * SV + 2 * QM_HH + 2 * E + g] = xh;
      t.x[r * t.G4 + g] = fmaf(xh, par[a.of.o[P_LNS] + g], par[a.of.o[P_LNB] + g]);
    }
    if (a.save && row < a.R && l == 0) a.save[row * SV + 2 * QM_HH + 2 * E + t.G4] = rstd;
  } else if (a.save) {
    for (int i = tid; i < QM_RT * G; i += 256) {
      const int r = i / G, g = i - r * G;
      if (row0 + r < a.R) a.save[(row0 + r) * SV + 2 * QM_HH + 2 * E + g] = t.x[r * t.G4 + g];
    }
  }
  __syncthreads();
  // ---- the four first layers: columns [h1 64 | h2 64 | b1 E | hb E], one per thread
  {
    const int c = tid;
    if (c < 2 * QM_HH + 2 * E) {
      const float* W; const float* bias; float* dst; int ld, cc; bool relu = true;
      if (c < QM_HH) { cc = c; ld = QM_HH; W = par + a.of.o[P_W1A]; bias = par + a.of.o[P_W1AB]; dst = t.h1; }
      else if (c < 2 * QM_HH) { cc = c - QM_HH; ld = QM_HH; W = par + a.of.o[P_W2A]; bias = par + a.of.o[P_W2AB]; dst = t.h2; }
      else if (c < 2 * QM_HH + E) { cc = c - 2 * QM_HH; ld = E; W = par + a.of.o[P_B1W]; bias = par + a.of.o[P_B1B]; dst = t.b1; relu = false; }
      else { cc = c - 2 * QM_HH - E; ld = E; W = par + a.of.o[P_B2A]; bias = par + a.of.o[P_B2AB]; dst = t.hb; }
      float acc[QM_RT];
      qm_col(t.x, t.G4, G, W + cc, ld, acc);
      const float b = bias[cc];
      // save slots: h1 | h2 | hb | hidden (b1 is not needed by the backward; its slot takes hidden below)
      const int so = c < 2 * QM_HH ? c : (c < 2 * QM_HH + E ? -1 : 2 * QM_HH + cc);
#pragma unroll
      for (int r = 0; r < QM_RT; ++r) {
        float v = acc[r] + b;
        if (relu) v = fmaxf(v, 0.f);
        dst[r * ld + cc] = v;
        if (a.save && so >= 0 && row0 + r < a.R) a.save[(row0 + r) * SV + so] = v;
      }
    }
  }
  __syncthreads();
  qm_hyper_out(t, d, par, a.of);
  __syncthreads();
  // ---- hidden = elu(q . |w1| + b1)
  for (int i = tid; i < QM_RT * E; i += 256) {
    const int r = i / E, e = i - r * E;
    float s = 0.f;
    for (int ag = 0; ag < A; ++ag) s = fmaf(t.q[r * t.A4 + ag], fabsf(t.w1[r * t.AE + ag * E + e]), s);
    s += t.b1[r * E + e];
    const float h = s > 0.f ? s : expm1f(s);
    t.hid[r * E + e] = h;
    if (a.save && row0 + r < a.R) a.save[(row0 + r) * SV + 2 * QM_HH + E + e] = h;
  }
  __syncthreads();
  // ---- q_tot = hidden . |w2| + (hb . v + c): 16 lanes per row
  {
    const int r = tid >> 4, l = tid & 15;
    float s = 0.f;
    for (int e = l; e < E; e += 16) s = fmaf(t.hid[r * E + e], fabsf(t.w2[r * E + e]), fmaf(t.hb[r * E + e], par[a.of.o[P_B2W] + e], s));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0 && row0 + r < a.R) a.q_tot[row0 + r] = s + par[a.of.o[P_B2B]];
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void qm_put4(float* dst, float4 v, bool first) {
  float4* p = reinterpret_cast<float4*>(dst);
  if (!first) { const float4 o = *p; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
  *p = v;
}
// slab dW [KIN][NOUT] (+)= xs^T ds and db [NOUT] (+)= column sums of ds over the tile; NOUT a multiple of 4.  Every slab element is owned
// by one thread, the same for every tile of the workgroup.
__device__ __forceinline__ void qm_wgrad(const float* __restrict__ xs, int ldx, int KIN, const float* __restrict__ ds, int ldd, int NOUT,
                                         float* __restrict__ sw, float* __restrict__ sb, bool first) {
  const int n4 = NOUT >> 2, items = (KIN + 1) * n4;
  for (int i = threadIdx.x; i < items; i += 256) {
    const int g = i / n4, c4 = (i - g * n4) << 2;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < QM_RT; ++r) {
      const float x = g < KIN ? xs[r * ldx + g] : 1.f;
      const float4 dv = *reinterpret_cast<const float4*>(ds + r * ldd + c4);
      acc.x = fmaf(x, dv.x, acc.x); acc.y = fmaf(x, dv.y, acc.y); acc.z = fmaf(x, dv.z, acc.z); acc.w = fmaf(x, dv.w, acc.w);
    }
    qm_put4(g < KIN ? sw + (long)g * NOUT + c4 : sb + c4, acc, first);
  }
}
// acc[r] += sum_c ds[r][c] W[k NOUT + c] for thread (k = tid / SUB, sub = tid % SUB): the SUB lanes of a k split the columns in float4
// steps; the caller folds them with qm_fold<SUB>.  Threads with k >= KIN add nothing.
template <int SUB>
__device__ __forceinline__ void qm_dx(const float* __restrict__ ds, int ldd, int NOUT, const float* __restrict__ W, int KIN, float (&acc)[QM_RT]) {
  const int k = threadIdx.x / SUB, sub = threadIdx.x % SUB;
  if (k >= KIN) return;
  for (int c4 = 4 * sub; c4 < NOUT; c4 += 4 * SUB) {
    const float4 w = *reinterpret_cast<const float4*>(W + (long)k * NOUT + c4);
#pragma unroll
    for (int r = 0; r < QM_RT; ++r) {
      const float4 dv = *reinterpret_cast<const float4*>(ds + r * ldd + c4);
      acc[r] = fmaf(dv.x, w.x, fmaf(dv.y, w.y, fmaf(dv.z, w.z, fmaf(dv.w, w.w, acc[r]))));
    }
  }
}
template <int SUB>
__device__ __forceinline__ void qm_fold(float (&acc)[QM_RT]) {
#pragma unroll
  for (int r = 0; r < QM_RT; ++r)
#pragma unroll
    for (int o = SUB >> 1; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
}

struct MixBwdArgs {
  MixDims d; MixOffs of; const float* par; long P;
  const float* save; const float* q_used; const float* dq_tot;
  float* dq; float* dq64; long lddq; const int* index; float* slab; long R;
};

__global__ __launch_bounds__(256) void k_qmix_bwd(MixBwdArgs a) {
  const MixDims& d = a.d;
  const Tile t = qm_tile(qm_smem, d);
  const int tid = threadIdx.x, A = d.A, E = d.E, G = d.G, SV = qm_save_floats(E, G);
  const float* par = a.par;
  float* slab = a.slab + (long)blockIdx.x * a.P;
  const long ntiles = (a.R + QM_RT - 1) / QM_RT;
  // the padding between the entries of the buffer, and the LayerNorm entries without normalisation: zero, once
  for (int i = tid; i < QM_NPAR * 4; i += 256) {
    const int e = i >> 2, j = i & 3, n = qm_entry_size(d, e);
    if (n + j < qm_round4(n)) slab[a.of.o[e] + n + j] = 0.f;
  }
  if (!d.norm)
    for (int g = tid; g < G; g += 256) { slab[a.of.o[P_LNS] + g] = 0.f; slab[a.of.o[P_LNB] + g] = 0.f; }
  bool first = true;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x, first = false) {
    const long row0 = tile * QM_RT;
    __syncthreads();
    // ---- what the forward saved; rows beyond R read as zero, so that they add nothing to any sum
    for (int i = tid; i < QM_RT * SV; i += 256) {
      const int r = i / SV, c = i - r * SV;
      const long row = row0 + r;
      const float v = row < a.R ? a.save[row * SV + c] : 0.f;
      if (c < QM_HH) t.h1[r * QM_HH + c] = v;
      else if (c < 2 * QM_HH) t.h2[r * QM_HH + c - QM_HH] = v;
      else if (c < 2 * QM_HH + E) t.hb[r * E + c - 2 * QM_HH] = v;
      else if (c < 2 * QM_HH + 2 * E) t.hid[r * E + c - 2 * QM_HH - E] = v;
      else if (c < 2 * QM_HH + 2 * E + G) {
        const int g = c - 2 * QM_HH - 2 * E;
        t.x[r * t.G4 + g] = (d.norm && row < a.R) ? fmaf(v, par[a.of.o[P_LNS] + g], par[a.of.o[P_LNB] + g]) : v;
      }
    }
    for (int i = tid; i < QM_RT * A; i += 256) {
      const int r = i / A, ag = i - r * A;
      t.q[r * t.A4 + ag] = row0 + r < a.R ? a.q_used[(row0 + r) * A + ag] : 0.f;
    }
    if (tid < QM_RT) t.dqt[tid] = row0 + tid < a.R ? a.dq_tot[row0 + tid] : 0.f;
    __syncthreads();
    qm_hyper_out(t, d, par, a.of);
    __syncthreads();
    // ---- through the second layer and the elu: b1 <- d(pre-activation), w2 <- d(w2 before |.|), dhb
    for (int i = tid; i < QM_RT * E; i += 256) {
      const int r = i / E, e = i - r * E;
      const float g = t.dqt[r], w2 = t.w2[i], h = t.hid[i];
      const float sg = w2 > 0.f ? 1.f : (w2 < 0.f ? -1.f : 0.f);
      t.b1[i] = g * fabsf(w2) * (h > 0.f ? 1.f : h + 1.f);   // elu' = 1 for x > 0, else exp(x) = elu(x) + 1
      t.w2[i] = g * h * sg;
      t.dhb[i] = t.hb[i] > 0.f ? g * par[a.of.o[P_B2W] + e] : 0.f;
    }
    __syncthreads();
    // ---- dq = d(pre) . |w1|
    for (int i = tid; i < QM_RT * A; i += 256) {
      const int r = i / A, ag = i - r * A;
      float s = 0.f;
      for (int e = 0; e < E; ++e) s = fmaf(t.b1[r * E + e], fabsf(t.w1[r * t.AE + ag * E + e]), s);
      if (row0 + r < a.R && a.dq) a.dq[(row0 + r) * A + ag] = s;
      t.dq[i] = s;   // (kept for the scatter below)
    }
    __syncthreads();
    // ---- the scatter into 64-wide Q-gradient rows (what seq_bwd takes): dq in column index[row][agent], zero elsewhere
    if (a.dq64) {
      for (int i = tid; i < QM_RT * A * 16; i += 256) {
        const int ra = i >> 4, c4 = (i & 15) << 2, r = ra / A, ag = ra - r * A;
        const long row = row0 + r;
        if (row >= a.R) continue;
        int k = a.index[row * A + ag];
        k = k < 0 ? 0 : (k >= d.K ? d.K - 1 : k);
        const float g = t.dq[ra];
        *reinterpret_cast<float4*>(a.dq64 + (qm_src_group(d, row) * A + ag) * a.lddq + c4) =
            make_float4(c4 == k ? g : 0.f, c4 + 1 == k ? g : 0.f, c4 + 2 == k ? g : 0.f, c4 + 3 == k ? g : 0.f);
      }
    }
    // ---- w1 <- d(w1 before |.|) = d(pre)[e] q[a] sign(w1)
    for (int i = tid; i < QM_RT * t.AE; i += 256) {
      const int r = i / t.AE, c = i - r * t.AE, ag = c / E, e = c - ag * E;
      const float w1 = t.w1[i];
      const float sg = w1 > 0.f ? 1.f : (w1 < 0.f ? -1.f : 0.f);
      t.w1[i] = t.b1[r * E + e] * t.q[r * t.A4 + ag] * sg;
    }
    __syncthreads();
    // ---- parameter gradients of the layers behind the hiddens
    qm_wgrad(t.h1, QM_HH, QM_HH, t.w1, t.AE, t.AE, slab + a.of.o[P_W1B], slab + a.of.o[P_W1BB], first);
    qm_wgrad(t.h2, QM_HH, QM_HH, t.w2, E, E, slab + a.of.o[P_W2B], slab + a.of.o[P_W2BB], first);
    qm_wgrad(t.x, t.G4, G, t.b1, E, E, slab + a.of.o[P_B1W], slab + a.of.o[P_B1B], first);
    if (tid <= E) {   // hyper_b2's last layer: dv[e] = sum_r dq_tot[r] hb[r][e], dc = sum_r dq_tot[r]
      float s = 0.f;
      for (int r = 0; r < QM_RT; ++r) s = fmaf(t.dqt[r], tid < E ? t.hb[r * E + tid] : 1.f, s);
      float* dst = tid < E ? slab + a.of.o[P_B2W] + tid : slab + a.of.o[P_B2B];
      *dst = first ? s : *dst + s;
    }
    __syncthreads();
    // ---- into the 64-wide hiddens (in place, masked by the relu)
    {
      float acc[QM_RT];
#pragma unroll
      for (int r = 0; r < QM_RT; ++r) acc[r] = 0.f;
      qm_dx<4>(t.w1, t.AE, t.AE, par + a.of.o[P_W1B], QM_HH, acc);
      qm_fold<4>(acc);
      float acc2[QM_RT];
#pragma unroll
      for (int r = 0; r < QM_RT; ++r) acc2[r] = 0.f;
      qm_dx<4>(t.w2, E, E, par + a.of.o[P_W2B], QM_HH, acc2);
      qm_fold<4>(acc2);
      if ((tid & 3) == 0) {
        const int k = tid >> 2;
#pragma unroll
        for (int r = 0; r < QM_RT; ++r) {
          t.h1[r * QM_HH + k] = t.h1[r * QM_HH + k] > 0.f ? acc[r] : 0.f;
          t.h2[r * QM_HH + k] = t.h2[r * QM_HH + k] > 0.f ? acc2[r] : 0.f;
        }
      }
    }
    __syncthreads();
    qm_wgrad(t.x, t.G4, G, t.h1, QM_HH, QM_HH, slab + a.of.o[P_W1A], slab + a.of.o[P_W1AB], first);
    qm_wgrad(t.x, t.G4, G, t.h2, QM_HH, QM_HH, slab + a.of.o[P_W2A], slab + a.of.o[P_W2AB], first);
    qm_wgrad(t.x, t.G4, G, t.dhb, E, E, slab + a.of.o[P_B2A], slab + a.of.o[P_B2AB], first);
    // ---- LayerNorm scale / bias: dx = the four first layers' input gradients; dscale = sum_r dx xhat, dbias = sum_r dx
    if (d.norm) {
      float acc[QM_RT];
#pragma unroll
      for (int r = 0; r < QM_RT; ++r) acc[r] = 0.f;
      qm_dx<2>(t.h1, QM_HH, QM_HH, par + a.of.o[P_W1A], G, acc);
      qm_dx<2>(t.h2, QM_HH, QM_HH, par + a.of.o[P_W2A], G, acc);
      qm_dx<2>(t.b1, E, E, par + a.of.o[P_B1W], G, acc);
      qm_dx<2>(t.dhb, E, E, par + a.of.o[P_B2A], G, acc);
      qm_fold<2>(acc);
      const int g = tid >> 1;
      if ((tid & 1) == 0 && g < G) {
        float ds = 0.f, db = 0.f;
        for (int r = 0; r < QM_RT; ++r) {
          const float xh = row0 + r < a.R ? a.save[(row0 + r) * SV + 2 * QM_HH + 2 * E + g] : 0.f;
          ds = fmaf(acc[r], xh, ds); db += acc[r];
        }
        float* ps = slab + a.of.o[P_LNS] + g; float* pb = slab + a.of.o[P_LNB] + g;
        *ps = first ? ds : *ps + ds; *pb = first ? db : *pb + db;
      }
    }
  }
}

// ---- TD loss (rec_qmix.py:358-367, :413, :423-425): one workgroup per stacked group -----------------------------------------------------
struct MixTdArgs {
  const float* q_tot; const float* next_q_tot; const float* reward; const unsigned char* tot;
  float* dq_tot; double* part; long R1; int L; float gamma, two_inv_R;
};
__global__ __launch_bounds__(256) void k_qmix_td(MixTdArgs a) {
#pragma clang fp contract(off)   // (the target's product and sum are two roundings: never fused)
  __shared__ double sh[8][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, T = a.L - 1;
  const long base = (long)blockIdx.x * a.R1, nseq = a.R1 / T, base_tot = (long)blockIdx.x * nseq * a.L;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // err^2, q, target, reward, next q, term_or_trunc
  float emax = 0.f, emin = INFINITY;
  for (long i = threadIdx.x; i < a.R1; i += 256) {
    const long r = base + i, s = i / T;
    const float done = a.tot[base_tot + s * a.L + (i - s * T) + 1] ? 1.f : 0.f;
    const float nq = a.next_q_tot[r], rew = a.reward[r], q = a.q_tot[r];
    // plain operators under the pragma above: one rounding each (the __f*_rn intrinsics carry the header's own contraction setting)
    const float keep = (1.f - done) * a.gamma;
    const float boot = keep * nq;
    const float target = rew + boot;
    const float err = q - target, e2 = err * err;
    a.dq_tot[r] = a.two_inv_R * err;
    acc[0] += (double)err * (double)err; acc[1] += (double)q; acc[2] += (double)target; acc[3] += (double)rew; acc[4] += (double)nq;
    emax = fmaxf(emax, e2); emin = fminf(emin, e2);
  }
  for (long i = threadIdx.x; i < nseq * a.L; i += 256) acc[5] += a.tot[base_tot + i] ? 1.0 : 0.0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    double w = q < 6 ? acc[q] : (q == 6 ? (double)emax : (double)emin);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double v = __shfl_xor(w, o, 64);
      w = q < 6 ? w + v : (q == 6 ? fmax(w, v) : fmin(w, v));
    }
    if (lane == 0) sh[q][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int q = threadIdx.x;
    const double* s = sh[q];
    a.part[8 * blockIdx.x + q] = q < 6 ? (s[0] + s[1]) + (s[2] + s[3]) : (q == 6 ? fmax(fmax(s[0], s[1]), fmax(s[2], s[3])) : fmin(fmin(s[0], s[1]), fmin(s[2], s[3])));
  }
}
// out: [q_loss, mean_q, max_q_error, min_q_error, mean_target, mean_reward_t0, mean_next_qval, done]
__global__ void k_qmix_td_final(const double* __restrict__ part, int U, double inv_R, double inv_tot, float* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int u = 0; u < U; ++u)
    for (int q = 0; q < 8; ++q) s[q] += part[8 * u + q];
  out[0] = (float)(s[0] * inv_R); out[1] = (float)(s[1] * inv_R);
  out[2] = (float)(s[6] / (double)U); out[3] = (float)(s[7] / (double)U);   // per-group extrema, averaged over the groups (pmean)
  out[4] = (float)(s[2] * inv_R); out[5] = (float)(s[3] * inv_R); out[6] = (float)(s[4] * inv_R); out[7] = (float)(s[5] * inv_tot);
}

}  // namespace magpo

using namespace magpo;

static const char* qmix_dims_error(const int* dims, int ndims, const long* offs, int noffs, long R) {
  if (!dims || ndims != 11 || !offs || noffs != QM_NPAR) return "dims_host must hold 11 ints and offs_host 16 offsets";
  const int A = dims[0], E = dims[1], G = dims[2], F_raw = dims[3], id_cols = dims[4], norm = dims[5], Tm = dims[6], Ts = dims[7], t_off = dims[8],
            qmode = dims[9], K = dims[10];
  if (R < 1 || R > 0x7fffffffL / 1024) return "need 1 <= R <= 2^21";
  if (E != 32 && E != 64) return "embed_dim must be 32 or 64";
  if (A < 1 || (long)A * E > 512) return "need 1 <= A and A * E <= 512";
  if (F_raw < 1 || G != A * F_raw || G > 128) return "need 1 <= G = A * F_raw <= 128";
  if (id_cols < 0 || (norm != 0 && norm != 1)) return "need id_cols >= 0 and norm_env_states 0 or 1";
  if (Tm < 1 || Ts < Tm || t_off < 0 || t_off + Tm > Ts) return "need 1 <= Tm, t_off >= 0 and t_off + Tm <= Ts";
  if (qmode < 0 || qmode > 2 || (qmode != 0 && (K < 1 || K > 32))) return "q mode must be 0, 1 or 2, with 1 <= K <= 32 for modes 1 and 2";
  for (int i = 0; i < QM_NPAR; ++i)
    if (offs[i] < 0 || (offs[i] & 3)) return "parameter offsets must be non-negative multiples of 4 floats";
  return nullptr;
}
static MixDims qmix_dims(const int* v) { return MixDims{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]}; }

template <typename K>
static int qmix_raise_lds(K kernel, size_t lds, size_t& have) {
  if (lds > 65536 && lds > have) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MAGPO_ELAUNCH;
    have = lds;   // (memoised device attribute: idempotent)
  }
  return MAGPO_OK;
}

extern "C" long magpo_qmix_save_floats(int E, int G) { return qm_save_floats(E, G); }
extern "C" long magpo_qmix_bwd_grid(long R) {
  const long n = (R + QM_RT - 1) / QM_RT;
  return n < 1 ? 1 : (n > 128 ? 128 : n);
}

extern "C" int magpo_qmix_fwd(const int* dims_host, int ndims, const float* params, const long* offs_host, int noffs, const float* obs,
                              long ldo, const float* q, const float* q_online, long ldq, const int* index, const unsigned char* mask,
                              float* q_tot, float* q_used, float* save, long R, hipStream_t st) {
  if (const char* e = qmix_dims_error(dims_host, ndims, offs_host, noffs, R)) { set_error(e); return MAGPO_EINVAL; }
  const MixDims d = qmix_dims(dims_host);
  if (ldo < (long)d.id_cols + d.F_raw) { set_error("qmix_fwd: the observation row stride must cover id_cols + F_raw"); return MAGPO_EINVAL; }
  if (d.qmode != 0 && ldq < d.K) { set_error("qmix_fwd: the Q row stride must cover K"); return MAGPO_EINVAL; }
  if (!params || !obs || !q || !q_tot || (d.qmode == 1 && !index) || (d.qmode == 2 && !q_online)) {
    set_error("qmix_fwd: params, obs, q and q_tot must not be NULL, nor index (mode 1) or q_online (mode 2)");
    return MAGPO_EINVAL;
  }
  if (save && !q_used) { set_error("qmix_fwd: the training mode (save) needs q_used"); return MAGPO_EINVAL; }
  MixFwdArgs a;
  a.d = d;
  for (int i = 0; i < QM_NPAR; ++i) a.of.o[i] = offs_host[i];
  a.par = params; a.obs = obs; a.ldo = ldo; a.q = q; a.qo = q_online; a.ldq = ldq; a.index = index; a.mask = mask;
  a.q_tot = q_tot; a.q_used = q_used; a.save = save; a.R = R;
  const size_t lds = (size_t)qm_lds_floats(d) * sizeof(float);
  static size_t have = 0;
  if (qmix_raise_lds(&k_qmix_fwd, lds, have)) { set_error("qmix_fwd: cannot raise the dynamic LDS limit"); return MAGPO_ELAUNCH; }
  hipLaunchKernelGGL(k_qmix_fwd, dim3((unsigned)((R + QM_RT - 1) / QM_RT)), dim3(256), lds, st, a);
  return check_launch("magpo_qmix_fwd");
}

extern "C" int magpo_reduce_slabs(const float* slab, float* out, int G, long P, long stride, float scale, int accumulate, hipStream_t stream);

extern "C" int magpo_qmix_bwd(const int* dims_host, int ndims, const float* params, const long* offs_host, int noffs, long P,
                              const float* save, const float* q_used, const float* dq_tot, float* dq, float* dq64, long lddq,
                              const int* index, float* slab, float* grads, long R, hipStream_t st) {
  if (const char* e = qmix_dims_error(dims_host, ndims, offs_host, noffs, R)) { set_error(e); return MAGPO_EINVAL; }
  const MixDims d = qmix_dims(dims_host);
  if (P < 4 || (P & 3)) { set_error("qmix_bwd: P must be a positive multiple of 4 floats"); return MAGPO_EINVAL; }
  for (int i = 0; i < QM_NPAR; ++i)
    if (offs_host[i] + qm_round4(qm_entry_size(d, i)) > P) { set_error("qmix_bwd: a parameter entry lies outside the P floats of the buffer"); return MAGPO_EINVAL; }
  if (!params || !save || !q_used || !dq_tot || !slab || !grads) {
    set_error("qmix_bwd: params, save, q_used, dq_tot, slab and grads must not be NULL");
    return MAGPO_EINVAL;
  }
  if (dq64 && (!index || lddq != 64 || d.K < 1 || d.K > 32)) { set_error("qmix_bwd: the scatter needs index, 1 <= K <= 32 and 64-wide gradient rows"); return MAGPO_EINVAL; }
  MixBwdArgs a;
  a.d = d;
  for (int i = 0; i < QM_NPAR; ++i) a.of.o[i] = offs_host[i];
  a.par = params; a.P = P; a.save = save; a.q_used = q_used; a.dq_tot = dq_tot; a.dq = dq; a.dq64 = dq64; a.lddq = lddq; a.index = index;
  a.slab = slab; a.R = R;
  const size_t lds = (size_t)qm_lds_floats(d) * sizeof(float);
  static size_t have = 0;
  if (qmix_raise_lds(&k_qmix_bwd, lds, have)) { set_error("qmix_bwd: cannot raise the dynamic LDS limit"); return MAGPO_ELAUNCH; }
  const int nb = (int)magpo_qmix_bwd_grid(R);
  hipLaunchKernelGGL(k_qmix_bwd, dim3(nb), dim3(256), lds, st, a);
  if (int e = check_launch("magpo_qmix_bwd")) return e;
  return magpo_reduce_slabs(slab, grads, nb, P, P, 1.0f, 0, st);
}

// workspace: >= 8 * U doubles
extern "C" int magpo_qmix_td_loss(const float* q_tot, const float* next_q_tot, const float* reward, const unsigned char* term_or_trunc,
                                  int L, float gamma, float* dq_tot, double* workspace, float* loss_out, long R, int U, hipStream_t st) {
  if (R < 1 || U < 1 || U > 1024 || L < 2 || R % U || (R / U) % (L - 1)) {
    set_error("qmix_td_loss: need L >= 2, 1 <= U <= 1024 and R >= 1 a multiple of U (L - 1)");
    return MAGPO_EINVAL;
  }
  if (!q_tot || !next_q_tot || !reward || !term_or_trunc || !dq_tot || !workspace || !loss_out) { set_error("qmix_td_loss: NULL pointer"); return MAGPO_EINVAL; }
  MixTdArgs a{q_tot, next_q_tot, reward, term_or_trunc, dq_tot, workspace, R / U, L, gamma, 2.0f / (float)R};
  hipLaunchKernelGGL(k_qmix_td, dim3(U), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_qmix_td_final, dim3(1), dim3(64), 0, st, workspace, U, 1.0 / (double)R, 1.0 / ((double)(R / (L - 1)) * (double)L), loss_out);
  return check_launch("magpo_qmix_td_loss");
}
