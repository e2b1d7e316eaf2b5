// One acting step of the memoryless Sable (ff_sable) in ONE launch: SableGuider.act with memory_type "ff_sable"
// (mava/networks/sable_network.py:443-482, utils/decode.py:111-153 on zero hidden states): encoder over the A tokens of the step, value
// head, the A autoregressive decoder iterations and the sampling.  Stateless: no retention state, no decay (kappa = 1), no timestep
// positional encoding (the pe table is zero), no done handling.
//
// Layout.  A workgroup (4 waves) owns a tile of 32 envs; the 32-row tile of agent a holds token a of those 32 envs, so every dense layer
// of every decoder iteration is a full 32-row product on v_mfma_f32_32x32x2_f32 and the per-team retention (A^2 dot products of hs
// features per env) is row-local work.  A lane holds one half (32 consecutive features) of one row, as in k_linear_pro: row statistics are a
// 32-term local sum plus one shuffle with the partner lane, and that fragment IS the MFMA A operand.  An accumulator (column on the lane,
// rows in the registers) becomes a row fragment again through a row-major tile: the LDS tile T for rows that live for one layer, the
// launch's scratch for rows that several agents or iterations read (below).
//   encoder   wave w carries the agents a = w, w + 4 through embedding, q|k|v|g (all eight 32-column groups), retention over the team's A
//             rows, W_o, the norms and the value head; the waves meet only to exchange the q|k|v|g rows.
//   decoder   the iterations are sequential; the waves split a layer's 32-column groups (group c on wave c mod 4) and every wave evaluates the
//             row-wise ops (norms, gelu, retention, GroupNorm + gate) of all 32 rows itself from the shared tile.
//   sampling  lanes 0..31 of wave 0, one env each: masked log-softmax + Gumbel-argmax exactly as k_sample (counter n K + k of agent i's key).
// Scratch (HBM, from the caller's workspace; written and read by the same workgroup): per tile of 32 envs and per token row xn [64], rep [64],
// the encoder's q|k|v|g [256] and per block the decoder's k1|v1|k2|v2 [256].  At A = 8 with four blocks a tile's rows are 1.4 MB, at the
// smallest shape (A = 1, one block) 80 KB: they do not fit the 160 KB of LDS beside the tile T in general, so they go through L2.
// Rows of envs >= N in the last tile shadow env N - 1 (loads clamped) and are never stored outside the scratch.
//
// Summation order: a dense layer sums k in k_linear_pro's order (MFMA step (u, j) holds k = 4 u + j and 32 + 4 u + j); the retention sums its
// dot products and its agents in ascending order on the VALU -- not the order of the team kernels' MFMA products, so the two acting paths
// agree to rounding, not bit for bit.  The value head, the logit head and the reported log-prob are evaluated in double from the fp32 trunk rows
// (fa_head_stream, the sampling block); the sampled action on equal fp32 logits is k_sample's bit for bit.  No atomics: two launches on equal inputs give identical bits.
#include "common.hpp"
#include <string.h>

namespace magpo {

constexpr int FA_MAXA = 8, FA_MAXB = 4, FA_ENVS = 32;
constexpr int FA_TP = 256 + LDP;   // pitch of the LDS tile (floats): bank = 4 row + c, the row-per-lane ds_read_b128 pattern is conflict-free
constexpr float FA_FMIN = -3.4028234663852886e38f;   // jnp.finfo(float32).min masks illegal actions

struct FfBlk {
  const float *qkvg_t, *wo_t, *ln1, *ln2, *gn_g, *gn_b;
  const float *qkvg1_t, *wo1_t, *dln1, *gn1_g, *gn1_b;
  const float *q2_t, *kvg2_t, *wo2_t, *dln2, *dln3, *gn2_g, *gn2_b;
};
struct FfActArgs {
  const float* obs; const unsigned char* mask; const uint32_t* keys_dev;
  const float *s_obs, *W_obs, *s_encln, *W_act, *s_decln;
  const float *vh0_t, *vh0_b, *vh_s, *vh_w, *vh_b1;
  const float *h0_t, *h0_b, *h_s, *h1_t, *h1_b;
  float* scratch; int* action; float* logp; float* value;
  FfBlk blk[FA_MAXB];
  uint32_t keys[FA_MAXA][2];
  int N, A, K, F, nb, nh, hs, gs, value_only, ldo;
};

struct FaFrag { float4 v[8]; };   // features 32 h + 4 u .. + 3 of the lane's row

__device__ __forceinline__ FaFrag fa_load(const float* p) {
  FaFrag f;
#pragma unroll
  for (int u = 0; u < 8; ++u) f.v[u] = *reinterpret_cast<const float4*>(p + 4 * u);
  return f;
}
__device__ __forceinline__ void fa_store(float* p, const FaFrag& f) {
#pragma unroll
  for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(p + 4 * u) = f.v[u];
}
__device__ __forceinline__ float fa_sum4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// x = rmsnorm(x) * scale over the 64 features of the row (the two lane halves).  The statistic and the scaling in double, one rounding per
// element (linear.hip's rms_inplace rounds the statistic, rstd * scale and the product): a norm follows every layer, so this is most of the
// trunk's VALU rounding
__device__ __forceinline__ void fa_rms(FaFrag& x, const float* __restrict__ scale, int h) {
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
    s += ((double)x.v[u].x * x.v[u].x + (double)x.v[u].y * x.v[u].y) + ((double)x.v[u].z * x.v[u].z + (double)x.v[u].w * x.v[u].w);
  s += __shfl_xor(s, 32, 64);
  const double rstd = 1.0 / sqrt(s * (1.0 / 64.0) + 1e-6);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 sc = *reinterpret_cast<const float4*>(scale + 32 * h + 4 * u);
    x.v[u].x = (float)(x.v[u].x * (rstd * sc.x)); x.v[u].y = (float)(x.v[u].y * (rstd * sc.y));
    x.v[u].z = (float)(x.v[u].z * (rstd * sc.z)); x.v[u].w = (float)(x.v[u].w * (rstd * sc.w));
  }
}
// gelu of the two embeddings with libm's tanhf: gelu_tanh's hardware exp / rcp form has an absolute error of ~1e-7, twice an fp32 rounding of
// these O(1) values, and everything downstream inherits it (32 values per row and embedding: the cost does not show)
__device__ __forceinline__ float fa_gelu1(float x) {
  return 0.5f * x * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * x * x * x)));
}
__device__ __forceinline__ void fa_gelu(FaFrag& x) {
#pragma unroll
  for (int u = 0; u < 8; ++u) { x.v[u].x = fa_gelu1(x.v[u].x); x.v[u].y = fa_gelu1(x.v[u].y); x.v[u].z = fa_gelu1(x.v[u].z); x.v[u].w = fa_gelu1(x.v[u].w); }
}
// The two heads (value: rep -> Dense 64 -> gelu -> rmsnorm -> . w; logits: x -> Dense 64 -> gelu -> rmsnorm -> Dense K) end in the outputs with
// nothing after them, so every rounding in them lands in value / logp at full size.  They are evaluated in double on the VALU from the fp32
// row fragment (64 x 64 + 64 K products per row: 3 % of a row's work) and rounded once; what is left is the error of the fp32 trunk.
// fa_dot_d: the lane's half of k of one output; the partner lane holds the other half
__device__ __forceinline__ double fa_dot_d(const FaFrag& x, const float* __restrict__ w) {
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 wv = *reinterpret_cast<const float4*>(w + 4 * u);
    s += (double)x.v[u].x * (double)wv.x; s += (double)x.v[u].y * (double)wv.y; s += (double)x.v[u].z * (double)wv.z; s += (double)x.v[u].w * (double)wv.w;
  }
  return s;
}
__device__ __forceinline__ double fa_gelu_d(double x) {
  return 0.5 * x * (1.0 + tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)));
}
// Streams the 64 outputs o_n = gelu((x Wt^T + bias)_n) * scale_n of a head's first layer in double; the lane whose half holds n calls
// f(n, o_n).  Returns the row's rstd: rmsnorm(.) * scale is o_n times that common factor, which the caller applies to its sums.
// (A rolled loop: the unrolled form kept every weight row in flight and spilled.)
template <typename F>
__device__ __forceinline__ double fa_head_stream(const FaFrag& x, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                 const float* __restrict__ scale, int h, F&& f) {
  double ss = 0.0;
#pragma unroll 1
  for (int n = 0; n < 64; ++n) {
    double s = fa_dot_d(x, Wt + n * 64 + 32 * h);
    s += __shfl_xor(s, 32, 64);
    if ((n >> 5) == h) {
      const double g = fa_gelu_d(s + (double)bias[n]);
      ss += g * g;
      f(n, g * (double)scale[n]);
    }
  }
  ss += __shfl_xor(ss, 32, 64);
  return 1.0 / sqrt(ss * (1.0 / 64.0) + 1e-6);
}
__device__ __forceinline__ void fa_add(FaFrag& x, const FaFrag& y) {
#pragma unroll
  for (int u = 0; u < 8; ++u) { x.v[u].x += y.v[u].x; x.v[u].y += y.v[u].y; x.v[u].z += y.v[u].z; x.v[u].w += y.v[u].w; }
}

// 32 rows x 32 columns n0 .. n0 + 31 of X Wt^T (Wt [n][64]): the lane's row fragment against the lane's column of Wt, k in k_linear_pro's order
__device__ __forceinline__ f32x16 fa_mma(const FaFrag& x, const float* __restrict__ Wt, int n0, int lr, int h) {
  const float* wp = Wt + (long)(n0 + lr) * 64 + 32 * h;
  float4 w[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) w[u] = *reinterpret_cast<const float4*>(wp + 4 * u);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.v[u].x, w[u].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.v[u].y, w[u].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.v[u].z, w[u].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.v[u].w, w[u].w, acc, 0, 0, 0);
  }
  return acc;
}
// the accumulator's column (this lane's) into a row-major tile: row r of the tile at base + r * pitch
__device__ __forceinline__ void fa_put(float* base, long pitch, int col, const f32x16& acc, float bias, int h) {
#pragma unroll
  for (int i = 0; i < 16; ++i) base[(long)((i & 3) + 8 * (i >> 2) + 4 * h) * pitch + col] = acc[i] + bias;
}

// r += (q . k_j per head) v_j for one key row: the lane's halves of q, k_j, v_j
__device__ __forceinline__ void fa_ret_add(FaFrag& r, const FaFrag& q, const FaFrag& k, const FaFrag& v, int hs) {
  double dl = 0.0, dh = 0.0;   // features 0..15 / 16..31 of the lane's half; the dot products in double, rounded once
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    dl += ((double)q.v[u].x * k.v[u].x + (double)q.v[u].y * k.v[u].y) + ((double)q.v[u].z * k.v[u].z + (double)q.v[u].w * k.v[u].w);
    dh += ((double)q.v[u + 4].x * k.v[u + 4].x + (double)q.v[u + 4].y * k.v[u + 4].y) + ((double)q.v[u + 4].z * k.v[u + 4].z + (double)q.v[u + 4].w * k.v[u + 4].w);
  }
  if (hs >= 32) {
    dl += dh;
    if (hs == 64) dl += __shfl_xor(dl, 32, 64);
    dh = dl;
  }
  const float lo = (float)dl, hi = (float)dh;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float d = u < 4 ? lo : hi;
    r.v[u].x += d * v.v[u].x; r.v[u].y += d * v.v[u].y; r.v[u].z += d * v.v[u].z; r.v[u].w += d * v.v[u].w;
  }
}
// retention epilogue (retention.py:289-294) as k_team_ret_fwd's: u = swish(g) * GroupNorm(r), groups of gs (4 / 16 / 64) consecutive channels,
// gamma / beta [hs] shared by the heads.  In place on r.
__device__ __forceinline__ void fa_ret_post(FaFrag& r, const FaFrag& g, const float* __restrict__ gamma, const float* __restrict__ beta,
                                            int hs, int gs, int h) {
  float s1[8], s2[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    s1[u] = (r.v[u].x + r.v[u].y) + (r.v[u].z + r.v[u].w);
    s2[u] = fa_sum4(r.v[u], r.v[u]);
  }
  if (gs >= 16) {
#pragma unroll
    for (int b = 0; b < 8; b += 4) {
      const float a1 = (s1[b] + s1[b + 1]) + (s1[b + 2] + s1[b + 3]), a2 = (s2[b] + s2[b + 1]) + (s2[b + 2] + s2[b + 3]);
#pragma unroll
      for (int u = b; u < b + 4; ++u) { s1[u] = a1; s2[u] = a2; }
    }
    if (gs == 64) {
      float a1 = s1[0] + s1[4], a2 = s2[0] + s2[4];
      a1 += __shfl_xor(a1, 32, 64); a2 += __shfl_xor(a2, 32, 64);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s1[u] = a1; s2[u] = a2; }
    }
  }
  const float inv = 1.0f / (float)gs;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float mu = s1[u] * inv, m2 = s2[u] * inv;
    const float rstd = rsqrtf(fmaxf(m2 - mu * mu, 0.f) + 1e-6f);
    const int c = (32 * h + 4 * u) & (hs - 1);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    r.v[u].x = swishf_(g.v[u].x) * ((r.v[u].x - mu) * rstd * ga.x + be.x);
    r.v[u].y = swishf_(g.v[u].y) * ((r.v[u].y - mu) * rstd * ga.y + be.y);
    r.v[u].z = swishf_(g.v[u].z) * ((r.v[u].z - mu) * rstd * ga.z + be.z);
    r.v[u].w = swishf_(g.v[u].w) * ((r.v[u].w - mu) * rstd * ga.w + be.w);
  }
}

__global__ __launch_bounds__(256) void k_ff_sable_act(FfActArgs a) {
  __shared__ __align__(16) float T[FA_ENVS * FA_TP];
  __shared__ int sprev[FA_ENVS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, h = lane >> 5;
  const int A = a.A, nb = a.nb, hs = a.hs, gs = a.gs, K = a.K;
  const long env = (long)blockIdx.x * FA_ENVS + lr;          // the lane's env; rows of envs >= N shadow env N - 1
  const long envc = env < a.N ? env : (long)a.N - 1;
  const long trows = (long)FA_ENVS * A;                      // token rows of the tile; row of (env lr, agent x) = lr A + x
  float* tb = a.scratch + (long)blockIdx.x * trows * (384 + 256 * nb);
  float* XN = tb;
  float* REP = tb + trows * 64;
  float* QE = tb + trows * 128;
  float* KVD = tb + trows * 384;                             // [nb][trows][256]: k1 | v1 | k2 | v2
  float* Tl = T + lr * FA_TP + 32 * h;                       // the lane's half row of the LDS tile

  // ------------------------------------------------------------------ encoder: wave w carries agents w and w + 4
  for (int b = 0; b < nb; ++b) {
    const FfBlk& B = a.blk[b];
    for (int a0 = 0; a0 < A; a0 += 4) {
      const int ag = a0 + wave;
      if (ag < A) {
        const long row = lr * A + ag;
        FaFrag x;
        if (b == 0) {   // x = rmsnorm(gelu((rmsnorm_F(obs) * s_obs) W_obs)) * s_encln   (k_linear_pro: PRO_EMBED_OBS)
          const float* o = a.obs + (envc * A + ag) * a.ldo;
          float ms = 0.f;
          for (int f = 0; f < a.F; ++f) ms += o[f] * o[f];
          const float rstd = rsqrtf(ms / (float)a.F + 1e-6f);
#pragma unroll
          for (int u = 0; u < 8; ++u) x.v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          for (int f = 0; f < a.F; ++f) {
            const float of = o[f] * rstd * a.s_obs[f];
            const float* wp = a.W_obs + (long)f * 64 + 32 * h;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const float4 w = *reinterpret_cast<const float4*>(wp + 4 * u);
              x.v[u].x += of * w.x; x.v[u].y += of * w.y; x.v[u].z += of * w.z; x.v[u].w += of * w.w;
            }
          }
          fa_gelu(x);
        } else {        // x = rmsnorm(rep of the previous block) * s_encln
          x = fa_load(REP + row * 64 + 32 * h);
        }
        fa_rms(x, a.s_encln, h);
        fa_store(XN + row * 64 + 32 * h, x);
        for (int cg = 0; cg < 8; ++cg) fa_put(QE + (long)ag * 256, (long)A * 256, 32 * cg + lr, fa_mma(x, B.qkvg_t, 32 * cg, lr, h), 0.f, h);
      }
    }
    __syncthreads();   // the team's q | k | v | g rows are complete
    for (int a0 = 0; a0 < A; a0 += 4) {
      const int ag = a0 + wave;
      const bool on = ag < A;
      const long row = lr * A + (on ? ag : 0);
      float* Tw = T + 64 * wave;   // the wave's own 32 x 64 columns of the tile
      FaFrag r;
      if (on) {
        const float* qrow = QE + row * 256 + 32 * h;
        const FaFrag q = fa_load(qrow);
#pragma unroll
        for (int u = 0; u < 8; ++u) r.v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < A; ++j) {   // unmasked: every agent of the team
          const float* kv = QE + (long)(lr * A + j) * 256 + 32 * h;
          fa_ret_add(r, q, fa_load(kv + 64), fa_load(kv + 128), hs);
        }
        fa_ret_post(r, fa_load(qrow + 192), B.gn_g, B.gn_b, hs, gs, h);
        for (int cg = 0; cg < 2; ++cg) fa_put(Tw, FA_TP, 32 * cg + lr, fa_mma(r, B.wo_t, 32 * cg, lr, h), 0.f, h);
      }
      __syncthreads();
      if (on) {          // rep = rmsnorm(rmsnorm(xn + y) * ln1) * ln2
        r = fa_load(XN + row * 64 + 32 * h);
        fa_add(r, fa_load(Tl + 64 * wave));
        fa_rms(r, B.ln1, h);
        fa_rms(r, B.ln2, h);
        fa_store(REP + row * 64 + 32 * h, r);
      }
      if (b == nb - 1 && on) {   // value head: v = (rmsnorm(gelu(rep W_0 + b_0)) * s) . w + b_1, in double from the fp32 rep row
        double s = 0.0;
        const float* __restrict__ vw = a.vh_w;
        const double rstd = fa_head_stream(r, a.vh0_t, a.vh0_b, a.vh_s, h, [&](int n, double o) { s += o * (double)vw[n]; });
        s += __shfl_xor(s, 32, 64);
        if (h == 0 && env < a.N) a.value[env * A + ag] = (float)(rstd * s + (double)a.vh_b1[0]);
      }
      __syncthreads();
    }
  }
  if (a.value_only) return;

  // ------------------------------------------------------------------ decoder: A sequential iterations, column groups split over the waves
  if (tid < FA_ENVS) sprev[tid] = 0;   // start token
  __syncthreads();
  for (int i = 0; i < A; ++i) {
    const long row = lr * A + i;
    const FaFrag rep = fa_load(REP + row * 64 + 32 * h);
    FaFrag x;   // the block's input row (every wave holds all 32 rows)
    {           // x = rmsnorm(gelu(W_act[prev])) * s_decln   (PRO_EMBED_ACT)
      x = fa_load(a.W_act + (long)sprev[lr] * 64 + 32 * h);
      fa_gelu(x);
      fa_rms(x, a.s_decln, h);
    }
    for (int b = 0; b < nb; ++b) {
      const FfBlk& B = a.blk[b];
      float* kvd = KVD + (long)b * trows * 256;
      // q1 | k1 | v1 | g1 = x W_qkvg1: groups 0, 1 (q) and 6, 7 (g) into the tile's columns 0..127, 2..5 (k | v) into the scratch rows of agent i
      for (int cg = wave; cg < 8; cg += 4) {
        const f32x16 acc = fa_mma(x, B.qkvg1_t, 32 * cg, lr, h);
        if (cg < 2) fa_put(T, FA_TP, 32 * cg + lr, acc, 0.f, h);
        else if (cg >= 6) fa_put(T, FA_TP, 32 * (cg - 4) + lr, acc, 0.f, h);
        else fa_put(kvd + (long)i * 256, (long)A * 256, 32 * (cg - 2) + lr, acc, 0.f, h);
      }
      __syncthreads();
      FaFrag r;
      {   // self-retention of token i over the decoder tokens j <= i, GroupNorm + gate, W_o1
        const FaFrag q = fa_load(Tl);
#pragma unroll
        for (int u = 0; u < 8; ++u) r.v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j <= i; ++j) {
          const float* kv = kvd + (long)(lr * A + j) * 256 + 32 * h;
          fa_ret_add(r, q, fa_load(kv), fa_load(kv + 64), hs);
        }
        fa_ret_post(r, fa_load(Tl + 64), B.gn1_g, B.gn1_b, hs, gs, h);
        if (wave < 2) fa_put(T, FA_TP, 128 + 32 * wave + lr, fa_mma(r, B.wo1_t, 32 * wave, lr, h), 0.f, h);
      }
      __syncthreads();
      {   // c = rmsnorm(x + y1) * ln1;  k2 | v2 | g2 = c W_kvg2;  q2 = rep W_q2
        r = fa_load(Tl + 128);
        fa_add(r, x);
        fa_rms(r, B.dln1, h);
        for (int cg = wave; cg < 6; cg += 4) {
          const f32x16 acc = fa_mma(r, B.kvg2_t, 32 * cg, lr, h);
          if (cg < 4) fa_put(kvd + (long)i * 256 + 128, (long)A * 256, 32 * cg + lr, acc, 0.f, h);
          else fa_put(T, FA_TP, 64 + 32 * (cg - 4) + lr, acc, 0.f, h);
        }
        if (wave >= 2) fa_put(T, FA_TP, 32 * (wave - 2) + lr, fa_mma(rep, B.q2_t, 32 * (wave - 2), lr, h), 0.f, h);
      }
      __syncthreads();
      {   // cross-retention of q2 over the k2 | v2 rows j <= i, GroupNorm + gate, W_o2
        const FaFrag q = fa_load(Tl);
#pragma unroll
        for (int u = 0; u < 8; ++u) r.v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j <= i; ++j) {
          const float* kv = kvd + (long)(lr * A + j) * 256 + 128 + 32 * h;
          fa_ret_add(r, q, fa_load(kv), fa_load(kv + 64), hs);
        }
        fa_ret_post(r, fa_load(Tl + 64), B.gn2_g, B.gn2_b, hs, gs, h);
        if (wave < 2) fa_put(T, FA_TP, 128 + 32 * wave + lr, fa_mma(r, B.wo2_t, 32 * wave, lr, h), 0.f, h);
      }
      __syncthreads();
      // x = rmsnorm(rmsnorm(rep + y2) * ln2) * ln3: the next block's input, or the logit head's
      x = fa_load(Tl + 128);
      fa_add(x, rep);
      fa_rms(x, B.dln2, h);
      fa_rms(x, B.dln3, h);
    }
    // logit head: logits = (rmsnorm(gelu(x W_0 + b_0)) * s) W_1 + b_1
    if (wave == 0) {   // in double from the fp32 row x; row lr's logits into the tile: floats at columns 0 .. K-1, doubles from column 64
      double lacc[31];   // rows K .. 30 of the padded W_1^T are zero
#pragma unroll
      for (int k = 0; k < 31; ++k) lacc[k] = 0.0;
      const float* __restrict__ w1 = a.h1_t;
      const double rstd = fa_head_stream(x, a.h0_t, a.h0_b, a.h_s, h, [&](int n, double o) {
#pragma unroll
        for (int k = 0; k < 31; ++k) lacc[k] += o * (double)w1[k * 64 + n];
      });
      double* ld = reinterpret_cast<double*>(T + lr * FA_TP + 64);
#pragma unroll
      for (int k = 0; k < 31; ++k) {
        double s = lacc[k];
        s += __shfl_xor(s, 32, 64);
        if (h == 0 && k < K) {
          s = rstd * s + (double)a.h1_b[k];
          ld[k] = s;
          T[lr * FA_TP + k] = (float)s;
        }
      }
    }
    __syncthreads();
    if (tid < FA_ENVS) {   // masked log-softmax + Gumbel-argmax of env `env` (rl.hip: k_sample)
      int arg = 0;
      if (env < a.N) {
        const uint32_t k0 = a.keys_dev ? a.keys_dev[2 * i] : a.keys[i][0], k1 = a.keys_dev ? a.keys_dev[2 * i + 1] : a.keys[i][1];
        const float* xl = T + lr * FA_TP;
        const unsigned char* m = a.mask ? a.mask + (env * A + i) * K : nullptr;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, (m && !m[k]) ? FA_FMIN : xl[k]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(((m && !m[k]) ? FA_FMIN : xl[k]) - mx);
        const float lse = mx + logf(se);
        float best = -INFINITY, best_lp = 0.f;
        for (int k = 0; k < K; ++k) {
          const float lp = ((m && !m[k]) ? FA_FMIN : xl[k]) - lse;
          const float v = gumbel_exact_from_bits(random_bits32(k0, k1, (uint32_t)(env * K + k))) + lp;
          if (v > best) { best = v; arg = k; best_lp = lp; }
        }
        // the action is k_sample's on the fp32 logits, bit for bit; its reported log-prob is taken from the double logits and rounded once
        const double* ld = reinterpret_cast<const double*>(T + lr * FA_TP + 64);
        double mxd = -INFINITY, sd = 0.0;
        for (int k = 0; k < K; ++k) mxd = fmax(mxd, (m && !m[k]) ? (double)FA_FMIN : ld[k]);
        for (int k = 0; k < K; ++k) sd += exp(((m && !m[k]) ? (double)FA_FMIN : ld[k]) - mxd);
        best_lp = (float)(((m && !m[arg]) ? (double)FA_FMIN : ld[arg]) - (mxd + log(sd)));
        a.action[env * A + i] = arg;
        a.logp[env * A + i] = best_lp;
      }
      sprev[tid] = arg + 1;
    }
    __syncthreads();
  }
}

}  // namespace magpo

using namespace magpo;

// Tables: see include/magpo.h.
extern "C" int magpo_ff_sable_act(const int* dims_host, const uint32_t* keys_host, const void* const* p, int nptrs, const void* const* bp,
                                  int nblk_ptrs, long scratch_floats, hipStream_t st) {
  constexpr int NG = 22, NBP = 18;
  if (!dims_host || !p || !bp) { set_error("magpo_ff_sable_act: null dims or pointer table"); return MAGPO_EINVAL; }
  FfActArgs a;
  memset(&a, 0, sizeof(a));
  a.N = dims_host[0]; a.A = dims_host[1]; a.K = dims_host[2]; a.F = dims_host[3]; a.nb = dims_host[4]; a.nh = dims_host[5];
  a.hs = dims_host[6]; a.gs = dims_host[7]; a.value_only = dims_host[8] ? 1 : 0; a.ldo = dims_host[9];
  if (a.N < 1) { set_error("magpo_ff_sable_act: N must be at least 1"); return MAGPO_EINVAL; }
  if (a.A < 1 || a.A > FA_MAXA) { set_error("magpo_ff_sable_act: 1 <= A <= 8 required"); return MAGPO_EINVAL; }
  if (a.nb < 1 || a.nb > FA_MAXB) { set_error("magpo_ff_sable_act: 1 <= n_block <= 4 required"); return MAGPO_EINVAL; }
  if ((a.nh != 1 && a.nh != 2 && a.nh != 4) || a.hs * a.nh != 64 || a.gs * a.nh != a.hs) {
    set_error("magpo_ff_sable_act: n_head must be 1, 2 or 4 with hs = 64 / n_head and gs = hs / n_head (64-wide rows)");
    return MAGPO_EINVAL;
  }
  if (a.K < 1 || a.K > 31) { set_error("magpo_ff_sable_act: 1 <= K <= 31 required"); return MAGPO_EINVAL; }
  if (a.F < 1 || a.F > 128 || a.ldo < a.F) { set_error("magpo_ff_sable_act: 1 <= F <= 128 and obs_ld >= F required"); return MAGPO_EINVAL; }
  if (nptrs != NG || nblk_ptrs != NBP * a.nb) { set_error("magpo_ff_sable_act: pointer table size mismatch (22 global, 18 per block)"); return MAGPO_EINVAL; }
  if ((long)a.N * a.K >= (1L << 32)) { set_error("magpo_ff_sable_act: N K must be < 2^32"); return MAGPO_EINVAL; }
  const long tiles = ((long)a.N + FA_ENVS - 1) / FA_ENVS;
  const long need = tiles * FA_ENVS * a.A * (384 + 256 * a.nb);
  if (scratch_floats < need) { set_error("magpo_ff_sable_act: scratch too small (32 ceil(N / 32) A (384 + 256 n_block) floats)"); return MAGPO_EINVAL; }
  for (int i = 0; i < NG; ++i) {
    const bool optional = i == 1 || i == 2 || (a.value_only && (i == 19 || i == 20));
    if (!p[i] && !optional) { set_error("magpo_ff_sable_act: null pointer in a required slot of the global table"); return MAGPO_EINVAL; }
  }
  for (int i = 0; i < NBP * a.nb; ++i)
    if (!bp[i]) { set_error("magpo_ff_sable_act: null pointer in the per-block table"); return MAGPO_EINVAL; }
  if (!a.value_only && !keys_host && !p[2]) { set_error("magpo_ff_sable_act: no sampling keys"); return MAGPO_EINVAL; }
  if (keys_host) for (int i = 0; i < a.A; ++i) { a.keys[i][0] = keys_host[2 * i]; a.keys[i][1] = keys_host[2 * i + 1]; }
  int q = 0;
#define P(Tp, f) a.f = (Tp)p[q++];
  P(const float*, obs) P(const unsigned char*, mask) P(const uint32_t*, keys_dev)
  P(const float*, s_obs) P(const float*, W_obs) P(const float*, s_encln) P(const float*, W_act) P(const float*, s_decln)
  P(const float*, vh0_t) P(const float*, vh0_b) P(const float*, vh_s) P(const float*, vh_w) P(const float*, vh_b1)
  P(const float*, h0_t) P(const float*, h0_b) P(const float*, h_s) P(const float*, h1_t) P(const float*, h1_b)
  P(float*, scratch) P(int*, action) P(float*, logp) P(float*, value)
#undef P
  if (keys_host) a.keys_dev = nullptr;   // keys by value win
  for (int b = 0; b < a.nb; ++b) {
    const void* const* s = bp + NBP * b;
    FfBlk& B = a.blk[b];
    B.qkvg_t = (const float*)s[0]; B.wo_t = (const float*)s[1]; B.ln1 = (const float*)s[2]; B.ln2 = (const float*)s[3];
    B.gn_g = (const float*)s[4]; B.gn_b = (const float*)s[5];
    B.qkvg1_t = (const float*)s[6]; B.wo1_t = (const float*)s[7]; B.dln1 = (const float*)s[8]; B.gn1_g = (const float*)s[9]; B.gn1_b = (const float*)s[10];
    B.q2_t = (const float*)s[11]; B.kvg2_t = (const float*)s[12]; B.wo2_t = (const float*)s[13]; B.dln2 = (const float*)s[14]; B.dln3 = (const float*)s[15];
    B.gn2_g = (const float*)s[16]; B.gn2_b = (const float*)s[17];
  }
  hipLaunchKernelGGL(k_ff_sable_act, dim3((unsigned)tiles), dim3(256), 0, st, a);
  return check_launch("magpo_ff_sable_act");
}
