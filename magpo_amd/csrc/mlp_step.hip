// One acting step of feed-forward PPO (ff_ippo / ff_mappo: mava/systems/ppo/anakin/ff_mappo.py:75-100), for one or two networks (actor,
// critic) in a single launch:  Y = head(MLPTorso(X))  on R rows, per layer Dense -> activation (mava/networks/torsos.py:36-47 without
// LayerNorm), then the head Dense(NOUT) without activation.
//
// Composed from the dense kernels an acting step is one launch per layer and network, and every hidden activation ([R][width]) is
// written to HBM by one launch and read by the next.  Here a block takes 64 rows through the whole torso and the head with the
// activations in LDS; what reaches HBM is the NOUT columns of the head.
//
// Grid (ceil(R / 64), nnets), 256 threads.  Two LDS tiles [64][P] (P = widest operand of the launch + 4), used in turn as a layer's input
// and output, so a layer needs one barrier (after its writes).  The rows are staged once: rows beyond R shadow row R - 1 and are never
// stored; only columns < F of a row are read (scalar loads: a row may start at any 4-byte boundary).
//
// Summation order.  Every product chain is summed in the order of the composed path's kernel for that layer, so the two paths sum the
// same products in the same order:
//   first layer, F <= 32, Dense(128) + ReLU ("small"): magpo_small_linear's chain on the VALU, acc = b, then acc += x[f] W[f][n] for
//       f = 0 .. F - 1, from the natural-layout weights [F][128];
//   every other layer, and the head: k_linear_lds's chain on v_mfma_f32_32x32x2_f32 from zero, lane half h of MFMA step (c, u, j) holding
//       k = 64 c + 32 h + 4 u + j, the bias added to the finished sum, then fmaxf(., 0) / tanhf.  A first layer that is not "small" reads
//       the rows zero-extended to KP = 64 (F <= 32) or 128 columns against Wt [width][KP] with zero columns beyond F, which is the
//       operand magpo_small_operand / the padded observation rows give the composed path.
// The weights stream from L2, one 128-byte line per lane and 64-k chunk, the next chunk requested before the MFMAs of the current one.
// Wave w owns the column groups w, w + 4 of a layer (32 columns each) for both 32-row halves; the head (one column group) is computed
// by waves 0 and 1, one row half each.
#include "common.hpp"

namespace magpo {

constexpr int MLP_MAXL = 3;
constexpr int MLP_ACT_RELU = 1, MLP_ACT_TANH = 5;   // magpo_linear's codes

struct MlpNet {
  const float* X;              // [R] rows of F features, ldx floats apart
  const float* W[MLP_MAXL];    // layer 0: [F][128] natural ("small") or Wt [wd0][KP]; layer i > 0: Wt [wd_i][wd_{i-1}]
  const float* b[MLP_MAXL];
  const float* Wh;             // Wt [>= 32][wd_last], rows >= nout never reach the output
  const float* bh;             // [nout]
  float* Y;                    // [R] rows of nout values, ldy floats apart
  int F, ldx, nl, nout, ldy, small;
  int wd[MLP_MAXL], act[MLP_MAXL];   // act: 0 none, 1 relu, 5 tanh
};
struct MlpArgs {
  MlpNet net[2];
  int R, P;                    // P: LDS tile pitch in floats
};

#define MLP_MFMA4(ACC, X, W)                                          \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.x, W.x, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.y, W.y, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.z, W.z, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.w, W.w, ACC, 0, 0, 0);

// acc[q] += rows (a0 + 32 q P) x the lane's weight row, NK chunks of 64 k in k_linear_lds's order.  wrow = the lane's column of Wt,
// already offset by 32 h; a0 = the lane's row of the input tile, offset by 32 h.
template <int NQ>
__device__ __forceinline__ void mlp_chain(const float* __restrict__ wrow, int NK, const float* a0, int P, f32x16 (&acc)[NQ]) {
  float4 wa[8], wb[8];
  auto loadw = [&](int c, float4 (&dst)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[u] = *reinterpret_cast<const float4*>(wrow + 64 * c + 4 * u);
  };
  auto mma = [&](int c, const float4 (&w)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(a0 + q * 32 * P + 64 * c + 4 * u);
        MLP_MFMA4(acc[q], x, w[u])
      }
    }
  };
  loadw(0, wa);
  for (int c = 0; c < NK; c += 2) {
    const bool two = c + 1 < NK;
    if (two) loadw(c + 1, wb);
    mma(c, wa);
    if (two) {
      if (c + 2 < NK) loadw(c + 2, wa);
      mma(c + 1, wb);
    }
  }
}
#undef MLP_MFMA4

__device__ __forceinline__ float mlp_act(float v, int act) {
  if (act == MLP_ACT_RELU) return fmaxf(v, 0.f);
  if (act == MLP_ACT_TANH) return tanhf(v);
  return v;
}

// out[64][N] = act(in[64][K] Wt^T + b)
__device__ __forceinline__ void mlp_layer(const float* __restrict__ Wt, const float* __restrict__ bias, int K, int N, int act,
                                          const float* in, float* out, int P) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, h = lane >> 5;
  for (int cg = wave; cg < N / 32; cg += 4) {
    const int col = 32 * cg + lr;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
    mlp_chain<2>(Wt + (long)col * K + 32 * h, K / 64, in + lr * P + 32 * h, P, acc);
    const float bv = bias[col];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int rl = 32 * q + (i & 3) + 8 * (i >> 2) + 4 * h;
        out[rl * P + col] = mlp_act(acc[q][i] + bv, act);
      }
  }
}

__global__ __launch_bounds__(256) void k_mlp_act_step(MlpArgs a) {
  extern __shared__ __align__(16) float mlp_smem[];
  const MlpNet& n = a.net[blockIdx.y ? 1 : 0];
  const int R = a.R, P = a.P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, h = lane >> 5;
  const int rho0 = blockIdx.x * 64;
  float* in = mlp_smem + 64 * P;   // the staged rows
  float* out = mlp_smem;
  const int F = n.F, ldx = n.ldx;
  const float* __restrict__ X = n.X;

  if (n.small) {
    // rows compact [64][F]; Dense(F -> 128) + ReLU as magpo_small_linear sums it
    for (int i = tid; i < 64 * F; i += 256) {
      const int r = i / F, c = i - r * F;
      in[i] = X[(long)min(rho0 + r, R - 1) * ldx + c];
    }
    __syncthreads();
    const int c4 = 4 * (tid & 31), slot = tid >> 5;
    const float* __restrict__ W = n.W[0];
    const float4 bias = *reinterpret_cast<const float4*>(n.b[0] + c4);
    float4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bias;
    for (int f = 0; f < F; ++f) {
      const float4 w = *reinterpret_cast<const float4*>(W + f * 128 + c4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = in[(slot + 8 * j) * F + f];
        acc[j].x += xv * w.x; acc[j].y += xv * w.y; acc[j].z += xv * w.z; acc[j].w += xv * w.w;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float4 v = acc[j];
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      *reinterpret_cast<float4*>(&out[(slot + 8 * j) * P + c4]) = v;
    }
  } else {
    const int KP = F <= 32 ? 64 : 128;
    for (int i = tid; i < 64 * KP; i += 256) {
      const int r = i / KP, c = i - r * KP;
      in[r * P + c] = c < F ? X[(long)min(rho0 + r, R - 1) * ldx + c] : 0.f;
    }
    __syncthreads();
    mlp_layer(n.W[0], n.b[0], KP, n.wd[0], n.act[0], in, out, P);
  }
  __syncthreads();
  int K = n.wd[0];
#pragma unroll
  for (int l = 1; l < MLP_MAXL; ++l) {
    if (l < n.nl) {
      float* t = in; in = out; out = t;
      mlp_layer(n.W[l], n.b[l], K, n.wd[l], n.act[l], in, out, P);
      K = n.wd[l];
      __syncthreads();
    }
  }
  // head: waves 0 and 1, one 32-row half each
  if (wave < 2 && rho0 + 32 * wave < R) {
    f32x16 acc[1];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
    mlp_chain<1>(n.Wh + (long)lr * K + 32 * h, K / 64, out + (32 * wave + lr) * P + 32 * h, P, acc);
    const int nout = n.nout, ldy = n.ldy;
    if (lr < nout) {
      const float bv = n.bh[lr];
      float* __restrict__ Y = n.Y;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = rho0 + 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (row < R) Y[(long)row * ldy + lr] = acc[0][i] + bv;
      }
    }
  }
}

}  // namespace magpo

using namespace magpo;

// Tables: see include/magpo.h.  dims_host[1 + 10 nnets] = {nnets; per network F, ldx, layers, width 0, width 1, width 2, activation,
// activate_final, NOUT, ldy}; ptrs_host[10 nnets], per network X, W0, b0, W1, b1, W2, b2, Wh, bh, Y.
extern "C" int magpo_mlp_act_step(const int* dims_host, const void* const* p, int nptrs, int R, hipStream_t st) {
  constexpr int ND = 10, NP = 10;
  if (!dims_host || !p) { set_error("magpo_mlp_act_step: null dims or pointer table"); return MAGPO_EINVAL; }
  const int nnets = dims_host[0];
  if (nnets != 1 && nnets != 2) { set_error("magpo_mlp_act_step: nnets must be 1 or 2"); return MAGPO_EINVAL; }
  if (nptrs != NP * nnets) { set_error("magpo_mlp_act_step: pointer table size mismatch (10 per network)"); return MAGPO_EINVAL; }
  if (R < 1) { set_error("magpo_mlp_act_step: R must be at least 1"); return MAGPO_EINVAL; }
  MlpArgs a{};
  int dmax = 0;
  for (int k = 0; k < nnets; ++k) {
    const int* d = dims_host + 1 + ND * k;
    const void* const* q = p + NP * k;
    MlpNet& n = a.net[k];
    n.F = d[0]; n.ldx = d[1]; n.nl = d[2]; n.nout = d[8]; n.ldy = d[9];
    const int act = d[6], final_act = d[7];
    if (n.nl < 1 || n.nl > MLP_MAXL) { set_error("magpo_mlp_act_step: 1 to 3 layers"); return MAGPO_EINVAL; }
    if (n.F < 1 || n.F > 128 || n.ldx < n.F) { set_error("magpo_mlp_act_step: F must be in [1, 128] and ldx >= F"); return MAGPO_EINVAL; }
    if (n.nout < 1 || n.nout > 32 || n.ldy < n.nout) { set_error("magpo_mlp_act_step: NOUT must be in [1, 32] and ldy >= NOUT"); return MAGPO_EINVAL; }
    if (act != MLP_ACT_RELU && act != MLP_ACT_TANH) { set_error("magpo_mlp_act_step: activation must be 1 (relu) or 5 (tanh)"); return MAGPO_EINVAL; }
    if (final_act != 0 && final_act != 1) { set_error("magpo_mlp_act_step: activate_final must be 0 or 1"); return MAGPO_EINVAL; }
    for (int l = 0; l < n.nl; ++l) {
      const int w = d[3 + l];
      if (w != 64 && w != 128 && w != 192 && w != 256) { set_error("magpo_mlp_act_step: layer widths must be 64, 128, 192 or 256"); return MAGPO_EINVAL; }
      n.wd[l] = w;
      n.act[l] = (l < n.nl - 1 || final_act) ? act : 0;
      if (!q[1 + 2 * l] || !q[2 + 2 * l]) { set_error("magpo_mlp_act_step: null weight or bias pointer of a used layer"); return MAGPO_EINVAL; }
      n.W[l] = (const float*)q[1 + 2 * l]; n.b[l] = (const float*)q[2 + 2 * l];
      dmax = w > dmax ? w : dmax;
    }
    if (!q[0] || !q[7] || !q[8] || !q[9]) { set_error("magpo_mlp_act_step: null X, head or Y pointer"); return MAGPO_EINVAL; }
    n.X = (const float*)q[0]; n.Wh = (const float*)q[7]; n.bh = (const float*)q[8]; n.Y = (float*)q[9];
    // the first layer the composed path serves with magpo_small_linear
    n.small = n.F <= 32 && n.wd[0] == 128 && n.act[0] == MLP_ACT_RELU;
    if (!n.small) { const int kp = n.F <= 32 ? 64 : 128; dmax = kp > dmax ? kp : dmax; }
  }
  a.R = R; a.P = dmax + LDP;
  const size_t lds = (size_t)2 * 64 * a.P * sizeof(float);
  static size_t lds_set = 0;   // (memoised device attribute: idempotent)
  if (lds > lds_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mlp_act_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("magpo_mlp_act_step: cannot raise the dynamic LDS limit");
      return MAGPO_ELAUNCH;
    }
    lds_set = lds;
  }
  hipLaunchKernelGGL(k_mlp_act_step, dim3((unsigned)((R + 63) / 64), (unsigned)nnets), dim3(256), lds, st, a);
  return check_launch("magpo_mlp_act_step");
}
