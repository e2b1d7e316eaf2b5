// One GRU cell step for the acting path of recurrent PPO (rec_ippo / rec_mappo: mava/systems/ppo/anakin/rec_mappo.py:96-141), for one
// or two networks (actor, critic) in a single launch.  The recurrence is the one in the header of gru.hip:
//
//   r = sigmoid(x W_ir + b_ir + h W_hr) ; z = sigmoid(x W_iz + b_iz + h W_hz) ; n = tanh(x W_in + b_in + r * (h W_hn + b_hn))
//   h' = (1 - z) n + z h ,   h <- 0 before the step wherever the env's reset flag is set
//
// In PPO the actor's sample drives the environment, so both networks advance one step per env step and nothing is batched over
// time.  The composed step (GruActor.step) is magpo_linear for xi = x W_i + b_i, [R][384] through HBM, then a T = 1 scan.  Here the
// input projection, the recurrent projection and the gate math are one kernel and xi stays in the accumulators.
//
// Grid (ceil(R / 64), nnets), 256 threads.  A block stages its 64 rows of emb ([64][D + 4]) and of h ([64][132], reset applied) in
// LDS; wave w owns hidden columns 32w .. 32w + 31 for both 32-row halves, as in k_gru_scan_fwd.  Per half six fp32 MFMA accumulators:
// the input side and the hidden side of r, z and n, each one chain from zero in the k order of the composed step's kernel (k_linear_lds
// for the input side, k_gru_scan_fwd for the hidden side), with the biases added and the gates formed by the scan's own expressions
// (fast_sigmoid / fast_tanh).  An fp32 MFMA is a k-ordered fma chain, so the fused step sums the same products in the same order as
// the composed one; what is left between the two paths is the compiler's choice of fma contraction in the gate expressions (last-bit
// differences in part of the outputs, the same maximum error against fp64).
// W_i^T [384][D] and W_h^T [384][128] stream from L2 in chunks of 32 k per lane-half (a whole 128-byte line per lane and gate); one
// fetched chunk serves both row halves.  The source asks for the next chunk before the MFMAs of the current one; how far ahead the
// loads really run is the compiler's schedule (132 VGPRs: less than a whole chunk in flight).
// Rows beyond R shadow row R - 1 on the emb load, start from h = 0 and are never stored.  h_out may alias h_in: a block reads only
// its own rows of h_in, all of them before its first store.
#include "common.hpp"

namespace magpo {

constexpr int CH = 128;            // hidden width
constexpr int CHP = CH + LDP;      // h tile pitch

struct CellNet {
  const float* emb;    // [R][D] pre-torso output
  const float* Wit;    // [3H][D]  W_i transposed (row n = output column n of [W_ir|W_iz|W_in])
  const float* bi;     // [3H]
  const float* Wht;    // [3H][H]
  const float* b_hn;   // [H]
  const float* h_in;   // [R][H]
  float* h_out;        // [R][H] (may be h_in)
  int D;
};
struct CellArgs {
  CellNet net[2];
  const unsigned char* reset;   // [ceil(R / A)] reset-before-step flag per env; row r belongs to env r / A
  int R, A;
};

#define CELL_MFMA4(ACC, X, W)                                         \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.x, W.x, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.y, W.y, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.z, W.z, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(X.w, W.w, ACC, 0, 0, 0);

template <int D>
__device__ __forceinline__ void cell_tile(const CellNet& n, const unsigned char* __restrict__ reset, int R, int A, float* smem) {
  constexpr int DP = D + LDP;
  constexpr int NI = D / 64;       // 64-k chunks of the input side: lane half h holds k in [64 c + 32 h, 64 c + 32 h + 32) of chunk c
  constexpr int NC = NI + 2;       // + the hidden side's two
  float* et = smem;                // [64][DP]
  float* ht = smem + 64 * DP;      // [64][CHP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, h = lane >> 5;
  const int rho0 = blockIdx.x * 64;
  const int col = 32 * wave + lr;

  // weight chunk c of this lane: 8 float4 per gate
  float4 w[2][3][8];
  auto loadw = [&](int c, float4 (&dst)[3][8]) {
    const bool in = c < NI;
    const float* base = in ? n.Wit + (long)col * D + 64 * c + 32 * h : n.Wht + (long)col * CH + 64 * h + 32 * (c - NI);
    const long gstride = in ? (long)CH * D : (long)CH * CH;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int u = 0; u < 8; ++u) dst[g][u] = *reinterpret_cast<const float4*>(base + g * gstride + 4 * u);
  };
  loadw(0, w[0]);   // in flight under the staging below

  for (int i = tid; i < 64 * (D / 4); i += 256) {
    const int r = i / (D / 4), c4 = i - r * (D / 4);
    const int rho = min(rho0 + r, R - 1);
    *reinterpret_cast<float4*>(&et[r * DP + 4 * c4]) = *reinterpret_cast<const float4*>(n.emb + (long)rho * D + 4 * c4);
  }
  for (int i = tid; i < 64 * (CH / 4); i += 256) {
    const int r = i / (CH / 4), c4 = i - r * (CH / 4);
    const int rho = rho0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rho < R && !reset[rho / A]) v = *reinterpret_cast<const float4*>(n.h_in + (long)rho * CH + 4 * c4);
    *reinterpret_cast<float4*>(&ht[r * CHP + 4 * c4]) = v;
  }
  const float b_r = n.bi[col], b_z = n.bi[CH + col], b_n = n.bi[2 * CH + col], b_hn = n.b_hn[col];
  __syncthreads();

  // Six accumulators per 32-row half, all from zero: the input side and the hidden side of r, z and n.  Chain order and gate
  // expressions are those of the composed step (k_linear_lds: k = 64 c + 32 h + 4 u + j, bias added to the finished sum;
  // k_gru_scan_fwd: k = 64 h + 4 u + j), and an fp32 MFMA is a k-ordered fma chain: same products, same order, same roundings.
  f32x16 ai[2][3], ah[2][3];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int i = 0; i < 16; ++i) { ai[q][g][i] = 0.f; ah[q][g][i] = 0.f; }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) loadw(c + 1, w[(c + 1) & 1]);
    const bool in = c < NI;
    const float* a0 = in ? et + lr * DP + 64 * c + 32 * h : ht + lr * CHP + 64 * h + 32 * (c - NI);
    const int half = 32 * (in ? DP : CHP);   // the second 32-row half of the tile
    float4 (&wc)[3][8] = w[c & 1];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float4 x = *reinterpret_cast<const float4*>(a0 + q * half + 4 * u);
        if (in) { CELL_MFMA4(ai[q][0], x, wc[0][u]) CELL_MFMA4(ai[q][1], x, wc[1][u]) CELL_MFMA4(ai[q][2], x, wc[2][u]) }
        else { CELL_MFMA4(ah[q][0], x, wc[0][u]) CELL_MFMA4(ah[q][1], x, wc[1][u]) CELL_MFMA4(ah[q][2], x, wc[2][u]) }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int rl = 32 * q + (i & 3) + 8 * (i >> 2) + 4 * h;
      const float xr = ai[q][0][i] + b_r, xz = ai[q][1][i] + b_z, xn = ai[q][2][i] + b_n;   // xi as magpo_linear rounds it
      const float hb = ah[q][2][i] + b_hn;
      const float r = fast_sigmoid(xr + ah[q][0][i]);
      const float z = fast_sigmoid(xz + ah[q][1][i]);
      const float nn = fast_tanh(xn + r * hb);
      const float hp = ht[rl * CHP + col];
      const float hn_new = (1.0f - z) * nn + z * hp;
      if (rho0 + rl < R) n.h_out[(long)(rho0 + rl) * CH + col] = hn_new;
    }
}
#undef CELL_MFMA4

__global__ __launch_bounds__(256, 1) void k_gru_cell_step(CellArgs a) {
  extern __shared__ __align__(16) float cell_smem[];
  const bool second = blockIdx.y != 0;
  CellNet n;
  n.emb = second ? a.net[1].emb : a.net[0].emb;
  n.Wit = second ? a.net[1].Wit : a.net[0].Wit;
  n.bi = second ? a.net[1].bi : a.net[0].bi;
  n.Wht = second ? a.net[1].Wht : a.net[0].Wht;
  n.b_hn = second ? a.net[1].b_hn : a.net[0].b_hn;
  n.h_in = second ? a.net[1].h_in : a.net[0].h_in;
  n.h_out = second ? a.net[1].h_out : a.net[0].h_out;
  n.D = second ? a.net[1].D : a.net[0].D;
  switch (n.D) {   // uniform over the block
    case 64: cell_tile<64>(n, a.reset, a.R, a.A, cell_smem); break;
    case 128: cell_tile<128>(n, a.reset, a.R, a.A, cell_smem); break;
    case 192: cell_tile<192>(n, a.reset, a.R, a.A, cell_smem); break;
    default: cell_tile<256>(n, a.reset, a.R, a.A, cell_smem); break;
  }
}

// gs[(n, a)][c] = raw[(n, c / F_raw)][c % F_raw] for c < A F_raw, 0 beyond: the concatenation over agents of the raw agent views,
// tiled to every agent (mava/wrappers/matrax.py:128-131, jumanji.py:61-67), read from the stored observation rows behind their
// id_cols leading agent-id columns.  One thread per float4 of the output.
__global__ void k_global_state(const float* __restrict__ obs, long ldo, int id_cols, int F_raw, float* __restrict__ out, int ld, long N, int A) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = ld / 4;
  if (i >= N * A * q) return;
  const long row = i / q;
  const int c0 = 4 * (int)(i - row * q);
  const long env = row / A;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + j;
    const int ag = c / F_raw, f = c - ag * F_raw;
    v[j] = ag < A ? obs[(env * A + ag) * ldo + id_cols + f] : 0.f;
  }
  *reinterpret_cast<float4*>(out + row * ld + c0) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace magpo

using namespace magpo;

// dims_host[3] = {nnets, D of network 0, D of network 1 (ignored for one network)}; ptrs_host[7 nnets] (device pointers), per network:
// emb Wit bi Wht b_hn h_in h_out.
extern "C" int magpo_gru_cell_step(const int* dims_host, const void* const* p, int nptrs, const unsigned char* reset, int R, int A,
                                   hipStream_t st) {
  if (!dims_host || !p || !reset) { set_error("magpo_gru_cell_step: null dims, pointer table or reset flags"); return MAGPO_EINVAL; }
  const int nnets = dims_host[0];
  if (nnets != 1 && nnets != 2) { set_error("magpo_gru_cell_step: nnets must be 1 or 2"); return MAGPO_EINVAL; }
  if (nptrs != 7 * nnets) { set_error("magpo_gru_cell_step: pointer table size mismatch (7 per network)"); return MAGPO_EINVAL; }
  if (R < 1 || A < 1) { set_error("magpo_gru_cell_step: R and A must be at least 1"); return MAGPO_EINVAL; }
  CellArgs a{};
  int dmax = 0;
  for (int k = 0; k < nnets; ++k) {
    const int D = dims_host[1 + k];
    if (D != 64 && D != 128 && D != 192 && D != 256) { set_error("magpo_gru_cell_step: D must be 64, 128, 192 or 256"); return MAGPO_EINVAL; }
    for (int j = 0; j < 7; ++j)
      if (!p[7 * k + j]) { set_error("magpo_gru_cell_step: null pointer in the table"); return MAGPO_EINVAL; }
    CellNet& n = a.net[k];
    n.emb = (const float*)p[7 * k]; n.Wit = (const float*)p[7 * k + 1]; n.bi = (const float*)p[7 * k + 2];
    n.Wht = (const float*)p[7 * k + 3]; n.b_hn = (const float*)p[7 * k + 4]; n.h_in = (const float*)p[7 * k + 5];
    n.h_out = (float*)p[7 * k + 6]; n.D = D;
    dmax = D > dmax ? D : dmax;
  }
  a.reset = reset; a.R = R; a.A = A;
  const size_t lds = (size_t)64 * (dmax + LDP + CHP) * sizeof(float);
  static size_t lds_set = 0;   // (memoised device attribute: idempotent)
  if (lds > lds_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_cell_step), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      set_error("magpo_gru_cell_step: cannot raise the dynamic LDS limit");
      return MAGPO_ELAUNCH;
    }
    lds_set = lds;
  }
  hipLaunchKernelGGL(k_gru_cell_step, dim3((unsigned)((R + 63) / 64), (unsigned)nnets), dim3(256), lds, st, a);
  return check_launch("magpo_gru_cell_step");
}

extern "C" int magpo_global_state(const float* obs, long ldo, int id_cols, int F_raw, float* out, int ld, int N, int A, hipStream_t st) {
  if (!obs || !out) { set_error("magpo_global_state: null pointer"); return MAGPO_EINVAL; }
  if (N < 1 || A < 1 || F_raw < 1 || id_cols < 0 || ldo < (long)id_cols + F_raw) { set_error("magpo_global_state: bad N, A, F_raw, id_cols or ldo"); return MAGPO_EINVAL; }
  if (ld != 64 && ld != 128) { set_error("magpo_global_state: ld must be 64 or 128"); return MAGPO_EINVAL; }
  if ((long)A * F_raw > ld) { set_error("magpo_global_state: A * F_raw exceeds ld (the centralised critic reads at most 128 inputs)"); return MAGPO_EINVAL; }
  const long n = (long)N * A * (ld / 4);
  hipLaunchKernelGGL(k_global_state, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, obs, ldo, id_cols, F_raw, out, ld, (long)N, A);
  return check_launch("magpo_global_state");
}
