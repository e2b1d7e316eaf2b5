// Row kernels of the actor's MLPTorso layers with LayerNorm (mava/networks/torsos.py:36-47):
//   y = act(LayerNorm(z) + b),  LayerNorm(use_scale=False): (z - mean) * rsqrt(var + 1e-6), var = max(E[z^2] - E[z]^2, 0)
// (flax's fast variance), act = identity / relu / tanh.  The Dense layer before it (z = x W + b_dense) is magpo_linear.
//
// Row geometry: a D-wide row (D = 64, 128, 192, 256) is held as float4 by LPR = D / 4 lanes; rows sit in aligned lane groups of RW
// (16, 32, 64, 64: the next power of two), RPW = 64 / RW rows per wave (D = 192: lanes 48..63 of the wave idle, holding zeros).
// Row statistics are DPP sums over 16 lanes plus xor-shuffles over 16 / 32 (no LDS).  HBM-bound: one read of z and two row writes
// forward; four row reads and one write backward.
#include "common.hpp"

namespace magpo {

namespace {

constexpr float LN_EPS = 1e-6f;
enum { TACT_NONE = 0, TACT_RELU = 1, TACT_TANH = 5 };   // the activation codes of magpo_linear

template <int D> struct LnGeo {
  static constexpr int LPR = D / 4, RW = LPR <= 16 ? 16 : (LPR <= 32 ? 32 : 64), RPW = 64 / RW;
};

template <int RW> __device__ __forceinline__ float group_sum(float v) {
  v = sum16(v);
  if (RW >= 32) v += __shfl_xor(v, 16, 64);
  if (RW >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float f4sum(float4 a) { return (a.x + a.y) + (a.z + a.w); }

__device__ __forceinline__ float act_fwd(float v, int act) {
  return act == TACT_RELU ? fmaxf(v, 0.f) : (act == TACT_TANH ? tanhf(v) : v);
}
// dL/d(pre-activation) from dL/dy and the activated output y
__device__ __forceinline__ float act_bwd(float d, float y, int act) {
  return act == TACT_RELU ? (y > 0.f ? d : 0.f) : (act == TACT_TANH ? d * (1.f - y * y) : d);
}

template <int D>
__global__ __launch_bounds__(256) void k_ln_act_fwd(const float* __restrict__ z, int ldz, const float* __restrict__ bias,
                                                    float* __restrict__ y, int ldy, float* __restrict__ xhat, int ldxh,
                                                    float* __restrict__ rstd, long R, int act) {
  using G = LnGeo<D>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G::RW, c = lane % G::RW;
  const bool on = c < G::LPR;
  const float4 b = on ? ld4(bias + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (long base = ((long)blockIdx.x * 4 + wave) * G::RPW; base < R; base += (long)gridDim.x * 4 * G::RPW) {   // wave-uniform
    const long row = base + sub;
    const bool ok = on && row < R;
    const float4 x = ok ? ld4(z + row * ldz + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float mean = group_sum<G::RW>(f4sum(x)) * (1.f / D);
    const float msq = group_sum<G::RW>((x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w)) * (1.f / D);
    const float r = rsqrtf(fmaxf(msq - mean * mean, 0.f) + LN_EPS);
    const float4 xh = make_float4((x.x - mean) * r, (x.y - mean) * r, (x.z - mean) * r, (x.w - mean) * r);
    const float4 v = make_float4(act_fwd(xh.x + b.x, act), act_fwd(xh.y + b.y, act), act_fwd(xh.z + b.z, act), act_fwd(xh.w + b.w, act));
    if (ok) {
      st4(y + row * ldy + 4 * c, v);
      st4(xhat + row * ldxh + 4 * c, xh);
      if (c == 0) rstd[row] = r;
    }
  }
}

// slab_b [gridDim.x][D]: per-workgroup column sums of g = dy * act'(y) (the LayerNorm bias gradient), fixed summation order
template <int D>
__global__ __launch_bounds__(256) void k_ln_act_bwd(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                    const float* __restrict__ xhat, int ldxh, const float* __restrict__ rstd,
                                                    float* __restrict__ dz, int lddz, float* __restrict__ slab_b, long R, int act) {
  using G = LnGeo<D>;
  __shared__ __align__(16) float lds[4 * D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G::RW, c = lane % G::RW;
  const bool on = c < G::LPR;
  float4 bacc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long base = ((long)blockIdx.x * 4 + wave) * G::RPW; base < R; base += (long)gridDim.x * 4 * G::RPW) {
    const long row = base + sub;
    const bool ok = on && row < R;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), xh = g;
    float r = 0.f;
    if (ok) {
      const float4 d = ld4(dy + row * lddy + 4 * c), yv = ld4(y + row * ldy + 4 * c);
      xh = ld4(xhat + row * ldxh + 4 * c);
      r = rstd[row];
      g = make_float4(act_bwd(d.x, yv.x, act), act_bwd(d.y, yv.y, act), act_bwd(d.z, yv.z, act), act_bwd(d.w, yv.w, act));
    }
    bacc.x += g.x; bacc.y += g.y; bacc.z += g.z; bacc.w += g.w;
    const float mg = group_sum<G::RW>(f4sum(g)) * (1.f / D);
    const float mgx = group_sum<G::RW>((g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w)) * (1.f / D);
    if (ok)
      st4(dz + row * lddz + 4 * c, make_float4(r * (g.x - mg - xh.x * mgx), r * (g.y - mg - xh.y * mgx),
                                               r * (g.z - mg - xh.z * mgx), r * (g.w - mg - xh.w * mgx)));
  }
  // column sums: over the RPW rows of a wave (lanes c, c + RW, ...), then over the 4 waves through LDS
#pragma unroll
  for (int o = G::RW; o < 64; o <<= 1) {
    bacc.x += __shfl_xor(bacc.x, o, 64); bacc.y += __shfl_xor(bacc.y, o, 64);
    bacc.z += __shfl_xor(bacc.z, o, 64); bacc.w += __shfl_xor(bacc.w, o, 64);
  }
  if (sub == 0 && on) st4(&lds[wave * D + 4 * c], bacc);
  __syncthreads();
  if (threadIdx.x < D)
    slab_b[(long)blockIdx.x * D + threadIdx.x] = (lds[threadIdx.x] + lds[D + threadIdx.x]) + (lds[2 * D + threadIdx.x] + lds[3 * D + threadIdx.x]);
}

// the row-kernel grid of rowops.hip (magpo_row_grid): about 16 rows per workgroup, at most 2048 workgroups
inline int ln_grid(long R) {
  const long b = (R + 15) / 16;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int check_ln(const char* what, long R, int D, int act, std::initializer_list<long> lds, std::initializer_list<const void*> ptrs) {
  if (D != 64 && D != 128 && D != 192 && D != 256) { set_error(what); return MAGPO_EINVAL; }
  if (act != TACT_NONE && act != TACT_RELU && act != TACT_TANH) { set_error(what); return MAGPO_EINVAL; }
  for (long l : lds)
    if (l < D || (l & 3)) { set_error(what); return MAGPO_EINVAL; }
  for (const void* p : ptrs)
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15)) { set_error(what); return MAGPO_EINVAL; }
  return R < 0 ? (set_error(what), MAGPO_EINVAL) : MAGPO_OK;
}

}  // namespace

}  // namespace magpo

using namespace magpo;

extern "C" int magpo_ln_act_fwd(const float* z, int ldz, const float* bias, float* y, int ldy, float* xhat, int ldxh, float* rstd,
                                long R, int D, int act, hipStream_t st) {
  if (int e = check_ln("magpo_ln_act_fwd: D in {64, 128, 192, 256}, act in {0, 1, 5}, strides >= D and multiples of 4, 16-B aligned "
                       "non-null row pointers", R, D, act, {ldz, ldy, ldxh}, {z, bias, y, xhat}))
    return e;
  if (!rstd) { set_error("magpo_ln_act_fwd: rstd is required"); return MAGPO_EINVAL; }
  if (R == 0) return MAGPO_OK;
  const dim3 g(ln_grid(R)), b(256);
  switch (D) {
    case 64: hipLaunchKernelGGL(k_ln_act_fwd<64>, g, b, 0, st, z, ldz, bias, y, ldy, xhat, ldxh, rstd, R, act); break;
    case 128: hipLaunchKernelGGL(k_ln_act_fwd<128>, g, b, 0, st, z, ldz, bias, y, ldy, xhat, ldxh, rstd, R, act); break;
    case 192: hipLaunchKernelGGL(k_ln_act_fwd<192>, g, b, 0, st, z, ldz, bias, y, ldy, xhat, ldxh, rstd, R, act); break;
    default: hipLaunchKernelGGL(k_ln_act_fwd<256>, g, b, 0, st, z, ldz, bias, y, ldy, xhat, ldxh, rstd, R, act); break;
  }
  return check_launch("magpo_ln_act_fwd");
}

extern "C" int magpo_ln_act_bwd(const float* dy, int lddy, const float* y, int ldy, const float* xhat, int ldxh, const float* rstd,
                                float* dz, int lddz, float* slab_b, long R, int D, int act, hipStream_t st) {
  if (int e = check_ln("magpo_ln_act_bwd: D in {64, 128, 192, 256}, act in {0, 1, 5}, strides >= D and multiples of 4, 16-B aligned "
                       "non-null row pointers", R, D, act, {lddy, ldy, ldxh, lddz}, {dy, y, xhat, dz}))
    return e;
  if (!rstd || !slab_b) { set_error("magpo_ln_act_bwd: rstd and slab_b are required"); return MAGPO_EINVAL; }
  if (R == 0) return MAGPO_OK;
  const dim3 g(ln_grid(R)), b(256);
  switch (D) {
    case 64: hipLaunchKernelGGL(k_ln_act_bwd<64>, g, b, 0, st, dy, lddy, y, ldy, xhat, ldxh, rstd, dz, lddz, slab_b, R, act); break;
    case 128: hipLaunchKernelGGL(k_ln_act_bwd<128>, g, b, 0, st, dy, lddy, y, ldy, xhat, ldxh, rstd, dz, lddz, slab_b, R, act); break;
    case 192: hipLaunchKernelGGL(k_ln_act_bwd<192>, g, b, 0, st, dy, lddy, y, ldy, xhat, ldxh, rstd, dz, lddz, slab_b, R, act); break;
    default: hipLaunchKernelGGL(k_ln_act_bwd<256>, g, b, 0, st, dy, lddy, y, ldy, xhat, ldxh, rstd, dz, lddz, slab_b, R, act); break;
  }
  return check_launch("magpo_ln_act_bwd");
}
