// Greedy action selection shared by the Q-learning kernels (csrc/qlearn.hip, csrc/qmix.hip).
#pragma once
#include "common.hpp"

namespace magpo {

constexpr float Q_FMIN = -3.4028234663852886e38f;  // jnp.finfo(float32).min: what an illegal action's Q value is replaced by

// argmax over the legal columns of one Q row, first maximum wins (jnp.argmax of where(mask, q, finfo.min)); m == nullptr: all legal
__device__ __forceinline__ int masked_argmax(const float* __restrict__ q, const unsigned char* __restrict__ m, int K) {
  float best = (m && !m[0]) ? Q_FMIN : q[0];
  int arg = 0;
  for (int k = 1; k < K; ++k) {
    const float v = (m && !m[k]) ? Q_FMIN : q[k];
    if (v > best) { best = v; arg = k; }
  }
  return arg;
}

}  // namespace magpo
