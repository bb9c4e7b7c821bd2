// SwiGLU formulas, fp32, one definition each: y = silu(g) * u with silu(g) =
// g * s, s = 1 / (1 + exp(-g)).  Shared by swiglu.hip (element-wise kernels,
// dense dual-weight GEMM) and moe_swiglu.hip (grouped expert kernels), so the
// forward and every gradient epilogue compute the same bits from the same g, u.
// exp(-g) overflowing to inf gives s = 0 and silu = g * 0 = -0; s is always
// finite, so no inf * 0 arises.
#pragma once
#include "common.h"

namespace ffk {

__device__ __forceinline__ float swiglu_sigmoid(float g) { return 1.f / (1.f + expf(-g)); }
__device__ __forceinline__ float swiglu_y(float g, float u) { return g * swiglu_sigmoid(g) * u; }
__device__ __forceinline__ void swiglu_grad(float dy, float g, float u, float& dg, float& du) {
  const float s = swiglu_sigmoid(g);
  dg = dy * u * s * (1.f + g * (1.f - s));
  du = dy * g * s;
}

}  // namespace ffk
