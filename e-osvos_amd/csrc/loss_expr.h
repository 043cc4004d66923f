// The per-pixel expressions of BCE with logits, shared by the kernels that evaluate them (misc_kernels.hip: bce_partial_kernel,
// bce_grad_kernel; bootstrap_kernels.hip): one source, so every loss kind that sums BCE terms rounds them alike.
#pragma once
#include <hip/hip_runtime.h>

namespace eosvos {
// max(x, 0) - x * t + log(1 + exp(-|x|)), e = exp(-|x|)
__device__ __forceinline__ float bce_value(float xv, float tv, float e /*exp(-|xv|)*/) {
  return fmaxf(xv, 0.f) - xv * tv + log1pf(e);
}
// (sigmoid(x) - t) * inv_n
__device__ __forceinline__ float bce_grad(float xv, float tv, float e /*exp(-|xv|)*/, float inv_n) {
  const float sig = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  return (sig - tv) * inv_n;
}
}  // namespace eosvos
