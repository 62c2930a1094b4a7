// norm_rows.hpp — F.normalize of ONE row by one workgroup of kThreads, forward and backward: the row
// arithmetic shared by l2norm_rows_kernel (gru_rows.hpp) / step_norm_kernel and by l2norm_bwd_kernel /
// step_norm_bwd_kernel (loss_kernels.hpp), so the fused step losses are bit-identical to the
// operator-by-operator form by construction.  Device functions only: any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "nt_core.hpp"

namespace cmhse {

// y = x / max(||x||_2, 1e-12).  Every thread of the workgroup calls it (it holds barriers).
__device__ __forceinline__ void l2norm_row(const float* xr, float* yr, int cols) {
  float ss = 0.f;
  for (int c = threadIdx.x; c < cols; c += kThreads) {
    const float v = xr[c];
    ss += v * v;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ss += __shfl_xor(ss, d, 64);
  __shared__ float s_part[kThreads / 64];
  __shared__ float s_inv;
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < kThreads / 64; ++i) t += s_part[i];
    s_inv = 1.0f / fmaxf(sqrtf(t), 1e-12f);
  }
  __syncthreads();
  const float inv = s_inv;
  for (int c = threadIdx.x; c < cols; c += kThreads) yr[c] = xr[c] * inv;
}

// dx = (g - y (y.g)) / ||x|| for ||x|| >= eps, y = x / ||x||, and dx = g / eps below it (the clamp
// passes no gradient to the norm, as torch's clamp_min does not); grad(c) is the upstream gradient
// of column c, evaluated twice per column.
template <typename Grad>
__device__ __forceinline__ void l2norm_bwd_row(const float* xr, float* dxr, int cols, Grad grad) {
  float ss = 0.f, sg = 0.f;
  for (int c = threadIdx.x; c < cols; c += kThreads) {
    ss += xr[c] * xr[c];
    sg += xr[c] * grad(c);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    ss += __shfl_xor(ss, o, 64);
    sg += __shfl_xor(sg, o, 64);
  }
  __shared__ float p1[4], p2[4];
  __shared__ float s_inv, s_dot;
  if ((threadIdx.x & 63) == 0) {
    p1[threadIdx.x >> 6] = ss;
    p2[threadIdx.x >> 6] = sg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float n2 = p1[0] + p1[1] + p1[2] + p1[3];
    const float nrm = sqrtf(n2);
    const float inv = 1.0f / fmaxf(nrm, 1e-12f);
    s_inv = inv;
    // (y.g)/||x||; inside the clamp the denominator is the constant eps: no projection term
    s_dot = nrm < 1e-12f ? 0.f : (p2[0] + p2[1] + p2[2] + p2[3]) * inv * inv;
  }
  __syncthreads();
  const float inv = s_inv, d = s_dot;
  for (int c = threadIdx.x; c < cols; c += kThreads) dxr[c] = (grad(c) - xr[c] * d) * inv;
}

}  // namespace cmhse
