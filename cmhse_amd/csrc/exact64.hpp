// exact64.hpp — the float64 side of the certified scoring calls: sim.hip (cmhse_sim_rank_exact) and
// topk.hip (cmhse_sim_topk_exact) take their float64 score, their error bound and the launch that turns
// norms into per-row tolerances from here, so a pair of rows has ONE float64 score whichever call asks.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace cmhse {

// THE float64 score of two fp32 rows: every s64 of cmhse_sim_rank_exact and cmhse_sim_topk_exact — the
// diagonal's, an undecided pair's, a top-K candidate's, the squared norms of the tolerance — comes out of
// this one routine, so two pairs of bit-identical rows have bit-identical scores whichever kernel asked.
// One wave, all 64 lanes: lane l runs the chain
// acc = fma(double(a[k]), double(b[k]), acc) over k = l, l + 64, ... ascending from acc = 0 (the product of
// two fp32 values is exact in float64: one rounding per term), then the 64 partial sums are added in a
// butterfly over lane distances 32, 16, 8, 4, 2, 1 (x + y is commutative, so every lane holds the same
// bits).  Reads are coalesced (256 B per wave and step); the rows are L2-hot in the tile passes.
__device__ __forceinline__ double dot64(const float* a, const float* b, int D, int lane) {
  double acc = 0.0;
  for (int k = lane; k < D; k += 64) acc = fma(static_cast<double>(a[k]), static_cast<double>(b[k]), acc);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  return acc;
}

// dot64 of one row a with four rows b0 .. b3 at once: out[c] is dot64(a, b_c), term for term — the same chain
// per lane (the identical fused multiply-add on the identical operands, in the same order) and the same
// butterfly, so the bits are dot64's.  The four chains are independent: their loads and float64 operations
// overlap where one dot64 after the other waits on each in turn.
__device__ __forceinline__ void dot64x4(const float* a, const float* b0, const float* b1, const float* b2,
                                        const float* b3, int D, int lane, double out[4]) {
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  for (int k = lane; k < D; k += 64) {
    const double x = static_cast<double>(a[k]);
    acc0 = fma(x, static_cast<double>(b0[k]), acc0);
    acc1 = fma(x, static_cast<double>(b1[k]), acc1);
    acc2 = fma(x, static_cast<double>(b2[k]), acc2);
    acc3 = fma(x, static_cast<double>(b3[k]), acc3);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    acc0 += __shfl_xor(acc0, d, 64);
    acc1 += __shfl_xor(acc1, d, 64);
    acc2 += __shfl_xor(acc2, d, 64);
    acc3 += __shfl_xor(acc3, d, 64);
  }
  out[0] = acc0, out[1] = acc1, out[2] = acc2, out[3] = acc3;
}

// ---------------------------------------------------------------------------------------------
// The bound.  v(i,j) is the MFMA k-chain: D fused multiply-adds in fp32, one rounding each (unit roundoff
// u = 2^-24), in an order that does not matter here.  With gamma_n(u) = n u / (1 - n u), the standard
// bound of such a chain (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) is
//   |v(i,j) - a_i . b_j| <= gamma_D(u) sum_k |a_ik b_jk| <= gamma_D(u) |a_i| |b_j|    (Cauchy-Schwarz)
// as long as no step underflows.  fp32 subnormals are kept here (neither the operands nor the
// accumulator of the MFMA flush), so a step whose result falls below 2^-126 is off by at most half a
// subnormal step, 2^-150: D 2^-149 in all, added as an absolute term.  No other assumption is made on
// small products; the inputs are assumed finite, and D < 2^24.
// s64(i,j) is dot64: chains of at most ceil(D / 64) fused multiply-adds in float64 (u' = 2^-53; the
// products are exact) and six more additions: |s64(i,j) - a_i . b_j| <= gamma_{ceil(D/64)+6}(u') |a_i| |b_j|,
// taken here as (D / 64 + 8) 2^-53 (the denominator 1 - n u' is covered by the slack below).  So
//   |v(i,j) - s64(i,j)| <= E_i = (gamma_D(u) + (D / 64 + 8) 2^-53) |a_i| max_j |b_j| + D 2^-149
// for every column j, and |fl(v(i,j) - v(i,j'))| > 2 E_i / (1 - u) decides the sign of s64(i,j) - s64(i,j')
// (the fp32 subtraction is off by a factor 1 + d, |d| <= u).  What is left is the
// arithmetic of the tolerance itself: the norms are sqrt(dot64(x, x)), relative error below 2^-45 for
// D < 2^24; the maximum over j is rounded UP to fp32 before its atomic max; the dozen float64 operations
// below are off by 2^-53 each; the result, times the tunable rank_exact_tol_scale, is rounded UP to the
// fp32 the kernel compares with.  All of that, 1 / (1 - u) included, lies far inside the factor 1 + 2^-18.
// The value stays within 1 + 2^-11 of the textbook 2 D u |a| |b| up to D = 4096: nothing is given away.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline double exact_tolerance(int32_t D, double norm_a, double norm_b_max) {
  const double du = static_cast<double>(D) * 0x1p-24;
  if (!(du < 1.0)) return INFINITY;
  const double gamma = du / (1.0 - du);
  const double e64 = static_cast<double>(D / 64 + 8) * 0x1p-53;
  const double e = (gamma + e64) * norm_a * norm_b_max + static_cast<double>(D) * 0x1p-149;
  return 2.0 * e * (1.0 + 0x1p-18);
}

// the smallest fp32 that is not below x >= 0
__device__ __forceinline__ float round_up_f32(double x) {
  float f = static_cast<float>(x);
  if (static_cast<double>(f) < x) f = __uint_as_float(__float_as_uint(f) + 1u);   // (f >= 0, finite)
  return f;
}

// tol[i] from |a_i| and the bits of the largest |b_j| (rounded up to fp32 before its atomic max; the bits
// of floats >= 0 order as integers).  (static: one copy per translation unit that launches it)
static __global__ void exact_tol_kernel(const double* norm_a, const unsigned* norm_b_max, float* tol, int32_t D,
                                        int32_t scale, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double nb = static_cast<double>(__uint_as_float(*norm_b_max));
  tol[i] = round_up_f32(exact_tolerance(D, norm_a[i], nb) * static_cast<double>(scale));
}

}  // namespace cmhse
