// exact64.hpp — the float64 side of the certified scoring calls: sim.hip (cmhse_sim_rank_exact) and
// topk.hip (cmhse_sim_topk_exact) take their float64 score, their error bound and the launch that turns
// norms into per-row tolerances from here, so a pair of rows has ONE float64 score whichever call asks;
// group.hip (cmhse_group_rank_exact) takes the float64 block score built on it (block64) and its bound.
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

// dot64 for N rows b[0 .. N) at once, for block64 and the norms of its tolerance: N chains — per lane the
// identical fused multiply-adds on the identical operands in the same order (k = lane, lane + 64, ...
// ascending), the same butterfly, so each out[c] has dot64's bits — written with a wave-uniform trip count and
// U k steps to an iteration, so that the U (N + 1) loads of an iteration are in flight together (the loops of
// dot64 and dot64x4 wait for every load in turn: their trip count differs between lanes, and a certified
// group call is a chain of such round trips).  A step past D is skipped, not added as a zero.
template <int N, int U>
__device__ __forceinline__ void dot64_wide(const float* a, const float* const (&b)[N], int D, int lane,
                                           double (&out)[N]) {
  double acc[N];
#pragma unroll
  for (int c = 0; c < N; ++c) acc[c] = 0.0;
  for (int kb = 0; kb < D; kb += 64 * U) {   // (wave-uniform)
    float x[U], y[N][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kb + 64 * u + lane;
      const int kk = k < D ? k : 0;          // (a step past D reads element 0 and is not used)
      x[u] = a[kk];
#pragma unroll
      for (int c = 0; c < N; ++c) y[c][u] = b[c][kk];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kb + 64 * u + lane < D) {
        const double xd = static_cast<double>(x[u]);
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = fma(xd, static_cast<double>(y[c][u]), acc[c]);
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] += __shfl_xor(acc[c], d, 64);
  }
#pragma unroll
  for (int c = 0; c < N; ++c) out[c] = acc[c];
}

// THE float64 block score G64 of a (video, paragraph) pair: every float64 group score of
// cmhse_group_rank_exact — the diagonal's, an undecided block's — comes out of this one routine.  One wave, all
// 64 lanes; a [r0, r1) clip rows of C, b [c0, c1) caption rows of S, both ascending:
//   s64(r, c) = dot64(C[r], S[c])  (dot64_wide on four captions at a time, the last chunk padded with its
//               last caption and the padding ignored: each s64 keeps dot64's bits);
//   max:  the largest s64(r, c) — nothing is rounded, so the result does not depend on the order;
//   mean: acc = 0.0; for r: for c: acc += s64(r, c) — sequential float64, clip-major then caption, the order
//         cmhse_group_scores documents for its fp32 mean — then acc / double(count).
// Consequence: two bit-identical groups with their rows in the same order have bit-identical G64 against
// anything.  A paragraph whose captions are permuted has the same G64 under max, and under mean in general
// does not (float64 addition does not associate); nor do groups of equal rows but different counts
// (the sum of n equal terms divided by n need not return the term).
__device__ __forceinline__ double block64(const float* C, const float* S, int D, int r0, int r1, int c0, int c1,
                                          bool use_max, int lane) {
  double m = -INFINITY, acc = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float* a = C + static_cast<int64_t>(r) * D;
    for (int c = c0; c < c1; c += 4) {
      const int last = c1 - 1;
      const int c1_ = c + 1 < last ? c + 1 : last, c2_ = c + 2 < last ? c + 2 : last, c3_ = c + 3 < last ? c + 3 : last;
      const float* const b[4] = {S + static_cast<int64_t>(c) * D, S + static_cast<int64_t>(c1_) * D,
                                 S + static_cast<int64_t>(c2_) * D, S + static_cast<int64_t>(c3_) * D};
      double s[4];
      dot64_wide<4, 4>(a, b, D, lane, s);
      const int n = c1 - c < 4 ? c1 - c : 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          m = s[k] > m ? s[k] : m;
          acc += s[k];
        }
      }
    }
  }
  return use_max ? m : acc / static_cast<double>((r1 - r0) * (c1 - c0));
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

// ---------------------------------------------------------------------------------------------
// The bound of the group scores (cmhse_group_rank_exact).  G32 is cmhse_group_scores' block score of the fp32
// scores v(r,c), G64 is block64 above.  Video -> paragraph: A_i = max |a_r| over the clips of video i, Bmax = max
// |b_c| over ALL caption rows, so every entry of every block of row i has |v(r,c) - s64(r,c)| <= E_i =
// E(A_i, Bmax), the bound above.
// max:  |max v - max s64| <= max |v - s64| (a maximum is 1-Lipschitz in the sup norm) and neither side rounds:
//       |G32 - G64| <= E_i, the tolerance is exact_tolerance(D, A_i, Bmax) unchanged.
// mean: G32 = fl32(fl64(fl64-sum(v) / n)), G64 = fl64(fl64-sum(s64) / n), n <= 128 * 128 = 2^14 entries.
//       (1) the exact means differ by at most E_i;
//       (2) each sequential float64 sum of n terms and its division are off by at most gamma_n(u') max |term| of
//           the mean, n u' <= 2^-39; |v|, |s64| <= (1 + gamma_D(u) + small) A_i Bmax: 2 * 2^-39 A_i Bmax for the
//           two sides, and 2^-38 gamma_D A_i Bmax more, which is 2^-38 of term (1), inside the slack;
//       (3) the rounding to fp32: u |G| <= u A_i Bmax, and u gamma_D A_i Bmax more, 2^-24 of term (1), inside the
//           slack; a result in the subnormal range is off by 2^-150 instead, which D 2^-149 covers beside the
//           chain's D 2^-150.
//       |G32 - G64| <= E_mean = (gamma_D(u) + u + 2^-38 + (D / 64 + 8) 2^-53) A_i Bmax + D 2^-149.
// Both compared values, G32[i,j] and G32[i,i], lie in row i: |fl(G32[i,j] - G32[i,i])| > 2 E (1 + 2^-18) decides
// the sign of G64[i,j] - G64[i,i] as above.  The slack 1 + 2^-18 now carries 1 / (1 - u), the two 2^-24 and
// 2^-38 remainders of (2) and (3), the norms (2^-45), the maximum of the norms of a group (exact: a maximum
// rounds nothing) and about fifteen float64 operations: below 2^-22 in all.
// Paragraph -> video: the roles swap — B_j = max |b_c| over the captions of paragraph j, Amax = max |a_r| over
// ALL clip rows; G32[i,j] and G32[j,j] lie in column j, so both are within E(Amax, B_j).
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline double group_exact_tolerance(int32_t D, bool use_max, double norm_a, double norm_b_max) {
  if (use_max) return exact_tolerance(D, norm_a, norm_b_max);
  const double du = static_cast<double>(D) * 0x1p-24;
  if (!(du < 1.0)) return INFINITY;
  const double gamma = du / (1.0 - du);
  const double e64 = static_cast<double>(D / 64 + 8) * 0x1p-53;
  const double e = (gamma + 0x1p-24 + 0x1p-38 + e64) * norm_a * norm_b_max + static_cast<double>(D) * 0x1p-149;
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
