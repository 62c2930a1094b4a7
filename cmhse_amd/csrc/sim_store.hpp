// sim_store.hpp — the stored-score GEMM of sim.hip (sim_kernel<kSimStore>) for the other translation
// units: scores[i][j] = A[i] . B[j], exact fp32, bit-identical to the scores the ranking compares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmhse {

// A [n, D], B [m, D] -> scores [n, m].  blk_off != nullptr: n_blocks square blocks in one launch
// (n = m = the largest block): block b is rows [blk_off[b], blk_off[b+1]) of A and B, its scores at
// scores + b * blk_stride with the block's own size as leading dimension.  Returns a CMHSE_* code.
int launch_sim_store(const float* A, const float* B, int n, int m, int D, float* scores,
                     hipStream_t stream, const int32_t* blk_off = nullptr, int n_blocks = 1,
                     int64_t blk_stride = 0);

}  // namespace cmhse
