// topk.hip — cmhse_sim_topk: the K best gallery columns of every query row, matrix-free.
//
// For the stripe [row0, row0 + nrows) of A [N, D] against B [M, D], d[i, j] = A[i] . B[j]: the K
// columns with the largest d, by score descending and then column ascending on exact ties: the order
// of the score key of score_tile.hpp, which also decides sim_rank's top-1.
//
// Bit-exactness: every d[i, j] comes out of nt_phase (nt_core.hpp), whose k order per output does
// not depend on the tile shape or position — the scores returned are bit-identical to
// cmhse_cosine_sim's, and the float is recovered from the key's bits, never recomputed.
//
// Shape ("Top-K retrieval"):
//   topk_select_kernel  grid = 64-row tiles x column PANELS (runs of 128-wide column tiles).  A
//                       workgroup walks its panel's tiles; after each tile's MFMA loop it stages the
//                       64 x 128 scores in LDS and each wave takes 16 rows: a ballot of key > the
//                       row's current K-th key picks the candidates (few once the list is warm: about
//                       K (1 + ln(M / K)) per row over a random-order gallery), which are merged into
//                       the row's sorted list in LDS.  The panel's K keys per row go to the workspace.
//   topk_merge_kernel   one wave per row merges the P panel lists the same way and decodes the keys
//                       (wave_merge and merge_panel_lists: topk_lists.hpp, shared with group.hip).
// 64-row tiles rather than sim_rank's 128: the running lists live in LDS, 64 rows x K x 8 B (64 KB at
// K = 128); 128 rows would need 128 KB beside the tile buffers, more than a CU has for one workgroup
// at K = 128, and half of that already leaves one workgroup per CU at K = 50.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "nt_core.hpp"
#include "score_tile.hpp"
#include "topk_lists.hpp"

namespace cmhse {
namespace {

constexpr int kTkBM = 64;                 // query rows per workgroup
constexpr int kTkBN = 128;                // gallery columns per tile
constexpr int kTkLd = kTkBN + 8;          // staged score row stride (floats): the two half-waves' rows
                                          // (4 apart) start on different banks
constexpr int kTkCUs = 256;               // MI355X compute units: the panel count fills them once
constexpr size_t kTkLdsPerCU = 160 * 1024;
constexpr size_t kTkTileBytes =
    (TileSmem<kTkBM, kTkBN>::kBytes > sizeof(float) * kTkBM * kTkLd) ? TileSmem<kTkBM, kTkBN>::kBytes
                                                                       : sizeof(float) * kTkBM * kTkLd;
constexpr size_t kTkCandBytes = sizeof(score_key_t) * kTkBN * (kThreads / 64);   // one buffer per wave

struct TopkParams {
  const float* A;    // [N, D]
  const float* B;    // [M, D]
  int32_t M, D, row0, nrows, K;
  int32_t row_tiles, col_tiles, panels;
  score_key_t* ws;   // [panels, nrows, K] sorted keys of each panel
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void topk_select_kernel(const TopkParams p) {
  // blocks b and b + 8 share an XCD (round-robin dispatch): each XCD takes a contiguous run of the
  // panel-major work list, so the row tiles of a panel stream its gallery tiles through one L2
  const int per_xcd = static_cast<int>(gridDim.x >> 3);
  const int L = static_cast<int>(blockIdx.x & 7) * per_xcd + static_cast<int>(blockIdx.x >> 3);
  if (L >= p.row_tiles * p.panels) return;   // padding of the grid to a multiple of 8
  const int panel = L / p.row_tiles;
  const int i0 = (L % p.row_tiles) * kTkBM;
  const int t_begin = static_cast<int>(static_cast<int64_t>(panel) * p.col_tiles / p.panels);
  const int t_end = static_cast<int>(static_cast<int64_t>(panel + 1) * p.col_tiles / p.panels);
  const int K = p.K;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* stage = smem;   // nt_phase's tile buffers, then the tile's scores [kTkBM][kTkLd]
  score_key_t* lists =
      reinterpret_cast<score_key_t*>(reinterpret_cast<char*>(smem) + kTkTileBytes);   // [kTkBM][K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  score_key_t* cand = lists + kTkBM * K + wave * kTkBN;
  for (int e = tid; e < kTkBM * K; e += kThreads) lists[e] = 0ull;   // (seen after nt_phase's barriers)

  rowaddr_t ar[1];
  bool av[1];
  ar[0] = tile_row(p.A, p.D, p.row0, i0 + srow, p.nrows, &av[0]);
  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * kTkBN;
    rowaddr_t br[2];
    bool bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) br[i] = tile_row(p.B, p.D, 0, j0 + srow + 64 * i, p.M, &bv[i]);
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    // starts with a barrier (every wave is done with the previous tile's staged scores) and ends
    // with one (every wave has read its last fragments)
    nt_phase<kTkBM, kTkBN, 1, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 32, b_row0, acc);
#pragma unroll
    for (int ns = 0; ns < 2; ++ns)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        stage[(wm * 32 + acc_row(r, lane)) * kTkLd + wn * 64 + ns * 32 + acc_col(lane)] = acc[0][ns][r];
    __syncthreads();
    for (int rr = 0; rr < kTkBM / 4; ++rr) {
      const int row = wave * (kTkBM / 4) + rr;
      if (i0 + row >= p.nrows) break;   // (wave-uniform)
      score_key_t* lst = lists + row * K;
      const score_key_t thr = lst[K - 1];
      const float* srow_scores = stage + row * kTkLd;
      // columns past M (and rows past the tile's edge) hold garbage: key 0 never beats a threshold
      const score_key_t k0 = (j0 + lane < p.M) ? score_key(srow_scores[lane], j0 + lane) : 0ull;
      const score_key_t k1 = (j0 + 64 + lane < p.M) ? score_key(srow_scores[64 + lane], j0 + 64 + lane) : 0ull;
      const bool c0 = k0 > thr, c1 = k1 > thr;
      const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
      if ((m0 | m1) == 0ull) continue;
      const unsigned long long below = (1ull << lane) - 1ull;
      if (c0) cand[__popcll(m0 & below)] = k0;
      if (c1) cand[__popcll(m0) + __popcll(m1 & below)] = k1;
      __builtin_amdgcn_wave_barrier();
      wave_merge(lst, K, cand, __popcll(m0) + __popcll(m1), lane);
    }
  }
  __syncthreads();
  const int rows = (p.nrows - i0 < kTkBM) ? p.nrows - i0 : kTkBM;
  score_key_t* out = p.ws + (static_cast<int64_t>(panel) * p.nrows + i0) * K;
  for (int e = tid; e < rows * K; e += kThreads) out[e] = lists[e];
}

// One wave per row: the P panel lists (each sorted: its candidates are a prefix) into one, decoded.
__global__ __launch_bounds__(kThreads) void topk_merge_kernel(const PanelLists p) {
  __shared__ score_key_t s_list[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ score_key_t s_cand[kThreads / 64][CMHSE_TOPK_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = blockIdx.x * (kThreads / 64) + wave;
  if (li >= p.nrows) return;   // (no barrier below)
  merge_panel_lists(p, li, s_list[wave], s_cand[wave], lane);
}

size_t topk_smem(int K) {
  return kTkTileBytes + sizeof(score_key_t) * kTkBM * static_cast<size_t>(K) + kTkCandBytes;
}

// Panels per row tile: as many as fill every CU's resident workgroups ONCE (LDS decides how many fit),
// never more than there are column tiles.  The count does not grow with M — nor does the workspace.
int topk_panels(int nrows, int M, int K) {
  const int row_tiles = (nrows + kTkBM - 1) / kTkBM;
  const int col_tiles = (M + kTkBN - 1) / kTkBN;
  int per_cu = static_cast<int>(kTkLdsPerCU / topk_smem(K));
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  int P = kTkCUs * per_cu / row_tiles;
  if (P > col_tiles) P = col_tiles;
  return P < 1 ? 1 : P;
}

}  // namespace
}  // namespace cmhse

using namespace cmhse;

extern "C" size_t cmhse_sim_topk_workspace(int32_t nrows, int32_t M, int32_t K) {
  if (nrows <= 0 || M <= 0 || K < 1 || K > CMHSE_TOPK_MAX) return 0;
  return align256(static_cast<size_t>(topk_panels(nrows, M, K)) * static_cast<size_t>(nrows) *
                  static_cast<size_t>(K) * sizeof(score_key_t));
}

extern "C" int cmhse_sim_topk(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                              int32_t row0, int32_t nrows, int32_t K, float* scores, int32_t* index,
                              void* workspace, size_t workspace_bytes, void* stream_) {
  if (!A || !B) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (K < 1 || K > M || K > CMHSE_TOPK_MAX) return CMHSE_ERR_ARG;
  if (row0 < 0 || nrows < 0 || static_cast<int64_t>(row0) + nrows > N) return CMHSE_ERR_ARG;
  if (nrows == 0) return CMHSE_OK;
  if (!scores || !index || !workspace) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_topk_workspace(nrows, M, K))
    return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TopkParams p;
  p.A = A;
  p.B = B;
  p.M = M;
  p.D = D;
  p.row0 = row0;
  p.nrows = nrows;
  p.K = K;
  p.row_tiles = (nrows + kTkBM - 1) / kTkBM;
  p.col_tiles = (M + kTkBN - 1) / kTkBN;
  p.panels = topk_panels(nrows, M, K);
  p.ws = static_cast<score_key_t*>(workspace);
  const int64_t blocks = (static_cast<int64_t>(p.row_tiles) * p.panels + 7) / 8 * 8;
  if (blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  // (past 64 KiB of LDS for K > 52)
  const int rc = launch_tiles(topk_select_kernel<true>, topk_select_kernel<false>, D,
                              dim3(static_cast<unsigned>(blocks)), topk_smem(K), stream, p);
  if (rc != CMHSE_OK) return rc;
  const PanelLists lists = {p.ws, p.panels, nrows, K, scores, index};
  hipLaunchKernelGGL(topk_merge_kernel, dim3((nrows + 3) / 4), dim3(kThreads), 0, stream, lists);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}
