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
//
// cmhse_sim_topk_exact: the K best columns by the FLOAT64 scores of the same rows (dot64, exact64.hpp),
// certified.  The launches above give the K-th fp32 score v_K(i) of every row; a second tile pass of the same
// shape, topk_exact_select_kernel, takes every column with fl(v_K - v(i,j)) <= tol_i through dot64 and keeps
// the K best (float64 bits, column) pairs per row in LDS; topk_exact_merge_kernel merges the panels.
// Why the candidates hold the whole float64 top-K.  E_i bounds |v(i,j) - s64(i,j)| for every j (exact64.hpp)
// and tol_i = 2 E_i (1 + 2^-18).  The K columns of the fp32 list have v >= v_K, hence s64 >= v_K - E_i: the
// K-th largest s64 of the row is at least v_K - E_i.  A member j of the float64 top-K has s64(i,j) at least
// that (with ties at the boundary too: the column decides among equals, the score bound is the same), so
// v(i,j) >= s64(i,j) - E_i >= v_K - 2 E_i; the factor on tol_i covers the rounding of fl(v_K - v).  The
// scores of the second pass are nt_phase's again, bit for bit, so the fp32 list's own K columns always
// qualify (v_K - v <= 0) and every list fills.  The exact top-K of a superset of the top-K is the top-K.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "exact64.hpp"
#include "gru_ws.hpp"
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

// (the walk of the work list below is restated as panel_work / panel_grid_blocks in topk_lists.hpp for
// topk_exact_select_kernel; this kernel keeps it inline so that its instructions stay what they were)
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
int panels_for_smem(int nrows, int M, size_t smem) {
  const int row_tiles = (nrows + kTkBM - 1) / kTkBM;
  const int col_tiles = (M + kTkBN - 1) / kTkBN;
  int per_cu = static_cast<int>(kTkLdsPerCU / smem);
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  int P = kTkCUs * per_cu / row_tiles;
  if (P > col_tiles) P = col_tiles;
  return P < 1 ? 1 : P;
}

int topk_panels(int nrows, int M, int K) { return panels_for_smem(nrows, M, topk_smem(K)); }

// ---------------------------------------------------------------------------------------------
// cmhse_sim_topk_exact
// ---------------------------------------------------------------------------------------------
struct TopkExactPreParams {
  const float* A;          // [N, D]
  const float* B;          // [M, D]
  int32_t M, D, row0, nrows;
  double* norm_a;          // [nrows]
  unsigned* norm_b_max;    // the bits of the largest |b_j| (rounded up), zeroed
};

// One wave per row: the norms of the nrows stripe rows, then the M gallery rows' into the maximum
// (exact_pre_kernel of sim.hip without its diagonal).
__global__ __launch_bounds__(kThreads) void topk_exact_pre_kernel(const TopkExactPreParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (r < p.nrows) {
    const float* a = p.A + (static_cast<int64_t>(p.row0) + r) * p.D;
    const double na = sqrt(dot64(a, a, p.D, lane));
    if (lane == 0) p.norm_a[r] = na;
  } else if (r < static_cast<int64_t>(p.nrows) + p.M) {
    const float* b = p.B + (r - p.nrows) * p.D;
    const double nb = sqrt(dot64(b, b, p.D, lane));
    if (lane == 0) atomicMax(p.norm_b_max, __float_as_uint(round_up_f32(nb)));
  }
}

struct TopkExactParams {
  const float* A;    // [N, D]
  const float* B;    // [M, D]
  int32_t M, D, row0, nrows, K;
  int32_t row_tiles, col_tiles, panels;
  const float* v32;         // [nrows, K] the fp32 lists' scores: column K - 1 is v_K
  const float* tol;         // [nrows]
  score_bits64_t* ws_bits;  // [panels, nrows, K] sorted pairs of each panel
  int32_t* ws_cols;         // [panels, nrows, K]
  int32_t* ws_count;        // [panels, nrows] candidates of each panel
};

constexpr size_t kTkPairBytes = sizeof(score_bits64_t) + sizeof(int32_t);
constexpr size_t kTkRowWords = 3;   // per tile row: candidate count, v_K, tolerance

// LDS: [stage][list bits 64 x K][candidate bits 4 x 128][list columns 64 x K][candidate columns 4 x 128]
// [count 64][v_K 64][tol 64] — the 64-bit arrays first.
size_t topk_exact_smem(int K) {
  return kTkTileBytes + kTkPairBytes * (kTkBM * static_cast<size_t>(K) + kTkBN * (kThreads / 64)) +
         sizeof(int32_t) * kTkRowWords * kTkBM;
}

int topk_exact_panels(int nrows, int M, int K) { return panels_for_smem(nrows, M, topk_exact_smem(K)); }

// topk_select_kernel's walk and tile loop; per row, the columns that v_K cannot rule out get their dot64, four
// at a time (dot64x4: four independent chains, each dot64's own; all candidates, so the count is a function of
// the inputs), and their pairs are merged into the row's list.  Loops are bounded by the tile's 64 x 128
// elements; nothing waits on another workgroup.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void topk_exact_select_kernel(const TopkExactParams p) {
  const PanelWork w = panel_work(blockIdx.x, gridDim.x, p.row_tiles, p.col_tiles, p.panels);
  if (w.panel < 0) return;
  const int i0 = w.row_tile * kTkBM;
  const int K = p.K;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* stage = smem;   // nt_phase's tile buffers, then the tile's scores [kTkBM][kTkLd]
  score_bits64_t* lbits = reinterpret_cast<score_bits64_t*>(reinterpret_cast<char*>(smem) + kTkTileBytes);   // [kTkBM][K]
  score_bits64_t* cbits_all = lbits + kTkBM * K;                                     // [waves][kTkBN]
  int32_t* lcols = reinterpret_cast<int32_t*>(cbits_all + kTkBN * (kThreads / 64));  // [kTkBM][K]
  int32_t* ccols_all = lcols + kTkBM * K;                                            // [waves][kTkBN]
  int32_t* s_count = ccols_all + kTkBN * (kThreads / 64);                            // [kTkBM]
  float* s_vk = reinterpret_cast<float*>(s_count + kTkBM);                           // [kTkBM]
  float* s_tol = s_vk + kTkBM;                                                       // [kTkBM]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  score_bits64_t* cbits = cbits_all + wave * kTkBN;
  int32_t* ccols = ccols_all + wave * kTkBN;
  // (all seen after nt_phase's barriers; every panel has a tile: panels <= col_tiles)
  for (int e = tid; e < kTkBM * K; e += kThreads) {
    lbits[e] = 0ull;
    lcols[e] = kNoColumn;
  }
  if (tid < kTkBM) {
    const bool ok = i0 + tid < p.nrows;
    s_count[tid] = 0;
    s_vk[tid] = ok ? p.v32[static_cast<int64_t>(i0 + tid) * K + (K - 1)] : 0.f;
    s_tol[tid] = ok ? p.tol[i0 + tid] : 0.f;
  }

  rowaddr_t ar[1];
  bool av[1];
  ar[0] = tile_row(p.A, p.D, p.row0, i0 + srow, p.nrows, &av[0]);
  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  for (int t = w.t_begin; t < w.t_end; ++t) {
    const int j0 = t * kTkBN;
    rowaddr_t br[2];
    bool bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) br[i] = tile_row(p.B, p.D, 0, j0 + srow + 64 * i, p.M, &bv[i]);
    f32x16 acc[1][2] = {{zero16(), zero16()}};
    // (a barrier in front: every wave is done with the previous tile's staged scores; one behind)
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
      const float* tile_scores = stage + row * kTkLd;
      const float vk = s_vk[row];
      const float tol = s_tol[row];
      // not ruled out: NOT (fl(v_K - v) > tol); tol >= 0, possibly +inf (every column); inputs finite, so the
      // difference is no NaN.  Columns past M hold garbage and are never candidates.
      const bool c0 = (j0 + lane < p.M) && !(vk - tile_scores[lane] > tol);
      const bool c1 = (j0 + 64 + lane < p.M) && !(vk - tile_scores[64 + lane] > tol);
      const unsigned long long m[2] = {__ballot(c0), __ballot(c1)};
      if ((m[0] | m[1]) == 0ull) continue;
      const float* arow = p.A + static_cast<int64_t>(p.row0 + i0 + row) * p.D;
      // the candidates' columns, ascending, then their float64 scores four at a time (dot64x4: each is
      // dot64's chain; a short last group repeats its last column and drops the repeats)
      const unsigned long long below = (1ull << lane) - 1ull;
      const int n0 = __popcll(m[0]), c = n0 + __popcll(m[1]);
      if (c0) ccols[__popcll(m[0] & below)] = j0 + lane;             // (< M)
      if (c1) ccols[n0 + __popcll(m[1] & below)] = j0 + 64 + lane;
      __builtin_amdgcn_wave_barrier();
      for (int q = 0; q < c; q += 4) {
        const float* b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = p.B + static_cast<int64_t>(ccols[(q + u < c) ? q + u : c - 1]) * p.D;
        double s[4];
        dot64x4(arow, b[0], b[1], b[2], b[3], p.D, lane, s);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (lane == u && q + u < c) cbits[q + u] = ordered_bits64(s[u]);
      }
      if (lane == 0) s_count[row] += c;
      __builtin_amdgcn_wave_barrier();
      wave_merge_pairs(lbits + row * K, lcols + row * K, K, cbits, ccols, c, lane);
    }
  }
  __syncthreads();
  const int rows = (p.nrows - i0 < kTkBM) ? p.nrows - i0 : kTkBM;
  const int64_t out_row = static_cast<int64_t>(w.panel) * p.nrows + i0;
  for (int e = tid; e < rows * K; e += kThreads) {
    p.ws_bits[out_row * K + e] = lbits[e];
    p.ws_cols[out_row * K + e] = lcols[e];
  }
  if (tid < rows) p.ws_count[out_row + tid] = s_count[tid];
}

// One wave per row: the P panel lists into one, decoded to float64, and the panels' counts summed.
__global__ __launch_bounds__(kThreads) void topk_exact_merge_kernel(const PanelPairLists p) {
  __shared__ score_bits64_t s_lb[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ score_bits64_t s_cb[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ int32_t s_li[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ int32_t s_ci[kThreads / 64][CMHSE_TOPK_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = blockIdx.x * (kThreads / 64) + wave;
  if (li >= p.nrows) return;   // (no barrier below)
  merge_panel_pair_lists(p, li, s_lb[wave], s_li[wave], s_cb[wave], s_ci[wave], lane);
}

// Workspace: cmhse_sim_topk's (its panel keys), its two outputs (the fp32 lists), the norms and tolerances,
// and one list of K pairs and one count per row and panel.
struct TopkExactWs {
  size_t keys32, scores32, index32, norm_a, tol, norm_b_max, bits, cols, count, total;
};

TopkExactWs topk_exact_ws(int32_t nrows, int32_t M, int32_t K) {
  const size_t n = static_cast<size_t>(nrows), nk = n * static_cast<size_t>(K);
  const size_t P = static_cast<size_t>(topk_exact_panels(nrows, M, K));
  TopkExactWs L;
  size_t off = 0;
  L.keys32 = off, off += cmhse_sim_topk_workspace(nrows, M, K);
  L.scores32 = off, off += align256(nk * sizeof(float));
  L.index32 = off, off += align256(nk * sizeof(int32_t));
  L.norm_a = off, off += align256(n * sizeof(double));
  L.tol = off, off += align256(n * sizeof(float));
  L.norm_b_max = off, off += 256;
  L.bits = off, off += align256(P * nk * sizeof(score_bits64_t));
  L.cols = off, off += align256(P * nk * sizeof(int32_t));
  L.count = off, off += align256(P * n * sizeof(int32_t));
  L.total = off;
  return L;
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

extern "C" size_t cmhse_sim_topk_exact_workspace(int32_t nrows, int32_t M, int32_t K) {
  if (nrows <= 0 || M <= 0 || K < 1 || K > CMHSE_TOPK_MAX) return 0;
  return topk_exact_ws(nrows, M, K).total;
}

extern "C" int cmhse_sim_topk_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                                    int32_t row0, int32_t nrows, int32_t K, double* scores, int32_t* index,
                                    int32_t* resolved, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!A || !B) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (K < 1 || K > M || K > CMHSE_TOPK_MAX) return CMHSE_ERR_ARG;
  if (row0 < 0 || nrows < 0 || static_cast<int64_t>(row0) + nrows > N) return CMHSE_ERR_ARG;
  if (nrows == 0) return CMHSE_OK;
  if (!scores || !index || !resolved || !workspace) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_topk_exact_workspace(nrows, M, K))
    return CMHSE_ERR_WORKSPACE;
  if (D >= (1 << 24)) return CMHSE_ERR_UNSUPPORTED;   // (the bound needs D u < 1)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const TopkExactWs L = topk_exact_ws(nrows, M, K);
  char* const ws = static_cast<char*>(workspace);
  TopkExactParams p;
  p.A = A;
  p.B = B;
  p.M = M;
  p.D = D;
  p.row0 = row0;
  p.nrows = nrows;
  p.K = K;
  p.row_tiles = (nrows + kTkBM - 1) / kTkBM;
  p.col_tiles = (M + kTkBN - 1) / kTkBN;
  p.panels = topk_exact_panels(nrows, M, K);
  p.v32 = reinterpret_cast<float*>(ws + L.scores32);
  p.tol = reinterpret_cast<float*>(ws + L.tol);
  p.ws_bits = reinterpret_cast<score_bits64_t*>(ws + L.bits);
  p.ws_cols = reinterpret_cast<int32_t*>(ws + L.cols);
  p.ws_count = reinterpret_cast<int32_t*>(ws + L.count);
  const int64_t blocks = panel_grid_blocks(p.row_tiles, p.panels);
  const int64_t pre_rows = static_cast<int64_t>(nrows) + M;
  const int64_t pre_blocks = (pre_rows + kThreads / 64 - 1) / (kThreads / 64);
  // (the fp32 pass's grid too: nothing is launched for a shape any of the four launches would refuse)
  const int64_t blocks32 = panel_grid_blocks(p.row_tiles, topk_panels(nrows, M, K));
  if (blocks > 0x7fffffffLL || blocks32 > 0x7fffffffLL || pre_blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  // 1. the fp32 lists: v_K (first: the one nested call that checks arguments of its own)
  int rc = cmhse_sim_topk(A, B, N, M, D, row0, nrows, K, reinterpret_cast<float*>(ws + L.scores32),
                          reinterpret_cast<int32_t*>(ws + L.index32), ws + L.keys32,
                          cmhse_sim_topk_workspace(nrows, M, K), stream_);
  if (rc != CMHSE_OK) return rc;
  // 2. norms and tolerances
  TopkExactPreParams q;
  q.A = A;
  q.B = B;
  q.M = M;
  q.D = D;
  q.row0 = row0;
  q.nrows = nrows;
  q.norm_a = reinterpret_cast<double*>(ws + L.norm_a);
  q.norm_b_max = reinterpret_cast<unsigned*>(ws + L.norm_b_max);
  const int32_t scale = tunables().rank_exact_tol_scale.load(std::memory_order_relaxed);
  if (hipMemsetAsync(q.norm_b_max, 0, sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  hipLaunchKernelGGL(topk_exact_pre_kernel, dim3(static_cast<unsigned>(pre_blocks)), dim3(kThreads), 0, stream, q);
  hipLaunchKernelGGL(exact_tol_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, q.norm_a, q.norm_b_max,
                     reinterpret_cast<float*>(ws + L.tol), D, scale, nrows);
  // 3. the candidates in float64, 4. the panels merged
  rc = launch_tiles(topk_exact_select_kernel<true>, topk_exact_select_kernel<false>, D,
                    dim3(static_cast<unsigned>(blocks)), topk_exact_smem(K), stream, p);
  if (rc != CMHSE_OK) return rc;
  const PanelPairLists lists = {p.ws_bits, p.ws_cols, p.ws_count, p.panels, nrows, K, scores, index, resolved};
  hipLaunchKernelGGL(topk_exact_merge_kernel, dim3((nrows + 3) / 4), dim3(kThreads), 0, stream, lists);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}
