// group.hip — group-wise (video, paragraph) scores and their ranking, matrix-free at the clip level.
//
// G[i, j] reduces the clip x caption scores C[r] . S[c] over the clips r of video i and the captions
// c of paragraph j: the block maximum (CMHSE_GROUP_MAX) or the block mean (CMHSE_GROUP_MEAN: the
// fp32 scores summed in fp64 sequentially in row-major order — clip-major, then caption — divided in
// fp64 by the count, rounded to fp32).  That is the block reduction of GroupWiseContrastiveLoss
// (loss.py:26-41, loss_kernels.hpp: block_reduce_kernel, which adds in exactly this order for blocks of at most
// 256 entries), evaluated on the whole validation split without the Nc x Ns clip x caption matrix.
//
//   cmhse_group_plan    host only: packs WHOLE videos into row tiles of at most 128 clip rows and
//                       whole paragraphs into column tiles of at most 128 caption rows, so every
//                       block lies inside exactly one tile: no atomics, no partials, no combine.
//   group_sim_kernel    one workgroup per (row tile, column tile), dealt to the XCDs by score_tile.hpp:
//                       nt_phase unchanged (every score is bit-identical to cmhse_cosine_sim's), then
//                       the tile's scores are staged in LDS in two 64-row halves — in the tile buffers
//                       nt_phase has just freed — and each (video, paragraph) block of the tile is
//                       reduced by one thread in the contract's order; a block whose video straddles
//                       the halves carries its running fp64 sum (and max) across in LDS, which keeps
//                       the order.
//   group_rank_kernel   64 x 64 tiles of the stored G: per row (video -> paragraph) and per column
//                       (paragraph -> video) the count of entries above the diagonal and the top-1 key
//                       (score_tile.hpp's score key), one partial per tile;
//   group_rank_final_kernel   sums / maxes the partials of each row and column.
//
// Certified group-wise ranking (cmhse_group_rank_exact: the ranks of the float64 block scores):
//   group_exact_pre_kernel / group_exact_tol_kernel / group_exact_diag_kernel   norms, tolerances, G64[i, i];
//   group_rank_exact_kernel   group_rank_kernel's tiles with a tolerance per query; the undecided blocks go
//                             through block64 (exact64.hpp) before the workgroup leaves;
//   group_rank_exact_final_kernel   the partials, rank_hi, top-1.
//
// Group-wise top-K (cmhse_group_topk: any video set against any paragraph set, either way round):
//   cmhse_group_topk_plan     host only: the gallery side packed as above, the query side also capped
//                             at gt_qcap(K) groups a tile (the LDS of its lists);
//   group_topk_select_kernel  query tiles x gallery panels: group_sim_kernel's tile loop and block
//                             reduction (group_tile_reduce, shared) with a top-K epilogue — a ballot
//                             against each query's K-th key, wave_merge (topk_lists.hpp) into its
//                             sorted list in LDS, the panel's lists to the workspace at the end;
//   group_topk_merge_kernel   merge_panel_lists (topk_lists.hpp): the panels' lists of each query.
//
// Certified group-wise top-K (cmhse_group_topk_exact: the K best gallery groups by the float64 block scores):
//   cmhse_group_topk itself   into a private region of the workspace: G_K(q), the K-th fp32 block score;
//   group_topk_exact_pre_kernel / group_topk_exact_tol_kernel   the query rows' norms, the largest norm of
//                             each side, a tolerance per query group;
//   group_topk_exact_select_kernel   group_topk_select_kernel's grid, tile loop and block reduction; every
//                             gallery group that G_K cannot rule out goes through block64 and into the query's
//                             list of K (float64 bits, index) pairs in LDS (wave_merge_pairs);
//   group_topk_exact_merge_kernel    merge_panel_pair_lists: the panels' lists and counts of each query.
//
// Labelled group-wise ranking (cmhse_group_rank_labelled: any video set, any paragraph set, any set of positive
// gallery groups per query group; neither G nor the clip x caption matrix is stored):
//   cmhse_group_rank_labelled_plan   host only: cmhse_group_topk_plan's tiles with the query side capped at
//                             kGlQcap groups a tile, the labels (CSR, validated in full) and the PAIR TILES of
//                             the threshold pass: the (query, positive) pairs in CSR order, whole pairs packed
//                             greedily while both the clip rows and the caption rows of a tile stay <= 128;
//   group_label_threshold_kernel   one workgroup per pair tile: the groups of its pairs gathered row by row
//                             (an address per operand row, no copy), nt_phase, group_tile_reduce with the
//                             tile's local offsets; only the diagonal blocks (pair k's query x pair k's
//                             positive) are sunk, each into its query's 64-bit key by atomic max;
//   group_label_count_kernel  group_topk_select_kernel's grid, tile loop and block reduction with a counting
//                             epilogue: per query group a ballot of blk > thr and a popcount into a
//                             per-(panel, query) count, and the running top-1 key;
//   group_label_final_kernel  sums the counts and maxes the keys of the panels; decodes the threshold keys.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "exact64.hpp"
#include "gru_ws.hpp"
#include "nt_core.hpp"
#include "score_tile.hpp"
#include "topk_lists.hpp"

namespace cmhse {
namespace {

constexpr int kGrBM = CMHSE_GROUP_TILE_ROWS;   // clip rows per row tile (at most)
constexpr int kGrBN = CMHSE_GROUP_TILE_ROWS;   // caption rows per column tile (at most)
constexpr int kGrHdr = 5;                  // plan header: B, Nc, Ns, row tiles, column tiles
constexpr int kGrLd = kGrBN + 4;           // staged score row stride (floats)
// Staged rows per pass: two 64-row halves in the freed tile buffers (40 KB of LDS in all, the
// occupancy of sim_rank's counting pass; one 128-row stage beside them measured slower: DESIGN.md §4).
constexpr int kGrStageRows = 64;
constexpr size_t kGrStageBytes = sizeof(float) * kGrStageRows * kGrLd;
constexpr size_t kGrCarryOff = kGrStageBytes;                                 // double [kGrBN]
constexpr size_t kGrCmaxOff = kGrCarryOff + sizeof(double) * kGrBN;           // float [kGrBN]
constexpr size_t kGrVoffOff = kGrCmaxOff + sizeof(float) * kGrBN;             // int [kGrBM + 1]
constexpr size_t kGrPoffOff = kGrVoffOff + sizeof(int32_t) * (kGrBM + 1);     // int [kGrBN + 1]
constexpr size_t kGrEpiBytes = kGrPoffOff + sizeof(int32_t) * (kGrBN + 1);
constexpr size_t kGrSmem = TileSmem<kGrBM, kGrBN>::kBytes;
static_assert(kGrEpiBytes <= kGrSmem, "the epilogue must fit in the freed tile buffers");

constexpr int kGrRankT = 64;               // G tile of the rank kernel

struct GroupParams {
  const float* C;          // [Nc, D] clip rows
  const float* S;          // [Ns, D] caption rows
  int32_t D, B, use_max;
  int32_t row_tiles, col_tiles;
  int32_t group;           // row tiles per XCD group (2..4), 0 = plain row-major order
  const int32_t* clip_off; // [B + 1] (device copy of the plan)
  const int32_t* cap_off;  // [B + 1]
  const int32_t* rt_vid;   // [row_tiles + 1] first video of each row tile
  const int32_t* ct_par;   // [col_tiles + 1] first paragraph of each column tile
  float* G;                // [B, B]
};

// The (video, paragraph) blocks of one clip x caption tile, reduced from the accumulators nt_phase
// left (acc[2][2]: the wave's 64 x 64 quarter of the 128 x 128 tile) — the epilogue of
// group_sim_kernel and group_topk_select_kernel, called after nt_phase's closing barrier.  nv videos
// of nr clip rows, nq paragraphs; my_voff / my_poff: thread t <= nv / nq holds local offset t.  The
// scores are staged in two 64-row halves in the freed tile buffers and each block is reduced by one
// thread, clip-major then caption; a block whose video straddles the halves carries its running fp64
// sum (and max) across in LDS, which keeps the order.  sink(v, q, value) receives each block's value
// once (local video, local paragraph).  Ends with a barrier: the stage is free, every value sunk.
template <typename Sink>
__device__ __forceinline__ void group_tile_reduce(float* smem, const f32x16 (&acc)[2][2], int nv, int nq, int nr,
                                                  int my_voff, int my_poff, int use_max, Sink sink) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  char* lds = reinterpret_cast<char*>(smem);
  float* stage = smem;
  double* carry = reinterpret_cast<double*>(lds + kGrCarryOff);
  float* cmax = reinterpret_cast<float*>(lds + kGrCmaxOff);
  int* s_voff = reinterpret_cast<int*>(lds + kGrVoffOff);
  int* s_poff = reinterpret_cast<int*>(lds + kGrPoffOff);
  if (tid <= nv) s_voff[tid] = my_voff;
  if (tid <= nq) s_poff[tid] = my_poff;
  // work items of a pass: (video, paragraph) pairs, paragraph fastest (neighbouring threads read
  // neighbouring columns of the same staged rows)
  const int step_v = kThreads / nq, step_q = kThreads % nq;
  for (int h0 = 0; h0 < nr; h0 += kGrStageRows) {   // (uniform)
    const int h1 = (h0 + kGrStageRows < nr) ? h0 + kGrStageRows : nr;
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      const int row = wm * 64 + ms * 32 - h0;       // the wave's sub-tile origin relative to the pass
      if (row < 0 || row >= kGrStageRows) continue;  // (wave-uniform)
#pragma unroll
      for (int ns = 0; ns < 2; ++ns)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stage[(row + acc_row(r, lane)) * kGrLd + wn * 64 + ns * 32 + acc_col(lane)] = acc[ms][ns][r];
    }
    __syncthreads();   // staged scores (and, the first time, the offsets) visible to every wave
    // videos whose rows meet [h0, h1): [va, vb)
    int va = 0, vb = nv;
    while (s_voff[va + 1] <= h0) ++va;
    if (h1 < nr) {
      vb = va;
      while (s_voff[vb] < h1) ++vb;
    }
    const int items = (vb - va) * nq;
    int v = va + tid / nq, q = tid % nq;
    for (int w = tid; w < items; w += kThreads) {
      const int rs = s_voff[v], re = s_voff[v + 1];
      const int lo = rs > h0 ? rs : h0, hi = re < h1 ? re : h1;
      const int cs = s_poff[q], ce = s_poff[q + 1];
      const bool cont = rs < h0;                    // started in the previous pass
      if (use_max) {
        float m = cont ? cmax[q] : -INFINITY;
        for (int r = lo; r < hi; ++r) {
          const float* srow_ = stage + (r - h0) * kGrLd;
          for (int c = cs; c < ce; ++c) {
            const float x = srow_[c];
            m = x > m ? x : m;
          }
        }
        if (re > h1) cmax[q] = m;
        else sink(v, q, m);
      } else {
        double sum = cont ? carry[q] : 0.0;
        for (int r = lo; r < hi; ++r) {
          const float* srow_ = stage + (r - h0) * kGrLd;
          for (int c = cs; c < ce; ++c) sum += static_cast<double>(srow_[c]);
        }
        if (re > h1) carry[q] = sum;
        else sink(v, q, static_cast<float>(sum / static_cast<double>((re - rs) * (ce - cs))));
      }
      v += step_v;
      q += step_q;
      if (q >= nq) {
        q -= nq;
        ++v;
      }
    }
    __syncthreads();   // every thread is done with the stage (and has written its carries)
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_sim_kernel(const GroupParams p) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  int rt, ct;
  if (p.group > 0) {
    // a caption tile crosses the fabric once per group, the group's clip tiles stay L2-resident
    const TileIdx t = xcd_deal_tile(blockIdx.x, p.group, p.col_tiles);
    rt = t.rt;
    ct = t.ct;
    if (rt >= p.row_tiles) return;   // padding of the last row group / the grid
  } else {
    rt = blockIdx.x / p.col_tiles;
    ct = blockIdx.x % p.col_tiles;
  }
  const int v0 = p.rt_vid[rt], nv = p.rt_vid[rt + 1] - v0;
  const int q0 = p.ct_par[ct], nq = p.ct_par[ct + 1] - q0;
  const int r_begin = p.clip_off[v0], nr = p.clip_off[v0 + nv] - r_begin;
  const int c_begin = p.cap_off[q0], nc = p.cap_off[q0 + nq] - c_begin;
  // the tile's local video / paragraph offsets, loaded in front of the K loop (they go to LDS once
  // the tile buffers are free); nv, nq <= 128 (every video / paragraph has a row)
  const int my_voff = (tid <= nv) ? p.clip_off[v0 + tid] - r_begin : 0;
  const int my_poff = (tid <= nq) ? p.cap_off[q0 + tid] - c_begin : 0;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  rowaddr_t ar[kGrBM / 64], br[kGrBN / 64];
  bool av[kGrBM / 64], bv[kGrBN / 64];
#pragma unroll
  for (int i = 0; i < kGrBM / 64; ++i) ar[i] = tile_row(p.C, p.D, r_begin, srow + 64 * i, nr, &av[i]);
#pragma unroll
  for (int i = 0; i < kGrBN / 64; ++i) br[i] = tile_row(p.S, p.D, c_begin, srow + 64 * i, nc, &bv[i]);
  f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  // ends with a barrier: every wave is done with the tile buffers
  nt_phase<kGrBM, kGrBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
  group_tile_reduce(smem, acc, nv, nq, nr, my_voff, my_poff, p.use_max, [&](int v, int q, float g) {
    p.G[static_cast<int64_t>(v0 + v) * p.B + q0 + q] = g;
  });
}

// ---- group-wise top-K (cmhse_group_topk) ----------------------------------------------------------
// The query side is a clip row tile (v2p) or a caption column tile (p2v); the MFMA tile stays clips x
// captions either way, so group_tile_reduce's clip-major order holds for both directions.  LDS of a
// workgroup: the 40 KB tile buffers (the reduction's stage too), one 128-key candidate buffer per
// wave, then per query group its running list (K keys) and a row of block scores of the current
// gallery tile (at most 128 groups: every group has a row), for at most qcap(K) query groups.
constexpr int kGtGalleryMax = kGrBN;                       // groups of a gallery tile, at most
constexpr int kGtBlkLd = kGtGalleryMax + 1;                // block score row stride (floats)
constexpr size_t kGtCandOff = kGrSmem;                     // score_key_t [4 waves][128]
constexpr size_t kGtListOff = kGtCandOff + sizeof(score_key_t) * kGtGalleryMax * (kThreads / 64);
constexpr int kGtHdr = 8;                                  // Bv, Bp, Nc, Ns, direction, K, R, C
constexpr int kGtQcapMax = 64;
constexpr int kGtCUs = 256;                                // MI355X compute units
constexpr size_t kGtLdsPerCU = 160 * 1024;

struct GroupTopkParams {
  const float* C;          // [Nc, D] clip rows
  const float* S;          // [Ns, D] caption rows
  int32_t D, use_max, p2v, K;
  int32_t Bq;              // query groups
  int32_t q_tiles, g_tiles, panels;
  const int32_t* clip_off; // [Bv + 1] (device copy of the plan)
  const int32_t* cap_off;  // [Bp + 1]
  const int32_t* rt_vid;   // [R + 1] first video of each clip tile
  const int32_t* ct_par;   // [C + 1] first paragraph of each caption tile
  score_key_t* ws;         // [panels, Bq, K] sorted keys of each panel
};

// Grid: query tiles x gallery PANELS (runs of gallery tiles), panel-major, dealt to the XCDs in
// contiguous runs as topk_select_kernel's: the query tiles of a panel stream its gallery tiles
// through one L2.  Per gallery tile: nt_phase, the block reduction into blk [query][gallery], then
// each wave takes every fourth query group: a ballot of key > the query's K-th key picks the
// candidates, wave_merge adds them to its list.  The panel's lists go to the workspace.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_topk_select_kernel(const GroupTopkParams p) {
  const int per_xcd = static_cast<int>(gridDim.x >> 3);
  const int L = static_cast<int>(blockIdx.x & 7) * per_xcd + static_cast<int>(blockIdx.x >> 3);
  if (L >= p.q_tiles * p.panels) return;   // padding of the grid to a multiple of 8
  const int panel = L / p.q_tiles, qt = L % p.q_tiles;
  const int t_begin = static_cast<int>(static_cast<int64_t>(panel) * p.g_tiles / p.panels);
  const int t_end = static_cast<int>(static_cast<int64_t>(panel + 1) * p.g_tiles / p.panels);
  const int K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  const int32_t* q_start = p.p2v ? p.ct_par : p.rt_vid;
  const int32_t* g_start = p.p2v ? p.rt_vid : p.ct_par;
  const int qg0 = q_start[qt], nQ = q_start[qt + 1] - qg0;   // nQ <= qcap(K): the plan is checked

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  score_key_t* cand = reinterpret_cast<score_key_t*>(lds + kGtCandOff) + wave * kGtGalleryMax;
  score_key_t* lists = reinterpret_cast<score_key_t*>(lds + kGtListOff);   // [nQ][K]
  float* blk = reinterpret_cast<float*>(lds + kGtListOff + sizeof(score_key_t) * nQ * K);   // [nQ][kGtBlkLd]
  for (int e = tid; e < nQ * K; e += kThreads) lists[e] = 0ull;   // (seen after nt_phase's barriers)

  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  for (int t = t_begin; t < t_end; ++t) {
    const int gg0 = g_start[t], nG = g_start[t + 1] - gg0;
    const int v0 = p.p2v ? gg0 : qg0, nv = p.p2v ? nG : nQ;
    const int q0 = p.p2v ? qg0 : gg0, nq = p.p2v ? nQ : nG;
    const int r_begin = p.clip_off[v0], nr = p.clip_off[v0 + nv] - r_begin;
    const int c_begin = p.cap_off[q0], nc = p.cap_off[q0 + nq] - c_begin;
    const int my_voff = (tid <= nv) ? p.clip_off[v0 + tid] - r_begin : 0;
    const int my_poff = (tid <= nq) ? p.cap_off[q0 + tid] - c_begin : 0;
    rowaddr_t ar[kGrBM / 64], br[kGrBN / 64];
    bool av[kGrBM / 64], bv[kGrBN / 64];
#pragma unroll
    for (int i = 0; i < kGrBM / 64; ++i) ar[i] = tile_row(p.C, p.D, r_begin, srow + 64 * i, nr, &av[i]);
#pragma unroll
    for (int i = 0; i < kGrBN / 64; ++i) br[i] = tile_row(p.S, p.D, c_begin, srow + 64 * i, nc, &bv[i]);
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    // ends with a barrier: every wave is done with the tile buffers (and with the previous tile's
    // selection, so blk is free)
    nt_phase<kGrBM, kGrBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
    const bool p2v = p.p2v;
    group_tile_reduce(smem, acc, nv, nq, nr, my_voff, my_poff, p.use_max, [&](int v, int q, float g) {
      blk[p2v ? q * kGtBlkLd + v : v * kGtBlkLd + q] = g;
    });
    for (int qi = wave; qi < nQ; qi += kThreads / 64) {   // (wave-uniform)
      score_key_t* lst = lists + qi * K;
      const score_key_t thr = lst[K - 1];
      const float* row = blk + qi * kGtBlkLd;
      const score_key_t k0 = lane < nG ? score_key(row[lane], gg0 + lane) : 0ull;
      const score_key_t k1 = lane + 64 < nG ? score_key(row[lane + 64], gg0 + lane + 64) : 0ull;
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
  score_key_t* out = p.ws + (static_cast<int64_t>(panel) * p.Bq + qg0) * K;
  for (int e = tid; e < nQ * K; e += kThreads) out[e] = lists[e];
}

__global__ __launch_bounds__(kThreads) void group_topk_merge_kernel(const PanelLists p) {
  __shared__ score_key_t s_list[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ score_key_t s_cand[kThreads / 64][CMHSE_TOPK_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = blockIdx.x * (kThreads / 64) + wave;
  if (li >= p.nrows) return;   // (no barrier below)
  merge_panel_lists(p, li, s_list[wave], s_cand[wave], lane);
}

// ---- certified group-wise top-K (cmhse_group_topk_exact) -------------------------------------------
// The K best gallery groups of every query group by the FLOAT64 block scores G64 (exact64.hpp: block64, the one
// routine cmhse_group_rank_exact takes its scores from), certified.  cmhse_group_topk gives the K-th fp32 block
// score G_K(q) of every query; a second pass of the same grid, group_topk_exact_select_kernel, takes every
// gallery group with fl(G_K(q) - G32(q,g)) <= tol_q through block64 and keeps the K best (float64 bits, gallery
// index) pairs per query in LDS; group_topk_exact_merge_kernel merges the panels.
// Why the candidates hold the whole float64 top-K: topk.hip's argument with group_exact_tolerance (exact64.hpp)
// in the place of exact_tolerance.  E_q bounds |G32(q,g) - G64(q,g)| for every gallery group g: the row-wise
// statement of exact64.hpp for a video query (A_q = the largest clip norm of video q, Bmax = the largest caption
// norm of the call), the column-wise one for a paragraph query (B_q and Amax); under 'mean' E_q carries the two
// float64 summations and the rounding of G32 to fp32, terms (2) and (3) there, which bound |G32 - G64| of ONE
// block and so serve a threshold G_K taken from another block of the same line as they serve the diagonal.
// tol_q = 2 E_q (1 + 2^-18).  The K groups of the fp32 list have G32 >= G_K, hence G64 >= G_K - E_q: the K-th
// largest G64 of the query is at least G_K - E_q.  A member g of the float64 top-K has G64(q,g) at least that
// (on a tie at the boundary too: the index decides among equals, the score bound is the same), so
// G32(q,g) >= G64(q,g) - E_q >= G_K - 2 E_q; the factor on tol_q covers the rounding of fl(G_K - G32).  The
// block scores of the second pass come out of the same nt_phase call and the same group_tile_reduce as the
// first's, bit for bit, so the fp32 list's own K groups always qualify (G_K - G32 <= 0) and every list fills.
// The exact top-K of a superset of the top-K is the top-K.
//
// LDS of a workgroup: the 40 KB tile buffers, one 128-pair candidate buffer per wave, then per query group its
// list (K pairs of 12 bytes), its row of block scores and three words (candidate count, G_K, tolerance):
// [tile][candidate bits 4 x 128][list bits nQ x K][candidate index 4 x 128][list index nQ x K][blk nQ x 129]
// [count nQ][G_K nQ][tol nQ] — the 64-bit arrays first.
constexpr size_t kGteFixed = kGrSmem + (sizeof(score_bits64_t) + sizeof(int32_t)) * kGtGalleryMax * (kThreads / 64);
constexpr size_t kGteRowWords = 3;

struct GroupTopkExactParams {
  GroupTopkParams t;        // the inputs, the plan and the grid (panels: this pass's own; ws unused)
  const float* g32;         // [Bq, K] the fp32 lists' scores: column K - 1 is G_K
  const float* tol;         // [Bq]
  score_bits64_t* ws_bits;  // [panels, Bq, K] sorted pairs of each panel
  int32_t* ws_idx;          // [panels, Bq, K]
  int32_t* ws_count;        // [panels, Bq] candidates of each panel
};

struct GroupTopkExactPreParams {
  const float* C;           // [Nc, D] clip rows
  const float* S;           // [Ns, D] caption rows
  int32_t D, Nc, Ns, p2v, Bq, use_max, scale;
  const int32_t* q_off;     // [Bq + 1] the query side's offsets (device copy of the plan)
  double* norm_q;           // [query rows]
  unsigned* norm_max;       // [0]: bits of the largest clip norm, [1]: of the largest caption norm (zeroed)
  float* tol;               // [Bq]
};

// group_exact_pre_kernel for two independent sets: one wave per clip / caption row, the largest norm of each
// side (rounded up to fp32, atomic max on the bits), and the norms of the QUERY side's rows stored (the
// gallery's are needed through their maximum only: the workspace does not grow with the gallery).
__global__ __launch_bounds__(kThreads) void group_topk_exact_pre_kernel(const GroupTopkExactPreParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= static_cast<int64_t>(p.Nc) + p.Ns) return;   // (wave-uniform)
  const bool cap = r >= p.Nc;
  const int64_t row = cap ? r - p.Nc : r;
  const float* x = (cap ? p.S : p.C) + row * p.D;
  const float* const xs[1] = {x};
  double xx[1];
  dot64_wide<1, 8>(x, xs, p.D, lane, xx);   // (dot64(x, x)'s bits, eight loads in flight)
  const double n = sqrt(xx[0]);
  if (lane == 0) {
    if (cap == (p.p2v != 0)) p.norm_q[row] = n;
    atomicMax(p.norm_max + (cap ? 1 : 0), __float_as_uint(round_up_f32(n)));
  }
}

// thread q < Bq: the query group's largest norm against the largest norm of the gallery side
__global__ void group_topk_exact_tol_kernel(const GroupTopkExactPreParams p) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.Bq) return;
  double mine = 0.0;
  for (int r = p.q_off[q]; r < p.q_off[q + 1]; ++r) mine = p.norm_q[r] > mine ? p.norm_q[r] : mine;
  const double other = static_cast<double>(__uint_as_float(p.norm_max[p.p2v ? 0 : 1]));
  p.tol[q] = round_up_f32(group_exact_tolerance(p.D, p.use_max != 0, mine, other) * static_cast<double>(p.scale));
}

// group_topk_select_kernel's walk, tile loop and block reduction (the fp32 block scores in blk are pass one's,
// bit for bit); per query group, the gallery groups that G_K cannot rule out get their block64 — all of them,
// so the count is a function of the inputs — and their pairs are merged into the query's list.  block64 keeps
// its clip-major orientation whichever side is the query.  Loops are bounded by the tile's 128 gallery groups
// and a block's 128 x 128 rows; nothing waits on another workgroup.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_topk_exact_select_kernel(const GroupTopkExactParams pp) {
  const GroupTopkParams& p = pp.t;
  // (group_topk_select_kernel's walk of the panel-major work list, as topk_lists.hpp restates it)
  const PanelWork w = panel_work(blockIdx.x, gridDim.x, p.q_tiles, p.g_tiles, p.panels);
  if (w.panel < 0) return;   // padding of the grid to a multiple of 8
  const int panel = w.panel, qt = w.row_tile;
  const int t_begin = w.t_begin, t_end = w.t_end;
  const int K = p.K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  const int32_t* q_start = p.p2v ? p.ct_par : p.rt_vid;
  const int32_t* g_start = p.p2v ? p.rt_vid : p.ct_par;
  const int qg0 = q_start[qt], nQ = q_start[qt + 1] - qg0;   // nQ <= gte_qcap(K): the plan is checked

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  score_bits64_t* cbits_all = reinterpret_cast<score_bits64_t*>(lds + kGrSmem);          // [waves][128]
  score_bits64_t* lbits = cbits_all + kGtGalleryMax * (kThreads / 64);                   // [nQ][K]
  int32_t* cidx_all = reinterpret_cast<int32_t*>(lbits + nQ * K);                        // [waves][128]
  int32_t* lidx = cidx_all + kGtGalleryMax * (kThreads / 64);                            // [nQ][K]
  float* blk = reinterpret_cast<float*>(lidx + nQ * K);                                  // [nQ][kGtBlkLd]
  int32_t* s_count = reinterpret_cast<int32_t*>(blk + nQ * kGtBlkLd);                    // [nQ]
  float* s_gk = reinterpret_cast<float*>(s_count + nQ);                                  // [nQ]
  float* s_tol = s_gk + nQ;                                                              // [nQ]
  score_bits64_t* cbits = cbits_all + wave * kGtGalleryMax;
  int32_t* cidx = cidx_all + wave * kGtGalleryMax;
  // (all seen after nt_phase's barriers; every panel has a tile: panels <= g_tiles)
  for (int e = tid; e < nQ * K; e += kThreads) {
    lbits[e] = 0ull;
    lidx[e] = kNoColumn;
  }
  if (tid < nQ) {
    s_count[tid] = 0;
    s_gk[tid] = pp.g32[static_cast<int64_t>(qg0 + tid) * K + (K - 1)];
    s_tol[tid] = pp.tol[qg0 + tid];
  }
  const bool use_max = p.use_max != 0;

  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  for (int t = t_begin; t < t_end; ++t) {
    const int gg0 = g_start[t], nG = g_start[t + 1] - gg0;
    const int v0 = p.p2v ? gg0 : qg0, nv = p.p2v ? nG : nQ;
    const int q0 = p.p2v ? qg0 : gg0, nq = p.p2v ? nQ : nG;
    const int r_begin = p.clip_off[v0], nr = p.clip_off[v0 + nv] - r_begin;
    const int c_begin = p.cap_off[q0], nc = p.cap_off[q0 + nq] - c_begin;
    const int my_voff = (tid <= nv) ? p.clip_off[v0 + tid] - r_begin : 0;
    const int my_poff = (tid <= nq) ? p.cap_off[q0 + tid] - c_begin : 0;
    rowaddr_t ar[kGrBM / 64], br[kGrBN / 64];
    bool av[kGrBM / 64], bv[kGrBN / 64];
#pragma unroll
    for (int i = 0; i < kGrBM / 64; ++i) ar[i] = tile_row(p.C, p.D, r_begin, srow + 64 * i, nr, &av[i]);
#pragma unroll
    for (int i = 0; i < kGrBN / 64; ++i) br[i] = tile_row(p.S, p.D, c_begin, srow + 64 * i, nc, &bv[i]);
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    // ends with a barrier: every wave is done with the tile buffers (and with the previous tile's
    // selection, so blk is free)
    nt_phase<kGrBM, kGrBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
    const bool p2v = p.p2v;
    group_tile_reduce(smem, acc, nv, nq, nr, my_voff, my_poff, p.use_max, [&](int v, int q, float g) {
      blk[p2v ? q * kGtBlkLd + v : v * kGtBlkLd + q] = g;
    });
    // (the wave index in a scalar register: the candidates' offsets and block64's loop bounds stay scalar)
    for (int qi = __builtin_amdgcn_readfirstlane(wave); qi < nQ; qi += kThreads / 64) {
      const float* row = blk + qi * kGtBlkLd;
      const float gk = s_gk[qi];
      const float tol = s_tol[qi];
      // not ruled out: NOT (fl(G_K - G32) > tol); tol >= 0, possibly +inf (every group); inputs finite, so the
      // difference is no NaN.  Slots past nG hold the previous tile's scores and are never candidates.
      const bool c0 = lane < nG && !(gk - row[lane] > tol);
      const bool c1 = lane + 64 < nG && !(gk - row[lane + 64] > tol);
      const unsigned long long m[2] = {__ballot(c0), __ballot(c1)};   // (wave-uniform, scalar registers)
      if ((m[0] | m[1]) == 0ull) continue;
      const int qg = qg0 + qi;
      // the query's own rows: its clips (v2p) or its captions (p2v); the candidate gives the other side
      const int own0 = p2v ? p.cap_off[qg] : p.clip_off[qg], own1 = p2v ? p.cap_off[qg + 1] : p.clip_off[qg + 1];
      int c = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        unsigned long long bits = m[h];
        while (bits != 0ull) {
          const int g = gg0 + 64 * h + (__ffsll(static_cast<long long>(bits)) - 1);
          bits &= bits - 1ull;
          const double s = p2v ? block64(p.C, p.S, p.D, p.clip_off[g], p.clip_off[g + 1], own0, own1, use_max, lane)
                               : block64(p.C, p.S, p.D, own0, own1, p.cap_off[g], p.cap_off[g + 1], use_max, lane);
          if (lane == 0) {
            cbits[c] = ordered_bits64(s);
            cidx[c] = g;
          }
          ++c;
        }
      }
      if (lane == 0) s_count[qi] += c;
      __builtin_amdgcn_wave_barrier();
      wave_merge_pairs(lbits + qi * K, lidx + qi * K, K, cbits, cidx, c, lane);
    }
  }
  __syncthreads();
  const int64_t out_row = static_cast<int64_t>(panel) * p.Bq + qg0;
  for (int e = tid; e < nQ * K; e += kThreads) {
    pp.ws_bits[out_row * K + e] = lbits[e];
    pp.ws_idx[out_row * K + e] = lidx[e];
  }
  if (tid < nQ) pp.ws_count[out_row + tid] = s_count[tid];
}

// One wave per query: the P panel lists into one, decoded to float64, and the panels' counts summed.
__global__ __launch_bounds__(kThreads) void group_topk_exact_merge_kernel(const PanelPairLists p) {
  __shared__ score_bits64_t s_lb[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ score_bits64_t s_cb[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ int32_t s_li[kThreads / 64][CMHSE_TOPK_MAX];
  __shared__ int32_t s_ci[kThreads / 64][CMHSE_TOPK_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = blockIdx.x * (kThreads / 64) + wave;
  if (li >= p.nrows) return;   // (no barrier below)
  merge_panel_pair_lists(p, li, s_lb[wave], s_li[wave], s_cb[wave], s_ci[wave], lane);
}

struct GroupRankParams {
  const float* G;          // [B, B]
  int32_t B, tiles;        // tiles = ceil(B / 64)
  int32_t* cnt_row;        // [tiles (column tile), B]
  score_key_t* key_row;
  int32_t* cnt_col;        // [tiles (row tile), B]
  score_key_t* key_col;
  int32_t *rank_v2p, *top1_v2p, *rank_p2v, *top1_p2v;
};

// count of x > d (x at an index other than `self`) and the top-1 key over the 64 lanes of a wave
__device__ __forceinline__ void wave_rank64(float x, bool valid, bool self, float d, int idx0, int* cnt,
                                            score_key_t* key) {
  const unsigned long long gt = __ballot(valid && !self && x > d);
  const unsigned ob = valid ? ordered_bits(x) : 0u;
  unsigned obmax = ob;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned o = __shfl_xor(obmax, s, 64);
    obmax = o > obmax ? o : obmax;
  }
  const unsigned long long eq = __ballot(valid && ob == obmax);
  const int best = idx0 + (__ffsll(static_cast<long long>(eq)) - 1);
  *cnt = __popcll(gt);
  *key = bits_key(obmax, best);
}

__global__ __launch_bounds__(kThreads) void group_rank_kernel(const GroupRankParams p) {
  __shared__ float s[kGrRankT][kGrRankT + 1];
  __shared__ float s_drow[kGrRankT], s_dcol[kGrRankT];
  const int it = blockIdx.x / p.tiles, jt = blockIdx.x % p.tiles;
  const int i0 = it * kGrRankT, j0 = jt * kGrRankT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t B = p.B;
  for (int e = tid; e < kGrRankT * kGrRankT; e += kThreads) {
    const int r = e / kGrRankT, c = e % kGrRankT;
    s[r][c] = (i0 + r < p.B && j0 + c < p.B) ? p.G[(i0 + r) * B + j0 + c] : 0.f;
  }
  if (tid < kGrRankT) {
    const int i = i0 + tid;
    s_drow[tid] = i < p.B ? p.G[i * (B + 1)] : 0.f;
  } else if (tid < 2 * kGrRankT) {
    const int j = j0 + tid - kGrRankT;
    s_dcol[tid - kGrRankT] = j < p.B ? p.G[j * (B + 1)] : 0.f;
  }
  __syncthreads();
  constexpr int kPerWave = kGrRankT / (kThreads / 64);
  for (int k = 0; k < kPerWave; ++k) {
    const int rr = wave * kPerWave + k;
    int cnt;
    score_key_t key;
    // row i = i0 + rr against the tile's 64 columns (lane = column)
    if (i0 + rr < p.B) {   // (wave-uniform)
      const int j = j0 + lane;
      wave_rank64(s[rr][lane], j < p.B, j == i0 + rr, s_drow[rr], j0, &cnt, &key);
      if (lane == 0) {
        p.cnt_row[jt * B + i0 + rr] = cnt;
        p.key_row[jt * B + i0 + rr] = key;
      }
    }
    // column j = j0 + rr against the tile's 64 rows (lane = row)
    if (j0 + rr < p.B) {
      const int i = i0 + lane;
      wave_rank64(s[lane][rr], i < p.B, i == j0 + rr, s_dcol[rr], i0, &cnt, &key);
      if (lane == 0) {
        p.cnt_col[it * B + j0 + rr] = cnt;
        p.key_col[it * B + j0 + rr] = key;
      }
    }
  }
}

// thread t < B: row t (video -> paragraph); B <= t < 2B: column t - B (paragraph -> video)
__global__ void group_rank_final_kernel(const GroupRankParams p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * p.B) return;
  const bool col = t >= p.B;
  const int i = col ? t - p.B : t;
  const int32_t* cnt = col ? p.cnt_col : p.cnt_row;
  const score_key_t* key = col ? p.key_col : p.key_row;
  int c = 0;
  score_key_t k = 0;
  for (int q = 0; q < p.tiles; ++q) {
    const int64_t e = static_cast<int64_t>(q) * p.B + i;
    c += cnt[e];
    k = key[e] > k ? key[e] : k;
  }
  const int32_t top1 = key_index(k);
  (col ? p.rank_p2v : p.rank_v2p)[i] = c;
  (col ? p.top1_p2v : p.top1_v2p)[i] = top1;
}

// ---- certified group-wise ranking (cmhse_group_rank_exact) ------------------------------------------
// The ranks of the FLOAT64 block scores G64 (exact64.hpp: block64, its bound and its tolerance) at the cost of
// cmhse_group_rank: group_sim_kernel's fp32 G decides every comparison whose difference exceeds the certified
// tolerance of its row (video -> paragraph) or column (paragraph -> video); the others are recomputed with
// block64 inside the G tile that found them.
//   group_exact_pre_kernel    one wave per clip / caption row: its norm sqrt(dot64(x, x)), and the largest norm
//                             of each side (rounded up to fp32, atomic max on the bits);
//   group_exact_tol_kernel    per video i: A_i and tol_v2p[i]; per paragraph j: B_j and tol_p2v[j]; the call's
//                             counters zeroed;
//   group_exact_diag_kernel   one wave per group: G64[i, i];
//   group_rank_exact_kernel   group_rank_kernel's tiles, two compares per element and direction, and the
//                             resolve step;
//   group_rank_exact_final_kernel   the partials, rank_hi = rank_lo + ties, top1 decoded.
struct GroupExactParams {
  const float* C;          // [Nc, D] clip rows
  const float* S;          // [Ns, D] caption rows
  int32_t D, B, Nc, Ns, use_max, scale;
  const int32_t* clip_off; // [B + 1] (device copy of the plan)
  const int32_t* cap_off;  // [B + 1]
  double* norm_c;          // [Nc]
  double* norm_s;          // [Ns]
  unsigned* norm_max;      // [0]: bits of the largest clip norm, [1]: of the largest caption norm (zeroed)
  double* d64;             // [B] G64[i, i]
  float* tol_v2p;          // [B]
  float* tol_p2v;          // [B]
  // rank_lo: the float64 "above" counts until the last launch adds the fp32 ones; rank_hi: the float64 ties
  int32_t *lo_v2p, *hi_v2p, *res_v2p, *lo_p2v, *hi_p2v, *res_p2v;
};

__global__ __launch_bounds__(kThreads) void group_exact_pre_kernel(const GroupExactParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (r >= static_cast<int64_t>(p.Nc) + p.Ns) return;   // (wave-uniform)
  const bool cap = r >= p.Nc;
  const float* x = cap ? p.S + (r - p.Nc) * p.D : p.C + r * p.D;
  const float* const xs[1] = {x};
  double xx[1];
  dot64_wide<1, 8>(x, xs, p.D, lane, xx);   // (dot64(x, x)'s bits, eight loads in flight)
  const double n = sqrt(xx[0]);
  if (lane == 0) {
    (cap ? p.norm_s[r - p.Nc] : p.norm_c[r]) = n;
    atomicMax(p.norm_max + (cap ? 1 : 0), __float_as_uint(round_up_f32(n)));
  }
}

// thread t < B: video t; B <= t < 2B: paragraph t - B (every group has 1 .. 128 rows: the plan is checked)
__global__ void group_exact_tol_kernel(const GroupExactParams p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * p.B) return;
  const bool par = t >= p.B;
  const int g = par ? t - p.B : t;
  const int32_t* off = par ? p.cap_off : p.clip_off;
  const double* norm = par ? p.norm_s : p.norm_c;
  double mine = 0.0;
  for (int r = off[g]; r < off[g + 1]; ++r) mine = norm[r] > mine ? norm[r] : mine;
  const double other = static_cast<double>(__uint_as_float(p.norm_max[par ? 0 : 1]));
  (par ? p.tol_p2v : p.tol_v2p)[g] =
      round_up_f32(group_exact_tolerance(p.D, p.use_max != 0, mine, other) * static_cast<double>(p.scale));
  (par ? p.lo_p2v : p.lo_v2p)[g] = 0;
  (par ? p.hi_p2v : p.hi_v2p)[g] = 0;
  (par ? p.res_p2v : p.res_v2p)[g] = 0;
}

__global__ __launch_bounds__(kThreads) void group_exact_diag_kernel(const GroupExactParams p) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (i >= p.B) return;   // (wave-uniform)
  const double g = block64(p.C, p.S, p.D, p.clip_off[i], p.clip_off[i + 1], p.cap_off[i], p.cap_off[i + 1],
                           p.use_max != 0, lane);
  if (lane == 0) p.d64[i] = g;
}

// wave_rank64 with a tolerance: the count of x surely above d, the mask of the undecided x, the top-1 key
__device__ __forceinline__ void wave_rank64_exact(float x, bool valid, bool self, float d, float tol, int idx0,
                                                  int* cnt, unsigned long long* amb, score_key_t* key) {
  // surely above: fl(x - d) > tol; surely below: fl(d - x) = -fl(x - d) > tol; else undecided (tol >= 0, finite
  // inputs: the difference is no NaN)
  const float diff = x - d;
  const bool mine = valid && !self;
  const unsigned long long gt = __ballot(mine && diff > tol);
  *amb = __ballot(mine && fabsf(diff) <= tol);
  const unsigned ob = valid ? ordered_bits(x) : 0u;
  unsigned obmax = ob;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned o = __shfl_xor(obmax, s, 64);
    obmax = o > obmax ? o : obmax;
  }
  const unsigned long long eq = __ballot(valid && ob == obmax);
  const int best = idx0 + (__ffsll(static_cast<long long>(eq)) - 1);
  *cnt = __popcll(gt);
  *key = bits_key(obmax, best);
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long x) {
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x));
  const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x >> 32));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

struct GroupRankExactParams {
  GroupRankParams r;       // G, the partials (cnt: the fp32-decided "above" counts), top1_*; rank_* unused
  GroupExactParams e;
};

// group_rank_kernel's tile and partials.  s_arow[r] holds the undecided columns of tile row r for the query
// "video i0 + r" (bit = tile column), s_acol[c] the undecided rows of tile column c for the query "paragraph
// j0 + c" (bit = tile row); every word is written before the barrier.  The resolve step: wave w takes the tile
// rows w, w + 4, ...; for row r the blocks either direction wants are the union of s_arow[r] and bit r of the 64
// s_acol words, each computed ONCE by block64 and compared with G64[i, i] and / or G64[j, j].  The barrier is
// reached by every thread, the loops are bounded by the tile's 64 rows and 64 bits, nothing waits on another
// workgroup, and the sums are integer atomics: they do not depend on who adds first.
__global__ __launch_bounds__(kThreads) void group_rank_exact_kernel(const GroupRankExactParams pp) {
  const GroupRankParams& p = pp.r;
  const GroupExactParams& q = pp.e;
  __shared__ float s[kGrRankT][kGrRankT + 1];
  __shared__ float s_drow[kGrRankT], s_dcol[kGrRankT], s_trow[kGrRankT], s_tcol[kGrRankT];
  __shared__ unsigned long long s_arow[kGrRankT], s_acol[kGrRankT];
  __shared__ int s_any;
  const int it = blockIdx.x / p.tiles, jt = blockIdx.x % p.tiles;
  const int i0 = it * kGrRankT, j0 = jt * kGrRankT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t B = p.B;
  for (int e = tid; e < kGrRankT * kGrRankT; e += kThreads) {
    const int r = e / kGrRankT, c = e % kGrRankT;
    s[r][c] = (i0 + r < p.B && j0 + c < p.B) ? p.G[(i0 + r) * B + j0 + c] : 0.f;
  }
  if (tid < kGrRankT) {
    const int i = i0 + tid;
    s_drow[tid] = i < p.B ? p.G[i * (B + 1)] : 0.f;
    s_trow[tid] = i < p.B ? q.tol_v2p[i] : 0.f;
  } else if (tid < 2 * kGrRankT) {
    const int j = j0 + tid - kGrRankT;
    s_dcol[tid - kGrRankT] = j < p.B ? p.G[j * (B + 1)] : 0.f;
    s_tcol[tid - kGrRankT] = j < p.B ? q.tol_p2v[j] : 0.f;
  } else if (tid == 2 * kGrRankT) {
    s_any = 0;
  }
  __syncthreads();
  constexpr int kPerWave = kGrRankT / (kThreads / 64);
  for (int k = 0; k < kPerWave; ++k) {
    const int rr = wave * kPerWave + k;
    int cnt;
    unsigned long long amb;
    score_key_t key;
    // row i = i0 + rr against the tile's 64 columns (lane = column)
    if (i0 + rr < p.B) {   // (wave-uniform)
      const int j = j0 + lane;
      wave_rank64_exact(s[rr][lane], j < p.B, j == i0 + rr, s_drow[rr], s_trow[rr], j0, &cnt, &amb, &key);
      if (lane == 0) {
        p.cnt_row[jt * B + i0 + rr] = cnt;
        p.key_row[jt * B + i0 + rr] = key;
      }
    } else {
      amb = 0ull;
    }
    if (lane == 0) {
      s_arow[rr] = amb;
      if (amb != 0ull) s_any = 1;
    }
    // column j = j0 + rr against the tile's 64 rows (lane = row)
    if (j0 + rr < p.B) {
      const int i = i0 + lane;
      wave_rank64_exact(s[lane][rr], i < p.B, i == j0 + rr, s_dcol[rr], s_tcol[rr], i0, &cnt, &amb, &key);
      if (lane == 0) {
        p.cnt_col[it * B + j0 + rr] = cnt;
        p.key_col[it * B + j0 + rr] = key;
      }
    } else {
      amb = 0ull;
    }
    if (lane == 0) {
      s_acol[rr] = amb;
      if (amb != 0ull) s_any = 1;
    }
  }
  __syncthreads();
  if (s_any == 0) return;   // (workgroup-uniform: every thread reads the same word, past the last barrier)
  const bool use_max = q.use_max != 0;
  for (int r = wave; r < kGrRankT; r += kThreads / 64) {
    // (rows and columns past B set no bit; both masks are wave-uniform, and held in scalar registers)
    const unsigned long long rbits = uniform64(s_arow[r]);
    const unsigned long long cbits = __ballot((s_acol[lane] >> r) & 1ull);
    unsigned long long bits = rbits | cbits;
    if (bits == 0ull) continue;
    const int i = i0 + r;
    const int r_begin = q.clip_off[i], r_end = q.clip_off[i + 1];
    const double dii = q.d64[i];
    int above = 0, equal = 0, n = 0;
    while (bits != 0ull) {
      const int c = __ffsll(static_cast<long long>(bits)) - 1;
      bits &= bits - 1ull;
      const int j = j0 + c;
      const double g = block64(q.C, q.S, q.D, r_begin, r_end, q.cap_off[j], q.cap_off[j + 1], use_max, lane);
      if ((rbits >> c) & 1ull) {   // query: video i, its row of G
        above += g > dii;
        equal += g == dii;
        ++n;
      }
      if (((cbits >> c) & 1ull) && lane == 0) {   // query: paragraph j, its column of G
        const double djj = q.d64[j];
        if (g > djj) atomicAdd(&q.lo_p2v[j], 1);
        if (g == djj) atomicAdd(&q.hi_p2v[j], 1);
        atomicAdd(&q.res_p2v[j], 1);
      }
    }
    if (lane == 0 && n != 0) {
      if (above) atomicAdd(&q.lo_v2p[i], above);
      if (equal) atomicAdd(&q.hi_v2p[i], equal);
      atomicAdd(&q.res_v2p[i], n);
    }
  }
}

// thread t < B: row t (video -> paragraph); B <= t < 2B: column t - B (paragraph -> video).  rank_lo arrives
// holding the float64-decided "above" count, rank_hi the float64 ties.
__global__ void group_rank_exact_final_kernel(const GroupRankExactParams pp) {
  const GroupRankParams& p = pp.r;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * p.B) return;
  const bool col = t >= p.B;
  const int i = col ? t - p.B : t;
  const int32_t* cnt = col ? p.cnt_col : p.cnt_row;
  const score_key_t* key = col ? p.key_col : p.key_row;
  int c = 0;
  score_key_t k = 0;
  for (int q = 0; q < p.tiles; ++q) {
    const int64_t e = static_cast<int64_t>(q) * p.B + i;
    c += cnt[e];
    k = key[e] > k ? key[e] : k;
  }
  int32_t* lo = col ? pp.e.lo_p2v : pp.e.lo_v2p;
  int32_t* hi = col ? pp.e.hi_p2v : pp.e.hi_v2p;
  const int32_t rank_lo = lo[i] + c;
  lo[i] = rank_lo;
  hi[i] += rank_lo;
  (col ? p.top1_p2v : p.top1_v2p)[i] = key_index(k);
}

// prefix sums of B >= 1 positive counts, Nc / Ns at the end
bool offsets_ok(const int32_t* off, int32_t B) {
  if (off[0] != 0) return false;
  for (int32_t b = 0; b < B; ++b)
    if (off[b + 1] <= off[b]) return false;
  return true;
}

// the plan's tile starts: [0, ..., B], strictly increasing, every tile's rows <= cap and groups
// <= max_groups
bool tiles_ok(const int32_t* start, int32_t T, const int32_t* off, int32_t B, int cap,
              int32_t max_groups = 0x7fffffff) {
  if (T < 1 || T > B || start[0] != 0 || start[T] != B) return false;
  for (int32_t t = 0; t < T; ++t)
    if (start[t + 1] <= start[t] || off[start[t + 1]] - off[start[t]] > cap || start[t + 1] - start[t] > max_groups)
      return false;
  return true;
}

int32_t plan_len(int32_t B, int32_t R, int32_t Cc) { return kGrHdr + 2 * (B + 1) + (R + 1) + (Cc + 1); }

// The host plan checked in full (O(B)): what the kernel trusts — tile rows within the LDS arrays.
bool plan_ok(const int32_t* ph, int32_t plan_len_, int32_t B, int32_t Nc, int32_t Ns) {
  if (plan_len_ < kGrHdr || ph[0] != B || ph[1] != Nc || ph[2] != Ns) return false;
  const int32_t R = ph[3], Cc = ph[4];
  if (R < 1 || R > B || Cc < 1 || Cc > B || plan_len_ != plan_len(B, R, Cc)) return false;
  const int32_t* clip_off = ph + kGrHdr;
  const int32_t* cap_off = clip_off + B + 1;
  const int32_t* rt = cap_off + B + 1;
  const int32_t* ctp = rt + R + 1;
  return offsets_ok(clip_off, B) && offsets_ok(cap_off, B) && clip_off[B] == Nc && cap_off[B] == Ns &&
         tiles_ok(rt, R, clip_off, B, kGrBM) && tiles_ok(ctp, Cc, cap_off, B, kGrBN);
}

// greedy packing of whole groups (in order) into tiles of at most `cap` rows and `max_groups`
// groups; returns the tile count
int32_t pack(const int32_t* off, int32_t B, int cap, int32_t* start, int32_t max_groups = 0x7fffffff) {
  int32_t T = 0;
  start[T++] = 0;
  int32_t first = 0;
  for (int32_t b = 1; b < B; ++b)
    if (off[b + 1] - off[first] > cap || b - first >= max_groups) {
      start[T++] = b;
      first = b;
    }
  start[T] = B;
  return T;
}

// Query groups per query tile at K: as many as leave two workgroups' LDS per CU (the occupancy the
// GEMM keeps most of its rate at), in multiples of 8, at most 64; where that would be fewer than 32
// (K > 72), one workgroup per CU with 64.  K = 1 / 10 / 50 / 128: 64 / 56 / 40 / 64 query groups,
// 77 / 77 / 80 / 140 KB of LDS, 2 / 2 / 2 / 1 workgroups per CU.
int32_t gt_qcap(int32_t K) {
  const size_t per_q = sizeof(score_key_t) * K + sizeof(float) * kGtBlkLd;
  int32_t q = static_cast<int32_t>((kGtLdsPerCU / 2 - kGtListOff) / per_q) / 8 * 8;
  if (q < 32) q = static_cast<int32_t>((kGtLdsPerCU - kGtListOff) / per_q) / 8 * 8;
  return q > kGtQcapMax ? kGtQcapMax : q;
}

size_t gt_smem(int32_t K) {
  return kGtListOff + (sizeof(score_key_t) * K + sizeof(float) * kGtBlkLd) * static_cast<size_t>(gt_qcap(K));
}

// Panels per query tile, never more than there are gallery tiles.  Equal workgroups (a panel's share
// of the gallery each) run in rounds of `slots` resident ones, so a launch takes rounds / P panel
// lengths; from P0, the count that fills the slots once, up to 4 P0 + 3, a larger P is taken when it
// takes at least 10 % fewer (more panels: more workspace, more merging, more warm-up tiles).  At val_1
// (~140 query tiles) P0 is 1 at K = 128 (256 slots: over 100 CUs idle) and 3 at K = 50 (512 slots,
// ~420 busy); P = 7 runs both in nearly whole rounds.  The count depends on the query tiles and K
// only — it does not grow with the gallery, nor does the workspace.
int32_t gt_panels_for_smem(int32_t q_tiles, int32_t g_tiles, size_t smem) {
  int per_cu = static_cast<int>(kGtLdsPerCU / smem);
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  const int64_t slots = static_cast<int64_t>(kGtCUs) * per_cu;
  const int64_t P0 = slots / q_tiles < 1 ? 1 : slots / q_tiles;
  int64_t best = P0, best_rounds = (q_tiles * P0 + slots - 1) / slots;
  for (int64_t P = P0 + 1; P <= 4 * P0 + 3; ++P) {
    const int64_t rounds = (q_tiles * P + slots - 1) / slots;
    if (10 * rounds * best < 9 * best_rounds * P) {   // rounds / P < 0.9 best_rounds / best
      best = P;
      best_rounds = rounds;
    }
  }
  return static_cast<int32_t>(best < g_tiles ? best : g_tiles);
}

int32_t gt_panels(int32_t q_tiles, int32_t g_tiles, int32_t K) {
  return gt_panels_for_smem(q_tiles, g_tiles, gt_smem(K));
}

int64_t gt_plan_len(int64_t Bv, int64_t Bp, int64_t R, int64_t Cc) { return kGtHdr + Bv + Bp + R + Cc + 4; }

// The host top-K plan checked in full (O(Bv + Bp)) against the call: what the kernels trust — tile
// rows within the tile buffers, query groups per tile within the LDS lists.
bool gt_plan_ok(const int32_t* ph, int32_t len, int32_t Nc, int32_t Ns, int32_t direction, int32_t K) {
  if (!ph || len < kGtHdr) return false;
  const int32_t Bv = ph[0], Bp = ph[1], R = ph[6], Cc = ph[7];
  if (Bv < 1 || Bp < 1 || ph[2] != Nc || ph[3] != Ns || ph[4] != direction || ph[5] != K) return false;
  if (direction != CMHSE_GROUP_P2V && direction != CMHSE_GROUP_V2P) return false;
  const int32_t Bg = direction == CMHSE_GROUP_P2V ? Bv : Bp;
  if (K < 1 || K > CMHSE_TOPK_MAX || K > Bg) return false;
  if (R < 1 || R > Bv || Cc < 1 || Cc > Bp || len != gt_plan_len(Bv, Bp, R, Cc)) return false;
  const int32_t* clip_off = ph + kGtHdr;
  const int32_t* cap_off = clip_off + Bv + 1;
  const int32_t* rt = cap_off + Bp + 1;
  const int32_t* ctp = rt + R + 1;
  const int32_t qcap = gt_qcap(K);
  return offsets_ok(clip_off, Bv) && offsets_ok(cap_off, Bp) && clip_off[Bv] == Nc && cap_off[Bp] == Ns &&
         tiles_ok(rt, R, clip_off, Bv, kGrBM, direction == CMHSE_GROUP_V2P ? qcap : 0x7fffffff) &&
         tiles_ok(ctp, Cc, cap_off, Bp, kGrBN, direction == CMHSE_GROUP_P2V ? qcap : 0x7fffffff);
}


// ---- cmhse_group_topk_exact: its query-group cap, LDS, panels and plan check ----
// Query groups per query tile of the certified pass: gt_qcap's rule with this kernel's LDS (12-byte list
// entries, the pair candidate buffers, three words a group) — two workgroups per CU where that leaves at least
// 32 groups, else one — and never above gt_qcap(K), so a plan packed to this cap is valid for the nested fp32
// call too.  K = 1 / 10 / 50 / 128: 64 / 48 / 40 / 56 query groups, 80 / 76 / 90 / 159 KB of LDS, 2 / 2 / 1 / 1
// workgroups per CU (at K = 50 the rule's 64 is cut to gt_qcap's 40).
constexpr size_t gte_per_q(int32_t K) {
  return (sizeof(score_bits64_t) + sizeof(int32_t)) * K + sizeof(float) * kGtBlkLd + sizeof(int32_t) * kGteRowWords;
}

int32_t gte_qcap(int32_t K) {
  const size_t per_q = gte_per_q(K);
  int32_t q = static_cast<int32_t>((kGtLdsPerCU / 2 - kGteFixed) / per_q) / 8 * 8;
  if (q < 32) q = static_cast<int32_t>((kGtLdsPerCU - kGteFixed) / per_q) / 8 * 8;
  const int32_t q32 = gt_qcap(K);
  return q > q32 ? q32 : q;
}

size_t gte_smem(int32_t K) { return kGteFixed + gte_per_q(K) * static_cast<size_t>(gte_qcap(K)); }

int32_t gte_panels(int32_t q_tiles, int32_t g_tiles, int32_t K) {
  return gt_panels_for_smem(q_tiles, g_tiles, gte_smem(K));
}

// gt_plan_ok, and the query tiles within this pass's cap (a plan of cmhse_group_topk_plan can exceed it)
bool gte_plan_ok(const int32_t* ph, int32_t len, int32_t Nc, int32_t Ns, int32_t direction, int32_t K) {
  if (!gt_plan_ok(ph, len, Nc, Ns, direction, K)) return false;
  const int32_t Bv = ph[0], Bp = ph[1], R = ph[6], Cc = ph[7];
  const int32_t* rt = ph + kGtHdr + Bv + 1 + Bp + 1;
  const int32_t* start = direction == CMHSE_GROUP_P2V ? rt + R + 1 : rt;
  const int32_t T = direction == CMHSE_GROUP_P2V ? Cc : R, qcap = gte_qcap(K);
  for (int32_t t = 0; t < T; ++t)
    if (start[t + 1] - start[t] > qcap) return false;
  return true;
}

// cmhse_group_topk_plan and cmhse_group_topk_exact_plan: one layout, the query side capped at qcap groups a tile
int32_t gt_plan_fill(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host, int32_t Bp,
                     int32_t direction, int32_t K, int32_t* plan, int32_t plan_cap, int32_t (*qcap_of)(int32_t)) {
  if (!clip_off_host || !cap_off_host || !plan || Bv <= 0 || Bp <= 0) return CMHSE_ERR_ARG;
  if (direction != CMHSE_GROUP_P2V && direction != CMHSE_GROUP_V2P) return CMHSE_ERR_ARG;
  const int32_t Bg = direction == CMHSE_GROUP_P2V ? Bv : Bp;
  if (K < 1 || K > CMHSE_TOPK_MAX || K > Bg) return CMHSE_ERR_ARG;
  if (!offsets_ok(clip_off_host, Bv) || !offsets_ok(cap_off_host, Bp)) return CMHSE_ERR_ARG;
  for (int32_t b = 0; b < Bv; ++b)
    if (clip_off_host[b + 1] - clip_off_host[b] > kGrBM) return CMHSE_ERR_UNSUPPORTED;
  for (int32_t b = 0; b < Bp; ++b)
    if (cap_off_host[b + 1] - cap_off_host[b] > kGrBN) return CMHSE_ERR_UNSUPPORTED;
  if (plan_cap < gt_plan_len(Bv, Bp, Bv, Bp)) return CMHSE_ERR_WORKSPACE;   // CMHSE_GROUP_TOPK_PLAN_MAX
  plan[0] = Bv;
  plan[1] = Bp;
  plan[2] = clip_off_host[Bv];
  plan[3] = cap_off_host[Bp];
  plan[4] = direction;
  plan[5] = K;
  int32_t* clip_off = plan + kGtHdr;
  int32_t* cap_off = clip_off + Bv + 1;
  for (int32_t b = 0; b <= Bv; ++b) clip_off[b] = clip_off_host[b];
  for (int32_t b = 0; b <= Bp; ++b) cap_off[b] = cap_off_host[b];
  const int32_t qcap = qcap_of(K);
  int32_t* rt = cap_off + Bp + 1;
  const int32_t R = pack(clip_off, Bv, kGrBM, rt, direction == CMHSE_GROUP_V2P ? qcap : 0x7fffffff);
  const int32_t Cc = pack(cap_off, Bp, kGrBN, rt + R + 1, direction == CMHSE_GROUP_P2V ? qcap : 0x7fffffff);
  plan[6] = R;
  plan[7] = Cc;
  return static_cast<int32_t>(gt_plan_len(Bv, Bp, R, Cc));
}

bool group_args_ok(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D, int32_t B,
                   const int32_t* plan_host, const int32_t* plan, int32_t plan_len_, int32_t reduce) {
  if (!clips || !caps || !plan_host || !plan) return false;
  if (Nc <= 0 || Ns <= 0 || D <= 0 || B <= 0) return false;
  if (reduce != CMHSE_GROUP_MAX && reduce != CMHSE_GROUP_MEAN) return false;
  return plan_ok(plan_host, plan_len_, B, Nc, Ns);
}

int launch_group_sim(const float* clips, const float* caps, int32_t D, int32_t B, const int32_t* plan_host,
                     const int32_t* plan, int32_t reduce, float* G, hipStream_t stream) {
  GroupParams p;
  p.C = clips;
  p.S = caps;
  p.D = D;
  p.B = B;
  p.use_max = reduce == CMHSE_GROUP_MAX;
  p.row_tiles = plan_host[3];
  p.col_tiles = plan_host[4];
  p.clip_off = plan + kGrHdr;
  p.cap_off = p.clip_off + B + 1;
  p.rt_vid = p.cap_off + B + 1;
  p.ct_par = p.rt_vid + p.row_tiles + 1;
  p.G = G;
  const XcdDeal deal = xcd_deal(p.row_tiles, p.col_tiles);
  p.group = deal.group;
  if (deal.blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  return launch_tiles(group_sim_kernel<true>, group_sim_kernel<false>, D, dim3(static_cast<unsigned>(deal.blocks)),
                      kGrSmem, stream, p);
}


// ---- labelled group-wise ranking (cmhse_group_rank_labelled) ----------------------------------------
// rank[q] = #{ g : G(q, g) > thr[q] }, thr[q] = max over the positives p of query q of G(q, p), with G the block
// score of group_sim_kernel / group_topk_select_kernel, bit for bit: both passes below take every block score
// from nt_phase (each clip x caption score is its own MFMA k-chain: it depends on neither the row's place in the
// tile nor the tile's other rows) and group_tile_reduce (one thread per block, clip-major then caption, fp64 sum
// for the mean: a function of the block's scores alone).  So a threshold equals, bit for bit, the score the
// counting pass computes for the same (query, positive) block, and the strict compare is exact.
//
// Counting pass LDS: the 40 KB tile buffers, then per query group its running top-1 key (8 bytes), its threshold
// and its count (4 + 4) and a row of block scores of the current gallery tile (129 floats): 532 bytes a group.
// There are no K lists, so the query cap is kGlQcap = 72 groups a tile (gt_qcap(1) is 64): 40960 + 72 x 532 =
// 79264 bytes, the most that keeps TWO workgroups in a CU's 160 KB (the occupancy group_topk_select_kernel runs
// at; the whole 128 groups of a tile would take 109 KB, one workgroup per CU).  The cap binds only where groups
// average fewer than 1.8 rows; at val_1 (3.6 rows a group) the 128-row limit packs the query tiles.
constexpr int kGlHdr = 10;             // plan header: Bv, Bp, Nc, Ns, direction, R, C, n_pairs, T pair tiles, query cap
constexpr int kGlQcap = 72;            // query groups per query tile
constexpr int kGlPairMax = CMHSE_GROUP_TILE_ROWS;   // pairs of a pair tile, at most (every group has a row)
constexpr size_t kGlKeyOff = kGrSmem;                                            // score_key_t [kGlQcap]
constexpr size_t kGlThrOff = kGlKeyOff + sizeof(score_key_t) * kGlQcap;          // float [kGlQcap]
constexpr size_t kGlCntOff = kGlThrOff + sizeof(float) * kGlQcap;                // int [kGlQcap]
constexpr size_t kGlBlkOff = kGlCntOff + sizeof(int32_t) * kGlQcap;              // float [kGlQcap][kGtBlkLd]
constexpr size_t kGlCountSmem = kGlBlkOff + sizeof(float) * kGtBlkLd * kGlQcap;
static_assert(2 * kGlCountSmem <= kGtLdsPerCU, "two counting workgroups per CU");
// Threshold pass LDS behind the tile buffers (int32): the local clip / caption offsets of the tile's pairs
// [129 each, padded to 132], the first clip row of each pair's video and the first caption row of its paragraph,
// the pair's query and its positive [128 each], and the first wave's two scan totals.
constexpr int kGlLd = kGlPairMax + 4;
constexpr size_t kGlThresholdSmem = kGrSmem + sizeof(int32_t) * (2 * kGlLd + 4 * kGlPairMax + 4);

struct GroupLabelParams {
  const float* C;           // [Nc, D] clip rows
  const float* S;           // [Ns, D] caption rows
  int32_t D, use_max, p2v;
  int32_t Bq, Bg, n_pairs;
  int32_t q_tiles, g_tiles, panels;
  const int32_t* clip_off;  // [Bv + 1] (device copy of the plan)
  const int32_t* cap_off;   // [Bp + 1]
  const int32_t* rt_vid;    // [R + 1] first video of each clip tile
  const int32_t* ct_par;    // [C + 1] first paragraph of each caption tile
  const int32_t* pos_off;   // [Bq + 1]
  const int32_t* pos_idx;   // [n_pairs]
  const int32_t* pt_pair;   // [T + 1] first pair of each pair tile
  score_key_t* thrkey;      // [Bq] (zeroed)
  int32_t* cnt;             // [panels, Bq]
  score_key_t* key;         // [panels, Bq]
  int32_t *rank, *top1, *best_pos;
  float* best_score;        // or null
};

// One workgroup per pair tile.  Pair i of the tile (thread i) contributes the clip rows of its video and the
// caption rows of its paragraph — the query's group on one side, the positive's on the other — so local video i
// and local paragraph i are pair i's and the wanted blocks are the diagonal of the tile's np x np blocks.  A
// group that occurs in several pairs is simply gathered again.  The plan keeps the rows of either side <= 128.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_label_threshold_kernel(const GroupLabelParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int32_t* s_lv = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(smem) + kGrSmem);   // [np + 1]
  int32_t* s_lp = s_lv + kGlLd;                                                          // [np + 1]
  int32_t* s_vrow = s_lp + kGlLd;
  int32_t* s_prow = s_vrow + kGlPairMax;
  int32_t* s_query = s_prow + kGlPairMax;
  int32_t* s_pos = s_query + kGlPairMax;
  int32_t* s_tot = s_pos + kGlPairMax;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  const int k0 = p.pt_pair[blockIdx.x];
  int np = p.pt_pair[blockIdx.x + 1] - k0;
  np = np > kGlPairMax ? kGlPairMax : np;   // (validated on the host copy)
  if (np <= 0) return;                      // (workgroup-uniform, no barrier passed)
  int cv = 0, cp = 0;
  if (tid < np) {
    const int k = k0 + tid;
    // The query of pair k: the last q with pos_off[q] <= k.  Every list holds a positive, so q lies in
    // [k - (n_pairs - Bq), k]; every index read lies in [0, Bq), whatever the device copy holds.
    int lo = k - (p.n_pairs - p.Bq), hi = (k < p.Bq - 1) ? k : p.Bq - 1;
    lo = lo < 0 ? 0 : lo;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (p.pos_off[mid] <= k) lo = mid; else hi = mid - 1;
    }
    int g = p.pos_idx[k];
    g = g < 0 ? 0 : (g < p.Bg ? g : p.Bg - 1);   // (validated on the host copy)
    const int v = p.p2v ? g : lo, par = p.p2v ? lo : g;
    const int c0 = p.clip_off[v], s0 = p.cap_off[par];
    cv = p.clip_off[v + 1] - c0;
    cp = p.cap_off[par + 1] - s0;
    s_vrow[tid] = c0;
    s_prow[tid] = s0;
    s_query[tid] = lo;
    s_pos[tid] = g;
  }
  // inclusive scans of the two row counts over the tile's pairs (threads 0..127: two waves)
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int a = __shfl_up(cv, s, 64), b = __shfl_up(cp, s, 64);
    if (lane >= s) {
      cv += a;
      cp += b;
    }
  }
  if (tid == 63) {
    s_tot[0] = cv;
    s_tot[1] = cp;
  }
  __syncthreads();
  if (wave == 1) {
    cv += s_tot[0];
    cp += s_tot[1];
  }
  if (tid < kGlPairMax) {
    s_lv[tid + 1] = cv;
    s_lp[tid + 1] = cp;
  }
  if (tid == 0) {
    s_lv[0] = 0;
    s_lp[0] = 0;
  }
  __syncthreads();
  const int nr = s_lv[np], nc = s_lp[np];
  const int my_voff = (tid <= np) ? s_lv[tid] : 0;
  const int my_poff = (tid <= np) ? s_lp[tid] : 0;
  // operand rows: local row r belongs to the pair j with s_l*[j] <= r < s_l*[j + 1]
  rowaddr_t ar[kGrBM / 64], br[kGrBN / 64];
  bool av[kGrBM / 64], bv[kGrBN / 64];
#pragma unroll
  for (int i = 0; i < kGrBM / 64; ++i) {
    const int r = srow + 64 * i;
    av[i] = r < nr;
    int row = 0;
    if (av[i]) {
      int lo = 0, hi = np - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_lv[mid] <= r) lo = mid; else hi = mid - 1;
      }
      row = s_vrow[lo] + r - s_lv[lo];
    }
    ar[i] = row_addr(p.C + static_cast<int64_t>(row) * p.D);
  }
#pragma unroll
  for (int i = 0; i < kGrBN / 64; ++i) {
    const int r = srow + 64 * i;
    bv[i] = r < nc;
    int row = 0;
    if (bv[i]) {
      int lo = 0, hi = np - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_lp[mid] <= r) lo = mid; else hi = mid - 1;
      }
      row = s_prow[lo] + r - s_lp[lo];
    }
    br[i] = row_addr(p.S + static_cast<int64_t>(row) * p.D);
  }
  f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  nt_phase<kGrBM, kGrBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
  group_tile_reduce(smem, acc, np, np, nr, my_voff, my_poff, p.use_max, [&](int v, int q, float g) {
    if (v == q) atomicMax(&p.thrkey[s_query[v]], score_key(g, s_pos[v]));
  });
}

// group_topk_select_kernel's grid (panel_work restates its walk), tile loop and block reduction; the epilogue
// counts.  Wave w owns the query groups w, w + 4, ... of the tile through every gallery tile of the panel, so
// their running words in LDS have one writer.  The top-1 key is reduced over the wave only when some lane beats
// the running key (after the first tiles almost never).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_label_count_kernel(const GroupLabelParams p) {
  const PanelWork w = panel_work(blockIdx.x, gridDim.x, p.q_tiles, p.g_tiles, p.panels);
  if (w.panel < 0) return;   // padding of the grid to a multiple of 8
  const int panel = w.panel, qt = w.row_tile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, srow = tid >> 2;
  const int32_t* q_start = p.p2v ? p.ct_par : p.rt_vid;
  const int32_t* g_start = p.p2v ? p.rt_vid : p.ct_par;
  const int qg0 = q_start[qt], nQ = q_start[qt + 1] - qg0;   // nQ <= kGlQcap: the plan is checked

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);
  score_key_t* s_key = reinterpret_cast<score_key_t*>(lds + kGlKeyOff);
  float* s_thr = reinterpret_cast<float*>(lds + kGlThrOff);
  int32_t* s_cnt = reinterpret_cast<int32_t*>(lds + kGlCntOff);
  float* blk = reinterpret_cast<float*>(lds + kGlBlkOff);   // [nQ][kGtBlkLd]
  if (tid < nQ) {   // (seen after nt_phase's barriers; every panel has a tile: panels <= g_tiles)
    s_key[tid] = 0ull;
    s_cnt[tid] = 0;
    s_thr[tid] = key_score(p.thrkey[qg0 + tid]);
  }

  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  for (int t = w.t_begin; t < w.t_end; ++t) {
    const int gg0 = g_start[t], nG = g_start[t + 1] - gg0;
    const int v0 = p.p2v ? gg0 : qg0, nv = p.p2v ? nG : nQ;
    const int q0 = p.p2v ? qg0 : gg0, nq = p.p2v ? nQ : nG;
    const int r_begin = p.clip_off[v0], nr = p.clip_off[v0 + nv] - r_begin;
    const int c_begin = p.cap_off[q0], nc = p.cap_off[q0 + nq] - c_begin;
    const int my_voff = (tid <= nv) ? p.clip_off[v0 + tid] - r_begin : 0;
    const int my_poff = (tid <= nq) ? p.cap_off[q0 + tid] - c_begin : 0;
    rowaddr_t ar[kGrBM / 64], br[kGrBN / 64];
    bool av[kGrBM / 64], bv[kGrBN / 64];
#pragma unroll
    for (int i = 0; i < kGrBM / 64; ++i) ar[i] = tile_row(p.C, p.D, r_begin, srow + 64 * i, nr, &av[i]);
#pragma unroll
    for (int i = 0; i < kGrBN / 64; ++i) br[i] = tile_row(p.S, p.D, c_begin, srow + 64 * i, nc, &bv[i]);
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    // ends with a barrier: every wave is done with the tile buffers (and with the previous tile's
    // counting, so blk is free)
    nt_phase<kGrBM, kGrBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
    const bool p2v = p.p2v;
    group_tile_reduce(smem, acc, nv, nq, nr, my_voff, my_poff, p.use_max, [&](int v, int q, float g) {
      blk[p2v ? q * kGtBlkLd + v : v * kGtBlkLd + q] = g;
    });
    for (int qi = wave; qi < nQ; qi += kThreads / 64) {   // (wave-uniform)
      const float* row = blk + qi * kGtBlkLd;
      const float thr = s_thr[qi];
      const bool in0 = lane < nG, in1 = lane + 64 < nG;   // (slots past nG hold an earlier tile's scores)
      const float x0 = row[lane], x1 = row[lane + 64];
      const int c = __popcll(__ballot(in0 && x0 > thr)) + __popcll(__ballot(in1 && x1 > thr));
      const score_key_t k0 = in0 ? score_key(x0, gg0 + lane) : 0ull;
      const score_key_t k1 = in1 ? score_key(x1, gg0 + lane + 64) : 0ull;
      score_key_t best = k0 > k1 ? k0 : k1;
      const bool beats = __ballot(best > s_key[qi]) != 0ull;
      if (beats) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
          const unsigned hi = __shfl_xor(static_cast<unsigned>(best >> 32), s, 64);
          const unsigned lo = __shfl_xor(static_cast<unsigned>(best), s, 64);
          const score_key_t o = (static_cast<score_key_t>(hi) << 32) | lo;
          best = o > best ? o : best;
        }
      }
      if (lane == 0) {
        if (beats) s_key[qi] = best;
        s_cnt[qi] += c;
      }
    }
  }
  __syncthreads();
  if (tid < nQ) {
    const int64_t e = static_cast<int64_t>(panel) * p.Bq + qg0 + tid;
    p.cnt[e] = s_cnt[tid];
    p.key[e] = s_key[tid];
  }
}

// thread q < Bq: the panels' counts summed and keys maxed (integers: no order), the threshold key decoded
__global__ void group_label_final_kernel(const GroupLabelParams p) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.Bq) return;
  int c = 0;
  score_key_t k = 0;
  for (int P = 0; P < p.panels; ++P) {
    const int64_t e = static_cast<int64_t>(P) * p.Bq + q;
    c += p.cnt[e];
    k = p.key[e] > k ? p.key[e] : k;
  }
  const score_key_t tk = p.thrkey[q];
  p.rank[q] = c;
  p.top1[q] = key_index(k);
  p.best_pos[q] = key_index(tk);
  if (p.best_score) p.best_score[q] = key_score(tk);
}

// ---- cmhse_group_rank_labelled: its plan, its check and its workspace ----
// Layout (int32): the header (kGlHdr words), clip_off[Bv+1], cap_off[Bp+1], the first video of each clip tile
// [R+1], the first paragraph of each caption tile [C+1], pos_off[Bq+1], pos_idx[n_pairs], the first pair of
// each pair tile [T+1].
struct GlPlan {
  int32_t Bv, Bp, R, Cc, Bq, Bg, n_pairs, T;
  size_t clip_off, cap_off, rt, ct, pos_off, pos_idx, pt, len;   // word offsets
};

GlPlan gl_layout(int32_t Bv, int32_t Bp, int32_t direction, int32_t R, int32_t Cc, int32_t n_pairs, int32_t T) {
  GlPlan L;
  L.Bv = Bv, L.Bp = Bp, L.R = R, L.Cc = Cc, L.n_pairs = n_pairs, L.T = T;
  L.Bq = direction == CMHSE_GROUP_P2V ? Bp : Bv;
  L.Bg = direction == CMHSE_GROUP_P2V ? Bv : Bp;
  size_t o = kGlHdr;
  L.clip_off = o, o += static_cast<size_t>(Bv) + 1;
  L.cap_off = o, o += static_cast<size_t>(Bp) + 1;
  L.rt = o, o += static_cast<size_t>(R) + 1;
  L.ct = o, o += static_cast<size_t>(Cc) + 1;
  L.pos_off = o, o += static_cast<size_t>(L.Bq) + 1;
  L.pos_idx = o, o += static_cast<size_t>(n_pairs);
  L.pt = o, o += static_cast<size_t>(T) + 1;
  L.len = o;
  return L;
}

// the labels in full: 0 first, every list non-empty, n_pairs last, every index in [0, Bg)
bool labels_ok(const int32_t* pos_off, const int32_t* pos_idx, int32_t Bq, int32_t Bg, int32_t n_pairs) {
  if (n_pairs < Bq || pos_off[0] != 0 || pos_off[Bq] != n_pairs) return false;
  for (int32_t q = 0; q < Bq; ++q)
    if (pos_off[q + 1] <= pos_off[q]) return false;
  for (int32_t e = 0; e < n_pairs; ++e)
    if (pos_idx[e] < 0 || pos_idx[e] >= Bg) return false;
  return true;
}

// The pair tiles: whole pairs in CSR order, a tile closed when the next pair would take its clip rows or its
// caption rows past 128 (every group has at most 128 rows: a pair alone always fits).  start == nullptr only
// counts.  pair_tiles_ok accepts any cut that respects the limits, greedy or not.
int32_t pair_tiles(const int32_t* clip_off, const int32_t* cap_off, bool p2v, const int32_t* pos_off,
                   const int32_t* pos_idx, int32_t Bq, int32_t* start) {
  int32_t T = 0, k = 0;
  int rows_v = 0, rows_p = 0;
  for (int32_t q = 0; q < Bq; ++q)
    for (int32_t e = pos_off[q]; e < pos_off[q + 1]; ++e, ++k) {
      const int32_t v = p2v ? pos_idx[e] : q, par = p2v ? q : pos_idx[e];
      const int nv = clip_off[v + 1] - clip_off[v], npar = cap_off[par + 1] - cap_off[par];
      if (k == 0 || rows_v + nv > kGrBM || rows_p + npar > kGrBN) {
        if (start) start[T] = k;
        ++T;
        rows_v = rows_p = 0;
      }
      rows_v += nv;
      rows_p += npar;
    }
  if (start) start[T] = k;
  return T;
}

bool pair_tiles_ok(const int32_t* clip_off, const int32_t* cap_off, bool p2v, const int32_t* pos_off,
                   const int32_t* pos_idx, int32_t Bq, int32_t n_pairs, const int32_t* start, int32_t T) {
  if (T < 1 || T > n_pairs || start[0] != 0 || start[T] != n_pairs) return false;
  for (int32_t t = 0; t < T; ++t)
    if (start[t + 1] <= start[t]) return false;
  int32_t t = 0, k = 0;
  int rows_v = 0, rows_p = 0;
  for (int32_t q = 0; q < Bq; ++q)
    for (int32_t e = pos_off[q]; e < pos_off[q + 1]; ++e, ++k) {
      if (k == start[t + 1]) {
        ++t;
        rows_v = rows_p = 0;
      }
      const int32_t v = p2v ? pos_idx[e] : q, par = p2v ? q : pos_idx[e];
      rows_v += clip_off[v + 1] - clip_off[v];
      rows_p += cap_off[par + 1] - cap_off[par];
      if (rows_v > kGrBM || rows_p > kGrBN) return false;
    }
  return true;
}

// The host plan checked in full (O(Bv + Bp + n_pairs)) against the call: what the kernels trust — tile rows
// within the tile buffers, query groups per tile within the LDS words, labels inside the gallery, pair tiles
// within 128 rows either side.
bool gl_plan_ok(const int32_t* ph, int32_t len, int32_t Nc, int32_t Ns, int32_t direction) {
  if (!ph || len < kGlHdr) return false;
  const int32_t Bv = ph[0], Bp = ph[1], R = ph[5], Cc = ph[6], n_pairs = ph[7], T = ph[8];
  if (Bv < 1 || Bp < 1 || ph[2] != Nc || ph[3] != Ns || ph[4] != direction || ph[9] != kGlQcap) return false;
  if (direction != CMHSE_GROUP_P2V && direction != CMHSE_GROUP_V2P) return false;
  if (R < 1 || R > Bv || Cc < 1 || Cc > Bp || n_pairs < 1 || T < 1 || T > n_pairs) return false;
  const GlPlan L = gl_layout(Bv, Bp, direction, R, Cc, n_pairs, T);
  if (static_cast<size_t>(len) != L.len) return false;
  const bool p2v = direction == CMHSE_GROUP_P2V;
  return offsets_ok(ph + L.clip_off, Bv) && offsets_ok(ph + L.cap_off, Bp) && ph[L.clip_off + Bv] == Nc &&
         ph[L.cap_off + Bp] == Ns && tiles_ok(ph + L.rt, R, ph + L.clip_off, Bv, kGrBM, p2v ? 0x7fffffff : kGlQcap) &&
         tiles_ok(ph + L.ct, Cc, ph + L.cap_off, Bp, kGrBN, p2v ? kGlQcap : 0x7fffffff) &&
         labels_ok(ph + L.pos_off, ph + L.pos_idx, L.Bq, L.Bg, n_pairs) &&
         pair_tiles_ok(ph + L.clip_off, ph + L.cap_off, p2v, ph + L.pos_off, ph + L.pos_idx, L.Bq, n_pairs,
                       ph + L.pt, T);
}

// (plan_host: gl_plan_ok has passed)
GlPlan gl_plan_of(const int32_t* ph) { return gl_layout(ph[0], ph[1], ph[4], ph[5], ph[6], ph[7], ph[8]); }

int32_t gl_panels(const GlPlan& L, bool p2v) {
  return gt_panels_for_smem(p2v ? L.Cc : L.R, p2v ? L.R : L.Cc, kGlCountSmem);
}

// the threshold keys [Bq], then one count and one key per (panel, query group)
struct GlWs {
  size_t thrkey, cnt, key, total;
};
GlWs gl_ws(int32_t Bq, int32_t panels) {
  const size_t part = static_cast<size_t>(panels) * static_cast<size_t>(Bq);
  GlWs W;
  size_t off = 0;
  W.thrkey = off, off += align256(static_cast<size_t>(Bq) * sizeof(score_key_t));
  W.cnt = off, off += align256(part * sizeof(int32_t));
  W.key = off, off += align256(part * sizeof(score_key_t));
  W.total = off;
  return W;
}

}  // namespace
}  // namespace cmhse

using namespace cmhse;

extern "C" int32_t cmhse_group_plan(const int32_t* clip_off_host, const int32_t* cap_off_host, int32_t B,
                                    int32_t* plan, int32_t plan_cap) {
  if (!clip_off_host || !cap_off_host || !plan || B <= 0) return CMHSE_ERR_ARG;
  if (!offsets_ok(clip_off_host, B) || !offsets_ok(cap_off_host, B)) return CMHSE_ERR_ARG;
  for (int32_t b = 0; b < B; ++b)
    if (clip_off_host[b + 1] - clip_off_host[b] > kGrBM || cap_off_host[b + 1] - cap_off_host[b] > kGrBN)
      return CMHSE_ERR_UNSUPPORTED;
  if (plan_cap < CMHSE_GROUP_PLAN_MAX(B)) return CMHSE_ERR_WORKSPACE;
  plan[0] = B;
  plan[1] = clip_off_host[B];
  plan[2] = cap_off_host[B];
  int32_t* clip_off = plan + kGrHdr;
  int32_t* cap_off = clip_off + B + 1;
  for (int32_t b = 0; b <= B; ++b) {
    clip_off[b] = clip_off_host[b];
    cap_off[b] = cap_off_host[b];
  }
  int32_t* rt = cap_off + B + 1;
  const int32_t R = pack(clip_off, B, kGrBM, rt);
  const int32_t Cc = pack(cap_off, B, kGrBN, rt + R + 1);
  plan[3] = R;
  plan[4] = Cc;
  return plan_len(B, R, Cc);
}

extern "C" int cmhse_group_scores(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                  int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len_,
                                  int32_t reduce, float* G, void* stream_) {
  if (!G || !group_args_ok(clips, caps, Nc, Ns, D, B, plan_host, plan, plan_len_, reduce)) return CMHSE_ERR_ARG;
  const int rc = launch_group_sim(clips, caps, D, B, plan_host, plan, reduce, G, static_cast<hipStream_t>(stream_));
  if (rc != CMHSE_OK) return rc;
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" size_t cmhse_group_rank_workspace(int32_t B) {
  if (B <= 0) return 0;
  const size_t tiles = (static_cast<size_t>(B) + kGrRankT - 1) / kGrRankT;
  const size_t part = tiles * static_cast<size_t>(B);
  return align256(static_cast<size_t>(B) * static_cast<size_t>(B) * sizeof(float)) +
         2 * (align256(part * sizeof(int32_t)) + align256(part * sizeof(score_key_t)));
}

extern "C" int cmhse_group_rank(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len_,
                                int32_t reduce, int32_t* rank_v2p, int32_t* top1_v2p, int32_t* rank_p2v,
                                int32_t* top1_p2v, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!rank_v2p || !top1_v2p || !rank_p2v || !top1_p2v || !workspace ||
      !group_args_ok(clips, caps, Nc, Ns, D, B, plan_host, plan, plan_len_, reduce))
    return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 || workspace_bytes < cmhse_group_rank_workspace(B))
    return CMHSE_ERR_WORKSPACE;
  const int32_t tiles = (B + kGrRankT - 1) / kGrRankT;
  if (static_cast<int64_t>(tiles) * tiles > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  GroupRankParams rp;
  rp.G = reinterpret_cast<float*>(ws);
  ws += align256(static_cast<size_t>(B) * static_cast<size_t>(B) * sizeof(float));
  const size_t part = static_cast<size_t>(tiles) * static_cast<size_t>(B);
  rp.cnt_row = reinterpret_cast<int32_t*>(ws);
  ws += align256(part * sizeof(int32_t));
  rp.key_row = reinterpret_cast<score_key_t*>(ws);
  ws += align256(part * sizeof(score_key_t));
  rp.cnt_col = reinterpret_cast<int32_t*>(ws);
  ws += align256(part * sizeof(int32_t));
  rp.key_col = reinterpret_cast<score_key_t*>(ws);
  rp.B = B;
  rp.tiles = tiles;
  rp.rank_v2p = rank_v2p;
  rp.top1_v2p = top1_v2p;
  rp.rank_p2v = rank_p2v;
  rp.top1_p2v = top1_p2v;
  const int rc = launch_group_sim(clips, caps, D, B, plan_host, plan, reduce, const_cast<float*>(rp.G), stream);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(group_rank_kernel, dim3(static_cast<unsigned>(tiles * tiles)), dim3(kThreads), 0, stream, rp);
  hipLaunchKernelGGL(group_rank_final_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, stream, rp);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

namespace {
// cmhse_group_rank's regions first (G, the partials), then the O(B + Nc + Ns) vectors of the certified call
struct GroupExactWs {
  size_t d64, tol_v2p, tol_p2v, norm_c, norm_s, norm_max, total;
};
GroupExactWs group_exact_ws(int32_t B, int32_t Nc, int32_t Ns) {
  GroupExactWs L;
  size_t off = cmhse_group_rank_workspace(B);
  L.d64 = off, off += align256(static_cast<size_t>(B) * sizeof(double));
  L.tol_v2p = off, off += align256(static_cast<size_t>(B) * sizeof(float));
  L.tol_p2v = off, off += align256(static_cast<size_t>(B) * sizeof(float));
  L.norm_c = off, off += align256(static_cast<size_t>(Nc) * sizeof(double));
  L.norm_s = off, off += align256(static_cast<size_t>(Ns) * sizeof(double));
  L.norm_max = off, off += 256;
  L.total = off;
  return L;
}
}  // namespace

extern "C" size_t cmhse_group_rank_exact_workspace(int32_t B, int32_t Nc, int32_t Ns) {
  if (B <= 0 || Nc < B || Ns < B) return 0;   // (every group has a row)
  return group_exact_ws(B, Nc, Ns).total;
}

extern "C" double cmhse_group_rank_exact_tolerance(int32_t D, int32_t reduce, double norm_a, double norm_b_max) {
  if (D <= 0 || !(norm_a >= 0.0) || !(norm_b_max >= 0.0)) return NAN;
  if (reduce != CMHSE_GROUP_MAX && reduce != CMHSE_GROUP_MEAN) return NAN;
  return group_exact_tolerance(D, reduce == CMHSE_GROUP_MAX, norm_a, norm_b_max);
}

extern "C" int cmhse_group_rank_exact(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                      int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len_,
                                      int32_t reduce, int32_t* rank_lo_v2p, int32_t* rank_hi_v2p, int32_t* top1_v2p,
                                      int32_t* resolved_v2p, int32_t* rank_lo_p2v, int32_t* rank_hi_p2v,
                                      int32_t* top1_p2v, int32_t* resolved_p2v, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  if (!rank_lo_v2p || !rank_hi_v2p || !top1_v2p || !resolved_v2p || !rank_lo_p2v || !rank_hi_p2v || !top1_p2v ||
      !resolved_p2v || !workspace || !group_args_ok(clips, caps, Nc, Ns, D, B, plan_host, plan, plan_len_, reduce))
    return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_group_rank_exact_workspace(B, Nc, Ns))
    return CMHSE_ERR_WORKSPACE;
  const int32_t tiles = (B + kGrRankT - 1) / kGrRankT;
  if (static_cast<int64_t>(tiles) * tiles > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  if (D >= (1 << 24)) return CMHSE_ERR_UNSUPPORTED;   // (the bound needs D u < 1)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* const base = static_cast<char*>(workspace);
  char* ws = base;
  GroupRankExactParams pp;
  GroupRankParams& rp = pp.r;
  rp.G = reinterpret_cast<float*>(ws);
  ws += align256(static_cast<size_t>(B) * static_cast<size_t>(B) * sizeof(float));
  const size_t part = static_cast<size_t>(tiles) * static_cast<size_t>(B);
  rp.cnt_row = reinterpret_cast<int32_t*>(ws);
  ws += align256(part * sizeof(int32_t));
  rp.key_row = reinterpret_cast<score_key_t*>(ws);
  ws += align256(part * sizeof(score_key_t));
  rp.cnt_col = reinterpret_cast<int32_t*>(ws);
  ws += align256(part * sizeof(int32_t));
  rp.key_col = reinterpret_cast<score_key_t*>(ws);
  rp.B = B;
  rp.tiles = tiles;
  rp.rank_v2p = nullptr;
  rp.rank_p2v = nullptr;
  rp.top1_v2p = top1_v2p;
  rp.top1_p2v = top1_p2v;
  const GroupExactWs L = group_exact_ws(B, Nc, Ns);
  GroupExactParams& q = pp.e;
  q.C = clips;
  q.S = caps;
  q.D = D;
  q.B = B;
  q.Nc = Nc;
  q.Ns = Ns;
  q.use_max = reduce == CMHSE_GROUP_MAX;
  q.scale = tunables().rank_exact_tol_scale.load(std::memory_order_relaxed);
  q.clip_off = plan + kGrHdr;
  q.cap_off = q.clip_off + B + 1;
  q.norm_c = reinterpret_cast<double*>(base + L.norm_c);
  q.norm_s = reinterpret_cast<double*>(base + L.norm_s);
  q.norm_max = reinterpret_cast<unsigned*>(base + L.norm_max);
  q.d64 = reinterpret_cast<double*>(base + L.d64);
  q.tol_v2p = reinterpret_cast<float*>(base + L.tol_v2p);
  q.tol_p2v = reinterpret_cast<float*>(base + L.tol_p2v);
  q.lo_v2p = rank_lo_v2p;
  q.hi_v2p = rank_hi_v2p;
  q.res_v2p = resolved_v2p;
  q.lo_p2v = rank_lo_p2v;
  q.hi_p2v = rank_hi_p2v;
  q.res_p2v = resolved_p2v;
  constexpr int kWaves = kThreads / 64;
  if (hipMemsetAsync(q.norm_max, 0, 2 * sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  const int64_t pre_rows = static_cast<int64_t>(Nc) + Ns;
  hipLaunchKernelGGL(group_exact_pre_kernel, dim3(static_cast<unsigned>((pre_rows + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, stream, q);
  hipLaunchKernelGGL(group_exact_tol_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, stream, q);
  const int rc = launch_group_sim(clips, caps, D, B, plan_host, plan, reduce, const_cast<float*>(rp.G), stream);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(group_exact_diag_kernel, dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, q);
  hipLaunchKernelGGL(group_rank_exact_kernel, dim3(static_cast<unsigned>(tiles * tiles)), dim3(kThreads), 0, stream,
                     pp);
  hipLaunchKernelGGL(group_rank_exact_final_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, stream, pp);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int32_t cmhse_group_topk_plan(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host,
                                         int32_t Bp, int32_t direction, int32_t K, int32_t* plan, int32_t plan_cap) {
  return gt_plan_fill(clip_off_host, Bv, cap_off_host, Bp, direction, K, plan, plan_cap, gt_qcap);
}

extern "C" size_t cmhse_group_topk_workspace(const int32_t* plan_host, int32_t plan_len_) {
  if (!plan_host || plan_len_ < kGtHdr ||
      !gt_plan_ok(plan_host, plan_len_, plan_host[2], plan_host[3], plan_host[4], plan_host[5]))
    return 0;
  const bool p2v = plan_host[4] == CMHSE_GROUP_P2V;
  const int32_t Bq = p2v ? plan_host[1] : plan_host[0], K = plan_host[5];
  const int32_t q_tiles = p2v ? plan_host[7] : plan_host[6], g_tiles = p2v ? plan_host[6] : plan_host[7];
  return align256(static_cast<size_t>(gt_panels(q_tiles, g_tiles, K)) * static_cast<size_t>(Bq) *
                  static_cast<size_t>(K) * sizeof(score_key_t));
}

extern "C" int cmhse_group_topk(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                const int32_t* plan_host, const int32_t* plan, int32_t plan_len_, int32_t direction,
                                int32_t reduce, int32_t K, float* scores, int32_t* index, void* workspace,
                                size_t workspace_bytes, void* stream_) {
  if (!clips || !caps || !plan_host || !plan || !scores || !index || !workspace) return CMHSE_ERR_ARG;
  if (Nc <= 0 || Ns <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (reduce != CMHSE_GROUP_MAX && reduce != CMHSE_GROUP_MEAN) return CMHSE_ERR_ARG;
  if (!gt_plan_ok(plan_host, plan_len_, Nc, Ns, direction, K)) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_group_topk_workspace(plan_host, plan_len_))
    return CMHSE_ERR_WORKSPACE;
  const int32_t Bv = plan_host[0], Bp = plan_host[1], R = plan_host[6], Cc = plan_host[7];
  GroupTopkParams p;
  p.C = clips;
  p.S = caps;
  p.D = D;
  p.use_max = reduce == CMHSE_GROUP_MAX;
  p.p2v = direction == CMHSE_GROUP_P2V;
  p.K = K;
  p.Bq = p.p2v ? Bp : Bv;
  p.q_tiles = p.p2v ? Cc : R;
  p.g_tiles = p.p2v ? R : Cc;
  p.panels = gt_panels(p.q_tiles, p.g_tiles, K);
  p.clip_off = plan + kGtHdr;
  p.cap_off = p.clip_off + Bv + 1;
  p.rt_vid = p.cap_off + Bp + 1;
  p.ct_par = p.rt_vid + R + 1;
  p.ws = static_cast<score_key_t*>(workspace);
  const int64_t blocks = (static_cast<int64_t>(p.q_tiles) * p.panels + 7) / 8 * 8;
  if (blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = launch_tiles(group_topk_select_kernel<true>, group_topk_select_kernel<false>, D,
                              dim3(static_cast<unsigned>(blocks)), gt_smem(K), stream, p);
  if (rc != CMHSE_OK) return rc;
  const PanelLists lists = {p.ws, p.panels, p.Bq, K, scores, index};
  hipLaunchKernelGGL(group_topk_merge_kernel, dim3((p.Bq + 3) / 4), dim3(kThreads), 0, stream, lists);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int32_t cmhse_group_topk_exact_plan(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host,
                                               int32_t Bp, int32_t direction, int32_t K, int32_t* plan,
                                               int32_t plan_cap) {
  return gt_plan_fill(clip_off_host, Bv, cap_off_host, Bp, direction, K, plan, plan_cap, gte_qcap);
}

namespace {
// cmhse_group_topk's workspace (its panel keys) and its two outputs (the fp32 lists), the query rows' norms, the
// tolerances, the two largest norms, and one list of K pairs and one count per query group and panel.
struct GroupTopkExactWs {
  size_t keys32, scores32, index32, norm_q, tol, norm_max, bits, idx, count, total;
  int32_t panels;
};

// (plan_host: gte_plan_ok has passed)
GroupTopkExactWs group_topk_exact_ws(const int32_t* plan_host, int32_t plan_len_) {
  const bool p2v = plan_host[4] == CMHSE_GROUP_P2V;
  const int32_t K = plan_host[5];
  const size_t Bq = static_cast<size_t>(p2v ? plan_host[1] : plan_host[0]), nk = Bq * static_cast<size_t>(K);
  const size_t q_rows = static_cast<size_t>(p2v ? plan_host[3] : plan_host[2]);
  const int32_t q_tiles = p2v ? plan_host[7] : plan_host[6], g_tiles = p2v ? plan_host[6] : plan_host[7];
  GroupTopkExactWs L;
  L.panels = gte_panels(q_tiles, g_tiles, K);
  const size_t P = static_cast<size_t>(L.panels);
  size_t off = 0;
  L.keys32 = off, off += cmhse_group_topk_workspace(plan_host, plan_len_);
  L.scores32 = off, off += align256(nk * sizeof(float));
  L.index32 = off, off += align256(nk * sizeof(int32_t));
  L.norm_q = off, off += align256(q_rows * sizeof(double));
  L.tol = off, off += align256(Bq * sizeof(float));
  L.norm_max = off, off += 256;
  L.bits = off, off += align256(P * nk * sizeof(score_bits64_t));
  L.idx = off, off += align256(P * nk * sizeof(int32_t));
  L.count = off, off += align256(P * Bq * sizeof(int32_t));
  L.total = off;
  return L;
}
}  // namespace

extern "C" size_t cmhse_group_topk_exact_workspace(const int32_t* plan_host, int32_t plan_len_) {
  if (!plan_host || plan_len_ < kGtHdr ||
      !gte_plan_ok(plan_host, plan_len_, plan_host[2], plan_host[3], plan_host[4], plan_host[5]))
    return 0;
  return group_topk_exact_ws(plan_host, plan_len_).total;
}

extern "C" int cmhse_group_topk_exact(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                      const int32_t* plan_host, const int32_t* plan, int32_t plan_len_,
                                      int32_t direction, int32_t reduce, int32_t K, double* scores, int32_t* index,
                                      int32_t* resolved, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!clips || !caps || !plan_host || !plan || !scores || !index || !resolved || !workspace) return CMHSE_ERR_ARG;
  if (Nc <= 0 || Ns <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (reduce != CMHSE_GROUP_MAX && reduce != CMHSE_GROUP_MEAN) return CMHSE_ERR_ARG;
  // (cmhse_group_topk's plan check, and the query tiles within this pass's LDS)
  if (!gte_plan_ok(plan_host, plan_len_, Nc, Ns, direction, K)) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_group_topk_exact_workspace(plan_host, plan_len_))
    return CMHSE_ERR_WORKSPACE;
  if (D >= (1 << 24)) return CMHSE_ERR_UNSUPPORTED;   // (the bound needs D u < 1)
  const int32_t Bv = plan_host[0], Bp = plan_host[1], R = plan_host[6], Cc = plan_host[7];
  const GroupTopkExactWs L = group_topk_exact_ws(plan_host, plan_len_);
  char* const ws = static_cast<char*>(workspace);
  GroupTopkExactParams pp;
  GroupTopkParams& p = pp.t;
  p.C = clips;
  p.S = caps;
  p.D = D;
  p.use_max = reduce == CMHSE_GROUP_MAX;
  p.p2v = direction == CMHSE_GROUP_P2V;
  p.K = K;
  p.Bq = p.p2v ? Bp : Bv;
  p.q_tiles = p.p2v ? Cc : R;
  p.g_tiles = p.p2v ? R : Cc;
  p.panels = L.panels;
  p.clip_off = plan + kGtHdr;
  p.cap_off = p.clip_off + Bv + 1;
  p.rt_vid = p.cap_off + Bp + 1;
  p.ct_par = p.rt_vid + R + 1;
  p.ws = nullptr;
  pp.g32 = reinterpret_cast<float*>(ws + L.scores32);
  pp.tol = reinterpret_cast<float*>(ws + L.tol);
  pp.ws_bits = reinterpret_cast<score_bits64_t*>(ws + L.bits);
  pp.ws_idx = reinterpret_cast<int32_t*>(ws + L.idx);
  pp.ws_count = reinterpret_cast<int32_t*>(ws + L.count);
  constexpr int kWaves = kThreads / 64;
  const int64_t blocks = panel_grid_blocks(p.q_tiles, p.panels);
  const int64_t pre_blocks = (static_cast<int64_t>(Nc) + Ns + kWaves - 1) / kWaves;
  if (blocks > 0x7fffffffLL || pre_blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // 1. the fp32 lists: G_K (first: the one nested call that checks arguments of its own)
  int rc = cmhse_group_topk(clips, caps, Nc, Ns, D, plan_host, plan, plan_len_, direction, reduce, K,
                            reinterpret_cast<float*>(ws + L.scores32), reinterpret_cast<int32_t*>(ws + L.index32),
                            ws + L.keys32, cmhse_group_topk_workspace(plan_host, plan_len_), stream_);
  if (rc != CMHSE_OK) return rc;
  // 2. norms and tolerances
  GroupTopkExactPreParams q;
  q.C = clips;
  q.S = caps;
  q.D = D;
  q.Nc = Nc;
  q.Ns = Ns;
  q.p2v = p.p2v;
  q.Bq = p.Bq;
  q.use_max = p.use_max;
  q.scale = tunables().rank_exact_tol_scale.load(std::memory_order_relaxed);
  q.q_off = p.p2v ? p.cap_off : p.clip_off;
  q.norm_q = reinterpret_cast<double*>(ws + L.norm_q);
  q.norm_max = reinterpret_cast<unsigned*>(ws + L.norm_max);
  q.tol = reinterpret_cast<float*>(ws + L.tol);
  if (hipMemsetAsync(q.norm_max, 0, 2 * sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  hipLaunchKernelGGL(group_topk_exact_pre_kernel, dim3(static_cast<unsigned>(pre_blocks)), dim3(kThreads), 0, stream,
                     q);
  hipLaunchKernelGGL(group_topk_exact_tol_kernel, dim3((p.Bq + 255) / 256), dim3(256), 0, stream, q);
  // 3. the candidates in float64, 4. the panels merged
  rc = launch_tiles(group_topk_exact_select_kernel<true>, group_topk_exact_select_kernel<false>, D,
                    dim3(static_cast<unsigned>(blocks)), gte_smem(K), stream, pp);
  if (rc != CMHSE_OK) return rc;
  const PanelPairLists lists = {pp.ws_bits, pp.ws_idx, pp.ws_count, p.panels, p.Bq, K, scores, index, resolved};
  hipLaunchKernelGGL(group_topk_exact_merge_kernel, dim3((p.Bq + 3) / 4), dim3(kThreads), 0, stream, lists);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int32_t cmhse_group_rank_labelled_plan(const int32_t* clip_off_host, int32_t Bv,
                                                  const int32_t* cap_off_host, int32_t Bp, int32_t direction,
                                                  const int32_t* pos_off_host, const int32_t* pos_idx_host,
                                                  int32_t n_pairs, int32_t* plan, int32_t plan_cap) {
  if (!clip_off_host || !cap_off_host || !pos_off_host || !pos_idx_host || !plan || Bv <= 0 || Bp <= 0)
    return CMHSE_ERR_ARG;
  if (direction != CMHSE_GROUP_P2V && direction != CMHSE_GROUP_V2P) return CMHSE_ERR_ARG;
  if (!offsets_ok(clip_off_host, Bv) || !offsets_ok(cap_off_host, Bp)) return CMHSE_ERR_ARG;
  const bool p2v = direction == CMHSE_GROUP_P2V;
  const int32_t Bq = p2v ? Bp : Bv, Bg = p2v ? Bv : Bp;
  if (!labels_ok(pos_off_host, pos_idx_host, Bq, Bg, n_pairs)) return CMHSE_ERR_ARG;
  for (int32_t b = 0; b < Bv; ++b)
    if (clip_off_host[b + 1] - clip_off_host[b] > kGrBM) return CMHSE_ERR_UNSUPPORTED;
  for (int32_t b = 0; b < Bp; ++b)
    if (cap_off_host[b + 1] - cap_off_host[b] > kGrBN) return CMHSE_ERR_UNSUPPORTED;
  const int64_t need =
      3 * static_cast<int64_t>(Bv) + 3 * static_cast<int64_t>(Bp) + 2 * static_cast<int64_t>(n_pairs) + 16;
  if (need > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  if (plan_cap < need) return CMHSE_ERR_WORKSPACE;   // CMHSE_GROUP_RANK_LABELLED_PLAN_MAX
  // the offsets and the tiles first: the places of the labels and the pair tiles follow from R and C
  int32_t* clip_off = plan + kGlHdr;
  int32_t* cap_off = clip_off + Bv + 1;
  for (int32_t b = 0; b <= Bv; ++b) clip_off[b] = clip_off_host[b];
  for (int32_t b = 0; b <= Bp; ++b) cap_off[b] = cap_off_host[b];
  int32_t* rt = cap_off + Bp + 1;
  const int32_t R = pack(clip_off, Bv, kGrBM, rt, p2v ? 0x7fffffff : kGlQcap);
  int32_t* ctp = rt + R + 1;
  const int32_t Cc = pack(cap_off, Bp, kGrBN, ctp, p2v ? kGlQcap : 0x7fffffff);
  const int32_t T = pair_tiles(clip_off, cap_off, p2v, pos_off_host, pos_idx_host, Bq, nullptr);
  const GlPlan L = gl_layout(Bv, Bp, direction, R, Cc, n_pairs, T);
  for (int32_t q = 0; q <= Bq; ++q) plan[L.pos_off + q] = pos_off_host[q];
  for (int32_t e = 0; e < n_pairs; ++e) plan[L.pos_idx + e] = pos_idx_host[e];
  pair_tiles(clip_off, cap_off, p2v, pos_off_host, pos_idx_host, Bq, plan + L.pt);
  plan[0] = Bv;
  plan[1] = Bp;
  plan[2] = clip_off_host[Bv];
  plan[3] = cap_off_host[Bp];
  plan[4] = direction;
  plan[5] = R;
  plan[6] = Cc;
  plan[7] = n_pairs;
  plan[8] = T;
  plan[9] = kGlQcap;
  return static_cast<int32_t>(L.len);
}

extern "C" size_t cmhse_group_rank_labelled_workspace(const int32_t* plan_host, int32_t plan_len_) {
  if (!plan_host || plan_len_ < kGlHdr || !gl_plan_ok(plan_host, plan_len_, plan_host[2], plan_host[3], plan_host[4]))
    return 0;
  const GlPlan L = gl_plan_of(plan_host);
  return gl_ws(L.Bq, gl_panels(L, plan_host[4] == CMHSE_GROUP_P2V)).total;
}

extern "C" int cmhse_group_rank_labelled(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                                         const int32_t* plan_host, const int32_t* plan, int32_t plan_len_,
                                         int32_t direction, int32_t reduce, int32_t* rank, int32_t* top1,
                                         int32_t* best_pos, float* best_score, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
  if (!clips || !caps || !plan_host || !plan || !rank || !top1 || !best_pos || !workspace) return CMHSE_ERR_ARG;
  if (Nc <= 0 || Ns <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (reduce != CMHSE_GROUP_MAX && reduce != CMHSE_GROUP_MEAN) return CMHSE_ERR_ARG;
  if (!gl_plan_ok(plan_host, plan_len_, Nc, Ns, direction)) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_group_rank_labelled_workspace(plan_host, plan_len_))
    return CMHSE_ERR_WORKSPACE;
  const GlPlan L = gl_plan_of(plan_host);
  GroupLabelParams p;
  p.C = clips;
  p.S = caps;
  p.D = D;
  p.use_max = reduce == CMHSE_GROUP_MAX;
  p.p2v = direction == CMHSE_GROUP_P2V;
  p.Bq = L.Bq;
  p.Bg = L.Bg;
  p.n_pairs = L.n_pairs;
  p.q_tiles = p.p2v ? L.Cc : L.R;
  p.g_tiles = p.p2v ? L.R : L.Cc;
  p.panels = gl_panels(L, p.p2v != 0);
  p.clip_off = plan + L.clip_off;
  p.cap_off = plan + L.cap_off;
  p.rt_vid = plan + L.rt;
  p.ct_par = plan + L.ct;
  p.pos_off = plan + L.pos_off;
  p.pos_idx = plan + L.pos_idx;
  p.pt_pair = plan + L.pt;
  const GlWs W = gl_ws(L.Bq, p.panels);
  char* const ws = static_cast<char*>(workspace);
  p.thrkey = reinterpret_cast<score_key_t*>(ws + W.thrkey);
  p.cnt = reinterpret_cast<int32_t*>(ws + W.cnt);
  p.key = reinterpret_cast<score_key_t*>(ws + W.key);
  p.rank = rank;
  p.top1 = top1;
  p.best_pos = best_pos;
  p.best_score = best_score;
  const int64_t blocks = panel_grid_blocks(p.q_tiles, p.panels);
  if (blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (hipMemsetAsync(p.thrkey, 0, sizeof(score_key_t) * static_cast<size_t>(L.Bq), stream) != hipSuccess)
    return CMHSE_ERR_LAUNCH;
  // 1. the thresholds, 2. the counts and top-1 keys of each panel, 3. the panels combined
  int rc = launch_tiles(group_label_threshold_kernel<true>, group_label_threshold_kernel<false>, D,
                        dim3(static_cast<unsigned>(L.T)), kGlThresholdSmem, stream, p);
  if (rc != CMHSE_OK) return rc;
  rc = launch_tiles(group_label_count_kernel<true>, group_label_count_kernel<false>, D,
                    dim3(static_cast<unsigned>(blocks)), kGlCountSmem, stream, p);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(group_label_final_kernel, dim3((L.Bq + 255) / 256), dim3(256), 0, stream, p);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}
