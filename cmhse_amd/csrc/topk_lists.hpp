// topk_lists.hpp — the sorted key lists of the top-K kernels: topk.hip (cmhse_sim_topk) and group.hip
// (cmhse_group_topk) keep, per query, a descending list of K score keys (score_tile.hpp) in LDS,
// grown by wave_merge, one list per gallery panel in the workspace, and merged across the panels by
// merge_panel_lists.  cmhse_sim_topk_exact (topk.hip) keeps the same lists with a two-word key, the ordered
// bits of a float64 score and the column: wave_merge_pairs / merge_panel_pair_lists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "score_tile.hpp"

namespace cmhse {

// One wave merges c candidate keys (cand[0, c), unsorted, c <= 128, all above lst[K - 1]) into the
// descending list lst[0, K) (0 = empty slot; a real key is never 0).  Keys are unique, so each one's
// place in the merged order is its rank: a list entry moves down by the candidates above it, a
// candidate lands at (list entries above it) + (candidates above it); what lands past K drops out.
// Every lane has read all it needs before any lane writes (lock-step wave, in-order LDS).
__device__ __forceinline__ void wave_merge(score_key_t* lst, int K, const score_key_t* cand, int c, int lane) {
  score_key_t lv[2], cv[2];
  int lr[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    lv[h] = e < K ? lst[e] : 0ull;
    cv[h] = e < c ? cand[e] : 0ull;
  }
  for (int q = 0; q < c; ++q) {
    const score_key_t x = cand[q];   // (one address for the whole wave: a broadcast read)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      lr[h] += x > lv[h];
      cr[h] += x > cv[h];
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (lane + 64 * h < c) {
      int lo = 0, hi = K;       // list entries above the candidate (descending, empty slots last)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lst[mid] > cv[h]) lo = mid + 1;
        else hi = mid;
      }
      cr[h] += lo;
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    if (e < K && e + lr[h] < K) lst[e + lr[h]] = lv[h];
    if (e < c && cr[h] < K) lst[cr[h]] = cv[h];
  }
  __builtin_amdgcn_wave_barrier();
}

// The panel lists of one query row: ws [panels, nrows, K] (each list sorted, its real keys a prefix).
struct PanelLists {
  const score_key_t* ws;
  int32_t panels, nrows, K;
  float* scores;     // [nrows, K]
  int32_t* index;    // [nrows, K]
};

// One wave merges the P panel lists of row li into one and decodes the keys (the float comes back
// from its bits).  lst / cand: the wave's CMHSE_TOPK_MAX keys of LDS each.
__device__ __forceinline__ void merge_panel_lists(const PanelLists& p, int li, score_key_t* lst, score_key_t* cand,
                                                  int lane) {
  const int K = p.K;
  for (int e = lane; e < K; e += 64) lst[e] = 0ull;
  __builtin_amdgcn_wave_barrier();
  for (int q = 0; q < p.panels; ++q) {
    const score_key_t* src = p.ws + (static_cast<int64_t>(q) * p.nrows + li) * K;
    const score_key_t thr = lst[K - 1];
    const score_key_t k0 = lane < K ? src[lane] : 0ull;
    const score_key_t k1 = lane + 64 < K ? src[lane + 64] : 0ull;
    const bool c0 = k0 > thr, c1 = k1 > thr;
    const int c = __popcll(__ballot(c0)) + __popcll(__ballot(c1));
    if (c == 0) continue;
    if (c0) cand[lane] = k0;
    if (c1) cand[lane + 64] = k1;
    __builtin_amdgcn_wave_barrier();
    wave_merge(lst, K, cand, c, lane);
  }
  for (int e = lane; e < K; e += 64) {
    const score_key_t key = lst[e];
    p.scores[static_cast<int64_t>(li) * K + e] = key_score(key);
    p.index[static_cast<int64_t>(li) * K + e] = key_index(key);
  }
}

// ---------------------------------------------------------------------------------------------
// The same lists with a two-word key (cmhse_sim_topk_exact): a float64 score does not fit a 64-bit key
// beside its column, so a list is two arrays, the ordered bits of the score (64-bit) and the column
// (32-bit), ordered by (bits descending, column ascending) — the order of the score key, on float64.
// ---------------------------------------------------------------------------------------------
typedef unsigned long long score_bits64_t;
constexpr int32_t kNoColumn = 0x7fffffff;   // the column of an empty slot (bits 0)

// monotone map double -> uint64 (total order of non-NaN doubles; never 0).  -0.0 and +0.0 compare equal
// as doubles and must tie: the sign of zero is canonicalised first.
__device__ __forceinline__ score_bits64_t ordered_bits64(double s) {
  if (s == 0.0) s = 0.0;
  const score_bits64_t u = static_cast<score_bits64_t>(__double_as_longlong(s));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double bits64_score(score_bits64_t ob) {
  return __longlong_as_double(static_cast<long long>((ob >> 63) ? (ob & 0x7fffffffffffffffull) : ~ob));
}

// x before y in a list: the larger score, then the smaller column.  Columns are unique per row, so no two
// real pairs are equal; every real pair (bits != 0) lies before an empty slot (0, kNoColumn).
__device__ __forceinline__ bool pair_before(score_bits64_t xb, int32_t xi, score_bits64_t yb, int32_t yi) {
  return xb > yb || (xb == yb && xi < yi);
}

// wave_merge on pairs: c candidates (cb / ci [0, c), unsorted, c <= 128, any values) into the descending
// list (lb / li [0, K)).  Same ranks, same lock-step reads before writes.
__device__ __forceinline__ void wave_merge_pairs(score_bits64_t* lb, int32_t* li, int K, const score_bits64_t* cb,
                                                 const int32_t* ci, int c, int lane) {
  score_bits64_t lvb[2], cvb[2];
  int32_t lvi[2], cvi[2];
  int lr[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    lvb[h] = e < K ? lb[e] : 0ull;
    lvi[h] = e < K ? li[e] : kNoColumn;
    cvb[h] = e < c ? cb[e] : 0ull;
    cvi[h] = e < c ? ci[e] : kNoColumn;
  }
  for (int q = 0; q < c; ++q) {
    const score_bits64_t xb = cb[q];   // (one address for the whole wave: a broadcast read)
    const int32_t xi = ci[q];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      lr[h] += pair_before(xb, xi, lvb[h], lvi[h]);
      cr[h] += pair_before(xb, xi, cvb[h], cvi[h]);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (lane + 64 * h < c) {
      int lo = 0, hi = K;       // list entries before the candidate (descending, empty slots last)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pair_before(lb[mid], li[mid], cvb[h], cvi[h])) lo = mid + 1;
        else hi = mid;
      }
      cr[h] += lo;
    }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = lane + 64 * h;
    if (e < K && e + lr[h] < K) {
      lb[e + lr[h]] = lvb[h];
      li[e + lr[h]] = lvi[h];
    }
    if (e < c && cr[h] < K) {
      lb[cr[h]] = cvb[h];
      li[cr[h]] = cvi[h];
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// The panel lists of one query row: bits / cols [panels, nrows, K] (each list sorted, its real pairs a
// prefix) and count [panels, nrows], the candidates each panel scored in float64.
struct PanelPairLists {
  const score_bits64_t* bits;
  const int32_t* cols;
  const int32_t* count;
  int32_t panels, nrows, K;
  double* scores;      // [nrows, K]
  int32_t* index;      // [nrows, K]
  int32_t* resolved;   // [nrows]
};

// One wave merges the P panel lists of row li into one, decodes them and sums the panels' counts.
// lb / li_ / cb / ci: the wave's CMHSE_TOPK_MAX entries of LDS each.
__device__ __forceinline__ void merge_panel_pair_lists(const PanelPairLists& p, int li, score_bits64_t* lb, int32_t* li_,
                                                       score_bits64_t* cb, int32_t* ci, int lane) {
  const int K = p.K;
  for (int e = lane; e < K; e += 64) {
    lb[e] = 0ull;
    li_[e] = kNoColumn;
  }
  __builtin_amdgcn_wave_barrier();
  int total = 0;
  for (int q = 0; q < p.panels; ++q) {
    const int64_t row = static_cast<int64_t>(q) * p.nrows + li;
    total += p.count[row];
    const score_bits64_t tb = lb[K - 1];
    const int32_t ti = li_[K - 1];
    const score_bits64_t b0 = lane < K ? p.bits[row * K + lane] : 0ull;
    const score_bits64_t b1 = lane + 64 < K ? p.bits[row * K + lane + 64] : 0ull;
    const int32_t i0 = lane < K ? p.cols[row * K + lane] : kNoColumn;
    const int32_t i1 = lane + 64 < K ? p.cols[row * K + lane + 64] : kNoColumn;
    // (an empty slot is before nothing; the pairs before the list's last form a prefix of a sorted list)
    const bool c0 = pair_before(b0, i0, tb, ti), c1 = pair_before(b1, i1, tb, ti);
    const int c = __popcll(__ballot(c0)) + __popcll(__ballot(c1));
    if (c == 0) continue;
    if (c0) {
      cb[lane] = b0;
      ci[lane] = i0;
    }
    if (c1) {
      cb[lane + 64] = b1;
      ci[lane + 64] = i1;
    }
    __builtin_amdgcn_wave_barrier();
    wave_merge_pairs(lb, li_, K, cb, ci, c, lane);
  }
  for (int e = lane; e < K; e += 64) {
    p.scores[static_cast<int64_t>(li) * K + e] = bits64_score(lb[e]);
    p.index[static_cast<int64_t>(li) * K + e] = li_[e];
  }
  if (lane == 0) p.resolved[li] = total;
}

// The walk of the panel-major work list, as topk_select_kernel and cmhse_sim_topk (topk.hip) state it inline
// (a second copy of the rule: change both together; moving the fp32 kernel onto this helper is a follow-up): blocks b and b + 8 share
// an XCD (round-robin dispatch), each XCD takes a contiguous run of the list, so the row tiles of a panel
// stream its gallery tiles through one L2.  The grid is padded to a multiple of 8 (panel_grid_blocks).
struct PanelWork {
  int panel, row_tile;   // panel < 0: a padding block
  int t_begin, t_end;    // the panel's run of column tiles
};

__device__ __forceinline__ PanelWork panel_work(unsigned block, unsigned blocks, int row_tiles, int col_tiles,
                                                int panels) {
  const int run = static_cast<int>(blocks >> 3);
  const int w = static_cast<int>(block & 7) * run + static_cast<int>(block >> 3);
  if (w >= row_tiles * panels) return {-1, 0, 0, 0};
  const int panel = w / row_tiles;
  return {panel, w % row_tiles, static_cast<int>(static_cast<int64_t>(panel) * col_tiles / panels),
          static_cast<int>((static_cast<int64_t>(panel) + 1) * col_tiles / panels)};
}

inline int64_t panel_grid_blocks(int row_tiles, int panels) {
  return (static_cast<int64_t>(row_tiles) * panels + 7) / 8 * 8;
}

}  // namespace cmhse
