// topk_lists.hpp — the sorted key lists of the top-K kernels: topk.hip (cmhse_sim_topk) and group.hip
// (cmhse_group_topk) keep, per query, a descending list of K score keys (score_tile.hpp) in LDS,
// grown by wave_merge, one list per gallery panel in the workspace, and merged across the panels by
// merge_panel_lists.
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

}  // namespace cmhse
