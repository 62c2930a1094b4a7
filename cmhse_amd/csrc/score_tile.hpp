// score_tile.hpp — what the scoring kernels around nt_phase share: sim.hip (sim_rank's top-1),
// topk.hip (top-K retrieval) and group.hip (group-wise ranking) define these decisions here, once.
//
//   the score key       64-bit (ordered bits of the score) << 32 | (0xFFFFFFFF - index): the tie rule
//                       of top-1, top-K and group top-1 — larger score first, then the smaller index.
//                       Unique per row, so a max / sort over keys depends on neither tiling nor
//                       scheduling.  The ordered bits of a non-NaN float are never 0, so key 0 lies
//                       below every real key (an empty slot, "no column").
//   the XCD-grouped deal   xcd_deal (host) / xcd_deal_tile (device): G row tiles x one column tile
//                       per group, group Q to XCD label Q % 8.
//   operand row setup   tile_row: an entry of the rowaddr_t / valid arrays nt_phase takes.
//   launch              launch_tiles: the VEC instance, opted into more than 64 KiB of dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "nt_core.hpp"

namespace cmhse {

typedef unsigned long long score_key_t;

// monotone map float -> uint32 (total order of non-NaN floats)
__device__ __forceinline__ unsigned ordered_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the key of a score given by its ordered bits (what a max reduction over ordered bits leaves)
__device__ __forceinline__ score_key_t bits_key(unsigned ob, int index) {
  return (static_cast<score_key_t>(ob) << 32) | static_cast<score_key_t>(0xFFFFFFFFu - static_cast<unsigned>(index));
}

__device__ __forceinline__ score_key_t score_key(float v, int index) { return bits_key(ordered_bits(v), index); }

__device__ __forceinline__ int32_t key_index(score_key_t key) {
  return static_cast<int32_t>(0xFFFFFFFFu - static_cast<unsigned>(key & 0xFFFFFFFFull));
}

// the score back from its bits, never recomputed
__device__ __forceinline__ float key_score(score_key_t key) {
  const unsigned ob = static_cast<unsigned>(key >> 32);
  return __uint_as_float((ob & 0x80000000u) ? (ob & 0x7FFFFFFFu) : ~ob);
}

// XCD-grouped deal of a row tiles x column tiles grid.  Blocks b, b + 8 share an XCD (round-robin
// dispatch), whose 4 MB L2 holds neither operand at the validation shapes (2 x 20 MB at N = 4917).
// The tiles are dealt in GROUPS — G consecutive row tiles x one column tile — group Q to XCD label
// Q % 8, its G workgroups back to back in that XCD's order: they run together and pull their column
// tile through the fabric once instead of G times, and the G row tiles of a group stay L2-resident
// while the group's column tiles stream by (931 -> 424 MB per launch at N = 4917, rocprofv3
// FETCH_SIZE).  G is the largest of 4, 3, 2 that keeps every XCD within the rounds of resident
// workgroups a perfectly even deal needs: a launch is two rounds at N = 4917, and one XCD with a
// handful of workgroups in a third round costs a third of the launch (sim_rank: 0.70 ms with a deal
// by row tile, 0.49 with G = 4, against 0.45 ms).
constexpr int kXcds = 8;
constexpr int kWgsPerXcd = 96;   // resident 128 x 128-tile workgroups per XCD: 3 per CU, 32 CUs

struct XcdDeal {
  int group;        // G, or 0: no G fits, plain row-major order over `blocks` = row x column tiles
  int64_t blocks;   // grid size, padded to whole groups on every XCD label
};

inline XcdDeal xcd_deal(int row_tiles, int col_tiles) {
  const int64_t tiles = static_cast<int64_t>(row_tiles) * col_tiles;
  const int64_t ideal_rounds = (tiles + kXcds * kWgsPerXcd - 1) / (kXcds * kWgsPerXcd);
  for (int g = 4; g >= 2; --g) {
    const int64_t groups = static_cast<int64_t>((row_tiles + g - 1) / g) * col_tiles;
    const int64_t per_label = (groups + kXcds - 1) / kXcds;   // groups per XCD label
    if ((per_label * g + kWgsPerXcd - 1) / kWgsPerXcd <= ideal_rounds) return {g, per_label * kXcds * g};
  }
  return {0, tiles};
}

// Block -> (row tile, column tile) under xcd_deal's G > 0.  The caller returns for a padding block,
// whose row tile lies past the last (the last group's missing rows, the grid's padding), testing it in
// its own units.  `block` stays unsigned, as blockIdx.x is: a signed block index costs the prologue
// a signed division.
struct TileIdx {
  int rt, ct;
};

__device__ __forceinline__ TileIdx xcd_deal_tile(unsigned block, int G, int col_tiles) {
  const int x = block & 7, q = block >> 3;
  const int Q = (q / G) * 8 + x;
  return {G * (Q / col_tiles) + (q % G), Q % col_tiles};
}

// One operand row of nt_phase: the address of row r of src (D floats a row, counted from row `base`)
// and *valid = r < limit; past the limit, row `base` (a valid address; nt_phase zeroes the row).
// Callers loop over their rows r = first + (threadIdx.x >> 2) + 64 i themselves: that loop unrolled
// inside a helper changes the register allocation of nt_phase's K loop.
__device__ __forceinline__ rowaddr_t tile_row(const float* src, int D, int base, int r, int limit, bool* valid) {
  *valid = r < limit;
  return row_addr(src + static_cast<int64_t>(base + (*valid ? r : 0)) * D);
}

// Launch the float4-loading instance `vec` when D % 4 == 0, else `plain`; past the 64 KiB of dynamic
// LDS a launch may ask for by default, opt the kernel in first (per device, host-side, no
// synchronisation).
template <typename P>
int launch_tiles(void (*vec)(P), void (*plain)(P), int D, dim3 grid, size_t smem, hipStream_t stream, const P& p) {
  void (*fn)(P) = (D % 4 == 0) ? vec : plain;
  if (smem > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(smem)) != hipSuccess)
    return CMHSE_ERR_LAUNCH;
  hipLaunchKernelGGL(fn, grid, dim3(kThreads), smem, stream, p);
  return CMHSE_OK;
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }   // workspace regions

}  // namespace cmhse
