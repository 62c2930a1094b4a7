// sim.hip — N x M cosine-similarity contraction with fused ranking epilogues.
//
//   cmhse_sim_rank        evaluation.i2t / t2i  (/root/reference/evaluation.py:160-213):
//                         numpy.dot + per-row numpy.argsort become one exact-fp32 MFMA GEMM whose
//                         epilogue counts, per row, the columns that beat the diagonal and tracks
//                         the arg-max column — the N x M matrix never reaches HBM.  Its top-1 key,
//                         operand rows and XCD-grouped deal of the tiles are score_tile.hpp's, shared
//                         with topk.hip and group.hip.
//   cmhse_sim_rank_labelled  the same ranking against any set of positives per query, any gallery
//                         size: a threshold pass over the (query, positive) pairs in the place of the
//                         diagonal pass, then the same counting pass without the excluded column.
//   cmhse_sim_rank_exact  the ranking of the FLOAT64 scores of the same rows, as an interval [optimistic,
//                         pessimistic]: the counting pass decides every comparison that the fp32 scores
//                         provably decide and recomputes the others in float64 inside the tile.
//   cmhse_sim_rank_labelled_exact  the certified interval for any set of positives per query, any gallery
//                         size: a float64 threshold pass over the (query, positive) pairs, then the
//                         certified counting pass against the rounded threshold, no column excluded.
//   cmhse_cosine_sim      loss.cosine_sim       (/root/reference/loss.py:12-13): the stored-score GEMM,
//                         which the training losses of loss.hip launch through sim_store.hpp
//
// Bit-exactness of the ranks: every d[i][j] is produced by the same MFMA k-chain (nt_core.hpp:
// the k order per output element does not depend on the tile position), so the diagonal values
// written by the diagonal pass are bit-identical to what the counting pass recomputes, and
// `d[i][j] > d[i][i]` is evaluated on consistently rounded fp32 values, like the reference's
// comparison inside numpy.argsort.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "exact64.hpp"
#include "gru_ws.hpp"
#include "nt_core.hpp"
#include "score_tile.hpp"
#include "sim_store.hpp"

namespace cmhse {

constexpr int kSimBM = 128;
constexpr int kSimBN = 128;
constexpr int kSimSmallMax = 512;   // stored-score matrices up to this size use 64 x 64 tiles

// kSimLabel: the counting pass of cmhse_sim_rank_labelled — kSimRank's, except that p.diag holds a
// per-row threshold (the best positive's score) instead of the diagonal and no column is excluded.
// kSimExact: the counting pass of cmhse_sim_rank_exact — kSimRank's with a per-row tolerance: two compares
// per element, and the pairs neither decides go through dot64 (below) before the workgroup leaves.
// kSimLabelExact: the counting pass of cmhse_sim_rank_labelled_exact — kSimExact's, except that p.diag holds
// thr32(i) = float(thr64(i)) and p.s64_diag holds thr64(i), the float64 score of the query's best positive,
// and no column is excluded (kSimLabel's relation to kSimRank).
enum { kSimDiag = 0, kSimRank = 1, kSimStore = 2, kSimLabel = 3, kSimExact = 4, kSimLabelExact = 5 };

struct SimParams {
  const float* A;  // [N, D]
  const float* B;  // [M, D]
  int32_t N, M, D, row0, nrows, n_tiles;
  int32_t group;                // counting pass: row tiles per XCD group (xcd_deal), 0 = plain row-major order
  float* diag;                  // [nrows]
  int32_t* rank;                // [nrows]
  score_key_t* top1key;         // [nrows]
  float* scores;                // [nrows, M] (kSimStore)
  // batched square blocks (blockIdx.y = block): rows/cols [blk_off[b], blk_off[b+1]) of A and B,
  // scores of block b at scores + b * blk_stride, leading dimension = the block's size
  const int32_t* blk_off;
  int64_t blk_stride;
  // kSimExact / kSimLabelExact only (behind everything the other modes read)
  const float* tol;             // [nrows] the certified half-width of "undecided" around diag[i]
  const double* s64_diag;       // [nrows] dot64 of row i with its diagonal column (kSimLabelExact: thr64(i))
  int32_t* ties;                // [nrows] resolved pairs whose float64 score EQUALS the diagonal's (the threshold)
  int32_t* resolved;            // [nrows] pairs that went through dot64
};

// (dot64, THE float64 score of two fp32 rows, its error bound and the tolerance launch: exact64.hpp)
constexpr int kExactWords = kSimBM * kSimBN / 32;   // bitmap of a tile's undecided pairs: 2 KB of LDS

// TS = 32 x 32 blocks per wave in each direction: 2 = the 128 x 128 tile; 1 = a 64 x 64 tile for the
// small matrices of the training losses (n = 32 ... ~130: ONE 128 x 128 workgroup there is a
// 62 us MFMA chain per wave, four to nine 64 x 64 workgroups run it in a quarter of that).  Same k
// order per output: bit-identical.
#ifdef TILE_TRACE_BUILD
// Timing-only debug build (tools/tile_trace.py --sim): per-workgroup stamps of the counting pass —
// [0] first instruction, [1] K loop start, [3] K loop end, [4] epilogue done (s_memrealtime, 10 ns);
// [5] / [7] s_memtime at [1] / [3]; [6] HW_ID | XCC_ID << 32.
__device__ uint64_t* g_sim_trace = nullptr;
#define SIM_MARK(i)                                                                                     \
  do {                                                                                                  \
    if (MODE == kSimRank && threadIdx.x == 0 && g_sim_trace)                                            \
      g_sim_trace[static_cast<size_t>(blockIdx.x) * 8 + (i)] = wall_clock64();                          \
  } while (0)
#define SIM_CLOCK(i)                                                                                    \
  do {                                                                                                  \
    if (MODE == kSimRank && threadIdx.x == 0 && g_sim_trace)                                            \
      g_sim_trace[static_cast<size_t>(blockIdx.x) * 8 + (i)] = __builtin_amdgcn_s_memtime();            \
  } while (0)
#else
#define SIM_MARK(i) do {} while (0)
#define SIM_CLOCK(i) do {} while (0)
#endif

template <int MODE, bool VEC, int TS = 2>
__global__ __launch_bounds__(kThreads) void sim_kernel(const SimParams p_) {
  constexpr int BM = 64 * TS, BN = 64 * TS;
  SIM_MARK(0);
#ifdef TILE_TRACE_BUILD
  if (MODE == kSimRank && threadIdx.x == 0 && g_sim_trace) {
    g_sim_trace[static_cast<size_t>(blockIdx.x) * 8 + 6] =
        static_cast<uint64_t>(__builtin_amdgcn_s_getreg((31 << 11) | 4)) |
        (static_cast<uint64_t>(__builtin_amdgcn_s_getreg((31 << 11) | 20)) << 32);
  }
#endif
  constexpr bool EXACT = MODE == kSimExact || MODE == kSimLabelExact;                  // the certified ones
  constexpr bool COUNT = MODE == kSimRank || MODE == kSimLabel || EXACT;               // the counting passes
  static_assert(!EXACT || TS == 2, "the bitmap is laid out for the 128 x 128 tile");
  SimParams p = p_;
  if (p.blk_off != nullptr) {
    const int off = p.blk_off[blockIdx.y];
    const int n = p.blk_off[blockIdx.y + 1] - off;
    p.A += static_cast<int64_t>(off) * p.D;
    p.B += static_cast<int64_t>(off) * p.D;
    p.N = p.M = p.nrows = n;
    p.scores += static_cast<int64_t>(blockIdx.y) * p.blk_stride;
    const int jt = blockIdx.x % p.n_tiles, it = blockIdx.x / p.n_tiles;
    if (jt * BN >= n || it * BM >= n) return;  // tile outside this (smaller) block
  }
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = tid >> 2;
  int i0, j0;  // tile origin: local stripe row, global column
  if (MODE == kSimDiag) {
    i0 = blockIdx.x * BM;
    j0 = p.row0 + i0;  // the column block that holds this row block's diagonal
  } else if (COUNT && p.group > 0) {
    // counting pass: the XCD-grouped deal (score_tile.hpp)
    const TileIdx t = xcd_deal_tile(blockIdx.x, p.group, p.n_tiles);
    j0 = t.ct * BN;
    i0 = t.rt * BM;
    if (i0 >= p.nrows) return;     // padding: groups beyond the last row group, rows of a partial group
  } else {
    j0 = (blockIdx.x % p.n_tiles) * BN;
    i0 = (blockIdx.x / p.n_tiles) * BM;
  }
  rowaddr_t ar[BM / 64];
  rowaddr_t br[BN / 64];
  bool av[BM / 64], bv[BN / 64];
#pragma unroll
  for (int i = 0; i < BM / 64; ++i) ar[i] = tile_row(p.A, p.D, p.row0, i0 + srow + 64 * i, p.nrows, &av[i]);
#pragma unroll
  for (int i = 0; i < BN / 64; ++i) br[i] = tile_row(p.B, p.D, 0, j0 + srow + 64 * i, p.M, &bv[i]);
  f32x16 acc[TS][TS];
#pragma unroll
  for (int ms = 0; ms < TS; ++ms)
#pragma unroll
    for (int ns = 0; ns < TS; ++ns) acc[ms][ns] = zero16();
  int b_row0[TS];
#pragma unroll
  for (int ns = 0; ns < TS; ++ns) b_row0[ns] = wn * 32 * TS + 32 * ns;
  // counting pass: the diagonal scores of the tile's rows, ONE coalesced request in front of the K
  // loop (the epilogue used to load diag[row] inside its 32-iteration loop: 32 dependent global
  // round trips per lane, ~50 of the 62 us the epilogue took — profiles/r04_sim_kernel_trace.txt);
  // they go through LDS once the tile buffers are free
  float my_diag = 0.f;
  if (COUNT && tid < BM) my_diag = (i0 + tid < p.nrows) ? p.diag[i0 + tid] : 0.f;
  float my_tol = 0.f;
  if (EXACT && tid < BM) my_tol = (i0 + tid < p.nrows) ? p.tol[i0 + tid] : 0.f;
  SIM_MARK(1);
  SIM_CLOCK(5);
  nt_phase<BM, BN, TS, TS, TS, TS - 1, VEC>(smem, ar, av, br, bv, p.D, wm * 32 * TS, b_row0, acc);
  SIM_MARK(3);
  SIM_CLOCK(7);
  if (COUNT) {
    // (what is left of the epilogue is ~12 us of vector / scalar work on its own and 48 beside two
    // workgroups inside their MFMA loops on the same SIMDs; raising its wave priority changes
    // nothing: 404 / 407 us per launch)
    __syncthreads();                 // every wave has read its last fragments
    if (tid < BM) smem[tid] = my_diag;
    if (EXACT) {
      if (tid < BM) smem[BM + tid] = my_tol;
      if (tid == 0) smem[2 * BM + kExactWords] = 0.f;    // "some pair of this tile is undecided"
    }
    __syncthreads();
  }
  // kSimExact / kSimLabelExact, behind the diagonals and tolerances: word 4 row + c holds the undecided pairs of
  // tile row `row` and tile columns [32 c, 32 c + 32), bit = column; every word is written below, by one half-wave
  unsigned* const s_amb = reinterpret_cast<unsigned*>(smem + 2 * BM);

#pragma unroll
  for (int ms = 0; ms < TS; ++ms) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int li = i0 + wm * 32 * TS + ms * 32 + acc_row(r, lane);  // local stripe row
      const int gi = p.row0 + li;                                  // its diagonal column
      const bool rok = li < p.nrows;
      if (MODE == kSimDiag) {
#pragma unroll
        for (int ns = 0; ns < TS; ++ns) {
          const int j = j0 + b_row0[ns] + acc_col(lane);
          if (rok && j == gi) p.diag[li] = acc[ms][ns][r];
        }
      } else if (MODE == kSimStore) {
#pragma unroll
        for (int ns = 0; ns < TS; ++ns) {
          const int j = j0 + b_row0[ns] + acc_col(lane);
          if (rok && j < p.M) p.scores[static_cast<int64_t>(li) * p.M + j] = acc[ms][ns][r];
        }
      } else {
        // The 32 lanes of a half-wave hold the 32 columns of ONE row (lanes 0-31: row acc_row(r, 0),
        // lanes 32-63: the row four below), so the row's count is a population count of the compare
        // mask (v_cmp writes the mask; scalar s_bcnt1) and its arg-max one 32-bit max reduction plus
        // an equality mask whose lowest set lane is the smallest column among the maxima — instead
        // of five shuffle steps on (count, 64-bit key) per element: the epilogue was 27 % of a
        // tile's time, VALU work beside the other workgroups' MFMA loops
        // (profiles/r04_sim_kernel_trace.txt).  Same count, same key (ordered bits of the score,
        // then the smaller column), same atomics.
        const float dii = smem[li - i0];          // (0 for rows past the stripe: never counted)
        const float tol = EXACT ? smem[BM + li - i0] : 0.f;
        const bool hi = lane >= 32;
        int cnt = 0;
        unsigned ob[TS];
        unsigned obmax = 0u;
#pragma unroll
        for (int ns = 0; ns < TS; ++ns) {
          const int j = j0 + b_row0[ns] + acc_col(lane);
          const float v = acc[ms][ns][r];
          const bool valid = rok && j < p.M;
          unsigned long long gt;
          if (EXACT) {
            // surely above: fl(v - dii) > tol; surely below: fl(dii - v) = -fl(v - dii) > tol; else undecided
            // (tol >= 0, possibly +inf: everything undecided; inputs finite, so the difference is no NaN)
            const float diff = v - dii;
            const bool mine = valid && (MODE == kSimLabelExact || j != gi);
            gt = __ballot(mine && diff > tol);
            const unsigned long long amb = __ballot(mine && fabsf(diff) <= tol);
            if ((lane & 31) == 0) {
              const unsigned w = hi ? static_cast<unsigned>(amb >> 32) : static_cast<unsigned>(amb);
              s_amb[(li - i0) * 4 + (b_row0[ns] >> 5)] = w;
              if (w != 0u) smem[2 * BM + kExactWords] = 1.f;
            }
          } else {
            gt = __ballot(valid && (MODE == kSimLabel || j != gi) && v > dii);
          }
          cnt += __popc(hi ? static_cast<unsigned>(gt >> 32) : static_cast<unsigned>(gt));
          ob[ns] = valid ? ordered_bits(v) : 0u;
          obmax = ob[ns] > obmax ? ob[ns] : obmax;
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {      // (xor masks < 32 stay inside a half-wave)
          const unsigned o = __shfl_xor(obmax, d, 64);
          obmax = o > obmax ? o : obmax;
        }
        int jbest = -1;
#pragma unroll
        for (int ns = 0; ns < TS; ++ns) {        // ns = 0 holds the smaller columns
          const unsigned long long eq = __ballot(obmax != 0u && ob[ns] == obmax);
          const unsigned m = hi ? static_cast<unsigned>(eq >> 32) : static_cast<unsigned>(eq);
          if (jbest < 0 && m != 0u) jbest = j0 + b_row0[ns] + (__ffs(m) - 1);
        }
        if (rok && (lane & 31) == 0) {
          if (cnt) atomicAdd(&p.rank[li], cnt);
          if (jbest >= 0) atomicMax(&p.top1key[li], bits_key(obmax, jbest));
        }
      }
    }
  }
  if (EXACT) {
    // The resolve step.  The barrier and the test are workgroup-uniform (every thread of a workgroup that
    // gets here reads the same LDS word), the loops are bounded by the 512 bitmap words and their 32 bits,
    // and nothing waits on another workgroup.  Wave w takes the words w, w + 4, ...: the 32 columns of one
    // tile row each; every set bit is one dot64 of that row with the bit's column, compared with the row's
    // dot64 diagonal (kSimLabelExact: its float64 threshold).  Integer atomics: the sums do not depend on who adds first.
    __syncthreads();
    if (smem[2 * BM + kExactWords] != 0.f) {
      for (int w = wave; w < kExactWords; w += kThreads / 64) {
        unsigned bits = __builtin_amdgcn_readfirstlane(s_amb[w]);
        if (bits == 0u) continue;
        const int li = i0 + (w >> 2);              // (< nrows: rows past the stripe set no bit)
        const int jw = j0 + (w & 3) * 32;
        const float* arow = p.A + static_cast<int64_t>(p.row0 + li) * p.D;
        const double sii = p.s64_diag[li];
        int above = 0, equal = 0, n = 0;
        while (bits != 0u) {
          const int c = __ffs(bits) - 1;           // (column jw + c < M: columns past the gallery set no bit)
          bits &= bits - 1u;
          const double s = dot64(arow, p.B + static_cast<int64_t>(jw + c) * p.D, p.D, lane);
          above += s > sii;
          equal += s == sii;
          ++n;
        }
        if (lane == 0) {
          if (above) atomicAdd(&p.rank[li], above);
          if (equal) atomicAdd(&p.ties[li], equal);
          atomicAdd(&p.resolved[li], n);
        }
      }
    }
  }
#ifdef TILE_TRACE_BUILD
  __builtin_amdgcn_s_waitcnt(0);
  SIM_MARK(4);
#endif
}

__global__ void top1_finalize_kernel(const score_key_t* key, int32_t* top1, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) top1[i] = key_index(key[i]);
}

// ---------------------------------------------------------------------------------------------
// cmhse_sim_rank_labelled: the threshold pass (in the place of sim_kernel<kSimDiag>) and the decoding
// of its keys.  The (query, positive) pairs of the stripe's CSR, in CSR order, are cut into tiles of
// 128: operand A row r of a tile is the query of pair r, operand B row c the gallery row of pair c,
// and the wanted scores are the tile's diagonal — out of nt_phase like every score of the counting
// pass, so bit-identical to what that pass compares them with.  Each goes into its query's 64-bit
// key by atomicMax (larger score, then smaller gallery index: independent of tiling and scheduling).
// ---------------------------------------------------------------------------------------------
struct PairParams {
  const float* A;            // [N, D]
  const float* B;            // [M, D]
  int32_t M, D, row0, nrows, n_pairs;
  const int32_t* pos_off;    // [nrows + 1] device copy
  const int32_t* pos_idx;    // [n_pairs]   device copy
  score_key_t* thrkey;       // [nrows], zeroed
};

constexpr size_t kPairSmem = TileSmem<kSimBM, kSimBN>::kBytes + 2 * kSimBM * sizeof(int32_t);

template <bool VEC>
__global__ __launch_bounds__(kThreads) void pair_threshold_kernel(const PairParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // behind nt_phase's tile buffers: the query (local stripe row; -1 past the last pair) and the
  // gallery row of each pair of the tile, for the lanes that end up holding the diagonal
  int32_t* s_query = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(smem) + TileSmem<kSimBM, kSimBN>::kBytes);
  int32_t* s_pos = s_query + kSimBM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int srow = tid >> 2;
  const int g0 = blockIdx.x * kSimBM;   // the tile's first pair
  rowaddr_t ar[kSimBM / 64], br[kSimBN / 64];
  bool av[kSimBM / 64], bv[kSimBN / 64];
#pragma unroll
  for (int i = 0; i < kSimBM / 64; ++i) {
    const int g = g0 + srow + 64 * i;
    const bool ok = g < p.n_pairs;
    int q = 0, c = 0;
    if (ok) {
      // The query of pair g: the last q with pos_off[q] <= g.  Every list holds a positive, so
      // pos_off[q] - q never decreases and ends at n_pairs - nrows: q lies in [g - (n_pairs - nrows), g]
      // (one positive per query: no search at all).  Every index read lies in [0, nrows), whatever
      // the arrays hold.
      int lo = g - (p.n_pairs - p.nrows), hi = (g < p.nrows - 1) ? g : p.nrows - 1;
      lo = lo < 0 ? 0 : lo;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.pos_off[mid] <= g) lo = mid; else hi = mid - 1;
      }
      q = lo;
      // (validated on the host copy; the clamp keeps a device copy that differs from it inside B)
      c = p.pos_idx[g];
      c = c < 0 ? 0 : (c < p.M ? c : p.M - 1);
    }
    ar[i] = row_addr(p.A + static_cast<int64_t>(p.row0 + q) * p.D);
    br[i] = row_addr(p.B + static_cast<int64_t>(c) * p.D);
    av[i] = bv[i] = ok;
    if ((tid & 3) == 0) {
      s_query[srow + 64 * i] = ok ? q : -1;
      s_pos[srow + 64 * i] = c;
    }
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int ms = 0; ms < 2; ++ms)
#pragma unroll
    for (int ns = 0; ns < 2; ++ns) acc[ms][ns] = zero16();
  const int b_row0[2] = {wn * 64, wn * 64 + 32};
  // (its barriers also order the s_query / s_pos writes above before the reads below)
  nt_phase<kSimBM, kSimBN, 2, 2, 2, 1, VEC>(smem, ar, av, br, bv, p.D, wm * 64, b_row0, acc);
  if (wm != wn) return;   // (wave-uniform) no diagonal in this wave's 64 x 64
#pragma unroll
  for (int ms = 0; ms < 2; ++ms) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (acc_row(r, lane) != acc_col(lane)) continue;
      const int lr = wm * 64 + ms * 32 + acc_row(r, lane);   // pair g0 + lr: row and column of the tile
      const int q = s_query[lr];
      if (q >= 0) atomicMax(&p.thrkey[q], score_key(acc[ms][ms][r], s_pos[lr]));
    }
  }
}

__global__ void label_decode_kernel(const score_key_t* key, float* thr, int32_t* best_pos, float* best_score, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const score_key_t k = key[i];
  thr[i] = key_score(k);
  best_pos[i] = key_index(k);
  if (best_score) best_score[i] = key_score(k);
}

// ---------------------------------------------------------------------------------------------
// cmhse_sim_rank_exact: the pre-pass and the last pass around sim_kernel<kSimExact>.  The bound E_i on
// |v(i,j) - s64(i,j)|, the tolerance 2 E_i (1 + 2^-18) and exact_tol_kernel are exact64.hpp's, shared with
// cmhse_sim_topk_exact (topk.hip).
// ---------------------------------------------------------------------------------------------
struct ExactPreParams {
  const float* A;            // [N, D]
  const float* B;            // [M, D]
  int32_t M, D, row0, nrows;
  double* s64_diag;          // [nrows]
  double* norm_a;            // [nrows]
  unsigned* norm_b_max;      // the bits of the largest |b_j| (rounded up), zeroed; bits of floats >= 0 order as integers
  int32_t* rank_lo;          // [nrows] the call's counters, zeroed here
  int32_t* ties;
  int32_t* resolved;
  score_key_t* top1key;
};

// One wave per row: the nrows stripe rows first (diagonal score, norm, zeroed counters), then the M
// gallery rows (norm into the maximum).
__global__ __launch_bounds__(kThreads) void exact_pre_kernel(const ExactPreParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (r < p.nrows) {
    const float* a = p.A + (static_cast<int64_t>(p.row0) + r) * p.D;
    const float* b = p.B + (static_cast<int64_t>(p.row0) + r) * p.D;
    const double sii = dot64(a, b, p.D, lane);
    const double na = sqrt(dot64(a, a, p.D, lane));
    if (lane == 0) {
      p.s64_diag[r] = sii;
      p.norm_a[r] = na;
      p.rank_lo[r] = 0;
      p.ties[r] = 0;
      p.resolved[r] = 0;
      p.top1key[r] = 0ull;
    }
  } else if (r < static_cast<int64_t>(p.nrows) + p.M) {
    const float* b = p.B + (r - p.nrows) * p.D;
    const double nb = sqrt(dot64(b, b, p.D, lane));
    if (lane == 0) atomicMax(p.norm_b_max, __float_as_uint(round_up_f32(nb)));
  }
}

// rank_hi arrives holding the ties of the resolved pairs
__global__ void exact_finalize_kernel(const score_key_t* key, const int32_t* rank_lo, int32_t* rank_hi,
                                      int32_t* top1, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  top1[i] = key_index(key[i]);
  rank_hi[i] += rank_lo[i];
}

// ---------------------------------------------------------------------------------------------
// cmhse_sim_rank_labelled_exact: the launches around sim_kernel<kSimLabelExact>.
//
// thr64(i) = max over p in P_i of s64(i,p) is itself a float64 score (the best positive under fp32 is not always
// the best positive under float64, so the fp32 threshold pass cannot serve), and the counting pass compares the
// fp32 MFMA scores v(i,j) with its rounding thr32(i) = float(thr64(i)).  Why tol_i = 2 E_i (1 + 2^-18)
// (exact64.hpp) stays valid unchanged:
//   |v(i,j) - s64(i,j)| <= E_i                                               as for cmhse_sim_rank_exact;
//   |thr32 - thr64| <= u |thr64| <= u (1 + (D / 64 + 8) 2^-53) |a_i| max_j |b_j|   round to nearest, normal range
//                   <= gamma_D(u) |a_i| max_j |b_j| <= E_i      gamma_D >= gamma_1 = u / (1 - u) = u (1 + 2^-24 + ...),
//                                                               which covers the factor 1 + (D / 64 + 8) 2^-53 for
//                                                               D < 2^24;
//   where thr64 falls into the fp32 subnormal range the rounding is off by at most 2^-150 instead, and
//   u |thr64| + 2^-150 <= gamma_D(u) |a_i| max_j |b_j| + D 2^-149 <= E_i covers both cases at once.
// So |(v - thr32) - (s64(i,j) - thr64)| <= 2 E_i, the fp32 subtraction adds a factor 1 + d, |d| <= u, exactly as
// in the diagonal call (where the second term is |v(i,i) - s64(i,i)| <= E_i), and fl(v - thr32) > tol_i proves
// s64(i,j) > thr64(i); the reverse likewise.  No gap found: the tolerance is not widened.  thr32 is finite
// whenever the fp32 scores are (|thr64| <= |a_i| max |b_j| (1 + tiny)); inputs whose fp32 scores overflow are
// outside the contract here as in the diagonal call.
// A column whose s64 EQUALS thr64 is never decided by the two compares (either would prove a strict
// inequality), so every tie — the best positive's own column, other positives at the threshold, tied negatives
// — reaches the resolve step and is counted in `ties`; the threshold pass counts the list entries at the
// threshold (lists are strictly ascending: distinct columns), and rank_hi = rank_lo + ties - that count.
// ---------------------------------------------------------------------------------------------
struct LabelExactPreParams {
  const float* A;            // [N, D]
  const float* B;            // [M, D]
  int32_t M, D, row0, nrows;
  double* norm_a;            // [nrows]
  unsigned* norm_b_max;      // as ExactPreParams'
  int32_t* rank_lo;          // [nrows] the call's counters, zeroed here
  int32_t* ties;
  int32_t* resolved;
  score_key_t* top1key;
};

// exact_pre_kernel without the diagonal (there is none: M may be smaller than N)
__global__ __launch_bounds__(kThreads) void label_exact_pre_kernel(const LabelExactPreParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (r < p.nrows) {
    const float* a = p.A + (static_cast<int64_t>(p.row0) + r) * p.D;
    const double na = sqrt(dot64(a, a, p.D, lane));
    if (lane == 0) {
      p.norm_a[r] = na;
      p.rank_lo[r] = 0;
      p.ties[r] = 0;
      p.resolved[r] = 0;
      p.top1key[r] = 0ull;
    }
  } else if (r < static_cast<int64_t>(p.nrows) + p.M) {
    const float* b = p.B + (r - p.nrows) * p.D;
    const double nb = sqrt(dot64(b, b, p.D, lane));
    if (lane == 0) atomicMax(p.norm_b_max, __float_as_uint(round_up_f32(nb)));
  }
}

struct PairExactParams {
  const float* A;            // [N, D]
  const float* B;            // [M, D]
  int32_t M, D, row0, nrows, n_pairs;
  const int32_t* pos_off;    // [nrows + 1] device copy
  const int32_t* pos_idx;    // [n_pairs]   device copy
  double* pair64;            // [n_pairs] s64 of every pair, CSR order
  double* thr64;             // [nrows]
  float* thr32;              // [nrows] float(thr64): what the counting pass compares with
  int32_t* at_thr;           // [nrows] list entries whose s64 equals thr64
  int32_t* best_pos;         // [nrows]
  double* best_score;        // [nrows] or null
};

// The float64 threshold pass, first half: one wave per pair of the CSR, pair64[g] = s64(query of g, pos_idx[g]).
// The query of a pair and the clamp of its column are pair_threshold_kernel's (wave-uniform here).
__global__ __launch_bounds__(kThreads) void pair_exact_kernel(const PairExactParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t g64 = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (g64 >= p.n_pairs) return;
  const int g = static_cast<int>(g64);
  // the last q with pos_off[q] <= g, inside [g - (n_pairs - nrows), min(g, nrows - 1)]: every index read lies
  // in [0, nrows), whatever the arrays hold
  int lo = g - (p.n_pairs - p.nrows), hi = (g < p.nrows - 1) ? g : p.nrows - 1;
  lo = lo < 0 ? 0 : lo;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.pos_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  int c = p.pos_idx[g];
  c = c < 0 ? 0 : (c < p.M ? c : p.M - 1);   // (validated on the host copy; keeps a differing device copy inside B)
  const double s = dot64(p.A + static_cast<int64_t>(p.row0 + lo) * p.D, p.B + static_cast<int64_t>(c) * p.D, p.D, lane);
  if (lane == 0) p.pair64[g] = s;
}

// Second half: one wave per query reduces its list to (thr64, the smallest column at thr64, the entries at
// thr64).  Lane l folds the entries l, l + 64, ... of the list, the 64 partial results are combined in a
// butterfly; (max, then min of the column, then sum of the counts) is associative and commutative in exact
// arithmetic — no rounding anywhere — so the result does not depend on the order, and nothing here is atomic.
__global__ __launch_bounds__(kThreads) void label_exact_reduce_kernel(const PairExactParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t q64 = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (q64 >= p.nrows) return;
  const int q = static_cast<int>(q64);
  // (validated on the host copy; the clamps keep a differing device copy inside pair64 and pos_idx)
  int beg = p.pos_off[q], end = p.pos_off[q + 1];
  beg = beg < 0 ? 0 : (beg < p.n_pairs ? beg : p.n_pairs);
  end = end < beg ? beg : (end < p.n_pairs ? end : p.n_pairs);
  double best = -INFINITY;      // (every s64 is finite: products of fp32 values, D < 2^24 of them)
  int col = 0x7fffffff, cnt = 0;
  for (int e = beg + lane; e < end; e += 64) {
    const double s = p.pair64[e];
    int c = p.pos_idx[e];
    c = c < 0 ? 0 : (c < p.M ? c : p.M - 1);
    if (s > best) best = s, col = c, cnt = 1;
    else if (s == best) col = c < col ? c : col, ++cnt;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ob = __shfl_xor(best, d, 64);
    const int oc = __shfl_xor(col, d, 64), on = __shfl_xor(cnt, d, 64);
    if (ob > best) best = ob, col = oc, cnt = on;
    else if (ob == best) col = oc < col ? oc : col, cnt += on;
  }
  if (lane == 0) {
    if (cnt == 0) best = 0.0, col = 0;    // (an empty list: only a device copy that differs from the host's)
    p.thr64[q] = best;
    p.thr32[q] = static_cast<float>(best);
    p.at_thr[q] = cnt;
    p.best_pos[q] = col;
    if (p.best_score) p.best_score[q] = best;
  }
}

// rank_hi arrives holding the ties of the resolved pairs, the list entries at the threshold among them
__global__ void label_exact_finalize_kernel(const score_key_t* key, const int32_t* rank_lo, int32_t* rank_hi,
                                            const int32_t* at_thr, int32_t* top1, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  top1[i] = key_index(key[i]);
  rank_hi[i] += rank_lo[i] - at_thr[i];
}

// The stored-score GEMM (sim_store.hpp): the one place that chooses its tile size.
int launch_sim_store(const float* A, const float* B, int n, int m, int D, float* scores,
                     hipStream_t stream, const int32_t* blk_off, int n_blocks, int64_t blk_stride) {
  SimParams p;
  p.A = A;
  p.B = B;
  p.N = n;
  p.M = m;
  p.D = D;
  p.row0 = 0;
  p.nrows = n;
  const bool small = n <= kSimSmallMax && m <= kSimSmallMax;   // training-loss sizes: 64 x 64 tiles
  const int bt = small ? 64 : kSimBN;
  p.n_tiles = (m + bt - 1) / bt;
  p.group = 0;
  p.diag = nullptr;
  p.rank = nullptr;
  p.top1key = nullptr;
  p.scores = scores;
  p.blk_off = blk_off;
  p.blk_stride = blk_stride;
  const int64_t blocks = static_cast<int64_t>(p.n_tiles) * ((n + bt - 1) / bt);
  if (blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  const size_t smem = small ? TileSmem<64, 64>::kBytes : TileSmem<kSimBM, kSimBN>::kBytes;
  const dim3 grid(static_cast<unsigned>(blocks), n_blocks);
  if (small)
    return launch_tiles(sim_kernel<kSimStore, true, 1>, sim_kernel<kSimStore, false, 1>, D, grid, smem, stream, p);
  return launch_tiles(sim_kernel<kSimStore, true>, sim_kernel<kSimStore, false>, D, grid, smem, stream, p);
}

}  // namespace cmhse

using namespace cmhse;

extern "C" size_t cmhse_sim_rank_workspace(int32_t nrows) {
  if (nrows <= 0) return 0;
  return align256(static_cast<size_t>(nrows) * sizeof(float)) +
         align256(static_cast<size_t>(nrows) * sizeof(score_key_t));
}

extern "C" int cmhse_sim_rank_ex(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                                 int32_t row0, int32_t nrows, int32_t* rank, int32_t* top1,
                                 void* workspace, size_t workspace_bytes, void* stream_,
                                 void* timer_) {
  if (!A || !B || !rank || !top1 || !workspace) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0 || row0 < 0 || nrows < 0 || row0 + nrows > N) return CMHSE_ERR_ARG;
  if (row0 + nrows > M) return CMHSE_ERR_ARG;  // diagonal d[i][i] must exist
  if (nrows == 0) return CMHSE_OK;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_rank_workspace(nrows))
    return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SimParams p;
  p.A = A;
  p.B = B;
  p.N = N;
  p.M = M;
  p.D = D;
  p.row0 = row0;
  p.nrows = nrows;
  p.n_tiles = (M + kSimBN - 1) / kSimBN;
  p.diag = static_cast<float*>(workspace);
  p.top1key = reinterpret_cast<score_key_t*>(
      static_cast<char*>(workspace) + align256(static_cast<size_t>(nrows) * sizeof(float)));
  p.rank = rank;
  p.scores = nullptr;
  p.blk_off = nullptr;
  p.blk_stride = 0;
  const int m_tiles = (nrows + kSimBM - 1) / kSimBM;
  const XcdDeal deal = xcd_deal(m_tiles, p.n_tiles);
  p.group = deal.group;
  if (deal.blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  if (hipMemsetAsync(rank, 0, sizeof(int32_t) * nrows, stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  if (hipMemsetAsync(p.top1key, 0, sizeof(score_key_t) * nrows, stream) != hipSuccess)
    return CMHSE_ERR_LAUNCH;
  const size_t smem = TileSmem<kSimBM, kSimBN>::kBytes;
  Timer* timer = static_cast<Timer*>(timer_);   // brackets the counting pass alone
  int rc = launch_tiles(sim_kernel<kSimDiag, true>, sim_kernel<kSimDiag, false>, D, dim3(m_tiles), smem, stream, p);
  if (rc != CMHSE_OK) return rc;
  if (timer) (void)hipEventRecord(timer->start, stream);
  rc = launch_tiles(sim_kernel<kSimRank, true>, sim_kernel<kSimRank, false>, D,
                    dim3(static_cast<unsigned>(deal.blocks)), smem, stream, p);
  if (rc != CMHSE_OK) return rc;
  if (timer) {
    (void)hipEventRecord(timer->stop, stream);
    timer->launches = 1;
  }
  hipLaunchKernelGGL(top1_finalize_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream,
                     p.top1key, top1, nrows);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int cmhse_sim_rank(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                              int32_t row0, int32_t nrows, int32_t* rank, int32_t* top1,
                              void* workspace, size_t workspace_bytes, void* stream_) {
  return cmhse_sim_rank_ex(A, B, N, M, D, row0, nrows, rank, top1, workspace, workspace_bytes,
                           stream_, nullptr);
}

namespace {
struct ExactWs {
  size_t diag, top1key, s64_diag, norm_a, tol, norm_b_max, total;
};
ExactWs exact_ws(int32_t nrows) {
  const size_t n = static_cast<size_t>(nrows);
  ExactWs L;
  size_t off = 0;
  L.diag = off, off += align256(n * sizeof(float));
  L.top1key = off, off += align256(n * sizeof(score_key_t));
  L.s64_diag = off, off += align256(n * sizeof(double));
  L.norm_a = off, off += align256(n * sizeof(double));
  L.tol = off, off += align256(n * sizeof(float));
  L.norm_b_max = off, off += 256;
  L.total = off;
  return L;
}

// The SimParams and the tile deal of a certified counting pass (kSimExact, kSimLabelExact): one setup for the
// two calls.  thr32 / thr64 are the fp32 and float64 values every row is compared with (the diagonal score
// or the best positive's); rank_hi collects the ties until the call's last launch.
int exact_count_params(SimParams* p_, int64_t* blocks, const float* A, const float* B, int32_t N, int32_t M,
                       int32_t D, int32_t row0, int32_t nrows, float* thr32, const double* thr64,
                       score_key_t* top1key, const float* tol, int32_t* rank_lo, int32_t* rank_hi,
                       int32_t* resolved) {
  SimParams& p = *p_;
  p.A = A;
  p.B = B;
  p.N = N;
  p.M = M;
  p.D = D;
  p.row0 = row0;
  p.nrows = nrows;
  p.n_tiles = (M + kSimBN - 1) / kSimBN;
  p.diag = thr32;
  p.top1key = top1key;
  p.rank = rank_lo;
  p.scores = nullptr;
  p.blk_off = nullptr;
  p.blk_stride = 0;
  p.tol = tol;
  p.s64_diag = thr64;
  p.ties = rank_hi;
  p.resolved = resolved;
  const int m_tiles = (nrows + kSimBM - 1) / kSimBM;
  const XcdDeal deal = xcd_deal(m_tiles, p.n_tiles);
  p.group = deal.group;
  *blocks = deal.blocks;
  return deal.blocks > 0x7fffffffLL ? CMHSE_ERR_UNSUPPORTED : CMHSE_OK;
}
}  // namespace

extern "C" size_t cmhse_sim_rank_exact_workspace(int32_t nrows) {
  if (nrows <= 0) return 0;
  return exact_ws(nrows).total;
}

extern "C" double cmhse_sim_rank_exact_tolerance(int32_t D, double norm_a, double norm_b_max) {
  if (D <= 0 || !(norm_a >= 0.0) || !(norm_b_max >= 0.0)) return NAN;
  return exact_tolerance(D, norm_a, norm_b_max);
}

extern "C" int cmhse_sim_rank_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                                    int32_t row0, int32_t nrows, int32_t* rank_lo, int32_t* rank_hi,
                                    int32_t* top1, int32_t* resolved, void* workspace,
                                    size_t workspace_bytes, void* stream_) {
  if (!A || !B || !rank_lo || !rank_hi || !top1 || !resolved || !workspace) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0 || row0 < 0 || nrows < 0 || static_cast<int64_t>(row0) + nrows > N)
    return CMHSE_ERR_ARG;
  if (static_cast<int64_t>(row0) + nrows > M) return CMHSE_ERR_ARG;  // diagonal d[i][i] must exist
  if (nrows == 0) return CMHSE_OK;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_rank_exact_workspace(nrows))
    return CMHSE_ERR_WORKSPACE;
  if (D >= (1 << 24)) return CMHSE_ERR_UNSUPPORTED;   // (the bound needs D u < 1)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const ExactWs L = exact_ws(nrows);
  char* const ws = static_cast<char*>(workspace);
  SimParams p;
  int64_t blocks;
  int rc = exact_count_params(&p, &blocks, A, B, N, M, D, row0, nrows, reinterpret_cast<float*>(ws + L.diag),
                              reinterpret_cast<double*>(ws + L.s64_diag),
                              reinterpret_cast<score_key_t*>(ws + L.top1key),
                              reinterpret_cast<float*>(ws + L.tol), rank_lo, rank_hi, resolved);
  if (rc != CMHSE_OK) return rc;
  const int m_tiles = (nrows + kSimBM - 1) / kSimBM;
  ExactPreParams q;
  q.A = A;
  q.B = B;
  q.M = M;
  q.D = D;
  q.row0 = row0;
  q.nrows = nrows;
  q.s64_diag = reinterpret_cast<double*>(ws + L.s64_diag);
  q.norm_a = reinterpret_cast<double*>(ws + L.norm_a);
  q.norm_b_max = reinterpret_cast<unsigned*>(ws + L.norm_b_max);
  q.rank_lo = rank_lo;
  q.ties = rank_hi;
  q.resolved = resolved;
  q.top1key = p.top1key;
  const int32_t scale = tunables().rank_exact_tol_scale.load(std::memory_order_relaxed);
  if (hipMemsetAsync(q.norm_b_max, 0, sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  const int64_t pre_rows = static_cast<int64_t>(nrows) + M;
  hipLaunchKernelGGL(exact_pre_kernel, dim3(static_cast<unsigned>((pre_rows + kThreads / 64 - 1) / (kThreads / 64))),
                     dim3(kThreads), 0, stream, q);
  hipLaunchKernelGGL(exact_tol_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, q.norm_a,
                     q.norm_b_max, reinterpret_cast<float*>(ws + L.tol), D, scale, nrows);
  const size_t smem = TileSmem<kSimBM, kSimBN>::kBytes;
  rc = launch_tiles(sim_kernel<kSimDiag, true>, sim_kernel<kSimDiag, false>, D, dim3(m_tiles), smem, stream, p);
  if (rc != CMHSE_OK) return rc;
  rc = launch_tiles(sim_kernel<kSimExact, true>, sim_kernel<kSimExact, false>, D,
                    dim3(static_cast<unsigned>(blocks)), smem, stream, p);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(exact_finalize_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, p.top1key,
                     rank_lo, rank_hi, top1, nrows);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" size_t cmhse_sim_rank_labelled_workspace(int32_t nrows, int32_t n_pairs) {
  if (nrows <= 0 || n_pairs < nrows) return 0;   // (n_pairs: every query has a positive)
  return align256(static_cast<size_t>(nrows) * sizeof(float)) +
         align256(2 * static_cast<size_t>(nrows) * sizeof(score_key_t));
}

extern "C" int cmhse_sim_rank_labelled(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                                       int32_t row0, int32_t nrows, const int32_t* pos_off_host,
                                       const int32_t* pos_idx_host, const int32_t* pos_off,
                                       const int32_t* pos_idx, int32_t n_pairs, int32_t* rank,
                                       int32_t* top1, int32_t* best_pos, float* best_score,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
  if (!A || !B) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (row0 < 0 || nrows < 0 || static_cast<int64_t>(row0) + nrows > N) return CMHSE_ERR_ARG;
  if (nrows == 0) return n_pairs == 0 ? CMHSE_OK : CMHSE_ERR_ARG;
  if (!pos_off_host || !pos_idx_host || !pos_off || !pos_idx || n_pairs < nrows) return CMHSE_ERR_ARG;
  // the labels, in full, on the host copy: nothing is launched on a list that fails
  if (pos_off_host[0] != 0 || pos_off_host[nrows] != n_pairs) return CMHSE_ERR_ARG;
  for (int32_t i = 0; i < nrows; ++i)
    if (pos_off_host[i + 1] <= pos_off_host[i]) return CMHSE_ERR_ARG;
  for (int32_t e = 0; e < n_pairs; ++e)
    if (pos_idx_host[e] < 0 || pos_idx_host[e] >= M) return CMHSE_ERR_ARG;
  if (!rank || !top1 || !best_pos || !workspace) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_rank_labelled_workspace(nrows, n_pairs))
    return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SimParams p;
  p.A = A;
  p.B = B;
  p.N = N;
  p.M = M;
  p.D = D;
  p.row0 = row0;
  p.nrows = nrows;
  p.n_tiles = (M + kSimBN - 1) / kSimBN;
  p.diag = static_cast<float*>(workspace);   // the thresholds
  p.top1key = reinterpret_cast<score_key_t*>(
      static_cast<char*>(workspace) + align256(static_cast<size_t>(nrows) * sizeof(float)));
  p.rank = rank;
  p.scores = nullptr;
  p.blk_off = nullptr;
  p.blk_stride = 0;
  const int m_tiles = (nrows + kSimBM - 1) / kSimBM;
  const XcdDeal deal = xcd_deal(m_tiles, p.n_tiles);
  p.group = deal.group;
  if (deal.blocks > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  PairParams q;
  q.A = A;
  q.B = B;
  q.M = M;
  q.D = D;
  q.row0 = row0;
  q.nrows = nrows;
  q.n_pairs = n_pairs;
  q.pos_off = pos_off;
  q.pos_idx = pos_idx;
  q.thrkey = p.top1key + nrows;
  if (hipMemsetAsync(rank, 0, sizeof(int32_t) * nrows, stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  if (hipMemsetAsync(p.top1key, 0, 2 * sizeof(score_key_t) * nrows, stream) != hipSuccess)   // and thrkey
    return CMHSE_ERR_LAUNCH;
  int rc = launch_tiles(pair_threshold_kernel<true>, pair_threshold_kernel<false>, D,
                        dim3((n_pairs + kSimBM - 1) / kSimBM), kPairSmem, stream, q);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(label_decode_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, q.thrkey,
                     p.diag, best_pos, best_score, nrows);
  rc = launch_tiles(sim_kernel<kSimLabel, true>, sim_kernel<kSimLabel, false>, D,
                    dim3(static_cast<unsigned>(deal.blocks)), TileSmem<kSimBM, kSimBN>::kBytes, stream, p);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(top1_finalize_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream,
                     p.top1key, top1, nrows);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

namespace {
struct LabelExactWs {
  size_t thr32, top1key, thr64, norm_a, tol, norm_b_max, at_thr, pair64, total;
};
LabelExactWs label_exact_ws(int32_t nrows, int32_t n_pairs) {
  const size_t n = static_cast<size_t>(nrows);
  LabelExactWs L;
  size_t off = 0;
  L.thr32 = off, off += align256(n * sizeof(float));
  L.top1key = off, off += align256(n * sizeof(score_key_t));
  L.thr64 = off, off += align256(n * sizeof(double));
  L.norm_a = off, off += align256(n * sizeof(double));
  L.tol = off, off += align256(n * sizeof(float));
  L.norm_b_max = off, off += 256;
  L.at_thr = off, off += align256(n * sizeof(int32_t));
  L.pair64 = off, off += align256(static_cast<size_t>(n_pairs) * sizeof(double));
  L.total = off;
  return L;
}
}  // namespace

extern "C" size_t cmhse_sim_rank_labelled_exact_workspace(int32_t nrows, int32_t n_pairs) {
  if (nrows <= 0 || n_pairs < nrows) return 0;   // (n_pairs: every query has a positive)
  return label_exact_ws(nrows, n_pairs).total;
}

extern "C" int cmhse_sim_rank_labelled_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                                             int32_t row0, int32_t nrows, const int32_t* pos_off_host,
                                             const int32_t* pos_idx_host, const int32_t* pos_off,
                                             const int32_t* pos_idx, int32_t n_pairs, int32_t* rank_lo,
                                             int32_t* rank_hi, int32_t* top1, int32_t* best_pos,
                                             double* best_score, int32_t* resolved, void* workspace,
                                             size_t workspace_bytes, void* stream_) {
  if (!A || !B) return CMHSE_ERR_ARG;
  if (N <= 0 || M <= 0 || D <= 0) return CMHSE_ERR_ARG;
  if (row0 < 0 || nrows < 0 || static_cast<int64_t>(row0) + nrows > N) return CMHSE_ERR_ARG;
  if (nrows == 0) return n_pairs == 0 ? CMHSE_OK : CMHSE_ERR_ARG;
  if (!pos_off_host || !pos_idx_host || !pos_off || !pos_idx || n_pairs < nrows) return CMHSE_ERR_ARG;
  // the labels, in full, on the host copy: nothing is launched on a list that fails
  if (pos_off_host[0] != 0 || pos_off_host[nrows] != n_pairs) return CMHSE_ERR_ARG;
  for (int32_t i = 0; i < nrows; ++i)
    if (pos_off_host[i + 1] <= pos_off_host[i]) return CMHSE_ERR_ARG;
  for (int32_t e = 0; e < n_pairs; ++e)
    if (pos_idx_host[e] < 0 || pos_idx_host[e] >= M) return CMHSE_ERR_ARG;
  // (the offsets increase from 0 to n_pairs: every e below lies inside pos_idx_host)
  for (int32_t i = 0; i < nrows; ++i)            // strictly ascending: rank_hi needs DISTINCT positives
    for (int32_t e = pos_off_host[i] + 1; e < pos_off_host[i + 1]; ++e)
      if (pos_idx_host[e] <= pos_idx_host[e - 1]) return CMHSE_ERR_ARG;
  if (!rank_lo || !rank_hi || !top1 || !best_pos || !resolved || !workspace) return CMHSE_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0 ||
      workspace_bytes < cmhse_sim_rank_labelled_exact_workspace(nrows, n_pairs))
    return CMHSE_ERR_WORKSPACE;
  if (D >= (1 << 24)) return CMHSE_ERR_UNSUPPORTED;   // (the bound needs D u < 1)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const LabelExactWs L = label_exact_ws(nrows, n_pairs);
  char* const ws = static_cast<char*>(workspace);
  SimParams p;
  int64_t blocks;
  int rc = exact_count_params(&p, &blocks, A, B, N, M, D, row0, nrows, reinterpret_cast<float*>(ws + L.thr32),
                              reinterpret_cast<double*>(ws + L.thr64),
                              reinterpret_cast<score_key_t*>(ws + L.top1key),
                              reinterpret_cast<float*>(ws + L.tol), rank_lo, rank_hi, resolved);
  if (rc != CMHSE_OK) return rc;
  LabelExactPreParams q;
  q.A = A;
  q.B = B;
  q.M = M;
  q.D = D;
  q.row0 = row0;
  q.nrows = nrows;
  q.norm_a = reinterpret_cast<double*>(ws + L.norm_a);
  q.norm_b_max = reinterpret_cast<unsigned*>(ws + L.norm_b_max);
  q.rank_lo = rank_lo;
  q.ties = rank_hi;
  q.resolved = resolved;
  q.top1key = p.top1key;
  PairExactParams t;
  t.A = A;
  t.B = B;
  t.M = M;
  t.D = D;
  t.row0 = row0;
  t.nrows = nrows;
  t.n_pairs = n_pairs;
  t.pos_off = pos_off;
  t.pos_idx = pos_idx;
  t.pair64 = reinterpret_cast<double*>(ws + L.pair64);
  t.thr64 = reinterpret_cast<double*>(ws + L.thr64);
  t.thr32 = p.diag;
  t.at_thr = reinterpret_cast<int32_t*>(ws + L.at_thr);
  t.best_pos = best_pos;
  t.best_score = best_score;
  const int32_t scale = tunables().rank_exact_tol_scale.load(std::memory_order_relaxed);
  constexpr int kWaves = kThreads / 64;
  if (hipMemsetAsync(q.norm_b_max, 0, sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;
  const int64_t pre_rows = static_cast<int64_t>(nrows) + M;
  hipLaunchKernelGGL(label_exact_pre_kernel, dim3(static_cast<unsigned>((pre_rows + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, stream, q);
  hipLaunchKernelGGL(exact_tol_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, q.norm_a,
                     q.norm_b_max, reinterpret_cast<float*>(ws + L.tol), D, scale, nrows);
  hipLaunchKernelGGL(pair_exact_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(n_pairs) + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, stream, t);
  hipLaunchKernelGGL(label_exact_reduce_kernel, dim3((nrows + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, t);
  rc = launch_tiles(sim_kernel<kSimLabelExact, true>, sim_kernel<kSimLabelExact, false>, D,
                    dim3(static_cast<unsigned>(blocks)), TileSmem<kSimBM, kSimBN>::kBytes, stream, p);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(label_exact_finalize_kernel, dim3((nrows + 255) / 256), dim3(256), 0, stream, p.top1key,
                     rank_lo, rank_hi, t.at_thr, top1, nrows);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int cmhse_cosine_sim(const float* im, const float* s, int32_t n, int32_t m, int32_t D,
                                float* scores, void* stream_) {
  if (!im || !s || !scores || n <= 0 || m <= 0 || D <= 0) return CMHSE_ERR_ARG;
  const int rc = launch_sim_store(im, s, n, m, D, scores, static_cast<hipStream_t>(stream_));
  if (rc != CMHSE_OK) return rc;
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

#ifdef TILE_TRACE_BUILD
extern "C" int cmhse_debug_set_sim_trace(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(cmhse::g_sim_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" const char* cmhse_strerror(int code) {
  switch (code) {
    case CMHSE_OK: return "ok";
    case CMHSE_ERR_ARG: return "invalid argument";
    case CMHSE_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
    case CMHSE_ERR_LAUNCH: return "HIP launch/runtime error";
    case CMHSE_ERR_UNSUPPORTED: return "shape not supported";
    case CMHSE_ERR_TIMEOUT:
      return "a resident chain kernel gave up at a grid barrier (its workgroups were not all on the chip: "
             "shared GPU, CU mask?); results of that call are invalid; clear with cmhse_async_status(1) and "
             "set the *_tail_min_steps / *_chain_min_steps tunables to 0 on such a GPU";
    default: return "unknown error";
  }
}

extern "C" const char* cmhse_version(void) { return "cmhse_hip 0.6.0 gfx950"; }
