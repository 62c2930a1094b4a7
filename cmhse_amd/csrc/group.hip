// group.hip — group-wise (video, paragraph) scores and their ranking, matrix-free at the clip level.
//
// G[i, j] reduces the clip x caption scores C[r] . S[c] over the clips r of video i and the captions
// c of paragraph j: the block maximum (CMHSE_GROUP_MAX) or the block mean (CMHSE_GROUP_MEAN: the
// fp32 scores summed in fp64 sequentially in row-major order — clip-major, then caption — divided in
// fp64 by the count, rounded to fp32).  That is the block reduction of GroupWiseContrastiveLoss
// (loss.py:26-41, sim.hip: block_reduce_kernel, which adds in exactly this order for blocks of at most
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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "nt_core.hpp"
#include "score_tile.hpp"

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

template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_sim_kernel(const GroupParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
      if (p.use_max) {
        float m = cont ? cmax[q] : -INFINITY;
        for (int r = lo; r < hi; ++r) {
          const float* srow_ = stage + (r - h0) * kGrLd;
          for (int c = cs; c < ce; ++c) {
            const float x = srow_[c];
            m = x > m ? x : m;
          }
        }
        if (re > h1) cmax[q] = m;
        else p.G[static_cast<int64_t>(v0 + v) * p.B + q0 + q] = m;
      } else {
        double sum = cont ? carry[q] : 0.0;
        for (int r = lo; r < hi; ++r) {
          const float* srow_ = stage + (r - h0) * kGrLd;
          for (int c = cs; c < ce; ++c) sum += static_cast<double>(srow_[c]);
        }
        if (re > h1) carry[q] = sum;
        else
          p.G[static_cast<int64_t>(v0 + v) * p.B + q0 + q] =
              static_cast<float>(sum / static_cast<double>((re - rs) * (ce - cs)));
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

// prefix sums of B >= 1 positive counts, Nc / Ns at the end
bool offsets_ok(const int32_t* off, int32_t B) {
  if (off[0] != 0) return false;
  for (int32_t b = 0; b < B; ++b)
    if (off[b + 1] <= off[b]) return false;
  return true;
}

// the plan's tile starts: [0, ..., B], strictly increasing, every tile's rows <= cap
bool tiles_ok(const int32_t* start, int32_t T, const int32_t* off, int32_t B, int cap) {
  if (T < 1 || T > B || start[0] != 0 || start[T] != B) return false;
  for (int32_t t = 0; t < T; ++t)
    if (start[t + 1] <= start[t] || off[start[t + 1]] - off[start[t]] > cap) return false;
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

// greedy packing of whole groups (in order) into tiles of at most `cap` rows; returns the tile count
int32_t pack(const int32_t* off, int32_t B, int cap, int32_t* start) {
  int32_t T = 0;
  start[T++] = 0;
  int32_t first = 0;
  for (int32_t b = 1; b < B; ++b)
    if (off[b + 1] - off[first] > cap) {
      start[T++] = b;
      first = b;
    }
  start[T] = B;
  return T;
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
