"""The launches of the scoring kernels — sim.hip (sim_rank, sim_rank_labelled, sim_rank_exact),
topk.hip (sim_topk) and group.hip (group_scores, group_rank, group_topk) — restated for one request,
and the case tables, inputs and references of tests/test_gpu_score_shapes.py.

How a grid of tiles is dealt to workgroups (xcd_deal / xcd_deal_tile, score_tile.hpp), how many
gallery panels a top-K launch walks and which tiles each panel holds (topk_panels, gt_panels), how
many query groups share a workgroup (gt_qcap): all of it is decided on the host from the shapes
alone, and no result can show which arm ran.  This module lets a CPU test prove that every case
reaches the arm it names (tests/test_score_shapes_cpu.py); the constants the rules use are parsed
from the sources there.

Two input families, neither of which depends on a product kernel:
  lattice   rows of small integers: every score is an integer far below 2^24, exact in fp32 and
            in float64 whatever the summation order; the expected values are int64 NumPy and every
            output is compared bit for bit, ties included (they are abundant);
  gaussian  unit-norm fp32 rows, the paired rows correlated, against float64 under score_bar()."""
import functools
import os
import re

import numpy as np

from loss_shapes import CSRC, REPO, SIM_SMALL_MAX  # noqa: F401

# constants of the sources (checked against them by tests/test_score_shapes_cpu.py)
XCDS, WGS_PER_XCD = 8, 96                    # score_tile.hpp kXcds / kWgsPerXcd
SIM_BM, SIM_BN = 128, 128                    # sim.hip kSimBM / kSimBN
TK_BM, TK_BN = 64, 128                       # topk.hip kTkBM / kTkBN
TK_CUS, TK_LDS_PER_CU = 256, 160 * 1024      # topk.hip kTkCUs / kTkLdsPerCU
GR_BM, GR_BN, GR_RANK_T = 128, 128, 64       # group.hip kGrBM / kGrBN / kGrRankT
GT_CUS, GT_LDS_PER_CU, GT_QCAP_MAX = 256, 160 * 1024, 64   # group.hip kGtCUs / kGtLdsPerCU / kGtQcapMax
LDS_LD, BK, THREADS = 20, 16, 256            # nt_core.hpp kLdsLd / kBK / kThreads
TOPK_MAX = 128                               # cmhse_hip.h CMHSE_TOPK_MAX
KEY_BYTES = 8                                # sizeof(score_key_t)
GT_HDR = 8                                   # group.hip kGtHdr
GR_HDR = 5                                   # group.hip kGrHdr

U32 = 2.0 ** -24                             # the unit roundoff of fp32


def ceil_div(a, b):
  return -(-a // b)


def align256(v):
  return (v + 255) // 256 * 256


def tile_smem(bm, bn):
  """nt_core.hpp TileSmem<BM, BN>::kBytes: two buffers of (BM + BN) rows of kLdsLd floats."""
  return 4 * 2 * (bm + bn) * LDS_LD


# --------------------------------------------------------------------------------------------
# the XCD-grouped deal (score_tile.hpp)
# --------------------------------------------------------------------------------------------
def xcd_deal(row_tiles, col_tiles):
  """(G, blocks): G row tiles x one column tile per group, or G = 0: plain row-major order."""
  tiles = row_tiles * col_tiles
  ideal_rounds = ceil_div(tiles, XCDS * WGS_PER_XCD)
  for g in (4, 3, 2):
    groups = ceil_div(row_tiles, g) * col_tiles
    per_label = ceil_div(groups, XCDS)
    if ceil_div(per_label * g, WGS_PER_XCD) <= ideal_rounds:
      return g, per_label * XCDS * g
  return 0, tiles


def xcd_deal_tile(block, G, col_tiles):
  """Block -> (row tile, column tile) for G > 0; also works on NumPy arrays of blocks."""
  x, q = block & 7, block >> 3
  Q = (q // G) * 8 + x
  return G * (Q // col_tiles) + q % G, Q % col_tiles


def deal_tile(block, G, row_tiles, col_tiles):
  """(row tile, column tile) of a block of the counting pass / group_sim_kernel, None for padding."""
  if G == 0:
    return block // col_tiles, block % col_tiles
  rt, ct = xcd_deal_tile(block, G, col_tiles)
  return None if rt >= row_tiles else (int(rt), int(ct))


def count_plan(nrows, M):
  """The counting pass of sim_rank / sim_rank_labelled / sim_rank_exact over a stripe of nrows rows."""
  row_tiles, col_tiles = ceil_div(nrows, SIM_BM), ceil_div(M, SIM_BN)
  G, blocks = xcd_deal(row_tiles, col_tiles)
  return dict(row_tiles=row_tiles, col_tiles=col_tiles, G=G, blocks=blocks, padding=blocks - row_tiles * col_tiles)


def sim_store_tile(n, m):
  """launch_sim_store: 64 x 64 tiles when both sizes are at most kSimSmallMax, else 128 x 128."""
  return 64 if n <= SIM_SMALL_MAX and m <= SIM_SMALL_MAX else SIM_BN


# --------------------------------------------------------------------------------------------
# top-K (topk.hip)
# --------------------------------------------------------------------------------------------
def topk_smem(K):
  tile = max(tile_smem(TK_BM, TK_BN), 4 * TK_BM * (TK_BN + 8))
  return tile + KEY_BYTES * TK_BM * K + KEY_BYTES * TK_BN * (THREADS // 64)


def topk_per_cu(K):
  return max(1, min(4, TK_LDS_PER_CU // topk_smem(K)))


def topk_panels(nrows, M, K):
  row_tiles, col_tiles = ceil_div(nrows, TK_BM), ceil_div(M, TK_BN)
  return max(1, min(TK_CUS * topk_per_cu(K) // row_tiles, col_tiles))


def panel_bounds(tiles, panels):
  """[t_begin, t_end) of every panel: the split panel * tiles / panels of both select kernels."""
  return [(p * tiles // panels, (p + 1) * tiles // panels) for p in range(panels)]


def panel_block(block, blocks, q_tiles, panels):
  """Block -> (panel, query tile) of topk_select_kernel / group_topk_select_kernel, None for padding."""
  per_xcd = blocks >> 3
  L = (block & 7) * per_xcd + (block >> 3)
  return None if L >= q_tiles * panels else (L // q_tiles, L % q_tiles)


def topk_plan(nrows, M, K):
  row_tiles, col_tiles = ceil_div(nrows, TK_BM), ceil_div(M, TK_BN)
  panels = topk_panels(nrows, M, K)
  blocks = ceil_div(row_tiles * panels, 8) * 8
  return dict(row_tiles=row_tiles, col_tiles=col_tiles, panels=panels, blocks=blocks,
              padding=blocks - row_tiles * panels, bounds=panel_bounds(col_tiles, panels),
              uncapped=TK_CUS * topk_per_cu(K) // row_tiles, smem=topk_smem(K),
              workspace=align256(panels * nrows * K * KEY_BYTES))


# --------------------------------------------------------------------------------------------
# group-wise top-K (group.hip)
# --------------------------------------------------------------------------------------------
GT_LIST_OFF = tile_smem(GR_BM, GR_BN) + KEY_BYTES * GR_BN * (THREADS // 64)


def gt_qcap(K):
  """Query groups per query tile at K: two workgroups' LDS per CU, in multiples of 8, at most 64;
  below 32 (K > 72) one workgroup per CU.  The fixed part is the 40 KB tile buffers and four 128-key
  candidate buffers; a query group costs its K keys and a row of 129 block scores."""
  per_q = KEY_BYTES * K + 4 * (GR_BN + 1)
  q = (GT_LDS_PER_CU // 2 - GT_LIST_OFF) // per_q // 8 * 8
  if q < 32:
    q = (GT_LDS_PER_CU - GT_LIST_OFF) // per_q // 8 * 8
  return min(q, GT_QCAP_MAX)


qcap = gt_qcap      # the name tests/test_group_topk_cpu.py uses


def gt_smem(K):
  return GT_LIST_OFF + (KEY_BYTES * K + 4 * (GR_BN + 1)) * gt_qcap(K)


def gt_per_cu(K):
  return max(1, min(4, GT_LDS_PER_CU // gt_smem(K)))


def gt_panels(q_tiles, g_tiles, K):
  slots = GT_CUS * gt_per_cu(K)
  P0 = max(1, slots // q_tiles)
  best, best_rounds = P0, ceil_div(q_tiles * P0, slots)
  for P in range(P0 + 1, 4 * P0 + 4):
    rounds = ceil_div(q_tiles * P, slots)
    if 10 * rounds * best < 9 * best_rounds * P:
      best, best_rounds = P, rounds
  return min(best, g_tiles)


def _lib():
  from cmhse_amd import _lib
  return _lib.load()


def _offsets(counts):
  off = np.zeros(len(counts) + 1, dtype=np.int32)
  np.cumsum(counts, out=off[1:])
  return off


def group_tiles(nclips, ncaps):
  """(row tiles, column tiles) of cmhse_group_plan (host only) for these counts."""
  B = len(nclips)
  assert len(ncaps) == B
  oc, op = _offsets(nclips), _offsets(ncaps)
  plan = np.empty(4 * B + 9, dtype=np.int32)
  n = _lib().cmhse_group_plan(oc.ctypes.data, op.ctypes.data, B, plan.ctypes.data, plan.size)
  assert n > 0, n
  return int(plan[3]), int(plan[4])


def group_plan(nclips, ncaps):
  R, C = group_tiles(nclips, ncaps)
  G, blocks = xcd_deal(R, C)
  return dict(row_tiles=R, col_tiles=C, G=G, blocks=blocks, padding=blocks - R * C)


def group_topk_host_plan(nclips, ncaps, direction, K):
  """cmhse_group_topk_plan (host only): the int32 plan, direction 'p2v' (0) or 'v2p' (1)."""
  Bv, Bp = len(nclips), len(ncaps)
  oc, op = _offsets(nclips), _offsets(ncaps)
  plan = np.empty(2 * Bv + 2 * Bp + 12, dtype=np.int32)
  n = _lib().cmhse_group_topk_plan(oc.ctypes.data, Bv, op.ctypes.data, Bp, 0 if direction == 'p2v' else 1, K,
                                   plan.ctypes.data, plan.size)
  assert n > 0, n
  return plan[:n].copy()


def group_topk_plan(nclips, ncaps, direction, K):
  plan = group_topk_host_plan(nclips, ncaps, direction, K)
  Bv, Bp, R, C = (int(plan[i]) for i in (0, 1, 6, 7))
  p2v = direction == 'p2v'
  q_tiles, g_tiles, Bq = (C, R, Bp) if p2v else (R, C, Bv)
  start = plan[GT_HDR + Bv + Bp + 2:]
  q_start = start[R + 1:R + C + 2] if p2v else start[:R + 1]
  panels = gt_panels(q_tiles, g_tiles, K)
  blocks = ceil_div(q_tiles * panels, 8) * 8
  return dict(q_tiles=q_tiles, g_tiles=g_tiles, panels=panels, blocks=blocks, padding=blocks - q_tiles * panels,
              bounds=panel_bounds(g_tiles, panels), qcap=gt_qcap(K), smem=gt_smem(K), host_plan=plan,
              most_queries=int(np.diff(q_start).max()), workspace=align256(panels * Bq * K * KEY_BYTES))


# --------------------------------------------------------------------------------------------
# the bars ("Bars and conditions" of the issue of this file)
# --------------------------------------------------------------------------------------------
def gamma(D):
  """gamma_D(u) = D u / (1 - D u), u = 2^-24 (Higham, Accuracy and Stability, section 3.1)."""
  return D * U32 / (1.0 - D * U32)


def score_bar(D, norm_a, norm_b):
  """A score is a chain of D fp32 fused multiply-adds: it lies within gamma_D(u) |a| |b| of the
  exact product (the derivation above exact_tolerance in sim.hip, without its float64, underflow
  and slack terms, which only add).  The margin bar of an exact rank / index comparison is twice
  it: two scores, one bar each."""
  return gamma(D) * norm_a * norm_b


# --------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------
def lattice_rows(n, D, seed):
  """[n, D] fp32 rows of integers in [-2, 2]."""
  return np.random.RandomState(seed).randint(-2, 3, size=(n, D)).astype(np.float32)


def gaussian_pair(n, M, D, seed, corr):
  """(a [n, D], b [M, D]) unit-norm fp32 rows; b[i] += corr * a[i] for the paired rows i < min(n, M)."""
  rng = np.random.RandomState(seed)
  a = rng.standard_normal((n, D))
  b = rng.standard_normal((M, D))
  p = min(n, M)
  b[:p] += corr * a[:p]
  a /= np.linalg.norm(a, axis=1, keepdims=True)
  b /= np.linalg.norm(b, axis=1, keepdims=True)
  return a.astype(np.float32), b.astype(np.float32)


def scores_int(a, b):
  """The exact scores of lattice rows, int64 (integers far below 2^53: the float64 product is exact)."""
  return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def scores_f64(a, b):
  return a.astype(np.float64) @ b.astype(np.float64).T


def row_bars(a, b, D):
  """score_bar per query row: its own norm times the largest gallery norm ([n] float64)."""
  na = np.linalg.norm(a.astype(np.float64), axis=1)
  nb = np.linalg.norm(b.astype(np.float64), axis=1).max()
  return score_bar(D, na, nb)


def positives_of(n, M, row0=0):
  """The labels of the labelled-ranking cases as CSR over n queries: the paired row row0 + i, for
  every third query a second positive and for every seventh a third one (distinct, anywhere)."""
  lists = []
  for i in range(n):
    g = row0 + i
    p = [g % M]
    if i % 3 == 0:
      p.append((g * 7 + 3) % M)
    if i % 7 == 0:
      p.append((g * 13 + M // 2) % M)
    lists.append(sorted(set(p)))
  off = np.zeros(n + 1, dtype=np.int64)
  np.cumsum([len(p) for p in lists], out=off[1:])
  return off, np.concatenate(lists).astype(np.int64)


# --------------------------------------------------------------------------------------------
# references (NumPy; S is int64 or float64 [n, M], row r belongs to query row0 + r)
# --------------------------------------------------------------------------------------------
def rank_reference(S, row0=0):
  """sim_rank: (rank, top1) = the columns strictly above the diagonal, the first largest column."""
  n = S.shape[0]
  diag = S[np.arange(n), row0 + np.arange(n)][:, None]
  return np.count_nonzero(S > diag, axis=1), S.argmax(axis=1)


def exact_reference(S, row0=0):
  """sim_rank_exact: (rank_lo, rank_hi): the other columns strictly above / at or above the diagonal."""
  n = S.shape[0]
  diag = S[np.arange(n), row0 + np.arange(n)][:, None]
  return np.count_nonzero(S > diag, axis=1), np.count_nonzero(S >= diag, axis=1) - 1


def labelled_reference(S, off, idx):
  """sim_rank_labelled: (rank, top1, best_pos, best_score): the best positive is the largest score
  among the query's positives (smallest index on ties), the rank counts every column above it."""
  n = S.shape[0]
  best_pos = np.empty(n, dtype=np.int64)
  for i in range(n):
    p = idx[off[i]:off[i + 1]]           # ascending
    best_pos[i] = p[np.argmax(S[i, p])]
  thr = S[np.arange(n), best_pos]
  return np.count_nonzero(S > thr[:, None], axis=1), S.argmax(axis=1), best_pos, thr


def topk_reference(S, K):
  """(score [n, K], index [n, K]): score descending, then index ascending."""
  n, M = S.shape
  if M <= 4 * K:
    order = np.argsort(-S, axis=1, kind='stable')[:, :K]
  else:      # the same order from the columns at or above each row's K-th largest score only
    kth = -np.partition(-S, K - 1, axis=1)[:, K - 1]
    order = np.empty((n, K), dtype=np.int64)
    for r in range(n):
      cand = np.flatnonzero(S[r] >= kth[r])                 # ascending index
      order[r] = cand[np.argsort(-S[r, cand], kind='stable')[:K]]
  return np.take_along_axis(S, order, axis=1), order


def block_reduce(S, nrow, ncol, reduce):
  """The (row group, column group) blocks of S reduced: 'max', or 'sum' (divide by block_counts)."""
  ro, co = _offsets(nrow)[:-1], _offsets(ncol)[:-1]
  f = np.maximum if reduce == 'max' else np.add
  return f.reduceat(f.reduceat(S, ro, axis=0), co, axis=1)


def block_counts(nrow, ncol):
  return np.outer(np.asarray(nrow, dtype=np.int64), np.asarray(ncol, dtype=np.int64))


def lattice_group_scores(S, nclips, ncaps, reduce):
  """group_scores of integer scores as fp32: the block max, or the exact integer sum divided in
  float64 by the count and rounded to fp32 (the two correctly rounded operations the contract
  names; with power-of-two counts the quotient is exact and nothing rounds at all)."""
  if reduce == 'max':
    return block_reduce(S, nclips, ncaps, 'max').astype(np.float32)
  return (block_reduce(S, nclips, ncaps, 'sum').astype(np.float64) / block_counts(nclips, ncaps)).astype(np.float32)


def f64_group_scores(S, nclips, ncaps, reduce):
  if reduce == 'max':
    return block_reduce(S, nclips, ncaps, 'max')
  return block_reduce(S, nclips, ncaps, 'sum') / block_counts(nclips, ncaps)


def group_rank_reference(G):
  """(rank_v2p, top1_v2p, rank_p2v, top1_p2v) of a square G: sim_rank's rules along rows and columns."""
  d = np.diag(G)
  return ((G > d[:, None]).sum(axis=1), G.argmax(axis=1), (G > d[None, :]).sum(axis=0), G.argmax(axis=0))


# --------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------
VOCABULARY = {
    'Count G=4 partial group and padding',
    'Count G=3 one row tile', 'Count G=3 row tiles not a multiple',
    'Count G=2 one row tile', 'Count G=2 row tiles not a multiple',
    'Count G=0 one row tile', 'Count G=0 several row tiles',
    'Count stripe G=4', 'Count stripe G=3', 'Count stripe G=2', 'Count stripe G=0',
    'Count float4 loads below kBK', 'Count scalar loads', 'Count whole k chunks', 'Count partial k chunk',
    'Count ragged gallery', 'Count grid over 2^31 blocks',
    'Group G=4', 'Group G=3', 'Group G=2', 'Group G=0', 'Group padding blocks',
    'Topk multi-tile panels', 'Topk uneven split', 'Topk partial last tile', 'Topk padding blocks',
    'Topk K=1', 'Topk K mid', 'Topk K=128', 'Topk ragged rows', 'Topk stripe', 'Topk fewer panels than one',
    'Topk LDS for less than one workgroup',
    'GroupTopk multi-tile panels p2v', 'GroupTopk multi-tile panels v2p', 'GroupTopk uneven split',
    'GroupTopk query cap below 64', 'GroupTopk padding blocks', 'GroupTopk full query tile',
}

# Arms that no test-size case can reach, with the size at which they start (an explicit list:
# tests/test_score_shapes_cpu.py holds it to these entries and checks the sizes).
UNREACHABLE = {
    'Count grid over 2^31 blocks':
        'CMHSE_ERR_UNSUPPORTED of the counting passes, group_sim_kernel and both top-K launches: a grid of 2^31 '
        'workgroups is 46 341 x 46 341 tiles of 128 x 128, about 5.9 million rows on each side',
    'Topk LDS for less than one workgroup':
        'the per_cu < 1 floors of topk_panels and gt_panels: the LDS of one workgroup grows with K and is 102 KB '
        '(topk) / 140 KB (group) at K = CMHSE_TOPK_MAX = 128, below the 160 KB of a CU; no K the API accepts gets there',
}

# Counting passes: (id, N, M, D, row0, nrows, gaussian correlation, targets).  Every case runs through
# sim_rank, sim_rank_labelled and sim_rank_exact.  The stripe is [row0, row0 + nrows) of N query rows.
COUNT_CASES = [
    ('g4_partial_group', 600, 5000, 12, 0, 600, 1.0,                  # 5 x 40 tiles: 320 blocks for 200 tiles
     {'Count G=4 partial group and padding', 'Count float4 loads below kBK', 'Count ragged gallery',
      'Count partial k chunk'}),
    ('g3_one_row_tile', 100, 24654, 8, 0, 100, 2.0,                   # 1 x 193
     {'Count G=3 one row tile', 'Count float4 loads below kBK', 'Count ragged gallery'}),
    ('g3_five_row_tiles', 603, 12413, 30, 0, 603, 0.7,                # 5 x 97
     {'Count G=3 row tiles not a multiple', 'Count scalar loads', 'Count partial k chunk'}),
    ('g2_one_row_tile', 70, 32796, 12, 0, 70, 1.5,                    # 1 x 257
     {'Count G=2 one row tile'}),
    ('g2_thirteen_row_tiles', 1644, 6649, 8, 0, 1644, 2.0,            # 13 x 52
     {'Count G=2 row tiles not a multiple'}),
    ('g0_one_row_tile', 128, 49279, 8, 0, 128, 2.0,                   # 1 x 385
     {'Count G=0 one row tile'}),
    ('g0_five_row_tiles', 639, 16503, 64, 0, 639, 0.5,                # 5 x 129
     {'Count G=0 several row tiles', 'Count whole k chunks', 'Count ragged gallery'}),
    ('stripe_g4', 900, 5000, 12, 77, 600, 1.0, {'Count stripe G=4'}),
    ('stripe_g3', 800, 12413, 8, 101, 603, 2.0, {'Count stripe G=3'}),
    ('stripe_g2', 1800, 6649, 8, 45, 1644, 2.0, {'Count stripe G=2'}),
    ('stripe_g0', 700, 16503, 12, 33, 639, 1.5, {'Count stripe G=0'}),
]
# the stripes that must concatenate to a full call: (id, N, M, D, cuts) — the pieces land on different arms
COUNT_STRIPES = ('stripes_concatenate', 1644, 6649, 8, (0, 45, 685, 1644))


def count_tags(case):
  name, N, M, D, row0, nrows, corr, _ = case
  pl = count_plan(nrows, M)
  G, R = pl['G'], pl['row_tiles']
  tags = set()
  stripe = row0 > 0 and row0 % 64 != 0
  if stripe:
    tags.add('Count stripe G=%d' % G)
  if G == 4 and R % 4 != 0 and pl['padding'] > 0:
    tags.add('Count G=4 partial group and padding')
  if G in (2, 3):
    if R == 1:
      tags.add('Count G=%d one row tile' % G)
    elif R % G != 0:
      tags.add('Count G=%d row tiles not a multiple' % G)
  if G == 0:
    tags.add('Count G=0 one row tile' if R == 1 else 'Count G=0 several row tiles')
  if D % 4 == 0 and D < BK:
    tags.add('Count float4 loads below kBK')
  if D % 4 != 0:
    tags.add('Count scalar loads')
  tags.add('Count whole k chunks' if D % BK == 0 else 'Count partial k chunk')
  if M % SIM_BN != 0:
    tags.add('Count ragged gallery')
  if pl['blocks'] > 0x7fffffff:
    tags.add('Count grid over 2^31 blocks')
  return tags


def _tiled(spec):
  """Counts from [(groups, rows per group)] runs."""
  out = []
  for groups, rows in spec:
    out += [rows] * groups
  return out


# group_scores / group_rank: (id, clip counts, caption counts, D, targets).  Every count is a power
# of two, so a block's element count is one and the mean of integer scores is exact.  Single-clip
# videos pack 128 to a row tile; paragraphs of 8 / 4 / 2 / 1 captions pack 16 / 32 / 64 / 128 to a column tile.
GROUP_CASES = [
    ('group_g4', _tiled([(600, 1)]), _tiled([(300, 8), (300, 2)]), 8, {'Group G=4', 'Group padding blocks'}),         # 5 x 24
    ('group_g3', _tiled([(1152, 1)]), _tiled([(928, 8), (224, 4)]), 8, {'Group G=3', 'Group padding blocks'}),        # 9 x 65
    ('group_g2', _tiled([(1280, 1)]), _tiled([(800, 8), (480, 4)]), 8, {'Group G=2', 'Group padding blocks'}),        # 10 x 65
    ('group_g0', _tiled([(128, 2), (1152, 1)]), _tiled([(800, 8), (480, 4)]), 12, {'Group G=0'}),                     # 11 x 65
]


def group_tags(case):
  name, nclips, ncaps, D, _ = case
  pl = group_plan(nclips, ncaps)
  tags = {'Group G=%d' % pl['G']}
  if pl['padding'] > 0:
    tags.add('Group padding blocks')
  return tags


# sim_topk: (id, N, M, D, K, row0, nrows, gaussian correlation, targets)
TOPK_CASES = [
    ('topk_k1', 1200, 8300, 8, 1, 0, 1200, 2.0,
     {'Topk multi-tile panels', 'Topk uneven split', 'Topk partial last tile', 'Topk padding blocks', 'Topk K=1',
      'Topk ragged rows'}),
    ('topk_k17', 1290, 8300, 12, 17, 0, 1290, 1.0,
     {'Topk multi-tile panels', 'Topk uneven split', 'Topk partial last tile', 'Topk padding blocks', 'Topk K mid',
      'Topk ragged rows'}),
    ('topk_k128', 1290, 3700, 30, 128, 0, 1290, 0.7,
     {'Topk multi-tile panels', 'Topk uneven split', 'Topk partial last tile', 'Topk padding blocks', 'Topk K=128',
      'Topk ragged rows'}),
    ('topk_stripe', 1500, 3700, 8, 128, 150, 1290, 2.0,
     {'Topk multi-tile panels', 'Topk uneven split', 'Topk stripe', 'Topk K=128'}),
    ('topk_one_panel', 16448, 300, 8, 128, 0, 16448, 2.0,                 # 257 row tiles: 256 / 257 = 0 panels -> 1
     {'Topk fewer panels than one', 'Topk multi-tile panels', 'Topk K=128'}),
]
TOPK_STRIPES = ('topk_stripes_concatenate', 1290, 3700, 8, 128, (0, 150, 700, 1290))


def topk_tags(case):
  name, N, M, D, K, row0, nrows, corr, _ = case
  pl = topk_plan(nrows, M, K)
  tags = set()
  sizes = [e - b for b, e in pl['bounds']]
  if max(sizes) >= 2:
    tags.add('Topk multi-tile panels')
  if pl['col_tiles'] % pl['panels'] != 0:
    tags.add('Topk uneven split')
  if M % TK_BN != 0:
    tags.add('Topk partial last tile')
  if pl['padding'] > 0:
    tags.add('Topk padding blocks')
  tags.add('Topk K=1' if K == 1 else ('Topk K=128' if K == TOPK_MAX else 'Topk K mid'))
  if nrows % TK_BM != 0:
    tags.add('Topk ragged rows')
  if row0 > 0 and row0 % 64 != 0:
    tags.add('Topk stripe')
  if pl['uncapped'] < 1:
    tags.add('Topk fewer panels than one')
  if TK_LDS_PER_CU // topk_smem(K) < 1:
    tags.add('Topk LDS for less than one workgroup')
  return tags


# group_topk: (id, clip counts, caption counts, D, K, targets); every case runs both reductions in the
# direction its query side names.  Gallery groups of 128 and 64 rows alternate: one group a tile (64 +
# 128 > 128), tiles of both heights, power-of-two counts.  Single-row query groups fill the cap.
_GT_GALLERY = [128, 64] * 21 + [128]           # 43 gallery tiles
GTOPK_CASES = [
    ('gtopk_p2v', _GT_GALLERY, [1] * 5590, 8, 10, 'p2v',
     {'GroupTopk multi-tile panels p2v', 'GroupTopk uneven split', 'GroupTopk query cap below 64',
      'GroupTopk full query tile', 'GroupTopk padding blocks'}),
    ('gtopk_v2p', [1] * 5590, _GT_GALLERY, 12, 10, 'v2p',
     {'GroupTopk multi-tile panels v2p', 'GroupTopk uneven split', 'GroupTopk query cap below 64',
      'GroupTopk full query tile', 'GroupTopk padding blocks'}),
]


def gtopk_tags(case):
  name, nclips, ncaps, D, K, direction, _ = case
  pl = group_topk_plan(nclips, ncaps, direction, K)
  tags = set()
  if max(e - b for b, e in pl['bounds']) >= 2:
    tags.add('GroupTopk multi-tile panels ' + direction)
  if pl['g_tiles'] % pl['panels'] != 0:
    tags.add('GroupTopk uneven split')
  if pl['qcap'] < GT_QCAP_MAX:
    tags.add('GroupTopk query cap below 64')
  if pl['most_queries'] == pl['qcap']:
    tags.add('GroupTopk full query tile')
  if pl['padding'] > 0:
    tags.add('GroupTopk padding blocks')
  if GT_LDS_PER_CU // gt_smem(K) < 1:
    tags.add('Topk LDS for less than one workgroup')
  return tags


def all_case_tags():
  """{case id: tags} over the four tables."""
  out = {}
  for table, fn in ((COUNT_CASES, count_tags), (GROUP_CASES, group_tags), (TOPK_CASES, topk_tags),
                    (GTOPK_CASES, gtopk_tags)):
    for case in table:
      assert case[0] not in out, case[0]
      out[case[0]] = fn(case)
  return out


# --------------------------------------------------------------------------------------------
# the case inputs (cached: the CPU proofs and the GPU tests of one process share them)
# --------------------------------------------------------------------------------------------
def _seed(name):
  return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


@functools.lru_cache(maxsize=None)
def count_inputs(name, family):
  """(a [N, D], b [M, D]) of a COUNT_CASES / TOPK_CASES entry."""
  for case in COUNT_CASES:
    if case[0] == name:
      _, N, M, D, row0, nrows, corr, _ = case
      break
  else:
    case = [c for c in TOPK_CASES if c[0] == name][0]
    _, N, M, D, K, row0, nrows, corr, _ = case
  if family == 'lattice':
    return lattice_rows(N, D, _seed(name)), lattice_rows(M, D, _seed(name) + 1)
  return gaussian_pair(N, M, D, _seed(name), corr)


@functools.lru_cache(maxsize=None)
def group_inputs(name, family):
  """(clips [Nc, D], caps [Ns, D]) of a GROUP_CASES / GTOPK_CASES entry."""
  case = [c for c in GROUP_CASES + GTOPK_CASES if c[0] == name][0]
  Nc, Ns, D = sum(case[1]), sum(case[2]), case[3]
  if family == 'lattice':
    return lattice_rows(Nc, D, _seed(name)), lattice_rows(Ns, D, _seed(name) + 1)
  return gaussian_pair(Nc, Ns, D, _seed(name), 0.0)


def margin_ok(S, bars, ref_col):
  """Rows of the float64 scores S whose comparisons with column ref_col[r] are all decided beyond the
  margin bar 2 bars[r] — and whose two largest scores are as far apart (the top-1): (rank rows, top-1 rows)."""
  n = S.shape[0]
  gap = np.abs(S - S[np.arange(n), ref_col][:, None])
  gap[np.arange(n), ref_col] = np.inf
  top2 = -np.partition(-S, 1, axis=1)[:, :2]
  return gap.min(axis=1) > 2 * bars, (top2[:, 0] - top2[:, 1]) > 2 * bars


# --------------------------------------------------------------------------------------------
# the sources
# --------------------------------------------------------------------------------------------
def _read(*path):
  return open(os.path.join(*path)).read()


def _one(pattern, text, what):
  m = re.findall(pattern, text)
  assert len(m) == 1, (what, m)
  return m[0]


def source_constants():
  """The constants above as the sources state them, and the lines of the deal and of the panel walk
  that the rules restate (asserted present, once each where they are unique)."""
  tile, sim, topk, group, core = (_read(CSRC, n) for n in ('score_tile.hpp', 'sim.hip', 'topk.hip', 'group.hip',
                                                            'nt_core.hpp'))
  header = _read(REPO, 'include', 'cmhse_hip.h')
  defines = {k: int(v) for k, v in re.findall(r'#define (CMHSE_\w+) (\d+)\b', header)}

  def const(text, name):
    v = _one(r'\b%s\s*=\s*([\w ]+?(?:\s*\*\s*\d+)?)\s*;' % name, text, name).strip()
    if v in defines:
      return defines[v]
    prod = 1
    for f in v.split('*'):
      prod *= int(f)
    return prod
  found = dict(CMHSE_TOPK_MAX=defines['CMHSE_TOPK_MAX'])
  for text, names in ((tile, ('kXcds', 'kWgsPerXcd')), (sim, ('kSimBM', 'kSimBN', 'kSimSmallMax')),
                      (topk, ('kTkBM', 'kTkBN', 'kTkCUs', 'kTkLdsPerCU')),
                      (group, ('kGrBM', 'kGrBN', 'kGrRankT', 'kGtCUs', 'kGtLdsPerCU', 'kGtQcapMax', 'kGtHdr', 'kGrHdr')),
                      (core, ('kLdsLd', 'kBK', 'kThreads'))):
    for name in names:
      found[name] = const(text, name)
  # xcd_deal: G from 4 down to 2, groups per label, rounds against the even deal's
  assert len(re.findall(r'for \(int g = 4; g >= 2; --g\) \{', tile)) == 1
  assert len(re.findall(r'if \(\(per_label \* g \+ kWgsPerXcd - 1\) / kWgsPerXcd <= ideal_rounds\) '
                        r'return \{g, per_label \* kXcds \* g\};', tile)) == 1
  # xcd_deal_tile
  assert len(re.findall(r'const int x = block & 7, q = block >> 3;\s*const int Q = \(q / G\) \* 8 \+ x;\s*'
                        r'return \{G \* \(Q / col_tiles\) \+ \(q % G\), Q % col_tiles\};', tile)) == 1
  # the plain order of the counting pass, the three entry points' deal
  assert len(re.findall(r'j0 = \(blockIdx\.x % p\.n_tiles\) \* BN;\s*i0 = \(blockIdx\.x / p\.n_tiles\) \* BM;', sim)) == 1
  assert len(re.findall(r'const XcdDeal deal = xcd_deal\(m_tiles, p\.n_tiles\);', sim)) == 3
  assert len(re.findall(r'const XcdDeal deal = xcd_deal\(p\.row_tiles, p\.col_tiles\);', group)) == 1
  # the panel walk of both select kernels and their padded grids
  for text, tiles, q in ((topk, 'col_tiles', 'row_tiles'), (group, 'g_tiles', 'q_tiles')):
    assert len(re.findall(r'static_cast<int64_t>\(panel\) \* p\.%s / p\.panels' % tiles, text)) == 1
    assert len(re.findall(r'static_cast<int64_t>\(panel \+ 1\) \* p\.%s / p\.panels' % tiles, text)) == 1
    assert len(re.findall(r'\(static_cast<int64_t>\(p\.%s\) \* p\.panels \+ 7\) / 8 \* 8' % q, text)) == 1
    assert len(re.findall(r'const int L = static_cast<int>\(blockIdx\.x & 7\) \* per_xcd \+ '
                          r'static_cast<int>\(blockIdx\.x >> 3\);', text)) == 1
  return found
