"""What cmhse_gru_pool_bwd launches BESIDE the BPTT chain: the host-side rules of bwd_begin /
bwd_steps / bwd_chunk (cmhse_amd/csrc/bwd.hip) restated for one request, and the case table of
tests/test_gpu_bwd_side_shapes.py.

Beside the chain run the pooling backward, the d(input) product (launch_nt_rows_once: K cut into
segments whose partials a second launch adds in order; or launch_nt_out with float atomics into an
embedding table or a time-constant input), the attention backward's dpool += du . W_lin (the same
launcher, its reduce ADDING), the weight-gradient products over chunks of packed rows
(TnRowsLaunch: tile height, row split, accumulate) and the column sums.  Which of their arms a
request takes is decided on the host from the shapes; the results cannot show it.  This module
lets a CPU test prove that every case lands on the arm it names and that the crossovers are the
ones the sources hold (tests/test_bwd_side_shapes_cpu.py).

The `split == 1` ("own_zero") arm of launch_nt_out has no caller (no_own_zero_caller() checks
that), so the rule below does not model it."""
import os
import re

import numpy as np

from bptt_shapes import CSRC, counts_of, lens_of, tail_of  # noqa: F401  (lens_of, counts_of: for the tests)

# defaults of the knobs (gru_ws.hpp CMHSE_TUNABLES) and the constants the rule reads; checked
# against the sources by tests/test_bwd_side_shapes_cpu.py
KNOBS = dict(bwd_chunk_rows=2048, tn_rows_bm=0)
DET_SPLIT_ROWS, DET_SPLIT_MAX = 256, 12      # bwd.hip kDetSplitRows / kDetSplitMax
SEG_MIN_K = 256                              # K / 256: at least 16 chunks of 16 k per segment (both split rules)
ATOMIC_GRID_MAX, ATOMIC_MIN_K, ATOMIC_WGS = 512, 512, 768    # launch_nt_out: grid < 512 && K >= 512; ceil(768 / grid)
COLSUM_ROWS = 512                            # bwd_pool_kernels.hpp kColsumRows
TN_BM_SMALL, TN_BM_TALL = 128, 192           # tn_rows.hpp kTnRowsBmSmall / kTnRowsBmTall
ATT_BN = 256                                 # gru_ws.hpp kAttBN
BK = 16                                      # nt_core.hpp kBK: packed rows per chunk of gemm_tn_rows_kernel
TN_SPLIT_MAX, TN_SPLIT_MIN_ROWS = 8, 256     # TnRowsLaunch::launch: sp <= 8, rows / sp >= 256
TN_LIMIT_BESIDE, TN_LIMIT_LAST = 1024, 2048  # ... 64-row tile units below which a launch may be split
WG_PART_MIN_ROWS, WG_PART_MAX = 512, 4       # wg_part_floats: none below 512 rows, min(sum_T / 256, 4) parts
POOL_BWD_WAVES = 16                          # bwd_pool_kernels.hpp kPoolBwdThreads / 64


def chunks_of(counts, H, knobs=None):
  """The weight-gradient chunks of one chain in launch order: (p0, p1, tail_rows).  bwd_steps walks
  the steps last first; a chunk closes when it spans bwd_chunk_rows packed rows, and at t = 0.  The
  steps of a resident tail are one launch in front of everything, so their rows (tail_rows of them
  in this chunk) simply join whichever chunk the walk closes at or after them."""
  k = dict(KNOBS, **(knobs or {}))
  T = len(counts)
  tail = tail_of(counts, H)
  off = hi = sum(counts)
  out, tail_rows = [], 0
  for t in range(T - 1, -1, -1):
    off -= counts[t]
    if tail is not None and t >= tail[0]:
      tail_rows += counts[t]
    if t == 0 or hi - off >= k['bwd_chunk_rows']:
      out.append((off, hi, tail_rows))
      hi, tail_rows = off, 0
  return out


def _vec(K, lda, ldb):
  return K % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0


def nt_rows_once(M, N, K, lda, ldb, add):
  """launch_nt_rows_once: {'kind': 'det' (mode-3 partials + splitk_reduce_kernel, which adds to the
  old value when `add`), 'store' (plain store through c_addr) or 'acc' (mode-1 accumulate)}."""
  splits = min(K // SEG_MIN_K, DET_SPLIT_MAX)
  d = dict(M=M, N=N, K=K, vec=_vec(K, lda, ldb), n_tiles=(N + 127) // 128, row_tiles=(M + 127) // 128,
           by_k=K // SEG_MIN_K, add=bool(add))
  if M > DET_SPLIT_ROWS or splits < 2:
    d.update(kind='acc' if add else 'store', splits=1, k_seg=0, last=K)
    return d
  k_seg = ((K + splits - 1) // splits + 15) // 16 * 16
  splits = (K + k_seg - 1) // k_seg
  d.update(kind='det', splits=splits, k_seg=k_seg, last=K - (splits - 1) * k_seg)
  return d


def nt_out_atomic(M, N, K, lda, ldb):
  """launch_nt_out(..., mode 2, split = 2): float atomics into rows the caller zeroed (pre_zero),
  K split over gridDim.y when the tiles are few."""
  grid = ((N + 127) // 128) * ((M + 127) // 128)
  d = dict(kind='atomic', M=M, N=N, K=K, vec=_vec(K, lda, ldb), grid=grid, pre_zero=True, splits=1,
           k_seg=0, last=K)
  if grid < ATOMIC_GRID_MAX and K >= ATOMIC_MIN_K:
    splits = min((ATOMIC_WGS + grid - 1) // grid, K // SEG_MIN_K)
    if splits > 1:
      k_seg = ((K + splits - 1) // splits + 15) // 16 * 16
      splits = (K + k_seg - 1) // k_seg
      d.update(splits=splits, k_seg=k_seg, last=K - (splits - 1) * k_seg)
  return d


def wg_part_floats(sum_T, I, H):
  if sum_T < WG_PART_MIN_ROWS:
    return 0
  return 3 * H * (I + H + 2) * min(sum_T // SEG_MIN_K, WG_PART_MAX)


def det_split_scratch_floats(sum_T, N):
  return DET_SPLIT_MAX * min(sum_T, DET_SPLIT_ROWS) * N


def tn_rows_launch(problems, rows, accumulate, part_floats, beside, knobs=None):
  """TnRowsLaunch::launch over `rows` packed rows; problems = [(M, N)] (C is [M, N], bias [M])."""
  k = dict(KNOBS, **(knobs or {}))
  bm = k['tn_rows_bm']
  if bm not in (TN_BM_SMALL, TN_BM_TALL):
    bm = TN_BM_TALL if all(M % TN_BM_TALL == 0 for M, _ in problems) else TN_BM_SMALL
  grid = sum(((N + 127) // 128) * ((M + bm - 1) // bm) for M, N in problems)
  per_split = sum(M * N + M for M, N in problems)
  best = 1
  if part_floats > 0 and grid * (bm // 64) < (TN_LIMIT_BESIDE if beside else TN_LIMIT_LAST):
    best_cost, sp = 1e30, 1
    while sp <= TN_SPLIT_MAX and (sp == 1 or (rows // sp >= TN_SPLIT_MIN_ROWS and per_split * sp <= part_floats)):
      wgs = float(grid * sp)
      per_cu = wgs / 256.0
      busiest = float((int(wgs) + 255) // 256)
      fill = 1.0 if per_cu >= 3 else (1.15 if per_cu >= 2.0 else 1.6)
      cost = busiest / sp * fill * (1.0 + 0.03 * (sp - 1))
      if cost < best_cost - 1e-9:
        best_cost, best = cost, sp
      sp += 1
  seg, splits = 0, 1
  if best > 1:
    seg = ((rows + best - 1) // best + BK - 1) // BK * BK
    splits = (rows + seg - 1) // seg
  longest = seg if splits > 1 else rows      # rows of the longest workgroup's range
  return dict(problems=list(problems), rows=rows, bm=bm, grid=grid, per_split=per_split, best=best, seg=seg,
              splits=splits, accumulate=bool(accumulate), beside=bool(beside), part_floats=part_floats,
              chunks16=(longest + BK - 1) // BK, masked_last=rows % BK != 0,
              ragged_m=any(M % bm != 0 for M, _ in problems))


def plan(counts, I, H, pool, feed, knobs=None):
  """Everything one request launches beside its chain.  pool: 'attention' | 'maxout' | 'seq2seq' |
  'all'; feed: 'padded' (d input rows written once), 'tokens' (sums into the embedding table),
  'repeat' (sums into a time-constant input) or None (no d input)."""
  counts = list(counts)
  sum_T = sum(counts)
  part = wg_part_floats(sum_T, I, H)
  out = dict(sum_T=sum_T, I=I, H=H, pool=pool, feed=feed, chunks=[], attn=None)
  if pool == 'attention':
    lens = lens_of(counts)
    out['attn'] = dict(
        e_tiles=(H + ATT_BN - 1) // ATT_BN,
        steps_per_wave=(int(lens.max()) + POOL_BWD_WAVES - 1) // POOL_BWD_WAVES,
        dpool=nt_rows_once(sum_T, H, H, H, H, True),
        dwlin=tn_rows_launch([(H, H)], sum_T, False, part, False, knobs),
        colsum_slabs=(sum_T + COLSUM_ROWS - 1) // COLSUM_ROWS)
  for n, (p0, p1, tail_rows) in enumerate(chunks_of(counts, H, knobs)):
    ch = dict(p0=p0, p1=p1, rows=p1 - p0, tail_rows=tail_rows,
              tn=tn_rows_launch([(3 * H, I), (3 * H, H)], p1 - p0, n > 0, part, p0 > 0, knobs), dx=None)
    if feed == 'padded':
      ch['dx'] = nt_rows_once(p1 - p0, I, 3 * H, 3 * H, 3 * H, False)
    elif feed in ('tokens', 'repeat'):
      ch['dx'] = nt_out_atomic(p1 - p0, I, 3 * H, 3 * H, 3 * H)
    out['chunks'].append(ch)
  return out


def tn_launches(pl):
  return [c['tn'] for c in pl['chunks']] + ([pl['attn']['dwlin']] if pl['attn'] else [])


VOCABULARY = {
    'DetSplit dx', 'DetSplit dx short last segment', 'DetSplit dx scalar', 'DetSplit dx two row tiles',
    'DetSplit dx ragged N', 'DetSplit dx two column tiles', 'DetSplit at 256 rows', 'NoSplit at 257 rows',
    'DetSplit 12 segments', 'DetSplit capped at kDetSplitMax',
    'DetSplit dpool', 'DetSplit dpool short last segment', 'DetSplit dpool more than two segments',
    'dpool accumulate unsplit',
    'Atomic split emb', 'Atomic split repeat', 'Atomic unsplit', 'Atomic split scalar',
    'Atomic split short last segment', 'Atomic unsplit many tiles',
    'TnRows tall', 'TnRows small', 'TnRows forced tall ragged M', 'TnRows row split',
    'TnRows accumulate after split', 'TnRows one 16-row chunk', 'TnRows masked last chunk',
    'TnRows beside unsplit', 'TnRows accumulate across chunks',
    'Colsum several slabs', 'AttnBwd several steps per wave', 'AttnBwd H < 64', 'AttnBwd several energy tiles',
}

# Arms no small case can reach, with the reason (an explicit list: tests/test_bwd_side_shapes_cpu.py
# holds it to these entries).  kDetSplitMax is NOT here: H = 1112 reaches the cap (dx_split_cap).
UNREACHABLE = {
    'Atomic unsplit many tiles':
        'launch_nt_out keeps K whole from 512 tiles of 128 x 128 on: one chunk of about 22 000 packed rows at the '
        'three column tiles of I = 300 (65 000 at I <= 128); the full-size training step is the only place with them',
}


def side_tags(pl):
  """The named targets one request's side launches reach (the vocabulary of the coverage test)."""
  tags = set()
  for ch in pl['chunks']:
    dx = ch['dx']
    if dx is None:
      continue
    if dx['kind'] == 'det':
      tags.add('DetSplit dx')
      if dx['last'] < dx['k_seg']:
        tags.add('DetSplit dx short last segment')
      if not dx['vec']:
        tags.add('DetSplit dx scalar')
      if dx['row_tiles'] == 2:
        tags.add('DetSplit dx two row tiles')
      if dx['N'] % 128 != 0:
        tags.add('DetSplit dx ragged N')
      if dx['n_tiles'] == 2:
        tags.add('DetSplit dx two column tiles')
      if dx['M'] == DET_SPLIT_ROWS:
        tags.add('DetSplit at 256 rows')
      if dx['splits'] == DET_SPLIT_MAX:
        tags.add('DetSplit 12 segments')
      if dx['by_k'] > DET_SPLIT_MAX:
        tags.add('DetSplit capped at kDetSplitMax')
    elif dx['kind'] == 'store':
      if dx['M'] == DET_SPLIT_ROWS + 1 and dx['by_k'] >= 2:
        tags.add('NoSplit at 257 rows')
    elif dx['kind'] == 'atomic':
      if dx['splits'] > 1:
        tags.add('Atomic split emb' if pl['feed'] == 'tokens' else 'Atomic split repeat')
        if not dx['vec']:
          tags.add('Atomic split scalar')
        if dx['last'] < dx['k_seg']:
          tags.add('Atomic split short last segment')
      elif dx['K'] >= ATOMIC_MIN_K and dx['K'] // SEG_MIN_K >= 2:
        tags.add('Atomic unsplit many tiles')
      else:
        tags.add('Atomic unsplit')
  at = pl['attn']
  if at is not None:
    dp = at['dpool']
    if dp['kind'] == 'det':
      tags.add('DetSplit dpool')
      if dp['last'] < dp['k_seg']:
        tags.add('DetSplit dpool short last segment')
      if dp['splits'] > 2:
        tags.add('DetSplit dpool more than two segments')
    elif dp['by_k'] >= 2:
      tags.add('dpool accumulate unsplit')      # wide enough to be split, too many rows: mode-1 accumulate
    if at['colsum_slabs'] > 1:
      tags.add('Colsum several slabs')
    if at['steps_per_wave'] > 1:
      tags.add('AttnBwd several steps per wave')
    if pl['H'] < 64:
      tags.add('AttnBwd H < 64')
    if at['e_tiles'] > 1:
      tags.add('AttnBwd several energy tiles')
  for tn in tn_launches(pl):
    if tn['bm'] == TN_BM_TALL:
      tags.add('TnRows forced tall ragged M' if tn['ragged_m'] else 'TnRows tall')
    else:
      tags.add('TnRows small')
    if tn['splits'] > 1:
      tags.add('TnRows row split')
      if tn['accumulate']:
        tags.add('TnRows accumulate after split')      # tn_rows_reduce_kernel adds the parts to C
    elif tn['beside']:
      tags.add('TnRows beside unsplit')
    if tn['accumulate']:
      tags.add('TnRows accumulate across chunks')
    if tn['chunks16'] == 1:
      tags.add('TnRows one 16-row chunk')
    if tn['masked_last']:
      tags.add('TnRows masked last chunk')
  return tags


# The cases of tests/test_gpu_bwd_side_shapes.py: (id, feed, knobs, cls, I, H, profile, targets).
# `profile` is the active-sequence count of steps t = 0, 1, ... (bptt_shapes.lens_of); cls names the
# layer: Seq2Seq / Maxout / Attention (cmhse_amd.layers) or Seq2Seq_Decode (all-states pooling).
POOL_OF = {'Attention': 'attention', 'Maxout': 'maxout', 'Seq2Seq': 'seq2seq', 'Seq2Seq_Decode': 'all'}
CASES = [
    # ---- ordinary d(input), default knobs, one chunk ----
    ('dx_two_segments', 'padded', {}, 'Seq2Seq', 20, 172, (40, 40, 38, 35, 30, 17),      # 200 rows; K = 516: 272 + 244
     {'DetSplit dx', 'DetSplit dx short last segment', 'DetSplit dx two row tiles', 'DetSplit dx ragged N',
      'TnRows small'}),
    ('dx_scalar', 'padded', {}, 'Maxout', 17, 173, (30, 28, 25, 20, 15, 8),               # 126 rows; K = 519: 272 + 247
     {'DetSplit dx', 'DetSplit dx scalar', 'DetSplit dx short last segment'}),
    ('dx_256_rows', 'padded', {}, 'Seq2Seq', 130, 176, (70, 66, 62, 58),
     {'DetSplit dx', 'DetSplit at 256 rows', 'DetSplit dx two column tiles', 'DetSplit dx two row tiles'}),
    ('dx_257_rows', 'padded', {}, 'Seq2Seq', 130, 176, (70, 66, 62, 59), {'NoSplit at 257 rows'}),
    ('dx_12_segments', 'padded', {}, 'Seq2Seq', 64, 1024, (28, 26, 22, 16, 8),            # 100 rows; 12 x 256
     {'DetSplit dx', 'DetSplit 12 segments', 'TnRows tall'}),
    ('dx_split_cap', 'padded', {}, 'Seq2Seq', 64, 1112, (28, 26, 22, 16, 8),              # K = 3336: 11 x 288 + 168
     {'DetSplit dx', 'DetSplit 12 segments', 'DetSplit capped at kDetSplitMax', 'DetSplit dx short last segment'}),
    # ---- chunked: chunks of 165, 230, 300 and 520 rows; the last one row-split and added to C ----
    ('dx_chunked', 'padded', dict(bwd_chunk_rows=128), 'Maxout', 24, 256, (520, 300, 130, 100, 60, 40, 30, 20, 10, 5),
     {'DetSplit dx', 'TnRows tall', 'TnRows row split', 'TnRows accumulate after split', 'TnRows beside unsplit',
      'TnRows accumulate across chunks', 'TnRows masked last chunk'}),
    # ---- the attention backward's dpool += du . W_lin ----
    ('dpool_two_segments', 'padded', {}, 'Attention', 16, 512,                            # 188 rows, 20 steps
     (12, 12, 12, 12, 12, 12, 12, 12, 10, 10, 10, 10, 8, 8, 8, 8, 6, 6, 4, 4),
     {'DetSplit dpool', 'AttnBwd several steps per wave', 'AttnBwd several energy tiles', 'DetSplit dx'}),
    ('dpool_short_last', 'padded', {}, 'Attention', 16, 516, (60, 50, 40, 30, 20),        # K = 516: 272 + 244
     {'DetSplit dpool', 'DetSplit dpool short last segment'}),
    ('dpool_four_segments', 'padded', {}, 'Attention', 16, 1024, (50, 45, 40, 35, 30),
     {'DetSplit dpool', 'DetSplit dpool more than two segments'}),
    ('dpool_257_rows', 'padded', {}, 'Attention', 16, 512, (60, 55, 50, 48, 44), {'dpool accumulate unsplit'}),
    ('attn_h40', 'padded', {}, 'Attention', 12, 40, (9, 7, 4, 2), {'AttnBwd H < 64'}),
    ('attn_colsum_two_slabs', 'padded', {}, 'Attention', 20, 72, (130, 120, 100, 90, 73),  # 513 rows
     {'Colsum several slabs', 'TnRows row split'}),
    # ---- token-fed: sums into the embedding table ----
    ('emb_two_segments', 'tokens', {}, 'Attention', 20, 172, (40, 36, 30, 20, 10), {'Atomic split emb'}),
    ('emb_four_segments', 'tokens', {}, 'Maxout', 130, 344, (40, 36, 30, 20, 10),         # K = 1032: 3 x 272 + 216
     {'Atomic split emb', 'Atomic split short last segment'}),
    ('emb_scalar', 'tokens', {}, 'Seq2Seq', 17, 173, (40, 36, 30, 20, 10), {'Atomic split emb', 'Atomic split scalar'}),
    ('emb_unsplit', 'tokens', {}, 'Attention', 24, 64, (40, 36, 30, 20, 10), {'Atomic unsplit'}),
    # ---- a time-constant input: d rows[s] is the sum over the steps ----
    ('repeat_split', 'repeat', {}, 'Seq2Seq_Decode', 36, 176, (30, 26, 20, 12, 6), {'Atomic split repeat'}),
    # ---- one 16-row chunk on the tall tile ----
    ('tn_one_chunk_tall', 'padded', dict(tn_rows_bm=192), 'Seq2Seq', 10, 64, (3, 2),
     {'TnRows tall', 'TnRows one 16-row chunk', 'TnRows masked last chunk'}),
]
VOCAB = 50      # rows of the token-fed cases' embedding table


def case_plan(case):
  name, feed, knobs, cls, I, H, profile, _ = case
  return plan(list(profile), I, H, POOL_OF[cls], feed, knobs)


def case_tokens(rng, lens, vocab=VOCAB):
  """Token ids [S, T] of a token-fed case: few distinct ids (many repeats per table row), an id of
  -1 and one of vocab + 3 at valid steps (the kernels clamp them to rows 0 and vocab - 1)."""
  S, T = len(lens), int(max(lens))
  tok = rng.randint(0, vocab, size=(S, T)).astype(np.int64)
  tok[:, ::2] = rng.randint(0, 7, size=tok[:, ::2].shape)
  tok[0, 0] = -1
  tok[1, 1] = vocab + 3
  assert lens[0] >= 1 and lens[1] >= 2
  return tok


# tests/test_gpu_gru.py test_weight_gradient_tall_tile_vs_small_tile: (cls, pool, I, H, S, T)
TALL_TILE_CASES = [
    ('Seq2Seq', 'seq2seq', 24, 64, 37, 9),        # 3H = 192: one tall tile, N < 128
    ('Attention', 'attention', 200, 128, 150, 7),   # 3H = 384: two tall tiles; rows split into parts
    ('Maxout', 'maxout', 36, 40, 21, 5),          # 3H = 120: a tall tile forced onto a ragged M
    ('Seq2Seq', 'seq2seq', 130, 192, 300, 4),     # N = 130: a second column tile of 2; 744 rows in two parts
]
# tests/test_gpu_gru.py test_weight_gradients_in_time_chunks_beside_the_chain: (pool, cls), its shape
# (S, T, I, H) and its bwd_chunk_rows
TIME_CHUNK_CASES = [('attention', 'Attention'), ('maxout', 'Maxout')]
TIME_CHUNK_SHAPE = (330, 14, 36, 72)
TIME_CHUNK_ROWS = 1024


def tall_tile_lens(rng, S, T):
  """Lengths of a TALL_TILE_CASES entry, drawn as the test draws them (rng = RandomState(5 + H + S))."""
  lens = rng.randint(1, T + 1, size=S)
  lens[0] = T
  return lens


def time_chunk_lens(rng, S, T):
  """Lengths of the time-chunk test, drawn as the test draws them (rng = RandomState(77))."""
  lens = rng.randint(1, T + 1, size=S)
  lens[:200] = rng.randint(T - 2, T + 1, size=200)
  lens[0] = T
  return lens


# --------------------------------------------------------------------------------------------
# oracle-side helpers of the GPU test (checked against brute-force loops by the CPU test)
# --------------------------------------------------------------------------------------------
def clamp_ids(tok, vocab):
  return np.clip(np.asarray(tok, dtype=np.int64), 0, vocab - 1)


def d_table_from_dx(dx, tok, lens, vocab):
  """d table [vocab, I] = scatter-add of dx[s, t] (t < lens[s]) by the clamped id of (s, t)."""
  dx = np.asarray(dx, dtype=np.float64)
  ids = clamp_ids(tok, vocab)[:, :dx.shape[1]]
  valid = np.arange(dx.shape[1])[None, :] < np.asarray(lens)[:, None]
  out = np.zeros((vocab, dx.shape[2]), dtype=np.float64)
  np.add.at(out, ids[valid], dx[valid])
  return out


def d_rows_from_dx(dx, lens):
  """d rows [S, I] of a time-constant input = sum of dx[s, t] over the steps t < lens[s]."""
  dx = np.asarray(dx, dtype=np.float64)
  valid = np.arange(dx.shape[1])[None, :] < np.asarray(lens)[:, None]
  return (dx * valid[:, :, None]).sum(axis=1)


# --------------------------------------------------------------------------------------------
# the sources
# --------------------------------------------------------------------------------------------
def _read(name):
  return open(os.path.join(CSRC, name)).read()


def _one(pattern, text, what):
  m = re.findall(pattern, text)
  assert len(m) == 1, (what, m)
  return m[0]


def source_constants():
  """The knob defaults, constants and literals above, as the sources state them."""
  bwd, pool, tn, ws, core = (_read(n) for n in ('bwd.hip', 'bwd_pool_kernels.hpp', 'tn_rows.hpp', 'gru_ws.hpp',
                                                 'nt_core.hpp'))
  found = {}
  for name in KNOBS:
    found[name] = int(_one(r'X\(%s,\s*(-?\d+)\)' % name, ws, name))

  def const(text, name):
    return int(_one(r'\b%s\s*=\s*(\d+)\s*[,;]' % name, text, name))
  found['kDetSplitRows'], found['kDetSplitMax'] = const(bwd, 'kDetSplitRows'), const(bwd, 'kDetSplitMax')
  found['kColsumRows'] = const(pool, 'kColsumRows')
  found['kTnRowsBmSmall'], found['kTnRowsBmTall'] = const(tn, 'kTnRowsBmSmall'), const(tn, 'kTnRowsBmTall')
  found['kAttBN'] = const(ws, 'kAttBN')
  found['kBK'] = const(core, 'kBK')
  found['kPoolBwdThreads'] = const(pool, 'kPoolBwdThreads')
  # launch_nt_out: if ((own_zero || pre_zero) && grid < 512 && K >= 512) { splits = (768 + grid - 1) / grid; ... K / 256
  found['atomic_grid_max'], found['atomic_min_k'] = (
      int(v) for v in _one(r'\(own_zero \|\| pre_zero\) && grid < (\d+) && K >= (\d+)\)', bwd, 'atomic split condition'))
  found['atomic_wgs'] = int(_one(r'splits = \((\d+) \+ grid - 1\) / grid;', bwd, 'atomic split count'))
  found['atomic_seg_min_k'] = int(_one(r'max_splits = static_cast<unsigned>\(K / (\d+)\);', bwd, 'atomic segment floor'))
  # launch_nt_rows_once: int splits = K / 256; ... if (M > kDetSplitRows || splits < 2)
  found['det_seg_min_k'] = int(_one(r'int splits = K / (\d+);', bwd, 'det segment floor'))
  assert len(re.findall(r'if \(M > kDetSplitRows \|\| splits < 2\)', bwd)) == 1
  # both: segments of whole 16-k chunks
  assert len(re.findall(r'k_seg = \(\(K \+ (?:static_cast<int>\(splits\)|splits) - 1\) / '
                        r'(?:static_cast<int>\(splits\)|splits) \+ 15\) / 16 \* 16;', bwd)) == 2
  # TnRowsLaunch::launch
  found['tn_limit_beside'], found['tn_limit_last'] = (
      int(v) for v in _one(r'\(bm / 64\) < \(beside \? (\d+)u : (\d+)u\)', bwd, 'row split threshold'))
  found['tn_split_max'], found['tn_split_min_rows'] = (
      int(v) for v in _one(r'sp <= (\d+) && \(sp == 1 \|\| \(rows / sp >= (\d+) && per_split \* sp <= part_floats\)\)',
                           bwd, 'row split loop'))
  # wg_part_floats
  found['wg_part_min_rows'] = int(_one(r'if \(sum_T < (\d+)\) return 0;', bwd, 'wg_part_floats floor'))
  found['wg_part_max'] = int(_one(r'want = sum_T / 256 < (\d+) \?', bwd, 'wg_part_floats parts'))
  # chunk count of launch_colsum and the pool backward's energy tiles use the constants by name
  assert len(re.findall(r'\(rows \+ kColsumRows - 1\) / kColsumRows', bwd)) == 1
  assert len(re.findall(r'ap\.n_tiles = \(H \+ kAttBN - 1\) / kAttBN;', bwd)) == 1
  return found


def _call_args(text, pos):
  """The top-level arguments of the call whose '(' is at text[pos]."""
  depth, args, cur = 0, [], ''
  for ch in text[pos:]:
    if ch == '(':
      depth += 1
      if depth == 1:
        continue
    elif ch == ')':
      depth -= 1
      if depth == 0:
        args.append(cur.strip())
        return args
    if ch == ',' and depth == 1:
      args.append(cur.strip())
      cur = ''
    else:
      cur += ch
  raise AssertionError('unbalanced call')


def nt_out_call_sites():
  """The argument lists of every call of launch_nt_out in bwd.hip (13 parameters, the last one,
  `split`, defaulted to 0)."""
  bwd = _read('bwd.hip')
  sites = []
  for m in re.finditer(r'(?<![\w])launch_nt_out\(', bwd):
    if bwd[:m.start()].rstrip().endswith('static void'):
      continue      # the definition
    sites.append(_call_args(bwd, m.end() - 1))
  return sites


def no_own_zero_caller():
  """True when no call site of launch_nt_out passes split = 1 (the arm that zeroes a dense C itself)."""
  sites = nt_out_call_sites()
  assert len(sites) >= 3, sites
  for args in sites:
    assert len(args) in (12, 13), args
    if len(args) == 13 and args[12] not in ('0', '2'):
      return False
  return True
