"""Long sequences through every per-step loop: the few rules that change behaviour only at lengths
the other shape suites never reach, restated, and the case tables of tests/test_gpu_long_shapes.py.

The dispatch itself is NOT restated here: fwd_shapes.call_steps (forward launches, the chain's cuts,
the resident forward tail, the token table, the exact attention projection's partial and final
launches), bptt_shapes.tail_of / step_shapes (the BPTT chain and its resident tail) and
bwd_side_shapes.plan (weight-gradient chunks, column-sum slabs) decide where a case lands.  New here
are the trip counts of the loops inside attn_pool_kernel (gru_attention.hpp) and attn_pool_bwd_kernel
(bwd_pool_kernels.hpp), which depend on a sequence's length and on H alone:

  attn_pool_rounds(len)        t0 rounds of the weighted sum (and trips of its denominator loop):
                               weights and packed row numbers are staged kThreads steps at a time
  attn_pool_unit_rounds(H)     ub rounds of the output loop: 4 kThreads units per round
  attn_bwd_steps_per_wave(len) steps the busiest of the backward's 16 waves takes, round-robin
  attn_bwd_den_trips(len)      trips of the backward's denominator loop (kPoolBwdThreads steps each)
  energy_tiles(H)              column tiles of the attention projection and the width of the last

tests/test_long_shapes_cpu.py proves that every case reaches exactly the tags it names, that the
constants are the ones the sources hold, and that the loops are still written the way the rules read
them.  Taken on trust: the pooling kernel's 16-byte alignment test (torch allocations are aligned, so
`vec` there is H % 4 == 0), and everything the three modules above take on trust.

A training call has at most two requests: ops.stream_set pairs two job streams with two companion
streams, so the four layers of `train_long_tails` run as two calls (`_a`, `_b`)."""
import os
import re

import numpy as np

import bptt_shapes
import bwd_side_shapes
import fwd_shapes
from bptt_shapes import CSRC, counts_of, lens_of  # noqa: F401  (re-exported for the tests)
from fwd_shapes import job

THREADS = 256                 # nt_core.hpp kThreads: attn_pool_kernel's workgroup
POOL_BWD_THREADS = 1024       # bwd_pool_kernels.hpp kPoolBwdThreads
POOL_BWD_WAVES = POOL_BWD_THREADS // 64
CHAIN_MAX_STEPS = fwd_shapes.CHAIN_MAX_STEPS
ATT_BN = fwd_shapes.ATT_BN
COLSUM_ROWS = bwd_side_shapes.COLSUM_ROWS
TAIL_MAX_WIDTH = 1024         # gru.hip launch_steps / bwd.hip bwd_tail: no resident tail above this H
LONG = 500                    # "long": what the tags ending in `500` count

_ORACLE_POOL = {'ATTN': 'attention', 'MAX': 'maxout', 'LAST': 'seq2seq', 'ALL': 'all'}


def _ceil(a, b):
  return -(-a // b)


def attn_pool_rounds(n):
  return _ceil(n, THREADS)


def attn_pool_unit_rounds(H):
  return _ceil(H, 4 * THREADS)


def attn_bwd_steps_per_wave(n):
  return _ceil(n, POOL_BWD_WAVES)


def attn_bwd_den_trips(n):
  return _ceil(n, POOL_BWD_THREADS)


def energy_tiles(H):
  """(column tiles of the attention projection, columns of the last one)."""
  n = _ceil(H, ATT_BN)
  return n, H - (n - 1) * ATT_BN


# the tag vocabulary of the coverage test; every tag is reached by a case
VOCABULARY = {
    'AttnPool 2 rounds', 'AttnPool 3 rounds', 'AttnPool round boundary',
    'AttnPool 2 unit rounds vec', 'AttnPool 2 unit rounds scalar',
    'AttnPool alias past 256', 'AttnPool alias full length',
    'Attn exact partial then final',
    'Chain resumed 3 times',
    'FwdTail 500 steps', 'BwdTail 500 steps',
    'per-step 500 fwd', 'per-step 500 bwd',
    'AttnBwd 33 steps per wave', 'AttnBwd 2 denominator trips',
    'wgrad 2+ chunks with tail rows', 'colsum 3+ slabs', 'xproj 3+ chunks',
    'tails refused by width fwd', 'tails refused by width bwd',
    'token table long',
}
UNREACHABLE = {}


def _launches(case):
  name, knobs, train, tail_stream, jobs, _ = case
  return fwd_shapes.call_steps(jobs, knobs, tail_stream, attn=True)


def chain_launches(case):
  """Per request of a case: the step count of every launch of the step chain that serves it."""
  return [[len(ln['ts']) for ln in lns if ln['kind'] == 'chain'] for lns in _launches(case)]


def fwd_tail_of(case, m, H=None):
  """The steps of request m's resident forward tail ([] = none); `H`: as if it had this width."""
  name, knobs, train, tail_stream, jobs, _ = case
  if H is not None:
    jobs = [dict(j, H=H) if q == m else j for q, j in enumerate(jobs)]
  lns = fwd_shapes.call_steps(jobs, knobs, tail_stream, attn=True)[m]
  return next((ln['ts'] for ln in lns if ln['kind'] == 'tail'), [])


def bwd_tail_of(case, m, H=None):
  """(t_lo, KB, MB) of request m's resident BPTT tail, or None; `H`: as if it had this width."""
  name, knobs, train, tail_stream, jobs, _ = case
  j = jobs[m]
  return bptt_shapes.tail_of(j['counts'], j['H'] if H is None else H,
                             {k: v for k, v in knobs.items() if k in bptt_shapes.KNOBS})


def bwd_plan(case, m):
  name, knobs, train, tail_stream, jobs, _ = case
  j = jobs[m]
  return bwd_side_shapes.plan(j['counts'], j['I'], j['H'], _ORACLE_POOL[j['pool']], 'padded',
                              {k: v for k, v in knobs.items() if k in bwd_side_shapes.KNOBS})


def case_tags(case):
  """Every tag of VOCABULARY one case reaches."""
  name, knobs, train, tail_stream, jobs, _ = case
  tags = set()
  k = dict(fwd_shapes.KNOBS, **knobs)
  for m, (j, lns) in enumerate(zip(jobs, _launches(case))):
    lens = [int(l) for l in lens_of(j['counts'])]
    H, T = j['H'], len(j['counts'])
    if j['pool'] == 'ATTN':
      pooled = lens + [n for _, n in j.get('aliases', ())]
      rounds = [attn_pool_rounds(n) for n in pooled]
      if 2 in rounds:
        tags.add('AttnPool 2 rounds')
      if max(rounds) >= 3:
        tags.add('AttnPool 3 rounds')
      if {THREADS - 1, THREADS, THREADS + 1} <= set(lens):
        tags.add('AttnPool round boundary')
      if attn_pool_unit_rounds(H) == 2 and max(rounds) >= 2:
        tags.add('AttnPool 2 unit rounds %s' % ('vec' if H % 4 == 0 else 'scalar'))
      for src, n in j.get('aliases', ()):
        assert 1 <= n <= lens[src], (name, src, n)
        if THREADS < n < lens[src]:
          tags.add('AttnPool alias past 256')
        if n == lens[src] and n > THREADS:
          tags.add('AttnPool alias full length')
      attn = [ln for ln in lns if ln['kind'] == 'attn']
      if (len(attn) == 2 and not attn[0]['bf3'] and attn[0]['partial'] and attn[0]['hi'] > attn[0]['lo'] == 0 and
          not attn[1]['partial'] and attn[1]['lo'] == attn[0]['hi'] < attn[1]['hi'] == sum(j['counts'])):
        tags.add('Attn exact partial then final')
    if len([ln for ln in lns if ln['kind'] == 'chain']) >= 4:
      tags.add('Chain resumed 3 times')
    if any(ln['tag'] == 'token table' for ln in lns) and T >= LONG:
      tags.add('token table long')
    if any(ln['kind'] == 'tail' and len(ln['ts']) >= LONG for ln in lns):
      tags.add('FwdTail 500 steps')
    if not train:
      continue
    assert j['save'] and j['stream'] is not None, name
    if not fwd_tail_of(case, m):
      if len([ln for ln in lns if ln['kind'] == 'step']) >= LONG:
        tags.add('per-step 500 fwd')
      if H > TAIL_MAX_WIDTH and fwd_tail_of(case, m, TAIL_MAX_WIDTH):
        tags.add('tails refused by width fwd')
    if any(ln['tag'] == 'xproj chunked' for ln in lns) and len(fwd_shapes.xproj_chunks(j['counts'], k)) >= 3:
      tags.add('xproj 3+ chunks')
    tail = bwd_tail_of(case, m)
    if tail is not None and T - tail[0] >= LONG:
      tags.add('BwdTail 500 steps')
    if tail is None:
      steps = bptt_shapes.step_shapes(j['counts'], H, j['h0'],
                                      {q: v for q, v in knobs.items() if q in bptt_shapes.KNOBS})
      if len(steps) >= LONG:
        tags.add('per-step 500 bwd')
      if H > TAIL_MAX_WIDTH and bwd_tail_of(case, m, TAIL_MAX_WIDTH) is not None:
        tags.add('tails refused by width bwd')
    pl = bwd_plan(case, m)
    if len(pl['chunks']) >= 2 and any(c['tail_rows'] > 0 for c in pl['chunks']):
      tags.add('wgrad 2+ chunks with tail rows')
    if pl['attn'] is not None:
      if pl['attn']['colsum_slabs'] >= 3:
        tags.add('colsum 3+ slabs')
      if attn_bwd_steps_per_wave(max(lens)) >= 33:
        tags.add('AttnBwd 33 steps per wave')
      if attn_bwd_den_trips(max(lens)) == 2:
        tags.add('AttnBwd 2 denominator trips')
  return tags


def _j(pool, lens, I, H, **kw):
  return job(pool, counts_of(lens), I, H, **kw)


def _aliased(j, aliases):
  """A request with prefix aliases (src, len): extra output rows behind its S own ones."""
  return dict(j, aliases=tuple(aliases))


def _t(pool, lens, I, H, stream, h0=False):
  return _j(pool, lens, I, H, save=True, h0=h0, stream=stream)


_LONG8 = (513, 400, 300, 257, 256, 40, 9, 3)
_A = dict(tiny_max_seqs=8, mid_max_seqs=8)
# chain_cuts: 40 attention-pooled sequences — 20 of 300 steps, two that run on to 330, three each ending
# at 1, 9, 95, 96, 97 and 193; a max-pooled request of 24 sequences, 12 of them 200 steps long
_CUT_ATTN = (300,) * 20 + (330,) * 2 + tuple(n for n in (1, 9, 95, 96, 97, 193) for _ in range(3))
_CUT_MAX = (200,) * 12 + (3,) * 4 + (50,) * 4 + (130,) * 4

# The cases, in fwd_shapes.CASES' format: (id, knobs, train, tail_stream, jobs, targets).
CASES = [
    # ---- inference: one ops.gru_pool_fwd_multi call each ----
    ('pool_rounds', {}, False, True,
     [_j('ATTN', (513, 512, 257, 256, 255, 3, 1), 20, 72, vocab=60), _j('ATTN', (300, 257, 2), 20, 72),
      _j('MAX', (513, 1), 20, 72), _j('ALL', (260, 5), 20, 72, h0=True)],
     {'AttnPool 2 rounds', 'AttnPool 3 rounds', 'AttnPool round boundary', 'Attn exact partial then final',
      'token table long'}),
    # five energy tiles, the last 16 (6) columns wide, and a second round of output units
    ('pool_wide_vec', {}, False, False,
     [_j('ATTN', (260, 257, 9, 1), 12, 1040), _j('LAST', (9, 4, 1), 12, 1040)],
     {'AttnPool 2 rounds', 'AttnPool 2 unit rounds vec'}),
    ('pool_wide_scalar', {}, False, False,
     [_j('ATTN', (260, 257, 9, 1), 10, 1030), _j('LAST', (9, 4, 1), 10, 1030)],
     {'AttnPool 2 rounds', 'AttnPool 2 unit rounds scalar'}),
    # the step chain cut at 96 steps three times and once by a request that ends, then latency-shaped steps
    ('chain_cuts', _A, False, True, [_j('ATTN', _CUT_ATTN, 40, 96), _j('MAX', _CUT_MAX, 40, 96)],
     {'AttnPool 2 rounds', 'Chain resumed 3 times'}),
    ('aliases_long', {}, False, False,
     [_aliased(_j('ATTN', (513, 300, 40), 20, 72, vocab=60), ((0, 257), (0, 513), (1, 256), (2, 1)))],
     {'AttnPool 2 rounds', 'AttnPool 3 rounds', 'AttnPool alias past 256', 'AttnPool alias full length',
      'token table long'}),
    # ---- training: layers.run_grouped, each request on a stream of its own ----
    ('train_long_tails_a', {}, True, False,
     [_t('ATTN', _LONG8, 20, 64, 's0'), _t('MAX', (513, 2), 20, 48, 's1')],
     {'AttnPool 2 rounds', 'AttnPool 3 rounds', 'FwdTail 500 steps', 'BwdTail 500 steps',
      'AttnBwd 33 steps per wave', 'colsum 3+ slabs'}),
    ('train_long_tails_b', {}, True, False,
     [_t('LAST', (400, 1), 20, 64, 's0', h0=True), _t('ALL', (260, 5), 20, 64, 's1', h0=True)],
     set()),
    # H % 16 != 0: the library refuses both tails, 513 launches each way; I % 4 != 0: scalar loads
    ('train_long_per_step', {}, True, False,
     [_t('ATTN', _LONG8, 10, 72, 's0'), _t('MAX', (513, 2), 10, 72, 's1')],
     {'AttnPool 2 rounds', 'AttnPool 3 rounds', 'per-step 500 fwd', 'per-step 500 bwd',
      'AttnBwd 33 steps per wave', 'colsum 3+ slabs'}),
    # 2052 packed rows in three sequences: two weight-gradient chunks (2049 + 3 rows), the projection in
    # eight chunks (xproj_chunk_rows 256: the default 1536 needs 6144 rows), a tail of 1024 steps each way
    ('train_attn_1025', dict(xproj_chunk_rows=256), True, False,
     [_t('ATTN', (1025, 1024, 3), 8, 32, 's0')],
     {'AttnPool 3 rounds', 'FwdTail 500 steps', 'BwdTail 500 steps', 'AttnBwd 33 steps per wave',
      'AttnBwd 2 denominator trips', 'wgrad 2+ chunks with tail rows', 'colsum 3+ slabs', 'xproj 3+ chunks'}),
    ('train_wide', {}, True, False,
     [_t('ATTN', (20, 9, 1), 12, 1040, 's0'), _t('MAX', (20, 9, 1), 12, 1040, 's1')],
     {'tails refused by width fwd', 'tails refused by width bwd'}),
]
TAIL_CASES = ('train_long_tails_a', 'train_attn_1025')            # a resident tail of 500 steps and more, both ways
NO_TAIL_CASES = ('train_long_per_step', 'train_wide')
VOCAB_ROWS = 60


def case(name):
  return next(c for c in CASES if c[0] == name)


# --------------------------------------------------------------------------------------------
# the validation pass with an outlier paragraph (tests/test_gpu_long_shapes.py, item "end to end")
# --------------------------------------------------------------------------------------------
OUTLIER_BATCH = 5       # loader batch: the outlier shares its batch with four small videos
OUTLIER_SEED = 3        # make_batches seed; the CPU test proves the oracle's ranks are robust under it
RANK_EPS = 1e-5         # _robust_rank_rows margin
RANK_LEFT_OUT_MAX = 1   # rows of the 9 a direction may leave out


def outlier_spec():
  """9 videos: one of 25 sentences x 21 words (a 525-word paragraph) and 300 frames, eight small
  ones with items of length 1 in every list."""
  from cmhse_amd import synthetic
  num_clips = [25, 1, 2, 3, 1, 4, 2, 1, 3]
  frames_per_video = [300, 1, 7, 12, 3, 9, 5, 2, 11]
  words = [21] * 25 + [1] + [3, 5] + [2, 7, 4] + [6] + [1, 4, 2, 5] + [7, 3] + [2] + [5, 1, 6]
  frames = [(3 * q) % 9 + 1 for q in range(25)] + [1] + [4, 2] + [9, 1, 5] + [3] + [2, 8, 1, 6] + [5, 7] + [1] + [6, 3, 2]
  assert len(words) == len(frames) == sum(num_clips) and sum(words[:25]) == 525
  return synthetic.SplitSpec(num_clips, frames, frames_per_video, words)


def outlier_batches(img_dim, vocab):
  from cmhse_amd import synthetic
  return synthetic.make_batches(outlier_spec(), OUTLIER_BATCH, img_dim, vocab, seed=OUTLIER_SEED)


def robust_rows(want):
  """Per direction (i2t, t2i) of an oracle result: (float64 ranks, float64 top-1, the rows kept)."""
  from gpu_common import _robust_rank_rows
  v, p = np.asarray(want[0], dtype=np.float64), np.asarray(want[1], dtype=np.float64)
  out = []
  for q, g in ((v, p), (p, v)):
    ranks, ok, d = _robust_rank_rows(q, g, RANK_EPS)
    out.append((ranks, d.argmax(1), ok))
  return out


# --------------------------------------------------------------------------------------------
# the sources
# --------------------------------------------------------------------------------------------
# the loops the rules above read, as written in the sources (each exactly once unless a count is given)
LOOPS = {
    'gru_attention.hpp': [('for (int t = tid; t < len; t += kThreads) {', 1),
                          ('for (int ub = 0; ub < H; ub += 4 * kThreads) {', 1),
                          ('for (int t0 = 0; t0 < len; t0 += kThreads) {', 1)],
    'bwd_pool_kernels.hpp': [('for (int t = tid; t < len; t += NT) part += expf(energy(t));', 1),
                             ('const int used = len < NT ? len : NT;', 1),
                             ('for (int t = wave; t < len; t += NW) {', 2),
                             ('constexpr int NT = kPoolBwdThreads, NW = NT / 64;', 1),
                             ('for (int i = 0; i < slabs; ++i) s += part[static_cast<int64_t>(i) * cols + c];', 1)],
    'gru.hip': [('b->H % 16 != 0 || b->H > 1024 ||', 1), ('hipLaunchKernelGGL(attn_pool_kernel, dim3(static_cast<unsigned>(b->S) + '
                                                        'static_cast<unsigned>(b->n_alias)),\n                     dim3(kThreads)', 1)],
    'bwd.hip': [('H % 16 != 0 || H > 1024 ||', 1),
                ('hipLaunchKernelGGL(attn_pool_bwd_kernel, dim3(S), dim3(kPoolBwdThreads), 0, st, ap);', 1)],
}


def source_constants():
  def read(n):
    return open(os.path.join(CSRC, n)).read()

  def const(text, name):
    m = re.findall(r'\b%s\s*=\s*(\d+)\s*[,;]' % name, text)
    assert len(m) == 1, (name, m)
    return int(m[0])
  found = dict(kThreads=const(read('nt_core.hpp'), 'kThreads'),
               kPoolBwdThreads=const(read('bwd_pool_kernels.hpp'), 'kPoolBwdThreads'),
               kChainMaxStepsWs=const(read('gru_ws.hpp'), 'kChainMaxStepsWs'),
               kAttBN=const(read('gru_ws.hpp'), 'kAttBN'),
               kColsumRows=const(read('bwd_pool_kernels.hpp'), 'kColsumRows'))
  found['loops'] = {(f, text): read(f).count(text) for f, loops in LOOPS.items() for text, _ in loops}
  return found
