"""Which kernel runs each FORWARD step: the rule of step_shape / plan_chain / launch_steps /
launch_fwd_tail / launch_hoisted_xproj (cmhse_amd/csrc/gru.hip) restated for one
cmhse_gru_pool_fwd_multi call, and the case tables of tests/test_gpu_fwd_shapes.py and of
test_gpu_chain.py's forward resident-tail test.

The step shapes are a host-side decision the GPU tests cannot see from their results; this module
lets a CPU test prove that every case lands on the shapes it names, and that the crossovers it
assumes are the ones the sources hold (tests/test_fwd_shapes_cpu.py).  The bf16x3 math mode is
restated too (`bf3=True`: which requests carry the flag, the TiledBf3 step, rows_split, and every
launch of the attention projection with its cut), with a tag vocabulary (BF3_TAGS) and a case table
(BF3_CASES) of its own for tests/test_gpu_bf3_shapes.py, proved by tests/test_bf3_shapes_cpu.py.  Not
restated: upload events (cmhse_pull_steps), prefix aliases and the halving of a chain whose launch
would exceed 2^32 threads (no case comes near them).  Taken on trust: resident_fits
(the full chip: 256 CUs hold every resident tail), the token table's workspace (ops sizes it with
cmhse_gru_pool_workspace_tok, so the gate of tok_table_rows decides), and that a training request's
companion stream exists and is not its job stream (ops.side_stream: stream_set()[0] and [1] as job
streams pair with [2] and [3]; the training cases use at most two requests).  The GPU tests cannot
see which kernel ran: these rules are the link between a case and its tags."""
import os
import re

import numpy as np

from bptt_shapes import counts_of, lens_of, tail_case_lens  # noqa: F401  (re-exported for the tests)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'cmhse_amd', 'csrc')

# defaults of the knobs the forward dispatch reads (gru_ws.hpp CMHSE_TUNABLES) and its constants;
# checked against the sources by tests/test_fwd_shapes_cpu.py
KNOBS = dict(tiny_max_seqs=1024, mid_max_seqs=1024, mid_units=0, mid_waves=0, tall_tile_min_wgs=2048,
             fwd_tail_min_steps=4, mid_tall_min_seqs=129, xproj_chunk_rows=1536, chain_min_steps=2,
             early_xproj=1, chain_tall_min_wgs=256, tok_table=1)
TINY_BM, TINY_BU = 32, 8      # gru_small_batch.hpp kTinyBM / kTinyBU
GRU_BU = 64                   # gru_step_tile.hpp kGruBU: hidden units of an LDS-tiled step's column tile
FWD_TAIL_MAX_SEQS = 32        # gru_small_batch.hpp kFwdTailMaxSeqs
CHAIN_MAX_STEPS = 96          # gru_ws.hpp kChainMaxStepsWs
CHIP_CUS = 256                # gru.hip kChipCUs (mid_units)
FWD_TAIL_KBS = (2, 4, 8)      # the gru_fwd_tail_kernel instantiations of launch_fwd_tail
XPROJ_FIRST_ROWS = 512        # gru.hip kXprojFirstRows: the chunked projection's first chunk

POOLS = ('LAST', 'MAX', 'ALL', 'ATTN')
# the kernel families and the pool modes each has an epilogue for (ATTN is pooled afterwards from hs)
FAMILY_POOLS = {'Tiny': POOLS, 'Tiled': POOLS, 'Chain': POOLS, 'Mid': POOLS, 'FwdTail': ('LAST', 'MAX', 'ALL')}

# the tag vocabulary of the coverage test
ALL_TAGS = ({'Tiny vec', 'Tiny scalar'} |
            {'%s%d %s' % (f, r, v) for f in ('Tiled', 'Chain') for r in (64, 128) for v in ('vec', 'scalar')} |
            {'Mid MB%d U%d W%d' % (mb, u, w) for mb in (1, 2) for u in (4, 8, 16) for w in (4, 8)} | {'Mid64'} |
            {'FwdTail KB%d MB%d' % (kb, mb) for kb in FWD_TAIL_KBS for mb in (1, 2)} |
            {'xproj chunked', 'xproj early', 'token table'} |
            {'%s %s' % (f, p) for f, ps in FAMILY_POOLS.items() for p in ps})
# tags no case of the tables reaches, with the reason (none at present)
UNREACHABLE = {}

# The bf16x3 math mode (call_steps(..., bf3=True)): a vocabulary of its own, beside ALL_TAGS.
ATT_BN = 256                  # gru_ws.hpp kAttBN: columns of W_lin per attention-energy workgroup
ATT_BM_BF3 = 128              # gru.hip launch_attention: tile height of the bf16x3 projection (att_bm)
BF3_FAMILY_POOLS = {'TiledBf3': POOLS}
#   TiledBf3             the 128-row ring step (gru_step_kernel<true, 2, true>), and its pool epilogues
#   Attn ring            attn_energy_kernel<true, 2, true, true>: pre-split rows [lo, cut)
#   Attn split-in-loop   attn_energy_kernel<true, 2, true, false>: fp32 rows [cut, hi), split in the loop
#   Attn fp32            the exact projection of a request of a bf16x3-mode call
#   Attn partial ring / both    a partial launch of launch_early_attention wholly below the cut / cut inside
#   Attn final both / plain     a request's last launch cut inside / behind a partial one and wholly above the cut
#   bf3 untouched        a request of a bf16x3-mode call no kernel of which is a bf16x3 one
BF3_TAGS = ({'TiledBf3'} | {'%s %s' % (f, p) for f, ps in BF3_FAMILY_POOLS.items() for p in ps} |
            {'Attn ring', 'Attn split-in-loop', 'Attn fp32', 'Attn partial ring', 'Attn partial both',
             'Attn final both', 'Attn final plain', 'bf3 untouched'})
BF3_UNREACHABLE = {}


def job(pool, profile, I, H, save=False, plan=None, vocab=0, h0=False, stream=None):
  """One request of a call: `profile` = active sequences of steps 0, 1, ... (its lengths: lens_of);
  `plan` = the step plan of the whole split it is a share of (inference only); `vocab` > 0: token-fed;
  `stream`: a label of its own stream (cmhse_gru_job.stream), None = the caller's."""
  return dict(pool=pool, counts=list(profile), I=I, H=H, save=save, plan=None if plan is None else list(plan),
              vocab=vocab, h0=h0, stream=stream)


def tail_kb(H):
  """KB of gru_fwd_tail_kernel for width H (launch_fwd_tail): 16-k blocks per wave in whole pairs."""
  kb = 2 * ((H // 16 + 15) // 16)
  return next((k for k in FWD_TAIL_KBS if kb <= k), FWD_TAIL_KBS[-1])


def mid_m_blocks(S_t):
  return 1 if S_t <= 16 else (S_t + 31) // 32


def mid_units(H, m_blocks, k):
  if k['mid_units'] in (16, 8, 4):
    return k['mid_units']
  for bu in (4, 8):
    if -(-H // bu) * m_blocks <= CHIP_CUS:
      return bu
  return 16


def gru_msub_for(wgs64, k):
  thr = k['tall_tile_min_wgs']
  return 2 if (thr > 0 and wgs64 >= thr) else 1


def _prepare(j, k, bf3=False):
  """prepare_job: vec, the kind counts, t_mid and the token table of one request; in a bf16x3-mode call
  (`bf3`) also the request's own flag and rows_split, the packed rows its TiledBf3 steps produce."""
  c = j['counts']
  T = len(c)
  j = dict(j, T=T, sum_T=sum(c))
  j['vec'] = j['I'] % 4 == 0 and j['H'] % 4 == 0
  j['kind'] = j['plan'] if (j['plan'] is not None and not j['save']) else c
  j['t_mid'] = T
  if j['vec'] and k['mid_max_seqs'] > 0:
    j['t_mid'] = next((t for t in range(T) if j['kind'][t] <= k['mid_max_seqs']), T)
  # (the mode flag of the CALL closes the table — tok_table_rows — whether or not the request runs a bf16x3 kernel)
  j['tok_tab'] = (j['vocab'] > 0 and k['tok_table'] != 0 and not j['save'] and j['vec'] and not bf3 and
                  j['sum_T'] >= 4 * j['vocab'] and j['vocab'] * 3 * j['H'] < 2 ** 31)
  j['bf3'] = bool(bf3 and not j['save'] and j['vec'] and (j['kind'][0] > k['tiny_max_seqs'] or j['pool'] == 'ATTN'))
  j['rows_split'] = 0
  if j['bf3']:
    for t in range(min(T, j['t_mid'])):
      if j['kind'][t] <= k['tiny_max_seqs']:
        break
      j['rows_split'] += c[t]
  return j


def step_shape(j, t, S_t, mid_blocks, alone, tiled_wgs, k):
  """(family, vec, rows, units, waves) of request j's step t."""
  if t >= j['t_mid']:
    if k['mid_waves'] == 4:
      alone = False
    if k['mid_waves'] == 8:
      alone = True
    bu = mid_units(j['H'], mid_blocks, k)
    tall = k['mid_tall_min_seqs']
    if tall > 0 and S_t >= tall and bu == 16 and alone and j['save']:
      return ('Mid', j['vec'], 64, 16, 8)
    return ('Mid', j['vec'], 16 if S_t <= 16 else 32, bu, 8 if alone else 4)
  if j['kind'][t] <= k['tiny_max_seqs']:
    return ('Tiny', j['vec'], TINY_BM, TINY_BU, 4)
  if j['bf3']:
    return ('TiledBf3', j['vec'], 128, GRU_BU, 4)
  return ('Tiled', j['vec'], 128 if gru_msub_for(tiled_wgs, k) == 2 else 64, GRU_BU, 4)


def xproj_chunks(counts, k):
  """launch_hoisted_xproj's chunked form: the first step of every chunk of the projection (the first
  one, in front of the chain, holds at least kXprojFirstRows packed rows; the others, on the side
  stream, at least xproj_chunk_rows)."""
  starts, row, begin, t0 = [], 0, 0, 0
  for q, c in enumerate(counts):
    row += c
    if row - begin >= (XPROJ_FIRST_ROWS if t0 == 0 else k['xproj_chunk_rows']) or q == len(counts) - 1:
      starts.append(t0)
      begin, t0 = row, q + 1
  return starts


def _tiled64_grid(H, S_t):
  return -(-H // GRU_BU) * -(-S_t // 64)


def call_steps(jobs, knobs=None, tail_stream=False, side_streams=True, bf3=False, attn=False):
  """launch_steps of one call.  `tail_stream`: the call has a side stream (ops passes one for two or
  more requests); `side_streams`: a training request gets its companion stream (ops.side_stream);
  `bf3`: the call runs in the bf16x3 math mode.  Returns, per request, a list of the launches that
  serve it: dicts with `kind` ('step', 'chain', 'tail', 'xproj'), the steps `ts` and `tag`, plus the
  pool modes its epilogue ran with; a 'step' launch also names the requests that share it (`group`).
  With `bf3`, the launches of the attention projection follow (`kind` 'attn': the rows [lo, hi), the
  `cut`, `partial`), and every list carries the request's `bf3` flag and `rows_split`; `attn` lists
  them for an exact call too (tests/long_shapes.py: a partial launch, then a final one)."""
  k = dict(KNOBS, **(knobs or {}))
  jobs = [_prepare(j, k, bf3) for j in jobs]
  n = len(jobs)
  js = ['main' if j['stream'] is None else j['stream'] for j in jobs]
  side = 'side' if (tail_stream and n > 1) else None
  forked = [False]

  def fork(m):
    if side is None or js[m] != 'main':
      return
    js[m] = side
    forked[0] = True

  out = [_Launches() for _ in jobs]
  for m, j in enumerate(jobs):
    j['tail_lo'], j['chain_until'], j['early'], j['pooled'] = -1, 0, False, False
    j['att_done'] = 0
    out[m].bf3, out[m].rows_split = j['bf3'], j['rows_split']
    if (j['save'] and k['fwd_tail_min_steps'] > 0 and j['vec'] and j['H'] % 16 == 0 and j['H'] <= 1024 and
        js[m] != 'main' and j['t_mid'] == 0):
      lo = j['T']
      while lo - 1 >= 1 and j['counts'][lo - 1] <= FWD_TAIL_MAX_SEQS:
        lo -= 1
      if j['T'] - lo >= k['fwd_tail_min_steps']:
        j['tail_lo'] = lo
    if j['tok_tab']:
      out[m].append(dict(kind='xproj', ts=[], tag='token table'))
  if side is not None and k['early_xproj'] != 0:
    for m, j in enumerate(jobs):
      if j['save'] or j['t_mid'] <= 0 or j['t_mid'] >= j['T'] or j['stream'] is not None or j['tok_tab']:
        continue
      j['early'] = True
  Tmax = max(j['T'] for j in jobs)
  for t in range(Tmax):
    live = [t < j['T'] for j in jobs]
    mid_blocks = sum(mid_m_blocks(j['counts'][t]) for m, j in enumerate(jobs)
                     if live[m] and t >= j['t_mid'] and not (0 <= j['tail_lo'] <= t))
    alone = not forked[0]
    tiled_wgs = 0
    for m, j in enumerate(jobs):
      if live[m] and t < j['t_mid']:
        alone = False
        if j['kind'][t] > k['tiny_max_seqs'] and not j['bf3']:
          tiled_wgs += _tiled64_grid(j['H'], j['counts'][t])
    shape = [step_shape(j, t, j['counts'][t], mid_blocks, alone, tiled_wgs, k) if live[m] else None
             for m, j in enumerate(jobs)]
    any_tiled = any(s is not None and s[0] in ('Tiled', 'TiledBf3') for s in shape)
    chain = _plan_chain(jobs, t, shape, live, js, tiled_wgs, k)
    done = [not x for x in live]
    for m, j in enumerate(jobs):
      if done[m]:
        continue
      if 0 <= j['tail_lo'] <= t:
        if t == j['tail_lo']:
          if any_tiled:
            fork(m)
          lo = j['tail_lo']
          out[m].append(dict(kind='tail', ts=list(range(lo, j['T'])), kb=tail_kb(j['H']),
                             mb=2 if j['counts'][lo] > 16 else 1,
                             tag='FwdTail KB%d MB%d' % (tail_kb(j['H']), 2 if j['counts'][lo] > 16 else 1)))
        done[m] = True
        continue
      if shape[m][0] not in ('Tiled', 'TiledBf3') and any_tiled:
        fork(m)
      if t == j['t_mid'] and not j['tok_tab']:
        chunked = (j['save'] and side_streams and t == 0 and k['xproj_chunk_rows'] > 0 and
                   j['sum_T'] >= 4 * k['xproj_chunk_rows'] and len(xproj_chunks(j['counts'], k)) > 1)
        if j['early']:
          out[m].append(dict(kind='xproj', ts=[], tag='xproj early'))
        elif chunked:
          out[m].append(dict(kind='xproj', ts=[], tag='xproj chunked'))
    if chain is not None:
      rows, vec = chain['rows'], chain['vec']
      for m in chain['members']:
        jobs[m]['chain_until'] = chain['end']
        out[m].append(dict(kind='chain', ts=list(range(t, chain['end'])), rows=rows,
                           tag='Chain%d %s' % (rows, 'vec' if vec else 'scalar')))
        done[m] = True
    for m, j in enumerate(jobs):
      if done[m] or t < j['chain_until']:
        continue
      fam, vec, rows, units, waves = shape[m]
      if fam == 'Mid':
        tag = 'Mid64' if rows == 64 else 'Mid MB%d U%d W%d' % (rows // 16, units, waves)
      elif fam == 'Tiny':
        tag = 'Tiny %s' % ('vec' if vec else 'scalar')
      elif fam == 'TiledBf3':
        tag = 'TiledBf3'
      else:
        tag = 'Tiled%d %s' % (rows, 'vec' if vec else 'scalar')
      # (same kernel, same stream: one launch)
      group = [q for q in range(n) if not done[q] and t >= jobs[q]['chain_until'] and shape[q] == shape[m] and
               js[q] == js[m]]
      out[m].append(dict(kind='step', ts=[t], tag=tag, shape=shape[m], group=group))
    _early_attention(jobs, t, Tmax, js, side, fork, out if (bf3 or attn) else None, k)
  if bf3 or attn:
    for m, j in enumerate(jobs):
      if j['pool'] == 'ATTN' and not j['pooled']:
        _attention(j, out[m], j['sum_T'], True, k)
  return out


class _Launches(list):
  """The launches of one request, with the request's bf16x3 flag and rows_split."""
  bf3, rows_split = False, 0


def _attention(j, launches, row_end, pool, k):
  """launch_attention: the projection of packed rows [att_done, row_end) — exact, or in bf16x3 on 128-row
  tiles when the request carries the flag and its PLAN has more rows than tiny_max_seqs: then [lo, cut)
  from the pre-split rows (ring) and [cut, hi) from the fp32 rows, cut = clamp(rows_split, lo, hi)."""
  lo, hi = j['att_done'], max(row_end, j['att_done'])
  j['att_done'] = hi
  if hi == lo:
    return
  att_bf3 = j['bf3'] and sum(j['kind']) > k['tiny_max_seqs']
  ln = dict(kind='attn', ts=[], lo=lo, hi=hi, partial=not pool, bf3=att_bf3,
            col_tiles=-(-j['H'] // ATT_BN))
  if not att_bf3:
    ln.update(tag='Attn fp32', tags={'Attn fp32'}, cut=lo, row_tiles=-(-(hi - lo) // 64))
  else:
    cut = min(max(j['rows_split'], lo), hi)
    tags = set()
    if cut > lo:
      tags.add('Attn ring')
    if hi > cut:
      tags.add('Attn split-in-loop')
    if not pool and cut > lo:
      tags.add('Attn partial both' if cut < hi else 'Attn partial ring')
    elif lo < cut < hi:
      tags.add('Attn final both')
    elif lo > 0 and cut == lo:
      tags.add('Attn final plain')
    ln.update(tag=sorted(tags)[0], tags=tags, cut=cut,
              row_tiles=(-(-(cut - lo) // ATT_BM_BF3), -(-(hi - cut) // ATT_BM_BF3)))
  launches.append(ln)


def _plan_chain(jobs, t, shape, live, js, tiled_wgs, k):
  if k['chain_min_steps'] <= 0:
    return None
  members, c_shape, c_tiles, c_stream = [], None, None, None
  for m, j in enumerate(jobs):
    if not live[m] or shape[m][0] != 'Tiled':
      continue
    if t < j['chain_until'] or j['save'] or j['tail_lo'] >= 0 or j['H'] % 32 != 0:
      return None
    tiles = -(-j['H'] // GRU_BU)
    if not members:
      c_shape, c_tiles, c_stream = shape[m], tiles, js[m]
    elif shape[m] != c_shape or tiles != c_tiles or js[m] != c_stream:
      return None
    members.append(m)
  if not members:
    return None
  tall = k['chain_tall_min_wgs'] * (4 if any(jobs[m]['I'] < jobs[m]['H'] for m in members) else 1)
  rows = 128 if (tall > 0 and tiled_wgs >= tall) else 64
  end = t + 1
  while end - t < CHAIN_MAX_STEPS:
    same = True
    for m, j in enumerate(jobs):
      tiled_next = end < j['T'] and end < j['t_mid'] and not j['bf3'] and j['kind'][end] > k['tiny_max_seqs']
      if tiled_next != (m in members):
        same = False
        break
    if not same:
      break
    end += 1
  if end - t < k['chain_min_steps']:
    return None
  return dict(members=members, rows=rows, vec=c_shape[1], end=end)


def _early_attention(jobs, t, Tmax, js, side, fork, out=None, k=None):
  """launch_early_attention's forks: an attention request on the caller's stream that ends before
  the call does moves the requests still stepping to the side stream.  With `out` (a bf16x3-mode
  call) also its launches: that request's whole projection, then the rows the other attention
  requests have produced so far (a partial launch each)."""
  for m, j in enumerate(jobs):      # (a request on a stream of its own pools there: no fork)
    if j['pool'] == 'ATTN' and not j['pooled'] and js[m] != 'main' and js[m] == j['stream'] and t == j['T'] - 1:
      j['pooled'] = True
      if out is not None:
        _attention(j, out[m], j['sum_T'], True, k)
  for m, j in enumerate(jobs):
    if (j['pooled'] or side is None or js[m] != 'main' or j['pool'] != 'ATTN' or t != j['T'] - 1 or
        t == Tmax - 1):
      continue
    others = False
    for o in range(len(jobs)):
      if o != m and t < jobs[o]['T'] - 1:
        fork(o)
        others = True
    if others:
      j['pooled'] = True
      if out is None:
        continue
      _attention(j, out[m], j['sum_T'], True, k)
      for o, jo in enumerate(jobs):
        if o == m or jo['pool'] != 'ATTN' or jo['pooled'] or t >= jo['T'] - 1 or jo['stream'] is not None:
          continue
        _attention(jo, out[o], sum(jo['counts'][:t + 1]), False, k)


def _family(tag):
  """'Tiled64 vec' -> 'Tiled', 'Mid64' / 'Mid MB2 U4 W8' -> 'Mid', 'FwdTail KB4 MB1' -> 'FwdTail'."""
  fam = tag.split(' ')[0]
  return fam if fam in BF3_FAMILY_POOLS else fam.rstrip('0123456789')


def pool_tags(j, launches):
  """'<family> <pool>' for every family whose epilogue really ran request j's pool mode: LAST on a
  step where a sequence ends, MAX on a step t >= 1 (a running maximum to compare with), ALL and
  ATTN on any step."""
  c = j['counts']
  tags = set()
  for ln in launches:
    if ln['kind'] in ('xproj', 'attn'):
      continue
    fam = _family(ln['tag'])
    for t in ln['ts']:
      ends = t == len(c) - 1 or c[t + 1] < c[t]
      ran = (j['pool'] == 'LAST' and ends) or (j['pool'] == 'MAX' and t >= 1) or j['pool'] in ('ALL', 'ATTN')
      if ran and j['pool'] in dict(FAMILY_POOLS, **BF3_FAMILY_POOLS)[fam]:
        tags.add('%s %s' % (fam, j['pool']))
  return tags


def bf3_kernels(launches):
  """Does a request of a bf16x3-mode call run a bf16x3 kernel (a TiledBf3 step, a bf16x3 projection)?"""
  return any(ln['tag'] == 'TiledBf3' or (ln['kind'] == 'attn' and ln['bf3']) for ln in launches)


def call_tags(jobs, knobs=None, tail_stream=False, bf3=False):
  """Every tag one call reaches (shapes, projections and pool epilogues of all its requests; in the
  bf16x3 mode also the attention projection's launches and the requests the mode leaves alone)."""
  tags = set()
  for j, launches in zip(jobs, call_steps(jobs, knobs, tail_stream, bf3=bf3)):
    tags |= {ln['tag'] for ln in launches} | pool_tags(j, launches)
    for ln in launches:
      tags |= ln.get('tags', set())
    if bf3 and not bf3_kernels(launches):
      tags.add('bf3 untouched')
  return tags


# The cases of tests/test_gpu_fwd_shapes.py: (id, knobs, train, tail_stream, jobs, targets).
# train: the call runs through layers.run_grouped, each request on a job stream of its own, with
# gradients; else one ops.gru_pool_fwd_multi call (tail_stream: ops passes the call a side stream).
# Profiles hold the edges: S_t at 16/17, 32/33, 64k +- 1 and 128k +- 1, length-1 sequences, a last
# step with one active sequence.
_P33 = (33, 32, 17, 16, 9, 1)
CASES = [
    # the latency-shaped step: scalar loads at default knobs (I, H odd), dwordx4 loads with the mid-size
    # kernel moved out of the way; all four pool modes in one call
    ('tiny_scalar_all_pools', {}, False, False,
     [job('LAST', (40, 33, 32, 17, 16, 1), 17, 45, h0=True), job('MAX', (33, 32, 17, 9, 2), 17, 45),
      job('ALL', (20, 16, 5, 1), 17, 45), job('ATTN', (33, 17, 16, 1), 17, 45)],
     {'Tiny scalar', 'Tiny LAST', 'Tiny MAX', 'Tiny ALL', 'Tiny ATTN'}),
    ('tiny_vec_all_pools', dict(mid_max_seqs=0), False, False,
     [job('LAST', (65, 64, 33, 32, 17, 1), 24, 72, h0=True), job('MAX', (33, 32, 16, 2), 24, 72),
      job('ALL', (17, 16, 3, 1), 24, 72), job('ATTN', (40, 33, 1), 24, 72)],
     {'Tiny vec', 'Tiny LAST', 'Tiny MAX', 'Tiny ALL', 'Tiny ATTN'}),
    # per-step LDS-tiled launches (H % 32 != 0: no chain) with 64- and 128-row tiles, vec and scalar
    ('tiled64_vec_all_pools', dict(tiny_max_seqs=8, mid_max_seqs=8), False, False,
     [job('LAST', (129, 128, 65, 64, 63, 9, 1), 36, 80, h0=True), job('MAX', (127, 64, 63, 33, 9), 36, 80),
      job('ALL', (65, 64, 17, 1), 36, 80), job('ATTN', (64, 63, 1), 36, 80)],
     {'Tiled64 vec', 'Tiled LAST', 'Tiled MAX', 'Tiled ALL', 'Tiled ATTN', 'Mid MB1 U4 W8'}),
    ('tiled128_scalar', dict(tiny_max_seqs=8, tall_tile_min_wgs=4), False, False,
     [job('MAX', (257, 256, 129, 128, 127, 9, 1), 21, 40, h0=True), job('LAST', (129, 127, 65, 1), 21, 40)],
     {'Tiled128 scalar', 'Tiled64 scalar', 'Tiny scalar'}),
    ('tiled128_vec', dict(tiny_max_seqs=8, mid_max_seqs=8, tall_tile_min_wgs=4), False, False,
     [job('ALL', (257, 255, 129, 127, 64, 9, 1), 40, 48)],
     {'Tiled128 vec', 'Tiled64 vec', 'Tiled ALL'}),
    # the step chain: 64- and 128-row tiles, vec and scalar, H % 64 == 32 (a half column tile), all four
    # pool modes; the tall-tile threshold with I >= H (at it) and with I < H (x4: below it, then at it)
    ('chain64_vec_all_pools', dict(tiny_max_seqs=8, mid_max_seqs=8), False, True,
     [job('LAST', (129, 128, 65, 64, 63, 33, 9, 1), 40, 96, h0=True), job('MAX', (127, 65, 64, 63, 40, 9), 40, 96),
      job('ALL', (100, 65, 64, 33, 9, 1), 40, 96), job('ATTN', (64, 63, 17, 16, 1), 40, 96)],
     {'Chain64 vec', 'Chain LAST', 'Chain MAX', 'Chain ALL', 'Chain ATTN', 'xproj early'}),
    # (two requests: the chain is cut where the shorter one ends, and the longer one's second chain
    # starts one 64-row workgroup below the threshold its first chain met exactly)
    ('chain_tall_threshold_i_ge_h', dict(tiny_max_seqs=8, mid_max_seqs=8, chain_tall_min_wgs=5), False, False,
     [job('LAST', (256, 255, 255, 193, 193, 129, 127, 65, 9), 64, 64, h0=True), job('MAX', (64, 33, 17), 64, 64)],
     {'Chain128 vec', 'Chain64 vec', 'Chain LAST', 'Chain MAX'}),
    ('chain_tall_threshold_i_lt_h', dict(tiny_max_seqs=8, mid_max_seqs=8, chain_tall_min_wgs=6), False, False,
     [job('MAX', (385, 385, 385, 385, 257, 129, 127, 9), 64, 160), job('LAST', (64, 63, 33), 64, 160, h0=True)],
     {'Chain128 vec', 'Chain64 vec', 'Chain MAX'}),
    ('chain_scalar', dict(tiny_max_seqs=8, chain_tall_min_wgs=4), False, False,
     [job('ALL', (257, 256, 129, 128, 63, 33, 9, 1), 30, 96, h0=True), job('ATTN', (200, 129, 127, 65, 33), 30, 96)],
     {'Chain128 scalar', 'Chain64 scalar', 'Chain ALL', 'Chain ATTN', 'Tiny scalar'}),
    # a share of a split: the whole split's counts pass 1024 (kernel kind: LDS-tiled, a chain) while
    # the share's own counts are 1 to 63; then the mid-size kernel from the plan's t_mid on
    ('split_share', {}, False, False,
     [job('LAST', (63, 40, 33, 33, 17, 5, 1), 40, 64, plan=(1500, 1400, 1100, 1025, 900, 300, 2), h0=True),
      job('MAX', (50, 33, 32, 30, 9, 2), 40, 64, plan=(1500, 1400, 1100, 1025, 1024, 7))],
     {'Chain64 vec', 'Mid MB1 U4 W8', 'Mid MB2 U4 W8'}),
    # the mid-size kernel: every unit tile x waves x row block form; H % 16 != 0 (72)
    ('mid_u4_all_pools', dict(mid_units=4, mid_waves=4), False, False,
     [job('LAST', (33, 32, 17, 16, 1), 24, 72, h0=True), job('MAX', (17, 16, 9, 2), 24, 72),
      job('ALL', (33, 17, 1), 24, 72), job('ATTN', (16, 15, 1), 24, 72)],
     {'Mid MB1 U4 W4', 'Mid MB2 U4 W4', 'Mid LAST', 'Mid MAX', 'Mid ALL', 'Mid ATTN'}),
    ('mid_u8', dict(mid_units=8), False, False,
     [job('MAX', (65, 64, 33, 17, 16, 1), 32, 200, h0=True)], {'Mid MB1 U8 W8', 'Mid MB2 U8 W8'}),
    ('mid_u8_w4', dict(mid_units=8, mid_waves=4), False, False,
     [job('LAST', (33, 32, 17, 16, 1), 32, 200)], {'Mid MB1 U8 W4', 'Mid MB2 U8 W4'}),
    ('mid_u16', dict(mid_units=16), False, False,
     [job('ALL', (129, 128, 64, 33, 17, 16, 1), 48, 200, h0=True)], {'Mid MB1 U16 W8', 'Mid MB2 U16 W8'}),
    ('mid_u16_w4', dict(mid_units=16, mid_waves=4), False, False,
     [job('LAST', (40, 33, 32, 17, 16, 1), 40, 136)], {'Mid MB1 U16 W4', 'Mid MB2 U16 W4'}),
    ('mid_u4_w8', dict(mid_units=4), False, False,
     [job('ATTN', (33, 17, 16, 1), 20, 52, h0=True)], {'Mid MB1 U4 W8', 'Mid MB2 U4 W8'}),
    # the token projection table (inference, token-fed)
    ('token_table', {}, False, False,
     [job('MAX', (40, 33, 32, 17, 16, 9, 1), 24, 64, vocab=30)], {'token table', 'Mid MB2 U4 W8'}),
    # training: the 64-sequence mid-size tile (gru_step_mid_kernel<4, 16, 8>)
    ('mid64_train', dict(mid_units=16), True, False,
     [job('LAST', (200, 193, 129, 128, 100, 33, 9), 40, 128, save=True, h0=True, stream='s0')],
     {'Mid64', 'Mid MB2 U16 W8', 'Mid LAST'}),
    # ... the projection in chunks of time steps on the side stream beside the chain; an all-states
    # request with initial states (d h0 of all-states pooling: the rows of `out`, ops._prepare_bwd)
    ('xproj_chunked_train', dict(xproj_chunk_rows=32), True, False,
     [job('ALL', (100, 97, 90, 80, 70, 65, 64, 40, 33, 17, 16, 1), 24, 72, save=True, h0=True, stream='s0')],
     {'xproj chunked', 'Mid ALL', 'Mid MB2 U4 W8', 'Mid MB1 U4 W8'}),
    # ... the resident tail waiting for every chunk that holds its rows
    ('xproj_chunked_tail_train', dict(xproj_chunk_rows=32), True, False,
     [job('LAST', (100, 97, 90, 80, 70, 65, 64, 40, 33, 32, 20, 17, 16, 9, 3, 1), 24, 64, save=True,
          stream='s0')],
     {'xproj chunked', 'FwdTail KB2 MB2', 'FwdTail LAST'}),
    # the resident tail's all-states and max epilogues, at the default knobs, two requests on two streams
    ('fwd_tail_all_train', {}, True, False,
     [job('ALL', (20, 16, 16, 9, 5, 2), 32, 48, save=True, h0=True, stream='s0'),
      job('MAX', (40, 33, 32, 17, 16, 9, 3, 1), 24, 64, save=True, stream='s1')],
     {'FwdTail KB2 MB1', 'FwdTail KB2 MB2', 'FwdTail ALL', 'FwdTail MAX'}),
]

# The cases of tests/test_gpu_bf3_shapes.py, in the format of CASES: one inference call each, under
# ops.set_math_mode('bf16x3').  Edges: S_t at 127 / 128 / 129 and 255 / 256 / 257 (the 128-row tile), a
# last tile with one valid row, length-1 sequences, H % 16 != 0 (the zeroed chunk padding of hs_s),
# H % 64 != 0, H < 64, and 1, 2, 3, 4, 5 and >= 7 chunks of 16 k in either phase of the ring.
_A = dict(tiny_max_seqs=8, mid_max_seqs=8)
_SPLIT_SHARE = next(c for c in CASES if c[0] == 'split_share')
BF3_CASES = [
    # the four epilogues of the ring step in ONE launch per step, H % 16 = 8, then the mid-size kernel
    ('bf3_all_pools', _A, False, False,
     [job('LAST', (257, 256, 129, 128, 127, 9, 1), 36, 72, h0=True), job('MAX', (255, 129, 128, 65, 33, 9, 2), 36, 72),
      job('ALL', (130, 128, 17, 1), 36, 72, h0=True), job('ATTN', (129, 127, 64, 9, 3), 36, 72)],
     {'TiledBf3', 'TiledBf3 LAST', 'TiledBf3 MAX', 'TiledBf3 ALL', 'TiledBf3 ATTN', 'Mid MB1 U4 W8', 'Attn ring',
      'Attn split-in-loop', 'Attn final both'}),
] + [
    # the ring's prologue and steady state: 1, 1, 2, 3, 4, 7 chunks in the x phase and 1, 2, 3, 4, 5, 10 in
    # the h phase (the clamped re-loads dma(1, last) and dma(2, last) at one and two chunks)
    ('bf3_ring_chunks[%d,%d]' % (I, H), _A, False, False,
     [job('LAST', (130, 129, 65, 9, 1), I, H, h0=True), job('ATTN', (129, 64, 33, 2), I, H)],
     {'TiledBf3', 'TiledBf3 LAST', 'TiledBf3 ATTN', 'Attn ring', 'Attn split-in-loop'})
    for I, H in ((4, 16), (16, 32), (20, 48), (48, 64), (64, 80), (100, 160))
] + [
    # the validation pass's widths: 128- and 64-chunk loops, 16 column tiles
    ('bf3_wide', _A, False, False, [job('MAX', (140, 129, 128, 33, 3), 2048, 1024, h0=True)],
     {'TiledBf3', 'TiledBf3 MAX'}),
    # the latency-shaped kernel reads the fp32 states a ring step wrote
    ('bf3_to_tiny', dict(tiny_max_seqs=32, mid_max_seqs=0), False, False,
     [job('MAX', (130, 129, 128, 65, 33, 32, 17, 1), 24, 64), job('LAST', (65, 64, 33, 9), 24, 64, h0=True)],
     {'TiledBf3', 'TiledBf3 MAX', 'TiledBf3 LAST', 'Tiny vec', 'Tiny MAX', 'Tiny LAST'}),
    # rows_split = 458 of 470: three ring tiles and one of 74 rows, then the fp32 rows from a row that is
    # no multiple of 128; two column tiles of the projection, the second 8 columns wide
    ('bf3_attn_cut', _A, False, False, [job('ATTN', (129, 128, 127, 65, 9, 8, 3, 1), 40, 264, h0=True)],
     {'TiledBf3', 'TiledBf3 ATTN', 'Attn ring', 'Attn split-in-loop', 'Attn final both'}),
    # bf16x3 by the pooling alone (rows_split == 0, the projection splits fp32 rows); 42 plan rows: exact
    ('bf3_attn_only', dict(tiny_max_seqs=64, mid_max_seqs=0), False, False,
     [job('ATTN', (40, 33, 17, 1), 24, 72), job('ATTN', (20, 16, 5, 1), 24, 72), job('MAX', (40, 33, 9), 24, 72)],
     {'Attn split-in-loop', 'Attn fp32', 'bf3 untouched', 'Tiny vec'}),
    # t_mid == 0: every step on the mid-size kernel, the projection in bf16x3; the LAST request carries
    # the flag and runs no bf16x3 kernel
    ('bf3_mid_only', dict(tiny_max_seqs=8), False, False,
     [job('ATTN', (65, 64, 33, 17, 16, 1), 24, 72, h0=True), job('LAST', (33, 17, 1), 24, 72)],
     {'Attn split-in-loop', 'bf3 untouched'}),
    # the partial launches of launch_early_attention: [0, 357) wholly below rows_split = 464, then
    # [357, 468) cut at 464 ...
    ('bf3_partial_a', _A, False, True,
     [job('ATTN', (64, 63, 17), 40, 96), job('ATTN', (129, 128, 100, 65, 33, 9, 3, 1), 40, 96)],
     {'TiledBf3', 'Attn partial ring', 'Attn final both', 'xproj early'}),
    # ... [0, 349) cut at rows_split = 336, then [349, 353) wholly above it
    ('bf3_partial_b', _A, False, True,
     [job('ATTN', (64, 40, 33, 20, 17, 16, 9), 40, 96), job('ATTN', (129, 100, 65, 33, 9, 8, 5, 3, 1), 40, 96)],
     {'TiledBf3', 'Attn partial both', 'Attn final plain'}),
    # split_rows_kernel's token lookup (no token projection table in this mode)
    ('bf3_tokens', _A, False, False,
     [job('MAX', (129, 128, 65, 33, 9, 1), 24, 64, vocab=30), job('LAST', (130, 64, 9), 24, 64, vocab=50, h0=True)],
     {'TiledBf3', 'TiledBf3 MAX', 'TiledBf3 LAST'}),
    # shares of a split at the default knobs: the ring step chosen by the plan while the share's own
    # tiles hold 1 to 63 rows; the projection's kind from the plan's rows
    ('bf3_split_share', {}, False, False,
     list(_SPLIT_SHARE[4]) + [job('ATTN', (40, 33, 17, 2), 40, 64, plan=(1500, 1400, 1100, 2))],
     {'TiledBf3', 'TiledBf3 LAST', 'TiledBf3 MAX', 'TiledBf3 ATTN', 'Attn ring', 'Attn split-in-loop'}),
    # a scalar-load request keeps the exact 64-row tile beside a bf16x3 one: tiled_wgs counts only its 3
    # workgroups of the 9 at step 0, below the tall-tile threshold of 4 the two together would pass
    ('bf3_beside_exact', dict(_A, tall_tile_min_wgs=4), False, False,
     [job('LAST', (129, 65, 9), 36, 72, h0=True), job('MAX', (129, 127, 65, 1), 21, 40)],
     {'TiledBf3', 'Tiled64 scalar', 'Tiny scalar', 'bf3 untouched'}),
]

# tests/test_gpu_chain.py test_forward_tail_as_one_resident_kernel: (pool, cls, H, S, n_long)
FWD_TAIL_CASES = [('attention', 'Attention', 32, 11, 13), ('maxout', 'Maxout', 48, 40, 13),
                  ('seq2seq', 'Seq2Seq', 256, 23, 13), ('attention', 'Attention', 1024, 32, 13),
                  ('maxout', 'Maxout', 64, 40, 29), ('attention', 'Attention', 1024, 32, 30),
                  ('seq2seq', 'Seq2Seq', 384, 13, 13), ('attention', 'Attention', 512, 40, 29),
                  ('seq2seq', 'Seq2Seq', 1024, 13, 13)]
FWD_TAIL_T = 37
_TAIL_POOL = {'attention': 'ATTN', 'maxout': 'MAX', 'seq2seq': 'LAST'}


def fwd_tail_case_job(pool, H, S, n_long):
  """The request of a FWD_TAIL_CASES entry, its lengths drawn as the test draws them."""
  lens = tail_case_lens(np.random.RandomState(11 + H), S, n_long, FWD_TAIL_T)
  I = 20 if H < 1024 else 64
  return job(_TAIL_POOL[pool], counts_of(lens, FWD_TAIL_T), I, H, save=True, h0=True, stream='s0')


def source_constants():
  """The knob defaults and constants above, as the sources state them."""
  ws = open(os.path.join(CSRC, 'gru_ws.hpp')).read()
  gru = open(os.path.join(CSRC, 'gru.hip')).read()
  small = open(os.path.join(CSRC, 'gru_small_batch.hpp')).read()
  tile = open(os.path.join(CSRC, 'gru_step_tile.hpp')).read()
  found = {}
  for name in KNOBS:
    m = re.findall(r'X\(%s,\s*(-?\d+)\)' % name, ws)
    assert len(m) == 1, (name, m)
    found[name] = int(m[0])

  def const(text, name):
    m = re.findall(r'\b%s\s*=\s*(\d+)\s*[,;]' % name, text)
    assert len(m) == 1, (name, m)
    return int(m[0])
  found['kTinyBM'] = const(small, 'kTinyBM')
  found['kTinyBU'] = const(small, 'kTinyBU')
  found['kFwdTailMaxSeqs'] = const(small, 'kFwdTailMaxSeqs')
  found['kGruBU'] = const(tile, 'kGruBU')
  found['kChainMaxStepsWs'] = const(ws, 'kChainMaxStepsWs')
  found['kChipCUs'] = const(gru, 'kChipCUs')
  m = re.findall(r'\bkXprojFirstRows\s*=\s*(\d+)\s*;', gru)
  assert len(m) == 1, m
  found['kXprojFirstRows'] = int(m[0])
  found['fwd_tail_kbs'] = tuple(int(v) for v in re.findall(r'FWD_TAIL_\((\d+)\)', gru))
  # the bf16x3 mode: the projection's column and row tiles, the request's flag and the projection's kind
  found['kAttBN'] = const(ws, 'kAttBN')
  m = re.findall(r'const int att_bm = att_bf3 \? (\d+) : 64 \* msub;', gru)
  assert len(m) == 1, m
  found['att_bm_bf3'] = int(m[0])
  m = re.findall(r'job->bf3 = ([^;]+);', gru)
  assert len(m) == 1, m
  found['job_bf3'] = ' '.join(m[0].split())
  m = re.findall(r'if \(jobs\[k\]\.kind_count\[t\] > tiny_max_seqs\(\)([^)]*)\)\s*\n\s*tiled_wgs \+=', gru)
  assert len(m) == 1, m
  found['tiled_wgs_also'] = m[0].strip()      # what else a request needs to count towards tiled_wgs
  m = re.findall(r'const bool att_bf3 = ([^;]+);', gru)
  assert len(m) == 1, m
  found['att_bf3'] = ' '.join(m[0].split())
  return found


# the expressions the restatement of the bf16x3 mode assumes (source_constants()['job_bf3'], ['att_bf3'])
JOB_BF3_EXPR = ('bf3 && !save && job->vec && (job->kind_count[0] > tiny_max_seqs() || '
                'pool_mode == CMHSE_POOL_ATTN)')
ATT_BF3_EXPR = 'job.bf3 && plan_rows > tiny_max_seqs()'
TILED_WGS_ALSO = '&& !jobs[k].bf3'
