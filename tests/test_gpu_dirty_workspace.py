"""Every workspace-taking entry point on dirty workspaces and dirty outputs.

The float64 oracle tests establish that the numbers are right in a clean buffer; this file establishes
that they do not depend on the buffer.  Each case runs four times through tests/dirty_alloc.py — every
workspace and every output of every wrapper call starts as 0x00 ('zero'), 0xFF ('ones'), 0xA5 ('a5') or
the bytes a larger call of the same family left behind ('stale', the arena-reuse state).  After every
run the 256 guard bytes on both sides of every buffer are intact and cmhse_async_status(0) is 0.  The
'zero' run is held to the independent reference under the existing bar (the float64 oracle with
assert_emb_close / grad_close for the GRU paths; int64 NumPy on lattice rows, bit for bit, for the scoring
calls); every output of the three dirty runs is torch.equal to the 'zero' run — diagnostics (`resolved`),
the float64 lists, every gradient and what the forward saved (hs, gates, argmax, v) included.

Exempt from the bit comparison, because float atomics sum them in an order that changes from run to run
(tests/test_gpu_pipeline.py test_train_step_on_a_packed_batch_is_bit_identical documents both): the
gradient of an embedding table (`d_src` of the token-fed case) and the gradient of a decoder's
time-constant input (`d_src` of the 'repeat' case).  They are held to the oracle under grad_close in all
four runs.  The train_emb step holds every gradient to the oracle under 'ones' and, against a twin model on
zeroed buffers, every gradient but the word table's bit for bit.  Nothing else is exempt.

The tables: FWD_CASES, TRAIN_CASES, SIDE_CASES (the formats of fwd_shapes.CASES and bwd_side_shapes.CASES)
and the SCORE shapes; tests/test_dirty_alloc_cpu.py proves from the restated dispatch rules which regions
and arms they reach.  Stale images come from STALE_FWD / STALE_TRAIN / STALE_SIDE / the STALE_SCORE shapes:
larger calls of the same family that are recorded, not checked.

Audit (read before the first GPU run): who initialises what, on which stream, and who reads it
----------------------------------------------------------------------------------------------
`st` = the stream of the call or of the request's chain; `side` = its companion stream, forked from st
(stream_after) behind the initialisations listed and joined back before the call returns.

GruWs (gru_ws.hpp), forward
  hs           step kernels write every packed row before a later step / the pooling reads it       st
  e_part       attn_energy_kernel writes every (column tile, row); attn pooling reads               st
  gates, v     training steps / attention pooling write every row; cmhse_gru_pool_bwd reads         st
  argmax       max-pooling epilogue writes every (sequence, unit) at its step 0; bwd reads          st
  wih_s whh_s wlin_s   launch_split writes whole padded rows (zero chunk padding) in prepare_job    call stream
  xs, h0_s     split_rows_kernel writes rows [0, rows_split) / [0, S) incl. chunk padding           call stream
  hs_s         hipMemsetAsync of rows [0, rows_split) when H % 16 != 0 (gru.hip prepare_job), then
               the ring step's epilogue writes the (hi, lo) pairs; next step and projection read   call stream -> st
  gx           launch_hoisted_xproj writes the rows of the steps >= t_mid before they are read      st or side (event)
  tail_sync    hipMemsetAsync 256 B on the request's stream in front of gru_fwd_tail_kernel         st
  chain_sync   hipMemsetAsync of tickets, abort word and done[] on the chain's stream in front of
               EVERY gru_step_chain_kernel launch (launch_chain)                                    chain stream
  tok_tab      launch_tok_table writes all vocab rows in front of the request's first step          st
BwdWs (bwd.hip)
  dgx, dgh     every BPTT step writes its rows before the weight-gradient chunk that reads them     st -> side (event)
  dpool        LAST / MAX: hipMemsetAsync then pool_scatter_bwd_kernel; ALL: scatter writes every
               row; ATTN: attn_pool_bwd_kernel writes every row, the W_lin product adds             st
  carry        hipMemsetAsync S * H floats in bwd_begin — redundant: every step writes the rows of
               its active sequences and reads only rows m < S_next, which the step before it wrote  st
  whh_t wih_t wlin_t   launch_transpose writes all of it; st waits for whh_t's event                side / st
  du, de       attention backward writes every row before the products read                         st
  xaddr hpaddr hsaddr p_t   row_addr_kernel writes all sum_T entries on `side`, which was forked
               behind the zero_row memset; every reader (TnRowsLaunch) runs on `side` behind it     side
  dxaddr       second row_addr_kernel on `side`; readers (launch_nt_out / nt_rows_once) on `side`   side
  zero_row, tail_sync   ONE hipMemsetAsync over both, first thing in bwd_begin; gru_bwd_tail_kernel
               runs on st behind it                                                                 st
  colsum, dx_part, wg_part, rec_part   partials: written by the producing launch, read by the
               reduce launch queued right behind it on the same stream                              st / side
  outputs      dW, db: first chunk stores, later chunks accumulate (TnRowsLaunch accumulate flag);
               dx rows written once; dh0 written by the t = -1 step; the two scatter outputs
               (d table, d time-constant rows) are zeroed by the CALLER (layers._bwd_request uses
               torch.zeros — part of the contract, cmhse_hip.h) and summed with float atomics
Scoring (sim.hip, topk.hip, group.hip)
  sim_rank / labelled      rank, top1key (and thrkey): hipMemsetAsync; diag / thresholds written by
                           sim_kernel<kSimDiag> / label_decode_kernel; top1, best_pos, score by finalize
  sim_rank_exact / labelled_exact   rank_lo, rank_hi (ties), resolved, top1key zeroed by (label_)exact_pre_kernel,
                           which also writes s64_diag and norm_a; norm_b_max: hipMemsetAsync then atomicMax;
                           tol by exact_tol_kernel; pair64, thr64, thr32, at_thr by pair_exact / reduce
  sim_topk                 every (panel, row) list written whole by topk_select_kernel; merge reads
  sim_topk_exact           keys32 / scores32 / index32 by the nested cmhse_sim_topk; norm_b_max memset;
                           bits, cols, count written whole per (panel, row) by the select kernel
  group_rank(_exact)       G by group_sim_kernel (every block); per-tile partial counts and keys written
                           whole by group_rank(_exact)_kernel; norm_max: hipMemsetAsync of 2 words; d64,
                           tolerances, norms written per group / row
  group_topk               as sim_topk
All on the caller's stream, in order.

Sync words, address tables, cross-stream initialisations — read, not tried:
  chain tickets / done[] / abort word: zeroed per launch on the launch's own stream (gru.hip launch_chain);
  tail_sync (forward): zeroed on the job stream the tail kernel runs on; tail_sync (backward): zeroed with
  zero_row on st before gru_bwd_tail_kernel on st.  No resident kernel can meet a stale counter.
  xaddr / hpaddr / dxaddr / hsaddr: written in full by row_addr_kernel on the stream that reads them.
  Initialisations on another stream than the consumer's: prepare_job's bf16x3 splits and the hs_s memset
  run on the call's stream and the job streams are forked behind it (stream_after in launch_steps); whh_t
  on `side` is handed to st by an event.  The reading found nothing to fix.

Not reachable, so not covered: the `own_zero` arm of launch_nt_out (bwd.hip, `split == 1`) has no caller
(bwd_side_shapes.no_own_zero_caller); its hipMemsetAsync cannot run."""
import numpy as np
import pytest
import torch

from conftest import EMB_TOL, GOLDEN_TOL, assert_emb_close, load_golden
from gpu_common import _blas_threads, _check_train_step_vs_oracle, golden_model, golden_opt, grad_close

import bptt_shapes
import bwd_side_shapes as bss
import fwd_shapes
import score_shapes as ss
from dirty_alloc import BYTE, dirty, stale
from fwd_shapes import job

pytestmark = pytest.mark.gpu

FILLS = ('zero', 'ones', 'a5', 'stale')

# ---------------------------------------------------------------------------------------------
# the case tables (no GPU needed to import them: tests/test_dirty_alloc_cpu.py reads them)
# ---------------------------------------------------------------------------------------------
_TILED = dict(tiny_max_seqs=8, mid_max_seqs=8)
# Forward, inference: (id, knobs, train, tail_stream, jobs, bf3) — one ops.gru_pool_fwd_multi call each.
FWD_CASES = [
    # four requests, one per pool mode, with a tail stream: the latency-shaped step (I = 17: scalar loads),
    # the mid-size step with its hoisted projection (gx) on the side stream, prefix aliases on the
    # attention request
    ('tiny_mid_all_pools', {}, False, True,
     [job('LAST', (33, 32, 17, 16, 1), 24, 72, h0=True), job('MAX', (33, 17, 9, 2), 17, 36),
      job('ALL', (20, 16, 5, 1), 24, 72),
      dict(job('ATTN', (33, 17, 16, 1), 24, 72), aliases=((0, 2), (1, 1), (2, 3)))], False),
    # per-step LDS-tiled launches (H % 32 != 0: no chain), then the mid-size step
    ('tiled', _TILED, False, False,
     [job('MAX', (129, 65, 64, 33, 9, 1), 36, 72, h0=True), job('ALL', (65, 64, 17, 1), 36, 72)], False),
    # the step chain, cut into two launches where the shorter request ends; the hoisted projection early
    ('chain_two_launches', _TILED, False, True,
     [job('LAST', (129, 128, 65, 64, 63, 33, 9, 1), 24, 128, h0=True), job('ATTN', (127, 65, 9), 24, 128)], False),
    # the token projection table
    ('token_table', {}, False, False, [job('MAX', (40, 33, 32, 17, 16, 9, 1), 24, 72, vocab=30)], False),
    # bf16x3: H % 16 != 0 and I % 16 != 0 (zeroed chunk padding), caller h0, the attention projection cut
    ('bf3_h36_i20', _TILED, False, False,
     [job('LAST', (130, 129, 65, 9, 1), 20, 36, h0=True), job('ATTN', (129, 64, 33, 2), 20, 36)], True),
]
STALE_FWD = ('stale_fwd', _TILED, False, True,
             [job('LAST', (300, 257, 129, 65, 33, 17, 9, 5, 3, 2, 1, 1), 40, 128, h0=True),
              job('ATTN', (200, 129, 64, 9, 1), 40, 128), job('MAX', (150, 100, 50, 9), 24, 72),
              job('ALL', (100, 50, 9, 1), 24, 72)], False)

# Training through layers.run_grouped, every request on a job stream of its own with its companion
# stream (forward and backward): (id, knobs, jobs).
_T37 = bptt_shapes.TAIL_CASES[2]            # ('seq2seq', 'Seq2Seq', 128, 23, 13)
TRAIN_CASES = [
    # gates + v (attention), gates + argmax (max); dpool under ATTN and MAX; mid-size steps
    ('train_attn_max', {},
     [job('ATTN', (40, 33, 17, 16, 1), 24, 72, save=True, h0=True, stream='s0'),
      job('MAX', (33, 32, 17, 9, 2), 20, 36, save=True, stream='s1')]),
    # the projection in chunks on the side stream, the forward resident tail waiting for them, dpool under
    # LAST; all-states pooling with h0 (dpool under ALL: no memset), the tail's all-states epilogue
    ('train_chunked_tail', dict(xproj_chunk_rows=32),
     [job('LAST', (100, 97, 90, 80, 70, 65, 64, 40, 33, 32, 20, 17, 16, 9, 3, 1), 24, 128, save=True, stream='s0'),
      job('ALL', (20, 16, 16, 9, 5, 2), 24, 128, save=True, h0=True, stream='s1')]),
    # bptt_shapes.TAIL_CASES[2] at T = 37: the BPTT resident tail (and the forward one)
    ('train_bptt_tail_t37', {},
     [job('LAST', bptt_shapes.tail_case_counts(_T37[2], _T37[3], _T37[4]), 20, _T37[2], save=True, h0=True,
          stream='s0')]),
]
STALE_TRAIN = ('stale_train', {},
               [job('ATTN', (300, 257, 200, 100, 50, 33, 17, 9, 5, 3, 2, 1), 40, 128, save=True, h0=True, stream='s0'),
                job('MAX', (200, 150, 64, 33, 9, 2), 24, 72, save=True, stream='s1')])

# Beside the BPTT chain, through the layers' own forward: (id, feed, knobs, cls, I, H, profile, h0).
SIDE_CASES = [
    # d(input) with K split into segments (launch_nt_rows_once) — the split-K product that exists
    ('side_dx_split', 'padded', {}, 'Seq2Seq', 24, 176, (38, 36, 33, 30, 17), True),                 # 154 rows; K = 528: 272 + 256
    # weight gradients in time chunks beside the chain, accumulated across chunks
    ('side_time_chunked', 'padded', dict(bwd_chunk_rows=128), 'Maxout', 24, 128, (130, 100, 60, 40, 30, 20, 10, 5), True),
    # token-fed: float atomics into d_emb_table (exempt: d_src)
    ('side_tokens', 'tokens', {}, 'Attention', 24, 176, (38, 33, 30, 20, 10), False),
    # Seq2Seq_Decode, a time-constant input with h0: float atomics into dx rows (exempt: d_src)
    ('side_repeat_h0', 'repeat', {}, 'Seq2Seq_Decode', 40, 172, (28, 26, 20, 12, 6), True),
]
STALE_SIDE = ('stale_side', 'padded', {}, 'Attention', 40, 256, (200, 150, 100, 64, 33, 17, 9, 5, 3, 1), True)
EXEMPT = {'side_tokens': ('d_src',), 'side_repeat_h0': ('d_src',)}      # float atomics: the oracle in all four runs

# Scoring: lattice rows, A [300, D], B [700, D], the stripe row0 = 5, nrows = 257.
SCORE_N, SCORE_M, SCORE_ROW0, SCORE_NROWS = 300, 700, 5, 257
SCORE_DS = (12, 10)                 # D % 4 == 0 (float4 loads) and D % 4 != 0 (scalar loads)
SCORE_KS = (1, 17, 128)
STALE_SCORE = dict(N=520, M=900, D=16, row0=3, nrows=515, K=128)
GROUP_B, GROUP_D = 150, 12
GTOPK_K = 10
GTOPK_GALLERY = [16] * 12           # 12 gallery groups of 16 rows: 192 rows, two 128-row tiles -> two panels
GTOPK_QUERY = [1, 2] * 35           # 70 query groups


def group_counts(B, seed):
  """Counts drawn from {1, 2, 4, 8}: powers of two, so the mean of integer scores is exact."""
  return [int(c) for c in np.random.RandomState(seed).choice([1, 2, 4, 8], size=B)]


def score_positives(N, M, dup):
  """1 to 4 positives per query, unsorted; with `dup` every fifth query repeats its first positive."""
  lists = []
  for g in range(N):
    p = [(g * 7 + 3 * j * j + 11 * j) % M for j in range(1 + g % 4)]
    p = list(dict.fromkeys(p))
    if dup and g % 5 == 0:
      p.append(p[0])
    lists.append(np.asarray(p, dtype=np.int64))
  return lists


# ---------------------------------------------------------------------------------------------
# the four runs
# ---------------------------------------------------------------------------------------------
_IMAGES = {}


def _image(monkeypatch, family, record):
  """The stale image of a family: record() once per process under a 'zero' proxy that keeps its blocks."""
  if family not in _IMAGES:
    rec = dirty(monkeypatch, 'zero')
    record()
    rec.check_guards('recording ' + family)
    _IMAGES[family] = rec.image()
    rec.release()
  return _IMAGES[family]


def _four_runs(monkeypatch, where, run, family, record, fills=FILLS):
  """{fill: run()'s dict of cloned outputs}, guards and async status checked after every run."""
  from cmhse_amd import ops
  outs = {}
  for fill in fills:
    proxy = dirty(monkeypatch, stale(_image(monkeypatch, family, record)) if fill == 'stale' else fill)
    res = run(proxy)
    torch.cuda.synchronize()
    proxy.check_guards('%s [%s]' % (where, fill))
    assert ops.async_status() == 0, '%s [%s]: a resident kernel gave up waiting' % (where, fill)
    assert len(proxy.blocks) > 0, '%s: nothing went through the allocator seam' % where
    outs[fill] = {k: v.clone() for k, v in res.items() if v is not None}
    proxy.release()
  return outs


def _same_as_zero(outs, where, exempt=()):
  zero = outs['zero']
  for fill, res in outs.items():
    if fill == 'zero':
      continue
    assert set(res) == set(zero), (where, fill)
    for k in sorted(res):
      if k in exempt:
        continue
      assert res[k].dtype == zero[k].dtype and res[k].shape == zero[k].shape, (where, fill, k)
      assert torch.equal(res[k], zero[k]), \
          '%s: output `%s` differs between a zeroed and a `%s` buffer (%d of %d elements)' % (
              where, k, fill, int((res[k] != zero[k]).sum()), zero[k].numel())


def _t(x, dev):
  return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _ints(got, want, what):
  got, want = got.cpu().numpy().astype(np.int64), np.asarray(want).astype(np.int64)
  assert got.shape == want.shape, what
  bad = got != want
  assert not bad.any(), '%s: %d of %d differ' % (what, int(bad.sum()), bad.size)


def _bits(got, want, what):
  got = got.cpu().numpy()
  want = np.ascontiguousarray(want, dtype=got.dtype)
  assert got.shape == want.shape, what
  assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what + ': bits differ'


# ---------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------
def _labelled_exact_reference(S, lists):
  """(rank_lo, rank_hi, best_pos, thr) on exact integer scores: the best positive (smallest index on ties),
  the columns above it, plus the NEGATIVES that tie it."""
  n = S.shape[0]
  lo, hi, pos, thr = (np.zeros(n, dtype=np.int64) for _ in range(4))
  for i in range(n):
    p = np.unique(lists[i])
    pos[i] = p[np.argmax(S[i, p])]
    thr[i] = S[i, pos[i]]
    lo[i] = np.count_nonzero(S[i] > thr[i])
    hi[i] = lo[i] + np.count_nonzero(S[i] == thr[i]) - np.count_nonzero(S[i, p] == thr[i])
  return lo, hi, pos, thr


def _count_calls(ops, a, b, N, M, row0, nrows):
  """The four counting entry points on one stripe: {name: tensor}."""
  out = {}
  out['rank'], out['top1'] = ops.sim_rank(a, b, row0=row0, nrows=nrows)
  (out['lab_rank'], out['lab_top1'], out['lab_pos'], out['lab_score']) = ops.sim_rank_labelled(
      a, b, score_positives(N, M, True), row0=row0, nrows=nrows, return_score=True)
  out['ex_lo'], out['ex_hi'], out['ex_top1'], out['ex_resolved'] = ops.sim_rank_exact(a, b, row0=row0, nrows=nrows)
  (out['lex_lo'], out['lex_hi'], out['lex_top1'], out['lex_pos'], out['lex_resolved'], out['lex_score']) = \
      ops.sim_rank_labelled_exact(a, b, score_positives(N, M, False), row0=row0, nrows=nrows, return_score=True)
  return out


def _record_score(dev):
  from cmhse_amd import ops
  c = STALE_SCORE
  a, b = _t(ss.lattice_rows(c['N'], c['D'], 91), dev), _t(ss.lattice_rows(c['M'], c['D'], 92), dev)
  _count_calls(ops, a, b, c['N'], c['M'], c['row0'], c['nrows'])
  ops.sim_topk(a, b, c['K'], row0=c['row0'], nrows=c['nrows'])
  ops.sim_topk_exact(a, b, c['K'], row0=c['row0'], nrows=c['nrows'])
  nc, ns = group_counts(260, 5), group_counts(260, 6)
  cl, cp = _t(ss.lattice_rows(sum(nc), c['D'], 93), dev), _t(ss.lattice_rows(sum(ns), c['D'], 94), dev)
  for reduce in ('max', 'mean'):
    ops.group_rank(cl, cp, nc, ns, reduce=reduce)
    ops.group_rank_exact(cl, cp, nc, ns, reduce=reduce)
  ops.group_topk(cl, cp, nc, ns, 64, direction='p2v')
  torch.cuda.synchronize()


@pytest.mark.parametrize('D', SCORE_DS)
def test_counting_calls_on_dirty_buffers(dev, monkeypatch, D):
  """sim_rank, sim_rank_labelled, sim_rank_exact and sim_rank_labelled_exact on the stripe."""
  from cmhse_amd import ops
  N, M, row0, nrows = SCORE_N, SCORE_M, SCORE_ROW0, SCORE_NROWS
  an, bn = ss.lattice_rows(N, D, 3 + D), ss.lattice_rows(M, D, 4 + D)
  a, b = _t(an, dev), _t(bn, dev)
  outs = _four_runs(monkeypatch, 'counting calls D=%d' % D,
                    lambda proxy: _count_calls(ops, a, b, N, M, row0, nrows), 'score', lambda: _record_score(dev))
  z = outs['zero']
  S = ss.scores_int(an[row0:row0 + nrows], bn)
  want_rank, want_top1 = ss.rank_reference(S, row0)
  _ints(z['rank'], want_rank, 'sim_rank rank')
  _ints(z['top1'], want_top1, 'sim_rank top1')
  lo, hi = ss.exact_reference(S, row0)
  _ints(z['ex_lo'], lo, 'sim_rank_exact rank_lo')
  _ints(z['ex_hi'], hi, 'sim_rank_exact rank_hi')
  _ints(z['ex_top1'], want_top1, 'sim_rank_exact top1')
  assert int((hi - lo).max()) >= 3, 'the lattice ties the diagonal'
  assert bool((z['ex_resolved'].cpu().numpy() >= hi - lo).all())
  lists = score_positives(N, M, True)[row0:row0 + nrows]
  llo, lhi, lpos, lthr = _labelled_exact_reference(S, lists)
  _ints(z['lab_rank'], llo, 'sim_rank_labelled rank')
  _ints(z['lab_top1'], want_top1, 'sim_rank_labelled top1')
  _ints(z['lab_pos'], lpos, 'sim_rank_labelled best_pos')
  _bits(z['lab_score'], lthr.astype(np.float32), 'sim_rank_labelled best_score')
  _ints(z['lex_lo'], llo, 'sim_rank_labelled_exact rank_lo')
  _ints(z['lex_hi'], lhi, 'sim_rank_labelled_exact rank_hi')
  _ints(z['lex_top1'], want_top1, 'sim_rank_labelled_exact top1')
  _ints(z['lex_pos'], lpos, 'sim_rank_labelled_exact best_pos')
  _bits(z['lex_score'], lthr.astype(np.float64), 'sim_rank_labelled_exact thr64')
  assert bool((z['lex_resolved'].cpu().numpy() >= 1).all())
  _same_as_zero(outs, 'counting calls D=%d' % D)


@pytest.mark.parametrize('K', SCORE_KS)
def test_topk_calls_on_dirty_buffers(dev, monkeypatch, K):
  """sim_topk and sim_topk_exact (more than one gallery panel) on the stripe."""
  from cmhse_amd import ops
  N, M, row0, nrows, D = SCORE_N, SCORE_M, SCORE_ROW0, SCORE_NROWS, SCORE_DS[0]
  assert ss.topk_plan(nrows, M, K)['panels'] > 1
  an, bn = ss.lattice_rows(N, D, 5 + K), ss.lattice_rows(M, D, 6 + K)
  a, b = _t(an, dev), _t(bn, dev)

  def run(proxy):
    out = {}
    out['scores'], out['index'] = ops.sim_topk(a, b, K, row0=row0, nrows=nrows)
    out['ex_scores'], out['ex_index'], out['ex_resolved'] = ops.sim_topk_exact(a, b, K, row0=row0, nrows=nrows)
    return out
  outs = _four_runs(monkeypatch, 'top-K K=%d' % K, run, 'score', lambda: _record_score(dev))
  z = outs['zero']
  ws, wi = ss.topk_reference(ss.scores_int(an[row0:row0 + nrows], bn), K)
  _ints(z['index'], wi, 'sim_topk index')
  _bits(z['scores'], ws.astype(np.float32), 'sim_topk scores')
  _ints(z['ex_index'], wi, 'sim_topk_exact index')
  _bits(z['ex_scores'], ws.astype(np.float64), 'sim_topk_exact scores')
  assert bool((z['ex_resolved'].cpu().numpy() >= K).all())
  _same_as_zero(outs, 'top-K K=%d' % K)


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_group_calls_on_dirty_buffers(dev, monkeypatch, reduce):
  """group_scores, group_rank, group_rank_exact at B = 150 (three 64-group rank tiles) and group_topk in
  both directions with two gallery panels."""
  from cmhse_amd import ops
  B, D = GROUP_B, GROUP_D
  nc, ns = group_counts(B, 1), group_counts(B, 2)
  cn, sn = ss.lattice_rows(sum(nc), D, 7), ss.lattice_rows(sum(ns), D, 8)
  c, s = _t(cn, dev), _t(sn, dev)
  gal, qry = GTOPK_GALLERY, GTOPK_QUERY
  gn, qn = ss.lattice_rows(sum(gal), D, 9), ss.lattice_rows(sum(qry), D, 10)
  g, q = _t(gn, dev), _t(qn, dev)
  names = ('lo_v2p', 'hi_v2p', 'top1_v2p', 'res_v2p', 'lo_p2v', 'hi_p2v', 'top1_p2v', 'res_p2v')

  def run(proxy):
    out = dict(G=ops.group_scores(c, s, nc, ns, reduce=reduce))
    out['rank_v2p'], out['rtop1_v2p'], out['rank_p2v'], out['rtop1_p2v'] = ops.group_rank(c, s, nc, ns, reduce=reduce)
    for name, t in zip(names, ops.group_rank_exact(c, s, nc, ns, reduce=reduce)):
      out['ex_' + name] = t
    # p2v: the paragraphs (caps / num_caps) query the videos; v2p: the reverse
    out['p2v_scores'], out['p2v_index'] = ops.group_topk(g, q, gal, qry, GTOPK_K, direction='p2v', reduce=reduce)
    out['v2p_scores'], out['v2p_index'] = ops.group_topk(q, g, qry, gal, GTOPK_K, direction='v2p', reduce=reduce)
    return out
  outs = _four_runs(monkeypatch, 'group calls ' + reduce, run, 'score', lambda: _record_score(dev))
  z = outs['zero']
  G = ss.lattice_group_scores(ss.scores_int(cn, sn), nc, ns, reduce)
  _bits(z['G'], G, 'group_scores')
  for got, ref, what in zip((z['rank_v2p'], z['rtop1_v2p'], z['rank_p2v'], z['rtop1_p2v']), ss.group_rank_reference(G),
                            ('rank v2p', 'top1 v2p', 'rank p2v', 'top1 p2v')):
    _ints(got, ref, 'group_rank ' + what)
  d = np.diag(G)
  _ints(z['ex_lo_v2p'], (G > d[:, None]).sum(1), 'group_rank_exact rank_lo v2p')
  _ints(z['ex_hi_v2p'], (G >= d[:, None]).sum(1) - 1, 'group_rank_exact rank_hi v2p')
  _ints(z['ex_lo_p2v'], (G > d[None, :]).sum(0), 'group_rank_exact rank_lo p2v')
  _ints(z['ex_hi_p2v'], (G >= d[None, :]).sum(0) - 1, 'group_rank_exact rank_hi p2v')
  _ints(z['ex_top1_v2p'], G.argmax(1), 'group_rank_exact top1 v2p')
  _ints(z['ex_top1_p2v'], G.argmax(0), 'group_rank_exact top1 p2v')
  assert int(((G >= d[:, None]).sum(1) - 1 - (G > d[:, None]).sum(1)).max()) >= 1, 'the lattice ties the diagonal'
  Gq = ss.lattice_group_scores(ss.scores_int(gn, qn), gal, qry, reduce)          # [videos, paragraphs]
  for direction, Q in (('p2v', Gq.T), ('v2p', ss.lattice_group_scores(ss.scores_int(qn, gn), qry, gal, reduce))):
    ws, wi = ss.topk_reference(Q.astype(np.float64), GTOPK_K)
    _ints(z[direction + '_index'], wi, 'group_topk %s index' % direction)
    _bits(z[direction + '_scores'], ws.astype(np.float32), 'group_topk %s scores' % direction)
  _same_as_zero(outs, 'group calls ' + reduce)


@pytest.mark.parametrize('fill', ['ones', 'a5'])
def test_empty_stripes_leave_poisoned_outputs_alone(dev, monkeypatch, fill):
  """nrows == 0: every entry point returns CMHSE_OK and touches neither its outputs nor its workspace."""
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  N, M, D = 40, 50, 12
  a, b = _t(ss.lattice_rows(N, D, 1), dev), _t(ss.lattice_rows(M, D, 2), dev)
  proxy = dirty(monkeypatch, fill)
  bufs = [proxy.empty(64, dtype=torch.int32, device=dev) for _ in range(6)]
  f32, f64 = proxy.empty(64, dtype=torch.float32, device=dev), proxy.empty(64, dtype=torch.float64, device=dev)
  ws = proxy.empty(4096, dtype=torch.uint8, device=dev)
  p = [t.data_ptr() for t in bufs]
  st = ops._stream()
  host = np.zeros(1, dtype=np.int32)
  assert lib.cmhse_sim_rank(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, p[0], p[1], ws.data_ptr(), 4096, st) == 0
  assert lib.cmhse_sim_rank_exact(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, p[0], p[1], p[2], p[3], ws.data_ptr(),
                                  4096, st) == 0
  assert lib.cmhse_sim_rank_labelled(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, host.ctypes.data, host.ctypes.data,
                                     p[4], p[5], 0, p[0], p[1], p[2], f32.data_ptr(), ws.data_ptr(), 4096, st) == 0
  assert lib.cmhse_sim_rank_labelled_exact(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, host.ctypes.data,
                                           host.ctypes.data, p[4], p[5], 0, p[0], p[1], p[2], p[3], f64.data_ptr(),
                                           p[4], ws.data_ptr(), 4096, st) == 0
  assert lib.cmhse_sim_topk(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, 4, f32.data_ptr(), p[0], ws.data_ptr(), 4096,
                            st) == 0
  assert lib.cmhse_sim_topk_exact(a.data_ptr(), b.data_ptr(), N, M, D, 3, 0, 4, f64.data_ptr(), p[0], p[1],
                                  ws.data_ptr(), 4096, st) == 0
  torch.cuda.synchronize()
  proxy.check_guards('empty stripes')
  for block, _, _ in proxy.blocks:
    assert bool((block == BYTE[fill]).all()), 'an empty stripe wrote into a buffer'
  # the wrappers: empty results, no call
  for out in (ops.sim_rank(a, b, row0=3, nrows=0), ops.sim_rank_exact(a, b, row0=3, nrows=0),
              ops.sim_topk(a, b, 4, row0=3, nrows=0), ops.sim_topk_exact(a, b, 4, row0=3, nrows=0)):
    assert all(t.numel() == 0 for t in out)


# ---------------------------------------------------------------------------------------------
# utilities
# ---------------------------------------------------------------------------------------------
def test_row_utilities_on_dirty_buffers(dev, monkeypatch):
  """pad_rows (padding comes out zero), gather_rows, l2norm_rows with ld > cols (the gap columns keep
  their fill), rows_differ, tok_prefix_check."""
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  rng = np.random.RandomState(3)
  lens = np.array([5, 1, 9, 3, 7], dtype=np.int64)
  I = 10
  data = rng.standard_normal((int(lens.sum()), I)).astype(np.float32)
  table = rng.standard_normal((37, 6)).astype(np.float32)
  ids = rng.randint(0, 37, size=(7, 3)).astype(np.int64)
  x = rng.standard_normal((33, 18)).astype(np.float32)
  cols, ld = 13, 18
  tok_a = rng.randint(0, 50, size=(4, 6)).astype(np.int64)
  tok_b = tok_a.copy()
  tok_b[2, 1] += 1                       # pair 2 differs inside the prefix
  a_len, b_len = np.array([3, 6, 4, 5], dtype=np.int32), np.array([6, 6, 6, 4], dtype=np.int32)   # pair 3: b shorter
  data_d, table_d, ids_d, x_d = _t(data, dev), _t(table, dev), _t(ids, dev), _t(x, dev)
  ta, tb = _t(tok_a, dev), _t(tok_b, dev)
  x2 = x_d.clone()
  x2.view(-1)[-1] += 1.0
  fills = {}

  def run(proxy):
    out = dict(padded=ops.Ragged(data_d, lens).padded(), gathered=ops.gather_rows(table_d, ids_d),
               normed=ops.l2norm_rows(x_d))
    y = proxy.empty(x.shape, dtype=torch.float32, device=dev)
    fills[id(proxy)] = y.clone()
    _lib.check(lib.cmhse_l2norm_rows(x_d.data_ptr(), y.data_ptr(), x.shape[0], cols, ld, ops._stream()),
               'cmhse_l2norm_rows')
    out['normed_ld'] = y[:, :cols]
    gap_kept = torch.equal(y[:, cols:].contiguous().view(torch.uint8), fills[id(proxy)][:, cols:].contiguous().view(torch.uint8))
    out['gap_kept'] = torch.tensor([gap_kept])
    out['differ'] = torch.tensor([ops.rows_differ([(x_d, x_d.clone())]), ops.rows_differ([(x_d, x2)])])
    out['prefix'] = ops.tok_prefix_check(ops.padded_row_ptrs(ta), ops.padded_row_ptrs(tb), a_len, b_len, dev)
    return out
  outs = _four_runs(monkeypatch, 'row utilities', run, 'util', lambda: (ops.l2norm_rows(_t(rng.standard_normal((90, 40)).astype(np.float32), dev)),
                                                                        ops.gather_rows(table_d, _t(rng.randint(0, 37, size=(50, 9)), dev))))
  z = outs['zero']
  want = np.zeros((len(lens), int(lens.max()), I), dtype=np.float32)
  first = np.concatenate([[0], np.cumsum(lens)[:-1]])
  for s, l in enumerate(lens):
    want[s, :l] = data[first[s]:first[s] + l]
  _bits(z['padded'], want, 'pad_rows')
  _bits(z['gathered'], table[ids], 'gather_rows')
  n64 = x.astype(np.float64)
  assert_emb_close(z['normed'].cpu().numpy(), n64 / np.maximum(np.linalg.norm(n64, axis=1, keepdims=True), 1e-12))
  c64 = n64[:, :cols]
  assert_emb_close(z['normed_ld'].cpu().numpy(), c64 / np.maximum(np.linalg.norm(c64, axis=1, keepdims=True), 1e-12))
  assert z['differ'].tolist() == [False, True]
  assert z['prefix'].tolist() == [1, 1, 0, 0]
  for fill, res in outs.items():
    assert bool(res['gap_kept'].item()), 'l2norm_rows wrote the columns between cols and ld [%s]' % fill
  _same_as_zero(outs, 'row utilities')


# ---------------------------------------------------------------------------------------------
# GRU forward and backward
# ---------------------------------------------------------------------------------------------
class _Contexts(object):
  """Records the forward contexts of every ops.gru_pool_fwd_multi call (what the forward saved)."""

  def __init__(self, monkeypatch):
    from cmhse_amd import ops
    self.ctxs = []
    real = ops.gru_pool_fwd_multi

    def wrapper(requests, *a, **kw):
      res = real(requests, *a, **kw)
      self.ctxs.append([ctx for _, ctx in res])
      return res
    monkeypatch.setattr(ops, 'gru_pool_fwd_multi', wrapper)

  def take(self):
    out, self.ctxs = self.ctxs, []
    return out


def _saved(ops, ctx, names, rows=None):
  out = {}
  for name in names:
    v = ops.saved_region(ctx, name)
    if v is not None:
      out[name] = (v if rows is None or name == 'h0_s' else v[:rows]).clone()
  return out


def _fwd_run(case, dev):
  """(run(proxy) -> outputs of one inference call incl. the saved hidden states, setup) of a FWD case."""
  import test_gpu_fwd_shapes as fs
  from cmhse_amd import ops
  name, knobs, _, tail_stream, jobs, bf3 = case
  layers_, sds, data, _ = fs._setup(jobs, dev)
  plan = fwd_shapes.call_steps(jobs, knobs, tail_stream, bf3=bf3)

  def run(proxy):
    with ops.tuned(**knobs):
      if bf3:
        ops.set_math_mode('bf16x3')
      try:
        res = fs._run_inference(jobs, layers_, data, dev, tail_stream)
      finally:
        ops.set_math_mode('fp32')
    out = {}
    for k, (o, ctx) in enumerate(res):
      out['out%d' % k] = o
      out['hs%d' % k] = ops.saved_region(ctx, 'hs')
      if bf3 and plan[k].bf3 and plan[k].rows_split > 0:
        for r, v in _saved(ops, ctx, ('xs', 'hs_s') + (('h0_s',) if jobs[k]['h0'] else ()), plan[k].rows_split).items():
          out['%s%d' % (r, k)] = v
    return out
  return run, (jobs, sds, data, plan)


def _packed(hs, order, counts):
  return np.concatenate([hs[order[:c], t] for t, c in enumerate(counts)])


@pytest.mark.parametrize('case', FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_on_dirty_buffers(dev, oracle, monkeypatch, case):
  import test_gpu_fwd_shapes as fs
  name, knobs, _, tail_stream, jobs, bf3 = case
  run, (jobs, sds, data, plan) = _fwd_run(case, dev)
  outs = _four_runs(monkeypatch, name, run, 'fwd', lambda: _fwd_run(STALE_FWD, dev)[0](None))
  z = outs['zero']
  for k, (j, (lens, x, h0, _, _)) in enumerate(zip(jobs, data)):
    tag = '%s request %d (%s, I %d, H %d)' % (name, k, j['pool'], j['I'], j['H'])
    order = np.argsort(-lens, kind='stable')
    with _blas_threads():
      want, cache = fs._oracle(oracle, j, x, lens, sds[k], h0)
      rows = [want]
      for src, n in j.get('aliases', ()):
        rows.append(oracle.pooled_gru_forward_cache('attention', x[src:src + 1, :n], np.asarray([n]), sds[k],
                                                    None if h0 is None else h0[src:src + 1])[0])
      want = np.concatenate(rows)
      if bf3:
        split_steps = sum(len(ln['ts']) for ln in plan[k] if ln['tag'] == 'TiledBf3')
        split_att = any(ln['kind'] == 'attn' and ln['bf3'] for ln in plan[k])
        emu, emu_hs = oracle.pooled_gru_forward(fs._ORACLE_POOL[j['pool']], x, lens, sds[k], h0, np.float64,
                                                products='bf16x3', split_steps=split_steps, split_attention=split_att)
    got, got_hs = z['out%d' % k].cpu().numpy(), z['hs%d' % k].cpu().numpy()
    want_hs = _packed(cache['hs'], order, j['counts'])
    if bf3:      # the bars of tests/test_gpu_bf3_shapes.py: the mode against the oracle and against its emulation
      from test_gpu_bf3_shapes import BF3_TOL
      d_or = max(np.abs(got - want).max(), np.abs(got_hs - want_hs).max())
      d_emu = max(np.abs(got - emu).max(), np.abs(got_hs - _packed(emu_hs, order, j['counts'])).max())
      assert d_or <= min(EMB_TOL, BF3_TOL), '%s: %.3e from the float64 oracle' % (tag, d_or)
      assert d_emu <= GOLDEN_TOL, '%s: %.3e from the emulation of the split' % (tag, d_emu)
    else:
      assert_emb_close(got, want, tag)
      assert_emb_close(got_hs, want_hs, tag + ' hs')
  _same_as_zero(outs, name)


def _train_run(case, dev, contexts):
  import test_gpu_fwd_shapes as fs
  from cmhse_amd import ops
  name, knobs, jobs = case
  layers_, sds, data, rng = fs._setup(jobs, dev)
  ws = [rng.standard_normal((int(d[0].sum()) if j['pool'] == 'ALL' else len(d[0]), j['H'])).astype(np.float32)
        for j, d in zip(jobs, data)]

  def run(proxy):
    saved = {}

    def after_forward():
      (ctxs,) = contexts.take()
      for k, ctx in enumerate(ctxs):
        for r, v in _saved(ops, ctx, ('hs', 'gates', 'argmax', 'v')).items():
          saved['%s%d' % (r, k)] = v
    with ops.tuned(**knobs):
      res = fs._run_training(jobs, layers_, data, ws, dev, after_forward=after_forward)
    out = dict(saved)
    for k, (j, r) in enumerate(zip(jobs, res)):
      names = ['out', 'dx'] + (['dh0'] if j['h0'] else []) + [pn for pn, _ in layers_[k].named_parameters()]
      assert len(names) == len(r)
      for n, t in zip(names, r):
        out['%s%d' % (n, k)] = t
    return out
  return run, (jobs, layers_, sds, data, ws)


@pytest.mark.parametrize('case', TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_training_on_dirty_buffers(dev, oracle, monkeypatch, case):
  """layers.run_grouped forward and backward: outputs, what the forward saved, dx, dh0, every parameter gradient."""
  import test_gpu_fwd_shapes as fs
  name = case[0]
  contexts = _Contexts(monkeypatch)
  run, (jobs, layers_, sds, data, ws) = _train_run(case, dev, contexts)
  outs = _four_runs(monkeypatch, name, run, 'train', lambda: _train_run(STALE_TRAIN, dev, contexts)[0](None))
  z = outs['zero']
  for k, (j, (lens, x, h0, _, _)) in enumerate(zip(jobs, data)):
    tag = '%s request %d (%s, I %d, H %d)' % (name, k, j['pool'], j['I'], j['H'])
    order = np.argsort(-lens, kind='stable')
    with _blas_threads():
      want, cache = fs._oracle(oracle, j, x, lens, sds[k], h0)
      grads, dx, dh0 = fs._backward(oracle, j, cache, lens, ws[k])
    assert_emb_close(z['out%d' % k].cpu().numpy(), want, tag)
    assert_emb_close(z['hs%d' % k].cpu().numpy(), _packed(cache['hs'], order, j['counts']), tag + ' saved hs')
    assert 'gates%d' % k in z and (j['pool'] != 'MAX' or 'argmax%d' % k in z) and (j['pool'] != 'ATTN' or 'v%d' % k in z)
    grad_close(z['dx%d' % k].cpu().numpy()[:, :dx.shape[1]], dx, tag + ' dx')
    if h0 is not None:
      grad_close(z['dh0%d' % k].cpu().numpy(), dh0, tag + ' dh0')
    for pn, _ in layers_[k].named_parameters():
      grad_close(z['%s%d' % (pn, k)].cpu().numpy(), grads['rnn.' + pn], tag + ' ' + pn)
  _same_as_zero(outs, name)


def _side_run(case, dev):
  """A SIDE case through the layer's own forward (the run of tests/test_gpu_bwd_side_shapes.py)."""
  import test_gpu_bwd_side_shapes as tb
  from cmhse_amd import layers, ops
  name, feed, knobs, cls, I, H, profile, with_h0 = case
  lens = bss.lens_of(profile)
  S, T = len(lens), int(lens.max())
  rng = np.random.RandomState(S + 7 * H + I)
  layer, sd = tb._layer(cls, I, H, H + I)
  layer = layer.to(dev)
  pool = bss.POOL_OF[cls]
  tok = None
  h0 = (0.5 * rng.standard_normal((S, H))).astype(np.float32) if with_h0 else None
  if feed == 'padded':
    src = x = tb._padded(rng, lens, I)
  elif feed == 'tokens':
    src = rng.standard_normal((bss.VOCAB, I)).astype(np.float32)
    tok = bss.case_tokens(rng, lens)
    ids = bss.clamp_ids(tok, bss.VOCAB)
    x = np.zeros((S, T, I), dtype=np.float32)
    for i, l in enumerate(lens):
      x[i, :l] = src[ids[i, :l]]
  else:
    src = rng.standard_normal((S, I)).astype(np.float32)
    x = np.zeros((S, T, I), dtype=np.float32)
    for i, l in enumerate(lens):
      x[i, :l] = src[i]
  n_out = int(lens.sum()) if pool == 'all' else S
  w = rng.standard_normal((n_out, H)).astype(np.float32)
  lens_t = torch.from_numpy(lens)

  def run(proxy):
    layer.zero_grad()
    st = torch.from_numpy(src).to(dev).requires_grad_(True)
    ht = torch.from_numpy(h0).to(dev).requires_grad_(True) if h0 is not None else None
    with ops.tuned(**knobs):
      if feed == 'padded':
        y = layer(st, lens_t, ht)
      elif feed == 'tokens':
        y = layer.forward_tokens(torch.from_numpy(tok).to(dev), lens_t, st)
      else:
        y = layer._run(layers.SeqInput('repeat', lens, layer.POOL), st, ht, None)
      (y * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = dict(y=y.detach().clone(), d_src=st.grad.clone())
    if ht is not None:
      out['dh0'] = ht.grad.clone()
    for pn, p in layer.named_parameters():
      out[pn] = p.grad.clone()
    return out
  return run, dict(layer=layer, sd=sd, lens=lens, x=x, h0=h0, tok=tok, w=w, pool=pool, feed=feed)


@pytest.mark.parametrize('case', SIDE_CASES, ids=[c[0] for c in SIDE_CASES])
def test_side_launches_on_dirty_buffers(dev, oracle, monkeypatch, case):
  """What cmhse_gru_pool_bwd launches beside the chain: the split-K d(input), time-chunked weight gradients,
  the two float-atomic scatters (held to the oracle in every run)."""
  name = case[0]
  run, c = _side_run(case, dev)
  outs = _four_runs(monkeypatch, name, run, 'side', lambda: _side_run(STALE_SIDE, dev)[0](None))
  lens, x, h0, w, pool, feed = c['lens'], c['x'], c['h0'], c['w'], c['pool'], c['feed']
  with _blas_threads():
    if pool == 'all':
      cache = oracle.gru_forward_cache(x, lens, c['sd'], h0, np.float64)
      want = np.concatenate([cache['hs'][i, :l] for i, l in enumerate(lens)])
      starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
      dhs = np.zeros_like(cache['hs'])
      for i, l in enumerate(lens):
        dhs[i, :l] = w[starts[i]:starts[i] + l]
      grads, dx, dh0 = oracle.gru_backward(cache, dhs)
    else:
      want, cache = oracle.pooled_gru_forward_cache(pool, x, lens, c['sd'], h0)
      grads, dx, dh0 = oracle.pooled_gru_backward(cache, w.astype(np.float64))
  if feed == 'padded':
    want_src = None
  elif feed == 'tokens':
    want_src = bss.d_table_from_dx(dx, c['tok'], lens, bss.VOCAB)
  else:
    want_src = bss.d_rows_from_dx(dx, lens)
  exempt = EXEMPT.get(name, ())
  assert (feed != 'padded') == ('d_src' in exempt)
  for fill, res in outs.items():
    if fill != 'zero' and not exempt:
      continue
    tag = '%s [%s] ' % (name, fill)
    if want_src is not None:
      grad_close(res['d_src'].cpu().numpy(), want_src, tag + 'd_src')
    if fill != 'zero':
      continue
    assert_emb_close(res['y'].cpu().numpy(), want, tag + 'out')
    if feed == 'padded':
      grad_close(res['d_src'].cpu().numpy()[:, :dx.shape[1]], dx, tag + 'dx')
    if h0 is not None:
      grad_close(res['dh0'].cpu().numpy(), dh0, tag + 'dh0')
    for pn, _ in c['layer'].named_parameters():
      grad_close(res[pn].cpu().numpy(), grads['rnn.' + pn], tag + pn)
  _same_as_zero(outs, name, exempt)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_validation_pass_zero_against_ones(dev, monkeypatch):
  """One small validation pass of the golden attention model: embeddings and all ranks bit-equal whether
  every buffer starts as zeros or as 0xFF.  evaluation.encode_data_device leaves the padding of its device
  batches uninitialised "and never read": here that is a test."""
  from cmhse_amd import ops, synthetic
  from cmhse_amd.evaluation import encode_data, i2t, t2i
  opt, model = golden_model('attention', load_golden('model_attention.npz'))
  spec = synthetic.ragged_spec(29, seed=6)
  batches = synthetic.make_batches(spec, 5, opt.img_dim, opt.vocab_size, seed=2)
  got = {}
  for fill in ('zero', 'ones'):
    proxy = dirty(monkeypatch, fill)
    res = encode_data(opt, model, synthetic.ListLoader(batches), logging=lambda *a: None)
    ri, rt = i2t(res[0], res[1]), t2i(res[0], res[1])
    torch.cuda.synchronize()
    proxy.check_guards('validation pass [%s]' % fill)
    assert ops.async_status() == 0
    assert len(proxy.blocks) > 0
    got[fill] = ([np.array(r) for r in res[:6]], ri, rt)
    proxy.release()
  for k, (a, b) in enumerate(zip(got['zero'][0], got['ones'][0])):
    assert a.dtype == b.dtype and a.shape == b.shape and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'embedding %d depends on what the buffers held' % k
  for za, oa in zip(got['zero'][1:], got['ones'][1:]):
    assert za[0] == oa[0]                                   # the report
    assert np.array_equal(za[1], oa[1]) and np.array_equal(za[2], oa[2])      # top-1, ranks


@pytest.mark.parametrize('rnn_type', ['attention', 'maxout', 'seq2seq'])
def test_train_step_with_reconstruction_under_ones(dev, oracle, monkeypatch, rnn_type):
  """One VSE.train_emb step with --reconstruct_loss, every buffer starting as 0xFF, against the float64
  oracle: the logged losses and every parameter gradient (gpu_common._check_train_step_vs_oracle).  A twin
  model runs the same step on zeroed buffers: the logged losses and every gradient are bit-equal, all but
  the word table's (`embed.weight`: float atomics, tests/test_gpu_pipeline.py
  test_train_step_on_a_packed_batch_is_bit_identical), which the oracle comparison holds under grad_close."""
  import copy
  from gpu_common import MeterLog, _RecordForward
  from cmhse_amd import ops, synthetic
  from cmhse_amd.model import VSE
  opt = golden_opt(rnn_type, low_level_loss=True, reconstruct_loss=True, norm=True, weight_recon=0.0005,
                   lowest_weight_recon=0.0001, decode_rnn_type='seq2seq')
  torch.manual_seed(21)
  model = VSE(opt)
  twin = VSE(opt)
  twin.load_state_dict(copy.deepcopy(model.state_dict(opt)), opt)
  spec = synthetic.ragged_spec(9, seed=2, max_frames=11, max_video=13)
  batch = synthetic.make_batches(spec, 9, opt.img_dim, opt.vocab_size, seed=1)[0]
  rec = _RecordForward(monkeypatch)
  proxy = dirty(monkeypatch, 'zero')
  twin.logger = MeterLog()
  twin.train_start(opt)
  twin.train_emb(opt, *batch)
  torch.cuda.synchronize()
  proxy.check_guards('train_emb [%s, zero]' % rnn_type)
  assert ops.async_status() == 0 and len(proxy.blocks) > 0
  proxy.release()
  rec.calls = []
  proxy = dirty(monkeypatch, 'ones')
  _check_train_step_vs_oracle(model, opt, batch, oracle, rnn_type, rec, recon=True)
  proxy.check_guards('train_emb [%s, ones]' % rnn_type)
  assert ops.async_status() == 0 and len(proxy.blocks) > 0
  proxy.release()
  logs = [[c for c in m.logger.calls if c[0].startswith('Le')] for m in (twin, model)]
  assert logs[0] == logs[1] and len(logs[0]) >= 9, 'the logged losses depend on what the buffers held'
  seen = 0
  for mz, mo in zip(twin._modules(), model._modules()):
    for (nz, pz), (no, po) in zip(mz.named_parameters(), mo.named_parameters()):
      assert nz == no and pz.grad is not None and po.grad is not None
      if nz == 'embed.weight':      # float atomics: run to run in the last bits (the oracle comparison above holds it)
        scale = float(pz.grad.abs().max())
        assert float((pz.grad - po.grad).abs().max()) <= 1e-5 * scale + 1e-12, nz
        seen += 1
      else:
        assert torch.equal(pz.grad, po.grad), 'the gradient of %s depends on what the buffers held' % nz
  assert seen == 1
