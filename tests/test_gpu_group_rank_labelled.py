"""Labelled group-wise ranking (cmhse_group_rank_labelled / ops.group_rank_labelled /
evaluation.group_rank_labelled / evaluation.group_i2t_t2i_labelled) on the MI355X.

The oracle of every test is the stored G of ops.group_scores (rectangular problems: the padding trick of
test_gpu_group_topk._group_scores_rect) with the contract applied in NumPy
(test_group_rank_labelled_cpu.group_labelled_reference), or ops.group_rank where the issue is the square
diagonal case.  Every comparison is exact: integers equal, scores equal in their bits."""
import numpy as np
import pytest
import torch

from dirty_alloc import dirty
from test_gpu_group_rank import CASES, STRADDLE, _inputs, _rand
from test_gpu_group_topk import _group_scores_rect, _rows_of
from test_group_rank_labelled_cpu import (MANY, cap_case, group_labelled_reference, panel_case, rect_counts,
                                          rect_labels)

pytestmark = pytest.mark.gpu

NAMES = ('rank', 'top1', 'best_pos', 'best_score')


def _host(out):
  return [t.cpu().numpy() for t in out]


def _assert_same(got, want, where=''):
  """(rank, top1, best_pos[, best_score]) device tensors against the NumPy contract: integers equal, the
  score equal in its bits."""
  got = _host(got)
  for g, w, name in zip(got, want, NAMES):
    if name == 'best_score':
      assert g.dtype == np.float32 and g.shape == w.shape
      assert np.array_equal(g.view(np.int32), np.ascontiguousarray(w, np.float32).view(np.int32)), \
          '%s %s differs in its bits in %d places' % (where, name, int((g != w).sum()))
    else:
      assert g.dtype == np.int32 and g.shape == w.shape
      assert np.array_equal(g, w), '%s %s differs in %d places' % (where, name, int((g != w).sum()))


def _check(c, s, nclips, ncaps, off, idx, direction, reduce, G=None, where=''):
  from cmhse_amd import ops
  G = _group_scores_rect(c, s, nclips, ncaps, reduce) if G is None else G
  got = ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True)
  for t in got:
    assert t.is_cuda
  _assert_same(got, group_labelled_reference(G, direction, off, idx), '%s %s %s' % (where, direction, reduce))
  return got


# ---------------------------------------------------------------------------------------------
# 1. the diagonal equals ops.group_rank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('name,nclips,ncaps,d', CASES, ids=[c[0] for c in CASES])
def test_diagonal_equals_group_rank(dev, name, nclips, ncaps, d, reduce):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  B = len(nclips)
  rank_v, top1_v, rank_p, top1_p = _host(ops.group_rank(c, s, nclips, ncaps, reduce=reduce))
  diag = np.arange(B)
  for direction, rank, top1 in (('v2p', rank_v, top1_v), ('p2v', rank_p, top1_p)):
    got = ops.group_rank_labelled(c, s, nclips, ncaps, diag, direction, reduce)
    assert len(got) == 3
    for t in got:
      assert t.dtype == torch.int32 and t.shape == (B,) and t.is_cuda
    g_rank, g_top1, g_pos = _host(got)
    assert np.array_equal(g_rank, rank), direction
    assert np.array_equal(g_top1, top1), direction
    assert np.array_equal(g_pos, diag), direction


# ---------------------------------------------------------------------------------------------
# 2. rectangular, many positives
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rect(dev):
  """700 videos x 500 paragraphs (counts 1..19, D = 256) and its stored G in both reduce modes."""
  nclips, ncaps = rect_counts()
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=60)
  G = {reduce: _group_scores_rect(c, s, nclips, ncaps, reduce) for reduce in ('max', 'mean')}
  return c, s, nclips, ncaps, G


@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_rectangular_many_positives(rect, direction, reduce):
  c, s, nclips, ncaps, G = rect
  Bq, Bg = (500, 700) if direction == 'p2v' else (700, 500)
  off, idx = rect_labels(41, Bq, Bg, many_at=Bq // 2)     # one query with MANY positives: several pair tiles
  assert off[Bq // 2 + 1] - off[Bq // 2] == MANY
  _check(c, s, nclips, ncaps, off, idx, direction, reduce, G[reduce], '700 x 500')


@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_rectangular_reversed(dev, direction, reduce):
  """The reverse problem: 500 videos x 700 paragraphs (the same counts, the sides swapped)."""
  ncaps, nclips = rect_counts()
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=61)
  Bq, Bg = (700, 500) if direction == 'p2v' else (500, 700)
  off, idx = rect_labels(42, Bq, Bg, many_at=3)
  _check(c, s, nclips, ncaps, off, idx, direction, reduce, None, '500 x 700')


# ---------------------------------------------------------------------------------------------
# 3. more than one panel, more query groups than the cap
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
@pytest.mark.parametrize('case', ['panels', 'cap'])
def test_panels_and_query_cap(dev, case, direction):
  qn, gn = panel_case() if case == 'panels' else cap_case()
  nclips, ncaps = (gn, qn) if direction == 'p2v' else (qn, gn)
  c, s, _ = _inputs(dev, nclips, ncaps, 128, seed=70)
  off, idx = rect_labels(43 if case == 'panels' else 47, len(qn), len(gn))
  for reduce in ('max', 'mean'):
    _check(c, s, nclips, ncaps, off, idx, direction, reduce, None, case)


# ---------------------------------------------------------------------------------------------
# 4. the tie rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_tie_rule_duplicated_gallery(dev, reduce):
  """The gallery three times over: the copies of a positive tie thr exactly and are not counted, best_pos is
  the smallest of tied positives, top1 the smaller index."""
  from cmhse_amd import ops
  rng = np.random.RandomState(23)
  base = [int(x) for x in rng.randint(1, 9, 60)]
  vids = _rand(dev, sum(base), 128, 51)
  ncaps = [int(x) for x in rng.randint(1, 9, 70)]
  paras = _rand(dev, sum(ncaps), 128, 52)
  c3, n3 = torch.cat([vids, vids, vids]).contiguous(), base * 3
  G = _group_scores_rect(c3, paras, n3, ncaps, reduce)
  assert np.array_equal(G[:60].view(np.int32), G[60:120].view(np.int32))
  # p2v: paragraph j's positives are the second and third copy of video j % 60 (the larger index first)
  lists = [[j % 60 + 120, j % 60 + 60] for j in range(70)]
  off, idx = np.arange(0, 141, 2), np.concatenate(lists)
  rank, top1, best_pos, _ = _host(_check(c3, paras, n3, ncaps, off, idx, 'p2v', reduce, G, 'tripled gallery'))
  assert np.array_equal(best_pos, np.arange(70) % 60 + 60)            # the smallest of the tied positives
  assert (top1 < 60).all()                                            # the first copy of the best video
  alone = _host(ops.group_rank_labelled(vids, paras, base, ncaps, np.arange(70) % 60, 'p2v', reduce))
  assert np.array_equal(rank, 3 * alone[0])                           # the first copy ties thr: not counted
  assert np.array_equal(top1, alone[1])
  # v2p: paragraph j and j + 70 hold the same captions; the positive is the second copy
  p2, m2 = torch.cat([paras, paras]).contiguous(), ncaps * 2
  target = np.arange(60) % 70 + 70
  rank, top1, best_pos, _ = _host(_check(vids, p2, base, m2, np.arange(61), target, 'v2p', reduce, None, 'doubled'))
  assert np.array_equal(best_pos, target) and (top1 < 70).all()
  alone = _host(ops.group_rank_labelled(vids, paras, base, ncaps, np.arange(60) % 70, 'v2p', reduce))
  assert np.array_equal(rank, 2 * alone[0])


@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_collapsed_input_ranks_zero(dev, direction, reduce):
  """All rows equal: every block score ties, nothing is counted, top1 is group 0, best_pos the smallest."""
  from cmhse_amd import ops
  row = _rand(dev, 1, 64, 81)
  nclips, ncaps = [2] * 90, [3] * 50                       # equal counts per side: the means tie in their bits too
  c, s = row.repeat(sum(nclips), 1).contiguous(), row.repeat(sum(ncaps), 1).contiguous()
  Bq, Bg = (50, 90) if direction == 'p2v' else (90, 50)
  off, idx = rect_labels(83, Bq, Bg)
  rank, top1, best_pos = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce))
  assert (rank == 0).all() and (top1 == 0).all()
  assert np.array_equal(best_pos, [idx[off[q]:off[q + 1]].min() for q in range(Bq)])


# ---------------------------------------------------------------------------------------------
# 5. stripes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_query_stripes_concatenate(rect, direction, reduce):
  from cmhse_amd import ops
  c, s, nclips, ncaps, _ = rect
  Bq, Bg = (500, 700) if direction == 'p2v' else (700, 500)
  off, idx = rect_labels(41, Bq, Bg, many_at=Bq // 2)
  whole = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
  q, qn = (s, ncaps) if direction == 'p2v' else (c, nclips)
  parts = []
  for a, b in [(0, 1), (1, 130), (130, 131), (131, Bq)]:
    rows, counts = _rows_of(q, qn, range(a, b))
    labels = (off[a:b + 1] - off[a], idx[off[a]:off[b]])
    args = (c, rows, nclips, counts) if direction == 'p2v' else (rows, s, counts, ncaps)
    parts.append(_host(ops.group_rank_labelled(*args, labels, direction, reduce, return_score=True)))
  for k, name in enumerate(NAMES):
    joined = np.concatenate([p[k] for p in parts])
    assert joined.dtype == whole[k].dtype
    assert np.array_equal(joined.view(np.int32), whole[k].view(np.int32)), name


# ---------------------------------------------------------------------------------------------
# 6. determinism, 7. dirty memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_math_mode_and_repeats_change_no_bit(dev, reduce):
  from cmhse_amd import ops
  nclips, ncaps = STRADDLE * 4, STRADDLE[::-1] * 3
  c, s, _ = _inputs(dev, nclips, ncaps, 1024, seed=50)
  for direction, Bq, Bg in (('p2v', len(ncaps), len(nclips)), ('v2p', len(nclips), len(ncaps))):
    off, idx = rect_labels(51, Bq, Bg, many_at=1)
    first = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
    for _ in range(3):
      again = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
      for a, b in zip(again, first):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    mode = ops.math_mode()
    ops.set_math_mode('bf16x3')
    try:
      bf3 = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
    finally:
      ops.set_math_mode(mode)
    for a, b in zip(bf3, first):
      assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_dirty_workspace_and_outputs(dev, monkeypatch, direction):
  """The workspace and the outputs start as 0xFF bytes: the call initialises what it reads."""
  from cmhse_amd import ops
  qn, gn = panel_case()
  gn = gn[:400]                                            # several gallery tiles: several panels
  nclips, ncaps = (gn, qn) if direction == 'p2v' else (qn, gn)
  c, s, _ = _inputs(dev, nclips, ncaps, 96, seed=90)
  off, idx = rect_labels(91, len(qn), len(gn), many_at=7)
  for reduce in ('max', 'mean'):
    clean = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
    with monkeypatch.context() as m:
      proxy = dirty(m, 'ones', modules=('cmhse_amd.ops',))
      got = _host(ops.group_rank_labelled(c, s, nclips, ncaps, (off, idx), direction, reduce, return_score=True))
      assert len(proxy.blocks) >= 3                        # the outputs, the score, the workspace
      proxy.check_guards('group_rank_labelled ' + direction)
      proxy.release()
    for a, b in zip(got, clean):
      assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------------------------------------
# 8. the full val_1 shape
# ---------------------------------------------------------------------------------------------
def test_full_val1_shape_equals_group_rank(dev):
  from cmhse_amd import _lib, ops, synthetic
  counts = synthetic.anet_like_spec(4917).num_clips
  B, n = len(counts), sum(counts)
  assert n == 17502
  a, b = synthetic.correlated_embeddings(n, 1024, seed=3)
  c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  diag = np.arange(B)
  lib = _lib.load()
  for direction in ('p2v', 'v2p'):
    plan = ops.group_rank_labelled_plan(counts, counts, n, n, diag, direction)
    ws = lib.cmhse_group_rank_labelled_workspace(plan.ctypes.data, plan.size)
    assert 0 < ws < lib.cmhse_group_rank_workspace(B) // 10
  for reduce in ('max', 'mean'):
    rank_v, top1_v, rank_p, top1_p = _host(ops.group_rank(c, s, counts, reduce=reduce))
    for direction, rank, top1 in (('v2p', rank_v, top1_v), ('p2v', rank_p, top1_p)):
      g_rank, g_top1, g_pos = _host(ops.group_rank_labelled(c, s, counts, counts, diag, direction, reduce))
      assert np.array_equal(g_rank, rank), (direction, reduce)
      assert np.array_equal(g_top1, top1), (direction, reduce)
      assert np.array_equal(g_pos, diag), (direction, reduce)
    assert rank_v.max() > 0 and rank_p.max() > 0          # non-trivial ranks


# ---------------------------------------------------------------------------------------------
# 9. evaluation's conventions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_evaluation_diagonal_equals_group_i2t_t2i(dev, reduce):
  from cmhse_amd import evaluation
  rng = np.random.RandomState(9)
  nclips = [int(x) for x in rng.randint(1, 9, 120)]
  ncaps = [int(x) for x in rng.randint(1, 9, 120)]
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=40)
  pairs = np.stack([np.arange(120), np.arange(120)], axis=1)
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  want = evaluation.group_i2t_t2i(c.cpu().numpy(), s.cpu().numpy(), nclips, ncaps, reduce=reduce)
  got = evaluation.group_i2t_t2i_labelled(c.cpu().numpy(), s.cpu().numpy(), nclips, ncaps, pairs, reduce=reduce)
  for (w_rep, w_top1, w_ranks), (g_rep, g_top1, g_ranks) in zip(want, got):
    assert g_rep == w_rep
    for g, w in ((g_top1, w_top1), (g_ranks, w_ranks)):
      assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == (120,) and np.array_equal(g, w)
  # device tensors in: device tensors out, the same values and reports
  dgot = evaluation.group_i2t_t2i_labelled(c, s, nclips, ncaps, torch.from_numpy(pairs), reduce=reduce)
  for (w_rep, w_top1, w_ranks), (g_rep, g_top1, g_ranks) in zip(want, dgot):
    assert g_rep == w_rep
    for g, w in ((g_top1, w_top1), (g_ranks, w_ranks)):
      assert g.is_cuda and g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_evaluation_two_annotation_sets(dev, reduce):
  """A val_1 + val_2 shaped problem: 150 videos, 300 paragraphs, paragraph j <-> video j % 150."""
  from cmhse_amd import evaluation
  rng = np.random.RandomState(13)
  nclips = [int(x) for x in rng.randint(1, 9, 150)]
  ncaps = [int(x) for x in rng.randint(1, 9, 300)]
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=44)
  ids = ['v%d' % i for i in range(150)]
  pairs = evaluation.pairs_from_ids(ids, ids + ids)
  assert pairs.shape == (300, 2)
  G = _group_scores_rect(c, s, nclips, ncaps, reduce)
  want_v = group_labelled_reference(G, 'v2p', np.arange(0, 301, 2),
                                    np.stack([np.arange(150), np.arange(150) + 150], axis=1).ravel())
  want_p = group_labelled_reference(G, 'p2v', np.arange(301), np.arange(300) % 150)
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  (rep_v, top1_v, ranks_v), (rep_p, top1_p, ranks_p) = evaluation.group_i2t_t2i_labelled(
      c.cpu().numpy(), s.cpu().numpy(), nclips, ncaps, pairs, reduce=reduce)
  for arr, want, n in ((ranks_v, want_v[0], 150), (top1_v, want_v[1], 150), (ranks_p, want_p[0], 300),
                       (top1_p, want_p[1], 300)):
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.shape == (n,)
    assert np.array_equal(arr, want)
  assert rep_v == evaluation.report_from_ranks(want_v[0].astype(np.float64))
  assert rep_p == evaluation.report_from_ranks(want_p[0].astype(np.float64))
  # one direction through group_rank_labelled: NumPy in / out, then tensors in / device tensors out
  rep, top1, ranks = evaluation.group_rank_labelled(c.cpu().numpy(), s.cpu().numpy(), nclips, ncaps,
                                                    np.arange(300) % 150, 'p2v', reduce)
  assert rep == rep_p and np.array_equal(top1, top1_p) and np.array_equal(ranks, ranks_p)
  assert top1.dtype == np.float64 and ranks.dtype == np.float64
  rep, top1, ranks = evaluation.group_rank_labelled(c, s, nclips, ncaps, [[i, i + 150] for i in range(150)], 'v2p',
                                                    reduce)
  assert rep == rep_v and top1.is_cuda and ranks.is_cuda and top1.dtype == torch.int32 and ranks.dtype == torch.int32
  assert np.array_equal(top1.cpu().numpy(), want_v[1]) and np.array_equal(ranks.cpu().numpy(), want_v[0])
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
