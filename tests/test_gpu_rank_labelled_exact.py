"""Certified labelled ranking (cmhse_sim_rank_labelled_exact / ops.sim_rank_labelled_exact /
evaluation.rank_labelled_exact / i2t_t2i_labelled_exact) on the MI355X.

The expected values come from a float64 score matrix through the NumPy statement of the contract in
test_rank_labelled_exact_cpu.py and are compared by exact integer equality over all rows.  Every fixture's
gap condition (no column within 1e-11 of a row's threshold unless its gallery row is bit-identical to the best
positive's) is asserted on the CPU, here or in that file: any fixed float64 summation order then makes the same
comparisons, the kernel's included."""
import numpy as np
import pytest
import torch

from test_rank_exact_cpu import GAP, NEAR_TIE_SHAPES, min_gap
from test_rank_labelled_exact_cpu import (RANDOM_SHAPES, VAL_N, csr_of, labelled_exact_reference, labelled_min_gap,
                                          near_tie_case, random_case, validation_case)

pytestmark = pytest.mark.gpu


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.randn(n, d, device=dev, generator=gen)


def _dev(dev, *arrays):
  return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(*tensors):
  return [t.cpu().numpy().astype(np.int64) for t in tensors]


def _run(q, g, lists, row0=0, nrows=None, score=False):
  """(rank_lo, rank_hi, top1, best_pos, resolved[, best_score]) with the types checked."""
  from cmhse_amd import ops
  out = ops.sim_rank_labelled_exact(q, g, csr_of(lists), row0, nrows, return_score=score)
  assert len(out) == (6 if score else 5)
  for t in out[:5]:
    assert t.dtype == torch.int32 and t.is_cuda and t.shape == out[0].shape
  if score:
    assert out[5].dtype == torch.float64 and out[5].is_cuda and out[5].shape == out[0].shape
  return out


def _check(out, want):
  """rank_lo, rank_hi, best_pos against the reference (lo, hi, best, thr); best_score when returned."""
  lo, hi, _, best, resolved = _host(*out[:5])
  np.testing.assert_array_equal(lo, want[0])
  np.testing.assert_array_equal(hi, want[1])
  np.testing.assert_array_equal(best, want[2])
  if len(out) == 6:
    err = np.abs(out[5].cpu().numpy() - want[3]).max() if want[3].size else 0.0
    assert err <= GAP, err
  return resolved


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_ties_rank_as_in_float64(dev, n, d):
  q, g, S, lists, want = near_tie_case(n, d)
  q, g = _dev(dev, q, g)
  resolved = _check(_run(q, g, lists, score=True), want)
  assert (resolved >= 1).all(), resolved.min()
  print('near-tie %d x %d with labels: resolved per row %d .. %d' % (n, d, resolved.min(), resolved.max()))


def test_fp32_ranks_differ_on_the_near_ties(dev):
  """What the certified call is for: ops.sim_rank_labelled (the same rows and labels, fp32 scores) ranks some
  row of the near-tie fixtures differently from float64."""
  from cmhse_amd import ops
  differ, other = {}, {}
  for n, d in NEAR_TIE_SHAPES:
    q, g, S, lists, want = near_tie_case(n, d)
    q, g = _dev(dev, q, g)
    rank, _, best = ops.sim_rank_labelled(q, g, csr_of(lists))
    differ[(n, d)] = int(np.count_nonzero(rank.cpu().numpy() != want[0]))
    other[(n, d)] = int(np.count_nonzero(best.cpu().numpy() != want[2]))
  print('rows where sim_rank_labelled differs from the float64 rank:', differ, '; from its best positive:', other)
  assert sum(differ.values()) > 0


@pytest.mark.parametrize('n,m,d', RANDOM_SHAPES)
def test_random_rows_not_normalised(dev, n, m, d):
  from cmhse_amd import ops
  q, g, S, lists, want = random_case(n, m, d)
  if m > 1:
    assert labelled_min_gap(S, g, lists) > GAP
  q, g = _dev(dev, q, g)
  out = _run(q, g, lists, score=True)
  resolved = _check(out, want)
  assert torch.equal(out[2], ops.sim_rank_labelled(q, g, csr_of(lists))[1])     # top1: the fp32 call's, unchanged
  assert (resolved >= 1).all() and (resolved <= m).all()


@pytest.mark.parametrize('n,m,d', [(257, 400, 30), (515, 515, 1024)])
def test_results_do_not_depend_on_the_tolerance(dev, tune, n, m, d):
  q, g, S, lists, want = random_case(n, m, d)
  q, g = _dev(dev, q, g)
  outs = {}
  for scale in (1, 16, 1 << 20):
    tune(rank_exact_tol_scale=scale)
    outs[scale] = _run(q, g, lists, score=True)
  for scale in (16, 1 << 20):
    for k in (0, 1, 3, 5):                                          # rank_lo, rank_hi, best_pos, best_score
      assert torch.equal(outs[scale][k], outs[1][k]), (scale, k)
    assert torch.equal(outs[scale][2], outs[1][2])                  # (and top1)
    assert bool((outs[scale][4] >= outs[1][4]).all())
  assert bool((outs[1 << 20][4] >= outs[16][4]).all())
  # at 2^20 the float64 path has ranked every column, and it equals the reference
  resolved = _check(outs[1 << 20], want)
  assert (resolved == m).all()
  print('%d x %d x %d: resolved in all %d / %d / %d at scale 1 / 16 / 2^20'
        % (n, m, d, int(outs[1][4].sum()), int(outs[16][4].sum()), int(outs[1 << 20][4].sum())))


@pytest.mark.parametrize('which', ['random 515 x 515 x 1024', 'near-tie 260 x 1024'])
def test_identity_labels_equal_the_diagonal_call(dev, which):
  """P_i = {i}: two kernels that share only dot64 give the same interval."""
  from cmhse_amd import ops
  q, g = (random_case(515, 515, 1024) if which.startswith('random') else near_tie_case(260, 1024))[:2]
  q, g = _dev(dev, q, g)
  n = q.shape[0]
  out = _run(q, g, [[i] for i in range(n)])
  lo, hi, _, _ = ops.sim_rank_exact(q, g)
  assert torch.equal(out[0], lo) and torch.equal(out[1], hi)
  assert torch.equal(out[3], torch.arange(n, dtype=torch.int32, device=dev))
  print('%s, identity labels: %d tied rows' % (which, int((hi != lo).sum())))


def test_collapsed_model(dev):
  """All embeddings equal: one positive each says first / last; every row a positive says first, both ways."""
  x = _rand(dev, 1, 64, 5).expand(200, 64).contiguous()
  lo, hi, _, best, resolved = _host(*_run(x, x.clone(), [[i] for i in range(200)]))
  assert (lo == 0).all() and (hi == 199).all() and (resolved == 200).all()
  assert best.tolist() == list(range(200))
  lo, hi, _, best, resolved = _host(*_run(x, x.clone(), [list(range(200))] * 200))
  assert (lo == 0).all() and (hi == 0).all() and (best == 0).all() and (resolved == 200).all()


def test_stripes_concatenate(dev):
  q, g = _rand(dev, 300, 64, 31), _rand(dev, 400, 64, 32)
  # (bit-identical gallery rows: exact ties, and resolved pairs, in every stripe)
  g[350] = g[120]
  g[10] = g[299]
  rng = np.random.RandomState(33)
  # query i owns column i and up to two columns past every planted duplicate; rows 10, 120 and 299 own their
  # column alone, so its copy (columns 299, 350 and 10) is a tied negative
  lists = [sorted({i} | set(rng.randint(351, 400, size=0 if i in (10, 120, 299) else rng.randint(0, 3)).tolist()))
           for i in range(300)]
  assert {len(P) for P in lists} == {1, 2, 3}
  S = q.cpu().numpy().astype(np.float64) @ g.cpu().numpy().astype(np.float64).T
  S[:, 350], S[:, 10] = S[:, 120], S[:, 299]
  assert labelled_min_gap(S, g.cpu().numpy(), lists) > GAP
  want = labelled_exact_reference(S, lists)
  whole = _run(q, g, lists, score=True)
  _check(whole, want)
  parts = [_run(q, g, lists, row0, nrows, score=True) for row0, nrows in ((0, 100), (100, 157), (257, 43))]
  for k in range(6):
    assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
  assert np.flatnonzero(want[1] > want[0]).tolist() == [10, 120, 299] and int((want[1] - want[0]).sum()) == 3
  empty = _run(q, g, lists, 300, 0, score=True)
  assert all(t.numel() == 0 for t in empty)


def test_repeated_calls_are_identical(dev):
  q, g, S, lists, want = near_tie_case(260, 1024)
  q, g = _dev(dev, q, g)
  first = [t.clone() for t in _run(q, g, lists, score=True)]
  for _ in range(19):
    again = _run(q, g, lists, score=True)
    assert all(torch.equal(a, b) for a, b in zip(again, first))
  _check(first, want)


def test_unsorted_and_duplicated_lists_are_accepted(dev):
  from cmhse_amd import ops
  q, g, S, lists, want = random_case(129, 300, 64)
  q, g = _dev(dev, q, g)
  messy = [list(P[::-1]) + [int(P[0])] for P in lists]               # descending, the first entry twice
  out = ops.sim_rank_labelled_exact(q, g, messy)
  clean = _run(q, g, lists)
  assert all(torch.equal(a, b) for a, b in zip(out, clean))


def _i2t_fixture():
  """The 150 x 64 fixture of test_gpu_rank_exact.test_i2t_t2i_exact: caption 7 is a copy of caption 2."""
  rng = np.random.RandomState(3)
  caps = rng.standard_normal((150, 64))
  imgs = caps + 0.8 * rng.standard_normal((150, 64))
  caps = (caps / np.linalg.norm(caps, axis=1, keepdims=True)).astype(np.float32)
  imgs = (imgs / np.linalg.norm(imgs, axis=1, keepdims=True)).astype(np.float32)
  caps[7] = caps[2]
  S = imgs.astype(np.float64) @ caps.astype(np.float64).T
  S[:, 7] = S[:, 2]                      # (bit-equal in the oracle too, whatever BLAS does)
  skip = np.arange(150)
  skip[2], skip[7] = 7, 2
  assert min_gap(S, skip=skip) > GAP and min_gap(S.T) > GAP
  return imgs, caps, S


def test_i2t_t2i_labelled_exact(dev):
  from cmhse_amd import evaluation, ops
  from cmhse_amd.evaluation import (CACHE_STATS, i2t_t2i_exact, i2t_t2i_labelled_exact, rank_labelled_exact,
                                    report_from_ranks)
  imgs, caps, S = _i2t_fixture()
  ident = np.stack([np.arange(150), np.arange(150)], axis=1)
  stats, last = dict(CACHE_STATS), evaluation._LAST_ENCODE[0]
  # pairs (i, i): i2t_t2i_exact's result.  NumPy in, NumPy out
  for ties in ('optimistic', 'pessimistic'):
    got = i2t_t2i_labelled_exact(imgs, caps, ident, ties=ties)
    ref = i2t_t2i_exact(imgs, caps, ties=ties)
    for side in (0, 1):
      assert got[side][0] == ref[side][0]
      for k in (1, 2):
        assert isinstance(got[side][k], np.ndarray) and got[side][k].dtype == np.float64
        np.testing.assert_array_equal(got[side][k], ref[side][k])
    assert set(got[2]) == set(ref[2]) == {'i2t', 't2i', 'resolved'}
    for name in ('i2t', 't2i'):
      assert set(got[2][name]) == set(ref[2][name]) == {'report_lo', 'report_hi', 'tied_rows', 'resolved'}
      assert got[2][name]['report_lo'] == ref[2][name]['report_lo']
      assert got[2][name]['report_hi'] == ref[2][name]['report_hi']
      assert got[2][name]['tied_rows'].tolist() == ref[2][name]['tied_rows'].tolist()
    assert got[2]['i2t']['tied_rows'].tolist() == [2, 7] and got[2]['t2i']['tied_rows'].tolist() == []
    assert got[2]['resolved'] == got[2]['i2t']['resolved'] + got[2]['t2i']['resolved'] >= 300
  # the extra pair (2, 7): image 2 owns both copies of its caption — a tied positive is not a tie
  pairs = np.concatenate([ident, [[2, 7]]])
  lists_i = [[i] for i in range(150)]
  lists_i[2] = [2, 7]
  lists_t = [[i] for i in range(150)]
  lists_t[7] = [2, 7]
  want_i, want_t = labelled_exact_reference(S, lists_i), labelled_exact_reference(S.T, lists_t)
  assert labelled_min_gap(S, caps, lists_i) > GAP and labelled_min_gap(S.T, imgs, lists_t) > GAP
  for ties, pick in (('optimistic', 0), ('pessimistic', 1)):
    (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), info = i2t_t2i_labelled_exact(imgs, caps, pairs, ties=ties)
    np.testing.assert_array_equal(ranks_i, want_i[pick])
    np.testing.assert_array_equal(ranks_t, want_t[pick])
    assert rep_i == report_from_ranks(want_i[pick]) and rep_t == report_from_ranks(want_t[pick])
    assert info['i2t']['tied_rows'].tolist() == [7] and info['t2i']['tied_rows'].tolist() == []
    assert info['i2t']['report_lo'] == report_from_ranks(want_i[0])
    assert info['i2t']['report_hi'] == report_from_ranks(want_i[1])
  # top1='exact': the arg-max of the float64 scores, the smaller index on the planted tie
  first = S.copy()
  first[:, 7] = -np.inf                  # (column 7 repeats column 2: the smaller index wins)
  for M in (first, S.T):
    two = np.sort(M, axis=1)[:, -2:]
    assert (two[:, 1] - two[:, 0]).min() > GAP
  (_, top1_i, _), (_, top1_t, _), info = i2t_t2i_labelled_exact(imgs, caps, pairs, top1='exact')
  np.testing.assert_array_equal(top1_i, first.argmax(axis=1))
  np.testing.assert_array_equal(top1_t, S.T.argmax(axis=1))
  assert info['top1_resolved'] >= 300 and 'top1_resolved' not in i2t_t2i_labelled_exact(imgs, caps, pairs)[2]
  # GPU tensors in: top1 and ranks stay on the device
  v, p = _dev(dev, imgs, caps)
  (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), info = i2t_t2i_labelled_exact(v, p, pairs, ties='pessimistic')
  direct_i = ops.sim_rank_labelled_exact(v, p, csr_of(lists_i))
  direct_t = ops.sim_rank_labelled_exact(p, v, csr_of(lists_t))
  for x in (top1_i, ranks_i, top1_t, ranks_t):
    assert x.is_cuda and x.dtype == torch.int32
  assert torch.equal(ranks_i, direct_i[1]) and torch.equal(top1_i, direct_i[2])
  assert torch.equal(ranks_t, direct_t[1]) and torch.equal(top1_t, direct_t[2])
  assert rep_i == report_from_ranks(want_i[1]) and rep_t == report_from_ranks(want_t[1])
  assert info['resolved'] == int(direct_i[4].sum()) + int(direct_t[4].sum())
  # one direction alone: rank_labelled_exact, both forms
  for ties, pick in (('optimistic', 0), ('pessimistic', 1)):
    report, top1, ranks, one = rank_labelled_exact(imgs, caps, lists_i, ties=ties)
    assert isinstance(ranks, np.ndarray) and ranks.dtype == np.float64 and top1.dtype == np.float64
    np.testing.assert_array_equal(ranks, want_i[pick])
    assert report == report_from_ranks(want_i[pick]) and one['tied_rows'].tolist() == [7]
    assert one['report_lo'] == report_from_ranks(want_i[0]) and one['report_hi'] == report_from_ranks(want_i[1])
    assert one['resolved'] == int(direct_i[4].sum()) and 'top1_resolved' not in one
  report, top1, ranks, one = rank_labelled_exact(v, p, lists_i, ties='pessimistic', top1='exact')
  assert ranks.is_cuda and ranks.dtype == torch.int32 and top1.is_cuda and top1.dtype == torch.int32
  assert torch.equal(ranks, direct_i[1]) and one['top1_resolved'] >= 150
  np.testing.assert_array_equal(top1.cpu().numpy(), first.argmax(axis=1))
  assert CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


def test_validation_shape(dev):
  """4917 queries against both copies of their gallery: bit-identical positives, so no tie counts."""
  q, g, S, lists, want = validation_case()
  gap = labelled_min_gap(S, g, lists)
  assert gap > GAP
  assert np.array_equal(want[0], want[1])
  q, g = _dev(dev, q, g)
  resolved = _check(_run(q, g, lists, score=True), want)
  total = int(resolved.sum())
  print('validation shape %d x %d: smallest gap %.3g, resolved %d columns of %d'
        % (VAL_N, 2 * VAL_N, gap, total, VAL_N * 2 * VAL_N))
  assert (resolved >= 2).all()                    # both copies of the best positive
  assert total < 0.01 * VAL_N * 2 * VAL_N
