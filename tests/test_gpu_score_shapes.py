"""Every tile deal and panel walk of the scoring kernels against references that no product kernel
computes: sim_rank / sim_rank_labelled / sim_rank_exact on the four arms of the XCD-grouped deal
(G = 4, 3, 2 and the plain order), group_scores / group_rank on the same arms, sim_topk and
group_topk with panels of several tiles, uneven panel splits and padded grids.

Each case of score_shapes' tables targets arms by name, and tests/test_score_shapes_cpu.py proves
from the restated launch rules that it lands on them.  Two input families per case:
  lattice   integer rows: every score is exact, so ranks, top-1, top-K lists, returned scores, group
            max and mean are compared bit for bit with int64 NumPy, no row left out — and ties with
            the diagonal and inside the lists are everywhere, at every tile, panel and group edge;
  gaussian  unit-norm rows against float64 under score_shapes.score_bar (gamma_D(2^-24) |a| |b|,
            nothing measured): sim_rank_exact on every row, sim_rank and sim_rank_labelled on the
            rows whose float64 margin exceeds two bars (at most 1 % may fall out), top-K position by
            position with no exclusions, the group scores entry by entry.
Top-K note: a returned index holds the k-th largest float64 score within ONE bar — what the issue of
this file sets; order statistics of scores perturbed by one bar each are guaranteed to two.
(Measured distances: profiles/score_shapes_distances.txt.)"""
import numpy as np
import pytest
import torch

import score_shapes as ss

pytestmark = pytest.mark.gpu

FAMILIES = ('lattice', 'gaussian')
EXCLUDED_MAX = 0.01      # the share of rows a float64 rank comparison may leave out


def _t(x, dev):
  return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(ts):
  torch.cuda.synchronize()
  return [t.cpu().numpy() for t in ts]


def _same(first, again, what):
  for k, (x, y) in enumerate(zip(first, again)):
    assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32)), \
        '%s: output %d differs on a second call' % (what, k)


def _bits(got, want, what):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=np.float32)
  assert got.dtype == np.float32 and got.shape == want.shape, what
  bad = got.view(np.int32) != want.view(np.int32)
  assert not bad.any(), '%s: %d of %d values differ in their bits' % (what, int(bad.sum()), bad.size)


def _ints(got, want, what):
  got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
  assert got.shape == want.shape, what
  bad = got != want
  assert not bad.any(), '%s: %d of %d differ (first at %s: got %s, want %s)' % (
      what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _within(err, bar, what):
  """err <= bar elementwise (bar broadcasts), the largest ratio printed first."""
  ratio = np.max(err / bar)
  print('\nscore_shapes %-58s |diff| %.3e  bar %.3e  ratio %.4f' % (what, np.max(err), np.min(bar), ratio), end='')
  assert ratio <= 1.0, '%s: %.3e over a bar of %.3e' % (what, np.max(err), np.min(bar))


def _excluded(ok, what):
  share = 1.0 - np.count_nonzero(ok) / ok.size
  print('\nscore_shapes %-58s rows left out %.4f %%' % (what, 100 * share), end='')
  assert share <= EXCLUDED_MAX, '%s: the float64 margin leaves out %.2f %% of the rows' % (what, 100 * share)


def _stripe_labels(off, idx, row0, nrows):
  lo, hi = int(off[row0]), int(off[row0 + nrows])
  return off[row0:row0 + nrows + 1] - lo, idx[lo:hi]


def _count_calls(ops, a, b, labels, row0, nrows):
  rank = _np(ops.sim_rank(a, b, row0=row0, nrows=nrows))
  lab = _np(ops.sim_rank_labelled(a, b, labels, row0=row0, nrows=nrows, return_score=True))
  exact = _np(ops.sim_rank_exact(a, b, row0=row0, nrows=nrows))
  return rank, lab, exact


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('case', ss.COUNT_CASES, ids=[c[0] for c in ss.COUNT_CASES])
def test_counting_pass_score_shape(dev, case, family):
  """sim_rank, sim_rank_labelled and sim_rank_exact of one stripe on the deal arm the case names."""
  from cmhse_amd import ops
  name, N, M, D, row0, nrows, corr, _ = case
  a, b = ss.count_inputs(name, family)
  off, idx = ss.positives_of(N, M)
  ad, bd = _t(a, dev), _t(b, dev)
  labels = (off, idx)
  (rank, top1), (lrank, ltop1, lpos, lscore), (lo, hi, etop1, resolved) = first = \
      _count_calls(ops, ad, bd, labels, row0, nrows)
  again = _count_calls(ops, ad, bd, labels, row0, nrows)
  for f, g, what in zip(first, again, ('sim_rank', 'sim_rank_labelled', 'sim_rank_exact')):
    _same(f, g, name + ' ' + what)
  soff, sidx = _stripe_labels(off, idx, row0, nrows)
  rows = a[row0:row0 + nrows]
  tag = '%s %s ' % (name, family)
  if family == 'lattice':
    S = ss.scores_int(rows, b)
    want_rank, want_top1 = ss.rank_reference(S, row0)
    _ints(rank, want_rank, tag + 'sim_rank rank')
    _ints(top1, want_top1, tag + 'sim_rank top1')
    want_lo, want_hi = ss.exact_reference(S, row0)
    _ints(lo, want_lo, tag + 'rank_exact rank_lo')
    _ints(hi, want_hi, tag + 'rank_exact rank_hi (ties)')
    _ints(etop1, want_top1, tag + 'rank_exact top1')
    assert (resolved >= want_hi - want_lo).all(), tag + 'every exact tie goes through float64'
    assert int((want_hi - want_lo).max()) >= 5, 'the lattice ties the diagonal'
    wr, wt, wp, ws = ss.labelled_reference(S, soff, sidx)
    _ints(lrank, wr, tag + 'rank_labelled rank')
    _ints(ltop1, wt, tag + 'rank_labelled top1')
    _ints(lpos, wp, tag + 'rank_labelled best positive')
    _bits(lscore, ws, tag + 'rank_labelled best score')
    return
  S = ss.scores_f64(rows, b)
  bars = ss.row_bars(rows, b, D)
  want_lo, want_hi = ss.exact_reference(S, row0)
  _ints(lo, want_lo, tag + 'rank_exact rank_lo')          # certified: every row
  _ints(hi, want_hi, tag + 'rank_exact rank_hi')
  want_rank, want_top1 = ss.rank_reference(S, row0)
  ok_rank, ok_top = ss.margin_ok(S, bars, row0 + np.arange(nrows))
  _excluded(ok_rank, tag + 'sim_rank rank')
  _excluded(ok_top, tag + 'sim_rank top1')
  _ints(rank[ok_rank], want_rank[ok_rank], tag + 'sim_rank rank')
  _ints(top1[ok_top], want_top1[ok_top], tag + 'sim_rank top1')
  _ints(etop1[ok_top], want_top1[ok_top], tag + 'rank_exact top1')
  wr, wt, wp, ws = ss.labelled_reference(S, soff, sidx)
  ok_lab, _ = ss.margin_ok(S, bars, wp)
  _excluded(ok_lab, tag + 'rank_labelled rank')
  _ints(lrank[ok_lab], wr[ok_lab], tag + 'rank_labelled rank')
  _ints(lpos[ok_lab], wp[ok_lab], tag + 'rank_labelled best positive')
  _ints(ltop1[ok_top], wt[ok_top], tag + 'rank_labelled top1')
  # the best positive's score: that of the returned positive, every row
  _within(np.abs(lscore.astype(np.float64) - S[np.arange(nrows), lpos]), bars, tag + 'rank_labelled best score')


def test_counting_pass_stripes_concatenate(dev):
  """The stripes of one query set are dealt on another arm (G = 4) than the full call (G = 2);
  together they are the full call."""
  from cmhse_amd import ops
  name, N, M, D, cuts = ss.COUNT_STRIPES
  arms = {ss.count_plan(hi - lo, M)['G'] for lo, hi in zip(cuts[:-1], cuts[1:])}
  assert ss.count_plan(N, M)['G'] not in arms, arms
  a, b = ss.gaussian_pair(N, M, D, 5, 2.0)
  ad, bd = _t(a, dev), _t(b, dev)
  labels = ss.positives_of(N, M)
  full = _count_calls(ops, ad, bd, labels, 0, N)
  parts = [_count_calls(ops, ad, bd, labels, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
  for e in range(3):
    joined = [np.concatenate([p[e][k] for p in parts]) for k in range(len(full[e]))]
    _same(full[e], joined, '%s entry point %d' % (name, e))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('case', ss.GROUP_CASES, ids=[c[0] for c in ss.GROUP_CASES])
def test_group_scores_score_shape(dev, case, reduce, family):
  """group_scores and group_rank on the deal arm the case names."""
  from cmhse_amd import ops
  name, nclips, ncaps, D, _ = case
  c, s = ss.group_inputs(name, family)
  cd, sd = _t(c, dev), _t(s, dev)
  G, = first = _np([ops.group_scores(cd, sd, nclips, ncaps, reduce=reduce)])
  _same(first, _np([ops.group_scores(cd, sd, nclips, ncaps, reduce=reduce)]), name + ' group_scores')
  ranks = _np(ops.group_rank(cd, sd, nclips, ncaps, reduce=reduce))
  _same(ranks, _np(ops.group_rank(cd, sd, nclips, ncaps, reduce=reduce)), name + ' group_rank')
  tag = '%s %s %s ' % (name, reduce, family)
  if family == 'lattice':
    want = ss.lattice_group_scores(ss.scores_int(c, s), nclips, ncaps, reduce)
    _bits(G, want, tag + 'group_scores')
    for got, ref, what in zip(ranks, ss.group_rank_reference(want), ('rank v2p', 'top1 v2p', 'rank p2v', 'top1 p2v')):
      _ints(got, ref, tag + 'group_rank ' + what)
    return
  want = ss.f64_group_scores(ss.scores_f64(c, s), nclips, ncaps, reduce)
  bar = ss.score_bar(D, np.linalg.norm(c.astype(np.float64), axis=1).max(),
                     np.linalg.norm(s.astype(np.float64), axis=1).max())
  _within(np.abs(G.astype(np.float64) - want), np.float64(bar), tag + 'group_scores')


def _check_topk_f64(scores, index, S, bars, K, tag):
  """The float64 checks of a top-K result, position by position, no row left out."""
  n, M = S.shape
  top, order = ss.topk_reference(S, min(K + 1, M))
  index = index.astype(np.int64)
  assert index.min() >= 0 and index.max() < M, tag + 'an index outside the gallery'
  own = np.take_along_axis(S, index, axis=1)
  bars = bars[:, None] if np.ndim(bars) else np.float64(bars)
  _within(np.abs(own - top[:, :K]), bars, tag + 'score of the k-th index')
  assert (np.diff(np.sort(index, axis=1), axis=1) != 0).all(), tag + 'an index twice in one row'
  _within(np.abs(scores.astype(np.float64) - own), bars, tag + 'returned score')
  gap = np.full((n, K + 1), np.inf)
  gap[:, 1:top.shape[1]] = top[:, :-1] - top[:, 1:]        # gap[k]: between positions k - 1 and k
  decided = (gap[:, :K] > 2 * bars) & (gap[:, 1:] > 2 * bars)
  print('\nscore_shapes %-58s positions decided beyond two bars %.2f %%' % (tag, 100 * decided.mean()), end='')
  assert decided.mean() > 0.5, tag + 'the inputs decide too few positions'
  bad = decided & (index != order[:, :K])
  assert not bad.any(), '%s%d decided positions hold another index than float64' % (tag, int(bad.sum()))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('case', ss.TOPK_CASES, ids=[c[0] for c in ss.TOPK_CASES])
def test_sim_topk_score_shape(dev, case, family):
  from cmhse_amd import ops
  name, N, M, D, K, row0, nrows, corr, _ = case
  a, b = ss.count_inputs(name, family)
  ad, bd = _t(a, dev), _t(b, dev)
  scores, index = first = _np(ops.sim_topk(ad, bd, K, row0=row0, nrows=nrows))
  _same(first, _np(ops.sim_topk(ad, bd, K, row0=row0, nrows=nrows)), name + ' sim_topk')
  assert scores.shape == index.shape == (nrows, K)
  rows = a[row0:row0 + nrows]
  tag = '%s %s ' % (name, family)
  if family == 'lattice':
    ws, wi = ss.topk_reference(ss.scores_int(rows, b), K)
    _ints(index, wi, tag + 'sim_topk index')
    _bits(scores, ws, tag + 'sim_topk scores')
    assert (ws[:, :-1] == ws[:, 1:]).any() or K == 1, 'the lattice ties inside the lists'
    return
  _check_topk_f64(scores, index, ss.scores_f64(rows, b), ss.row_bars(rows, b, D), K, tag + 'sim_topk ')


def test_sim_topk_stripes_concatenate(dev):
  from cmhse_amd import ops
  name, N, M, D, K, cuts = ss.TOPK_STRIPES
  plans = [ss.topk_plan(hi - lo, M, K) for lo, hi in zip(cuts[:-1], cuts[1:])]
  assert len({p['panels'] for p in plans}) >= 2      # the stripes walk other panels than the full call
  a, b = ss.lattice_rows(N, D, 21), ss.lattice_rows(M, D, 22)
  ad, bd = _t(a, dev), _t(b, dev)
  full = _np(ops.sim_topk(ad, bd, K))
  parts = [_np(ops.sim_topk(ad, bd, K, row0=lo, nrows=hi - lo)) for lo, hi in zip(cuts[:-1], cuts[1:])]
  _same(full, [np.concatenate([p[k] for p in parts]) for k in range(2)], name)
  ws, wi = ss.topk_reference(ss.scores_int(a, b), K)
  _ints(full[1], wi, name + ' index')
  _bits(full[0], ws, name + ' scores')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('case', ss.GTOPK_CASES, ids=[c[0] for c in ss.GTOPK_CASES])
def test_group_topk_score_shape(dev, case, reduce, family):
  from cmhse_amd import ops
  name, nclips, ncaps, D, K, direction, _ = case
  c, s = ss.group_inputs(name, family)
  cd, sd = _t(c, dev), _t(s, dev)
  scores, index = first = _np(ops.group_topk(cd, sd, nclips, ncaps, K, direction=direction, reduce=reduce))
  _same(first, _np(ops.group_topk(cd, sd, nclips, ncaps, K, direction=direction, reduce=reduce)), name + ' group_topk')
  Bq = len(ncaps) if direction == 'p2v' else len(nclips)
  assert scores.shape == index.shape == (Bq, K)
  tag = '%s %s %s ' % (name, reduce, family)
  if family == 'lattice':
    G = ss.lattice_group_scores(ss.scores_int(c, s), nclips, ncaps, reduce)
    Q = (G.T if direction == 'p2v' else G).astype(np.float64)       # (fp32 values, exact in float64)
    ws, wi = ss.topk_reference(Q, K)
    _ints(index, wi, tag + 'group_topk index')
    _bits(scores, ws, tag + 'group_topk scores')
    assert (ws[:, :-1] == ws[:, 1:]).any(), 'the lattice ties inside the lists'
    return
  G = ss.f64_group_scores(ss.scores_f64(c, s), nclips, ncaps, reduce)
  bar = ss.score_bar(D, np.linalg.norm(c.astype(np.float64), axis=1).max(),
                     np.linalg.norm(s.astype(np.float64), axis=1).max())
  _check_topk_f64(scores, index, np.ascontiguousarray(G.T if direction == 'p2v' else G), bar, K, tag + 'group_topk ')
