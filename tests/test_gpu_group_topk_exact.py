"""Certified group-wise top-K (cmhse_group_topk_exact / ops.group_topk_exact / evaluation.group_retrieve(exact=True) /
evaluation.group_i2t_t2i_exact(top1='exact')) on the MI355X against NumPy float64.

The expected lists are test_group_topk_exact_cpu.group_topk_exact_reference of a float64 block-score matrix.  Index
lists are compared exactly on the COMPARABLE queries (comparable_queries: among the first K + 1 float64 scores of
the query every gap is above the fixture's gap, far above what a float64 summation order can move, or exactly zero
between planted bit-identical groups); test_group_topk_exact_cpu.py asserts how few queries that leaves out.
Scores are compared on every query, within float64_noise() of the reference (sorting is 1-Lipschitz in the largest
difference, so the bound holds place by place whatever the order inside a near tie)."""
import functools

import numpy as np
import pytest
import torch

from dirty_alloc import dirty
from test_group_rank_exact_cpu import GROUP_GAP, GROUP_NEAR_TIE_SHAPES, REDUCES, _offsets, block_scores, float64_noise
from test_group_topk_exact_cpu import (DIRECTIONS, FULL_SORT_SHAPES, MAX_LEFT_OUT, comparable_queries,
                                       group_topk_exact_reference, near_tie_case, near_tie_ks, planted_pairs, query_view)
from test_gpu_group_topk import TOPK_CASES as TILING     # the tiling cases of the fp32 call, shape for shape

pytestmark = pytest.mark.gpu


def _dev(dev, x):
  return torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)      # (the cached fixtures are read-only arrays)


def _run(dev, clips, caps, nc, ns, k, direction, reduce):
  """(scores float64 [Bq, k], index int32 [Bq, k], resolved int32 [Bq]) as NumPy, shapes and types asserted."""
  from cmhse_amd import ops
  out = ops.group_topk_exact(_dev(dev, clips), _dev(dev, caps), nc, ns, k, direction=direction, reduce=reduce)
  Bq = len(ns) if direction == 'p2v' else len(nc)
  scores, index, resolved = out
  assert scores.dtype == torch.float64 and scores.is_cuda and tuple(scores.shape) == (Bq, k)
  assert index.dtype == torch.int32 and index.is_cuda and tuple(index.shape) == (Bq, k)
  assert resolved.dtype == torch.int32 and resolved.is_cuda and tuple(resolved.shape) == (Bq,)
  return scores.cpu().numpy(), index.cpu().numpy(), resolved.cpu().numpy()


def _bits(x):
  return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _check(got, Q, k, noise, planted=None, orig=None, gap=GROUP_GAP, what=''):
  """index == the reference on the comparable queries (at least 95 % of them), scores within `noise` of it on all,
  descending, every index a distinct gallery group, k <= resolved <= gallery."""
  scores, index, resolved = got
  want_s, want_i = group_topk_exact_reference(Q, k)
  ok = comparable_queries(Q, k, planted=planted, orig=orig, gap=gap)
  assert np.count_nonzero(~ok) <= MAX_LEFT_OUT * len(ok), (what, int(np.count_nonzero(~ok)), len(ok))
  bad = np.flatnonzero((index[ok] != want_i[ok]).any(axis=1))
  assert bad.size == 0, '%s K=%d: %d of %d comparable queries differ, first %r' % (what, k, bad.size, ok.sum(), bad[:5])
  err = np.abs(scores - want_s)
  assert (err <= noise).all(), (what, k, float(err.max()), noise)
  assert (np.diff(scores, axis=1) <= 0).all()
  assert (index >= 0).all() and (index < Q.shape[1]).all()
  assert all(len(set(r)) == k for r in index.tolist())
  assert (resolved >= k).all() and (resolved <= Q.shape[1]).all(), (what, k, resolved.min(), resolved.max())
  return ok


def _assert_planted_order(scores, index, stride, count):
  """Where both copies of a planted pair are listed: the smaller index first, right in front, bit-equal scores."""
  seen = 0
  for q, row in enumerate(index.tolist()):
    at = {g: p for p, g in enumerate(row)}
    for g, p in at.items():
      if g < count and g + stride in at:
        assert at[g + stride] == p + 1, (q, g, p, at[g + stride])
        assert _bits(scores[q, p]) == _bits(scores[q, p + 1]), (q, g)
        seen += 1
  return seen


# ---------------------------------------------------------------------------------------------
# 1: the near-tie fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', GROUP_NEAR_TIE_SHAPES)
def test_near_tie_fixtures_list_as_in_float64(dev, n, d, max_rows, reduce):
  clips, caps, nc, ns, G64, noise = near_tie_case(n, d, max_rows, reduce)
  B = 6 * n
  ks = sorted(set(near_tie_ks(B) + ([B] if (n, d, max_rows) in FULL_SORT_SHAPES else [])))
  pairs = 0
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    for k in ks:
      got = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      ok = _check(got, Q, k, noise, planted=planted_pairs(n), what='%s %s' % ((n, d, max_rows), direction))
      pairs += _assert_planted_order(got[0], got[1], 5 * n, n)
      print('near-tie %s %s %s K=%d: %d queries left out, resolved per query %d .. %d of %d'
            % ((n, d, max_rows), reduce, direction, k, np.count_nonzero(~ok), got[2].min(), got[2].max(), B))
  assert pairs > 0


@pytest.mark.parametrize('reduce', REDUCES)
def test_fp32_lists_differ_on_the_fixture(dev, reduce):
  """Why the call exists: ops.group_topk on the same rows is the list of one fp32 summation order."""
  from cmhse_amd import ops
  n, d, max_rows = 44, 1024, 5
  clips, caps, nc, ns, G64, _ = near_tie_case(n, d, max_rows, reduce)
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    ok = comparable_queries(Q, 10, planted=planted_pairs(n))
    want = group_topk_exact_reference(Q, 10)[1]
    index = ops.group_topk(_dev(dev, clips), _dev(dev, caps), nc, ns, 10, direction=direction, reduce=reduce)[1]
    differ = int(np.count_nonzero((index.cpu().numpy() != want).any(axis=1) & ok))
    print('fp32 group_topk differs from the float64 list on %d of %d comparable queries (%s, %s)'
          % (differ, ok.sum(), reduce, direction))
    assert differ > 0


# ---------------------------------------------------------------------------------------------
# 2: independent sets (Bv != Bp): a gallery subset against another query subset
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', [(22, 50, 5), (4, 96, 100)])
def test_independent_query_and_gallery_subsets(dev, n, d, max_rows, reduce):
  """Gallery: the groups [2, 6 n - 1) (6 n - 3 of them: no multiple of anything, planted pairs 2 .. n - 1 inside);
  queries: the groups [1, 4 n + 3) of the other side."""
  clips, caps, nc, ns, G64, noise = near_tie_case(n, d, max_rows, reduce)
  oc, os_ = _offsets(nc), _offsets(ns)
  gsel, qsel = np.arange(2, 6 * n - 1), np.arange(1, 4 * n + 3)
  for direction in DIRECTIONS:
    if direction == 'p2v':       # query paragraphs qsel, gallery videos gsel
      c, cn = clips[oc[gsel[0]]:oc[gsel[-1] + 1]], nc[gsel]
      s, sn = caps[os_[qsel[0]]:os_[qsel[-1] + 1]], ns[qsel]
      Q = G64[np.ix_(gsel, qsel)].T
    else:                        # query videos qsel, gallery paragraphs gsel
      c, cn = clips[oc[qsel[0]]:oc[qsel[-1] + 1]], nc[qsel]
      s, sn = caps[os_[gsel[0]]:os_[gsel[-1] + 1]], ns[gsel]
      Q = G64[np.ix_(qsel, gsel)]
    assert len(cn) != len(sn)
    for k in sorted({1, 10, min(50, len(gsel))}):
      got = _run(dev, c, s, cn, sn, k, direction, reduce)
      _check(got, Q, k, noise, planted=planted_pairs(n), orig=gsel, what='subsets %s' % direction)
      # (local gallery index g is group g + 2: local pairs g, g + 5 n with g + 2 < n)
      _assert_planted_order(got[0], got[1], 5 * n, n - 2)


# ---------------------------------------------------------------------------------------------
# 3: the tiling cases of test_gpu_group_topk.py, un-normalised rows; the cross-check with group_rank_exact
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiling_inputs(idx):
  """Rows of norm ~ sqrt(D) and the float64 clip x caption matrix (shared by the two reduce modes; not modified)."""
  _, nc, ns, d = TILING[idx]
  ns = nc if ns is None else ns
  rng = np.random.RandomState(200 + idx)
  clips = rng.standard_normal((int(sum(nc)), d)).astype(np.float32)
  caps = rng.standard_normal((int(sum(ns)), d)).astype(np.float32)
  S64 = clips.astype(np.float64) @ caps.astype(np.float64).T
  scale = float(np.linalg.norm(clips.astype(np.float64), axis=1).max() *
                np.linalg.norm(caps.astype(np.float64), axis=1).max())
  return clips, caps, np.asarray(nc), np.asarray(ns), S64, scale


@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('idx', range(len(TILING)), ids=[c[0] for c in TILING])
def test_tiling_cases_unnormalised_rows(dev, idx, reduce):
  clips, caps, nc, ns, S64, scale = _tiling_inputs(idx)
  d = clips.shape[1]
  G64 = block_scores(S64, nc, ns, reduce)
  noise = float64_noise(S64, nc, ns, d, reduce, scale)
  assert 4 * noise < GROUP_GAP * scale                     # the shape-scaled gap (|a| |b| up to `scale`, not 1)
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    for k in sorted({1, min(10, Q.shape[1]), min(128, Q.shape[1])}):
      got = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      _check(got, Q, k, noise, gap=GROUP_GAP * scale, what='%s %s' % (TILING[idx][0], direction))


@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', FULL_SORT_SHAPES)
def test_full_sort_agrees_with_group_rank_exact(dev, n, d, max_rows, reduce):
  """One block64 serves both calls: on a square case the K = B list of a query holds rank_lo entries strictly above
  the query's own score, and rank_hi - rank_lo more that tie it (the planted duplicate)."""
  from cmhse_amd import ops
  clips, caps, nc, ns, G64, _ = near_tie_case(n, d, max_rows, reduce)
  B = 6 * n
  ranks = [t.cpu().numpy() for t in ops.group_rank_exact(_dev(dev, clips), _dev(dev, caps), nc, ns, reduce)]
  for direction, lo, hi in (('v2p', ranks[0], ranks[1]), ('p2v', ranks[4], ranks[5])):
    scores, index, resolved = _run(dev, clips, caps, nc, ns, B, direction, reduce)
    assert (np.sort(index, axis=1) == np.arange(B)).all() and (resolved == B).all()
    own = scores[index == np.arange(B)[:, None]]                   # the query's own group, once per row
    assert own.shape == (B,)
    assert np.array_equal((scores > own[:, None]).sum(axis=1), lo), direction
    assert np.array_equal((scores == own[:, None]).sum(axis=1) - 1, hi - lo), direction
    assert (hi - lo).sum() == 2 * n


# ---------------------------------------------------------------------------------------------
# 4: the tolerance only moves `resolved`
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', [(22, 64, 5), (4, 96, 100)])
def test_results_do_not_depend_on_the_tolerance(dev, tune, n, d, max_rows, reduce):
  clips, caps, nc, ns, G64, noise = near_tie_case(n, d, max_rows, reduce)
  B = 6 * n
  for direction in DIRECTIONS:
    for k in (1, 10):
      tune(rank_exact_tol_scale=1)
      base = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      _check(base, query_view(G64, direction), k, noise, planted=planted_pairs(n))
      prev = base
      for scale in (16, 1 << 20):
        tune(rank_exact_tol_scale=scale)
        got = _run(dev, clips, caps, nc, ns, k, direction, reduce)
        assert np.array_equal(got[1], base[1]) and np.array_equal(_bits(got[0]), _bits(base[0])), (direction, k, scale)
        assert (got[2] >= prev[2]).all()                     # a wider tolerance rules out no more
        prev = got
      assert (prev[2] == B).all()                            # 2^20, D >= 16: every gallery group


# ---------------------------------------------------------------------------------------------
# 5: a collapsed low level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,reduce', [('equal_counts_random_row', 'max'), ('equal_counts_random_row', 'mean'),
                                         ('ragged_random_row', 'max'), ('ragged_exact_sums', 'max'),
                                         ('ragged_exact_sums', 'mean')])
def test_collapsed_model_lists_the_first_k(dev, kind, reduce):
  """All rows equal.  Bit-identical groups tie exactly (the contract), so every query lists the gallery groups
  0 .. K - 1 with one score.  Under 'max' that holds for ragged counts too (nothing is rounded); under 'mean' groups
  of different counts tie only where the float64 sums are exact (the contract: the sum of n equal terms divided by n
  need not return the term), so the ragged 'mean' case uses a row whose score is 1.0 — its sums n * 1.0 and their
  quotients by n round nothing — and the ragged random row comes under 'max' only."""
  rng = np.random.RandomState(2)
  B = 70
  if kind == 'equal_counts_random_row':
    d, nc, ns = 300, np.full(B, 3), np.full(B, 2)
  else:
    d, nc, ns = 64, rng.randint(1, 9, B), rng.randint(1, 9, B)
  if kind == 'ragged_exact_sums':
    row = np.zeros(d, dtype=np.float32)
    row[[3, 17, 40, 63]] = 0.5
  else:
    row = rng.standard_normal(d).astype(np.float32)
    row /= np.linalg.norm(row)
  clips, caps = np.tile(row, (int(nc.sum()), 1)), np.tile(row, (int(ns.sum()), 1))
  for direction in DIRECTIONS:
    for k in (1, 10, B):
      scores, index, resolved = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      assert (index == np.arange(k)).all(), (direction, k)
      assert (_bits(scores) == _bits(scores[0, 0])).all(), (direction, k)
      assert (resolved == B).all()                           # every tie went through float64
  if kind == 'ragged_exact_sums':
    assert scores[0, 0] == 1.0


# ---------------------------------------------------------------------------------------------
# 6: bit-identical gallery groups at places K and K + 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_tie_across_the_kth_place(dev, reduce):
  """Every gallery group has a bit-identical copy `half` places later, so a query's sorted list runs in pairs and an
  odd K cuts a pair: the smaller index is in, the larger out."""
  rng = np.random.RandomState(8)
  half, Bq, d = 60, 50, 128
  gn, qn = rng.randint(1, 7, half), rng.randint(1, 7, Bq)
  g = rng.standard_normal((int(gn.sum()), d)).astype(np.float32)
  q = rng.standard_normal((int(qn.sum()), d)).astype(np.float32)
  g2, gn2 = np.concatenate([g, g]), np.tile(gn, 2)
  scale = float(np.linalg.norm(g.astype(np.float64), axis=1).max() * np.linalg.norm(q.astype(np.float64), axis=1).max())
  for direction in DIRECTIONS:
    clips, caps, nc, ns = (g2, q, gn2, qn) if direction == 'p2v' else (q, g2, qn, gn2)
    # (from the distinct rows, then gathered: the copies are bit-equal in it whatever BLAS does)
    once = g.astype(np.float64) @ q.astype(np.float64).T
    S64 = np.concatenate([once, once]) if direction == 'p2v' else np.concatenate([once.T, once.T], axis=1)
    Q = query_view(block_scores(S64, nc, ns, reduce), direction)
    assert np.array_equal(Q[:, :half], Q[:, half:])
    noise = float64_noise(S64, nc, ns, d, reduce, scale)
    assert 4 * noise < GROUP_GAP * scale
    for k in (1, 7, 33):
      got = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      ok = _check(got, Q, k, noise, planted=(half, half), gap=GROUP_GAP * scale, what='boundary %s' % direction)
      assert ok.all()
      last = got[1][:, -1]
      assert (last < half).all() and not (got[1] == (last + half)[:, None]).any()
      assert _assert_planted_order(got[0], got[1], half, half) == Bq * (k // 2)


# ---------------------------------------------------------------------------------------------
# 7: query stripes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('direction', DIRECTIONS)
def test_query_stripes_concatenate(dev, direction):
  n, d, max_rows, reduce, k = 34, 300, 5, 'mean', 10
  clips, caps, nc, ns, _, _ = near_tie_case(n, d, max_rows, reduce)
  whole = _run(dev, clips, caps, nc, ns, k, direction, reduce)
  q, qn = (caps, ns) if direction == 'p2v' else (clips, nc)
  off = _offsets(qn)
  parts = []
  for a, b in [(0, 1), (1, 70), (70, 71), (71, len(qn))]:
    stripe = q[off[a]:off[b]]
    args = (clips, stripe, nc, qn[a:b]) if direction == 'p2v' else (stripe, caps, qn[a:b], ns)
    parts.append(_run(dev, *args, k, direction, reduce))
  assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
  assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(whole[0]))
  assert np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])


# ---------------------------------------------------------------------------------------------
# 8: repeatability, and buffers that held something else
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_repeated_and_dirty_calls_give_identical_bits(dev, monkeypatch, reduce):
  clips, caps, nc, ns, _, _ = near_tie_case(34, 300, 5, reduce)
  for direction in DIRECTIONS:
    first = _run(dev, clips, caps, nc, ns, 50, direction, reduce)
    runs = [_run(dev, clips, caps, nc, ns, 50, direction, reduce)]
    for fill in ('ones', 'a5'):
      with monkeypatch.context() as m:
        proxy = dirty(m, fill)
        runs.append(_run(dev, clips, caps, nc, ns, 50, direction, reduce))
        proxy.check_guards('group_topk_exact %s [%s]' % (direction, fill))
        assert len(proxy.blocks) >= 4                        # the three outputs and the workspace came from it
        proxy.release()
    for r in runs:
      assert np.array_equal(r[1], first[1]) and np.array_equal(_bits(r[0]), _bits(first[0]))
      assert np.array_equal(r[2], first[2])


# ---------------------------------------------------------------------------------------------
# 9: well-separated groups: nothing beyond the fp32 list's own K goes through float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_well_separated_groups_resolve_k(dev, reduce):
  """Video i: copies of the axis e_i; paragraph j: copies of sum_i (1 + 0.1 ((37 i + 11 j) mod 70)) e_i.  Every block
  score is one exact component, 0.1 apart from every other of its row and of its column: the tolerance (below
  1e-3 here) rules out all but the fp32 list's own K."""
  from cmhse_amd import ops
  rng = np.random.RandomState(4)
  B, d = 70, 96
  nc, ns = rng.randint(1, 6, B), rng.randint(1, 6, B)
  clips = np.zeros((int(nc.sum()), d), dtype=np.float32)
  clips[np.arange(len(clips)), np.repeat(np.arange(B), nc)] = 1.0
  w = np.zeros((B, d), dtype=np.float32)
  w[:, :B] = 1.0 + 0.1 * ((37 * np.arange(B)[None, :] + 11 * np.arange(B)[:, None]) % 70)
  caps = np.repeat(w, ns, axis=0)
  G64 = w[:, :B].astype(np.float64).T                        # [video i, paragraph j], exact in either precision
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    for k in (1, 10, B):
      got = _run(dev, clips, caps, nc, ns, k, direction, reduce)
      assert (got[2] == k).all(), (direction, k, got[2].min(), got[2].max())
      s32, i32 = ops.group_topk(_dev(dev, clips), _dev(dev, caps), nc, ns, k, direction=direction, reduce=reduce)
      assert np.array_equal(got[1], i32.cpu().numpy())
      assert np.array_equal(got[0], s32.cpu().numpy().astype(np.float64))
      want_s, want_i = group_topk_exact_reference(Q, k)
      assert np.array_equal(got[1], want_i) and np.array_equal(got[0], want_s)


# ---------------------------------------------------------------------------------------------
# 10: evaluation.group_retrieve(exact=...) and evaluation.group_i2t_t2i_exact(top1=...)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_group_retrieve_exact_conventions(dev, reduce):
  from cmhse_amd import evaluation, ops
  n, d, max_rows, k = 22, 64, 5, 10
  clips, caps, nc, ns, G64, noise = near_tie_case(n, d, max_rows, reduce)
  clips, caps = clips.copy(), caps.copy()          # (writable: they go to torch.from_numpy as they are)
  c, s = _dev(dev, clips), _dev(dev, caps)
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  for direction in DIRECTIONS:
    raw = _run(dev, clips, caps, nc, ns, k, direction, reduce)
    _check(raw, query_view(G64, direction), k, noise, planted=planted_pairs(n))
    # NumPy in, NumPy out
    sc, ix = evaluation.group_retrieve(clips, caps, nc, ns, k=k, direction=direction, reduce=reduce, exact=True)
    assert isinstance(sc, np.ndarray) and isinstance(ix, np.ndarray)
    assert sc.dtype == np.float64 and ix.dtype == np.int64 and sc.shape == ix.shape == (6 * n, k)
    assert np.array_equal(ix, raw[1]) and np.array_equal(_bits(sc), _bits(raw[0]))
    # tensors in, device tensors out
    ts, ti = evaluation.group_retrieve(c, s, nc, ns, k=k, direction=direction, reduce=reduce, exact=True)
    assert ts.is_cuda and ti.is_cuda and ts.dtype == torch.float64 and ti.dtype == torch.int32
    assert np.array_equal(ti.cpu().numpy(), raw[1]) and np.array_equal(_bits(ts.cpu().numpy()), _bits(raw[0]))
    # the default (and exact=False) is the fp32 call as it was, bit for bit
    want = ops.group_topk(c, s, nc, ns, k, direction=direction, reduce=reduce)
    for kw in ({}, dict(exact=False)):
      fs, fi = evaluation.group_retrieve(c, s, nc, ns, k=k, direction=direction, reduce=reduce, **kw)
      assert fs.dtype == torch.float32 and torch.equal(fi, want[1])
      assert torch.equal(fs.view(torch.int32), want[0].view(torch.int32))
    hs, hi = evaluation.group_retrieve(clips, caps, nc, ns, k=k, direction=direction, reduce=reduce)
    assert hs.dtype == np.float32 and hi.dtype == np.int64 and np.array_equal(hi, want[1].cpu().numpy())
    assert np.array_equal(hs, want[0].cpu().numpy())
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
  with pytest.raises(ValueError):
    evaluation.group_retrieve(c, s, nc, ns, k=k, exact='yes')


@pytest.mark.parametrize('reduce', REDUCES)
def test_group_i2t_t2i_exact_top1(dev, reduce):
  from cmhse_amd import evaluation, ops
  n, d, max_rows = 22, 64, 5
  clips, caps, nc, ns, G64, _ = near_tie_case(n, d, max_rows, reduce)
  clips, caps = clips.copy(), caps.copy()
  c, s = _dev(dev, clips), _dev(dev, caps)
  B = 6 * n
  ranks = [t.cpu().numpy() for t in ops.group_rank_exact(c, s, nc, ns, reduce)]
  want, res = {}, {}
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    assert comparable_queries(Q, 1, planted=planted_pairs(n)).all()
    want[direction] = group_topk_exact_reference(Q, 1)[1][:, 0]
    res[direction] = int(_run(dev, clips, caps, nc, ns, 1, direction, reduce)[2].sum())
  # the planted tie at the top resolves to the smaller index: some query's best group has a bit-identical copy
  tied_top = sum(int(np.count_nonzero((want[dr] < n) & (query_view(G64, dr)[np.arange(B), want[dr]] ==
                                                        query_view(G64, dr)[np.arange(B), (want[dr] + 5 * n) % B])))
                 for dr in DIRECTIONS)
  assert tied_top > 0
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  # the default keeps today's output: group_rank_exact's uncertified fp32 top1, the same info keys
  (rep_v, top1_v, ranks_v), (rep_p, top1_p, ranks_p), info = evaluation.group_i2t_t2i_exact(clips, caps, nc, ns,
                                                                                           reduce=reduce)
  assert np.array_equal(top1_v, ranks[2]) and np.array_equal(top1_p, ranks[6])
  assert np.array_equal(ranks_v, ranks[0]) and np.array_equal(ranks_p, ranks[4])
  assert sorted(info) == ['p2v', 'resolved', 'v2p']
  assert sorted(info['v2p']) == ['report_hi', 'report_lo', 'resolved', 'tied_rows']
  # top1='exact': the certified arg-max, NumPy out
  (xrep_v, xtop1_v, xranks_v), (xrep_p, xtop1_p, xranks_p), xinfo = evaluation.group_i2t_t2i_exact(
      clips, caps, nc, ns, reduce=reduce, top1='exact')
  assert isinstance(xtop1_v, np.ndarray) and xtop1_v.dtype == np.float64 and xtop1_p.dtype == np.float64
  assert np.array_equal(xtop1_v, want['v2p']) and np.array_equal(xtop1_p, want['p2v'])
  assert np.array_equal(xranks_v, ranks_v) and np.array_equal(xranks_p, ranks_p) and xrep_v == rep_v and xrep_p == rep_p
  assert xinfo['v2p']['top1_resolved'] == res['v2p'] and xinfo['p2v']['top1_resolved'] == res['p2v']
  assert xinfo['top1_resolved'] == res['v2p'] + res['p2v'] and xinfo['resolved'] == info['resolved']
  assert xinfo['v2p']['report_lo'] == info['v2p']['report_lo'] and xinfo['p2v']['resolved'] == info['p2v']['resolved']
  # device tensors in: top1 and ranks stay int32 device tensors
  (_, dtop1_v, dranks_v), (_, dtop1_p, dranks_p), dinfo = evaluation.group_i2t_t2i_exact(
      c, s, nc, ns, reduce=reduce, ties='pessimistic', top1='exact')
  for t in (dtop1_v, dranks_v, dtop1_p, dranks_p):
    assert t.is_cuda and t.dtype == torch.int32
  assert np.array_equal(dtop1_v.cpu().numpy(), want['v2p']) and np.array_equal(dtop1_p.cpu().numpy(), want['p2v'])
  assert np.array_equal(dranks_v.cpu().numpy(), ranks[1]) and np.array_equal(dranks_p.cpu().numpy(), ranks[5])
  assert dinfo['top1_resolved'] == xinfo['top1_resolved']
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(clips, caps, nc, ns, reduce=reduce, top1='best')


# ---------------------------------------------------------------------------------------------
# 11: a mid-size case: panels, the XCD deal and several gallery tiles per panel together
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_size_inputs():
  """2048 videos and 512 paragraphs of 1 .. 8 rows at D = 1024, correlated (a paragraph's video is near it):
  72 clip tiles and 18 caption tiles, so either direction walks several gallery tiles per panel."""
  from cmhse_amd import synthetic
  Bv, Bp, d = 2048, 512, 1024
  rng = np.random.RandomState(6)
  nc, ns = rng.randint(1, 9, Bv), rng.randint(1, 9, Bp)
  a, b = synthetic.correlated_embeddings(Bv, d, seed=5)
  clips = (np.repeat(a, nc, axis=0) + 0.005 * rng.standard_normal((int(nc.sum()), d))).astype(np.float32)
  caps = (np.repeat(b[:Bp], ns, axis=0) + 0.005 * rng.standard_normal((int(ns.sum()), d))).astype(np.float32)
  S64 = clips.astype(np.float64) @ caps.astype(np.float64).T
  scale = float(np.linalg.norm(clips.astype(np.float64), axis=1).max() *
                np.linalg.norm(caps.astype(np.float64), axis=1).max())
  return clips, caps, nc, ns, S64, scale


@pytest.mark.parametrize('reduce', REDUCES)
def test_mid_size_case(dev, reduce):
  clips, caps, nc, ns, S64, scale = _mid_size_inputs()
  G64 = block_scores(S64, nc, ns, reduce)
  noise = float64_noise(S64, nc, ns, clips.shape[1], reduce, scale)
  assert 4 * noise < GROUP_GAP * scale
  for direction in DIRECTIONS:
    Q = query_view(G64, direction)
    got = _run(dev, clips, caps, nc, ns, 50, direction, reduce)
    ok = _check(got, Q, 50, noise, gap=GROUP_GAP * scale, what='mid-size %s' % direction)
    print('mid-size %s %s: %d x %d rows, %d of %d queries left out, resolved per query %d .. %d (mean %.1f) of %d'
          % (reduce, direction, len(clips), len(caps), np.count_nonzero(~ok), len(ok), got[2].min(), got[2].max(),
             got[2].mean(), Q.shape[1]))
