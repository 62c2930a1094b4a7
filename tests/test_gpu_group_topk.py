"""Group-wise top-K retrieval (cmhse_group_topk / ops.group_topk / evaluation.group_retrieve) on the
MI355X.

The expected result is a stable descending sort of the columns (p2v: the videos of each paragraph) or
rows (v2p: the paragraphs of each video) of ops.group_scores' G — np.lexsort((index, -score)) —
truncated to K; indices are compared exactly and scores bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_group_rank import CASES, STRADDLE, _inputs, _rand

pytestmark = pytest.mark.gpu

TOPK_CASES = CASES + [('all_ones', [1] * 300, [1] * 300, 64),
                      ('straddle_128', STRADDLE + [128, 128, 1], STRADDLE[::-1] + [1, 128, 128], 256)]


def _sorted(G, direction, k):
  """(scores float32 [Bq, k], index int64 [Bq, k]): each query's gallery sorted by score descending,
  then index ascending."""
  M = np.asarray(G, dtype=np.float32)
  M = M.T if direction == 'p2v' else M            # rows: queries
  idx = np.broadcast_to(np.arange(M.shape[1]), M.shape)
  order = np.lexsort((idx, -M), axis=-1)[:, :k]
  return np.take_along_axis(M, order, axis=1), order


def _assert_same(got, want):
  (gs, gi), (ws, wi) = got, want
  gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
  assert gs.shape == ws.shape and gi.shape == wi.shape
  assert np.array_equal(gi, wi), 'indices differ in %d places' % int((gi != wi).sum())
  assert np.array_equal(gs.view(np.int32), np.ascontiguousarray(ws, np.float32).view(np.int32)), \
      'scores differ in their bits'


def _ks(gallery):
  return sorted({min(k, gallery) for k in (1, 10, 128)} | ({gallery} if gallery <= 128 else set()))


@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('name,nclips,ncaps,d', TOPK_CASES, ids=[c[0] for c in TOPK_CASES])
def test_square_cases_vs_sorted_G(dev, name, nclips, ncaps, d, reduce):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  G = ops.group_scores(c, s, nclips, ncaps, reduce=reduce).cpu().numpy()
  B = len(nclips)
  for direction in ('p2v', 'v2p'):
    for k in _ks(B):
      got = ops.group_topk(c, s, nclips, ncaps, k, direction=direction, reduce=reduce)
      assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[0].is_cuda
      assert got[0].shape == (B, k) and got[1].shape == (B, k)
      _assert_same(got, _sorted(G, direction, k))


def _rows_of(x, counts, groups):
  """The rows of the given groups (in that order) and their counts."""
  off = np.concatenate([[0], np.cumsum(counts)])
  rows = np.concatenate([np.arange(off[g], off[g + 1]) for g in groups])
  return x[torch.from_numpy(rows).to(x.device)].contiguous(), [int(counts[g]) for g in groups]


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_rectangular_subsets(dev, reduce):
  """Query subsets (strided, contiguous) against a gallery slice: the sort of the G sub-matrix, with
  gallery indices renumbered from 0."""
  from cmhse_amd import ops
  rng = np.random.RandomState(17)
  B = 400
  nclips = [int(x) for x in rng.randint(1, 30, B)]
  ncaps = [int(x) for x in rng.randint(1, 30, B)]
  c, s, _ = _inputs(dev, nclips, ncaps, 512, seed=40)
  G = ops.group_scores(c, s, nclips, ncaps, reduce=reduce).cpu().numpy()
  queries = {'strided': np.arange(3, B, 7), 'slice': np.arange(101, 230)}
  gallery = np.arange(37, 311)
  for qname, qsel in queries.items():
    # p2v: paragraphs qsel against the videos of the gallery slice
    cq, cq_n = _rows_of(s, ncaps, qsel)
    cg, cg_n = _rows_of(c, nclips, gallery)
    for k in (1, 50, 128):
      got = ops.group_topk(cg, cq, cg_n, cq_n, k, direction='p2v', reduce=reduce)
      _assert_same(got, _sorted(G[np.ix_(gallery, qsel)], 'p2v', k))
    # v2p: videos qsel against the paragraphs of the gallery slice
    vq, vq_n = _rows_of(c, nclips, qsel)
    pg, pg_n = _rows_of(s, ncaps, gallery)
    for k in (1, 50, 128):
      got = ops.group_topk(vq, pg, vq_n, pg_n, k, direction='v2p', reduce=reduce)
      _assert_same(got, _sorted(G[np.ix_(qsel, gallery)], 'v2p', k))


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_tie_rule_duplicated_gallery(dev, reduce):
  """Duplicated gallery groups (identical rows) tie exactly and come back in ascending index order."""
  from cmhse_amd import ops
  rng = np.random.RandomState(23)
  base = [int(x) for x in rng.randint(1, 9, 60)]
  vids = _rand(dev, sum(base), 128, 51)
  ncaps = [int(x) for x in rng.randint(1, 9, 70)]
  paras = _rand(dev, sum(ncaps), 128, 52)
  # p2v: video j, j + 60, j + 120 hold the same clips
  c3, n3 = torch.cat([vids, vids, vids]).contiguous(), base * 3
  scores, index = ops.group_topk(c3, paras, n3, ncaps, 30, direction='p2v', reduce=reduce)
  first = index[:, :3].long().cpu().numpy()
  assert (first % 60 == first[:, :1] % 60).all()          # the best video's three copies first ...
  assert (np.diff(first, axis=1) == 60).all()             # ... in ascending index order
  sc = scores.cpu().numpy()
  assert np.array_equal(sc[:, 0], sc[:, 2])
  _assert_same((scores, index), _sorted(_group_scores_rect(c3, paras, n3, ncaps, reduce), 'p2v', 30))
  # v2p: paragraph j and j + 70 hold the same captions
  p2, m2 = torch.cat([paras, paras]).contiguous(), ncaps * 2
  got = ops.group_topk(vids, p2, base, m2, 40, direction='v2p', reduce=reduce)
  _assert_same(got, _sorted(_group_scores_rect(vids, p2, base, m2, reduce), 'v2p', 40))
  top = got[1][:, :2].long().cpu().numpy()
  assert (top[:, 1] == top[:, 0] + 70).all()


def _group_scores_rect(c, s, nclips, ncaps, reduce):
  """G [Bv, Bp] of a rectangular problem from the square group_scores: both sets padded with
  one-row groups to the same count (the extra rows / columns are dropped)."""
  from cmhse_amd import ops
  Bv, Bp = len(nclips), len(ncaps)
  B = max(Bv, Bp)
  pad_c = torch.zeros(B - Bv, c.shape[1], device=c.device)
  pad_s = torch.zeros(B - Bp, s.shape[1], device=s.device)
  G = ops.group_scores(torch.cat([c, pad_c]).contiguous(), torch.cat([s, pad_s]).contiguous(),
                       list(nclips) + [1] * (B - Bv), list(ncaps) + [1] * (B - Bp), reduce=reduce)
  return G.cpu().numpy()[:Bv, :Bp]


@pytest.mark.parametrize('direction', ['p2v', 'v2p'])
def test_query_stripes_concatenate(dev, direction):
  from cmhse_amd import ops
  rng = np.random.RandomState(29)
  nclips = [int(x) for x in rng.randint(1, 20, 700)]
  ncaps = [int(x) for x in rng.randint(1, 20, 500)]
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=60)
  whole = ops.group_topk(c, s, nclips, ncaps, 64, direction=direction, reduce='mean')
  q, qn = (s, ncaps) if direction == 'p2v' else (c, nclips)
  off = np.concatenate([[0], np.cumsum(qn)])
  parts = []
  for a, b in [(0, 1), (1, 130), (130, 131), (131, len(qn))]:
    stripe = q[int(off[a]):int(off[b])]
    args = (c, stripe, nclips, qn[a:b]) if direction == 'p2v' else (stripe, s, qn[a:b], ncaps)
    parts.append(ops.group_topk(*args, 64, direction=direction, reduce='mean'))
  assert torch.equal(torch.cat([p[1] for p in parts]), whole[1])
  assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), whole[0].view(torch.int32))


def _merge_by_key(parts, k):
  """Host merge of gallery chunks' results: (score desc, global index asc), the kernel's key order."""
  sc = np.concatenate([p[0] for p in parts], axis=1)
  ix = np.concatenate([p[1] for p in parts], axis=1)
  order = np.lexsort((ix, -sc), axis=-1)[:, :k]
  return np.take_along_axis(sc, order, 1), np.take_along_axis(ix, order, 1)


def test_gallery_split_merges_to_single_call(dev):
  """2000 query paragraphs against 40 000 videos in one call, and in four gallery chunks merged on
  the host by key."""
  from cmhse_amd import ops
  rng = np.random.RandomState(31)
  nclips = [int(x) for x in rng.randint(1, 7, 40000)]
  ncaps = [int(x) for x in rng.randint(1, 7, 2000)]
  c, s, _ = _inputs(dev, nclips, ncaps, 128, seed=70)
  k = 50
  whole = ops.group_topk(c, s, nclips, ncaps, k, direction='p2v', reduce='max')
  off = np.concatenate([[0], np.cumsum(nclips)])
  parts = []
  for a, b in [(0, 9000), (9000, 9100), (9100, 27000), (27000, 40000)]:
    sc, ix = ops.group_topk(c[int(off[a]):int(off[b])], s, nclips[a:b], ncaps, k, direction='p2v', reduce='max')
    parts.append((sc.cpu().numpy(), ix.cpu().numpy().astype(np.int64) + a))
  ms, mi = _merge_by_key(parts, k)
  assert np.array_equal(whole[1].cpu().numpy(), mi)
  assert np.array_equal(whole[0].cpu().numpy().view(np.int32), ms.view(np.int32))


def test_full_val1_shape(dev):
  """4917 videos, 17 502 x 17 502 x 1024: K = 50 against the sorted G, K = 1 against group_rank's
  top-1, both directions, both reductions."""
  from cmhse_amd import ops, synthetic
  counts = synthetic.anet_like_spec(4917).num_clips
  a, b = synthetic.correlated_embeddings(sum(counts), 1024, seed=3)
  c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  for reduce in ('max', 'mean'):
    G = ops.group_scores(c, s, counts, counts, reduce=reduce)
    _, top1_v2p, _, top1_p2v = ops.group_rank(c, s, counts, counts, reduce=reduce)
    for direction, top1 in (('p2v', top1_p2v), ('v2p', top1_v2p)):
      M = G.t() if direction == 'p2v' else G
      want_s, want_i = torch.sort(M, dim=1, descending=True, stable=True)   # ties: ascending index
      got = ops.group_topk(c, s, counts, counts, 50, direction=direction, reduce=reduce)
      assert torch.equal(got[1], want_i[:, :50].to(torch.int32))
      assert torch.equal(got[0].view(torch.int32), want_s[:, :50].contiguous().view(torch.int32))
      one = ops.group_topk(c, s, counts, counts, 1, direction=direction, reduce=reduce)
      assert torch.equal(one[1][:, 0], top1)


def test_math_mode_changes_no_bit(dev):
  from cmhse_amd import ops
  nclips, ncaps, d = CASES[3][1], CASES[3][2], CASES[3][3]
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  want = ops.group_topk(c, s, nclips, ncaps, 10, direction='v2p', reduce='mean')
  old = ops.math_mode()
  try:
    ops.set_math_mode('bf16x3')
    got = ops.group_topk(c, s, nclips, ncaps, 10, direction='v2p', reduce='mean')
  finally:
    ops.set_math_mode(old)
  assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


def test_repeat_calls_identical(dev):
  from cmhse_amd import ops
  rng = np.random.RandomState(37)
  nclips = [int(x) for x in rng.randint(1, 12, 900)]
  ncaps = [int(x) for x in rng.randint(1, 12, 1100)]
  c, s, _ = _inputs(dev, nclips, ncaps, 1024, seed=80)
  runs = [ops.group_topk(c, s, nclips, ncaps, 100, direction='p2v', reduce='max') for _ in range(3)]
  for r in runs[1:]:
    assert torch.equal(r[1], runs[0][1]) and torch.equal(r[0].view(torch.int32), runs[0][0].view(torch.int32))


def test_group_retrieve_conventions(dev):
  from cmhse_amd import evaluation, ops
  rng = np.random.RandomState(41)
  nclips = [int(x) for x in rng.randint(1, 10, 150)]
  c, s, _ = _inputs(dev, nclips, nclips, 256, seed=90)
  stats = dict(evaluation.CACHE_STATS)
  last = evaluation._LAST_ENCODE[0]
  want = ops.group_topk(c, s, nclips, nclips, 10, direction='p2v', reduce='mean')
  # NumPy in, NumPy out (num_caps defaults to num_clips)
  sc, ix = evaluation.group_retrieve(c.cpu().numpy(), s.cpu().numpy(), nclips, k=10, direction='p2v',
                                     reduce='mean')
  assert isinstance(sc, np.ndarray) and isinstance(ix, np.ndarray)
  assert sc.dtype == np.float32 and ix.dtype == np.int64 and sc.shape == ix.shape == (150, 10)
  assert np.array_equal(ix, want[1].cpu().numpy()) and np.array_equal(sc, want[0].cpu().numpy())
  # tensors in, device tensors out
  ts, ti = evaluation.group_retrieve(c, s, nclips, nclips, k=10, direction='p2v', reduce='mean')
  assert ts.is_cuda and ti.is_cuda and ts.dtype == torch.float32 and ti.dtype == torch.int32
  assert torch.equal(ti, want[1]) and torch.equal(ts.view(torch.int32), want[0].view(torch.int32))
  v = evaluation.group_retrieve(c, s, nclips, k=5, direction='v2p')
  assert torch.equal(v[1], ops.group_topk(c, s, nclips, nclips, 5, direction='v2p')[1])
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
