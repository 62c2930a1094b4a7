"""Group-wise video <-> paragraph scores and ranking (cmhse_group_scores / cmhse_group_rank,
ops.group_scores / ops.group_rank, evaluation.group_i2t_t2i) on the MI355X.

The expected G is the contract restated on the stored clip x caption matrix of ops.cosine_sim:
block max, or the block's fp32 scores summed in fp64 sequentially in row-major order / count
(test_group_rank_cpu.numpy_group_scores); ranks and top-1 are sim_rank's rules applied to it."""
import numpy as np
import pytest
import torch

from test_group_rank_cpu import numpy_group_scores

pytestmark = pytest.mark.gpu


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=gen))


def _ranks_from_G(G):
  """(rank_v2p, top1_v2p, rank_p2v, top1_p2v) of a stored G, NumPy int64."""
  G = np.asarray(G)
  d = np.diag(G)
  rank_v = (G > d[:, None]).sum(axis=1)
  rank_p = (G > d[None, :]).sum(axis=0)
  return rank_v, G.argmax(axis=1), rank_p, G.argmax(axis=0)      # argmax: the first maximum


def _bits_equal(a, b):
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# every pattern a naive 64 / 128-row tiling would split, counts of 1, and num_caps != num_clips
STRADDLE = [63, 2, 64, 1, 127, 1, 3, 128, 65, 1, 1, 62, 5, 120, 9]


def _cases():
  rng = np.random.RandomState(11)
  return [
      ('B1', [5], [3], 64),
      ('B1_single_row', [1], [1], 30),
      ('ragged', list(rng.randint(1, 30, 50)), None, 1024),
      ('straddle', STRADDLE, STRADDLE[::-1], 1024),
      ('caps_differ_D30', list(rng.randint(1, 12, 80)), list(rng.randint(1, 12, 80)), 30),
      ('ones', [1] * 200, list(rng.randint(1, 4, 200)), 96),
      ('B300', list(rng.randint(1, 30, 300)), list(rng.randint(1, 30, 300)), 1024),
  ]


CASES = _cases()


def _inputs(dev, nclips, ncaps, d, seed=0):
  ncaps = nclips if ncaps is None else ncaps
  return _rand(dev, int(sum(nclips)), d, seed + 1), _rand(dev, int(sum(ncaps)), d, seed + 2), ncaps


@pytest.mark.parametrize('name,nclips,ncaps,d', CASES, ids=[c[0] for c in CASES])
def test_group_scores_max_bit_identical_to_cosine_sim_blocks(dev, name, nclips, ncaps, d):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  G = ops.group_scores(c, s, nclips, ncaps, reduce='max')
  assert G.shape == (len(nclips), len(nclips)) and G.dtype == torch.float32
  scores = ops.cosine_sim(c, s).cpu().numpy()
  oc = np.concatenate([[0], np.cumsum(nclips)[:-1]])
  os_ = np.concatenate([[0], np.cumsum(ncaps)[:-1]])
  want = np.maximum.reduceat(np.maximum.reduceat(scores, oc, axis=0), os_, axis=1)
  assert _bits_equal(G.cpu().numpy(), want)


@pytest.mark.parametrize('name,nclips,ncaps,d', CASES, ids=[c[0] for c in CASES])
def test_group_scores_mean_bit_identical_to_restatement(dev, name, nclips, ncaps, d):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  G = ops.group_scores(c, s, nclips, ncaps, reduce='mean')
  want = numpy_group_scores(ops.cosine_sim(c, s).cpu().numpy(), nclips, ncaps, 'mean')
  got = G.cpu().numpy()
  assert _bits_equal(got, want), 'differ in %d entries' % int((got != want).sum())


@pytest.mark.parametrize('max_violation', [False, True])
def test_group_scores_equal_training_loss_reduced(dev, max_violation):
  """A training-size batch, every block <= 256 entries: G is the loss's `reduced` bit for bit."""
  from cmhse_amd import ops
  rng = np.random.RandomState(5)
  counts = [int(x) for x in rng.randint(1, 17, 128)]
  n = sum(counts)
  c, s = _rand(dev, n, 1024, 21), _rand(dev, n, 1024, 22)
  _, st = ops.groupwise_fwd(c, s, counts, counts, 0.2, max_violation, False)
  G = ops.group_scores(c, s, counts, counts, reduce='max' if max_violation else 'mean')
  assert _bits_equal(G.cpu().numpy(), st['reduced'].cpu().numpy())


@pytest.mark.parametrize('reduce', ['max', 'mean'])
@pytest.mark.parametrize('name,nclips,ncaps,d', CASES, ids=[c[0] for c in CASES])
def test_group_rank_equals_ranks_of_stored_G(dev, name, nclips, ncaps, d, reduce):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, nclips, ncaps, d)
  G = ops.group_scores(c, s, nclips, ncaps, reduce=reduce).cpu().numpy()
  got = ops.group_rank(c, s, nclips, ncaps, reduce=reduce)
  for t in got:
    assert t.dtype == torch.int32 and t.shape == (len(nclips),) and t.is_cuda
  for g, w, what in zip(got, _ranks_from_G(G), ['rank_v2p', 'top1_v2p', 'rank_p2v', 'top1_p2v']):
    assert np.array_equal(g.cpu().numpy(), w), what


def test_group_rank_tie_rule(dev):
  """Duplicated paragraphs tie exactly: top-1 goes to the smallest index, ties do not count."""
  from cmhse_amd import ops
  nclips = [3, 2, 4, 1, 5, 2]
  c = _rand(dev, sum(nclips), 64, 31)
  base = _rand(dev, 3, 64, 32)
  s = torch.cat([base, base]).contiguous()        # paragraphs j and j + 3 hold the same caption
  ncaps = [1] * 6
  G = ops.group_scores(c, s, nclips, ncaps, 'max').cpu().numpy()
  assert _bits_equal(G[:, :3], G[:, 3:])
  got = [t.cpu().numpy() for t in ops.group_rank(c, s, nclips, ncaps, 'max')]
  want = _ranks_from_G(G)
  for g, w in zip(got, want):
    assert np.array_equal(g, w)
  assert (got[1] < 3).all()


def _segment_ref(scores, rid, cid, B, how):
  """Block reductions of a stored [Nc, Ns] matrix with torch segment ops (rows, then columns)."""
  if how == 'amax':
    t = torch.full((B, scores.shape[1]), -float('inf'), dtype=scores.dtype, device=scores.device)
    t.scatter_reduce_(0, rid[:, None].expand_as(scores), scores, 'amax', include_self=False)
    g = torch.full((B, B), -float('inf'), dtype=scores.dtype, device=scores.device)
    g.scatter_reduce_(1, cid[None, :].expand_as(t), t, 'amax', include_self=False)
    return g
  t = torch.zeros(B, scores.shape[1], dtype=scores.dtype, device=scores.device).index_add_(0, rid, scores)
  return torch.zeros(B, B, dtype=scores.dtype, device=scores.device).index_add_(1, cid, t)


def test_group_rank_full_size(dev):
  """val_1 shape: anet_like_spec(4917) counts, 17 502 correlated clip / caption rows of 1024."""
  from cmhse_amd import ops, synthetic
  counts = synthetic.anet_like_spec(4917).num_clips
  B, n = len(counts), sum(counts)
  assert n == 17502
  a, b = synthetic.correlated_embeddings(n, 1024, seed=3)
  c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  ids = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))
  scores = ops.cosine_sim(c, s)

  # 'max': G and every rank bit for bit against cosine_sim + scatter_reduce('amax')
  G_ref = _segment_ref(scores, ids, ids, B, 'amax').cpu().numpy()
  G = ops.group_scores(c, s, counts, reduce='max')
  assert _bits_equal(G.cpu().numpy(), G_ref)
  want = _ranks_from_G(G_ref)
  got = [t.cpu().numpy() for t in ops.group_rank(c, s, counts, reduce='max')]
  for g, w, what in zip(got, want, ['rank_v2p', 'top1_v2p', 'rank_p2v', 'top1_p2v']):
    assert np.array_equal(g, w), what
  assert got[0].max() > 0 and got[2].max() > 0 and np.median(got[0]) < B / 4   # non-trivial ranks

  # 'mean': within 2^-22 relative of the fp64 block means of the same fp32 scores
  cnt = torch.tensor(counts, dtype=torch.float64, device=dev)
  M_ref = (_segment_ref(scores.double(), ids, ids, B, 'sum') / (cnt[:, None] * cnt[None, :])).cpu().numpy()
  del scores
  torch.cuda.empty_cache()
  Gm = ops.group_scores(c, s, counts, reduce='mean').cpu().numpy().astype(np.float64)
  assert (np.abs(Gm - M_ref) <= 2.0 ** -22 * np.abs(M_ref) + 1e-15).all()
  rank_v, _, rank_p, _ = [t.cpu().numpy() for t in ops.group_rank(c, s, counts, reduce='mean')]
  d = np.diag(M_ref)
  gap = np.abs(M_ref - d[:, None])
  np.fill_diagonal(gap, np.inf)
  clear_v = gap.min(axis=1) > 1e-6
  gap = np.abs(M_ref - d[None, :])
  np.fill_diagonal(gap, np.inf)
  clear_p = gap.min(axis=0) > 1e-6
  assert clear_v.mean() > 0.5 and clear_p.mean() > 0.5
  assert np.array_equal(rank_v[clear_v], (M_ref > d[:, None]).sum(axis=1)[clear_v])
  assert np.array_equal(rank_p[clear_p], (M_ref > d[None, :]).sum(axis=0)[clear_p])


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_group_i2t_t2i_reports(dev, reduce):
  from cmhse_amd import evaluation, ops
  rng = np.random.RandomState(9)
  nclips = [int(x) for x in rng.randint(1, 9, 120)]
  ncaps = [int(x) for x in rng.randint(1, 9, 120)]
  c, s, _ = _inputs(dev, nclips, ncaps, 256, seed=40)
  want = [x.cpu().numpy() for x in ops.group_rank(c, s, nclips, ncaps, reduce)]
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  (rep_v, top1_v, ranks_v), (rep_p, top1_p, ranks_p) = evaluation.group_i2t_t2i(
      c.cpu().numpy(), s.cpu().numpy(), nclips, ncaps, reduce=reduce)
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
  for arr in (top1_v, ranks_v, top1_p, ranks_p):
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float64
  assert rep_v == evaluation.report_from_ranks(want[0].astype(np.float64))
  assert rep_p == evaluation.report_from_ranks(want[2].astype(np.float64))
  assert np.array_equal(ranks_v, want[0]) and np.array_equal(top1_v, want[1])
  assert np.array_equal(ranks_p, want[2]) and np.array_equal(top1_p, want[3])
  # device tensors in: device tensors out, the same values and reports
  (drep_v, dtop1_v, dranks_v), (drep_p, dtop1_p, dranks_p) = evaluation.group_i2t_t2i(
      c, s, nclips, ncaps, reduce=reduce)
  assert dranks_v.is_cuda and dtop1_p.is_cuda
  assert drep_v == rep_v and drep_p == rep_p
  assert np.array_equal(dranks_p.cpu().numpy(), want[2]) and np.array_equal(dtop1_v.cpu().numpy(), want[1])
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_group_calls_repeat_bitwise(dev, reduce):
  from cmhse_amd import ops
  c, s, ncaps = _inputs(dev, STRADDLE * 6, None, 1024, seed=50)
  g0 = ops.group_scores(c, s, STRADDLE * 6, reduce=reduce).cpu().numpy()
  r0 = [t.cpu().numpy() for t in ops.group_rank(c, s, STRADDLE * 6, reduce=reduce)]
  for _ in range(3):
    assert _bits_equal(ops.group_scores(c, s, STRADDLE * 6, reduce=reduce).cpu().numpy(), g0)
    for g, w in zip(ops.group_rank(c, s, STRADDLE * 6, reduce=reduce), r0):
      assert np.array_equal(g.cpu().numpy(), w)
