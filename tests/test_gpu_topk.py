"""Top-K retrieval (cmhse_sim_topk / ops.sim_topk / evaluation.retrieve) on the MI355X.

Unless a test says otherwise the expected result is a stable descending sort of the stored score
matrix of ops.cosine_sim, truncated to K, and scores and indices are compared bit for bit."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_common import golden_model

pytestmark = pytest.mark.gpu


def _expected(q, g, k):
  from cmhse_amd import ops
  s, i = torch.sort(ops.cosine_sim(q, g), dim=1, descending=True, stable=True)
  return s[:, :k].contiguous(), i[:, :k].to(torch.int32).contiguous()


def _assert_same(got, want):
  (gs, gi), (ws, wi) = got, want
  assert gs.shape == ws.shape and gi.shape == wi.shape
  assert gs.dtype == torch.float32 and gi.dtype == torch.int32
  assert torch.equal(gi, wi), 'indices differ in %d places' % int((gi != wi).sum())
  assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)), 'scores differ in their bits'


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.randn(n, d, device=dev, generator=gen)


@pytest.mark.parametrize('n,m,d,k', [(1, 1, 8, 1), (129, 300, 64, 5), (257, 400, 30, 128),
                                     (515, 515, 1024, 50), (300, 128, 64, 128), (64, 1000, 1024, 128)])
def test_sim_topk_vs_sorted_cosine_sim(dev, n, m, d, k):
  from cmhse_amd import ops
  q = _rand(dev, n, d, 1 + n)
  g = _rand(dev, m, d, 2 + m)
  _assert_same(ops.sim_topk(q, g, k), _expected(q, g, k))


def test_sim_topk_tie_rule_duplicated_gallery(dev):
  """Equal scores come out in ascending gallery index."""
  from cmhse_amd import ops
  base = _rand(dev, 50, 64, 7)
  g = base[torch.arange(300, device=dev) % 50].contiguous()      # every row six times
  q = _rand(dev, 70, 64, 8)
  scores, index = ops.sim_topk(q, g, 24)
  _assert_same((scores, index), _expected(q, g, 24))
  # the top score of a row is shared by the six copies of one base row, in index order
  first = index[:, :6].long()
  assert torch.equal(first % 50, first[:, :1].expand(-1, 6) % 50)
  assert bool((first[:, 1:] > first[:, :-1]).all())


def test_sim_topk_zero_query_row(dev):
  from cmhse_amd import ops
  q = _rand(dev, 5, 96, 9)
  q[2] = 0.0
  g = _rand(dev, 700, 96, 10)
  scores, index = ops.sim_topk(q, g, 40)
  assert index[2].tolist() == list(range(40))
  assert scores[2].tolist() == [0.0] * 40
  _assert_same((scores, index), _expected(q, g, 40))


def test_sim_topk_agrees_with_sim_rank_4917(dev):
  from cmhse_amd import ops, synthetic
  a, b = synthetic.correlated_embeddings(4917)
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  k = 50
  scores, index = ops.sim_topk(q, g, k)
  rank, top1 = ops.sim_rank(q, g)
  assert torch.equal(index[:, 0], top1)
  d = ops.cosine_sim(q, g)
  diag = d.diagonal()
  rows = torch.arange(4917, device=dev)
  cols = torch.arange(4917, device=dev)
  ties_before = ((d == diag[:, None]) & (cols[None, :] < rows[:, None])).sum(1)
  hit = rank < k
  assert int(hit.sum()) > 1000            # the check below covers most rows
  pos = (index == rows[:, None].to(torch.int32)).float().argmax(1)
  found = (index == rows[:, None].to(torch.int32)).any(1)
  assert bool(found[hit].all())
  assert torch.equal(pos[hit], (rank.long() + ties_before)[hit])
  _assert_same((scores, index), _expected(q, g, k))


@pytest.mark.parametrize('parts', [2, 3, 8])
def test_sim_topk_stripes_concatenate(dev, parts):
  """Row stripes (the unit a sharded evaluation would deal out) give the full call's rows."""
  from cmhse_amd import ops
  q = _rand(dev, 1000, 256, 11)
  g = _rand(dev, 3000, 256, 12)
  k = 17
  full = ops.sim_topk(q, g, k)
  bounds = np.linspace(0, 1000, parts + 1).astype(int)
  pieces = [ops.sim_topk(q, g, k, row0=int(lo), nrows=int(hi - lo)) for lo, hi in zip(bounds[:-1], bounds[1:])]
  _assert_same((torch.cat([p[0] for p in pieces]), torch.cat([p[1] for p in pieces])), full)


def test_sim_topk_large_gallery(dev):
  """256 queries x 200 000 gallery rows, K = 100: many column panels and the merge."""
  from cmhse_amd import ops
  q = _rand(dev, 256, 1024, 13)
  g = _rand(dev, 200000, 1024, 14)
  k = 100
  got = ops.sim_topk(q, g, k)
  cand_s, cand_i = [], []
  for lo in range(0, 200000, 25000):
    s, i = torch.sort(ops.cosine_sim(q, g[lo:lo + 25000]), dim=1, descending=True, stable=True)
    cand_s.append(s[:, :k])
    cand_i.append(i[:, :k] + lo)
  s, order = torch.sort(torch.cat(cand_s, 1), dim=1, descending=True, stable=True)   # chunks in index order
  want = (s[:, :k].contiguous(), torch.gather(torch.cat(cand_i, 1), 1, order)[:, :k].to(torch.int32).contiguous())
  _assert_same(got, want)


def test_sim_topk_ignores_bf16x3_mode(dev):
  from cmhse_amd import ops
  q = _rand(dev, 200, 1024, 15)
  g = _rand(dev, 900, 1024, 16)
  want = ops.sim_topk(q, g, 30)
  ops.set_math_mode('bf16x3')
  try:
    got = ops.sim_topk(q, g, 30)
  finally:
    ops.set_math_mode('fp32')
  _assert_same(got, want)
  _assert_same(got, _expected(q, g, 30))


def test_retrieve_numpy_and_tensors(dev):
  from cmhse_amd import ops
  from cmhse_amd.evaluation import retrieve
  rng = np.random.RandomState(3)
  q = rng.standard_normal((90, 128)).astype(np.float32)
  g = rng.standard_normal((400, 128)).astype(np.float32)
  scores, index = retrieve(q, g, 12)
  assert isinstance(scores, np.ndarray) and isinstance(index, np.ndarray)
  assert scores.dtype == np.float32 and index.dtype == np.int64
  assert scores.shape == (90, 12) and index.shape == (90, 12)
  ws, wi = ops.sim_topk(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), 12)
  np.testing.assert_array_equal(index, wi.cpu().numpy())
  np.testing.assert_array_equal(scores.view(np.int32), ws.cpu().numpy().view(np.int32))
  ts, ti = retrieve(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), 12)
  assert ts.is_cuda and ti.is_cuda
  _assert_same((ts, ti), (ws, wi))
  with pytest.raises(ValueError):
    retrieve(q, g, 0)
  with pytest.raises(ValueError):
    retrieve(q, g[:5], 6)


def test_retrieve_on_encode_data_keeps_the_rank_cache(dev):
  """retrieve on encode_data's own (pinned) arrays, in both directions; i2t / t2i are still served
  from the ranks that encode_data queued."""
  from cmhse_amd import ops, synthetic
  from cmhse_amd.evaluation import CACHE_STATS, encode_data, i2t, retrieve, t2i
  g = load_golden('model_maxout.npz')
  opt, model = golden_model('maxout', g)
  spec = synthetic.ragged_spec(19, seed=6)
  batches = synthetic.make_batches(spec, 5, opt.img_dim, opt.vocab_size, seed=2)
  vid, para, *_ = encode_data(opt, model, synthetic.ListLoader(batches), logging=lambda *a: None)
  k = 7
  for qry, gal in [(para, vid), (vid, para)]:
    scores, index = retrieve(qry, gal, k)
    ws, wi = ops.sim_topk(torch.from_numpy(np.array(qry)).to(dev), torch.from_numpy(np.array(gal)).to(dev), k)
    np.testing.assert_array_equal(index, wi.cpu().numpy())
    np.testing.assert_array_equal(scores.view(np.int32), ws.cpu().numpy().view(np.int32))
    _, top1 = ops.sim_rank(torch.from_numpy(np.array(qry)).to(dev), torch.from_numpy(np.array(gal)).to(dev))
    np.testing.assert_array_equal(index[:, 0], top1.cpu().numpy())
  hits = CACHE_STATS['hits']
  rep_i, top1_i, ranks_i = i2t(vid, para)
  assert CACHE_STATS['hits'] == hits + 1
  rep_t, top1_t, ranks_t = t2i(vid, para)
  assert CACHE_STATS['hits'] == hits + 2
  # what was served equals a fresh ranking of the same matrices
  r_i, t_i = ops.sim_rank(torch.from_numpy(np.array(vid)).to(dev), torch.from_numpy(np.array(para)).to(dev))
  np.testing.assert_array_equal(ranks_i, r_i.cpu().numpy())
  np.testing.assert_array_equal(top1_i, t_i.cpu().numpy())
