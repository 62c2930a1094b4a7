"""Certified ranking (cmhse_sim_rank_exact / ops.sim_rank_exact / evaluation.i2t_t2i_exact) on the
MI355X.

The expected ranks come from a float64 score matrix through the NumPy statement of the contract in
test_rank_exact_cpu.py and are compared by exact integer equality over all rows.  Wherever the matrix
comes out of BLAS, the test first asserts on the CPU that every gap between a diagonal score and another
column exceeds 1e-11, far above what the order of a float64 summation can move: any fixed order then gives
the same comparisons, the kernel's included."""
import numpy as np
import pytest
import torch

from test_rank_exact_cpu import GAP, NEAR_TIE_SHAPES, exact_reference, min_gap, near_tie_fixture

pytestmark = pytest.mark.gpu

_NEAR = {}


def _near(n, d):
  """The near-tie fixture of a shape, built once and never changed: (q, g, rank_lo, rank_hi)."""
  if (n, d) not in _NEAR:
    q, g, S = near_tie_fixture(n, d, 7 * n + d)
    _NEAR[(n, d)] = (q, g) + exact_reference(S)
  return _NEAR[(n, d)]


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.randn(n, d, device=dev, generator=gen)


def _host(*tensors):
  return [t.cpu().numpy().astype(np.int64) for t in tensors]


def _run(q, g, row0=0, nrows=None):
  from cmhse_amd import ops
  out = ops.sim_rank_exact(q, g, row0, nrows)
  for t in out:
    assert t.dtype == torch.int32 and t.is_cuda and t.shape == out[0].shape
  return out


def _float64_scores(q, g):
  """q64 @ g64.T of two device matrices, with the gap condition asserted."""
  S = q.cpu().numpy().astype(np.float64) @ g.cpu().numpy().astype(np.float64).T
  if S.shape[1] > 1:
    gap = min_gap(S)
    print('smallest gap to a diagonal score: %.3g' % gap)
    assert gap > GAP
  return S


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_ties_rank_as_in_float64(dev, n, d):
  q, g, want_lo, want_hi = _near(n, d)
  lo, hi, top1, resolved = _host(*_run(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)))
  np.testing.assert_array_equal(lo, want_lo)
  np.testing.assert_array_equal(hi, want_hi)
  # the duplicate and the four near-copies lie inside the tolerance of every row
  assert (resolved >= 5).all(), resolved.min()
  print('near-tie %d x %d: resolved per row %d .. %d' % (n, d, resolved.min(), resolved.max()))


def test_fp32_ranks_differ_on_the_near_ties(dev):
  """What the certified ranks are for: ops.sim_rank (the same rows, fp32 scores) ranks some row of the
  near-tie fixtures differently from float64."""
  from cmhse_amd import ops
  differ = {}
  for n, d in NEAR_TIE_SHAPES:
    q, g, want_lo, _ = _near(n, d)
    rank, _ = ops.sim_rank(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev))
    differ[(n, d)] = int(np.count_nonzero(rank.cpu().numpy() != want_lo))
  print('rows where sim_rank differs from the float64 rank:', differ)
  assert max(differ.values()) > 0


RANDOM_SHAPES = [(1, 1, 8), (129, 300, 64), (257, 400, 30), (515, 515, 1024), (64, 5000, 1024)]


@pytest.mark.parametrize('n,m,d', RANDOM_SHAPES)
def test_random_rows_not_normalised(dev, n, m, d):
  q, g = _rand(dev, n, d, 11 + n), _rand(dev, m, d, 12 + m)
  want_lo, want_hi = exact_reference(_float64_scores(q, g))
  from cmhse_amd import ops
  out = _run(q, g)
  lo, hi, top1, resolved = _host(*out)
  np.testing.assert_array_equal(lo, want_lo)
  np.testing.assert_array_equal(hi, want_hi)
  assert torch.equal(out[2], ops.sim_rank(q, g)[1])                 # top1: sim_rank's, unchanged
  assert (resolved >= 0).all() and (resolved <= m - 1).all()


@pytest.mark.parametrize('n,m,d', [(257, 400, 30), (515, 515, 1024)])
def test_results_do_not_depend_on_the_tolerance(dev, tune, n, m, d):
  q, g = _rand(dev, n, d, 21 + n), _rand(dev, m, d, 22 + m)
  want_lo, want_hi = exact_reference(_float64_scores(q, g))
  outs = {}
  for scale in (1, 16, 1 << 20):
    tune(rank_exact_tol_scale=scale)
    outs[scale] = _run(q, g)
  for scale in (16, 1 << 20):
    for k in range(3):                                              # rank_lo, rank_hi, top1: bit-equal
      assert torch.equal(outs[scale][k], outs[1][k]), (scale, k)
    assert bool((outs[scale][3] >= outs[1][3]).all())
  # at 2^20 the float64 path has ranked every element, and it equals the reference
  lo, hi, _, resolved = _host(*outs[1 << 20])
  assert (resolved == m - 1).all()
  np.testing.assert_array_equal(lo, want_lo)
  np.testing.assert_array_equal(hi, want_hi)
  print('%d x %d x %d: resolved in all %d / %d / %d at scale 1 / 16 / 2^20'
        % (n, m, d, int(outs[1][3].sum()), int(outs[16][3].sum()), int(outs[1 << 20][3].sum())))


def test_collapsed_model(dev):
  """All embeddings equal: the optimistic rank says first, the pessimistic one last."""
  row = _rand(dev, 1, 64, 5)
  x = row.expand(200, 64).contiguous()
  lo, hi, top1, resolved = _host(*_run(x, x.clone()))
  assert (lo == 0).all() and (hi == 199).all() and (resolved == 199).all()


def test_well_separated_input_resolves_nothing(dev):
  from cmhse_amd import ops
  x = torch.nn.functional.normalize(_rand(dev, 300, 64, 6))
  S = _float64_scores(x, x)
  off = S - np.eye(300)
  assert np.abs(off).max() < 0.9 and np.abs(np.diag(off)).max() < 1e-6   # diagonal 1, nothing near it
  lo, hi, top1, resolved = _run(x, x.clone())
  rank, rtop1 = ops.sim_rank(x, x.clone())
  assert int(resolved.abs().sum()) == 0
  assert torch.equal(lo, rank) and torch.equal(hi, rank) and torch.equal(top1, rtop1)
  np.testing.assert_array_equal(lo.cpu().numpy(), exact_reference(S)[0])


def test_stripes_concatenate(dev):
  q, g = _rand(dev, 300, 64, 31), _rand(dev, 400, 64, 32)
  # (bit-identical gallery rows: exact ties, and resolved pairs, in every stripe — rows 10 and 299 tie
  # each other's diagonal, row 120 ties column 350)
  g[350] = g[120]
  g[10] = g[299]
  whole = _run(q, g)
  parts = [_run(q, g, row0, nrows) for row0, nrows in ((0, 100), (100, 157), (257, 43))]
  for k in range(4):
    assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
  lo, hi = _host(whole[0], whole[1])
  assert all(hi[i] == lo[i] + 1 for i in (10, 120, 299)) and int((hi - lo).sum()) == 3
  empty = _run(q, g, 300, 0)
  assert all(t.numel() == 0 for t in empty)


def test_repeated_calls_are_identical(dev):
  q, g, want_lo, want_hi = _near(260, 1024)
  q, g = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
  first = [t.clone() for t in _run(q, g)]
  for _ in range(19):
    again = _run(q, g)
    assert all(torch.equal(a, b) for a, b in zip(again, first))
  np.testing.assert_array_equal(first[0].cpu().numpy(), want_lo)


def test_i2t_t2i_exact(dev):
  from cmhse_amd import evaluation, ops
  from cmhse_amd.evaluation import CACHE_STATS, i2t_t2i_exact, report_from_ranks
  rng = np.random.RandomState(3)
  caps = rng.standard_normal((150, 64))
  imgs = caps + 0.8 * rng.standard_normal((150, 64))
  caps = (caps / np.linalg.norm(caps, axis=1, keepdims=True)).astype(np.float32)
  imgs = (imgs / np.linalg.norm(imgs, axis=1, keepdims=True)).astype(np.float32)
  caps[7] = caps[2]                      # a duplicate caption: images 2 and 7 see an exact tie
  S = imgs.astype(np.float64) @ caps.astype(np.float64).T
  S[:, 7] = S[:, 2]                      # (bit-equal in the oracle too, whatever BLAS does)
  skip = np.arange(150)
  skip[2], skip[7] = 7, 2
  assert min_gap(S, skip=skip) > GAP and min_gap(S.T) > GAP
  want = exact_reference(S), exact_reference(S.T)
  assert want[0][1][2] == want[0][0][2] + 1 and want[0][1][7] == want[0][0][7] + 1
  stats, last = dict(CACHE_STATS), evaluation._LAST_ENCODE[0]
  # NumPy in, NumPy out
  for ties, pick in (('optimistic', 0), ('pessimistic', 1)):
    (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), info = i2t_t2i_exact(imgs, caps, ties=ties)
    for x in (top1_i, ranks_i, top1_t, ranks_t):
      assert isinstance(x, np.ndarray) and x.dtype == np.float64
    np.testing.assert_array_equal(ranks_i, want[0][pick])
    np.testing.assert_array_equal(ranks_t, want[1][pick])
    assert rep_i == report_from_ranks(want[0][pick]) and rep_t == report_from_ranks(want[1][pick])
    for name, w in (('i2t', want[0]), ('t2i', want[1])):
      assert info[name]['report_lo'] == report_from_ranks(w[0])
      assert info[name]['report_hi'] == report_from_ranks(w[1])
    assert info['i2t']['tied_rows'].tolist() == [2, 7] and info['t2i']['tied_rows'].tolist() == []
    assert info['resolved'] == info['i2t']['resolved'] + info['t2i']['resolved'] >= 2
  assert i2t_t2i_exact(imgs, caps)[0][2].tolist() == want[0][0].tolist()      # the default: optimistic
  # GPU tensors in: top1 and ranks stay on the device
  v, p = torch.from_numpy(imgs).to(dev), torch.from_numpy(caps).to(dev)
  (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), info = i2t_t2i_exact(v, p, ties='pessimistic')
  direct_i, direct_t = ops.sim_rank_exact(v, p), ops.sim_rank_exact(p, v)
  for x in (top1_i, ranks_i, top1_t, ranks_t):
    assert x.is_cuda and x.dtype == torch.int32
  assert torch.equal(ranks_i, direct_i[1]) and torch.equal(top1_i, direct_i[2])
  assert torch.equal(ranks_t, direct_t[1]) and torch.equal(top1_t, direct_t[2])
  assert rep_i == report_from_ranks(want[0][1]) and rep_t == report_from_ranks(want[1][1])
  assert info['resolved'] == int(direct_i[3].sum()) + int(direct_t[3].sum())
  assert CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


def test_full_size_correlated_split(dev):
  """The validation shape, both directions, every row against float64."""
  from cmhse_amd import synthetic
  a, b = synthetic.correlated_embeddings(4917)
  S = a.astype(np.float64) @ b.astype(np.float64).T
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  total = 0
  for name, qq, gg, SS in (('a -> b', q, g, S), ('b -> a', g, q, S.T)):
    gap = min_gap(SS)
    assert gap > GAP
    want_lo, want_hi = exact_reference(SS)
    assert np.array_equal(want_lo, want_hi)
    lo, hi, top1, resolved = _host(*_run(qq, gg))
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(hi, want_lo)
    print('correlated 4917 %s: smallest gap %.3g, resolved %d pairs of %d'
          % (name, gap, int(resolved.sum()), 4917 * 4916))
    total += int(resolved.sum())
  print('correlated 4917: resolved %d pairs in both directions' % total)
  assert total < 0.01 * 2 * 4917 * 4916
