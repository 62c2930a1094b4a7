"""Labelled ranking (cmhse_sim_rank_labelled / ops.sim_rank_labelled / evaluation.rank_labelled,
i2t_t2i_labelled) on the MI355X.

Unless a test says otherwise the expected values come from the stored score matrix of
ops.cosine_sim (whose entries every scoring kernel reproduces bit for bit) through the NumPy
statement of the contract in test_rank_labelled_cpu.py, and are compared by exact integer equality
over all rows, ties included."""
import numpy as np
import pytest
import torch

from test_rank_labelled_cpu import labelled_reference, random_labels

pytestmark = pytest.mark.gpu


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.randn(n, d, device=dev, generator=gen)


def _check(q, g, off, idx, row0=0, nrows=None):
  """ops.sim_rank_labelled against the stored matrix: every output, every row; returns them."""
  from cmhse_amd import ops
  rank, top1, best_pos, score = ops.sim_rank_labelled(q, g, (off, idx), row0, nrows, return_score=True)
  for t in (rank, top1, best_pos):
    assert t.dtype == torch.int32 and t.is_cuda
  S = ops.cosine_sim(q, g).cpu().numpy()
  hi = S.shape[0] if nrows is None else row0 + nrows
  off = np.asarray(off)
  w_rank, w_top1, w_pos, w_score = labelled_reference(S[row0:hi], off[row0:hi + 1] - off[row0],
                                                      np.asarray(idx)[off[row0]:off[hi]])
  np.testing.assert_array_equal(rank.cpu().numpy(), w_rank)
  np.testing.assert_array_equal(top1.cpu().numpy(), w_top1)
  np.testing.assert_array_equal(best_pos.cpu().numpy(), w_pos)
  np.testing.assert_array_equal(score.cpu().numpy().view(np.int32), w_score.view(np.int32))
  return rank, top1, best_pos


SHAPES = [(1, 1, 8), (129, 300, 64), (257, 400, 30), (515, 515, 1024), (300, 128, 64), (64, 5000, 1024)]


@pytest.mark.parametrize('n,m,d', SHAPES)
def test_one_random_target_per_query(dev, n, m, d):
  q, g = _rand(dev, n, d, 1 + n), _rand(dev, m, d, 2 + m)
  target = np.random.RandomState(n + m).randint(0, m, size=n)
  _check(q, g, np.arange(n + 1), target)


@pytest.mark.parametrize('n,m,d', SHAPES)
def test_one_to_five_random_positives(dev, n, m, d):
  q, g = _rand(dev, n, d, 3 + n), _rand(dev, m, d, 4 + m)
  off, idx = random_labels(np.random.RandomState(n * m), n, m, 1, 5)
  _check(q, g, off, idx)


@pytest.mark.parametrize('n,m,d', SHAPES)
def test_a_query_with_every_gallery_row_positive(dev, n, m, d):
  q, g = _rand(dev, n, d, 5 + n), _rand(dev, m, d, 6 + m)
  who = n // 2
  lists = [[int(t)] for t in np.random.RandomState(n).randint(0, m, size=n)]
  lists[who] = list(range(m))
  off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
  rank, top1, best_pos = _check(q, g, off, np.concatenate(lists))
  assert int(rank[who]) == 0 and int(best_pos[who]) == int(top1[who])


def test_the_three_label_forms_give_one_result(dev):
  from cmhse_amd import ops
  q, g = _rand(dev, 70, 64, 7), _rand(dev, 90, 64, 8)
  target = np.random.RandomState(5).randint(0, 90, size=70)
  want = ops.sim_rank_labelled(q, g, target)
  for form in (target.tolist(), torch.from_numpy(target).to(dev), (np.arange(71), target),
               [[int(t)] for t in target]):
    got = ops.sim_rank_labelled(q, g, form)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
  with pytest.raises(ValueError, match='query row 3'):
    ops.sim_rank_labelled(q, g, [0, 1, 2, 90] + [0] * 66)


@pytest.mark.parametrize('n,m,d', [(515, 515, 1024), (300, 777, 256)])
def test_identity_labels_equal_sim_rank(dev, n, m, d):
  from cmhse_amd import ops
  q, g = _rand(dev, n, d, 9), _rand(dev, m, d, 10)
  rank, top1, best_pos = ops.sim_rank_labelled(q, g, np.arange(n))
  w_rank, w_top1 = ops.sim_rank(q, g)
  assert torch.equal(rank, w_rank) and torch.equal(top1, w_top1)
  assert best_pos.tolist() == list(range(n))


def test_identity_labels_equal_sim_rank_4917(dev):
  from cmhse_amd import ops, synthetic
  a, b = synthetic.correlated_embeddings(4917)
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  for x, y in ((q, g), (g, q)):
    rank, top1, _ = ops.sim_rank_labelled(x, y, np.arange(4917))
    w_rank, w_top1 = ops.sim_rank(x, y)
    assert torch.equal(rank, w_rank) and torch.equal(top1, w_top1)
  assert 1000 < int((rank == 0).sum()) < 3000        # a non-trivial rank distribution


def test_tie_rule_duplicated_gallery(dev):
  """Every gallery row six times: the copies of a positive tie it exactly and are not counted; the
  best positive is the smallest index among the tied positives."""
  from cmhse_amd import ops
  base = _rand(dev, 50, 64, 7)
  g = base[torch.arange(300, device=dev) % 50].contiguous()      # row r = base row r % 50
  q = _rand(dev, 70, 64, 8)
  rows = np.random.RandomState(3).randint(0, 50, size=70)
  S = ops.cosine_sim(q, base).cpu().numpy()
  above = (S > S[np.arange(70), rows][:, None]).sum(1) * 6        # six copies of every better base row
  # one copy as the positive (the fourth): its five twins are not counted
  rank, top1, best_pos = _check(q, g, np.arange(71), rows + 150)
  np.testing.assert_array_equal(rank.cpu().numpy(), above)
  np.testing.assert_array_equal(best_pos.cpu().numpy(), rows + 150)
  assert bool((top1 < 50).all())
  # several copies, listed in descending order: the smallest index among them
  idx = np.stack([rows + 250, rows + 100, rows + 200], axis=1).reshape(-1)
  rank, _, best_pos = _check(q, g, 3 * np.arange(71), idx)
  np.testing.assert_array_equal(rank.cpu().numpy(), above)
  np.testing.assert_array_equal(best_pos.cpu().numpy(), rows + 100)


def test_zero_query_row(dev):
  q = _rand(dev, 5, 96, 9)
  q[2] = 0.0
  g = _rand(dev, 700, 96, 10)
  rank, top1, best_pos = _check(q, g, np.array([0, 1, 2, 5, 6, 7]), np.array([3, 3, 650, 9, 400, 3, 3]))
  assert int(rank[2]) == 0 and int(top1[2]) == 0 and int(best_pos[2]) == 9   # all scores 0


@pytest.mark.parametrize('parts', [2, 3, 8])
def test_stripes_concatenate(dev, parts):
  from cmhse_amd import ops
  q, g = _rand(dev, 1000, 256, 11), _rand(dev, 3000, 256, 12)
  off, idx = random_labels(np.random.RandomState(parts), 1000, 3000, 1, 4)
  full = ops.sim_rank_labelled(q, g, (off, idx), return_score=True)
  bounds = np.linspace(0, 1000, parts + 1).astype(int)
  pieces = [ops.sim_rank_labelled(q, g, (off, idx), row0=int(lo), nrows=int(hi - lo), return_score=True)
            for lo, hi in zip(bounds[:-1], bounds[1:])]
  for k in range(3):
    assert torch.equal(torch.cat([p[k] for p in pieces]), full[k])
  assert torch.equal(torch.cat([p[3] for p in pieces]).view(torch.int32), full[3].view(torch.int32))
  _check(q, g, off, idx, row0=int(bounds[1]), nrows=int(bounds[2] - bounds[1]))
  empty = ops.sim_rank_labelled(q, g, (off, idx), row0=1000, nrows=0)
  assert all(t.numel() == 0 for t in empty)


def test_many_positives(dev):
  """256 queries x 20 000 gallery rows, 40 positives each: 80 pair tiles, three and a fifth queries
  to a tile, so most tiles end inside a query's list."""
  q, g = _rand(dev, 256, 1024, 13), _rand(dev, 20000, 1024, 14)
  off, idx = random_labels(np.random.RandomState(40), 256, 20000, 40, 40)
  assert off[-1] == 10240 and any(off[k] % 128 for k in range(1, 256))
  _check(q, g, off, idx)


def test_ignores_bf16x3_mode(dev):
  from cmhse_amd import ops
  q, g = _rand(dev, 200, 1024, 15), _rand(dev, 900, 1024, 16)
  off, idx = random_labels(np.random.RandomState(2), 200, 900, 1, 3)
  want = ops.sim_rank_labelled(q, g, (off, idx))
  ops.set_math_mode('bf16x3')
  try:
    got = ops.sim_rank_labelled(q, g, (off, idx))
  finally:
    ops.set_math_mode('fp32')
  assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_evaluation_rank_labelled(dev):
  from cmhse_amd import ops
  from cmhse_amd.evaluation import CACHE_STATS, rank_labelled, report_from_ranks
  rng = np.random.RandomState(3)
  q = rng.standard_normal((90, 128)).astype(np.float32)
  g = rng.standard_normal((400, 128)).astype(np.float32)
  off, idx = random_labels(rng, 90, 400, 1, 3)
  lists = [idx[off[i]:off[i + 1]].tolist() for i in range(90)]
  stats = dict(CACHE_STATS)
  w_rank, w_top1, _ = ops.sim_rank_labelled(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), lists)
  report, top1, ranks = rank_labelled(q, g, lists)
  assert isinstance(top1, np.ndarray) and isinstance(ranks, np.ndarray)
  assert top1.dtype == np.float64 and ranks.dtype == np.float64
  np.testing.assert_array_equal(ranks, w_rank.cpu().numpy())
  np.testing.assert_array_equal(top1, w_top1.cpu().numpy())
  assert report == report_from_ranks(ranks)
  t_report, t_top1, t_ranks = rank_labelled(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), (off, idx))
  assert t_top1.is_cuda and t_ranks.is_cuda
  assert torch.equal(t_ranks, w_rank) and torch.equal(t_top1, w_top1) and t_report == report
  with pytest.raises(ValueError, match='query row 0 has no positive'):
    rank_labelled(q, g, [[]] + lists[1:])
  assert CACHE_STATS == stats


def test_evaluation_i2t_t2i_labelled(dev):
  from cmhse_amd import ops
  from cmhse_amd.evaluation import (CACHE_STATS, csr_from_pairs, i2t_t2i, i2t_t2i_labelled, pairs_from_ids,
                                    report_from_ranks)
  rng = np.random.RandomState(4)
  v = rng.standard_normal((60, 128)).astype(np.float32)
  p = rng.standard_normal((100, 128)).astype(np.float32)
  ids_v = ['v%d' % i for i in range(60)]
  ids_p = ids_v + ['v%d' % i for i in rng.permutation(60)[:40]]   # 40 videos have a second paragraph
  pairs = pairs_from_ids(ids_v, ids_p)
  assert pairs.shape == (100, 2)
  stats = dict(CACHE_STATS)
  vd, pd = torch.from_numpy(v).to(dev), torch.from_numpy(p).to(dev)
  csr_i, csr_t = csr_from_pairs(pairs, 60, 100)
  w_i = ops.sim_rank_labelled(vd, pd, csr_i)
  w_t = ops.sim_rank_labelled(pd, vd, csr_t)
  (r_i, top1_i, ranks_i), (r_t, top1_t, ranks_t) = i2t_t2i_labelled(v, p, pairs)
  for got, want in ((ranks_i, w_i[0]), (top1_i, w_i[1]), (ranks_t, w_t[0]), (top1_t, w_t[1])):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want.cpu().numpy())
  assert r_i == report_from_ranks(ranks_i) and r_t == report_from_ranks(ranks_t)
  (d_i, dtop1_i, dranks_i), (d_t, dtop1_t, dranks_t) = i2t_t2i_labelled(vd, pd, torch.from_numpy(pairs))
  assert torch.equal(dranks_i, w_i[0]) and torch.equal(dtop1_i, w_i[1])
  assert torch.equal(dranks_t, w_t[0]) and torch.equal(dtop1_t, w_t[1])
  assert d_i == r_i and d_t == r_t
  # identity pairs: what i2t_t2i returns, arrays and report dictionaries
  sq = p[:60]
  eye = np.stack([np.arange(60), np.arange(60)], axis=1)
  got, want = i2t_t2i_labelled(v, sq, eye), i2t_t2i(v, sq)
  for (g_rep, g_top1, g_ranks), (w_rep, w_top1, w_ranks) in zip(got, want):
    assert g_rep == w_rep
    np.testing.assert_array_equal(g_top1, w_top1)
    np.testing.assert_array_equal(g_ranks, w_ranks)
    assert g_top1.dtype == w_top1.dtype and g_ranks.dtype == w_ranks.dtype
  with pytest.raises(ValueError, match='caption row 99 appears in no pair'):
    i2t_t2i_labelled(v, p, pairs[pairs[:, 1] != 99])
  assert CACHE_STATS == stats


# ---------------------------------------------------------------------------------------------
# the two-annotation-set shape against float64
# ---------------------------------------------------------------------------------------------
def two_set_problem():
  """4917 videos, 4917 + 4885 paragraphs (ActivityNet Captions' val_1 and val_2 sizes): the second
  set annotates a sorted random subset of the videos.  (v, p, keep) float32 / indices."""
  rng = np.random.RandomState(0)
  n, n2, dim, sigma = 4917, 4885, 1024, 3.0
  z = rng.standard_normal((n, dim))
  keep = np.sort(rng.permutation(n)[:n2])

  def view(zz):                       # float64 until the final cast
    x = zz + sigma * rng.standard_normal(zz.shape)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
  v, p1, p2 = view(z), view(z), view(z[keep])
  return v, np.concatenate([p1, p2]), keep


def fp64_expected(S64, off, idx, gap=1e-6):
  """(rank, kept) from a float64 score matrix: the labelled rank of every row, and whether no other
  score lies within `gap` of the row's threshold (min over j != best_pos of |S64[i, j] - thr| >= gap)."""
  n = S64.shape[0]
  rank = np.empty(n, dtype=np.int64)
  kept = np.empty(n, dtype=bool)
  for i in range(n):
    pos = idx[off[i]:off[i + 1]]
    best = pos[np.argmax(S64[i, pos])]
    thr = S64[i, best]
    rank[i] = np.count_nonzero(S64[i] > thr)
    dist = np.abs(S64[i] - thr)
    dist[best] = np.inf
    kept[i] = dist.min() >= gap
  return rank, kept


def test_two_annotation_sets_against_float64(dev):
  """The one test whose yardstick is independent of this library's kernels: ranks from the float64
  product of the float32 inputs, both directions.  A row is left out only if, in float64, some other
  score lies within 1e-6 of its threshold (fp32 summation order can legitimately flip such a compare;
  1e-6 is about ten times the distance measured between the exact path and float64); every other row
  must match exactly, and at most 2 % of a direction's rows may be left out.  Measured on the CPU in
  NumPy with this generator: 17 of 4917 video -> paragraph rows (0.35 %) and 69 of 9802 paragraph ->
  video rows (0.70 %) are left out; R@1 45.6 % and 33.5 %."""
  from cmhse_amd.evaluation import csr_from_pairs, i2t_t2i_labelled
  v, p, keep = two_set_problem()
  n, m = len(v), len(p)
  pairs = np.concatenate([np.stack([np.arange(n), np.arange(n)], 1), np.stack([keep, n + np.arange(len(keep))], 1)])
  (off_v, idx_v), (off_p, idx_p) = csr_from_pairs(pairs, n, m)
  assert off_v[-1] == m and set(np.diff(off_v).tolist()) == {1, 2} and (np.diff(off_p) == 1).all()
  (rep_v, _, ranks_v), (rep_p, _, ranks_p) = i2t_t2i_labelled(v, p, pairs)
  S64 = v.astype(np.float64) @ p.astype(np.float64).T
  for name, S, off, idx, ranks, rep in (('v2p', S64, off_v, idx_v, ranks_v, rep_v),
                                        ('p2v', np.ascontiguousarray(S64.T), off_p, idx_p, ranks_p, rep_p)):
    want, kept = fp64_expected(S, off, idx)
    left_out = int((~kept).sum())
    wrong = int((ranks[kept] != want[kept]).sum())
    print('%s: %d of %d rows left out (%.2f %%), %d of the kept rows differ, R@1 %.1f %% (float64: %.1f %%)'
          % (name, left_out, len(kept), 100.0 * left_out / len(kept), wrong, rep['r1'],
             100.0 * np.mean(want == 0)))
    assert left_out <= 0.02 * len(kept)
    np.testing.assert_array_equal(ranks[kept], want[kept])
    # a non-trivial rank distribution: zeros, or anything constant, could not pass by accident
    assert 20.0 < rep['r1'] < 70.0 and rep['r1'] < rep['r5'] < rep['r10'] and rep['medr'] >= 2
    assert abs(rep['r1'] - 100.0 * np.mean(want == 0)) < 1.0
