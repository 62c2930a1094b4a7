"""Certified top-K retrieval (cmhse_sim_topk_exact / ops.sim_topk_exact / evaluation.retrieve(exact=True) /
evaluation.i2t_t2i_exact(top1='exact')) on the MI355X.

The expected lists come from a float64 score matrix through the NumPy statement of the contract in
test_topk_exact_cpu.py and are compared by exact integer equality over all rows.  Wherever the matrix comes
out of BLAS, the test first asserts on the CPU that every non-zero gap between consecutive entries among the
first K + 1 of each row exceeds 1e-11, far above what the order of a float64 summation can move, and that
the zero gaps belong to bit-identical gallery rows: any fixed order then gives the same list, the kernel's
included.

(Cost, which no test asserts: tools/bench_topk_exact.py, profiles/topk_exact.txt — 1.99x / 2.00x / 2.41x / 2.69x
sim_topk at K = 1 / 10 / 50 / 128 on the correlated 4917 split, 2.13x on 4917 x 200 000 at K = 50.)"""
import numpy as np
import pytest
import torch

from test_rank_exact_cpu import GAP, NEAR_TIE_SHAPES, near_tie_fixture
from test_topk_exact_cpu import (NEAR_TIE_KS, SCATTERED_KS, SCATTERED_SHAPES, members_below_vk, scattered_copies_fixture,
                                 topk_exact_reference, topk_min_gap)

pytestmark = pytest.mark.gpu

_NEAR = {}


def _near(n, d):
  """The near-tie fixture of a shape, built once and never changed: (q, g, S)."""
  if (n, d) not in _NEAR:
    _NEAR[(n, d)] = near_tie_fixture(n, d, 7 * n + d)
  return _NEAR[(n, d)]


def _rand(dev, n, d, seed):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  return torch.randn(n, d, device=dev, generator=gen)


def _run(q, g, k, row0=0, nrows=None):
  from cmhse_amd import ops
  scores, index, resolved = ops.sim_topk_exact(q, g, k, row0, nrows)
  n = q.shape[0] - row0 if nrows is None else nrows
  assert scores.dtype == torch.float64 and scores.is_cuda and tuple(scores.shape) == (n, k)
  assert index.dtype == torch.int32 and index.is_cuda and tuple(index.shape) == (n, k)
  assert resolved.dtype == torch.int32 and resolved.is_cuda and tuple(resolved.shape) == (n,)
  return scores, index, resolved


def _float64_scores(q, g, k):
  """q64 @ g64.T of two device matrices, with the gap condition asserted."""
  gn = g.cpu().numpy()
  S = q.cpu().numpy().astype(np.float64) @ gn.astype(np.float64).T
  if S.shape[1] > 1:
    gap = topk_min_gap(S, k, gallery=gn)
    print('smallest non-zero gap among the first %d of a row: %.3g' % (k + 1, gap))
    assert gap > GAP
  return S


def _score_bound(q, g, index):
  """2 D 2^-53 |a_i| |b_j| at the returned columns: twice the error bound of either float64 summation."""
  na = np.linalg.norm(q.astype(np.float64), axis=1)[:, None]
  nb = np.linalg.norm(g.astype(np.float64), axis=1)[index]
  return 2.0 * q.shape[1] * 2.0 ** -53 * na * nb


def _check(out, q, g, S, k):
  """index == the reference exactly; scores within the float64 bound of S at those columns; K <= resolved <= M."""
  scores, index, resolved = (t.cpu().numpy() for t in out)
  want_scores, want = topk_exact_reference(S, k)
  np.testing.assert_array_equal(index, want)
  err = np.abs(scores - want_scores)
  bound = _score_bound(q, g, want)
  assert (err <= bound).all(), (float(err.max()), float(bound.min()))
  assert (np.diff(scores, axis=1) <= 0).all()                       # descending
  assert (resolved >= k).all() and (resolved <= g.shape[0]).all(), (resolved.min(), resolved.max())
  return scores, index, resolved


# ---------------------------------------------------------------------------------------------
# near ties: the fp32 list is wrong on most rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', NEAR_TIE_KS)
@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_ties_list_as_in_float64(dev, n, d, k):
  """Every K below 6 cuts the list inside the six copies, and on some rows (1 to 104 of them, counted on the CPU)
  between the query's own row i and its bit-identical duplicate 5 n + i: the smaller index is in, the larger
  out.  K = 6 holds all six, the duplicate right behind the original."""
  q, g, S = _near(n, d)
  out = _run(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), k)
  _, index, resolved = _check(out, q, g, S, k)
  rows = np.arange(n)
  if k < 6:
    cut = np.flatnonzero(index[:, -1] == rows)                      # the list ends on the original
    assert cut.size > 0 and not (index[cut] == (5 * n + cut)[:, None]).any()
  else:
    at = np.argmax(index == rows[:, None], axis=1)
    assert (index == rows[:, None]).any(axis=1).all() and (at < 5).all()
    assert (index[rows, at + 1] == 5 * n + rows).all()
  print('near-tie %d x %d, K = %d: resolved per row %d .. %d' % (n, d, k, resolved.min(), resolved.max()))


def test_fp32_lists_differ_on_the_near_ties(dev):
  """What the certified call is for: ops.sim_topk (the same rows, fp32 scores) lists some row of the
  near-tie fixtures differently from float64."""
  from cmhse_amd import ops
  differ = {}
  for n, d in NEAR_TIE_SHAPES:
    q, g, S = _near(n, d)
    _, want = topk_exact_reference(S, 5)
    _, index = ops.sim_topk(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), 5)
    differ[(n, d)] = int(np.count_nonzero((index.cpu().numpy() != want).any(axis=1)))
  print('rows where sim_topk differs from the float64 list at K = 5:', differ)
  assert max(differ.values()) > 0


_SCATTERED = {}


@pytest.mark.parametrize('k', SCATTERED_KS)
@pytest.mark.parametrize('n,d', SCATTERED_SHAPES)
def test_members_that_fp32_puts_below_its_kth_score(dev, n, d, k):
  """The check on the tolerance itself.  On the scattered-copies fixture the kernel's own fp32 scores put
  members of the float64 top-K strictly below v_K (asserted first, with ops.cosine_sim's bit-identical
  scores, and that ops.sim_topk's membership differs): only a second pass whose tolerance reaches them
  returns the float64 list."""
  from cmhse_amd import ops
  if (n, d) not in _SCATTERED:
    _SCATTERED[(n, d)] = scattered_copies_fixture(n, d, 5)
  q, g, S = _SCATTERED[(n, d)]
  dq, dg = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
  _, want = topk_exact_reference(S, k)
  below = members_below_vk(ops.cosine_sim(dq, dg).cpu().numpy(), want, k)
  index32 = ops.sim_topk(dq, dg, k)[1].cpu().numpy()
  members = np.count_nonzero([set(a) != set(b) for a, b in zip(index32.tolist(), want.tolist())])
  print('scattered %d x %d, K = %d: fp32 puts a member below v_K on %d rows, sim_topk membership differs on %d of %d'
        % (n, d, k, below.size, members, q.shape[0]))
  assert below.size > 0 and members > 0
  _check(_run(dq, dg, k), q, g, S, k)


# ---------------------------------------------------------------------------------------------
# random rows, not normalised
# ---------------------------------------------------------------------------------------------
def _exact_panels(nrows, M, K):
  """The host rule of topk.hip for the second pass: LDS of a workgroup = the 64 x 136 fp32 stage, 12 bytes per
  list and candidate entry (64 rows x K, 4 waves x 128), three words per tile row; as many panels as fill
  256 CUs' resident workgroups (160 KB of LDS each, 4 at most) once, never more than column tiles."""
  smem = 4 * 64 * 136 + 12 * (64 * K + 128 * 4) + 4 * 3 * 64
  per_cu = max(1, min(4, 160 * 1024 // smem))
  row_tiles, col_tiles = (nrows + 63) // 64, (M + 127) // 128
  return row_tiles, col_tiles, max(1, min(256 * per_cu // row_tiles, col_tiles))


# 130 x 12700, K = 128: three row tiles, 100 column tiles in 85 panels of one or two tiles each
PANEL_REMAINDER = (130, 12700, 32, 128)
RANDOM_SHAPES = [(1, 1, 8, 1), (129, 300, 64, 10), (257, 400, 30, 50), (70, 1500, 1024, 128),
                 (64, 5000, 1024, 50), (65, 100, 20, 100), PANEL_REMAINDER]


def test_panel_remainder_case_is_one():
  row_tiles, col_tiles, panels = _exact_panels(*[PANEL_REMAINDER[i] for i in (0, 1, 3)])
  assert row_tiles > 1 and panels < col_tiles and col_tiles % panels != 0, (row_tiles, col_tiles, panels)


@pytest.mark.parametrize('n,m,d,k', RANDOM_SHAPES)
def test_random_rows_not_normalised(dev, n, m, d, k):
  q, g = _rand(dev, n, d, 11 + n), _rand(dev, m, d, 12 + m)
  S = _float64_scores(q, g, k)
  _check(_run(q, g, k), q.cpu().numpy(), g.cpu().numpy(), S, k)


@pytest.mark.parametrize('n,m,d,k', [(257, 400, 30, 50), (130, 700, 64, 10)])
def test_results_do_not_depend_on_the_tolerance(dev, tune, n, m, d, k):
  q, g = _rand(dev, n, d, 21 + n), _rand(dev, m, d, 22 + m)
  S = _float64_scores(q, g, k)
  outs = {}
  for scale in (1, 16, 1 << 20):
    tune(rank_exact_tol_scale=scale)
    outs[scale] = _run(q, g, k)
  for scale in (16, 1 << 20):
    assert torch.equal(outs[scale][0].view(torch.int64), outs[1][0].view(torch.int64)), scale    # bit-equal
    assert torch.equal(outs[scale][1], outs[1][1]), scale
  assert bool((outs[16][2] >= outs[1][2]).all()) and bool((outs[1 << 20][2] >= outs[16][2]).all())
  # at 2^20 every column went through float64, and the list equals the reference
  assert bool((outs[1 << 20][2] == m).all())
  _check(outs[1 << 20], q.cpu().numpy(), g.cpu().numpy(), S, k)
  print('%d x %d x %d, K = %d: resolved in all %d / %d / %d at scale 1 / 16 / 2^20'
        % (n, m, d, k, int(outs[1][2].sum()), int(outs[16][2].sum()), int(outs[1 << 20][2].sum())))


# ---------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------
def test_collapsed_model(dev):
  """All embeddings equal: every score is one bit pattern and the column decides."""
  row = _rand(dev, 1, 64, 5)
  x = row.expand(200, 64).contiguous()
  scores, index, resolved = _run(x, x.clone(), 10)
  assert torch.equal(index, torch.arange(10, dtype=torch.int32, device=dev).expand(200, 10))
  assert len(torch.unique(scores.view(torch.int64))) == 1
  assert bool((resolved == 200).all())


def _boundary_fixture():
  """(queries [70, 256], gallery [400, 256], S float64) with g[350] = g[120] and g[10] = g[299]: query 0 puts
  columns 5 and 7 first and the pair 120 / 350 at places 3 and 4, query 1 the pair 10 / 299 there, query 2 the
  pair 120 / 350 in front, query 69 the pair 120 / 350 in front and 10 / 299 at places 3 and 4."""
  rng = np.random.RandomState(32)
  g = rng.standard_normal((400, 256)).astype(np.float32)
  q = rng.standard_normal((70, 256)).astype(np.float32)
  g[350] = g[120]
  g[10] = g[299]
  q[0] = g[120] + 1.5 * g[5] + 1.5 * g[7]
  q[1] = g[10] + 1.5 * g[5] + 1.5 * g[7]
  q[2] = g[120]
  q[69] = g[299] + 1.5 * g[350]
  S = q.astype(np.float64) @ g.astype(np.float64).T
  S[:, 350] = S[:, 120]                          # (bit-equal in the oracle too, whatever BLAS does)
  S[:, 299] = S[:, 10]
  return q, g, S


BOUNDARY_CASES = ((3, {0: (120, 350), 1: (10, 299), 69: (10, 299)}), (1, {2: (120, 350), 69: (120, 350)}))


def test_boundary_fixture_does_what_it_says():
  q, g, S = _boundary_fixture()
  for k, rows in BOUNDARY_CASES:
    assert topk_min_gap(S, k, gallery=g) > GAP
    _, want = topk_exact_reference(S, k + 1)
    for i, (inside, outside) in rows.items():
      assert want[i, k - 1] == inside and want[i, k] == outside and S[i, inside] == S[i, outside]


def test_ties_at_the_boundary(dev):
  """Bit-identical gallery rows at places K and K + 1: the smaller column is in, the larger is out."""
  q, g, S = _boundary_fixture()
  dq, dg = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
  for k, rows in BOUNDARY_CASES:
    _, index, _ = _check(_run(dq, dg, k), q, g, S, k)
    for i, (inside, outside) in rows.items():
      assert index[i, k - 1] == inside and outside not in index[i]


def test_stripes_concatenate(dev):
  q, g = _rand(dev, 300, 64, 31), _rand(dev, 400, 64, 32)
  g[350] = g[120]
  g[10] = g[299]
  whole = _run(q, g, 10)
  parts = [_run(q, g, 10, row0, nrows) for row0, nrows in ((0, 100), (100, 157), (257, 43))]
  assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int64), whole[0].view(torch.int64))
  for t in (1, 2):
    assert torch.equal(torch.cat([p[t] for p in parts]), whole[t]), t
  empty = _run(q, g, 10, 300, 0)
  assert all(t.numel() == 0 for t in empty)


def test_well_separated_input_resolves_one_column_per_row(dev):
  x = torch.nn.functional.normalize(_rand(dev, 300, 64, 6))
  S = _float64_scores(x, x, 1)
  off = S - np.eye(300)
  assert np.abs(off).max() < 0.9 and np.abs(np.diag(off)).max() < 1e-6   # diagonal 1, nothing near it
  scores, index, resolved = _run(x, x.clone(), 1)
  assert torch.equal(index[:, 0], torch.arange(300, dtype=torch.int32, device=dev))
  assert bool((resolved == 1).all())


def test_repeated_calls_are_identical(dev):
  q, g, S = _near(260, 1024)
  q, g = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
  first = [t.clone() for t in _run(q, g, 5)]
  for _ in range(4):
    again = _run(q, g, 5)
    assert torch.equal(again[0].view(torch.int64), first[0].view(torch.int64))
    assert torch.equal(again[1], first[1]) and torch.equal(again[2], first[2])
  np.testing.assert_array_equal(first[1].cpu().numpy(), topk_exact_reference(S, 5)[1])


# ---------------------------------------------------------------------------------------------
# the Python layers
# ---------------------------------------------------------------------------------------------
def _duplicated_caption_fixture():
  rng = np.random.RandomState(3)
  caps = rng.standard_normal((150, 64))
  imgs = caps + 0.8 * rng.standard_normal((150, 64))
  caps = (caps / np.linalg.norm(caps, axis=1, keepdims=True)).astype(np.float32)
  imgs = (imgs / np.linalg.norm(imgs, axis=1, keepdims=True)).astype(np.float32)
  caps[7] = caps[2]                      # a duplicate caption: image 2's best two captions tie exactly
  S = imgs.astype(np.float64) @ caps.astype(np.float64).T
  S[:, 7] = S[:, 2]                      # (bit-equal in the oracle too, whatever BLAS does)
  return imgs, caps, S


def test_retrieve_exact(dev):
  from cmhse_amd import evaluation, ops
  from cmhse_amd.evaluation import CACHE_STATS, retrieve
  imgs, caps, S = _duplicated_caption_fixture()
  assert topk_min_gap(S, 5, gallery=caps) > GAP
  want_scores, want = topk_exact_reference(S, 5)
  assert 2 in want[2] and 7 in want[2]
  stats, last = dict(CACHE_STATS), evaluation._LAST_ENCODE[0]
  scores, index = retrieve(imgs, caps, 5, exact=True)              # NumPy in, NumPy out
  assert isinstance(scores, np.ndarray) and scores.dtype == np.float64 and scores.shape == (150, 5)
  assert isinstance(index, np.ndarray) and index.dtype == np.int64
  np.testing.assert_array_equal(index, want)
  assert (np.abs(scores - want_scores) <= _score_bound(imgs, caps, want)).all()
  v, p = torch.from_numpy(imgs).to(dev), torch.from_numpy(caps).to(dev)
  dscores, dindex = retrieve(v, p, 5, exact=True)                  # device in, device out
  assert dscores.is_cuda and dscores.dtype == torch.float64 and dindex.is_cuda and dindex.dtype == torch.int32
  np.testing.assert_array_equal(dindex.cpu().numpy(), want)
  np.testing.assert_array_equal(dscores.cpu().numpy(), scores)
  # the default is the fp32 call, bit for bit
  s32, i32 = retrieve(v, p, 5)
  t32, j32 = ops.sim_topk(v, p, 5)
  assert s32.dtype == torch.float32 and torch.equal(s32, t32) and torch.equal(i32, j32)
  n32, m32 = retrieve(imgs, caps, 5, exact=False)
  assert n32.dtype == np.float32 and m32.dtype == np.int64
  np.testing.assert_array_equal(n32, t32.cpu().numpy())
  np.testing.assert_array_equal(m32, j32.cpu().numpy())
  assert CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


def test_i2t_t2i_exact_top1(dev):
  from cmhse_amd import ops
  from cmhse_amd.evaluation import i2t_t2i_exact
  imgs, caps, S = _duplicated_caption_fixture()
  assert topk_min_gap(S, 1, gallery=caps) > GAP and topk_min_gap(S.T, 1, gallery=imgs) > GAP
  want_i, want_t = topk_exact_reference(S, 1)[1][:, 0], topk_exact_reference(S.T, 1)[1][:, 0]
  assert want_i[2] == 2 and S[2, 7] == S[2, 2]                     # the tie is image 2's arg-max: the smaller index
  base = i2t_t2i_exact(imgs, caps)
  (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), info = i2t_t2i_exact(imgs, caps, top1='exact')
  assert top1_i.dtype == np.float64 and top1_t.dtype == np.float64
  np.testing.assert_array_equal(top1_i, want_i)
  np.testing.assert_array_equal(top1_t, want_t)
  np.testing.assert_array_equal(ranks_i, base[0][2])               # the ranks are unchanged
  np.testing.assert_array_equal(ranks_t, base[1][2])
  assert rep_i == base[0][0] and rep_t == base[1][0]
  assert info['resolved'] == base[2]['resolved'] and 'top1_resolved' not in base[2]
  v, p = torch.from_numpy(imgs).to(dev), torch.from_numpy(caps).to(dev)
  res = int(ops.sim_topk_exact(v, p, 1)[2].sum()) + int(ops.sim_topk_exact(p, v, 1)[2].sum())
  assert info['top1_resolved'] == res >= 150 + 150 + 1             # one column a row, and the duplicate
  # GPU tensors in: top1 stays an int32 device tensor
  (_, dtop1_i, dranks_i), (_, dtop1_t, _), dinfo = i2t_t2i_exact(v, p, ties='pessimistic', top1='exact')
  assert dtop1_i.is_cuda and dtop1_i.dtype == torch.int32 and tuple(dtop1_i.shape) == (150,)
  np.testing.assert_array_equal(dtop1_i.cpu().numpy(), want_i)
  np.testing.assert_array_equal(dtop1_t.cpu().numpy(), want_t)
  assert dinfo['top1_resolved'] == res
  # top1='fp32' is the call as it was
  direct_i, direct_t = ops.sim_rank_exact(v, p), ops.sim_rank_exact(p, v)
  (rep_i, top1_i, ranks_i), (rep_t, top1_t, ranks_t), finfo = i2t_t2i_exact(v, p, ties='pessimistic', top1='fp32')
  assert torch.equal(ranks_i, direct_i[1]) and torch.equal(top1_i, direct_i[2])
  assert torch.equal(ranks_t, direct_t[1]) and torch.equal(top1_t, direct_t[2])
  assert torch.equal(dranks_i, direct_i[1])
  assert sorted(finfo) == ['i2t', 'resolved', 't2i']
  np.testing.assert_array_equal(base[0][1], direct_i[2].cpu().numpy())


# ---------------------------------------------------------------------------------------------
# the validation shape
# ---------------------------------------------------------------------------------------------
def test_full_size_correlated_split(dev):
  """The correlated 4917 split, both directions, K = 50, every row against float64; about one column in a
  hundred beyond K goes through float64 (NumPy fp32: 1.01 K per row), and a pass that sends far more has a
  wrong threshold."""
  from cmhse_amd import synthetic
  K = 50
  a, b = synthetic.correlated_embeddings(4917)
  S = a.astype(np.float64) @ b.astype(np.float64).T
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  for name, qq, gg, qn, gn, SS in (('a -> b', q, g, a, b, S), ('b -> a', g, q, b, a, S.T)):
    gap = topk_min_gap(SS, K, gallery=gn)
    assert gap > GAP
    _, _, resolved = _check(_run(qq, gg, K), qn, gn, SS, K)
    print('correlated 4917 %s, K = %d: smallest gap %.3g, resolved %d columns (%.4f K per row, max %d)'
          % (name, K, gap, int(resolved.sum()), resolved.mean() / K, resolved.max()))
    assert resolved.sum() <= 1.1 * K * 4917
