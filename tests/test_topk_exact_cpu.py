"""Certified top-K retrieval without a GPU: a NumPy statement of cmhse_sim_topk_exact's contract, the
validity of the near-tie fixtures (test_rank_exact_cpu.py) as top-K cases, the candidate rule of the
second pass restated in NumPy, and the C ABI's workspace size and argument validation
(include/cmhse_hip.h).  The GPU tests (test_gpu_topk_exact.py) import the contract from here."""
import ctypes

import numpy as np
import pytest

from test_rank_exact_cpu import GAP, NEAR_TIE_SHAPES, near_tie_fixture

NEAR_TIE_KS = (1, 2, 3, 5, 6)     # (not 8 or more: other queries' copies enter the list and the gap falls
                                  # to 1.5e-12 at 260 x 1024, below GAP)
TOPK_MAX = 128


def _ordered_head(S, k):
  """The first k columns of every row of S by (score descending, column ascending): a lexsort by
  (-score, column) of the columns at or above the row's k-th largest score (every tie of it included), which
  is the head of the lexsort of the whole row."""
  n, M = S.shape
  kth = np.partition(S, M - k, axis=1)[:, M - k]
  head = np.empty((n, k), dtype=np.int64)
  for i in range(n):
    c = np.flatnonzero(S[i] >= kth[i])
    head[i] = c[np.lexsort((c, -S[i, c]))[:k]]          # last key first: -score, then column
  return head


def topk_exact_reference(S64, k):
  """cmhse_sim_topk_exact's contract from a float64 score matrix S64 [n, M]: (scores [n, k], index [n, k]),
  the first k columns of every row by (score descending, column ascending)."""
  S = np.asarray(S64, dtype=np.float64)
  index = _ordered_head(S, k)
  return np.take_along_axis(S, index, axis=1), index


def topk_min_gap(S64, k, gallery=None):
  """The smallest NON-ZERO gap between consecutive entries among the first k + 1 of each row's descending
  sort (inf if there is none).  With `gallery`, every ZERO gap among them is asserted to come from
  bit-identical gallery rows: a float64 matrix out of BLAS is a valid reference for the order only if
  the returned gap exceeds GAP and this holds."""
  S = np.asarray(S64, dtype=np.float64)
  order = _ordered_head(S, min(k + 1, S.shape[1]))
  top = np.take_along_axis(S, order, axis=1)
  gaps = top[:, :-1] - top[:, 1:]
  if gallery is not None:
    r, c = np.nonzero(gaps == 0)
    assert np.array_equal(gallery[order[r, c]], gallery[order[r, c + 1]])
  nz = gaps[gaps > 0]
  return float(nz.min()) if nz.size else float('inf')


SCATTERED_SHAPES = [(200, 256), (150, 300)]
SCATTERED_KS = (1, 3, 5)


def scattered_copies_fixture(n, d, seed, copies=8):
  """(queries fp32 [m, d], gallery fp32 [8 m, d], S float64 [m, 8 m]), m <= n: unit-norm queries and eight
  copies of each whose EVERY coordinate is moved by -1, 0 or +1 ulp.  The float64 scores of a query's copies
  differ by about 1e-9; their fp32 scores are scattered over a few fp32 steps by the summation's own rounding
  (they do not tie, unlike near_tie_fixture's), so fp32 puts true members of the float64 top-K strictly BELOW
  its own K-th score: a second pass whose tolerance is too small misses them.  Queries whose copies come
  closer than 1e-10 in float64 are dropped (chosen on the CPU, from float64 alone), so the order of the first
  K + 1 is beyond what a float64 summation order can move.  Copy c of query i is gallery row c m + i."""
  rng = np.random.RandomState(seed)
  q = rng.standard_normal((n, d))
  q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
  cs = []
  for _ in range(copies):
    x = q.copy()
    bits = x.view(np.int32)
    bits += rng.randint(-1, 2, size=bits.shape).astype(np.int32)
    cs.append(x)
  C = np.stack(cs, 1)                                                # [n, copies, d]
  s = -np.sort(-np.einsum('nd,ncd->nc', q.astype(np.float64), C.astype(np.float64)), axis=1)
  keep = (s[:, :-1] - s[:, 1:]).min(axis=1) > 1e-10
  q, C = q[keep], C[keep]
  g = np.ascontiguousarray(C.transpose(1, 0, 2).reshape(-1, d))
  return q, g, q.astype(np.float64) @ g.astype(np.float64).T


def members_below_vk(S32, want, k):
  """Rows on which fp32 scores put a member of the float64 top-K (want [n, k]) strictly below the k-th
  largest fp32 score of the row."""
  vk = -np.sort(-S32, axis=1)[:, k - 1]
  return np.flatnonzero((np.take_along_axis(S32, want, axis=1) < vk[:, None]).any(axis=1))


def candidates_fp32(S32, k, tol):
  """The candidate rule of the second pass on an fp32 score matrix: NOT (fl(v_K - v) > tol_i), with v_K the
  k-th largest fp32 score of the row and tol_i (float64 [n]) rounded up to fp32."""
  S32 = np.asarray(S32, dtype=np.float32)
  vk = -np.sort(-S32, axis=1)[:, k - 1]
  t32 = tol.astype(np.float32)
  t32 = np.where(t32.astype(np.float64) < tol, np.nextafter(t32, np.float32(np.inf)), t32)
  return ~((vk[:, None] - S32) > t32[:, None])


def tolerances(lib, q, g):
  nb = float(np.linalg.norm(g.astype(np.float64), axis=1).max())
  return np.array([lib.cmhse_sim_rank_exact_tolerance(q.shape[1], float(na), nb)
                   for na in np.linalg.norm(q.astype(np.float64), axis=1)])


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------
def test_reference_orders_by_score_then_column():
  S = np.array([[2.0, 3.0, 2.0, 1.0, 2.0],
                [0.0, -0.0, 0.0, 0.0, 0.0],
                [5.0, 4.0, 3.0, 9.0, 3.0]])
  scores, index = topk_exact_reference(S, 3)
  assert index.tolist() == [[1, 0, 2], [0, 1, 2], [3, 0, 1]]        # (-0.0 == 0.0: a tie)
  assert scores.tolist() == [[3.0, 2.0, 2.0], [0.0, 0.0, 0.0], [9.0, 5.0, 4.0]]
  assert topk_exact_reference(S, 5)[1].tolist() == [[1, 0, 2, 4, 3], [0, 1, 2, 3, 4], [3, 0, 1, 2, 4]]
  assert topk_min_gap(S, 1) == 1.0 and topk_min_gap(S[:1], 3) == 1.0 and topk_min_gap(S[1:2], 4) == float('inf')
  R = np.random.RandomState(0).standard_normal((30, 50))
  assert np.array_equal(topk_exact_reference(R, 7)[1], np.argsort(-R, axis=1)[:, :7])
  T = np.round(R)                                        # many ties: the head of the whole row's lexsort
  col = np.arange(50)
  for k in (1, 7, 50):
    assert topk_exact_reference(T, k)[1].tolist() == [np.lexsort((col, -T[i]))[:k].tolist() for i in range(30)]


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_tie_fixture_is_a_valid_topk_case(n, d):
  """The float64 order of the first k + 1 entries is beyond what a float64 summation order can move, and the
  NumPy fp32 list differs from it on some row for every K."""
  q, g, S = near_tie_fixture(n, d, 7 * n + d)
  S32 = q @ g.T
  for k in NEAR_TIE_KS:
    gap = topk_min_gap(S, k, gallery=g)
    _, want = topk_exact_reference(S, k)
    _, got32 = topk_exact_reference(S32.astype(np.float64), k)
    order = np.count_nonzero((got32 != want).any(axis=1))
    members = np.count_nonzero([set(a) != set(b) for a, b in zip(got32.tolist(), want.tolist())])
    print('near-tie %d x %d, K = %d: gap %.3g, fp32 order differs on %d rows, membership on %d of %d'
          % (n, d, k, gap, order, members, n))
    assert gap > GAP
    assert order > 0


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_candidate_rule_in_numpy(lib, n, d):
  """v_K from fp32 scores and the certified tolerance: the candidates hold the float64 top-K, and the exact
  top-K of the candidates is the float64 top-K."""
  q, g, S = near_tie_fixture(n, d, 7 * n + d)
  S32 = q @ g.T
  tol = tolerances(lib, q, g)
  for k in NEAR_TIE_KS:
    want_scores, want = topk_exact_reference(S, k)
    cand = candidates_fp32(S32, k, tol)
    assert np.take_along_axis(cand, want, axis=1).all()
    got_scores, got = topk_exact_reference(np.where(cand, S, -np.inf), k)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_scores, want_scores)
    per_row = cand.sum(axis=1)
    print('near-tie %d x %d, K = %d: %d .. %d candidates per row' % (n, d, k, per_row.min(), per_row.max()))
    assert (per_row >= k).all() and per_row.max() <= 6 * n


@pytest.mark.parametrize('n,d', SCATTERED_SHAPES)
def test_scattered_copies_fixture_needs_the_tolerance(lib, n, d):
  """NumPy fp32 puts members of the float64 top-K below v_K (by one to four fp32 steps of a unit score), so
  the candidates of a zero tolerance miss them; the certified tolerance holds them, and a thousandth of it
  (below one fp32 step at these widths) does not."""
  q, g, S = scattered_copies_fixture(n, d, 5)
  assert q.shape[0] >= n // 2 and g.shape == (8 * q.shape[0], d)
  S32 = q @ g.T
  tol = tolerances(lib, q, g)
  assert (tol * 1e-3 < 2.0 ** -24).all()
  for k in SCATTERED_KS:
    assert topk_min_gap(S, k, gallery=g) > GAP
    _, want = topk_exact_reference(S, k)
    below = members_below_vk(S32, want, k)
    print('scattered %d x %d, K = %d: fp32 puts a member below v_K on %d of %d rows' % (n, d, k, below.size, q.shape[0]))
    assert below.size > 0
    for scale, holds in ((1.0, True), (1e-3, False), (0.0, False)):
      cand = candidates_fp32(S32, k, tol * scale)
      assert bool(np.take_along_axis(cand, want, axis=1).all()) == holds, (k, scale)


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_workspace(lib):
  """0 for bad arguments, 256-aligned, the fp32 pass's region and more, and independent of M once the panel
  count is capped.  Monotone in nrows and in K wherever the column tiles pin the panel count (M = 300: three
  panels up to 85 row tiles; nrows = 64, M = 4917: 39 panels for every K): past that the count is
  256 * (workgroups per CU) // row_tiles, by the rule of cmhse_sim_topk_workspace, and its product with nrows
  carries that floor (13 panels x 4917 rows, 6 x 9802 at K = 1) as cmhse_sim_topk_workspace's does."""
  ws = lib.cmhse_sim_topk_exact_workspace
  for bad in ((0, 10, 1), (-1, 10, 1), (4, 0, 1), (4, -3, 1), (4, 10, 0), (4, 10, -1), (4, 10, TOPK_MAX + 1)):
    assert ws(*bad) == 0, bad
  for K in (1, 10, 50, TOPK_MAX):
    prev = 0
    for nrows in (1, 2, 63, 64, 65, 128, 129, 1000, 4917):
      b = ws(nrows, 300, K)
      assert b > 0 and b % 256 == 0 and b >= prev, (nrows, K)
      assert b > lib.cmhse_sim_topk_workspace(nrows, 300, K)        # the fp32 pass's region and more
      assert b >= 3 * nrows * K * 12 + nrows * K * 8 + nrows * 16   # three panels of pairs, the fp32 lists, norm / tol
      prev = b
  for nrows, M in ((1, 128), (64, 4917), (4917, 300)):
    sizes = [ws(nrows, M, K) for K in (1, 2, 10, 16, 17, 50, 52, 53, 100, TOPK_MAX)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], (nrows, M, sizes)
  for nrows, M, K in ((9802, 4917, 1), (4917, 4917, 50), (70, 1500, 128), (256, 200000, 10)):
    assert ws(nrows, M, K) > 0 and ws(nrows, M, K) % 256 == 0
  # the panel count is fixed by nrows and K (LDS occupancy), not by M
  assert ws(4917, 4917, 50) == ws(4917, 10 ** 6, 50)
  assert ws(256, 200000, 10) == ws(256, 2000000, 10)
  assert ws(4917, 4917, 50) < 4917 * 4917 * 4                       # far below the fp32 score matrix


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_sim_topk_exact is returned before anything touches the device: cmhse_sim_topk's
  cases, codes and order."""
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_sim_topk_exact_workspace(4, 10, 3)
  good = dict(A=fake, B=fake, N=8, M=10, D=8, row0=2, nrows=4, K=3, scores=fake, index=fake, res=fake,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=0, stream=None)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_sim_topk_exact(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'], a['K'],
                                    a['scores'], a['index'], a['res'], a['ws'], a['ws_bytes'], a['stream'])

  def call32(**kw):                    # the fp32 call with the same arguments
    a = dict(good, **kw)
    return lib.cmhse_sim_topk(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'], a['K'],
                              a['scores'], a['index'], a['ws'], a['ws_bytes'], a['stream'])

  assert call() == -2                  # valid arguments, no workspace: stopped by the workspace check
  for bad in [dict(A=None), dict(B=None), dict(scores=None), dict(index=None), dict(ws=None),
              dict(N=0), dict(M=0), dict(D=0), dict(N=-8), dict(M=-1), dict(D=-1),
              dict(K=0), dict(K=-1), dict(K=11), dict(K=TOPK_MAX + 1), dict(M=1000, K=TOPK_MAX + 1),
              dict(row0=-1), dict(nrows=-1), dict(row0=5), dict(nrows=7), dict(N=5)]:
    assert call(**bad) == -1, bad
    assert call(ws_bytes=ws_ok, **bad) == -1, bad
    assert call32(**bad) == -1, bad                                  # the same cases as cmhse_sim_topk
  assert call(res=None) == -1 and call(res=None, ws_bytes=ws_ok) == -1
  assert call(ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=ws_ok) == -2      # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == -2                                        # too small
  assert call(K=10, ws_bytes=0) == -2                                          # K == M is fine
  assert call(N=4, M=3, row0=0, K=3, ws_bytes=0) == -2                         # N > M: no diagonal convention
  # D past the bound's range: after the argument and workspace checks, before any launch
  assert call(D=1 << 24, ws_bytes=0) == -2
  assert call(D=1 << 24, ws_bytes=ws_ok) == -4
  # an empty stripe is a no-op that succeeds (nothing launched), whatever the output pointers
  assert call(nrows=0) == 0
  assert call(row0=8, nrows=0, scores=None, index=None, res=None, ws=None) == 0
  assert call(row0=9, nrows=0) == -1
  assert call(nrows=0, K=11) == -1                                             # arguments are checked first


def test_python_layers_validate():
  import torch
  from cmhse_amd import evaluation, ops
  from cmhse_amd.dropin import evaluation as dropin
  with pytest.raises(RuntimeError):
    ops.sim_topk_exact(torch.zeros(2, 4), torch.zeros(3, 4), 1)
  assert dropin.retrieve is evaluation.retrieve and dropin.i2t_t2i_exact is evaluation.i2t_t2i_exact
  with pytest.raises(ValueError):
    evaluation.retrieve(np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32), 1, exact='yes')
  with pytest.raises(ValueError):
    evaluation.retrieve(np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32), 1, exact=None)
  with pytest.raises(ValueError):
    evaluation.i2t_t2i_exact(np.zeros((2, 4)), np.zeros((2, 4)), top1='neither')
  with pytest.raises(ValueError):
    evaluation.i2t_t2i_exact(np.zeros((2, 4)), np.zeros((2, 4)), ties='neither', top1='exact')
