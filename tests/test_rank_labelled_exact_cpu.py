"""Certified labelled ranking without a GPU: a NumPy statement of cmhse_sim_rank_labelled_exact's contract,
the fixtures that the GPU tests (test_gpu_rank_labelled_exact.py) import, with their validity asserted here,
and the C ABI's workspace size and argument validation (include/cmhse_hip.h)."""
import ctypes

import numpy as np
import pytest

from test_rank_exact_cpu import GAP, NEAR_TIE_SHAPES, near_tie_fixture


def labelled_exact_reference(S64, lists):
  """The contract from a float64 score matrix S64 [n, M] and one strictly ascending list of positives per
  row: (rank_lo, rank_hi, best_pos, thr) with thr[i] = S[i, P_i].max(), rank_lo[i] = #{j : S[i,j] > thr[i]},
  rank_hi[i] = rank_lo[i] + #{j not in P_i : S[i,j] == thr[i]}, best_pos[i] the first of the list at thr[i]."""
  S = np.asarray(S64, dtype=np.float64)
  n = S.shape[0]
  lo, hi, best = (np.empty(n, dtype=np.int64) for _ in range(3))
  thr = np.empty(n, dtype=np.float64)
  for i in range(n):
    P = np.asarray(lists[i], dtype=np.int64)
    assert P.size > 0 and (np.diff(P) > 0).all()
    thr[i] = S[i, P].max()
    lo[i] = np.count_nonzero(S[i] > thr[i])
    negative = np.ones(S.shape[1], dtype=bool)
    negative[P] = False
    hi[i] = lo[i] + np.count_nonzero((S[i] == thr[i]) & negative)
    best[i] = P[S[i, P] == thr[i]][0]
  return lo, hi, best, thr


def labelled_min_gap(S64, gallery, lists):
  """The smallest |S[i, j] - thr[i]| over the columns j whose gallery row is NOT bit-identical to the row of
  query i's best positive (those tie it exactly, in any summation order)."""
  S = np.asarray(S64, dtype=np.float64)
  g = np.ascontiguousarray(gallery)
  _, group = np.unique(g.view(np.dtype((np.void, g.dtype.itemsize * g.shape[1]))).ravel(), return_inverse=True)
  group = group.ravel()
  _, _, best, thr = labelled_exact_reference(S, lists)
  gap = np.abs(S - thr[:, None])
  gap[group[None, :] == group[best][:, None]] = np.inf
  return float(gap.min())


def csr_of(lists):
  off = np.zeros(len(lists) + 1, dtype=np.int64)
  np.cumsum([len(x) for x in lists], out=off[1:])
  return off, np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])


# ---------------------------------------------------------------------------------------------
# fixtures shared with the GPU tests: built once, never changed
# ---------------------------------------------------------------------------------------------
_CACHE = {}


def near_tie_labels(n):
  """The lists over the 6 n gallery rows [q, 1-ulp, 2-ulp, 8-ulp, 64-ulp copies, q] of near_tie_fixture."""
  lists = []
  for i in range(n):
    if i % 4 == 0:
      lists.append([n + i, 3 * n + i])                  # the best positive is decided below fp32 resolution
    elif i % 4 == 1:
      lists.append([i, 5 * n + i])                      # two bit-identical positives, no tied negative
    elif i % 4 == 2:
      lists.append([i])                                 # the duplicate 5 n + i is a tied negative
    else:
      lists.append(sorted({2 * n + i, 4 * n + i, (i + 1) % n}))
  return lists


def near_tie_case(n, d):
  """(q, g, S, lists, (rank_lo, rank_hi, best_pos, thr)) of a near-tie shape."""
  key = ('near', n, d)
  if key not in _CACHE:
    q, g, S = near_tie_fixture(n, d, 7 * n + d)
    lists = near_tie_labels(n)
    _CACHE[key] = (q, g, S, lists, labelled_exact_reference(S, lists))
  return _CACHE[key]


RANDOM_SHAPES = [(1, 1, 8), (129, 300, 64), (257, 400, 30), (515, 515, 1024), (300, 130, 64), (64, 5000, 1024)]


def random_case(n, m, d):
  """(q, g, S, lists, reference): unnormalised fp32 rows, 1 to 5 distinct sorted positives per query; query 0
  owns up to 260 evenly spread columns, a list that crosses a 128-pair boundary."""
  key = ('random', n, m, d)
  if key not in _CACHE:
    rng = np.random.RandomState(1000 * n + m + d)
    q = rng.standard_normal((n, d)).astype(np.float32)
    g = rng.standard_normal((m, d)).astype(np.float32)
    lists = [np.sort(rng.choice(m, size=rng.randint(1, min(5, m) + 1), replace=False)) for _ in range(n)]
    lists[0] = np.arange(0, m, max(1, m // 260))[:260]
    S = q.astype(np.float64) @ g.astype(np.float64).T
    _CACHE[key] = (q, g, S, lists, labelled_exact_reference(S, lists))
  return _CACHE[key]


VAL_N = 4917


def validation_case():
  """The two-annotation-set shape with bit-identical positives: synthetic.correlated_embeddings(4917) against
  the gallery [b; b[perm]] (M = 9834), positives {i, 4917 + inv_perm[i]}.  (q, g, S, lists, reference)."""
  if 'val' not in _CACHE:
    from cmhse_amd import synthetic
    a, b = synthetic.correlated_embeddings(VAL_N)
    perm = np.random.RandomState(4917).permutation(VAL_N)
    inv = np.empty(VAL_N, dtype=np.int64)
    inv[perm] = np.arange(VAL_N)
    g = np.ascontiguousarray(np.concatenate([b, b[perm]]))
    # (from the distinct rows, then gathered: the duplicate columns are bit-equal whatever BLAS does)
    S = (a.astype(np.float64) @ b.astype(np.float64).T)[:, np.concatenate([np.arange(VAL_N), perm])]
    lists = [[i, VAL_N + int(inv[i])] for i in range(VAL_N)]
    _CACHE['val'] = (a, g, S, lists, labelled_exact_reference(S, lists))
  return _CACHE['val']


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract and the fixtures
# ---------------------------------------------------------------------------------------------
def test_reference_on_a_hand_made_matrix():
  S = np.array([[2.0, 3.0, 2.0, 1.0, 2.0],        # P = {0}: column 1 above, columns 2 and 4 tied negatives
                [1.0, 5.0, 0.0, 5.0, 5.0],        # P = {1, 3}: a tied second positive and one tied negative
                [5.0, 4.0, 3.0, 9.0, 1.0]])       # P = {1, 4}: tie-free
  lo, hi, best, thr = labelled_exact_reference(S, [[0], [1, 3], [1, 4]])
  assert lo.tolist() == [1, 0, 2] and hi.tolist() == [3, 1, 2]
  assert best.tolist() == [0, 1, 1] and thr.tolist() == [2.0, 5.0, 4.0]
  # every column of a row a positive: nothing can tie against it
  lo, hi, best, _ = labelled_exact_reference(np.zeros((2, 4)), [[0, 1, 2, 3], [2]])
  assert lo.tolist() == [0, 0] and hi.tolist() == [0, 3] and best.tolist() == [0, 2]
  # identity labels: the diagonal contract of cmhse_sim_rank_exact
  from test_rank_exact_cpu import exact_reference
  R = np.random.RandomState(0).standard_normal((30, 50)).round(1)          # (rounded: exact ties exist)
  lo, hi, best, _ = labelled_exact_reference(R, [[i] for i in range(30)])
  want = exact_reference(R)
  assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]) and best.tolist() == list(range(30))
  assert (hi > lo).any()
  with pytest.raises(AssertionError):
    labelled_exact_reference(S, [[0], [3, 1], [1]])                        # lists are strictly ascending


def test_min_gap_skips_bit_identical_rows_only():
  g = np.array([[1, 0], [0, 1], [1, 0], [0.5, 0.5]], dtype=np.float32)
  S = np.array([[1.0, 0.0, 1.0, 0.5]])
  assert labelled_min_gap(S, g, [[0]]) == 0.5                               # column 2 = row 0 again: skipped
  assert labelled_min_gap(S, g, [[3]]) == 0.5
  assert labelled_min_gap(np.array([[1.0, 0.0, 1.0, 1.0]]), g, [[0]]) == 0.0   # column 3 ties, another row


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_tie_fixture_with_labels(n, d):
  q, g, S, lists, (lo, hi, best, thr) = near_tie_case(n, d)
  assert g.shape == (6 * n, d) and len(lists) == n
  for i, P in enumerate(lists):
    assert list(P) == sorted(set(P)) and len(P) == (2, 2, 1, 3)[i % 4]
  gap = labelled_min_gap(S, g, lists)
  assert gap > GAP
  assert int((hi - lo).sum()) == len(range(2, n, 4))                       # the rows with i % 4 == 2, once each
  assert all(hi[i] == lo[i] + 1 for i in range(2, n, 4))
  # what makes the fixture discriminate: fp32 scores rank these rows differently, and choose another positive
  S32 = (q @ g.T).astype(np.float64)
  lo32, _, best32, _ = labelled_exact_reference(S32, lists)
  differ, other = np.count_nonzero(lo32 != lo), np.count_nonzero(best32 != best)
  print('near-tie %d x %d with labels: min gap %.3g, NumPy-fp32 ranks differ on %d rows, best positive on %d of %d'
        % (n, d, gap, differ, other, n))
  assert differ > 0 and other > 0


@pytest.mark.parametrize('n,m,d', RANDOM_SHAPES)
def test_random_case_is_valid(n, m, d):
  q, g, S, lists, (lo, hi, best, thr) = random_case(n, m, d)
  assert q.dtype == np.float32 and g.dtype == np.float32 and S.shape == (n, m)
  for P in lists:
    assert 1 <= len(P) and (np.diff(P) > 0).all() and P[0] >= 0 and P[-1] < m
  assert all(len(P) <= 5 for P in lists[1:])
  assert len(lists[0]) == min(m, 260)                                      # m >= 260: crosses a 128-pair boundary
  gap = labelled_min_gap(S, g, lists)
  print('random %d x %d x %d: min gap %.3g' % (n, m, d, gap))
  if m > 1:
    assert gap > GAP
  assert np.array_equal(lo, hi)


def test_validation_shape_is_valid(lib):
  """The gap of the full-size case, and the condition behind the GPU test's cap on `resolved`: the columns
  the counting pass CAN send through float64 are those with |v - thr32| <= tol_i, and |v - thr32| differs
  from |s64 - thr64| by at most 2 E_i <= tol_i, so they lie among the columns with |s64 - thr64| <= 2 tol_i."""
  q, g, S, lists, (lo, hi, best, thr) = validation_case()
  gap = labelled_min_gap(S, g, lists)
  assert gap > GAP
  assert np.array_equal(lo, hi)                                            # bit-identical positives: no tie counts
  assert np.array_equal(best, np.arange(VAL_N))                            # the smaller of the two copies
  nb = float(np.linalg.norm(g.astype(np.float64), axis=1).max())
  na = np.linalg.norm(q.astype(np.float64), axis=1)
  tol = np.array([lib.cmhse_sim_rank_exact_tolerance(q.shape[1], float(x), nb * (1 + 2.0 ** -23)) for x in na])
  tol = tol * (1 + 2.0 ** -23)                                             # (rounded up to fp32 in the kernel)
  within = int(np.count_nonzero(np.abs(S - thr[:, None]) <= 2.0 * tol[:, None]))
  print('validation shape: min gap %.3g, %d of %d columns within 2 tol of their threshold'
        % (gap, within, S.size))
  assert within < 0.01 * S.size


# ---------------------------------------------------------------------------------------------
# the host side of ops.sim_rank_labelled_exact and the evaluation entry points
# ---------------------------------------------------------------------------------------------
def test_labels_are_sorted_and_deduplicated_on_the_host():
  from cmhse_amd.ops import positives_csr, sorted_unique_csr
  off, idx = sorted_unique_csr(*positives_csr([[5, 1, 5, 3], [2], [0, 0, 0], [9, 8, 7, 8]], 4, 10))
  assert off.dtype == np.int32 and idx.dtype == np.int32
  assert off.tolist() == [0, 3, 4, 5, 8] and idx.tolist() == [1, 3, 5, 2, 0, 7, 8, 9]
  # already normal: unchanged; a stripe of the labels; one target per query
  o2, i2 = sorted_unique_csr(off, idx)
  assert o2.tolist() == off.tolist() and i2.tolist() == idx.tolist()
  o3, i3 = sorted_unique_csr(*positives_csr([[5, 1, 5, 3], [2], [0, 0, 0], [9, 8, 7, 8]], 4, 10, 1, 2))
  assert o3.tolist() == [0, 1, 2] and i3.tolist() == [2, 0]
  o4, i4 = sorted_unique_csr(*positives_csr([3, 1, 2], 3, 4))
  assert o4.tolist() == [0, 1, 2, 3] and i4.tolist() == [3, 1, 2]
  o5, i5 = sorted_unique_csr(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
  assert o5.tolist() == [0] and i5.size == 0
  # random lists with duplicates against a per-list statement
  rng = np.random.RandomState(1)
  lists = [rng.randint(0, 12, size=rng.randint(1, 9)) for _ in range(50)]
  o6, i6 = sorted_unique_csr(*positives_csr(lists, 50, 12))
  for k, P in enumerate(lists):
    assert i6[o6[k]:o6[k + 1]].tolist() == sorted(set(P.tolist()))


def test_python_argument_errors_before_any_upload():
  import torch
  from cmhse_amd import evaluation, ops
  from cmhse_amd.dropin import evaluation as dropin
  assert dropin.rank_labelled_exact is evaluation.rank_labelled_exact
  assert dropin.i2t_t2i_labelled_exact is evaluation.i2t_t2i_labelled_exact
  x = np.zeros((2, 4), dtype=np.float32)
  pairs = np.array([[0, 0], [1, 1]])
  for bad in (dict(ties='neither'), dict(ties='Optimistic'), dict(ties=None), dict(top1='fp64'),
              dict(top1='Exact'), dict(top1=True)):
    with pytest.raises(ValueError, match="must be '"):
      evaluation.rank_labelled_exact(x, x, [0, 1], **bad)
    with pytest.raises(ValueError, match="must be '"):
      evaluation.i2t_t2i_labelled_exact(x, x, pairs, **bad)
  # the labels are checked on the host, before the matrices go anywhere
  with pytest.raises(ValueError, match='outside the gallery'):
    evaluation.rank_labelled_exact(x, x, [0, 2])
  with pytest.raises(ValueError, match='no positive'):
    evaluation.rank_labelled_exact(x, x, [[0], []])
  with pytest.raises(ValueError, match='appears in no pair'):
    evaluation.i2t_t2i_labelled_exact(x, x, pairs[:1])
  with pytest.raises(RuntimeError):
    ops.sim_rank_labelled_exact(torch.zeros(2, 4), torch.zeros(3, 4), [[1, 0, 1], [2]])


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_workspace_values(lib):
  ws = lib.cmhse_sim_rank_labelled_exact_workspace
  for nrows, pairs in [(0, 0), (0, 5), (-1, 0), (-3, 10)]:
    assert ws(nrows, pairs) == 0
  assert ws(10, 9) == 0 and ws(10, -1) == 0                        # fewer pairs than queries: no valid labels
  prev = 0
  for nrows in (1, 2, 63, 64, 65, 128, 129, 1000, 4917, 9802, 100000):
    b = ws(nrows, nrows)
    assert b > 0 and b % 256 == 0 and b >= prev
    assert b >= lib.cmhse_sim_rank_exact_workspace(nrows)
    # it grows with the pairs: a float64 score each
    big = ws(nrows, nrows + 100000)
    assert big % 256 == 0 and big >= b + 8 * 100000 and big <= b + 8 * 100000 + 256
    assert ws(nrows, 0x7fffffff) % 256 == 0 and ws(nrows, 0x7fffffff) >= 8 * 0x7fffffff
    prev = b
  assert ws(4917, 9834) < 4917 * 64 + 9834 * 8                     # a few vectors: far from the N x M matrix


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_sim_rank_labelled_exact is returned before anything touches the device."""
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  off = np.array([0, 2, 3, 4, 6], dtype=np.int32)
  idx = np.array([1, 9, 0, 5, 3, 5], dtype=np.int32)
  ws_ok = lib.cmhse_sim_rank_labelled_exact_workspace(4, 6)
  good = dict(A=fake, B=fake, N=4, M=10, D=8, row0=0, nrows=4, off_h=off, idx_h=idx, off_d=fake,
              idx_d=fake, n_pairs=6, lo=fake, hi=fake, top1=fake, best_pos=fake, best_score=fake, res=fake,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok, stream=None)

  def ptr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_sim_rank_labelled_exact(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'],
                                             ptr(a['off_h']), ptr(a['idx_h']), a['off_d'], a['idx_d'],
                                             a['n_pairs'], a['lo'], a['hi'], a['top1'], a['best_pos'],
                                             a['best_score'], a['res'], a['ws'], a['ws_bytes'], a['stream'])

  def i32(*v):
    return np.array(v, dtype=np.int32)

  unsupported = dict(D=1 << 24)        # the LAST check: a call that is otherwise valid returns -4 ...
  assert call(**unsupported) == -4
  for bad in [dict(A=None), dict(B=None), dict(N=0), dict(M=0), dict(D=0), dict(N=-4), dict(D=-1),
              dict(row0=-1), dict(nrows=-1), dict(row0=1), dict(N=3),
              dict(off_h=None), dict(idx_h=None), dict(off_d=None), dict(idx_d=None),
              dict(n_pairs=5), dict(n_pairs=7), dict(n_pairs=3), dict(n_pairs=-1),
              dict(off_h=i32(1, 2, 3, 4, 6)),                       # does not start at 0
              dict(off_h=i32(0, 2, 2, 4, 6)),                       # an empty list
              dict(off_h=i32(0, 3, 2, 4, 6)),                       # decreasing
              dict(off_h=i32(0, 2, 3, 4, 5)),                       # != n_pairs
              dict(idx_h=i32(1, 9, 0, 5, 3, 10)),                   # index == M
              dict(idx_h=i32(-1, 9, 0, 5, 3, 5)),
              dict(M=9),                                            # index 9 outside a gallery of 9
              dict(idx_h=i32(1, 1, 0, 5, 3, 5)),                    # a duplicated index
              dict(idx_h=i32(1, 9, 0, 5, 5, 5)),
              dict(idx_h=i32(9, 1, 0, 5, 3, 5)),                    # a descending list
              dict(idx_h=i32(1, 9, 0, 5, 5, 3)),
              dict(lo=None), dict(hi=None), dict(top1=None), dict(best_pos=None), dict(res=None),
              dict(ws=None)]:
    assert call(**bad) == -1, bad
    # ... and every argument error comes before the workspace check and before that one
    assert call(ws_bytes=0, **bad) == -1, bad
    if 'D' not in bad:
      assert call(**dict(unsupported, **bad)) == -1, bad
  assert call(best_score=None, ws_bytes=0) == -2                   # best_score may be NULL
  # ascending across the boundary of two lists is not required: only inside a list
  assert call(idx_h=i32(8, 9, 0, 5, 3, 4), ws_bytes=0) == -2
  assert call(ws=ctypes.c_void_p((1 << 20) + 16)) == -2            # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == -2                            # too small
  assert call(ws_bytes=0) == -2
  assert call(ws_bytes=0, **unsupported) == -2                     # the workspace before the width
  # an empty stripe is a no-op that succeeds (nothing launched, no labels or buffers needed)
  empty = dict(off_h=None, idx_h=None, off_d=None, idx_d=None, n_pairs=0, lo=None, hi=None, top1=None,
               best_pos=None, best_score=None, res=None, ws=None, ws_bytes=0)
  assert call(nrows=0, **empty) == 0
  assert call(row0=4, nrows=0, **empty) == 0
  assert call(row0=5, nrows=0, **empty) == -1
  assert call(nrows=0, **dict(empty, n_pairs=2)) == -1
  # M < N is fine for the argument checks (the diagonal call refuses it): only the workspace is missing
  assert call(N=40, M=10, ws_bytes=0) == -2
