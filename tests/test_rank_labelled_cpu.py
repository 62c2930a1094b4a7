"""Labelled ranking without a GPU: the label helpers (ops.positives_csr, evaluation.pairs_from_ids /
csr_from_pairs), the C ABI's workspace size and argument validation (include/cmhse_hip.h), and a
NumPy statement of the contract that the GPU tests (test_gpu_rank_labelled.py) import."""
import ctypes

import numpy as np
import pytest


def labelled_reference(S, off, idx):
  """cmhse_sim_rank_labelled's contract from a stored score matrix S [n, M] and CSR labels:
  (rank, top1, best_pos, best_score) with thr[i] = max S[i, P_i], rank[i] = #{j : S[i, j] > thr[i]},
  best_pos[i] the smallest p in P_i with S[i, p] == thr[i], top1[i] the first arg-max of row i."""
  S = np.asarray(S)
  n = S.shape[0]
  rank = np.empty(n, dtype=np.int64)
  best_pos = np.empty(n, dtype=np.int64)
  best_score = np.empty(n, dtype=S.dtype)
  for i in range(n):
    pos = np.asarray(idx[off[i]:off[i + 1]], dtype=np.int64)
    thr = S[i, pos].max()
    rank[i] = np.count_nonzero(S[i] > thr)
    best_pos[i] = pos[S[i, pos] == thr].min()
    best_score[i] = thr
  return rank, S.argmax(axis=1), best_pos, best_score


def random_labels(rng, n, m, lo, hi):
  """CSR labels: between lo and hi random positives (duplicates possible) for each of n queries."""
  counts = rng.randint(lo, hi + 1, size=n)
  off = np.zeros(n + 1, dtype=np.int64)
  np.cumsum(counts, out=off[1:])
  return off, rng.randint(0, m, size=int(off[-1]))


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------
def test_reference_equals_argsort_form():
  """On tie-free rows the rank is the position of the best-placed positive in the descending sort."""
  rng = np.random.RandomState(0)
  S = rng.standard_normal((40, 300))
  off, idx = random_labels(rng, 40, 300, 1, 5)
  rank, top1, best_pos, best_score = labelled_reference(S, off, idx)
  order = np.argsort(-S, axis=1)
  for i in range(40):
    where = {int(c): k for k, c in enumerate(order[i])}
    places = [where[int(p)] for p in idx[off[i]:off[i + 1]]]
    assert rank[i] == min(places)
    assert where[int(best_pos[i])] == rank[i]
    assert best_score[i] == S[i, best_pos[i]]
    assert top1[i] == order[i, 0]


def test_reference_tie_rule():
  S = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                [0.0, 0.0, 0.0, 0.0, 0.0]])
  off, idx = np.array([0, 3, 5]), np.array([4, 3, 2, 3, 1])
  rank, top1, best_pos, _ = labelled_reference(S, off, idx)
  # row 0: positives 4, 3, 2; the best score 3.0 is shared by 2 and 4 -> the smaller; column 1 ties
  # the threshold and is not counted
  assert rank.tolist() == [0, 0] and best_pos.tolist() == [2, 1] and top1.tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------
# ops.positives_csr
# ---------------------------------------------------------------------------------------------
def test_positives_three_forms_agree():
  import torch
  from cmhse_amd.ops import positives_csr
  targets = [4, 0, 2]
  want_off, want_idx = [0, 1, 2, 3], [4, 0, 2]
  for form in (targets, np.array(targets), np.array(targets, dtype=np.int32), torch.tensor(targets),
               (np.array([0, 1, 2, 3]), np.array(targets)), ([0, 1, 2, 3], targets), [[4], [0], [2]],
               [np.array([4]), torch.tensor([0]), (2,)]):
    off, idx = positives_csr(form, 3, 5)
    assert off.dtype == np.int32 and idx.dtype == np.int32
    assert off.tolist() == want_off and idx.tolist() == want_idx
  off, idx = positives_csr([[1, 1, 0], [3], [2, 4]], 3, 5)          # duplicates are allowed
  assert off.tolist() == [0, 3, 4, 6] and idx.tolist() == [1, 1, 0, 3, 2, 4]
  same = positives_csr((np.array([0, 3, 4, 6]), np.array([1, 1, 0, 3, 2, 4])), 3, 5)
  assert same[0].tolist() == off.tolist() and same[1].tolist() == idx.tolist()


def test_positives_two_queries_are_not_ambiguous():
  from cmhse_amd.ops import positives_csr
  # a LIST of two sequences: per-query lists; a TUPLE of two arrays: CSR
  off, idx = positives_csr([[0, 1, 2], [1, 2]], 2, 3)
  assert off.tolist() == [0, 3, 5] and idx.tolist() == [0, 1, 2, 1, 2]
  off, idx = positives_csr(([0, 1, 2], [1, 2]), 2, 3)
  assert off.tolist() == [0, 1, 2] and idx.tolist() == [1, 2]
  off, idx = positives_csr([2, 0], 2, 3)                           # a list of scalars: targets
  assert off.tolist() == [0, 1, 2] and idx.tolist() == [2, 0]


@pytest.mark.parametrize('positives,needle', [
    ([1, 2], 'query matrix has 3 rows'),                             # wrong length, targets
    ([[1], [2]], 'query matrix has 3 rows'),                         # wrong length, lists
    (([0, 1, 2], [1, 2]), 'need 4'),                                 # wrong length, CSR
    (([0, 1, 2, 2], [1, 2, 3]), '0 to len(indices)'),                # last offset != pairs
    (([1, 1, 2, 3], [1, 2, 3]), '0 to len(indices)'),                # first offset != 0
    (([0, 2, 1, 3], [1, 2, 3]), 'decrease at query row 1'),
    (([0, 1, 1, 3], [1, 2, 3]), 'query row 1 has no positive'),
    ([[1], [], [2]], 'query row 1 has no positive'),
    ([1, 5, 2], 'query row 1: positive 5'),                          # index == M
    ([[1], [2, 0], [4, -1]], 'query row 2: positive -1'),
    (([0, 1, 2, 4], [1, 2, 3, 7]), 'query row 2: positive 7'),
    ([1.0, 2.0, 3.0], 'integers'),
    ([[1], [2.5], [3]], 'query row 1'),
    (np.array([True, False, True]), 'integers'),
    ([[1], 2, [3]], 'query row 1'),                                  # a scalar among the lists
    (np.zeros((3, 1), dtype=np.int64), '1-D'),
    (([0, 1, 2, 3], [1, 2, 3], [4]), '(offsets, indices)'),
])
def test_positives_errors(positives, needle):
  from cmhse_amd.ops import positives_csr
  with pytest.raises(ValueError) as e:
    positives_csr(positives, 3, 5)
  assert needle in str(e.value), str(e.value)


def test_positives_stripes_slice_the_csr():
  from cmhse_amd.ops import positives_csr
  rng = np.random.RandomState(1)
  off, idx = random_labels(rng, 37, 50, 1, 4)
  full = positives_csr((off, idx), 37, 50)
  assert full[0].tolist() == off.tolist() and full[1].tolist() == idx.tolist()
  for row0, nrows in [(0, 37), (0, 10), (10, 20), (30, 7), (36, 1), (5, 0), (37, 0)]:
    o, x = positives_csr((off, idx), 37, 50, row0, nrows)
    assert o.size == nrows + 1 and o[0] == 0 and o[-1] == x.size
    for q in range(nrows):
      assert x[o[q]:o[q + 1]].tolist() == idx[off[row0 + q]:off[row0 + q + 1]].tolist()
  o, x = positives_csr((off, idx), 37, 50, 12)                     # nrows defaults to the rest
  assert o.size == 26 and x.tolist() == idx[off[12]:].tolist()
  for row0, nrows in [(-1, 2), (30, 8), (38, 0), (0, -1)]:
    with pytest.raises(ValueError):
      positives_csr((off, idx), 37, 50, row0, nrows)
  # the whole label set is checked, whatever the stripe
  with pytest.raises(ValueError):
    positives_csr([0, 1, 99], 3, 5, 0, 1)


def test_sim_rank_labelled_needs_device_tensors():
  import torch
  from cmhse_amd import ops
  with pytest.raises(RuntimeError):
    ops.sim_rank_labelled(torch.zeros(2, 4), torch.zeros(3, 4), [0, 1])


# ---------------------------------------------------------------------------------------------
# evaluation.pairs_from_ids / csr_from_pairs
# ---------------------------------------------------------------------------------------------
def test_pairs_from_ids():
  from cmhse_amd.evaluation import pairs_from_ids
  images = ['v_a', 'v_b', 'v_c']
  captions = ['v_a', 'v_b', 'v_c', 'v_c', 'v_x', 'v_a']            # v_a, v_c twice; v_x matches no image
  pairs = pairs_from_ids(images, captions)
  assert pairs.dtype == np.int64 and pairs.shape == (5, 2)
  assert pairs.tolist() == [[0, 0], [0, 5], [1, 1], [2, 2], [2, 3]]
  assert pairs_from_ids(images, images).tolist() == [[0, 0], [1, 1], [2, 2]]
  assert pairs_from_ids(('a', 'b'), ['c']).shape == (0, 2)
  assert pairs_from_ids((7, 8), np.array([8, 7, 8])).tolist() == [[0, 1], [1, 0], [1, 2]]


def test_csr_from_pairs_both_directions():
  from cmhse_amd.evaluation import csr_from_pairs, pairs_from_ids
  from cmhse_amd.ops import positives_csr
  pairs = pairs_from_ids(['a', 'b', 'c'], ['a', 'b', 'c', 'c', 'a'])
  (off_i, idx_i), (off_t, idx_t) = csr_from_pairs(pairs, 3, 5)
  assert off_i.tolist() == [0, 2, 3, 5] and idx_i.tolist() == [0, 4, 1, 2, 3]
  assert off_t.tolist() == [0, 1, 2, 3, 4, 5] and idx_t.tolist() == [0, 1, 2, 2, 0]
  positives_csr((off_i, idx_i), 3, 5)
  positives_csr((off_t, idx_t), 5, 3)
  # any order of the pairs, any integer container
  shuffled = pairs[[3, 0, 4, 2, 1]].astype(np.int32)
  (o2, x2), (o3, x3) = csr_from_pairs(shuffled.tolist(), 3, 5)
  assert o2.tolist() == off_i.tolist() and x2.tolist() == idx_i.tolist()
  assert o3.tolist() == off_t.tolist() and x3.tolist() == idx_t.tolist()


def test_csr_from_pairs_errors():
  from cmhse_amd.evaluation import csr_from_pairs, pairs_from_ids
  pairs = pairs_from_ids(['a', 'b', 'c'], ['a', 'b', 'c', 'x'])    # caption 3 has no image
  with pytest.raises(ValueError, match='caption row 3 appears in no pair'):
    csr_from_pairs(pairs, 3, 4)
  with pytest.raises(ValueError, match='image row 1 appears in no pair'):
    csr_from_pairs([[0, 0], [2, 1]], 3, 2)
  with pytest.raises(ValueError, match='image row 3 outside'):
    csr_from_pairs([[0, 0], [3, 1]], 3, 2)
  with pytest.raises(ValueError, match='caption row -1 outside'):
    csr_from_pairs([[0, 0], [1, -1]], 2, 2)
  with pytest.raises(ValueError, match='integer'):
    csr_from_pairs([[0.0, 0.0]], 1, 1)
  with pytest.raises(ValueError, match=r'\[P, 2\]'):
    csr_from_pairs([0, 1, 2], 3, 3)
  with pytest.raises(ValueError, match='appears in no pair'):
    csr_from_pairs(np.zeros((0, 2), dtype=np.int64), 1, 1)


def test_dropin_reexports():
  from cmhse_amd.dropin import evaluation as dropin
  from cmhse_amd import evaluation
  for name in ('rank_labelled', 'i2t_t2i_labelled', 'pairs_from_ids', 'csr_from_pairs'):
    assert getattr(dropin, name) is getattr(evaluation, name)


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_workspace_values(lib):
  ws = lib.cmhse_sim_rank_labelled_workspace
  for nrows, pairs in [(0, 0), (0, 5), (-1, 0), (-3, 10)]:
    assert ws(nrows, pairs) == 0
  assert ws(10, 9) == 0 and ws(10, -1) == 0                        # fewer pairs than queries: no valid labels
  assert ws(1, 1) == 512                                           # one threshold | two keys
  assert ws(4917, 4917) >= 4917 * (4 + 8 + 8)
  prev = 0
  for nrows in (1, 2, 63, 64, 65, 128, 129, 1000, 4917, 9802, 100000):
    b = ws(nrows, nrows)
    assert b > 0 and b % 256 == 0 and b >= prev
    # more pairs never need less
    assert ws(nrows, nrows) <= ws(nrows, 2 * nrows) <= ws(nrows, 0x7fffffff)
    prev = b
  # a few vectors of nrows entries, however many pairs: far from the N x M matrix
  assert ws(4917, 98340) < 4917 * 64


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_sim_rank_labelled is returned before anything touches the device."""
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  off = np.array([0, 2, 3, 4, 6], dtype=np.int32)
  idx = np.array([1, 9, 0, 5, 5, 3], dtype=np.int32)
  ws_ok = lib.cmhse_sim_rank_labelled_workspace(4, 6)
  good = dict(A=fake, B=fake, N=4, M=10, D=8, row0=0, nrows=4, off_h=off, idx_h=idx, off_d=fake,
              idx_d=fake, n_pairs=6, rank=fake, top1=fake, best_pos=fake, best_score=fake,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok, stream=None)

  def ptr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_sim_rank_labelled(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'],
                                       ptr(a['off_h']), ptr(a['idx_h']), a['off_d'], a['idx_d'],
                                       a['n_pairs'], a['rank'], a['top1'], a['best_pos'],
                                       a['best_score'], a['ws'], a['ws_bytes'], a['stream'])

  def i32(*v):
    return np.array(v, dtype=np.int32)

  for bad in [dict(A=None), dict(B=None), dict(off_h=None), dict(idx_h=None), dict(off_d=None),
              dict(idx_d=None), dict(rank=None), dict(top1=None), dict(best_pos=None), dict(ws=None),
              dict(N=0), dict(M=0), dict(D=0), dict(N=-4), dict(D=-1), dict(row0=-1), dict(nrows=-1),
              dict(row0=1), dict(N=3), dict(n_pairs=5), dict(n_pairs=7), dict(n_pairs=3), dict(n_pairs=-1),
              dict(off_h=i32(1, 2, 3, 4, 6)),                       # does not start at 0
              dict(off_h=i32(0, 2, 2, 4, 6)),                       # an empty list
              dict(off_h=i32(0, 3, 2, 4, 6)),                       # decreasing
              dict(off_h=i32(0, 2, 3, 4, 5)),                       # != n_pairs
              dict(idx_h=i32(1, 9, 0, 5, 5, 10)),                   # index == M
              dict(idx_h=i32(1, -1, 0, 5, 5, 3)),
              dict(M=9)]:                                           # index 9 outside a gallery of 9
    assert call(**bad) == -1, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16)) == -2            # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == -2                            # too small
  assert call(ws_bytes=0) == -2
  # bad labels are reported before the workspace is looked at
  assert call(ws_bytes=0, idx_h=i32(1, 9, 0, 5, 5, 10)) == -1
  # an empty stripe is a no-op that succeeds (nothing launched, no labels or buffers needed)
  empty = dict(off_h=None, idx_h=None, off_d=None, idx_d=None, n_pairs=0, rank=None, top1=None,
               best_pos=None, best_score=None, ws=None, ws_bytes=0)
  assert call(nrows=0, **empty) == 0
  assert call(row0=4, nrows=0, **empty) == 0
  assert call(nrows=0, **dict(empty, n_pairs=2)) == -1
  # M < N is fine for the argument checks (cmhse_sim_rank refuses it): only the workspace is missing
  assert call(N=40, M=10, ws_bytes=0) == -2
