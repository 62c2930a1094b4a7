"""Certified ranking without a GPU: a NumPy statement of cmhse_sim_rank_exact's contract and the near-tie
fixture that the GPU tests (test_gpu_rank_exact.py) import, the tolerance function against the textbook
bound, and the C ABI's workspace size, argument validation and tunable (include/cmhse_hip.h)."""
import ctypes

import numpy as np
import pytest

GAP = 1e-11      # far above D * 2^-53 * |a| |b| at every shape used here: any fixed float64 summation
                 # order compares such a pair of scores the same way


def exact_reference(S64, row0=0):
  """cmhse_sim_rank_exact's contract from a float64 score matrix S64 [n, M] whose row r belongs to the
  query row0 + r (its diagonal column): (rank_lo, rank_hi) = the columns j != row0 + r strictly above /
  at or above the diagonal score."""
  S = np.asarray(S64, dtype=np.float64)
  n = S.shape[0]
  diag = S[np.arange(n), row0 + np.arange(n)][:, None]
  other = np.ones(S.shape, dtype=bool)
  other[np.arange(n), row0 + np.arange(n)] = False
  return (np.count_nonzero((S > diag) & other, axis=1).astype(np.int64),
          np.count_nonzero((S >= diag) & other, axis=1).astype(np.int64))


def min_gap(S64, row0=0, skip=None):
  """The smallest |S[r, j] - S[r, row0 + r]| over the columns j != row0 + r (and not skip[r])."""
  S = np.asarray(S64, dtype=np.float64)
  n = S.shape[0]
  gap = np.abs(S - S[np.arange(n), row0 + np.arange(n)][:, None])
  gap[np.arange(n), row0 + np.arange(n)] = np.inf
  if skip is not None:
    gap[np.arange(n), skip] = np.inf
  return float(gap.min())


def near_tie_fixture(n, d, seed):
  """(queries fp32 [n, d], gallery fp32 [6 n, d], S float64 [n, 6 n]): unit-norm queries q; the gallery
  is q, four near-copies of q (copy c moves the magnitude of each row's largest coordinate by
  +-{1, 2, 8, 64}[c] ulps, sign random) and q again: every positive has one bit-identical duplicate and
  four neighbours below fp32 resolution.  S is taken from the distinct rows and then gathered, so the
  duplicate columns are bit-equal in it whatever BLAS does.  Asserts its validity: every gap between a
  diagonal score and a non-duplicate column exceeds GAP."""
  rng = np.random.RandomState(seed)
  q = rng.standard_normal((n, d))
  q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
  big = np.abs(q).argmax(axis=1)
  base = [q]
  for ulps in (1, 2, 8, 64):
    c = q.copy()
    bits = c.view(np.int32)              # (sign-magnitude: adding to the integer moves the magnitude)
    bits[np.arange(n), big] += ulps * rng.choice([-1, 1], size=n).astype(np.int32)
    base.append(c)
  base = np.concatenate(base)
  col = np.concatenate([np.arange(5 * n), np.arange(n)])
  S = (q.astype(np.float64) @ base.astype(np.float64).T)[:, col]
  assert min_gap(S, skip=5 * n + np.arange(n)) > GAP
  assert np.array_equal(S[:, :n], S[:, 5 * n:])
  return q, np.ascontiguousarray(base[col]), S


NEAR_TIE_SHAPES = [(130, 64), (130, 50), (260, 1024), (200, 300)]


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract and the fixture
# ---------------------------------------------------------------------------------------------
def test_reference_counts_strict_and_non_strict():
  S = np.array([[2.0, 3.0, 2.0, 1.0, 2.0],
                [0.0, 0.0, 0.0, 0.0, 0.0],
                [5.0, 4.0, 3.0, 9.0, 3.0]])
  lo, hi = exact_reference(S)
  assert lo.tolist() == [1, 0, 3] and hi.tolist() == [3, 4, 4]
  lo, hi = exact_reference(S[1:], row0=1)                 # rows 1, 2 of the same matrix as a stripe
  assert lo.tolist() == [0, 3] and hi.tolist() == [4, 4]
  # tie-free rows: both are the position of the diagonal in the descending sort
  R = np.random.RandomState(0).standard_normal((30, 50))
  lo, hi = exact_reference(R)
  order = np.argsort(-R, axis=1)
  assert np.array_equal(lo, hi)
  assert lo.tolist() == [int(np.flatnonzero(order[i] == i)[0]) for i in range(30)]


@pytest.mark.parametrize('n,d', NEAR_TIE_SHAPES)
def test_near_tie_fixture(n, d):
  q, g, S = near_tie_fixture(n, d, 7 * n + d)
  assert q.dtype == np.float32 and g.dtype == np.float32 and g.shape == (6 * n, d) and S.shape == (n, 6 * n)
  assert np.array_equal(g[:n], q) and np.array_equal(g[5 * n:], q)
  for c in range(4):
    assert (np.count_nonzero(g[(c + 1) * n:(c + 2) * n] != q, axis=1) == 1).all()
  lo, hi = exact_reference(S)
  assert np.array_equal(hi - lo, np.ones(n, dtype=np.int64))      # the duplicate, and nothing else
  # what makes the fixture discriminate: fp32 scores rank these rows differently
  S32 = q @ g.T
  lo32, _ = exact_reference(S32.astype(np.float64))
  differ = np.count_nonzero(lo32 != lo)
  print('near-tie %d x %d: min gap %.3g, NumPy-fp32 ranks differ on %d of %d rows'
        % (n, d, min_gap(S, skip=5 * n + np.arange(n)), differ, n))
  assert differ > 0


# ---------------------------------------------------------------------------------------------
# the tolerance
# ---------------------------------------------------------------------------------------------
DS = (1, 8, 30, 1024, 4096)
NORMS = (1e-3, 1.0, 32.0)


def test_tolerance_against_the_textbook_value(lib):
  tol = lib.cmhse_sim_rank_exact_tolerance
  for D in DS:
    for na in NORMS:
      for nb in NORMS:
        textbook = 2.0 * D * 2.0 ** -24 * na * nb
        t = tol(D, na, nb)
        assert t >= textbook, (D, na, nb, t, textbook)
        assert t <= 1.1 * textbook, (D, na, nb, t, textbook)     # no vacuous "everything is undecided"


def test_tolerance_is_monotone(lib):
  tol = lib.cmhse_sim_rank_exact_tolerance
  for na in NORMS:
    for nb in NORMS:
      vals = [tol(D, na, nb) for D in DS]
      assert all(a < b for a, b in zip(vals, vals[1:]))
  for D in DS:
    for fixed in NORMS:
      a = [tol(D, x, fixed) for x in NORMS]
      b = [tol(D, fixed, x) for x in NORMS]
      assert all(x < y for x, y in zip(a, a[1:])) and all(x < y for x, y in zip(b, b[1:]))
  assert tol(64, 0.0, 1.0) > 0.0 and tol(64, 0.0, 1.0) < 1e-40     # the underflow term alone
  assert np.isnan(tol(0, 1.0, 1.0)) and np.isnan(tol(8, -1.0, 1.0)) and np.isnan(tol(8, 1.0, -1.0))
  assert np.isinf(tol(1 << 24, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_workspace_is_a_function_of_nrows(lib):
  ws = lib.cmhse_sim_rank_exact_workspace
  for nrows in (0, -1, -4917):
    assert ws(nrows) == 0
  prev = 0
  for nrows in (1, 2, 63, 64, 65, 128, 129, 1000, 4917, 9802, 100000):
    b = ws(nrows)
    assert b > 0 and b % 256 == 0 and b >= prev
    assert b >= lib.cmhse_sim_rank_workspace(nrows)       # cmhse_sim_rank's regions and more
    prev = b
  assert ws(4917) < 4917 * 64                              # a few vectors of nrows entries


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_sim_rank_exact is returned before anything touches the device."""
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_sim_rank_exact_workspace(4)
  good = dict(A=fake, B=fake, N=8, M=10, D=8, row0=2, nrows=4, lo=fake, hi=fake, top1=fake, res=fake,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=0, stream=None)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_sim_rank_exact(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'],
                                    a['lo'], a['hi'], a['top1'], a['res'], a['ws'], a['ws_bytes'],
                                    a['stream'])

  # (the valid arguments with no workspace: past every argument check, stopped by the workspace check)
  assert call() == -2
  for bad in [dict(A=None), dict(B=None), dict(lo=None), dict(hi=None), dict(top1=None), dict(res=None),
              dict(ws=None), dict(N=0), dict(M=0), dict(D=0), dict(N=-8), dict(D=-1), dict(row0=-1),
              dict(nrows=-1),
              dict(row0=5), dict(nrows=7), dict(N=5),             # stripe outside the matrix
              dict(N=20, row0=7),                                 # row0 + nrows > M
              dict(N=20, M=5)]:
    assert call(**bad) == -1, bad
    assert call(ws_bytes=ws_ok, **bad) == -1, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=ws_ok) == -2      # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == -2                                        # too small
  assert call(N=20, row0=6, ws_bytes=0) == -2                                  # row0 + nrows == M is fine
  # an empty stripe is a no-op that succeeds (nothing launched)
  assert call(nrows=0) == 0
  assert call(row0=8, nrows=0) == 0
  assert call(row0=9, nrows=0) == -1


def test_tunable_range_and_round_trip(lib):
  from cmhse_amd import ops
  name = b'rank_exact_tol_scale'
  old = ctypes.c_int32(-7)
  assert lib.cmhse_tune(name, -1, ctypes.byref(old)) == 0 and old.value == 1        # the default
  for bad in (0, (1 << 20) + 1, 0x7fffffff):
    assert lib.cmhse_tune(name, bad, None) == -1
  assert lib.cmhse_tune(name, -1, ctypes.byref(old)) == 0 and old.value == 1        # refused: unchanged
  try:
    assert ops.tune('rank_exact_tol_scale', 16) == 1
    assert ops.tune('rank_exact_tol_scale') == 16
    assert ops.tune('rank_exact_tol_scale', 1 << 20) == 16
    ctx = ops.TuneContext()                               # a context starts from the process defaults
    assert ctx.tune('rank_exact_tol_scale') == 1 << 20
    assert ctx.tune('rank_exact_tol_scale', 3) == 1 << 20
    assert lib.cmhse_ctx_tune(ctx.handle, name, 0, None) == -1
    assert lib.cmhse_ctx_tune(ctx.handle, name, (1 << 20) + 1, None) == -1
    assert ctx.tune('rank_exact_tol_scale') == 3
    assert ops.tune('rank_exact_tol_scale') == 1 << 20    # ... and does not write them
    with ctx:
      assert ops.tune('rank_exact_tol_scale') == 3
  finally:
    assert lib.cmhse_tune(name, 1, None) == 0
  with ops.tuned(rank_exact_tol_scale=16):
    assert ops.tune('rank_exact_tol_scale') == 16
  assert ops.tune('rank_exact_tol_scale') == 1


def test_needs_device_tensors_and_dropin_reexport():
  import torch
  from cmhse_amd import evaluation, ops
  from cmhse_amd.dropin import evaluation as dropin
  with pytest.raises(RuntimeError):
    ops.sim_rank_exact(torch.zeros(2, 4), torch.zeros(3, 4))
  assert dropin.i2t_t2i_exact is evaluation.i2t_t2i_exact
  with pytest.raises(ValueError):
    evaluation.i2t_t2i_exact(np.zeros((2, 4)), np.zeros((2, 4)), ties='neither')
