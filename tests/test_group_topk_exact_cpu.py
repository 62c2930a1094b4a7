"""Certified group-wise top-K without a GPU: a NumPy statement of cmhse_group_topk_exact's contract, the validity
of the group near-tie fixtures for list comparisons (which queries a GPU test may compare index by index, and that
the fixtures discriminate), and the C ABI's plan, workspace size and argument validation (include/cmhse_hip.h).
test_gpu_group_topk_exact.py imports the helpers."""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

from test_group_rank_exact_cpu import (GROUP_GAP, GROUP_NEAR_TIE_SHAPES, REDUCES, _offsets, block_scores, float64_noise,
                                       group_near_tie_fixture, near_tie_seed)

ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
P2V, V2P = 0, 1
DIRECTIONS = ['p2v', 'v2p']
HDR = 8                       # Bv, Bp, Nc, Ns, direction, K, R, C
# the most query-side omissions a (shape, reduce, direction, K) case may have: 5 % of its queries
MAX_LEFT_OUT = 0.05


def query_view(G, direction):
  """[Bq, Bg] from the [videos, paragraphs] matrix: a paragraph's row holds its videos under 'p2v'."""
  return np.asarray(G).T if direction == 'p2v' else np.asarray(G)


def group_topk_exact_reference(Q, k):
  """cmhse_group_topk_exact's contract from the float64 block scores Q [Bq, Bg] of every (query, gallery group):
  (scores float64 [Bq, k], index int64 [Bq, k]), score descending, then gallery index ascending; -0.0 and +0.0
  tie (x + 0.0 has no negative zero)."""
  Q = np.asarray(Q, dtype=np.float64) + 0.0
  idx = np.broadcast_to(np.arange(Q.shape[1]), Q.shape)
  order = np.lexsort((idx, -Q), axis=-1)[:, :k]
  return np.take_along_axis(Q, order, axis=1), order


def planted_pairs(n):
  """The planted duplicates of group_near_tie_fixture(n, ...): groups i and 5 n + i, i < n (families 0 and 5 of one
  base group), as comparable_queries' (stride, count)."""
  return (5 * n, n)


def comparable_queries(Q, k, planted=None, orig=None, gap=GROUP_GAP):
  """bool [Bq]: the queries whose first k reference indices any correct float64 implementation returns.  Among the
  first k + 1 sorted scores of the query (k when the gallery has no more) every gap between consecutive entries is
  either above `gap` or exactly zero between PLANTED duplicates: planted = (stride, count) names the gallery groups
  whose original indices orig[.] are i and i + stride with i < count — bit-equal rows, so bit-equal scores in any
  implementation.  Everything else — a gap in (0, gap], a zero gap between other groups — leaves the query out."""
  Q = np.asarray(Q, dtype=np.float64)
  s, ix = group_topk_exact_reference(Q, min(k + 1, Q.shape[1]))
  g = -np.diff(s, axis=1)
  ok = g > gap
  if planted is not None:
    stride, count = planted
    o = ix if orig is None else np.asarray(orig)[ix]
    a, b = np.minimum(o[:, :-1], o[:, 1:]), np.maximum(o[:, :-1], o[:, 1:])
    ok |= (g == 0) & (b - a == stride) & (a < count)
  return ok.all(axis=1)


@functools.lru_cache(maxsize=None)
def near_tie_case(n, d, max_rows, reduce):
  """(clips, caps, num_clips, num_caps, G64 [videos, paragraphs], noise) of a near-tie shape — cached, read-only.
  noise: float64_noise() of the fixture (unit rows), the bound on |implementation - true| of any G64."""
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  S64 = clips.astype(np.float64) @ caps.astype(np.float64).T
  return clips, caps, nc, ns, G64, float64_noise(S64, nc, ns, d, reduce)


def fp32_block_scores(clips, caps, nc, ns, reduce):
  """NumPy's fp32 block scores: cmhse_group_scores' reduction of one fp32 summation order (BLAS's)."""
  return block_scores(clips @ caps.T, nc, ns, reduce).astype(np.float32).astype(np.float64)


def near_tie_ks(B):
  return sorted({1, 10, min(50, B)})


# K = B (the full sort) on the shapes where the CPU re-check below finds no query left out under the test's own
# rule, in both reduce modes and both directions.  (22, 64, 5) has B = 132 groups, past CMHSE_TOPK_MAX = 128: no
# K = B call exists for it.  On the two shapes here min(50, B) is B already.
FULL_SORT_SHAPES = [(4, 96, 100), (3, 1024, 128)]


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------
def test_reference_on_a_hand_written_matrix():
  Q = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                [0.0, -0.0, -1.0, 0.0, -0.0],
                [5.0, 4.0, 4.0, 4.0, 1.0],
                [-2.0, -2.0, -3.0, -2.0, -2.0]])
  s, ix = group_topk_exact_reference(Q, 2)
  assert ix.tolist() == [[1, 2], [0, 1], [0, 1], [0, 1]]      # the tie across the K-th place: smaller index in
  assert s.tolist() == [[3.0, 3.0], [0.0, 0.0], [5.0, 4.0], [-2.0, -2.0]]
  s, ix = group_topk_exact_reference(Q, 5)                    # K = gallery: a full stable sort
  assert ix.tolist() == [[1, 2, 4, 3, 0], [0, 1, 3, 4, 2], [0, 1, 2, 3, 4], [0, 1, 3, 4, 2]]
  assert not np.signbit(s[1, :4]).any()                       # +-0.0 tie, in index order, and come back as +0.0
  s, ix = group_topk_exact_reference(Q, 1)
  assert ix.ravel().tolist() == [1, 0, 0, 0]
  # tie-free: numpy's argsort
  R = np.random.RandomState(0).standard_normal((20, 33))
  assert np.array_equal(group_topk_exact_reference(R, 7)[1], np.argsort(-R, axis=1)[:, :7])
  assert np.array_equal(group_topk_exact_reference(query_view(R, 'p2v'), 3)[1], np.argsort(-R.T, axis=1)[:, :3])


def test_comparable_rule():
  big = 1.0
  Q = np.array([[9.0, 7.0, 5.0, 3.0, 3.0 - big, 0.0],           # all gaps large
                [9.0, 9.0 - 1e-13, 5.0, 3.0, 1.0, 0.0],         # a gap inside (0, GROUP_GAP] at the top
                [9.0, 7.0, 5.0, 5.0, 1.0, 0.0],                 # a zero gap between groups 2 and 3: not planted
                [7.0, 1.0, 5.0, 3.0, 2.0, 7.0]])                # a zero gap between groups 0 and 5: planted (n = 1)
  assert comparable_queries(Q, 1, planted=(5, 1)).tolist() == [True, False, True, True]
  assert comparable_queries(Q, 3, planted=(5, 1)).tolist() == [True, False, False, True]
  assert comparable_queries(Q, 6, planted=(5, 1)).tolist() == [True, False, False, True]      # K = gallery: K entries
  assert comparable_queries(Q, 1).tolist() == [True, False, True, False]                # no planted pairs known
  # a gallery subset: the original indices decide what is planted
  assert comparable_queries(Q[:, [5, 1, 0]], 1, planted=(5, 1), orig=[5, 1, 0]).tolist() == [True, False, True, True]
  assert comparable_queries(Q[:, [5, 1, 0]], 1, planted=(5, 1), orig=[4, 1, 0]).tolist() == [True, False, True, False]


# ---------------------------------------------------------------------------------------------
# the fixtures: which queries are compared, and that the comparison has teeth
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', GROUP_NEAR_TIE_SHAPES)
def test_near_tie_fixture_serves_lists(n, d, max_rows, reduce):
  clips, caps, nc, ns, G64, noise = near_tie_case(n, d, max_rows, reduce)
  B = 6 * n
  assert 4 * noise < GROUP_GAP
  G32 = fp32_block_scores(clips, caps, nc, ns, reduce)
  for direction in DIRECTIONS:
    Q, Q32 = query_view(G64, direction), query_view(G32, direction)
    ks = near_tie_ks(B) + ([B] if (n, d, max_rows) in FULL_SORT_SHAPES else [])
    for k in ks:
      left_out = int(B - np.count_nonzero(comparable_queries(Q, k, planted=planted_pairs(n))))
      print('%s %s K=%d: %d of %d queries left out' % ((n, d, max_rows), direction, k, left_out, B))
      assert left_out <= MAX_LEFT_OUT * B, (direction, k, left_out, B)
      if k == 1 or k == B and k not in near_tie_ks(B):
        assert left_out == 0, (direction, k, left_out)
    # teeth: one fp32 summation order lists at least half the queries differently at K = 10
    k = min(10, B)
    want, got = group_topk_exact_reference(Q, k)[1], group_topk_exact_reference(Q32, k)[1]
    differ = int(np.count_nonzero((want != got).any(axis=1)))
    print('%s %s %s: NumPy-fp32 lists differ on %d of %d queries at K = %d' % ((n, d, max_rows), reduce, direction,
                                                                                differ, B, k))
    assert 2 * differ >= B


def members_below_gk(Q32, want, k):
  """The queries with a member of the float64 top-k whose fp32 block score lies strictly below the k-th largest
  fp32 block score of the query: a re-sort of the fp32 list's own k members cannot return them."""
  gk = -np.sort(-Q32, axis=1)[:, k - 1]
  return np.flatnonzero((np.take_along_axis(Q32, want, axis=1) < gk[:, None]).any(axis=1))


def test_some_float64_member_lies_below_the_fp32_kth_score():
  """The 2 E candidate rule is exercised: an implementation that re-sorts, or recomputes in float64, only the
  fp32 list's own K members fails the GPU comparison on these queries."""
  hit = {}
  for n, d, max_rows in GROUP_NEAR_TIE_SHAPES:
    for reduce in REDUCES:
      clips, caps, nc, ns, G64, _ = near_tie_case(n, d, max_rows, reduce)
      G32 = fp32_block_scores(clips, caps, nc, ns, reduce)
      for direction in DIRECTIONS:
        Q, Q32 = query_view(G64, direction), query_view(G32, direction)
        for k in near_tie_ks(6 * n):
          ok = comparable_queries(Q, k, planted=planted_pairs(n))
          below = members_below_gk(Q32, group_topk_exact_reference(Q, k)[1], k)
          hit[(n, d, max_rows, reduce, direction, k)] = int(np.count_nonzero(ok[below]))
  print('comparable queries with a float64 member below the fp32 K-th score:', hit)
  assert max(hit.values()) > 0        # (under 'mean', where fp32 rounds the block score itself; none under 'max')


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def _plan(lib, nclips, ncaps, direction, k, exact=True):
  Bv, Bp = len(nclips), len(ncaps)
  oc, os_ = _offsets(nclips).astype(np.int32), _offsets(ncaps).astype(np.int32)
  plan = np.zeros(2 * Bv + 2 * Bp + 12, dtype=np.int32)
  fn = lib.cmhse_group_topk_exact_plan if exact else lib.cmhse_group_topk_plan
  n = fn(oc.ctypes.data, Bv, os_.ctypes.data, Bp, direction, k, plan.ctypes.data, plan.size)
  assert n > 0, n
  return plan[:n].copy()


def _query_tile_groups(plan):
  Bv, Bp, direction, R, C = int(plan[0]), int(plan[1]), int(plan[4]), int(plan[6]), int(plan[7])
  rt = plan[HDR + Bv + 1 + Bp + 1:]
  start = rt[R + 1:R + 1 + C + 1] if direction == P2V else rt[:R + 1]
  return np.diff(start)


def test_plan_layout_and_cap(lib):
  rng = np.random.RandomState(5)
  nclips, ncaps = rng.randint(1, 9, 300).tolist(), rng.randint(1, 5, 210).tolist()
  for direction in (P2V, V2P):
    for k in (1, 10, 50, 128):
      plan = _plan(lib, nclips, ncaps, direction, k)
      plan32 = _plan(lib, nclips, ncaps, direction, k, exact=False)
      Bv, Bp, R, C = 300, 210, int(plan[6]), int(plan[7])
      assert plan[:6].tolist() == [Bv, Bp, sum(nclips), sum(ncaps), direction, k] == plan32[:6].tolist()
      assert len(plan) == HDR + Bv + Bp + R + C + 4
      assert np.array_equal(plan[HDR:HDR + Bv + 1], _offsets(nclips))
      assert np.array_equal(plan[HDR + Bv + 1:HDR + Bv + Bp + 2], _offsets(ncaps))
      rt = plan[HDR + Bv + Bp + 2:]
      assert rt[0] == 0 and rt[R] == Bv and rt[R + 1] == 0 and rt[R + 1 + C] == Bp
      assert (np.diff(rt[:R + 1]) > 0).all() and (np.diff(rt[R + 1:]) > 0).all()
      # the gallery side packs as cmhse_group_topk_plan's; the query side is never looser
      g = slice(HDR + Bv + Bp + 2, HDR + Bv + Bp + 2 + R + 1) if direction == P2V else None
      if g is not None:
        assert np.array_equal(plan[g], plan32[g])
      assert _query_tile_groups(plan).max() <= _query_tile_groups(plan32).max()
      assert lib.cmhse_group_topk_exact_workspace(plan.ctypes.data, len(plan)) > 0
      # a plan for the certified call serves the nested fp32 call
      assert lib.cmhse_group_topk_workspace(plan.ctypes.data, len(plan)) > 0
  # the cap itself, from single-row groups: never above the fp32 plan's, at every K
  ones = [1] * 200
  for k in range(1, 129):
    cap = int(_query_tile_groups(_plan(lib, ones, ones, P2V, k)).max())
    cap32 = int(_query_tile_groups(_plan(lib, ones, ones, P2V, k, exact=False)).max())
    assert 8 <= cap <= cap32 <= 64 and cap % 8 == 0, (k, cap, cap32)
    assert cap == int(_query_tile_groups(_plan(lib, ones, ones, V2P, k)).max())


def test_fp32_plan_past_the_exact_cap_is_refused(lib):
  ones = [1] * 200
  plan32 = _plan(lib, ones, ones, P2V, 128, exact=False)
  plan = _plan(lib, ones, ones, P2V, 128)
  assert _query_tile_groups(plan32).max() > _query_tile_groups(plan).max()
  assert lib.cmhse_group_topk_workspace(plan32.ctypes.data, len(plan32)) > 0
  assert lib.cmhse_group_topk_exact_workspace(plan32.ctypes.data, len(plan32)) == 0
  fake = ctypes.c_void_p(256)
  args = lambda p: (fake, fake, 200, 200, 8, p.ctypes.data, fake, len(p), P2V, 1, 128, fake, fake, fake,
                    ctypes.c_void_p(1 << 20), 1 << 40, None)
  assert lib.cmhse_group_topk_exact(*args(plan32)) == ERR_ARG
  # (the exact plan with D past the bound: through every argument and workspace check, nothing launched)
  a = list(args(plan))
  a[4] = 1 << 24
  assert lib.cmhse_group_topk_exact(*a) == ERR_UNSUPPORTED


def test_workspace_size(lib):
  ws = lib.cmhse_group_topk_exact_workspace
  assert ws(None, 0) == 0
  plan = _plan(lib, [2, 1, 3], [1, 1, 2, 4], P2V, 2)
  assert ws(plan.ctypes.data, len(plan)) % 256 == 0 and ws(plan.ctypes.data, len(plan)) > 0
  assert ws(plan.ctypes.data, len(plan) - 1) == 0 and ws(plan.ctypes.data, HDR - 1) == 0
  for idx, val in [(0, 0), (4, 2), (5, 0), (5, 4), (6, 0), (HDR, 1), (HDR + 1, 0)]:
    edited = plan.copy()
    edited[idx] = val
    assert ws(edited.ctypes.data, len(edited)) == 0, (idx, val)
  # fixed by the query side and K once the gallery has a tile per panel: twice the gallery, the same bytes
  queries = np.random.RandomState(2).randint(1, 6, 300).tolist()
  for direction in (P2V, V2P):
    for k in (1, 10, 50, 128):
      sizes = []
      for groups in (2000, 4000):
        gallery = [64] * groups
        nclips, ncaps = (gallery, queries) if direction == P2V else (queries, gallery)
        plan = _plan(lib, nclips, ncaps, direction, k)
        b = ws(plan.ctypes.data, len(plan))
        base = lib.cmhse_group_topk_workspace(plan.ctypes.data, len(plan))
        assert b % 256 == 0 and b > base + 8 * 300 * k + 8 * sum(queries) + 4 * 300 + 12 * 300 * k + 4 * 300
        sizes.append(b)
      assert sizes[0] == sizes[1], (direction, k, sizes)


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_group_topk_exact is returned before anything touches the device, in the documented
  order: arguments, then the workspace, then D."""
  nclips, ncaps = [2, 1, 3], [1, 1, 2, 4]
  plan = _plan(lib, nclips, ncaps, P2V, 2)
  n = len(plan)
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_group_topk_exact_workspace(plan.ctypes.data, n)
  good = dict(C=fake, S=fake, Nc=6, Ns=8, D=8, ph=plan.ctypes.data, pd=fake, plen=n, direction=P2V, reduce=1, K=2,
              scores=fake, index=fake, resolved=fake, ws=ctypes.c_void_p(1 << 20), ws_bytes=0)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_topk_exact(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['ph'], a['pd'], a['plen'],
                                      a['direction'], a['reduce'], a['K'], a['scores'], a['index'], a['resolved'],
                                      a['ws'], a['ws_bytes'], None)

  assert call() == ERR_WORKSPACE                 # valid arguments, no workspace
  assert call(reduce=0) == ERR_WORKSPACE
  bads = [dict(C=None), dict(S=None), dict(ph=None), dict(pd=None), dict(scores=None), dict(index=None),
          dict(resolved=None), dict(ws=None), dict(Nc=7), dict(Ns=7), dict(Nc=0), dict(Ns=0), dict(D=0), dict(D=-1),
          dict(plen=n - 1), dict(plen=n + 1), dict(reduce=2), dict(reduce=-1), dict(direction=V2P),
          dict(direction=2), dict(K=1), dict(K=3), dict(K=0)]
  for bad in bads:
    assert call(**bad) == ERR_ARG, bad                              # before the workspace check ...
    assert call(ws_bytes=ws_ok, **bad) == ERR_ARG, bad              # ... and with a workspace that would pass it
    if 'D' not in bad:                                              # ... and before the check on D
      assert call(D=1 << 24, ws_bytes=ws_ok, **bad) == ERR_ARG, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=ws_ok) == ERR_WORKSPACE     # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == ERR_WORKSPACE                                       # too small
  assert call(ws_bytes=lib.cmhse_group_topk_workspace(plan.ctypes.data, n)) == ERR_WORKSPACE   # the fp32 call's
  assert call(D=1 << 24) == ERR_WORKSPACE                          # the workspace before D
  assert call(D=1 << 24, ws_bytes=ws_ok) == ERR_UNSUPPORTED
  assert call(D=(1 << 24) + 5, ws_bytes=ws_ok) == ERR_UNSUPPORTED
  # a host plan whose tiles were edited: rejected (the kernels trust its bounds)
  for idx, val in [(HDR, 1), (6, 2), (7, 0), (HDR + 4 + 5, 1)]:
    edited = plan.copy()
    edited[idx] = val
    assert call(ph=edited.ctypes.data, ws_bytes=ws_ok) == ERR_ARG, (idx, val)


def test_plan_errors_and_degenerate_inputs(lib):
  oc, os_ = _offsets([2, 1, 3]).astype(np.int32), _offsets([1, 1, 2, 4]).astype(np.int32)
  buf = np.zeros(2 * 3 + 2 * 4 + 12, dtype=np.int32)

  def plan(oc_=oc, Bv=3, os__=os_, Bp=4, direction=P2V, K=2, out=buf, cap=None):
    return lib.cmhse_group_topk_exact_plan(None if oc_ is None else oc_.ctypes.data, Bv,
                                           None if os__ is None else os__.ctypes.data, Bp, direction, K,
                                           None if out is None else out.ctypes.data, buf.size if cap is None else cap)

  assert plan() == HDR + 3 + 4 + 1 + 1 + 4
  for bad in [dict(oc_=None), dict(os__=None), dict(out=None), dict(Bv=0), dict(Bp=0), dict(Bv=-1), dict(direction=2),
              dict(direction=-1), dict(K=0), dict(K=4), dict(K=-1), dict(direction=V2P, K=5), dict(K=129)]:
    assert plan(**bad) == ERR_ARG, bad
  assert plan(K=3) > 0 and plan(direction=V2P, K=4) > 0             # K = gallery groups
  assert plan(cap=buf.size - 1) == ERR_WORKSPACE
  bad_off = np.array([0, 2, 2, 6], dtype=np.int32)                  # an empty video
  assert plan(oc_=bad_off) == ERR_ARG
  long_ = _offsets([3, 129, 1]).astype(np.int32)
  assert plan(oc_=long_) == ERR_UNSUPPORTED
  # one query, one gallery group, one row each
  one = _plan(lib, [1], [1], P2V, 1)
  assert one.tolist() == [1, 1, 1, 1, P2V, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1]
  assert lib.cmhse_group_topk_exact_workspace(one.ctypes.data, len(one)) > 0


def test_ops_and_evaluation_argument_errors():
  from cmhse_amd import evaluation, ops
  c, s = torch.zeros(6, 4), torch.zeros(8, 4)
  good = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], k=2, direction='p2v', reduce='max')
  for kw in [dict(num_clips=[2, 0, 4]), dict(num_clips=[2, 1, 2]), dict(num_caps=[1, 1, 2]), dict(reduce='sum'),
             dict(direction='both'), dict(k=0), dict(k=4), dict(k=True), dict(k=2.0), dict(direction='v2p', k=5),
             dict(num_clips=[]), dict(num_clips=[2, 1.5, 2.5])]:
    args = dict(good, **kw)
    with pytest.raises(ValueError):
      ops.group_topk_exact(c, s, **args)
    if 'reduce' not in kw:
      with pytest.raises(ValueError):
        ops.group_topk_exact_plan(args['num_clips'], args['num_caps'], 6, 8, args['k'], args['direction'])
    with pytest.raises(ValueError):
      evaluation.group_retrieve(c.numpy(), s.numpy(), exact=True, **args)
  with pytest.raises(ValueError):
    ops.group_topk_exact(torch.zeros(130, 4), torch.zeros(2, 4), [129, 1], [1, 1], 1)
  with pytest.raises(ValueError):
    ops.group_topk_exact(torch.zeros(6, 4), torch.zeros(8, 5), **good)
  with pytest.raises(ValueError):
    ops.group_topk_exact(torch.zeros(6), s, **good)
  for exact in ('yes', None, 1, 0, 'exact', 1.0):                    # anything other than a bool
    with pytest.raises(ValueError):
      evaluation.group_retrieve(c.numpy(), s.numpy(), exact=exact, **good)
  for top1 in ('best', None, True, 'float64'):
    with pytest.raises(ValueError):
      evaluation.group_i2t_t2i_exact(c.numpy(), s[:6].numpy(), [2, 1, 3], top1=top1)
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(c.numpy(), s.numpy(), [2, 1, 3], [1, 1, 6], top1='exact', ties='neither')
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(c.numpy(), s.numpy(), [2, 1, 3], top1='exact')      # 6 != 8 caption rows
  plan = ops.group_topk_exact_plan([2, 1, 3], [1, 1, 2, 4], 6, 8, 2, 'p2v')
  assert plan.dtype == np.int32 and plan[:6].tolist() == [3, 4, 6, 8, P2V, 2]


def test_needs_device_tensors_and_dropin_reexport():
  from cmhse_amd import evaluation, ops
  from cmhse_amd.dropin import evaluation as dropin
  with pytest.raises(RuntimeError):
    ops.group_topk_exact(torch.zeros(6, 4), torch.zeros(8, 4), [2, 1, 3], [1, 1, 2, 4], 2)
  assert dropin.group_retrieve is evaluation.group_retrieve
  assert dropin.group_i2t_t2i_exact is evaluation.group_i2t_t2i_exact
  assert inspect.signature(dropin.group_retrieve).parameters['exact'].default is False
  assert inspect.signature(dropin.group_i2t_t2i_exact).parameters['top1'].default == 'fp32'
