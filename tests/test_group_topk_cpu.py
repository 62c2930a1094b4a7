"""Group-wise top-K without a GPU: the tile plan of cmhse_group_topk_plan, the workspace size, argument
validation (include/cmhse_hip.h) and the ValueErrors of ops.group_topk / evaluation.group_retrieve."""
import ctypes
import os

import numpy as np
import pytest
import torch

from score_shapes import qcap      # group.hip gt_qcap restated: query groups per query tile at K

HDR = 8
P2V, V2P = 0, 1
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def _offsets(counts):
  off = np.zeros(len(counts) + 1, dtype=np.int32)
  np.cumsum(counts, out=off[1:])
  return off


def _plan(lib, clips, caps, direction, K, cap=None):
  Bv, Bp = len(clips), len(caps)
  oc, op = _offsets(clips), _offsets(caps)
  plan = np.full(2 * Bv + 2 * Bp + 12 if cap is None else cap, -7, dtype=np.int32)
  n = lib.cmhse_group_topk_plan(oc.ctypes.data, Bv, op.ctypes.data, Bp, direction, K, plan.ctypes.data,
                                plan.size)
  return n, plan


def _tiles(plan):
  Bv, Bp, R, C = (int(x) for x in (plan[0], plan[1], plan[6], plan[7]))
  clip_off = plan[HDR:HDR + Bv + 1]
  cap_off = plan[HDR + Bv + 1:HDR + Bv + Bp + 2]
  rt = plan[HDR + Bv + Bp + 2:HDR + Bv + Bp + 3 + R]
  ct = plan[HDR + Bv + Bp + 3 + R:HDR + Bv + Bp + 4 + R + C]
  return clip_off, cap_off, rt, ct


def _check_tiling(off, start, B, max_groups):
  assert start[0] == 0 and start[-1] == B
  assert (np.diff(start) > 0).all()                       # every group whole in exactly one tile, in order
  rows = off[start[1:]] - off[start[:-1]]
  assert (rows <= 128).all() and (rows >= 1).all()        # no tile holds more than 128 rows
  assert rows.sum() == off[B]                             # the tiles cover every row, in order
  assert (np.diff(start) <= max_groups).all()             # the query side's group cap
  for t in range(len(start) - 2):                         # greedy: the next group would not have fitted
    nxt = start[t + 1]
    assert off[nxt + 1] - off[start[t]] > 128 or nxt - start[t] >= max_groups


def _check_plan(lib, clips, caps, direction, K):
  n, plan = _plan(lib, clips, caps, direction, K)
  assert n > 0, n
  Bv, Bp = len(clips), len(caps)
  assert list(plan[:6]) == [Bv, Bp, sum(clips), sum(caps), direction, K]
  R, C = int(plan[6]), int(plan[7])
  assert n == HDR + Bv + Bp + R + C + 4 <= 2 * Bv + 2 * Bp + 12
  assert (plan[n:] == -7).all()                           # nothing written past the returned length
  clip_off, cap_off, rt, ct = _tiles(plan)
  assert np.array_equal(clip_off, _offsets(clips)) and np.array_equal(cap_off, _offsets(caps))
  big = 1 << 30
  _check_tiling(clip_off, rt, Bv, qcap(K) if direction == V2P else big)
  _check_tiling(cap_off, ct, Bp, qcap(K) if direction == P2V else big)
  return plan[:n]


def test_header_constants_match_lib():
  from cmhse_amd import _lib
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             'include', 'cmhse_hip.h')).read()
  assert '#define CMHSE_GROUP_P2V %d' % _lib.GROUP_P2V in header
  assert '#define CMHSE_GROUP_V2P %d' % _lib.GROUP_V2P in header
  assert (_lib.GROUP_P2V, _lib.GROUP_V2P) == (P2V, V2P)
  assert '#define CMHSE_GROUP_TOPK_PLAN_MAX(Bv, Bp) (2 * (Bv) + 2 * (Bp) + 12)' in header
  assert _lib.group_topk_plan_max(10, 7) == 46
  assert '#define CMHSE_TOPK_MAX %d' % _lib.TOPK_MAX in header


def test_query_cap_table():
  # the numbers group.hip's comment states: K = 1 / 10 / 50 / 128 -> 64 / 56 / 40 / 64 query groups
  assert [qcap(k) for k in (1, 10, 50, 128)] == [64, 56, 40, 64]


@pytest.mark.parametrize('direction', [P2V, V2P])
@pytest.mark.parametrize('seed,Bv,Bp,hi,K', [(0, 1, 1, 5, 1), (1, 7, 40, 40, 7), (2, 300, 120, 30, 10),
                                             (3, 500, 700, 128, 50), (4, 4917, 2000, 6, 128),
                                             (5, 900, 900, 2, 128), (6, 200, 300, 2, 1)])
def test_plan_invariants_random_counts(lib, direction, seed, Bv, Bp, hi, K):
  rng = np.random.RandomState(seed)
  clips = rng.randint(1, hi, size=Bv)
  caps = rng.randint(1, hi, size=Bp)
  K = min(K, Bv if direction == P2V else Bp)
  _check_plan(lib, clips, caps, direction, K)


@pytest.mark.parametrize('direction', [P2V, V2P])
@pytest.mark.parametrize('K', [1, 10, 50, 128])
def test_plan_val1_profile(lib, direction, K):
  from cmhse_amd import synthetic
  nclips = np.asarray(synthetic.anet_like_spec(4917).num_clips)
  assert nclips.sum() == 17502
  plan = _check_plan(lib, nclips, nclips, direction, K)
  R, C = int(plan[6]), int(plan[7])
  q_tiles, g_tiles = (C, R) if direction == P2V else (R, C)
  assert g_tiles <= 145                                   # the gallery packs as cmhse_group_plan does
  assert q_tiles >= -(-4917 // qcap(K))


def test_plan_all_ones_hits_the_cap(lib):
  ones = [1] * 1000
  for K in (1, 10, 50, 128):
    plan = _check_plan(lib, ones, ones, P2V, K)
    _, _, rt, ct = _tiles(plan)
    assert set(np.diff(ct)[:-1]) == {qcap(K)}             # query tiles: full at the cap
    assert set(np.diff(rt)[:-1]) == {128}                 # gallery tiles: full at 128 rows


def test_plan_errors(lib):
  clips, caps = [2, 1, 3], [1, 1, 2, 4]
  assert _plan(lib, clips, caps, P2V, 1)[0] > 0
  assert _plan(lib, clips, caps, P2V, 0)[0] == ERR_ARG                 # K = 0
  assert _plan(lib, clips, caps, P2V, 4)[0] == ERR_ARG                 # K > 3 videos in the gallery
  assert _plan(lib, clips, caps, V2P, 4)[0] > 0                        # ... 4 paragraphs in this one
  assert _plan(lib, clips, caps, V2P, 5)[0] == ERR_ARG
  big = [1] * 200
  assert _plan(lib, big, big, P2V, 128)[0] > 0
  assert _plan(lib, big, big, P2V, 129)[0] == ERR_ARG                  # K > CMHSE_TOPK_MAX
  assert _plan(lib, clips, caps, 2, 1)[0] == ERR_ARG                   # direction
  assert _plan(lib, clips, caps, -1, 1)[0] == ERR_ARG
  assert _plan(lib, [2, 0, 3], caps, P2V, 1)[0] == ERR_ARG             # bad prefix sums
  assert _plan(lib, clips, [1, -1, 2, 4], V2P, 1)[0] == ERR_ARG
  assert _plan(lib, [3, 129, 2], caps, P2V, 1)[0] == ERR_UNSUPPORTED   # an oversize video
  assert _plan(lib, clips, [1, 1, 129, 4], P2V, 1)[0] == ERR_UNSUPPORTED
  assert _plan(lib, clips, caps, P2V, 1, cap=2 * 3 + 2 * 4 + 11)[0] == ERR_WORKSPACE
  oc, op = _offsets(clips), _offsets(caps)
  plan = np.zeros(64, dtype=np.int32)
  assert lib.cmhse_group_topk_plan(None, 3, op.ctypes.data, 4, P2V, 1, plan.ctypes.data, 64) == ERR_ARG
  assert lib.cmhse_group_topk_plan(oc.ctypes.data, 3, None, 4, P2V, 1, plan.ctypes.data, 64) == ERR_ARG
  assert lib.cmhse_group_topk_plan(oc.ctypes.data, 3, op.ctypes.data, 4, P2V, 1, None, 64) == ERR_ARG
  assert lib.cmhse_group_topk_plan(oc.ctypes.data, 0, op.ctypes.data, 4, P2V, 1, plan.ctypes.data, 64) == ERR_ARG
  assert lib.cmhse_group_topk_plan(oc.ctypes.data, 3, op.ctypes.data, 0, P2V, 1, plan.ctypes.data, 64) == ERR_ARG
  bad = np.array([1, 2, 3, 6], dtype=np.int32)                         # does not start at 0
  assert lib.cmhse_group_topk_plan(bad.ctypes.data, 3, op.ctypes.data, 4, P2V, 1, plan.ctypes.data,
                                   64) == ERR_ARG


def _workspace(lib, plan):
  plan = np.ascontiguousarray(plan, dtype=np.int32)
  return lib.cmhse_group_topk_workspace(plan.ctypes.data, plan.size)


def test_workspace_does_not_grow_with_the_gallery(lib):
  from cmhse_amd import synthetic
  queries = np.asarray(synthetic.anet_like_spec(4917).num_clips)
  rng = np.random.RandomState(9)
  sizes = {}
  for G in (5000, 1000000):
    videos = rng.randint(1, 7, size=G)
    for K in (10, 50):
      n, plan = _plan(lib, videos, queries, P2V, K)
      assert n > 0
      sizes[G, K] = _workspace(lib, plan[:n])
      n, plan = _plan(lib, queries, videos, V2P, K)
      assert n > 0
      assert _workspace(lib, plan[:n]) == sizes[G, K]     # the same query side, the other direction
  for K in (10, 50):
    assert sizes[5000, K] == sizes[1000000, K] > 0
    assert sizes[5000, K] % 256 == 0
    assert sizes[5000, K] >= 4917 * K * 8
  assert sizes[5000, 50] < 16 * 1000 * 1000


def test_workspace_of_invalid_plans_is_zero(lib):
  n, plan = _plan(lib, [2, 1, 3], [1, 1, 2, 4], P2V, 2)
  plan = plan[:n].copy()
  assert _workspace(lib, plan) > 0
  assert lib.cmhse_group_topk_workspace(None, n) == 0
  assert lib.cmhse_group_topk_workspace(plan.ctypes.data, n - 1) == 0
  edited = plan.copy()
  edited[5] = 4                                           # K beyond the 3-video gallery
  assert _workspace(lib, edited) == 0


def test_call_argument_errors_without_gpu(lib):
  """Every error of cmhse_group_topk is returned before anything is launched."""
  clips, caps = [2, 1, 3], [1, 1, 2, 4]
  n, plan = _plan(lib, clips, caps, P2V, 2)
  plan = plan[:n].copy()
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = _workspace(lib, plan)
  good = dict(C=fake, S=fake, Nc=6, Ns=8, D=8, ph=plan.ctypes.data, pd=fake, plen=n, direction=P2V,
              reduce=1, K=2, scores=fake, index=fake, ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_topk(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['ph'], a['pd'], a['plen'],
                                a['direction'], a['reduce'], a['K'], a['scores'], a['index'], a['ws'],
                                a['ws_bytes'], None)

  bads = [dict(C=None), dict(S=None), dict(ph=None), dict(pd=None), dict(scores=None), dict(index=None),
          dict(ws=None), dict(Nc=7), dict(Ns=7), dict(Nc=0), dict(D=0), dict(D=-1), dict(plen=n - 1),
          dict(plen=n + 1), dict(reduce=2), dict(reduce=-1),
          dict(direction=V2P), dict(direction=2),              # the plan's direction is p2v
          dict(K=1), dict(K=3), dict(K=0), dict(K=129)]        # the plan's K is 2
  for bad in bads:
    assert call(**bad) == ERR_ARG, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16)) == ERR_WORKSPACE
  assert call(ws_bytes=ws_ok - 1) == ERR_WORKSPACE
  assert call(ws_bytes=0) == ERR_WORKSPACE
  # a host plan whose tiles or counts were edited: rejected (the kernels trust its bounds)
  for idx, val in [(0, 4), (1, 3), (HDR, 1), (HDR + 2, 0), (6, 2), (7, 2), (HDR + 3 + 1 + 4, 0)]:
    edited = plan.copy()
    edited[idx] = val
    assert call(ph=edited.ctypes.data) == ERR_ARG, (idx, val)
  # a query tile over the group cap of K: rejected
  ones = [1] * 100
  n2, p2 = _plan(lib, ones, ones, P2V, 50)
  p2 = p2[:n2].copy()
  _, _, rt, ct = _tiles(p2)
  assert int(ct[1]) == qcap(50)
  p2[HDR + 101 + 101 + len(rt) + 1] += 1                  # the second caption tile starts one later
  assert lib.cmhse_group_topk(fake, fake, 100, 100, 8, p2.ctypes.data, fake, n2, P2V, 1, 50, fake, fake,
                              ctypes.c_void_p(1 << 20), 1 << 30, None) == ERR_ARG


def test_ops_group_topk_value_errors_without_gpu():
  from cmhse_amd import ops
  c, s = torch.zeros(6, 4), torch.zeros(8, 4)
  good = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], k=2, direction='p2v', reduce='max')
  bads = [dict(reduce='sum'), dict(direction='both'), dict(k=0), dict(k=4), dict(k=129), dict(k=2.5),
          dict(direction='v2p', k=5), dict(num_clips=[2, 0, 4]), dict(num_clips=[2, 1, 2]),
          dict(num_caps=[1, 1, 2, 3]), dict(num_caps=[]), dict(num_clips=[2, 1.5, 2.5])]
  for bad in bads:
    with pytest.raises(ValueError):
      ops.group_topk(c, s, **dict(good, **bad))
  with pytest.raises(ValueError):
    ops.group_topk(torch.zeros(6), s, **good)
  with pytest.raises(ValueError):
    ops.group_topk(c, torch.zeros(8, 5), **good)
  with pytest.raises(ValueError):
    ops.group_topk(c.numpy(), s, **good)
  with pytest.raises(ValueError):
    ops.group_topk(torch.zeros(200, 4), torch.zeros(200, 4), [1] * 200, [1] * 200, 129)
  with pytest.raises(ValueError):                        # a 129-clip video
    ops.group_topk(torch.zeros(130, 4), torch.zeros(2, 4), [129, 1], [1, 1], 1)


def test_group_retrieve_value_errors_without_gpu():
  from cmhse_amd import evaluation
  c, s = np.zeros((6, 4), np.float32), np.zeros((8, 4), np.float32)
  good = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], k=2, direction='p2v', reduce='max')
  for bad in [dict(reduce='median'), dict(direction='x'), dict(k=0), dict(k=4), dict(k=129),
              dict(num_caps=None), dict(num_clips=[3, 3, 1])]:
    with pytest.raises(ValueError):
      evaluation.group_retrieve(c, s, **dict(good, **bad))
  with pytest.raises(ValueError):
    evaluation.group_retrieve(c, np.zeros((8, 5), np.float32), **good)
  with pytest.raises(ValueError):
    evaluation.group_retrieve(np.zeros(6, np.float32), s, **good)
  stats = dict(evaluation.CACHE_STATS)
  last = evaluation._LAST_ENCODE[0]
  with pytest.raises(ValueError):
    evaluation.group_retrieve(c, np.zeros((6, 4), np.float32), [2, 1, 3], k=3, direction='v2p', reduce='sum')
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
