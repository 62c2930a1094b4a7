"""Group-wise scores without a GPU: the tile plan of cmhse_group_plan, workspace size, argument
validation (include/cmhse_hip.h), and the NumPy restatement of G the GPU tests compare against."""
import ctypes
import os

import numpy as np
import pytest
import torch

HDR = 5
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def _offsets(counts):
  off = np.zeros(len(counts) + 1, dtype=np.int32)
  np.cumsum(counts, out=off[1:])
  return off


def _plan(lib, clips, caps, cap=None):
  B = len(clips)
  oc, os_ = _offsets(clips), _offsets(caps)
  plan = np.full(4 * B + 9 if cap is None else cap, -7, dtype=np.int32)
  n = lib.cmhse_group_plan(oc.ctypes.data, os_.ctypes.data, B, plan.ctypes.data, plan.size)
  return n, plan


def _tiles(plan):
  B, R, C = int(plan[0]), int(plan[3]), int(plan[4])
  clip_off = plan[HDR:HDR + B + 1]
  cap_off = plan[HDR + B + 1:HDR + 2 * B + 2]
  rt = plan[HDR + 2 * B + 2:HDR + 2 * B + 3 + R]
  ct = plan[HDR + 2 * B + 3 + R:HDR + 2 * B + 4 + R + C]
  return clip_off, cap_off, rt, ct


def _check_tiling(off, start, B):
  assert start[0] == 0 and start[-1] == B
  assert (np.diff(start) > 0).all()                       # every group in exactly one tile, in order
  rows = off[start[1:]] - off[start[:-1]]
  assert (rows <= 128).all() and (rows >= 1).all()        # no tile exceeds its rows
  assert rows.sum() == off[B]                             # the tiles cover every row, in order
  # greedy: the next group would not have fitted into a tile
  for t in range(len(start) - 2):
    assert off[start[t + 1] + 1] - off[start[t]] > 128


def _ragged(rng, B, hi=30):
  return rng.randint(1, hi, size=B)


@pytest.mark.parametrize('seed,B,hi', [(0, 1, 5), (1, 7, 40), (2, 300, 30), (3, 500, 128), (4, 4917, 6)])
def test_plan_invariants(lib, seed, B, hi):
  rng = np.random.RandomState(seed)
  clips = _ragged(rng, B, hi)
  caps = _ragged(rng, B, hi)
  n, plan = _plan(lib, clips, caps)
  assert n > 0
  assert plan[0] == B and plan[1] == clips.sum() and plan[2] == caps.sum()
  R, C = int(plan[3]), int(plan[4])
  assert n == HDR + 2 * (B + 1) + R + 1 + C + 1 <= 4 * B + 9
  clip_off, cap_off, rt, ct = _tiles(plan)
  assert np.array_equal(clip_off, _offsets(clips)) and np.array_equal(cap_off, _offsets(caps))
  _check_tiling(clip_off, rt, B)
  _check_tiling(cap_off, ct, B)
  assert (plan[n:] == -7).all()          # nothing written past the returned length


def test_plan_val1_shape(lib):
  from cmhse_amd import synthetic
  nclips = np.asarray(synthetic.anet_like_spec(4917).num_clips)
  assert nclips.sum() == 17502
  n, plan = _plan(lib, nclips, nclips)
  clip_off, cap_off, rt, ct = _tiles(plan)
  _check_tiling(clip_off, rt, 4917)
  assert np.array_equal(rt, ct)
  # whole-video packing costs few tiles over a plain 128-row tiling (137 there)
  assert int(plan[3]) <= 145


def test_plan_exact_tile_and_oversize(lib):
  n, plan = _plan(lib, [128, 1, 127, 1], [64, 64, 1, 128])
  assert n > 0
  clip_off, cap_off, rt, ct = _tiles(plan)
  assert list(rt) == [0, 1, 3, 4] and list(ct) == [0, 2, 3, 4]
  # a 129-clip (or 129-caption) video cannot lie inside one tile
  assert _plan(lib, [3, 129, 2], [3, 4, 2])[0] == ERR_UNSUPPORTED
  assert _plan(lib, [3, 4, 2], [1, 2, 129])[0] == ERR_UNSUPPORTED


def test_plan_argument_errors(lib):
  assert _plan(lib, [2, 3], [2, 3], cap=4 * 2 + 8)[0] == ERR_WORKSPACE
  assert _plan(lib, [2, 0, 3], [2, 1, 3])[0] == ERR_ARG            # a zero count
  assert _plan(lib, [2, 1, 3], [2, -1, 3])[0] == ERR_ARG
  ok = _offsets([1, 2])
  plan = np.zeros(32, dtype=np.int32)
  assert lib.cmhse_group_plan(None, ok.ctypes.data, 2, plan.ctypes.data, 32) == ERR_ARG
  assert lib.cmhse_group_plan(ok.ctypes.data, ok.ctypes.data, 2, None, 32) == ERR_ARG
  assert lib.cmhse_group_plan(ok.ctypes.data, ok.ctypes.data, 0, plan.ctypes.data, 32) == ERR_ARG
  bad = np.array([1, 2, 3], dtype=np.int32)                        # does not start at 0
  assert lib.cmhse_group_plan(bad.ctypes.data, ok.ctypes.data, 2, plan.ctypes.data, 32) == ERR_ARG


def test_plan_max_matches_header():
  from cmhse_amd import _lib
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             'include', 'cmhse_hip.h')).read()
  assert '#define CMHSE_GROUP_PLAN_MAX(B) (4 * (B) + 9)' in header
  assert '#define CMHSE_GROUP_MAX %d' % _lib.GROUP_MAX in header
  assert '#define CMHSE_GROUP_MEAN %d' % _lib.GROUP_MEAN in header
  assert '#define CMHSE_GROUP_TILE_ROWS %d' % _lib.GROUP_TILE_ROWS in header
  assert _lib.group_plan_max(10) == 49


def test_workspace_values(lib):
  ws = lib.cmhse_group_rank_workspace
  assert ws(0) == 0 and ws(-3) == 0
  for B in [1, 63, 64, 65, 300, 4917]:
    t = (B + 63) // 64
    b = ws(B)
    assert b % 256 == 0
    assert b >= B * B * 4 + 2 * t * B * 12
    assert b < B * B * 4 + 2 * t * B * 12 + 5 * 256
  assert ws(4917) < 110 * 1000 * 1000


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_group_scores / cmhse_group_rank is returned before anything is launched."""
  clips, caps = [2, 1, 3], [1, 1, 2]
  n, plan = _plan(lib, clips, caps)
  plan = plan[:n].copy()
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_group_rank_workspace(3)
  good = dict(C=fake, S=fake, Nc=6, Ns=4, D=8, B=3, ph=plan.ctypes.data, pd=fake, plen=n, reduce=1,
              G=fake, ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok)

  def scores(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_scores(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['B'], a['ph'], a['pd'],
                                  a['plen'], a['reduce'], a['G'], None)

  def rank(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_rank(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['B'], a['ph'], a['pd'],
                                a['plen'], a['reduce'], fake, fake, fake, fake, a['ws'], a['ws_bytes'],
                                None)

  bads = [dict(C=None), dict(S=None), dict(ph=None), dict(pd=None), dict(Nc=7), dict(Ns=3),
          dict(Nc=0), dict(D=0), dict(D=-1), dict(B=2), dict(B=0), dict(plen=n - 1), dict(plen=n + 1),
          dict(reduce=2), dict(reduce=-1)]
  for bad in bads + [dict(G=None)]:
    assert scores(**bad) == ERR_ARG, bad
  for bad in bads:
    assert rank(**bad) == ERR_ARG, bad
  assert rank(ws=None) == ERR_ARG
  assert rank(ws=ctypes.c_void_p((1 << 20) + 16)) == ERR_WORKSPACE
  assert rank(ws_bytes=ws_ok - 1) == ERR_WORKSPACE
  # a host plan whose tiles were edited: rejected (the kernels trust its bounds)
  for idx, val in [(HDR, 1), (HDR + 2, 0), (3, 4), (HDR + 2 * 4 + 1, 1)]:
    edited = plan.copy()
    edited[idx] = val
    assert scores(ph=edited.ctypes.data) == ERR_ARG, (idx, val)


def test_ops_argument_errors_raise_value_error():
  from cmhse_amd import ops
  c, s = torch.zeros(6, 4), torch.zeros(4, 4)
  for kw in [dict(num_clips=[2, 0, 4]), dict(num_clips=[2, 1, 2]), dict(num_clips=[2, 1, 3], num_caps=[1, 1]),
             dict(num_clips=[2, 1, 3], num_caps=[1, 1, 1]), dict(num_clips=[2, 1, 3], reduce='sum'),
             dict(num_clips=[]), dict(num_clips=[2, 1.5, 2.5])]:
    args = dict(num_caps=[1, 1, 2], reduce='max')
    args.update(kw)
    for fn in (ops.group_scores, ops.group_rank):
      with pytest.raises(ValueError):
        fn(c, s, **args)
  with pytest.raises(ValueError):
    ops.group_plan([129, 1], [1, 1], 130, 2)
  with pytest.raises(ValueError):
    ops.group_scores(torch.zeros(6, 4), torch.zeros(4, 5), [2, 1, 3], [1, 1, 2])


def test_group_i2t_t2i_argument_errors():
  from cmhse_amd import evaluation
  c, s = np.zeros((6, 4), np.float32), np.zeros((4, 4), np.float32)
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i(c, s, [2, 1, 3], [1, 1, 2], reduce='median')
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i(c, s, [2, 1, 3])                 # num_caps = num_clips: 6 != 4 rows


def numpy_group_scores(scores, num_clips, num_caps, reduce):
  """The contract of G on a stored score matrix: block max, or the block's fp32 scores summed in
  fp64 sequentially in row-major order, / count in fp64, rounded to fp32."""
  scores = np.asarray(scores, dtype=np.float32)
  oc, os_ = _offsets(num_clips), _offsets(num_caps)
  B = len(num_clips)
  G = np.empty((B, B), dtype=np.float32)
  for i in range(B):
    for j in range(B):
      block = scores[oc[i]:oc[i + 1], os_[j]:os_[j + 1]]
      if reduce == 'max':
        G[i, j] = block.max()
      else:
        G[i, j] = np.float32(np.cumsum(block.astype(np.float64).ravel())[-1] / block.size)
  return G


def upstream_group_scores(scores, num_clips, num_caps, max_violation):
  """GroupWiseContrastiveLoss's block loop (loss.py:33-40), in torch on the CPU."""
  scores = torch.as_tensor(scores)
  B = len(num_clips)
  out = torch.zeros(B, B)
  ci = 0
  for i in range(B):
    cj = 0
    for j in range(B):
      block = scores[ci:ci + num_clips[i], cj:cj + num_caps[j]]
      out[i, j] = block.max() if max_violation else block.mean()
      cj += num_caps[j]
    ci += num_clips[i]
  return out.numpy()


@pytest.mark.parametrize('seed,B', [(0, 1), (1, 9), (2, 40)])
def test_numpy_restatement_matches_torch_blocks(seed, B):
  rng = np.random.RandomState(seed)
  nclips = _ragged(rng, B, 9)
  ncaps = _ragged(rng, B, 9)
  scores = rng.standard_normal((nclips.sum(), ncaps.sum())).astype(np.float32)
  assert np.array_equal(numpy_group_scores(scores, nclips, ncaps, 'max'),
                        upstream_group_scores(scores, nclips, ncaps, True))
  mean = numpy_group_scores(scores, nclips, ncaps, 'mean')
  want = upstream_group_scores(scores, nclips, ncaps, False)
  # torch's fp32 mean and the fp64 sum agree to fp32 rounding; both are the block mean
  np.testing.assert_allclose(mean, want, rtol=2e-6, atol=1e-6)
  exact = np.array([[scores[a:b, c:d].astype(np.float64).mean() for c, d in
                     zip(_offsets(ncaps)[:-1], _offsets(ncaps)[1:])]
                    for a, b in zip(_offsets(nclips)[:-1], _offsets(nclips)[1:])])
  np.testing.assert_allclose(mean, exact, rtol=2 ** -23, atol=0)
