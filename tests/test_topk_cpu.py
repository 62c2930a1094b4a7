"""cmhse_sim_topk without a GPU: workspace size and argument validation (include/cmhse_hip.h)."""
import ctypes

import pytest

MATRIX_4917 = 4917 * 4917 * 4


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def test_topk_max_matches_header():
  import os
  from cmhse_amd import _lib
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             'include', 'cmhse_hip.h')).read()
  assert '#define CMHSE_TOPK_MAX %d' % _lib.TOPK_MAX in header


def test_workspace_values(lib):
  ws = lib.cmhse_sim_topk_workspace
  # K keys of 8 bytes per row and column panel, 256-byte aligned
  for nrows, m, k in [(1, 1, 1), (129, 300, 5), (4917, 4917, 50), (256, 200000, 100), (64, 1000, 128)]:
    b = ws(nrows, m, k)
    assert b > 0 and b % 256 == 0
    assert b >= nrows * k * 8
  # one column tile: one panel
  assert ws(1, 1, 1) == 256
  assert ws(64, 128, 128) == 64 * 128 * 8
  # degenerate sizes have no workspace
  assert ws(0, 10, 1) == 0
  assert ws(10, 0, 1) == 0
  assert ws(10, 10, 0) == 0
  assert ws(10, 1000, 129) == 0


def test_workspace_bounds(lib):
  ws = lib.cmhse_sim_topk_workspace
  assert ws(4917, 4917, 50) < MATRIX_4917
  assert ws(4917, 1000000, 100) < (1 << 30)
  # the panel count is capped: the workspace stops growing with the gallery
  assert ws(4917, 1000000, 100) == ws(4917, 10000000, 100)
  assert ws(256, 200000, 10) == ws(256, 2000000, 10)


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_sim_topk is returned before anything touches the device."""
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_sim_topk_workspace(4, 10, 3)
  good = dict(A=fake, B=fake, N=4, M=10, D=8, row0=0, nrows=4, K=3, scores=fake, index=fake,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok, stream=None)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_sim_topk(a['A'], a['B'], a['N'], a['M'], a['D'], a['row0'], a['nrows'],
                              a['K'], a['scores'], a['index'], a['ws'], a['ws_bytes'], a['stream'])

  for bad in [dict(A=None), dict(B=None), dict(scores=None), dict(index=None), dict(ws=None),
              dict(K=0), dict(K=-1), dict(K=11), dict(M=200, K=129), dict(row0=-1),
              dict(nrows=-1), dict(row0=3, nrows=2), dict(row0=4, nrows=1), dict(N=0), dict(M=0),
              dict(D=0), dict(N=-4), dict(D=-1)]:
    assert call(**bad) == -1, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16)) == -2     # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == -2                     # too small
  assert call(ws_bytes=0) == -2
  # an empty stripe is a no-op that succeeds (nothing launched, no buffers needed)
  assert call(nrows=0, scores=None, index=None, ws=None, ws_bytes=0) == 0
  assert call(row0=4, nrows=0, scores=None, index=None, ws=None, ws_bytes=0) == 0


def test_sim_topk_needs_device_tensors():
  import torch
  from cmhse_amd import ops
  with pytest.raises(RuntimeError):
    ops.sim_topk(torch.zeros(2, 4), torch.zeros(3, 4), 1)
