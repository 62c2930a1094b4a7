"""The workspace ABI of the training-loss entry points (no GPU needed): every size query returns the
bytes it has always returned (Python keeps a forward workspace as the stored scores of the backward,
so the sizes and the offsets behind them are ABI), and every workspace-taking entry point refuses a
workspace one byte short or off the 256-byte alignment before it touches the device."""
import ctypes

import pytest

from cmhse_amd import _lib

ERR_WORKSPACE = -2

# n: (contrastive_workspace, contrastive_bwd_workspace)
CONTRASTIVE = {1: (512, 1536), 5: (512, 1536), 64: (16640, 33792), 65: (17408, 36352),
               128: (65792, 133120), 513: (1053184, 2115072), 520: (1081856, 2172416)}
# (n_blocks, max_n): (contrastive_blocks_workspace, contrastive_blocks_bwd_workspace)
BLOCKS = {(1, 5): (512, 1536), (3, 65): (51200, 109056), (8, 128): (524544, 1064960),
          (7, 513): (7369984, 14805504)}
# (n, B): (groupwise_workspace, groupwise_bwd_workspace)
GROUPWISE = {(5, 1): (512, 2048), (6, 3): (512, 2048), (452, 33): (817664, 1645056),
             (520, 130): (1081856, 2301952)}


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import build
  build.build()
  return _lib.load()


def test_workspace_sizes_are_the_abi(lib):
  for n, (fwd, bwd) in CONTRASTIVE.items():
    assert lib.cmhse_contrastive_workspace(n) == fwd, n
    assert lib.cmhse_contrastive_bwd_workspace(n) == bwd, n
    # the single loss is the one-block case of the batched layout
    assert lib.cmhse_contrastive_blocks_workspace(1, n) == fwd, n
    assert lib.cmhse_contrastive_blocks_bwd_workspace(1, n) == bwd, n
  for (nb, max_n), (fwd, bwd) in BLOCKS.items():
    assert lib.cmhse_contrastive_blocks_workspace(nb, max_n) == fwd, (nb, max_n)
    assert lib.cmhse_contrastive_blocks_bwd_workspace(nb, max_n) == bwd, (nb, max_n)
  for (n, B), (fwd, bwd) in GROUPWISE.items():
    assert lib.cmhse_groupwise_workspace(n, B) == fwd, (n, B)
    assert lib.cmhse_groupwise_bwd_workspace(n, B) == bwd, (n, B)


def test_workspace_sizes_of_non_positive_arguments_are_zero(lib):
  for bad in (0, -1):
    assert lib.cmhse_contrastive_workspace(bad) == 0
    assert lib.cmhse_contrastive_bwd_workspace(bad) == 0
    for name in ('cmhse_contrastive_blocks_workspace', 'cmhse_contrastive_blocks_bwd_workspace',
                 'cmhse_groupwise_workspace', 'cmhse_groupwise_bwd_workspace'):
      fn = getattr(lib, name)
      assert fn(bad, 5) == 0 and fn(5, bad) == 0 and fn(bad, bad) == 0, name


def _calls(lib, n, B, nb, D=8):
  """(name, bytes needed, call(workspace address, workspace bytes)) of the six entry points; every
  pointer argument is the address of one live dummy buffer that no call gets as far as reading."""
  dummy = ctypes.create_string_buffer(64)
  p = ctypes.addressof(dummy)
  calls = [
      ('cmhse_contrastive_fwd', lib.cmhse_contrastive_workspace(n),
       lambda ws, nbytes: lib.cmhse_contrastive_fwd(p, p, n, D, 0.2, 0, 0, p, None, ws, nbytes, None)),
      ('cmhse_contrastive_bwd', lib.cmhse_contrastive_bwd_workspace(n),
       lambda ws, nbytes: lib.cmhse_contrastive_bwd(p, p, p, n, D, 0.2, 0, 0, p, p, p, ws, nbytes, None)),
      ('cmhse_contrastive_blocks_fwd', lib.cmhse_contrastive_blocks_workspace(nb, n),
       lambda ws, nbytes: lib.cmhse_contrastive_blocks_fwd(p, p, p, nb, n, D, 0.2, 0, 0, p, ws, nbytes, None)),
      ('cmhse_contrastive_blocks_bwd', lib.cmhse_contrastive_blocks_bwd_workspace(nb, n),
       lambda ws, nbytes: lib.cmhse_contrastive_blocks_bwd(p, p, p, p, nb, n, D, 0.2, 0, 0, p, p, p, ws, nbytes,
                                                           None)),
      ('cmhse_groupwise_fwd', lib.cmhse_groupwise_workspace(n, B),
       lambda ws, nbytes: lib.cmhse_groupwise_fwd(p, p, n, D, p, p, B, 0.2, 0, 0, p, p, p, None, ws, nbytes, None)),
      ('cmhse_groupwise_bwd', lib.cmhse_groupwise_bwd_workspace(n, B),
       lambda ws, nbytes: lib.cmhse_groupwise_bwd(p, p, n, D, p, p, B, 0.2, 0, 0, p, p, p, p, p, ws, nbytes, None)),
  ]
  return dummy, calls


@pytest.mark.parametrize('n,B,nb', [(5, 2, 1), (65, 3, 3)])
def test_short_or_misaligned_workspace_is_refused_before_the_device(lib, n, B, nb):
  dummy, calls = _calls(lib, n, B, nb)
  aligned = 1 << 20            # an address only: the check comes before anything reads through it
  for name, need, call in calls:
    assert need > 0 and need % 256 == 0, name
    assert call(aligned, need - 1) == ERR_WORKSPACE, name
    assert call(aligned + 4, need) == ERR_WORKSPACE, name
    assert call(aligned + 4, need + 256) == ERR_WORKSPACE, name     # however large: alignment is required
  del dummy
