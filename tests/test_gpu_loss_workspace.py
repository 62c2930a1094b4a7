"""Every workspace-taking loss entry point stays inside the workspace it asks for.

Each call goes through _lib with its workspace at bytes [256, 256 + need) of one uint8 tensor of
need + 512 bytes pre-filled with 0xA5: afterwards the 256 bytes on either side are untouched (the
guards lie inside a live allocation, so an overrun is seen, not faulted on), and every output is
torch.equal to what the ops.* wrapper returns for the same inputs.  The shapes are the smallest that
reach every carved region and both sides of the 64-row loss block."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
MARGIN = 0.2


class Guarded(object):
  """`need` workspace bytes between two guards of one allocation."""

  def __init__(self, need, dev):
    assert need > 0
    self.need = need
    self.buf = torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert self.buf.data_ptr() % 256 == 0
    self.ptr = self.buf.data_ptr() + GUARD

  def check(self, where):
    torch.cuda.synchronize()
    assert bool((self.buf[:GUARD] == FILL).all()), where + ': wrote in front of its workspace'
    assert bool((self.buf[GUARD + self.need:] == FILL).all()), where + ': wrote past its workspace'


def _rows(n, D, seed, dev):
  g = torch.Generator(device='cpu').manual_seed(seed)
  return torch.nn.functional.normalize(torch.randn(n, D, generator=g)).to(dev)


def _check(rc, name):
  from cmhse_amd import _lib
  _lib.check(rc, name)


@pytest.mark.parametrize('max_violation', [0, 1])
def test_contrastive_stays_inside_its_workspace(dev, max_violation):
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  n, D = 65, 30
  im, s = _rows(n, D, 1, dev), _rows(n, D, 2, dev)
  gout = torch.full((1,), 0.5, device=dev)
  want_loss, want_scores = ops.contrastive_fwd(im, s, MARGIN, max_violation, 1, want_scores=True)
  want_dim, want_ds = ops.contrastive_bwd(im, s, want_scores, MARGIN, max_violation, 1, gout)

  loss = torch.empty((), device=dev)
  fwd = Guarded(lib.cmhse_contrastive_workspace(n), dev)
  _check(lib.cmhse_contrastive_fwd(im.data_ptr(), s.data_ptr(), n, D, MARGIN, max_violation, 1, loss.data_ptr(),
                                   None, fwd.ptr, fwd.need, ops._stream()), 'cmhse_contrastive_fwd')
  fwd.check('cmhse_contrastive_fwd')
  assert torch.equal(loss, want_loss)
  # without scores_out the stored scores are the head of the workspace
  scores = fwd.buf[GUARD:GUARD + n * n * 4].view(torch.float32).view(n, n)
  assert torch.equal(scores, want_scores)

  d_im, d_s = torch.empty_like(im), torch.empty_like(s)
  bwd = Guarded(lib.cmhse_contrastive_bwd_workspace(n), dev)
  _check(lib.cmhse_contrastive_bwd(im.data_ptr(), s.data_ptr(), scores.data_ptr(), n, D, MARGIN, max_violation, 1,
                                   gout.data_ptr(), d_im.data_ptr(), d_s.data_ptr(), bwd.ptr, bwd.need,
                                   ops._stream()), 'cmhse_contrastive_bwd')
  bwd.check('cmhse_contrastive_bwd')
  fwd.check('cmhse_contrastive_bwd (the stored scores)')
  assert torch.equal(d_im, want_dim) and torch.equal(d_s, want_ds)
  assert float(want_loss) > 0 and float(want_dim.abs().max()) > 0


@pytest.mark.parametrize('max_violation', [0, 1])
def test_contrastive_blocks_stay_inside_their_workspace(dev, max_violation):
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  sizes, D = (5, 64, 65), 30
  nb, max_n, R = len(sizes), max(sizes), sum(sizes)
  im, s = _rows(R, D, 3, dev), _rows(R, D, 4, dev)
  gout = torch.tensor([1.0, 0.5, 2.0], device=dev)
  want_losses, st = ops.contrastive_blocks_fwd(im, s, sizes, MARGIN, max_violation, 0, keep=True)
  want_dim, want_ds = ops.contrastive_blocks_bwd(im, s, st, MARGIN, max_violation, 0, gout)

  off = ops.upload(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
  losses = torch.empty(nb, device=dev)
  fwd = Guarded(lib.cmhse_contrastive_blocks_workspace(nb, max_n), dev)
  _check(lib.cmhse_contrastive_blocks_fwd(im.data_ptr(), s.data_ptr(), off.data_ptr(), nb, max_n, D, MARGIN,
                                          max_violation, 0, losses.data_ptr(), fwd.ptr, fwd.need, ops._stream()),
         'cmhse_contrastive_blocks_fwd')
  fwd.check('cmhse_contrastive_blocks_fwd')
  assert torch.equal(losses, want_losses)
  # block b's scores sit at scores + b * max_n * max_n, unaligned between blocks, leading dimension = its n
  for b, nblk in enumerate(sizes):
    lo = b * max_n * max_n * 4
    got = fwd.buf[GUARD + lo:GUARD + lo + nblk * nblk * 4].view(torch.float32)
    assert torch.equal(got, st['scores'][lo:lo + nblk * nblk * 4].view(torch.float32)), b

  d_im, d_s = torch.empty_like(im), torch.empty_like(s)
  bwd = Guarded(lib.cmhse_contrastive_blocks_bwd_workspace(nb, max_n), dev)
  _check(lib.cmhse_contrastive_blocks_bwd(im.data_ptr(), s.data_ptr(), fwd.ptr, off.data_ptr(), nb, max_n, D,
                                          MARGIN, max_violation, 0, gout.data_ptr(), d_im.data_ptr(),
                                          d_s.data_ptr(), bwd.ptr, bwd.need, ops._stream()),
         'cmhse_contrastive_blocks_bwd')
  bwd.check('cmhse_contrastive_blocks_bwd')
  fwd.check('cmhse_contrastive_blocks_bwd (the stored scores)')
  assert torch.equal(d_im, want_dim) and torch.equal(d_s, want_ds)
  assert float(want_losses.min()) > 0 and float(want_dim.abs().max()) > 0


@pytest.mark.parametrize('max_violation', [0, 1])
def test_groupwise_stays_inside_its_workspace(dev, max_violation):
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  num_clips, num_caps, D = (1, 3, 2), (2, 1, 3), 8
  n, B = sum(num_clips), len(num_clips)
  im, s = _rows(n, D, 5, dev), _rows(n, D, 6, dev)
  gout = torch.full((1,), 0.5, device=dev)
  want_loss, st = ops.groupwise_fwd(im, s, num_clips, num_caps, MARGIN, max_violation, 1)
  want_dim, want_ds = ops.groupwise_bwd(im, s, st, MARGIN, max_violation, 1, gout)

  off = ops.upload(np.concatenate([[0], np.cumsum(num_clips), [0], np.cumsum(num_caps)]).astype(np.int32), dev)
  row_off, col_off = off.data_ptr(), off.data_ptr() + 4 * (B + 1)
  loss = torch.empty((), device=dev)
  reduced = torch.empty(B, B, device=dev)
  arg = torch.empty(B, B, dtype=torch.int32, device=dev)
  fwd = Guarded(lib.cmhse_groupwise_workspace(n, B), dev)
  _check(lib.cmhse_groupwise_fwd(im.data_ptr(), s.data_ptr(), n, D, row_off, col_off, B, MARGIN, max_violation, 1,
                                 loss.data_ptr(), reduced.data_ptr(), arg.data_ptr(), None, fwd.ptr, fwd.need,
                                 ops._stream()), 'cmhse_groupwise_fwd')
  fwd.check('cmhse_groupwise_fwd')
  assert torch.equal(loss, want_loss) and torch.equal(reduced, st['reduced']) and torch.equal(arg, st['arg'])

  d_im, d_s = torch.empty_like(im), torch.empty_like(s)
  bwd = Guarded(lib.cmhse_groupwise_bwd_workspace(n, B), dev)
  _check(lib.cmhse_groupwise_bwd(im.data_ptr(), s.data_ptr(), n, D, row_off, col_off, B, MARGIN, max_violation, 1,
                                 reduced.data_ptr(), arg.data_ptr(), gout.data_ptr(), d_im.data_ptr(),
                                 d_s.data_ptr(), bwd.ptr, bwd.need, ops._stream()), 'cmhse_groupwise_bwd')
  bwd.check('cmhse_groupwise_bwd')
  assert torch.equal(d_im, want_dim) and torch.equal(d_s, want_ds)
  assert float(want_loss) > 0 and float(want_dim.abs().max()) > 0


@pytest.mark.parametrize('max_violation', [0, 1])
def test_step_losses_stay_inside_their_workspace(dev, max_violation):
  from cmhse_amd import _lib, ops
  lib = _lib.load()
  rows, D = (5, 5, 7, 7), 12
  terms = [(0, 1, 1.0), (2, 3, 0.5), (1, 0, 2.0)]
  g = torch.Generator(device='cpu').manual_seed(7)
  xs = [torch.randn(r, D, generator=g).to(dev) for r in rows]       # un-normalised: the call normalises
  gtot = torch.full((1,), 0.5, device=dev)
  want_values, want_total, st = ops.step_losses_fwd(xs, terms, MARGIN, max_violation, 0)
  want_dxs = ops.step_losses_bwd(st, gtot)

  d = _lib.StepLosses()
  d.n_emb, d.n_terms, d.D = len(xs), len(terms), D
  for e, x in enumerate(xs):
    d.x[e], d.rows[e] = x.data_ptr(), rows[e]
  for k, (a, b, w) in enumerate(terms):
    d.term_a[k], d.term_b[k], d.weight[k] = a, b, w
  d.margin, d.max_violation, d.norm = MARGIN, max_violation, 0
  need = lib.cmhse_step_losses_workspace(ctypes.byref(d))
  assert need == st['ws_bytes']
  ws = Guarded(need, dev)
  out = torch.empty(len(terms) + 1, device=dev)
  _check(lib.cmhse_step_losses_fwd(ctypes.byref(d), out.data_ptr(), out.data_ptr() + 4 * len(terms), ws.ptr, need,
                                   ops._stream()), 'cmhse_step_losses_fwd')
  ws.check('cmhse_step_losses_fwd')
  assert torch.equal(out[:len(terms)], want_values) and torch.equal(out[len(terms):], want_total)

  dxs = [torch.empty_like(x) for x in xs]
  ptrs = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in dxs])
  _check(lib.cmhse_step_losses_bwd(ctypes.byref(d), gtot.data_ptr(), ptrs, ws.ptr, need, ops._stream()),
         'cmhse_step_losses_bwd')
  ws.check('cmhse_step_losses_bwd')
  for got, want in zip(dxs, want_dxs):
    assert torch.equal(got, want)
  assert float(want_values.min()) > 0 and all(float(w.abs().max()) > 0 for w in want_dxs)
