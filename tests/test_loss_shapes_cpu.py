"""The loss-shape tables prove what they claim (no GPU needed): every case of tests/loss_shapes.py
has the property its row names, by the constants the sources hold; the dyadic inputs are exact in
fp32; the random inputs keep every hinge clear of its kink, so tests/test_gpu_loss_shapes.py
compares every element of every case; and the oracle the GPU tests trust is itself checked against
float64 autograd at these sizes.  A moved constant fails here instead of quietly moving a case off
its target."""
import numpy as np
import pytest
import torch

import loss_shapes as ls


def test_constants_match_the_sources():
  src = ls.source_constants()
  assert src['kThreads'] == ls.K_THREADS
  assert src['kSimSmallMax'] == ls.SIM_SMALL_MAX
  assert src['loss_blocks'] == '(B + %d) / %d' % (ls.LOSS_BLOCK_ROWS - 1, ls.LOSS_BLOCK_ROWS)
  assert src['vec'] == '(n % 4 == 0) && (D % 4 == 0)'
  assert src['step_loss_max'] == ls.STEP_LOSS_MAX


def test_every_groupwise_case_has_its_property():
  assert set(ls.GW_PROPERTIES) == set(ls.GW_BY_ID)
  for name, B, _, D, _, _ in ls.GW_CASES:
    nc, ncap = ls.gw_counts(name)
    n = sum(nc)
    assert len(nc) == len(ncap) == B and sum(ncap) == n and min(nc + ncap) >= 1, name
    blocks = sorted((r * c for r in nc for c in ncap), reverse=True)
    for key, want in ls.GW_PROPERTIES[name].items():
      got = {'max_block_over': lambda: blocks[0] > want,
             'blocks_over_256': lambda: sum(b > ls.K_THREADS for b in blocks) >= want,
             'max_block': lambda: blocks[0] == want,
             'B_over_64': lambda: (B > ls.LOSS_BLOCK_ROWS) == want,
             'n_range': lambda: want[0] <= n <= want[1],
             'n': lambda: n == want,
             'n_over_512': lambda: (n > ls.SIM_SMALL_MAX) == want,
             'n_mod4': lambda: (n % 4 == 0) == want,
             'D_mod4': lambda: (D % 4 == 0) == want,
             'D': lambda: D == want,
             'unequal': lambda: (nc != ncap and sorted(nc) == sorted(ncap)) == want}[key]()
      assert got, (name, key, want, n, blocks[:3])
  # the rows of the issue's table, literally
  nc, _ = ls.gw_counts('big_blocks')
  assert nc[0] == 27 and nc[1] == 20 and max(nc) == 27 and 27 * 27 == 729 and 27 * 20 == 540
  assert ls.gw_counts('two_videos')[0] == [1, 3] and ls.gw_counts('one_video')[0] == [5]
  assert set(ls.gw_counts('vec_big_tile')[0]) == {4} and set(ls.gw_counts('singletons')[0]) == {1}
  # every case runs in all four modes
  runs = ls.gw_runs()
  for name in ls.GW_BY_ID:
    assert {(mv, nm) for c, mv, nm, _ in runs if c == name} == {(a, b) for a in (0, 1) for b in (0, 1)}
  assert all(kind == 'dyadic' for _, mv, _, kind in runs if mv)
  assert {c for c, mv, _, kind in runs if not mv and kind == 'dyadic'} == {'big_blocks', 'batch128'}


def _tied_blocks(sc, nc, ncap):
  """Blocks whose maximum is reached more than once, and those among them where two of the tied
  elements are a multiple of kThreads apart (two candidates of one thread of the strided scan)."""
  ro = np.concatenate([[0], np.cumsum(nc)])
  co = np.concatenate([[0], np.cumsum(ncap)])
  tied, same_thread = 0, 0
  for i in range(len(nc)):
    for j in range(len(nc)):
      blk = sc[ro[i]:ro[i + 1], co[j]:co[j + 1]]
      e = np.flatnonzero(blk.ravel() == blk.max())
      tied += len(e) > 1
      same_thread += len(set(e % ls.K_THREADS)) < len(e)
  return tied, same_thread


@pytest.mark.parametrize('name', sorted(ls.GW_BY_ID))
def test_dyadic_inputs_are_exact(oracle, name):
  nc, ncap, a, b, margin = ls.gw_dyadic(name)
  sc32 = a @ b.T
  sc64 = a.astype(np.float64) @ b.astype(np.float64).T
  assert sc32.dtype == np.float32 and np.array_equal(sc32.astype(np.float64), sc64)
  # ... in any summation order
  perm = np.random.RandomState(0).permutation(a.shape[1])
  assert np.array_equal(a[:, perm] @ b[:, perm].T, sc32)
  assert np.array_equal((a[:, ::-1].astype(np.float64) @ b[:, ::-1].astype(np.float64).T), sc64)
  for mv in sorted({mv for c, mv, _, kind in ls.gw_runs() if c == name and kind == 'dyadic'}):
    margin = ls.gw_inputs(name, 'dyadic', mv)[4]
    l64, da64, db64 = oracle.groupwise_contrastive_loss(a, b, nc, ncap, margin, mv, True, np.float64, True)
    l32, da32, db32 = oracle.groupwise_contrastive_loss(a, b, nc, ncap, margin, mv, True, np.float32, True)
    big = max(np.abs(da64).max(), np.abs(db64).max())
    assert np.abs(da64 - da32).max() <= 1e-6 * big and np.abs(db64 - db32).max() <= 1e-6 * big, (name, mv)
    assert abs(l64 - l32) <= 1e-6 * max(1e-30, abs(l64))
    if not mv:     # the dyadic mean runs: block means are not dyadic, the hinges must clear fp32 rounding
      red = ls._reduced64(a, b, nc, ncap, False)
      assert ls.hinge_clearance(red, ls.gw_inputs(name, 'dyadic', False)[4], False) >= ls.KINK_CLEARANCE, name
  tied, same_thread = _tied_blocks(sc64, nc, ncap)
  if name in ('big_blocks', 'batch128', 'b65'):
    assert tied >= 1, name
  if name == 'big_blocks':
    # the forced tie: block (0, 0)'s maximum at elements 256 apart, first of them at (2, 3)
    assert same_thread >= 1
    blk = sc64[:nc[0], :ncap[0]]
    e = np.flatnonzero(blk.ravel() == blk.max())
    assert list(e) == [r * ncap[0] + c for r in ls.TIE_ROWS for c in ls.TIE_COLS]
    assert e[-1] - e[0] == ls.K_THREADS


@pytest.mark.parametrize('name', sorted(ls.GW_BY_ID))
def test_random_inputs_clear_every_kink(name):
  nc, ncap, a, b, margin = ls.gw_random(name)
  assert a.dtype == b.dtype == np.float32
  assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1).max() < 1e-6
  red = ls._reduced64(a, b, nc, ncap, False)
  assert np.float32(margin) == margin
  if len(nc) >= 2:
    assert ls.hinge_clearance(red, margin, False) >= ls.KINK_CLEARANCE, name
    assert ls.KINK_CLEARANCE > 2 * ls.REDUCED_ATOL


def _active_share(red, margin):
  return float((margin - ls.kinks_of(red) > 0).mean())


def test_no_case_is_vacuous():
  for name, mv, norm, kind in ls.gw_runs():
    nc, ncap, a, b, margin = ls.gw_inputs(name, kind, mv)
    if len(nc) < 2:
      continue
    share = _active_share(ls._reduced64(a, b, nc, ncap, mv), margin)
    assert share >= 0.05, (name, mv, kind, share)
    if not mv:
      assert share <= 0.95, (name, mv, kind, share)


def _torch_groupwise(a, b, nc, ncap, margin, max_violation, norm):
  """GroupWiseContrastiveLoss restated in float64 torch from its formula: block
  max / mean of the clip x caption scores, then the two hinges of ContrastiveLoss on [B, B]."""
  B = len(nc)
  sc = a @ b.t()
  ro = np.concatenate([[0], np.cumsum(nc)])
  co = np.concatenate([[0], np.cumsum(ncap)])
  rows = []
  for i in range(B):
    blks = [sc[ro[i]:ro[i + 1], co[j]:co[j + 1]] for j in range(B)]
    rows.append(torch.stack([blk.max() if max_violation else blk.mean() for blk in blks]))
  red = torch.stack(rows)
  diag = red.diag().view(B, 1)
  eye = torch.eye(B, dtype=torch.bool)
  cost_s = (margin + red - diag).clamp(min=0).masked_fill(eye, 0)
  cost_im = (margin + red - diag.t()).clamp(min=0).masked_fill(eye, 0)
  if max_violation:
    cost_s, cost_im = cost_s.max(1)[0], cost_im.max(0)[0]
  loss = cost_s.sum() + cost_im.sum()
  return loss / (B * B) if norm else loss


@pytest.mark.parametrize('name,mv,norm', [('b65', False, True), ('unequal', True, False),
                                          ('big_blocks', False, False)])
def test_oracle_groupwise_gradient_vs_autograd(oracle, name, mv, norm):
  """The oracle's backward is pinned to the reference at n = 11 and n = 9 only; here against
  float64 autograd on random (tie-free) inputs at the sizes of the GPU cases."""
  nc, ncap, a, b, margin = ls.gw_random(name)
  ta = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
  tb = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
  loss = _torch_groupwise(ta, tb, nc, ncap, margin, mv, norm)
  loss.backward()
  got, da, db = oracle.groupwise_contrastive_loss(a, b, nc, ncap, margin, mv, norm, np.float64, True)
  assert loss.item() > 0
  assert abs(loss.item() - got) <= 1e-12 * abs(got)
  for g, w in ((ta.grad.numpy(), da), (tb.grad.numpy(), db)):
    assert np.abs(w).max() > 0
    assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max(), name


def test_singletons_oracle_equals_contrastive(oracle):
  for kind in ('dyadic', 'random'):
    for mv in (False, True):
      nc, ncap, a, b, margin = ls.gw_inputs('singletons', kind, mv)
      got = oracle.groupwise_contrastive_loss(a, b, nc, ncap, margin, mv, True, np.float64)
      assert got == oracle.contrastive_loss(a, b, margin, mv, True, np.float64)


def test_elementwise_tables():
  rows = {r for r, _ in ls.EUCLID_SHAPES}
  cols = {c for _, c in ls.EUCLID_SHAPES}
  assert rows == {1, 255, 256, 257, 1000} and cols == {1, 3, 256, 257, 2048}
  assert len(ls.EUCLID_SHAPES) == 19
  for r, c in [(1, 1), (1, 2048), (1000, 1), (1000, 2048), (255, 3), (256, 256), (257, 257), (257, 2048)]:
    assert (r, c) in ls.EUCLID_SHAPES
  assert {c for _, c in ls.NORMALIZE_SHAPES} >= {ls.K_THREADS - 1, ls.K_THREADS, ls.K_THREADS + 1}
  for r, c in ls.NORMALIZE_SHAPES:
    x, g = ls.normalize_inputs(r, c)
    if r >= 2:
      assert not x[0].any()
      nrm = np.linalg.norm(x[1].astype(np.float64))
      assert 0.5e-20 < nrm < 2e-20 and x[1].any()
      assert (np.linalg.norm(x[2:].astype(np.float64), axis=1) > 1e-3).all()


@pytest.mark.parametrize('shape', ls.NORMALIZE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_oracle_normalize_backward_vs_autograd(oracle, shape):
  """oracle.l2_normalize_backward against float64 torch.nn.functional.normalize autograd, row by
  row (a clamped row's gradient is 1e12 times the others'), the zero and the 1e-20 row included."""
  x, g = ls.normalize_inputs(*shape)
  tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
  y = torch.nn.functional.normalize(tx)
  y.backward(torch.from_numpy(g.astype(np.float64)))
  np.testing.assert_allclose(oracle.l2_normalize(x, np.float64), y.detach().numpy(), rtol=1e-14, atol=0)
  want, got = tx.grad.numpy(), oracle.l2_normalize_backward(x, g)
  assert np.isfinite(want).all()
  for r in range(shape[0]):
    assert np.abs(got[r] - want[r]).max() <= 1e-12 * np.abs(want[r]).max(), (shape, r)


def test_step_cases(oracle):
  for name, rows, D, terms, norm, seed, _ in ls.STEP_CASES:
    raw, margin = ls.step_inputs(name)
    assert [x.shape for x in raw] == [(n, D) for n in rows]
    assert all(rows[a] == rows[b] for a, b, _ in terms)
    scores = ls.step_scores64(raw, terms)
    for mv in (False, True):
      for k, s in enumerate(scores):
        assert ls.hinge_clearance(s, margin, mv) >= ls.KINK_CLEARANCE, (name, mv, k)
    for k, s in enumerate(scores):      # every term of more than one row has active and inactive hinges
      if len(s) > 1:
        assert 0.002 <= _active_share(s, margin) <= 0.95, (name, k, _active_share(s, margin))
  name, rows, D, terms, norm, _, _ = ls.STEP_CASES[0]
  assert len(rows) == len(terms) == ls.STEP_LOSS_MAX and D % 4 != 0 and not norm and 1 in rows
  assert {(0, 1), (2, 3), (4, 5), (6, 7), (0, 0), (4, 4)} <= {(a, b) for a, b, _ in terms}
  name, rows, D, terms, norm, _, _ = ls.STEP_CASES[1]
  assert max(rows) > ls.SIM_SMALL_MAX and min(rows) == 1 and rows == (520, 520, 1, 1) and D == 64
  assert [(a, b) for a, b, _ in terms] == [(0, 1), (2, 3), (0, 0)]
