"""The loss kernels at training shapes against the float64 oracle.

GroupWiseContrastiveLoss (cmhse_groupwise_fwd / _bwd: block_reduce_kernel, contrastive_partial_kernel
and loss_bwd_stats_kernel on the reduced [B, B] matrix, groupwise_expand_kernel, the two TN GEMMs),
EuclideanLoss, F.normalize and the step's fused contrastive terms, at the sizes where their loops
take a second trip, their tiles change and their GEMMs change form: tests/loss_shapes.py holds the
cases, tests/test_loss_shapes_cpu.py proves each has the property it is there for.  max_violation
runs use dyadic inputs, exact in fp32 in any summation order, so `reduced` and the block arg-max
(tied blocks included) are compared for equality; the mean runs use inputs whose hinges all clear
their kinks by 1e-5, so no element is masked.

With CMHSE_LOSS_SHAPES_REPORT=<file> the largest observed |got - want| / tolerance of every
comparison family is written there (profiles/loss_shapes_errors.txt)."""
import os

import numpy as np
import pytest
import torch

from gpu_common import grad_close, loss_close

import loss_shapes as ls

pytestmark = pytest.mark.gpu

_WORST = {}    # family -> (ratio, err, tol, where)


def _note(family, err, tol, where):
  if family not in _WORST or err / tol > _WORST[family][0]:
    _WORST[family] = (err / tol, err, tol, where)


@pytest.fixture(scope='module', autouse=True)
def _report():
  yield
  path = os.environ.get('CMHSE_LOSS_SHAPES_REPORT')
  if path and _WORST:
    with open(path, 'w') as f:
      f.write('# largest |got - want| / tolerance per comparison family (tests/test_gpu_loss_shapes.py)\n')
      f.write('# %-28s %10s %12s %12s  %s\n' % ('family', 'err / tol', 'err', 'tol', 'worst case'))
      for fam in sorted(_WORST):
        f.write('%-30s %10.4f %12.3e %12.3e  %s\n' % ((fam,) + _WORST[fam]))


def _grad_close(got, want, where, family):
  """gpu_common.grad_close, its error recorded first."""
  want = np.asarray(want, dtype=np.float64)
  got = np.asarray(got, dtype=np.float64)
  if got.shape == want.shape:
    _note(family, np.abs(got - want).max(), 2e-4 * max(1e-30, np.abs(want).max()) + 2e-6, where)
  grad_close(got, want, where)


def _loss_close(got, want, where, family):
  _note(family, abs(float(got) - float(want)), 1e-4 * max(1.0, abs(float(want))), where)
  assert loss_close(got, want), (where, float(got), float(want))


def _dev(x, dev):
  return torch.from_numpy(np.array(x)).to(dev)      # (a copy: the builders' arrays are read-only)


# ------------------------------------------------------------------------------------------------
# GroupWiseContrastiveLoss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', ls.gw_runs(), ids=[ls.run_id(r) for r in ls.gw_runs()])
def test_groupwise_shape_vs_oracle(dev, oracle, run):
  """cmhse_groupwise_fwd / _bwd of one (case, max_violation, norm): the saved `reduced` matrix and
  block arg-max, the loss and both gradients against the float64 oracle."""
  from cmhse_amd import ops
  from cmhse_amd.loss import ContrastiveLoss
  name, mv, norm, kind = run
  where = ls.run_id(run)
  nc, ncap, a, b, margin = ls.gw_inputs(name, kind, mv)
  n, B = len(a), len(nc)
  ta, tb = _dev(a, dev), _dev(b, dev)
  loss, st = ops.groupwise_fwd(ta, tb, nc, ncap, margin, mv, norm)
  gout = torch.ones((), device=dev)
  d_im, d_s = ops.groupwise_bwd(ta, tb, st, margin, mv, norm, gout)
  torch.cuda.synchronize()

  sc64 = a.astype(np.float64) @ b.astype(np.float64).T
  red64, arg64 = oracle.groupwise_reduce(sc64, nc, ncap, mv)
  want, da, db = oracle.groupwise_contrastive_loss(a, b, nc, ncap, margin, mv, norm, np.float64, True)
  red = st['reduced'].cpu().numpy()
  assert red.shape == (B, B)
  _note('reduced (atol 2e-6)', np.abs(red - red64).max(), ls.REDUCED_ATOL, where)
  if kind == 'dyadic' and mv:
    assert np.array_equal(red.astype(np.float64), red64), where
    # first maximum in row-major order, for every block, the tied ones included
    np.testing.assert_array_equal(st['arg'].cpu().numpy().astype(np.int64),
                                  arg64[:, :, 0] * n + arg64[:, :, 1], err_msg=where)
  else:
    np.testing.assert_allclose(red, red64, atol=ls.REDUCED_ATOL, rtol=0, err_msg=where)
  _loss_close(loss.item(), want, where, 'groupwise loss')
  _grad_close(d_im.cpu().numpy(), da, where + ' d_im', 'groupwise d_im')
  _grad_close(d_s.cpu().numpy(), db, where + ' d_s', 'groupwise d_s')

  if name == 'one_video':
    assert want == 0.0 and loss.item() == 0.0
    assert not d_im.cpu().numpy().any() and not d_s.cpu().numpy().any()
  if name == 'singletons':
    x = ta.clone().requires_grad_(True)
    y = tb.clone().requires_grad_(True)
    plain = ContrastiveLoss(margin=margin, measure='cosine', max_violation=mv, norm=norm)(x, y)
    plain.backward()
    assert plain.item() == loss.item(), (where, plain.item(), loss.item())
    assert loss_close(plain.item(), oracle.contrastive_loss(a, b, margin, mv, norm, np.float64))
    _grad_close(d_im.cpu().numpy(), x.grad.cpu().numpy(), where + ' d_im vs ContrastiveLoss', 'groupwise d_im')
    _grad_close(d_s.cpu().numpy(), y.grad.cpu().numpy(), where + ' d_s vs ContrastiveLoss', 'groupwise d_s')


def test_groupwise_module_with_normalize(dev, oracle):
  """GroupWiseContrastiveLoss on normalize() of un-normalised rows with unequal clip and caption
  counts and a non-unit upstream gradient: value and gradients wrt the raw rows against the
  float64 oracle."""
  from cmhse_amd.loss import GroupWiseContrastiveLoss, normalize
  nc, ncap, a, b, margin = ls.gw_inputs('unequal', 'random', False)
  rng = np.random.RandomState(len(a))
  # power-of-two row scales: normalize() gives the builder's rows back to rounding, which the
  # hinges of these inputs clear
  xa = (a * 2.0 ** rng.randint(-2, 3, size=(len(a), 1))).astype(np.float32)
  xb = (b * 2.0 ** rng.randint(-2, 3, size=(len(b), 1))).astype(np.float32)
  crit = GroupWiseContrastiveLoss(margin=margin, measure='cosine', max_violation=False, norm=True)
  ta, tb = _dev(xa, dev).requires_grad_(True), _dev(xb, dev).requires_grad_(True)
  loss = crit(normalize(ta), normalize(tb), nc, ncap)
  (loss * 1.5).backward()
  ya, yb = oracle.l2_normalize(xa, np.float64), oracle.l2_normalize(xb, np.float64)
  want, da, db = oracle.groupwise_contrastive_loss(ya, yb, nc, ncap, margin, False, True, np.float64, True)
  _loss_close(loss.item(), want, 'unequal module', 'groupwise loss')
  _grad_close(ta.grad.cpu().numpy(), 1.5 * oracle.l2_normalize_backward(xa, da), 'unequal module da',
              'groupwise module d rows')
  _grad_close(tb.grad.cpu().numpy(), 1.5 * oracle.l2_normalize_backward(xb, db), 'unequal module db',
              'groupwise module d rows')


# ------------------------------------------------------------------------------------------------
# EuclideanLoss
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('shape', ls.EUCLID_SHAPES, ids=lambda s: '%dx%d' % s)
def test_euclid_shape_vs_oracle(dev, oracle, shape, norm):
  """euclid_rows_kernel / euclid_final_kernel: value and gradient against the float64 oracle, the
  target given contiguous and by row address into a larger tensor; the two forms agree bitwise."""
  from cmhse_amd.decoder import EuclideanLoss
  rows, cols = shape
  a_np, pool_np, idx = ls.euclid_inputs(rows, cols)
  b_np = pool_np[idx]
  where = 'euclid %dx%d norm%d' % (rows, cols, norm)
  crit = EuclideanLoss(norm=norm)
  a1 = _dev(a_np, dev).requires_grad_(True)
  l1 = crit(a1, _dev(b_np, dev))
  (l1 * 3.0).backward()
  a2 = _dev(a_np, dev).requires_grad_(True)
  pool = _dev(pool_np, dev)
  addrs = np.uint64(pool.data_ptr()) + idx.astype(np.uint64) * np.uint64(cols * 4)
  l2 = crit.forward_rows(a2, addrs, pool)
  (l2 * 3.0).backward()
  torch.cuda.synchronize()
  assert torch.equal(l1, l2) and torch.equal(a1.grad, a2.grad), where
  _loss_close(l1.item(), oracle.euclidean_loss(a_np, b_np, norm, np.float64), where, 'euclid loss')
  _grad_close(a1.grad.cpu().numpy(), 3.0 * oracle.euclidean_loss_backward(a_np, b_np, norm, np.float64),
              where, 'euclid d_a')


# ------------------------------------------------------------------------------------------------
# F.normalize
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ls.NORMALIZE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_normalize_shape_vs_oracle(dev, oracle, shape):
  """l2norm_rows_kernel / l2norm_bwd_kernel with a zero row and a row below the 1e-12 clamp:
  forward to 1e-6 (the zero row exactly zero), backward row by row — a clamped row's gradient is
  1e12 times the others'."""
  from cmhse_amd.loss import normalize
  rows, cols = shape
  x_np, g_np = ls.normalize_inputs(rows, cols)
  x = _dev(x_np, dev).requires_grad_(True)
  y = normalize(x)
  y.backward(_dev(g_np, dev))
  torch.cuda.synchronize()
  got = y.detach().cpu().numpy()
  want = oracle.l2_normalize(x_np, np.float64)
  where = 'normalize %dx%d' % shape
  _note('normalize fwd (atol 1e-6)', np.abs(got - want).max(), 1e-6, where)
  np.testing.assert_allclose(got, want, atol=1e-6, rtol=0, err_msg=where)
  if rows >= 2:
    assert not got[0].any()
  dx = x.grad.cpu().numpy()
  want_dx = oracle.l2_normalize_backward(x_np, g_np)
  assert np.isfinite(dx).all()
  for r in range(rows):
    _grad_close(dx[r], want_dx[r], '%s row %d' % (where, r), 'normalize bwd (per row)')


# ------------------------------------------------------------------------------------------------
# the step's fused contrastive terms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_violation', [False, True], ids=['sum', 'max'])
@pytest.mark.parametrize('case', ls.STEP_CASES, ids=[c[0] for c in ls.STEP_CASES])
def test_step_losses_shape(dev, oracle, case, max_violation):
  """loss.step_losses (cmhse_step_losses_fwd / _bwd over cmhse_contrastive_blocks_*) against
  normalize() + criterion(a, b) term by term — values bit for bit, total and gradients to fp32
  rounding — and against the float64 oracle, at the tolerances of
  test_step_losses_node_equals_normalize_plus_criterion."""
  from cmhse_amd.loss import ContrastiveLoss, normalize, step_losses
  name, rows, D, terms, norm, _, _ = case
  raw_np, margin = ls.step_inputs(name)
  where = '%s mv%d' % (name, max_violation)
  crit = ContrastiveLoss(margin=margin, max_violation=max_violation, norm=norm)
  raw = [_dev(x, dev) for x in raw_np]
  sep = [x.clone().requires_grad_(True) for x in raw]
  ns = [normalize(x) for x in sep]
  sep_vals = torch.stack([crit(ns[a], ns[b]) for a, b, _ in terms])
  sep_total = sum(w * sep_vals[k] for k, (_, _, w) in enumerate(terms))
  (sep_total * 1.5).backward()
  fus = [x.clone().requires_grad_(True) for x in raw]
  total, vals = step_losses(crit, fus, terms)
  (total * 1.5).backward()
  torch.cuda.synchronize()
  assert torch.equal(vals, sep_vals), (where, vals, sep_vals)
  tol = 1e-6 * max(1.0, abs(sep_total.item()))
  _note('step total vs separate', abs(total.item() - sep_total.item()), tol, where)
  assert abs(total.item() - sep_total.item()) <= tol
  for e in range(len(rows)):
    g, r = fus[e].grad, sep[e].grad
    tol = 2e-6 * max(1e-3, float(r.abs().max()))
    _note('step grads vs separate', float((g - r).abs().max()), tol, '%s emb %d' % (where, e))
    assert float((g - r).abs().max()) <= tol, (where, e)
  host = [x.astype(np.float64) for x in raw_np]
  y = [oracle.l2_normalize(x, dtype=np.float64) for x in host]
  gy = [np.zeros_like(x) for x in host]
  live = 0
  for k, (a, b, w) in enumerate(terms):
    want = oracle.contrastive_loss(y[a], y[b], margin=margin, max_violation=max_violation, norm=norm,
                                   dtype=np.float64)
    tol = 2e-5 * max(1.0, abs(float(want)))
    _note('step values vs oracle', abs(float(vals[k]) - float(want)), tol, '%s term %d' % (where, k))
    assert abs(float(vals[k]) - float(want)) <= tol, (where, k, float(vals[k]), float(want))
    live += float(want) > 0
    d_im, d_s = oracle.contrastive_loss_backward(y[a], y[b], margin=margin, max_violation=max_violation,
                                                 norm=norm)
    gy[a] += 1.5 * w * d_im
    gy[b] += 1.5 * w * d_s
  assert live == sum(1 for a, _, _ in terms if rows[a] > 1), where      # every term of > 1 row bites
  for e in range(len(rows)):
    want = oracle.l2_normalize_backward(host[e], gy[e])
    got = fus[e].grad.cpu().numpy()
    tol = 2e-5 * max(1e-3, np.abs(want).max())
    _note('step grads vs oracle', np.abs(got - want).max(), tol, '%s emb %d' % (where, e))
    assert np.abs(got - want).max() <= tol, (where, e, np.abs(got - want).max(), tol)
