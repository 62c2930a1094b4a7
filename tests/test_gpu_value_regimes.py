"""Gate, softmax and normalisation math at extreme values against the float64 oracle.

The shape suites (test_gpu_fwd_shapes.py, test_gpu_bf3_shapes.py, test_gpu_bptt_shapes.py) settle which
kernel runs; all their cases draw the same numbers.  Here the cases of tests/value_regimes.py run the
same shapes under value regimes — saturated gates, update gates of exactly 1, reset gates of exactly 0
(through exp -> inf -> rcp = 0), inputs and states of 1e-2 .. 1e-4, a peaked and a starved attention
softmax — each regime proved to be what it says by tests/test_value_regimes_cpu.py.  Every case runs
twice (same bits), then goes against the oracle at bars scaled from the oracle's own fp32 error
(value_regimes.py's docstring, with the measured table).  The row kernels of F.normalize and the losses
built on them run at the 1e-12 clamp against float64 torch autograd.

Two findings these tests were written for, both fixed with them:
  * tanhf_ = 1 - 2 rcp(exp(2x) + 1) cancels for small |x| (absolute error ~1e-7, relative ~1e-7 / |x|); the
    model L2-normalises every encoder output, which turns that into the error of the embedding.  The
    normalised assertion of test_value_regime_vs_oracle fails on every small_1e-3 and small_1e-4 case without
    the polynomial branch of tanhf_ (gru_step_tile.hpp): 3e-5 and 3e-4 from the oracle, 3e-6 at small_1e-2
    (under the bar), against 1e-7 with it.
  * l2norm_bwd_row kept the projection term inside the clamp, where torch's clamp_min passes no gradient
    to the norm: test_l2norm_rows_bwd_at_the_clamp and test_step_losses_at_the_clamp fail on the sub-eps
    rows without the fix (norm_rows.hpp).
The saved update gate of a `frozen` unit is exactly 1.0f (v_rcp_f32(1.0f) == 1.0f, measured here), so the
frozen units are compared bit for bit."""

import numpy as np
import pytest
import torch

from conftest import GOLDEN_TOL, assert_emb_close
from gpu_common import _RecordForward, _blas_threads, grad_close

import fwd_shapes
import value_regimes as vr
from test_gpu_bf3_shapes import BF3_TOL, packed
from test_gpu_fwd_shapes import _backward, _run_inference, _run_training

pytestmark = pytest.mark.gpu

_EXACT = [c for c in vr.CASES if c[1] != 'bf3']
_BF3 = [c for c in vr.CASES if c[1] == 'bf3']
ROUTE_GAP = 1e-5      # a pair routed away from the float64 arg-max is a near-tie (gpu_common._check_train_step_vs_oracle)


def _dist(a, b):
  return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def _held(h0, lens, H):
  return np.zeros((len(lens), H), dtype=np.float32) if h0 is None else h0


def _check_frozen_outputs(j, got, h0, lens, tag):
  """On the frozen units h_t == h0 at every step: LAST and MAX give h0 back bit for bit, POOL_ALL writes it
  at every step."""
  u = vr.marked_units(j['H'])
  held = _held(h0, lens, j['H'])[:, u]
  if j['pool'] in ('LAST', 'MAX'):
    assert np.array_equal(got[:, u], held), tag + ': a frozen unit moved'
  elif j['pool'] == 'ALL':
    assert np.array_equal(got[:, u], np.repeat(held, lens, axis=0)), tag + ': a frozen unit moved'


@pytest.mark.parametrize('case', _EXACT, ids=[c[0] for c in _EXACT])
def test_value_regime_vs_oracle(dev, oracle, tune, monkeypatch, case):
  from cmhse_amd import ops
  cid, source, name, regime, _ = case
  knobs, train, tail_stream, jobs = vr.jobs_of(source, name)
  _, layers_, _, data, ws = vr.setup(source, name, regime, dev)
  refs = vr.reference(oracle, source, name, regime)
  d32, scale = vr.case_d32(oracle, source, name, regime), vr.bar_scale(oracle, source, name, regime)
  bar = GOLDEN_TOL * scale
  tune(**knobs)
  recorder = _RecordForward(monkeypatch)
  saved = []

  def read_saved():
    """What the forward kept for the BPTT: the arg-max in input order, the update gate of the frozen units."""
    for j, ctx in zip(jobs, recorder.calls[-1]):
      a, g = ops.saved_region(ctx, 'argmax'), ops.saved_region(ctx, 'gates')
      route = None
      if a is not None:
        route = np.empty(tuple(a.shape), dtype=np.int64)
        route[ctx['sched'].order] = a.cpu().numpy()
      z = None if g is None else g.cpu().numpy()[:, j['H']:2 * j['H']]
      saved.append((route, z))

  def run():
    if train:
      del saved[:]
      return _run_training(jobs, layers_, data, ws, dev, after_forward=read_saved)
    return [[o.clone()] for o, _ in _run_inference(jobs, layers_, data, dev, tail_stream)]

  first, again = run(), run()
  for k, (a, b) in enumerate(zip(first, again)):
    for i, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), '%s: request %d result %d not reproducible from run to run' % (cid, k, i)

  d_out = d_norm = 0.0
  outs = [f[0].cpu().numpy() for f in first]
  for j, got, ref in zip(jobs, outs, refs):
    d_out = max(d_out, _dist(got, ref['want']))
    if j['pool'] != 'ALL':
      d_norm = max(d_norm, _dist(vr.normalised(got), vr.normalised(ref['want'])))
  print('value_regimes %-40s d32 %.3e  bar %.3e  kernel %.3e  norm %.3e' % (cid, d32, bar, d_out, d_norm))

  for k, (j, got, ref, (lens, x, h0, _, _)) in enumerate(zip(jobs, outs, refs, data)):
    tag = '%s request %d (%s, I %d, H %d)' % (cid, k, j['pool'], j['I'], j['H'])
    assert np.isfinite(got).all(), tag
    assert_emb_close(got, ref['want'], tag, tight=bar)
    if regime in vr.NORMALISED_REGIMES and j['pool'] != 'ALL':
      assert_emb_close(vr.normalised(got), vr.normalised(ref['want']), tag + ' L2-normalised', tight=bar)
    if regime == 'frozen':
      _check_frozen_outputs(j, got, h0, lens, tag)
    if not train:
      continue
    u = vr.marked_units(j['H'])
    route, z = saved[k]
    cache = dict(ref['cache'])
    if regime == 'frozen':
      assert z is not None and (z[:, u] == 1.0).all(), tag + ': the saved update gate of a frozen unit is not 1.0f'
    if j['pool'] == 'MAX':
      assert route is not None, tag
      if regime == 'frozen':
        assert not route[:, u].any(), tag + ': the arg-max of a frozen unit left step 0'
      report = {}
      oracle.apply_argmax_route({'r': cache}, {'r': route}, report)
      n_diff, gap, n_pairs = report['r']
      assert gap <= ROUTE_GAP, '%s: routed away from the fp64 arg-max across a gap of %.3e (%d of %d pairs)' % (
          tag, gap, n_diff, n_pairs)
    with _blas_threads(), np.errstate(over='ignore'):
      grads, dx, dh0 = _backward(oracle, j, cache, lens, ws[k])
    res = first[k]
    grad_close(res[1].cpu().numpy()[:, :dx.shape[1]], dx, tag + ' dx')
    if h0 is not None:
      grad_close(res[2].cpu().numpy(), dh0, tag + ' dh0')
    params = res[3:] if h0 is not None else res[2:]
    names = [pn for pn, _ in layers_[k].named_parameters()]
    assert len(names) == len(params), tag
    if j['pool'] == 'ATTN':      # dw_att, dw_lin, db_lin go through grad_close like the rest
      assert {'lin.weight', 'lin.bias', 'att_w.weight'} <= set(names), tag
    for pn, g in zip(names, params):
      grad_close(g.cpu().numpy(), grads['rnn.' + pn], tag + ' ' + pn)


@pytest.mark.parametrize('case', _BF3, ids=[c[0] for c in _BF3])
def test_value_regime_bf3_vs_oracle_and_emulation(dev, oracle, tune, case):
  """The bf16x3 cases: output and every packed hidden state against the oracle and against the emulation
  of the split, at the bars of test_gpu_bf3_shapes.py scaled by the regime's d32 ratio; the re-split
  states (pack_bf16 in the TiledBf3 epilogue) are, bit for bit, the split of the fp32 states."""
  from cmhse_amd import ops
  cid, source, name, regime, _ = case
  knobs, _, tail_stream, jobs = vr.jobs_of(source, name)
  _, layers_, _, data, _ = vr.setup(source, name, regime, dev)
  refs = vr.reference(oracle, source, name, regime)
  d32, scale = vr.case_d32(oracle, source, name, regime), vr.bar_scale(oracle, source, name, regime)
  plan = fwd_shapes.call_steps(jobs, knobs, tail_stream, bf3=True)
  tune(**knobs)

  def run():
    got = []
    for out, ctx in _run_inference(jobs, layers_, data, dev, tail_stream):
      views = {r: ops.saved_region(ctx, r) for r in ('hs', 'hs_s')}
      got.append(dict(out=out.cpu().numpy(), order=ctx['sched'].order,
                      **{r: None if v is None else v.cpu().numpy() for r, v in views.items()}))
    return got

  assert ops.math_mode() == 'fp32'
  ops.set_math_mode('bf16x3')
  try:
    first, again = run(), run()
  finally:
    ops.set_math_mode('fp32')
  failures = []
  d_or = d_emu = d_norm = d_mode = 0.0
  for k, (j, launches, ref, g, g2, (lens, x, h0, _, _)) in enumerate(zip(jobs, plan, refs, first, again, data)):
    tag = '%s request %d (%s, I %d, H %d)' % (cid, k, j['pool'], j['I'], j['H'])
    order, counts = g['order'], j['counts']
    if not (np.array_equal(g['out'], g2['out']) and np.array_equal(g['hs'], g2['hs'])):
      failures.append(tag + ': not reproducible')
    want_hs = packed(ref['cache']['hs'], order, counts)
    emu_hs = packed(ref['emu_hs'], order, counts)
    r_or = max(_dist(g['out'], ref['want']), _dist(g['hs'], want_hs))
    r_emu = max(_dist(g['out'], ref['emu']), _dist(g['hs'], emu_hs))
    d_or, d_emu = max(d_or, r_or), max(d_emu, r_emu)
    # against the oracle: test_gpu_bf3_shapes.py's bar for the mode, scaled; and never further than the
    # mode's own arithmetic is (the emulation's distance from the oracle) plus the bar against the emulation
    r_mode = max(_dist(ref['emu'], ref['want']), _dist(ref['emu_hs'], ref['cache']['hs']))
    d_mode = max(d_mode, r_mode)
    if r_or > min(BF3_TOL * scale, r_mode + GOLDEN_TOL * scale):
      failures.append(tag + ': %.3e from the float64 oracle (the emulation: %.3e)' % (r_or, r_mode))
    if r_emu > GOLDEN_TOL * scale:
      failures.append(tag + ': %.3e from the emulation of the split' % r_emu)
    if regime in vr.NORMALISED_REGIMES and j['pool'] != 'ALL':
      r_norm = _dist(vr.normalised(g['out']), vr.normalised(ref['emu']))
      d_norm = max(d_norm, r_norm)
      if r_norm > GOLDEN_TOL * scale:
        failures.append(tag + ': L2-normalised, %.3e from the emulation of the split' % r_norm)
    if regime == 'frozen':
      _check_frozen_outputs(j, g['out'], h0, lens, tag)
    rows = launches.rows_split
    if launches.bf3 and rows > 0:
      hs_s = oracle.split_rows_bits(g['hs'][:rows], j['H'])
      if not np.array_equal(g['hs_s'][:rows].view(np.uint32), hs_s):
        failures.append(tag + ': hs_s is not the split of hs')
  print('value_regimes %-40s d32 %.3e  bar %.3e  kernel %.3e  norm %.3e  (emulation; oracle: kernel %.3e, emulation %.3e, '
        'bar %.3e)' % (cid, d32, GOLDEN_TOL * scale, d_emu, d_norm, d_or, d_mode, BF3_TOL * scale))
  assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------
# the row kernels at the 1e-12 clamp
# ------------------------------------------------------------------------------------------------
def _autograd_normalize(x, g):
  xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
  y = torch.nn.functional.normalize(xt)
  y.backward(torch.from_numpy(np.asarray(g, dtype=np.float64)))
  return y.detach().numpy(), xt.grad.numpy()


# y = x * (1 / max(sqrt(sum x^2), eps)): one fp32 sum of squares (its relative error halves under the
# root), one sqrt, one divide, one multiply — about 3 roundings of 6e-8 on every element
NORM_FWD_RTOL = 2e-7
# dx = (g - x d) / max(||x||, eps), d = (x.g) / ||x||^2: two fp32 dot products over the row and a handful
# of roundings on terms no larger than ||g|| / max(||x||, eps) each (|x (x.g)| <= ||x||^2 ||g||): 2e-6
# of that magnitude is ~30 roundings of 6e-8, the depth of the 1028-column sums (5 per thread, 6
# shuffles, 4 partials) plus the elementwise ones
NORM_BWD_RTOL = 2e-6


@pytest.mark.parametrize('cols,ld', [(c, c) for c in vr.NORM_COLS] + [(33, 40)], ids=lambda v: str(v))
def test_l2norm_rows_at_the_clamp(dev, cols, ld):
  from cmhse_amd import _lib, ops
  x, _ = vr.clamp_rows(cols)
  want, _ = _autograd_normalize(x, np.zeros_like(x))
  buf = np.full((vr.NORM_ROWS, ld), 7.0, dtype=np.float32)
  buf[:, :cols] = x
  xd = torch.from_numpy(buf).to(dev)
  yd = torch.full((vr.NORM_ROWS, ld), -3.0, dtype=torch.float32, device=dev)
  rc = _lib.load().cmhse_l2norm_rows(xd.data_ptr(), yd.data_ptr(), vr.NORM_ROWS, cols, ld, ops._stream())
  _lib.check(rc, 'cmhse_l2norm_rows')
  torch.cuda.synchronize()
  got = yd.cpu().numpy()
  assert (got[:, cols:] == -3.0).all(), 'a row was written past its columns'
  got = got[:, :cols]
  assert not got[0].any()
  for r in range(vr.NORM_ROWS):
    top = np.abs(want[r]).max()
    err = np.abs(got[r] - want[r]).max()
    print('value_regimes l2norm fwd cols %4d ld %4d row %d  err %.3e  bound %.3e' % (cols, ld, r, err, NORM_FWD_RTOL * top))
    assert err <= NORM_FWD_RTOL * top, (cols, r, err, top)


@pytest.mark.parametrize('cols', vr.NORM_COLS)
def test_l2norm_rows_bwd_at_the_clamp(dev, cols):
  """Against float64 torch autograd (not oracle.l2_normalize_backward): inside the clamp dx = g / 1e-12."""
  from cmhse_amd import ops
  x, g = vr.clamp_rows(cols)
  _, want = _autograd_normalize(x, g)
  got = ops.l2norm_rows_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)).cpu().numpy()
  assert np.isfinite(got).all()
  nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
  for r in range(vr.NORM_ROWS):
    mag = np.sqrt((g[r].astype(np.float64) ** 2).sum()) / max(nrm[r], vr.NORM_EPS)
    err = np.abs(got[r] - want[r]).max()
    print('value_regimes l2norm bwd cols %4d row %d  err %.3e  bound %.3e' % (cols, r, err, NORM_BWD_RTOL * mag))
    assert err <= NORM_BWD_RTOL * mag, (cols, r, err, mag)


def _torch_contrastive(im, s, margin, max_violation):
  """oracle.contrastive_loss (norm=True) in torch, for autograd."""
  scores = im @ s.t()
  n = scores.shape[0]
  diag = scores.diag().view(n, 1)
  eye = torch.eye(n, dtype=torch.bool)
  cost_s = (margin + scores - diag).clamp(min=0).masked_fill(eye, 0)
  cost_im = (margin + scores - diag.t()).clamp(min=0).masked_fill(eye, 0)
  if max_violation:
    cost_s, cost_im = cost_s.max(1)[0], cost_im.max(0)[0]
  return (cost_s.sum() + cost_im.sum()) / (n * n)


@pytest.mark.parametrize('max_violation', [False, True], ids=['sum', 'max'])
def test_step_losses_at_the_clamp(dev, oracle, max_violation):
  """cmhse_step_losses_fwd / _bwd (F.normalize straight into the row-blocked operands, l2norm_bwd_row through a
  functor) with a zero row and a sub-eps row in one embedding: the normalised rows, the loss value and dx
  against float64 autograd of F.normalize + the contrastive loss (its value checked against the oracle's)."""
  from cmhse_amd import ops
  n, D, margin = 5, 8, 0.2
  rng = np.random.RandomState(8)
  a = rng.standard_normal((n, D))
  b = rng.standard_normal((n, D))
  a[1] = 0
  a[3] *= 0.9e-12 / np.sqrt((a[3] ** 2).sum())
  a, b = a.astype(np.float32), b.astype(np.float32)
  at, bt = (torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for v in (a, b))
  ya, yb = torch.nn.functional.normalize(at), torch.nn.functional.normalize(bt)
  ya.retain_grad()
  yb.retain_grad()
  with torch.no_grad():      # no score sits at its hinge: fp32 and float64 select the same terms
    sc = ya @ yb.t()
    off = ~torch.eye(n, dtype=torch.bool)
    assert min((margin + sc - sc.diag().view(n, 1))[off].abs().min(), (margin + sc - sc.diag().view(1, n))[off].abs().min()) > 1e-3
  loss = _torch_contrastive(ya, yb, margin, max_violation)
  (1.5 * loss).backward()
  want = oracle.contrastive_loss(ya.detach().numpy(), yb.detach().numpy(), margin=margin,
                                 max_violation=max_violation, norm=True, dtype=np.float64)
  assert abs(loss.item() - float(want)) <= 1e-14 and float(want) > 0
  ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  values, total, st = ops.step_losses_fwd([ad, bd], [(0, 1, 1.0)], margin, max_violation, True)
  dxs = ops.step_losses_bwd(st, torch.full((1,), 1.5, device=dev))
  torch.cuda.synchronize()
  # the normalised rows in the workspace (loss_layout.hpp StepLossLayout: y_im at 512, y_s one 256-aligned
  # [R, D] matrix behind it); a moved layout fails the bit comparison with cmhse_l2norm_rows first
  mat = (n * D * 4 + 255) // 256 * 256
  for side, (xd, y64) in enumerate(((ad, ya), (bd, yb))):
    rows = st['ws'][512 + side * mat:512 + side * mat + n * D * 4].view(torch.float32).view(n, D)
    assert torch.equal(rows, ops.l2norm_rows(xd)), 'the workspace rows are not the normalised rows (layout?)'
    y64 = y64.detach().numpy()
    for r in range(n):
      assert np.abs(rows[r].cpu().numpy() - y64[r]).max() <= NORM_FWD_RTOL * np.abs(y64[r]).max(), (side, r)
  # the loss: a mean of n^2 hinge terms of O(1) scores, each an 8-term fp32 dot product of rows normalised to 2e-7
  assert abs(values[0].item() - float(want)) <= 2e-6 * max(1.0, abs(float(want))), (values[0].item(), float(want))
  assert abs(total.item() - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
  # dx = the F.normalize backward of the gradient gy wrt the normalised rows.  NORM_BWD_RTOL is relative to
  # ||gy_r|| / max(||x_r||, eps); gy itself is an fp32 sum of up to 2n normalised rows (2e-7 each) with
  # coefficients of 1.5 / n^2, another ~2e-6 of its magnitude, which the division by the norm carries along
  for e, (x, xt, yt, dx) in enumerate(((a, at, ya, dxs[0]), (b, bt, yb, dxs[1]))):
    got, ref, gy = dx.cpu().numpy(), xt.grad.numpy(), yt.grad.numpy()
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    for r in range(n):
      mag = np.sqrt((gy[r] ** 2).sum()) / max(nrm[r], vr.NORM_EPS)
      err = np.abs(got[r] - ref[r]).max()
      print('value_regimes step_losses mv%d emb %d row %d  err %.3e  bound %.3e' % (max_violation, e, r, err, 2 * NORM_BWD_RTOL * mag))
      assert err <= 2 * NORM_BWD_RTOL * mag, (e, r, err, mag)


def test_euclid_bwd_nan_stays_in_its_row(dev, oracle):
  """decoder/loss.py's EuclideanLoss has no epsilon under its sqrt: an exactly reconstructed row (a == b) gives
  NaN upstream and here (loss_kernels.hpp).  Exactly that row of d_a is NaN; every other row matches."""
  from cmhse_amd import ops
  rows, cols = 6, 33
  rng = np.random.RandomState(12)
  a = rng.standard_normal((rows, cols)).astype(np.float32)
  b = rng.standard_normal((rows, cols)).astype(np.float32)
  b[2] = a[2]
  for norm in (True, False):
    got = ops.euclid_bwd(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), None, norm,
                         torch.full((1,), 3.0, device=dev)).cpu().numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
      want = 3.0 * oracle.euclidean_loss_backward(a, b, norm, np.float64)
    assert np.isnan(want[2]).all() and np.isnan(got[2]).all()
    keep = [r for r in range(rows) if r != 2]
    assert np.isfinite(got[keep]).all()
    grad_close(got[keep], want[keep], 'euclid d_a norm%d' % norm)
