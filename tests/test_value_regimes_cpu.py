"""The value regimes are what their names say, and their cases land on the kernels they name (no GPU
needed): every property of tests/value_regimes.py's regimes proved from the float64 oracle alone, the
head-room of the fp32 oracle under every bar tests/test_gpu_value_regimes.py asserts (outputs,
normalised outputs, gradients), the (family, regime) coverage from the dispatch rules of fwd_shapes and
bptt_shapes, and the clamp branch of the oracle's F.normalize backward against float64 autograd."""
import numpy as np
import pytest
import torch

from conftest import EMB_TOL, GOLDEN_TOL

import bptt_shapes
import fwd_shapes as fs
import value_regimes as vr
from test_gpu_fwd_shapes import _backward

_IDS = [c[0] for c in vr.CASES]
HEADROOM = 4.0


def _active(ref):
  """[S, Tmax] mask of the steps inside their sequences."""
  c = ref['cache']
  return np.arange(c['Tmax'])[None, :] < c['lens'][:, None]


def _grad_err(got, want):
  """(max |diff|, the tolerance of gpu_common.grad_close)."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape
  return np.abs(got - want).max(), 2e-4 * max(1e-30, np.abs(want).max()) + 2e-6


# ------------------------------------------------------------------------------------------------
# the case table and its coverage
# ------------------------------------------------------------------------------------------------
def test_cases_are_taken_by_name_and_reach_their_tags():
  assert len(set(_IDS)) == len(_IDS)
  vocabulary = fs.ALL_TAGS | fs.BF3_TAGS | set(vr.REGIMES)
  vocabulary |= set().union(*[c[8] for c in bptt_shapes.CASES]) | {'Mid16', 'Mid32', 'Split'}
  vocabulary |= {'Tail KB%d MB%d' % (kb, mb) for kb in bptt_shapes.TAIL_KBS for mb in (1, 2)}
  for cid, source, name, regime, tags in vr.CASES:
    assert regime in tags and regime in vr.REGIMES, cid
    family_tags = tags - {regime}
    assert family_tags and family_tags <= vocabulary, (cid, sorted(family_tags - vocabulary))
    reached = vr.shape_tags(source, name)
    assert family_tags <= reached, (cid, sorted(family_tags - reached))
    knobs, train, tail_stream, jobs = vr.jobs_of(source, name)
    assert all(not j['vocab'] for j in jobs), cid       # a regime scales inputs: no token-fed request
    if regime in vr.ATTN_REGIMES:
      assert any(j['pool'] == 'ATTN' for j in jobs), cid
    if source == 'bf3':
      assert regime in vr.BF3_REGIMES and not train, cid
  # the BPTT tags come from bptt_shapes' vocabulary
  for source, name, tags in vr.SHAPES:
    if source == 'bptt':
      case = next(c for c in bptt_shapes.CASES if c[0] == name)
      assert tags <= case[8] | {'Mid16'}, name


def test_every_family_meets_every_regime():
  reached = set()
  for cid, source, name, regime, tags in vr.CASES:
    reached |= vr.families_reached(source, name, regime)
  required = {(f, r) for f in vr.FWD_FAMILIES for r in vr.REGIMES}
  required |= {(f, r) for f in vr.BWD_FAMILIES for r in vr.GATE_REGIMES}
  required |= {('AttnPoolBwd', r) for r in vr.REGIMES}
  assert set(vr.UNREACHABLE) <= required and not set(vr.UNREACHABLE) & reached, sorted(set(vr.UNREACHABLE) & reached)
  assert all(isinstance(why, str) and why for why in vr.UNREACHABLE.values())
  missing = required - reached - set(vr.UNREACHABLE)
  assert not missing, sorted(missing)
  # the bf16x3 attention projection on both sides of its cut, under every regime of the mode
  for r in vr.BF3_REGIMES:
    tags = set().union(*[t for _, s, _, reg, t in vr.CASES if s == 'bf3' and reg == r])
    assert {'Attn ring', 'Attn split-in-loop', 'Attn final both', 'TiledBf3'} <= tags, r


def test_frozen_holds_a_nonzero_state_in_inference_and_in_training():
  seen = set()
  for cid, source, name, regime, tags in vr.CASES:
    if regime == 'frozen':
      knobs, train, _, jobs = vr.jobs_of(source, name)
      seen |= {(train, j['h0'], j['pool']) for j in jobs}
  for train in (False, True):
    assert any(t == train and h0 for t, h0, _ in seen), train
    assert any(t == train and not h0 for t, h0, _ in seen), train      # ... and a state that stays exactly 0
    assert any(t == train and pool == 'MAX' for t, _, pool in seen), train


# ------------------------------------------------------------------------------------------------
# the regimes are what their names say (float64 oracle)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', vr.CASES, ids=_IDS)
def test_regime_property(oracle, case):
  cid, source, name, regime, _ = case
  refs = vr.reference(oracle, source, name, regime)
  base = vr.reference(oracle, source, name, 'baseline')
  jobs = vr.jobs_of(source, name)[3]
  _, _, sds, data, _ = vr.setup(source, name, regime, torch.device('cpu'))
  sat_rz, sat_n, n_gate = 0, 0, 0
  e_lo, e_hi, peaked, n_seq = np.inf, -np.inf, 0, 0
  for j, ref, b, sd, (lens, x, h0, _, _) in zip(jobs, refs, base, sds, data):
    c, act = ref['cache'], _active(ref)
    H = j['H']
    r, z, n = (c['gates'][:, :, k][act] for k in range(3))      # [active steps, H]
    for v in [ref['want'], ref['want32'], c['hs'], c['gates']]:
      assert np.isfinite(v).all(), cid
    assert np.abs(x).max() < 1e4 and all(np.abs(v).max() < 1e4 for v in sd.values()), cid
    u = vr.marked_units(H)
    if regime == 'saturated':
      # |pre-activation| > 8 <=> the gate is outside (sigmoid(-8), sigmoid(8)); > 4 <=> |n| > tanh(4)
      s8 = 1.0 / (1.0 + np.exp(-8.0))
      sat_rz += ((r > s8) | (r < 1 - s8)).sum() + ((z > s8) | (z < 1 - s8)).sum()
      sat_n += (np.abs(n) > np.tanh(4.0)).sum()
      n_gate += r.size
    elif regime == 'frozen':
      assert (z[:, u] == 1.0).all(), cid
      held = np.zeros((len(lens), H)) if h0 is None else h0.astype(np.float64)
      for t in range(c['Tmax']):
        rows = act[:, t]
        assert np.array_equal(c['hs'][rows, t][:, u], held[rows][:, u]), (cid, t)
      if j['pool'] == 'MAX':
        assert not c['argmax'][:, u].any(), cid
      if j['pool'] in ('LAST', 'MAX'):
        assert np.array_equal(ref['want'][:, u], held[:, u]), cid
    elif regime == 'reset_off':
      assert (r[:, u] < 1e-40).all() and (r[:, u] >= 0).all(), cid
      # ... so the r * (W_hn h + b_hn) term vanishes: far below an ulp of anything it is added to
      assert np.abs(r[:, u] * c['gates'][:, :, 3][act][:, u]).max() < 1e-38, cid
    elif regime in vr.SMALL_SCALES:
      scale = vr.SMALL_SCALES[regime]
      ratio = np.abs(ref['want']).max() / (scale * np.abs(b['want']).max())
      assert 0.1 <= ratio <= 10.0, (cid, ratio)
      if j['pool'] != 'ALL':
        assert ref['d32n'] <= 5e-7, (cid, ref['d32n'])
    elif regime in vr.ATTN_REGIMES and j['pool'] == 'ATTN':
      e = (c['v'] @ c['w_att'])[act]
      att = c['att']
      assert np.abs(e).max() <= 60.0, (cid, np.abs(e).max())      # exp stays inside fp32
      if regime == 'attn_peaked':
        e_lo, e_hi = min(e_lo, e.min()), max(e_hi, e.max())
        peaked += (att.max(axis=1) > 0.99).sum()
        n_seq += len(lens)
      else:
        sums = att.sum(axis=1)
        assert sums.max() < 0.5 and sums.min() > 0.0, (cid, sums.min(), sums.max())
  if regime == 'saturated':
    assert sat_rz >= 0.5 * 2 * n_gate, (cid, sat_rz / (2.0 * n_gate))
    assert sat_n >= 0.25 * n_gate, (cid, sat_n / float(n_gate))
  if regime == 'attn_peaked':
    assert e_lo < -30 and e_hi > 30, (cid, e_lo, e_hi)
    assert peaked > 0.5 * n_seq, (cid, peaked, n_seq)


# ------------------------------------------------------------------------------------------------
# head-room: the oracle in fp32 passes every bar of the GPU tests with room to spare
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', vr.CASES, ids=_IDS)
def test_fp32_oracle_has_headroom_under_the_bars(oracle, case):
  cid, source, name, regime, _ = case
  refs = vr.reference(oracle, source, name, regime)
  jobs = vr.jobs_of(source, name)[3]
  scale = vr.bar_scale(oracle, source, name, regime)
  bar = GOLDEN_TOL * scale
  d32 = vr.case_d32(oracle, source, name, regime)
  assert HEADROOM * d32 <= min(bar, EMB_TOL), (cid, d32, bar)
  if regime in vr.NORMALISED_REGIMES:
    d32n = max(r['d32n'] for j, r in zip(jobs, refs) if j['pool'] != 'ALL')
    assert HEADROOM * d32n <= bar, (cid, d32n, bar)
  if not vr.jobs_of(source, name)[1]:
    return
  # gradients: the oracle's own backward in fp32 against float64 (max pooling: both through the float64
  # arg-max, the check is on the arithmetic)
  for k, (j, ref) in enumerate(zip(jobs, refs)):
    c32 = dict(ref['cache32'])
    if j['pool'] == 'MAX':
      c32['argmax'] = ref['cache']['argmax']
    with np.errstate(over='ignore'):
      g64, dx64, dh64 = _backward(oracle, j, ref['cache'], ref['lens'], ref['w'])
      g32, dx32, dh32 = _backward(oracle, j, c32, ref['lens'], ref['w'])
    assert dx32.dtype == np.float32 and all(v.dtype == np.float32 for v in g32.values()), cid
    pairs = [('dx', dx32, dx64), ('dh0', dh32, dh64)] + [(n, g32[n], g64[n]) for n in sorted(g64)]
    for what, a, b in pairs:
      err, tol = _grad_err(a, b)
      assert HEADROOM * err <= tol, (cid, k, what, err, tol)


# ------------------------------------------------------------------------------------------------
# F.normalize at the clamp
# ------------------------------------------------------------------------------------------------
def _autograd_normalize(x, g):
  xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
  y = torch.nn.functional.normalize(xt)
  y.backward(torch.from_numpy(np.asarray(g, dtype=np.float64)))
  return y.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize('cols', vr.NORM_COLS)
def test_clamp_rows_are_what_they_say(cols):
  x, g = vr.clamp_rows(cols)
  nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
  assert nrm[0] == 0 and not x[0].any()
  for r, want in ((1, 0.5e-12), (2, 0.9e-12), (3, 1.1e-12)):
    assert abs(nrm[r] / want - 1) < 1e-6, (r, nrm[r])
  assert nrm[2] < np.float32(1e-12) < nrm[3]
  sq = x.astype(np.float64) ** 2
  tiny, huge = np.finfo(np.float32).tiny, np.finfo(np.float32).max
  assert (sq[x != 0] > tiny).all() and sq.sum(axis=1).max() < huge      # no square flushes, no sum overflows
  assert 1e-16 < np.abs(x[4]).mean() < 1e-14 and 1e14 < np.abs(x[5]).mean() < 1e16
  assert 0.1 < nrm[6] / np.sqrt(cols) < 10


@pytest.mark.parametrize('cols', vr.NORM_COLS)
def test_oracle_normalize_backward_matches_autograd_at_the_clamp(oracle, cols):
  """Inside the clamp (0 < ||x|| < 1e-12) torch's clamp_min passes no gradient to the norm: dx = g / 1e-12,
  without the projection term (at ||x|| = 0.9e-12 the term is worth 81 % of (y.g) y)."""
  x, g = vr.clamp_rows(cols)
  y, dx = _autograd_normalize(x, g)
  np.testing.assert_allclose(oracle.l2_normalize(x, np.float64), y, rtol=1e-13, atol=0)
  got = oracle.l2_normalize_backward(x, g)
  for r in range(vr.NORM_ROWS):
    np.testing.assert_allclose(got[r], dx[r], rtol=0, atol=1e-12 * np.abs(dx[r]).max(), err_msg='row %d' % r)
  for r in (0, 1, 2, 4):
    np.testing.assert_allclose(dx[r], g[r].astype(np.float64) / 1e-12, rtol=1e-13)
  # the projection formula inside the clamp differs visibly on the sub-eps rows: the test can tell the two
  x64, g64 = x.astype(np.float64), g.astype(np.float64)
  yy = x64 / 1e-12
  old = (g64 - yy * (yy * g64).sum(axis=1, keepdims=True)) / 1e-12
  for r in (1, 2):
    assert np.abs(old[r] - dx[r]).max() > 1e-3 * np.abs(dx[r]).max(), r
