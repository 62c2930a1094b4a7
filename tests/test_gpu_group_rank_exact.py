"""Certified group-wise ranking (cmhse_group_rank_exact, ops.group_rank_exact, evaluation.group_i2t_t2i_exact)
on the MI355X against NumPy float64: the contract is test_group_rank_exact_cpu.group_exact_reference of the
float64 block scores; every fixture asserts the gaps that make that reference independent of summation order
before anything is compared, and every comparison is over all queries."""
import functools

import numpy as np
import pytest
import torch

from test_group_rank_exact_cpu import (GROUP_GAP, GROUP_NEAR_TIE_SHAPES, REDUCES, block_scores, float64_noise,
                                       group_exact_reference, group_min_gaps, group_near_tie_fixture,
                                       near_tie_seed)
from test_gpu_group_rank import CASES as TILING      # the tiling cases of the fp32 call, shape for shape

pytestmark = pytest.mark.gpu

NAMES = ['rank_lo_v2p', 'rank_hi_v2p', 'top1_v2p', 'resolved_v2p', 'rank_lo_p2v', 'rank_hi_p2v', 'top1_p2v',
         'resolved_p2v']
RANKS = [0, 1, 4, 5]          # the four certified vectors among the eight outputs


def _dev(dev, x):
  return torch.from_numpy(x.copy()).to(dev)      # (the cached fixtures are read-only arrays)


def _run(dev, clips, caps, nc, ns, reduce):
  from cmhse_amd import ops
  out = ops.group_rank_exact(_dev(dev, clips), _dev(dev, caps), nc, ns, reduce)
  assert len(out) == 8
  for t in out:
    assert t.dtype == torch.int32 and t.shape == (len(nc),) and t.is_cuda
  return [t.cpu().numpy() for t in out]


def _assert_ranks(got, G64, what=''):
  for k, want in zip(RANKS, group_exact_reference(G64)):
    assert np.array_equal(got[k], want), '%s %s: %d of %d queries differ' % (
        what, NAMES[k], np.count_nonzero(got[k] != want), len(want))


# ---------------------------------------------------------------------------------------------
# 1, 2: the near-tie fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', GROUP_NEAR_TIE_SHAPES)
def test_near_tie_fixtures_equal_the_float64_reference(dev, n, d, max_rows, reduce):
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  got = _run(dev, clips, caps, nc, ns, reduce)
  print('near-tie n=%d d=%d rows<=%d %s: resolved %d + %d of %d blocks'
        % (n, d, max_rows, reduce, got[3].sum(), got[7].sum(), len(nc) * (len(nc) - 1)))
  _assert_ranks(got, G64)
  tied = np.r_[0:n, 5 * n:6 * n]                           # an exact tie is undecided by construction
  assert (got[3][tied] >= 1).all() and (got[7][tied] >= 1).all()


@pytest.mark.parametrize('reduce', REDUCES)
def test_fp32_group_ranks_differ_on_the_fixture(dev, reduce):
  """Why the call exists: ops.group_rank on the same rows is the ranking of one fp32 summation order."""
  from cmhse_amd import ops
  n, d, max_rows = 44, 1024, 5
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  c, s = _dev(dev, clips), _dev(dev, caps)
  r_v, t_v, r_p, t_p = [t.cpu().numpy() for t in ops.group_rank(c, s, nc, ns, reduce)]
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(G64)
  differ = np.count_nonzero(r_v != lo_v), np.count_nonzero(r_p != lo_p)
  print('fp32 group_rank differs from the float64 ranks on %d / %d of %d queries (%s)' % (differ + (len(nc), reduce)))
  assert differ[0] > 0 and differ[1] > 0
  got = _run(dev, clips, caps, nc, ns, reduce)
  _assert_ranks(got, G64)
  assert np.array_equal(got[2], t_v) and np.array_equal(got[6], t_p)     # top1 is group_rank's


# ---------------------------------------------------------------------------------------------
# 3: the tiling cases of test_gpu_group_rank.py, un-normalised rows
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiling_inputs(idx):
  """Rows of norm ~ sqrt(D) and the float64 clip x caption matrix (shared by the two reduce modes; not modified)."""
  _, nc, ns, d = TILING[idx]
  ns = nc if ns is None else ns
  rng = np.random.RandomState(100 + idx)
  clips = rng.standard_normal((int(sum(nc)), d)).astype(np.float32)
  caps = rng.standard_normal((int(sum(ns)), d)).astype(np.float32)
  S64 = clips.astype(np.float64) @ caps.astype(np.float64).T
  scale = float(np.linalg.norm(clips.astype(np.float64), axis=1).max() *
                np.linalg.norm(caps.astype(np.float64), axis=1).max())
  return clips, caps, np.asarray(nc), np.asarray(ns), S64, scale


@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('idx', range(len(TILING)), ids=[c[0] for c in TILING])
def test_tiling_cases_unnormalised_rows(dev, idx, reduce):
  clips, caps, nc, ns, S64, scale = _tiling_inputs(idx)
  d = clips.shape[1]
  G64 = block_scores(S64, nc, ns, reduce)
  gaps = group_min_gaps(G64)
  print('%s %s: min gaps %.3g / %.3g, bar %.3g' % (TILING[idx][0], reduce, gaps[0], gaps[1], GROUP_GAP * scale))
  assert min(gaps) > GROUP_GAP * scale                     # the shape-scaled gap (|a| |b| up to `scale`, not 1)
  assert 4 * float64_noise(S64, nc, ns, d, reduce, scale) < GROUP_GAP * scale
  got = _run(dev, clips, caps, nc, ns, reduce)
  _assert_ranks(got, G64, TILING[idx][0])
  assert np.array_equal(got[0], got[1]) and np.array_equal(got[4], got[5])     # no ties in random rows
  assert (got[3] <= len(nc) - 1).all() and (got[7] <= len(nc) - 1).all()


# ---------------------------------------------------------------------------------------------
# 4: the tolerance only moves `resolved`
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', [(22, 64, 5), (4, 96, 100)])
def test_results_do_not_depend_on_the_tolerance(dev, tune, n, d, max_rows, reduce):
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  B = len(nc)
  base = _run(dev, clips, caps, nc, ns, reduce)
  _assert_ranks(base, G64)
  prev = base
  for scale in (16, 1 << 20):
    tune(rank_exact_tol_scale=scale)
    got = _run(dev, clips, caps, nc, ns, reduce)
    for k in (0, 1, 2, 4, 5, 6):
      assert np.array_equal(got[k], base[k]), (scale, NAMES[k])
    assert (got[3] >= prev[3]).all() and (got[7] >= prev[7]).all()        # a wider tolerance decides no more
    prev = got
  assert (prev[3] == B - 1).all() and (prev[7] == B - 1).all()            # 2^20, D >= 16: every block


# ---------------------------------------------------------------------------------------------
# 5: a collapsed low level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('kind', ['ragged_exact_sums', 'equal_counts_random_row'])
def test_collapsed_model_reports_the_whole_interval(dev, kind, reduce):
  """All rows equal.  Bit-identical groups tie exactly (the contract); groups of different counts do under 'mean'
  only where the float64 sums are exact, so the ragged case uses a row whose score is 1.0 (its sums n * 1.0 and
  their quotients by n round nothing) and the random row comes with equal counts."""
  rng = np.random.RandomState(2)
  if kind == 'ragged_exact_sums':
    B, d = 70, 64
    nc, ns = rng.randint(1, 9, B), rng.randint(1, 9, B)
    row = np.zeros(d, dtype=np.float32)
    row[[3, 17, 40, 63]] = 0.5
  else:
    B, d = 70, 300
    nc, ns = np.full(B, 3), np.full(B, 2)
    row = rng.standard_normal(d).astype(np.float32)
    row /= np.linalg.norm(row)
  clips, caps = np.tile(row, (int(nc.sum()), 1)), np.tile(row, (int(ns.sum()), 1))
  got = _run(dev, clips, caps, nc, ns, reduce)
  for k in (0, 4):
    assert (got[k] == 0).all(), NAMES[k]
  for k in (1, 5):
    assert (got[k] == B - 1).all(), NAMES[k]
  assert (got[3] == B - 1).all() and (got[7] == B - 1).all()              # every tie went through float64


# ---------------------------------------------------------------------------------------------
# 6: well-separated groups never reach float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_well_separated_groups_resolve_nothing(dev, reduce):
  """Orthogonal groups: video i lives on axis i (clip r scaled by r + 1), paragraph j holds 0.1 e_j + e_(j+1):
  G[i, i] <= 0.5, G[j + 1, j] >= 1, every other block 0 — apart by 0.1 at least, the tolerance is below 1e-4."""
  from cmhse_amd import ops
  rng = np.random.RandomState(4)
  B, d = 70, 96
  nc, ns = rng.randint(1, 6, B), rng.randint(1, 6, B)
  clips = np.zeros((int(nc.sum()), d), dtype=np.float32)
  caps = np.zeros((int(ns.sum()), d), dtype=np.float32)
  clips[np.arange(len(clips)), np.repeat(np.arange(B), nc)] = np.concatenate([np.arange(1, k + 1) for k in nc])
  pj = np.repeat(np.arange(B), ns)
  caps[np.arange(len(caps)), pj] = 0.1
  caps[np.arange(len(caps)), (pj + 1) % B] = 1.0
  got = _run(dev, clips, caps, nc, ns, reduce)
  assert (got[3] == 0).all() and (got[7] == 0).all()
  want = [t.cpu().numpy() for t in ops.group_rank(_dev(dev, clips), _dev(dev, caps), nc, ns, reduce)]
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[0])
  assert np.array_equal(got[4], want[2]) and np.array_equal(got[5], want[2])
  assert np.array_equal(got[2], want[1]) and np.array_equal(got[6], want[3])
  assert (got[0] == 1).all() and (got[4] == 1).all()       # the planted better match: ranks are not all zero
  _assert_ranks(got, block_scores(clips.astype(np.float64) @ caps.astype(np.float64).T, nc, ns, reduce))


# ---------------------------------------------------------------------------------------------
# 7: repeatability
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_two_calls_give_identical_bits(dev, reduce):
  clips, caps, nc, ns, _ = group_near_tie_fixture(34, 300, near_tie_seed(34, 300), 5, reduce)
  first = _run(dev, clips, caps, nc, ns, reduce)
  second = _run(dev, clips, caps, nc, ns, reduce)
  for a, b, name in zip(first, second, NAMES):
    assert np.array_equal(a, b), name


# ---------------------------------------------------------------------------------------------
# 8: evaluation.group_i2t_t2i_exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', REDUCES)
def test_group_i2t_t2i_exact_reports(dev, reduce):
  from cmhse_amd import evaluation
  n, d, max_rows = 22, 64, 5
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  clips, caps = clips.copy(), caps.copy()          # (writable: they go to torch.from_numpy as they are)
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(G64)
  raw = _run(dev, clips, caps, nc, ns, reduce)
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  for ties, want_v, want_p in (('optimistic', lo_v, lo_p), ('pessimistic', hi_v, hi_p)):
    (rep_v, top1_v, ranks_v), (rep_p, top1_p, ranks_p), info = evaluation.group_i2t_t2i_exact(
        clips, caps, nc, ns, reduce=reduce, ties=ties)
    for arr in (top1_v, ranks_v, top1_p, ranks_p):
      assert isinstance(arr, np.ndarray) and arr.dtype == np.float64
    assert np.array_equal(ranks_v, want_v) and np.array_equal(ranks_p, want_p)
    assert np.array_equal(top1_v, raw[2]) and np.array_equal(top1_p, raw[6])
    assert rep_v == evaluation.report_from_ranks(want_v.astype(np.float64))
    assert rep_p == evaluation.report_from_ranks(want_p.astype(np.float64))
    assert sorted(info) == ['p2v', 'resolved', 'v2p']
    for name, lo, hi, res in (('v2p', lo_v, hi_v, raw[3]), ('p2v', lo_p, hi_p, raw[7])):
      side = info[name]
      assert sorted(side) == ['report_hi', 'report_lo', 'resolved', 'tied_rows']
      assert side['report_lo'] == evaluation.report_from_ranks(lo.astype(np.float64))
      assert side['report_hi'] == evaluation.report_from_ranks(hi.astype(np.float64))
      assert np.array_equal(side['tied_rows'], np.flatnonzero(lo < hi)) and len(side['tied_rows']) == 2 * n
      assert side['resolved'] == int(res.sum())
    assert info['resolved'] == int(raw[3].sum()) + int(raw[7].sum())
    # device tensors in: ranks and top1 stay on the device, the same values and reports
    c, s = _dev(dev, clips), _dev(dev, caps)
    (drep_v, dtop1_v, dranks_v), (drep_p, dtop1_p, dranks_p), dinfo = evaluation.group_i2t_t2i_exact(
        c, s, nc, ns, reduce=reduce, ties=ties)
    for t in (dtop1_v, dranks_v, dtop1_p, dranks_p):
      assert t.is_cuda and t.dtype == torch.int32
    assert drep_v == rep_v and drep_p == rep_p and dinfo['resolved'] == info['resolved']
    assert np.array_equal(dranks_v.cpu().numpy(), want_v) and np.array_equal(dranks_p.cpu().numpy(), want_p)
    assert np.array_equal(dtop1_v.cpu().numpy(), raw[2]) and np.array_equal(dtop1_p.cpu().numpy(), raw[6])
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(clips, caps, nc, ns, reduce=reduce, ties='both')
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(clips, caps, nc, ns, reduce='median')


# ---------------------------------------------------------------------------------------------
# 9: a mid-size split
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_size_inputs():
  from cmhse_amd import synthetic
  B, d = 1024, 1024
  nc = np.asarray(synthetic.anet_like_spec(B).num_clips)
  ns = np.asarray(synthetic.anet_like_spec(B, seed=1).num_clips)
  a, b = synthetic.correlated_embeddings(B, d, seed=5)
  rng = np.random.RandomState(6)
  clips = (np.repeat(a, nc, axis=0) + 0.005 * rng.standard_normal((int(nc.sum()), d))).astype(np.float32)
  caps = (np.repeat(b, ns, axis=0) + 0.005 * rng.standard_normal((int(ns.sum()), d))).astype(np.float32)
  S64 = clips.astype(np.float64) @ caps.astype(np.float64).T
  scale = float(np.linalg.norm(clips.astype(np.float64), axis=1).max() *
                np.linalg.norm(caps.astype(np.float64), axis=1).max())
  return clips, caps, nc, ns, S64, scale


@pytest.mark.parametrize('reduce', REDUCES)
def test_mid_size_split(dev, reduce):
  clips, caps, nc, ns, S64, scale = _mid_size_inputs()
  G64 = block_scores(S64, nc, ns, reduce)
  gaps = group_min_gaps(G64)
  assert min(gaps) > GROUP_GAP * scale
  assert 4 * float64_noise(S64, nc, ns, clips.shape[1], reduce, scale) < GROUP_GAP * scale
  got = _run(dev, clips, caps, nc, ns, reduce)
  print('mid-size %s: %d clip x %d caption rows, min gaps %.3g / %.3g, resolved %d + %d of %d blocks'
        % (reduce, len(clips), len(caps), gaps[0], gaps[1], got[3].sum(), got[7].sum(), 1024 * 1023))
  _assert_ranks(got, G64)
  assert got[0].max() > 0 and got[4].max() > 0 and np.median(got[0]) < 1024 / 4      # non-trivial ranks
