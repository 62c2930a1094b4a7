"""Certified group-wise ranking without a GPU: a NumPy statement of cmhse_group_rank_exact's contract and the
group-structured near-tie fixture that the GPU tests (test_gpu_group_rank_exact.py) import, the tolerance
function against the textbook bound, and the C ABI's workspace size and argument validation
(include/cmhse_hip.h)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

ERR_ARG, ERR_WORKSPACE = -1, -2

# Every gap between a query's own float64 block score and another group's that the fixtures rely on exceeds
# this.  A float64 dot product of unit rows is within D 2^-53 |a| |b| of the true one whatever its summation
# order: 1.14e-13 at D = 1024.  Two implementations compare two such scores each, so their comparisons agree
# once the gap exceeds 4 of these; GROUP_GAP is above 8 (9.1e-13).  Under 'mean' the sequential float64 sum of a
# block adds at most (n - 1) 2^-53 mean |s64| to each side, which float64_noise() adds in, block by block, and the
# fixtures assert 4 x the total stays below GROUP_GAP (unit rows; the un-normalised GPU cases scale both).
GROUP_GAP = 1e-12


def _offsets(counts):
  off = np.zeros(len(counts) + 1, dtype=np.int64)
  np.cumsum(counts, out=off[1:])
  return off


def block_scores(S, num_clips, num_caps, reduce):
  """The block reduction of the contract on a stored clip x caption matrix, in float64: the block maximum, or the
  block's entries added sequentially in float64, clip-major then caption, divided by float64(count).  (A float32
  S gives cmhse_group_scores' G once the result is rounded to float32.)"""
  S = np.asarray(S)
  nc, ns = np.asarray(num_clips, dtype=np.int64), np.asarray(num_caps, dtype=np.int64)
  oc, os_ = _offsets(nc), _offsets(ns)
  if reduce == 'max':
    return np.maximum.reduceat(np.maximum.reduceat(S, oc[:-1], axis=0), os_[:-1], axis=1).astype(np.float64)
  acc = np.zeros((len(nc), len(ns)), dtype=np.float64)
  for rl in range(int(nc.max())):            # clip-major, then caption: every block advances in its own order
    vi = np.flatnonzero(nc > rl)
    for cl in range(int(ns.max())):
      pj = np.flatnonzero(ns > cl)
      acc[np.ix_(vi, pj)] += S[np.ix_(oc[vi] + rl, os_[pj] + cl)]
  return acc / (nc[:, None] * ns[None, :]).astype(np.float64)


def float64_noise(S64, num_clips, num_caps, d, reduce, scale=1.0):
  """An upper bound on how far a float64 implementation of G64 (any dot product order; the contract's block
  order) can be from the true block score: D 2^-53 |a| |b| (`scale` = the largest |a| |b|) and, under 'mean',
  the sequential sum's (n - 1) 2^-53 mean |s64| of the worst block."""
  e = d * 2.0 ** -53 * scale * 1.0001
  if reduce == 'mean':
    n = (np.asarray(num_clips)[:, None] * np.asarray(num_caps)[None, :]).astype(np.float64)
    e += float(((n - 1) * 2.0 ** -53 * block_scores(np.abs(S64), num_clips, num_caps, 'mean')).max())
  return e


def group_exact_reference(G64):
  """cmhse_group_rank_exact's contract from the float64 block scores G64 [B, B] (video i, paragraph j):
  (rank_lo_v2p, rank_hi_v2p, rank_lo_p2v, rank_hi_p2v) — per row (query = video) and per column (query =
  paragraph) the other entries strictly above / at or above the diagonal one."""
  G = np.asarray(G64, dtype=np.float64)
  d = np.diag(G)
  off = ~np.eye(len(G), dtype=bool)
  return (np.count_nonzero((G > d[:, None]) & off, axis=1), np.count_nonzero((G >= d[:, None]) & off, axis=1),
          np.count_nonzero((G > d[None, :]) & off, axis=0), np.count_nonzero((G >= d[None, :]) & off, axis=0))


def group_min_gaps(G64, skip=None):
  """The smallest |G[q, k] - G[q, q]| over k != q per direction (v2p, p2v); skip [B, B] bool masks (q, k) pairs
  of the v2p view (its transpose serves p2v: entry [i, j] is the pair of query j and video i there)."""
  G = np.asarray(G64, dtype=np.float64)
  d = np.diag(G)
  out = []
  for gap in (np.abs(G - d[:, None]), np.abs(G - d[None, :])):
    gap[np.eye(len(G), dtype=bool)] = np.inf
    if skip is not None:
      gap[skip] = np.inf
    out.append(float(gap.min()) if gap.size > 1 else np.inf)
  return out


def _unit(x):
  return x / np.linalg.norm(x, axis=1, keepdims=True)


def _near_copy(rows, counts, ulps, rng):
  """Every row's largest coordinate moved by `ulps` ulps, one random sign per group."""
  c = rows.copy()
  bits = c.view(np.int32)                  # (sign-magnitude: adding to the integer moves the magnitude)
  sign = np.repeat(rng.choice([-1, 1], size=len(counts)), counts).astype(np.int32)
  big = np.abs(rows).argmax(axis=1)
  bits[np.arange(len(rows)), big] += ulps * sign
  return c


def fp32_group_ranks(clips, caps, num_clips, num_caps, reduce):
  """(rank_v2p, rank_p2v) of NumPy's fp32 scores reduced as cmhse_group_scores does: one fp32 summation order."""
  G32 = block_scores(clips @ caps.T, num_clips, num_caps, reduce).astype(np.float32).astype(np.float64)
  lo_v, _, lo_p, _ = group_exact_reference(G32)
  return lo_v, lo_p


@functools.lru_cache(maxsize=None)
def group_near_tie_fixture(n, d, seed, max_rows, reduce):
  """(clips fp32 [6 Nc, d], caps fp32 [6 Ns, d], num_clips [6 n], num_caps [6 n], G64 float64 [6 n, 6 n]) — not
  to be modified (cached).  n base videos of 1 .. max_rows unit-norm clip rows; paragraph v has an independently
  drawn 1 .. max_rows captions, each a clip of video v plus 0.3 noise / sqrt(d), renormalised: distinct rows.
  Six families of videos and of paragraphs: the base, four near-copies (every row's largest coordinate moved by
  1 / 2 / 8 / 64 ulps, one random sign per group) and the base again, so B = 6 n on both sides, every query of
  families 0 and 5 has one bit-identical duplicate and four neighbours below fp32 resolution.  The float64
  clip x caption matrix is computed from the five distinct families and then gathered, so duplicates are
  bit-equal in it whatever BLAS does.  Asserts its validity: every gap outside the planted duplicates exceeds
  GROUP_GAP, and GROUP_GAP exceeds 4 x float64_noise()."""
  rng = np.random.RandomState(seed)
  nc = rng.randint(1, max_rows + 1, size=n)
  ns = rng.randint(1, max_rows + 1, size=n)
  clips = _unit(rng.standard_normal((int(nc.sum()), d))).astype(np.float32)
  oc = _offsets(nc)
  src = np.concatenate([oc[v] + rng.randint(0, nc[v], size=ns[v]) for v in range(n)])
  caps = clips[src].astype(np.float64) + 0.3 * rng.standard_normal((len(src), d)) / np.sqrt(d)
  caps = _unit(caps).astype(np.float32)
  cfam = [clips] + [_near_copy(clips, nc, u, rng) for u in (1, 2, 8, 64)]
  sfam = [caps] + [_near_copy(caps, ns, u, rng) for u in (1, 2, 8, 64)]
  Cd, Sd = np.concatenate(cfam), np.concatenate(sfam)
  rmap = np.concatenate([np.arange(len(Cd)), np.arange(len(clips))])
  cmap = np.concatenate([np.arange(len(Sd)), np.arange(len(caps))])
  S64 = (Cd.astype(np.float64) @ Sd.astype(np.float64).T)[np.ix_(rmap, cmap)]
  num_clips, num_caps = np.tile(nc, 6), np.tile(ns, 6)
  G64 = block_scores(S64, num_clips, num_caps, reduce)
  B = 6 * n
  dup = np.zeros((B, B), dtype=bool)        # (query q, its duplicate): families 0 and 5 of the same base group
  dup[np.arange(n), 5 * n + np.arange(n)] = dup[5 * n + np.arange(n), np.arange(n)] = True
  gaps = group_min_gaps(G64, skip=dup)
  assert min(gaps) > GROUP_GAP, (n, d, seed, max_rows, reduce, gaps)
  assert 4 * float64_noise(S64, num_clips, num_caps, d, reduce) < GROUP_GAP
  assert np.array_equal(G64[:, :n], G64[:, 5 * n:]) and np.array_equal(G64[:n], G64[5 * n:])
  out = (np.ascontiguousarray(Cd[rmap]), np.ascontiguousarray(Sd[cmap]), num_clips, num_caps, G64)
  for a in out:
    a.setflags(write=False)
  return out


# (n, d, max_rows): small groups at aligned, unaligned and full-width D, and groups up to the 128-row limit
GROUP_NEAR_TIE_SHAPES = [(22, 64, 5), (22, 50, 5), (44, 1024, 5), (34, 300, 5), (4, 96, 100), (3, 1024, 128)]
REDUCES = ['max', 'mean']


def near_tie_seed(n, d):
  return 7 * n + d


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


# ---------------------------------------------------------------------------------------------
# the contract and the fixture
# ---------------------------------------------------------------------------------------------
def test_reference_on_a_hand_written_matrix():
  G = np.array([[2.0, 3.0, 2.0, 1.0],
                [0.0, 0.0, 0.0, 0.0],
                [5.0, 4.0, 3.0, 9.0],
                [2.0, 0.0, 9.0, 2.0]])
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(G)
  assert lo_v.tolist() == [1, 0, 3, 1] and hi_v.tolist() == [2, 3, 3, 2]
  # columns: [2, 0, 5, 2] vs 2; [3, 0, 4, 0] vs 0; [2, 0, 3, 9] vs 3; [1, 0, 9, 2] vs 2
  assert lo_p.tolist() == [1, 2, 1, 1] and hi_p.tolist() == [2, 3, 1, 1]
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(np.array([[7.0]]))
  assert lo_v.tolist() == hi_v.tolist() == lo_p.tolist() == hi_p.tolist() == [0]
  # tie-free: both are the position of the diagonal in the descending sort, per row and per column
  R = np.random.RandomState(0).standard_normal((30, 30))
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(R)
  assert np.array_equal(lo_v, hi_v) and np.array_equal(lo_p, hi_p)
  assert lo_v.tolist() == [int(np.flatnonzero(np.argsort(-R[i]) == i)[0]) for i in range(30)]
  assert lo_p.tolist() == [int(np.flatnonzero(np.argsort(-R[:, j]) == j)[0]) for j in range(30)]


def test_block_scores_order_and_values():
  rng = np.random.RandomState(3)
  nc, ns = [2, 1, 3], [1, 3, 2]
  S = rng.standard_normal((6, 6))
  oc, os_ = _offsets(nc), _offsets(ns)
  for i in range(3):
    for j in range(3):
      blk = S[oc[i]:oc[i + 1], os_[j]:os_[j + 1]]
      assert block_scores(S, nc, ns, 'max')[i, j] == blk.max()
      assert block_scores(S, nc, ns, 'mean')[i, j] == np.cumsum(blk.ravel())[-1] / blk.size    # sequential


@pytest.mark.parametrize('reduce', REDUCES)
@pytest.mark.parametrize('n,d,max_rows', GROUP_NEAR_TIE_SHAPES)
def test_group_near_tie_fixture(n, d, max_rows, reduce):
  clips, caps, nc, ns, G64 = group_near_tie_fixture(n, d, near_tie_seed(n, d), max_rows, reduce)
  B = 6 * n
  assert clips.dtype == np.float32 and caps.dtype == np.float32 and G64.shape == (B, B)
  assert len(nc) == len(ns) == B and clips.shape == (nc.sum(), d) and caps.shape == (ns.sum(), d)
  assert nc.max() <= max_rows and ns.max() <= max_rows and not np.array_equal(nc, ns)
  Nc, Ns = len(clips) // 6, len(caps) // 6
  assert np.array_equal(clips[:Nc], clips[5 * Nc:]) and np.array_equal(caps[:Ns], caps[5 * Ns:])
  for f in range(1, 5):
    assert (np.count_nonzero(clips[f * Nc:(f + 1) * Nc] != clips[:Nc], axis=1) == 1).all()
    assert (np.count_nonzero(caps[f * Ns:(f + 1) * Ns] != caps[:Ns], axis=1) == 1).all()
  assert len(np.unique(caps[:Ns], axis=0)) == Ns                   # distinct caption rows
  lo_v, hi_v, lo_p, hi_p = group_exact_reference(G64)
  tied = np.zeros(B, dtype=np.int64)
  tied[:n] = tied[5 * n:] = 1                                      # the duplicate, and nothing else
  assert np.array_equal(hi_v - lo_v, tied) and np.array_equal(hi_p - lo_p, tied)
  # what makes the fixture discriminate: fp32 scores rank these groups differently
  r32_v, r32_p = fp32_group_ranks(clips, caps, nc, ns, reduce)
  differ = np.count_nonzero(r32_v != lo_v), np.count_nonzero(r32_p != lo_p)
  dup = np.zeros((B, B), dtype=bool)
  dup[np.arange(n), 5 * n + np.arange(n)] = dup[5 * n + np.arange(n), np.arange(n)] = True
  print('group near-tie n=%d d=%d rows<=%d %s: min gaps %.3g / %.3g, NumPy-fp32 ranks differ on %d / %d of %d queries'
        % ((n, d, max_rows, reduce) + tuple(group_min_gaps(G64, skip=dup)) + differ + (B,)))
  assert differ[0] > 0 and differ[1] > 0


# ---------------------------------------------------------------------------------------------
# the tolerance
# ---------------------------------------------------------------------------------------------
DS = (1, 8, 30, 1024, 4096)
NORMS = (1e-3, 1.0, 32.0)
MAX, MEAN = 1, 0


def test_tolerance_against_the_textbook_value(lib):
  tol = lib.cmhse_group_rank_exact_tolerance
  for D in DS:
    for na in NORMS:
      for nb in NORMS:
        for reduce, terms in ((MAX, D), (MEAN, D + 1)):
          textbook = 2.0 * terms * 2.0 ** -24 * na * nb
          t = tol(D, reduce, na, nb)
          assert t >= textbook, (D, reduce, na, nb, t, textbook)
          assert t <= 1.1 * textbook, (D, reduce, na, nb, t, textbook)   # no vacuous "everything is undecided"
        assert tol(D, MEAN, na, nb) > tol(D, MAX, na, nb)
        assert tol(D, MAX, na, nb) == lib.cmhse_sim_rank_exact_tolerance(D, na, nb)


def test_tolerance_is_monotone(lib):
  tol = lib.cmhse_group_rank_exact_tolerance
  for reduce in (MAX, MEAN):
    for na in NORMS:
      for nb in NORMS:
        vals = [tol(D, reduce, na, nb) for D in DS]
        assert all(a < b for a, b in zip(vals, vals[1:]))
    for D in DS:
      for fixed in NORMS:
        a = [tol(D, reduce, x, fixed) for x in NORMS]
        b = [tol(D, reduce, fixed, x) for x in NORMS]
        assert all(x < y for x, y in zip(a, a[1:])) and all(x < y for x, y in zip(b, b[1:]))
    assert 0.0 < tol(64, reduce, 0.0, 1.0) < 1e-40                  # the underflow term alone
    assert np.isnan(tol(0, reduce, 1.0, 1.0)) and np.isnan(tol(8, reduce, -1.0, 1.0))
    assert np.isnan(tol(8, reduce, 1.0, -1.0)) and np.isnan(tol(8, reduce, float('nan'), 1.0))
    assert np.isinf(tol(1 << 24, reduce, 1.0, 1.0))
  assert np.isnan(tol(8, 2, 1.0, 1.0)) and np.isnan(tol(8, -1, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_workspace_size(lib):
  ws = lib.cmhse_group_rank_exact_workspace
  for bad in [(0, 5, 5), (-1, 5, 5), (3, 2, 5), (3, 5, 2), (3, 0, 0), (3, -7, 9)]:
    assert ws(*bad) == 0, bad
  prev = 0
  for B in (1, 2, 63, 64, 65, 128, 129, 1000, 4917):
    b = ws(B, 4 * B, 3 * B)
    assert b > 0 and b % 256 == 0 and b >= prev
    base = lib.cmhse_group_rank_workspace(B)
    assert b >= base + 16 * B + 8 * 7 * B                 # cmhse_group_rank's regions and the new vectors
    assert b <= base + 16 * B + 8 * 7 * B + 7 * 256
    assert ws(B, 4 * B + 1000, 3 * B) >= b and ws(B, 4 * B, 3 * B + 1000) >= b     # monotone in the rows too
    prev = b


def _plan(lib, clips, caps):
  B = len(clips)
  oc, os_ = _offsets(clips).astype(np.int32), _offsets(caps).astype(np.int32)
  plan = np.zeros(4 * B + 9, dtype=np.int32)
  n = lib.cmhse_group_plan(oc.ctypes.data, os_.ctypes.data, B, plan.ctypes.data, plan.size)
  assert n > 0
  return plan[:n].copy()


def test_argument_validation_without_gpu(lib):
  """Every error of cmhse_group_rank_exact is returned before anything touches the device."""
  plan = _plan(lib, [2, 1, 3], [1, 1, 2])
  n = len(plan)
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = lib.cmhse_group_rank_exact_workspace(3, 6, 4)
  assert ws_ok > 0
  outs = ['lo_v', 'hi_v', 'top1_v', 'res_v', 'lo_p', 'hi_p', 'top1_p', 'res_p']
  good = dict(C=fake, S=fake, Nc=6, Ns=4, D=8, B=3, ph=plan.ctypes.data, pd=fake, plen=n, reduce=1,
              ws=ctypes.c_void_p(1 << 20), ws_bytes=0)
  good.update((o, fake) for o in outs)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_rank_exact(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['B'], a['ph'], a['pd'],
                                      a['plen'], a['reduce'], *([a[o] for o in outs] + [a['ws'], a['ws_bytes'], None]))

  # (the valid arguments with no workspace: past every argument check, stopped by the workspace check)
  assert call() == ERR_WORKSPACE
  assert call(reduce=0) == ERR_WORKSPACE
  bads = [dict(C=None), dict(S=None), dict(ph=None), dict(pd=None), dict(ws=None), dict(Nc=7), dict(Ns=3),
          dict(Nc=0), dict(Ns=0), dict(D=0), dict(D=-1), dict(B=2), dict(B=0), dict(plen=n - 1),
          dict(plen=n + 1), dict(reduce=2), dict(reduce=-1)] + [{o: None} for o in outs]
  for bad in bads:
    assert call(**bad) == ERR_ARG, bad                      # before the workspace check ...
    assert call(ws_bytes=ws_ok, **bad) == ERR_ARG, bad      # ... and with a workspace that would pass it
  assert call(ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=ws_ok) == ERR_WORKSPACE    # not 256-byte aligned
  assert call(ws_bytes=ws_ok - 1) == ERR_WORKSPACE                                      # too small
  assert call(ws_bytes=lib.cmhse_group_rank_workspace(3)) == ERR_WORKSPACE              # cmhse_group_rank's
  # a host plan whose tiles were edited: rejected (the kernels trust its bounds)
  for idx, val in [(5, 1), (7, 0), (3, 4), (5 + 2 * 4 + 1, 1)]:
    edited = plan.copy()
    edited[idx] = val
    assert call(ph=edited.ctypes.data, ws_bytes=ws_ok) == ERR_ARG, (idx, val)
  # a group of more than 128 rows never gets a plan: cmhse_group_plan's CMHSE_ERR_UNSUPPORTED
  oc, os_ = _offsets([3, 129]).astype(np.int32), _offsets([1, 1]).astype(np.int32)
  buf = np.zeros(17, dtype=np.int32)
  assert lib.cmhse_group_plan(oc.ctypes.data, os_.ctypes.data, 2, buf.ctypes.data, buf.size) == -4


def test_ops_and_evaluation_argument_errors():
  from cmhse_amd import evaluation, ops
  c, s = torch.zeros(6, 4), torch.zeros(4, 4)
  for kw in [dict(num_clips=[2, 0, 4]), dict(num_clips=[2, 1, 2]), dict(num_clips=[2, 1, 3], num_caps=[1, 1]),
             dict(num_clips=[2, 1, 3], num_caps=[1, 1, 1]), dict(num_clips=[2, 1, 3], reduce='sum'),
             dict(num_clips=[]), dict(num_clips=[2, 1.5, 2.5])]:
    args = dict(num_caps=[1, 1, 2], reduce='max')
    args.update(kw)
    with pytest.raises(ValueError):
      ops.group_rank_exact(c, s, **args)
    with pytest.raises(ValueError):
      evaluation.group_i2t_t2i_exact(c.numpy(), s.numpy(), **args)
  with pytest.raises(ValueError):
    ops.group_rank_exact(torch.zeros(130, 4), torch.zeros(2, 4), [129, 1], [1, 1])
  with pytest.raises(ValueError):
    ops.group_rank_exact(torch.zeros(6, 4), torch.zeros(4, 5), [2, 1, 3], [1, 1, 2])
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(c.numpy(), s.numpy(), [2, 1, 3], [1, 1, 2], ties='neither')
  with pytest.raises(ValueError):
    evaluation.group_i2t_t2i_exact(c.numpy(), s.numpy(), [2, 1, 3])          # num_caps = num_clips: 6 != 4 rows


def test_needs_device_tensors_and_dropin_reexport():
  from cmhse_amd import evaluation, ops
  from cmhse_amd.dropin import evaluation as dropin
  with pytest.raises(RuntimeError):
    ops.group_rank_exact(torch.zeros(6, 4), torch.zeros(4, 4), [2, 1, 3], [1, 1, 2])
  assert dropin.group_i2t_t2i_exact is evaluation.group_i2t_t2i_exact
