"""Labelled group-wise ranking without a GPU: the plan of cmhse_group_rank_labelled_plan (tiles, labels, pair
tiles), the workspace size, argument validation (include/cmhse_hip.h), the ValueErrors of
ops.group_rank_labelled / evaluation.group_rank_labelled / evaluation.group_i2t_t2i_labelled, and the label
handling of the front end on a NumPy stand-in.  The GPU tests (test_gpu_group_rank_labelled.py) import the
NumPy statement of the contract and their label sets from here; this file proves that those cases reach the
code paths they are meant to reach (several pair tiles per query, more than one panel, the query cap)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_rank_labelled_cpu import labelled_reference, random_labels

HDR = 10                # group.hip kGlHdr
QCAP = 72               # group.hip kGlQcap: query groups per query tile
P2V, V2P = 0, 1
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -4
DIRECTION = {'p2v': P2V, 'v2p': V2P}


# ---------------------------------------------------------------------------------------------
# the contract and the label sets the GPU tests use
# ---------------------------------------------------------------------------------------------
def group_labelled_reference(G, direction, off, idx):
  """cmhse_group_rank_labelled's contract on a stored G [Bv, Bp] (video, paragraph): labelled_reference
  on the queries' lines — the columns for 'p2v' (query = paragraph), the rows for 'v2p'."""
  G = np.asarray(G, dtype=np.float32)
  return labelled_reference(np.ascontiguousarray(G.T) if direction == 'p2v' else G, off, idx)


MANY = 40               # the positives of the one query whose pairs span several pair tiles


def rect_labels(seed, Bq, Bg, many_at=None):
  """1..5 random positives per query with duplicates (random_labels); query `many_at` gets MANY positives."""
  rng = np.random.RandomState(seed)
  off, idx = random_labels(rng, Bq, Bg, 1, 5)
  if many_at is None:
    return off, idx
  lists = [idx[off[q]:off[q + 1]] for q in range(Bq)]
  lists[many_at] = rng.randint(0, Bg, size=MANY)
  counts = np.array([len(x) for x in lists])
  off = np.zeros(Bq + 1, dtype=np.int64)
  np.cumsum(counts, out=off[1:])
  return off, np.concatenate(lists)


def rect_counts(seed=29):
  """The rectangular problem of the GPU tests: 700 videos x 500 paragraphs, counts 1..19."""
  rng = np.random.RandomState(seed)
  return [int(x) for x in rng.randint(1, 20, 700)], [int(x) for x in rng.randint(1, 20, 500)]


def panel_case():
  """40 queries of 1..6 rows against 3000 gallery groups of 1..6 rows: (query counts, gallery counts)."""
  rng = np.random.RandomState(31)
  return [int(x) for x in rng.randint(1, 7, 40)], [int(x) for x in rng.randint(1, 7, 3000)]


def cap_case():
  """600 one-row query groups against 50 gallery groups of 1..6 rows."""
  rng = np.random.RandomState(37)
  return [1] * 600, [int(x) for x in rng.randint(1, 7, 50)]


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def _offsets(counts):
  off = np.zeros(len(counts) + 1, dtype=np.int32)
  np.cumsum(counts, out=off[1:])
  return off


def _plan_max(Bv, Bp, n_pairs):
  return 3 * Bv + 3 * Bp + 2 * n_pairs + 16


def _plan(lib, clips, caps, direction, off, idx, cap=None):
  Bv, Bp = len(clips), len(caps)
  oc, op = _offsets(clips), _offsets(caps)
  off = np.ascontiguousarray(off, dtype=np.int32)
  idx = np.ascontiguousarray(idx, dtype=np.int32)
  plan = np.full(_plan_max(Bv, Bp, idx.size) if cap is None else cap, -7, dtype=np.int32)
  n = lib.cmhse_group_rank_labelled_plan(oc.ctypes.data, Bv, op.ctypes.data, Bp, direction, off.ctypes.data,
                                         idx.ctypes.data, idx.size, plan.ctypes.data, plan.size)
  return n, plan


def _parts(plan):
  Bv, Bp, _, _, direction, R, C, n_pairs, T, _ = (int(x) for x in plan[:HDR])
  Bq = Bp if direction == P2V else Bv
  sizes = [Bv + 1, Bp + 1, R + 1, C + 1, Bq + 1, n_pairs, T + 1]
  cuts = HDR + np.concatenate([[0], np.cumsum(sizes)])
  names = ('clip_off', 'cap_off', 'rt', 'ct', 'pos_off', 'pos_idx', 'pt')
  out = {name: plan[cuts[k]:cuts[k + 1]] for k, name in enumerate(names)}
  out['len'] = int(cuts[-1])
  return out


def _check_tiling(off, start, B, max_groups):
  assert start[0] == 0 and start[-1] == B
  assert (np.diff(start) > 0).all()                       # every group whole in exactly one tile, in order
  rows = off[start[1:]] - off[start[:-1]]
  assert (rows <= 128).all() and (rows >= 1).all()        # no tile holds more than 128 rows
  assert rows.sum() == off[B]                             # the tiles cover every row, in order
  assert (np.diff(start) <= max_groups).all()             # the query side's group cap
  for t in range(len(start) - 2):                         # greedy: the next group would not have fitted
    nxt = start[t + 1]
    assert off[nxt + 1] - off[start[t]] > 128 or nxt - start[t] >= max_groups


def _pair_rows(parts, direction):
  """(clip rows, caption rows) of every pair, in CSR order."""
  off, idx = parts['pos_off'].astype(np.int64), parts['pos_idx'].astype(np.int64)
  query = np.repeat(np.arange(off.size - 1), np.diff(off))
  vid, par = (idx, query) if direction == P2V else (query, idx)
  return np.diff(parts['clip_off'])[vid], np.diff(parts['cap_off'])[par]


def _check_pair_tiles(parts, direction):
  pt = parts['pt']
  n_pairs = parts['pos_idx'].size
  assert pt[0] == 0 and pt[-1] == n_pairs and (np.diff(pt) > 0).all()   # every pair in exactly one tile, in order
  rv, rp = _pair_rows(parts, direction)
  for t in range(pt.size - 1):
    a, b = int(pt[t]), int(pt[t + 1])
    assert rv[a:b].sum() <= 128 and rp[a:b].sum() <= 128               # both sides of the tile
    if b < n_pairs:                                                     # greedy: the next pair would not have fitted
      assert rv[a:b + 1].sum() > 128 or rp[a:b + 1].sum() > 128


def _check_plan(lib, clips, caps, direction, off, idx):
  n, plan = _plan(lib, clips, caps, direction, off, idx)
  assert n > 0, n
  Bv, Bp = len(clips), len(caps)
  assert list(plan[:5]) == [Bv, Bp, sum(clips), sum(caps), direction]
  assert int(plan[7]) == len(idx) and int(plan[9]) == QCAP
  parts = _parts(plan)
  assert n == parts['len'] <= _plan_max(Bv, Bp, len(idx))
  assert (plan[n:] == -7).all()                           # nothing written past the returned length
  assert np.array_equal(parts['clip_off'], _offsets(clips)) and np.array_equal(parts['cap_off'], _offsets(caps))
  assert np.array_equal(parts['pos_off'], off) and np.array_equal(parts['pos_idx'], idx)
  big = 1 << 30
  _check_tiling(parts['clip_off'], parts['rt'], Bv, QCAP if direction == V2P else big)
  _check_tiling(parts['cap_off'], parts['ct'], Bp, QCAP if direction == P2V else big)
  _check_pair_tiles(parts, direction)
  return plan[:n]


def _sizes(direction, Bv, Bp):
  return (Bp, Bv) if direction == P2V else (Bv, Bp)


# ---------------------------------------------------------------------------------------------
# the header and the bindings
# ---------------------------------------------------------------------------------------------
def test_header_constants_match_lib():
  from cmhse_amd import _lib
  header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             'include', 'cmhse_hip.h')).read()
  assert ('#define CMHSE_GROUP_RANK_LABELLED_PLAN_MAX(Bv, Bp, n_pairs) '
          '(3 * (Bv) + 3 * (Bp) + 2 * (n_pairs) + 16)') in header
  assert _lib.group_rank_labelled_plan_max(10, 7, 30) == _plan_max(10, 7, 30) == 127
  assert (_lib.GROUP_P2V, _lib.GROUP_V2P) == (P2V, V2P)
  for name in ('cmhse_group_rank_labelled_plan', 'cmhse_group_rank_labelled_workspace',
               'cmhse_group_rank_labelled'):
    assert name in _lib.SIGNATURES and ' %s(' % name in header
  assert len(_lib.SIGNATURES['cmhse_group_rank_labelled'][1]) == 17
  assert 'at 72' in header                                # the query cap the header states


def test_dropin_reexports():
  from cmhse_amd.dropin import evaluation as dropin
  from cmhse_amd import evaluation
  for name in ('group_rank_labelled', 'group_i2t_t2i_labelled'):
    assert getattr(dropin, name) is getattr(evaluation, name)


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('direction', [P2V, V2P])
@pytest.mark.parametrize('seed,Bv,Bp,hi', [(0, 1, 1, 5), (1, 7, 40, 40), (2, 300, 120, 30), (3, 500, 700, 128),
                                           (4, 4917, 2000, 6), (5, 900, 900, 2), (6, 200, 300, 2)])
def test_plan_invariants_random_counts(lib, direction, seed, Bv, Bp, hi):
  rng = np.random.RandomState(seed)
  clips = rng.randint(1, hi + 1, size=Bv)
  caps = rng.randint(1, hi + 1, size=Bp)
  Bq, Bg = _sizes(direction, Bv, Bp)
  off, idx = random_labels(rng, Bq, Bg, 1, 5)
  _check_plan(lib, clips, caps, direction, off, idx)


@pytest.mark.parametrize('direction', [P2V, V2P])
def test_plan_val1_profile_diagonal(lib, direction):
  from cmhse_amd import synthetic
  nclips = np.asarray(synthetic.anet_like_spec(4917).num_clips)
  assert nclips.sum() == 17502
  plan = _check_plan(lib, nclips, nclips, direction, np.arange(4918), np.arange(4917))
  R, C, T = int(plan[5]), int(plan[6]), int(plan[8])
  assert R <= 145 and C <= 145                            # both sides pack as cmhse_group_plan does: the cap is idle
  assert T == R                                           # diagonal pairs with equal counts: the row tiles again


def test_plan_all_ones_hits_the_cap(lib):
  ones = [1] * 1000
  plan = _check_plan(lib, ones, ones, P2V, np.arange(1001), np.arange(1000))
  parts = _parts(plan)
  assert set(np.diff(parts['ct'])[:-1]) == {QCAP}         # query tiles: full at the cap
  assert set(np.diff(parts['rt'])[:-1]) == {128}          # gallery tiles: full at 128 rows
  assert set(np.diff(parts['pt'])[:-1]) == {128}          # pair tiles: 128 one-row pairs
  parts = _parts(_check_plan(lib, ones, ones, V2P, np.arange(1001), np.arange(1000)))
  assert set(np.diff(parts['rt'])[:-1]) == {QCAP} and set(np.diff(parts['ct'])[:-1]) == {128}


def test_pair_tiles_of_a_query_with_long_positives(lib):
  """One paragraph whose positives are videos of 128 + 128 + 1 clips: three pair tiles, the caption side far
  from its limit; the next query's pair joins the last of them."""
  clips, caps = [128, 3, 128, 1, 2], [4, 2]
  off, idx = [0, 3, 4], [0, 2, 3, 1]                      # paragraph 0: videos 0, 2, 3; paragraph 1: video 1
  parts = _parts(_check_plan(lib, clips, caps, P2V, off, idx))
  assert parts['pt'].tolist() == [0, 1, 2, 4]
  # the other way round: one video with paragraphs of 128 + 128 + 1 captions
  parts = _parts(_check_plan(lib, caps, clips, V2P, off, idx))
  assert parts['pt'].tolist() == [0, 1, 2, 4]
  # the caption side closes a tile as well: 40 paragraphs of 4 captions for one 1-clip video -> 32 a tile
  parts = _parts(_check_plan(lib, [1], [4] * 40, V2P, [0, 40], list(range(40))))
  assert parts['pt'].tolist() == [0, 32, 40]


def test_plan_errors(lib):
  clips, caps = [2, 1, 3], [1, 1, 2, 4]
  off, idx = [0, 1, 3, 4, 5], [0, 2, 2, 1, 0]             # p2v: 4 query paragraphs, 3 gallery videos
  assert _plan(lib, clips, caps, P2V, off, idx)[0] > 0
  assert _plan(lib, clips, caps, 2, off, idx)[0] == ERR_ARG                      # direction
  assert _plan(lib, clips, caps, -1, off, idx)[0] == ERR_ARG
  assert _plan(lib, clips, caps, V2P, off, idx)[0] == ERR_ARG                    # 3 queries that way: pos_off[3] != 5
  assert _plan(lib, [2, 0, 3], caps, P2V, off, idx)[0] == ERR_ARG                # bad prefix sums
  assert _plan(lib, clips, [1, -1, 2, 4], P2V, off, idx)[0] == ERR_ARG
  assert _plan(lib, clips, caps, P2V, [1, 1, 3, 4, 5], idx)[0] == ERR_ARG        # pos_off[0] != 0
  assert _plan(lib, clips, caps, P2V, [0, 1, 1, 4, 5], idx)[0] == ERR_ARG        # an empty list
  assert _plan(lib, clips, caps, P2V, [0, 2, 1, 4, 5], idx)[0] == ERR_ARG        # decreasing
  assert _plan(lib, clips, caps, P2V, [0, 1, 3, 4, 6], idx)[0] == ERR_ARG        # pos_off[Bq] != n_pairs
  assert _plan(lib, clips, caps, P2V, off, [0, 2, 3, 1, 0])[0] == ERR_ARG        # index == Bg
  assert _plan(lib, clips, caps, P2V, off, [0, 2, 2, -1, 0])[0] == ERR_ARG
  assert _plan(lib, clips, caps, V2P, [0, 1, 3, 4], [3, 0, 3, 2])[0] > 0         # index 3 is a paragraph this way
  assert _plan(lib, [3, 129, 2], caps, P2V, off, idx)[0] == ERR_UNSUPPORTED      # an oversize video
  assert _plan(lib, clips, [1, 1, 129, 4], P2V, off, idx)[0] == ERR_UNSUPPORTED
  assert _plan(lib, clips, caps, P2V, off, idx, cap=_plan_max(3, 4, 5) - 1)[0] == ERR_WORKSPACE
  # bad labels are reported before the oversize group and the capacity
  assert _plan(lib, [3, 129, 2], caps, P2V, off, [0, 2, 3, 1, 0], cap=1)[0] == ERR_ARG
  oc, op = _offsets(clips), _offsets(caps)
  o, x = np.array(off, dtype=np.int32), np.array(idx, dtype=np.int32)
  plan = np.zeros(64, dtype=np.int32)
  good = [oc.ctypes.data, 3, op.ctypes.data, 4, P2V, o.ctypes.data, x.ctypes.data, 5, plan.ctypes.data, 64]
  assert lib.cmhse_group_rank_labelled_plan(*good) > 0
  for k, bad in [(0, None), (2, None), (5, None), (6, None), (8, None), (1, 0), (3, 0), (1, -1), (7, 4), (7, 6),
                 (7, 3)]:
    args = list(good)
    args[k] = bad
    assert lib.cmhse_group_rank_labelled_plan(*args) == ERR_ARG, (k, bad)
  bad0 = np.array([1, 2, 3, 6], dtype=np.int32)                                  # does not start at 0
  args = list(good)
  args[0] = bad0.ctypes.data
  assert lib.cmhse_group_rank_labelled_plan(*args) == ERR_ARG


# ---------------------------------------------------------------------------------------------
# the workspace
# ---------------------------------------------------------------------------------------------
def _workspace(lib, plan):
  plan = np.ascontiguousarray(plan, dtype=np.int32)
  return lib.cmhse_group_rank_labelled_workspace(plan.ctypes.data, plan.size)


def _align(n):
  return (n + 255) // 256 * 256


def _workspace_at(Bq, panels):
  """One 8-byte threshold key per query; per panel one 4-byte count and one 8-byte key per query."""
  return _align(8 * Bq) + _align(4 * panels * Bq) + _align(8 * panels * Bq)


def _panels_of(lib, plan):
  ws, Bq = _workspace(lib, plan), int(plan[1] if plan[4] == P2V else plan[0])
  for P in range(1, 2000):
    if _workspace_at(Bq, P) == ws:
      return P
  raise AssertionError('workspace %d of %d queries is no panel count' % (ws, Bq))


def test_workspace_does_not_grow_with_the_gallery(lib):
  from cmhse_amd import synthetic
  queries = np.asarray(synthetic.anet_like_spec(4917).num_clips)
  rng = np.random.RandomState(9)
  sizes = {}
  for G in (5000, 1000000):
    videos = rng.randint(1, 7, size=G)
    off, idx = random_labels(rng, 4917, G, 1, 3)
    n, plan = _plan(lib, videos, queries, P2V, off, idx)
    assert n > 0
    sizes[G] = _workspace(lib, plan[:n])
    n, plan = _plan(lib, queries, videos, V2P, off, idx)
    assert n > 0
    assert _workspace(lib, plan[:n]) == sizes[G]          # the same query side, the other direction
  assert sizes[5000] == sizes[1000000] > 0                # nor does it grow with the pairs' rows
  assert sizes[5000] % 256 == 0
  assert sizes[5000] >= 4917 * (8 + 4 + 8)
  # far from the Bq x Bg matrix cmhse_group_rank stores: under 1/10 of its workspace at B = 4917
  n, plan = _plan(lib, queries, queries, P2V, np.arange(4918), np.arange(4917))
  assert 0 < _workspace(lib, plan[:n]) < lib.cmhse_group_rank_workspace(4917) // 10
  assert _workspace(lib, plan[:n]) < 1 << 20


def test_workspace_shrinks_only_below_the_panel_count(lib):
  """A gallery of fewer tiles than panels gives one panel per tile."""
  rng = np.random.RandomState(10)
  off, idx = random_labels(rng, 40, 3, 1, 2)
  n, plan = _plan(lib, [128, 128, 128], [2] * 40, P2V, off, idx)
  assert _panels_of(lib, plan[:n]) == 3
  n, plan = _plan(lib, [128], [2] * 40, P2V, np.arange(41), [0] * 40)
  assert _panels_of(lib, plan[:n]) == 1


def test_workspace_of_invalid_plans_is_zero(lib):
  n, plan = _plan(lib, [2, 1, 3], [1, 1, 2, 4], P2V, [0, 1, 3, 4, 5], [0, 2, 2, 1, 0])
  plan = plan[:n].copy()
  assert _workspace(lib, plan) > 0
  assert lib.cmhse_group_rank_labelled_workspace(None, n) == 0
  assert lib.cmhse_group_rank_labelled_workspace(plan.ctypes.data, n - 1) == 0
  assert lib.cmhse_group_rank_labelled_workspace(plan.ctypes.data, HDR - 1) == 0
  parts = _parts(plan)
  first_idx = n - (parts['pt'].size + parts['pos_idx'].size)
  for at, val in [(4, 2), (9, QCAP - 1), (7, 4), (8, 0), (first_idx, 3), (first_idx, -1), (n - 1, 4)]:
    edited = plan.copy()
    edited[at] = val
    assert _workspace(lib, edited) == 0, (at, val)


# ---------------------------------------------------------------------------------------------
# the call's errors
# ---------------------------------------------------------------------------------------------
def test_call_argument_errors_without_gpu(lib):
  """Every error of cmhse_group_rank_labelled is returned before anything is launched."""
  clips, caps = [2, 1, 3], [1, 1, 2, 4]
  n, plan = _plan(lib, clips, caps, P2V, [0, 1, 3, 4, 5], [0, 2, 2, 1, 0])
  plan = plan[:n].copy()
  fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first
  ws_ok = _workspace(lib, plan)
  good = dict(C=fake, S=fake, Nc=6, Ns=8, D=8, ph=plan.ctypes.data, pd=fake, plen=n, direction=P2V, reduce=1,
              rank=fake, top1=fake, best_pos=fake, best_score=fake, ws=ctypes.c_void_p(1 << 20), ws_bytes=ws_ok)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cmhse_group_rank_labelled(a['C'], a['S'], a['Nc'], a['Ns'], a['D'], a['ph'], a['pd'], a['plen'],
                                         a['direction'], a['reduce'], a['rank'], a['top1'], a['best_pos'],
                                         a['best_score'], a['ws'], a['ws_bytes'], None)

  bads = [dict(C=None), dict(S=None), dict(ph=None), dict(pd=None), dict(rank=None), dict(top1=None),
          dict(best_pos=None), dict(ws=None), dict(Nc=7), dict(Ns=7), dict(Nc=0), dict(Ns=0), dict(D=0), dict(D=-1),
          dict(plen=n - 1), dict(plen=n + 1), dict(reduce=2), dict(reduce=-1),
          dict(direction=V2P), dict(direction=2)]              # the plan's direction is p2v
  for bad in bads:
    assert call(**bad) == ERR_ARG, bad
  assert call(ws=ctypes.c_void_p((1 << 20) + 16)) == ERR_WORKSPACE
  assert call(ws_bytes=ws_ok - 1) == ERR_WORKSPACE
  assert call(ws_bytes=0) == ERR_WORKSPACE
  # best_score may be NULL: only the workspace is missing
  assert call(best_score=None, ws_bytes=0) == ERR_WORKSPACE
  # a host plan whose counts, tiles, labels or pair tiles were edited: rejected (the kernels trust its bounds)
  parts = _parts(plan)
  at_off = HDR + 4 + 5 + parts['rt'].size + parts['ct'].size
  at_idx = at_off + 5
  at_pt = at_idx + 5
  for at, val in [(0, 4), (1, 3), (HDR, 1), (HDR + 2, 0), (5, 2), (6, 2), (7, 4), (8, 2), (9, 64),
                  (at_off, 1), (at_off + 1, 0), (at_off + 4, 4), (at_idx, 3), (at_idx + 2, -1),
                  (at_pt, 1), (at_pt + 1, 4)]:
    edited = plan.copy()
    edited[at] = val
    assert call(ph=edited.ctypes.data) == ERR_ARG, (at, val)
  # a query tile over the group cap: rejected
  ones = [1] * 100
  n2, p2 = _plan(lib, ones, ones, P2V, np.arange(101), np.arange(100))
  p2 = p2[:n2].copy()
  parts = _parts(p2)
  assert parts['ct'].tolist() == [0, QCAP, 100]
  at_ct = HDR + 101 + 101 + parts['rt'].size
  ws2 = ctypes.c_void_p(1 << 20)
  assert lib.cmhse_group_rank_labelled(fake, fake, 100, 100, 8, p2.ctypes.data, fake, n2, P2V, 1, fake, fake, fake,
                                       None, ws2, 0, None) == ERR_WORKSPACE
  p2[at_ct + 1] += 1                                       # the second caption tile starts one later: 73 groups
  assert lib.cmhse_group_rank_labelled(fake, fake, 100, 100, 8, p2.ctypes.data, fake, n2, P2V, 1, fake, fake, fake,
                                       None, ws2, 1 << 30, None) == ERR_ARG
  # a pair tile over 128 rows: rejected
  n3, p3 = _plan(lib, [128, 128], [1, 1], P2V, [0, 1, 2], [0, 1])
  p3 = p3[:n3].copy()
  assert _parts(p3)['pt'].tolist() == [0, 1, 2]
  merged = np.concatenate([p3[:-3], [0, 2]]).astype(np.int32)
  merged[8] = 1
  assert lib.cmhse_group_rank_labelled(fake, fake, 256, 2, 8, merged.ctypes.data, fake, merged.size, P2V, 1, fake,
                                       fake, fake, None, ws2, 1 << 30, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------
# ops / evaluation: ValueErrors, no GPU
# ---------------------------------------------------------------------------------------------
def test_ops_plan_matches_the_c_plan(lib):
  from cmhse_amd import ops
  clips, caps = [2, 1, 3], [1, 1, 2, 4]
  lists = [[0], [2, 2], [1], [0]]
  want_n, want = _plan(lib, clips, caps, P2V, [0, 1, 3, 4, 5], [0, 2, 2, 1, 0])
  got = ops.group_rank_labelled_plan(clips, caps, 6, 8, lists, 'p2v')
  assert got.dtype == np.int32 and np.array_equal(got, want[:want_n])
  got = ops.group_rank_labelled_plan(torch.tensor(clips), np.array(caps), 6, 8, [0, 3, 1], 'v2p')
  assert got[4] == V2P and got[7] == 3


def test_ops_value_errors_without_gpu():
  from cmhse_amd import ops
  c, s = torch.zeros(6, 4), torch.zeros(8, 4)
  good = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], positives=[0, 2, 1, 0], direction='p2v', reduce='max')
  bads = [dict(reduce='sum'), dict(direction='both'), dict(num_clips=[2, 0, 4]), dict(num_clips=[2, 1, 2]),
          dict(num_caps=[1, 1, 2, 3]), dict(num_caps=[]), dict(num_clips=[2, 1.5, 2.5]),
          dict(positives=[0, 2, 1]), dict(direction='v2p'), dict(positives=[[0], [], [1], [2]])]
  for bad in bads:
    with pytest.raises(ValueError):
      ops.group_rank_labelled(c, s, **dict(good, **bad))
  for positives, needle in [([0, 3, 1, 0], 'query row 1: positive 3'), ([[0], [1], [2, -1], [0]], 'query row 2'),
                            ([[0], [1], [], [0]], 'query row 2 has no positive'),
                            (([0, 1, 2, 3, 3], [0, 1, 2]), 'query row 3 has no positive')]:
    with pytest.raises(ValueError) as e:
      ops.group_rank_labelled(c, s, **dict(good, positives=positives))
    assert needle in str(e.value), str(e.value)
  with pytest.raises(ValueError) as e:                   # v2p: 3 queries, 4 gallery paragraphs
    ops.group_rank_labelled(c, s, **dict(good, direction='v2p', positives=[3, 4, 0]))
  assert 'query row 1: positive 4' in str(e.value)
  with pytest.raises(ValueError):
    ops.group_rank_labelled(torch.zeros(6), s, **good)
  with pytest.raises(ValueError):
    ops.group_rank_labelled(c, torch.zeros(8, 5), **good)
  with pytest.raises(ValueError):
    ops.group_rank_labelled(c.numpy(), s, **good)
  with pytest.raises(ValueError):                        # a 129-clip video
    ops.group_rank_labelled(torch.zeros(130, 4), torch.zeros(2, 4), [129, 1], [1, 1], [0, 1])
  with pytest.raises(RuntimeError):                      # valid arguments, host tensors: no CPU fallback
    ops.group_rank_labelled(c, s, **good)


def test_evaluation_value_errors_without_gpu():
  from cmhse_amd import evaluation
  c, s = np.zeros((6, 4), np.float32), np.zeros((8, 4), np.float32)
  good = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], positives=[0, 2, 1, 0], direction='p2v', reduce='max')
  stats, last = dict(evaluation.CACHE_STATS), evaluation._LAST_ENCODE[0]
  for bad in [dict(reduce='median'), dict(direction='x'), dict(num_clips=[3, 3, 1]), dict(positives=[0, 2, 1]),
              dict(positives=[0, 2, 3, 0])]:
    with pytest.raises(ValueError):
      evaluation.group_rank_labelled(c, s, **dict(good, **bad))
  with pytest.raises(ValueError) as e:
    evaluation.group_rank_labelled(c, s, **dict(good, positives=[0, 2, 3, 0]))
  assert 'query row 2: positive 3' in str(e.value)
  with pytest.raises(ValueError):
    evaluation.group_rank_labelled(c, np.zeros((8, 5), np.float32), **good)
  with pytest.raises(ValueError):
    evaluation.group_rank_labelled(np.zeros(6, np.float32), s, **good)
  pairs = [[0, 0], [1, 1], [2, 2], [0, 3]]
  both = dict(num_clips=[2, 1, 3], num_caps=[1, 1, 2, 4], pairs=pairs, reduce='max')
  for bad, needle in [(dict(pairs=pairs[:3]), 'caption row 3 appears in no pair'),
                      (dict(pairs=pairs[1:]), 'caption row 0 appears in no pair'),
                      (dict(pairs=[[0, 0], [0, 1], [2, 2], [0, 3]]), 'image row 1 appears in no pair'),
                      (dict(pairs=pairs + [[3, 0]]), 'pair 4: image row 3 outside'),
                      (dict(pairs=pairs + [[0, 4]]), 'pair 4: caption row 4 outside'),
                      (dict(pairs=np.zeros((4, 2))), 'integer'), (dict(reduce='sum'), 'reduce'),
                      (dict(num_caps=[1, 1, 2, 5]), 'tile the rows'), (dict(num_clips=[2, 1, 2]), 'tile the rows')]:
    with pytest.raises(ValueError) as e:
      evaluation.group_i2t_t2i_labelled(c, s, **dict(both, **bad))
    assert needle in str(e.value), str(e.value)
  assert evaluation.CACHE_STATS == stats and evaluation._LAST_ENCODE[0] is last


# ---------------------------------------------------------------------------------------------
# the front end on a NumPy stand-in
# ---------------------------------------------------------------------------------------------
def numpy_block_scores(clips, caps, num_clips, num_caps, reduce):
  """G [Bv, Bp] in NumPy for a rectangular problem (the statement of test_group_rank_cpu.numpy_group_scores)."""
  scores = np.asarray(clips, dtype=np.float32) @ np.asarray(caps, dtype=np.float32).T
  oc, op = _offsets(num_clips), _offsets(num_caps)
  G = np.empty((len(num_clips), len(num_caps)), dtype=np.float32)
  for i in range(G.shape[0]):
    for j in range(G.shape[1]):
      block = scores[oc[i]:oc[i + 1], op[j]:op[j + 1]]
      G[i, j] = block.max() if reduce == 'max' else np.float32(np.cumsum(block.astype(np.float64).ravel())[-1]
                                                                 / block.size)
  return G


def _stand_in(calls):
  """ops.group_rank_labelled in NumPy on host tensors: the contract on numpy_block_scores' G."""
  from cmhse_amd import ops

  def group_rank_labelled(c, s, num_clips, num_caps, positives, direction='p2v', reduce='max', return_score=False):
    Bv, Bp = len(num_clips), len(num_caps)
    off, idx = ops.positives_csr(positives, *((Bp, Bv) if direction == 'p2v' else (Bv, Bp)))
    calls.append((direction, off.tolist(), idx.tolist()))
    G = numpy_block_scores(c.numpy(), s.numpy(), num_clips, num_caps, reduce)
    rank, top1, best_pos, _ = group_labelled_reference(G, direction, off, idx)
    return tuple(torch.from_numpy(x.astype(np.int32)) for x in (rank, top1, best_pos))
  return group_rank_labelled


def test_front_end_label_handling_on_numpy_stand_in(monkeypatch):
  from cmhse_amd import evaluation, ops
  calls = []
  monkeypatch.setattr(ops, 'group_rank_labelled', _stand_in(calls))
  monkeypatch.setattr(evaluation, '_as_device', lambda x, device=None: torch.from_numpy(np.asarray(x, np.float32)))
  rng = np.random.RandomState(3)
  nclips, ncaps = [2, 1, 3, 2], [1, 2, 1, 3, 2, 1, 1, 2]          # 4 videos, 8 paragraphs: j <-> j % 4
  c = rng.standard_normal((sum(nclips), 16)).astype(np.float32)
  s = rng.standard_normal((sum(ncaps), 16)).astype(np.float32)
  ids_v = ['a', 'b', 'c', 'd']
  pairs = evaluation.pairs_from_ids(ids_v, ids_v + ids_v)
  assert pairs.tolist() == [[i, j] for i in range(4) for j in (i, i + 4)]
  for reduce in ('max', 'mean'):
    del calls[:]
    (rep_v, top1_v, ranks_v), (rep_p, top1_p, ranks_p) = evaluation.group_i2t_t2i_labelled(
        c, s, nclips, ncaps, pairs[::-1], reduce=reduce)         # any order of the pairs
    assert calls == [('v2p', [0, 2, 4, 6, 8], [0, 4, 1, 5, 2, 6, 3, 7]),
                     ('p2v', list(range(9)), [0, 1, 2, 3, 0, 1, 2, 3])]
    G = numpy_block_scores(c, s, nclips, ncaps, reduce)
    want_v = group_labelled_reference(G, 'v2p', *calls[0][1:])
    want_p = group_labelled_reference(G, 'p2v', *calls[1][1:])
    for arr, want in ((ranks_v, want_v[0]), (top1_v, want_v[1]), (ranks_p, want_p[0]), (top1_p, want_p[1])):
      assert isinstance(arr, np.ndarray) and arr.dtype == np.float64 and np.array_equal(arr, want)
    assert ranks_v.shape == (4,) and ranks_p.shape == (8,)
    assert rep_v == evaluation.report_from_ranks(want_v[0].astype(np.float64))
    assert rep_p == evaluation.report_from_ranks(want_p[0].astype(np.float64))
    # one direction, any of positives_csr's forms
    rep, top1, ranks = evaluation.group_rank_labelled(c, s, nclips, ncaps, [[j % 4] for j in range(8)], 'p2v',
                                                      reduce)
    assert rep == rep_p and np.array_equal(top1, top1_p) and np.array_equal(ranks, ranks_p)
    assert calls[-1] == calls[1]


def test_contract_square_diagonal_is_group_rank():
  """With P_q = {q} the contract is cmhse_group_rank's: the diagonal never beats itself."""
  rng = np.random.RandomState(5)
  G = rng.standard_normal((30, 30)).astype(np.float32)
  G[:, 7] = G[:, 3]                                       # exact ties across two paragraphs
  d = np.diag(G)
  B = 30
  rank, top1, best_pos, best = group_labelled_reference(G, 'v2p', np.arange(B + 1), np.arange(B))
  off_diag = ~np.eye(B, dtype=bool)
  assert np.array_equal(rank, ((G > d[:, None]) & off_diag).sum(axis=1)) and np.array_equal(top1, G.argmax(axis=1))
  assert np.array_equal(best_pos, np.arange(B)) and np.array_equal(best, d)
  rank, top1, _, _ = group_labelled_reference(G, 'p2v', np.arange(B + 1), np.arange(B))
  assert np.array_equal(rank, ((G > d[None, :]) & off_diag).sum(axis=0)) and np.array_equal(top1, G.argmax(axis=0))


# ---------------------------------------------------------------------------------------------
# the GPU file's cases reach what they are meant to reach
# ---------------------------------------------------------------------------------------------
def test_gpu_cases_reach_their_paths(lib):
  # the rectangular problem: one query's 40 pairs span several pair tiles, the gallery has several tiles
  nclips, ncaps = rect_counts()
  for direction, Bq, Bg in (('p2v', 500, 700), ('v2p', 700, 500)):
    off, idx = rect_labels(41, Bq, Bg, many_at=Bq // 2)
    assert off[Bq // 2 + 1] - off[Bq // 2] == MANY
    lists = [idx[off[q]:off[q + 1]] for q in range(Bq)]
    assert any(len(set(x)) < len(x) for x in lists)        # duplicates inside a list
    parts = _parts(_check_plan(lib, nclips, ncaps, DIRECTION[direction], off, idx))
    a, b = int(off[Bq // 2]), int(off[Bq // 2 + 1])
    tiles = np.searchsorted(parts['pt'], [a, b - 1], side='right')
    assert tiles[1] - tiles[0] >= 2                        # at least three pair tiles hold its pairs
  # 40 queries x 3000 gallery groups: one query tile, many panels
  qn, gn = panel_case()
  for direction, (clips, caps) in (('p2v', (gn, qn)), ('v2p', (qn, gn))):
    off, idx = rect_labels(43, 40, 3000)
    plan = _check_plan(lib, clips, caps, DIRECTION[direction], off, idx)
    assert _panels_of(lib, plan) > 8
  # 600 one-row query groups: nine query tiles, eight of them at the cap
  qn, gn = cap_case()
  for direction, (clips, caps) in (('p2v', (gn, qn)), ('v2p', (qn, gn))):
    off, idx = rect_labels(47, 600, 50)
    parts = _parts(_check_plan(lib, clips, caps, DIRECTION[direction], off, idx))
    q_tiles = parts['ct'] if direction == 'p2v' else parts['rt']
    assert np.diff(q_tiles).tolist() == [QCAP] * 8 + [600 - 8 * QCAP]
