"""The bf16x3 cases reach the kernels, cuts and hand-overs they name, and the float64 emulation of the
mode's split products is a yardstick worth its bar (no GPU needed).

The dispatch of the bf16x3 math mode as tests/fwd_shapes.py restates it (which requests carry the flag,
the TiledBf3 step, rows_split, every launch of the attention projection and its cut), applied to the
cases of tests/test_gpu_bf3_shapes.py; the constants and the two expressions it assumes, read from the
sources; the emulation (oracle.split_bf16x3 / matmul_nt) against the float64 oracle on every case, and
two wrong splits it must tell from the right one."""
import numpy as np
import pytest

from conftest import GOLDEN_TOL

import fwd_shapes as fs
import test_gpu_bf3_shapes as g


def _calls():
  for name, knobs, train, tail_stream, jobs, targets in fs.BF3_CASES:
    yield name, jobs, targets, fs.call_steps(jobs, knobs, tail_stream, bf3=True), fs.call_tags(jobs, knobs, tail_stream, bf3=True)


def test_rule_constants_match_the_sources():
  src = fs.source_constants()
  assert src['kAttBN'] == fs.ATT_BN and src['att_bm_bf3'] == fs.ATT_BM_BF3
  assert src['job_bf3'] == fs.JOB_BF3_EXPR, src['job_bf3']
  assert src['att_bf3'] == fs.ATT_BF3_EXPR, src['att_bf3']
  # (the tile height of an exact request shows in no result — its shapes are bit-identical — so the
  # one line that keeps the bf16x3 requests out of tiled_wgs is pinned here)
  assert src['tiled_wgs_also'] == fs.TILED_WGS_ALSO, src['tiled_wgs_also']


def test_every_case_reaches_its_targets():
  assert len({c[0] for c in fs.BF3_CASES}) == len(fs.BF3_CASES)
  assert not fs.BF3_TAGS & fs.ALL_TAGS
  for name, jobs, targets, plan, tags in _calls():
    assert 1 <= len(jobs) <= 4 and sum(j['counts'][0] for j in jobs) <= 800, name   # a few hundred sequences
    assert targets <= fs.BF3_TAGS | fs.ALL_TAGS, (name, sorted(targets - fs.BF3_TAGS - fs.ALL_TAGS))
    for j in jobs:
      assert fs.counts_of(fs.lens_of(j['counts'])) == j['counts'] and not j['save'] and j['stream'] is None, name
      if j['plan'] is not None:
        assert all(p >= c for p, c in zip(j['plan'], j['counts'])) and len(j['plan']) == len(j['counts'])
    assert targets <= tags, (name, sorted(targets - tags))
    assert 'token table' not in tags, name          # the mode's flag closes the table for the whole call
    assert not any(t.startswith('Chain') or t.startswith('FwdTail') for t in tags), name
    for launches in plan:
      # the ring steps are a prefix of the request's steps, and rows_split is their packed rows
      ring = [ln['ts'][0] for ln in launches if ln['tag'] == 'TiledBf3']
      assert ring == list(range(len(ring))), name
      assert (len(ring) > 0) <= launches.bf3, name


def test_the_table_reaches_the_whole_vocabulary():
  reached = set()
  for name, jobs, targets, plan, tags in _calls():
    reached |= tags
  assert set(fs.BF3_UNREACHABLE) <= fs.BF3_TAGS and not set(fs.BF3_UNREACHABLE) & reached
  assert fs.BF3_TAGS - set(fs.BF3_UNREACHABLE) <= reached, sorted(fs.BF3_TAGS - set(fs.BF3_UNREACHABLE) - reached)
  assert set().union(*(c[5] for c in fs.BF3_CASES)) >= fs.BF3_TAGS - set(fs.BF3_UNREACHABLE)


def _by_name():
  return {name: (jobs, plan, tags) for name, jobs, targets, plan, tags in _calls()}


def _knob(name, knob):
  return next(c for c in fs.BF3_CASES if c[0] == name)[1][knob]


def _attn(plan):
  return [[(ln['lo'], ln['cut'], ln['hi'], ln['partial']) for ln in launches if ln['kind'] == 'attn'] for launches in plan]


def test_cuts_and_hand_overs_land_where_the_cases_say():
  c = _by_name()
  # one shared launch per step for the four pool modes
  jobs, plan, _ = c['bf3_all_pools']
  for t in range(3):
    assert all(launches[t]['tag'] == 'TiledBf3' and launches[t]['group'] == [0, 1, 2, 3] for launches in plan)
  assert [p.rows_split for p in plan] == [906, 619, 275, 329] and _attn(plan)[3] == [(0, 329, 332, False)]
  # rows_split = 458 of 470: ring tiles of 128, 128, 128, 74 rows, then 12 fp32 rows; two column tiles, 8 columns in the second
  jobs, plan, _ = c['bf3_attn_cut']
  ln, = [ln for ln in plan[0] if ln['kind'] == 'attn']
  assert (ln['lo'], ln['cut'], ln['hi']) == (0, 458, 470) and ln['row_tiles'] == (4, 1) and ln['col_tiles'] == 2
  assert 458 % 128 == 74 and jobs[0]['H'] - fs.ATT_BN == 8 and jobs[0]['H'] % 16 == 8
  # bf16x3 by the pooling alone; an exact projection (42 plan rows <= 64); an untouched request
  jobs, plan, _ = c['bf3_attn_only']
  assert [p.bf3 for p in plan] == [True, True, False] and [p.rows_split for p in plan] == [0, 0, 0]
  assert [fs.bf3_kernels(p) for p in plan] == [True, False, False]
  assert _attn(plan)[:2] == [[(0, 0, 91, False)], [(0, 0, 42, False)]]
  assert [ln['tag'] for ln in plan[1] if ln['kind'] == 'attn'] == ['Attn fp32']
  # every step on the mid-size kernel
  jobs, plan, _ = c['bf3_mid_only']
  assert all(ln['tag'].startswith('Mid') for p in plan for ln in p if ln['kind'] == 'step')
  assert [p.bf3 for p in plan] == [True, True] and [fs.bf3_kernels(p) for p in plan] == [True, False]
  # the partial launches and the three positions of the cut
  assert _attn(c['bf3_partial_a'][1]) == [[(0, 144, 144, False)], [(0, 357, 357, True), (357, 464, 468, False)]]
  assert _attn(c['bf3_partial_b'][1]) == [[(0, 199, 199, False)], [(0, 336, 349, True), (349, 349, 353, False)]]
  # the ring step read by the latency-shaped kernel
  jobs, plan, _ = c['bf3_to_tiny']
  assert [ln['tag'] for ln in plan[0]] == ['TiledBf3'] * 5 + ['Tiny vec'] * 3
  # a share: the ring step by the plan while the share's own tiles hold 1 to 63 rows
  jobs, plan, _ = c['bf3_split_share']
  assert all(max(j['counts']) <= 63 and max(j['plan']) > 1024 for j in jobs)
  assert [p.rows_split for p in plan] == [169, 145, 90] and _attn(plan)[2] == [(0, 90, 92, False)]
  # the exact scalar tile beside the ring step: 64 rows, because tiled_wgs counts the exact request only
  jobs, plan, _ = c['bf3_beside_exact']
  assert [ln['tag'] for ln in plan[1]] == ['Tiled64 scalar'] * 3 + ['Tiny scalar'] and not plan[1].bf3
  wgs = [fs._tiled64_grid(j['H'], j['counts'][0]) for j in jobs]
  assert wgs[1] < _knob('bf3_beside_exact', 'tall_tile_min_wgs') <= sum(wgs)


def test_required_edges_are_in_the_table():
  """S_t at 127 / 128 / 129 and 255 / 256 / 257 on the 128-row ring tile, a last tile with one valid row,
  length-1 sequences, H % 16 != 0, H % 64 != 0, H < 64, and 1, 2, 3, 4, 5 and >= 7 chunks of 16 k in
  either phase of the ring."""
  counts, hs, x_chunks, h_chunks, len1 = set(), set(), set(), set(), False
  for name, jobs, targets, plan, tags in _calls():
    for j, launches in zip(jobs, plan):
      ring = [ln['ts'][0] for ln in launches if ln['tag'] == 'TiledBf3']
      if not ring:
        continue
      counts |= {j['counts'][t] for t in ring}
      hs.add(j['H'])
      x_chunks.add(-(-j['I'] // 16))
      if len(ring) > 1 or j['h0']:
        h_chunks.add(-(-j['H'] // 16))
      len1 = len1 or (len(j['counts']) > 1 and j['counts'][1] < j['counts'][0])
  for c in (127, 128, 129, 255, 256, 257):
    assert c in counts, c
  assert any(c % 128 == 1 for c in counts) and len1
  assert any(h % 16 for h in hs) and any(h % 64 for h in hs) and any(h < 64 for h in hs)
  for n in (1, 2, 3, 4, 5):
    assert n in x_chunks or n in h_chunks, n
  assert {1, 2, 3, 4} <= x_chunks and {1, 2, 3, 4, 5} <= h_chunks
  assert max(x_chunks) >= 7 and max(h_chunks) >= 7


def _distance(refs, a, b):
  return max(float(np.abs(r[a] - r[b]).max()) for r in refs)


def _hs_distance(refs, other=None):
  other = refs if other is None else other
  return max(float(np.abs(r['emu_hs'] - o['hs' if other is refs else 'emu_hs']).max()) for r, o in zip(refs, other))


@pytest.mark.parametrize('name', [c[0] for c in fs.BF3_CASES])
def test_emulation_is_within_half_the_modes_bar(oracle, name):
  """The emulation alone against the float64 oracle: at most 2.5e-5, half the 5e-5 the mode is held to,
  so that bar is one the reference keeps with room.  (bf3_wide: its first three steps.)"""
  refs = g.references(oracle, name, steps=3 if name == 'bf3_wide' else None)
  d = max(_distance(refs, 'emu', 'want'), _hs_distance(refs))
  print('bf3 emulation vs float64 oracle: %-24s %.3e' % (name, d))
  assert d <= 2.5e-5, d
  assert 2.5e-5 == g.BF3_TOL / 2


def test_emulation_tells_wrong_splits_from_the_right_one(oracle):
  """A truncating split misses GOLDEN_TOL (the bar against the emulation); a split without a_lo b_hi
  misses the 5e-5 of the float64 oracle."""
  good = g.references(oracle, 'bf3_all_pools')
  trunc = g.references(oracle, 'bf3_all_pools', products='bf16x3-truncate')
  two = g.references(oracle, 'bf3_all_pools', products='bf16x3-two-terms')
  d_trunc = max(max(float(np.abs(a['emu'] - b['emu']).max()) for a, b in zip(trunc, good)), _hs_distance(trunc, good))
  d_two = max(_distance(two, 'emu', 'want'), _hs_distance(two))
  print('truncating split: %.3e from the emulation; two-term split: %.3e from the float64 oracle' % (d_trunc, d_two))
  assert d_trunc > GOLDEN_TOL and d_two > g.BF3_TOL


def test_split_is_round_to_nearest_even_and_rows_are_laid_out_in_chunks(oracle):
  x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 3.0e-39, 0.0], dtype=np.float32)
  hi, lo = oracle.split_bf16x3(x)
  # ties go to the even bf16: 1 + 2^-8 -> 1 (lo 2^-8), 1 + 3 2^-8 -> 1 + 2^-6 (lo -2^-8); above a tie: up
  assert hi[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)]
  assert lo[:3].tolist() == [0.0, 2.0 ** -8, -(2.0 ** -8)]
  assert np.all(np.abs(x.astype(np.float64) - hi - lo) <= np.abs(x) * 2.0 ** -16 + 1e-40)
  rng = np.random.RandomState(3)
  rows = (rng.standard_normal((3, 20)) * 3).astype(np.float32)
  bits = oracle.split_rows_bits(rows, 20)
  assert bits.shape == (3, 32) and bits.dtype == np.uint32
  hi, lo = oracle.split_bf16x3(rows)
  for k in range(20):
    c, q, odd = k // 16, (k % 16) // 2, k % 2
    assert np.array_equal((bits[:, 16 * c + q] >> (16 * odd)) & 0xffff, hi[:, k].view(np.uint32) >> 16)
    assert np.array_equal((bits[:, 16 * c + 8 + q] >> (16 * odd)) & 0xffff, lo[:, k].view(np.uint32) >> 16)
  assert not bits[:, 18:24].any() and not bits[:, 26:].any()      # k >= K reads zero
