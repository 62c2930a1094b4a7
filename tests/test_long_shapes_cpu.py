"""The cases of tests/test_gpu_long_shapes.py reach the loops they name (no GPU needed): the trip
counts tests/long_shapes.py restates, their constants and the loops themselves checked against the
sources, applied to the case table through the dispatch rules of fwd_shapes, bptt_shapes and
bwd_side_shapes.  A retuned threshold or a rewritten loop fails here instead of quietly moving a
case off its target."""
import numpy as np
import pytest

from conftest import golden_state_dicts, load_golden

import fwd_shapes
import long_shapes as ls


def test_rule_constants_match_the_sources():
  src = ls.source_constants()
  assert src['kThreads'] == ls.THREADS
  assert src['kPoolBwdThreads'] == ls.POOL_BWD_THREADS == 64 * ls.POOL_BWD_WAVES
  assert src['kChainMaxStepsWs'] == ls.CHAIN_MAX_STEPS
  assert src['kAttBN'] == ls.ATT_BN
  assert src['kColsumRows'] == ls.COLSUM_ROWS
  for f, loops in ls.LOOPS.items():
    for text, n in loops:
      assert src['loops'][(f, text)] == n, (f, text, src['loops'][(f, text)])
  # the forward dispatch's defaults (the cases name their own knobs on top of these)
  fsrc = fwd_shapes.source_constants()
  for name, dflt in fwd_shapes.KNOBS.items():
    assert fsrc[name] == dflt, name


def test_trip_counts():
  assert [ls.attn_pool_rounds(n) for n in (1, 255, 256, 257, 512, 513)] == [1, 1, 1, 2, 2, 3]
  assert [ls.attn_pool_unit_rounds(H) for H in (72, 1024, 1028, 1030, 1040)] == [1, 1, 2, 2, 2]
  assert [ls.attn_bwd_steps_per_wave(n) for n in (16, 17, 512, 513, 1025)] == [1, 2, 32, 33, 65]
  assert [ls.attn_bwd_den_trips(n) for n in (513, 1024, 1025)] == [1, 1, 2]
  assert ls.energy_tiles(1040) == (5, 16) and ls.energy_tiles(1030) == (5, 6) and ls.energy_tiles(72) == (1, 72)


def test_every_case_reaches_exactly_its_tags():
  names = [c[0] for c in ls.CASES]
  assert len(set(names)) == len(names)
  for case in ls.CASES:
    name, knobs, train, tail_stream, jobs, targets = case
    assert targets <= ls.VOCABULARY, (name, sorted(targets - ls.VOCABULARY))
    assert 1 <= len(jobs) <= (2 if train else 4), name
    for j in jobs:
      assert ls.counts_of(ls.lens_of(j['counts'])) == list(j['counts']), name
    tags = ls.case_tags(case)
    assert tags == targets, (name, 'missing', sorted(targets - tags), 'not named', sorted(tags - targets))


def test_the_vocabulary_is_covered():
  assert ls.UNREACHABLE == {}
  reached = set().union(*(c[5] for c in ls.CASES))
  assert reached == ls.VOCABULARY, sorted(ls.VOCABULARY - reached)


def test_the_lengths_are_the_ones_the_table_states():
  """What the comments of the case table say about its requests."""
  jobs = ls.case('pool_rounds')[4]
  assert [list(ls.lens_of(j['counts'])) for j in jobs] == [[513, 512, 257, 256, 255, 3, 1], [300, 257, 2], [513, 1], [260, 5]]
  assert jobs[0]['vocab'] == ls.VOCAB_ROWS and not jobs[1]['vocab'] and jobs[3]['h0']
  # the shorter attention request ends first: the longer one's projection is [0, rows of steps 0..299) then the rest
  attn = [ln for ln in ls._launches(ls.case('pool_rounds'))[0] if ln['kind'] == 'attn']
  assert [(a['lo'], a['hi'], a['partial']) for a in attn] == [(0, 1372, True), (1372, 1797, False)]
  assert attn[0]['hi'] == sum(jobs[0]['counts'][:300]) and attn[0]['col_tiles'] == 1
  for name, H, last in (('pool_wide_vec', 1040, 16), ('pool_wide_scalar', 1030, 6)):
    j = ls.case(name)[4][0]
    assert j['H'] == H and ls.energy_tiles(H) == (5, last) and ls.attn_pool_unit_rounds(H) == 2
    assert list(ls.lens_of(j['counts'])) == [260, 257, 9, 1]
  a, m = ls.case('chain_cuts')[4]
  la, lm = ls.lens_of(a['counts']), ls.lens_of(m['counts'])
  assert len(la) == 40 and int((la == 300).sum()) == 20 and int((la == 330).sum()) == 2
  assert sorted(set(int(n) for n in la)) == [1, 9, 95, 96, 97, 193, 300, 330]
  assert len(lm) == 24 and int(lm.max()) == 200
  j = ls.case('aliases_long')[4][0]
  assert list(ls.lens_of(j['counts'])) == [513, 300, 40] and j['aliases'] == ((0, 257), (0, 513), (1, 256), (2, 1))
  j = ls.case('train_attn_1025')[4][0]
  assert list(ls.lens_of(j['counts'])) == [1025, 1024, 3] and sum(j['counts']) == 2052


def test_the_chain_is_cut_at_96_steps_and_resumed():
  case = ls.case('chain_cuts')
  attn, mx = ls.chain_launches(case)
  assert attn == [96, 96, 8, 96, 4] and mx == [96, 96, 8]      # the third cut: the max-pooled request ends
  assert max(attn) <= ls.CHAIN_MAX_STEPS and len(attn) >= 4
  # ... and latency-shaped steps follow the chain's last launch
  lns = ls._launches(case)[0]
  last_chain = max(ln['ts'][-1] for ln in lns if ln['kind'] == 'chain')
  after = [ln for ln in lns if ln['kind'] == 'step' and ln['ts'][0] > last_chain]
  assert last_chain == 299 and len(after) == 30 and all(ln['tag'].startswith('Mid') for ln in after)


def test_the_tail_cases_have_tails_of_500_steps():
  for name in ls.TAIL_CASES:
    case = ls.case(name)
    ts = ls.fwd_tail_of(case, 0)
    T = len(case[4][0]['counts'])
    assert len(ts) >= ls.LONG and ts[-1] == T - 1, (name, len(ts))
    tail = ls.bwd_tail_of(case, 0)
    assert tail is not None and T - tail[0] >= ls.LONG, (name, tail)
  # 2052 rows: the walk closes a chunk of 2049 rows at step 1, the tail's 2046 rows among them
  pl = ls.bwd_plan(ls.case('train_attn_1025'), 0)
  assert [(c['rows'], c['tail_rows']) for c in pl['chunks']] == [(2049, 2049), (3, 0)]
  assert pl['attn']['colsum_slabs'] == 5
  j = ls.case('train_attn_1025')[4][0]
  k = dict(fwd_shapes.KNOBS, **ls.case('train_attn_1025')[1])
  assert len(fwd_shapes.xproj_chunks(j['counts'], k)) == 8
  assert sum(j['counts']) < 4 * fwd_shapes.KNOBS['xproj_chunk_rows']      # why the case names the knob


def test_the_per_step_and_wide_cases_have_no_tail():
  for name in ls.NO_TAIL_CASES:
    case = ls.case(name)
    for m, j in enumerate(case[4]):
      assert ls.fwd_tail_of(case, m) == [] and ls.bwd_tail_of(case, m) is None, (name, m)
  # the wide case: refused by the width alone (both rules give a tail at H = 1024)
  case = ls.case('train_wide')
  for m in range(2):
    assert len(ls.fwd_tail_of(case, m, 1024)) == 19 and ls.bwd_tail_of(case, m, 1024) is not None
  # the per-step case: 513 launches each way
  case = ls.case('train_long_per_step')
  for lns in ls._launches(case):
    assert len([ln for ln in lns if ln['kind'] == 'step']) == 513


@pytest.mark.parametrize('rnn_type', ['attention', 'maxout'])
def test_the_oracle_alone_meets_the_rank_cap(oracle, rnn_type):
  """The outlier split: a 525-word paragraph, 300 frames, items of length 1 — and float64 ranks that
  leave out at most one row of nine at the margin the GPU test uses."""
  spec = ls.outlier_spec()
  assert spec.n_videos == 9 and spec.num_clips[0] == 25 and set(spec.words_per_sent[:25]) == {21}
  assert spec.frames_per_video[0] == 300
  assert 1 in spec.words_per_sent and 1 in spec.frames_per_clip and 1 in spec.frames_per_video and 1 in spec.num_clips
  g = load_golden('model_%s.npz' % rnn_type)
  batches = ls.outlier_batches(24, 60)
  assert int(batches[0][7][0]) == 525 and len(batches) == 2
  nb = [tuple(x.numpy() if hasattr(x, 'numpy') else x for x in b) for b in batches]
  want = oracle.encode_data(rnn_type, golden_state_dicts(g), nb, margin=0.2, dtype=np.float64)
  for ranks, top1, ok in ls.robust_rows(want):
    assert int((~ok).sum()) <= ls.RANK_LEFT_OUT_MAX, ok
