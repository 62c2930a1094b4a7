"""The cases of tests/test_gpu_bwd_side_shapes.py reach the launches they name (no GPU needed): the
host-side rules of what cmhse_gru_pool_bwd runs beside its chain as tests/bwd_side_shapes.py
restates them, their constants checked against the sources, applied to the case table and to the
two weight-gradient tests of tests/test_gpu_gru.py whose docstrings make claims about the row
split.  A retuned cost model or a moved crossover fails here instead of quietly moving a case off
its target."""
import numpy as np

import bwd_side_shapes as ss


def test_rule_constants_match_the_sources():
  src = ss.source_constants()
  for name, dflt in ss.KNOBS.items():
    assert src[name] == dflt, (name, src[name], dflt)
  assert (src['kDetSplitRows'], src['kDetSplitMax']) == (ss.DET_SPLIT_ROWS, ss.DET_SPLIT_MAX)
  assert src['det_seg_min_k'] == src['atomic_seg_min_k'] == ss.SEG_MIN_K
  assert (src['atomic_grid_max'], src['atomic_min_k'], src['atomic_wgs']) == (
      ss.ATOMIC_GRID_MAX, ss.ATOMIC_MIN_K, ss.ATOMIC_WGS)
  assert src['kColsumRows'] == ss.COLSUM_ROWS
  assert (src['kTnRowsBmSmall'], src['kTnRowsBmTall']) == (ss.TN_BM_SMALL, ss.TN_BM_TALL)
  assert src['kAttBN'] == ss.ATT_BN
  assert src['kBK'] == ss.BK
  assert src['kPoolBwdThreads'] == 64 * ss.POOL_BWD_WAVES
  assert (src['tn_limit_beside'], src['tn_limit_last']) == (ss.TN_LIMIT_BESIDE, ss.TN_LIMIT_LAST)
  assert (src['tn_split_max'], src['tn_split_min_rows']) == (ss.TN_SPLIT_MAX, ss.TN_SPLIT_MIN_ROWS)
  assert (src['wg_part_min_rows'], src['wg_part_max']) == (ss.WG_PART_MIN_ROWS, ss.WG_PART_MAX)


def test_the_own_zero_arm_has_no_caller():
  """launch_nt_out's split = 1 arm (a dense C the call zeroes itself) is dead: every call site
  passes split = 0 (by default) or 2, so the rule does not model it."""
  sites = ss.nt_out_call_sites()
  assert ss.no_own_zero_caller(), sites
  assert sorted(len(a) for a in sites) == [12, 12, 13], sites      # two unsplit fall-backs, one atomic call
  assert [a[12] for a in sites if len(a) == 13] == ['2']


def test_every_case_reaches_its_targets():
  names = [c[0] for c in ss.CASES]
  assert len(set(names)) == len(names)
  for case in ss.CASES:
    name, feed, knobs, cls, I, H, profile, targets = case
    assert targets <= ss.VOCABULARY, (name, sorted(targets - ss.VOCABULARY))
    lens = ss.lens_of(profile)
    assert ss.counts_of(lens) == list(profile), name
    tags = ss.side_tags(ss.case_plan(case))
    assert targets <= tags, (name, sorted(targets - tags))


def test_the_segments_are_the_ones_the_table_states():
  """The segment lengths the comments of the case table give (issue of this test file)."""
  plans = {c[0]: ss.case_plan(c) for c in ss.CASES}

  def seg(d):
    return (d['splits'], d['k_seg'], d['last'])
  assert seg(plans['dx_two_segments']['chunks'][0]['dx']) == (2, 272, 244)
  assert seg(plans['dx_scalar']['chunks'][0]['dx']) == (2, 272, 247)
  assert plans['dx_scalar']['chunks'][0]['dx']['K'] == 519
  d = plans['dx_256_rows']['chunks'][0]['dx']
  assert (d['M'], d['kind'], d['N'] - 128) == (256, 'det', 2)
  d = plans['dx_257_rows']['chunks'][0]['dx']
  assert (d['M'], d['kind']) == (257, 'store')
  assert seg(plans['dx_12_segments']['chunks'][0]['dx']) == (12, 256, 256)
  assert seg(plans['dx_split_cap']['chunks'][0]['dx']) == (12, 288, 168)
  assert seg(plans['dpool_two_segments']['attn']['dpool']) == (2, 256, 256)
  assert seg(plans['dpool_short_last']['attn']['dpool']) == (2, 272, 244)
  assert seg(plans['dpool_four_segments']['attn']['dpool']) == (4, 256, 256)
  d = plans['dpool_257_rows']['attn']['dpool']
  assert (d['M'], d['kind']) == (257, 'acc')
  assert seg(plans['emb_two_segments']['chunks'][0]['dx']) == (2, 272, 244)
  assert seg(plans['emb_four_segments']['chunks'][0]['dx']) == (4, 272, 216)
  assert seg(plans['emb_scalar']['chunks'][0]['dx']) == (2, 272, 247)
  assert seg(plans['repeat_split']['chunks'][0]['dx']) == (2, 272, 256)
  assert plans['attn_colsum_two_slabs']['sum_T'] == 513 and plans['attn_colsum_two_slabs']['attn']['colsum_slabs'] == 2
  # the chunked case: split and unsplit d(input) chunks in one backward, chunks on both sides of 256
  # rows; only the last weight-gradient launch is not `beside`, and it is the row-split one
  ch = plans['dx_chunked']['chunks']
  assert [c['rows'] for c in ch] == [165, 230, 300, 520]
  assert [c['dx']['kind'] for c in ch] == ['det', 'det', 'store', 'store']
  assert [c['dx']['splits'] for c in ch] == [3, 3, 1, 1]
  assert [c['tn']['beside'] for c in ch] == [True, True, True, False]
  assert [c['tn']['accumulate'] for c in ch] == [False, True, True, True]
  assert [c['tn']['splits'] for c in ch] == [1, 1, 1, 2]
  assert ch[0]['tail_rows'] == 65       # the resident tail's steps (30 + 20 + 10 + 5 rows) close inside the first chunk
  # one 16-row chunk, masked, on the tall tile
  tn = plans['tn_one_chunk_tall']['chunks'][0]['tn']
  assert (tn['bm'], tn['rows'], tn['chunks16'], tn['masked_last']) == (192, 5, 1, True)


def test_the_table_reaches_the_whole_vocabulary():
  reached = set()
  for case in ss.CASES:
    reached |= ss.side_tags(ss.case_plan(case))
  for cls, pool, I, H, S, T in ss.TALL_TILE_CASES:
    counts = ss.counts_of(ss.tall_tile_lens(np.random.RandomState(5 + H + S), S, T))
    reached |= ss.side_tags(ss.plan(counts, I, H, pool, 'padded', dict(tn_rows_bm=192)))
  assert reached <= ss.VOCABULARY, sorted(reached - ss.VOCABULARY)
  unreachable = set(ss.UNREACHABLE)
  assert not (reached & unreachable), sorted(reached & unreachable)
  assert reached | unreachable == ss.VOCABULARY, sorted(ss.VOCABULARY - reached - unreachable)


def test_the_unreachable_set_is_the_one_argued():
  """An explicit list of at most two entries: the atomic split's many-tiles arm (and, if the step
  kernels refused H = 1112, the kDetSplitMax cap — they do not, dx_split_cap reaches it)."""
  assert set(ss.UNREACHABLE) == {'Atomic unsplit many tiles'}
  assert len(ss.UNREACHABLE) <= 2 and all(len(r) > 40 for r in ss.UNREACHABLE.values())
  # the arm really needs that many rows: 512 tiles of 128 x 128
  assert ss.side_tags(ss.plan([21760], 300, 176, 'seq2seq', 'tokens', dict(bwd_chunk_rows=1 << 30))) >= {'Atomic split emb'}
  assert ss.side_tags(ss.plan([21761], 300, 176, 'seq2seq', 'tokens', dict(bwd_chunk_rows=1 << 30))) >= {'Atomic unsplit many tiles'}


def test_tall_tile_test_docstring_claims():
  """test_gpu_gru.py test_weight_gradient_tall_tile_vs_small_tile: the comments of its table."""
  plans = []
  for cls, pool, I, H, S, T in ss.TALL_TILE_CASES:
    counts = ss.counts_of(ss.tall_tile_lens(np.random.RandomState(5 + H + S), S, T))
    plans.append({bm: ss.plan(counts, I, H, pool, 'padded', dict(tn_rows_bm=bm)) for bm in (128, 192)})
  # 3H = 192: one tall tile, N < 128
  tn = plans[0][192]['chunks'][0]['tn']
  assert tn['bm'] == 192 and not tn['ragged_m'] and tn['grid'] == 2 and all(N < 128 for _, N in tn['problems'])
  # 3H = 384: two tall tiles; rows split into parts
  tn = plans[1][192]['chunks'][0]['tn']
  assert (3 * 128) // 192 == 2 and tn['splits'] > 1, tn
  assert 'TnRows row split' in ss.side_tags(plans[1][192])
  # 3H = 120: a tall tile forced onto a ragged M
  assert 'TnRows forced tall ragged M' in ss.side_tags(plans[2][192])
  # N = 130: a second column tile of 2 columns; row counts that are not a multiple of 16
  tn = plans[3][192]['chunks'][0]['tn']
  assert tn['problems'][0] == (576, 130) and not tn['ragged_m']
  assert (tn['rows'], tn['splits']) == (744, 2)
  assert any(p[192]['chunks'][0]['tn']['masked_last'] for p in plans)
  # the knob moves the tile height and nothing else of the launch's shape rule
  for p in plans:
    assert p[128]['chunks'][0]['tn']['bm'] == 128 and p[192]['chunks'][0]['tn']['bm'] == 192


def test_time_chunk_test_docstring_claims():
  """test_gpu_gru.py test_weight_gradients_in_time_chunks_beside_the_chain: several chunks that
  close every >= 1024 rows, 'every launch is row-split', 'the last one mid-tile'."""
  S, T, I, H = ss.TIME_CHUNK_SHAPE
  lens = ss.time_chunk_lens(np.random.RandomState(77), S, T)
  counts = ss.counts_of(lens)
  assert sum(counts) > 3 * 1024
  assert ss.KNOBS['bwd_chunk_rows'] != ss.TIME_CHUNK_ROWS
  assert len(ss.plan(counts, I, H, 'maxout', 'padded')['chunks']) == 2      # (default 2048: two chunks)
  for pool, cls in ss.TIME_CHUNK_CASES:
    pl = ss.plan(counts, I, H, pool, 'padded', dict(bwd_chunk_rows=ss.TIME_CHUNK_ROWS))
    ch = pl['chunks']
    assert len(ch) >= 3, [c['rows'] for c in ch]
    assert all(c['rows'] >= ss.TIME_CHUNK_ROWS for c in ch[:-1])
    assert all(tn['splits'] > 1 for tn in ss.tn_launches(pl)), [tn['splits'] for tn in ss.tn_launches(pl)]
    assert all(tn['bm'] == ss.TN_BM_SMALL and tn['ragged_m'] for tn in ss.tn_launches(pl))   # 3H = 216 rows of C
    # chunks of 1179, 1124 and 1264 rows: the chunk of the LAST time steps (launched first) and the
    # one after it end mid-tile (11 and 4 rows into a 16-row tile); the one that closes at t = 0 is
    # whole tiles, so the docstring's "the last one mid-tile" holds for the last steps' chunk only
    assert [c['rows'] % ss.BK for c in ch] == [11, 4, 0], [c['rows'] for c in ch]
    assert [c['tn']['masked_last'] for c in ch] == [True, True, False]
    assert [c['tn']['accumulate'] for c in ch] == [False] + [True] * (len(ch) - 1)
    assert [c['tn']['beside'] for c in ch] == [True] * (len(ch) - 1) + [False]


def test_scratch_sizes_cover_what_the_rule_launches():
  """det_split_scratch_bytes and wg_part_floats (bwd.hip, restated) against every modelled split:
  the partials of all segments / all row parts fit the workspace region they are written to."""
  plans = [ss.case_plan(c) for c in ss.CASES]
  S, T, I, H = ss.TIME_CHUNK_SHAPE
  counts = ss.counts_of(ss.time_chunk_lens(np.random.RandomState(77), S, T))
  plans += [ss.plan(counts, I, H, pool, 'padded', dict(bwd_chunk_rows=ss.TIME_CHUNK_ROWS))
            for pool, _ in ss.TIME_CHUNK_CASES]
  # a sweep over widths and row counts around every crossover
  for H_ in (171, 172, 256, 344, 512, 516, 1024, 1112):
    for rows in (1, 127, 255, 256, 257, 511, 512, 513, 1023, 1024, 2047):
      for I_ in (17, 130, 300):
        for pool in ('attention', 'maxout'):
          plans.append(ss.plan([rows], I_, H_, pool, 'padded'))
  n_det = n_split = 0
  for pl in plans:
    I, H, sum_T = pl['I'], pl['H'], pl['sum_T']
    scratch = ss.det_split_scratch_floats(sum_T, max(I, H))
    dets = [c['dx'] for c in pl['chunks'] if c['dx'] is not None] + ([pl['attn']['dpool']] if pl['attn'] else [])
    for d in dets:
      if d['kind'] == 'det':
        n_det += 1
        assert d['splits'] * d['M'] * d['N'] <= scratch, (pl['pool'], I, H, sum_T, d)
        assert 2 <= d['splits'] <= ss.DET_SPLIT_MAX and d['k_seg'] % 16 == 0 and 0 < d['last'] <= d['k_seg']
    part = ss.wg_part_floats(sum_T, I, H)
    for tn in ss.tn_launches(pl):
      if tn['splits'] > 1:
        n_split += 1
        assert tn['splits'] * tn['per_split'] <= part, (pl['pool'], I, H, sum_T, tn)
        assert tn['seg'] % ss.BK == 0 and (tn['splits'] - 1) * tn['seg'] < tn['rows'] <= tn['splits'] * tn['seg']
  assert n_det > 50 and n_split > 50, (n_det, n_split)


def test_oracle_side_helpers_against_brute_force():
  """d table = scatter-add of dx by clamped id; d rows = sum over the steps (float64 loops)."""
  rng = np.random.RandomState(3)
  lens = np.array([4, 3, 3, 1])
  vocab, I = 5, 3
  dx = rng.standard_normal((4, 4, I))
  tok = ss.case_tokens(rng, lens, vocab)
  assert tok[0, 0] == -1 and tok[1, 1] == vocab + 3
  want = np.zeros((vocab, I))
  want_rows = np.zeros((4, I))
  for s in range(4):
    for t in range(lens[s]):
      row = min(max(int(tok[s, t]), 0), vocab - 1)
      for i in range(I):
        want[row, i] += dx[s, t, i]
        want_rows[s, i] += dx[s, t, i]
  np.testing.assert_allclose(ss.d_table_from_dx(dx, tok, lens, vocab), want, rtol=0, atol=1e-15)
  np.testing.assert_allclose(ss.d_rows_from_dx(dx, lens), want_rows, rtol=0, atol=1e-15)
  # the out-of-range ids land in rows 0 and vocab - 1, and padding steps add nothing
  only = np.zeros_like(dx)
  only[0, 0], only[1, 1], only[3, 2] = 1.0, 2.0, 99.0       # (3, 2) is past lens[3]
  got = ss.d_table_from_dx(only, tok, lens, vocab)
  assert (got[0] == 1.0).all() and (got[vocab - 1] == 2.0).all() and got.sum() == 3.0 * I
  # the token-fed cases really repeat ids: more valid steps than table rows touched, many times over
  big = ss.case_tokens(np.random.RandomState(1), ss.lens_of((40, 36, 30, 20, 10)))
  assert len(np.unique(ss.clamp_ids(big, ss.VOCAB))) <= ss.VOCAB < 136
