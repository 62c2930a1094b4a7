"""The cases of tests/test_gpu_score_shapes.py reach the launches they name (no GPU needed): the tile
deal and the panel walk of the scoring kernels as tests/score_shapes.py restates them — constants
checked against the sources, the block maps proved to be bijections by brute force, the workspace
sizes compared with the library's — applied to the case tables and to the shapes of the older
scoring tests, whose docstring claims about panels are checked here; and the references of the GPU
file stay inside their own conditions on the inputs it uses (lattice scores exact, the float64
margins within the 1 % cap, the score bar below half the certified tolerance)."""
import numpy as np
import pytest

import score_shapes as ss


@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def test_rule_constants_match_the_sources():
  src = ss.source_constants()
  assert (src['kXcds'], src['kWgsPerXcd']) == (ss.XCDS, ss.WGS_PER_XCD)
  assert (src['kSimBM'], src['kSimBN'], src['kSimSmallMax']) == (ss.SIM_BM, ss.SIM_BN, ss.SIM_SMALL_MAX)
  assert (src['kTkBM'], src['kTkBN'], src['kTkCUs'], src['kTkLdsPerCU']) == (ss.TK_BM, ss.TK_BN, ss.TK_CUS, ss.TK_LDS_PER_CU)
  assert (src['kGrBM'], src['kGrBN'], src['kGrRankT']) == (ss.GR_BM, ss.GR_BN, ss.GR_RANK_T)
  assert (src['kGtCUs'], src['kGtLdsPerCU'], src['kGtQcapMax']) == (ss.GT_CUS, ss.GT_LDS_PER_CU, ss.GT_QCAP_MAX)
  assert (src['kGtHdr'], src['kGrHdr']) == (ss.GT_HDR, ss.GR_HDR)
  assert (src['kLdsLd'], src['kBK'], src['kThreads']) == (ss.LDS_LD, ss.BK, ss.THREADS)
  assert src['CMHSE_TOPK_MAX'] == ss.TOPK_MAX
  # the numbers group.hip's comment states for gt_qcap
  assert [ss.gt_qcap(k) for k in (1, 10, 50, 128)] == [64, 56, 40, 64]
  assert [ss.gt_smem(k) // 1024 for k in (1, 10, 50, 128)] == [76, 76, 79, 140]
  assert ss.sim_store_tile(512, 512) == 64 and ss.sim_store_tile(513, 8) == 128 and ss.sim_store_tile(8, 513) == 128


# --------------------------------------------------------------------------------------------
# the block maps are bijections
# --------------------------------------------------------------------------------------------
MAX_ROW_TILES, MAX_COL_TILES = 48, 800


def test_the_deal_is_a_bijection_onto_the_tiles_plus_padding():
  """Every (row tiles, column tiles) up to 48 x 800, by brute force: under the G that xcd_deal
  picks, the blocks [0, blocks) visit every tile exactly once, and every other block is padding (a
  row tile past the last).  For a fixed (G, column tiles) the block -> tile map does not depend on
  the row tiles, so it is evaluated once per pair over the largest grid and each row-tile count then
  reads it: no block below `blocks` repeats a tile, every tile's block lies below `blocks`."""
  arms = {0: 0, 2: 0, 3: 0, 4: 0}
  for C in range(1, MAX_COL_TILES + 1):
    deals = {R: ss.xcd_deal(R, C) for R in range(1, MAX_ROW_TILES + 1)}
    for G in (2, 3, 4):
      mine = [R for R, d in deals.items() if d[0] == G]
      if not mine:
        continue
      top = max(deals[R][1] for R in mine)
      blocks = np.arange(top, dtype=np.int64)
      rt, ct = ss.xcd_deal_tile(blocks, G, C)
      assert ct.min() >= 0 and ct.max() < C and rt.min() >= 0
      key = rt * C + ct
      assert np.unique(key).size == top, (G, C)                 # no tile twice, whatever the grid
      first_block = np.full((int(rt.max()) + 1) * C, top, dtype=np.int64)
      first_block[key] = blocks
      last_needed = np.maximum.accumulate(first_block.reshape(-1, C).max(axis=1))   # by row tile
      for R in mine:
        n = deals[R][1]
        assert n % (8 * G) == 0 and n >= R * C
        assert R - 1 < last_needed.size and last_needed[R - 1] < n, (G, R, C)      # every tile has a block
        assert np.count_nonzero(rt[:n] < R) == R * C, (G, R, C)                    # ... the rest is padding
        arms[G] += 1
    for R, (G, n) in deals.items():
      if G == 0:
        assert n == R * C
        arms[0] += 1
  # the plain order: block = rt * C + ct
  assert [ss.deal_tile(b, 0, 3, 5) for b in range(15)] == [(r, c) for r in range(3) for c in range(5)]
  assert sum(arms.values()) == MAX_ROW_TILES * MAX_COL_TILES and min(arms.values()) > 500, arms
  # the scalar form the GPU cases are read with agrees with the array form
  assert [ss.deal_tile(b, 3, 5, 97) for b in range(600)].count(None) == 600 - 5 * 97


def test_the_panel_grid_is_a_bijection_and_the_panels_cover_the_tiles():
  for q_tiles in (1, 2, 7, 19, 21, 100, 257):
    for panels in (1, 2, 5, 12, 36, 53):
      blocks = ss.ceil_div(q_tiles * panels, 8) * 8
      seen = [ss.panel_block(b, blocks, q_tiles, panels) for b in range(blocks)]
      real = [s for s in seen if s is not None]
      assert len(real) == q_tiles * panels == len(set(real))
      assert set(real) == {(p, q) for p in range(panels) for q in range(q_tiles)}
  for tiles in range(1, 200):
    for panels in range(1, tiles + 1):
      b = ss.panel_bounds(tiles, panels)
      assert b[0][0] == 0 and b[-1][1] == tiles
      assert all(x[1] == y[0] for x, y in zip(b[:-1], b[1:])) and all(e > s for s, e in b)


# --------------------------------------------------------------------------------------------
# coverage
# --------------------------------------------------------------------------------------------
def test_every_case_reaches_its_targets():
  tags = ss.all_case_tags()
  for table in (ss.COUNT_CASES, ss.GROUP_CASES, ss.TOPK_CASES, ss.GTOPK_CASES):
    for case in table:
      targets = case[-1]
      assert targets <= ss.VOCABULARY, (case[0], sorted(targets - ss.VOCABULARY))
      assert targets <= tags[case[0]], (case[0], sorted(targets - tags[case[0]]))


def test_the_tables_reach_the_whole_vocabulary():
  reached = set().union(*ss.all_case_tags().values())
  assert reached <= ss.VOCABULARY, sorted(reached - ss.VOCABULARY)
  unreachable = set(ss.UNREACHABLE)
  assert not (reached & unreachable)
  assert reached | unreachable == ss.VOCABULARY, sorted(ss.VOCABULARY - reached - unreachable)


def test_the_unreachable_set_is_the_one_argued():
  assert set(ss.UNREACHABLE) == {'Count grid over 2^31 blocks', 'Topk LDS for less than one workgroup'}
  assert all(len(r) > 40 for r in ss.UNREACHABLE.values())
  # a grid of 2^31 blocks: 46 341 x 46 341 tiles and not one fewer
  assert ss.xcd_deal(46340, 46340)[1] <= 0x7fffffff < ss.xcd_deal(46341, 46341)[1]
  assert 46341 * ss.SIM_BM > 5900000
  # one workgroup's LDS fits a CU at every K the API accepts (so per_cu >= 1 without its floor)
  for K in range(1, ss.TOPK_MAX + 1):
    assert ss.TK_LDS_PER_CU // ss.topk_smem(K) >= 1 and ss.GT_LDS_PER_CU // ss.gt_smem(K) >= 1
  assert (ss.topk_smem(ss.TOPK_MAX), ss.gt_smem(ss.TOPK_MAX)) == (104448, 143616)


def test_the_cases_are_the_ones_the_table_states():
  """The tile counts the comments of the case tables give, and what the issue of this file asks of them."""
  plans = {c[0]: ss.count_plan(c[5], c[2]) for c in ss.COUNT_CASES}
  want = dict(g4_partial_group=(5, 40, 4), g3_one_row_tile=(1, 193, 3), g3_five_row_tiles=(5, 97, 3),
              g2_one_row_tile=(1, 257, 2), g2_thirteen_row_tiles=(13, 52, 2), g0_one_row_tile=(1, 385, 0),
              g0_five_row_tiles=(5, 129, 0), stripe_g4=(5, 40, 4), stripe_g3=(5, 97, 3), stripe_g2=(13, 52, 2),
              stripe_g0=(5, 129, 0))
  assert {k: (p['row_tiles'], p['col_tiles'], p['G']) for k, p in plans.items()} == want
  assert plans['g4_partial_group']['blocks'] == 320
  # the further shapes the issue names
  assert [ss.xcd_deal(*rc)[0] for rc in ((10, 65), (11, 65), (9, 65))] == [2, 0, 3]
  for name, N, M, D, row0, nrows, corr, _ in ss.COUNT_CASES:
    assert row0 + nrows <= N <= M and (row0 == 0 or row0 % 64 != 0)
    assert nrows * M * D <= 20000 * 20000 * 64
  assert sum(c[2] % 128 != 0 for c in ss.COUNT_CASES) > len(ss.COUNT_CASES) // 2
  assert {c[3] for c in ss.COUNT_CASES} == {8, 12, 30, 64}
  groups = {c[0]: ss.group_plan(c[1], c[2]) for c in ss.GROUP_CASES}
  assert {k: (p['row_tiles'], p['col_tiles'], p['G']) for k, p in groups.items()} == dict(
      group_g4=(5, 24, 4), group_g3=(9, 65, 3), group_g2=(10, 65, 2), group_g0=(11, 65, 0))
  for name, nclips, ncaps, D, _ in ss.GROUP_CASES:            # power-of-two counts: exact means
    assert all(x & (x - 1) == 0 for x in set(nclips) | set(ncaps))
  for case in ss.TOPK_CASES:
    name, N, M, D, K, row0, nrows, corr, _ = case
    pl = ss.topk_plan(nrows, M, K)
    assert pl['panels'] < pl['col_tiles'] and max(e - b for b, e in pl['bounds']) >= 2, name
  assert ss.topk_plan(16448, 300, 128)['uncapped'] == 0
  for case in ss.GTOPK_CASES:
    name, nclips, ncaps, D, K, direction, _ = case
    pl = ss.group_topk_plan(nclips, ncaps, direction, K)
    assert (pl['q_tiles'], pl['g_tiles'], pl['panels'], pl['qcap']) == (100, 43, 5, 56), name
    assert [e - b for b, e in pl['bounds']] == [8, 9, 8, 9, 9]
    assert all(x & (x - 1) == 0 for x in set(nclips) | set(ncaps))
  # the stripes of the concatenation tests land on other arms / panel counts than the full call
  _, N, M, D, cuts = ss.COUNT_STRIPES
  assert [ss.count_plan(hi - lo, M)['G'] for lo, hi in zip(cuts[:-1], cuts[1:])] == [4, 4, 4]
  assert ss.count_plan(N, M)['G'] == 2
  _, N, M, D, K, cuts = ss.TOPK_STRIPES
  assert [ss.topk_plan(hi - lo, M, K)['panels'] for lo, hi in zip(cuts[:-1], cuts[1:])] == [29, 28, 25]
  assert ss.topk_plan(N, M, K)['panels'] == 12


# --------------------------------------------------------------------------------------------
# workspace sizes
# --------------------------------------------------------------------------------------------
def test_workspace_sizes_equal_the_restatement(lib):
  for nrows in (1, 63, 64, 65, 150, 1200, 1290, 4917, 16448, 20000):
    for M in (1, 127, 128, 129, 300, 3700, 8300, 200000):
      for K in (1, 5, 17, 50, 52, 53, 100, 128):
        if K <= M:
          assert lib.cmhse_sim_topk_workspace(nrows, M, K) == ss.topk_plan(nrows, M, K)['workspace'], (nrows, M, K)
  rng = np.random.RandomState(4)
  shapes = [(c[1], c[2], c[4], c[5]) for c in ss.GTOPK_CASES]
  for Bv, Bp, hi, K in ((300, 120, 30, 10), (500, 700, 128, 50), (4917, 2000, 6, 128), (900, 9000, 2, 1)):
    for direction in ('p2v', 'v2p'):
      shapes.append((list(rng.randint(1, hi, Bv)), list(rng.randint(1, hi, Bp)), K, direction))
  for nclips, ncaps, K, direction in shapes:
    pl = ss.group_topk_plan(nclips, ncaps, direction, K)
    plan = pl['host_plan']
    assert lib.cmhse_group_topk_workspace(plan.ctypes.data, plan.size) == pl['workspace'], (len(nclips), len(ncaps), K)
    assert pl['most_queries'] <= pl['qcap']


# --------------------------------------------------------------------------------------------
# what the older GPU files reach, and the claims of their docstrings
# --------------------------------------------------------------------------------------------
def _existing_group_topk():
  """The top-K plans of tests/test_gpu_group_topk.py's larger tests, inputs drawn as they draw them."""
  from cmhse_amd import synthetic
  out = {}
  rng = np.random.RandomState(29)
  nclips, ncaps = list(rng.randint(1, 20, 700)), list(rng.randint(1, 20, 500))
  out['query_stripes p2v'] = ss.group_topk_plan(nclips, ncaps, 'p2v', 64)
  out['query_stripes v2p'] = ss.group_topk_plan(nclips, ncaps, 'v2p', 64)
  rng = np.random.RandomState(31)
  nclips, ncaps = list(rng.randint(1, 7, 40000)), list(rng.randint(1, 7, 2000))
  out['gallery_split'] = ss.group_topk_plan(nclips, ncaps, 'p2v', 50)
  out['all_ones'] = ss.group_topk_plan([1] * 300, [1] * 300, 'p2v', 128)
  counts = list(synthetic.anet_like_spec(4917).num_clips)
  out['val1 K=50'] = ss.group_topk_plan(counts, counts, 'p2v', 50)
  rng = np.random.RandomState(37)
  nclips, ncaps = list(rng.randint(1, 12, 900)), list(rng.randint(1, 12, 1100))
  out['repeat_calls'] = ss.group_topk_plan(nclips, ncaps, 'p2v', 100)
  return out


# counting-pass shapes (stripe rows, gallery rows) of the older GPU files
EXISTING_COUNT = {
    'test_gpu_scoring.py': [(1, 1), (129, 300), (515, 515), (257, 400), (700, 700), (350, 700), (234, 700), (88, 700),
                            (260, 523), (300, 777), (203, 203)],
    'test_gpu_rank_exact.py': [(1, 1), (129, 300), (257, 400), (515, 515), (64, 5000), (130, 780), (260, 1560),
                               (200, 1200), (300, 400), (100, 400), (157, 400), (43, 400)],
    'test_gpu_rank_labelled.py': [(1000, 3000), (500, 3000), (334, 3000), (125, 3000), (256, 20000), (200, 900),
                                  (70, 300), (5, 700)],
    'test_gpu_pipeline.py': [(615, 4917), (1230, 4917), (2459, 4917)],
    'test_gpu_fullsize.py': [(4917, 4917), (4917, 9802), (9802, 4917)],
}
# (rows, gallery, K) of tests/test_gpu_topk.py
EXISTING_TOPK = [(1, 1, 1), (129, 300, 5), (257, 400, 128), (515, 515, 50), (300, 128, 128), (64, 1000, 128),
                 (70, 300, 24), (5, 700, 40), (1000, 3000, 17), (500, 3000, 17), (334, 3000, 17), (125, 3000, 17),
                 (200, 900, 30), (90, 400, 12)]


def test_what_the_older_gpu_files_reach():
  """The record the new cases were chosen against: the deal arms and panel walks of the older tests."""
  arms = {f: sorted({ss.count_plan(n, m)['G'] for n, m in shapes}) for f, shapes in EXISTING_COUNT.items()}
  assert arms == {'test_gpu_scoring.py': [4], 'test_gpu_rank_exact.py': [4], 'test_gpu_rank_labelled.py': [4],
                  'test_gpu_pipeline.py': [4], 'test_gpu_fullsize.py': [3]}
  # G = 2 and the plain order: nowhere; G = 3: in the full-size file only
  assert not any(g in (0, 2) for a in arms.values() for g in a)
  # tests/test_gpu_topk.py: a panel is one tile in every small test ...
  for n, m, k in EXISTING_TOPK:
    pl = ss.topk_plan(n, m, k)
    assert pl['panels'] == pl['col_tiles'], (n, m, k)
  # ... and several in the two large ones
  pl = ss.topk_plan(4917, 4917, 50)
  assert (pl['panels'], pl['col_tiles']) == (6, 39) and pl['col_tiles'] % pl['panels'] != 0
  # test_sim_topk_large_gallery: "256 queries x 200 000 gallery rows, K = 100: many column panels and the merge"
  pl = ss.topk_plan(256, 200000, 100)
  assert (pl['row_tiles'], pl['panels'], pl['col_tiles']) == (4, 64, 1563)      # 64 panels of 24 or 25 tiles: true
  assert {e - b for b, e in pl['bounds']} == {24, 25}
  # tests/test_gpu_group_rank.py / test_gpu_group_topk.py: every group_scores deal is G = 4
  from test_gpu_group_rank import CASES
  for name, nclips, ncaps, d in CASES:
    assert ss.group_plan(list(nclips), list(nclips if ncaps is None else ncaps))['G'] == 4, name
  gt = _existing_group_topk()
  walk = {k: (p['q_tiles'], p['g_tiles'], p['panels']) for k, p in gt.items()}
  # one gallery tile per panel in the all-ones case; the stripes test, the repeat-calls test, the gallery-split
  # test and the val_1 test walk panels of several tiles
  assert walk['all_ones'][1] == walk['all_ones'][2]
  for k in ('query_stripes p2v', 'query_stripes v2p', 'gallery_split', 'val1 K=50', 'repeat_calls'):
    assert walk[k][1] > walk[k][2] >= 1, (k, walk[k])
  assert walk == {'query_stripes p2v': (40, 58, 12), 'query_stripes v2p': (58, 40, 8), 'gallery_split': (57, 1112, 8),
                  'all_ones': (5, 3, 3), 'val1 K=50': (139, 139, 7), 'repeat_calls': (54, 45, 9)}
  # (so an uneven split of several tiles, 58 over 12 panels, was already walked at test size on the group side —
  # against ops.group_scores, the same nt_phase, never against anything independent)
  assert 58 % 12 != 0


def test_stripes_docstring_claims():
  """The stripes tests call row stripes 'the unit a sharded evaluation would deal out' / 'the
  multi-GPU sharding unit': the stripes they cut are dealt as the sharded evaluation's are (G = 4,
  tests/test_gpu_pipeline.py's 615 / 1230 / 2459 x 4917), but not as the single-GPU full-size call
  (G = 3) — and none of them reaches G = 2 or the plain order."""
  for parts in (2, 3, 8):
    bounds = np.linspace(0, 700, parts + 1).astype(int)
    assert {ss.count_plan(int(hi - lo), 700)['G'] for lo, hi in zip(bounds[:-1], bounds[1:])} == {4}
    bounds = np.linspace(0, 1000, parts + 1).astype(int)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
      assert ss.count_plan(int(hi - lo), 3000)['G'] == 4
      pl = ss.topk_plan(int(hi - lo), 3000, 17)
      assert pl['panels'] == pl['col_tiles'] == 24
  assert {ss.count_plan(n, 4917)['G'] for n in (615, 1230, 2459)} == {4}
  assert ss.count_plan(4917, 4917)['G'] == 3
  # test_many_positives: "80 pair tiles, three and a fifth queries to a tile"
  assert 256 * 40 // ss.SIM_BM == 80 and ss.SIM_BM / 40 == 3.2 and ss.count_plan(256, 20000)['G'] == 4


# --------------------------------------------------------------------------------------------
# the references stay inside their own conditions
# --------------------------------------------------------------------------------------------
def test_score_bar_is_at_most_half_the_certified_tolerance(lib):
  tol = lib.cmhse_sim_rank_exact_tolerance
  for D in (1, 8, 12, 30, 64, 1024, 4096):
    for na in (1e-3, 1.0, 2.9, 32.0):
      for nb in (1e-3, 1.0, 2.9, 32.0):
        bar = ss.score_bar(D, na, nb)
        assert 0 < bar <= 0.5 * tol(D, na, nb), (D, na, nb)
        assert bar >= D * 2.0 ** -24 * na * nb          # nothing given away below the textbook value either


def test_reference_helpers_against_brute_force():
  rng = np.random.RandomState(1)
  S = rng.randint(-3, 4, size=(6, 9)).astype(np.int64)
  row0 = 2
  rank, top1 = ss.rank_reference(S, row0)
  lo, hi = ss.exact_reference(S, row0)
  for r in range(6):
    d = S[r, row0 + r]
    assert rank[r] == lo[r] == sum(S[r, j] > d for j in range(9))
    assert hi[r] == sum(S[r, j] >= d for j in range(9) if j != row0 + r)
    assert top1[r] == min(j for j in range(9) if S[r, j] == S[r].max())
  off, idx = np.array([0, 2, 3, 6, 7, 8, 10]), np.array([1, 4, 0, 2, 3, 8, 5, 5, 0, 7])
  lr, lt, lp, lsc = ss.labelled_reference(S, off, idx)
  for r in range(6):
    p = idx[off[r]:off[r + 1]]
    best = max(S[r, j] for j in p)
    assert lsc[r] == best and lp[r] == min(j for j in p if S[r, j] == best)
    assert lr[r] == sum(S[r, j] > best for j in range(9))
  for K in (1, 2, 4, 9):                                    # both forms: the full sort and the thresholded one
    ws, wi = ss.topk_reference(S, K)
    for r in range(6):
      order = sorted(range(9), key=lambda j: (-S[r, j], j))[:K]
      assert wi[r].tolist() == order and ws[r].tolist() == [S[r, j] for j in order]
  big = rng.randint(-2, 3, size=(5, 400)).astype(np.float64) / 4
  ws, wi = ss.topk_reference(big, 7)
  for r in range(5):
    assert wi[r].tolist() == sorted(range(400), key=lambda j: (-big[r, j], j))[:7]
  nrow, ncol = [1, 3, 2], [2, 2, 4, 1]
  for reduce, f in (('max', np.max), ('sum', np.sum)):
    got = ss.block_reduce(S, nrow, ncol, reduce)
    ro, co = np.cumsum([0] + nrow), np.cumsum([0] + ncol)
    for i in range(3):
      for j in range(4):
        assert got[i, j] == f(S[ro[i]:ro[i + 1], co[j]:co[j + 1]])
  assert ss.block_counts(nrow, ncol)[1, 2] == 12
  # the labels of the cases: a positive list per query, ascending and distinct, the pair among them
  off, idx = ss.positives_of(50, 60)
  assert off[-1] == idx.size and (np.diff(off) >= 1).all() and np.diff(off).max() == 3
  for i in range(50):
    p = idx[off[i]:off[i + 1]]
    assert i in p and (np.diff(p) > 0).all() and p.max() < 60


def test_lattice_inputs_are_exact():
  """max |score| < 2^24; where the mean is compared, every sum is an integer below 2^24 (so any
  order of adding it, in fp32 or float64, is exact) and every count a power of two."""
  for case in ss.COUNT_CASES + ss.TOPK_CASES:
    a, b = ss.count_inputs(case[0], 'lattice')
    assert np.abs(a).max() <= 2 and np.abs(b).max() <= 2 and (a == np.rint(a)).all() and (b == np.rint(b)).all()
    assert 4 * a.shape[1] < 2 ** 24                       # |score| <= 2 * 2 * D
  for case in ss.GROUP_CASES + ss.GTOPK_CASES:
    c, s = ss.group_inputs(case[0], 'lattice')
    D = c.shape[1]
    assert np.abs(c).max() <= 2 and np.abs(s).max() <= 2
    assert 4 * D * max(case[1]) * max(case[2]) < 2 ** 24  # the largest block's sum of |score|
  # the diagonal is tied many times: at D = 8 and 8320 gallery rows a row ties its diagonal hundreds of times
  a, b = ss.lattice_rows(64, 8, 1), ss.lattice_rows(8320, 8, 2)
  lo, hi = ss.exact_reference(ss.scores_int(a, b))
  assert np.median(hi - lo) > 200


@pytest.mark.parametrize('case', ss.COUNT_CASES, ids=[c[0] for c in ss.COUNT_CASES])
def test_gaussian_references_stay_within_the_cap(case):
  """On the float64 scores alone: the margin bar leaves out at most 1 % of a case's rows for the
  rank, for the labelled rank and for the top-1; fewer than half of the rows sit at rank 0; no float64
  comparison with the diagonal is closer than a float64 summation could move it."""
  name, N, M, D, row0, nrows, corr, _ = case
  a, b = ss.count_inputs(name, 'gaussian')
  rows = a[row0:row0 + nrows]
  S = ss.scores_f64(rows, b)
  bars = ss.row_bars(rows, b, D)
  assert bars.max() < 1.01 * ss.gamma(D) and ss.gamma(D) < 1.0001 * D * 2.0 ** -24
  ok_rank, ok_top = ss.margin_ok(S, bars, row0 + np.arange(nrows))
  rank, _ = ss.rank_reference(S, row0)
  off, idx = ss.positives_of(N, M)
  lo, hi = int(off[row0]), int(off[row0 + nrows])
  lrank, _, lpos, _ = ss.labelled_reference(S, off[row0:row0 + nrows + 1] - lo, idx[lo:hi])
  ok_lab, _ = ss.margin_ok(S, bars, lpos)
  share0 = np.mean(rank == 0)
  print('\n%-24s rank 0: %.1f %%, median rank %d; left out: rank %.3f %%, labelled %.3f %%, top-1 %.3f %%'
        % (name, 100 * share0, np.median(rank), 100 * (1 - ok_rank.mean()), 100 * (1 - ok_lab.mean()),
           100 * (1 - ok_top.mean())), end='')
  assert share0 < 0.5 and np.mean(lrank == 0) < 0.5
  assert rank.max() > 10
  for ok in (ok_rank, ok_lab, ok_top):
    assert 1 - ok.mean() <= 0.01
  gap = np.abs(S - S[np.arange(nrows), row0 + np.arange(nrows)][:, None])
  gap[np.arange(nrows), row0 + np.arange(nrows)] = np.inf
  assert gap.min() > 1e-12                                 # (D 2^-53 is below 1e-14 here)
