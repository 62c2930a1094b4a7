"""Case tables and input builders of tests/test_gpu_loss_shapes.py: the loss kernels at training
shapes (GroupWiseContrastiveLoss, EuclideanLoss, F.normalize, the step's fused contrastive terms).

Which loop trip, tile or GEMM form a loss call takes is decided by its sizes alone; the GPU tests
cannot see that from their results.  tests/test_loss_shapes_cpu.py proves from this module that
every row of the tables has the property it names, that the dyadic inputs are exact in fp32 and
that the random inputs keep every hinge away from its kink, so the GPU comparison needs no mask."""
import functools
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'cmhse_amd', 'csrc')

# constants of the sources the tables rely on (checked by tests/test_loss_shapes_cpu.py)
K_THREADS = 256        # nt_core.hpp kThreads: the stride of the group-wise block loops
SIM_SMALL_MAX = 512    # sim.hip kSimSmallMax: stored-score matrices above it use 128 x 128 tiles
LOSS_BLOCK_ROWS = 64   # loss_layout.hpp (n + 63) / 64: rows per workgroup of contrastive_partial_kernel
STEP_LOSS_MAX = 8      # cmhse_hip.h CMHSE_STEP_LOSS_MAX

DYADIC_MARGIN = 0.25
# the GPU test holds `reduced` to REDUCED_ATOL (the project's cosine_sim tolerance), so a hinge
# argument margin + red_ij - red_ii moves by at most twice that; KINK_CLEARANCE clears it
REDUCED_ATOL = 2e-6
KINK_CLEARANCE = 1e-5


def source_constants():
  """The constants above and the `vec` condition of cmhse_groupwise_bwd, as the sources state them."""
  def read(*p):
    return open(os.path.join(*p)).read()

  def const(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]
  sim, loss, layout = read(CSRC, 'sim.hip'), read(CSRC, 'loss.hip'), read(CSRC, 'loss_layout.hpp')
  gw_fwd = layout[layout.index('LossFwdLayout groupwise_fwd_layout('):]    # the group-wise loss's nrb
  gw_fwd = gw_fwd[:gw_fwd.index('\n}\n')]
  gw_bwd = loss[loss.index('extern "C" int cmhse_groupwise_bwd'):]
  gw_bwd = gw_bwd[:gw_bwd.index('\n}\n')]
  return dict(
      kThreads=int(const(read(CSRC, 'nt_core.hpp'), r'constexpr int kThreads = (\d+);')),
      kSimSmallMax=int(const(sim, r'constexpr int kSimSmallMax = (\d+);')),
      loss_blocks=const(gw_fwd, r'loss_fwd_layout\([^;]*, (\(B \+ 63\) / 64)\);'),
      vec=const(gw_bwd, r'const bool vec = ([^;]+);'),
      step_loss_max=int(const(read(REPO, 'include', 'cmhse_hip.h'), r'#define CMHSE_STEP_LOSS_MAX (\d+)')))


# ------------------------------------------------------------------------------------------------
# GroupWiseContrastiveLoss
# ------------------------------------------------------------------------------------------------
# (id, B, counts, D, seed, what it is there for).  `counts` is the recipe of gw_counts: 'lo' / 'hi'
# draw every video's clip count, 'force' pins some, 'each' sets all, 'list' is literal, 'caps'
# = 'perm' makes num_caps a permutation of num_clips (same total), else num_caps = num_clips.
GW_CASES = [
    ('big_blocks', 33, dict(lo=1, hi=27, force=((0, 27), (1, 20))), 64, 5,
     'blocks of 729 and 540 elements: second and third trip of the strided loops, cross-thread arg-max'),
    ('batch128', 128, dict(lo=1, hi=6), 64, 2, 'the upstream default batch; nrb = 2'),
    ('b64', 64, dict(lo=1, hi=8), 30, 2, 'the 64-row loss-block edge; scalar-load GEMMs (D % 4 != 0)'),
    ('b65', 65, dict(lo=1, hi=8), 30, 2, 'one row past the 64-row loss block; scalar-load GEMMs'),
    ('vec_big_tile', 130, dict(each=4), 64, 2,
     'n = 520 > 512 takes the 128 x 128 store tile; n % 4 == 0 and D % 4 == 0 take the float4 TN GEMMs'),
    ('scalar_big_tile', 129, dict(each=4, force=((0, 3), (1, 3), (2, 3))), 36, 2,
     'n = 513: the same tile with n % 4 != 0'),
    ('unequal', 40, dict(lo=1, hi=9, caps='perm'), 64, 2, 'row_off != col_off'),
    ('singletons', 70, dict(each=1), 8, 2, 'degenerates to ContrastiveLoss'),
    ('one_video', 1, dict(list=(5,)), 8, 2, 'B = 1: loss 0 and gradient 0'),
    ('two_videos', 2, dict(list=(1, 3)), 8, 2, 'the smallest batch with a negative'),
    ('wide', 9, dict(lo=1, hi=5), 1024, 2, "the workload's embedding width"),
]
GW_BY_ID = {c[0]: c for c in GW_CASES}

# what the CPU test checks of each row: largest block (elements), B vs 64, n vs 512, n % 4, D % 4
GW_PROPERTIES = {
    'big_blocks': dict(max_block_over=2 * K_THREADS, blocks_over_256=3, n_range=(430, 470)),
    'batch128': dict(B_over_64=True, n_range=(380, 520)),
    'b64': dict(B_over_64=False, D_mod4=False),
    'b65': dict(B_over_64=True, D_mod4=False),
    'vec_big_tile': dict(n=520, n_over_512=True, n_mod4=True, D_mod4=True),
    'scalar_big_tile': dict(n=513, n_over_512=True, n_mod4=False, D_mod4=True),
    'unequal': dict(unequal=True, n_over_512=False),
    'singletons': dict(max_block=1, B_over_64=True),
    'one_video': dict(n=5),
    'two_videos': dict(n=4),
    'wide': dict(D=1024),
}

# a forced tie of big_blocks' dyadic inputs inside block (0, 0), 27 x 27: clip rows 2 and 11 and
# caption rows 3 and 16 of video 0 are each other's copies, so the block's maximum sits at elements
# (2, 3), (2, 16), (11, 3), (11, 16); the first and the last are 9 * 27 + 13 = 256 elements apart,
# i.e. two candidates of ONE thread of the strided scan.
TIE_ROWS, TIE_COLS = (2, 11), (3, 16)


def gw_counts(name):
  """(num_clips, num_caps) of a case, drawn from its seed."""
  _, B, spec, D, seed, _ = GW_BY_ID[name]
  rng = np.random.RandomState(1000 + seed)
  if 'list' in spec:
    nc = list(spec['list'])
  elif 'each' in spec:
    nc = [spec['each']] * B
  else:
    nc = [int(v) for v in rng.randint(spec['lo'], spec['hi'] + 1, size=B)]
  for i, v in spec.get('force', ()):
    nc[i] = v
  assert len(nc) == B
  ncap = list(nc)
  if spec.get('caps') == 'perm':
    ncap = [nc[i] for i in rng.permutation(B)]
  return nc, ncap


def gw_runs():
  """(case id, max_violation, norm, input kind) of every GPU test: all four modes of every case,
  dyadic inputs for max_violation, random ones for the mean, and one dyadic mean run each of
  big_blocks and batch128."""
  runs = []
  for c in GW_CASES:
    for mv in (False, True):
      for norm in (False, True):
        runs.append((c[0], mv, norm, 'dyadic' if mv else 'random'))
  runs += [('big_blocks', False, True, 'dyadic'), ('batch128', False, True, 'dyadic')]
  return runs


def run_id(run):
  return '%s-%s-norm%d-%s' % (run[0], 'max' if run[1] else 'mean', run[2], run[3])


@functools.lru_cache(maxsize=None)
def gw_dyadic(name):
  """(num_clips, num_caps, a, b, margin): every entry a small integer over a power of two, so every
  dot product is exact in fp32 and fp64 in any summation order; scores are O(1)."""
  _, B, _, D, seed, _ = GW_BY_ID[name]
  nc, ncap = gw_counts(name)
  n = sum(nc)
  rng = np.random.RandomState(seed)
  a = rng.randint(-8, 9, size=(n, D)).astype(np.float32) / 8
  b = rng.randint(-8, 9, size=(n, D)).astype(np.float32) / 8
  vid = rng.randint(-8, 9, size=(B, D)).astype(np.float32) / 8
  a = a / 2 + np.repeat(vid, nc, 0) / 2
  b = b / 2 + np.repeat(vid, ncap, 0) / 2
  if name == 'big_blocks':
    u = np.where(rng.randint(0, 2, size=D) > 0, 1.0, -1.0).astype(np.float32)
    a[list(TIE_ROWS)] = u      # |entry| = 1 everywhere: no other pair of rows reaches u . u
    b[list(TIE_COLS)] = u
  a = a * np.float32(2.0 ** -np.ceil(np.log2(D)))
  a.setflags(write=False)
  b.setflags(write=False)
  return nc, ncap, a, b, DYADIC_MARGIN


def _reduced64(a, b, nc, ncap, max_violation):
  sc = a.astype(np.float64) @ b.astype(np.float64).T
  ro = np.concatenate([[0], np.cumsum(nc)])
  co = np.concatenate([[0], np.cumsum(ncap)])
  red = np.empty((len(nc), len(nc)))
  for i in range(len(nc)):
    for j in range(len(nc)):
      blk = sc[ro[i]:ro[i + 1], co[j]:co[j + 1]]
      red[i, j] = blk.max() if max_violation else blk.mean()
  return red


def kinks_of(red):
  """Every margin at which a hinge of the contrastive loss on `red` switches: red_ii - red_ij and
  red_jj - red_ij for i != j."""
  d = np.diag(red)
  off = ~np.eye(len(red), dtype=bool)
  return np.concatenate([(d[:, None] - red)[off], (d[None, :] - red)[off]])


def pick_margin(kinks, min_share=0.1, default=0.2):
  """The fp32 value nearest the middle of the widest gap between two neighbouring kinks inside
  (0.05, 1) that leaves at least `min_share` of the hinges active and as many inactive (a hinge
  is active when its kink lies below the margin).  The widest gap of all usually sits in the sparse
  lower tail, where next to no hinge is active."""
  k = np.sort(kinks)
  n = len(k)
  if n < 2:
    return default
  ok = (k[:-1] > 0.05) & (k[1:] < 1.0)
  below = np.arange(1, n)          # kinks below a margin placed in gap i
  fair = ok & (below >= min_share * n) & (below <= (1 - min_share) * n)
  ok = fair if fair.any() else ok
  if not ok.any():
    return default
  i = int(np.where(ok, np.diff(k), -1.0).argmax())
  return float(np.float32((k[i] + k[i + 1]) / 2))


@functools.lru_cache(maxsize=None)
def gw_random(name):
  """(num_clips, num_caps, a, b, margin): video centroid + 0.7 noise, captions = clips + 0.7 noise,
  L2-normalised fp32 rows; the margin sits in the widest gap between the hinge kinks of the block
  mean, so fp32 rounding of the scores cannot move a hinge across its kink.  (Most kinks of these
  inputs lie at 0.6 - 0.9: a margin below 0.5 would leave next to no hinge active.)"""
  _, B, _, D, seed, _ = GW_BY_ID[name]
  nc, ncap = gw_counts(name)
  n = sum(nc)
  rng = np.random.RandomState(seed + 50)
  vid = rng.standard_normal((B, D))
  a = np.repeat(vid, nc, 0) + 0.7 * rng.standard_normal((n, D))
  b = a + 0.7 * rng.standard_normal((n, D))
  a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
  b = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)
  margin = pick_margin(kinks_of(_reduced64(a, b, nc, ncap, False)))
  a.setflags(write=False)
  b.setflags(write=False)
  return nc, ncap, a, b, margin


@functools.lru_cache(maxsize=None)
def gw_inputs(name, kind, max_violation):
  """(num_clips, num_caps, a, b, margin) of a run.  Dyadic max runs use DYADIC_MARGIN, where the
  whole hinge arithmetic is exact.  A dyadic mean run has exact scores but block means that are no
  dyadic numbers, and at 0.25 every one of its hinges would be active: its margin is picked from
  the kinks like that of the random inputs."""
  if kind == 'random':
    return gw_random(name)
  nc, ncap, a, b, margin = gw_dyadic(name)
  if not max_violation:
    margin = pick_margin(kinks_of(_reduced64(a, b, nc, ncap, False)))
  return nc, ncap, a, b, margin


# ------------------------------------------------------------------------------------------------
# EuclideanLoss and F.normalize
# ------------------------------------------------------------------------------------------------
_E_ROWS, _E_COLS = (1, 255, 256, 257, 1000), (1, 3, 256, 257, 2048)
# first and last row and column of the grid, and its diagonal: row counts on either side of the
# 256-thread final reduction, columns on either side of the 256-thread row loop
EUCLID_SHAPES = sorted({(r, c) for r in _E_ROWS for c in _E_COLS
                        if r in (_E_ROWS[0], _E_ROWS[-1]) or c in (_E_COLS[0], _E_COLS[-1])} |
                       set(zip(_E_ROWS, _E_COLS)))


def euclid_inputs(rows, cols):
  """(a, pool, idx): the target of row r is pool[idx[r]], a row of a larger tensor; no row of `a`
  equals its target (dist = 0 is a NaN upstream and here)."""
  rng = np.random.RandomState(rows * 7 + cols)
  a = rng.standard_normal((rows, cols)).astype(np.float32)
  pool = rng.standard_normal((rows + 9, cols)).astype(np.float32)
  idx = np.sort(rng.choice(rows + 9, rows, replace=False))
  assert (np.abs(a - pool[idx]).max(axis=1) > 0).all()
  return a, pool, idx


# row 0 all zero and row 1 of norm 1e-20 (below F.normalize's 1e-12 clamp) wherever rows >= 2
NORMALIZE_SHAPES = [(1, 1), (3, 255), (3, 256), (3, 257), (5, 1024), (2, 2049), (300, 33)]


def normalize_inputs(rows, cols):
  """(x, g) float32."""
  rng = np.random.RandomState(rows * 11 + cols)
  x = rng.standard_normal((rows, cols)) * rng.uniform(0.5, 4.0, size=(rows, 1))
  if rows >= 2:
    x[0] = 0.0
    x[1] *= 1e-20 / np.linalg.norm(x[1])
  return x.astype(np.float32), rng.standard_normal((rows, cols)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the step's fused contrastive terms (cmhse_step_losses_*, cmhse_contrastive_blocks_*)
# ------------------------------------------------------------------------------------------------
# (id, rows of every embedding, D, terms (a, b, weight), norm, seed, what it is there for)
STEP_CASES = [
    ('eight_terms', (32, 32, 1, 1, 130, 130, 7, 7), 30,
     ((0, 1, 1.0), (2, 3, 1.0), (4, 5, 1.0), (6, 7, 0.25), (0, 0, 0.5), (4, 4, 0.5), (1, 1, 0.5),
      (5, 5, 2.0)), False, 3,
     'CMHSE_STEP_LOSS_MAX embeddings and terms; norm=False; D % 4 != 0; 1-row blocks'),
    ('big_beside_one_row', (520, 520, 1, 1), 64, ((0, 1, 1.0), (2, 3, 1.0), (0, 0, 0.5)), True, 5,
     'max_n > 512 (128 x 128 store tile) beside a block of 1 row: shared max_n tiles and strides'),
]


@functools.lru_cache(maxsize=None)
def step_inputs(name):
  """(raw embeddings float32, margin).  Rows come in clusters of 8 around a centroid (the clips of
  a video), odd embeddings are their left neighbour + 0.8 noise (the step's clip / caption pairs),
  every embedding at its own scale.  Only the hinges inside a cluster have kinks below 0.5, few
  enough even at 520 rows for a gap that clears fp32 rounding; the margin sits in the widest one."""
  _, rows, D, terms, _, seed, _ = [c for c in STEP_CASES if c[0] == name][0]
  rng = np.random.RandomState(seed)
  raw = []
  for e, n in enumerate(rows):
    x = rng.standard_normal((n, D))
    if e % 2 == 1:
      x = raw[e - 1] / (0.5 + e - 1) + 0.8 * x
    else:
      x = np.repeat(rng.standard_normal(((n + 7) // 8, D)), 8, 0)[:n] + 0.5 * x
    raw.append((x * (0.5 + e)).astype(np.float32))
  kinks = np.concatenate([kinks_of(s) for s in step_scores64(raw, terms) if len(s) > 1])
  margin = pick_margin(kinks[kinks < 0.5], min_share=0.25)
  for x in raw:
    x.setflags(write=False)
  return tuple(raw), margin


def step_scores64(raw, terms):
  y = [x.astype(np.float64) for x in raw]
  y = [x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12) for x in y]
  return [y[a] @ y[b].T for a, b, _ in terms]


def hinge_clearance(red, margin, max_violation):
  """How far the fp64 hinges of the contrastive loss on `red` are from changing their active set:
  the smallest |margin + red_ij - red_ii| and |margin + red_ij - red_jj| over i != j; for
  max_violation also the smallest gap between the two largest costs of a row / column whose
  largest cost is positive (the hardest negative is an arg-max)."""
  n = len(red)
  if n < 2:
    return np.inf
  clear = np.abs(margin - kinks_of(red)).min()
  if max_violation:
    d = np.diag(red)
    eye = np.eye(n, dtype=bool)
    for cost in (np.where(eye, 0, np.maximum(margin + red - d[:, None], 0)),
                 np.where(eye, 0, np.maximum(margin + red - d[None, :], 0)).T):
      if n > 2:
        top = np.sort(np.where(eye, -np.inf, cost), axis=1)[:, -2:]
        live = top[:, 1] > 0
        if live.any():
          clear = min(clear, (top[live, 1] - top[live, 0]).min())
  return float(clear)
