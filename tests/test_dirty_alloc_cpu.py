"""tests/dirty_alloc.py and the tables of tests/test_gpu_dirty_workspace.py can see what they claim to see
(no GPU needed).

  1. the helper on host buffers: fills land, views have the shape, dtype and alignment asked for, a byte
     written in front of or behind a block makes check_guards fail, stale() replays the recorded bytes;
  2. the seam is complete: every call of the seven wrapper modules that creates uninitialised tensor memory
     resolves through the module-level name `torch`, which dirty() replaces;
  3. the cases reach the workspace regions and launch arms they are there for, proved from the restated
     dispatch rules (fwd_shapes.call_steps, bptt_shapes.step_shapes, bwd_side_shapes.plan, the score_shapes
     plans) and from the library's own host-only size functions."""
import ast
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import bptt_shapes
import bwd_side_shapes as bss
import dirty_alloc
import fwd_shapes
import score_shapes as ss
import test_gpu_dirty_workspace as T
from dirty_alloc import GUARD, dirty, stale


# ---------------------------------------------------------------------------------------------
# 1. the helper
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def seam(monkeypatch):
  import types
  mod = types.ModuleType('dirty_alloc_cpu_holder')      # stands in for a wrapper module
  mod.torch = torch
  monkeypatch.setitem(importlib.sys.modules, mod.__name__, mod)

  def make(fill):
    return dirty(monkeypatch, fill, modules=(mod.__name__,), host=True), mod
  return make


@pytest.mark.parametrize('fill,byte', [('zero', 0x00), ('ones', 0xFF), ('a5', 0xA5)])
def test_fills_land_and_views_are_what_was_asked_for(seam, fill, byte):
  proxy, mod = seam(fill)
  assert mod.torch is proxy
  a = mod.torch.empty(3, 5, dtype=torch.float32, device='cpu')
  b = mod.torch.empty((7,), dtype=torch.int32, device='cpu')
  c = mod.torch.empty((), dtype=torch.float64, device='cpu')
  d = mod.torch.empty_like(a, dtype=torch.int64)
  e = mod.torch.empty_strided((2, 3), (3, 1), dtype=torch.uint8, device='cpu')
  z = mod.torch.empty(0, 4, dtype=torch.float32, device='cpu')
  for t, shape, dtype in ((a, (3, 5), torch.float32), (b, (7,), torch.int32), (c, (), torch.float64),
                          (d, (3, 5), torch.int64), (e, (2, 3), torch.uint8), (z, (0, 4), torch.float32)):
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 256 == 0
  assert len(proxy.blocks) == 6
  for (block, nbytes, _), t in zip(proxy.blocks, (a, b, c, d, e, z)):
    assert block.dtype == torch.uint8 and block.numel() == nbytes + 2 * GUARD
    assert nbytes == t.numel() * t.element_size()
    assert block.data_ptr() % 256 == 0
    if nbytes:                  # (an empty tensor reports a null pointer)
      assert t.data_ptr() == block.data_ptr() + GUARD
    assert bool((block == byte).all())
  if fill == 'ones':
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(c)) and bool((b == -1).all()) and bool((d == -1).all())
  if fill == 'zero':
    assert not a.any() and not b.any()
  proxy.check_guards('untouched')
  # writes inside the views leave the guards alone
  a.fill_(1.0), b.fill_(7), c.fill_(2.0), d.fill_(3), e.fill_(9)
  proxy.check_guards('written inside')
  assert bool((proxy.blocks[0][0][GUARD:GUARD + 60].view(torch.float32) == 1.0).all())


def test_everything_else_passes_through(seam):
  proxy, mod = seam('ones')
  assert mod.torch.float32 is torch.float32 and mod.torch.Tensor is torch.Tensor and mod.torch.nn is torch.nn
  assert not mod.torch.zeros(4, device='cpu').any()
  assert len(proxy.blocks) == 0
  # without host=True a CPU allocation is not the seam's business (pinned and host buffers pass through)
  plain = dirty_alloc.DirtyTorch('ones')
  t = plain.empty(5, dtype=torch.uint8)
  assert len(plain.blocks) == 0 and tuple(t.shape) == (5,)
  assert len(proxy.blocks) == 0


@pytest.mark.parametrize('fill', ['zero', 'ones', 'a5'])
@pytest.mark.parametrize('where', ['front', 'behind'])
def test_one_byte_outside_a_block_fails_the_guards(seam, fill, where):
  proxy, mod = seam(fill)
  mod.torch.empty(10, dtype=torch.float32, device='cpu')
  t = mod.torch.empty(33, dtype=torch.uint8, device='cpu')
  mod.torch.empty(4, dtype=torch.int32, device='cpu')
  proxy.check_guards('clean')
  block, nbytes, _ = proxy.blocks[1]
  at = GUARD - 1 if where == 'front' else GUARD + nbytes
  block[at] = 0x5A                                   # plain torch on the host
  with pytest.raises(AssertionError, match='in front of it' if where == 'front' else 'past its end'):
    proxy.check_guards('dirty')
  block[at] = dirty_alloc.BYTE[fill]
  proxy.check_guards('restored')
  del t


def test_stale_replays_the_recorded_bytes(seam):
  rec, mod = seam('zero')
  a = mod.torch.empty(5, dtype=torch.int32, device='cpu')
  b = mod.torch.empty(300, dtype=torch.uint8, device='cpu')
  a.copy_(torch.arange(1, 6, dtype=torch.int32))
  b.copy_((torch.arange(300) % 251).to(torch.uint8))
  mod.torch.empty(0, dtype=torch.float32, device='cpu')          # an empty block is skipped by stale()
  image = rec.image()
  assert [t.numel() for t in image] == [20, 300, 0]
  a.zero_()                                                       # the image is a copy
  assert image[0].view(torch.int32).tolist() == [1, 2, 3, 4, 5]
  proxy, mod = seam(stale(image))
  # allocation 0: image block 0 (20 bytes) repeated cyclically over guard + payload + guard
  x = mod.torch.empty(40, dtype=torch.uint8, device='cpu')
  whole = image[0].repeat(-(-(40 + 2 * GUARD) // 20))[:40 + 2 * GUARD]
  assert torch.equal(proxy.blocks[0][0], whole) and torch.equal(x, whole[GUARD:GUARD + 40])
  # allocation 1: block 1; allocation 2 cycles back to block 0 (the recorded run made two non-empty blocks)
  y = mod.torch.empty(100, dtype=torch.uint8, device='cpu')
  assert torch.equal(y, image[1].repeat(3)[GUARD:GUARD + 100])
  w = mod.torch.empty(2, dtype=torch.int32, device='cpu')
  assert torch.equal(proxy.blocks[2][0], image[0].repeat(-(-(8 + 2 * GUARD) // 20))[:8 + 2 * GUARD])
  proxy.check_guards('stale, untouched')
  x.zero_(), y.zero_(), w.zero_()
  proxy.check_guards('stale, written inside')
  proxy.blocks[1][0][GUARD + 100] ^= 0xFF
  with pytest.raises(AssertionError, match='past its end'):
    proxy.check_guards('stale, overrun')
  with pytest.raises(AssertionError):
    stale([torch.zeros(0, dtype=torch.uint8)])


# ---------------------------------------------------------------------------------------------
# 2. completeness of the seam
# ---------------------------------------------------------------------------------------------
CREATORS = {'empty', 'empty_like', 'empty_strided', 'new_empty', 'new_empty_strided', 'new', 'empty_permuted',
            'empty_quantized'}
LEGACY = {'Tensor', 'FloatTensor', 'DoubleTensor', 'HalfTensor', 'IntTensor', 'LongTensor', 'ByteTensor', 'BoolTensor'}
HOST_ARRAYS = {'np', 'numpy'}


def _dotted(node):
  parts = []
  while isinstance(node, ast.Attribute):
    parts.append(node.attr)
    node = node.value
  parts.append(node.id if isinstance(node, ast.Name) else '?')
  return list(reversed(parts))


def uninitialised_sites(source, filename='<module>'):
  """(ok sites, offending sites) of one module: every call that creates uninitialised tensor memory, as
  (line, text).  ok = `torch.empty*(...)` with `torch` the module's global name bound by `import torch`."""
  tree = ast.parse(source, filename)
  bad, ok = [], []
  torch_global = False
  for node in tree.body:
    if isinstance(node, ast.Import):
      torch_global = torch_global or any(a.name == 'torch' and a.asname is None for a in node.names)
  for node in ast.walk(tree):
    if isinstance(node, ast.Import):
      for a in node.names:      # `import torch as th` / `import torch.x as y` bound to a creator-bearing module
        if a.name == 'torch' and a.asname not in (None, 'torch'):
          bad.append((node.lineno, 'import torch as %s' % a.asname))
    elif isinstance(node, ast.ImportFrom) and (node.module or '').split('.')[0] == 'torch':
      for a in node.names:
        if a.name in CREATORS | LEGACY or a.name == '*':
          bad.append((node.lineno, 'from %s import %s' % (node.module, a.name)))
    elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign, ast.arg, ast.For, ast.With, ast.FunctionDef)):
      names = []
      if isinstance(node, ast.arg):
        names = [node.arg]
      elif isinstance(node, ast.FunctionDef):
        names = [node.name]
      else:
        for t in ast.walk(node.targets[0] if isinstance(node, ast.Assign) else getattr(node, 'target', node)):
          if isinstance(t, ast.Name) and isinstance(t.ctx, ast.Store):
            names.append(t.id)
      if 'torch' in names:
        bad.append((node.lineno, 'the name `torch` is rebound'))
    if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
      continue
    path = _dotted(node.func)
    attr = path[-1]
    text = '.'.join(path)
    if attr in CREATORS:
      if path[0] in HOST_ARRAYS and len(path) == 2:
        continue                                      # NumPy: host memory
      if path == ['torch', attr] and attr in ('empty', 'empty_like', 'empty_strided') and torch_global:
        ok.append((node.lineno, text))
      else:
        bad.append((node.lineno, text))
    elif attr in LEGACY and path[0] == 'torch' and node.args and not (
        len(node.args) == 1 and isinstance(node.args[0], (ast.List, ast.ListComp, ast.Call, ast.Name, ast.Attribute))):
      bad.append((node.lineno, text + '(sizes)'))     # torch.Tensor(3, 4): uninitialised
  return ok, bad


def test_the_walk_sees_what_it_must():
  ok, bad = uninitialised_sites('import torch\nimport numpy as np\n'
                                'a = torch.empty(3, device="cuda")\nb = np.empty(3)\nc = torch.empty_like(a)\n')
  assert [t for _, t in ok] == ['torch.empty', 'torch.empty_like'] and not bad
  for src in ('import torch\nx = y.new_empty(3)\n', 'import torch as th\nx = th.empty(3)\n',
              'from torch import empty\nx = empty(3)\n', 'import torch\nx = torch.Tensor(3, 4)\n',
              'import torch\nx = torch.cuda.FloatTensor(3)\n', 'import torch\ndef f(torch):\n  return torch.empty(1)\n',
              'import torch\nx = torch.cuda.empty(3)\n', 'import torch\nx = t.new(3)\n',
              'def f():\n  import torch\n  return torch.empty(2)\n'):
    assert uninitialised_sites(src)[1], src
  assert not uninitialised_sites('import torch\nx = torch.Tensor([1, 2])\ny = torch.zeros(3)\n')[1]


def test_every_uninitialised_allocation_goes_through_the_seam():
  total = 0
  for name in dirty_alloc.MODULES:
    mod = importlib.import_module(name)
    assert getattr(mod, 'torch') is torch, name
    source = open(mod.__file__).read()
    ok, bad = uninitialised_sites(source, mod.__file__)
    assert not bad, '%s: these sites bypass tests/dirty_alloc.py: %s' % (name, bad)
    total += len(ok)
  assert total >= 60, total           # ops.py alone has some 70 sites; the walk has not gone blind


# ---------------------------------------------------------------------------------------------
# 3. coverage of the regions
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from cmhse_amd import _lib
  return _lib.load()


def _align(v):
  return (v + 255) // 256 * 256


def _split_ld(k):
  return (k + 15) // 16 * 16


POOL_FLAG = {'LAST': 'POOL_LAST', 'MAX': 'POOL_MAX', 'ATTN': 'POOL_ATTN', 'ALL': 'POOL_ALL'}
GRU_REGIONS = ('hs', 'e_part', 'gates', 'argmax', 'v', 'wih_s', 'whh_s', 'wlin_s', 'xs', 'hs_s', 'h0_s', 'gx',
               'tail_sync', 'chain_sync', 'tok_tab')
BWD_REGIONS = ('dgx', 'dgh', 'dpool', 'carry', 'whh_t', 'wih_t', 'wlin_t', 'du', 'de', 'xaddr', 'hpaddr', 'dxaddr',
               'hsaddr', 'p_t', 'zero_row', 'tail_sync', 'colsum', 'dx_part', 'wg_part', 'rec_part')


def gru_ws_sizes(j, knobs, bf3, tok_rows):
  """gru_ws_layout (gru_ws.hpp) restated: {region: bytes} of one request, in layout order."""
  k = dict(fwd_shapes.KNOBS, **knobs)
  c = j['counts']
  S, T, sum_T, I, H = c[0], len(c), sum(c), j['I'], j['H']
  save, attn, mx = j['save'], j['pool'] == 'ATTN', j['pool'] == 'MAX'
  mm = k['mid_max_seqs']
  gx_rows = 0 if mm <= 0 else (sum_T if S <= mm else min(mm * T, sum_T))
  f = 4
  sizes = dict(
      hs=_align(sum_T * H * f), e_part=_align(-(-H // fwd_shapes.ATT_BN) * sum_T * f) if attn else 0,
      gates=_align(sum_T * 4 * H * f) if save else 0, argmax=_align(S * H * 4) if save and mx else 0,
      v=_align(sum_T * H * f) if save and attn else 0,
      wih_s=_align(3 * H * _split_ld(I) * f) if bf3 else 0, whh_s=_align(3 * H * _split_ld(H) * f) if bf3 else 0,
      wlin_s=_align(H * _split_ld(H) * f) if bf3 and attn else 0,
      xs=_align(sum_T * _split_ld(I) * f) if bf3 else 0, hs_s=_align(sum_T * _split_ld(H) * f) if bf3 else 0,
      h0_s=_align(S * _split_ld(H) * f) if bf3 else 0,
      gx=_align(gx_rows * 3 * H * f) if I % 4 == 0 and H % 4 == 0 else 0, tail_sync=256,
      chain_sync=0 if save else _align(256 + 4 * min(T, fwd_shapes.CHAIN_MAX_STEPS) * ((S + 63) // 64)),
      tok_tab=_align(tok_rows * 3 * H * f))
  assert tuple(sizes) == GRU_REGIONS
  return sizes


def _flags(ops, j, bf3):
  return (getattr(ops, POOL_FLAG[j['pool']]) | (ops.SAVE_FOR_BACKWARD if j['save'] else 0) |
          (ops.MATH_BF16X3 if bf3 and not j['save'] else 0))


def _check_gru_layout(lib, ops, j, knobs, bf3, sizes):
  """The restated layout against the library: the total and the offsets of the regions it names."""
  c = j['counts']
  S, T, sum_T = c[0], len(c), sum(c)
  flags = _flags(ops, j, bf3)
  with ops.tuned(**knobs):
    total = lib.cmhse_gru_pool_workspace_tok(S, T, sum_T, j['I'], j['H'], flags, j['vocab'])
  assert total == sum(sizes.values()), (j, total, sizes)
  off, nbytes, at = ctypes.c_size_t(0), ctypes.c_size_t(0), 0
  for name in GRU_REGIONS:
    if name in ('hs', 'gates', 'argmax', 'v', 'xs', 'hs_s', 'h0_s'):
      assert lib.cmhse_gru_pool_ws_region(S, T, sum_T, j['I'], j['H'], flags, name.encode(), ctypes.byref(off),
                                          ctypes.byref(nbytes)) == 0
      assert off.value == at and _align(nbytes.value) == sizes[name], (name, j)
    at += sizes[name]


def gru_regions_reached(j, launches, sizes, bf3):
  """The regions of one request that are non-empty AND that a launch of the call uses."""
  tags = {ln['tag'] for ln in launches}
  kinds = {ln['kind'] for ln in launches}
  used = dict(hs=True, e_part=True, gates=True, argmax=True, v=True,
              wih_s=launches.bf3, whh_s=launches.bf3, wlin_s=any(ln['kind'] == 'attn' and ln['bf3'] for ln in launches),
              xs=launches.rows_split > 0, hs_s=launches.rows_split > 0, h0_s=launches.rows_split > 0 and j['h0'],
              gx=any(t.startswith('Mid') for t in tags), tail_sync='tail' in kinds, chain_sync='chain' in kinds,
              tok_tab='token table' in tags)
  return {r for r in GRU_REGIONS if sizes[r] > 0 and used[r]}


def bwd_ws_sizes(S, sum_T, I, H, attn):
  """bwd_ws_layout (bwd.hip) restated."""
  n_tiles = -(-H // bptt_shapes.REC_BN)
  rec = 0 if H % 4 else (256 // n_tiles + 1 + (S + 31) // 32) * 32 * H
  sizes = dict(
      dgx=sum_T * 3 * H * 4, dgh=sum_T * 3 * H * 4, dpool=sum_T * H * 4, carry=S * H * 4, whh_t=3 * H * H * 4,
      wih_t=3 * H * I * 4, wlin_t=H * H * 4 if attn else 0, du=sum_T * H * 4 if attn else 0, de=sum_T * 4 if attn else 0,
      xaddr=sum_T * 8, hpaddr=sum_T * 8, dxaddr=sum_T * 8, hsaddr=sum_T * 8 if attn else 0, p_t=sum_T * 4,
      zero_row=max(H, I) * 4, tail_sync=256, colsum=-(-sum_T // bss.COLSUM_ROWS) * 3 * H * 4,
      dx_part=bss.det_split_scratch_floats(sum_T, max(I, H)) * 4, wg_part=bss.wg_part_floats(sum_T, I, H) * 4,
      rec_part=rec * 4)
  assert tuple(sizes) == BWD_REGIONS
  return {r: _align(v) for r, v in sizes.items()}


def _train_requests():
  """(case id, counts, I, H, pool, feed, has h0, knobs) of every backward request of the GPU file."""
  out = []
  for name, knobs, jobs in T.TRAIN_CASES:
    for j in jobs:
      out.append((name, j['counts'], j['I'], j['H'], j['pool'], 'padded', j['h0'], knobs))
  for name, feed, knobs, cls, I, H, profile, h0 in T.SIDE_CASES:
    pool = {'attention': 'ATTN', 'maxout': 'MAX', 'seq2seq': 'LAST', 'all': 'ALL'}[bss.POOL_OF[cls]]
    out.append((name, list(profile), I, H, pool, feed, h0, knobs))
  return out


def _table(rows):
  return '\n' + '\n'.join('  %-24s %s' % (k, ', '.join(sorted(v))) for k, v in rows)


def test_forward_cases_reach_every_gru_region(lib):
  from cmhse_amd import ops
  reached, tags, rows = set(), set(), []
  chain_launches, bf3_edges = 0, set()
  for name, knobs, train, tail_stream, jobs, bf3 in T.FWD_CASES + [(n, k, True, False, j, False) for n, k, j in T.TRAIN_CASES]:
    assert 1 <= len(jobs) <= (2 if train else 4), name
    for j in jobs:
      assert fwd_shapes.counts_of(fwd_shapes.lens_of(j['counts'])) == j['counts'], name
      assert j['save'] == train and (j['stream'] is not None) == train, name
      # the sizes the issue sets: S <= ~300, T <= ~12 (the T = 37 tail case apart), H of the four widths
      assert j['counts'][0] <= 300 and (len(j['counts']) <= 16 or name == 'train_bptt_tail_t37'), name
      assert j['H'] in (24, 36, 72, 128), name
    plan = fwd_shapes.call_steps(jobs, knobs, tail_stream, bf3=bf3, attn=True)
    call_tags = fwd_shapes.call_tags(jobs, knobs, tail_stream, bf3=bf3)
    tags |= call_tags
    got = set()
    for j, launches in zip(jobs, plan):
      tok_rows = j['vocab'] if any(ln['tag'] == 'token table' for ln in launches) else 0
      sizes = gru_ws_sizes(j, knobs, bf3 and not j['save'], tok_rows)
      _check_gru_layout(lib, ops, j, knobs, bf3, sizes)
      got |= gru_regions_reached(j, launches, sizes, bf3)
      chain_launches = max(chain_launches, sum(1 for ln in launches if ln['kind'] == 'chain'))
      if launches.bf3 and launches.rows_split > 0:
        bf3_edges |= {'H%16' if j['H'] % 16 else '', 'I%16' if j['I'] % 16 else '', 'h0' if j['h0'] else ''}
    reached |= got
    rows.append((name, got | {t for t in call_tags if t.split(' ')[0] in ('xproj', 'token') or t.startswith('FwdTail KB')}))
  missing = set(GRU_REGIONS) - reached
  assert not missing, 'GruWs regions no case reaches: %s%s' % (sorted(missing), _table(rows))
  # bf16x3 with H % 16 != 0, I % 16 != 0 and caller h0; a chain cut into more than one launch; the forward
  # resident tail; every family, the projections, the token table, the aliases, all four pools, training
  assert {'H%16', 'I%16', 'h0'} <= bf3_edges, _table(rows)
  assert chain_launches >= 2, 'no request runs two chain launches' + _table(rows)
  fams = {fwd_shapes._family(t) for t in tags if t.split(' ')[0] not in ('xproj', 'token', 'Attn', 'bf3')}
  assert {'Tiny', 'Mid', 'Tiled', 'Chain', 'FwdTail', 'TiledBf3'} <= fams, (sorted(fams), _table(rows))
  assert {'xproj chunked', 'xproj early', 'token table'} <= tags, _table(rows)
  for p in fwd_shapes.POOLS:      # every pool mode's epilogue runs in some family, and in the four-request call
    assert any(t.endswith(' ' + p) and t.split(' ')[0] in fwd_shapes.FAMILY_POOLS for t in tags), (p, sorted(tags))
  assert {'FwdTail LAST', 'FwdTail ALL'} <= tags
  assert any(j.get('aliases') for c in T.FWD_CASES for j in c[4])
  multi = [c for c in T.FWD_CASES if len(c[4]) == 4 and c[3]]
  assert multi and {j['pool'] for j in multi[0][4]} == set(fwd_shapes.POOLS)      # four requests, a tail stream
  # the stale source is larger than every case of its family
  for table, big in ((T.FWD_CASES, T.STALE_FWD[4]), ([(n, k, 0, 0, j) for n, k, j in T.TRAIN_CASES], T.STALE_TRAIN[2])):
    assert max(sum(j['counts']) * j['H'] for j in big) > max(sum(j['counts']) * j['H'] for c in table for j in c[4])


def test_backward_cases_reach_every_bwd_region_and_arm(lib):
  from cmhse_amd import ops
  reached, rows = set(), []
  arms = set()
  for name, counts, I, H, pool, feed, h0, knobs in _train_requests():
    S, sum_T = counts[0], sum(counts)
    sizes = bwd_ws_sizes(S, sum_T, I, H, pool == 'ATTN')
    total = lib.cmhse_gru_pool_bwd_workspace(S, len(counts), sum_T, I, H, getattr(ops, POOL_FLAG[pool]))
    assert total == sum(sizes.values()), (name, total, sizes)
    got = {r for r in BWD_REGIONS if sizes[r] > 0}
    steps = bptt_shapes.step_shapes(counts, H, h0, knobs)
    pl = bss.plan(counts, I, H, {'ATTN': 'attention', 'MAX': 'maxout', 'LAST': 'seq2seq', 'ALL': 'all'}[pool], feed, knobs)
    mine = {'dpool ' + pool}
    if any(st['shape'] == 'Tail' for st in steps):
      mine.add('BPTT resident tail')
    else:
      got.discard('tail_sync')                     # (cleared, not waited on)
    if not any(st['shape'] == 'Split' for st in steps):
      got.discard('rec_part')
    if not any(tn['splits'] > 1 for tn in bss.tn_launches(pl)):
      got.discard('wg_part')
    if not any(c['dx'] and c['dx']['kind'] == 'det' for c in pl['chunks']) and not (pl['attn'] and pl['attn']['dpool']['kind'] == 'det'):
      got.discard('dx_part')
    if any(c['dx'] and c['dx']['kind'] == 'det' and c['dx']['splits'] > 1 for c in pl['chunks']):
      mine.add('split-K d(input)')
    if len(pl['chunks']) > 1 and any(tn['accumulate'] for tn in bss.tn_launches(pl)):
      mine.add('time-chunked weight gradients')
    if feed == 'tokens':
      mine.add('token-fed d_emb_table')
      assert pl['chunks'][0]['dx']['kind'] == 'atomic'
    if feed == 'repeat':
      mine.add('time-constant dx rows' + (' with h0' if h0 else ''))
      assert pl['chunks'][0]['dx']['kind'] == 'atomic'
    if not h0:
      mine.add('zero_row read as h0')
    reached |= got
    arms |= mine
    rows.append((name, got | mine))
  missing = set(BWD_REGIONS) - reached
  assert not missing, 'BwdWs regions no case reaches: %s%s' % (sorted(missing), _table(rows))
  want = {'dpool LAST', 'dpool MAX', 'dpool ALL', 'dpool ATTN', 'BPTT resident tail', 'split-K d(input)',
          'time-chunked weight gradients', 'token-fed d_emb_table', 'time-constant dx rows with h0', 'zero_row read as h0'}
  assert want <= arms, 'arms no case reaches: %s%s' % (sorted(want - arms), _table(rows))
  # the T = 37 case is the one of bptt_shapes.TAIL_CASES, and its tail is long
  t37 = [r for r in _train_requests() if r[0] == 'train_bptt_tail_t37'][0]
  assert len(t37[1]) == bptt_shapes.TAIL_T == 37
  tail = bptt_shapes.tail_of(t37[1], t37[3])
  assert tail is not None and 37 - tail[0] >= 20
  # the own_zero arm of launch_nt_out (the issue's "split-K own_zero product") has no caller: nothing to reach
  assert bss.no_own_zero_caller()
  # exempt outputs: exactly the two float-atomic scatters
  assert T.EXEMPT == {c[0]: ('d_src',) for c in T.SIDE_CASES if c[1] in ('tokens', 'repeat')}
  # the sizes differ from those of tests/bwd_side_shapes.py
  theirs = {(c[4], c[5], tuple(c[6])) for c in bss.CASES}
  assert not {(c[4], c[5], tuple(c[6])) for c in T.SIDE_CASES} & theirs


def test_scoring_cases_cross_their_tile_boundaries(lib):
  N, M, row0, nrows = T.SCORE_N, T.SCORE_M, T.SCORE_ROW0, T.SCORE_NROWS
  pl = ss.count_plan(nrows, M)
  assert pl['row_tiles'] >= 2 and pl['col_tiles'] >= 2 and row0 % 64 != 0 and M >= N and row0 + nrows <= N
  assert any(D % 4 == 0 for D in T.SCORE_DS) and any(D % 4 != 0 for D in T.SCORE_DS)
  assert T.SCORE_KS == (1, 17, 128)
  for K in T.SCORE_KS:
    assert ss.topk_plan(nrows, M, K)['panels'] > 1, K
  lists = T.score_positives(N, M, True)
  sizes = {len(set(p.tolist())) for p in lists}
  assert sizes == {1, 2, 3, 4} and any(len(p) != len(set(p.tolist())) for p in lists)         # 1 to 4, duplicates
  assert all(len(p) == len(set(p.tolist())) for p in T.score_positives(N, M, False))
  assert any(list(p) != sorted(p) for p in lists)                                                # unsorted
  B = T.GROUP_B
  assert B > ss.GR_RANK_T and -(-B // ss.GR_RANK_T) >= 3
  for seed in (1, 2):
    counts = T.group_counts(B, seed)
    assert set(counts) == {1, 2, 4, 8}
  gp = ss.group_plan(T.group_counts(B, 1), T.group_counts(B, 2))
  assert gp['row_tiles'] >= 2 and gp['col_tiles'] >= 2
  for direction, (nc, ns) in (('p2v', (T.GTOPK_GALLERY, T.GTOPK_QUERY)), ('v2p', (T.GTOPK_QUERY, T.GTOPK_GALLERY))):
    tp = ss.group_topk_plan(nc, ns, direction, T.GTOPK_K)
    assert tp['panels'] >= 2 and tp['g_tiles'] >= 2, (direction, tp['panels'])
  # the stale image comes from larger shapes
  c = T.STALE_SCORE
  assert c['nrows'] > nrows and c['M'] > M and c['K'] == max(T.SCORE_KS) and c['row0'] + c['nrows'] <= c['N'] <= c['M']


def test_fills_and_their_meaning():
  assert T.FILLS == ('zero', 'ones', 'a5', 'stale')
  assert dirty_alloc.BYTE == {'zero': 0x00, 'ones': 0xFF, 'a5': 0xA5}
  assert np.isnan(np.frombuffer(b'\xff' * 4, dtype=np.float32)[0]) and np.isnan(np.frombuffer(b'\xff' * 8, dtype=np.float64)[0])
  assert np.frombuffer(b'\xff' * 4, dtype=np.int32)[0] == -1
  assert abs(float(np.frombuffer(b'\xa5' * 4, dtype=np.float32)[0])) < 1e-15        # tiny, not zero
  assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_loss_workspace.py'))
