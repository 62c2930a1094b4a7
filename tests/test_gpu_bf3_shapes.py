"""Every shape of the opt-in bf16x3 math mode against the float64 oracle and against a float64 emulation
of its split products.

The mode's device code is the most delicate of the library: the ring step (gru_step_kernel<true, 2, true>:
an LDS-DMA ring with counted waits over operand rows three producers pre-split into bf16 (hi | lo) pairs),
and an attention projection cut at rows_split into a launch over pre-split rows and one over fp32 rows.
Each case of fwd_shapes.BF3_CASES is one inference call under ops.set_math_mode('bf16x3') whose requests
land on the kernels, cuts and hand-overs its id names; tests/test_bf3_shapes_cpu.py proves from the
dispatch rule that they do.  Checked for every request: the output AND every packed hidden state, against
the oracle (the project's bars for the mode) and against the emulation, which differs from the kernels in
fp32 accumulation order only and so tells rounding from truncation; a second run gives the same bits; the
mode engaged where the rule says so and left the other requests' bits alone; the pre-split rows the
producers wrote are, bit for bit, the split of their sources."""
import functools

import numpy as np
import pytest
import torch

from conftest import EMB_TOL, GOLDEN_TOL
from gpu_common import _blas_threads

import fwd_shapes
from test_gpu_fwd_shapes import _ORACLE_POOL, _oracle, _run_inference, _setup

BF3_TOL = 5e-5          # the mode against the float64 oracle: the bar of test_gpu_gru.py's test_bf16x3_mode_vs_oracle
# The mode against its emulation: GOLDEN_TOL, what the exact path holds against its oracle at these shapes
# (the two differ in fp32 accumulation order only).  A case a CORRECT kernel cannot hold it on gets
# 4 x the exact path's measured distance from the oracle on that case (the split products carry three
# times the terms), never more than 1e-5 — half of what truncating the split costs.  None at present:
# measured 1.8e-7 to 3.1e-6 (profiles/bf3_shapes_distances.txt).
EMU_TOL = {}

_CASES = {c[0]: c for c in fwd_shapes.BF3_CASES}


@functools.lru_cache(maxsize=None)
def references(oracle, name, products='bf16x3', steps=None):
  """Per request of case `name`: the float64 oracle's (out, hs) and the emulation's, with the split
  products where the dispatch rule puts the mode's kernels — the leading TiledBf3 steps, and the
  attention projection when it runs in bf16x3.  `steps`: only the first time steps (a CPU test's
  shortcut for the widest case).  Computed once per process; the arrays are read-only."""
  _, knobs, _, tail_stream, jobs, _ = _CASES[name]
  _, sds, data, _ = _setup(jobs, torch.device('cpu'))
  out = []
  for j, sd, (lens, x, h0, _, _), launches in zip(jobs, sds, data,
                                                   fwd_shapes.call_steps(jobs, knobs, tail_stream, bf3=True)):
    if steps is not None:
      lens, x = np.minimum(lens, steps), x[:, :steps]
    split_steps = sum(len(ln['ts']) for ln in launches if ln['tag'] == 'TiledBf3')
    split_att = any(ln['kind'] == 'attn' and ln['bf3'] for ln in launches)
    with _blas_threads():
      want, cache = _oracle(oracle, j, x, lens, sd, h0)
      emu, emu_hs = oracle.pooled_gru_forward(_ORACLE_POOL[j['pool']], x, lens, sd, h0, np.float64,
                                              products=products, split_steps=split_steps, split_attention=split_att)
    if j['pool'] == 'ALL':
      emu = np.concatenate([emu_hs[i, :l] for i, l in enumerate(lens)])
    ref = dict(want=want, hs=cache['hs'], emu=emu, emu_hs=emu_hs, lens=lens)
    for v in ref.values():
      v.setflags(write=False)
    out.append(ref)
  return out


def packed(hs, order, counts):
  """[S, T, ..] in input order -> the library's time-major packed rows (sorted sequences per step)."""
  return np.concatenate([hs[order[:c], t] for t, c in enumerate(counts)])


def _dist(a, b):
  return float(np.abs(np.asarray(a, dtype=np.float64) - b).max())


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', [c[0] for c in fwd_shapes.BF3_CASES])
def test_bf3_shape_vs_oracle_and_emulation(dev, oracle, tune, name):
  from cmhse_amd import ops
  _, knobs, _, tail_stream, jobs, _ = _CASES[name]
  layers_, _, data, _ = _setup(jobs, dev)
  plan = fwd_shapes.call_steps(jobs, knobs, tail_stream, bf3=True)
  tune(**knobs)

  def run(regions):
    res = _run_inference(jobs, layers_, data, dev, tail_stream)
    got = []
    for out, ctx in res:
      views = {r: ops.saved_region(ctx, r) for r in regions}
      got.append(dict(out=out.cpu().numpy(), order=ctx['sched'].order,
                      **{r: None if v is None else v.cpu().numpy() for r, v in views.items()}))
    return got

  assert ops.math_mode() == 'fp32'
  exact = run(('hs', 'xs', 'hs_s', 'h0_s'))
  ops.set_math_mode('bf16x3')
  try:
    first = run(('hs', 'xs', 'hs_s', 'h0_s'))
    again = run(('hs',))
  finally:
    ops.set_math_mode('fp32')
  refs = references(oracle, name)
  failures = []

  def check(ok, msg):
    if not ok:
      failures.append(msg)

  for k, (j, launches, ref, g, g2, ex) in enumerate(zip(jobs, plan, refs, first, again, exact)):
    tag = '%s request %d (%s, I %d, H %d)' % (name, k, j['pool'], j['I'], j['H'])
    lens, x, h0, _, _ = data[k]
    order, counts = g['order'], j['counts']
    assert ex['xs'] is None and ex['hs_s'] is None and ex['h0_s'] is None, tag   # the exact mode keeps no split rows
    # a second run gives the same bits
    check(np.array_equal(g['out'], g2['out']) and np.array_equal(g['hs'], g2['hs']), tag + ': not reproducible')
    # the mode engaged, or left the request alone
    if fwd_shapes.bf3_kernels(launches):
      check(not np.array_equal(g['out'], ex['out']), tag + ': the bf16x3 mode changed no bit of the output')
    else:
      check(np.array_equal(g['out'], ex['out']) and np.array_equal(g['hs'], ex['hs']),
            tag + ': a request no bf16x3 kernel serves differs from the fp32-mode call')
    # every packed hidden state and the output: against the oracle and against the emulation
    want_hs, emu_hs = packed(ref['hs'], order, counts), packed(ref['emu_hs'], order, counts)
    d_or = max(_dist(g['out'], ref['want']), _dist(g['hs'], want_hs))
    d_emu = max(_dist(g['out'], ref['emu']), _dist(g['hs'], emu_hs))
    d_exact = max(_dist(ex['out'], ref['want']), _dist(ex['hs'], want_hs))
    print('bf3_shapes_distance %-24s request %d  emulation %.3e  oracle %.3e  exact-path-vs-oracle %.3e'
          % (name, k, d_emu, d_or, d_exact))
    check(d_or <= min(EMB_TOL, BF3_TOL), tag + ': %.3e from the float64 oracle' % d_or)
    check(d_emu <= EMU_TOL.get(name, GOLDEN_TOL), tag + ': %.3e from the emulation of the split' % d_emu)
    # the pre-split rows: bit for bit the split of their sources (x - hi is exact in fp32, both sides
    # round to nearest even), chunk padding included
    rows = launches.rows_split
    if not launches.bf3:
      continue
    for r in ('xs', 'hs_s', 'h0_s'):
      assert g[r] is not None, (tag, r)
    if rows > 0:
      xs = oracle.split_rows_bits(packed(x, order, counts)[:rows], j['I'])
      check(np.array_equal(g['xs'][:rows].view(np.uint32), xs), tag + ': xs is not the split of the input rows')
      hs_s = oracle.split_rows_bits(g['hs'][:rows], j['H'])
      check(np.array_equal(g['hs_s'][:rows].view(np.uint32), hs_s), tag + ': hs_s is not the split of hs')
      if h0 is not None:
        h0_s = oracle.split_rows_bits(h0[order], j['H'])
        check(np.array_equal(g['h0_s'].view(np.uint32), h0_s), tag + ': h0_s is not the split of the initial states')
  assert not failures, '\n'.join(failures)
