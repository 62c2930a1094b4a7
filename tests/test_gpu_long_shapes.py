"""Long sequences through every per-step loop against the float64 oracle.

The other shape suites compare short sequences (37 steps at most) element-wise with the oracle.  The
loops that change behaviour only with length — attn_pool_kernel's staging rounds of 256 steps, its
second trip through the denominator and its second round of output units from H > 1024, the 16 waves
of attn_pool_bwd_kernel taking 33 and 65 steps each, the step chain cut every 96 steps and resumed,
the resident tails running 500 and 1024 steps behind one grid barrier each, per-step launches 513
deep, the weight-gradient chunks, column-sum slabs and projection chunks of 2000 packed rows in a
handful of sequences, the tails refused at H > 1024, the exact attention projection in a partial and a
final launch — are the cases of long_shapes.CASES; tests/test_long_shapes_cpu.py proves from the
dispatch rules that each case reaches the loops it names.  Every case runs twice (same bits), every
output, d input, d h0 and parameter gradient is compared with the oracle under the project's bars
(conftest.assert_emb_close, gpu_common.grad_close), and next to each bar the distance of the oracle
in float32 from the oracle in float64 is printed: what fp32 arithmetic alone costs at these lengths.
Then one validation pass over a split with an outlier paragraph of 525 words.
(Measured distances and wall times: profiles/long_shapes_distances.txt.)

RELAXED names the gradient tensors whose bar is 8x the float32 oracle's own distance instead of
grad_close's (allowed only where that oracle is itself beyond a quarter of the bar): none."""
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN_TOL, assert_emb_close, golden_state_dicts, load_golden
from gpu_common import _blas_threads, _np_batches, golden_model, grad_close

import long_shapes as ls
import test_gpu_fwd_shapes as fs

pytestmark = pytest.mark.gpu

# '<case> request <k> <tensor>' -> (kernel distance, float32 oracle's distance) when the entry was made
RELAXED = {}


def _dist(got, want):
  return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def _line(what, d, d32, bar):
  print('\nlong_shapes %-62s |diff| %.3e  fp32 oracle %.3e  bar %.3e' % (what, d, d32, bar), end='')


def _emb(got, want, want32, what):
  _line(what, _dist(got, want), _dist(want32, want), GOLDEN_TOL)
  assert_emb_close(got, want, what)


def _grad(got, want, want32, what):
  bar = 2e-4 * max(1e-30, float(np.abs(want).max())) + 2e-6      # gpu_common.grad_close
  d, d32 = _dist(got, want), _dist(want32, want)
  _line(what, d, d32, bar)
  if what in RELAXED:
    assert d32 > bar / 4, '%s: the float32 oracle is within a quarter of the bar; the bar stays' % what
    assert got.shape == want.shape and d <= 8 * d32, '%s: %.3e > 8 x %.3e' % (what, d, d32)
  else:
    grad_close(got, want, what)


def _backward(oracle, j, cache, lens, w):
  """test_gpu_fwd_shapes._backward in the cache's own precision (w already cast to it)."""
  if j['pool'] != 'ALL':
    return oracle.pooled_gru_backward(cache, w)
  dhs = np.zeros_like(cache['hs'])
  starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
  for i, l in enumerate(lens):
    dhs[i, :l] = w[starts[i]:starts[i] + l]
  return oracle.gru_backward(cache, dhs)


def _oracles(oracle, j, x, lens, sd, h0, w):
  """Per dtype (float64, float32): [out, dx, dh0, {parameter gradients}] (the last three when w is given)."""
  res = []
  for dtype in (np.float64, np.float32):
    want, cache = oracle.pooled_gru_forward_cache(fs._ORACLE_POOL[j['pool']], x, lens, sd, h0, dtype)
    if j['pool'] == 'ALL':
      want = np.concatenate([cache['hs'][i, :l] for i, l in enumerate(lens)])
    rows = [want]
    for src, n in j.get('aliases', ()):      # an alias row: the attention encoding of the truncated sequence
      rows.append(oracle.pooled_gru_forward_cache('attention', x[src:src + 1, :n], np.asarray([n]), sd,
                                                  None if h0 is None else h0[src:src + 1], dtype)[0])
    out = [np.concatenate(rows)]
    if w is not None:
      grads, dx, dh0 = _backward(oracle, j, cache, lens, w.astype(dtype))
      out += [dx, dh0, grads]
    res.append(out)
  return res


@pytest.mark.parametrize('case', ls.CASES, ids=[c[0] for c in ls.CASES])
def test_long_shape_vs_oracle(dev, oracle, tune, case):
  from cmhse_amd import ops
  name, knobs, train, tail_stream, jobs, _ = case
  t_start = time.perf_counter()
  layers_, sds, data, rng = fs._setup(jobs, dev)
  tune(**knobs)
  assert ops.async_status() == 0
  ws = [rng.standard_normal((int(d[0].sum()) if j['pool'] == 'ALL' else len(d[0]), j['H'])).astype(np.float32)
        for j, d in zip(jobs, data)]

  def run():
    if train:
      return fs._run_training(jobs, layers_, data, ws, dev)
    return [[o.clone()] for o, _ in fs._run_inference(jobs, layers_, data, dev, tail_stream)]

  t0 = time.perf_counter()
  first = run()
  t_gpu = time.perf_counter() - t0
  again = run()
  assert ops.async_status() == 0, '%s: a resident kernel gave up waiting' % name
  for k, (a, b) in enumerate(zip(first, again)):
    for i, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), '%s: request %d result %d not reproducible from run to run' % (name, k, i)
  for k, (j, (lens, x, h0, _, _)) in enumerate(zip(jobs, data)):
    tag = '%s request %d' % (name, k)
    with _blas_threads():
      w64, w32 = _oracles(oracle, j, x, lens, sds[k], h0, ws[k] if train else None)
    got = [t.cpu().numpy() for t in first[k]]
    assert got[0].shape == w64[0].shape, tag
    _emb(got[0], w64[0], w32[0], '%s out (%s, I %d, H %d)' % (tag, j['pool'], j['I'], j['H']))
    if not train:
      continue
    T = w64[1].shape[1]
    _grad(got[1][:, :T], w64[1], w32[1], tag + ' dx')
    if h0 is not None:
      _grad(got[2], w64[2], w32[2], tag + ' dh0')
    params = got[3:] if h0 is not None else got[2:]
    named = list(layers_[k].named_parameters())
    assert len(named) == len(params)
    for (pn, _), g in zip(named, params):
      _grad(g, w64[3]['rnn.' + pn], w32[3]['rnn.' + pn], '%s %s' % (tag, pn))
  print('\nlong_shapes %-62s wall %.2f s (first GPU run %.2f s)' % (name, time.perf_counter() - t_start, t_gpu), end='')


@pytest.mark.parametrize('rnn_type', ['attention', 'maxout'])
def test_validation_pass_with_an_outlier_paragraph(dev, oracle, rnn_type):
  """evaluation.encode_data over 9 videos, one with a paragraph of 25 x 21 = 525 words and 300 frames:
  share_prefix 1 and 0 bit for bit, the six matrices against the float64 oracle, i2t / t2i ranks and
  top-1 equal to the oracle's on every row whose float64 margin exceeds 1e-5 (at most one of nine left
  out per direction; the CPU test proves the oracle alone meets that)."""
  from cmhse_amd import evaluation, ops, synthetic
  t_start = time.perf_counter()
  g = load_golden('model_%s.npz' % rnn_type)
  opt, model = golden_model(rnn_type, g)
  batches = ls.outlier_batches(opt.img_dim, opt.vocab_size)
  assert int(batches[0][7][0]) == 525 and int(batches[0][6][0]) == 300

  def run(share):
    with ops.tuned(share_prefix=share):
      res = evaluation.encode_data(opt, model, synthetic.ListLoader(batches), logging=lambda *a, **k: None)
      return [np.array(r) for r in res[:6]], evaluation.SHARE_STATS['aliases']
  off, n_off = run(0)
  on, n_on = run(1)
  assert ops.async_status() == 0
  assert (n_off, n_on) == (0, 9 if rnn_type == 'attention' else 0)
  names = ['vid_emb', 'para_emb', 'clip_emb', 'cap_emb', 'vid_ctx', 'para_ctx']
  for nm, a, b in zip(names, on, off):
    assert a.shape == b.shape and np.array_equal(a, b), '%s differs between share_prefix 1 and 0' % nm
  with _blas_threads():
    want, want32 = (oracle.encode_data(rnn_type, golden_state_dicts(g), _np_batches(batches), margin=0.2, dtype=dt)
                    for dt in (np.float64, np.float32))
  for i, nm in enumerate(names):
    assert on[i].shape == want[i].shape, nm
    _emb(on[i], want[i], want32[i], 'outlier %s %s' % (rnn_type, nm))
  for fn, (ranks64, top64, ok) in zip((evaluation.i2t, evaluation.t2i), ls.robust_rows(want)):
    rep, top1, ranks = fn(on[0], on[1])
    left_out = int((~ok).sum())
    print('\nlong_shapes %-62s rows left out %d of %d' % ('outlier %s %s' % (rnn_type, fn.__name__), left_out, len(ok)), end='')
    assert left_out <= ls.RANK_LEFT_OUT_MAX
    np.testing.assert_array_equal(np.asarray(ranks)[ok], ranks64[ok])
    np.testing.assert_array_equal(np.asarray(top1)[ok], top64[ok])
  print('\nlong_shapes %-62s wall %.2f s' % ('outlier ' + rnn_type, time.perf_counter() - t_start), end='')
