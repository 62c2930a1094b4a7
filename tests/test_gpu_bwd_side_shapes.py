"""Everything cmhse_gru_pool_bwd launches beside its BPTT chain against the float64 oracle.

The d(input) product with K cut into segments and added in order (launch_nt_rows_once), the same
launcher ADDING du . W_lin to the attention backward's dpool, the atomic split-K into an embedding
table and into a time-constant input (launch_nt_out), the weight-gradient products' tile height,
row split and accumulation over chunks (TnRowsLaunch), the row-address tables with out-of-range
token ids, the column sums and the pooling backward: their arms are host-side shape decisions
(cmhse_amd/csrc/bwd.hip) that the other oracle tests reach at one full-size shape or not at all.
Each case of bwd_side_shapes.CASES targets arms by name, and tests/test_bwd_side_shapes_cpu.py
proves from the restated rules that it lands on them.  (Measured distances:
profiles/bwd_side_distances.txt.)"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_TOL, assert_emb_close
from gpu_common import _blas_threads, grad_close

import bwd_side_shapes as ss

pytestmark = pytest.mark.gpu


def _layer(cls, I, H, seed):
  from cmhse_amd import decoder, layers
  torch.manual_seed(seed)
  layer = (decoder.Seq2Seq_Decode if cls == 'Seq2Seq_Decode' else getattr(layers, cls))(I, H)
  with torch.no_grad():
    layer.rnn.bias_ih_l0.normal_(0, 0.1)
    layer.rnn.bias_hh_l0.normal_(0, 0.1)
  sd = {'rnn.' + k: v.detach().numpy().astype(np.float64) for k, v in layer.state_dict().items()}
  return layer, sd


def _padded(rng, lens, I):
  x = np.zeros((len(lens), int(lens.max()), I), dtype=np.float32)
  for i, l in enumerate(lens):
    x[i, :l] = rng.standard_normal((l, I))
  return x


def _emb(got, want, name):
  """assert_emb_close, the distance over its tight bar printed first."""
  err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
  print('\nbwd_side %-46s |diff| %.3e  bar %.3e  ratio %.4f' % (name, err, GOLDEN_TOL, err / GOLDEN_TOL), end='')
  assert_emb_close(got, want, name)


def _grad(got, want, name):
  """gpu_common.grad_close, the distance over its bar printed first."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  if got.shape == want.shape:
    err, bar = np.abs(got - want).max(), 2e-4 * max(1e-30, np.abs(want).max()) + 2e-6
    print('\nbwd_side %-46s |diff| %.3e  bar %.3e  ratio %.4f' % (name, err, bar, err / bar), end='')
  grad_close(got, want, name)


@pytest.mark.parametrize('case', ss.CASES, ids=[c[0] for c in ss.CASES])
def test_bwd_side_shape_vs_oracle(dev, oracle, tune, case):
  """Forward output and every gradient (d input or d table or d rows, d h0 of the padded cases, all
  parameters, nonzero biases) against the float64 oracle.  A second run is bitwise identical on
  every output but the two summed with float atomics (d table, d rows of a time-constant input),
  which both runs hold against the oracle."""
  name, feed, knobs, cls, I, H, profile, _ = case
  lens = ss.lens_of(profile)
  S, T = len(lens), int(lens.max())
  rng = np.random.RandomState(S + 7 * H + I)
  layer, sd = _layer(cls, I, H, H + I)
  layer = layer.to(dev)
  pool = ss.POOL_OF[cls]
  lens_t = torch.from_numpy(lens)
  tok = h0 = None
  if feed == 'padded':
    x = _padded(rng, lens, I)
    h0 = (0.5 * rng.standard_normal((S, H))).astype(np.float32)
    src = x
  elif feed == 'tokens':
    src = rng.standard_normal((ss.VOCAB, I)).astype(np.float32)      # the embedding table
    tok = ss.case_tokens(rng, lens)
    x = np.zeros((S, T, I), dtype=np.float32)
    ids = ss.clamp_ids(tok, ss.VOCAB)
    for i, l in enumerate(lens):
      x[i, :l] = src[ids[i, :l]]
  else:
    src = rng.standard_normal((S, I)).astype(np.float32)             # one row per sequence, repeated
    x = np.zeros((S, T, I), dtype=np.float32)
    for i, l in enumerate(lens):
      x[i, :l] = src[i]
  n_out = int(lens.sum()) if pool == 'all' else S
  w = rng.standard_normal((n_out, H)).astype(np.float32)
  tune(**knobs)

  def run():
    layer.zero_grad()
    st = torch.from_numpy(src).to(dev).requires_grad_(True)
    ht = None
    if feed == 'padded':
      ht = torch.from_numpy(h0).to(dev).requires_grad_(True)
      y = layer(st, lens_t, ht)
    elif feed == 'tokens':
      y = layer.forward_tokens(torch.from_numpy(tok).to(dev), lens_t, st)
    else:
      y = layer.forward_repeat(st, lens)
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    out = dict(y=y.detach().clone(), d_src=st.grad.clone())
    if ht is not None:
      out['dh0'] = ht.grad.clone()
    for pn, p in layer.named_parameters():
      out[pn] = p.grad.clone()
    return out

  first, again = run(), run()
  for k in first:
    if k == 'd_src' and feed != 'padded':
      continue      # float atomics: each run against the oracle below
    assert torch.equal(first[k], again[k]), '%s: %s not reproducible from run to run' % (name, k)

  with _blas_threads():
    if pool == 'all':
      cache = oracle.gru_forward_cache(x, lens, sd, None, np.float64)
      want = np.concatenate([cache['hs'][i, :l] for i, l in enumerate(lens)])
      starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
      dhs = np.zeros_like(cache['hs'])
      for i, l in enumerate(lens):
        dhs[i, :l] = w[starts[i]:starts[i] + l]
      grads, dx, dh0 = oracle.gru_backward(cache, dhs)
    else:
      want, cache = oracle.pooled_gru_forward_cache(pool, x, lens, sd, h0)
      grads, dx, dh0 = oracle.pooled_gru_backward(cache, w.astype(np.float64))
  _emb(first['y'].cpu().numpy(), want, name + ' out')
  if feed == 'padded':
    _grad(first['d_src'].cpu().numpy()[:, :dx.shape[1]], dx, name + ' dx')
    _grad(first['dh0'].cpu().numpy(), dh0, name + ' dh0')
  elif feed == 'tokens':
    want_table = ss.d_table_from_dx(dx, tok, lens, ss.VOCAB)
    assert np.abs(want_table[0]).max() > 0 and np.abs(want_table[ss.VOCAB - 1]).max() > 0   # the clamped ids' rows
    for r, tag in ((first, ''), (again, ' (second run)')):
      _grad(r['d_src'].cpu().numpy(), want_table, name + ' d table' + tag)
  else:
    for r, tag in ((first, ''), (again, ' (second run)')):
      _grad(r['d_src'].cpu().numpy(), ss.d_rows_from_dx(dx, lens), name + ' d rows' + tag)
  for pn, _ in layer.named_parameters():
    _grad(first[pn].cpu().numpy(), grads['rnn.' + pn], name + ' ' + pn)


# Jobs of one grouped call: a split d(input) job, a token-fed job and an attention job whose dpool
# product is split (case ids of bwd_side_shapes.CASES).
GROUPED = ['dx_two_segments', 'emb_two_segments', 'dpool_two_segments']


def test_grouped_backward_bwd_side_shapes(dev, oracle):
  """The side launches of three jobs in ONE cmhse_gru_pool_bwd_multi call (layers.run_grouped):
  outputs and every gradient bit-identical to one call per job — all but the embedding table's,
  which float atomics sum: that one is held to the float64 oracle."""
  from cmhse_amd import layers
  cases = {c[0]: c for c in ss.CASES}
  rng = np.random.RandomState(31)
  jobs = []
  for name in GROUPED:
    _, feed, knobs, cls, I, H, profile, _ = cases[name]
    assert not knobs
    lens = ss.lens_of(profile)
    layer, sd = _layer(cls, I, H, 3 + H)
    job = dict(name=name, feed=feed, layer=layer.to(dev), sd=sd, lens=lens, pool=ss.POOL_OF[cls],
               w=rng.standard_normal((len(lens), H)).astype(np.float32))
    if feed == 'padded':
      job['x'] = _padded(rng, lens, I)
      job['h0'] = (0.5 * rng.standard_normal((len(lens), H))).astype(np.float32)
      job['leaves'] = [torch.from_numpy(job['x']).to(dev).requires_grad_(True),
                       torch.from_numpy(job['h0']).to(dev).requires_grad_(True)]
    else:
      job['table'] = rng.standard_normal((ss.VOCAB, I)).astype(np.float32)
      job['tok'] = ss.case_tokens(rng, lens)
      job['tok_dev'] = torch.from_numpy(job['tok']).to(dev)
      job['leaves'] = [torch.from_numpy(job['table']).to(dev).requires_grad_(True)]
    jobs.append(job)

  def call(j):
    if j['feed'] == 'padded':
      return (j['layer'], layers.SeqInput('padded', j['lens'], j['layer'].POOL), j['leaves'][0], j['leaves'][1], None)
    return (j['layer'], layers.SeqInput('tokens', j['lens'], j['layer'].POOL, tokens=j['tok_dev']), None, None,
            j['leaves'][0])

  def grads_of(outs):
    params = [p for j in jobs for p in list(j['layer'].parameters()) + j['leaves']]
    for p in params:
      p.grad = None
    sum((o * torch.from_numpy(j['w']).to(dev)).sum() for o, j in zip(outs, jobs)).backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in params], [o.detach().clone() for o in outs]

  g_grp, o_grp = grads_of(layers.run_grouped([call(j) for j in jobs]))
  g_sep, o_sep = grads_of([layers.run_grouped([call(j)])[0] for j in jobs])
  for a, b in zip(o_grp, o_sep):
    assert torch.equal(a, b)
  atomic = []
  pos = 0
  for j in jobs:
    n = len(list(j['layer'].parameters())) + len(j['leaves'])
    if j['feed'] == 'tokens':
      atomic.append(pos + n - 1)      # its table gradient
    pos += n
  assert len(atomic) == 1
  for i, (a, b) in enumerate(zip(g_grp, g_sep)):
    if i not in atomic:
      assert torch.equal(a, b), i
  j = jobs[1]
  ids = ss.clamp_ids(j['tok'], ss.VOCAB)
  x = np.zeros((len(j['lens']), int(j['lens'].max()), j['table'].shape[1]), dtype=np.float32)
  for i, l in enumerate(j['lens']):
    x[i, :l] = j['table'][ids[i, :l]]
  with _blas_threads():
    _, cache = oracle.pooled_gru_forward_cache(j['pool'], x, j['lens'], j['sd'], None)
    _, dx, _ = oracle.pooled_gru_backward(cache, j['w'].astype(np.float64))
  want = ss.d_table_from_dx(dx, j['tok'], j['lens'], ss.VOCAB)
  for g, tag in ((g_grp, 'grouped'), (g_sep, 'separate')):
    _grad(g[atomic[0]].cpu().numpy(), want, 'grouped_call d table (%s)' % tag)
