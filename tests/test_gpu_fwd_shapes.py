"""Every forward step shape of cmhse_gru_pool_fwd_multi against the float64 oracle.

launch_steps (cmhse_amd/csrc/gru.hip) picks, for every time step of every request, one of about 30
kernel instantiations — the latency-shaped tile, the LDS-tiled step with 64- or 128-row tiles, the
step chain, the mid-size tile in 4-, 8- or 16-unit, 4- or 8-wave and 16-, 32- or 64-row forms, the
resident tail — from the step's active sequences, the request's widths, the other requests of the
call and the knobs.  The tests that compare two shapes bit for bit cannot see an error both share.
Each case of fwd_shapes.CASES is one call whose requests (up to four, one per pool mode) land on the
shapes its id names, and tests/test_fwd_shapes_cpu.py proves from the dispatch rule that they do.
Every output is compared with the oracle, a second run must give the same bits, and the training
cases (their kernels also write the gates and arg-max the BPTT reads) check every gradient.  (The
resident tail at every KB x MB: tests/test_gpu_chain.py test_forward_tail_as_one_resident_kernel.)"""
import numpy as np
import pytest
import torch

from conftest import assert_emb_close
from gpu_common import _blas_threads, grad_close

import fwd_shapes

pytestmark = pytest.mark.gpu

_ORACLE_POOL = {'LAST': 'seq2seq', 'MAX': 'maxout', 'ATTN': 'attention', 'ALL': 'seq2seq'}


def _layer(pool, I, H, seed):
  from cmhse_amd import decoder, layers
  torch.manual_seed(seed)
  if pool == 'ALL':
    layer = decoder.Seq2Seq_Decode(I, H)
  else:
    layer = getattr(layers, {'LAST': 'Seq2Seq', 'MAX': 'Maxout', 'ATTN': 'Attention'}[pool])(I, H)
  with torch.no_grad():
    layer.rnn.bias_ih_l0.normal_(0, 0.1)
    layer.rnn.bias_hh_l0.normal_(0, 0.1)
  return layer


def _inputs(j, rng, dev):
  """lens, the padded fp32 inputs (a float64 copy for the oracle), h0 and — token-fed — the ids and table."""
  lens = fwd_shapes.lens_of(j['counts'])
  S, T, I, H = len(lens), len(j['counts']), j['I'], j['H']
  tok = table = None
  if j['vocab']:
    table = rng.standard_normal((j['vocab'], I)).astype(np.float32)
    tok = rng.randint(0, j['vocab'], size=(S, T)).astype(np.int64)
    x = table[tok]
  else:
    x = rng.standard_normal((S, T, I)).astype(np.float32)
  for i, l in enumerate(lens):
    x[i, l:] = 0
  h0 = (0.5 * rng.standard_normal((S, H))).astype(np.float32) if j['h0'] else None
  return lens, x, h0, tok, table


def _oracle(oracle, j, x, lens, sd, h0):
  """(the expected output, the forward cache) in float64."""
  want, cache = oracle.pooled_gru_forward_cache(_ORACLE_POOL[j['pool']], x, lens, sd, h0)
  if j['pool'] == 'ALL':
    want = np.concatenate([cache['hs'][i, :l] for i, l in enumerate(lens)])
  return want, cache


def _backward(oracle, j, cache, lens, w):
  """The oracle's gradients for d(out) = w, in the type of the cache."""
  if j['pool'] != 'ALL':
    return oracle.pooled_gru_backward(cache, w.astype(cache['hs'].dtype))
  dhs = np.zeros_like(cache['hs'])
  starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
  for i, l in enumerate(lens):
    dhs[i, :l] = w[starts[i]:starts[i] + l]
  return oracle.gru_backward(cache, dhs)


def _id(case):
  return '%s[%s]' % (case[0], ','.join(sorted(t.replace(' ', '_') for t in case[5])))


def _apply_regime(regime, layer, inputs, rng):
  """A value regime of tests/value_regimes.py on one request: (fp32 state dict, x, h0, rng) -> the same,
  modified, loaded back into the layer.  The lengths and the padding stay as they are."""
  lens, x, h0, tok, table = inputs
  assert tok is None, 'a value regime scales the inputs: not for token-fed requests'
  sd = {n: v.detach().numpy().copy() for n, v in layer.state_dict().items()}
  sd, x, h0 = regime(sd, x.copy(), None if h0 is None else h0.copy(), rng)
  layer.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for n, v in sd.items()})
  x = np.ascontiguousarray(x, dtype=np.float32)
  for i, l in enumerate(lens):
    assert not x[i, l:].any()
  return layer, (lens, x, None if h0 is None else np.ascontiguousarray(h0, dtype=np.float32), tok, table)


def _setup(jobs, dev, regime=None):
  """The layers of a case's requests (on `dev`), their float64 state dicts, the inputs (_inputs) and
  the case's random stream.  `regime` (tests/value_regimes.py) modifies every request's numbers after
  they are drawn, from a random stream of its own: the baseline numbers of a case do not depend on it."""
  rng = np.random.RandomState(sum(j['counts'][0] + 3 * j['H'] for j in jobs))
  layers_, sds, data = [], [], []
  for k, j in enumerate(jobs):
    layer = _layer(j['pool'], j['I'], j['H'], seed=17 * k + j['H'])
    inputs = _inputs(j, rng, dev)
    if regime is not None:
      layer, inputs = _apply_regime(regime, layer, inputs, np.random.RandomState(977 + k))
    sds.append({'rnn.' + n: v.detach().numpy().astype(np.float64) for n, v in layer.state_dict().items()})
    layers_.append(layer.to(dev))
    data.append(inputs)
  return layers_, sds, data, rng


def _run_inference(jobs, layers_, data, dev, tail_stream):
  """One ops.gru_pool_fwd_multi call of a case, finished: [(out, forward context)] per request."""
  from cmhse_amd import evaluation, ops
  keep, reqs = [], []
  for j, layer, (lens, x, h0, tok, table) in zip(jobs, layers_, data):
    w_lin, b_lin, w_att = layer._extra_weights()
    weights = dict(w_ih=layer.rnn.weight_ih_l0.detach(), w_hh=layer.rnn.weight_hh_l0.detach(),
                   b_ih=layer.rnn.bias_ih_l0.detach(), b_hh=layer.rnn.bias_hh_l0.detach())
    if j['pool'] == 'ATTN':
      weights.update(w_lin=w_lin.detach(), b_lin=b_lin.detach(), w_att=w_att.detach().reshape(-1))
    req = dict(weights=weights, pool_mode=getattr(ops, 'POOL_' + j['pool']), lens=lens, I=j['I'], H=j['H'],
               device=dev)
    if tok is not None:
      tt, tb = torch.from_numpy(tok).to(dev), torch.from_numpy(table).to(dev)
      keep += [tt, tb]
      req.update(tok_ptrs=ops.padded_row_ptrs(tt), emb_table=tb)
    else:
      xt = torch.from_numpy(x).to(dev)
      keep.append(xt)
      req['x_ptrs'] = ops.padded_row_ptrs(xt)
    if h0 is not None:
      ht = torch.from_numpy(h0).to(dev)
      keep.append(ht)
      req['h0_ptrs'] = ops.padded_row_ptrs(ht)
    if j['plan'] is not None:
      req['step_plan'] = np.asarray(j['plan'], dtype=np.int32)
    if j.get('aliases'):      # prefix aliases (src, len): output rows S, S + 1, ... behind the request's own
      src, n = (np.asarray(a, dtype=np.int64) for a in zip(*j['aliases']))
      S = len(lens)
      req.update(out_rows=np.arange(S), aliases=(src, n, S + np.arange(len(src))), n_out=S + len(src))
    reqs.append(req)
  res = ops.gru_pool_fwd_multi(reqs, tail_stream=evaluation._tail_stream(dev) if tail_stream else None)
  torch.cuda.synchronize()
  del keep
  return res


def _run_training(jobs, layers_, data, ws, dev, after_forward=None):
  """One layers.run_grouped call of a case with its backward pass, every request on a job stream of
  its own: per request [out, dx, (dh0,) every parameter gradient].  `after_forward()` runs between the
  two passes, the forward finished (a test reads what the forward saved before the backward runs)."""
  from cmhse_amd import layers, ops
  calls, ins = [], []
  for j, layer, (lens, x, h0, tok, table) in zip(jobs, layers_, data):
    layer.zero_grad()
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    ht = torch.from_numpy(h0).to(dev).requires_grad_(True) if h0 is not None else None
    calls.append((layer, layers.SeqInput('padded', lens.astype(np.int64), layer.POOL), xt, ht, None))
    ins.append((xt, ht))
  st = ops.stream_set(dev)
  outs = layers.run_grouped(calls, [st[k] for k in range(len(calls))])
  if after_forward is not None:
    torch.cuda.synchronize()
    after_forward()
  sum((o * torch.from_numpy(w).to(dev)).sum() for o, w in zip(outs, ws)).backward()
  torch.cuda.synchronize()
  return [[o.detach().clone(), xt.grad.clone()] + ([ht.grad.clone()] if ht is not None else []) +
          [p.grad.clone() for p in layer.parameters()] for o, (xt, ht), layer in zip(outs, ins, layers_)]


@pytest.mark.parametrize('case', fwd_shapes.CASES, ids=[_id(c) for c in fwd_shapes.CASES])
def test_fwd_step_shape_vs_oracle(dev, oracle, tune, case):
  name, knobs, train, tail_stream, jobs, _ = case
  layers_, sds, data, rng = _setup(jobs, dev)
  tune(**knobs)
  ws = [rng.standard_normal((int(d[0].sum()) if j['pool'] == 'ALL' else len(d[0]), j['H'])).astype(np.float32)
        for j, d in zip(jobs, data)]

  def run_inference():
    return [[o.clone()] for o, _ in _run_inference(jobs, layers_, data, dev, tail_stream)]

  def run_training():
    return _run_training(jobs, layers_, data, ws, dev)

  run = run_training if train else run_inference
  first, again = run(), run()
  for k, (a, b) in enumerate(zip(first, again)):
    for i, (u, v) in enumerate(zip(a, b)):
      assert torch.equal(u, v), '%s: request %d result %d not reproducible from run to run' % (name, k, i)
  for k, (j, (lens, x, h0, _, _)) in enumerate(zip(jobs, data)):
    tag = '%s request %d (%s, I %d, H %d)' % (name, k, j['pool'], j['I'], j['H'])
    with _blas_threads():
      want, cache = _oracle(oracle, j, x, lens, sds[k], h0)
      if train:
        grads, dx, dh0 = _backward(oracle, j, cache, lens, ws[k])
    assert_emb_close(first[k][0].cpu().numpy(), want, tag)
    if not train:
      continue
    got = first[k]
    grad_close(got[1].cpu().numpy()[:, :dx.shape[1]], dx, tag + ' dx')
    if h0 is not None:
      grad_close(got[2].cpu().numpy(), dh0, tag + ' dh0')
    params = got[3:] if h0 is not None else got[2:]
    for (pn, _), g in zip(layers_[k].named_parameters(), params):
      grad_close(g.cpu().numpy(), grads['rnn.' + pn], tag + ' ' + pn)
