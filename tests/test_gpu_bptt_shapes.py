"""Every BPTT step shape of cmhse_gru_pool_bwd against the float64 oracle.

bwd_steps (cmhse_amd/csrc/bwd.hip) picks one of six kernels for each step of a chain from the
step's active sequences, H and the knobs; the tests that compare two shapes bit for bit cannot see
an error both shapes share.  Each case of bptt_shapes.CASES targets shapes no other oracle test
reaches — the 4- and 8-wave 32 x 32 tiles with dwordx4 and scalar loads, the mid-size tile over
many row tiles, the two-launch split step at its edges — and tests/test_bptt_shapes_cpu.py proves
from the dispatch rule that it lands on them.  (The resident tail at every KB x MB:
tests/test_gpu_chain.py test_bptt_tail_as_one_resident_kernel.)"""
import numpy as np
import pytest
import torch

from conftest import assert_emb_close
from gpu_common import _blas_threads, grad_close

import bptt_shapes

pytestmark = pytest.mark.gpu

_CLS = {'attention': 'Attention', 'maxout': 'Maxout', 'seq2seq': 'Seq2Seq'}


@pytest.mark.parametrize('case', bptt_shapes.CASES, ids=[c[0] for c in bptt_shapes.CASES])
def test_bptt_step_shape_vs_oracle(dev, oracle, tune, case):
  """Forward output and every gradient (d input, d h0 through the t = -1 launch, all parameters,
  nonzero biases) against the float64 oracle; a second run bitwise identical (no atomics on these
  paths)."""
  from cmhse_amd import layers
  name, knobs, S, T, I, H, profile, pool, _ = case
  lens = bptt_shapes.lens_of(profile)
  assert len(lens) == S and lens.max() == T
  rng = np.random.RandomState(S + 7 * H)
  torch.manual_seed(H)
  layer = getattr(layers, _CLS[pool])(I, H)
  with torch.no_grad():
    layer.rnn.bias_ih_l0.normal_(0, 0.1)
    layer.rnn.bias_hh_l0.normal_(0, 0.1)
  sd = {'rnn.' + k: v.detach().numpy().astype(np.float64) for k, v in layer.state_dict().items()}
  layer = layer.to(dev)
  x = np.zeros((S, T, I), dtype=np.float32)
  for i, l in enumerate(lens):
    x[i, :l] = rng.standard_normal((l, I))
  h0 = (0.5 * rng.standard_normal((S, H))).astype(np.float32)
  w = rng.standard_normal((S, H)).astype(np.float32)
  tune(**knobs)

  def run():
    layer.zero_grad()
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    ht = torch.from_numpy(h0).to(dev).requires_grad_(True)
    y = layer(xt, torch.from_numpy(lens), ht)
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    return [y.detach().clone(), xt.grad.clone(), ht.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

  first, again = run(), run()
  for i, (a, b) in enumerate(zip(first, again)):
    assert torch.equal(a, b), '%s: result %d not reproducible from run to run' % (name, i)
  with _blas_threads():
    want, cache = oracle.pooled_gru_forward_cache(pool, x, lens, sd, h0)
    grads, dx, dh0 = oracle.pooled_gru_backward(cache, w.astype(np.float64))
  assert_emb_close(first[0].cpu().numpy(), want, name)
  grad_close(first[1].cpu().numpy()[:, :dx.shape[1]], dx, name + ' dx')
  grad_close(first[2].cpu().numpy(), dh0, name + ' dh0')
  for (pn, _), got in zip(layer.named_parameters(), first[3:]):
    grad_close(got.cpu().numpy(), grads['rnn.' + pn], name + ' ' + pn)


# Jobs of one cmhse_gru_pool_bwd_multi call: (cls, I, H, profile).  Aligned at their last step,
# launch i = 0 holds two vec Waves4 jobs of different H in ONE launch (per-job workgroup offsets,
# u_tiles of 64 and 72 columns), a scalar Waves4 job beside them and a Split job; the chains have
# different lengths, so the later launches mix other subsets (tests/test_bptt_shapes_cpu.py).
MIXED_JOBS = [('Attention', 20, 64, (600, 600, 580, 550)),
              ('Maxout', 16, 72, (560, 560, 560, 540, 530, 520)),
              ('Maxout', 12, 45, (300, 290, 280)),
              ('Seq2Seq', 24, 128, (100, 90, 80, 60, 40))]


def test_grouped_backward_mixed_step_shapes(dev, oracle):
  """Jobs whose BPTT steps take different kernels at the same launch: outputs and gradients of
  the grouped call bit-identical to one call per job, and every gradient against the float64
  oracle."""
  from cmhse_amd import layers
  rng = np.random.RandomState(21)
  torch.manual_seed(6)
  encs, sds, xs, lens_l, rows_l, h0_l = [], [], [], [], [], []
  for cls, I, H, profile in MIXED_JOBS:
    enc = getattr(layers, cls)(I, H)
    with torch.no_grad():
      enc.rnn.bias_ih_l0.normal_(0, 0.1)
      enc.rnn.bias_hh_l0.normal_(0, 0.1)
    sds.append({'rnn.' + k: v.detach().numpy().astype(np.float64) for k, v in enc.state_dict().items()})
    encs.append(enc.to(dev))
    lens = bptt_shapes.lens_of(profile)
    x = np.zeros((len(lens), len(profile), I), dtype=np.float32)
    for i, l in enumerate(lens):
      x[i, :l] = rng.standard_normal((l, I))
    xs.append(x)
    lens_l.append(lens)
    rows_l.append(torch.from_numpy(np.concatenate([x[i, :l] for i, l in enumerate(lens)])).to(dev).requires_grad_(True))
    h0_l.append(torch.from_numpy((0.5 * rng.standard_normal((len(lens), H))).astype(np.float32)).to(dev)
                .requires_grad_(True))
  ws = [rng.standard_normal((len(l), e.rnn.hidden_size)).astype(np.float32) for l, e in zip(lens_l, encs)]

  def calls():
    return [e.call_rows(r, l, h) for e, r, l, h in zip(encs, rows_l, lens_l, h0_l)]

  def grads_of(outs):
    params = [p for e in encs for p in e.parameters()] + rows_l + h0_l
    for p in params:
      p.grad = None
    sum((o * torch.from_numpy(w).to(dev)).sum() for o, w in zip(outs, ws)).backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in params], [o.detach().clone() for o in outs]

  g_grp, o_grp = grads_of(layers.run_grouped(calls()))
  g_sep, o_sep = grads_of([layers.run_grouped([c])[0] for c in calls()])
  for a, b in zip(o_grp, o_sep):
    assert torch.equal(a, b)
  for i, (a, b) in enumerate(zip(g_grp, g_sep)):
    assert torch.equal(a, b), i

  n_par = [len(list(e.parameters())) for e in encs]
  pool = {'Attention': 'attention', 'Maxout': 'maxout', 'Seq2Seq': 'seq2seq'}
  for k, (cls, I, H, profile) in enumerate(MIXED_JOBS):
    tag = '%s H%d' % (cls, H)
    h0 = h0_l[k].detach().cpu().numpy()
    with _blas_threads():
      want, cache = oracle.pooled_gru_forward_cache(pool[cls], xs[k], lens_l[k], sds[k], h0)
      grads, dx, dh0 = oracle.pooled_gru_backward(cache, ws[k].astype(np.float64))
    assert_emb_close(o_grp[k].cpu().numpy(), want, tag)
    p0 = sum(n_par[:k])
    for (pn, _), got in zip(encs[k].named_parameters(), g_grp[p0:p0 + n_par[k]]):
      grad_close(got.cpu().numpy(), grads['rnn.' + pn], tag + ' ' + pn)
    drows = g_grp[sum(n_par) + k].cpu().numpy()
    want_rows = np.concatenate([dx[i, :l] for i, l in enumerate(lens_l[k])])
    grad_close(drows, want_rows, tag + ' d rows')
    grad_close(g_grp[sum(n_par) + len(encs) + k].cpu().numpy(), dh0, tag + ' dh0')
