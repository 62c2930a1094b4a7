"""Prefix sharing of the text tower (tunable share_prefix): a video's first caption is not encoded but
pooled from the first rows of its paragraph (cmhse_seq_batch.n_alias).  The claim is IDENTITY: every
comparison is share_prefix=1 against share_prefix=0 with np.array_equal on all six matrices (and on the
ranks of both directions where the call ranks) — no tolerance anywhere in this file."""
import argparse
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_common import KEYS6, MeterLog, golden_model, golden_opt

from cmhse_amd import evaluation, ops, synthetic

pytestmark = pytest.mark.gpu

quiet = lambda *a, **k: None


def _to_dev(batches, dev):
  return [tuple(x.to(dev) if isinstance(x, torch.Tensor) and i < 4 else x for i, x in enumerate(b))
          for b in batches]


def _device_pass(opt, model, batches, **kw):
  """encode_data_device + both rankings -> ({name: array}, aliases the call reports)."""
  cat = evaluation.encode_data_device(opt, model, batches, logging=quiet, **kw)[0]
  n_alias = evaluation.SHARE_STATS['aliases']
  out = {k: cat[k] for k in KEYS6}
  if cat['vid_emb'].shape == cat['para_emb'].shape:
    out['rank_i2t'], out['top1_i2t'] = ops.sim_rank(cat['vid_emb'], cat['para_emb'])
    out['rank_t2i'], out['top1_t2i'] = ops.sim_rank(cat['para_emb'], cat['vid_emb'])
  torch.cuda.synchronize()
  return {k: v.cpu().numpy() for k, v in out.items()}, n_alias


def _identical(on, off, what):
  assert sorted(on) == sorted(off)
  for k in sorted(on):
    assert on[k].shape == off[k].shape, (what, k)
    assert np.array_equal(on[k], off[k]), '%s: %s differs in %d of %d entries' % (
        what, k, int((on[k] != off[k]).sum()), on[k].size)


def _both(fn, what, want_aliases):
  """fn() under share_prefix 1 and 0: identical results; the shared run reports `want_aliases`."""
  with ops.tuned(share_prefix=0):
    off, n_off = fn()
  with ops.tuned(share_prefix=1):
    on, n_on = fn()
  assert n_off == 0, what
  assert n_on == want_aliases, '%s: %d aliases reported, %d expected' % (what, n_on, want_aliases)
  _identical(on, off, what)
  return on


LOADERS = {
    'ragged0': lambda: (synthetic.ragged_spec(24, seed=0), 5),
    'ragged1': lambda: (synthetic.ragged_spec(24, seed=1), 7),
    'ragged2': lambda: (synthetic.ragged_spec(24, seed=2), 24),
    'ragged3': lambda: (synthetic.ragged_spec(24, seed=3), 4),
    'uniform': lambda: (synthetic.uniform_spec(10, clips=3, frames=6, words=5), 4),
}


@pytest.mark.parametrize('loader', sorted(LOADERS))
def test_every_path_of_the_validation_pass(dev, loader):
  """One group, several groups, a kept plan (twice, and across a flip of the tunable), the NumPy path
  (host batches) and a share of the loader under the whole loader's step plan.  Every video of these
  loaders qualifies, so the alias count is the video count: sharing that never engages fails."""
  g = load_golden('model_attention.npz')
  opt, model = golden_model('attention', g)
  spec, bs = LOADERS[loader]()
  host = synthetic.make_batches(spec, bs, opt.img_dim, opt.vocab_size, seed=11)
  batches = _to_dev(host, dev)
  n = spec.n_videos
  whole = _both(lambda: _device_pass(opt, model, batches), 'one group', n)
  # several super-batches (one or two loader batches each): the split's step plan pins the kernels
  small = 2 * max(b[0].numel() * 4 + b[2].numel() * 4 for b in batches)
  several = _both(lambda: _device_pass(opt, model, batches, superbatch_bytes=small), 'several groups', n)
  _identical(several, whole, 'several groups against one')
  # a plan kept between passes: built by the first pass, served from by the second
  plans = {0: {}, 1: {}}

  def planned():
    return _device_pass(opt, model, batches, plan=plans[ops.tune('share_prefix')])
  _both(planned, 'plan, first pass', n)
  again = _both(planned, 'plan, second pass', n)
  _identical(again, whole, 'plan against none')
  assert plans[1][0]['n_alias'] == n and plans[0][0]['n_alias'] == 0
  one = {}      # ONE plan dict under a flipping tunable: rebuilt, never served across the flip
  _both(lambda: _device_pass(opt, model, batches, plan=one), 'one plan, flipped tunable', n)
  _both(lambda: _device_pass(opt, model, batches, plan=one), 'one plan, flipped again', n)

  # the NumPy path: host batches through encode_data (tokens compared on the host)
  def numpy_path():
    res = evaluation.encode_data(opt, model, synthetic.ListLoader(host), logging=quiet)
    n_alias = evaluation.SHARE_STATS['aliases']
    out = dict(zip(KEYS6, res[:6]))
    out['rank_i2t'] = evaluation.i2t(res[0], res[1])[2]
    out['rank_t2i'] = evaluation.t2i(res[0], res[1])[2]
    return {k: np.array(v) for k, v in out.items()}, n_alias
  host_res = _both(numpy_path, 'encode_data', n)
  for k in KEYS6:
    assert np.array_equal(host_res[k], whole[k]), k
  # a share of the loader under the step plan of the whole loader
  if len(batches) > 1:
    sp = evaluation.split_step_plan(batches)
    cut = len(batches) // 2
    n_share = sum(len(b[8]) for b in batches[:cut])
    share = _both(lambda: _device_pass(opt, model, batches[:cut], step_plan=sp), 'share of the split', n_share)
    for k, rows in (('cap_emb', sum(sum(b[9]) for b in batches[:cut])), ('para_ctx', n_share), ('para_emb', n_share)):
      assert np.array_equal(share[k], whole[k][:rows]), k


def _anet_setup(dev, n_videos, H, rnn_type='attention', img_dim=64, seed=0):
  from cmhse_amd.model import VSE
  opt = argparse.Namespace(
      margin=0.2, word_dim=300, embed_size=H, grad_clip=0.0, learning_rate=0.001, max_violation=False,
      img_dim=img_dim, measure='cosine', rnn_type=rnn_type, img_first_size=H, cap_first_size=H,
      low_level_loss=False, weak_low_level_loss=False, reconstruct_loss=False,
      lowest_reconstruct_loss=False, norm=False, data_name='anet_precomp', vocab_size=300)
  torch.manual_seed(4)
  model = VSE(opt)
  spec = synthetic.anet_like_spec(n_videos, seed=seed)
  batches = _to_dev(synthetic.make_batches(spec, 32, img_dim, opt.vocab_size, seed=3), dev)
  return opt, model, spec, batches


def test_the_step_plan_does_not_move(dev):
  """Which kernel serves step t is chosen from the active count of step t.  With tiny_max_seqs =
  mid_max_seqs = 256 the text tower of this split leaves the tiled kernel at step 33 with its first
  captions and at step 31 without them: a reduced request that chose its kernels from its own counts
  would run steps 31 and 32 of every long sequence on the other kernel (K in 8 slices: other bits)."""
  opt, model, spec, batches = _anet_setup(dev, 256, 256)
  num_caps = np.asarray(spec.num_clips, dtype=np.int64)
  len_cap = np.asarray(spec.words_per_sent, dtype=np.int64)
  starts = np.cumsum(num_caps) - num_caps
  len_par = np.add.reduceat(len_cap, starts)
  kept, _ = evaluation.text_prefix_aliases(len_cap, len_par, num_caps)
  with_first = int((ops.step_counts(np.concatenate([len_cap, len_par])) > 256).sum())
  without = int((ops.step_counts(np.concatenate([len_cap[kept], len_par])) > 256).sum())
  assert (with_first, without) == (33, 31)      # else this test tests nothing
  with ops.tuned(tiny_max_seqs=256, mid_max_seqs=256):
    _both(lambda: _device_pass(opt, model, batches), 'plan trap, one group', 256)
    small = 3 * max(b[0].numel() * 4 + b[2].numel() * 4 for b in batches)
    _both(lambda: _device_pass(opt, model, batches, superbatch_bytes=small), 'plan trap, several groups', 256)


def test_a_kept_plan_keeps_the_original_step_plan(dev):
  """A plan dict built in a pass that was given a split step plan and served later without one, and
  the reverse: the reduced request must choose its kernels from the ORIGINAL lengths either way (here
  the split's plan equals the group's own counts, so without sharing the two passes are the same
  bits).  On the plan-trap fixture: a served pass that fell back to the reduced request's own counts
  would run steps 31 and 32 on the other kernel."""
  opt, model, spec, batches = _anet_setup(dev, 256, 256)
  sp = evaluation.split_step_plan(batches)
  with ops.tuned(tiny_max_seqs=256, mid_max_seqs=256):
    with ops.tuned(share_prefix=0):
      want, _ = _device_pass(opt, model, batches)
    for first, second in (({'step_plan': sp}, {}), ({}, {'step_plan': sp})):
      plans = {0: {}, 1: {}}

      def pass_with(kw):
        return lambda: _device_pass(opt, model, batches, plan=plans[ops.tune('share_prefix')], **kw)
      built = _both(pass_with(first), 'plan built %s' % sorted(first), 256)
      served = _both(pass_with(second), 'plan served %s' % sorted(second), 256)
      assert plans[1][0]['n_alias'] == 256 and plans[1][0]['t_own_plan'] is not None
      _identical(built, want, 'built against no plan')
      _identical(served, want, 'served against no plan')


def test_the_precondition_is_checked_on_the_data(dev):
  """A third of the videos do not satisfy 'the first caption is the paragraph's prefix': one token of
  the prefix changed, the paragraph truncated below the first caption's length, or the caption differs
  from the prefix by an out-of-range id pair (ids out of range on BOTH sides at the same place still
  match: raw ids are compared and both are clamped alike).  Identity, and exactly the untouched videos
  are aliased — on device tokens and on host tokens."""
  g = load_golden('model_attention.npz')
  opt, model = golden_model('attention', g)
  spec = synthetic.ragged_spec(30, seed=7, max_words=9)
  host = synthetic.make_batches(spec, 8, opt.img_dim, opt.vocab_size, seed=5)
  touched = 0
  v_global = 0
  edited = []
  for b in host:
    b = list(b)
    caps, pars, len_par = b[1].clone(), b[3].clone(), b[7].clone()
    first = np.cumsum(b[9]) - np.asarray(b[9])
    for v in range(len(b[9])):
      l0 = int(b[5][first[v]])
      kind = v_global % 9
      if kind == 0:                      # one token of the paragraph's prefix changed
        pars[v, l0 - 1] = (int(pars[v, l0 - 1]) + 1 - 4) % (opt.vocab_size - 4) + 4
        touched += 1
      elif kind == 3 and l0 > 1:         # the paragraph ends inside the first caption
        len_par[v] = l0 - 1
        touched += 1
      elif kind == 6:                    # an out-of-range id on the caption's side only
        caps[first[v], 0] = opt.vocab_size + 5
        touched += 1
      elif kind == 1:                    # out of range on both sides alike: still a prefix
        caps[first[v], 0] = opt.vocab_size + 7
        pars[v, 0] = opt.vocab_size + 7
      elif kind == 2:
        caps[first[v], l0 - 1] = -2
        pars[v, l0 - 1] = -2
      v_global += 1
    b[1], b[3], b[7] = caps, pars, len_par
    edited.append(tuple(b))
  assert 7 <= touched <= 10      # a third of the 30 videos
  batches = _to_dev(edited, dev)
  on_dev = _both(lambda: _device_pass(opt, model, batches), 'device tokens', 30 - touched)

  def numpy_path():
    res = evaluation.encode_data(opt, model, synthetic.ListLoader(edited), logging=quiet)
    return {k: np.array(v) for k, v in zip(KEYS6, res[:6])}, evaluation.SHARE_STATS['aliases']
  on_host = _both(numpy_path, 'host tokens', 30 - touched)
  for k in KEYS6:
    assert np.array_equal(on_host[k], on_dev[k]), k


@pytest.mark.parametrize('rnn_type', ['maxout', 'seq2seq'])
def test_other_poolings_do_not_alias(dev, rnn_type):
  g = load_golden('model_%s.npz' % rnn_type)
  opt, model = golden_model(rnn_type, g)
  spec = synthetic.ragged_spec(24, seed=2)
  batches = _to_dev(synthetic.make_batches(spec, 6, opt.img_dim, opt.vocab_size, seed=11), dev)
  _both(lambda: _device_pass(opt, model, batches), rnn_type, 0)


def test_a_training_step_is_untouched(dev):
  """VSE.train_emb never aliases (the backward pass needs every sequence's own rows): losses and
  every parameter gradient bitwise against share_prefix=0.  The tokens of the batch are all different,
  so every row of the embedding table's gradient receives exactly two float-atomic contributions (its
  caption's and its paragraph's) and their order cannot show: embed.weight is compared bitwise too."""
  from cmhse_amd.model import VSE
  opt = golden_opt('attention', low_level_loss=True, norm=True, vocab_size=400)
  torch.manual_seed(5)
  model_a = VSE(opt)
  model_b = VSE(opt)
  model_b.load_state_dict(copy.deepcopy(model_a.state_dict(opt)), opt)
  spec = synthetic.ragged_spec(9, seed=2, max_frames=11, max_video=13)
  batch = list(synthetic.make_batches(spec, 9, opt.img_dim, opt.vocab_size, seed=3)[0])
  caps, pars = batch[1].clone(), batch[3].clone()
  ids = torch.randperm(opt.vocab_size - 4, generator=torch.Generator().manual_seed(1)) + 4
  first = np.cumsum(batch[9]) - np.asarray(batch[9])
  at = 0
  for v in range(len(batch[9])):
    row = []
    for c in range(batch[9][v]):
      n = int(batch[5][first[v] + c])
      caps[first[v] + c, :n] = ids[at:at + n]
      row.append(ids[at:at + n])
      at += n
    pars[v, :int(batch[7][v])] = torch.cat(row)
  assert at <= len(ids)
  batch[1], batch[3] = caps, pars
  logs = []
  for model, share in [(model_a, 0), (model_b, 1)]:
    with ops.tuned(share_prefix=share):
      model.logger = MeterLog()
      model.train_start(opt)
      model.train_emb(opt, *batch)
      torch.cuda.synchronize()
    logs.append([c for c in model.logger.calls if c[0].startswith('Le')])
  assert logs[0] == logs[1] and len(logs[0]) >= 2
  for ma, mb in zip(model_a._modules(), model_b._modules()):
    for (na, pa), (nb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
      assert na == nb and pa.grad is not None and pb.grad is not None
      assert torch.equal(pa.grad, pb.grad), na


# ---- the ABI -------------------------------------------------------------------------------------
def _weights(dev, I, H, attn, seed=3):
  g = torch.Generator().manual_seed(seed)
  w = dict(w_ih=torch.randn(3 * H, I, generator=g).mul_(0.1), w_hh=torch.randn(3 * H, H, generator=g).mul_(0.05),
           b_ih=torch.randn(3 * H, generator=g).mul_(0.1), b_hh=torch.randn(3 * H, generator=g).mul_(0.1))
  if attn:
    w.update(w_lin=torch.randn(H, H, generator=g).mul_(0.05), b_lin=torch.randn(H, generator=g).mul_(0.1),
             w_att=torch.randn(1, H, generator=g).mul_(0.2))
  return {k: v.to(dev) for k, v in w.items()}


@pytest.mark.parametrize('tokens', [True, False])
def test_alias_rows_equal_the_prefix_encoded_on_its_own(dev, tokens):
  """ops level: S sequences plus, for some of them, their prefixes as sequences of their own, against
  the S sequences with those prefixes as aliases: every output row identical."""
  S, T, I, H, V = 40, 13, 20, 64, 50
  rng = np.random.RandomState(2)
  g = torch.Generator().manual_seed(2)
  lens = rng.randint(1, T + 1, size=S).astype(np.int64)
  lens[0] = T
  src = np.asarray([0, 3, 3, 7, 11, 39, 20], dtype=np.int64)
  a_len = np.asarray([int(rng.randint(1, lens[s] + 1)) for s in src], dtype=np.int64)
  a_len[0], a_len[1] = lens[0], 1            # a whole sequence, and a single step
  w = _weights(dev, I, H, True)
  if tokens:
    data = torch.randint(0, V, (S, T), generator=g).to(dev)
    table = torch.randn(V, I, generator=g).to(dev)
    feed = dict(emb_table=table)
    key = 'tok_ptrs'
  else:
    data = torch.randn(S, T, I, generator=g).to(dev)
    feed = {}
    key = 'x_ptrs'
  ptrs = ops.padded_row_ptrs(data)
  # separately: [sequences | prefixes]
  full = dict(weights=w, pool_mode=ops.POOL_ATTN, lens=np.concatenate([lens, a_len]), I=I, H=H, device=dev,
              step_plan=ops.step_counts(np.concatenate([lens, a_len])), **feed)
  full[key] = np.concatenate([ptrs, ptrs[src]])
  want, _ = ops.gru_pool_fwd(**full)
  # aliased: the same output rows, the same step plan
  al = dict(weights=w, pool_mode=ops.POOL_ATTN, lens=lens, I=I, H=H, device=dev,
            step_plan=ops.step_counts(np.concatenate([lens, a_len])), out_rows=np.arange(S),
            aliases=(src, a_len, S + np.arange(len(src))), n_out=S + len(src), **feed)
  al[key] = ptrs
  got, _ = ops.gru_pool_fwd(**al)
  torch.cuda.synchronize()
  assert got.shape == want.shape
  assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_alias_argument_errors(dev):
  S, T, I, H = 6, 5, 8, 16
  data = torch.randn(S, T, I, generator=torch.Generator().manual_seed(0)).to(dev)
  lens = np.asarray([5, 4, 4, 2, 1, 3], dtype=np.int64)
  base = dict(lens=lens, I=I, H=H, device=dev, x_ptrs=ops.padded_row_ptrs(data), out_rows=np.arange(S),
              aliases=(np.asarray([3]), np.asarray([2]), np.asarray([S])), n_out=S + 1)
  ok, _ = ops.gru_pool_fwd(weights=_weights(dev, I, H, True), pool_mode=ops.POOL_ATTN, **base)
  torch.cuda.synchronize()
  assert ok.shape == (S + 1, H)
  for mode in (ops.POOL_LAST, ops.POOL_MAX):                 # aliases on a non-attention request
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
      ops.gru_pool_fwd(weights=_weights(dev, I, H, False), pool_mode=mode, **base)
  with pytest.raises(RuntimeError, match=r'\(-1\)'):         # ... on a save-for-backward request
    ops.gru_pool_fwd(weights=_weights(dev, I, H, True), pool_mode=ops.POOL_ATTN, save_for_backward=True, **base)
  with pytest.raises(ValueError):                            # alias_len beyond the source: the schedule refuses
    ops.SeqSchedule(lens, dev, x_ptrs=base['x_ptrs'], out_rows=np.arange(S),
                    aliases=(np.asarray([3]), np.asarray([3]), np.asarray([S])), n_out=S + 1)
  # output rows: each of the n_out rows once, inside `out`
  for rows, al_row, n_out in ((np.arange(S), S + 1, S + 1), (np.arange(S), S - 1, S + 1), (np.arange(S) + 1, 0, S),
                              (np.arange(S), -1, S + 1)):
    with pytest.raises(ValueError):
      ops.SeqSchedule(lens, dev, x_ptrs=base['x_ptrs'], out_rows=rows,
                      aliases=(np.asarray([3]), np.asarray([2]), np.asarray([al_row])), n_out=n_out)
  with pytest.raises(ValueError):                            # a caller's `out` without the alias rows
    ops.gru_pool_fwd(weights=_weights(dev, I, H, True), pool_mode=ops.POOL_ATTN,
                     out=torch.empty(S, H, device=dev), **base)
  # ... and so does the library when it is handed one anyway
  for bad_src, bad_len in ((None, 3), (None, 0), (S, None), (-1, None)):
    sched = ops.SeqSchedule(lens, dev, x_ptrs=base['x_ptrs'], out_rows=np.arange(S),
                            aliases=(np.asarray([3]), np.asarray([2]), np.asarray([S])), n_out=S + 1)
    if bad_len is not None:
      sched.alias_host[1][0] = bad_len
    if bad_src is not None:
      sched.alias_host[0][0] = bad_src
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
      ops.gru_pool_fwd(weights=_weights(dev, I, H, True), pool_mode=ops.POOL_ATTN, lens=lens, I=I, H=H,
                       device=dev, x_ptrs=base['x_ptrs'], sched=sched)
  torch.cuda.synchronize()
  assert ops.async_status() == 0


def test_tok_prefix_check_kernel(dev):
  """cmhse_tok_prefix_check against NumPy: equal prefixes, one id changed at the first / last / a
  middle place, b shorter than a, empty-by-length pairs, lengths over one wave's 64 ids."""
  rng = np.random.RandomState(5)
  n, T = 200, 150
  a = rng.randint(-3, 1 << 40, size=(n, T)).astype(np.int64)
  b = a.copy()
  a_len = rng.randint(1, T + 1, size=n).astype(np.int64)
  b_len = np.minimum(T, a_len + rng.randint(0, 9, size=n)).astype(np.int64)
  a_len[3::20] = 0                            # the empty sequence is a prefix of anything,
  b_len[3::40] = 0                            # of the empty sequence too
  want = np.ones(n, dtype=bool)
  for i in range(0, n, 4):
    where = [0, a_len[i] - 1, a_len[i] // 2][(i // 4) % 3]
    b[i, where] ^= 1 << ((i * 7) % 40)
    want[i] = False
  for i in range(1, n, 10):
    if a_len[i] > 1:
      b_len[i] = a_len[i] - 1
      want[i] = False
  for i in range(2, n, 25):                   # a difference just behind the prefix does not count
    if a_len[i] < T:
      b[i, a_len[i]] += 1
  ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  flags = ops.tok_prefix_check(ops.padded_row_ptrs(ta), ops.padded_row_ptrs(tb), a_len, b_len, dev)
  torch.cuda.synchronize()
  assert np.array_equal(flags.cpu().numpy() != 0, want)
