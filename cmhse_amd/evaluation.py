"""Host-side mirror of the reference's `evaluation.py` on the MI355X hot path.

Exports the names train.py imports (train.py:10): i2t, t2i, AverageMeter, LogCollector,
encode_data, LogReporter — with the reference's signatures and return values
(/root/reference/evaluation.py:18-213).

MI355X-first differences in HOW (not WHAT) things are computed:
  * encode_data fuses many loader batches into one "super-batch" per encoder launch sequence
    (clips and whole-video streams of all those batches go through `clip_enc` together, sentences
    and paragraphs through `txt_enc` together), keeps every embedding on the device, and still
    reports the per-loader-batch 'Letest' loss (evaluation.py:129) and returns the same 8-tuple;
  * i2t / t2i never build the N x N matrix or sort: ranks and arg-max come out of the fused
    similarity kernel (cmhse_sim_rank).
"""
from __future__ import annotations

import contextlib
import gc
import hashlib
import itertools
import os
import time
import collections
from collections import OrderedDict

import numpy
import numpy as np
import torch

from . import ops


class AverageMeter(object):
  """Running value + weighted mean of one logged quantity — the contract of
  /root/reference/evaluation.py:18-45: `update(val, n=0)` (a weight of 0 only refreshes `val`),
  `avg = sum / (1e-4 + count)` (so an empty meter reads 0, not NaN), and the printed form."""
  __slots__ = ('val', 'avg', 'sum', 'count')

  def __init__(self):
    self.reset()

  def reset(self):
    self.val = self.avg = self.sum = self.count = 0

  def update(self, val, n=0):
    self.val = val
    self.sum += n * val
    self.count += n
    self.avg = self.sum / (self.count + 1e-4)

  def __str__(self):
    return str(self.val) if self.count == 0 else '%.4f (%.4f)' % (self.val, self.avg)


class LogCollector(object):
  """Named AverageMeters in first-use order (/root/reference/evaluation.py:48-72): what
  VSE.forward_loss writes to (`model.logger.update('Le'+name, value, n)`, model.py:291) and what
  train.py prints / sends to tensorboard.

  Values may arrive late: VSE.train_emb hands the step's loss values over as a copy that is still
  in flight (`defer`), so that the host can queue the next step instead of waiting for this one.
  Everything that READS the collector (`meters`, str()) first settles what is outstanding, and
  `update` / `tb_log` calls made in the meantime wait in the same queue, so every reader — and the
  tensorboard sink — sees exactly the reference's sequence of updates."""

  def __init__(self):
    self._meters = OrderedDict()
    self._deferred = []

  def _update(self, k, v, n=0):
    self._meters.setdefault(k, AverageMeter()).update(v, n)

  def update(self, k, v, n=0):
    if self._deferred:
      self._deferred.append(lambda: self._update(k, v, n))
    else:
      self._update(k, v, n)

  def defer(self, thunk):
    """Queue `thunk()` (which calls `_update`) to run before the next read."""
    self._deferred.append(thunk)

  def settle(self):
    while self._deferred:
      self._deferred.pop(0)()

  @property
  def meters(self):
    self.settle()
    return self._meters

  @meters.setter
  def meters(self, value):      # `collector.meters = OrderedDict()`: a reset
    # what is still queued belongs to the meters being replaced: deliver it first (the reference's
    # tb_log would already have emitted those rows), then reset
    self.settle()
    self._meters = value

  def flush(self):
    """Deliver everything still queued (late loss values, tb_log rows): call after the LAST step of
    a loop that no reader follows (a reader — `meters`, str(), train_start / val_start — does it
    implicitly)."""
    self.settle()

  def __str__(self):
    return '  '.join('%s %s' % (k, m) for k, m in self.meters.items())

  # A collector that still holds late values (closures over device events) cannot be pickled or
  # deep-copied as it is: both first settle what is outstanding, so the copy carries plain meters.
  def __getstate__(self):
    self.settle()
    return {'_meters': self._meters, '_deferred': []}

  def __deepcopy__(self, memo):
    import copy
    self.settle()
    other = LogCollector()
    other._meters = copy.deepcopy(self._meters, memo)
    return other

  def tb_log(self, tb_logger, prefix='', step=None):
    """evaluation.py:68-72.  train.py calls this after EVERY step (train.py:215).  While the step's
    loss values are still in flight the call takes its place in the queue instead of waiting for
    them: the sink receives exactly the (key, value, step) triples it would have, a step later in
    wall time, and the host goes on queueing the next step."""
    if self._deferred:
      self._deferred.append(lambda: self._tb_log_now(tb_logger, prefix, step))
    else:
      self._tb_log_now(tb_logger, prefix, step)

  def _tb_log_now(self, tb_logger, prefix, step):
    for k, m in self._meters.items():
      tb_logger.log_value(prefix + k, m.val, step=step)


def LogReporter(tb_logger, result, epoch, name):
  """/root/reference/evaluation.py:74-78: one tensorboard scalar per report entry."""
  for key, value in result.items():
    tb_logger.log_value(name + key, value, step=epoch)


# ---------------------------------------------------------------------------------------------
# encode_data
# ---------------------------------------------------------------------------------------------
def _to_dev(t, device):
  return t if t.is_cuda else t.to(device, non_blocking=True)


# Schedule of encode_group (module attributes; all give bit-identical embeddings, tested):
#   GROUP_TOWERS  step t of both level-1 encoders in shared launches (default);
#   EARLY_POOL    the visual attention pass beside the text chain's few-sequence tail (default);
#   TWO_STREAMS   instead: the two towers on two HIP streams (+3 % wall, measured; off).
TWO_STREAMS = [False]
GROUP_TOWERS = [True]
EARLY_POOL = [True]


def _tail_stream(device):
  return ops.stream_set(device)[0]


def _side_streams(device):
  st = ops.stream_set(device)
  return st[0], st[1]


PIPELINE_UPLOAD = [True]      # pinned host batches are pulled chunk by chunk under the step pipeline
UPLOAD_CHUNK = [8]             # time steps per pull chunk once the pipeline is full (4 and 8 level, 12+ slower: DESIGN §7b)


def _copy_stream(device):
  # a stream on a hardware queue of its own (ops.stream_set): a copy stream that shares the compute
  # stream's hardware queue runs in submission order with it — no overlap at all, measured
  return ops.stream_set(device)[1]


# Pinned float32 blocks for the deferred 'Letest' values, recycled by flush(): page-locking a fresh
# block while the GPU is busy costs milliseconds (see ops.upload).
_HOST_SCALARS = []
_HOST_EVENTS = []


def _host_scalars(n):
  """A pinned float32 BLOCK of at least n elements (callers slice it for use and hand the whole
  block back to the pool, so its capacity never shrinks)."""
  for i, h in enumerate(_HOST_SCALARS):
    if h.numel() >= n:
      return _HOST_SCALARS.pop(i)
  return torch.empty(max(n, 1024), dtype=torch.float32).pin_memory()


_HOST_ROWS, _HOST_ROW_EVENTS = [], []


def _hold_host_rows(stream, tensors, keep=3):
  while _HOST_ROWS and (_HOST_ROWS[0][0].query() or len(_HOST_ROWS) >= keep):
    if not _HOST_ROWS[0][0].query():
      _HOST_ROWS[0][0].synchronize()
    _HOST_ROW_EVENTS.append(_HOST_ROWS.pop(0)[0])
  ev = _HOST_ROW_EVENTS.pop() if _HOST_ROW_EVENTS else torch.cuda.Event()
  ev.record(stream)
  _HOST_ROWS.append((ev, tensors))


def _pinned_f32(t):
  return (isinstance(t, (torch.Tensor, ops.Ragged)) and not t.is_cuda and t.dtype == torch.float32
          and t.is_contiguous() and t.is_pinned())


def _empty_like_on(t, device):
  """Uninitialised device storage of the same layout as loader tensor `t` (padded or Ragged)."""
  if isinstance(t, ops.Ragged):
    return ops.Ragged(torch.empty(t.data.shape, dtype=torch.float32, device=device), t.lens)
  return torch.empty(t.shape, dtype=torch.float32, device=device)


def _lens_i64(x):
  """A batch's length member (host int64 tensor from the loader, list, or array) as int64 NumPy;
  the tensor case without the detour through `__array__` (616 of these per pass of the full split)."""
  if type(x) is torch.Tensor and x.dtype == torch.int64 and not x.is_cuda:
    return x.numpy()
  return np.asarray(x, dtype=np.int64)


def _dev_seq(t, device, dtype):
  """Loader tensor (padded or Ragged; host or device) -> contiguous `dtype` storage on `device`."""
  if type(t) is torch.Tensor and t.is_cuda and t.dtype == dtype and t.is_contiguous():
    return t          # already in place (616 of these per pass of the full split: keep it cheap)
  if isinstance(t, ops.Ragged):
    return ops.seq_keep(t if t.is_cuda else t.to(device, non_blocking=True), dtype)
  return ops.seq_keep(_to_dev(t, device), dtype)


def _plan_key(group):
  """What a cached plan of `group` is valid for: EVERY batch's four length arrays and clip /
  sentence counts (hashed in full) and the base addresses of its four feature / token tensors.  An
  in-place edit of any batch's lengths, a swapped or re-uploaded batch anywhere in the list, or a
  different number of batches gives a different key, and encode_group rebuilds the plan
  (tests/test_gpu_pipeline.py::test_plan_key_*).  What the key cannot see is an in-place edit of the
  VALUES.  Feature values are read afresh on every pass anyway (a plan holds addresses and schedules),
  with ONE exception since the prefix sharing (tunable share_prefix): the plan also keeps which first
  captions were token-for-token prefixes of their paragraphs when it was built, a fact derived from
  the token values.  Token ids edited in place under a kept plan would leave the edited captions'
  `cap_emb` rows pooled from their paragraphs: drop the plan (or clear the dict) after such an edit.
  A plan keeps its group's device tensors alive (`keep`): the whole resident
  split, 14.7 GB for ActivityNet-ICEP val; drop the plan dict to release them."""
  h = hashlib.blake2b(digest_size=16)
  ptrs = np.empty(4 * len(group), dtype=np.uint64)
  for i, b in enumerate(group):
    for k in (4, 5, 6, 7, 8, 9):
      v = b[k]
      a = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
      h.update(np.ascontiguousarray(a, dtype=np.int64).data)
      h.update(b'|')
    for k in range(4):
      ptrs[4 * i + k] = _base_ptr(b[k])
  h.update(ptrs.data)
  return (len(group), h.hexdigest())


def _base_ptr(t):
  return t.data.data_ptr() if isinstance(t, ops.Ragged) else t.data_ptr()


TOWERS = ('v1', 't1', 'v2', 't2')   # clips + whole videos | sentences + paragraphs | clips per video | sentences per paragraph


def length_histograms(batches):
  """{tower: np.bincount of the sequence lengths} of the four encoders over `batches` (12-tuples
  with their length members; a stub batch contributes nothing).  Histograms add over any partition
  of a split, which is how ranks that hold different batches agree on split_step_plan."""
  acc = {k: [] for k in TOWERS}
  for b in batches:
    if b[4] is None:
      continue
    acc['v1'] += [_lens_i64(b[4]), _lens_i64(b[6])]
    acc['t1'] += [_lens_i64(b[5]), _lens_i64(b[7])]
    acc['v2'].append(np.asarray(b[8], dtype=np.int64))
    acc['t2'].append(np.asarray(b[9] if b[9] is not None else b[8], dtype=np.int64))
  return {k: (np.bincount(np.concatenate(v)) if v else np.zeros(1, dtype=np.int64)).astype(np.int64)
          for k, v in acc.items()}


def plan_from_histograms(hists):
  """{tower: #{s : len_s > t} for t = 0 .. Tmax - 1} from length histograms."""
  return {k: (int(h.sum()) - np.cumsum(h)[:-1]).astype(np.int64) for k, h in hists.items()}


def split_step_plan(batches):
  """The step plan of a validation split: for each of the four encoders the number of sequences of
  the WHOLE split still active at time step t.  Handed to every encoder call that encodes a share
  of that split (one super-batch of several, one rank's batches: cmhse_seq_batch.step_plan_host), it
  pins which kernel serves each time step, so every sequence is encoded bit for bit as in a
  single call over the whole split — and the integer ranks do not depend on how the split was cut
  ("ranks must be identical for G in {1,2,4,8}")."""
  return plan_from_histograms(length_histograms(batches))


# Prefix sharing of the text tower (tunable "share_prefix", include/cmhse_hip.h).  A paragraph is the
# concatenation of its captions (activity_net/data.py:78) and both run through txt_enc from h0 = 0 in one
# request, so the hidden states and attention energies of a video's FIRST caption are those of its
# paragraph's first len(caption) steps, bit for bit.  Where the tokens say so (checked on the data of
# every call, text_prefix_flags) the caption is left out of the level-1 text request and its embedding is
# pooled from the paragraph's rows (cmhse_seq_batch.n_alias).  Attention pooling only: max and last
# pooling are fused into the step epilogue and would need a second epilogue target (a possible follow-up).
# Write-only for the library (tests and tools read it): the first captions the last encode_data_device
# call pooled from their paragraphs, of how many captions.  encode_group reports its own in its result.
SHARE_STATS = {'aliases': 0, 'captions': 0}

# What the token check of one group hands to encode_group: the flags and, for a group of resident padded
# batches, the level-1 text tables the check had to build anyway (captions then paragraphs), else None.
PrefixCheck = collections.namedtuple('PrefixCheck', 'flags t_lens t_ptrs num_caps')


def text_prefix_aliases(len_cap, len_par, num_caps, ok_flags=None):
  """The planner of the prefix sharing, pure NumPy.  len_cap [n_cap] caption lengths in loader order
  (video after video), len_par [n_vid] paragraph lengths, num_caps [n_vid] captions per video (>= 1),
  ok_flags [n_vid] (optional): nonzero where the first caption's tokens ARE the paragraph's first
  tokens.  Returns (kept, (vid, length, cap_row)): the caption indices that stay in the request, and per
  alias the video whose paragraph is the source, the caption's length and its row of cap_emb.  A video
  is aliased only if its flag is set and its paragraph is at least as long as its first caption; a
  single-caption video aliases its whole paragraph."""
  len_cap = np.asarray(len_cap, dtype=np.int64).reshape(-1)
  len_par = np.asarray(len_par, dtype=np.int64).reshape(-1)
  num_caps = np.asarray(num_caps, dtype=np.int64).reshape(-1)
  if len(num_caps) != len(len_par) or int(num_caps.sum()) != len(len_cap) or (num_caps < 1).any():
    raise ValueError('text_prefix_aliases: one paragraph and at least one caption per video')
  first = np.cumsum(num_caps) - num_caps
  l0 = len_cap[first]
  ok = len_par >= l0
  if ok_flags is not None:
    ok &= np.asarray(ok_flags).reshape(-1) != 0
  keep = np.ones(len(len_cap), dtype=bool)
  keep[first[ok]] = False
  vid = np.flatnonzero(ok)
  return np.flatnonzero(keep), (vid, l0[vid], first[vid])


def _share_on(model):
  """Does encode_group share first captions for this model under the current settings?"""
  rnn = model.txt_enc.rnn
  return (GROUP_TOWERS[0] and not TWO_STREAMS[0] and rnn.POOL == ops.POOL_ATTN and
          not getattr(rnn.rnn, 'bidirectional', False) and ops.tune('share_prefix') != 0)


def _resident_tokens(t, device):
  """A token tensor the encoders read in place (what _dev_seq hands back unchanged)."""
  d = t.data if isinstance(t, ops.Ragged) else t
  return (isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.int64 and d.is_contiguous() and
          d.device == device)


def _host_prefix_flags(caps, pars, first, l0, len_par):
  """text_prefix_flags for one batch whose token tensors are in host memory."""
  ok = len_par >= l0
  if isinstance(caps, ops.Ragged) or isinstance(pars, ops.Ragged) or caps.dim() != 2 or pars.dim() != 2:
    rows_c = (lambda i: caps.data[caps.first[i]:caps.first[i] + caps.lens[i]]) if isinstance(caps, ops.Ragged) \
        else (lambda i: caps[i])
    rows_p = (lambda i: pars.data[pars.first[i]:pars.first[i] + pars.lens[i]]) if isinstance(pars, ops.Ragged) \
        else (lambda i: pars[i])
    for v in np.flatnonzero(ok):
      n = int(l0[v])
      a, b = rows_c(int(first[v]))[:n], rows_p(int(v))[:n]
      ok[v] = a.shape[0] == n and b.shape[0] == n and bool(torch.equal(a.long(), b.long()))
    return ok
  a, b = caps.numpy()[first], pars.numpy()
  w = min(a.shape[1], b.shape[1])
  ok &= l0 <= w
  inside = np.arange(w, dtype=np.int64)[None, :] < l0[:, None]
  return ok & ((a[:, :w] == b[:, :w]) | ~inside).all(axis=1)


def text_prefix_flags(groups, device):
  """The flags of _prefix_checks alone."""
  return [c.flags for c in _prefix_checks(groups, device)]


def _prefix_checks(groups, device):
  """For every group (list of loader batches) a bool array [videos of the group]: True where the tokens
  of the video's first caption are the first tokens of its paragraph (raw ids).  Token tensors that
  are resident on `device` are compared there by one cmhse_tok_prefix_check launch over ALL groups and
  one read-back (the only host synchronisation of the sharing; it stands in front of every launch of
  the pass); token tensors in host memory are compared on the host.  Anything else: False.
  Returns one PrefixCheck per group; for a group of resident padded batches it carries the level-1 text
  tables (t_lens, t_ptrs, num_caps), which encode_group takes over instead of building them again."""
  out, parts, tables = [], [], []
  for gi, group in enumerate(groups):
    if all(type(b[1]) is torch.Tensor and type(b[3]) is torch.Tensor and _resident_tokens(b[1], device) and
           _resident_tokens(b[3], device) for b in group):
      # a resident split of padded batches (bench.py, a validation set kept in HBM): one pass of NumPy
      # over the whole group instead of a few small arrays per loader batch
      nc = np.fromiter(itertools.chain.from_iterable(b[9] for b in group), dtype=np.int64)
      first = np.cumsum(nc) - nc
      t_ptrs = ops.seq_row_ptrs_many([b[1] for b in group] + [b[3] for b in group])
      t_lens = np.concatenate([_lens_i64(b[5]) for b in group] + [_lens_i64(b[7]) for b in group])
      n_cap = len(t_lens) - len(nc)
      parts.append((gi, 0, t_ptrs[first], t_ptrs[n_cap:], t_lens[first], t_lens[n_cap:]))
      out.append(np.zeros(len(nc), dtype=bool))
      tables.append((t_lens, t_ptrs, nc))
      continue
    tables.append((None, None, None))
    flags = np.zeros(sum(len(b[9]) for b in group), dtype=bool)
    off = 0
    for b in group:
      nc = np.asarray(b[9], dtype=np.int64)
      first = np.cumsum(nc) - nc
      l0, lp = _lens_i64(b[5])[first], _lens_i64(b[7])
      caps, pars = b[1], b[3]
      if _resident_tokens(caps, device) and _resident_tokens(pars, device):
        parts.append((gi, off, ops.seq_row_ptrs(caps)[first], ops.seq_row_ptrs(pars), l0, lp))
      elif not caps.is_cuda and not pars.is_cuda:
        flags[off:off + len(nc)] = _host_prefix_flags(caps, pars, first, l0, lp)
      off += len(nc)
    out.append(flags)
  if parts:
    cols = [p[2:] for p in parts]
    cols = cols[0] if len(cols) == 1 else [np.concatenate([c[k] for c in cols]) for k in range(4)]
    host = ops.tok_prefix_check(*cols, device).cpu().numpy() != 0
    at = 0
    for gi, off, a, _, _, _ in parts:
      out[gi][off:off + len(a)] = host[at:at + len(a)]
      at += len(a)
  return [PrefixCheck(f, *t) for f, t in zip(out, tables)]


def _text_request(t_lens, t_ptrs, n_cap, num_caps, flags):
  """The level-1 text request of encode_group: all captions + paragraphs (t_lens, t_ptrs in that
  order), or — with `flags` (text_prefix_flags of the group) — the kept captions + paragraphs with
  every shared first caption as a prefix alias of its paragraph.  The step plan is that of the
  ORIGINAL sequences — the caller's split plan, else `own_plan`, the original sequences' own counts,
  which every request with aliases carries whether or not a split plan was given when it was built (a
  kept plan may be served later without one): which kernel serves step t is chosen from the active
  count of step t, and must not move because sequences left the request."""
  req = dict(lens=t_lens, ptrs=t_ptrs, out_rows=None, aliases=None, n_out=None, own_plan=None, n_alias=0)
  if flags is None:
    return req
  if len(t_lens) - n_cap != len(flags):
    raise ValueError('encode_group: one prefix flag per video of the group')
  kept, (vid, a_len, a_row) = text_prefix_aliases(t_lens[:n_cap], t_lens[n_cap:], num_caps, flags)
  if len(vid) == 0:
    return req
  sel = np.concatenate([kept, n_cap + np.arange(len(t_lens) - n_cap, dtype=np.int64)])
  req.update(lens=t_lens[sel], ptrs=t_ptrs[sel], out_rows=sel, aliases=(len(kept) + vid, a_len, a_row),
             n_out=len(t_lens), n_alias=len(vid), own_plan=ops.step_counts(t_lens))
  return req


def encode_group(model, group, contextual_model=True, device=None, plan=None, step_plan=None, stage=None,
                 share=None, plan_key=None):
  """Encode a list of loader batches (12-tuples) as ONE super-batch.  Returns a dict of device
  tensors: the six un-normalised embedding matrices plus their L2-normalised versions, rows in
  loader order.  Arithmetic per sequence is identical to per-batch encoding (sequences are
  independent), only the launch granularity differs.
  `plan`: a dict the caller keeps between passes over the SAME resident batches (a validation set
  held in HBM across epochs; bench.py): the level-1 schedules (sort, step counts, the uploaded
  pointer tables) are built on the first pass and reused afterwards — 2 ms of host work in front
  of the first launch, 5 % of a rank's 45 ms share of the split.
  `stage`: a HostStage (encode_data): the level-1 matrices of each tower are normalised on ITS copy
  stream and start for the host as soon as that tower's level-1 output is final — the visual
  tower's while the text tower's few-sequence tail still steps, the text tower's under level 2 —
  instead of after the whole pass (the values do not depend on it).
  `share`: the PrefixCheck of this group when the caller has it (encode_data_device checks all its
  groups in front of the first launch), False = encode every caption, None = decided and checked here;
  `plan_key`: _plan_key(group) when the caller has computed it.  The returned dict's 'n_alias' counts
  the first captions that were pooled from their paragraph's rows, 'n_cap' all captions."""
  device = device or torch.device('cuda', torch.cuda.current_device())
  sp = step_plan or {}
  share_on = share is not False and _share_on(model)
  if plan is not None:
    plan_key = plan_key or _plan_key(group)
    if (plan.get('key') == plan_key and plan.get('share') == share_on and GROUP_TOWERS[0] and
        not TWO_STREAMS[0]):
      return _encode_group_planned(model, group, contextual_model, device, plan, sp, stage)
  check = None
  if share_on:
    check = share if share is not None else _prefix_checks([group], device)[0]
  # (tables only with sharing on, i.e. in the grouped schedule below: the other schedules build their own)
  tables = check if check is not None and check.t_lens is not None else None
  clips_l, caps_l, vids_l, pars_l = [], [], [], []
  len_clip, len_cap, len_vid, len_par = [], [], [], []
  num_clips, num_caps = [], []
  # The loader hands over pinned HOST tensors (activity_net/data.py:157-162, pin_memory=True).  In
  # the grouped schedule their features are not copied up front: device buffers are only allocated
  # here, and the rows travel time-chunk by time-chunk on a copy stream while earlier GRU steps
  # already compute (ops.pull_steps; only valid steps cross PCIe, padding stays uninitialised and
  # is never read).
  pull = (PIPELINE_UPLOAD[0] and GROUP_TOWERS[0] and not TWO_STREAMS[0] and
          all(_pinned_f32(b[0]) and _pinned_f32(b[2]) for b in group))
  v_sched = v_events = None
  if pull:
    # features first: the copy stream starts pulling step 0 before anything else of this group is
    # queued (schedule metadata travels on the copy stream too; step 0's event orders it)
    for b in group:
      clips_l.append(_empty_like_on(b[0], device))
      vids_l.append(_empty_like_on(b[2], device))
    main, copy = torch.cuda.current_stream(device), _copy_stream(device)
    copy.wait_stream(main)         # the fresh device buffers may recycle blocks still in use
    with torch.cuda.stream(copy):
      v_sched = ops.SeqSchedule(
          np.concatenate([_lens_i64(b[4]) for b in group] + [_lens_i64(b[6]) for b in group]), device,
          x_ptrs=ops.seq_row_ptrs_many(clips_l + vids_l),
          src_ptrs=ops.seq_row_ptrs_many([b[0] for b in group] + [b[2] for b in group]))
      v_events = ops.pull_steps(v_sched, int(group[0][0].shape[2]), copy, UPLOAD_CHUNK[0])
      # the pull kernels read the pinned tensors by address, possibly after this function has
      # returned: they stay referenced here until an event behind the last chunk has completed (a
      # caller that drops its loader batches right away would otherwise hand the blocks back to
      # torch's pinned-memory allocator while they are still being read)
      _hold_host_rows(copy, [b[0] for b in group] + [b[2] for b in group])
    for t in clips_l + vids_l:
      t.record_stream(copy)        # allocated on the caller's stream, written on the copy stream
    v_sched.meta.record_stream(main)   # the other way round
  for b in group:
    if not pull:
      clips_l.append(_dev_seq(b[0], device, torch.float32))
      vids_l.append(_dev_seq(b[2], device, torch.float32))
    caps_l.append(_dev_seq(b[1], device, torch.int64))
    pars_l.append(_dev_seq(b[3], device, torch.int64))
    len_clip.append(_lens_i64(b[4]))
    len_vid.append(_lens_i64(b[6]))
    if tables is None:
      len_cap.append(_lens_i64(b[5]))
      len_par.append(_lens_i64(b[7]))
    num_clips.extend(b[8])
    num_caps.extend(b[9])
  n_clip = int(sum(len(l) for l in len_clip))
  n_vid = len(num_clips)
  n_cap = int(sum(len(l) for l in len_cap)) if tables is None else len(tables.t_lens) - n_vid
  if n_clip != sum(num_clips) or n_cap != sum(num_caps):
    raise ValueError('batch contract violated: sum(num_clips) != number of clip rows')

  clip_rnn, txt_rnn = model.clip_enc.rnn, model.txt_enc.rnn
  H1v = clip_rnn.rnn.weight_hh_l0.shape[1]
  H1t = txt_rnn.rnn.weight_hh_l0.shape[1]
  img_dim = clips_l[0].shape[2]
  table = model.txt_enc.embed.weight.detach()

  def level2(enc, rows, counts, ctx_rows, Hin, tower):
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    x_ptrs = np.uint64(rows.data_ptr()) + starts * np.uint64(Hin * 4)
    h0 = ops.padded_row_ptrs(ctx_rows) if contextual_model else None
    return enc.rnn.forward_ptrs(counts, Hin, device, x_ptrs=x_ptrs, h0_ptrs=h0, step_plan=sp.get(tower))

  n = ops.l2norm_rows
  n_alias = 0

  def visual_tower():
    # level 1: clips of all batches, then whole-video streams of all batches (same weights)
    ptrs = ops.seq_row_ptrs_many(clips_l + vids_l)
    lens = np.concatenate(len_clip + len_vid)
    vis = clip_rnn.forward_ptrs(lens, img_dim, device, x_ptrs=ptrs, step_plan=sp.get('v1'))
    clip_emb, vid_ctx = vis[:n_clip], vis[n_clip:]
    # level 2: each video's clips are consecutive rows of clip_emb -> addressed in place
    vid_emb = level2(model.vid_seq_enc, clip_emb, num_clips, vid_ctx, H1v, 'v2')
    return n(vid_emb), n(clip_emb), n(vid_ctx)

  def text_tower():
    # level 1: sentences, then paragraphs (embedding lookup fused into the operand load)
    ptrs = ops.seq_row_ptrs_many(caps_l + pars_l)
    lens = np.concatenate(len_cap + len_par)
    txt = txt_rnn.forward_ptrs(lens, table.shape[1], device, tok_ptrs=ptrs, table=table,
                               step_plan=sp.get('t1'))
    cap_emb, para_ctx = txt[:n_cap], txt[n_cap:]
    para_emb = level2(model.txt_seq_enc, cap_emb, num_caps, para_ctx, H1t, 't2')
    return n(para_emb), n(cap_emb), n(para_ctx)

  if TWO_STREAMS[0]:
    # The two towers are independent until the loss.  On two HIP streams the dispatcher can fill
    # the partial last round of one tower's step grid, and the CUs idle during the other's short
    # ragged-tail launches, with the other tower's workgroups.
    main = torch.cuda.current_stream(device)
    s_vis, s_txt = _side_streams(device)
    s_vis.wait_stream(main)
    s_txt.wait_stream(main)
    with torch.cuda.stream(s_txt):
      out_txt = text_tower()
    with torch.cuda.stream(s_vis):
      out_vis = visual_tower()
    main.wait_stream(s_vis)
    main.wait_stream(s_txt)
    for t in out_vis + out_txt:
      t.record_stream(main)      # allocated on a side stream, consumed on the caller's stream
  elif GROUP_TOWERS[0]:
    # The two towers are independent: step t of both level-1 encoders shares one launch
    # (cmhse_gru_pool_fwd_multi), then step t of both level-2 encoders.
    v_ptrs = ops.seq_row_ptrs_many(clips_l + vids_l)
    if tables is None:
      t_ptrs = ops.seq_row_ptrs_many(caps_l + pars_l)
      t_lens = np.concatenate(len_cap + len_par)
    else:       # (resident tokens: the tensors of caps_l / pars_l are the loader's own)
      t_ptrs, t_lens = tables.t_ptrs, tables.t_lens
    # The visual chain (<= 80 frames) ends long before the text chain (paragraphs of hundreds of
    # tokens, a handful of sequences per step by then): the text tail continues on a separate (own hardware queue; ops.stream_set)
    # side stream while the visual attention pass runs on this one, instead of after it.
    tail = _tail_stream(device) if EARLY_POOL[0] else None
    v_lens = np.concatenate(len_clip + len_vid)
    # (first captions that are a prefix of their paragraph leave the request: _text_request)
    tr = _text_request(t_lens, t_ptrs, n_cap, num_caps if tables is None else tables.num_caps,
                       None if check is None else check.flags)
    n_alias = tr['n_alias']
    t_sched = None
    if plan is not None and not pull:     # resident batches: the schedules outlive this pass
      v_sched = ops.SeqSchedule(v_lens, device, x_ptrs=v_ptrs)
      t_sched = ops.SeqSchedule(tr['lens'], device, tok_ptrs=tr['ptrs'], out_rows=tr['out_rows'],
                                aliases=tr['aliases'], n_out=tr['n_out'])
      plan.clear()
      plan.update(key=plan_key, share=share_on, v_sched=v_sched, t_sched=t_sched, v_lens=v_lens,
                  t_lens=tr['lens'], v_ptrs=v_ptrs, t_ptrs=tr['ptrs'], t_own_plan=tr['own_plan'],
                  n_alias=tr['n_alias'], img_dim=img_dim, n_clip=n_clip,
                  n_cap=n_cap, n_vid=n_vid, num_clips=np.asarray(num_clips, dtype=np.int64),
                  num_caps=np.asarray(num_caps, dtype=np.int64),
                  batch_sizes=[len(b[8]) for b in group], keep=(clips_l, vids_l, caps_l, pars_l))
    ready = None if stage is None else stage.tower_events()
    (vis, _), (txt, _) = ops.gru_pool_fwd_multi([
        clip_rnn.request_ptrs(v_lens, img_dim, device, x_ptrs=v_ptrs,
                              sched=v_sched, step_events=v_events, step_plan=sp.get('v1')),
        txt_rnn.request_ptrs(tr['lens'], table.shape[1], device,
                             tok_ptrs=tr['ptrs'], table=table, sched=t_sched,
                             step_plan=sp.get('t1') if sp.get('t1') is not None else tr['own_plan'],
                             out_rows=tr['out_rows'], aliases=tr['aliases'], n_out=tr['n_out'])],
        tail_stream=tail, ready_events=ready)
    clip_emb, vid_ctx = vis[:n_clip], vis[n_clip:]
    cap_emb, para_ctx = txt[:n_cap], txt[n_cap:]
    lvl1 = None if stage is None else stage.level1(ready, clip_emb, cap_emb, vid_ctx, para_ctx)

    def level2_request(enc, rows, counts, ctx_rows, Hin, tower):
      counts = np.asarray(counts, dtype=np.int64)
      starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
      x_ptrs = np.uint64(rows.data_ptr()) + starts * np.uint64(Hin * 4)
      h0 = ops.padded_row_ptrs(ctx_rows) if contextual_model else None
      return enc.rnn.request_ptrs(counts, Hin, device, x_ptrs=x_ptrs, h0_ptrs=h0,
                                  step_plan=sp.get(tower))

    (vid_emb, _), (para_emb, _) = ops.gru_pool_fwd_multi([
        level2_request(model.vid_seq_enc, clip_emb, num_clips, vid_ctx, H1v, 'v2'),
        level2_request(model.txt_seq_enc, cap_emb, num_caps, para_ctx, H1t, 't2')])
    if lvl1 is not None:
      out_vis = (n(vid_emb), lvl1['clip_emb'], lvl1['vid_ctx'])
      out_txt = (n(para_emb), lvl1['cap_emb'], lvl1['para_ctx'])
    else:
      out_vis = (n(vid_emb), n(clip_emb), n(vid_ctx))
      out_txt = (n(para_emb), n(cap_emb), n(para_ctx))
  else:
    out_vis = visual_tower()
    out_txt = text_tower()
  return dict(vid_emb=out_vis[0], para_emb=out_txt[0], clip_emb=out_vis[1], cap_emb=out_txt[1],
              vid_ctx=out_vis[2], para_ctx=out_txt[2], n_vid=n_vid,
              batch_sizes=[len(b[8]) for b in group], n_alias=n_alias, n_cap=n_cap)


def _encode_group_planned(model, group, contextual_model, device, plan, sp, stage=None):
  """encode_group's grouped schedule with the level-1 schedules of an earlier pass over the same
  batches (encode_group(plan=...)): same launches, same values."""
  clip_rnn, txt_rnn = model.clip_enc.rnn, model.txt_enc.rnn
  H1v = clip_rnn.rnn.weight_hh_l0.shape[1]
  H1t = txt_rnn.rnn.weight_hh_l0.shape[1]
  table = model.txt_enc.embed.weight.detach()
  n_clip, n_cap = plan['n_clip'], plan['n_cap']
  tail = _tail_stream(device) if EARLY_POOL[0] else None
  ready = None if stage is None else stage.tower_events()
  (vis, _), (txt, _) = ops.gru_pool_fwd_multi([
      clip_rnn.request_ptrs(plan['v_lens'], plan['img_dim'], device, x_ptrs=plan['v_ptrs'],
                            sched=plan['v_sched'], step_plan=sp.get('v1')),
      txt_rnn.request_ptrs(plan['t_lens'], table.shape[1], device, tok_ptrs=plan['t_ptrs'],
                           table=table, sched=plan['t_sched'],
                           step_plan=sp.get('t1') if sp.get('t1') is not None else plan['t_own_plan'])],
      tail_stream=tail, ready_events=ready)
  clip_emb, vid_ctx = vis[:n_clip], vis[n_clip:]
  cap_emb, para_ctx = txt[:n_cap], txt[n_cap:]
  lvl1 = None if stage is None else stage.level1(ready, clip_emb, cap_emb, vid_ctx, para_ctx)

  def level2_request(enc, rows, counts, ctx_rows, Hin, tower):
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    x_ptrs = np.uint64(rows.data_ptr()) + starts * np.uint64(Hin * 4)
    h0 = ops.padded_row_ptrs(ctx_rows) if contextual_model else None
    return enc.rnn.request_ptrs(counts, Hin, device, x_ptrs=x_ptrs, h0_ptrs=h0,
                                step_plan=sp.get(tower))

  (vid_emb, _), (para_emb, _) = ops.gru_pool_fwd_multi([
      level2_request(model.vid_seq_enc, clip_emb, plan['num_clips'], vid_ctx, H1v, 'v2'),
      level2_request(model.txt_seq_enc, cap_emb, plan['num_caps'], para_ctx, H1t, 't2')])
  n = ops.l2norm_rows
  if lvl1 is None:
    lvl1 = dict(clip_emb=n(clip_emb), cap_emb=n(cap_emb), vid_ctx=n(vid_ctx), para_ctx=n(para_ctx))
  return dict(vid_emb=n(vid_emb), para_emb=n(para_emb), n_vid=plan['n_vid'],
              batch_sizes=plan['batch_sizes'], n_alias=plan['n_alias'], n_cap=n_cap, **lvl1)


@contextlib.contextmanager
def _no_gc_pause():
  """No cyclic garbage collection while a pass's launches are being queued: the GPU has nothing
  to do until the first of them arrives, and a full collection over a training process's objects
  was measured at 70-90 ms in that spot (tools/pass_jitter.py; a pass is 281).  The collector is
  switched back on right after (the pass allocates a few thousand short-lived objects)."""
  was = gc.isenabled()
  gc.disable()
  try:
    yield
  finally:
    if was:
      gc.enable()


def _group_batches(batches, max_bytes):
  """Split the loader's batches into super-batches of at most `max_bytes` of padded features."""
  groups, cur, cur_bytes = [], [], 0
  for b in batches:
    nbytes = b[0].numel() * 4 + b[2].numel() * 4
    if cur and cur_bytes + nbytes > max_bytes:
      groups.append(cur)
      cur, cur_bytes = [], 0
    cur.append(b)
    cur_bytes += nbytes
  if cur:
    groups.append(cur)
  return groups


def encode_data_device(opt, model, data_loader, log_step=10, logging=print, contextual_model=True,
                       superbatch_bytes=48 << 30, defer_logging=False, plan=None, step_plan=None,
                       stage=None):
  """Device-resident core of encode_data: returns (dict of six [N,*] normalised embedding tensors
  on the GPU, num_clips_total, cur_vid_total).  With `defer_logging` the per-batch 'Letest' values
  travel to the host asynchronously and a fourth return value, `finish()`, replays the logger
  updates: a caller that scores the embeddings right away (bench.py, parallel_eval) queues its
  ranking kernels first and calls finish() afterwards, so the GPU does not idle through that
  device-to-host round trip.  `plan`: a dict kept by a caller that encodes the SAME resident
  batches again and again (encode_group): schedules built once.  `step_plan`: split_step_plan() of
  the whole split when `data_loader` is only a share of it (parallel_eval passes the one all ranks
  agree on); by default the plan of `data_loader` itself, so that cutting it into several
  super-batches (`superbatch_bytes`) does not change a bit of any embedding.  `stage`: a HostStage
  that receives every group's six matrices as soon as they are queued (encode_data)."""
  batch_time = AverageMeter()
  val_logger = LogCollector()
  model.val_start(opt)
  end = time.time()
  outs = {k: [] for k in ['vid_emb', 'para_emb', 'clip_emb', 'cap_emb', 'vid_ctx', 'para_ctx']}
  num_clips_total, cur_vid_total = [], []
  batches = list(data_loader)
  n_loader = len(batches)
  pending, state = [], {'i': 0, 'end': end}

  def flush():
    """Replay model.logger.update('Letest', value, batch size) (model.py:291) for the groups whose
    loss values have reached the host, batch by batch in loader order."""
    while pending:
      group, sizes, host, ev, block = pending.pop(0)
      if ev is not None:
        ev.synchronize()
      values = host.tolist()
      if ev is not None:
        _HOST_SCALARS.append(block)    # read: the pinned block may carry the next group's values
        _HOST_EVENTS.append(ev)        # ... and its event the next group's copy
      for b, bs, lv in zip(group, sizes, values):
        val_logger.update('Letest', lv, bs)
        batch_time.update(time.time() - state['end'])
        state['end'] = time.time()
        if state['i'] % log_step == 0:
          logging('Test: [{0}/{1}]\t{e_log}\tTime {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                  .format(state['i'], n_loader, batch_time=batch_time, e_log=str(val_logger)))
        state['i'] += 1

  with torch.no_grad(), _no_gc_pause():
    groups = _group_batches(batches, superbatch_bytes)
    if step_plan is None and len(groups) > 1:       # (one group: its own step counts ARE the split's)
      step_plan = split_step_plan(batches)
    # Prefix sharing: the token check of ALL groups in front of the first launch (one read-back while
    # the GPU has nothing queued; a read-back in a later group would stall a host that runs a group
    # ahead).  A group whose cached plan is still valid was checked when that plan was built.
    keys = [None if plan is None else _plan_key(g) for g in groups]
    share = [False] * len(groups)
    if _share_on(model):
      share = [None] * len(groups)     # (None: served from the group's valid plan)
      todo = [gi for gi in range(len(groups))
              if plan is None or not (plan.get(gi, {}).get('key') == keys[gi] and plan[gi].get('share'))]
      device = torch.device('cuda', torch.cuda.current_device())
      for gi, check in zip(todo, _prefix_checks([groups[gi] for gi in todo], device)):
        share[gi] = check
    n_alias = n_caps = 0
    for gi, group in enumerate(groups):
      model.logger = val_logger                     # evaluation.py:99
      enc = encode_group(model, group, contextual_model,
                         plan=None if plan is None else plan.setdefault(gi, {}), step_plan=step_plan,
                         stage=stage, share=share[gi], plan_key=keys[gi])
      n_alias += enc['n_alias']
      n_caps += enc['n_cap']
      if stage is not None:
        stage.put({k: enc[k] for k in outs})     # (what left early is skipped)
      for k in outs:
        outs[k].append(enc[k])
      # per-loader-batch 'Letest' loss (evaluation.py:129), all on device, one sync per group
      crit = model.criterion
      loss_dev = ops.contrastive_blocks_fwd(enc['vid_emb'], enc['para_emb'], enc['batch_sizes'],
                                            crit.margin, crit.max_violation, crit.norm)
      for b in group:
        num_clips_total.extend(b[8])
        cur_vid_total.extend(b[11])
      if defer_logging:
        block = _host_scalars(loss_dev.numel())
        host = block[:loss_dev.numel()]
        host.copy_(loss_dev.reshape(-1), non_blocking=True)   # (stream-ordered after the loss kernels)
        ev = _HOST_EVENTS.pop() if _HOST_EVENTS else torch.cuda.Event()
        ev.record()
        pending.append((group, enc['batch_sizes'], host, ev, block))
      else:
        pending.append((group, enc['batch_sizes'], loss_dev.cpu(), None, None))
        flush()
  cat = {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in outs.items()}
  SHARE_STATS.update(aliases=n_alias, captions=n_caps)      # of the whole call
  if defer_logging:
    return cat, num_clips_total, cur_vid_total, flush
  return cat, num_clips_total, cur_vid_total


MATRICES = ('vid_emb', 'para_emb', 'clip_emb', 'cap_emb', 'vid_ctx', 'para_ctx')
PUSH_KERNEL = [True]     # device-to-host staging by cmhse_push_rows (a few waves) instead of hipMemcpyAsync


_STAGE_EVENTS = []


class HostStage(object):
  """The device-to-host side of encode_data: six page-locked float32 matrices (what the reference
  builds row by row with `.data.cpu()` + list.extend, evaluation.py:120-125,139-144) filled by
  asynchronous copies on the package's copy stream while the encoders and the ranking still run.
  `put(mats)` is called with the CURRENT stream having queued the producers of `mats`; a matrix a
  group has already handed over (the level-1 rows, early) is skipped the second time.  The pinned
  blocks come from torch's caching host allocator: the arrays encode_data returns view them, and
  they go back to the cache when the caller drops those arrays."""

  def __init__(self, rows, dims, device):
    self.device = device
    self.host = {k: torch.empty((rows[k], dims[k]), dtype=torch.float32, pin_memory=True)
                 for k in MATRICES}
    self.filled = {k: 0 for k in MATRICES}
    self.seen = set()
    self.copy = _copy_stream(device)
    self._keep = []      # the staged device tensors: their ids stay unique until wait()
    self._events = _STAGE_EVENTS     # recycled between groups and passes (creating an event beside a
                                     # busy GPU was seen to stall the host for milliseconds, ops.upload)

  def tower_events(self):
    """Two events (visual, text) for gru_pool_fwd_multi(ready_events=): recorded once here so that
    they own a handle; the library re-records each where its tower's level-1 output is final."""
    main = torch.cuda.current_stream(self.device)
    evs = []
    for _ in range(2):
      ev = self._events.pop() if self._events else torch.cuda.Event()
      ev.record(main)
      evs.append(ev)
    return evs

  def level1(self, ready, clip_emb, cap_emb, vid_ctx, para_ctx):
    """Normalise the four level-1 matrices on the copy stream, each tower behind ITS ready event,
    and send them off; returns them ({name: normalised device tensor}).  The caller's stream is
    made to wait for the normalisations (not for the copies) before it returns."""
    main = torch.cuda.current_stream(self.device)
    out = {}
    normed = self._events.pop() if self._events else torch.cuda.Event()
    towers = ((ready[0], (('clip_emb', clip_emb), ('vid_ctx', vid_ctx))),
              (ready[1], (('cap_emb', cap_emb), ('para_ctx', para_ctx))))
    for i, (ev, pair) in enumerate(towers):
      self.copy.wait_event(ev)
      with torch.cuda.stream(self.copy):
        for k, raw in pair:
          raw.record_stream(self.copy)
          out[k] = ops.l2norm_rows(raw)
      if i == len(towers) - 1:
        normed.record(self.copy)      # (behind the first tower's copies, in front of the last one's)
      self._send([(k, out[k]) for k, _ in pair])
    main.wait_event(normed)           # consumers of the returned tensors on the caller's stream
    for t in out.values():
      t.record_stream(main)
    self._events += list(ready) + [normed]
    return out

  def put(self, mats):
    todo = [(k, t) for k, t in mats.items() if k in self.host and id(t) not in self.seen]
    if not todo:
      return
    self.copy.wait_stream(torch.cuda.current_stream(self.device))
    self._send(todo, ops.PUSH_WORKGROUPS_LATE[0])

  def _send(self, todo, workgroups=None):
    for k, t in todo:
      n = t.shape[0]
      dst = self.host[k][self.filled[k]:self.filled[k] + n]
      if PUSH_KERNEL[0]:
        tc = t.contiguous()
        self._keep.append(tc)
        ops.push_rows(tc, dst, self.copy, workgroups)
      else:             # the runtime's copy: a chip-wide blit kernel on this image (A/B only)
        with torch.cuda.stream(self.copy):
          dst.copy_(t, non_blocking=True)
      t.record_stream(self.copy)
      self.filled[k] += n
      self.seen.add(id(t))
    self._keep += [t for _, t in todo]

  def wait(self):
    """Block until every queued copy has landed; returns {name: pinned tensor}."""
    for k in MATRICES:
      if self.filled[k] != self.host[k].shape[0]:
        raise RuntimeError('encode_data: %s received %d of %d rows' % (k, self.filled[k], self.host[k].shape[0]))
    self.copy.synchronize()
    self._keep = []
    return self.host


def _stage_for(model, batches, device):
  """A HostStage sized for `batches` (12-tuples with their count members) and `model`'s widths."""
  n_vid = sum(len(b[8]) for b in batches)
  n_clip = sum(int(sum(b[8])) for b in batches)
  n_cap = sum(int(sum(b[9] if b[9] is not None else b[8])) for b in batches)
  h = lambda enc: int(enc.rnn.rnn.weight_hh_l0.shape[1])
  rows = dict(vid_emb=n_vid, para_emb=n_vid, clip_emb=n_clip, cap_emb=n_cap, vid_ctx=n_vid, para_ctx=n_vid)
  dims = dict(vid_emb=h(model.vid_seq_enc), para_emb=h(model.txt_seq_enc), clip_emb=h(model.clip_enc),
              cap_emb=h(model.txt_enc), vid_ctx=h(model.clip_enc), para_ctx=h(model.txt_enc))
  return HostStage(rows, dims, device)


# What the last encode_data left on the device for the i2t / t2i calls that follow it in
# train.validate (train.py:225-236): the two [N, D] matrices themselves and — queued speculatively
# behind the encoders, under the tail of the device-to-host copies — the ranks of both directions.
# i2t / t2i serve a call from it only when they are handed the very ndarray OBJECTS encode_data
# returned AND the bytes those arrays hold now still equal the device copies (the arrays view pinned
# memory: cmhse_rows_differ reads them in place over PCIe, 0.7 ms for the two 20 MB matrices).  One
# entry, replaced by the next encode_data, dropped when either array is garbage-collected.
TRACE = None           # tools/api_path_profile.py: a list that receives (phase, perf_counter) marks
SPECULATE_RANKS = [True]
SUPERBATCH_BYTES = [48 << 30]    # padded feature bytes per super-batch of encode_data (288 GB of HBM)
_LAST_ENCODE = [None]
CACHE_STATS = {'hits': 0, 'stale': 0}


def _forget_last_encode(_ref=None):
  _LAST_ENCODE[0] = None


def _mark(name):
  if TRACE is not None:
    TRACE.append((name, time.perf_counter()))


def encode_data(opt, model, data_loader, log_step=10, logging=print, contextual_model=True):
  """/root/reference/evaluation.py:80-158: returns (vid_embs, para_embs, clip_embs, cap_embs,
  vid_contexts, para_contexts, num_clips_total, cur_vid_total); the six arrays are float32 NumPy
  like the reference's.  They leave the device through page-locked memory on the copy stream: the
  level-1 matrices (clips, sentences, contexts: 4/5 of the bytes) while level 2 runs, the two
  level-2 matrices under the ranking of both directions, which is queued here already
  (SPECULATE_RANKS) for the i2t / t2i calls train.validate makes next."""
  import weakref
  batches = list(data_loader)
  device = torch.device('cuda', torch.cuda.current_device())
  stage = _stage_for(model, batches, device)
  _mark('pinned matrices allocated')
  cat, num_clips_total, cur_vid_total, finish_log = encode_data_device(
      opt, model, batches, log_step, logging, contextual_model, superbatch_bytes=SUPERBATCH_BYTES[0],
      defer_logging=True, stage=stage)
  _mark('encoders queued')
  ranks_host = ranks_event = None
  if SPECULATE_RANKS[0] and cat['vid_emb'].shape == cat['para_emb'].shape:
    r_i, t_i = ops.sim_rank(cat['vid_emb'], cat['para_emb'])
    r_t, t_t = ops.sim_rank(cat['para_emb'], cat['vid_emb'])
    ranks_host = torch.empty((4, r_i.shape[0]), dtype=torch.int32, pin_memory=True)
    ranks_host.copy_(torch.stack([r_i, t_i, r_t, t_t]), non_blocking=True)
    ranks_event = _HOST_EVENTS.pop() if _HOST_EVENTS else torch.cuda.Event()
    ranks_event.record()
  _mark('ranking queued')
  finish_log()          # the per-batch 'Letest' meters (evaluation.py:129), behind everything queued
  _mark('Letest values on the host (encoders done)')
  host = stage.wait()
  _mark('six matrices on the host')
  arrays = {k: host[k].numpy() for k in MATRICES}
  if ranks_event is not None:
    ranks_event.synchronize()
    _HOST_EVENTS.append(ranks_event)
    _mark('ranks on the host')
    _LAST_ENCODE[0] = dict(
        vid=weakref.ref(arrays['vid_emb'], _forget_last_encode),
        para=weakref.ref(arrays['para_emb'], _forget_last_encode),
        vid_host=host['vid_emb'], para_host=host['para_emb'],
        vid_dev=cat['vid_emb'], para_dev=cat['para_emb'], ranks=ranks_host.numpy())
  else:
    _LAST_ENCODE[0] = None
  return tuple(arrays[k] for k in MATRICES) + (num_clips_total, cur_vid_total)


# ---------------------------------------------------------------------------------------------
# i2t / t2i
# ---------------------------------------------------------------------------------------------
def report_from_ranks(ranks):
  """The six numbers of evaluation.py:173-184 from the 0-based ranks of the matching item:
  recall at 1 / 5 / 50 in percent (the key 'r10' IS Recall@50 upstream: `ranks < 50`, :175),
  median and mean rank 1-based, and the recall sum train.py uses as its model-selection score."""
  ranks = numpy.asarray(ranks)
  recall = {key: 100.0 * numpy.count_nonzero(ranks < k) / len(ranks)
            for key, k in (('r1', 1), ('r5', 5), ('r10', 50))}
  recall['medr'] = numpy.floor(numpy.median(ranks)) + 1
  recall['meanr'] = ranks.mean() + 1
  recall['sum'] = recall['r1'] + recall['r5'] + recall['r10']
  return recall


def _as_device(x, device=None):
  if isinstance(x, torch.Tensor):
    return x if x.is_cuda else x.cuda()
  if not torch.cuda.is_available():
    raise RuntimeError('cmhse_amd.evaluation needs an MI355X (no CPU fallback)')
  t = torch.from_numpy(numpy.ascontiguousarray(x, dtype=numpy.float32))
  # an array that views page-locked memory (encode_data's own) goes up without the pageable stop-over
  return t.to(device or 'cuda', non_blocking=t.is_pinned())


def _from_last_encode(images, captions):
  """The ranks [4, N] int32 the last encode_data queued, when `images` / `captions` are the arrays
  that call returned and still hold what it wrote; else None."""
  e = _LAST_ENCODE[0]
  if e is None or e['vid']() is not images or e['para']() is not captions:
    return None
  _mark('content check queued')
  # the arrays view page-locked memory: the device compares them in place with its own copies (one pass
  # over PCIe, nothing staged)
  differ = ops.rows_differ([(e['vid_host'], e['vid_dev']), (e['para_host'], e['para_dev'])])
  _mark('content check done')
  if not differ:
    CACHE_STATS['hits'] += 1
    return e['ranks']
  CACHE_STATS['stale'] += 1
  _LAST_ENCODE[0] = None         # edited in place since: never again served from here
  return None


def retrieve(queries, gallery, k=10, exact=False):
  """Top-k retrieval: for every query row, the k gallery rows with the largest dot product
  (cosine similarity on encode_data's normalised embeddings), best first, smaller gallery index
  first on exact ties (ops.sim_topk: matrix-free, exact fp32).

    vid, para, *_ = encode_data(opt, model, loader)
    scores, index = retrieve(para, vid, k)   # the k best videos for each paragraph
    scores, index = retrieve(vid, para, k)   # the k best paragraphs for each video

  NumPy in (encode_data's arrays, pinned views included), NumPy out: scores float32 [n, k] and
  index int64 [n, k].  GPU tensors in: device tensors out (float32, int32), on the current
  stream.  The ranking cache i2t / t2i serve from is neither read nor changed.

  exact=True: the list of the FLOAT64 scores of the same embeddings, certified (ops.sim_topk_exact):
  its order and its membership at the k-th place depend on neither summation order, tile shape nor
  machine, where the fp32 list can differ on most rows of a nearly tied gallery.  scores are float64;
  the rest as above."""
  if exact not in (False, True):
    raise ValueError('exact must be False or True, got %r' % (exact,))
  topk = (lambda q, g: ops.sim_topk_exact(q, g, k)[:2]) if exact else (lambda q, g: ops.sim_topk(q, g, k))
  if isinstance(queries, torch.Tensor) and queries.is_cuda:
    return tuple(topk(queries, _as_device(gallery, queries.device)))
  q = _as_device(queries)
  scores, index = topk(q, _as_device(gallery, q.device))
  return scores.cpu().numpy(), index.cpu().numpy().astype(numpy.int64)


def group_i2t_t2i(clip_embs, cap_embs, num_clips, num_caps=None, reduce='max'):
  """Video <-> paragraph ranking by the group-wise score of the low level (the score
  GroupWiseContrastiveLoss trains on: block max of the clip x caption scores of a (video, paragraph)
  pair with max_violation, block mean without), from encode_data's clip and caption rows and
  num_clips_total:

    vid, para, clip, cap, _, _, nclips, _ = encode_data(opt, model, loader)
    (r_v2p, top1_v2p, ranks_v2p), (r_p2v, top1_p2v, ranks_p2v) = group_i2t_t2i(
        clip, cap, nclips, reduce='max' if opt.max_violation else 'mean')

  Returns ((report, top1, ranks) video -> paragraph, the same paragraph -> video), each in the format
  of i2t / t2i (report_from_ranks; top1 and ranks float64 NumPy), with one device-to-host copy.
  num_caps defaults to num_clips.  GPU tensors in: top1 and ranks stay int32 device tensors (the
  reports still come from one host copy).  The ranking cache i2t / t2i serve from is neither read nor
  changed."""
  on_device = isinstance(clip_embs, torch.Tensor) and clip_embs.is_cuda
  if reduce not in ('max', 'mean'):
    raise ValueError("reduce must be 'max' or 'mean', got %r" % (reduce,))
  ops.group_plan(num_clips, num_caps, len(clip_embs), len(cap_embs))   # argument errors before the upload
  c = _as_device(clip_embs)
  s = _as_device(cap_embs, c.device)
  r_v, t_v, r_p, t_p = ops.group_rank(c, s, num_clips, num_caps, reduce)
  host = torch.stack([r_v, t_v, r_p, t_p]).cpu().numpy().astype(numpy.float64)
  if on_device:
    return ((report_from_ranks(host[0]), t_v, r_v), (report_from_ranks(host[2]), t_p, r_p))
  return ((report_from_ranks(host[0]), host[1], host[0]),
          (report_from_ranks(host[2]), host[3], host[2]))


def group_i2t_t2i_exact(clip_embs, cap_embs, num_clips, num_caps=None, reduce='max', ties='optimistic',
                        top1='fp32'):
  """group_i2t_t2i on the ranks of the FLOAT64 block scores, certified (ops.group_rank_exact): independent of
  summation order, tile shape and machine, where the fp32 group ranks differ from a float64 ranking of the
  same rows wherever captions are shared or clips nearly repeat.  Returns ((report, top1, ranks) video ->
  paragraph, the same paragraph -> video, info), the first two in group_i2t_t2i's format; `ranks` is rank_lo
  for ties='optimistic' (a group that ties the query's own exactly is not counted: group_i2t_t2i's rule) and
  rank_hi for ties='pessimistic' (it is: a model that collapses the low level reports the last rank, not the
  first).  info = {'v2p': d, 'p2v': d, 'resolved': total}, each d with 'report_lo', 'report_hi', 'tied_rows'
  (the queries with rank_lo < rank_hi) and 'resolved' (the blocks that went through float64).  top1='fp32'
  (the default): top1 is group_i2t_t2i's, not certified; top1='exact': the arg-max of the float64 block
  scores, the smaller index on a float64 tie, from a certified k = 1 retrieval (ops.group_topk_exact) per
  direction, whose float64 blocks are counted in info['v2p' / 'p2v']['top1_resolved'] and, summed, in
  info['top1_resolved'].  NumPy in: NumPy out (float64) with one device-to-host copy; GPU tensors in:
  top1 and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is neither read nor
  changed."""
  _check_exact_options(ties, top1)
  if reduce not in ('max', 'mean'):
    raise ValueError("reduce must be 'max' or 'mean', got %r" % (reduce,))
  on_device = isinstance(clip_embs, torch.Tensor) and clip_embs.is_cuda
  ops.group_plan(num_clips, num_caps, len(clip_embs), len(cap_embs))   # argument errors before the upload
  c = _as_device(clip_embs)
  s = _as_device(cap_embs, c.device)
  out = ops.group_rank_exact(c, s, num_clips, num_caps, reduce)
  tail = []
  if top1 == 'exact':
    ncaps = num_clips if num_caps is None else num_caps
    _, top_v, res_v = ops.group_topk_exact(c, s, num_clips, ncaps, 1, 'v2p', reduce)
    _, top_p, res_p = ops.group_topk_exact(c, s, num_clips, ncaps, 1, 'p2v', reduce)
    out = out[:2] + (top_v.reshape(-1),) + out[3:6] + (top_p.reshape(-1),) + out[7:]
    tail = [res_v, res_p]        # (per-query counts: summed on the host)
  host = torch.stack(list(out) + tail).cpu().numpy().astype(numpy.float64)
  pick = 0 if ties == 'optimistic' else 1
  info, sides = {}, []
  for name, h, dev in (('v2p', host[:4], out[:4]), ('p2v', host[4:8], out[4:8])):
    info[name] = _exact_side_info(h)
    report = info[name]['report_lo' if pick == 0 else 'report_hi']
    sides.append((report, dev[2], dev[pick]) if on_device else (report, h[2], h[pick]))
  info['resolved'] = info['v2p']['resolved'] + info['p2v']['resolved']
  if top1 == 'exact':
    info['v2p']['top1_resolved'], info['p2v']['top1_resolved'] = int(host[8].sum()), int(host[9].sum())
    info['top1_resolved'] = info['v2p']['top1_resolved'] + info['p2v']['top1_resolved']
  return sides[0], sides[1], info


def group_retrieve(clip_embs, cap_embs, num_clips, num_caps=None, k=10, direction='p2v', reduce='max',
                   exact=False):
  """Top-k retrieval by the group-wise score of the low level (group_i2t_t2i's score: block max of
  the clip x caption scores of a (video, paragraph) pair with max_violation, block mean without):
  direction 'p2v' gives the k best videos for every paragraph, 'v2p' the k best paragraphs for every
  video, best first, smaller index first on exact ties (ops.group_topk: matrix-free, exact fp32).
  The video set (clip rows, num_clips) and the paragraph set (caption rows, num_caps) may differ in
  size — a new set of query paragraphs against a video gallery:

    vid, para, clip, cap, _, _, nclips, _ = encode_data(opt, model, loader)
    scores, index = group_retrieve(clip, cap, nclips, k=10, direction='p2v',
                                   reduce='max' if opt.max_violation else 'mean')

  NumPy in, NumPy out: scores float32 [Bq, k] and index int64 [Bq, k].  GPU tensors in: device
  tensors out (float32, int32), on the current stream.  num_caps defaults to num_clips.  The ranking
  cache i2t / t2i serve from is neither read nor changed.

  exact=True: the list of the FLOAT64 block scores of the same rows, certified (ops.group_topk_exact; the
  block score of group_i2t_t2i_exact): its order and its membership at the k-th place depend on neither
  summation order, tile shape nor machine, where the fp32 list differs on nearly every query once captions
  are shared or clips nearly repeat.  scores are float64; the rest as above."""
  if not isinstance(exact, (bool, numpy.bool_)):
    raise ValueError('exact must be False or True, got %r' % (exact,))
  num_caps = num_clips if num_caps is None else num_caps
  if reduce not in ('max', 'mean'):
    raise ValueError("reduce must be 'max' or 'mean', got %r" % (reduce,))
  for x, name in ((clip_embs, 'clip_embs'), (cap_embs, 'cap_embs')):
    if len(getattr(x, 'shape', ())) != 2:
      raise ValueError('%s must be 2-D' % name)
  if clip_embs.shape[1] != cap_embs.shape[1]:
    raise ValueError('embedding widths differ')
  # argument errors before the upload
  ops.group_topk_plan(num_clips, num_caps, len(clip_embs), len(cap_embs), k, direction)
  on_device = isinstance(clip_embs, torch.Tensor) and clip_embs.is_cuda
  c = _as_device(clip_embs)
  s = _as_device(cap_embs, c.device)
  if exact:
    scores, index, _ = ops.group_topk_exact(c, s, num_clips, num_caps, k, direction, reduce)
  else:
    scores, index = ops.group_topk(c, s, num_clips, num_caps, k, direction, reduce)
  if on_device:
    return scores, index
  return scores.cpu().numpy(), index.cpu().numpy().astype(numpy.int64)


def pairs_from_ids(image_ids, caption_ids):
  """The (image row, caption row) pairs whose ids are equal, int64 [P, 2], sorted by image row, then
  caption row: the `pairs` of i2t_t2i_labelled from two id lists (encode_data's eighth return value
  is the id list of its rows).  A caption whose id no image carries gives no pair.  No GPU."""
  rows = {}
  for c, key in enumerate(caption_ids):
    rows.setdefault(key, []).append(c)
  pairs = [(i, c) for i, key in enumerate(image_ids) for c in rows.get(key, ())]
  return numpy.asarray(pairs, dtype=numpy.int64).reshape(-1, 2)


def csr_from_pairs(pairs, n_images, n_captions):
  """Both label sets of i2t_t2i_labelled from `pairs`, an integer [P, 2] array of (image row, caption
  row): ((offsets, indices) image -> its captions, (offsets, indices) caption -> its images), each
  list ascending.  ValueError for a row outside its matrix and for a row of either side that appears
  in no pair (it would have nothing to be ranked against), naming it.  No GPU."""
  pairs = numpy.asarray(pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
  if pairs.ndim != 2 or pairs.shape[1] != 2 or not (pairs.size == 0 or numpy.issubdtype(pairs.dtype, numpy.integer)):
    raise ValueError('pairs must be an integer [P, 2] array of (image row, caption row), got %s %r'
                     % (pairs.dtype, pairs.shape))
  pairs = pairs.astype(numpy.int64)
  out = []
  for side, other, n, n_other, name, other_name in ((0, 1, n_images, n_captions, 'image', 'caption'),
                                                    (1, 0, n_captions, n_images, 'caption', 'image')):
    key, val = pairs[:, side], pairs[:, other]
    bad = (key < 0) | (key >= n)
    if bad.any():
      raise ValueError('pair %d: %s row %d outside [0, %d)' % (int(numpy.flatnonzero(bad)[0]), name,
                                                               int(key[bad][0]), n))
    counts = numpy.bincount(key, minlength=n)
    if (counts == 0).any():
      raise ValueError('%s row %d appears in no pair: it has no correct %s to be ranked against'
                       % (name, int(numpy.flatnonzero(counts == 0)[0]), other_name))
    off = numpy.zeros(n + 1, dtype=numpy.int64)
    numpy.cumsum(counts, out=off[1:])
    out.append((off, val[numpy.lexsort((val, key))]))
  return out[0], out[1]


def rank_labelled(queries, gallery, positives):
  """i2t's report for any gallery and any set of correct answers per query: `positives` gives, for
  every query row, the gallery rows that count as correct (a 1-D target index per query, a CSR tuple
  (offsets, indices) or a list of per-query index lists: ops.positives_csr), and the rank of a query
  is the rank of its best-placed positive (ops.sim_rank_labelled: matrix-free, exact fp32).
  Returns (report, top1, ranks) in i2t's format (report_from_ranks; float64 NumPy).  GPU tensors in:
  top1 and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is neither read
  nor changed."""
  on_device = isinstance(queries, torch.Tensor) and queries.is_cuda
  csr = ops.positives_csr(positives, len(queries), len(gallery))   # argument errors before the upload
  q = _as_device(queries)
  rank, top1, _ = ops.sim_rank_labelled(q, _as_device(gallery, q.device), csr)
  host = torch.stack([rank, top1]).cpu().numpy().astype(numpy.float64)
  if on_device:
    return report_from_ranks(host[0]), top1, rank
  return report_from_ranks(host[0]), host[1], host[0]


def i2t_t2i_labelled(images, captions, pairs):
  """i2t_t2i for matrices whose correct answers are given by `pairs`, an integer [P, 2] array of
  (image row, caption row) — any number of rows on either side, any number of correct partners per
  row, at least one (pairs_from_ids builds it from two id lists).  Two annotation sets scored against
  one video set:

    vid, para1, *_, ids1 = encode_data(opt, model, val_1_loader)
    _,   para2, *_, ids2 = encode_data(opt, model, val_2_loader)
    paras = numpy.concatenate([para1, para2])
    (r_v2p, _, _), (r_p2v, _, _) = i2t_t2i_labelled(vid, paras, pairs_from_ids(ids1, ids1 + ids2))

  Returns ((report, top1, ranks) image -> caption, the same caption -> image), each in i2t's format,
  with one device-to-host copy; with pairs (i, i) exactly what i2t_t2i returns.  GPU tensors in: top1
  and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is neither read nor
  changed."""
  on_device = isinstance(images, torch.Tensor) and images.is_cuda
  csr_i, csr_t = csr_from_pairs(pairs, len(images), len(captions))   # argument errors before the upload
  v = _as_device(images)
  p = _as_device(captions, v.device)
  r_i, t_i, _ = ops.sim_rank_labelled(v, p, csr_i)
  r_t, t_t, _ = ops.sim_rank_labelled(p, v, csr_t)
  # (the two sides differ in length: one flat vector, cut on the host)
  n, m = r_i.numel(), r_t.numel()
  host = numpy.split(torch.cat([r_i, t_i, r_t, t_t]).cpu().numpy().astype(numpy.float64), [n, 2 * n, 2 * n + m])
  if on_device:
    return ((report_from_ranks(host[0]), t_i, r_i), (report_from_ranks(host[2]), t_t, r_t))
  return ((report_from_ranks(host[0]), host[1], host[0]),
          (report_from_ranks(host[2]), host[3], host[2]))


def _group_labelled_args(clip_embs, cap_embs, reduce):
  if reduce not in ('max', 'mean'):
    raise ValueError("reduce must be 'max' or 'mean', got %r" % (reduce,))
  for x, name in ((clip_embs, 'clip_embs'), (cap_embs, 'cap_embs')):
    if len(getattr(x, 'shape', ())) != 2:
      raise ValueError('%s must be 2-D' % name)
  if clip_embs.shape[1] != cap_embs.shape[1]:
    raise ValueError('embedding widths differ')


def group_rank_labelled(clip_embs, cap_embs, num_clips, num_caps, positives, direction='p2v', reduce='max'):
  """rank_labelled by the group-wise score of the low level (group_i2t_t2i's score) for any video set
  (clip rows, num_clips), any paragraph set (caption rows, num_caps) and any set of correct answers per
  query: direction 'p2v' ranks the videos for every paragraph, 'v2p' the paragraphs for every video, and
  `positives` gives, for every query group, the gallery groups that count as correct (ops.positives_csr's
  forms).  The rank of a query is the rank of its best-placed positive (ops.group_rank_labelled:
  matrix-free, exact fp32).  Returns (report, top1, ranks) in i2t's format (report_from_ranks; float64
  NumPy).  GPU tensors in: top1 and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve
  from is neither read nor changed."""
  _group_labelled_args(clip_embs, cap_embs, reduce)
  # argument errors before the upload
  ops.group_rank_labelled_plan(num_clips, num_caps, len(clip_embs), len(cap_embs), positives, direction)
  on_device = isinstance(clip_embs, torch.Tensor) and clip_embs.is_cuda
  c = _as_device(clip_embs)
  s = _as_device(cap_embs, c.device)
  rank, top1, _ = ops.group_rank_labelled(c, s, num_clips, num_caps, positives, direction, reduce)
  host = torch.stack([rank, top1]).cpu().numpy().astype(numpy.float64)
  if on_device:
    return report_from_ranks(host[0]), top1, rank
  return report_from_ranks(host[0]), host[1], host[0]


def group_i2t_t2i_labelled(clip_embs, cap_embs, num_clips, num_caps, pairs, reduce='max'):
  """group_i2t_t2i for a video set and a paragraph set whose correct answers are given by `pairs`, an
  integer [P, 2] array of (video, paragraph) — any number of groups on either side, any number of correct
  partners per group, at least one (pairs_from_ids builds it from two id lists).  Two annotation sets
  scored against one video set at the low level:

    _, _, clip, cap1, _, _, nclips, ids1 = encode_data(opt, model, val_1_loader)
    _, _, _,    cap2, _, _, ncaps2, ids2 = encode_data(opt, model, val_2_loader)
    caps = numpy.concatenate([cap1, cap2])
    (r_v2p, _, _), (r_p2v, _, _) = group_i2t_t2i_labelled(
        clip, caps, nclips, list(nclips) + list(ncaps2), pairs_from_ids(ids1, ids1 + ids2))

  Returns ((report, top1, ranks) video -> paragraph, the same paragraph -> video), each in i2t's format,
  with one device-to-host copy; with a square problem and pairs (i, i) exactly what group_i2t_t2i returns.
  GPU tensors in: top1 and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is
  neither read nor changed."""
  _group_labelled_args(clip_embs, cap_embs, reduce)
  nv = len(num_clips)
  npar = len(num_caps)
  csr_v, csr_p = csr_from_pairs(pairs, nv, npar)   # argument errors before the upload
  ops.group_rank_labelled_plan(num_clips, num_caps, len(clip_embs), len(cap_embs), csr_v, 'v2p')
  on_device = isinstance(clip_embs, torch.Tensor) and clip_embs.is_cuda
  c = _as_device(clip_embs)
  s = _as_device(cap_embs, c.device)
  r_v, t_v, _ = ops.group_rank_labelled(c, s, num_clips, num_caps, csr_v, 'v2p', reduce)
  r_p, t_p, _ = ops.group_rank_labelled(c, s, num_clips, num_caps, csr_p, 'p2v', reduce)
  # (the two sides differ in length: one flat vector, cut on the host)
  n, m = r_v.numel(), r_p.numel()
  host = numpy.split(torch.cat([r_v, t_v, r_p, t_p]).cpu().numpy().astype(numpy.float64), [n, 2 * n, 2 * n + m])
  if on_device:
    return ((report_from_ranks(host[0]), t_v, r_v), (report_from_ranks(host[2]), t_p, r_p))
  return ((report_from_ranks(host[0]), host[1], host[0]),
          (report_from_ranks(host[2]), host[3], host[2]))


def i2t_t2i_exact(images, captions, ties='optimistic', top1='fp32'):
  """i2t_t2i on the ranks of the FLOAT64 scores of the two matrices, certified (ops.sim_rank_exact):
  independent of summation order, tile shape and machine, where the fp32 ranks of i2t / t2i differ from
  a float64 ranking of the same embeddings on about one row in a few thousand.  Returns
  ((report, top1, ranks) image -> caption, the same caption -> image, info), the first two in i2t_t2i's
  format; `ranks` is rank_lo for ties='optimistic' (a gallery row that ties the positive exactly is not
  counted: i2t's rule) and rank_hi for ties='pessimistic' (it is: a collapsed model reports the last
  rank, not the first).  info = {'i2t': d, 't2i': d, 'resolved': total}, each d with 'report_lo',
  'report_hi' (report_from_ranks of the two vectors), 'tied_rows' (the rows with rank_lo < rank_hi) and
  'resolved' (the pairs that went through float64).  top1='fp32' (the default): top1 is sim_rank's, not
  certified; top1='exact': the arg-max of the float64 scores, the smaller index on a float64 tie, from a
  certified k = 1 retrieval (ops.sim_topk_exact) per direction, whose float64 columns are counted in
  info['top1_resolved'].  NumPy arrays or GPU tensors; one device-to-host copy; GPU tensors in: top1 and
  ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is neither read nor changed."""
  if ties not in ('optimistic', 'pessimistic'):
    raise ValueError("ties must be 'optimistic' or 'pessimistic', got %r" % (ties,))
  if top1 not in ('fp32', 'exact'):
    raise ValueError("top1 must be 'fp32' or 'exact', got %r" % (top1,))
  on_device = isinstance(images, torch.Tensor) and images.is_cuda
  v = _as_device(images)
  p = _as_device(captions, v.device)
  out_i = ops.sim_rank_exact(v, p)
  out_t = ops.sim_rank_exact(p, v)
  n, m = out_i[0].numel(), out_t[0].numel()
  tail = []
  if top1 == 'exact':
    _, top_i, res_i = ops.sim_topk_exact(v, p, 1)
    _, top_t, res_t = ops.sim_topk_exact(p, v, 1)
    out_i = (out_i[0], out_i[1], top_i.reshape(-1), out_i[3])
    out_t = (out_t[0], out_t[1], top_t.reshape(-1), out_t[3])
    tail = [res_i, res_t]        # (per-row counts: summed on the host, where n * M does not overflow)
  # (the two sides may differ in length: one flat vector, cut on the host)
  flat = torch.cat(list(out_i) + list(out_t) + tail).cpu().numpy()
  host_i = [x.astype(numpy.float64) for x in numpy.split(flat[:4 * n], 4)] if n else [numpy.zeros(0)] * 4
  host_t = [x.astype(numpy.float64) for x in numpy.split(flat[4 * n:4 * (n + m)], 4)] if m else [numpy.zeros(0)] * 4
  pick = 0 if ties == 'optimistic' else 1
  info, sides = {}, []
  for name, host, dev in (('i2t', host_i, out_i), ('t2i', host_t, out_t)):
    info[name] = dict(report_lo=report_from_ranks(host[0]), report_hi=report_from_ranks(host[1]),
                      tied_rows=numpy.flatnonzero(host[0] < host[1]), resolved=int(host[3].sum()))
    report = info[name]['report_lo' if pick == 0 else 'report_hi']
    sides.append((report, dev[2], dev[pick]) if on_device else (report, host[2], host[pick]))
  info['resolved'] = info['i2t']['resolved'] + info['t2i']['resolved']
  if top1 == 'exact':
    info['top1_resolved'] = int(flat[4 * (n + m):].astype(numpy.int64).sum())
  return sides[0], sides[1], info


def _check_exact_options(ties, top1):
  if ties not in ('optimistic', 'pessimistic'):
    raise ValueError("ties must be 'optimistic' or 'pessimistic', got %r" % (ties,))
  if top1 not in ('fp32', 'exact'):
    raise ValueError("top1 must be 'fp32' or 'exact', got %r" % (top1,))


def _labelled_exact_side(q, g, csr, top1):
  """(rank_lo, rank_hi, top1, resolved) device tensors of one direction, and the float64 columns of the
  certified arg-max (None with top1='fp32')."""
  lo, hi, t1, _, res = ops.sim_rank_labelled_exact(q, g, csr)
  if top1 != 'exact':
    return (lo, hi, t1, res), None
  _, top, top_res = ops.sim_topk_exact(q, g, 1)
  return (lo, hi, top.reshape(-1), res), top_res


def _exact_side_info(host):
  return dict(report_lo=report_from_ranks(host[0]), report_hi=report_from_ranks(host[1]),
              tied_rows=numpy.flatnonzero(host[0] < host[1]), resolved=int(host[3].sum()))


def rank_labelled_exact(queries, gallery, positives, ties='optimistic', top1='fp32'):
  """rank_labelled on the ranks of the FLOAT64 scores, certified (ops.sim_rank_labelled_exact): the rank of
  a query is the rank of its best-placed positive among the float64 scores of the same embeddings,
  independent of summation order, tile shape and machine.  `positives` as for rank_labelled (lists may be
  unsorted and repeat an index).  Returns (report, top1, ranks, info) with the first three in rank_labelled's
  format; `ranks` is rank_lo for ties='optimistic' (a negative that ties the best positive exactly is not
  counted) and rank_hi for ties='pessimistic' (it is; a positive that ties the best positive never is).
  info = {'report_lo', 'report_hi', 'tied_rows' (the rows with rank_lo < rank_hi), 'resolved' (the columns
  that went through float64)}, and 'top1_resolved' with top1='exact' (the arg-max of the float64 scores from
  ops.sim_topk_exact(..., 1); the default 'fp32' is sim_rank_labelled's top1, not certified).  NumPy in,
  NumPy out (float64), one device-to-host copy; GPU tensors in: top1 and ranks stay int32 device tensors.
  The ranking cache i2t / t2i serve from is neither read nor changed."""
  _check_exact_options(ties, top1)
  on_device = isinstance(queries, torch.Tensor) and queries.is_cuda
  csr = ops.positives_csr(positives, len(queries), len(gallery))   # argument errors before the upload
  q = _as_device(queries)
  dev, top_res = _labelled_exact_side(q, _as_device(gallery, q.device), csr, top1)
  flat = torch.cat(list(dev) + ([top_res] if top_res is not None else [])).cpu().numpy()
  n = dev[0].numel()
  host = [x.astype(numpy.float64) for x in numpy.split(flat[:4 * n], 4)]
  pick = 0 if ties == 'optimistic' else 1
  info = _exact_side_info(host)
  if top1 == 'exact':
    info['top1_resolved'] = int(flat[4 * n:].astype(numpy.int64).sum())
  report = info['report_lo' if pick == 0 else 'report_hi']
  if on_device:
    return report, dev[2], dev[pick], info
  return report, host[2], host[pick], info


def i2t_t2i_labelled_exact(images, captions, pairs, ties='optimistic', top1='fp32'):
  """i2t_t2i_labelled on the ranks of the FLOAT64 scores, certified (ops.sim_rank_labelled_exact): the
  two-annotation-set report of i2t_t2i_labelled's example with i2t_t2i_exact's guarantees and its
  [optimistic, pessimistic] interval.  `pairs` as for i2t_t2i_labelled.  Returns
  ((report, top1, ranks) image -> caption, the same caption -> image, info) with i2t_t2i_exact's structure
  and keys: `ranks` is rank_lo for ties='optimistic' and rank_hi for ties='pessimistic' (every NEGATIVE that
  ties a row's best positive exactly counts against it; another positive of the row that ties it does not:
  two annotation sets that share a caption are not a tie); info = {'i2t': d, 't2i': d, 'resolved': total},
  each d with 'report_lo', 'report_hi', 'tied_rows' and 'resolved'; top1='exact' makes top1 the certified
  float64 arg-max (ops.sim_topk_exact(..., 1) per direction, counted in info['top1_resolved']).  With pairs
  (i, i) exactly what i2t_t2i_exact returns.  NumPy arrays or GPU tensors; one device-to-host copy; GPU
  tensors in: top1 and ranks stay int32 device tensors.  The ranking cache i2t / t2i serve from is neither
  read nor changed."""
  _check_exact_options(ties, top1)
  on_device = isinstance(images, torch.Tensor) and images.is_cuda
  csr_i, csr_t = csr_from_pairs(pairs, len(images), len(captions))   # argument errors before the upload
  v = _as_device(images)
  p = _as_device(captions, v.device)
  out_i, res_i = _labelled_exact_side(v, p, csr_i, top1)
  out_t, res_t = _labelled_exact_side(p, v, csr_t, top1)
  n, m = out_i[0].numel(), out_t[0].numel()
  tail = [res_i, res_t] if top1 == 'exact' else []
  # (the two sides differ in length: one flat vector, cut on the host)
  flat = torch.cat(list(out_i) + list(out_t) + tail).cpu().numpy()
  host_i = [x.astype(numpy.float64) for x in numpy.split(flat[:4 * n], 4)]
  host_t = [x.astype(numpy.float64) for x in numpy.split(flat[4 * n:4 * (n + m)], 4)]
  pick = 0 if ties == 'optimistic' else 1
  info, sides = {}, []
  for name, host, dev in (('i2t', host_i, out_i), ('t2i', host_t, out_t)):
    info[name] = _exact_side_info(host)
    report = info[name]['report_lo' if pick == 0 else 'report_hi']
    sides.append((report, dev[2], dev[pick]) if on_device else (report, host[2], host[pick]))
  info['resolved'] = info['i2t']['resolved'] + info['t2i']['resolved']
  if top1 == 'exact':
    info['top1_resolved'] = int(flat[4 * (n + m):].astype(numpy.int64).sum())
  return sides[0], sides[1], info


def _rank_report(queries, gallery):
  rank, top1 = ops.sim_rank(_as_device(queries), _as_device(gallery))
  ranks = rank.cpu().numpy().astype(numpy.float64)      # the reference stores ranks in float64
  top1 = top1.cpu().numpy().astype(numpy.float64)
  return report_from_ranks(ranks), top1, ranks


def _served(ranks, direction):
  r = ranks[2 * direction].astype(numpy.float64)
  return report_from_ranks(r), ranks[2 * direction + 1].astype(numpy.float64), r


def i2t_t2i(images, captions):
  """Both directions of train.validate's scoring (train.py:234-236: i2t then t2i on the same two
  matrices) with ONE device-to-host copy: the two ranking launches are queued back to back and
  their four int32 vectors come down together.  Returns ((report, top1, ranks) of i2t, same of
  t2i), each exactly what i2t / t2i return."""
  v, p = _as_device(images), _as_device(captions)
  r_i, t_i = ops.sim_rank(v, p)
  r_t, t_t = ops.sim_rank(p, v)
  host = torch.stack([r_i, t_i, r_t, t_t]).cpu().numpy().astype(numpy.float64)
  return ((report_from_ranks(host[0]), host[1], host[0]),
          (report_from_ranks(host[2]), host[3], host[2]))


def i2t(images, captions, npts=None, measure='cosine'):
  """/root/reference/evaluation.py:160-185 (video -> paragraph).  `npts`, `measure` are ignored
  upstream too (:161).  Accepts NumPy arrays (reference contract) or GPU tensors.  Handed the
  arrays the last encode_data returned, unchanged, it reports the ranks that call already
  computed on the device copies (bit-identical: same kernel, same operands)."""
  ranks = _from_last_encode(images, captions)
  if ranks is not None:
    return _served(ranks, 0)
  return _rank_report(images, captions)


def t2i(images, captions, npts=None, measure='cosine'):
  """/root/reference/evaluation.py:188-213 (paragraph -> video)."""
  ranks = _from_last_encode(images, captions)
  if ranks is not None:
    return _served(ranks, 1)
  return _rank_report(captions, images)
