"""Which kernel runs each BPTT step: the rule of bwd_steps / bwd_tail (cmhse_amd/csrc/bwd.hip)
restated for one chain, and the case table of tests/test_gpu_bptt_shapes.py.

The step shapes are a host-side decision the GPU tests cannot see from their results; this module
lets a CPU test prove that every case of the table lands on the shape it names, and that the
crossovers it assumes are the ones the sources hold (tests/test_bptt_shapes_cpu.py)."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'cmhse_amd', 'csrc')

# defaults of the knobs (gru_ws.hpp CMHSE_TUNABLES) and the constants the rule reads; checked
# against the sources by tests/test_bptt_shapes_cpu.py
KNOBS = dict(bwd_mid_max_seqs=512, bwd_split_min_seqs=33, bwd_tail_min_steps=4)
NW8_MAX = 256          # bwd.hip kBwdNw8Max
TAIL_MAX_SEQS = 32     # bwd_step_kernels.hpp kTailMaxSeqs
REC_BM, REC_BN, REC_BK = 32, 128, 32   # bwd_step_kernels.hpp kRecBM / kRecBN / kRecBK
TAIL_KBS = (2, 4, 6, 12, 24)           # the gru_bwd_tail_kernel instantiations of bwd_tail


def counts_of(lens, T=None):
  """Active sequences of every step t = 0 .. T-1 of a batch of sequence lengths."""
  lens = np.asarray(lens)
  T = int(lens.max()) if T is None else T
  return [int((lens > t).sum()) for t in range(T)]


def lens_of(profile):
  """Sequence lengths whose active-sequence counts are `profile` (non-increasing, first > 0)."""
  assert all(a >= b for a, b in zip(profile, profile[1:])) and profile[-1] > 0, profile
  return np.array([sum(1 for c in profile if c > s) for s in range(profile[0])], dtype=np.int64)


def tail_kb(H):
  """KB of gru_bwd_tail_kernel for width H: 16-k blocks per wave in whole pairs, rounded up to an
  instantiation."""
  kb = 2 * ((3 * H // 16 + 15) // 16)
  return next((k for k in TAIL_KBS if kb <= k), TAIL_KBS[-1])


def tail_of(counts, H, knobs=None):
  """(t_lo, KB, MB) of the chain's resident tail, or None.  (Assumes the full chip: resident_fits.)"""
  k = dict(KNOBS, **(knobs or {}))
  T = len(counts)
  if k['bwd_tail_min_steps'] <= 0 or H % 16 != 0 or H > 1024:
    return None
  lo = T
  while lo - 1 >= 1 and counts[lo - 1] <= TAIL_MAX_SEQS:
    lo -= 1
  if T - lo < k['bwd_tail_min_steps']:
    return None
  return lo, tail_kb(H), 2 if counts[lo] > 16 else 1


def split_plan(S_next, H):
  """(splits, k_slice) of bwd_rec_part_kernel's launch for one Split step with S_next > 0."""
  K = 3 * H
  tiles = ((H + REC_BN - 1) // REC_BN) * ((S_next + REC_BM - 1) // REC_BM)
  splits = max(1, min(256 // tiles, K // 64))
  k_slice = ((K + splits - 1) // splits + REC_BK - 1) // REC_BK * REC_BK
  return (K + k_slice - 1) // k_slice, k_slice


def step_shapes(counts, H, dh0, knobs=None):
  """The launched steps of one chain, last step first: dicts with t, S_t, S_next and `shape`
  ('Waves4' / 'Waves8' with `vec`, 'Mid16', 'Mid32', 'Split' with splits / k_slice), then the
  resident tail as one entry {'shape': 'Tail', 'kb', 'mb', 't_lo'} if the chain has one."""
  k = dict(KNOBS, **(knobs or {}))
  T, S = len(counts), counts[0]
  tail = tail_of(counts, H, k)
  out = []
  for t in range(T - 1, -2 if dh0 else -1, -1):
    if tail is not None and t >= tail[0]:
      continue
    S_t = counts[t] if t >= 0 else S
    S_next = counts[t + 1] if t + 1 < T else 0
    vec = H % 4 == 0
    st = dict(t=t, S_t=S_t, S_next=S_next, H=H, vec=vec)
    st['shape'] = 'Waves8' if S_t <= NW8_MAX else 'Waves4'
    if vec and S_t <= k['bwd_mid_max_seqs']:
      st['shape'] = 'Mid16' if S_t <= 16 else 'Mid32'
      if k['bwd_split_min_seqs'] > 0 and S_t >= k['bwd_split_min_seqs']:
        st['shape'] = 'Split'
        st['splits'], st['k_slice'] = split_plan(S_next, H) if S_next > 0 else (0, 0)
    out.append(st)
  if tail is not None:
    out.append(dict(shape='Tail', t_lo=tail[0], kb=tail[1], mb=tail[2], H=H))
  return out


def shape_tags(steps):
  """The named targets one chain's steps reach (the vocabulary of the coverage test)."""
  tags = set()
  for st in steps:
    s = st['shape']
    if s in ('Waves4', 'Waves8'):
      tags.add('%s %s' % (s, 'vec' if st['vec'] else 'scalar'))
    elif s == 'Tail':
      tags.add('Tail KB%d MB%d' % (st['kb'], st['mb']))
    elif s == 'Split':
      tags.add('Split')
      if st['S_next'] == 0:
        tags.add('Split S_next=0')
      else:
        K = 3 * st['H']
        if st['splits'] == 1:
          tags.add('Split splits=1')
        if K - (st['splits'] - 1) * st['k_slice'] < st['k_slice']:
          tags.add('Split short last K slice')
        if st['H'] % REC_BN != 0:
          tags.add('Split ragged column tile')
      if st['S_t'] <= 16:
        tags.add('Split <=16 rows')
    else:
      tags.add(s)
    if s == 'Mid32' and st['S_t'] > 8 * 32:     # more than 8 row tiles of 32 sequences
      tags.add('Mid32 many row tiles')
  return tags


# The cases of tests/test_gpu_bptt_shapes.py: (id, knobs, S, T, I, H, profile, pool, targets).
# `profile` is the active-sequence count of steps t = 0, 1, ...; the BPTT runs them last first.
CASES = [
    ('waves4_vec_to_split', {}, 700, 5, 20, 72, (700, 640, 520, 300, 40), 'attention',
     {'Waves4 vec', 'Split', 'Split S_next=0'}),
    ('waves4_vec_h1024', {}, 600, 3, 64, 1024, (600, 560, 530), 'maxout', {'Waves4 vec'}),
    ('waves4_to_waves8_scalar', {}, 400, 5, 17, 45, (400, 300, 200, 60, 10), 'maxout',
     {'Waves4 scalar', 'Waves8 scalar'}),
    ('waves8_vec_to_one_row', dict(bwd_mid_max_seqs=0, bwd_tail_min_steps=0), 250, 6, 36, 96,
     (250, 200, 120, 33, 16, 1), 'attention', {'Waves8 vec'}),
    ('waves8_vec_h1024', dict(bwd_mid_max_seqs=0, bwd_tail_min_steps=0), 200, 4, 64, 1024,
     (200, 150, 70, 9), 'seq2seq', {'Waves8 vec'}),
    ('mid32_many_row_tiles', dict(bwd_split_min_seqs=0), 480, 6, 24, 128, (480, 400, 200, 33, 17, 5),
     'attention', {'Mid32', 'Mid32 many row tiles', 'Mid16'}),
    ('split_edges', dict(bwd_split_min_seqs=1, bwd_tail_min_steps=0), 64, 6, 20, 200,
     (64, 64, 64, 64, 9, 3), 'seq2seq',
     {'Split S_next=0', 'Split ragged column tile', 'Split short last K slice', 'Split <=16 rows'}),
    # (seq2seq: max pooling over 1100 x 1024 pairs meets fp32 near-ties, where the arg-max may differ
    # from the float64 one; the attention oracle takes a minute at this size)
    ('split_one_slice', dict(bwd_mid_max_seqs=2048), 1100, 3, 32, 1024, (1100, 1100, 1100), 'seq2seq',
     {'Split', 'Split splits=1'}),
]

# tests/test_gpu_chain.py test_bptt_tail_as_one_resident_kernel: (pool, cls, H, S, n_long)
TAIL_CASES = [('attention', 'Attention', 32, 11, 13), ('maxout', 'Maxout', 48, 40, 13),
              ('seq2seq', 'Seq2Seq', 128, 23, 13), ('attention', 'Attention', 1024, 32, 13),
              ('maxout', 'Maxout', 64, 40, 29), ('attention', 'Attention', 1024, 32, 30),
              ('seq2seq', 'Seq2Seq', 128, 13, 13), ('maxout', 'Maxout', 1024, 13, 13),
              ('attention', 'Attention', 256, 13, 13), ('maxout', 'Maxout', 256, 40, 29),
              ('seq2seq', 'Seq2Seq', 512, 13, 13), ('attention', 'Attention', 512, 40, 29)]
TAIL_T = 37


def tail_case_lens(rng, S, n_long, T=TAIL_T):
  """Lengths of a tail case: most sequences end within 9 steps, up to n_long run on to T."""
  lens = rng.randint(1, 9, size=S)
  long_ones = rng.permutation(S)[:min(S, n_long)]
  lens[long_ones] = rng.randint(10, T + 1, size=len(long_ones))
  lens[long_ones[0]] = T
  return lens


def tail_case_counts(H, S, n_long):
  """The active-sequence counts of a TAIL_CASES entry, drawn as the test draws them."""
  return counts_of(tail_case_lens(np.random.RandomState(5 + H), S, n_long), TAIL_T)


def source_constants():
  """The knob defaults and constants above, as the sources state them."""
  ws = open(os.path.join(CSRC, 'gru_ws.hpp')).read()
  bwd = open(os.path.join(CSRC, 'bwd.hip')).read()
  kern = open(os.path.join(CSRC, 'bwd_step_kernels.hpp')).read()
  found = {}
  for name in KNOBS:
    m = re.findall(r'X\(%s,\s*(-?\d+)\)' % name, ws)
    assert len(m) == 1, (name, m)
    found[name] = int(m[0])

  def const(text, name):
    m = re.findall(r'\b%s\s*=\s*(\d+)\s*[,;]' % name, text)
    assert len(m) == 1, (name, m)
    return int(m[0])
  found['kBwdNw8Max'] = const(bwd, 'kBwdNw8Max')
  found['kTailMaxSeqs'] = const(kern, 'kTailMaxSeqs')
  for name in ('kRecBM', 'kRecBN', 'kRecBK'):
    found[name] = const(kern, name)
  found['tail_kbs'] = tuple(int(v) for v in re.findall(r'BWD_TAIL_\((\d+)\)', bwd))
  return found
