"""What NUMBERS the GRU, attention and normalisation kernels see: value regimes crossed with the shape
cases of tests/fwd_shapes.py and tests/bptt_shapes.py, for tests/test_gpu_value_regimes.py.

The shape suites decide which kernel runs; every one of their cases draws unit-normal inputs, weights
of scale 1/sqrt(H) and biases of 0.1 randn, so the gates sit mid-range, an attention softmax sums to 1
within 1e-4 and no hidden state is small.  The elementwise math is hand-written (sigmoidf_ / tanhf_ on
v_exp_f32 / v_rcp_f32, a softmax without max-subtraction and with +1e-4 in its denominator, a strict->
running maximum, the hi/lo split of pack_bf16): a kernel wrong only where a gate saturates, where the
epsilon dominates the softmax or where tanh is taken near 0 passes all of them.  A REGIME is a function
(fp32 state dict of the layer, x, h0, rng) -> the same, modified; it is applied after the baseline
numbers are drawn (test_gpu_fwd_shapes._setup), so the kernel family of a case is still decided by
fwd_shapes / bptt_shapes alone.  tests/test_value_regimes_cpu.py proves from the float64 oracle that
each regime is what its name says, and from the dispatch rules that each case lands on the kernels it
names.  All inputs stay finite and nothing overflows fp32 in the float64 oracle's intermediates.

Bars.  Outputs: conftest.assert_emb_close with tight = GOLDEN_TOL * max(1, d32(regime) / d32(baseline)),
d32 = the largest distance between the oracle run in fp32 and in float64 on that same case: the
project's 30x head-room over what fp32 arithmetic costs in that regime, taken from the reference and
never from the kernel; EMB_TOL stays fixed.  `baseline` and `small_*`: the same bar on the L2-normalised
rows of the LAST / MAX / ATTN outputs (the model normalises every encoder output before it is scored),
which is where a tanh that cancels near 0 shows.  The bf16x3 cases: the bars of test_gpu_bf3_shapes.py
(BF3_TOL against the oracle, GOLDEN_TOL against the emulation of the split) scaled by the same ratio, and
against the oracle never more than the emulation's own distance from it plus the bar against the emulation.
Under `saturated` and `attn_peaked` the mode's arithmetic itself — the float64 emulation of the split — is
1.4e-3 and 1.8e-4 from the oracle, beyond EMB_TOL: a limit of the opt-in mode at weights eight times the
initialisation's, not of its kernels, which stay within 5e-5 of the emulation there.

Measured on an MI355X (tests/test_gpu_value_regimes.py prints one line per case; largest over the
requests of a case, `norm` = distance of the L2-normalised rows):

  case-regime                          d32        bar        kernel     norm
  tiny_vec_all_pools-baseline          1.986e-07  5.000e-06  2.057e-07  7.612e-08
  tiny_vec_all_pools-saturated         8.366e-06  2.106e-04  6.681e-06  8.376e-07
  tiny_vec_all_pools-frozen            3.173e-07  7.989e-06  1.988e-07  7.448e-08
  tiny_vec_all_pools-reset_off         1.814e-07  5.000e-06  2.186e-07  7.112e-08
  tiny_vec_all_pools-attn_peaked       1.529e-06  3.849e-05  5.324e-07  7.303e-07
  tiny_vec_all_pools-attn_starved      1.986e-07  5.000e-06  2.057e-07  1.586e-07
  tiny_vec_all_pools-small_1e-2        3.695e-09  5.000e-06  2.975e-09  6.880e-08
  tiny_vec_all_pools-small_1e-3        3.516e-10  5.000e-06  2.443e-10  6.773e-08
  tiny_vec_all_pools-small_1e-4        3.245e-11  5.000e-06  3.070e-11  6.805e-08
  tiled64_vec_all_pools-baseline       3.216e-07  5.000e-06  3.812e-07  1.071e-07
  tiled64_vec_all_pools-saturated      1.476e-05  2.296e-04  1.636e-05  1.964e-06
  tiled64_vec_all_pools-frozen         3.431e-07  5.335e-06  3.149e-07  9.293e-08
  tiled64_vec_all_pools-reset_off      4.111e-07  6.392e-06  3.105e-07  1.025e-07
  tiled64_vec_all_pools-attn_peaked    6.669e-07  1.037e-05  2.163e-06  1.838e-07
  tiled64_vec_all_pools-attn_starved   3.216e-07  5.000e-06  3.812e-07  1.875e-07
  tiled64_vec_all_pools-small_1e-2     5.230e-09  5.000e-06  5.471e-09  1.191e-07
  tiled64_vec_all_pools-small_1e-3     6.532e-10  5.000e-06  3.908e-10  1.011e-07
  tiled64_vec_all_pools-small_1e-4     4.104e-11  5.000e-06  5.217e-11  1.083e-07
  chain64_vec_all_pools-baseline       4.003e-07  5.000e-06  3.538e-07  1.187e-07
  chain64_vec_all_pools-saturated      1.192e-05  1.489e-04  1.731e-05  1.909e-06
  chain64_vec_all_pools-frozen         3.447e-07  5.000e-06  3.070e-07  1.048e-07
  chain64_vec_all_pools-reset_off      2.975e-07  5.000e-06  3.299e-07  9.137e-08
  chain64_vec_all_pools-attn_peaked    1.486e-06  1.856e-05  1.558e-06  2.156e-07
  chain64_vec_all_pools-attn_starved   4.003e-07  5.000e-06  3.538e-07  1.576e-07
  chain64_vec_all_pools-small_1e-2     5.026e-09  5.000e-06  5.339e-09  1.093e-07
  chain64_vec_all_pools-small_1e-3     5.991e-10  5.000e-06  6.573e-10  1.449e-07
  chain64_vec_all_pools-small_1e-4     5.649e-11  5.000e-06  5.863e-11  9.438e-08
  mid_u4_all_pools-baseline            2.177e-07  5.000e-06  2.197e-07  7.942e-08
  mid_u4_all_pools-saturated           8.421e-06  1.934e-04  6.065e-06  7.911e-07
  mid_u4_all_pools-frozen              1.711e-07  5.000e-06  2.150e-07  7.009e-08
  mid_u4_all_pools-reset_off           1.774e-07  5.000e-06  1.897e-07  7.009e-08
  mid_u4_all_pools-attn_peaked         2.612e-07  6.000e-06  2.240e-07  8.547e-08
  mid_u4_all_pools-attn_starved        2.177e-07  5.000e-06  2.197e-07  1.309e-07
  mid_u4_all_pools-small_1e-2          3.386e-09  5.000e-06  3.386e-09  7.420e-08
  mid_u4_all_pools-small_1e-3          3.570e-10  5.000e-06  3.570e-10  9.471e-08
  mid_u4_all_pools-small_1e-4          2.522e-11  5.000e-06  3.019e-11  7.060e-08
  mid64_train-baseline                 3.124e-07  5.000e-06  3.076e-07  8.111e-08
  mid64_train-saturated                2.318e-05  3.710e-04  1.253e-05  1.180e-06
  mid64_train-frozen                   2.739e-07  5.000e-06  3.091e-07  6.589e-08
  mid64_train-reset_off                2.751e-07  5.000e-06  3.173e-07  8.115e-08
  mid64_train-small_1e-2               5.390e-09  5.000e-06  4.319e-09  9.855e-08
  mid64_train-small_1e-3               4.797e-10  5.000e-06  4.984e-10  8.721e-08
  mid64_train-small_1e-4               4.027e-11  5.000e-06  3.810e-11  7.725e-08
  fwd_tail_all_train-baseline          2.579e-07  5.000e-06  3.881e-07  8.748e-08
  fwd_tail_all_train-saturated         5.128e-06  9.941e-05  6.695e-06  4.928e-07
  fwd_tail_all_train-frozen            3.006e-07  5.828e-06  3.170e-07  1.036e-07
  fwd_tail_all_train-reset_off         3.619e-07  7.015e-06  2.821e-07  8.472e-08
  fwd_tail_all_train-small_1e-2        5.295e-09  5.000e-06  4.054e-09  8.735e-08
  fwd_tail_all_train-small_1e-3        4.615e-10  5.000e-06  3.642e-10  7.507e-08
  fwd_tail_all_train-small_1e-4        4.180e-11  5.000e-06  4.180e-11  9.009e-08
  waves4_vec_to_split-baseline         2.547e-07  5.000e-06  2.543e-07  7.738e-08
  waves4_vec_to_split-saturated        5.054e-06  9.923e-05  4.909e-06  1.014e-06
  waves4_vec_to_split-frozen           2.325e-07  5.000e-06  2.544e-07  6.167e-08
  waves4_vec_to_split-reset_off        2.308e-07  5.000e-06  2.652e-07  7.924e-08
  waves4_vec_to_split-attn_peaked      3.959e-06  7.774e-05  4.883e-06  2.644e-06
  waves4_vec_to_split-attn_starved     1.069e-07  5.000e-06  9.612e-08  1.863e-07
  waves4_vec_to_split-small_1e-2       2.987e-09  5.000e-06  3.246e-09  9.835e-08
  waves4_vec_to_split-small_1e-3       2.906e-10  5.000e-06  2.931e-10  9.314e-08
  waves4_vec_to_split-small_1e-4       3.732e-11  5.000e-06  3.300e-11  9.550e-08
  waves8_vec_to_one_row-baseline       2.737e-07  5.000e-06  2.643e-07  8.445e-08
  waves8_vec_to_one_row-saturated      8.170e-06  1.493e-04  5.005e-06  8.865e-07
  waves8_vec_to_one_row-frozen         2.581e-07  5.000e-06  2.977e-07  7.899e-08
  waves8_vec_to_one_row-reset_off      2.573e-07  5.000e-06  2.914e-07  9.285e-08
  waves8_vec_to_one_row-attn_peaked    3.385e-06  6.183e-05  5.596e-06  1.588e-06
  waves8_vec_to_one_row-attn_starved   6.872e-08  5.000e-06  5.628e-08  1.319e-07
  waves8_vec_to_one_row-small_1e-2     3.728e-09  5.000e-06  4.065e-09  8.089e-08
  waves8_vec_to_one_row-small_1e-3     4.115e-10  5.000e-06  4.280e-10  8.309e-08
  waves8_vec_to_one_row-small_1e-4     4.391e-11  5.000e-06  4.391e-11  8.437e-08
  mid32_many_row_tiles-baseline        2.620e-07  5.000e-06  2.818e-07  5.948e-08
  mid32_many_row_tiles-saturated       4.390e-06  8.378e-05  3.857e-06  5.077e-07
  mid32_many_row_tiles-frozen          2.505e-07  5.000e-06  2.497e-07  4.960e-08
  mid32_many_row_tiles-reset_off       3.117e-07  5.949e-06  2.174e-07  5.935e-08
  mid32_many_row_tiles-attn_peaked     3.837e-06  7.322e-05  6.179e-06  1.766e-06
  mid32_many_row_tiles-attn_starved    1.192e-07  5.000e-06  6.508e-08  1.333e-07
  mid32_many_row_tiles-small_1e-2      3.695e-09  5.000e-06  2.826e-09  6.783e-08
  mid32_many_row_tiles-small_1e-3      4.012e-10  5.000e-06  3.318e-10  7.019e-08
  mid32_many_row_tiles-small_1e-4      2.735e-11  5.000e-06  2.505e-11  5.748e-08
  bf3_all_pools-saturated              1.139e-05  1.866e-04  4.647e-05  -          emulation; oracle 1.392e-03 (its emulation 1.388e-03, bar 1.866e-03)
  bf3_all_pools-small_1e-2             6.330e-09  5.000e-06  1.068e-08  3.017e-07  emulation; oracle 1.126e-07 (its emulation 1.140e-07, bar 5.000e-05)
  bf3_all_pools-attn_peaked            4.839e-06  7.927e-05  2.857e-05  -          emulation; oracle 1.784e-04 (its emulation 1.649e-04, bar 7.927e-04)
  bf3_all_pools-frozen                 3.263e-07  5.345e-06  1.907e-06  -          emulation; oracle 1.264e-05 (its emulation 1.251e-05, bar 5.345e-05)
  bf3_attn_cut-saturated               9.789e-06  1.712e-04  4.134e-05  -          emulation; oracle 1.107e-03 (its emulation 1.106e-03, bar 1.712e-03)
  bf3_attn_cut-small_1e-2              2.601e-09  5.000e-06  8.382e-09  9.699e-08  emulation; oracle 7.721e-08 (its emulation 7.675e-08, bar 5.000e-05)
  bf3_attn_cut-attn_peaked             5.329e-06  9.322e-05  2.694e-05  -          emulation; oracle 1.647e-04 (its emulation 1.576e-04, bar 9.322e-04)
  bf3_attn_cut-frozen                  2.963e-07  5.182e-06  9.984e-07  -          emulation; oracle 9.304e-06 (its emulation 9.304e-06, bar 5.182e-05)
"""
import functools

import numpy as np

import bptt_shapes
import fwd_shapes as fs

# ------------------------------------------------------------------------------------------------
# regimes
# ------------------------------------------------------------------------------------------------
W_IH, W_HH, B_IH, B_HH = 'rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0'
W_LIN, B_LIN, W_ATT = 'lin.weight', 'lin.bias', 'att_w.weight'
FROZEN_EVERY = 4          # `frozen` / `reset_off` touch units 0, 4, 8, ...
FROZEN_BIAS = 60.0        # z pre-activation > 37: 1 / (1 + exp(-a)) == 1.0 exactly in float64
RESET_BIAS = -110.0       # exp(110) overflows fp32 in the kernel: rcp(inf) = 0, the "saturates cleanly" path
ATTN_PEAK_L1 = 60.0       # sum |w_att|: |e| <= 60, exp(60) = 1.1e26 stays inside fp32
ATTN_PEAK_ALIGN = 8.0
SMALL_SCALES = {'small_1e-2': 1e-2, 'small_1e-3': 1e-3, 'small_1e-4': 1e-4}


def marked_units(H):
  return np.arange(0, H, FROZEN_EVERY)


def baseline(sd, x, h0, rng):
  return sd, x, h0


def saturated(sd, x, h0, rng):
  sd[W_IH] = sd[W_IH] * 8
  sd[W_HH] = sd[W_HH] * 8
  return sd, x * 4, h0


def frozen(sd, x, h0, rng):
  H = sd[W_HH].shape[1]
  sd[B_IH][H + marked_units(H)] = FROZEN_BIAS
  return sd, x, h0


def reset_off(sd, x, h0, rng):
  H = sd[W_HH].shape[1]
  sd[B_IH][marked_units(H)] = RESET_BIAS
  return sd, x, h0


def _small(scale):
  def regime(sd, x, h0, rng):
    sd[B_IH][:] = 0
    sd[B_HH][:] = 0
    return sd, x * np.float32(scale), None if h0 is None else h0 * np.float32(scale)
  return regime


def attn_peaked(sd, x, h0, rng):
  """w_att scaled to sum |w_att| = 60 and w_lin x 4 alone leave e = sum_k w_att[k] v[k] a sum of random
  signs (std 60 / sqrt(H), about 7 at these widths): it cannot span +-30.  So w_lin also gets a rank-one
  term sign(w_att) (d . h) of a random direction d, which lines v up with the signs of w_att: e is then
  about 60 tanh(ATTN_PEAK_ALIGN d . h), of either sign, and |e| < 60 whatever h is (|v| < 1)."""
  if W_ATT in sd:
    H = sd[W_LIN].shape[0]
    sd[W_ATT] = sd[W_ATT] * np.float32(ATTN_PEAK_L1 * (1 - 1e-6) / np.abs(sd[W_ATT]).sum())
    d = rng.standard_normal(H) / np.sqrt(H)
    sd[W_LIN] = (sd[W_LIN] * 4 + ATTN_PEAK_ALIGN * np.outer(np.sign(sd[W_ATT]).reshape(-1), d)).astype(np.float32)
  return sd, x, h0


def attn_starved(sd, x, h0, rng):
  if W_ATT in sd:
    H = sd[W_LIN].shape[0]
    sd[B_LIN][:] = 10.0
    sd[W_LIN] = sd[W_LIN] * 8
    sd[W_ATT] = (-12.0 / H + 0.02 * rng.standard_normal(sd[W_ATT].shape)).astype(np.float32)
  return sd, x, h0


REGIMES = dict(baseline=baseline, saturated=saturated, frozen=frozen, reset_off=reset_off,
               attn_peaked=attn_peaked, attn_starved=attn_starved,
               **{n: _small(s) for n, s in SMALL_SCALES.items()})
ATTN_REGIMES = ('attn_peaked', 'attn_starved')                  # requests with attention pooling only
GATE_REGIMES = tuple(r for r in REGIMES if r not in ATTN_REGIMES)
NORMALISED_REGIMES = ('baseline',) + tuple(SMALL_SCALES)        # the normalised rows are compared too
BF3_REGIMES = ('saturated', 'small_1e-2', 'attn_peaked', 'frozen')

# ------------------------------------------------------------------------------------------------
# cases: a shape case taken BY NAME from the tables, crossed with a regime
# ------------------------------------------------------------------------------------------------
_FWD = {c[0]: c for c in fs.CASES}
_BF3 = {c[0]: c for c in fs.BF3_CASES}
_BPTT = {c[0]: c for c in bptt_shapes.CASES}
_BPTT_POOL = {'attention': 'ATTN', 'maxout': 'MAX', 'seq2seq': 'LAST'}

# (source table, case, the family tags it is here for).  Forward families: the gate epilogue of
# gru_step_tile (Tiled, Chain with its agent-scope running maximum, TiledBf3 with the hi/lo re-split of
# the new state), gru_small_batch.hpp's three (Tiny, Mid in both heights, FwdTail).  BPTT families: the
# backward step kernels reading the saved gates, the resident tail.  'Attn ...': the attention projection.
SHAPES = [
    ('fwd', 'tiny_vec_all_pools', {'Tiny vec'}),
    ('fwd', 'tiled64_vec_all_pools', {'Tiled64 vec', 'Mid MB1 U4 W8'}),
    ('fwd', 'chain64_vec_all_pools', {'Chain64 vec'}),
    ('fwd', 'mid_u4_all_pools', {'Mid MB1 U4 W4', 'Mid MB2 U4 W4'}),
    ('fwd', 'mid64_train', {'Mid64', 'Mid MB2 U16 W8', 'Split', 'Mid16'}),
    ('fwd', 'fwd_tail_all_train', {'FwdTail KB2 MB1', 'FwdTail KB2 MB2', 'Tail KB2 MB1', 'Tail KB2 MB2', 'Mid32',
                                   'Split'}),
    ('bf3', 'bf3_all_pools', {'TiledBf3', 'Attn ring', 'Attn split-in-loop', 'Mid MB1 U4 W8'}),
    ('bf3', 'bf3_attn_cut', {'TiledBf3', 'Attn ring', 'Attn split-in-loop', 'Attn final both'}),
    # one BPTT case per backward step family the training cases above do not reach, all with attention
    # pooling (attn_pool_bwd_kernel under every regime)
    ('bptt', 'waves4_vec_to_split', {'Waves4 vec', 'Split'}),
    ('bptt', 'waves8_vec_to_one_row', {'Waves8 vec'}),
    ('bptt', 'mid32_many_row_tiles', {'Mid32', 'Mid16'}),
]

FWD_FAMILIES = ('Tiny', 'Tiled', 'Chain', 'Mid', 'FwdTail', 'TiledBf3')
BWD_FAMILIES = ('Waves4', 'Waves8', 'Mid16', 'Mid32', 'Split', 'Tail', 'AttnPoolBwd')
# (family, regime) pairs no case reaches, with the reason
UNREACHABLE = {}
for _r in ATTN_REGIMES:
  UNREACHABLE[('FwdTail', _r)] = ('the resident forward tail has no ATTN epilogue (fwd_shapes.FAMILY_POOLS) and the '
                                  'training cases hold no attention request')
for _r in REGIMES:
  if _r not in BF3_REGIMES and _r != 'baseline':
    UNREACHABLE[('TiledBf3', _r)] = ('the bf16x3 cases run in %s only: the epilogue is the one of Tiled (the same '
                                     'gru_step_tile); these four cover what the split adds' % ', '.join(BF3_REGIMES))
UNREACHABLE[('TiledBf3', 'baseline')] = 'tests/test_gpu_bf3_shapes.py is the baseline of every bf16x3 case'


def jobs_of(source, name):
  """(knobs, train, tail_stream, jobs) of a shape case.  A BPTT case becomes one training request with
  initial states on a job stream of its own (layers.run_grouped), under the case's BPTT knobs."""
  if source == 'bptt':
    _, knobs, S, T, I, H, profile, pool, _ = _BPTT[name]
    return knobs, True, False, [fs.job(_BPTT_POOL[pool], profile, I, H, save=True, h0=True, stream='s0')]
  _, knobs, train, tail_stream, jobs, _ = (_FWD if source == 'fwd' else _BF3)[name]
  return knobs, train, tail_stream, jobs


def regimes_of(source, name):
  jobs = jobs_of(source, name)[3]
  regs = BF3_REGIMES if source == 'bf3' else tuple(REGIMES)
  if not any(j['pool'] == 'ATTN' for j in jobs):
    regs = tuple(r for r in regs if r not in ATTN_REGIMES)
  return regs


# the case table: (id, source, shape case, regime, the tags it claims: its families' tags plus the regime)
CASES = [('%s-%s' % (name, r), source, name, r, set(tags) | {r})
         for source, name, tags in SHAPES for r in regimes_of(source, name)]


def shape_tags(source, name):
  """Every tag the dispatch rules give a shape case under its knobs: the forward call's (fwd_shapes.call_tags)
  and, for a training case, the BPTT chain's of every request (bptt_shapes.shape_tags; 'AttnPoolBwd' for
  an attention request)."""
  knobs, train, tail_stream, jobs = jobs_of(source, name)
  fwd_knobs = {k: v for k, v in knobs.items() if k in fs.KNOBS}
  bwd_knobs = {k: v for k, v in knobs.items() if k in bptt_shapes.KNOBS}
  assert set(knobs) == set(fwd_knobs) | set(bwd_knobs)
  tags = fs.call_tags(jobs, fwd_knobs, tail_stream, bf3=source == 'bf3')
  if train:
    for j in jobs:
      tags |= bptt_shapes.shape_tags(bptt_shapes.step_shapes(j['counts'], j['H'], j['h0'], bwd_knobs))
      if j['pool'] == 'ATTN':
        tags.add('AttnPoolBwd')
  return tags


def families_reached(source, name, regime):
  """The (family, regime) pairs a case reaches.  A gate regime: every family that runs a step of the case.
  An attention regime: the forward families that write the states an ATTENTION request pools, and the
  attention pooling's backward."""
  tags = shape_tags(source, name)
  out = set()
  for t in tags:
    fam = 'Tail' if t.startswith('Tail KB') else t.split(' ')[0]
    if fam in BWD_FAMILIES:
      if regime not in ATTN_REGIMES or fam == 'AttnPoolBwd':
        out.add((fam, regime))
      continue
    fam = fs._family(t)
    if fam in FWD_FAMILIES and (regime not in ATTN_REGIMES or '%s ATTN' % fam in tags):
      out.add((fam, regime))
  return out


# ------------------------------------------------------------------------------------------------
# references: the oracle in float64 and in fp32, once per (case, regime) and process, read-only
# ------------------------------------------------------------------------------------------------
def setup(source, name, regime, dev):
  """test_gpu_fwd_shapes._setup of a case under a regime, plus the d(out) weights of a training case."""
  from test_gpu_fwd_shapes import _setup
  jobs = jobs_of(source, name)[3]
  layers_, sds, data, rng = _setup(jobs, dev, REGIMES[regime])
  ws = [rng.standard_normal((int(d[0].sum()) if j['pool'] == 'ALL' else len(d[0]), j['H'])).astype(np.float32)
        for j, d in zip(jobs, data)]
  return jobs, layers_, sds, data, ws


def normalised(a):
  """F.normalize of the rows, in float64."""
  a = np.asarray(a, dtype=np.float64)
  return a / np.maximum(np.sqrt((a * a).sum(axis=1, keepdims=True)), 1e-12)


def _frozen(v):
  if isinstance(v, np.ndarray):
    v.setflags(write=False)
  return v


@functools.lru_cache(maxsize=None)
def reference(oracle, source, name, regime):
  """Per request of the case: want / cache (float64), want32 / cache32 (the same oracle in fp32), d32 and
  d32n (their distance, raw and on the normalised rows); for a bf16x3 case also the emulation of the split
  (emu, emu_hs, as tests/test_gpu_bf3_shapes.py builds it).  The oracle's exp overflows on purpose in
  `reset_off` (exp(110) in fp32): that warning is silenced here, not in the oracle."""
  import torch
  from gpu_common import _blas_threads
  from test_gpu_fwd_shapes import _ORACLE_POOL, _oracle
  knobs, train, tail_stream, jobs = jobs_of(source, name)
  _, _, sds, data, ws = setup(source, name, regime, torch.device('cpu'))
  plan = fs.call_steps(jobs, knobs, tail_stream, bf3=True) if source == 'bf3' else [None] * len(jobs)
  out = []
  for j, sd, (lens, x, h0, _, _), w, launches in zip(jobs, sds, data, ws, plan):
    with _blas_threads(), np.errstate(over='ignore'):
      want, cache = _oracle(oracle, j, x, lens, sd, h0)
      want32, cache32 = oracle.pooled_gru_forward_cache(_ORACLE_POOL[j['pool']], x, lens, sd, h0, dtype=np.float32)
      if j['pool'] == 'ALL':
        want32 = np.concatenate([cache32['hs'][i, :l] for i, l in enumerate(lens)])
      ref = dict(want=want, cache=cache, want32=want32, cache32=cache32, lens=lens, w=w,
                 d32=float(np.abs(want32.astype(np.float64) - want).max()),
                 d32n=float(np.abs(normalised(want32) - normalised(want)).max()))
      if source == 'bf3':
        split_steps = sum(len(ln['ts']) for ln in launches if ln['tag'] == 'TiledBf3')
        split_att = any(ln['kind'] == 'attn' and ln['bf3'] for ln in launches)
        emu, emu_hs = oracle.pooled_gru_forward(_ORACLE_POOL[j['pool']], x, lens, sd, h0, np.float64,
                                                products='bf16x3', split_steps=split_steps,
                                                split_attention=split_att)
        if j['pool'] == 'ALL':
          emu = np.concatenate([emu_hs[i, :l] for i, l in enumerate(lens)])
        ref.update(emu=emu, emu_hs=emu_hs)
    for c in (cache, cache32):
      for v in c.values():
        _frozen(v)
    out.append({k: _frozen(v) for k, v in ref.items()})
  return tuple(out)


def case_d32(oracle, source, name, regime):
  """d32 of a case: the largest distance between the fp32 and the float64 oracle over its requests."""
  return max(r['d32'] for r in reference(oracle, source, name, regime))


def bar_scale(oracle, source, name, regime):
  """max(1, d32(regime) / d32(baseline)): what scales every bar of the case."""
  return max(1.0, case_d32(oracle, source, name, regime) / case_d32(oracle, source, name, 'baseline'))


# ------------------------------------------------------------------------------------------------
# F.normalize at the clamp: the rows of tests/test_gpu_value_regimes.py's row-kernel tests
# ------------------------------------------------------------------------------------------------
NORM_ROWS = 7
NORM_COLS = (8, 33, 1024, 1028)     # vector and scalar paths, more than one trip of the 256-thread column loop
NORM_EPS = 1e-12


def clamp_rows(cols, seed=0):
  """(x [7, cols] fp32, g [7, cols] fp32): an all-zero row, rows of norm 0.5e-12, 0.9e-12 and 1.1e-12, rows
  of elements about 1e-15 and about 1e+15 (no square overflows or flushes: 1e-30 and 1e+30 are normal
  fp32 numbers), an ordinary row."""
  rng = np.random.RandomState(100 + cols + seed)
  x = rng.standard_normal((NORM_ROWS, cols))
  x[0] = 0
  for r, n in ((1, 0.5e-12), (2, 0.9e-12), (3, 1.1e-12)):
    x[r] *= n / np.sqrt((x[r] ** 2).sum())
  x[4] *= 1e-15
  x[5] *= 1e+15
  g = rng.standard_normal((NORM_ROWS, cols))
  return x.astype(np.float32), g.astype(np.float32)
