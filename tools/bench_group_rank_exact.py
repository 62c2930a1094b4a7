#!/usr/bin/env python3
"""Certified group-wise ranking timings: ops.group_rank_exact against ops.group_rank (the fp32 group ranking, the
yardstick) on the same rows, the two calls ALTERNATED in one process.  HIP events around each whole call (plan,
upload and workspace allocation included, as a caller pays them) after warm-up; median, minimum and maximum of
--reps calls.  One JSON line per case and reduce mode.

  val1      synthetic.anet_like_spec(4917) counts (17 502 clip and caption rows) of
            synthetic.correlated_embeddings rows, D = 1024: the validation shape
  all_f64   the 512-video shape with rank_exact_tol_scale = 2^20: every off-diagonal block through float64,
            the upper bound of the cost (--reps is cut to 3 for it)

`resolved` is the number of blocks that went through float64 (the sum of the two `resolved` outputs; a block
both directions want is counted twice and computed once); `vs_group_rank` the ratio of the medians.  Kernel-level
times come from a separate rocprofv3 --kernel-trace --stats run of this tool.

On a build without group_rank_exact (the parent of the change that added it) only the group_rank leg runs, so
the same tool shows whether that call moved.

  python tools/bench_group_rank_exact.py [--reps 20] [--warmup 3] [--cases val1 all_f64] [--reduce max mean]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cmhse_amd import ops, synthetic  # noqa: E402


def timed_alternating(fns, reps, warmup):
  """[(median, min, max) ms] of each fn, called in turn: a, b, a, b, ..."""
  for _ in range(warmup):
    for fn in fns:
      fn()
  ms = [[] for _ in fns]
  for _ in range(reps):
    for k, fn in enumerate(fns):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      e1.synchronize()
      ms[k].append(e0.elapsed_time(e1))
  return [(statistics.median(m), min(m), max(m)) for m in ms]


def r4(t):
  return [round(x, 4) for x in t]


def case(name, c, s, counts, reduce, reps, warmup, have_exact, scale=1):
  B = len(counts)
  out = dict(case=name, reduce=reduce, videos=B, clip_rows=c.shape[0], cap_rows=s.shape[0], d=c.shape[1], reps=reps)
  if not have_exact:
    t, = timed_alternating([lambda: ops.group_rank(c, s, counts, reduce=reduce)], reps, warmup)
    out.update(group_rank_ms=r4(t), note='this build has no group_rank_exact')
  else:
    with ops.tuned(rank_exact_tol_scale=scale):
      got = ops.group_rank_exact(c, s, counts, reduce=reduce)
      r_v, _, r_p, _ = ops.group_rank(c, s, counts, reduce=reduce)
      t = timed_alternating([lambda: ops.group_rank_exact(c, s, counts, reduce=reduce),
                             lambda: ops.group_rank(c, s, counts, reduce=reduce)], reps, warmup)
    out.update(tol_scale=scale, exact_ms=r4(t[0]), group_rank_ms=r4(t[1]),
               vs_group_rank=round(t[0][0] / t[1][0], 3),
               resolved=int(got[3].sum()) + int(got[7].sum()), blocks=2 * B * (B - 1),
               queries_fp32_rank_differs=int((r_v != got[0]).sum()) + int((r_p != got[4]).sum()),
               queries_tied=int((got[1] != got[0]).sum()) + int((got[5] != got[4]).sum()))
  print(json.dumps(out), flush=True)


def inputs(n_videos, dev):
  counts = synthetic.anet_like_spec(n_videos).num_clips
  a, b = synthetic.correlated_embeddings(sum(counts), 1024, seed=3)
  return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), counts


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--cases', nargs='*', default=['val1', 'all_f64'])
  ap.add_argument('--reduce', nargs='*', default=['max', 'mean'])
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  have_exact = hasattr(ops, 'group_rank_exact')
  if 'val1' in args.cases:
    c, s, counts = inputs(4917, dev)
    for reduce in args.reduce:
      case('val1', c, s, counts, reduce, args.reps, args.warmup, have_exact)
  if 'all_f64' in args.cases and have_exact:
    c, s, counts = inputs(512, dev)
    for reduce in args.reduce:
      case('all_f64', c, s, counts, reduce, min(args.reps, 3), 1, True, scale=1 << 20)


if __name__ == '__main__':
  main()
