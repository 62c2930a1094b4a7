#!/usr/bin/env python3
"""Labelled ranking timings: ops.sim_rank_labelled against ops.sim_rank (the diagonal ranking, the
yardstick) on the same inputs, the two calls ALTERNATED in one process.  HIP events around each call
after warm-up; median, minimum and maximum of --reps calls.  One JSON line per case.

  identity   4917 x 4917 x 1024, labels P_i = {i}: the same tile work as sim_rank (39 threshold tiles
             for 39 diagonal tiles, the same 1521 counting tiles) plus one decoding launch
  val        the two-annotation-set shape: 4917 videos x 9802 paragraphs with 9802 pairs (one or two
             positives per video), and the reverse, 9802 x 4917 with one target each
  many       4917 x 4917, 20 positives per query: 98 340 pairs = 769 threshold tiles

Cost model: ceil(n_pairs / 128) threshold tiles + ceil(n / 128) * ceil(m / 128) counting tiles, every
tile 128 x 128 x d.  `threshold_ms` is measured by difference: the call's median minus the median of
the same call with only the first positive of every query (ceil(n / 128) threshold tiles, the least a
call can have); `tflops` is 2 n m d over the whole call's median.  Kernel-level times come from a
separate rocprofv3 --kernel-trace --stats run of this tool.

On a build without sim_rank_labelled (the parent of the change that added it) only the sim_rank leg
of `identity` runs, so the same tool shows whether that call moved.

  python tools/bench_rank_labelled.py [--reps 20] [--warmup 3] [--cases identity val many]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
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


def labelled_case(name, q, g, off, idx, args, rank_too):
  n, d = q.shape
  m = g.shape[0]
  first = (np.arange(n + 1), idx[off[:-1]])
  fns = [lambda: ops.sim_rank_labelled(q, g, (off, idx)), lambda: ops.sim_rank_labelled(q, g, first)]
  if rank_too:
    fns.append(lambda: ops.sim_rank(q, g))
  t = timed_alternating(fns, args.reps, args.warmup)
  pairs = int(off[-1])
  out = dict(case=name, n=n, m=m, d=d, pairs=pairs, reps=args.reps,
             threshold_tiles=math.ceil(pairs / 128), counting_tiles=math.ceil(n / 128) * math.ceil(m / 128),
             labelled_ms=r4(t[0]), one_positive_ms=r4(t[1]),
             threshold_ms=round(t[0][0] - t[1][0], 4) if pairs > n else None,
             tflops=round(2.0 * n * m * d / 1e9 / t[0][0], 1))
  if pairs > n:
    out['threshold_share'] = round((t[0][0] - t[1][0]) / t[0][0], 3)
  if rank_too:
    out['sim_rank_ms'] = r4(t[2])
    out['vs_sim_rank'] = round(t[0][0] / t[2][0], 3)
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--cases', nargs='*', default=['identity', 'val', 'many'])
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  a, b = synthetic.correlated_embeddings(4917)
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  n = 4917
  if not hasattr(ops, 'sim_rank_labelled'):
    t, = timed_alternating([lambda: ops.sim_rank(q, g)], args.reps, args.warmup)
    print(json.dumps(dict(case='identity', n=n, m=n, d=1024, reps=args.reps, sim_rank_ms=r4(t),
                          note='this build has no sim_rank_labelled')), flush=True)
    return
  rng = np.random.RandomState(0)
  if 'identity' in args.cases:
    labelled_case('identity', q, g, np.arange(n + 1), np.arange(n), args, True)
  if 'val' in args.cases:
    # a second annotation set for a sorted random subset of 4885 videos: fresh noise around the same rows
    keep = np.sort(rng.permutation(n)[:4885])
    g2 = torch.nn.functional.normalize(g[torch.from_numpy(keep).to(dev)] + 0.05 * torch.randn(4885, 1024, device=dev))
    paras = torch.cat([g, g2])
    second = np.full(n, -1)
    second[keep] = n + np.arange(4885)
    lists = [[i] if second[i] < 0 else [i, int(second[i])] for i in range(n)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    labelled_case('val v2p', q, paras, off, np.concatenate(lists), args, True)
    labelled_case('val p2v', paras, q, np.arange(9802 + 1), np.concatenate([np.arange(n), keep]), args, False)
    del paras, g2
  if 'many' in args.cases:
    idx = rng.randint(0, n, size=(n, 20))
    idx[:, 0] = np.arange(n)
    labelled_case('many', q, g, 20 * np.arange(n + 1), idx.reshape(-1), args, True)


if __name__ == '__main__':
  main()
