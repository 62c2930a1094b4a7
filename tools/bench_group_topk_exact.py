#!/usr/bin/env python3
"""Certified group-wise top-K timings: ops.group_topk_exact against ops.group_topk (the fp32 list, the yardstick)
on the same rows, the two calls ALTERNATED in one process.  HIP events around each whole call after warm-up;
median, minimum and maximum of --reps calls.  One JSON line per shape, direction, reduce mode and K.

  val1      4917 ActivityNet-shaped videos (17 502 clip rows x 17 502 caption rows x 1024), correlated
            embeddings: K = 1 / 10 / 50 / 128, p2v and v2p, 'max' and 'mean'
  all_f64   the 512-video shape with rank_exact_tol_scale = 2^20: every gallery group of every query goes through
            float64, the upper bound of the cost on that shape (K = 50, 3 calls)

`resolved` is the number of (query, gallery group) blocks that went through float64 (the sum of the call's third
output), `per_query_over_k` its mean over K, `max_per_query` its largest entry, `vs_group_topk` the ratio of the
medians, `queries_fp32_list_differs` the queries whose fp32 list is not the certified one.  Kernel-level times
come from a separate rocprofv3 --kernel-trace --stats run of this tool.

On a build without group_topk_exact (the parent of the change that added it) only the group_topk leg runs, so the
same tool shows whether that call moved.

  python tools/bench_group_topk_exact.py [--reps 20] [--warmup 3] [--cases val1 all_f64] [--ks 1 10 50 128]
                                         [--directions p2v v2p] [--reduce max mean]
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


def case(name, c, s, counts, k, direction, reduce, reps, warmup, have_exact, scale=1):
  out = dict(case=name, direction=direction, reduce=reduce, k=k, videos=len(counts), clip_rows=c.shape[0],
             cap_rows=s.shape[0], d=c.shape[1], reps=reps)
  fp32 = lambda: ops.group_topk(c, s, counts, counts, k, direction, reduce)
  if not have_exact:
    t, = timed_alternating([fp32], reps, warmup)
    out.update(group_topk_ms=r4(t), note='this build has no group_topk_exact')
  else:
    exact = lambda: ops.group_topk_exact(c, s, counts, counts, k, direction, reduce)
    with ops.tuned(rank_exact_tol_scale=scale):
      _, index, resolved = exact()
      _, index32 = fp32()
      t = timed_alternating([exact, fp32], reps, warmup)
    out.update(tol_scale=scale, exact_ms=r4(t[0]), group_topk_ms=r4(t[1]), vs_group_topk=round(t[0][0] / t[1][0], 3),
               resolved=int(resolved.sum()), per_query_over_k=round(float(resolved.float().mean()) / k, 4),
               max_per_query=int(resolved.max()), queries_fp32_list_differs=int((index32 != index).any(dim=1).sum()))
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
  ap.add_argument('--ks', nargs='*', type=int, default=[1, 10, 50, 128], help='K of the val1 case')
  ap.add_argument('--directions', nargs='*', default=['p2v', 'v2p'])
  ap.add_argument('--reduce', nargs='*', default=['max', 'mean'])
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  have_exact = hasattr(ops, 'group_topk_exact')
  if 'val1' in args.cases:
    c, s, counts = inputs(4917, dev)
    for reduce in args.reduce:
      for direction in args.directions:
        for k in args.ks:
          case('val1', c, s, counts, k, direction, reduce, args.reps, args.warmup, have_exact)
  if 'all_f64' in args.cases and have_exact:
    c, s, counts = inputs(512, dev)
    for reduce in args.reduce:
      for direction in args.directions:
        case('all_f64', c, s, counts, 50, direction, reduce, min(args.reps, 3), 1, True, scale=1 << 20)


if __name__ == '__main__':
  main()
