#!/usr/bin/env python3
"""Certified top-K timings: ops.sim_topk_exact against ops.sim_topk (the fp32 list, the yardstick) on the
same matrices, the two calls ALTERNATED in one process.  HIP events around each call after warm-up; median,
minimum and maximum of --reps calls.  One JSON line per shape and K.

  correlated   synthetic.correlated_embeddings(4917), 4917 x 4917 x 1024, K = 1 / 10 / 50 / 128
  wide         4917 unit-norm random queries against 200 000 unit-norm random gallery rows, K = 50

`resolved` is the number of columns that went through float64 (the sum of the call's third output),
`per_row` its mean over K, `vs_sim_topk` the ratio of the medians, `rows_fp32_list_differs` the rows whose
fp32 list is not the certified one.  Kernel-level times come from a separate
rocprofv3 --kernel-trace --stats run of this tool.

On a build without sim_topk_exact (the parent of the change that added it) only the sim_topk leg runs, so
the same tool shows whether that call moved.

  python tools/bench_topk_exact.py [--reps 20] [--warmup 3] [--cases correlated wide] [--ks 1 10 50 128]
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


def case(name, q, g, k, reps, warmup, have_exact):
  out = dict(case=name, n=q.shape[0], m=g.shape[0], d=q.shape[1], k=k, reps=reps)
  if not have_exact:
    t, = timed_alternating([lambda: ops.sim_topk(q, g, k)], reps, warmup)
    out.update(sim_topk_ms=r4(t), note='this build has no sim_topk_exact')
  else:
    _, index, resolved = ops.sim_topk_exact(q, g, k)
    _, index32 = ops.sim_topk(q, g, k)
    t = timed_alternating([lambda: ops.sim_topk_exact(q, g, k), lambda: ops.sim_topk(q, g, k)], reps, warmup)
    out.update(exact_ms=r4(t[0]), sim_topk_ms=r4(t[1]), vs_sim_topk=round(t[0][0] / t[1][0], 3),
               resolved=int(resolved.sum()), per_row_over_k=round(float(resolved.float().mean()) / k, 4),
               max_per_row=int(resolved.max()), rows_fp32_list_differs=int((index32 != index).any(dim=1).sum()))
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--cases', nargs='*', default=['correlated', 'wide'])
  ap.add_argument('--ks', nargs='*', type=int, default=[1, 10, 50, 128], help='K of the correlated case')
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  have_exact = hasattr(ops, 'sim_topk_exact')
  if 'correlated' in args.cases:
    a, b = synthetic.correlated_embeddings(4917)
    q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for k in args.ks:
      case('correlated a->b', q, g, k, args.reps, args.warmup, have_exact)
    del q, g
  if 'wide' in args.cases:
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(4917, 1024, device=dev, generator=gen))
    g = torch.nn.functional.normalize(torch.randn(200000, 1024, device=dev, generator=gen))
    case('wide', q, g, 50, args.reps, args.warmup, have_exact)


if __name__ == '__main__':
  main()
