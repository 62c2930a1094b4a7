#!/usr/bin/env python3
"""Certified ranking timings: ops.sim_rank_exact against ops.sim_rank (the fp32 ranking, the yardstick) on
the same matrices, the two calls ALTERNATED in one process.  HIP events around each call after warm-up;
median, minimum and maximum of --reps calls.  One JSON line per case.

  correlated   synthetic.correlated_embeddings(4917), 4917 x 4917 x 1024, both directions: the validation
               shape; a few thousand of its 24 M pairs are undecided in fp32
  flat         a random-init-like case of the same shape: every row is one common unit vector plus noise,
               so all scores lie within 1e-3 of each other — the worst realistic share of undecided pairs
  all_f64      `correlated` with rank_exact_tol_scale = 2^20: every pair through float64, the upper bound
               of the cost (--reps is cut to 3 for it)

`resolved` is the number of pairs that went through float64 (the sum of the call's fourth output);
`vs_sim_rank` the ratio of the medians.  Kernel-level times come from a separate
rocprofv3 --kernel-trace --stats run of this tool.

On a build without sim_rank_exact (the parent of the change that added it) only the sim_rank leg runs,
so the same tool shows whether that call moved.

  python tools/bench_rank_exact.py [--reps 20] [--warmup 3] [--cases correlated flat all_f64]
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


def case(name, q, g, reps, warmup, have_exact, scale=1):
  n, d = q.shape
  out = dict(case=name, n=n, m=g.shape[0], d=d, reps=reps)
  if not have_exact:
    t, = timed_alternating([lambda: ops.sim_rank(q, g)], reps, warmup)
    out.update(sim_rank_ms=r4(t), note='this build has no sim_rank_exact')
  else:
    with ops.tuned(rank_exact_tol_scale=scale):
      lo, hi, _, resolved = ops.sim_rank_exact(q, g)
      rank, _ = ops.sim_rank(q, g)
      t = timed_alternating([lambda: ops.sim_rank_exact(q, g), lambda: ops.sim_rank(q, g)], reps, warmup)
    out.update(tol_scale=scale, exact_ms=r4(t[0]), sim_rank_ms=r4(t[1]), vs_sim_rank=round(t[0][0] / t[1][0], 3),
               resolved=int(resolved.sum()), pairs=n * (g.shape[0] - 1),
               rows_fp32_rank_differs=int((rank != lo).sum()), rows_tied=int((hi != lo).sum()))
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--cases', nargs='*', default=['correlated', 'flat', 'all_f64'])
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  have_exact = hasattr(ops, 'sim_rank_exact')
  a, b = synthetic.correlated_embeddings(4917)
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  if 'correlated' in args.cases:
    case('correlated a->b', q, g, args.reps, args.warmup, have_exact)
    case('correlated b->a', g, q, args.reps, args.warmup, have_exact)
  if 'flat' in args.cases:
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    common = torch.nn.functional.normalize(torch.randn(1, 1024, device=dev, generator=gen))
    # noise of norm ~ 1e-2 per row: the scores are 1 + O(1e-2 * 1e-2 + 1e-4) — all within 1e-3
    fq = torch.nn.functional.normalize(common + 3e-4 * torch.randn(4917, 1024, device=dev, generator=gen))
    fg = torch.nn.functional.normalize(common + 3e-4 * torch.randn(4917, 1024, device=dev, generator=gen))
    spread = float((fq[:64] @ fg.T).max() - (fq[:64] @ fg.T).min())
    print(json.dumps(dict(case='flat', score_spread_first_64_rows=round(spread, 6))), flush=True)
    case('flat', fq, fg, args.reps, args.warmup, have_exact)
  if 'all_f64' in args.cases and have_exact:
    case('all_f64', q, g, min(args.reps, 3), 1, True, scale=1 << 20)


if __name__ == '__main__':
  main()
