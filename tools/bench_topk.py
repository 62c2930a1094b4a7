#!/usr/bin/env python3
"""Top-K retrieval timings: ops.sim_topk against ops.sim_rank (the same exact-fp32 GEMM with its
rank epilogue, the yardstick) and ops.cosine_sim + torch.topk (the whole matrix through HBM).
HIP events around each launch after warm-up; the median of --reps launches per shape.  One JSON
line per shape.

  python tools/bench_topk.py [--reps 20] [--warmup 3] [--shapes 4917x4917x1024:1,10,50,128 ...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cmhse_amd import ops  # noqa: E402

SHAPES = ['4917x4917x1024:1,10,50,128', '4917x200000x1024:50', '256x200000x1024:10']


def timed(fn, reps, warmup):
  for _ in range(warmup):
    fn()
  ms = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
  return statistics.median(ms)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--shapes', nargs='*', default=SHAPES, help='NxMxD:K1,K2,...')
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  gen = torch.Generator(device=dev)
  gen.manual_seed(0)
  for spec in args.shapes:
    dims, ks = spec.split(':')
    n, m, d = (int(x) for x in dims.split('x'))
    q = torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=gen))
    g = torch.nn.functional.normalize(torch.randn(m, d, device=dev, generator=gen))
    gflop = 2.0 * n * m * d / 1e9
    rank_ms = timed(lambda: ops.sim_rank(q, g), args.reps, args.warmup) if n <= m else None
    for k in (int(x) for x in ks.split(',')):
      topk_ms = timed(lambda: ops.sim_topk(q, g, k), args.reps, args.warmup)
      mm_ms = timed(lambda: torch.topk(ops.cosine_sim(q, g), k, dim=1), args.reps, args.warmup)
      print(json.dumps(dict(
          n=n, m=m, d=d, k=k, gflop=round(gflop, 1), reps=args.reps,
          sim_topk_ms=round(topk_ms, 4), sim_rank_ms=None if rank_ms is None else round(rank_ms, 4),
          cosine_sim_topk_ms=round(mm_ms, 4),
          sim_topk_tflops=round(gflop / topk_ms, 1),
          vs_sim_rank=None if rank_ms is None else round(topk_ms / rank_ms, 2),
          vs_cosine_sim_topk=round(topk_ms / mm_ms, 2))), flush=True)
    del q, g
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
