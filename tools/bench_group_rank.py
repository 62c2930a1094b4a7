#!/usr/bin/env python3
"""Group-wise ranking timings: ops.group_rank and ops.group_scores against ops.sim_rank(C, S) on the
same clip / caption rows (the same exact-fp32 GEMM with its rank epilogue, the yardstick) and
against ops.cosine_sim + torch segment reductions (the whole clip x caption matrix through HBM).
HIP events around each call after warm-up; the median of --reps calls per shape.  One JSON line per
shape and reduction.

  python tools/bench_group_rank.py [--reps 20] [--warmup 3] [--videos 4917 512] [--reduce max mean]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cmhse_amd import ops, synthetic  # noqa: E402


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


def torch_group(c, s, ids, B, reduce):
  """cosine_sim + segment reductions (rows, then columns) + the ranks of G."""
  scores = ops.cosine_sim(c, s)
  if reduce == 'max':
    t = torch.empty(B, scores.shape[1], device=c.device)
    t.scatter_reduce_(0, ids[:, None].expand_as(scores), scores, 'amax', include_self=False)
    G = torch.empty(B, B, device=c.device)
    G.scatter_reduce_(1, ids[None, :].expand_as(t), t, 'amax', include_self=False)
  else:
    t = torch.zeros(B, scores.shape[1], dtype=torch.float64, device=c.device).index_add_(0, ids, scores.double())
    G = torch.zeros(B, B, dtype=torch.float64, device=c.device).index_add_(1, ids, t)
    cnt = torch.bincount(ids, minlength=B).double()
    G = (G / (cnt[:, None] * cnt[None, :])).float()
  d = G.diagonal()
  return (G > d[:, None]).sum(1), G.argmax(1), (G > d[None, :]).sum(0), G.argmax(0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--videos', type=int, nargs='*', default=[4917, 512])
  ap.add_argument('--reduce', nargs='*', default=['max', 'mean'])
  ap.add_argument('--dim', type=int, default=1024)
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  for B in args.videos:
    counts = synthetic.anet_like_spec(B).num_clips
    n = sum(counts)
    a, b = synthetic.correlated_embeddings(n, args.dim, seed=0)
    c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    ids = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))
    rank_ms = timed(lambda: ops.sim_rank(c, s), args.reps, args.warmup)
    gflop = 2.0 * n * n * args.dim / 1e9
    for reduce in args.reduce:
      rank_g = timed(lambda: ops.group_rank(c, s, counts, reduce=reduce), args.reps, args.warmup)
      scores_g = timed(lambda: ops.group_scores(c, s, counts, reduce=reduce), args.reps, args.warmup)
      torch_ms = timed(lambda: torch_group(c, s, ids, B, reduce), args.reps, args.warmup)
      print(json.dumps(dict(
          videos=B, clips=n, d=args.dim, reduce=reduce, gflop=round(gflop, 1), reps=args.reps,
          group_rank_ms=round(rank_g, 4), group_scores_ms=round(scores_g, 4), sim_rank_ms=round(rank_ms, 4),
          cosine_sim_torch_ms=round(torch_ms, 4),
          group_rank_vs_sim_rank=round(rank_g / rank_ms, 3),
          group_rank_vs_cosine_sim_torch=round(rank_g / torch_ms, 3))), flush=True)
    del c, s
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
