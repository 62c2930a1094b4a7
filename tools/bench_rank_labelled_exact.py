#!/usr/bin/env python3
"""Certified labelled ranking timings: ops.sim_rank_labelled_exact against ops.sim_rank_labelled (the fp32
labelled ranking, the yardstick) on the same inputs and labels, the calls ALTERNATED in one process.  HIP
events around each call after warm-up; median, minimum and maximum of --reps calls.  One JSON line per case.

  identity   4917 x 4917 x 1024, labels P_i = {i}: the diagonal protocol through the labelled calls.  The
             diagonal calls (ops.sim_rank_exact, ops.sim_rank) are alternated with them, so all four cells of
             the ranking grid and both certified / fp32 ratios come from one loop on one box
  val        tools/bench_rank_labelled.py's two-annotation-set shape: 4917 videos x 9802 paragraphs with 9802
             pairs (one or two positives per video), and the reverse, 9802 x 4917 with one target each
  many       4917 x 4917, 20 positives per query (distinct after the call's de-duplication: `pairs` counts them)
  all_f64    `identity` with rank_exact_tol_scale = 2^20: every column through float64, the upper bound of the
             cost (--reps is cut to 3 for it)

Per-launch times by difference, no profiler: `threshold_ms` is the call's median minus the median of the same
call with only the first positive of every query (nrows float64 pair scores, the least a call can have);
`vs_labelled` is the ratio of the medians; on `identity`, `exact_minus_labelled_ms` set beside
`rank_exact_minus_sim_rank_ms` shows what the certified counting pass, the pre-pass and the float64 threshold
pass cost over their fp32 counterparts in either protocol.  `resolved` is the number of columns that went
through float64 (the sum of the call's fifth output).

  python tools/bench_rank_labelled_exact.py [--reps 20] [--warmup 3] [--cases identity val many all_f64]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

from cmhse_amd import ops, synthetic  # noqa: E402
from bench_rank_exact import r4, timed_alternating  # noqa: E402


def case(name, q, g, off, idx, reps, warmup, diagonal=False, scale=1):
  n, d = q.shape
  m = g.shape[0]
  off, idx = ops.sorted_unique_csr(off, idx)        # what the call would do itself: outside the timed region
  first = (np.arange(n + 1), idx[off[:-1]])
  with ops.tuned(rank_exact_tol_scale=scale):
    lo, hi, _, best, resolved = ops.sim_rank_labelled_exact(q, g, (off, idx))
    rank, _, best32 = ops.sim_rank_labelled(q, g, (off, idx))
    fns = [lambda: ops.sim_rank_labelled_exact(q, g, (off, idx)), lambda: ops.sim_rank_labelled(q, g, (off, idx)),
           lambda: ops.sim_rank_labelled_exact(q, g, first)]
    if diagonal:
      fns += [lambda: ops.sim_rank_exact(q, g), lambda: ops.sim_rank(q, g)]
    t = timed_alternating(fns, reps, warmup)
  pairs = int(off[-1])
  out = dict(case=name, n=n, m=m, d=d, pairs=pairs, reps=reps, tol_scale=scale,
             labelled_exact_ms=r4(t[0]), labelled_ms=r4(t[1]), vs_labelled=round(t[0][0] / t[1][0], 3),
             exact_minus_labelled_ms=round(t[0][0] - t[1][0], 4), one_positive_exact_ms=r4(t[2]),
             threshold_ms=round(t[0][0] - t[2][0], 4) if pairs > n else None,
             resolved=int(resolved.sum().item()), columns=n * m,
             rows_fp32_rank_differs=int((rank != lo).sum()), rows_fp32_best_pos_differs=int((best32 != best).sum()),
             rows_tied=int((hi != lo).sum()))
  if diagonal:
    out.update(rank_exact_ms=r4(t[3]), sim_rank_ms=r4(t[4]), rank_exact_vs_sim_rank=round(t[3][0] / t[4][0], 3),
               rank_exact_minus_sim_rank_ms=round(t[3][0] - t[4][0], 4))
  print(json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--cases', nargs='*', default=['identity', 'val', 'many', 'all_f64'])
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  a, b = synthetic.correlated_embeddings(4917)
  q, g = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  n = 4917
  rng = np.random.RandomState(0)
  if 'identity' in args.cases:
    case('identity', q, g, np.arange(n + 1), np.arange(n), args.reps, args.warmup, diagonal=True)
  if 'val' in args.cases:
    # (tools/bench_rank_labelled.py's: a second annotation set for a sorted random subset of 4885 videos)
    keep = np.sort(rng.permutation(n)[:4885])
    g2 = torch.nn.functional.normalize(g[torch.from_numpy(keep).to(dev)] + 0.05 * torch.randn(4885, 1024, device=dev))
    paras = torch.cat([g, g2])
    second = np.full(n, -1)
    second[keep] = n + np.arange(4885)
    lists = [[i] if second[i] < 0 else [i, int(second[i])] for i in range(n)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    case('val v2p', q, paras, off, np.concatenate(lists), args.reps, args.warmup)
    case('val p2v', paras, q, np.arange(9802 + 1), np.concatenate([np.arange(n), keep]), args.reps, args.warmup)
    del paras, g2
  if 'many' in args.cases:
    idx = rng.randint(0, n, size=(n, 20))
    idx[:, 0] = np.arange(n)
    case('many', q, g, 20 * np.arange(n + 1), idx.reshape(-1), args.reps, args.warmup)
  if 'all_f64' in args.cases:
    case('all_f64', q, g, np.arange(n + 1), np.arange(n), min(args.reps, 3), 1, scale=1 << 20)


if __name__ == '__main__':
  main()
