#!/usr/bin/env python3
"""Labelled group-wise ranking timings: ops.group_rank_labelled (p2v and v2p, diagonal labels) against
ops.group_rank — one call of which serves both directions — on the val_1 shape: the 4917 videos /
paragraphs of synthetic.anet_like_spec(4917), 17 502 clip x 17 502 caption rows, D = 1024.  The calls are
ALTERNATED in one process; HIP events around each call after warm-up; median, minimum and maximum of
--reps calls.  One JSON line per reduce mode, then the device (its clocks: `rocm-smi --showclocks` beside the run).

`both_ms` is the sum of the two labelled medians, `vs_group_rank` that over group_rank's median: the
counting pass does the tile work of group_sim_kernel once per direction, so about 2 is the expected order.
The threshold pass and the counting pass are told apart in a separate
`rocprofv3 --kernel-trace --stats` run of this tool (group_label_threshold_kernel / group_label_count_kernel).

  python tools/bench_group_rank_labelled.py [--reps 20] [--warmup 3] [--videos 4917]
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

from cmhse_amd import _lib, ops, synthetic  # noqa: E402


def timed_alternating(fns, reps, warmup):
  """[(median, min, max) ms] of each fn, called in turn: a, b, c, a, b, c, ..."""
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--videos', type=int, default=4917)
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  counts = synthetic.anet_like_spec(args.videos).num_clips
  B, n = len(counts), sum(counts)
  a, b = synthetic.correlated_embeddings(n, 1024, seed=3)
  c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  diag = np.arange(B)
  lib = _lib.load()
  shape = {}
  for direction in ('p2v', 'v2p'):
    plan = ops.group_rank_labelled_plan(counts, counts, n, n, diag, direction)
    shape[direction] = dict(query_tiles=int(plan[6] if direction == 'p2v' else plan[5]),
                            gallery_tiles=int(plan[5] if direction == 'p2v' else plan[6]), pair_tiles=int(plan[8]),
                            workspace_bytes=int(lib.cmhse_group_rank_labelled_workspace(plan.ctypes.data, plan.size)))
  for reduce in ('max', 'mean'):
    fns = [lambda: ops.group_rank(c, s, counts, reduce=reduce),
           lambda: ops.group_rank_labelled(c, s, counts, counts, diag, 'p2v', reduce),
           lambda: ops.group_rank_labelled(c, s, counts, counts, diag, 'v2p', reduce)]
    t = timed_alternating(fns, args.reps, args.warmup)
    both = t[1][0] + t[2][0]
    print(json.dumps(dict(case='val_1 diagonal', videos=B, rows=n, d=1024, reduce=reduce, reps=args.reps,
                          group_rank_ms=r4(t[0]), labelled_p2v_ms=r4(t[1]), labelled_v2p_ms=r4(t[2]),
                          both_ms=round(both, 4), vs_group_rank=round(both / t[0][0], 3),
                          group_rank_workspace_bytes=int(lib.cmhse_group_rank_workspace(B)), plans=shape)),
          flush=True)
  props = torch.cuda.get_device_properties(dev)
  print(json.dumps(dict(device=props.name, compute_units=props.multi_processor_count)), flush=True)


if __name__ == '__main__':
  main()
