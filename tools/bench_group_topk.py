#!/usr/bin/env python3
"""Group-wise top-K timings: ops.group_topk against ops.group_scores alone (the same exact-fp32 GEMM
with the block reduction, G stored) and against ops.group_scores + torch.topk (G through HBM, then
torch's selection) in the same run; HIP events around each call after warm-up, the median of --reps
calls.  One JSON line per shape, direction and K.

  val_1 shape   4917 videos, 17 502 clip rows x 17 502 caption rows x 1024, both directions,
                K = 1 / 10 / 50 / 128;
  rectangular   the 4917 val_1 paragraphs as queries against a gallery of --gallery_factor x as many
                videos (49 170 by default; no square G exists, so group_topk alone), with the
                workspace bytes beside the square case's: the workspace does not grow with the gallery.

  python tools/bench_group_topk.py [--reps 20] [--warmup 3] [--ks 1 10 50 128] [--reduce max]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cmhse_amd import _lib, ops, synthetic  # noqa: E402


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


def workspace_bytes(num_clips, num_caps, n_clip_rows, n_cap_rows, k, direction):
  plan = ops.group_topk_plan(num_clips, num_caps, n_clip_rows, n_cap_rows, k, direction)
  return int(_lib.load().cmhse_group_topk_workspace(plan.ctypes.data, plan.size))


def scores_then_topk(c, s, counts, k, direction, reduce):
  G = ops.group_scores(c, s, counts, counts, reduce=reduce)
  return torch.topk(G.t() if direction == 'p2v' else G, k, dim=1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--videos', type=int, default=4917)
  ap.add_argument('--ks', type=int, nargs='*', default=[1, 10, 50, 128])
  ap.add_argument('--reduce', default='max')
  ap.add_argument('--dim', type=int, default=1024)
  ap.add_argument('--gallery_factor', type=int, default=10)
  ap.add_argument('--rect_k', type=int, default=50)
  ap.add_argument('--skip_rect', action='store_true')
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  torch.cuda.set_device(dev)
  ops.set_math_mode('fp32')
  B = args.videos
  counts = [int(x) for x in synthetic.anet_like_spec(B).num_clips]
  n = sum(counts)
  a, b = synthetic.correlated_embeddings(n, args.dim, seed=0)
  c, s = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
  reduce = args.reduce
  scores_ms = timed(lambda: ops.group_scores(c, s, counts, counts, reduce=reduce), args.reps, args.warmup)
  for direction in ('p2v', 'v2p'):
    for k in args.ks:
      topk_ms = timed(lambda: ops.group_topk(c, s, counts, counts, k, direction, reduce), args.reps, args.warmup)
      torch_ms = timed(lambda: scores_then_topk(c, s, counts, k, direction, reduce), args.reps, args.warmup)
      print(json.dumps(dict(
          shape='square', videos=B, paragraphs=B, clips=n, caps=n, d=args.dim, reduce=reduce,
          direction=direction, k=k, reps=args.reps, group_topk_ms=round(topk_ms, 4),
          group_scores_ms=round(scores_ms, 4), group_scores_torch_topk_ms=round(torch_ms, 4),
          group_topk_vs_group_scores=round(topk_ms / scores_ms, 3),
          group_topk_vs_scores_torch_topk=round(topk_ms / torch_ms, 3),
          workspace_bytes=workspace_bytes(counts, counts, n, n, k, direction))), flush=True)
  if args.skip_rect:
    return
  # paragraphs of the val_1 shape against a gallery of gallery_factor x as many videos
  Bg = B * args.gallery_factor
  gcounts = [int(x) for x in synthetic.anet_like_spec(Bg, seed=1).num_clips]
  ng = sum(gcounts)
  gen = torch.Generator(device=dev)
  gen.manual_seed(5)
  gallery = torch.nn.functional.normalize(torch.randn(ng, args.dim, device=dev, generator=gen))
  k = args.rect_k
  ms = timed(lambda: ops.group_topk(gallery, s, gcounts, counts, k, 'p2v', reduce), args.reps, args.warmup)
  square_ms = timed(lambda: ops.group_topk(c, s, counts, counts, k, 'p2v', reduce), args.reps, args.warmup)
  print(json.dumps(dict(
      shape='rectangular', videos=Bg, paragraphs=B, clips=ng, caps=n, d=args.dim, reduce=reduce,
      direction='p2v', k=k, reps=args.reps, group_topk_ms=round(ms, 4),
      square_group_topk_ms=round(square_ms, 4), gallery_ratio=round(ng / n, 3),
      time_ratio=round(ms / square_ms, 3),
      workspace_bytes=workspace_bytes(gcounts, counts, ng, n, k, 'p2v'),
      square_workspace_bytes=workspace_bytes(counts, counts, n, n, k, 'p2v'),
      gflop=round(2.0 * ng * n * args.dim / 1e9, 1))), flush=True)


if __name__ == '__main__':
  main()
