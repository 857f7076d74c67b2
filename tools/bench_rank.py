#!/usr/bin/env python3
"""The rank criterion (dcts_rank_f32) at every hooked shape of the ResNet-50 and CIFAR schedules: one JSON line per
distinct [N, C, H, W] with

  ms            kernel time per launch (HIP events, mean of --reps launches after --warmup)
  mmaps_s       maps per second / 1e6
  gflops_f64    fp64 GFLOP/s under the flop model  2 m n^2 (Gram)  +  4 n^3 / 3 (tridiagonalisation)  per map,
                n = min(H, W), m = max(H, W) (the Sturm counts are not counted)
  torch_ms      torch.linalg.matrix_rank on the same GPU tensor, on the first torch_maps maps (capped at
                --torch-cap: the batched SVD is slow), one timed call after one warm-up call
  speedup       per-map time of torch.linalg.matrix_rank / per-map time of the kernel
  agree         fraction of the capped subset on which the two ranks agree (maps near the threshold may differ)

N is chosen per shape so that a launch holds about --maps maps (ResNet-50's batch 64 at 56 x 56).
"""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dct_pruning_amd as dpa  # noqa: E402
from dct_pruning_amd import schedules  # noqa: E402


def shapes():
    seen = {}
    for net in ("resnet_50", "vgg_16_bn", "resnet_56", "resnet_110", "densenet_40", "googlenet"):
        for p in schedules.SCHEDULES[net]():
            c = schedules.scored_shape(p)[1]
            seen.setdefault((c, p.H, p.W), (net, p.C))
    return [(net, C, H, W, c) for (c, H, W), (net, C) in sorted(seen.items(), key=lambda kv: (-kv[0][1], kv[0][0]))]


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", type=int, default=16384, help="maps per launch (N = maps / C, at least 1)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-cap", type=int, default=2048, help="maps given to torch.linalg.matrix_rank")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank.py needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for net, C, H, W, c in shapes():
        N = max(1, args.maps // c)
        x = torch.relu(torch.randn(N, C, H, W, device=dev, generator=g))
        c0 = C - c
        out = torch.empty(N, c, device=dev)
        for _ in range(args.warmup):
            dpa.rank_nc(x, c0, c, out=out)
        ms = timed(lambda: dpa.rank_nc(x, c0, c, out=out), args.reps)
        maps = N * c
        n, m = min(H, W), max(H, W)
        flops = maps * (2.0 * m * n * n + 4.0 * n ** 3 / 3.0)
        sub = x[:, c0:].reshape(-1, H, W)[:args.torch_cap]
        torch.linalg.matrix_rank(sub)
        torch.cuda.synchronize()
        tms = timed(lambda: torch.linalg.matrix_rank(sub), 1)
        ref = torch.linalg.matrix_rank(sub).float()
        ours = dpa.rank_nc(x, c0, c).reshape(-1)[:sub.shape[0]]
        line = {"shape": [N, C, H, W], "net": net, "c_count": c, "maps": maps, "ms": round(ms, 4),
                "mmaps_s": round(maps / ms / 1e3, 3), "gflops_f64": round(flops / ms / 1e6, 1),
                "torch_ms": round(tms, 3), "torch_maps": sub.shape[0],
                "speedup": round((tms / sub.shape[0]) / (ms / maps), 1),
                "agree": round((ref == ours).float().mean().item(), 4)}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
