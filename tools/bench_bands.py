#!/usr/bin/env python3
"""The fused band kernel (dcts_band_energy_f32) against the plain energy and against the only earlier way to the same
numbers: one JSON line per (shape, K) with

  band_ms       (a) band_energy_nc, K one-hot "square" bands, fused kernel
  energy_ms     (b) energy_nc on the same tensor
  weighted_ms   (c) K calls of weighted_energy_nc, one per band (two launches per sample and call, coefficients written
                to the workspace and read back)
  *_spread      (max - min) / median over the timed launches
  a_over_b      band_ms / energy_ms: the price of the K accumulators and of the weight reads
  c_over_a      weighted_ms / band_ms: what the fused kernel buys
  band_gbs      bytes of x streamed per second by (a), GB/s

Method: every timed launch reads a different one of --buffers tensors (together well past the 256 MB last-level
cache, so no launch finds its input cached), HIP events around single launches, medians. Shapes: ResNet-50's
56 / 28 / 14 / 7 stages at batch 256 and the CIFAR nets' 32 / 16 / 8 (batch scaled so a tensor is 100-200 MB; --scale
shrinks every batch for a quick run).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dct_pruning_amd as dpa  # noqa: E402
from dct_pruning_amd import bands  # noqa: E402

SHAPES = [(256, 256, 56), (256, 512, 28), (256, 1024, 14), (256, 2048, 7), (2048, 64, 32), (4096, 128, 16), (8192, 256, 8)]


def timed(fns, reps):
    """One HIP-event pair per launch; launch i runs fns[i % len(fns)]. Returns the list of milliseconds."""
    out = []
    for i in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fns[i % len(fns)]()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return out


def stats(ms):
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--weighted-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size by this")
    ap.add_argument("--ks", type=str, default="1,4,8")
    ap.add_argument("--skip-weighted", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bands.py needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    for N, C, H in SHAPES:
        N = max(1, int(N * args.scale))
        xs = [torch.relu(torch.randn(N, C, H, H, device=dev, generator=g)) for _ in range(args.buffers)]
        nbytes = xs[0].numel() * 4
        for _ in range(args.warmup):
            dpa.energy_nc(xs[0])
        e_ms, e_sp = stats(timed([lambda x=x: dpa.energy_nc(x) for x in xs], args.reps))
        for K in [int(k) for k in args.ks.split(",")]:
            w = torch.from_numpy(bands.partition(H, H, K, "square")).to(dev)
            for _ in range(args.warmup):
                dpa.band_energy_nc(xs[0], w, algo=dpa.ALGO_CODELET)
            b_ms, b_sp = stats(timed([lambda x=x: dpa.band_energy_nc(x, w, algo=dpa.ALGO_CODELET) for x in xs], args.reps))
            line = {"shape": [N, C, H, H], "K": K, "mbytes": round(nbytes / 1e6, 1), "band_ms": round(b_ms, 4),
                    "band_spread": round(b_sp, 3), "energy_ms": round(e_ms, 4), "energy_spread": round(e_sp, 3),
                    "a_over_b": round(b_ms / e_ms, 2), "band_gbs": round(nbytes / b_ms / 1e6, 1)}
            if not args.skip_weighted:
                def k_calls(x):
                    for b in range(K):
                        dpa.weighted_energy_nc(x, w[b])
                k_calls(xs[0])
                w_ms, w_sp = stats(timed([lambda x=x: k_calls(x) for x in xs], args.weighted_reps))
                line.update(weighted_ms=round(w_ms, 3), weighted_spread=round(w_sp, 3), c_over_a=round(w_ms / b_ms, 1))
            print(json.dumps(line), flush=True)
        del xs


if __name__ == "__main__":
    main()
