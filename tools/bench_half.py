#!/usr/bin/env python3
"""The native fp16 / bf16 energy kernel (dcts_energy_typed) against the only earlier way to score a half-precision
feature map, and against the fp32 kernel: one JSON line per (shape, dtype) with

  half_ms       (a) energy_nc(x_half): the native kernel reads the 2-byte elements
  upcast_ms     (b) energy_nc(x_half.float()): what a caller had to do before, the upcast inside the timed region
  fp32_ms       (c) energy_nc on an fp32 tensor of the same shape
  *_spread      (max - min) / median over the timed launches
  b_over_a      upcast_ms / half_ms: what the native kernel buys; `wins` says whether (a) beats (b) by more than the
                larger of the two spreads (in ms)
  a_over_c      half_ms / fp32_ms: the same maps for half the bytes
  half_gbs      bytes of x_half streamed per second by (a), GB/s;  mmaps_s: maps per second of (a), millions

Method: every timed launch reads a different one of --buffers tensors (together well past the 256 MB last-level cache,
so no launch finds its input cached), one HIP-event pair per launch, medians and spreads. Shapes: the native edges at
the hooked shapes of ResNet-50 (56 / 28 / 14 / 7) and of the CIFAR nets (32 / 16 / 8 / 4 / 2), batch scaled so that a
tensor has about 100 M elements (--scale shrinks every batch for a quick run). Every shape is measured in a child
process of its own under `timeout`; the first child that fails ends the run.
--lib PATH measures another build of libdctscore.so (a variant of the load path under development); `load` labels the
lines.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 256, 56), (256, 512, 28), (512, 1024, 14), (1024, 2048, 7), (1024, 96, 32), (2048, 192, 16),
          (4096, 384, 8), (16384, 512, 4), (32768, 512, 2)]
DTYPES = ("fp16", "bf16")


def timed(fns, reps):
    """One HIP-event pair per launch; launch i runs fns[i % len(fns)]. Returns the list of milliseconds."""
    import torch
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


def measure(args, index):
    import torch
    from dct_pruning_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import dct_pruning_amd as dpa
    if not torch.cuda.is_available():
        raise SystemExit("bench_half.py needs a GPU")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(index)
    N, C, H = SHAPES[index]
    N = max(1, int(N * args.scale))
    assert dpa.has_half_kernel(H, H)
    x32 = [torch.relu(torch.randn(N, C, H, H, device=dev, generator=g)) for _ in range(args.buffers)]
    for _ in range(args.warmup):
        dpa.energy_nc(x32[0])
    c_ms, c_sp = stats(timed([lambda x=x: dpa.energy_nc(x) for x in x32], args.reps))
    for dt in DTYPES:
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dt]
        xh = [x.to(dtype) for x in x32]
        for _ in range(args.warmup):
            dpa.energy_nc(xh[0])
            dpa.energy_nc(xh[0].float())
        # (a) and (b) alternate, so that a drift of the clock hits both
        a_all, b_all = [], []
        for _ in range(args.rounds):
            a_all += timed([lambda x=x: dpa.energy_nc(x) for x in xh], args.reps)
            b_all += timed([lambda x=x: dpa.energy_nc(x.float()) for x in xh], args.reps)
        a_ms, a_sp = stats(a_all)
        b_ms, b_sp = stats(b_all)
        same = torch.equal(dpa.energy_nc(xh[0]), dpa.energy_nc(xh[0].float()))
        nbytes = xh[0].numel() * 2
        print(json.dumps({
            "load": args.load, "dtype": dt, "shape": [N, C, H, H], "maps": N * C, "mbytes_half": round(nbytes / 1e6, 1),
            "half_ms": round(a_ms, 4), "half_spread": round(a_sp, 3), "upcast_ms": round(b_ms, 4),
            "upcast_spread": round(b_sp, 3), "fp32_ms": round(c_ms, 4), "fp32_spread": round(c_sp, 3),
            "b_over_a": round(b_ms / a_ms, 2), "a_over_c": round(a_ms / c_ms, 3),
            "wins": bool(b_ms - a_ms > max(a_sp * a_ms, b_sp * b_ms)),
            "half_gbs": round(nbytes / a_ms / 1e6, 1), "mmaps_s": round(N * C / a_ms / 1e3, 1),
            "bit_equal_to_upcast_route": bool(same)}), flush=True)
        del xh


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size by this")
    ap.add_argument("--lib", type=str, default=None, help="another build of libdctscore.so to measure")
    ap.add_argument("--load", type=str, default="2byte", help="label of the load path the library was built with")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--shape", type=int, default=None, help="(internal) measure SHAPES[i] in this process")
    args = ap.parse_args(argv)
    if args.shape is not None:
        return measure(args, args.shape)
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--shape", str(i)]
        cmd += [a for a in (argv if argv is not None else sys.argv[1:])]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("bench_half.py: shape %s ended with status %d; nothing more is started" % (SHAPES[i], rc))


if __name__ == "__main__":
    main()
