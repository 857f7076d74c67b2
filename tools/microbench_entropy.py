#!/usr/bin/env python3
"""What one logf per coefficient costs on top of the energy epilogue: the fused spectral-entropy kernel against the band
kernel with K = 1 (the same schedule and the same bytes) and the plain energy kernel, on the same inputs in one process.
Buffers rotate past the 256 MiB Infinity Cache, every call is timed with HIP events on the launch stream, the three
kernels alternate call by call, medians are reported. One JSON line per edge.
usage: tools/microbench_entropy.py [edge ...]   (default 56 28 14 8)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dct_pruning_amd as dpa  # noqa: E402

LAUNCH_BYTES = 400e6   # per launch: long enough that the enqueue of the next call hides behind it
WORKING_SET = 1200e6   # rotated buffers: several times the Infinity Cache
REPS = 21


def run(edge):
    nmaps = int(LAUNCH_BYTES // (edge * edge * 4))
    nbuf = max(3, int(WORKING_SET // (nmaps * edge * edge * 4)))
    bufs = [torch.relu(torch.randn(1, nmaps, edge, edge, device="cuda")) for _ in range(nbuf)]
    ones = torch.ones(1, edge, edge, device="cuda")
    out = torch.empty(1, nmaps, device="cuda")
    calls = {
        "entropy": lambda b: dpa.spectral_entropy_nc(b, algo=dpa.ALGO_CODELET, out=out),
        "band_k1": lambda b: dpa.band_energy_nc(b, ones, algo=dpa.ALGO_CODELET),
        "energy": lambda b: dpa.energy_nc(b, algo=dpa.ALGO_CODELET, out=out),
    }
    for f in calls.values():
        for b in bufs:
            f(b)
    torch.cuda.synchronize()
    ev = {k: [] for k in calls}
    for i in range(REPS):
        for j, (k, f) in enumerate(calls.items()):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f(bufs[(3 * i + j) % nbuf])
            z.record()
            ev[k].append((a, z))
    torch.cuda.synchronize()
    res = {"edge": edge, "maps": nmaps, "buffers": nbuf, "reps": REPS}
    by = nmaps * (4 * edge * edge + 4)
    for k, pairs in ev.items():
        ts = sorted(a.elapsed_time(z) for a, z in pairs)
        res[k + "_us"] = round(ts[len(ts) // 2] * 1e3, 1)
        res[k + "_min_us"] = round(ts[0] * 1e3, 1)
        res[k + "_gbps"] = round(by / ts[len(ts) // 2] / 1e6, 1)
    res["entropy_over_band_k1"] = round(res["entropy_us"] / res["band_k1_us"], 3)
    res["entropy_over_energy"] = round(res["entropy_us"] / res["energy_us"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    for e in [int(a) for a in sys.argv[1:]] or [56, 28, 14, 8]:
        run(e)
