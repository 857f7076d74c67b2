#!/usr/bin/env python3
"""The low-pass signature pass (dcts_dct2d_lowpass_f32, lowpass.hip) against the energy pass on the same bytes, and what it
buys the geometric-median criterion: at the 56 x 56 and 28 x 28 hook shapes of ResNet-50 at batch 256 and at U2-Net-p's
64 x 288 x 288 at batch 12.

Per shape, in one process: lowpass_nc (K, --drop_dc) and energy_nc alternate call by call over buffers rotated past the
256 MiB Infinity Cache; every call is timed with a pair of HIP events on the launch stream; the median of --reps calls
(default 21) after two warm-up calls each is reported, as GB/s of input read and as a share of the 8000 GB/s HBM peak.
energy_nc reads the same bytes (through the same two-pass schedule where the edge has a codelet), so it is the yardstick.
Then gm_distance_nc with lowpass=K and with lowpass=0 alternate on one of the buffers (the plain kernel is compute-bound: one
buffer, as tools/microbench_gm.py has it); the low-pass call's launches (signatures, then the distances on them) are all
inside its event pair. One JSON line per shape.
--chains times lowpass_nc alone, on an output that lies on a 16-byte boundary against one 4 bytes past it, alternating call by
call: with K a multiple of 4 the first takes the kernel's 16-byte store chain and the second its dword chain, in one binary.
--lib PATH loads another build of the library (a development build of another epilogue, to compare as alternating processes).
usage: tools/microbench_lowpass.py [--reps R] [--K K] [--drop_dc] [--no_gm] [--chains] [--lib PATH] [N,C,H,W ...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dct_pruning_amd as dpa  # noqa: E402

SHAPES = [(256, 256, 56, 56), (256, 512, 28, 28), (12, 64, 288, 288)]
HBM_PEAK_GBS = 8000.0
WORKING_SET = 1200e6  # rotated buffers: several times the Infinity Cache
WARMUP = 2


def _timed(fn, *a):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(*a)
    e.record()
    return s, e


def _stats(events):
    ts = sorted(s.elapsed_time(e) for s, e in events)  # ms
    return ts[len(ts) // 2], ts[0], ts[-1]


def _alternate(calls, args, reps):
    """{name: (median, min, max) ms}: the calls alternate, call i of every name gets args(i)."""
    for i in range(WARMUP):
        for fn in calls.values():
            fn(*args(i))
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for i in range(reps):
        for j, (k, fn) in enumerate(calls.items()):
            events[k].append(_timed(fn, *args(len(calls) * i + j)))
    torch.cuda.synchronize()
    return {k: _stats(ev) for k, ev in events.items()}


def run_chains(shape, reps, K):
    from dct_pruning_amd import _lib
    n, c, h, w = shape
    nbytes = n * c * h * w * 4
    nbuf = max(2, int(-(-WORKING_SET // nbytes)))
    bufs = [torch.relu(torch.randn(n, c, h, w, device="cuda")) for _ in range(nbuf)]
    oshape = (n, c, min(K, h), min(K, w))
    numel = oshape[0] * oshape[1] * oshape[2] * oshape[3]
    flat = torch.empty(numel + 4, device="cuda")
    assert flat.data_ptr() % 16 == 0
    outs = {"aligned16": flat[:numel].view(oshape), "offset4": flat[1:numel + 1].view(oshape)}
    t = _alternate({k: (lambda b, o=o: dpa.lowpass_nc(b, K, out=o)) for k, o in outs.items()}, lambda i: (bufs[i % nbuf],), reps)
    res = {"lib": os.path.basename(_lib.LIB_PATH), "shape": list(shape), "K": K, "reps": reps, "buffers": nbuf, "input_bytes": nbytes}
    for k, (med, lo, hi) in t.items():
        res[k + "_median_ms"], res[k + "_min_ms"], res[k + "_max_ms"] = round(med, 3), round(lo, 3), round(hi, 3)
    res["offset4_over_aligned16"] = round(t["offset4"][0] / t["aligned16"][0], 3)
    print(json.dumps(res), flush=True)


def run(shape, reps, K, drop_dc, with_gm):
    n, c, h, w = shape
    nbytes = n * c * h * w * 4
    nbuf = max(2, int(-(-WORKING_SET // nbytes)))
    bufs = [torch.relu(torch.randn(n, c, h, w, device="cuda")) for _ in range(nbuf)]
    sig = torch.empty(n, c, min(K, h), min(K, w), device="cuda")
    out = torch.empty(n, c, device="cuda")
    t = _alternate({"lowpass": lambda b: dpa.lowpass_nc(b, K, drop_dc=drop_dc, out=sig), "energy": lambda b: dpa.energy_nc(b, out=out)},
                   lambda i: (bufs[i % nbuf],), reps)
    from dct_pruning_amd import _lib
    res = {"lib": os.path.basename(_lib.LIB_PATH), "shape": list(shape), "K": K, "drop_dc": bool(drop_dc), "reps": reps,
           "buffers": nbuf, "input_bytes": nbytes,
           "fused": bool(dpa.has_codelet(h, w))}
    for k, (med, lo, hi) in t.items():
        res[k + "_median_ms"], res[k + "_min_ms"], res[k + "_max_ms"] = round(med, 3), round(lo, 3), round(hi, 3)
        res[k + "_gbps"] = round(nbytes / med / 1e6, 1)
        res[k + "_share_of_hbm_peak"] = round(nbytes / med / 1e6 / HBM_PEAK_GBS, 4)
    res["lowpass_rate_over_energy_rate"] = round(t["energy"][0] / t["lowpass"][0], 4)
    if with_gm:
        x = bufs[0]
        g = _alternate({"gm_lowpass": lambda: dpa.gm_distance_nc(x, out=out, lowpass=K), "gm_plain": lambda: dpa.gm_distance_nc(x, out=out)},
                       lambda i: (), reps)
        for k, (med, lo, hi) in g.items():
            res[k + "_median_ms"], res[k + "_min_ms"], res[k + "_max_ms"] = round(med, 3), round(lo, 3), round(hi, 3)
        res["gm_plain_over_gm_lowpass"] = round(g["gm_plain"][0] / g["gm_lowpass"][0], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--drop_dc", action="store_true")
    ap.add_argument("--no_gm", action="store_true", help="leave the gm_distance_nc comparison out")
    ap.add_argument("--chains", action="store_true", help="16-byte-aligned output against one 4 bytes past it")
    ap.add_argument("--lib", default=None, help="another build of libdctscore.so to load")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    if a.lib:
        from dct_pruning_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    for s in [tuple(int(v) for v in s.split(",")) for s in a.shapes] or SHAPES:
        if a.chains:
            run_chains(s, a.reps, a.K)
        else:
            run(s, a.reps, a.K, a.drop_dc, not a.no_gm)
