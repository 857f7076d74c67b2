#!/usr/bin/env python3
"""The geometric-median kernel (k_gm_distance, gm.hip) at the hook shapes of ResNet-50 at batch 256 and at U2-Net-p's
64 x 288 x 288 at batch 12: every call scores all channels of a post-ReLU normal tensor against all of them and is timed
with a pair of HIP events on the launch stream; the median of --reps calls (default 21) after two warm-up calls is
reported. One JSON line per shape.

The kernel is compute-bound (every element loaded is used against 64 maps), so the input is one buffer, not rotated.
pair_elems = N * C * C * H * W element pairs per call; each costs two fp32 VALU operations in the difference form (a
subtract and a fused multiply-add): valu_ops = 2 * pair_elems. Reported: pair elements per second, and valu_ops per second
as a share of the 157.3e12 of the MI355X's fp32 vector peak. That peak counts a packed fma as four operations (two lanes'
multiply and add): one operation (a subtract or an fma) per lane and clock is 39.3e12 per second at 2.4 GHz, a share of 0.25.
--metric cosine | correlation times the normalised call (dcts_gm_distance_metric_f32): the stats launch that reads every map
twice and the distance kernel that stages unit maps; pair_elems and the shares count the distance kernel's arithmetic alone.
--pairs times the pair-matrix call (dcts_gm_pairs_f32, gm_pairs.hip: the same inner loop, every distance kept and summed over
the samples) and, alternating with it call by call in the same session, the row-sum call on the same tensor; one JSON line
per shape holds both medians and their ratio. The pair-matrix call's launches (the stats of a metric, the kernel, the sum over
the slices where there are several) are all inside its event pair. --lib PATH loads another build of the library, e.g. one
compiled with -DDCTS_GM_PAIRS_ONE_SLICE, to measure the slice rule against no slicing.
usage: tools/microbench_gm.py [--reps R] [--metric M] [--pairs] [--lib PATH] [N,C,H,W ...]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dct_pruning_amd as dpa  # noqa: E402

SHAPES = [(256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7), (12, 64, 288, 288)]
PEAK_FP32_VECTOR = 157.3e12
WARMUP = 2


def run(shape, reps, metric):
    n, c, h, w = shape
    x = torch.relu(torch.randn(n, c, h, w, device="cuda"))
    out = torch.empty(n, c, device="cuda")
    for _ in range(WARMUP):
        dpa.gm_distance_nc(x, out=out, metric=metric)
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dpa.gm_distance_nc(x, out=out, metric=metric)
        z.record()
        pairs.append((a, z))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(z) for a, z in pairs)  # ms
    med = ts[len(ts) // 2]
    pair_elems = n * c * c * h * w
    workgroups = n * -(-c // 64)
    res = {"shape": list(shape), "metric": metric, "reps": reps, "workgroups": workgroups, "median_ms": round(med, 3), "min_ms": round(ts[0], 3),
           "max_ms": round(ts[-1], 3), "pair_elems": pair_elems, "pair_elems_per_s": round(pair_elems / med * 1e3, 1),
           "valu_ops_per_s": round(2 * pair_elems / med * 1e3, 1),
           "share_of_fp32_vector_peak": round(2 * pair_elems / med * 1e3 / PEAK_FP32_VECTOR, 4),
           "input_gbps": round(x.numel() * 4 / med / 1e6, 1)}
    print(json.dumps(res), flush=True)


def _timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    return a, z


def run_pairs(shape, reps, metric):
    from dct_pruning_amd import _lib
    n, c, h, w = shape
    x = torch.relu(torch.randn(n, c, h, w, device="cuda"))
    out, mat = torch.empty(n, c, device="cuda"), torch.empty(c, c, device="cuda")
    calls = {"pairs": lambda: dpa.gm_pair_matrix(x, metric=metric, out=mat), "rows": lambda: dpa.gm_distance_nc(x, out=out, metric=metric)}
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for _ in range(reps):  # alternating: both see the same clocks and the same neighbours
        for k, fn in calls.items():
            events[k].append(_timed(fn))
    torch.cuda.synchronize()
    med, lo, hi = {}, {}, {}
    for k, ev in events.items():
        ts = sorted(a.elapsed_time(z) for a, z in ev)
        med[k], lo[k], hi[k] = ts[len(ts) // 2], ts[0], ts[-1]
    pair_elems = n * c * c * h * w
    slices = _lib.load().dcts_gm_pairs_slices(n, c)
    res = {"shape": list(shape), "metric": metric, "reps": reps, "slices": slices, "workgroups": slices * (-(-c // 64)) ** 2,
           "rows_workgroups": n * -(-c // 64), "lib": os.path.basename(_lib.LIB_PATH),
           "pairs_median_ms": round(med["pairs"], 3), "pairs_min_ms": round(lo["pairs"], 3), "pairs_max_ms": round(hi["pairs"], 3),
           "rows_median_ms": round(med["rows"], 3), "rows_min_ms": round(lo["rows"], 3), "rows_max_ms": round(hi["rows"], 3),
           "pair_elems": pair_elems, "pairs_pair_elems_per_s": round(pair_elems / med["pairs"] * 1e3, 1),
           "rows_pair_elems_per_s": round(pair_elems / med["rows"] * 1e3, 1),
           "pairs_rate_over_rows_rate": round(med["rows"] / med["pairs"], 4),
           "pairs_share_of_fp32_vector_peak": round(2 * pair_elems / med["pairs"] * 1e3 / PEAK_FP32_VECTOR, 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--metric", default="l2", choices=("l2", "cosine", "correlation"))
    ap.add_argument("--pairs", action="store_true", help="time the pair-matrix call, alternating with the row-sum call")
    ap.add_argument("--lib", default=None, help="another build of libdctscore.so to load")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    if a.lib:
        from dct_pruning_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    for s in [tuple(int(v) for v in s.split(",")) for s in a.shapes] or SHAPES:
        (run_pairs if a.pairs else run)(s, a.reps, a.metric)
