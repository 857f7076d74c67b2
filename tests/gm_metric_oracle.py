"""The normalised metrics of the geometric-median criterion (dcts_gm_distance_metric_f32): the float64 definition, an fp32
numpy restatement of what k_gm_stats and k_gm_distance<.., NORM> do, and the tolerance derived from the two. The inputs are
those of tests/gm_oracle.py.

Definition (float64). Every map x (the H * W elements of one channel of one sample) has a unit map u:
    cosine       u = x / ||x||                     flat (u = 0, every element +0.0) where sum x^2 == 0
    correlation  u = (x - mu) / ||x - mu||         flat where max(x) == min(x), an exact comparison
and the score is gm_oracle's on the unit maps: G[n, j] = sum_{k in the reference range} ||u[n, c_begin + j] - u[n, k]||.

The restatement does in float32 what the kernels do. The stats in the kernel's order: the elements in groups of four, group
q = p / 4 on lane q % 64, a chain per position in the group, (c0 + c1) + (c2 + c3), a xor tree over the 64 lanes; the centred
sum of squares in a second pass with a fused multiply-add; s = 1 / sqrt. The staging u = (x - mu) * s rounded once. Then
gm_oracle.gm_nc_f32 on the staged maps.

TOLERANCE. Absolute per reference channel: |got - f64| <= TOL[metric] * r_count. Every term lies in [0, 2] and near-duplicate
maps make single terms as small as one likes, so a relative bound is the wrong one here. R[metric] is the restatement's largest
|error| / r_count over the GPU tests' own inputs (gm_oracle.gpu_inputs() and the looping-lanes case), measured on a CPU with

    python tests/gm_metric_oracle.py

and TOL = 8 R (DESIGN.md section 5's convention). The inputs hold no map that is nearly constant without being flat, the one
thing fp32 centring is ill-conditioned for (include/dctscore.h names the limit).
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:  # run as a script
    sys.path.insert(0, _HERE)
import gm_oracle as go  # noqa: E402

METRICS = ("cosine", "correlation")
# measured with the command above (x86-64, numpy float32); the kernel's own worst error on an MI355X is in DESIGN.md 7i
# cosine: "C=200 15x17" sets it; correlation: the 72 x 72 case, whose 5184-element chains in
# gm_oracle.gm_nc_f32 run one after the other (the other inputs stay below 8.8e-7)
R = {"cosine": 8.001e-7, "correlation": 6.410e-6}
TOL = {m: 8 * r for m, r in R.items()}


def loop_case():
    """[2, 5, 72, 72]: 81 elements per lane of the stats kernel, 21 groups of four per lane."""
    return go.maps(2, 5, 72, 72, 7200)


# ----------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------
def unit_maps_f64(x, metric):
    """[N, C, H, W] float64 unit maps of a float32 tensor."""
    assert metric in METRICS, metric
    a = x.detach().cpu().numpy().astype(np.float64)
    flat = a.reshape(a.shape[0], a.shape[1], -1)
    if metric == "correlation":
        dead = flat.max(axis=-1) == flat.min(axis=-1)
        flat = flat - flat.mean(axis=-1, keepdims=True)
    else:
        dead = (flat * flat).sum(axis=-1) == 0
    norm = np.sqrt((flat * flat).sum(axis=-1))
    u = np.zeros_like(flat)
    live = ~dead
    u[live] = flat[live] / norm[live][:, None]
    return u.reshape(a.shape)


def gm_metric_nc_f64(x, metric, c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """The definition: numpy float64 [N, c_count]."""
    return go.gm_nc_f64(torch.from_numpy(unit_maps_f64(x, metric)), c_begin, c_count, ref_begin, ref_count)


def gm_metric_nc(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, out=None, metric="l2"):
    """ops.gm_distance_nc's signature on the CPU: the definition rounded to float32 (torch [N, c_count])."""
    if metric == "l2":
        return go.gm_nc(x, c_begin, c_count, ref_begin, ref_count)
    return torch.from_numpy(gm_metric_nc_f64(x, metric, c_begin, c_count, ref_begin, ref_count).astype(np.float32))


# ----------------------------------------------------------------------------------------------------
# the fp32 restatement of the kernels' order
# ----------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """float32 fma: the float64 product of two float32 is exact, the sum is rounded twice in rare ties only."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_tree(lanes, op=np.add):
    """[M, 64] -> [M]: v += v[lane ^ off] for off = 32 ... 1; every lane ends with the same value."""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = op(lanes, lanes[:, idx ^ off])
    assert (lanes == lanes[:, :1]).all() or np.isnan(lanes).any()
    return lanes[:, 0]


def stats_f32(x, metric):
    """(mu, s), float32 [N, C] each, in k_gm_stats's order."""
    assert metric in METRICS, metric
    a = x.detach().cpu().numpy().astype(np.float32)
    N, C = a.shape[:2]
    v = a.reshape(N * C, -1)
    hw = v.shape[1]
    iters = -(-hw // 256)
    pad = np.zeros((N * C, iters * 256), np.float32)
    pad[:, :hw] = v
    live = np.zeros(iters * 256, bool)
    live[:hw] = True
    pad, live = pad.reshape(N * C, iters, 64, 4), live.reshape(iters, 64, 4)  # [map, step, lane, position in the group]

    def reduce(term):
        c = np.zeros((N * C, 64, 4), np.float32)
        for t in range(iters):
            c = np.where(live[t], term(pad[:, t], c), c)
        return _wave_tree((c[:, :, 0] + c[:, :, 1]) + (c[:, :, 2] + c[:, :, 3]))

    mu = np.zeros(N * C, np.float32)
    dead = np.zeros(N * C, bool)
    if metric == "correlation":
        mu = reduce(lambda e, c: c + e) / np.float32(hw)
        dead = v.max(axis=1) == v.min(axis=1)
    ss = reduce(lambda e, c: _fma(e - mu[:, None, None], e - mu[:, None, None], c))
    dead = dead | (ss == 0)
    with np.errstate(divide="ignore"):
        s = np.where(dead, np.float32(0), np.float32(1) / np.sqrt(ss)).astype(np.float32)
    assert mu.dtype == np.float32 and s.dtype == np.float32
    return mu.reshape(N, C), s.reshape(N, C)


def staged_f32(x, metric):
    """The unit maps as k_gm_distance<.., NORM> stages them: float32 (x - mu) * s + 0 (torch [N, C, H, W])."""
    mu, s = stats_f32(x, metric)
    a = x.detach().cpu().numpy().astype(np.float32)
    u = (a - mu[:, :, None, None]) * s[:, :, None, None] + np.float32(0)
    assert u.dtype == np.float32
    return torch.from_numpy(u)


def gm_metric_nc_f32(x, metric, c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    return go.gm_nc_f32(staged_f32(x, metric), c_begin, c_count, ref_begin, ref_count)


# ----------------------------------------------------------------------------------------------------
# inputs and the error measure
# ----------------------------------------------------------------------------------------------------
def gpu_inputs():
    """(name, x, ranges): every input tests/test_gm_metric_gpu.py compares with the definition."""
    for item in go.gpu_inputs():
        yield item
    yield "loop 72x72", loop_case(), (0, None, 0, None)


def r_count_of(x, ranges):
    return x.shape[1] - ranges[2] if ranges[3] is None else ranges[3]


def error_per_reference(got, ref, r_count):
    """max |got - ref| / r_count."""
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max()) / r_count


def restatement_error(x, metric, ranges=(0, None, 0, None)):
    return error_per_reference(gm_metric_nc_f32(x, metric, *ranges), gm_metric_nc_f64(x, metric, *ranges), r_count_of(x, ranges))


def measure(metric, verbose=False, small_only=False):
    worst = 0.0
    for name, x, ranges in gpu_inputs():
        if small_only and x.shape[2] * x.shape[3] > 64:
            continue
        err = restatement_error(x, metric, ranges)
        worst = max(worst, err)
        if verbose:
            print("%-12s %-16s %-18s err / r_count %.3e" % (metric, name, tuple(x.shape), err))
    return worst


if __name__ == "__main__":
    for m in METRICS:
        r = measure(m, verbose=True)
        print("%s: r = %.3e   8 r = %.3e   (R = %.3e in this file)" % (m, r, 8 * r, R[m]))
