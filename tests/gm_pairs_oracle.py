"""The pair matrix of the geometric-median criterion (dcts_gm_pairs_f32): the definition it is tested against, an fp32
restatement of the kernel's order, the inputs of tests/test_gm_pairs_gpu.py, and the tolerances derived from them.

Definition (float64):  D[j, k] = sum_n d(x[n, c_begin + j], x[n, ref_begin + k]):  gm_oracle.pair_distances_f64(...).sum(0),
and under a metric the same on the float64 unit maps of tests/gm_metric_oracle.py.

The restatement (pair_matrix_f32) does in float32 what the kernels do: the staged maps (the maps themselves, or
gm_metric_oracle.staged_f32's unit maps), per pair the squared differences added one after the other with p ascending, sqrt,
the samples of a slice added one after the other with n ascending, the slices added one after the other with s ascending. The
slices are those of slices(N, r_count), the rule of grid_caps.h restated (tests/test_gm_pairs_cpu.py holds it against the
library's dcts_gm_pairs_slices).

TOLERANCES, measured on a CPU with

    python tests/gm_pairs_oracle.py

which prints the restatement's error against float64 per GPU-test input and the maximum R per metric; the kernel gets
TOL = 8 R (DESIGN.md section 5's convention: room for the kernel's two fused chains per pair and a sqrtf an ulp off).
  l2           relative, per entry: every term of an entry is non-negative, so nothing cancels;
  cosine, correlation   absolute per sample, |got - f64| <= TOL * N: every term lies in [0, 2], and near-duplicate unit maps
               make single terms as small as one likes (gm_metric_oracle.py has the same rule per reference channel).
Where the definition is 0 the restatement and the kernel must give 0: for l2 everywhere, under a metric wherever the two maps
are identical in every sample (exact_zeros says why not on every float64 zero).
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:  # run as a script
    sys.path.insert(0, _HERE)
import gm_metric_oracle as mo  # noqa: E402
import gm_oracle as go  # noqa: E402

METRICS = ("l2", "cosine", "correlation")
# measured with the command above (x86-64, numpy float32). "ragged" sets all three: 1025 samples per entry, 513 slices added
# one after the other (the other inputs stay below 4e-7, 4e-7 and 9.6e-7)
R = {"l2": 1.218e-6, "cosine": 1.206e-6, "correlation": 1.424e-6}
TOL = {m: 8 * r for m, r in R.items()}

PAIR_TARGET, TILE = 4096, 64  # kGmPairTarget, kGmTR (grid_caps.h)

N = 3
CHANNELS = (1, 2, 3, 12, 33, 64, 65, 129, 200)
SIZES = ((1, 1), (7, 7), (5, 13), (8, 8), (15, 17))
# C number i takes the sizes 3 i, 3 i + 1, 3 i + 2 (mod 5): three sizes per C, every size at least five C
SWEEP = tuple((c, SIZES[(3 * i + k) % len(SIZES)]) for i, c in enumerate(CHANNELS) for k in range(3))
ZERO_SAMPLE_CASE = (33, (15, 17))  # the sweep case whose sample 1 is all zeros
# (name, N, C, (H, W)) of the three slice regimes: S = N, 1 < S < N with a shorter last slice, S = 1
REGIMES = (("S=N", 5, 3, (4, 4)), ("ragged", 1025, 65, (2, 2)), ("S=1", 2, 2945, (1, 1)))


def slices(n, r_count):
    """dcts_gm_pairs_slices: S = clamp(PAIR_TARGET / ceil(r_count / 64)^2, 1, N), then the slices of ceil(N / S) samples that
    hold one. 0 for arguments it cannot take."""
    if n <= 0 or r_count <= 0:
        return 0
    rt = -(-r_count // TILE)
    s = min(max(PAIR_TARGET // (rt * rt), 1), n)
    per = -(-n // s)
    return -(-n // per)


def slice_bounds(n, r_count):
    """[(n0, n1), ...]: slice s is the samples [s * ceil(N / S), ...)."""
    s = slices(n, r_count)
    per = -(-n // s)
    return [(k * per, min(n, (k + 1) * per)) for k in range(s)]


# ----------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------
def pair_matrix_f64(x, metric="l2", c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """numpy float64 [c_count, ref_count]."""
    assert metric in METRICS, metric
    u = x if metric == "l2" else torch.from_numpy(mo.unit_maps_f64(x, metric))
    return go.pair_distances_f64(u, c_begin, c_count, ref_begin, ref_count).sum(axis=0)


def pair_matrix(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, metric="l2", out=None):
    """ops.gm_pair_matrix's signature on the CPU: the definition rounded to float32 (torch [c_count, ref_count])."""
    return torch.from_numpy(pair_matrix_f64(x, metric, c_begin, c_count, ref_begin, ref_count).astype(np.float32))


# ----------------------------------------------------------------------------------------------------
# the fp32 restatement of the kernels' order
# ----------------------------------------------------------------------------------------------------
def pair_matrix_f32(x, metric="l2", c_begin=0, c_count=None, ref_begin=0, ref_count=None, bounds=None):
    """Every step in float32, one after the other (numpy float32 [c_count, ref_count]). bounds: the sample slices, by default
    those of the rule."""
    assert metric in METRICS, metric
    a = go._flat(x if metric == "l2" else mo.staged_f32(x, metric), np.float32)
    cb, cc, rb, rc = go._ranges(a.shape[1], c_begin, c_count, ref_begin, ref_count)
    s, ref = a[:, cb:cb + cc], a[:, rb:rb + rc]
    acc = np.zeros((a.shape[0], cc, rc), np.float32)
    for p in range(a.shape[2]):
        d = s[:, :, None, p] - ref[:, None, :, p]
        acc += d * d
    dist = np.sqrt(acc)
    total = None
    for n0, n1 in (slice_bounds(a.shape[0], rc) if bounds is None else bounds):
        part = np.zeros((cc, rc), np.float32)
        for n in range(n0, n1):
            part += dist[n]
        total = part if total is None else total + part
    assert dist.dtype == np.float32 and total.dtype == np.float32
    return total


# ----------------------------------------------------------------------------------------------------
# the inputs of tests/test_gm_pairs_gpu.py
# ----------------------------------------------------------------------------------------------------
def sweep_case(c, hw):
    x = go.maps(N, c, hw[0], hw[1], 200000 + 1000 * c + 31 * hw[0] + hw[1])
    if (c, hw) == ZERO_SAMPLE_CASE:
        x[1] = 0
    return x


def regime_case(name):
    for nm, n, c, hw in REGIMES:
        if nm == name:
            return go.maps(n, c, hw[0], hw[1], 7300 + c)
    raise KeyError(name)


def integer_case(name):
    """The regime's shape with small-integer maps: every sum of squared differences is an integer below 2^24, exact in fp32 in
    any order, so the kernel and the restatement differ in nothing but the order of the sums over the samples."""
    x = regime_case(name)
    g = torch.Generator().manual_seed(7400 + x.shape[1])
    y = torch.randint(0, 8, x.shape, generator=g).float()
    y[:, -1] = y[:, 0]
    return y


def piece_case():
    """The unsplit tensor of the channel-range tests: [4, 77, 5, 13]."""
    return go.maps(4, 77, 5, 13, 7501)


def subrange_case():
    """[3, 67, 8, 8]: rows [5, 5 + 40) against the reference channels [3, 3 + 62)."""
    return go.maps(3, 67, 8, 8, 7503)


def view_case(h, w):
    """[4, 21, h, w]: the bank the view and the alignment tests cut."""
    return go.maps(4, 21, h, w, 7600 + h * w)


def duplicate_case():
    """DESIGN.md 7j's example: 12 channels, 6 patterns, each present twice (channel i + 6 is a copy of channel i)."""
    base = torch.relu(torch.randn(3, 6, 6, 5, generator=torch.Generator().manual_seed(901)))
    return torch.cat([base, base], 1)


def gpu_inputs():
    """(name, x, (c_begin, c_count, ref_begin, ref_count)): every input test_gm_pairs_gpu.py compares with the definition."""
    for c, hw in SWEEP:
        yield "C=%d %dx%d" % (c, hw[0], hw[1]), sweep_case(c, hw), (0, None, 0, None)
    for name, _, _, _ in REGIMES:
        yield name, regime_case(name), (0, None, 0, None)
    yield "pieces", piece_case(), (0, None, 0, None)
    yield "subrange", subrange_case(), (5, 40, 3, 62)
    for h, w in ((6, 6), (7, 7)):
        yield "views %dx%d" % (h, w), view_case(h, w), (0, None, 0, None)
    yield "duplicates", duplicate_case(), (0, None, 0, None)


def exact_zeros(x, metric, ranges=(0, None, 0, None)):
    """bool [c_count, ref_count]: the entries that must come out as 0. l2: wherever the definition is 0 (two maps differ in no
    element of any sample). Under a metric: the same pairs, identical maps in every sample, the diagonal among them. There
    float64 has further zeros that float32 arithmetic does not owe: every positive 1 x 1 map has the unit map 1 under the
    cosine, but x * (1 / sqrt(x * x)) is 1 only to an ulp; those entries are held to the tolerance like any other."""
    a = go._flat(x, np.float32)
    cb, cc, rb, rc = go._ranges(a.shape[1], *ranges)
    return (a[:, cb:cb + cc, None, :] == a[:, None, rb:rb + rc, :]).all(axis=(0, 3))


def error(got, ref, metric, n, zeros):
    """The measure the metric's tolerance bounds: l2 relative per entry, the unit-map metrics absolute per sample; inf if an
    entry of `zeros` (exact_zeros) is not 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if (got[zeros] != 0).any() or (ref[zeros] != 0).any():
        return float("inf")
    if metric == "l2":
        assert ((ref == 0) == zeros).all()
        return go.relative_error(got, ref)
    return float(np.abs(got - ref).max()) / n


def restatement_error(x, metric, ranges=(0, None, 0, None)):
    return error(pair_matrix_f32(x, metric, *ranges), pair_matrix_f64(x, metric, *ranges), metric, x.shape[0],
                 exact_zeros(x, metric, ranges))


def measure(metric, verbose=False, small_only=False):
    worst = 0.0
    for name, x, ranges in gpu_inputs():
        if small_only and x.shape[0] * x.shape[1] ** 2 * x.shape[2] * x.shape[3] > 3e6:
            continue
        err = restatement_error(x, metric, ranges)
        worst = max(worst, err)
        if verbose:
            print("%-12s %-16s %-18s err %.3e" % (metric, name, tuple(x.shape), err))
    return worst


if __name__ == "__main__":
    for m in METRICS:
        r = measure(m, verbose=True)
        print("%s: r = %.3e   8 r = %.3e   (R = %.3e in this file)" % (m, r, 8 * r, R[m]))
