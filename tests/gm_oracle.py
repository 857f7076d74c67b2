"""The geometric-median criterion on feature maps: the definition dcts_gm_distance_f32 is tested against, an fp32
restatement of the kernel's arithmetic (the yardstick for round-off), the inputs of tests/test_gm_gpu.py, and the tolerance
derived from them.

Definition (float64):  G[n, j] = sum_{k in the reference range} sqrt(sum_p (x[n, c_begin + j, p] - x[n, k, p])^2),
p over the H * W elements of a map, in the difference form.

The restatement (gm_nc_f32) does in float32 what the kernel does: float32 differences, their squares added one after the
other with p ascending, sqrt in float32, the distances added one after the other with k ascending.

TOLERANCE. It is relative: every term is non-negative, so nothing cancels. R is the largest |restatement - definition| /
definition over the GPU tests' own inputs (gpu_inputs()), measured on a CPU with

    python tests/gm_oracle.py

which prints the error per input and the maximum; the kernel gets TOL = 8 * R (DESIGN.md section 5's convention: room for
another accumulation order over p - the kernel fuses the multiply and the add - and over k - the kernel adds 16 lanes'
partial sums in a tree - and a sqrtf that differs by an ulp). tests/test_gm_cpu.py re-measures R on the small inputs and
checks that the constant below still covers them. Where the definition is 0 the restatement (and the kernel) must give 0.
"""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # run as a script
    sys.path.insert(0, _ROOT)

R = 1.241e-6     # measured with the command above: "C=128 1x1" sets it; 8 R = 9.928e-6
TOL = 8 * R

N = 3
CHANNELS = (1, 2, 3, 12, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
SIZES = ((1, 1), (2, 2), (7, 7), (7, 9), (8, 8), (5, 13), (14, 14), (15, 17), (16, 16), (1, 257), (25, 40))
# every C meets three map sizes and every map size at least three C: C number i takes sizes 3 i, 3 i + 1, 3 i + 2 (mod 11)
SWEEP = tuple((c, SIZES[(3 * i + k) % len(SIZES)]) for i, c in enumerate(CHANNELS) for k in range(3))
ZERO_SAMPLE_CASE = (33, (15, 17))  # the sweep case whose sample 1 is all zeros


# ----------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------
def _ranges(C, c_begin, c_count, ref_begin, ref_count):
    c_count = C - c_begin if c_count is None else c_count
    ref_count = C - ref_begin if ref_count is None else ref_count
    return int(c_begin), int(c_count), int(ref_begin), int(ref_count)


def _flat(x, dtype):
    a = x.detach().cpu().numpy().astype(dtype)
    return a.reshape(a.shape[0], a.shape[1], -1)


def pair_distances_f64(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """[N, c_count, ref_count] float64: the distance of every scored map to every reference map."""
    a = _flat(x, np.float64)
    cb, cc, rb, rc = _ranges(a.shape[1], c_begin, c_count, ref_begin, ref_count)
    out = np.empty((a.shape[0], cc, rc))
    for n in range(a.shape[0]):
        ref = a[n, rb:rb + rc]
        for j0 in range(0, cc, 16):
            s = a[n, cb + j0:cb + min(j0 + 16, cc)]
            d = s[:, None, :] - ref[None, :, :]
            out[n, j0:j0 + s.shape[0]] = np.sqrt((d * d).sum(axis=-1))
    return out


def gm_nc_f64(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """The definition: numpy float64 [N, c_count]."""
    return pair_distances_f64(x, c_begin, c_count, ref_begin, ref_count).sum(axis=-1)


def gm_nc(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, out=None):
    """ops.gm_distance_nc's signature on the CPU: the definition rounded to float32 (torch [N, c_count])."""
    return torch.from_numpy(gm_nc_f64(x, c_begin, c_count, ref_begin, ref_count).astype(np.float32))


# ----------------------------------------------------------------------------------------------------
# the fp32 restatement of the kernel's order
# ----------------------------------------------------------------------------------------------------
def gm_nc_f32(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """Every step in float32, one after the other (numpy float32 [N, c_count])."""
    a = _flat(x, np.float32)
    cb, cc, rb, rc = _ranges(a.shape[1], c_begin, c_count, ref_begin, ref_count)
    s, ref = a[:, cb:cb + cc], a[:, rb:rb + rc]
    acc = np.zeros((a.shape[0], cc, rc), np.float32)
    for p in range(a.shape[2]):
        d = s[:, :, None, p] - ref[:, None, :, p]
        acc += d * d
    dist = np.sqrt(acc)
    total = np.zeros((a.shape[0], cc), np.float32)
    for k in range(rc):
        total += dist[:, :, k]
    assert dist.dtype == np.float32 and total.dtype == np.float32
    return total


# ----------------------------------------------------------------------------------------------------
# the inputs of tests/test_gm_gpu.py
# ----------------------------------------------------------------------------------------------------
def maps(n, c, h, w, seed):
    """[n, c, h, w] post-ReLU normal maps with, where c allows, channel 1 all zeros (c >= 3) and the last channel a copy of
    channel 0 (c >= 2)."""
    x = torch.relu(torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed)))
    if c >= 3:
        x[:, 1] = 0
    if c >= 2:
        x[:, c - 1] = x[:, 0]
    return x


def sweep_case(c, hw):
    x = maps(N, c, hw[0], hw[1], 100000 + 1000 * c + 31 * hw[0] + hw[1])
    if (c, hw) == ZERO_SAMPLE_CASE:
        x[1] = 0
    return x


def piece_case():
    """The unsplit tensor of the channel-range tests: [2, 77, 5, 13]."""
    return maps(2, 77, 5, 13, 7001)


def batch_case():
    """[5, 70, 7, 7]: sample 3 on its own must give the bits it gives here."""
    return maps(5, 70, 7, 7, 7002)


def subrange_case():
    """[2, 67, 8, 8]: scored against the reference channels [3, 3 + 62)."""
    return maps(2, 67, 8, 8, 7003)


def view_case(h, w):
    """[4, 21, h, w]: the bank the view tests cut (h * w a multiple of 4 and not)."""
    return maps(4, 21, h, w, 7100 + h * w)


def gpu_inputs():
    """(name, x, (c_begin, c_count, ref_begin, ref_count)): every input test_gm_gpu.py compares with the definition."""
    for c, hw in SWEEP:
        yield "C=%d %dx%d" % (c, hw[0], hw[1]), sweep_case(c, hw), (0, None, 0, None)
    yield "pieces", piece_case(), (0, None, 0, None)
    yield "batch", batch_case(), (0, None, 0, None)
    x = subrange_case()
    yield "subrange", x, (0, None, 3, x.shape[1] - 5)
    for h, w in ((6, 6), (7, 7)):
        yield "views %dx%d" % (h, w), view_case(h, w), (0, None, 0, None)


def relative_error(got, ref):
    """max |got - ref| / ref over ref > 0; where ref == 0, got must be 0 (inf otherwise)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ((ref == 0) & (got != 0)).any():
        return float("inf")
    live = ref > 0
    return float((np.abs(got - ref)[live] / ref[live]).max()) if live.any() else 0.0


def restatement_error(x, ranges=(0, None, 0, None)):
    return relative_error(gm_nc_f32(x, *ranges), gm_nc_f64(x, *ranges))


def measure(verbose=False):
    worst = 0.0
    for name, x, ranges in gpu_inputs():
        err = restatement_error(x, ranges)
        worst = max(worst, err)
        if verbose:
            print("%-16s %-18s err %.3e" % (name, tuple(x.shape), err))
    return worst


if __name__ == "__main__":
    r = measure(verbose=True)
    print("r = %.3e   8 r = %.3e   (R = %.3e in this file)" % (r, 8 * r, R))
