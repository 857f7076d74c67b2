"""The low-pass DCT signature and the band-limited gm distance in float64: the definitions dcts_dct2d_lowpass_f32 and
ops.gm_distance_nc(lowpass=K) / ops.gm_pair_matrix(lowpass=K) are tested against.

Definition:  S[n, j] = dctn(x[n, j], type=2, norm='ortho')[:K, :K]  (SciPy, float64; an edge below K keeps every coefficient).
drop_dc: S[n, j, 0, 0] = +0.0, and a FLAT map (max == min on the map itself, exact; an all-zero map is one) gets an all-+0.0
signature whatever round-off its coefficients hold.
The distances are those of tests/gm_oracle.py (l2) and tests/gm_metric_oracle.py (cosine) on the signature tensor; "correlation"
is the cosine of the signatures without their DC term: the mean of a map is its DC coefficient, so dropping it is the centring.

TOLERANCES (derived here, not measured on the code under test).
  signature   2e-6 * max |coefficient| of the batch: the bound tests/test_gpu_coeff_large.py holds dct2d to (SIG_TOL).
  distance    a signature element is off by at most SIG_TOL * S, S the batch's coefficient scale, so a signature of Kh * Kw
              elements by at most sqrt(Kh * Kw) * SIG_TOL * S in norm, and a term ||a - b|| by the sum of both maps' errors,
              2 * sqrt(Kh * Kw) * SIG_TOL * S; a score adds r_count terms (a pair-matrix entry N). On top of it comes the
              relative round-off of the distance kernels themselves, TOL of tests/gm_oracle.py. distance_bound() returns the
              absolute part. Under a metric the signatures are normalised first: the error of a unit signature is the absolute
              one divided by the signature's norm, so metric_bound() takes the smallest norm of a live signature.
No product import: numpy, scipy and torch only.
"""
import numpy as np
import torch
from scipy.fft import dctn

import gm_oracle as go

SIG_TOL = 2e-6
METRICS = ("l2", "cosine", "correlation")


def _f64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


def flat_maps(x):
    """[N, C] bool: every element of the map equals every other (max == min on the map as it is stored)."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = a.reshape(a.shape[0], a.shape[1], -1)
    return a.max(axis=-1) == a.min(axis=-1)


def coefficients_f64(x):
    """[N, C, H, W] float64: the orthonormal 2-D DCT-II of every map."""
    return dctn(_f64(x), type=2, norm="ortho", axes=(-2, -1))


def lowpass_f64(x, K, c_begin=0, c_count=None, drop_dc=False):
    """The definition: numpy float64 [N, c_count, min(K, H), min(K, W)]."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    c_count = x.shape[1] - c_begin if c_count is None else c_count
    xs = x[:, c_begin:c_begin + c_count]
    s = np.ascontiguousarray(coefficients_f64(xs)[..., :K, :K])
    if drop_dc:
        s[..., 0, 0] = 0.0
        s[flat_maps(xs)] = 0.0
    return s


def coefficient_scale(x):
    """S: the largest |coefficient| of the batch (all of them, not the corner)."""
    return float(np.abs(coefficients_f64(x)).max())


def signature_tolerance(x):
    return SIG_TOL * coefficient_scale(x)


def _unit(s):
    """The signatures [N, C, p] scaled to unit norm; one without a norm is the zero vector."""
    n = np.sqrt((s * s).sum(axis=-1, keepdims=True))
    return np.where(n > 0, s / np.where(n > 0, n, 1.0), 0.0), n[..., 0]


def signatures(x, K, metric="l2"):
    """What the distance is taken between, [N, C, Kh * Kw] float64, and the norms of the raw signatures [N, C]."""
    if metric not in METRICS:
        raise ValueError("metric")
    s = lowpass_f64(x, K, drop_dc=(metric == "correlation"))
    s = s.reshape(s.shape[0], s.shape[1], -1)
    if metric == "l2":
        return s, np.sqrt((s * s).sum(axis=-1))
    return _unit(s)


def pair_distances_f64(x, K, metric="l2", c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """[N, c_count, ref_count] float64: d_K of every scored map to every reference map."""
    s, _ = signatures(x, K, metric)
    cb, cc, rb, rc = go._ranges(s.shape[1], c_begin, c_count, ref_begin, ref_count)
    d = s[:, cb:cb + cc, None, :] - s[:, None, rb:rb + rc, :]
    return np.sqrt((d * d).sum(axis=-1))


def gm_lowpass_f64(x, K, metric="l2", c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """[N, c_count] float64: the summed band-limited distance to the reference channels."""
    return pair_distances_f64(x, K, metric, c_begin, c_count, ref_begin, ref_count).sum(axis=-1)


def pair_matrix_f64(x, K, metric="l2", c_begin=0, c_count=None, ref_begin=0, ref_count=None):
    """[c_count, ref_count] float64: the pair distances summed over the samples."""
    return pair_distances_f64(x, K, metric, c_begin, c_count, ref_begin, ref_count).sum(axis=0)


def gm_lowpass_nc(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, out=None, metric="l2", lowpass=0):
    """ops.gm_distance_nc's signature on the CPU, `lowpass` included (torch float32 [N, c_count]); lowpass=0 is gm_oracle's."""
    if not lowpass:
        if metric != "l2":
            raise ValueError("the stand-in knows the plain distance under l2 only")
        return go.gm_nc(x, c_begin, c_count, ref_begin, ref_count)
    return torch.from_numpy(gm_lowpass_f64(x, lowpass, metric, c_begin, c_count, ref_begin, ref_count).astype(np.float32))


def gm_lowpass_pairs(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, metric="l2", out=None, lowpass=0):
    """ops.gm_pair_matrix's signature on the CPU with `lowpass` (torch float32 [c_count, ref_count])."""
    if not lowpass:
        raise ValueError("the stand-in knows the low-pass matrix only")
    return torch.from_numpy(pair_matrix_f64(x, lowpass, metric, c_begin, c_count, ref_begin, ref_count).astype(np.float32))


def distance_bound(x, K, terms):
    """The absolute part of the tolerance of a sum of `terms` l2 distances between signatures of x (see the module text)."""
    kh, kw = min(K, x.shape[2]), min(K, x.shape[3])
    return terms * 2.0 * np.sqrt(kh * kw) * SIG_TOL * coefficient_scale(x)


def metric_bound(x, K, metric, terms):
    """The same for unit signatures: the absolute error divided by the smallest norm of a live signature."""
    if metric == "l2":
        return distance_bound(x, K, terms)
    _, norms = signatures(x, K, metric)
    live = norms[norms > 0]
    return distance_bound(x, K, terms) / float(live.min()) if live.size else 0.0


# ----------------------------------------------------------------------------------------------------
# the cases of the per-edge probes (tests/test_lowpass_gpu.py, tests/test_lowpass_probes_gpu.py, tests/test_lowpass_cpu.py)
# ----------------------------------------------------------------------------------------------------
# Every edge with a codelet: each is an instantiation of k_lowpass_codelet of its own. The GPU and CPU files assert that this
# is the library's list.
CODELET_EDGES = (2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 48, 56, 60, 64)
FLAT_VALUES = (3.7, 0.0, -1.25)                  # what a flat map holds, in turn
NOT_FLAT = ("random", "last", "first", "nan")    # what a map that is not flat is, in turn


def group_size(n):
    """G: the maps a wave of the codelet kernel holds at edge n."""
    return 64 // n


def corner_sizes(n):
    """The K of a probe at edge n: small ones, both sides of a multiple of 4, the last two."""
    return sorted({k for k in (1, 2, 3, 4, 5, 8, 12, n - 1, n) if 1 <= k <= n})


def on_vector_chain(n, K, aligned=True):
    """The kernel's own rule for the 16-byte store chain: several maps per wave, K a multiple of 4, a 16-byte-aligned out."""
    return group_size(n) >= 2 and K % 4 == 0 and aligned


def chain_sizes(n):
    """(K on the 16-byte chain or None, K on the scalar chain) for the drop_dc probe at edge n. No K <= 2 is a multiple
    of 4, so edge 2 has the scalar chain only."""
    vec = 8 if n >= 8 else (4 if n >= 4 else None)
    return (vec if group_size(n) >= 2 else None), (5 if n >= 5 else min(n, 3))


def flat_pattern_count(n):
    """Maps of a flat pattern: at least 2 G + 1 (two full groups and a ragged one), and enough that each parity holds all
    four kinds of a map that is not flat."""
    return max(2 * group_size(n) + 1, 9)


def flat_pattern_maps(n, parity, seed=0):
    """(x [1, C, n, n] float32, kinds): channel j is flat iff j % 2 == parity, with the values of FLAT_VALUES in turn; the
    others take the kinds of NOT_FLAT in turn: a random map, 3.7 except for the last element, 3.7 except for the first
    element, 3.7 except for one NaN. kinds[j] is "flat" or the kind."""
    C = flat_pattern_count(n)
    x = torch.randn(1, C, n, n, generator=torch.Generator().manual_seed(8000 + 10 * n + seed))
    kinds, nf, fl = [], 0, 0
    for j in range(C):
        if j % 2 == parity:
            x[0, j] = FLAT_VALUES[fl % len(FLAT_VALUES)]
            fl += 1
            kinds.append("flat")
            continue
        kind = NOT_FLAT[nf % len(NOT_FLAT)]
        nf += 1
        kinds.append(kind)
        if kind == "random":
            continue
        x[0, j] = 3.7
        if kind == "last":
            x[0, j, n - 1, n - 1] = 3.7000003
        elif kind == "first":
            x[0, j, 0, 0] = 0.0
        else:
            x[0, j, n // 2, 0] = float("nan")
    return x, kinds


def basis_bank(n):
    """[1, n * n, n, n] float64: map u * n + v is basis_map(n, u, v)."""
    k = np.arange(n)
    c = np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * n)) * np.sqrt(2.0 / n)
    c[0] = np.sqrt(1.0 / n)
    return np.einsum("ui,vj->uvij", c, c).reshape(1, n * n, n, n)


def basis_map(n, u, v):
    """The n x n map whose orthonormal DCT is 1 at [u, v] and 0 elsewhere: outer(C[u, :], C[v, :])."""
    k = np.arange(n)
    cu = np.cos(np.pi * (2 * k + 1) * u / (2 * n)) * (np.sqrt(1.0 / n) if u == 0 else np.sqrt(2.0 / n))
    cv = np.cos(np.pi * (2 * k + 1) * v / (2 * n)) * (np.sqrt(1.0 / n) if v == 0 else np.sqrt(2.0 / n))
    return np.outer(cu, cv)
