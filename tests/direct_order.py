"""A numpy model of the summation order of the cosine-matrix kernel (k_energy_direct, csrc/direct.hip). No product import.

The kernel computes Y = C_h x C_w^T in two phases, T[k][c] = sum_r C_h[k][r] x[r][c] and Y[k][l] = sum_c T[k][c] C_w[l][c],
every dot product from fp32 FMAs in ascending index order, the tables fp32(C) with C the float64 orthonormal DCT-II matrix
(dct_probes.dct_matrix). `sizes` states how a dot product is cut, from the outermost level inwards:

  sizes=()         one FMA chain over all terms: the order of the kernel before tests/test_direct_order_cpu.py existed;
  sizes=(B,)       chains over B consecutive terms, each from +0.0, the chain sums added in ascending order, each add
                   rounded to fp32;
  sizes=(G, B)     the same within every run of G consecutive terms (G a multiple of B), and the sums of the runs added
                   in ascending order: ORDER = (64, 16) is the kernel's (kDirectGroup = 4 blocks of kDirectBlock = 16).

Where a level has one part its sum is that part: an edge of at most B is the single chain, bit for bit.
One FMA is acc = fp32(fp64(acc) + fp64(a) * fp64(b)): the product of two fp32 values is exact in float64, so the only
departure from a hardware FMA is the double rounding of the sum, an error of 2^-53 relative before the fp32 rounding.
The squares of Y are summed in float64, so the model's energy error is a LOWER bound on the kernel's, which sums them in
fp32 (per lane one chain per 16 output rows, then a 256-lane tree)."""
import numpy as np

import dct_probes as dp

ORDER = (64, 16)    # csrc/direct.hip: kDirectBlock * kDirectGroup, kDirectBlock
_CHUNK = 1 << 15    # elements of one accumulator slab: the model's working set stays in the cache


def table(n):
    """fp32(C), C[k][r] the float64 orthonormal DCT-II matrix of edge n."""
    return dp.dct_matrix(n).numpy().astype(np.float32)


def _chain(a, x, lo, hi):
    """[K, N] fp32: the FMA chain sum_{r = lo}^{hi - 1} a[k][r] * x[r][n] from +0.0 (a, x float64 copies of fp32 values)."""
    shape = (a.shape[0], x.shape[1])
    acc64, prod, acc32 = np.zeros(shape), np.empty(shape), np.empty(shape, dtype=np.float32)
    for r in range(lo, hi):
        np.multiply(a[:, r, None], x[r][None, :], out=prod)
        np.add(acc64, prod, out=acc64)
        acc32[...] = acc64   # the fp32 rounding of the FMA
        acc64[...] = acc32
    return acc32


def _ordered(a, x, lo, hi, sizes):
    if not sizes:
        return _chain(a, x, lo, hi)
    tot = _ordered(a, x, lo, min(lo + sizes[0], hi), sizes[1:])
    for part in range(lo + sizes[0], hi, sizes[0]):
        # the sum of two fp32 values is exact in float64 (or far below its rounding): one rounding, to fp32
        tot = (tot.astype(np.float64) + _ordered(a, x, part, min(part + sizes[0], hi), sizes[1:])).astype(np.float32)
    return tot


def ordered_matmul(a, x, sizes=ORDER):
    """[K, N] fp32 = a [K, R] @ x [R, N], every entry summed over r in the order `sizes` states (module docstring)."""
    a64 = a.astype(np.float64)
    out = np.empty((a.shape[0], x.shape[1]), dtype=np.float32)
    step = max(1, _CHUNK // a.shape[0])
    for n0 in range(0, x.shape[1], step):
        out[:, n0:n0 + step] = _ordered(a64, x[:, n0:n0 + step].astype(np.float64), 0, a.shape[1], tuple(sizes))
    return out


def coefficients(x, sizes=ORDER):
    """x [P, H, W] fp32 -> Y [H, P, W] fp32 in the kernel's order: phase 1 over r, phase 2 over c."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    p, h, w = x.shape
    t = ordered_matmul(table(h), x.transpose(1, 0, 2).reshape(h, p * w), sizes)         # T[k][(p, c)]
    t = t.reshape(h, p, w).transpose(2, 0, 1).reshape(w, h * p)                         # T[c][(k, p)]
    y = ordered_matmul(table(w), np.ascontiguousarray(t), sizes)                        # Y[l][(k, p)]
    return y.reshape(w, h, p).transpose(1, 2, 0)


def energy(x, sizes=ORDER):
    """float64 [P]: sum of the squares of the model's fp32 coefficients, in float64."""
    y = coefficients(x, sizes).astype(np.float64)
    return np.einsum("kpl,kpl->p", y, y)


def worst_basis_error(n_h, n_w, pairs, sizes=ORDER, maps_per_call=256):
    """(worst relative error against float64 sum(x^2), its (u, v)) of the model over the basis sweep `pairs`."""
    worst, at = 0.0, None
    for lo in range(0, len(pairs), maps_per_call):
        part = pairs[lo:lo + maps_per_call]
        x = dp.basis_maps(n_h, n_w, part).numpy()
        ref = (x.astype(np.float64) ** 2).sum(axis=(1, 2))
        err = np.abs(energy(x, sizes) - ref) / ref
        i = int(err.argmax())
        if err[i] > worst:
            worst, at = float(err[i]), (int(part[i][0]), int(part[i][1]))
    return worst, at
