"""The spectral entropy of a map's DCT coefficients: the definition dcts_spectral_entropy_f32 is tested against, an fp32
restatement of the kernels' one-pass formula (the yardstick for round-off), the inputs of tests/test_entropy_gpu.py, and
the tolerance derived from them.

Definition (float64, on oracle.dct_oracle's SciPy coefficients, the odd front pad included):
    c = dct_2d(x[n, c_begin + j], norm='ortho'),  E = sum c^2,  p = c^2 / E,  H = -sum_{p > 0} p ln p;  H = 0 where E == 0.

The restatement (entropy_nc_f32) does in float32 what the kernels do: a DCT-II of each axis as a float32 matrix product
with the cosine basis on the kernel's scale (`scale="kernel"`: the unnormalised transform of the fused kernel, w = c *
sqrt(H' W') / 2; `scale="ortho"`: the orthonormal coefficients the fallback's reduction reads), then
    e = sum w^2,  s = sum w^2 ln(w^2) (zero squares add 0),  H = ln e - s / e, clamped into [0, ln(H' W')].

TOLERANCE. It is absolute. R is the largest |restatement - definition| over the GPU tests' own inputs (gpu_inputs(): every
input with the scale of each route the tests send it through), measured on a CPU with

    python tests/entropy_oracle.py

which prints the error per input and the maximum; the kernels get TOL = 8 * R (DESIGN.md section 5's convention: room for
another summation order and a logf that differs by an ulp). tests/test_entropy_cpu.py re-measures R on a few of the
inputs and checks that the constant below still covers them. The largest errors come from the maps scaled by 2^20 (ln e is
near 37 there, and ln e - s / e cancels most of it).
"""
import math
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # run as a script: the repository root holds oracle/
    sys.path.insert(0, _ROOT)

from oracle import dct_oracle as orc  # noqa: E402

R = 5.192e-6     # measured with the command above: "scale 2^20" sets it; 8 R = 4.154e-5
TOL = 8 * R

# every codelet edge and every odd edge the front pad takes to one: each (edge, pad) is an instantiation of k_entropy_codelet
# of its own (tests/test_entropy_gpu.py and tests/test_entropy_cpu.py assert that these are the library's lists)
FUSED_EDGES = (2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 48, 56, 60, 64)
PAD_EDGES = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 23, 27, 29, 31, 35, 39, 47, 55, 59, 63)  # h -> h + 1 with pad_front_if_odd
BASIS_EDGES = (8, 14)
FALLBACK_SHAPES = ((56, 28), (13, 13), (72, 72), (288, 288))
DIRECT_SHAPES = ((100, 72), (260, 9))  # non-square with an edge beyond 64: the coefficients of the cosine-matrix kernel alone
PITCH_EDGE, PITCH = 16, 20


# ----------------------------------------------------------------------------------------------------
# the definition
# ----------------------------------------------------------------------------------------------------
def _slice(x, c_begin, c_count, pad_front_if_odd, dtype):
    a = x.detach().cpu().numpy().astype(dtype)
    if c_count is None:
        c_count = a.shape[1] - c_begin
    a = a[:, c_begin:c_begin + c_count]
    if pad_front_if_odd and a.shape[2] % 2 != 0:
        a = np.pad(a, ((0, 0), (0, 0), (1, 0), (1, 0)))
    return a


def entropy_of_coefficients_f64(c):
    """H of float64 coefficients [..., H, W] -> [...]."""
    sq = np.asarray(c, np.float64) ** 2
    e = sq.sum(axis=(-2, -1), keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(e > 0, sq / e, 0.0)
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=(-2, -1))


def entropy_nc_f64(x, c_begin=0, c_count=None, pad_front_if_odd=False):
    """The definition: numpy float64 [N, c_count]."""
    return entropy_of_coefficients_f64(orc.dct_2d_f64(_slice(x, c_begin, c_count, pad_front_if_odd, np.float64)))


def entropy_nc(x, c_begin=0, c_count=None, pad_front_if_odd=False, algo=0, out=None):
    """ops.spectral_entropy_nc's signature on the CPU: the definition rounded to float32 (torch [N, c_count])."""
    return torch.from_numpy(entropy_nc_f64(x, c_begin, c_count, pad_front_if_odd).astype(np.float32))


# ----------------------------------------------------------------------------------------------------
# the fp32 restatement of the one-pass formula
# ----------------------------------------------------------------------------------------------------
def _basis32(n, ortho):
    k = np.arange(n, dtype=np.float64)
    b = np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * n))
    b[0] /= math.sqrt(2.0)
    if ortho:
        b *= math.sqrt(2.0 / n)
    return b.astype(np.float32)


def coefficients_f32(x, c_begin=0, c_count=None, pad_front_if_odd=False, scale="kernel"):
    """The restatement's coefficients, numpy float32 [N, c_count, H', W']: a float32 matrix product per axis."""
    a = _slice(x, c_begin, c_count, pad_front_if_odd, np.float32)
    bh, bw = _basis32(a.shape[2], scale == "ortho"), _basis32(a.shape[3], scale == "ortho")
    w = np.matmul(np.matmul(bh, a), bw.T)
    assert w.dtype == np.float32
    return w


def entropy_nc_f32(x, c_begin=0, c_count=None, pad_front_if_odd=False, scale="kernel"):
    """Every step in float32 (numpy float32 [N, c_count]); scale: "kernel" (unnormalised) or "ortho"."""
    return entropy_of_coefficients_f32(coefficients_f32(x, c_begin, c_count, pad_front_if_odd, scale))


def entropy_of_coefficients_f32(w):
    """The one-pass formula on float32 coefficients [..., H', W'] of any common scale -> float32 [...]."""
    assert w.dtype == np.float32
    hp, wp = w.shape[-2], w.shape[-1]
    sq = w * w
    e = sq.sum(axis=(-2, -1), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(sq == 0, np.float32(0), sq * np.log(sq))
        s = t.sum(axis=(-2, -1), dtype=np.float32)
        h = np.log(e) - s / e
    assert t.dtype == np.float32 and h.dtype == np.float32
    h = np.where(e == 0, np.float32(0), h)
    return np.clip(h, np.float32(0), np.float32(math.log(hp * wp))).astype(np.float32)


# ----------------------------------------------------------------------------------------------------
# the inputs of tests/test_entropy_gpu.py
# ----------------------------------------------------------------------------------------------------
def mixed_maps(n, c, h, w, seed):
    """[n, c, h, w]: random normal maps in the even channels, post-ReLU maps (about half exact zeros) in the odd ones."""
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed))
    x[:, 1::2] = torch.relu(x[:, 1::2])
    return x


def fused_case(edge):
    """Map counts that are no multiple of the wave's group size: 3 x 7 maps, 2 x 5 at 56 and 64."""
    n, c = (2, 5) if edge >= 56 else (3, 7)
    return mixed_maps(n, c, edge, edge, 1000 + edge)


def pad_case(edge):
    return mixed_maps(3, 7, edge, edge, 2000 + edge)


def basis_maps(n):
    """[1, n * n, n, n]: map u * n + v is the (u, v) basis function of the orthonormal n x n DCT (entropy 0)."""
    b = _basis64(n)
    return torch.from_numpy(np.einsum("ui,vj->uvij", b, b).reshape(1, n * n, n, n).astype(np.float32))


def pair_maps(n):
    """[1, 6, n, n]: sums of two basis functions of equal amplitude (entropy ln 2)."""
    b = _basis64(n)
    pairs = [((0, 0), (1, 1)), ((0, 1), (n - 1, n - 1)), ((2, 3), (3, 2)), ((n - 1, 0), (0, n - 1)), ((1, 0), (n // 2, n // 2)),
             ((0, 0), (n - 1, n - 1))]
    maps = [np.outer(b[u0], b[v0]) + np.outer(b[u1], b[v1]) for (u0, v0), (u1, v1) in pairs]
    return torch.from_numpy(np.stack(maps)[None].astype(np.float32))


def unequal_pair_maps(n):
    """[1, n * n, n, n]: map u * n + v is basis(p) + 0.5 * basis(u, v), built in float64 and rounded once; the partner p is
    (1 % n, 2 % n), or (2 % n, 1 % n) where that is (u, v) itself. p = (0.8, 0.2): H = -(0.8 ln 0.8 + 0.2 ln 0.2) = 0.5004,
    and where the equal pairs sit at the maximum of H (a relative error eps in one weight moves ln 2 by eps^2 / 2), here it
    moves H by 0.44 eps: every coefficient's weight is seen, the 1 / sqrt(2) of the DC row and column included."""
    b = _basis64(n)
    u, v = np.divmod(np.arange(n * n), n)
    first = (u == 1 % n) & (v == 2 % n)
    pu, pv = np.where(first, 2 % n, 1 % n), np.where(first, 1 % n, 2 % n)
    assert not ((pu == u) & (pv == v)).any()
    maps = b[pu][:, :, None] * b[pv][:, None, :] + 0.5 * (b[u][:, :, None] * b[v][:, None, :])
    return torch.from_numpy(maps[None].astype(np.float32))


def padded_unequal_pair_maps(edge):
    """[1, (edge + 1)^2, edge, edge] for an odd edge: the unequal pairs of the padded tile without their first row and
    column. The front pad puts zeros there, so no such map is a pair any more; the float64 definition, which pads the same
    way, is the yardstick."""
    return unequal_pair_maps(edge + 1)[:, :, 1:, 1:].contiguous()


H_UNEQUAL = -(0.8 * math.log(0.8) + 0.2 * math.log(0.2))


def _basis64(n):
    k = np.arange(n, dtype=np.float64)
    b = np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * n)) * math.sqrt(2.0 / n)
    b[0] /= math.sqrt(2.0)
    return b


def scale_case():
    """(x, x * 2^20, x * 2^-20): [1, 6, 14, 14] each; the scalings are exact in float32."""
    x = mixed_maps(1, 6, 14, 14, 3000)
    return x, x * 2.0 ** 20, x * 2.0 ** -20


def fallback_case(h, w):
    return mixed_maps(1, 3, h, w, 4000 + h + w)


def direct_case(h, w):
    """[2, 5, h, w]: two samples, so that a channel slice of it is not contiguous."""
    return mixed_maps(2, 5, h, w, 4100 + h + w)


def pitch_case(device="cpu"):
    """A [2, 5, 16, 16] view with strideH = 20 of a tensor on `device` whose pad columns hold 3.0. The tensor is moved
    first and sliced there: .to() of the view itself would hand back a dense copy."""
    big = torch.full((2, 5, PITCH_EDGE, PITCH), 3.0)
    big[..., :PITCH_EDGE] = mixed_maps(2, 5, PITCH_EDGE, PITCH_EDGE, 5000)
    return big.to(device)[..., :PITCH_EDGE]


def loop_banks():
    """The banks of the two grid-loop cases (tests/loop_cases.py): 4 x 4 for the fused kernel, 5 x 5 for the reduction."""
    import loop_cases as lc
    return lc.make_bank(4, 4, 1304)[None], lc.make_bank(5, 5, 1305)[None]


def gpu_inputs():
    """(name, x [N, C, H, W], pad_front_if_odd, scales): every input test_entropy_gpu.py compares with the definition,
    with the scale of each route it is sent through there."""
    for e in FUSED_EDGES:
        yield "fused %d" % e, fused_case(e), False, ("kernel",)
    for e in PAD_EDGES:
        yield "pad %d" % e, pad_case(e), True, ("kernel",)
    for e in BASIS_EDGES:
        yield "basis %d" % e, basis_maps(e), False, ("kernel",)
        yield "pairs %d" % e, pair_maps(e), False, ("kernel",)
    for e in FUSED_EDGES:
        yield "unequal %d" % e, unequal_pair_maps(e), False, ("kernel",)
    for e in PAD_EDGES:
        yield "pad unequal %d" % e, padded_unequal_pair_maps(e), True, ("kernel",)
    for name, x in zip(("scale 1", "scale 2^20", "scale 2^-20"), scale_case()):
        yield name, x, False, ("kernel",)
    for h, w in FALLBACK_SHAPES:
        yield "fallback %dx%d" % (h, w), fallback_case(h, w), False, ("ortho",)
    for h, w in DIRECT_SHAPES:
        yield "direct %dx%d" % (h, w), direct_case(h, w), False, ("ortho",)
    yield "pitched 16", pitch_case().contiguous(), False, ("ortho",)
    yield "direct 16", fused_case(16), False, ("ortho",)
    b4, b5 = loop_banks()
    yield "loop bank 4", b4, False, ("kernel",)
    yield "loop bank 5", b5, False, ("ortho",)


def restatement_error(x, pad, scales):
    ref = entropy_nc_f64(x, pad_front_if_odd=pad)
    return max(float(np.abs(entropy_nc_f32(x, pad_front_if_odd=pad, scale=s).astype(np.float64) - ref).max()) for s in scales)


def measure(verbose=False):
    worst = 0.0
    for name, x, pad, scales in gpu_inputs():
        err = restatement_error(x, pad, scales)
        worst = max(worst, err)
        if verbose:
            print("%-18s %-16s %s  err %.3e" % (name, tuple(x.shape), "+".join(scales), err))
    return worst


if __name__ == "__main__":
    r = measure(verbose=True)
    print("r = %.3e   8 r = %.3e   (R = %.3e in this file)" % (r, 8 * r, R))
