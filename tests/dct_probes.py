"""Per-coefficient and per-sample probes of an energy function, at fp32 accuracy.

The energy of a map is Parseval-invariant, so two families of inputs turn one number per map into a
look at every weight a kernel applies:
  * a map that is one orthonormal DCT-II basis function outer(C[u, :], C[v, :]): its energy IS the
    weight the kernel gives coefficient (u, v);
  * a map with one non-zero sample at (i, j): its energy IS the weight the kernel gives that sample.
The float64 reference of both (and of any other map) is sum(x^2) of the fp32 input itself.

Everything here takes a callable `energy_fn(x[N, C, H, W]) -> [N, C]` (`coeff_fn(x) -> [N, C, H, W]` for
the coefficient check) and a torch device, so the same code runs against the oracle on the CPU
(tests/test_probes_cpu.py) and against the HIP kernels (tests/test_gpu_probes.py). No product import.

THE TOLERANCE RULE. No fixed number: E_ref is the largest relative error of the fp32 restatement of the
reference (oracle.dct_oracle.energy_nc_batched, on the CPU) against float64 on a subsample of the test's own
inputs, and tol = FACTOR * max(E_ref, FLOOR). FLOOR = 2^-22 is the reference's typical error (1.6e-7 ... 3.0e-7
at every edge from 7 to 512), so a lucky draw cannot shrink the budget. FACTOR = 8: the reference's error
comes from a log-depth FFT; the kernels have direct sums for odd factors, another reduction tree and, in
the cosine-matrix kernel, dot products of up to 512 terms. The same rule with the reference's coefficient
errors bounds check_coefficients. No family has a margin of its own (DESIGN.md section 5 holds the table).
"""
import math

import torch

from helpers import synth
from oracle import dct_oracle as orc

FLOOR = 2.0 ** -22          # the reference's typical relative error against float64
FACTOR = 8.0                # tol = FACTOR * max(E_ref, FLOOR)
SUBSAMPLE_MAPS = 512        # E_ref is measured on at most this many maps of a sweep ...
SUBSAMPLE_BYTES = 16 << 20  # ... and at most this many bytes of them (16 maps at 512 x 512)
CHUNK_BYTES = 1 << 30       # a sweep hands its maps over in pieces of at most 1 GiB
EXHAUSTIVE_BYTES = 1 << 30  # all u x all v where (n_h n_w) maps of (n_h n_w) floats fit in this (edges <= 128)
POW2_K = 20                 # check_pow2_scaling: x * 2^+-20
FIXED_RANDOM_K = 8          # seeded random indices per axis that cover() adds by default


# ----------------------------------------------------------------------------------------------------
# index sets
# ----------------------------------------------------------------------------------------------------
def axis_picks(n, k, seed=0):
    """V(n): 0, 1, 2, 3, n/2-1, n/2, n-2, n-1 (those that exist) plus seeded random indices: first one of
    every residue mod 8 the fixed ones miss, then further ones until k random indices are in (more than k
    if the residues need more: the residues are never cut)."""
    if n <= 8:
        return list(range(n))
    picks = {i for i in (0, 1, 2, 3, n // 2 - 1, n // 2, n - 2, n - 1) if 0 <= i < n}
    g = torch.Generator().manual_seed(1000 * n + seed)
    added = 0
    for r in range(8):
        if not any(p % 8 == r for p in picks):
            cand = list(range(r, n, 8))
            picks.add(cand[int(torch.randint(len(cand), (1,), generator=g))])
            added += 1
    while added < k and len(picks) < n:
        i = int(torch.randint(n, (1,), generator=g))
        if i not in picks:
            picks.add(i)
            added += 1
    return sorted(picks)


def cover(n_h, n_w, k=FIXED_RANDOM_K, seed=0, exhaustive=None):
    """The (u, v) index set of a sweep, a sorted LongTensor [P, 2]: (all u) x V(n_w) together with V(n_h) x (all v).
    The amplitude weights of the split kernels are separable per axis, so this reaches every table entry of
    both axes. All u x all v where that fits in EXHAUSTIVE_BYTES (or where `exhaustive` says so)."""
    if exhaustive is None:
        exhaustive = (n_h * n_w) ** 2 * 4 <= EXHAUSTIVE_BYTES
    if exhaustive:
        us, vs = torch.meshgrid(torch.arange(n_h), torch.arange(n_w), indexing="ij")
        return torch.stack([us.reshape(-1), vs.reshape(-1)], dim=1)
    vh, vw = axis_picks(n_h, k, seed), axis_picks(n_w, k, seed + 1)
    pairs = {(u, v) for u in range(n_h) for v in vw} | {(u, v) for u in vh for v in range(n_w)}
    return torch.tensor(sorted(pairs), dtype=torch.long)


def chunk_ranges(count, bytes_per_map, limit=CHUNK_BYTES):
    step = max(1, limit // bytes_per_map)
    return [(lo, min(lo + step, count)) for lo in range(0, count, step)]


def subsample(pairs, n_h, n_w, seed=0):
    """Seeded subsample of a sweep's index set for E_ref: at most SUBSAMPLE_MAPS maps and SUBSAMPLE_BYTES."""
    m = min(SUBSAMPLE_MAPS, len(pairs), max(8, SUBSAMPLE_BYTES // (n_h * n_w * 4)))
    g = torch.Generator().manual_seed(77 + seed)
    return pairs[torch.randperm(len(pairs), generator=g)[:m].sort().values]


# ----------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------
def dct_matrix(n, device="cpu"):
    """Orthonormal DCT-II matrix C[u, i] = s(u) cos(pi (2 i + 1) u / 2 n), float64."""
    i = torch.arange(n, dtype=torch.float64, device=device)
    c = torch.cos(math.pi * (2.0 * i[None, :] + 1.0) * i[:, None] / (2.0 * n)) * math.sqrt(2.0 / n)
    c[0] = math.sqrt(1.0 / n)
    return c


def basis_maps(n_h, n_w, pairs, device="cpu"):
    """[P, n_h, n_w] fp32: outer(C_h[u, :], C_w[v, :]) built in float64 and rounded once."""
    pairs = pairs.to(device)
    cu = dct_matrix(n_h, device)[pairs[:, 0]]
    cv = dct_matrix(n_w, device)[pairs[:, 1]]
    out = torch.empty((len(pairs), n_h, n_w), dtype=torch.float32, device=device)
    torch.mul(cu[:, :, None], cv[:, None, :], out=out)  # the product is formed in float64, rounded on the store
    return out


def impulse_maps(n_h, n_w, pairs, seed=0, device="cpu"):
    """[P, n_h, n_w] fp32: map p is zero but for one sample at pairs[p], uniform in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    val = (0.5 + 1.5 * torch.rand(len(pairs), generator=g)).to(device)
    pairs = pairs.to(device)
    out = torch.zeros((len(pairs), n_h, n_w), dtype=torch.float32, device=device)
    out[torch.arange(len(pairs), device=device), pairs[:, 0], pairs[:, 1]] = val
    return out


def random_maps(n, c, n_h, n_w, seed, signed=False, device="cpu"):
    """The suite's synthetic maps (relu(randn) * per-channel scale, every c % 8 == 5 dead), or the SIGNED
    variant (randn, no ReLU: a normalised image, as U^2-Net-p's input hook scores), dead channels alike."""
    if not signed:
        return synth(n, c, n_h, n_w, seed).to(device)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, n_h, n_w, generator=g)
    s = torch.exp(0.5 * torch.randn(c, generator=g))
    s[torch.arange(c) % 8 == 5] = 0
    return (x * s[None, :, None, None]).to(device)


# ----------------------------------------------------------------------------------------------------
# the tolerance rule
# ----------------------------------------------------------------------------------------------------
def parseval(x):
    return x.double().pow(2).sum(dim=(-2, -1))


def reference_error(x, **kw):
    """E_ref: largest relative error of the fp32 reference restatement against float64 on the maps x [N, C, H, W]."""
    x = x.detach().cpu()
    ref = parseval(x)
    got = orc.energy_nc_batched(x, **kw).double()
    nz = ref > 0
    return ((got - ref).abs() / ref.clamp_min(1e-300))[nz].max().item() if nz.any() else 0.0


def tolerance(e_ref):
    return FACTOR * max(e_ref, FLOOR)


def reference_coefficient_errors(n_h, n_w, pairs, x):
    """(|peak - 1|, leak elsewhere) of the fp32 reference transform on the basis maps x [P, H, W] of `pairs`."""
    return _peak_and_leak(orc.dct_2d(x.detach().cpu()[None])[0], pairs)


def _peak_and_leak(c, pairs):
    idx = torch.arange(len(pairs), device=c.device)
    pairs = pairs.to(c.device)
    c = c.clone()
    peak = c[idx, pairs[:, 0], pairs[:, 1]].double()
    c[idx, pairs[:, 0], pairs[:, 1]] = 0
    leak = c.abs().flatten(1).amax(dim=1).double() if c[0].numel() > 0 else torch.zeros_like(peak)
    return (peak - 1).abs(), leak


# ----------------------------------------------------------------------------------------------------
# checkers: each returns what it measured and raises AssertionError naming the map that missed
# ----------------------------------------------------------------------------------------------------
def _name(labels, flat, what):
    if labels is None:
        return "%s map %d" % (what, flat)
    return "%s (%d, %d)" % (what, int(labels[flat][0]), int(labels[flat][1]))


def check_energy(energy_fn, x, tol, labels=None, what="map"):
    """energy_fn(x) against sum(x^2) in float64: relative error <= tol where the map is not zero, exactly +0.0
    where it is. x: [N, C, H, W]; labels: optional [N*C, 2] indices that name a map in the message."""
    ref = parseval(x).reshape(-1)
    got = energy_fn(x)
    assert tuple(got.shape) == tuple(x.shape[:2]), "energy shape %s for input %s" % (tuple(got.shape), tuple(x.shape))
    got = got.reshape(-1)
    zero = ref == 0
    if zero.any():
        bad = zero & ((got != 0) | torch.signbit(got))
        if bad.any():
            i = int(bad.nonzero()[0])
            raise AssertionError("%s: zero map gives %r, expected +0.0" % (_name(labels, i, what), got[i].item()))
    if zero.all():
        return 0.0
    err = (got.double() - ref).abs() / ref.clamp_min(1e-300)
    err = torch.where(zero, torch.zeros_like(err), err)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    worst, i = err.max(dim=0)
    worst, i = worst.item(), int(i)
    if not worst <= tol:
        raise AssertionError("%s: energy %.9g, float64 sum(x^2) %.9g, relative error %.3g > %.3g"
                             % (_name(labels, i, what), got[i].item(), ref[i].item(), worst, tol))
    return worst


def sweep(energy_fn, make, pairs, n_h, n_w, tol, what, chunk_bytes=CHUNK_BYTES):
    """check_energy over make(pairs[lo:hi]) -> [p, H, W], in chunks; the worst relative error."""
    worst = 0.0
    for lo, hi in chunk_ranges(len(pairs), n_h * n_w * 4, chunk_bytes):
        x = make(pairs[lo:hi])
        worst = max(worst, check_energy(energy_fn, x[None], tol, labels=pairs[lo:hi], what=what))
        del x
    return worst


def sweep_tolerance(make, pairs, n_h, n_w, seed=0, **kw):
    """The rule of the module docstring on a subsample of a sweep's own maps: (tol, E_ref)."""
    e_ref = reference_error(make(subsample(pairs, n_h, n_w, seed))[None], **kw)
    return tolerance(e_ref), e_ref


def check_coefficients(coeff_fn, n_h, n_w, pairs, device="cpu", tol_peak=None, tol_leak=None, chunk_bytes=CHUNK_BYTES):
    """Basis input: coefficient (u, v) is 1 and every other one is 0. Bounds by the tolerance rule on the reference's
    own coefficient errors unless given. Returns (worst |peak - 1|, worst leak)."""
    if tol_peak is None or tol_leak is None:
        sub = subsample(pairs, n_h, n_w)
        e_peak, e_leak = reference_coefficient_errors(n_h, n_w, sub, basis_maps(n_h, n_w, sub, device))
        tol_peak, tol_leak = tolerance(e_peak.max().item()), tolerance(e_leak.max().item())
    worst_peak = worst_leak = 0.0
    for lo, hi in chunk_ranges(len(pairs), n_h * n_w * 4, chunk_bytes):
        part = pairs[lo:hi]
        c = coeff_fn(basis_maps(n_h, n_w, part, device)[None])
        assert tuple(c.shape) == (1, len(part), n_h, n_w), tuple(c.shape)
        peak, leak = _peak_and_leak(c[0], part)
        for err, tol, name in ((peak, tol_peak, "|c[u, v] - 1|"), (leak, tol_leak, "max |c| elsewhere")):
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
            w, i = err.max(dim=0)
            if not w.item() <= tol:
                raise AssertionError("basis (%d, %d): %s = %.3g > %.3g" % (int(part[int(i)][0]), int(part[int(i)][1]), name, w.item(), tol))
        worst_peak, worst_leak = max(worst_peak, peak.max().item()), max(worst_leak, leak.max().item())
        del c
    return worst_peak, worst_leak


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_pow2_scaling(energy_fn, x, k=POW2_K):
    """energy(x * 2^k) == energy(x) * 2^(2k) bit for bit, k = +-POW2_K. Derived, not measured: scaling by a power of
    two commutes with every fp32 add, multiply and FMA as long as nothing under- or overflows, and with |x| of order 1
    nothing does. Catches additive constants, epsilons and any value that does not come from the map (a zero map
    among x must stay +0.0 at every scale)."""
    e0 = energy_fn(x).float()
    for s in (k, -k):
        want = e0 * (2.0 ** (2 * s))
        got = energy_fn(x * (2.0 ** s)).float()
        if not torch.equal(_bits(got), _bits(want)):
            i = int((_bits(got) != _bits(want)).reshape(-1).nonzero()[0])
            raise AssertionError("scaling by 2^%d: map %d gives %r, energy(x) * 2^%d is %r"
                                 % (s, i, got.reshape(-1)[i].item(), 2 * s, want.reshape(-1)[i].item()))


def check_isolation(energy_fn, x):
    """One map of x [N, C, H, W] replaced by NaN, another by +inf: the call returns, every OTHER map keeps its bits,
    and the poisoned maps do not come out finite. Purely numerical."""
    e0 = energy_fn(x).reshape(-1)
    count = e0.numel()
    for value, m in ((float("nan"), count // 2), (float("inf"), count // 3)):
        y = x.clone()
        y.view(count, x.shape[2], x.shape[3])[m] = value
        e = energy_fn(y).reshape(-1)
        assert not torch.isfinite(e[m]), "map %d is all %r and scores %r" % (m, value, e[m].item())
        keep = torch.ones(count, dtype=torch.bool, device=e.device)
        keep[m] = False
        diff = keep & (_bits(e) != _bits(e0))
        if diff.any():
            i = int(diff.nonzero()[0])
            raise AssertionError("map %d filled with %r changes map %d: %r -> %r" % (m, value, i, e0[i].item(), e[i].item()))
