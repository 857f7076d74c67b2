"""tests/dct_probes.py without a GPU: (1) the reference restatement passes every checker at the tolerance rule,
which proves that the inputs and bounds can be met; (2) a float64 transform with ONE defect is caught by the checker
named for it and is NOT caught by the suite's older rule (synthetic maps, relative error <= 1e-4) at edge 224 - the
gap these probes close, written down as a test; (3) the host build of dct_codelets.hpp through the basis and the
impulse sweep, exhaustively, for the 22 codelet sizes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dct_probes as dp
from helpers import synth
from oracle import dct_oracle as orc

OLD_RTOL = 1e-4  # tests/test_gpu_parity.py: RTOL
CPU_CHUNK = 64 << 20
# edges 224 and 512: a seeded subsample of the cover (the whole cover at 512 is 10 GiB through a CPU FFT)
SHAPES = [(7, 7), (56, 56), (72, 72), (224, 224), (512, 512), (56, 28), (9, 18)]
MAX_MAPS = {224: 512, 512: 96}


def oracle_energy(x, **kw):
    return orc.energy_nc_batched(x, **kw)


def oracle_coeff(x):
    return orc.dct_2d(x)


def pairs_for(h, w):
    pairs = dp.cover(h, w)
    cap = MAX_MAPS.get(h)
    if cap is not None and len(pairs) > cap:
        g = torch.Generator().manual_seed(h)
        pairs = pairs[torch.randperm(len(pairs), generator=g)[:cap].sort().values]
    return pairs


def test_cover_reaches_every_row_column_and_residue():
    for h, w in [(224, 224), (512, 336), (144, 72)]:
        pairs = dp.cover(h, w, exhaustive=False)
        assert set(pairs[:, 0].tolist()) == set(range(h)) and set(pairs[:, 1].tolist()) == set(range(w))
        for n, k in ((h, 0), (w, 4)):
            v = dp.axis_picks(n, k)
            assert {0, 1, 2, 3, n // 2 - 1, n // 2, n - 2, n - 1} <= set(v) and {i % 8 for i in v} == set(range(8))
        full_rows = [u for u in range(h) if (pairs[:, 0] == u).sum() == w]
        assert set(dp.axis_picks(h, dp.FIXED_RANDOM_K)) == set(full_rows)
    assert len(dp.cover(64, 64)) == 64 ** 2 and len(dp.cover(128, 128)) == 128 ** 2 and len(dp.cover(136, 136)) < 136 ** 2
    assert dp.cover(1, 1).tolist() == [[0, 0]]


def test_basis_maps_are_orthonormal_and_impulses_are_single_samples():
    pairs = dp.cover(12, 10)
    b = dp.basis_maps(12, 10, pairs).double().flatten(1)
    assert (b @ b.T - torch.eye(len(pairs), dtype=torch.float64)).abs().max() <= 1e-6
    x = dp.impulse_maps(12, 10, pairs, seed=3)
    assert ((x != 0).flatten(1).sum(1) == 1).all()
    val = x[torch.arange(len(pairs)), pairs[:, 0], pairs[:, 1]]
    assert (val >= 0.5).all() and (val <= 2.0).all() and val.unique().numel() > len(pairs) // 2


@pytest.mark.parametrize("hw", SHAPES)
def test_reference_passes_every_checker(hw):
    h, w = hw
    pairs = pairs_for(h, w)
    basis = lambda p: dp.basis_maps(h, w, p)
    impulse = lambda p: dp.impulse_maps(h, w, p, seed=h + w)
    for make, what in ((basis, "basis"), (impulse, "impulse")):
        tol, e_ref = dp.sweep_tolerance(make, pairs, h, w)
        worst = dp.sweep(oracle_energy, make, pairs, h, w, tol, what, chunk_bytes=CPU_CHUNK)
        print("%dx%d %s: E_ref %.3g tol %.3g worst %.3g over %d maps" % (h, w, what, e_ref, tol, worst, len(pairs)))
    peak, leak = dp.check_coefficients(oracle_coeff, h, w, pairs, chunk_bytes=CPU_CHUNK)
    print("%dx%d coefficients: |peak - 1| %.3g leak %.3g" % (h, w, peak, leak))
    for signed in (False, True):
        x = dp.random_maps(1, 13, h, w, 5 + h, signed=signed)
        tol = dp.tolerance(dp.reference_error(x))
        dp.check_energy(oracle_energy, x, tol)
        dp.check_pow2_scaling(oracle_energy, x)
        dp.check_isolation(oracle_energy, x)
    if h % 2 == 1:  # the odd front pad keeps sum(x^2)
        x = dp.random_maps(1, 13, h, w, 6 + h, signed=True)
        tol = dp.tolerance(dp.reference_error(x, pad_front_if_odd=True))
        dp.check_energy(lambda t: oracle_energy(t, pad_front_if_odd=True), x, tol)


# ----------------------------------------------------------------------------------------------------
# mutants: a float64 transform with one defect
# ----------------------------------------------------------------------------------------------------
N = 224
U, V = 113, 2          # a row and a column of the cover (2 is in V(n); every u is swept)
I, J = 1, 77           # a sample of the cover


def f64_coefficients(x):
    return orc.dct_2d_f64(x.detach().cpu().numpy())


def mutant_weight(x):
    d2 = f64_coefficients(x) ** 2
    d2[..., U, V] *= 1.0 + 1e-4
    return torch.from_numpy(d2.sum(axis=(-2, -1))).float()


def mutant_dropped(x):
    d2 = f64_coefficients(x) ** 2
    d2[..., U, V] = 0.0
    return torch.from_numpy(d2.sum(axis=(-2, -1))).float()


def mutant_sample_zero(x):
    y = x.clone()
    y[..., I, J] = 0.0
    return torch.from_numpy(orc.energy_nc_f64(y)).float()


def mutant_sample_from_next_map(x):
    y = x.clone()
    flat = y.view(-1, y.shape[2], y.shape[3])
    flat[:-1, I, J] = x.view(-1, x.shape[2], x.shape[3])[1:, I, J]
    return torch.from_numpy(orc.energy_nc_f64(y)).float()


def mutant_additive(x):
    return torch.from_numpy(orc.energy_nc_f64(x)).float() + 1e-30


def mutant_nan_spreads(x):
    e = torch.from_numpy(orc.energy_nc_f64(x)).float().reshape(-1)
    bad = torch.isnan(e).nonzero().reshape(-1)
    e[(bad + 1) % e.numel()] = float("nan")
    return e.view(x.shape[0], x.shape[1])


def old_rule_passes(energy_fn):
    x = synth(1, 6, N, N, 10 + N)
    got, ref = energy_fn(x).double(), orc.energy_nc_batched(x).double()
    nz = ref != 0
    return ((got - ref).abs() / ref.abs().clamp_min(1e-30))[nz].max().item() <= OLD_RTOL and bool((got[~nz] == 0).all())


def line_of_cover(n, fixed, axis):
    """The pairs of the cover on one line: u = fixed (axis 0) or v = fixed (axis 1)."""
    pairs = dp.cover(n, n)
    return pairs[pairs[:, axis] == fixed]


@pytest.mark.parametrize("mutant", [mutant_weight, mutant_dropped])
def test_basis_sweep_catches_one_wrong_coefficient(mutant):
    pairs = line_of_cover(N, V, 1)
    assert [U, V] in pairs.tolist() and len(pairs) == N
    make = lambda p: dp.basis_maps(N, N, p)
    tol, _ = dp.sweep_tolerance(make, pairs, N, N)
    with pytest.raises(AssertionError, match=r"basis \(%d, %d\)" % (U, V)):
        dp.sweep(mutant, make, pairs, N, N, tol, "basis", chunk_bytes=CPU_CHUNK)
    assert old_rule_passes(mutant)


@pytest.mark.parametrize("mutant", [mutant_sample_zero, mutant_sample_from_next_map])
def test_impulse_sweep_catches_one_wrong_sample(mutant):
    pairs = line_of_cover(N, I, 0)
    assert [I, J] in pairs.tolist() and len(pairs) == N
    make = lambda p: dp.impulse_maps(N, N, p, seed=1)
    tol, _ = dp.sweep_tolerance(make, pairs, N, N)
    # read from the next map, the map in front of the impulse at (I, J) gains that sample and is the worse of the two
    with pytest.raises(AssertionError, match=r"impulse \(%d, (%d|%d)\)" % (I, J - 1, J)):
        dp.sweep(mutant, make, pairs, N, N, tol, "impulse", chunk_bytes=CPU_CHUNK)
    assert old_rule_passes(mutant)


def test_pow2_scaling_catches_an_additive_constant():
    x = dp.random_maps(1, 13, N, N, 3, signed=True)
    with pytest.raises(AssertionError, match="scaling by 2"):
        dp.check_pow2_scaling(mutant_additive, x)
    assert old_rule_passes(lambda t: mutant_additive(t) * (orc.energy_nc_f64(t) != 0))  # dead channels aside (the old rule wants +0.0)
    dp.check_pow2_scaling(lambda t: torch.from_numpy(orc.energy_nc_f64(t)).float(), x)


def test_isolation_catches_a_nan_that_spreads():
    x = dp.random_maps(1, 13, N, N, 4, signed=True)
    with pytest.raises(AssertionError, match="changes map"):
        dp.check_isolation(mutant_nan_spreads, x)
    assert old_rule_passes(mutant_nan_spreads)


# ----------------------------------------------------------------------------------------------------
# the header the kernels include, compiled for the host
# ----------------------------------------------------------------------------------------------------
FP = ctypes.POINTER(ctypes.c_float)
CODELET = [2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 48, 56, 60, 64]


@pytest.fixture(scope="module")
def lib(repo_root):
    d = os.path.join(repo_root, "tests", "native")
    subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return ctypes.CDLL(os.path.join(d, "_build", "libcodelet_host.so"))


@pytest.mark.parametrize("n", CODELET)
def test_host_codelets_per_coefficient_and_per_sample(lib, n):
    def host_energy(x):
        maps = np.ascontiguousarray(x.reshape(-1, n, n).numpy())
        out = np.zeros(len(maps), np.float32)
        e = ctypes.c_float()
        for i, m in enumerate(maps):
            assert lib.codelet_energy_2d(n, m.ctypes.data_as(FP), None, ctypes.byref(e)) == 0
            out[i] = e.value
        return torch.from_numpy(out).view(x.shape[0], x.shape[1])

    pairs = dp.cover(n, n)
    assert len(pairs) == n * n
    for make, what in ((lambda p: dp.basis_maps(n, n, p), "basis"), (lambda p: dp.impulse_maps(n, n, p, seed=n), "impulse")):
        tol, _ = dp.sweep_tolerance(make, pairs, n, n)
        dp.sweep(host_energy, make, pairs, n, n, tol, what)
