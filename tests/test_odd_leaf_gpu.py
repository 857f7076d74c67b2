"""The odd-length DCT-IV leaf (dct_codelets.hpp, odd M >= 5) on the GPU, at the smallest shapes that reach each leaf
through each kernel family: edges 2^s * M through the codelet kernels and k_energy_rect, 2G+1 maps each (a ragged last
group), and the large tiles through k_tile2g, k_tile2d and k_split_fused2 with 3 maps each. Coefficients against the
float64 oracle, single basis functions, zero maps, and the multi-tensor entry against the single-tensor one."""
import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import grid_capacity as cap
from oracle import dct_oracle as orc
from helpers import synth

pytestmark = pytest.mark.gpu

TOL = 2e-6        # of max |coefficient|: the bound of the coefficient tests of test_gpu_parity.py and test_gpu_coeff_large.py
BASIS_TOL = 5e-6  # absolute, unit coefficient: the bound of the single-basis tests of test_gpu_coeff_large.py

# edge -> odd part M
SMALL = {10: 5, 20: 5, 40: 5, 14: 7, 28: 7, 56: 7, 18: 9, 36: 9, 60: 15, 22: 11, 26: 13, 62: 31}
LARGE = {72: 9, 80: 5, 112: 7, 224: 7, 288: 9, 320: 5}


def algos(edge):
    """The families a shape is sent through by name, besides the library's own choice."""
    if edge in LARGE:
        return ["AUTO", "FUSED"] + (["TILE2D"] if edge <= 224 else [])
    return ["AUTO", "RECT"] if edge in cap.CODELET_SIZES else ["AUTO"]


def count(edge, at_least=0):
    """2G+1 maps for the small shapes (G of the codelet and of the rect kernel, whichever is larger), never a multiple
    of either group size where that is above 1; 3 maps for the large tiles."""
    if edge in LARGE:
        return 3
    gs = [64 // edge, cap.rect_group(edge, edge).G, cap.rect_group(edge, edge, store_coeff=True).G]
    n = max(2 * max(gs) + 1, at_least)
    while any(g > 1 and n % g == 0 for g in gs):
        n += 1
    return n


def leaf_rows(edge):
    """Output indices of Dct2<edge> that the odd DCT-IV leaf writes: 2^(s-1) (2j+1), j < M, edge = 2^s M."""
    m = {**SMALL, **LARGE}[edge]
    half = edge // m // 2
    return [half * (2 * j + 1) for j in range(m)]


def basis(n, u):
    k = np.arange(n)
    return np.cos(np.pi * (2 * k + 1) * u / (2 * n)) * (np.sqrt(1.0 / n) if u == 0 else np.sqrt(2.0 / n))


CASES = [(e, a) for e in list(SMALL) + list(LARGE) for a in algos(e)]


@pytest.mark.parametrize("edge,algo", CASES)
def test_coefficients_vs_float64(edge, algo):
    x = synth(1, count(edge), edge, edge, 7000 + edge, dead=False)
    got = dpa.dct2d(x.cuda(), algo=getattr(dpa, "ALGO_" + algo)).cpu().numpy()
    ref = orc.dct_2d_f64(x.numpy())
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("ODD-LEAF coeff %d %s maps=%d err=%.3g" % (edge, algo, x.shape[1], err))
    assert got.shape == ref.shape and err <= TOL


@pytest.mark.parametrize("edge,algo", CASES)
def test_single_basis_function(edge, algo):
    """x = outer(C[u, :], C[v, :]) has one unit coefficient, at (u, v); u and v run over the rows the leaf writes."""
    rows = leaf_rows(edge)
    picks = list(zip(rows, rows[::-1])) + [(0, rows[0]), (rows[-1], 0), (edge - 1, edge - 1), (1, rows[len(rows) // 2])]
    if edge in LARGE:
        picks = [picks[0], picks[len(rows) // 2 + 1], picks[-1]]
    n = count(edge, at_least=len(picks))
    x = np.stack([np.outer(basis(edge, u), basis(edge, v)) for u, v in (picks[i % len(picks)] for i in range(n))])
    got = dpa.dct2d(torch.from_numpy(x[None].astype(np.float32)).cuda(), algo=getattr(dpa, "ALGO_" + algo)).cpu().numpy()[0]
    for i in range(n):
        want = np.zeros((edge, edge))
        want[picks[i % len(picks)]] = 1.0
        assert np.abs(got[i] - want).max() <= BASIS_TOL, (picks[i % len(picks)], i)


@pytest.mark.parametrize("edge,algo", CASES)
def test_zero_maps_score_plus_zero(edge, algo):
    a = getattr(dpa, "ALGO_" + algo)
    n = count(edge)
    e = dpa.energy_nc(torch.zeros(1, n, edge, edge).cuda(), algo=a).cpu()
    assert (e == 0).all() and not torch.signbit(e).any()
    x = synth(1, n, edge, edge, 7100 + edge, dead=False)
    x[:, 1] = 0
    e = dpa.energy_nc(x.cuda(), algo=a).cpu()
    assert e[0, 1] == 0 and not torch.signbit(e[0, 1]) and (e[0, [0, 2]] > 0).all()
    ref = orc.energy_nc(x)
    assert ((e - ref).abs() <= 1e-5 * ref.abs()).all()


@pytest.mark.parametrize("edge", [7, 14, 28, 56])
def test_multi_entry_equals_single_entry_bit_for_bit(edge):
    """dcts_energy_multi_f32 against dcts_energy_f32 per tensor; 7 x 7 has no odd DCT-IV and is the control."""
    g = 64 if edge == 7 else 64 // edge
    xs = [synth(1, 2 * g + 1, edge, edge, 7200 + edge).cuda(), synth(2, g + 1, edge, edge, 7300 + edge).cuda()]
    multi = dpa.energy_multi([(x, 0, None) for x in xs])
    for x, m in zip(xs, multi):
        single = dpa.energy_nc(x)
        assert torch.equal(single.view(torch.int32), m.view(torch.int32))
        ref = orc.energy_nc(x.cpu())
        assert ((single.cpu() - ref).abs() <= 1e-5 * ref.abs()).all()
