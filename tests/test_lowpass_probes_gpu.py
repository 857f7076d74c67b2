"""k_lowpass_codelet<N> at every codelet edge (each edge is an instantiation of its own: group size, slab strides, idle lanes)
and on both store chains of its epilogue: every coefficient of every basis function, every K as the corner of K = n bit for
bit, an aligned and a misaligned `out`, and drop_dc with the flat rule in every position of a wave's group.

The scalar chain stores w[v] * sc one float at a time, the 16-byte chain four at a time; the kernel takes the second where a
wave holds several maps (G = 64 // n >= 2), K is a multiple of 4 and `out` is 16-byte aligned. Both store the lone product
w[v] * sc of the same registers, and K is a run-time argument of one binary, so whatever K, chain or alignment a call has,
an element it writes has the bits of the same element of the K = n call. That is derived, not measured: a difference is a
defect. Every figure is printed before it is asserted (`pytest -s`: lines starting with LOWPASS)."""
import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import dct_probes as dp
import lowpass_oracle as lo
from helpers import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = lo.SIG_TOL

EDGES = lo.CODELET_EDGES
GROUPED = [n for n in EDGES if lo.group_size(n) >= 2]  # several maps per wave: the edges that have the 16-byte chain ...
VECTOR = [n for n in GROUPED if n >= 4]                # ... and a K <= n that takes it


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_edge_lists():
    assert [e for e in range(1, 65) if dpa.has_codelet(e, e)] == list(EDGES) and len(EDGES) == 22
    assert GROUPED == [2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32] and VECTOR == GROUPED[1:]
    for n in EDGES:
        vec, scalar = lo.chain_sizes(n)
        assert (vec is not None) == (n in VECTOR) and 1 <= scalar <= n
        assert vec is None or (vec <= n and lo.on_vector_chain(n, vec))
        assert not lo.on_vector_chain(n, scalar)


# ----------------------------------------------------------------------------------------------------
# every coefficient
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGES)
def test_basis_sweep(n):
    """Basis function (u, v), all n * n of them in one launch: element [u][v] of the K = n signature is 1, every other one 0,
    within dct_probes' rule (8 x the fp32 reference's own coefficient error, floor 2^-22)."""
    pairs = dp.cover(n, n, exhaustive=True)
    peak, leak = dp.check_coefficients(lambda x: dpa.lowpass_nc(x, n), n, n, pairs, device=DEV)
    print("LOWPASS basis sweep %dx%d maps=%d peak=%.3g leak=%.3g" % (n, n, len(pairs), peak, leak))


@pytest.mark.parametrize("n", EDGES)
def test_every_corner_is_the_corner_of_the_whole_map(n):
    """lowpass_nc(x, K) == lowpass_nc(x, n)[..., :K, :K] in bits, for every K of the float64 test, on the basis sweep (the
    unit coefficient walks over the whole tile, so a lane that stores another row's registers or an offset that is off by
    one shows) and on random maps with a ragged last group."""
    G = lo.group_size(n)
    basis = dp.basis_maps(n, n, dp.cover(n, n, exhaustive=True), device=DEV)[None]
    rand = synth(1, 3 * G + 1, n, n, 500 + n, dead=True).to(DEV)
    sizes = lo.corner_sizes(n)
    for what, x in (("basis", basis), ("random", rand)):
        whole = dpa.lowpass_nc(x, n)
        assert whole.shape == (1, x.shape[1], n, n)
        for K in sizes:
            got = dpa.lowpass_nc(x, K)
            assert got.shape == (1, x.shape[1], K, K)
            diff = _bits(got) != _bits(whole[..., :K, :K])
            if bool(diff.any()):
                m, u, v = (int(i) for i in diff[0].nonzero()[0])
                raise AssertionError("edge %d K=%d %s map %d: [%d][%d] is %r, the K = n call has %r"
                                     % (n, K, what, m, u, v, got[0, m, u, v].item(), whole[0, m, u, v].item()))
    print("LOWPASS corners %dx%d G=%d K=%s 16-byte chain at K=%s: the bits of K = n on %d basis and %d random maps"
          % (n, n, G, sizes, [K for K in sizes if lo.on_vector_chain(n, K)], basis.shape[1], rand.shape[1]))


# ----------------------------------------------------------------------------------------------------
# aligned and misaligned out
# ----------------------------------------------------------------------------------------------------
def _into(x, K, drop_dc, guard):
    """The call with out= a view `guard` floats into a NaN-filled buffer: (the view, both guards intact)."""
    oshape = (1, x.shape[1], K, K)
    count = int(np.prod(oshape))
    tail = 64
    buf = torch.full((guard + count + tail,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:guard] = 1234.5
    buf[guard + count:] = -4321.5
    out = buf[guard:guard + count].view(oshape)
    ret = dpa.lowpass_nc(x, K, drop_dc=drop_dc, out=out)
    assert ret.data_ptr() == out.data_ptr()
    intact = bool((buf[:guard] == 1234.5).all()) and bool((buf[guard + count:] == -4321.5).all())
    return out, intact


@pytest.mark.parametrize("drop_dc", [False, True])
@pytest.mark.parametrize("n", VECTOR)
def test_aligned_and_misaligned_out(n, drop_dc):
    """An `out` that starts one float behind a 16-byte boundary takes the scalar chain, an aligned one the 16-byte chain:
    the same bits, those of the call without out=, and not a float outside the view."""
    G = lo.group_size(n)
    x = synth(1, 3 * G + 1, n, n, 1500 + n, dead=True)
    x[0, 1] = 3.7   # flat maps in a group with live ones
    x[0, G] = -1.25
    xd = x.to(DEV)
    sizes = [K for K in lo.corner_sizes(n) if K % 4 == 0]
    assert sizes and all(lo.on_vector_chain(n, K) for K in sizes)
    for K in sizes:
        plain = dpa.lowpass_nc(xd, K, drop_dc=drop_dc)
        assert plain.data_ptr() % 16 == 0
        al, al_ok = _into(xd, K, drop_dc, 64)
        mis, mis_ok = _into(xd, K, drop_dc, 65)
        assert al.data_ptr() % 16 == 0 and mis.data_ptr() % 16 == 4
        assert not lo.on_vector_chain(n, K, aligned=False)
        assert al_ok and mis_ok, (n, K, al_ok, mis_ok)
        assert bool(torch.isfinite(al).all()) and bool(torch.isfinite(mis).all())  # every element written
        assert torch.equal(_bits(al), _bits(mis)), (n, K)
        assert torch.equal(_bits(al), _bits(plain)), (n, K)
    print("LOWPASS alignment %dx%d G=%d drop_dc=%d K=%s: aligned, misaligned and own output bit-identical, guards intact"
          % (n, n, G, drop_dc, sizes))


# ----------------------------------------------------------------------------------------------------
# drop_dc on both chains
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GROUPED)
def test_drop_dc_on_both_chains(n):
    """tests/test_lowpass_gpu.py::test_drop_dc's assertions where a wave holds several maps, for one K on each chain and two
    complementary patterns (flat iff the channel is even, flat iff it is odd): every position of a group holds a flat map
    beside maps that are not, and the reverse. Among those that are not: constant except for the last element, except for
    the first, and except for one NaN - not flat, its signature stays NaN, and no other map's bits change."""
    G = lo.group_size(n)
    vec, scalar = lo.chain_sizes(n)
    for parity in (0, 1):
        x, kinds = lo.flat_pattern_maps(n, parity)
        C = x.shape[1]
        assert C >= 2 * G + 1 and set(kinds) == {"flat"} | set(lo.NOT_FLAT)
        flat = np.array([k == "flat" for k in kinds])
        assert lo.flat_maps(x).tolist() == [flat.tolist()]
        nan = np.array([k == "nan" for k in kinds])
        finite = torch.from_numpy(~nan)
        xd = x.to(DEV)
        healed = x.clone()
        healed[0, torch.from_numpy(nan)] = 3.7  # the NaN maps replaced: what the other maps must not notice
        scale = lo.coefficient_scale(x[:, finite])
        for K in [k for k in (vec, scalar) if k is not None]:
            chain = "16-byte" if lo.on_vector_chain(n, K) else "scalar"
            plain, drop = dpa.lowpass_nc(xd, K), dpa.lowpass_nc(xd, K, drop_dc=True)
            assert drop.shape == (1, C, K, K) and drop.data_ptr() % 16 == 0
            pb, db = _bits(plain).cpu(), _bits(drop).cpu()
            # the definition, on the maps without a NaN
            ref = lo.lowpass_f64(x[:, finite], K, drop_dc=True)
            g = drop.cpu().numpy()[:, ~nan]
            assert np.isfinite(g).all(), (n, K)
            err = np.abs(g - ref).max() / scale
            print("LOWPASS drop_dc %dx%d G=%d K=%d (%s chain) flat iff c %% 2 == %d, %d maps: worst |got - f64| / max |coeff| = %.3e (tol %.1e)"
                  % (n, n, G, K, chain, parity, C, err, TOL))
            assert err <= TOL, (n, K, parity, err)
            # flat maps: +0.0 in every element, sign bit included
            assert (db[0, torch.from_numpy(flat)] == 0).all(), (n, K, parity)
            # the others: +0.0 at [0, 0], every other element the bits of the call without the flag
            live = torch.from_numpy(~flat)
            assert (db[0, live, 0, 0] == 0).all(), (n, K, parity)
            rest = torch.ones(K, K, dtype=torch.bool)
            rest[0, 0] = False
            assert torch.equal(db[0, live][:, rest], pb[0, live][:, rest]), (n, K, parity)
            if K > 1:
                for kind in ("last", "first"):
                    j = kinds.index(kind)
                    assert float(drop[0, j].abs().max()) > 0, (n, K, kind)
            # a map with a NaN keeps a NaN signature (its DC term sums every element) and touches no other map
            assert bool(torch.isnan(plain[0, torch.from_numpy(nan), 0, 0]).all()), (n, K)
            if K > 1:
                assert bool(torch.isnan(drop[0, torch.from_numpy(nan)]).flatten(1).any(dim=1).all()), (n, K)
            for flag, with_nan in ((False, pb), (True, db)):
                clean = _bits(dpa.lowpass_nc(healed.to(DEV), K, drop_dc=flag)).cpu()
                assert torch.equal(with_nan[0, finite], clean[0, finite]), (n, K, parity, flag)
