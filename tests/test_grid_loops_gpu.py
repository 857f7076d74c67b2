"""Every capped, grid-stride kernel with more work than one grid holds ("grid-stride loops").

Each case scores ceil(2.3 x capacity) + r maps, capacity from tests/grid_capacity.py for this device's CU count and r so
that the map count is no multiple of the group and the group count no multiple of the grid: some waves run three
iterations, others two, and the ragged group comes last. The maps are a bank of 251 gathered through a seeded random
index (tests/loop_cases.py), so every one of the millions of outputs is checked on the device against (a) the float64
oracle of the bank within the bound the entry point's own test module uses and (b) bit for bit the same entry point's
call on the bank alone; every entry finite, +0.0 for zero maps, in NaN-filled outputs with a NaN guard behind them.

The persistent kernels (PREFETCH, LANE through energy_nc, FUSED, PIPE, TILE2D / 2G, DIRECT) are tested with more maps than
workgroups by test_gpu_parity.py (test_codelet_sizes' 40 x 77 PREFETCH maps, test_lane_per_map_kernel, the fused / pipe / tile2d
tests) and are not repeated here."""
import time

import numpy as np
import pytest
import torch

import band_oracle as bo
import dct_probes as dp
import dct_pruning_amd as dpa
import grid_capacity as gc
import loop_cases as lc
import rank_oracle as ro
from dct_pruning_amd import ops
from oracle import dct_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = lc.B
RTOL = 1e-4        # test_gpu_parity.py: fp32 energies
COEFF_TOL = 2e-6   # test_gpu_parity.py: coefficients, relative to the map's largest
WEIGHTED_TOL = 2e-5  # test_gpu_parity.py: weighted energies with weights in [0, 1)
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _need(nbytes, what):
    """A case that needs more device memory than is free fails with a message (it is never skipped)."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert free >= nbytes, "%s needs %.2f GiB of device memory, %.2f GiB are free" % (what, nbytes / 2 ** 30, free / 2 ** 30)
    assert nbytes <= 6 << 30, "%s would take %.2f GiB: a case stays under 6 GiB" % (what, nbytes / 2 ** 30)


class _GuardedTorch:
    """Stands in for the `torch` name inside dct_pruning_amd.ops while a case runs: every float32 output an entry point
    allocates with torch.empty comes out of a NaN-filled buffer with lc.GUARD NaN floats behind it, which check() then
    inspects. Everything else is torch's own."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        if kw.get("dtype") != torch.float32:
            return torch.empty(*shape, **kw)
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        n = int(np.prod(shape))
        buf = torch.full((n + lc.GUARD,), float("nan"), dtype=torch.float32, device=kw.get("device"))
        self.bufs.append((buf, n))
        return buf[:n].view(shape)

    def check(self, what, outputs):
        """`outputs`: how many float32 outputs the case's calls into ops return. An entry point that allocated one in
        another way (empty_like, zeros ...) would leave it without NaN fill and guard: the count says so."""
        assert len(self.bufs) == outputs, "%s: %d outputs came through the guarded torch.empty, %d calls were made" % (what, len(self.bufs), outputs)
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[n:]).all()), "%s: the guard behind an output was written" % what


@pytest.fixture
def guarded(monkeypatch):
    g = _GuardedTorch()
    monkeypatch.setattr(ops, "torch", g)
    return g


def _report(name, nmaps, units, per, worst, tol, t0):
    torch.cuda.synchronize()
    lo, hi = gc.iterations(nmaps, units, per)
    print("GRIDLOOP %s maps=%d grid=%d x %d iterations=%d..%d worst=%.3g tol=%.3g secs=%.2f"
          % (name, nmaps, units, per, lo, hi, worst, tol, time.time() - t0))
    assert (lo, hi) == (2, 3), (name, lo, hi)


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _energy_refs(bank, pad=False):
    """(ref64 [B] on the device, the bound of the half / nhwc modules on this bank)."""
    x = bank.float()[None]
    return _f64(orc.energy_nc_f64(x, pad_front_if_odd=pad)[0]), dp.tolerance(dp.reference_error(x, pad_front_if_odd=pad))


def _gather(bank_dev, idx, shape):
    return bank_dev[idx].view(shape)


# ----------------------------------------------------------------------------------------------------
# k_energy_codelet
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.CODELET_SIZES)
def test_codelet_pad0(n, guarded):
    t0 = time.time()
    cap = gc.codelet(n, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(nmaps * n * n * 4 + (64 << 20), "codelet %d" % n)
    bank = lc.make_bank(n, n, 100 + n)
    ref64, _ = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 7 * n, DEV)
    x = _gather(bd, idx, (1, nmaps, n, n))
    got = dpa.energy_nc(x, algo=dpa.ALGO_CODELET)
    twin = dpa.energy_nc(bd[None], algo=dpa.ALGO_CODELET)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, RTOL, what="codelet %d" % n, group=cap.maps_per_unit, units=cap.units)
    if n not in (7, 9):  # AUTO = this kernel (test_codelet_sizes): the same bits
        assert torch.equal(dpa.energy_nc(x), got)
    guarded.check("codelet %d" % n, 2 if n in (7, 9) else 3)
    _report("codelet-pad0 %d" % n, nmaps, cap.units, cap.maps_per_unit, worst, RTOL, t0)


@pytest.mark.parametrize("n", [9, 55])  # the dispatch trace: 9 x 9 p1 -> codelet 10 x 10 p1, 55 x 55 p1 -> codelet 56 x 56 p1
def test_codelet_pad1(n, guarded):
    t0 = time.time()
    cap = gc.codelet(n + 1, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(nmaps * n * n * 4 + (64 << 20), "codelet pad %d" % n)
    bank = lc.make_bank(n, n, 200 + n)
    ref64, _ = _energy_refs(bank, pad=True)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 11 * n, DEV)
    got = dpa.energy_nc(_gather(bd, idx, (1, nmaps, n, n)), pad_front_if_odd=True)
    twin = dpa.energy_nc(bd[None], pad_front_if_odd=True)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, RTOL, what="codelet pad %d" % n, group=cap.maps_per_unit, units=cap.units)
    guarded.check("codelet pad %d" % n, 2)
    _report("codelet-pad1 %d" % n, nmaps, cap.units, cap.maps_per_unit, worst, RTOL, t0)


@pytest.mark.parametrize("n", [4, 16])
def test_codelet_coefficients(n, guarded):
    t0 = time.time()
    cap = gc.codelet(n, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(2 * nmaps * n * n * 4 + (512 << 20), "coefficients %d" % n)
    bank = lc.make_bank(n, n, 300 + n)
    c64 = orc.dct_2d_f64(bank.numpy())
    ref64, peak = _f64(c64), _f64(np.abs(c64).max(axis=(1, 2)))
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 13 * n, DEV)
    got = dpa.dct2d(_gather(bd, idx, (1, nmaps, n, n)), algo=dpa.ALGO_CODELET)
    twin = dpa.dct2d(bd[None], algo=dpa.ALGO_CODELET)[0]
    # coefficients, not scores: those of a zero map are zeros of either sign (check_scores), bitwise the bank call's
    worst = lc.check_scores(got[0], idx, ref64, twin, COEFF_TOL, denom64=peak, what="coefficients %d" % n,
                            group=cap.maps_per_unit, units=cap.units, signed_zero=True)
    guarded.check("coefficients %d" % n, 2)
    _report("codelet-coeff %d" % n, nmaps, cap.units, cap.maps_per_unit, worst, COEFF_TOL, t0)


@pytest.mark.parametrize("n", [8, 56])
def test_codelet_channel_slice_of_a_batch_strided_view(n, guarded):
    """c_begin > 0, c_count < C, strideN != C * strideC: map_base divides and does its 64-bit strided arithmetic in every
    iteration. The channels around the slice and the gap between samples hold 3.0: a map read from there is no bank map."""
    t0 = time.time()
    cc, ctot, cb = 13, 15, 1
    cap = gc.codelet(n, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit, multiple_of=cc)
    N = nmaps // cc
    _need(N * (ctot + 1) * n * n * 4 + nmaps * n * n * 4 + (64 << 20), "strided %d" % n)
    bank = lc.make_bank(n, n, 400 + n)
    ref64, _ = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 17 * n, DEV)
    big = torch.full((N, ctot + 1, n, n), 3.0, device=DEV)
    big[:, cb:cb + cc] = _gather(bd, idx, (N, cc, n, n))
    x = big[:, :ctot]
    assert x.stride(0) != ctot * x.stride(1) and not x.is_contiguous()
    got = dpa.energy_nc(x, c_begin=cb, c_count=cc, algo=dpa.ALGO_CODELET)
    twin = dpa.energy_nc(bd[None], algo=dpa.ALGO_CODELET)[0]
    worst = lc.check_scores(got.reshape(-1), idx, ref64, twin, RTOL, what="strided %d" % n, group=cap.maps_per_unit, units=cap.units)
    guarded.check("strided %d" % n, 2)
    _report("codelet-strided %d" % n, nmaps, cap.units, cap.maps_per_unit, worst, RTOL, t0)


# ----------------------------------------------------------------------------------------------------
# the multi-tensor kernels
# ----------------------------------------------------------------------------------------------------
def _multi_sizes(first_total, chunk):
    """More tensors than one launch takes (`chunk` = kMultiItems or kMixedItems): the first launch holds first_total maps
    in `chunk` tensors (one a quarter of them, runs of 1-map tensors between large ones), twelve more follow."""
    return (lc.multi_sizes(first_total, count=chunk, runs=((5, 4), (17, 3), (chunk - 6, 4)))
            + lc.multi_sizes(max(64, first_total // 8), count=12, runs=((3, 3),)))


@pytest.mark.parametrize("n", [2, 8, 56, 7])
def test_energy_multi(n, guarded):
    """k_energy_codelet_multi (2, 8, 56) and k_energy_lane_multi (7): the `t` walk carried across iterations. The lane
    kernel's grid is one residency, taken as cus x 16 workgroups: a safe upper bound (grid_capacity.py), so the case
    loops at least 2.3 times."""
    t0 = time.time()
    cap = gc.lane_multi(_cus()) if n == 7 else gc.codelet(n, _cus())
    G, units = cap.maps_per_unit, cap.units
    total = gc.loop_count(units, G)
    sizes = _multi_sizes(total, gc.MULTI_ITEMS)
    while lc.multi_layout(sizes[:gc.MULTI_ITEMS], G)[1] % units == 0 or lc.multi_layout(sizes[:gc.MULTI_ITEMS], G)[1] < 23 * units // 10:
        total += G + 1
        sizes = _multi_sizes(total, gc.MULTI_ITEMS)
    groups = lc.multi_layout(sizes[:gc.MULTI_ITEMS], G)[1]
    assert len(sizes) >= 40 and groups * 10 >= 23 * units
    nmaps = sum(sizes)
    _need(nmaps * n * n * 4 + (64 << 20), "multi %d" % n)
    bank = lc.make_bank(n, n, 500 + n)
    ref64, _ = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 19 * n, DEV)
    flat = bd[idx]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    xs = [flat[offs[i]:offs[i + 1]].view(1, sizes[i], n, n) for i in range(len(sizes))]
    outs = dpa.energy_multi([(x, 0, None) for x in xs])
    twin = dpa.energy_nc(bd[None])[0]
    worst = 0.0
    for i, (x, out) in enumerate(zip(xs, outs)):
        what = "multi %d tensor %d of %d maps" % (n, i, sizes[i])
        worst = max(worst, lc.check_scores(out[0], idx[offs[i]:offs[i + 1]], ref64, twin, RTOL, what=what, group=G))
        assert torch.equal(out, dpa.energy_nc(x)), what  # its own call: the same bits
    guarded.check("multi %d" % n, 2 * len(sizes) + 1)
    _report("multi %d (%d tensors)" % (n, len(sizes)), groups * G, units, G, worst, RTOL, t0)


def test_energy_mixed(guarded):
    """k_energy_codelet_mixed over edges 2 ... 32; its persistent grid taken as cus x 16 workgroups of four waves (a safe
    upper bound, grid_capacity.py). Sizes are counted in groups, so every tensor's map count follows from its edge."""
    t0 = time.time()
    units = gc.mixed_groups(_cus())
    groups_first = gc.loop_count(units, 1)
    gsizes = _multi_sizes(groups_first, gc.MIXED_ITEMS)
    edges = [gc.MIXED_SIZES[(3 * i) % 5] for i in range(len(gsizes))]
    sizes = [1 if g == 1 else g * (64 // e) - 1 for g, e in zip(gsizes, edges)]  # 1-map tensors; a ragged last group in the others
    total_groups = sum(-(-s // (64 // e)) for s, e in list(zip(sizes, edges))[:gc.MIXED_ITEMS])
    assert len(sizes) >= 40 and total_groups * 10 >= 23 * units and total_groups % units != 0
    _need(sum(s * e * e * 4 for s, e in zip(sizes, edges)) + (64 << 20), "mixed")
    banks = {e: lc.make_bank(e, e, 600 + e) for e in gc.MIXED_SIZES}
    refs = {e: _energy_refs(banks[e])[0] for e in banks}
    bds = {e: banks[e].to(DEV) for e in banks}
    twins = {e: dpa.energy_nc(bds[e][None])[0] for e in banks}
    idxs = [lc.random_index(s, 23 * i + 1, DEV) for i, s in enumerate(sizes)]
    xs = [bds[e][idx].view(1, -1, e, e) for e, idx in zip(edges, idxs)]
    outs = dpa.energy_mixed([(x, 0, None, False) for x in xs])
    worst = 0.0
    for i, (x, out, e) in enumerate(zip(xs, outs, edges)):
        what = "mixed tensor %d: %d maps of edge %d" % (i, sizes[i], e)
        worst = max(worst, lc.check_scores(out[0], idxs[i], refs[e], twins[e], RTOL, what=what, group=64 // e))
        assert torch.equal(out, dpa.energy_nc(x)), what
    guarded.check("mixed", 2 * len(sizes) + len(banks))
    _report("mixed (%d tensors)" % len(sizes), total_groups, units, 1, worst, RTOL, t0)


# ----------------------------------------------------------------------------------------------------
# band and weighted energies
# ----------------------------------------------------------------------------------------------------
def _band_refs(bank, w, **kw):
    x = bank[None]
    e_ref = bo.band_error(bo.band_energy_nc_f32(x, w, **kw), x, w, **kw)
    return _f64(bo.band_energy_nc_f64(x, w, **kw)[0]), _f64(bo.map_energy_f64(x)[0]), dp.tolerance(e_ref)


@pytest.mark.parametrize("n,K", [(2, 3), (8, 3), (14, 3), (56, 3), (16, 8)])
def test_band_codelet(n, K, guarded):
    t0 = time.time()
    cap = gc.codelet(n, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(nmaps * n * n * 4 + (64 << 20), "band %d" % n)
    bank = lc.make_bank(n, n, 700 + n)
    w = torch.randn(K, n, n, generator=torch.Generator().manual_seed(n))  # arbitrary signed weights
    ref64, emap, tol = _band_refs(bank, w)
    bd, wd = bank.to(DEV), w.to(DEV)
    idx = lc.random_index(nmaps, 29 * n, DEV)
    got = dpa.band_energy_nc(_gather(bd, idx, (1, nmaps, n, n)), wd, algo=dpa.ALGO_CODELET)
    twin = dpa.band_energy_nc(bd[None], wd, algo=dpa.ALGO_CODELET)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, tol, denom64=emap, what="band %d K=%d" % (n, K),
                            group=cap.maps_per_unit, units=cap.units)
    guarded.check("band %d" % n, 2)
    _report("band-codelet %d K=%d" % (n, K), nmaps, cap.units, cap.maps_per_unit, worst, tol, t0)


def test_band_fallback_reduce(guarded):
    """ALGO_DIRECT at 9 x 9: coefficients of a chunk, then ONE k_band_reduce launch over the chunk's maps - enough maps
    for its 4096 x 4 waves to loop, and few enough to stay inside one chunk."""
    t0 = time.time()
    n, K = 9, 3
    cap = gc.reduce()
    nmaps = gc.loop_count(cap.units, 1)
    assert nmaps <= gc.band_fallback_chunk_maps(n, n)
    bank = lc.make_bank(n, n, 709)
    w = torch.randn(K, n, n, generator=torch.Generator().manual_seed(9))
    ref64, emap, tol = _band_refs(bank, w)
    bd, wd = bank.to(DEV), w.to(DEV)
    idx = lc.random_index(nmaps, 31, DEV)
    got = dpa.band_energy_nc(_gather(bd, idx, (1, nmaps, n, n)), wd, algo=dpa.ALGO_DIRECT)
    twin = dpa.band_energy_nc(bd[None], wd, algo=dpa.ALGO_DIRECT)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, tol, denom64=emap, what="band fallback")
    guarded.check("band fallback", 2)
    _report("band-reduce 9", nmaps, cap.units, 1, worst, tol, t0)


def test_weighted_energy(guarded):
    """k_weighted_energy: one launch per sample over the sample's channels, 4096 x 4 waves, one map per wave."""
    t0 = time.time()
    n = 8
    cap = gc.reduce()
    nmaps = gc.loop_count(cap.units, 1)
    bank = lc.make_bank(n, n, 808)
    w = torch.rand(n, n, generator=torch.Generator().manual_seed(8))
    ref64 = _f64(orc.weighted_energy_nc_f64(bank[None], w.numpy())[0])
    bd, wd = bank.to(DEV), w.to(DEV)
    idx = lc.random_index(nmaps, 37, DEV)
    got = dpa.weighted_energy_nc(_gather(bd, idx, (1, nmaps, n, n)), wd)
    twin = dpa.weighted_energy_nc(bd[None], wd)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, WEIGHTED_TOL, what="weighted")
    guarded.check("weighted", 2)
    _report("weighted 8", nmaps, cap.units, 1, worst, WEIGHTED_TOL, t0)


# ----------------------------------------------------------------------------------------------------
# fp16 / bf16
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [(n, (F16, BF16)[i % 2]) for i, n in enumerate(gc.HALF_SIZES)],
                         ids=["%d-%s" % (n, ("fp16", "bf16")[i % 2]) for i, n in enumerate(gc.HALF_SIZES)])
def test_half_native(n, dtype, guarded):
    t0 = time.time()
    cap = gc.codelet(n, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(nmaps * n * n * 2 + (64 << 20), "half %d" % n)
    bank = lc.make_bank(n, n, 900 + n, dtype)
    ref64, tol = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 41 * n, DEV)
    assert dpa.has_half_kernel(n, n)
    got = dpa.energy_nc(_gather(bd, idx, (1, nmaps, n, n)))
    twin = dpa.energy_nc(bd[None])[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, tol, what="half %d" % n, group=cap.maps_per_unit, units=cap.units)
    guarded.check("half %d" % n, 2)
    _report("half %d %s" % (n, dtype), nmaps, cap.units, cap.maps_per_unit, worst, tol, t0)


def test_half_staged_upcast(guarded):
    """72 x 72 fp16 takes the staged route: k_upcast_half's cus x 32 blocks of 256 threads loop over a chunk's elements."""
    t0 = time.time()
    n = 72
    units = gc.upcast_elems(_cus())
    nmaps = -(-gc.loop_count(units, 1) // (n * n)) + 1
    assert nmaps <= gc.half_stage_chunk_maps(n, n) and not dpa.has_half_kernel(n, n)  # one chunk, one upcast launch
    lo, hi = gc.iterations(nmaps * n * n, units, 1)
    assert (lo, hi) == (2, 3)
    bank = lc.make_bank(n, n, 972, F16)
    ref64, tol = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 43, DEV)
    x = _gather(bd, idx, (1, nmaps, n, n))
    got = dpa.energy_nc(x)
    twin = dpa.energy_nc(bd[None])[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, tol, what="half staged 72")
    assert torch.equal(got, dpa.energy_nc(x.float()))  # the fp32 kernels on the same values (test_half_gpu.py)
    guarded.check("half staged", 3)
    _report("half-staged 72 (elements)", nmaps * n * n, units, 1, worst, tol, t0)


# ----------------------------------------------------------------------------------------------------
# channels-last
# ----------------------------------------------------------------------------------------------------
def _nhwc_case(name, n, dtype, C, items_cap, per_item, guarded, ctot=None, cb=0):
    """N samples of C scored channels, ceil(C / per_item) = 2 items per sample (the second one ragged), the twin an nhwc
    call on the bank (one sample of 251 channels). ctot > C: a channel slice of a wider channels-last tensor, the other
    channels holding 3.0."""
    t0 = time.time()
    assert -(-C // per_item) == 2 and C % per_item != 0
    N = gc.loop_count(items_cap, 1, multiple_of=2) // 2
    nmaps, esize = N * C, torch.empty(0, dtype=dtype).element_size()
    ctot = ctot or C
    _need(N * (ctot + C) * n * n * esize + (64 << 20), name)
    bank = lc.make_bank(n, n, 1000 + n, dtype)
    ref64, tol = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 47 * n + C, DEV)
    mem = torch.full((N, n, n, ctot), 3.0, dtype=dtype, device=DEV)  # the NHWC memory image
    mem[..., cb:cb + C] = bd[idx].view(N, C, n, n).permute(0, 2, 3, 1)
    x = mem.permute(0, 3, 1, 2)
    assert ops.energy_route(x.shape, x.stride()) == ops.ROUTE_NHWC
    got = dpa.energy_nc(x, c_begin=cb, c_count=C)
    bx = bd.permute(1, 2, 0).contiguous().permute(2, 0, 1)[None]  # the bank as one channels-last sample
    assert ops.energy_route(bx.shape, bx.stride()) == ops.ROUTE_NHWC
    twin = dpa.energy_nc(bx)[0]
    worst = lc.check_scores(got.reshape(-1), idx, ref64, twin, tol, what=name, group=C)
    guarded.check(name, 2)
    _report(name + " (items)", 2 * N, items_cap, 1, worst, tol, t0)


@pytest.mark.parametrize("n,dtype", [(2, F32), (4, F16), (7, BF16), (8, F16)], ids=["2-fp32", "4-fp16", "7-bf16", "8-fp16"])
def test_nhwc_lane(n, dtype, guarded):
    # 67 channels: one full run of 64 and a run of 3 per sample - half the bytes of two full runs
    _nhwc_case("nhwc-lane %d %s" % (n, dtype), n, dtype, 67, gc.nhwc_lane_items(n, _cus()), 64, guarded)


@pytest.mark.parametrize("n,dtype", [(14, F32), (16, F16), (28, BF16), (32, F32)], ids=["14-fp32", "16-fp16", "28-bf16", "32-fp32"])
def test_nhwc_block(n, dtype, guarded):
    cb = gc.nhwc_block_cb(n)
    _nhwc_case("nhwc-block %d %s" % (n, dtype), n, dtype, cb + 5, gc.nhwc_block_items(n, _cus()), cb, guarded)


def test_nhwc_block_channel_slice(guarded):
    cb = gc.nhwc_block_cb(14)
    _nhwc_case("nhwc-block 14 slice fp16", 14, F16, cb + 5, gc.nhwc_block_items(14, _cus()), cb, guarded, ctot=cb + 8, cb=2)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_nhwc_strip(dtype, guarded):
    _nhwc_case("nhwc-strip 56 %s" % dtype, 56, dtype, 5, gc.nhwc_block_items(56, _cus()), 4, guarded)


# ----------------------------------------------------------------------------------------------------
# rect and rank
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,pitch", [(3, 5, 0), (17, 20, 0), (33, 34, 0), (14, 14, 16)],
                         ids=["3x5", "17x20", "33x34", "14x14-pitched"])
def test_rect(h, w, pitch, guarded):
    """One shape per template size class (max edge <= 16, <= 32, <= 64) and dense 14 x 14 maps with a row pitch of 16 (the
    pad columns hold 3.0)."""
    t0 = time.time()
    cap = gc.rect(h, w, _cus())
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    _need(2 * nmaps * h * max(w, pitch) * 4 + (64 << 20), "rect %dx%d" % (h, w))
    bank = lc.make_bank(h, w, 1100 + h)
    ref64, _ = _energy_refs(bank)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 53 * h + w, DEV)

    def view(maps):
        if not pitch:
            return maps[None]
        big = torch.full((1, maps.shape[0], h, pitch), 3.0, device=DEV)
        big[..., :w] = maps
        return big[..., :w]

    x = view(bd[idx])
    assert x.stride(2) == (pitch or w)
    got = dpa.energy_nc(x, algo=dpa.ALGO_RECT)
    twin = dpa.energy_nc(view(bd), algo=dpa.ALGO_RECT)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, RTOL, what="rect %dx%d" % (h, w), group=cap.maps_per_unit, units=cap.units)
    guarded.check("rect", 2)
    _report("rect %dx%d pitch=%d" % (h, w, pitch), nmaps, cap.units, cap.maps_per_unit, worst, RTOL, t0)


@pytest.mark.parametrize("h,w", [(4, 4), (8, 8), (33, 17)])
def test_rank(h, w, guarded):
    t0 = time.time()
    cap = gc.rank(h, w)
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    bank = lc.make_rank_bank(h, w, 1200 + h)
    want = ro.rank_nc(bank[None])[0]
    assert torch.equal(want, lc.known_ranks(h, w)) and not ro.undecidable(bank[None]).any()
    assert (want == 0).sum() == len(lc.ZERO_MAPS) and (want < min(h, w)).sum() > B // 4 and (want == min(h, w)).any()
    ref64 = want.double().to(DEV)
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 59 * h + w, DEV)
    got = dpa.rank_nc(_gather(bd, idx, (1, nmaps, h, w)))
    twin = dpa.rank_nc(bd[None])[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, 0.0, what="rank %dx%d" % (h, w), group=cap.maps_per_unit, units=cap.units)
    assert worst == 0.0  # exact integers
    guarded.check("rank", 2)
    _report("rank %dx%d" % (h, w), nmaps, cap.units, cap.maps_per_unit, worst, 0.0, t0)
