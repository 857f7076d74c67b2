"""dcts_dct2d_lowpass_f32 on the GPU against the float64 definition of tests/lowpass_oracle.py at 2e-6 of the batch's largest
|coefficient| (the bound tests/test_gpu_coeff_large.py holds dct2d to): both routes, the orientation of the corner, the bits that
must not depend on the call, drop_dc and the flat rule, the extent of what is written, the grid loop and far offsets.
tests/test_lowpass_probes_gpu.py holds the per-coefficient probes of the fused route at every codelet edge."""
import time

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import grid_capacity as gc
import loop_cases as lc
import lowpass_oracle as lo
from helpers import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = lo.SIG_TOL    # of max |coefficient| of the batch
BASIS_TOL = 5e-6    # a single basis function: one unit coefficient, everything else below this

CODELET_EDGES = lo.CODELET_EDGES  # every instantiation of k_lowpass_codelet: G = 32 ... 1, the special strides, idle lanes
FALLBACK = {  # name: (shape of the tensor the view is cut from, K)
    "13x17": ((2, 5, 13, 17), 8), "5x40": ((2, 5, 5, 40), 8), "33x33": ((1, 6, 33, 33), 8), "72x72": ((1, 5, 72, 72), 8),
    "pitched16": ((2, 5, 16, 20), 5),
    # non-square with an edge beyond 64, one of them beyond 256: the coefficients of the cosine-matrix kernel alone
    "100x72": ((2, 5, 100, 72), 8), "260x9": ((2, 5, 260, 9), 8),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, x, K, what, drop_dc=False, **sl):
    ref = lo.lowpass_f64(x, K, drop_dc=drop_dc, **sl)
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == ref.shape, (what, g.shape, ref.shape)
    assert np.isfinite(g).all(), what
    scale = lo.coefficient_scale(x)
    err = np.abs(g - ref).max() / scale
    print("LOWPASS %s K=%d worst |got - f64| / max |coeff| = %.3e (tol %.1e)" % (what, K, err, TOL))
    assert err <= TOL, (what, K, err)
    return g


def _fallback_view(name):
    shape, K = FALLBACK[name]
    x = synth(*shape, seed=900 + shape[2] * shape[3], dead=False)
    xd = x.to(DEV)
    if name == "pitched16":
        return x[..., :16], xd[..., :16], K
    return x, xd, K


# ----------------------------------------------------------------------------------------------------
# the fused route
# ----------------------------------------------------------------------------------------------------
def test_codelet_edge_list_is_the_librarys():
    assert [e for e in range(1, 65) if dpa.has_codelet(e, e)] == list(CODELET_EDGES) and len(CODELET_EDGES) == 22


@pytest.mark.parametrize("n", CODELET_EDGES)
def test_codelet_route_against_float64(n):
    G = 64 // n
    x = synth(1, 3 * G + 1, n, n, 500 + n, dead=True)  # the last group is ragged
    xd = x.to(DEV)
    assert dpa.has_codelet(n, n)
    sizes = lo.corner_sizes(n)
    # which store chain a K takes (the output of a call without out= is 16-byte aligned): where a wave holds several maps
    # both chains run, but at edge 2, where no K <= n is a multiple of 4
    vec = [K for K in sizes if G >= 2 and K % 4 == 0]
    scalar = [K for K in sizes if not (G >= 2 and K % 4 == 0)]
    assert scalar and (bool(vec) == (G >= 2 and n >= 4)), (n, G, vec, scalar)
    assert vec == [K for K in sizes if lo.on_vector_chain(n, K)]
    for K in sizes:
        got = dpa.lowpass_nc(xd, K)
        assert got.shape == (1, 3 * G + 1, K, K) and got.data_ptr() % 16 == 0
        _check(got, x, K, "codelet %d (G = %d, %s chain)" % (n, G, "16-byte" if K in vec else "scalar"))
    # K beyond the edge: the whole map, the same bits as K = n
    big = dpa.lowpass_nc(xd, n + 3)
    assert big.shape == (1, 3 * G + 1, n, n) and torch.equal(_bits(big), _bits(dpa.lowpass_nc(xd, n)))
    _check(big, x, n + 3, "codelet %d clamp" % n)


def test_codelet_channel_slice_of_a_sample_strided_view():
    big = synth(5, 11, 14, 14, 77, dead=True)
    view, vd = big[::2], big.to(DEV)[::2]
    assert not vd.is_contiguous() and vd.stride(0) == 2 * 11 * 196
    got = dpa.lowpass_nc(vd, 5, c_begin=3, c_count=7)
    _check(got, view, 5, "slice of a strided view", c_begin=3, c_count=7)
    assert torch.equal(_bits(got), _bits(dpa.lowpass_nc(vd.contiguous(), 5)[:, 3:10]))


@pytest.mark.parametrize("n", [7, 56])
def test_orientation_single_basis_function(n):
    """x = outer(C[1, :], C[3, :]) has one unit coefficient at [u, v] = [1, 3]; an output written as [v][u] has it at [3, 1]."""
    x = torch.from_numpy(lo.basis_map(n, 1, 3)[None, None].astype(np.float32)).to(DEV)
    for K in (4, 5, n):
        got = dpa.lowpass_nc(x, K).cpu().numpy()[0, 0]
        want = np.zeros((K, K))
        want[1, 3] = 1.0
        assert np.abs(got - want).max() <= BASIS_TOL, (n, K, got[1, 3], got[3, 1])
    for K in (1, 2, 3):
        assert np.abs(dpa.lowpass_nc(x, K).cpu().numpy()).max() <= BASIS_TOL, (n, K)


@pytest.mark.parametrize("n", [7, 14, 56, 64])
def test_codelet_against_dct2d(n):
    x = synth(2, 9, n, n, 640 + n, dead=True)
    xd = x.to(DEV)
    got = dpa.lowpass_nc(xd, 5)
    full = dpa.dct2d(xd)[..., :5, :5]
    scale = lo.coefficient_scale(x)
    err = float((got - full).abs().max()) / scale
    print("LOWPASS codelet %d vs dct2d: bit-identical=%s worst diff / max |coeff| = %.3e" % (n, torch.equal(_bits(got), _bits(full)), err))
    assert err <= TOL, (n, err)
    _check(got, x, 5, "codelet %d (the dct2d case)" % n)


# ----------------------------------------------------------------------------------------------------
# the fallback
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_fallback_is_the_corner_of_dct2d_bit_for_bit(name):
    x, xd, K = _fallback_view(name)
    H, W = x.shape[2:]
    got = dpa.lowpass_nc(xd, K)
    assert got.shape == (x.shape[0], x.shape[1], min(K, H), min(K, W)) and got.is_contiguous()
    _check(got, x, K, "fallback " + name)
    full = dpa.dct2d(xd)
    assert torch.equal(_bits(got), _bits(full[..., :min(K, H), :min(K, W)])), name
    sl = dpa.lowpass_nc(xd, K, c_begin=1, c_count=3)
    assert torch.equal(_bits(sl), _bits(got[:, 1:4])), name


# ----------------------------------------------------------------------------------------------------
# a map's signature depends on that map alone
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,K", [(14, 14, 5), (13, 17, 8)])
@pytest.mark.parametrize("drop_dc", [False, True])
def test_signature_does_not_depend_on_the_call(h, w, K, drop_dc):
    bank = synth(1, 11, h, w, 31 * h + w, dead=True)[0]
    bank[4] = 2.5  # a flat map among them
    bd = bank.to(DEV)
    alone = dpa.lowpass_nc(bd[None], K, drop_dc=drop_dc)[0]
    idx = torch.randint(11, (3 * 37,), generator=torch.Generator().manual_seed(5)).to(DEV)
    x = bd[idx].view(3, 37, h, w)
    got = dpa.lowpass_nc(x, K, drop_dc=drop_dc)
    assert torch.equal(_bits(got.view(3 * 37, *alone.shape[1:])), _bits(alone[idx]))
    part = dpa.lowpass_nc(x[1:], K, c_begin=5, c_count=30, drop_dc=drop_dc)
    assert torch.equal(_bits(part), _bits(got[1:, 5:35]))
    one = dpa.lowpass_nc(x[2:3, 36:37], K, drop_dc=drop_dc)
    assert torch.equal(_bits(one[0, 0]), _bits(got[2, 36]))


# ----------------------------------------------------------------------------------------------------
# drop_dc and the flat rule
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(56, 8), (72, 8), (14, 14), (13, 5)])
def test_drop_dc(n, K):
    w = 17 if n == 13 else n
    x = synth(2, 8, n, w, 70 + n, dead=False)
    x[:, 1] = 3.7                      # a conv that died onto a positive bias
    x[:, 2] = 0.0
    x[:, 3] = -1.25
    x[:, 4] = 3.7
    x[:, 4, n - 1, w - 2] = 3.7000003  # constant except for one element: not flat
    x[0, 5] = 3.7
    x[0, 5, 0, 0] = 0.0                # the first element is the odd one
    xd = x.to(DEV)
    plain, drop = dpa.lowpass_nc(xd, K), dpa.lowpass_nc(xd, K, drop_dc=True)
    _check(drop, x, K, "drop_dc %dx%d" % (n, w), drop_dc=True)
    assert lo.flat_maps(x).tolist() == [[False, True, True, True, False, False, False, False]] * 2
    pb, db = _bits(plain).cpu(), _bits(drop).cpu()
    for c in (1, 2, 3):
        assert (db[:, c] == 0).all(), c        # all +0.0, sign bit included
    live = [0, 4, 5, 6, 7]
    assert (db[:, live, 0, 0] == 0).all()      # [0, 0] is +0.0
    rest = torch.ones(db.shape[2:], dtype=torch.bool)
    rest[0, 0] = False
    assert torch.equal(db[:, live][:, :, rest], pb[:, live][:, :, rest])  # every other element: the bits of the plain call
    if K > 1:
        assert float(drop[:, 4].abs().max()) > 0 and float(drop[0, 5].abs().max()) > 0
    if n in (56, 14):  # an odd-base edge: the plain call shows the round-off the rule is there for
        print("LOWPASS flat %d: largest AC coefficient of the constant map without the rule = %.3e"
              % (n, float(plain[:, 1].reshape(2, -1)[:, 1:].abs().max())))


# ----------------------------------------------------------------------------------------------------
# what is written
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K", [((2, 7, 14, 14), 5), ((1, 13, 4, 4), 3), ((2, 5, 13, 17), 8), ((1, 3, 72, 72), 8)])
@pytest.mark.parametrize("drop_dc", [False, True])
def test_guard_words_and_full_overwrite(shape, K, drop_dc):
    x = synth(*shape, seed=11, dead=True).to(DEV)
    oshape = (shape[0], shape[1], min(K, shape[2]), min(K, shape[3]))
    n = int(np.prod(oshape))
    guard = 64
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:guard] = 1234.5
    buf[guard + n:] = -4321.5
    out = buf[guard:guard + n].view(oshape)
    ret = dpa.lowpass_nc(x, K, drop_dc=drop_dc, out=out)
    assert ret.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 1234.5).all()) and bool((buf[guard + n:] == -4321.5).all())
    assert bool(torch.isfinite(out).all())
    assert torch.equal(_bits(out), _bits(dpa.lowpass_nc(x, K, drop_dc=drop_dc)))


# ----------------------------------------------------------------------------------------------------
# more maps than one grid holds
# ----------------------------------------------------------------------------------------------------
def test_grid_loop_edge_4():
    t0 = time.time()
    n, K = 4, 2
    cap = gc.codelet(n, torch.cuda.get_device_properties(0).multi_processor_count)
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    assert gc.iterations(nmaps, cap.units, cap.maps_per_unit) == (2, 3)
    bank = lc.make_bank(n, n, 104)
    coeff = lo.coefficients_f64(bank[None])[0]
    ref64 = torch.from_numpy(np.ascontiguousarray(coeff[:, :K, :K])).to(DEV)
    denom = torch.from_numpy(np.abs(coeff).reshape(lc.B, -1).max(axis=1)).to(DEV)  # per map: never wider than the batch's
    bd = bank.to(DEV)
    idx = lc.random_index(nmaps, 29, DEV)
    x = bd[idx].view(1, nmaps, n, n)
    buf, view = lc.guarded(nmaps, K * K, DEV)
    got = dpa.lowpass_nc(x, K, out=view.view(1, nmaps, K, K))
    twin = dpa.lowpass_nc(bd[None], K)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, TOL, denom64=denom, guard=buf[nmaps * K * K:], what="lowpass 4",
                            group=cap.maps_per_unit, units=cap.units, signed_zero=True)
    torch.cuda.synchronize()
    print("GRIDLOOP lowpass-codelet 4 maps=%d grid=%d x %d worst=%.3g tol=%.3g secs=%.2f"
          % (nmaps, cap.units, cap.maps_per_unit, worst, TOL, time.time() - t0))


# ----------------------------------------------------------------------------------------------------
# far offsets
# ----------------------------------------------------------------------------------------------------
def test_second_sample_beyond_four_gib():
    n, C, K = 14, 6, 5
    stride_n = (1 << 30) + 64  # elements: sample 1 starts 4 GiB + 256 bytes behind sample 0
    need = (stride_n + C * n * n) * 4
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    assert free >= need + (256 << 20), "the far-offset case needs %.2f GiB of device memory, %.2f GiB are free" % (need / 2 ** 30, free / 2 ** 30)
    arena = torch.empty(stride_n + C * n * n, dtype=torch.float32, device=DEV)  # untouched between the two samples
    x = torch.as_strided(arena, (2, C, n, n), (stride_n, n * n, n, 1))
    assert (x[1].data_ptr() - x[0].data_ptr()) > 1 << 32
    maps = synth(2, C, n, n, 4242, dead=True)
    maps[1, 2] = 1.5
    x.copy_(maps.to(DEV))
    twin = maps.to(DEV)
    for drop_dc in (False, True):
        got = dpa.lowpass_nc(x, K, c_begin=1, c_count=4, drop_dc=drop_dc)
        small = dpa.lowpass_nc(twin, K, c_begin=1, c_count=4, drop_dc=drop_dc)
        assert torch.equal(_bits(got), _bits(small)), drop_dc
    _check(dpa.lowpass_nc(x, K), maps, K, "far sample")
    del x, arena
    torch.cuda.empty_cache()
