"""dcts_spectral_entropy_f32 on the GPU against the float64 definition of tests/entropy_oracle.py, at the absolute tolerance
derived there (TOL = 8 R, R the fp32 restatement's own error on these inputs): the fused kernel on every codelet edge and,
with the odd pad, on every odd edge below one (each an instantiation of its own), known answers and the unequal pairs that
see the weight of every single coefficient, dead and poisoned maps, the fallback with its chunking, both grid-stride loops with
more maps than a grid holds, and the harness modes."""
import math
import time

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import entropy_oracle as eo
import grid_capacity as gc
import loop_cases as lc
from dct_pruning_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = eo.TOL
LN2 = math.log(2.0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, x, pad=False, c_begin=0, c_count=None, what=""):
    """got [N, c] float32 on the device against the definition: within TOL, inside [0, ln(H'W')], +0.0 for zero maps."""
    ref = eo.entropy_nc_f64(x, c_begin, c_count, pad)
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == ref.shape, (what, g.shape, ref.shape)
    err = np.abs(g.astype(np.float64) - ref)
    print("ENTROPY %s worst |got - f64| = %.3e (tol %.3e)" % (what, err.max(), TOL))
    assert np.isfinite(g).all(), what
    assert err.max() <= TOL, (what, float(err.max()), int(err.argmax()))
    p = 1 if (pad and x.shape[2] % 2) else 0
    top = np.float32(math.log((x.shape[2] + p) * (x.shape[3] + p)))
    assert (g >= 0).all() and (g <= top).all(), what
    return ref


# ----------------------------------------------------------------------------------------------------
# fused route
# ----------------------------------------------------------------------------------------------------
def test_edge_lists_are_the_librarys():
    """Every codelet edge is an instantiation k_entropy_codelet<N, 0>, every odd edge below one a k_entropy_codelet<N, 1>."""
    edges = [e for e in range(1, 65) if dpa.has_codelet(e, e)]
    assert edges == list(eo.FUSED_EDGES) and len(edges) == 22 and all(dpa.has_entropy_kernel(e, e) for e in edges)
    odd = [h for h in range(1, 64, 2) if dpa.has_codelet(h + 1, h + 1)]
    assert odd == list(eo.PAD_EDGES) and len(odd) == 20
    assert set(eo.BASIS_EDGES) <= set(eo.FUSED_EDGES)


@pytest.mark.parametrize("edge", eo.FUSED_EDGES)
def test_fused_kernel(edge):
    x = eo.fused_case(edge)
    xd = x.to(DEV)
    assert dpa.has_entropy_kernel(edge, edge) and _lib.load().dcts_entropy_workspace_bytes(*x.shape[:2], edge, edge) == 0
    got = dpa.spectral_entropy_nc(xd, algo=dpa.ALGO_CODELET)
    _check(got, x, what="fused %d" % edge)
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(xd, algo=dpa.ALGO_CODELET)))  # repeated call
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(xd)))                          # AUTO is this kernel
    out = torch.full_like(got, float("nan"))
    assert dpa.spectral_entropy_nc(xd, out=out) is out and torch.equal(_bits(out), _bits(got))


@pytest.mark.parametrize("edge", eo.FUSED_EDGES)
def test_fused_kernel_on_a_channel_slice_of_a_sample_strided_view(edge):
    """The densenet-style call: the last 12 channels of a wider tensor that is itself a view with a gap between samples.
    Bitwise what a call on the dense bank of those maps gives: a map's value depends on that map alone."""
    n = 2 if edge >= 56 else 3
    bank = eo.mixed_maps(n, 12, edge, edge, 6000 + edge).to(DEV)
    ctot = 17
    big = torch.full((n, ctot + 2, edge, edge), 3.0, device=DEV)
    big[:, ctot - 12:ctot] = bank
    view = big[:, :ctot]
    assert view.stride(0) != ctot * view.stride(1)
    got = dpa.spectral_entropy_nc(view, c_begin=ctot - 12, c_count=12)
    twin = dpa.spectral_entropy_nc(bank)
    assert torch.equal(_bits(got), _bits(twin))
    # and the maps one by one, each at the head of a wave of its own
    flat = bank.reshape(1, n * 12, edge, edge)
    for m in (0, 5, n * 12 - 1):
        one = dpa.spectral_entropy_nc(flat[:, m:m + 1].contiguous())
        assert torch.equal(_bits(one.reshape(-1)), _bits(twin.reshape(-1)[m:m + 1])), (edge, m)


@pytest.mark.parametrize("edge", eo.PAD_EDGES)
def test_odd_pad(edge):
    x = eo.pad_case(edge)
    assert dpa.has_entropy_kernel(edge + 1, edge + 1)
    got = dpa.spectral_entropy_nc(x.to(DEV), pad_front_if_odd=True)
    _check(got, x, pad=True, what="pad %d -> %d" % (edge, edge + 1))
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(x.to(DEV), pad_front_if_odd=True, algo=dpa.ALGO_CODELET)))
    padded = torch.nn.functional.pad(x, (1, 0, 1, 0)).to(DEV)
    np.testing.assert_allclose(dpa.spectral_entropy_nc(padded).cpu().numpy(), got.cpu().numpy(), rtol=0, atol=TOL)
    sl = dpa.spectral_entropy_nc(x.to(DEV), c_begin=2, c_count=3, pad_front_if_odd=True)
    assert torch.equal(_bits(sl), _bits(got[:, 2:5]))


# ----------------------------------------------------------------------------------------------------
# known answers
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", eo.BASIS_EDGES)
def test_basis_functions_and_pairs(n):
    got = dpa.spectral_entropy_nc(eo.basis_maps(n).to(DEV)).cpu().numpy()
    print("ENTROPY basis %d worst |H| = %.3e" % (n, np.abs(got).max()))
    assert got.shape == (1, n * n) and (np.abs(got) <= TOL).all() and (got >= 0).all()
    pairs = dpa.spectral_entropy_nc(eo.pair_maps(n).to(DEV)).cpu().numpy().astype(np.float64)
    print("ENTROPY pairs %d worst |H - ln 2| = %.3e" % (n, np.abs(pairs - LN2).max()))
    assert (np.abs(pairs - LN2) <= TOL).all()


def _report_unequal(what, got, ref):
    dev = np.abs(got.cpu().numpy().astype(np.float64) - eo.H_UNEQUAL)
    print("ENTROPY %s maps=%d H_f64 in [%.6f, %.6f], worst |got - %.4f| = %.3e"
          % (what, ref.size, ref.min(), ref.max(), eo.H_UNEQUAL, dev.max()))


@pytest.mark.parametrize("n", eo.FUSED_EDGES)
def test_unequal_pairs(n):
    """basis(p) + 0.5 * basis(u, v) for every (u, v) of the tile: p = (0.8, 0.2), where a relative error eps in the weight of
    one coefficient moves H by 0.44 eps (the equal pairs sit at the maximum of H and move by eps^2 / 2:
    tests/test_entropy_cpu.py holds the mutant that passes them and fails here)."""
    x = eo.unequal_pair_maps(n)
    assert tuple(x.shape) == (1, n * n, n, n)
    got = dpa.spectral_entropy_nc(x.to(DEV), algo=dpa.ALGO_CODELET)
    ref = _check(got, x, what="unequal pairs %d" % n)
    assert np.abs(ref - eo.H_UNEQUAL).max() <= 1e-6  # the construction: rounding the maps to fp32 moves H by 2e-8
    _report_unequal("unequal pairs %d" % n, got, ref)


@pytest.mark.parametrize("edge", eo.PAD_EDGES)
def test_unequal_pairs_under_the_odd_pad(edge):
    """The unequal pairs of the padded tile without their first row and column, which the pad fills with zeros: no map is a
    pair any more, so every value is compared with the float64 definition, which pads the same way."""
    x = eo.padded_unequal_pair_maps(edge)
    assert tuple(x.shape) == (1, (edge + 1) ** 2, edge, edge) and dpa.has_entropy_kernel(edge + 1, edge + 1)
    got = dpa.spectral_entropy_nc(x.to(DEV), pad_front_if_odd=True, algo=dpa.ALGO_CODELET)
    ref = _check(got, x, pad=True, what="unequal pairs, pad %d -> %d" % (edge, edge + 1))
    _report_unequal("unequal pairs, pad %d -> %d" % (edge, edge + 1), got, ref)


def test_scale_invariance():
    x, big, small = eo.scale_case()
    ref = _check(dpa.spectral_entropy_nc(x.to(DEV)), x, what="scale 1")
    for name, y in (("2^20", big), ("2^-20", small)):
        got = dpa.spectral_entropy_nc(y.to(DEV))
        _check(got, y, what="scale " + name)
        assert np.abs(got.cpu().numpy().astype(np.float64) - ref).max() <= TOL  # the unscaled value


# ----------------------------------------------------------------------------------------------------
# dead and poisoned maps
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,algo,pad", [(8, dpa.ALGO_AUTO, False), (14, dpa.ALGO_AUTO, False), (56, dpa.ALGO_AUTO, False),
                                           (13, dpa.ALGO_AUTO, False), (16, dpa.ALGO_DIRECT, False),
                                           (10, dpa.ALGO_AUTO, False), (20, dpa.ALGO_AUTO, False),  # special strides, G = 6 and 3
                                           (9, dpa.ALGO_AUTO, True)],                               # runs <10, 1>
                         ids=["8", "14", "56", "13-fallback", "16-direct", "10", "20", "9-pad"])
def test_zero_maps_give_plus_zero_and_a_nan_map_stays_alone(edge, algo, pad):
    x = eo.fused_case(edge if edge != 13 else 14)[..., :edge, :edge].contiguous()
    x[:, 2] = 0
    x[0, 4] = 0
    xd = x.to(DEV)
    if pad:
        assert dpa.has_entropy_kernel(edge + 1, edge + 1)
        run = lambda t, algo: dpa.spectral_entropy_nc(t, pad_front_if_odd=True, algo=algo)
    else:
        run = lambda t, algo: dpa.spectral_entropy_nc(t, algo=algo)
    clean = run(xd, algo)
    assert (_bits(clean[:, 2]) == 0).all() and int(_bits(clean[0, 4])) == 0  # +0.0: the sign bit too
    assert (clean[:, 0] > 0).all()
    for poison in (float("nan"), float("inf")):
        y = xd.clone()
        y[1, 3, edge // 2, 1] = poison
        got = run(y, algo)
        assert bool(torch.isnan(got[1, 3])), poison
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[1, 3] = False
        assert torch.equal(_bits(got)[keep], _bits(clean)[keep]), poison


# ----------------------------------------------------------------------------------------------------
# fallback route
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", eo.FALLBACK_SHAPES, ids=["%dx%d" % s for s in eo.FALLBACK_SHAPES])
def test_fallback_shapes(h, w):
    x = eo.fallback_case(h, w)
    xd = x.to(DEV)
    lib = _lib.load()
    assert not (h == w and dpa.has_entropy_kernel(h, w)) and lib.dcts_entropy_workspace_bytes(1, 3, h, w) > 0
    got = dpa.spectral_entropy_nc(xd)
    _check(got, x, what="fallback %dx%d" % (h, w))
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(xd)))
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(xd, algo=dpa.ALGO_DIRECT)))
    with pytest.raises(_lib.DctScoreError) as e:
        dpa.spectral_entropy_nc(xd, algo=dpa.ALGO_CODELET)
    assert e.value.code == -6
    # a map of its own and a channel slice: the same bits
    assert torch.equal(_bits(dpa.spectral_entropy_nc(xd, c_begin=1, c_count=2)), _bits(got[:, 1:3]))


@pytest.mark.parametrize("h,w", eo.DIRECT_SHAPES, ids=["%dx%d" % s for s in eo.DIRECT_SHAPES])
def test_fallback_on_the_cosine_matrix_kernels_own_shapes(h, w):
    """A non-square map with an edge beyond 64 (one of them beyond 256): every coefficient the reduction reads is a dot
    product of the cosine-matrix kernel. Channels 1 ... 3 of 5 in two samples: the slice is not contiguous."""
    x = eo.direct_case(h, w)
    xd = x.to(DEV)
    got = dpa.spectral_entropy_nc(xd, c_begin=1, c_count=3)
    _check(got, x, c_begin=1, c_count=3, what="direct %dx%d, channels 1..3 of 5" % (h, w))
    full = dpa.spectral_entropy_nc(xd)
    _check(full, x, what="direct %dx%d" % (h, w))
    assert torch.equal(_bits(got), _bits(full[:, 1:4]))
    assert torch.equal(_bits(full), _bits(dpa.spectral_entropy_nc(xd, algo=dpa.ALGO_DIRECT)))


def test_fallback_pitched_rows_and_direct_against_codelet():
    view = eo.pitch_case(DEV)
    assert view.stride(2) == eo.PITCH and view.stride(3) == 1
    got = dpa.spectral_entropy_nc(view)  # AUTO: rows are not dense, so the fallback reads the view where it lies
    _check(got, view.cpu().contiguous(), what="pitched 16")
    with pytest.raises(_lib.DctScoreError) as e:
        dpa.spectral_entropy_nc(view, algo=dpa.ALGO_CODELET)
    assert e.value.code == -6
    assert torch.equal(_bits(got), _bits(dpa.spectral_entropy_nc(view)))
    # the dense copy through the fallback: its coefficients may come from another kernel, so the definition is the yardstick
    _check(dpa.spectral_entropy_nc(view.contiguous(), algo=dpa.ALGO_DIRECT), view.cpu().contiguous(), what="pitched 16, dense copy")
    x = eo.fused_case(16)
    direct = dpa.spectral_entropy_nc(x.to(DEV), algo=dpa.ALGO_DIRECT)
    _check(direct, x, what="direct 16")
    fused = dpa.spectral_entropy_nc(x.to(DEV), algo=dpa.ALGO_CODELET)
    assert (direct - fused).abs().max().item() <= TOL


@pytest.mark.parametrize("h,w,n,c", [(13, 13, 2, 5), (72, 72, 1, 3), (56, 28, 2, 3)], ids=["13x13", "72x72", "56x28"])
def test_fallback_chunking_does_not_change_a_bit(h, w, n, c):
    """A workspace of the coefficient path's own need, one map's two tiles and one byte: one map per chunk, as many
    launches as maps. Bitwise the result with the full workspace."""
    lib = _lib.load()
    x = eo.mixed_maps(n, c, h, w, 7000 + h).to(DEV)
    full = dpa.spectral_entropy_nc(x)
    need = lib.dcts_entropy_workspace_bytes(n, c, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(nbytes, out):
        lib.dcts_workspace_invalidate_range(ws.data_ptr(), ws.numel())
        return lib.dcts_spectral_entropy_f32(x.data_ptr(), n, c, h, w, x.stride(0), x.stride(1), x.stride(2), 1, 0, c, 0,
                                             out.data_ptr(), ws.data_ptr(), nbytes, stream, 0)

    # the smallest workspace the call takes holds one map per chunk: found by the call's own answer (-5 below it)
    tile = h * w * 4
    lo = next(b for b in range(2 * tile, need + 1, 256) if call(b, torch.empty(n, c, device=DEV)) == 0)
    assert call(lo - 256, torch.empty(n, c, device=DEV)) == -5
    small = lo + 1  # one map's coefficients and scratch, plus one: still one map per chunk (two need another 2 tiles)
    assert 2 * tile > 257 and small < need and n * c >= 3
    out = torch.full((n, c), float("nan"), device=DEV)
    assert call(small, out) == 0
    assert torch.equal(_bits(out), _bits(full))
    out2 = torch.full((n, c), float("nan"), device=DEV)
    assert call(need, out2) == 0 and torch.equal(_bits(out2), _bits(full))


# ----------------------------------------------------------------------------------------------------
# grid-stride loops (tests/test_grid_loops_gpu.py's method)
# ----------------------------------------------------------------------------------------------------
def _loop_refs(bank):
    ref = eo.entropy_nc_f64(bank)[0]
    live = (bank[0].double() ** 2).sum(dim=(-2, -1)) > 0
    return torch.from_numpy(ref).to(DEV), live.double().to(DEV)  # denom 1 for live maps: TOL is absolute; 0 -> exactly +0.0


def _loop_report(name, nmaps, units, per, worst, t0):
    torch.cuda.synchronize()
    lo, hi = gc.iterations(nmaps, units, per)
    print("GRIDLOOP %s maps=%d grid=%d x %d iterations=%d..%d worst=%.3g tol=%.3g secs=%.2f"
          % (name, nmaps, units, per, lo, hi, worst, TOL, time.time() - t0))
    assert (lo, hi) == (2, 3), (name, lo, hi)


def test_grid_loop_fused_kernel_edge_4():
    t0 = time.time()
    n = 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = gc.codelet(n, cus)  # k_entropy_codelet<4> launches by codelet_grid<4>, as the kernels gc.codelet names
    nmaps = gc.loop_count(cap.units, cap.maps_per_unit)
    bank = eo.loop_banks()[0]
    ref64, denom = _loop_refs(bank)
    bd = bank[0].to(DEV)
    idx = lc.random_index(nmaps, 61 * n, DEV)
    buf, out = lc.guarded(nmaps, 1, DEV)
    got = dpa.spectral_entropy_nc(bd[idx].view(1, nmaps, n, n), algo=dpa.ALGO_CODELET, out=out.view(1, nmaps))
    twin = dpa.spectral_entropy_nc(bd[None], algo=dpa.ALGO_CODELET)[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, TOL, denom64=denom, guard=buf[nmaps:], what="entropy codelet 4",
                            group=cap.maps_per_unit, units=cap.units)
    _loop_report("entropy-codelet 4", nmaps, cap.units, cap.maps_per_unit, worst, t0)


def test_grid_loop_reduce_kernel_5x5():
    """5 x 5 has no codelet: coefficients of ONE chunk, then one k_entropy_reduce launch whose 4096 x 4 waves loop."""
    t0 = time.time()
    n = 5
    cap = gc.reduce()  # k_entropy_reduce launches by kReduceWaves / kReduceMaxBlocks, as k_band_reduce
    nmaps = gc.loop_count(cap.units, 1)
    assert not dpa.has_entropy_kernel(n, n) and nmaps <= gc.band_fallback_chunk_maps(n, n)  # the band fallback's chunk rule
    bank = eo.loop_banks()[1]
    ref64, denom = _loop_refs(bank)
    bd = bank[0].to(DEV)
    idx = lc.random_index(nmaps, 67, DEV)
    buf, out = lc.guarded(nmaps, 1, DEV)
    got = dpa.spectral_entropy_nc(bd[idx].view(1, nmaps, n, n), out=out.view(1, nmaps))
    twin = dpa.spectral_entropy_nc(bd[None])[0]
    worst = lc.check_scores(got[0], idx, ref64, twin, TOL, denom64=denom, guard=buf[nmaps:], what="entropy reduce 5x5")
    _loop_report("entropy-reduce 5x5", nmaps, cap.units, 1, worst, t0)


# ----------------------------------------------------------------------------------------------------
# harness
# ----------------------------------------------------------------------------------------------------
def _run(name, root, **kw):
    import contextlib
    import io
    import os
    import types
    from dct_pruning_amd import harness, nets
    from dct_pruning_amd.data import SyntheticLoader
    from helpers import HARNESS_CASES, deterministic_init
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).to(DEV)
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.makedirs(str(root), exist_ok=True)
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(net, args, train_loader=loader, criterion="entropy", **kw)
    finally:
        os.chdir(cwd)
    d = os.path.join(str(root), "entropy_score", "%s_limit%d" % (name, limit))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_harness_modes_agree_on_resnet_56(tmp_path):
    base = _run("resnet_56", tmp_path / "host")
    assert len(base) == 55 and all(k.startswith("ent_") for k in base)
    for mode, kw in (("device", {"accumulate": "device"}), ("single", {"single_sweep": True}),
                     ("single-device", {"single_sweep": True, "accumulate": "device"})):
        out = _run("resnet_56", tmp_path / mode, **kw)
        assert sorted(out) == sorted(base), mode
        for k in base:
            assert out[k].dtype == np.float32 and out[k].shape == base[k].shape
            np.testing.assert_allclose(out[k], base[k], rtol=1e-4, atol=1e-6 * float(base[k].max()), err_msg="%s %s" % (mode, k))
    for k, v in base.items():
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= math.log(32 * 32)).all(), k


def test_harness_u2netp_every_hook_point_writes_a_bounded_file(tmp_path, monkeypatch):
    """U2-Net-p at the harness tests' input (72 x 72: maps of 72, 36, 18, 9, 5 and 3, the input hooks with the odd pad).
    Batch 1, limit 1: a file holds the values of one call, so each call's bound is its file's."""
    from dct_pruning_amd import harness, schedules
    calls = []

    def scorer(x, c_begin=0, c_count=None, pad_front_if_odd=False):
        out = ops.spectral_entropy_nc(x, c_begin, c_count, pad_front_if_odd)
        p = 1 if (pad_front_if_odd and x.shape[2] % 2) else 0
        top = np.float32(math.log((x.shape[2] + p) * (x.shape[3] + p)))
        assert bool(torch.isfinite(out).all()) and bool((out >= 0).all()) and bool((out <= float(top)).all()), tuple(x.shape)
        calls.append((x.shape[2] + p, x.shape[3] + p))
        return out

    monkeypatch.setattr(harness, "_entropy_nc", scorer)
    out = _run("u2netp", tmp_path / "u2", single_sweep=True)
    pts = schedules.SCHEDULES["u2netp"]()
    stems = [stem for p in pts for stem, _, _ in p.files]
    assert sorted(out) == sorted("ent_" + s for s in stems) and len(out) == 118 and len(calls) >= len(pts)
    assert {72, 36, 18} <= {h for h, _ in calls}  # the large-tile fallback and the codelets
    for k, v in out.items():
        assert v.dtype == np.float32 and v.ndim == 1 and v.size > 0 and np.isfinite(v).all() and (v >= 0).all(), k
        assert (v <= math.log(73 * 73)).all(), k
