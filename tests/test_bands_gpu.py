"""The band energies on the GPU (dcts_band_energy_f32 / ops.band_energy_nc / imp_score(criterion="bands") / the CLI)
against the float64 definition of tests/band_oracle.py.

Error measure everywhere: |got[b] - f64[b]| / E_map with E_map the map's float64 total energy (a coefficient's fp32 error
scales with the map's norm, so a near-empty band has no relative accuracy of its own to offer). Bound: dct_probes' rule,
tol = 8 * max(E_ref, 2^-22), E_ref the same measure for the fp32 restatement of the reference (band_oracle.band_energy_nc_f32)
on a subsample of the test's own inputs, computed here on the CPU. Every figure is printed before it is asserted
(`pytest -s` shows them): lines starting with BANDS_."""
import os

import numpy as np
import pytest
import torch

import band_oracle as bo
import dct_pruning_amd as dpa
import dct_probes as dp
from dct_pruning_amd import _lib, bands, harness, masks, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import deterministic_init

pytestmark = pytest.mark.gpu

CODELET_EDGES = [2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 48, 56, 60, 64]
SUB = 64  # maps of a case that E_ref is measured on


def _tol(x, w, **kw):
    """(tol, E_ref) by the rule of the module docstring on (a subsample of) the maps x [N, C, H, W]."""
    n, c = x.shape[:2]
    flat = x.reshape(1, n * c, x.shape[2], x.shape[3]) if not kw else x
    if not kw and n * c > SUB:
        g = torch.Generator().manual_seed(77)
        flat = flat[:, torch.randperm(n * c, generator=g)[:SUB].sort().values]
    flat = flat.cpu()
    e_ref = bo.band_error(bo.band_energy_nc_f32(flat, w, **kw), flat, w, **kw)
    return dp.tolerance(e_ref), e_ref


def _pairs(n_h, n_w):
    """all u x all v up to edge 32, the probe file's index set V per axis above that."""
    if max(n_h, n_w) <= 32:
        return dp.cover(n_h, n_w, exhaustive=True)
    return torch.tensor([(u, v) for u in dp.axis_picks(n_h, dp.FIXED_RANDOM_K) for v in dp.axis_picks(n_w, dp.FIXED_RANDOM_K, 1)])


def _placement(n_h, n_w, kind, K, algo, what):
    """Basis map (u, v): band b(u, v) receives 1 and every other band 0."""
    pairs = _pairs(n_h, n_w)
    x = dp.basis_maps(n_h, n_w, pairs)[None]  # [1, P, H, W]
    w = torch.from_numpy(bands.partition(n_h, n_w, K, kind))
    tol, e_ref = _tol(x, w)
    got = dpa.band_energy_nc(x.cuda(), w.cuda(), algo=algo)[0].cpu().double()  # [P, K]
    idx = torch.from_numpy(bands.band_index(n_h, n_w, K, kind))[pairs[:, 0], pairs[:, 1]]
    want = torch.zeros_like(got)
    want[torch.arange(len(pairs)), idx] = 1.0
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    worst, i = err.reshape(-1).max(dim=0)
    p = int(i) // K
    print("BANDS_PLACE %s %dx%d %s K=%d maps=%d worst=%.3g E_ref=%.3g tol=%.3g" % (what, n_h, n_w, kind, K, len(pairs), worst.item(), e_ref, tol))
    assert worst.item() <= tol, "basis (%d, %d): bands %s, expected band %d" % (int(pairs[p][0]), int(pairs[p][1]), got[p].tolist(), int(idx[p]))
    return worst.item()


# ---------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------
def test_codelet_edge_list_is_the_librarys():
    lib = _lib.load()
    assert [e for e in range(1, 65) if lib.dcts_has_band_kernel(e, e)] == CODELET_EDGES


@pytest.mark.parametrize("edge", CODELET_EDGES)
def test_placement_fused(edge):
    for kind in ("square", "diag"):
        for K in (2, 4, 8):
            _placement(edge, edge, kind, K, dpa.ALGO_CODELET, "fused")


@pytest.mark.parametrize("n_h,n_w", [(72, 72), (224, 224), (288, 288), (56, 28)])
def test_placement_fallback(n_h, n_w):
    assert not dpa.has_band_kernel(n_h, n_w)
    for kind in ("square", "diag"):
        for K in (2, 4, 8):
            _placement(n_h, n_w, kind, K, dpa.ALGO_AUTO, "fallback")


@pytest.mark.parametrize("edge", [8, 56])
def test_placement_fallback_on_a_codelet_shape(edge):
    _placement(edge, edge, "square", 4, dpa.ALGO_DIRECT, "fallback")


PAD_EDGES = [h for h in range(1, 64, 2) if h + 1 in CODELET_EDGES]  # the odd edges the front pad takes to a codelet
PAD_CASES = [(dpa.ALGO_CODELET, h) for h in PAD_EDGES] + [(dpa.ALGO_DIRECT, 7), (dpa.ALGO_DIRECT, 9)]


def test_padded_edge_list_is_the_librarys():
    assert PAD_EDGES == [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 23, 27, 29, 31, 35, 39, 47, 55, 59, 63]
    assert PAD_EDGES == [h for h in range(1, 64, 2) if dpa.has_codelet(h + 1, h + 1)]


@pytest.mark.parametrize("algo,edge", PAD_CASES, ids=["%d-%d" % c for c in PAD_CASES])
def test_placement_with_the_odd_pad(edge, algo):
    """A basis function of the padded (edge + 1)^2 tile is not zero in its first row and column, so a padded map cannot
    be a single basis function: the maps are the basis functions of the padded tile with that row and column cut off,
    and every band is compared with the float64 definition (which pads the same way) instead of with 0 / 1. Every padded
    edge is a kernel of its own (the load with its zero fill, the group size and the slab strides of edge + 1)."""
    p = edge + 1
    assert dpa.has_band_kernel(p, p)
    pairs = _pairs(p, p)  # all u x all v up to a padded edge of 32, as the unpadded placement test
    x = dp.basis_maps(p, p, pairs)[None, :, 1:, 1:].contiguous()
    for kind in ("square", "diag"):
        for K in (2, 4, 8):
            w = torch.from_numpy(bands.partition(p, p, K, kind))
            tol, e_ref = _tol(x, w, pad_front_if_odd=True)
            got = dpa.band_energy_nc(x.cuda(), w.cuda(), pad_front_if_odd=True, algo=algo).cpu()
            err = bo.band_error(got, x, w, pad_front_if_odd=True)
            print("BANDS_PLACE pad algo=%d %dx%d %s K=%d worst=%.3g E_ref=%.3g tol=%.3g" % (algo, edge, edge, kind, K, err, e_ref, tol))
            assert err <= tol


# ---------------------------------------------------------------------------------------------------------
# accuracy on activations
# ---------------------------------------------------------------------------------------------------------
def _hooked_shapes():
    """Every distinct (H, W, odd pad) the hooks of the seven nets score."""
    seen = set()
    for name, fn in schedules.SCHEDULES.items():
        for p in fn():
            seen.add((p.H, p.W, p.kind != "full" and p.H % 2 == 1))
    return sorted(seen)


@pytest.mark.parametrize("H,W,pad", _hooked_shapes())
def test_accuracy_on_activations(H, W, pad):
    hp, wp = H + int(pad), W + int(pad)
    fused = dpa.has_band_kernel(hp, wp)
    n, c = (2, 16) if H * W <= 64 * 64 else ((1, 8) if H * W <= 160 * 160 else (1, 4))
    g = torch.Generator().manual_seed(H * 1000 + W)
    cases = [("rand5", torch.rand(5, hp, wp, generator=g) * 2.0), ("square4", torch.from_numpy(bands.partition(hp, wp, 4, "square"))),
             ("diag8", torch.from_numpy(bands.partition(hp, wp, 8, "diag")))]
    for signed in (False, True):
        x = dp.random_maps(n, c, H, W, seed=H + 7 * W + int(signed), signed=signed)
        for label, w in cases:
            tol, e_ref = _tol(x, w, pad_front_if_odd=pad)
            got = dpa.band_energy_nc(x.cuda(), w.cuda(), pad_front_if_odd=pad).cpu()
            err = bo.band_error(got, x, w, pad_front_if_odd=pad)
            print("BANDS_ACC %s %dx%d pad=%d signed=%d %s worst=%.3g E_ref=%.3g tol=%.3g"
                  % ("fused" if fused else "fallback", H, W, pad, signed, label, err, e_ref, tol))
            assert err <= tol
            if fused:  # the two families on one shape
                alt = dpa.band_energy_nc(x.cuda(), w.cuda(), pad_front_if_odd=pad, algo=dpa.ALGO_DIRECT).cpu()
                err_alt = bo.band_error(alt, x, w, pad_front_if_odd=pad)
                print("BANDS_ACC fallback-on-codelet-shape %dx%d %s worst=%.3g" % (H, W, label, err_alt))
                assert err_alt <= tol


@pytest.mark.parametrize("H,W", [(100, 72), (260, 9)])
def test_accuracy_on_the_cosine_matrix_kernels_own_shapes(H, W):
    """A non-square map with an edge beyond 64 (one of them beyond 256): every coefficient the band reduction reads is a dot
    product of the cosine-matrix kernel. K = 4, channels 1 ... 3 of 5 in two samples: the slice is not contiguous."""
    assert not dpa.has_band_kernel(H, W)
    for signed in (False, True):
        x = dp.random_maps(2, 5, H, W, seed=H + 7 * W + int(signed), signed=signed)
        for kind in ("square", "diag"):
            w = torch.from_numpy(bands.partition(H, W, 4, kind))
            tol, e_ref = _tol(x[:, 1:4].contiguous(), w)
            got = dpa.band_energy_nc(x.cuda(), w.cuda(), c_begin=1, c_count=3)
            err = bo.band_error(got.cpu(), x, w, c_begin=1, c_count=3)
            print("BANDS_ACC fallback %dx%d signed=%d %s4 channels 1..3 of 5 worst=%.3g E_ref=%.3g tol=%.3g" % (H, W, signed, kind, err, e_ref, tol))
            assert err <= tol
            full = dpa.band_energy_nc(x.cuda(), w.cuda())
            assert torch.equal(got.view(torch.int32), full[:, 1:4].contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("H,pad,algo", [(14, False, 0), (56, False, 0), (8, False, 0), (9, True, 0), (7, False, 0), (72, False, 0),
                                        (28, False, 1)])
def test_a_maps_bands_depend_on_nothing_else(H, pad, algo):
    hp = H + int(pad and H % 2 == 1)
    n, c = (5, 11) if H <= 64 else (2, 6)
    x = dp.random_maps(n, c, H, H, seed=3).cuda()
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(4, hp, hp, generator=g) - 0.25).cuda()  # arbitrary floats, some negative
    kw = dict(pad_front_if_odd=pad, algo=algo)
    full = dpa.band_energy_nc(x, w, **kw)
    assert tuple(full.shape) == (n, c, 4) and full.dtype == torch.float32
    assert torch.equal(_bits(dpa.band_energy_nc(x, w, **kw)), _bits(full))                       # launch to launch
    assert torch.equal(_bits(dpa.band_energy_nc(x, w, c_begin=3, c_count=2, **kw)), _bits(full[:, 3:5]))  # channel slices
    assert torch.equal(_bits(dpa.band_energy_nc(x, w, c_begin=c - 1, **kw)), _bits(full[:, c - 1:]))
    for i in (0, n - 1):                                                                        # single samples
        assert torch.equal(_bits(dpa.band_energy_nc(x[i:i + 1], w, **kw)), _bits(full[i:i + 1]))
    perm = torch.randperm(n * c, generator=torch.Generator().manual_seed(2))                    # other maps permuted
    xp = x.reshape(1, n * c, H, H)[:, perm.cuda()].contiguous()
    assert torch.equal(_bits(dpa.band_energy_nc(xp, w, **kw))[0], _bits(full).reshape(n * c, 4)[perm.cuda()])
    # dead channels: +0.0 in every band
    dead = full[:, 5]
    assert (dead == 0).all() and not torch.signbit(dead).any()
    # K padded by zero-weight bands: +0.0 there, unchanged bits elsewhere (K = 3 -> 4 accumulators, 5 -> 8)
    for k_small, k_big in ((3, 4), (4, 6), (1, 2), (2, 8)):
        wz = torch.zeros(k_big, hp, hp, device="cuda")
        wz[:k_small] = w[:k_small]
        a = dpa.band_energy_nc(x, wz, **kw)
        b = dpa.band_energy_nc(x, w[:k_small].contiguous(), **kw)
        assert torch.equal(_bits(a[..., :k_small]), _bits(b)) and torch.equal(_bits(b), _bits(full[..., :k_small]))
        assert (a[..., k_small:] == 0).all() and not torch.signbit(a[..., k_small:]).any()


@pytest.mark.parametrize("H,pad", [(16, False), (56, False), (7, True), (7, False), (72, False), (20, False)])
def test_k1_against_the_existing_entry_points(H, pad):
    hp = H + int(pad and H % 2 == 1)
    x = dp.random_maps(3, 9, H, H, seed=5).cuda()
    ones = torch.ones(1, hp, hp, device="cuda")
    got = dpa.band_energy_nc(x, ones, pad_front_if_odd=pad)[..., 0]
    torch.testing.assert_close(got, dpa.energy_nc(x, pad_front_if_odd=pad), rtol=1e-5, atol=0)
    w = torch.rand(1, hp, hp, generator=torch.Generator().manual_seed(9)).cuda()
    got = dpa.band_energy_nc(x, w, pad_front_if_odd=pad)[..., 0]
    torch.testing.assert_close(got, dpa.weighted_energy_nc(x, w[0], pad_front_if_odd=pad), rtol=1e-5, atol=0)


@pytest.mark.parametrize("H,algo", [(14, 0), (56, 0), (9, 0), (28, 1), (72, 0)])
def test_nan_and_inf_maps_touch_only_their_own_bands(H, algo):
    x = dp.random_maps(3, 10, H, H, seed=8).cuda()
    w = torch.from_numpy(bands.partition(H, H, 4, "square")).cuda()
    fn = lambda t: dpa.band_energy_nc(t, w, algo=algo)
    e0 = fn(x).reshape(-1, 4)
    count = e0.shape[0]
    for value, m in ((float("nan"), count // 2), (float("inf"), count // 3)):
        y = x.clone()
        y.view(count, H, H)[m] = value
        e = fn(y).reshape(-1, 4)
        torch.cuda.synchronize()
        assert not torch.isfinite(e[m]).any()
        keep = torch.ones(count, dtype=torch.bool, device="cuda")
        keep[m] = False
        assert torch.equal(_bits(e[keep]), _bits(e0[keep]))


@pytest.mark.parametrize("H,pad", [(14, False), (56, False), (9, True), (72, False)])
def test_misaligned_base_pitched_rows_and_guard_words(H, pad):
    hp = H + int(pad and H % 2 == 1)
    n, c, K = 2, 6, 3
    src = dp.random_maps(n, c, H, H, seed=4)
    w = torch.rand(K, hp, hp, generator=torch.Generator().manual_seed(6))
    ref = dpa.band_energy_nc(src.cuda(), w.cuda(), pad_front_if_odd=pad)
    tol, e_ref = _tol(src, w, pad_front_if_odd=pad)
    # a base that is only 4-byte aligned: the fused kernel's bits do not change; the fallback's coefficient path picks
    # its kernel by alignment (the large-tile kernels need 16 bytes), so there the bound applies
    buf = torch.zeros(n * c * H * H + 8, device="cuda")
    for off in (1, 3):
        v = buf[off:off + n * c * H * H].view(n, c, H, H)
        v.copy_(src)
        assert v.data_ptr() % 16 != 0
        got = dpa.band_energy_nc(v, w.cuda(), pad_front_if_odd=pad)
        if dpa.has_band_kernel(hp, hp):
            assert torch.equal(_bits(got), _bits(ref))
        else:
            assert bo.band_error(got.cpu(), src, w, pad_front_if_odd=pad) <= tol
    # a row-pitched crop (strideH > W): the fallback's coefficient path, within the bound of the fused result
    wide = torch.zeros(n, c, H, H + 3)
    wide[..., :H] = src
    wide[..., H:] = 7.0
    crop = wide.cuda()[..., :H]
    assert crop.stride(2) == H + 3
    got = dpa.band_energy_nc(crop, w.cuda(), pad_front_if_odd=pad).cpu()
    err = bo.band_error(got, src, w, pad_front_if_odd=pad)
    print("BANDS_PITCH %dx%d worst=%.3g tol=%.3g" % (H, H, err, tol))
    assert err <= tol
    # outputs inside guard words only: the raw entry point writes [N, c_count, K] and not a float more
    lib = _lib.load()
    x = src.cuda()
    wd = w.cuda()
    guard = 16
    out = torch.full((n * 4 * K + 2 * guard,), -123.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for algo in (0, 1):
        out.fill_(-123.0)
        ws = torch.empty(lib.dcts_band_workspace_bytes(n, 4, H, H, K) + 256, dtype=torch.uint8, device="cuda")
        body = out[guard:guard + n * 4 * K]
        _lib.check(lib.dcts_band_energy_f32(x.data_ptr(), n, c, H, H, x.stride(0), x.stride(1), x.stride(2), 1, 1, 4,
                                            1 if pad else 0, wd.data_ptr(), K, body.data_ptr(), ws.data_ptr(),
                                            ws.numel() - 256, stream, algo))
        lib.dcts_workspace_invalidate_range(ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        assert (out[:guard] == -123.0).all() and (out[guard + n * 4 * K:] == -123.0).all()
        if algo == 0:
            assert torch.equal(_bits(body.view(n, 4, K)), _bits(ref[:, 1:5]))


def test_fused_only_and_bad_arguments():
    x = torch.zeros(1, 2, 72, 72, device="cuda")
    w = torch.ones(2, 72, 72, device="cuda")
    with pytest.raises(_lib.DctScoreError) as e:
        dpa.band_energy_nc(x, w, algo=dpa.ALGO_CODELET)
    assert e.value.code == -6
    out = dpa.band_energy_nc(x, w)
    assert (out == 0).all() and not torch.signbit(out).any()
    with pytest.raises(ValueError):
        dpa.band_energy_nc(x, torch.ones(2, 71, 72, device="cuda"))
    with pytest.raises(_lib.DctScoreError) as e:
        dpa.band_energy_nc(x, torch.ones(9, 72, 72, device="cuda"))
    assert e.value.code == -2


# ---------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------
def _memoise(net, pts, limit, cache):
    """The same activations for every sweep: the first time a hooked module sees batch i its scored tensor is kept, and
    every later sweep (the per-hook mode runs one per hook point, the other modes one more each) gets that tensor back
    in place of its own. Convolutions on the GPU are not bit-reproducible from sweep to sweep (measured here: ResNet-50
    at 224, differences of 1e-7 of a map's norm), and a nearly empty band magnifies that to 2e-3 of the band; with the
    tensors pinned, what is compared is the harness and the kernel. The hooks are registered before imp_score's."""
    handles, seen = [], {}

    def key_of(path):
        i = seen.get(path, 0)
        seen[path] = i + 1
        return (path, i % limit)

    for p in pts:
        mod = harness._resolve(net, p.module)
        if p.kind == "input":
            def pre(m, args, _p=p.module):
                k = key_of(_p)
                if k not in cache:
                    cache[k] = args[0].detach().clone()
                return (cache[k].clone(),) + tuple(args[1:])
            handles.append(mod.register_forward_pre_hook(pre))
        else:
            def post(m, args, out, _p=p.module):
                k = key_of(_p)
                if k not in cache:
                    cache[k] = out.detach().clone()
                return cache[k].clone()
            handles.append(mod.register_forward_hook(post))
    return handles


def _run(name, root, size, bs, limit, cfg, as_dict=False, cache=None, **kw):
    import contextlib
    import io
    import types
    net = deterministic_init(nets.get_network(name)).cuda()
    memo = _memoise(net, harness._schedule_for(net, name), limit, cache) if cache is not None else []
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=11, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.makedirs(str(root), exist_ok=True)
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(net, args, train_loader=loader, criterion="bands", bands=cfg, **kw)
    finally:
        os.chdir(cwd)
        for h in memo:
            h.remove()
    d = os.path.join(str(root), "band_score", "%s_limit%d_%s%d" % (name, limit, cfg[1], cfg[0]))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.mark.parametrize("name,size,bs,cfg,as_dict", [("resnet_56", 32, 4, (4, "square"), False),
                                                     ("resnet_50", 224, 2, (4, "diag"), False),
                                                     ("u2netp", 288, 1, (8, "square"), True)])
def test_harness_modes_agree(name, size, bs, cfg, as_dict, tmp_path):
    limit = 2 if name != "u2netp" else 1
    pts = schedules.SCHEDULES[name]()
    runs, cache = {}, {}
    for mode, kw in [("per_hook", {}), ("single", {"single_sweep": True}),
                     ("device", {"single_sweep": True, "accumulate": "device"})]:
        runs[mode] = _run(name, tmp_path / mode, size, bs, limit, cfg, as_dict, cache=cache, **kw)
    base = runs["per_hook"]
    assert len(base) == sum(len(p.files) for p in pts)
    for mode, files in runs.items():
        assert sorted(files) == sorted(base), mode
        for k, v in files.items():
            assert v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == cfg[0], (mode, k)
            np.testing.assert_allclose(v, base[k], rtol=1e-4, atol=0, err_msg="%s %s" % (mode, k))
    # the spectrum adds up to the dct criterion's score on the same (pinned) activations
    for pt in (pts[1], pts[-1]):
        cb, cc, pad = schedules.scored_shape(pt)
        acc = harness.HostAccumulator()
        for i in range(limit):
            acc.update(dpa.energy_nc(cache[(pt.module, i)], cb, cc, pad))
        stem = harness._file_stem("bands", pt.files[0][0])
        lo, hi = pt.files[0][1], pt.files[0][2]
        want = acc.scores() if lo is None else acc.scores()[lo:hi]
        np.testing.assert_allclose(base[stem].astype(np.float64).sum(1), want, rtol=1e-4)


def test_cli_writes_the_spectrum_directory(tmp_path):
    from test_cli_gpu import run_cli
    common = ["--net", "vgg_16_bn", "--dataset", "cifar10", "--synthetic", "--pretrain_dir", "", "--batch_size", "32",
              "--limit", "2", "--single_sweep"]
    out = run_cli(tmp_path, *common, "--criterion", "bands", "--bands", "4", "--band_kind", "square")
    assert "The importance score generation has been completed!" in out
    d = tmp_path / "band_score" / "vgg_16_bn_limit2_square4"
    assert sorted(os.listdir(d)) == sorted("band_conv%d.npy" % i for i in range(1, 13))
    for p, i in zip(schedules.vgg_16_bn(), range(1, 13)):
        a = np.load(d / ("band_conv%d.npy" % i))
        assert a.dtype == np.float32 and a.shape == (p.C, 4) and (a >= 0).all()
    assert not (tmp_path / "importance_score").exists()
    assert masks.main(["--imp_score", str(d), "--band_weights", "1,0.5,0.25,0", "--compress_rate", "[0.50]*7+[0.95]*5"]) == 0
    coll = tmp_path / "collapsed"
    assert bands.main(["--spectrum", str(d), "--band_weights", "1,1,1,1", "--out", str(coll)]) == 0
    assert sorted(os.listdir(coll)) == sorted("imp_conv%d.npy" % i for i in range(1, 13))


@pytest.mark.parametrize("name,bs", [("vgg_16_bn", 32), ("resnet_56", 16)])
def test_collapse_with_all_ones_gives_the_dct_masks_on_the_same_activations(name, bs, tmp_path):
    """One sweep; every hook point scores the SAME tensor with the dct criterion's operator and with the band operator
    (two processes, or two sweeps, do not see bit-identical activations). The spectra go through the files and
    bands.collapse, the masks are taken at the README compress rates."""
    from mask_parity import readme_kept
    limit, cfg = 2, (4, "square")
    net = deterministic_init(nets.get_network(name)).cuda()
    pts = harness._schedule_for(net, name)
    acc_d = [harness.HostAccumulator() for _ in pts]
    acc_b = [harness.HostAccumulator() for _ in pts]

    def make(i, pt):
        def hook(m, inputs, out):
            x = inputs[0] if pt.kind == "input" else out
            cb, cc, pad = schedules.scored_shape(pt._replace(C=x.shape[1]))
            hp = x.shape[2] + int(pad and x.shape[2] % 2 == 1)
            w = torch.from_numpy(bands.partition(hp, hp, *cfg)).cuda()
            acc_d[i].update(dpa.energy_nc(x, cb, cc, pad))
            acc_b[i].update(dpa.band_energy_nc(x, w, cb, cc, pad))
        return hook

    handles = [harness._resolve(net, pt.module).register_forward_hook(make(i, pt)) for i, pt in enumerate(pts)]
    harness.inference(net, SyntheticLoader((3, 32, 32), bs, limit + 1, seed=11), limit)
    for h in handles:
        h.remove()
    spec_dir, dct_dir = tmp_path / "spec", tmp_path / "dct"
    os.makedirs(spec_dir)
    os.makedirs(dct_dir)
    for i, pt in enumerate(pts):
        harness._save(str(spec_dir), name, pt, np.ascontiguousarray(acc_b[i].scores().reshape(-1, cfg[0]), dtype=np.float32), "bands")
        harness._save(str(dct_dir), name, pt, np.ascontiguousarray(acc_d[i].scores(), dtype=np.float32))
    coll = tmp_path / "collapsed"
    bands.collapse(str(spec_dir), np.ones(cfg[0]), str(coll))
    kept = readme_kept(name)
    assert kept
    for stem, k in kept.items():
        a, b = np.load(coll / (stem + ".npy")), np.load(dct_dir / (stem + ".npy"))
        np.testing.assert_allclose(a, b, rtol=1e-5, err_msg=stem)
        np.testing.assert_array_equal(masks.select_index(a, a.size, k), masks.select_index(b, b.size, k), err_msg=stem)
