"""channels_last feature maps on the GPU (dcts_energy_nhwc / ops.energy_nc / imp_score(channels_last=True) / the CLI).

The reference value everywhere is the float64 energy of the EXACTLY upcast input, and the bound is the rule of
tests/dct_probes.py (8 x the fp32 reference's own round-off on the same maps, floor 2^-22). The maps of
a sweep are laid out channels_last with the map index on the channel axis."""
import contextlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dct_probes as dp
import dct_pruning_amd as dpa
from dct_pruning_amd import harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import deterministic_init
from oracle import dct_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NATIVE_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
CL = torch.channels_last


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cl(x):
    """x [N, C, H, W] as a channels_last tensor on the GPU that really has the channel stride 1."""
    y = x.cuda().contiguous(memory_format=CL)
    assert x.shape[1] == 1 or (y.stride(1) == 1 and y.stride(3) == x.shape[1])
    return y


def _nhwc_fn(dtype):
    """energy_fn for dct_probes: x [N, C, H, W] fp32, exactly representable in `dtype`, scored in channels_last with all
    N * C maps on the channel axis of one sample."""
    def fn(x):
        n, c, h, w = x.shape
        xh = x.reshape(1, n * c, h, w).to(dtype)
        assert torch.equal(xh.float(), x.reshape(1, n * c, h, w))
        y = _cl(xh)
        assert dpa.ops.energy_route(y.shape, y.stride()) == dpa.ops.ROUTE_NHWC
        return dpa.energy_nc(y).cpu().reshape(n, c)
    return fn


def _rounded(x, dtype):
    return x.to(dtype).float()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", NATIVE_EDGES)
def test_native_edges_within_the_fp32_bound(n, dt):
    dtype = DTYPES[dt]
    assert dpa.has_nhwc_kernel(n, n)
    fn = _nhwc_fn(dtype)
    pairs = dp.cover(n, n)
    worst = {}
    for what, make in (("basis", lambda p: _rounded(dp.basis_maps(n, n, p), dtype)),
                       ("impulse", lambda p: _rounded(dp.impulse_maps(n, n, p, seed=n), dtype))):
        tol, e_ref = dp.sweep_tolerance(make, pairs, n, n)
        worst[what] = (dp.sweep(fn, make, pairs, n, n, tol, what), tol)
    g = torch.Generator().manual_seed(100 + n)
    sub = (torch.randint(1, 1024, (3, 20, n, n), generator=g).float() * 2.0 ** -24)  # fp16 subnormals, exact in fp32
    sets = {"relu": _rounded(dp.random_maps(5, 40, n, n, seed=n), dtype),
            "signed": _rounded(dp.random_maps(5, 40, n, n, seed=n + 1, signed=True), dtype),
            "subnormal": _rounded(sub, dtype)}
    for what, x in sets.items():
        tol = dp.tolerance(dp.reference_error(x))
        worst[what] = (dp.check_energy(fn, x, tol, what=what), tol)
        # against the NCHW route on the same values: within the sum of the two tolerances (bit equality is reported)
        xc = _cl(x.to(dtype))
        a, b = dpa.energy_nc(xc).cpu(), dpa.energy_nc(xc.contiguous()).cpu()
        ref = dp.parseval(x)
        nz = ref > 0
        assert ((a.double() - b.double()).abs()[nz] / ref[nz]).max().item() <= 2 * tol, what
        assert torch.equal(a[~nz], b[~nz])
        worst[what + "_biteq_nchw_route"] = bool(torch.equal(_bits(a), _bits(b)))
    print("NHWC_NATIVE %s %dx%d %s" % (dt, n, n, " ".join("%s=%s" % kv for kv in sorted(worst.items()))))


def _check_f64(e, x, what):
    """e [N, c] against the float64 energy of x [N, c, H, W] (already the scored slice, on the CPU, fp32 values)."""
    tol = dp.tolerance(dp.reference_error(x))
    ref = dp.parseval(x)
    nz = ref > 0
    e = e.cpu()
    assert ((e.double() - ref).abs()[nz] / ref[nz]).max().item() <= tol, what
    assert (e[~nz] == 0).all() and not torch.signbit(e[~nz]).any(), what


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", NATIVE_EDGES)
def test_native_contract(n, dt):
    dtype = DTYPES[dt]
    big = dp.random_maps(3, 130, n, n, seed=7 * n).to(dtype)
    big[:, 3] = 0
    xd = _cl(big)
    full = dpa.energy_nc(xd)
    assert full.dtype == torch.float32 and tuple(full.shape) == (3, 130)
    _check_f64(full, big.float(), "C=130")
    assert (full[:, 3] == 0).all() and not torch.signbit(full[:, 3]).any()  # an all-zero map: +0.0 bits
    assert (_bits(full[:, 3]) == 0).all()
    # the same maps in tensors of C = 3, 17, 64, 67 channels (tail lanes, C < CB, C < 64, one block or wave plus a remainder):
    # against float64 and bit for bit against their place in the 130-channel tensor
    for C in (3, 17, 64, 67):
        for lo in (0, 130 - C):
            y = _cl(big[:, lo:lo + C])
            assert y.stride(3) == C
            e = dpa.energy_nc(y)
            _check_f64(e, big[:, lo:lo + C].float(), "C=%d" % C)
            assert torch.equal(_bits(e), _bits(full[:, lo:lo + C])), (C, lo)
    # c_begin / c_count slices that are aligned to nothing
    for cb, cc in ((5, 61), (0, 1), (129, 1), (63, 2), (31, 66)):
        e = dpa.energy_nc(xd, c_begin=cb, c_count=cc)
        assert torch.equal(_bits(e), _bits(full[:, cb:cb + cc])), (cb, cc)
    # a channel-sliced view: strideW > C and, for half, a base at an odd element offset
    v = xd[:, 7:40]
    assert v.stride(3) == 130 and v.stride(1) == 1 and v.storage_offset() % 2 == 1
    assert dpa.ops.energy_route(v.shape, v.stride()) == dpa.ops.ROUTE_NHWC
    assert torch.equal(_bits(dpa.energy_nc(v)), _bits(full[:, 7:40]))
    assert torch.equal(_bits(dpa.energy_nc(v, c_begin=2, c_count=9)), _bits(full[:, 9:18]))
    # a sample-pitched view, and one sample alone
    assert torch.equal(_bits(dpa.energy_nc(xd[::2])), _bits(full[::2]))
    assert torch.equal(_bits(dpa.energy_nc(xd[1:2])), _bits(full[1:2]))
    # one NaN map changes no other output; power-of-two scaling is exact
    fn = lambda x: dpa.energy_nc(_cl(x.to(dtype))).cpu()  # noqa: E731
    small = big[:, :67].float()
    dp.check_isolation(fn, small)
    if dtype == torch.float16:
        # 2^+-20 leaves fp16's range: 2^+-4 on multiples of 1/8 below 128 (10 significant bits, normal after either scaling)
        dp.check_pow2_scaling(fn, (small * 8).round().clamp(max=1000) / 8, k=4)
    else:
        dp.check_pow2_scaling(fn, small)
    # out= is honoured, and nothing but [N, c_count] floats is written
    guard = 16
    buf = torch.full((3 * 12 + 2 * guard,), -123.0, device="cuda")
    body = buf[guard:guard + 36].view(3, 12)
    assert dpa.energy_nc(xd, c_begin=118, c_count=12, out=body) is body
    torch.cuda.synchronize()
    assert (buf[:guard] == -123.0).all() and (buf[guard + 36:] == -123.0).all()
    assert torch.equal(_bits(body), _bits(full[:, 118:]))


@pytest.mark.parametrize("n", NATIVE_EDGES)
def test_explicit_algo_takes_the_copy_route(n):
    x = _cl(dp.random_maps(3, 17, n, n, seed=n))
    for algo in (dpa.ALGO_CODELET, dpa.ALGO_DIRECT):
        assert torch.equal(_bits(dpa.energy_nc(x, algo=algo)), _bits(dpa.energy_nc(x.contiguous(), algo=algo)))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_other_shapes_are_the_contiguous_route(dt):
    dtype = DTYPES[dt]
    for (h, w), pad in (((7, 7), True), ((72, 72), False), ((56, 28), False)):
        x = _cl(dp.random_maps(2, 5, h, w, seed=h + w).to(dtype))
        assert dpa.ops.energy_route(x.shape, x.stride(), pad) == dpa.ops.ROUTE_COPY
        got = dpa.energy_nc(x, pad_front_if_odd=pad)
        assert torch.equal(_bits(got), _bits(dpa.energy_nc(x.contiguous(), pad_front_if_odd=pad))), (h, w)


def test_no_copy_is_allocated():
    x = _cl(dp.random_maps(8, 256, 28, 28, seed=3))
    nbytes = x.numel() * x.element_size()
    out = torch.empty(8, 256, device="cuda")
    dpa.energy_nc(x.contiguous(), out=out)  # warms the workspace with an NCHW call of the same shape
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    dpa.energy_nc(x, out=out)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < nbytes // 4, (rise, nbytes)


# ---------------------------------------------------------------------------------------------------------
# harness and CLI
# ---------------------------------------------------------------------------------------------------------
def _capture_run(name, root, bs, limit, size, net=None, **kw):
    """imp_score on the GPU with a capturing hook ahead of every scoring hook: the files, stdout, the layouts the hooks saw
    and, per file, the float64 expectation on that run's own activations together with its tolerance."""
    dev = torch.device("cuda")
    if net is None:
        net = deterministic_init(nets.get_network(name)).to(dev)
    pts = harness._schedule_for(net, name)
    acts, layouts = {}, {}

    def capture(mod, i, o, _p=None):
        if len(mod._forward_hooks) > 1:  # the scoring hook is registered: this sweep scores this module
            t = (i[0] if _p.kind == "input" else o).detach()
            route = dpa.ops.energy_route(t.shape, t.stride(), _p.kind != "full")
            layouts[route] = layouts.get(route, 0) + 1
            acts.setdefault(_p.module, []).append(t.cpu().contiguous())

    handles = [harness._resolve(net, p.module).register_forward_hook(lambda m, i, o, _p=p: capture(m, i, o, _p))
               for p in pts]
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=11, as_dict=False)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.makedirs(str(root), exist_ok=True)
    cwd = os.getcwd()
    os.chdir(str(root))
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            harness.imp_score(net, args, train_loader=loader, **kw)
    finally:
        os.chdir(cwd)
        for h in handles:
            h.remove()
    d = os.path.join(str(root), "importance_score", "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    expect, tols = {}, {}
    for p in pts:
        batches = acts[p.module]
        assert len(batches) == limit
        total, tol = 0.0, 0.0
        for a in batches:
            cb, cc, pad = schedules.scored_shape(p._replace(C=a.shape[1]))
            a32 = a[:, cb:cb + cc].float()
            total = total + orc.energy_nc_f64(a32, pad_front_if_odd=pad).sum(0)
            tol = max(tol, dp.tolerance(dp.reference_error(a32[:, :64], pad_front_if_odd=pad)))
        mean = total / (limit * batches[0].shape[0])
        for stem, lo, hi in p.files:
            expect[stem] = mean if lo is None else mean[lo:hi]
            tols[stem] = tol
    return files, buf.getvalue().splitlines(), expect, tols, layouts


def _check_files(files, expect, tols):
    assert sorted(files) == sorted(expect)
    for k, v in files.items():
        ref = expect[k]
        assert v.dtype == np.float32 and v.shape == ref.shape, k
        assert np.all(v[ref == 0] == 0), k
        # every map is within tol of its float64 energy; the fp32 batch sum and running mean add one rounding per accumulated
        # sample (8 at most here) and three per update, 2^-24 each - 16 * 2^-24 covers them
        nz = ref > 0
        err = np.abs(v.astype(np.float64) - ref)[nz] / ref[nz]
        assert err.size == 0 or err.max() <= tols[k] + 16 * 2.0 ** -24, (k, err.max(), tols[k])


@pytest.mark.parametrize("autocast", [None, "bf16"])
@pytest.mark.parametrize("name,bs,size", [("resnet_56", 2, 32), ("vgg_16_bn", 4, 32), ("resnet_50", 2, 224)])
def test_imp_score_channels_last_scores_its_own_activations(name, bs, size, autocast, tmp_path):
    files, lines, expect, tols, layouts = _capture_run(name, tmp_path / "cl", bs, 1, size, channels_last=True, autocast=autocast)
    _check_files(files, expect, tols)
    assert lines[-1] == "The importance score generation has been completed!"
    print("NHWC_HARNESS %s autocast=%s routes seen by the hooks (1 NCHW, 2 NHWC, 3 copy): %s" % (name, autocast, sorted(layouts.items())))


class _Pinned(torch.nn.Module):
    """The harness nets run MIOpen convolutions that are not bit-reproducible between sweeps. This one pins the
    activations: a fixed channels_last tensor per hooked module, whatever the input."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.relu1, self.relu2, self.relu3 = torch.nn.ReLU(), torch.nn.ReLU(), torch.nn.ReLU()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.acts = [torch.relu(torch.randn(4, c, e, e, generator=g)).contiguous(memory_format=CL)
                     for c, e in ((24, 32), (40, 16), (70, 8))]

    def forward(self, x):
        for m, a in zip((self.relu1, self.relu2, self.relu3), self.acts):
            m(a.to(x.device))
        return x


def test_modes_agree_on_pinned_activations(tmp_path, monkeypatch):
    from dct_pruning_amd.schedules import HookPoint
    net = _Pinned().cuda()
    pts = [HookPoint("relu%d" % (i + 1), "full", [("imp_pin%d" % i, None, None)], a.shape[1], a.shape[2], a.shape[3])
           for i, a in enumerate(net.acts)]
    monkeypatch.setitem(schedules.SCHEDULES, "vgg_16_bn", lambda: pts)
    runs = {}
    for mode, kw in [("per_hook", {}), ("single", {"single_sweep": True}),
                     ("device", {"single_sweep": True, "accumulate": "device"})]:
        files, lines, expect, tols, layouts = _capture_run("vgg_16_bn", tmp_path / mode, 4, 2, 32, net=net, channels_last=True, **kw)
        assert set(layouts) == {dpa.ops.ROUTE_NHWC}
        _check_files(files, expect, tols)
        runs[mode] = (files, lines)
    base, base_lines = runs["per_hook"]
    for mode, (files, lines) in runs.items():
        assert lines == base_lines and sorted(files) == sorted(base), mode
        for k in base:
            np.testing.assert_allclose(files[k], base[k], rtol=1e-4, atol=0, err_msg="%s %s" % (mode, k))


def test_cli_channels_last(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.join(ROOT, "importance_generation.py"),
                        "--net", "resnet_56", "--dataset", "cifar10", "--synthetic", "--pretrain_dir", "", "--batch_size", "16",
                        "--limit", "1", "--channels_last"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "The importance score generation has been completed!" in p.stdout
    d = tmp_path / "importance_score" / "resnet_56_limit1"
    want = sorted(stem + ".npy" for pt in schedules.resnet_56() for stem, _, _ in pt.files)
    assert sorted(os.listdir(d)) == want
    for f in want:
        a = np.load(d / f)
        assert a.dtype == np.float32 and np.isfinite(a).all() and (a >= 0).all()
