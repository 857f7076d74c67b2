"""fp16 / bf16 feature maps on the GPU (dcts_energy_typed / ops.energy_nc / imp_score(autocast=...) / the CLI).

The reference value everywhere is the float64 energy of the EXACTLY upcast input (x.float().double()), so the
quantisation of the input is not part of the error; the bound is the rule of tests/dct_probes.py (8 x the fp32
reference's own round-off on the same maps, floor 2^-22). The staged shapes must give the bits of
the fp32 path on a dense fp32 copy, because the same kernels see the same values."""
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
from dct_pruning_amd import _lib, harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import deterministic_init
from oracle import dct_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NATIVE_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _half_fn(dtype):
    """energy_fn for dct_probes: the fp32 maps it is given are exactly representable in `dtype` (rounded beforehand)."""
    def fn(x):
        xh = x.to(dtype)
        assert torch.equal(xh.float(), x)
        return dpa.energy_nc(xh.cuda()).cpu()
    return fn


def _rounded(x, dtype):
    return x.to(dtype).float()


# ---------------------------------------------------------------------------------------------------------
# native edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", NATIVE_EDGES)
def test_native_edges_within_the_fp32_bound(n, dt):
    dtype = DTYPES[dt]
    assert dpa.has_half_kernel(n, n)
    fn = _half_fn(dtype)
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
    if dtype == torch.float16:
        assert torch.equal(sets["subnormal"], sub) and (sub.half().abs() < 2.0 ** -14).all()
    for what, x in sets.items():
        tol = dp.tolerance(dp.reference_error(x))
        worst[what] = (dp.check_energy(fn, x, tol, what=what), tol)
        # the route of the parent commit, upcast first: within the same bound of each other (bit equality is reported)
        xh = x.to(dtype).cuda()
        a, b = dpa.energy_nc(xh).cpu(), dpa.energy_nc(xh.float()).cpu()
        ref = dp.parseval(x)
        nz = ref > 0
        assert ((a.double() - b.double()).abs()[nz] / ref[nz]).max().item() <= tol, what
        assert torch.equal(a[~nz], b[~nz])
        worst[what + "_biteq_fp32_path"] = bool(torch.equal(_bits(a), _bits(b)))
    print("HALF_NATIVE %s %dx%d %s" % (dt, n, n, " ".join("%s=%s" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", NATIVE_EDGES)
def test_native_contract(n, dt):
    dtype = DTYPES[dt]
    G = 64 // n
    C = 29  # with N = 3: 87 maps, a ragged last group at every edge but 2 and 4 ... and 257 * 29 is odd as well
    x = dp.random_maps(257, C, n, n, seed=7 * n).to(dtype)
    x[:, 3] = 0
    xd = x.cuda()
    full = dpa.energy_nc(xd)
    assert full.dtype == torch.float32 and tuple(full.shape) == (257, C)
    # an all-zero map: +0.0
    assert (full[:, 3] == 0).all() and not torch.signbit(full[:, 3]).any()
    # the same bits alone, inside N = 1 / 3 / 257 and through a channel slice
    assert torch.equal(_bits(dpa.energy_nc(xd[:1])), _bits(full[:1]))
    assert torch.equal(_bits(dpa.energy_nc(xd[:3])), _bits(full[:3]))
    assert torch.equal(_bits(dpa.energy_nc(xd[5:6, 7:8].contiguous())), _bits(full[5:6, 7:8]))
    assert torch.equal(_bits(dpa.energy_nc(xd, c_begin=C - 12, c_count=12)), _bits(full[:, C - 12:]))
    assert torch.equal(_bits(dpa.energy_nc(xd[:3], c_begin=1, c_count=5)), _bits(full[:3, 1:6]))
    # a base that is 2-byte aligned only (an odd element offset): the same bits
    flat = torch.zeros(3 * C * n * n + 1, dtype=dtype, device="cuda")
    flat[1:] = xd[:3].reshape(-1)
    assert torch.equal(_bits(dpa.energy_nc(flat[1:].view(3, C, n, n))), _bits(full[:3]))
    # a ragged last group: one map more than whole groups
    m = 5 * G + 1
    y = xd.reshape(-1, n, n)[:m].reshape(1, m, n, n)
    assert torch.equal(_bits(dpa.energy_nc(y)), _bits(full.reshape(-1)[:m].reshape(1, m)))
    # one NaN changes one output
    z = xd[:3].clone()
    z[1, 11, n // 2, n - 1] = float("nan")
    e = dpa.energy_nc(z)
    keep = torch.ones(3, C, dtype=torch.bool, device="cuda")
    keep[1, 11] = False
    assert torch.isnan(e[1, 11]) and torch.equal(_bits(e[keep]), _bits(full[:3][keep]))
    # out= is honoured, and nothing but [N, c_count] floats is written
    out = torch.empty(3, 12, device="cuda")
    assert dpa.energy_nc(xd[:3], c_begin=C - 12, c_count=12, out=out) is out
    assert torch.equal(_bits(out), _bits(full[:3, C - 12:]))
    guard = 16
    buf = torch.full((3 * 12 + 2 * guard,), -123.0, device="cuda")
    body = buf[guard:guard + 36].view(3, 12)
    dpa.energy_nc(xd[:3], c_begin=C - 12, c_count=12, out=body)
    torch.cuda.synchronize()
    assert (buf[:guard] == -123.0).all() and (buf[guard + 36:] == -123.0).all()
    assert torch.equal(_bits(body), _bits(full[:3, C - 12:]))
    with pytest.raises(ValueError):
        dpa.energy_nc(xd[:1], algo=dpa.ALGO_CODELET)


# ---------------------------------------------------------------------------------------------------------
# every other shape: staged through the fp32 kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------
FALLBACK = [  # (N, C, H, W, pad, pitched, c_begin, c_count)
    (3, 10, 7, 7, True, False, 0, None),
    (3, 10, 13, 13, True, False, 2, 6),
    (3, 10, 13, 13, False, False, 0, None),
    (3, 10, 56, 28, False, False, 1, 8),
    (3, 10, 28, 28, False, True, 2, 7),
    (2, 5, 72, 72, False, False, 1, 3),
    (2, 5, 144, 144, False, False, 0, None),
    (2, 4, 224, 224, False, False, 0, 3),
    (5, 48, 288, 288, False, False, 0, None),  # 240 maps of 324 KiB: more than one 64 MiB chunk
]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("N,C,H,W,pad,pitched,cb,cc", FALLBACK)
def test_staged_shapes_equal_the_fp32_path_bit_for_bit(N, C, H, W, pad, pitched, cb, cc, dt):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(H * 1000 + W)
    if pitched:
        x = torch.relu(torch.randn(N, C, H, W + 4, generator=g)).to(dtype).cuda()[..., :W]
        assert x.stride(2) == W + 4
    else:
        x = torch.relu(torch.randn(N, C, H, W, generator=g)).to(dtype).cuda()
    x[:, C - 1] = 0
    cc_ = C - cb if cc is None else cc
    if H == 288:
        lib = _lib.load()
        assert lib.dcts_typed_workspace_bytes(1, N, cc_, H, W) - lib.dcts_workspace_bytes(N, cc_, H, W) < N * cc_ * H * W * 4
    got = dpa.energy_nc(x, c_begin=cb, c_count=cc, pad_front_if_odd=pad)
    want = dpa.energy_nc(x[:, cb:cb + cc_].float().contiguous(), pad_front_if_odd=pad)
    assert tuple(got.shape) == (N, cc_)
    assert torch.equal(_bits(got), _bits(want))
    if cb + cc_ == C:
        assert (got[:, -1] == 0).all() and not torch.signbit(got[:, -1]).any()
    # and within the bound of the float64 energy of the upcast maps (small shapes: the CPU reference is slow beyond)
    if H <= 72:
        xs = x[:, cb:cb + cc_].float().cpu()
        ref = torch.from_numpy(orc.energy_nc_f64(xs, pad_front_if_odd=pad))
        tol = dp.tolerance(dp.reference_error(xs, pad_front_if_odd=pad))
        nz = ref > 0
        assert ((got.cpu().double() - ref).abs()[nz] / ref[nz]).max().item() <= tol


def test_channel_run_chunks_when_the_workspace_holds_less_than_a_sample():
    """The raw entry point with a workspace of three upcast maps: runs of channels of one sample, the same bits."""
    lib = _lib.load()
    N, C, H = 2, 7, 72
    g = torch.Generator().manual_seed(9)
    x = torch.relu(torch.randn(N, C, H, H, generator=g)).half().cuda()
    want = dpa.energy_nc(x.float())
    inner = (lib.dcts_workspace_bytes(N, C, H, H) + 255) // 256 * 256
    ws = torch.empty(inner + 3 * H * H * 4 + 100, dtype=torch.uint8, device="cuda")
    out = torch.full((N, C), -1.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dcts_energy_typed(x.data_ptr(), 1, N, C, H, H, x.stride(0), x.stride(1), x.stride(2), 1, 0, C, 0,
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    lib.dcts_workspace_invalidate_range(ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    # dtype 0 is dcts_energy_f32
    xf = x.float()
    ws = torch.empty(max(lib.dcts_typed_workspace_bytes(0, N, C, H, H), 16), dtype=torch.uint8, device="cuda")
    out.fill_(-1.0)
    _lib.check(lib.dcts_energy_typed(xf.data_ptr(), 0, N, C, H, H, xf.stride(0), xf.stride(1), xf.stride(2), 1, 0, C, 0,
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    lib.dcts_workspace_invalidate_range(ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))


# ---------------------------------------------------------------------------------------------------------
# harness and CLI
# ---------------------------------------------------------------------------------------------------------
def _capture_run(name, root, bs, limit, size, as_dict, net=None, want=True, **kw):
    """imp_score on the GPU with a capturing hook ahead of every scoring hook: the files, stdout, the dtypes the hooks
    saw and, per file, the float64 expectation on that run's own activations together with its tolerance."""
    dev = torch.device("cuda")
    if net is None:
        net = deterministic_init(nets.get_network(name)).to(dev)
    pts = harness._schedule_for(net, name)
    acts = {}

    def capture(mod, i, o, _p=None):
        if len(mod._forward_hooks) > 1:  # the scoring hook is registered: this sweep scores this module
            acts.setdefault(_p.module, []).append((i[0] if _p.kind == "input" else o).detach().cpu())

    handles = [harness._resolve(net, p.module).register_forward_hook(lambda m, i, o, _p=p: capture(m, i, o, _p))
               for p in pts]
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=11, as_dict=as_dict)
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
    expect, tols, dtypes = {}, {}, set()
    for p in pts:
        batches = acts[p.module]
        assert len(batches) == limit
        total, tol = 0.0, 0.0
        for a in batches:
            dtypes.add(a.dtype)
            if not want:
                continue
            cb, cc, pad = schedules.scored_shape(p._replace(C=a.shape[1]))
            a32 = a[:, cb:cb + cc].float()
            total = total + orc.energy_nc_f64(a32, pad_front_if_odd=pad).sum(0)
            tol = max(tol, dp.tolerance(dp.reference_error(a32[:, :64], pad_front_if_odd=pad)))
        if not want:
            continue
        mean = total / (limit * batches[0].shape[0])
        for stem, lo, hi in p.files:
            expect[stem] = mean if lo is None else mean[lo:hi]
            tols[stem] = tol
    return files, buf.getvalue().splitlines(), expect, tols, dtypes


def _check_files(files, expect, tols):
    assert sorted(files) == sorted(expect)
    for k, v in files.items():
        ref = expect[k]
        assert v.dtype == np.float32 and v.shape == ref.shape, k
        assert np.all(v[ref == 0] == 0), k
        # every map is within tol of its float64 energy; energies are >= 0, so their batch mean is as well. The fp32 batch
        # sum and running mean add their own roundings on top: one per accumulated sample (8 at most here) and three per
        # update, 2^-24 each - 16 * 2^-24 covers them
        nz = ref > 0
        err = np.abs(v.astype(np.float64) - ref)[nz] / ref[nz]
        assert err.size == 0 or err.max() <= tols[k] + 16 * 2.0 ** -24, (k, err.max(), tols[k])


NETS = [("vgg_16_bn", 4, 32, False), ("resnet_56", 2, 32, False), ("resnet_110", 1, 32, False),
        ("densenet_40", 2, 32, False), ("googlenet", 2, 32, False), ("resnet_50", 2, 224, False),
        ("u2netp", 2, 288, True)]


@pytest.mark.parametrize("name,bs,size,as_dict", NETS)
def test_imp_score_autocast_scores_its_own_activations(name, bs, size, as_dict, tmp_path):
    dt = "bf16" if name in ("resnet_110", "googlenet") else "fp16"
    kw = {"single_sweep": True} if name in ("u2netp", "resnet_110") else {}
    files, lines, expect, tols, dtypes = _capture_run(name, tmp_path / dt, bs, 1, size, as_dict, autocast=dt, **kw)
    assert harness.AUTOCAST[dt] in dtypes, dtypes  # (U2-Net-p's first input hook sees the fp32 image)
    _check_files(files, expect, tols)
    base, base_lines, _, _, base_dtypes = _capture_run(name, tmp_path / "fp32", bs, 1, size, as_dict, want=False, **kw)
    assert base_dtypes == {torch.float32}
    assert sorted(files) == sorted(base) and lines == base_lines
    assert lines[-1] == "The importance score generation has been completed!"


class _Pinned(torch.nn.Module):
    """The harness nets run MIOpen convolutions that are not bit-reproducible between sweeps. This one pins the
    activations: a fixed half-precision tensor per hooked module, whatever the input."""

    def __init__(self, dtype):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.relu1, self.relu2, self.relu3 = torch.nn.ReLU(), torch.nn.ReLU(), torch.nn.ReLU()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.acts = [torch.relu(torch.randn(4, c, e, e, generator=g)).to(dtype) for c, e in ((24, 32), (40, 16), (70, 8))]

    def forward(self, x):
        for m, a in zip((self.relu1, self.relu2, self.relu3), self.acts):
            m(a.to(x.device))
        return x


@pytest.mark.parametrize("dt", list(DTYPES))
def test_modes_agree_on_pinned_activations(dt, tmp_path, monkeypatch):
    from dct_pruning_amd.schedules import HookPoint
    dtype = DTYPES[dt]
    net = _Pinned(dtype).cuda()
    pts = [HookPoint("relu%d" % (i + 1), "full", [("imp_pin%d" % i, None, None)], a.shape[1], a.shape[2], a.shape[3])
           for i, a in enumerate(net.acts)]
    monkeypatch.setitem(schedules.SCHEDULES, "vgg_16_bn", lambda: pts)
    runs = {}
    for mode, kw in [("per_hook", {}), ("single", {"single_sweep": True}),
                     ("device", {"single_sweep": True, "accumulate": "device"}), ("per_hook_device", {"accumulate": "device"})]:
        files, lines, expect, tols, dtypes = _capture_run("vgg_16_bn", tmp_path / mode, 4, 2, 32, False, net=net,
                                                          autocast=dt, **kw)
        assert dtypes == {dtype}
        _check_files(files, expect, tols)
        runs[mode] = (files, lines)
    base, base_lines = runs["per_hook"]
    for mode, (files, lines) in runs.items():
        assert lines == base_lines and sorted(files) == sorted(base), mode
        for k in base:
            np.testing.assert_allclose(files[k], base[k], rtol=1e-4, atol=0, err_msg="%s %s" % (mode, k))


def test_cli_autocast_fp16(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.join(ROOT, "importance_generation.py"),
                        "--net", "vgg_16_bn", "--dataset", "cifar10", "--synthetic", "--pretrain_dir", "", "--batch_size", "16",
                        "--limit", "1", "--autocast", "fp16"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert "The importance score generation has been completed!" in p.stdout
    d = tmp_path / "importance_score" / "vgg_16_bn_limit1"
    assert sorted(os.listdir(d)) == sorted("imp_conv%d.npy" % i for i in range(1, 13))
    for p_, i in zip(schedules.vgg_16_bn(), range(1, 13)):
        a = np.load(d / ("imp_conv%d.npy" % i))
        assert a.dtype == np.float32 and a.shape == (p_.C,) and np.isfinite(a).all() and (a >= 0).all() and a.max() > 0
