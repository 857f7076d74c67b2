"""channels_last inputs without a GPU: the three entry points are declared, bound and exported, the validation paths that
never launch return the documented codes, energy_nc's route is a pure stride computation, and imp_score(channels_last=True)
hands channels-last tensors to the scoring function (swapped for the CPU oracle) and writes the files of the plain run.
The kernels themselves: tests/test_nhwc_gpu.py."""
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

from dct_pruning_amd import _lib, harness, nets, ops
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

NAMES = ("dcts_energy_nhwc", "dcts_nhwc_workspace_bytes", "dcts_has_nhwc_kernel")
NATIVE_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
F32, F16, BF16 = 0, 1, 2
_i64, _i32, _vp, _sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t


def test_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    # the documented signatures
    assert _lib.SIGNATURES["dcts_has_nhwc_kernel"] == (ctypes.c_int, [_i64, _i64])
    assert _lib.SIGNATURES["dcts_nhwc_workspace_bytes"] == (_sz, [_i32, _i64, _i64, _i64, _i64])
    assert _lib.SIGNATURES["dcts_energy_nhwc"] == (
        ctypes.c_int, [_vp, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _sz, _vp])
    proto = re.search(r"int\s+dcts_energy_nhwc\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == [
        "x", "dtype", "N", "C_total", "H", "W", "strideN", "strideH", "strideW", "c_begin", "c_count", "out_nc",
        "workspace", "workspace_bytes", "stream"]
    assert "#define DCTS_ABI_VERSION 3" in text
    assert _lib.load().dcts_version() == 3


def test_has_nhwc_kernel_names_the_documented_edges():
    lib = _lib.load()
    native = [n for n in range(0, 80) if lib.dcts_has_nhwc_kernel(n, n)]
    assert native == list(NATIVE_EDGES)
    assert lib.dcts_has_nhwc_kernel(8, 16) == 0 and lib.dcts_has_nhwc_kernel(56, 28) == 0
    assert lib.dcts_has_nhwc_kernel(72, 72) == 0 and lib.dcts_has_nhwc_kernel(0, 0) == 0
    import dct_pruning_amd as dpa
    assert dpa.has_nhwc_kernel(28, 28) is True and dpa.has_nhwc_kernel(28, 14) is False
    assert "has_nhwc_kernel" in dpa.__all__
    for dt in (F32, F16, BF16):
        for n in NATIVE_EDGES:
            assert lib.dcts_nhwc_workspace_bytes(dt, 4, 16, n, n) == 0


def test_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def nhwc(dt, x=fake, n=1, c=4, h=8, w=8, sn=256, sh=32, sw=4, cb=0, cc=4, out=fake):
        return lib.dcts_energy_nhwc(x, dt, n, c, h, w, sn, sh, sw, cb, cc, out, None, 0, None)

    for dt in (F32, F16, BF16):
        assert nhwc(dt, x=None) == -1 and nhwc(dt, out=None) == -1
        assert nhwc(dt, h=0) == -2 and nhwc(dt, n=0) == -2
        assert nhwc(dt, cb=2, cc=3) == -3 and nhwc(dt, cc=0) == -3 and nhwc(dt, cb=-1) == -3
        assert nhwc(dt, sw=3) == -4            # strideW < C_total
        assert nhwc(dt, sh=31) == -4           # strideH < W * strideW
        assert nhwc(dt, sw=1, sh=8) == -4      # an NCHW tensor is not this entry point's
        assert nhwc(dt, out=0x1002) == -7
        # a shape without a native kernel: the copy stays with the caller
        assert nhwc(dt, h=72, w=72, sh=288, sn=72 * 288) == -6
        assert nhwc(dt, h=56, w=28, sh=112, sn=56 * 112) == -6
        assert nhwc(dt, h=8, w=16, sh=64, sn=512) == -6
    assert nhwc(F16, x=0x1001) == -7 and nhwc(BF16, x=0x1001) == -7     # an odd byte address for half
    assert nhwc(F32, x=0x1002) == -7
    assert nhwc(7) == -6 and nhwc(3) == -6 and nhwc(-1) == -6           # an unknown dtype
    # the existing entry points are untouched: strideW != 1 stays a stride error there
    assert lib.dcts_energy_f32(fake, 1, 4, 8, 8, 256, 1, 32, 4, 0, 4, 0, fake, None, 0, None) == -4
    assert lib.dcts_energy_typed(fake, F16, 1, 4, 8, 8, 256, 1, 32, 4, 0, 4, 0, fake, None, 0, None) == -4


def test_route_is_a_pure_stride_computation():
    has = lambda H, W: H == W and H in NATIVE_EDGES  # noqa: E731

    def route(x, **kw):
        return ops.energy_route(x.shape, x.stride(), has_kernel=has, **kw)

    x = torch.zeros(3, 10, 8, 8)
    assert route(x) == ops.ROUTE_NCHW
    assert route(torch.zeros(3, 10, 8, 12)[..., :8]) == ops.ROUTE_NCHW          # pitched rows
    assert route(x.transpose(2, 3)) == ops.ROUTE_COPY
    assert route(torch.zeros(3, 1, 8, 8).contiguous(memory_format=torch.channels_last)) == ops.ROUTE_NCHW  # C == 1
    cl = x.contiguous(memory_format=torch.channels_last)
    assert cl.stride() == (640, 1, 80, 10)
    assert route(cl) == ops.ROUTE_NHWC
    assert route(cl[:, 3:8]) == ops.ROUTE_NHWC and route(cl[::2]) == ops.ROUTE_NHWC
    assert route(cl.half()) == ops.ROUTE_NHWC
    # what keeps a channels_last tensor on the copy route
    assert route(cl, algo=ops.ALGO_CODELET) == ops.ROUTE_COPY
    assert route(torch.zeros(2, 4, 7, 7).contiguous(memory_format=torch.channels_last), pad_front_if_odd=True) == ops.ROUTE_COPY
    assert route(torch.zeros(2, 4, 7, 7).contiguous(memory_format=torch.channels_last)) == ops.ROUTE_NHWC
    assert route(torch.zeros(2, 4, 8, 8).contiguous(memory_format=torch.channels_last), pad_front_if_odd=True) == ops.ROUTE_NHWC
    for h, w in ((72, 72), (9, 9), (56, 28)):
        assert route(torch.zeros(1, 4, h, w).contiguous(memory_format=torch.channels_last)) == ops.ROUTE_COPY
    # a transposed channels_last tensor: strideH < W * strideW
    assert route(x.permute(0, 1, 3, 2).contiguous(memory_format=torch.channels_last).permute(0, 1, 3, 2)) == ops.ROUTE_COPY
    # the default predicate is the built library's
    assert ops.energy_route(cl.shape, cl.stride()) == ops.ROUTE_NHWC


# ---------------------------------------------------------------------------------------------------------
# harness and CLI
# ---------------------------------------------------------------------------------------------------------
def run_harness(name, root, double=True, **kw):
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name))
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    if double:
        net, loader = net.double(), [(data.double(), target) for data, target in loader]
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
    d = os.path.join(str(root), "importance_score", "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return files, buf.getvalue().splitlines()


@pytest.fixture
def oracle_ops(monkeypatch):
    """The swap point of the harness tests, recording what the hooks hand over: [(is channels_last, dtype, energies)]."""
    calls = []

    def energy(x, c_begin=0, c_count=None, pad_front_if_odd=False):
        e = orc.energy_nc_batched(x.detach().float().contiguous(), c_begin, c_count, pad_front_if_odd)
        nhwc = x.shape[1] > 1 and x.stride(1) == 1 and x.stride(3) >= x.shape[1]
        calls.append((bool(nhwc), x.dtype, e))
        return e

    monkeypatch.setattr(harness, "_energy_nc", energy)
    return calls


@pytest.mark.parametrize("name", ["resnet_56", "vgg_16_bn"])
def test_channels_last_hands_on_channels_last_tensors(name, tmp_path, oracle_ops):
    # The forward passes run in float64 (the scoring call rounds what it is given to fp32). In fp32 the CPU's channels-last
    # and NCHW convolutions add in different orders, and 12 / 55 layers of random-init weights amplify that to 1.5e-4 ... 3.4e-4
    # in single channels of the deepest layers (imp_conv11 of vgg_16_bn, imp_conv48 / imp_conv50 of resnet_56; with
    # oneDNN switched off as well): a difference between two forward passes, which is not what is compared here.
    files, lines = run_harness(name, tmp_path / "cl", channels_last=True)
    cl_calls = list(oracle_ops)
    del oracle_ops[:]
    base, base_lines = run_harness(name, tmp_path / "plain")
    assert sorted(files) == sorted(base) and lines == base_lines
    # on the CPU convolutions, batch norm and ReLU keep the memory format
    assert cl_calls and all(nhwc and dt == torch.float64 for nhwc, dt, _ in cl_calls)
    assert oracle_ops and not any(nhwc for nhwc, _, _ in oracle_ops)
    for k in base:
        np.testing.assert_allclose(files[k], base[k], rtol=1e-4, atol=0, err_msg=k)
    # one sweep for all hook points: the same tensors, the same scores
    del oracle_ops[:]
    single, lines_s = run_harness(name, tmp_path / "single", channels_last=True, single_sweep=True)
    assert lines_s == lines and sorted(single) == sorted(files)
    assert all(nhwc for nhwc, _, _ in oracle_ops)
    for k in files:
        np.testing.assert_allclose(single[k], files[k], rtol=1e-4, atol=0, err_msg=k)


@pytest.mark.parametrize("name", ["resnet_56", "vgg_16_bn"])
def test_channels_last_fp32_run_hands_on_channels_last_tensors(name, tmp_path, oracle_ops):
    """The fp32 forward pass users run: layout, dtype and file set (the values are compared in float64 above)."""
    files, lines = run_harness(name, tmp_path / "cl", double=False, channels_last=True)
    assert oracle_ops and all(nhwc and dt == torch.float32 for nhwc, dt, _ in oracle_ops)
    del oracle_ops[:]
    base, base_lines = run_harness(name, tmp_path / "plain", double=False)
    assert oracle_ops and not any(nhwc for nhwc, _, _ in oracle_ops)
    assert sorted(files) == sorted(base) and lines == base_lines
    for k in base:
        assert files[k].dtype == np.float32 and files[k].shape == base[k].shape and np.isfinite(files[k]).all(), k


def test_channels_last_rejections_before_any_sweep(tmp_path, oracle_ops):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for net, kw in [("resnet_56", {"deferred": True}), ("resnet_56", {"criterion": "rank"}),
                        ("resnet_56", {"criterion": "bands"}), ("u2netp", {})]:
            args = types.SimpleNamespace(net=net, limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), channels_last=True, **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


def test_cli_channels_last_flag():
    import importance_generation as ig
    assert ig.parse_args(["--net", "resnet_56"]).channels_last is False
    assert ig.parse_args(["--net", "resnet_56", "--channels_last", "--single_sweep"]).channels_last is True
    assert ig.parse_args(["--net", "resnet_56", "--channels_last", "--autocast", "bf16"]).autocast == "bf16"
    for extra in (["--deferred"], ["--criterion", "rank"], ["--criterion", "bands"], ["--net", "u2netp"]):
        with pytest.raises(SystemExit) as e:
            ig.main(["--net", "resnet_56", "--synthetic", "--channels_last"] + extra)  # exits in the parser
        assert e.value.code == 2
    assert "--channels_last" in ig.__doc__
