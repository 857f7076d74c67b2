"""fp16 / bf16 inputs without a GPU: the three entry points are declared, bound and exported, the validation paths that
never launch return the documented codes, and imp_score(autocast=...) hands half-precision tensors to the scoring
function (swapped for the CPU oracle), writes the files of the fp32 run and scores that run's own activations.
The kernels themselves: tests/test_half_gpu.py."""
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

from dct_pruning_amd import _lib, harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

NAMES = ("dcts_energy_typed", "dcts_typed_workspace_bytes", "dcts_has_half_kernel")
NATIVE_EDGES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
F32, F16, BF16 = 0, 1, 2


def test_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert re.search(r"DCTS_DTYPE_F32\s*=\s*0\s*,\s*DCTS_DTYPE_F16\s*=\s*1\s*,\s*DCTS_DTYPE_BF16\s*=\s*2", code)
    assert "#define DCTS_ABI_VERSION 3" in text
    assert _lib.load().dcts_version() == 3


def test_has_half_kernel_names_the_nine_edges():
    lib = _lib.load()
    native = [n for n in range(1, 80) if lib.dcts_has_half_kernel(n, n)]
    assert native == list(NATIVE_EDGES)
    assert lib.dcts_has_half_kernel(57, 57) == 0 and lib.dcts_has_half_kernel(8, 16) == 0
    assert lib.dcts_has_half_kernel(72, 72) == 0
    import dct_pruning_amd as dpa
    assert dpa.has_half_kernel(28, 28) is True and dpa.has_half_kernel(28, 14) is False
    assert "has_half_kernel" in dpa.__all__


def test_typed_workspace_query():
    lib = _lib.load()
    for dt in (F16, BF16):
        for n in NATIVE_EDGES:
            assert lib.dcts_typed_workspace_bytes(dt, 4, 16, n, n) == 0, n
        small = lib.dcts_typed_workspace_bytes(dt, 1, 2, 72, 72)
        assert small >= lib.dcts_workspace_bytes(1, 2, 72, 72) + 2 * 72 * 72 * 4
        # the staging part is capped (64 MiB of upcast maps): a large call is chunked, not given a larger workspace
        big = lib.dcts_typed_workspace_bytes(dt, 64, 64, 288, 288)
        assert big - lib.dcts_workspace_bytes(64, 64, 288, 288) <= (64 << 20) + 512
        # a native edge whose call the kernel does not take (pitched rows, the odd pad) is sized as (H, W + 1)
        assert lib.dcts_typed_workspace_bytes(dt, 2, 3, 7, 8) >= 6 * 7 * 8 * 4
        assert lib.dcts_typed_workspace_bytes(dt, 0, 1, 72, 72) == 0
    assert lib.dcts_typed_workspace_bytes(F32, 4, 4, 72, 72) == lib.dcts_workspace_bytes(4, 4, 72, 72)
    assert lib.dcts_typed_workspace_bytes(7, 4, 4, 72, 72) == 0


def test_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def typed(dt, x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, out=fake, ws=None, wsb=0):
        return lib.dcts_energy_typed(x, dt, n, c, h, w, sn, sc, sh, sw, cb, cc, 0, out, ws, wsb, None)

    def f32(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, out=fake):
        return lib.dcts_energy_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, 0, out, None, 0, None)

    assert typed(F16, x=0x1001) == -7 and typed(BF16, x=0x1001) == -7
    assert typed(F16, out=0x1002) == -7
    assert typed(7) == -6 and typed(3) == -6 and typed(-1) == -6
    # dtype 0 is dcts_energy_f32: the same codes for the same bad arguments (0x1002 is 2-byte aligned only)
    for kw in ({"sw": 2}, {"sh": 4}, {"x": None}, {"out": None}, {"h": 0}, {"cb": 2, "cc": 3}, {"cc": 0}, {"x": 0x1002},
               {"h": 513, "w": 513, "sh": 513}):
        assert typed(F32, **kw) == f32(**kw) != 0, kw
    # the half dtypes check in the same order
    for dt in (F16, BF16):
        assert typed(dt, x=None) == -1 and typed(dt, out=None) == -1
        assert typed(dt, h=0) == -2 and typed(dt, h=513, w=513, sh=513) == -2
        assert typed(dt, cb=2, cc=3) == -3 and typed(dt, cc=0) == -3
        assert typed(dt, sw=2) == -4 and typed(dt, sh=4) == -4
        # a shape without a native kernel needs the workspace: missing, too small, misaligned
        assert typed(dt, h=72, w=72, sh=72, sc=72 * 72, sn=4 * 72 * 72) == -5
        assert typed(dt, h=72, w=72, sh=72, sc=72 * 72, sn=4 * 72 * 72, ws=0x2000, wsb=64) == -5
        assert typed(dt, h=72, w=72, sh=72, sc=72 * 72, sn=4 * 72 * 72, ws=0x2004, wsb=1 << 30) == -7
        # rows with a pitch at a native edge are staged, so they need one too
        assert typed(dt, sh=12, sc=96, sn=384) == -5
    for code in (-5, -6, -7):
        assert lib.dcts_strerror(code)
    assert b"dtype" in lib.dcts_strerror(-6)


def test_ops_reject_what_they_should():
    import dct_pruning_amd as dpa
    with pytest.raises(TypeError):
        dpa.energy_nc(torch.zeros(1, 1, 8, 8, dtype=torch.float64))
    with pytest.raises(TypeError):
        dpa.energy_nc(torch.zeros(1, 1, 8, 8, dtype=torch.int16))
    x = torch.zeros(1, 1, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        dpa.energy_nc(x)  # no CPU fallback, whatever the dtype
    for fn in (dpa.dct2d, dpa.rank_nc):  # the other entry points stay fp32-only
        with pytest.raises(TypeError):
            fn(x)
    with pytest.raises(TypeError):
        dpa.energy_multi([(x, 0, None)])


# ---------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------
def run_autocast(name, root, seen=None, **kw):
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name))
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
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
    """The swap point of the harness tests, recording what the hooks hand over: [(dtype, energies)] in call order."""
    calls = []

    def energy(x, c_begin=0, c_count=None, pad_front_if_odd=False):
        e = orc.energy_nc_batched(x.detach().float(), c_begin, c_count, pad_front_if_odd)
        calls.append((x.dtype, e))
        return e

    monkeypatch.setattr(harness, "_energy_nc", energy)
    return calls


@pytest.mark.parametrize("name", ["resnet_56", "densenet_40"])
def test_autocast_bf16_scores_the_half_tensors_it_is_given(name, tmp_path, oracle_ops):
    files, lines = run_autocast(name, tmp_path / "bf16", autocast="bf16")
    half_calls = list(oracle_ops)
    del oracle_ops[:]
    base, base_lines = run_autocast(name, tmp_path / "fp32")
    assert sorted(files) == sorted(base) and lines == base_lines
    assert half_calls and all(dt == torch.bfloat16 for dt, _ in half_calls)  # conv / relu outputs under autocast
    assert all(dt == torch.float32 for dt, _ in oracle_ops)
    # limit = 1: the score of a hook point is the batch mean of the one call made for it, in schedule order
    pts = harness._schedule_for(nets.get_network(name), name)
    assert len(half_calls) == len(pts)
    for p, (_, e) in zip(pts, half_calls):
        want = (e.sum(0) / e.shape[0]).numpy()
        for stem, lo, hi in p.files:
            got = files[stem]
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, want if lo is None else want[lo:hi], rtol=1e-6, atol=0, err_msg=stem)
    # one sweep for all hook points: the same tensors, the same scores
    del oracle_ops[:]
    single, lines_s = run_autocast(name, tmp_path / "single", autocast="bf16", single_sweep=True)
    assert lines_s == lines and sorted(single) == sorted(files)
    assert len(oracle_ops) == len(pts) and all(dt == torch.bfloat16 for dt, _ in oracle_ops)
    for k in files:
        np.testing.assert_allclose(single[k], files[k], rtol=1e-6, atol=0, err_msg=k)
    # the autocast forward pass is another forward pass: close to the fp32 one, not equal to it
    k = sorted(files)[0]
    assert not np.array_equal(files[k], base[k])
    np.testing.assert_allclose(files[k], base[k], rtol=0.2, atol=1e-3 * float(np.abs(base[k]).max()))


def test_autocast_rejections_before_any_sweep(tmp_path, oracle_ops):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in [{"deferred": True}, {"criterion": "rank"}, {"criterion": "bands"}, {"autocast": "fp8"}]:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            kw.setdefault("autocast", "fp16")
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


def test_cli_autocast_flag():
    import importance_generation as ig
    assert ig.parse_args(["--net", "resnet_56"]).autocast is None
    assert ig.parse_args(["--net", "resnet_56", "--autocast", "bf16", "--single_sweep"]).autocast == "bf16"
    for extra in (["--deferred"], ["--criterion", "rank"], ["--criterion", "bands"], ["--autocast", "fp8"]):
        with pytest.raises(SystemExit) as e:
            ig.main(["--net", "resnet_56", "--synthetic", "--autocast", "fp16"] + extra)  # exits in the parser
        assert e.value.code == 2
    assert "--autocast" in ig.__doc__
