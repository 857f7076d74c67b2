"""The band criterion's host side without a GPU: the C ABI entry points (declared, bound, exported, argument codes), the
partitions of dct_pruning_amd.bands, imp_score(criterion="bands") with the CPU oracle (tests/band_oracle.py) in place of
the kernel, the collapse step, the mask tool on band spectra, the CLI's parse errors and a world-2 gloo run."""
import contextlib
import ctypes
import io
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import band_oracle as bo
from dct_pruning_amd import _lib, bands, harness, masks, nets, sharding
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

NEW = ("dcts_band_workspace_bytes", "dcts_has_band_kernel", "dcts_band_energy_f32")


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_band_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_BAND_MAX 8\b", text) and bands.BAND_MAX == 8
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    assert "without a bump" in text.lower()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    # the prototype's argument count is the binding's
    proto = re.search(r"int dcts_band_energy_f32\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["dcts_band_energy_f32"][1]) == 19
    proto = re.search(r"size_t dcts_band_workspace_bytes\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["dcts_band_workspace_bytes"][1]) == 5
    assert _lib.load().dcts_version() == 3


def test_has_band_kernel_is_the_codelet_table():
    lib = _lib.load()
    for e in range(1, 80):
        assert lib.dcts_has_band_kernel(e, e) == lib.dcts_has_codelet(e, e), e
    assert lib.dcts_has_band_kernel(7, 7) == 1 and lib.dcts_has_band_kernel(9, 9) == 1
    assert lib.dcts_has_band_kernel(56, 28) == 0 and lib.dcts_has_band_kernel(72, 72) == 0


def test_band_workspace_query():
    lib = _lib.load()
    q = lib.dcts_band_workspace_bytes
    assert q(4, 16, 56, 56, 0) == 0 and q(4, 16, 56, 56, 9) == 0 and q(0, 16, 56, 56, 4) == 0 and q(1, 1, 513, 8, 1) == 0
    for (n, c, h, w) in [(1, 1, 2, 2), (4, 16, 56, 56), (2, 3, 64, 64), (1, 2, 288, 288), (2, 3, 56, 28), (1, 1, 512, 512)]:
        for k in (1, 3, 8):
            b = q(n, c, h, w, k)
            assert b % 256 == 0
            assert b >= 8 * (h + 1) * (w + 1) * 4 if k == 8 else b > 0  # the re-laid weight table fits
            assert b >= 2 * (h + 1) * (w + 1) * 4                       # and one map of the fallback's two halves


def test_band_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, pad=0, wt=fake, k=4, out=fake, ws=fake,
             wsb=1 << 20, algo=0):
        return lib.dcts_band_energy_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, pad, wt, k, out, ws, wsb, None, algo)

    assert call(x=None) == -1 and call(out=None) == -1 and call(wt=None) == -1
    assert call(n=0) == -2 and call(h=0) == -2 and call(w=-1) == -2 and call(h=513, w=513, sh=513) == -2
    assert call(k=0) == -2 and call(k=9) == -2 and call(k=-1) == -2
    assert call(cb=2, cc=3) == -3 and call(cc=0) == -3 and call(cb=-1) == -3
    assert call(sw=2) == -4 and call(sh=4) == -4
    assert call(x=0x1001) == -7 and call(out=0x1002) == -7 and call(wt=0x1002) == -7
    assert call(ws=None) == -5 and call(ws=0x1004) == -7
    assert call(wsb=16) == -5                      # fused kernel: the weight table does not fit
    assert call(wsb=16, algo=1) == -5              # fallback: not even one map
    assert call(h=56, w=28, sh=28, algo=2) == -6   # no fused kernel for a non-square map
    assert call(sh=12, algo=2) == -6               # nor for row-pitched maps
    assert call(algo=3) == -6 and call(algo=9) == -6


# ---------------------------------------------------------------------------------------------------------
# partitions
# ---------------------------------------------------------------------------------------------------------
def _band_of(u, v, H, W, K, kind):
    """The issue's formulas, in plain Python integers."""
    if kind == "square":
        return max(u * K // H, v * K // W)
    return (u * W + v * H) * K // (2 * H * W)


@pytest.mark.parametrize("kind", ["square", "diag"])
@pytest.mark.parametrize("H,W", [(8, 8), (7, 7), (9, 9), (10, 10), (56, 56), (56, 28), (13, 64), (33, 17), (1, 1), (2, 5)])
def test_partition(H, W, kind):
    for K in range(1, 9):
        w = bands.partition(H, W, K, kind)
        assert w.dtype == np.float32 and w.shape == (K, H, W)
        assert set(np.unique(w)) <= {0.0, 1.0}
        np.testing.assert_array_equal(w.sum(0), np.ones((H, W), np.float32))  # every cell in exactly one band
        assert w[0, 0, 0] == 1.0                                              # band 0 holds DC
        for u in range(H):
            for v in range(W):
                assert w[_band_of(u, v, H, W, K, kind), u, v] == 1.0, (u, v)
        if K <= min(H, W):
            assert (w.reshape(K, -1).sum(1) > 0).all(), "empty band at K = %d" % K
    with pytest.raises(ValueError):
        bands.partition(H, W, 9, kind)
    with pytest.raises(ValueError):
        bands.partition(H, W, 0, kind)


def test_partition_rejects_unknown_kind():
    with pytest.raises(ValueError):
        bands.partition(8, 8, 4, "ring")


# ---------------------------------------------------------------------------------------------------------
# the oracle is the definition
# ---------------------------------------------------------------------------------------------------------
def test_band_oracle_is_the_weighted_oracle_stacked():
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(2, 6, 9, 9, generator=g))
    w = torch.rand(3, 10, 10, generator=g)
    f64 = bo.band_energy_nc_f64(x, w, 1, 4, True)
    assert f64.shape == (2, 4, 3)
    for b in range(3):
        np.testing.assert_array_equal(f64[..., b], orc.weighted_energy_nc_f64(x, w[b].numpy(), 1, 4, True))
    f32 = bo.band_energy_nc(x, w, 1, 4, True)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (2, 4, 3)
    assert bo.band_error(f32, x, w, 1, 4, True) < 1e-6
    # one-hot bands add up to the plain energy (Parseval)
    p = bands.partition(9, 9, 4, "square")
    np.testing.assert_allclose(bo.band_energy_nc_f64(x, p).sum(-1), bo.map_energy_f64(x), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------
def run_bands(name, root, cfg=(4, "square"), criterion="bands", **kw):
    """imp_score on the CPU net with the harness-test inputs; returns (files, stdout lines, directory)."""
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
            if criterion == "bands":
                harness.imp_score(net, args, train_loader=loader, criterion="bands", bands=cfg, **kw)
            else:
                harness.imp_score(net, args, train_loader=loader, **kw)
    finally:
        os.chdir(cwd)
    if criterion == "bands":
        d = os.path.join(str(root), "band_score", "%s_limit%d_%s%d" % (name, limit, cfg[1], cfg[0]))
    else:
        d = os.path.join(str(root), "importance_score", "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return files, buf.getvalue().splitlines(), d


@pytest.fixture
def oracle_ops(monkeypatch):
    monkeypatch.setattr(harness, "_band_energy_nc", bo.band_energy_nc)
    monkeypatch.setattr(harness, "_energy_nc", orc.energy_nc_batched)


@pytest.mark.parametrize("name,cfg", [("densenet_40", (4, "square")), ("googlenet", (3, "diag"))])
def test_per_hook_equals_single_sweep_and_sums_to_the_dct_files(name, cfg, tmp_path, oracle_ops):
    per_hook, lines, d = run_bands(name, tmp_path / "per_hook", cfg)
    single, lines_s, _ = run_bands(name, tmp_path / "single", cfg, single_sweep=True)
    dct, lines_d, _ = run_bands(name, tmp_path / "dct", criterion="dct")
    assert sorted(per_hook) == sorted(single) == sorted("band_" + s[4:] for s in dct)
    assert lines == lines_s == [ln.replace("./importance_score/%s_limit%d" % (name, HARNESS_CASES[name][1]),
                                           "./band_score/%s_limit%d_%s%d" % (name, HARNESS_CASES[name][1], cfg[1], cfg[0]))
                                for ln in lines_d]
    for k, spec in per_hook.items():
        ref = dct["imp_" + k[5:]]
        assert spec.dtype == np.float32 and spec.shape == (ref.shape[0], cfg[0]), k
        assert spec.tobytes() == single[k].tobytes(), k
        np.testing.assert_allclose(spec.astype(np.float64).sum(1), ref, rtol=2e-5, atol=0, err_msg=k)
        assert (spec >= 0).all()
    # on-disk format: NumPy v1.0 header, '<f4', C order, data at byte 128
    f = os.path.join(d, sorted(os.listdir(d))[0])
    raw = open(f, "rb").read()
    assert raw[:8] == b"\x93NUMPY\x01\x00" and b"'descr': '<f4'" in raw[:128] and b"'fortran_order': False" in raw[:128]
    assert len(raw) == 128 + 4 * np.load(f).size
    assert not (tmp_path / "per_hook" / "importance_score").exists()


def test_u2netp_single_sweep_with_the_odd_pad(tmp_path, oracle_ops):
    cfg = (4, "square")
    spec, _, _ = run_bands("u2netp", tmp_path / "bands", cfg, single_sweep=True)
    dct, _, _ = run_bands("u2netp", tmp_path / "dct", criterion="dct", single_sweep=True)
    assert len(spec) == len(dct) == 118
    for k, v in spec.items():
        assert k.startswith("band_net."), k
        ref = dct[k[5:]]  # U2-Net-p's score files are net.<module path>.npy
        assert v.shape == (ref.shape[0], 4), k
        np.testing.assert_allclose(v.astype(np.float64).sum(1), ref, rtol=2e-5, atol=0, err_msg=k)
    assert bands.score_file_name("band_net.stage1.rebnconv1.relu_s1.npy") == "net.stage1.rebnconv1.relu_s1.npy"
    assert bands.score_file_name("band_conv3.npy") == "imp_conv3.npy"


def test_band_hooks_have_reference_signature(oracle_ops, monkeypatch):
    monkeypatch.setattr(harness, "_band_cfg", (3, "diag"))
    m = torch.nn.ReLU()
    x = torch.relu(torch.randn(2, 24, 9, 9))
    for hook, cb, cc, pad, src in [(harness.get_feature_hook_bands, 0, 24, False, "out"),
                                   (harness.get_feature_hook_densenet_bands, 12, 12, True, "out"),
                                   (harness.get_feature_hook_u2net_input_bands, 0, 24, True, "in")]:
        harness._acc.reset()
        h = m.register_forward_hook(hook)
        m(x)
        h.remove()
        e = 10 if pad else 9
        w = bands.partition(e, e, 3, "diag")
        want = bo.band_energy_nc(x, w, cb, cc, pad).sum(0)  # x is non-negative: relu(x) == x, input == output
        got = harness._acc.feature_result.numpy().reshape(-1, 3)
        assert got.shape == (cc, 3) and harness._acc.total.item() == 2
        np.testing.assert_allclose(got, want.numpy() / 2, rtol=1e-6)
    harness._acc.reset()


def test_bands_rejections_before_any_sweep(tmp_path, oracle_ops):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in [{"deferred": True}, {"bands": (9, "square")}, {"bands": (0, "square")}, {"bands": (4, "ring")}]:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), criterion="bands", **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []
    assert "bands" in harness.CRITERIA


def test_cli_bands_flags():
    import importance_generation as ig
    a = ig.parse_args(["--net", "resnet_56", "--criterion", "bands"])
    assert (a.criterion, a.bands, a.band_kind) == ("bands", 4, "square")
    a = ig.parse_args(["--net", "u2netp", "--criterion", "bands", "--bands", "8", "--band_kind", "diag", "--single_sweep"])
    assert (a.bands, a.band_kind) == (8, "diag")
    for extra in (["--deferred"], ["--bands", "9"], ["--bands", "0"], ["--band_kind", "ring"]):
        with pytest.raises(SystemExit) as e:
            ig.main(["--net", "resnet_56", "--criterion", "bands", "--synthetic"] + extra)  # exits in the parser
        assert e.value.code == 2
    assert ig.parse_args(["--net", "resnet_56"]).criterion == "dct"
    assert "--bands" in ig.__doc__


def _worker(rank, world, port, name, out_root, cfg, kw):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sharding.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    torch.set_num_threads(2)  # as the single-process run
    from dct_pruning_amd import harness as h
    import band_oracle
    from test_bands_cpu import run_bands as rb
    h._band_energy_nc = band_oracle.band_energy_nc
    d = os.path.join(out_root, "rank%d" % rank)
    os.makedirs(d)
    rb(name, d, cfg, **kw)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name,kw", [("densenet_40", {}), ("vgg_16_bn", {"single_sweep": True})])
def test_two_rank_gloo_equals_single_process(name, kw, tmp_path, oracle_ops):
    cfg = (4, "square")
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        single, _, _ = run_bands(name, tmp_path / "single", cfg, **kw)
    finally:
        torch.set_num_threads(before)
    port = 37500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, name, str(tmp_path), cfg, kw), nprocs=2, join=True)
    d0 = tmp_path / "rank0" / "band_score" / ("%s_limit%d_square4" % (name, HARNESS_CASES[name][1]))
    got = {f[:-4]: np.load(d0 / f) for f in os.listdir(d0)}
    assert sorted(got) == sorted(single)
    for k in single:
        assert got[k].shape == single[k].shape and got[k].tobytes() == single[k].tobytes(), k
    assert not (tmp_path / "rank1" / "band_score").exists()


# ---------------------------------------------------------------------------------------------------------
# collapse and the mask tool
# ---------------------------------------------------------------------------------------------------------
def test_collapse_and_masks(tmp_path, oracle_ops):
    name = "densenet_40"
    spec, _, d = run_bands(name, tmp_path / "bands", single_sweep=True)
    dct, _, d_dct = run_bands(name, tmp_path / "dct", criterion="dct", single_sweep=True)
    # one-hot band weights pick a column
    out1 = str(tmp_path / "col2")
    written = bands.collapse(d, [0, 0, 1, 0], out1)
    assert sorted(written) == sorted(f + ".npy" for f in dct)
    for k, v in spec.items():
        a = np.load(os.path.join(out1, "imp_" + k[5:] + ".npy"))
        assert a.dtype == np.float32 and a.ndim == 1 and a.tobytes() == np.ascontiguousarray(v[:, 2]).tobytes(), k
        raw = open(os.path.join(out1, "imp_" + k[5:] + ".npy"), "rb").read()
        ref_raw = open(os.path.join(d_dct, "imp_" + k[5:] + ".npy"), "rb").read()
        assert raw[:128] == ref_raw[:128]  # the dct files' own header, byte for byte
    # all ones: float64 product rounded once, and the same masks as the dct run's files
    out2 = str(tmp_path / "ones")
    assert bands.main(["--spectrum", d, "--band_weights", "1,1,1,1", "--out", out2]) == 0
    for k, v in spec.items():
        a = np.load(os.path.join(out2, "imp_" + k[5:] + ".npy"))
        assert a.tobytes() == v.astype(np.float64).sum(1).astype(np.float32).tobytes(), k
    for rate in (0.3, 0.5, 0.7):
        assert masks.compare(masks.masks_for_dir(out2, rate), masks.masks_for_dir(d_dct, rate)) == []
    assert masks.main(["--imp_score", out2, "--compress_rate", "[0.5]*39", "--compare", d_dct]) == 0
    # the mask tool on the spectrum directory itself
    with pytest.raises(ValueError, match="band_weights"):
        masks.masks_for_dir(d, 0.5)
    with pytest.raises(SystemExit) as e:
        masks.main(["--imp_score", d, "--compress_rate", "[0.5]*39"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        masks.main(["--imp_score", d, "--compress_rate", "[0.5]*39", "--band_weights", "1,1"])  # K is 4
    assert e.value.code == 2
    m_spec = masks.masks_for_dir(d, 0.5, np.ones(4))
    m_dct = masks.masks_for_dir(d_dct, 0.5)
    assert sorted(m_spec) == sorted("band_" + k[4:] for k in m_dct)
    for k, v in m_dct.items():
        np.testing.assert_array_equal(m_spec["band_" + k[4:]], v)
    assert masks.main(["--imp_score", d, "--compress_rate", "[0.5]*39", "--band_weights", "1,0.5,0.25,0",
                       "--out", str(tmp_path / "m.npz")]) == 0
    # 1-D files behave exactly as before, with or without the flag
    np.testing.assert_array_equal(masks.masks_for_dir(d_dct, 0.5, np.ones(4))["imp_conv3"], m_dct["imp_conv3"])
    # CLI parse errors of the collapse tool
    for argv in (["--spectrum", d, "--out", out2], ["--spectrum", d, "--band_weights", "1,x", "--out", out2],
                 ["--spectrum", d, "--band_weights", "1,1,1", "--out", out2],
                 ["--spectrum", d_dct, "--band_weights", "1,1,1,1", "--out", out2]):
        with pytest.raises(SystemExit) as e:
            bands.main(argv)
        assert e.value.code == 2
