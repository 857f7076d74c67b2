"""The rank criterion's host side without a GPU: the C ABI entry point (declared, bound, exported, argument codes),
imp_score(criterion="rank") with the fp64 oracle in place of the kernel against HRank's hook body restated literally,
the CLI's parse errors, a world-2 gloo run and the mask tool on a rank directory."""
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

import rank_oracle as ro
from dct_pruning_amd import _lib, harness, masks, nets, schedules, sharding
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from test_harness_cpu import load_golden


def test_rank_entry_point_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_RANK_MAX_EDGE 64\b", text)
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    assert "dcts_rank_f32" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dcts_rank_f32")
    assert _lib.load().dcts_version() == 3


def test_rank_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, out=fake):
        return lib.dcts_rank_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, out, None)

    assert call(x=None) == -1 and call(out=None) == -1
    assert call(n=0) == -2 and call(h=0) == -2 and call(w=-1) == -2 and call(h=513, w=513, sh=513) == -2
    assert call(cb=2, cc=3) == -3 and call(cc=0) == -3 and call(cb=-1) == -3
    assert call(sw=2) == -4 and call(sh=4) == -4
    assert call(h=65) == -6 and call(w=100, sh=100) == -6 and call(h=512, w=512, sh=512) == -6
    assert call(x=0x1001) == -7 and call(out=0x1002) == -7
    assert b"rank: edges up to 64" in lib.dcts_strerror(-6)


def test_oracle_rule():
    """The oracle is torch.linalg.matrix_rank's fp32 rule (atol 0, rtol max(H, W) * eps) in fp64."""
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(3, 5, 9, 6, generator=g))
    x[:, 1] = 0
    x[:, 2, 4:] = 0
    want = torch.linalg.matrix_rank(x.double(), rtol=9 * 2.0 ** -23).float()
    assert torch.equal(ro.rank_nc(x), want)
    assert (ro.rank_nc(x)[:, 1] == 0).all() and (ro.rank_nc(x)[:, 2] <= 4).all()
    assert not ro.undecidable(x).any()
    assert torch.equal(ro.rank_nc(x, 1, 3), want[:, 1:4])


def run_rank(name, root, bs=None, limit=None, **kw):
    """imp_score(criterion="rank") on the CPU net with the harness-test inputs; returns (files, stdout lines)."""
    bs0, limit0, size, _ = HARNESS_CASES[name]
    bs, limit = bs or bs0, limit or limit0
    net = deterministic_init(nets.get_network(name))
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.makedirs(str(root), exist_ok=True)
    cwd = os.getcwd()
    os.chdir(str(root))
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            harness.imp_score(net, args, train_loader=loader, criterion="rank", **kw)
    finally:
        os.chdir(cwd)
    d = os.path.join(str(root), "rank_conv", "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return files, buf.getvalue().splitlines()


def hrank_expected(name):
    """HRank's hook body restated literally (rank_oracle.hrank_hook_scores) over the tensors each hook point sees,
    captured by forward hooks on a plain inference pass with the same weights and batches."""
    bs, limit, size, _ = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name))
    pts = harness._schedule_for(net, name)
    acts = {}
    handles = [harness._resolve(net, p.module).register_forward_hook(
        lambda m, i, o, _k=p.module: acts.setdefault(_k, []).append(o.detach().clone())) for p in pts]
    harness.inference(net, SyntheticLoader((3, size, size), bs, limit + 1, seed=7), limit)
    for h in handles:
        h.remove()
    out = {}
    for p in pts:
        if p.kind == "last12":
            scores = ro.hrank_hook_scores(acts[p.module], acts[p.module][0].shape[1] - 12, 12)
        else:
            scores = ro.hrank_hook_scores(acts[p.module])
        for stem, lo, hi in p.files:
            assert stem.startswith("imp_")
            out["rank_" + stem[4:]] = scores if lo is None else scores[lo:hi]
    return out


@pytest.fixture
def oracle_rank(monkeypatch):
    monkeypatch.setattr(harness, "_rank_nc", ro.rank_nc)


@pytest.mark.parametrize("name", ["resnet_56", "densenet_40", "googlenet"])
def test_imp_score_rank_equals_hrank_hook_body(name, tmp_path, oracle_rank):
    expect = hrank_expected(name)
    meta, _ = load_golden(name)
    per_hook, lines = run_rank(name, tmp_path / "per_hook")
    single, lines_s = run_rank(name, tmp_path / "single", single_sweep=True)
    # directory and stems: the DCT run's stems with imp_ -> rank_ (chart.py's rank_conv%d.npy for the ResNets)
    assert sorted(per_hook) == sorted(expect) == sorted("rank_" + s[4:] for s in meta["files"])
    # progress lines: the DCT run's, with the rank directory
    assert lines == lines_s == [ln.replace("./importance_score/", "./rank_conv/") for ln in meta["stdout"]]
    for k, v in expect.items():
        for files in (per_hook, single):
            got = files[k]
            assert got.dtype == np.float32 and got.shape == v.shape == (v.size,), k
            assert got.tobytes() == v.astype(np.float32).tobytes(), k
    assert not (tmp_path / "per_hook" / "importance_score").exists()


def test_rank_hooks_have_reference_signature(oracle_rank):
    m = torch.nn.ReLU()
    x = torch.relu(torch.randn(2, 24, 9, 9))
    harness._acc.reset()
    h = m.register_forward_hook(harness.get_feature_hook_rank)
    m(x)
    h.remove()
    np.testing.assert_array_equal(harness._acc.feature_result.numpy(), ro.hrank_hook_scores([x]))
    assert harness._acc.total.item() == 2
    harness._acc.reset()
    h = m.register_forward_hook(harness.get_feature_hook_densenet_rank)
    m(x)
    h.remove()
    np.testing.assert_array_equal(harness._acc.feature_result.numpy(), ro.hrank_hook_scores([x], 12, 12))
    harness._acc.reset()


def test_rank_rejections_before_any_sweep(tmp_path, oracle_rank):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for net_name, kw in [("resnet_56", {"deferred": True}), ("u2netp", {}), ("resnet_56", {"criterion": "hrank"})]:
            args = types.SimpleNamespace(net=net_name, limit=1)
            kw = dict({"criterion": "rank"}, **kw)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


def test_cli_criterion_flag():
    import importance_generation as ig
    assert ig.parse_args(["--net", "resnet_56"]).criterion == "dct"
    a = ig.parse_args(["--net", "resnet_56", "--criterion", "rank", "--single_sweep", "--device_accumulate"])
    assert a.criterion == "rank"
    for extra in (["--net", "u2netp"], ["--net", "resnet_56", "--deferred"]):
        with pytest.raises(SystemExit) as e:
            ig.main(extra + ["--criterion", "rank", "--synthetic"])  # exits in the parser, before any CUDA call
        assert e.value.code == 2
    assert "--criterion" in ig.__doc__


def _worker(rank, world, port, name, out_root, kw):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sharding.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    torch.set_num_threads(2)  # as the single-process run
    from dct_pruning_amd import harness as h
    import rank_oracle
    from test_rank_cpu import run_rank as rr
    h._rank_nc = rank_oracle.rank_nc
    d = os.path.join(out_root, "rank%d" % rank)
    os.makedirs(d)
    rr(name, d, **kw)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name,kw", [("resnet_56", {}), ("densenet_40", {"single_sweep": True})])
def test_two_rank_gloo_equals_single_process(name, kw, tmp_path, oracle_rank):
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        single, _ = run_rank(name, tmp_path / "single", **kw)
    finally:
        torch.set_num_threads(before)
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, name, str(tmp_path), kw), nprocs=2, join=True)
    d0 = tmp_path / "rank0" / "rank_conv" / ("%s_limit%d" % (name, HARNESS_CASES[name][1]))
    got = {f[:-4]: np.load(d0 / f) for f in os.listdir(d0)}
    assert sorted(got) == sorted(single)
    for k in single:
        assert got[k].tobytes() == single[k].tobytes(), k
    assert not (tmp_path / "rank1" / "rank_conv").exists()


def test_lpt_cost_is_the_rank_kernels_work():
    """world > 1 balances the rank kernel's O(H W min(H, W)) work, not the DCT path's bytes."""
    pts = schedules.resnet_50()
    seen = []
    orig = sharding.make_units

    def spy(chans, cost, **kw):
        seen.append(list(cost))
        return orig(chans, cost, **kw)

    old = sharding.make_units
    sharding.make_units = spy
    try:
        args = types.SimpleNamespace(net="resnet_50", limit=0)

        class Empty:
            def __iter__(self):
                return iter(())

        cwd = os.getcwd()
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            os.chdir(d)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    harness.imp_score(deterministic_init(nets.get_network("resnet_50")), args, train_loader=Empty(),
                                      criterion="rank", single_sweep=True)
            except KeyError:
                pass  # no batch ran, so there are no scores to save; the cost vector is what this test reads
            finally:
                os.chdir(cwd)
    finally:
        sharding.make_units = old
    assert seen and seen[0] == [float(p.H * p.W * min(p.H, p.W)) for p in pts]


def test_masks_on_a_rank_directory(tmp_path, oracle_rank):
    files, _ = run_rank("resnet_56", tmp_path)
    d = str(tmp_path / "rank_conv" / "resnet_56_limit1")
    names = masks.score_files(d)
    assert names == ["rank_conv%d.npy" % i for i in range(1, 56)]
    m = masks.masks_for_dir(d, 0.5)
    assert list(m) == ["rank_conv%d" % i for i in range(1, 56)]
    for k, v in m.items():
        imp = files[k]
        np.testing.assert_array_equal(v, np.sort(np.argsort(imp)[imp.size - int(imp.size * 0.5):]))
    assert masks.main(["--imp_score", d, "--compress_rate", "[0.5]*55", "--compare", d,
                       "--out", str(tmp_path / "m.npz")]) == 0
