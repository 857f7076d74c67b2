"""The rank criterion on the GPU (dcts_rank_f32 / ops.rank_nc / imp_score(criterion="rank") / the CLI) against the
fp64 oracle of tests/rank_oracle.py: exact ranks of constructed maps, ReLU-conv activations at every hooked shape of
the six nets, edge cases, the harness in three modes and the CLI."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import rank_oracle as ro
from dct_pruning_amd import _lib, harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import deterministic_init

pytestmark = pytest.mark.gpu


def _factor(rows, r, g):
    """rows x r small-integer matrix of rank r: 16 I on top of {-1, 0, 1} noise (well conditioned)."""
    m = torch.randint(-1, 2, (rows, r), generator=g).double()
    m[:r] += 16.0 * torch.eye(r, dtype=torch.float64)
    return m


def _exact_map(H, W, r, g, extra=False):
    """An fp32-exact H x W map of rank exactly r. extra=True: one zero row and one duplicated row (U), one zero column
    and one duplicated column (V)."""
    k = 2 if extra else 0
    U, V = _factor(H - k, r, g), _factor(W - k, r, g).t()
    if extra:
        U = torch.cat([U, torch.zeros(1, r, dtype=U.dtype), U[:1]], 0)
        V = torch.cat([V, torch.zeros(r, 1, dtype=V.dtype), V[:, :1]], 1)
    U = U[torch.randperm(H, generator=g)]
    V = V[:, torch.randperm(W, generator=g)]
    return (U @ V).float()


SHAPES = [(e, e) for e in range(1, 65)] + [(1, 64), (64, 1), (7, 56), (56, 28), (13, 64), (33, 17)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_exact_ranks(H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    n = min(H, W)
    maps, want = [], []
    for r in sorted({0, 1, 2, n // 2, n - 1, n}):
        if not 0 <= r <= n:
            continue
        variants = [False] + ([True] if r <= n - 2 else [])
        for extra in variants:
            a = _exact_map(H, W, r, g, extra)
            for scale in (1.0, 2.0 ** 60, 2.0 ** -60):
                maps.append(a * scale)
                want.append(r)
    x = torch.stack(maps)[None]  # [1, maps, H, W]
    want = torch.tensor(want, dtype=torch.float32)[None]
    assert torch.equal(ro.rank_nc(x), want)  # the construction is what it claims
    assert not ro.undecidable(x).any()
    got = dpa.rank_nc(x.cuda()).cpu()
    assert torch.equal(got, want), (got - want).nonzero()


def _hooked_shapes():
    """Every distinct hooked (H, W) of the six nets with edges <= 64, with the channel count capped."""
    seen = {}
    for name in ("vgg_16_bn", "resnet_56", "resnet_110", "densenet_40", "googlenet", "resnet_50"):
        for p in schedules.SCHEDULES[name]():
            seen.setdefault((p.H, p.W), min(p.C, 48))
    return sorted(seen.items())


@pytest.mark.parametrize("hw,C", _hooked_shapes())
def test_relu_conv_activations_match_oracle(hw, C):
    H, W = hw
    g = torch.Generator().manual_seed(H * 131 + W)
    N = 4 if H * W <= 1024 else 2
    inp = torch.randn(N, 8, H, W + 3, generator=g)
    wgt = torch.randn(C, 8, 3, 3, generator=g) / 8.0
    bias = -torch.linspace(0.0, 2.0, C)  # sparser channels further on: ranks below full as well
    act = torch.relu(torch.nn.functional.conv2d(inp, wgt, bias, padding=1))
    x = act[..., :W]  # strideH = W + 3 > W: rows are not dense
    cb, cc = 3, C - 5
    got = dpa.rank_nc(x.cuda(), c_begin=cb, c_count=cc).cpu()
    ref = ro.rank_nc(x, cb, cc)
    band = ro.undecidable(x, cb, cc)
    assert band.float().mean().item() < 0.01, "band too wide: the test would be vacuous"
    ok = ~band
    assert torch.equal(got[ok], ref[ok]), (got - ref)[ok].abs().max()
    torch_rank = torch.linalg.matrix_rank(x[:, cb:cb + cc].contiguous()).float()  # CPU fp32
    assert torch.equal(torch_rank[ok], ref[ok])
    assert ((got >= 0) & (got <= min(H, W))).all()


def test_edge_cases():
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(6, 20, 14, 14, generator=g))
    x[:, 4] = 0  # a dead channel
    xd = x.cuda()
    a = dpa.rank_nc(xd)
    b = dpa.rank_nc(xd)
    assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert (a[:, 4] == 0).all() and not torch.signbit(a[:, 4]).any()
    # a channel's result does not depend on the slice or on N
    assert torch.equal(dpa.rank_nc(xd, c_begin=5, c_count=3), a[:, 5:8])
    assert torch.equal(dpa.rank_nc(xd[:1]), a[:1])
    assert torch.equal(dpa.rank_nc(xd[2:5], c_begin=9), a[2:5, 9:])
    # one NaN map: the call returns and every other map keeps its value
    y = x.clone()
    y[2, 7, 3, 3] = float("nan")
    c = dpa.rank_nc(y.cuda())
    torch.cuda.synchronize()
    keep = torch.ones_like(c, dtype=torch.bool)
    keep[2, 7] = False
    assert torch.equal(c[keep], a[keep])
    # out= and the unsupported / bad shapes
    out = torch.empty(6, 20, device="cuda")
    assert dpa.rank_nc(xd, out=out) is out and torch.equal(out, a)
    with pytest.raises(_lib.DctScoreError) as e:
        dpa.rank_nc(torch.zeros(1, 1, 72, 72, device="cuda"))
    assert e.value.code == -6 and "rank: edges up to 64" in str(e.value)


def _capture_run(name, root, bs, limit, **kw):
    """imp_score(criterion="rank") on the GPU with a capturing hook ahead of every scoring hook: returns the files,
    stdout, and the oracle's per-file expectation on that run's own activations (plus a per-file decidable mask)."""
    dev = torch.device("cuda")
    net = deterministic_init(nets.get_network(name)).to(dev)
    pts = harness._schedule_for(net, name)
    acts = {}

    def capture(mod, i, o, _m=None):
        if len(mod._forward_hooks) > 1:  # the scoring hook is registered: this sweep scores this module
            acts.setdefault(_m, []).append(o.detach().cpu())

    handles = []
    for p in pts:
        mod = harness._resolve(net, p.module)
        handles.append(mod.register_forward_hook(lambda m, i, o, _p=p.module: capture(m, i, o, _p)))
    loader = SyntheticLoader((3, 32, 32), bs, limit + 1, seed=11)
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
        for h in handles:
            h.remove()
    d = os.path.join(str(root), "rank_conv", "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    expect, decidable = {}, {}
    for p in pts:
        batches = acts[p.module]
        assert len(batches) == limit
        cb, cc, _ = schedules.scored_shape(p)
        ranks = [ro.rank_nc(a, cb, cc) for a in batches]
        ok = torch.stack([~ro.undecidable(a, cb, cc).any(0) for a in batches]).all(0)
        acc = harness.HostAccumulator()
        for r in ranks:
            acc.update(r)
        for stem, lo, hi in p.files:
            s = harness._file_stem("rank", stem)
            sl = slice(lo, hi) if lo is not None else slice(None)
            expect[s] = acc.scores()[sl]
            decidable[s] = ok.numpy()[sl]
    return files, buf.getvalue().splitlines(), expect, decidable


@pytest.mark.parametrize("name", ["resnet_56", "densenet_40"])
def test_harness_modes_match_oracle(name, tmp_path):
    bs, limit = 2, 2
    runs = {}
    for mode, kw in [("per_hook", {}), ("single", {"single_sweep": True}),
                     ("device", {"single_sweep": True, "accumulate": "device"})]:
        files, lines, expect, decidable = _capture_run(name, tmp_path / mode, bs, limit, **kw)
        assert sorted(files) == sorted(expect)
        assert all(k.startswith("rank_conv") for k in files)
        n_dec = 0
        for k, v in files.items():
            assert v.dtype == np.float32 and v.shape == expect[k].shape, k
            np.testing.assert_array_equal(v[decidable[k]], expect[k][decidable[k]], err_msg="%s %s" % (mode, k))
            n_dec += int(decidable[k].sum())
        assert n_dec >= 0.99 * sum(v.size for v in files.values())
        runs[mode] = (files, lines)
    base_files, base_lines = runs["per_hook"]
    assert base_lines[-1] == "The importance score generation has been completed!"
    for mode, (files, lines) in runs.items():
        assert lines == base_lines and sorted(files) == sorted(base_files), mode
        for k in base_files:
            assert np.abs(files[k] - base_files[k]).max() <= 2.0 / (bs * limit), (mode, k)


def test_cli_rank(tmp_path):
    from test_cli_gpu import run_cli
    out = run_cli(tmp_path, "--net", "vgg_16_bn", "--dataset", "cifar10", "--synthetic", "--pretrain_dir", "",
                  "--criterion", "rank", "--batch_size", "16", "--limit", "1")
    assert "The importance score generation has been completed!" in out
    d = tmp_path / "rank_conv" / "vgg_16_bn_limit1"
    files = sorted(os.listdir(d))
    assert files == sorted("rank_conv%d.npy" % i for i in range(1, 13))
    assert not (tmp_path / "importance_score").exists()
    for p, i in zip(schedules.vgg_16_bn(), range(1, 13)):
        a = np.load(d / ("rank_conv%d.npy" % i))
        assert a.dtype == np.float32 and a.shape == (p.C,)
        assert (a >= 0).all() and (a <= min(p.H, p.W)).all()
