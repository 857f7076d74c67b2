"""dcts_gm_distance_metric_f32 on the GPU against the float64 definition of tests/gm_metric_oracle.py at the absolute
tolerance derived there (|got - f64| <= TOL[metric] * r_count, TOL = 8 R): the shape sweep of tests/gm_oracle.py, stats lanes
that loop, what the unit maps make exact (with the sign bit), bits that must not depend on the call, metric "l2" against the
operator as it was, the extent of what is written, a NaN map, and imp_score / the CLI end to end."""
import contextlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import gm_metric_oracle as mo
import gm_oracle as go
from dct_pruning_amd import _lib, harness, nets, ops, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = mo.METRICS


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gm(x, metric, **kw):
    return dpa.gm_distance_nc(x, metric=metric, **kw)


def _check(got, x, metric, ranges=(0, None, 0, None), what=""):
    """got [N, c] float32 on the device against the definition: within TOL * r_count, +0.0 where the definition is 0."""
    ref = mo.gm_metric_nc_f64(x, metric, *ranges)
    g = got.cpu().numpy()
    rc = mo.r_count_of(x, ranges)
    assert g.dtype == np.float32 and g.shape == ref.shape, (what, g.shape, ref.shape)
    assert np.isfinite(g).all(), what
    err = mo.error_per_reference(g, ref, rc)
    print("GM %s %s worst |got - f64| / r_count = %.3e (tol %.3e)" % (metric, what, err, mo.TOL[metric]))
    assert err <= mo.TOL[metric], (what, err)
    assert (g[ref == 0].view(np.int32) == 0).all(), what  # +0.0, the sign bit too
    return ref


# ----------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,hw", go.SWEEP, ids=["C%d-%dx%d" % (c, hw[0], hw[1]) for c, hw in go.SWEEP])
def test_shape_sweep(c, hw):
    x = go.sweep_case(c, hw)
    xd = x.to(DEV)
    for metric in METRICS:
        got = _gm(xd, metric)
        _check(got, x, metric, what="C=%d %dx%d" % (c, hw[0], hw[1]))
        assert torch.equal(_bits(got), _bits(_gm(xd, metric)))  # repeated call
        if c >= 2:
            assert torch.equal(_bits(got[:, 0]), _bits(got[:, c - 1]))  # the duplicated channel
        if (c, hw) == go.ZERO_SAMPLE_CASE:
            assert (_bits(got[1]) == 0).all() and (got[0] > 0).all() and (got[2] > 0).all()
        if hw == (1, 1) and metric == "correlation":
            assert (_bits(got) == 0).all()  # every 1 x 1 map is flat


def test_stats_lanes_that_loop():
    x = mo.loop_case()  # 72 x 72: 81 elements per lane
    xd = x.to(DEV)
    for metric in METRICS:
        got = _gm(xd, metric)
        _check(got, x, metric, what="loop 72x72")
        off = torch.zeros(x.numel() + 4, device=DEV)[1:1 + x.numel()].view(x.shape)  # the dword path on the same maps
        off.copy_(xd)
        assert off.data_ptr() % 16 == 4 and torch.equal(_bits(_gm(off, metric)), _bits(got))


# ----------------------------------------------------------------------------------------------------
# exactness
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(2, 2), (7, 7), (8, 8), (25, 40)], ids=lambda s: "%dx%d" % s)
def test_duplicates_multiples_and_flat_maps_are_at_distance_plus_zero(hw):
    x = torch.randn(3, 70, hw[0], hw[1], generator=torch.Generator().manual_seed(51))
    x[:, 1] = x[:, 0]
    x[:, 66] = x[:, 0] * 2.0 ** 10
    x[:, 3] = x[:, 0] * 2.0 ** -9
    x[:, 5] = 0.0
    x[:, 69] = 0.0
    xd = x.to(DEV)
    for metric in METRICS:
        if metric == "correlation":
            xd[:, 69] = 0.1  # a constant map is as flat as a zero map
        for j, k in ((0, 1), (0, 66), (0, 3), (66, 3), (3, 1), (5, 69), (69, 5), (7, 7), (68, 68)):
            d = _gm(xd, metric, c_begin=j, c_count=1, ref_begin=k, ref_count=1)
            assert (_bits(d) == 0).all(), (metric, j, k)
        full = _gm(xd, metric)
        _check(full, xd.cpu(), metric, what="exactness %dx%d" % hw)
        for j in (1, 66, 3):
            assert torch.equal(_bits(full[:, j]), _bits(full[:, 0])), (metric, j)  # the same unit map, the same score
        assert torch.equal(_bits(full[:, 5]), _bits(full[:, 69]))
        # a flat map: distance 1 to each of the 68 maps that are not flat, 0 to the other flat one and to itself
        np.testing.assert_allclose(full[:, 5].cpu().numpy(), 68.0, rtol=1e-5)
        assert (_bits(_gm(torch.zeros(2, 70, hw[0], hw[1], device=DEV), metric)) == 0).all()  # an all-zero tensor


@pytest.mark.parametrize("metric", METRICS)
def test_distance_is_symmetric_bit_for_bit(metric):
    x = go.maps(2, 140, 5, 13, 32)
    xd = x.to(DEV)
    for j, k in ((0, 2), (0, 138), (3, 64), (63, 65), (17, 130), (129, 2), (70, 71)):
        a = _gm(xd, metric, c_begin=j, c_count=1, ref_begin=k, ref_count=1)
        b = _gm(xd, metric, c_begin=k, c_count=1, ref_begin=j, ref_count=1)
        assert torch.equal(_bits(a), _bits(b)) and bool((a > 0).all()) and bool((a <= 2).all()), (j, k)


# ----------------------------------------------------------------------------------------------------
# bits that must not depend on the call
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_pieces_batches_and_subranges(metric):
    x = go.piece_case()
    xd = x.to(DEV)
    full = _gm(xd, metric)
    _check(full, x, metric, what="pieces, unsplit")
    for cb, cc in ((1, 1), (3, 5), (65, 5), (1, 37), (63, 2)):
        assert torch.equal(_bits(_gm(xd, metric, c_begin=cb, c_count=cc)), _bits(full[:, cb:cb + cc])), (cb, cc)
    cuts = (0, 1, 6, 43, 77)
    cat = torch.cat([_gm(xd, metric, c_begin=a, c_count=b - a) for a, b in zip(cuts, cuts[1:])], dim=1)
    assert torch.equal(_bits(cat), _bits(full))

    x = go.batch_case()
    xd = x.to(DEV)
    full = _gm(xd, metric)
    _check(full, x, metric, what="batch of 5")
    for n in (0, 3, 4):
        assert torch.equal(_bits(_gm(xd[n:n + 1].contiguous(), metric)), _bits(full[n:n + 1])), n

    x = go.subrange_case()
    C = x.shape[1]
    xd = x.to(DEV)
    got = _gm(xd, metric, ref_begin=3, ref_count=C - 5)
    _check(got, x, metric, (0, None, 3, C - 5), what="subrange")
    assert not torch.equal(_bits(got), _bits(_gm(xd, metric)))
    both = torch.cat([xd[:, 3:C - 2].contiguous(), xd], dim=1)
    twin = _gm(both, metric, c_begin=C - 5, c_count=C, ref_begin=0, ref_count=C - 5)
    assert torch.equal(_bits(got), _bits(twin))


@pytest.mark.parametrize("hw", [(6, 6), (7, 7)], ids=lambda s: "%dx%d" % s)
def test_views_give_the_bits_of_a_contiguous_aligned_copy(hw):
    h, w = hw
    x = go.view_case(h, w)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0
    for metric in METRICS:
        base = _gm(xd, metric)
        _check(base, x, metric, what="views %dx%d" % hw)
        assert torch.equal(_bits(_gm(xd[::2], metric)), _bits(base[::2]))  # a sample-strided view
        wide = torch.full((4, 30, h, w), 3.0, device=DEV)
        wide[:, 4:25] = xd
        assert torch.equal(_bits(_gm(wide[:, 4:25], metric)), _bits(base))
        assert torch.equal(_bits(_gm(wide, metric, c_begin=4, c_count=21, ref_begin=4, ref_count=21)), _bits(base))
        flat = torch.zeros(xd.numel() + 4, device=DEV)
        off = flat[1:1 + xd.numel()].view(xd.shape)  # a base off by one float
        off.copy_(xd)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert torch.equal(_bits(_gm(off, metric)), _bits(base))


# ----------------------------------------------------------------------------------------------------
# "l2" is the operator as it was
# ----------------------------------------------------------------------------------------------------
def test_l2_is_gm_distance_nc_as_it_is():
    x = go.piece_case().to(DEV)
    plain = dpa.gm_distance_nc(x, c_begin=3, c_count=70, ref_begin=1, ref_count=75)
    assert torch.equal(_bits(_gm(x, "l2", c_begin=3, c_count=70, ref_begin=1, ref_count=75)), _bits(plain))
    out = torch.full((2, 70), float("nan"), device=DEV)
    rc = _lib.load().dcts_gm_distance_metric_f32(x.data_ptr(), 2, 77, 5, 13, x.stride(0), x.stride(1), 13, 1, 3, 70, 1, 75,
                                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream, 0, None, 0)
    assert rc == 0 and torch.equal(_bits(out), _bits(plain))


# ----------------------------------------------------------------------------------------------------
# what is written, a NaN map
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("c,cb,cc,rb,rc", [(70, 0, 70, 0, 70), (70, 3, 65, 0, 70), (12, 5, 1, 2, 9)], ids=["full", "piece", "one"])
def test_only_the_output_and_the_declared_workspace_are_written(metric, c, cb, cc, rb, rc):
    lib = _lib.load()
    x = go.maps(3, c, 7, 9, 41).to(DEV)
    code = ops.GM_METRICS[metric]
    need = lib.dcts_gm_workspace_bytes(code, 3, cc, rc)
    assert need > 0 and need % 16 == 0
    guard = 1024
    obuf = torch.full((guard + 3 * cc + guard,), float("nan"), device=DEV)
    out = obuf[guard:guard + 3 * cc]
    wbuf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wbuf[guard:guard + need]
    assert ws.data_ptr() % 16 == 0
    lib.dcts_workspace_invalidate_range(ws.data_ptr(), need)
    status = lib.dcts_gm_distance_metric_f32(x.data_ptr(), 3, c, 7, 9, x.stride(0), x.stride(1), 9, 1, cb, cc, rb, rc,
                                             out.data_ptr(), torch.cuda.current_stream().cuda_stream, code, ws.data_ptr(), need)
    assert status == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert bool(torch.isnan(obuf[:guard]).all()) and bool(torch.isnan(obuf[guard + 3 * cc:]).all())
    assert bool((wbuf[:guard] == 0xA5).all()) and bool((wbuf[guard + need:] == 0xA5).all())
    assert torch.equal(_bits(out.view(3, cc)), _bits(_gm(x, metric, c_begin=cb, c_count=cc, ref_begin=rb, ref_count=rc)))


@pytest.mark.parametrize("metric", METRICS)
def test_a_nan_map_stays_in_its_sample(metric):
    x = go.maps(3, 70, 7, 7, 42).to(DEV)
    clean = _gm(x, metric)
    y = x.clone()
    y[1, 66, 3, 1] = float("nan")
    got = _gm(y, metric)
    assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(_bits(got[2]), _bits(clean[2]))
    assert not bool(torch.isfinite(got[1]).any())  # a term of every sum of its sample
    part = _gm(y, metric, ref_begin=0, ref_count=64)  # a reference set without the NaN map
    assert torch.equal(_bits(part[:, :66]), _bits(_gm(x, metric, ref_begin=0, ref_count=64)[:, :66]))
    assert not bool(torch.isfinite(part[1, 66]))


# ----------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------
def test_imp_score_gm_cosine_on_resnet_56_against_the_oracle(tmp_path):
    name = "resnet_56"
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).to(DEV)
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    seen = {}
    pts = schedules.SCHEDULES[name]()
    handles = [harness._resolve(net, p.module).register_forward_hook(
        lambda m, i, o, _p=p: seen.__setitem__(_p.module, o.detach().cpu())) for p in pts]  # the activations the hooks see
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(net, args, train_loader=loader, criterion="gm", gm_metric="cosine", single_sweep=True)
    finally:
        os.chdir(cwd)
        for h in handles:
            h.remove()
    d = tmp_path / "gm_score" / ("%s_limit%d_cosine" % (name, limit))
    out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert len(out) == 55 and all(k.startswith("gm_") for k in out)
    checked = 0
    for p in pts:
        C = seen[p.module].shape[1]
        want = mo.gm_metric_nc_f64(seen[p.module], "cosine").mean(axis=0)
        for stem, lo, hi in p.files:
            got = out["gm_" + stem[len("imp_"):]]
            ref = want if lo is None else want[lo:hi]
            assert got.dtype == np.float32 and got.shape == ref.shape, stem
            assert np.abs(got - ref).max() <= mo.TOL["cosine"] * C + 1e-6 * ref.max(), stem  # + the float32 mean over the batch
            checked += 1
    assert checked == 55


def test_cli_writes_gm_score_correlation(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "importance_generation.py"), "--net", "resnet_56", "--dataset", "cifar10",
                        "--synthetic", "--pretrain_dir", "", "--batch_size", "4", "--limit", "1", "--criterion", "gm",
                        "--gm_metric", "correlation", "--single_sweep"], cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    assert "Importance Score is located at ./gm_score/resnet_56_limit1_correlation" in p.stdout
    assert os.listdir(tmp_path / "gm_score") == ["resnet_56_limit1_correlation"]
    d = tmp_path / "gm_score" / "resnet_56_limit1_correlation"
    pts = schedules.SCHEDULES["resnet_56"]()
    assert sorted(os.listdir(d)) == sorted("gm_" + s[len("imp_"):] + ".npy" for pt in pts for s, _, _ in pt.files)
    for pt in pts:
        for s, _, _ in pt.files:
            v = np.load(d / ("gm_" + s[len("imp_"):] + ".npy"))
            assert v.dtype == np.float32 and v.ndim == 1 and np.isfinite(v).all() and (v >= 0).all(), s
            assert (v <= 2 * v.shape[0]).all(), s  # every term lies in [0, 2]
