"""dcts_gm_distance_f32 on the GPU against the float64 definition of tests/gm_oracle.py, at the relative tolerance derived
there (TOL = 8 R, R the fp32 restatement's own error on these inputs): shapes on both sides of every tile and chunk edge
(64 scored channels, 64 reference channels, 64 elements: grid_caps.h), what the difference form makes exact, independence of
N and of the scored range bit for bit, views on 4- and 16-byte bases, the output's extent, a poisoned sample, and
imp_score(criterion="gm") end to end. The grid is one workgroup per (sample, scored tile) without a cap, so there is no
grid-loop case."""
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
import gm_oracle as go
import loop_cases as lc
from dct_pruning_amd import _lib, harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = go.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, x, ranges=(0, None, 0, None), what=""):
    """got [N, c] float32 on the device against the definition: within TOL relative, +0.0 where the definition is 0."""
    ref = go.gm_nc_f64(x, *ranges)
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == ref.shape, (what, g.shape, ref.shape)
    assert np.isfinite(g).all(), what
    err = go.relative_error(g, ref)
    print("GM %s worst |got - f64| / f64 = %.3e (tol %.3e)" % (what, err, TOL))
    assert err <= TOL, (what, err)
    assert (g[ref == 0].view(np.int32) == 0).all(), what  # +0.0, the sign bit too
    return ref


# ----------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,hw", go.SWEEP, ids=["C%d-%dx%d" % (c, hw[0], hw[1]) for c, hw in go.SWEEP])
def test_shape_sweep(c, hw):
    x = go.sweep_case(c, hw)
    xd = x.to(DEV)
    got = dpa.gm_distance_nc(xd)
    _check(got, x, what="C=%d %dx%d" % (c, hw[0], hw[1]))
    assert torch.equal(_bits(got), _bits(dpa.gm_distance_nc(xd)))  # repeated call
    if c >= 2:
        assert torch.equal(_bits(got[:, 0]), _bits(got[:, c - 1]))  # the duplicated channel: the same reference set, the same bits
    if (c, hw) == go.ZERO_SAMPLE_CASE:
        assert (_bits(got[1]) == 0).all() and (got[0] > 0).all() and (got[2] > 0).all()


# ----------------------------------------------------------------------------------------------------
# exactness
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (8, 8), (25, 40)], ids=lambda s: "%dx%d" % s)
def test_identical_maps_are_at_distance_plus_zero(hw):
    x = go.maps(3, 2, hw[0], hw[1], 31)  # C = 2: channel 1 is channel 0
    assert torch.equal(x[:, 0], x[:, 1]) and (x != 0).any()
    got = dpa.gm_distance_nc(x.to(DEV))
    assert got.shape == (3, 2) and (_bits(got) == 0).all()
    assert (_bits(dpa.gm_distance_nc(torch.zeros(2, 70, hw[0], hw[1], device=DEV))) == 0).all()  # an all-zero tensor


@pytest.mark.parametrize("hw", [(5, 13), (8, 8), (15, 17)], ids=lambda s: "%dx%d" % s)
def test_distance_is_symmetric_bit_for_bit(hw):
    """r_count = 1: reference {k} scored from {j} against reference {j} scored from {k}, for pairs in the same and in
    different tiles of 64 and at every lane distance."""
    x = go.maps(2, 140, hw[0], hw[1], 32)
    xd = x.to(DEV)
    pd = go.pair_distances_f64(x)
    for j, k in ((0, 1), (0, 139), (3, 64), (63, 65), (17, 130), (129, 2), (70, 71), (5, 5)):
        a = dpa.gm_distance_nc(xd, c_begin=j, c_count=1, ref_begin=k, ref_count=1)
        b = dpa.gm_distance_nc(xd, c_begin=k, c_count=1, ref_begin=j, ref_count=1)
        assert torch.equal(_bits(a), _bits(b)), (j, k)
        assert go.relative_error(a.cpu().numpy()[:, 0], pd[:, j, k]) <= TOL, (j, k)
    # and as entries of whole rows: the full pairwise matrix, one reference channel per call
    cols = torch.stack([dpa.gm_distance_nc(xd, ref_begin=k, ref_count=1) for k in range(0, 140, 7)], dim=2)  # [N, C, 20]
    for i, k in enumerate(range(0, 140, 7)):
        assert torch.equal(_bits(cols[:, k, i]), torch.zeros(2, dtype=torch.int32, device=DEV))  # d(k, k) = +0.0
    sym = cols[:, 0:140:7, :]  # [N, 20, 20]: d(7 a, 7 b)
    assert torch.equal(_bits(sym), _bits(sym.transpose(1, 2)))


# ----------------------------------------------------------------------------------------------------
# independence, bit for bit
# ----------------------------------------------------------------------------------------------------
def test_channel_range_pieces_are_slices_of_the_unsplit_call():
    x = go.piece_case()
    xd = x.to(DEV)
    full = dpa.gm_distance_nc(xd)
    _check(full, x, what="pieces, unsplit")
    for cb, cc in ((1, 1), (7, 1), (3, 5), (65, 5), (1, 37), (39, 37), (63, 2)):
        piece = dpa.gm_distance_nc(xd, c_begin=cb, c_count=cc)  # against the full reference set
        assert torch.equal(_bits(piece), _bits(full[:, cb:cb + cc])), (cb, cc)
    # consecutive pieces concatenate to the whole
    cuts = (0, 1, 6, 43, 77)
    cat = torch.cat([dpa.gm_distance_nc(xd, c_begin=a, c_count=b - a) for a, b in zip(cuts, cuts[1:])], dim=1)
    assert torch.equal(_bits(cat), _bits(full))


def test_a_sample_alone_gives_the_bits_it_gives_in_a_batch():
    x = go.batch_case()
    xd = x.to(DEV)
    full = dpa.gm_distance_nc(xd)
    _check(full, x, what="batch of 5")
    for n in (0, 3, 4):
        one = dpa.gm_distance_nc(xd[n:n + 1].contiguous())
        assert torch.equal(_bits(one), _bits(full[n:n + 1])), n


def test_reference_set_that_is_a_proper_subrange():
    x = go.subrange_case()
    C = x.shape[1]
    xd = x.to(DEV)
    ranges = (0, None, 3, C - 5)
    got = dpa.gm_distance_nc(xd, ref_begin=3, ref_count=C - 5)
    _check(got, x, ranges, what="subrange")
    assert not torch.equal(_bits(got), _bits(dpa.gm_distance_nc(xd)))
    # the same reference maps at channel 0 of a tensor of their own: the sum's order follows the position in the reference set
    ref_only = xd[:, 3:C - 2].contiguous()
    both = torch.cat([ref_only, xd], dim=1)
    twin = dpa.gm_distance_nc(both, c_begin=C - 5, c_count=C, ref_begin=0, ref_count=C - 5)
    assert torch.equal(_bits(got), _bits(twin))


# ----------------------------------------------------------------------------------------------------
# views
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(6, 6), (7, 7)], ids=lambda s: "%dx%d" % s)
def test_views_give_the_bits_of_a_contiguous_aligned_copy(hw):
    """h * w = 36 takes the 16-byte loads on an aligned dense tensor, 49 the dword loads; every view below takes whichever
    its base and strides allow and must not differ by a bit."""
    h, w = hw
    x = go.view_case(h, w)
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0
    base = dpa.gm_distance_nc(xd)
    _check(base, x, what="views %dx%d" % hw)
    # a sample-strided view
    v = xd[::2]
    assert not v.is_contiguous()
    assert torch.equal(_bits(dpa.gm_distance_nc(v)), _bits(base[::2]))
    # a channel-sliced view of a wider tensor: strideC unchanged, nothing is copied
    wide = torch.full((4, 30, h, w), 3.0, device=DEV)
    wide[:, 4:25] = xd
    sl = wide[:, 4:25]
    assert sl.stride(1) == h * w and sl.stride(0) == 30 * h * w and not sl.is_contiguous()
    assert torch.equal(_bits(dpa.gm_distance_nc(sl)), _bits(base))
    assert torch.equal(_bits(dpa.gm_distance_nc(wide, c_begin=4, c_count=21, ref_begin=4, ref_count=21)), _bits(base))
    # a base that is 4-byte but not 16-byte aligned: a flat buffer offset by one element
    flat = torch.zeros(xd.numel() + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    off = flat[1:1 + xd.numel()].view(xd.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(_bits(dpa.gm_distance_nc(off)), _bits(base))
    # a row-pitched view goes through the operator's copy
    pitched = torch.full((4, 21, h, w + 3), 3.0, device=DEV)
    pitched[..., :w] = xd
    pv = pitched[..., :w]
    assert pv.stride(2) == w + 3
    assert torch.equal(_bits(dpa.gm_distance_nc(pv)), _bits(base))
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(4, 21, device=DEV)
    rc = _lib.load().dcts_gm_distance_f32(pv.data_ptr(), 4, 21, h, w, pv.stride(0), pv.stride(1), pv.stride(2), 1, 0, 21, 0, 21,
                                          out.data_ptr(), stream)
    assert rc == -6  # the C entry refuses the pitch: the copy is the operator's


# ----------------------------------------------------------------------------------------------------
# the output's extent, a poisoned sample
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cb,cc", [(70, 0, 70), (70, 3, 65), (12, 5, 1)], ids=["full", "piece", "one"])
def test_only_the_output_is_written(c, cb, cc):
    x = go.maps(3, c, 7, 9, 41).to(DEV)
    front = 64
    buf = torch.full((front + 3 * cc + lc.GUARD,), float("nan"), device=DEV)
    out = buf[front:front + 3 * cc].view(3, cc)
    assert dpa.gm_distance_nc(x, c_begin=cb, c_count=cc, out=out) is out
    assert bool(torch.isfinite(out).all())
    assert bool(torch.isnan(buf[:front]).all()) and bool(torch.isnan(buf[front + 3 * cc:]).all())
    assert torch.equal(_bits(out), _bits(dpa.gm_distance_nc(x)[:, cb:cb + cc]))


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_poisoned_map_stays_in_its_sample(poison):
    x = go.maps(3, 70, 7, 7, 42).to(DEV)
    clean = dpa.gm_distance_nc(x)
    y = x.clone()
    y[1, 66, 3, 1] = poison
    got = dpa.gm_distance_nc(y)
    assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(_bits(got[2]), _bits(clean[2]))
    assert not bool(torch.isfinite(got[1]).any())  # a term of every sum of its sample
    # a reference set without the poisoned map: its sample is clean again, except the poisoned map's own score
    part = dpa.gm_distance_nc(y, ref_begin=0, ref_count=64)
    assert torch.equal(_bits(part[:, :66]), _bits(dpa.gm_distance_nc(x, ref_begin=0, ref_count=64)[:, :66]))
    assert not bool(torch.isfinite(part[1, 66]))


# ----------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------
def test_imp_score_gm_on_resnet_56_against_the_oracle(tmp_path):
    name = "resnet_56"
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).to(DEV)
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(net, args, train_loader=loader, criterion="gm", single_sweep=True)
    finally:
        os.chdir(cwd)
    d = tmp_path / "gm_score" / ("%s_limit%d" % (name, limit))
    out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert len(out) == 55 and all(k.startswith("gm_") for k in out)

    # the oracle over the same batch through the same net on the CPU (MIOpen differs from the CPU's convolutions: the
    # tolerance of test_imp_score_on_gpu_matches_reference_run)
    cpu = deterministic_init(nets.get_network(name)).eval()
    x = next(iter(SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)))[0]
    pts = schedules.SCHEDULES[name]()
    seen = {}
    handles = [harness._resolve(cpu, p.module).register_forward_hook(
        lambda m, i, o, _p=p: seen.__setitem__(_p.module, o.detach().clone())) for p in pts]
    with torch.no_grad():
        cpu(x)
    for h in handles:
        h.remove()
    checked = 0
    for p in pts:
        want = go.gm_nc_f64(seen[p.module]).mean(axis=0)
        for stem, lo, hi in p.files:
            got = out["gm_" + stem[len("imp_"):]]
            ref = want if lo is None else want[lo:hi]
            assert got.dtype == np.float32 and got.shape == ref.shape, stem
            big = ref > 1e-6 * ref.max()  # as there: relative on the live channels, dead ones stay (near-)dead
            np.testing.assert_allclose(got[big], ref[big], rtol=2e-3, err_msg=stem)
            assert np.all(got[ref == 0] <= 1e-6 * max(ref.max(), 1e-30)), stem
            checked += 1
    assert checked == 55


def test_cli_writes_gm_score(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "importance_generation.py"), "--net", "resnet_56", "--dataset", "cifar10",
                        "--synthetic", "--pretrain_dir", "", "--batch_size", "4", "--limit", "1", "--criterion", "gm",
                        "--single_sweep"], cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout
    assert "Importance Score is located at ./gm_score/resnet_56_limit1" in p.stdout
    d = tmp_path / "gm_score" / "resnet_56_limit1"
    pts = schedules.SCHEDULES["resnet_56"]()
    assert sorted(os.listdir(d)) == sorted("gm_" + s[len("imp_"):] + ".npy" for pt in pts for s, _, _ in pt.files)
    assert not (tmp_path / "importance_score").exists()
    for f in os.listdir(d):
        v = np.load(d / f)
        assert v.dtype == np.float32 and v.ndim == 1 and np.isfinite(v).all() and (v >= 0).all(), f
    from dct_pruning_amd import masks
    m = masks.masks_for_dir(str(d), 0.5)
    assert len(m) == 55
