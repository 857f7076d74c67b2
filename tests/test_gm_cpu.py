"""The geometric-median criterion's host side without a GPU: the C ABI entry point (declared, bound, exported, argument
codes), the oracle's own properties (tests/gm_oracle.py), the operator's input checks, imp_score(criterion="gm") with the
oracle in the kernel's place - the reference set of every hook kind, and of a hook point scored in channel ranges -, the mask
tool on its files and the CLI's parse errors."""
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import gm_oracle as go
import dct_pruning_amd as dpa
from dct_pruning_amd import _lib, harness, masks, nets, ops, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_gm_entry_point_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    head = text[:text.index("#define DCTS_ABI_VERSION")]
    assert "dcts_gm_distance_f32" in head, "not listed among the additions to ABI 3"
    proto = re.search(r"int dcts_gm_distance_f32\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["dcts_gm_distance_f32"][1]) == 15
    assert "pad_front_if_odd" not in proto and "no-op by construction" in text
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dcts_gm_distance_f32") and _lib.load().dcts_version() == 3
    assert "gm_distance_nc" in dpa.__all__ and dpa.gm_distance_nc is ops.gm_distance_nc
    assert harness._gm_nc is ops.gm_distance_nc


def test_gm_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, rb=0, rc=4, out=fake):
        return lib.dcts_gm_distance_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, rb, rc, out, None)

    assert call(x=None) == -1 and call(out=None) == -1
    assert call(n=0) == -2 and call(c=0) == -2 and call(h=0) == -2 and call(w=-1) == -2
    assert call(h=513, w=513, sh=513) == -2 and call(h=1, w=513, sh=513) == -2
    # the scored range
    assert call(cb=2, cc=3) == -3 and call(cc=0) == -3 and call(cb=-1) == -3
    # the reference range
    assert call(rc=0) == -3 and call(rb=2, rc=3) == -3 and call(rb=-1) == -3 and call(rb=4, rc=1) == -3
    assert call(cb=1, cc=2, rb=3, rc=2) == -3
    # dense maps only: rows that overlap or a stride between elements are malformed, a row pitch is the caller's copy
    assert call(sw=2) == -4 and call(sh=4) == -4 and call(sh=0) == -4
    assert call(sh=12, sc=96, sn=384) == -6
    assert call(x=0x1001) == -7 and call(x=0x1002) == -7 and call(out=0x1002) == -7
    # the order of the checks: NULL, shape, channels, stride, alignment
    assert call(x=None, h=0) == -1 and call(h=0, cc=0) == -2 and call(rc=0, sw=2) == -3 and call(sw=2, x=0x1001) == -4
    assert call(sh=12, x=0x1001) == -7


# ---------------------------------------------------------------------------------------------------------
# the operator's input checks
# ---------------------------------------------------------------------------------------------------------
def test_ops_reject_half_cpu_and_3d_tensors():
    with pytest.raises(TypeError):
        ops.gm_distance_nc(torch.zeros(1, 2, 8, 8, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.gm_distance_nc(torch.zeros(1, 2, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gm_distance_nc(torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError):
        ops.gm_distance_nc(torch.zeros(2, 8, 8))
    with pytest.raises(TypeError):
        ops.gm_distance_nc(np.zeros((1, 2, 8, 8), np.float32))


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def test_oracle_duplicates_zero_maps_and_known_answer():
    x = go.maps(2, 9, 5, 7, 11)  # channel 1 zero, channel 8 a copy of channel 0
    for f in (go.gm_nc_f64, go.gm_nc_f32):
        d = f(x, 0, 1, 8, 1)
        assert (d == 0).all() and not np.signbit(d).any()          # a duplicate pair: exactly +0.0
        full = f(x)
        assert (full[:, 0] == full[:, 8]).all() and (full > 0).all()
        assert (f(torch.zeros(2, 5, 3, 3)) == 0).all()
        assert (f(x, 3, 1, 3, 1) == 0).all()                         # the k == c term
    # a known answer: maps e_0, 2 e_1, 0 in R^4: distances sqrt(5), 1, 2
    k = torch.zeros(1, 3, 2, 2)
    k[0, 0, 0, 0], k[0, 1, 0, 1] = 1.0, 2.0
    np.testing.assert_allclose(go.gm_nc_f64(k)[0], [5 ** 0.5 + 1, 5 ** 0.5 + 2, 3.0], rtol=1e-15)
    # the norm of a zero channel's partner: the distance to the zero map is the map's own norm
    a = go._flat(x, np.float64)
    np.testing.assert_allclose(go.gm_nc_f64(x, 0, None, 1, 1), np.sqrt((a * a).sum(-1)), rtol=1e-15)
    got = go.gm_nc(x, 2, 3, 1, 5)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3)


def test_oracle_symmetry_ranges_and_pad_invariance():
    x = go.maps(2, 9, 5, 7, 12)
    for f in (go.gm_nc_f64, go.gm_nc_f32):
        for j, k in ((0, 3), (2, 7), (1, 4), (8, 0)):
            np.testing.assert_array_equal(f(x, j, 1, k, 1), f(x, k, 1, j, 1))  # d(a, b) == d(b, a), bit for bit
        full = f(x)
        np.testing.assert_array_equal(np.concatenate([f(x, 0, 1), f(x, 1, 5), f(x, 6, 3)], axis=1), full)
        # a zero row and a zero column in front of every map change nothing: the odd pad is a no-op. The float32 chain meets
        # the same non-zero terms in the same order (bit for bit); numpy's float64 sum blocks a longer row differently
        padded = torch.nn.functional.pad(x, (1, 0, 1, 0))
        if f is go.gm_nc_f32:
            np.testing.assert_array_equal(f(padded), full)
        np.testing.assert_allclose(f(padded), full, rtol=1e-14)
    pd = go.pair_distances_f64(x, 2, 4, 1, 6)
    np.testing.assert_array_equal(pd.sum(-1), go.gm_nc_f64(x, 2, 4, 1, 6))
    np.testing.assert_array_equal(pd, go.pair_distances_f64(x)[:, 2:6, 1:7])


def test_sweep_covers_what_the_issue_asks_for():
    assert len(go.SWEEP) == len(set(go.SWEEP)) == 3 * len(go.CHANNELS)
    for c in go.CHANNELS:
        assert sum(1 for cc, _ in go.SWEEP if cc == c) >= 3, c
    for hw in go.SIZES:
        assert sum(1 for _, s in go.SWEEP if s == hw) >= 3, hw
    assert go.ZERO_SAMPLE_CASE in go.SWEEP
    x = go.sweep_case(*go.ZERO_SAMPLE_CASE)
    assert (x[1] == 0).all() and (x[0, 1] == 0).all() and torch.equal(x[0, 0], x[0, -1]) and (x[0, 0] != 0).any()


def test_tolerance_is_eight_times_the_measured_restatement_error():
    """The constant in gm_oracle.py against a fresh measurement on the small inputs (H * W <= 64; the one that sets R,
    128 channels of 1 x 1 maps, among them)."""
    assert go.TOL == 8 * go.R and 1e-7 < go.R < 1e-5
    worst = 0.0
    for name, x, ranges in go.gpu_inputs():
        if x.shape[2] * x.shape[3] <= 64:
            worst = max(worst, go.restatement_error(x, ranges))
    assert go.R / 4 <= worst <= 2 * go.R, worst


# ---------------------------------------------------------------------------------------------------------
# harness, mask tool, CLI
# ---------------------------------------------------------------------------------------------------------
def _run(name, root, criterion, **kw):
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
            harness.imp_score(net, args, train_loader=loader, criterion=criterion, **kw)
    finally:
        os.chdir(cwd)
    top = "gm_score" if criterion == "gm" else "importance_score"
    d = os.path.join(str(root), top, "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return files, buf.getvalue().splitlines(), d


def _activations(name):
    """{module path: the tensor its hook scores} of the one batch the harness cases run."""
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).eval()
    x = next(iter(SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)))[0]
    pts = schedules.SCHEDULES[name]()
    seen = {}
    handles = [harness._resolve(net, p.module).register_forward_hook(
        lambda m, i, o, _p=p: seen.__setitem__(_p.module, (i[0] if _p.kind == "input" else o).detach().clone())) for p in pts]
    with torch.no_grad():
        net(x)
    for h in handles:
        h.remove()
    return pts, seen


@pytest.fixture
def oracle_ops(monkeypatch):
    monkeypatch.setattr(harness, "_gm_nc", go.gm_nc)
    monkeypatch.setattr(harness, "_energy_nc", orc.energy_nc_batched)


@pytest.mark.parametrize("name", ["resnet_56", "densenet_40"])
def test_imp_score_gm(name, tmp_path, oracle_ops):
    assert "gm" in harness.CRITERIA
    gm, lines, d = _run(name, tmp_path / "gm", "gm")
    dct, lines_d, d_dct = _run(name, tmp_path / "dct", "dct")
    assert d.endswith(os.path.join("gm_score", "%s_limit1" % name))
    assert len(gm) == len(dct) > 0 and sorted(gm) == sorted("gm_" + s[len("imp_"):] for s in dct)
    assert lines == [ln.replace("./importance_score/", "./gm_score/") for ln in lines_d]
    assert not (tmp_path / "gm" / "importance_score").exists()
    single, _, _ = _run(name, tmp_path / "single", "gm", single_sweep=True)
    assert sorted(single) == sorted(gm)

    # the values: the oracle's mean over the very activations the hooks saw (one batch of two samples), every scored map
    # against the channels that compete for its mask: all of them, or the last 12
    pts, seen = _activations(name)
    checked, kinds = 0, set()
    for p in pts:
        x = seen[p.module]
        C = x.shape[1]
        cb, cc = (C - 12, 12) if p.kind == "last12" else (0, C)
        want = go.gm_nc_f64(x, cb, cc, cb, cc).mean(axis=0)
        kinds.add(p.kind)
        for stem, lo, hi in p.files:
            got = gm["gm_" + stem[len("imp_"):]]
            ref = want if lo is None else want[lo:hi]
            assert got.dtype == np.float32 and got.shape == ref.shape, stem
            np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0, err_msg=stem)
            np.testing.assert_allclose(single["gm_" + stem[len("imp_"):]], got, rtol=1e-6, atol=0, err_msg=stem)
            checked += 1
        if p.kind == "last12" and C > 12:  # not the whole tensor's channels
            assert not np.allclose(want, go.gm_nc_f64(x, cb, cc, 0, C).mean(axis=0), rtol=1e-3)
    assert checked == len(gm)
    assert kinds == ({"full", "last12"} if name == "densenet_40" else {"full"})

    # on-disk format: the dct files' own header, byte for byte (NumPy v1.0, '<f4', C order, data at byte 128)
    for k in gm:
        raw = open(os.path.join(d, k + ".npy"), "rb").read()
        ref_raw = open(os.path.join(d_dct, "imp_" + k[len("gm_"):] + ".npy"), "rb").read()
        assert raw[:128] == ref_raw[:128] and raw[:8] == b"\x93NUMPY\x01\x00" and len(raw) == 128 + 4 * gm[k].size, k

    # the mask tool reads the directory as it reads any directory of per-channel scores
    m = masks.masks_for_dir(d, 0.5)
    assert sorted(m) == sorted(gm)
    for k, v in m.items():
        c = gm[k].shape[0]
        np.testing.assert_array_equal(v, orc.select_index(gm[k], c, orc.kept_filters(c, 0.5)))
    assert masks.main(["--imp_score", d, "--compress_rate", "[0.5]*%d" % len(gm), "--out", str(tmp_path / "m.npz")]) == 0
    assert sorted(np.load(str(tmp_path / "m.npz")).files) == sorted(gm)


@pytest.mark.parametrize("kind,C", [("full", 24), ("last12", 24), ("input", 24)])
def test_point_hook_in_channel_ranges_scores_against_the_whole_reference_set(kind, C, oracle_ops):
    """A hook point cut in two (what sharding.make_units does to a wide layer): the pieces are the unsplit values exactly,
    which they are only if every piece is compared with the hook kind's WHOLE channel set."""
    x = go.maps(2, C, 6, 5, 21)
    base, count = (C - 12, 12) if kind == "last12" else (0, C)
    cut = 5
    whole = harness._PointHook(kind, "host", torch.device("cpu"), key="w", criterion="gm")
    split = harness._PointHook(kind, "host", torch.device("cpu"), ranges=[("a", 0, cut), ("b", cut, count)], nominal_c=count,
                               criterion="gm")
    for hook in (whole, split):
        hook(None, (x,), x)
    want = go.gm_nc_f64(x, base, count, base, count).mean(axis=0).astype(np.float32)
    np.testing.assert_allclose(whole.scores("w"), want, rtol=1e-6)
    np.testing.assert_array_equal(np.concatenate([split.scores("a"), split.scores("b")]), whole.scores("w"))
    # what the pieces would be without the reference set handed through: each piece against itself
    alone = go.gm_nc_f64(x, base, cut, base, cut).mean(axis=0)
    assert not np.allclose(split.scores("a"), alone, rtol=1e-3)


def test_gm_hooks_have_reference_signature(oracle_ops):
    m = torch.nn.ReLU()
    x = torch.relu(torch.randn(2, 24, 9, 9, generator=torch.Generator().manual_seed(3)))
    for hook, cb, cc in [(harness.get_feature_hook_gm, 0, 24), (harness.get_feature_hook_densenet_gm, 12, 12),
                         (harness.get_feature_hook_u2net_input_gm, 0, 24)]:
        harness._acc.reset()
        h = m.register_forward_hook(hook)
        m(x)
        h.remove()
        want = go.gm_nc_f64(x, cb, cc, cb, cc).mean(axis=0)  # x is non-negative: relu(x) == x, input == output
        got = harness._acc.feature_result.numpy()
        assert got.shape == (cc,) and harness._acc.total.item() == 2
        np.testing.assert_allclose(got, want, rtol=1e-6)
    harness._acc.reset()
    assert harness._file_stem("gm", "imp_conv3") == "gm_conv3"
    assert harness._file_stem("gm", "net.stage1.rebnconv1.relu_s1") == "gm_net.stage1.rebnconv1.relu_s1"
    row = harness._TABLE["gm"]
    assert row.cross and not row.pad and row.kinds == ("full", "last12", "input") and not row.excluded
    assert not (row.deferred or row.autocast or row.channels_last)
    assert [c.name for c in harness._TABLE.values() if c.cross] == ["gm"]


def test_gm_rejections_before_any_sweep(tmp_path, oracle_ops):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in [{"deferred": True}, {"autocast": "fp16"}, {"autocast": "bf16"}, {"channels_last": True}]:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), criterion="gm", **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


def test_cli_gm_flags():
    import importance_generation as ig
    a = ig.parse_args(["--net", "resnet_56", "--criterion", "gm", "--synthetic", "--limit", "1"])
    assert (a.criterion, a.limit) == ("gm", 1)
    assert ig.parse_args(["--net", "u2netp", "--criterion", "gm", "--single_sweep"]).net == "u2netp"
    for extra in (["--deferred"], ["--autocast", "fp16"], ["--channels_last"]):
        with pytest.raises(SystemExit) as e:
            ig.main(["--net", "resnet_56", "--criterion", "gm", "--synthetic"] + extra)  # exits in the parser
        assert e.value.code == 2
    assert ig.parse_args(["--net", "resnet_56"]).criterion == "dct"
    assert "gm_score/" in ig.__doc__
