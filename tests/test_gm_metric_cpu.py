"""The normalised metrics of the geometric-median criterion without a GPU: the two new C entry points (declared, bound,
exported, argument codes and their order, the size query), the oracle's own properties (tests/gm_metric_oracle.py),
imp_score(criterion="gm", gm_metric=...) with the oracle in the kernel's place, the rejections, the CLI and the mask tool."""
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import gm_metric_oracle as mo
import gm_oracle as go
from dct_pruning_amd import _lib, harness, masks, nets, ops, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

L2, COSINE, CORRELATION = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_metric_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    head = text[:text.index("#define DCTS_ABI_VERSION")]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dcts_gm_distance_metric_f32", "dcts_gm_workspace_bytes"):
        assert name in head, "%s not listed among the additions to ABI 3" % name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    for name, value in (("DCTS_GM_L2", L2), ("DCTS_GM_COSINE", COSINE), ("DCTS_GM_CORRELATION", CORRELATION)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert ops.GM_METRICS == {"l2": L2, "cosine": COSINE, "correlation": CORRELATION}
    plain = re.search(r"int dcts_gm_distance_f32\((.*?)\);", text, re.S).group(1)
    proto = re.search(r"int dcts_gm_distance_metric_f32\((.*?)\);", text, re.S).group(1)
    strip = lambda s: re.sub(r"\s+", " ", s).strip()
    assert strip(proto) == strip(plain) + ", int32_t metric, void* workspace, size_t workspace_bytes"
    assert _lib.SIGNATURES["dcts_gm_distance_metric_f32"][1] == _lib.SIGNATURES["dcts_gm_distance_f32"][1] + [
        ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t]
    assert _lib.SIGNATURES["dcts_gm_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                                           ctypes.c_int32])


def test_metric_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, rb=0, rc=4, out=fake, metric=COSINE, ws=fake,
             nbytes=1 << 20):
        return lib.dcts_gm_distance_metric_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, rb, rc, out, None, metric, ws, nbytes)

    for m in (L2, COSINE, CORRELATION, 7):  # what dcts_gm_distance_f32 checks, whatever the metric
        assert call(x=None, metric=m) == -1 and call(out=None, metric=m) == -1
        assert call(n=0, metric=m) == -2 and call(h=513, w=513, sh=513, metric=m) == -2
        assert call(cb=2, cc=3, metric=m) == -3 and call(rc=0, metric=m) == -3 and call(rb=4, rc=1, metric=m) == -3
        assert call(sw=2, metric=m) == -4 and call(sh=4, metric=m) == -4
        assert call(sh=12, sc=96, sn=384, metric=m) == -6
        assert call(x=0x1001, metric=m) == -7 and call(out=0x1002, metric=m) == -7
        assert call(x=None, h=0, metric=m) == -1 and call(h=0, cc=0, metric=m) == -2 and call(rc=0, sw=2, metric=m) == -3
        assert call(sw=2, x=0x1001, metric=m) == -4 and call(sh=12, x=0x1001, metric=m) == -7
    # then the metric, then the workspace
    for m in (-1, 3, 7, 1 << 20):
        assert call(metric=m) == -6 and call(metric=m, ws=None, nbytes=0) == -6 and call(metric=m, ws=0x1004) == -6
        assert call(metric=m, x=0x1001) == -7 and call(metric=m, sw=2) == -4  # the tensor's checks come first
    for m in (COSINE, CORRELATION):
        need = lib.dcts_gm_workspace_bytes(m, 1, 4, 4)
        assert call(metric=m, ws=None) == -5 and call(metric=m, ws=None, nbytes=0) == -5
        assert call(metric=m, nbytes=need - 1) == -5 and call(metric=m, nbytes=0) == -5
        assert call(metric=m, ws=0x1004) == -7 and call(metric=m, ws=0x1008, nbytes=0) == -7  # alignment before size
        assert call(metric=m, ws=None, cb=2, cc=3) == -3 and call(metric=m, ws=None, sh=12, sc=96, sn=384) == -6


def test_workspace_size_query():
    lib = _lib.load()
    q = lib.dcts_gm_workspace_bytes
    for args in ((1, 1, 1), (4, 64, 64), (256, 2048, 2048)):
        assert q(L2, *args) == 0 and q(5, *args) == 0 and q(-1, *args) == 0
    for m in (COSINE, CORRELATION):
        assert q(m, 0, 4, 4) == 0 and q(m, 1, 0, 4) == 0 and q(m, 1, 4, 0) == 0
        assert q(m, 1, 1, 1) >= 16 and q(m, 1, 1, 1) % 16 == 0
        last = 0
        for n, c, r in ((1, 1, 1), (1, 4, 4), (2, 4, 4), (2, 64, 4), (2, 64, 200), (256, 2048, 2048)):
            got = q(m, n, c, r)
            assert got >= 8 * n * (c + r) and got >= last, (n, c, r)  # a (mu, s) pair per scored and per reference map
            last = got
    assert q(COSINE, 3, 7, 9) == q(CORRELATION, 3, 7, 9)


def test_ops_reject_an_unknown_metric_before_anything_else():
    for bad in ("L2", "euclid", None, 1):
        with pytest.raises(ValueError, match="metric"):
            ops.gm_distance_nc(torch.zeros(1, 2, 8, 8), metric=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gm_distance_nc(torch.zeros(1, 2, 8, 8), metric="cosine")


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def _zero(d):
    return (d == 0).all() and not np.signbit(d).any()


@pytest.mark.parametrize("metric", mo.METRICS)
def test_oracle_exact_properties(metric):
    x = go.maps(2, 9, 5, 7, 11)  # channel 1 zero, channel 8 a copy of channel 0
    x[:, 3] = x[:, 2] * 2.0 ** 10
    x[:, 4] = x[:, 2] * 2.0 ** -9
    x[:, 5] = 0.1 if metric == "correlation" else 0.0
    fs = (lambda *a: mo.gm_metric_nc_f64(x, metric, *a), lambda *a: mo.gm_metric_nc_f32(x, metric, *a))
    for f in fs:
        assert _zero(f(0, 1, 8, 1))                                  # a duplicate
        assert _zero(f(2, 1, 3, 1)) and _zero(f(2, 1, 4, 1)) and _zero(f(3, 1, 4, 1))  # power-of-two multiples
        for k in range(9):
            assert _zero(f(k, 1, k, 1))                              # the k == c term
        assert _zero(f(1, 1, 5, 1)) and _zero(f(5, 1, 1, 1))         # two flat maps
        for j, k in ((0, 3), (2, 7), (1, 4), (8, 0), (5, 6)):
            np.testing.assert_array_equal(f(j, 1, k, 1), f(k, 1, j, 1))  # symmetric, bit for bit
        full = f()
        np.testing.assert_array_equal(full[:, 1], full[:, 5])        # a zero map and a constant map score alike
        np.testing.assert_array_equal(full[:, 0], full[:, 8])
        np.testing.assert_array_equal(np.concatenate([f(0, 1), f(1, 5), f(6, 3)], axis=1), full)
        assert (full >= 0).all() and (full <= 2 * 9).all()
    # a flat map is at distance 1 from every map that is not flat
    np.testing.assert_allclose(fs[0](1, 1, 6, 2), 2.0, rtol=1e-14)
    np.testing.assert_allclose(fs[1](1, 1, 6, 2), 2.0, rtol=1e-6)
    u = mo.staged_f32(x, metric).numpy()
    assert (u[:, 1].view(np.int32) == 0).all() and (u[:, 5].view(np.int32) == 0).all()  # +0.0 in every element


def test_oracle_known_answers():
    k = torch.zeros(1, 3, 2, 2)
    k[0, 0, 0, 0], k[0, 1, 0, 1], k[0, 2, 1, 0] = 3.0, 0.5, 7.0  # orthogonal maps: sqrt(2) per pair under the cosine
    np.testing.assert_allclose(mo.gm_metric_nc_f64(k, "cosine")[0], [2 * 2 ** 0.5] * 3, rtol=1e-15)
    np.testing.assert_allclose(mo.gm_metric_nc_f32(k, "cosine")[0], [2 * 2 ** 0.5] * 3, rtol=1e-6)
    x = torch.randn(1, 2, 4, 5, generator=torch.Generator().manual_seed(5))
    x[0, 1] = -x[0, 0]  # rho = -1: d = 2
    np.testing.assert_allclose(mo.gm_metric_nc_f64(x, "correlation")[0], [2.0, 2.0], rtol=1e-14)
    np.testing.assert_allclose(mo.gm_metric_nc_f32(x, "correlation")[0], [2.0, 2.0], rtol=1e-6)
    # 2 - 2 rho against numpy's own correlation coefficient
    y = torch.randn(1, 2, 6, 6, generator=torch.Generator().manual_seed(6))
    rho = np.corrcoef(y[0, 0].numpy().ravel().astype(np.float64), y[0, 1].numpy().ravel().astype(np.float64))[0, 1]
    np.testing.assert_allclose(mo.gm_metric_nc_f64(y, "correlation", 0, 1, 1, 1)[0, 0], (2 - 2 * rho) ** 0.5, rtol=1e-12)
    # the stats order does not depend on the batch or on the channel range: a map alone gives its pair
    z = go.maps(3, 6, 9, 9, 8)
    mu, s = mo.stats_f32(z, "correlation")
    mu1, s1 = mo.stats_f32(z[2:3, 4:5], "correlation")
    assert mu1[0, 0] == mu[2, 4] and s1[0, 0] == s[2, 4]
    assert mo.gm_metric_nc(z, metric="l2").equal(go.gm_nc(z))


@pytest.mark.parametrize("metric", mo.METRICS)
def test_tolerance_is_eight_times_the_measured_restatement_error(metric):
    """The constants in gm_metric_oracle.py against a fresh measurement on the small inputs (H * W <= 64) and the 72 x 72
    case, which sets the correlation's."""
    assert mo.TOL[metric] == 8 * mo.R[metric] and 1e-7 < mo.R[metric] < 1e-5
    worst = max(mo.measure(metric, small_only=True), mo.restatement_error(mo.loop_case(), metric))
    assert mo.R[metric] / 4 <= worst <= 2 * mo.R[metric], worst


# ---------------------------------------------------------------------------------------------------------
# harness, mask tool, CLI
# ---------------------------------------------------------------------------------------------------------
def _run(name, root, **kw):
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
            harness.imp_score(net, args, train_loader=loader, criterion="gm", **kw)
    finally:
        os.chdir(cwd)
    dirs = sorted(os.listdir(os.path.join(str(root), "gm_score")))
    assert len(dirs) == 1, dirs
    d = os.path.join(str(root), "gm_score", dirs[0])
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}, buf.getvalue().splitlines(), d


def _activations(name):
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
def metric_oracle(monkeypatch):
    monkeypatch.setattr(harness, "_gm_nc", mo.gm_metric_nc)


@pytest.fixture
def plain_oracle(monkeypatch):
    monkeypatch.setattr(harness, "_gm_nc", go.gm_nc)  # has no `metric` keyword: gm_metric="l2" must not pass one


@pytest.mark.parametrize("name,metric", [("resnet_56", "cosine"), ("densenet_40", "correlation")])
def test_imp_score_gm_metric(name, metric, tmp_path, metric_oracle):
    got, lines, d = _run(name, tmp_path / "m", gm_metric=metric, single_sweep=True)
    assert d.endswith(os.path.join("gm_score", "%s_limit1_%s" % (name, metric)))
    assert "Importance Score is located at ./gm_score/%s_limit1_%s" % (name, metric) in lines
    pts, seen = _activations(name)
    assert sorted(got) == sorted("gm_" + s[len("imp_"):] for p in pts for s, _, _ in p.files)
    kinds = set()
    for p in pts:
        x = seen[p.module]
        C = x.shape[1]
        cb, cc = (C - 12, 12) if p.kind == "last12" else (0, C)
        want = mo.gm_metric_nc_f64(x, metric, cb, cc, cb, cc).mean(axis=0)
        kinds.add(p.kind)
        for stem, lo, hi in p.files:
            v = got["gm_" + stem[len("imp_"):]]
            ref = want if lo is None else want[lo:hi]
            assert v.dtype == np.float32 and v.shape == ref.shape, stem
            np.testing.assert_allclose(v, ref, rtol=1e-6, atol=1e-6, err_msg=stem)
    assert kinds == ({"full", "last12"} if name == "densenet_40" else {"full"})
    for k, v in got.items():
        raw = open(os.path.join(d, k + ".npy"), "rb").read()
        assert raw[:8] == b"\x93NUMPY\x01\x00" and b"'descr': '<f4'" in raw[:128] and len(raw) == 128 + 4 * v.size, k
    # the mask tool reads the directory as any directory of per-channel scores
    m = masks.masks_for_dir(d, 0.5)
    assert sorted(m) == sorted(got)
    for k, v in m.items():
        c = got[k].shape[0]
        np.testing.assert_array_equal(v, orc.select_index(got[k], c, orc.kept_filters(c, 0.5)))


def test_l2_writes_what_gm_writes_and_the_setting_does_not_leak(tmp_path, monkeypatch):
    seen = []

    def spy(x, **kw):
        seen.append(kw.get("metric"))
        return mo.gm_metric_nc(x, **kw)

    monkeypatch.setattr(harness, "_gm_nc", spy)
    cos, _, d_cos = _run("resnet_56", tmp_path / "cos", gm_metric="cosine", single_sweep=True)
    assert set(seen) == {"cosine"} and harness._gm_metric == "cosine"
    del seen[:]
    monkeypatch.setattr(harness, "_gm_nc", go.gm_nc)  # no `metric` keyword: the default must not name one
    plain, lines_p, d_plain = _run("resnet_56", tmp_path / "plain", single_sweep=True)  # after a cosine run: no leak
    assert harness._gm_metric == "l2"
    l2, lines_l, d_l2 = _run("resnet_56", tmp_path / "l2", gm_metric="l2", single_sweep=True)
    assert d_plain.endswith("resnet_56_limit1") and d_l2.endswith("resnet_56_limit1") and lines_p == lines_l
    assert sorted(plain) == sorted(l2) == sorted(cos)
    for k in plain:
        assert open(os.path.join(d_plain, k + ".npy"), "rb").read() == open(os.path.join(d_l2, k + ".npy"), "rb").read(), k
    assert any(not np.allclose(plain[k], cos[k], rtol=1e-3) for k in plain)


@pytest.mark.parametrize("kind,C", [("full", 24), ("last12", 24), ("input", 24)])
def test_point_hook_in_channel_ranges_equals_the_unsplit_one(kind, C, metric_oracle, monkeypatch):
    monkeypatch.setattr(harness, "_gm_metric", "correlation")
    x = go.maps(2, C, 6, 5, 21)
    base, count = (C - 12, 12) if kind == "last12" else (0, C)
    whole = harness._PointHook(kind, "host", torch.device("cpu"), key="w", criterion="gm")
    split = harness._PointHook(kind, "host", torch.device("cpu"), ranges=[("a", 0, 5), ("b", 5, count)], nominal_c=count,
                               criterion="gm")
    for hook in (whole, split):
        hook(None, (x,), x)
    want = mo.gm_metric_nc_f64(x, "correlation", base, count, base, count).mean(axis=0).astype(np.float32)
    np.testing.assert_allclose(whole.scores("w"), want, rtol=1e-6)
    np.testing.assert_array_equal(np.concatenate([split.scores("a"), split.scores("b")]), whole.scores("w"))


def test_table_row_and_rejections_before_any_sweep(tmp_path, plain_oracle):
    assert len(harness._TABLE) == 5 and [c.name for c in harness._TABLE.values() if c.cross] == ["gm"]
    assert harness._TABLE["gm"].metrics == ("l2", "cosine", "correlation")
    assert all(c.metrics == () for c in harness._TABLE.values() if c.name != "gm")

    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cases = [dict(criterion=c, gm_metric=m) for c in ("dct", "rank", "bands", "entropy") for m in ("cosine", "correlation")]
    cases += [dict(criterion="gm", gm_metric=m) for m in ("euclid", "L2", None)]
    cases += [dict(criterion="gm", gm_metric="cosine", **kw)
              for kw in ({"deferred": True}, {"autocast": "fp16"}, {"autocast": "bf16"}, {"channels_last": True})]
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in cases:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), **kw)
            with pytest.raises(ValueError):
                harness.check_options(kw["criterion"], "resnet_56", kw.get("deferred", False), kw.get("autocast"),
                                      kw.get("channels_last", False), gm_metric=kw["gm_metric"])
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []
    for c in harness.CRITERIA:
        harness.check_options(c, "resnet_56", gm_metric="l2")  # the default goes with every criterion
    harness.check_options("gm", "u2netp", gm_metric="correlation")


def test_cli_gm_metric_flag():
    import importance_generation as ig
    base = ["--net", "resnet_56", "--synthetic", "--limit", "1"]
    assert ig.parse_args(base).gm_metric == "l2" and ig.parse_args(base + ["--criterion", "gm"]).gm_metric == "l2"
    for m in ("l2", "cosine", "correlation"):
        assert ig.parse_args(base + ["--criterion", "gm", "--gm_metric", m]).gm_metric == m
    assert ig.parse_args(base + ["--criterion", "entropy", "--gm_metric", "l2"]).criterion == "entropy"
    bad = [["--criterion", "gm", "--gm_metric", "euclid"], ["--gm_metric", "cosine"],
           ["--criterion", "rank", "--gm_metric", "correlation"], ["--criterion", "bands", "--gm_metric", "cosine"],
           ["--criterion", "gm", "--gm_metric", "cosine", "--deferred"],
           ["--criterion", "gm", "--gm_metric", "cosine", "--autocast", "fp16"],
           ["--criterion", "gm", "--gm_metric", "correlation", "--channels_last"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            ig.main(base + extra)  # exits in the parser
        assert e.value.code == 2, extra
    assert "--gm_metric" in ig.__doc__ and "_<metric>" in ig.__doc__


def test_masks_cli_on_a_cosine_directory(tmp_path, metric_oracle):
    got, _, d = _run("resnet_56", tmp_path / "m", gm_metric="cosine", single_sweep=True)
    assert d.endswith("_cosine")
    out = str(tmp_path / "m.npz")
    assert masks.main(["--imp_score", d, "--compress_rate", "[0.5]*%d" % len(got), "--out", out]) == 0
    assert sorted(np.load(out).files) == sorted(got)
