"""The pair matrix of the geometric-median criterion without a GPU: the three C entry points (declared, bound, exported,
argument codes and their order, the slice rule, the size query), the oracle's own properties (tests/gm_pairs_oracle.py), the
selection rules of dct_pruning_amd/pairs.py and the mask tool's --pair_rule, and imp_score(criterion="gm", gm_pairs=True) with
the oracle in the kernel's place: files and shapes, values, schedules and accumulator forms, channel ranges, rejections, the
CLI and the sharded runs."""
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dct_pruning_amd as dpa
import gm_oracle as go
import gm_pairs_oracle as po
from dct_pruning_amd import _lib, accumulate, harness, masks, nets, ops, pairs, schedules, sharding
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init

L2, COSINE, CORRELATION = 0, 1, 2
NAMES = ("dcts_gm_pairs_f32", "dcts_gm_pairs_workspace_bytes", "dcts_gm_pairs_slices")


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3 and _lib.load().dcts_version() == 3
    head = text[:text.index("#define DCTS_ABI_VERSION")]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in head, "%s not listed among the additions to ABI 3" % name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    strip = lambda s: re.sub(r"\s+", " ", s).strip()
    metric = re.search(r"int dcts_gm_distance_metric_f32\((.*?)\);", text, re.S).group(1)
    proto = re.search(r"int dcts_gm_pairs_f32\((.*?)\);", text, re.S).group(1)
    assert strip(proto) == strip(metric).replace("float* out_nc", "float* out_cr")
    assert _lib.SIGNATURES["dcts_gm_pairs_f32"] == _lib.SIGNATURES["dcts_gm_distance_metric_f32"]
    assert _lib.SIGNATURES["dcts_gm_pairs_workspace_bytes"] == _lib.SIGNATURES["dcts_gm_workspace_bytes"]
    assert _lib.SIGNATURES["dcts_gm_pairs_slices"] == (ctypes.c_int32, [ctypes.c_int64, ctypes.c_int32])
    assert "gm_pair_matrix" in dpa.__all__ and dpa.gm_pair_matrix is ops.gm_pair_matrix
    assert harness._gm_pairs_nc is ops.gm_pair_matrix
    mk = open(os.path.join(repo_root, "dct_pruning_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS = .*\bgm_pairs\b", mk, re.M) and re.search(r"^single:.*\n.*\bgm_pairs\.hip\b", mk, re.M)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, rb=0, rc=4, out=fake, metric=COSINE, ws=fake,
             nbytes=1 << 20):
        return lib.dcts_gm_pairs_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, rb, rc, out, None, metric, ws, nbytes)

    for m in (L2, COSINE, CORRELATION, 7):  # what dcts_gm_distance_f32 checks, in its order, whatever the metric
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
    for m in (COSINE, CORRELATION):  # one sample: one slice, the workspace is the pairs alone
        need = lib.dcts_gm_pairs_workspace_bytes(m, 1, 4, 4)
        assert need == lib.dcts_gm_workspace_bytes(m, 1, 4, 4) > 0
        assert call(metric=m, ws=None) == -5 and call(metric=m, ws=None, nbytes=0) == -5
        assert call(metric=m, nbytes=need - 1) == -5 and call(metric=m, nbytes=0) == -5
        assert call(metric=m, ws=0x1004) == -7 and call(metric=m, ws=0x1008, nbytes=0) == -7  # alignment before size
        assert call(metric=m, ws=None, cb=2, cc=3) == -3 and call(metric=m, ws=None, sh=12, sc=96, sn=384) == -6
    # the plain distance needs a workspace as soon as there is more than one slice
    assert lib.dcts_gm_pairs_slices(3, 4) == 3
    need = lib.dcts_gm_pairs_workspace_bytes(L2, 3, 4, 4)
    assert need >= 3 * 4 * 4 * 4
    kw = dict(n=3, sn=256, metric=L2)
    assert call(ws=None, **kw) == -5 and call(ws=None, nbytes=0, **kw) == -5 and call(nbytes=need - 1, **kw) == -5
    assert call(ws=0x1004, **kw) == -7 and call(ws=0x1008, nbytes=0, **kw) == -7
    assert call(ws=None, x=0x1001, **kw) == -7 and call(ws=None, cb=2, cc=3, **kw) == -3
    # a grid beyond 2^31 - 1 workgroups is refused with everything else in order, before any launch: 1024 slices x 2^22 scored
    # tiles x 1 reference tile; under a metric the stats grid as well (2^33 maps, four per workgroup)
    wide = dict(n=1024, c=1 << 28, h=1, w=1, sn=1 << 28, sc=1, sh=1, cc=1 << 28, rc=64, nbytes=1 << 62)
    assert lib.dcts_gm_pairs_slices(1024, 64) == 1024
    assert call(metric=L2, **wide) == -2 and call(metric=COSINE, **wide) == -2
    assert call(metric=L2, **dict(wide, ws=None)) == -5 and call(metric=7, **wide) == -6  # after the metric and the workspace
    many = dict(n=1 << 33, c=4096, h=1, w=1, sn=4096, sc=1, sh=1, cc=4096, rc=4096, nbytes=1 << 62)
    assert lib.dcts_gm_pairs_slices(1 << 33, 4096) == 1 and call(metric=CORRELATION, **many) == -2


def test_slices_and_workspace_size_queries():
    lib = _lib.load()
    s, q = lib.dcts_gm_pairs_slices, lib.dcts_gm_pairs_workspace_bytes
    assert s(0, 4) == 0 and s(-1, 4) == 0 and s(4, 0) == 0 and s(4, -3) == 0
    for n in (1, 2, 3, 5, 7, 64, 70, 71, 255, 256, 1000, 1 << 20, 1 << 40):
        for r in (1, 3, 64, 65, 128, 129, 200, 512, 2047, 2048, 2049, 4096, 1 << 20):
            got = s(n, r)
            assert got == po.slices(n, r) and 1 <= got <= n, (n, r, got)
            per = -(-n // got)
            assert (got - 1) * per < n <= got * per, (n, r, got)  # no empty slice, every sample in one
            assert got <= max(1, po.PAIR_TARGET // (-(-r // 64)) ** 2)
            if r <= 4096 and n <= 1 << 20:
                # the partial matrices of a square layer stay within 64 MiB (+ one 256-byte round-up)
                assert q(L2, n, r, r) <= (64 << 20) + 256, (n, r)
    # the rule at the shapes the docs and the GPU tests name
    assert s(5, 3) == 5 and s(1025, 65) == 513 and s(1024, 65) == 1024 and s(2, 2945) == 1 and s(256, 64) == 256
    assert s(256, 2048) == 4 and s(256, 1024) == 16 and s(256, 4096) == 1
    for args in ((1, 1, 1), (2, 2945, 2945), (256, 4096, 4096), (1, 64, 64)):
        assert s(args[0], args[2]) == 1 and q(L2, *args) == 0  # one slice, no metric: no workspace
        for m in (COSINE, CORRELATION):
            assert q(m, *args) == lib.dcts_gm_workspace_bytes(m, *args) > 0
    for m in (L2, COSINE, CORRELATION):
        assert q(m, 0, 4, 4) == 0 and q(m, 1, 0, 4) == 0 and q(m, 1, 4, 0) == 0
        for n, c, r in ((3, 4, 4), (5, 3, 3), (71, 200, 200), (71, 10, 200), (256, 64, 64)):
            got, S = q(m, n, c, r), s(n, r)
            assert S > 1 and got % 16 == 0
            assert got >= lib.dcts_gm_workspace_bytes(m, n, c, r) + 4 * S * c * r, (m, n, c, r)
    for bad in (-1, 3, 5, 1 << 20):
        assert q(bad, 4, 4, 4) == 0
    assert q(COSINE, 3, 7, 9) == q(CORRELATION, 3, 7, 9) > q(L2, 3, 7, 9) > 0


def test_ops_rejections_before_any_launch():
    for bad in ("L2", "euclid", None, 1):
        with pytest.raises(ValueError, match="metric"):
            ops.gm_pair_matrix(torch.zeros(1, 2, 8, 8), metric=bad)
    with pytest.raises(TypeError, match="float32"):
        ops.gm_pair_matrix(torch.zeros(1, 2, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="N, C, H, W"):
        ops.gm_pair_matrix(torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gm_pair_matrix(torch.zeros(1, 2, 8, 8), metric="cosine")


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def _zero(d):
    return (d == 0).all() and not np.signbit(d).any()


@pytest.mark.parametrize("metric", po.METRICS)
def test_oracle_exact_properties(metric):
    x = go.maps(5, 9, 5, 7, 11)  # channel 1 zero, channel 8 a copy of channel 0
    x[:, 3] = x[:, 2] * 2.0 ** 10
    x[:, 5] = 0.1 if metric == "correlation" else 0.0
    assert po.slices(5, 9) == 5
    for f in (lambda *a: po.pair_matrix_f64(x, metric, *a), lambda *a: po.pair_matrix_f32(x, metric, *a)):
        full = f()
        assert full.shape == (9, 9) and _zero(np.diag(full)) and _zero(full[0, 8]) and _zero(full[8, 0]) and _zero(full[1, 5])
        assert full.tobytes() == full.T.copy().tobytes()  # symmetric, bit for bit
        if metric != "l2":
            assert _zero(full[2, 3])  # a power-of-two multiple
        np.testing.assert_array_equal(np.concatenate([f(0, 1), f(1, 5), f(6, 3)], axis=0), full)
        np.testing.assert_array_equal(f(2, 4, 3, 5), full[2:6, 3:8])
        assert _zero(po.pair_matrix_f32(torch.zeros(3, 4, 2, 3), metric))
    # the sum over the samples of gm_oracle's definition, and its row sums are gm's scores summed over the samples
    np.testing.assert_array_equal(po.pair_matrix_f64(x, "l2"), go.pair_distances_f64(x).sum(0))
    np.testing.assert_allclose(po.pair_matrix_f64(x, "l2").sum(1), go.gm_nc_f64(x).sum(0), rtol=1e-14)
    # the slice order is part of the restatement: one slice and five differ in rounding only
    one = po.pair_matrix_f32(x, metric, bounds=[(0, 5)])
    np.testing.assert_allclose(one, po.pair_matrix_f32(x, metric), rtol=1e-6, atol=1e-6)
    assert po.slice_bounds(1025, 65)[-1] == (1024, 1025) and len(po.slice_bounds(1025, 65)) == 513
    assert po.slice_bounds(5, 3) == [(n, n + 1) for n in range(5)] and po.slice_bounds(2, 2945) == [(0, 2)]


@pytest.mark.parametrize("metric", po.METRICS)
def test_tolerance_is_eight_times_the_measured_restatement_error(metric):
    """The constants in gm_pairs_oracle.py against a fresh measurement on the inputs small enough for a unit test, the cases
    the one that sets all three constants ("ragged") among them."""
    assert po.TOL[metric] == 8 * po.R[metric] and 1e-7 < po.R[metric] < 1e-5
    worst = max(po.restatement_error(po.regime_case("ragged"), metric), po.restatement_error(po.sweep_case(200, (15, 17)), metric),
                po.restatement_error(po.duplicate_case(), metric))
    assert po.R[metric] / 4 <= worst <= po.R[metric] * 1.001, worst
    names = [n for n, _, _ in po.gpu_inputs()]
    assert len(names) == len(set(names)) == 27 + 3 + 5
    assert {s for _, s in po.SWEEP} == set(po.SIZES) and all(sum(1 for c, _ in po.SWEEP if c == k) == 3 for k in po.CHANNELS)
    assert po.ZERO_SAMPLE_CASE in po.SWEEP and not po.sweep_case(*po.ZERO_SAMPLE_CASE)[1].any()


# ---------------------------------------------------------------------------------------------------------
# pairs.py and the mask tool
# ---------------------------------------------------------------------------------------------------------
def _keep(imp, rate):
    c = imp.shape[0]
    return masks.select_index(imp, c, int(c * (1 - rate)))


def test_duplicates_example_sum_keeps_pairs_kcenter_keeps_patterns():
    D = po.pair_matrix_f64(po.duplicate_case())  # 12 channels: 6 patterns, channel i + 6 a copy of channel i
    assert _keep(pairs.score(D, "sum"), 0.5).tolist() == [0, 3, 4, 6, 9, 10]  # three patterns twice, three lost
    kept = _keep(pairs.score(D, "kcenter"), 0.5)
    assert kept.size == 6 and sorted(k % 6 for k in kept) == list(range(6))  # one copy of each
    assert kept.tolist() == [0, 1, 2, 3, 4, 5]  # ties to the lowest index
    assert (pairs.score(D, "nn") == 0).all()  # every channel has a copy
    # the same from the float32 matrix a sweep writes
    assert _keep(pairs.score(D.astype(np.float32), "kcenter"), 0.5).tolist() == [0, 1, 2, 3, 4, 5]


def test_kcenter_masks_are_nested_over_rates():
    D = po.pair_matrix_f64(go.maps(3, 20, 4, 4, 77))
    imp = pairs.score(D, "kcenter")
    assert imp.dtype == np.float32 and sorted(imp.tolist()) == list(range(1, 21))
    order = pairs.kcenter_order(D)
    assert imp[order].tolist() == list(range(20, 0, -1)) and order[0] == np.argmax(D.sum(1))
    last = set()
    for rate in (0.9, 0.7, 0.5, 0.3, 0.1):
        kept = _keep(imp, rate)
        assert set(kept.tolist()) == set(order[:kept.size].tolist()) and last <= set(kept.tolist())
        last = set(kept.tolist())
    # farthest point: the t-th one is the unselected channel farthest from the ones before it
    for t in range(1, 20):
        mind = D[:, order[:t]].min(axis=1)
        mind[order[:t]] = -1
        assert mind[order[t]] == mind.max()


def test_known_answers_and_ties():
    D = np.array([[0, 1, 4, 6], [1, 0, 2, 5], [4, 2, 0, 3], [6, 5, 3, 0]], dtype=np.float32)
    assert pairs.score(D, "sum").tolist() == [11, 8, 9, 14]
    assert pairs.score(D, "nn").tolist() == [1, 1, 2, 3]
    # first 3 (sum 14); mind = [6, 5, 3, 0] -> 0; mind = [0, 1, 3, 0] -> 2; then 1
    assert pairs.kcenter_order(D).tolist() == [3, 0, 2, 1] and pairs.score(D, "kcenter").tolist() == [3, 1, 2, 4]
    for rule in pairs.RULES:
        assert pairs.score(D, rule).dtype == np.float32
    # every tie to the lowest index: equal row sums, equal distances
    T = np.ones((5, 5)) - np.eye(5)
    assert pairs.kcenter_order(T).tolist() == [0, 1, 2, 3, 4] and pairs.score(T, "kcenter").tolist() == [5, 4, 3, 2, 1]
    Z = np.zeros((3, 3))
    assert pairs.kcenter_order(Z).tolist() == [0, 1, 2]
    one = np.zeros((1, 1), np.float32)
    assert pairs.score(one, "nn").tolist() == [0] and pairs.score(one, "kcenter").tolist() == [1] and pairs.score(one, "sum").tolist() == [0]
    # float64 arithmetic on the float32 file, rounded once
    big = np.array([[0, 1e8, 1], [1e8, 0, 1], [1, 1, 0]], dtype=np.float32)
    assert pairs.score(big, "sum")[0] == np.float32(1e8 + 1.0)
    for bad in (np.zeros((3, 4)), np.zeros(4), np.zeros((2, 2, 2))):
        for rule in pairs.RULES:
            with pytest.raises(ValueError, match="square"):
                pairs.score(bad, rule)
    with pytest.raises(ValueError, match="rule"):
        pairs.score(D, "median")


def test_pairs_cli_file_names_and_masks_pair_rule(tmp_path):
    src, dst = tmp_path / "m", tmp_path / "out"
    src.mkdir()
    mats = {"gm_conv1": po.pair_matrix_f64(po.duplicate_case()).astype(np.float32),
            "gm_conv2_n3x3": po.pair_matrix_f64(go.maps(2, 8, 3, 3, 5)).astype(np.float32),
            "gm_net.stage1.rebnconv1.relu_s1": po.pair_matrix_f64(go.maps(2, 5, 3, 3, 6)).astype(np.float32)}
    for k, v in mats.items():
        np.save(str(src / (k + ".npy")), v)
    assert pairs.score_file_name("gm_conv3.npy") == "imp_conv3.npy"
    assert pairs.score_file_name("gm_net.stage1.rebnconv1.relu_s1.npy") == "net.stage1.rebnconv1.relu_s1.npy"
    for rule in pairs.RULES:
        d = dst / rule
        assert pairs.main(["--matrix", str(src), "--rule", rule, "--out", str(d)]) == 0
        assert sorted(os.listdir(str(d))) == ["imp_conv1.npy", "imp_conv2_n3x3.npy", "net.stage1.rebnconv1.relu_s1.npy"]
        for k, v in mats.items():
            got = np.load(str(d / pairs.score_file_name(k + ".npy")))
            assert got.dtype == np.float32 and got.shape == (v.shape[0],)
            assert got.tobytes() == pairs.score(v, rule).tobytes()
        # the mask tool on the matrices under --pair_rule is the mask tool on the scores
        a, b = str(tmp_path / ("a_%s.npz" % rule)), str(tmp_path / ("b_%s.npz" % rule))
        assert masks.main(["--imp_score", str(src), "--compress_rate", "[0.5]*3", "--pair_rule", rule, "--out", a]) == 0
        assert masks.main(["--imp_score", str(d), "--compress_rate", "[0.5]*3", "--out", b]) == 0
        za, zb = np.load(a), np.load(b)
        assert sorted(za.files) == sorted(zb.files) == ["imp_conv1", "imp_conv2_n3x3", "net.stage1.rebnconv1.relu_s1"]
        for k in za.files:
            np.testing.assert_array_equal(za[k], zb[k])
        assert masks.compare(masks.masks_for_dir(str(src), 0.5, pair_rule=rule), masks.masks_for_dir(str(d), 0.5)) == []
    assert np.load(str(tmp_path / "a_kcenter.npz"))["imp_conv1"].tolist() == [0, 1, 2, 3, 4, 5]
    # without the flag a matrix directory is what it was before: a 2-D file without band weights
    with pytest.raises(masks.BandWeightsError):
        masks.masks_for_dir(str(src), 0.5)
    # a non-square file is an error, and nothing is written
    np.save(str(src / "gm_conv9.npy"), np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="square"):
        pairs.collapse(str(src), "sum", str(tmp_path / "never"))
    assert not (tmp_path / "never").exists()
    with pytest.raises(SystemExit) as e:
        pairs.main(["--matrix", str(src), "--rule", "nn", "--out", str(tmp_path / "never")])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        masks.main(["--imp_score", str(src), "--pair_rule", "kcenter"])
    with pytest.raises(SystemExit):
        pairs.main(["--matrix", str(src), "--rule", "median", "--out", str(tmp_path / "never")])
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no gm_"):
        pairs.collapse(str(empty), "sum", str(tmp_path / "never"))


# ---------------------------------------------------------------------------------------------------------
# harness
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
            harness.imp_score(net, args, train_loader=loader, criterion="gm", gm_pairs=True, **kw)
    finally:
        os.chdir(cwd)
    dirs = sorted(os.listdir(os.path.join(str(root), "gm_score")))
    assert len(dirs) == 1, dirs
    d = os.path.join(str(root), "gm_score", dirs[0])
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}, buf.getvalue().splitlines(), d


def _activations(name):
    """The hooked tensors of every batch of the sweep: {module: [x of batch 0, ...]}."""
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).eval()
    pts = schedules.SCHEDULES[name]()
    seen = {}
    handles = [harness._resolve(net, p.module).register_forward_hook(
        lambda m, i, o, _p=p: seen.setdefault(_p.module, []).append((i[0] if _p.kind == "input" else o).detach().clone()))
        for p in pts]
    (harness.u2netp_inference if name == "u2netp" else harness.inference)(
        net, SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict), limit)
    for h in handles:
        h.remove()
    return pts, seen


@pytest.fixture
def pair_oracle(monkeypatch):
    monkeypatch.setattr(harness, "_gm_pairs_nc", po.pair_matrix)

    def no_row_sums(*a, **kw):
        raise AssertionError("gm_pairs must not call the row-sum operator")

    monkeypatch.setattr(harness, "_gm_nc", no_row_sums)


def _check_files(name, got, metric):
    pts, seen = _activations(name)
    assert sorted(got) == sorted("gm_" + (s[len("imp_"):] if s.startswith("imp_") else s) for p in pts for s, _, _ in p.files)
    kinds, sliced = set(), 0
    for p in pts:
        xs = seen[p.module]
        C = xs[0].shape[1]
        cb, cc = (C - 12, 12) if p.kind == "last12" else (0, C)
        total = sum(x.shape[0] for x in xs)
        want = sum(po.pair_matrix_f64(x, metric, cb, cc, cb, cc) for x in xs) / total  # the float64 mean over the samples
        kinds.add(p.kind)
        for stem, lo, hi in p.files:
            v = got["gm_" + (stem[len("imp_"):] if stem.startswith("imp_") else stem)]
            ref = want if lo is None else want[lo:hi, lo:hi]
            sliced += lo is not None
            assert v.dtype == np.float32 and v.shape == ref.shape and v.ndim == 2 and v.shape[0] == v.shape[1], stem
            np.testing.assert_allclose(v, ref, rtol=1e-6, atol=1e-6, err_msg=stem)
    return kinds, sliced


@pytest.mark.parametrize("name,metric,kw", [("densenet_40", "l2", {}), ("googlenet", "cosine", {"single_sweep": True}),
                                            ("vgg_16_bn", "correlation", {"single_sweep": True}), ("u2netp", "l2", {})])
def test_imp_score_gm_pairs_files_shapes_values(name, metric, kw, tmp_path, pair_oracle):
    got, lines, d = _run(name, tmp_path / "p", gm_metric=metric, **kw)
    limit = HARNESS_CASES[name][1]
    tail = "%s_limit%d%s_pairs" % (name, limit, "" if metric == "l2" else "_" + metric)
    assert d.endswith(os.path.join("gm_score", tail))
    assert "Importance Score is located at ./gm_score/" + tail in lines
    assert lines[-1] == "The importance score generation has been completed!"
    kinds, sliced = _check_files(name, got, metric)
    if name == "densenet_40":
        assert kinds == {"full", "last12"} and got["gm_conv1"].shape == (24, 24)
        assert got["gm_conv2"].shape == (12, 12)
    if name == "googlenet":
        assert sliced > 0 and got["gm_conv2_n3x3"].shape == (128, 128) and got["gm_conv1_"].shape == (192, 192)
    if name == "u2netp":
        assert "input" in kinds
        assert all(k.startswith("gm_net.") for k in got)
    if name == "vgg_16_bn":
        assert HARNESS_CASES[name][1] == 2  # two batches: the sum over the batches, divided once
    for k, v in got.items():
        raw = open(os.path.join(d, k + ".npy"), "rb").read()
        assert raw[:8] == b"\x93NUMPY\x01\x00" and b"'descr': '<f4'" in raw[:128] and len(raw) == 128 + 4 * v.size, k
        assert (np.diag(v) == 0).all()
    # the README's route: matrices -> pairs --rule kcenter -> masks
    out = str(tmp_path / "scores")
    assert pairs.main(["--matrix", d, "--rule", "kcenter", "--out", out]) == 0
    m = masks.masks_for_dir(out, 0.5)
    assert len(m) == len(got) and all(v.size == int(got["gm_" + k[len("imp_"):] if k.startswith("imp_") else "gm_" + k].shape[0] * 0.5)
                                       for k, v in m.items())


def test_schedules_and_accumulator_forms_give_identical_bytes(tmp_path, pair_oracle):
    name = "vgg_16_bn"  # two batches of four samples
    runs = {"per-hook": {}, "single": {"single_sweep": True}, "per-hook device": {"accumulate": "device"},
            "single device": {"single_sweep": True, "accumulate": "device"}}
    out = {k: _run(name, tmp_path / k.replace(" ", "_"), **kw) for k, kw in runs.items()}
    base, _, d0 = out["per-hook"]
    assert len(base) == 12
    for k, (got, _, d) in out.items():
        assert sorted(got) == sorted(base) and d.endswith("vgg_16_bn_limit2_pairs")
        for f in base:
            assert open(os.path.join(d, f + ".npy"), "rb").read() == open(os.path.join(d0, f + ".npy"), "rb").read(), (k, f)
    # the two forms of the accumulator on their own: the fp32 sum in batch order, divided once by the samples
    g = torch.Generator().manual_seed(3)
    mats = [torch.rand(5, 7, generator=g) * 100 for _ in range(4)]
    host, dev = accumulate.PairAccumulator(), accumulate.PairAccumulator(torch.device("cpu"))
    for m in mats:
        host.update(m, 3)
        dev.update(m, 3)
    want = ((((torch.zeros(5, 7) + mats[0]) + mats[1]) + mats[2]) + mats[3]) / 12.0
    assert host.scores().tobytes() == dev.scores().tobytes() == want.numpy().tobytes() and host.scores().dtype == np.float32
    with pytest.raises(ValueError):
        host.update(torch.zeros(5, 6), 1)


@pytest.mark.parametrize("kind,C", [("full", 24), ("last12", 24), ("input", 24)])
def test_point_hook_in_channel_ranges_equals_the_unsplit_one(kind, C, monkeypatch):
    calls = []

    def spy(x, **kw):
        calls.append((kw["c_begin"], kw["c_count"], kw["ref_begin"], kw["ref_count"], kw.get("metric")))
        return po.pair_matrix(x, **kw)

    monkeypatch.setattr(harness, "_gm_pairs_nc", spy)
    monkeypatch.setattr(harness, "_gm_metric", "correlation")
    xs = [go.maps(2, C, 6, 5, 21), go.maps(3, C, 6, 5, 22)]
    base, count = (C - 12, 12) if kind == "last12" else (0, C)
    whole = harness._PointHook(kind, "host", torch.device("cpu"), key="w", criterion="gm", pairs=True)
    split = harness._PointHook(kind, "host", torch.device("cpu"), ranges=[("a", 0, 5), ("b", 5, count)], nominal_c=count,
                               criterion="gm", pairs=True)
    for x in xs:
        whole(None, (x,), x)
    assert calls == [(base, count, base, count, "correlation")] * 2
    del calls[:]
    for x in xs:
        split(None, (x,), x)
    # every piece: its rows against the hook kind's whole channel set
    assert calls == [(base, 5, base, count, "correlation"), (base + 5, count - 5, base, count, "correlation")] * 2
    want = sum(po.pair_matrix_f64(x, "correlation", base, count, base, count) for x in xs) / 5.0
    w = whole.scores("w")
    assert w.shape == (count, count) and w.dtype == np.float32
    np.testing.assert_allclose(w, want, rtol=1e-6, atol=1e-6)
    a, b = split.scores("a"), split.scores("b")
    assert a.shape == (5, count) and b.shape == (count - 5, count)
    assert np.concatenate([a, b]).tobytes() == w.tobytes()

    # an operator that is not handed `ref` (the pieces scored against themselves) does not pass
    def self_ref(x, c_begin=0, c_count=None, ref_begin=0, ref_count=None, **kw):
        return po.pair_matrix(x, c_begin, c_count, c_begin, c_count, **kw)

    monkeypatch.setattr(harness, "_gm_pairs_nc", self_ref)
    broken = harness._PointHook(kind, "host", torch.device("cpu"), ranges=[("a", 0, 5), ("b", 5, count)], nominal_c=count,
                                criterion="gm", pairs=True)
    broken(None, (xs[0],), xs[0])
    assert broken.scores("a").shape != a.shape
    with pytest.raises(ValueError):
        harness._PointHook("full", "host", torch.device("cpu"), key="w", criterion="dct", pairs=True)


def test_rejections_before_any_sweep_and_the_table_is_unchanged(tmp_path, pair_oracle):
    assert len(harness._TABLE) == 5 and harness.CRITERIA == ("dct", "rank", "bands", "entropy", "gm")
    row = harness._TABLE["gm"]
    assert (row.root, row.prefix, row.cross, row.metrics, row.pad) == ("gm_score", "gm_", True, ("l2", "cosine", "correlation"), False)
    assert not (row.deferred or row.autocast or row.channels_last)

    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cases = [dict(criterion=c) for c in ("dct", "rank", "bands", "entropy")]
    cases += [dict(criterion="gm", **kw) for kw in ({"deferred": True}, {"autocast": "fp16"}, {"autocast": "bf16"},
                                                    {"channels_last": True}, {"gm_metric": "euclid"})]
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in cases:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), gm_pairs=True, **kw)
            with pytest.raises(ValueError):
                harness.check_options(kw["criterion"], "resnet_56", kw.get("deferred", False), kw.get("autocast"),
                                      kw.get("channels_last", False), gm_metric=kw.get("gm_metric", "l2"), gm_pairs=True)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError, match="gm_pairs"):
        harness.check_options("entropy", "resnet_56", gm_pairs=True)
    for c in harness.CRITERIA:
        harness.check_options(c, "resnet_56")  # the default goes with every criterion
        harness.check_options(c, "resnet_56", False, None, False, (4, "square"), "l2", False)  # the new keyword is the last
    for net in ("resnet_56", "u2netp", "googlenet"):
        for m in ("l2", "cosine", "correlation"):
            harness.check_options("gm", net, gm_metric=m, gm_pairs=True)


def test_cli_gm_pairs_flag():
    import importance_generation as ig
    base = ["--net", "resnet_56", "--synthetic", "--limit", "1"]
    assert ig.parse_args(base).gm_pairs is False and ig.parse_args(base + ["--criterion", "gm"]).gm_pairs is False
    assert ig.parse_args(base + ["--criterion", "gm", "--gm_pairs"]).gm_pairs is True
    a = ig.parse_args(base + ["--criterion", "gm", "--gm_pairs", "--gm_metric", "cosine", "--single_sweep", "--device_accumulate"])
    assert a.gm_pairs and a.gm_metric == "cosine" and a.single_sweep and a.device_accumulate
    bad = [["--gm_pairs"], ["--criterion", "dct", "--gm_pairs"], ["--criterion", "rank", "--gm_pairs"],
           ["--criterion", "bands", "--gm_pairs"], ["--criterion", "entropy", "--gm_pairs"],
           ["--criterion", "gm", "--gm_pairs", "--deferred"], ["--criterion", "gm", "--gm_pairs", "--autocast", "fp16"],
           ["--criterion", "gm", "--gm_pairs", "--channels_last"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            ig.main(base + extra)  # exits in the parser
        assert e.value.code == 2, extra
    assert "--gm_pairs" in ig.__doc__ and "_pairs" in ig.__doc__ and "dct_pruning_amd.pairs" in ig.__doc__
    assert "gm_pairs" in harness.__doc__ and "gm_pairs" in harness.imp_score.__doc__


# ---------------------------------------------------------------------------------------------------------
# sharded runs
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, name, out_root, kw):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sharding.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    torch.set_num_threads(2)  # CPU convolutions round differently at other thread counts; the single-process run uses 2 as well
    import gm_pairs_oracle
    from dct_pruning_amd import harness as h
    h._gm_pairs_nc = gm_pairs_oracle.pair_matrix
    d = os.path.join(out_root, "rank%d" % rank)
    os.makedirs(d)
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name))
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.chdir(d)
    with contextlib.redirect_stdout(io.StringIO()):
        h.imp_score(net, args, train_loader=loader, criterion="gm", gm_pairs=True, **kw)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("name,world,kw", [
    ("densenet_40", 2, {}),                       # whole hook points, one sweep each: 24 x 24 next to 12 x 12 matrices
    ("googlenet", 4, {"single_sweep": True}),     # channel-range units: rows [lo, hi) against the whole layer; sliced files
])
def test_gloo_worlds_equal_single_process(name, world, kw, tmp_path, pair_oracle):
    before = torch.get_num_threads()
    torch.set_num_threads(2)  # as the workers: the comparison is about the sharding, not about the thread split
    try:
        single, _, d1 = _run(name, tmp_path / "single", **kw)
    finally:
        torch.set_num_threads(before)
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, name, str(tmp_path), kw), nprocs=world, join=True)
    d0 = tmp_path / "rank0" / "gm_score" / os.path.basename(d1)
    got = sorted(os.listdir(str(d0)))
    assert got == sorted(k + ".npy" for k in single)
    for f in got:
        assert open(str(d0 / f), "rb").read() == open(os.path.join(d1, f), "rb").read(), f
    for r in range(1, world):
        assert not (tmp_path / ("rank%d" % r) / "gm_score").exists()
    if kw.get("single_sweep"):  # the run did cut hook points into channel ranges
        pts = schedules.SCHEDULES[name]()
        chans = [schedules.scored_shape(p)[1] for p in pts]
        cost = [float(p.H * p.W) for p in pts]
        units = sharding.make_units(chans, cost, max_unit_cost=sum(c * k for c, k in zip(chans, cost)) / (8.0 * world))
        assert len(units) > len(pts)
