"""The low-pass signature and gm's lowpass option without a GPU: the oracle against known answers, the C entry point's argument
checks and their order, the size query, check_options, the output directories, what the harness passes to the operators, and
the CLI."""
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
import lowpass_oracle as lo
from dct_pruning_amd import _lib, harness, nets, ops
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init

DROP_DC = 1


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def test_oracle_known_answers():
    for n, (u, v) in ((7, (1, 3)), (8, (0, 0)), (56, (1, 3)), (14, (5, 6))):
        x = torch.from_numpy(lo.basis_map(n, u, v)[None, None])
        s = lo.lowpass_f64(x, n)
        want = np.zeros((n, n))
        want[u, v] = 1.0
        np.testing.assert_allclose(s[0, 0], want, atol=1e-14)
        k = max(u, v)  # the band that just misses it
        if k >= 1:
            np.testing.assert_allclose(lo.lowpass_f64(x, k), 0.0, atol=1e-14)
        assert lo.lowpass_f64(x, k + 1)[0, 0, u, v] == pytest.approx(1.0, abs=1e-14)
    # a constant map: c * sqrt(H * W) at [0, 0], nothing else; the corner of a short edge keeps the whole edge
    x = torch.full((1, 1, 5, 40), 3.0)
    s = lo.lowpass_f64(x, 8)
    assert s.shape == (1, 1, 5, 8) and s[0, 0, 0, 0] == pytest.approx(3.0 * np.sqrt(200.0), rel=1e-14)
    assert np.abs(s[0, 0].ravel()[1:]).max() < 1e-12
    # Parseval: every coefficient kept, the distance is the plain one
    y = go.maps(2, 6, 5, 7, 3)
    np.testing.assert_allclose(lo.gm_lowpass_f64(y, 7), go.gm_nc_f64(y), rtol=1e-12)
    np.testing.assert_allclose(lo.gm_lowpass_f64(y, 99), go.gm_nc_f64(y), rtol=1e-12)


def test_oracle_drop_dc_and_flat_rule():
    x = go.maps(2, 6, 14, 14, 5)        # channel 1 zero, channel 5 a copy of channel 0
    x[:, 2] = 3.7                        # constant: an odd-base edge leaves round-off in the AC terms
    x[:, 3] = -0.25
    x[0, 4] = 1.0
    x[0, 4, 9, 11] = 1.0 + 2.0 ** -20    # constant except for one element: not flat
    plain, drop = lo.lowpass_f64(x, 5), lo.lowpass_f64(x, 5, drop_dc=True)
    assert lo.flat_maps(x).tolist() == [[False, True, True, True, False, False]] * 2
    for c in (1, 2, 3):
        assert (drop[:, c].view(np.int64) == 0).all()  # +0.0 in every element
    for c in (0, 4, 5):
        assert (drop[:, c, 0, 0].view(np.int64) == 0).all()
        rest = np.ones((5, 5), bool)
        rest[0, 0] = False
        np.testing.assert_array_equal(drop[:, c][:, rest], plain[:, c][:, rest])
    assert np.abs(drop[0, 4]).max() > 0
    # correlation = cosine of the centred maps, whose low band is the signature without its DC term
    centred = x.double() - x.double().mean(dim=(2, 3), keepdim=True)
    centred[:, 1:4] = 0
    a, _ = lo.signatures(x, 14, "correlation")
    b, _ = lo.signatures(centred, 14, "cosine")
    np.testing.assert_allclose(a, b, atol=1e-7)  # (channel 4's AC terms are 2^-20 small: their own round-off, normalised)
    d = lo.pair_distances_f64(x, 5, "correlation")
    assert (d[:, 1, 2] == 0).all() and (d[:, 2, 3] == 0).all() and (d[:, 0, 5] == 0).all()
    np.testing.assert_allclose(d[:, 1, 0], 1.0, rtol=1e-14)  # a flat map is at 1 from a live one
    assert (np.diagonal(d, axis1=1, axis2=2) == 0).all()


def test_probe_edge_list_is_the_librarys():
    lib = _lib.load()
    assert [e for e in range(1, 65) if lib.dcts_has_codelet(e, e)] == list(lo.CODELET_EDGES) and len(lo.CODELET_EDGES) == 22
    for n in lo.CODELET_EDGES:
        sizes = lo.corner_sizes(n)
        assert sizes[0] == 1 and sizes[-1] == n and all(1 <= k <= n for k in sizes) and (n == 2 or n - 1 in sizes)
        # both store chains wherever a wave holds several maps, but at edge 2 (no K <= 2 is a multiple of 4)
        assert any(lo.on_vector_chain(n, k) for k in sizes) == (lo.group_size(n) >= 2 and n >= 4), n
        assert any(not lo.on_vector_chain(n, k) for k in sizes)
        assert not any(lo.on_vector_chain(n, k, aligned=False) for k in sizes)
        vec, scalar = lo.chain_sizes(n)
        assert (vec is None) == (n == 2 or n > 32) and (vec is None or (vec <= n and lo.on_vector_chain(n, vec)))
        assert 1 <= scalar <= n and not lo.on_vector_chain(n, scalar)


@pytest.mark.parametrize("n", lo.CODELET_EDGES)
def test_oracle_on_the_basis_sweep_gives_the_identity_corner(n):
    """The probe of tests/test_lowpass_probes_gpu.py before it meets a kernel: on basis map (u, v) the definition has 1 at
    [u][v] where u, v < K and 0 everywhere else, for every K the GPU files use, from float64 maps and from the fp32 maps the
    kernels get (dct_probes.basis_maps: rounded once, so every coefficient is within a few 2^-24 of the ideal)."""
    import dct_probes as dp
    bank = lo.basis_bank(n)
    for u, v in ((0, 0), (1, 3 % n), (n - 1, n - 1)):
        np.testing.assert_array_equal(bank[0, u * n + v], lo.basis_map(n, u, v))
    pairs = dp.cover(n, n, exhaustive=True)
    assert pairs.tolist() == [[u, v] for u in range(n) for v in range(n)]  # map u * n + v is basis (u, v)
    maps32 = dp.basis_maps(n, n, pairs)[None]
    np.testing.assert_array_equal(maps32.numpy(), bank.astype(np.float32))
    whole64, whole32 = lo.lowpass_f64(bank, n), lo.lowpass_f64(maps32, n)
    eye = np.eye(n * n).reshape(1, n * n, n, n)
    np.testing.assert_allclose(whole64, eye, atol=1e-13)
    np.testing.assert_allclose(whole32, eye, atol=4 * 2.0 ** -24)
    step = 1 if n <= 32 else (n * n // 512) | 1  # every K on at most ~600 of the maps: an odd stride visits every column
    for K in lo.corner_sizes(n) + [n + 3]:
        k = min(K, n)
        s = lo.lowpass_f64(maps32[:, ::step], K)
        assert s.shape == (1, len(range(0, n * n, step)), k, k)
        np.testing.assert_array_equal(s, whole32[:, ::step, :k, :k])  # the definition's corner is a slice
        np.testing.assert_allclose(s, eye[:, ::step, :k, :k], atol=4 * 2.0 ** -24)


@pytest.mark.parametrize("n", [n for n in lo.CODELET_EDGES if lo.group_size(n) >= 2])
def test_flat_patterns_classify_as_intended(n):
    G = lo.group_size(n)
    seen = {}
    for parity in (0, 1):
        x, kinds = lo.flat_pattern_maps(n, parity)
        C = x.shape[1]
        assert x.dtype == torch.float32 and tuple(x.shape) == (1, C, n, n) and C == lo.flat_pattern_count(n) >= 2 * G + 1 and C % 2 == 1
        assert [k == "flat" for k in kinds] == [j % 2 == parity for j in range(C)]
        assert lo.flat_maps(x).tolist() == [[k == "flat" for k in kinds]]
        assert set(kinds) == {"flat"} | set(lo.NOT_FLAT)
        flat_values = {float(x[0, j, 0, 0]) for j, k in enumerate(kinds) if k == "flat"}
        assert flat_values == {float(np.float32(v)) for v in lo.FLAT_VALUES}
        for j, k in enumerate(kinds):
            m = x[0, j]
            if k == "last":
                assert (m.reshape(-1)[:-1] == np.float32(3.7)).all() and m[-1, -1] != np.float32(3.7) and abs(float(m[-1, -1]) - 3.7) < 1e-6
            elif k == "first":
                assert (m.reshape(-1)[1:] == np.float32(3.7)).all() and m[0, 0] == 0
            elif k == "nan":
                assert int(torch.isnan(m).sum()) == 1 and (m[~torch.isnan(m)] == np.float32(3.7)).all()
            elif k == "random":
                assert m.max() > m.min()
        seen[parity] = [k == "flat" for k in kinds]
        # the definition under drop_dc: flat maps all +0.0, a NaN map stays NaN
        s = lo.lowpass_f64(x, min(n, 5), drop_dc=True)
        for j, k in enumerate(kinds):
            if k == "flat":
                assert (s[0, j].view(np.int64) == 0).all()
            elif k == "nan":
                assert s[0, j, 0, 0] == 0 and np.isnan(s[0, j]).any()
            else:
                assert s[0, j, 0, 0] == 0 and np.abs(s[0, j]).max() > 0
    # complementary: every position of a group of G maps holds a flat map in one pattern and a live one in the other
    # (map j sits at position j % G of its group), and each map's neighbours in the wave are of the other kind
    assert all(a != b for a, b in zip(seen[0], seen[1])) and len(seen[0]) > G
    assert all(seen[0][j] != seen[0][j + 1] for j in range(len(seen[0]) - 1))


def test_oracle_sees_what_the_option_is_for():
    a = torch.relu(torch.randn(1, 1, 14, 14, generator=torch.Generator().manual_seed(4))).double()
    b = a + torch.from_numpy(lo.basis_map(14, 5, 6))[None, None]
    x = torch.cat([a, b], dim=1)
    assert lo.gm_lowpass_f64(x, 4, "l2", 0, 1, 1, 1)[0, 0] < 1e-12
    assert go.gm_nc_f64(x, 0, 1, 1, 1)[0, 0] == pytest.approx(1.0, rel=1e-12)
    assert lo.gm_lowpass_f64(x, 7, "l2", 0, 1, 1, 1)[0, 0] == pytest.approx(1.0, rel=1e-12)


def test_bounds_are_what_the_module_text_derives():
    x = go.maps(2, 5, 13, 17, 9)
    s = lo.coefficient_scale(x)
    assert lo.SIG_TOL == 2e-6 and lo.signature_tolerance(x) == 2e-6 * s
    assert lo.distance_bound(x, 8, 5) == pytest.approx(5 * 2 * np.sqrt(64) * 2e-6 * s)
    assert lo.distance_bound(x, 16, 1) == pytest.approx(2 * np.sqrt(13 * 16) * 2e-6 * s)  # the short edge keeps 13
    _, norms = lo.signatures(x, 8, "cosine")
    assert lo.metric_bound(x, 8, "cosine", 5) == pytest.approx(lo.distance_bound(x, 8, 5) / norms[norms > 0].min())
    assert go.TOL == pytest.approx(9.93e-6, rel=1e-3)


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    head = text[:text.index("#define DCTS_ABI_VERSION")]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dcts_dct2d_lowpass_f32", "dcts_dct2d_lowpass_workspace_bytes"):
        assert name in head, "%s not listed among the additions to ABI 3" % name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert re.search(r"#define DCTS_LOWPASS_DROP_DC 1\b", text) and ops.LOWPASS_DROP_DC == DROP_DC
    i64, i32, vp, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["dcts_dct2d_lowpass_workspace_bytes"] == (sz, [i64, i32, i64, i64, i32])
    assert _lib.SIGNATURES["dcts_dct2d_lowpass_f32"] == (ctypes.c_int, [vp] + [i64] * 8 + [i32] * 4 + [vp, vp, sz, vp])
    assert "lowpass_nc" in __import__("dct_pruning_amd").__all__


def test_argument_validation_and_its_order_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, K=4, flags=0, out=fake, ws=fake, nbytes=1 << 30):
        return lib.dcts_dct2d_lowpass_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, K, flags, out, ws, nbytes, None)

    def fb(**kw):  # 13 x 17: a shape of the fallback, the only route that looks at the workspace
        kw = dict(dict(h=13, w=17, sh=17, sc=221, sn=884), **kw)
        return call(**kw)

    for f in (call, fb):
        # what every entry point checks, in its order
        assert f(x=None) == -1 and f(out=None) == -1
        assert f(h=0) == -2 and f(n=0) == -2 and f(h=513, w=513, sh=513) == -2
        assert f(cb=2, cc=3) == -3 and f(cc=0) == -3
        assert f(sw=2) == -4 and f(sh=4) == -4
        assert f(x=0x1001) == -7 and f(out=0x1002) == -7
        # then K, then the flags
        assert f(K=0) == -2 and f(K=-3) == -2
        for bad in (2, 3, 4, 1 << 20, -1):
            assert f(flags=bad) == -6
        # doubly bad: the earlier check wins
        assert f(x=None, K=0) == -1 and f(sw=2, K=0) == -4 and f(x=0x1001, flags=2) == -7 and f(cb=2, cc=3, flags=2) == -3
        assert f(K=0, flags=2) == -2 and f(K=0, ws=None) == -2 and f(flags=2, ws=None, nbytes=0) == -6
    # the workspace, on the fallback only: NULL, alignment before size, too small
    need = lib.dcts_dct2d_lowpass_workspace_bytes(1, 4, 13, 17, 4)
    assert need > 0
    for flags in (0, DROP_DC):
        assert fb(ws=None, flags=flags) == -5 and fb(ws=None, nbytes=0, flags=flags) == -5
        assert fb(ws=0x1004, flags=flags) == -7 and fb(ws=0x1008, nbytes=0, flags=flags) == -7
        assert fb(nbytes=0, flags=flags) == -5 and fb(nbytes=16, flags=flags) == -5 and fb(nbytes=2 * 13 * 17 * 4, flags=flags) == -5
    # a codelet shape whose rows have a pitch takes the fallback: it needs a workspace as well
    assert call(sh=12, sc=96, sn=384, ws=None, nbytes=0) == -5
    assert call(sc=80, sn=320, ws=None, nbytes=0) == -5  # dense rows, maps not adjacent to their rows' end: not one dense block


def test_workspace_size_query():
    lib = _lib.load()
    q = lib.dcts_dct2d_lowpass_workspace_bytes
    for n in (2, 4, 7, 8, 9, 10, 14, 16, 18, 20, 28, 32, 36, 40, 56, 64):
        assert lib.dcts_has_codelet(n, n) == 1
        assert q(1, 1, n, n, 1) == 0 and q(256, 2048, n, n, 8) == 0 and q(3, 5, n, n, 999) == 0
    assert q(0, 4, 13, 17, 4) == 0 and q(1, 0, 13, 17, 4) == 0 and q(1, 4, 0, 17, 4) == 0 and q(1, 4, 13, 17, 0) == 0
    assert q(1, 4, 513, 513, 4) == 0
    # everything else: the coefficient layout of the band / entropy fallback for the same tile (those two size theirs for
    # the odd front pad, (H + 1, W + 1); there is none here)
    for n, c, h, w in ((1, 4, 13, 17), (2, 20, 5, 40), (3, 7, 33, 33), (2, 9, 72, 72), (12, 64, 288, 288), (1, 1, 8, 9), (4, 4, 16, 17)):
        got = q(n, c, h, w, 8)
        if not lib.dcts_has_codelet(h - 1, w - 1):  # (32 x 32 is fused there: its query says 0)
            assert got == lib.dcts_entropy_workspace_bytes(n, c, h - 1, w - 1), (h, w)
        assert got % 256 == 0, (h, w)
        assert got >= 2 * h * w * 4 and got == q(n, c, h, w, 1) == q(n, c, h, w, 600)  # K does not size it
        assert q(n * 4, c, h, w, 8) >= got


# ---------------------------------------------------------------------------------------------------------
# operators: what is refused before any GPU call
# ---------------------------------------------------------------------------------------------------------
def test_ops_refusals():
    x = torch.zeros(1, 4, 8, 8)
    for f in (ops.gm_distance_nc, ops.gm_pair_matrix):
        with pytest.raises(ValueError, match="lowpass"):
            f(x, lowpass=-1)
        with pytest.raises(ValueError, match="nothing is left"):
            f(x, lowpass=1, metric="correlation")
        with pytest.raises(ValueError, match="metric"):
            f(x, lowpass=4, metric="euclid")
        with pytest.raises(RuntimeError, match="GPU only"):
            f(x, lowpass=4)
        with pytest.raises(TypeError):
            f(x.half(), lowpass=4)
    with pytest.raises(ValueError, match="K >= 1"):
        ops.lowpass_nc(x, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.lowpass_nc(x, 4)
    with pytest.raises(TypeError):
        ops.lowpass_nc(x.half(), 4)


# ---------------------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------------------
def test_check_options_rules():
    assert len(harness._TABLE) == 5 and harness.CRITERIA == ("dct", "rank", "bands", "entropy", "gm")
    assert harness._TABLE["gm"].metrics == ("l2", "cosine", "correlation")
    for c in harness.CRITERIA:
        harness.check_options(c, "resnet_56", gm_lowpass=0)  # the default goes with every criterion
    for c in ("dct", "rank", "bands", "entropy"):
        for k in (1, 4, -1):
            with pytest.raises(ValueError, match="gm_lowpass"):
                harness.check_options(c, "resnet_56", gm_lowpass=k)
    for m in ("l2", "cosine", "correlation"):
        with pytest.raises(ValueError, match="gm_lowpass"):
            harness.check_options("gm", "resnet_56", gm_metric=m, gm_lowpass=-2)
        harness.check_options("gm", "u2netp", gm_metric=m, gm_lowpass=8, gm_pairs=True)
    with pytest.raises(ValueError, match="nothing is left"):
        harness.check_options("gm", "resnet_56", gm_metric="correlation", gm_lowpass=1)
    for bad in (True, False, 4.0, "4", None, [4]):  # an integer, nothing that merely converts to one
        for c in ("gm", "dct"):
            with pytest.raises(ValueError, match="gm_lowpass must be an integer"):
                harness.check_options(c, "resnet_56", gm_lowpass=bad)
    harness.check_options("gm", "resnet_56", gm_lowpass=np.int64(4))
    harness.check_options("gm", "resnet_56", gm_metric="cosine", gm_lowpass=1)
    harness.check_options("gm", "resnet_56", gm_lowpass=1)
    for kw in ({"deferred": True}, {"autocast": "fp16"}, {"channels_last": True}):  # gm's own refusals stand
        with pytest.raises(ValueError):
            harness.check_options("gm", "resnet_56", gm_lowpass=4, **kw)
    # the new keyword is the last one: every positional call of before means what it meant
    harness.check_options("gm", "resnet_56", False, None, False, (4, "square"), "cosine", True)
    harness.check_options("gm", "resnet_56", False, None, False, (4, "square"), "cosine", True, 4)
    with pytest.raises(ValueError, match="nothing is left"):
        harness.check_options("gm", "resnet_56", False, None, False, (4, "square"), "correlation", False, 1)
    import inspect
    for f in (harness.check_options, harness.imp_score):
        assert list(inspect.signature(f).parameters)[-1] == "gm_lowpass" and inspect.signature(f).parameters["gm_lowpass"].default == 0
    for f in (ops.gm_distance_nc, ops.gm_pair_matrix):
        assert list(inspect.signature(f).parameters)[-1] == "lowpass" and inspect.signature(f).parameters["lowpass"].default == 0


def test_rejections_happen_before_any_sweep(tmp_path):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cases = [dict(criterion=c, gm_lowpass=4) for c in ("dct", "rank", "bands", "entropy")]
    cases += [dict(criterion="gm", gm_lowpass=-1), dict(criterion="gm", gm_lowpass=1, gm_metric="correlation"),
              dict(criterion="gm", gm_lowpass=1, gm_metric="correlation", gm_pairs=True)]
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in cases:
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), types.SimpleNamespace(net="resnet_56", limit=1), train_loader=Loader(), **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


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


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("metric", ["l2", "cosine", "correlation"])
def test_output_directory_and_keywords(metric, pairs, tmp_path, monkeypatch):
    seen = []

    def spy(f):
        def g(x, **kw):
            seen.append((kw.get("metric"), kw.get("lowpass")))
            return f(x, **kw)
        return g

    monkeypatch.setattr(harness, "_gm_nc", spy(lo.gm_lowpass_nc))
    monkeypatch.setattr(harness, "_gm_pairs_nc", spy(lo.gm_lowpass_pairs))
    got, lines, d = _run("resnet_56", tmp_path / "r", gm_metric=metric, gm_pairs=pairs, gm_lowpass=3, single_sweep=True)
    name = "resnet_56_limit1" + ("" if metric == "l2" else "_" + metric) + "_low3" + ("_pairs" if pairs else "")
    assert d.endswith(os.path.join("gm_score", name))
    assert "Importance Score is located at ./gm_score/" + name in lines
    assert set(seen) == {(None if metric == "l2" else metric, 3)} and harness._gm_lowpass == 3
    for k, v in got.items():
        assert k.startswith("gm_") and v.dtype == np.float32 and v.ndim == (2 if pairs else 1), k
        if pairs:
            assert v.shape[0] == v.shape[1] and (np.diagonal(v) == 0).all()
            np.testing.assert_array_equal(v, v.T)


def test_lowpass_zero_names_no_keyword_and_the_setting_does_not_leak(tmp_path, monkeypatch):
    monkeypatch.setattr(harness, "_gm_nc", lo.gm_lowpass_nc)
    low, _, d_low = _run("resnet_56", tmp_path / "low", gm_lowpass=2, single_sweep=True)
    assert harness._gm_lowpass == 2 and d_low.endswith("resnet_56_limit1_low2")
    monkeypatch.setattr(harness, "_gm_nc", go.gm_nc)  # knows neither `metric` nor `lowpass`: the defaults must name neither
    plain, lines_p, d_plain = _run("resnet_56", tmp_path / "plain", single_sweep=True)  # after a low-pass run: no leak
    assert harness._gm_lowpass == 0
    zero, lines_z, d_zero = _run("resnet_56", tmp_path / "zero", gm_lowpass=0, single_sweep=True)
    assert d_plain.endswith("resnet_56_limit1") and d_zero.endswith("resnet_56_limit1") and lines_p == lines_z
    assert sorted(plain) == sorted(zero) == sorted(low)
    for k in plain:
        assert open(os.path.join(d_plain, k + ".npy"), "rb").read() == open(os.path.join(d_zero, k + ".npy"), "rb").read(), k
    assert any(not np.allclose(plain[k], low[k], rtol=1e-3) for k in plain)
    # the scorers themselves
    x = go.maps(1, 5, 6, 6, 2)
    monkeypatch.setattr(harness, "_gm_lowpass", 0)
    monkeypatch.setattr(harness, "_gm_metric", "l2")
    monkeypatch.setattr(harness, "_gm_pairs_nc", lambda x, c_begin, c_count, ref_begin, ref_count: "no keyword")
    assert harness._score_gm(x, 0, 5, False, ref=(0, 5)).equal(go.gm_nc(x))
    assert harness._pair_matrix(x, 0, 5, (0, 5)) == "no keyword"


@pytest.mark.parametrize("metric", ["l2", "correlation"])
@pytest.mark.parametrize("kind,C", [("full", 24), ("last12", 24), ("input", 24)])
def test_point_hook_in_channel_ranges_equals_the_unsplit_one(kind, C, metric, monkeypatch):
    monkeypatch.setattr(harness, "_gm_nc", lo.gm_lowpass_nc)
    monkeypatch.setattr(harness, "_gm_pairs_nc", lo.gm_lowpass_pairs)
    monkeypatch.setattr(harness, "_gm_metric", metric)
    monkeypatch.setattr(harness, "_gm_lowpass", 3)
    x = go.maps(2, C, 6, 5, 21)
    base, count = (C - 12, 12) if kind == "last12" else (0, C)
    for pairs in (False, True):
        whole = harness._PointHook(kind, "host", torch.device("cpu"), key="w", criterion="gm", pairs=pairs)
        split = harness._PointHook(kind, "host", torch.device("cpu"), ranges=[("a", 0, 5), ("b", 5, count)], nominal_c=count,
                                   criterion="gm", pairs=pairs)
        for hook in (whole, split):
            hook(None, (x,), x)
        d = lo.pair_distances_f64(x, 3, metric, base, count, base, count)
        want = (d.sum(axis=0) / x.shape[0] if pairs else d.sum(axis=-1).mean(axis=0)).astype(np.float32)
        np.testing.assert_allclose(whole.scores("w"), want, rtol=1e-6, atol=1e-7)
        np.testing.assert_array_equal(np.concatenate([split.scores("a"), split.scores("b")]), whole.scores("w"))


# ---------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------
def test_cli_gm_lowpass_flag():
    import importance_generation as ig
    base = ["--net", "resnet_56", "--synthetic", "--limit", "1"]
    assert ig.parse_args(base).gm_lowpass == 0 and ig.parse_args(base + ["--criterion", "gm"]).gm_lowpass == 0
    for m in ("l2", "cosine", "correlation"):
        a = ig.parse_args(base + ["--criterion", "gm", "--gm_metric", m, "--gm_lowpass", "8", "--gm_pairs"])
        assert a.gm_lowpass == 8 and a.gm_metric == m and a.gm_pairs
    assert ig.parse_args(base + ["--criterion", "gm", "--gm_lowpass", "1", "--gm_metric", "cosine"]).gm_lowpass == 1
    assert ig.parse_args(base + ["--criterion", "entropy", "--gm_lowpass", "0"]).criterion == "entropy"
    bad = [["--gm_lowpass", "4"], ["--criterion", "rank", "--gm_lowpass", "4"], ["--criterion", "bands", "--gm_lowpass", "2"],
           ["--criterion", "entropy", "--gm_lowpass", "8"], ["--criterion", "gm", "--gm_lowpass", "-1"],
           ["--criterion", "gm", "--gm_lowpass", "1", "--gm_metric", "correlation"],
           ["--criterion", "gm", "--gm_lowpass", "four"], ["--criterion", "gm", "--gm_lowpass", "4", "--deferred"],
           ["--criterion", "gm", "--gm_lowpass", "4", "--autocast", "bf16"]]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            ig.main(base + extra)  # exits in the parser
        assert e.value.code == 2, extra
    assert "--gm_lowpass" in ig.__doc__ and "_low<K>" in ig.__doc__
