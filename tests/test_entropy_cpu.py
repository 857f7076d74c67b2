"""The entropy criterion's host side without a GPU: the C ABI entry points (declared, bound, exported, argument codes, the
workspace query), known answers of the oracle (tests/entropy_oracle.py), the operator's input checks,
imp_score(criterion="entropy") with the oracle in the kernel's place, the mask tool on its files and the CLI's parse errors."""
import contextlib
import ctypes
import io
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import entropy_oracle as eo
import dct_pruning_amd as dpa
from dct_pruning_amd import _lib, harness, masks, nets, ops
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

NEW = ("dcts_entropy_workspace_bytes", "dcts_has_entropy_kernel", "dcts_spectral_entropy_f32")


# ---------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------
def test_entropy_entry_points_declared_bound_exported(repo_root):
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    assert re.search(r"#define DCTS_ABI_VERSION 3\b", text) and _lib.ABI_VERSION == 3
    head = text[:text.index("#define DCTS_ABI_VERSION")]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in head, "%s is not listed among the additions to ABI 3" % name
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    proto = re.search(r"int dcts_spectral_entropy_f32\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["dcts_spectral_entropy_f32"][1]) == 17
    proto = re.search(r"size_t dcts_entropy_workspace_bytes\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["dcts_entropy_workspace_bytes"][1]) == 4
    assert _lib.load().dcts_version() == 3
    assert "spectral_entropy_nc" in dpa.__all__ and "has_entropy_kernel" in dpa.__all__
    assert dpa.spectral_entropy_nc is ops.spectral_entropy_nc and dpa.has_entropy_kernel is ops.has_entropy_kernel


def test_has_entropy_kernel_is_the_band_kernels_table():
    lib = _lib.load()
    for e in range(1, 81):
        assert lib.dcts_has_entropy_kernel(e, e) == lib.dcts_has_band_kernel(e, e), e
        assert ops.has_entropy_kernel(e, e) == bool(lib.dcts_has_band_kernel(e, e))
    assert lib.dcts_has_entropy_kernel(56, 28) == lib.dcts_has_band_kernel(56, 28) == 0
    assert lib.dcts_has_entropy_kernel(7, 7) == 1 and lib.dcts_has_entropy_kernel(9, 9) == 1


def test_entropy_workspace_query():
    q = _lib.load().dcts_entropy_workspace_bytes
    for e in eo.FUSED_EDGES:  # the fused kernel takes the tile, with the odd pad (7 -> 8, 9 -> 10) as well
        assert q(3, 7, e, e) == 0, e
    assert q(0, 1, 8, 8) == 0 and q(1, 1, 513, 8) == 0
    for (n, c, h, w) in [(1, 3, 72, 72), (1, 3, 56, 28), (1, 3, 13, 13), (1, 3, 288, 288), (2, 5, 16, 17), (1, 1, 512, 512)]:
        b = q(n, c, h, w)
        assert b > 0 and b % 256 == 0
        assert b >= 2 * (h + 1) * (w + 1) * 4  # one map of the fallback's two halves, with the odd pad


def test_entropy_argument_validation_without_gpu():
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every case fails validation before any launch

    def call(x=fake, n=1, c=4, h=8, w=8, sn=256, sc=64, sh=8, sw=1, cb=0, cc=4, pad=0, out=fake, ws=fake, wsb=1 << 20, algo=0):
        return lib.dcts_spectral_entropy_f32(x, n, c, h, w, sn, sc, sh, sw, cb, cc, pad, out, ws, wsb, None, algo)

    assert call(x=None) == -1 and call(out=None) == -1
    assert call(n=0) == -2 and call(h=0) == -2 and call(w=-1) == -2 and call(h=513, w=513, sh=513) == -2
    assert call(cb=2, cc=3) == -3 and call(cc=0) == -3 and call(cb=-1) == -3
    assert call(sw=2) == -4 and call(sh=4) == -4
    assert call(x=0x1001) == -7 and call(out=0x1002) == -7
    # the fallback needs a workspace: DIRECT on a fused shape, a non-square map, an edge beyond the codelets
    assert call(ws=None, wsb=0, algo=1) == -5 and call(ws=0x1004, algo=1) == -7
    assert call(wsb=16, algo=1) == -5                                          # not even one map
    assert call(h=56, w=28, sn=4 * 56 * 28, sc=56 * 28, sh=28, ws=None, wsb=0) == -5
    assert call(h=72, w=72, sn=4 * 72 * 72, sc=72 * 72, sh=72, wsb=2 * 72 * 72 * 4) == -5  # two tiles, nothing for the tables
    assert call(h=56, w=28, sn=4 * 56 * 28, sc=56 * 28, sh=28, algo=2) == -6   # no fused kernel for a non-square map
    assert call(sh=12, sc=96, sn=384, algo=2) == -6                            # nor for row-pitched maps
    assert call(algo=3) == -6 and call(algo=9) == -6


# ---------------------------------------------------------------------------------------------------------
# the oracle: known answers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", eo.BASIS_EDGES)
def test_oracle_single_basis_function_and_constant_map(n):
    h = eo.entropy_nc_f64(eo.basis_maps(n))
    assert h.shape == (1, n * n) and np.abs(h).max() < 1e-9  # fp32 maps: the other coefficients are 2^-24 of the one
    const = torch.full((1, 2, n, n), 3.25)
    const[0, 1] = -0.5
    assert np.abs(eo.entropy_nc_f64(const)).max() < 1e-12
    assert (eo.entropy_nc_f64(torch.zeros(1, 3, n, n)) == 0).all()


@pytest.mark.parametrize("n", eo.BASIS_EDGES)
def test_oracle_two_equal_basis_functions_give_ln2(n):
    np.testing.assert_allclose(eo.entropy_nc_f64(eo.pair_maps(n)), math.log(2.0), rtol=0, atol=1e-6)
    np.testing.assert_allclose(eo.entropy_nc_f32(eo.pair_maps(n)), math.log(2.0), rtol=0, atol=eo.TOL)


def test_probe_edge_lists_are_the_librarys():
    lib = _lib.load()
    edges = [e for e in range(1, 65) if lib.dcts_has_codelet(e, e)]
    assert edges == list(eo.FUSED_EDGES) and len(edges) == 22
    assert [h for h in range(1, 64, 2) if lib.dcts_has_codelet(h + 1, h + 1)] == list(eo.PAD_EDGES) and len(eo.PAD_EDGES) == 20
    assert all(lib.dcts_has_entropy_kernel(e, e) == 1 for e in edges)
    names = [name for name, _, _, _ in eo.gpu_inputs()]
    for e in eo.FUSED_EDGES:
        assert "fused %d" % e in names and "unequal %d" % e in names
    for e in eo.PAD_EDGES:
        assert "pad %d" % e in names and "pad unequal %d" % e in names


@pytest.mark.parametrize("n", [2, 7, 8, 14, 20])
def test_oracle_unequal_pairs(n):
    x = eo.unequal_pair_maps(n)
    assert tuple(x.shape) == (1, n * n, n, n) and x.dtype == torch.float32
    # the construction: coefficient p is 1 and (u, v) is 1 / 2, everything else 0
    c = orc.dct_2d_f64(x.numpy().astype(np.float64))[0]
    for m in range(n * n):
        u, v = divmod(m, n)
        p = (1 % n, 2 % n) if (u, v) != (1 % n, 2 % n) else (2 % n, 1 % n)
        want = np.zeros((n, n))
        want[p] = 1.0
        want[u, v] = 0.5
        np.testing.assert_allclose(c[m], want, atol=1e-6)
    assert eo.H_UNEQUAL == pytest.approx(0.5004024, abs=1e-7)
    np.testing.assert_allclose(eo.entropy_nc_f64(x), eo.H_UNEQUAL, rtol=0, atol=1e-6)
    np.testing.assert_allclose(eo.entropy_nc_f32(x), eo.H_UNEQUAL, rtol=0, atol=eo.TOL)
    if n % 2 == 0:  # under the pad: the padded tile's pairs without the row and column the pad gives back as zeros
        y = eo.padded_unequal_pair_maps(n - 1)
        assert tuple(y.shape) == (1, n * n, n - 1, n - 1)
        np.testing.assert_array_equal(y.numpy(), x.numpy()[:, :, 1:, 1:])
        ref = eo.entropy_nc_f64(y, pad_front_if_odd=True)
        np.testing.assert_array_equal(ref, eo.entropy_nc_f64(torch.nn.functional.pad(y, (1, 0, 1, 0))))
        assert np.abs(eo.entropy_nc_f32(y, pad_front_if_odd=True).astype(np.float64) - ref).max() <= eo.TOL


@pytest.mark.parametrize("n", eo.BASIS_EDGES)
@pytest.mark.parametrize("where", ["dc-row", "interior"])
def test_unequal_pairs_catch_one_wrong_weight_that_the_equal_pairs_miss(n, where):
    """What the unequal pairs are for. The mutant is the fp32 restatement with the weight of ONE coefficient off by 1e-3
    (a wrong 1 / sqrt(2) of the DC row, a wrong entry of a twiddle table). At p = (1/2, 1/2), the maximum of H, that moves
    ln 2 by eps^2 / 2 = 5e-7; a single basis function has H = 0 whatever its weight. Both old probes pass the mutant at
    TOL = 4.2e-5. At p = (0.8, 0.2) it moves H by 0.44 eps = 4.4e-4, ten times TOL."""
    u, v = (0, 1) if where == "dc-row" else (2, 3)
    eps = 1e-3

    def mutant(x):
        w = eo.coefficients_f32(x).copy()
        w[..., u, v] *= np.float32(1.0 + eps)
        return eo.entropy_of_coefficients_f32(w).astype(np.float64)

    def honest(x):
        return eo.entropy_nc_f32(x).astype(np.float64)

    pairs, basis, unequal = eo.pair_maps(n), eo.basis_maps(n), eo.unequal_pair_maps(n)
    # the mutated coefficient is one of an equal pair (tests/entropy_oracle.py: (0, 1) + (n-1, n-1) and (2, 3) + (3, 2))
    c = orc.dct_2d_f64(pairs.numpy().astype(np.float64))[0]
    assert (np.abs(c[:, u, v]) > 0.9).any()
    err_pairs = np.abs(mutant(pairs) - math.log(2.0)).max()
    err_basis = np.abs(mutant(basis)).max()
    ref = eo.entropy_nc_f64(unequal)
    err_unequal = np.abs(mutant(unequal) - ref)
    err_honest = np.abs(honest(unequal) - ref).max()
    print("ENTROPY mutant %d (%d, %d) * (1 + %.0e): pairs %.3e, basis %.3e, unequal pairs %.3e (honest %.3e), tol %.3e"
          % (n, u, v, eps, err_pairs, err_basis, err_unequal.max(), err_honest, eo.TOL))
    assert err_pairs <= eo.TOL and err_basis <= eo.TOL          # the old probes: blind to it
    assert err_honest <= eo.R                                    # the restatement itself meets the new one
    assert err_unequal.max() > 4 * eo.TOL                        # the new probe: far outside
    # and it is the map whose half-amplitude partner is (u, v) that shows it, by 0.44 eps
    assert int(err_unequal.argmax()) == u * n + v
    assert err_unequal.max() == pytest.approx(0.4436 * eps, rel=0.05)


def test_oracle_scale_invariance_bounds_and_pad():
    x, big, small = eo.scale_case()
    ref = eo.entropy_nc_f64(x)
    np.testing.assert_allclose(eo.entropy_nc_f64(big), ref, rtol=1e-12)
    np.testing.assert_allclose(eo.entropy_nc_f64(small), ref, rtol=1e-12)
    assert (ref > 0).all() and (ref <= math.log(14 * 14)).all()
    # a textured map comes close to the top (white noise: ln(HW) - 0.73 in expectation), a blob stays near the bottom
    assert eo.entropy_nc_f64(torch.randn(1, 1, 32, 32, generator=torch.Generator().manual_seed(1)))[0, 0] > math.log(1024) - 1.0
    blob = torch.exp(-((torch.arange(32.0) - 15.5) ** 2) / 200.0)
    assert eo.entropy_nc_f64((blob[:, None] * blob[None, :])[None, None])[0, 0] < 0.2 * math.log(1024)
    # the odd front pad: the definition on the 14 x 14 tile with a zero row and column in front
    p = eo.pad_case(13)
    padded = torch.nn.functional.pad(p, (1, 0, 1, 0))
    np.testing.assert_array_equal(eo.entropy_nc_f64(p, 2, 3, True), eo.entropy_nc_f64(padded, 2, 3, False))
    assert not np.array_equal(eo.entropy_nc_f64(p, 2, 3, True), eo.entropy_nc_f64(p, 2, 3, False))
    # the float32 stand-in for the operator
    got = eo.entropy_nc(p, 2, 3, True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3)


def test_tolerance_is_eight_times_the_measured_restatement_error():
    """The constant in entropy_oracle.py against a fresh measurement on the cheap inputs (the worst one, the map scaled by
    2^20, among them). Matrix products block differently from one CPU to the next, so the fresh figure may differ a
    little from the recorded one: it must stay within twice R, which leaves the kernels' 8 R meaningful."""
    assert eo.TOL == 8 * eo.R and 1e-6 < eo.R < 1e-5
    worst = 0.0
    for name, x, pad, scales in eo.gpu_inputs():
        if max(x.shape[2:]) <= 16:
            worst = max(worst, eo.restatement_error(x, pad, scales))
    assert eo.R / 4 <= worst <= 2 * eo.R, worst


# ---------------------------------------------------------------------------------------------------------
# the operator's input checks
# ---------------------------------------------------------------------------------------------------------
def test_ops_reject_half_cpu_and_3d_tensors():
    with pytest.raises(TypeError):
        ops.spectral_entropy_nc(torch.zeros(1, 2, 8, 8, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.spectral_entropy_nc(torch.zeros(1, 2, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.spectral_entropy_nc(torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError):
        ops.spectral_entropy_nc(torch.zeros(2, 8, 8))
    with pytest.raises(TypeError):
        ops.spectral_entropy_nc(np.zeros((1, 2, 8, 8), np.float32))


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
    top = "entropy_score" if criterion == "entropy" else "importance_score"
    d = os.path.join(str(root), top, "%s_limit%d" % (name, limit))
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return files, buf.getvalue().splitlines(), d


@pytest.fixture
def oracle_ops(monkeypatch):
    monkeypatch.setattr(harness, "_entropy_nc", eo.entropy_nc)
    monkeypatch.setattr(harness, "_energy_nc", orc.energy_nc_batched)


def test_imp_score_entropy_on_resnet_56(tmp_path, oracle_ops):
    assert "entropy" in harness.CRITERIA
    ent, lines, d = _run("resnet_56", tmp_path / "ent", "entropy")
    dct, lines_d, d_dct = _run("resnet_56", tmp_path / "dct", "dct")
    assert d.endswith(os.path.join("entropy_score", "resnet_56_limit1"))
    assert len(ent) == len(dct) > 0 and sorted(ent) == sorted("ent_" + s[len("imp_"):] for s in dct)
    assert lines == [ln.replace("./importance_score/", "./entropy_score/") for ln in lines_d]
    assert not (tmp_path / "ent" / "importance_score").exists()
    single, _, _ = _run("resnet_56", tmp_path / "single", "entropy", single_sweep=True)
    assert sorted(single) == sorted(ent)

    # the values: the oracle's running mean over the very activations the hooks saw (one batch of two samples)
    from dct_pruning_amd import schedules
    bs, limit, size, as_dict = HARNESS_CASES["resnet_56"]
    net = deterministic_init(nets.get_network("resnet_56")).eval()
    x = next(iter(SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)))[0]
    pts = schedules.SCHEDULES["resnet_56"]()
    seen = {}
    handles = [harness._resolve(net, p.module).register_forward_hook(
        lambda m, i, o, _p=p: seen.__setitem__(_p.module, o.detach().clone())) for p in pts]
    with torch.no_grad():
        net(x)
    for h in handles:
        h.remove()
    checked = 0
    for p in pts:
        want = eo.entropy_nc_f64(seen[p.module]).mean(axis=0)
        for stem, lo, hi in p.files:
            got = ent["ent_" + stem[len("imp_"):]]
            ref = want if lo is None else want[lo:hi]
            assert got.dtype == np.float32 and got.shape == ref.shape, stem
            np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6, err_msg=stem)
            np.testing.assert_allclose(single["ent_" + stem[len("imp_"):]], got, rtol=0, atol=2e-6, err_msg=stem)
            hw = seen[p.module].shape[2] * seen[p.module].shape[3]
            assert (got >= 0).all() and (got <= math.log(hw)).all()
            checked += 1
    assert checked == len(ent)

    # on-disk format: the dct files' own header, byte for byte (NumPy v1.0, '<f4', C order, data at byte 128)
    for k in ent:
        raw = open(os.path.join(d, k + ".npy"), "rb").read()
        ref_raw = open(os.path.join(d_dct, "imp_" + k[len("ent_"):] + ".npy"), "rb").read()
        assert raw[:128] == ref_raw[:128] and raw[:8] == b"\x93NUMPY\x01\x00" and len(raw) == 128 + 4 * ent[k].size, k

    # the mask tool reads the directory as it reads any directory of per-channel scores
    m = masks.masks_for_dir(d, 0.5)
    assert sorted(m) == sorted(ent)
    for k, v in m.items():
        c = ent[k].shape[0]
        np.testing.assert_array_equal(v, orc.select_index(ent[k], c, orc.kept_filters(c, 0.5)))
    assert masks.main(["--imp_score", d, "--compress_rate", "[0.5]*%d" % len(ent), "--out", str(tmp_path / "m.npz")]) == 0
    assert sorted(np.load(str(tmp_path / "m.npz")).files) == sorted(ent)


def test_entropy_hooks_have_reference_signature(oracle_ops):
    m = torch.nn.ReLU()
    x = torch.relu(torch.randn(2, 24, 9, 9, generator=torch.Generator().manual_seed(3)))
    for hook, cb, cc, pad in [(harness.get_feature_hook_entropy, 0, 24, False),
                              (harness.get_feature_hook_densenet_entropy, 12, 12, True),
                              (harness.get_feature_hook_u2net_input_entropy, 0, 24, True)]:
        harness._acc.reset()
        h = m.register_forward_hook(hook)
        m(x)
        h.remove()
        want = eo.entropy_nc_f64(x, cb, cc, pad).mean(axis=0)  # x is non-negative: relu(x) == x, input == output
        got = harness._acc.feature_result.numpy()
        assert got.shape == (cc,) and harness._acc.total.item() == 2
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    harness._acc.reset()
    assert harness._file_stem("entropy", "imp_conv3") == "ent_conv3"
    assert harness._file_stem("entropy", "net.stage1.rebnconv1.relu_s1") == "ent_net.stage1.rebnconv1.relu_s1"
    assert harness._file_stem("bands", "net.stage1.rebnconv1.relu_s1") == "band_net.stage1.rebnconv1.relu_s1"  # the rule followed


def test_entropy_rejections_before_any_sweep(tmp_path, oracle_ops):
    class Loader:
        def __iter__(self):
            raise AssertionError("a sweep started")

    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        for kw in [{"deferred": True}, {"autocast": "fp16"}, {"autocast": "bf16"}, {"channels_last": True}]:
            args = types.SimpleNamespace(net="resnet_56", limit=1)
            with pytest.raises(ValueError):
                harness.imp_score(torch.nn.Identity(), args, train_loader=Loader(), criterion="entropy", **kw)
    finally:
        os.chdir(cwd)
    assert os.listdir(str(tmp_path)) == []


def test_cli_entropy_flags():
    import importance_generation as ig
    a = ig.parse_args(["--net", "resnet_56", "--criterion", "entropy", "--synthetic", "--limit", "1"])
    assert (a.criterion, a.limit) == ("entropy", 1)
    assert ig.parse_args(["--net", "u2netp", "--criterion", "entropy", "--single_sweep"]).net == "u2netp"
    for extra in (["--deferred"], ["--autocast", "fp16"], ["--channels_last"]):
        with pytest.raises(SystemExit) as e:
            ig.main(["--net", "resnet_56", "--criterion", "entropy", "--synthetic"] + extra)  # exits in the parser
        assert e.value.code == 2
    assert ig.parse_args(["--net", "resnet_56"]).criterion == "dct"
    assert "entropy_score/" in ig.__doc__
