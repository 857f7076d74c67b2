"""Host logic of the harness against fixtures captured from the REFERENCE's imp_score
(tests/golden/make_harness_goldens.py): hook order, slicing, running mean, file names, stdout.
No GPU here: the energy operator is swapped for the CPU oracle (test-only injection), so this
checks everything around the kernel; tests/test_harness_gpu.py runs the real kernel."""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest
import torch

from dct_pruning_amd import harness, nets, schedules
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init
from oracle import dct_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    meta = json.load(open(os.path.join(GOLD, "harness_%s.json" % name)))
    arrays = dict(np.load(os.path.join(GOLD, "harness_%s.npz" % name)))
    return meta, arrays


def run_harness(name, tmp_path, device="cpu", **kw):
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).to(device)
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    cwd = os.getcwd()
    os.makedirs(str(tmp_path), exist_ok=True)
    os.chdir(tmp_path)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            harness.imp_score(net, args, train_loader=loader, **kw)
    finally:
        os.chdir(cwd)
    d = os.path.join(str(tmp_path), "importance_score", "%s_limit%d" % (name, limit))
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)} if os.path.isdir(d) else {}
    return out, buf.getvalue().splitlines(), d


def compare(out, lines, meta, arrays, rtol):
    assert sorted(out) == meta["files"]
    assert lines == meta["stdout"]
    for k, ref in arrays.items():
        got = out[k]
        assert got.dtype == np.float32 and got.shape == ref.shape, k
        np.testing.assert_array_equal(got == 0, ref == 0, err_msg=k)
        np.testing.assert_allclose(got, ref, rtol=rtol, atol=0, err_msg=k)


@pytest.fixture
def oracle_energy(monkeypatch):
    monkeypatch.setattr(harness, "_energy_nc", orc.energy_nc_batched)


@pytest.mark.parametrize("name", list(HARNESS_CASES))
def test_state_dict_layout_matches_reference(name):
    keys = json.load(open(os.path.join(GOLD, "state_dict_keys.json")))[name]
    sd = nets.get_network(name).state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == keys


@pytest.mark.parametrize("name", ["vgg_16_bn", "resnet_56", "densenet_40", "googlenet", "resnet_50", "u2netp"])
def test_per_hook_sweeps_match_reference_run(name, tmp_path, oracle_energy):
    meta, arrays = load_golden(name)
    out, lines, d = run_harness(name, tmp_path)
    compare(out, lines, meta, arrays, rtol=2e-5)
    # on-disk format: NumPy v1.0 header, '<f4', C order, data at byte 128 (utils/common.py:394)
    f = os.path.join(d, sorted(os.listdir(d))[0])
    raw = open(f, "rb").read()
    assert raw[:8] == b"\x93NUMPY\x01\x00" and b"'descr': '<f4'" in raw[:128] and b"'fortran_order': False" in raw[:128]
    assert len(raw) == 128 + 4 * np.load(f).size


@pytest.mark.parametrize("name", ["vgg_16_bn", "resnet_50", "densenet_40"])
def test_single_sweep_equals_per_hook(name, tmp_path, oracle_energy):
    meta, arrays = load_golden(name)
    out, lines, _ = run_harness(name, tmp_path, single_sweep=True)
    compare(out, lines, meta, arrays, rtol=2e-5)


def test_shipped_reference_files_have_the_same_format():
    """The 41 .npy files the reference ships (format only; values are not reproducible), kept as
    fixtures under tests/golden/reference_importance_score/."""
    ref_dir = os.path.join(GOLD, "reference_importance_score")
    n = 0
    for sub in os.listdir(ref_dir):
        for f in os.listdir(os.path.join(ref_dir, sub)):
            raw = open(os.path.join(ref_dir, sub, f), "rb").read()
            a = np.load(os.path.join(ref_dir, sub, f), allow_pickle=False)
            assert a.dtype == np.float32 and a.ndim == 1
            assert raw[:8] == b"\x93NUMPY\x01\x00" and len(raw) == 128 + 4 * a.size
            n += 1
    assert n == 41
    stems = {f[:-4] for f in os.listdir(os.path.join(ref_dir, "googlenet_limit5"))}
    ours = {s for p in schedules.googlenet() for s, _, _ in p.files}
    assert stems == ours


def test_schedule_tables_census():
    """sweeps, files and maps per sample for every net."""
    expect = {"vgg_16_bn": (12, 12, 3712), "resnet_56": (55, 55, 2032), "resnet_110": (109, 109, 4048),
              "densenet_40": (39, 39, 936), "googlenet": (10, 37, 5680), "resnet_50": (49, 53, 22720),
              "u2netp": (118, 118, 3232)}
    for name, (sweeps, files, maps) in expect.items():
        pts = schedules.SCHEDULES[name]()
        assert len(pts) == sweeps
        assert sum(len(p.files) for p in pts) == files
        assert sum(schedules.scored_shape(p)[1] for p in pts) == maps


def test_hooks_have_reference_signature(oracle_energy):
    m = torch.nn.ReLU()
    x = torch.relu(torch.randn(2, 24, 9, 9))
    harness._acc.reset()
    h = m.register_forward_hook(harness.get_feature_hook)
    m(x)
    h.remove()
    assert harness._acc.feature_result.shape == (24,) and harness._acc.total.item() == 2
    harness._acc.reset()
    h = m.register_forward_hook(harness.get_feature_hook_densenet)
    m(x)
    h.remove()
    assert harness._acc.feature_result.shape == (12,)
    harness._acc.reset()
    h = m.register_forward_hook(harness.get_feature_hook_u2net_input)
    m(x)
    h.remove()
    assert harness._acc.feature_result.shape == (24,)
    harness._acc.reset()
