"""The pruned nets on the GPU: forward against the reference's float64 fixtures, the whole path score ->
prune -> run for a ResNet-50 with dead mid channels, and prune_network on GPU tensors.

Error measure everywhere: max|got - want| / max|want| over the compared values. The nets' arithmetic is
PyTorch's convolutions, so the yardstick for fp32 on the GPU is the same module in fp32 on the CPU, and the
bound is the project's factor of eight on it: 8 * max(e_cpu32, 2^-22). DESIGN.md §7l has the measured table."""
import contextlib
import io
import os
import types

import numpy as np
import pytest
import torch

import pruned_cases as pc
from dct_pruning_amd import harness, nets, prune
from dct_pruning_amd import transplant as tp
from helpers import HARNESS_CASES, det_scores, det_tensor, tensor_digest

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("net", pc.NETS)
def test_forward_on_the_gpu_equals_the_reference_model(net):
    fx = pc.forward_fixture(net)["readme"]
    model = pc.slim_net(net, fx["rates"])
    x = pc.net_input(net)
    e_cpu = pc.rel_err(pc.outputs_of(model, x), fx["outputs"])
    outs = pc.outputs_of(model.to(DEV), x.to(DEV))
    assert [list(t.shape) for t in outs] == [w["shape"] for w in fx["outputs"]]
    e_gpu = pc.rel_err(outs, fx["outputs"])
    print("%s: fp32 gpu %.3g, fp32 cpu %.3g (against the reference in float64)" % (net, e_gpu, e_cpu))
    assert e_gpu <= 8 * max(e_cpu, 2.0 ** -22)


# ---------------------------------------------------------------------------------------------------------
# end to end, ResNet-50 with dead mid channels (index % 3 == 0)
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dead_case(tmp_path_factory):
    """The full net scored by imp_score as it stands (per-hook mode, SyntheticLoader, the HARNESS_CASES batch, limit
    1), pruned from those files at the mid-only rates; the full net's float64 output on the CPU and its own fp32 GPU
    error are the yardstick."""
    root = tmp_path_factory.mktemp("dead_resnet_50")
    bs, limit, _, _ = HARNESS_CASES["resnet_50"]
    full = pc.dead_resnet_50().to(DEV)
    loader, x = pc.dead_batch()
    args = types.SimpleNamespace(net="resnet_50", limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(full, args, train_loader=loader)
    finally:
        os.chdir(cwd)
    score_dir = os.path.join(str(root), "importance_score", "resnet_50_limit%d" % limit)
    want = pc.outputs_of(pc.dead_resnet_50().double(), x.double())[0]
    got_full = pc.outputs_of(full.eval(), x.to(DEV))[0]
    e_full = float((got_full.double().cpu() - want).abs().max() / want.abs().max())
    torch.manual_seed(0)
    pruned = prune.prune_network("resnet_50", full, score_dir, pc.MID_ONLY).eval()
    return types.SimpleNamespace(full=full, pruned=pruned, x=x, want=want, e_full=e_full, score_dir=score_dir)


def _err(case, model):
    got = pc.outputs_of(model, case.x.to(DEV))[0]
    return float((got.double().cpu() - case.want).abs().max() / case.want.abs().max())


def test_score_files_hold_plus_zero_at_every_dead_channel(dead_case):
    for (stem, ori, _), (_, _, _, _, kind) in zip(tp.resnet_50_kept(pc.MID_ONLY), tp.resnet_50_convs()):
        if kind != "mid":
            continue
        s = np.load(os.path.join(dead_case.score_dir, stem + ".npy"))
        dead = np.arange(ori) % 3 == 0
        assert s.shape == (ori,) and np.all(s[dead] == 0) and not np.signbit(s[dead]).any(), stem
        kept = tp.select_index(s, ori, ori - ori // 4)
        assert np.all(s[np.setdiff1d(np.arange(ori), kept)] == 0), stem  # what goes has no energy on this batch
    p = next(dead_case.pruned.parameters())
    assert p.is_cuda and p.dtype == torch.float32


def test_pruned_from_gpu_scores_equals_the_full_net(dead_case):
    e = _err(dead_case, dead_case.pruned)
    print("pruned %.3g, full %.3g (fp32 gpu against the full net in float64 on the cpu)" % (e, dead_case.e_full))
    assert e <= 8 * dead_case.e_full


# ---------------------------------------------------------------------------------------------------------
# strict load on the GPU
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["resnet_56", "u2netp"])
def test_prune_network_on_gpu_tensors_hashes_to_the_goldens(net, monkeypatch):
    fx = pc.transplant_fixture(net)
    orig = nets.get_network
    monkeypatch.setattr(prune.nets, "get_network", lambda n, r=None: pc.fill_slim(orig(n, r)))  # the caller's seed
    ori = {k: det_tensor(k, s, "").to(DEV) for k, s in fx["ori"]}
    imp = {stem: det_scores(stem, c) for stem, c in fx["stems"]}
    got = prune.prune_network(net, ori, imp, fx["rates"])  # load_state_dict(strict=True) inside
    sd = got.state_dict()
    assert list(sd) == [k for k, _ in fx["slim"]] and all(v.is_cuda for v in sd.values())
    assert not [k for k, v in sd.items() if tensor_digest(v) != fx["digest"][k]]
