"""score -> rates.allocate -> prune(carry=True) -> run on the GPU, for vgg_16_bn, resnet_56 and densenet_40
(the follower case). The allocation is host arithmetic; what the GPU adds is that the score files are the kernels' own:
imp_score(single_sweep=True) writes them from the full net where it lives, as tests/test_carry_gpu.py has it.

Bound, the project's own: the pruned net's error <= 8 x the full net's own fp32 GPU error, both against the full net in
float64 on the CPU as max|got - want| / max|want| over all outputs. The budget case bounds nothing: it prunes live
filters, and what that costs a seeded net before fine-tuning is printed (DESIGN.md §7o has the values)."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import carry_cases as cc
import pruned_cases as pc
from dct_pruning_amd import prune
from dct_pruning_amd import rates as R
from dct_pruning_amd.masks import parse_compress_rate

pytestmark = pytest.mark.gpu
DEV = "cuda"
GPU_NETS = ["vgg_16_bn", "resnet_56", "densenet_40"]


@pytest.fixture(scope="module", params=GPU_NETS)
def case(request, tmp_path_factory):
    name = request.param
    _, x = cc.batches(name)
    full, stems = cc.dead_net(name, calibrate_on=x)
    want = pc.outputs_of(copy.deepcopy(full).double(), x.double())
    full = full.to(DEV)
    score_dir = cc.score(name, full, tmp_path_factory.mktemp("rates_" + name))
    e_full = cc.error_against(pc.outputs_of(full.eval(), x.to(DEV)), want)
    return types.SimpleNamespace(name=name, full=full, stems=stems, score_dir=score_dir, x=x, want=want, e_full=e_full)


def _file(case, stem):
    return np.load(os.path.join(case.score_dir, stem + ".npy"))


def test_zero_loss_on_device_written_files_finds_the_dead_filters_and_the_net_runs(case):
    """measured on one MI355X, fp32 (pruned, full): see DESIGN.md §7o"""
    for stem in case.stems:
        s = _file(case, stem)
        dead = np.arange(s.size) % cc.MOD == 0
        assert s.ndim == 1 and np.all(s[dead] == 0) and not np.signbit(s[dead]).any(), stem
    assert cc.removed_not_dead(lambda stem: _file(case, stem), case.name, cc.RATES[case.name], case.stems) == []
    a = R.allocate(case.name, case.score_dir, max_loss=0.0)
    assert R.widths(case.name, a.rates) == R.widths(case.name, cc.RATES[case.name])
    assert a.level == 0.0 and all(f[3] == 0.0 for f in a.files)
    torch.manual_seed(0)
    pruned = prune.prune_network(case.name, case.full, case.score_dir, parse_compress_rate(a.text), carry=True).eval()
    assert all(t.is_cuda for t in pruned.state_dict().values()) and next(pruned.parameters()).dtype == torch.float32
    e = cc.error_against(pc.outputs_of(pruned, case.x.to(DEV)), case.want)
    print("%s: %s: pruned %.3g, full %.3g (fp32 gpu against the full net in float64 on the cpu)" % (case.name, a.text, e, case.e_full))
    assert e <= 8 * case.e_full


def test_half_the_macs_from_device_written_files(case):
    """measured on one MI355X: see DESIGN.md §7o (level, MACs kept, gap of the pruned net; the gap is not bounded)"""
    a = R.allocate(case.name, case.score_dir, target_macs=0.5)
    assert a.macs <= 0.5 * a.full_macs and a.level > 0
    assert all(lam <= a.level for _, _, _, lam, tag in a.files if tag == "free")
    pruned = prune.prune_network(case.name, case.full, case.score_dir, parse_compress_rate(a.text), carry=True).eval()
    assert prune.cost(pruned, case.x.shape[1:]) == {"macs": a.macs, "params": a.params}
    outs = pc.outputs_of(pruned, case.x.to(DEV))
    assert all(t.is_cuda and bool(torch.isfinite(t).all()) for t in outs)
    assert [t.shape for t in outs] == [w.shape for w in case.want]
    e = cc.error_against(outs, case.want)
    print("%s: level %.4g, MACs %.4f, params %.4f of the full net, %s: gap %.3g (full %.3g)"
          % (case.name, a.level, a.macs / a.full_macs, a.params / a.full_params, a.text, e, case.e_full))
