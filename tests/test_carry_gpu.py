"""score -> prune(carry=True) -> run on the GPU for five nets with dead filters: the full net is scored
by imp_score(single_sweep=True) where it lives, pruned from those files on GPU tensors and evaluated on the scoring batch.

Bound, the project's own: the pruned net's error <= 8 x the full net's own fp32 GPU error, both taken against the full
net in float64 on the CPU as max|got - want| / max|want| over all outputs. Nothing is compared before the files are
shown to hold exactly +0.0 at every dead index and every removed index is shown to be dead, read from the files."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import carry_cases as cc
import pruned_cases as pc
from dct_pruning_amd import prune

pytestmark = pytest.mark.gpu
DEV = "cuda"
GPU_NETS = ["vgg_16_bn", "densenet_40", "googlenet", "resnet_56", "u2netp"]


@pytest.fixture(scope="module", params=GPU_NETS)
def case(request, tmp_path_factory):
    name = request.param
    _, x = cc.batches(name)
    full, stems = cc.dead_net(name, calibrate_on=x)
    want = pc.outputs_of(copy.deepcopy(full).double(), x.double())
    full = full.to(DEV)
    score_dir = cc.score(name, full, tmp_path_factory.mktemp("carry_" + name))
    e_full = cc.error_against(pc.outputs_of(full.eval(), x.to(DEV)), want)
    return types.SimpleNamespace(name=name, full=full, stems=stems, score_dir=score_dir, x=x, want=want, e_full=e_full)


def _file(case, stem):
    return np.load(os.path.join(case.score_dir, stem + ".npy"))


def test_score_files_hold_plus_zero_at_every_dead_index(case):
    assert case.stems
    for stem in case.stems:
        s = _file(case, stem)
        dead = np.arange(s.size) % cc.MOD == 0
        assert s.ndim == 1 and np.all(s[dead] == 0) and not np.signbit(s[dead]).any(), stem
    assert cc.removed_not_dead(lambda stem: _file(case, stem), case.name, cc.RATES[case.name], case.stems) == []


def test_pruned_from_gpu_scores_equals_the_full_net(case):
    """measured on one MI355X, fp32 (pruned, full): see DESIGN.md §7m"""
    assert cc.removed_not_dead(lambda stem: _file(case, stem), case.name, cc.RATES[case.name], case.stems) == []
    torch.manual_seed(0)
    pruned = prune.prune_network(case.name, case.full, case.score_dir, cc.RATES[case.name], carry=True).eval()
    assert all(t.is_cuda for t in pruned.state_dict().values()) and next(pruned.parameters()).dtype == torch.float32
    e = cc.error_against(pc.outputs_of(pruned, case.x.to(DEV)), case.want)
    print("%s: pruned %.3g, full %.3g (fp32 gpu against the full net in float64 on the cpu)" % (case.name, e, case.e_full))
    assert e <= 8 * case.e_full
