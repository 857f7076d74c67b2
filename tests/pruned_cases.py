"""What tests/test_pruned_nets_cpu.py and tests/test_pruned_nets_gpu.py share: the fixtures of
tests/golden/make_pruned_goldens.py (the reference's own pruned models, float64), the seeded slim nets and
inputs they were made from, and the ResNet-50 with dead mid channels."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

from dct_pruning_amd import nets
from dct_pruning_amd import transplant as tp
from helpers import HARNESS_CASES, det_tensor, deterministic_init

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ["vgg_16_bn", "resnet_56", "resnet_110", "densenet_40", "googlenet", "resnet_50", "u2netp"]
MID_ONLY = [0.0] * 4 + [0.25] * 16  # ResNet-50: stem and block outputs whole, every mid width x 0.75


@functools.lru_cache(None)
def transplant_fixture(net):
    return json.load(open(os.path.join(GOLDEN, "transplant_%s.json" % net)))


@functools.lru_cache(None)
def forward_fixture(net):
    fx = json.load(open(os.path.join(GOLDEN, "pruned_forward_%s.json" % net)))
    return {c["name"]: c for c in fx["cases"]}


def key_shapes(sd):
    return [[k, list(v.shape)] for k, v in sd.items()]


def keys_digest(sd):
    return hashlib.sha256(json.dumps(key_shapes(sd)).encode()).hexdigest()[:20]


def fill_slim(net):
    with torch.no_grad():
        for k, t in net.state_dict().items():
            t.copy_(det_tensor(k, t.shape, "slim:"))
    return net


def slim_net(net, rates):
    """get_network(net, rates) with the weights the fixture's reference model had (float32, eval)."""
    return fill_slim(nets.get_network(net, rates)).eval()


def net_input(net):
    bs, _, edge, _ = HARNESS_CASES[net]
    return det_tensor("input:" + net, [bs, 3, edge, edge])


def outputs_of(model, x):
    with torch.no_grad():
        y = model(x)
    return list(y) if isinstance(y, (tuple, list)) else [y]


def sample_of(t, want):
    return t.detach().double().cpu().reshape(-1)[::want["stride"]][:len(want["sample"])].numpy()


def rel_err(outs, wants):
    """max|got - want| / max|want| over the fixture's subsamples of all outputs."""
    num = max(float(np.abs(sample_of(t, w) - np.asarray(w["sample"])).max()) for t, w in zip(outs, wants))
    den = max(float(np.abs(np.asarray(w["sample"])).max()) for w in wants)
    return num / den


# ---------------------------------------------------------------------------------------------------------
# ResNet-50 with dead mid channels
# ---------------------------------------------------------------------------------------------------------
def dead_resnet_50(modulus=3):
    """A full-width ResNet-50 (seeded) whose mid channels with index % modulus == 0 are dead: zero conv filter,
    zero batch-norm weight and bias, for both convs of mid width in every block. Such a channel is exactly 0 behind
    its ReLU, so the net computes the same with or without it."""
    net = deterministic_init(nets.get_network("resnet_50")).eval()
    sd = net.state_dict()
    with torch.no_grad():
        for conv, bn, _, _, kind in tp.resnet_50_convs():
            if kind != "mid":
                continue
            dead = torch.arange(sd[conv + ".weight"].size(0)) % modulus == 0
            sd[conv + ".weight"][dead] = 0
            sd[bn + ".weight"][dead] = 0
            sd[bn + ".bias"][dead] = 0
    return net


def dead_scores(modulus=3):
    """{stem: scores} for the 53 files: 0.0 at the dead mid channels, positive everywhere else."""
    imp = {}
    for (stem, ori, _), (_, _, _, _, kind) in zip(tp.resnet_50_kept(MID_ONLY), tp.resnet_50_convs()):
        s = 1.0 + np.random.RandomState(ori + len(imp)).rand(ori).astype(np.float32)
        if kind == "mid":
            s[np.arange(ori) % modulus == 0] = 0.0
        imp[stem] = s
    return imp


def restore_downsample(pruned, full):
    """Undo what the reference's loader does to the four downsample convs under mid-only rates (it slices their input
    channels by the kept filters of the block's conv2, utils/load_models.py:547-551): take them whole from `full`."""
    sd, ori = pruned.state_dict(), full.state_dict()
    with torch.no_grad():
        for s in range(1, 5):
            key = "layer%d.0.downsample.0.weight" % s
            sd[key].copy_(ori[key])
    return pruned


def dead_batch():
    from dct_pruning_amd.data import SyntheticLoader
    bs, limit, edge, _ = HARNESS_CASES["resnet_50"]
    loader = SyntheticLoader((3, edge, edge), bs, limit + 1, seed=7)
    return loader, next(iter(loader))[0]
