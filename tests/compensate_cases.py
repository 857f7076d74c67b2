"""What tests/test_compensate_cpu.py and tests/test_compensate_gpu.py share: full-width nets in which
half of every scored conv's filters are copies of kept ones, live nets with random scores, and the calibration batches.

A duplicate-filter net is built from transplant.dataflow. In every conv a score file shrinks at DUP_RATES (VGG: the 12
scored convs; resnet_56: each block's conv1; googlenet: the 3x3 conv and both 5x5-branch convs), each odd filter is a
copy of its left neighbour, bias included, and the batch-norm behind it has the neighbour's running statistics and twice
its weight and bias: behind the ReLU, through pooling, the odd map is exactly 2 x its neighbour's. The odd filters score
0, the even ones in [1, 2), so rate 0.5 removes exactly the copies. carry drops what they fed into the next layer; the
least-squares merge finds x_odd = 2 x_even and gives it back.
"""
import zlib

import numpy as np
import torch

import carry_cases as cc
import pruned_cases as pc
from dct_pruning_amd import nets
from dct_pruning_amd import transplant as tp
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init

DUP_RATES = {
    "vgg_16_bn": [0.5] * 12,
    "resnet_56": [0.0] * 3 + [0.5] * 27,   # stem and stage outputs whole: they end in a residual sum (§7m)
    "googlenet": [0.0] + [0.5] * 9,
}
CALIB_BATCHES, CALIB_BATCH = 2, 64      # 128 calibration samples
CALIB_SEED, FRESH_SEED, FRESH_BATCH = 11, 12, 8


def _edge(name):
    return HARNESS_CASES[name][2]


def calibration(name, batches=CALIB_BATCHES, batch=CALIB_BATCH):
    """The re-iterable loader of the calibration batches (dict batches for U2-Net-p, as the harness's loader gives)."""
    return SyntheticLoader((3, _edge(name), _edge(name)), batch, batches, seed=CALIB_SEED, as_dict=HARNESS_CASES[name][3])


def fresh(name, batch=FRESH_BATCH):
    """A batch no calibration sweep saw: the gaps are measured on it."""
    return next(iter(SyntheticLoader((3, _edge(name), _edge(name)), batch, 1, seed=FRESH_SEED)))[0]


def duplicated(name):
    """[(conv module, batch-norm module behind it, score file stem)] of the convs DUP_RATES[name] shrinks, from the table."""
    table = tp.dataflow(name)
    behind = {f.sources[0][0]: f.module for f in table if f.kind == "bn" and len(f.sources) == 1 and f.sources[0][1] == 0}
    slim = nets.get_network(name, DUP_RATES[name]).state_dict()
    return [(f.module, behind[f.module], f.stem) for f in table
            if f.kind == "conv" and f.stem is not None and slim[f.module + ".weight"].size(0) != f.width]


def duplicate_net(name):
    """(full-width net, float32, eval mode, seeded by deterministic_init, every odd filter of duplicated(name) a copy
    that comes out as 2 x its left neighbour; {stem: scores} with 0 at the odd indices of those files)."""
    net = deterministic_init(nets.get_network(name))
    sd = net.state_dict()
    stems = set()
    with torch.no_grad():
        for conv, bn, stem in duplicated(name):
            stems.add(stem)
            odd = torch.arange(1, sd[conv + ".weight"].size(0), 2)
            for key in [conv + ".weight", bn + ".running_mean", bn + ".running_var"] + ([conv + ".bias"] if conv + ".bias" in sd else []):
                sd[key][odd] = sd[key][odd - 1]
            for key in (bn + ".weight", bn + ".bias"):
                sd[key][odd] = 2 * sd[key][odd - 1]
    imp = {}
    for k, (stem, c) in enumerate(pc.transplant_fixture(name)["stems"]):
        s = 1.0 + np.random.RandomState(c + k).rand(c).astype(np.float32)
        if stem in stems:
            s[1::2] = 0.0
        imp[stem] = s
    return net.eval(), imp


def removed_are_the_copies(name, imp):
    """True where select_index removes exactly the odd filters of every conv DUP_RATES[name] shrinks."""
    table = cc.shrunk(name, DUP_RATES[name])
    return bool(table) and all(np.array_equal(tp.select_index(np.asarray(imp[stem]), o, c), np.arange(0, o, 2)) for stem, o, c in table)


LIVE_SEED = 0


def live_scores(name):
    """{stem: uniform random scores} for every file imp_score writes for `name`."""
    return {stem: np.random.RandomState(zlib.crc32(stem.encode())).rand(c).astype(np.float32)
            for stem, c in pc.transplant_fixture(name)["stems"]}


def live_net(name, init="constructor"):
    """A full-width net with nothing dead and nothing duplicated, float32, eval mode.

    init="constructor": torch.manual_seed(LIVE_SEED), then the constructor - the full net the command-line tool prunes
    when it is given no checkpoint, and the "seeded" net the figures of DESIGN.md §7n were first taken on. torch's default
    initialisation with identity batch-norms lets the activations shrink from layer to layer until the biases carry
    them: the outputs of the VGG move by 6e-6 of their size between inputs, deep maps are close to constant and so
    close to linear in one another.
    init="scaled": helpers.deterministic_init - Kaiming-scaled convs and seeded batch-norm tensors, activations that stay
    alive through the depth. The harder case: the maps of random filters behind a ReLU are far from linear in one another."""
    if init == "scaled":
        return deterministic_init(nets.get_network(name)).eval()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(LIVE_SEED)
        return nets.get_network(name).eval()
