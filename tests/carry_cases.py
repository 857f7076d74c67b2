"""What tests/test_carry_cpu.py and tests/test_carry_gpu.py share: full-width nets with dead filters, the rate lists
that remove only dead filters, and score dicts with 0.0 at the dead indices.

The dead nets are built from the full net's own modules and from the tables transplant.py had before the carry mode
(the *_kept and *_convs functions), not from transplant.dataflow: the tests check that table against them.

Dead means index % 4 == 0 of a conv whose rows a score file selects at the rates below.
  * Post-activation nets (conv - batch-norm - ReLU: VGG, GoogLeNet's 3x3 and 5x5-branch convs, the ResNets' mid convs,
    U2-Net-p's units of inner width): zero filter, zero conv bias, zero batch-norm weight and bias. The channel is exactly
    0 behind its ReLU, and stays 0 through pooling and bilinear up-sampling.
  * DenseNet (batch-norm - ReLU - conv): zero filter, and at that channel's position running mean 0 and bias 0 in every
    batch-norm that later reads the concatenation: the following dense layers of the block and the transition or the
    final `bn` that closes it; for a transition's filter, every batch-norm of the next block. The channel is exactly 0
    where it is written (and behind the transition's average pool) and exactly 0 behind each reader's ReLU.
"""
import numpy as np
import torch
import torch.nn as nn

import pruned_cases as pc
from dct_pruning_amd import nets
from dct_pruning_amd import transplant as tp
from helpers import deterministic_init

MOD = 4
RATES = {
    "vgg_16_bn": [0.25] * 12,                                                     # C / 4 go: exactly the dead set
    "googlenet": [0.0] + [0.25] * 9,                                              # every 3x3 / 5x5 width divides by 4
    "densenet_40": [0.0] + [0.25] * 12 + [0.0] + [0.25] * 12 + [0.0] + [0.25] * 12,  # growth 12 -> 9; transitions lose 36 of 168
    "resnet_56": [0.0] * 3 + [0.25] * 27,                                         # and 72 of 312, inside the 42 and 78 dead
    "resnet_110": [0.0] * 3 + [0.25] * 54,
    "resnet_50": pc.MID_ONLY,
    "u2netp": [0.25] * 34 + [0.0] * 5,
}


def _kill(sd, conv, bn):
    dead = torch.arange(sd[conv + ".weight"].size(0)) % MOD == 0
    sd[conv + ".weight"][dead] = 0
    if conv + ".bias" in sd:
        sd[conv + ".bias"][dead] = 0
    sd[bn + ".weight"][dead] = 0
    sd[bn + ".bias"][dead] = 0


def dead_convs(name, net):
    """[(conv module, batch-norm module behind it, score file stem)] of a post-activation net, from its modules."""
    convs = [n for n, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    if name == "vgg_16_bn":  # features.conv<i> / features.norm<i>, file k for the k-th conv; the 13th has none and keeps its width
        feats = [n for n in convs if n.startswith("features.")]
        return [(n, n.replace("conv", "norm"), "imp_conv%d" % (k + 1)) for k, n in enumerate(feats[:-1])]
    if name == "googlenet":
        out = []
        for b, blk in enumerate(tp.GOOGLENET_BLOCKS):
            out += [(blk + ".branch3x3.3", blk + ".branch3x3.4", "imp_conv%d_n3x3" % (b + 2)),
                    (blk + ".branch5x5.3", blk + ".branch5x5.4", "imp_conv%d_n5x5" % (b + 2)),  # one file, two convs:
                    (blk + ".branch5x5.6", blk + ".branch5x5.7", "imp_conv%d_n5x5" % (b + 2))]  # the same indices dead
        return out
    if name in ("resnet_56", "resnet_110"):
        return [(conv, conv.replace(".conv", ".bn"), stem) for conv, stem, _, kind in tp.resnet_cifar_convs(int(name[7:]))
                if kind == "mid"]
    if name == "resnet_50":
        return [(conv, bn, "imp_conv%d" % (k + 1)) for k, (conv, bn, _, _, kind) in enumerate(tp.resnet_50_convs()) if kind == "mid"]
    if name == "u2netp":  # every unit of inner width (16): net.<unit>.relu_s1
        return [(n, n[:-len("conv_s1")] + "bn_s1", "net." + n[:-len("conv_s1")] + "relu_s1") for n in convs
                if n.endswith(".conv_s1") and net.get_submodule(n).out_channels == 16]
    raise ValueError(name)


def _dead_densenet(net):
    sd = net.state_dict()
    stems = []
    cov_id = 1
    for b in (1, 2, 3):
        layers = list(getattr(net, "dense%d" % b))
        closing = "trans%d.bn1" % b if b < 3 else "bn"
        for j, layer in enumerate(layers):
            cov_id += 1
            stems.append("imp_conv%d" % cov_id)
            conv = "dense%d.%d.conv1" % (b, j)
            dead = torch.arange(layer.conv1.out_channels) % MOD == 0
            sd[conv + ".weight"][dead] = 0
            pos = layer.conv1.in_channels + torch.nonzero(dead).flatten()  # where torch.cat puts this conv's filters
            for reader in ["dense%d.%d.bn1" % (b, k) for k in range(j + 1, len(layers))] + [closing]:
                sd[reader + ".running_mean"][pos] = 0
                sd[reader + ".bias"][pos] = 0
        if b < 3:
            cov_id += 1
            stems.append("imp_conv%d" % cov_id)
            conv = "trans%d.conv1" % b
            pos = torch.nonzero(torch.arange(sd[conv + ".weight"].size(0)) % MOD == 0).flatten()
            sd[conv + ".weight"][pos] = 0
            nxt = "dense%d" % (b + 1)
            for reader in ["%s.%d.bn1" % (nxt, k) for k in range(len(getattr(net, nxt)))] + ["trans%d.bn1" % (b + 1) if b < 2 else "bn"]:
                sd[reader + ".running_mean"][pos] = 0
                sd[reader + ".bias"][pos] = 0
    return stems


def dead_net(name, calibrate_on=None):
    """(full-width net in eval mode, float32, seeded by deterministic_init; the score file stems with dead indices).

    calibrate_on: a batch whose statistics every batch-norm's running mean and variance are set to (one forward pass in
    training mode with momentum 1), as a trained net's are to its data. Behind such a batch-norm a live channel is
    standardised over the batch, so it is positive somewhere and has energy: without this, seeded running statistics
    leave some live channels at exactly 0 on a small batch (173 of VGG's on the HARNESS_CASES batches), their scores tie
    with the dead ones' and select_index may remove a live filter. The dead indices stay exactly dead: a zero channel
    has batch mean 0, and the rules above do not read the variance."""
    net = deterministic_init(nets.get_network(name))
    with torch.no_grad():
        if name == "densenet_40":
            stems = _dead_densenet(net)
        else:
            sd = net.state_dict()
            table = dead_convs(name, net)
            for conv, bn, _ in table:
                _kill(sd, conv, bn)
            stems = sorted({stem for _, _, stem in table})
        if calibrate_on is not None:
            norms = [m for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
            for m in norms:
                m.momentum = 1.0
            net.train()(calibrate_on)
            for m in norms:
                m.momentum = 0.1
                m.num_batches_tracked.zero_()
    return net.eval(), stems


def dead_scores(name, dead_stems):
    """{stem: scores} for every file imp_score writes for `name`: 0.0 at index % 4 == 0 of the files in `dead_stems`,
    in [1, 2) everywhere else."""
    imp = {}
    for k, (stem, c) in enumerate(pc.transplant_fixture(name)["stems"]):
        s = 1.0 + np.random.RandomState(c + k).rand(c).astype(np.float32)
        if stem in dead_stems:
            s[np.arange(c) % MOD == 0] = 0.0
        imp[stem] = s
    return imp


def shrunk(name, rates):
    """[(score file stem, original width, kept width)] of the convs that lose filters at `rates`, from the width
    tables (for U2-Net-p from u2netp_conv_shapes; GoogLeNet's _n5x5 file once per conv it serves)."""
    if name == "u2netp":
        full = {n: o for n, o, _ in tp.u2netp_conv_shapes([0.0] * 39)}
        rows = [("net." + n[:-len("conv_s1")] + "relu_s1", full[n], o) for n, o, _ in tp.u2netp_conv_shapes(rates)
                if n.endswith(".conv_s1")]
    elif name == "googlenet":
        rows = []
        for i, (w, f) in enumerate(zip(tp.googlenet_widths(rates), tp.GOOGLENET_FILTERS)):
            rows += [("imp_conv%d_n3x3" % (i + 2), f[1], w[1]), ("imp_conv%d_n5x5" % (i + 2), f[2], w[2]),
                     ("imp_conv%d_n5x5" % (i + 2), f[2], w[3])]
    elif name in ("resnet_56", "resnet_110"):
        overall, _ = tp.resnet_cifar_widths(rates, int(name[7:]))
        rows = [("imp_conv1", 16, overall[0])] + tp.resnet_cifar_kept(rates, int(name[7:]))
    else:
        rows = {"vgg_16_bn": tp.vgg_16_bn_kept, "densenet_40": tp.densenet_40_kept, "resnet_50": tp.resnet_50_kept}[name](rates)
    return [(stem, o, c) for stem, o, c in rows if o != c]


def removed_not_dead(imp, name, rates, dead_stems):
    """The (stem, index) pairs select_index removes although they are not dead: [] is what the equivalence needs."""
    bad = []
    for stem, o, c in shrunk(name, rates):
        scores = imp(stem) if callable(imp) else imp[stem]
        gone = np.setdiff1d(np.arange(o), tp.select_index(np.asarray(scores), o, c))
        bad += [(stem, int(i)) for i in gone if stem not in dead_stems or i % MOD != 0]
    return bad


# ---------------------------------------------------------------------------------------------------------
# score -> prune -> run
# ---------------------------------------------------------------------------------------------------------
# Of the synthetic batches. Chosen on the CPU with the oracle as the energy operator (test_carry_cpu.py keeps that check):
# with it no live filter of the five GPU nets scores exactly 0, so every index the rates remove is dead. Seed 7, which
# the other harness tests use, leaves a live U2-Net-p unit (stage1d.rebnconv6d, 3 x 3 maps, batch 1) at 0 and tied.
SEED = 2


def batches(name):
    """(the SyntheticLoader of the HARNESS_CASES batches, its first batch's images)."""
    from dct_pruning_amd.data import SyntheticLoader
    from helpers import HARNESS_CASES
    bs, limit, edge, as_dict = HARNESS_CASES[name]
    loader = SyntheticLoader((3, edge, edge), bs, limit + 1, seed=SEED, as_dict=as_dict)
    first = next(iter(loader))
    return loader, first["image"] if as_dict else first[0]


def score(name, full, root):
    """imp_score(single_sweep=True) of `full` (where it lives) on the HARNESS_CASES batches, files under `root`:
    the score directory."""
    import contextlib
    import io
    import os
    import types
    from dct_pruning_amd import harness
    from helpers import HARNESS_CASES
    bs, limit, _, _ = HARNESS_CASES[name]
    loader, _ = batches(name)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(full, args, train_loader=loader, single_sweep=True)
    finally:
        os.chdir(cwd)
    return os.path.join(str(root), "importance_score", "%s_limit%d" % (name, limit))


def error_against(outs, wants):
    """max|got - want| / max|want| over all outputs, `wants` in float64 on the CPU."""
    num = max(float((t.detach().double().cpu() - w).abs().max()) for t, w in zip(outs, wants))
    return num / max(float(w.abs().max()) for w in wants)
