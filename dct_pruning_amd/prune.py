"""From score files to a runnable pruned network - the last step of the path:

    python importance_generation.py --net resnet_56 --pretrain_dir checkpoints/resnet_56.pt --limit 5
    python -m dct_pruning_amd.prune --net resnet_56 --pretrain_dir checkpoints/resnet_56.pt \\
        --imp_score importance_score/resnet_56_limit5 --compress_rate '[0.]+[0.18]*29' --out resnet_56_pruned.pt

prune_network builds the slim architecture (nets.get_network with the rate list), runs that net's weight-transplant
loader (transplant.py) on the slim net's own state dict and loads the result back with strict=True; cost counts what
the pruning saved. What comes out is what the reference's prune_*.py hold right after load_model (utils/load_models.py
:775-830) and before their first fine-tuning epoch: fine-tuning, datasets and evaluation stay with the user.

--carry (prune_network(..., carry=True)) is the second mode, for a net that runs before any fine-tuning, for all seven
architectures: the same rows by the same score files, columns by the data flow of the forward pass
(transplant.dataflow), conv biases and batch-norm tensors with their channels, everything else brought over; the tool then
prints output_gap(full, pruned, x) on one synthetic batch as a third line. The default mode is untouched by it.

--carry --compensate (prune_network(..., carry=True, moments=...)) goes one step further (compensate.py): carry
drops what a removed filter fed into the next layer, which is exact for dead filters only. The tool sweeps --calib_batches
batches of --batch_size samples through the full net once (compensate.collect_moments: the second moments of every consumer's
input), fits each removed input channel as a linear combination of the kept ones and folds the fit into the consumer's
weights; no bias or batch-norm tensor changes. A fourth line reports the gap after the merge, on the third line's batch,
and the largest residual of the fits.

The tool needs no GPU: the transplant is index_select on whatever device the tensors live on.
"""
import argparse
import sys
import types

import torch
import torch.nn as nn

from . import nets
from . import transplant as _tp
from .masks import parse_compress_rate

LOADERS = {
    "vgg_16_bn": _tp.transplant_vgg,
    "resnet_56": lambda sd, ori, imp: _tp.transplant_resnet_cifar(sd, ori, imp, 56),
    "resnet_110": lambda sd, ori, imp: _tp.transplant_resnet_cifar(sd, ori, imp, 110),
    "densenet_40": _tp.transplant_densenet_40,
    "googlenet": _tp.transplant_googlenet,
    "resnet_50": _tp.transplant_resnet_50,
    "u2netp": _tp.transplant_u2netp,
}


def prune_network(name, full, imp_score, compress_rate, exact=False, carry=False, moments=None, rtol=1e-10):
    """The pruned `name` (an nn.Module in training mode, as constructed) with the kept filters of `full`.

    full: the full-width module or its state dict; imp_score: a score directory or a {file stem: scores} dict, as the
    loaders of transplant.py take; compress_rate: the reference's rate list (nets.RATE_LEN[name] entries at least,
    ValueError otherwise). The slim net is built on the device and in the floating dtype of `full`'s tensors, its own
    state dict goes through the net's loader, and the result is loaded back with strict=True. A missing score file
    raises FileNotFoundError (KeyError for a dict), one whose length is not its convolution's filter count ValueError.

    The loaders copy what the reference's loaders copy, no more. Tensors they leave alone keep the slim net's OWN
    INITIALISATION, which comes from torch's global generator: seed it (torch.manual_seed) before the call if the result
    has to be reproducible. Those are
      * vgg_16_bn: every conv bias and batch-norm tensor, and the classifier;
      * resnet_56 / resnet_110: every batch-norm tensor;
      * densenet_40: conv1, every batch-norm tensor and the classifier;
      * googlenet: pre_layers, every conv bias and the batch-norms behind the pruned convs;
      * u2netp: every conv bias and batch-norm tensor, and outconv.
    Only resnet_50 carries its batch-norms over with the kept filters, so it is the only net whose pruned model is
    usable before fine-tuning; the others are starting points for it. For that to hold, one thing is NOT the
    reference's here: its loader selects the INPUT channels of each stage's downsample conv by the kept filters of that
    block's conv2 (the loop's last index at that point, utils/load_models.py:525-529, :547-551), although the conv reads
    the block's input; prune_network selects them by the kept filters of what feeds the block
    (transplant_resnet_50(..., downsample_input="block")). With dead filters pruned from the mid channels the result then
    computes what the full net computes; with the reference's choice it differs by 58 % of the largest output
    (tests/test_pruned_nets_cpu.py). exact=True gives the reference's state dict bit for bit, for resnet_50 too.

    carry=True is the second mode (transplant.transplant_carry), for a net that runs before any
    fine-tuning, for all seven: rows as above, by the same score files and so with the same masks; a module's input
    channels by the kept filters of whatever feeds it in the forward pass (transplant.dataflow(name): concatenations in
    torch.cat order at the original offsets, GoogLeNet's included; after a residual sum the kept list of the block's last
    conv; the block input for ResNet-50's downsample convs); conv biases and batch-norm tensors with their channels;
    stems, pre_layers, classifiers, side convs and outconv brought over, a Linear behind pruned features with their
    kept list as its columns. No tensor keeps its initialisation, so the result does not depend on torch's seed; a conv
    that kept its width reads no score file, and nothing raises because the reference's control flow would have.
    With only dead filters removed the result computes what the full net computes wherever the architecture allows it:
    every rate of vgg_16_bn, googlenet and densenet_40, the mid-channel rates of the three ResNets, the 34 inner rates
    of u2netp. It cannot for a width that ends in a residual sum - the ResNets' stage outputs, the CIFAR stems with their
    positional pad-or-crop shortcut, u2netp's five outer widths (d + xin): there each writer of the stream has a kept
    list of its own, from a score file of its own, and the columns follow the last main-path writer. carry=True with
    exact=True raises ValueError.

    moments (with carry=True; ValueError without) compensates the prune: compensate.collect_moments(name,
    full, batches, compress_rate) gives the second moments of every consumer's input over a few calibration batches, and
    compensate.compensate then adds to each consumer's kept columns the least-squares image of the removed ones,
    W_S + W_D M_DS pinv(M_SS, rtol). A removed filter whose map is a linear combination of kept maps then goes without a
    trace too, not only a dead one; consumer weights change, nothing else. With moments=None the result is carry's."""
    if name not in LOADERS:
        raise ValueError("the network name you have entered is not supported yet: %r" % (name,))
    if carry and exact:
        raise ValueError("prune_network: carry=True and exact=True exclude each other (exact is the reference's state dict)")
    if moments is not None and not carry:
        raise ValueError("prune_network: moments compensate the carry mode, pass carry=True with them")
    ori = full.state_dict() if isinstance(full, nn.Module) else full
    like = next((t for t in ori.values() if t.is_floating_point()), None)
    if like is None:
        raise ValueError("prune_network: `full` holds no floating-point tensor")
    net = nets.get_network(name, compress_rate).to(device=like.device, dtype=like.dtype)
    with torch.no_grad():
        if carry:
            sd = _tp.transplant_carry(name, net.state_dict(), ori, imp_score)
        elif name == "resnet_50" and not exact:
            sd = _tp.transplant_resnet_50(net.state_dict(), ori, imp_score, downsample_input="block")
        else:
            sd = LOADERS[name](net.state_dict(), ori, imp_score)
        net.load_state_dict(sd, strict=True)
    if moments is not None:
        from .compensate import compensate
        compensate(name, net, ori, imp_score, moments, rtol=rtol)
    return net


def cost(net, input_shape):
    """{"params": int, "macs": int} of one forward pass on one (C, H, W) input.

    params: numel over net.parameters(). macs: multiply-accumulates of the Conv2d and Linear modules only - output
    elements x (C_in / groups x kh x kw), or output elements x in_features - counted by forward hooks on one zero batch
    of size 1 in eval mode (the training flag is put back), so the spatial sizes are the ones the net really produces.
    Bias adds, batch-norms, pooling, interpolation and activations count as nothing. Exact Python integers."""
    macs = [0]

    def hook(mod, inputs, output):
        if isinstance(mod, nn.Conv2d):
            per_out = mod.in_channels // mod.groups * mod.kernel_size[0] * mod.kernel_size[1]
        else:
            per_out = mod.in_features
        macs[0] += output.numel() * per_out

    handles = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    like = next(net.parameters())
    training = net.training
    net.eval()
    try:
        with torch.no_grad():
            net(torch.zeros((1,) + tuple(input_shape), device=like.device, dtype=like.dtype))
    finally:
        for h in handles:
            h.remove()
        net.train(training)
    return {"params": sum(p.numel() for p in net.parameters()), "macs": macs[0]}


def output_gap(full, pruned, x):
    """max|pruned(x) - full(x)| / max|full(x)| over all outputs (a float): both nets in eval mode and under no_grad, their
    training flags put back. 0 where the pruning changed nothing the input can show."""
    flags = full.training, pruned.training
    full.eval()
    pruned.eval()
    try:
        with torch.no_grad():
            want, got = full(x), pruned(x)
    finally:
        full.train(flags[0])
        pruned.train(flags[1])
    want = list(want) if isinstance(want, (tuple, list)) else [want]
    got = list(got) if isinstance(got, (tuple, list)) else [got]
    num = max(float((g - w).abs().max()) for g, w in zip(got, want))
    return num / max(float(w.abs().max()) for w in want)


def _report(tag, name, c, base=None):
    line = "%s %s: params %d, MACs %d" % (tag, name, c["params"], c["macs"])
    if base is not None:
        line += ", reduction %.2f %% params, %.2f %% MACs" % (100.0 * (1 - c["params"] / base["params"]),
                                                              100.0 * (1 - c["macs"] / base["macs"]))
    return line


def main(argv=None):
    from .data import INPUT_SHAPES, NET_DATASET
    ap = argparse.ArgumentParser(prog="python -m dct_pruning_amd.prune", description=__doc__.split("\n")[0])
    ap.add_argument("--net", required=True, choices=tuple(LOADERS), help="net type")
    ap.add_argument("--imp_score", required=True, help="directory of score files (importance_score/<net>_limit<L>)")
    ap.add_argument("--compress_rate", required=True, help="reference DSL, e.g. '[0.]+[0.18]*29'")
    ap.add_argument("--pretrain_dir", default=None, help="checkpoint of the full-width net (default: its seeded initialisation)")
    ap.add_argument("--input_size", type=int, default=None, help="H=W of the input the MACs are counted on (default: the dataset's)")
    ap.add_argument("--seed", type=int, default=0, help="seeds what the loaders do not copy (and the full net without a checkpoint)")
    ap.add_argument("--exact", action="store_true",
                    help="resnet_50: select the downsample convs' input channels as the reference's loader does (by conv2's kept "
                         "filters) instead of by the block input's")
    ap.add_argument("--carry", action="store_true",
                    help="columns by data flow, biases and batch-norms with their channels, everything else brought over: a net "
                         "that runs before fine-tuning (all seven nets); prints max|pruned - full| / max|full| on one "
                         "synthetic batch seeded by --seed as a third line")
    ap.add_argument("--compensate", action="store_true",
                    help="with --carry: fit every removed input channel as a linear combination of the kept ones on calibration "
                         "batches and fold the fit into the consumer's weights; prints the gap after it and the largest "
                         "residual as a fourth line")
    ap.add_argument("--calib_batches", type=int, default=4, help="--compensate: number of calibration batches")
    ap.add_argument("--batch_size", type=int, default=64, help="--compensate: samples per calibration batch")
    ap.add_argument("--synthetic", action="store_true", help="--compensate: synthetic batches of the dataset's shape, seeded by --seed + 1 (not the gap's batch)")
    ap.add_argument("--dataset", default=None, choices=("cifar10", "imagenet", "DUTS", "synthetic"),
                    help="--compensate: where the calibration batches come from (default: the net's dataset)")
    ap.add_argument("--data_dir", default="./data", help="--compensate: path to the dataset")
    ap.add_argument("--out", required=True,
                    help="torch.save target: {'net', 'compress_rate', 'carry', 'compensate', 'state_dict'}")
    args = ap.parse_args(argv)
    if args.carry and args.exact:
        ap.error("--carry and --exact exclude each other")
    if args.compensate and not args.carry:
        ap.error("--compensate needs --carry")
    if args.compensate and args.calib_batches < 1:
        ap.error("--calib_batches is at least 1")
    torch.manual_seed(args.seed)
    try:
        rates = parse_compress_rate(args.compress_rate)
        full = nets.get_network(args.net)
        if args.pretrain_dir:
            nets.load_checkpoint(full, types.SimpleNamespace(net=args.net, pretrain_dir=args.pretrain_dir))
        pruned = prune_network(args.net, full, args.imp_score, rates, exact=args.exact, carry=args.carry)
    except (ValueError, OSError) as exc:  # short rate list, wrong-length or missing score file, unreadable checkpoint
        ap.error(str(exc))
    shape = list(INPUT_SHAPES[NET_DATASET[args.net]])
    if args.input_size:
        shape[1] = shape[2] = args.input_size
    base = cost(full, shape)
    print(_report("full  ", args.net, base))
    print(_report("pruned", args.net, cost(pruned, shape), base))
    if args.carry:
        from .data import SyntheticLoader
        x = next(iter(SyntheticLoader(shape, 2, 1, seed=args.seed)))[0]
        print("gap    %s: max|pruned - full| / max|full| %.3g on one synthetic batch" % (args.net, output_gap(full, pruned, x)))
    if args.compensate:
        import itertools
        from . import compensate as _cp
        from .data import load_data
        try:  # synthetic batches by --seed + 1: the batch the gaps are taken on is not among them
            loader, _ = load_data(types.SimpleNamespace(
                net=args.net, dataset=args.dataset or NET_DATASET[args.net], synthetic=args.synthetic, data_dir=args.data_dir,
                batch_size=args.batch_size, limit=args.calib_batches, input_size=args.input_size, seed=args.seed + 1))
        except RuntimeError as exc:  # a real dataset without torchvision
            ap.error(str(exc))
        moments = _cp.collect_moments(args.net, full, itertools.islice(loader, args.calib_batches), rates)
        merged = _cp.compensate(args.net, pruned, full, args.imp_score, moments)
        print("merged %s: max|pruned - full| / max|full| %.3g on the same batch, largest residual %.3g over %d modules"
              % (args.net, output_gap(full, pruned, x), max([m.residual for m in merged] + [0.0]), len(merged)))
    torch.save({"net": args.net, "compress_rate": rates, "carry": bool(args.carry), "compensate": bool(args.compensate),
                "state_dict": {k: v.detach().cpu() for k, v in pruned.state_dict().items()}}, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
