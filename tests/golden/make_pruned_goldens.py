#!/usr/bin/env python3
"""Generate tests/golden/pruned_forward_<net>.json by running the REFERENCE's own pruned models
(models/cifar10/*.py, models/imagenet/resnet.py, models/DUTS/u2net.py through utils/common.get_network) in
this build container: seeded weights (tests/helpers.det_tensor(key, shape, "slim:"), the slim model of the
transplant fixtures), eval(), float64, on the seeded input det_tensor("input:" + net, [batch, 3, edge, edge])
with batch and edge of helpers.HARNESS_CASES. Never runs on the GPU box: the reference does not travel, only
these fixtures do. Same stand-ins for the absent packages as make_harness_goldens.py / make_transplant_goldens.py.

A fixture holds data only. Per rate list: the list, the input shape, a digest of the pruned model's
[(key, shape)] list, and for every output tensor its shape, its sum, its absolute sum and a strided subsample
(every `stride`-th element of the flattened tensor, at most SAMPLES of them) as float64 values; and
`thread_delta`, max|a - b| / max|a| over the outputs between the reference's forward at 1 thread and at the
default thread count: what summation order alone moves in float64.

Two rate lists per net: "readme", make_transplant_goldens.CASES, and "extra", which reaches what the README's
list leaves out (EXTRA below says what). tests/test_pruned_nets_cpu.py and tests/test_pruned_nets_gpu.py rebuild
the same weights and input from the seeds, run dct_pruning_amd.nets.get_network(net, rates) and compare.

usage: python tests/golden/make_pruned_goldens.py [net ...]
"""
import hashlib
import json
import os
import sys
import types
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from helpers import HARNESS_CASES, det_tensor  # noqa: E402
from make_transplant_goldens import CASES, fill  # noqa: E402

SAMPLES = 96

EXTRA = {
    # net: (what the list reaches that the README's does not, rate list)
    "vgg_16_bn": ("full-width layers behind pruned ones (convs 2, 3, 5, 7, 8, 10, 12), uneven rates",
                  [0.3, 0.0, 0.0, 0.5, 0.0, 0.25, 0.0, 0.0, 0.6, 0.0, 0.1, 0.0]),
    "resnet_56": ("a stem narrower than stage 1 by an odd count (9 -> 16: a real PAD at stride 1, 3 in front and 4 behind), "
                  "an odd CROP at stride 2 (16 -> 13), an odd pad at stride 2 (13 -> 64), full-width first convs between "
                  "pruned ones",
                  [0.4, 0.0, 0.58] + [0.0, 0.5] * 13 + [0.3]),
    "resnet_110": ("an even crop at stride 1 (11 -> 9), an odd positive pad at stride 2 (9 -> 28), stage 2 pruned on its "
                   "output, one first-conv rate for the whole net",
                   [0.3, 0.4, 0.1] + [0.25] * 54),
    "densenet_40": ("pruned transitions (0.3, 0.45), a different growth per layer in block 1, a growth of 6 in block 2 and "
                    "a full-width block 3 behind them",
                    [0.0] + [0.1 * (i % 5) for i in range(12)] + [0.3] + [0.5] * 12 + [0.45] + [0.0] * 12),
    "googlenet": ("full-width blocks between pruned ones, a different rate per block, the last block's rule (its middle "
                  "5x5-branch conv shrinks, its outputs do not) behind a full-width block",
                  [0.0, 0.3, 0.0, 0.5, 0.25, 0.0, 0.6, 0.1, 0.0, 0.7]),
    "resnet_50": ("mid channels only: every block output and the stem at full width, so all identity shortcuts and "
                  "downsamples keep their shapes",
                  [0.0] * 4 + [0.25] * 16),
    "u2netp": ("a different rate per unit, the floor of one channel (rates 0.95 ... 0.97 of 16), full-width units next to "
               "pruned ones, five different outer widths",
               [0.0, 0.5, 0.95, 0.25, 0.0] + [0.97, 0.0, 0.5, 0.3] + [0.2, 0.0, 0.6] + [0.5, 0.0] + [0.0, 0.3] + [0.96, 0.2]
               + [0.1, 0.2, 0.3, 0.4, 0.5] + [0.5, 0.4, 0.3, 0.2] + [0.0, 0.95, 0.1] + [0.3, 0.0] + [0.25, 0.75]
               + [0.1, 0.3, 0.0, 0.5, 0.2]),
}


def keys_digest(sd):
    return hashlib.sha256(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode()).hexdigest()[:20]


def outputs_of(net, x):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = net(x)
    return list(y) if isinstance(y, (tuple, list)) else [y]


def describe(t):
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SAMPLES)
    return {"shape": list(t.shape), "sum": float(flat.sum()), "abs_sum": float(flat.abs().sum()), "stride": stride,
            "sample": [float(v) for v in flat[::stride][:SAMPLES]]}


def main(nets):
    from make_harness_goldens import _install_stand_ins
    _install_stand_ins()
    sys.path.insert(0, REF)
    import utils.common as rc
    default_threads = torch.get_num_threads()
    for name in nets:
        bs, _, edge, _ = HARNESS_CASES[name]
        shape = [bs, 3, edge, edge]
        x = det_tensor("input:" + name, shape).double()
        cases = []
        for tag, reaches, rates in (("readme", "the README's rate list", CASES[name]), ("extra",) + EXTRA[name]):
            net = fill(rc.get_network(types.SimpleNamespace(net=name), list(rates)), "slim:").cpu().eval().double()
            torch.set_num_threads(1)
            one = outputs_of(net, x)
            torch.set_num_threads(default_threads)
            outs = outputs_of(net, x)
            delta = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(one, outs))
            cases.append({"name": tag, "reaches": reaches, "rates": [float(r) for r in rates], "input_shape": shape,
                          "keys_digest": keys_digest(net.state_dict()), "threads": [1, default_threads],
                          "thread_delta": delta, "outputs": [describe(t) for t in outs]})
            print("%s/%s: %d outputs, thread_delta %.3g" % (name, tag, len(outs), delta), flush=True)
        path = os.path.join(HERE, "pruned_forward_%s.json" % name)
        json.dump({"net": name, "cases": cases}, open(path, "w"))
        assert os.path.getsize(path) < 100 * 1024, path


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
