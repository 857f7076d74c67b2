"""Weight transplant from the full-width network into the pruned one - the step right after the
score path, vectorised.

The reference walks the convolutions in order, derives the kept filters of each from its score file
    select_index = np.argsort(imp)[orifilter_num - currentfilter_num:]; select_index.sort()
and copies weights one scalar slice at a time in Python double / triple loops
(utils/load_models.py:17-64 for VGG-16-bn, :67-143 for the CIFAR ResNets, :385-438 for DenseNet-40,
:441-582 for ResNet-50: ~10^7 interpreter-level copies for ResNet-50). Here every such loop is one index_select on the output-filter axis, one on the
input-channel axis (the previous layer's kept filters) and one assignment: same result, bit for
bit, on whatever device the tensors live on.

Quirks kept because the result must equal the reference's state dict:
  * VGG: only conv `.weight` tensors are transplanted; conv biases and batch-norm tensors of the
    slim model stay as the caller's state dict has them (utils/load_models.py:43-61 never touches them);
  * VGG: once a layer keeps its full width and the previous layer did too, `last_select_index` is
    reset; a full-width layer after a pruned one gets its input channels sliced and the index
    stays as it was (:55-61);
  * ResNet-50: the downsample conv of a stage's first block does not update `last_select_index`
    (record_last = False, :506), batch-norm tensors follow the conv's kept filters, and every
    `num_batches_tracked` is copied (:560); the downsample conv's INPUT channels are therefore selected by the
    kept filters of the block's conv2, not of the block's input (downsample_input="block" selects by the latter:
    not the reference, what prune.prune_network uses).

  * CIFAR ResNet-56/110: only `layerX.k.conv1/conv2` weights are transplanted (score files
    imp_conv2 ... - the counter starts at 1 and is incremented before use, :80, :89); a full-width conv
    after a pruned one gets its input channels sliced and then RESETS the index (:123); the stem
    conv and the linear layer come over whole, batch-norm tensors are never touched (:129-141);
  * DenseNet-40: `last_select_index` starts as an EMPTY LIST, not None (:388), so the "no previous
    index" branches are unreachable and the first conv copies nothing at all - conv1 keeps the slim
    model's own weights; after every conv the kept filters are appended at the position the
    concatenated feature map gives them in the ORIGINAL network (offset cov_id*12 - (cov_id-1)//13*12,
    :435), restarted after conv1 and after each transition (cov_id 1, 14, 27, :432); neither
    batch-norm tensors nor the classifier are copied;
  * GoogLeNet: inside an Inception block only the 3x3 conv and the two 5x5-branch convs lose filters
    (score files imp_conv<id>_n3x3 / _n5x5, the latter read for both 5x5-branch convs, :264, :313); the
    four entry convs get their input channels sliced by the previous block's kept list, which is
    assembled in the order [1x1, pool, 3x3, 5x5] (:233-242, :275-277, :320-322) - not the order
    torch.cat uses - with offsets from the ORIGINAL filter table; every conv of the net is on the
    "sketch" list, so no conv bias is ever copied and `pre_layers.0` (never pruned by the constructor)
    keeps the slim model's own weights; the batch-norms behind pruned convs and `pre_layers.1` are not
    copied either, the other batch-norms (four tensors, not num_batches_tracked) and the linear layer
    come over whole (:361-380).

  * U^2-Net-p: only conv weights are written, and the control flow raises for ordinary rate lists: with every rate 0 a
    stage starts with no live index and list(None) is evaluated (:617 / :621); with inner widths pruned only, the first
    decoder stage's un-pruned rebnconvin behind a pruned unit evaluates int('i') (:658).

Beside these loaders stands the carry mode (dataflow, transplant_carry, at the end of this file): the same rows
by the same score files, but input channels by the data flow of nets.py's forward passes, per-channel tensors with their
channels and every other tensor brought over - one table per net and one copy routine, none of the quirks above.

Widths of the pruned networks (what `currentfilter_num` is) follow the model constructors:
models/cifar10/vgg.py:37, models/cifar10/resnet.py:5-30 and models/imagenet/resnet.py:8-27 (adapt_channel),
models/cifar10/densenet.py:71-75, :91-104, models/cifar10/googlenet.py:28-66, :147-149.
"""
import functools
import math
import os
from collections import namedtuple

import numpy as np
import torch

from .masks import select_index

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]  # models/cifar10/vgg.py:5
RESNET50_STAGE_REPEAT = [3, 4, 6, 3]                                                                # models/imagenet/resnet.py:3
RESNET50_STAGE_OUT = [64] + [256] * 3 + [512] * 4 + [1024] * 6 + [2048] * 3                         # :4
RESNET_CIFAR_REPEAT = {56: [9, 9, 9], 110: [18, 18, 18]}                                           # models/cifar10/resnet.py:7-12
DENSENET40_GROWTH, DENSENET40_BLOCK = 12, 12                                                        # models/cifar10/densenet.py:53, :58
GOOGLENET_FILTERS = [[64, 128, 32, 32], [128, 192, 96, 64], [192, 208, 48, 64], [160, 224, 64, 64], [128, 256, 64, 64],
                     [112, 288, 64, 64], [256, 320, 128, 128], [256, 320, 128, 128], [384, 384, 128, 128]]  # utils/load_models.py:149-159
GOOGLENET_BLOCKS = ["inception_a3", "inception_b3", "inception_a4", "inception_b4", "inception_c4", "inception_d4",
                    "inception_e4", "inception_a5", "inception_b5"]                                  # models/cifar10/googlenet.py:171-184
_BN_PARTS = [".weight", ".bias", ".running_mean", ".running_var"]


def vgg_16_bn_widths(compress_rate):
    """Output channels of the 13 convolutions (models/cifar10/vgg.py:18-19, :37: the rate list gets a
    trailing 0.0, so the 13th conv keeps its width)."""
    rates = list(compress_rate) + [0.0]
    widths, cnt = [], 0
    for x in VGG_CFG:
        if x == "M":
            continue
        widths.append(int(x * (1 - rates[cnt])))
        cnt += 1
    return widths


def resnet_50_widths(compress_rate):
    """(overall_channel, mid_channel) of models/imagenet/resnet.py:8-27."""
    rates = list(compress_rate)
    stage_oup = [rates[0]]
    for i in range(len(RESNET50_STAGE_REPEAT) - 1):
        stage_oup += [rates[i + 1]] * RESNET50_STAGE_REPEAT[i]
    stage_oup += [0.0] * RESNET50_STAGE_REPEAT[-1]
    mid_rates = rates[len(RESNET50_STAGE_REPEAT):]
    overall, mid = [], []
    for i, c in enumerate(RESNET50_STAGE_OUT):
        overall.append(int(c * (1 - stage_oup[i])))
        if i > 0:
            mid.append(int(c // 4 * (1 - mid_rates[i - 1])))
    return overall, mid


@functools.lru_cache(None)  # the rate solver (rates.py) asks thousands of times: callers read the list, none writes it
def resnet_50_convs():
    """The convolutions in the order load_resnet_imagenet_model visits them (utils/load_models.py:457-512):
    (conv name, bn name, record_last, block index or None, kind) with kind in
    {'stem', 'mid', 'downsample', 'out'}; score file k+1 belongs to entry k."""
    convs = [("conv1", "bn1", True, None, "stem")]
    blk = 0
    for layer, num in enumerate(RESNET50_STAGE_REPEAT):
        for k in range(num):
            base = "layer%d.%d." % (layer + 1, k)
            convs.append((base + "conv1", base + "bn1", True, blk, "mid"))
            convs.append((base + "conv2", base + "bn2", True, blk, "mid"))
            if k == 0:
                convs.append((base + "downsample.0", base + "downsample.1", False, blk, "downsample"))
            convs.append((base + "conv3", base + "bn3", True, blk, "out"))
            blk += 1
    return convs


def resnet_50_kept(compress_rate):
    """[(score file stem, original width, kept width)] for the 53 files, consumer order."""
    overall, mid = resnet_50_widths(compress_rate)
    out = []
    for k, (_, _, _, blk, kind) in enumerate(resnet_50_convs()):
        if kind == "stem":
            ori, cur = RESNET50_STAGE_OUT[0], overall[0]
        elif kind == "mid":
            ori, cur = RESNET50_STAGE_OUT[blk + 1] // 4, mid[blk]
        else:
            ori, cur = RESNET50_STAGE_OUT[blk + 1], overall[blk + 1]
        out.append(("imp_conv%d" % (k + 1), ori, cur))
    return out


def vgg_16_bn_kept(compress_rate):
    """[(score file stem, original width, kept width)] for the 13 convolutions (the 13th has no score
    file and never shrinks)."""
    widths = vgg_16_bn_widths(compress_rate)
    ori = [x for x in VGG_CFG if x != "M"]
    return [("imp_conv%d" % (k + 1), o, w) for k, (o, w) in enumerate(zip(ori, widths))]


def _resnet_cifar_stage_out(num_layers):
    rep = RESNET_CIFAR_REPEAT[num_layers]
    return [16] + [16] * rep[0] + [32] * rep[1] + [64] * rep[2]


def resnet_cifar_widths(compress_rate, num_layers):
    """(overall_channel, mid_channel) of models/cifar10/resnet.py:5-30 for resnet_56 / resnet_110."""
    rep = RESNET_CIFAR_REPEAT[num_layers]
    rates = list(compress_rate)
    stage_oup = [rates[0]]
    for i in range(len(rep) - 1):
        stage_oup += [rates[i + 1]] * rep[i]
    stage_oup += [0.0] * rep[-1]
    mid_rates = rates[len(rep):]
    stage_out = _resnet_cifar_stage_out(num_layers)
    overall = [int(c * (1 - r)) for c, r in zip(stage_out, stage_oup)]
    mid = [int(stage_out[i] * (1 - mid_rates[i - 1])) for i in range(1, len(stage_out))]
    return overall, mid


@functools.lru_cache(None)
def resnet_cifar_convs(num_layers):
    """[(conv name, score file stem, block index, 'mid' | 'out')] in the order load_resnet_model visits
    them (utils/load_models.py:83-94): score file cnt with cnt = 2, 3, ... (imp_conv1 is the stem's)."""
    convs, cnt, blk = [], 1, 0
    for layer, num in enumerate(RESNET_CIFAR_REPEAT[num_layers]):
        for k in range(num):
            for l in range(2):
                cnt += 1
                convs.append(("layer%d.%d.conv%d" % (layer + 1, k, l + 1), "imp_conv%d" % cnt, blk, "mid" if l == 0 else "out"))
            blk += 1
    return convs


def resnet_cifar_kept(compress_rate, num_layers):
    """[(score file stem, original width, kept width)] for the files the consumer reads."""
    overall, mid = resnet_cifar_widths(compress_rate, num_layers)
    stage_out = _resnet_cifar_stage_out(num_layers)
    return [(stem, stage_out[blk + 1], mid[blk] if kind == "mid" else overall[blk + 1])
            for _, stem, blk, kind in resnet_cifar_convs(num_layers)]


def densenet_40_conv_names():
    """The 39 convolutions in named_modules() order (models/cifar10/densenet.py:68-75)."""
    names = ["conv1"]
    for b in (1, 2, 3):
        names += ["dense%d.%d.conv1" % (b, i) for i in range(DENSENET40_BLOCK)]
        if b < 3:
            names.append("trans%d.conv1" % b)
    return names


def densenet_40_widths(compress_rate):
    """Output channels of the 39 convolutions (models/cifar10/densenet.py:67-75, :91-104): conv1 is never
    pruned (compress_rate[0] is not read), a dense layer keeps int(12*(1-r)) filters, a transition
    int(floor(inplanes*(1-r)))."""
    n, rates = DENSENET40_BLOCK, list(compress_rate)
    inplanes = 2 * DENSENET40_GROWTH
    widths = [inplanes]
    for b in range(3):
        for r in rates[b * (n + 1) + 1:b * (n + 1) + 1 + n]:
            w = int(DENSENET40_GROWTH * (1 - r))
            widths.append(w)
            inplanes += w
        if b < 2:
            inplanes = int(math.floor(inplanes * (1 - rates[(b + 1) * (n + 1)]) // 1))
            widths.append(inplanes)
    return widths


def densenet_40_kept(compress_rate):
    """[(score file stem, original width, kept width)], consumer order (cov_id = 1 ... 39)."""
    ori = densenet_40_widths([0.0] * 39)
    return [("imp_conv%d" % (k + 1), o, w) for k, (o, w) in enumerate(zip(ori, densenet_40_widths(compress_rate)))]


def googlenet_widths(compress_rate, filters=None):
    """Per Inception block (n1x1, 3x3 conv out, 5x5-branch middle conv out, 5x5-branch last conv out,
    pool_planes) of the pruned net (models/cifar10/googlenet.py:28-66: int(n*(1-rate)), the last block
    keeps the full width on its two branch outputs but not on the middle 5x5-branch conv)."""
    filters = filters or GOOGLENET_FILTERS
    out = []
    for i, (n1, n3, n5, pool) in enumerate(filters):
        keep = 1 - compress_rate[i + 1]
        last = i == len(filters) - 1
        out.append((n1, n3 if last else int(n3 * keep), int(n5 * keep), n5 if last else int(n5 * keep), pool))
    return out


def googlenet_kept(compress_rate, filters=None):
    """[(score file stem, original width, kept width)] for the files the consumer reads (the _n5x5 file
    of a block serves both 5x5-branch convs; listed once, with the middle conv's width)."""
    filters = filters or GOOGLENET_FILTERS
    out = []
    for i, (w, f) in enumerate(zip(googlenet_widths(compress_rate, filters), filters)):
        out.append(("imp_conv%d_n3x3" % (i + 2), f[1], w[1]))
        out.append(("imp_conv%d_n5x5" % (i + 2), f[2], w[2]))
    return out


def _load_imp(imp_score, stem):
    if isinstance(imp_score, dict):
        return np.asarray(imp_score[stem])
    return np.load(os.path.join(imp_score, stem + ".npy"))


def _kept_rows(imp_score, stem, o, c):
    """select_index on score file `stem`, which must hold one score per filter of its conv: with any other
    length the argsort below would still return c indices, into the wrong filters or past the last one."""
    imp = _load_imp(imp_score, stem)
    if imp.shape != (o,):
        raise ValueError("score file %s holds %s scores, its convolution has %d filters" % (stem, "x".join(map(str, imp.shape)), o))
    return select_index(imp, o, c)


def _rows(t, idx):
    return t.index_select(0, torch.as_tensor(idx, dtype=torch.long, device=t.device))


def _rows_cols(t, rows, cols):
    if rows is not None:
        t = _rows(t, rows)
    if cols is not None:
        t = t.index_select(1, torch.as_tensor(cols, dtype=torch.long, device=t.device))
    return t


def transplant_vgg(state_dict, oristate_dict, imp_score, conv_names=None):
    """utils/load_models.py:17-64. `state_dict`: the pruned model's (updated in place and returned);
    `imp_score`: score directory or {stem: array}; conv_names: the Conv2d modules in named_modules()
    order (default: features.conv<i> of the reference's VGG)."""
    if conv_names is None:
        conv_names = ["features.conv%d" % i for i, x in enumerate(VGG_CFG) if x != "M"]
    last = None
    for cnt, name in enumerate(conv_names, start=1):
        key = name + ".weight"
        ori, cur = oristate_dict[key], state_dict[key]
        o, c = ori.size(0), cur.size(0)
        if o != c:
            sel = _kept_rows(imp_score, "imp_conv%d" % cnt, o, c)
            if last is not None:
                # [index_i][index_j] = ori[i][j] for i in select_index, j in last_select_index (:43-47);
                # input channels beyond len(last) keep what the slim tensor had
                cur[:, :len(last)] = _rows_cols(ori, sel, last).to(cur.dtype)
            else:
                cur.copy_(_rows(ori, sel))
            last = sel
        elif last is not None:
            cur[:, :len(last)] = _rows_cols(ori, None, last).to(cur.dtype)  # :55-59
        else:
            state_dict[key] = ori  # :61 (the reference rebinds the entry to the original tensor)
            last = None
    return state_dict


def transplant_resnet_50(state_dict, oristate_dict, imp_score, downsample_input="conv2"):
    """utils/load_models.py:441-582 for args.net == 'resnet_50'.

    downsample_input: whose kept filters select the INPUT channels of a stage's downsample conv. "conv2", the default, is
    the reference bit for bit: it uses last_select_index as it stands when the loop reaches the downsample conv, which
    holds the kept filters of the block's conv2 (:525-529, :547-551), although that conv reads the block's input.
    "block" uses the index the block was entered with (the kept filters of what feeds the block: the stem or the
    previous stage's last conv3; None, the whole input, where that was not pruned), which is what the pruned module
    computes with; prune.prune_network asks for it. Every other tensor is the same under both."""
    if downsample_input not in ("conv2", "block"):
        raise ValueError("downsample_input is 'conv2' or 'block', not %r" % (downsample_input,))
    honey = set()
    last = block_in = None
    for k, (conv, bn, record_last, _, kind) in enumerate(resnet_50_convs()):
        key = conv + ".weight"
        honey.add(key)
        ori, cur = oristate_dict[key], state_dict[key]
        o, c = ori.size(0), cur.size(0)
        stem = k == 0
        if conv.endswith(".0.conv1"):
            block_in = last  # a stage's first block: what its conv1 and its downsample conv both read
        cols = block_in if kind == "downsample" and downsample_input == "block" else last
        if o != c:
            sel = _kept_rows(imp_score, "imp_conv%d" % (k + 1), o, c)
            if cols is not None and not stem:
                cur[:, :len(cols)] = _rows_cols(ori, sel, cols)
            else:
                cur.copy_(_rows(ori, sel))
            for part in _BN_PARTS:
                state_dict[bn + part].copy_(_rows(oristate_dict[bn + part], sel))
            if record_last or stem:
                last = sel
        elif cols is not None and not stem:
            cur[:, :len(cols)] = _rows_cols(ori, None, cols)
            for part in _BN_PARTS:
                state_dict[bn + part] = oristate_dict[bn + part]
            if record_last:
                last = None
        else:
            state_dict[key] = ori
            for part in _BN_PARTS:
                state_dict[bn + part] = oristate_dict[bn + part]
            if record_last and not stem:
                last = None
        state_dict[bn + ".num_batches_tracked"] = oristate_dict[bn + ".num_batches_tracked"]
    # :570-580: every other conv (none for resnet_50) and the linear layer come over unchanged
    for key in oristate_dict:
        if key.endswith(".weight") and oristate_dict[key].dim() == 4 and key not in honey:
            state_dict[key] = oristate_dict[key]
    for key in ("fc.weight", "fc.bias"):
        if key in oristate_dict:
            state_dict[key] = oristate_dict[key]
    return state_dict


def transplant_resnet_cifar(state_dict, oristate_dict, imp_score, num_layers):
    """utils/load_models.py:67-143 (load_resnet_model, layer = 56 or 110)."""
    visited = set()
    last = None
    for conv, stem, _, _ in resnet_cifar_convs(num_layers):
        key = conv + ".weight"
        visited.add(key)
        ori, cur = oristate_dict[key], state_dict[key]
        o, c = ori.size(0), cur.size(0)
        if o != c:
            sel = _kept_rows(imp_score, stem, o, c)
            if last is not None:
                cur[:, :len(last)] = _rows_cols(ori, sel, last)
            else:
                cur.copy_(_rows(ori, sel))
            last = sel
        elif last is not None:
            cur[:, :len(last)] = _rows_cols(ori, None, last)
            last = None  # :123 (the VGG loader keeps it here)
        else:
            state_dict[key] = ori
            last = None
    # :126-141: every other conv (the stem; shortcuts are parameter-free pads) and the linear layer whole
    for key, t in oristate_dict.items():
        if key.endswith(".weight") and t.dim() == 4 and key not in visited and "shortcut" not in key:
            state_dict[key] = t
        elif key.endswith(".weight") and t.dim() == 2:
            state_dict[key] = t
            state_dict[key[:-len("weight")] + "bias"] = oristate_dict[key[:-len("weight")] + "bias"]
    return state_dict


def transplant_densenet_40(state_dict, oristate_dict, imp_score, conv_names=None):
    """utils/load_models.py:385-438 (load_densenet_model)."""
    last = []  # :388 - a list from the start: the `last_select_index is not None` tests are always true
    for cov_id, name in enumerate(conv_names or densenet_40_conv_names(), start=1):
        key = name + ".weight"
        ori, cur = oristate_dict[key], state_dict[key]
        o, c = ori.size(0), cur.size(0)
        if o != c:
            sel = [int(i) for i in _kept_rows(imp_score, "imp_conv%d" % cov_id, o, c)]
            if last:
                cur[:, :len(last)] = _rows_cols(ori, sel, last)
        else:
            if last:
                cur[:, :len(last)] = _rows_cols(ori, None, last)
            sel = list(range(o))
        if cov_id in (1, 14, 27):  # :432 conv1 and the transitions restart the concatenation
            last = list(sel)
        else:
            shift = cov_id * 12 - (cov_id - 1) // 13 * 12  # :435
            last = last + [x + shift for x in sel]
    return state_dict


def transplant_googlenet(state_dict, oristate_dict, imp_score, filters=None, blocks=None):
    """utils/load_models.py:146-382 (load_google_model with cpr=None, as load_model calls it). `filters`:
    the original filter table the offsets come from (default: the reference's; tests pass a miniature)."""
    filters = filters or GOOGLENET_FILTERS
    blocks = blocks or GOOGLENET_BLOCKS
    sketch_bn = {"pre_layers.1"}
    cur_last = []
    # pre_layers (cov_id 1, :332-358): transplanted only if it lost filters - the constructor never prunes it
    ori, cur = oristate_dict["pre_layers.0.weight"], state_dict["pre_layers.0.weight"]
    if ori.size(0) != cur.size(0):
        sel = _kept_rows(imp_score, "imp_conv1", ori.size(0), cur.size(0))
        cur_last = [int(i) for i in sel]
        cur.copy_(_rows(ori, sel))
    for b, name in enumerate(blocks):
        cov_id, f = b + 2, filters[b]
        sketch_bn |= {name + ".branch3x3.4", name + ".branch5x5.4", name + ".branch5x5.7"}
        last, cur_last = cur_last, []
        pool_part = []
        for entry in (".branch1x1.0", ".branch3x3.0", ".branch5x5.0", ".branch_pool.1"):  # :208-242 input channels only
            key = name + entry + ".weight"
            ori, cur = oristate_dict[key], state_dict[key]
            cols = last if ori.size(1) != cur.size(1) else None
            n = len(cols) if cols is not None else ori.size(1)
            if n:
                cur[:, :n] = _rows_cols(ori[:cur.size(0)], None, cols)
            if entry == ".branch1x1.0":
                cur_last += list(range(cur.size(0)))
            elif entry == ".branch_pool.1":
                pool_part = [x + f[0] + f[1] + f[2] for x in range(cur.size(0))]
        cur_last += pool_part  # appended before the 3x3 / 5x5 parts (:236-242 run before :275, :320)
        sel5 = None
        for entry, stem in ((".branch3x3.3", "_n3x3"), (".branch5x5.3", "_n5x5")):  # :244-279 filters only
            key = name + entry + ".weight"
            ori, cur = oristate_dict[key], state_dict[key]
            o, c = ori.size(0), cur.size(0)
            sel = [int(i) for i in _kept_rows(imp_score, "imp_conv%d%s" % (cov_id, stem), o, c)] if o != c else list(range(o))
            cur[:len(sel)] = _rows(ori, sel)
            if stem == "_n3x3":
                cur_last += [x + f[0] for x in sel]
            else:
                sel5 = sel
        key = name + ".branch5x5.6.weight"  # :281-328 filters and input channels
        ori, cur = oristate_dict[key], state_dict[key]
        cols = sel5 if ori.size(1) != cur.size(1) else list(range(ori.size(1)))
        o, c = ori.size(0), cur.size(0)
        sel = [int(i) for i in _kept_rows(imp_score, "imp_conv%d_n5x5" % cov_id, o, c)] if o != c else list(range(o))
        cur_last += [x + f[0] + f[1] for x in sel]
        cur[:len(sel), :len(cols)] = _rows_cols(ori, sel, cols)
    # :361-380: every conv is on the sketch list (nothing to copy, biases included); batch-norms off the
    # list and the linear layer come over whole
    for key in oristate_dict:
        if key.endswith(".running_mean") and key[:-len(".running_mean")] not in sketch_bn:
            for part in _BN_PARTS:
                state_dict[key[:-len(".running_mean")] + part] = oristate_dict[key[:-len(".running_mean")] + part]
        elif key.endswith(".weight") and oristate_dict[key].dim() == 2:
            state_dict[key] = oristate_dict[key]
            state_dict[key[:-len("weight")] + "bias"] = oristate_dict[key[:-len("weight")] + "bias"]
    return state_dict


# ---------------------------------------------------------------------------------------------
# U^2-Net-p (models/DUTS/u2net.py, utils/load_models.py:585-769)
# ---------------------------------------------------------------------------------------------
U2NETP_DEPTH = {1: 7, 2: 6, 3: 5, 4: 4, 5: 4, 6: 4}   # RSU7, RSU6, RSU5, RSU4, RSU4F, RSU4F (models/DUTS/u2net.py:455-477)


def u2netp_conv_shapes(compress_rate, in_ch=3, out_ch=1, inner=16, outer=64):
    """[(conv module name, out channels, in channels)] of U2NETP(compress_rate) in named_modules() order,
    'outconv' excluded (models/DUTS/u2net.py:34-79, :137-175, :219-251, :288-313, :344-365, :386-486).
    Inside an RSU of depth D the first D-2 inner widths follow the rates (at least 1 channel), the two
    deepest convs keep `inner`; the five outer widths follow compress_rate[34:39]. `inner` / `outer`
    are 16 / 64 in the reference (smaller values give the tests a cheap network of the same shape)."""
    r = list(compress_rate)
    spans = {(1, False): (0, 5), (2, False): (5, 9), (3, False): (9, 12), (4, False): (12, 14), (5, False): (14, 16),
             (6, False): (16, 18), (1, True): (18, 23), (2, True): (23, 27), (3, True): (27, 30), (4, True): (30, 32),
             (5, True): (32, 34)}                                                     # adapt_channel, :386-401
    ext = [max(1, int((1 - x) * outer)) for x in r[34:39]]                           # :438-452
    m1, m2, m3, m4, m5 = ext

    def rsu(prefix, stage, rates, cin, cout):
        depth = U2NETP_DEPTH[stage]
        mid = [max(1, int((1 - rates[k]) * inner)) for k in range(depth - 2)] + [inner]  # mid_ch1 .. mid_ch{D-1}
        convs = [(prefix + ".rebnconvin.conv_s1", cout, cin), (prefix + ".rebnconv1.conv_s1", mid[0], cout)]
        for k in range(2, depth):
            convs.append((prefix + ".rebnconv%d.conv_s1" % k, mid[k - 1], mid[k - 2]))
        convs.append((prefix + ".rebnconv%d.conv_s1" % depth, mid[depth - 2], mid[depth - 2]))
        for k in range(depth - 1, 1, -1):
            convs.append((prefix + ".rebnconv%dd.conv_s1" % k, mid[k - 2], 2 * mid[k - 1]))
        convs.append((prefix + ".rebnconv1d.conv_s1", cout, 2 * mid[0]))
        return convs

    enc = [(1, in_ch, m1), (2, m1, m2), (3, m2, m3), (4, m3, m4), (5, m4, m5), (6, m5, m5)]
    dec = [(5, 2 * m5, m4), (4, 2 * m4, m3), (3, 2 * m3, m2), (2, 2 * m2, m1), (1, 2 * m1, m1)]
    out = []
    for stage, cin, cout in enc:
        lo, hi = spans[(stage, False)]
        out += rsu("stage%d" % stage, stage, r[lo:hi], cin, cout)
    for stage, cin, cout in dec:
        lo, hi = spans[(stage, True)]
        out += rsu("stage%dd" % stage, stage, r[lo:hi], cin, cout)
    for k, c in zip(range(1, 7), (m1, m1, m2, m3, m4, m5)):                          # :479-484
        out.append(("side%d" % k, out_ch, c))
    return out


def transplant_u2netp(state_dict, oristate_dict, imp_score, conv_names=None):
    """utils/load_models.py:585-769 (load_u2netp_model), the copy loops as index_select. Only conv
    `.weight` tensors are written (no conv bias, no batch-norm tensor, :609-610); the control flow -
    stage counter, the three lists of remembered indices, which branches read a score file - is the
    reference's, including where it raises (an un-pruned decoder `rebnconvin` behind a pruned layer
    evaluates int('i'), :658; a stage that starts with no live index evaluates list(None), :617/:621)."""
    if conv_names is None:
        conv_names = [n for n, _, _ in u2netp_conv_shapes([0.0] * 39)]
    last = None
    cnt, stage_id = 0, 1
    saved, saved_stage, saved_side = [], [], []

    def cols(dst, src_rows, col_idx, col_base, dst0):
        """dst[:, dst0 + k] = src_rows[:, col_idx[k] + col_base]"""
        idx = torch.as_tensor(np.asarray(col_idx, dtype=np.int64) + col_base, dtype=torch.long, device=src_rows.device)
        dst[:, dst0:dst0 + len(col_idx)] = src_rows.index_select(1, idx).to(dst.dtype)

    for name in conv_names:
        if name == "outconv":
            break
        side_name = name.split(".")[0]
        is_side = side_name[:4] == "side"
        decode = side_name[-1] == "d"
        flag = "d." if decode else "."
        midfix = None if is_side else name.split(".")[1]
        key = name + ".weight"
        ori, cur = oristate_dict[key], state_dict[key]
        o, c, oin = ori.size(0), cur.size(0), ori.size(1)
        cov_id = None if is_side else midfix[-2:]
        if decode and side_name[-2] != str(stage_id):                                   # :616-619
            stage_id -= 1
            saved_side.append(list(last))
            saved = []
        elif (not decode) and side_name[-1] != str(stage_id):                           # :620-623
            stage_id += 1
            saved_stage.append(list(last))
            saved = []

        def kept():
            return _kept_rows(imp_score, "net.stage%d%s%s.relu_s1" % (stage_id, flag, midfix), o, c)

        if not is_side:
            if decode and cov_id == "in":
                second = "stage"          # second half of the input: the encoder stage's output (:638)
            elif cov_id[1] != "d":
                second = None
            else:
                second = "unit"           # the RSU's own rebnconv<k> (:717)
            if o != c:
                sel = kept()
                rows = _rows(ori, sel)
                if second is None:
                    if last is not None:
                        cols(cur, rows, last, 0, 0)
                    else:
                        cur.copy_(rows)
                else:
                    other = saved_stage[stage_id - 1] if second == "stage" else saved[int(cov_id[0])]
                    cols(cur, rows, last, 0, 0)
                    cols(cur, rows, other, int(oin / 2), len(last))
                last = sel
                if second != "unit":
                    saved.append(list(sel))
            elif last is not None:
                sel = kept()
                if second is not None:
                    other = saved[int(cov_id[0])]  # :658 reads cov_id[0] for 'in' too (ValueError there)
                cols(cur, ori, last, 0, 0)
                if second is not None:
                    cols(cur, ori, other, int(oin / 2), len(last))
                last = sel
                if second != "unit":
                    saved.append(list(sel))
            else:
                state_dict[key] = ori
                last = None
                if second != "unit":
                    saved.append(None)
        else:
            cnt += 1
            if o != c:
                sel = _kept_rows(imp_score, "net.side%d" % cnt, o, c)
                rows = _rows(ori, sel)
                if last is not None:
                    cols(cur, rows, last, 0, 0)
                else:
                    cur.copy_(rows)
            elif last is not None:
                cols(cur, ori, last, 0, 0)
            else:
                state_dict[key] = ori
            last = saved_side[5 - cnt]                                                   # :767
    return state_dict


# ---------------------------------------------------------------------------------------------
# The carry mode: rows by the score files, columns by data flow, per-channel tensors with their channels
# ---------------------------------------------------------------------------------------------
GOOGLENET_REDUCE = [[96, 16], [128, 32], [96, 16], [112, 24], [128, 24], [144, 32], [160, 32], [160, 32], [192, 48]]  # models/cifar10/googlenet.py:171-184

Flow = namedtuple("Flow", "module kind stem width sources")
Flow.__doc__ = """One parameterised module of a net's data flow (DESIGN.md §7m).

module   the module's name below the net: its tensors are module + ".weight" and so on
kind     "conv" (Conv2d), "bn" (BatchNorm1d / 2d) or "linear" (Linear)
stem     conv: the score file that selects its ROWS once its width shrank (the file the reference's loader reads for
         that conv); None for a conv no constructor shrinks, for batch-norms and for linear layers
width    output channels of the module in the full-width net (bn: its channels)
sources  whose kept filters make up the module's INPUT channels (bn: its channels), as ((producer conv, offset), ...)
         in channel order: the producer's kept list shifted by its offset in the ORIGINAL tensor. () is an input that
         never shrinks and comes whole: the net's own, or VGG's classifier behind its first Linear. A linear layer's columns are its sources' channels (every net pools to 1 x 1 first)."""


def _conv_bn(out, conv, bn, stem, width, sources):
    out.append(Flow(conv, "conv", stem, width, tuple(sources)))
    out.append(Flow(bn, "bn", None, width, ((conv, 0),)))


def _flow_vgg_16_bn():
    out, prev = [], ()
    idx = [i for i, x in enumerate(VGG_CFG) if x != "M"]
    for k, i in enumerate(idx):
        # the 13th conv has no rate of its own (vgg_16_bn_widths): no file
        _conv_bn(out, "features.conv%d" % i, "features.norm%d" % i, "imp_conv%d" % (k + 1) if k < len(idx) - 1 else None,
                 VGG_CFG[i], prev)
        prev = (("features.conv%d" % i, 0),)
    out.append(Flow("classifier.linear1", "linear", None, 512, prev))
    out.append(Flow("classifier.norm1", "bn", None, 512, ()))
    out.append(Flow("classifier.linear2", "linear", None, 10, ()))
    return out


def _flow_resnet_cifar(num_layers):
    stage_out = _resnet_cifar_stage_out(num_layers)
    out = []
    _conv_bn(out, "conv1", "bn1", "imp_conv1", stage_out[0], ())
    stream = (("conv1", 0),)  # the residual stream: written last by the stem, then by each block's conv2
    for conv, stem, blk, kind in resnet_cifar_convs(num_layers):
        _conv_bn(out, conv, conv.replace(".conv", ".bn"), stem, stage_out[blk + 1], stream)
        stream = ((conv, 0),)  # conv2 reads conv1; the next block reads this block's conv2
    out.append(Flow("fc" if num_layers == 56 else "linear", "linear", None, 10, stream))
    return out


def _flow_resnet_50():
    out, stream, block_in, held = [], (), (), []
    for k, (conv, bn, _, blk, kind) in enumerate(resnet_50_convs()):
        width = RESNET50_STAGE_OUT[0] if kind == "stem" else RESNET50_STAGE_OUT[blk + 1] // (4 if kind == "mid" else 1)
        if conv.endswith(".0.conv1"):
            block_in = stream  # what a stage's first block is entered with: its conv1 and its downsample conv read it
        if kind == "downsample":  # the loader's file order has it before conv3, the module order behind it
            _conv_bn(held, conv, bn, "imp_conv%d" % (k + 1), width, block_in)
            continue
        _conv_bn(out, conv, bn, "imp_conv%d" % (k + 1), width, stream)
        stream = ((conv, 0),)
        out += held
        del held[:]
    out.append(Flow("fc", "linear", None, 1000, stream))
    return out


def _flow_densenet_40():
    names = densenet_40_conv_names()
    widths = densenet_40_widths([0.0] * 39)
    out = [Flow("conv1", "conv", "imp_conv1", widths[0], ())]
    cat, off = [("conv1", 0)], widths[0]  # the growing concatenation, restarted at conv1 and after each transition
    for cov_id, (name, w) in enumerate(zip(names[1:], widths[1:]), start=2):
        base = name[:-len("conv1")]
        out.append(Flow(base + "bn1", "bn", None, off, tuple(cat)))
        out.append(Flow(name, "conv", "imp_conv%d" % cov_id, w, tuple(cat)))
        if name.startswith("trans"):
            cat, off = [(name, 0)], w
        else:
            cat.append((name, off))
            off += w
    out.append(Flow("bn", "bn", None, off, tuple(cat)))
    out.append(Flow("fc", "linear", None, 10, tuple(cat)))
    return out


def _flow_googlenet():
    out = []
    _conv_bn(out, "pre_layers.0", "pre_layers.1", None, 192, ())
    prev = (("pre_layers.0", 0),)
    for b, (name, f, r) in enumerate(zip(GOOGLENET_BLOCKS, GOOGLENET_FILTERS, GOOGLENET_REDUCE)):
        n3, n5 = "imp_conv%d_n3x3" % (b + 2), "imp_conv%d_n5x5" % (b + 2)
        p = name + "."
        _conv_bn(out, p + "branch1x1.0", p + "branch1x1.1", None, f[0], prev)
        _conv_bn(out, p + "branch3x3.0", p + "branch3x3.1", None, r[0], prev)
        _conv_bn(out, p + "branch3x3.3", p + "branch3x3.4", n3, f[1], ((p + "branch3x3.0", 0),))
        _conv_bn(out, p + "branch5x5.0", p + "branch5x5.1", None, r[1], prev)
        _conv_bn(out, p + "branch5x5.3", p + "branch5x5.4", n5, f[2], ((p + "branch5x5.0", 0),))
        _conv_bn(out, p + "branch5x5.6", p + "branch5x5.7", n5, f[2], ((p + "branch5x5.3", 0),))  # one file, both convs
        _conv_bn(out, p + "branch_pool.1", p + "branch_pool.2", None, f[3], prev)
        # torch.cat order: 1x1, 3x3, 5x5, pool
        prev = ((p + "branch1x1.0", 0), (p + "branch3x3.3", f[0]), (p + "branch5x5.6", f[0] + f[1]),
                (p + "branch_pool.1", f[0] + f[1] + f[2]))
    out.append(Flow("linear", "linear", None, 10, prev))
    return out


def _flow_u2netp():
    width = {n: o for n, o, _ in u2netp_conv_shapes([0.0] * 39)}
    out = []

    def unit(prefix, name, sources):
        conv = "%s.%s.conv_s1" % (prefix, name)
        _conv_bn(out, conv, "%s.%s.bn_s1" % (prefix, name), "net.%s.%s.relu_s1" % (prefix, name), width[conv], sources)
        return conv

    def rsu(prefix, depth, sources):
        """The units in module order; returns the conv that writes the stage's output last (d + xin: rebnconv1d)."""
        enc = [unit(prefix, "rebnconvin", sources)]
        for k in range(1, depth + 1):
            enc.append(unit(prefix, "rebnconv%d" % k, ((enc[-1], 0),)))
        d = enc[-1]
        for k in range(depth - 1, 0, -1):
            d = unit(prefix, "rebnconv%dd" % k, ((d, 0), (enc[k], width[d])))  # torch.cat((d, enc[k - 1])), enc[0] is xin here
        return d

    h, prev = {}, ()
    for s in range(1, 7):
        h[s] = rsu("stage%d" % s, U2NETP_DEPTH[s], prev)
        prev = ((h[s], 0),)
    d, deeper = {}, h[6]
    for s in range(5, 0, -1):
        d[s] = rsu("stage%dd" % s, U2NETP_DEPTH[s], ((deeper, 0), (h[s], width[deeper])))  # torch.cat((up(deeper), h_s))
        deeper = d[s]
    for k, src in zip(range(1, 7), (d[1], d[2], d[3], d[4], d[5], h[6])):
        out.append(Flow("side%d" % k, "conv", None, 1, ((src, 0),)))
    out.append(Flow("outconv", "conv", None, 1, tuple(("side%d" % k, k - 1) for k in range(1, 7))))
    return out


_DATAFLOW = {"vgg_16_bn": _flow_vgg_16_bn, "resnet_56": lambda: _flow_resnet_cifar(56), "resnet_110": lambda: _flow_resnet_cifar(110),
             "densenet_40": _flow_densenet_40, "googlenet": _flow_googlenet, "resnet_50": _flow_resnet_50, "u2netp": _flow_u2netp}


def dataflow(name):
    """[Flow] for every parameterised module of `name`, in state-dict order: which score file selects a conv's rows,
    and from which producers, at which offsets of the original tensor, a module's input channels come. The table does
    not depend on the rates: it is derived from the constants the width functions use (VGG_CFG, RESNET_CIFAR_REPEAT,
    RESNET50_STAGE_OUT, DENSENET40_GROWTH, GOOGLENET_FILTERS, U2NETP_DEPTH) and from the forward passes of nets.py.

    Pooling, up-sampling and activations are transparent; a concatenation lists its parts in torch.cat order; after a
    residual sum the stream carries the kept list of the main-path conv that wrote it last (the block's last conv, an
    RSU's rebnconv1d), the stem's for the first block; ResNet-50's downsample convs read the block's input."""
    if name not in _DATAFLOW:
        raise ValueError("the network name you have entered is not supported yet: %r" % (name,))
    return _DATAFLOW[name]()


def _channels(sources, kept):
    """The original channel indices a module with these sources still reads (None: the net's input, whole)."""
    if not sources:
        return None
    return np.concatenate([np.asarray(kept[p], dtype=np.int64) + off for p, off in sources])


def kept_filters(name, state_dict, oristate_dict, imp_score):
    """{conv module: the rows of the full conv that the slim one keeps (ascending int64 indices)} for every conv of
    dataflow(name): rule 1 of transplant_carry, which compensate.compensate reads too. `state_dict` is read for its
    shapes only."""
    kept = {}
    for f in dataflow(name):
        if f.kind != "conv":
            continue
        ori, cur = oristate_dict[f.module + ".weight"], state_dict[f.module + ".weight"]
        o, c = ori.size(0), cur.size(0)
        if o != f.width:
            raise ValueError("%s has %d filters in the full net, the %s table says %d" % (f.module, o, name, f.width))
        if c == o:
            kept[f.module] = np.arange(o)
        elif f.stem is None:
            raise ValueError("%s lost filters (%d of %d left) and has no score file" % (f.module, c, o))
        else:
            kept[f.module] = _kept_rows(imp_score, f.stem, o, c)
    return kept


def transplant_carry(name, state_dict, oristate_dict, imp_score):
    """The carry mode: a new state dict with the keys, order and shapes of `state_dict` (the slim
    net's, read for its shapes only: none of its values survives) and the values of `oristate_dict`, copied by
    dataflow(name):

      1. a conv whose width shrank keeps select_index(scores of its file, original width, slim width) rows, a conv
         that kept its width keeps every row and its file is not read;
      2. input channels are the kept filters of the module's sources, each shifted by its offset in the original tensor;
      3. conv biases and the batch-norm tensors behind a conv take the conv's rows, a batch-norm in front of a conv
         the kept channels of its input; every num_batches_tracked is copied;
      4. everything else - stems, classifiers, side convs - comes over, a Linear behind pruned features with their
         kept list as its columns.

    Where a width ends in a residual sum (the CIFAR stems and stage outputs, ResNet-50's stage outputs, U2-Net-p's
    five outer widths) every writer of the stream has a kept list from a score file of its own and rule 2 follows the
    last main-path writer: there the pruned net is not the full net with dead filters removed, whatever the scores.
    A shape that the table cannot produce (a conv without a score file that lost filters, a Linear whose columns
    are not one per channel) raises ValueError."""
    table = dataflow(name)
    kept = kept_filters(name, state_dict, oristate_dict, imp_score)
    out = {}

    def take(key, rows, cols=None):
        t = oristate_dict[key]
        if rows is not None and len(rows) == t.size(0):
            rows = None  # nothing removed on this axis: the tensor itself
        if cols is not None and len(cols) == t.size(1):
            cols = None
        out[key] = _rows_cols(t, rows, cols).clone() if (rows is not None or cols is not None) else t.clone()

    for f in table:
        chan = _channels(f.sources, kept)
        if f.kind == "conv":
            take(f.module + ".weight", kept[f.module], chan)
            if f.module + ".bias" in oristate_dict:
                take(f.module + ".bias", kept[f.module])
        elif f.kind == "bn":
            for part in _BN_PARTS:
                take(f.module + part, chan)
            out[f.module + ".num_batches_tracked"] = oristate_dict[f.module + ".num_batches_tracked"].clone()
        else:
            w = oristate_dict[f.module + ".weight"]
            if chan is not None and w.size(1) != sum(next(g.width for g in table if g.module == p) for p, _ in f.sources):
                raise ValueError("%s reads %d columns, not one per channel of its input" % (f.module, w.size(1)))
            take(f.module + ".weight", None, chan)
            take(f.module + ".bias", None)
    missing = [k for k in state_dict if k not in out]
    if missing:
        raise ValueError("the %s table does not cover %s" % (name, ", ".join(missing[:4])))
    for k, t in state_dict.items():
        if out[k].shape != t.shape:
            raise ValueError("%s: the table gives %s, the pruned net holds %s" % (k, list(out[k].shape), list(t.shape)))
    return type(state_dict)((k, out[k]) for k in state_dict)
