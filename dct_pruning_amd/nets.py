"""The seven architectures imp_score knows, at full width (compress_rate = 0, what the score path
hooks) and at the pruned widths of the reference's constructors (what the transplanted weights load into).

They keep the reference's public surface for this path:
  * the attribute paths imp_score hooks (utils/common.py:384-977), e.g. net.features[idx],
    net.layer1[j].relu1, net.dense1[j].relu, net.inception_a3, net.stage1.rebnconvin.relu_s1;
  * the helper attributes it reads: net.relucfg (vgg), net.num_blocks (resnet_50),
    net.filters_p (googlenet);
  * state_dict keys and shapes of the reference's models/ (models/cifar10/vgg.py:27-46,
    resnet.py:52-139, densenet.py:12-101, googlenet.py:8-183, models/imagenet/resnet.py:40-130,
    models/DUTS/u2net.py:6-486) so the checkpoints importance_generation.py loads
    (importance_generation.py:25-53) fit these modules too.
Every class takes the reference's rate list (`compress_rate`, None = all zeros) and derives its widths
from the tables of transplant.py (vgg_16_bn_widths, resnet_cifar_widths, resnet_50_widths,
densenet_40_widths, googlenet_widths, u2netp_conv_shapes), which restate the reference's adapt_channel /
constructor arithmetic once; at the reference's rates the state-dict keys, order and shapes are the
reference's pruned model's, and the forward passes are its forward passes (option-A shortcut crop / pad,
per-branch Inception widths and concatenation order, pruned dense growth, RSU widths): DESIGN.md §7l.
imp_score itself is model-agnostic and accepts the reference's own model objects as well.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import transplant as _tp

# shortest rate list each constructor reads to its end (the reference indexes past a shorter one)
RATE_LEN = {"vgg_16_bn": 12, "resnet_56": 30, "resnet_110": 57, "densenet_40": 39, "googlenet": 10, "resnet_50": 20,
            "u2netp": 39}


def _rates(name, compress_rate):
    if compress_rate is None:
        return [0.0] * RATE_LEN[name]
    rates = [float(r) for r in compress_rate]
    if len(rates) < RATE_LEN[name]:
        raise ValueError("%s reads %d rates, compress_rate has %d" % (name, RATE_LEN[name], len(rates)))
    return rates


def _relu():
    return nn.ReLU(inplace=True)


# ----------------------------------------------------------------------------------------
# VGG-16-bn (CIFAR)
# ----------------------------------------------------------------------------------------
class VGG16BN(nn.Module):
    CFG = tuple(_tp.VGG_CFG)

    def __init__(self, num_classes=10, compress_rate=None):
        super().__init__()
        self.relucfg = [2, 6, 9, 13, 16, 19, 23, 26, 29, 33, 36, 39]
        widths = iter(_tp.vgg_16_bn_widths(_rates("vgg_16_bn", compress_rate)))
        mods, c_in = OrderedDict(), 3
        for i, v in enumerate(self.CFG):
            if v == "M":
                mods["pool%d" % i] = nn.MaxPool2d(2, 2)
                continue
            v = next(widths)
            mods["conv%d" % i] = nn.Conv2d(c_in, v, 3, padding=1)
            mods["norm%d" % i] = nn.BatchNorm2d(v)
            mods["relu%d" % i] = _relu()
            c_in = v
        self.features = nn.Sequential(mods)
        self.classifier = nn.Sequential(OrderedDict(
            linear1=nn.Linear(512, 512), norm1=nn.BatchNorm1d(512), relu1=_relu(), linear2=nn.Linear(512, num_classes)))

    def forward(self, x):
        x = F.avg_pool2d(self.features(x), 2)
        return self.classifier(x.flatten(1))


# ----------------------------------------------------------------------------------------
# ResNet-56 / -110 (CIFAR): option-A shortcuts (strided slice + zero channel pad)
# ----------------------------------------------------------------------------------------
class _PadShortcut(nn.Module):
    """`extra` = planes - inplanes channels of zeros, extra // 2 in front and the rest behind. In a pruned net
    `extra` can be negative; the floor division then rounds away from zero (-3 // 2 = -2) and F.pad crops:
    2 channels in front and 1 behind for -3, as the reference's lambda does."""

    def __init__(self, extra, stride):
        super().__init__()
        self.lo, self.hi, self.stride = extra // 2, extra - extra // 2, stride

    def forward(self, x):
        if self.stride != 1:
            x = x[:, :, ::self.stride, ::self.stride]
        return F.pad(x, (0, 0, 0, 0, self.lo, self.hi))


class _BasicBlock(nn.Module):
    def __init__(self, c_in, mid, c_out, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, mid, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.relu1 = _relu()
        self.conv2 = nn.Conv2d(mid, c_out, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(c_out)
        self.relu2 = _relu()
        self.shortcut = nn.Sequential() if (stride == 1 and c_in == c_out) else _PadShortcut(c_out - c_in, stride)

    def forward(self, x):
        y = self.bn2(self.conv2(self.relu1(self.bn1(self.conv1(x)))))
        y = y + self.shortcut(x)
        return self.relu2(y)


class ResNetCifar(nn.Module):
    def __init__(self, depth, num_classes=10, compress_rate=None):
        super().__init__()
        n = (depth - 2) // 6
        # overall[0]: the stem; overall[b + 1], mid[b]: block b's output and its first conv's
        overall, mid = _tp.resnet_cifar_widths(_rates("resnet_%d" % depth, compress_rate), depth)
        self.conv1 = nn.Conv2d(3, overall[0], 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(overall[0])
        self.relu = _relu()
        b = 0
        for s, stride in enumerate([1, 2, 2]):
            blocks = []
            for j in range(n):
                blocks.append(_BasicBlock(overall[b], mid[b], overall[b + 1], stride if j == 0 else 1))
                b += 1
            setattr(self, "layer%d" % (s + 1), nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        # the reference names the classifier `fc` for depth 56 and `linear` for 110
        setattr(self, "fc" if depth == 56 else "linear", nn.Linear(64, num_classes))
        self._head = "fc" if depth == 56 else "linear"

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.layer3(self.layer2(self.layer1(x)))
        return getattr(self, self._head)(self.avgpool(x).flatten(1))


# ----------------------------------------------------------------------------------------
# ResNet-50 (ImageNet)
# ----------------------------------------------------------------------------------------
class _Bottleneck(nn.Module):
    def __init__(self, c_in, mid, c_out, stride, project):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.relu1 = _relu()
        self.conv2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.relu2 = _relu()
        self.conv3 = nn.Conv2d(mid, c_out, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(c_out)
        self.relu3 = _relu()
        self.is_downsample = project
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride, bias=False), nn.BatchNorm2d(c_out))

    def forward(self, x):
        y = self.relu1(self.bn1(self.conv1(x)))
        y = self.relu2(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        y = y + (self.downsample(x) if self.is_downsample else x)
        return self.relu3(y)


class ResNet50(nn.Module):
    def __init__(self, num_classes=1000, compress_rate=None):
        super().__init__()
        self.num_blocks = [3, 4, 6, 3]
        # overall[0]: the stem; overall[b + 1], mid[b]: block b's output (one rate per stage, so the identity
        # shortcuts of a stage fit; the last stage keeps 2048) and its two inner convs'
        overall, mid = _tp.resnet_50_widths(_rates("resnet_50", compress_rate))
        self.conv1 = nn.Conv2d(3, overall[0], 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(overall[0])
        self.relu = _relu()
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        b = 0
        for s, n in enumerate(self.num_blocks):
            stage = nn.ModuleList()
            for j in range(n):
                stage.append(_Bottleneck(overall[b], mid[b], overall[b + 1], (1 if s == 0 else 2) if j == 0 else 1, j == 0))
                b += 1
            setattr(self, "layer%d" % (s + 1), stage)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(2048, num_classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in stage:
                x = blk(x)
        return self.fc(self.avgpool(x).flatten(1))


# ----------------------------------------------------------------------------------------
# DenseNet-40 (growth 12, no bottleneck, no compression)
# ----------------------------------------------------------------------------------------
class _DenseLayer(nn.Module):
    def __init__(self, c_in, growth):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(c_in)
        self.relu = _relu()
        self.conv1 = nn.Conv2d(c_in, growth, 3, padding=1, bias=False)

    def forward(self, x):
        return torch.cat((x, self.conv1(self.relu(self.bn1(x)))), 1)


class _Transition(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(c_in)
        self.relu = _relu()
        self.conv1 = nn.Conv2d(c_in, c_out, 1, bias=False)

    def forward(self, x):
        return F.avg_pool2d(self.conv1(self.relu(self.bn1(x))), 2)


class DenseNet40(nn.Module):
    def __init__(self, num_classes=10, compress_rate=None):
        super().__init__()
        # the 39 convs' output widths in module order: conv1, then per block 12 dense layers (each adds its own
        # pruned growth to the concatenation) and, after blocks 1 and 2, a transition to its own width
        widths = iter(_tp.densenet_40_widths(_rates("densenet_40", compress_rate)))
        c = next(widths)
        self.conv1 = nn.Conv2d(3, c, 3, padding=1, bias=False)
        for s in range(3):
            layers = []
            for _ in range(_tp.DENSENET40_BLOCK):
                growth = next(widths)
                layers.append(_DenseLayer(c, growth))
                c += growth
            setattr(self, "dense%d" % (s + 1), nn.Sequential(*layers))
            if s < 2:
                c_in, c = c, next(widths)
                setattr(self, "trans%d" % (s + 1), _Transition(c_in, c))
        self.bn = nn.BatchNorm2d(c)
        self.relu = _relu()
        self.avgpool = nn.AvgPool2d(8)
        self.fc = nn.Linear(c, num_classes)

    def forward(self, x):
        x = self.trans1(self.dense1(self.conv1(x)))
        x = self.trans2(self.dense2(x))
        x = self.relu(self.bn(self.dense3(x)))
        return self.fc(self.avgpool(x).flatten(1))


# ----------------------------------------------------------------------------------------
# GoogLeNet (CIFAR variant: 5x5 branch = two 3x3 convs)
# ----------------------------------------------------------------------------------------
def _cbr(*pairs):
    mods = []
    for c_in, c_out, k in pairs:
        mods += [nn.Conv2d(c_in, c_out, k, padding=k // 2), nn.BatchNorm2d(c_out), nn.ReLU(True)]
    return mods


class _Inception(nn.Module):
    def __init__(self, c_in, n1, r3, n3, r5, n5mid, n5, npool):
        super().__init__()
        self.branch1x1 = nn.Sequential(*_cbr((c_in, n1, 1)))
        self.branch3x3 = nn.Sequential(*_cbr((c_in, r3, 1), (r3, n3, 3)))
        self.branch5x5 = nn.Sequential(*_cbr((c_in, r5, 1), (r5, n5mid, 3), (n5mid, n5, 3)))
        self.branch_pool = nn.Sequential(nn.MaxPool2d(3, 1, 1), *_cbr((c_in, npool, 1)))

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch3x3(x), self.branch5x5(x), self.branch_pool(x)], 1)


class GoogLeNet(nn.Module):
    FILTERS = tuple(_tp.GOOGLENET_FILTERS)
    REDUCE = tuple(_tp.GOOGLENET_REDUCE)
    NAMES = ("a3", "b3", "a4", "b4", "c4", "d4", "e4", "a5", "b5")

    def __init__(self, num_classes=10, compress_rate=None):
        super().__init__()
        rates = _rates("googlenet", compress_rate)
        self.filters = [list(f) for f in self.FILTERS]
        # the table imp_score slices its files by: the reference shrinks the 3x3 and 5x5 entries of all nine rows,
        # the last one included, whose two branch outputs the constructor then leaves at full width
        self.filters_p = [[f[0], int(f[1] * (1 - r)), int(f[2] * (1 - r)), f[3]] for f, r in zip(self.FILTERS, rates[1:])]
        self.pre_layers = nn.Sequential(*_cbr((3, 192, 3)))  # rates[0] is not read: the stem is never pruned
        c_in = 192
        for name, (n1, n3, n5mid, n5, npool), r in zip(self.NAMES, _tp.googlenet_widths(rates, self.filters), self.REDUCE):
            setattr(self, "inception_" + name, _Inception(c_in, n1, r[0], n3, r[1], n5mid, n5, npool))
            c_in = n1 + n3 + n5 + npool  # torch.cat order: 1x1, 3x3, 5x5, pool
        self.maxpool1 = nn.MaxPool2d(3, 2, 1)
        self.maxpool2 = nn.MaxPool2d(3, 2, 1)
        self.avgpool = nn.AvgPool2d(8, 1)
        self.linear = nn.Linear(c_in, num_classes)

    def forward(self, x):
        x = self.inception_b3(self.inception_a3(self.pre_layers(x)))
        x = self.maxpool1(x)
        for n in ("a4", "b4", "c4", "d4", "e4"):
            x = getattr(self, "inception_" + n)(x)
        x = self.maxpool2(x)
        x = self.inception_b5(self.inception_a5(x))
        return self.linear(self.avgpool(x).flatten(1))


# ----------------------------------------------------------------------------------------
# U^2-Net-p (DUTS): residual U-blocks of depth 7/6/5/4 and the dilated 4F variant
# ----------------------------------------------------------------------------------------
class _ReBnConv(nn.Module):
    def __init__(self, c_in, c_out, dirate=1):
        super().__init__()
        self.conv_s1 = nn.Conv2d(c_in, c_out, 3, padding=dirate, dilation=dirate)
        self.bn_s1 = nn.BatchNorm2d(c_out)
        self.relu_s1 = _relu()

    def forward(self, x):
        return self.relu_s1(self.bn_s1(self.conv_s1(x)))


def _up_like(src, ref):
    return F.interpolate(src, size=ref.shape[2:], mode="bilinear", align_corners=False)


class _RSU(nn.Module):
    """Residual U-block with `depth` encoder units. dilated=True is the RSU-4F form: no
    pooling, dilations 1/2/4/8 instead. `shapes`: {conv module name: (out, in)} of the whole net
    (transplant.u2netp_conv_shapes), read under `prefix`: decoder unit k takes unit k+1's output next to
    encoder unit k's, which have the same (pruned) width, so every concatenation is 2 x that width."""

    def __init__(self, prefix, depth, shapes, dilated=False):
        super().__init__()
        self.depth, self.dilated = depth, dilated

        def unit(name, d=1):
            c_out, c_in = shapes["%s.%s.conv_s1" % (prefix, name)]
            setattr(self, name, _ReBnConv(c_in, c_out, d))

        unit("rebnconvin")
        for k in range(1, depth + 1):
            if dilated:
                d = 2 ** (k - 1)
            else:
                d = 2 if k == depth else 1
            unit("rebnconv%d" % k, d)
            if not dilated and k < depth - 1:
                setattr(self, "pool%d" % k, nn.MaxPool2d(2, 2, ceil_mode=True))
        for k in range(depth - 1, 0, -1):
            unit("rebnconv%dd" % k, 2 ** (k - 1) if dilated else 1)

    def forward(self, x):
        xin = self.rebnconvin(x)
        enc, h = [], xin
        for k in range(1, self.depth + 1):
            h = getattr(self, "rebnconv%d" % k)(h)
            enc.append(h)
            if not self.dilated and k < self.depth - 1:
                h = getattr(self, "pool%d" % k)(h)
        d = enc[-1]
        for k in range(self.depth - 1, 0, -1):
            d = getattr(self, "rebnconv%dd" % k)(torch.cat((d, enc[k - 1]), 1))
            if k > 1 and not self.dilated:
                d = _up_like(d, enc[k - 2])
        return d + xin


class U2NETP(nn.Module):
    def __init__(self, in_ch=3, out_ch=1, compress_rate=None):
        super().__init__()
        shapes = {n: (o, i) for n, o, i in _tp.u2netp_conv_shapes(_rates("u2netp", compress_rate), in_ch, out_ch)}
        for s in range(1, 7):
            setattr(self, "stage%d" % s, _RSU("stage%d" % s, _tp.U2NETP_DEPTH[s], shapes, dilated=s >= 5))
            if s < 6:
                setattr(self, "pool%d%d" % (s, s + 1), nn.MaxPool2d(2, 2, ceil_mode=True))
        for s in range(5, 0, -1):
            setattr(self, "stage%dd" % s, _RSU("stage%dd" % s, _tp.U2NETP_DEPTH[s], shapes, dilated=s >= 5))
        for k in range(1, 7):
            setattr(self, "side%d" % k, nn.Conv2d(shapes["side%d" % k][1], out_ch, 3, padding=1))
        self.outconv = nn.Conv2d(6, out_ch, 1)

    def forward(self, x):
        h1 = self.stage1(x)
        h2 = self.stage2(self.pool12(h1))
        h3 = self.stage3(self.pool23(h2))
        h4 = self.stage4(self.pool34(h3))
        h5 = self.stage5(self.pool45(h4))
        h6 = self.stage6(self.pool56(h5))
        d5 = self.stage5d(torch.cat((_up_like(h6, h5), h5), 1))
        d4 = self.stage4d(torch.cat((_up_like(d5, h4), h4), 1))
        d3 = self.stage3d(torch.cat((_up_like(d4, h3), h3), 1))
        d2 = self.stage2d(torch.cat((_up_like(d3, h2), h2), 1))
        d1 = self.stage1d(torch.cat((_up_like(d2, h1), h1), 1))
        s1 = self.side1(d1)
        sides = [s1] + [_up_like(getattr(self, "side%d" % k)(t), s1)
                        for k, t in zip(range(2, 7), (d2, d3, d4, d5, h6))]
        s0 = self.outconv(torch.cat(sides, 1))
        return tuple(torch.sigmoid(t) for t in [s0] + sides)


def get_network(name, compress_rate=None):
    """Counterpart of utils/common.py:31-54 (no .cuda(): the caller places it). compress_rate=None is the
    full-width net; a rate list gives the pruned net of the reference's constructor and must be at least
    RATE_LEN[name] long (ValueError otherwise: the reference would index past its end)."""
    table = {
        "vgg_16_bn": VGG16BN, "resnet_56": lambda **k: ResNetCifar(56, **k), "resnet_110": lambda **k: ResNetCifar(110, **k),
        "densenet_40": DenseNet40, "googlenet": GoogLeNet, "resnet_50": ResNet50, "u2netp": U2NETP,
    }
    if name not in table:
        raise ValueError("the network name you have entered is not supported yet: %r" % (name,))
    return table[name](compress_rate=compress_rate)


def load_checkpoint(net, args):
    """The five state-dict layouts of importance_generation.py:25-53."""
    ckpt = torch.load(args.pretrain_dir, map_location="cpu", weights_only=True)
    if args.net == "u2netp":
        own = net.state_dict()
        own.update({k: v for k, v in ckpt.items() if k in own})
        net.load_state_dict(own)
    elif args.net == "resnet_50":
        net.load_state_dict(ckpt)
    elif args.net in ("densenet_40", "resnet_110"):
        net.load_state_dict(OrderedDict((k.replace("module.", ""), v) for k, v in ckpt["state_dict"].items()))
    else:
        net.load_state_dict(ckpt["state_dict"])
