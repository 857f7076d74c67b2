"""Host-side mirror of the reference's hook / imp_score interface (utils/common.py:258-977).

Same entry points, same argument meaning, same side effects:
  get_feature_hook / get_feature_hook_densenet / get_feature_hook_u2net_input
      forward-hook callables `(module, input, output) -> None` updating the module-level
      accumulator (the reference's globals feature_result / total, utils/common.py:258-259);
  inference / u2netp_inference   (utils/common.py:312-332);
  imp_score(net, args)           (utils/common.py:367-977): creates
      importance_score/<net>_limit<L>/ under the CWD, runs one forward sweep of `limit`
      batches per hook point, np.save()s the (C,) fp32 vectors under the reference's file
      names and prints the reference's progress lines.
What changed underneath: the per-map Python loop over dct_2d + .item() is ONE
dcts_energy_f32 launch per hooked tensor (ops.energy_nc), and the hooked tensor never
leaves the GPU.

Additions (opt-in, results identical on fixed batches):
  single_sweep=True   all hook points registered at once, one sweep instead of 12..118
                      (SURVEY.md §8 f1);
  accumulate="device" running mean kept on the GPU (dcts_running_mean_update_f32);
  deferred=True       single sweep where the hooks only keep references; at the end of each batch
                      all tensors of one tile shape are scored in ONE launch
                      (dcts_energy_multi_f32) and all running means in one more;
  world_size > 1      hook points LPT-sharded over ranks, one all-gather at the end,
                      rank 0 writes the files;
  criterion="rank"    HRank's score instead of the DCT energy: the numerical rank of every map
                      (dcts_rank_f32, ops.rank_nc) through the same hooks, accumulators, schedules and
                      sharding; files go to rank_conv/<net>_limit<L>/rank_*.npy (hooks
                      get_feature_hook_rank / get_feature_hook_densenet_rank);
  criterion="bands"   the DCT energy split into K frequency bands (bands.partition; dcts_band_energy_f32,
                      ops.band_energy_nc: all K bands in one pass over the map): a [C, K] spectrum per hook point in
                      band_score/<net>_limit<L>_<kind><K>/band_*.npy, which bands.collapse turns into imp_*.npy for
                      any band weighting afterwards, on the host (hooks get_feature_hook_bands /
                      get_feature_hook_densenet_bands / get_feature_hook_u2net_input_bands);
  criterion="entropy" the spectral entropy of every map's DCT coefficients (dcts_spectral_entropy_f32,
                      ops.spectral_entropy_nc) over the channels and with the odd pad of the DCT hook of that kind: one
                      number per map, higher = richer, through the same hooks, accumulators, schedules and sharding;
                      files go to entropy_score/<net>_limit<L>/ent_*.npy (hooks get_feature_hook_entropy /
                      get_feature_hook_densenet_entropy / get_feature_hook_u2net_input_entropy);
  criterion="gm"      the geometric-median criterion on feature maps (dcts_gm_distance_f32, ops.gm_distance_nc): the summed
                      distance of every map to the maps of the channels that compete for its mask (every channel for the
                      "full" and "input" hooks, the last 12 for "last12"), high = far from the others = keep; the one
                      criterion that looks at a second channel. No odd pad (it changes no distance). Files go to
                      gm_score/<net>_limit<L>/gm_*.npy (hooks get_feature_hook_gm / get_feature_hook_densenet_gm /
                      get_feature_hook_u2net_input_gm). gm_metric="cosine" | "correlation" compares unit maps instead
                      (x / |x|, or (x - mean) / |x - mean|: ops.gm_distance_nc(metric=...)), so that a channel's gain, which
                      BatchNorm sets per channel, does not count as distance and a scaled copy of a map is a duplicate; flat
                      (dead) maps land at the low end with the duplicates. Those files go to
                      gm_score/<net>_limit<L>_<metric>/gm_*.npy. gm_pairs=True keeps the terms instead of their sum
                      (dcts_gm_pairs_f32, ops.gm_pair_matrix): a [c, c] matrix per file, the mean over the samples of the
                      distance between every two of the channels that compete for that file's mask (all C for "full" and
                      "input", the last 12 for "last12", the block [lo:hi, lo:hi] for a file that is a channel slice of its
                      hook point), in gm_score/<net>_limit<L>[_<metric>]_pairs/gm_*.npy. A row sum cannot tell two
                      duplicates that are far from everything else from two distinct maps; the matrix can, and
                      dct_pruning_amd.pairs turns it into imp_*.npy under a selection rule (row sum, nearest neighbour,
                      farthest point) afterwards, on the host, as bands.collapse does for a spectrum. Its value is the fp32
                      sum of the batch matrices in batch order divided once by the number of samples
                      (accumulate.PairAccumulator), in every schedule and for every world size. gm_lowpass=K > 0 compares the
                      maps' low-pass signatures, their K x K lowest DCT coefficients (dcts_dct2d_lowpass_f32,
                      ops.gm_distance_nc(lowpass=K) / ops.gm_pair_matrix(lowpass=K)), instead of the maps: the one form of
                      the distance that depends on the transform, under which maps that share their coarse structure and
                      differ in texture or noise are close. It combines with gm_metric and gm_pairs and every schedule.
                      Square maps of an edge with a codelet (every hook point of the six classification nets) take one
                      fused pass and the score is several times faster than plain gm; u2netp's hook shapes (72 ... 288)
                      take dct2d's coefficient path and are slower than plain gm;
                      the output dir is gm_score/<net>_limit<L>[_<metric>]_low<K>[_pairs]/;
  autocast="fp16" | "bf16"
                      the forward sweeps run under torch.autocast; the hooks hand the tensors to ops.energy_nc in
                      whatever dtype arrives (float16 / bfloat16 maps are scored natively, dcts_energy_typed; a tensor
                      autocast left in float32 takes the float32 path). Same files; the scores are those of the
                      autocast forward pass. The "dct" criterion only, and not with deferred=True.
  channels_last=True  the net and every input batch are converted to torch.channels_last; the hooks hand on whatever
                      layout arrives and ops.energy_nc reads channels-last tensors where they lie (dcts_energy_nhwc).
                      Same files. Combines with autocast. The "dct" criterion only, not with deferred=True, not u2netp.

A criterion is defined in one place here: its scorer `_score_<name>(x, c_begin, c_count, pad)` (a cross-channel one takes
`ref=(begin, count)`, the hook kind's whole channel set, as well) and its row of the
criterion table below it (output root and file prefix, hook kinds and odd pad, score width, LPT cost, supported modes and
excluded nets). The hooks, _PointHook, imp_score, check_options and importance_generation.py's parser read the row, so
adding a criterion takes an operator in ops.py, a scorer, a row, and tests and docs for it.
"""
import collections
import contextlib
import os

import numpy as np
import torch

from . import bands as _bands
from . import ops, schedules, sharding
from .accumulate import DeviceAccumulator, DeviceBatchAccumulator, HostAccumulator, PairAccumulator

# tests swap these for the oracle to exercise the host logic without a GPU
_energy_nc = ops.energy_nc
_rank_nc = ops.rank_nc
_band_energy_nc = ops.band_energy_nc
_entropy_nc = ops.spectral_entropy_nc
_gm_nc = ops.gm_distance_nc
_gm_pairs_nc = ops.gm_pair_matrix

AUTOCAST = {"fp16": torch.float16, "bf16": torch.bfloat16}

# the band criterion's partition (K, kind): imp_score(criterion="bands", bands=...) sets it for its hooks
_band_cfg = (4, "square")
_band_weight_cache = {}
# the gm criterion's metric: imp_score(criterion="gm", gm_metric=...) sets it for its hooks, on every call
_gm_metric = "l2"
# the gm criterion's low-pass band (0: the maps as they are): imp_score(criterion="gm", gm_lowpass=...) sets it likewise
_gm_lowpass = 0


def _band_weights(H, W, device):
    """The one-hot [K, H, W] partition of the current band configuration on `device` (H, W after the odd pad)."""
    key = (H, W, str(device)) + tuple(_band_cfg)
    w = _band_weight_cache.get(key)
    if w is None:
        w = _band_weight_cache[key] = torch.from_numpy(_bands.partition(H, W, *_band_cfg)).to(device)
    return w


# The scorers: (x, c_begin, c_count, pad) -> [N, c_count] (bands: [N, c_count, K]) of a channel range of x; pad is the
# cv2 path's odd front pad. They read the swap points above when they are called.
def _score_dct(x, c_begin, c_count, pad):
    return _energy_nc(x, c_begin=c_begin, c_count=c_count, pad_front_if_odd=pad)


def _score_rank(x, c_begin, c_count, pad):
    """HRank's per-map matrix_rank (no odd pad: the rank is taken of the map as it is)."""
    return _rank_nc(x, c_begin=c_begin, c_count=c_count)


def _score_bands(x, c_begin, c_count, pad):
    H, W = x.shape[2], x.shape[3]
    p = 1 if (pad and H % 2 == 1) else 0
    return _band_energy_nc(x, _band_weights(H + p, W + p, x.device), c_begin=c_begin, c_count=c_count, pad_front_if_odd=pad)


def _score_entropy(x, c_begin, c_count, pad):
    return _entropy_nc(x, c_begin=c_begin, c_count=c_count, pad_front_if_odd=pad)


def _gm_kwargs():
    """The metric and the low-pass band, each named only where it is not the default's: "l2" on whole maps is the call it
    always was."""
    kw = {} if _gm_metric == "l2" else {"metric": _gm_metric}
    if _gm_lowpass:
        kw["lowpass"] = _gm_lowpass
    return kw


def _score_gm(x, c_begin, c_count, pad, ref):
    """The summed distance to the maps of `ref` = (begin, count), the hook kind's whole channel set, whichever channel range
    of it is scored here (no odd pad: zeros in front of both maps change no distance). The metric and the low-pass band are
    named only where they are not the default's (_gm_kwargs)."""
    kw = _gm_kwargs()
    return _gm_nc(x, c_begin=c_begin, c_count=c_count, ref_begin=ref[0], ref_count=ref[1], **kw)


def _pair_matrix(x, c_begin, c_count, ref):
    """gm's option gm_pairs: the [c_count, ref[1]] distances of a channel range to the maps of `ref`, summed over the samples
    of x. The metric and the low-pass band are named as _score_gm names them."""
    kw = _gm_kwargs()
    return _gm_pairs_nc(x, c_begin=c_begin, c_count=c_count, ref_begin=ref[0], ref_count=ref[1], **kw)


# A criterion is its scorer above and its row here; everything below reads the row.
#   root, prefix  output root under the CWD; the file stem is the schedule's with its leading imp_ replaced by `prefix`
#                 (a stem without imp_, U2-Net-p's net.<module path>, gets it in front); None keeps the stem
#   what          the hooks' docstring: what stands in place of get_feature_hook's DCT energy
#   kinds, pad    the hook kinds it serves, and whether it takes the odd front pad of the "last12" / "input" kinds
#   banded        scores are [N, c, K] for the K of bands=(K, kind): files hold [C, K], the output dir ends in _<kind><K>
#   cost          LPT cost of one channel of an H x W hook point: the bytes the DCT kernels stream, or the kernel's arithmetic
#   deferred, autocast, channels_last   the modes it supports; `excluded`: {net: why it is out of scope}
#   cross         the score of a map depends on other channels: the scorer also takes ref=(begin, count), the channels of the
#                 hook kind (_kind_slice), which stay whole when a hook point is scored in channel ranges
#   metrics       the distances it can be taken under (gm_metric=...), the default first; another than the default adds
#                 _<metric> to the output dir. () for a criterion that has no such choice
Criterion = collections.namedtuple(
    "Criterion", "name root prefix score what kinds pad banded cost deferred autocast channels_last excluded cross metrics",
    defaults=(("full", "last12", "input"), True, False, lambda H, W: H * W, False, False, False, {}, False, ()))
_TABLE = {c.name: c for c in (
    Criterion("dct", "importance_score", None, _score_dct, "the DCT energy of every map",
              deferred=True, autocast=True, channels_last=True),
    Criterion("rank", "rank_conv", "rank_", _score_rank,
              "HRank's score: the numerical rank of every map, c.view(a, -1).float().sum(0), then the running mean of "
              "utils/common.py:271-277. The ranks are exact small integers in fp32, so the batch sum is exact",
              kinds=("full", "last12"), pad=False, cost=lambda H, W: H * W * min(H, W),
              excluded={"u2netp": "supports edges up to 64; u2netp (up to 288) is out of scope"}),
    Criterion("bands", "band_score", "band_", _score_bands,
              "the DCT energy split into K bands: the accumulator's view(a, -1).sum(0) runs over the flat [a, C*K] view, "
              "so feature_result is the [C, K] spectrum in row-major order", banded=True),
    Criterion("entropy", "entropy_score", "ent_", _score_entropy, "the spectral entropy of every map"),
    Criterion("gm", "gm_score", "gm_", _score_gm,
              "the summed distance of every map to the maps of the hook's channels (the geometric-median criterion)",
              pad=False, cross=True, metrics=tuple(ops.GM_METRICS)),
)}
CRITERIA = tuple(_TABLE)

# the reference's module globals (utils/common.py:258-259)
_acc = HostAccumulator()


def _scored_tensor(kind, inputs, output):
    return inputs[0] if kind == "input" else output


def _kind_slice(crit, kind, C):
    """(c_begin, c_count, pad_front_if_odd) of a hook kind on a C-channel tensor, the rule of the reference's three
    hooks: "full" is every channel as it is, "last12" the channels [C-12, C) on the cv2 path (odd front pad), "input"
    every channel on the cv2 path."""
    if kind not in crit.kinds:
        raise ValueError("the %s criterion has no %s hook (U2-Net-p is out of its scope)" % (crit.name, kind))
    if kind == "last12":
        return C - 12, 12, crit.pad
    return 0, C, crit.pad and kind == "input"


def _hook_score(criterion, kind, x):
    """The scores of every map the hook of that kind scores."""
    crit = _TABLE[criterion]
    base, count, pad = _kind_slice(crit, kind, x.shape[1])
    return _score(crit, x, base, count, pad, (base, count))


def _score(crit, x, c_begin, c_count, pad, ref):
    """The criterion's scorer on a channel range; `ref`: the hook kind's whole range, which a cross-channel criterion needs."""
    if crit.cross:
        return crit.score(x, c_begin, c_count, pad, ref=ref)
    return crit.score(x, c_begin, c_count, pad)


def _hook_energy(kind, x):
    return _hook_score("dct", kind, x)


def get_feature_hook(self, input, output):
    """utils/common.py:262-277."""
    _acc.update(_hook_energy("full", output))


def get_feature_hook_densenet(self, input, output):
    """utils/common.py:280-293: channels [b-12, b), cv2 path."""
    _acc.update(_hook_energy("last12", output))


def get_feature_hook_u2net_input(self, input, output):
    """utils/common.py:296-309: scores input[0], cv2 path."""
    _acc.update(_hook_energy("input", input[0]))


def make_weighted_feature_hook(weights_for):
    """Score variant in the coefficient domain (the reference only hints at variants,
    utils/common.py:268-269): a forward hook with get_feature_hook's signature and accumulation that scores
    sum_{u,v} w[u,v] * coeff[u,v]^2 instead of sum coeff^2. `weights_for(H, W)` returns the [H, W] weights
    (any array-like); they are cached per shape on the hooked tensor's device."""
    cache = {}

    def hook(self, input, output):
        key = (output.shape[2], output.shape[3], output.device)
        if key not in cache:
            cache[key] = torch.as_tensor(weights_for(output.shape[2], output.shape[3]), dtype=torch.float32).to(output.device)
        _acc.update(ops.weighted_energy_nc(output, cache[key]))

    return hook


def _make_hook(crit, kind, like):
    """The hook `like` (one of the reference's three above) with another criterion's score: <like's name>_<criterion>."""
    def hook(self, input, output):
        _acc.update(_hook_score(crit.name, kind, _scored_tensor(kind, input, output)))

    hook.__name__ = hook.__qualname__ = "%s_%s" % (like.__name__, crit.name)
    hook.__doc__ = "%s with %s." % (like.__name__, crit.what)
    return hook


# (criterion, kind) -> the module-level hook of the per-hook host mode: get_feature_hook, get_feature_hook_rank,
# get_feature_hook_densenet_bands, get_feature_hook_u2net_input_entropy, ...
_HOOKS = {("dct", "full"): get_feature_hook, ("dct", "last12"): get_feature_hook_densenet,
          ("dct", "input"): get_feature_hook_u2net_input}
for _crit in _TABLE.values():
    for _kind in _crit.kinds:
        if (_crit.name, _kind) not in _HOOKS:
            _hook = _HOOKS[_crit.name, _kind] = _make_hook(_crit, _kind, _HOOKS["dct", _kind])
            globals()[_hook.__name__] = _hook


def _net_device(net):
    for p in net.parameters():
        return p.device
    return torch.device("cpu")


def inference(net, train_loader, limit):
    """utils/common.py:312-320 (data goes to the net's device instead of an unconditional .cuda())."""
    net.eval()
    dev = _net_device(net)
    for batch_idx, (data, _) in enumerate(train_loader):
        if batch_idx >= limit:
            break
        data = data.to(dev)
        with torch.no_grad():
            net(data)


def u2netp_inference(net, train_loader, limit):
    """utils/common.py:323-332: dict batches with key 'image', cast to float."""
    net.eval()
    dev = _net_device(net)
    with torch.no_grad():
        for batch_idx, data in enumerate(train_loader):
            if batch_idx >= limit:
                break
            inputs = data["image"].type(torch.FloatTensor)
            net(inputs.to(dev))


def _resolve(net, path):
    """'features.2' -> net.features[2], 'layer1.0.relu1' -> net.layer1[0].relu1 (what the
    reference's eval('net.' + name) / net.features[idx] expressions reach)."""
    mod = net
    for atom in path.split("."):
        mod = mod[int(atom)] if atom.isdigit() else getattr(mod, atom)
    return mod


def _schedule_for(net, name):
    if name == "googlenet":
        return schedules.googlenet(getattr(net, "filters_p", None))
    if name == "resnet_50":
        return schedules.resnet_50(tuple(getattr(net, "num_blocks", (3, 4, 6, 3))))
    if name not in schedules.SCHEDULES:
        raise ValueError("imp_score: unknown net %r" % (name,))
    return schedules.SCHEDULES[name]()


def _done_line(net_name, idx, stem):
    """The progress line the reference prints after saving (e.g. utils/common.py:395, :510, :515)."""
    if net_name == "u2netp":
        return None
    if net_name == "googlenet":
        if stem.endswith("_"):
            return "/" + stem[:-1] + ":done!"
        head, tp = stem.split("_", 2)[0:2], stem.split("_", 2)[2]
        return "/" + "_".join(head) + tp + ":done!"
    return "/" + stem + ":done!"


def _file_stem(criterion, stem):
    """The schedule's stem under the criterion's prefix: imp_conv3 -> rank_conv3 / band_conv3 / ent_conv3 / gm_conv3, U2-Net-p's
    net.<module path> -> band_net.<module path>; "dct" keeps the stem."""
    prefix = _TABLE[criterion].prefix
    if prefix is None:
        return stem
    return prefix + (stem[len("imp_"):] if stem.startswith("imp_") else stem)


def _save(out_dir, net_name, pt, scores, criterion="dct", pairs=False):
    """pairs: `scores` is the hook point's [C, C] pair matrix and a file that is a channel slice gets its diagonal block."""
    for stem, lo, hi in pt.files:
        arr = scores if lo is None else (scores[lo:hi, lo:hi] if pairs else scores[lo:hi])
        np.save(os.path.join(out_dir, _file_stem(criterion, stem) + ".npy"), arr)
        line = _done_line(net_name, 0, stem)
        if line:
            print(line)


class _PointHook:
    """A hook with its own accumulator (single-sweep / device modes). With `batch` set, the
    device-side update is deferred and fused across hook points (DeviceBatchAccumulator).

    `ranges` (multi-GPU, single-sweep modes): the channel ranges [(key, lo, hi), ...] of this hook point's
    scored channels that THIS rank owns (sharding.make_units cuts wide layers so that eight ranks balance);
    None = the whole hook point under `key`. Per-channel scores do not depend on which call computes them,
    so the pieces concatenate to the unsplit result bit for bit (a cross-channel criterion's pieces are all scored against
    the hook kind's whole channel set).

    `pairs` (the gm criterion's gm_pairs): every piece is a [c, C] pair matrix, rows [lo, hi) against the hook kind's whole
    channel set, in a PairAccumulator of its own (host or device form, by `accumulate`; `batch` is not used)."""

    def __init__(self, kind, accumulate, device, batch=None, key=None, deferred=False, ranges=None, nominal_c=None,
                 criterion="dct", pairs=False):
        self.kind, self.accumulate, self.device, self.acc = kind, accumulate, device, None
        self.crit = _TABLE[criterion]
        self.batch, self.key, self.deferred = batch, key, deferred
        self.ranges, self.nominal_c, self.accs = ranges, nominal_c, {}
        self.width = None  # K of the band criterion: scores come back as [c, K]
        self.pairs = pairs
        if pairs and not self.crit.cross:
            raise ValueError("pair matrices go with a cross-channel criterion, not with %r" % criterion)

    def _pieces(self, x):
        """(key, c_begin, c_count, pad_front_if_odd) of every operator call this hook makes on x."""
        base, count, pad = _kind_slice(self.crit, self.kind, x.shape[1])
        if self.ranges is None:
            return [(self.key, base, count, pad)]
        if count != self.nominal_c:
            raise RuntimeError(
                "channel-range sharding cut this hook point by the schedule's channel count (%d) but the hooked "
                "tensor has %d: run pruned / non-standard nets without --single_sweep under torch.distributed"
                % (self.nominal_c, count))
        return [(k, base + lo, hi - lo, pad) for k, lo, hi in self.ranges]

    def __call__(self, module, inputs, output):
        x = _scored_tensor(self.kind, inputs, output)
        ref = _kind_slice(self.crit, self.kind, x.shape[1])[:2]
        for key, cb, cc, pad in self._pieces(x):
            if self.pairs:
                m = _pair_matrix(x, cb, cc, ref)
                acc = self.accs.get(key)
                if acc is None:
                    acc = self.accs[key] = PairAccumulator(m.device if self.accumulate == "device" else None)
                acc.update(m, x.shape[0])
                continue
            if self.deferred and self.batch is not None:
                self.batch.add_tensor(key, x, cb, cc, pad)
                continue
            e = _score(self.crit, x, cb, cc, pad, ref)
            if e.dim() == 3:  # [N, c, K] band energies: the accumulators see the dense [N, c*K] view
                self.width = e.shape[2]
                e = e.reshape(e.shape[0], -1)
            if self.batch is not None:
                self.batch.add(key, e)
                continue
            acc = self.accs.get(key)
            if acc is None:
                acc = self.accs[key] = (DeviceAccumulator(e.shape[1], e.device) if self.accumulate == "device"
                                        else HostAccumulator())
            acc.update(e)

    def scores(self, key=None):
        key = self.key if key is None else key
        if self.pairs:
            return np.ascontiguousarray(self.accs[key].scores(), dtype=np.float32)
        if self.batch is not None:
            flat = np.ascontiguousarray(self.batch.scores(key), dtype=np.float32)
        else:
            flat = np.ascontiguousarray(self.accs[key].scores(), dtype=np.float32)
        return flat if self.width is None else flat.reshape(-1, self.width)


def _autocast(autocast, dev):
    """The context the forward sweeps run in: torch.autocast on the net's device, or nothing."""
    if autocast is None:
        return contextlib.nullcontext()
    return torch.autocast(dev.type, dtype=AUTOCAST[autocast])


class _ChannelsLastLoader:
    """The (data, target) batches of `loader` with data in torch.channels_last."""

    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        for data, target in self.loader:
            yield data.contiguous(memory_format=torch.channels_last), target


def check_options(criterion, net, deferred=False, autocast=None, channels_last=False, bands=(4, "square"), gm_metric="l2",
                  gm_pairs=False, gm_lowpass=0):
    """Raises the ValueError of the first rule an imp_score call with these options breaks: what the criterion's row
    supports, and the two rules that hold for every criterion (autocast and channels_last have no deferred mode,
    channels_last does not cover u2netp). importance_generation.py's parser rejects its command lines with it."""
    if criterion not in CRITERIA:
        raise ValueError("imp_score: unknown criterion %r (expected one of %s)" % (criterion, ", ".join(CRITERIA)))
    crit = _TABLE[criterion]
    if gm_metric != "l2" and gm_metric not in crit.metrics:
        if crit.metrics:
            raise ValueError("imp_score: gm_metric must be one of %s, got %r" % (", ".join(crit.metrics), gm_metric))
        raise ValueError("imp_score: gm_metric=%r goes with criterion='gm' only (the %s criterion compares no maps)"
                         % (gm_metric, criterion))
    if gm_pairs and not crit.cross:
        raise ValueError("imp_score: gm_pairs goes with criterion='gm' only (the %s criterion compares no maps)" % criterion)
    if isinstance(gm_lowpass, bool) or not isinstance(gm_lowpass, (int, np.integer)) or gm_lowpass < 0:
        raise ValueError("imp_score: gm_lowpass must be an integer >= 0 (0: whole maps), got %r" % (gm_lowpass,))
    if gm_lowpass:
        if not crit.cross:
            raise ValueError("imp_score: gm_lowpass goes with criterion='gm' only (the %s criterion compares no maps)" % criterion)
        if gm_lowpass == 1 and gm_metric == "correlation":
            raise ValueError("imp_score: gm_lowpass=1 keeps the DC coefficient alone, which gm_metric='correlation' removes: "
                             "nothing is left to compare")
    if autocast is not None:
        if autocast not in AUTOCAST:
            raise ValueError("imp_score: autocast must be None, 'fp16' or 'bf16', got %r" % (autocast,))
        if deferred:
            raise ValueError("imp_score: autocast has no deferred mode (no multi-tensor half-precision launch); "
                             "use single_sweep / accumulate instead")
        if not crit.autocast:
            raise ValueError("imp_score: autocast supports criterion='dct' only (the %s kernels take float32)" % criterion)
    if channels_last:
        if deferred:
            raise ValueError("imp_score: channels_last has no deferred mode (the multi-tensor launches take NCHW tensors); "
                             "use single_sweep / accumulate instead")
        if not crit.channels_last:
            raise ValueError("imp_score: channels_last supports criterion='dct' only (the %s kernels take NCHW tensors)"
                             % criterion)
        if net == "u2netp":
            raise ValueError("imp_score: channels_last does not cover u2netp (dict batches, and no channels-last "
                             "kernel for its 288 x 288 maps)")
    if deferred and not crit.deferred:
        raise ValueError("imp_score: criterion=%r has no deferred mode; use single_sweep / accumulate instead" % criterion)
    if net in crit.excluded:
        raise ValueError("imp_score: criterion=%r %s" % (criterion, crit.excluded[net]))
    if crit.banded and (not 1 <= int(bands[0]) <= _bands.BAND_MAX or bands[1] not in _bands.KINDS):
        raise ValueError("imp_score: bands=(K, kind) needs 1 <= K <= %d and kind in %s, got %r"
                         % (_bands.BAND_MAX, _bands.KINDS, (bands,)))


def imp_score(net, args, train_loader=None, single_sweep=False, accumulate="host", group=None, deferred=False,
              criterion="dct", bands=(4, "square"), autocast=None, channels_last=False, gm_metric="l2", gm_pairs=False,
              gm_lowpass=0):
    """Counterpart of utils/common.py:367-977. `args` needs .net, .limit (and whatever
    load_data reads when train_loader is None). criterion="rank" scores HRank's feature-map rank instead of the
    DCT energy and writes rank_conv/<net>_limit<L>/rank_*.npy. criterion="bands" with bands=(K, kind) writes the
    [C, K] band spectrum of every hook point to band_score/<net>_limit<L>_<kind><K>/band_*.npy. criterion="entropy"
    scores the spectral entropy of every map's DCT coefficients and writes entropy_score/<net>_limit<L>/ent_*.npy (all
    seven nets; not with deferred, autocast or channels_last). criterion="gm" scores every map's summed distance to the
    maps of its hook's channels and writes gm_score/<net>_limit<L>/gm_*.npy (all seven nets; same exclusions); with
    gm_metric="cosine" / "correlation" the distance is taken between unit maps and the files go to
    gm_score/<net>_limit<L>_<metric>/ (criterion "gm" only). gm_pairs=True (criterion "gm" only) writes the [c, c] matrix of
    mean pair distances per file instead, to gm_score/<net>_limit<L>[_<metric>]_pairs/, for dct_pruning_amd.pairs to score.
    gm_lowpass=K > 0 (criterion "gm" only; not K = 1 with "correlation") takes every distance between the maps' K x K lowest
    DCT coefficients instead of the maps; those files go to gm_score/<net>_limit<L>[_<metric>]_low<K>[_pairs]/.
    autocast="fp16" / "bf16" runs the forward sweeps under torch.autocast and scores the half-precision tensors the
    hooks then see as they are (criterion "dct" only, not with deferred).
    channels_last=True converts the net (in place) and every input batch to torch.channels_last; the tensors the hooks
    then see are scored in the layout they arrive in (criterion "dct" only, not with deferred, not u2netp)."""
    global _acc, _band_cfg, _gm_metric, _gm_lowpass
    check_options(criterion, args.net, deferred, autocast, channels_last, bands, gm_metric, gm_pairs, gm_lowpass)
    _gm_metric = gm_metric
    _gm_lowpass = int(gm_lowpass)
    crit = _TABLE[criterion]
    if not hasattr(args, "limit"):
        # utils/load_models.py:819 calls imp_score from prune_*.py whose parsers define no --limit
        # (AttributeError in the reference as shipped); fall back to importance_generation.py's default
        args.limit = 5
    root = crit.root
    out_dir = root + "/" + args.net + "_limit" + str(args.limit)
    width = 1  # floats per channel in a score
    if crit.banded:
        _band_cfg = (int(bands[0]), bands[1])
        width = _band_cfg[0]
        out_dir += "_%s%d" % (_band_cfg[1], width)
    if gm_metric != "l2":
        out_dir += "_" + gm_metric
    if gm_lowpass:
        out_dir += "_low%d" % gm_lowpass
    if gm_pairs:
        out_dir += "_pairs"
    world, rank = 1, 0
    if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
        world = torch.distributed.get_world_size(group)
        rank = torch.distributed.get_rank(group)
    if rank == 0:
        if not os.path.isdir(root):
            os.mkdir(root)
        if not os.path.isdir(out_dir):
            os.mkdir(out_dir)

    print("==> Loading data of {}..".format(getattr(args, "dataset", "synthetic")))
    if train_loader is None:
        from .data import load_data
        train_loader, _ = load_data(args)

    if channels_last:
        net.to(memory_format=torch.channels_last)
        train_loader = _ChannelsLastLoader(train_loader)

    print("==> Generating importance score..")
    print("Importance Score is located at ./" + out_dir)
    _acc = HostAccumulator()

    pts = _schedule_for(net, args.net)
    dev = _net_device(net)
    sweep_fn = u2netp_inference if args.net == "u2netp" else inference

    def sweep(net, train_loader, limit):
        with _autocast(autocast, dev):
            sweep_fn(net, train_loader, limit)

    if deferred:
        single_sweep, accumulate = True, "device"

    # Work units and their owners. A unit is a hook point, or - in the single-sweep modes, where every rank
    # runs the one forward sweep anyway and only the scoring is divisible - a channel range of a wide hook
    # point (sharding.make_units): VGG-16-bn has 12 hook points and GoogLeNet 10, fewer than LPT needs to
    # balance eight ranks. In the reference's one-sweep-per-hook-point schedule a hook point stays whole:
    # cutting it would repeat its forward sweep on another rank.
    scored = [schedules.scored_shape(p) for p in pts]
    chans = [sc[1] for sc in scored]
    # LPT cost per channel: the bytes the DCT kernels stream, or the rank kernel's O(H W min(H, W)) arithmetic (the row's)
    cost_pc = [float(crit.cost(p.H, p.W)) for p in pts]
    if world > 1:
        total_cost = sum(c * k for c, k in zip(chans, cost_pc))
        cut = total_cost / (8.0 * world) if single_sweep else None  # G = 8: every net within 6 % of balance
        units = sharding.make_units(chans, cost_pc, max_unit_cost=cut)
        owner, load = sharding.assign(units, world)
        if rank == 0 and max(load) > 0:
            print("==> %d work units over %d ranks, load imbalance %.3f" % (len(units), world, max(load) * world / sum(load)))
    else:
        units = sharding.make_units(chans, cost_pc)
        owner = [0] * len(units)
    per_layer = {}
    for u in units:
        per_layer[u.layer] = per_layer.get(u.layer, 0) + 1
    mine = [k for k in range(len(units)) if owner[k] == rank]
    results = {}  # unit index -> (channels of the unit,) fp32

    if single_sweep:
        hooks, handles = {}, []
        batch = DeviceBatchAccumulator(dev) if (accumulate == "device" and dev.type == "cuda") else None
        by_layer = {}
        for k in mine:
            by_layer.setdefault(units[k].layer, []).append(k)
        for i, ks in by_layer.items():
            whole = per_layer[i] == 1
            hooks[i] = _PointHook(pts[i].kind, accumulate, dev, batch=batch, key=ks[0], deferred=deferred,
                                  ranges=None if whole else [(k, units[k].c_lo, units[k].c_hi) for k in ks],
                                  nominal_c=chans[i], criterion=criterion, pairs=gm_pairs)
            handles.append(_resolve(net, pts[i].module).register_forward_hook(hooks[i]))
        sweep(net, train_loader, args.limit)
        for h in handles:
            h.remove()
        for i, ks in by_layer.items():
            for k in ks:
                results[k] = hooks[i].scores(k)
    else:
        for k in mine:  # one unit per hook point here
            i = units[k].layer
            pt = pts[i]
            if args.net == "u2netp" and world == 1:
                print("current layer:", "net." + pt.module)
            layer = _resolve(net, pt.module)
            if accumulate == "device" or gm_pairs:  # the pair matrices have no module-level hook: _PointHook in both forms
                hook = _PointHook(pt.kind, accumulate, dev, key=k, criterion=criterion, pairs=gm_pairs)
                handler = layer.register_forward_hook(hook)
                sweep(net, train_loader, args.limit)
                handler.remove()
                results[k] = hook.scores()
            else:
                handler = layer.register_forward_hook(_HOOKS[criterion, pt.kind])
                sweep(net, train_loader, args.limit)
                handler.remove()
                results[k] = np.ascontiguousarray(_acc.feature_result.numpy(), dtype=np.float32)
                if crit.banded:
                    results[k] = results[k].reshape(-1, width)
                _acc.reset()
            if world == 1:
                _save(out_dir, args.net, pt, results[k], criterion, gm_pairs)
        if world == 1:
            print("The importance score generation has been completed!")  # utils/common.py:977
            return

    if world > 1:
        # floats per channel of a layer's score: the criterion's width, or the layer's own channel count for a pair matrix
        # (None: as wide as the owners' results say, which also holds for a net pruned below the schedule's widths)
        layer_scores = _gather_results(results, units, len(pts), owner, world, rank, dev, group,
                                       width=[None] * len(pts) if gm_pairs else width)
    else:
        layer_scores = {units[k].layer: results[k] for k in mine}
    if rank == 0:
        for i, pt in enumerate(pts):
            if args.net == "u2netp":
                print("current layer:", "net." + pt.module)
            _save(out_dir, args.net, pt, layer_scores[i], criterion, gm_pairs)
        print("The importance score generation has been completed!")
    if world > 1:
        torch.distributed.barrier(group)


def _gather_results(local, units, n_layers, owner, world, rank, dev, group, width=1):
    """One all-gather of the flat, equally padded score buffer (plus a tiny all-reduce that tells every rank
    the channel counts of the units, which only their owners know for certain: imp_score also runs on
    already-pruned nets whose widths differ from the schedule's). Returns {layer: (C,) scores}.
    width: the floats a channel of a score carries, one number for every layer or one per layer: 1 gives (C,) scores; K > 1
    (the band criterion's K; a pair matrix's row length) means a unit of c channels carries c * K floats and the layer's
    scores come back as (C, K). None for a layer: whatever the owners of its units report (the all-reduce carries the row
    lengths as well), which must agree among them."""
    import torch.distributed as dist
    backend = dist.get_backend(group)
    cdev = dev if backend == "nccl" else torch.device("cpu")
    widths = list(width) if isinstance(width, (list, tuple)) else [width] * n_layers
    counts = torch.zeros(2, len(units), dtype=torch.int64, device=cdev)  # channels; floats per channel
    for k, v in local.items():
        counts[0, k] = v.shape[0]
        counts[1, k] = v.shape[1] if v.ndim == 2 else 1
    dist.all_reduce(counts, group=group)
    counts, rows = counts.cpu().tolist()
    for k, u in enumerate(units):
        if widths[u.layer] is None:
            widths[u.layer] = rows[k]
        if rows[k] != widths[u.layer]:
            raise RuntimeError("unit %d of hook point %d came back with %d floats per channel, expected %d"
                               % (k, u.layer, rows[k], widths[u.layer]))
    # actual units: a whole hook point spans [0, actual C); a channel range keeps its bounds
    per_layer = [0] * n_layers
    for u in units:
        per_layer[u.layer] += 1
    real = []
    for k, u in enumerate(units):
        if per_layer[u.layer] == 1:
            real.append(sharding.Unit(u.layer, 0, counts[k], float(counts[k])))
        else:
            if counts[k] != u.c_hi - u.c_lo:
                raise RuntimeError("unit %d of hook point %d came back with %d channels, expected %d"
                                   % (k, u.layer, counts[k], u.c_hi - u.c_lo))
            real.append(u)
    chans = [0] * n_layers
    for u in real:
        chans[u.layer] = max(chans[u.layer], u.c_hi)
    # in floats: a unit of channels [lo, hi) of a layer of width w is the floats [lo * w, hi * w) of the layer's flat scores
    real = [sharding.Unit(u.layer, u.c_lo * widths[u.layer], u.c_hi * widths[u.layer], u.cost) for u in real]
    chans = [c * w for c, w in zip(chans, widths)]
    off, seg = sharding.layout(real, owner, world)
    flat = torch.zeros(seg, dtype=torch.float32, device=cdev)
    for k, v in local.items():
        flat[off[k]:off[k] + v.size] = torch.from_numpy(v.reshape(-1)).to(cdev)
    gathered = sharding.all_gather_scores(flat, world, group)
    res = sharding.unpack(gathered, real, owner, off, chans)
    # a layer whose width was given as 1 keeps its (C,) shape; one that was given K > 1 or learned its width is (C, K)
    given = list(width) if isinstance(width, (list, tuple)) else [width] * n_layers
    return {i: r.cpu().numpy() if given[i] == 1 else r.cpu().numpy().reshape(-1, widths[i]) for i, r in enumerate(res)}
