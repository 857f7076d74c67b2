"""From a MACs or parameter budget to the compress-rate list - the step between scoring and pruning:

    python importance_generation.py --net vgg_16_bn --pretrain_dir checkpoints/vgg_16_bn.pt --limit 5
    python -m dct_pruning_amd.rates --net vgg_16_bn --imp_score importance_score/vgg_16_bn_limit5 --target_macs 0.5
    python -m dct_pruning_amd.prune --net vgg_16_bn ... --compress_rate "$(python -m dct_pruning_amd.rates ... | head -1)" --carry

The rule is equal loss. A score file holds one non-negative number per filter; removing the filters masks.select_index
drops at a kept width c costs that layer the share lambda = sum(removed scores) / sum(scores) of its score (removed_share).
The allocation at level eps (at_level) gives every movable rate the largest value at which none of the files it governs
loses more than eps; allocate returns the smallest eps whose allocation meets the budget, so no layer gives up a larger
share of its score than any other has to.

Which widths a rate moves is learned from the width tables of transplant.py (widths), never restated: a rate GOVERNS the
rows that move with it and with no later rate; a row that also moves with an earlier rate is that rate's FOLLOWER (a
DenseNet-40 transition keeps floor(inplanes * (1 - r)) of an input the dense rates before it made narrower). Followers
of a moved rate shrink without being asked: their share is reported as "forced" and not held to eps.

Host arithmetic on score files, like masks.py, bands.py and pairs.py: no kernel, no GPU.
"""
import argparse
import json
import math
import sys
from collections import namedtuple

import numpy as np

from . import nets
from . import transplant as _tp
from .masks import parse_compress_rate, select_index

# the rate indices the solver moves by default: widths that neither end in a residual sum nor follow other widths
FREE = {
    "vgg_16_bn": tuple(range(12)),
    "googlenet": tuple(range(1, 10)),                                                  # 0 is pre_layers: never read
    "densenet_40": tuple(range(1, 13)) + tuple(range(14, 26)) + tuple(range(27, 39)),  # 0 is not read; 13, 26: transitions
    "resnet_56": tuple(range(3, 30)),                                                  # 0 .. 2: stem and stage outputs
    "resnet_110": tuple(range(3, 57)),
    "resnet_50": tuple(range(4, 20)),                                                  # 0 .. 3: stem and stage outputs
    "u2netp": tuple(range(34)),                                                        # 34 .. 38: the outer widths (d + xin)
}

Allocation = namedtuple("Allocation", "rates text level macs params full_macs full_params files")
Allocation.__doc__ = """What allocate returns.

rates        the rate list (floats, len(base) of them); text parses back to it where the solver moved a rate
text         the same list in the reference's DSL, run-length grouped: what --compress_rate takes
level        the largest share of its score a governed file may lose (eps)
macs params  prune.cost of nets.get_network(name, rates); full_macs, full_params: of the full-width net
files        [(stem, original, kept, lambda, "free" | "forced" | "fixed")], one per row of widths(name, rates)"""

Step = namedtuple("Step", "rate kept")
Step.__doc__ = """One distinct width tuple on the walk of a rate index: `rate` produces it (the emitted decimal; the
base value for step 0), `kept` is {row of widths(): kept width} over the rows that move with the index."""

_SCALE = 10 ** 6   # rates live on the grid k / 10^6: what six decimal places can say
_PROBE = 0.9       # the rate at which _moves looks which rows an index moves


def _check_len(name, rates):
    if name not in nets.RATE_LEN:
        raise ValueError("the network name you have entered is not supported yet: %r" % (name,))
    rates = [float(r) for r in rates]
    if len(rates) < nets.RATE_LEN[name]:
        raise ValueError("%s reads %d rates, the list has %d" % (name, nets.RATE_LEN[name], len(rates)))
    return rates


_ROWS = {}


def _rows(name):
    """((score file stem, conv module, original width), ...): the convs of dataflow(name) a score file selects rows for."""
    if name not in _ROWS:
        _ROWS[name] = tuple((f.stem, f.module, f.width) for f in _tp.dataflow(name) if f.kind == "conv" and f.stem is not None)
    return _ROWS[name]


_VGG_CONVS = ["features.conv%d" % i for i, x in enumerate(_tp.VGG_CFG) if x != "M"]


def _kept_by_module(name, rates):
    """{conv module: output channels at `rates`} from the width tables the constructors of nets.py read."""
    if name == "vgg_16_bn":
        return dict(zip(_VGG_CONVS, _tp.vgg_16_bn_widths(rates)))
    if name in ("resnet_56", "resnet_110"):
        n = int(name[7:])
        out = {"conv1": _tp.resnet_cifar_widths(rates, n)[0][0]}
        out.update((conv, c) for (conv, _, _, _), (_, _, c) in zip(_tp.resnet_cifar_convs(n), _tp.resnet_cifar_kept(rates, n)))
        return out
    if name == "resnet_50":
        return {conv: c for (conv, _, _, _, _), (_, _, c) in zip(_tp.resnet_50_convs(), _tp.resnet_50_kept(rates))}
    if name == "densenet_40":
        return dict(zip(_tp.densenet_40_conv_names(), _tp.densenet_40_widths(rates)))
    if name == "googlenet":
        out = {}
        for blk, w in zip(_tp.GOOGLENET_BLOCKS, _tp.googlenet_widths(rates)):
            out[blk + ".branch3x3.3"], out[blk + ".branch5x5.3"], out[blk + ".branch5x5.6"] = w[1], w[2], w[3]
        return out
    return {n: o for n, o, _ in _tp.u2netp_conv_shapes(rates)}


def _kept(name, rates):
    by = _kept_by_module(name, rates)
    return tuple(by[module] for _, module, _ in _rows(name))


def widths(name, rates):
    """[(score file stem, original width, kept width)], one row per conv a score file selects rows for, unchanged convs
    included, in transplant.dataflow order: GoogLeNet's _n5x5 file once per conv it serves, the CIFAR stems included,
    VGG's 13th conv (no file, never shrinks) not. Derived from the width tables of transplant.py."""
    rates = _check_len(name, rates)
    return [(stem, o, c) for (stem, _, o), c in zip(_rows(name), _kept(name, rates))]


_MOVES = {}


def _moves(name):
    """(moved, owner): moved[i] is the set of rows of widths() that change when rate i alone goes from 0 to _PROBE,
    owner[row] the LAST index that moves the row (None: no rate does). An index governs the rows it owns; a row it
    moves and does not own has a rate of its own further on and follows."""
    if name not in _MOVES:
        n = nets.RATE_LEN[name]
        zero = _kept(name, [0.0] * n)
        moved, owner = [], [None] * len(zero)
        for i in range(n):
            r = [0.0] * n
            r[i] = _PROBE
            rows = frozenset(k for k, (a, b) in enumerate(zip(zero, _kept(name, r))) if a != b)
            moved.append(rows)
            for k in rows:
                owner[k] = i
        coupled = [tuple(j for j in range(n) if j != i and moved[j] & moved[i]) for i in range(n)]
        _MOVES[name] = (tuple(moved), tuple(owner), tuple(coupled))
    return _MOVES[name]


def owners(name):
    """Per row of widths(name, ...): the rate index that governs it - the last one that moves it - or None."""
    return _moves(name)[1]


def moved(name):
    """Per rate index: the rows of widths(name, ...) that move with it (a frozenset; empty for a rate no constructor reads)."""
    return _moves(name)[0]


def removed_share(scores, original, kept):
    """lambda: the share of a layer's total score that the filters masks.select_index(scores, original, kept) drops
    carry, in float64 - 0.0 when kept == original or the scores sum to 0, 0.0 exactly while only zero scores go, never
    smaller at a smaller `kept` (the removed sets are nested, and the removed scores are summed in ascending order, so
    each further filter adds a non-negative term to the same running sum).

    scores: 1-D, `original` of them, finite and >= 0; anything else is a ValueError."""
    s = np.asarray(scores)
    if s.ndim == 2:
        raise ValueError("the score file holds a [%d, %d] array, not one score per filter: reduce a [C, K] band spectrum first "
                         "with python -m dct_pruning_amd.bands, a [C, C] pair matrix with python -m dct_pruning_amd.pairs"
                         % s.shape)
    if s.ndim != 1:
        raise ValueError("the score file holds a %d-dimensional array, not one score per filter" % s.ndim)
    if s.shape[0] != original:
        raise ValueError("the score file holds %d scores, its convolution has %d filters" % (s.shape[0], original))
    if not 0 <= kept <= original:
        raise ValueError("kept width %d is not in 0 .. %d" % (kept, original))
    s = s.astype(np.float64)
    if not np.isfinite(s).all():
        raise ValueError("the score file holds %d scores that are not finite" % int((~np.isfinite(s)).sum()))
    if (s < 0).any():
        raise ValueError("the score file holds %d negative scores: a share needs scores >= 0" % int((s < 0).sum()))
    if kept == original:
        return 0.0
    total = float(np.cumsum(np.sort(s))[-1])
    if total == 0.0:
        return 0.0
    gone = np.ones(original, dtype=bool)
    gone[select_index(np.asarray(scores), original, kept)] = False
    return float(np.cumsum(np.sort(s[gone]))[-1]) / total


def format_rate(r):
    """`r` as a fixed-point decimal of at most 6 places that parses back to exactly `r` (ValueError if none does)."""
    text = ("%.6f" % r).rstrip("0")
    text += "0" if text.endswith(".") else ""
    if float(text) != r:
        raise ValueError("rate %r needs more than 6 decimal places" % (r,))
    return text


def to_text(rates):
    """The rate list in the reference's DSL: [r]*n+[r]+..., equal neighbours grouped."""
    terms, k = [], 0
    while k < len(rates):
        n = 1
        while k + n < len(rates) and rates[k + n] == rates[k]:
            n += 1
        terms.append("[%s]" % format_rate(rates[k]) + ("*%d" % n if n > 1 else ""))
        k += n
    return "+".join(terms)


def _decimal(lo, hi):
    """The rate for the grid interval lo .. hi (every k / 10^6 in it gives the same widths): on the coarsest of the grids
    10^-2 .. 10^-6 that has a point inside, the largest point. Two places is where the search starts because that is how
    the reference writes its lists; the largest because the interval's upper end is where a width is met exactly (C / 4
    removed: 0.25)."""
    for places in range(2, 7):
        unit = 10 ** (6 - places)
        k = hi // unit * unit
        if k >= lo:
            return k / _SCALE
    raise AssertionError("empty interval")


_WALKS = {}


def walk(name, i, rates, max_rate=0.9):
    """[Step]: the distinct width tuples rates[i] in [rates[i], max_rate] can produce with every other rate as given, in
    order of growing removal, found by bisection on the grid k / 10^6 through the width tables (every width is
    non-increasing in every rate, in float arithmetic too: 1 - r, the product and int() are monotone). Step 0 is the
    list as given. The walk ends before any width reaches 0."""
    rates = _check_len(name, rates)
    moved, _, coupled = _moves(name)
    key = (name, i, rates[i], max_rate, tuple(rates[j] for j in coupled[i]))
    if key in _WALKS:
        return _WALKS[key]
    rows = sorted(moved[i])

    def at(r):
        rr = list(rates)
        rr[i] = r
        k = _kept(name, rr)
        return tuple(k[x] for x in rows)

    t0 = at(rates[i])
    k0, k1 = int(math.ceil(rates[i] * _SCALE)), int(math.floor(max_rate * _SCALE))
    k0 += k0 / _SCALE < rates[i]
    k1 -= k1 / _SCALE > max_rate
    steps = [Step(rates[i], dict(zip(rows, t0)))]
    if rows and k0 <= k1:
        memo = {k0: at(k0 / _SCALE), k1: at(k1 / _SCALE)}
        starts, todo = [k0], [(k0, k1)]  # starts: the first k of each run of equal tuples
        while todo:
            lo, hi = todo.pop()
            if memo[lo] == memo[hi]:
                continue
            if hi == lo + 1:
                starts.append(hi)
                continue
            mid = (lo + hi) // 2
            memo[mid] = at(mid / _SCALE)
            todo += [(lo, mid), (mid, hi)]
        starts.sort()
        for lo, nxt in zip(starts, starts[1:] + [k1 + 1]):
            t = memo[lo]
            if min(t) <= 0:
                break
            if t != t0:
                steps.append(Step(_decimal(lo, nxt - 1), dict(zip(rows, t))))
    if len(_WALKS) > 4096:
        _WALKS.clear()
    _WALKS[key] = steps
    return steps


def _setup(name, base, free, max_rate):
    if name not in FREE:
        raise ValueError("the network name you have entered is not supported yet: %r" % (name,))
    n = nets.RATE_LEN[name]
    base = [0.0] * n if base is None else [float(r) for r in base]
    if len(base) < n:
        raise ValueError("%s reads %d rates, base has %d" % (name, n, len(base)))
    free = FREE[name] if free is None else tuple(sorted(set(int(i) for i in free)))
    for i in free:
        if not 0 <= i < n:
            raise ValueError("free index %d is not in 0 .. %d, the rates %s reads" % (i, n - 1, name))
    if not 0 <= max_rate < 1:
        raise ValueError("max_rate is in [0, 1), not %r" % (max_rate,))
    for i in free:
        if not 0 <= base[i] <= max_rate:
            raise ValueError("base[%d] = %r is not in [0, max_rate = %r]" % (i, base[i], max_rate))
    return base, free


class _Shares:
    """lambda per (row, kept width), each computed once; the score file of a row is read when a share of it is first asked for."""

    def __init__(self, name, imp_score):
        self.name, self.imp, self.memo, self.files = name, imp_score, {}, {}

    def __call__(self, row, kept):
        stem, _, original = _rows(self.name)[row]
        if kept == original:
            return 0.0
        if (row, kept) not in self.memo:
            if stem not in self.files:
                self.files[stem] = _tp._load_imp(self.imp, stem)
            try:
                self.memo[row, kept] = removed_share(self.files[stem], original, kept)
            except ValueError as exc:
                raise ValueError("%s: %s" % (stem, exc))
        return self.memo[row, kept]


def _level(name, share, eps, base, free, max_rate, met=None):
    """The rate list at level eps; `met` collects every share looked at on the way."""
    if not 0 <= eps <= 1:
        raise ValueError("a level is a share of a layer's score, in [0, 1], not %r" % (eps,))
    owner = _moves(name)[1]
    rates = list(base)
    for i in free:
        steps = walk(name, i, rates, max_rate)
        held = [row for row in steps[0].kept if owner[row] == i]
        for step in steps[1:]:
            lams = [share(row, step.kept[row]) for row in held if step.kept[row] != steps[0].kept[row]]
            if met is not None:
                met.update(lams)
            if any(lam > eps for lam in lams):
                break  # the shares never fall again: the first failure ends the walk
            rates[i] = step.rate
    return rates


def at_level(name, imp_score, eps, base=None, free=None, max_rate=0.9):
    """The rate list at level eps: from `base` (default all 0.0), every index of `free` (default FREE[name]) in ascending
    order walks through the width tuples its rate can produce up to max_rate (walk) and keeps the last step at which
    every file it governs, and whose width differs from step 0's, has removed_share <= eps. Every other index keeps its
    base value. imp_score: a score directory or a {stem: scores} dict. Needs 0 <= base[i] <= max_rate < 1 on the free
    indices (ValueError otherwise)."""
    base, free = _setup(name, base, free, max_rate)
    return _level(name, _Shares(name, imp_score), eps, base, free, max_rate)


def levels(name, imp_score, base=None, free=None, max_rate=0.9):
    """E, sorted: 0 and every share met on the walk at eps = 1. The level allocate returns is one of these."""
    base, free = _setup(name, base, free, max_rate)
    met = {0.0}
    _level(name, _Shares(name, imp_score), 1.0, base, free, max_rate, met)
    return sorted(met)


_COSTS = {}


def _cost(name, rates, input_shape):
    """prune.cost of the net built from `rates`; the widths decide it, so it is computed once per width tuple."""
    from .prune import cost
    key = (name, _kept(name, rates), tuple(input_shape))
    if key not in _COSTS:
        if len(_COSTS) > 1024:
            _COSTS.clear()
        _COSTS[key] = cost(nets.get_network(name, rates), input_shape)
    return _COSTS[key]


def _files(name, share, rates, base, free):
    owner = _moves(name)[1]
    before = _kept(name, base)
    out = []
    for row, (stem, o, c) in enumerate(widths(name, rates)):
        tag = "free" if owner[row] in free else "forced" if c != before[row] else "fixed"
        out.append((stem, o, c, share(row, c), tag))
    return out


def allocate(name, imp_score, target_macs=None, target_params=None, max_loss=None, base=None, free=None, max_rate=0.9,
             input_shape=None):
    """The equal-loss allocation that meets a budget, as an Allocation.

    target_macs, target_params: the fraction of the full net's count that may remain, in (0, 1]; max_loss: the largest
    level allowed. At least one of the three is needed. With max_loss alone the result is at_level(max_loss). With
    targets, `level` is the smallest element of levels(...) whose allocation meets every target given, found by bisection
    (valid because rates grow and costs fall with the level: DESIGN.md §7o); a level above max_loss, and a target that
    even level 1 misses, are ValueErrors - the latter names the smallest reachable fraction. Counts are
    prune.cost(nets.get_network(name, rates), input_shape), input_shape defaulting to the net's dataset's."""
    from .data import INPUT_SHAPES, NET_DATASET
    if target_macs is None and target_params is None and max_loss is None:
        raise ValueError("allocate needs a goal: target_macs, target_params or max_loss")
    for what, t in (("target_macs", target_macs), ("target_params", target_params)):
        if t is not None and not 0 < t <= 1:
            raise ValueError("%s is the fraction of the full net that may remain, in (0, 1], not %r" % (what, t))
    if max_loss is not None and not 0 <= max_loss <= 1:
        raise ValueError("max_loss is a share of a layer's score, in [0, 1], not %r" % (max_loss,))
    base, free = _setup(name, base, free, max_rate)
    shape = tuple(input_shape) if input_shape is not None else INPUT_SHAPES[NET_DATASET[name]]
    share = _Shares(name, imp_score)
    full = _cost(name, [0.0] * nets.RATE_LEN[name], shape)

    def solve(eps):
        rates = _level(name, share, eps, base, free, max_rate)
        return rates, _cost(name, rates, shape)

    def meets(c):
        return ((target_macs is None or c["macs"] <= target_macs * full["macs"])
                and (target_params is None or c["params"] <= target_params * full["params"]))

    if target_macs is None and target_params is None:
        level = float(max_loss)
        rates, c = solve(level)
    else:
        met = {0.0}
        _level(name, share, 1.0, base, free, max_rate, met)
        grid = sorted(met)
        rates, c = solve(grid[-1])
        if not meets(c):
            raise ValueError("the target is out of reach: with every free rate at its largest admissible value (max_rate %g) "
                             "%s keeps %.6f of the MACs and %.6f of the parameters"
                             % (max_rate, name, c["macs"] / full["macs"], c["params"] / full["params"]))
        lo, hi = 0, len(grid) - 1  # grid[hi] meets; the smallest index that does
        while lo < hi:
            mid = (lo + hi) // 2
            if meets(solve(grid[mid])[1]):
                hi = mid
            else:
                lo = mid + 1
        level = grid[hi]
        rates, c = solve(level)
        if max_loss is not None and level > max_loss:
            raise ValueError("the target needs level %.6g, above max_loss %.6g" % (level, max_loss))
    text = to_text(rates)
    if widths(name, parse_compress_rate(text)) != widths(name, rates):
        raise ValueError("the rate list %s does not reproduce its widths in 6 decimal places" % (rates,))
    return Allocation(rates, text, level, c["macs"], c["params"], full["macs"], full["params"],
                      _files(name, share, rates, base, free))


def parse_free(text):
    """'i,j-k' -> (i, j, ..., k)."""
    out = []
    for part in text.split(","):
        a, _, b = part.strip().partition("-")
        try:
            out += range(int(a), int(b or a) + 1)
        except ValueError:
            raise ValueError("--free takes indices and ranges, 'i,j-k', not %r" % (part,))
    return tuple(out)


def main(argv=None):
    from .data import INPUT_SHAPES, NET_DATASET
    ap = argparse.ArgumentParser(prog="python -m dct_pruning_amd.rates", description=__doc__.split("\n")[0])
    ap.add_argument("--net", required=True, choices=tuple(FREE), help="net type")
    ap.add_argument("--imp_score", required=True, help="directory of score files (importance_score/<net>_limit<L>)")
    ap.add_argument("--target_macs", type=float, default=None, help="fraction of the full net's MACs that may remain, in (0, 1]")
    ap.add_argument("--target_params", type=float, default=None, help="fraction of the full net's parameters that may remain")
    ap.add_argument("--max_loss", type=float, default=None, help="largest share of its score a layer may lose; alone: the level itself")
    ap.add_argument("--max_rate", type=float, default=0.9, help="no free rate goes above this")
    ap.add_argument("--base", default=None, help="reference DSL: the list the solver starts from and the fixed indices keep (default all 0.)")
    ap.add_argument("--free", default=None, help="the rate indices the solver moves, 'i,j-k' (default: rates.FREE[net])")
    ap.add_argument("--input_size", type=int, default=None, help="H=W of the input the MACs are counted on (default: the dataset's)")
    ap.add_argument("--json", default=None, help="write the Allocation's fields to this file")
    args = ap.parse_args(argv)
    shape = list(INPUT_SHAPES[NET_DATASET[args.net]])
    if args.input_size:
        shape[1] = shape[2] = args.input_size
    try:
        alloc = allocate(args.net, args.imp_score, args.target_macs, args.target_params, args.max_loss,
                         base=parse_compress_rate(args.base) if args.base else None,
                         free=parse_free(args.free) if args.free else None, max_rate=args.max_rate, input_shape=shape)
    except (ValueError, OSError) as exc:  # no goal, unreachable target, bad list, missing or wrong-shaped score file
        ap.error(str(exc))
    print(alloc.text)
    print("level %.6g: MACs %d (%.2f %% kept), params %d (%.2f %% kept)" % (
        alloc.level, alloc.macs, 100.0 * alloc.macs / alloc.full_macs, alloc.params, 100.0 * alloc.params / alloc.full_params))
    owner = owners(args.net)
    start = parse_compress_rate(args.base) if args.base else [0.0] * len(alloc.rates)
    for i, (r, b) in enumerate(zip(alloc.rates, start)):
        if r != b:
            print("rate %d: %s -> %s  %s" % (i, format_rate(b), format_rate(r), ", ".join(
                "%s %d -> %d (%.4g)" % (stem, o, c, lam) for row, (stem, o, c, lam, _) in enumerate(alloc.files) if owner[row] == i)))
    forced = ["%s %d -> %d (%.4g)" % (stem, o, c, lam) for stem, o, c, lam, tag in alloc.files if tag == "forced"]
    if forced:
        print("forced: " + ", ".join(forced))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(alloc._asdict(), f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
