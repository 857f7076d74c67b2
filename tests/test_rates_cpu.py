"""rates.py on the CPU: from score files and a MACs or parameter budget to the compress-rate list.

Widths, counts and rate lists are integers or exact decimals and compared as such; a share (lambda) is compared with the
float64 value the definition gives, bit for bit where the sum is taken in the definition's order and to 1e-12 where a test
sums in another (at most 512 float64 terms of one sign: 512 x 2^-53 = 6e-14 of the sum). The score files are
carry_cases.dead_scores: 0.0 at index % 4 == 0 of the files whose convs lose filters at carry_cases.RATES, in [1, 2)
elsewhere.
"""
import functools
import json

import numpy as np
import pytest
import torch

import carry_cases as cc
import pruned_cases as pc
from dct_pruning_amd import masks, nets, prune
from dct_pruning_amd import rates as R
from dct_pruning_amd import transplant as tp
from dct_pruning_amd.masks import parse_compress_rate

SHAPES = {"resnet_50": (3, 64, 64), "u2netp": (3, 72, 72)}  # the others: their dataset's (3, 32, 32)
LADDER = [0.0, 0.05, 0.1, 0.2, 0.4, 1.0]
# where the all-zero list cannot reach the target: the list the case starts from (the five outer rates of U2-Net-p)
BASES = {("u2netp", 0.5): [0.0] * 34 + [0.25] * 5}


@functools.lru_cache(None)
def scores(name):
    _, stems = cc.dead_net(name)
    return cc.dead_scores(name, stems)


def shape_of(name):
    return SHAPES.get(name, (3, 32, 32))


def cost_of(name, rates):
    return prune.cost(nets.get_network(name, rates), shape_of(name))


def ragged(name):
    r = [0.0] * nets.RATE_LEN[name]
    for i in R.FREE[name]:
        r[i] = 0.3
    return r


# ---------------------------------------------------------------------------------------------------------
# 1, 2: the free indices and the width rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NETS)
def test_free_is_the_nonzero_positions_of_the_carry_rates(name):
    assert R.FREE[name] == tuple(i for i, r in enumerate(cc.RATES[name]) if r != 0)
    assert set(R.FREE) == set(pc.NETS)


@pytest.mark.parametrize("name", pc.NETS)
def test_a_free_index_governs_rows_no_other_index_moves(name):
    """what makes rates grow and costs fall with the level; followers exist in DenseNet-40 only"""
    moved, owner = R.moved(name), R.owners(name)
    assert len(moved) == nets.RATE_LEN[name] and len(owner) == len(R.widths(name, [0.0] * nets.RATE_LEN[name]))
    for i in R.FREE[name]:
        mine = {row for row, o in enumerate(owner) if o == i}
        assert mine and mine <= moved[i]
        assert not [j for j in range(len(moved)) if j != i and moved[j] & mine]
    shared = {row for row in range(len(owner)) if sum(row in m for m in moved) > 1}
    stems = sorted(R.widths(name, [0.0] * nets.RATE_LEN[name])[row][0] for row in shared)
    assert stems == (["imp_conv14", "imp_conv27"] if name == "densenet_40" else [])
    assert [owner[row] for row in sorted(shared)] == ([13, 26] if name == "densenet_40" else [])


@pytest.mark.parametrize("name", pc.NETS)
@pytest.mark.parametrize("which", ["carry", "ragged"])
def test_widths_are_the_tables_and_the_constructors(name, which):
    rates = cc.RATES[name] if which == "carry" else ragged(name)
    rows = R.widths(name, rates)
    assert sorted(r for r in rows if r[1] != r[2]) == sorted(cc.shrunk(name, rates)) and cc.shrunk(name, rates)
    convs = [f for f in tp.dataflow(name) if f.kind == "conv" and f.stem is not None]
    assert [(f.stem, f.width) for f in convs] == [(s, o) for s, o, _ in rows]  # one row per conv with a file, dataflow order
    sd = nets.get_network(name, rates).state_dict()
    assert [sd[f.module + ".weight"].shape[0] for f in convs] == [c for _, _, c in rows]
    assert all(isinstance(c, int) for _, _, c in rows)


def test_widths_lists_shared_files_once_per_conv_and_the_cifar_stems():
    g = R.widths("googlenet", cc.RATES["googlenet"])
    assert [s for s, _, _ in g].count("imp_conv2_n5x5") == 2 and len(g) == 27
    assert R.widths("resnet_56", [0.5] + [0.0] * 29)[0] == ("imp_conv1", 16, 8)
    assert len(R.widths("vgg_16_bn", [0.0] * 12)) == 12  # the 13th conv has no file
    with pytest.raises(ValueError, match="12 rates"):
        R.widths("vgg_16_bn", [0.0] * 11)
    with pytest.raises(ValueError, match="alexnet"):
        R.widths("alexnet", [0.0] * 12)


# ---------------------------------------------------------------------------------------------------------
# 3: the share
# ---------------------------------------------------------------------------------------------------------
def test_removed_share_by_hand():
    s = np.array([4.0, 1.0, 3.0, 2.0], dtype=np.float32)
    assert R.removed_share(s, 4, 4) == 0.0
    assert R.removed_share(s, 4, 3) == 1.0 / 10.0
    assert R.removed_share(s, 4, 2) == 3.0 / 10.0
    assert R.removed_share(s, 4, 1) == 6.0 / 10.0
    assert R.removed_share(s, 4, 0) == 1.0
    # ties: whichever of the equal filters select_index drops, the share is the same
    t = np.array([2.0, 1.0, 1.0, 1.0, 5.0])
    assert R.removed_share(t, 5, 4) == 0.1 and R.removed_share(t, 5, 3) == 0.2 and R.removed_share(t, 5, 1) == 0.5
    assert R.removed_share(np.zeros(6), 6, 2) == 0.0  # an all-zero file: nothing to lose
    assert isinstance(R.removed_share(s, 4, 2), float)


def test_removed_share_describes_the_filters_select_index_removes():
    s = np.random.RandomState(3).rand(37).astype(np.float32)
    for kept in (36, 20, 1):
        gone = np.setdiff1d(np.arange(37), masks.select_index(s, 37, kept))
        want = float(np.sort(s[gone].astype(np.float64)).cumsum()[-1]) / float(np.sort(s.astype(np.float64)).cumsum()[-1])
        assert R.removed_share(s, 37, kept) == want


@pytest.mark.parametrize("seed", range(4))
def test_removed_share_never_decreases_as_the_width_shrinks(seed):
    rng = np.random.RandomState(seed)
    c = 97
    s = (rng.rand(c) * 10.0 ** rng.randint(-6, 6, c)).astype(np.float32)  # many magnitudes: sums that round
    s[rng.rand(c) < 0.2] = 0.0
    lam = [R.removed_share(s, c, kept) for kept in range(c, 0, -1)]
    assert all(b >= a for a, b in zip(lam, lam[1:])) and lam[0] == 0.0 and 0 < lam[-1] <= 1.0
    zeros = int((s == 0).sum())
    assert zeros > 3 and all(x == 0.0 for x in lam[:zeros + 1]) and lam[zeros + 1] > 0.0  # exactly 0 while only zeros go


def test_removed_share_refuses_what_is_not_a_score_file():
    ok = np.arange(8.0)
    with pytest.raises(ValueError, match="negative"):
        R.removed_share(np.array([1.0, -1.0, 2.0]), 3, 2)
    with pytest.raises(ValueError, match="not finite"):
        R.removed_share(np.array([1.0, np.nan, 2.0]), 3, 2)
    with pytest.raises(ValueError, match="not finite"):
        R.removed_share(np.array([1.0, np.inf, 2.0]), 3, 2)
    with pytest.raises(ValueError, match="8 scores.*9 filters"):
        R.removed_share(ok, 9, 4)
    with pytest.raises(ValueError, match=r"\[8, 4\].*dct_pruning_amd\.bands.*dct_pruning_amd\.pairs"):
        R.removed_share(np.ones((8, 4)), 8, 4)
    with pytest.raises(ValueError, match="3-dimensional"):
        R.removed_share(np.ones((8, 1, 1)), 8, 4)
    with pytest.raises(ValueError, match="kept width"):
        R.removed_share(ok, 8, 9)


# ---------------------------------------------------------------------------------------------------------
# 4: zero loss finds the dead filters
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NETS)
def test_zero_loss_finds_the_dead_filters(name):
    a = R.allocate(name, scores(name), max_loss=0.0, input_shape=shape_of(name))
    assert R.widths(name, a.rates) == R.widths(name, cc.RATES[name])
    assert a.level == 0.0 and all(f[3] == 0.0 for f in a.files)
    assert [(s, o, c) for s, o, c, _, _ in a.files] == R.widths(name, a.rates)
    terms = set(t.split("*")[0] for t in a.text.split("+"))
    assert "[0.25]" in terms and terms <= {"[0.]", "[0.0]", "[0.25]"}
    assert parse_compress_rate(a.text) == a.rates == R.at_level(name, scores(name), 0.0)
    want = cost_of(name, cc.RATES[name])
    assert (a.macs, a.params) == (want["macs"], want["params"])
    # DenseNet's transitions have no free rate and shrink all the same: forced, and inside their dead sets
    forced = [f[:3] for f in a.files if f[4] == "forced"]
    assert forced == ([("imp_conv14", 168, 132), ("imp_conv27", 312, 240)] if name == "densenet_40" else [])


# ---------------------------------------------------------------------------------------------------------
# 5: budgets
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NETS)
@pytest.mark.parametrize("target", [0.7, 0.5])
def test_budget_is_met_at_the_smallest_level(name, target):
    """target_macs, target_params and both at once, on dead_scores. Measured (level, MACs kept, params kept) for
    target_macs: DESIGN.md §7o.

    u2netp at 0.5 starts from BASES: from the all-zero list half of U2-Net-p is out of reach. With all 34 inner rates at
    the point where every inner width is 1 (the constructor keeps at least one channel, and the two deepest convs of an
    RSU keep all 16) the net still holds 0.609574 of its MACs on a 72 x 72 input and 0.542235 of its parameters
    (0.609858 and 0.542235 at 288 x 288): the outer widths, which end in d + xin and are not free, carry the rest. The
    case asserts that first, then does what a user has to do: it sets the five outer rates to 0.25 in `base`, which the
    solver keeps, and asks for half of the FULL net. Every assertion is the same as for the other thirteen cases."""
    imp, shape = scores(name), shape_of(name)
    base = BASES.get((name, target), [0.0] * nets.RATE_LEN[name])
    full = cost_of(name, [0.0] * nets.RATE_LEN[name])
    if (name, target) in BASES:
        with pytest.raises(ValueError, match="out of reach.*0.609574 of the MACs and 0.542235 of the parameters"):
            R.allocate(name, imp, input_shape=shape, target_macs=target)
        with pytest.raises(ValueError, match="out of reach"):
            R.allocate(name, imp, input_shape=shape, target_params=target)
    grid = R.levels(name, imp, base=base)
    assert grid[0] == 0.0 and grid == sorted(set(grid)) and grid[-1] <= 1.0
    for goal in ({"target_macs": target}, {"target_params": target}, {"target_macs": target, "target_params": target}):
        a = R.allocate(name, imp, input_shape=shape, base=base, **goal)
        print("%s %s: level %.6g, MACs %.4f, params %.4f of the full net" % (name, goal, a.level, a.macs / full["macs"],
                                                                           a.params / full["params"]))
        assert (a.full_macs, a.full_params) == (full["macs"], full["params"])
        if "target_macs" in goal:
            assert a.macs <= target * full["macs"]
        if "target_params" in goal:
            assert a.params <= target * full["params"]
        got = cost_of(name, parse_compress_rate(a.text))
        assert (a.macs, a.params) == (got["macs"], got["params"])
        assert all(lam <= a.level for _, _, _, lam, tag in a.files if tag == "free")
        assert all(a.rates[i] == base[i] for i in range(len(a.rates)) if i not in R.FREE[name])
        assert all(a.rates[i] >= base[i] for i in R.FREE[name])
        assert a.level in grid
        k = grid.index(a.level)
        if k:  # minimality: one level down misses
            c = cost_of(name, R.at_level(name, imp, grid[k - 1], base=base))
            assert (("target_macs" in goal and c["macs"] > target * full["macs"])
                    or ("target_params" in goal and c["params"] > target * full["params"]))
    if (name, target) in BASES:
        assert a.level > 0 and [f[4] for f in a.files].count("forced") == 0


# ---------------------------------------------------------------------------------------------------------
# 6: monotone in the level; the smallest maximum
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NETS)
def test_rates_grow_and_costs_fall_with_the_level(name):
    prev = None
    for eps in LADDER:
        rates = R.at_level(name, scores(name), eps)
        c = cost_of(name, rates)
        if prev is not None:
            assert all(b >= a for a, b in zip(prev[0], rates))
            assert c["macs"] <= prev[1]["macs"] and c["params"] <= prev[1]["params"]
        prev = (rates, c)
    assert prev[0] != R.at_level(name, scores(name), 0.0)


def test_no_allocation_with_a_smaller_largest_share_meets_the_target():
    """VGG-16-bn with three free rates (convs of 64, 64 and 128 filters), live scores, every admissible width triple."""
    name, free, target = "vgg_16_bn", (0, 1, 2), 0.85
    rng = np.random.RandomState(11)
    imp = {stem: (rng.rand(c) ** 2).astype(np.float32) for stem, c in pc.transplant_fixture(name)["stems"]}
    a = R.allocate(name, imp, target_macs=target, free=free)
    assert a.level > 0 and a.macs <= target * a.full_macs
    walks = [R.walk(name, i, [0.0] * 12, 0.9) for i in free]
    w = [np.array([s.kept[i] for s in walk]) for i, walk in zip(free, walks)]
    assert [list(ws) for ws in w] == [list(range(64, 5, -1)), list(range(64, 5, -1)), list(range(128, 11, -1))]  # int(C * (1 - 0.9))
    lam = [np.array([R.removed_share(imp["imp_conv%d" % (i + 1)], int(ws[0]), int(c)) for c in ws]) for i, ws in zip(free, w)]

    def macs(w0, w1, w2):  # the four convs whose MACs move: 3 -> w0 -> w1 at 32 x 32, w1 -> w2 -> 128 at 16 x 16
        return 9 * 1024 * (3 * w0 + w0 * w1) + 9 * 256 * (w1 * w2 + w2 * 128)

    rest = a.full_macs - macs(64, 64, 128)
    for pick in ((5, 9, 30), (57, 0, 115), (20, 57, 1)):  # the formula is prune.cost
        rates = [walk[k].rate for walk, k in zip(walks, pick)] + [0.0] * 9
        assert cost_of(name, rates)["macs"] == rest + macs(*[int(ws[k]) for ws, k in zip(w, pick)])
    total = rest + macs(w[0][:, None, None], w[1][None, :, None], w[2][None, None, :])
    worst = np.maximum(np.maximum(lam[0][:, None, None], lam[1][None, :, None]), lam[2][None, None, :])
    feasible = total <= target * a.full_macs
    assert feasible.any() and not feasible.all()
    assert worst[feasible].min() == a.level
    assert max(f[3] for f in a.files) == a.level


# ---------------------------------------------------------------------------------------------------------
# 7: the rounding trap
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.NETS)
def test_every_emitted_decimal_reproduces_its_widths(name):
    n = nets.RATE_LEN[name]
    zero = R.widths(name, [0.0] * n)
    seen = set()
    for i in R.FREE[name]:
        steps = R.walk(name, i, [0.0] * n, 0.9)
        originals = tuple(sorted(zero[row][1] for row in steps[0].kept))
        if originals in seen:  # one index per set of original widths: the arithmetic is the same
            continue
        seen.add(originals)
        assert steps[0].rate == 0.0 and len(steps) > 1
        for a, b in zip(steps, steps[1:]):
            assert b.rate > a.rate and a.kept != b.kept
        for step in steps:
            rates = [0.0] * n
            rates[i] = step.rate
            text = R.to_text(rates)
            assert "e" not in text and len(R.format_rate(step.rate).split(".")[1]) <= 6
            rows = R.widths(name, parse_compress_rate(text))
            assert {row: rows[row][2] for row in step.kept} == step.kept
        # every kept width from the original down to what max_rate leaves (at least 1) is reached
        for row in steps[0].kept:
            if name == "densenet_40" and zero[row][0] in ("imp_conv14", "imp_conv27"):
                continue  # followers: they move with the dense rate, a filter at a time
            rates = [0.0] * n
            rates[i] = 0.9
            low = max(1, R.widths(name, rates)[row][2])
            assert sorted(set(s.kept[row] for s in steps)) == list(range(low, zero[row][1] + 1)), (i, zero[row])
    # every original width a free rate governs was walked
    assert {o for t in seen for o in t} >= {o for (_, o, _), i in zip(zero, R.owners(name)) if i in R.FREE[name]}


def test_removed_over_width_is_not_the_rate():
    """48 filters, 17 removed: 17 / 48 keeps 30, not 31 (GoogLeNet's inception_a4 has 48 filters in its 5x5 branch)"""
    assert int(48 * (1 - 17 / 48)) == 30
    rates = [0.0] * 10
    rates[3] = 17 / 48
    rows = R.widths("googlenet", rates)
    hit = [k for k, (s, o, _) in enumerate(rows) if s == "imp_conv4_n5x5"]
    assert [rows[k][1:] for k in hit] == [(48, 30), (48, 30)]
    steps = [s for s in R.walk("googlenet", 3, [0.0] * 10) if s.kept[hit[0]] == 31]
    assert len(steps) > 1  # the rate moves the block's 3x3 conv (208 filters) too: several tuples hold 31
    for step in steps:
        assert 1 - 32 / 48 < step.rate <= 1 - 31 / 48 and step.rate != 17 / 48
        rates[3] = step.rate
        assert [R.widths("googlenet", parse_compress_rate(R.to_text(rates)))[k][2] for k in hit] == [31, 31]
    assert 0.35 in [s.rate for s in steps]


def test_text_is_run_length_grouped_fixed_point():
    assert R.to_text([0.0, 0.25, 0.25, 0.25, 0.5, 0.0, 0.0]) == "[0.0]+[0.25]*3+[0.5]+[0.0]*2"
    assert R.to_text([0.000001]) == "[0.000001]" and parse_compress_rate("[0.000001]") == [0.000001]
    with pytest.raises(ValueError, match="6 decimal places"):
        R.to_text([1.0 / 3.0])


# ---------------------------------------------------------------------------------------------------------
# 8: refusals
# ---------------------------------------------------------------------------------------------------------
def test_allocate_refuses_bad_goals():
    imp = scores("vgg_16_bn")
    with pytest.raises(ValueError, match="needs a goal"):
        R.allocate("vgg_16_bn", imp)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            R.allocate("vgg_16_bn", imp, target_macs=bad)
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            R.allocate("vgg_16_bn", imp, target_params=bad)
    with pytest.raises(ValueError, match="max_loss"):
        R.allocate("vgg_16_bn", imp, max_loss=1.5)
    with pytest.raises(ValueError, match="alexnet"):
        R.allocate("alexnet", imp, max_loss=0.0)
    a = R.allocate("vgg_16_bn", imp, target_macs=1.0)  # 1 is allowed, and nothing has to go
    assert a.level == 0.0 and a.rates == R.at_level("vgg_16_bn", imp, 0.0)


@pytest.mark.parametrize("name", ["vgg_16_bn", "u2netp"])
def test_unreachable_target_names_the_reachable_fraction(name):
    imp = scores(name)
    c = cost_of(name, R.at_level(name, imp, 1.0))
    full = cost_of(name, [0.0] * nets.RATE_LEN[name])
    with pytest.raises(ValueError) as exc:
        R.allocate(name, imp, target_macs=0.001, input_shape=shape_of(name))
    assert "out of reach" in str(exc.value)
    assert "%.6f of the MACs" % (c["macs"] / full["macs"]) in str(exc.value)
    assert "%.6f of the parameters" % (c["params"] / full["params"]) in str(exc.value)
    assert 0.001 < c["macs"] / full["macs"] < 1


def test_level_above_max_loss_is_refused():
    imp = scores("vgg_16_bn")
    a = R.allocate("vgg_16_bn", imp, target_macs=0.5)
    assert a.level > 0.01
    with pytest.raises(ValueError, match="above max_loss"):
        R.allocate("vgg_16_bn", imp, target_macs=0.5, max_loss=0.01)
    b = R.allocate("vgg_16_bn", imp, target_macs=0.5, max_loss=a.level)
    assert b == a


def test_bad_rates_and_indices_are_refused():
    imp = scores("vgg_16_bn")
    for max_rate in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="max_rate"):
            R.at_level("vgg_16_bn", imp, 0.1, max_rate=max_rate)
    with pytest.raises(ValueError, match=r"base\[2\]"):
        R.at_level("vgg_16_bn", imp, 0.1, base=[0.0, 0.0, 0.95] + [0.0] * 9)
    with pytest.raises(ValueError, match=r"base\[0\]"):
        R.allocate("vgg_16_bn", imp, max_loss=0.1, base=[-0.1] + [0.0] * 11)
    for bad in ((12,), (-1, 3)):
        with pytest.raises(ValueError, match="free index"):
            R.at_level("vgg_16_bn", imp, 0.1, free=bad)
    with pytest.raises(ValueError, match="base has 11"):
        R.allocate("vgg_16_bn", imp, max_loss=0.1, base=[0.0] * 11)
    with pytest.raises(ValueError, match="level"):
        R.at_level("vgg_16_bn", imp, 1.5)
    # a base above max_rate at an index that is NOT free is the user's business
    assert R.at_level("vgg_16_bn", imp, 0.0, base=[0.0] * 11 + [0.95], free=(0,))[11] == 0.95


def test_band_and_pair_files_are_refused_with_the_tool_that_reduces_them():
    imp = dict(scores("vgg_16_bn"))
    imp["imp_conv3"] = np.ones((128, 4), dtype=np.float32)      # a [C, K] band spectrum
    with pytest.raises(ValueError, match=r"imp_conv3.*\[128, 4\].*dct_pruning_amd\.bands"):
        R.allocate("vgg_16_bn", imp, max_loss=0.1)
    imp["imp_conv3"] = np.ones((128, 128), dtype=np.float32)    # a [C, C] pair matrix
    with pytest.raises(ValueError, match=r"imp_conv3.*\[128, 128\].*dct_pruning_amd\.pairs"):
        R.at_level("vgg_16_bn", imp, 0.1)
    imp["imp_conv3"] = scores("vgg_16_bn")["imp_conv3"][:-1]
    with pytest.raises(ValueError, match="imp_conv3.*127 scores.*128 filters"):
        R.at_level("vgg_16_bn", imp, 0.1)
    del imp["imp_conv3"]
    with pytest.raises(KeyError):
        R.at_level("vgg_16_bn", imp, 0.1)


# ---------------------------------------------------------------------------------------------------------
# 9: base and free
# ---------------------------------------------------------------------------------------------------------
def test_a_freed_transition_is_walked_after_the_dense_rates_before_it():
    """at level 0 on dead_scores: the dense rates leave the transitions 132 of 168 and 240 of 312 wide (forced); the first
    has 42 dead filters and only 36 went, so its own rate takes the other 6: floor(132 * (1 - 0.05)) = 125 is one too many,
    0.04 keeps 126. The second then reads 126 + 108 = 234 channels: its 78 dead filters are gone already and its rate stays."""
    name, imp = "densenet_40", scores("densenet_40")
    free = R.FREE[name] + (13, 26)
    rates = R.at_level(name, imp, 0.0, free=free)
    default = R.at_level(name, imp, 0.0)
    assert [r for i, r in enumerate(rates) if i not in (13, 26)] == [r for i, r in enumerate(default) if i not in (13, 26)]
    rows = {s: c for s, _, c in R.widths(name, rates)}
    assert rows["imp_conv14"] == 126 and rows["imp_conv27"] == 234 and rates[26] == 0.0
    assert rates[13] == 0.04 and int(132 * (1 - 0.04)) == 126 and int(132 * (1 - 0.05)) == 125
    a = R.allocate(name, imp, max_loss=0.0, free=free)
    assert a.rates == rates and all(f[3] == 0.0 for f in a.files) and not [f for f in a.files if f[4] == "forced"]
    # the walk of the transition's rate depends on the dense rates before it: that is why it comes after them
    assert R.walk(name, 13, [0.0] * 39)[-1].kept != R.walk(name, 13, default)[-1].kept


def test_a_user_base_is_kept_at_the_fixed_indices_and_is_where_the_free_ones_start():
    imp = scores("resnet_56")
    base = [0.1, 0.2, 0.3] + [0.0] * 27
    a = R.allocate("resnet_56", imp, target_macs=0.6, base=base)
    assert a.rates[:3] == [0.1, 0.2, 0.3] and a.text.startswith("[0.1]+[0.2]+[0.3]+")
    assert R.widths("resnet_56", parse_compress_rate(a.text)) == R.widths("resnet_56", a.rates)
    assert [f[4] for f in a.files][0] == "fixed" and a.files[0][:3] == ("imp_conv1", 16, 14)
    assert a.files[0][3] == R.removed_share(imp["imp_conv1"], 16, 14)  # reported, not held to the level
    # a free index never goes below its base value
    imp = scores("vgg_16_bn")
    base = [0.5] + [0.0] * 11
    rates = R.at_level("vgg_16_bn", imp, 0.0, base=base, free=(0, 1))
    assert rates == [0.5, 0.25] + [0.0] * 10
    assert R.at_level("vgg_16_bn", imp, 0.3, free=(4,))[:4] == [0.0] * 4


# ---------------------------------------------------------------------------------------------------------
# 10: the command-line tool
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def score_dir(tmp_path):
    d = tmp_path / "scores"
    d.mkdir()
    for stem, s in scores("resnet_56").items():
        np.save(str(d / (stem + ".npy")), s)
    return d


def test_cli_first_line_feeds_masks_and_prune(score_dir, tmp_path, capsys):
    out = tmp_path / "alloc.json"
    assert R.main(["--net", "resnet_56", "--imp_score", str(score_dir), "--target_macs", "0.5", "--json", str(out)]) == 0
    lines = capsys.readouterr().out.splitlines()
    a = R.allocate("resnet_56", str(score_dir), target_macs=0.5)
    assert lines[0] == a.text and parse_compress_rate(lines[0]) == a.rates
    assert lines[1].startswith("level %.6g:" % a.level) and "%.2f %% kept" % (100.0 * a.macs / a.full_macs) in lines[1]
    moved = [i for i, r in enumerate(a.rates) if r != 0.0]
    assert [int(l.split(":")[0].split()[1]) for l in lines[2:]] == moved == list(range(3, 30))
    assert "imp_conv2 16 -> " in lines[2] and "imp_conv4 16 -> " in lines[3]
    saved = json.load(open(str(out)))
    assert set(saved) == set(R.Allocation._fields)
    assert saved["rates"] == a.rates and saved["text"] == a.text and saved["level"] == a.level
    assert (saved["macs"], saved["params"], saved["full_macs"], saved["full_params"]) == (a.macs, a.params, a.full_macs, a.full_params)
    assert [tuple(f) for f in saved["files"]] == a.files
    # prune --carry takes the line as it is: the saved rate list gives the allocation's widths
    pt = tmp_path / "pruned.pt"
    assert prune.main(["--net", "resnet_56", "--imp_score", str(score_dir), "--compress_rate", lines[0], "--carry",
                       "--out", str(pt)]) == 0
    report = capsys.readouterr().out.splitlines()
    assert "MACs %d," % a.macs in report[1] and "params %d," % a.params in report[1]
    got = torch.load(str(pt), weights_only=True)
    assert R.widths("resnet_56", got["compress_rate"]) == [f[:3] for f in a.files]
    nets.get_network("resnet_56", got["compress_rate"]).load_state_dict(got["state_dict"], strict=True)


def test_cli_first_line_feeds_masks(tmp_path, capsys):
    """VGG-16-bn: one file per rate in natural order, which is what masks.py assumes"""
    for stem, _, _ in R.widths("vgg_16_bn", [0.0] * 12):
        np.save(str(tmp_path / (stem + ".npy")), scores("vgg_16_bn")[stem])
    assert R.main(["--net", "vgg_16_bn", "--imp_score", str(tmp_path), "--target_params", "0.5"]) == 0
    line = capsys.readouterr().out.splitlines()[0]
    a = R.allocate("vgg_16_bn", str(tmp_path), target_params=0.5)
    assert line == a.text and a.params <= 0.5 * a.full_params
    npz = tmp_path / "m.npz"
    assert masks.main(["--imp_score", str(tmp_path), "--compress_rate", line, "--out", str(npz)]) == 0
    kept = np.load(str(npz))
    assert [(s, kept[s].size) for s, _, _, _, _ in a.files] == [(s, c) for s, _, c, _, _ in a.files]
    for stem, o, c, lam, _ in a.files:  # the share is the share of exactly the filters the mask drops
        gone = np.setdiff1d(np.arange(o), kept[stem])
        s = scores("vgg_16_bn")[stem].astype(np.float64)
        assert abs(s[gone].sum() / s.sum() - lam) <= 1e-12  # numpy's pairwise sum against the ascending one


def test_cli_options(score_dir, capsys):
    argv = ["--net", "resnet_56", "--imp_score", str(score_dir)]
    assert R.main(argv + ["--max_loss", "0", "--free", "3,5-7", "--base", "[0.1]*3+[0.]*27"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "[0.1]*3+[0.25]+[0.0]+[0.25]*3+[0.0]*22" and len(lines) == 2 + 4
    assert R.main(argv + ["--max_loss", "0", "--input_size", "16"]) == 0
    small = capsys.readouterr().out.splitlines()[1]
    assert R.main(argv + ["--max_loss", "0"]) == 0
    assert capsys.readouterr().out.splitlines()[1] != small  # other MACs, the same rates
    assert R.parse_free("3, 5-7") == (3, 5, 6, 7)


@pytest.mark.parametrize("extra,word", [
    (["--target_macs", "0.001"], "out of reach"),
    ([], "needs a goal"),
    (["--target_params", "1.5"], "(0, 1]"),
    (["--max_loss", "0", "--free", "3,x"], "--free"),
    (["--max_loss", "0", "--free", "40"], "free index"),
    (["--max_loss", "0", "--max_rate", "1"], "max_rate"),
    (["--max_loss", "0", "--base", "[0.]*5"], "base has 5"),
])
def test_cli_errors_exit_through_the_parser(score_dir, capsys, extra, word):
    with pytest.raises(SystemExit) as exc:
        R.main(["--net", "resnet_56", "--imp_score", str(score_dir)] + extra)
    assert exc.value.code == 2 and word in capsys.readouterr().err


def test_cli_missing_score_file_exits_through_the_parser(tmp_path, capsys):
    with pytest.raises(SystemExit) as exc:
        R.main(["--net", "resnet_56", "--imp_score", str(tmp_path), "--max_loss", "0.1"])
    assert exc.value.code == 2 and "imp_conv" in capsys.readouterr().err
