"""The summation order of the cosine-matrix kernel, on the CPU (tests/direct_order.py is the model).

(a) The model is faithful: as one FMA chain per dot product it gives 1.9e-6 on the basis sweep of 80 x 80, the figure
    DESIGN.md section 5 recorded for k_energy_direct on an MI355X while the kernel summed that way.
(b) The record of why the kernel changed: the single chain misses the rule of dct_probes on the basis sweeps of 512 x 3 and
    260 x 9 (on the GPU the kernel gave 1.08e-5 at (128, 1) and 5.5e-6 at (0, 0) against 3.8e-6 and 2.9e-6; the model has the
    same figures, at other maps of the same worst rows: the device's table entries differ from torch's in their last bit).
(c) The order the kernel has now (direct_order.ORDER) meets the bound on both sweeps and on 80 x 80, with half of it to spare.
Why blocks of 16 in runs of 4: with one level of blocks, B terms each, the kernel on the GPU gave on the basis sweeps
    B = 64   2.8e-6 at 512 x 512 (bound 1.9e-6),
    B = 32   1.13e-6 at 264 x 264 (bound 1.96e-6; the model has 1.13e-6 at the same maps: the 32-term chain itself),
    B = 16   9.542e-7 at 512 x 512 (bound 1.907e-6: 0.06 % above half of it; the 32 block sums are a chain again),
so no single level keeps half the bound on every sweep.
(d) That finding as far as it fits on a CPU: blocks of 32 against the kernel's order on ten maps of 264 x 264."""
import pytest

import dct_probes as dp
import direct_order as do

SINGLE_CHAIN = ()
SWEEPS = {(80, 80): dict(k=4, exhaustive=False), (512, 3): dict(exhaustive=True), (260, 9): dict(exhaustive=True)}
_cache = {}


def pairs_of(h, w):
    return dp.cover(h, w, **SWEEPS[(h, w)])


def bound(h, w):
    """The rule of dct_probes on the sweep's own maps: 8 * max(E_ref, 2^-22)."""
    if (h, w) not in _cache:
        _cache[(h, w)] = dp.sweep_tolerance(lambda p: dp.basis_maps(h, w, p), pairs_of(h, w), h, w)[0]
    return _cache[(h, w)]


def worst(h, w, sizes):
    if (h, w, sizes) not in _cache:
        _cache[(h, w, sizes)] = do.worst_basis_error(h, w, pairs_of(h, w), sizes)
    return _cache[(h, w, sizes)]


def test_order_constants_are_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dct_pruning_amd", "csrc", "direct.hip")).read()
    block = int(re.search(r"constexpr int kDirectBlock = (\d+);", src).group(1))
    group = int(re.search(r"constexpr int kDirectGroup = (\d+);", src).group(1))
    assert do.ORDER == (block * group, block)


def test_single_chain_model_reproduces_the_measured_error_at_80():
    err, at = worst(80, 80, SINGLE_CHAIN)
    print("DIRECT_ORDER 80x80 single chain worst=%.3g at %s bound=%.3g" % (err, at, bound(80, 80)))
    assert "%.1e" % err == "1.9e-06", err


@pytest.mark.parametrize("hw", [(512, 3), (260, 9)])
def test_single_chain_misses_the_bound(hw):
    h, w = hw
    err, at = worst(h, w, SINGLE_CHAIN)
    print("DIRECT_ORDER %dx%d single chain worst=%.3g at %s bound=%.3g" % (h, w, err, at, bound(h, w)))
    assert err > bound(h, w), (err, bound(h, w))


@pytest.mark.parametrize("hw", [(512, 3), (260, 9), (80, 80)])
def test_the_kernels_order_meets_the_bound(hw):
    h, w = hw
    err, at = worst(h, w, do.ORDER)
    print("DIRECT_ORDER %dx%d order %s worst=%.3g at %s bound=%.3g" % (h, w, do.ORDER, err, at, bound(h, w)))
    assert err <= bound(h, w) / 2, (err, bound(h, w))


def test_one_level_of_blocks_does_not_keep_half_the_bound():
    """Blocks of 32 at 264 x 264 on ten maps of the rows and columns that are worst there (a constant row or column, or one
    that alternates in long runs: terms of one sign). Blocks of 16 in runs of 4 on the same maps stay under half."""
    import torch
    pairs = torch.tensor([(u, v) for u in (0, 132) for v in (0, 66, 99, 132, 198)])
    tol = dp.sweep_tolerance(lambda p: dp.basis_maps(264, 264, p), dp.cover(264, 264), 264, 264)[0]
    one = do.worst_basis_error(264, 264, pairs, (32,), maps_per_call=64)
    now = do.worst_basis_error(264, 264, pairs, do.ORDER, maps_per_call=64)
    print("DIRECT_ORDER 264x264 blocks of 32 worst=%.3g at %s, order %s worst=%.3g at %s, bound=%.3g" % (one + (do.ORDER,) + now + (tol,)))
    assert tol / 2 < one[0] <= tol and now[0] <= tol / 2
