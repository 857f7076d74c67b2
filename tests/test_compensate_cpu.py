"""compensate.py on the CPU: the fit, the sweep that collects its moments, and prune_network(...,
carry=True, moments=...) on nets with duplicated, live and dead filters. Nets in float64, CIFAR nets at 32 x 32, 128
calibration samples in 2 batches (compensate_cases.calibration), gaps on a batch the sweep did not see.

Bounds. merge_matrix on planted data: float64 round-off of a well-conditioned 6 x 6 solve, 1e-9 on A and 1e-12 on the
residual. collect_moments against the definition: two float64 summation orders of at most 1.3e5 products, 1e-12
relative to the largest entry. Duplicate-filter nets: compensated gap <= 1e-3 x carry's gap, a separation (measured
ratios are 1e-5 and below: what rtol = 1e-10 cuts off). Live filters: strictly below carry's gap; VGG <= 0.1 x.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import carry_cases as cc
import compensate_cases as k
import pruned_cases as pc
from dct_pruning_amd import compensate as cp
from dct_pruning_amd import nets, prune
from dct_pruning_amd import transplant as tp
from helpers import det_scores, deterministic_init


# ---------------------------------------------------------------------------------------------------------
# merge_matrix
# ---------------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


S9 = [0, 2, 3, 5, 7, 8]   # kept channels of 9; D = [1, 4, 6]


def test_merge_matrix_recovers_planted_combinations():
    n = 200
    X = torch.zeros(9, n, dtype=torch.float64)
    X[S9] = _rand(6, n, seed=1)
    B = _rand(3, 6, seed=2)
    X[[1, 4, 6]] = B @ X[S9]
    A, residual = cp.merge_matrix(X @ X.t(), n, S9)
    print("planted: max|A - B| = %.3g, residual %.3g" % (float((A - B).abs().max()), residual))
    assert A.shape == (3, 6) and A.dtype == torch.float64
    assert float((A - B).abs().max()) <= 1e-9 and 0 <= residual <= 1e-12


def test_merge_matrix_takes_a_singular_kept_block():
    """a dead kept channel and two kept channels that are copies of each other: M_SS has rank 4 of 6"""
    n = 200
    X = torch.zeros(9, n, dtype=torch.float64)
    X[[0, 2, 3, 5]] = _rand(4, n, seed=3)
    X[7] = X[2]          # a copy among the kept; channel 8 stays dead
    B = _rand(3, 4, seed=4)
    X[[1, 4, 6]] = B @ X[[0, 2, 3, 5]]
    G = X @ X.t()
    assert int(torch.linalg.matrix_rank(G[S9][:, S9])) == 4
    A, residual = cp.merge_matrix(G, n, S9)
    assert bool(torch.isfinite(A).all()) and 0 <= residual <= 1e-12
    assert float((A @ X[S9] - X[[1, 4, 6]]).abs().max()) <= 1e-9 * float(X.abs().max())


def test_merge_matrix_never_makes_a_pointwise_consumer_worse():
    """the projection argument: the residual of W_D x_D is its own projection residual"""
    n = 300
    X = torch.relu(_rand(9, n, seed=5))          # nothing planted: the removed channels are not in the span
    W = _rand(5, 9, seed=6)
    A, residual = cp.merge_matrix(X @ X.t(), n, S9)
    D = [1, 4, 6]
    left = float(torch.linalg.norm(W[:, D] @ (X[D] - A @ X[S9])))
    drop = float(torch.linalg.norm(W[:, D] @ X[D]))
    print("random: |W_D (X_D - A X_S)| = %.4g <= |W_D X_D| = %.4g, residual %.3g" % (left, drop, residual))
    assert left <= drop and 0 < residual < 1
    assert abs(residual - float(torch.linalg.norm(X[D] - A @ X[S9]) ** 2 / torch.linalg.norm(X[D]) ** 2)) <= 1e-12


def test_merge_matrix_without_removed_energy_and_with_a_bad_matrix():
    G = torch.zeros(4, 4, dtype=torch.float64)
    G[0, 0] = G[1, 1] = 3.0
    A, residual = cp.merge_matrix(G, 3, [0, 1])  # channels 2 and 3 are dead: nothing to explain
    assert A.shape == (2, 2) and not A.any() and residual == 0.0
    A, residual = cp.merge_matrix(G, 3, [0, 1, 2, 3])
    assert A.shape == (0, 4) and residual == 0.0
    with pytest.raises(ValueError):
        cp.merge_matrix(torch.zeros(4, 3, dtype=torch.float64), 3, [0, 1])


# ---------------------------------------------------------------------------------------------------------
# collect_moments (resnet_56, float64)
# ---------------------------------------------------------------------------------------------------------
NAME = "resnet_56"
WATCHED = ["layer1.0.conv1", "layer2.0.conv1", "layer3.8.conv2", "fc"]   # 32 x 32, 32 x 32 (stride 2 behind it), 8 x 8, [N, 64]


@pytest.fixture(scope="module")
def swept():
    full = deterministic_init(nets.get_network(NAME)).double().eval()
    return full, cp.collect_moments(NAME, full, k.calibration(NAME))


def _no_hooks(net):
    return all(not m._forward_pre_hooks and not m._forward_hooks for m in net.modules())


def test_collect_moments_is_the_definition(swept):
    full, moments = swept
    seen = {m: [] for m in WATCHED}
    handles = [full.get_submodule(m).register_forward_pre_hook(lambda mod, inp, m=m: seen[m].append(inp[0].detach().clone()))
               for m in WATCHED]
    with torch.no_grad():
        for x, _ in k.calibration(NAME):
            full(x.double())
    for h in handles:
        h.remove()
    assert sorted(moments) == sorted(f.module for f in tp.dataflow(NAME) if f.kind in ("conv", "linear") and f.sources)
    for m in WATCHED:
        x = torch.cat(seen[m])
        want = torch.einsum("nchw,ndhw->cd", x, x) if x.dim() == 4 else torch.einsum("nc,nd->cd", x, x)
        n, G = moments[m]
        err = float((G - want).abs().max() / want.abs().max())
        print("%s: n = %d, max|G - einsum| / max|einsum| = %.3g" % (m, n, err))
        assert G.dtype == torch.float64 and G.shape == want.shape and err <= 1e-12
        assert n == x.numel() // x.size(1)


def test_collect_moments_counts_positions(swept):
    _, moments = swept
    samples = k.CALIB_BATCHES * k.CALIB_BATCH
    assert samples >= 128 and k.CALIB_BATCHES >= 2
    assert moments["layer1.0.conv1"].n == samples * 32 * 32 and moments["layer2.0.conv1"].n == samples * 32 * 32
    assert moments["layer2.0.conv2"].n == samples * 16 * 16 and moments["layer3.8.conv2"].n == samples * 8 * 8
    assert moments["fc"].n == samples and moments["fc"].G.shape == (64, 64)


def test_collect_moments_in_forced_runs_equals_one_run(swept):
    """chunk_bytes = 4096: a stage-1 sample alone is 16 * 32 * 32 * 8 bytes, so every conv input goes one sample at a
    time (64 runs per batch), and the classifier's [64, 64] input in 8 runs of 8 samples"""
    full, moments = swept
    forced = cp.collect_moments(NAME, full, k.calibration(NAME), chunk_bytes=4096)
    assert sorted(forced) == sorted(moments)
    worst = max(float((forced[m].G - moments[m].G).abs().max() / moments[m].G.abs().max()) for m in moments)
    print("forced runs against one run: %.3g" % worst)
    assert worst <= 1e-12 and all(forced[m].n == moments[m].n for m in moments)


def test_collect_moments_puts_flags_back_and_removes_hooks():
    full = deterministic_init(nets.get_network(NAME)).double().train()
    full.layer2.eval()
    flags = [m.training for m in full.modules()]
    small = k.calibration(NAME, batches=1, batch=2)
    got = cp.collect_moments(NAME, full, small)
    assert got and [m.training for m in full.modules()] == flags and _no_hooks(full)
    # eval mode during the sweep: no running statistic moved
    assert all(int(m.num_batches_tracked) == 0 for m in full.modules() if isinstance(m, nn.BatchNorm2d))

    def failing():
        yield next(iter(small))
        raise RuntimeError("loader broke")

    with pytest.raises(RuntimeError, match="loader broke"):
        cp.collect_moments(NAME, full, failing())
    assert [m.training for m in full.modules()] == flags and _no_hooks(full)


def test_collect_moments_takes_the_loaders_batch_forms():
    full = deterministic_init(nets.get_network(NAME)).double().eval()
    x = next(iter(k.calibration(NAME, batches=1, batch=2)))[0]
    a = cp.collect_moments(NAME, full, [x])
    b = cp.collect_moments(NAME, full, [(x, None)])
    c = cp.collect_moments(NAME, full, [{"image": x, "label": None}])
    assert all(torch.equal(a[m].G, b[m].G) and torch.equal(a[m].G, c[m].G) for m in a)


def test_collect_moments_hooks_only_what_the_rates_shrink():
    full = deterministic_init(nets.get_network(NAME)).double().eval()
    small = k.calibration(NAME, batches=1, batch=2)
    assert cp.collect_moments(NAME, full, small, [0.0] * nets.RATE_LEN[NAME]) == {}
    # mid widths only: each block's conv2 reads a shrunk conv1, nothing else loses input channels
    got = cp.collect_moments(NAME, full, small, cc.RATES[NAME])
    assert sorted(got) == sorted(conv for conv, _, _, kind in tp.resnet_cifar_convs(56) if kind == "out")
    # every width: every conv behind the stem and the classifier
    got = cp.collect_moments(NAME, full, small, [0.25] * nets.RATE_LEN[NAME])
    assert "layer1.0.conv1" in got and "fc" not in got  # the last stage's outputs keep their width


# ---------------------------------------------------------------------------------------------------------
# duplicate filters: carry loses them, the merge gives them back
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k.DUP_RATES))
def test_duplicate_filters_go_without_a_trace(name):
    """measured (carry's gap, compensated gap), float64, rtol 1e-10: vgg_16_bn 0.999, 4.5e-06; resnet_56 1, 6.5e-14;
    googlenet 0.995, 8.0e-07"""
    full, imp = k.duplicate_net(name)
    full = full.double()
    rates = k.DUP_RATES[name]
    assert k.removed_are_the_copies(name, imp)
    moments = cp.collect_moments(name, full, k.calibration(name), rates)
    x = k.fresh(name).double()
    carry = prune.output_gap(full, prune.prune_network(name, full, imp, rates, carry=True), x)
    pruned = prune.prune_network(name, full, imp, rates, carry=True, moments=moments)
    merged = prune.output_gap(full, pruned, x)
    print("%s duplicates: carry %.3g, compensated %.3g, ratio %.3g" % (name, carry, merged, merged / carry))
    assert pruned.training and next(pruned.parameters()).dtype == torch.float64
    assert carry >= 0.05
    assert merged <= 1e-3 * carry


# ---------------------------------------------------------------------------------------------------------
# live filters
# ---------------------------------------------------------------------------------------------------------
def _live_gaps(name, init):
    full = k.live_net(name, init).double()
    imp, rates = k.live_scores(name), cc.RATES[name]
    moments = cp.collect_moments(name, full, k.calibration(name), rates)
    x = k.fresh(name).double()
    carry = prune.output_gap(full, prune.prune_network(name, full, imp, rates, carry=True), x)
    merged = prune.output_gap(full, prune.prune_network(name, full, imp, rates, carry=True, moments=moments), x)
    print("%s live filters (%s): carry %.3g, compensated %.3g, ratio %.3g" % (name, init, carry, merged, merged / carry))
    return carry, merged


@pytest.mark.filterwarnings("ignore:.*under-determined")   # densenet_40's classifier: 128 samples, 348 kept channels
@pytest.mark.parametrize("name", pc.NETS)
def test_live_filters_compensated_gap_is_below_carrys(name):
    """the constructor's seeded nets (compensate_cases.live_net), random scores, carry_cases.RATES; measured ratios
    compensated / carry: vgg_16_bn 1.2e-3, resnet_56 0.24, resnet_110 0.16, densenet_40 0.022, googlenet 4.5e-4,
    resnet_50 0.22, u2netp 0.74. The small ones are small because these nets' deep maps are close to constant
    (compensate_cases.live_net); the next test has the harder nets"""
    carry, merged = _live_gaps(name, "constructor")
    assert merged < carry
    if name == "vgg_16_bn":
        assert merged <= 0.1 * carry


@pytest.mark.parametrize("name", ["vgg_16_bn", "resnet_56", "resnet_50"])   # the three cheapest sweeps
def test_live_filters_of_nets_with_scaled_activations(name):
    """helpers.deterministic_init's nets, whose activations stay alive through the depth: the maps of random filters
    are far from linear in one another (residuals of 0.2 to 0.3 in VGG's first three layers) and the merge recovers
    less; measured ratios vgg_16_bn 0.23, resnet_56 0.33, resnet_50 0.14. Not 0.1 for VGG here: DESIGN.md §7n."""
    carry, merged = _live_gaps(name, "scaled")
    assert merged < carry


# ---------------------------------------------------------------------------------------------------------
# dead filters: nothing to merge
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:.*under-determined")
@pytest.mark.parametrize("name", pc.NETS)
def test_dead_filters_leave_carrys_state_dict(name):
    full, stems = cc.dead_net(name)
    full = full.double()
    imp, rates = cc.dead_scores(name, stems), cc.RATES[name]
    moments = cp.collect_moments(name, full, k.calibration(name), rates)
    assert moments
    a = prune.prune_network(name, full, imp, rates, carry=True)
    b = prune.prune_network(name, full, imp, rates, carry=True, moments=moments)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and not [key for key in sa if not torch.equal(sa[key], sb[key])]
    merged = cp.compensate(name, a, full, imp, moments)
    assert sorted(m.module for m in merged) == sorted(moments) and all(m.residual == 0.0 and m.removed > 0 for m in merged)
    gap = prune.output_gap(full, b, pc.net_input(name).double())
    print("%s dead filters, compensated: max|pruned - full| / max|full| = %.3g" % (name, gap))
    assert gap <= 1e-9   # test_carry_cpu.TOL


# ---------------------------------------------------------------------------------------------------------
# what compensate writes, errors, warning
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """resnet_56 in float64 with its carry-pruned net's inputs: (full, scores, rates, moments)"""
    full = deterministic_init(nets.get_network(NAME)).double().eval()
    rates = cc.RATES[NAME]
    return full, k.live_scores(NAME), rates, cp.collect_moments(NAME, full, k.calibration(NAME), rates)


def test_compensate_writes_the_formula_and_nothing_else(small):
    full, imp, rates, moments = small
    before = prune.prune_network(NAME, full, imp, rates, carry=True)
    after = prune.prune_network(NAME, full, imp, rates, carry=True)
    merged = cp.compensate(NAME, after, full, imp, moments)
    assert [m.module for m in merged] == [conv for conv, _, _, kind in tp.resnet_cifar_convs(56) if kind == "out"]
    sa, sb = before.state_dict(), after.state_dict()
    changed = sorted(key for key in sa if not torch.equal(sa[key], sb[key]))
    assert changed == sorted(m.module + ".weight" for m in merged)   # no bias, no batch-norm tensor, no other conv
    rec = merged[0]
    S = tp.select_index(imp["imp_conv2"], 16, 12)
    D = np.setdiff1d(np.arange(16), S)
    assert (rec.module, rec.n, rec.kept, rec.removed) == ("layer1.0.conv2", 128 * 32 * 32, 12, 4)
    A, residual = cp.merge_matrix(moments[rec.module].G, rec.n, S)
    W = full.state_dict()["layer1.0.conv2.weight"]
    want = W[:, S] + torch.einsum("odhw,ds->oshw", W[:, D], A)
    assert torch.equal(sb["layer1.0.conv2.weight"], want) and rec.residual == residual and 0 < residual < 1


def test_compensate_errors_and_warning(small):
    full, imp, rates, moments = small
    pruned = prune.prune_network(NAME, full, imp, rates, carry=True)
    with pytest.raises(KeyError, match="layer2.3.conv2"):
        cp.compensate(NAME, pruned, full, imp, {m: v for m, v in moments.items() if m != "layer2.3.conv2"})
    with pytest.raises(KeyError, match="layer2.3.conv2"):
        prune.prune_network(NAME, full, imp, rates, carry=True, moments={m: v for m, v in moments.items() if m != "layer2.3.conv2"})
    bad = dict(moments)
    bad["layer1.0.conv2"] = cp.Moments(moments["layer1.0.conv2"].n, moments["layer1.0.conv2"].G[:12, :12])
    with pytest.raises(ValueError, match="layer1.0.conv2"):
        cp.compensate(NAME, pruned, full, imp, bad)
    few = dict(moments)
    few["layer3.1.conv2"] = cp.Moments(47, moments["layer3.1.conv2"].G)   # 48 channels kept of 64
    with pytest.warns(UserWarning, match="layer3.1.conv2"):
        cp.compensate(NAME, pruned, full, imp, few)
    with pytest.raises(ValueError, match="carry"):
        prune.prune_network(NAME, full, imp, rates, moments=moments)
    with pytest.raises(ValueError, match="carry"):
        prune.prune_network(NAME, full, imp, rates, exact=True, moments=moments)


def test_without_moments_nothing_changed(small):
    full, imp, rates, _ = small
    a = prune.prune_network(NAME, full, imp, rates, carry=True).state_dict()
    b = tp.transplant_carry(NAME, nets.get_network(NAME, rates).double().state_dict(), full.state_dict(), imp)
    assert list(a) == list(b) and not [key for key in a if not torch.equal(a[key], b[key])]
    kept = tp.kept_filters(NAME, a, full.state_dict(), imp)
    assert np.array_equal(kept["layer1.0.conv1"], tp.select_index(imp["imp_conv2"], 16, 12)) and len(kept["conv1"]) == 16


# ---------------------------------------------------------------------------------------------------------
# command-line tool
# ---------------------------------------------------------------------------------------------------------
DSL = "[0.]*3+[0.25]*27"


@pytest.fixture()
def score_dir(tmp_path):
    d = tmp_path / "scores"
    d.mkdir()
    for stem, c in pc.transplant_fixture(NAME)["stems"]:
        np.save(str(d / (stem + ".npy")), det_scores(stem, c))
    return d


def _argv(score_dir, out):
    return ["--net", NAME, "--imp_score", str(score_dir), "--compress_rate", DSL, "--seed", "3", "--out", str(out)]


def test_cli_compensate_prints_a_fourth_line_and_records_it(score_dir, tmp_path, capsys):
    out = tmp_path / "pruned.pt"
    assert prune.main(_argv(score_dir, out) + ["--carry", "--compensate", "--synthetic", "--calib_batches", "2", "--batch_size", "64"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and [l.split()[0] for l in lines] == ["full", "pruned", "gap", "merged"]
    saved = torch.load(str(out), weights_only=True)
    assert saved["compensate"] is True and saved["carry"] is True
    slim = nets.get_network(NAME, saved["compress_rate"])
    slim.load_state_dict(saved["state_dict"], strict=True)
    # the fourth line holds the gap of exactly this net on the third line's batch, and it is the smaller one
    from dct_pruning_amd.data import SyntheticLoader
    torch.manual_seed(3)
    full = nets.get_network(NAME)
    x = next(iter(SyntheticLoader((3, 32, 32), 2, 1, seed=3)))[0]
    merged = prune.output_gap(full, slim, x)
    assert lines[3].split("max|full| ")[1].split()[0] == "%.3g" % merged
    assert merged < float(lines[2].split("max|full| ")[1].split()[0])
    assert "largest residual" in lines[3] and "27 modules" in lines[3]
    # the same net from the library; the tool seeds its calibration batches with --seed + 1
    moments = cp.collect_moments(NAME, full, SyntheticLoader((3, 32, 32), 64, 2, seed=4), saved["compress_rate"])
    lib = prune.prune_network(NAME, full, str(score_dir), saved["compress_rate"], carry=True, moments=moments).state_dict()
    assert not [key for key in lib if not torch.equal(lib[key], saved["state_dict"][key])]


def test_cli_carry_alone_is_as_before(score_dir, tmp_path, capsys):
    out = tmp_path / "pruned.pt"
    assert prune.main(_argv(score_dir, out) + ["--carry"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and lines[2].startswith("gap")
    saved = torch.load(str(out), weights_only=True)
    assert saved["compensate"] is False and saved["carry"] is True
    torch.manual_seed(3)
    full = nets.get_network(NAME)
    want = prune.prune_network(NAME, full, str(score_dir), saved["compress_rate"], carry=True).state_dict()
    assert not [key for key in want if not torch.equal(want[key], saved["state_dict"][key])]


def test_cli_compensate_without_carry_exits_in_the_parser(score_dir, tmp_path, capsys):
    out = tmp_path / "pruned.pt"
    with pytest.raises(SystemExit) as exc:
        prune.main(_argv(score_dir, out) + ["--compensate", "--synthetic"])
    assert exc.value.code == 2 and "--carry" in capsys.readouterr().err and not out.exists()
