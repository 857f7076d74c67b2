"""prune_network(..., carry=True) on the CPU: a pruned net that computes what the full net computes
once only dead filters go, for all seven architectures, and what the mode promises about every tensor.

Bound of the equivalence: 1e-9 * max|full output| in float64, the bound tests/test_pruned_nets_cpu.py holds the same
statement to for ResNet-50 (float64 round-off over the at most 1e5 accumulations behind an output is about 1e-11; a
wrong column or a batch-norm that did not follow its channel moves outputs by percent). Measured: see each test's print.
"""
import numpy as np
import pytest
import torch

import carry_cases as cc
import pruned_cases as pc
from dct_pruning_amd import nets, prune
from dct_pruning_amd import transplant as tp
from helpers import det_scores, det_tensor, deterministic_init

TOL = 1e-9


def _fixture_inputs(net):
    fx = pc.transplant_fixture(net)
    ori = {k: det_tensor(k, s, "") for k, s in fx["ori"]}
    imp = {stem: det_scores(stem, c) for stem, c in fx["stems"]}
    slim = {k: det_tensor(k, s, "slim:") for k, s in fx["slim"]}
    return fx, ori, imp, slim


# ---------------------------------------------------------------------------------------------------------
# dead filters go without a trace
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=pc.NETS)
def dead(request):
    name = request.param
    full, stems = cc.dead_net(name)
    return name, full.double(), cc.dead_scores(name, stems), stems


def test_carry_removes_dead_filters_without_a_trace(dead):
    """measured max|pruned - full| / max|full|, float64: vgg_16_bn 4.7e-16, resnet_56 0, resnet_110 0,
    densenet_40 3.2e-16, googlenet 5.0e-16, resnet_50 8.8e-16, u2netp 0"""
    name, full, imp, stems = dead
    assert cc.removed_not_dead(imp, name, cc.RATES[name], stems) == []
    assert cc.shrunk(name, cc.RATES[name])
    torch.manual_seed(1)
    pruned = prune.prune_network(name, full, imp, cc.RATES[name], carry=True)
    assert pruned.training and next(pruned.parameters()).dtype == torch.float64
    gap = prune.output_gap(full, pruned, pc.net_input(name).double())
    print("%s carry: max|pruned - full| / max|full| = %.3g" % (name, gap))
    assert gap <= TOL
    assert pruned.training and not full.training  # output_gap puts the flags back


def test_default_mode_misses_on_the_same_inputs(dead):
    """the reference's loaders on the same nets, scores and rates: measured gaps vgg_16_bn 0.98, resnet_56 0.92,
    resnet_110 0.98, densenet_40 1.07, googlenet 0.91 (resnet_50 8.8e-16: its loader carries the batch-norms);
    u2netp's control flow raises where only inner widths are pruned (int('i') at the first decoder stage's un-pruned
    rebnconvin behind a pruned unit, utils/load_models.py:658)"""
    name, full, imp, _ = dead
    torch.manual_seed(1)
    if name == "u2netp":
        with pytest.raises(ValueError, match="invalid literal for int"):
            prune.prune_network(name, full, imp, cc.RATES[name])
        return
    pruned = prune.prune_network(name, full, imp, cc.RATES[name])
    gap = prune.output_gap(full, pruned, pc.net_input(name).double())
    print("%s default: max|pruned - full| / max|full| = %.3g" % (name, gap))
    if name == "resnet_50":
        assert gap <= TOL
    else:
        assert gap > 0.01


@pytest.mark.parametrize("name", ["vgg_16_bn", "densenet_40", "googlenet", "resnet_56", "u2netp"])
def test_score_prune_run_with_the_oracle_as_energy_operator(name, tmp_path, monkeypatch):
    """the path of tests/test_carry_gpu.py without a GPU: imp_score's files (energy by the float64 oracle) give the
    masks, and they remove dead filters only on the batches of carry_cases.SEED"""
    import copy
    import os
    from dct_pruning_amd import harness
    from oracle import dct_oracle as orc
    monkeypatch.setattr(harness, "_energy_nc", orc.energy_nc_batched)
    _, x = cc.batches(name)
    full, stems = cc.dead_net(name, calibrate_on=x)
    score_dir = cc.score(name, full, tmp_path)
    load = lambda stem: np.load(os.path.join(score_dir, stem + ".npy"))
    for stem in stems:
        s = load(stem)
        dead = np.arange(s.size) % cc.MOD == 0
        assert np.all(s[dead] == 0) and not np.signbit(s[dead]).any() and np.all(s[~dead] > 0), stem
    assert cc.removed_not_dead(load, name, cc.RATES[name], stems) == []
    full = copy.deepcopy(full).double()
    gap = prune.output_gap(full, prune.prune_network(name, full, score_dir, cc.RATES[name], carry=True), x.double())
    print("%s from score files: max|pruned - full| / max|full| = %.3g" % (name, gap))
    assert gap <= TOL


def test_output_gap_is_the_definition():
    full = deterministic_init(nets.get_network("u2netp")).double()
    other = deterministic_init(nets.get_network("u2netp")).double().eval()
    with torch.no_grad():
        other.side3.bias += 0.5
    x = pc.net_input("u2netp").double()
    assert prune.output_gap(full, full, x) == 0.0
    got = prune.output_gap(full, other, x)
    assert full.training and not other.training
    a, b = pc.outputs_of(full.eval(), x), pc.outputs_of(other, x)
    want = max(float((q - p).abs().max()) for p, q in zip(a, b)) / max(float(p.abs().max()) for p in a)
    assert isinstance(got, float) and got == want and got > 0


# ---------------------------------------------------------------------------------------------------------
# what the mode promises about every tensor
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", pc.NETS)
def test_zero_rates_give_the_full_net_tensor_for_tensor(net):
    full = deterministic_init(nets.get_network(net))
    got = prune.prune_network(net, full, {}, [0.0] * nets.RATE_LEN[net], carry=True)  # {}: no score file is read
    a, b = got.state_dict(), full.state_dict()
    assert list(a) == list(b) and not [k for k in a if not torch.equal(a[k], b[k])]


def test_zero_rates_raise_for_u2netp_in_the_default_mode():
    full = deterministic_init(nets.get_network("u2netp"))
    with pytest.raises(TypeError):  # list(None) where stage 2 starts with no live index (utils/load_models.py:621)
        prune.prune_network("u2netp", full, {}, [0.0] * 39)


@pytest.mark.parametrize("net", pc.NETS)
def test_result_does_not_depend_on_the_seed_and_loads_strictly(net):
    fx, ori, imp, _ = _fixture_inputs(net)
    torch.manual_seed(1)
    a = prune.prune_network(net, ori, imp, fx["rates"], carry=True).state_dict()
    torch.manual_seed(2)
    b = prune.prune_network(net, ori, imp, fx["rates"], carry=True).state_dict()
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    assert pc.key_shapes(a) == fx["slim"]  # the reference constructor's keys, order and shapes
    # no tensor keeps an initialisation: every value is one the full net holds
    # (per-channel tensors, whose initialisation is the same constant under every seed)
    for k, t in a.items():
        if t.dim() == 1:
            assert np.isin(t.numpy(), ori[k].numpy()).all(), k


@pytest.mark.parametrize("net,case", [(n, c) for n in pc.NETS for c in ("readme", "extra")])
def test_both_rate_lists_build_the_constructors_net(net, case):
    fx, ori, imp, _ = _fixture_inputs(net)
    rates = pc.forward_fixture(net)[case]["rates"]
    got = prune.prune_network(net, ori, imp, rates, carry=True)
    assert pc.key_shapes(got.state_dict()) == pc.key_shapes(nets.get_network(net, rates).state_dict())
    nets.get_network(net, rates).load_state_dict(got.state_dict(), strict=True)


def test_carry_and_exact_exclude_each_other():
    fx, ori, imp, _ = _fixture_inputs("resnet_50")
    with pytest.raises(ValueError, match="carry"):
        prune.prune_network("resnet_50", ori, imp, fx["rates"], exact=True, carry=True)


def test_bad_scores_raise_as_in_the_default_mode():
    fx, ori, imp, _ = _fixture_inputs("resnet_56")
    with pytest.raises(ValueError, match="imp_conv2"):
        prune.prune_network("resnet_56", ori, dict(imp, imp_conv2=imp["imp_conv2"][:-1]), fx["rates"], carry=True)
    with pytest.raises(KeyError):
        prune.prune_network("resnet_56", ori, {k: v for k, v in imp.items() if k != "imp_conv2"}, fx["rates"], carry=True)
    # the stem keeps its width at these rates: its file is not read
    prune.prune_network("resnet_56", ori, {k: v for k, v in imp.items() if k != "imp_conv1"}, fx["rates"], carry=True)


# ---------------------------------------------------------------------------------------------------------
# the two modes where the reference's loader is already right (README rates)
# ---------------------------------------------------------------------------------------------------------
def _both(net):
    fx, ori, imp, slim = _fixture_inputs(net)
    return prune.LOADERS[net](dict(slim), ori, imp), tp.transplant_carry(net, dict(slim), ori, imp)


def _conv_weights(sd):
    return [k for k, t in sd.items() if t.dim() == 4]


def test_resnet_50_agrees_with_todays_default_in_every_tensor():
    fx, ori, imp, slim = _fixture_inputs("resnet_50")
    ref = tp.transplant_resnet_50(dict(slim), ori, imp, downsample_input="block")
    got = tp.transplant_carry("resnet_50", dict(slim), ori, imp)
    assert list(got) == list(ref) and not [k for k in ref if not torch.equal(ref[k], got[k])]


@pytest.mark.parametrize("net", ["vgg_16_bn", "resnet_56", "resnet_110"])
def test_conv_weights_agree_with_the_reference_loader(net):
    ref, got = _both(net)
    assert len(_conv_weights(ref)) > 10 and not [k for k in _conv_weights(ref) if not torch.equal(ref[k], got[k])]


def test_densenet_conv_weights_agree_except_conv1():
    """conv1: the reference's `last_select_index` starts as an empty list, so its first conv copies nothing and keeps the
    slim net's own weights (transplant.py's docstring, DenseNet-40); carry brings the full net's conv1 over"""
    ref, got = _both("densenet_40")
    assert [k for k in _conv_weights(ref) if not torch.equal(ref[k], got[k])] == ["conv1.weight"]
    assert torch.equal(got["conv1.weight"], det_tensor("conv1.weight", got["conv1.weight"].shape, ""))


@pytest.mark.parametrize("case", ["readme", "extra"])
def test_googlenet_entry_convs_read_torch_cat_order(case):
    """written from GOOGLENET_FILTERS and nets.py's torch.cat([1x1, 3x3, 5x5, pool]), not from the table: the entry convs
    of block k + 1 hold the original's columns [1x1 whole | kept 3x3 + n1 | kept last-5x5 + n1 + n3 | pool whole + n1 + n3 + n5]"""
    fx, ori, imp, _ = _fixture_inputs("googlenet")
    rates = pc.forward_fixture("googlenet")[case]["rates"]
    got = prune.prune_network("googlenet", ori, imp, rates, carry=True).state_dict()
    widths = tp.googlenet_widths(rates)
    blocks = tp.GOOGLENET_BLOCKS
    differs = 0
    for b in range(len(blocks) - 1):
        n1, n3, n5, npool = tp.GOOGLENET_FILTERS[b]
        _, w3, _, w5, _ = widths[b]
        k3 = tp.select_index(imp["imp_conv%d_n3x3" % (b + 2)], n3, w3) if w3 != n3 else np.arange(n3)
        k5 = tp.select_index(imp["imp_conv%d_n5x5" % (b + 2)], n5, w5) if w5 != n5 else np.arange(n5)
        cols = np.concatenate([np.arange(n1), k3 + n1, k5 + n1 + n3, np.arange(npool) + n1 + n3 + n5])
        loader_order = np.concatenate([np.arange(n1), np.arange(npool) + n1 + n3 + n5, k3 + n1, k5 + n1 + n3])
        differs += not np.array_equal(cols, loader_order)
        for entry in ("branch1x1.0", "branch3x3.0", "branch5x5.0", "branch_pool.1"):
            key = "%s.%s.weight" % (blocks[b + 1], entry)
            assert torch.equal(got[key], ori[key][:, torch.as_tensor(cols)]), key
    assert differs  # the reference assembles [1x1, pool, 3x3, 5x5]: other columns
    # the first block reads pre_layers, which never shrinks; the classifier reads the last block, which keeps its outputs
    assert torch.equal(got["inception_a3.branch1x1.0.weight"], ori["inception_a3.branch1x1.0.weight"])
    assert torch.equal(got["linear.weight"], ori["linear.weight"])


def test_densenet_classifier_and_final_bn_take_the_kept_concatenation():
    fx, ori, imp, _ = _fixture_inputs("densenet_40")
    got = prune.prune_network("densenet_40", ori, imp, fx["rates"], carry=True).state_dict()
    kept = {stem: (tp.select_index(imp[stem], o, c) if o != c else np.arange(o)) for stem, o, c in tp.densenet_40_kept(fx["rates"])}
    cols = np.concatenate([kept["imp_conv27"]] + [kept["imp_conv%d" % (28 + j)] + 312 + 12 * j for j in range(12)])
    idx = torch.as_tensor(cols)
    assert torch.equal(got["fc.weight"], ori["fc.weight"][:, idx]) and torch.equal(got["fc.bias"], ori["fc.bias"])
    for part in ("weight", "bias", "running_mean", "running_var"):
        assert torch.equal(got["bn." + part], ori["bn." + part][idx])


# ---------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", pc.NETS)
def test_dataflow_lists_every_parameterised_module_in_order(net):
    table = tp.dataflow(net)
    model = nets.get_network(net)
    want = [n for n, m in model.named_modules() if list(m.parameters(recurse=False))]
    assert [f.module for f in table] == want
    producers = {f.module: f for f in table if f.kind == "conv"}
    for f in table:
        m = model.get_submodule(f.module)
        assert f.kind == {"Conv2d": "conv", "Linear": "linear"}.get(type(m).__name__, "bn")
        read = sum(producers[p].width for p, _ in f.sources)
        if f.kind == "conv":
            assert f.width == m.out_channels and (not f.sources or read == m.in_channels)
        elif f.kind == "bn":
            assert f.width == m.num_features and (not f.sources or read == f.width)
        else:
            assert not f.sources or read == m.in_features
        # offsets: each part starts where the parts before it end in the original tensor
        off = 0
        for p, o in f.sources:
            assert o == off, (f.module, p)
            off += producers[p].width
    with pytest.raises(ValueError):
        tp.dataflow("alexnet")


# ---------------------------------------------------------------------------------------------------------
# command-line tool
# ---------------------------------------------------------------------------------------------------------
DSL = "[0.]+[0.18]*29"


@pytest.fixture()
def score_dir(tmp_path):
    d = tmp_path / "scores"
    d.mkdir()
    for stem, c in pc.transplant_fixture("resnet_56")["stems"]:
        np.save(str(d / (stem + ".npy")), det_scores(stem, c))
    return d


def test_cli_carry_writes_a_net_that_loads_back(score_dir, tmp_path, capsys):
    out = tmp_path / "pruned.pt"
    argv = ["--net", "resnet_56", "--imp_score", str(score_dir), "--compress_rate", DSL, "--seed", "3", "--out", str(out)]
    assert prune.main(argv + ["--carry"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and lines[0].startswith("full ") and lines[1].startswith("pruned") and lines[2].startswith("gap")
    saved = torch.load(str(out), weights_only=True)
    assert saved["carry"] is True and saved["net"] == "resnet_56" and saved["compress_rate"] == [0.0] + [0.18] * 29
    slim = nets.get_network("resnet_56", saved["compress_rate"])
    slim.load_state_dict(saved["state_dict"], strict=True)
    # the third line holds the gap of exactly this net, on the synthetic batch the seed names
    from dct_pruning_amd.data import SyntheticLoader
    torch.manual_seed(3)
    full = nets.get_network("resnet_56")
    x = next(iter(SyntheticLoader((3, 32, 32), 2, 1, seed=3)))[0]
    assert lines[2].split("max|full| ")[1].split()[0] == "%.3g" % prune.output_gap(full, slim, x)
    sd = full.state_dict()
    kept = torch.as_tensor(tp.select_index(np.load(str(score_dir / "imp_conv2.npy")), 16, 13))
    assert torch.equal(saved["state_dict"]["layer1.0.conv1.weight"], sd["layer1.0.conv1.weight"][kept])
    # without --carry: two lines, and the dict says so
    assert prune.main(argv) == 0
    assert len(capsys.readouterr().out.splitlines()) == 2 and torch.load(str(out), weights_only=True)["carry"] is False


def test_cli_carry_with_exact_exits_2_and_writes_nothing(score_dir, tmp_path, capsys):
    out = tmp_path / "pruned.pt"
    with pytest.raises(SystemExit) as exc:
        prune.main(["--net", "resnet_56", "--imp_score", str(score_dir), "--compress_rate", DSL, "--out", str(out), "--carry",
                    "--exact"])
    assert exc.value.code == 2 and "--exact" in capsys.readouterr().err and not out.exists()
