"""collect_moments and prune_network(..., carry=True, moments=...) on the GPU: the duplicate-filter nets of
compensate_cases.py in fp32 on the device, 128 calibration samples in 2 batches.

Bound: compensated gap <= 1e-3 x carry's gap on the same device, the separation tests/test_compensate_cpu.py holds in
float64; the moments of forced runs against one run to 1e-12 of the largest entry (two float64 summation orders). The
compensated net's fp32 error against the full net in float64 on the CPU is printed next to the full net's own, with no
bound: the fit is float64 from fp32 maps, and what its conditioning leaves in fp32 had not been measured before."""
import copy
import types

import pytest
import torch

import carry_cases as cc
import compensate_cases as k
import pruned_cases as pc
from dct_pruning_amd import compensate as cp
from dct_pruning_amd import prune

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", params=["vgg_16_bn", "resnet_56"])
def case(request):
    name = request.param
    full, imp = k.duplicate_net(name)
    x = k.fresh(name)
    want = pc.outputs_of(copy.deepcopy(full).double(), x.double())
    full = full.to(DEV)
    moments = cp.collect_moments(name, full, k.calibration(name), k.DUP_RATES[name])
    return types.SimpleNamespace(name=name, full=full, imp=imp, rates=k.DUP_RATES[name], x=x, want=want, moments=moments)


def test_moments_are_float64_on_the_device(case):
    assert len(case.moments) == len(k.duplicated(case.name))   # one consumer behind each conv that shrinks
    for module, (n, G) in case.moments.items():
        assert G.is_cuda and G.dtype == torch.float64 and G.dim() == 2 and G.size(0) == G.size(1), module
        assert n >= k.CALIB_BATCHES * k.CALIB_BATCH and bool(torch.isfinite(G).all()) and float(G.diagonal().min()) >= 0, module


def test_forced_runs_equal_one_run_on_the_device(case):
    """On the inputs of the forced sweep itself, kept by pre-hooks of the test's own: two fp32 forward passes of the VGG
    are not bit-identical on the device (its 2 x 2 maps differ by 5e-7 of their size between calls), which moves the
    moments of a second sweep by 4e-8 and says nothing about the runs."""
    seen = {m: [] for m in case.moments}
    handles = [case.full.get_submodule(m).register_forward_pre_hook(lambda mod, inp, m=m: seen[m].append(inp[0].detach().clone()))
               for m in seen]
    try:
        forced = cp.collect_moments(case.name, case.full, k.calibration(case.name), case.rates, chunk_bytes=4096)  # one sample a run
    finally:
        for h in handles:
            h.remove()
    assert sorted(forced) == sorted(case.moments)
    worst = 0.0
    for m, (n, G) in forced.items():
        x = torch.cat(seen[m])
        rows = x.transpose(0, 1).reshape(x.size(1), -1).double()
        one = rows @ rows.t()
        worst = max(worst, float((G - one).abs().max() / one.abs().max()))
        assert n == case.moments[m].n == rows.size(1), m
    print("%s: forced runs against one run %.3g" % (case.name, worst))
    assert worst <= 1e-12


def test_duplicate_filters_go_without_a_trace_on_the_device(case):
    """measured on one MI355X, fp32: see DESIGN.md §7n"""
    assert k.removed_are_the_copies(case.name, case.imp)
    x = case.x.to(DEV)
    carry = prune.output_gap(case.full, prune.prune_network(case.name, case.full, case.imp, case.rates, carry=True), x)
    pruned = prune.prune_network(case.name, case.full, case.imp, case.rates, carry=True, moments=case.moments).eval()
    assert all(t.is_cuda for t in pruned.state_dict().values()) and next(pruned.parameters()).dtype == torch.float32
    merged = prune.output_gap(case.full, pruned, x)
    e = cc.error_against(pc.outputs_of(pruned, x), case.want)
    e_full = cc.error_against(pc.outputs_of(case.full.eval(), x), case.want)
    print("%s duplicates: carry %.3g, compensated %.3g, ratio %.3g; against the full net in float64 on the cpu: "
          "compensated %.3g, full %.3g" % (case.name, carry, merged, merged / carry, e, e_full))
    assert carry >= 0.05
    assert merged <= 1e-3 * carry
