"""tests/reduce_oracle.py without a GPU: the fp32 model of the batch sum is a valid sum, a bitwise comparison with it
catches every order, loop-boundary and rounding mutant, the update rule has the bits of the reference's own torch CPU ops
where the sum is exact, and the descriptor the multi-point entry takes is laid out as the header says."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import reduce_oracle as ro
from dct_pruning_amd import _lib
from dct_pruning_amd.accumulate import HostAccumulator

C_SUM, C_MEAN, SEED = 2049, 4096, 5


def _share(a, b):
    return float(np.mean(ro.bits(a) != ro.bits(b)))


def test_model_is_an_accurate_sum():
    """Any order of fp32 additions of N non-negative terms is within (N - 1) 2^-24 relative of the exact sum."""
    for N in ro.NS:
        e = ro.energies(N, 257, SEED + N)
        ref = e.astype(np.float64).sum(0)
        got = ro.batch_sum_model(e)
        assert got.dtype == np.float32
        rel = np.abs(got.astype(np.float64) - ref) / ref
        assert rel.max() <= (N - 1) * 2.0 ** -24, (N, rel.max())


def test_model_edges():
    z = np.zeros((5, 3), np.float32)
    assert (ro.bits(ro.batch_sum_model(z)) == 0).all()
    assert (ro.bits(ro.batch_sum_model(-z)) == 0).all()  # +0.0 + -0.0 = +0.0: the empty slices clear the sign
    e = ro.energies(40, 4, 1)
    e[7, 1], e[9, 2] = np.nan, np.inf
    t, clean = ro.batch_sum_model(e), ro.batch_sum_model(ro.energies(40, 4, 1))
    assert np.isnan(t[1]) and t[2] == np.inf and (ro.bits(t)[[0, 3]] == ro.bits(clean)[[0, 3]]).all()


@pytest.mark.parametrize("name", sorted(ro.SUM_MUTANTS))
def test_sum_mutants_are_caught(name):
    mutant, worst = ro.SUM_MUTANTS[name], 1.0
    for N in ro.NS:
        e = ro.energies(N, C_SUM, SEED)
        share = _share(mutant(e), ro.batch_sum_model(e))
        if N <= 16:
            # no slice holds two samples and +0.0 + x = x, so these two orders ARE the model: sample counts up to 16
            # cannot tell them apart, which is why the GPU cases go beyond 16
            if name in ro.EQUAL_UP_TO_16:
                assert share == 0.0, (name, N)
            continue
        if name == "256-doubled" and N <= 256:
            assert share == 0.0, (name, N)  # there is no sample 256
            continue
        worst = min(worst, share)
        assert share >= 0.25, (name, N, share)
    print("SUM MUTANT %-20s differs in at least %.1f %% of %d columns" % (name, 100 * worst, C_SUM))


@pytest.mark.parametrize("name", sorted(ro.MEAN_MUTANTS))
def test_mean_mutants_are_caught(name):
    # neither total + N a power of two nor total 0: the division by a power of two and the product with 0 are exact
    for total, N in [(5, 256), (261, 3)]:
        e = ro.energies(N, C_MEAN, SEED)
        fr = ro.feature_result(C_MEAN, SEED + 1, total, N)
        share = _share(ro.MEAN_MUTANTS[name](fr, total, e), ro.running_mean_model(fr, total, e))
        print("MEAN MUTANT %-16s total %d N %d: differs in %.1f %% of %d columns" % (name, total, N, 100 * share, C_MEAN))
        assert share >= 0.05, (name, total, N, share)


def test_integer_energies_have_the_bits_of_the_reference_ops():
    """Integer energies up to 1000 and N <= 1000: every partial sum is an integer below 2^24, exact in any order, so the
    model and torch's sum(0) agree on the sum and the three roundings of the update are all that is compared."""
    rng = np.random.default_rng(SEED)
    batches = [rng.integers(0, 1001, size=(n, 37)).astype(np.float32) for n in (5, 1000, 3)]
    host = HostAccumulator()
    for e in batches:
        host.update(torch.from_numpy(e))
    got = ro.chain_model(batches, 37)
    assert host.total.item() == 1008
    assert host.scores().dtype == np.float32 and (ro.bits(got) == ro.bits(host.scores())).all()
    assert len(np.unique(got)) > 30 and not (got == np.round(got)).all()  # the roundings did happen


def test_rule_f64_is_the_rule():
    batches = [ro.energies(n, 9, 40 + n) for n in (5, 256, 3)]
    allrows = np.concatenate(batches).astype(np.float64)
    np.testing.assert_allclose(ro.rule_f64(batches), allrows.mean(0), rtol=1e-13)
    np.testing.assert_allclose(ro.chain_model(batches, 9), ro.rule_f64(batches), rtol=2 * (256 + 9) * 2.0 ** -24)


def test_update_desc_layout(repo_root):
    """_lib.UpdateDesc against struct dcts_update_desc of include/dctscore.h: 40 bytes, fields in the header's order."""
    text = open(os.path.join(repo_root, "include", "dctscore.h")).read()
    body = re.search(r"typedef struct dcts_update_desc \{(.*?)\} dcts_update_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [re.match(r"\s*(.*?)\s*(\w+)$", d).groups() for d in body.split(";") if d.strip()]
    size = {"const float*": 8, "float*": 8, "int64_t": 8, "float": 4, "int32_t": 4}
    off, want = 0, []
    for ctype, name in decl:
        off = (off + size[ctype] - 1) // size[ctype] * size[ctype]
        want.append((name, off, size[ctype]))
        off += size[ctype]
    have = [(n, getattr(_lib.UpdateDesc, n).offset, getattr(_lib.UpdateDesc, n).size) for n, _ in _lib.UpdateDesc._fields_]
    assert have == want
    assert have == [("energy_nc", 0, 8), ("feature_result", 8, 8), ("N", 16, 8), ("C_count", 24, 8), ("total_before", 32, 4),
                    ("reserved", 36, 4)]
    assert ctypes.sizeof(_lib.UpdateDesc) == 40 and ctypes.sizeof(_lib.UpdateDesc * 3) == 120
