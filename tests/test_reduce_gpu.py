"""k_batch_sum, k_running_mean and k_running_mean_multi (reduce.hip) against the exact fp32 model of tests/reduce_oracle.py.

The header fixes the summation order (16 interleaved slices, combined in slice order) and the update's three roundings, so
every comparison here is on bits (int32 views), against the model and against the kernels' own twin calls; the one bounded
comparison is that of host and device accumulation with the rule in float64. Sample counts sit around the slice count and
the 64- and 256-sample loop tiers of strip_batch_sum, channel counts around the 32-channel strip; tests/test_reduce_cpu.py
shows that the comparison catches each order, loop-boundary and rounding mutant at these sizes. Outputs and feature_result
buffers are cut from NaN-filled arenas with 64 guard floats around each, which must stay NaN."""
import functools
import random

import numpy as np
import pytest
import torch

import reduce_oracle as ro
from dct_pruning_amd import _lib, ops
from dct_pruning_amd.accumulate import DeviceAccumulator, DeviceBatchAccumulator, HostAccumulator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
CMAX = max(ro.CS)


class Arena:
    """Float buffers of the given sizes cut from one NaN-filled allocation, GUARD floats before, between and after them."""

    def __init__(self, sizes):
        self.spans, at = [], GUARD
        for s in sizes:
            self.spans.append((at, s))
            at += s + GUARD
        self.buf = torch.full((at,), float("nan"), dtype=torch.float32, device=DEV)
        self.guard = torch.ones(at, dtype=torch.bool, device=DEV)
        for o, s in self.spans:
            self.guard[o:o + s] = False

    def __getitem__(self, i):
        o, s = self.spans[i]
        return self.buf[o:o + s]

    def fill(self, i, values):
        self[i].copy_(torch.from_numpy(np.ascontiguousarray(values)))
        return self[i]

    def guards_intact(self):
        return bool(torch.isnan(self.buf[self.guard]).all())


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(got, want):
    """got: device or host float32 tensor; want: numpy float32 or tensor. Equal as int32."""
    want = ro.bits(want) if isinstance(want, np.ndarray) else _bits(want)
    return np.array_equal(_bits(got), want)


def _sum_into(e, out):
    _lib.check(_lib.load().dcts_batch_sum_f32(e.data_ptr(), e.shape[0], e.shape[1], out.data_ptr(), _stream()))


def _update(e, fr, total):
    _lib.check(_lib.load().dcts_running_mean_update_f32(e.data_ptr(), e.shape[0], e.shape[1], fr.data_ptr(), float(total), _stream()))


@functools.lru_cache(maxsize=None)
def _wide_case(N):
    """[N, CMAX] energies and their model sum, computed once per N and left unchanged (76 MB over all N): columns are
    independent, so the first C columns are the case (N, C)."""
    e = ro.energies(N, CMAX, 1000 + N)
    e.setflags(write=False)
    return e, ro.batch_sum_model(e)


def _case(N, C):
    e, t = _wide_case(N)
    return e[:, :C].copy(), t[:C]


# ---- dcts_batch_sum_f32 / ops.batch_sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ro.NS)
def test_batch_sum_has_the_models_bits(N):
    """dcts_batch_sum_f32 on [N, C] for every C of the list against batch_sum_model, a second call into another buffer
    against the first, and ops.batch_sum against both."""
    first, again = Arena(ro.CS), Arena(ro.CS)
    for i, C in enumerate(ro.CS):
        e_np, want = _case(N, C)
        e = torch.from_numpy(e_np).to(DEV)
        _sum_into(e, first[i])
        _sum_into(e, again[i])
        assert _same_bits(first[i], want), (N, C)
        assert _same_bits(again[i], first[i]), (N, C)
        assert _same_bits(ops.batch_sum(e), want), (N, C)
    assert first.guards_intact() and again.guards_intact()


def test_batch_sum_many_strips():
    N, C = ro.WIDE
    e_np = ro.energies(N, C, 7)
    out = Arena([C])
    _sum_into(torch.from_numpy(e_np).to(DEV), out[0])
    assert _same_bits(out[0], ro.batch_sum_model(e_np))
    assert out.guards_intact()


@pytest.mark.parametrize("N", [5, 16, 17, 321])
def test_batch_sum_zero_columns_give_plus_zero(N):
    e_np = ro.energies(N, 37, 11)
    e_np[:, 3] = 0.0
    e_np[:, 35] = -0.0
    assert np.signbit(e_np[:, 35]).all()
    got = ops.batch_sum(torch.from_numpy(e_np).to(DEV))
    assert _same_bits(got, ro.batch_sum_model(e_np))
    assert (_bits(got)[[3, 35]] == 0).all()  # +0.0: value zero, sign bit clear


def test_batch_sum_nan_and_inf_stay_in_their_column():
    e_np = ro.energies(321, 65, 12)
    clean = ops.batch_sum(torch.from_numpy(e_np).to(DEV))
    e_np[100, 5], e_np[257, 40] = np.nan, np.inf
    got = ops.batch_sum(torch.from_numpy(e_np).to(DEV)).cpu()
    assert torch.isnan(got[5]) and got[40] == float("inf")
    others = np.setdiff1d(np.arange(65), [5, 40])
    assert np.array_equal(_bits(got)[others], _bits(clean)[others])
    assert np.array_equal(_bits(got)[others], ro.bits(ro.batch_sum_model(e_np))[others])


def test_batch_sum_of_a_column_slice():
    """A non-contiguous [N, C] view goes through ops.batch_sum's .contiguous()."""
    e_np = ro.energies(79, 150, 13)
    view = torch.from_numpy(e_np).to(DEV)[:, 3:68]
    assert not view.is_contiguous()
    assert _same_bits(ops.batch_sum(view), ro.batch_sum_model(np.ascontiguousarray(e_np[:, 3:68])))


# ---- dcts_running_mean_update_f32 ----------------------------------------------------------------------------------------
# the cross product thinned to one C per N in rotation, and every C at N = 257
MEAN_CASES = [(N, ro.CS[i % len(ro.CS)]) for i, N in enumerate(ro.NS)]
MEAN_CASES += [(257, C) for C in ro.CS if (257, C) not in MEAN_CASES]


@pytest.mark.parametrize("N,C", MEAN_CASES)
def test_running_mean_has_the_models_bits(N, C):
    """One update of a random positive feature_result for every total_before of the list against running_mean_model."""
    e_np, _ = _case(N, C)
    e = torch.from_numpy(e_np).to(DEV)
    frs = Arena([C] * len(ro.TOTALS))
    for i, total in enumerate(ro.TOTALS):
        fr0 = ro.feature_result(C, 2000 + N + i, total, N)
        _update(e, frs.fill(i, fr0), total)
        assert _same_bits(frs[i], ro.running_mean_model(fr0, total, e_np)), (N, C, total)
    assert frs.guards_intact()


CHAIN = (5, 256, 3, 321)


@pytest.mark.parametrize("C", [37, 2049])
def test_device_accumulator_chain_has_the_models_bits(C):
    batches = [ro.energies(n, C, 3000 + n) for n in CHAIN]
    dev = DeviceAccumulator(C, DEV)
    for e in batches:
        dev.update(torch.from_numpy(e).to(DEV))
    assert dev.total == sum(CHAIN)
    assert ro.bits(dev.scores()).tolist() == ro.bits(ro.chain_model(batches, C)).tolist()


def test_integer_energies_device_bytes_are_the_hosts():
    """Integer energies: every sum is exact in any order, so host (torch CPU ops, the reference's own) and device differ in
    nothing but the three roundings of the update - which the header says are the same."""
    rng = np.random.default_rng(5)
    batches = [rng.integers(0, 1001, size=(n, 37)).astype(np.float32) for n in (5, 1000, 3)]
    host, dev = HostAccumulator(), DeviceAccumulator(37, DEV)
    for e in batches:
        host.update(torch.from_numpy(e))
        dev.update(torch.from_numpy(e).to(DEV))
    assert host.total.item() == dev.total == 1008
    assert dev.scores().tobytes() == host.scores().tobytes()
    assert dev.scores().tobytes() == ro.chain_model(batches, 37).tobytes()


def test_random_energies_host_and_device_within_the_bound_of_the_rule():
    """Bound: the sum bound (N_max - 1) 2^-24 of the largest batch plus three roundings per update over B updates, all
    terms non-negative so that nothing cancels, times 2 for the second-order terms: 2 (N_max + 3 B) 2^-24."""
    batches = [ro.energies(n, 2049, 4000 + n) for n in CHAIN]
    host, dev = HostAccumulator(), DeviceAccumulator(2049, DEV)
    for e in batches:
        host.update(torch.from_numpy(e))
        dev.update(torch.from_numpy(e).to(DEV))
    ref = ro.rule_f64(batches)
    bound = 2 * (max(CHAIN) + 3 * len(CHAIN)) * 2.0 ** -24
    worst = {k: float((np.abs(v.astype(np.float64) - ref) / ref).max()) for k, v in (("host", host.scores()), ("device", dev.scores()))}
    print("REDUCE rule_f64: worst relative error host %.3e device %.3e bound %.3e" % (worst["host"], worst["device"], bound))
    assert worst["host"] <= bound and worst["device"] <= bound


# ---- dcts_running_mean_update_multi_f32 ----------------------------------------------------------------------------------
MULTI_N = (1, 15, 17, 65, 257, 321)
MULTI_C = (1, 31, 32, 33, 37, 64, 65, 257, 2049)
MULTI_T = (0, 5, 261, 1000)
MULTI_MAX = 129


def _multi_shape(i):
    # periods 6, 9 and 4 (together 36): a launch of 64 holds every C, the C = 1 strip next to cmax = 2049
    return MULTI_N[i % len(MULTI_N)], MULTI_C[i % len(MULTI_C)], MULTI_T[i % len(MULTI_T)]


@functools.lru_cache(maxsize=1)
def _multi_inputs():
    """Per descriptor: energies, start state and the model's result; computed once for all counts."""
    out = []
    for i in range(MULTI_MAX):
        N, C, total = _multi_shape(i)
        e = ro.energies(N, C, 5000 + i)
        fr0 = ro.feature_result(C, 6000 + i, total, N)
        out.append((e, fr0, total, ro.running_mean_model(fr0, total, e)))
    return out


def _descs(es, frs, totals):
    descs = (_lib.UpdateDesc * len(es))()
    for d, e, fr, total in zip(descs, es, frs, totals):
        d.energy_nc, d.feature_result, d.N, d.C_count, d.total_before = e.data_ptr(), fr.data_ptr(), e.shape[0], e.shape[1], float(total)
    return descs


def _multi_state(count):
    inputs = _multi_inputs()[:count]
    es = [torch.from_numpy(e).to(DEV) for e, _, _, _ in inputs]
    frs = Arena([len(fr0) for _, fr0, _, _ in inputs])
    for i, (_, fr0, _, _) in enumerate(inputs):
        frs.fill(i, fr0)
    return inputs, es, frs


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_multi_has_the_models_and_the_single_calls_bits(count):
    inputs, es, frs = _multi_state(count)
    _, _, twins = _multi_state(count)
    totals = [t for _, _, t, _ in inputs]
    descs = _descs(es, [frs[i] for i in range(count)], totals)
    _lib.check(_lib.load().dcts_running_mean_update_multi_f32(descs, count, _stream()))
    for i in range(count):
        _update(es[i], twins[i], totals[i])
    for i in range(count):
        assert _same_bits(frs[i], inputs[i][3]), (i, _multi_shape(i))
        assert _same_bits(frs[i], twins[i]), (i, _multi_shape(i))
    assert frs.guards_intact() and twins.guards_intact()


def test_batch_accumulator_has_the_models_bits():
    """Three batches over 70 keys, added in another order each time; the first repeated key flushes the batch before."""
    keys = list(range(70))
    widths = [MULTI_C[k % len(MULTI_C)] for k in keys]
    sizes = (17, 65, 5)
    batches = [[ro.energies(n, widths[k], 7000 + 100 * b + k) for k in keys] for b, n in enumerate(sizes)]
    acc = DeviceBatchAccumulator(DEV)
    single = [DeviceAccumulator(w, DEV) for w in widths]
    order = random.Random(9)
    for b in range(3):
        for k in order.sample(keys, len(keys)):
            e = torch.from_numpy(batches[b][k]).to(DEV)
            acc.add(k, e)
            single[k].update(e)
        assert len(acc.pending) == 70  # nothing was flushed inside a batch
    for k in keys:
        got = acc.scores(k)
        assert acc.state[k][1] == sum(sizes)
        assert got.tobytes() == ro.chain_model([batches[b][k] for b in range(3)], widths[k]).tobytes(), k
        assert got.tobytes() == single[k].scores().tobytes(), k


@pytest.mark.parametrize("fault,code", [("N", -2), ("energy_nc", -1)])
def test_multi_refuses_before_it_updates_anything(fault, code):
    """A bad descriptor in the second chunk of 64: the call returns its code and no feature_result has changed, the 64 of
    the first chunk included (a caller that raises and keeps its totals may then retry the batch)."""
    inputs, es, frs = _multi_state(65)
    descs = _descs(es, [frs[i] for i in range(65)], [t for _, _, t, _ in inputs])
    if fault == "N":
        descs[64].N = 0
    else:
        descs[64].energy_nc = None
    assert _lib.load().dcts_running_mean_update_multi_f32(descs, 65, _stream()) == code
    torch.cuda.synchronize()
    changed = [i for i in range(65) if not _same_bits(frs[i], inputs[i][1])]
    assert changed == []
    assert frs.guards_intact()
