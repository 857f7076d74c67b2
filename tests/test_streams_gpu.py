"""The stream contract of include/dctscore.h on the GPU: "every entry point only ENQUEUES work on that stream; there is no
implicit synchronisation". tests/test_streams_cpu.py pins the stream every dispatcher is handed; this module pins what the
dispatchers do with it, launch site by launch site (tests/stream_cases.py), in two ways.

Eager, behind a delayed producer. The input and the workspace hold NaN and the output a sentinel. A side stream (non-blocking
towards the null stream) gets: a sleep, an event, the copy of the real input, the entry point. The call must return while the
sleep still runs (the event has not fired: nothing made the host wait), and after the stream has drained the output must hold
no sentinel and no NaN, the bits of the same call on the default stream, and the float64 oracle of the family's own test at
that test's tolerance. A launch that leaked to another stream runs at once: it reads NaN, or writes before the producer has
run. If the event HAS fired when the call returns, the case fails whatever the reason (the library waited, or the delay was
too short for this host: inconclusive is not a pass).

The delay: measured on an MI355X host after warm-up (time.perf_counter on an idle stream, five repeats per case), the slowest
call of the table takes 0.018 ms on the host (weighted72: three inner coefficient calls and three reductions), and the slowest
producer-plus-call, from the sleep's enqueue to the call's return, 0.31 ms in steady state (running-mean-multi70: 70 copies,
then the call) with one outlier of 1.85 ms on the first use of a stream. DELAY_MS = 40 is more than 20 times the outlier and
above the 20 ms floor; torch.cuda._sleep is calibrated against events once per module.

Capture and replay. No delay to rest on: one representative per .hip unit is captured into a graph on a side stream (nothing
may run during capture: the output is still all sentinel afterwards), then replayed on two other inputs; each replay has the
bits of an eager call. The direct family twice: tables built before the capture, and k_basis inside the graph.

Then the Python layer under `with torch.cuda.stream(s)`: every op whose docstring promises "no synchronisation", the device
accumulators, and imp_score on ResNet-56 in its three device modes against a default-stream run, byte for byte."""
import contextlib
import functools
import io
import os
import re
import time
import types

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import stream_cases as sc
from dct_pruning_amd import _lib, accumulate, harness, nets, ops
from dct_pruning_amd.data import SyntheticLoader
from helpers import HARNESS_CASES, deterministic_init, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MEASURED_CALL_MS, MEASURED_HOST_MS = 0.018, 1.85  # the module docstring: slowest call, slowest producer-plus-call
DELAY_MS = 40.0
assert DELAY_MS >= 20.0 and DELAY_MS >= 20 * max(MEASURED_CALL_MS, MEASURED_HOST_MS)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep spins for a number of device clock cycles: how many make a millisecond here."""
    torch.cuda._sleep(1000000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20000000
    a.record()
    torch.cuda._sleep(n)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.5, "torch.cuda._sleep(%d) took %.3f ms: cannot calibrate a delay" % (n, ms)
    return n / ms


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream()


class Producer:
    """sleep, event, then the copies of `fresh` into `dst`, enqueued on the current stream; after(): the check of step 4."""

    def __init__(self, cycles_per_ms):
        self.cycles = int(DELAY_MS * cycles_per_ms)

    def start(self, dst, fresh):
        self.ev = torch.cuda.Event()
        self.t0 = time.perf_counter()
        torch.cuda._sleep(self.cycles)
        self.ev.record()
        for d, f in zip(dst, fresh):
            d.copy_(f, non_blocking=True)

    def after(self, what):
        fired = self.ev.query()
        host_ms = (time.perf_counter() - self.t0) * 1e3
        assert not fired, ("%s: the delay of %.0f ms on the stream was over when the call returned, %.2f ms after it was enqueued: "
                           "the call waited for the stream, or the delay is too short for this host (inconclusive)"
                           % (what, DELAY_MS, host_ms))


def _poison(run):
    """Step 2: NaN input and workspace (the library is told), sentinel output."""
    for x in run.xs:
        x.fill_(float("nan"))
    if run.ws is not None:
        run.ws.fill_(0xFF)
        _lib.load().dcts_workspace_invalidate_range(run.ws.data_ptr(), run.ws.numel())
    run.reset_outs()


def _ok(rc, what):
    assert rc == 0, "%s returned %d (%s)" % (what, rc, _lib.load().dcts_strerror(rc).decode())


def _default_stream_result(run, v):
    """The same call on the default stream on input variant v: the bits everything is compared with."""
    for x, f in zip(run.xs, run.fresh[v]):
        x.copy_(f)
    if run.ws is not None:
        _lib.load().dcts_workspace_invalidate_range(run.ws.data_ptr(), run.ws.numel())
    run.reset_outs()
    _ok(run.call(torch.cuda.current_stream().cuda_stream), "default-stream call")
    torch.cuda.synchronize()
    return [o.clone() for o in run.outs]


def _assert_written(run, outs, what):
    for o in outs:
        assert not torch.isnan(o).any(), "%s: NaN in the output" % what
        if not run.inout:
            assert not (o == sc.SENTINEL).any(), "%s: output elements were never written" % what


def _assert_same_bits(got, want, what):
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w)), "%s: not the bits of the default-stream call" % what


# ----------------------------------------------------------------------------------------------------
# completeness
# ----------------------------------------------------------------------------------------------------
def test_every_entry_point_with_a_stream_has_a_case():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dctscore.h")).read(), flags=re.S)
    entries = set(re.findall(r"\b(dcts_\w+)\s*\([^;{}]*?\bvoid\s*\*\s*stream\b[^;{}]*?\)\s*;", text))
    assert len(entries) >= 20
    assert entries == {c.entry for c in sc.CASES}
    # one capture representative per .hip unit that holds a kernel
    csrc = os.path.join(ROOT, "dct_pruning_amd", "csrc")
    units = {f[:-4] for f in os.listdir(csrc) if f.endswith(".hip")} - {"api", "all_units"}
    assert units == {u for c in sc.CASES if c.capture for u in c.units}
    assert units == {u for c in sc.CASES for u in c.units}
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)


# ----------------------------------------------------------------------------------------------------
# layer 2: eager, behind a delayed producer on a side stream
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_eager_behind_a_delayed_producer(case, side, cycles_per_ms):
    run = case.build()
    want = _default_stream_result(run, 0)  # step 1 as well: code objects loaded, once-per-process reads made
    if case.reuse_tables:  # the tables are built on the side stream now and must be found there by the call under test
        _ok(run.call(side.cuda_stream), "table-building call")
        side.synchronize()
        ws, run.ws = run.ws, None
        _poison(run)
        run.ws = ws
    else:
        _poison(run)
    torch.cuda.synchronize()
    producer = Producer(cycles_per_ms)
    with torch.cuda.stream(side):
        producer.start(run.xs, run.fresh[0])
        rc = run.call(side.cuda_stream)
        producer.after(case.name)
    _ok(rc, case.name)
    side.synchronize()
    got = [o.clone() for o in run.outs]
    torch.cuda.synchronize()
    _assert_written(run, got, case.name)
    _assert_same_bits(got, want, case.name)
    run.check(0, [g.cpu() for g in got])


def test_basis_memo_across_two_streams(side, cycles_per_ms):
    """One workspace, ALGO_DIRECT 13 x 13 on s1, on s2 behind its own delayed producer, on s1 again: the memo is per stream
    (the tables are rebuilt on s2, in stream order before their use), and all three carry the default-stream bits."""
    case = next(c for c in sc.CASES if c.name == "energy-direct13-built")
    run = case.build()
    want = _default_stream_result(run, 0)
    s1, s2 = side, torch.cuda.Stream()
    _poison(run)
    torch.cuda.synchronize()
    for i, s in enumerate((s1, s2, s1)):
        run.reset_outs()
        for x in run.xs:
            x.fill_(float("nan"))
        if i == 1:  # whatever s1 left in the workspace: s2 must not rely on it
            run.ws.fill_(0xFF)
        torch.cuda.synchronize()
        producer = Producer(cycles_per_ms)
        with torch.cuda.stream(s):
            producer.start(run.xs, run.fresh[0])
            rc = run.call(s.cuda_stream)
            producer.after("direct 13x13, call %d" % i)
        _ok(rc, "direct 13x13, call %d" % i)
        s.synchronize()
        got = [o.clone() for o in run.outs]
        _assert_written(run, got, "call %d" % i)
        _assert_same_bits(got, want, "call %d" % i)


# ----------------------------------------------------------------------------------------------------
# layer 3: capture and replay
# ----------------------------------------------------------------------------------------------------
def _capture_and_replay(case, side, tables_before):
    run = case.build()
    lib = _lib.load()
    want = [_default_stream_result(run, v) for v in (1, 2)]
    # 1. warm up eagerly on the side stream (direct family: this builds the tables there, under the stream the capture uses)
    for x, f in zip(run.xs, run.fresh[0]):
        x.copy_(f)
    torch.cuda.synchronize()
    _ok(run.call(side.cuda_stream), "warm-up on the side stream")
    side.synchronize()
    if run.ws is not None and not tables_before:
        lib.dcts_workspace_invalidate_range(run.ws.data_ptr(), run.ws.numel())
        run.ws.fill_(0xFF)
    run.reset_outs()  # 2.
    before = [o.clone() for o in run.outs]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # 3.
        rc = run.call(side.cuda_stream)
    _ok(rc, "%s during capture" % case.name)
    torch.cuda.synchronize()
    for o, b in zip(run.outs, before):  # 4. nothing ran outside the capture
        assert torch.equal(_bits(o), _bits(b)), "%s: the output changed during capture" % case.name
    for v in (1, 2):  # 5., 6.
        for x, f in zip(run.xs, run.fresh[v]):
            x.copy_(f)
        run.reset_outs()
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in run.outs]
        _assert_written(run, got, "%s replay %d" % (case.name, v))
        _assert_same_bits(got, want[v - 1], "%s replay %d" % (case.name, v))
    if run.ws is not None:
        lib.dcts_workspace_invalidate_range(run.ws.data_ptr(), run.ws.numel())


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.capture], ids=repr)
def test_capture_and_replay(case, side):
    # direct family: "-reused" has its tables built before the capture on the same stream, "-built" has k_basis in the graph
    _capture_and_replay(case, side, tables_before=case.reuse_tables)


# ----------------------------------------------------------------------------------------------------
# the Python layer under `with torch.cuda.stream(s)`
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _band_w(h):  # made once, by the default-stream call: a host-to-device copy under the delay would wait for the stream
    return torch.rand(3, h, h, generator=torch.Generator().manual_seed(3)).to(DEV)


# name: (ops function, make(x) -> result on the current stream, input shape); the direct, staged and fallback routes as well,
# whose workspace is the one ops.py keeps per (device, stream)
OPS = {
    "energy_nc": (ops.energy_nc, lambda x: dpa.energy_nc(x), (2, 5, 14, 14)),
    "energy_nc-direct13": (ops.energy_nc, lambda x: dpa.energy_nc(x), (2, 5, 13, 13)),
    "energy_nc-split88": (ops.energy_nc, lambda x: dpa.energy_nc(x), (2, 5, 88, 88)),
    "energy_nc-bf16-staged20": (ops.energy_nc, lambda x: dpa.energy_nc(x.bfloat16()), (2, 5, 20, 20)),
    "energy_nc-channels-last": (ops.energy_nc, lambda x: dpa.energy_nc(x.contiguous(memory_format=torch.channels_last)), (2, 5, 14, 14)),
    "band_energy_nc": (ops.band_energy_nc, lambda x: dpa.band_energy_nc(x, _band_w(14)), (2, 5, 14, 14)),
    "band_energy_nc-fallback72": (ops.band_energy_nc, lambda x: dpa.band_energy_nc(x, _band_w(72)), (2, 5, 72, 72)),
    "spectral_entropy_nc": (ops.spectral_entropy_nc, lambda x: dpa.spectral_entropy_nc(x), (2, 5, 14, 14)),
    "spectral_entropy_nc-fallback13": (ops.spectral_entropy_nc, lambda x: dpa.spectral_entropy_nc(x), (2, 5, 13, 13)),
    "rank_nc": (ops.rank_nc, lambda x: dpa.rank_nc(x), (2, 5, 14, 14)),
    "lowpass_nc": (ops.lowpass_nc, lambda x: dpa.lowpass_nc(x, 4), (2, 5, 14, 14)),
    "lowpass_nc-fallback13x17": (ops.lowpass_nc, lambda x: dpa.lowpass_nc(x, 4, drop_dc=True), (2, 5, 13, 17)),
    "gm_distance_nc": (ops.gm_distance_nc, lambda x: dpa.gm_distance_nc(x), (2, 12, 7, 7)),
    "gm_distance_nc-cosine": (ops.gm_distance_nc, lambda x: dpa.gm_distance_nc(x, metric="cosine"), (2, 12, 7, 7)),
    "gm_distance_nc-lowpass": (ops.gm_distance_nc, lambda x: dpa.gm_distance_nc(x, metric="correlation", lowpass=3), (2, 12, 14, 14)),
    "gm_pair_matrix": (ops.gm_pair_matrix, lambda x: dpa.gm_pair_matrix(x, metric="cosine"), (5, 3, 4, 4)),
    "gm_pair_matrix-lowpass": (ops.gm_pair_matrix, lambda x: dpa.gm_pair_matrix(x, lowpass=3), (5, 3, 14, 14)),
}


def test_every_op_that_promises_no_synchronisation_is_tested():
    promised = {f for name, f in vars(ops).items() if callable(f) and not name.startswith("_")
                and "no synchronisation" in " ".join((getattr(f, "__doc__", None) or "").split())}
    assert len(promised) >= 7
    assert promised == {fn for fn, _, _ in OPS.values()}
    for fn in (ops.gm_distance_nc, ops.gm_pair_matrix):
        assert any(f is fn and "lowpass" in name for name, (f, _, _) in OPS.items())


def _python_layer(make, x_shape, side, cycles_per_ms, what, half=False):
    """make(x) under the side stream behind a delayed producer: returns while the delay runs, and gives the bits of the
    default-stream call."""
    fresh = synth(*x_shape, seed=7).to(DEV)
    want = make(fresh)
    torch.cuda.synchronize()
    x = torch.empty_like(fresh)
    with torch.cuda.stream(side):
        make(fresh)  # warm-up on the side stream: ops.py allocates that stream's workspace now, not under the delay
        side.synchronize()
        ws = ops._workspaces.get((x.device.index, side.cuda_stream))
        if ws is not None:
            ws.fill_(0xFF)
            _lib.load().dcts_workspace_invalidate_range(ws.data_ptr(), ws.numel())
        x.fill_(float("nan"))
        side.synchronize()
        producer = Producer(cycles_per_ms)
        producer.start([x], [fresh])
        got = make(x)
        producer.after(what)
    side.synchronize()
    got = got if isinstance(got, (list, tuple)) else [got]
    want = want if isinstance(want, (list, tuple)) else [want]
    for g, w in zip(got, want):
        g, w = torch.as_tensor(g), torch.as_tensor(w)
        assert not torch.isnan(g.float()).any(), what
        assert torch.equal(_bits(g), _bits(w)), "%s: not the bits of the default-stream call" % what


@pytest.mark.parametrize("name", sorted(OPS))
def test_ops_on_a_side_stream(name, side, cycles_per_ms):
    _, make, shape = OPS[name]
    _python_layer(make, shape, side, cycles_per_ms, name)


def test_accumulators_on_a_side_stream(side, cycles_per_ms):
    def device_accumulator(e):
        acc = accumulate.DeviceAccumulator(e.shape[1], DEV)
        acc.update(e)
        acc.update(e)
        return acc.feature_result

    def batch_accumulator(x):
        acc = accumulate.DeviceBatchAccumulator(DEV)
        acc.add_tensor("a", x, 0, 5, False)
        acc.add_tensor("b", x, 1, 3, False)
        acc.flush()
        acc.add_tensor("a", x, 0, 5, False)
        acc.flush()
        return [acc.state["a"][0], acc.state["b"][0]]

    def pair_accumulator(x):
        acc = accumulate.PairAccumulator(torch.device(DEV))
        m = dpa.gm_pair_matrix(x)
        acc.update(m, x.shape[0])
        acc.update(m, x.shape[0])
        return acc.sum

    _python_layer(lambda x: device_accumulator(x.reshape(4, -1)[:, :37].contiguous()), (4, 5, 4, 4), side, cycles_per_ms, "DeviceAccumulator.update")
    _python_layer(batch_accumulator, (2, 5, 16, 16), side, cycles_per_ms, "DeviceBatchAccumulator.add_tensor / flush")
    _python_layer(pair_accumulator, (5, 3, 4, 4), side, cycles_per_ms, "PairAccumulator (device)")


def _imp_score(root, **kw):
    name = "resnet_56"
    bs, limit, size, as_dict = HARNESS_CASES[name]
    net = deterministic_init(nets.get_network(name)).to(DEV)
    loader = SyntheticLoader((3, size, size), bs, limit + 1, seed=7, as_dict=as_dict)
    args = types.SimpleNamespace(net=name, limit=limit, dataset="synthetic", batch_size=bs, data_dir=".")
    os.makedirs(str(root), exist_ok=True)
    cwd = os.getcwd()
    os.chdir(str(root))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            harness.imp_score(net, args, train_loader=loader, **kw)
    finally:
        os.chdir(cwd)
    d = os.path.join(str(root), "importance_score", "%s_limit%d" % (name, limit))
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("mode,kw", [("per-hook", {}), ("device-accumulate", {"accumulate": "device"}),
                                     ("single-sweep-deferred", {"single_sweep": True, "accumulate": "device", "deferred": True})])
def test_imp_score_with_a_side_stream_current(mode, kw, side, tmp_path):
    """The forward pass, the hooks' launches and the accumulators all follow the current stream: the score files of a run with
    a side stream current are those of a default-stream run, byte for byte."""
    base = _imp_score(tmp_path / "default", **kw)
    assert len(base) == 55
    with torch.cuda.stream(side):
        got = _imp_score(tmp_path / "side", **kw)
    side.synchronize()
    assert sorted(got) == sorted(base)
    for f in base:
        assert got[f] == base[f], "%s %s" % (mode, f)
        assert np.isfinite(np.load(io.BytesIO(got[f]))).all()
