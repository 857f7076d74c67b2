"""The stream contract of include/dctscore.h ("every entry point only ENQUEUES work on that stream"), pinned without a GPU:
`make -C dct_pruning_amd/csrc streams` builds api.hip with every dispatcher that takes a hipStream_t redirected to a recorder
(tests/native/stream_trace.cpp) that notes its name and the stream it received, and runs the driver as a fresh process with
the GPU hidden. The driver makes every call once with each of two fake stream tokens; every dispatcher call api.hip makes for
an entry point - in a chunk loop, in the one-sample inner calls of the weighted path, behind the fp16 upcast, per batch of a
long list - must carry the token that entry point was given. What happens INSIDE a dispatcher (the hipLaunchKernelGGL sites)
is the business of tests/test_streams_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dct_pruning_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def trace():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    env = {k: v for k, v in os.environ.items() if k != "DCTS_SPLIT_CHUNK_MB"}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # the make recipe sets these too; the driver refuses to start otherwise
    p = subprocess.run(["make", "-j6", "-C", CSRC, "streams"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=1500, env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    calls, memo = [], []
    for line in _read("dct_pruning_amd", "csrc", "_obj", "stream_trace.txt").splitlines():
        head, _, records = line.partition("|")
        f = head.split()
        if f[0] == "call":  # call <entry> <case> <token> rc=<rc> | name@token ...
            calls.append(dict(entry=f[1], case=f[2], given=f[3], rc=int(f[4][3:]), records=[r.split("@") for r in records.split()]))
        else:  # memo <i> <token> rc=<rc> built|reused | ...
            assert f[0] == "memo", line
            memo.append(dict(given=f[2], rc=int(f[3][3:]), tables=f[4], records=[r.split("@") for r in records.split()]))
    redirected = set(_read("dct_pruning_amd", "csrc", "_obj", "stream_redirected.txt").split())
    return calls, memo, redirected


def test_every_dispatcher_call_carries_the_stream_of_its_entry_point(trace):
    calls, _, _ = trace
    assert len(calls) > 250
    assert {c["given"] for c in calls} == {"S1", "S2"}
    for c in calls:
        where = "%s %s on %s" % (c["entry"], c["case"], c["given"])
        # 0, or the call stopped early or launched for real (a dispatcher that is not redirected: positive hipError_t, no GPU here)
        assert c["rc"] == 0, "%s returned %d after %s" % (where, c["rc"], c["records"])
        assert c["records"], "%s dispatched nothing" % where
        strays = [r for r in c["records"] if r[1] != c["given"]]
        assert not strays, "%s: %s" % (where, ", ".join("%s got stream %s" % (n, s) for n, s in strays))
    # the S2 sweep is the S1 sweep: same calls, same dispatchers in the same order (the direct family's memo is per stream)
    s1 = [(c["entry"], c["case"], [r[0] for r in c["records"]]) for c in calls if c["given"] == "S1"]
    s2 = [(c["entry"], c["case"], [r[0] for r in c["records"]]) for c in calls if c["given"] == "S2"]
    assert s1 == s2


def test_the_driver_reaches_every_route_of_api_hip(trace):
    """The routes the issue of this test names, read off the records: a shape that stopped reaching its route would leave the
    contract of that route unchecked without failing anything above."""
    calls, _, redirected = trace
    by = {}
    for c in calls:
        if c["given"] == "S1":
            by[(c["entry"], c["case"])] = [r[0] for r in c["records"]]
    seen = {n for names in by.values() for n in names}
    assert seen == redirected, "never dispatched: %s" % sorted(redirected - seen)
    # tables built, then reused on the same workspace and stream (an explicit request at 13 x 13, AUTO at 67 x 67)
    for edge in ("13", "67"):
        assert by[("dcts_energy_f32_ex", "direct" + edge)] == ["launch_basis", "dispatch_direct"]
        assert by[("dcts_energy_f32_ex", "direct%sagain" % edge)] == ["dispatch_direct"]
    # the weighted path: one inner coefficient call and one reduction per sample (N = 3), or per run of channels of a sample;
    # its inner calls never cache their tables
    assert by[("dcts_weighted_energy_f32", "tile2g72")] == ["dispatch_tile2g_coeff", "launch_weighted_reduce"] * 3
    assert by[("dcts_weighted_energy_f32", "direct67")] == ["launch_basis", "dispatch_direct", "launch_weighted_reduce"] * 3
    assert by[("dcts_weighted_energy_f32", "tile2g72_runs")] == ["dispatch_tile2g_coeff", "launch_weighted_reduce"] * 9  # runs of 2, 2, 1
    # both regimes of for_chunks(): whole samples per chunk, runs of channels of one sample (N = 3, five channels in 2, 2, 1)
    direct = ["launch_basis", "dispatch_direct"]
    for entry, reduce, large in (("dcts_band_energy_f32", "launch_band_reduce", ["dispatch_tile2g_coeff"]),
                                 ("dcts_spectral_entropy_f32", "launch_entropy_reduce", ["dispatch_tile2g_coeff"]),
                                 ("dcts_dct2d_lowpass_f32", "launch_lowpass_gather", direct)):  # its inner calls ask for AUTO
        assert by[(entry, "fallback72_samples")] == large + [reduce]
        assert by[(entry, "fallback72_runs")] == (large + [reduce]) * 9
        assert by[(entry, "fallback13x17_samples")] == ["dispatch_rect", reduce]
        assert by[(entry, "fallback13x17_runs")] == ["dispatch_rect", reduce] * 9
        assert by[(entry, "fallback67_samples")] == (direct + [reduce]) * 3  # a chunk of five maps: one sample
    # the staged fp16 route: upcast, then run()
    assert by[("dcts_energy_typed", "f16_staged20")] == ["launch_upcast_half", "dispatch_codelet"]
    assert by[("dcts_energy_typed", "bf16_staged20_runs")] == ["launch_upcast_half", "dispatch_codelet"] * 9
    assert by[("dcts_energy_typed", "f16_staged67")] == ["launch_upcast_half"] + direct
    runs67 = by[("dcts_energy_typed", "bf16_staged67_runs")]
    assert runs67.count("launch_upcast_half") == 9 and runs67.count("dispatch_direct") == 9
    # lists cut at 32 tensors per launch, 48 per mixed launch, 64 per shape group of the mixed call
    assert by[("dcts_energy_multi_f32", "codelet14x40")] == ["dispatch_codelet_multi"] * 2
    assert by[("dcts_energy_multi_f32", "tile2g72x70")] == ["dispatch_tile2g"] * 3
    assert by[("dcts_energy_multi_f32", "pipe128_unaligned_between")] == ["dispatch_tile2g", "dispatch_pipe"]
    mixed = by[("dcts_energy_mixed_f32", "175items")]
    assert mixed.count("dispatch_codelet_mixed") == 3 and mixed.count("dispatch_codelet_multi") == 3 + 1
    assert by[("dcts_running_mean_update_multi_f32", "150descs")] == ["launch_running_mean_multi"] * 3


def test_the_basis_memo_is_per_stream(trace):
    """basis_cached() / basis_remember(): one shape per workspace, and a same-stream entry only - what orders the build before
    the reuse. Direct 13 x 13 on one workspace on S1, S1, S2, S2, S1."""
    _, memo, _ = trace
    assert [m["given"] for m in memo] == ["S1", "S1", "S2", "S2", "S1"]
    assert all(m["rc"] == 0 for m in memo)
    assert [m["tables"] for m in memo] == ["built", "reused", "built", "reused", "built"]
    for m in memo:
        assert m["records"] and all(s == m["given"] for _, s in m["records"]), m


def _stream_dispatchers():
    """dispatch_* / launch_* declared in dcts_internal.h or rect.h with a hipStream_t parameter."""
    text = _read("dct_pruning_amd", "csrc", "dcts_internal.h") + _read("dct_pruning_amd", "csrc", "rect.h")
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"\bint\s+((?:dispatch|launch)_\w+)\s*\([^;{}]*?\bhipStream_t\b[^;{}]*?\)\s*;", text))


def _stream_entry_points():
    """dcts_* functions of include/dctscore.h with a `void* stream` parameter."""
    text = re.sub(r"/\*.*?\*/", "", _read("include", "dctscore.h"), flags=re.S)
    return set(re.findall(r"\b(dcts_\w+)\s*\([^;{}]*?\bvoid\s*\*\s*stream\b[^;{}]*?\)\s*;", text))


def test_no_dispatcher_and_no_entry_point_is_left_out(trace):
    """So that the next kernel family cannot be forgotten: every dispatcher with a stream that api.hip mentions is redirected,
    and the driver called every entry point with a stream that api.hip defines."""
    calls, _, redirected = trace
    api = re.sub(r"//[^\n]*", "", _read("dct_pruning_amd", "csrc", "api.hip"))
    declared = _stream_dispatchers()
    assert len(declared) >= 38 and "dispatch_rect" in declared and "launch_lowpass_gather" in declared
    used = {d for d in declared if re.search(r"\b%s\b" % d, api)}
    assert {"dispatch_gm", "dispatch_gm_metric", "dispatch_gm_pairs", "dispatch_lowpass", "launch_lowpass_gather"} <= used
    assert used - redirected == set(), "add to STREAMED in csrc/Makefile, with a recorder in tests/native/stream_trace.cpp"
    assert redirected - declared == set()

    entries = _stream_entry_points()
    assert len(entries) >= 20 and "dcts_energy_f32_ex" in entries and "dcts_debug_stream_read_f32" in entries
    called = {c["entry"] for c in calls}
    # an entry point defined beside its kernel launches there: no dispatcher of api.hip carries its stream (dcts_rank_f32,
    # rank.hip; tests/test_streams_gpu.py covers it on the GPU)
    in_api = {e for e in entries if re.search(r"\bint\s+%s\s*\(" % e, api)}
    assert entries - in_api == {"dcts_rank_f32"}
    assert in_api - called == set(), "add calls to tests/native/stream_trace.cpp"
    assert called <= entries
