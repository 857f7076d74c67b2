"""The grid-loop tests without a GPU:
(1) tests/grid_capacity.py, the Python restatement of the launch rules the GPU cases are sized by, equals what
    tests/native/grid_probe.cpp prints from the headers the launch sites include (`make -C dct_pruning_amd/csrc probe`),
    for 256 and 304 CUs;
(2) the checking function of tests/loop_cases.py passes a numpy model of the grid-stride schedule, with the fp32 oracle in
    the library's place, at a small fake capacity - and fails every mutant of that schedule the GPU cases exist to catch;
(3) a periodic index would let the "re-reads its first group" mutant through: the reason the index is random."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import grid_capacity as gc
import loop_cases as lc
from oracle import dct_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dct_pruning_amd", "csrc")
CUS = (256, 304)


@pytest.fixture(scope="module")
def probe():
    """The probe's lines as {family: [dict of its key=value fields]}."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    p = subprocess.run(["make", "-C", CSRC, "probe"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    out = {}
    for line in open(os.path.join(CSRC, "_obj", "grid_probe.txt")).read().splitlines():
        family, *fields = line.split()
        out.setdefault(family, []).append({k: int(v) for k, v in (f.split("=") for f in fields)})
    return out


def test_codelet_table_equals_the_headers(probe):
    for family, sizes in (("codelet", gc.CODELET_SIZES), ("half", gc.HALF_SIZES)):
        assert tuple(r["N"] for r in probe[family]) == sizes
        for r in probe[family]:
            c = gc.codelet_cfg(r["N"])
            assert (c.G, c.WAVES, c.GRID_WAVES_PER_CU) == (r["G"], r["WAVES"], r["GRID_WAVES_PER_CU"]), r
            assert gc.codelet_grid(r["N"], 256) == r["grid256"]
            for cus in CUS:  # the rule of codelet_grid<N> on the probe's own constants
                cap = gc.codelet(r["N"], cus)
                assert cap.units == cus * r["GRID_WAVES_PER_CU"] // r["WAVES"] * r["WAVES"] and cap.maps_per_unit == r["G"]
    assert tuple(r["N"] for r in probe["mixed"]) == gc.MIXED_SIZES
    assert all(gc.codelet_cfg(r["N"]).G == r["G"] for r in probe["mixed"])
    assert probe["multi"] == [{"items": gc.MULTI_ITEMS, "mixed_items": gc.MIXED_ITEMS, "lane_waves": gc.LANE_MULTI_WAVES,
                               "lane_group": gc.LANE_MULTI_G, "mixed_waves": gc.MIXED_WAVES}]


def test_the_issue_counts_on_256_cus():
    """The counts above which a wave of k_energy_codelet takes a second group on a 256-CU MI355X."""
    assert [gc.codelet(n, 256).maps for n in (56, 14, 8, 2)] == [65536, 524288, 1048576, 262144]


def test_nhwc_table_equals_the_headers(probe):
    assert tuple(r["N"] for r in probe["nhwc_lane"]) == gc.NHWC_LANE_SIZES
    for r in probe["nhwc_lane"]:
        assert r["waves"] == gc.NHWC_LANE_WAVES and r["GRID_WAVES_PER_CU"] == gc.codelet_cfg(r["N"]).GRID_WAVES_PER_CU
        for cus in CUS:
            assert gc.nhwc_lane_items(r["N"], cus) == cus * r["GRID_WAVES_PER_CU"] // r["waves"] * r["waves"]
    assert tuple(r["N"] for r in probe["nhwc_block"]) == gc.NHWC_BLOCK_SIZES
    assert [r["N"] for r in probe["nhwc_strip"]] == [gc.NHWC_STRIP_SIZE]
    for r in probe["nhwc_block"] + probe["nhwc_strip"]:
        assert gc.nhwc_block_cb(r["N"]) == r["CB"] and gc.nhwc_block_items(r["N"], 256) == r["grid256"]
        for cus in CUS:
            assert gc.nhwc_block_items(r["N"], cus) == cus * r["GRID_WAVES_PER_CU"] // r["WAVES"]


def test_rect_rank_reduce_and_upcast_tables_equal_the_headers(probe):
    (caps,) = probe["rect_caps"]
    assert (caps["waves"], caps["blocks_per_cu"]) == (gc.RECT_WAVES, gc.RECT_BLOCKS_PER_CU)
    assert [caps["slab16"], caps["slab32"], caps["slab64"]] == [gc.rect_slab_cap(e) for e in (16, 32, 64)]
    assert len(probe["rect"]) == 64 * 64 * 2
    for r in probe["rect"]:
        g = gc.rect_group(r["HP"], r["WP"], bool(r["store"]))
        assert (g.G, g.G1, g.G2, g.map_lds) == (r["G"], r["G1"], r["G2"], r["map_lds"]), r
    for cus in CUS:
        assert gc.rect(14, 14, cus).units == cus * caps["blocks_per_cu"] * caps["waves"]
    assert probe["rank"] == [{"max_blocks": gc.RANK_MAX_BLOCKS}]
    assert [gc.rank(h, w).maps_per_unit for h, w in ((4, 4), (8, 8), (33, 17), (64, 64))] == [16, 8, 2, 1]
    (red,) = probe["reduce"]
    assert (red["waves"], red["max_blocks"]) == (gc.REDUCE_WAVES, gc.REDUCE_MAX_BLOCKS) and gc.reduce().maps == 16384
    assert (red["band_chunk_small"], red["band_chunk_large"]) == (gc.band_chunk_bytes(65, 65), gc.band_chunk_bytes(66, 66))
    (up,) = probe["upcast"]
    assert (up["threads"], up["blocks_per_cu"], up["stage_cap"]) == (gc.UPCAST_THREADS, gc.UPCAST_BLOCKS_PER_CU, gc.HALF_STAGE_CAP)
    for cus in CUS:
        assert gc.upcast_elems(cus) == cus * up["blocks_per_cu"] * up["threads"]


@pytest.mark.parametrize("units,per", [(8, 1), (8, 9), (2048, 32), (131072, 8), (65536, 1), (8192, 2)])
def test_loop_count_runs_three_iterations_and_two_with_a_ragged_last_group(units, per):
    n = gc.loop_count(units, per)
    assert n * 10 >= 23 * units * per and n < 23 * units * per // 10 + 2 * per + 2
    assert gc.iterations(n, units, per) == (2, 3)
    assert per == 1 or n % per != 0


# ----------------------------------------------------------------------------------------------------
# the checker against the model
# ----------------------------------------------------------------------------------------------------
UNITS, WG = 8, 4  # the fake capacity: a grid of eight waves in workgroups of four


@pytest.fixture(scope="module")
def bank8():
    bank = lc.make_bank(8, 8, 5)
    ref64 = torch.from_numpy(orc.energy_nc_f64(bank[None]))[0]
    e32 = orc.energy_nc_batched(bank[None])[0]  # the library's place: the fp32 restatement of the reference
    return bank, ref64, e32


def test_the_bank_is_what_the_cases_rely_on(bank8):
    bank, ref64, e32 = bank8
    assert bank.shape == (lc.B, 8, 8) and all(not bank[i].any() for i in lc.ZERO_MAPS)
    live = ref64[ref64 > 0]
    assert live.unique().numel() == live.numel() >= lc.B - 8  # every live map distinct
    assert ref64[lc.BIG_MAP] > 1e6 * ref64.median() and ref64[lc.SMALL_MAP] < 1e-6 * ref64.median()
    h = lc.make_bank(8, 8, 5, torch.float16)
    assert torch.isfinite(h.float()).all() and h[lc.BIG_MAP].max() >= 5e3
    assert torch.equal(lc.known_ranks(8, 8)[:5], torch.tensor([1.0, 6.0, 3.0, 0.0, 5.0]))


def _check(got, idx, bank8, **kw):
    _, ref64, e32 = bank8
    return lc.check_scores(got, idx, ref64, e32, 1e-4, **kw)


@pytest.mark.parametrize("G", [1, 4, 9])
def test_checker_passes_the_schedule_and_catches_every_mutant(bank8, G):
    nmaps = gc.loop_count(UNITS, G)
    assert gc.iterations(nmaps, UNITS, G) == (2, 3) and (G == 1 or nmaps % G != 0)
    idx = lc.random_index(nmaps, 11 + G)
    src = lc.schedule_sources(nmaps, G, UNITS, WG)
    assert np.array_equal(src, np.arange(nmaps))
    assert _check(lc.model_scores(src, idx, bank8[2]), idx, bank8, group=G, units=UNITS) <= 1e-4
    for mutant in lc.MUTANTS:
        if mutant == "drop_ragged" and G == 1:
            continue  # no ragged group with one map per group
        got = lc.model_scores(lc.schedule_sources(nmaps, G, UNITS, WG, mutant), idx, bank8[2])
        with pytest.raises(AssertionError):
            _check(got, idx, bank8, group=G, units=UNITS)
        if mutant in ("reread_first", "short_stride", "fence_leak"):
            # every entry is written and finite: each comparison ALONE catches these
            _, ref64, e32 = bank8
            with pytest.raises(AssertionError, match="float64|zero bank map"):  # (a) without the twin
                lc.check_scores(got, idx, ref64, None, 1e-4)
            with pytest.raises(AssertionError, match="bank alone"):  # (b) without the bound
                lc.check_scores(got, idx, ref64, e32, None)


def test_a_guard_word_or_an_unwritten_entry_is_caught(bank8):
    nmaps = gc.loop_count(UNITS, 4)
    idx = lc.random_index(nmaps, 3)
    buf, out = lc.guarded(nmaps, 1, "cpu")
    out.copy_(bank8[2][idx])
    assert _check(out, idx, bank8, guard=buf[nmaps:]) <= 1e-4
    buf[nmaps + 1] = 0.0
    with pytest.raises(AssertionError, match="guard"):
        _check(out, idx, bank8, guard=buf[nmaps:])
    z = int((idx == lc.ZERO_MAPS[0]).nonzero()[0])
    out[z] = -0.0
    with pytest.raises(AssertionError, match="zero bank map"):
        _check(out, idx, bank8)
    ref64 = bank8[1]
    assert lc.check_scores(out, idx, ref64, None, 1e-4, signed_zero=True) <= 1e-4  # a coefficient of a zero map may be -0.0 ...
    with pytest.raises(AssertionError, match="bank alone"):  # ... where the bank call gives the same bits ...
        _check(out, idx, bank8, signed_zero=True)
    out[z] = 1e-30
    with pytest.raises(AssertionError, match="zero bank map"):  # ... and nothing but a zero
        lc.check_scores(out, idx, ref64, None, 1e-4, signed_zero=True)
    out[z] = float("nan")
    with pytest.raises(AssertionError, match="not written"):
        _check(out, idx, bank8)


def test_a_periodic_index_would_miss_the_reread_mutant(bank8):
    """A wave that re-reads its first group reads `units * G` places before the right map on every later iteration: an
    index with that period (or a divisor of it) hands it an equal map. The random index does not."""
    G = 4
    nmaps = gc.loop_count(UNITS, G)
    src = lc.schedule_sources(nmaps, G, UNITS, WG, "reread_first")
    assert (src != np.arange(nmaps)).sum() > nmaps // 2
    periodic = lc.periodic_index(nmaps, UNITS * G, 9)
    assert _check(lc.model_scores(src, periodic, bank8[2]), periodic, bank8) <= 1e-4  # the mutant passes
    rnd = lc.random_index(nmaps, 9)
    assert (rnd[torch.from_numpy(src)] != rnd).float().mean() > 0.5
    with pytest.raises(AssertionError):
        _check(lc.model_scores(src, rnd, bank8[2]), rnd, bank8)


@pytest.mark.parametrize("G", [1, 8])
def test_checker_catches_a_multi_tensor_walk_that_loses_its_place(bank8, G):
    total_groups = 23 * UNITS // 10 + 3
    sizes = lc.multi_sizes(4 * total_groups * G - (G // 2), count=12, runs=((2, 3), (7, 2)))
    begin, total = lc.multi_layout(sizes, G)
    assert total % UNITS != 0 and total > 2 * UNITS and sizes.count(1) == 5 and max(sizes) == sum(sizes) // 4
    # some wave's consecutive groups lie two or more tensors apart: what t_one_step needs to go wrong
    tensor_of = np.searchsorted(np.array(begin), np.arange(total), side="right") - 1
    assert (tensor_of[UNITS:] - tensor_of[:-UNITS]).max() >= 2
    idxs = [lc.random_index(s, 100 + i) for i, s in enumerate(sizes)]

    def run(mutant):
        srcs = lc.multi_sources(sizes, G, UNITS, mutant)
        for t, (src, idx) in enumerate(zip(srcs, idxs)):
            _check(lc.model_scores(src, idx, bank8[2]), idx, bank8, what="tensor %d" % t, group=G)

    run(None)
    for mutant in lc.MULTI_MUTANTS:
        with pytest.raises(AssertionError):
            run(mutant)


def test_multi_sizes_span_one_map_to_a_quarter_and_cross_the_chunking():
    for total in (9000, 1234567):
        sizes = lc.multi_sizes(total)
        assert len(sizes) >= 40 and len(sizes) > gc.MULTI_ITEMS and sum(sizes) == total
        assert min(sizes) == 1 and max(sizes) == total // 4
        runs = "".join("1" if s == 1 else "." for s in sizes)
        assert "1111" in runs and "111" in runs.replace("1111", "", 1)
