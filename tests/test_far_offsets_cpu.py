"""tests/far_views.py without a GPU, at unit = cpu_unit(H, W) (2^10 floats for the small tiles) instead of 2^29:
(1) the construction invariants of every view kind at every tile shape the GPU file uses - which maps contain which
boundary, alignment, no overlap between placed maps, the arena all zero after restore, the twin's properties;
(2) gather(), the numpy model of the addressing, scored by the fp32 oracle passes the checking function the GPU test
uses, and each of the three 32-bit truncations of the offset ("s32_bytes", "u32_bytes", "i32_elems") is caught by it
for every view kind that reaches the boundary at which that truncation first changes an offset. A checker that lets
such a mutant through fails here."""
import numpy as np
import pytest
import torch

import far_views as fv
from oracle import dct_oracle as orc

SHAPE_KINDS = fv.all_shape_kinds()
IDS = ["%dx%d-%s-%dB" % sk for sk in SHAPE_KINDS]


def specs_of(h, w, kind, esize):
    return fv.build(kind, h, w, fv.cpu_unit(h, w), esize)


def arena_for(specs, esize):
    n = max(fv.extent(s) for s in specs) + 8
    return torch.zeros(n, dtype=torch.float32)


def np_arena(arena, esize):
    return arena.numpy() if esize == 4 else arena.view(torch.float16).numpy()


DT = {4: torch.float32, 2: torch.float16}


def test_the_gpu_unit_puts_the_boundaries_at_2_gib_4_gib_and_2_pow_31_elements():
    s = fv.far_n(8, 8, fv.GPU_UNIT)
    assert [b * 4 for b in s.bounds[:2]] == [1 << 31, 1 << 32] and s.bounds[2] == 1 << 31
    h = fv.far_n(8, 8, fv.GPU_UNIT, esize=2)
    assert [b * 2 for b in h.bounds] == [1 << 31, 1 << 32, 1 << 33] and h.bounds[1] == 1 << 31
    assert fv.arena_elems(fv.GPU_UNIT) * 4 == (8 << 30) + (128 << 20)
    # every GPU case fits the arena and touches less than 256 MiB
    for hh, ww, kind, esize in SHAPE_KINDS:
        for sp in fv.build(kind, hh, ww, fv.GPU_UNIT, esize):
            for v in (sp, fv.twin(sp)):
                assert fv.extent(v) <= fv.arena_elems(fv.GPU_UNIT), (hh, ww, kind)
                assert v.shape[0] * v.p_count * hh * ww * esize < 256 << 20, (hh, ww, kind)
            assert v.c_begin + v.c_count < 1 << 31


@pytest.mark.parametrize("h,w,kind,esize", SHAPE_KINDS, ids=IDS)
def test_construction_invariants(h, w, kind, esize):
    for unit in (fv.cpu_unit(h, w), fv.GPU_UNIT):
        for s in fv.build(kind, h, w, unit, esize):
            b0, b1, b2 = s.bounds
            n, c, _, _ = s.shape
            sn, sc, sh = s.strides
            assert fv.no_overlap(s) and fv.no_overlap(fv.twin(s))
            assert fv.assert_reach(s, fv.expected_reach(s)) == fv.expected_reach(s)
            assert 0 <= s.p_begin <= s.c_begin and s.c_begin + s.c_count <= s.p_begin + s.p_count <= c
            off = fv.map_offsets(s)
            if kind in ("far-N", "slice"):
                assert n == 5 and sc == h * w and sh == w and sn % 4 == 0 and sn != s.c_count * sc
                for smp, b in ((1, b0), (2, b1), (4, b2)):  # sample smp holds boundary b inside a scored map, not at its start
                    hit = fv.maps_containing(s, b)
                    assert hit.sum() == 1 and hit[smp].sum() == 1 and off[smp, 0] < b
                    if h * w > 4:
                        assert off[hit][0] < b  # strictly inside the map as well
                if kind == "slice":
                    assert s.c_begin > 0 and s.c_count < c and s.p_count == c
            elif kind.startswith("far-C"):
                assert n == 1 and sc >= 4 * h * w and sc & (sc - 1) == 0 and c == 4 * s.eunit // sc + 3 and sh == w
                for b in s.bounds:  # a channel starts at every boundary
                    assert off[0, b // sc] == b
                assert (off[0, -3:] >= b2).all() and s.base == (0 if kind == "far-C" else 1)
            elif kind == "far-H":
                assert n == 1 and c == 2 and h >= 33 and sh == s.eunit // 16 and sc >= w and sc != h * w
                assert off[0, 0] + 16 * sh == b0 and off[0, 0] + 32 * sh == b1
            else:  # far-D
                k = int(s.kind[-1])
                assert n == 1 and sc == h * w and sh == w and s.p_begin == s.c_begin - 1 and s.p_count == s.c_count + 2
                hit = fv.maps_containing(s, s.bounds[k])
                assert hit.sum() == 1 and hit[0, 1]
            # the twin: same shape, same branches, small
            t = fv.twin(s)
            assert t.shape[2:] == s.shape[2:] and t.shape[0] == n and t.c_count == s.c_count and t.base == s.base
            assert (t.strides[1] == h * w) == (sc == h * w) and (t.strides[2] == w) == (sh == w)
            assert (t.c_begin * t.strides[1]) % 4 == (s.c_begin * sc) % 4 and (t.c_begin > 0) == (s.c_begin > 0)
            assert (n == 1 or t.strides[0] != t.c_count * t.strides[1]) and t.strides[0] % 4 == sn % 4
            if unit == fv.GPU_UNIT:
                assert fv.extent(t) * 4 <= 256 << 20 and not fv.reached_bounds(t)


@pytest.mark.parametrize("h,w,kind,esize", SHAPE_KINDS, ids=IDS)
def test_checker_passes_the_model_and_catches_every_truncation(h, w, kind, esize):
    specs = specs_of(h, w, kind, esize)
    arena = arena_for(specs + [fv.twin(s) for s in specs], esize)
    caught = set()
    for i, s in enumerate(specs):
        maps = fv.make_maps(s, 100 * h + w + i, DT[esize])
        flat = maps.float().reshape(-1, h, w)
        norms = flat.flatten(1).norm(dim=1)
        dead = norms == 0
        assert dead.sum() >= 1 or len(flat) <= fv.DEAD_AT
        live = norms[~dead]
        assert live.unique().numel() == live.numel()  # every placed map distinct
        if live.numel() >= 32:
            assert live.max() / live.min() >= 30  # scales spread over about two decades

        def score(spec, wrap=None):
            fv.place(arena, spec, maps)
            x = torch.from_numpy(fv.gather(np_arena(arena, esize), spec, wrap))
            assert fv.restore(arena, spec, DT[esize])
            bad = ~torch.isfinite(x).flatten(2).all(-1)
            e = orc.energy_nc_batched(torch.nan_to_num(x))
            e[bad] = float("nan")
            return e

        got, got_twin = score(s), score(fv.twin(s))
        assert np.array_equal(fv.gather(np_arena(arena, esize), s), np.zeros((s.shape[0], s.c_count, h, w), np.float32))
        worst, tol = fv.check_energies(s, maps, got, got_twin, fv.expected_reach(s))
        assert worst <= tol
        for wrap in fv.WRAPS:
            if not fv.reaches(s, wrap):
                continue
            mutant = score(s, wrap)
            with pytest.raises(AssertionError):  # the float64 comparison alone catches it ...
                fv.check_energies(s, maps, mutant, None, fv.expected_reach(s))
            with pytest.raises(AssertionError):  # ... and so does the twin alone
                fv.assert_bitwise(mutant, got_twin, s)
            caught.add(wrap)
    assert not arena.any()  # every case put its zeros back
    # every truncation is exercised by every kind that reaches its boundary: far-H stops short of 2^31 fp32 elements
    want = set(fv.WRAPS) - ({"i32_elems"} if kind == "far-H" and esize == 4 else set())
    assert caught == want, (caught, want)


def test_rank_contents_have_the_ranks_they_claim():
    import rank_oracle as ro
    s = fv.far_n(13, 22, fv.cpu_unit(13, 22))
    maps = fv.make_maps(s, 3, content="rank")
    r = ro.rank_nc(maps).reshape(-1)
    want = torch.tensor([0.0 if i % fv.DEAD_EVERY == fv.DEAD_AT else 1.0 + (5 * i) % 13 for i in range(r.numel())])
    assert torch.equal(r, want) and not ro.undecidable(maps).any()
