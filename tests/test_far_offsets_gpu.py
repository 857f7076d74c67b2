"""Every kernel family and entry point on views whose elements lie beyond byte offset 2^31, byte offset 2^32 and element
index 2^31 from the tensor's base pointer (tests/far_views.py describes the views; tests/test_far_offsets_cpu.py shows that
the checks used here catch each 32-bit truncation of an offset).

The module allocates ONE zero-filled arena of 2^31 + 2^25 floats (8.125 GiB; no skip when that fails) and every case
writes its maps into it through an as_strided view, calls the entry point on that view, and writes zeros back. Per case:
  (a) accuracy against float64 on the compact CPU copy of the same maps: energies within dct_probes' bound
      tolerance(reference_error(x)) with exactly +0.0 for all-zero maps, coefficients / weighted / band / rank
      outputs within the bounds of their own GPU tests (2e-6 of the coefficient scale; rtol 2e-5, atol 1e-6 max;
      test_bands_gpu._tol; equality on decidable maps);
  (b) bit for bit the result of a twin view: the same shape, N == 1 or not, strideC == H W or not, strideH == W or not,
      base address mod 16, c_begin alignment and c_count, at small strides near the arena's start;
  (c) the places written read as zero after the restore, and the whole arena is zero at module teardown;
(energy_multi / energy_mixed: the list call on all far items, the list call on the twins of all items, and one
energy_nc call per item on either, all four bit for bit the same per item);
and every case asserts that a checked map lies beyond each boundary its kind of view reaches.

The families for arrays of dense tiles (PREFETCH, SPLIT, FUSED, PIPE, TILE2D; the large-tile coefficient path) refuse
far-N, far-C and the slice with DCTS_E_UNSUPPORTED - asserted here - and AUTO scores those views with the cosine-matrix
kernel; the far view they accept is far-D, a dense tensor scored from a c_begin beyond each boundary in turn."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import dct_pruning_amd as dpa
import far_views as fv
from dct_pruning_amd import bands
from dct_pruning_amd._lib import DctScoreError
from oracle import dct_oracle as orc

pytestmark = pytest.mark.gpu

UNIT = fv.GPU_UNIT
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
ANY_VIEW = ("CODELET", "LANE", "RECT", "DIRECT")  # families that take strided samples and pitched channels
COEFF_TOL = 2e-6  # tests/test_gpu_parity.py, tests/test_gpu_coeff_large.py: of the coefficient scale


@pytest.fixture(scope="module")
def arena():
    a = torch.zeros(fv.arena_elems(UNIT), dtype=torch.float32, device="cuda")
    yield a
    step = 1 << 28
    dirty = [i for i in range(0, a.numel(), step) if bool(a[i:i + step].any())]
    del a
    torch.cuda.empty_cache()
    assert not dirty, "the arena is not all zero at teardown: floats from %s on" % dirty


def on_view(arena, s, maps_dev, fn):
    """Place, call, restore: fn(view, spec)'s result on the CPU. The restore runs whatever fn does."""
    v = fv.place(arena, s, maps_dev)
    try:
        assert torch.equal(v[-1, s.c_begin + s.c_count - 1], fv.scored(s, maps_dev)[-1, -1])  # the farthest map is where it belongs
        out = fn(v, s)
        out = tuple(o.cpu() for o in out) if isinstance(out, tuple) else out.cpu()
    finally:
        clean = fv.restore(arena, s, maps_dev.dtype)
    assert clean, "%s: the places written do not read as zero after the restore" % s.kind
    return out


def far_and_twin(arena, s, maps, fn):
    dev = maps.cuda()
    return on_view(arena, s, dev, fn), on_view(arena, fv.twin(s), dev, fn)


def or_auto(call, algo, s):
    """call(algo) where the family takes the view; where it takes arrays of dense tiles only and the view is not one,
    the refusal is asserted and AUTO scores the view."""
    if algo == "AUTO" or algo in ANY_VIEW or "far-D" in s.kind:
        return call(getattr(dpa, "ALGO_" + algo))
    with pytest.raises(DctScoreError) as ei:
        call(getattr(dpa, "ALGO_" + algo))
    assert ei.value.code == -6  # DCTS_E_UNSUPPORTED
    return call(dpa.ALGO_AUTO)


def flat_cases(table):
    return [row[:-1] + (kind,) for row in table for kind in row[-1]]


def run_energy(arena, algo, h, w, kind, pad=False, seed=0, witness=None):
    """witness: an explicit family that must give the bits of `algo` on the same view - it names the kernel AUTO ran (the
    family either runs its own kernel or refuses)."""
    kw = {"pad_front_if_odd": True} if pad else {}

    def fn(v, sp):
        out = or_auto(lambda a: dpa.energy_nc(v, sp.c_begin, sp.c_count, pad, algo=a), algo, sp)
        if witness:
            assert torch.equal(out, dpa.energy_nc(v, sp.c_begin, sp.c_count, pad, algo=getattr(dpa, "ALGO_" + witness)))
        return out

    for s in fv.build(kind, h, w, UNIT):
        maps = fv.make_maps(s, seed + 7 * h + w)
        got, got_twin = far_and_twin(arena, s, maps, fn)
        worst, tol = fv.check_energies(s, maps, got, got_twin, fv.expected_reach(s), **kw)
        print("FAR %s %dx%d %s pad=%d maps=%d worst=%.3g tol=%.3g" % (algo, h, w, s.kind, pad, got.numel(), worst, tol))


@pytest.mark.parametrize("algo,h,w,kind", flat_cases(fv.ENERGY_CASES))
def test_energy_families(arena, algo, h, w, kind):
    run_energy(arena, algo, h, w, kind)


@pytest.mark.parametrize("n,kind", flat_cases(fv.PAD_CASES))
def test_auto_with_the_odd_front_pad(arena, n, kind):
    """7 and 9: the padded codelet kernels; 71 dense (far-D): tile2g_pad, whose buffer resource starts in front of the
    map's base - the bits of an explicit TILE2D request, which has no other kernel for a padded 71 x 71 map."""
    run_energy(arena, "AUTO", n, n, kind, pad=True, seed=1, witness="TILE2D" if (n, kind) == (71, "far-D") else None)


@pytest.mark.parametrize("algo,n,kind", flat_cases(fv.COEFF_CASES))
def test_coefficients(arena, algo, n, kind):
    for s in fv.build(kind, n, n, UNIT):
        maps = fv.make_maps(s, 2 + n)
        fn = lambda v, sp: or_auto(lambda a: dpa.dct2d(v, sp.c_begin, sp.c_count, algo=a), algo, sp)
        got, got_twin = far_and_twin(arena, s, maps, fn)
        fv.assert_reach(s, fv.expected_reach(s))
        ref = orc.dct_2d_f64(fv.scored(s, maps).numpy())
        err, scale = np.abs(got.numpy() - ref).max(), np.abs(ref).max()
        print("FAR dct2d %s %d %s maps=%d err=%.3g of %.3g" % (algo, n, s.kind, ref.shape[0] * ref.shape[1], err, scale))
        assert got.shape == ref.shape and err <= COEFF_TOL * scale
        fv.assert_bitwise(got, got_twin, s, "coefficient")


@pytest.mark.parametrize("n,kind", flat_cases(fv.WEIGHTED_CASES))
def test_weighted_energy(arena, n, kind):
    """The host walks the samples (x + n * strideN) and runs of channels; 72 dense-square views take the large-tile
    coefficient path per sample."""
    g = torch.Generator().manual_seed(n)
    wts = torch.rand(n, n, generator=g)
    wd = wts.cuda()
    for s in fv.build(kind, n, n, UNIT):
        maps = fv.make_maps(s, 3 + n)
        fn = lambda v, sp: dpa.weighted_energy_nc(v, wd, sp.c_begin, sp.c_count)
        got, got_twin = far_and_twin(arena, s, maps, fn)
        fv.assert_reach(s, fv.expected_reach(s))
        ref = orc.weighted_energy_nc_f64(fv.scored(s, maps), wts.numpy())
        print("FAR weighted %d %s maps=%d worst=%.3g" % (n, s.kind, ref.size, np.abs(got.numpy() - ref).max() / ref.max()))
        assert np.allclose(got.numpy(), ref, rtol=2e-5, atol=1e-6 * ref.max())  # tests/test_gpu_coeff_large.py
        assert (got[torch.from_numpy(ref == 0)] == 0).all()
        fv.assert_bitwise(got, got_twin, s, "weighted energy")


@pytest.mark.parametrize("algo,h,w,kind", flat_cases(fv.BAND_CASES))
def test_band_energy(arena, algo, h, w, kind):
    """K = 4: the fused kernel at 14 and 56, the fallback (coefficients of a chunk of maps, then one reduction) at 72 and
    56 x 28."""
    import band_oracle as bo
    from test_bands_gpu import _tol
    assert dpa.has_band_kernel(h, w) == (algo == "CODELET")
    wts = torch.from_numpy(bands.partition(h, w, 4, "square"))
    wd = wts.cuda()
    for s in fv.build(kind, h, w, UNIT):
        maps = fv.make_maps(s, 4 + h)
        fn = lambda v, sp: dpa.band_energy_nc(v, wd, sp.c_begin, sp.c_count, algo=getattr(dpa, "ALGO_" + algo))
        got, got_twin = far_and_twin(arena, s, maps, fn)
        fv.assert_reach(s, fv.expected_reach(s))
        x = fv.scored(s, maps).contiguous()
        tol, e_ref = _tol(x, wts)
        err = bo.band_error(got, x, wts)
        print("FAR bands %s %dx%d %s maps=%d worst=%.3g E_ref=%.3g tol=%.3g" % (algo, h, w, s.kind, x.shape[0] * x.shape[1], err, e_ref, tol))
        assert err <= tol
        dead = x.flatten(2).abs().amax(-1) == 0
        assert (got[dead] == 0).all() and not torch.signbit(got[dead]).any()
        fv.assert_bitwise(got, got_twin, s, "band energy")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("h,w,kind", flat_cases(fv.HALF_CASES))
def test_half_precision_maps(arena, h, w, kind, dt):
    """2-byte elements: the byte boundaries fall at 2, 4 and 8 unit elements. Native kernel at 2, 7 and 56; staged at 20
    and at a pitched 56 (far-H)."""
    dtype = DTYPES[dt]
    assert dpa.has_half_kernel(h, w) == (h != 20)
    for s in fv.build(kind, h, w, UNIT, esize=2):
        maps = fv.make_maps(s, 5 + h, dtype)
        fn = lambda v, sp: dpa.energy_nc(v, sp.c_begin, sp.c_count)
        got, got_twin = far_and_twin(arena, s, maps, fn)
        worst, tol = fv.check_energies(s, maps, got, got_twin, fv.expected_reach(s))
        print("FAR %s %dx%d %s maps=%d worst=%.3g tol=%.3g" % (dt, h, w, s.kind, got.numel(), worst, tol))


@pytest.mark.parametrize("h,w,kind", flat_cases(fv.RANK_CASES))
def test_rank(arena, h, w, kind):
    import rank_oracle as ro
    for s in fv.build(kind, h, w, UNIT):
        maps = fv.make_maps(s, 6 + h, content="rank")
        fn = lambda v, sp: dpa.rank_nc(v, sp.c_begin, sp.c_count)
        got, got_twin = far_and_twin(arena, s, maps, fn)
        fv.assert_reach(s, fv.expected_reach(s))
        x = fv.scored(s, maps)
        ref, ok = ro.rank_nc(x), ~ro.undecidable(x)
        assert ok.float().mean().item() >= 0.99 and ref.unique().numel() >= min(ref.numel(), min(h, w)) // 2
        assert torch.equal(got[ok], ref[ok]), (got - ref)[ok].abs().max()
        fv.assert_bitwise(got, got_twin, s, "rank")


# ----------------------------------------------------------------------------------------------------
# several tensors per call
# ----------------------------------------------------------------------------------------------------
def rows_do_not_overlap(specs):
    rows = []
    for s in specs:
        h, w = s.shape[2], s.shape[3]
        r = fv.map_offsets(s, True)[:, :, None] + (np.arange(h, dtype=np.int64) * s.strides[2])[None, None] + s.base
        rows.append(np.stack([r.reshape(-1), r.reshape(-1) + w], 1))
    rows = np.concatenate(rows)
    rows = rows[np.argsort(rows[:, 0])]
    return bool((rows[1:, 0] >= rows[:-1, 1]).all())


def item_specs(edges, count, spacing):
    """`count` far views at arena offsets `spacing` apart: far-N, far-C and the channel slice in turn, edges in turn."""
    out = []
    for i in range(count):
        n = edges[i % len(edges)]
        build = (fv.far_n, fv.far_c, fv.slice_n)[i % 3]
        out.append(replace(build(n, n, UNIT), base=i * spacing))
    return out


def dense_far_items(n, count=5):
    """Three dense [1, count, n, n] tensors whose BASE POINTERS lie beyond the three boundaries (256, 512 and 768 maps
    beyond them, clear of the views of item_specs): what the families for arrays of dense tiles batch into one launch."""
    out = []
    for k in range(3):
        d = fv.far_d(n, n, UNIT, k, count=count)
        out.append(replace(d, kind="dense@%d" % k, base=(d.c_begin + 256 * (k + 1)) * n * n, shape=(1, count, n, n),
                           strides=(count * n * n, n * n, n), c_begin=0, p_begin=0, p_count=count))
    assert [s.base > b for s, b in zip(out, out[0].bounds)] == [True] * 3
    return out


def twin_items(specs):
    """The twin of every item, one behind the other from the arena's start (16-byte steps: the base alignment of every
    item, a multiple of 16 bytes, is kept). A dense@k item is its own twin at a small base."""
    out, at = [], 0
    for s in specs:
        assert s.base % 4 == 0
        t = replace(s, kind="twin of " + s.kind) if s.kind.startswith("dense@") else fv.twin(s)
        t = replace(t, base=at)
        out.append(t)
        at = (fv.extent(t) + 3) // 4 * 4 + 4
    assert not any(fv.reached_bounds(replace(t, base=0)) for t in out) and at < UNIT // 4  # all of them far below the first boundary
    return out


def score_items(arena, specs, dev, call, single):
    """All items placed at once: (the list entry point's outputs, one call of `single` per item), on the CPU."""
    assert rows_do_not_overlap(specs) and all(fv.extent(s) <= fv.arena_elems(UNIT) for s in specs)
    try:
        views = [fv.place(arena, s, d) for s, d in zip(specs, dev)]
        outs = [o.cpu() for o in call(views, specs)]
        alone = [single(v, s).cpu() for v, s in zip(views, specs)]
    finally:
        clean = [fv.restore(arena, s) for s in specs]
    assert all(clean)
    return outs, alone


def run_items(arena, specs, call, single):
    """(a) every item against float64, (b) the list entry point on the twins of all items bit for bit, and the bits of
    one call per tensor on the far views and on the twins."""
    import dct_probes as dp
    maps = [fv.make_maps(s, 900 + i) for i, s in enumerate(specs)]
    dev = [m.cuda() for m in maps]
    outs, alone = score_items(arena, specs, dev, call, single)
    twins = twin_items(specs)
    t_outs, t_alone = score_items(arena, twins, dev, call, single)
    for s, m, got, one, t_got, t_one in zip(specs, maps, outs, alone, t_outs, t_alone):
        assert torch.equal(got, one) and torch.equal(t_got, t_one), s
        if s.kind.startswith("dense@"):  # far by its base pointer: the offsets from it are small
            x = fv.scored(s, m)
            dp.check_energy(lambda _: got, x, fv.energy_tolerance(x)[0], what=s.kind)
        else:
            fv.check_energies(s, m, got, None, fv.expected_reach(s))
        fv.assert_bitwise(got, t_got, s, "energy")


def multi(views, specs):
    return dpa.energy_multi([(v, s.c_begin, s.c_count) for v, s in zip(views, specs)])


def mixed(views, specs):
    return dpa.energy_mixed([(v, s.c_begin, s.c_count, False) for v, s in zip(views, specs)])


def single(v, s):
    return dpa.energy_nc(v, s.c_begin, s.c_count)


def test_energy_multi_second_launch(arena):
    """35 tensors of 8 x 8 maps, every one a far view at its own arena offset: items 32 ... 34 land in the second launch."""
    specs = item_specs([8], 35, 4096)
    assert len(specs) > 32 and sum(s.kind == "slice" for s in specs) >= 1
    run_items(arena, specs, multi, single)


def test_energy_multi_large_tiles(arena):
    """72 x 72: far-N, far-C and the slice are not arrays of dense tiles and go tensor by tensor; three dense tensors whose
    base pointers lie beyond the three boundaries share one tile2g launch."""
    run_items(arena, item_specs([72], 3, 1 << 17) + dense_far_items(72), multi, single)


def test_energy_mixed_second_launch(arena):
    """50 tensors with tiles of edge 2, 4, 8, 16 and 32 (one launch per 48) and two of 7 x 7 (grouped by shape): far views
    throughout, so the second launch scores far items as well."""
    specs = item_specs([2, 4, 8, 16, 32], 50, 1 << 15) + item_specs([7], 52, 1 << 15)[50:]
    assert len(specs) > 48
    run_items(arena, specs, mixed, single)
