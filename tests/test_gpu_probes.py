"""Every energy kernel family per coefficient and per sample, at fp32 accuracy (tests/dct_probes.py holds the
probes and the tolerance rule; tests/test_probes_cpu.py shows that the reference meets it and that the older
1e-4 rule misses the defects these probes catch).

For every (family, shape): basis sweep and impulse sweep over cover() (thousands of maps in one launch: looping
workgroups, short last groups and chunked workspaces on the way), random maps unsigned and signed with a prime
map count, power-of-two scaling bit for bit, NaN / inf isolation between maps.

| family (algo)                         | shapes                                                              | cover                                  |
|---------------------------------------|---------------------------------------------------------------------|----------------------------------------|
| CODELET, PREFETCH (even), LANE (7, 9) | the 22 codelet sizes                                                | exhaustive                             |
| RECT                                  | every square edge 1 ... 64, the RECT pairs, two crops, strideH > W  | exhaustive                             |
| SPLIT                                 | SPLIT + SPLIT_MORE, 48 edges                                        | exhaustive <= 128, k = 8 above         |
| FUSED, PIPE, TILE2D                   | their own lists (12, 2, 8 edges)                                    | exhaustive <= 128, k = 8 above         |
| DIRECT                                | 3, 5, 13, 22 exhaustive; 72 and 80                                  | k = 4 at 72 and 80                     |
| DIRECT, one edge beyond 256           | (260, 9), (9, 260), (512, 3), (3, 512)                              | exhaustive                             |
| DIRECT, where no other kernel goes    | 65, 264, 512 square; (260, 264)                                     | exhaustive at 65, k = 8 above          |
| AUTO -> the cosine-matrix kernel      | 72 x 72 with strideH = 79, 72 x 72 channel slice of N = 2, (100, 72)| exhaustive (edges <= 128)              |
| AUTO, pad_front_if_odd                | 7, 9, 13, 63, 65, 71, 73, 79, 143, 159, 287: impulse sweep, random  | the padded tile has no free first row  |

k counts the seeded random indices per axis on top of the eight fixed ones; what the residues mod 8 need is never
cut. Nothing had to be shrunk for run time: the whole file takes about twelve seconds on an MI355X (512 x 512 with its 16 128
maps of 1 MiB per sweep: one second).
Coefficients (dpa.dct2d) over the same cover for CODELET, RECT, FUSED, TILE2D and DIRECT (<= 64, 65, 72 and the four shapes
with one edge beyond 256). H = 511, W = 512 under the odd pad (W' = 513) is refused with code -2."""
import pytest
import torch

import dct_pruning_amd as dpa
import dct_probes as dp
from dct_pruning_amd._lib import DctScoreError
from test_gpu_parity import CODELET, DIRECT_ONLY, FUSED, PIPE, RECT, SPLIT, SPLIT_MORE, TILE2D, TILE2G

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 512 << 20   # well under the 1 GiB the probes allow: the float64 rows of the generators come on top
RANDOM_MAPS = 61    # prime: not a multiple of any group size (2, 3, 4 maps per round, 64 lanes, 4 maps per wave ...)
PAD_EDGES = [7, 9, 13, 63, 65, 71, 73, 79, 143, 159, 287]  # 65 -> 66 and 73 -> 74: not in the split table, so the cosine-matrix kernel
CROPS = [(56, 56), (9, 18)]
_tol_cache = {}


def algo_fn(algo, **kw):
    return lambda x: dpa.energy_nc(x, algo=getattr(dpa, "ALGO_" + algo), **kw)


def cached_tol(kind, h, w, make, pairs, **kw):
    key = (kind, h, w, tuple(sorted(kw.items())))
    if key not in _tol_cache:
        _tol_cache[key] = dp.sweep_tolerance(make, pairs, h, w, **kw)
    return _tol_cache[key]


def probe(family, energy_fn, h, w, pairs, basis=True, **ref_kw):
    """All probes of one (family, shape); prints what it measured (pytest -s)."""
    sweeps = [("impulse", lambda p: dp.impulse_maps(h, w, p, seed=h + 3 * w, device=DEV))]
    if basis:
        sweeps.insert(0, ("basis", lambda p: dp.basis_maps(h, w, p, device=DEV)))
    for what, make in sweeps:
        tol, e_ref = cached_tol(what, h, w, make, pairs, **ref_kw)
        worst = dp.sweep(energy_fn, make, pairs, h, w, tol, what, chunk_bytes=CHUNK)
        print("PROBE %s %dx%d %s maps=%d E_ref=%.3g tol=%.3g worst=%.3g" % (family, h, w, what, len(pairs), e_ref, tol, worst))
    for signed in (False, True):
        x = dp.random_maps(1, RANDOM_MAPS, h, w, 40 + h + w, signed=signed, device=DEV)
        key = ("signed" if signed else "unsigned", h, w, tuple(sorted(ref_kw.items())))
        if key not in _tol_cache:
            e_ref = dp.reference_error(x[:, :max(8, min(RANDOM_MAPS, dp.SUBSAMPLE_BYTES // (h * w * 4)))], **ref_kw)
            _tol_cache[key] = (dp.tolerance(e_ref), e_ref)
        tol, e_ref = _tol_cache[key]
        worst = dp.check_energy(energy_fn, x, tol, what="signed" if signed else "unsigned")
        print("PROBE %s %dx%d %s E_ref=%.3g tol=%.3g worst=%.3g" % (family, h, w, key[0], e_ref, tol, worst))
    dp.check_pow2_scaling(energy_fn, x)
    dp.check_isolation(energy_fn, x)


def coefficients(family, coeff_fn, h, w, pairs):
    peak, leak = dp.check_coefficients(coeff_fn, h, w, pairs, device=DEV, chunk_bytes=CHUNK)
    print("PROBE %s %dx%d coefficients maps=%d peak=%.3g leak=%.3g" % (family, h, w, len(pairs), peak, leak))


SMALL = [("CODELET", n) for n in CODELET] + [("PREFETCH", n) for n in CODELET if n % 2 == 0] + [("LANE", n) for n in (7, 9)]


@pytest.mark.parametrize("algo,n", SMALL)
def test_codelet_families(algo, n):
    probe(algo, algo_fn(algo), n, n, dp.cover(n, n))


RECT_SHAPES = [(n, n) for n in range(1, 65)] + [hw for hw in RECT if hw[0] != hw[1]]


@pytest.mark.parametrize("hw", RECT_SHAPES)
def test_rect(hw):
    h, w = hw
    probe("RECT", algo_fn("RECT"), h, w, dp.cover(h, w))


@pytest.mark.parametrize("hw", CROPS)
def test_rect_crops_with_a_row_pitch(hw):
    """A spatial crop of a wider tensor (strideH > W), the surrounding samples non-zero: a sample read from outside
    the crop shows in the impulse sweep."""
    h, w = hw

    def crop_energy(x):
        base = torch.full((x.shape[0], x.shape[1], h + 5, w + 7), 3.0, device=x.device)
        view = base[:, :, 2:2 + h, 3:3 + w]
        view.copy_(x)
        assert view.stride(2) == w + 7 and not view.is_contiguous()
        return dpa.energy_nc(view)

    probe("RECT-crop", crop_energy, h, w, dp.cover(h, w))


@pytest.mark.parametrize("n", SPLIT + SPLIT_MORE)
def test_split(n):
    probe("SPLIT", algo_fn("SPLIT"), n, n, dp.cover(n, n))


@pytest.mark.parametrize("algo,n", [("FUSED", n) for n in FUSED] + [("PIPE", n) for n in PIPE] + [("TILE2D", n) for n in TILE2G + TILE2D])
def test_single_launch_large_tiles(algo, n):
    probe(algo, algo_fn(algo), n, n, dp.cover(n, n))


DIRECT = [n for n in DIRECT_ONLY if n <= 64] + [72, 80]


@pytest.mark.parametrize("n", DIRECT)
def test_direct(n):
    probe("DIRECT", algo_fn("DIRECT"), n, n, dp.cover(n, n, 4, exhaustive=n <= 64))


# One edge beyond 256 (the 256-thread loops over c and l take a second trip, the basis block fills more than 256 rows and,
# at 512, its last row), the other tiny; 260 and 3 leave a short last block of 8 output rows. All u x all v.
DIRECT_LONG = [(260, 9), (9, 260), (512, 3), (3, 512)]
# Squares no other kernel takes (65 is the smallest) or at the far end of the table, and both edges beyond 256, non-square.
DIRECT_LARGE = [(65, 65), (264, 264), (260, 264), (512, 512)]


@pytest.mark.parametrize("hw", DIRECT_LONG)
def test_direct_one_long_edge(hw):
    h, w = hw
    probe("DIRECT", algo_fn("DIRECT"), h, w, dp.cover(h, w, exhaustive=True))


@pytest.mark.parametrize("hw", DIRECT_LARGE)
def test_direct_large(hw):
    h, w = hw
    probe("DIRECT", algo_fn("DIRECT"), h, w, dp.cover(h, w))


def test_auto_large_crop_with_a_row_pitch():
    """72 x 72 is a tile2g shape, but rows with a pitch (strideH = 79) leave the cosine-matrix kernel; the surrounding
    samples are non-zero, so a sample read from outside the crop shows in the impulse sweep."""
    h = w = 72

    def crop_energy(x):
        base = torch.full((x.shape[0], x.shape[1], h + 5, w + 7), 3.0, device=x.device)
        view = base[:, :, 2:2 + h, 3:3 + w]
        view.copy_(x)
        assert view.stride(2) == 79 and not view.is_contiguous()
        return dpa.energy_nc(view)

    probe("AUTO-crop", crop_energy, h, w, dp.cover(h, w))


def test_auto_large_channel_slice_of_two_samples():
    """Channels 2 ... C - 2 of an N = 2 tensor: the slice is not contiguous, so 72 x 72 leaves the large-tile families.
    Sample 1 holds the maps of sample 0 in reverse order and every channel outside the slice holds 3.0: a sample or
    channel stride gone wrong shows as another map's energy."""
    h = w = 72

    def slice_energy(x):
        p = x.shape[1]
        big = torch.full((2, p + 3, h, w), 3.0, device=x.device)
        big[0, 2:2 + p] = x[0]
        big[1, 2:2 + p] = x[0].flip(0)
        got = dpa.energy_nc(big, c_begin=2, c_count=p)
        assert tuple(got.shape) == (2, p)
        assert torch.equal(got[0].view(torch.int32), got[1].flip(0).view(torch.int32)), "sample 1 is sample 0 reversed"
        return got[:1]

    probe("AUTO-slice", slice_energy, h, w, dp.cover(h, w))


def test_auto_large_non_square():
    """(100, 72): no family but the cosine-matrix kernel takes a non-square map with an edge beyond 64."""
    h, w = 100, 72
    probe("AUTO-nonsquare", lambda x: dpa.energy_nc(x), h, w, dp.cover(h, w))
    for signed in (False, True):
        x = dp.random_maps(2, RANDOM_MAPS, h, w, 7, signed=signed, device=DEV)
        auto, direct = dpa.energy_nc(x), dpa.energy_nc(x, algo=dpa.ALGO_DIRECT)
        assert torch.equal(auto.view(torch.int32), direct.view(torch.int32))


def test_padded_edge_513_is_refused():
    """H = 511 is odd: the front pad makes the tile 512 x 513, one column beyond DCTS_MAX_EDGE."""
    x = torch.zeros(1, 1, 511, 512, device=DEV)
    assert dpa.energy_nc(x, algo=dpa.ALGO_DIRECT).item() == 0.0  # without the pad the map is in range
    for algo in (dpa.ALGO_AUTO, dpa.ALGO_DIRECT):
        with pytest.raises(DctScoreError) as e:
            dpa.energy_nc(x, pad_front_if_odd=True, algo=algo)
        assert e.value.code == -2


@pytest.mark.parametrize("n", PAD_EDGES)
def test_auto_with_the_odd_front_pad(n):
    probe("AUTO-pad", lambda x: dpa.energy_nc(x, pad_front_if_odd=True), n, n, dp.cover(n, n),
          basis=False, pad_front_if_odd=True)


COEFF = ([("CODELET", n, n) for n in CODELET] + [("RECT", h, w) for h, w in RECT_SHAPES] + [("FUSED", n, n) for n in FUSED]
         + [("TILE2D", n, n) for n in TILE2G + TILE2D] + [("DIRECT", n, n) for n in DIRECT if n <= 64]
         + [("DIRECT", h, w) for h, w in [(65, 65), (72, 72)] + DIRECT_LONG])


@pytest.mark.parametrize("algo,h,w", COEFF)
def test_coefficients(algo, h, w):
    coefficients(algo, lambda x: dpa.dct2d(x, algo=getattr(dpa, "ALGO_" + algo)), h, w, dp.cover(h, w))
