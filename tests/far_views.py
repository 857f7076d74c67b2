"""Views whose elements lie beyond 2 GiB, 4 GiB and 2^31 elements from the tensor's base pointer.

One description of a "far view" serves the GPU tests (tests/test_far_offsets_gpu.py) and a CPU self-check
(tests/test_far_offsets_cpu.py). Everything is parameterised by `unit`, counted in fp32 elements: 2^29 on the GPU
(2 GiB), cpu_unit(h, w) on the CPU. The three boundaries a 32-bit register breaks at are

    unit      byte offset 2^31: a signed 32-bit byte offset goes negative            wrap="s32_bytes"
    2 unit    byte offset 2^32: an unsigned 32-bit byte offset wraps                 wrap="u32_bytes"
    4 unit    element index 2^31: an int element index overflows (fp32)              wrap="i32_elems"

For 2-byte elements the same byte boundaries fall at 2, 4 and 8 unit ELEMENTS (and the element index overflows at
4 unit elements, where the unsigned byte offset wraps). A Spec counts in elements of its own type: eunit = unit * 4 / esize.

The arena is one zero-filled 1-D fp32 tensor of arena_elems(unit) elements (4 unit + slack). Cases write their maps
into it through as_strided views (place) and write zeros back to exactly those places (restore). Kinds of view:

    far-N    [5, C, H, W], dense maps, strideN = eunit - q: samples 1, 2 and 4 contain the three boundaries
    far-C    [1, C, H, W], channel pitch P (a power of two >= 4 H W): channels eunit / P, 2 eunit / P, 4 eunit / P start at
             the boundaries, the last three maps lie wholly beyond the third; also on a base that is only 4-byte aligned
    far-H    [1, 2, H, W], strideH = eunit / 16, H >= 33: rows 16 and 32 sit at the first two boundaries
    slice    a far-N view scored with c_begin > 0, c_count < C
    far-D    [1, C_total, H, W] DENSE (strideC = H W) scored with a c_begin that puts the scored maps at boundary k:
             the only far view the families for arrays of dense tiles accept (they refuse far-N and far-C); what is
             far is the host's x + c_begin * strideC and the absolute address, the kernel's own offsets stay small

WHAT FAR-D DOES NOT COVER. PREFETCH, SPLIT, FUSED, PIPE and TILE2D are handed x + c_begin * strideC by the host and see
five maps: their in-kernel map * map_elems arithmetic never comes near 2^31, so a 32-bit truncation of the MAP offset
inside fused*.hip, pipe.hip, tile2d.hip or tile2g.hip would still pass. Reaching it takes a dense tensor of 2^31
elements (8 GiB read per call), beyond what a case of this suite may touch; for these families the tests cover the host
arithmetic and absolute addresses beyond each boundary, not in-kernel offsets.

No product import: torch and numpy only, on either device.
"""
from dataclasses import dataclass, replace

import numpy as np
import torch

GPU_UNIT = 1 << 29
WRAPS = ("s32_bytes", "u32_bytes", "i32_elems")
FACTORS = (1, 2, 4)  # the boundaries in eunit


def pow2ceil(v):
    return 1 << max(0, int(v - 1).bit_length())


def cpu_unit(h, w):
    """The smallest unit at which every kind of view of an (h, w) tile exists without overlap."""
    return max(1 << 10, pow2ceil(32 * h * w))


def arena_elems(unit):
    """fp32 elements of the arena of the GPU tests: 4 unit + unit / 16 of slack (2^31 + 2^25 floats, 8.125 GiB at 2^29)."""
    return 4 * unit + unit // 16


@dataclass(frozen=True)
class Spec:
    kind: str
    unit: int            # fp32 elements
    esize: int           # bytes per element: 4, or 2 for fp16 / bf16
    base: int            # arena offset of the tensor's base pointer, in elements of esize
    shape: tuple         # (N, C_total, H, W) as the entry point is told
    strides: tuple       # (strideN, strideC, strideH) in elements; strideW == 1
    c_begin: int
    c_count: int
    p_begin: int         # channels [p_begin, p_begin + p_count) hold maps; the others are never written nor scored
    p_count: int

    @property
    def eunit(self):
        return self.unit * 4 // self.esize

    @property
    def bounds(self):
        return tuple(f * self.eunit for f in FACTORS)


def _r4(v):
    return (v + 3) // 4 * 4


# ----------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------
def far_n(h, w, unit, esize=4):
    """Dense maps, five samples eunit - q apart. q (a multiple of 4, about 1.4 maps) puts boundary k at q, 2 q and 4 q
    elements into samples 1, 2 and 4: strictly inside them, and inside a map wherever a map has more than 4 elements.
    C is large enough for 4 q."""
    eunit = unit * 4 // esize
    hw = h * w
    q = max(4, 4 * round(1.375 * hw / 4))
    c = 4 * q // hw + 3
    return Spec("far-N", unit, esize, 0, (5, c, h, w), (eunit - q, hw, w), 0, c, 0, c)


def far_c_pitch(h, w, unit, esize=4):
    """Channel pitch of far-C: a power of two >= 4 H W that leaves about 1024 channels (256 beyond edge 128) on the GPU,
    so that a case touches well under 256 MiB."""
    eunit = unit * 4 // esize
    return max(pow2ceil(4 * h * w), 4 * eunit // (1024 if max(h, w) <= 128 else 256))


def far_c(h, w, unit, esize=4, base=0):
    eunit = unit * 4 // esize
    p = far_c_pitch(h, w, unit, esize)
    c = 4 * eunit // p + 3
    return Spec("far-C" if base == 0 else "far-C+%d" % base, unit, esize, base, (1, c, h, w), (c * p, p, w), 0, c, 0, c)


def far_h(h, w, unit, esize=4):
    """Two channels whose rows interleave: row r of channel j at r * eunit / 16 + j * strideC."""
    assert h >= 33
    eunit = unit * 4 // esize
    sc = _r4(w) + 4
    return Spec("far-H", unit, esize, 0, (1, 2, h, w), (h * (eunit // 16), sc, eunit // 16), 0, 2, 0, 2)


def slice_n(h, w, unit, esize=4):
    """Channels [2, C - 1) of a far-N view whose q is two maps larger: the boundaries lie in maps 3, 6 and 13 of samples
    1, 2 and 4, so n * strideN + c_begin * strideC still crosses each of them inside a scored map. Every channel is
    placed: a slice that starts or ends one map off reads another map."""
    eunit = unit * 4 // esize
    hw = h * w
    q = max(4, 4 * round(3.375 * hw / 4))
    c = 4 * q // hw + 4
    return Spec("slice", unit, esize, 0, (5, c, h, w), (eunit - q, hw, w), 2, c - 3, 0, c)


def far_d(h, w, unit, k, esize=4, count=5):
    """A dense [1, C_total, h, w] tensor at the arena's start, scored from a c_begin that puts boundary k inside the
    second scored map (at its first element where h w divides the boundary). One map in front and one behind are
    placed as well, so a slice that is off by one map reads another map, not zeros."""
    eunit = unit * 4 // esize
    hw = h * w
    cb = FACTORS[k] * eunit // hw - 1
    return Spec("far-D%d" % k, unit, esize, 0, (1, cb + count + 1, h, w), ((cb + count + 1) * hw, hw, w), cb, count, cb - 1, count + 2)


def twin(s):
    """The same shape and the same value of everything a dispatcher or kernel branches on (N == 1 or not, strideC == H W
    or not, strideH == W or not, base address mod 16, c_count and the alignment of c_begin * strideC), at small strides
    near the arena's start: only addresses differ."""
    n, c, h, w = s.shape
    sn, sc, sh = s.strides
    if s.kind.startswith("far-D"):
        cb = 4 + s.c_begin % 4
        return replace(s, kind="twin of " + s.kind, shape=(1, cb + s.c_count + 1, h, w),
                       strides=((cb + s.c_count + 1) * h * w, sc, sh), c_begin=cb, p_begin=cb - 1)
    tsh = sh if sh == w else _r4(2 * w) + 8 + sh % 4
    if sc == h * w:
        tsc = sc
    else:
        tsc = sc if s.kind == "far-H" else _r4(h * w) + 4 + sc % 4
    tsn = _r4(max(c * tsc, h * tsh)) + 4 + sn % 4
    t = replace(s, kind="twin of " + s.kind, strides=(tsn, tsc, tsh))
    assert (n == 1 or tsn != s.c_count * tsc) and (tsc == h * w) == (sc == h * w) and (tsh == w) == (sh == w)
    return t


# ----------------------------------------------------------------------------------------------------
# addressing: int64 throughout
# ----------------------------------------------------------------------------------------------------
def map_offsets(s, placed=False):
    """[N, c] int64: offset of the first element of every scored (or placed) map from the tensor's base."""
    n = np.arange(s.shape[0], dtype=np.int64)[:, None]
    lo, cnt = (s.p_begin, s.p_count) if placed else (s.c_begin, s.c_count)
    c = lo + np.arange(cnt, dtype=np.int64)[None, :]
    return n * np.int64(s.strides[0]) + c * np.int64(s.strides[1])


def map_span(s):
    """Elements from a map's first to its last, inclusive of both: (H - 1) strideH + W."""
    return (s.shape[2] - 1) * s.strides[2] + s.shape[3]


def elem_offsets(s, placed=False):
    """[N, c, H, W] int64 offsets from the tensor's base."""
    r = np.arange(s.shape[2], dtype=np.int64)[:, None] * np.int64(s.strides[2])
    col = np.arange(s.shape[3], dtype=np.int64)[None, :]
    return map_offsets(s, placed)[:, :, None, None] + (r + col)[None, None]


def extent(s):
    """fp32 arena elements the view needs: one behind the last element of its last placed map."""
    last = s.base + int(map_offsets(s, True).max()) + map_span(s)
    return (last * s.esize + 3) // 4


def wrap_offsets(s, off, wrap):
    """The offsets a 32-bit register would hold, scaled to `unit`."""
    if wrap is None:
        return off
    if wrap == "s32_bytes":
        m = np.int64(s.eunit)
        return (off + m) % (2 * m) - m
    if wrap == "u32_bytes":
        return off % np.int64(2 * s.eunit)
    if wrap == "i32_elems":
        m = np.int64(4 * s.unit)
        return (off + m) % (2 * m) - m
    raise ValueError(wrap)


def reaches(s, wrap):
    """True if some scored element lies at or beyond the offset at which `wrap` first changes an offset."""
    first = {"s32_bytes": s.eunit, "u32_bytes": 2 * s.eunit, "i32_elems": 4 * s.unit}[wrap]
    return int(map_offsets(s).max()) + map_span(s) - 1 >= first


def reached_bounds(s):
    """The boundaries (elements from the base) that some scored map reaches beyond."""
    top = int(map_offsets(s).max()) + map_span(s) - 1
    return tuple(b for b in s.bounds if top > b)


def maps_beyond(s, b):
    """[N, c_count] bool: scored maps with an element beyond boundary b."""
    return map_offsets(s) + (map_span(s) - 1) > b


def maps_containing(s, b):
    """[N, c_count] bool: scored maps whose span holds element b."""
    o = map_offsets(s)
    return (o <= b) & (b < o + map_span(s))


def assert_reach(s, expect=None):
    """Every boundary the view can reach has a checked map beyond it (and the kind reaches what it is meant to)."""
    got = reached_bounds(s)
    if expect is not None:
        assert got == tuple(expect), "%s reaches %s, expected %s" % (s.kind, got, tuple(expect))
    assert got, "%s reaches no boundary" % s.kind
    for b in got:
        assert maps_beyond(s, b).any()
    return got


def gather(arena, s, wrap=None):
    """A plain numpy model of the addressing: the [N, c_count, H, W] maps a kernel reads from `arena` (a 1-D numpy array
    of the view's element type), its offsets from the base truncated as `wrap` says. An element outside the arena reads
    as NaN."""
    idx = wrap_offsets(s, elem_offsets(s), wrap) + np.int64(s.base)
    ok = (idx >= 0) & (idx < arena.shape[0])
    out = arena[np.where(ok, idx, 0)].astype(np.float32)
    out[~ok] = np.nan
    return out


# ----------------------------------------------------------------------------------------------------
# the arena
# ----------------------------------------------------------------------------------------------------
def typed(arena, s, dtype=None):
    """The arena as elements of the view's type (a reinterpreting view of the fp32 tensor)."""
    if s.esize == 4:
        return arena
    assert dtype in (torch.float16, torch.bfloat16)
    return arena.view(dtype)


def view(arena, s, dtype=None, placed=False):
    """The tensor an entry point is handed ([N, C_total, H, W]), or the block of channels that holds maps."""
    a = typed(arena, s, dtype)
    n, c, h, w = s.shape
    sn, sc, sh = s.strides
    assert extent(s) <= arena.numel(), "%s needs %d floats, the arena has %d" % (s.kind, extent(s), arena.numel())
    if placed:
        return a.as_strided((n, s.p_count, h, w), (sn, sc, sh, 1), s.base + s.p_begin * sc)
    return a.as_strided((n, c, h, w), (sn, sc, sh, 1), s.base)


def place(arena, s, maps):
    """Writes the compact maps [N, p_count, H, W] into their places; returns the entry point's tensor."""
    assert no_overlap(s)
    view(arena, s, maps.dtype, placed=True).copy_(maps)
    return view(arena, s, maps.dtype)


def restore(arena, s, dtype=None):
    """Zeros back to exactly the places place() wrote; True if they read as zero afterwards."""
    v = view(arena, s, dtype, placed=True)
    v.zero_()
    return not bool(v.any())


def no_overlap(s):
    """No two placed maps share an element (rows of different maps may interleave, as in far-H)."""
    n, _, h, w = s.shape
    rows = (map_offsets(s, True)[:, :, None] + (np.arange(h, dtype=np.int64) * np.int64(s.strides[2]))[None, None]).reshape(-1)
    rows.sort()
    return bool((np.diff(rows) >= w).all())


# ----------------------------------------------------------------------------------------------------
# contents
# ----------------------------------------------------------------------------------------------------
DEAD_EVERY, DEAD_AT = 8, 5  # placed map i is all zero where i % 8 == 5


def make_maps(s, seed, dtype=torch.float32, content="randn"):
    """The compact CPU copy [N, p_count, H, W]: every map from a seed of its own, per-map scales spread over two decades
    (10^-1 ... 10^1), every eighth map all zero. A wrong address therefore yields zeros from the untouched arena, another
    map's clearly different energy, or non-zero for a dead map.
    content="rank": map i is an exact small-integer matrix of rank 1 + (5 i) % min(H, W) times a power of two, so that
    neighbouring maps differ in the one number the rank criterion returns."""
    n, _, h, w = s.shape
    count = n * s.p_count
    out = np.zeros((count, h, w), np.float32)
    for i in range(count):
        if i % DEAD_EVERY == DEAD_AT:
            continue
        g = np.random.default_rng((seed, i))
        if content == "rank":
            r = 1 + (5 * i) % min(h, w)
            u, v = g.integers(-1, 2, (h, r)).astype(np.float64), g.integers(-1, 2, (r, w)).astype(np.float64)
            u[:r] += 16.0 * np.eye(r)
            v[:, :r] += 16.0 * np.eye(r)
            out[i] = (u @ v) * 2.0 ** int(g.integers(-3, 4))
        else:
            out[i] = g.standard_normal((h, w)) * 10.0 ** g.uniform(-1.0, 1.0)
    return torch.from_numpy(out).view(n, s.p_count, h, w).to(dtype)


def scored(s, maps):
    """The scored channels of the compact copy, [N, c_count, H, W]."""
    lo = s.c_begin - s.p_begin
    return maps[:, lo:lo + s.c_count]


# ----------------------------------------------------------------------------------------------------
# the checking function of both test files
# ----------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_bitwise(got, got_twin, s, what="output"):
    """(b): the far view and its twin give the same bits."""
    a, b = bits(got), bits(got_twin)
    assert a.shape == b.shape, "%s: %s of shape %s, the twin's %s" % (s.kind, what, tuple(a.shape), tuple(b.shape))
    if not torch.equal(a, b):
        i = int((a != b).reshape(-1).nonzero()[0])
        raise AssertionError("%s: %s element %d is %r, the twin view gives %r"
                             % (s.kind, what, i, got.reshape(-1)[i].item(), got_twin.reshape(-1)[i].item()))


def energy_tolerance(x, **kw):
    """dct_probes' rule on (a seeded subsample of) the maps x [N, C, H, W]: (tol, E_ref)."""
    import dct_probes as dp
    h, w = x.shape[2], x.shape[3]
    flat = x.reshape(1, -1, h, w)
    m = min(dp.SUBSAMPLE_MAPS, flat.shape[1], max(8, dp.SUBSAMPLE_BYTES // (h * w * 4)))
    if m < flat.shape[1]:
        g = torch.Generator().manual_seed(77)
        flat = flat[:, torch.randperm(flat.shape[1], generator=g)[:m].sort().values]
    e_ref = dp.reference_error(flat.float(), **kw)
    return dp.tolerance(e_ref), e_ref


def check_energies(s, maps, got, got_twin, expect=None, **kw):
    """(a) got [N, c_count] against float64 sum(x^2) of the compact copy within dct_probes' bound, zero maps exactly +0.0;
    (b) bit for bit the twin view's result; and the case reaches beyond every boundary its kind can. Returns
    (worst relative error, tol)."""
    import dct_probes as dp
    assert_reach(s, expect)
    x = scored(s, maps).float()
    tol, _ = energy_tolerance(x, **kw)
    got = got.detach().cpu()
    worst = dp.check_energy(lambda _: got, x, tol, what=s.kind)
    if got_twin is not None:
        assert_bitwise(got, got_twin, s, "energy")
    return worst, tol


# ----------------------------------------------------------------------------------------------------
# the cases of tests/test_far_offsets_gpu.py (tests/test_far_offsets_cpu.py checks the construction of each)
# ----------------------------------------------------------------------------------------------------
SMALL_KINDS = ("far-N", "far-C", "far-C+1", "slice", "far-D")
TILE_KINDS = ("far-N", "far-C", "slice", "far-D")  # far-N, far-C and slice are refused by the explicit family: AUTO takes them

# (algo, H, W, kinds): the smallest edge at which each kernel or load path exists (codelet_sizes.h)
ENERGY_CASES = (
    [("CODELET", n, n, SMALL_KINDS) for n in (2, 8, 14, 56)]      # 32, 8, 4 and 1 maps per wave and round
    + [("PREFETCH", 8, 8, TILE_KINDS)]                            # dense 16-byte-aligned tiles only: far-D
    + [("LANE", 7, 7, SMALL_KINDS)]
    + [("RECT", 13, 22, SMALL_KINDS), ("RECT", 56, 28, SMALL_KINDS + ("far-H",))]
    + [("DIRECT", 5, 5, SMALL_KINDS), ("DIRECT", 33, 33, SMALL_KINDS + ("far-H",))]
    + [("SPLIT", 68, 68, TILE_KINDS), ("SPLIT", 272, 272, TILE_KINDS)]  # split.hip's smallest entry, split_more.hip's smallest
    + [("FUSED", 72, 72, TILE_KINDS), ("FUSED", 288, 288, TILE_KINDS)]  # 288: two roles per wave (fused2.hip)
    + [("PIPE", 128, 128, TILE_KINDS)]
    + [("TILE2D", 224, 224, TILE_KINDS), ("TILE2D", 72, 72, TILE_KINDS)]  # tile2d.hip, tile2g.hip
)
PAD_CASES = [(7, SMALL_KINDS), (9, SMALL_KINDS), (71, SMALL_KINDS)]  # AUTO with pad_front_if_odd; 71 dense: tile2g_pad
COEFF_CASES = [("CODELET", 8, ("far-N", "far-C", "slice")), ("DIRECT", 5, ("far-N", "far-C", "slice")),
               ("TILE2D", 72, ("far-N", "far-C", "slice", "far-D")), ("FUSED", 72, ("far-D",)),
               ("TILE2D", 224, ("far-N", "far-C", "slice", "far-D")), ("FUSED", 224, ("far-D",))]
WEIGHTED_CASES = [(8, ("far-N", "far-C", "slice")), (72, ("far-N", "far-C", "far-D"))]
BAND_CASES = [("CODELET", 14, 14, ("far-N", "far-C", "slice")), ("CODELET", 56, 56, ("far-N", "far-C", "slice")),
              ("AUTO", 72, 72, ("far-N", "far-C", "far-D")), ("AUTO", 56, 28, ("far-N", "far-C", "slice"))]
HALF_CASES = ([(n, n, ("far-N", "far-C", "far-C+1", "slice")) for n in (2, 7, 56)]  # native
              + [(20, 20, ("far-N", "far-C")), (56, 56, ("far-H",))])              # staged
RANK_CASES = [(8, 8, ("far-N", "far-C", "slice")), (13, 22, ("far-N", "far-C", "slice")), (33, 22, ("far-H",))]


def build(kind, h, w, unit, esize=4):
    """The specs of one case: one view, or far-D's three (one per boundary)."""
    if kind == "far-N":
        return [far_n(h, w, unit, esize)]
    if kind == "far-C":
        return [far_c(h, w, unit, esize)]
    if kind == "far-C+1":
        return [far_c(h, w, unit, esize, base=1)]
    if kind == "far-H":
        return [far_h(h, w, unit, esize)]
    if kind == "slice":
        return [slice_n(h, w, unit, esize)]
    if kind == "far-D":
        return [far_d(h, w, unit, k, esize) for k in range(3)]
    raise ValueError(kind)


def expected_reach(s):
    """The boundaries a kind is built to reach: all three, far-H the first two, far-D k the first k + 1."""
    if s.kind == "far-H":
        return s.bounds[:2]
    if s.kind.startswith("far-D"):
        return s.bounds[:int(s.kind[-1]) + 1]
    return s.bounds


def all_shape_kinds():
    """Every (H, W, kind, esize) of the tables above, once."""
    seen = []
    def add(h, w, kinds, esize=4):
        for k in kinds:
            if (h, w, k, esize) not in seen:
                seen.append((h, w, k, esize))
    for _, h, w, kinds in ENERGY_CASES + BAND_CASES:
        add(h, w, kinds)
    for n, kinds in PAD_CASES + WEIGHTED_CASES:
        add(n, n, kinds)
    for _, n, kinds in COEFF_CASES:
        add(n, n, kinds)
    for h, w, kinds in RANK_CASES:
        add(h, w, kinds)
    for h, w, kinds in HALF_CASES:
        add(h, w, kinds, 2)
    return seen
