"""How many maps ONE full grid of every capped, grid-stride kernel family holds - the launch rules restated in Python.

At capacity(cus) maps every wave (or workgroup) of the capped grid takes exactly one group, item or map; one more and
some wave runs its loop a second time. tests/test_grid_loops_gpu.py sizes its cases by these numbers (2.3 x capacity:
some waves run three iterations, others two). tests/test_grid_loops_cpu.py compares every constant below with what
tests/native/grid_probe.cpp prints from the headers the launch sites include, for 256 and 304 CUs, so the table cannot
drift from the code. Each rule names the source it restates. No product import; integers only.
"""
from collections import namedtuple

# codelet_sizes.h: DCTS_CODELET_SIZES, dcts_internal.h: DCTS_HALF_SIZES, DCTS_MIXED_SIZES, DCTS_NHWC_*_SIZES
CODELET_SIZES = (2, 4, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 24, 28, 30, 32, 36, 40, 48, 56, 60, 64)
HALF_SIZES = (2, 4, 7, 8, 14, 16, 28, 32, 56)
MIXED_SIZES = (2, 4, 8, 16, 32)
NHWC_LANE_SIZES = (2, 4, 7, 8)
NHWC_BLOCK_SIZES = (14, 16, 28, 32)
NHWC_STRIP_SIZE = 56
MULTI_ITEMS, MIXED_ITEMS = 32, 48  # dcts_internal.h: kMultiItems, kMixedItems (the chunking of the multi-tensor calls)

CodeletCfg = namedtuple("CodeletCfg", "G S MAP_LDS WAVE_LDS WAVES GRID_WAVES_PER_CU")


def codelet_cfg(n):
    """codelet_schedule.hpp: CodeletCfg<N>."""
    g = 64 // n
    s = 8 if n == 7 else 17 if n in (10, 14) else 25 if n == 20 else 33 if n == 28 else (n | 1)
    map_lds = 71 if n == 7 else n * s
    wave_lds = g * map_lds
    waves = 4 if wave_lds * 4 * 4 <= 49152 else (2 if wave_lds * 4 * 2 <= 49152 else 1)
    per_cu = 256 if n * n >= 48 * 48 else (512 if n * n >= 8 * 8 else 32)
    return CodeletCfg(g, s, map_lds, wave_lds, waves, per_cu)


def codelet_grid(n, cus):
    """codelet_schedule.hpp: codelet_grid<N> for more groups than the cap - workgroups of CodeletCfg<N>::WAVES waves."""
    c = codelet_cfg(n)
    return max(1, cus * c.GRID_WAVES_PER_CU // c.WAVES)


Capacity = namedtuple("Capacity", "units maps_per_unit")  # units: waves or workgroups, each taking one group / item / map
Capacity.maps = property(lambda self: self.units * self.maps_per_unit)


def codelet(n, cus):
    """k_energy_codelet, k_energy_codelet_multi, k_band_codelet, k_energy_half (codelet.hip launch_codelet[_multi],
    band.hip launch_band, half.hip launch_half): codelet_grid<N> workgroups of WAVES waves, a wave takes one group of G maps."""
    c = codelet_cfg(n)
    return Capacity(codelet_grid(n, cus) * c.WAVES, c.G)


# The two persistent kernels of codelet.hip (launch_lane, dispatch_codelet_mixed) launch num_cus x
# hipOccupancyMaxActiveBlocksPerMultiprocessor workgroups, a number only the runtime knows. 16 workgroups per CU is a safe
# UPPER bound on it: a CU holds at most 32 waves (8 per SIMD), the workgroups have 2 and 4 waves, so at most 16 and 8
# of them fit whatever their registers and LDS allow. A case sized by this bound loops at least as often as one sized exactly.
PERSISTENT_BLOCKS_PER_CU = 16
LANE_MULTI_WAVES, LANE_MULTI_G = 2, 64   # grid_caps.h: kLaneMultiWaves, kLaneMultiGroup (LaneCfg<N>::WAVES, ::G; edges 7 and 9)
MIXED_WAVES = 4                          # grid_caps.h: kMixedWaves


def lane_multi(cus):
    """k_energy_lane_multi: a wave takes one group of 64 maps."""
    return Capacity(cus * PERSISTENT_BLOCKS_PER_CU * LANE_MULTI_WAVES, LANE_MULTI_G)


def mixed_groups(cus):
    """k_energy_codelet_mixed: waves of the (upper-bounded) persistent grid; a wave takes one group of 64 // edge maps of
    the tensor the group belongs to."""
    return cus * PERSISTENT_BLOCKS_PER_CU * MIXED_WAVES


NHWC_LANE_WAVES = 4  # grid_caps.h: kNhwcLaneWaves


def nhwc_lane_items(n, cus):
    """nhwc.hip launch_nhwc_lane: cus * GRID_WAVES_PER_CU / kLaneWaves workgroups of kLaneWaves waves; a wave takes one
    item = 64 consecutive channels of one sample (the last run of a sample may be shorter)."""
    return max(1, cus * codelet_cfg(n).GRID_WAVES_PER_CU // NHWC_LANE_WAVES) * NHWC_LANE_WAVES


def nhwc_block_cb(n):
    """grid_caps.h: nhwc_block_cb (NhwcBlockCfg<N>::CB) and kNhwcStripCb - channels per workgroup."""
    if n == NHWC_STRIP_SIZE:
        return 4
    return 32 if n <= 16 else (16 if n <= 28 else 8)


def nhwc_block_items(n, cus):
    """nhwc.hip launch_nhwc_block / launch_nhwc_strip: codelet_grid<N>(items * WAVES) workgroups; a workgroup takes one
    item = CB consecutive channels of one sample."""
    return codelet_grid(n, cus)


RECT_WAVES, RECT_BLOCKS_PER_CU = 4, 64  # grid_caps.h: kRectWaves, kRectBlocksPerCu
RectGroup = namedtuple("RectGroup", "G G1 G2 S map_lds")


def rect_slab_cap(edge):
    """grid_caps.h: rect_slab_cap - floats of LDS slab per wave by size class."""
    return 1536 if edge <= 16 else (2304 if edge <= 32 else 3400)


def rect_group(hp, wp, store_coeff=False):
    """grid_caps.h: rect_group - the maps per wave iteration dispatch_rect chooses."""
    g1, g2 = 64 // wp, 64 // hp
    s = wp | 1
    map_lds = hp * s + (1 if (hp * s) % 2 == 0 else 0)
    gmax = max(1, rect_slab_cap(max(hp, wp)) // map_lds)
    best = min(g1, g2, gmax)
    runs = lambda g: -(-g // g1) - (-g // g2)
    if not store_coeff:
        for g in range(best + 1, gmax + 1):
            if runs(g) * best < runs(best) * g:
                best = g
    return RectGroup(best, min(g1, best), min(g2, best), s, map_lds)


def rect(hp, wp, cus):
    """rect.hip dispatch_rect: cus * kRectBlocksPerCu workgroups of kRectWaves waves, a wave takes one group of G maps."""
    return Capacity(cus * RECT_BLOCKS_PER_CU * RECT_WAVES, rect_group(hp, wp).G)


RANK_MAX_BLOCKS = 8192  # grid_caps.h: kRankMaxBlocks


def rank(h, w, cus=None):
    """rank.hip launch<G>: kRankMaxBlocks single-wave workgroups of MPW = 64 / G maps, G the smallest power of two >= 4
    that holds min(H, W). Does not depend on the CU count."""
    g = 4
    while g < min(h, w):
        g *= 2
    return Capacity(RANK_MAX_BLOCKS, 64 // g)


REDUCE_WAVES, REDUCE_MAX_BLOCKS = 4, 4096  # grid_caps.h: kReduceWaves, kReduceMaxBlocks


def reduce(cus=None):
    """band.hip launch_band_reduce and reduce.hip launch_weighted_reduce: 4096 workgroups of four waves, one wave per map."""
    return Capacity(REDUCE_MAX_BLOCKS * REDUCE_WAVES, 1)


def band_chunk_bytes(hp, wp):
    """grid_caps.h: band_chunk_bytes - bytes of coefficients per chunk dcts_band_workspace_bytes sizes the workspace for."""
    return (16 << 20) if hp <= 65 and wp <= 65 else (128 << 20)


def band_fallback_chunk_maps(h, w):
    """A LOWER bound on api.hip coeff_layout().chunk (maps per k_band_reduce launch) with the workspace of
    dcts_band_workspace_bytes: that is sized for the tile with the odd pad, (H + 1) x (W + 1), so a call without the pad
    gets at least this many maps per chunk."""
    return band_chunk_bytes(h + 1, w + 1) // ((h + 1) * (w + 1) * 4)


UPCAST_THREADS, UPCAST_BLOCKS_PER_CU, HALF_STAGE_CAP = 256, 32, 64 << 20  # grid_caps.h


def upcast_elems(cus):
    """half.hip launch_upcast_half: cus * 32 workgroups of 256 threads, one element per thread and step."""
    return cus * UPCAST_BLOCKS_PER_CU * UPCAST_THREADS


def half_stage_chunk_maps(h, w):
    """api.hip dcts_energy_typed, staged route: maps per chunk (one k_upcast_half launch each) once the call has more."""
    return HALF_STAGE_CAP // (h * w * 4)


# ----------------------------------------------------------------------------------------------------
# sizing a case
# ----------------------------------------------------------------------------------------------------
FACTOR_NUM, FACTOR_DEN = 23, 10  # 2.3 x capacity


def loop_count(units, maps_per_unit=1, factor=(FACTOR_NUM, FACTOR_DEN), multiple_of=1):
    """The smallest count >= ceil(factor * units * maps_per_unit) of maps (a multiple of `multiple_of`) that is NOT a
    multiple of maps_per_unit (where that is > 1 and multiple_of allows) and whose number of groups is not a multiple
    of `units`: some units then run ceil(factor) iterations and others one fewer, and the ragged group comes last."""
    cap = units * maps_per_unit
    n = -(-factor[0] * cap // factor[1])
    n = -(-n // multiple_of) * multiple_of
    while True:
        groups = -(-n // maps_per_unit)
        ragged_ok = maps_per_unit == 1 or n % maps_per_unit != 0 or multiple_of % maps_per_unit == 0
        if ragged_ok and groups % units != 0:
            return n
        n += multiple_of


def iterations(count, units, maps_per_unit=1):
    """(fewest, most) iterations a unit of the capped grid runs for `count` maps."""
    groups = -(-count // maps_per_unit)
    return groups // units, -(-groups // units)
