// grid_caps.h - the grid caps of the grid-stride kernels that do not take theirs from CodeletCfg (codelet_schedule.hpp),
// and the host-side group rule of rect.hip. Plain constants and host arithmetic, no HIP: the units that launch the kernels
// include it, and so does tests/native/grid_probe.cpp, which prints what it sees so that tests/grid_capacity.py (the
// capacities the grid-loop tests size their cases by) cannot drift from the launch sites.
#pragma once

namespace dctsi {

// the grid rule of every grid-stride kernel: one unit of `per_block` per group, at most `cap` workgroups (the loops take
// the rest), at least one
inline unsigned grid_blocks(long long groups, int per_block, long long cap) {
  long long blocks = (groups + per_block - 1) / per_block;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// rank.hip, k_rank: single-wave workgroups of 64 / G maps; grid-stride beyond (256 CUs x 32 workgroups)
constexpr int kRankMaxBlocks = 8192;

// rect.hip, k_energy_rect: workgroups of kRectWaves waves, at most kRectBlocksPerCu per CU - a grid several times the
// residency (codelet_schedule.hpp, GRID_WAVES_PER_CU)
constexpr int kRectWaves = 4;
constexpr int kRectBlocksPerCu = 64;
// floats of LDS slab a wave of k_energy_rect may have, by size class (edge = max(HP, WP)): what leaves the LDS room for as
// many waves as the registers of the size class allow (14 x 20 with a 14 KB slab of twelve maps ran two workgroups per
// CU: 28 % of the HBM peak against 45 % with three maps)
constexpr int rect_slab_cap(int edge) { return edge <= 16 ? 1536 : (edge <= 32 ? 2304 : 3400); }

// Maps per wave iteration of k_energy_rect and per pass step, the LDS row stride and the floats per map. Maps per pass
// step: floor(64 / WP) with columns as lanes, floor(64 / HP) with rows as lanes. A group is G maps, each pass taking them
// in ceil(G / G1) resp. ceil(G / G2) steps: G is chosen to minimise the codelet runs per map (56 x 28: G = 2, pass 1 once,
// pass 2 twice; 14 x 20: G = 12, four steps of three and three of four), within the slab a wave may have.
struct RectGroup {
  int G, G1, G2, S, map_lds;
};
inline RectGroup rect_group(int HP, int WP, bool store_coeff) {
  RectGroup r;
  const int edge = HP > WP ? HP : WP;
  r.G1 = 64 / WP;
  r.G2 = 64 / HP;
  r.S = WP | 1;  // odd row stride: the row-wise reads of pass 2 hit distinct banks within a map
  r.map_lds = HP * r.S + ((HP * r.S) % 2 == 0 ? 1 : 0);
  const int slab_cap = rect_slab_cap(edge);
  const int gmax = slab_cap / r.map_lds > 0 ? slab_cap / r.map_lds : 1;
  int best = r.G1 < r.G2 ? r.G1 : r.G2;
  if (best > gmax) best = gmax;
  auto runs = [&](int G) { return (G + r.G1 - 1) / r.G1 + (G + r.G2 - 1) / r.G2; };
  if (!store_coeff)
    for (int G = best + 1; G <= gmax; ++G)
      if ((long long)runs(G) * best < (long long)runs(best) * G) best = G;  // strictly fewer runs per map
  r.G = best;
  if (r.G1 > r.G) r.G1 = r.G;
  if (r.G2 > r.G) r.G2 = r.G;
  return r;
}

// band.hip, k_band_reduce, entropy.hip, k_entropy_reduce and reduce.hip, k_weighted_energy: one wave per map, workgroups of kReduceWaves waves
constexpr int kReduceWaves = 4;
constexpr int kReduceMaxBlocks = 4096;

// api.hip, coeff_layout_bytes(): bytes of coefficients per chunk that dcts_band_workspace_bytes and
// dcts_entropy_workspace_bytes size the workspace for (one reduction launch per chunk)
constexpr long long band_chunk_bytes(int HP, int WP) { return (HP <= 65 && WP <= 65) ? (16LL << 20) : (128LL << 20); }

// half.hip, k_upcast_half: one thread per element and step, workgroups of kUpcastThreads threads; api.hip, the staged
// route: bytes of upcast maps per chunk at most (one k_upcast_half launch per chunk)
constexpr int kUpcastThreads = 256;
constexpr int kUpcastBlocksPerCu = 32;
constexpr unsigned long long kHalfStageCap = 64ull << 20;

// codelet.hip, the two persistent kernels (their grids are one residency, which the runtime's occupancy query decides):
// k_energy_lane_multi - workgroups of kLaneMultiWaves waves, a wave takes kLaneMultiGroup maps per iteration;
// k_energy_codelet_mixed - workgroups of kMixedWaves waves, a wave takes one group of its tensor's shape
constexpr int kLaneMultiWaves = 2;
constexpr int kLaneMultiGroup = 64;
constexpr int kMixedWaves = 4;

// gm.hip, k_gm_distance: a workgroup of kGmThreads threads owns one sample and kGmTS scored channels, walks the reference set
// kGmTR channels at a time and the flattened H * W axis kGmKP elements at a time; kGmLD: floats per channel row of its LDS
// image. One workgroup per (sample, scored tile) and no grid-stride loop: kGmMaxBlocks is the largest grid.x there is,
// and a call that would need more is refused (DCTS_E_SHAPE)
constexpr int kGmThreads = 256;
constexpr int kGmTS = 64;
constexpr int kGmTR = 64;
constexpr int kGmKP = 64;
constexpr int kGmLD = kGmKP + 4;
constexpr long long kGmMaxBlocks = 0x7fffffffLL;
// gm.hip, k_gm_stats (the normalised metrics' pass over every map): one wave per map, workgroups of kGmStatsThreads threads
// = kGmStatsMaps waves, one workgroup per kGmStatsMaps maps and no grid-stride loop either: the same largest grid, the same refusal
constexpr int kGmStatsThreads = 256;
constexpr int kGmStatsMaps = kGmStatsThreads / 64;
// gm_pairs.hip, k_gm_pairs: a workgroup of kGmThreads threads owns kGmTS scored channels, kGmTR reference channels and one
// slice of the samples; with more than one slice k_gm_pairs_sum (one thread per entry, workgroups of kGmPairSumThreads) adds
// the slices' partial matrices. Both grids are exact and capped by kGmMaxBlocks as well.
// The slices: enough of them that a square layer launches about kGmPairTarget workgroups (sixteen per CU of an MI355X: four
// rounds of the four that are resident; measured against 1024 and 2048), never more than there are samples, every slice the same ceil(N / S) samples but the last, none empty. A function of N and r_count
// alone: a call on a sub-range of the scored channels cuts the samples as the call on the whole range does, and the partial
// matrices of a square layer stay within kGmPairTarget * 64 * 64 * 4 bytes = 64 MiB. DCTS_GM_PAIRS_ONE_SLICE is a development
// define: the measurement of the rule against no slicing.
constexpr int kGmPairTarget = 4096;
constexpr int kGmPairSumThreads = 256;
inline int gm_pair_slices(long long N, int r_count) {
  if (N <= 0 || r_count <= 0) return 0;
#ifdef DCTS_GM_PAIRS_ONE_SLICE
  return 1;
#else
  const long long rt = (r_count + kGmTR - 1) / kGmTR;
  long long s = kGmPairTarget / (rt * rt);
  s = s < 1 ? 1 : (s > N ? N : s);
  const long long per = (N + s - 1) / s;  // samples per slice
  return (int)((N + per - 1) / per);      // the slices that hold a sample
#endif
}

// nhwc.hip: waves per workgroup of the lane = channel kernel (a wave takes 64 channels of one sample), and the channels a
// workgroup of the block kernel (edges 14 ... 32) and of the strip kernel (edge 56) takes
constexpr int kNhwcLaneWaves = 4;
constexpr int nhwc_block_cb(int n) { return n <= 16 ? 32 : (n <= 28 ? 16 : 8); }
constexpr int kNhwcStripCb = 4;

}  // namespace dctsi
