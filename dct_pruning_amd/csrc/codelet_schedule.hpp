// codelet_schedule.hpp - what the kernels of the register-resident two-pass schedule (square tiles, edge <= 64) share:
// the slab geometry and launch rules (CodeletCfg), the wavefront fence, the segmented reduction, and the host-side grid
// rule, occupancy query and size switch. codelet.hip (fp32 energies and coefficients), band.hip (K weighted energies) and
// half.hip (fp16 / bf16 inputs) hold the kernels.
//
// One wave owns G = floor(64 / N) maps per iteration. Pass 1: lane = column, the lane holds the whole column in VGPRs
// (row r of a map is one contiguous segment across lanes: coalesced loads straight from HBM) and runs a straight-line
// factorised DCT-II (dct_codelets.hpp). The tile is transposed through the wave's private LDS slab (padded strides:
// conflict-free both ways), a wavefront fence orders the two sides, and in pass 2 lane = row runs the second codelet. The
// squares are summed in-lane, then across the N lanes of a map with a segmented wave shuffle reduction, and scaled by 4 / N^2.
// Every translation unit gets its own copy (anonymous namespace), as with split_roles.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "dct_codelets.hpp"
#include "dcts_internal.h"

namespace {

template <int N>
struct CodeletCfg {
  static constexpr int G = 64 / N;              // maps per wave per iteration
  // LDS row stride S and per-map stride: odd S is conflict-free inside one map; when several maps
  // share a wave the pair (S, MAP_LDS) below keeps the G*edge lanes of a half-wave on distinct
  // banks for both the column-wise store and the row-wise load (brute-force search over paddings,
  // SQ_LDS_BANK_CONFLICT was 18-47 % of LDS cycles before for these edges)
  static constexpr int S = N == 7 ? 8 : (N == 10 || N == 14) ? 17 : N == 20 ? 25 : N == 28 ? 33 : (N | 1);
  static constexpr int MAP_LDS = N == 7 ? 71 : N * S;  // floats per map in the transpose slab
  static constexpr int WAVE_LDS = G * MAP_LDS;  // floats per wave
  // waves per workgroup: keep a workgroup's slab <= 48 KiB so >= 3 workgroups fit a CU
  static constexpr int WAVES = (WAVE_LDS * 4 * 4 <= 49152) ? 4 : ((WAVE_LDS * 4 * 2 <= 49152) ? 2 : 1);
  // Waves launched per CU at most (the grid-stride loop takes the rest). NOT one residency (12 waves per CU
  // at 56 x 56): a grid several times the residency, whose workgroups the dispatcher hands out as CUs free up,
  // is faster than persistent waves in lock step - sweep of this cap on the bench's own launches, waves per
  // CU -> % of the HBM peak: 56 x 56 (344 k maps) 32: 67.2, 128...512: 69.6, 2048: 66.3; 28 x 28 (819 k) 32:
  // 68.4, 256: 74.7, 512: 76.4, 2048: 72.5; 14 x 14 (2.4 M) 32: 69.4, 512: 74.7, 2048: 74.9; 200 MB launches
  // of 8 / 14 / 28 / 32: 62 -> 71, 62 -> 71, 66 -> 72.5, 68 -> 73.5; whole ResNet-50 step 3259 -> 3561 Mmaps/s.
  // (4 x 4 and 2 x 2 groups are 1 KB and 512 B: there the wider grid costs more in wave launches than it
  // gains - 70 -> 61 % and 50 -> 46 % - and the cap stays at 32.)
  static constexpr int GRID_WAVES_PER_CU = (N * N >= 48 * 48) ? 256 : ((N * N >= 8 * 8) ? 512 : 32);
  static constexpr float SCALE = float(4.0 / (double(N) * double(N)));  // squared unnormalised coefficients -> ortho energy
};

// the wave's own LDS traffic is in order; only the compiler must not reorder
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Segmented reduction of `e` over the N lanes of each map: the lane of row c == 0 ends with the sum (idle lanes pass 0).
// A macro on purpose: as a __forceinline__ function the loop is unrolled and simplified before it meets the kernel, and
// 55 of the 149 kernels of codelet.hip then compile to another instruction order (bench.py measures them).
#define DCTS_MAP_SUM(N, e, c)                                   \
  _Pragma("unroll") for (int off = 32; off >= 1; off >>= 1) {   \
    if (off < (N)) {                                            \
      const float t = __shfl_down(e, off, 64);                  \
      if ((c) + off < (N)) e += t;                              \
    }                                                           \
  }

// ---- host side -------------------------------------------------------------------------------------------------------------
// the grid rule: one wave per group, at most `cap` workgroups (the grid-stride loops take the rest), at least one
inline unsigned grid_blocks(long long groups, int per_block, long long cap) {
  long long blocks = (groups + per_block - 1) / per_block;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
template <int N>
unsigned codelet_grid(long long groups) {
  using Cfg = CodeletCfg<N>;
  return grid_blocks(groups, Cfg::WAVES, (long long)dctsi::num_cus() * Cfg::GRID_WAVES_PER_CU / Cfg::WAVES);
}
// workgroups of `kernel` (WAVES waves, static LDS only) that fit a CU, queried once: the persistent grids are one residency
template <auto kernel, int WAVES>
int blocks_per_cu() {
  static const int per_cu = [] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 64 * WAVES, 0) != hipSuccess || n < 1) n = 1;
    return n;
  }();
  return per_cu;
}
// f(N, PAD) as integral constants for the edge n of DCTS_CODELET_SIZES; the odd front pad makes an even edge, so the
// padded variant exists only for even N
template <class F>
int switch_codelet_size(int n, int pad, F&& f) {
#define DCTS_CASE(N)                                                                                    \
  case N:                                                                                               \
    if (pad) {                                                                                          \
      if constexpr ((N % 2) == 0 && N >= 2)                                                             \
        return f(std::integral_constant<int, N>{}, std::integral_constant<int, 1>{});                   \
      else                                                                                              \
        return DCTS_E_UNSUPPORTED;                                                                      \
    }                                                                                                   \
    return f(std::integral_constant<int, N>{}, std::integral_constant<int, 0>{});
  switch (n) {
    DCTS_CODELET_SIZES(DCTS_CASE)
    default:
      return DCTS_E_UNSUPPORTED;
  }
#undef DCTS_CASE
}

}  // namespace
