// grid_probe.cpp - prints the constants the capped grids of the grid-stride kernels are sized by, as the headers the launch
// sites include state them: one line per family and edge. tests/test_grid_loops_cpu.py compares tests/grid_capacity.py (the
// Python restatement the grid-loop tests size their cases by) with this output, so the table cannot drift from the code.
// Host code only: nothing is launched. `make -C dct_pruning_amd/csrc probe` builds and runs it with the GPU hidden, where
// dctsi::num_cus() answers 256; grid256 is codelet_grid<N> itself for more groups than any grid holds.
#include <cstdio>

#include "../../dct_pruning_amd/csrc/codelet_schedule.hpp"
#include "../../dct_pruning_amd/csrc/grid_caps.h"

using namespace dctsi;

template <int N>
static void codelet_line(const char* family) {
  using Cfg = CodeletCfg<N>;
  std::printf("%s N=%d G=%d WAVES=%d GRID_WAVES_PER_CU=%d grid256=%u\n", family, N, Cfg::G, Cfg::WAVES, Cfg::GRID_WAVES_PER_CU,
              codelet_grid<N>(1LL << 40));
}

int main() {
  if (num_cus() != 256) {
    std::fprintf(stderr, "grid_probe: run with the GPU hidden (HIP_VISIBLE_DEVICES= ROCR_VISIBLE_DEVICES=)\n");
    return 2;
  }
#define DCTS_CASE(N) codelet_line<N>("codelet");
  DCTS_CODELET_SIZES(DCTS_CASE)
#undef DCTS_CASE
#define DCTS_CASE(N) codelet_line<N>("half");
  DCTS_HALF_SIZES(DCTS_CASE)
#undef DCTS_CASE
#define DCTS_CASE(N) std::printf("mixed N=%d G=%d\n", N, CodeletCfg<N>::G);
  DCTS_MIXED_SIZES(DCTS_CASE)
#undef DCTS_CASE
  std::printf("multi items=%d mixed_items=%d lane_waves=%d lane_group=%d mixed_waves=%d\n", kMultiItems, kMixedItems, kLaneMultiWaves,
              kLaneMultiGroup, kMixedWaves);
#define DCTS_CASE(N) \
  std::printf("nhwc_lane N=%d waves=%d GRID_WAVES_PER_CU=%d\n", N, kNhwcLaneWaves, CodeletCfg<N>::GRID_WAVES_PER_CU);
  DCTS_NHWC_LANE_SIZES(DCTS_CASE)
#undef DCTS_CASE
#define DCTS_CASE(N)                                                                                                   \
  std::printf("nhwc_block N=%d CB=%d WAVES=%d GRID_WAVES_PER_CU=%d grid256=%u\n", N, nhwc_block_cb(N), CodeletCfg<N>::WAVES, \
              CodeletCfg<N>::GRID_WAVES_PER_CU, codelet_grid<N>((1LL << 40) * CodeletCfg<N>::WAVES));
  DCTS_NHWC_BLOCK_SIZES(DCTS_CASE)
#undef DCTS_CASE
  std::printf("nhwc_strip N=%d CB=%d WAVES=%d GRID_WAVES_PER_CU=%d grid256=%u\n", 56, kNhwcStripCb, CodeletCfg<56>::WAVES,
              CodeletCfg<56>::GRID_WAVES_PER_CU, codelet_grid<56>((1LL << 40) * CodeletCfg<56>::WAVES));
  std::printf("rect_caps waves=%d blocks_per_cu=%d slab16=%d slab32=%d slab64=%d\n", kRectWaves, kRectBlocksPerCu,
              rect_slab_cap(16), rect_slab_cap(32), rect_slab_cap(64));
  for (int hp = 1; hp <= 64; ++hp)
    for (int wp = 1; wp <= 64; ++wp)
      for (int store = 0; store < 2; ++store) {
        const RectGroup r = rect_group(hp, wp, store != 0);
        std::printf("rect HP=%d WP=%d store=%d G=%d G1=%d G2=%d map_lds=%d\n", hp, wp, store, r.G, r.G1, r.G2, r.map_lds);
      }
  std::printf("rank max_blocks=%d\n", kRankMaxBlocks);
  std::printf("reduce waves=%d max_blocks=%d band_chunk_small=%lld band_chunk_large=%lld\n", kReduceWaves, kReduceMaxBlocks,
              band_chunk_bytes(65, 65), band_chunk_bytes(66, 66));
  std::printf("upcast threads=%d blocks_per_cu=%d stage_cap=%llu\n", kUpcastThreads, kUpcastBlocksPerCu, kHalfStageCap);
  return 0;
}
