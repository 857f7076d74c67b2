// codelet_schedule.hpp - the register-resident two-pass schedule (square tiles, edge <= 64), stated once: the slab geometry
// and launch rules (CodeletCfg), and the plain form of the body - lane role, group walk, fp32 column load, both passes
// through the wave's slab, energy epilogue - that band.hip, entropy.hip, half.hip and nhwc.hip build their kernels from;
// each of them adds a load or an epilogue of its own. codelet.hip's kernels (the ones bench.py measures) keep their own
// text of the body and say where they leave the plain form. Host side: the grid rule, the launch helper and the size
// switch (the occupancy query blocks_per_cu() is in dcts_internal.h).
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
#include "grid_caps.h"

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

// ---- the plain form of the body ----------------------------------------------------------------------------------------------
// Four of the five pieces are macros, for the reason given at DCTS_MAP_SUM. As __forceinline__ functions (tried: the role as
// a struct, load, passes and epilogue as templates) the same lines reach the kernel simplified in another order and every
// kernel built from them compiles to other code: up to 48 more VGPRs, a wave per SIMD lost at some edges (DESIGN.md 4.2,
// "The body, stated once"). As macros they compile to the code of the text they replace, instruction for instruction.
// The macros declare what they produce (g1, c, act; xr; w; e) in the scope they are used in, in the order given here:
//   DCTS_CODELET_LANE, [the group loop:] DCTS_CODELET_LOAD or a load of the kernel's own, DCTS_CODELET_PASSES,
//   DCTS_CODELET_ENERGY or an epilogue of the kernel's own, wave_fence() before the slab is written again.

// The lane's role for edge N: map g1 of the wave's group and column c in pass 1, row c of the same map in pass 2 (square
// tile: one role for both). Lanes beyond G * N are idle (act == false).
#define DCTS_CODELET_LANE(N, lane)                       \
  const int g1 = (lane) / (N), c = (lane) - g1 * (N);    \
  const bool act = g1 < CodeletCfg<N>::G;

// The grid-stride walk over the groups of `nmaps` maps for a kernel of CodeletCfg<N>::WAVES one-group waves:
//   for (grp = first; grp < ngroups; grp += step), the lane's map m1 = grp * G + g1, and it has one if act && m1 < nmaps.
struct CodeletGroups {
  long long first, step, ngroups;
};
template <int N>
__device__ __forceinline__ CodeletGroups codelet_groups(long long nmaps) {
  constexpr int G = CodeletCfg<N>::G, WAVES = CodeletCfg<N>::WAVES;
  CodeletGroups w;
  w.ngroups = (nmaps + G - 1) / G;
  w.first = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  w.step = (long long)gridDim.x * WAVES;
  return w;
}

// The fp32 column load: declares xr[N] = column c of map m1 of the MapGeom g (dense rows of N - PAD floats) behind PAD zero
// rows and columns. PAD == 0 has no branch and no zero fill: lanes without a map (has == false) load some valid map
// instead, and their results are never stored.
#define DCTS_CODELET_LOAD(N, PAD, g, m1, c, has, xr)                                    \
  float xr[N];                                                                          \
  if constexpr (PAD == 0) {                                                             \
    const float* p = map_base(g, (has) ? (m1) : (g).nmaps - 1) + ((has) ? (c) : 0);     \
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {                                \
      constexpr int r = decltype(i)::value;                                             \
      xr[r] = p[r * (N - PAD)];                                                         \
    });                                                                                 \
  } else {                                                                              \
    if ((has) && (c) >= PAD) {                                                          \
      const float* p = map_base(g, m1) + ((c) - PAD);                                   \
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {                              \
        constexpr int r = decltype(i)::value;                                           \
        if constexpr (r < PAD)                                                          \
          xr[r] = 0.f;                                                                  \
        else                                                                            \
          xr[r] = p[(r - PAD) * (N - PAD)];                                             \
      });                                                                               \
    } else {                                                                            \
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE { xr[decltype(i)::value] = 0.f; }); \
    }                                                                                   \
  }

// Both passes: the lane's column xr[N] in; declares w[N], the N unnormalised coefficients of the lane's row. Through the
// wave's slab `my` with plain transposing stores; idle lanes store nothing and read in bounds.
#define DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)                                                             \
  float dcts_y[N]; /* pass 1: column DCT-II, lane = column */                                                     \
  dcts::Dct2<N>::run(xr, dcts_y);                                                                                 \
  dcts_y[0] *= dcts::kInvSqrt2;                                                                                   \
  if (act) {                                                                                                      \
    float* dst = (my) + (g1) * CodeletCfg<N>::MAP_LDS + (c);                                                      \
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {                                                          \
      constexpr int kk = decltype(i)::value;                                                                      \
      dst[kk * CodeletCfg<N>::S] = dcts_y[kk];                                                                    \
    });                                                                                                           \
  }                                                                                                               \
  wave_fence();                                                                                                   \
  float dcts_z[N], w[N]; /* pass 2: row DCT-II, lane = row */                                                     \
  {                                                                                                               \
    const float* src = (my) + ((act) ? (g1) : 0) * CodeletCfg<N>::MAP_LDS + ((act) ? (c) : 0) * CodeletCfg<N>::S; \
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {                                                          \
      constexpr int cc = decltype(i)::value;                                                                      \
      dcts_z[cc] = src[cc];                                                                                       \
    });                                                                                                           \
  }                                                                                                               \
  dcts::Dct2<N>::run(dcts_z, w);                                                                                  \
  w[0] *= dcts::kInvSqrt2;

// The energy epilogue: declares e, the row's squares summed in row order (0 in idle lanes), then over the map's lanes. The
// map's lane c == 0 ends with the unscaled sum; times CodeletCfg<N>::SCALE it is the ortho energy.
#define DCTS_CODELET_ENERGY(N, w, c, act, e)               \
  float e = 0.f;                                           \
  dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {     \
    constexpr int l = decltype(i)::value;                  \
    e = fmaf(w[l], w[l], e);                               \
  });                                                      \
  if (!(act)) e = 0.f;                                     \
  DCTS_MAP_SUM(N, e, c)

// The whole schedule in one lane, for kernels that give a lane a map of its own (no LDS, no cross-lane step): both passes
// in registers, squares summed in (row, coefficient) order; returns the ortho energy.
template <int N>
__device__ __forceinline__ float lane_energy(float (&v)[N * N]) {
  dcts::static_for<N>([&](auto ic) DCTS_LAMBDA_INLINE {  // columns, in place
    constexpr int c = decltype(ic)::value;
    float in[N], o[N];
    dcts::static_for<N>([&](auto ir) DCTS_LAMBDA_INLINE { in[decltype(ir)::value] = v[decltype(ir)::value * N + c]; });
    dcts::Dct2<N>::run(in, o);
    o[0] *= dcts::kInvSqrt2;
    dcts::static_for<N>([&](auto ir) DCTS_LAMBDA_INLINE { v[decltype(ir)::value * N + c] = o[decltype(ir)::value]; });
  });
  float e = 0.f;
  dcts::static_for<N>([&](auto ir) DCTS_LAMBDA_INLINE {  // rows
    constexpr int r = decltype(ir)::value;
    float in[N], o[N];
    dcts::static_for<N>([&](auto ic) DCTS_LAMBDA_INLINE { in[decltype(ic)::value] = v[r * N + decltype(ic)::value]; });
    dcts::Dct2<N>::run(in, o);
    o[0] *= dcts::kInvSqrt2;
    dcts::static_for<N>([&](auto ic) DCTS_LAMBDA_INLINE { e = fmaf(o[decltype(ic)::value], o[decltype(ic)::value], e); });
  });
  constexpr float sc = float(4.0 / (double(N) * double(N)));
  return e * sc;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <int N>
unsigned codelet_grid(long long groups) {
  using Cfg = CodeletCfg<N>;
  return dctsi::grid_blocks(groups, Cfg::WAVES, (long long)dctsi::num_cus() * Cfg::GRID_WAVES_PER_CU / Cfg::WAVES);
}
// launches `kernel` - workgroups of CodeletCfg<N>::WAVES waves, one group of G maps per wave and iteration - over nmaps maps
template <int N, class... P, class... A>
int launch_codelet_grid(void (*kernel)(P...), long long nmaps, hipStream_t st, const A&... args) {
  using Cfg = CodeletCfg<N>;
  const long long ngroups = (nmaps + Cfg::G - 1) / Cfg::G;
  hipLaunchKernelGGL(kernel, dim3(codelet_grid<N>(ngroups)), dim3(64 * Cfg::WAVES), 0, st, args...);
  return (int)hipGetLastError();
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
