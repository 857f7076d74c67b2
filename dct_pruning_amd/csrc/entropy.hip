// entropy.hip - the spectral entropy of every map (dcts_spectral_entropy_f32, include/dctscore.h):
//   out[m] = -sum_{p > 0} p[u][v] * ln p[u][v],  p = c^2 / sum c^2,  c = dct_2d(map m, norm='ortho').
// A constant factor on the coefficients cancels in p, so both kernels work on whatever scale their coefficients have
// and use the one-pass form:  e = sum w^2,  s = sum w^2 * ln(w^2) (a zero square adds 0),
//   H = ln e - s / e, clamped into [+0.0, ln(H' * W')]; e == 0 (an all-zero map) gives +0.0.
//
//   k_entropy_codelet  the two-pass schedule of codelet_schedule.hpp (its group loop, load and passes): a lane ends with
//                      the N unnormalised coefficients of row u of its map in registers. What this unit adds is the
//                      epilogue: two accumulators per lane (e, s) fed coefficient by coefficient in the row's order,
//                      two segmented wave reductions, the final ln e - s / e in the map's lane 0, one store per map.
//                      A lane's two chains and the reduction tree depend on nothing but the map's row: the result of
//                      a map is the same bits for any N, channel slice, position in the wave or launch.
//   k_entropy_reduce   the fallback's reduction (every shape without a codelet, up to 512, and row-pitched views): one
//                      wave per map over dense tiles of orthonormal coefficients in the workspace; lanes stride the
//                      tile, every coefficient read once, fixed-order wave sums.
// ln is the accurate logf (denormal squares included), never the fast intrinsic. No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/dctscore.h"
#include "codelet_schedule.hpp"
#include "codelet_sizes.h"
#include "dct_codelets.hpp"
#include "dcts_internal.h"
#include "grid_caps.h"

using namespace dctsi;

namespace {

// e += sq, s += sq * ln(sq); a zero square (a dead coefficient, or one whose square underflows) adds nothing to s
__device__ __forceinline__ void entropy_term(float v, float& e, float& s) {
  const float sq = v * v;
  e += sq;
  const float t = sq * logf(sq);  // 0 * -inf = NaN for sq == 0: replaced below
  s += sq == 0.f ? 0.f : t;
}

// ln e - s / e for the sums of one map, clamped into [+0.0, hmax]. NaN (a poisoned map) passes through both clamps.
__device__ __forceinline__ float entropy_value(float e, float s, float hmax) {
  if (e == 0.f) return 0.f;
  float h = logf(e) - s / e;
  h = h < 0.f ? 0.f : h;
  h = h > hmax ? hmax : h;
  return h;
}

template <int N, int PAD>
__global__ __launch_bounds__((64 * CodeletCfg<N>::WAVES)) void k_entropy_codelet(MapGeom g, float hmax, float* __restrict__ out) {
  using Cfg = CodeletCfg<N>;
  __shared__ float slab[Cfg::WAVES][Cfg::WAVE_LDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  DCTS_CODELET_LANE(N, lane)

  const CodeletGroups walk = codelet_groups<N>(g.nmaps);
  for (long long grp = walk.first; grp < walk.ngroups; grp += walk.step) {
    const long long m1 = grp * Cfg::G + g1;
    const bool has = act && m1 < g.nmaps;
    DCTS_CODELET_LOAD(N, PAD, g, m1, c, has, xr)
    DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)
    // ---- epilogue: the row's e and s, coefficient by coefficient in the row's order ----------------
    float e = 0.f, s = 0.f;
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE { entropy_term(w[decltype(i)::value], e, s); });
    // idle lanes contribute nothing; the reduction is segmented, so a map's sums never see another map's lanes
    e = act ? e : 0.f;
    s = act ? s : 0.f;
    DCTS_MAP_SUM(N, e, c)
    DCTS_MAP_SUM(N, s, c)
    if (has && c == 0) out[m1] = entropy_value(e, s, hmax);
    wave_fence();
  }
}

// one wave per map over dense [hw] tiles of coefficients: lanes stride the tile, fixed-order wave sums
__global__ __launch_bounds__((64 * kReduceWaves)) void k_entropy_reduce(const float* __restrict__ coeff, long long nmaps, int hw,
                                                                        float hmax, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long m = wave; m < nmaps; m += nwaves) {
    const float* cm = coeff + m * hw;
    float e = 0.f, s = 0.f;
    for (int i = lane; i < hw; i += 64) entropy_term(cm[i], e, s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      e += __shfl_down(e, off, 64);
      s += __shfl_down(s, off, 64);
    }
    if (lane == 0) out[m] = entropy_value(e, s, hmax);
  }
}

template <int N, int PAD>
int launch_entropy(const MapGeom& g, float* out, hipStream_t st) {
  const float hmax = float(log(double(N) * double(N)));
  return launch_codelet_grid<N>(k_entropy_codelet<N, PAD>, g.nmaps, st, g, hmax, out);
}

}  // namespace

namespace dctsi {

int dispatch_entropy(int HP, int pad, const MapGeom& g, float* out, hipStream_t st) {
  return switch_codelet_size(HP, pad, [&](auto n, auto p) {
    return launch_entropy<decltype(n)::value, decltype(p)::value>(g, out, st);
  });
}

int launch_entropy_reduce(const float* coeff, long long nmaps, int hw, float* out, hipStream_t st) {
  const unsigned blocks = grid_blocks(nmaps, kReduceWaves, kReduceMaxBlocks);  // one wave per map
  hipLaunchKernelGGL(k_entropy_reduce, dim3(blocks), dim3(64 * kReduceWaves), 0, st, coeff, nmaps, hw,
                     float(log(double(hw))), out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
