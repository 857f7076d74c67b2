// lowpass.hip - the low-pass DCT signature of every map (dcts_dct2d_lowpass_f32, include/dctscore.h):
//   out[m][u][v] = dct_2d(map m, norm='ortho')[u][v]  for u < Kh = min(K, H), v < Kw = min(K, W):
// the K x K lowest frequencies of every map and nothing else, so that a map is read once and K^2 floats are written.
//
//   k_lowpass_codelet  the two-pass schedule of codelet_schedule.hpp (its group loop, load and passes): a lane ends with
//                      the N unnormalised coefficients of row u of its map in registers. What this unit adds is the
//                      epilogue: the lanes of the rows u < K store their first K coefficients, scaled as
//                      k_energy_codelet<..., STORE_COEFF> scales them. K is a run-time argument: the stores are a chain
//                      that ends at the first v >= K. A lane's coefficients depend on nothing but the map: the signature
//                      of a map is the same bits for any N, channel slice, position in the wave or launch.
//   k_lowpass_gather   the fallback's "reduction" (every shape without a codelet, up to 512, and row-pitched views): one
//                      wave per map copies the [Kh][Kw] corner of dense tiles of orthonormal coefficients in the workspace.
// drop_dc (both kernels; a run-time argument, so that the call with the flag runs the very code of the call without it and
// every element it does not zero has the same bits): element [0][0] of every signature is written as +0.0, and a FLAT map -
// every element equal - gets an all-+0.0 signature. Flat is decided on the spatial map, exactly: every element equals the
// map's first one, which is max == min for a map without a NaN and false for a map that holds one (its signature stays NaN).
// Never on coefficients: the AC terms of a constant map are exactly 0 for power-of-two edges only, the odd-base codelets
// leave round-off there.
// No atomics.
#include <hip/hip_runtime.h>
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

// o[v] = w[v] * sc for v = V, V + 1, ... < K: w lives in registers, so the index is static and the chain ends at the first
// v >= K (K is wave-uniform: scalar branches). zero: the flat rule; drop: this lane holds row 0 and loses [0][0].
template <int N, int V>
__device__ __forceinline__ void lowpass_store_row(const float (&w)[N], float sc, int K, bool zero, bool drop, float* __restrict__ o) {
  if constexpr (V < N) {
    if (V < K) {
      float t = w[V] * sc;
      if (zero || (V == 0 && drop)) t = 0.f;
      o[V] = t;
      lowpass_store_row<N, V + 1>(w, sc, K, zero, drop, o);
    }
  }
}

// The same chain four coefficients at a time, one 16-byte store each, for K a multiple of 4 on a 16-byte-aligned output (the
// row of a lane then starts on a 16-byte boundary): the same products, a quarter of the store instructions. Only where a
// wave holds several maps (kLowpassVec): there the stores are what the epilogue costs (K = 8 against the dword chain of the
// same kernel and against a build without this chain: 14 x 14 and 16 x 16 a quarter to a third faster, 28 x 28 a few
// percent); with one map per wave 8 of 64 lanes store, and the build with both chains was 5 % slower at 56 x 56.
template <int N>
constexpr bool kLowpassVec = CodeletCfg<N>::G >= 2;
template <int N, int V>
__device__ __forceinline__ void lowpass_store_row4(const float (&w)[N], float sc, int K, bool zero, bool drop, float* __restrict__ o) {
  if constexpr (V + 4 <= N) {
    if (V + 4 <= K) {
      float4 t = make_float4(w[V] * sc, w[V + 1] * sc, w[V + 2] * sc, w[V + 3] * sc);
      if (zero) t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (V == 0 && drop) t.x = 0.f;
      *reinterpret_cast<float4*>(o + V) = t;
      lowpass_store_row4<N, V + 4>(w, sc, K, zero, drop, o);
    }
  }
}

// K: already clamped to N by the dispatcher
template <int N>
__global__ __launch_bounds__((64 * CodeletCfg<N>::WAVES)) void k_lowpass_codelet(MapGeom g, int K, int drop_dc, float* __restrict__ out) {
  using Cfg = CodeletCfg<N>;
  __shared__ float slab[Cfg::WAVES][Cfg::WAVE_LDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  DCTS_CODELET_LANE(N, lane)
  // the lanes of this lane's map, as a mask over the wave
  const unsigned long long seg = act ? ((N == 64 ? ~0ull : ((1ull << (N & 63)) - 1ull)) << (g1 * N)) : 0ull;

  const bool vec = kLowpassVec<N> && (K & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;  // wave-uniform

  const CodeletGroups walk = codelet_groups<N>(g.nmaps);
  for (long long grp = walk.first; grp < walk.ngroups; grp += walk.step) {
    const long long m1 = grp * Cfg::G + g1;
    const bool has = act && m1 < g.nmaps;
    DCTS_CODELET_LOAD(N, 0, g, m1, c, has, xr)
    bool flat = false;
    if (drop_dc) {
      // every element of the column equals the map's first element (column 0's first register), then every column does
      const float x00 = __shfl(xr[0], g1 * N, 64);
      bool same = true;
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE { same = same && (xr[decltype(i)::value] == x00); });
      flat = act && (__ballot(same) & seg) == seg;
    }
    DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)
    // ---- epilogue: the first K coefficients of the rows u = c < K ------------------------------------
    if (has && c < K) {
      constexpr float sc = float(2.0 / dcts::cx_sqrt(double(N) * double(N)));
      float* o = out + ((long long)m1 * K + c) * K;
      if constexpr (kLowpassVec<N>) {
        if (vec)
          lowpass_store_row4<N, 0>(w, sc, K, flat, drop_dc && c == 0, o);
        else
          lowpass_store_row<N, 0>(w, sc, K, flat, drop_dc && c == 0, o);
      } else {
        lowpass_store_row<N, 0>(w, sc, K, flat, drop_dc && c == 0, o);
      }
    }
    wave_fence();
  }
}

// One wave per map: the [Kh][Kw] corner of tile m of `coeff` (dense [HP][WP]) to out[m]. g: the call's whole view, its map
// `first + m` is the spatial map of tile m (drop_dc reads it once more for the flat rule; rows of pitch g.strideH).
__global__ __launch_bounds__((64 * kReduceWaves)) void k_lowpass_gather(const float* __restrict__ coeff, long long nmaps, long long first,
                                                                        MapGeom g, int Kh, int Kw, int drop_dc, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const int kk = Kh * Kw;
  for (long long m = wave; m < nmaps; m += nwaves) {
    bool flat = false;
    if (drop_dc) {
      const float* p = map_base(g, first + m);
      const float x00 = p[0];
      bool same = true;
      const int hw = g.H * g.W;
      for (int i = lane; i < hw; i += 64) {
        const int r = i / g.W;
        same = same && (p[(long long)r * g.strideH + (i - r * g.W)] == x00);
      }
      flat = __all(same);
    }
    const float* cm = coeff + m * ((long long)g.H * g.W);
    float* o = out + (first + m) * (long long)kk;
    for (int i = lane; i < kk; i += 64) {
      const int u = i / Kw;
      float t = cm[(long long)u * g.W + (i - u * Kw)];
      if (drop_dc && (flat || i == 0)) t = 0.f;
      o[i] = t;
    }
  }
}

template <int N>
int launch_lowpass(const MapGeom& g, int K, int drop_dc, float* out, hipStream_t st) {
  const int kc = K < N ? K : N;
  return launch_codelet_grid<N>(k_lowpass_codelet<N>, g.nmaps, st, g, kc, drop_dc, out);
}

}  // namespace

namespace dctsi {

int dispatch_lowpass(int HP, const MapGeom& g, int K, int drop_dc, float* out, hipStream_t st) {
  return switch_codelet_size(HP, 0, [&](auto n, auto p) {
    if constexpr (decltype(p)::value == 0)
      return launch_lowpass<decltype(n)::value>(g, K, drop_dc, out, st);
    else
      return (int)DCTS_E_UNSUPPORTED;  // no odd front pad here
  });
}

int launch_lowpass_gather(const float* coeff, long long nmaps, long long first, const MapGeom& g, int Kh, int Kw, int drop_dc,
                          float* out, hipStream_t st) {
  const unsigned blocks = grid_blocks(nmaps, kReduceWaves, kReduceMaxBlocks);  // one wave per map
  hipLaunchKernelGGL(k_lowpass_gather, dim3(blocks), dim3(64 * kReduceWaves), 0, st, coeff, nmaps, first, g, Kh, Kw, drop_dc, out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
