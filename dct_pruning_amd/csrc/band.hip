// band.hip - K weighted energies per map in one pass (dcts_band_energy_f32, include/dctscore.h):
//   out[m][b] = sum_{u,v} weights[b][u][v] * c[u][v]^2,  c = dct_2d(map m, norm='ortho'),  b = 0 ... K-1.
// With one-hot weights (dct_pruning_amd/bands.py) that is the energy of K frequency bands of every map.
//
//   k_band_codelet   the two-pass schedule of codelet_schedule.hpp (its group loop, load and passes): a lane ends with the
//                    N coefficients of row u of its map in registers. What this unit adds is the
//                    epilogue: KB accumulators e[b] = fma(wt[b][u][l], w[l] * w[l], e[b]) instead of one, then
//                    the segmented wave reduction once per band and K stores per map. KB = K rounded up to 1, 2, 4, 8;
//                    the bands above K have zero weights and are not stored. A band's chain of FMAs and its reduction
//                    tree depend on nothing but the map's row and the band's weights: the result of a map is the same
//                    bits for any N, channel slice, K, position in the wave or launch.
//   k_band_table     where the weight rows live ("band energies"): in GLOBAL memory, re-laid by this kernel
//                    from the caller's [K][HP][WP] into T[l][u][KB] at the head of the workspace. A lane (row u) then
//                    reads the KB weights of coefficient (u, l) as ONE 4 * KB-byte vector, and the lanes of a map read
//                    consecutive vectors: every load instruction is fully coalesced. The table is at most 128 KiB and is
//                    read by every wave, so it stays in L2 (and, for the small tiles, in the vector L1). LDS was not
//                    an option at the large edges (8 x 64 x 64 x 4 B = 128 KiB beside a 17 KiB transpose slab per wave)
//                    and costs occupancy long before that.
//   k_band_reduce    the fallback's reduction (every shape without a codelet, up to 512): reads each coefficient of a
//                    chunk ONCE and produces all K values of a map; one wave per map, fixed-order sums.
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

template <int KB>
struct WVec {
  float v[KB];
};

// the KB weights of one coefficient: one aligned vector load of 4 * KB bytes
template <int KB>
__device__ __forceinline__ WVec<KB> load_weights(const float* __restrict__ p) {
  WVec<KB> r;
  if constexpr (KB == 1) {
    r.v[0] = p[0];
  } else if constexpr (KB == 2) {
    const float2 a = *reinterpret_cast<const float2*>(p);
    r.v[0] = a.x;
    r.v[1] = a.y;
  } else {
    dcts::static_for<KB / 4>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int q = decltype(i)::value;
      const float4 a = *reinterpret_cast<const float4*>(p + 4 * q);
      r.v[4 * q] = a.x;
      r.v[4 * q + 1] = a.y;
      r.v[4 * q + 2] = a.z;
      r.v[4 * q + 3] = a.w;
    });
  }
  return r;
}

// T[(l * HP + u) * KB + b] = weights[b][u][l] for b < K, 0 above
__global__ __launch_bounds__(256) void k_band_table(const float* __restrict__ weights, float* __restrict__ T, int HP,
                                                    int WP, int K, int KB) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= HP * WP * KB) return;
  const int b = idx % KB, lu = idx / KB;
  const int u = lu % HP, l = lu / HP;
  T[idx] = b < K ? weights[((long long)b * HP + u) * WP + l] : 0.f;
}

template <int N, int PAD, int KB>
__global__ __launch_bounds__((64 * CodeletCfg<N>::WAVES)) void k_band_codelet(MapGeom g, const float* __restrict__ T, int K,
                                                                           float* __restrict__ out) {
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
    float e[KB];
    dcts::static_for<KB>([&](auto ib) DCTS_LAMBDA_INLINE { e[decltype(ib)::value] = 0.f; });
    // The table does not depend on the group, so the compiler would hoist every weight load out of the grid-stride
    // loop and keep N * KB weights in registers for the kernel's lifetime (256 VGPRs and scratch at K = 8 from edge
    // 28 on). The empty asm makes the base opaque once per group: the loads stay here, served by L1 / L2.
    const float* Tg = T;
    asm volatile("" : "+s"(Tg));
    const float* Trow = Tg + c * KB;  // c < N always: in bounds for idle lanes too
    // The weight vectors come in chunks of CH coefficients (32 floats), double-buffered in registers: chunk i + 1 is in
    // flight while chunk i is consumed, and a scheduling barrier after each chunk keeps the scheduler from moving every
    // load of the row to the top.
    constexpr int CH = 32 / KB < N ? 32 / KB : N, NCH = (N + CH - 1) / CH;
    WVec<KB> wbuf[2][CH];
    auto fetch = [&](auto ci) DCTS_LAMBDA_INLINE {
      constexpr int ch = decltype(ci)::value;
      dcts::static_for<CH>([&](auto j) DCTS_LAMBDA_INLINE {
        constexpr int l = ch * CH + decltype(j)::value;
        if constexpr (l < N) wbuf[ch & 1][decltype(j)::value] = load_weights<KB>(Trow + l * (N * KB));
      });
    };
    fetch(std::integral_constant<int, 0>{});
    dcts::static_for<NCH>([&](auto ci) DCTS_LAMBDA_INLINE {
      constexpr int ch = decltype(ci)::value;
      if constexpr (ch + 1 < NCH) fetch(std::integral_constant<int, ch + 1>{});
      dcts::static_for<CH>([&](auto j) DCTS_LAMBDA_INLINE {
        constexpr int l = ch * CH + decltype(j)::value;
        if constexpr (l < N) {
          const float sq = w[l] * w[l];
          dcts::static_for<KB>([&](auto ib) DCTS_LAMBDA_INLINE {
            constexpr int b = decltype(ib)::value;
            e[b] = fmaf(wbuf[ch & 1][decltype(j)::value].v[b], sq, e[b]);
          });
        }
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    // segmented reduction over the N lanes of each map, once per band (lane c == 0 ends with the sums)
    dcts::static_for<KB>([&](auto ib) DCTS_LAMBDA_INLINE {
      constexpr int b = decltype(ib)::value;
      float eb = act ? e[b] : 0.f;
      DCTS_MAP_SUM(N, eb, c)
      e[b] = eb;
    });
    if (has && c == 0) {
      float* o = out + m1 * K;
      dcts::static_for<KB>([&](auto ib) DCTS_LAMBDA_INLINE {
        constexpr int b = decltype(ib)::value;
        if (b < K) o[b] = e[b] * Cfg::SCALE;
      });
    }
    wave_fence();
  }
}

// out[m][b] = sum_i weights[b][i] * coeff[m][i]^2 over dense [hw] coefficient tiles: one wave per map, lanes stride
// the tile, every coefficient read once for all K bands, fixed-order wave sums
__global__ __launch_bounds__((64 * kReduceWaves)) void k_band_reduce(const float* __restrict__ coeff, const float* __restrict__ weights,
                                                     long long nmaps, int hw, int K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long m = wave; m < nmaps; m += nwaves) {
    const float* cm = coeff + m * hw;
    float e[DCTS_BAND_MAX];
#pragma unroll
    for (int b = 0; b < DCTS_BAND_MAX; ++b) e[b] = 0.f;
    for (int i = lane; i < hw; i += 64) {
      const float v = cm[i];
      const float sq = v * v;
#pragma unroll
      for (int b = 0; b < DCTS_BAND_MAX; ++b)
        if (b < K) e[b] = fmaf(weights[(long long)b * hw + i], sq, e[b]);
    }
#pragma unroll
    for (int b = 0; b < DCTS_BAND_MAX; ++b) {
      float eb = e[b];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) eb += __shfl_down(eb, off, 64);
      if (lane == 0 && b < K) out[m * K + b] = eb;
    }
  }
}

template <int N, int PAD, int KB>
int launch_band(const MapGeom& g, const float* T, int K, float* out, hipStream_t st) {
  return launch_codelet_grid<N>(k_band_codelet<N, PAD, KB>, g.nmaps, st, g, T, K, out);
}

template <int N, int PAD>
int launch_band_k(int KB, const MapGeom& g, const float* T, int K, float* out, hipStream_t st) {
  switch (KB) {
    case 1:
      return launch_band<N, PAD, 1>(g, T, K, out, st);
    case 2:
      return launch_band<N, PAD, 2>(g, T, K, out, st);
    case 4:
      return launch_band<N, PAD, 4>(g, T, K, out, st);
    default:
      return launch_band<N, PAD, 8>(g, T, K, out, st);
  }
}

}  // namespace

namespace dctsi {

int band_kb(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : 8; }

size_t band_table_bytes(int HP, int WP, int K) { return align_up((size_t)HP * WP * band_kb(K) * 4, 256); }

int dispatch_band(int HP, int pad, const MapGeom& g, const float* weights, int K, float* table, float* out,
                  hipStream_t st) {
  const int KB = band_kb(K);
  const int cells = HP * HP * KB;
  hipLaunchKernelGGL(k_band_table, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, weights, table, HP, HP, K, KB);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  return switch_codelet_size(HP, pad, [&](auto n, auto p) {
    return launch_band_k<decltype(n)::value, decltype(p)::value>(KB, g, table, K, out, st);
  });
}

int launch_band_reduce(const float* coeff, const float* weights, long long nmaps, int hw, int K, float* out,
                       hipStream_t st) {
  const unsigned blocks = grid_blocks(nmaps, kReduceWaves, kReduceMaxBlocks);  // one wave per map
  hipLaunchKernelGGL(k_band_reduce, dim3(blocks), dim3(64 * kReduceWaves), 0, st, coeff, weights, nmaps, hw, K, out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
