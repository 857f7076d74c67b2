// half.hip - per-map DCT energy of IEEE fp16 and bfloat16 feature maps (dcts_energy_typed, include/dctscore.h).
//
//   k_energy_half    the fp32 codelet kernel's schedule with the slab geometry, grid rule, fence and segmented reduction of
//                    codelet_schedule.hpp (plain transposing stores, the fp32 kernel's energy epilogue). What this unit adds
//                    is the load: an element becomes fp32 EXACTLY (fp16 -> fp32 and bf16 -> fp32 are both exact, fp16
//                    subnormals included: they are fp32 normals) and every instruction after that is fp32 in the fp32
//                    kernel's order. A map's value depends on that map alone: not on N, the channel slice, its position
//                    in the wave or the launch count.
//                    The load is one 2-byte load per lane and row: the fp32 kernel's instruction count for half the
//                    bytes, any 2-byte-aligned base. (Packed pairs - one dword = two adjacent columns, split in registers
//                    after a DPP exchange - were built and measured: 3-19 % slower at 56, 28, 32, 16, 8 and 4, within
//                    the spread of the 2-byte loads at 14, 7 and 2. Dropped; DESIGN.md 7e has the numbers.)
//   k_upcast_half    the staged route of every other shape: upcasts a run of maps of the scored channel slice (any row
//                    pitch) into a dense fp32 array in the caller's workspace; the fp32 entry point then scores that.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "codelet_schedule.hpp"
#include "dct_codelets.hpp"
#include "dcts_internal.h"
#include "grid_caps.h"
#include "half_convert.hpp"

using namespace dctsi;

namespace {

template <int N, int DT>
__global__ __launch_bounds__((64 * CodeletCfg<N>::WAVES)) void k_energy_half(HalfGeom g, float* __restrict__ out) {
  using Cfg = CodeletCfg<N>;
  constexpr int G = Cfg::G, S = Cfg::S, MAP_LDS = Cfg::MAP_LDS, WAVES = Cfg::WAVES;
  __shared__ float slab[WAVES][Cfg::WAVE_LDS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  const int g1 = lane / N, c = lane - g1 * N;  // square tile: (map, column) in pass 1, (map, row) in pass 2
  const bool act = g1 < G;

  const long long ngroups = (g.nmaps + G - 1) / G;
  const long long wave_gid = (long long)blockIdx.x * WAVES + wave;
  const long long nwaves = (long long)gridDim.x * WAVES;

  for (long long grp = wave_gid; grp < ngroups; grp += nwaves) {
    // ---- pass 1: column DCT-II, lane = column ---------------------------------------------------
    const long long m1 = grp * G + g1;
    const bool has = act && m1 < g.nmaps;
    // lanes without a map load some valid map instead; their results are never stored
    const uint16_t* p = map_base(g, has ? m1 : g.nmaps - 1) + (has ? c : 0);
    float xr[N];
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(i)::value;
      xr[r] = half_to_float<DT>(p[r * N]);
    });
    float y[N];
    dcts::Dct2<N>::run(xr, y);
    y[0] *= dcts::kInvSqrt2;
    if (act) {
      float* dst = my + g1 * MAP_LDS + c;
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int kk = decltype(i)::value;
        dst[kk * S] = y[kk];
      });
    }
    wave_fence();

    // ---- pass 2: row DCT-II, lane = row u ------------------------------------------------------
    float z[N], w[N];
    {
      const float* src = my + (act ? g1 : 0) * MAP_LDS + (act ? c : 0) * S;
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int cc = decltype(i)::value;
        z[cc] = src[cc];
      });
    }
    dcts::Dct2<N>::run(z, w);
    w[0] *= dcts::kInvSqrt2;
    float e = 0.f;
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int l = decltype(i)::value;
      e = fmaf(w[l], w[l], e);
    });
    if (!act) e = 0.f;
    // segmented reduction over the N lanes of each map (lane c == 0 ends with the sum)
    DCTS_MAP_SUM(N, e, c)
    if (has && c == 0) {
      constexpr float sc = float(4.0 / (double(N) * double(N)));
      out[m1] = e * sc;
    }
    wave_fence();
  }
}

// dst[(m * H + h) * W + w] = float(map m of the slice)[h][w] for the g.nmaps maps of g: one element per thread and step,
// consecutive threads consecutive elements of a row
template <int DT>
__global__ __launch_bounds__(kUpcastThreads) void k_upcast_half(HalfGeom g, int H, int W, long long strideH, float* __restrict__ dst) {
  const long long hw = (long long)H * W;
  const long long total = g.nmaps * hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / hw;
    const int e = (int)(i - m * hw);
    const int h = e / W, w = e - h * W;
    dst[i] = half_to_float<DT>(map_base(g, m)[h * strideH + w]);
  }
}

template <int N, int DT>
int launch_half(const HalfGeom& g, float* out, hipStream_t st) {
  using Cfg = CodeletCfg<N>;
  const long long ngroups = (g.nmaps + Cfg::G - 1) / Cfg::G;
  hipLaunchKernelGGL((k_energy_half<N, DT>), dim3(codelet_grid<N>(ngroups)), dim3(64 * Cfg::WAVES), 0, st, g, out);
  return (int)hipGetLastError();
}

}  // namespace

namespace dctsi {

int dispatch_half(int N, int dtype, const HalfGeom& g, float* out, hipStream_t st) {
  if (dtype != DCTS_DTYPE_F16 && dtype != DCTS_DTYPE_BF16) return DCTS_E_UNSUPPORTED;
#define DCTS_CASE(N_)                                                                       \
  case N_:                                                                                  \
    return dtype == DCTS_DTYPE_F16 ? launch_half<N_, DCTS_DTYPE_F16>(g, out, st)            \
                                   : launch_half<N_, DCTS_DTYPE_BF16>(g, out, st);
  switch (N) {
    DCTS_HALF_SIZES(DCTS_CASE)
    default:
      return DCTS_E_UNSUPPORTED;
  }
#undef DCTS_CASE
}

int launch_upcast_half(int dtype, const HalfGeom& g, int H, int W, long long strideH, float* dst, hipStream_t st) {
  if (dtype != DCTS_DTYPE_F16 && dtype != DCTS_DTYPE_BF16) return DCTS_E_UNSUPPORTED;
  const long long total = g.nmaps * (long long)H * W;
  const unsigned blocks = grid_blocks(total, kUpcastThreads, (long long)num_cus() * kUpcastBlocksPerCu);  // one thread per element and step
  if (dtype == DCTS_DTYPE_F16)
    hipLaunchKernelGGL(k_upcast_half<DCTS_DTYPE_F16>, dim3(blocks), dim3(kUpcastThreads), 0, st, g, H, W, strideH, dst);
  else
    hipLaunchKernelGGL(k_upcast_half<DCTS_DTYPE_BF16>, dim3(blocks), dim3(kUpcastThreads), 0, st, g, H, W, strideH, dst);
  return (int)hipGetLastError();
}

}  // namespace dctsi
