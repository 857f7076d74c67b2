// half.hip - per-map DCT energy of IEEE fp16 and bfloat16 feature maps (dcts_energy_typed, include/dctscore.h).
//
//   k_energy_half    the two-pass schedule of codelet_schedule.hpp (its group loop, passes and energy epilogue). What this
//                    unit adds is the load: an element becomes fp32 EXACTLY (fp16 -> fp32 and bf16 -> fp32 are both exact, fp16
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
  __shared__ float slab[Cfg::WAVES][Cfg::WAVE_LDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  DCTS_CODELET_LANE(N, lane)

  const CodeletGroups walk = codelet_groups<N>(g.nmaps);
  for (long long grp = walk.first; grp < walk.ngroups; grp += walk.step) {
    const long long m1 = grp * Cfg::G + g1;
    const bool has = act && m1 < g.nmaps;
    // lanes without a map load some valid map instead; their results are never stored
    const uint16_t* p = map_base(g, has ? m1 : g.nmaps - 1) + (has ? c : 0);
    float xr[N];
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(i)::value;
      xr[r] = half_to_float<DT>(p[r * N]);
    });
    DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)
    DCTS_CODELET_ENERGY(N, w, c, act, e)
    if (has && c == 0) out[m1] = e * Cfg::SCALE;
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
  return launch_codelet_grid<N>(k_energy_half<N, DT>, g.nmaps, st, g, out);
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
