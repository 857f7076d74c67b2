// nhwc.hip - per-map DCT energy of channels-last feature maps (dcts_energy_nhwc, include/dctscore.h): element (n, c, h, w) is
// x[n*strideN + h*strideH + w*strideW + c], fp32, fp16 or bf16 through one loader. Every element becomes fp32 exactly and all
// arithmetic is fp32. A map's value depends on that map alone: not on N, C_total, the channel slice, its position in a wave
// or block, or the launch count. No atomics.
//
//   k_nhwc_lane<N>    edges 2, 4, 7, 8. Lane = channel: the 64 lanes of a wave are 64 consecutive channels of one sample, a
//                     lane holds its whole map in registers, so every load instruction is one contiguous run of 64 elements.
//                     Both passes run in registers (lane_energy, codelet_schedule.hpp): no LDS, no cross-lane step.
//   k_nhwc_block<N>   edges 14, 16, 28, 32. A workgroup takes one sample and CB consecutive channels, loads the [N*N][CB]
//                     block with lanes along the channel axis first (each pixel one contiguous run of CB elements), and
//                     writes it into LDS as CB maps. After one barrier each wave owns G = 64 / N of those maps and runs the
//                     passes and the energy epilogue of codelet_schedule.hpp on them, xr[r] read from LDS; its transpose
//                     slab overlays the maps it has just read.
//   k_nhwc_strip      edge 56. One sample and 4 channels per workgroup, one wave per map; the block goes through LDS in
//                     strips of 8 rows from which each wave picks its map's column values, then the same passes and
//                     epilogue through the wave's own transpose slab.
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

template <int DT>
struct NhwcElem {
  using type = uint16_t;
};
template <>
struct NhwcElem<DCTS_DTYPE_F32> {
  using type = float;
};

template <int DT>
__device__ __forceinline__ float load_elem(const typename NhwcElem<DT>::type* p) {
  if constexpr (DT == DCTS_DTYPE_F32)
    return *p;
  else
    return half_to_float<DT>(*p);
}

constexpr int kLaneWaves = kNhwcLaneWaves;  // waves per workgroup of the lane = channel kernel (grid_caps.h)

template <int N, int DT>
__global__ __launch_bounds__(64 * kLaneWaves) void k_nhwc_lane(NhwcGeom g, float* __restrict__ out) {
  using T = typename NhwcElem<DT>::type;
  const int lane = threadIdx.x & 63;
  const long long chunks = (g.c_count + 63) / 64;  // 64-channel runs per sample: the fastest-varying index
  const long long items = g.N * chunks;
  const long long wave_gid = (long long)blockIdx.x * kLaneWaves + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * kLaneWaves;

  for (long long it = wave_gid; it < items; it += nwaves) {
    const long long n = it / chunks;
    const int j = (int)(it - n * chunks) * 64 + lane;
    const bool has = j < g.c_count;
    // tail lanes load a valid channel instead; their results are never stored
    const T* p = reinterpret_cast<const T*>(g.x) + n * g.strideN + (long long)g.c_begin + (has ? j : g.c_count - 1);
    float v[N * N];
    dcts::static_for<N * N>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int h = decltype(i)::value / N, w = decltype(i)::value % N;
      v[h * N + w] = load_elem<DT>(p + (long long)h * g.strideH + (long long)w * g.strideW);
    });
    const float e = lane_energy<N>(v);
    if (has) out[n * g.c_count + j] = e;
  }
}

// The channel block of k_nhwc_block. CB: channels per workgroup, so that a pixel's run is at least 64 B where 64 KiB of
// static LDS allow it (14, 16: 32 channels, 128 B fp32 / 64 B half; 28: 16 channels, 64 B / 32 B; 32: 8 channels, 32 B / 16 B:
// sixteen 32 x 32 maps with any padding are beyond 64 KiB). One wave per group of G maps. MS: floats per map in LDS, at least
// CodeletCfg's MAP_LDS (the wave's transpose slab, G * MAP_LDS floats, overlays its G maps), searched so that the staging
// stores - a half-wave is 32 / CB pixels x CB channels - fall on 32 distinct banks; the pass-1 reads (lane = column of G maps)
// are then 2-way at 14, 16, 28 and conflict-free at 32.
template <int N>
struct NhwcBlockCfg {
  using Cfg = CodeletCfg<N>;
  static constexpr int CB = nhwc_block_cb(N);  // grid_caps.h: N <= 16 ? 32 : (N <= 28 ? 16 : 8)
  static constexpr int WAVES = CB / Cfg::G;
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int MS = N == 14 ? 239 : N == 16 ? 273 : N == 28 ? 926 : 1060;
  static constexpr int PSTEP = THREADS / CB;                    // pixels a workgroup loads per step
  static constexpr int STEPS = (N * N + PSTEP - 1) / PSTEP;
  static_assert(N == 14 || N == 16 || N == 28 || N == 32, "MS is searched per edge");
  static_assert(CB % Cfg::G == 0 && THREADS % CB == 0 && MS >= Cfg::MAP_LDS && MS >= N * N, "block geometry");
  static_assert(CB * MS * 4 <= 65536, "64 KiB of static LDS per workgroup");
};

constexpr int kStageLoads = 13;  // staging loads a lane keeps in flight

template <int N, int DT>
__global__ __launch_bounds__((NhwcBlockCfg<N>::THREADS)) void k_nhwc_block(NhwcGeom g, float* __restrict__ out) {
  using T = typename NhwcElem<DT>::type;
  using B = NhwcBlockCfg<N>;
  using Cfg = CodeletCfg<N>;
  constexpr int G = Cfg::G, CB = B::CB, MS = B::MS;
  __shared__ float blk[CB * MS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ch = threadIdx.x % CB, p0 = threadIdx.x / CB;  // staging role: lanes run along the channel axis first
  DCTS_CODELET_LANE(N, lane)                               // codelet role: (map, column) in pass 1, (map, row) in pass 2
  float* my = blk + wave * G * MS;                         // the wave's G maps, then its transpose slab

  const long long cblocks = (g.c_count + CB - 1) / CB;     // channel blocks per sample: the fastest-varying index
  const long long items = g.N * cblocks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long n = it / cblocks;
    const int c0 = (int)(it - n * cblocks) * CB;
    // ---- stage the [N*N][CB] block as CB maps; channels past the slice load its last channel instead ------------
    {
      const int jc = c0 + ch < g.c_count ? c0 + ch : g.c_count - 1;
      const T* p = reinterpret_cast<const T*>(g.x) + n * g.strideN + (long long)g.c_begin + jc;
      float* dstm = blk + ch * MS;
      // kStageLoads loads in flight per lane, then their LDS stores: all STEPS at once cost 165 VGPRs at 28 x 28
      dcts::static_for<(B::STEPS + kStageLoads - 1) / kStageLoads>([&](auto ic) DCTS_LAMBDA_INLINE {
        constexpr int k0 = decltype(ic)::value * kStageLoads;
        constexpr int cnt = B::STEPS - k0 < kStageLoads ? B::STEPS - k0 : kStageLoads;
        float tmp[cnt];
        dcts::static_for<cnt>([&](auto i) DCTS_LAMBDA_INLINE {
          constexpr int k = k0 + decltype(i)::value;
          const int pix = p0 + k * B::PSTEP;
          if ((k + 1) * B::PSTEP <= N * N || pix < N * N) {
            const int h = pix / N, w = pix - h * N;
            tmp[k - k0] = load_elem<DT>(p + (long long)h * g.strideH + (long long)w * g.strideW);
          }
        });
        dcts::static_for<cnt>([&](auto i) DCTS_LAMBDA_INLINE {
          constexpr int k = k0 + decltype(i)::value;
          const int pix = p0 + k * B::PSTEP;
          if ((k + 1) * B::PSTEP <= N * N || pix < N * N) dstm[pix] = tmp[k - k0];
        });
        __builtin_amdgcn_sched_barrier(0);  // or the scheduler hoists the next chunk's loads above these stores
      });
    }
    __syncthreads();

    // ---- the wave's own maps: xr[r] from LDS, lane = column, then the shared passes and epilogue ----------------------
    const int jm = c0 + wave * G + g1;
    const bool has = act && jm < g.c_count;
    float xr[N];
    {
      const float* src = my + (act ? g1 : 0) * MS + (act ? c : 0);
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int r = decltype(i)::value;
        xr[r] = src[r * N];
      });
    }
    wave_fence();  // the slab overlays the maps just read
    DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)
    DCTS_CODELET_ENERGY(N, w, c, act, e)
    if (has && c == 0) out[n * g.c_count + jm] = e * Cfg::SCALE;
    __syncthreads();  // the next item's staging overwrites every wave's maps
  }
}

// The strips of k_nhwc_strip (56 x 56: a channel block of whole maps does not fit in LDS). One wave owns one map (lane =
// column, G = 1 as in the fp32 kernel) and needs its own 56 x 57 transpose slab, 12.8 KB: four slabs are 51 KB, so a
// workgroup takes one sample and CB = 4 consecutive channels - runs of 16 B (fp32) or 8 B (half). (Eight waves on four
// slabs in two rounds were built: the column values of the waiting waves stay live through both passes, 256 VGPRs and
// 180 B of scratch per lane. Dropped.) The block goes through LDS in strips of R = 8 rows, [CB][R * 56] floats with CS
// floats per channel: CS = 8 mod 32 puts the staging stores of a half-wave (8 pixels x 4 channels) on 32 distinct banks, and
// a wave's reads (one channel, consecutive columns) are conflict-free. Each wave picks its map's values of the strip into xr.
struct NhwcStripCfg {
  static constexpr int N = 56, CB = kNhwcStripCb, R = 8, WAVES = CB, THREADS = 64 * WAVES, CS = 456;
  static constexpr int PSTEP = THREADS / CB;                     // pixels a workgroup loads per step
  static constexpr int STEPS = (R * N + PSTEP - 1) / PSTEP;      // per strip
  static_assert(N % R == 0 && CS >= R * N, "strip geometry");
  static_assert((WAVES * CodeletCfg<N>::WAVE_LDS + CB * CS) * 4 <= 65536, "64 KiB of static LDS per workgroup");
};

template <int DT>
__global__ __launch_bounds__(NhwcStripCfg::THREADS) void k_nhwc_strip(NhwcGeom g, float* __restrict__ out) {
  using T = typename NhwcElem<DT>::type;
  using B = NhwcStripCfg;
  constexpr int N = B::N;
  using Cfg = CodeletCfg<N>;
  constexpr int CB = B::CB, R = B::R, CS = B::CS;
  static_assert(Cfg::G == 1, "one map per wave");
  __shared__ float slab[B::WAVES][Cfg::WAVE_LDS];
  __shared__ float strip[CB * CS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ch = threadIdx.x % CB, p0 = threadIdx.x / CB;  // staging role: lanes run along the channel axis first
  constexpr int g1 = 0;                                    // codelet role, one map per wave: column in pass 1, row in pass 2
  const int c = lane;
  const bool act = lane < N;

  const long long cblocks = (g.c_count + CB - 1) / CB;     // channel blocks per sample: the fastest-varying index
  const long long items = g.N * cblocks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long n = it / cblocks;
    const int c0 = (int)(it - n * cblocks) * CB;
    const int jc = c0 + ch < g.c_count ? c0 + ch : g.c_count - 1;  // channels past the slice load its last channel instead
    const T* p = reinterpret_cast<const T*>(g.x) + n * g.strideN + (long long)g.c_begin + jc;
    float xr[N];
    dcts::static_for<N / R>([&](auto is) DCTS_LAMBDA_INLINE {
      constexpr int h0 = decltype(is)::value * R;
      float tmp[B::STEPS];
      dcts::static_for<B::STEPS>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(i)::value;
        const int pix = p0 + k * B::PSTEP;
        if ((k + 1) * B::PSTEP <= R * N || pix < R * N) {
          const int h = pix / N, w = pix - h * N;
          tmp[k] = load_elem<DT>(p + (long long)(h0 + h) * g.strideH + (long long)w * g.strideW);
        }
      });
      if (h0 != 0) __syncthreads();  // every wave has picked the strip before
      dcts::static_for<B::STEPS>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(i)::value;
        const int pix = p0 + k * B::PSTEP;
        if ((k + 1) * B::PSTEP <= R * N || pix < R * N) strip[ch * CS + pix] = tmp[k];
      });
      __syncthreads();
      const float* src = strip + wave * CS + (act ? c : 0);
      dcts::static_for<R>([&](auto ir) DCTS_LAMBDA_INLINE {
        constexpr int r = decltype(ir)::value;
        xr[h0 + r] = src[r * N];
      });
    });

    const int jm = c0 + wave;
    const bool has = jm < g.c_count;
    float* my = slab[wave];
    DCTS_CODELET_PASSES(N, xr, w, my, g1, c, act)
    DCTS_CODELET_ENERGY(N, w, c, act, e)
    if (has && c == 0) out[n * g.c_count + jm] = e * Cfg::SCALE;
    __syncthreads();  // the next item's strips follow
  }
}

template <int N, int DT>
int launch_nhwc_lane(const NhwcGeom& g, float* out, hipStream_t st) {
  const long long items = g.N * ((g.c_count + 63LL) / 64);  // one wave per sample and 64-channel run
  const unsigned blocks = grid_blocks(items, kLaneWaves, (long long)num_cus() * CodeletCfg<N>::GRID_WAVES_PER_CU / kLaneWaves);
  hipLaunchKernelGGL((k_nhwc_lane<N, DT>), dim3(blocks), dim3(64 * kLaneWaves), 0, st, g, out);
  return (int)hipGetLastError();
}

template <int N, int DT>
int launch_nhwc_block(const NhwcGeom& g, float* out, hipStream_t st) {
  using B = NhwcBlockCfg<N>;
  const long long items = g.N * ((g.c_count + (long long)B::CB - 1) / B::CB);  // one workgroup per sample and channel block
  // the codelet kernels' grid rule, counted in their workgroups of CodeletCfg<N>::WAVES one-group waves
  hipLaunchKernelGGL((k_nhwc_block<N, DT>), dim3(codelet_grid<N>(items * CodeletCfg<N>::WAVES)), dim3(B::THREADS), 0, st, g, out);
  return (int)hipGetLastError();
}

template <int DT>
int launch_nhwc_strip(const NhwcGeom& g, float* out, hipStream_t st) {
  using B = NhwcStripCfg;
  const long long items = g.N * ((g.c_count + (long long)B::CB - 1) / B::CB);  // one workgroup per sample and channel block
  hipLaunchKernelGGL((k_nhwc_strip<DT>), dim3(codelet_grid<B::N>(items * CodeletCfg<B::N>::WAVES)), dim3(B::THREADS), 0, st, g, out);
  return (int)hipGetLastError();
}

template <int DT>
int dispatch_nhwc_dt(int N, const NhwcGeom& g, float* out, hipStream_t st) {
  switch (N) {
#define DCTS_CASE(N_) \
  case N_:            \
    return launch_nhwc_lane<N_, DT>(g, out, st);
    DCTS_NHWC_LANE_SIZES(DCTS_CASE)
#undef DCTS_CASE
#define DCTS_CASE(N_) \
  case N_:            \
    return launch_nhwc_block<N_, DT>(g, out, st);
    DCTS_NHWC_BLOCK_SIZES(DCTS_CASE)
#undef DCTS_CASE
    case NhwcStripCfg::N:
      return launch_nhwc_strip<DT>(g, out, st);
    default:
      return DCTS_E_UNSUPPORTED;
  }
}

}  // namespace

namespace dctsi {

int dispatch_nhwc(int N, int dtype, const NhwcGeom& g, float* out, hipStream_t st) {
  switch (dtype) {
    case DCTS_DTYPE_F32: return dispatch_nhwc_dt<DCTS_DTYPE_F32>(N, g, out, st);
    case DCTS_DTYPE_F16: return dispatch_nhwc_dt<DCTS_DTYPE_F16>(N, g, out, st);
    case DCTS_DTYPE_BF16: return dispatch_nhwc_dt<DCTS_DTYPE_BF16>(N, g, out, st);
    default: return DCTS_E_UNSUPPORTED;
  }
}

}  // namespace dctsi
