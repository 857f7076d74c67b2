// codelet.hip - the register-resident codelet kernels behind include/dctscore.h: square tiles with both edges <= 64.
//
// Replaces the per-map Python loop of the reference hooks (utils/common.py:262-309):
//   c = [dct.dct_2d(output[i,j,:,:], norm='ortho') ...]; torch.sum(dct.mul(dct)).item()
// with one launch per hooked tensor: every (sample, channel) map gets its orthonormal
// 2-D DCT-II and the squared coefficients are reduced to one fp32 energy per map.
//
//   k_energy_codelet  maps with both edges <= 64 that have a codelet (codelet_sizes.h).
//                     One wave owns floor(64/edge) maps. Pass 1: lane = column, the lane
//                     holds the whole column in VGPRs (coalesced dword loads straight
//                     from HBM, row r of a map is one contiguous segment across lanes) and
//                     runs a straight-line factorised DCT-II (dct_codelets.hpp). The
//                     tile is transposed through a per-wave LDS slab (odd row stride ->
//                     conflict-free both ways). Pass 2: lane = row, second codelet, the
//                     squares are summed in-lane and then across the map's lanes with a
//                     segmented wave shuffle reduction. HBM traffic = the algorithmic
//                     4*H*W + 4 bytes per map; LDS traffic = one write + one read per
//                     element. codelet_schedule.hpp states the plain form of this schedule.
//   k_energy_lane_multi  7 x 7 and 9 x 9 maps, one lane per map (see below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "codelet_schedule.hpp"
#include "codelet_sizes.h"
#include "dct_codelets.hpp"
#include "dcts_internal.h"
#include "grid_caps.h"
#include "split_roles.hpp"

using namespace dctsi;

namespace {

// ---------------------------------------------------------------------------------------
// codelet family
// ---------------------------------------------------------------------------------------
// ds_write_addtid_b32 in the codelet kernel's transposing stores where a wave holds one map (edges 36 ... 64): same box,
// 200 MB launches, % of the HBM peak: 56: 60.7 -> 61.5-62.3, 48: 60.8 -> 63.0, 36: 52.9 -> 54.0, 64: 52.9 -> 54.2; the
// 4.3 GB in-step launch is unchanged within noise (the kernel is VALU-bound there). Bit-identical results.
// four lane-consecutive LDS stores at byte offsets O0..O3 from `base` (an LDS byte address below 64 KiB: M0[15:0])
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void lds_write_addtid4(unsigned base, float a, float b, float c, float d) {
  static_assert(O3 < 65536 && O0 >= 0, "16-bit offset field");
  asm volatile(
      "s_mov_b32 m0, %0\n\ts_nop 0\n\t"
      "ds_write_addtid_b32 %1 offset:%5\n\tds_write_addtid_b32 %2 offset:%6\n\t"
      "ds_write_addtid_b32 %3 offset:%7\n\tds_write_addtid_b32 %4 offset:%8"
      :
      : "s"(base), "v"(a), "v"(b), "v"(c), "v"(d), "n"(O0), "n"(O1), "n"(O2), "n"(O3)
      : "memory", "m0");
}

// One group of G maps: both passes, the LDS transpose and the reduction. The plain form of this body is stated in
// codelet_schedule.hpp (DCTS_CODELET_LOAD, _PASSES, _ENERGY), where band.hip, entropy.hip, half.hip and nhwc.hip
// take it from. This text is kept apart because bench.py measures these kernels and it leaves the plain form in two places:
// the ds_write_addtid stores at G == 1 (below), and two lane roles. Every caller passes HP == WP (the dispatchers refuse
// anything else; rect.hip serves non-square tiles), so the pass-2 role (g2, k, act2) equals the pass-1 role; folding the two,
// or calling the shared pieces, changes the instruction order of 55 to 90 of this unit's 149 kernels.
template <int HP, int WP, int PAD, bool STORE_COEFF>
__device__ __forceinline__ void codelet_group(const MapGeom& g, float* __restrict__ out, long long grp,
                                              float* my, int g1, int c, int g2, int k, bool act1, bool act2) {
  using Cfg = CodeletCfg<HP>;
  constexpr int G = Cfg::G, S = Cfg::S, MAP_LDS = Cfg::MAP_LDS;
  constexpr int W = WP - PAD;  // data row length == row stride (dense rows)
  // ---- pass 1: column DCT-II of length HP, lane = column -------------------------
  const long long m1 = grp * G + g1;
  float xr[HP];
  if constexpr (PAD == 0) {
    // No branch and no zero fill: lanes without a map (beyond G*WP, or past the last map of a ragged
    // group) load some valid map instead and their results are never stored. The kernel is
    // VALU-issue-bound; the HP v_mov 0 per iteration of the zero fill were 4-6 % of its instructions.
    const bool has = act1 && m1 < g.nmaps;
    const float* p = map_base(g, has ? m1 : g.nmaps - 1) + (has ? c : 0);
    dcts::static_for<HP>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(i)::value;
      xr[r] = p[r * W];
    });
  } else {
    const bool ld = act1 && m1 < g.nmaps && c >= PAD;
    if (ld) {
      const float* p = map_base(g, m1) + (c - PAD);
      dcts::static_for<HP>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int r = decltype(i)::value;
        if constexpr (r < PAD)
          xr[r] = 0.f;
        else
          xr[r] = p[(r - PAD) * W];
      });
    } else {
      dcts::static_for<HP>([&](auto i) DCTS_LAMBDA_INLINE { xr[decltype(i)::value] = 0.f; });
    }
  }
  float y[HP];
  dcts::Dct2<HP>::run(xr, y);
  y[0] *= dcts::kInvSqrt2;
  if constexpr (G == 1 && HP % 4 == 0) {
    // one map per wave: lane = column, so row kk of the transposed slab is lane-consecutive words - ds_write_addtid_b32
    // (address = M0 + offset + 4 * lane: no address VGPR, 2 cycles per wave instruction instead of 4)
    if (act1) {
      const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)(lds_ptr)my);  // the wave's slab: uniform
      dcts::static_for<HP / 4>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int k0 = 4 * decltype(i)::value;
        lds_write_addtid4<k0 * S * 4, (k0 + 1) * S * 4, (k0 + 2) * S * 4, (k0 + 3) * S * 4>(base, y[k0], y[k0 + 1], y[k0 + 2], y[k0 + 3]);
      });
    }
  } else
  if (act1) {
    float* dst = my + g1 * MAP_LDS + c;
    dcts::static_for<HP>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int kk = decltype(i)::value;
      dst[kk * S] = y[kk];
    });
  }
  wave_fence();

  // ---- pass 2: row DCT-II of length WP, lane = row --------------------------------
  float z[WP], w[WP];
  {
    const float* src = my + (act2 ? g2 : 0) * MAP_LDS + (act2 ? k : 0) * S;
    dcts::static_for<WP>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int cc = decltype(i)::value;
      z[cc] = src[cc];
    });
  }
  dcts::Dct2<WP>::run(z, w);
  w[0] *= dcts::kInvSqrt2;
  const long long m2 = grp * G + g2;
  if constexpr (STORE_COEFF) {
    // debug/parity path: out is [nmaps][HP][WP] orthonormal coefficients
    if (act2 && m2 < g.nmaps) {
      constexpr float sc = float(2.0 / dcts::cx_sqrt(double(HP) * double(WP)));
      float* o = out + (m2 * HP + k) * WP;
      dcts::static_for<WP>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int l = decltype(i)::value;
        o[l] = w[l] * sc;
      });
    }
  } else {
    float e = 0.f;
    dcts::static_for<WP>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int l = decltype(i)::value;
      e = fmaf(w[l], w[l], e);
    });
    if (!act2) e = 0.f;
    DCTS_MAP_SUM(HP, e, k)
    if (act2 && k == 0 && m2 < g.nmaps) {
      constexpr float sc = float(4.0 / (double(HP) * double(WP)));
      out[m2] = e * sc;
    }
  }
  wave_fence();
}

template <int HP, int WP, int PAD, bool STORE_COEFF>
__global__ __launch_bounds__((64 * CodeletCfg<HP>::WAVES)) void k_energy_codelet(
    MapGeom g, float* __restrict__ out) {
  using Cfg = CodeletCfg<HP>;
  constexpr int G = Cfg::G, WAVES = Cfg::WAVES;
  __shared__ float slab[WAVES][Cfg::WAVE_LDS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];

  // pass-1 role: (map g1, column c); pass-2 role: (map g2, row k)
  const int g1 = lane / WP, c = lane - g1 * WP;
  const int g2 = lane / HP, k = lane - g2 * HP;
  const bool act1 = g1 < G, act2 = g2 < G;

  const long long ngroups = (g.nmaps + G - 1) / G;
  const long long wave_gid = (long long)blockIdx.x * WAVES + wave;
  const long long nwaves = (long long)gridDim.x * WAVES;

  for (long long grp = wave_gid; grp < ngroups; grp += nwaves)
    codelet_group<HP, WP, PAD, STORE_COEFF>(g, out, grp, my, g1, c, g2, k, act1, act2);
}

// Several hooked tensors of the same tile shape in ONE launch (MultiGeom, dcts_internal.h)
template <int HP, int WP, int PAD>
__global__ __launch_bounds__((64 * CodeletCfg<HP>::WAVES)) void k_energy_codelet_multi(MultiGeom mg) {
  using Cfg = CodeletCfg<HP>;
  constexpr int G = Cfg::G, WAVES = Cfg::WAVES;
  __shared__ float slab[WAVES][Cfg::WAVE_LDS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  const int g1 = lane / WP, c = lane - g1 * WP;
  const int g2 = lane / HP, k = lane - g2 * HP;
  const bool act1 = g1 < G, act2 = g2 < G;

  const long long wave_gid = (long long)blockIdx.x * WAVES + wave;
  const long long nwaves = (long long)gridDim.x * WAVES;
  int t = 0;
  for (long long grp = wave_gid; grp < mg.total_groups; grp += nwaves) {
    while (t + 1 < mg.count && grp >= mg.it[t + 1].group_begin) ++t;  // wave-uniform, monotone
    t = __builtin_amdgcn_readfirstlane(t);
    const MultiItem& item = mg.it[t];
    codelet_group<HP, WP, PAD, false>(item.g, item.out, grp - item.group_begin, my, g1, c, g2, k, act1, act2);
  }
}

// Tensors of DIFFERENT small tile shapes in one launch (edges 2, 4, 8, 16, 32: every hooked tensor of
// the CIFAR nets). VGG-16-bn at batch 256 is 187 MB of activations in five tile shapes: five launches
// plus the running-mean update were 58 us, launch ramps and tails costing as much as the work. The
// groups of all tensors form one index space (a group = floor(64 / edge) maps of ITS tensor's shape);
// a wave switches on the shape of the tensor its group belongs to and runs that shape's codelet
// group: the same code as k_energy_codelet, results bit for bit those of one call per tensor.
constexpr int mixed_slab_floats() {
  int m = 0;
#define DCTS_CASE(N) \
  if (CodeletCfg<N>::WAVE_LDS > m) m = CodeletCfg<N>::WAVE_LDS;
  DCTS_MIXED_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return m;
}

template <int E>
__device__ __forceinline__ void mixed_group(const MultiItem& item, long long grp, float* my, int lane) {
  using Cfg = CodeletCfg<E>;
  const int g1 = lane / E, c = lane - g1 * E;  // square tile: pass-1 and pass-2 roles coincide
  const bool act = g1 < Cfg::G;
  codelet_group<E, E, 0, false>(item.g, item.out, grp, my, g1, c, g1, c, act, act);
}

__global__ __launch_bounds__((64 * kMixedWaves)) void k_energy_codelet_mixed(MixedGeom mg) {
  __shared__ float slab[kMixedWaves][mixed_slab_floats()];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  const long long wave_gid = (long long)blockIdx.x * kMixedWaves + wave;
  const long long nwaves = (long long)gridDim.x * kMixedWaves;
  int t = 0;
  for (long long grp = wave_gid; grp < mg.total_groups; grp += nwaves) {
    while (t + 1 < mg.count && grp >= mg.it[t + 1].group_begin) ++t;  // wave-uniform, monotone
    t = __builtin_amdgcn_readfirstlane(t);
    const MultiItem& item = mg.it[t];
    const long long local = grp - item.group_begin;
    switch (__builtin_amdgcn_readfirstlane(item.g.H)) {
#define DCTS_CASE(N)                          \
  case N:                                     \
    mixed_group<N>(item, local, my, lane);    \
    break;
      DCTS_MIXED_SIZES(DCTS_CASE)
#undef DCTS_CASE
      default:
        break;
    }
  }
}

// ---------------------------------------------------------------------------------------
// lane-per-map kernels for tiny odd tiles (7x7: the last stage of ResNet-50; 9x9: U2-Net-p)
// ---------------------------------------------------------------------------------------
// The codelet kernel above gives a 7x7 map to 7 lanes: 243 VALU instructions per 9 maps, of which
// 70 are arithmetic (the rest: addressing, the transpose, a segmented reduction over 7 lanes), and
// every load instruction touches nine 28-byte segments: VALU-issue-bound at 45-50 % of the HBM peak.
// Here a lane owns a whole map: a wave streams 64 consecutive maps (64*N*N floats, contiguous in
// memory) into its private LDS slab with direct-to-LDS loads, every lane reads its N*N values
// (stride N*N floats between lanes: odd, conflict-free), and both DCT passes run in registers with
// no transpose and no cross-lane reduction: ~9 instructions per map instead of 27. The slab is free
// as soon as the lanes have read it, so the next group's loads are in flight during the arithmetic.
// Channel-sliced (non-dense) tensors take per-lane loads into the same arithmetic: same results.
template <int N>
struct LaneCfg {
  static constexpr int NN = N * N;
  static constexpr int G = kLaneMultiGroup;            // maps per wave per iteration (grid_caps.h)
  static constexpr int SLAB = (G * NN + 3) / 4 * 4;    // floats
  static constexpr int ITERS = (G * NN / 4 + 63) / 64;  // direct-to-LDS instructions per group
  static constexpr int WAVES = kLaneMultiWaves;
  static_assert(NN % 2 == 1, "lane stride must be odd (bank conflicts) - even tiles use the codelet kernel");
};

struct LaneGroup {  // wave-uniform description of one group of <= 64 maps
  const float* src;  // dense: first float of the group
  float* out;        // &out[m0]
  long long m0;
  int nm;            // maps in the group
  int dense;
  int item;
};

template <int N>
__device__ __forceinline__ void lane_stage(const LaneGroup& gr, lds_ptr my, int lane) {
  using Cfg = LaneCfg<N>;
  if (!gr.dense) return;
  const int nfl = gr.nm * Cfg::NN, nq = nfl >> 2, rem = nfl & 3;
  // wave-uniform operands, made so explicitly (they derive from the wave index)
  const unsigned long long sa = reinterpret_cast<unsigned long long>(gr.src);
  const unsigned long long src = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(sa >> 32)) << 32) |
                                 (unsigned)__builtin_amdgcn_readfirstlane((int)sa);
  const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)my);
#pragma unroll
  for (int it = 0; it < Cfg::ITERS; ++it) {
    const int q = it * 64 + lane;
    if (q < nq) {
      const unsigned dst = base + it * 1024;
      const unsigned off = (unsigned)q * 16u;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                   :
                   : "s"(dst), "v"(off), "s"(src)
                   : "memory", "m0");
    }
  }
  if (lane < rem) my[4 * nq + lane] = gr.src[4 * nq + lane];  // last 1-3 floats of a ragged tail
}

template <int N>
__device__ __forceinline__ void lane_compute(const MapGeom& g, const LaneGroup& gr, lds_ptr my, int lane,
                                             float (&v)[N * N]) {
  constexpr int NN = N * N;
  const bool act = lane < gr.nm;
  if (gr.dense) {
    lds_cptr p = my + (act ? lane : 0) * NN;
    dcts::static_for<NN>([&](auto i) DCTS_LAMBDA_INLINE { v[decltype(i)::value] = p[decltype(i)::value]; });
  } else {
    const float* p = map_base(g, gr.m0 + (act ? lane : 0));
    dcts::static_for<NN>([&](auto i) DCTS_LAMBDA_INLINE { v[decltype(i)::value] = p[decltype(i)::value]; });
  }
}

__device__ __forceinline__ LaneGroup lane_group_of(const MapGeom& g, float* out, long long grp, int nn, int item) {
  LaneGroup gr;
  gr.m0 = grp * 64;
  const long long left = g.nmaps - gr.m0;
  gr.nm = (int)(left < 64 ? left : 64);
  gr.src = g.x + (long long)g.c_begin * g.strideC + gr.m0 * nn;
  gr.dense = (g.contiguous && g.strideC == nn && ((reinterpret_cast<unsigned long long>(gr.src) & 15) == 0)) ? 1 : 0;
  gr.out = out + gr.m0;
  gr.item = item;
  return gr;
}

// one kernel for the single-tensor and the multi-tensor entry points (count == 1 for the former)
template <int N>
__global__ __launch_bounds__((64 * LaneCfg<N>::WAVES)) void k_energy_lane_multi(MultiGeom mg) {
  using Cfg = LaneCfg<N>;
  __shared__ __attribute__((aligned(16))) float slab[Cfg::WAVES][Cfg::SLAB];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const lds_ptr my = (lds_ptr)slab[wave];
  const long long wave_gid = (long long)blockIdx.x * Cfg::WAVES + wave;
  const long long nwaves = (long long)gridDim.x * Cfg::WAVES;
  int t = 0;
  auto locate = [&](long long grp) DCTS_LAMBDA_INLINE {
    while (t + 1 < mg.count && grp >= mg.it[t + 1].group_begin) ++t;  // wave-uniform, monotone
    t = __builtin_amdgcn_readfirstlane(t);
    return lane_group_of(mg.it[t].g, mg.it[t].out, grp - mg.it[t].group_begin, Cfg::NN, t);
  };
  if (wave_gid >= mg.total_groups) return;
  LaneGroup cur = locate(wave_gid);
  lane_stage<N>(cur, my, lane);
  for (long long grp = wave_gid; grp < mg.total_groups; grp += nwaves) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the group has landed in the slab
    float v[Cfg::NN];
    lane_compute<N>(mg.it[cur.item].g, cur, my, lane, v);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and is in registers: the slab is free
    const LaneGroup done = cur;
    if (grp + nwaves < mg.total_groups) {
      cur = locate(grp + nwaves);
      lane_stage<N>(cur, my, lane);
    }
    const float e = lane_energy<N>(v);
    if (lane < done.nm) done.out[lane] = e;
  }
}

// Prefetching variant for dense square even-edge tiles (the common case: every hooked tensor of
// the reference nets except 7x7 / 9x9). Same two passes and the same LDS slab, but the NEXT
// group of maps is streamed into the slab with direct-to-LDS loads (global_load_lds_dwordx4, no
// VGPRs) as soon as pass 2 has read the transposed tile out of it, so the HBM latency of group
// i+1 hides under the pass-2 codelet of group i instead of stalling the wave (s_waitcnt was
// 28 % of the wave's cycles in k_energy_codelet). Pass 1 then reads its column from the linear
// LDS image (lane = column: consecutive addresses, conflict-free). The passes are those of
// DCTS_CODELET_PASSES (codelet_schedule.hpp) with the prefetch issued between the pass-2 reads
// and the pass-2 codelet, which is why they are written out here.
template <int N>
__global__ __launch_bounds__((64 * CodeletCfg<N>::WAVES)) void k_energy_codelet_dma(
    MapGeom g, float* __restrict__ out) {
  using Cfg = CodeletCfg<N>;
  constexpr int G = Cfg::G, S = Cfg::S, MAP_LDS = Cfg::MAP_LDS, WAVES = Cfg::WAVES;
  constexpr int NN = N * N;
  constexpr int QPG = G * NN / 4;                // 16-byte quads per full group
  constexpr int DMA_IT = (QPG + 63) / 64;        // direct-to-LDS instructions per group
  constexpr int SLAB = ((Cfg::WAVE_LDS > DMA_IT * 256 ? Cfg::WAVE_LDS : DMA_IT * 256) + 3) / 4 * 4;
  static_assert((G * NN) % 4 == 0, "group must be a whole number of 16-byte quads");
  __shared__ __attribute__((aligned(16))) float slab[WAVES][SLAB];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* my = slab[wave];
  const int g1 = lane / N, c = lane - g1 * N;  // square tile: pass-1 and pass-2 roles coincide
  const bool act = g1 < G;

  const long long ngroups = (g.nmaps + G - 1) / G;
  const long long wave_gid = (long long)blockIdx.x * WAVES + wave;
  const long long nwaves = (long long)gridDim.x * WAVES;
  const float* x0 = g.x + (long long)g.c_begin * g.strideC;  // dense: map m starts at x0 + m*NN

  auto prefetch = [&](long long grp) DCTS_LAMBDA_INLINE {
    const long long m0 = grp * G;
    const long long left = g.nmaps - m0;
    const int nq = (int)((left < G ? left : G) * (NN / 4));
    const float* src = x0 + m0 * NN;
#pragma unroll
    for (int it = 0; it < DMA_IT; ++it) {
      const int q = it * 64 + lane;
      if (q < nq)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 4 * q),
                                         (__attribute__((address_space(3))) void*)(my + it * 256), 16, 0, 0);
    }
  };

  if (wave_gid < ngroups) prefetch(wave_gid);
  for (long long grp = wave_gid; grp < ngroups; grp += nwaves) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the group's tiles have landed in LDS
    const long long m1 = grp * G + g1;
    const bool valid = act && m1 < g.nmaps;
    // ---- pass 1: column DCT-II, lane = column, input from the linear LDS image --------
    float xr[N], y[N];
    {
      const float* src = my + (valid ? g1 * NN + c : 0);
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int r = decltype(i)::value;
        xr[r] = src[r * N];
      });
      if (!valid) dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE { xr[decltype(i)::value] = 0.f; });
    }
    dcts::Dct2<N>::run(xr, y);
    y[0] *= dcts::kInvSqrt2;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (act) {
      float* dst = my + g1 * MAP_LDS + c;
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int kk = decltype(i)::value;
        dst[kk * S] = y[kk];
      });
    }
    wave_fence();
    // ---- pass 2: row DCT-II, lane = row -----------------------------------------------
    float z[N], w[N];
    {
      const float* src = my + (act ? g1 : 0) * MAP_LDS + (act ? c : 0) * S;
      dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int cc = decltype(i)::value;
        z[cc] = src[cc];
      });
    }
    // the slab is free once these reads have returned: stream the next group into it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (grp + nwaves < ngroups) prefetch(grp + nwaves);
    dcts::Dct2<N>::run(z, w);
    w[0] *= dcts::kInvSqrt2;
    float e = 0.f;
    dcts::static_for<N>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int l = decltype(i)::value;
      e = fmaf(w[l], w[l], e);
    });
    if (!act) e = 0.f;
    DCTS_MAP_SUM(N, e, c)
    if (valid && c == 0) {
      constexpr float sc = float(4.0 / (double(N) * double(N)));
      out[m1] = e * sc;
    }
  }
}

template <int HP, int WP, int PAD, bool STORE>
int launch_codelet(const MapGeom& g, float* out, hipStream_t st) {
  return launch_codelet_grid<HP>(k_energy_codelet<HP, WP, PAD, STORE>, g.nmaps, st, g, out);
}

template <int N>
int launch_codelet_dma(const MapGeom& g, float* out, hipStream_t st) {
  using Cfg = CodeletCfg<N>;
  if constexpr ((Cfg::G * N * N) % 4 != 0) {
    return DCTS_E_UNSUPPORTED;
  } else {
    const long long ngroups = (g.nmaps + Cfg::G - 1) / Cfg::G;
    // persistent grid = exactly one residency: every wave then loops over many groups and the
    // prefetch of group i+1 overlaps the arithmetic of group i
    const long long cap = (long long)num_cus() * blocks_per_cu<k_energy_codelet_dma<N>, Cfg::WAVES>();
    hipLaunchKernelGGL((k_energy_codelet_dma<N>), dim3(grid_blocks(ngroups, Cfg::WAVES, cap)), dim3(64 * Cfg::WAVES), 0, st, g, out);
    return (int)hipGetLastError();
  }
}

template <int HP, int WP, int PAD>
int launch_codelet_multi(const MultiGeom& mg, hipStream_t st) {
  hipLaunchKernelGGL((k_energy_codelet_multi<HP, WP, PAD>), dim3(codelet_grid<HP>(mg.total_groups)), dim3(64 * CodeletCfg<HP>::WAVES),
                     0, st, mg);
  return (int)hipGetLastError();
}

template <int N>
int launch_lane(const MultiGeom& mg, hipStream_t st) {
  using Cfg = LaneCfg<N>;
  const long long cap = (long long)num_cus() * blocks_per_cu<k_energy_lane_multi<N>, Cfg::WAVES>();
  hipLaunchKernelGGL((k_energy_lane_multi<N>), dim3(grid_blocks(mg.total_groups, Cfg::WAVES, cap)), dim3(64 * Cfg::WAVES), 0, st, mg);
  return (int)hipGetLastError();
}

}  // namespace

namespace dctsi {

int codelet_group_size(int HP) {
  if (has_lane_kernel(HP)) return 64;
#define DCTS_CASE(N) \
  if (HP == N) return CodeletCfg<N>::G;
  DCTS_CODELET_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return 0;
}

int dispatch_codelet_dma(int N, const MapGeom& g, float* out, hipStream_t st) {
#define DCTS_CASE(N_) \
  case N_:            \
    return launch_codelet_dma<N_>(g, out, st);
  switch (N) {
    DCTS_CODELET_SIZES(DCTS_CASE)
    default:
      return DCTS_E_UNSUPPORTED;
  }
#undef DCTS_CASE
}

int dispatch_codelet(int store, int HP, int WP, int pad, const MapGeom& g, float* out, hipStream_t st) {
  if (HP != WP) return DCTS_E_UNSUPPORTED;  // rect.hip serves non-square tiles
  return switch_codelet_size(HP, pad, [&](auto n, auto p) {
    constexpr int N = decltype(n)::value, PAD = decltype(p)::value;
    return store ? launch_codelet<N, N, PAD, true>(g, out, st) : launch_codelet<N, N, PAD, false>(g, out, st);
  });
}

int dispatch_codelet_mixed(const MixedGeom& mg, hipStream_t st) {
  const long long cap = (long long)num_cus() * blocks_per_cu<k_energy_codelet_mixed, kMixedWaves>();  // one residency of persistent waves
  hipLaunchKernelGGL(k_energy_codelet_mixed, dim3(grid_blocks(mg.total_groups, kMixedWaves, cap)), dim3(64 * kMixedWaves), 0, st, mg);
  return (int)hipGetLastError();
}

int dispatch_lane(int n, const MultiGeom& mg, hipStream_t st) {
  switch (n) {
    case 7:
      return launch_lane<7>(mg, st);
    case 9:
      return launch_lane<9>(mg, st);
    default:
      return DCTS_E_UNSUPPORTED;
  }
}

int dispatch_codelet_multi(int HP, int pad, const MultiGeom& mg, hipStream_t st) {
  if (has_lane_kernel(HP) && pad == 0) return dispatch_lane(HP, mg, st);
  return switch_codelet_size(HP, pad, [&](auto n, auto p) {
    return launch_codelet_multi<decltype(n)::value, decltype(n)::value, decltype(p)::value>(mg, st);
  });
}

}  // namespace dctsi
