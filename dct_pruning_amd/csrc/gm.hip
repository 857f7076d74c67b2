// gm.hip - the geometric-median criterion on feature maps (dcts_gm_distance_f32, include/dctscore.h):
//   out[n][j] = sum_{k in the reference set} || x[n, c_begin + j] - x[n, k] ||_2,  the norm over the H * W elements of a map.
// FPGM's rule for filter weights (prune what lies closest to the geometric median of its layer) applied to the maps a layer
// produces: a map whose summed distance to the others is small is the one the others can replace. High = far = keep.
//
// With a metric (dcts_gm_distance_metric_f32) the same sum runs over unit maps: x / |x| (cosine) or (x - mean) / |x - mean|
// (correlation), so that a map and a scaled copy of it are at distance 0 and a large norm alone is not "far". k_gm_stats
// leaves one (mu, s) pair per map in the caller's workspace, k_gm_distance<.., NORM = true> applies it where it stages a map.
//
// k_gm_distance is the only kernel of the library that is all-pairs within a sample: compute-bound, LDS-tiled, fp32 VALU.
//
//   k_gm_distance  one workgroup (kGmThreads = 256 = 16 x 16) owns one sample and a tile of kGmTS = 64 scored channels. It walks
//                  the reference set in tiles of kGmTR = 64 channels, ascending from r_begin, and for every reference tile
//                  stages both tiles' maps in LDS in chunks of kGmKP = 64 elements of the flattened H * W axis, ascending.
//                  Thread (ty, tx) keeps the 4 x 4 pair accumulators of scored rows ty + 16 i and reference columns tx + 16 j,
//                  each a pair of chains, one over the even p and one over the odd p (v_pk_add_f32, v_pk_fma_f32):
//                      acc[i][j].{x, y} = fma(a - b, a - b, acc[i][j].{x, y}),  p ascending, whatever the chunking.
//                  After the last chunk of a reference tile: row[i] += sqrtf(acc.x + acc.y), j ascending, columns beyond the
//                  reference set skipped. After the last reference tile: a xor-shuffle tree over the 16 tx lanes of a row
//                  (every lane ends with the same bits), one store per scored map.
//
// The difference form, never the Gram form |a|^2 + |b|^2 - 2 a.b: (a - b)^2 is exactly (b - a)^2 and exactly 0 for equal
// elements, so d(a, a) = +0.0, d(a, b) has the bits of d(b, a), and near-duplicate maps - the pairs this criterion exists to
// find - lose nothing to cancellation. A pair's chains depend on the two maps alone; a row's sum on the position of every
// reference channel RELATIVE TO r_begin (tile = k / 64, lane = k % 16, j = k % 64 / 16) and on nothing else: not on N, c_begin,
// c_count, the row's place in its tile or the launch. No atomics; without a metric no workspace and no second kernel.
//
// Tails in C and in H * W are zeros in LDS (a zero pair of elements adds fma(0, 0, acc) = acc); nothing is read from a clamped
// address. LDS image: [channel][kGmLD = 68] floats per tile. A thread reads four consecutive elements of a channel
// (ds_read_b128); the 16 tx lanes of a 16-lane group read channels tx + 16 j, 68 floats = 17 slots of 16 bytes apart: 17 tx mod 16
// are 16 distinct slots, so the reads are conflict-free, and the 4 ty values of a wave are 4 broadcast addresses.
// Global loads: 16 bytes per lane where the base, strideN, strideC and H * W are multiples of 4 floats (16 lanes cover the
// 256 bytes a channel contributes to a chunk), else single dwords (a wave per channel row). Both leave the same LDS image, so
// the same bits come out. Nothing is prefetched into registers: at 94 / 120 VGPRs and 34 KiB of LDS four workgroups share a
// CU, and one stages while the others compute (DESIGN.md 7h has the measurement against a register-prefetching version).
// stage_tile, unit, pair_step and the tile constants are in gm_common.hpp, which k_gm_pairs (gm_pairs.hip) shares.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "dcts_internal.h"
#include "gm_common.hpp"
#include "grid_caps.h"

using namespace dctsi;

namespace {

// NORM: the distance between the unit maps; sa / sb: the (mu, s) pairs of the scored and of the reference range, [N][c_count]
// and [N][r_count] (k_gm_stats). Without NORM they are not read.
template <bool VEC, bool NORM>
__global__ __launch_bounds__(THREADS) void k_gm_distance(GmGeom g, float* __restrict__ out, const float2* __restrict__ sa,
                                                         const float2* __restrict__ sb) {
  __shared__ __attribute__((aligned(16))) float sA[TS * LD];
  __shared__ __attribute__((aligned(16))) float sB[TR * LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int stiles = (g.c_count + TS - 1) / TS;
  const long long n = blockIdx.x / stiles;
  const int s0 = (int)(blockIdx.x - n * stiles) * TS;
  const float* xs = g.x + n * g.strideN;
  const float* abase = xs + (long long)g.c_begin * g.strideC;
  const float* bbase = xs + (long long)g.r_begin * g.strideC;
  const int hw = g.hw;
  if constexpr (NORM) {
    sa += n * g.c_count;
    sb += n * g.r_count;
  }

  float row[4] = {0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < g.r_count; r0 += TR) {
    v2f acc[4][4];  // .x: the chain of the even p, .y: of the odd p
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v2f{0.f, 0.f};

    for (int p0 = 0; p0 < hw; p0 += KP) {
      stage_tile<VEC, NORM>(abase, g.strideC, g.c_count, s0, hw, p0, sA, sa);
      stage_tile<VEC, NORM>(bbase, g.strideC, g.r_count, r0, hw, p0, sB, sb);
      __syncthreads();
#pragma unroll 2
      for (int q = 0; q < KP; q += 4) {
        v4f a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const v4f*>(sA + (ty + 16 * i) * LD + q);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const v4f*>(sB + (tx + 16 * j) * LD + q);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            pair_step(a[i].lo, b[j].lo, acc[i][j]);
            pair_step(a[i].hi, b[j].hi, acc[i][j]);
          }
      }
      __syncthreads();
    }
    // the distances of this reference tile into the row sums, j ascending; columns beyond the reference set are not counted
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = r0 + tx + 16 * j < g.r_count;
#pragma unroll
      for (int i = 0; i < 4; ++i) row[i] += live ? sqrtf(acc[i][j].x + acc[i][j].y) : 0.f;
    }
  }

  // the 16 tx lanes of a row: a xor tree, the same bits in every lane
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = row[i];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    const int j = s0 + ty + 16 * i;
    if (tx == 0 && j < g.c_count) out[n * g.c_count + j] = v;
  }
}

// ---- the unit maps' (mu, s) pairs ----------------------------------------------------------------------------------------
// One wave per map, kGmStatsMaps maps per workgroup, one workgroup per kGmStatsMaps maps and no grid loop. pairs[n * count + j] =
// (mu, s) of channel begin + j of sample n:
//   CENTER (correlation)  mu = sum / hw, s = 1 / sqrt(sum_p (x_p - mu)^2);  s = 0 for a flat map: max == min, an exact
//                         comparison taken in the pass of the sum. No threshold on the centred sum: the rounding of mu alone
//                         leaves a constant map a centred sum that is not 0, a unit vector of noise.
//   otherwise (cosine)    mu = 0, s = 1 / sqrt(sum_p x_p^2);  s = 0 where that sum is 0.
// Two passes, never sum x^2 - hw * mu^2, which cancels for the maps whose pattern is small against their mean; the second read
// of a map comes from the cache its first read filled. (A centred sum that underflows to 0 gives s = 0 as well, not 1 / 0: maps
// of denormal spread are outside the contract.)
// The order of every sum is a function of p and hw alone: the elements in groups of four, group q = p / 4 to lane q % 64, q
// ascending; a lane keeps one chain per position p % 4 in the group, adds them as (c0 + c1) + (c2 + c3), and a xor tree over
// the 64 lanes (32, 16, ... 1) leaves the same bits in every lane. Elements beyond hw are skipped, not added as zeros. The
// 16-byte path (a group is one load; hw is a multiple of 4 there) and the dword path feed the same chains: the same bits.
template <bool VEC>
__device__ __forceinline__ int load_group(const float* __restrict__ x, int q, int hw, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(x + 4 * q);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    return 4;
  } else {
    const int live = hw - 4 * q < 4 ? hw - 4 * q : 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < live ? x[4 * q + e] : 0.f;
    return live;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool VEC, bool CENTER>
__global__ __launch_bounds__(kGmStatsThreads) void k_gm_stats(GmGeom g, int begin, int count, float2* __restrict__ pairs) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * kGmStatsMaps + (threadIdx.x >> 6);
  if (m >= g.N * count) return;  // the whole wave
  const long long n = m / count;
  const float* x = g.x + n * g.strideN + (begin + (m - n * count)) * g.strideC;
  const int hw = g.hw, groups = (hw + 3) >> 2;

  float mu = 0.f;
  bool flat = false;
  if constexpr (CENTER) {
    float c[4] = {0.f, 0.f, 0.f, 0.f}, lo = INFINITY, hi = -INFINITY;
    for (int q = lane; q < groups; q += 64) {
      float v[4];
      const int live = load_group<VEC>(x, q, hw, v);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < live) c[e] += v[e], lo = fminf(lo, v[e]), hi = fmaxf(hi, v[e]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off, 64)), hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    mu = wave_sum((c[0] + c[1]) + (c[2] + c[3])) / (float)hw;
    flat = hi == lo;
  }
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  for (int q = lane; q < groups; q += 64) {
    float v[4];
    const int live = load_group<VEC>(x, q, hw, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < live) c[e] = __builtin_fmaf(v[e] - mu, v[e] - mu, c[e]);
  }
  const float ss = wave_sum((c[0] + c[1]) + (c[2] + c[3]));
  if (lane == 0) pairs[m] = float2{mu, (flat || ss == 0.f) ? 0.f : 1.0f / sqrtf(ss)};
}

}  // namespace

namespace dctsi {

int dispatch_gm(const GmGeom& g, float* out, hipStream_t st) {
  const long long blocks = g.N * ((g.c_count + TS - 1) / TS);  // one workgroup per sample and scored tile: no grid loop
  if (blocks > kGmMaxBlocks) return DCTS_E_SHAPE;
  if (gm_vec(g))
    hipLaunchKernelGGL((k_gm_distance<true, false>), dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out, nullptr, nullptr);
  else
    hipLaunchKernelGGL((k_gm_distance<false, false>), dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out, nullptr, nullptr);
  return (int)hipGetLastError();
}

// One k_gm_stats launch: the (mu, s) pairs of channels [begin, begin + count) of every sample, [N][count] at `pairs`. The
// caller has checked the grid against kGmMaxBlocks.
int launch_gm_stats(const GmGeom& g, bool center, int begin, int count, float2* pairs, hipStream_t st) {
  const bool vec = gm_vec(g);
  const dim3 grid((unsigned)((g.N * count + kGmStatsMaps - 1) / kGmStatsMaps)), block(kGmStatsThreads);
  const auto kernel = vec ? (center ? k_gm_stats<true, true> : k_gm_stats<true, false>)
                          : (center ? k_gm_stats<false, true> : k_gm_stats<false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, st, g, begin, count, pairs);
  return (int)hipGetLastError();
}

// The (mu, s) pairs of both ranges, then the distances between the unit maps: two or three launches on `st`, all or none (both
// grids are checked first). Where the scored range is the reference range its pairs are computed once, into sa.
int dispatch_gm_metric(const GmGeom& g, bool center, float2* sa, float2* sb, float* out, hipStream_t st) {
  const long long blocks = g.N * ((g.c_count + TS - 1) / TS);
  const int larger = g.c_count > g.r_count ? g.c_count : g.r_count;
  const long long stats_blocks = (g.N * larger + kGmStatsMaps - 1) / kGmStatsMaps;
  if (blocks > kGmMaxBlocks || stats_blocks > kGmMaxBlocks) return DCTS_E_SHAPE;
  if (const int rc = launch_gm_stats(g, center, g.c_begin, g.c_count, sa, st)) return rc;
  if (g.r_begin == g.c_begin && g.r_count == g.c_count)
    sb = sa;
  else if (const int rc = launch_gm_stats(g, center, g.r_begin, g.r_count, sb, st))
    return rc;
  if (gm_vec(g))
    hipLaunchKernelGGL((k_gm_distance<true, true>), dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out, sa, sb);
  else
    hipLaunchKernelGGL((k_gm_distance<false, true>), dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out, sa, sb);
  return (int)hipGetLastError();
}

}  // namespace dctsi
