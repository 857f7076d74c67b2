// gm_pairs.hip - the pair matrix of the geometric-median criterion (dcts_gm_pairs_f32, include/dctscore.h):
//   out[j][k] = sum_n d(x[n, c_begin + j], x[n, r_begin + k]),  d the distance of dcts_gm_distance_metric_f32 for the metric.
// k_gm_distance (gm.hip) computes every d(c, k) in registers and keeps their sum over k; a selection rule that has to tell two
// duplicates from two maps that are merely both far from the rest (nearest neighbour, k-center, clustering) needs the terms.
// One matrix per SAMPLE would be [N, C, C] floats, 4 GiB for a ResNet-50 layer at batch 256, so the sum over the samples is
// taken here and the caller divides by their count.
//
//   k_gm_pairs   one workgroup (kGmThreads = 256 = 16 x 16) owns a tile of kGmTS = 64 scored channels, a tile of kGmTR = 64
//                reference channels and one SLICE of the samples, a contiguous run [s * per, min(N, (s + 1) * per)). Per sample
//                it does what k_gm_distance does for one reference tile: both tiles' maps through LDS in chunks of kGmKP
//                elements (stage_tile of gm_common.hpp: both load paths, the unit maps of a metric), thread (ty, tx) keeping
//                the 4 x 4 pair accumulators of rows ty + 16 i and columns tx + 16 j, each two fused multiply-add chains
//                over the even and the odd p. After the last chunk: sum[i][j] += sqrtf(acc.x + acc.y), n ascending. After
//                its last sample a thread stores its live entries; for a fixed (i, j) the 16 tx lanes write 64 contiguous
//                bytes of a row. Rows and columns beyond the ranges are zeros in LDS, computed, and never stored.
//   k_gm_pairs_sum   with more than one slice the workgroups store to partials [S][c_count][r_count] in the workspace and this
//                kernel adds them, s ascending, one thread per entry. With one slice k_gm_pairs stores to `out` itself.
//
// The slices (gm_pair_slices, grid_caps.h) are a function of N and r_count alone, and an entry is a function of its two maps,
// the metric and the slices: not of c_begin, c_count, the alignment of x or the place of the channels in their tiles. So a row
// of a call on a channel sub-range has the bits it has in the call on the whole range, the two load paths agree, and with
// scored range = reference range the matrix is symmetric bit for bit ((a - b)^2 is (b - a)^2 in every chain). d(a, a) = +0.0,
// identical maps are at +0.0, a NaN map reaches its own row and column only. No atomics, nothing allocated.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "dcts_internal.h"
#include "gm_common.hpp"
#include "grid_caps.h"

using namespace dctsi;

namespace {

// out: [slices][c_count][r_count]; per: samples per slice. sa / sb as in k_gm_distance (NORM only).
template <bool VEC, bool NORM>
__global__ __launch_bounds__(THREADS) void k_gm_pairs(GmGeom g, float* __restrict__ out, const float2* __restrict__ sa,
                                                      const float2* __restrict__ sb, long long per) {
  __shared__ __attribute__((aligned(16))) float sA[TS * LD];
  __shared__ __attribute__((aligned(16))) float sB[TR * LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const unsigned stiles = (g.c_count + TS - 1) / TS, rtiles = (g.r_count + TR - 1) / TR;
  // the reference tile runs fastest: neighbouring workgroups share their scored tile and their samples
  const unsigned rt = blockIdx.x % rtiles, rest = blockIdx.x / rtiles;
  const int r0 = (int)rt * TR, s0 = (int)(rest % stiles) * TS;
  const long long slice = rest / stiles;
  const long long n0 = slice * per, n1 = n0 + per < g.N ? n0 + per : g.N;
  const int hw = g.hw;

  float sum[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[i][j] = 0.f;

  for (long long n = n0; n < n1; ++n) {
    const float* xs = g.x + n * g.strideN;
    const float* abase = xs + (long long)g.c_begin * g.strideC;
    const float* bbase = xs + (long long)g.r_begin * g.strideC;
    const float2* pa = NORM ? sa + n * g.c_count : nullptr;
    const float2* pb = NORM ? sb + n * g.r_count : nullptr;

    v2f acc[4][4];  // .x: the chain of the even p, .y: of the odd p
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v2f{0.f, 0.f};

    for (int p0 = 0; p0 < hw; p0 += KP) {
      stage_tile<VEC, NORM>(abase, g.strideC, g.c_count, s0, hw, p0, sA, pa);
      stage_tile<VEC, NORM>(bbase, g.strideC, g.r_count, r0, hw, p0, sB, pb);
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
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[i][j] += sqrtf(acc[i][j].x + acc[i][j].y);
  }

  float* dst = out + slice * ((long long)g.c_count * g.r_count);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = s0 + ty + 16 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = r0 + tx + 16 * j;
      if (row < g.c_count && col < g.r_count) dst[(long long)row * g.r_count + col] = sum[i][j];
    }
  }
}

// out[e] = part[0][e] + part[1][e] + ... + part[slices - 1][e], one after the other
__global__ __launch_bounds__(kGmPairSumThreads) void k_gm_pairs_sum(const float* __restrict__ part, long long entries, int slices,
                                                                    float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * kGmPairSumThreads + threadIdx.x;
  if (e >= entries) return;
  float v = part[e];
  for (int s = 1; s < slices; ++s) v += part[(long long)s * entries + e];
  out[e] = v;
}

}  // namespace

namespace dctsi {

// Every launch of a call on `st`, all or none: the grids are checked first. center < 0: no metric (sa, sb unused); else the
// (mu, s) pairs of both ranges first (launch_gm_stats, gm.hip), those of the scored range once where it is the reference range.
int dispatch_gm_pairs(const GmGeom& g, int center, float2* sa, float2* sb, float* partials, float* out, hipStream_t st) {
  const int slices = gm_pair_slices(g.N, g.r_count);
  const long long per = (g.N + slices - 1) / slices;
  const long long entries = (long long)g.c_count * g.r_count;
  const long long blocks = (long long)slices * ((g.c_count + TS - 1) / TS) * ((g.r_count + TR - 1) / TR);
  const long long sum_blocks = (entries + kGmPairSumThreads - 1) / kGmPairSumThreads;
  const int larger = g.c_count > g.r_count ? g.c_count : g.r_count;
  const long long stats_blocks = center < 0 ? 0 : (g.N * larger + kGmStatsMaps - 1) / kGmStatsMaps;
  if (blocks > kGmMaxBlocks || sum_blocks > kGmMaxBlocks || stats_blocks > kGmMaxBlocks) return DCTS_E_SHAPE;
  const bool vec = gm_vec(g);
  if (center >= 0) {
    if (const int rc = launch_gm_stats(g, center != 0, g.c_begin, g.c_count, sa, st)) return rc;
    if (g.r_begin == g.c_begin && g.r_count == g.c_count)
      sb = sa;
    else if (const int rc = launch_gm_stats(g, center != 0, g.r_begin, g.r_count, sb, st))
      return rc;
  }
  float* dst = slices > 1 ? partials : out;
  const auto kernel = center >= 0 ? (vec ? k_gm_pairs<true, true> : k_gm_pairs<false, true>)
                                  : (vec ? k_gm_pairs<true, false> : k_gm_pairs<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, g, dst, sa, sb, per);
  if (const int rc = (int)hipGetLastError()) return rc;
  if (slices > 1) {
    hipLaunchKernelGGL(k_gm_pairs_sum, dim3((unsigned)sum_blocks), dim3(kGmPairSumThreads), 0, st, partials, entries, slices, out);
    return (int)hipGetLastError();
  }
  return DCTS_OK;
}

}  // namespace dctsi
