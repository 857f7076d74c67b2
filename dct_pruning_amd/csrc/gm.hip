// gm.hip - the geometric-median criterion on feature maps (dcts_gm_distance_f32, include/dctscore.h):
//   out[n][j] = sum_{k in the reference set} || x[n, c_begin + j] - x[n, k] ||_2,  the norm over the H * W elements of a map.
// FPGM's rule for filter weights (prune what lies closest to the geometric median of its layer) applied to the maps a layer
// produces: a map whose summed distance to the others is small is the one the others can replace. High = far = keep.
//
// The only kernel of the library that is all-pairs within a sample: compute-bound, LDS-tiled, fp32 VALU.
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
// c_count, the row's place in its tile or the launch. No atomics, no workspace, no second kernel.
//
// Tails in C and in H * W are zeros in LDS (a zero pair of elements adds fma(0, 0, acc) = acc); nothing is read from a clamped
// address. LDS image: [channel][kGmLD = 68] floats per tile. A thread reads four consecutive elements of a channel
// (ds_read_b128); the 16 tx lanes of a 16-lane group read channels tx + 16 j, 68 floats = 17 slots of 16 bytes apart: 17 tx mod 16
// are 16 distinct slots, so the reads are conflict-free, and the 4 ty values of a wave are 4 broadcast addresses.
// Global loads: 16 bytes per lane where the base, strideN, strideC and H * W are multiples of 4 floats (16 lanes cover the
// 256 bytes a channel contributes to a chunk), else single dwords (a wave per channel row). Both leave the same LDS image, so
// the same bits come out. Nothing is prefetched into registers: at 94 / 120 VGPRs and 34 KiB of LDS four workgroups share a
// CU, and one stages while the others compute (DESIGN.md 7h has the measurement against a register-prefetching version).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "dcts_internal.h"
#include "grid_caps.h"

using namespace dctsi;

namespace {

constexpr int TS = kGmTS, TR = kGmTR, KP = kGmKP, LD = kGmLD, THREADS = kGmThreads;
static_assert(TS == 64 && TR == 64 && THREADS == 256, "thread (ty, tx) of 16 x 16 owns rows ty + 16 i and columns tx + 16 j, i, j < 4");
static_assert(KP % 4 == 0 && LD % 4 == 0 && (LD / 4) % 2 == 1 && LD >= KP, "16-byte rows, an odd number of 16-byte slots apart");

// One tile's share of a chunk, global -> LDS: channels [ch0, ch0 + 64) of the range that starts at `base` (element 0 of its
// channel 0 in this sample) and has `count` channels, elements [p0, p0 + KP). Out of range: zeros, and no load. Four loads are
// in flight per thread before their stores.
template <bool VEC>
__device__ __forceinline__ void stage_tile(const float* __restrict__ base, long long strideC, int count, int ch0, int hw, int p0,
                                           float* __restrict__ lds) {
  constexpr int PER = VEC ? KP / 4 : KP;     // threads per channel row
  constexpr int ROWS = THREADS / PER;        // channel rows per step
  constexpr int E = VEC ? 4 : 1;
  const int c = threadIdx.x / PER, e = E * (threadIdx.x % PER), p = p0 + e;
  const float* src = base + (long long)(ch0 + c) * strideC + p;
  float* dst = lds + c * LD + e;
  const bool inside = p < hw;
#pragma unroll 4
  for (int i = 0; i < TS / ROWS; ++i) {
    const bool ok = inside && ch0 + c + ROWS * i < count;
    const float* s = src + (long long)(ROWS * i) * strideC;
    if constexpr (VEC)
      *reinterpret_cast<float4*>(dst + ROWS * i * LD) = ok ? *reinterpret_cast<const float4*>(s) : float4{0.f, 0.f, 0.f, 0.f};
    else
      dst[ROWS * i * LD] = ok ? *s : 0.f;
  }
}

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// two consecutive elements of a pair at once: v_pk_add_f32 (with the negation as a source modifier), v_pk_fma_f32
__device__ __forceinline__ void pair_step(v2f a, v2f b, v2f& acc) {
  const v2f d = a - b;
  acc = __builtin_elementwise_fma(d, d, acc);
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gm_distance(GmGeom g, float* __restrict__ out) {
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

  float row[4] = {0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < g.r_count; r0 += TR) {
    v2f acc[4][4];  // .x: the chain of the even p, .y: of the odd p
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v2f{0.f, 0.f};

    for (int p0 = 0; p0 < hw; p0 += KP) {
      stage_tile<VEC>(abase, g.strideC, g.c_count, s0, hw, p0, sA);
      stage_tile<VEC>(bbase, g.strideC, g.r_count, r0, hw, p0, sB);
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

}  // namespace

namespace dctsi {

int dispatch_gm(const GmGeom& g, float* out, hipStream_t st) {
  const long long blocks = g.N * ((g.c_count + TS - 1) / TS);  // one workgroup per sample and scored tile: no grid loop
  if (blocks > kGmMaxBlocks) return DCTS_E_SHAPE;
  const bool vec = (reinterpret_cast<uintptr_t>(g.x) & 15) == 0 && g.strideN % 4 == 0 && g.strideC % 4 == 0 && g.hw % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(k_gm_distance<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out);
  else
    hipLaunchKernelGGL(k_gm_distance<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, g, out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
