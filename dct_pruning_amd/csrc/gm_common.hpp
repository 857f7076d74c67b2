// gm_common.hpp - what the two all-pairs kernels share: k_gm_distance (gm.hip: the distances of a scored map summed over the
// reference set) and k_gm_pairs (gm_pairs.hip: every distance, summed over the samples). The tile constants, the global -> LDS
// staging of a tile's share of a chunk (both load paths, with and without the unit-map normalisation), and the packed
// difference-square step. gm.hip's header comment describes the LDS image and the arithmetic; nothing here knows what is
// done with a finished pair accumulator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcts_internal.h"
#include "grid_caps.h"

using namespace dctsi;

namespace {

constexpr int TS = kGmTS, TR = kGmTR, KP = kGmKP, LD = kGmLD, THREADS = kGmThreads;
static_assert(TS == 64 && TR == 64 && THREADS == 256, "thread (ty, tx) of 16 x 16 owns rows ty + 16 i and columns tx + 16 j, i, j < 4");
static_assert(KP % 4 == 0 && LD % 4 == 0 && (LD / 4) % 2 == 1 && LD >= KP, "16-byte rows, an odd number of 16-byte slots apart");

// an element of a unit map from the element of the map and the map's (mu, s): see stage_tile
__device__ __forceinline__ float unit(float x, float2 ms) { return __builtin_fmaf(x - ms.x, ms.y, 0.f); }

// One tile's share of a chunk, global -> LDS: channels [ch0, ch0 + 64) of the range that starts at `base` (element 0 of its
// channel 0 in this sample) and has `count` channels, elements [p0, p0 + KP). Out of range: zeros, and no load. Four loads are
// in flight per thread before their stores.
// NORM: what lands in LDS is the unit map, (x - mu) * s with the (mu, s) pair k_gm_stats left for the element's channel in
// `stats` (pair 0: channel 0 of the range in this sample), fetched once per channel row of the call: a 16-byte-path thread holds
// four rows, a dword-path wave one row at a time, so there the pair is wave-uniform and read as such. The product is rounded
// once and +0.0 is added to it: a flat map (s = 0) becomes +0.0 in every element whatever the sign of x - mu, and no other
// value changes. Out of range stays 0, not (0 - mu) * s, and no pair is read for a channel beyond the range.
template <bool VEC, bool NORM>
__device__ __forceinline__ void stage_tile(const float* __restrict__ base, long long strideC, int count, int ch0, int hw, int p0,
                                           float* __restrict__ lds, const float2* __restrict__ stats) {
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
    if constexpr (!NORM) {
      if constexpr (VEC)
        *reinterpret_cast<float4*>(dst + ROWS * i * LD) = ok ? *reinterpret_cast<const float4*>(s) : float4{0.f, 0.f, 0.f, 0.f};
      else
        dst[ROWS * i * LD] = ok ? *s : 0.f;
    } else {
      const int ch = ch0 + ROWS * i + (VEC ? c : __builtin_amdgcn_readfirstlane(c));  // PER == 64: a wave is one channel row
      const float2 ms = ch < count ? stats[ch] : float2{0.f, 0.f};
      if constexpr (VEC) {
        float4 v{0.f, 0.f, 0.f, 0.f};
        if (ok) {
          const float4 t = *reinterpret_cast<const float4*>(s);
          v = float4{unit(t.x, ms), unit(t.y, ms), unit(t.z, ms), unit(t.w, ms)};
        }
        *reinterpret_cast<float4*>(dst + ROWS * i * LD) = v;
      } else {
        dst[ROWS * i * LD] = ok ? unit(*s, ms) : 0.f;
      }
    }
  }
}

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// two consecutive elements of a pair at once: v_pk_add_f32 (with the negation as a source modifier), v_pk_fma_f32
__device__ __forceinline__ void pair_step(v2f a, v2f b, v2f& acc) {
  const v2f d = a - b;
  acc = __builtin_elementwise_fma(d, d, acc);
}

}  // namespace

namespace dctsi {

// the 16-byte load path: the base, both strides and H * W are multiples of 4 floats
inline bool gm_vec(const GmGeom& g) {
  return (reinterpret_cast<uintptr_t>(g.x) & 15) == 0 && g.strideN % 4 == 0 && g.strideC % 4 == 0 && g.hw % 4 == 0;
}

}  // namespace dctsi
