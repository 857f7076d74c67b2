// api.hip - the C ABI of include/dctscore.h. Every entry point turns its arguments into a TensorView, validate() checks it,
// choose() names the kernel family that serves it (the only place where a shape becomes a family), and run() packs that family's
// descriptor and calls its dispatcher (dcts_internal.h, rect.h). Also the kernels that belong to no family.
//
// Replaces the per-map Python loop of the reference hooks (utils/common.py:262-309):
//   c = [dct.dct_2d(output[i,j,:,:], norm='ortho') ...]; torch.sum(dct.mul(dct)).item()
// with one launch per hooked tensor: every (sample, channel) map gets its orthonormal
// 2-D DCT-II and the squared coefficients are reduced to one fp32 energy per map.
//
// The kernel families are units of their own (codelet.hip, split.hip, fused.hip, fused2.hip, pipe.hip, tile2d.hip,
// tile2g.hip, rect.hip, rank.hip, band.hip, entropy.hip, half.hip). Here:
//   k_energy_direct   any (H, W) <= DCTS_MAX_EDGE: separable cosine-matrix transform with
//                     the basis block staged in LDS; intermediate tile in a caller-provided
//                     workspace (L2-resident). O(H*W*(H+W)) flops per map: the correct
//                     fallback, compute-bound for large tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <mutex>

#include "../../include/dctscore.h"
#include "dcts_internal.h"
#include "grid_caps.h"
#include "rect.h"
#ifdef DCTS_FUSED_STAMPS
#include "split_common.hpp"  // g_fused_stamps
#endif

using namespace dctsi;

namespace {

// ---------------------------------------------------------------------------------------
// direct family: basis tables + separable transform
// ---------------------------------------------------------------------------------------
// Bt[r*n + k] = s_k cos(pi (2r+1) k / (2n)), s_0 = sqrt(1/n), s_k = sqrt(2/n)
__global__ void k_basis(float* __restrict__ Bt, int n) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const int r = idx / n, k = idx - r * n;
  const long long num = ((long long)(2 * r + 1) * k) % (4LL * n);
  const double cv = cospi(double(num) / double(2 * n));
  const double s = (k == 0) ? sqrt(1.0 / double(n)) : sqrt(2.0 / double(n));
  Bt[idx] = float(cv * s);
}

constexpr int kDirectThreads = 256;
constexpr int kKB = 8;  // output rows per basis block

template <bool STORE_COEFF>
__global__ __launch_bounds__(kDirectThreads) void k_energy_direct(
    MapGeom g, int pad, const float* __restrict__ CHt, const float* __restrict__ CWt,
    float* __restrict__ T, float* __restrict__ out) {
  const int HP = g.H + pad, WP = g.W + pad;
  __shared__ __attribute__((aligned(16))) float Bs[DCTS_MAX_EDGE][kKB];
  __shared__ float red[kDirectThreads / 64];
  const int tid = threadIdx.x;
  float* Tm = T + (size_t)blockIdx.x * HP * WP;

  for (long long m = blockIdx.x; m < g.nmaps; m += gridDim.x) {
    const float* xm = map_base(g, m);
    // ---- phase 1: Tm[k][c] = sum_r CH[k][r] x'[r][c] --------------------------------
    for (int k0 = 0; k0 < HP; k0 += kKB) {
      __syncthreads();
      for (int i = tid; i < HP * kKB; i += kDirectThreads) {
        const int r = i / kKB, kk = i - r * kKB;
        Bs[r][kk] = (k0 + kk < HP) ? CHt[r * HP + k0 + kk] : 0.f;
      }
      __syncthreads();
      for (int c = tid; c < WP; c += kDirectThreads) {
        float acc[kKB];
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) acc[kk] = 0.f;
        if (c >= pad) {
          const float* col = xm + (c - pad);
          for (int r = pad; r < HP; ++r) {
            const float xv = col[(long long)(r - pad) * g.strideH];
            const float4 b0 = *reinterpret_cast<const float4*>(&Bs[r][0]);
            const float4 b1 = *reinterpret_cast<const float4*>(&Bs[r][4]);
            acc[0] = fmaf(xv, b0.x, acc[0]);
            acc[1] = fmaf(xv, b0.y, acc[1]);
            acc[2] = fmaf(xv, b0.z, acc[2]);
            acc[3] = fmaf(xv, b0.w, acc[3]);
            acc[4] = fmaf(xv, b1.x, acc[4]);
            acc[5] = fmaf(xv, b1.y, acc[5]);
            acc[6] = fmaf(xv, b1.z, acc[6]);
            acc[7] = fmaf(xv, b1.w, acc[7]);
          }
        }
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk)
          if (k0 + kk < HP) Tm[(k0 + kk) * WP + c] = acc[kk];
      }
    }
    // ---- phase 2: Y[k][l] = sum_c Tm[k][c] CW[l][c]; energy += Y^2 --------------------
    float e = 0.f;
    for (int k0 = 0; k0 < HP; k0 += kKB) {
      __syncthreads();  // also orders phase-1 global stores before these loads (same CU)
      for (int i = tid; i < WP * kKB; i += kDirectThreads) {
        const int cc = i / kKB, kk = i - cc * kKB;
        Bs[cc][kk] = (k0 + kk < HP) ? Tm[(k0 + kk) * WP + cc] : 0.f;
      }
      __syncthreads();
      for (int l = tid; l < WP; l += kDirectThreads) {
        float acc[kKB];
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) acc[kk] = 0.f;
        for (int cc = 0; cc < WP; ++cc) {
          const float wv = CWt[cc * WP + l];
          const float4 b0 = *reinterpret_cast<const float4*>(&Bs[cc][0]);
          const float4 b1 = *reinterpret_cast<const float4*>(&Bs[cc][4]);
          acc[0] = fmaf(wv, b0.x, acc[0]);
          acc[1] = fmaf(wv, b0.y, acc[1]);
          acc[2] = fmaf(wv, b0.z, acc[2]);
          acc[3] = fmaf(wv, b0.w, acc[3]);
          acc[4] = fmaf(wv, b1.x, acc[4]);
          acc[5] = fmaf(wv, b1.y, acc[5]);
          acc[6] = fmaf(wv, b1.z, acc[6]);
          acc[7] = fmaf(wv, b1.w, acc[7]);
        }
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) {
          if (k0 + kk < HP) {
            if constexpr (STORE_COEFF)
              out[(m * HP + k0 + kk) * WP + l] = acc[kk];
            else
              e = fmaf(acc[kk], acc[kk], e);
          }
        }
      }
    }
    if constexpr (!STORE_COEFF) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = e;
      __syncthreads();
      if (tid == 0) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kDirectThreads / 64; ++i) s += red[i];
        out[m] = s;
      }
    }
  }
}

// Batch sum over n of E[n][j] for a 32-channel strip per block: kSumSl = 16 n-slices run in parallel
// (slice s takes n = s, s+16, ...), partials are combined in slice order -> a fixed,
// launch-independent summation order (bit-reproducible, no atomics).
constexpr int kSumCh = 32, kSumSl = 16;
__device__ __forceinline__ float strip_batch_sum(const float* __restrict__ e, long long N,
                                                 long long C, long long j, int slice,
                                                 float (*part)[kSumCh]) {
  float s = 0.f;
  if (j < C) {
    long long n = slice;
    // sixteen loads in flight per lane and round trip (a batch of 256 samples is ONE round trip: the
    // kernel is pure latency, 3.8 us with four loads per trip); the additions keep their order
#pragma unroll 1
    for (; n + 15 * kSumSl < N; n += 16 * kSumSl) {
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = e[(n + i * kSumSl) * C + j];
#pragma unroll
      for (int i = 0; i < 16; ++i) s += a[i];
    }
#pragma unroll 1
    for (; n + 3 * kSumSl < N; n += 4 * kSumSl) {
      const float a0 = e[n * C + j], a1 = e[(n + kSumSl) * C + j];
      const float a2 = e[(n + 2 * kSumSl) * C + j], a3 = e[(n + 3 * kSumSl) * C + j];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; n < N; n += kSumSl) s += e[n * C + j];
  }
  part[slice][threadIdx.x % kSumCh] = s;
  __syncthreads();
  float t = 0.f;
  if (slice == 0) {
#pragma unroll
    for (int i = 0; i < kSumSl; ++i) t += part[i][threadIdx.x % kSumCh];
  }
  return t;  // valid in slice 0
}

// out_c[j] = sum_n e[n*C + j]
__global__ __launch_bounds__(kSumCh * kSumSl) void k_batch_sum(const float* __restrict__ e, long long N,
                                                               long long C, float* __restrict__ out_c) {
  __shared__ float part[kSumSl][kSumCh];
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(e, N, C, j, slice, part);
  if (slice == 0 && j < C) out_c[j] = t;
}

// fr[j] <- (fr[j] * total + sum_n e[n*C + j]) / (total + N): the running-mean update of
// utils/common.py:274-277 fused with the batch sum of :273 (same three fp32 roundings)
__global__ __launch_bounds__(kSumCh * kSumSl) void k_running_mean(const float* __restrict__ e, long long N,
                                                                  long long C, float* __restrict__ fr,
                                                                  float total) {
  __shared__ float part[kSumSl][kSumCh];
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(e, N, C, j, slice, part);
  if (slice == 0 && j < C) {
    const float acc = __fadd_rn(__fmul_rn(fr[j], total), t);
    fr[j] = __fdiv_rn(acc, __fadd_rn(total, float(N)));
  }
}

// the same update for up to kMultiMax hook points in one launch (descriptors by value in the
// kernel arguments): blockIdx.y = hook point, blockIdx.x = 32-channel strip
constexpr int kMultiMax = 64;
struct UpdateBatch {
  dcts_update_desc d[kMultiMax];
};
__global__ __launch_bounds__(kSumCh * kSumSl) void k_running_mean_multi(UpdateBatch b) {
  __shared__ float part[kSumSl][kSumCh];
  const dcts_update_desc d = b.d[blockIdx.y];
  if ((long long)blockIdx.x * kSumCh >= d.C_count) return;  // whole block leaves together
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(d.energy_nc, d.N, d.C_count, j, slice, part);
  if (slice == 0 && j < d.C_count) {
    const float acc = __fadd_rn(__fmul_rn(d.feature_result[j], d.total_before), t);
    d.feature_result[j] = __fdiv_rn(acc, __fadd_rn(d.total_before, float(d.N)));
  }
}

// Score variant in the coefficient domain: out[m] = sum_{u,v} weights[u,v] * coeff[m][u][v]^2.
// One wave per map over dense [HW] coefficient tiles; lanes stride the tile, fixed-order wave sum.
__global__ __launch_bounds__((64 * kReduceWaves)) void k_weighted_energy(const float* __restrict__ coeff, const float* __restrict__ weights,
                                                         long long nmaps, int hw, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long m = wave; m < nmaps; m += nwaves) {
    const float* c = coeff + m * hw;
    float e = 0.f;
    for (int i = lane; i < hw; i += 64) {
      const float v = c[i];
      e = fmaf(weights[i] * v, v, e);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
    if (lane == 0) out[m] = e;
  }
}

// PMC calibration aid: streams n floats with the codelet kernels' access width (one dword per
// lane, consecutive lanes consecutive addresses) so FETCH_SIZE can be compared with a known
// byte count in this exact pattern (MI355X_MICROARCH.md, HBM section: widths other than
// 16 B/lane are uncalibrated).
__global__ __launch_bounds__(256) void k_calib_read(const float* __restrict__ x, long long n,
                                                    float* __restrict__ sink) {
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    s += x[i];
  if (s == 123456.789f) sink[0] = s;  // keeps the loads alive without a store in practice
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
constexpr int kDirectGridCap = 512;

struct DirectWs {
  size_t off_ch, off_cw, off_t, total;
  int grid;
};
DirectWs direct_ws(long long nmaps, int HP, int WP) {
  DirectWs w;
  w.grid = (int)(nmaps < kDirectGridCap ? (nmaps > 0 ? nmaps : 1) : kDirectGridCap);
  w.off_ch = 0;
  w.off_cw = align_up(w.off_ch + (size_t)HP * HP * 4, 256);
  w.off_t = align_up(w.off_cw + (size_t)WP * WP * 4, 256);
  w.total = align_up(w.off_t + (size_t)w.grid * HP * WP * 4, 256);
  return w;
}

// ---- one tensor argument set ------------------------------------------------------------------------------------------
// What an entry point is given for one tensor, and the facts every path derives from it. The derived facts are
// functions: the weighted and band fallbacks re-aim a view at a run of channels of one sample, and nothing goes stale.
struct TensorView {
  const float* x;
  int64_t N, C_total, H, W, strideN, strideC, strideH, strideW;  // strides in elements
  int32_t c_begin, c_count;
  bool pad_front_if_odd;

  int pad() const { return (pad_front_if_odd && (H % 2 != 0)) ? 1 : 0; }  // the test is on H only, the pad on both axes
  int64_t HP() const { return H + pad(); }
  int64_t WP() const { return W + pad(); }
  int64_t nmaps() const { return N * (int64_t)c_count; }
  bool contiguous() const { return N == 1 || strideN == (int64_t)c_count * strideC; }  // map m starts at base() + m * strideC
  const float* base() const { return x + (long long)c_begin * strideC; }
  bool aligned16() const { return (reinterpret_cast<uintptr_t>(base()) & 15) == 0; }
  bool dense_rows() const { return strideW == 1 && strideH == W; }
  bool dense_square() const { return H == W && dense_rows() && strideC == H * W; }  // every map one dense H x H block
  bool dense_maps() const { return dense_square() && contiguous(); }                // and the blocks adjacent: an array of tiles
};

// the list entry points: rows are dense by contract
TensorView view_of(const dcts_tensor_item& t, int64_t H, int64_t W, int32_t pad_front_if_odd) {
  return TensorView{t.x, t.N, t.C_total, H, W, t.strideN, t.strideC, W, 1, t.c_begin, t.c_count, pad_front_if_odd != 0};
}
TensorView view_of(const dcts_shaped_item& it) { return view_of(it.t, it.H, it.W, it.pad_front_if_odd); }

// The argument checks, in the one order every entry point makes them in. `ptrs`: the other device pointers the call requires
// (out, weights), tested for NULL and 4-byte alignment together with x. `shape_ok`: the entry point's own shape condition (the
// band count). The entry points differ only in where they stop:
//   Channels  dcts_weighted_energy_f32: its workspace comes next; the first inner coefficient call checks the rest (so a bad
//             workspace is reported before a bad stride);
//   Align     the list entry points, per item: an edge beyond DCTS_MAX_EDGE or 2^40 maps is found by the per-tensor call;
//   All       everything else.
enum class Checks { Channels, Align, All };
int validate(const TensorView& v, std::initializer_list<const void*> ptrs, Checks upto, bool shape_ok = true) {
  bool null = !v.x, misaligned = (reinterpret_cast<uintptr_t>(v.x) & 3) != 0;
  for (const void* p : ptrs) {
    null = null || !p;
    misaligned = misaligned || (reinterpret_cast<uintptr_t>(p) & 3) != 0;
  }
  if (null) return DCTS_E_NULL;
  if (v.N <= 0 || v.C_total <= 0 || v.H <= 0 || v.W <= 0 || !shape_ok) return DCTS_E_SHAPE;
  if (v.c_count <= 0 || v.c_begin < 0 || (int64_t)v.c_begin + v.c_count > v.C_total) return DCTS_E_CHANNELS;
  if (upto == Checks::Channels) return DCTS_OK;
  if (v.strideW != 1 || v.strideH < v.W) return DCTS_E_STRIDE;
  if (misaligned) return DCTS_E_ALIGN;
  if (upto == Checks::Align) return DCTS_OK;
  if (v.HP() > DCTS_MAX_EDGE || v.WP() > DCTS_MAX_EDGE) return DCTS_E_SHAPE;
  if (v.nmaps() >= (1LL << 40)) return DCTS_E_SHAPE;
  return DCTS_OK;
}

// (aggregates in the field order of dcts_internal.h / rect.h; rect.hip fills in the launch parameters left zero here)
MapGeom map_geom(const TensorView& v) {
  return MapGeom{v.x, v.nmaps(), v.strideN, v.strideC, v.strideH, v.c_count, v.c_begin, (int)v.H, (int)v.W, v.contiguous() ? 1 : 0};
}
RectGeom rect_geom(const TensorView& v) {
  RectGeom r{v.x, v.nmaps(), v.strideN, v.strideC, v.strideH, v.c_count, v.c_begin, (int)v.H, (int)v.W, (int)v.HP(), (int)v.WP(), v.pad()};
  r.contiguous = v.contiguous() ? 1 : 0;
  return r;
}

// ---- how a shape finds its kernel (DESIGN.md, section of that name) -----------------------------------------------
// Every way a call can be served. Direct is api.hip's own cosine-matrix kernel, the others are units of their own.
enum class Family { Direct, Codelet, Lane, CodeletDma, Rect, Split, Fused, Fused2, Pipe, Tile2d, Tile2g, Tile2gPad };
struct FamilyTraits {
  int (*batch)(int, const TileBatch&, hipStream_t);  // its dispatcher if it takes a TileBatch: dense tensors of one shape as one map index space
  bool base16;  // stages with 16-byte direct-to-LDS loads: the first map must lie on a 16-byte boundary (tile2g.hip gathers single
                // dwords, the fused kernels load dwords into registers: any 4-byte-aligned base)
  bool coeff;   // can store coefficients (the large-tile kernels: leaf outputs + k_assemble, 16-byte base then)
};
constexpr FamilyTraits kTraits[] = {
    /* Direct     */ {nullptr, false, true},
    /* Codelet    */ {nullptr, false, true},
    /* Lane       */ {nullptr, false, false},
    /* CodeletDma */ {nullptr, true, false},
    /* Rect       */ {nullptr, false, true},
    /* Split      */ {nullptr, true, false},
    /* Fused      */ {dispatch_fused, false, true},
    /* Fused2     */ {dispatch_fused2, false, true},
    /* Pipe       */ {dispatch_pipe, true, false},
    /* Tile2d     */ {dispatch_tile2d, true, true},
    /* Tile2g     */ {dispatch_tile2g, false, true},
    /* Tile2gPad  */ {dispatch_tile2g_pad, false, false},
};
static_assert(sizeof kTraits / sizeof kTraits[0] == (size_t)Family::Tile2gPad + 1, "one row per Family, in its order");
constexpr FamilyTraits traits(Family f) { return kTraits[(int)f]; }

// the single-launch large-tile families in the order AUTO tries them, each with the explicit request that names it; below,
// which edges each serves
constexpr struct { Family fam; int algo; } kTileOrder[] = {{Family::Tile2g, DCTS_ALGO_TILE2D}, {Family::Tile2d, DCTS_ALGO_TILE2D},
    {Family::Pipe, DCTS_ALGO_PIPE}, {Family::Fused2, DCTS_ALGO_FUSED}, {Family::Fused, DCTS_ALGO_FUSED}};
bool serves(Family f, int HP) {
  switch (f) {
    case Family::Tile2g: return has_tile2g(HP) != 0;
    case Family::Tile2d: return HP == 224;
    case Family::Pipe: return has_pipe(HP) && has_fused(HP);
    case Family::Fused2: return has_fused2(HP);
    case Family::Fused: return has_fused(HP);
    default: return false;
  }
}
// Edges tile2g.hip has but AUTO leaves to the fused / pipelined kernels. Same box, % of the HBM peak, fused / pipelined kernel ->
// tile2g: 72: 30.9 -> 44.1 (9645 maps), 29.7 -> 45.1 (32768); 80: 33.2 -> 40.3, 32.9 -> 37.6; 144: 30.1 -> 33.7 (2411), 32.0 ->
// 42.4 (4992), 31.8 -> 41.0 (8192); 160: 31.2 -> 34.1 (1953), 33.5 -> 37.3 (4096); 128: 45.1 -> 43.3 (3051) but 44.1 -> 50.6
// (8192); 112: 38.8 -> 34.6, 39.8 -> 38.2 (profiles/r03_tile2g_vs_fused_same_box.txt). The choice must not depend on the map
// count: dcts_energy_multi_f32 promises the bits of one call per tensor, whatever the tensors' sizes. So 72, 80, 144, 160 take
// tile2g, 96, 112 and 128 keep the fused / pipelined kernels (DCTS_ALGO_TILE2D still selects it for them).
constexpr bool tile2g_loses(int HP) { return HP == 96 || HP == 112 || HP == 128; }

struct Choice { Family fam; int err; };  // err: DCTS_OK, or DCTS_E_UNSUPPORTED: the requested family has no kernel for this tensor
constexpr Choice kUnsupported{Family::Direct, DCTS_E_UNSUPPORTED};

// The family that serves a validated tensor: the whole policy, nothing launched, no workspace or memo touched. `aligned16`
// is v.aligned16() for a call of its own; dcts_energy_multi_f32 asks what the tensor would take on a 16-byte base.
Choice choose(const TensorView& v, int algo, bool store, bool aligned16) {
  if (algo < DCTS_ALGO_AUTO || algo > DCTS_ALGO_RECT) return kUnsupported;
  const int HP = (int)v.HP(), WP = (int)v.WP(), pad = v.pad();
  auto can = [&](Family f) { return !store || traits(f).coeff; };

  // 1. small tiles. Both edges have a 1-D codelet, but the maps are not square or their rows not dense: the run-time pair of
  // codelets (rect.hip). Square dense-row maps keep their own kernels unless ALGO_RECT asks (tests compare the two).
  const bool codelet_ok = has_codelet(HP, WP) && v.dense_rows();
  const bool lane_ok = codelet_ok && can(Family::Lane) && pad == 0 && has_lane_kernel(HP);
  const bool rect_ok = HP <= 64 && WP <= 64 && has_rect(HP, WP) != 0;
  if ((algo == DCTS_ALGO_CODELET || algo == DCTS_ALGO_PREFETCH) && !codelet_ok) return kUnsupported;
  if (algo == DCTS_ALGO_LANE && !lane_ok) return kUnsupported;
  if (algo == DCTS_ALGO_RECT && !rect_ok) return kUnsupported;
  if (rect_ok && (algo == DCTS_ALGO_RECT || (algo == DCTS_ALGO_AUTO && !codelet_ok))) return {Family::Rect, DCTS_OK};
  if (codelet_ok && algo != DCTS_ALGO_DIRECT) {  // (a request for a large-tile family is served by the codelet kernel too)
    if (lane_ok && (algo == DCTS_ALGO_AUTO || algo == DCTS_ALGO_LANE)) return {Family::Lane, DCTS_OK};
    // the prefetching variant is opt-in: on MI355X it measured equal to the register-load kernel in steady state (both at the
    // practical HBM rate) and ~2 % slower on the bench. Dense, 16-byte aligned, even-edge unpadded tiles only.
    if (algo == DCTS_ALGO_PREFETCH) {
      const bool dma_ok = can(Family::CodeletDma) && pad == 0 && HP % 2 == 0 && v.dense_maps() && aligned16;
      return dma_ok ? Choice{Family::CodeletDma, DCTS_OK} : kUnsupported;
    }
    return {Family::Codelet, DCTS_OK};
  }

  // 2. large tiles: arrays of dense unpadded square tiles of a split-table edge
  const bool tile_shape = has_split(HP, WP) && pad == 0 && v.dense_maps();
  if (store) {
    // coefficients through the large-tile kernels themselves, on request only: the parity tests check with them that those kernels
    // compute the DCT and not merely its energy. (An edge of the split table that the family lacks is refused by its dispatcher.)
    if (algo == DCTS_ALGO_SPLIT || algo == DCTS_ALGO_PIPE) return kUnsupported;  // neither family stores coefficients
    if (algo == DCTS_ALGO_TILE2D || algo == DCTS_ALGO_FUSED) {
      if (!tile_shape || !aligned16) return kUnsupported;
      if (algo == DCTS_ALGO_TILE2D) return {HP == 224 ? Family::Tile2d : Family::Tile2g, DCTS_OK};
      return {has_fused2(HP) ? Family::Fused2 : Family::Fused, DCTS_OK};
    }
    return {Family::Direct, DCTS_OK};
  }
  const bool split_ok = tile_shape && aligned16;  // pass 2 stages the intermediate as pass 1 stages the maps
  if (algo == DCTS_ALGO_SPLIT && !split_ok) return kUnsupported;
  if (algo == DCTS_ALGO_AUTO || algo == DCTS_ALGO_FUSED || algo == DCTS_ALGO_PIPE || algo == DCTS_ALGO_TILE2D) {
    // AUTO order: several-maps-per-round 2-D split (tile2g.hip), 2-D split (tile2d.hip; 224: 33-42 % of the HBM peak against
    // 31-37 % pipelined, same box, 996...16384 maps), pipelined, two roles per wave (288: 31 % vs 18 %, 320: 31 % vs 17 % of the
    // HBM peak for the fused kernel), fused
    if (tile_shape)
      for (const auto& t : kTileOrder) {
        const Family f = t.fam;
        if ((algo != DCTS_ALGO_AUTO && algo != t.algo) || !serves(f, HP)) continue;
        if (!aligned16 && traits(f).base16) continue;
        // (kept as found, DESIGN.md: the measured exception holds on a 16-byte base only, so a 4-byte base takes tile2g at 96, 112, 128)
        if (f == Family::Tile2g && algo == DCTS_ALGO_AUTO && aligned16 && tile2g_loses(HP)) continue;
        return {f, DCTS_OK};
      }
    // 71 / 79 / 143 / 159 with the odd front pad (the cv2 path on odd maps): tile2g.hip pads while it gathers
    if (pad == 1 && v.dense_maps() && (algo == DCTS_ALGO_AUTO || algo == DCTS_ALGO_TILE2D) && has_tile2g_pad(HP))
      return {Family::Tile2gPad, DCTS_OK};
    if (algo != DCTS_ALGO_AUTO) return kUnsupported;
  }
  // 3. two launches with the intermediate in the workspace, else the cosine-matrix kernel
  if (split_ok && algo != DCTS_ALGO_DIRECT) return {Family::Split, DCTS_OK};
  return {Family::Direct, DCTS_OK};
}

// one tensor as a batch of one
TileBatch single_batch(const TensorView& v, float* out) {
  TileBatch tb;
  for (int i = 0; i < kTileItems; ++i) {
    tb.x[i] = v.base();
    tb.out[i] = out;
    tb.begin[i] = 0;
  }
  tb.begin[1] = tb.begin[kTileItems] = v.nmaps();
  tb.map_elems = v.strideC;
  tb.total = v.nmaps();
  tb.count = 1;
  return tb;
}

// The direct kernel's basis tables live at the head of the caller's workspace. They are built once per
// (workspace, stream, H', W') and reused by later calls: the library remembers - on the host, nothing is read
// back - which BYTE RANGE of which workspace holds tables, and forgets an entry whenever any of its own paths
// is about to write bytes that overlap that range (another shape's tables, the direct kernel's T tiles, the
// split path's intermediate, the coefficient path's leaf outputs, the weighted path's coefficient chunk) or the
// caller says so (dcts_workspace_invalidate[_range]). Same stream only: that is what orders the build before
// the reuse. Calls that receive an INTERIOR pointer of a caller's workspace (the weighted path's inner calls)
// never cache: an interior offset depends on the tile shape, and the caller cannot name it to invalidate it.
struct BasisSlot {
  uintptr_t lo, hi;  // bytes [lo, hi) hold the two tables
  void* ws;          // the workspace pointer the call was made with
  void* stream;
  int HP, WP;
};
constexpr int kBasisSlots = 16;
BasisSlot g_basis[kBasisSlots] = {};
int g_basis_next = 0;
std::mutex g_basis_mu;

bool basis_cached(void* ws, void* stream, int HP, int WP) {
  std::lock_guard<std::mutex> lk(g_basis_mu);
  for (const BasisSlot& b : g_basis)
    if (b.hi && b.ws == ws && b.stream == stream && b.HP == HP && b.WP == WP) return true;
  return false;
}
// forget every entry whose tables overlap [p, p + bytes)
void basis_forget_range(const void* p, size_t bytes) {
  if (!p || !bytes) return;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
  std::lock_guard<std::mutex> lk(g_basis_mu);
  for (BasisSlot& b : g_basis)
    if (b.hi && b.lo < hi && lo < b.hi) b = BasisSlot{};
}
// the caller names a workspace by its base pointer only: forget what was cached under that pointer and
// whatever tables contain that address
void basis_forget(void* ws) {
  if (!ws) return;
  const uintptr_t a = reinterpret_cast<uintptr_t>(ws);
  std::lock_guard<std::mutex> lk(g_basis_mu);
  for (BasisSlot& b : g_basis)
    if (b.hi && (b.ws == ws || (b.lo <= a && a < b.hi))) b = BasisSlot{};
}
void basis_remember(void* ws, const void* tables, size_t table_bytes, void* stream, int HP, int WP) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(tables), hi = lo + table_bytes;
  std::lock_guard<std::mutex> lk(g_basis_mu);
  for (BasisSlot& b : g_basis)
    if (b.hi && (b.ws == ws || (b.lo < hi && lo < b.hi))) b = BasisSlot{};  // one shape per workspace, no overlapping tables
  g_basis[g_basis_next] = BasisSlot{lo, hi, ws, stream, HP, WP};
  g_basis_next = (g_basis_next + 1) % kBasisSlots;
}

// One tensor, energies (out is [N, c_count]) or coefficients (store: out is [N, c_count, H', W']): validate -> choose -> launch.
int run(bool store, const TensorView& v, float* out, void* workspace, size_t workspace_bytes, void* stream, int32_t algo,
        bool cache_basis = true) {
  if (const int rc = validate(v, {out}, Checks::All)) return rc;
  const Choice c = choose(v, algo, store, v.aligned16());
  if (c.err) return c.err;
  const int HP = (int)v.HP(), WP = (int)v.WP(), pad = v.pad();
  const MapGeom g = map_geom(v);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (c.fam) {
    case Family::Rect: return dispatch_rect(rect_geom(v), out, store ? 1 : 0, st);
    case Family::CodeletDma: return dispatch_codelet_dma(HP, g, out, st);
    case Family::Codelet: return dispatch_codelet(store ? 1 : 0, HP, WP, pad, g, out, st);
    case Family::Direct: break;
    case Family::Lane: {
      MultiGeom mg;
      for (int i = 0; i < kMultiItems; ++i) mg.it[i] = MultiItem{g, out, 0};
      mg.total_groups = (g.nmaps + 63) / 64;
      mg.count = 1;
      return dispatch_lane(HP, mg, st);
    }
    case Family::Split: {
      const SplitWs sws = split_ws(g.nmaps, HP);
      if (!workspace || workspace_bytes < sws.total) return DCTS_E_WORKSPACE;
      if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;  // pass 2 stages the intermediate the same way
      basis_forget_range(workspace, sws.total);
      return dispatch_split(HP, g, out, workspace, st);
    }
    default: {  // the TileBatch families
      if (!store) return traits(c.fam).batch(HP, single_batch(v, out), st);
      // leaf outputs of as many maps as the workspace holds, then k_assemble
      const long long tile_bytes = (long long)HP * WP * 4;
      const long long ws_maps = workspace ? (long long)(workspace_bytes / (size_t)tile_bytes) : 0;
      if (ws_maps < 1 || (reinterpret_cast<uintptr_t>(workspace) & 15)) return DCTS_E_WORKSPACE;
      float* scratch = reinterpret_cast<float*>(workspace);
      basis_forget_range(workspace, workspace_bytes);
      switch (c.fam) {
        case Family::Tile2d: return dispatch_tile2d_coeff(HP, v.base(), g.nmaps, out, scratch, ws_maps, st);
        case Family::Tile2g: return dispatch_tile2g_coeff(HP, v.base(), g.nmaps, out, scratch, ws_maps, st);
        case Family::Fused2: return dispatch_fused2_coeff(HP, v.base(), g.nmaps, out, scratch, ws_maps, st);
        default: return dispatch_fused_coeff(HP, v.base(), g.nmaps, out, scratch, ws_maps, st);
      }
    }
  }

  const DirectWs ws = direct_ws(g.nmaps, HP, WP);
  if (!workspace) return ws.total ? DCTS_E_WORKSPACE : DCTS_E_NULL;
  if (workspace_bytes < ws.total) return DCTS_E_WORKSPACE;
  char* wsp = reinterpret_cast<char*>(workspace);
  float* CHt = reinterpret_cast<float*>(wsp + ws.off_ch);
  float* CWt = reinterpret_cast<float*>(wsp + ws.off_cw);
  float* T = reinterpret_cast<float*>(wsp + ws.off_t);
  if (!cache_basis || !basis_cached(workspace, stream, HP, WP)) {
    basis_forget_range(workspace, ws.total);  // whatever tables lay in the bytes this call uses are gone
    hipLaunchKernelGGL(k_basis, dim3((unsigned)((HP * HP + 255) / 256)), dim3(256), 0, st, CHt, HP);
    hipLaunchKernelGGL(k_basis, dim3((unsigned)((WP * WP + 255) / 256)), dim3(256), 0, st, CWt, WP);
    if (cache_basis && hipGetLastError() == hipSuccess)
      basis_remember(workspace, wsp + ws.off_ch, ws.off_t - ws.off_ch, stream, HP, WP);
  } else {
    basis_forget_range(wsp + ws.off_t, ws.total - ws.off_t);  // the T tiles may cover another entry's tables
  }
  hipLaunchKernelGGL(store ? k_energy_direct<true> : k_energy_direct<false>, dim3((unsigned)ws.grid), dim3(kDirectThreads), 0, st,
                     g, pad, CHt, CWt, T, out);
  return (int)hipGetLastError();
}

// ---- the coefficient fallback of the weighted and band entry points ------------------------------------------------
// Which coefficient path their inner calls ask for: the large-tile kernels' own where the tensor suits them, else whatever
// AUTO picks (codelet / rect / direct). Every inner call covers whole samples or channels of ONE sample, so a sample
// stride that keeps each sample's base on a 16-byte boundary stands in for adjacency.
int coeff_algo(const TensorView& v) {
  const int HP = (int)v.HP();
  if (v.pad() != 0 || !v.dense_square() || (v.strideN * 4) % 16 != 0 || !v.aligned16()) return DCTS_ALGO_AUTO;
  if (serves(Family::Tile2d, HP) || serves(Family::Tile2g, HP)) return DCTS_ALGO_TILE2D;
  if (serves(Family::Fused, HP) || serves(Family::Fused2, HP)) return DCTS_ALGO_FUSED;
  return DCTS_ALGO_AUTO;
}

// Sample by sample, runs of at most `chunk` channels (one strided view of x each): coefficients into `coeff` through the
// coefficient path (scratch: `inner`), then reduce(n, c0, nc) over the nc tiles just written.
template <class Reduce>
int coeff_chunks_per_sample(const TensorView& v, long long chunk, int algo, float* coeff, void* inner, size_t inner_bytes,
                            void* stream, Reduce reduce) {
  for (int64_t n = 0; n < v.N; ++n) {
    for (long long c0 = 0; c0 < v.c_count; c0 += chunk) {
      const long long nc = (v.c_count - c0) < chunk ? (v.c_count - c0) : chunk;
      TensorView s = v;
      s.x = v.x + n * v.strideN;
      s.N = 1;
      s.c_begin = (int32_t)(v.c_begin + c0);
      s.c_count = (int32_t)nc;
      int rc = run(true, s, coeff, inner, inner_bytes, stream, algo, /*cache_basis=*/false);
      if (rc) return rc;
      rc = reduce(n, c0, nc);
      if (rc) return rc;
    }
  }
  return DCTS_OK;
}

}  // namespace

extern "C" {

int dcts_version(void) { return DCTS_ABI_VERSION; }

const char* dcts_strerror(int code) {
  switch (code) {
    case DCTS_OK: return "ok";
    case DCTS_E_NULL: return "required pointer is NULL";
    case DCTS_E_SHAPE: return "bad shape (N, C, H, W must be > 0 and tile edges <= 512)";
    case DCTS_E_CHANNELS: return "channel slice outside [0, C_total)";
    case DCTS_E_STRIDE: return "rows must be dense: strideW == 1 and strideH >= W";
    case DCTS_E_WORKSPACE: return "workspace missing or smaller than dcts_workspace_bytes()";
    case DCTS_E_UNSUPPORTED: return "no kernel of the requested family for this shape (rank: edges up to 64), or an unknown dtype";
    case DCTS_E_ALIGN: return "pointer not aligned: element size (tensors: 4 bytes, fp16 / bf16 input 2), 16 bytes (workspace)";
    default: break;
  }
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "unknown dctscore error";
}

size_t dcts_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  // worst case: odd front pad taken, direct kernel used
  const int64_t HP = H + 1, WP = W + 1;
  size_t need = direct_ws(N * C_count, (int)HP, (int)WP).total;
  if (has_split(H, W)) {
    const size_t s = split_ws(N * C_count, (int)H).total;
    if (s > need) need = s;
  }
  return need;
}

int dcts_has_codelet(int64_t H, int64_t W) { return has_codelet(H, W) ? 1 : 0; }

void dcts_workspace_invalidate(void* workspace) { basis_forget(workspace); }

void dcts_workspace_invalidate_range(void* workspace, size_t bytes) {
  basis_forget(workspace);
  basis_forget_range(workspace, bytes);
}

int dcts_energy_f32_ex(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                       int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                       int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                       float* out_nc, void* workspace, size_t workspace_bytes, void* stream,
                       int32_t algo) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  return run(false, v, out_nc, workspace, workspace_bytes, stream, algo);
}

int dcts_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                    int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                    int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd, float* out_nc,
                    void* workspace, size_t workspace_bytes, void* stream) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  return run(false, v, out_nc, workspace, workspace_bytes, stream, DCTS_ALGO_AUTO);
}

int dcts_dct2d_f32_ex(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                      int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                      int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                      float* out_coeff, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t algo) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  return run(true, v, out_coeff, workspace, workspace_bytes, stream, algo);
}

int dcts_dct2d_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                   int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                   int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd, float* out_coeff,
                   void* workspace, size_t workspace_bytes, void* stream) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  return run(true, v, out_coeff, workspace, workspace_bytes, stream, DCTS_ALGO_AUTO);
}

size_t dcts_weighted_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  // coefficients of a chunk of maps + what the coefficient path itself needs for that chunk
  const int64_t HP = H + 1, WP = W + 1;
  const long long tile = (long long)HP * WP * 4;
  long long chunk = (256LL << 20) / tile;  // 256 MiB of coefficients per chunk at most
  if (chunk < 1) chunk = 1;
  if (chunk > N * C_count) chunk = N * C_count;
  return align_up((size_t)(chunk * tile), 256) + align_up((size_t)(chunk * tile), 256) + dcts_workspace_bytes(N, C_count, H, W);
}

int dcts_weighted_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                             int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                             int32_t pad_front_if_odd, const float* weights, float* out_nc, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  if (const int rc = validate(v, {out_nc, weights}, Checks::Channels)) return rc;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return workspace ? DCTS_E_ALIGN : DCTS_E_WORKSPACE;
  const long long tile = (long long)v.HP() * v.WP() * 4;
  // workspace = [coefficients of a chunk][scratch the coefficient path may use]
  const size_t inner_min = dcts_workspace_bytes(1, 1, H, W);
  if (workspace_bytes < (size_t)(2 * tile) + inner_min) return DCTS_E_WORKSPACE;
  long long chunk = (long long)((workspace_bytes - inner_min) / (size_t)(2 * tile));
  if (chunk < 1) return DCTS_E_WORKSPACE;
  const size_t off_inner = align_up((size_t)(chunk * tile), 256);
  if (off_inner + (size_t)(chunk * tile) > workspace_bytes) --chunk;
  if (chunk < 1) return DCTS_E_WORKSPACE;
  char* wsp = reinterpret_cast<char*>(workspace);
  float* coeff = reinterpret_cast<float*>(wsp);
  void* inner = wsp + align_up((size_t)(chunk * tile), 256);
  const size_t inner_bytes = workspace_bytes - align_up((size_t)(chunk * tile), 256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // this call writes coefficients and scratch all over the workspace: no table cached in it survives, and the
  // inner calls (interior pointer, offset depends on the tile shape) do not cache theirs
  basis_forget(workspace);
  basis_forget_range(workspace, workspace_bytes);
  const int hw = (int)(v.HP() * v.WP());
  return coeff_chunks_per_sample(v, chunk, coeff_algo(v), coeff, inner, inner_bytes, stream, [&](int64_t n, long long c0, long long nc) {
    long long blocks = (nc + kReduceWaves - 1) / kReduceWaves;  // one wave per map
    if (blocks > kReduceMaxBlocks) blocks = kReduceMaxBlocks;
    hipLaunchKernelGGL(k_weighted_energy, dim3((unsigned)blocks), dim3(64 * kReduceWaves), 0, st, coeff, weights, nc, hw, out_nc + n * c_count + c0);
    return (int)hipGetLastError();
  });
}

// ---- K weighted energies per map (band.hip) ------------------------------------------------------------------------
// Fallback workspace: [coefficients of a chunk of maps][what the coefficient path needs for that chunk: the direct
// kernel's tables and T tiles, or leaf tiles of the large-tile kernels]. Both parts are at most align(chunk * tile).
static long long band_fallback_chunk(size_t workspace_bytes, int HP, int WP) {
  const size_t tile = (size_t)HP * WP * 4;
  const size_t fixed = direct_ws(1, HP, WP).off_t + 512;
  if (workspace_bytes < fixed + 2 * tile) return 0;
  return (long long)((workspace_bytes - fixed) / (2 * tile));
}

size_t dcts_band_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W, int32_t K) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0 || K < 1 || K > DCTS_BAND_MAX) return 0;
  if (H + 1 > DCTS_MAX_EDGE + 1 || W + 1 > DCTS_MAX_EDGE + 1) return 0;
  // worst case: odd front pad taken. Shapes the fused kernel serves meet the fallback only as row-pitched views.
  const int HP = (int)H + 1, WP = (int)W + 1;
  const long long tile = (long long)HP * WP * 4;
  const long long cap = band_chunk_bytes(HP, WP);  // bytes of coefficients per chunk (grid_caps.h)
  long long chunk = cap / tile;
  if (chunk < 1) chunk = 1;
  if (chunk > N * C_count) chunk = N * C_count;
  const size_t fallback = direct_ws(1, HP, WP).off_t + 512 + 2 * (size_t)(chunk * tile);
  const size_t table = band_table_bytes(HP, WP, K);
  return align_up(fallback > table ? fallback : table, 256);
}

int dcts_has_band_kernel(int64_t H, int64_t W) { return has_codelet(H, W) ? 1 : 0; }

int dcts_band_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                         int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                         int32_t pad_front_if_odd, const float* weights, int32_t K, float* out_nck, void* workspace,
                         size_t workspace_bytes, void* stream, int32_t algo) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  if (const int rc = validate(v, {out_nck, weights}, Checks::All, /*shape_ok=*/K >= 1 && K <= DCTS_BAND_MAX)) return rc;
  const int HP = (int)v.HP(), WP = (int)v.WP();
  if (algo != DCTS_ALGO_AUTO && algo != DCTS_ALGO_CODELET && algo != DCTS_ALGO_DIRECT) return DCTS_E_UNSUPPORTED;
  const bool fused_ok = has_codelet(HP, WP) && v.dense_rows();
  if (algo == DCTS_ALGO_CODELET && !fused_ok) return DCTS_E_UNSUPPORTED;
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  if (fused_ok && algo != DCTS_ALGO_DIRECT) {
    const size_t table_bytes = band_table_bytes(HP, WP, K);
    if (workspace_bytes < table_bytes) return DCTS_E_WORKSPACE;
    basis_forget_range(workspace, table_bytes);  // the table overwrites whatever basis tables lay there
    return dispatch_band(HP, v.pad(), map_geom(v), weights, K, reinterpret_cast<float*>(workspace), out_nck, st);
  }

  // fallback: coefficients of a chunk of maps through the coefficient path, then one reduction that reads each
  // coefficient once for all K bands
  long long chunk = band_fallback_chunk(workspace_bytes, HP, WP);
  if (chunk < 1) return DCTS_E_WORKSPACE;
  const long long tile = (long long)HP * WP * 4;
  char* wsp = reinterpret_cast<char*>(workspace);
  float* coeff = reinterpret_cast<float*>(wsp);
  const size_t off_inner = align_up((size_t)(chunk * tile), 256);
  void* inner = wsp + off_inner;
  const size_t inner_bytes = workspace_bytes - off_inner;
  // this call writes coefficients and scratch all over the workspace: no table cached in it survives, and the inner
  // calls (interior pointer) do not cache theirs
  basis_forget(workspace);
  basis_forget_range(workspace, workspace_bytes);
  const int inner_algo = coeff_algo(v);
  const int hw = HP * WP;
  if (chunk >= c_count && (v.contiguous() || inner_algo == DCTS_ALGO_AUTO)) {
    // whole samples per chunk: (n, channel) jointly, one strided view of x per call
    const int64_t ns = chunk / c_count;
    for (int64_t n0 = 0; n0 < N; n0 += ns) {
      TensorView s = v;
      s.x = x + n0 * strideN;
      s.N = (N - n0) < ns ? (N - n0) : ns;
      int rc = run(true, s, coeff, inner, inner_bytes, stream, inner_algo, /*cache_basis=*/false);
      if (rc) return rc;
      rc = launch_band_reduce(coeff, weights, s.N * c_count, hw, K, out_nck + n0 * c_count * K, st);
      if (rc) return rc;
    }
    return DCTS_OK;
  }
  if (chunk > c_count) chunk = c_count;
  return coeff_chunks_per_sample(v, chunk, inner_algo, coeff, inner, inner_bytes, stream, [&](int64_t n, long long c0, long long nc) {
    return launch_band_reduce(coeff, weights, nc, hw, K, out_nck + (n * c_count + c0) * K, st);
  });
}

// ---- the spectral entropy of every map (entropy.hip) -----------------------------------------------------------------
// The fused kernel needs no workspace. The fallback lays its workspace out as the band fallback does and chunks by what it
// is given: [coefficients of a chunk of maps][what the coefficient path needs for that chunk].
size_t dcts_entropy_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  if (H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return 0;
  // 0 where the fused kernel takes the tile with and without the odd front pad (dense rows)
  if (has_codelet(H, W) && (H % 2 == 0 || has_codelet(H + 1, W + 1))) return 0;
  // worst case: odd front pad taken
  const int HP = (int)H + 1, WP = (int)W + 1;
  const long long tile = (long long)HP * WP * 4;
  long long chunk = band_chunk_bytes(HP, WP) / tile;  // bytes of coefficients per chunk (grid_caps.h)
  if (chunk < 1) chunk = 1;
  if (chunk > N * C_count) chunk = N * C_count;
  return align_up(direct_ws(1, HP, WP).off_t + 512 + 2 * (size_t)(chunk * tile), 256);
}

int dcts_has_entropy_kernel(int64_t H, int64_t W) { return has_codelet(H, W) ? 1 : 0; }

int dcts_spectral_entropy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                              int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                              int32_t pad_front_if_odd, float* out_nc, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t algo) {
  const TensorView v{x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
  if (const int rc = validate(v, {out_nc}, Checks::All)) return rc;
  const int HP = (int)v.HP(), WP = (int)v.WP();
  if (algo != DCTS_ALGO_AUTO && algo != DCTS_ALGO_CODELET && algo != DCTS_ALGO_DIRECT) return DCTS_E_UNSUPPORTED;
  const bool fused_ok = has_codelet(HP, WP) && v.dense_rows();
  if (algo == DCTS_ALGO_CODELET && !fused_ok) return DCTS_E_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (fused_ok && algo != DCTS_ALGO_DIRECT) return dispatch_entropy(HP, v.pad(), map_geom(v), out_nc, st);

  // fallback: orthonormal coefficients of a chunk of maps through the coefficient path, then one reduction that reads
  // each coefficient once
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  long long chunk = band_fallback_chunk(workspace_bytes, HP, WP);
  if (chunk < 1) return DCTS_E_WORKSPACE;
  const long long tile = (long long)HP * WP * 4;
  char* wsp = reinterpret_cast<char*>(workspace);
  float* coeff = reinterpret_cast<float*>(wsp);
  const size_t off_inner = align_up((size_t)(chunk * tile), 256);
  void* inner = wsp + off_inner;
  const size_t inner_bytes = workspace_bytes - off_inner;
  // this call writes coefficients and scratch all over the workspace: no table cached in it survives, and the inner
  // calls (interior pointer) do not cache theirs
  basis_forget(workspace);
  basis_forget_range(workspace, workspace_bytes);
  const int inner_algo = coeff_algo(v);
  const int hw = HP * WP;
  if (chunk >= c_count && (v.contiguous() || inner_algo == DCTS_ALGO_AUTO)) {
    // whole samples per chunk: (n, channel) jointly, one strided view of x per call
    const int64_t ns = chunk / c_count;
    for (int64_t n0 = 0; n0 < N; n0 += ns) {
      TensorView s = v;
      s.x = x + n0 * strideN;
      s.N = (N - n0) < ns ? (N - n0) : ns;
      int rc = run(true, s, coeff, inner, inner_bytes, stream, inner_algo, /*cache_basis=*/false);
      if (rc) return rc;
      rc = launch_entropy_reduce(coeff, s.N * c_count, hw, out_nc + n0 * c_count, st);
      if (rc) return rc;
    }
    return DCTS_OK;
  }
  if (chunk > c_count) chunk = c_count;
  return coeff_chunks_per_sample(v, chunk, inner_algo, coeff, inner, inner_bytes, stream, [&](int64_t n, long long c0, long long nc) {
    return launch_entropy_reduce(coeff, nc, hw, out_nc + n * c_count + c0, st);
  });
}

// ---- fp16 / bf16 inputs (half.hip) -----------------------------------------------------------------------------------
// The staged route's workspace: [what the fp32 path needs for the chunk it is given][dense fp32 copy of a chunk of maps].
// The fp32 part is at the head, so that a direct-kernel call keeps its tables where dcts_energy_f32 would: run() is called as
// dcts_energy_f32 calls it, so the EXISTING basis-table memo (keyed on the caller's workspace pointer, forgotten through
// dcts_workspace_invalidate[_range]) serves the staged route as well. That is the only host state it touches; none is added.
// (at most kHalfStageCap bytes of upcast maps per chunk: grid_caps.h)

static bool is_half_dtype(int32_t dtype) { return dtype == DCTS_DTYPE_F16 || dtype == DCTS_DTYPE_BF16; }

size_t dcts_typed_workspace_bytes(int32_t dtype, int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (dtype == DCTS_DTYPE_F32) return dcts_workspace_bytes(N, C_count, H, W);
  if (!is_half_dtype(dtype) || N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  if (H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return 0;
  if (has_half(H, W)) return 0;
  const size_t map = (size_t)H * W * 4;
  size_t stage = (size_t)(N * C_count) * map;
  if (stage > kHalfStageCap) stage = kHalfStageCap > map ? kHalfStageCap / map * map : map;
  return align_up(dcts_workspace_bytes(N, C_count, H, W), 256) + align_up(stage, 256);
}

int dcts_has_half_kernel(int64_t H, int64_t W) { return has_half(H, W) ? 1 : 0; }

int dcts_energy_typed(const void* x, int32_t dtype, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                      int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                      int32_t pad_front_if_odd, float* out_nc, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype == DCTS_DTYPE_F32)
    return dcts_energy_f32(reinterpret_cast<const float*>(x), N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin,
                           c_count, pad_front_if_odd, out_nc, workspace, workspace_bytes, stream);
  if (!is_half_dtype(dtype)) return DCTS_E_UNSUPPORTED;
  // the checks of validate(), in its order, with the element size in the alignment test
  if (!x || !out_nc) return DCTS_E_NULL;
  if (N <= 0 || C_total <= 0 || H <= 0 || W <= 0) return DCTS_E_SHAPE;
  if (c_count <= 0 || c_begin < 0 || (int64_t)c_begin + c_count > C_total) return DCTS_E_CHANNELS;
  if (strideW != 1 || strideH < W) return DCTS_E_STRIDE;
  if ((reinterpret_cast<uintptr_t>(x) & 1) || (reinterpret_cast<uintptr_t>(out_nc) & 3)) return DCTS_E_ALIGN;
  const int pad = (pad_front_if_odd && (H % 2 != 0)) ? 1 : 0;
  if (H + pad > DCTS_MAX_EDGE || W + pad > DCTS_MAX_EDGE) return DCTS_E_SHAPE;
  if (N * (int64_t)c_count >= (1LL << 40)) return DCTS_E_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* xh = reinterpret_cast<const uint16_t*>(x);
  const bool contiguous = N == 1 || strideN == (int64_t)c_count * strideC;

  if (has_half(H, W) && pad == 0 && strideH == W) {
    const HalfGeom g{xh, N * (int64_t)c_count, strideN, strideC, c_count, c_begin, contiguous ? 1 : 0};
    return dispatch_half((int)H, dtype, g, out_nc, st);
  }

  // staged: upcast a chunk of maps into the workspace, score it through the fp32 path under AUTO. Whole samples per chunk
  // where the workspace holds one, else runs of channels of one sample (as the band fallback chunks).
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  const size_t map = (size_t)H * W * 4;
  // Sized for the whole call and handed to every chunk: direct_ws() and split_ws() never shrink as the map count grows, so
  // what N * c_count maps need covers any chunk of them (and run() itself refuses a workspace that is too small).
  const size_t inner_bytes = align_up(dcts_workspace_bytes(N, c_count, H, W), 256);
  if (workspace_bytes < inner_bytes + map) return DCTS_E_WORKSPACE;
  long long chunk = (long long)((workspace_bytes - inner_bytes) / map);
  if ((size_t)chunk * map > kHalfStageCap && kHalfStageCap >= map) chunk = (long long)(kHalfStageCap / map);
  float* stage = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + inner_bytes);
  void* inner = inner_bytes ? workspace : nullptr;
  basis_forget_range(stage, (size_t)chunk * map);  // the upcast maps overwrite whatever tables lay there
  auto score = [&](int64_t n0, int64_t ns, int32_t c0, int32_t nc) -> int {
    // samples [n0, n0 + ns), channels [c_begin + c0, c_begin + c0 + nc) of x
    const HalfGeom g{xh + n0 * strideN, ns * (int64_t)nc, strideN, strideC, nc, c_begin + c0,
                     (ns == 1 || strideN == (int64_t)nc * strideC) ? 1 : 0};
    int rc = launch_upcast_half(dtype, g, (int)H, (int)W, strideH, stage, st);
    if (rc) return rc;
    const TensorView v{stage, ns, nc, H, W, (int64_t)nc * H * W, H * W, W, 1, 0, nc, pad_front_if_odd != 0};
    return run(false, v, out_nc + n0 * c_count + c0, inner, inner_bytes, stream, DCTS_ALGO_AUTO);
  };
  if (chunk >= c_count) {
    const int64_t ns = chunk / c_count;
    for (int64_t n0 = 0; n0 < N; n0 += ns)
      if (const int rc = score(n0, (N - n0) < ns ? (N - n0) : ns, 0, c_count)) return rc;
    return DCTS_OK;
  }
  for (int64_t n = 0; n < N; ++n)
    for (int64_t c0 = 0; c0 < c_count; c0 += chunk)
      if (const int rc = score(n, 1, (int32_t)c0, (int32_t)((c_count - c0) < chunk ? (c_count - c0) : chunk))) return rc;
  return DCTS_OK;
}

// ---- channels-last maps (nhwc.hip) ------------------------------------------------------------------------------------
int dcts_has_nhwc_kernel(int64_t H, int64_t W) { return has_nhwc(H, W) ? 1 : 0; }

// nothing is staged: the native kernels read the tensor where it lies, and every other shape is refused
size_t dcts_nhwc_workspace_bytes(int32_t, int64_t, int64_t, int64_t, int64_t) { return 0; }

int dcts_energy_nhwc(const void* x, int32_t dtype, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                     int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, float* out_nc, void* workspace,
                     size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (dtype != DCTS_DTYPE_F32 && !is_half_dtype(dtype)) return DCTS_E_UNSUPPORTED;
  // the checks of dcts_energy_typed, in its order; the stride rules are those of the channels-last layout
  if (!x || !out_nc) return DCTS_E_NULL;
  if (N <= 0 || C_total <= 0 || H <= 0 || W <= 0) return DCTS_E_SHAPE;
  if (c_count <= 0 || c_begin < 0 || (int64_t)c_begin + c_count > C_total) return DCTS_E_CHANNELS;
  if (strideW < C_total || strideH / W < strideW) return DCTS_E_STRIDE;  // strideH >= W * strideW without the product
  const uintptr_t elem_mask = dtype == DCTS_DTYPE_F32 ? 3 : 1;
  if ((reinterpret_cast<uintptr_t>(x) & elem_mask) || (reinterpret_cast<uintptr_t>(out_nc) & 3)) return DCTS_E_ALIGN;
  if (H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return DCTS_E_SHAPE;
  if (N * (int64_t)c_count >= (1LL << 40)) return DCTS_E_SHAPE;
  if (!has_nhwc(H, W)) return DCTS_E_UNSUPPORTED;  // the caller's copy into the NCHW layout stays the caller's
  const NhwcGeom g{x, N, strideN, strideH, strideW, c_begin, c_count};
  return dispatch_nhwc((int)H, dtype, g, out_nc, reinterpret_cast<hipStream_t>(stream));
}

int dcts_batch_sum_f32(const float* energy_nc, int64_t N, int64_t C_count, float* out_c,
                       void* stream) {
  if (!energy_nc || !out_c) return DCTS_E_NULL;
  if (N <= 0 || C_count <= 0) return DCTS_E_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_batch_sum, dim3((unsigned)((C_count + kSumCh - 1) / kSumCh)), dim3(kSumCh * kSumSl), 0, st,
                     energy_nc, (long long)N, (long long)C_count, out_c);
  return (int)hipGetLastError();
}

int dcts_running_mean_update_f32(const float* energy_nc, int64_t N, int64_t C_count,
                                 float* feature_result, float total_before, void* stream) {
  if (!energy_nc || !feature_result) return DCTS_E_NULL;
  if (N <= 0 || C_count <= 0) return DCTS_E_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_running_mean, dim3((unsigned)((C_count + kSumCh - 1) / kSumCh)), dim3(kSumCh * kSumSl), 0, st,
                     energy_nc, (long long)N, (long long)C_count, feature_result, total_before);
  return (int)hipGetLastError();
}

int dcts_energy_multi_f32(const dcts_tensor_item* items, int32_t count, int64_t H, int64_t W,
                          int32_t pad_front_if_odd, void* workspace, size_t workspace_bytes, void* stream) {
  if (!items) return DCTS_E_NULL;
  if (count <= 0 || H <= 0 || W <= 0) return DCTS_E_SHAPE;
  for (int32_t i = 0; i < count; ++i)
    if (const int rc = validate(view_of(items[i], H, W, pad_front_if_odd), {items[i].out_nc}, Checks::Align)) return rc;
  const TensorView v0 = view_of(items[0], H, W, pad_front_if_odd);
  const int HP = (int)v0.HP(), WP = (int)v0.WP(), pad = v0.pad();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (has_codelet(HP, WP)) {
    const int G = codelet_group_size(HP);
    for (int32_t i0 = 0; i0 < count; i0 += kMultiItems) {
      const int n = (count - i0) < kMultiItems ? (count - i0) : kMultiItems;
      MultiGeom mg;
      long long groups = 0;
      for (int i = 0; i < n; ++i) {
        mg.it[i].g = map_geom(view_of(items[i0 + i], H, W, pad_front_if_odd));
        mg.it[i].out = items[i0 + i].out_nc;
        mg.it[i].group_begin = groups;
        groups += (mg.it[i].g.nmaps + G - 1) / G;
      }
      for (int i = n; i < kMultiItems; ++i) mg.it[i] = mg.it[0];
      mg.total_groups = groups;
      mg.count = n;
      const int rc = dispatch_codelet_multi(HP, pad, mg, st);
      if (rc) return rc;
    }
    return DCTS_OK;
  }
  // large tiles with a single-launch kernel: the dense tensors go into ONE launch per 32 of them (their
  // maps form one index space: a CU that would get a fraction of a map from one small tensor now
  // draws from all of them); results are those of one call per tensor, bit for bit
  TileBatch tb;
  Family fam = Family::Direct;  // of the open batch
  int nb = 0;
  auto flush = [&]() -> int {
    if (!nb) return DCTS_OK;
    for (int i = nb; i < kTileItems; ++i) {
      tb.x[i] = tb.x[0];
      tb.out[i] = tb.out[0];
      tb.begin[i + 1] = tb.begin[nb];
    }
    tb.map_elems = H * W;
    tb.total = tb.begin[nb];
    tb.count = nb;
    nb = 0;
    return traits(fam).batch(HP, tb, st);
  };
  for (int32_t i = 0; i < count; ++i) {
    const TensorView v = view_of(items[i], H, W, pad_front_if_odd);
    // The family the tensor takes on a 16-byte base: one per call, since shape and density decide it. (Kept as found,
    // a tensor on a 4-byte base joins the batch where that family tolerates such a base - at 96 and 112 the fused
    // kernel, where a call of its own takes tile2g.)
    const Choice c = choose(v, DCTS_ALGO_AUTO, /*store=*/false, /*aligned16=*/true);
    if (!c.err && traits(c.fam).batch && (v.aligned16() || !traits(c.fam).base16)) {
      if (nb == 0) tb.begin[0] = 0;
      fam = c.fam;
      tb.x[nb] = v.base();
      tb.out[nb] = items[i].out_nc;
      tb.begin[nb + 1] = tb.begin[nb] + v.nmaps();
      if (++nb == kTileItems) {
        const int rc = flush();
        if (rc) return rc;
      }
      continue;
    }
    // everything else: one call per tensor (split / direct / a family of its own), same stream
    const int rc = run(false, v, items[i].out_nc, workspace, workspace_bytes, stream, DCTS_ALGO_AUTO);
    if (rc) return rc;
  }
  return flush();
}

int dcts_energy_mixed_f32(const dcts_shaped_item* items, int32_t count, void* workspace, size_t workspace_bytes,
                          void* stream) {
  if (!items) return DCTS_E_NULL;
  if (count <= 0) return DCTS_E_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int32_t i = 0; i < count; ++i)
    if (const int rc = validate(view_of(items[i]), {items[i].t.out_nc}, Checks::Align)) return rc;
  auto eligible = [&](const dcts_shaped_item& it) {
    return it.H == it.W && mixed_has((int)it.H) && !(it.pad_front_if_odd && (it.H % 2 != 0));
  };
  // 1. every small-tile tensor, whatever its shape, in one launch per kMixedItems of them
  MixedGeom mg;
  int n = 0;
  long long groups = 0;
  auto flush = [&]() -> int {
    if (!n) return DCTS_OK;
    for (int i = n; i < kMixedItems; ++i) mg.it[i] = mg.it[0];
    mg.total_groups = groups;
    mg.count = n;
    n = 0;
    groups = 0;
    return dispatch_codelet_mixed(mg, st);
  };
  for (int32_t i = 0; i < count; ++i) {
    if (!eligible(items[i])) continue;
    mg.it[n].g = map_geom(view_of(items[i]));
    mg.it[n].out = items[i].t.out_nc;
    mg.it[n].group_begin = groups;
    const int G = 64 / (int)items[i].H;
    groups += (mg.it[n].g.nmaps + G - 1) / G;
    if (++n == kMixedItems) {
      const int rc = flush();
      if (rc) return rc;
    }
  }
  int rc = flush();
  if (rc) return rc;
  // 2. the rest shape by shape (first occurrence order), through dcts_energy_multi_f32
  dcts_tensor_item buf[64];
  for (int32_t i = 0; i < count; ++i) {
    if (eligible(items[i])) continue;
    bool seen = false;
    for (int32_t k = 0; k < i && !seen; ++k)
      seen = !eligible(items[k]) && items[k].H == items[i].H && items[k].W == items[i].W &&
             (items[k].pad_front_if_odd != 0) == (items[i].pad_front_if_odd != 0);
    if (seen) continue;
    int m = 0;
    for (int32_t k = i; k < count; ++k) {
      if (eligible(items[k]) || items[k].H != items[i].H || items[k].W != items[i].W ||
          (items[k].pad_front_if_odd != 0) != (items[i].pad_front_if_odd != 0))
        continue;
      buf[m++] = items[k].t;
      if (m == 64) {
        rc = dcts_energy_multi_f32(buf, m, items[i].H, items[i].W, items[i].pad_front_if_odd, workspace, workspace_bytes, stream);
        if (rc) return rc;
        m = 0;
      }
    }
    if (m) {
      rc = dcts_energy_multi_f32(buf, m, items[i].H, items[i].W, items[i].pad_front_if_odd, workspace, workspace_bytes, stream);
      if (rc) return rc;
    }
  }
  return DCTS_OK;
}

int dcts_running_mean_update_multi_f32(const dcts_update_desc* descs, int32_t count, void* stream) {
  if (!descs) return DCTS_E_NULL;
  if (count <= 0) return DCTS_E_SHAPE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int32_t i0 = 0; i0 < count; i0 += kMultiMax) {
    const int n = (count - i0) < kMultiMax ? (count - i0) : kMultiMax;
    UpdateBatch b;
    int64_t cmax = 0;
    for (int i = 0; i < n; ++i) {
      b.d[i] = descs[i0 + i];
      if (!b.d[i].energy_nc || !b.d[i].feature_result) return DCTS_E_NULL;
      if (b.d[i].N <= 0 || b.d[i].C_count <= 0) return DCTS_E_SHAPE;
      if (b.d[i].C_count > cmax) cmax = b.d[i].C_count;
    }
    for (int i = n; i < kMultiMax; ++i) b.d[i] = b.d[0];
    hipLaunchKernelGGL(k_running_mean_multi, dim3((unsigned)((cmax + kSumCh - 1) / kSumCh), (unsigned)n),
                       dim3(kSumCh * kSumSl), 0, st, b);
  }
  return (int)hipGetLastError();
}

#ifdef DCTS_FUSED_STAMPS
int dcts_debug_fused_stamps(unsigned long long* host_out /*[16][16]*/, int reset) {
  if (reset) {
    static unsigned long long zeros[16][16] = {};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fused_stamps), zeros, sizeof(zeros));
  }
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fused_stamps), 16 * 16 * sizeof(unsigned long long));
}
#endif

int dcts_debug_stream_read_f32(const float* x, int64_t n, float* sink, void* stream) {
  if (!x || !sink) return DCTS_E_NULL;
  if (n <= 0) return DCTS_E_SHAPE;
  hipLaunchKernelGGL(k_calib_read, dim3(256 * 32), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     (long long)n, sink);
  return (int)hipGetLastError();
}

}  // extern "C"
