// dcts_internal.h - what the translation units of libdctscore.so know of each other: the descriptor structs the kernels
// take by value, the dispatchers of every kernel family (each defined in its family's unit), and the host-side shape
// predicates and workspace sizes the C ABI (api.hip) needs without any kernel body.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "codelet_sizes.h"

struct dcts_update_desc;  // include/dctscore.h

namespace dctsi {

struct MapGeom {
  const float* x;
  long long nmaps;    // N * c_count
  long long strideN;  // elements
  long long strideC;  // elements
  long long strideH;  // elements (direct kernel only; codelet kernels require == W)
  int c_count;
  int c_begin;
  int H, W;           // data dims (before the odd front pad)
  int contiguous;     // 1: map m starts at x + c_begin*strideC + m*strideC (no div needed)
};

// first element of map m of the scored channel slice; Geom is MapGeom or HalfGeom (below)
template <class Geom>
__device__ __forceinline__ auto map_base(const Geom& g, long long m) -> decltype(g.x) {
  if (g.contiguous) return g.x + (long long)g.c_begin * g.strideC + m * g.strideC;
  const long long n = m / g.c_count;
  const long long j = m - n * g.c_count;
  return g.x + n * g.strideN + (g.c_begin + j) * g.strideC;
}

// Several hooked tensors of the same tile shape in ONE launch (single-sweep harness, bench): the
// groups of all tensors form one index space; a wave walks it with a grid stride and tracks which
// tensor its current group belongs to. CIFAR-sized layers are 5-20 us kernels when launched one
// by one - the launch ramp and tail cost more than the work.
constexpr int kMultiItems = 32;
struct MultiItem {
  MapGeom g;
  float* out;
  long long group_begin;  // first global group index of this tensor
};
struct MultiGeom {
  MultiItem it[kMultiItems];
  long long total_groups;
  int count;
};

// Tensors of DIFFERENT small tile shapes in one launch (k_energy_codelet_mixed, codelet.hip)
constexpr int kMixedItems = 48;
struct MixedGeom {
  MultiItem it[kMixedItems];
  long long total_groups;
  int count;
};
#define DCTS_MIXED_SIZES(X) X(2) X(4) X(8) X(16) X(32)
constexpr bool mixed_has(int e) {
#define DCTS_CASE(N) \
  if (e == N) return true;
  DCTS_MIXED_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

// Dense tensors of one large tile shape as ONE map index space (fused / pipelined kernels): map m of
// the batch is map m - begin[t] of tensor t. U2-Net-p hooks ten 288x288 tensors of 16 or 64 channels;
// launched one by one at batch 12 they give a CU 0.75 or 3 maps each, together 16.5.
constexpr int kTileItems = 32;
struct TileBatch {
  const float* x[kTileItems];
  float* out[kTileItems];
  long long begin[kTileItems + 1];  // begin[count] = total
  long long map_elems;              // floats per map (dense: maps of a tensor are adjacent)
  long long total;
  int count;
};

// one dense tensor of `nmaps` maps as a batch of one (every slot names it: a lookup never leaves the tensor)
inline TileBatch single_tensor_batch(const float* x, float* out, long long nmaps, long long map_elems) {
  TileBatch tb;
  for (int i = 0; i < kTileItems; ++i) {
    tb.x[i] = x;
    tb.out[i] = out;
    tb.begin[i] = 0;
  }
  tb.begin[1] = tb.begin[kTileItems] = nmaps;
  tb.map_elems = map_elems;
  tb.total = nmaps;
  tb.count = 1;
  return tb;
}

// compute units of the current device, queried once (256 on MI355X; the persistent grids are sized by it)
inline int num_cus() {
  static const int n = [] {
    int dev = 0, cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu < 1)
      cu = 256;
    return cu;
  }();
  return n;
}

// workgroups of `kernel` (WAVES waves, static LDS only) that fit a CU, queried once: the persistent grids of the codelet and
// the role-wave families are one residency
template <auto kernel, int WAVES>
int blocks_per_cu() {
  static const int per_cu = [] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 64 * WAVES, 0) != hipSuccess || n < 1) n = 1;
    return n;
  }();
  return per_cu;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- which shapes a family serves (from the tables of codelet_sizes.h) -----------------------------------------
inline bool has_codelet(long long HP, long long WP) {
  if (HP != WP) return false;
#define DCTS_CASE(N) \
  if (HP == N) return true;
  DCTS_CODELET_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

constexpr bool has_lane_kernel(int n) { return n == 7 || n == 9; }

inline bool has_split(long long HP, long long WP) {
  if (HP != WP) return false;
#define DCTS_CASE(N_, M_, L_) \
  if (HP == N_) return true;
  DCTS_SPLIT_TABLE(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

inline bool has_fused(long long N) {
#define DCTS_CASE(N_, M_, L_) \
  if (N == N_) return true;
  DCTS_FUSED_TABLE(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

inline bool has_fused2(long long N) {
#define DCTS_CASE(N_, M_, L_) \
  if (N == N_) return true;
  DCTS_FUSED2_TABLE(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

inline bool has_pipe(long long N) {
#define DCTS_CASE(N_, M_, L_) \
  if (N == N_) return true;
  DCTS_PIPE_TABLE(DCTS_CASE)
#undef DCTS_CASE
  return false;
}

// ---- codelet.hip: square tiles with both edges <= 64 ------------------------------------------------------------
int codelet_group_size(int HP);  // maps per wave and iteration of the kernel that serves edge HP
int dispatch_codelet(int store, int HP, int WP, int pad, const MapGeom& g, float* out, hipStream_t st);
int dispatch_codelet_dma(int N, const MapGeom& g, float* out, hipStream_t st);
int dispatch_codelet_multi(int HP, int pad, const MultiGeom& mg, hipStream_t st);
int dispatch_lane(int n, const MultiGeom& mg, hipStream_t st);
int dispatch_codelet_mixed(const MixedGeom& mg, hipStream_t st);

// ---- direct.hip: the cosine-matrix kernel, any (H, W) <= DCTS_MAX_EDGE, energies or coefficients -------------------------
// its workspace: [basis table of HP][basis table of WP][one HP x WP intermediate tile per workgroup of the grid]
struct DirectWs {
  size_t off_ch, off_cw, off_t, total;
  int grid;
};
DirectWs direct_ws(long long nmaps, int HP, int WP);
// both tables; the status of the two launches (api.hip's memo remembers tables only after a success)
int launch_basis(float* CHt, int HP, float* CWt, int WP, hipStream_t st);
int dispatch_direct(int store, int pad, const MapGeom& g, int grid, const float* CHt, const float* CWt, float* T, float* out,
                    hipStream_t st);

// ---- reduce.hip: what follows the energies (batch sum, running mean), the weighted reduction, the calibration read -------
int launch_batch_sum(const float* e, long long N, long long C, float* out_c, hipStream_t st);
int launch_running_mean(const float* e, long long N, long long C, float* fr, float total, hipStream_t st);
// n <= kMultiMax hook points in one launch; cmax: the largest C_count among them
constexpr int kMultiMax = 64;
int launch_running_mean_multi(const dcts_update_desc* descs, int n, long long cmax, hipStream_t st);
// out[m] = sum_i weights[i] * coeff[m][i]^2 over `nmaps` dense tiles of `hw` coefficients
int launch_weighted_reduce(const float* coeff, const float* weights, long long nmaps, int hw, float* out, hipStream_t st);
int launch_stream_read(const float* x, long long n, float* sink, hipStream_t st);

// ---- band.hip: K weighted energies per map (dcts_band_energy_f32) ------------------------------------------------
int band_kb(int K);                                // K rounded up to 1, 2, 4, 8: the fused kernel's accumulator count
size_t band_table_bytes(int HP, int WP, int K);    // the re-laid weight table T[l][u][KB] at the head of the workspace
// fused kernel for square tiles with a codelet (HP after the odd pad): builds the table from `weights`, then one launch
int dispatch_band(int HP, int pad, const MapGeom& g, const float* weights, int K, float* table, float* out, hipStream_t st);
// fallback reduction: out[m][b] = sum_i weights[b][i] * coeff[m][i]^2 over `nmaps` dense tiles of `hw` coefficients
int launch_band_reduce(const float* coeff, const float* weights, long long nmaps, int hw, int K, float* out, hipStream_t st);

// ---- entropy.hip: the spectral entropy of every map (dcts_spectral_entropy_f32) ---------------------------------------
// fused kernel for square tiles with a codelet (HP after the odd pad), dense rows: one launch, no workspace
int dispatch_entropy(int HP, int pad, const MapGeom& g, float* out, hipStream_t st);
// fallback reduction: out[m] = entropy of the squares of `nmaps` dense tiles of `hw` coefficients (any common scale)
int launch_entropy_reduce(const float* coeff, long long nmaps, int hw, float* out, hipStream_t st);

// ---- lowpass.hip: the K x K lowest DCT coefficients of every map (dcts_dct2d_lowpass_f32) -----------------------------
// fused kernel for dense square unpadded tiles with a codelet: one launch, no workspace; out is [nmaps][k][k], k = min(K, HP).
// drop_dc: [0][0] is written as +0.0 and a map whose elements are all equal gets an all-+0.0 signature.
int dispatch_lowpass(int HP, const MapGeom& g, int K, int drop_dc, float* out, hipStream_t st);
// fallback "reduction": the [Kh][Kw] corner of `nmaps` dense [g.H][g.W] tiles of coefficients to out[first + m]; g is the call's
// whole view, whose map first + m is the spatial map of tile m (read for the flat rule of drop_dc only)
int launch_lowpass_gather(const float* coeff, long long nmaps, long long first, const MapGeom& g, int Kh, int Kw, int drop_dc,
                          float* out, hipStream_t st);

// ---- gm.hip: summed distance of every scored map to the maps of a reference set (dcts_gm_distance_f32) -----------------
// Dense maps of hw = H * W elements; the scored channels [c_begin, c_begin + c_count) and the reference channels
// [r_begin, r_begin + r_count) of every sample. One launch, no workspace.
struct GmGeom {
  const float* x;
  long long N;
  long long strideN, strideC;  // elements
  int c_begin, c_count;
  int r_begin, r_count;
  int hw;
};
int dispatch_gm(const GmGeom& g, float* out, hipStream_t st);
// The normalised metrics (dcts_gm_distance_metric_f32): the same sum over the unit maps (x - mu) * s. One (mu, s) pair per map
// of the scored range at sa ([N][c_count]) and of the reference range at sb ([N][r_count]), each gm_stats_bytes() long, written
// by a launch of their own in front of the distance kernel. center: mu is the map's mean (correlation), else 0 (cosine).
inline size_t gm_stats_bytes(long long N, int count) { return align_up((size_t)N * (size_t)count * sizeof(float2), 256); }
int dispatch_gm_metric(const GmGeom& g, bool center, float2* sa, float2* sb, float* out, hipStream_t st);
int launch_gm_stats(const GmGeom& g, bool center, int begin, int count, float2* pairs, hipStream_t st);  // one range's pairs

// ---- gm_pairs.hip: every distance between a scored and a reference map, summed over the samples (dcts_gm_pairs_f32) --------
// out: [c_count][r_count]. The samples are cut into gm_pair_slices(N, r_count) slices (grid_caps.h); with more than one, the
// slices' matrices go to `partials`, gm_pair_partial_bytes() long, and a second launch adds them. center: -1 for the plain
// distance, else 0 (cosine) / 1 (correlation) with sa / sb as for dispatch_gm_metric.
inline size_t gm_pair_partial_bytes(int slices, int c_count, int r_count) {
  return slices > 1 ? align_up((size_t)slices * (size_t)c_count * (size_t)r_count * sizeof(float), 256) : 0;
}
int dispatch_gm_pairs(const GmGeom& g, int center, float2* sa, float2* sb, float* partials, float* out, hipStream_t st);

// ---- half.hip: fp16 / bf16 inputs (dcts_energy_typed) -------------------------------------------------------------
// MapGeom for 2-byte elements (raw bits; the dtype travels beside it). Rows are dense: strideH == W.
struct HalfGeom {
  const uint16_t* x;
  long long nmaps;    // N * c_count
  long long strideN;  // elements
  long long strideC;  // elements
  int c_count;
  int c_begin;
  int contiguous;     // 1: map m starts at x + c_begin*strideC + m*strideC
};
// dense square edges with a native half kernel: what the six classification nets hook
#define DCTS_HALF_SIZES(X) X(2) X(4) X(7) X(8) X(14) X(16) X(28) X(32) X(56)
inline bool has_half(long long H, long long W) {
  if (H != W) return false;
#define DCTS_CASE(N) \
  if (H == N) return true;
  DCTS_HALF_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return false;
}
int dispatch_half(int N, int dtype, const HalfGeom& g, float* out, hipStream_t st);
// the staged route: the g.nmaps maps of g (H x W, row pitch strideH elements) as a dense fp32 array at dst
int launch_upcast_half(int dtype, const HalfGeom& g, int H, int W, long long strideH, float* dst, hipStream_t st);

// ---- nhwc.hip: channels-last maps of fp32 / fp16 / bf16 elements (dcts_energy_nhwc) ---------------------------------
// element (n, c, h, w) of the scored slice is x[n*strideN + h*strideH + w*strideW + c_begin + c] (elements of the dtype that
// travels beside the descriptor): the channel stride is 1
struct NhwcGeom {
  const void* x;
  long long N;
  long long strideN, strideH, strideW;  // elements
  int c_begin;
  int c_count;
};
// dense square edges with a native channels-last kernel (no odd pad)
#define DCTS_NHWC_LANE_SIZES(X) X(2) X(4) X(7) X(8)        /* lane = channel, the map in registers */
#define DCTS_NHWC_BLOCK_SIZES(X) X(14) X(16) X(28) X(32)   /* a channel block of whole maps through LDS */
inline bool has_nhwc(long long H, long long W) {
  if (H != W) return false;
#define DCTS_CASE(N) \
  if (H == N) return true;
  DCTS_NHWC_LANE_SIZES(DCTS_CASE)
  DCTS_NHWC_BLOCK_SIZES(DCTS_CASE)
#undef DCTS_CASE
  return H == 56;  // strips of rows through LDS
}
int dispatch_nhwc(int N, int dtype, const NhwcGeom& g, float* out, hipStream_t st);

// ---- split.hip, split_more.hip: two launches per chunk of maps, intermediate in the workspace ------------------
struct SplitWs {
  long long chunk_maps;
  size_t off_t, off_part, total;
};
int split_partials_per_map(int N);
SplitWs split_ws(long long nmaps, int N);
int dispatch_split(int N, const MapGeom& g, float* out, void* workspace, hipStream_t st);
int dispatch_split_more(int N, const MapGeom& g, float* out, void* workspace, hipStream_t st);  // the 8 * M entries added in round 3

// ---- single-launch large-tile kernels: fused.hip, fused2.hip, pipe.hip, tile2d.hip, tile2g.hip -----------------
int dispatch_fused(int N, const TileBatch& tb, hipStream_t st);
int dispatch_fused2(int N, const TileBatch& tb, hipStream_t st);
int dispatch_pipe(int N, const TileBatch& tb, hipStream_t st);
int dispatch_tile2d(int N, const TileBatch& tb, hipStream_t st);
// tile2g.hip: mid-size edges as a 2-D radix split with several maps per round
int has_tile2g(int N);
int has_tile2g_pad(int N);
int dispatch_tile2g(int N, const TileBatch& tb, hipStream_t st);
int dispatch_tile2g_pad(int N, const TileBatch& tb, hipStream_t st);  // tiles with the odd front pad (N = H + 1)
// coefficient output through the large-tile kernels (debug / parity): leaf outputs into `scratch`
// (scratch_maps tiles), then k_assemble
int dispatch_fused_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, hipStream_t st);
int dispatch_fused2_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, hipStream_t st);
int dispatch_tile2d_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, hipStream_t st);
int dispatch_tile2g_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, hipStream_t st);

}  // namespace dctsi
