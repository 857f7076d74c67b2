// Stream trace: which stream every dispatcher call of every C-ABI entry point carries - without a GPU.
//
// `make -C dct_pruning_amd/csrc streams` compiles api.hip once more with every dispatcher that takes a hipStream_t
// redirected on the compiler command line (-Ddispatch_gm=strm_dispatch_gm ...) to the recorders below, and links that
// object with the ordinary kernel objects and this driver, as the dispatch trace (dispatch_trace.cpp) is built. A recorder
// writes its own name and the stream it received, nothing else: what the arguments are is the dispatch trace's business.
// The driver calls every entry point of include/dctscore.h that api.hip defines with a stream parameter, over shapes that
// reach every route api.hip has for it, once with each of two fake non-null stream tokens (never dereferenced: nothing is
// launched), and prints one line per call:
//
//   call <entry point> <case> <token given> rc=<return code> | <dispatcher>@<token received> ...
//
// then the basis-table memo of one workspace over the token sequence S1 S1 S2 S2 S1. tests/test_streams_cpu.py reads the
// lines. The process refuses to start unless the GPU is hidden, so a dispatcher that was NOT redirected fails its launch
// (a positive return code on the line) and never runs on a fake pointer. (dcts_rank_f32 is defined in rank.hip beside its
// kernel and launches there: no dispatcher of api.hip carries its stream, the GPU tests of tests/test_streams_gpu.py do.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../dct_pruning_amd/csrc/dcts_internal.h"
#include "../../dct_pruning_amd/csrc/rect.h"
#include "../../include/dctscore.h"

namespace {

// fake "device" addresses: validation, descriptor packing and the memo only do arithmetic on them
float* const X = reinterpret_cast<float*>(0x100000000000ull);
float* const OUT = reinterpret_cast<float*>(0x200000000000ull);
char* const WS = reinterpret_cast<char*>(0x300000000000ull);
float* const WT = reinterpret_cast<float*>(0x400000000000ull);
char* const WS_MEMO = reinterpret_cast<char*>(0x500000000000ull);
constexpr size_t kBig = size_t(1) << 32;  // a workspace that holds any call here whole
// the two stream tokens
void* const S1 = reinterpret_cast<void*>(0x51000ull);
void* const S2 = reinterpret_cast<void*>(0x52000ull);

std::string g_records;

const char* token(const void* st) { return st == S1 ? "S1" : st == S2 ? "S2" : st ? "other" : "null"; }

int rec(const char* name, hipStream_t st) {
  g_records += " ";
  g_records += name;
  g_records += "@";
  g_records += token(st);
  return 0;
}

void finish(const char* entry, const char* tag, void* given, int rc) {
  std::printf("call %s %s %s rc=%d |%s\n", entry, tag, token(given), rc, g_records.c_str());
  g_records.clear();
}

}  // namespace

// ---- the recorders: same signatures as the dispatchers of dcts_internal.h / rect.h -----------------------------------
namespace dctsi {

#define REC(NAME, ...) \
  int strm_##NAME(__VA_ARGS__, hipStream_t st) { return rec(#NAME, st); }
REC(dispatch_codelet, int, int, int, int, const MapGeom&, float*)
REC(dispatch_codelet_dma, int, const MapGeom&, float*)
REC(dispatch_codelet_multi, int, int, const MultiGeom&)
REC(dispatch_lane, int, const MultiGeom&)
REC(dispatch_codelet_mixed, const MixedGeom&)
REC(dispatch_rect, const RectGeom&, float*, int)
REC(dispatch_split, int, const MapGeom&, float*, void*)
REC(dispatch_fused, int, const TileBatch&)
REC(dispatch_fused2, int, const TileBatch&)
REC(dispatch_pipe, int, const TileBatch&)
REC(dispatch_tile2d, int, const TileBatch&)
REC(dispatch_tile2g, int, const TileBatch&)
REC(dispatch_tile2g_pad, int, const TileBatch&)
REC(dispatch_fused_coeff, int, const float*, long long, float*, float*, long long)
REC(dispatch_fused2_coeff, int, const float*, long long, float*, float*, long long)
REC(dispatch_tile2d_coeff, int, const float*, long long, float*, float*, long long)
REC(dispatch_tile2g_coeff, int, const float*, long long, float*, float*, long long)
REC(dispatch_band, int, int, const MapGeom&, const float*, int, float*, float*)
REC(launch_band_reduce, const float*, const float*, long long, int, int, float*)
REC(dispatch_entropy, int, int, const MapGeom&, float*)
REC(launch_entropy_reduce, const float*, long long, int, float*)
REC(dispatch_lowpass, int, const MapGeom&, int, int, float*)
REC(launch_lowpass_gather, const float*, long long, long long, const MapGeom&, int, int, int, float*)
REC(dispatch_gm, const GmGeom&, float*)
REC(dispatch_gm_metric, const GmGeom&, bool, float2*, float2*, float*)
REC(dispatch_gm_pairs, const GmGeom&, int, float2*, float2*, float*, float*)
REC(dispatch_half, int, int, const HalfGeom&, float*)
REC(launch_upcast_half, int, const HalfGeom&, int, int, long long, float*)
REC(dispatch_nhwc, int, int, const NhwcGeom&, float*)
REC(launch_basis, float*, int, float*, int)
REC(dispatch_direct, int, int, const MapGeom&, int, const float*, const float*, float*, float*)
REC(launch_weighted_reduce, const float*, const float*, long long, int, float*)
REC(launch_batch_sum, const float*, long long, long long, float*)
REC(launch_running_mean, const float*, long long, long long, float*, float)
REC(launch_running_mean_multi, const dcts_update_desc*, int, long long)
REC(launch_stream_read, const float*, long long, float*)
#undef REC

}  // namespace dctsi

namespace {

// one dense [N, C, H, W] fp32 tensor (or of 2-byte elements: the strides count elements either way)
struct T {
  int64_t N, C, H, W;
  int64_t sH() const { return W; }
  int64_t sC() const { return H * W; }
  int64_t sN() const { return C * H * W; }
};

// the band / entropy / low-pass fallback's workspace for `chunk` maps per chunk (api.hip: coeff_layout)
size_t coeff_bytes(int HP, int WP, long long chunk) {
  return dctsi::direct_ws(1, HP, WP).off_t + 512 + 2 * (size_t)chunk * HP * WP * 4;
}

void energy(void* st) {
  struct { const char* tag; int64_t H, W; int pad, algo; } cases[] = {
      {"codelet8", 8, 8, 0, DCTS_ALGO_AUTO},      {"codelet56", 56, 56, 0, DCTS_ALGO_AUTO},
      {"codelet7pad", 7, 7, 1, DCTS_ALGO_AUTO},   {"prefetch16", 16, 16, 0, DCTS_ALGO_PREFETCH},
      {"lane7", 7, 7, 0, DCTS_ALGO_AUTO},         {"rect28x14", 28, 14, 0, DCTS_ALGO_AUTO},
      {"rect8", 8, 8, 0, DCTS_ALGO_RECT},         {"rect13", 13, 13, 0, DCTS_ALGO_AUTO},
      {"direct13", 13, 13, 0, DCTS_ALGO_DIRECT},  {"direct13again", 13, 13, 0, DCTS_ALGO_DIRECT},
      {"direct67", 67, 67, 0, DCTS_ALGO_AUTO},    {"direct67again", 67, 67, 0, DCTS_ALGO_AUTO},
      {"split88", 88, 88, 0, DCTS_ALGO_AUTO},     {"split96", 96, 96, 0, DCTS_ALGO_SPLIT},
      {"fused96", 96, 96, 0, DCTS_ALGO_AUTO},     {"fused2_288", 288, 288, 0, DCTS_ALGO_AUTO},
      {"pipe128", 128, 128, 0, DCTS_ALGO_AUTO},   {"tile2d224", 224, 224, 0, DCTS_ALGO_AUTO},
      {"tile2g72", 72, 72, 0, DCTS_ALGO_AUTO},    {"tile2gpad71", 71, 71, 1, DCTS_ALGO_AUTO},
      {"tile2g96", 96, 96, 0, DCTS_ALGO_TILE2D},  {"fused128", 128, 128, 0, DCTS_ALGO_FUSED},
  };
  for (const auto& c : cases) {
    const T t{2, 5, c.H, c.W};
    finish("dcts_energy_f32_ex", c.tag, st,
           dcts_energy_f32_ex(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, c.pad, OUT, WS, kBig, st, c.algo));
    if (c.algo == DCTS_ALGO_AUTO)
      finish("dcts_energy_f32", c.tag, st,
             dcts_energy_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, c.pad, OUT, WS, kBig, st));
  }
}

void coefficients(void* st) {
  struct { const char* tag; int64_t H; int algo; size_t ws_bytes; } cases[] = {
      {"codelet8", 8, DCTS_ALGO_AUTO, kBig},          {"direct13", 13, DCTS_ALGO_DIRECT, kBig},
      {"direct96", 96, DCTS_ALGO_AUTO, kBig},         {"fused96", 96, DCTS_ALGO_FUSED, kBig},
      {"fused2_288", 288, DCTS_ALGO_FUSED, kBig},     {"tile2d224", 224, DCTS_ALGO_TILE2D, kBig},
      {"tile2g72", 72, DCTS_ALGO_TILE2D, kBig},       {"tile2g72_3maps", 72, DCTS_ALGO_TILE2D, size_t(3) * 72 * 72 * 4},
      {"rect8", 8, DCTS_ALGO_RECT, kBig},
  };
  for (const auto& c : cases) {
    const T t{2, 5, c.H, c.H};
    finish("dcts_dct2d_f32_ex", c.tag, st,
           dcts_dct2d_f32_ex(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, OUT, WS, c.ws_bytes, st, c.algo));
    if (c.algo == DCTS_ALGO_AUTO)
      finish("dcts_dct2d_f32", c.tag, st,
             dcts_dct2d_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, OUT, WS, kBig, st));
  }
}

// weighted: always one-sample inner calls; a small workspace cuts a sample into runs of channels as well
void weighted(void* st) {
  struct { const char* tag; int64_t H, W; long long chunk; } cases[] = {
      {"codelet8", 8, 8, 0}, {"direct67", 67, 67, 0}, {"rect13x17_runs", 13, 17, 2}, {"tile2g72", 72, 72, 0},
      {"tile2g72_runs", 72, 72, 2}, {"fused96", 96, 96, 0}, {"tile2d224", 224, 224, 0}, {"fused2_288", 288, 288, 0},
  };
  for (const auto& c : cases) {
    const T t{3, 5, c.H, c.W};
    size_t bytes = kBig;
    if (c.chunk) bytes = 2 * dctsi::align_up((size_t)c.chunk * c.H * c.W * 4, 256) + dcts_workspace_bytes(1, 1, c.H, c.W) + 4096;
    finish("dcts_weighted_energy_f32", c.tag, st,
           dcts_weighted_energy_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, WT, OUT, WS, bytes, st));
  }
}

// band, entropy, low-pass: the fused kernel, and the coefficient fallback in both regimes of its chunk loop (whole samples
// per chunk; runs of channels of one sample), over the inner coefficient paths (direct, rect, large-tile + k_assemble)
void per_map_statistics(void* st) {
  struct { const char* tag; int64_t H, W; int algo; long long chunk; } cases[] = {
      {"fused14", 14, 14, DCTS_ALGO_AUTO, 0},          {"fallback14_direct", 14, 14, DCTS_ALGO_DIRECT, 0},
      {"fallback72_samples", 72, 72, DCTS_ALGO_AUTO, 0}, {"fallback72_runs", 72, 72, DCTS_ALGO_AUTO, 2},
      {"fallback13x17_samples", 13, 17, DCTS_ALGO_AUTO, 0}, {"fallback13x17_runs", 13, 17, DCTS_ALGO_AUTO, 2},
      {"fallback67_samples", 67, 67, DCTS_ALGO_AUTO, 5}, {"fallback96_runs", 96, 96, DCTS_ALGO_AUTO, 3},
      {"fallback224_samples", 224, 224, DCTS_ALGO_AUTO, 0}, {"fallback288_runs", 288, 288, DCTS_ALGO_AUTO, 1},
  };
  for (const auto& c : cases) {
    const T t{3, 5, c.H, c.W};
    const size_t bytes = c.chunk ? coeff_bytes((int)c.H, (int)c.W, c.chunk) : kBig;
    finish("dcts_band_energy_f32", c.tag, st,
           dcts_band_energy_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, WT, 3, OUT, WS, bytes, st, c.algo));
    finish("dcts_spectral_entropy_f32", c.tag, st,
           dcts_spectral_entropy_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, OUT, WS, bytes, st, c.algo));
    if (c.algo != DCTS_ALGO_AUTO) continue;  // the low-pass entry point takes no algo
    for (int flags : {0, DCTS_LOWPASS_DROP_DC})
      finish("dcts_dct2d_lowpass_f32", flags ? (std::string(c.tag) + "_dropdc").c_str() : c.tag, st,
             dcts_dct2d_lowpass_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 4, flags, OUT, WS, bytes, st));
  }
  const T t{3, 5, 56, 56};
  finish("dcts_dct2d_lowpass_f32", "fused56", st,
         dcts_dct2d_lowpass_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 8, 0, OUT, WS, kBig, st));
  // a row pitch sends a codelet edge to the fallback, whose inner calls take the run-time codelet pair
  finish("dcts_dct2d_lowpass_f32", "fallback14_pitched", st,
         dcts_dct2d_lowpass_f32(X, 3, 5, 14, 14, 5 * 14 * 18, 14 * 18, 18, 1, 0, 5, 4, 0, OUT, WS, kBig, st));
  finish("dcts_band_energy_f32", "fused14_pitched", st,
         dcts_band_energy_f32(X, 3, 5, 14, 14, 5 * 14 * 18, 14 * 18, 18, 1, 0, 5, 0, WT, 3, OUT, WS, kBig, st, DCTS_ALGO_AUTO));
}

void gm(void* st) {
  const T t{2, 12, 7, 7};
  finish("dcts_gm_distance_f32", "l2", st, dcts_gm_distance_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, 12, 0, 12, OUT, st));
  const struct { const char* tag; int metric; } metrics[] = {{"l2", DCTS_GM_L2}, {"cosine", DCTS_GM_COSINE}, {"correlation", DCTS_GM_CORRELATION}};
  for (const auto& m : metrics) {
    finish("dcts_gm_distance_metric_f32", m.tag, st,
           dcts_gm_distance_metric_f32(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, 12, 0, 12, OUT, st, m.metric, WS, kBig));
    for (int64_t N : {int64_t(2), int64_t(64)})  // one slice, several slices
      finish("dcts_gm_pairs_f32", (std::string(m.tag) + (N == 2 ? "_n2" : "_n64")).c_str(), st,
             dcts_gm_pairs_f32(X, N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, 12, 0, 12, OUT, st, m.metric, WS, kBig));
  }
}

void typed(void* st) {
  const struct { const char* tag; int dtype; int64_t H, W; long long chunk; } cases[] = {
      {"f32_14", DCTS_DTYPE_F32, 14, 14, 0},       {"f16_native14", DCTS_DTYPE_F16, 14, 14, 0},
      {"bf16_native56", DCTS_DTYPE_BF16, 56, 56, 0}, {"f16_staged20", DCTS_DTYPE_F16, 20, 20, 0},
      {"bf16_staged20_runs", DCTS_DTYPE_BF16, 20, 20, 2}, {"f16_staged13_samples", DCTS_DTYPE_F16, 13, 13, 7},
      {"bf16_staged13_runs", DCTS_DTYPE_BF16, 13, 13, 2}, {"f16_staged72", DCTS_DTYPE_F16, 72, 72, 0},
      {"f16_staged88_runs", DCTS_DTYPE_F16, 88, 88, 3}, {"bf16_staged28x14", DCTS_DTYPE_BF16, 28, 14, 0},
      {"f16_staged67", DCTS_DTYPE_F16, 67, 67, 0}, {"bf16_staged67_runs", DCTS_DTYPE_BF16, 67, 67, 2},
  };
  for (const auto& c : cases) {
    const T t{3, 5, c.H, c.W};
    size_t bytes = kBig;
    if (c.chunk) bytes = dctsi::align_up(dcts_workspace_bytes(t.N, t.C, t.H, t.W), 256) + (size_t)c.chunk * c.H * c.W * 4;
    finish("dcts_energy_typed", c.tag, st,
           dcts_energy_typed(X, c.dtype, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, OUT, WS, bytes, st));
  }
  const struct { const char* tag; int dtype; int64_t H; } nhwc[] = {
      {"f32_lane8", DCTS_DTYPE_F32, 8},   {"bf16_lane8", DCTS_DTYPE_BF16, 8},    {"f32_block14", DCTS_DTYPE_F32, 14},
      {"f16_block14", DCTS_DTYPE_F16, 14}, {"f32_strip56", DCTS_DTYPE_F32, 56}, {"bf16_strip56", DCTS_DTYPE_BF16, 56},
  };
  for (const auto& c : nhwc)
    finish("dcts_energy_nhwc", c.tag, st,
           dcts_energy_nhwc(X, c.dtype, 2, 5, c.H, c.H, c.H * c.H * 5, c.H * 5, 5, 0, 5, OUT, nullptr, 0, st));
}

void reductions(void* st) {
  finish("dcts_batch_sum_f32", "n4c5", st, dcts_batch_sum_f32(X, 4, 5, OUT, st));
  finish("dcts_running_mean_update_f32", "n4c5", st, dcts_running_mean_update_f32(X, 4, 5, OUT, 8.f, st));
  std::vector<dcts_update_desc> descs(150);  // more than twice kMultiMax: three launches
  for (size_t i = 0; i < descs.size(); ++i) descs[i] = dcts_update_desc{X + 64 * i, OUT + 16 * i, 4, (int64_t)(3 + i % 5), 8.f, 0};
  finish("dcts_running_mean_update_multi_f32", "150descs", st, dcts_running_mean_update_multi_f32(descs.data(), (int32_t)descs.size(), st));
  finish("dcts_running_mean_update_multi_f32", "1desc", st, dcts_running_mean_update_multi_f32(descs.data(), 1, st));
  finish("dcts_debug_stream_read_f32", "n1000", st, dcts_debug_stream_read_f32(X, 1000, OUT, st));
}

dcts_tensor_item item(int i, const T& t) {
  return dcts_tensor_item{X + (int64_t)i * t.N * t.sN(), OUT + (int64_t)i * t.N * t.C, t.N, t.C, t.sN(), t.sC(), 0, (int32_t)t.C};
}

// lists long enough to be cut: more than kMultiItems / kTileItems (32), kMixedItems (48) and the 64 of the mixed call's buffer
void lists(void* st) {
  const struct { const char* tag; int64_t H, W; int count, pad; } multi[] = {
      {"codelet14x40", 14, 14, 40, 0}, {"codelet7x3", 7, 7, 3, 0}, {"codelet7padx3", 7, 7, 3, 1}, {"tile2g72x3", 72, 72, 3, 0},
      {"tile2g72x70", 72, 72, 70, 0},  {"fused96x33", 96, 96, 33, 0}, {"tile2d224x2", 224, 224, 2, 0}, {"rect28x14x3", 28, 14, 3, 0},
      {"direct67x3", 67, 67, 3, 0},    {"split88x2", 88, 88, 2, 0},  {"tile2gpad71x2", 71, 71, 2, 1},
  };
  for (const auto& c : multi) {
    const T t{2, 5, c.H, c.W};
    std::vector<dcts_tensor_item> items;
    for (int i = 0; i < c.count; ++i) items.push_back(item(i, t));
    finish("dcts_energy_multi_f32", c.tag, st, dcts_energy_multi_f32(items.data(), c.count, c.H, c.W, c.pad, WS, kBig, st));
  }
  // a 128 x 128 tensor on a 4-byte base among aligned ones: a call of its own (the pipelined kernel stages 16 bytes a lane)
  {
    const T t{2, 5, 128, 128};
    std::vector<dcts_tensor_item> items;
    for (int i = 0; i < 5; ++i) items.push_back(item(i, t));
    items[2].x += 1;
    finish("dcts_energy_multi_f32", "pipe128_unaligned_between", st, dcts_energy_multi_f32(items.data(), 5, 128, 128, 0, WS, kBig, st));
  }
  // mixed: 100 small tiles (three launches of at most 48), 70 tensors of 14 x 14 (the 64-item buffer, then chunks of 32), the
  // CIFAR edges, an odd edge with the pad flag, a direct and a large-tile shape
  std::vector<dcts_shaped_item> items;
  int k = 0;
  auto add = [&](int64_t e, int pad) {
    const T t{2, 5, e, e};
    items.push_back(dcts_shaped_item{item(k++, t), e, e, pad, 0});
  };
  for (int i = 0; i < 100; ++i) add(int64_t(2) << (i % 5), 0);
  for (int i = 0; i < 70; ++i) add(14, 0);
  add(7, 1);
  add(13, 0);
  add(67, 0);
  add(72, 0);
  add(88, 0);
  finish("dcts_energy_mixed_f32", "175items", st, dcts_energy_mixed_f32(items.data(), (int32_t)items.size(), WS, kBig, st));
  finish("dcts_energy_mixed_f32", "cifar_and_oddpad", st, dcts_energy_mixed_f32(items.data() + 96, 75, WS, kBig, st));
}

// the basis-table memo of one workspace: one shape per workspace, and a same-stream entry only
void memo() {
  const T t{2, 5, 13, 13};
  dcts_workspace_invalidate(WS_MEMO);
  void* const seq[] = {S1, S1, S2, S2, S1};
  int i = 0;
  for (void* st : seq) {
    const int rc = dcts_energy_f32_ex(X, t.N, t.C, t.H, t.W, t.sN(), t.sC(), t.sH(), 1, 0, (int32_t)t.C, 0, OUT, WS_MEMO, kBig, st, DCTS_ALGO_DIRECT);
    std::printf("memo %d %s rc=%d %s |%s\n", i++, token(st), rc, g_records.find("launch_basis") != std::string::npos ? "built" : "reused",
                g_records.c_str());
    g_records.clear();
  }
}

bool hidden(const char* name) {
  const char* v = std::getenv(name);
  return v && !*v;
}

}  // namespace

int main() {
  if (!hidden("HIP_VISIBLE_DEVICES") || !hidden("ROCR_VISIBLE_DEVICES") || std::getenv("DCTS_SPLIT_CHUNK_MB")) {
    std::fprintf(stderr, "stream_trace: start me with HIP_VISIBLE_DEVICES= ROCR_VISIBLE_DEVICES= and without DCTS_SPLIT_CHUNK_MB\n");
    return 2;
  }
  int devices = 0;
  if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {  // belt and braces: the fake pointers must never meet a device
    std::fprintf(stderr, "stream_trace: %d GPU(s) still visible, refusing to run\n", devices);
    return 2;
  }
  for (void* st : {S1, S2}) {
    energy(st);
    coefficients(st);
    weighted(st);
    per_map_statistics(st);
    gm(st);
    typed(st);
    reductions(st);
    lists(st);
  }
  memo();
  return 0;
}
