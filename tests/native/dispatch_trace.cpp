// Dispatch trace: which kernel family, with which arguments, every C-ABI call of libdctscore reaches - without a GPU.
//
// `make -C dct_pruning_amd/csrc trace` compiles api.hip once more with every dispatcher name redirected on the compiler
// command line (-Ddispatch_tile2g=trace_dispatch_tile2g ...) to the recorders below, and links that object with the
// ordinary kernel objects (they supply the real has_tile2g, has_rect, split_ws, band_table_bytes, codelet_group_size)
// and this driver. A recorder appends its own name and arguments to the current line and returns 0; the driver prints
// one line per ABI call: the call, what it dispatched, its return code. Pointers are printed as offsets from four fake
// bases that are never dereferenced. api.hip holds no kernel, so every launch of a call is on record; a positive hipError_t
// (only the api.hip of a commit that still launched kernels of its own returns one) is printed as "launch". The process
// refuses to start unless the GPU is hidden (HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty, no device counted), so it
// can never launch on a fake pointer.
//
// Output: the AUTO part first (between "# AUTO begin" and "# AUTO end": what tests/golden/dispatch_trace_auto.txt
// pins), then the full sweep over explicit families, layouts, workspaces and doubly-bad calls, then the same for the
// entropy, fp16 / bf16 and channels-last entry points, the basis-table memo, and the reductions.
#include <cinttypes>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <set>
#include <string>
#include <vector>

#include "../../dct_pruning_amd/csrc/dcts_internal.h"
#include "../../dct_pruning_amd/csrc/rect.h"
#include "../../include/dctscore.h"

namespace {

// fake "device" addresses: validation, descriptor packing and the memo only do arithmetic on them
constexpr uintptr_t kX = 0x100000000000ull, kOut = 0x200000000000ull, kWs = 0x300000000000ull, kWt = 0x400000000000ull;
float* const X = reinterpret_cast<float*>(kX);
float* const OUT = reinterpret_cast<float*>(kOut);
char* const WS = reinterpret_cast<char*>(kWs);
float* const WT = reinterpret_cast<float*>(kWt);

std::string g_line;

void put(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_line += buf;
}

// x+12 / o+0 / ws+256 / wt+0: floats from the x, out and weights bases, bytes from the workspace base
std::string ptr(const void* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  char buf[64];
  if (!p) return "null";
  const char* name = a >= kWt ? "wt" : a >= kWs ? "ws" : a >= kOut ? "o" : a >= kX ? "x" : "?";
  const uintptr_t base = a >= kWt ? kWt : a >= kWs ? kWs : a >= kOut ? kOut : a >= kX ? kX : 0;
  const uintptr_t off = a - base;
  if (base == kWs || (off & 3))
    std::snprintf(buf, sizeof buf, "%s+%" PRIuPTR "B", name, off);
  else
    std::snprintf(buf, sizeof buf, "%s+%" PRIuPTR, name, off / 4);
  return buf;
}

void put_geom(const dctsi::MapGeom& g) {
  put("{%s n%lld sN%lld sC%lld sH%lld c%d@%d %dx%d %s}", ptr(g.x).c_str(), g.nmaps, g.strideN, g.strideC, g.strideH,
      g.c_count, g.c_begin, g.H, g.W, g.contiguous ? "cont" : "strided");
}

void put_geom(const dctsi::HalfGeom& g) {
  put("{%s n%lld sN%lld sC%lld c%d@%d %s}", ptr(g.x).c_str(), g.nmaps, g.strideN, g.strideC, g.c_count, g.c_begin,
      g.contiguous ? "cont" : "strided");
}
void put_geom(const dctsi::NhwcGeom& g) {
  put("{%s N%lld sN%lld sH%lld sW%lld c%d@%d}", ptr(g.x).c_str(), g.N, g.strideN, g.strideH, g.strideW, g.c_count, g.c_begin);
}

bool same_item(const dctsi::MultiItem& a, const dctsi::MultiItem& b) {
  return a.g.x == b.g.x && a.g.nmaps == b.g.nmaps && a.g.strideN == b.g.strideN && a.g.strideC == b.g.strideC &&
         a.g.strideH == b.g.strideH && a.g.c_count == b.g.c_count && a.g.c_begin == b.g.c_begin && a.g.H == b.g.H &&
         a.g.W == b.g.W && a.g.contiguous == b.g.contiguous && a.out == b.out && a.group_begin == b.group_begin;
}

// count, total_groups, the `count` items, and whether the unused tail repeats item 0 (what the kernels rely on)
void put_items(const dctsi::MultiItem* it, int cap, int count, long long total_groups) {
  put(" cnt%d tg%lld", count, total_groups);
  for (int i = 0; i < count && i < cap; ++i) {
    put(" ");
    put_geom(it[i].g);
    put(">%s@%lld", ptr(it[i].out).c_str(), it[i].group_begin);
  }
  bool tail = true;
  for (int i = count; i < cap; ++i) tail = tail && same_item(it[i], it[0]);
  put(tail ? " tail=it0" : " tail=OTHER");
}

// run-length list: 0,6,0*30,6
template <class T, class F>
void put_rle(const T* v, int n, F one) {
  for (int i = 0; i < n;) {
    int j = i;
    while (j < n && v[j] == v[i]) ++j;
    put("%s%s", i ? "," : "", one(v[i]).c_str());
    if (j - i > 1) put("*%d", j - i);
    i = j;
  }
}

void put_batch(const dctsi::TileBatch& tb) {
  put(" cnt%d tot%lld me%lld x[", tb.count, tb.total, tb.map_elems);
  put_rle(tb.x, dctsi::kTileItems, [](const float* p) { return ptr(p); });
  put("] o[");
  put_rle(tb.out, dctsi::kTileItems, [](float* p) { return ptr(p); });
  put("] b[");
  put_rle(tb.begin, dctsi::kTileItems + 1, [](long long b) { return std::to_string(b); });
  put("]");
}

}  // namespace

// ---- the recorders: same signatures as the dispatchers of dcts_internal.h / rect.h -----------------------------------
namespace dctsi {

// What a recorder returns: 0, the call goes on. A call whose record outgrows kLineCap is stopped with kCut, printed as "cut":
// dcts_weighted_energy_f32 leaves the 2^40-map limit to its inner calls, each of one sample, so with 2^39 samples it would
// go on for 2^39 chunks.
constexpr size_t kLineCap = size_t(1) << 20;
constexpr int kCut = 1 << 20;
int more() { return g_line.size() > kLineCap ? kCut : 0; }

int trace_dispatch_codelet(int store, int HP, int WP, int pad, const MapGeom& g, float* out, hipStream_t) {
  put(" codelet st%d %dx%d p%d ", store, HP, WP, pad);
  put_geom(g);
  put(">%s;", ptr(out).c_str());
  return more();
}
int trace_dispatch_codelet_dma(int N, const MapGeom& g, float* out, hipStream_t) {
  put(" codelet_dma %d ", N);
  put_geom(g);
  put(">%s;", ptr(out).c_str());
  return more();
}
int trace_dispatch_codelet_multi(int HP, int pad, const MultiGeom& mg, hipStream_t) {
  put(" codelet_multi %d p%d", HP, pad);
  put_items(mg.it, kMultiItems, mg.count, mg.total_groups);
  put(";");
  return more();
}
int trace_dispatch_lane(int n, const MultiGeom& mg, hipStream_t) {
  put(" lane %d", n);
  put_items(mg.it, kMultiItems, mg.count, mg.total_groups);
  put(";");
  return more();
}
int trace_dispatch_codelet_mixed(const MixedGeom& mg, hipStream_t) {
  put(" codelet_mixed");
  put_items(mg.it, kMixedItems, mg.count, mg.total_groups);
  put(";");
  return more();
}
int trace_dispatch_band(int HP, int pad, const MapGeom& g, const float* weights, int K, float* table, float* out, hipStream_t) {
  put(" band %d p%d ", HP, pad);
  put_geom(g);
  put(" w%s K%d t%s >%s;", ptr(weights).c_str(), K, ptr(table).c_str(), ptr(out).c_str());
  return more();
}
int trace_launch_band_reduce(const float* coeff, const float* weights, long long nmaps, int hw, int K, float* out, hipStream_t) {
  put(" band_reduce %s w%s n%lld hw%d K%d >%s;", ptr(coeff).c_str(), ptr(weights).c_str(), nmaps, hw, K, ptr(out).c_str());
  return more();
}
int trace_dispatch_entropy(int HP, int pad, const MapGeom& g, float* out, hipStream_t) {
  put(" entropy %d p%d ", HP, pad);
  put_geom(g);
  put(">%s;", ptr(out).c_str());
  return more();
}
int trace_launch_entropy_reduce(const float* coeff, long long nmaps, int hw, float* out, hipStream_t) {
  put(" entropy_reduce %s n%lld hw%d >%s;", ptr(coeff).c_str(), nmaps, hw, ptr(out).c_str());
  return more();
}
int trace_dispatch_half(int N, int dtype, const HalfGeom& g, float* out, hipStream_t) {
  put(" half %d d%d ", N, dtype);
  put_geom(g);
  put(">%s;", ptr(out).c_str());
  return more();
}
int trace_launch_upcast_half(int dtype, const HalfGeom& g, int H, int W, long long strideH, float* dst, hipStream_t) {
  put(" upcast d%d ", dtype);
  put_geom(g);
  put(" %dx%d sH%lld >%s;", H, W, strideH, ptr(dst).c_str());
  return more();
}
int trace_dispatch_nhwc(int N, int dtype, const NhwcGeom& g, float* out, hipStream_t) {
  put(" nhwc %d d%d ", N, dtype);
  put_geom(g);
  put(">%s;", ptr(out).c_str());
  return more();
}
// direct.hip. Kept short, the record lands on most lines: what of x the call reads, the tile, pad, store flag, grid, the three
// workspace regions, whether this call built the tables (a launch_basis went before) or reused what the memo knew of
bool g_tables_built = false;
int trace_launch_basis(float*, int, float*, int, hipStream_t) {
  g_tables_built = true;
  return more();
}
int trace_dispatch_direct(int store, int pad, const MapGeom& g, int grid, const float* CHt, const float* CWt, float* T, float* out,
                          hipStream_t) {
  put(" direct st%d %dx%d p%d {%s n%lld c%d@%d} g%d %s,%s,%s %s >%s;", store, g.H + pad, g.W + pad, pad, ptr(g.x).c_str(), g.nmaps,
      g.c_count, g.c_begin, grid, ptr(CHt).c_str(), ptr(CWt).c_str(), ptr(T).c_str(), g_tables_built ? "built" : "reused",
      ptr(out).c_str());
  g_tables_built = false;
  return more();
}
// reduce.hip
int trace_launch_weighted_reduce(const float* coeff, const float* weights, long long nmaps, int hw, float* out, hipStream_t) {
  put(" weighted_reduce %s w%s n%lld hw%d >%s;", ptr(coeff).c_str(), ptr(weights).c_str(), nmaps, hw, ptr(out).c_str());
  return more();
}
int trace_launch_batch_sum(const float* e, long long N, long long C, float* out_c, hipStream_t) {
  put(" batch_sum %s N%lld C%lld >%s;", ptr(e).c_str(), N, C, ptr(out_c).c_str());
  return more();
}
int trace_launch_running_mean(const float* e, long long N, long long C, float* fr, float total, hipStream_t) {
  put(" running_mean %s N%lld C%lld %s t%g;", ptr(e).c_str(), N, C, ptr(fr).c_str(), total);
  return more();
}
int trace_launch_running_mean_multi(const dcts_update_desc* d, int n, long long cmax, hipStream_t) {
  put(" running_mean_multi n%d cmax%lld %s..%s;", n, cmax, ptr(d[0].energy_nc).c_str(), ptr(d[n - 1].energy_nc).c_str());
  return more();
}
int trace_launch_stream_read(const float* x, long long n, float* sink, hipStream_t) {
  put(" stream_read %s n%lld >%s;", ptr(x).c_str(), n, ptr(sink).c_str());
  return more();
}
int trace_dispatch_split(int N, const MapGeom& g, float* out, void* workspace, hipStream_t) {
  put(" split %d ", N);
  put_geom(g);
  put(">%s %s;", ptr(out).c_str(), ptr(workspace).c_str());
  return more();
}
#define TRACE_TILE(NAME)                                                      \
  int trace_dispatch_##NAME(int N, const TileBatch& tb, hipStream_t) {        \
    put(" " #NAME " %d", N);                                                  \
    put_batch(tb);                                                            \
    put(";");                                                                 \
    return more();                                                                 \
  }
TRACE_TILE(fused)
TRACE_TILE(fused2)
TRACE_TILE(pipe)
TRACE_TILE(tile2d)
TRACE_TILE(tile2g)
TRACE_TILE(tile2g_pad)
#undef TRACE_TILE
#define TRACE_COEFF(NAME)                                                                                             \
  int trace_dispatch_##NAME(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, \
                            hipStream_t) {                                                                            \
    put(" " #NAME " %d %s n%lld >%s scr%s*%lld;", N, ptr(x).c_str(), nmaps, ptr(out).c_str(), ptr(scratch).c_str(),   \
        scratch_maps);                                                                                                \
    return more();                                                                                                         \
  }
TRACE_COEFF(fused_coeff)
TRACE_COEFF(fused2_coeff)
TRACE_COEFF(tile2d_coeff)
TRACE_COEFF(tile2g_coeff)
#undef TRACE_COEFF
int trace_dispatch_rect(const RectGeom& g, float* out, int store_coeff, hipStream_t) {
  const bool rest0 = !g.G && !g.G1 && !g.G2 && !g.S && !g.map_lds && g.scale_e == 0.f && g.scale_c == 0.f;
  put(" rect st%d {%s n%lld sN%lld sC%lld sH%lld c%d@%d %dx%d>%dx%d p%d %s%s}>%s;", store_coeff, ptr(g.x).c_str(), g.nmaps,
      g.strideN, g.strideC, g.strideH, g.c_count, g.c_begin, g.H, g.W, g.HP, g.WP, g.pad, g.contiguous ? "cont" : "strided",
      rest0 ? "" : " REST!=0", ptr(out).c_str());
  return more();
}

}  // namespace dctsi

namespace {

std::string rc_text(int rc) {
  static const char* const names[] = {"ok", "E_NULL", "E_SHAPE", "E_CHANNELS", "E_STRIDE", "E_WORKSPACE", "E_UNSUPPORTED", "E_ALIGN"};
  if (rc == dctsi::kCut) return "cut";
  if (rc > 0) return "launch";  // an api.hip that launched kernels of its own (no device here)
  if (rc >= -7) return names[-rc];
  return std::to_string(rc);
}

void finish(int rc) {
  std::printf("%s => %s\n", g_line.c_str(), rc_text(rc).c_str());
  g_line.clear();
}

enum Entry { ENERGY, COEFF, WEIGHTED, BAND, ENTROPY, TYPED, NHWC };
enum Layout { DENSE, UNALIGNED, PITCHED, BATCH_GAP, SLICE, SLICE_UNALIGNED };
const char* const kEntryName[] = {"e", "c", "w", "b", "s", "t", "n"};
const char* const kLayoutName[] = {"a", "u", "p", "g", "s", "su"};

// one single-tensor call, described by what the sweeps vary
struct Call {
  Entry entry = ENERGY;
  int64_t N = 2, C = 3, H = 8, W = 8;
  Layout layout = DENSE;
  int32_t pad = 0, algo = DCTS_ALGO_AUTO, K = 1;
  const void* ws = WS;
  size_t ws_bytes = size_t(1) << 30;
  // faults, applied on top (doubly-bad calls)
  const float* x = X;
  float* out = OUT;
  const float* weights = WT;
  int64_t strideW = 1;
  int32_t c_begin = -1, c_count = -1;  // -1: from the layout
  // TYPED and NHWC: the element type; the layouts then count in elements of it
  int32_t dtype = DCTS_DTYPE_F16;
  int64_t sW_delta = 0, sH_delta = 0;  // NHWC: added to strideW = C_total and to strideH = W * strideW
};

int issue(const Call& c, const char* tag) {
  int64_t sH = c.W, C_total = c.C;
  int32_t cb = 0, cc = (int32_t)c.C;
  const bool typed = c.entry == TYPED || c.entry == NHWC;
  const size_t elem = typed && c.dtype != DCTS_DTYPE_F32 ? 2 : 4;
  const char* xb = reinterpret_cast<const char*>(c.x);
  if (c.layout == PITCHED) sH = c.W + 4;
  int64_t sC = c.H * sH, sN = c.C * sC;
  if (c.layout == UNALIGNED && xb) xb += elem;
  if (c.layout == BATCH_GAP) sN += 16;
  if (c.layout == SLICE || c.layout == SLICE_UNALIGNED) {
    C_total = c.C + 2;
    cb = 1;
    sN = C_total * sC;
    if (c.layout == SLICE_UNALIGNED && xb) xb += elem;
  }
  if (c.c_begin != -1) cb = c.c_begin;
  if (c.c_count != -1) cc = c.c_count;
  const float* x = reinterpret_cast<const float*>(xb);
  put("%s%s %" PRId64 "x%" PRId64 " p%d a%d %s", kEntryName[c.entry], tag, c.H, c.W, c.pad, c.algo, kLayoutName[c.layout]);
  if (c.entry == BAND) put(" K%d", c.K);
  if (typed) put(" d%d", c.dtype);
  put(" :");
  void* ws = const_cast<void*>(c.ws);
  if (c.entry == NHWC) {
    // channels-last: the channel stride is 1, pixels C_total (+ delta) apart; PITCHED pads the rows, BATCH_GAP the samples
    const int64_t sW = (c.strideW != 1 ? c.strideW : C_total) + c.sW_delta;
    const int64_t nsH = c.W * sW + c.sH_delta + (c.layout == PITCHED ? 4 * sW : 0);
    const int64_t nsN = c.H * nsH + (c.layout == BATCH_GAP ? 16 : 0);
    return dcts_energy_nhwc(xb, c.dtype, c.N, C_total, c.H, c.W, nsN, nsH, sW, cb, cc, c.out, ws, c.ws_bytes, nullptr);
  }
  switch (c.entry) {
    case ENTROPY:
      return dcts_spectral_entropy_f32(x, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.out, ws, c.ws_bytes, nullptr, c.algo);
    case TYPED:
      return dcts_energy_typed(xb, c.dtype, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.out, ws, c.ws_bytes, nullptr);
    case ENERGY:
      return dcts_energy_f32_ex(x, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.out, ws, c.ws_bytes, nullptr, c.algo);
    case COEFF:
      return dcts_dct2d_f32_ex(x, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.out, ws, c.ws_bytes, nullptr, c.algo);
    case WEIGHTED:
      return dcts_weighted_energy_f32(x, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.weights, c.out, ws, c.ws_bytes, nullptr);
    default:
      return dcts_band_energy_f32(x, c.N, C_total, c.H, c.W, sN, sC, sH, c.strideW, cb, cc, c.pad, c.weights, c.K, c.out, ws, c.ws_bytes, nullptr, c.algo);
  }
}
void trace(const Call& c, const char* tag = "") { finish(issue(c, tag)); }

// every edge 1 ... 66, every edge of every family table with its neighbours, 513
std::vector<int> sweep_edges() {
  std::set<int> s;
  for (int e = 1; e <= 66; ++e) s.insert(e);
  auto add = [&](int n) {
    for (int d = -1; d <= 1; ++d) s.insert(n + d);
  };
#define ADD1(N) add(N);
#define ADD3(N, M, L) add(N);
  DCTS_CODELET_SIZES(ADD1)
  DCTS_SPLIT_TABLE(ADD3)
  DCTS_FUSED_TABLE(ADD3)
  DCTS_FUSED2_TABLE(ADD3)
  DCTS_PIPE_TABLE(ADD3)
#undef ADD1
#undef ADD3
  for (int n : {72, 80, 96, 112, 128, 144, 160, 224}) add(n);  // tile2g.hip's and tile2d.hip's own tables
  s.insert(513);
  s.erase(0);
  return std::vector<int>(s.begin(), s.end());
}

// ---- multi / mixed lists --------------------------------------------------------------------------------------------
// What a list holds. BATCHABLE: 16-byte base, base + 1 float, a channel slice of one sample - in turn; all dense, so the
// large-tile families batch them. WITH_GAP: the same with a gap between the samples of the LAST tensor: it takes a call
// of its own (split or direct for some shapes), in the middle of the batch that is still open.
enum Mix { DENSE_ONLY, BATCHABLE, WITH_GAP };
const char* const kMixName[] = {"dense", "batchable", "gap-last"};
dcts_tensor_item make_item(int i, int count, int64_t H, int64_t W, Mix mix) {
  dcts_tensor_item t;
  const int kind = mix == DENSE_ONLY ? 0 : i % 3;
  t.N = 2;
  t.C_total = 3;
  t.strideC = H * W;
  t.strideN = 3 * t.strideC;
  t.c_begin = 0;
  t.c_count = 3;
  t.x = X + (size_t)i * (1u << 22) + (kind == 1 ? 1 : 0);
  t.out_nc = OUT + (size_t)i * 64;
  if (kind == 2) {
    t.N = 1;
    t.C_total = 5;
    t.c_begin = 1;
    t.strideN = 5 * t.strideC;
  }
  if (mix == WITH_GAP && i == count - 1) t.strideN += 16;
  return t;
}

void trace_multi(int count, int64_t H, int64_t W, int pad, Mix mix, bool with_ws) {
  std::vector<dcts_tensor_item> items;
  for (int i = 0; i < count; ++i) items.push_back(make_item(i, count, H, W, mix));
  put("multi %dx %" PRId64 "x%" PRId64 " p%d %s %s :", count, H, W, pad, kMixName[mix], with_ws ? "ws" : "nows");
  finish(dcts_energy_multi_f32(items.data(), count, H, W, pad, with_ws ? WS : nullptr, with_ws ? size_t(1) << 30 : 0, nullptr));
}

struct Shape {
  int64_t H, W;
  int pad;
};
std::vector<dcts_shaped_item> make_mixed(int count, Mix mix) {
  static const Shape shapes[] = {{8, 8, 0}, {4, 4, 0}, {23, 23, 0}, {72, 72, 0}, {32, 32, 0}, {16, 16, 0}, {71, 71, 1}, {13, 17, 0}, {9, 9, 1}, {2, 2, 0}};
  std::vector<dcts_shaped_item> v;
  for (int i = 0; i < count; ++i) {
    const Shape& s = shapes[i % 10];
    dcts_shaped_item it;
    it.t = make_item(i, count, s.H, s.W, mix);
    it.H = s.H;
    it.W = s.W;
    it.pad_front_if_odd = s.pad;
    it.reserved = 0;
    v.push_back(it);
  }
  return v;
}
void trace_mixed(int count, Mix mix, bool with_ws) {
  std::vector<dcts_shaped_item> items = make_mixed(count, mix);
  put("mixed %dx %s %s :", count, kMixName[mix], with_ws ? "ws" : "nows");
  finish(dcts_energy_mixed_f32(items.data(), count, with_ws ? WS : nullptr, with_ws ? size_t(1) << 30 : 0, nullptr));
}

// ---- the AUTO part: what a shape gets when nobody names a family ---------------------------------------------------
void auto_part(const std::vector<int>& edges) {
  std::printf("# AUTO begin\n");
  std::printf("# <entry> HxW p<pad flag> a<algo> <layout a: 16-byte base, u: base + 1 float, p: pitched rows> : dispatches => return\n");
  for (int e : edges)
    for (int pad = 0; pad <= 1; ++pad)
      for (Entry en : {ENERGY, COEFF})
        for (Layout l : {DENSE, UNALIGNED, PITCHED}) {
          if (en == COEFF && l == UNALIGNED) continue;  // no coefficient path looks at the base under AUTO (the full sweep has it)
          Call c;
          c.entry = en;
          c.H = c.W = e;
          c.pad = pad;
          c.layout = l;
          trace(c);
        }
  for (const Shape& s : {Shape{13, 17, 0}, Shape{17, 13, 1}, Shape{56, 28, 0}, Shape{64, 65, 0}, Shape{72, 80, 0}, Shape{1, 512, 0}})
    for (Entry en : {ENERGY, COEFF}) {
      Call c;
      c.entry = en;
      c.H = s.H;
      c.W = s.W;
      c.pad = s.pad;
      trace(c);
    }
  for (const Shape& s : {Shape{8, 8, 0}, Shape{9, 9, 1}, Shape{71, 71, 1}, Shape{72, 72, 0}, Shape{96, 96, 0}, Shape{112, 112, 0}, Shape{128, 128, 0},
                         Shape{224, 224, 0}, Shape{288, 288, 0}, Shape{100, 100, 0}, Shape{67, 67, 0}, Shape{13, 17, 0}})
    for (int count : {2, 3}) trace_multi(count, s.H, s.W, s.pad, BATCHABLE, true);
  for (int e : {72, 96, 8}) trace_multi(33, e, e, 0, BATCHABLE, true);  // across the 32-item chunk; at 96 a 4-byte base joins the fused batch
  // (a tensor that takes a call of its own is served before the open batch is flushed)
  trace_multi(33, 128, 128, 0, WITH_GAP, true);
  trace_multi(33, 71, 71, 1, WITH_GAP, true);
  trace_mixed(12, WITH_GAP, true);
  std::printf("# AUTO end\n");
}

// ---- the full sweep -------------------------------------------------------------------------------------------------
void explicit_families(const std::vector<int>& edges) {
  std::printf("# explicit families: every edge, pad flag, algo 0 ... 9 and an invalid one, both entry points, both bases\n");
  for (int e : edges)
    for (int pad = 0; pad <= 1; ++pad)
      for (int algo = 0; algo <= 10; ++algo)
        for (Entry en : {ENERGY, COEFF})
          for (Layout l : {DENSE, UNALIGNED}) {
            Call c;
            c.entry = en;
            c.H = c.W = e;
            c.pad = pad;
            c.algo = algo == 10 ? 99 : algo;
            c.layout = l;
            trace(c);
          }
  std::printf("# layouts and workspaces\n");
  for (int e : edges)
    for (int pad = 0; pad <= 1; ++pad)
      for (int algo : {DCTS_ALGO_AUTO, DCTS_ALGO_DIRECT, DCTS_ALGO_CODELET, DCTS_ALGO_SPLIT, DCTS_ALGO_PREFETCH, DCTS_ALGO_FUSED, DCTS_ALGO_TILE2D, DCTS_ALGO_RECT})
        for (Entry en : {ENERGY, COEFF})
          for (Layout l : {PITCHED, BATCH_GAP, SLICE, SLICE_UNALIGNED})
            for (int w = 0; w < 3; ++w) {
              if (w != 2 && l != SLICE && l != PITCHED) continue;
              Call c;
              c.entry = en;
              c.H = c.W = e;
              c.pad = pad;
              c.algo = algo;
              c.layout = l;
              if (w == 0) c.ws = nullptr, c.ws_bytes = 0;
              if (w == 1) c.ws_bytes = 64;
              trace(c, w == 0 ? "/nows" : w == 1 ? "/ws64" : "");
            }
  for (Layout l : {DENSE, UNALIGNED})
    for (int e : edges)
      for (int w = 0; w < 2; ++w)
        for (int algo : {DCTS_ALGO_AUTO, DCTS_ALGO_DIRECT, DCTS_ALGO_SPLIT, DCTS_ALGO_FUSED, DCTS_ALGO_TILE2D})
          for (Entry en : {ENERGY, COEFF}) {
            Call c;
            c.entry = en;
            c.H = c.W = e;
            c.algo = algo;
            c.layout = l;
            c.ws = w ? WS : nullptr;
            c.ws_bytes = w ? 64 : 0;
            trace(c, w ? "/ws64" : "/nows");
          }
  std::printf("# non-square\n");
  for (const Shape& s : {Shape{13, 17, 0}, Shape{17, 13, 1}, Shape{56, 28, 0}, Shape{64, 65, 0}, Shape{72, 80, 0}, Shape{1, 512, 0}, Shape{7, 9, 1}})
    for (int algo = 0; algo <= 9; ++algo)
      for (Entry en : {ENERGY, COEFF})
        for (Layout l : {DENSE, UNALIGNED, PITCHED, SLICE}) {
          Call c;
          c.entry = en;
          c.H = s.H;
          c.W = s.W;
          c.pad = s.pad;
          c.algo = algo;
          c.layout = l;
          trace(c);
        }
  std::printf("# one sample, many maps\n");
  for (int e : {7, 8, 72, 128, 224, 100, 67})
    for (Entry en : {ENERGY, COEFF})
      for (Layout l : {DENSE, BATCH_GAP}) {
        Call c;
        c.entry = en;
        c.H = c.W = e;
        c.N = l == DENSE ? 1 : 3;
        c.C = 700;
        c.layout = l;
        trace(c, "/big");
      }
}

void weighted_and_band() {
  std::printf("# weighted and band: fused and fallback shapes, K 1 / 3 / 8, workspaces from too small to ample\n");
  const Shape shapes[] = {{8, 8, 0}, {56, 56, 0}, {9, 9, 1}, {13, 13, 0}, {13, 13, 1}, {23, 23, 1}, {67, 67, 0}, {72, 72, 0}, {71, 71, 1},
                          {100, 100, 0}, {128, 128, 0}, {224, 224, 0}, {288, 288, 0}, {13, 17, 0}, {512, 512, 0}};
  for (const Shape& s : shapes)
    for (Layout l : {DENSE, UNALIGNED, PITCHED, BATCH_GAP, SLICE}) {
      const size_t tile = (size_t)(s.H + 1) * (s.W + 1) * 4, tile0 = (size_t)(s.H + (s.pad && s.H % 2)) * (s.W + (s.pad && s.H % 2)) * 4;
      for (int k : {1, 2, 3, 5, 8, 64}) {
        Call c;
        c.entry = WEIGHTED;
        c.H = s.H;
        c.W = s.W;
        c.pad = s.pad;
        c.layout = l;
        c.ws_bytes = dcts_workspace_bytes(1, 1, s.H, s.W) + k * tile0;
        char tag[32];
        std::snprintf(tag, sizeof tag, "/ws+%dt", k);
        trace(c, tag);
      }
      for (int K : {1, 3, 8})
        for (int algo : {DCTS_ALGO_AUTO, DCTS_ALGO_CODELET, DCTS_ALGO_DIRECT})
          for (int k : {1, 3, 5, 7, 9, 16, 64, 0}) {
            Call c;
            c.entry = BAND;
            c.H = s.H;
            c.W = s.W;
            c.pad = s.pad;
            c.layout = l;
            c.K = K;
            c.algo = algo;
            c.ws_bytes = k ? k * tile : dcts_band_workspace_bytes(c.N, c.C, s.H, s.W, K);
            char tag[32];
            std::snprintf(tag, sizeof tag, k ? "/ws%dt" : "/wsq", k);
            trace(c, tag);
          }
    }
  // more samples than a chunk holds, and more channels than a chunk holds
  for (int e : {13, 72, 100})
    for (int64_t N : {1, 5})
      for (int64_t C : {1, 7}) {
        Call c;
        c.H = c.W = e;
        c.N = N;
        c.C = C;
        c.ws_bytes = 40 * (size_t)(e + 1) * (e + 1) * 4;
        c.entry = BAND;
        c.K = 3;
        trace(c, "/nc");
        c.entry = WEIGHTED;
        trace(c, "/nc");
      }
}

void lists() {
  std::printf("# multi and mixed lists across the 32 / 48 / 64-item chunking\n");
  for (const Shape& s : {Shape{8, 8, 0}, Shape{7, 7, 0}, Shape{9, 9, 1}, Shape{71, 71, 1}, Shape{72, 72, 0}, Shape{96, 96, 0}, Shape{112, 112, 0},
                         Shape{128, 128, 0}, Shape{224, 224, 0}, Shape{288, 288, 0}, Shape{100, 100, 0}, Shape{67, 67, 0}, Shape{23, 23, 1},
                         Shape{13, 17, 0}, Shape{513, 513, 0}})
    for (int count : {1, 2, 31, 32, 33, 47, 48, 49, 63, 64, 65, 70})
      for (Mix mix : {DENSE_ONLY, BATCHABLE, WITH_GAP})
        for (int w = 0; w <= 1; ++w) trace_multi(count, s.H, s.W, s.pad, mix, w != 0);
  for (int count : {1, 2, 31, 32, 33, 47, 48, 49, 63, 64, 65, 70, 130, 500})
    for (Mix mix : {DENSE_ONLY, BATCHABLE, WITH_GAP})
      for (int w = 0; w <= 1; ++w) trace_mixed(count, mix, w != 0);
}

// ---- doubly-bad calls: two faults at once fix the order of the checks ----------------------------------------------
struct Fault {
  const char* name;
  void (*apply)(Call&);
};
const Fault kFaults[] = {
    {"x0", [](Call& c) { c.x = nullptr; }},
    {"out0", [](Call& c) { c.out = nullptr; }},
    {"wt0", [](Call& c) { c.weights = nullptr; }},
    {"N0", [](Call& c) { c.N = 0; }},
    {"W0", [](Call& c) { c.W = 0; }},
    {"edge", [](Call& c) { c.H = c.W = 513; }},
    {"maps", [](Call& c) { c.N = int64_t(1) << 39; c.c_begin = 0; c.c_count = 2; }},
    {"cc0", [](Call& c) { c.c_count = 0; }},
    {"cb", [](Call& c) { c.c_begin = 2; c.c_count = 2; }},
    {"sW", [](Call& c) { c.strideW = 2; }},
    {"xal", [](Call& c) { c.x = reinterpret_cast<const float*>(kX + 2); }},
    {"oal", [](Call& c) { c.out = reinterpret_cast<float*>(kOut + 2); }},
    {"wal", [](Call& c) { c.weights = reinterpret_cast<const float*>(kWt + 2); }},
    {"algo", [](Call& c) { c.algo = 99; }},
    {"K0", [](Call& c) { c.K = 0; }},
    {"K9", [](Call& c) { c.K = 9; }},
    {"ws0", [](Call& c) { c.ws = nullptr; c.ws_bytes = 0; }},
    {"wsal", [](Call& c) { c.ws = WS + 4; }},
    {"ws64", [](Call& c) { c.ws_bytes = 64; }},
};
constexpr int kNFaults = sizeof kFaults / sizeof kFaults[0];

void doubly_bad() {
  std::printf("# doubly-bad calls, single-tensor entry points\n");
  for (Entry en : {ENERGY, COEFF, WEIGHTED, BAND})
    for (int e : {8, 23, 72, 100})
      for (int algo : {DCTS_ALGO_AUTO, DCTS_ALGO_CODELET, DCTS_ALGO_SPLIT, DCTS_ALGO_FUSED})
        for (int i = 0; i < kNFaults; ++i)
          for (int j = i; j < kNFaults; ++j) {
            if (en == WEIGHTED && algo != DCTS_ALGO_AUTO) continue;  // it takes no algo
            Call c;
            c.entry = en;
            c.H = c.W = e;
            c.algo = algo;
            kFaults[i].apply(c);
            if (j != i) kFaults[j].apply(c);
            char tag[48];
            std::snprintf(tag, sizeof tag, "/%s+%s", kFaults[i].name, kFaults[j].name);
            trace(c, tag);
          }

  std::printf("# doubly-bad calls, list entry points\n");
  struct ItemFault {
    const char* name;
    void (*apply)(dcts_tensor_item&);
  };
  const ItemFault ifaults[] = {
      {"x0", [](dcts_tensor_item& t) { t.x = nullptr; }},
      {"out0", [](dcts_tensor_item& t) { t.out_nc = nullptr; }},
      {"N0", [](dcts_tensor_item& t) { t.N = 0; }},
      {"C0", [](dcts_tensor_item& t) { t.C_total = 0; }},
      {"cc0", [](dcts_tensor_item& t) { t.c_count = 0; }},
      {"cb", [](dcts_tensor_item& t) { t.c_begin = 2; }},
      {"xal", [](dcts_tensor_item& t) { t.x = reinterpret_cast<const float*>(kX + 2); }},
      {"oal", [](dcts_tensor_item& t) { t.out_nc = reinterpret_cast<float*>(kOut + 2); }},
      {"maps", [](dcts_tensor_item& t) { t.N = int64_t(1) << 39; t.c_count = 2; }},
  };
  constexpr int n = sizeof ifaults / sizeof ifaults[0];
  for (const Shape& s : {Shape{8, 8, 0}, Shape{72, 72, 0}, Shape{23, 23, 0}, Shape{513, 513, 0}, Shape{0, 8, 0}})
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        for (int where = 0; where < 2; ++where) {  // both faults on item 3, or the first on item 40 and the second on item 3
          std::vector<dcts_tensor_item> items;
          for (int k = 0; k < 45; ++k) items.push_back(make_item(k, 45, s.H ? s.H : 8, s.W, DENSE_ONLY));
          ifaults[i].apply(items[where ? 40 : 3]);
          ifaults[j].apply(items[3]);
          put("multi/%s@%d+%s@3 %" PRId64 "x%" PRId64 " :", ifaults[i].name, where ? 40 : 3, ifaults[j].name, s.H, s.W);
          finish(dcts_energy_multi_f32(items.data(), 45, s.H, s.W, s.pad, WS, size_t(1) << 30, nullptr));
          if (s.H != 8) continue;
          for (int v = 0; v < 3; ++v) {  // and a bad shape on item 1: none, H = 0, an edge beyond DCTS_MAX_EDGE
            std::vector<dcts_shaped_item> mixed = make_mixed(45, DENSE_ONLY);
            ifaults[i].apply(mixed[where ? 40 : 3].t);
            ifaults[j].apply(mixed[3].t);
            if (v == 1) mixed[1].H = 0;
            if (v == 2) mixed[1].H = mixed[1].W = 513;
            put("mixed/%s@%d+%s@3%s :", ifaults[i].name, where ? 40 : 3, ifaults[j].name, v == 1 ? " H0@1" : v == 2 ? " edge@1" : "");
            finish(dcts_energy_mixed_f32(mixed.data(), 45, WS, size_t(1) << 30, nullptr));
          }
        }
  put("multi/null :");
  finish(dcts_energy_multi_f32(nullptr, 0, 0, 8, 0, WS, 64, nullptr));
  std::vector<dcts_tensor_item> one{make_item(0, 1, 8, 8, DENSE_ONLY)};
  one[0].x = nullptr;
  put("multi/count0+x0 :");
  finish(dcts_energy_multi_f32(one.data(), 0, 8, 8, 0, WS, 64, nullptr));
  put("multi/W0+x0 :");
  finish(dcts_energy_multi_f32(one.data(), 1, 8, 0, 0, WS, 64, nullptr));
  put("mixed/null :");
  finish(dcts_energy_mixed_f32(nullptr, 0, WS, 64, nullptr));
  std::vector<dcts_shaped_item> m1 = make_mixed(1, DENSE_ONLY);
  m1[0].t.x = nullptr;
  put("mixed/count0+x0 :");
  finish(dcts_energy_mixed_f32(m1.data(), 0, WS, 64, nullptr));
}

void size_queries(const std::vector<int>& edges) {
  std::printf("# size queries\n");
  for (int e : edges)
    for (int64_t n : {1, 256})
      std::printf("sizes %d n%" PRId64 " : ws %zu weighted %zu band1 %zu band8 %zu has %d/%d\n", e, n, dcts_workspace_bytes(n, 5, e, e),
                  dcts_weighted_workspace_bytes(n, 5, e, e), dcts_band_workspace_bytes(n, 5, e, e, 1),
                  dcts_band_workspace_bytes(n, 5, e, e, 8), dcts_has_codelet(e, e), dcts_has_band_kernel(e, e));
}

// ---- the entry points that came after the first trace: entropy, fp16 / bf16, channels-last ---------------------------
// (all of it after the sections above, which stay as they were)
void entropy_sweep() {
  std::printf("# entropy: fused and fallback shapes, workspaces from none to ample\n");
  const Shape shapes[] = {{8, 8, 0}, {56, 56, 0}, {9, 9, 1}, {13, 13, 0}, {13, 13, 1}, {23, 23, 1}, {67, 67, 0}, {72, 72, 0}, {71, 71, 1},
                          {100, 100, 0}, {128, 128, 0}, {224, 224, 0}, {288, 288, 0}, {13, 17, 0}, {512, 512, 0}};
  for (const Shape& s : shapes)
    for (Layout l : {DENSE, UNALIGNED, PITCHED, BATCH_GAP, SLICE}) {
      const size_t tile = (size_t)(s.H + 1) * (s.W + 1) * 4;
      for (int algo : {DCTS_ALGO_AUTO, DCTS_ALGO_CODELET, DCTS_ALGO_DIRECT})
        for (int k : {-1, 1, 3, 5, 7, 9, 16, 64, 0}) {
          Call c;
          c.entry = ENTROPY;
          c.H = s.H;
          c.W = s.W;
          c.pad = s.pad;
          c.layout = l;
          c.algo = algo;
          c.ws_bytes = k > 0 ? k * tile : k == 0 ? dcts_entropy_workspace_bytes(c.N, c.C, s.H, s.W) : 0;
          if (k < 0) c.ws = nullptr;
          char tag[32];
          std::snprintf(tag, sizeof tag, k > 0 ? "/ws%dt" : k == 0 ? "/wsq" : "/nows", k);
          trace(c, tag);
        }
    }
  // more samples than a chunk holds, and more channels than a chunk holds
  for (int e : {13, 72, 100})
    for (int64_t N : {1, 5})
      for (int64_t C : {1, 7})
        for (Layout l : {DENSE, BATCH_GAP}) {
          Call c;
          c.entry = ENTROPY;
          c.H = c.W = e;
          c.N = N;
          c.C = C;
          c.layout = l;
          c.ws_bytes = 40 * (size_t)(e + 1) * (e + 1) * 4;
          trace(c, "/nc");
        }
}

void typed_sweep() {
  std::printf("# typed: native and staged shapes, dtypes 0 / 1 / 2 and an invalid one, workspaces from none to ample\n");
  const Shape shapes[] = {{8, 8, 0}, {56, 56, 0}, {7, 7, 1}, {13, 13, 0}, {13, 13, 1}, {72, 72, 0}, {100, 100, 0}, {288, 288, 0}, {13, 17, 0}};
  for (const Shape& s : shapes)
    for (int32_t dtype : {0, 1, 2, 7})
      for (Layout l : {DENSE, UNALIGNED, PITCHED, BATCH_GAP, SLICE}) {
        const size_t map = (size_t)s.H * s.W * 4;
        for (int k : {-1, -2, 0, 1, 3, 7, -3, -4}) {  // maps of stage beyond the fp32 path's own need
          Call c;
          c.entry = TYPED;
          c.dtype = dtype;
          c.H = s.H;
          c.W = s.W;
          c.pad = s.pad;
          c.layout = l;
          const size_t inner = dctsi::align_up(dcts_workspace_bytes(c.N, c.C, s.H, s.W), 256);
          if (k >= 0) c.ws_bytes = inner + k * map;
          if (k == -1) c.ws = nullptr, c.ws_bytes = 0;
          if (k == -2) c.ws_bytes = 64;
          if (k == -3) c.ws_bytes = dcts_typed_workspace_bytes(dtype, c.N, c.C, s.H, s.W + 1);  // (H, W + 1): never native
          char tag[32];
          std::snprintf(tag, sizeof tag, k >= 0 ? "/ws+%dm" : k == -1 ? "/nows" : k == -2 ? "/ws64" : k == -3 ? "/wsq" : "/ample", k);
          trace(c, tag);
        }
      }
  // both chunk regimes: whole samples per chunk, and runs of channels of one sample
  for (int e : {13, 72, 100})
    for (int64_t N : {1, 5})
      for (int64_t C : {1, 7})
        for (int k : {3, 16})
          for (Layout l : {DENSE, SLICE}) {
            Call c;
            c.entry = TYPED;
            c.dtype = DCTS_DTYPE_BF16;
            c.H = c.W = e;
            c.N = N;
            c.C = C;
            c.layout = l;
            c.ws_bytes = dctsi::align_up(dcts_workspace_bytes(N, C, e, e), 256) + k * (size_t)e * e * 4;
            trace(c, k == 3 ? "/nc3" : "/nc16");
          }
}

void nhwc_sweep() {
  std::printf("# channels-last: edges with and without a kernel, the three dtypes and an invalid one, the stride rule, a channel slice\n");
  for (const Shape& s : {Shape{1, 1, 0}, Shape{2, 2, 0}, Shape{4, 4, 0}, Shape{7, 7, 0}, Shape{8, 8, 0}, Shape{9, 9, 0}, Shape{13, 13, 0}, Shape{14, 14, 0},
                         Shape{16, 16, 0}, Shape{28, 28, 0}, Shape{32, 32, 0}, Shape{56, 56, 0}, Shape{64, 64, 0}, Shape{72, 72, 0}, Shape{8, 4, 0},
                         Shape{513, 513, 0}})
    for (int32_t dtype : {0, 1, 2, 7})
      for (Layout l : {DENSE, UNALIGNED, PITCHED, BATCH_GAP, SLICE}) {
        Call c;
        c.entry = NHWC;
        c.dtype = dtype;
        c.H = s.H;
        c.W = s.W;
        c.layout = l;
        trace(c);
      }
  // strideW >= C_total and strideH >= W * strideW, one element either side
  for (int e : {8, 28, 9})
    for (Layout l : {DENSE, SLICE})
      for (int64_t dW : {-1, 0, 1, 5})
        for (int64_t dH : {-1, 0, 1}) {
          Call c;
          c.entry = NHWC;
          c.dtype = DCTS_DTYPE_F32;
          c.H = c.W = e;
          c.layout = l;
          c.sW_delta = dW;
          c.sH_delta = dH;
          char tag[32];
          std::snprintf(tag, sizeof tag, "/sW%+d/sH%+d", (int)dW, (int)dH);
          trace(c, tag);
        }
}

const Fault kTypedFaults[] = {
    {"xodd", [](Call& c) { c.x = reinterpret_cast<const float*>(kX + 1); }},
    {"dt", [](Call& c) { c.dtype = 7; }},
};

void doubly_bad_typed() {
  std::printf("# doubly-bad calls, entropy / typed / channels-last\n");
  std::vector<Fault> faults(kFaults, kFaults + kNFaults);
  faults.insert(faults.end(), std::begin(kTypedFaults), std::end(kTypedFaults));
  const int n = (int)faults.size();
  for (Entry en : {ENTROPY, TYPED, NHWC})
    for (int e : {8, 23, 72, 100})
      for (int v = 0; v < 4; ++v)  // entropy: the algo; typed, channels-last: the dtype
        for (int i = 0; i < n; ++i)
          for (int j = i; j < n; ++j) {
            if (en != ENTROPY && v == 3) continue;
            Call c;
            c.entry = en;
            c.H = c.W = e;
            if (en == ENTROPY) c.algo = (const int[]){DCTS_ALGO_AUTO, DCTS_ALGO_CODELET, DCTS_ALGO_SPLIT, DCTS_ALGO_FUSED}[v];
            else c.dtype = v;
            faults[i].apply(c);
            if (j != i) faults[j].apply(c);
            char tag[48];
            std::snprintf(tag, sizeof tag, "/%s+%s", faults[i].name, faults[j].name);
            trace(c, tag);
          }
}

// ---- the basis-table memo: built once per (workspace, stream, shape), forgotten by whatever writes over the tables -----
void memo_pairs() {
  std::printf("# memo: the direct kernel's tables are reused by an identical call and forgotten after a call that overwrites them\n");
  auto direct = [](int e, const char* tag) {
    Call c;
    c.H = c.W = e;
    c.algo = DCTS_ALGO_DIRECT;
    trace(c, tag);
  };
  auto other = [](Entry en, int e, const char* tag) {
    Call c;
    c.entry = en;
    c.H = c.W = e;
    c.algo = en == BAND || en == ENTROPY ? DCTS_ALGO_DIRECT : DCTS_ALGO_AUTO;
    trace(c, tag);
  };
  dcts_workspace_invalidate(WS);
  direct(13, "/first");
  direct(13, "/again");
  other(WEIGHTED, 13, "/over");
  direct(13, "/after-weighted");
  direct(13, "/again");
  direct(15, "/other-shape");
  direct(13, "/after-other-shape");
  other(BAND, 13, "/over");
  direct(13, "/after-band");
  other(ENTROPY, 13, "/over");
  direct(13, "/after-entropy");
  other(COEFF, 72, "/over");  // leaf tiles of the large-tile coefficient path
  direct(13, "/after-coeff");
  other(TYPED, 13, "/staged");  // the staged route calls run() as dcts_energy_f32 does: same tables, same memo
  direct(13, "/after-typed");
  dcts_workspace_invalidate(WS);
  direct(13, "/after-invalidate");
  dcts_workspace_invalidate_range(WS + 64, 16);
  direct(13, "/after-invalidate-range");
}

// ---- what follows the energies: batch sum, running mean (one hook point, many across the 64-item chunking), the read ----
void reductions() {
  std::printf("# reductions\n");
  put("batch_sum :");
  finish(dcts_batch_sum_f32(X, 5, 70, OUT, nullptr));
  put("batch_sum/N0 :");
  finish(dcts_batch_sum_f32(X, 0, 70, OUT, nullptr));
  put("batch_sum/out0 :");
  finish(dcts_batch_sum_f32(X, 5, 70, nullptr, nullptr));
  put("running_mean :");
  finish(dcts_running_mean_update_f32(X, 5, 70, OUT, 3.f, nullptr));
  put("running_mean/C0 :");
  finish(dcts_running_mean_update_f32(X, 5, 0, OUT, 3.f, nullptr));
  put("running_mean/x0 :");
  finish(dcts_running_mean_update_f32(nullptr, 5, 70, OUT, 3.f, nullptr));
  for (int count : {1, 63, 64, 65, 130})
    for (int bad : {-1, 0}) {
      std::vector<dcts_update_desc> d(count);
      for (int i = 0; i < count; ++i) d[i] = dcts_update_desc{X + 4096 * i, OUT + 512 * i, 4, 16 + i, float(i), 0};
      if (bad >= 0) d[bad].C_count = 0;
      put("running_mean_multi %dx bad%d :", count, bad);
      finish(dcts_running_mean_update_multi_f32(d.data(), count, nullptr));
    }
  put("running_mean_multi/null :");
  finish(dcts_running_mean_update_multi_f32(nullptr, 1, nullptr));
  put("stream_read :");
  finish(dcts_debug_stream_read_f32(X, 1 << 20, OUT, nullptr));
  put("stream_read/n0 :");
  finish(dcts_debug_stream_read_f32(X, 0, OUT, nullptr));
}

void size_queries_typed(const std::vector<int>& edges) {
  std::printf("# size queries, entropy / typed / channels-last\n");
  for (int e : edges)
    for (int64_t n : {1, 256})
      std::printf("sizes2 %d n%" PRId64 " : entropy %zu typed %zu/%zu/%zu/%zu nhwc %zu/%zu has %d/%d/%d\n", e, n,
                  dcts_entropy_workspace_bytes(n, 5, e, e), dcts_typed_workspace_bytes(0, n, 5, e, e),
                  dcts_typed_workspace_bytes(1, n, 5, e, e), dcts_typed_workspace_bytes(2, n, 5, e, e),
                  dcts_typed_workspace_bytes(7, n, 5, e, e), dcts_nhwc_workspace_bytes(0, n, 5, e, e),
                  dcts_nhwc_workspace_bytes(1, n, 5, e, e), dcts_has_entropy_kernel(e, e), dcts_has_half_kernel(e, e),
                  dcts_has_nhwc_kernel(e, e));
}

bool hidden(const char* name) {
  const char* v = std::getenv(name);
  return v && !*v;
}

}  // namespace

int main() {
  if (!hidden("HIP_VISIBLE_DEVICES") || !hidden("ROCR_VISIBLE_DEVICES") || std::getenv("DCTS_SPLIT_CHUNK_MB")) {
    std::fprintf(stderr, "dispatch_trace: start me with HIP_VISIBLE_DEVICES= ROCR_VISIBLE_DEVICES= and without DCTS_SPLIT_CHUNK_MB\n");
    return 2;
  }
  int devices = 0;
  if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {  // belt and braces: the fake pointers must never meet a device
    std::fprintf(stderr, "dispatch_trace: %d GPU(s) still visible, refusing to run\n", devices);
    return 2;
  }
  const std::vector<int> edges = sweep_edges();
  auto_part(edges);
  explicit_families(edges);
  weighted_and_band();
  lists();
  doubly_bad();
  size_queries(edges);
  entropy_sweep();
  typed_sweep();
  nhwc_sweep();
  doubly_bad_typed();
  memo_pairs();
  reductions();
  size_queries_typed(edges);
  return 0;
}
