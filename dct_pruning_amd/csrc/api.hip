// api.hip - the C ABI of include/dctscore.h. Every entry point turns its arguments into a TensorView, validate() checks it,
// choose() names the kernel family that serves it (the only place where a shape becomes a family), and run() packs that family's
// descriptor and calls its dispatcher (dcts_internal.h, rect.h). Host code only: every kernel lives in a unit of its own.
//
// Replaces the per-map Python loop of the reference hooks (utils/common.py:262-309):
//   c = [dct.dct_2d(output[i,j,:,:], norm='ortho') ...]; torch.sum(dct.mul(dct)).item()
// with one launch per hooked tensor: every (sample, channel) map gets its orthonormal
// 2-D DCT-II and the squared coefficients are reduced to one fp32 energy per map.
//
// The kernel families are units of their own (codelet.hip, split.hip, fused.hip, fused2.hip, pipe.hip, tile2d.hip,
// tile2g.hip, rect.hip, rank.hip, band.hip, entropy.hip, lowpass.hip, gm.hip, gm_pairs.hip, half.hip, nhwc.hip, direct.hip: the cosine-matrix fallback for any
// (H, W) <= DCTS_MAX_EDGE, reduce.hip: batch sum, running mean, weighted reduction). What stays here of the direct family is
// the memo of its basis tables: which workspace holds which tables is host policy.
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

// the single-tensor entry points' common argument list (x of a 2-byte dtype is tested, never offset: base() is for fp32)
TensorView view_of(const void* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC, int64_t strideH,
                   int64_t strideW, int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd) {
  return TensorView{static_cast<const float*>(x), N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd != 0};
}
// the list entry points: rows are dense by contract
TensorView view_of(const dcts_tensor_item& t, int64_t H, int64_t W, int32_t pad_front_if_odd) {
  return TensorView{t.x, t.N, t.C_total, H, W, t.strideN, t.strideC, W, 1, t.c_begin, t.c_count, pad_front_if_odd != 0};
}
TensorView view_of(const dcts_shaped_item& it) { return view_of(it.t, it.H, it.W, it.pad_front_if_odd); }

// The argument checks, in the one order every entry point makes them in. `ptrs`: the other device pointers the call requires
// (out, weights), tested for NULL and 4-byte alignment together with x. `shape_ok`: the entry point's own shape condition (the
// band count). `x_mask`: the alignment of x, 3 or elem_mask() of its dtype. `channels_last`: the stride rule of that layout
// (pixels at least C_total apart, rows at least W pixels; strideH >= W * strideW without the product) in place of dense NCHW
// rows. The entry points differ only in where they stop:
//   Channels  dcts_weighted_energy_f32: its workspace comes next; the first inner coefficient call checks the rest (so a bad
//             workspace is reported before a bad stride);
//   Align     the list entry points, per item: an edge beyond DCTS_MAX_EDGE or 2^40 maps is found by the per-tensor call;
//   All       everything else.
enum class Checks { Channels, Align, All };
int validate(const TensorView& v, std::initializer_list<const void*> ptrs, Checks upto, bool shape_ok = true, uintptr_t x_mask = 3,
             bool channels_last = false) {
  bool null = !v.x, misaligned = (reinterpret_cast<uintptr_t>(v.x) & x_mask) != 0;
  for (const void* p : ptrs) {
    null = null || !p;
    misaligned = misaligned || (reinterpret_cast<uintptr_t>(p) & 3) != 0;
  }
  if (null) return DCTS_E_NULL;
  if (v.N <= 0 || v.C_total <= 0 || v.H <= 0 || v.W <= 0 || !shape_ok) return DCTS_E_SHAPE;
  if (v.c_count <= 0 || v.c_begin < 0 || (int64_t)v.c_begin + v.c_count > v.C_total) return DCTS_E_CHANNELS;
  if (upto == Checks::Channels) return DCTS_OK;
  if (channels_last ? (v.strideW < v.C_total || v.strideH / v.W < v.strideW) : (v.strideW != 1 || v.strideH < v.W)) return DCTS_E_STRIDE;
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
// Every way a call can be served.
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
TileBatch single_batch(const TensorView& v, float* out) { return single_tensor_batch(v.base(), out, v.nmaps(), v.strideC); }

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
  int rc_tables = 0;
  if (!cache_basis || !basis_cached(workspace, stream, HP, WP)) {
    basis_forget_range(workspace, ws.total);  // whatever tables lay in the bytes this call uses are gone
    const int rc = launch_basis(CHt, HP, CWt, WP, st);
    if (cache_basis && rc == hipSuccess) basis_remember(workspace, wsp + ws.off_ch, ws.off_t - ws.off_ch, stream, HP, WP);
    // (kept as found: a caching call spends the tables' status on the memo; a non-caching one reports it unless the kernel's own is worse)
    if (!cache_basis) rc_tables = rc;
  } else {
    basis_forget_range(wsp + ws.off_t, ws.total - ws.off_t);  // the T tiles may cover another entry's tables
  }
  const int rc = dispatch_direct(store ? 1 : 0, pad, g, ws.grid, CHt, CWt, T, out, st);
  return rc ? rc : rc_tables;
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

// The one chunk loop of the weighted, band, entropy and staged paths: f(n0, ns, c0, nc) for samples [n0, n0 + ns), channels
// [c0, c0 + nc) of the scored slice, at most `chunk` maps each. Whole samples per chunk where the caller says so (chunk >=
// c_count then), else runs of channels of ONE sample. Which of the two is the caller's rule.
template <class F>
int for_chunks(int64_t N, int64_t c_count, long long chunk, bool whole_samples, F f) {
  if (whole_samples) {
    const int64_t ns = chunk / c_count;
    for (int64_t n0 = 0; n0 < N; n0 += ns)
      if (const int rc = f(n0, (N - n0) < ns ? (N - n0) : ns, (int64_t)0, c_count)) return rc;
    return DCTS_OK;
  }
  for (int64_t n = 0; n < N; ++n)
    for (int64_t c0 = 0; c0 < c_count; c0 += chunk)
      if (const int rc = f(n, (int64_t)1, c0, (c_count - c0) < chunk ? (c_count - c0) : chunk)) return rc;
  return DCTS_OK;
}

// A workspace split into [coefficients of `chunk` maps][inner: the scratch the coefficient path may use for them]
struct CoeffWs {
  long long chunk;  // maps; < 1: the workspace is too small
  float* coeff;
  void* inner;
  size_t inner_bytes;
};
CoeffWs coeff_ws(void* workspace, size_t workspace_bytes, long long chunk, size_t tile) {
  const size_t off_inner = align_up((size_t)chunk * tile, 256);
  char* wsp = reinterpret_cast<char*>(workspace);
  return CoeffWs{chunk, reinterpret_cast<float*>(wsp), wsp + off_inner, workspace_bytes - off_inner};
}

// Chunk by chunk (one strided view of x each): coefficients into w.coeff through the coefficient path, then reduce(nmaps,
// first) over the tiles just written; `first` is the index of their first map in the [N, c_count] output.
template <class Reduce>
int coeff_chunks(const TensorView& v, const CoeffWs& w, bool whole_samples, int algo, void* workspace, size_t workspace_bytes,
                 void* stream, Reduce reduce) {
  // this call writes coefficients and scratch all over the workspace: no table cached in it survives, and the inner calls
  // (interior pointer, offset depends on the tile shape) do not cache theirs
  basis_forget(workspace);
  basis_forget_range(workspace, workspace_bytes);
  return for_chunks(v.N, v.c_count, w.chunk, whole_samples, [&](int64_t n0, int64_t ns, int64_t c0, int64_t nc) {
    TensorView s = v;
    s.x = v.x + n0 * v.strideN;
    s.N = ns;
    s.c_begin = (int32_t)(v.c_begin + c0);
    s.c_count = (int32_t)nc;
    if (const int rc = run(true, s, w.coeff, w.inner, w.inner_bytes, stream, algo, /*cache_basis=*/false)) return rc;
    return reduce(ns * nc, n0 * v.c_count + c0);
  });
}

// ---- the band / entropy fallback: workspace = [coefficients of a chunk][the same again + coeff_fixed() for the inner call:
// the direct kernel's tables and T tiles, or leaf tiles of the large-tile kernels] -----------------------------------------
size_t coeff_fixed(int HP, int WP) { return direct_ws(1, HP, WP).off_t + 512; }
// what a workspace of that many bytes holds ...
CoeffWs coeff_layout(void* workspace, size_t workspace_bytes, int HP, int WP) {
  const size_t tile = (size_t)HP * WP * 4, fixed = coeff_fixed(HP, WP);
  const long long chunk = workspace_bytes < fixed + 2 * tile ? 0 : (long long)((workspace_bytes - fixed) / (2 * tile));
  return coeff_ws(workspace, workspace_bytes, chunk, tile);
}
// ... and the bytes the size queries ask for: a chunk of band_chunk_bytes() of coefficients (grid_caps.h), the whole call if less
size_t coeff_layout_bytes(int64_t nmaps, int HP, int WP) {
  const long long tile = (long long)HP * WP * 4;
  long long chunk = band_chunk_bytes(HP, WP) / tile;
  if (chunk < 1) chunk = 1;
  if (chunk > nmaps) chunk = nmaps;
  return coeff_fixed(HP, WP) + 2 * (size_t)(chunk * tile);
}
// Whole samples per chunk where the chunk holds one and one strided view can cover them, else runs of channels of one sample.
// `algo`: the coefficient path of the inner calls; kCoeffAlgoOwn: what coeff_algo() names for the tensor.
constexpr int kCoeffAlgoOwn = -1;
template <class Reduce>
int coeff_fallback(const TensorView& v, void* workspace, size_t workspace_bytes, void* stream, Reduce reduce, int algo = kCoeffAlgoOwn) {
  const CoeffWs w = coeff_layout(workspace, workspace_bytes, (int)v.HP(), (int)v.WP());
  if (w.chunk < 1) return DCTS_E_WORKSPACE;
  if (algo == kCoeffAlgoOwn) algo = coeff_algo(v);
  const bool whole_samples = w.chunk >= v.c_count && (v.contiguous() || algo == DCTS_ALGO_AUTO);
  return coeff_chunks(v, w, whole_samples, algo, workspace, workspace_bytes, stream, reduce);
}
// what the fused band / entropy kernels take, and the algo values those entry points know
bool fused_ok(const TensorView& v) { return has_codelet(v.HP(), v.WP()) && v.dense_rows(); }
bool fused_algo(int algo) { return algo == DCTS_ALGO_AUTO || algo == DCTS_ALGO_CODELET || algo == DCTS_ALGO_DIRECT; }

// ---- the weighted path: workspace = [coefficients of a chunk, to 256 bytes][the same again][what the coefficient path needs] --
size_t weighted_bytes(long long chunk, long long tile, size_t inner) { return 2 * align_up((size_t)(chunk * tile), 256) + inner; }
// the largest chunk a workspace holds beside `inner_min` bytes for the inner calls (the size query caps it at 256 MiB)
long long weighted_chunk(size_t workspace_bytes, long long tile, size_t inner_min) {
  if (workspace_bytes < (size_t)(2 * tile) + inner_min) return 0;
  long long chunk = (long long)((workspace_bytes - inner_min) / (size_t)(2 * tile));
  if (chunk >= 1 && align_up((size_t)(chunk * tile), 256) + (size_t)(chunk * tile) > workspace_bytes) --chunk;
  return chunk;
}

constexpr bool is_half_dtype(int32_t dtype) { return dtype == DCTS_DTYPE_F16 || dtype == DCTS_DTYPE_BF16; }
constexpr uintptr_t elem_mask(int32_t dtype) { return dtype == DCTS_DTYPE_F32 ? 3 : 1; }

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
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  return run(false, v, out_nc, workspace, workspace_bytes, stream, algo);
}

int dcts_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                    int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                    int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd, float* out_nc,
                    void* workspace, size_t workspace_bytes, void* stream) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  return run(false, v, out_nc, workspace, workspace_bytes, stream, DCTS_ALGO_AUTO);
}

int dcts_dct2d_f32_ex(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                      int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                      int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd,
                      float* out_coeff, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t algo) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  return run(true, v, out_coeff, workspace, workspace_bytes, stream, algo);
}

int dcts_dct2d_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W,
                   int64_t strideN, int64_t strideC, int64_t strideH, int64_t strideW,
                   int32_t c_begin, int32_t c_count, int32_t pad_front_if_odd, float* out_coeff,
                   void* workspace, size_t workspace_bytes, void* stream) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  return run(true, v, out_coeff, workspace, workspace_bytes, stream, DCTS_ALGO_AUTO);
}

size_t dcts_weighted_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  // worst case: odd front pad taken; 256 MiB of coefficients per chunk at most
  const long long tile = (long long)(H + 1) * (W + 1) * 4;
  long long chunk = (256LL << 20) / tile;
  if (chunk < 1) chunk = 1;
  if (chunk > N * C_count) chunk = N * C_count;
  return weighted_bytes(chunk, tile, dcts_workspace_bytes(N, C_count, H, W));
}

int dcts_weighted_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                             int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                             int32_t pad_front_if_odd, const float* weights, float* out_nc, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  if (const int rc = validate(v, {out_nc, weights}, Checks::Channels)) return rc;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return workspace ? DCTS_E_ALIGN : DCTS_E_WORKSPACE;
  const long long tile = (long long)v.HP() * v.WP() * 4;  // (the edges are checked by the first inner call, after the workspace)
  const long long chunk = weighted_chunk(workspace_bytes, tile, dcts_workspace_bytes(1, 1, H, W));
  if (chunk < 1) return DCTS_E_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const CoeffWs w = coeff_ws(workspace, workspace_bytes, chunk, (size_t)tile);
  const int hw = (int)(v.HP() * v.WP());
  // always sample by sample
  return coeff_chunks(v, w, /*whole_samples=*/false, coeff_algo(v), workspace, workspace_bytes, stream, [&](int64_t nmaps, int64_t first) {
    return launch_weighted_reduce(w.coeff, weights, nmaps, hw, out_nc + first, st);
  });
}

// ---- K weighted energies per map (band.hip) ------------------------------------------------------------------------
size_t dcts_band_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W, int32_t K) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0 || K < 1 || K > DCTS_BAND_MAX) return 0;
  if (H + 1 > DCTS_MAX_EDGE + 1 || W + 1 > DCTS_MAX_EDGE + 1) return 0;
  // worst case: odd front pad taken. Shapes the fused kernel serves meet the fallback only as row-pitched views.
  const int HP = (int)H + 1, WP = (int)W + 1;
  const size_t fallback = coeff_layout_bytes(N * C_count, HP, WP), table = band_table_bytes(HP, WP, K);
  return align_up(fallback > table ? fallback : table, 256);
}

int dcts_has_band_kernel(int64_t H, int64_t W) { return has_codelet(H, W) ? 1 : 0; }

int dcts_band_energy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                         int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                         int32_t pad_front_if_odd, const float* weights, int32_t K, float* out_nck, void* workspace,
                         size_t workspace_bytes, void* stream, int32_t algo) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  if (const int rc = validate(v, {out_nck, weights}, Checks::All, /*shape_ok=*/K >= 1 && K <= DCTS_BAND_MAX)) return rc;
  const int HP = (int)v.HP(), WP = (int)v.WP();
  if (!fused_algo(algo) || (algo == DCTS_ALGO_CODELET && !fused_ok(v))) return DCTS_E_UNSUPPORTED;
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (fused_ok(v) && algo != DCTS_ALGO_DIRECT) {
    const size_t table_bytes = band_table_bytes(HP, WP, K);
    if (workspace_bytes < table_bytes) return DCTS_E_WORKSPACE;
    basis_forget_range(workspace, table_bytes);  // the table overwrites whatever basis tables lay there
    return dispatch_band(HP, v.pad(), map_geom(v), weights, K, reinterpret_cast<float*>(workspace), out_nck, st);
  }
  // fallback: one reduction per chunk that reads each coefficient once for all K bands
  return coeff_fallback(v, workspace, workspace_bytes, stream, [&](int64_t nmaps, int64_t first) {
    return launch_band_reduce(reinterpret_cast<float*>(workspace), weights, nmaps, HP * WP, K, out_nck + first * K, st);
  });
}

// ---- the spectral entropy of every map (entropy.hip) -----------------------------------------------------------------
// The fused kernel needs no workspace; the fallback is the band fallback with another reduction.
size_t dcts_entropy_workspace_bytes(int64_t N, int64_t C_count, int64_t H, int64_t W) {
  if (N <= 0 || C_count <= 0 || H <= 0 || W <= 0) return 0;
  if (H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return 0;
  // 0 where the fused kernel takes the tile with and without the odd front pad (dense rows)
  if (has_codelet(H, W) && (H % 2 == 0 || has_codelet(H + 1, W + 1))) return 0;
  return align_up(coeff_layout_bytes(N * C_count, (int)H + 1, (int)W + 1), 256);  // worst case: odd front pad taken
}

int dcts_has_entropy_kernel(int64_t H, int64_t W) { return has_codelet(H, W) ? 1 : 0; }

int dcts_spectral_entropy_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                              int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                              int32_t pad_front_if_odd, float* out_nc, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t algo) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  if (const int rc = validate(v, {out_nc}, Checks::All)) return rc;
  const int HP = (int)v.HP(), WP = (int)v.WP();
  if (!fused_algo(algo) || (algo == DCTS_ALGO_CODELET && !fused_ok(v))) return DCTS_E_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (fused_ok(v) && algo != DCTS_ALGO_DIRECT) return dispatch_entropy(HP, v.pad(), map_geom(v), out_nc, st);
  // fallback: one reduction per chunk that reads each coefficient once
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  return coeff_fallback(v, workspace, workspace_bytes, stream, [&](int64_t nmaps, int64_t first) {
    return launch_entropy_reduce(reinterpret_cast<float*>(workspace), nmaps, HP * WP, out_nc + first, st);
  });
}

// ---- the low-pass DCT signature of every map (lowpass.hip) -------------------------------------------------------------
// The fused kernel needs no workspace; the fallback is the band / entropy fallback with a gather in place of the reduction. Its
// inner calls ask for DCTS_ALGO_AUTO, the path dcts_dct2d_f32 takes: the signature is the corner of that call's output bit for
// bit, whatever the chunking.
namespace {
bool lowpass_fused(int64_t H, int64_t W) { return has_codelet(H, W); }
}  // namespace

size_t dcts_dct2d_lowpass_workspace_bytes(int64_t N, int32_t c_count, int64_t H, int64_t W, int32_t K) {
  if (N <= 0 || c_count <= 0 || H <= 0 || W <= 0 || K < 1) return 0;
  if (H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return 0;
  if (lowpass_fused(H, W)) return 0;
  return align_up(coeff_layout_bytes(N * (int64_t)c_count, (int)H, (int)W), 256);
}

int dcts_dct2d_lowpass_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC,
                           int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, int32_t K, int32_t flags,
                           float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, /*pad_front_if_odd=*/0);
  if (const int rc = validate(v, {out}, Checks::All)) return rc;
  if (K < 1) return DCTS_E_SHAPE;
  if (flags & ~DCTS_LOWPASS_DROP_DC) return DCTS_E_UNSUPPORTED;
  const int drop_dc = (flags & DCTS_LOWPASS_DROP_DC) ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const MapGeom g = map_geom(v);
  if (lowpass_fused(H, W) && v.dense_square()) return dispatch_lowpass((int)H, g, K, drop_dc, out, st);
  // fallback: one gather per chunk that copies the corner of every tile
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  const int Kh = (int)(K < H ? K : H), Kw = (int)(K < W ? K : W);
  return coeff_fallback(v, workspace, workspace_bytes, stream, [&](int64_t nmaps, int64_t first) {
    return launch_lowpass_gather(reinterpret_cast<float*>(workspace), nmaps, first, g, Kh, Kw, drop_dc, out, st);
  }, DCTS_ALGO_AUTO);
}

// ---- the summed distance of every scored map to a reference set (gm.hip) ------------------------------------------------
// Two channel ranges, each checked as the scored one of every other entry; then the common checks on the scored range. Dense
// maps only: a row pitch is the caller's copy. No workspace, no host state.
namespace {
int gm_geom(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC, int64_t strideH,
            int64_t strideW, int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count, const float* out_nc, GmGeom* g) {
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, /*pad_front_if_odd=*/0);
  const TensorView r = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, r_begin, r_count, /*pad_front_if_odd=*/0);
  if (const int rc = validate(v, {out_nc}, Checks::Channels)) return rc;
  if (const int rc = validate(r, {out_nc}, Checks::Channels)) return rc;
  if (const int rc = validate(v, {out_nc}, Checks::All)) return rc;
  if (!v.dense_rows()) return DCTS_E_UNSUPPORTED;  // strideH > W
  *g = GmGeom{x, N, strideN, strideC, c_begin, c_count, r_begin, r_count, (int)(H * W)};
  return DCTS_OK;
}
}  // namespace

int dcts_gm_distance_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC,
                         int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count,
                         float* out_nc, void* stream) {
  GmGeom g;
  if (const int rc = gm_geom(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, r_begin, r_count, out_nc, &g))
    return rc;
  return dispatch_gm(g, out_nc, reinterpret_cast<hipStream_t>(stream));
}

// The normalised metrics: the workspace holds the (mu, s) pairs of the scored range, then those of the reference range.
size_t dcts_gm_workspace_bytes(int32_t metric, int64_t N, int32_t c_count, int32_t r_count) {
  if (metric != DCTS_GM_COSINE && metric != DCTS_GM_CORRELATION) return 0;
  if (N <= 0 || c_count <= 0 || r_count <= 0) return 0;
  return gm_stats_bytes(N, c_count) + gm_stats_bytes(N, r_count);
}

int dcts_gm_distance_metric_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC,
                                int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, int32_t r_begin,
                                int32_t r_count, float* out_nc, void* stream, int32_t metric, void* workspace,
                                size_t workspace_bytes) {
  GmGeom g;
  if (const int rc = gm_geom(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, r_begin, r_count, out_nc, &g))
    return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (metric == DCTS_GM_L2) return dispatch_gm(g, out_nc, st);
  if (metric != DCTS_GM_COSINE && metric != DCTS_GM_CORRELATION) return DCTS_E_UNSUPPORTED;
  if (!workspace) return DCTS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
  const size_t scored = gm_stats_bytes(N, c_count), need = scored + gm_stats_bytes(N, r_count);
  if (workspace_bytes < need) return DCTS_E_WORKSPACE;
  basis_forget_range(workspace, need);  // the pairs overwrite whatever basis tables lay there
  char* ws = reinterpret_cast<char*>(workspace);
  return dispatch_gm_metric(g, metric == DCTS_GM_CORRELATION, reinterpret_cast<float2*>(ws), reinterpret_cast<float2*>(ws + scored),
                            out_nc, st);
}

// ---- the pair matrix (gm_pairs.hip) -------------------------------------------------------------------------------------
// The workspace: [the (mu, s) pairs of the scored range][those of the reference range] as dcts_gm_distance_metric_f32 lays them
// out (a metric only), then [S][c_count][r_count] partial matrices where the samples are cut into S > 1 slices.
int32_t dcts_gm_pairs_slices(int64_t N, int32_t r_count) { return gm_pair_slices(N, r_count); }

size_t dcts_gm_pairs_workspace_bytes(int32_t metric, int64_t N, int32_t c_count, int32_t r_count) {
  if (metric != DCTS_GM_L2 && metric != DCTS_GM_COSINE && metric != DCTS_GM_CORRELATION) return 0;
  if (N <= 0 || c_count <= 0 || r_count <= 0) return 0;
  return dcts_gm_workspace_bytes(metric, N, c_count, r_count) + gm_pair_partial_bytes(gm_pair_slices(N, r_count), c_count, r_count);
}

int dcts_gm_pairs_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN, int64_t strideC,
                      int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, int32_t r_begin, int32_t r_count,
                      float* out_cr, void* stream, int32_t metric, void* workspace, size_t workspace_bytes) {
  GmGeom g;
  if (const int rc = gm_geom(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, r_begin, r_count, out_cr, &g))
    return rc;
  if (metric != DCTS_GM_L2 && metric != DCTS_GM_COSINE && metric != DCTS_GM_CORRELATION) return DCTS_E_UNSUPPORTED;
  const size_t stats = dcts_gm_workspace_bytes(metric, N, c_count, r_count);
  const size_t need = stats + gm_pair_partial_bytes(gm_pair_slices(N, r_count), c_count, r_count);
  char* ws = reinterpret_cast<char*>(workspace);
  if (need) {  // one slice without a metric needs none: NULL / 0 are fine
    if (!workspace) return DCTS_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return DCTS_E_ALIGN;
    if (workspace_bytes < need) return DCTS_E_WORKSPACE;
    basis_forget_range(workspace, need);  // the pairs and partials overwrite whatever basis tables lay there
  }
  const size_t scored = stats ? gm_stats_bytes(N, c_count) : 0;
  return dispatch_gm_pairs(g, metric == DCTS_GM_L2 ? -1 : (metric == DCTS_GM_CORRELATION ? 1 : 0), reinterpret_cast<float2*>(ws),
                           reinterpret_cast<float2*>(ws + scored), reinterpret_cast<float*>(ws + stats), out_cr,
                           reinterpret_cast<hipStream_t>(stream));
}

// ---- fp16 / bf16 inputs (half.hip) -----------------------------------------------------------------------------------
// The staged route's workspace: [what the fp32 path needs for the chunk it is given][dense fp32 copy of a chunk of maps].
// The fp32 part is at the head, so that a direct-kernel call keeps its tables where dcts_energy_f32 would: run() is called as
// dcts_energy_f32 calls it, so the EXISTING basis-table memo (keyed on the caller's workspace pointer, forgotten through
// dcts_workspace_invalidate[_range]) serves the staged route as well. That is the only host state it touches; none is added.
// (at most kHalfStageCap bytes of upcast maps per chunk: grid_caps.h)
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
  const TensorView v = view_of(x, N, C_total, H, W, strideN, strideC, strideH, strideW, c_begin, c_count, pad_front_if_odd);
  if (const int rc = validate(v, {out_nc}, Checks::All, true, elem_mask(dtype))) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const uint16_t* xh = reinterpret_cast<const uint16_t*>(x);
  if (has_half(H, W) && v.pad() == 0 && strideH == W)
    return dispatch_half((int)H, dtype, HalfGeom{xh, v.nmaps(), strideN, strideC, c_count, c_begin, v.contiguous() ? 1 : 0}, out_nc, st);

  // staged: upcast a chunk of maps into the workspace, score it through the fp32 path under AUTO. Whole samples per chunk
  // where the workspace holds one, else runs of channels of one sample.
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
  return for_chunks(N, c_count, chunk, /*whole_samples=*/chunk >= c_count, [&](int64_t n0, int64_t ns, int64_t c0, int64_t nc) -> int {
    const HalfGeom g{xh + n0 * strideN, ns * nc, strideN, strideC, (int)nc, (int)(c_begin + c0), (ns == 1 || strideN == nc * strideC) ? 1 : 0};
    if (const int rc = launch_upcast_half(dtype, g, (int)H, (int)W, strideH, stage, st)) return rc;
    const TensorView s{stage, ns, nc, H, W, nc * H * W, H * W, W, 1, 0, (int32_t)nc, pad_front_if_odd != 0};
    return run(false, s, out_nc + n0 * c_count + c0, inner, inner_bytes, stream, DCTS_ALGO_AUTO);
  });
}

// ---- channels-last maps (nhwc.hip) ------------------------------------------------------------------------------------
int dcts_has_nhwc_kernel(int64_t H, int64_t W) { return has_nhwc(H, W) ? 1 : 0; }

// nothing is staged: the native kernels read the tensor where it lies, and every other shape is refused
size_t dcts_nhwc_workspace_bytes(int32_t, int64_t, int64_t, int64_t, int64_t) { return 0; }

int dcts_energy_nhwc(const void* x, int32_t dtype, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                     int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count, float* out_nc, void*, size_t, void* stream) {
  if (dtype != DCTS_DTYPE_F32 && !is_half_dtype(dtype)) return DCTS_E_UNSUPPORTED;
  const TensorView v = view_of(x, N, C_total, H, W, strideN, /*strideC=*/1, strideH, strideW, c_begin, c_count, /*pad_front_if_odd=*/0);
  if (const int rc = validate(v, {out_nc}, Checks::All, true, elem_mask(dtype), /*channels_last=*/true)) return rc;
  if (!has_nhwc(H, W)) return DCTS_E_UNSUPPORTED;  // the caller's copy into the NCHW layout stays the caller's
  return dispatch_nhwc((int)H, dtype, NhwcGeom{x, N, strideN, strideH, strideW, c_begin, c_count}, out_nc, reinterpret_cast<hipStream_t>(stream));
}

int dcts_batch_sum_f32(const float* energy_nc, int64_t N, int64_t C_count, float* out_c,
                       void* stream) {
  if (!energy_nc || !out_c) return DCTS_E_NULL;
  if (N <= 0 || C_count <= 0) return DCTS_E_SHAPE;
  return launch_batch_sum(energy_nc, N, C_count, out_c, reinterpret_cast<hipStream_t>(stream));
}

int dcts_running_mean_update_f32(const float* energy_nc, int64_t N, int64_t C_count,
                                 float* feature_result, float total_before, void* stream) {
  if (!energy_nc || !feature_result) return DCTS_E_NULL;
  if (N <= 0 || C_count <= 0) return DCTS_E_SHAPE;
  return launch_running_mean(energy_nc, N, C_count, feature_result, total_before, reinterpret_cast<hipStream_t>(stream));
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
  // every descriptor before the first launch: the update is in place, so a refusal after a chunk had been enqueued would
  // leave that chunk's feature_result advanced under a caller that keeps its totals and retries
  for (const dcts_update_desc* d = descs; d < descs + count; ++d) {
    if (!d->energy_nc || !d->feature_result) return DCTS_E_NULL;
    if (d->N <= 0 || d->C_count <= 0) return DCTS_E_SHAPE;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc = DCTS_OK;  // of the last launch that failed: every chunk is launched
  for (int32_t i0 = 0; i0 < count; i0 += kMultiMax) {
    const int n = (count - i0) < kMultiMax ? (count - i0) : kMultiMax;
    int64_t cmax = 0;
    for (const dcts_update_desc* d = descs + i0; d < descs + i0 + n; ++d)
      if (d->C_count > cmax) cmax = d->C_count;
    if (const int r = launch_running_mean_multi(descs + i0, n, cmax, st)) rc = r;
  }
  return rc;
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
  return launch_stream_read(x, n, sink, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
