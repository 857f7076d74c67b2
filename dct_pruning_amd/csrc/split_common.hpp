// split_common.hpp - what the split, fused, two-roles and pipelined kernels (split_kernels.hpp, fused.hip, fused2.hip,
// pipe.hip) share on top of split_roles.hpp: the role butterflies on an LDS image, the role codelet, the stamp diagnostic,
// the deferred workgroup sum, the balanced dump and the tail of a pass-2 round, pass 1 on samples loaded into registers with
// its pipeline, and on the host the table switch and the coefficient launcher.
// See split_kernels.hpp for the role tree these pieces implement.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dctscore.h"
#include "dct_codelets.hpp"
#include "dcts_internal.h"
#include "split_roles.hpp"

namespace {

// LDS pointers stay in address space 3 end to end: a generic pointer handed through these helpers
// needs a flat->local cast (with a null check) at every use, which ROCm 7.2's gfx950 backend
// mis-selects inside the fused kernel ("V_CMP_NE_U32 0, $src_shared_base": illegal instruction)

// role butterflies, in place: `base` is an LDS image [N rows][rs floats], lanes = columns
struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// `hook` runs once per sample iteration: the fused kernel uses it to trickle out the direct-to-LDS
// loads of the next strip between butterflies instead of issuing them in one burst (a burst of
// 8 x 8 KiB per CU back-pressures the issue: stamps showed 470 cycles per load instruction)
template <int M, int L, class Hook = NoHook>
__device__ __forceinline__ void split_butterflies_pk(lds_ptr base, int rs, bool lane_ok, int lane, int wave,
                                                     Hook hook = Hook{}) {
  // Two samples p, p+1 per iteration as the halves of packed-f32 registers (v_pk_add/mul/fma_f32:
  // two results per issue slot): the network is the same for every p, only the rotation constants
  // differ. This phase is VALU-issue-bound, and the pairs halve its instruction count.
  typedef float f2 __attribute__((ext_vector_type(2)));
  constexpr int S = 1 << L;
  constexpr int NPAIR = (M + 1) / 2;
  constexpr RolePlan<L> plan{};
  const RotTable<M, L>& tab = kRotTable<M, L>;
  lds_ptr colp = base + (lane_ok ? lane : 0);
  for (int j = wave; j < NPAIR; j += S) {
    const int p = 2 * j;                   // even: (-1)^p = +1, (-1)^(p+1) = -1
    const bool two = (M % 2 == 0) || (p + 1 < M);
    const int p1 = two ? p + 1 : p;
    f2 y[S];
    dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int s = decltype(i)::value;
      const int row0 = (s % 2 == 0) ? s * M + p : s * M + M - 1 - p;
      const int row1 = (s % 2 == 0) ? s * M + p1 : s * M + M - 1 - p1;
      y[s] = f2{colp[row0 * rs], colp[row1 * rs]};
    });
    dcts::static_for<plan.NOPS>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int o = decltype(i)::value;
      constexpr int a = plan.op_a[o], bb = plan.op_b[o], r = plan.op_rot[o];
      const f2 ya = y[a], yb = y[bb];
      if constexpr (r < 0) {
        y[a] = ya + yb;
        y[bb] = ya - yb;
      } else {
        constexpr float k0 = RotTable<M, L>::sign0(r);
        const f2 c = f2{tab.c[r][p], tab.c[r][p1]}, sn = f2{tab.s[r][p], tab.s[r][p1]};
        const f2 cs = f2{k0 * c.x, -k0 * c.y}, ss = f2{k0 * sn.x, -k0 * sn.y};  // sign of the second output folded in
        y[a] = ya * c + yb * sn;
        y[bb] = yb * cs - ya * ss;
      }
    });
    if (lane_ok) {
      dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int s = decltype(i)::value;
        const int row0 = (s % 2 == 0) ? s * M + p : s * M + M - 1 - p;
        const int row1 = (s % 2 == 0) ? s * M + p1 : s * M + M - 1 - p1;
        colp[row0 * rs] = y[s].x;
        if (two) colp[row1 * rs] = y[s].y;
      });
    }
    hook();
  }
}

template <int M, int L, class Hook = NoHook, int NW = (1 << L)>
__device__ __forceinline__ void split_butterflies_1(lds_ptr base, int rs, bool lane_ok, int lane, int wave,
                                                    Hook hook = Hook{}) {
  constexpr int S = 1 << L;  // samples of one item; NW waves share the M items (NW < S: two roles per wave)
  constexpr RolePlan<L> plan{};
  const RotTable<M, L>& tab = kRotTable<M, L>;
  lds_ptr colp = base + (lane_ok ? lane : 0);
  for (int p = wave; p < M; p += NW) {
    const float sp = (p & 1) ? -1.f : 1.f;  // (-1)^p
    float y[S];
    dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int s = decltype(i)::value;
      const int row = (s % 2 == 0) ? s * M + p : s * M + M - 1 - p;
      y[s] = colp[row * rs];
    });
    dcts::static_for<plan.NOPS>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int o = decltype(i)::value;
      constexpr int a = plan.op_a[o], bb = plan.op_b[o], r = plan.op_rot[o];
      const float ya = y[a], yb = y[bb];
      if constexpr (r < 0) {
        y[a] = ya + yb;
        y[bb] = ya - yb;
      } else {
        const float c = tab.c[r][p], sn = tab.s[r][p];
        constexpr float k0 = RotTable<M, L>::sign0(r);
        y[a] = ya * c + yb * sn;
        y[bb] = (k0 * sp) * (yb * c - ya * sn);
      }
    });
    if (lane_ok) {
      dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int s = decltype(i)::value;
        const int row = (s % 2 == 0) ? s * M + p : s * M + M - 1 - p;
        colp[row * rs] = y[s];
      });
    }
    hook();
  }
}

// The packed form halves the instruction count but also the number of busy waves, and doubles the
// 2^L live samples. Measured: +3..5 % in the two-launch pass kernel (288, 320), -2..8 % in the
// eight-wave fused kernels (too few waves left to hide LDS latency), spills in the sixteen-wave
// ones. So only k_pass1d asks for it.
template <int M, int L, class Hook = NoHook, bool PACK = false, int NW = (1 << L)>
__device__ __forceinline__ void split_butterflies(lds_ptr base, int rs, bool lane_ok, int lane, int wave,
                                                  Hook hook = Hook{}) {
  if constexpr (PACK)
    split_butterflies_pk<M, L>(base, rs, lane_ok, lane, wave, hook);
  else
    split_butterflies_1<M, L, Hook, NW>(base, rs, lane_ok, lane, wave, hook);
}

// role r's M-point transform of one column of the butterflied image: gathers the role's input
// segment, runs the codelet, applies the role's amplitude weights
template <int M, int L, int ROLE>
__device__ __forceinline__ void split_role_transform(lds_cptr col, int rs, float (&out)[M]) {
  using Leaf = typename RoleLeaf<(M << L), L, ROLE>::type;
  constexpr RolePlan<L> plan{};
  constexpr int SLOT = plan.slot_of_role[ROLE];
  constexpr bool ASC = plan.asc_of_role[ROLE] != 0;
  static_assert(Leaf::len == M, "role tree depth");
  static_assert((plan.is4_of_role[ROLE] != 0) == Leaf::is4, "role plan and role tree disagree");
  float in[M];
  dcts::static_for<M>([&](auto i) DCTS_LAMBDA_INLINE {
    constexpr int q = decltype(i)::value;   // index of the sample in the role's input
    constexpr int p = ASC ? q : M - 1 - q;  // the (p, line) item that produced it
    constexpr int row = (SLOT % 2 == 0) ? SLOT * M + p : SLOT * M + M - 1 - p;
    in[q] = col[row * rs];
  });
  if constexpr (Leaf::is4)
    dcts::Dct4<M>::run(in, out);
  else
    dcts::Dct2<M>::run(in, out);
  constexpr float w0 = float(Leaf::wt(true)), w1 = float(Leaf::wt(false));
  if constexpr (w0 != 1.0f) out[0] *= w0;
  if constexpr (w1 != 1.0f)
    dcts::static_for<M - 1>([&](auto i) DCTS_LAMBDA_INLINE { out[decltype(i)::value + 1] *= w1; });
}

// waves per SIMD the register file allows the fused and the pipelined kernel: STRIPS*M parked values + the codelet's
// working set (STRIPS = the 64-column strips of an edge: FusedCfg::STRIPS, PipeCfg::T)
template <int M, int L>
constexpr int fused_waves_per_simd() {
  const int need = (((M << L) + 63) / 64) * M + 72;
  int w = 512 / ((need + 7) / 8 * 8);
  const int per_wg = (1 << L) / 4 > 0 ? (1 << L) / 4 : 1;
  if (w < per_wg) w = per_wg;
  if (w > 8) w = 8;
  return w;
}

// Diagnostic build only (-DDCTS_FUSED_STAMPS, tools/stamp_fused.sh): s_memtime stamps at the phase
// boundaries of the fused, two-roles and pipelined kernels, summed per wave into g_fused_stamps (never touches an
// output). One __device__ symbol, read back by dcts_debug_fused_stamps (api.hip): all families in one unit (all_units.hip).
// DCTS_STAMP_BEGIN() declares a body's acc_ / last_ and takes the first stamp; DCTS_STAMP_END(wave, lane) adds the wave's sums.
#ifdef DCTS_FUSED_STAMPS
__device__ unsigned long long g_fused_stamps[16][16];
#define DCTS_STAMP(slot) DCTS_STAMP_BODY(slot)
#define DCTS_STAMP_BEGIN()                  \
  unsigned long long acc_[16] = {}, last_; \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(last_)::"memory")
#define DCTS_STAMP_END(wave, lane) \
  if ((lane) == 0)                 \
    for (int i = 0; i < 16; ++i) atomicAdd(&g_fused_stamps[wave][i], acc_[i])
#else
#define DCTS_STAMP(slot) ((void)0)
#define DCTS_STAMP_BEGIN() ((void)0)
#define DCTS_STAMP_END(wave, lane) ((void)0)
#endif

// sum of a map's NP per-wave partials in fixed order (wave 0, lane 0) and the final scale
template <int M, int L, int NP, int WAVE, class Src>
__device__ __forceinline__ void fused_finish(lds_ptr partials, int slot, long long m, const Src& tb, int lane, int* hint = nullptr) {
  constexpr int N = M << L;
  if (WAVE == 0 && lane == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) t += partials[slot * NP + i];
    constexpr float sc = float(4.0 / (double(N) * double(N)));
    *tile_out(tb, m, hint) = t * sc;
  }
}

// ---- a pass-2 round of the fused, two-roles and pipelined kernels: the balanced dump and the round's tail --------------------
// Balanced dump of round r (constexpr), for a body with M, N, SW, KPR and RW in scope: the KPR coefficients r * KPR ... of role
// ROLE's parked rows go to columns ROLE * KPR ... of the image `blk` [line][RW], lane = line within a strip; a padding column
// (coefficient >= M) is written as zero. `val` names the parked value in terms of s (strip) and k (coefficient), the
// constexpr ints declared here. A macro: as a __forceinline__ template that takes the value as a callable it moved the
// listings of 112, though not those of 96 ("One statement of the shared phases").
#define DCTS_DUMP_BALANCED(ROLE, STRIPS, r, blk, lane, val)                              \
  dcts::static_for<STRIPS>([&](auto is) DCTS_LAMBDA_INLINE {                             \
    constexpr int s = decltype(is)::value;                                               \
    const int line = s * SW + lane;                                                      \
    const int off = (line < N ? line : 0) * RW + (ROLE) * KPR;                           \
    dcts::static_for<KPR>([&](auto ic) DCTS_LAMBDA_INLINE {                              \
      constexpr int c = decltype(ic)::value, k = r * KPR + c;                            \
      if constexpr (k < M) {                                                             \
        if (line < N) blk[off + c] = val;                                                \
      } else {                                                                           \
        if (line < N) blk[off + c] = 0.f; /* padding column: exactly zero energy */      \
      }                                                                                  \
    });                                                                                  \
  });

// image column `lane` of balanced round r holds the H-axis leaf output q * M + kh of role q; -1 for a padding column
template <int M, int KPR>
__device__ __forceinline__ int balanced_leaf_row(int lane, int r) {
  const int q = lane / KPR, kh = r * KPR + (lane - q * KPR);
  return kh < M ? q * M + kh : -1;
}

// Tail of a pass-2 round, for a body with M, L and N = M << L in scope: role ROLE's codelet on the image column `col` (row
// stride rs) into o[M] and the sum of squares of the outputs into er, both declared here; the caller pins and adds er. With
// STORE the outputs also go to row `row` (an int expression, evaluated once) of map m's leaf tile at leaf_out, columns
// ROLE * M ..., if `act` holds and the row is not negative. A macro: as a __forceinline__ template that takes the row as a
// callable it moved the listings of the fused family ("One statement of the shared phases").
#define DCTS_ROUND_TAIL(ROLE, STORE, col, rs, act, row, leaf_out, m, o, er)                                          \
  float o[M];                                                                                                        \
  split_role_transform<M, L, ROLE>(col, rs, o);                                                                      \
  if constexpr (STORE) {                                                                                             \
    const int iH = row;                                                                                              \
    if ((act) && iH >= 0) {                                                                                          \
      float* dst = leaf_out + ((long long)m * N + iH) * N + (ROLE) * M;                                              \
      dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE { dst[decltype(ik)::value] = o[decltype(ik)::value]; });   \
    }                                                                                                                \
  }                                                                                                                  \
  float er = 0.f;                                                                                                    \
  dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {                                                              \
    constexpr int k = decltype(ik)::value;                                                                           \
    er = fmaf(o[k], o[k], er);                                                                                       \
  });

// ---- pass 1 of the fused and the two-roles kernel with the samples loaded straight into registers ----------------------
// The staged version (in git history) brought a strip into LDS with direct-to-LDS loads, runs the role butterflies IN PLACE (16 reads, the
// network, 16 writes per item) and then the role codelets read their rows: two LDS writes and two reads per sample, and
// during pass 2 - no free buffer - nothing can stream in. Here an item's 16 samples x[a*M + p~][line] are buffer loads
// (lane = line: 256 contiguous bytes per wave instruction; p is a compile-time constant of the wave, so every row offset
// is an immediate and the rotation constants are literals), the network runs on them in registers and its outputs are
// written once into the role image: one LDS write and one read per sample, one workgroup barrier per strip (the two
// buffers alternate as images), no alignment requirement. The samples of the next strip are requested as soon as an
// item's registers are free (they fly during the remaining butterflies, the barrier and the codelets); those of the next
// map's first strip during pass 2, item by item as the dumps free registers.
// Same box, % of the HBM peak, staged -> register loads -> + pass-2 rounds alternating between the two buffers (two barriers
// per round instead of three): 288 x 288: 28.7 -> 30.4 -> 31.2 (2048 maps), 30.8 -> 33.0 -> 34.2 (4999), 27.3 -> 28.9 -> 29.5 (768);
// 320 x 320: 29.7 -> 31.0 -> 31.5 (2048). 219 / 248 VGPRs, no scratch.
template <int M, int L, int P, int STRIP>
__device__ __forceinline__ void f2_load_item(__amdgpu_buffer_rsrc_t rs, int voff, float (&y)[1 << L]) {
  constexpr int S = 1 << L, N = M << L;
  dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
    constexpr int s = decltype(i)::value;
    constexpr int row = (s % 2 == 0) ? s * M + P : s * M + M - 1 - P;
    y[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, (row * N + STRIP * 64) * 4, 0));
  });
}
template <int M, int L, int P>
__device__ __forceinline__ void f2_network_store(float (&y)[1 << L], lds_ptr image, int rs_lds, int lane, bool act) {
  constexpr int S = 1 << L;
  constexpr RolePlan<L> plan{};
  constexpr RotTable<M, L> tab{};
  constexpr float sp = (P & 1) ? -1.f : 1.f;
  dcts::static_for<plan.NOPS>([&](auto i) DCTS_LAMBDA_INLINE {
    constexpr int o = decltype(i)::value;
    constexpr int a = plan.op_a[o], bb = plan.op_b[o], r = plan.op_rot[o];
    const float ya = y[a], yb = y[bb];
    if constexpr (r < 0) {
      y[a] = ya + yb;
      y[bb] = ya - yb;
    } else {
      constexpr float c = tab.c[r][P], sn = tab.s[r][P];
      constexpr float k0 = RotTable<M, L>::sign0(r);
      y[a] = ya * c + yb * sn;
      y[bb] = (k0 * sp) * (yb * c - ya * sn);
    }
  });
  if (act) {
    lds_ptr colp = image + lane;
    dcts::static_for<S>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int s = decltype(i)::value;
      constexpr int row = (s % 2 == 0) ? s * M + P : s * M + M - 1 - P;
      colp[row * rs_lds] = y[s];
    });
  }
}

// The pipeline around those two for wave W of NW (the fused kernel: NW = 2^L, the two-roles kernel: half of that): the
// wave's butterfly items are p = W, W + NW, ... below M, all compile time; pre[i] holds the samples of item i.
template <int M, int L, int W, int NW>
struct F2Pass1 {
  static constexpr int N = M << L, SW = 64, STRIPS = (N + SW - 1) / SW;
  static constexpr int ITEMS = W < M ? (M - W + NW - 1) / NW : 0;
  using Pre = float[ITEMS > 0 ? ITEMS : 1][1 << L];

  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t map_rsrc(const float* base, bool valid) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, valid ? (unsigned)(N * N * 4) : 0u, 0x00020000);
  }
  static __device__ __forceinline__ int lane_voff(int lane, int strip) {
    const int ln = launder(lane);
    return (strip * SW + ln < N) ? ln * 4 : kLaneOut;
  }
};
// The three places of the pipeline, for a body with M and L in scope and P1 = F2Pass1<M, L, W, NW>. Macros that take W and
// NW as the body writes them: as __forceinline__ members of F2Pass1, or with the item index taken from P1, they moved the
// listings of the fused family ("One statement of the shared phases").
// prologue: the first strip of the workgroup's first map
#define DCTS_F2_FIRST_STRIP(W, NW, first, lane, pre)                 \
  {                                                                  \
    const __amdgpu_buffer_rsrc_t rs = P1::map_rsrc(first, true);     \
    const int vo = P1::lane_voff(lane, 0);                           \
    dcts::static_for<P1::ITEMS>([&](auto ii) DCTS_LAMBDA_INLINE {    \
      constexpr int i = decltype(ii)::value;                         \
      f2_load_item<M, L, W + NW * i, 0>(rs, vo, pre[i]);             \
    });                                                              \
  }
// strip s (constexpr): the network on every item and its outputs into the role image `buf` (ln: the laundered lane, act: it
// has a line); the registers of an item are then free: request its samples of the next strip
#define DCTS_F2_STRIP(W, NW, s, in_b, buf, lane, ln, act, pre)                                                              \
  {                                                                                                                         \
    const __amdgpu_buffer_rsrc_t rs = P1::map_rsrc(in_b, true);                                                             \
    const int vo = (s + 1 < P1::STRIPS) ? P1::lane_voff(lane, s + 1) : 0;                                                   \
    dcts::static_for<P1::ITEMS>([&](auto ii) DCTS_LAMBDA_INLINE {                                                           \
      constexpr int i = decltype(ii)::value;                                                                                \
      f2_network_store<M, L, W + NW * i>(pre[i], buf, P1::SW, ln, act);                                                     \
      if constexpr (s + 1 < P1::STRIPS) f2_load_item<M, L, W + NW * i, (s + 1 < P1::STRIPS ? s + 1 : 0)>(rs, vo, pre[i]);   \
      __builtin_amdgcn_sched_barrier(0);                                                                                    \
    });                                                                                                                     \
  }
// in pass-2 round r (constexpr), whose dump has freed registers: item r of the next map's first strip (no request behind
// the workgroup's last map)
#define DCTS_F2_NEXT_MAP_ITEM(W, NW, r, next_b, more_maps, lane, pre)                                                   \
  if constexpr (r < P1::ITEMS) {                                                                                        \
    const __amdgpu_buffer_rsrc_t rs = P1::map_rsrc(next_b, more_maps);                                                  \
    f2_load_item<M, L, W + NW * (r < P1::ITEMS ? r : 0), 0>(rs, P1::lane_voff(lane, 0), pre[r < P1::ITEMS ? r : 0]);    \
  }

// ---- host side ---------------------------------------------------------------------------------------------------------
// a dispatcher's body: returns f(M, L), both integral constants, for the row of TABLE (an X(N, M, L) list of codelet_sizes.h)
// whose edge is n
#define DCTS_TABLE_CASE(N_, M_, L_) \
  case N_:                          \
    return table_f_(std::integral_constant<int, M_>{}, std::integral_constant<int, L_>{});
#define DCTS_SWITCH_TABLE(TABLE, n, ...) \
  auto&& table_f_ = __VA_ARGS__;         \
  switch (n) {                           \
    TABLE(DCTS_TABLE_CASE)               \
    default:                             \
      return DCTS_E_UNSUPPORTED;         \
  }

// coefficient output of the fused and the two-roles family: `kernel` (workgroups of WAVES waves, one per CU at most) writes
// the leaf outputs of a chunk of maps, k_assemble the coefficients
template <int M, int L, auto kernel, int WAVES>
int coeff_role_waves(const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps, hipStream_t st) {
  auto launch = [st](const TileBatch& tb, float* leaf) {
    const long long grid = tb.total < dctsi::num_cus() ? tb.total : dctsi::num_cus();
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * WAVES), 0, st, tb, leaf);
    return (int)hipGetLastError();
  };
  return run_coeff_chunks(launch, launch_assemble<M, L, true>, M << L, x, nmaps, out, scratch, scratch_maps, st);
}

}  // namespace
