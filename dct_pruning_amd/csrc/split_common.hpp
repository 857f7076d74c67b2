// split_common.hpp - what the split, fused, two-roles and pipelined kernels (split_kernels.hpp, fused.hip, fused2.hip,
// pipe.hip) share on top of split_roles.hpp: the role butterflies on an LDS image, the role codelet, pass 1 on samples
// loaded into registers, the deferred workgroup sum and the stamp diagnostic.
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
#ifdef DCTS_FUSED_STAMPS
__device__ unsigned long long g_fused_stamps[16][16];
#define DCTS_STAMP(slot) DCTS_STAMP_BODY(slot)
#else
#define DCTS_STAMP(slot) ((void)0)
#endif

// sum of a map's per-wave partials in fixed order (wave 0, lane 0) and the final scale
template <int M, int L, int ROLE, class Src>
__device__ __forceinline__ void fused_finish(lds_ptr partials, int slot, long long m, const Src& tb, int lane, int* hint = nullptr) {
  constexpr int S = 1 << L, N = M << L;
  if (ROLE == 0 && lane == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) t += partials[slot * S + i];
    constexpr float sc = float(4.0 / (double(N) * double(N)));
    *tile_out(tb, m, hint) = t * sc;
  }
}

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

}  // namespace
