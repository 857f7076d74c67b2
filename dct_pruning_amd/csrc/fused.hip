// fused.hip - the single-launch fused split kernel (k_split_fused): one role per wave, the intermediate tile parked in
// registers. Edges of DCTS_FUSED_TABLE.
#include <hip/hip_runtime.h>
#include <utility>

#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "split_common.hpp"

using namespace dctsi;

namespace {

// ---------------------------------------------------------------------------------------
// fused split kernel: one launch, HBM traffic = the input, for tiles the register file can park
// ---------------------------------------------------------------------------------------
// One persistent workgroup (2^L role waves) per CU walks over maps. Pass 1 as in k_pass1d, strip
// by strip (64 columns, double-buffered direct-to-LDS staging: strip s+1 streams in while strip s
// is transformed), but the role outputs are not written out: wave q keeps T[line][q*M + k] for
// all its lines in VGPRs (STRIPS*M registers per lane: the whole N x N intermediate tile lives in
// the register file). Pass 2 runs in rounds of 56-64 coefficient columns (KPR from every role):
// the waves dump those parked rows into LDS as an image [line][column], the role butterflies
// run in place along the lines, every wave runs one W-role codelet with lane = column, and the
// squares are accumulated.
template <int M, int L>
struct FusedCfg {
  static constexpr int N = M << L;
  static constexpr int S = 1 << L;
  static constexpr int SW = 64;
  static constexpr int STRIPS = (N + SW - 1) / SW;
  // whole roles per unbalanced round: a power of two, or as many as fit the 64 lanes where that
  // saves a round on the eight-wave kernels (144 = 18 x 8: rounds of 3+3+2 roles instead of four
  // rounds of 2, 26.7 -> 30.9 % of peak; no gain measured at 160 = 10 x 16)
  static constexpr int RPR_P2 = (64 / M) >= 4 ? 4 : ((64 / M) >= 2 ? 2 : 1);
  static constexpr int RPR_FIT = (64 / M) > (1 << L) ? (1 << L) : ((64 / M) >= 1 ? 64 / M : 1);
  static constexpr int RPR = (L <= 3 && (S + RPR_FIT - 1) / RPR_FIT < S / RPR_P2) ? RPR_FIT : RPR_P2;
  // which parked rows go into a pass-2 round:
  //  BALANCED: KPR = 64/S coefficients of EVERY role (all waves dump, equal work; M is padded up to
  //            ROUNDS*KPR with zero columns) - used where the padding wastes <= 1/6 of the columns;
  //  otherwise RPR whole roles per round (only their waves dump).
  static constexpr int KPR_B = 64 / S;
  static constexpr int ROUNDS_B = (M + KPR_B - 1) / KPR_B;
  static constexpr bool BALANCED = (S <= 64) && (6 * (ROUNDS_B * KPR_B - M) <= ROUNDS_B * KPR_B) &&
                                   !(M == 14 && L == 4) && M != 28;  // those two spill when every wave keeps its parked set live
  static constexpr int KPR = KPR_B;
  static constexpr int COLS = BALANCED ? S * KPR_B : RPR * M;  // pass-2 columns (lanes) per round
  static constexpr int ROUNDS = BALANCED ? ROUNDS_B : (S + RPR - 1) / RPR;  // the last round may hold fewer roles
  static constexpr int RW = COLS | 1;                          // pass-2 image row stride (odd: conflict-free dump)
  static constexpr int BUF = (N * SW > N * RW ? N * SW : N * RW);  // floats per LDS buffer
  static_assert(N % 4 == 0, "shape");
};

// image column `lane` of pass-2 round r holds the H-axis leaf output of this row (-1: a padding column)
template <int M, int L, int r>
__device__ __forceinline__ int fused_leaf_row(int lane) {
  using Cfg = FusedCfg<M, L>;
  if constexpr (Cfg::BALANCED) {
    return balanced_leaf_row<M, Cfg::KPR>(lane, r);
  } else {
    const int q = lane / M;
    return (r * Cfg::RPR + q) * M + (lane - q * M);
  }
}

// The one-role-per-wave fused kernel with pass 1 on samples loaded into registers and alternating pass-2 buffers (see
// f2_load_item in split_common.hpp; the staged pass 1 is in git history). Same box, staged -> register loads, % of the
// HBM peak: 96: 38.1 -> 43.2, 192: 33.0 -> 33.9, 256: 35.3 -> 35.8
// (762 maps) / 39.0 -> 41.0 (3000), 112: 38.2 -> 38.3; the shapes AUTO gives to other kernels: 128 45.3 -> 48.9, 144 31.9 -> 34.6,
// 224 29.4 -> 30.8, 160 32.9 -> 33.8, 72 33.4 -> 31.8. No scratch (one coefficient instantiation: 12 B).
//
// STORE: debug / parity instantiation (dcts_dct2d_f32_ex with DCTS_ALGO_FUSED): the weighted leaf outputs
// of pass 2 also go to leaf_out[map][roleH * M + kH][roleW * M + kW]; k_assemble (split_roles.hpp) applies
// the DCT-IV add/sub layers the energy path folds into its weights. No energy is written.
template <int M, int L, int ROLE, bool STORE = false>
__device__ __forceinline__ void fused_body(const TileBatch& tb, lds_ptr lds, lds_ptr partials, int lane,
                                           float* leaf_out = nullptr) {
  using Cfg = FusedCfg<M, L>;
  using P1 = F2Pass1<M, L, ROLE, Cfg::S>;  // this wave's butterfly items: p = ROLE, ROLE + S, ...
  constexpr int N = Cfg::N, S = Cfg::S, SW = Cfg::SW, STRIPS = Cfg::STRIPS, COLS = Cfg::COLS, KPR = Cfg::KPR,
                RPR = Cfg::RPR, ROUNDS = Cfg::ROUNDS, RW = Cfg::RW, BUF = Cfg::BUF;
  int cur = 0, pslot = 0, pending_slot = 0;
  long long pending_m = -1;
  long long m = blockIdx.x;
  DCTS_STAMP_BEGIN();
  const long long nmaps = tb.total;
  int hint_in = 0, hint_next = 0, hint_out = 0;  // tensor of the current / next / finished map (tile_item)
  static_assert(P1::ITEMS <= ROUNDS, "one item of the next map per pass-2 round");
  typename P1::Pre pre;
  if (m < nmaps) DCTS_F2_FIRST_STRIP(ROLE, S, tile_in(tb, m), lane, pre)
  for (; m < nmaps; m += gridDim.x) {
    const float* in_b = tile_in(tb, m, &hint_in);
    float parked[STRIPS][M];
    const bool more_maps = m + gridDim.x < nmaps;
    const float* next_b = more_maps ? tile_in(tb, m + gridDim.x, &hint_next) : in_b;
    // ---- pass 1 on samples in registers: one barrier per strip, the two buffers alternate as role images ---------------
    dcts::static_for<STRIPS>([&](auto is) DCTS_LAMBDA_INLINE {
      constexpr int s = decltype(is)::value;
      const lds_ptr buf = lds + cur * BUF;
      const int ln = launder(lane);
      const bool act = s * SW + ln < N;
      DCTS_STAMP(2);
      DCTS_F2_STRIP(ROLE, S, s, in_b, buf, lane, ln, act, pre)
      DCTS_STAMP(3);
      lds_barrier();
      DCTS_STAMP(4);
      if constexpr (s == 0) {
        if (pending_m >= 0) {
          if constexpr (!STORE) fused_finish<M, L, S, ROLE>(partials, pending_slot, pending_m, tb, lane, &hint_out);
          pending_m = -1;
        }
      }
      split_role_transform<M, L, ROLE>(buf + (act ? launder(lane) : 0), SW, parked[s]);
      DCTS_STAMP(5);
      cur ^= 1;
    });
    // ---- pass 2: W axis, RPR role groups of parked rows per round ---------------------------
    const lds_ptr blk0 = lds + (cur ^ 1) * BUF;  // the last strip's buffer; the other one is free
    const lds_ptr blk1 = lds + cur * BUF;          // rounds alternate between the buffers: two barriers per round (see fused2.hip)
    float e = 0.f;
    dcts::static_for<ROUNDS>([&](auto ir) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(ir)::value;
      const lds_ptr blk = (r % 2 == 1) ? blk1 : blk0;
      DCTS_STAMP(11);
      if constexpr (r == 0) lds_barrier();  // previous readers of blk are done
      DCTS_STAMP(6);
      if constexpr (Cfg::BALANCED) {
        DCTS_DUMP_BALANCED(ROLE, STRIPS, r, blk, lane, parked[s][k])
      } else if constexpr (ROLE / RPR == r) {
        dcts::static_for<STRIPS>([&](auto is) DCTS_LAMBDA_INLINE {
          constexpr int s = decltype(is)::value;
          const int line = s * SW + lane;
          const int off = (line < N ? line : 0) * RW + (ROLE % RPR) * M;
          dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {
            constexpr int k = decltype(ik)::value;
            if (line < N) blk[off + k] = parked[s][k];
          });
        });
      }
      DCTS_STAMP(7);
      DCTS_F2_NEXT_MAP_ITEM(ROLE, S, r, next_b, more_maps, lane, pre)
      lds_barrier();
      DCTS_STAMP(8);
      // columns of this round: all of them, or fewer whole roles in the last unbalanced round
      constexpr int cols_r = Cfg::BALANCED ? COLS : ((S - r * RPR) < RPR ? (S - r * RPR) : RPR) * M;
      const bool act = lane < cols_r;
      split_butterflies<M, L>(blk, RW, act, lane, ROLE);
      DCTS_STAMP(9);
      lds_barrier();
      DCTS_STAMP(10);
      DCTS_ROUND_TAIL(ROLE, STORE, blk + (act ? lane : 0), RW, act, (fused_leaf_row<M, L, r>(lane)), leaf_out, m, o, er)
      if (act) e += er;
      DCTS_STAMP(12);
    });
    // ---- reduce: lanes -> wave -> workgroup, fixed order -------------------------------------
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
    // the workgroup-level sum is deferred past the next barrier the loop executes anyway (the first
    // one of the next map, or the one after the loop): partials are double-buffered by map parity
    if (lane == 0) partials[pslot * S + ROLE] = e;
    pending_m = m;
    pending_slot = pslot;
    pslot ^= 1;
    if constexpr (ROUNDS % 2 == 0) cur ^= 1;  // the next map's first strip must not overwrite the last round's image
    DCTS_STAMP(13);
  }
  if (pending_m >= 0) {
    lds_barrier();
    if constexpr (!STORE) fused_finish<M, L, S, ROLE>(partials, pending_slot, pending_m, tb, lane, &hint_out);
  }
  DCTS_STAMP_END(ROLE, lane);
}

template <int M, int L, bool STORE, int... R>
__device__ __forceinline__ void fused_dispatch(int role, const TileBatch& tb, lds_ptr lds, lds_ptr partials, int lane,
                                               float* leaf_out, std::integer_sequence<int, R...>) {
  ((role == R ? fused_body<M, L, R, STORE>(tb, lds, partials, lane, leaf_out) : (void)0), ...);
}

template <int M, int L>
__global__ __launch_bounds__((64 << L), (fused_waves_per_simd<M, L>())) void k_split_fused(TileBatch tb) {
  using Cfg = FusedCfg<M, L>;
  __shared__ __attribute__((aligned(16))) float lds[2 * Cfg::BUF];
  __shared__ float partials[2 * Cfg::S];
  fused_dispatch<M, L, false>(threadIdx.x >> 6, tb, (lds_ptr)lds, (lds_ptr)partials, threadIdx.x & 63, nullptr,
                              std::make_integer_sequence<int, Cfg::S>{});
}
template <int M, int L>
__global__ __launch_bounds__((64 << L), (fused_waves_per_simd<M, L>())) void k_split_fused_coeff(TileBatch tb, float* leaf_out) {
  using Cfg = FusedCfg<M, L>;
  __shared__ __attribute__((aligned(16))) float lds[2 * Cfg::BUF];
  __shared__ float partials[2 * Cfg::S];
  fused_dispatch<M, L, true>(threadIdx.x >> 6, tb, (lds_ptr)lds, (lds_ptr)partials, threadIdx.x & 63, leaf_out,
                             std::make_integer_sequence<int, Cfg::S>{});
}

template <int M, int L>
int launch_fused(const TileBatch& tb, hipStream_t st) {
  // persistent grid: exactly the workgroups one residency holds (LDS- or register-limited)
  const long long cap = (long long)num_cus() * blocks_per_cu<k_split_fused<M, L>, (1 << L)>();
  const long long grid = tb.total < cap ? tb.total : cap;
  hipLaunchKernelGGL((k_split_fused<M, L>), dim3((unsigned)grid), dim3(64 << L), 0, st, tb);
  return (int)hipGetLastError();
}

}  // namespace

namespace dctsi {

int dispatch_fused_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps,
                         hipStream_t st) {
  DCTS_SWITCH_TABLE(DCTS_FUSED_TABLE, N, [&](auto m, auto l) {
    constexpr int M = decltype(m)::value, L = decltype(l)::value;
    return coeff_role_waves<M, L, k_split_fused_coeff<M, L>, (1 << L)>(x, nmaps, out, scratch, scratch_maps, st);
  })
}

int dispatch_fused(int N, const TileBatch& tb, hipStream_t st) {
  DCTS_SWITCH_TABLE(DCTS_FUSED_TABLE, N,
                    [&](auto m, auto l) { return launch_fused<decltype(m)::value, decltype(l)::value>(tb, st); })
}

}  // namespace dctsi
