// fused2.hip - the fused split kernel with two roles per wave (k_split_fused2): edges of DCTS_FUSED2_TABLE (288, 320).
#include <hip/hip_runtime.h>
#include <utility>

#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "split_common.hpp"

using namespace dctsi;

namespace {

// ---------------------------------------------------------------------------------------
// fused kernel with two roles per wave: 288 = 18 x 16 roles on eight waves
// ---------------------------------------------------------------------------------------
// A 288 x 288 tile (81 K floats) fits the register file of a CU (128 K floats) but not next to the
// codelet working set at 16 waves x 128 VGPRs (5 strips x 18 parked + ~60). Eight waves own 256
// VGPRs each: wave w runs roles 2w and 2w+1 one after the other (2 x 5 x 18 = 180 parked values),
// the butterfly items are shared by the eight waves, the pass-2 dump is the balanced one (KPR
// coefficients of every role per round). Otherwise the fused kernel (fused.hip): pass 1 on samples
// in registers, two alternating LDS images, LDS-only barriers, deferred workgroup sum. One launch, HBM traffic = the
// input once, instead of the 3x of the two-launch path.
template <int M, int L>
struct Fused2Cfg {
  static constexpr int N = M << L, S = 1 << L, NW = S / 2, SW = 64;
  static constexpr int STRIPS = (N + SW - 1) / SW;
  // Two LDS buffers of max(strip, pass-2 image) floats. With all 64 columns per round the image
  // (N x 65) is the larger one; where two of those exceed the 160 KiB (320: 166 KB) a round takes
  // 48 columns (KPR = 3 per role, image N x 49) and the workgroup partials move into the slack behind
  // the image, which costs the deferred workgroup sum (one more barrier per map).
  static constexpr int LDS_FLOATS = 160 * 1024 / 4;
  static constexpr bool WIDE = 2 * N * 65 + 2 * NW <= LDS_FLOATS;
  static constexpr int KPR = WIDE ? 64 / S : 48 / S;
  static constexpr int COLS = S * KPR;
  static constexpr int ROUNDS = (M + KPR - 1) / KPR;
  static constexpr int RW = COLS + 1;
  static constexpr int BUF = N * RW > N * SW ? N * RW : N * SW;
  static constexpr bool DEFER = 2 * BUF + 2 * NW <= LDS_FLOATS;  // room for separate partials
  static_assert(S >= 2 && S <= 16 && N % 4 == 0 && KPR >= 1, "shape");
  static_assert(DEFER || N * RW + NW <= BUF, "partials must fit the slack behind the image");
  static_assert(2 * BUF <= LDS_FLOATS, "LDS");
};

template <int M, int L, int W, bool STORE = false>
__device__ __forceinline__ void fused2_body(const TileBatch& tb, lds_ptr buf0, lds_ptr buf1, lds_ptr partials,
                                            int lane_in, float* leaf_out = nullptr) {
  using Cfg = Fused2Cfg<M, L>;
  using P1 = F2Pass1<M, L, W, Cfg::NW>;
  constexpr int N = Cfg::N, NW = Cfg::NW, SW = Cfg::SW, STRIPS = Cfg::STRIPS, KPR = Cfg::KPR,
                ROUNDS = Cfg::ROUNDS, RW = Cfg::RW, COLS = Cfg::COLS;
  constexpr int R0 = 2 * W, R1 = 2 * W + 1;
  int cur = 0, pslot = 0, pending_slot = 0;
  long long pending_m = -1;
  long long m = blockIdx.x;
  const long long nmaps = tb.total;
  DCTS_STAMP_BEGIN();
  int hint_in = 0, hint_next = 0, hint_out = 0;  // tensor of the current / next / finished map (tile_item)
  // (a lambda: with fused_finish called at its three places, which capture tb and hint_out, both listings moved)
  auto finish = [&](lds_ptr part, int slot, long long mm) DCTS_LAMBDA_INLINE {
    if constexpr (!STORE) fused_finish<M, L, NW, W>(part, slot, mm, tb, lane_in, &hint_out);
  };
  // register-load pass 1: this wave's butterfly items are p = W, W + NW, ... (compile time); pre[i] holds item i's samples
  static_assert(P1::ITEMS <= ROUNDS, "one item of the next map per pass-2 round");
  typename P1::Pre pre;
  if (m < nmaps) DCTS_F2_FIRST_STRIP(W, NW, tile_in(tb, m), lane_in, pre)
  for (; m < nmaps; m += gridDim.x) {
    const float* in_b = tile_in(tb, m, &hint_in);
    float parked[2][STRIPS][M];
    const bool more_maps = m + gridDim.x < nmaps;
    const float* next_b = more_maps ? tile_in(tb, m + gridDim.x, &hint_next) : in_b;
    // ---- pass 1: H axis, strip by strip; butterflies on samples in registers, one barrier per strip ------------
    dcts::static_for<STRIPS>([&](auto is) DCTS_LAMBDA_INLINE {
      constexpr int s = decltype(is)::value;
      const lds_ptr buf = cur ? buf1 : buf0;
      int lane = launder(lane_in);
      const bool act = s * SW + lane < N;
      DCTS_STAMP(2);
      DCTS_F2_STRIP(W, NW, s, in_b, buf, lane_in, lane, act, pre)
      DCTS_STAMP(3);
      lds_barrier();  // the image of strip s is complete; everyone is past the codelets of strip s - 1 (the other buffer)
      DCTS_STAMP(4);
      if constexpr (s == 0) {
        if (pending_m >= 0) {
          finish(partials, pending_slot, pending_m);
          pending_m = -1;
        }
      }
      dcts::static_for<2>([&](auto ii) DCTS_LAMBDA_INLINE {
        constexpr int i = decltype(ii)::value;
        const int ln = launder(lane_in);
        float o[M];
        split_role_transform<M, L, 2 * W + i>(buf + (act ? ln : 0), SW, o);
        dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {
          constexpr int k = decltype(ik)::value;
          asm volatile("" : "+v"(o[k]));  // pin the codelet here (LLVM would sink it to the dump)
          parked[i][s][k] = o[k];
        });
      });
      DCTS_STAMP(5);
      cur ^= 1;
    });
    // ---- pass 2: W axis, KPR coefficients of every role per round ---------------------------
    const lds_ptr blk0 = cur ? buf0 : buf1;  // the last strip's buffer; the other one is free
    const lds_ptr blk1 = cur ? buf1 : buf0;
    // With the samples loaded into registers nothing streams into the second buffer during pass 2: the rounds alternate
    // between the two, and a round's dump need not wait for the readers of the previous round (they use the other buffer;
    // the readers of the round before that are two barriers back): two barriers per round instead of three.
    float e = 0.f;
    dcts::static_for<ROUNDS>([&](auto ir) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(ir)::value;
      const lds_ptr blk = (r % 2 == 1) ? blk1 : blk0;
      DCTS_STAMP(11);
      if constexpr (r == 0) lds_barrier();  // previous readers of blk are done
      DCTS_STAMP(6);
      int lane = launder(lane_in);
      dcts::static_for<2>([&](auto ii) DCTS_LAMBDA_INLINE {
        constexpr int i = decltype(ii)::value;
        DCTS_DUMP_BALANCED(2 * W + i, STRIPS, r, blk, lane, parked[i][s][k])
      });
      DCTS_STAMP(7);
      DCTS_F2_NEXT_MAP_ITEM(W, NW, r, next_b, more_maps, lane_in, pre)
      lds_barrier();
      DCTS_STAMP(8);
      lane = launder(lane_in);
      const bool colact = lane < COLS;
      split_butterflies<M, L, NoHook, false, NW>(blk, RW, colact, lane, W);
      DCTS_STAMP(9);
      lds_barrier();
      DCTS_STAMP(10);
      dcts::static_for<2>([&](auto ii) DCTS_LAMBDA_INLINE {
        constexpr int i = decltype(ii)::value;
        const int ln = launder(lane_in);
        // DCTS_ROUND_TAIL written out: its row test (act && iH >= 0) moved the listing of k_split_fused2_coeff
        float o[M];
        split_role_transform<M, L, 2 * W + i>(blk + (ln < COLS ? ln : 0), RW, o);
        if constexpr (STORE) {  // balanced_leaf_row()
          const int q = ln / KPR, kh = r * KPR + (ln - q * KPR);
          if (ln < COLS && kh < M) {
            float* dst = leaf_out + ((long long)m * N + q * M + kh) * N + (2 * W + i) * M;
            dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE { dst[decltype(ik)::value] = o[decltype(ik)::value]; });
          }
        }
        float er = 0.f;
        dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {
          constexpr int k = decltype(ik)::value;
          er = fmaf(o[k], o[k], er);
        });
        asm volatile("" : "+v"(er));
        if (ln < COLS) e += er;
      });
      DCTS_STAMP(12);
    });
    e = wave_sum_dpp(e);
    if constexpr (Cfg::DEFER) {
      if (lane_in == 0) partials[pslot * NW + W] = e;
      pending_m = m;
      pending_slot = pslot;
      pslot ^= 1;
    } else {
      // no room for a partials array: it lives behind the image, and the sum is taken right away
      // (the next strip only streams into this buffer after the next top-of-strip barrier)
      lds_barrier();  // every wave has finished reading the image
      const lds_ptr blk = ((ROUNDS - 1) % 2 == 1) ? blk1 : blk0;  // the last round's buffer
      const lds_ptr part = blk + N * RW;
      if (lane_in == 0) part[W] = e;
      lds_barrier();
      finish(part, 0, m);
    }
    if constexpr (ROUNDS % 2 == 0) cur ^= 1;  // the next map's first strip must not overwrite the last round's image
  }
  if (pending_m >= 0) {
    lds_barrier();
    finish(partials, pending_slot, pending_m);
  }
  DCTS_STAMP_END(W, lane_in);
}

template <int M, int L, bool STORE, int... Wv>
__device__ __forceinline__ void fused2_dispatch(int wave, const TileBatch& tb, lds_ptr buf0, lds_ptr buf1,
                                                lds_ptr partials, int lane, float* leaf_out,
                                                std::integer_sequence<int, Wv...>) {
  ((wave == Wv ? fused2_body<M, L, Wv, STORE>(tb, buf0, buf1, partials, lane, leaf_out) : (void)0), ...);
}

template <int M, int L>
__global__ __launch_bounds__((64 * Fused2Cfg<M, L>::NW), 2) void k_split_fused2(TileBatch tb) {
  using Cfg = Fused2Cfg<M, L>;
  __shared__ __attribute__((aligned(16))) float buf0[Cfg::BUF];
  __shared__ __attribute__((aligned(16))) float buf1[Cfg::BUF];
  __shared__ float partials[Cfg::DEFER ? 2 * Cfg::NW : 1];
  fused2_dispatch<M, L, false>(threadIdx.x >> 6, tb, (lds_ptr)buf0, (lds_ptr)buf1, (lds_ptr)partials, threadIdx.x & 63,
                               nullptr, std::make_integer_sequence<int, Cfg::NW>{});
}
template <int M, int L>
__global__ __launch_bounds__((64 * Fused2Cfg<M, L>::NW), 2) void k_split_fused2_coeff(TileBatch tb, float* leaf_out) {
  using Cfg = Fused2Cfg<M, L>;
  __shared__ __attribute__((aligned(16))) float buf0[Cfg::BUF];
  __shared__ __attribute__((aligned(16))) float buf1[Cfg::BUF];
  __shared__ float partials[Cfg::DEFER ? 2 * Cfg::NW : 1];
  fused2_dispatch<M, L, true>(threadIdx.x >> 6, tb, (lds_ptr)buf0, (lds_ptr)buf1, (lds_ptr)partials, threadIdx.x & 63,
                              leaf_out, std::make_integer_sequence<int, Cfg::NW>{});
}

template <int M, int L>
int launch_fused2(const TileBatch& tb, hipStream_t st) {
  const long long cap = num_cus();  // LDS: one workgroup per CU
  const long long grid = tb.total < cap ? tb.total : cap;
  hipLaunchKernelGGL((k_split_fused2<M, L>), dim3((unsigned)grid), dim3(64 * Fused2Cfg<M, L>::NW), 0, st, tb);
  return (int)hipGetLastError();
}

}  // namespace

namespace dctsi {

int dispatch_fused2_coeff(int N, const float* x, long long nmaps, float* out, float* scratch, long long scratch_maps,
                          hipStream_t st) {
  DCTS_SWITCH_TABLE(DCTS_FUSED2_TABLE, N, [&](auto m, auto l) {
    constexpr int M = decltype(m)::value, L = decltype(l)::value;
    return coeff_role_waves<M, L, k_split_fused2_coeff<M, L>, Fused2Cfg<M, L>::NW>(x, nmaps, out, scratch, scratch_maps, st);
  })
}

int dispatch_fused2(int N, const TileBatch& tb, hipStream_t st) {
  DCTS_SWITCH_TABLE(DCTS_FUSED2_TABLE, N,
                    [&](auto m, auto l) { return launch_fused2<decltype(m)::value, decltype(l)::value>(tb, st); })
}

}  // namespace dctsi
