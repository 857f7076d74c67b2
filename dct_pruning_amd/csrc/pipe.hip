// pipe.hip - the pipelined fused split kernel (k_split_pipe): edges of DCTS_PIPE_TABLE (128, 224).
#include <hip/hip_runtime.h>
#include <utility>

#include "../../include/dctscore.h"
#include "codelet_sizes.h"
#include "split_common.hpp"

using namespace dctsi;

namespace {

// ---------------------------------------------------------------------------------------
// pipelined fused kernel: pass 2 of map m interleaved with pass 1 of map m+1
// ---------------------------------------------------------------------------------------
// The fused kernel (fused.hip) streams a map in (pass 1, HBM-bound), then transforms the parked tile
// (pass 2, no HBM traffic at all): the two halves alternate and neither the memory system nor the
// VALUs are ever busy for more than half of the time. Here one step = pass-2 round r of the
// previous map followed by pass-1 strip r of the current one, so the direct-to-LDS loads of strip
// r+1 are in flight for a whole step (both halves) and the kernel becomes VALU-issue-bound.
// Registers: every round dumps KPR coefficients of every wave's parked rows (the balanced dump),
// which frees exactly the registers the next strip's M outputs need, so the parked set never
// exceeds one tile: slots P[T][T][KPR], T = strips = rounds. A map parked with layout 0 keeps
// T[strip s][coef k] in P[k/KPR][s][k%KPR], layout 1 in P[s][k/KPR][k%KPR]: round r of a
// layout-0 map frees P[r][*][*], which is where strip r of the next map (layout 1) goes, and vice
// versa; maps alternate layouts, the loop body is unrolled over the two parities.
// LDS: two buffers. Step k transforms the staged strip in B[k%2]; the pass-2 image of that step
// lives in B[(k+1)%2], which then receives strip k+1 while B[k%2] is transformed.
template <int M, int L>
struct PipeCfg {
  static constexpr int N = M << L, S = 1 << L, SW = 64;
  static constexpr int T = (N + SW - 1) / SW;
  static constexpr int KPR = 64 / S;
  static constexpr int RW = 65;  // pass-2 image row stride: 64 columns, odd
  static constexpr int BUF = N * RW;
  static_assert((M + KPR - 1) / KPR == T, "rounds == strips");
  static_assert(S <= 16 && N % 4 == 0, "shape");
  // Register relief: NP of the M outputs of strip s are parked in LDS instead (one dword per thread
  // and value, conflict-free), namely the last NP real coefficients of round s. Those are dumped
  // in step s of the next map, before strip s of that map overwrites them, so one copy is enough.
  static constexpr int LDS_FLOATS = 160 * 1024 / 4 - 2 * S - 64;
  static constexpr int last_real = M - (T - 1) * KPR;  // real coefficients in the last round
  static constexpr int NP_FIT = (LDS_FLOATS - 2 * BUF) / (T * 64 * S);
  static constexpr int NP = NP_FIT < 0 ? 0 : (NP_FIT > 2 ? 2 : NP_FIT) > last_real ? last_real : (NP_FIT > 2 ? 2 : NP_FIT);
  static constexpr int nreal(int r) { return r == T - 1 ? last_real : KPR; }
  // index (0..NP-1) of coefficient k of strip s in the LDS park, or -1 if it stays in a register
  static constexpr int park_index(int s, int k) {
    if (k / KPR != s) return -1;
    const int c = k % KPR, first = nreal(s) - NP;
    return (c >= first && c < nreal(s)) ? c - first : -1;
  }
};

// one direct-to-LDS instruction (64 lanes x 16 B) of a strip's staging: piece `it` of PIECES.
// lane q = it*THREADS + wave*64 + lane covers row q/16, columns 4*(q%16).. of the 64-wide strip
template <int M, int L>
struct FusedStage {
  static constexpr int N = M << L, SW = 64, THREADS = 64 << L;
  static constexpr int NQUADS = N * SW / 4;
  static constexpr int PIECES = (NQUADS + THREADS - 1) / THREADS;
  static_assert(SW == 64, "piece addressing assumes 16 quads per row");
  // One direct-to-LDS load, issued as a raw instruction. The compiler tracks direct-to-LDS loads it knows about and
  // puts s_waitcnt vmcnt(0) in front of the next LDS access that may alias the destination; its
  // alias information does not survive this kernel's pointer arithmetic, so EVERY following
  // ds_read/ds_write waited for the prefetch to land (one memory round trip per instalment). The
  // pipelined kernel orders these loads itself: s_waitcnt vmcnt(0) + barrier before the strip is read.
  static __device__ __forceinline__ void piece_raw(const float* __restrict__ in_b, int strip, lds_ptr buf, int lane,
                                                   int wave, int it) {
    const int qbase = it * THREADS + wave * 64;  // wave-uniform
    const int q = qbase + lane;
    const int row = q >> 4, col = (q & 15) << 2;
    if (q < NQUADS && strip * SW + col < N) {
      const float* base = in_b + strip * SW;                // wave-uniform (tile_in)
      const unsigned off = (unsigned)(row * N + col) * 4u;  // bytes
      const unsigned dst = (unsigned)(unsigned long long)(buf + 4 * qbase);
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                   :
                   : "s"(dst), "v"(off), "s"(base)
                   : "memory", "m0");
    }
  }
};

template <int PAR, int SI, int K, int T, int KPR>
__device__ __forceinline__ float& pipe_slot(float (&P)[T][T][KPR]) {
  if constexpr (PAR == 0)
    return P[K / KPR][SI][K % KPR];
  else
    return P[SI][K / KPR][K % KPR];
}

template <int M, int L, int ROLE>
__device__ __forceinline__ void pipe_body(const PlainMaps& tb, lds_ptr buf0, lds_ptr buf1, lds_ptr parkbuf,
                                          lds_ptr partials, int lane_in) {
  using Cfg = PipeCfg<M, L>;
  using Stage = FusedStage<M, L>;
  constexpr int N = Cfg::N, S = Cfg::S, SW = Cfg::SW, T = Cfg::T, KPR = Cfg::KPR, RW = Cfg::RW, BUF = Cfg::BUF;
  float P[T][T][KPR];
  const lds_ptr park = parkbuf + (ROLE * 64 + lane_in);  // [T * NP][64 * S]
  long long m_cur = blockIdx.x, m_prev = -1, pending_m = -1;
  int pslot = 0, pending_slot = 0;
  DCTS_STAMP_BEGIN();
  const long long nmaps = tb.total;
  if (m_cur < nmaps) {
    const float* first = tile_in(tb, m_cur);
#pragma unroll
    for (int it = 0; it < Stage::PIECES; ++it) Stage::piece_raw(first, 0, buf0, lane_in, ROLE, it);
  }

  // The direct-to-LDS loads of a strip are issued in four instalments spread over one whole step
  // (pass-1 butterflies and transform of the previous strip, then the dump and the butterflies of
  // the following pass-2 round): a wave stalls on such an instruction while the CU's memory queue
  // is full, and with all of a strip's loads in one phase every wave sat out that stall at the
  // phase's barrier (stamps: 4.8k of a step's 13k cycles) while the queue idled in the other four.
  auto issue = [&](const float* src, int strip, lds_ptr buf, auto slot) DCTS_LAMBDA_INLINE {
#pragma unroll
    for (int it = decltype(slot)::value; it < Stage::PIECES; it += 4)
      Stage::piece_raw(src, strip, buf, launder(lane_in), ROLE, it);
  };
  using Q0 = std::integral_constant<int, 0>;
  using Q1 = std::integral_constant<int, 1>;
  using Q2 = std::integral_constant<int, 2>;
  using Q3 = std::integral_constant<int, 3>;
  auto iteration = [&](auto par, auto hp, auto hc) DCTS_LAMBDA_INLINE {
    constexpr int PAR = decltype(par)::value;  // layout of the previous map; the current one gets 1 - PAR
    constexpr bool have_prev = decltype(hp)::value, have_cur = decltype(hc)::value;
    const float* in_b = tile_in(tb, have_cur ? m_cur : 0);
    float e = 0.f;
    dcts::static_for<T>([&](auto ir) DCTS_LAMBDA_INLINE {
      constexpr int r = decltype(ir)::value;
      constexpr int k = PAR * T + r;
      // The two buffers are separate __shared__ objects, statically selected: that is what lets the
      // compiler see that LDS reads of one do not alias direct-to-LDS loads in flight to the other.
      // With one array and offsets it put s_waitcnt vmcnt(0) in front of the first LDS access after
      // every such load: a full memory round trip per instalment.
      const lds_ptr dat = (k % 2) ? buf1 : buf0;  // strip r of the current map (landing / landed)
      const lds_ptr img = (k % 2) ? buf0 : buf1;  // pass-2 image of this step, then strip r+1
      if constexpr (have_prev) {
        DCTS_STAMP(12);
        lds_barrier();  // the strip that lived in img has been consumed by everyone
        DCTS_STAMP(0);
        if constexpr (r == 0) {
          if (pending_m >= 0) {
            fused_finish<M, L, S, ROLE>(partials, pending_slot, pending_m, tb, lane_in);
            pending_m = -1;
          }
        }
        if constexpr (have_cur) issue(in_b, r, dat, Q2{});
        int lane = launder(lane_in);
        // DCTS_DUMP_BALANCED written out: a value from the LDS park is read before the line test, not under it
        dcts::static_for<T>([&](auto is) DCTS_LAMBDA_INLINE {
          constexpr int s = decltype(is)::value;
          const int line = s * SW + lane;
          const int off = (line < N ? line : 0) * RW + ROLE * KPR;
          dcts::static_for<KPR>([&](auto ic) DCTS_LAMBDA_INLINE {
            constexpr int c = decltype(ic)::value;
            if constexpr (r * KPR + c < M) {
              constexpr int pi = Cfg::park_index(s, r * KPR + c);
              if constexpr (pi >= 0) {
                const float v = park[(s * Cfg::NP + pi) * (64 * S)];
                if (line < N) img[off + c] = v;
              } else {
                if (line < N) img[off + c] = pipe_slot<PAR, s, r * KPR + c>(P);
              }
            } else {
              if (line < N) img[off + c] = 0.f;  // padding column: contributes exactly zero energy
            }
          });
        });
        DCTS_STAMP(1);
        lds_barrier();
        DCTS_STAMP(2);
        if constexpr (have_cur) issue(in_b, r, dat, Q3{});
        lane = launder(lane_in);
        split_butterflies<M, L>(img, RW, true, lane, ROLE);
        DCTS_STAMP(3);
        lds_barrier();
        DCTS_STAMP(4);
        lane = launder(lane_in);
        DCTS_ROUND_TAIL(ROLE, false, img + lane, RW, true, 0, (float*)nullptr, 0, o, er)  // no coefficient instantiation
        asm volatile("" : "+v"(er));
        e += er;
        DCTS_STAMP(5);
      }
      if constexpr (have_cur) {
        DCTS_STAMP(12);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // my pieces of this strip have landed
        DCTS_STAMP(6);
        lds_barrier();                                   // ... everyone's; img has been consumed
        DCTS_STAMP(7);
        const bool more = (r + 1 < T) || (m_cur + gridDim.x < nmaps);
        const float* nsrc = (r + 1 < T || !more) ? in_b : tile_in(tb, m_cur + gridDim.x);
        constexpr int nstrip = (r + 1 < T) ? r + 1 : 0;
        // the step that transforms the next strip starts with a pass-2 round (which issues the other
        // two instalments) unless this is the first map of the workgroup
        constexpr bool next_has_p2 = have_prev || (r + 1 == T);
        if (more) {
          issue(nsrc, nstrip, img, Q0{});
          if constexpr (!next_has_p2) issue(nsrc, nstrip, img, Q2{});
        }
        int lane = launder(lane_in);
        const bool act = r * SW + lane < N;
        split_butterflies<M, L>(dat, SW, act, lane, ROLE);
        DCTS_STAMP(8);
        lds_barrier();
        DCTS_STAMP(9);
        if (more) {
          issue(nsrc, nstrip, img, Q1{});
          if constexpr (!next_has_p2) issue(nsrc, nstrip, img, Q3{});
        }
        lane = launder(lane_in);
        float o[M];
        split_role_transform<M, L, ROLE>(dat + (act ? lane : 0), SW, o);
        dcts::static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {
          constexpr int kk = decltype(ik)::value;
          // pin the codelet here: LLVM otherwise sinks its arithmetic down to the dump one map later
          // (the first use of the outputs) and keeps the inputs and half-finished temporaries alive
          constexpr int pi = Cfg::park_index(r, kk);
          if constexpr (pi >= 0) {
            park[(r * Cfg::NP + pi) * (64 * S)] = o[kk];
          } else {
            asm volatile("" : "+v"(o[kk]));
            pipe_slot<1 - PAR, r, kk>(P) = o[kk];
          }
        });
        DCTS_STAMP(10);
      }
    });
    if constexpr (have_prev) {
      e = wave_sum_dpp(e);
      if (lane_in == 0) partials[pslot * S + ROLE] = e;
      pending_m = m_prev;
      pending_slot = pslot;
      pslot ^= 1;
      DCTS_STAMP(11);
    }
    m_prev = have_cur ? m_cur : -1;
    m_cur += gridDim.x;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // every workgroup owns at least one map (grid <= nmaps): prologue, steady pairs, epilogue
  iteration(I0{}, std::false_type{}, std::true_type{});
  for (;;) {
    if (m_cur >= nmaps) {
      iteration(I1{}, std::true_type{}, std::false_type{});
      break;
    }
    iteration(I1{}, std::true_type{}, std::true_type{});
    if (m_cur >= nmaps) {
      iteration(I0{}, std::true_type{}, std::false_type{});
      break;
    }
    iteration(I0{}, std::true_type{}, std::true_type{});
  }
  if (pending_m >= 0) {
    lds_barrier();
    fused_finish<M, L, S, ROLE>(partials, pending_slot, pending_m, tb, lane_in);
  }
  DCTS_STAMP_END(ROLE, lane_in);
}

template <int M, int L, int... R>
__device__ __forceinline__ void pipe_dispatch(int role, const PlainMaps& tb, lds_ptr buf0, lds_ptr buf1, lds_ptr park,
                                              lds_ptr partials, int lane, std::integer_sequence<int, R...>) {
  ((role == R ? pipe_body<M, L, R>(tb, buf0, buf1, park, partials, lane) : (void)0), ...);
}

template <int M, int L>
__global__ __launch_bounds__((64 << L), (fused_waves_per_simd<M, L>())) void k_split_pipe(const float* __restrict__ x, long long map_stride,
                                                             long long nmaps, float* __restrict__ out) {
  const PlainMaps tb{x, out, map_stride, nmaps};
  using Cfg = PipeCfg<M, L>;
  __shared__ __attribute__((aligned(16))) float buf0[Cfg::BUF];
  __shared__ __attribute__((aligned(16))) float buf1[Cfg::BUF];
  __shared__ float park[Cfg::T * Cfg::NP * 64 * Cfg::S > 0 ? Cfg::T * Cfg::NP * 64 * Cfg::S : 1];
  __shared__ float partials[2 * Cfg::S];
  pipe_dispatch<M, L>(threadIdx.x >> 6, tb, (lds_ptr)buf0, (lds_ptr)buf1, (lds_ptr)park, (lds_ptr)partials,
                      threadIdx.x & 63, std::make_integer_sequence<int, Cfg::S>{});
}

template <int M, int L>
int launch_pipe(const TileBatch& tb, hipStream_t st) {  // one tensor per launch (PlainMaps)
  const long long cap = (long long)num_cus() * blocks_per_cu<k_split_pipe<M, L>, (1 << L)>();
  int rc = 0;
  for (int i = 0; i < tb.count && !rc; ++i) {
    const long long nm = tb.begin[i + 1] - tb.begin[i];
    const long long grid = nm < cap ? nm : cap;
    hipLaunchKernelGGL((k_split_pipe<M, L>), dim3((unsigned)grid), dim3(64 << L), 0, st, tb.x[i], tb.map_elems, nm,
                       tb.out[i]);
    rc = (int)hipGetLastError();
  }
  return rc;
}

}  // namespace

namespace dctsi {

int dispatch_pipe(int N, const TileBatch& tb, hipStream_t st) {
  DCTS_SWITCH_TABLE(DCTS_PIPE_TABLE, N,
                    [&](auto m, auto l) { return launch_pipe<decltype(m)::value, decltype(l)::value>(tb, st); })
}

}  // namespace dctsi
