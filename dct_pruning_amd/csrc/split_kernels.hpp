// split_kernels.hpp - the two-launch split kernels (k_pass1d, k_split_reduce) and their launcher. Instantiated by
// split.hip and split_more.hip, one half of DCTS_SPLIT_TABLE each, so that the two halves compile in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

#include "dcts_internal.h"
#include "split_common.hpp"

namespace {

// ---------------------------------------------------------------------------------------
// split family: tiles whose edge N = 2^L * M is too long for one lane's registers
// ---------------------------------------------------------------------------------------
// The top L radix-2 levels of the codelet recursion (dct_codelets.hpp) are unrolled across
// 2^L "role" waves instead of inside a lane; each role runs an M-point codelet on a length-M
// input it gathers from 2^L mirrored samples. The role tree, with y the input of a node:
//   DCT-II node (length n):  child 0 = DCT-II(n/2) of y[j] + y[n-1-j]
//                            child 1 = DCT-IV(n/2) of y[j] - y[n-1-j]
//   DCT-IV node (length n):  child 0 = DCT-II(n/2) of  y[j] cos(b_j) + y[n-1-j] sin(b_j)
//                            child 1 = DCT-II(n/2) of (-1)^j (y[n-1-j] cos(b_j) - y[j] sin(b_j)),
//                            b_j = (2j+1) pi / (4n); outputs A (child 0), B (child 1)
// A DCT-II node's outputs are its children's, interleaved (exact). A DCT-IV node's outputs are
// X[0] = A[0], X[n-1] = -B[0], X[2j] = A[j] + B[n/2-j], X[2j-1] = A[j] - B[n/2-j]: that last
// add/sub layer is a rotation of each pair scaled by sqrt(2); the energy kernels fuse it into the
// reduction, (a+b)^2 + (a-b)^2 = 2a^2 + 2b^2, i.e. A[j], B[j] (j > 0) are carried with weight
// sqrt(2) (SplitNode::wt). Every other butterfly, rotation and twiddle is computed.
//
// k_pass1d transforms the row axis of In[b][n][line] (lines contiguous): one workgroup per
// (<= 64-line strip), one wave per role; the strip is staged once with direct-to-LDS loads and
// every role wave gathers its mirrored rows from LDS. Non-final pass: the result goes to
// T[b][line][role*M + k] through a per-wave LDS transpose (coalesced stores), so the second launch
// of the same kernel transforms the other axis. Final pass: squares are reduced per wave into
// partial sums which k_split_reduce adds in fixed order.

template <int M, int L>
struct SplitCfg {
  static constexpr int N = M << L;
  static constexpr int ROLES = 1 << L;
  static constexpr int STRIPS = (N + 63) / 64;
  // lines per strip: 64 when rows are whole 128-byte lines (N % 32 == 0), so every staged row
  // segment is two aligned cache lines (56-column strips of a 224-wide tile straddled lines:
  // PMC showed 1.43x read over-fetch); otherwise balanced strips, multiple of 4
  static constexpr int SW = (N % 32 == 0) ? 64 : (((N + STRIPS - 1) / STRIPS) + 3) / 4 * 4;
  static constexpr int SWP = SW | 1;                                    // odd LDS stride for the transpose
  static constexpr int IN_LDS = N * SW;                                 // floats: the staged input strip
  static constexpr int TR_LDS = ROLES * M * SWP;                        // floats: per-wave transpose slabs
  static constexpr int LDS_NONFINAL = IN_LDS > TR_LDS ? IN_LDS : TR_LDS;
};

// register budget (waves/SIMD): the role waves only hold an M-point codelet
template <int M>
constexpr int split_waves_per_simd() { return M <= 32 ? 4 : (M <= 48 ? 3 : 2); }

template <int M, int L, int ROLE, bool FINAL>
__device__ __forceinline__ void split_wave(lds_cptr lds_in, float* __restrict__ t_b, lds_ptr lds_tr,
                                           int strip, int lane, float* part) {
  using Cfg = SplitCfg<M, L>;
  constexpr int N = Cfg::N, SW = Cfg::SW, SWP = Cfg::SWP;
  const int line = strip * SW + lane;
  const bool act = lane < SW && line < N;
  float out[M];
  split_role_transform<M, L, ROLE>(lds_in + (act ? lane : 0), SW, out);
  if constexpr (FINAL) {
    float e = 0.f;
    dcts::static_for<M>([&](auto i) DCTS_LAMBDA_INLINE {
      constexpr int k = decltype(i)::value;
      e = fmaf(out[k], out[k], e);
    });
    if (!act) e = 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
    if (lane == 0) *part = e;
  } else {
    __syncthreads();  // every wave has consumed the staged strip: its LDS becomes the transpose slabs
    lds_ptr my = lds_tr + ROLE * (M * SWP);
    if (act) {
      dcts::static_for<M>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(i)::value;
        my[k * SWP + lane] = out[k];
      });
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int nl = (N - strip * SW) < SW ? (N - strip * SW) : SW;
#pragma unroll
    for (int k0 = 0; k0 < M; k0 += 64) {  // M may exceed the 64 lanes of a wave
      const int k = k0 + lane;
      if (k < M) {
        float* dst = t_b + (long long)(strip * SW) * N + ROLE * M + k;
        lds_cptr src = my + k * SWP;
#pragma unroll 4
        for (int j = 0; j < nl; ++j) {
          *dst = src[j];
          dst += N;
        }
      }
    }
  }
}

template <int M, int L, bool FINAL, int... R>
__device__ __forceinline__ void split_dispatch(int role, lds_cptr lds_in, float* t_b, lds_ptr lds_tr,
                                               int strip, int lane, float* part,
                                               std::integer_sequence<int, R...>) {
  // exactly one branch is taken per wave (role is wave-uniform); every branch reaches the
  // barrier inside split_wave, so the workgroup stays in step
  ((role == R ? split_wave<M, L, R, FINAL>(lds_in, t_b, lds_tr, strip, lane, part) : (void)0), ...);
}

// grid.x = nmaps_in_launch * STRIPS; block = 2^L waves.
//  1. the strip In[b][0..N)[strip*SW .. +SW) is staged into LDS by direct-to-LDS loads
//     (global_load_lds_dwordx4: no VGPRs, the whole N*SW*4-byte strip in flight at once);
//  2. role butterflies, in place in LDS: wave w takes the samples p = w, w + 2^L, ... of every
//     line (lane = line): 2^L reads, L*2^(L-1) butterflies/rotations, 2^L writes per (p, line);
//  3. wave r = role r: reads its M inputs (one contiguous segment of rows), M-point codelet,
//     then the transposed store or the energy reduction.
template <int M, int L, bool FINAL>
__global__ __launch_bounds__((64 << L), (split_waves_per_simd<M>())) void k_pass1d(
    const float* __restrict__ in, long long in_map_stride, float* __restrict__ t, float* __restrict__ partial) {
  using Cfg = SplitCfg<M, L>;
  constexpr int N = Cfg::N, SW = Cfg::SW, THREADS = 64 << L, S = Cfg::ROLES;
  __shared__ __attribute__((aligned(16))) float lds[FINAL ? Cfg::IN_LDS : Cfg::LDS_NONFINAL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long b = blockIdx.x / Cfg::STRIPS;
  const int strip = blockIdx.x - (int)(b * Cfg::STRIPS);
  const float* in_b = in + b * in_map_stride;

  constexpr int NQUADS = N * SW / 4;
  constexpr int ITERS = (NQUADS + THREADS - 1) / THREADS;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int qbase = it * THREADS + wave * 64;  // wave-uniform
    const int q = qbase + lane;
    const int e = 4 * q;
    const int row = e / SW, col = e - row * SW;
    if (q < NQUADS && strip * SW + col < N) {
      const float* g = in_b + (long long)row * N + strip * SW + col;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                       (__attribute__((address_space(3))) void*)(lds + 4 * qbase), 16, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const lds_ptr lds3 = (lds_ptr)lds;
  split_butterflies<M, L, NoHook, true>(lds3, SW, lane < SW, lane, wave);
  __syncthreads();

  float* t_b = FINAL ? nullptr : t + b * (long long)N * N;
  float* part = partial + (long long)blockIdx.x * Cfg::ROLES + wave;
  split_dispatch<M, L, FINAL>(wave, lds3, t_b, lds3, strip, lane, part,
                              std::make_integer_sequence<int, Cfg::ROLES>{});
}

// out[b] = scale * sum of the map's ROLES*STRIPS partials, fixed order
__global__ void k_split_reduce(const float* __restrict__ partial, int per_map, long long nmaps,
                               float scale, float* __restrict__ out) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nmaps) return;
  float s = 0.f;
  for (int i = 0; i < per_map; ++i) s += partial[b * per_map + i];
  out[b] = s * scale;
}

template <int M, int L>
int launch_split(const dctsi::MapGeom& g, float* out, void* workspace, hipStream_t st) {
  using Cfg = SplitCfg<M, L>;
  constexpr int N = Cfg::N;
  const dctsi::SplitWs ws = dctsi::split_ws(g.nmaps, N);
  char* wsp = reinterpret_cast<char*>(workspace);
  float* T = reinterpret_cast<float*>(wsp + ws.off_t);
  float* part = reinterpret_cast<float*>(wsp + ws.off_part);
  const float* x0 = g.x + (long long)g.c_begin * g.strideC;
  const float scale = float(4.0 / (double(N) * double(N)));
  for (long long m0 = 0; m0 < g.nmaps; m0 += ws.chunk_maps) {
    const long long nb = (g.nmaps - m0) < ws.chunk_maps ? (g.nmaps - m0) : ws.chunk_maps;
    const unsigned grid = (unsigned)(nb * Cfg::STRIPS);
    hipLaunchKernelGGL((k_pass1d<M, L, false>), dim3(grid), dim3(64 << L), 0, st, x0 + m0 * g.strideC,
                       g.strideC, T, part);
    hipLaunchKernelGGL((k_pass1d<M, L, true>), dim3(grid), dim3(64 << L), 0, st, T, (long long)N * N,
                       (float*)nullptr, part);
    hipLaunchKernelGGL(k_split_reduce, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, part,
                       Cfg::STRIPS * Cfg::ROLES, nb, scale, out + m0);
  }
  return (int)hipGetLastError();
}

}  // namespace
