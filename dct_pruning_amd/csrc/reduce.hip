// reduce.hip - the reductions that follow the energies: the batch sum and the running-mean update of the hook (one hook point
// or up to kMultiMax per launch), the weighted reduction over stored coefficients, and the PMC calibration read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "dcts_internal.h"
#include "grid_caps.h"

using namespace dctsi;

namespace {

// Batch sum over n of E[n][j] for a 32-channel strip per block: kSumSl = 16 n-slices run in parallel
// (slice s takes n = s, s+16, ...), partials are combined in slice order -> a fixed,
// launch-independent summation order (bit-reproducible, no atomics).
constexpr int kSumCh = 32, kSumSl = 16;
__device__ __forceinline__ float strip_batch_sum(const float* __restrict__ e, long long N,
                                                 long long C, long long j, int slice,
                                                 float (*part)[kSumCh]) {
  float s = 0.f;
  if (j < C) {
    long long n = slice;
    // sixteen loads in flight per lane and round trip (a batch of 256 samples is ONE round trip: the
    // kernel is pure latency, 3.8 us with four loads per trip); the additions keep their order
#pragma unroll 1
    for (; n + 15 * kSumSl < N; n += 16 * kSumSl) {
      float a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = e[(n + i * kSumSl) * C + j];
#pragma unroll
      for (int i = 0; i < 16; ++i) s += a[i];
    }
#pragma unroll 1
    for (; n + 3 * kSumSl < N; n += 4 * kSumSl) {
      const float a0 = e[n * C + j], a1 = e[(n + kSumSl) * C + j];
      const float a2 = e[(n + 2 * kSumSl) * C + j], a3 = e[(n + 3 * kSumSl) * C + j];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; n < N; n += kSumSl) s += e[n * C + j];
  }
  part[slice][threadIdx.x % kSumCh] = s;
  __syncthreads();
  float t = 0.f;
  if (slice == 0) {
#pragma unroll
    for (int i = 0; i < kSumSl; ++i) t += part[i][threadIdx.x % kSumCh];
  }
  return t;  // valid in slice 0
}

// out_c[j] = sum_n e[n*C + j]
__global__ __launch_bounds__(kSumCh * kSumSl) void k_batch_sum(const float* __restrict__ e, long long N,
                                                               long long C, float* __restrict__ out_c) {
  __shared__ float part[kSumSl][kSumCh];
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(e, N, C, j, slice, part);
  if (slice == 0 && j < C) out_c[j] = t;
}

// (fr * total + t) / (total + n) in the reference's three fp32 roundings: product, sum, quotient. Plain operators under
// contract(off), not __fadd_rn(__fmul_rn(..), ..): the HIP headers define those two as `*` and `+`, and once they are
// inlined the default -ffp-contract=fast turns the pair into one v_fmac_f32 - a single rounding, other bits than the
// reference's in about a tenth of the channels (tests/test_reduce_gpu.py compares the bits). The division stays correctly rounded.
__device__ __forceinline__ float mean_update(float fr, float total, float t, float n) {
#pragma clang fp contract(off)
  const float prod = fr * total;
  const float acc = prod + t;
  const float den = total + n;
  return __fdiv_rn(acc, den);
}

// fr[j] <- (fr[j] * total + sum_n e[n*C + j]) / (total + N): the running-mean update of
// utils/common.py:274-277 fused with the batch sum of :273 (same three fp32 roundings)
__global__ __launch_bounds__(kSumCh * kSumSl) void k_running_mean(const float* __restrict__ e, long long N,
                                                                  long long C, float* __restrict__ fr,
                                                                  float total) {
  __shared__ float part[kSumSl][kSumCh];
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(e, N, C, j, slice, part);
  if (slice == 0 && j < C) fr[j] = mean_update(fr[j], total, t, float(N));
}

// the same update for up to kMultiMax hook points in one launch (descriptors by value in the
// kernel arguments): blockIdx.y = hook point, blockIdx.x = 32-channel strip
struct UpdateBatch {
  dcts_update_desc d[kMultiMax];
};
__global__ __launch_bounds__(kSumCh * kSumSl) void k_running_mean_multi(UpdateBatch b) {
  __shared__ float part[kSumSl][kSumCh];
  const dcts_update_desc d = b.d[blockIdx.y];
  if ((long long)blockIdx.x * kSumCh >= d.C_count) return;  // whole block leaves together
  const int slice = threadIdx.x / kSumCh;
  const long long j = (long long)blockIdx.x * kSumCh + threadIdx.x % kSumCh;
  const float t = strip_batch_sum(d.energy_nc, d.N, d.C_count, j, slice, part);
  if (slice == 0 && j < d.C_count) d.feature_result[j] = mean_update(d.feature_result[j], d.total_before, t, float(d.N));
}

// Score variant in the coefficient domain: out[m] = sum_{u,v} weights[u,v] * coeff[m][u][v]^2.
// One wave per map over dense [HW] coefficient tiles; lanes stride the tile, fixed-order wave sum.
__global__ __launch_bounds__((64 * kReduceWaves)) void k_weighted_energy(const float* __restrict__ coeff, const float* __restrict__ weights,
                                                         long long nmaps, int hw, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long m = wave; m < nmaps; m += nwaves) {
    const float* c = coeff + m * hw;
    float e = 0.f;
    for (int i = lane; i < hw; i += 64) {
      const float v = c[i];
      e = fmaf(weights[i] * v, v, e);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
    if (lane == 0) out[m] = e;
  }
}

// PMC calibration aid: streams n floats with the codelet kernels' access width (one dword per
// lane, consecutive lanes consecutive addresses) so FETCH_SIZE can be compared with a known
// byte count in this exact pattern (MI355X_MICROARCH.md, HBM section: widths other than
// 16 B/lane are uncalibrated).
__global__ __launch_bounds__(256) void k_calib_read(const float* __restrict__ x, long long n,
                                                    float* __restrict__ sink) {
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    s += x[i];
  if (s == 123456.789f) sink[0] = s;  // keeps the loads alive without a store in practice
}

unsigned strips(long long C) { return (unsigned)((C + kSumCh - 1) / kSumCh); }

}  // namespace

namespace dctsi {

int launch_batch_sum(const float* e, long long N, long long C, float* out_c, hipStream_t st) {
  hipLaunchKernelGGL(k_batch_sum, dim3(strips(C)), dim3(kSumCh * kSumSl), 0, st, e, N, C, out_c);
  return (int)hipGetLastError();
}

int launch_running_mean(const float* e, long long N, long long C, float* fr, float total, hipStream_t st) {
  hipLaunchKernelGGL(k_running_mean, dim3(strips(C)), dim3(kSumCh * kSumSl), 0, st, e, N, C, fr, total);
  return (int)hipGetLastError();
}

int launch_running_mean_multi(const dcts_update_desc* descs, int n, long long cmax, hipStream_t st) {
  UpdateBatch b;
  for (int i = 0; i < kMultiMax; ++i) b.d[i] = descs[i < n ? i : 0];
  hipLaunchKernelGGL(k_running_mean_multi, dim3(strips(cmax), (unsigned)n), dim3(kSumCh * kSumSl), 0, st, b);
  return (int)hipGetLastError();
}

int launch_weighted_reduce(const float* coeff, const float* weights, long long nmaps, int hw, float* out, hipStream_t st) {
  const unsigned blocks = grid_blocks(nmaps, kReduceWaves, kReduceMaxBlocks);  // one wave per map
  hipLaunchKernelGGL(k_weighted_energy, dim3(blocks), dim3(64 * kReduceWaves), 0, st, coeff, weights, nmaps, hw, out);
  return (int)hipGetLastError();
}

int launch_stream_read(const float* x, long long n, float* sink, hipStream_t st) {
  hipLaunchKernelGGL(k_calib_read, dim3(256 * 32), dim3(256), 0, st, x, n, sink);
  return (int)hipGetLastError();
}

}  // namespace dctsi
