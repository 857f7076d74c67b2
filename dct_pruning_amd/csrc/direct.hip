// direct.hip - the cosine-matrix fallback: any (H, W) <= DCTS_MAX_EDGE, energies or coefficients.
//   k_basis           the orthonormal DCT-II matrix of one edge, built into the caller's workspace
//   k_energy_direct   separable cosine-matrix transform with the basis block staged in LDS; intermediate tile in a
//                     caller-provided workspace (L2-resident). O(H*W*(H+W)) flops per map: the correct fallback,
//                     compute-bound for large tiles. Two instantiations per output kind: ONE_BLOCK for tiles whose
//                     edges are at most kDirectBlock (every dot product one FMA chain), the other for all larger ones.
// Which calls build the tables and which reuse them is host policy: the memo of api.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "dcts_internal.h"

using namespace dctsi;

namespace {

// Bt[r*n + k] = s_k cos(pi (2r+1) k / (2n)), s_0 = sqrt(1/n), s_k = sqrt(2/n)
__global__ void k_basis(float* __restrict__ Bt, int n) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const int r = idx / n, k = idx - r * n;
  const long long num = ((long long)(2 * r + 1) * k) % (4LL * n);
  const double cv = cospi(double(num) / double(2 * n));
  const double s = (k == 0) ? sqrt(1.0 / double(n)) : sqrt(2.0 / double(n));
  Bt[idx] = float(cv * s);
}

constexpr int kDirectThreads = 256;
constexpr int kKB = 8;  // output rows per basis block
// Summation order (a function of the shape alone). A dot product is cut into blocks of kDirectBlock consecutive
// terms, each block one FMA chain in ascending order; kDirectGroup consecutive block sums are added in ascending order into a
// group sum, and the group sums in ascending order into the total (both from +0.0). A lane's squares: one chain per kDirectBlock
// output rows, the chains added in ascending order. An edge of at most kDirectBlock has one block, which is the single chain
// over the whole edge that this kernel ran at every edge before, bit for bit. That chain drifts where the terms have one sign: the
// basis function (128, 1) of a 512 x 3 map came out 1.08e-5 off against a bound of 3.8e-6, (0, 128) of 512 x 512 1.7e-5 against
// 1.9e-6. tests/direct_order.py is a numpy model of this order, tests/test_direct_order_cpu.py the record.
constexpr int kDirectBlock = 16;
constexpr int kDirectGroup = 4;
constexpr int kDirectGroupTerms = kDirectBlock * kDirectGroup;
static_assert(kDirectBlock % kKB == 0, "a block of output rows is a whole number of basis blocks");

// acc[kk] += v * b[kk] for the kKB output rows of one staged basis row
__device__ __forceinline__ void fma_row(float (&acc)[kKB], float v, const float* b) {
  const float4 b0 = *reinterpret_cast<const float4*>(b);
  const float4 b1 = *reinterpret_cast<const float4*>(b + 4);
  acc[0] = fmaf(v, b0.x, acc[0]);
  acc[1] = fmaf(v, b0.y, acc[1]);
  acc[2] = fmaf(v, b0.z, acc[2]);
  acc[3] = fmaf(v, b0.w, acc[3]);
  acc[4] = fmaf(v, b1.x, acc[4]);
  acc[5] = fmaf(v, b1.y, acc[5]);
  acc[6] = fmaf(v, b1.z, acc[6]);
  acc[7] = fmaf(v, b1.w, acc[7]);
}

// acc[kk] = sum_{i < n} load(i) * rows[i][kk], one FMA chain from +0.0 per output row. A whole block has a fixed trip count:
// its loads issue together, ahead of the FMAs that wait for them.
template <typename Load>
__device__ __forceinline__ void fma_chain(float (&acc)[kKB], const float (*rows)[kKB], int n, Load load) {
#pragma unroll
  for (int kk = 0; kk < kKB; ++kk) acc[kk] = 0.f;
  if (n == kDirectBlock) {
    float v[kDirectBlock];
#pragma unroll
    for (int i = 0; i < kDirectBlock; ++i) v[i] = load(i);
#pragma unroll
    for (int i = 0; i < kDirectBlock; ++i) fma_row(acc, v[i], rows[i]);
  } else {
    for (int i = 0; i < n; ++i) fma_row(acc, load(i), rows[i]);
  }
}

// tot[kk] = sum_{i < n} load(i) * rows[i][kk] in the order stated above. ONE_BLOCK: the caller knows that n <= kDirectBlock, and
// the kernel for small edges holds nothing but the plain chain (the same bits: 0 + 0 + acc).
template <bool ONE_BLOCK, typename Load>
__device__ __forceinline__ void dot_ordered(float (&tot)[kKB], const float (*rows)[kKB], int n, Load load) {
#pragma unroll
  for (int kk = 0; kk < kKB; ++kk) tot[kk] = 0.f;
  if constexpr (ONE_BLOCK) {
    for (int i = 0; i < n; ++i) fma_row(tot, load(i), rows[i]);
    return;
  }
  for (int g0 = 0; g0 < n; g0 += kDirectGroupTerms) {
    const int gend = min(g0 + kDirectGroupTerms, n);
    float grp[kKB];
#pragma unroll
    for (int kk = 0; kk < kKB; ++kk) grp[kk] = 0.f;
    for (int b0 = g0; b0 < gend; b0 += kDirectBlock) {
      float acc[kKB];
      fma_chain(acc, rows + b0, min(gend - b0, kDirectBlock), [&](int i) { return load(b0 + i); });
#pragma unroll
      for (int kk = 0; kk < kKB; ++kk) grp[kk] += acc[kk];  // (0 + acc keeps the bits of acc, but for -0.0)
    }
#pragma unroll
    for (int kk = 0; kk < kKB; ++kk) tot[kk] += grp[kk];
  }
}

template <bool STORE_COEFF, bool ONE_BLOCK>
__global__ __launch_bounds__(kDirectThreads) void k_energy_direct(
    MapGeom g, int pad, const float* __restrict__ CHt, const float* __restrict__ CWt,
    float* __restrict__ T, float* __restrict__ out) {
  const int HP = g.H + pad, WP = g.W + pad;
  __shared__ __attribute__((aligned(16))) float Bs[DCTS_MAX_EDGE][kKB];
  __shared__ float red[kDirectThreads / 64];
  const int tid = threadIdx.x;
  float* Tm = T + (size_t)blockIdx.x * HP * WP;

  for (long long m = blockIdx.x; m < g.nmaps; m += gridDim.x) {
    const float* xm = map_base(g, m);
    // ---- phase 1: Tm[k][c] = sum_r CH[k][r] x'[r][c] --------------------------------
    for (int k0 = 0; k0 < HP; k0 += kKB) {
      __syncthreads();
      for (int i = tid; i < HP * kKB; i += kDirectThreads) {
        const int r = i / kKB, kk = i - r * kKB;
        Bs[r][kk] = (k0 + kk < HP) ? CHt[r * HP + k0 + kk] : 0.f;
      }
      __syncthreads();
      for (int c = tid; c < WP; c += kDirectThreads) {
        float tot[kKB];
        if (c >= pad) {  // the padded tile's row in front is zero and skipped: the term count stays wave-uniform
          const float* col = xm + (c - pad);
          dot_ordered<ONE_BLOCK>(tot, Bs + pad, HP - pad, [&](int i) { return col[(long long)i * g.strideH]; });
        } else {  // the column in front is zero
#pragma unroll
          for (int kk = 0; kk < kKB; ++kk) tot[kk] = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk)
          if (k0 + kk < HP) Tm[(k0 + kk) * WP + c] = tot[kk];
      }
    }
    // ---- phase 2: Y[k][l] = sum_c Tm[k][c] CW[l][c]; energy += Y^2 --------------------
    float e = 0.f, eb = 0.f;  // this lane's squares: the rows of the block so far, and the blocks before it
    for (int k0 = 0; k0 < HP; k0 += kKB) {
      if constexpr (!ONE_BLOCK) {
        if (k0 % kDirectBlock == 0) {
          e += eb;  // (eb is a sum of squares, never -0.0: 0 + eb keeps its bits)
          eb = 0.f;
        }
      }
      __syncthreads();  // also orders phase-1 global stores before these loads (same CU)
      for (int i = tid; i < WP * kKB; i += kDirectThreads) {
        const int cc = i / kKB, kk = i - cc * kKB;
        Bs[cc][kk] = (k0 + kk < HP) ? Tm[(k0 + kk) * WP + cc] : 0.f;
      }
      __syncthreads();
      for (int l = tid; l < WP; l += kDirectThreads) {
        float tot[kKB];
        dot_ordered<ONE_BLOCK>(tot, Bs, WP, [&](int i) { return CWt[i * WP + l]; });
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) {
          if (k0 + kk < HP) {
            if constexpr (STORE_COEFF)
              out[(m * HP + k0 + kk) * WP + l] = tot[kk];
            else
              eb = fmaf(tot[kk], tot[kk], eb);
          }
        }
      }
    }
    if constexpr (!STORE_COEFF) {
      e += eb;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) e += __shfl_down(e, off, 64);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = e;
      __syncthreads();
      if (tid == 0) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kDirectThreads / 64; ++i) s += red[i];
        out[m] = s;
      }
    }
  }
}

constexpr int kDirectGridCap = 512;

}  // namespace

namespace dctsi {

DirectWs direct_ws(long long nmaps, int HP, int WP) {
  DirectWs w;
  w.grid = (int)(nmaps < kDirectGridCap ? (nmaps > 0 ? nmaps : 1) : kDirectGridCap);
  w.off_ch = 0;
  w.off_cw = align_up(w.off_ch + (size_t)HP * HP * 4, 256);
  w.off_t = align_up(w.off_cw + (size_t)WP * WP * 4, 256);
  w.total = align_up(w.off_t + (size_t)w.grid * HP * WP * 4, 256);
  return w;
}

int launch_basis(float* CHt, int HP, float* CWt, int WP, hipStream_t st) {
  hipLaunchKernelGGL(k_basis, dim3((unsigned)((HP * HP + 255) / 256)), dim3(256), 0, st, CHt, HP);
  hipLaunchKernelGGL(k_basis, dim3((unsigned)((WP * WP + 255) / 256)), dim3(256), 0, st, CWt, WP);
  return (int)hipGetLastError();
}

int dispatch_direct(int store, int pad, const MapGeom& g, int grid, const float* CHt, const float* CWt, float* T, float* out,
                    hipStream_t st) {
  const bool one = g.H + pad <= kDirectBlock && g.W + pad <= kDirectBlock;  // every dot product is one block
  auto kernel = store ? (one ? k_energy_direct<true, true> : k_energy_direct<true, false>)
                      : (one ? k_energy_direct<false, true> : k_energy_direct<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kDirectThreads), 0, st, g, pad, CHt, CWt, T, out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
