// direct.hip - the cosine-matrix fallback: any (H, W) <= DCTS_MAX_EDGE, energies or coefficients.
//   k_basis           the orthonormal DCT-II matrix of one edge, built into the caller's workspace
//   k_energy_direct   separable cosine-matrix transform with the basis block staged in LDS; intermediate tile in a
//                     caller-provided workspace (L2-resident). O(H*W*(H+W)) flops per map: the correct fallback,
//                     compute-bound for large tiles.
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

template <bool STORE_COEFF>
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
        float acc[kKB];
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) acc[kk] = 0.f;
        if (c >= pad) {
          const float* col = xm + (c - pad);
          for (int r = pad; r < HP; ++r) {
            const float xv = col[(long long)(r - pad) * g.strideH];
            const float4 b0 = *reinterpret_cast<const float4*>(&Bs[r][0]);
            const float4 b1 = *reinterpret_cast<const float4*>(&Bs[r][4]);
            acc[0] = fmaf(xv, b0.x, acc[0]);
            acc[1] = fmaf(xv, b0.y, acc[1]);
            acc[2] = fmaf(xv, b0.z, acc[2]);
            acc[3] = fmaf(xv, b0.w, acc[3]);
            acc[4] = fmaf(xv, b1.x, acc[4]);
            acc[5] = fmaf(xv, b1.y, acc[5]);
            acc[6] = fmaf(xv, b1.z, acc[6]);
            acc[7] = fmaf(xv, b1.w, acc[7]);
          }
        }
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk)
          if (k0 + kk < HP) Tm[(k0 + kk) * WP + c] = acc[kk];
      }
    }
    // ---- phase 2: Y[k][l] = sum_c Tm[k][c] CW[l][c]; energy += Y^2 --------------------
    float e = 0.f;
    for (int k0 = 0; k0 < HP; k0 += kKB) {
      __syncthreads();  // also orders phase-1 global stores before these loads (same CU)
      for (int i = tid; i < WP * kKB; i += kDirectThreads) {
        const int cc = i / kKB, kk = i - cc * kKB;
        Bs[cc][kk] = (k0 + kk < HP) ? Tm[(k0 + kk) * WP + cc] : 0.f;
      }
      __syncthreads();
      for (int l = tid; l < WP; l += kDirectThreads) {
        float acc[kKB];
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) acc[kk] = 0.f;
        for (int cc = 0; cc < WP; ++cc) {
          const float wv = CWt[cc * WP + l];
          const float4 b0 = *reinterpret_cast<const float4*>(&Bs[cc][0]);
          const float4 b1 = *reinterpret_cast<const float4*>(&Bs[cc][4]);
          acc[0] = fmaf(wv, b0.x, acc[0]);
          acc[1] = fmaf(wv, b0.y, acc[1]);
          acc[2] = fmaf(wv, b0.z, acc[2]);
          acc[3] = fmaf(wv, b0.w, acc[3]);
          acc[4] = fmaf(wv, b1.x, acc[4]);
          acc[5] = fmaf(wv, b1.y, acc[5]);
          acc[6] = fmaf(wv, b1.z, acc[6]);
          acc[7] = fmaf(wv, b1.w, acc[7]);
        }
#pragma unroll
        for (int kk = 0; kk < kKB; ++kk) {
          if (k0 + kk < HP) {
            if constexpr (STORE_COEFF)
              out[(m * HP + k0 + kk) * WP + l] = acc[kk];
            else
              e = fmaf(acc[kk], acc[kk], e);
          }
        }
      }
    }
    if constexpr (!STORE_COEFF) {
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
  hipLaunchKernelGGL(store ? k_energy_direct<true> : k_energy_direct<false>, dim3((unsigned)grid), dim3(kDirectThreads), 0, st,
                     g, pad, CHt, CWt, T, out);
  return (int)hipGetLastError();
}

}  // namespace dctsi
