// rank.hip - the HRank criterion: numerical rank of every feature map (dcts_rank_f32, include/dctscore.h).
//
// Replaces the per-map Python loop  torch.linalg.matrix_rank(output[i, j])  that HRank's hooks run (the reference
// keeps it as the commented alternative of utils/common.py:268). Contract: rank(A) = #{ sigma_i > max(H, W) * 2^-23 *
// sigma_max } over the exact singular values of the fp32 map (torch.linalg.matrix_rank's default rule for fp32); an
// all-zero map has rank 0.
//
// Arithmetic, all fp64 ("rank criterion"):
//   1. Gram matrix S = a_i . a_j of the n = min(H, W) vectors along the short side (length m = max(H, W)). fp32 -> fp64
//      is exact and so is every fp32 x fp32 product, so S carries only the summation error, about n^2 * 1e-16 *
//      sigma_max^2: ~1 % of tau^2 = (m * 2^-23 * sigma_max)^2, the threshold the eigenvalues sigma_i^2 are compared with.
//   2. Householder tridiagonalisation of S (n - 2 steps).
//   3. lambda_max by multisection: every lane of the group evaluates one Sturm count per round, so a round narrows the
//      bracket [max d_i, Gershgorin bound] (a factor <= 3 wide) by G + 1; a fixed number of rounds gives 2^-44.
//   4. One Sturm count at tau^2 = m^2 * 2^-46 * lambda_max: rank = n - #{lambda <= tau^2}.
// Every loop has a bound fixed by the shape; nothing iterates to convergence. A map with NaN / Inf gets some value in
// [0, n] and touches nothing but its own output.
//
// Layout: a group of G lanes (G = 4 ... 64, the smallest power of two >= n) owns one map; lane l owns row l of S. A
// workgroup is ONE wave holding 64 / G groups, so small maps (ResNet-50's 7 x 7: hundreds of thousands of them) run 8
// or 16 to a wave. The map (fp32, row stride W | 1) and S (row stride n | 1) live in the group's LDS slab; reductions
// are xor shuffles inside the group, whose result is the same in every lane and independent of where in the wave
// the group sits: a map's rank does not depend on which maps share its launch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dctscore.h"
#include "grid_caps.h"

namespace {

struct RankGeom {
  const float* x;
  float* out;
  int64_t maps;  // N * c_count; map q = n * c_count + j
  int64_t strideN, strideC, strideH;
  int32_t c_begin, c_count;
  int32_t H, W, n, m;
  int32_t ldS, ldA;  // row strides of S (doubles) and of the map image (floats)
  int32_t slab;      // doubles of LDS per group
};

template <int G>
__device__ inline double group_sum(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int G>
__device__ inline double group_max(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

template <int G>
__device__ inline double group_min(double v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}

// #{eigenvalues of the tridiagonal (d, e) <= s}; e2[i] = e_i^2. A pivot smaller than pivmin counts as negative.
__device__ inline int sturm_count(const double* d, const double* e2, int n, double s, double pivmin) {
  double q = d[0] - s;
  if (fabs(q) < pivmin) q = -pivmin;
  int c = q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = (d[i] - s) - e2[i - 1] / q;
    if (fabs(q) < pivmin) q = -pivmin;
    c += q < 0.0;
  }
  return c;
}

// multisection rounds: (G + 1)^R >= 2^44
template <int G>
constexpr int rounds() {
  return G == 4 ? 19 : G == 8 ? 14 : G == 16 ? 11 : G == 32 ? 9 : 8;
}

template <int G>
__global__ __launch_bounds__(64) void k_rank(RankGeom g) {
  extern __shared__ double lds[];
  constexpr int MPW = 64 / G;
  const int lane = threadIdx.x;
  const int grp = lane / G, l = lane % G, gbase = lane - l;
  const int n = g.n, m = g.m, H = g.H, W = g.W, ldS = g.ldS, ldA = g.ldA;
  double* S = lds + (size_t)grp * g.slab;
  double* vb = S + (size_t)n * ldS;  // [G]: Householder vector, then the diagonal d
  double* wb = vb + G;               // [G]: p - K v, then e^2
  float* A = reinterpret_cast<float*>(wb + G);
  const bool row = l < n;

  for (int64_t base = (int64_t)blockIdx.x * MPW; base < g.maps; base += (int64_t)gridDim.x * MPW) {
    const int64_t q = base + grp;
    const bool live = q < g.maps;

    // 1. the map into LDS (dead groups of the last round score zeros)
    if (live) {
      const int64_t ni = q / g.c_count;
      const int64_t ch = g.c_begin + (q - ni * g.c_count);
      const float* src = g.x + ni * g.strideN + ch * g.strideC;
      for (int e = l; e < H * W; e += G) {
        const int h = e / W, w = e - h * W;
        A[h * ldA + w] = src[h * g.strideH + w];
      }
    } else {
      for (int e = l; e < H * W; e += G) {
        const int h = e / W, w = e - h * W;
        A[h * ldA + w] = 0.0f;
      }
    }
    __syncthreads();

    // 2. Gram matrix over the long side: lane l computes row l
    if (row) {
      for (int j = 0; j < n; ++j) {
        double acc = 0.0;
        if (H <= W) {
          const float* ai = A + l * ldA;
          const float* aj = A + j * ldA;
          for (int t = 0; t < m; ++t) acc = fma((double)ai[t], (double)aj[t], acc);
        } else {
          for (int t = 0; t < m; ++t) acc = fma((double)A[t * ldA + l], (double)A[t * ldA + j], acc);
        }
        S[l * ldS + j] = acc;
      }
    }
    __syncthreads();

    // 3. Householder tridiagonalisation; step k zeroes column k below the subdiagonal and leaves alpha there.
    // The column is divided by its largest magnitude first (LAPACK dlarfg): once a rank-deficient map's trailing
    // block is down to round-off, its entries can be small enough for their squares to underflow.
    for (int k = 0; k < n - 2; ++k) {
      const bool act = row && l > k;
      const double xraw = act ? S[l * ldS + k] : 0.0;
      const double scale = group_max<G>(fabs(xraw));
      const double xl = scale > 0.0 ? xraw / scale : 0.0;
      const double x0 = __shfl(xl, gbase + k + 1, 64);
      const double nrm2 = group_sum<G>(xl * xl);  // in [1, n] unless the column is zero
      const double nrm = sqrt(nrm2);
      const double alpha = x0 >= 0.0 ? -nrm : nrm;
      const double vl = (l == k + 1) ? xl - alpha : xl;
      const double vtv = 2.0 * (nrm2 + fabs(x0) * nrm);  // |v|^2, no cancellation
      const double beta = vtv > 0.0 ? 2.0 / vtv : 0.0;
      vb[l] = vl;
      __syncthreads();
      double pl = 0.0;
      if (act) {
        for (int j = k + 1; j < n; ++j) pl = fma(S[l * ldS + j], vb[j], pl);
        pl *= beta;
      }
      const double K = 0.5 * beta * group_sum<G>(vl * pl);
      const double wl = pl - K * vl;
      wb[l] = wl;
      __syncthreads();
      if (act) {
        for (int j = k + 1; j < n; ++j) S[l * ldS + j] -= vl * wb[j] + wl * vb[j];
        if (l == k + 1) S[l * ldS + k] = alpha * scale;
      }
      __syncthreads();
    }

    // 4. the tridiagonal (d, e^2) into vb / wb; bracket of lambda_max: [max d_i, max Gershgorin bound]
    double dl = 0.0, el = 0.0, ep = 0.0;
    if (row) {
      dl = S[l * ldS + l];
      el = l + 1 < n ? S[(l + 1) * ldS + l] : 0.0;
      ep = l > 0 ? S[l * ldS + l - 1] : 0.0;
    }
    vb[l] = dl;
    wb[l] = el * el;
    const double upper = group_max<G>(row ? dl + fabs(el) + fabs(ep) : 0.0);
    double lo = group_max<G>(row ? dl : 0.0), hi = upper;
    const double pivmin = DBL_MIN * fmax(1.0, group_max<G>(el * el));
    __syncthreads();

    for (int r = 0; r < rounds<G>(); ++r) {
      const double s = lo + (hi - lo) * ((double)(l + 1) / (double)(G + 1));
      const bool above = sturm_count(vb, wb, n, s, pivmin) == n;  // lambda_max <= s
      hi = group_min<G>(above ? s : hi);
      lo = group_max<G>(above ? lo : s);
    }
    const double lmax = 0.5 * (lo + hi);
    const double tau2 = (double)m * (double)m * 0x1p-46 * lmax;
    int rank = n - sturm_count(vb, wb, n, tau2, pivmin);
    if (!(upper > 0.0)) rank = 0;  // all-zero map (and NaN maps)
    if (live && l == 0) g.out[q] = (float)rank;
    __syncthreads();
  }
}

template <int G>
int launch(RankGeom g, hipStream_t st) {
  constexpr int MPW = 64 / G;
  const int64_t tasks = (g.maps + MPW - 1) / MPW;
  const int blocks = (int)(tasks < dctsi::kRankMaxBlocks ? tasks : dctsi::kRankMaxBlocks);  // grid-stride beyond (grid_caps.h)
  const size_t lds = (size_t)MPW * g.slab * sizeof(double);
  hipLaunchKernelGGL((k_rank<G>), dim3(blocks), dim3(64), lds, st, g);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DCTS_OK : (int)e;
}

}  // namespace

extern "C" int dcts_rank_f32(const float* x, int64_t N, int64_t C_total, int64_t H, int64_t W, int64_t strideN,
                             int64_t strideC, int64_t strideH, int64_t strideW, int32_t c_begin, int32_t c_count,
                             float* out_nc, void* stream) {
  if (!x || !out_nc) return DCTS_E_NULL;
  if (N <= 0 || C_total <= 0 || H <= 0 || W <= 0 || H > DCTS_MAX_EDGE || W > DCTS_MAX_EDGE) return DCTS_E_SHAPE;
  if (c_count <= 0 || c_begin < 0 || (int64_t)c_begin + c_count > C_total) return DCTS_E_CHANNELS;
  if (strideW != 1 || strideH < W) return DCTS_E_STRIDE;
  if (H > DCTS_RANK_MAX_EDGE || W > DCTS_RANK_MAX_EDGE) return DCTS_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(out_nc) & 3)) return DCTS_E_ALIGN;
  if (N * (int64_t)c_count >= (1LL << 40)) return DCTS_E_SHAPE;

  RankGeom g;
  g.x = x;
  g.out = out_nc;
  g.maps = N * (int64_t)c_count;
  g.strideN = strideN;
  g.strideC = strideC;
  g.strideH = strideH;
  g.c_begin = c_begin;
  g.c_count = c_count;
  g.H = (int32_t)H;
  g.W = (int32_t)W;
  g.n = (int32_t)(H < W ? H : W);
  g.m = (int32_t)(H < W ? W : H);
  g.ldS = g.n | 1;  // odd strides: lane l's row l spreads over the banks
  g.ldA = g.W | 1;
  int G = 4;
  while (G < g.n) G *= 2;
  g.slab = g.n * g.ldS + 2 * G + (g.H * g.ldA + 1) / 2;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (G) {
    case 4: return launch<4>(g, st);
    case 8: return launch<8>(g, st);
    case 16: return launch<16>(g, st);
    case 32: return launch<32>(g, st);
    default: return launch<64>(g, st);
  }
}
