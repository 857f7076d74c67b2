// dct_codelets.hpp — straight-line, register-resident 1-D DCT-II codelets.
//
// One lane transforms a whole length-N vector held in its own VGPRs: no cross-lane
// traffic, no LDS, every twiddle an instruction literal. The kernels in
// codelet.hip run one such codelet per lane along H, transpose the tile through
// LDS, and run a second one along W.
//
// What is computed (the unnormalised DCT-II; the orthonormal scaling of
// torch_dct.dct(norm='ortho') — SURVEY.md Appendix B step 4, reference call site
// utils/common.py:267 — is applied by the caller):
//
//     X[k] = sum_{n<N} x[n] * cos(pi * (2n+1) * k / (2N)),     k = 0..N-1
//
// Factorisation (any N = 2^s * m, m odd):
//   even N : u[n] = x[n] + x[N-1-n], v[n] = x[n] - x[N-1-n]  (n < N/2)
//            X[2k]   = DCT-II_{N/2}(u)[k]
//            X[2k+1] = DCT-IV_{N/2}(v)[k]
//   DCT-IV_M, M even, M1 = M/2, beta_n = (2n+1)pi/(4M):
//            a[n] =          v[n] cos(beta_n) + v[M-1-n] sin(beta_n)
//            b[n] = (-1)^n (-v[n] sin(beta_n) + v[M-1-n] cos(beta_n))
//            A = DCT-II_{M1}(a), B = DCT-II_{M1}(b)
//            X[0] = A[0], X[M-1] = -B[0],
//            X[2j] = A[j] + B[M1-j], X[2j-1] = A[j] - B[M1-j]   (0 < j < M1)
//            (rotations are orthogonal and the tail is add/sub only: numerically stable)
//   odd N  : direct, using the x[n] <-> x[N-1-n] symmetry (about N^2/2 FMAs)
//   DCT-IV odd M >= 5 : with a = 2n+1, b = 2k+1 and gcd(8, M) = 1 the angle splits (CRT):
//            pi a b / (4M) = t pi/4 + 2 pi n' k' / M  (mod 2 pi),
//            n' = a mod M, k' = (8^-1 mod M) b mod M, t = a b (M^-1 mod 8) mod 8 (odd),
//            cos(phi + t pi/4) = (chi_c(t) cos phi - chi_s(t) sin phi) / sqrt 2, chi_c, chi_s = +-1 and
//            multiplicative in t. With pc[n'] = chi_c(a) v[n], ps[n'] = chi_s(a) v[n], u = M^-1 mod 8:
//            X[k] = chi_c(b) chi_c(u) C[k'] - chi_s(b) chi_s(u) S[k'],
//            C[k'] = sum pc[n'] cos(2 pi n' k'/M) / sqrt 2,  S[k'] = sum ps[n'] sin(2 pi n' k'/M) / sqrt 2.
//            C[M-k'] = C[k'], S[M-k'] = -S[k'], S[0] = 0: pre-sums pc[j] + pc[M-j], ps[j] - ps[M-j],
//            rows k' = 0..(M-1)/2 only, one add or sub per output: about M^2/2 (M = 7: 34 against 49).
//            Signs and permutations are compile-time: add/sub choices and literals.
//   DCT-IV M = 3 : direct 3 x 3 (the split form saves nothing there).
//
// This header is plain C++17 and is also compiled for the host by the CPU test-suite
// (tests/native/codelet_host.cpp) so the algebra is checked without a GPU.
#pragma once

#include <utility>

#if defined(__HIPCC__)
#define DCTS_HD __host__ __device__ __forceinline__
#else
#define DCTS_HD inline __attribute__((always_inline))
#endif

namespace dcts {

// ---------------------------------------------------------------------------------
// compile-time trigonometry: cos(pi * p / q) for integers p, q > 0, evaluated in double
// ---------------------------------------------------------------------------------
constexpr double kPi = 3.14159265358979323846264338327950288;

constexpr double cx_sin_taylor(double x) {  // |x| <= pi/4
  const double x2 = x * x;
  double term = x, sum = x;
  for (int i = 1; i <= 12; ++i) {
    term *= -x2 / double((2 * i) * (2 * i + 1));
    sum += term;
  }
  return sum;
}
constexpr double cx_cos_taylor(double x) {  // |x| <= pi/4
  const double x2 = x * x;
  double term = 1.0, sum = 1.0;
  for (int i = 1; i <= 12; ++i) {
    term *= -x2 / double((2 * i - 1) * (2 * i));
    sum += term;
  }
  return sum;
}
// cos(pi * p / q), exact integer range reduction to [0, pi/4]
constexpr double cospi_frac(long long p, long long q) {
  long long r = p % (2 * q);
  if (r < 0) r += 2 * q;
  if (r > q) r = 2 * q - r;  // cos(2pi - t) = cos t          -> t in [0, pi]
  double sign = 1.0;
  if (2 * r > q) {           // cos(pi - t) = -cos t          -> t in [0, pi/2]
    r = q - r;
    sign = -1.0;
  }
  if (4 * r > q) {           // cos t = sin(pi/2 - t), pi/2 - t = pi (q - 2r) / (2q)
    return sign * cx_sin_taylor(kPi * double(q - 2 * r) / double(2 * q));
  }
  return sign * cx_cos_taylor(kPi * double(r) / double(q));
}
constexpr double sinpi_frac(long long p, long long q) {  // sin(pi p/q) = cos(pi (q - 2p) / (2q))
  return cospi_frac(q - 2 * p, 2 * q);
}

// index arithmetic of the odd-length DCT-IV (Dct4, odd M >= 5)
constexpr int inv_mod(int a, int q) {  // a^-1 mod q, gcd(a, q) = 1
  for (int x = 1; x < q; ++x)
    if ((a * x) % q == 1) return x;
  return 0;
}
constexpr int odd_index(int j, int M) {  // the n < M with 2n+1 = j (mod M), M odd
  for (int n = 0; n < M; ++n)
    if ((2 * n + 1) % M == j) return n;
  return -1;
}
constexpr int out_index(int kp, int M, int w) {  // the k < M with w (2k+1) = kp (mod M)
  for (int k = 0; k < M; ++k)
    if ((w * (2 * k + 1)) % M == kp) return k;
  return -1;
}
// sqrt(2) cos(t pi/4) and sqrt(2) sin(t pi/4) for odd t: the two real characters mod 8 other than (-1/t)
constexpr int chi_c(int t) { return (t % 8 == 1 || t % 8 == 7) ? 1 : -1; }
constexpr int chi_s(int t) { return (t % 8 == 1 || t % 8 == 3) ? 1 : -1; }

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [0, N)
template <class F, int... I>
DCTS_HD void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
DCTS_HD void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

#define DCTS_LAMBDA_INLINE __attribute__((always_inline))

// Two independent values carried through the same arithmetic: on gfx950 every +, -, * on this type
// is one packed-f32 instruction (v_pk_add/mul/fma_f32, two results per issue slot). A DCT-IV of
// even length M spawns two DCT-II of length M/2 on the rotated halves a, b: they run as ONE
// transform on pairs (a[n], b[n]): 17 % fewer VALU instructions at 56x56 (1385 -> 1151). MEASURED
// SLOWER on MI355X (56x56: 4.9 -> 4.4 TB/s): the packed-f32 instructions issue at half rate here
// (the timings fit 8 cycles per v_pk_* against 4 per scalar op), so two results per instruction buy
// nothing and the pair/unpair moves cost extra. Kept behind DCTS_PAIRS for other parts.
typedef float f2 __attribute__((vector_size(8)));

template <class T>
struct is_pair {
  static constexpr bool value = false;
};
template <>
struct is_pair<f2> {
  static constexpr bool value = true;
};

template <int N>
struct Dct2;
template <int M>
struct Dct4;

// ---------------------------------------------------------------------------------
// DCT-IV:  X[k] = sum_n v[n] cos(pi (2n+1)(2k+1) / (4M))
// ---------------------------------------------------------------------------------
template <int M>
struct Dct4 {
  template <class T>
  static DCTS_HD void run(const T (&v)[M], T (&X)[M]) {
    if constexpr (M == 1) {
      constexpr float c = float(cospi_frac(1, 4));
      X[0] = v[0] * c;
    } else if constexpr (M % 2 == 0) {
      constexpr int H = M / 2;
#ifdef DCTS_PAIRS
      if constexpr (!is_pair<T>::value) {
        // a[n], b[n] as the halves of one pair; the two half-length DCT-II run as one
        f2 ab[H];
        static_for<H>([&](auto i) DCTS_LAMBDA_INLINE {
          constexpr int n = decltype(i)::value;
          constexpr float c = float(cospi_frac(2 * n + 1, 4 * M));
          constexpr float s = float(sinpi_frac(2 * n + 1, 4 * M));
          constexpr float sg = (n % 2 == 0) ? 1.0f : -1.0f;
          const f2 p = {v[n], v[M - 1 - n]}, q = {v[M - 1 - n], v[n]};
          const f2 cc = {c, sg * c}, ss = {s, -sg * s};
          ab[n] = p * cc + q * ss;
        });
        f2 AB[H];
        Dct2<H>::run(ab, AB);
        X[0] = AB[0][0];
        X[M - 1] = -AB[0][1];
        static_for<H - 1>([&](auto i) DCTS_LAMBDA_INLINE {
          constexpr int j = decltype(i)::value + 1;
          X[2 * j] = AB[j][0] + AB[H - j][1];
          X[2 * j - 1] = AB[j][0] - AB[H - j][1];
        });
        return;
      }
#endif
      T a[H], b[H];
      static_for<H>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int n = decltype(i)::value;
        constexpr float c = float(cospi_frac(2 * n + 1, 4 * M));
        constexpr float s = float(sinpi_frac(2 * n + 1, 4 * M));
        constexpr float sg = (n % 2 == 0) ? 1.0f : -1.0f;
        a[n] = v[n] * c + v[M - 1 - n] * s;
        b[n] = v[M - 1 - n] * (sg * c) - v[n] * (sg * s);
      });
      T A[H], B[H];
      Dct2<H>::run(a, A);
      Dct2<H>::run(b, B);
      X[0] = A[0];
      X[M - 1] = -B[0];
      static_for<H - 1>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int j = decltype(i)::value + 1;
        X[2 * j] = A[j] + B[H - j];
        X[2 * j - 1] = A[j] - B[H - j];
      });
    } else if constexpr (M == 3) {
      // the split form below saves nothing at M = 3 (9 against 9) and costs registers: direct sum
      static_for<M>([&](auto ik) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(ik)::value;
        T acc{};
        static_for<M>([&](auto in) DCTS_LAMBDA_INLINE {
          constexpr int n = decltype(in)::value;
          constexpr float c = float(cospi_frac((2 * n + 1) * (2 * k + 1), 4 * M));
          if constexpr (n == 0)
            acc = v[0] * c;
          else
            acc += v[n] * c;
        });
        X[k] = acc;
      });
    } else {
      // odd M >= 5: pi a b / (4M) = t pi/4 + 2 pi n' k' / M (header comment). Every sign below is a
      // compile-time choice between + and -, or sits in a literal; nothing is multiplied by +-1.
      constexpr int m = (M - 1) / 2;
      constexpr int u = inv_mod(M % 8, 8), w = inv_mod(8 % M, M);
      constexpr double r = cospi_frac(1, 4);  // 1/sqrt(2)
      // The order of the statements is chosen by the compiler's register count: the sine half first
      // (pre-sums d, rows Sg), then the cosine half, each cosine row finishing its two outputs at once.
      // d[j-1] = chi_s(a1) (ps[j] - ps[M-j]),  s[j-1] = chi_c(a1) (pc[j] + pc[M-j]),  a1 = 2 n1 + 1 = j (mod M);
      // the factors chi_s(a1), chi_c(a1) go into the literals of the rows
      T d[m];
      static_for<m>([&](auto ij) DCTS_LAMBDA_INLINE {
        constexpr int j = decltype(ij)::value + 1;
        constexpr int n1 = odd_index(j, M), n2 = odd_index(M - j, M);
        if constexpr (chi_s(2 * n1 + 1) == chi_s(2 * n2 + 1))
          d[j - 1] = v[n1] - v[n2];
        else
          d[j - 1] = v[n1] + v[n2];
      });
      // row k' has two outputs, w b = k' (kA) and w b = -k' (kB) (mod M). With al = chi_c(b) chi_c(u) and
      // be = chi_s(b) chi_s(u) at each:  Sg[k'-1] = alA beA S[k'], C = C[k'], X[kA] = alA (C - Sg), X[kB] = alB (C + Sg)
      T Sg[m];
      static_for<m>([&](auto ik) DCTS_LAMBDA_INLINE {
        constexpr int kp = decltype(ik)::value + 1;
        constexpr int kA = out_index(kp, M, w), kB = out_index(M - kp, M, w);
        constexpr int abA = chi_c(2 * kA + 1) * chi_c(u) * chi_s(2 * kA + 1) * chi_s(u);
        constexpr int abB = chi_c(2 * kB + 1) * chi_c(u) * chi_s(2 * kB + 1) * chi_s(u);
        // 2 kA + 1 + 2 kB + 1 = 2M = 2 (mod 4): chi_c chi_s is the same at both outputs
        static_assert(abA == abB, "odd DCT-IV: sign pairing");
        static_for<m>([&](auto ij) DCTS_LAMBDA_INLINE {
          constexpr int j = decltype(ij)::value + 1;
          constexpr int a1 = 2 * odd_index(j, M) + 1;
          constexpr float ss = float(abA * chi_s(a1) * r * sinpi_frac(2 * j * kp, M));
          if constexpr (j == 1)
            Sg[kp - 1] = d[0] * ss;
          else
            Sg[kp - 1] += d[j - 1] * ss;
        });
      });
      T s[m];
      static_for<m>([&](auto ij) DCTS_LAMBDA_INLINE {
        constexpr int j = decltype(ij)::value + 1;
        constexpr int n1 = odd_index(j, M), n2 = odd_index(M - j, M);
        if constexpr (chi_c(2 * n1 + 1) == chi_c(2 * n2 + 1))
          s[j - 1] = v[n1] + v[n2];
        else
          s[j - 1] = v[n1] - v[n2];
      });
      // n' = 0 is the middle sample (a = M); it enters every cosine row with cos 0 = 1
      constexpr float r0 = float(chi_c(M) * r);
      const T t0 = v[m] * r0;
      {  // k' = 0: one output, b = M, no sine part
        constexpr int k = odd_index(0, M);
        constexpr int al = chi_c(2 * k + 1) * chi_c(u);
        constexpr int g1 = chi_c(2 * odd_index(1, M) + 1);
        T sum = s[0];
        static_for<m - 1>([&](auto ij) DCTS_LAMBDA_INLINE {
          constexpr int j = decltype(ij)::value + 2;
          if constexpr (chi_c(2 * odd_index(j, M) + 1) == g1)
            sum += s[j - 1];
          else
            sum -= s[j - 1];
        });
        constexpr float rg = float(g1 * r);
        if constexpr (al > 0)
          X[k] = sum * rg + t0;
        else
          X[k] = sum * (-rg) - t0;
      }
      static_for<m>([&](auto ik) DCTS_LAMBDA_INLINE {
        constexpr int kp = decltype(ik)::value + 1;
        constexpr int kA = out_index(kp, M, w), kB = out_index(M - kp, M, w);
        constexpr int alA = chi_c(2 * kA + 1) * chi_c(u), alB = chi_c(2 * kB + 1) * chi_c(u);
        T C = t0;
        static_for<m>([&](auto ij) DCTS_LAMBDA_INLINE {
          constexpr int j = decltype(ij)::value + 1;
          constexpr int a1 = 2 * odd_index(j, M) + 1;
          constexpr float cc = float(chi_c(a1) * r * cospi_frac(2 * j * kp, M));
          C += s[j - 1] * cc;
        });
        if constexpr (alA > 0)
          X[kA] = C - Sg[kp - 1];
        else
          X[kA] = Sg[kp - 1] - C;
        if constexpr (alB > 0)
          X[kB] = C + Sg[kp - 1];
        else
          X[kB] = -C - Sg[kp - 1];
      });
    }
  }
};

// ---------------------------------------------------------------------------------
// DCT-II:  X[k] = sum_n x[n] cos(pi (2n+1) k / (2N))
// ---------------------------------------------------------------------------------
template <int N>
struct Dct2 {
  template <class T>
  static DCTS_HD void run(const T (&x)[N], T (&X)[N]) {
    if constexpr (N == 1) {
      X[0] = x[0];
    } else if constexpr (N % 2 == 0) {
      constexpr int H = N / 2;
      T u[H], v[H];
      static_for<H>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int n = decltype(i)::value;
        u[n] = x[n] + x[N - 1 - n];
        v[n] = x[n] - x[N - 1 - n];
      });
      T E[H], O[H];
      Dct2<H>::run(u, E);
      Dct4<H>::run(v, O);
      static_for<H>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(i)::value;
        X[2 * k] = E[k];
        X[2 * k + 1] = O[k];
      });
    } else {
      constexpr int m = (N - 1) / 2;
      T u[m], v[m];
      static_for<m>([&](auto i) DCTS_LAMBDA_INLINE {
        constexpr int n = decltype(i)::value;
        u[n] = x[n] + x[N - 1 - n];
        v[n] = x[n] - x[N - 1 - n];
      });
      const T mid = x[m];
      static_for<N>([&](auto ik) DCTS_LAMBDA_INLINE {
        constexpr int k = decltype(ik)::value;
        if constexpr (k == 0) {
          T acc = mid;
          static_for<m>([&](auto in) DCTS_LAMBDA_INLINE { acc += u[decltype(in)::value]; });
          X[0] = acc;
        } else if constexpr (k % 2 == 0) {
          // middle sample: cos(pi N k / (2N)) = cos(pi k / 2) = (-1)^(k/2)
          T acc = ((k / 2) % 2 == 0) ? mid : -mid;
          static_for<m>([&](auto in) DCTS_LAMBDA_INLINE {
            constexpr int n = decltype(in)::value;
            constexpr float c = float(cospi_frac((2 * n + 1) * k, 2 * N));
            acc += u[n] * c;
          });
          X[k] = acc;
        } else {
          T acc{};
          static_for<m>([&](auto in) DCTS_LAMBDA_INLINE {
            constexpr int n = decltype(in)::value;
            constexpr float c = float(cospi_frac((2 * n + 1) * k, 2 * N));
            if constexpr (n == 0)
              acc = v[0] * c;
            else
              acc += v[n] * c;
          });
          X[k] = acc;
        }
      });
    }
  }
};

// Orthonormal scale of output k of a length-N transform:
// sqrt(1/N) for k == 0, sqrt(2/N) otherwise. cx_sqrt: Newton iteration in double.
constexpr double cx_sqrt(double a) {
  if (a <= 0.0) return 0.0;
  double x = a > 1.0 ? a : 1.0;
  for (int i = 0; i < 200; ++i) x = 0.5 * (x + a / x);
  return x;
}
template <int N>
constexpr float ortho_scale(int k) {
  return float(k == 0 ? cx_sqrt(1.0 / double(N)) : cx_sqrt(2.0 / double(N)));
}
constexpr float kInvSqrt2 = float(0.70710678118654752440084436210484903928);

}  // namespace dcts
