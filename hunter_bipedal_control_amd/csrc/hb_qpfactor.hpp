// Dense factorisation primitives shared by the three lane-cooperative active-set QP solvers (wbc_solve in hb_wbc.hpp; level 0 of
// hwbc_solve and small_lsqp in hb_hoqp.hpp).  All of them keep, for the Hessian A'A + diag(se^2), an upper triangular R with
// R'R = A'A + diag(se^2) and J = R^-1, both row-major in LDS with a leading dimension `ld`.  Lanes exchange data through LDS
// (cx.sync() is the ordering point) or through wave-uniform broadcasts; the host twin of tests/host_emu runs the same functions
// with one emulated lane.
#pragma once
#include "hb_math.hpp"

namespace hb {

// sum_{i < N} a[i * sa] * b[i * sb] in four interleaved partial sums: a single f64 FMA chain leaves most issue slots empty on a
// wave that has its SIMD to itself.
template <int N>
HB_HD double dot4(const double* a, int sa, const double* b, int sb) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < N; ++i) s[i & 3] += a[i * sa] * b[i * sb];
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// Givens insertion of one row into R (n x n upper triangular): R <- triangular factor of [R ; np'].  np is used up.
template <class Ctx>
HB_HD void givens_insert_row(const Ctx& cx, double* R, int ld, int n, double* np) {
  for (int k = 0; k < n; ++k) {
    const double a = R[k * ld + k], b = np[k];
    cx.sync();
    if (b != 0.0) {
      const double rh = rsqrt_t(a * a + b * b), cc = a * rh, ss = b * rh;
      for (int j = k + cx.lane; j < n; j += cx.nlanes) {
        const double t1 = R[k * ld + j], t2 = np[j];
        R[k * ld + j] = cc * t1 + ss * t2;
        np[j] = -ss * t1 + cc * t2;
      }
    }
    cx.sync();
  }
}

// The diagonal block diag(se) of a regularised factor.  se^2 enters every reflector twice, and how it is rounded is part of every
// solve's bits, so each form states it instead of leaving the contraction of se * se + x to the optimiser (which fused the product
// where se varies with k and hoisted it out of the loop where it does not).
// The two forms differ in the last bit only and may become one as soon as a change of the solvers' bits is allowed.
struct UniformDiag {   // se on every column; se^2 is rounded once
  double se, se2;
  HB_HD explicit UniformDiag(double s) : se(s), se2(s * s) {}
  HB_HD double at(int) const { return se; }
  HB_HD double plus_sq(int, double x) const { return se2 + x; }
  HB_HD double minus_sq(int, double x) const { return x - se2; }
};
struct HeadTailDiag {  // head on the first n_head columns, tail behind them; se^2 is never rounded on its own
  double head, tail;
  int n_head;
  HB_HD double at(int k) const { return k < n_head ? head : tail; }
  HB_HD double plus_sq(int k, double x) const { return fma(at(k), at(k), x); }
  HB_HD double minus_sq(int k, double x) const { return fma(-at(k), at(k), x); }
};

#if defined(__HIP_DEVICE_COMPILE__)
// Triangular factor of [diag(se) ; A] by n structured Householder reflectors.  Lane j holds column j of A (MA rows, zero where A has
// none) in registers; column k reaches the other lanes as wave-uniform values, so there is no LDS traffic and no ordering point
// inside.  Reflector k has its support on row k of the diagonal block and on the rows of A: row k of the factor is final after step k
// and the diagonal block is never stored.  Writes R(0..n-1, 0..wstore-1), zero outside the triangle; returns R_jj to lane j < n.
template <int MA, class Diag>
__device__ __forceinline__ double householder_factor(double (&acol)[MA], int j, int n, int wstore, const Diag& D, double* R, int ld) {
  double diag = 0.0;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    double dot = 0.0;
    double ck[MA];
#pragma unroll
    for (int r = 0; r < MA; ++r) {
      ck[r] = wave_bcast_f64(acol[r], k);
      dot += ck[r] * acol[r];
    }
    const double se = D.at(k);
    const double sig2 = D.plus_sq(k, wave_bcast_f64(dot, k));
    const double alpha = -sqrt(sig2);
    const double v0 = se - alpha;
    const double beta = 2.0 * rcp_t(D.minus_sq(k, sig2) + v0 * v0);
    const double w = beta * (dot + (j == k ? v0 * se : 0.0));
    const bool live = j > k && j < n;
#pragma unroll
    for (int r = 0; r < MA; ++r) acol[r] = live ? acol[r] - w * ck[r] : (j == k ? 0.0 : acol[r]);
    if (j < wstore) R[k * ld + j] = (j < k || j >= n) ? 0.0 : (j == k ? alpha : -w * v0);
    if (j == k) diag = alpha;
  }
  return diag;
}
#endif

// R(0..n-1, 0..wstore-1) <- the triangular factor of [diag(D) ; A] (A: mA x n, leading dimension lda) and, with kGrad,
// g <- A'b.  Device: householder_factor on register columns (MA >= mA rows).  Host twin: Givens insertion of the rows of A into
// diag(se), through np (n doubles).
template <int MA, bool kGrad, class Ctx, class Diag>
HB_HD void regularised_factor(const Ctx& cx, int n, int mA, const double* A, int lda, const double* b, double* g, const Diag& D, double* R,
                              int ld, int wstore, double* np) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int j = cx.lane;
  double acol[MA];
  double gj = 0.0;
#pragma unroll
  for (int r = 0; r < MA; ++r) {
    acol[r] = (j < n && r < mA) ? A[r * lda + j] : 0.0;
    if constexpr (kGrad) gj += acol[r] * (r < mA ? b[r] : 0.0);
  }
  if (kGrad && j < n) g[j] = gj;
  householder_factor<MA>(acol, j, n, wstore, D, R, ld);
  (void)np;
  cx.sync();
#else
  for (int idx = cx.lane; idx < n * wstore; idx += cx.nlanes) {
    const int i = idx / wstore, c = idx % wstore;
    R[i * ld + c] = i == c ? D.at(i) : 0.0;
  }
  if constexpr (kGrad)
    for (int i = cx.lane; i < n; i += cx.nlanes) g[i] = 0.0;
  cx.sync();
  for (int rw = 0; rw < mA; ++rw) {
    for (int j = cx.lane; j < n; j += cx.nlanes) {
      np[j] = A[rw * lda + j];
      if constexpr (kGrad) g[j] += A[rw * lda + j] * b[rw];
    }
    cx.sync();
    givens_insert_row(cx, R, ld, n, np);
  }
#endif
}

// J <- R^-1 of the n x n upper triangle, one column per lane (the part of J below the diagonal is zeroed).
// The substitution accumulates with fma(), spelled out: the device compiler fuses `s -= a * b` anyway (same code object with
// either spelling), the host compiler does not, and the twin then rounds twice per term where the device rounds once — on an
// ill-conditioned factor its |J R - I| came to 2.1 (n + 2) u |J||R| where the fused form stays below 0.9.
template <class Ctx>
HB_HD void invert_upper(const Ctx& cx, const double* R, int ld, int n, double* J) {
  for (int col = cx.lane; col < n; col += cx.nlanes) {
    for (int i = n - 1; i > col; --i) J[i * ld + col] = 0.0;
    for (int i = col; i >= 0; --i) {
      double s = (i == col) ? 1.0 : 0.0;
      for (int k = i + 1; k <= col; ++k) s = fma(-R[i * ld + k], J[k * ld + col], s);
      J[i * ld + col] = s * rcp_t(R[i * ld + i]);
    }
  }
  cx.sync();
}

// Drops active constraint l of q (J'N = [R; 0], R: q x q): column shift of R with the working-set records (act, lam), then the
// Givens sweep that restores the triangle; the same rotations go over the columns of J (n x n, one row per lane).
template <class Ctx>
HB_HD void drop_constraint(const Ctx& cx, int n, int ld, double* R, double* J, int* act, double* lam, int* is_active, int l, int& q) {
  if (cx.lane == 0) is_active[act[l]] = 0;
  cx.sync();
  for (int j = l; j < q - 1; ++j) {
    for (int i = cx.lane; i <= j + 1; i += cx.nlanes) R[i * ld + j] = R[i * ld + j + 1];
    if (cx.lane == 0) { act[j] = act[j + 1]; lam[j] = lam[j + 1]; }
    cx.sync();
  }
  for (int i = cx.lane; i < q; i += cx.nlanes) R[i * ld + q - 1] = 0.0;
  --q;
  cx.sync();
  for (int j = l; j < q; ++j) {
    const double a = R[j * ld + j], b = R[(j + 1) * ld + j];
    cx.sync();
    if (b != 0.0) {
      const double rh = rsqrt_t(a * a + b * b), cc = a * rh, ss = b * rh;
      for (int k = cx.lane; k < n; k += cx.nlanes) {
        if (k >= j && k < q) {
          const double t1 = R[j * ld + k], t2 = R[(j + 1) * ld + k];
          R[j * ld + k] = cc * t1 + ss * t2;
          R[(j + 1) * ld + k] = -ss * t1 + cc * t2;
        }
        const double u1 = J[k * ld + j], u2 = J[k * ld + j + 1];
        J[k * ld + j] = cc * u1 + ss * u2;
        J[k * ld + j + 1] = -ss * u1 + cc * u2;
      }
    }
    cx.sync();
    if (cx.lane == 0) R[(j + 1) * ld + j] = 0.0;
    cx.sync();
  }
}

}  // namespace hb
