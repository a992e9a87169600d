// strawberry_amd/csrc/info_rules.h -- the decisions of the isoform information (include/sbgpu.h: sbgpu_em_info_*,
// sbgpu_model_info_device): the observed information matrix of a locus' mixture over its free isoforms, its
// factorisation without pivoting (which isoforms the counted bins can tell apart, which are a combination of earlier ones), and
// the covariance of theta on the simplex -- as functions the host form (info_host.cpp) and the kernels (info_device.h) both
// call, so that the two forms cannot drift.  Who is kept, which bins are live, c_j, g_j, d_b and "possible" ARE the
// assignment's and the fit's (context_rules.h, assign_rules.h, fit_rules.h): called here, not restated.
// A plain C++ compiler takes this header (the host form is free of HIP).  Everything here is compiled under -ffp-contract=off.
//
// The matrices are packed lower triangles over the locus' FREE isoforms in ascending order (free-local indices 0 .. nf - 1):
// entry (i, j), i >= j, lies at info_tri(i, j).  st[p] is the state of free isoform p: an SBGPU_INFO_* ident code, or
// kInfoPending while it is observed and the factorisation has not reached it.  "k in R" is st[k] == SBGPU_INFO_IDENTIFIED.
// Every sum starts from 0.0 and adds its terms in ascending index.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sbgpu.h"
#include "fit_rules.h"

namespace sb {

constexpr int kInfoMaxFree = 64;                                   // free isoforms of a locus whose triangles fit LDS twice (2 x 16.25 KB)
constexpr int kInfoTri = kInfoMaxFree * (kInfoMaxFree + 1) / 2;    // entries of one packed triangle
constexpr int kInfoWave = 64;                                      // the partial sums of the wave order
constexpr uint8_t kInfoPending = 255;

__host__ __device__ inline int info_tri(int i, int j) { return i * (i + 1) / 2 + j; } // i >= j
__host__ __device__ inline double info_sym(const double *A, int i, int j) { return i >= j ? A[info_tri(i, j)] : A[info_tri(j, i)]; }
__host__ __device__ inline bool info_in_r(const uint8_t *st, int k) { return st[k] == SBGPU_INFO_IDENTIFIED; }

// Rule 2.  w_b of a possible bin: fit_ratio, then one more division; 0.0 otherwise.
__host__ __device__ inline double info_weight(int32_t n, double d, bool possible) { return possible ? fit_ratio(n, d) / d : 0.0; }

// Rule 3.  j is free when it is kept, c_j != 0 and g_j > 0.  asg_gain gives exactly 0.0 to an isoform that is not kept or whose
// column is empty, so the gain alone decides (a NaN gain is not free).
__host__ __device__ inline bool info_free(double g) { return g > 0.0; }

// Rule 4.  One term of S_jk, and H_jk from S_jk.
__host__ __device__ inline double info_term(double w, double fj, double fk) { return (w * fj) * fk; }
__host__ __device__ inline double info_h(double S, double cj, double ck) { return (S / cj) / ck; }

// THE WAVE ORDER, stated once.  partial[t], t = 0 .. 63, is the ascending sum of the terms of bins b = t, t + 64, ... (0.0 where
// there are none); then for s = 32, 16, ..., 1: partial[i] += partial[i + s] for i < s; the sum is partial[0].  It is a wave's
// natural reduction -- lane t walks its bins, lane i adds lane i + s (__shfl_down) -- which is how the kernels run it.
// Fl: the locus' weights, row-major [nb][niso]; w [nb]; gj, gk: the two columns.
__host__ __device__ inline double info_wave_order_sum(const double *w, const double *Fl, int nb, int niso, int gj, int gk)
{
   double partial[kInfoWave];
   for (int t = 0; t < kInfoWave; ++t) {
      double s = 0.0;
      for (int b = t; b < nb; b += kInfoWave) s += info_term(w[b], Fl[(int64_t)b * niso + gj], Fl[(int64_t)b * niso + gk]);
      partial[t] = s;
   }
   for (int s = kInfoWave / 2; s >= 1; s >>= 1)
      for (int i = 0; i < s; ++i) partial[i] += partial[i + s];
   return partial[0];
}

// Rule 5, 6.  A free j is observed when H_jj > 0 (a NaN is not); C_jk = (H_jk / dg_j) / dg_k with dg_j = sqrt(H_jj).
__host__ __device__ inline bool info_observed(double hjj) { return hjj > 0.0; }
__host__ __device__ inline double info_scaled(double h, double dgi, double dgj) { return (h / dgi) / dgj; }

// Rule 7.  A holds C; its off-diagonal entries (i, k) become L_ik as column k is retained, its diagonal stays C's (L_jj is
// kept beside it, in ld[j]).  piv_j = C_jj - sum over k in R, k < j, of L_jk * L_jk.
__host__ __device__ inline double info_pivot(const double *A, const uint8_t *st, int j)
{
   double s = 0.0;
   for (int k = 0; k < j; ++k)
      if (info_in_r(st, k)) s += A[info_tri(j, k)] * A[info_tri(j, k)];
   return A[info_tri(j, j)] - s;
}
__host__ __device__ inline bool info_retained(double piv) { return piv > SBGPU_INFO_PIVOT_EPS; }
// L_ij for i > j, j retained with L_jj = ljj
__host__ __device__ inline double info_lower(const double *A, const uint8_t *st, int i, int j, double ljj)
{
   double s = 0.0;
   for (int k = 0; k < j; ++k)
      if (info_in_r(st, k)) s += A[info_tri(i, k)] * A[info_tri(j, k)];
   return (A[info_tri(i, j)] - s) / ljj;
}
// alias_of an aliased j (free-local): the k in R, k < j, of largest |L_jk| under strict > in ascending k (a NaN never wins);
// -1 where there is none
__host__ __device__ inline int info_alias_of(const double *A, const uint8_t *st, int j)
{
   double best = -1.0;
   int best_k = -1;
   for (int k = 0; k < j; ++k)
      if (info_in_r(st, k)) {
         const double a = fabs(A[info_tri(j, k)]);
         if (a > best) best = a, best_k = k;
      }
   return best_k;
}

// Rule 8.  Y = L_R^-1 into B, a column at a time: the caller walks i = j, j + 1, ... over R in ascending order and stores each
// entry before it asks for the next.
__host__ __device__ inline double info_y(const double *A, const double *ld, const double *B, const uint8_t *st, int i, int j)
{
   if (i == j) return 1.0 / ld[j];
   double s = 0.0;
   for (int k = j; k < i; ++k)
      if (info_in_r(st, k)) s += A[info_tri(i, k)] * B[info_tri(k, j)];
   return -s / ld[i];
}
// V_ij for i >= j, both in R
__host__ __device__ inline double info_v(const double *B, const uint8_t *st, int nf, int i, int j)
{
   double s = 0.0;
   for (int k = i; k < nf; ++k)
      if (info_in_r(st, k)) s += B[info_tri(k, i)] * B[info_tri(k, j)];
   return s;
}
__host__ __device__ inline double info_hinv(double v, double dgi, double dgj) { return (v / dgi) / dgj; }

// Rule 9.  A holds Hinv (0.0 outside R): u_i, t, cov_ij, se_j.
__host__ __device__ inline double info_u(const double *A, const uint8_t *st, int nf, int i)
{
   double s = 0.0;
   for (int j = 0; j < nf; ++j)
      if (info_in_r(st, j)) s += info_sym(A, i, j);
   return s;
}
__host__ __device__ inline double info_t(const double *u, const uint8_t *st, int nf)
{
   double s = 0.0;
   for (int i = 0; i < nf; ++i)
      if (info_in_r(st, i)) s += u[i];
   return s;
}
__host__ __device__ inline double info_cov(double hinv, double ui, double uj, double t) { return t > 0.0 ? hinv - (ui * uj) / t : hinv; }
__host__ __device__ inline double info_se(double cov_jj) { return cov_jj > 0.0 ? sqrt(cov_jj) : 0.0; } // sqrt(max(cov_jj, 0.0))

// Rule 10.  A holds cov.  partner of j in R (free-local; -1: none) and the signed correlation (0.0: none): the k in R, k != j,
// with se_j, se_k > 0, of largest |corr_jk| under strict > in ascending k (a NaN never wins).
__host__ __device__ inline int info_partner(const double *A, const double *se, const uint8_t *st, int nf, int j, double *corr)
{
   double best = -1.0, best_c = 0.0;
   int best_k = -1;
   if (se[j] > 0.0)
      for (int k = 0; k < nf; ++k)
         if (k != j && info_in_r(st, k) && se[k] > 0.0) {
            const double c = info_sym(A, j, k) / (se[j] * se[k]);
            if (fabs(c) > best) best = fabs(c), best_c = c, best_k = k;
         }
   *corr = best_c;
   return best_k;
}

// Rule 13.  Where entry (gj, gk), gj <= gk, of the upper triangle over a locus' niso isoforms lies in its packed block (row-major)
__host__ __device__ inline int64_t info_cov_at(int64_t niso, int64_t gj, int64_t gk) { return gj * niso - gj * (gj - 1) / 2 + (gk - gj); }
// entries of a locus' block: the whole triangle up to the limit, none beyond
__host__ __device__ inline int64_t info_cov_entries(int64_t niso) { return niso <= kInfoMaxFree ? niso * (niso + 1) / 2 : 0; }

} // namespace sb
