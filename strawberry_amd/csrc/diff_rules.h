// strawberry_amd/csrc/diff_rules.h -- the decisions of the differential isoform usage (include/sbgpu.h: sbgpu_em_diff_*),
// as functions the host form (diff_host.cpp) and the kernels (diff_device.h) both call, so that the two forms cannot drift:
//   - which isoforms of a locus are kept, and what the locus' status is before the solves (diff_kept, diff_pre_status),
//   - the scale of a pooled column (diff_alpha),
//   - one locus' statistic, integers and final status from its three solves and five fits (diff_locus),
//   - usage and the isoform of largest change (diff_sum, diff_usage, diff_top).
// Compiled under -ffp-contract=off: alpha is a sum, a quotient and a product; the statistic two subtractions, a sum, a product.
#pragma once

#include <math.h>

#include <vector>

#include "loo_rules.h"

namespace sb {

constexpr int kDiffMaxKept = SBGPU_DIFF_MAX_KEPT;              // the EM plan's widest locus
constexpr int kDiffMaxPooledBins = SBGPU_DIFF_MAX_POOLED_BINS; // the fit's deepest locus: the pooled problem has nb_A + nb_B bins

// Isoform j of a locus is kept: kept in A or kept in B (a null side keeps everything)
__host__ __device__ inline bool diff_kept(const int32_t *keep_a_of_locus, const int32_t *keep_b_of_locus, int niso, int j)
{
   return loo_kept(keep_a_of_locus, niso, j) || loo_kept(keep_b_of_locus, niso, j);
}

// Rule 1: the status of a locus of K kept isoforms, nb_a and nb_b bins, before the solves
__host__ __device__ inline int32_t diff_pre_status(int64_t K, int64_t nb_a, int64_t nb_b)
{
   return K == 0 ? SBGPU_DIFF_EMPTY : K == 1 ? SBGPU_DIFF_SOLE : K > kDiffMaxKept ? SBGPU_DIFF_TOO_WIDE : nb_a + nb_b > kDiffMaxPooledBins ? SBGPU_DIFF_TOO_DEEP : SBGPU_DIFF_OK;
}

// Rule 3: the scale of sample s' column in the pooled problem; c_s is c_a or c_b
__host__ __device__ inline double diff_alpha(double c_a, double c_b, double c_s)
{
   if (!(c_s != 0.0)) return 1.0;
   const double sum = c_a + c_b;
   const double q = sum / c_s;
   return 0.5 * q;
}

// Rules 5-7 for an OK locus.  st_*, the three solves' statuses; ll_*: own fits; llx_*: A and B at the pooled theta; n_live /
// n_imp: of the bases' own fits; lost_* = n_dropped + n_impossible (own: a, b, p; cross: ax, bx).
struct DiffLocus {
   double lr_stat;
   long long n_a, n_b, lost_shift;
   int32_t status, dof;
};
__host__ __device__ inline DiffLocus diff_locus(int K, int32_t st_a, int32_t st_b, int32_t st_p, double ll_a, double ll_b, double llx_a, double llx_b,
                                                long long n_live_a, long long n_imp_a, long long n_live_b, long long n_imp_b, long long lost_a,
                                                long long lost_b, long long lost_p, long long lost_ax, long long lost_bx)
{
   DiffLocus o;
   o.n_a = n_live_a - n_imp_a, o.n_b = n_live_b - n_imp_b;
   o.status = SBGPU_DIFF_OK;
   if (o.n_a == 0 || o.n_b == 0 || st_a == SBGPU_EM_INIT_EMPTY || st_b == SBGPU_EM_INIT_EMPTY) o.status = SBGPU_DIFF_ONE_SAMPLE;
   else if (st_a == SBGPU_EM_DENOM_ZERO || st_b == SBGPU_EM_DENOM_ZERO || st_p == SBGPU_EM_DENOM_ZERO) o.status = SBGPU_DIFF_UNSOLVED;
   if (o.status != SBGPU_DIFF_OK) {
      o.lr_stat = 0.0, o.n_a = 0, o.n_b = 0, o.lost_shift = 0, o.dof = 0;
      return o;
   }
   const double loss_a = ll_a - llx_a, loss_b = ll_b - llx_b;
   const double both = loss_a + loss_b;
   o.lr_stat = 2.0 * both;
   o.lost_shift = lost_p - lost_a - lost_b + (lost_ax - lost_a) + (lost_bx - lost_b);
   o.dof = K - 1;
   return o;
}

// Rule 8: the ascending sum of a sub-problem's theta, and one isoform's usage
__host__ __device__ inline double diff_sum(const double *theta, int K)
{
   double s = 0.0;
   for (int k = 0; k < K; ++k) s += theta[k];
   return s;
}
__host__ __device__ inline double diff_usage(double theta, double sum) { return sum != 0.0 ? theta / sum : 0.0; }

// Rule 9: the kept rank of largest |usage_b - usage_a| (strict >, ascending, from -1.0; a NaN never wins), -1 where K = 0
__host__ __device__ inline int diff_top(const double *theta_a, double sum_a, const double *theta_b, double sum_b, int K)
{
   double best = -1.0;
   int top = -1;
   for (int k = 0; k < K; ++k) {
      const double d = fabs(diff_usage(theta_b[k], sum_b) - diff_usage(theta_a[k], sum_a));
      if (d > best) best = d, top = k;
   }
   return top;
}

} // namespace sb


namespace sb {

// Rules 1 and 2 for a whole pair of batches (host only; the offsets are the caller's to check): what both forms make first
struct DiffShapes {
   std::vector<int32_t> diff_status; // [n_loci], before the solves
   std::vector<int32_t> rank;        // [n_iso] the kept rank of an isoform of an OK or SOLE locus; -1: not kept; -2: kept, its locus is neither
   std::vector<int64_t> first_sub;   // [n_loci] the number of the locus' sub-problem A among all sub-problems, -1 where the locus is not OK
   std::vector<int64_t> kept_off;    // [n_loci + 1] into kept_col (the OK and SOLE loci's kept isoforms)
   std::vector<int32_t> kept_col;    // locus-local indices, ascending
   std::vector<int32_t> sub_locus, sub_kind;                 // [n_sub]
   std::vector<int64_t> sub_row_off, sub_iso_off, sub_f_off; // [n_sub + 1]
   int64_t n_sub() const { return (int64_t)sub_locus.size(); }
};
inline void diff_shapes(int64_t n_loci, const int64_t *row_off_a, const int64_t *row_off_b, const int64_t *iso_off, const int32_t *keep_a,
                        const int32_t *keep_b, DiffShapes *o)
{
   const int64_t n_iso = iso_off[n_loci];
   o->diff_status.assign((size_t)n_loci, SBGPU_DIFF_OK), o->first_sub.assign((size_t)n_loci, -1), o->kept_off.assign((size_t)n_loci + 1, 0);
   o->rank.assign((size_t)n_iso, -1);
   o->kept_col.clear(), o->sub_locus.clear(), o->sub_kind.clear();
   o->sub_row_off.assign(1, 0), o->sub_iso_off.assign(1, 0), o->sub_f_off.assign(1, 0);
   std::vector<int32_t> cols;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t i0 = iso_off[l];
      const int64_t nb[3] = {row_off_a ? row_off_a[l + 1] - row_off_a[l] : 0, row_off_b ? row_off_b[l + 1] - row_off_b[l] : 0, 0};
      const int niso = (int)(iso_off[l + 1] - i0);
      cols.clear();
      for (int j = 0; j < niso; ++j)
         if (diff_kept(keep_a ? keep_a + i0 : nullptr, keep_b ? keep_b + i0 : nullptr, niso, j)) cols.push_back(j);
      const int64_t K = (int64_t)cols.size();
      const int32_t st = diff_pre_status(K, nb[0], nb[1]);
      const bool listed = st == SBGPU_DIFF_OK || st == SBGPU_DIFF_SOLE;
      o->diff_status[(size_t)l] = st;
      for (int64_t r = 0; r < K; ++r) o->rank[(size_t)(i0 + cols[(size_t)r])] = listed ? (int32_t)r : -2;
      if (listed) o->kept_col.insert(o->kept_col.end(), cols.begin(), cols.end());
      if (st == SBGPU_DIFF_OK) {
         o->first_sub[(size_t)l] = o->n_sub();
         for (int kind = 0; kind < 3; ++kind) {
            const int64_t rows = kind == SBGPU_DIFF_KIND_POOLED ? nb[0] + nb[1] : nb[kind];
            o->sub_locus.push_back((int32_t)l), o->sub_kind.push_back(kind);
            o->sub_row_off.push_back(o->sub_row_off.back() + rows), o->sub_iso_off.push_back(o->sub_iso_off.back() + K);
            o->sub_f_off.push_back(o->sub_f_off.back() + rows * K);
         }
      }
      o->kept_off[(size_t)l + 1] = (int64_t)o->kept_col.size();
   }
}

} // namespace sb
