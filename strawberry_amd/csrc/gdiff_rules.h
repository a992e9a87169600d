// strawberry_amd/csrc/gdiff_rules.h -- the decisions of the differential isoform usage between two GROUPS of replicate samples
// (include/sbgpu.h: sbgpu_em_gdiff_*), as functions the host form (gdiff_host.cpp) and the kernels (gdiff_device.h)
// both call, so that the two forms cannot drift:
//   - which isoforms of a locus are kept, and what the locus' status is before the solves (gdiff_kept, gdiff_pre_status),
//   - the running sum of a pool's column sums and the scale of a pooled column (gdiff_add, gdiff_alpha),
//   - one locus' two statistics, integers and final status from its solves and three fits (GdiffAcc, gdiff_finish),
//   - the shapes of a whole call (gdiff_shapes; host only).
// Usage and the isoform of largest change are diff_rules.h's (diff_sum, diff_usage, diff_top).  Compiled under -ffp-contract=off.
#pragma once

#include <math.h>

#include <vector>

#include "diff_rules.h"

namespace sb {

constexpr int kGdiffMaxSamples = SBGPU_GDIFF_MAX_SAMPLES;

// Isoform j of a locus is kept: kept in ANY sample (a null keep keeps everything); keep_of_locus: [n_samples] pointers
__host__ __device__ inline bool gdiff_kept(const int32_t *const *keep_of_locus, int n_samples, int niso, int j)
{
   for (int s = 0; s < n_samples; ++s)
      if (loo_kept(keep_of_locus[s], niso, j)) return true;
   return false;
}

// Rule 1: the status of a locus of K kept isoforms, p_a and p_b present samples, `rows` bins over the present samples
__host__ __device__ inline int32_t gdiff_pre_status(int64_t K, int p_a, int p_b, int64_t rows)
{
   return K == 0 ? SBGPU_DIFF_EMPTY : K == 1 ? SBGPU_DIFF_SOLE : K > kDiffMaxKept ? SBGPU_DIFF_TOO_WIDE : p_a == 0 || p_b == 0 ? SBGPU_GDIFF_ONE_GROUP
        : rows > kDiffMaxPooledBins ? SBGPU_DIFF_TOO_DEEP : SBGPU_DIFF_OK;
}

// Rule 3: a pool's sum of column sums, from the first term in ascending sample order (n: the terms added so far)
__host__ __device__ inline double gdiff_add(double sum, int n, double c) { return n == 0 ? c : sum + c; }
// Rule 3: the scale of sample s' column in a pool of n present samples whose column sums add to `sum`.  At n = 2: diff_alpha's bits
// (a division by 2.0 and a product with 0.5 round alike).
__host__ __device__ inline double gdiff_alpha(double sum, double c_s, int n)
{
   if (!(c_s != 0.0)) return 1.0;
   const double q = sum / c_s;
   return q / (double)n;
}

// Rules 5-7 for an OK locus: the present samples are added in sample order, then the group and ALL sub-problems, then finish.
struct GdiffAcc {
   double between, within;
   long long lost_own, shift;
   int n;
   bool thin, unsolved;
};
__host__ __device__ inline void gdiff_begin(GdiffAcc *a)
{
   a->between = a->within = 0.0, a->lost_own = a->shift = 0, a->n = 0, a->thin = a->unsolved = false;
}
// One present sample: st: its solve's status; ll_*: its log-likelihood at its own, its group's and ALL's theta; lost_* =
// n_dropped + n_impossible of the same three fits; single: its group has no sub-problem of its own (the group's theta IS the
// sample's: its group-level numbers are its own, whatever was passed) -> n_frag
__host__ __device__ inline long long gdiff_add_sample(GdiffAcc *a, int32_t st, bool single, double ll_own, double ll_grp, double ll_all, long long n_live,
                                                      long long n_imp, long long lost_own, long long lost_grp, long long lost_all)
{
   const long long n_frag = n_live - n_imp;
   if (n_frag == 0 || st == SBGPU_EM_INIT_EMPTY) a->thin = true;
   if (st == SBGPU_EM_DENOM_ZERO) a->unsolved = true;
   const double grp = single ? ll_own : ll_grp;
   const double loss_b = grp - ll_all;
   const double loss_w = single ? 0.0 : ll_own - grp;
   a->between = a->n == 0 ? loss_b : a->between + loss_b;
   a->within = a->n == 0 ? loss_w : a->within + loss_w;
   a->lost_own += lost_own;
   a->shift += ((single ? lost_own : lost_grp) - lost_own) + (lost_all - lost_own);
   a->n += 1;
   return n_frag;
}
// A group's sub-problem (p_g >= 2): lost_members: the sum of its members' own lost
__host__ __device__ inline void gdiff_add_group(GdiffAcc *a, int32_t st, long long lost, long long lost_members)
{
   if (st == SBGPU_EM_DENOM_ZERO) a->unsolved = true;
   a->shift += lost - lost_members;
}
struct GdiffLocus {
   double lr_between, lr_within;
   long long lost_shift;
   int32_t status, dof_between, dof_within;
};
__host__ __device__ inline GdiffLocus gdiff_finish(const GdiffAcc &a, int K, int32_t st_all, long long lost_all)
{
   GdiffLocus o;
   o.status = a.thin ? SBGPU_GDIFF_THIN : a.unsolved || st_all == SBGPU_EM_DENOM_ZERO ? SBGPU_DIFF_UNSOLVED : SBGPU_DIFF_OK;
   if (o.status != SBGPU_DIFF_OK) {
      o.lr_between = o.lr_within = 0.0, o.lost_shift = 0, o.dof_between = o.dof_within = 0;
      return o;
   }
   o.lr_between = 2.0 * a.between, o.lr_within = 2.0 * a.within;
   o.lost_shift = a.shift + (lost_all - a.lost_own);
   o.dof_between = K - 1, o.dof_within = (a.n - 2) * (K - 1);
   return o;
}

} // namespace sb


namespace sb {

// Rules 1 and 2 for a whole call (host only; the offsets are the caller's to check): what both forms make first.  The slots of
// a locus: 0 .. S - 1 the samples, S and S + 1 the two groups, S + 2 ALL.
struct GdiffShapes {
   int S = 0, n_a = 0;
   std::vector<int32_t> status;      // [n_loci], before the solves
   std::vector<int32_t> p_a, p_b;    // [n_loci] the present samples of each group
   std::vector<int32_t> rank;        // [n_iso] as DiffShapes'
   std::vector<int64_t> first_sub;   // [n_loci] the locus' first sub-problem among all of the call, -1 where it is not OK
   std::vector<int64_t> slot_sub;    // [n_loci x (S + 3)] the sub-problem whose theta a slot reads: a sample's own (-1: absent, or the locus is
                                     // not OK), a group's (its one present sample's own where p_g = 1), ALL's
   std::vector<int64_t> kept_off;    // [n_loci + 1] into kept_col (the OK and SOLE loci's kept isoforms)
   std::vector<int32_t> kept_col;    // locus-local indices, ascending
   std::vector<int32_t> sub_locus, sub_kind, sub_sample;     // [n_sub]; sub_sample: -1 for a group's and ALL's
   std::vector<int64_t> sub_row_off, sub_iso_off, sub_f_off; // [n_sub + 1]
   int64_t n_sub() const { return (int64_t)sub_locus.size(); }
   int slots() const { return S + 3; }
   bool group_has_sub(int64_t l, int g) const { return (g ? p_b : p_a)[(size_t)l] >= 2 && first_sub[(size_t)l] >= 0; }
};
inline void gdiff_shapes(int64_t n_loci, int n_a, int n_b, const int64_t *const *row_off, const int64_t *iso_off, const int32_t *const *keep, GdiffShapes *o)
{
   const int S = n_a + n_b;
   const int64_t n_iso = iso_off[n_loci];
   o->S = S, o->n_a = n_a;
   o->status.assign((size_t)n_loci, SBGPU_DIFF_OK), o->first_sub.assign((size_t)n_loci, -1), o->kept_off.assign((size_t)n_loci + 1, 0);
   o->p_a.assign((size_t)n_loci, 0), o->p_b.assign((size_t)n_loci, 0);
   o->slot_sub.assign((size_t)n_loci * (size_t)(S + 3), -1);
   o->rank.assign((size_t)n_iso, -1);
   o->kept_col.clear(), o->sub_locus.clear(), o->sub_kind.clear(), o->sub_sample.clear();
   o->sub_row_off.assign(1, 0), o->sub_iso_off.assign(1, 0), o->sub_f_off.assign(1, 0);
   std::vector<int32_t> cols;
   const int32_t *keep_l[kGdiffMaxSamples];
   const auto push = [o](int64_t l, int kind, int sample, int64_t rows, int64_t K) {
      o->sub_locus.push_back((int32_t)l), o->sub_kind.push_back(kind), o->sub_sample.push_back(sample);
      o->sub_row_off.push_back(o->sub_row_off.back() + rows), o->sub_iso_off.push_back(o->sub_iso_off.back() + K);
      o->sub_f_off.push_back(o->sub_f_off.back() + rows * K);
   };
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t i0 = iso_off[l];
      const int niso = (int)(iso_off[l + 1] - i0);
      int64_t nb[kGdiffMaxSamples], rows_g[2] = {0, 0};
      int p[2] = {0, 0};
      for (int s = 0; s < S; ++s) {
         nb[s] = row_off[s][l + 1] - row_off[s][l];
         keep_l[s] = keep && keep[s] ? keep[s] + i0 : nullptr;
         if (nb[s] > 0) p[s >= n_a] += 1, rows_g[s >= n_a] += nb[s];
      }
      cols.clear();
      for (int j = 0; j < niso; ++j)
         if (gdiff_kept(keep_l, S, niso, j)) cols.push_back(j);
      const int64_t K = (int64_t)cols.size();
      const int32_t st = gdiff_pre_status(K, p[0], p[1], rows_g[0] + rows_g[1]);
      const bool listed = st == SBGPU_DIFF_OK || st == SBGPU_DIFF_SOLE;
      o->status[(size_t)l] = st, o->p_a[(size_t)l] = p[0], o->p_b[(size_t)l] = p[1];
      for (int64_t r = 0; r < K; ++r) o->rank[(size_t)(i0 + cols[(size_t)r])] = listed ? (int32_t)r : -2;
      if (listed) o->kept_col.insert(o->kept_col.end(), cols.begin(), cols.end());
      if (st == SBGPU_DIFF_OK) {
         int64_t *slot = o->slot_sub.data() + (size_t)l * (size_t)(S + 3);
         o->first_sub[(size_t)l] = o->n_sub();
         for (int s = 0; s < S; ++s)
            if (nb[s] > 0) slot[s] = o->n_sub(), push(l, SBGPU_GDIFF_KIND_OWN, s, nb[s], K);
         for (int g = 0; g < 2; ++g) {
            if (p[g] >= 2) {
               slot[S + g] = o->n_sub(), push(l, g ? SBGPU_GDIFF_KIND_GROUP_B : SBGPU_GDIFF_KIND_GROUP_A, -1, rows_g[g], K);
               continue;
            }
            for (int s = g ? n_a : 0; s < (g ? S : n_a); ++s)
               if (nb[s] > 0) slot[S + g] = slot[s];
         }
         slot[S + 2] = o->n_sub(), push(l, SBGPU_GDIFF_KIND_ALL, -1, rows_g[0] + rows_g[1], K);
      }
      o->kept_off[(size_t)l + 1] = (int64_t)o->kept_col.size();
   }
}

} // namespace sb
