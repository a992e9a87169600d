// strawberry_amd/csrc/loo_rules.h -- the decisions of the drop-one isoform support (include/sbgpu.h: sbgpu_em_loo_*),
// as functions the host form (loo_host.cpp) and the kernels (loo_device.h) both call, so that the two forms cannot drift:
//   - which isoforms of a locus are kept, and what the locus' status is (loo_kept, loo_locus_status),
//   - the column a sub-problem's column stands for (loo_sub_rank),
//   - one isoform's statistics from its sub-problem's and the base's results (loo_isoform).
// Compiled under -ffp-contract=off: the statistic is one subtraction and one product, the gain one subtraction.
#pragma once

#include <math.h>

#include <vector>

#include "context_rules.h"

namespace sb {

constexpr int kLooMaxKept = SBGPU_LOO_MAX_KEPT; // kept isoforms of a locus whose isoforms are tested

// Isoform j of a locus is kept: the bit ctx_kept_word gives it (keep_of_locus null: no filter was given, everything is kept)
__host__ __device__ inline bool loo_kept(const int32_t *keep_of_locus, int niso, int j)
{
   if (!keep_of_locus) return j < niso;
   return (ctx_kept_word(keep_of_locus, niso, SBGPU_EM_OK, j >> 5) >> (j & 31)) & 1u;
}

// The status of a locus of K kept isoforms
__host__ __device__ inline int32_t loo_locus_status(int64_t K) { return K == 0 ? SBGPU_LOO_EMPTY : K > kLooMaxKept ? SBGPU_LOO_TOO_WIDE : SBGPU_LOO_OK; }

// Sub-problems of a locus of K kept isoforms: the base, and one per kept isoform where there are two or more
__host__ __device__ inline int64_t loo_n_sub(int64_t K) { return loo_locus_status(K) != SBGPU_LOO_OK ? 0 : K >= 2 ? K + 1 : 1; }
// Columns of sub-problem s of such a locus (s = 0: the base)
__host__ __device__ inline int64_t loo_sub_cols(int64_t K, int64_t s) { return s == 0 ? K : K - 1; }
// Column c of the sub-problem that drops the kept isoform of rank `drop` (-1: the base) is the kept isoform of this rank
__host__ __device__ inline int loo_sub_rank(int c, int drop) { return drop >= 0 && c >= drop ? c + 1 : c; }

// What one tested isoform (kept rank r of K >= 2) gets.  theta_base [K]: the base's theta; theta_sub [K - 1]: its sub-problem's;
// kept_col [K]: the locus-local index of every kept isoform; fragments the fit could not place (n_dropped + n_impossible) in
// the sub-problem (lost_sub) and in the base (lost_base); the two log-likelihoods.
struct LooIsoform {
   long long n_unique;
   double lr_stat, heir_gain;
   int32_t heir;
};
__host__ __device__ inline LooIsoform loo_isoform(int K, int r, const double *theta_base, const double *theta_sub, const int32_t *kept_col,
                                                  long long lost_sub, long long lost_base, double loglik_sub, double loglik_base)
{
   LooIsoform o;
   o.n_unique = lost_sub - lost_base;
   o.lr_stat = o.n_unique > 0 ? (double)INFINITY : 2.0 * (loglik_base - loglik_sub);
   o.heir = -1, o.heir_gain = 0.0;
   for (int k = 0; k < K; ++k) {
      if (k == r) continue;
      const double gain = theta_sub[k < r ? k : k - 1] - theta_base[k];
      if (gain > o.heir_gain) o.heir_gain = gain, o.heir = kept_col[k];
   }
   return o;
}

} // namespace sb


namespace sb {

// Rules 1, 2 and 9 for a whole batch (host only; the offsets are the caller's to check): what both forms make first
struct LooShapes {
   std::vector<int32_t> loo_status; // [n_loci]
   std::vector<int32_t> rank;       // [n_iso] the kept rank of an isoform of an OK locus; -1: not kept; -2: kept, its locus is not OK
   std::vector<int64_t> first_sub;  // [n_loci] the number of the locus' base among all sub-problems, -1 where the locus is not OK
   std::vector<int64_t> kept_off;   // [n_loci + 1] into kept_col (the OK loci's kept isoforms)
   std::vector<int32_t> kept_col;   // locus-local indices, ascending
   std::vector<int32_t> sub_locus, sub_drop;                // [n_sub]
   std::vector<int64_t> sub_row_off, sub_iso_off, sub_f_off; // [n_sub + 1]
   std::vector<int64_t> without_off; // [n_iso + 1]
   int64_t n_sub() const { return (int64_t)sub_locus.size(); }
};
inline void loo_shapes(int64_t n_loci, const int64_t *row_off, const int64_t *iso_off, const int32_t *keep, LooShapes *o)
{
   const int64_t n_iso = iso_off[n_loci];
   o->loo_status.assign((size_t)n_loci, SBGPU_LOO_OK), o->first_sub.assign((size_t)n_loci, -1), o->kept_off.assign((size_t)n_loci + 1, 0);
   o->rank.assign((size_t)n_iso, -1), o->without_off.assign((size_t)n_iso + 1, 0);
   o->kept_col.clear(), o->sub_locus.clear(), o->sub_drop.clear();
   o->sub_row_off.assign(1, 0), o->sub_iso_off.assign(1, 0), o->sub_f_off.assign(1, 0);
   std::vector<int32_t> cols;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t i0 = iso_off[l], nb = row_off ? row_off[l + 1] - row_off[l] : 0;
      const int niso = (int)(iso_off[l + 1] - i0);
      cols.clear();
      for (int j = 0; j < niso; ++j)
         if (loo_kept(keep ? keep + i0 : nullptr, niso, j)) cols.push_back(j);
      const int64_t K = (int64_t)cols.size();
      const int32_t st = loo_locus_status(K);
      o->loo_status[(size_t)l] = st;
      for (int64_t r = 0; r < K; ++r) o->rank[(size_t)(i0 + cols[(size_t)r])] = st == SBGPU_LOO_OK ? (int32_t)r : -2;
      if (st == SBGPU_LOO_OK) {
         o->first_sub[(size_t)l] = o->n_sub();
         o->kept_col.insert(o->kept_col.end(), cols.begin(), cols.end());
         for (int64_t s = 0; s < loo_n_sub(K); ++s) {
            const int64_t c = loo_sub_cols(K, s);
            o->sub_locus.push_back((int32_t)l), o->sub_drop.push_back(s == 0 ? -1 : cols[(size_t)s - 1]);
            o->sub_row_off.push_back(o->sub_row_off.back() + nb), o->sub_iso_off.push_back(o->sub_iso_off.back() + c);
            o->sub_f_off.push_back(o->sub_f_off.back() + nb * c);
         }
      }
      o->kept_off[(size_t)l + 1] = (int64_t)o->kept_col.size();
      for (int j = 0; j < niso; ++j) {
         const bool tested = st == SBGPU_LOO_OK && K >= 2 && o->rank[(size_t)(i0 + j)] >= 0;
         o->without_off[(size_t)(i0 + j) + 1] = o->without_off[(size_t)(i0 + j)] + (tested ? K - 1 : 0);
      }
   }
}

} // namespace sb
