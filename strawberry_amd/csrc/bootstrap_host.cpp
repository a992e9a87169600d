// strawberry_amd/csrc/bootstrap_host.cpp -- sbgpu_bootstrap_counts_host (include/sbgpu.h): one bootstrap replicate's bin
// counts on the host, sbgpu_replicate_stats_host: the replicates' statistics, and sbgpu_locus_abundance_host: abundances per locus.  The one CPU statement of what csrc/bootstrap_device.h computes: every draw is a function of
// bootstrap_rules.h, which the kernels call too.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "bootstrap_rules.h"

using sb::api_fail;

extern "C" int sbgpu_bootstrap_counts_host(int64_t n_loci, const int64_t *row_off, const int32_t *count, const int64_t *locus_id, uint64_t seed,
                                           int32_t rep, int32_t *count_out)
{
   if (n_loci < 0 || !row_off) return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_counts_host: null offsets or a negative locus count");
   if (rep < 0 || rep >= sb::kBootMaxRep) return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_counts_host: the replicate number must lie in [0, 2^24)");
   for (int64_t l = 0; l < n_loci; ++l)
      if (row_off[l + 1] < row_off[l] || row_off[l + 1] - row_off[l] > INT32_MAX)
         return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_counts_host: row_off must not decrease (locus " + std::to_string(l) + ")");
   if (n_loci && row_off[n_loci] > row_off[0] && (!count || !count_out)) return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_counts_host: null count array");
   // all of the input is looked at before anything is written
   for (int64_t l = 0; l < n_loci; ++l) {
      int64_t N = 0;
      for (int64_t i = row_off[l]; i < row_off[l + 1]; ++i) {
         if (count[i] < 0) return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_counts_host: negative count in row " + std::to_string(i));
         N += count[i];
      }
      if (N >= sb::kBootMaxDraws) return api_fail(SBGPU_ESHAPE, "sbgpu_bootstrap_counts_host: locus " + std::to_string(l) + " holds 2^40 fragments or more");
   }
   std::vector<int64_t> incl;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t r0 = row_off[l];
      const int32_t nr = (int32_t)(row_off[l + 1] - r0);
      incl.resize((size_t)nr);
      int64_t N = 0;
      for (int32_t i = 0; i < nr; ++i) {
         N += count[r0 + i];
         incl[(size_t)i] = N;
         count_out[r0 + i] = 0;
      }
      const int64_t g = locus_id ? locus_id[l] : l;
      for (int64_t q = 0; 2 * q < N; ++q) {
         uint64_t t[2];
         sb::boot_draw_pair(g, rep, seed, q, N, t);
         ++count_out[r0 + sb::boot_row_of(incl.data(), nr, t[0])];
         if (2 * q + 1 < N) ++count_out[r0 + sb::boot_row_of(incl.data(), nr, t[1])];
      }
   }
   return SBGPU_OK;
}

// sbgpu_replicate_stats_host: mean, variance and two order statistics of every column of x[n_rep][n], by the rules of
// bootstrap_rules.h (the kernel boot_interval_kernel calls the same functions).  No cap on n_rep here.
extern "C" int sbgpu_replicate_stats_host(int32_t n_rep, int64_t n, const double *x, int32_t rank_lo, int32_t rank_hi, double *mean, double *var,
                                          double *lo, double *hi)
{
   if (n_rep < 1 || n < 0) return api_fail(SBGPU_EINVAL, "sbgpu_replicate_stats_host: n_rep must be at least 1 and n at least 0");
   if (rank_lo < 0 || rank_lo > rank_hi || rank_hi >= n_rep)
      return api_fail(SBGPU_EINVAL, "sbgpu_replicate_stats_host: the ranks must satisfy 0 <= rank_lo <= rank_hi < n_rep");
   if (n && !x) return api_fail(SBGPU_EINVAL, "sbgpu_replicate_stats_host: null matrix");
   std::vector<uint64_t> key((size_t)n_rep);
   for (int64_t j = 0; j < n; ++j) {
      double m = 0.0, q = 0.0;
      for (int32_t k = 0; k < n_rep; ++k) {
         const double v = x[(size_t)k * (size_t)n + (size_t)j];
         sb::boot_welford_step(v, k, m, q);
         key[(size_t)k] = sb::boot_sort_key(v);
      }
      if (mean) mean[j] = m;
      if (var) var[j] = sb::boot_welford_var(q, n_rep);
      if (lo || hi) std::sort(key.begin(), key.end());
      if (lo) lo[j] = sb::boot_key_value(key[(size_t)rank_lo]);
      if (hi) hi[j] = sb::boot_key_value(key[(size_t)rank_hi]);
   }
   return SBGPU_OK;
}

// sbgpu_locus_abundance_host: the loci's kept-FPKM sums, their numbers of kept isoforms and their TPM, by boot_locus_sum /
// boot_locus_tpm of bootstrap_rules.h (boot_locus_sum_kernel calls the same functions).
extern "C" int sbgpu_locus_abundance_host(int64_t n_loci, const int64_t *iso_off, const double *fpkm, const int32_t *keep, double total_fpkm,
                                          double *locus_fpkm, double *locus_tpm, int32_t *locus_kept)
{
   if (n_loci < 0 || !iso_off) return api_fail(SBGPU_EINVAL, "sbgpu_locus_abundance_host: null iso_off or a negative locus count");
   if (iso_off[0] < 0) return api_fail(SBGPU_EINVAL, "sbgpu_locus_abundance_host: iso_off must start at 0 or above");
   for (int64_t l = 0; l < n_loci; ++l)
      if (iso_off[l + 1] < iso_off[l]) return api_fail(SBGPU_EINVAL, "sbgpu_locus_abundance_host: iso_off must not decrease (locus " + std::to_string(l) + ")");
   if (iso_off[n_loci] > iso_off[0] && (!fpkm || !keep)) return api_fail(SBGPU_EINVAL, "sbgpu_locus_abundance_host: null fpkm or keep array");
   for (int64_t l = 0; l < n_loci; ++l) {
      double sum;
      int32_t kept;
      sb::boot_locus_sum(fpkm, keep, iso_off[l], iso_off[l + 1], sum, kept);
      if (locus_fpkm) locus_fpkm[l] = sum;
      if (locus_kept) locus_kept[l] = kept;
      if (locus_tpm) locus_tpm[l] = sb::boot_locus_tpm(sum, kept, total_fpkm);
   }
   return SBGPU_OK;
}
