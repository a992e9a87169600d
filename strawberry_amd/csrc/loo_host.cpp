// strawberry_amd/csrc/loo_host.cpp -- sbgpu_em_loo_offsets, sbgpu_em_loo_shapes_host, sbgpu_em_loo_expand_host,
// sbgpu_em_loo_stat_host (include/sbgpu.h): the drop-one isoform support on the host, in three calls around the caller's solve
// of the sub-batch (the library has no CPU EM).  The one CPU statement of what csrc/loo_device.h computes: every decision is a
// function of loo_rules.h, which the kernels call too.  No kernels and no HIP here: a plain C++ compiler takes this file (the
// library's error slot, sb::api_fail, is declared below instead of through api_internal.h).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "loo_rules.h"
#include "stage_host.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (sbgpu_api.hip) records sbgpu_last_error(), returns code
}
using sb::api_fail;

namespace {

// the offsets of a batch: begin at 0, ascend; row_off may be null (the statistics do not read the bins)
int check_offsets(const std::string &who, int64_t nl, const int64_t *row_off, const int64_t *iso_off, bool limits)
{
   if (nl < 0 || !iso_off) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
   if (iso_off[0] != 0 || (row_off && row_off[0] != 0)) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = row_off ? row_off[l + 1] - row_off[l] : 0, niso = iso_off[l + 1] - iso_off[l];
      if (nb < 0 || niso < 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: row_off / iso_off do not ascend");
      if (limits && nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > 32 * (int64_t)sb::kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
   }
   return SBGPU_OK;
}

template <class T>
void fill(T *out, const std::vector<T> &v)
{
   if (out) std::copy(v.begin(), v.end(), out);
}

} // namespace

extern "C" int sbgpu_em_loo_offsets(const int64_t *iso_off, const int32_t *keep, int64_t n_loci, int64_t *without_off)
{
   const std::string who = "sbgpu_em_loo_offsets";
   if (!iso_off || !without_off) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (const int rc = check_offsets(who, n_loci, nullptr, iso_off, false); rc != SBGPU_OK) return rc;
   sb::LooShapes sh;
   sb::loo_shapes(n_loci, nullptr, iso_off, keep, &sh);
   fill(without_off, sh.without_off);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_loo_shapes_host(int64_t n_loci, const int64_t *row_off, const int64_t *iso_off, const int32_t *keep, int64_t sizes[4],
                                        int32_t *loo_status, int32_t *sub_locus, int32_t *sub_drop, int64_t *sub_row_off, int64_t *sub_iso_off,
                                        int64_t *sub_f_off)
{
   const std::string who = "sbgpu_em_loo_shapes_host";
   if (!row_off || !iso_off || !sizes) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (const int rc = check_offsets(who, n_loci, row_off, iso_off, true); rc != SBGPU_OK) return rc;
   sb::LooShapes sh;
   sb::loo_shapes(n_loci, row_off, iso_off, keep, &sh);
   sizes[0] = sh.n_sub(), sizes[1] = sh.sub_row_off.back(), sizes[2] = sh.sub_iso_off.back(), sizes[3] = sh.sub_f_off.back();
   fill(loo_status, sh.loo_status), fill(sub_locus, sh.sub_locus), fill(sub_drop, sh.sub_drop);
   fill(sub_row_off, sh.sub_row_off), fill(sub_iso_off, sh.sub_iso_off), fill(sub_f_off, sh.sub_f_off);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_loo_expand_host(const sbgpu_batch_t *batch, const int32_t *keep, int32_t *sub_count, double *sub_F)
{
   const std::string who = "sbgpu_em_loo_expand_host";
   if (!batch) return api_fail(SBGPU_EINVAL, who + ": null argument");
   const int64_t nl = batch->n_loci;
   const int64_t *row_off = batch->row_off, *iso_off = batch->iso_off, *f_off = batch->f_off;
   if (!row_off || !f_off) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
   if (const int rc = check_offsets(who, nl, row_off, iso_off, true); rc != SBGPU_OK) return rc;
   if (f_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l)
      if (f_off[l + 1] - f_off[l] != (row_off[l + 1] - row_off[l]) * (iso_off[l + 1] - iso_off[l]))
         return api_fail(SBGPU_EINVAL, who + ": malformed offsets: f_off[l + 1] - f_off[l] is not rows x isoforms");
   const int32_t *count = batch->count;
   const double *F = batch->F;
   if ((row_off[nl] && !count) || (f_off[nl] && !F)) return api_fail(SBGPU_EINVAL, who + ": null count or F");
   for (int64_t b = 0; b < row_off[nl]; ++b)
      if (count[b] < 0) return api_fail(SBGPU_EINVAL, who + ": a negative count");
   sb::LooShapes sh;
   sb::loo_shapes(nl, row_off, iso_off, keep, &sh);
   if ((sh.sub_row_off.back() && !sub_count) || (sh.sub_f_off.back() && !sub_F)) return api_fail(SBGPU_EINVAL, who + ": null sub_count or sub_F");
   for (int64_t s = 0; s < sh.n_sub(); ++s) {
      const int64_t l = sh.sub_locus[(size_t)s], nb = row_off[l + 1] - row_off[l], niso = iso_off[l + 1] - iso_off[l];
      const int32_t *kc = sh.kept_col.data() + sh.kept_off[(size_t)l];
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      const int drop = (int)(s - sh.first_sub[(size_t)l]) - 1; // the dropped isoform's kept rank, -1: the base
      const int cols = (int)sb::loo_sub_cols(K, drop + 1);
      std::copy(count + row_off[l], count + row_off[l + 1], sub_count + sh.sub_row_off[(size_t)s]);
      const double *Fl = F + f_off[l];
      double *o = sub_F + sh.sub_f_off[(size_t)s];
      for (int64_t b = 0; b < nb; ++b)
         for (int c = 0; c < cols; ++c) o[b * cols + c] = Fl[b * niso + kc[sb::loo_sub_rank(c, drop)]];
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_em_loo_stat_host(int64_t n_loci, const int64_t *iso_off, const int32_t *keep, const double *sub_theta, const int32_t *sub_status,
                                      const int32_t *sub_iters, const double *sub_loglik, const int64_t *sub_n_live, const int64_t *sub_n_dropped,
                                      const int64_t *sub_n_impossible, sbgpu_em_loo_t *out)
{
   const std::string who = "sbgpu_em_loo_stat_host";
   if (!iso_off || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (const int rc = check_offsets(who, n_loci, nullptr, iso_off, false); rc != SBGPU_OK) return rc;
   sb::LooShapes sh;
   sb::loo_shapes(n_loci, nullptr, iso_off, keep, &sh);
   if (sh.n_sub() && (!sub_theta || !sub_status || !sub_iters || !sub_loglik || !sub_n_live || !sub_n_dropped || !sub_n_impossible))
      return api_fail(SBGPU_EINVAL, who + ": a null array of the sub-batch's solve or fit");
   const int64_t n_iso = iso_off[n_loci];
   if (out->theta_without) {
      if (!out->without_off) return api_fail(SBGPU_EINVAL, who + ": theta_without is given without without_off (sbgpu_em_loo_offsets makes it)");
      if (!std::equal(sh.without_off.begin(), sh.without_off.end(), out->without_off))
         return api_fail(SBGPU_EINVAL, who + ": without_off is not sbgpu_em_loo_offsets' for this batch");
   }
   out->d_lr_stat = nullptr, out->d_heir_gain = nullptr, out->d_theta_refit = nullptr, out->d_n_unique = nullptr;
   out->d_heir = nullptr, out->d_status_without = nullptr, out->d_iters_without = nullptr, out->d_support = nullptr;
   out->d_loglik_base = nullptr, out->d_loo_status = nullptr, out->d_status_base = nullptr, out->d_iters_base = nullptr;
   out->d_theta_without = nullptr, out->d_without_off = nullptr;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t fs = sh.first_sub[(size_t)l];
      const bool ok = fs >= 0;
      if (out->loo_status) out->loo_status[l] = sh.loo_status[(size_t)l];
      if (out->loglik_base) out->loglik_base[l] = ok ? sub_loglik[fs] : 0.0;
      if (out->status_base) out->status_base[l] = ok ? sub_status[fs] : -1;
      if (out->iters_base) out->iters_base[l] = ok ? sub_iters[fs] : -1;
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      const int32_t *kc = sh.kept_col.data() + sh.kept_off[(size_t)l];
      const double *tb = ok ? sub_theta + sh.sub_iso_off[(size_t)fs] : nullptr;
      for (int64_t i = iso_off[l]; i < iso_off[l + 1]; ++i) {
         const int r = sh.rank[(size_t)i];
         sb::LooIsoform o{0, 0.0, 0.0, -1};
         int32_t stw = -1, itw = -1, supp = r == -1 ? SBGPU_LOO_NOT_KEPT : SBGPU_LOO_LOCUS_SKIPPED;
         if (r >= 0 && K == 1) {
            supp = SBGPU_LOO_SOLE;
            o.n_unique = sub_n_live[fs] - sub_n_impossible[fs], o.lr_stat = (double)INFINITY;
         } else if (r >= 0) {
            const int64_t s = fs + 1 + r;
            const double *ts = sub_theta + sh.sub_iso_off[(size_t)s];
            supp = SBGPU_LOO_TESTED, stw = sub_status[s], itw = sub_iters[s];
            o = sb::loo_isoform(K, r, tb, ts, kc, sub_n_dropped[s] + sub_n_impossible[s], sub_n_dropped[fs] + sub_n_impossible[fs], sub_loglik[s], sub_loglik[fs]);
            if (out->theta_without) std::copy(ts, ts + K - 1, out->theta_without + sh.without_off[(size_t)i]);
         }
         if (out->lr_stat) out->lr_stat[i] = o.lr_stat;
         if (out->heir_gain) out->heir_gain[i] = o.heir_gain;
         if (out->theta_refit) out->theta_refit[i] = r >= 0 ? tb[r] : 0.0;
         if (out->n_unique) out->n_unique[i] = o.n_unique;
         if (out->heir) out->heir[i] = o.heir;
         if (out->status_without) out->status_without[i] = stw;
         if (out->iters_without) out->iters_without[i] = itw;
         if (out->support) out->support[i] = supp;
      }
   }
   (void)n_iso;
   return SBGPU_OK;
}
