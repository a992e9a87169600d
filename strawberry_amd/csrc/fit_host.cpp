// strawberry_amd/csrc/fit_host.cpp -- sbgpu_em_fit_host (include/sbgpu.h): how well theta explains every locus' bin counts, on
// the host.  The one CPU statement of what csrc/fit_device.h computes: every decision is a function of fit_rules.h (and, through
// it, of assign_rules.h), which the kernels call too.  Every sum runs in ascending order.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "fit_rules.h"
#include "stage_host.h"

using sb::api_fail;

extern "C" int sbgpu_em_fit_host(const sbgpu_batch_t *batch, const double *theta, const int32_t *keep, const int32_t *status, sbgpu_em_fit_t *out)
{
   if (!batch || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: null argument");
   if (!theta) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: theta is needed (the fit is theta's: give the EM's, or another estimate)");
   const int64_t nl = batch->n_loci;
   const int64_t *row_off = batch->row_off, *iso_off = batch->iso_off, *f_off = batch->f_off;
   if (nl < 0 || !row_off || !iso_off || !f_off) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: bad n_loci or null offset array");
   if (row_off[0] != 0 || iso_off[0] != 0 || f_off[0] != 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = row_off[l + 1] - row_off[l], niso = iso_off[l + 1] - iso_off[l];
      if (nb < 0 || niso < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: malformed offsets: row_off / iso_off do not ascend");
      if (niso > INT32_MAX || nb > INT32_MAX) return api_fail(SBGPU_ESHAPE, "sbgpu_em_fit_host: a locus of more than 2^31 - 1 bins or isoforms");
      if (f_off[l + 1] - f_off[l] != nb * niso) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: malformed offsets: f_off[l + 1] - f_off[l] is not rows x isoforms");
   }
   const int64_t n_bins = row_off[nl], n_iso = iso_off[nl], n_elem = f_off[nl];
   const int32_t *count = batch->count;
   const double *F = batch->F;
   if ((n_bins && !count) || (n_elem && !F)) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: null count or F");
   for (int64_t b = 0; b < n_bins; ++b)
      if (count[b] < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_host: a negative count");
   out->d_expected = nullptr, out->d_resid = nullptr, out->d_score = nullptr;
   out->d_loglik = nullptr, out->d_deviance = nullptr, out->d_pearson = nullptr;
   out->d_n_live = nullptr, out->d_n_dropped = nullptr, out->d_n_impossible = nullptr;
   out->d_dof = nullptr, out->d_worst_bin = nullptr;
   std::vector<uint32_t> kept;
   std::vector<uint8_t> live, possible;
   std::vector<double> c, g, d, e, r;
   std::vector<int32_t> all_kept;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t b0 = row_off[l], i0 = iso_off[l], f0 = f_off[l];
      const int nb = (int)(row_off[l + 1] - b0), niso = (int)(iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const double *Fl = F + f0;
      const int32_t *n = count + b0;
      // ---- rule 1: kept, live, c_j, g_j: the assignment's
      kept.assign((size_t)words + 1, 0u);
      sb::kept_words(keep ? keep + i0 : nullptr, niso, status ? status + l : nullptr, all_kept, kept.data());
      uint32_t any_kept = 0;
      for (int w = 0; w < words; ++w) any_kept |= kept[(size_t)w];
      live.assign((size_t)nb + 1, 0), possible.assign((size_t)nb + 1, 0);
      c.assign((size_t)niso + 1, 0.0), g.assign((size_t)niso + 1, 0.0);
      sb::column_pass_locus(Fl, nb, niso, theta + i0, kept.data(), live.data(), g.data(), c.data());
      int64_t A = 0;
      for (int j = 0; j < niso; ++j) A += g[(size_t)j] > 0.0;
      d.assign((size_t)nb + 1, 0.0), e.assign((size_t)nb + 1, 0.0), r.assign((size_t)nb + 1, 0.0);
      int64_t n_live = 0, n_dropped = 0, n_impossible = 0, P = 0;
      double D = 0.0, loglik = 0.0, dev = 0.0, pearson = 0.0, best = -1.0;
      int32_t best_b = INT32_MAX;
      if (!any_kept) {
         // a locus whose EM never started, or with nothing kept: zeros; its fragments are counted as dropped, live row or not
         for (int b = 0; b < nb; ++b) n_dropped += n[b];
         A = 0;
      } else {
         // ---- rules 2-4: the bins' masses, who is possible, the counts, D
         for (int b = 0; b < nb; ++b) {
            if (!live[(size_t)b]) {
               n_dropped += n[b];
               continue;
            }
            n_live += n[b];
            d[(size_t)b] = sb::fit_bin_mass(Fl + (int64_t)b * niso, niso, kept.data(), g.data());
            possible[(size_t)b] = sb::fit_possible(true, d[(size_t)b]);
            if (possible[(size_t)b]) ++P, D += d[(size_t)b];
            else n_impossible += n[b], d[(size_t)b] = 0.0;
         }
         const int64_t M = n_live - n_impossible;
         // ---- rules 5-9, 11
         for (int b = 0; b < nb; ++b) {
            if (!possible[(size_t)b]) continue;
            e[(size_t)b] = sb::fit_expected(M, d[(size_t)b], D);
            r[(size_t)b] = sb::fit_resid(n[b], e[(size_t)b]);
            if (n[b] > 0) loglik += sb::fit_loglik_term(n[b], d[(size_t)b], D), dev += sb::fit_deviance_term(n[b], e[(size_t)b]);
            pearson += r[(size_t)b] * r[(size_t)b];
            const double ra = fabs(r[(size_t)b]);
            if (sb::fit_worse(ra, b, best, best_b)) best = ra, best_b = b;
         }
      }
      if (out->expected) std::copy(e.begin(), e.begin() + nb, out->expected + b0);
      if (out->resid) std::copy(r.begin(), r.begin() + nb, out->resid + b0);
      if (out->loglik) out->loglik[l] = loglik;
      if (out->deviance) out->deviance[l] = 2.0 * dev;
      if (out->pearson) out->pearson[l] = pearson;
      if (out->n_live) out->n_live[l] = n_live;
      if (out->n_dropped) out->n_dropped[l] = n_dropped;
      if (out->n_impossible) out->n_impossible[l] = n_impossible;
      if (out->dof) out->dof[l] = any_kept ? sb::fit_dof(P, A) : 0;
      if (out->worst_bin) out->worst_bin[l] = best_b == INT32_MAX ? -1 : best_b;
      // ---- rule 12: the score, a column at a time over the possible bins in ascending order
      if (out->score)
         for (int j = 0; j < niso; ++j) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b)
               if (possible[(size_t)b]) s += sb::fit_score_term(sb::fit_ratio(n[b], d[(size_t)b]), Fl[(int64_t)b * niso + j]);
            out->score[i0 + j] = sb::fit_score(s, c[(size_t)j], (kept[(size_t)(j >> 5)] >> (j & 31)) & 1u);
         }
   }
   return SBGPU_OK;
}
