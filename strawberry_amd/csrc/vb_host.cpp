// strawberry_amd/csrc/vb_host.cpp -- sbgpu_em_vb_host (include/sbgpu.h): the variational Bayes solve of every locus, on the
// host.  The one CPU statement of what csrc/vb_device.h computes: every decision is a function of vb_rules.h, which the kernels
// call too.  Every sum runs in ascending order.  No kernels here, and nothing of HIP: a plain C++ compiler takes this file with
// vb_rules.h and stage_host.h.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "stage_host.h"
#include "vb_rules.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (api_internal.h; a stand-alone program over this file defines its own)
}
using sb::api_fail;

extern "C" int sbgpu_em_vb_host(const sbgpu_batch_t *batch, const sbgpu_vb_params_t *params, sbgpu_em_vb_t *out)
{
   const std::string who = "sbgpu_em_vb_host";
   if (!batch || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   sb::VbParams P;
   if (!sb::vb_params(params, &P)) return api_fail(SBGPU_EINVAL, who + ": alpha outside [1e-6, 1e3], change_limit <= 0 or max_iter < 1");
   const int64_t nl = batch->n_loci;
   const int64_t *row_off = batch->row_off, *iso_off = batch->iso_off, *f_off = batch->f_off;
   if (nl < 0 || !row_off || !iso_off || !f_off) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
   if (row_off[0] != 0 || iso_off[0] != 0 || f_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = row_off[l + 1] - row_off[l], niso = iso_off[l + 1] - iso_off[l];
      if (nb < 0 || niso < 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: row_off / iso_off do not ascend");
      if (nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > sb::kVbMaxIso) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 512 isoforms");
      if (f_off[l + 1] - f_off[l] != nb * niso) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: f_off[l + 1] - f_off[l] is not rows x isoforms");
   }
   const int64_t n_bins = row_off[nl], n_elem = f_off[nl];
   const int32_t *count = batch->count;
   const double *F = batch->F;
   if ((n_bins && !count) || (n_elem && !F)) return api_fail(SBGPU_EINVAL, who + ": null count or F");
   for (int64_t b = 0; b < n_bins; ++b)
      if (count[b] < 0) return api_fail(SBGPU_EINVAL, who + ": a negative count");
   out->d_count = nullptr, out->d_share = nullptr, out->d_share_sd = nullptr, out->d_status = nullptr, out->d_iters = nullptr;
   out->d_elbo = nullptr, out->d_n_active = nullptr, out->d_n_frag = nullptr;
   const double alpha = P.alpha;
   std::vector<double> A, r, s, c, w, cn;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t b0 = row_off[l], i0 = iso_off[l];
      const int nb = (int)(row_off[l + 1] - b0), niso = (int)(iso_off[l + 1] - i0);
      const double *Fl = F + f_off[l];
      const int32_t *n = count + b0;
      // ---- rules 1-3: the live bins (r < 0: not live), the columns' sums, who is active, N, the start
      r.assign((size_t)nb + 1, 0.0), s.assign((size_t)niso + 1, 0.0), c.assign((size_t)niso + 1, 0.0);
      w.assign((size_t)niso + 1, 0.0), cn.assign((size_t)niso + 1, 0.0), A.assign((size_t)nb * niso + 1, 0.0);
      int n_live = 0;
      int64_t N = 0;
      for (int i = 0; i < nb; ++i) {
         const bool live = sb::asg_row_live(Fl + (int64_t)i * niso, niso);
         r[(size_t)i] = live ? 0.0 : -1.0;
         if (live) ++n_live, N += n[i];
      }
      int32_t ka = 0;
      for (int j = 0; j < niso; ++j) {
         double sj = 0.0;
         for (int i = 0; i < nb; ++i)
            if (!(r[(size_t)i] < 0.0)) sj += Fl[(int64_t)i * niso + j];
         s[(size_t)j] = sj;
         ka += sj > 0.0;
      }
      for (int64_t e = 0; e < (int64_t)nb * niso; ++e) A[(size_t)e] = sb::vb_norm(Fl[e], s[(size_t)(e % niso)]);
      int32_t status = SBGPU_EM_MAXITER, iters = 0;
      double elbo = 0.0;
      const bool solved = n_live > 0 && N > 0;
      if (!n_live) status = SBGPU_EM_INIT_EMPTY, ka = 0;
      else if (N == 0) status = SBGPU_EM_OK, iters = 1;
      if (solved) {
         for (int j = 0; j < niso; ++j) c[(size_t)j] = s[(size_t)j] > 0.0 ? (double)N / (double)ka : 0.0;
         // ---- rule 5
         for (int it = 0; it < P.max_iter; ++it) {
            iters = it + 1;
            double m = -std::numeric_limits<double>::infinity();
            for (int j = 0; j < niso; ++j)
               if (s[(size_t)j] > 0.0) w[(size_t)j] = sb::vb_digamma(alpha + c[(size_t)j]), m = std::max(m, w[(size_t)j]);
            for (int j = 0; j < niso; ++j) w[(size_t)j] = s[(size_t)j] > 0.0 ? exp(w[(size_t)j] - m) : 0.0;
            bool zero = false;
            for (int i = 0; i < nb; ++i) {
               if (r[(size_t)i] < 0.0) continue;
               const double d = sb::vb_bin_mass(A.data() + (int64_t)i * niso, w.data(), niso);
               zero |= sb::vb_denom_zero(n[i], d);
               r[(size_t)i] = sb::vb_ratio(n[i], d);
            }
            if (zero) {
               status = SBGPU_EM_DENOM_ZERO;
               break;
            }
            double sq = 0.0;
            for (int j = 0; j < niso; ++j) {
               if (!(s[(size_t)j] > 0.0)) continue;
               cn[(size_t)j] = sb::vb_next(w[(size_t)j], sb::vb_col_sum(A.data(), r.data(), nb, niso, j));
               sq = sb::vb_step_term(cn[(size_t)j], c[(size_t)j], sq);
            }
            if (sqrt(sq) < P.change_limit) {
               status = SBGPU_EM_OK;
               break;
            }
            std::swap(c, cn);
         }
         // ---- rule 6
         const double a0 = sb::vb_a0(ka, alpha, N), psi0 = sb::vb_digamma(a0);
         double lg = 0.0, cl = 0.0, bins = 0.0;
         for (int j = 0; j < niso; ++j) {
            w[(size_t)j] = 0.0;
            if (!(s[(size_t)j] > 0.0)) continue;
            const double lw = sb::vb_digamma(alpha + c[(size_t)j]) - psi0;
            w[(size_t)j] = exp(lw);
            lg += lgamma(alpha + c[(size_t)j]);
            cl = fma(c[(size_t)j], lw, cl);
         }
         for (int i = 0; i < nb; ++i)
            if (!(r[(size_t)i] < 0.0) && n[i] > 0) bins += (double)n[i] * log(sb::vb_bin_mass(A.data() + (int64_t)i * niso, w.data(), niso));
         elbo = sb::vb_elbo(bins, a0, lg, cl, ka, alpha);
      }
      // ---- rule 7
      const double a0 = sb::vb_a0(ka, alpha, N);
      for (int j = 0; j < niso; ++j) {
         const bool on = solved && s[(size_t)j] > 0.0;
         if (out->count) out->count[i0 + j] = on ? c[(size_t)j] : 0.0;
         if (out->share) out->share[i0 + j] = on ? sb::vb_share(alpha, c[(size_t)j], a0) : 0.0;
         if (out->share_sd) out->share_sd[i0 + j] = on ? sb::vb_share_sd(alpha, c[(size_t)j], a0) : 0.0;
      }
      if (out->status) out->status[l] = status;
      if (out->iters) out->iters[l] = iters;
      if (out->elbo) out->elbo[l] = elbo;
      if (out->n_active) out->n_active[l] = ka;
      if (out->n_frag) out->n_frag[l] = n_live ? N : 0;
   }
   return SBGPU_OK;
}
