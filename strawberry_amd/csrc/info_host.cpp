// strawberry_amd/csrc/info_host.cpp -- sbgpu_em_info_host, sbgpu_em_info_cov_offsets (include/sbgpu.h): which isoforms of every
// locus the counted bins can tell apart, and the covariance of theta, on the host.  The one CPU statement of what
// csrc/info_device.h computes: every decision and every sum is a function of info_rules.h (and, through it, of fit_rules.h and
// assign_rules.h), which the kernels call too.  No kernels and no HIP here: a plain C++ compiler takes this file (the library's
// error slot, sb::api_fail, is declared below instead of through api_internal.h).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "info_rules.h"
#include "stage_host.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (sbgpu_api.hip) records sbgpu_last_error(), returns code
}
using sb::api_fail;

extern "C" int sbgpu_em_info_cov_offsets(const int64_t *iso_off, int64_t n_loci, int64_t *cov_off)
{
   if (!iso_off || !cov_off || n_loci < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_cov_offsets: null argument or bad n_loci");
   cov_off[0] = 0;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t niso = iso_off[l + 1] - iso_off[l];
      if (niso < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_cov_offsets: malformed offsets: iso_off does not ascend");
      cov_off[l + 1] = cov_off[l] + sb::info_cov_entries(niso);
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_em_info_host(const sbgpu_batch_t *batch, const double *theta, const int32_t *keep, const int32_t *status, sbgpu_em_info_t *out)
{
   if (!batch || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: null argument");
   if (!theta) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: theta is needed (the information is theta's: give the EM's, or another estimate)");
   const int64_t nl = batch->n_loci;
   const int64_t *row_off = batch->row_off, *iso_off = batch->iso_off, *f_off = batch->f_off;
   if (nl < 0 || !row_off || !iso_off || !f_off) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: bad n_loci or null offset array");
   if (row_off[0] != 0 || iso_off[0] != 0 || f_off[0] != 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = row_off[l + 1] - row_off[l], niso = iso_off[l + 1] - iso_off[l];
      if (nb < 0 || niso < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: malformed offsets: row_off / iso_off do not ascend");
      if (niso > INT32_MAX || nb > INT32_MAX) return api_fail(SBGPU_ESHAPE, "sbgpu_em_info_host: a locus of more than 2^31 - 1 bins or isoforms");
      if (f_off[l + 1] - f_off[l] != nb * niso) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: malformed offsets: f_off[l + 1] - f_off[l] is not rows x isoforms");
   }
   const int64_t n_bins = row_off[nl], n_elem = f_off[nl];
   const int32_t *count = batch->count;
   const double *F = batch->F;
   if ((n_bins && !count) || (n_elem && !F)) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: null count or F");
   for (int64_t b = 0; b < n_bins; ++b)
      if (count[b] < 0) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: a negative count");
   const int64_t *cov_off = out->cov_off;
   if (out->cov) {
      if (!cov_off) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: cov is given without cov_off (sbgpu_em_info_cov_offsets makes it)");
      bool good = cov_off[0] == 0;
      for (int64_t l = 0; l < nl && good; ++l) good = cov_off[l + 1] - cov_off[l] == sb::info_cov_entries(iso_off[l + 1] - iso_off[l]);
      if (!good) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_host: cov_off is not sbgpu_em_info_cov_offsets' for this batch");
   }
   out->d_se = nullptr, out->d_partner_corr = nullptr, out->d_ident = nullptr, out->d_alias_of = nullptr, out->d_partner = nullptr;
   out->d_min_pivot = nullptr, out->d_rank = nullptr, out->d_n_free = nullptr, out->d_info_status = nullptr;
   out->d_cov = nullptr, out->d_cov_off = nullptr;
   std::vector<uint32_t> kept;
   std::vector<uint8_t> live;
   std::vector<double> c, g, w;
   std::vector<int32_t> all_kept, idx;
   // the free isoforms' working set (info_rules.h: packed triangles over free-local indices)
   std::vector<double> A((size_t)sb::kInfoTri), B((size_t)sb::kInfoTri), cf(sb::kInfoMaxFree), dg(sb::kInfoMaxFree), ld(sb::kInfoMaxFree), piv(sb::kInfoMaxFree),
      u(sb::kInfoMaxFree), se(sb::kInfoMaxFree);
   std::vector<uint8_t> st(sb::kInfoMaxFree);
   std::vector<int32_t> alias(sb::kInfoMaxFree);
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t b0 = row_off[l], i0 = iso_off[l], f0 = f_off[l];
      const int nb = (int)(row_off[l + 1] - b0), niso = (int)(iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const double *Fl = F + f0;
      const int32_t *n = count + b0;
      // ---- rule 1: kept, live, c_j, g_j: the assignment's
      kept.assign((size_t)words + 1, 0u);
      sb::kept_words(keep ? keep + i0 : nullptr, niso, status ? status + l : nullptr, all_kept, kept.data());
      live.assign((size_t)nb + 1, 0);
      c.assign((size_t)niso + 1, 0.0), g.assign((size_t)niso + 1, 0.0);
      sb::column_pass_locus(Fl, nb, niso, theta + i0, kept.data(), live.data(), g.data(), c.data());
      // ---- rule 3: the free isoforms, in ascending order
      idx.clear();
      for (int j = 0; j < niso; ++j)
         if (sb::info_free(g[(size_t)j])) idx.push_back(j);
      const int64_t n_free = (int64_t)idx.size();
      const int32_t info_status = n_free == 0 ? SBGPU_INFO_EMPTY : n_free > sb::kInfoMaxFree ? SBGPU_INFO_TOO_WIDE : SBGPU_INFO_OK;
      // ---- the defaults: what an EMPTY or TOO_WIDE locus, and an isoform that is not free, get
      for (int j = 0; j < niso; ++j) {
         if (out->se) out->se[i0 + j] = 0.0;
         if (out->partner_corr) out->partner_corr[i0 + j] = 0.0;
         if (out->ident) out->ident[i0 + j] = info_status == SBGPU_INFO_TOO_WIDE ? SBGPU_INFO_SKIPPED : SBGPU_INFO_NOT_FREE;
         if (out->alias_of) out->alias_of[i0 + j] = -1;
         if (out->partner) out->partner[i0 + j] = -1;
      }
      if (out->cov) std::fill(out->cov + cov_off[l], out->cov + cov_off[l + 1], 0.0);
      if (out->info_status) out->info_status[l] = info_status;
      if (out->n_free) out->n_free[l] = info_status == SBGPU_INFO_OK ? (int32_t)n_free : 0;
      if (out->rank) out->rank[l] = 0;
      if (out->min_pivot) out->min_pivot[l] = 0.0;
      if (info_status != SBGPU_INFO_OK) continue;
      const int nf = (int)n_free;
      // ---- rule 2: the bins' weights
      w.assign((size_t)nb + 1, 0.0);
      for (int b = 0; b < nb; ++b) {
         const double d = live[(size_t)b] ? sb::fit_bin_mass(Fl + (int64_t)b * niso, niso, kept.data(), g.data()) : 0.0;
         w[(size_t)b] = sb::info_weight(n[b], d, sb::fit_possible(live[(size_t)b], d));
      }
      // ---- rule 4: H over the free isoforms
      for (int p = 0; p < nf; ++p) cf[(size_t)p] = c[(size_t)idx[(size_t)p]];
      for (int i = 0; i < nf; ++i)
         for (int j = 0; j <= i; ++j)
            A[(size_t)sb::info_tri(i, j)] = sb::info_h(sb::info_wave_order_sum(w.data(), Fl, nb, niso, idx[(size_t)j], idx[(size_t)i]), cf[(size_t)j], cf[(size_t)i]);
      // ---- rules 5, 6: who is observed, the scaling
      for (int p = 0; p < nf; ++p) {
         const double h = A[(size_t)sb::info_tri(p, p)];
         const bool obs = sb::info_observed(h);
         st[(size_t)p] = obs ? sb::kInfoPending : SBGPU_INFO_UNOBSERVED;
         dg[(size_t)p] = obs ? sqrt(h) : 0.0;
         alias[(size_t)p] = -1, ld[(size_t)p] = 0.0, piv[(size_t)p] = 0.0, u[(size_t)p] = 0.0, se[(size_t)p] = 0.0;
      }
      for (int i = 0; i < nf; ++i)
         for (int j = 0; j <= i; ++j)
            if (st[(size_t)i] == sb::kInfoPending && st[(size_t)j] == sb::kInfoPending)
               A[(size_t)sb::info_tri(i, j)] = sb::info_scaled(A[(size_t)sb::info_tri(i, j)], dg[(size_t)i], dg[(size_t)j]);
      // ---- rule 7: the factorisation, a column at a time
      for (int j = 0; j < nf; ++j) {
         if (st[(size_t)j] != sb::kInfoPending) continue;
         const double pj = sb::info_pivot(A.data(), st.data(), j);
         piv[(size_t)j] = pj;
         if (!sb::info_retained(pj)) {
            alias[(size_t)j] = sb::info_alias_of(A.data(), st.data(), j);
            st[(size_t)j] = SBGPU_INFO_ALIASED;
            continue;
         }
         const double ljj = sqrt(pj);
         ld[(size_t)j] = ljj;
         for (int i = j + 1; i < nf; ++i)
            if (st[(size_t)i] == sb::kInfoPending) A[(size_t)sb::info_tri(i, j)] = sb::info_lower(A.data(), st.data(), i, j, ljj);
         st[(size_t)j] = SBGPU_INFO_IDENTIFIED;
      }
      int32_t rank = 0;
      double min_pivot = 0.0;
      for (int j = 0; j < nf; ++j)
         if (sb::info_in_r(st.data(), j)) {
            if (!rank || piv[(size_t)j] < min_pivot) min_pivot = piv[(size_t)j];
            ++rank;
         }
      // ---- rule 8: Y = L_R^-1 into B, V, Hinv into A
      for (int j = 0; j < nf; ++j)
         if (sb::info_in_r(st.data(), j))
            for (int i = j; i < nf; ++i)
               if (sb::info_in_r(st.data(), i)) B[(size_t)sb::info_tri(i, j)] = sb::info_y(A.data(), ld.data(), B.data(), st.data(), i, j);
      for (int i = 0; i < nf; ++i)
         for (int j = 0; j <= i; ++j) {
            const bool both = sb::info_in_r(st.data(), i) && sb::info_in_r(st.data(), j);
            A[(size_t)sb::info_tri(i, j)] = both ? sb::info_hinv(sb::info_v(B.data(), st.data(), nf, i, j), dg[(size_t)i], dg[(size_t)j]) : 0.0;
         }
      // ---- rule 9: the covariance on the simplex
      for (int i = 0; i < nf; ++i)
         if (sb::info_in_r(st.data(), i)) u[(size_t)i] = sb::info_u(A.data(), st.data(), nf, i);
      const double t = sb::info_t(u.data(), st.data(), nf);
      for (int i = 0; i < nf; ++i)
         for (int j = 0; j <= i; ++j)
            if (sb::info_in_r(st.data(), i) && sb::info_in_r(st.data(), j))
               A[(size_t)sb::info_tri(i, j)] = sb::info_cov(A[(size_t)sb::info_tri(i, j)], u[(size_t)i], u[(size_t)j], t);
      for (int j = 0; j < nf; ++j)
         if (sb::info_in_r(st.data(), j)) se[(size_t)j] = sb::info_se(A[(size_t)sb::info_tri(j, j)]);
      // ---- rules 10-13: the results
      for (int p = 0; p < nf; ++p) {
         const int64_t at = i0 + idx[(size_t)p];
         double corr = 0.0;
         const int k = sb::info_in_r(st.data(), p) ? sb::info_partner(A.data(), se.data(), st.data(), nf, p, &corr) : -1;
         if (out->se) out->se[at] = se[(size_t)p];
         if (out->partner_corr) out->partner_corr[at] = corr;
         if (out->ident) out->ident[at] = st[(size_t)p];
         if (out->alias_of) out->alias_of[at] = alias[(size_t)p] < 0 ? -1 : idx[(size_t)alias[(size_t)p]];
         if (out->partner) out->partner[at] = k < 0 ? -1 : idx[(size_t)k];
      }
      if (out->rank) out->rank[l] = rank;
      if (out->min_pivot) out->min_pivot[l] = min_pivot;
      if (out->cov && cov_off[l + 1] > cov_off[l])
         for (int i = 0; i < nf; ++i)
            for (int j = 0; j <= i; ++j)
               if (sb::info_in_r(st.data(), i) && sb::info_in_r(st.data(), j))
                  out->cov[cov_off[l] + sb::info_cov_at(niso, idx[(size_t)j], idx[(size_t)i])] = A[(size_t)sb::info_tri(i, j)];
   }
   return SBGPU_OK;
}
