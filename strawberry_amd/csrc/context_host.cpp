// strawberry_amd/csrc/context_host.cpp -- sbgpu_context_table_host (include/sbgpu.h): the `-f` fragment-context table
// as arrays, on the host.  The one CPU statement of what csrc/context_device.h computes: every decision is a function
// of context_rules.h, which the kernels call too.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "stage_host.h"

using sb::api_fail;

extern "C" int sbgpu_context_table_host(const sbgpu_bins_t *bins, const uint32_t *compat, int32_t compat_words, const double *F,
                                        const int32_t *keep, const int32_t *status, sbgpu_context_table_t *out)
{
   if (!bins || !out) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_host: null argument");
   const sb::BinsContextView v = sb::bins_context_view(bins);
   const int64_t nl = v.n_loci, nh = v.n_hits;
   const int cw = compat_words, kw = v.key_words;
   if (nh && (!compat || cw < 1)) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_host: the hits' compat words are needed");
   if (!F) F = v.F;
   if (!F && v.n_elem && out->row_prob)
      return api_fail(SBGPU_EINVAL, "sbgpu_context_table_host: this handle holds no weights (give F, or a handle from sbgpu_quantify_host)");
   out->n_rows = 0;
   out->d_locus_row_off = nullptr, out->d_locus_hits = nullptr, out->d_row_bin = nullptr, out->d_row_hits = nullptr, out->d_row_prob = nullptr;
   std::vector<int64_t> hit_bin((size_t)std::max<int64_t>(nh, 1), -1);
   std::vector<uint32_t> key((size_t)std::max<int64_t>(v.n_bins * kw, 1), 0u);
   if (const int rc = sbgpu_bins_export(bins, nullptr, nullptr, nullptr, nullptr, nullptr, key.data(), nullptr, hit_bin.data(), nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
       rc != SBGPU_OK)
      return rc;
   // the count pass: per bin, the qualifying hits and the last of them (hits in index order: a later one overwrites)
   std::vector<uint32_t> n_in_bin((size_t)v.n_bins + 1, 0u);
   std::vector<int64_t> last_hit((size_t)v.n_bins + 1, -1);
   std::vector<uint32_t> kept;
   std::vector<int32_t> all_kept;
   int64_t l = 0;
   auto kept_mask_of = [&](int64_t locus) {
      const int niso = (int)(v.iso_off[locus + 1] - v.iso_off[locus]);
      kept.assign((size_t)(niso + 31) / 32 + 1, 0u);
      return sb::kept_words(keep ? keep + v.iso_off[locus] : nullptr, niso, status ? status + locus : nullptr, all_kept, kept.data());
   };
   int64_t mask_locus = -1;
   int words = 0;
   for (int64_t h = 0; h < nh; ++h) {
      const int64_t b = hit_bin[(size_t)h];
      if (b < 0) continue;
      if (b >= v.n_bins) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_host: hit -> bin out of range");
      l = sb::locus_of_hit(h, b, l, nl, v.row_off, nullptr);
      if (l != mask_locus) {
         words = kept_mask_of(l);
         if (words > cw) return api_fail(SBGPU_ESHAPE, "sbgpu_context_table_host: compat_words does not cover a locus");
         mask_locus = l;
      }
      if (sb::ctx_hit_qualifies(compat + h * cw, kept.data(), words)) {
         ++n_in_bin[(size_t)b];
         last_hit[(size_t)b] = h;
      }
   }
   // the order pass and the gather, locus by locus
   int64_t row = 0;
   std::vector<int32_t> order;
   for (l = 0; l < nl; ++l) {
      const int64_t b0 = v.row_off[l], nb = v.row_off[l + 1] - b0, niso = v.iso_off[l + 1] - v.iso_off[l], f0 = v.f_off[l];
      if (out->locus_row_off) out->locus_row_off[l] = row;
      const int64_t row0 = row;
      uint32_t hits = 0; // (uint, as the reference's gene_frag_count)
      for (int64_t b = 0; b < nb; ++b) hits += n_in_bin[(size_t)(b0 + b)];
      if (out->locus_hits) out->locus_hits[l] = hits;
      if (hits) {
         order.resize((size_t)nb);
         std::iota(order.begin(), order.end(), 0);
         const uint32_t *K = key.data() + b0 * kw;
         std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return sb::ctx_key_less(K + (int64_t)x * kw, K + (int64_t)y * kw, kw); });
         for (int64_t r = 0; r < nb; ++r) {
            const int64_t b = b0 + order[(size_t)r];
            if (!n_in_bin[(size_t)b]) continue;
            if (out->row_bin) out->row_bin[row] = b;
            if (out->row_hits) out->row_hits[row] = n_in_bin[(size_t)b];
            if (out->row_prob)
               for (int64_t j = 0; j < niso; ++j)
                  out->row_prob[f0 + (row - row0) * niso + j] =
                     sb::ctx_row_value(compat + last_hit[(size_t)b] * cw, (int)j, F[f0 + (b - b0) * niso + j]);
            ++row;
         }
      }
      if (out->row_prob) // behind the locus' rows: zeros, as the device form leaves them
         for (int64_t i = f0 + (row - row0) * niso; i < v.f_off[l + 1]; ++i) out->row_prob[i] = 0.0;
   }
   if (out->locus_row_off) out->locus_row_off[nl] = row;
   out->n_rows = row;
   return SBGPU_OK;
}
