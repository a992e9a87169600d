// strawberry_amd/csrc/assign_host.cpp -- sbgpu_fragment_assign_host (include/sbgpu.h): every hit's isoform posterior, on the
// host.  The one CPU statement of what csrc/assign_device.h computes: every decision is a function of assign_rules.h,
// which the kernels call too.  All sums run in hit order.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "assign_rules.h"

using sb::api_fail;

extern "C" int sbgpu_fragment_assign_host(const sbgpu_bins_t *bins, const uint32_t *compat, int32_t compat_words, const double *F,
                                          const double *theta, const int32_t *keep, const int32_t *status, const float *hit_mass,
                                          sbgpu_fragment_assign_t *out)
{
   if (!bins || !out) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: null argument");
   if (!theta) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: theta is needed (the posterior is theta's: give the EM's, or another estimate)");
   const sb::BinsContextView v = sb::bins_context_view(bins);
   const int64_t nl = v.n_loci, nh = v.n_hits;
   const int cw = compat_words;
   if (nh && (!compat || cw < 1)) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: the hits' compat words are needed");
   if (!F) F = v.F;
   if (!F && v.n_elem)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: this handle holds no weights (give F, or a handle from sbgpu_quantify_host)");
   if ((out->map_iso || out->map_prob || out->n_cand) && out->n_hits != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: out->n_hits must say how many hits the per-hit arrays hold: the handle's count");
   out->n_hits = 0;
   out->d_map_iso = nullptr, out->d_map_prob = nullptr, out->d_n_cand = nullptr;
   out->d_unique_mass = nullptr, out->d_map_mass = nullptr, out->d_post_mass = nullptr, out->d_unassigned = nullptr;
   std::vector<int64_t> hit_bin((size_t)std::max<int64_t>(nh, 1), -1);
   if (const int rc = sbgpu_bins_export(bins, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hit_bin.data(), nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
       rc != SBGPU_OK)
      return rc;
   if (nh == 0) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: this handle holds no hit -> bin (use one from sbgpu_bins_create or sbgpu_quantify_host)");
   // ---- the column pass, locus by locus: kept words, live bins, gains
   std::vector<int64_t> word_off((size_t)nl + 1, 0);
   for (int64_t l = 0; l < nl; ++l) word_off[(size_t)l + 1] = word_off[(size_t)l] + (v.iso_off[l + 1] - v.iso_off[l] + 31) / 32;
   std::vector<uint32_t> kept((size_t)word_off[(size_t)nl] + 1, 0u);
   std::vector<uint8_t> live((size_t)v.n_bins + 1, 0);
   std::vector<double> g((size_t)v.n_iso + 1, 0.0);
   std::vector<int32_t> all_kept;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t i0 = v.iso_off[l], b0 = v.row_off[l], nb = v.row_off[l + 1] - b0, f0 = v.f_off[l];
      const int niso = (int)(v.iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      if (words > cw && nh) return api_fail(SBGPU_ESHAPE, "sbgpu_fragment_assign_host: compat_words does not cover a locus");
      if (!keep && (int)all_kept.size() < niso) all_kept.assign((size_t)niso, 1); // (no filter given: every isoform is kept)
      uint32_t *K = kept.data() + word_off[(size_t)l];
      for (int w = 0; w < words; ++w) K[w] = sb::ctx_kept_word(keep ? keep + i0 : all_kept.data(), niso, status ? status[l] : SBGPU_EM_OK, w);
      for (int64_t b = 0; b < nb; ++b) live[(size_t)(b0 + b)] = sb::asg_row_live(F + f0 + b * niso, niso);
      for (int j = 0; j < niso; ++j) {
         double c = 0.0;
         for (int64_t b = 0; b < nb; ++b)
            if (live[(size_t)(b0 + b)]) c += F[f0 + b * niso + j];
         g[(size_t)(i0 + j)] = sb::asg_gain(theta[i0 + j], c, (K[j >> 5] >> (j & 31)) & 1u);
      }
   }
   if (out->unique_mass) std::fill(out->unique_mass, out->unique_mass + v.n_iso, 0.0);
   if (out->map_mass) std::fill(out->map_mass, out->map_mass + v.n_iso, 0.0);
   if (out->post_mass) std::fill(out->post_mass, out->post_mass + v.n_iso, 0.0);
   if (out->unassigned) std::fill(out->unassigned, out->unassigned + nl, (int64_t)0);
   // ---- the hit pass, in hit order
   int64_t l = 0;
   for (int64_t h = 0; h < nh; ++h) {
      const int64_t b = hit_bin[(size_t)h];
      if (b >= v.n_bins) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: hit -> bin out of range");
      if (b >= 0) {
         if (b < v.row_off[l] || b >= v.row_off[l + 1]) l = std::upper_bound(v.row_off, v.row_off + nl + 1, b) - v.row_off - 1;
      } else {
         // a hit without a bin says nothing of its locus: the hits' grouping does
         if (!v.locus_hit_off)
            return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: a hit without a bin, on a handle whose hits did not come grouped by locus: "
                                          "its locus is not known");
         if (h < v.locus_hit_off[l] || h >= v.locus_hit_off[l + 1]) l = std::upper_bound(v.locus_hit_off, v.locus_hit_off + nl + 1, h) - v.locus_hit_off - 1;
      }
      const int64_t i0 = v.iso_off[l];
      const int niso = (int)(v.iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const uint32_t *C = compat + h * cw, *K = kept.data() + word_off[(size_t)l];
      const double *G = g.data() + i0;
      const double *row = b >= 0 && live[(size_t)b] ? F + v.f_off[l] + (b - v.row_off[l]) * niso : nullptr;
      const sb::AsgHit r = sb::asg_hit_map(C, K, words, G, row);
      if (out->n_cand) out->n_cand[h] = r.n_cand;
      if (out->map_iso) out->map_iso[h] = r.map_iso;
      if (out->map_prob) out->map_prob[h] = r.map_prob;
      if (r.map_iso < 0) {
         if (out->unassigned) ++out->unassigned[l];
         continue;
      }
      const double m = hit_mass ? (double)hit_mass[h] : 1.0;
      if (out->map_mass) out->map_mass[i0 + r.map_iso] += m;
      if (out->unique_mass && r.n_cand == 1) out->unique_mass[i0 + r.map_iso] += m;
      if (out->post_mass)
         for (int w = 0; w < words; ++w)
            for (uint32_t bits = C[w] & K[w]; bits; bits &= bits - 1) {
               const int j = 32 * w + __builtin_ctz(bits);
               out->post_mass[i0 + j] += m * sb::asg_posterior(G[j], row[j], r.den);
            }
   }
   out->n_hits = nh;
   return SBGPU_OK;
}
