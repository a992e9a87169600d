// strawberry_amd/csrc/assign_host.cpp -- sbgpu_fragment_assign_host (include/sbgpu.h): every hit's isoform posterior, on the
// host.  The one CPU statement of what csrc/assign_device.h computes: every decision is a function of assign_rules.h,
// which the kernels call too.  All sums run in hit order.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "stage_host.h"

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
   // ---- the column pass: kept words, live bins, gains
   sb::ColumnPass col;
   if (!sb::column_pass(nl, v.row_off, v.iso_off, v.f_off, F, theta, keep, status, cw, &col))
      return api_fail(SBGPU_ESHAPE, "sbgpu_fragment_assign_host: compat_words does not cover a locus");
   if (out->unique_mass) std::fill(out->unique_mass, out->unique_mass + v.n_iso, 0.0);
   if (out->map_mass) std::fill(out->map_mass, out->map_mass + v.n_iso, 0.0);
   if (out->post_mass) std::fill(out->post_mass, out->post_mass + v.n_iso, 0.0);
   if (out->unassigned) std::fill(out->unassigned, out->unassigned + nl, (int64_t)0);
   // ---- the hit pass, in hit order
   int64_t l = 0;
   for (int64_t h = 0; h < nh; ++h) {
      const int64_t b = hit_bin[(size_t)h];
      if (b >= v.n_bins) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: hit -> bin out of range");
      // (a hit without a bin says nothing of its locus: the hits' grouping does)
      if ((l = sb::locus_of_hit(h, b, l, nl, v.row_off, v.locus_hit_off)) < 0)
         return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_host: a hit without a bin, on a handle whose hits did not come grouped by locus: "
                                       "its locus is not known");
      const int64_t i0 = v.iso_off[l];
      const int niso = (int)(v.iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const uint32_t *C = compat + h * cw, *K = col.kept.data() + col.word_off[(size_t)l];
      const double *G = col.gain.data() + i0;
      const double *row = b >= 0 && col.live[(size_t)b] ? F + v.f_off[l] + (b - v.row_off[l]) * niso : nullptr;
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
