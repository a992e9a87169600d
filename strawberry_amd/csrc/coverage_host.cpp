// strawberry_amd/csrc/coverage_host.cpp -- sbgpu_isoform_coverage_host (include/sbgpu.h): per-exon bases, per-junction mass,
// per-isoform bases and the bases no kept isoform explains, on the host.  The one CPU statement of what csrc/coverage_device.h
// computes: who is assigned and with what posterior is assign_rules.h's, what a (hit, candidate) pair adds is coverage_rules.h's,
// and the kernels call both.  Hits in index order, candidates in ascending j, exons in ascending order.  No kernels here.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "coverage_rules.h"
#include "stage_host.h"

using sb::api_fail;

extern "C" int sbgpu_isoform_coverage_host(const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits,
                                           const uint32_t *compat, int32_t compat_words, const double *F, const double *theta,
                                           const int32_t *keep, const int32_t *status, const float *hit_mass, sbgpu_isoform_coverage_t *out)
{
   if (!bins || !annot || !hits || !out) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: null argument");
   if (!theta) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: theta is needed (the posterior is theta's: give the EM's, or another estimate)");
   const sb::BinsContextView v = sb::bins_context_view(bins);
   const int64_t nl = v.n_loci, nh = v.n_hits;
   const int cw = compat_words;
   out->d_exon_bases = nullptr, out->d_junction_mass = nullptr, out->d_iso_bases = nullptr, out->d_unexplained_bases = nullptr;
   if (annot->n_loci != nl || !annot->iso_off || !annot->exon_off || annot->iso_off[nl] != v.n_iso)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: the annotation's loci or isoforms are not the handle's (give the annotation the handle was made from)");
   for (int64_t l = 0; l <= nl; ++l)
      if (annot->iso_off[l] != v.iso_off[l])
         return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: the annotation's loci or isoforms are not the handle's (give the annotation the handle was made from)");
   if (nh == 0) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: this handle holds no hit -> bin (use one from sbgpu_bins_create or sbgpu_quantify_host)");
   if (hits->n_hits != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: hits->n_hits is not the handle's hit count (give the hits the handle was made from)");
   if (!hits->feat_off || (hits->feat_off[nh] && (!hits->feat_code || !hits->feat_left || !hits->feat_right)))
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: the hits' features are needed");
   if (!compat || cw < 1) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: the hits' compat words are needed");
   if (!F) F = v.F;
   if (!F && v.n_elem)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: this handle holds no weights (give F, or a handle from sbgpu_quantify_host)");
   const int64_t n_exon = annot->exon_off[v.n_iso];
   if (n_exon && (!annot->exon_left || !annot->exon_right)) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: the annotation's exons are needed");
   std::vector<int64_t> hit_bin((size_t)nh, -1);
   if (const int rc = sbgpu_bins_export(bins, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hit_bin.data(), nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
       rc != SBGPU_OK)
      return rc;
   // ---- the assignment's column pass: kept words, live bins, gains
   sb::ColumnPass col;
   if (!sb::column_pass(nl, v.row_off, v.iso_off, v.f_off, F, theta, keep, status, cw, &col))
      return api_fail(SBGPU_ESHAPE, "sbgpu_isoform_coverage_host: compat_words does not cover a locus");
   // ---- the hit pass, in hit order (the exon sums are needed for iso_bases whether or not the caller asked for them)
   std::vector<double> own_exon;
   double *exon_bases = out->exon_bases;
   if (!exon_bases && out->iso_bases) own_exon.assign((size_t)n_exon + 1, 0.0), exon_bases = own_exon.data();
   if (out->exon_bases) std::fill(out->exon_bases, out->exon_bases + n_exon, 0.0);
   if (out->junction_mass) std::fill(out->junction_mass, out->junction_mass + n_exon, 0.0);
   if (out->unexplained_bases) std::fill(out->unexplained_bases, out->unexplained_bases + nl, 0.0);
   double *junction_mass = out->junction_mass;
   int64_t l = 0;
   for (int64_t h = 0; h < nh; ++h) {
      const int64_t b = hit_bin[(size_t)h];
      if (b >= v.n_bins) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: hit -> bin out of range");
      // (a hit without a bin says nothing of its locus: the hits' grouping does)
      if ((l = sb::locus_of_hit(h, b, l, nl, v.row_off, v.locus_hit_off)) < 0)
         return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_host: a hit without a bin, on a handle whose hits did not come grouped by locus: "
                                       "its locus is not known");
      const int64_t i0 = v.iso_off[l];
      const int niso = (int)(v.iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const uint32_t *C = compat + h * cw, *K = col.kept.data() + col.word_off[(size_t)l];
      const double *G = col.gain.data() + i0;
      const double *row = b >= 0 && col.live[(size_t)b] ? F + v.f_off[l] + (b - v.row_off[l]) * niso : nullptr;
      const sb::AsgHit r = sb::asg_hit_map(C, K, words, G, row);
      const double m = hit_mass ? (double)hit_mass[h] : 1.0;
      const int64_t q0 = hits->feat_off[h];
      const int nf = (int)(hits->feat_off[h + 1] - q0);
      const uint8_t *code = hits->feat_code + q0;
      const uint32_t *fl = hits->feat_left + q0, *fr = hits->feat_right + q0;
      if (r.map_iso < 0) {
         if (out->unexplained_bases) out->unexplained_bases[l] += m * (double)sb::cov_matchlen(code, fl, fr, nf);
         continue;
      }
      if (!exon_bases && !junction_mass) continue;
      for (int w = 0; w < words; ++w)
         for (uint32_t bits = C[w] & K[w]; bits; bits &= bits - 1) {
            const int j = 32 * w + __builtin_ctz(bits);
            const int64_t e0 = annot->exon_off[i0 + j];
            const int ne = (int)(annot->exon_off[i0 + j + 1] - e0);
            sb::cov_walk(
               code, fl, fr, nf, annot->exon_left + e0, annot->exon_right + e0, ne, sb::cov_weight(m, sb::asg_posterior(G[j], row[j], r.den)),
               [&](int e, double x) {
                  if (exon_bases) exon_bases[e0 + e] += x;
               },
               [&](int e, double x) {
                  if (junction_mass) junction_mass[e0 + e] += x;
               });
         }
   }
   if (out->iso_bases)
      for (int64_t i = 0; i < v.n_iso; ++i) out->iso_bases[i] = sb::cov_iso_bases(exon_bases, annot->exon_off[i], annot->exon_off[i + 1]);
   return SBGPU_OK;
}
