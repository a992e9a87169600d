// strawberry_amd/csrc/body_host.cpp -- sbgpu_body_profile_host (include/sbgpu.h): the posterior-weighted bases of every isoform by
// 5' -> 3' positional bin, the isoforms' totals, centres and coefficients of variation, and the sample's curve per length class,
// on the host.  The one CPU statement of what csrc/body_device.h computes: who is assigned and with what posterior is
// assign_rules.h's, the weight coverage_rules.h's, what a (hit, candidate) pair adds and what is made of an isoform's bins
// body_rules.h's, and the kernels call all three.  Hits in index order, candidates in ascending j, isoforms in ascending order.
// No kernels here, and -- in body_profile_arrays, the rule on plain arrays -- no HIP: a plain C++ compiler takes this file with
// SB_BODY_ARRAYS_ONLY defined (which leaves out the C entry, the one part that reads a handle).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "body_rules.h"
#include "stage_host.h"

namespace sb {
int api_fail(int code, const std::string &msg);

int body_profile_arrays(const BodyHostIn &in, sbgpu_body_profile_t *out)
{
   const std::string who = "sbgpu_body_profile_host";
   const int64_t nl = in.n_loci, nh = in.n_hits, n_iso = in.iso_off[nl];
   const int cw = in.compat_words, P = in.n_pos;
   const int64_t n_exon = in.exon_off[n_iso];
   for (int64_t i = 0; i < n_iso; ++i)
      if (in.exon_off[i + 1] < in.exon_off[i]) return api_fail(SBGPU_EINVAL, who + ": the annotation's exon offsets do not ascend");
   for (int64_t e = 0; e < n_exon; ++e)
      if (in.exon_right[e] < in.exon_left[e]) return api_fail(SBGPU_EINVAL, who + ": an exon of the annotation ends before it begins");
   std::vector<int64_t> exon_pre((size_t)n_exon + 1), iso_len((size_t)n_iso + 1);
   body_lengths(in.exon_off, in.exon_left, in.exon_right, n_iso, exon_pre.data(), iso_len.data());
   // ---- the assignment's column pass: kept words, live bins, gains
   ColumnPass col;
   if (!column_pass(nl, in.row_off, in.iso_off, in.f_off, in.F, in.theta, in.keep, in.status, cw, &col))
      return api_fail(SBGPU_ESHAPE, who + ": compat_words does not cover a locus");
   // ---- the hit pass, in hit order (the bins are needed for every other result, whether or not the caller asked for them)
   std::vector<double> own;
   double *bases = out->body_bases;
   if (!bases) own.assign((size_t)n_iso * (size_t)P + 1, 0.0), bases = own.data();
   else std::fill(bases, bases + n_iso * P, 0.0);
   int64_t l = 0;
   for (int64_t h = 0; h < nh; ++h) {
      const int64_t b = in.hit_bin[h];
      if (b >= in.n_bins) return api_fail(SBGPU_EINVAL, who + ": hit -> bin out of range");
      // (a hit without a bin says nothing of its locus: the hits' grouping does)
      if ((l = locus_of_hit(h, b, l, nl, in.row_off, in.locus_hit_off)) < 0)
         return api_fail(SBGPU_EINVAL, who + ": a hit without a bin, on a handle whose hits did not come grouped by locus: its locus is not known");
      const int64_t i0 = in.iso_off[l];
      const int niso = (int)(in.iso_off[l + 1] - i0);
      const int words = (niso + 31) / 32;
      const uint32_t *C = in.compat + h * cw, *K = col.kept.data() + col.word_off[(size_t)l];
      const double *G = col.gain.data() + i0;
      const double *row = b >= 0 && col.live[(size_t)b] ? in.F + in.f_off[l] + (b - in.row_off[l]) * niso : nullptr;
      const AsgHit r = asg_hit_map(C, K, words, G, row);
      if (r.map_iso < 0) continue;
      const double m = in.hit_mass ? (double)in.hit_mass[h] : 1.0;
      const int64_t q0 = in.feat_off[h];
      const int nf = (int)(in.feat_off[h + 1] - q0);
      for (int w = 0; w < words; ++w)
         for (uint32_t bits = C[w] & K[w]; bits; bits &= bits - 1) {
            const int j = 32 * w + __builtin_ctz(bits);
            const int64_t i = i0 + j, e0 = in.exon_off[i];
            const int strand = in.iso_strand ? in.iso_strand[i] : 0;
            double *mine = bases + i * P;
            body_walk(in.feat_code + q0, in.feat_left + q0, in.feat_right + q0, nf, in.exon_left + e0, in.exon_right + e0, exon_pre.data() + e0,
                      (int)(in.exon_off[i + 1] - e0), iso_len[(size_t)i], P, cov_weight(m, asg_posterior(G[j], row[j], r.den)),
                      [&](int q, double x) { mine[body_report(q, P, strand)] += x; });
         }
   }
   // ---- the isoforms in ascending order, and the classes
   if (out->class_profile) std::fill(out->class_profile, out->class_profile + 4 * P, 0.0);
   if (out->class_n) std::fill(out->class_n, out->class_n + 4, (int64_t)0);
   for (int64_t i = 0; i < n_iso; ++i) {
      const double *mine = bases + i * P;
      const BodyIso o = body_iso(mine, P, iso_len[(size_t)i], in.iso_strand ? in.iso_strand[i] : 0);
      if (out->body_total) out->body_total[i] = o.total;
      if (out->body_center) out->body_center[i] = o.center;
      if (out->body_cv) out->body_cv[i] = o.cv;
      if (!(o.total > 0.0)) continue;
      const int c = body_class(iso_len[(size_t)i]);
      if (out->class_profile)
         for (int p = 0; p < P; ++p) out->class_profile[c * P + p] += mine[p] / o.total;
      if (out->class_n) out->class_n[c] += 1;
   }
   return SBGPU_OK;
}
} // namespace sb

#ifndef SB_BODY_ARRAYS_ONLY
#include "api_internal.h"

using sb::api_fail;

extern "C" int sbgpu_body_profile_host(const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *hits, const uint32_t *compat,
                                       int32_t compat_words, const double *F, const double *theta, const int32_t *keep, const int32_t *status,
                                       const float *hit_mass, const uint8_t *iso_strand, int32_t n_pos, sbgpu_body_profile_t *out)
{
   const std::string who = "sbgpu_body_profile_host";
   if (!bins || !annot || !hits || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (!theta) return api_fail(SBGPU_EINVAL, who + ": theta is needed (the posterior is theta's: give the EM's, or another estimate)");
   if (n_pos < 1 || n_pos > SBGPU_BODY_MAX_POS) return api_fail(SBGPU_EINVAL, who + ": n_pos must be 1 .. 100");
   const sb::BinsContextView v = sb::bins_context_view(bins);
   const int64_t nl = v.n_loci, nh = v.n_hits;
   out->d_body_bases = nullptr, out->d_body_total = nullptr, out->d_body_center = nullptr, out->d_body_cv = nullptr;
   out->d_class_profile = nullptr, out->d_class_n = nullptr;
   if (annot->n_loci != nl || !annot->iso_off || !annot->exon_off || annot->iso_off[nl] != v.n_iso || !std::equal(v.iso_off, v.iso_off + nl + 1, annot->iso_off))
      return api_fail(SBGPU_EINVAL, who + ": the annotation's loci or isoforms are not the handle's (give the annotation the handle was made from)");
   if (nh == 0) return api_fail(SBGPU_EINVAL, who + ": this handle holds no hit -> bin (use one from sbgpu_bins_create or sbgpu_quantify_host)");
   if (hits->n_hits != nh) return api_fail(SBGPU_EINVAL, who + ": hits->n_hits is not the handle's hit count (give the hits the handle was made from)");
   if (!hits->feat_off || (hits->feat_off[nh] && (!hits->feat_code || !hits->feat_left || !hits->feat_right)))
      return api_fail(SBGPU_EINVAL, who + ": the hits' features are needed");
   if (!compat || compat_words < 1) return api_fail(SBGPU_EINVAL, who + ": the hits' compat words are needed");
   if (!F) F = v.F;
   if (!F && v.n_elem) return api_fail(SBGPU_EINVAL, who + ": this handle holds no weights (give F, or a handle from sbgpu_quantify_host)");
   if (annot->exon_off[v.n_iso] && (!annot->exon_left || !annot->exon_right)) return api_fail(SBGPU_EINVAL, who + ": the annotation's exons are needed");
   if (iso_strand)
      for (int64_t i = 0; i < v.n_iso; ++i)
         if (iso_strand[i] > 2) return api_fail(SBGPU_EINVAL, who + ": iso_strand holds a value above 2 (0: unknown, 1: +, 2: -)");
   std::vector<int64_t> hit_bin((size_t)nh, -1);
   if (const int rc = sbgpu_bins_export(bins, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hit_bin.data(), nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
       rc != SBGPU_OK)
      return rc;
   sb::BodyHostIn in;
   in.n_loci = nl, in.n_hits = nh, in.n_bins = v.n_bins;
   in.row_off = v.row_off, in.iso_off = v.iso_off, in.f_off = v.f_off, in.locus_hit_off = v.locus_hit_off;
   in.hit_bin = hit_bin.data();
   in.exon_off = annot->exon_off, in.exon_left = annot->exon_left, in.exon_right = annot->exon_right;
   in.feat_off = hits->feat_off, in.feat_code = hits->feat_code, in.feat_left = hits->feat_left, in.feat_right = hits->feat_right;
   in.compat = compat, in.compat_words = compat_words;
   in.F = F, in.theta = theta, in.keep = keep, in.status = status, in.hit_mass = hit_mass, in.iso_strand = iso_strand, in.n_pos = n_pos;
   return sb::body_profile_arrays(in, out);
}
#endif
