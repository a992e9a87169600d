// strawberry_amd/csrc/body_api.hip -- sbgpu_body_profile_device (include/sbgpu.h): every isoform's posterior-weighted bases by
// positional bin, its total, centre and coefficient of variation, and the sample's curve per length class, built where a
// resident call left its results (body_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "body_device.h"
#include "stage_common.h"

using sb::api_fail;

extern "C" int sbgpu_body_profile_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_body_profile_limits: null argument");
   const int64_t v[8] = {sb::kBodyItemHits, sb::kBodyLdsExons, sb::kBodyLdsIso, sb::kBodyLdsSums, sb::kBodyNarrowIso, sb::kBodyCopies,
                         sb::kBodyMaxBins, 32 * (int64_t)sb::kBodyMaxWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_body_profile_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                                         const double *d_theta, const float *d_hit_mass, const uint8_t *iso_strand, int32_t n_pos, void *stream,
                                         sbgpu_body_profile_t *out)
{
   const std::string who = "sbgpu_body_profile_device";
   if (!c || !bins || !annot || !d_hits || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (!d_theta) return api_fail(SBGPU_EINVAL, who + ": d_theta is needed (the posterior is theta's: give the call's, or another estimate)");
   if (n_pos < 1 || n_pos > SBGPU_BODY_MAX_POS) return api_fail(SBGPU_EINVAL, who + ": n_pos must be 1 .. 100");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   out->d_body_bases = nullptr, out->d_body_total = nullptr, out->d_body_center = nullptr, out->d_body_cv = nullptr;
   out->d_class_profile = nullptr, out->d_class_n = nullptr;
   if (const int rc = sb::check_context_keep(who, k, v, true); rc != SBGPU_OK) return rc;
   const int64_t nl = v.n_loci, n_iso = v.n_iso, nh = k->n_hits;
   const int P = n_pos;
   if (d_hits->n_hits != nh) return api_fail(SBGPU_EINVAL, who + ": d_hits->n_hits is not the retained call's hit count (give the hits that call was given)");
   if (nh && (!d_hits->feat_off || !d_hits->feat_code || !d_hits->feat_left || !d_hits->feat_right))
      return api_fail(SBGPU_EINVAL, who + ": the hits' features are needed");
   if (annot->n_loci != nl || !annot->iso_off || !annot->exon_off || annot->iso_off[nl] != n_iso || !std::equal(v.iso_off, v.iso_off + nl + 1, annot->iso_off))
      return api_fail(SBGPU_EINVAL, who + ": the annotation's loci or isoforms are not the handle's (give the annotation the call was given)");
   const int64_t n_exon = annot->exon_off[n_iso];
   if (n_exon && (!annot->exon_left || !annot->exon_right)) return api_fail(SBGPU_EINVAL, who + ": the annotation's exons are needed");
   if (const int rc = sb::check_locus_limits(who, v, ": a locus of more than 5632 bins", &k->locus_hit_off); rc != SBGPU_OK) return rc;
   for (int64_t i = 0; i < n_iso; ++i)
      if (annot->exon_off[i + 1] < annot->exon_off[i] || annot->exon_off[i + 1] - annot->exon_off[i] > INT32_MAX)
         return api_fail(SBGPU_EINVAL, who + ": the annotation's exon offsets do not ascend");
   for (int64_t e = 0; e < n_exon; ++e)
      if (annot->exon_right[e] < annot->exon_left[e]) return api_fail(SBGPU_EINVAL, who + ": an exon of the annotation ends before it begins");
   if (iso_strand)
      for (int64_t i = 0; i < n_iso; ++i)
         if (iso_strand[i] > 2) return api_fail(SBGPU_EINVAL, who + ": iso_strand holds a value above 2 (0: unknown, 1: +, 2: -)");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the hit pass' work items (a locus without bins too: its hits are nobody's, and the kernel passes them by)
   const std::vector<sb::HitItem> items = sb::build_hit_items(k->locus_hit_off.data(), nl, nullptr);
   const int64_t n_items = (int64_t)items.size();
   // the exon arrays: the context's pinned copy where this is the pinned annotation, else uploaded with the offsets
   const sb::ResidentAnnotation *res = sb::ctx_resident_annotation(c);
   if (res && !(res->matches(annot) && res->dev.exon_off && (!n_exon || (res->dev.exon_left && res->dev.exon_right)))) res = nullptr;
   // ---- the arena (stage_host.h: body_layout)
   const sb::BodyLayout L = sb::body_layout(nl, v.n_bins, n_iso, n_exon, n_items, P, !res);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchBody, L.bytes, &d); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   const size_t nl1 = (size_t)nl + 1;
   sb::HostBlock host(L.upload_bytes);
   host.put(L.roff, v.row_off, nl1), host.put(L.ioff, v.iso_off, nl1), host.put(L.foff, v.f_off, nl1);
   host.put(L.items, items.data(), items.size());
   if (!res) host.put(L.eoff, annot->exon_off, (size_t)n_iso + 1), host.put(L.eleft, annot->exon_left, (size_t)n_exon), host.put(L.eright, annot->exon_right, (size_t)n_exon);
   // every exon's prefix length and every isoform's length: once per call, here, not once per hit
   sb::body_lengths(annot->exon_off, annot->exon_left, annot->exon_right, n_iso, (int64_t *)(host.bytes.data() + L.epre), (int64_t *)(host.bytes.data() + L.ilen));
   if (iso_strand) host.put(L.strand, iso_strand, (size_t)n_iso);
   SB_STAGE_TRY(host.upload(d, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.bases, 0, L.sums_bytes, s));
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = sb::arena_at<int64_t>(d, L.roff), col.iso_off = sb::arena_at<int64_t>(d, L.ioff), col.f_off = sb::arena_at<int64_t>(d, L.foff);
   col.keep = k->d_keep, col.status = k->d_status;
   col.F = k->d_F, col.theta = d_theta;
   col.live = sb::arena_at<uint8_t>(d, L.live), col.gain = sb::arena_at<double>(d, L.gain);
   sb::BodyArgs a;
   a.n_loci = nl, a.n_items = n_items, a.n_iso = n_iso;
   a.compat_words = k->compat_words, a.n_pos = P;
   a.items = sb::arena_at<sb::HitItem>(d, L.items);
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.exon_off = res ? res->dev.exon_off : sb::arena_at<int64_t>(d, L.eoff);
   a.exon_left = res ? res->dev.exon_left : sb::arena_at<uint32_t>(d, L.eleft);
   a.exon_right = res ? res->dev.exon_right : sb::arena_at<uint32_t>(d, L.eright);
   a.exon_pre = sb::arena_at<int64_t>(d, L.epre), a.iso_len = sb::arena_at<int64_t>(d, L.ilen), a.iso_strand = sb::arena_at<uint8_t>(d, L.strand);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.F = k->d_F, a.hit_mass = d_hit_mass;
   a.feat_off = d_hits->feat_off, a.feat_code = d_hits->feat_code, a.feat_left = d_hits->feat_left, a.feat_right = d_hits->feat_right;
   a.live = col.live, a.gain = col.gain;
   a.body_bases = sb::arena_at<double>(d, L.bases), a.class_profile = sb::arena_at<double>(d, L.cprof);
   a.class_n = sb::arena_at<unsigned long long>(d, L.cn);
   a.body_total = sb::arena_at<double>(d, L.total), a.body_center = sb::arena_at<double>(d, L.center), a.body_cv = sb::arena_at<double>(d, L.cv);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   // (the three launches are stages of their own while sbgpu_set_timing is on: sbgpu_last_stage_ms)
   sb::ctx_stage_reset(c);
   sb::ctx_stage_begin(c, "body_column", s);
   SB_STAGE_TRY(sb::asg_launch_column_pass(col, sb::stage_grid(nl, cap), s));
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "body_hit", s);
   if (n_items) {
      hipLaunchKernelGGL(sb::body_hit_kernel, dim3(sb::stage_grid(n_items, cap)), dim3(sb::kBodyThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "body_iso", s);
   if (n_iso) {
      const int64_t blocks = (n_iso + sb::kBodyThreads - 1) / sb::kBodyThreads;
      hipLaunchKernelGGL(sb::body_iso_kernel, dim3(sb::stage_grid(blocks, cap)), dim3(sb::kBodyThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->body_bases, d, L.bases, n_iso * P, s));
   SB_STAGE_TRY(sb::copy_back(out->body_total, d, L.total, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->body_center, d, L.center, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->body_cv, d, L.cv, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->class_profile, d, L.cprof, 4 * (int64_t)P, s));
   SB_STAGE_TRY(sb::copy_back(out->class_n, d, L.cn, 4, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_body_bases = a.body_bases, out->d_body_total = a.body_total, out->d_body_center = a.body_center, out->d_body_cv = a.body_cv;
   out->d_class_profile = a.class_profile, out->d_class_n = sb::arena_at<int64_t>(d, L.cn);
   return SBGPU_OK;
}
