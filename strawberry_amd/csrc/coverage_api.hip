// strawberry_amd/csrc/coverage_api.hip -- sbgpu_isoform_coverage_device (include/sbgpu.h): per-exon bases, per-junction mass,
// per-isoform bases and the unexplained bases of every locus, built where a resident call left its results
// (coverage_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "coverage_device.h"
#include "stage_common.h"

using sb::api_fail;

extern "C" int sbgpu_isoform_coverage_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_limits: null argument");
   const int64_t v[8] = {sb::kCovItemHits, sb::kCovLdsExons, sb::kCovLdsIso, sb::kCovNarrowIso, sb::kCovCopyExons, sb::kCovCopies,
                         sb::kCovMaxBins, 32 * (int64_t)sb::kCovMaxWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_isoform_coverage_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_annotation_t *annot, const sbgpu_hits_t *d_hits,
                                             const double *d_theta, const float *d_hit_mass, void *stream, sbgpu_isoform_coverage_t *out)
{
   const std::string who = "sbgpu_isoform_coverage_device";
   if (!c || !bins || !annot || !d_hits || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (!d_theta) return api_fail(SBGPU_EINVAL, who + ": d_theta is needed (the posterior is theta's: give the call's, or another estimate)");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   out->d_exon_bases = nullptr, out->d_junction_mass = nullptr, out->d_iso_bases = nullptr, out->d_unexplained_bases = nullptr;
   if (const int rc = sb::check_context_keep(who, k, v, true); rc != SBGPU_OK) return rc;
   const int64_t nl = v.n_loci, n_iso = v.n_iso, nh = k->n_hits;
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
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the hit pass' work items (a locus without bins too: its hits are unexplained)
   const std::vector<sb::HitItem> items = sb::build_hit_items(k->locus_hit_off.data(), nl, nullptr);
   const int64_t n_items = (int64_t)items.size();
   // the exon arrays: the context's pinned copy where this is the pinned annotation, else uploaded with the offsets
   const sb::ResidentAnnotation *res = sb::ctx_resident_annotation(c);
   if (res && !(res->matches(annot) && res->dev.exon_off && (!n_exon || (res->dev.exon_left && res->dev.exon_right)))) res = nullptr;
   // ---- the arena (stage_host.h: cov_layout)
   const sb::CovLayout L = sb::cov_layout(nl, v.n_bins, n_iso, n_exon, n_items, !res);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchCoverage, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   const size_t nl1 = (size_t)nl + 1;
   sb::HostBlock host(L.upload_bytes);
   host.put(L.roff, v.row_off, nl1), host.put(L.ioff, v.iso_off, nl1), host.put(L.foff, v.f_off, nl1);
   host.put(L.items, items.data(), items.size());
   if (!res) host.put(L.eoff, annot->exon_off, (size_t)n_iso + 1), host.put(L.eleft, annot->exon_left, (size_t)n_exon), host.put(L.eright, annot->exon_right, (size_t)n_exon);
   SB_STAGE_TRY(host.upload(d, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.bases, 0, L.sums_bytes, s));
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = sb::arena_at<int64_t>(d, L.roff), col.iso_off = sb::arena_at<int64_t>(d, L.ioff), col.f_off = sb::arena_at<int64_t>(d, L.foff);
   col.keep = k->d_keep, col.status = k->d_status;
   col.F = k->d_F, col.theta = d_theta;
   col.live = sb::arena_at<uint8_t>(d, L.live), col.gain = sb::arena_at<double>(d, L.gain);
   sb::CovArgs a;
   a.n_loci = nl, a.n_items = n_items, a.n_iso = n_iso;
   a.compat_words = k->compat_words;
   a.items = sb::arena_at<sb::HitItem>(d, L.items);
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.exon_off = res ? res->dev.exon_off : sb::arena_at<int64_t>(d, L.eoff);
   a.exon_left = res ? res->dev.exon_left : sb::arena_at<uint32_t>(d, L.eleft);
   a.exon_right = res ? res->dev.exon_right : sb::arena_at<uint32_t>(d, L.eright);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.F = k->d_F, a.hit_mass = d_hit_mass;
   a.feat_off = d_hits->feat_off, a.feat_code = d_hits->feat_code, a.feat_left = d_hits->feat_left, a.feat_right = d_hits->feat_right;
   a.live = col.live, a.gain = col.gain;
   a.exon_bases = sb::arena_at<double>(d, L.bases), a.junction_mass = sb::arena_at<double>(d, L.junc);
   a.unexplained_bases = sb::arena_at<double>(d, L.unex), a.iso_bases = sb::arena_at<double>(d, L.iso);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   SB_STAGE_TRY(sb::asg_launch_column_pass(col, sb::stage_grid(nl, cap), s));
   if (n_items) {
      hipLaunchKernelGGL(sb::cov_hit_kernel, dim3(sb::stage_grid(n_items, cap)), dim3(sb::kCovThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   if (n_iso) {
      const int64_t blocks = (n_iso + sb::kCovThreads - 1) / sb::kCovThreads;
      hipLaunchKernelGGL(sb::cov_iso_kernel, dim3(sb::stage_grid(blocks, cap)), dim3(sb::kCovThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->exon_bases, d, L.bases, n_exon, s));
   SB_STAGE_TRY(sb::copy_back(out->junction_mass, d, L.junc, n_exon, s));
   SB_STAGE_TRY(sb::copy_back(out->iso_bases, d, L.iso, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->unexplained_bases, d, L.unex, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_exon_bases = a.exon_bases, out->d_junction_mass = a.junction_mass;
   out->d_iso_bases = a.iso_bases, out->d_unexplained_bases = a.unexplained_bases;
   return SBGPU_OK;
}
