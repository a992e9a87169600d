// strawberry_amd/csrc/coverage_api.hip -- sbgpu_isoform_coverage_device (include/sbgpu.h): per-exon bases, per-junction mass,
// per-isoform bases and the unexplained bases of every locus, built where a resident call left its results
// (coverage_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "coverage_device.h"

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
   if (!c || !bins || !annot || !d_hits || !out) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: null argument");
   if (!d_theta) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: d_theta is needed (the posterior is theta's: give the call's, or another estimate)");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   out->d_exon_bases = nullptr, out->d_junction_mass = nullptr, out->d_iso_bases = nullptr, out->d_unexplained_bases = nullptr;
   if (!v.context_serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: this handle was made without retention (sbgpu_context_table_keep was off for its call, "
                                    "or it is not from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.context_serial != k->serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that "
                                    "works in the context's scratch, such as sbgpu_bins_create_device) has reused what its call kept");
   const int64_t nl = v.n_loci, n_bins = v.n_bins, n_iso = v.n_iso, nh = k->n_hits;
   const int32_t cw = k->compat_words;
   if (nl != k->n_loci || n_iso != k->n_iso || (int64_t)k->locus_hit_off.size() != nl + 1 || k->locus_hit_off[0] != 0 || k->locus_hit_off[(size_t)nl] != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the handle and the context's record disagree");
   if (nh && (!k->d_hit_bin_local || !k->d_compat || cw < 1)) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the hits' bins are not on the device");
   if (v.n_elem && !k->d_F) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the weights are not on the device");
   if (d_hits->n_hits != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: d_hits->n_hits is not the retained call's hit count (give the hits that call was given)");
   if (nh && (!d_hits->feat_off || !d_hits->feat_code || !d_hits->feat_left || !d_hits->feat_right))
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the hits' features are needed");
   if (annot->n_loci != nl || !annot->iso_off || !annot->exon_off || annot->iso_off[nl] != n_iso || !std::equal(v.iso_off, v.iso_off + nl + 1, annot->iso_off))
      return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the annotation's loci or isoforms are not the handle's (give the annotation the call was given)");
   const int64_t n_exon = annot->exon_off[n_iso];
   if (n_exon && (!annot->exon_left || !annot->exon_right)) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the annotation's exons are needed");
   for (int64_t l = 0; l < nl; ++l) {
      if (v.row_off[l + 1] - v.row_off[l] > sb::kCovMaxBins) return api_fail(SBGPU_ESHAPE, "sbgpu_isoform_coverage_device: a locus of more than 5632 bins");
      if (v.iso_off[l + 1] - v.iso_off[l] > 32 * (int64_t)sb::kCovMaxWords) return api_fail(SBGPU_ESHAPE, "sbgpu_isoform_coverage_device: a locus of more than 4096 isoforms");
      if (k->locus_hit_off[(size_t)l + 1] < k->locus_hit_off[(size_t)l]) return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the handle and the context's record disagree");
   }
   for (int64_t i = 0; i < n_iso; ++i)
      if (annot->exon_off[i + 1] < annot->exon_off[i] || annot->exon_off[i + 1] - annot->exon_off[i] > INT32_MAX)
         return api_fail(SBGPU_EINVAL, "sbgpu_isoform_coverage_device: the annotation's exon offsets do not ascend");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
#define SB_TRY(expr)                                                                                        \
   do {                                                                                                     \
      hipError_t e_ = (expr);                                                                               \
      if (e_ != hipSuccess) {                                                                               \
         (void)hipStreamSynchronize(s); /* (the upload from `host` below may still be in flight) */         \
         return api_fail(SBGPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                    \
      }                                                                                                     \
   } while (0)
   SB_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the hit pass' work items: a locus' hits in ranges of kCovItemHits (a locus without bins too: its hits are unexplained)
   std::vector<sb::CovItem> items;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t q0 = k->locus_hit_off[(size_t)l], q1 = k->locus_hit_off[(size_t)l + 1];
      const int32_t split = q1 - q0 > sb::kCovItemHits;
      for (int64_t h = q0; h < q1; h += sb::kCovItemHits) items.push_back({h, std::min<int64_t>(h + sb::kCovItemHits, q1), (int32_t)l, split});
   }
   const int64_t n_items = (int64_t)items.size();
   // the exon arrays: the context's pinned copy where this is the pinned annotation, else uploaded with the offsets
   const sb::ResidentAnnotation *res = sb::ctx_resident_annotation(c);
   if (res && !(res->matches(annot) && res->dev.exon_off && (!n_exon || (res->dev.exon_left && res->dev.exon_right)))) res = nullptr;
   // ---- one arena: [uploads: the three offset arrays, the items (, the exon arrays) | live, gains | the sums (zeroed) | iso_bases]
   auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
   const size_t nl1 = (size_t)nl + 1, nb1 = (size_t)std::max<int64_t>(n_bins, 1), ni1 = (size_t)n_iso + 1, ne1 = (size_t)std::max<int64_t>(n_exon, 1);
   size_t off = 0;
   const size_t o_roff = off; off += up(nl1 * 8);
   const size_t o_ioff = off; off += up(nl1 * 8);
   const size_t o_foff = off; off += up(nl1 * 8);
   const size_t o_items = off; off += up((size_t)std::max<int64_t>(n_items, 1) * sizeof(sb::CovItem));
   const size_t o_eoff = off; off += res ? 0 : up(ni1 * 8);
   const size_t o_eleft = off; off += res ? 0 : up(ne1 * 4);
   const size_t o_eright = off; off += res ? 0 : up(ne1 * 4);
   const size_t upload_bytes = off;
   const size_t o_live = off; off += up(nb1);
   const size_t o_gain = off; off += up(ni1 * 8);
   const size_t o_sums = off;
   const size_t o_bases = off; off += up(ne1 * 8);
   const size_t o_junc = off; off += up(ne1 * 8);
   const size_t o_unex = off; off += up(nl1 * 8);
   const size_t sums_bytes = off - o_sums;
   const size_t o_iso = off; off += up(ni1 * 8);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, 10, off, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   // (one host block for the uploads: it lives until the call's last synchronisation; SB_TRY synchronises before it leaves early)
   std::vector<char> host(upload_bytes, 0);
   std::memcpy(host.data() + o_roff, v.row_off, nl1 * 8);
   std::memcpy(host.data() + o_ioff, v.iso_off, nl1 * 8);
   std::memcpy(host.data() + o_foff, v.f_off, nl1 * 8);
   if (n_items) std::memcpy(host.data() + o_items, items.data(), (size_t)n_items * sizeof(sb::CovItem));
   if (!res) {
      std::memcpy(host.data() + o_eoff, annot->exon_off, ni1 * 8);
      if (n_exon) std::memcpy(host.data() + o_eleft, annot->exon_left, (size_t)n_exon * 4), std::memcpy(host.data() + o_eright, annot->exon_right, (size_t)n_exon * 4);
   }
   SB_TRY(hipMemcpyAsync(d, host.data(), upload_bytes, hipMemcpyHostToDevice, s));
   SB_TRY(hipMemsetAsync(d + o_sums, 0, sums_bytes, s));
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = (const int64_t *)(d + o_roff), col.iso_off = (const int64_t *)(d + o_ioff), col.f_off = (const int64_t *)(d + o_foff);
   col.keep = k->d_keep, col.status = k->d_status;
   col.F = k->d_F, col.theta = d_theta;
   col.live = (uint8_t *)(d + o_live), col.gain = (double *)(d + o_gain);
   sb::CovArgs a;
   a.n_loci = nl, a.n_items = n_items, a.n_iso = n_iso;
   a.compat_words = cw;
   a.items = (const sb::CovItem *)(d + o_items);
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.exon_off = res ? res->dev.exon_off : (const int64_t *)(d + o_eoff);
   a.exon_left = res ? res->dev.exon_left : (const uint32_t *)(d + o_eleft);
   a.exon_right = res ? res->dev.exon_right : (const uint32_t *)(d + o_eright);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.F = k->d_F, a.hit_mass = d_hit_mass;
   a.feat_off = d_hits->feat_off, a.feat_code = d_hits->feat_code, a.feat_left = d_hits->feat_left, a.feat_right = d_hits->feat_right;
   a.live = col.live, a.gain = col.gain;
   a.exon_bases = (double *)(d + o_bases), a.junction_mass = (double *)(d + o_junc);
   a.unexplained_bases = (double *)(d + o_unex), a.iso_bases = (double *)(d + o_iso);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   SB_TRY(sb::asg_launch_column_pass(col, (unsigned)std::max<int64_t>(1, std::min<int64_t>(nl, cap)), s));
   if (n_items) {
      hipLaunchKernelGGL(sb::cov_hit_kernel, dim3((unsigned)std::min<int64_t>(n_items, cap)), dim3(sb::kCovThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   if (n_iso) {
      const int64_t blocks = (n_iso + sb::kCovThreads - 1) / sb::kCovThreads;
      hipLaunchKernelGGL(sb::cov_iso_kernel, dim3((unsigned)std::min<int64_t>(blocks, cap)), dim3(sb::kCovThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   // ---- results: what the caller asked for
   if (out->exon_bases && n_exon) SB_TRY(hipMemcpyAsync(out->exon_bases, d + o_bases, (size_t)n_exon * 8, hipMemcpyDeviceToHost, s));
   if (out->junction_mass && n_exon) SB_TRY(hipMemcpyAsync(out->junction_mass, d + o_junc, (size_t)n_exon * 8, hipMemcpyDeviceToHost, s));
   if (out->iso_bases && n_iso) SB_TRY(hipMemcpyAsync(out->iso_bases, d + o_iso, (size_t)n_iso * 8, hipMemcpyDeviceToHost, s));
   if (out->unexplained_bases && nl) SB_TRY(hipMemcpyAsync(out->unexplained_bases, d + o_unex, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
#undef SB_TRY
   out->d_exon_bases = (const double *)(d + o_bases), out->d_junction_mass = (const double *)(d + o_junc);
   out->d_iso_bases = (const double *)(d + o_iso), out->d_unexplained_bases = (const double *)(d + o_unex);
   return SBGPU_OK;
}
