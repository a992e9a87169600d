// strawberry_amd/csrc/assign_api.hip -- sbgpu_fragment_assign_device (include/sbgpu.h): every hit's isoform posterior, built
// where a resident call left its results (assign_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "assign_device.h"

using sb::api_fail;

namespace sb {
hipError_t asg_launch_column_pass(const AsgColumnPass &p, unsigned grid, hipStream_t s)
{
   AsgArgs a{};
   a.n_loci = p.n_loci;
   a.row_off = p.row_off, a.iso_off = p.iso_off, a.f_off = p.f_off;
   a.keep = p.keep, a.status = p.status;
   a.F = p.F, a.theta = p.theta;
   a.live = p.live, a.gain = p.gain;
   hipLaunchKernelGGL(asg_column_kernel, dim3(grid), dim3(kAsgThreads), 0, s, a);
   return hipGetLastError();
}
} // namespace sb

extern "C" int sbgpu_fragment_assign_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const double *d_theta, const float *d_hit_mass,
                                            void *stream, sbgpu_fragment_assign_t *out)
{
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: null argument");
   if (!d_theta) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: d_theta is needed (the posterior is theta's: give the call's, or another estimate)");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   if (!v.context_serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: this handle was made without retention (sbgpu_context_table_keep was off for its call, "
                                    "or it is not from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.context_serial != k->serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that "
                                    "works in the context's scratch, such as sbgpu_bins_create_device) has reused what its call kept");
   const int64_t nl = v.n_loci, n_bins = v.n_bins, n_iso = v.n_iso, nh = k->n_hits;
   const int32_t cw = k->compat_words;
   if (nl != k->n_loci || n_iso != k->n_iso || (int64_t)k->locus_hit_off.size() != nl + 1 || k->locus_hit_off[0] != 0 || k->locus_hit_off[(size_t)nl] != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: the handle and the context's record disagree");
   if (nh && (!k->d_hit_bin_local || !k->d_compat || cw < 1)) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: the hits' bins are not on the device");
   if (v.n_elem && !k->d_F) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: the weights are not on the device");
   if ((out->map_iso || out->map_prob || out->n_cand) && out->n_hits != nh)
      return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: out->n_hits must say how many hits the per-hit arrays hold: the retained call's count");
   out->n_hits = 0;
   out->d_map_iso = nullptr, out->d_map_prob = nullptr, out->d_n_cand = nullptr;
   out->d_unique_mass = nullptr, out->d_map_mass = nullptr, out->d_post_mass = nullptr, out->d_unassigned = nullptr;
   for (int64_t l = 0; l < nl; ++l) {
      if (v.row_off[l + 1] - v.row_off[l] > sb::kAsgMaxBins) return api_fail(SBGPU_ESHAPE, "sbgpu_fragment_assign_device: a locus of more than 5632 bins");
      if (v.iso_off[l + 1] - v.iso_off[l] > 32 * (int64_t)sb::kAsgMaxWords) return api_fail(SBGPU_ESHAPE, "sbgpu_fragment_assign_device: a locus of more than 4096 isoforms");
      if (k->locus_hit_off[(size_t)l + 1] < k->locus_hit_off[(size_t)l]) return api_fail(SBGPU_EINVAL, "sbgpu_fragment_assign_device: the handle and the context's record disagree");
   }
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
   // ---- the hit pass' work items: a locus' hits in ranges of kAsgItemHits (a locus without bins too: its hits are counted)
   std::vector<sb::AsgItem> items;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t q0 = k->locus_hit_off[(size_t)l], q1 = k->locus_hit_off[(size_t)l + 1];
      const int32_t split = q1 - q0 > sb::kAsgItemHits;
      for (int64_t h = q0; h < q1; h += sb::kAsgItemHits) items.push_back({h, std::min<int64_t>(h + sb::kAsgItemHits, q1), (int32_t)l, split});
   }
   const int64_t n_items = (int64_t)items.size();
   // ---- one arena: [uploads: the four offset arrays, the items | live, gains | the sums (zeroed) | the per-hit results]
   auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
   const size_t nl1 = (size_t)nl + 1, nb1 = (size_t)std::max<int64_t>(n_bins, 1), ni1 = (size_t)std::max<int64_t>(n_iso, 1), nh1 = (size_t)std::max<int64_t>(nh, 1);
   size_t off = 0;
   const size_t o_hoff = off; off += up(nl1 * 8);
   const size_t o_roff = off; off += up(nl1 * 8);
   const size_t o_ioff = off; off += up(nl1 * 8);
   const size_t o_foff = off; off += up(nl1 * 8);
   const size_t o_items = off; off += up((size_t)std::max<int64_t>(n_items, 1) * sizeof(sb::AsgItem));
   const size_t upload_bytes = off;
   const size_t o_live = off; off += up(nb1);
   const size_t o_gain = off; off += up(ni1 * 8);
   const size_t o_sums = off;
   const size_t o_uniq = off; off += up(ni1 * 8);
   const size_t o_map = off; off += up(ni1 * 8);
   const size_t o_post = off; off += up(ni1 * 8);
   const size_t o_unas = off; off += up(nl1 * 8);
   const size_t sums_bytes = off - o_sums;
   const size_t o_iso = off; off += up(nh1 * 4);
   const size_t o_cand = off; off += up(nh1 * 4);
   const size_t o_prob = off; off += up(nh1 * 8);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, 9, off, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   // (one host block for the uploads: it lives until the call's last synchronisation; SB_TRY synchronises before it leaves early)
   std::vector<char> host(upload_bytes, 0);
   std::memcpy(host.data() + o_hoff, k->locus_hit_off.data(), nl1 * 8);
   std::memcpy(host.data() + o_roff, v.row_off, nl1 * 8);
   std::memcpy(host.data() + o_ioff, v.iso_off, nl1 * 8);
   std::memcpy(host.data() + o_foff, v.f_off, nl1 * 8);
   if (n_items) std::memcpy(host.data() + o_items, items.data(), (size_t)n_items * sizeof(sb::AsgItem));
   SB_TRY(hipMemcpyAsync(d, host.data(), upload_bytes, hipMemcpyHostToDevice, s));
   SB_TRY(hipMemsetAsync(d + o_sums, 0, sums_bytes, s));
   sb::AsgArgs a;
   a.n_loci = nl, a.n_items = n_items;
   a.compat_words = cw;
   a.items = (const sb::AsgItem *)(d + o_items);
   a.locus_hit_off = (const int64_t *)(d + o_hoff), a.row_off = (const int64_t *)(d + o_roff);
   a.iso_off = (const int64_t *)(d + o_ioff), a.f_off = (const int64_t *)(d + o_foff);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.F = k->d_F, a.theta = d_theta, a.hit_mass = d_hit_mass;
   a.live = (uint8_t *)(d + o_live), a.gain = (double *)(d + o_gain);
   a.map_iso = (int32_t *)(d + o_iso), a.n_cand = (int32_t *)(d + o_cand), a.map_prob = (double *)(d + o_prob);
   a.unique_mass = (double *)(d + o_uniq), a.map_mass = (double *)(d + o_map), a.post_mass = (double *)(d + o_post);
   a.unassigned = (unsigned long long *)(d + o_unas);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   const unsigned lgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nl, cap));
   hipLaunchKernelGGL(sb::asg_column_kernel, dim3(lgrid), dim3(sb::kAsgThreads), 0, s, a);
   SB_TRY(hipGetLastError());
   if (n_items) {
      hipLaunchKernelGGL(sb::asg_hit_kernel, dim3((unsigned)std::min<int64_t>(n_items, cap)), dim3(sb::kAsgThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   // ---- results: what the caller asked for
   if (out->map_iso && nh) SB_TRY(hipMemcpyAsync(out->map_iso, d + o_iso, (size_t)nh * 4, hipMemcpyDeviceToHost, s));
   if (out->n_cand && nh) SB_TRY(hipMemcpyAsync(out->n_cand, d + o_cand, (size_t)nh * 4, hipMemcpyDeviceToHost, s));
   if (out->map_prob && nh) SB_TRY(hipMemcpyAsync(out->map_prob, d + o_prob, (size_t)nh * 8, hipMemcpyDeviceToHost, s));
   if (out->unique_mass && n_iso) SB_TRY(hipMemcpyAsync(out->unique_mass, d + o_uniq, (size_t)n_iso * 8, hipMemcpyDeviceToHost, s));
   if (out->map_mass && n_iso) SB_TRY(hipMemcpyAsync(out->map_mass, d + o_map, (size_t)n_iso * 8, hipMemcpyDeviceToHost, s));
   if (out->post_mass && n_iso) SB_TRY(hipMemcpyAsync(out->post_mass, d + o_post, (size_t)n_iso * 8, hipMemcpyDeviceToHost, s));
   if (out->unassigned && nl) SB_TRY(hipMemcpyAsync(out->unassigned, d + o_unas, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
#undef SB_TRY
   out->n_hits = nh;
   out->d_map_iso = (const int32_t *)(d + o_iso), out->d_map_prob = (const double *)(d + o_prob), out->d_n_cand = (const int32_t *)(d + o_cand);
   out->d_unique_mass = (const double *)(d + o_uniq), out->d_map_mass = (const double *)(d + o_map), out->d_post_mass = (const double *)(d + o_post);
   out->d_unassigned = (const int64_t *)(d + o_unas);
   return SBGPU_OK;
}
