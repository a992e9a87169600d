// strawberry_amd/csrc/assign_api.hip -- sbgpu_fragment_assign_device (include/sbgpu.h): every hit's isoform posterior, built
// where a resident call left its results (assign_device.h).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "assign_device.h"
#include "stage_common.h"

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
   const std::string who = "sbgpu_fragment_assign_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (!d_theta) return api_fail(SBGPU_EINVAL, who + ": d_theta is needed (the posterior is theta's: give the call's, or another estimate)");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   if (const int rc = sb::check_context_keep(who, k, v, true); rc != SBGPU_OK) return rc;
   const int64_t nl = v.n_loci, n_iso = v.n_iso, nh = k->n_hits;
   if ((out->map_iso || out->map_prob || out->n_cand) && out->n_hits != nh)
      return api_fail(SBGPU_EINVAL, who + ": out->n_hits must say how many hits the per-hit arrays hold: the retained call's count");
   out->n_hits = 0;
   out->d_map_iso = nullptr, out->d_map_prob = nullptr, out->d_n_cand = nullptr;
   out->d_unique_mass = nullptr, out->d_map_mass = nullptr, out->d_post_mass = nullptr, out->d_unassigned = nullptr;
   if (const int rc = sb::check_locus_limits(who, v, ": a locus of more than 5632 bins", &k->locus_hit_off); rc != SBGPU_OK) return rc;
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the hit pass' work items (a locus without bins too: its hits are counted), and the arena (stage_host.h: asg_layout)
   const std::vector<sb::HitItem> items = sb::build_hit_items(k->locus_hit_off.data(), nl, nullptr);
   const int64_t n_items = (int64_t)items.size();
   const sb::AsgLayout L = sb::asg_layout(nl, v.n_bins, n_iso, nh, n_items);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchAssign, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   const size_t nl1 = (size_t)nl + 1;
   sb::HostBlock host(L.upload_bytes);
   host.put(L.hoff, k->locus_hit_off.data(), nl1), host.put(L.roff, v.row_off, nl1), host.put(L.ioff, v.iso_off, nl1), host.put(L.foff, v.f_off, nl1);
   host.put(L.items, items.data(), items.size());
   SB_STAGE_TRY(host.upload(d, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.uniq, 0, L.sums_bytes, s));
   sb::AsgArgs a;
   a.n_loci = nl, a.n_items = n_items;
   a.compat_words = k->compat_words;
   a.items = sb::arena_at<sb::HitItem>(d, L.items);
   a.locus_hit_off = sb::arena_at<int64_t>(d, L.hoff), a.row_off = sb::arena_at<int64_t>(d, L.roff);
   a.iso_off = sb::arena_at<int64_t>(d, L.ioff), a.f_off = sb::arena_at<int64_t>(d, L.foff);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.F = k->d_F, a.theta = d_theta, a.hit_mass = d_hit_mass;
   a.live = sb::arena_at<uint8_t>(d, L.live), a.gain = sb::arena_at<double>(d, L.gain);
   a.map_iso = sb::arena_at<int32_t>(d, L.iso), a.n_cand = sb::arena_at<int32_t>(d, L.cand), a.map_prob = sb::arena_at<double>(d, L.prob);
   a.unique_mass = sb::arena_at<double>(d, L.uniq), a.map_mass = sb::arena_at<double>(d, L.map), a.post_mass = sb::arena_at<double>(d, L.post);
   a.unassigned = sb::arena_at<unsigned long long>(d, L.unas);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   hipLaunchKernelGGL(sb::asg_column_kernel, dim3(sb::stage_grid(nl, cap)), dim3(sb::kAsgThreads), 0, s, a);
   SB_STAGE_TRY(hipGetLastError());
   if (n_items) {
      hipLaunchKernelGGL(sb::asg_hit_kernel, dim3(sb::stage_grid(n_items, cap)), dim3(sb::kAsgThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->map_iso, d, L.iso, nh, s));
   SB_STAGE_TRY(sb::copy_back(out->n_cand, d, L.cand, nh, s));
   SB_STAGE_TRY(sb::copy_back(out->map_prob, d, L.prob, nh, s));
   SB_STAGE_TRY(sb::copy_back(out->unique_mass, d, L.uniq, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->map_mass, d, L.map, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->post_mass, d, L.post, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->unassigned, d, L.unas, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->n_hits = nh;
   out->d_map_iso = a.map_iso, out->d_map_prob = a.map_prob, out->d_n_cand = a.n_cand;
   out->d_unique_mass = a.unique_mass, out->d_map_mass = a.map_mass, out->d_post_mass = a.post_mass;
   out->d_unassigned = sb::arena_at<int64_t>(d, L.unas);
   return SBGPU_OK;
}
