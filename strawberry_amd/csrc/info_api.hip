// strawberry_amd/csrc/info_api.hip -- sbgpu_em_info_device, sbgpu_model_info_device, sbgpu_em_info_limits (include/sbgpu.h):
// which isoforms of every locus the counted bins can tell apart, and the covariance of theta, built from the arrays a batch
// has in HBM (info_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "info_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

void info_clear_device(sbgpu_em_info_t *out)
{
   out->d_se = nullptr, out->d_partner_corr = nullptr, out->d_ident = nullptr, out->d_alias_of = nullptr, out->d_partner = nullptr;
   out->d_min_pivot = nullptr, out->d_rank = nullptr, out->d_n_free = nullptr, out->d_info_status = nullptr;
   out->d_cov = nullptr, out->d_cov_off = nullptr;
}

// the two entry points' common part: `ps` says the shapes, everything else is device memory
int info_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &ps, const int32_t *d_count, const double *d_F, const double *d_theta,
             const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_info_t *out)
{
   const int64_t nl = ps.n_loci, n_bins = ps.n_rows, n_iso = ps.n_iso;
   // ---- the loci by form (info_device.h): a wave each, or a workgroup each (which also answers for a locus beyond the shape
   // limits: SBGPU_INFO_TOO_WIDE); the packed covariance's offsets
   std::vector<int32_t> small, large;
   std::vector<int64_t> cov_off((size_t)nl + 1, 0);
   bool any_weight = false;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = ps.row_off[l + 1] - ps.row_off[l], niso = ps.iso_off[l + 1] - ps.iso_off[l];
      any_weight |= nb * niso > 0;
      (sb::info_wave_form(nb, niso) ? small : large).push_back((int32_t)l);
      cov_off[(size_t)l + 1] = cov_off[(size_t)l] + sb::info_cov_entries(niso);
   }
   const int64_t n_cov = cov_off[(size_t)nl];
   if (out->cov) {
      if (!out->cov_off) return api_fail(SBGPU_EINVAL, who + ": cov is given without cov_off (sbgpu_em_info_cov_offsets makes it)");
      if (!std::equal(cov_off.begin(), cov_off.end(), out->cov_off)) return api_fail(SBGPU_EINVAL, who + ": cov_off is not sbgpu_em_info_cov_offsets' for this batch");
   }
   if (n_bins && !d_count) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if (any_weight && !d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the arena (stage_host.h: info_layout): keep / status have room in it where the caller gave none
   const sb::InfoLayout L = sb::info_layout(nl, n_bins, n_iso, n_cov, small.size(), large.size(), !d_keep, !d_status);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchInfo, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock host(L.upload_bytes);
   host.put(L.small, small.data(), small.size()), host.put(L.large, large.data(), large.size()), host.put(L.covoff, cov_off.data(), cov_off.size());
   SB_STAGE_TRY(host.upload(d, s));
   // no filter given: every isoform is kept (any non-zero word); no status given: every locus started (SBGPU_EM_OK is 0)
   if (!d_keep) SB_STAGE_TRY(hipMemsetAsync(d + L.keep, 1, sb::at_least_1(n_iso) * 4, s));
   if (!d_status) SB_STAGE_TRY(hipMemsetAsync(d + L.status, 0, ((size_t)nl + 1) * 4, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.cov, 0, L.cov_bytes, s));
   const int32_t *keep = d_keep ? d_keep : sb::arena_at<int32_t>(d, L.keep), *status = d_status ? d_status : sb::arena_at<int32_t>(d, L.status);
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = ps.d_row_off, col.iso_off = ps.d_iso_off, col.f_off = ps.d_f_off;
   col.keep = keep, col.status = status;
   col.F = d_F, col.theta = d_theta;
   col.live = sb::arena_at<uint8_t>(d, L.live), col.gain = sb::arena_at<double>(d, L.gain);
   sb::InfoArgs a;
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.cov_off = sb::arena_at<int64_t>(d, L.covoff);
   a.count = d_count, a.F = d_F;
   a.keep = keep, a.status = status;
   a.live = col.live, a.gain = col.gain;
   a.w = sb::arena_at<double>(d, L.w);
   a.se = sb::arena_at<double>(d, L.se), a.partner_corr = sb::arena_at<double>(d, L.pcorr);
   a.ident = sb::arena_at<int32_t>(d, L.ident), a.alias_of = sb::arena_at<int32_t>(d, L.alias), a.partner = sb::arena_at<int32_t>(d, L.partner);
   a.min_pivot = sb::arena_at<double>(d, L.minpiv);
   a.rank = sb::arena_at<int32_t>(d, L.rank), a.n_free = sb::arena_at<int32_t>(d, L.nfree), a.info_status = sb::arena_at<int32_t>(d, L.istatus);
   a.cov = sb::arena_at<double>(d, L.cov);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kInfoGridPerCu;
   // (sbgpu_set_timing: the three launches as stages of their own, for tools/bench_info.py)
   sb::ctx_stage_reset(c);
   sb::ctx_stage_begin(c, "info_column", s);
   if (nl) SB_STAGE_TRY(sb::asg_launch_column_pass(col, sb::stage_grid(nl, cap), s));
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "info_wave", s);
   if (!small.empty()) {
      a.n_list = (int64_t)small.size(), a.list = sb::arena_at<int32_t>(d, L.small);
      const int64_t blocks = (a.n_list + sb::kInfoWaveLoci - 1) / sb::kInfoWaveLoci;
      hipLaunchKernelGGL(sb::info_wave_kernel, dim3(sb::stage_grid(blocks, cap)), dim3(sb::kInfoThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "info_block", s);
   if (!large.empty()) {
      a.n_list = (int64_t)large.size(), a.list = sb::arena_at<int32_t>(d, L.large);
      hipLaunchKernelGGL(sb::info_block_kernel, dim3(sb::stage_grid(a.n_list, cap)), dim3(sb::kInfoThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->se, d, L.se, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->partner_corr, d, L.pcorr, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->ident, d, L.ident, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->alias_of, d, L.alias, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->partner, d, L.partner, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->min_pivot, d, L.minpiv, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->rank, d, L.rank, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_free, d, L.nfree, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->info_status, d, L.istatus, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->cov, d, L.cov, n_cov, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_se = a.se, out->d_partner_corr = a.partner_corr, out->d_ident = a.ident, out->d_alias_of = a.alias_of, out->d_partner = a.partner;
   out->d_min_pivot = a.min_pivot, out->d_rank = a.rank, out->d_n_free = a.n_free, out->d_info_status = a.info_status;
   out->d_cov = a.cov, out->d_cov_off = a.cov_off;
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_info_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_limits: null argument");
   const int64_t v[8] = {sb::kInfoMaxFree, sb::kInfoWaveVals, sb::kInfoWaveIso, sb::kInfoStage, sb::kInfoWaveLoci, sb::kInfoGridPerCu,
                         sb::kInfoMaxBins, 32 * (int64_t)sb::kInfoMaxWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_info_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const double *d_theta,
                                    const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_info_t *out)
{
   if (!c || !plan || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_device: null argument");
   info_clear_device(out);
   if (!d_theta) return api_fail(SBGPU_EINVAL, "sbgpu_em_info_device: d_theta is needed (the information is theta's: give the EM's, or another estimate)");
   return info_run("sbgpu_em_info_device", c, sb::plan_shape(plan), d_count, d_F, d_theta, d_keep, d_status, stream, out);
}

extern "C" int sbgpu_model_info_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const double *d_theta, const int32_t *d_keep, const int32_t *d_status,
                                       void *stream, sbgpu_em_info_t *out)
{
   const std::string who = "sbgpu_model_info_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   info_clear_device(out);
   if (!d_theta) return api_fail(SBGPU_EINVAL, who + ": d_theta is needed (the information is theta's: give the call's, or another estimate)");
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   sb::PlanShape ps;
   if (const int rc = sb::check_boot_keep(who, rec, sb::bins_context_view(bins), true, &ps); rc != SBGPU_OK) return rc;
   return info_run(who, c, ps, rec->d_count, rec->d_F, d_theta, d_keep, d_status, stream, out);
}
