// strawberry_amd/csrc/fit_api.hip -- sbgpu_em_fit_device, sbgpu_model_fit_device, sbgpu_em_fit_limits (include/sbgpu.h): how
// well theta explains every locus' bin counts, built from the arrays a batch has in HBM (fit_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "fit_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

void fit_clear_device(sbgpu_em_fit_t *out)
{
   out->d_expected = nullptr, out->d_resid = nullptr, out->d_score = nullptr;
   out->d_loglik = nullptr, out->d_deviance = nullptr, out->d_pearson = nullptr;
   out->d_n_live = nullptr, out->d_n_dropped = nullptr, out->d_n_impossible = nullptr;
   out->d_dof = nullptr, out->d_worst_bin = nullptr;
}

} // namespace

namespace sb {
// The loci by form (fit_device.h): a wave each, or a workgroup each; and the arena that follows from the two lists
int fit_plan(const std::string &who, const PlanShape &ps, bool own_keep, bool own_status, FitPlan *out)
{
   out->small.clear(), out->large.clear(), out->any_weight = false;
   for (int64_t l = 0; l < ps.n_loci; ++l) {
      const int64_t nb = ps.row_off[l + 1] - ps.row_off[l], niso = ps.iso_off[l + 1] - ps.iso_off[l];
      if (nb > kFitMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > 32 * (int64_t)kFitMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
      out->any_weight |= nb * niso > 0;
      (fit_wave_form(nb, niso) ? out->small : out->large).push_back((int32_t)l);
   }
   out->L = fit_layout(ps.n_loci, ps.n_rows, ps.n_iso, out->small.size(), out->large.size(), own_keep, own_status);
   return SBGPU_OK;
}

// The fit's launches on `s`, in arena `d` (p.L.bytes; any memory of the caller's): the lists' upload through `host`
// (p.L.upload_bytes, the caller's: it lives until the caller has synchronised), the column pass, the two forms.
int fit_launch(sbgpu_ctx_t *c, const PlanShape &ps, const FitPlan &p, HostBlock &host, char *d, const int32_t *d_count, const double *d_F,
               const double *d_theta, const int32_t *d_keep, const int32_t *d_status, hipStream_t s)
{
   const int64_t nl = ps.n_loci, n_iso = ps.n_iso;
   const FitLayout &L = p.L;
   const std::vector<int32_t> &small = p.small, &large = p.large;
   host.put(L.small, small.data(), small.size()), host.put(L.large, large.data(), large.size());
   SB_STAGE_TRY(host.upload(d, s));
   // no filter given: every isoform is kept (any non-zero word); no status given: every locus started (SBGPU_EM_OK is 0)
   if (!d_keep) SB_STAGE_TRY(hipMemsetAsync(d + L.keep, 1, sb::at_least_1(n_iso) * 4, s));
   if (!d_status) SB_STAGE_TRY(hipMemsetAsync(d + L.status, 0, ((size_t)nl + 1) * 4, s));
   const int32_t *keep = d_keep ? d_keep : sb::arena_at<int32_t>(d, L.keep), *status = d_status ? d_status : sb::arena_at<int32_t>(d, L.status);
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = ps.d_row_off, col.iso_off = ps.d_iso_off, col.f_off = ps.d_f_off;
   col.keep = keep, col.status = status;
   col.F = d_F, col.theta = d_theta;
   col.live = sb::arena_at<uint8_t>(d, L.live), col.gain = sb::arena_at<double>(d, L.gain);
   sb::FitArgs a;
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.count = d_count, a.F = d_F;
   a.keep = keep, a.status = status;
   a.live = col.live, a.gain = col.gain;
   a.expected = sb::arena_at<double>(d, L.exp), a.resid = sb::arena_at<double>(d, L.res), a.score = sb::arena_at<double>(d, L.score);
   a.loglik = sb::arena_at<double>(d, L.ll), a.deviance = sb::arena_at<double>(d, L.dev), a.pearson = sb::arena_at<double>(d, L.pear);
   a.n_live = sb::arena_at<long long>(d, L.nlive), a.n_dropped = sb::arena_at<long long>(d, L.ndrop), a.n_impossible = sb::arena_at<long long>(d, L.nimp);
   a.dof = sb::arena_at<int32_t>(d, L.dof), a.worst_bin = sb::arena_at<int32_t>(d, L.worst);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kFitGridPerCu;
   // (sbgpu_set_timing: the three launches as stages of their own, for tools/bench_fit.py)
   sb::ctx_stage_begin(c, "fit_column", s);
   if (nl) SB_STAGE_TRY(sb::asg_launch_column_pass(col, sb::stage_grid(nl, cap), s));
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "fit_wave", s);
   if (!small.empty()) {
      a.n_list = (int64_t)small.size(), a.list = sb::arena_at<int32_t>(d, L.small);
      const int64_t blocks = (a.n_list + sb::kFitWaveLoci - 1) / sb::kFitWaveLoci;
      hipLaunchKernelGGL(sb::fit_wave_kernel, dim3(sb::stage_grid(blocks, cap)), dim3(sb::kFitThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "fit_block", s);
   if (!large.empty()) {
      a.n_list = (int64_t)large.size(), a.list = sb::arena_at<int32_t>(d, L.large);
      hipLaunchKernelGGL(sb::fit_block_kernel, dim3(sb::stage_grid(a.n_list, cap)), dim3(sb::kFitThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   return SBGPU_OK;
}
} // namespace sb

namespace {

// the two entry points' common part: `ps` says the shapes, everything else is device memory
int fit_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &ps, const int32_t *d_count, const double *d_F, const double *d_theta,
            const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_fit_t *out)
{
   const int64_t nl = ps.n_loci, n_bins = ps.n_rows, n_iso = ps.n_iso;
   sb::FitPlan p;
   if (const int rc = sb::fit_plan(who, ps, !d_keep, !d_status, &p); rc != SBGPU_OK) return rc;
   if (n_bins && !d_count) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if (p.any_weight && !d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the arena (stage_host.h: fit_layout): keep / status have room in it where the caller gave none
   const sb::FitLayout &L = p.L;
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchFit, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock host(L.upload_bytes);
   sb::ctx_stage_reset(c);
   if (const int rc = sb::fit_launch(c, ps, p, host, d, d_count, d_F, d_theta, d_keep, d_status, s); rc != SBGPU_OK) return rc;
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->expected, d, L.exp, n_bins, s));
   SB_STAGE_TRY(sb::copy_back(out->resid, d, L.res, n_bins, s));
   SB_STAGE_TRY(sb::copy_back(out->score, d, L.score, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik, d, L.ll, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->deviance, d, L.dev, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->pearson, d, L.pear, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_live, d, L.nlive, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_dropped, d, L.ndrop, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_impossible, d, L.nimp, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->dof, d, L.dof, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->worst_bin, d, L.worst, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_expected = sb::arena_at<double>(d, L.exp), out->d_resid = sb::arena_at<double>(d, L.res), out->d_score = sb::arena_at<double>(d, L.score);
   out->d_loglik = sb::arena_at<double>(d, L.ll), out->d_deviance = sb::arena_at<double>(d, L.dev), out->d_pearson = sb::arena_at<double>(d, L.pear);
   out->d_n_live = sb::arena_at<int64_t>(d, L.nlive), out->d_n_dropped = sb::arena_at<int64_t>(d, L.ndrop), out->d_n_impossible = sb::arena_at<int64_t>(d, L.nimp);
   out->d_dof = sb::arena_at<int32_t>(d, L.dof), out->d_worst_bin = sb::arena_at<int32_t>(d, L.worst);
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_fit_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_limits: null argument");
   const int64_t v[8] = {sb::kFitWaveVals, sb::kFitStage, sb::kFitWaveLoci, sb::kFitGridPerCu, sb::kFitThreads, sb::kFitWave,
                         sb::kFitMaxBins, 32 * (int64_t)sb::kFitMaxWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_fit_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const double *d_theta,
                                   const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_fit_t *out)
{
   if (!c || !plan || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_device: null argument");
   fit_clear_device(out);
   if (!d_theta) return api_fail(SBGPU_EINVAL, "sbgpu_em_fit_device: d_theta is needed (the fit is theta's: give the EM's, or another estimate)");
   return fit_run("sbgpu_em_fit_device", c, sb::plan_shape(plan), d_count, d_F, d_theta, d_keep, d_status, stream, out);
}

extern "C" int sbgpu_model_fit_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const double *d_theta, const int32_t *d_keep, const int32_t *d_status,
                                      void *stream, sbgpu_em_fit_t *out)
{
   const std::string who = "sbgpu_model_fit_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   fit_clear_device(out);
   if (!d_theta) return api_fail(SBGPU_EINVAL, who + ": d_theta is needed (the fit is theta's: give the call's, or another estimate)");
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   sb::PlanShape ps;
   if (const int rc = sb::check_boot_keep(who, rec, sb::bins_context_view(bins), true, &ps); rc != SBGPU_OK) return rc;
   return fit_run(who, c, ps, rec->d_count, rec->d_F, d_theta, d_keep, d_status, stream, out);
}
