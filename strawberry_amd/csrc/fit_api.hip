// strawberry_amd/csrc/fit_api.hip -- sbgpu_em_fit_device, sbgpu_model_fit_device, sbgpu_em_fit_limits (include/sbgpu.h): how
// well theta explains every locus' bin counts, built from the arrays a batch has in HBM (fit_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "fit_device.h"

using sb::api_fail;

namespace {

void fit_clear_device(sbgpu_em_fit_t *out)
{
   out->d_expected = nullptr, out->d_resid = nullptr, out->d_score = nullptr;
   out->d_loglik = nullptr, out->d_deviance = nullptr, out->d_pearson = nullptr;
   out->d_n_live = nullptr, out->d_n_dropped = nullptr, out->d_n_impossible = nullptr;
   out->d_dof = nullptr, out->d_worst_bin = nullptr;
}

// the two entry points' common part: `ps` says the shapes, everything else is device memory
int fit_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &ps, const int32_t *d_count, const double *d_F, const double *d_theta,
            const int32_t *d_keep, const int32_t *d_status, void *stream, sbgpu_em_fit_t *out)
{
   const int64_t nl = ps.n_loci, n_bins = ps.n_rows, n_iso = ps.n_iso;
   // ---- the loci by form (fit_device.h): a wave each, or a workgroup each
   std::vector<int32_t> small, large;
   bool any_weight = false;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = ps.row_off[l + 1] - ps.row_off[l], niso = ps.iso_off[l + 1] - ps.iso_off[l];
      if (nb > sb::kFitMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > 32 * (int64_t)sb::kFitMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
      any_weight |= nb * niso > 0;
      (sb::fit_wave_form(nb, niso) ? small : large).push_back((int32_t)l);
   }
   if (n_bins && !d_count) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if (any_weight && !d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
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
   // ---- one arena: [uploads: the two lists | keep / status where the caller gave none | live, gains | the results]
   auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
   const size_t nl1 = (size_t)nl + 1, nb1 = (size_t)std::max<int64_t>(n_bins, 1), ni1 = (size_t)std::max<int64_t>(n_iso, 1);
   size_t off = 0;
   const size_t o_small = off; off += up((small.size() + 1) * 4);
   const size_t o_large = off; off += up((large.size() + 1) * 4);
   const size_t upload_bytes = off;
   const size_t o_keep = off; off += d_keep ? 0 : up(ni1 * 4);
   const size_t o_status = off; off += d_status ? 0 : up(nl1 * 4);
   const size_t o_live = off; off += up(nb1);
   const size_t o_gain = off; off += up(ni1 * 8);
   const size_t o_exp = off; off += up(nb1 * 8);
   const size_t o_res = off; off += up(nb1 * 8);
   const size_t o_score = off; off += up(ni1 * 8);
   const size_t o_ll = off; off += up(nl1 * 8);
   const size_t o_dev = off; off += up(nl1 * 8);
   const size_t o_pear = off; off += up(nl1 * 8);
   const size_t o_nlive = off; off += up(nl1 * 8);
   const size_t o_ndrop = off; off += up(nl1 * 8);
   const size_t o_nimp = off; off += up(nl1 * 8);
   const size_t o_dof = off; off += up(nl1 * 4);
   const size_t o_worst = off; off += up(nl1 * 4);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, 11, off, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   // (one host block for the uploads: it lives until the call's last synchronisation; SB_TRY synchronises before it leaves early)
   std::vector<char> host(upload_bytes, 0);
   if (!small.empty()) std::memcpy(host.data() + o_small, small.data(), small.size() * 4);
   if (!large.empty()) std::memcpy(host.data() + o_large, large.data(), large.size() * 4);
   SB_TRY(hipMemcpyAsync(d, host.data(), upload_bytes, hipMemcpyHostToDevice, s));
   // no filter given: every isoform is kept (any non-zero word); no status given: every locus started (SBGPU_EM_OK is 0)
   if (!d_keep) SB_TRY(hipMemsetAsync(d + o_keep, 1, ni1 * 4, s));
   if (!d_status) SB_TRY(hipMemsetAsync(d + o_status, 0, nl1 * 4, s));
   const int32_t *keep = d_keep ? d_keep : (const int32_t *)(d + o_keep), *status = d_status ? d_status : (const int32_t *)(d + o_status);
   sb::AsgColumnPass col;
   col.n_loci = nl;
   col.row_off = ps.d_row_off, col.iso_off = ps.d_iso_off, col.f_off = ps.d_f_off;
   col.keep = keep, col.status = status;
   col.F = d_F, col.theta = d_theta;
   col.live = (uint8_t *)(d + o_live), col.gain = (double *)(d + o_gain);
   sb::FitArgs a;
   a.row_off = col.row_off, a.iso_off = col.iso_off, a.f_off = col.f_off;
   a.count = d_count, a.F = d_F;
   a.keep = keep, a.status = status;
   a.live = col.live, a.gain = col.gain;
   a.expected = (double *)(d + o_exp), a.resid = (double *)(d + o_res), a.score = (double *)(d + o_score);
   a.loglik = (double *)(d + o_ll), a.deviance = (double *)(d + o_dev), a.pearson = (double *)(d + o_pear);
   a.n_live = (long long *)(d + o_nlive), a.n_dropped = (long long *)(d + o_ndrop), a.n_impossible = (long long *)(d + o_nimp);
   a.dof = (int32_t *)(d + o_dof), a.worst_bin = (int32_t *)(d + o_worst);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kFitGridPerCu;
   // (sbgpu_set_timing: the three launches as stages of their own, for tools/bench_fit.py)
   sb::ctx_stage_reset(c);
   sb::ctx_stage_begin(c, "fit_column", s);
   if (nl) SB_TRY(sb::asg_launch_column_pass(col, (unsigned)std::min<int64_t>(nl, cap), s));
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "fit_wave", s);
   if (!small.empty()) {
      a.n_list = (int64_t)small.size(), a.list = (const int32_t *)(d + o_small);
      const int64_t blocks = (a.n_list + sb::kFitWaveLoci - 1) / sb::kFitWaveLoci;
      hipLaunchKernelGGL(sb::fit_wave_kernel, dim3((unsigned)std::min<int64_t>(blocks, cap)), dim3(sb::kFitThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "fit_block", s);
   if (!large.empty()) {
      a.n_list = (int64_t)large.size(), a.list = (const int32_t *)(d + o_large);
      hipLaunchKernelGGL(sb::fit_block_kernel, dim3((unsigned)std::min<int64_t>(a.n_list, cap)), dim3(sb::kFitThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // ---- results: what the caller asked for
   if (out->expected && n_bins) SB_TRY(hipMemcpyAsync(out->expected, d + o_exp, (size_t)n_bins * 8, hipMemcpyDeviceToHost, s));
   if (out->resid && n_bins) SB_TRY(hipMemcpyAsync(out->resid, d + o_res, (size_t)n_bins * 8, hipMemcpyDeviceToHost, s));
   if (out->score && n_iso) SB_TRY(hipMemcpyAsync(out->score, d + o_score, (size_t)n_iso * 8, hipMemcpyDeviceToHost, s));
   if (out->loglik && nl) SB_TRY(hipMemcpyAsync(out->loglik, d + o_ll, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->deviance && nl) SB_TRY(hipMemcpyAsync(out->deviance, d + o_dev, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->pearson && nl) SB_TRY(hipMemcpyAsync(out->pearson, d + o_pear, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->n_live && nl) SB_TRY(hipMemcpyAsync(out->n_live, d + o_nlive, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->n_dropped && nl) SB_TRY(hipMemcpyAsync(out->n_dropped, d + o_ndrop, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->n_impossible && nl) SB_TRY(hipMemcpyAsync(out->n_impossible, d + o_nimp, (size_t)nl * 8, hipMemcpyDeviceToHost, s));
   if (out->dof && nl) SB_TRY(hipMemcpyAsync(out->dof, d + o_dof, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
   if (out->worst_bin && nl) SB_TRY(hipMemcpyAsync(out->worst_bin, d + o_worst, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
#undef SB_TRY
   out->d_expected = (const double *)(d + o_exp), out->d_resid = (const double *)(d + o_res), out->d_score = (const double *)(d + o_score);
   out->d_loglik = (const double *)(d + o_ll), out->d_deviance = (const double *)(d + o_dev), out->d_pearson = (const double *)(d + o_pear);
   out->d_n_live = (const int64_t *)(d + o_nlive), out->d_n_dropped = (const int64_t *)(d + o_ndrop), out->d_n_impossible = (const int64_t *)(d + o_nimp);
   out->d_dof = (const int32_t *)(d + o_dof), out->d_worst_bin = (const int32_t *)(d + o_worst);
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
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, "sbgpu_model_fit_device: null argument");
   fit_clear_device(out);
   if (!d_theta) return api_fail(SBGPU_EINVAL, "sbgpu_model_fit_device: d_theta is needed (the fit is theta's: give the call's, or another estimate)");
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   if (!v.boot_serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_model_fit_device: this handle was made without retention (sbgpu_bootstrap_keep was off for its call, or it is not "
                                    "from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.boot_serial != rec->serial || !rec->plan)
      return api_fail(SBGPU_EINVAL, "sbgpu_model_fit_device: a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that works in the "
                                    "context's scratch) has reused what its call kept");
   const sb::PlanShape ps = sb::plan_shape(rec->plan);
   if (ps.n_loci != v.n_loci || ps.n_iso != v.n_iso || ps.n_rows != v.n_bins || ps.n_loci != rec->n_loci || ps.n_iso != rec->n_iso)
      return api_fail(SBGPU_EINVAL, "sbgpu_model_fit_device: the handle and the context's record disagree");
   return fit_run("sbgpu_model_fit_device", c, ps, rec->d_count, rec->d_F, d_theta, d_keep, d_status, stream, out);
}
