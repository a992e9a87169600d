// strawberry_amd/csrc/vb_api.hip -- sbgpu_em_vb_device, sbgpu_model_vb_device, sbgpu_em_vb_limits (include/sbgpu.h): the
// variational Bayes solve of every locus of a batch, from the arrays the batch has in HBM (vb_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "stage_common.h"
#include "vb_device.h"

using sb::api_fail;

namespace {

void vb_clear_device(sbgpu_em_vb_t *out)
{
   out->d_count = nullptr, out->d_share = nullptr, out->d_share_sd = nullptr, out->d_status = nullptr, out->d_iters = nullptr;
   out->d_elbo = nullptr, out->d_n_active = nullptr, out->d_n_frag = nullptr;
}

// the two entry points' common part: `ps` says the shapes, everything else is device memory
int vb_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &ps, const int32_t *d_count, const double *d_F,
           const sbgpu_vb_params_t *params, void *stream, sbgpu_em_vb_t *out)
{
   sb::VbParams P;
   if (!sb::vb_params(params, &P)) return api_fail(SBGPU_EINVAL, who + ": alpha outside [1e-6, 1e3], change_limit <= 0 or max_iter < 1");
   const int64_t nl = ps.n_loci, n_bins = ps.n_rows, n_iso = ps.n_iso;
   // ---- the loci by form (vb_device.h): a wave each, or a workgroup each; whether one of those keeps A in the scratch
   std::vector<int32_t> small, large;
   bool any_weight = false, any_global = false;
   int64_t n_elem = 0;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = ps.row_off[l + 1] - ps.row_off[l], niso = ps.iso_off[l + 1] - ps.iso_off[l];
      if (nb > sb::kVbMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > sb::kVbMaxIso) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 512 isoforms");
      any_weight |= nb * niso > 0, n_elem += nb * niso;
      const bool wave = sb::vb_wave_form(nb, niso);
      any_global |= !wave && !sb::vb_staged(nb, niso);
      (wave ? small : large).push_back((int32_t)l);
   }
   if (n_bins && !d_count) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if (any_weight && !d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   const sb::VbLayout L = sb::vb_layout(nl, n_iso, any_global ? n_elem : 0, small.size(), large.size());
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchVb, L.bytes, &d); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock host(L.upload_bytes);
   host.put(L.small, small.data(), small.size()), host.put(L.large, large.data(), large.size());
   sb::ctx_stage_reset(c);
   SB_STAGE_TRY(host.upload(d, s));
   sb::VbArgs a;
   a.row_off = ps.d_row_off, a.iso_off = ps.d_iso_off, a.f_off = ps.d_f_off;
   a.count = d_count, a.F = d_F;
   a.norm = any_global ? sb::arena_at<double>(d, L.norm) : nullptr;
   a.alpha = P.alpha, a.change_limit = P.change_limit, a.max_iter = P.max_iter;
   a.out_count = sb::arena_at<double>(d, L.count), a.out_share = sb::arena_at<double>(d, L.share), a.out_sd = sb::arena_at<double>(d, L.sd);
   a.status = sb::arena_at<int32_t>(d, L.status), a.iters = sb::arena_at<int32_t>(d, L.iters), a.n_active = sb::arena_at<int32_t>(d, L.nact);
   a.elbo = sb::arena_at<double>(d, L.elbo), a.n_frag = sb::arena_at<long long>(d, L.nfrag);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kVbGridPerCu;
   // (sbgpu_set_timing: the two launches as stages of their own, for tools/bench_vb.py)
   sb::ctx_stage_begin(c, "vb_wave", s);
   if (!small.empty()) {
      a.n_list = (int64_t)small.size(), a.list = sb::arena_at<int32_t>(d, L.small);
      const int64_t blocks = (a.n_list + sb::kVbWaveLoci - 1) / sb::kVbWaveLoci;
      hipLaunchKernelGGL(sb::vb_wave_kernel, dim3(sb::stage_grid(blocks, cap)), dim3(sb::kVbThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   sb::ctx_stage_begin(c, "vb_block", s);
   if (!large.empty()) {
      a.n_list = (int64_t)large.size(), a.list = sb::arena_at<int32_t>(d, L.large);
      hipLaunchKernelGGL(sb::vb_block_kernel, dim3(sb::stage_grid(a.n_list, cap)), dim3(sb::kVbThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->count, d, L.count, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->share, d, L.share, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->share_sd, d, L.sd, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->status, d, L.status, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters, d, L.iters, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->elbo, d, L.elbo, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_active, d, L.nact, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_frag, d, L.nfrag, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_count = sb::arena_at<double>(d, L.count), out->d_share = sb::arena_at<double>(d, L.share), out->d_share_sd = sb::arena_at<double>(d, L.sd);
   out->d_status = sb::arena_at<int32_t>(d, L.status), out->d_iters = sb::arena_at<int32_t>(d, L.iters), out->d_elbo = sb::arena_at<double>(d, L.elbo);
   out->d_n_active = sb::arena_at<int32_t>(d, L.nact), out->d_n_frag = sb::arena_at<int64_t>(d, L.nfrag);
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_vb_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_vb_limits: null argument");
   const int64_t v[8] = {sb::kVbWaveVals, sb::kVbStage, sb::kVbWaveLoci, sb::kVbGridPerCu, sb::kVbThreads, sb::kVbWave, sb::kVbMaxBins, sb::kVbMaxIso};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_vb_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                                  const sbgpu_vb_params_t *params, void *stream, sbgpu_em_vb_t *out)
{
   if (!c || !plan || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_vb_device: null argument");
   vb_clear_device(out);
   return vb_run("sbgpu_em_vb_device", c, sb::plan_shape(plan), d_count, d_F, params, stream, out);
}

extern "C" int sbgpu_model_vb_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_vb_params_t *params, void *stream, sbgpu_em_vb_t *out)
{
   const std::string who = "sbgpu_model_vb_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   vb_clear_device(out);
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   sb::PlanShape ps;
   if (const int rc = sb::check_boot_keep(who, rec, sb::bins_context_view(bins), true, &ps); rc != SBGPU_OK) return rc;
   return vb_run(who, c, ps, rec->d_count, rec->d_F, params, stream, out);
}
