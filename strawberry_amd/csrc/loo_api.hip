// strawberry_amd/csrc/loo_api.hip -- sbgpu_em_loo_device, sbgpu_model_loo_device, sbgpu_em_loo_limits (include/sbgpu.h): the
// drop-one isoform support, built from the arrays a batch has in HBM (loo_device.h).  The shapes are made on the
// host (loo_rules.h: loo_shapes); then, a chunk of whole loci at a time: a plan for the chunk's sub-batch, the expansion, the EM
// through the library's own entry, the fit's launches (fit_api.hip: fit_launch) in this stage's scratch, the statistics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "loo_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

void loo_clear_device(sbgpu_em_loo_t *out)
{
   out->d_lr_stat = nullptr, out->d_heir_gain = nullptr, out->d_theta_refit = nullptr, out->d_n_unique = nullptr;
   out->d_heir = nullptr, out->d_status_without = nullptr, out->d_iters_without = nullptr, out->d_support = nullptr;
   out->d_loglik_base = nullptr, out->d_loo_status = nullptr, out->d_status_base = nullptr, out->d_iters_base = nullptr;
   out->d_theta_without = nullptr, out->d_without_off = nullptr;
}

// One chunk: loci [l0, l1), sub-problems [s0, s1) of the call, its sub-batch's offsets (beginning at 0) and its working set
struct LooChunk {
   int64_t l0 = 0, l1 = 0, s0 = 0, s1 = 0;
   std::vector<int64_t> row_off, iso_off, f_off;
   std::vector<sb::LooTile> tiles;
   sb::FitPlan fit;
   sb::LooChunkLayout L;
};

// the sub-batch's plan lives for one chunk
struct PlanGuard {
   sbgpu_plan_t *p = nullptr;
   ~PlanGuard() { sbgpu_plan_destroy(p); }
};

// the two entry points' common part: `ps` says the parent's shapes, everything else is device memory
int loo_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &ps, const int32_t *d_count, const double *d_F, const int32_t *d_keep,
            const sbgpu_loo_params_t *params, void *stream, sbgpu_em_loo_t *out)
{
   const int64_t nl = ps.n_loci, n_bins = ps.n_rows, n_iso = ps.n_iso;
   if (params && (params->max_bytes < 0 || params->reserved != 0)) return api_fail(SBGPU_EINVAL, who + ": max_bytes is negative, or reserved is not 0");
   const int64_t budget = params && params->max_bytes > 0 ? params->max_bytes : sb::kLooDefaultBytes;
   bool any_weight = false;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t nb = ps.row_off[l + 1] - ps.row_off[l], niso = ps.iso_off[l + 1] - ps.iso_off[l];
      if (nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      if (niso > 32 * (int64_t)sb::kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
      any_weight |= nb * niso > 0;
   }
   if (n_bins && !d_count) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if (any_weight && !d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   if (out->theta_without && !out->without_off) return api_fail(SBGPU_EINVAL, who + ": theta_without is given without without_off (sbgpu_em_loo_offsets makes it)");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the shapes (rules 1, 2, 9), on the host: keep comes back once
   std::vector<int32_t> keep;
   if (d_keep && n_iso) {
      keep.resize((size_t)n_iso);
      SB_STAGE_TRY(hipMemcpyAsync(keep.data(), d_keep, (size_t)n_iso * 4, hipMemcpyDeviceToHost, s));
      SB_STAGE_TRY(hipStreamSynchronize(s));
   }
   sb::LooShapes sh;
   sb::loo_shapes(nl, ps.row_off, ps.iso_off, d_keep ? keep.data() : nullptr, &sh);
   if (out->theta_without && !std::equal(sh.without_off.begin(), sh.without_off.end(), out->without_off))
      return api_fail(SBGPU_EINVAL, who + ": without_off is not sbgpu_em_loo_offsets' for this batch");
   // ---- the chunks: consecutive whole loci while their sub-problems fit the budget; a locus above it is a chunk alone
   std::vector<LooChunk> chunks;
   {
      int64_t used = 0;
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t fs = sh.first_sub[(size_t)l], K = sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l];
         const int64_t n = fs < 0 ? 0 : sb::loo_n_sub(K);
         int64_t bytes = 0;
         if (n) {
            const int64_t rows = sh.sub_row_off[(size_t)(fs + n)] - sh.sub_row_off[(size_t)fs], iso = sh.sub_iso_off[(size_t)(fs + n)] - sh.sub_iso_off[(size_t)fs];
            bytes = 8 * (sh.sub_f_off[(size_t)(fs + n)] - sh.sub_f_off[(size_t)fs]) + 21 * rows + 28 * iso + 80 * n; // F; count, live, expected, resid; theta, gain, score, keep; per-locus results
         }
         if (chunks.empty() || (used && used + bytes > budget)) {
            chunks.emplace_back();
            chunks.back().l0 = l;
            used = 0;
         }
         chunks.back().l1 = l + 1;
         used += bytes;
      }
   }
   size_t chunk_bytes = 0;
   int64_t s_next = 0;
   for (LooChunk &k : chunks) {
      k.s0 = s_next;
      for (int64_t l = k.l0; l < k.l1; ++l)
         if (sh.first_sub[(size_t)l] >= 0) s_next = sh.first_sub[(size_t)l] + sb::loo_n_sub(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      k.s1 = s_next;
      const int64_t n_sub = k.s1 - k.s0;
      k.row_off.resize((size_t)n_sub + 1), k.iso_off.resize((size_t)n_sub + 1), k.f_off.resize((size_t)n_sub + 1);
      for (int64_t q = 0; q <= n_sub; ++q) {
         k.row_off[(size_t)q] = sh.sub_row_off[(size_t)(k.s0 + q)] - sh.sub_row_off[(size_t)k.s0];
         k.iso_off[(size_t)q] = sh.sub_iso_off[(size_t)(k.s0 + q)] - sh.sub_iso_off[(size_t)k.s0];
         k.f_off[(size_t)q] = sh.sub_f_off[(size_t)(k.s0 + q)] - sh.sub_f_off[(size_t)k.s0];
      }
      for (int64_t l = k.l0; l < k.l1; ++l) {
         if (sh.first_sub[(size_t)l] < 0) continue;
         const int nb = (int)(ps.row_off[l + 1] - ps.row_off[l]);
         const int step = sb::loo_tile_rows((int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]));
         for (int r = 0; r < nb; r += step) k.tiles.push_back({(int32_t)l, r, std::min(step, nb - r), 0});
      }
      sb::PlanShape sub; // (the host side only: what fit_plan reads)
      sub.n_loci = n_sub, sub.n_rows = k.row_off.back(), sub.n_iso = k.iso_off.back();
      sub.row_off = k.row_off.data(), sub.iso_off = k.iso_off.data();
      if (const int rc = sb::fit_plan(who, sub, true, false, &k.fit); rc != SBGPU_OK) return rc;
      k.L = sb::loo_chunk_layout((int64_t)k.tiles.size(), n_sub, sub.n_rows, sub.n_iso, k.f_off.back(), k.fit.L.bytes);
      chunk_bytes = std::max(chunk_bytes, k.L.bytes);
   }
   // ---- the arena (stage_host.h: loo_layout): the call's results, then one chunk's working set
   const int64_t n_without = sh.without_off[(size_t)n_iso];
   const sb::LooLayout L = sb::loo_layout(nl, n_iso, (int64_t)sh.kept_col.size(), n_without, chunk_bytes);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchLoo, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock host(L.upload_bytes);
   host.put(L.lstat, sh.loo_status.data(), sh.loo_status.size()), host.put(L.woff, sh.without_off.data(), sh.without_off.size());
   host.put(L.rank, sh.rank.data(), sh.rank.size()), host.put(L.first, sh.first_sub.data(), sh.first_sub.size());
   host.put(L.koff, sh.kept_off.data(), sh.kept_off.size()), host.put(L.kcol, sh.kept_col.data(), sh.kept_col.size());
   SB_STAGE_TRY(host.upload(d, s));
   sb::LooStatArgs st;
   st.iso_off = ps.d_iso_off;
   st.loo_status = sb::arena_at<int32_t>(d, L.lstat), st.rank = sb::arena_at<int32_t>(d, L.rank);
   st.first_sub = sb::arena_at<int64_t>(d, L.first), st.kept_off = sb::arena_at<int64_t>(d, L.koff), st.kept_col = sb::arena_at<int32_t>(d, L.kcol);
   st.without_off = sb::arena_at<int64_t>(d, L.woff);
   st.lr_stat = sb::arena_at<double>(d, L.lr), st.heir_gain = sb::arena_at<double>(d, L.hgain), st.theta_refit = sb::arena_at<double>(d, L.refit);
   st.n_unique = sb::arena_at<long long>(d, L.nuniq);
   st.heir = sb::arena_at<int32_t>(d, L.heir), st.status_without = sb::arena_at<int32_t>(d, L.stw), st.iters_without = sb::arena_at<int32_t>(d, L.itw);
   st.support = sb::arena_at<int32_t>(d, L.supp);
   st.loglik_base = sb::arena_at<double>(d, L.llb), st.status_base = sb::arena_at<int32_t>(d, L.stb), st.iters_base = sb::arena_at<int32_t>(d, L.itb);
   st.theta_without = sb::arena_at<double>(d, L.wo);
   sb::LooExpandArgs ex;
   ex.row_off = ps.d_row_off, ex.iso_off = ps.d_iso_off, ex.f_off = ps.d_f_off;
   ex.count = d_count, ex.F = d_F;
   ex.first_sub = st.first_sub, ex.kept_off = st.kept_off, ex.kept_col = st.kept_col;
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kLooGridPerCu;
   char *w = d + L.chunk;
   // (sbgpu_set_timing: a chunk's launches as stages of their own, for tools/bench_support.py)
   sb::ctx_stage_reset(c);
   for (const LooChunk &k : chunks) {
      const int64_t n_sub = k.s1 - k.s0;
      PlanGuard plan;
      sb::HostBlock tiles(k.L.upload_bytes), lists(k.fit.L.upload_bytes);
      double *sub_theta = sb::arena_at<double>(w, k.L.theta);
      int32_t *sub_status = sb::arena_at<int32_t>(w, k.L.status), *sub_iters = sb::arena_at<int32_t>(w, k.L.iters);
      char *fit = w + k.L.fit;
      sb::PlanShape sub;
      if (n_sub) {
         if (const int rc = sbgpu_plan_create(c, n_sub, k.row_off.data(), k.iso_off.data(), k.f_off.data(), &plan.p); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sub = sb::plan_shape(plan.p);
         // ---- the expansion
         tiles.put(k.L.tiles, k.tiles.data(), k.tiles.size());
         SB_STAGE_TRY(tiles.upload(w, s));
         ex.n_tiles = (int64_t)k.tiles.size(), ex.tiles = sb::arena_at<sb::LooTile>(w, k.L.tiles);
         ex.sub0 = k.s0, ex.sub_row_off = sub.d_row_off, ex.sub_f_off = sub.d_f_off;
         ex.sub_count = sb::arena_at<int32_t>(w, k.L.count), ex.sub_F = sb::arena_at<double>(w, k.L.F);
         sb::ctx_stage_begin(c, "loo_expand", s);
         if (ex.n_tiles) {
            hipLaunchKernelGGL(sb::loo_expand_kernel, dim3(sb::stage_grid(ex.n_tiles, cap)), dim3(sb::kLooThreads), 0, s, ex);
            SB_STAGE_TRY(hipGetLastError());
         }
         sb::ctx_stage_end(c, s);
         if (out->sub_count) SB_STAGE_TRY(sb::copy_back(out->sub_count + sh.sub_row_off[(size_t)k.s0], w, k.L.count, k.row_off.back(), s));
         if (out->sub_F) SB_STAGE_TRY(sb::copy_back(out->sub_F + sh.sub_f_off[(size_t)k.s0], w, k.L.F, k.f_off.back(), s));
         // ---- the solves, then their fit with nothing erased
         sb::ctx_stage_begin(c, "loo_em", s);
         if (const int rc = sbgpu_em_run_device(c, plan.p, ex.sub_count, ex.sub_F, sub_theta, sub_status, sub_iters, s); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sb::ctx_stage_end(c, s);
         if (const int rc = sb::fit_launch(c, sub, k.fit, lists, fit, ex.sub_count, ex.sub_F, sub_theta, nullptr, sub_status, s); rc != SBGPU_OK) return rc;
      }
      // ---- the statistics of the chunk's loci (a locus without sub-problems gets its zeros here)
      st.l0 = k.l0, st.l1 = k.l1, st.sub0 = k.s0;
      st.sub_iso_off = sub.d_iso_off, st.sub_theta = sub_theta, st.sub_status = sub_status, st.sub_iters = sub_iters;
      st.sub_loglik = sb::arena_at<double>(fit, k.fit.L.ll);
      st.sub_n_live = sb::arena_at<long long>(fit, k.fit.L.nlive), st.sub_n_dropped = sb::arena_at<long long>(fit, k.fit.L.ndrop);
      st.sub_n_impossible = sb::arena_at<long long>(fit, k.fit.L.nimp);
      const int64_t n_threads = std::max(ps.iso_off[k.l1] - ps.iso_off[k.l0], k.l1 - k.l0);
      sb::ctx_stage_begin(c, "loo_stat", s);
      // (a few loads and stores per thread: one workgroup per CU is enough, the threads stride beyond)
      hipLaunchKernelGGL(sb::loo_stat_kernel, dim3(sb::stage_grid((n_threads + sb::kLooThreads - 1) / sb::kLooThreads, sb::ctx_cu_count(c))), dim3(sb::kLooThreads), 0, s, st);
      SB_STAGE_TRY(hipGetLastError());
      sb::ctx_stage_end(c, s);
      // the working set, the upload blocks and the plan are the next chunk's
      SB_STAGE_TRY(hipStreamSynchronize(s));
   }
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->lr_stat, d, L.lr, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->heir_gain, d, L.hgain, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_refit, d, L.refit, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->n_unique, d, L.nuniq, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->heir, d, L.heir, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->status_without, d, L.stw, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_without, d, L.itw, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->support, d, L.supp, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_base, d, L.llb, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loo_status, d, L.lstat, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_base, d, L.stb, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_base, d, L.itb, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_without, d, L.wo, n_without, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_lr_stat = st.lr_stat, out->d_heir_gain = st.heir_gain, out->d_theta_refit = st.theta_refit;
   out->d_n_unique = sb::arena_at<int64_t>(d, L.nuniq);
   out->d_heir = st.heir, out->d_status_without = st.status_without, out->d_iters_without = st.iters_without, out->d_support = st.support;
   out->d_loglik_base = st.loglik_base, out->d_loo_status = st.loo_status, out->d_status_base = st.status_base, out->d_iters_base = st.iters_base;
   out->d_theta_without = st.theta_without, out->d_without_off = st.without_off;
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_loo_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_loo_limits: null argument");
   const int64_t v[8] = {sb::kLooMaxKept, sb::kLooTileVals, sb::kLooTileRows, sb::kLooThreads, sb::kLooGridPerCu, sb::kLooDefaultBytes,
                         sb::kStageMaxBins, 32 * (int64_t)sb::kStageMaxWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_loo_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const int32_t *d_keep,
                                   const sbgpu_loo_params_t *params, void *stream, sbgpu_em_loo_t *out)
{
   if (!c || !plan || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_loo_device: null argument");
   loo_clear_device(out);
   return loo_run("sbgpu_em_loo_device", c, sb::plan_shape(plan), d_count, d_F, d_keep, params, stream, out);
}

extern "C" int sbgpu_model_loo_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const int32_t *d_keep, const sbgpu_loo_params_t *params, void *stream,
                                      sbgpu_em_loo_t *out)
{
   const std::string who = "sbgpu_model_loo_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   loo_clear_device(out);
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   sb::PlanShape ps;
   if (const int rc = sb::check_boot_keep(who, rec, sb::bins_context_view(bins), true, &ps); rc != SBGPU_OK) return rc;
   return loo_run(who, c, ps, rec->d_count, rec->d_F, d_keep, params, stream, out);
}
