// strawberry_amd/csrc/diff_api.hip -- sbgpu_em_diff_device, sbgpu_model_diff_device, sbgpu_em_diff_limits (include/sbgpu.h): the
// differential isoform usage of two samples, built from the arrays two batches have in HBM (diff_device.h).  The
// shapes are made on the host (diff_rules.h: diff_shapes); then, a chunk of whole loci at a time: a plan for the chunk's
// sub-batch, the column scales, the expansion, the EM through the library's own entry, the cross fit's inputs, the fit's launches
// (fit_api.hip: fit_launch) twice in this stage's scratch, the statistics.  The structure is loo_api.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "diff_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

void diff_clear_device(sbgpu_em_diff_t *out)
{
   out->d_theta_a = out->d_theta_b = out->d_theta_pooled = out->d_usage_a = out->d_usage_b = out->d_usage_pooled = out->d_delta_usage = nullptr;
   out->d_lr_stat = out->d_loglik_a = out->d_loglik_b = out->d_loglik_a_pooled = out->d_loglik_b_pooled = nullptr;
   out->d_n_a = out->d_n_b = out->d_lost_shift = nullptr;
   out->d_dof = out->d_diff_status = out->d_top_iso = out->d_status_a = out->d_status_b = out->d_status_pooled = nullptr;
   out->d_iters_a = out->d_iters_b = out->d_iters_pooled = nullptr;
}

// One chunk: loci [l0, l1), sub-problems [s0, s1) of the call, its sub-batch's offsets (beginning at 0) and its working set
struct DiffChunk {
   int64_t l0 = 0, l1 = 0, s0 = 0, s1 = 0;
   std::vector<int64_t> row_off, iso_off, f_off;
   std::vector<sb::DiffTile> tiles;
   std::vector<sb::DiffScaleItem> items;
   std::vector<int32_t> list; // the chunk's OK loci
   sb::FitPlan fit;
   sb::DiffChunkLayout L;
};

// the sub-batch's plan lives for one chunk
struct PlanGuard {
   sbgpu_plan_t *p = nullptr;
   ~PlanGuard() { sbgpu_plan_destroy(p); }
};

// The column-scale kernel's work: the OK loci of a chunk in order; consecutive narrow loci share a workgroup while their
// groups of lanes (the widest of them decides) fit its threads, a wide locus is alone.
void scale_items(const sb::DiffShapes &sh, const sb::PlanShape &pa, const sb::PlanShape &pb, DiffChunk *k)
{
   for (int64_t l = k->l0; l < k->l1; ++l) {
      if (sh.first_sub[(size_t)l] < 0) continue;
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      const int lanes = sb::diff_group_lanes(K);
      const int32_t rows = (int32_t)std::max(pa.row_off[l + 1] - pa.row_off[l], pb.row_off[l + 1] - pb.row_off[l]);
      const int32_t at = (int32_t)k->list.size();
      k->list.push_back((int32_t)l);
      if (lanes && !k->items.empty() && k->items.back().lanes > 0) {
         sb::DiffScaleItem &it = k->items.back();
         const int wider = std::max(it.lanes, lanes);
         if ((it.n + 1) * wider <= sb::kDiffThreads) {
            it.n += 1, it.lanes = wider, it.rows = std::max(it.rows, rows);
            continue;
         }
      }
      k->items.push_back({at, 1, lanes, rows});
   }
}

// the two entry points' common part: `pa` and `pb` say the samples' shapes, everything else is device memory
int diff_run(const std::string &who, sbgpu_ctx_t *c, const sb::PlanShape &pa, const int32_t *d_count_a, const double *d_F_a, const sb::PlanShape &pb,
             const int32_t *d_count_b, const double *d_F_b, const int32_t *d_keep_a, const int32_t *d_keep_b, const sbgpu_diff_params_t *params,
             void *stream, sbgpu_em_diff_t *out)
{
   const int64_t nl = pa.n_loci, n_iso = pa.n_iso;
   if (params && (params->max_bytes < 0 || params->reserved != 0)) return api_fail(SBGPU_EINVAL, who + ": max_bytes is negative, or reserved is not 0");
   const int64_t budget = params && params->max_bytes > 0 ? params->max_bytes : sb::kDiffDefaultBytes;
   if (pb.n_loci != nl) return api_fail(SBGPU_EINVAL, who + ": the two samples differ in n_loci");
   if (pb.n_iso != n_iso || !std::equal(pa.iso_off, pa.iso_off + nl + 1, pb.iso_off))
      return api_fail(SBGPU_EINVAL, who + ": the two samples differ in iso_off: they are not over one annotation");
   const sb::PlanShape *side[2] = {&pa, &pb};
   const int32_t *d_count[2] = {d_count_a, d_count_b};
   const double *d_F[2] = {d_F_a, d_F_b};
   for (int x = 0; x < 2; ++x) {
      bool any_weight = false;
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t nb = side[x]->row_off[l + 1] - side[x]->row_off[l], niso = pa.iso_off[l + 1] - pa.iso_off[l];
         if (nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
         if (niso > 32 * (int64_t)sb::kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
         any_weight |= nb * niso > 0;
      }
      if (side[x]->n_rows && !d_count[x]) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
      if (any_weight && !d_F[x]) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   }
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the shapes (rules 1, 2), on the host: the keeps come back once
   std::vector<int32_t> keep[2];
   const int32_t *d_keep[2] = {d_keep_a, d_keep_b};
   for (int x = 0; x < 2; ++x)
      if (d_keep[x] && n_iso) {
         keep[x].resize((size_t)n_iso);
         SB_STAGE_TRY(hipMemcpyAsync(keep[x].data(), d_keep[x], (size_t)n_iso * 4, hipMemcpyDeviceToHost, s));
      }
   SB_STAGE_TRY(hipStreamSynchronize(s));
   sb::DiffShapes sh;
   sb::diff_shapes(nl, pa.row_off, pb.row_off, pa.iso_off, d_keep_a ? keep[0].data() : nullptr, d_keep_b ? keep[1].data() : nullptr, &sh);
   // ---- the chunks: consecutive whole loci while their sub-problems fit the budget; a locus above it is a chunk alone
   std::vector<DiffChunk> chunks;
   {
      int64_t used = 0;
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t fs = sh.first_sub[(size_t)l];
         int64_t bytes = 0;
         if (fs >= 0) {
            const int64_t rows = sh.sub_row_off[(size_t)(fs + 3)] - sh.sub_row_off[(size_t)fs], iso = sh.sub_iso_off[(size_t)(fs + 3)] - sh.sub_iso_off[(size_t)fs];
            // F; count and the two fits' live, expected, resid; theta, the cross theta, alpha and the fits' gain, score, keep; per-sub results
            bytes = 8 * (sh.sub_f_off[(size_t)(fs + 3)] - sh.sub_f_off[(size_t)fs]) + 38 * rows + 64 * iso + 3 * 160;
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
   for (DiffChunk &k : chunks) {
      k.s0 = s_next;
      for (int64_t l = k.l0; l < k.l1; ++l)
         if (sh.first_sub[(size_t)l] >= 0) s_next = sh.first_sub[(size_t)l] + 3;
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
         const int step = sb::diff_tile_rows((int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]));
         for (int x = 0; x < 2; ++x) {
            const int nb = (int)(side[x]->row_off[l + 1] - side[x]->row_off[l]);
            for (int r = 0; r < nb; r += step) k.tiles.push_back({(int32_t)l, x, r, std::min(step, nb - r)});
         }
      }
      scale_items(sh, pa, pb, &k);
      sb::PlanShape sub; // (the host side only: what fit_plan reads)
      sub.n_loci = n_sub, sub.n_rows = k.row_off.back(), sub.n_iso = k.iso_off.back();
      sub.row_off = k.row_off.data(), sub.iso_off = k.iso_off.data();
      if (const int rc = sb::fit_plan(who, sub, true, false, &k.fit); rc != SBGPU_OK) return rc;
      k.L = sb::diff_chunk_layout((int64_t)k.tiles.size(), (int64_t)k.items.size(), (int64_t)k.list.size(),
                                  sh.kept_off[(size_t)k.l1] - sh.kept_off[(size_t)k.l0], n_sub, sub.n_rows, sub.n_iso, k.f_off.back(), k.fit.L.bytes);
      chunk_bytes = std::max(chunk_bytes, k.L.bytes);
   }
   // ---- the arena (stage_host.h: diff_layout): the call's results, then one chunk's working set
   const sb::DiffLayout L = sb::diff_layout(nl, n_iso, (int64_t)sh.kept_col.size(), chunk_bytes);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchDiff, L.bytes, &d); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock host(L.upload_bytes);
   host.put(L.lstat, sh.diff_status.data(), sh.diff_status.size()), host.put(L.rank, sh.rank.data(), sh.rank.size());
   host.put(L.first, sh.first_sub.data(), sh.first_sub.size()), host.put(L.koff, sh.kept_off.data(), sh.kept_off.size());
   host.put(L.kcol, sh.kept_col.data(), sh.kept_col.size());
   SB_STAGE_TRY(host.upload(d, s));
   const auto u = [](size_t at) { return (uint32_t)(at / 256); }; // (Arena::take's grain: every offset is a multiple of it)
   sb::DiffStatArgs st;
   st.iso_off = pa.d_iso_off, st.res = d;
   sb::DiffStatOff &so = st.o;
   so.pre_status = u(L.lstat), so.rank = u(L.rank), so.first_sub = u(L.first), so.kept_off = u(L.koff), so.kept_col = u(L.kcol);
   so.theta[0] = u(L.th_a), so.theta[1] = u(L.th_b), so.theta[2] = u(L.th_p), so.usage[0] = u(L.us_a), so.usage[1] = u(L.us_b), so.usage[2] = u(L.us_p);
   so.delta = u(L.delta), so.lr_stat = u(L.lr), so.loglik[0] = u(L.ll_a), so.loglik[1] = u(L.ll_b), so.loglik[2] = u(L.llx_a), so.loglik[3] = u(L.llx_b);
   so.n_a = u(L.n_a), so.n_b = u(L.n_b), so.lost_shift = u(L.shift), so.dof = u(L.dof), so.status = u(L.status), so.top_iso = u(L.top);
   so.st[0] = u(L.st_a), so.st[1] = u(L.st_b), so.st[2] = u(L.st_p), so.it[0] = u(L.it_a), so.it[1] = u(L.it_b), so.it[2] = u(L.it_p);
   so.sum[0] = u(L.sum_a), so.sum[1] = u(L.sum_b), so.sum[2] = u(L.sum_p);
   const int64_t *d_first = sb::arena_at<int64_t>(d, L.first), *d_koff = sb::arena_at<int64_t>(d, L.koff);
   const int32_t *d_kcol = sb::arena_at<int32_t>(d, L.kcol);
   sb::DiffScaleArgs sc;
   sb::DiffExpandArgs ex;
   for (int x = 0; x < 2; ++x) {
      sc.row_off[x] = ex.row_off[x] = st.row_off[x] = side[x]->d_row_off;
      sc.f_off[x] = ex.f_off[x] = side[x]->d_f_off;
      sc.F[x] = ex.F[x] = d_F[x];
      ex.count[x] = st.count[x] = d_count[x];
   }
   sc.iso_off = ex.iso_off = pa.d_iso_off;
   sc.kept_off = ex.kept_off = d_koff, sc.kept_col = ex.kept_col = d_kcol;
   ex.first_sub = d_first;
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kDiffGridPerCu;
   char *w = d + L.chunk;
   // (sbgpu_set_timing: a chunk's launches as stages of their own, as the support's are)
   sb::ctx_stage_reset(c);
   for (const DiffChunk &k : chunks) {
      const int64_t n_sub = k.s1 - k.s0;
      PlanGuard plan;
      sb::HostBlock work(k.L.upload_bytes), lists(k.fit.L.upload_bytes), x_lists(k.fit.L.upload_bytes);
      double *sub_theta = sb::arena_at<double>(w, k.L.theta), *x_theta = sb::arena_at<double>(w, k.L.x_theta);
      int32_t *sub_status = sb::arena_at<int32_t>(w, k.L.status), *sub_iters = sb::arena_at<int32_t>(w, k.L.iters);
      int32_t *x_status = sb::arena_at<int32_t>(w, k.L.x_status);
      char *fit = w + k.L.fit, *x_fit = w + k.L.x_fit;
      sb::PlanShape sub;
      if (n_sub) {
         if (const int rc = sbgpu_plan_create(c, n_sub, k.row_off.data(), k.iso_off.data(), k.f_off.data(), &plan.p); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sub = sb::plan_shape(plan.p);
         work.put(k.L.tiles, k.tiles.data(), k.tiles.size()), work.put(k.L.items, k.items.data(), k.items.size());
         work.put(k.L.list, k.list.data(), k.list.size());
         SB_STAGE_TRY(work.upload(w, s));
         // ---- rule 3: the column scales
         sc.n_items = (int64_t)k.items.size(), sc.items = sb::arena_at<sb::DiffScaleItem>(w, k.L.items), sc.list = sb::arena_at<int32_t>(w, k.L.list);
         sc.kept0 = ex.kept0 = sh.kept_off[(size_t)k.l0];
         sc.alpha = sb::arena_at<double>(w, k.L.alpha), ex.alpha = sc.alpha;
         sb::ctx_stage_begin(c, "diff_colscale", s);
         hipLaunchKernelGGL(sb::diff_colscale_kernel, dim3(sb::stage_grid(sc.n_items, cap)), dim3(sb::kDiffThreads), 0, s, sc);
         SB_STAGE_TRY(hipGetLastError());
         sb::ctx_stage_end(c, s);
         // ---- rule 2: the expansion
         ex.n_tiles = (int64_t)k.tiles.size(), ex.tiles = sb::arena_at<sb::DiffTile>(w, k.L.tiles);
         ex.sub0 = k.s0, ex.sub_row_off = sub.d_row_off, ex.sub_f_off = sub.d_f_off;
         ex.sub_count = sb::arena_at<int32_t>(w, k.L.count), ex.sub_F = sb::arena_at<double>(w, k.L.F);
         sb::ctx_stage_begin(c, "diff_expand", s);
         if (ex.n_tiles) {
            hipLaunchKernelGGL(sb::diff_expand_kernel, dim3(sb::stage_grid(ex.n_tiles, cap)), dim3(sb::kDiffThreads), 0, s, ex);
            SB_STAGE_TRY(hipGetLastError());
         }
         sb::ctx_stage_end(c, s);
         if (out->sub_count) SB_STAGE_TRY(sb::copy_back(out->sub_count + sh.sub_row_off[(size_t)k.s0], w, k.L.count, k.row_off.back(), s));
         if (out->sub_F) SB_STAGE_TRY(sb::copy_back(out->sub_F + sh.sub_f_off[(size_t)k.s0], w, k.L.F, k.f_off.back(), s));
         // ---- rule 4: the solves, their own fit, and the fit of A and B at the pooled theta, nothing erased
         sb::ctx_stage_begin(c, "diff_em", s);
         if (const int rc = sbgpu_em_run_device(c, plan.p, ex.sub_count, ex.sub_F, sub_theta, sub_status, sub_iters, s); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sb::ctx_stage_end(c, s);
         sb::DiffCrossArgs cr{n_sub, sub.d_iso_off, sub_theta, sub_status, x_theta, x_status};
         sb::ctx_stage_begin(c, "diff_cross", s);
         hipLaunchKernelGGL(sb::diff_cross_kernel, dim3(sb::stage_grid((std::max(sub.n_iso, n_sub) + sb::kDiffThreads - 1) / sb::kDiffThreads, sb::ctx_cu_count(c))),
                            dim3(sb::kDiffThreads), 0, s, cr);
         SB_STAGE_TRY(hipGetLastError());
         sb::ctx_stage_end(c, s);
         if (const int rc = sb::fit_launch(c, sub, k.fit, lists, fit, ex.sub_count, ex.sub_F, sub_theta, nullptr, sub_status, s); rc != SBGPU_OK) return rc;
         if (const int rc = sb::fit_launch(c, sub, k.fit, x_lists, x_fit, ex.sub_count, ex.sub_F, x_theta, nullptr, x_status, s); rc != SBGPU_OK) return rc;
      }
      // ---- the statistics of the chunk's loci (a locus without sub-problems gets its zeros here)
      st.l0 = k.l0, st.l1 = k.l1, st.sub0 = k.s0;
      st.sub_iso_off = sub.d_iso_off, st.sub_theta = sub_theta, st.sub_status = sub_status, st.sub_iters = sub_iters;
      st.fit = fit, st.x_fit = x_fit;
      so.fit_loglik = u(k.fit.L.ll), so.fit_n_live = u(k.fit.L.nlive), so.fit_n_dropped = u(k.fit.L.ndrop), so.fit_n_impossible = u(k.fit.L.nimp);
      const int64_t n_loci_k = k.l1 - k.l0, n_iso_k = pa.iso_off[k.l1] - pa.iso_off[k.l0];
      sb::ctx_stage_begin(c, "diff_stat", s);
      // the loci (a thread each), then their isoforms (a few loads and stores per thread: one workgroup per CU is enough, the
      // threads stride beyond)
      hipLaunchKernelGGL(sb::diff_stat_kernel<0>, dim3((unsigned)((n_loci_k + sb::kDiffThreads - 1) / sb::kDiffThreads)), dim3(sb::kDiffThreads), 0, s, st);
      SB_STAGE_TRY(hipGetLastError());
      if (n_iso_k) {
         hipLaunchKernelGGL(sb::diff_stat_kernel<1>, dim3(sb::stage_grid((n_iso_k + sb::kDiffThreads - 1) / sb::kDiffThreads, sb::ctx_cu_count(c))),
                            dim3(sb::kDiffThreads), 0, s, st);
         SB_STAGE_TRY(hipGetLastError());
      }
      sb::ctx_stage_end(c, s);
      // the working set, the upload blocks and the plan are the next chunk's
      SB_STAGE_TRY(hipStreamSynchronize(s));
   }
   // ---- results: what the caller asked for
   SB_STAGE_TRY(sb::copy_back(out->theta_a, d, L.th_a, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_b, d, L.th_b, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_pooled, d, L.th_p, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_a, d, L.us_a, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_b, d, L.us_b, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_pooled, d, L.us_p, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->delta_usage, d, L.delta, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->lr_stat, d, L.lr, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_a, d, L.ll_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_b, d, L.ll_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_a_pooled, d, L.llx_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_b_pooled, d, L.llx_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_a, d, L.n_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_b, d, L.n_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->lost_shift, d, L.shift, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->dof, d, L.dof, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->diff_status, d, L.status, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->top_iso, d, L.top, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_a, d, L.st_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_b, d, L.st_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_pooled, d, L.st_p, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_a, d, L.it_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_b, d, L.it_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_pooled, d, L.it_p, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_theta_a = sb::arena_at<double>(d, L.th_a), out->d_theta_b = sb::arena_at<double>(d, L.th_b), out->d_theta_pooled = sb::arena_at<double>(d, L.th_p);
   out->d_usage_a = sb::arena_at<double>(d, L.us_a), out->d_usage_b = sb::arena_at<double>(d, L.us_b), out->d_usage_pooled = sb::arena_at<double>(d, L.us_p);
   out->d_delta_usage = sb::arena_at<double>(d, L.delta), out->d_lr_stat = sb::arena_at<double>(d, L.lr);
   out->d_loglik_a = sb::arena_at<double>(d, L.ll_a), out->d_loglik_b = sb::arena_at<double>(d, L.ll_b);
   out->d_loglik_a_pooled = sb::arena_at<double>(d, L.llx_a), out->d_loglik_b_pooled = sb::arena_at<double>(d, L.llx_b);
   out->d_n_a = sb::arena_at<int64_t>(d, L.n_a), out->d_n_b = sb::arena_at<int64_t>(d, L.n_b), out->d_lost_shift = sb::arena_at<int64_t>(d, L.shift);
   out->d_dof = sb::arena_at<int32_t>(d, L.dof), out->d_diff_status = sb::arena_at<int32_t>(d, L.status), out->d_top_iso = sb::arena_at<int32_t>(d, L.top);
   out->d_status_a = sb::arena_at<int32_t>(d, L.st_a), out->d_status_b = sb::arena_at<int32_t>(d, L.st_b), out->d_status_pooled = sb::arena_at<int32_t>(d, L.st_p);
   out->d_iters_a = sb::arena_at<int32_t>(d, L.it_a), out->d_iters_b = sb::arena_at<int32_t>(d, L.it_b), out->d_iters_pooled = sb::arena_at<int32_t>(d, L.it_p);
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_diff_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_diff_limits: null argument");
   const int64_t v[8] = {sb::kDiffMaxKept,  sb::kDiffMaxPooledBins, sb::kDiffTileVals,  sb::kDiffTileRows,
                         sb::kDiffGroupMaxKept, sb::kDiffThreads,   sb::kDiffGridPerCu, sb::kDiffDefaultBytes};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_diff_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan_a, const int32_t *d_count_a, const double *d_F_a, const sbgpu_plan_t *plan_b,
                                    const int32_t *d_count_b, const double *d_F_b, const int32_t *d_keep_a, const int32_t *d_keep_b,
                                    const sbgpu_diff_params_t *params, void *stream, sbgpu_em_diff_t *out)
{
   if (!c || !plan_a || !plan_b || !out) return api_fail(SBGPU_EINVAL, "sbgpu_em_diff_device: null argument");
   diff_clear_device(out);
   return diff_run("sbgpu_em_diff_device", c, sb::plan_shape(plan_a), d_count_a, d_F_a, sb::plan_shape(plan_b), d_count_b, d_F_b, d_keep_a, d_keep_b, params,
                   stream, out);
}

extern "C" int sbgpu_model_diff_device(sbgpu_ctx_t *ctx_a, const sbgpu_bins_t *bins_a, sbgpu_ctx_t *ctx_b, const sbgpu_bins_t *bins_b,
                                       const int32_t *d_keep_a, const int32_t *d_keep_b, const sbgpu_diff_params_t *params, void *stream,
                                       sbgpu_em_diff_t *out)
{
   const std::string who = "sbgpu_model_diff_device";
   if (!ctx_a || !bins_a || !ctx_b || !bins_b || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   diff_clear_device(out);
   if (sb::ctx_device(ctx_a) != sb::ctx_device(ctx_b)) return api_fail(SBGPU_EINVAL, who + ": the two contexts are on different devices");
   const sb::BootKeep *rec_a = sb::ctx_boot_keep(ctx_a), *rec_b = sb::ctx_boot_keep(ctx_b);
   sb::PlanShape pa, pb;
   if (const int rc = sb::check_boot_keep(who, rec_a, sb::bins_context_view(bins_a), true, &pa); rc != SBGPU_OK) return rc;
   if (const int rc = sb::check_boot_keep(who, rec_b, sb::bins_context_view(bins_b), true, &pb); rc != SBGPU_OK) return rc;
   // sample B's arrays were written on ctx_b's stream: they are read on ctx_a's (or the caller's) from here on
   if (ctx_b != ctx_a) {
      if (hipError_t e = hipSetDevice(sb::ctx_device(ctx_b)); e != hipSuccess) return sb::api_fail_hip(e, "hipSetDevice");
      if (hipError_t e = hipStreamSynchronize(sb::ctx_stream(ctx_b)); e != hipSuccess) return sb::api_fail_hip(e, "hipStreamSynchronize");
   }
   return diff_run(who, ctx_a, pa, rec_a->d_count, rec_a->d_F, pb, rec_b->d_count, rec_b->d_F, d_keep_a, d_keep_b, params, stream, out);
}
