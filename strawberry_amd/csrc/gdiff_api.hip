// strawberry_amd/csrc/gdiff_api.hip -- sbgpu_em_gdiff_device, sbgpu_model_gdiff_device, sbgpu_em_gdiff_limits (include/sbgpu.h):
// the differential isoform usage between two groups of replicate samples, built from the arrays S batches have in HBM
// (gdiff_device.h).  The shapes are made on the host (gdiff_rules.h: gdiff_shapes); then, a chunk of whole loci at a
// time: a plan for the chunk's sub-batch, the column scales, the expansion, the EM through the library's own entry, the group
// level's cross inputs and fit, ALL's cross inputs and fit, the own fit (fit_api.hip: fit_launch, three times in this stage's
// scratch), the statistics.  The structure is diff_api.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "gdiff_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

void gdiff_clear_device(sbgpu_em_gdiff_t *out)
{
   out->d_theta_sample = out->d_theta_group = out->d_theta_all = out->d_usage_sample = out->d_usage_group = out->d_usage_all = out->d_delta_usage = nullptr;
   out->d_lr_between = out->d_lr_within = out->d_loglik_own = out->d_loglik_group = out->d_loglik_all = nullptr;
   out->d_n_frag = out->d_lost_shift = nullptr;
   out->d_dof_between = out->d_dof_within = out->d_p_a = out->d_p_b = out->d_gdiff_status = out->d_top_iso = nullptr;
   out->d_status_sample = out->d_iters_sample = out->d_status_group = out->d_iters_group = out->d_status_all = out->d_iters_all = nullptr;
}

int check_groups(const std::string &who, int32_t n_a, int32_t n_b)
{
   if (n_a < 1 || n_b < 1) return api_fail(SBGPU_EINVAL, who + ": a group without samples (n_a and n_b are at least 1)");
   if ((int64_t)n_a + n_b > sb::kGdiffMaxSamples) return api_fail(SBGPU_EINVAL, who + ": more than 16 samples");
   return SBGPU_OK;
}

// One chunk: loci [l0, l1), sub-problems [s0, s1) of the call, its sub-batch's offsets (beginning at 0) and its working set
struct GdiffChunk {
   int64_t l0 = 0, l1 = 0, s0 = 0, s1 = 0;
   std::vector<int64_t> row_off, iso_off, f_off;
   std::vector<sb::GdiffTile> tiles;
   std::vector<sb::GdiffScaleItem> items;
   std::vector<int32_t> list;         // the chunk's OK loci
   std::vector<int32_t> src_g, src_a; // per sub-problem: whose theta it is fitted at on the group level and on ALL's
   sb::FitPlan fit;
   sb::GdiffChunkLayout L;
};

// the sub-batch's plan lives for one chunk
struct PlanGuard {
   sbgpu_plan_t *p = nullptr;
   ~PlanGuard() { sbgpu_plan_destroy(p); }
};

// The column-scale kernel's work, as diff_api.hip's scale_items: the OK loci of a chunk in order; consecutive narrow loci share
// a workgroup while their groups of lanes fit its threads, a wide locus is alone.
void scale_items(const sb::GdiffShapes &sh, const std::vector<sb::PlanShape> &ps, GdiffChunk *k)
{
   for (int64_t l = k->l0; l < k->l1; ++l) {
      if (sh.first_sub[(size_t)l] < 0) continue;
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      const int lanes = sb::gdiff_group_lanes(K);
      int32_t rows = 0, mask = 0;
      for (int s = 0; s < sh.S; ++s) {
         const int64_t nb = ps[(size_t)s].row_off[l + 1] - ps[(size_t)s].row_off[l];
         rows = std::max(rows, (int32_t)nb);
         if (nb > 0) mask |= 1 << s;
      }
      const int32_t at = (int32_t)k->list.size();
      k->list.push_back((int32_t)l);
      if (lanes && !k->items.empty() && k->items.back().lanes > 0) {
         sb::GdiffScaleItem &it = k->items.back();
         const int wider = std::max(it.lanes, lanes);
         if ((it.n + 1) * wider <= sb::kGdiffThreads) {
            it.n += 1, it.lanes = wider, it.rows = std::max(it.rows, rows), it.mask |= mask;
            continue;
         }
      }
      k->items.push_back({at, 1, lanes, rows, mask, {0, 0, 0}});
   }
}

// the two entry points' common part: `ps` says the samples' shapes, everything else is device memory
int gdiff_run(const std::string &who, sbgpu_ctx_t *c, int n_a, int n_b, const std::vector<sb::PlanShape> &ps, const int32_t *const *d_count,
              const double *const *d_F, const int32_t *const *d_keep, const sbgpu_gdiff_params_t *params, void *stream, sbgpu_em_gdiff_t *out)
{
   const int S = n_a + n_b, slots = S + 3;
   const int64_t nl = ps[0].n_loci, n_iso = ps[0].n_iso;
   if (params && (params->max_bytes < 0 || params->reserved != 0)) return api_fail(SBGPU_EINVAL, who + ": max_bytes is negative, or reserved is not 0");
   const int64_t budget = params && params->max_bytes > 0 ? params->max_bytes : sb::kGdiffDefaultBytes;
   for (int x = 0; x < S; ++x) {
      if (ps[(size_t)x].n_loci != nl) return api_fail(SBGPU_EINVAL, who + ": the samples differ in n_loci");
      if (ps[(size_t)x].n_iso != n_iso || !std::equal(ps[0].iso_off, ps[0].iso_off + nl + 1, ps[(size_t)x].iso_off))
         return api_fail(SBGPU_EINVAL, who + ": the samples differ in iso_off: they are not over one annotation");
   }
   for (int x = 0; x < S; ++x) {
      bool any_weight = false;
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t nb = ps[(size_t)x].row_off[l + 1] - ps[(size_t)x].row_off[l], niso = ps[0].iso_off[l + 1] - ps[0].iso_off[l];
         if (nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
         if (niso > 32 * (int64_t)sb::kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
         any_weight |= nb * niso > 0;
      }
      if (ps[(size_t)x].n_rows && !d_count[x]) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
      if (any_weight && !d_F[x]) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   }
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the shapes (rules 1, 2), on the host: the keeps come back once
   std::vector<std::vector<int32_t>> keep((size_t)S);
   std::vector<const int32_t *> keep_p((size_t)S, nullptr);
   std::vector<const int64_t *> row_off((size_t)S);
   for (int x = 0; x < S; ++x) {
      row_off[(size_t)x] = ps[(size_t)x].row_off;
      if (d_keep && d_keep[x] && n_iso) {
         keep[(size_t)x].resize((size_t)n_iso);
         SB_STAGE_TRY(hipMemcpyAsync(keep[(size_t)x].data(), d_keep[x], (size_t)n_iso * 4, hipMemcpyDeviceToHost, s));
      }
   }
   SB_STAGE_TRY(hipStreamSynchronize(s));
   for (int x = 0; x < S; ++x)
      if (d_keep && d_keep[x]) keep_p[(size_t)x] = keep[(size_t)x].data(); // (n_iso = 0: nothing is read through it)
   sb::GdiffShapes sh;
   sb::gdiff_shapes(nl, n_a, n_b, row_off.data(), ps[0].iso_off, keep_p.data(), &sh);
   // the sub-problems of locus l: [first_sub[l], the next locus' first or the call's end)
   const auto subs_end = [&sh](int64_t l) { return sh.slot_sub[(size_t)l * (size_t)sh.slots() + (size_t)sh.S + 2] + 1; };
   // ---- the chunks: consecutive whole loci while their sub-problems fit the budget; a locus above it is a chunk alone
   std::vector<GdiffChunk> chunks;
   {
      int64_t used = 0;
      for (int64_t l = 0; l < nl; ++l) {
         const int64_t fs = sh.first_sub[(size_t)l];
         int64_t bytes = 0;
         if (fs >= 0) {
            const int64_t fe = subs_end(l);
            const int64_t rows = sh.sub_row_off[(size_t)fe] - sh.sub_row_off[(size_t)fs], iso = sh.sub_iso_off[(size_t)fe] - sh.sub_iso_off[(size_t)fs];
            // F; count and the three fits' live, expected, resid; theta, the two cross thetas, c, the alphas and the fits' gain, score, keep; per-sub results
            bytes = 8 * (sh.sub_f_off[(size_t)fe] - sh.sub_f_off[(size_t)fs]) + 55 * rows + 108 * iso + (fe - fs) * 240;
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
   for (GdiffChunk &k : chunks) {
      k.s0 = s_next;
      for (int64_t l = k.l0; l < k.l1; ++l)
         if (sh.first_sub[(size_t)l] >= 0) s_next = subs_end(l);
      k.s1 = s_next;
      const int64_t n_sub = k.s1 - k.s0;
      k.row_off.resize((size_t)n_sub + 1), k.iso_off.resize((size_t)n_sub + 1), k.f_off.resize((size_t)n_sub + 1);
      for (int64_t q = 0; q <= n_sub; ++q) {
         k.row_off[(size_t)q] = sh.sub_row_off[(size_t)(k.s0 + q)] - sh.sub_row_off[(size_t)k.s0];
         k.iso_off[(size_t)q] = sh.sub_iso_off[(size_t)(k.s0 + q)] - sh.sub_iso_off[(size_t)k.s0];
         k.f_off[(size_t)q] = sh.sub_f_off[(size_t)(k.s0 + q)] - sh.sub_f_off[(size_t)k.s0];
      }
      k.src_g.resize((size_t)n_sub), k.src_a.resize((size_t)n_sub);
      for (int64_t q = 0; q < n_sub; ++q) k.src_g[(size_t)q] = k.src_a[(size_t)q] = (int32_t)q; // (a group's and ALL's: their own)
      for (int64_t l = k.l0; l < k.l1; ++l) {
         if (sh.first_sub[(size_t)l] < 0) continue;
         const int64_t *slot = sh.slot_sub.data() + (size_t)l * (size_t)slots;
         const int step = sb::gdiff_tile_rows((int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]));
         int64_t grp_row[2] = {0, 0}, all_row = 0;
         for (int x = 0; x < S; ++x) {
            if (slot[x] < 0) continue;
            const int g = x >= n_a;
            const int nb = (int)(ps[(size_t)x].row_off[l + 1] - ps[(size_t)x].row_off[l]);
            const int32_t own_q = (int32_t)(slot[x] - k.s0), grp_q = sh.group_has_sub(l, g) ? (int32_t)(slot[S + g] - k.s0) : -1;
            const int32_t all_q = (int32_t)(slot[S + 2] - k.s0);
            k.src_g[(size_t)own_q] = (int32_t)(slot[S + g] - k.s0), k.src_a[(size_t)own_q] = all_q;
            for (int r = 0; r < nb; r += step)
               k.tiles.push_back({(int32_t)l, x, r, std::min(step, nb - r), own_q, grp_q, all_q, (int32_t)grp_row[g], (int32_t)all_row, {0, 0, 0}});
            grp_row[g] += nb, all_row += nb;
         }
      }
      scale_items(sh, ps, &k);
      sb::PlanShape sub; // (the host side only: what fit_plan reads)
      sub.n_loci = n_sub, sub.n_rows = k.row_off.back(), sub.n_iso = k.iso_off.back();
      sub.row_off = k.row_off.data(), sub.iso_off = k.iso_off.data();
      if (const int rc = sb::fit_plan(who, sub, true, false, &k.fit); rc != SBGPU_OK) return rc;
      k.L = sb::gdiff_chunk_layout(S, (int64_t)k.tiles.size(), (int64_t)k.items.size(), (int64_t)k.list.size(),
                                   sh.kept_off[(size_t)k.l1] - sh.kept_off[(size_t)k.l0], n_sub, sub.n_rows, sub.n_iso, k.f_off.back(), k.fit.L.bytes);
      chunk_bytes = std::max(chunk_bytes, k.L.bytes);
   }
   // ---- the arena (stage_host.h: gdiff_layout): the call's results, then one chunk's working set
   const sb::GdiffLayout L = sb::gdiff_layout(S, nl, n_iso, (int64_t)sh.kept_col.size(), chunk_bytes);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchGdiff, L.bytes, &d); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   std::vector<sb::GdiffSample> table((size_t)S);
   for (int x = 0; x < S; ++x) table[(size_t)x] = {ps[(size_t)x].d_row_off, ps[(size_t)x].d_f_off, d_count[x], d_F[x]};
   sb::HostBlock host(L.upload_bytes);
   host.put(L.lstat, sh.status.data(), sh.status.size()), host.put(L.p_a, sh.p_a.data(), sh.p_a.size()), host.put(L.p_b, sh.p_b.data(), sh.p_b.size());
   host.put(L.rank, sh.rank.data(), sh.rank.size()), host.put(L.koff, sh.kept_off.data(), sh.kept_off.size());
   host.put(L.kcol, sh.kept_col.data(), sh.kept_col.size()), host.put(L.slot, sh.slot_sub.data(), sh.slot_sub.size());
   host.put(L.table, table.data(), table.size());
   SB_STAGE_TRY(host.upload(d, s));
   const auto u = [](size_t at) { return (uint32_t)(at / 256); }; // (Arena::take's grain: every offset is a multiple of it)
   const sb::GdiffSample *d_table = sb::arena_at<sb::GdiffSample>(d, L.table);
   sb::GdiffStatArgs st;
   st.n_loci = nl, st.n_iso = n_iso, st.S = S, st.n_a = n_a, st.iso_off = ps[0].d_iso_off, st.table = d_table, st.res = d;
   sb::GdiffStatOff &so = st.o;
   so.pre_status = u(L.lstat), so.p_a = u(L.p_a), so.p_b = u(L.p_b), so.rank = u(L.rank), so.kept_off = u(L.koff), so.kept_col = u(L.kcol), so.slot = u(L.slot);
   so.theta_s = u(L.th_s), so.theta_g = u(L.th_g), so.theta_all = u(L.th_all), so.usage_s = u(L.us_s), so.usage_g = u(L.us_g), so.usage_all = u(L.us_all);
   so.delta = u(L.delta), so.lr_b = u(L.lr_b), so.lr_w = u(L.lr_w), so.ll_own = u(L.ll_own), so.ll_grp = u(L.ll_grp), so.ll_all = u(L.ll_all);
   so.n_frag = u(L.n_frag), so.lost_shift = u(L.shift), so.dof_b = u(L.dof_b), so.dof_w = u(L.dof_w), so.status = u(L.status), so.top_iso = u(L.top);
   so.st_s = u(L.st_s), so.it_s = u(L.it_s), so.st_g = u(L.st_g), so.it_g = u(L.it_g), so.st_all = u(L.st_all), so.it_all = u(L.it_all), so.sum = u(L.sum);
   sb::GdiffScaleArgs sc;
   sb::GdiffExpandArgs ex;
   sc.table = ex.table = d_table, sc.S = ex.S = S, sc.n_a = n_a;
   sc.iso_off = ex.iso_off = ps[0].d_iso_off;
   sc.kept_off = ex.kept_off = sb::arena_at<int64_t>(d, L.koff), sc.kept_col = ex.kept_col = sb::arena_at<int32_t>(d, L.kcol);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * sb::kGdiffGridPerCu;
   char *w = d + L.chunk;
   // (sbgpu_set_timing: a chunk's launches as stages of their own, as the two-sample test's are)
   sb::ctx_stage_reset(c);
   for (const GdiffChunk &k : chunks) {
      const int64_t n_sub = k.s1 - k.s0;
      PlanGuard plan;
      sb::HostBlock work(k.L.upload_bytes), lists(k.fit.L.upload_bytes), g_lists(k.fit.L.upload_bytes), a_lists(k.fit.L.upload_bytes);
      double *sub_theta = sb::arena_at<double>(w, k.L.theta), *g_theta = sb::arena_at<double>(w, k.L.g_theta), *a_theta = sb::arena_at<double>(w, k.L.a_theta);
      int32_t *sub_status = sb::arena_at<int32_t>(w, k.L.status), *sub_iters = sb::arena_at<int32_t>(w, k.L.iters);
      int32_t *g_status = sb::arena_at<int32_t>(w, k.L.g_status), *a_status = sb::arena_at<int32_t>(w, k.L.a_status);
      char *fit = w + k.L.fit, *g_fit = w + k.L.g_fit, *a_fit = w + k.L.a_fit;
      sb::PlanShape sub;
      if (n_sub) {
         if (const int rc = sbgpu_plan_create(c, n_sub, k.row_off.data(), k.iso_off.data(), k.f_off.data(), &plan.p); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sub = sb::plan_shape(plan.p);
         work.put(k.L.tiles, k.tiles.data(), k.tiles.size()), work.put(k.L.items, k.items.data(), k.items.size());
         work.put(k.L.list, k.list.data(), k.list.size()), work.put(k.L.src_g, k.src_g.data(), k.src_g.size());
         work.put(k.L.src_a, k.src_a.data(), k.src_a.size());
         SB_STAGE_TRY(work.upload(w, s));
         // ---- rule 3: the column scales
         sc.n_items = (int64_t)k.items.size(), sc.items = sb::arena_at<sb::GdiffScaleItem>(w, k.L.items), sc.list = sb::arena_at<int32_t>(w, k.L.list);
         sc.kept0 = ex.kept0 = sh.kept_off[(size_t)k.l0];
         sc.c = sb::arena_at<double>(w, k.L.c), sc.alpha_g = sb::arena_at<double>(w, k.L.alpha_g), sc.alpha_a = sb::arena_at<double>(w, k.L.alpha_a);
         ex.alpha_g = sc.alpha_g, ex.alpha_a = sc.alpha_a;
         sb::ctx_stage_begin(c, "gdiff_colscale", s);
         hipLaunchKernelGGL(sb::gdiff_colscale_kernel, dim3(sb::stage_grid(sc.n_items, cap)), dim3(sb::kGdiffThreads), 0, s, sc);
         SB_STAGE_TRY(hipGetLastError());
         sb::ctx_stage_end(c, s);
         // ---- rule 2: the expansion
         ex.n_tiles = (int64_t)k.tiles.size(), ex.tiles = sb::arena_at<sb::GdiffTile>(w, k.L.tiles), ex.n_sub = (int32_t)n_sub;
         ex.sub_row_off = sub.d_row_off, ex.sub_f_off = sub.d_f_off;
         ex.sub_count = sb::arena_at<int32_t>(w, k.L.count), ex.sub_F = sb::arena_at<double>(w, k.L.F);
         sb::ctx_stage_begin(c, "gdiff_expand", s);
         if (ex.n_tiles) {
            hipLaunchKernelGGL(sb::gdiff_expand_kernel, dim3(sb::stage_grid(ex.n_tiles, cap)), dim3(sb::kGdiffThreads), 0, s, ex);
            SB_STAGE_TRY(hipGetLastError());
         }
         sb::ctx_stage_end(c, s);
         if (out->sub_count) SB_STAGE_TRY(sb::copy_back(out->sub_count + sh.sub_row_off[(size_t)k.s0], w, k.L.count, k.row_off.back(), s));
         if (out->sub_F) SB_STAGE_TRY(sb::copy_back(out->sub_F + sh.sub_f_off[(size_t)k.s0], w, k.L.F, k.f_off.back(), s));
         // ---- rule 4: the solves; the group level's fit, ALL's, the own fit, nothing erased
         sb::ctx_stage_begin(c, "gdiff_em", s);
         if (const int rc = sbgpu_em_run_device(c, plan.p, ex.sub_count, ex.sub_F, sub_theta, sub_status, sub_iters, s); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
         sb::ctx_stage_end(c, s);
         const unsigned cross_grid = sb::stage_grid((std::max(sub.n_iso, n_sub) + sb::kGdiffThreads - 1) / sb::kGdiffThreads, sb::ctx_cu_count(c));
         sb::GdiffCrossArgs cr{n_sub, sub.d_iso_off, sub_theta, sub_status, sb::arena_at<int32_t>(w, k.L.src_g), sb::arena_at<int32_t>(w, k.L.src_a), g_theta, g_status};
         sb::ctx_stage_begin(c, "gdiff_cross_group", s);
         hipLaunchKernelGGL(sb::gdiff_cross_kernel, dim3(cross_grid), dim3(sb::kGdiffThreads), 0, s, cr, 0);
         SB_STAGE_TRY(hipGetLastError());
         sb::ctx_stage_end(c, s);
         if (const int rc = sb::fit_launch(c, sub, k.fit, g_lists, g_fit, ex.sub_count, ex.sub_F, g_theta, nullptr, g_status, s); rc != SBGPU_OK) return rc;
         cr.x_theta = a_theta, cr.x_status = a_status;
         sb::ctx_stage_begin(c, "gdiff_cross_all", s);
         hipLaunchKernelGGL(sb::gdiff_cross_kernel, dim3(cross_grid), dim3(sb::kGdiffThreads), 0, s, cr, 1);
         SB_STAGE_TRY(hipGetLastError());
         sb::ctx_stage_end(c, s);
         if (const int rc = sb::fit_launch(c, sub, k.fit, a_lists, a_fit, ex.sub_count, ex.sub_F, a_theta, nullptr, a_status, s); rc != SBGPU_OK) return rc;
         if (const int rc = sb::fit_launch(c, sub, k.fit, lists, fit, ex.sub_count, ex.sub_F, sub_theta, nullptr, sub_status, s); rc != SBGPU_OK) return rc;
      }
      // ---- the statistics of the chunk's loci (a locus without sub-problems gets its zeros here)
      st.l0 = k.l0, st.l1 = k.l1, st.sub0 = k.s0;
      st.sub_iso_off = sub.d_iso_off, st.sub_theta = sub_theta, st.sub_status = sub_status, st.sub_iters = sub_iters;
      st.fit = fit, st.g_fit = g_fit, st.a_fit = a_fit;
      so.fit_loglik = u(k.fit.L.ll), so.fit_n_live = u(k.fit.L.nlive), so.fit_n_dropped = u(k.fit.L.ndrop), so.fit_n_impossible = u(k.fit.L.nimp);
      const int64_t n_loci_k = k.l1 - k.l0, n_work = (ps[0].iso_off[k.l1] - ps[0].iso_off[k.l0]) * slots;
      sb::ctx_stage_begin(c, "gdiff_stat", s);
      hipLaunchKernelGGL(sb::gdiff_stat_kernel<0>, dim3((unsigned)((n_loci_k + sb::kGdiffThreads - 1) / sb::kGdiffThreads)), dim3(sb::kGdiffThreads), 0, s, st);
      SB_STAGE_TRY(hipGetLastError());
      if (n_work) {
         hipLaunchKernelGGL(sb::gdiff_stat_kernel<1>, dim3(sb::stage_grid((n_work + sb::kGdiffThreads - 1) / sb::kGdiffThreads, cap)), dim3(sb::kGdiffThreads), 0, s, st);
         SB_STAGE_TRY(hipGetLastError());
      }
      sb::ctx_stage_end(c, s);
      // the working set, the upload blocks and the plan are the next chunk's
      SB_STAGE_TRY(hipStreamSynchronize(s));
   }
   // ---- results: what the caller asked for
   const int64_t si = (int64_t)S * n_iso, sl = (int64_t)S * nl;
   SB_STAGE_TRY(sb::copy_back(out->theta_sample, d, L.th_s, si, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_group, d, L.th_g, 2 * n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->theta_all, d, L.th_all, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_sample, d, L.us_s, si, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_group, d, L.us_g, 2 * n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->usage_all, d, L.us_all, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->delta_usage, d, L.delta, n_iso, s));
   SB_STAGE_TRY(sb::copy_back(out->lr_between, d, L.lr_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->lr_within, d, L.lr_w, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_own, d, L.ll_own, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_group, d, L.ll_grp, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->loglik_all, d, L.ll_all, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->n_frag, d, L.n_frag, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->lost_shift, d, L.shift, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->dof_between, d, L.dof_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->dof_within, d, L.dof_w, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->p_a, d, L.p_a, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->p_b, d, L.p_b, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->gdiff_status, d, L.status, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->top_iso, d, L.top, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_sample, d, L.st_s, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_sample, d, L.it_s, sl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_group, d, L.st_g, 2 * nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_group, d, L.it_g, 2 * nl, s));
   SB_STAGE_TRY(sb::copy_back(out->status_all, d, L.st_all, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->iters_all, d, L.it_all, nl, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->d_theta_sample = sb::arena_at<double>(d, L.th_s), out->d_theta_group = sb::arena_at<double>(d, L.th_g), out->d_theta_all = sb::arena_at<double>(d, L.th_all);
   out->d_usage_sample = sb::arena_at<double>(d, L.us_s), out->d_usage_group = sb::arena_at<double>(d, L.us_g), out->d_usage_all = sb::arena_at<double>(d, L.us_all);
   out->d_delta_usage = sb::arena_at<double>(d, L.delta), out->d_lr_between = sb::arena_at<double>(d, L.lr_b), out->d_lr_within = sb::arena_at<double>(d, L.lr_w);
   out->d_loglik_own = sb::arena_at<double>(d, L.ll_own), out->d_loglik_group = sb::arena_at<double>(d, L.ll_grp), out->d_loglik_all = sb::arena_at<double>(d, L.ll_all);
   out->d_n_frag = sb::arena_at<int64_t>(d, L.n_frag), out->d_lost_shift = sb::arena_at<int64_t>(d, L.shift);
   out->d_dof_between = sb::arena_at<int32_t>(d, L.dof_b), out->d_dof_within = sb::arena_at<int32_t>(d, L.dof_w);
   out->d_p_a = sb::arena_at<int32_t>(d, L.p_a), out->d_p_b = sb::arena_at<int32_t>(d, L.p_b);
   out->d_gdiff_status = sb::arena_at<int32_t>(d, L.status), out->d_top_iso = sb::arena_at<int32_t>(d, L.top);
   out->d_status_sample = sb::arena_at<int32_t>(d, L.st_s), out->d_iters_sample = sb::arena_at<int32_t>(d, L.it_s);
   out->d_status_group = sb::arena_at<int32_t>(d, L.st_g), out->d_iters_group = sb::arena_at<int32_t>(d, L.it_g);
   out->d_status_all = sb::arena_at<int32_t>(d, L.st_all), out->d_iters_all = sb::arena_at<int32_t>(d, L.it_all);
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_em_gdiff_limits(int64_t out[9])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_em_gdiff_limits: null argument");
   const int64_t v[9] = {sb::kDiffMaxKept,      sb::kDiffMaxPooledBins, sb::kGdiffTileVals,      sb::kGdiffTileRows,      sb::kGdiffGroupMaxKept,
                         sb::kGdiffThreads,      sb::kGdiffGridPerCu,     sb::kGdiffDefaultBytes,  sb::kGdiffMaxSamples};
   std::copy(v, v + 9, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_gdiff_device(sbgpu_ctx_t *c, int32_t n_a, int32_t n_b, const sbgpu_plan_t *const *plans, const int32_t *const *d_count,
                                     const double *const *d_F, const int32_t *const *d_keep, const sbgpu_gdiff_params_t *params, void *stream,
                                     sbgpu_em_gdiff_t *out)
{
   const std::string who = "sbgpu_em_gdiff_device";
   if (!c || !plans || !d_count || !d_F || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   gdiff_clear_device(out);
   if (const int rc = check_groups(who, n_a, n_b); rc != SBGPU_OK) return rc;
   std::vector<sb::PlanShape> ps((size_t)(n_a + n_b));
   for (int x = 0; x < n_a + n_b; ++x) {
      if (!plans[x]) return api_fail(SBGPU_EINVAL, who + ": null argument");
      ps[(size_t)x] = sb::plan_shape(plans[x]);
   }
   return gdiff_run(who, c, n_a, n_b, ps, d_count, d_F, d_keep, params, stream, out);
}

extern "C" int sbgpu_model_gdiff_device(int32_t n_a, int32_t n_b, sbgpu_ctx_t *const *ctxs, const sbgpu_bins_t *const *bins, const int32_t *const *d_keep,
                                        const sbgpu_gdiff_params_t *params, void *stream, sbgpu_em_gdiff_t *out)
{
   const std::string who = "sbgpu_model_gdiff_device";
   if (!ctxs || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   gdiff_clear_device(out);
   if (const int rc = check_groups(who, n_a, n_b); rc != SBGPU_OK) return rc;
   const int S = n_a + n_b;
   for (int x = 0; x < S; ++x)
      if (!ctxs[x] || !bins[x]) return api_fail(SBGPU_EINVAL, who + ": null argument");
   for (int x = 1; x < S; ++x)
      if (sb::ctx_device(ctxs[x]) != sb::ctx_device(ctxs[0])) return api_fail(SBGPU_EINVAL, who + ": the contexts are on different devices");
   std::vector<sb::PlanShape> ps((size_t)S);
   std::vector<const int32_t *> d_count((size_t)S);
   std::vector<const double *> d_F((size_t)S);
   for (int x = 0; x < S; ++x) {
      const sb::BootKeep *rec = sb::ctx_boot_keep(ctxs[x]);
      if (const int rc = sb::check_boot_keep(who, rec, sb::bins_context_view(bins[x]), true, &ps[(size_t)x]); rc != SBGPU_OK) return rc;
      d_count[(size_t)x] = rec->d_count, d_F[(size_t)x] = rec->d_F;
   }
   // the other samples' arrays were written on their contexts' streams: they are read on the first's (or the caller's) from here on
   for (int x = 1; x < S; ++x) {
      bool seen = ctxs[x] == ctxs[0];
      for (int y = 1; y < x; ++y) seen |= ctxs[y] == ctxs[x];
      if (seen) continue;
      if (hipError_t e = hipSetDevice(sb::ctx_device(ctxs[x])); e != hipSuccess) return sb::api_fail_hip(e, "hipSetDevice");
      if (hipError_t e = hipStreamSynchronize(sb::ctx_stream(ctxs[x])); e != hipSuccess) return sb::api_fail_hip(e, "hipStreamSynchronize");
   }
   return gdiff_run(who, ctxs[0], n_a, n_b, ps, d_count.data(), d_F.data(), d_keep, params, stream, out);
}
