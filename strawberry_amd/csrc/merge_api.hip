// strawberry_amd/csrc/merge_api.hip -- sbgpu_bins_merge_device, sbgpu_bins_merge_fetch, sbgpu_bins_merge_limits,
// sbgpu_model_diff_merged_device (include/sbgpu.h): two samples' bin tables merged by key in HBM (merge_device.h),
// and the differential usage of two retained samples on the merged table.  The match works in a block of its own from the
// pool; its per-locus B-only counts come back once; the union's offsets are made on the host by the function the host form
// calls (merge_rules.h: merge_offsets); the fill writes into the context's scratch slot kScratchMerge, which outlives the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "merge_device.h"
#include "stage_common.h"

using sb::api_fail;

namespace {

// a block from the pool for the length of a call (dev_give waits for the device)
struct PoolBlock {
   char *d = nullptr;
   size_t cap = 0;
   hipError_t take(size_t bytes) { return sb::dev_take(bytes, &d, &cap); }
   ~PoolBlock()
   {
      if (d) sb::dev_give(d, cap);
   }
   PoolBlock() = default;
   PoolBlock(const PoolBlock &) = delete;
   PoolBlock &operator=(const PoolBlock &) = delete;
};
struct PlanGuard {
   sbgpu_plan_t *p = nullptr;
   ~PlanGuard() { sbgpu_plan_destroy(p); }
};

// (as diff_api.hip clears it: a refusal leaves no device pointer of an earlier call in the caller's struct)
void diff_out_clear(sbgpu_em_diff_t *out)
{
   out->d_theta_a = out->d_theta_b = out->d_theta_pooled = out->d_usage_a = out->d_usage_b = out->d_usage_pooled = out->d_delta_usage = nullptr;
   out->d_lr_stat = out->d_loglik_a = out->d_loglik_b = out->d_loglik_a_pooled = out->d_loglik_b_pooled = nullptr;
   out->d_n_a = out->d_n_b = out->d_lost_shift = nullptr;
   out->d_dof = out->d_diff_status = out->d_top_iso = out->d_status_a = out->d_status_b = out->d_status_pooled = nullptr;
   out->d_iters_a = out->d_iters_b = out->d_iters_pooled = nullptr;
}

void merged_clear(sbgpu_bins_merged_t *out)
{
   out->n_bins = out->n_elem = 0;
   out->d_row_a = out->d_row_b = out->d_count_a = out->d_count_b = nullptr;
   out->d_F_a = out->d_F_b = nullptr;
}

// the small form's work: consecutive small loci share a workgroup while their groups of lanes (the widest decides) fit its threads
void small_items(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, std::vector<int32_t> *small, std::vector<sb::MergeItem> *items,
                 std::vector<int32_t> *deep)
{
   for (int64_t l = 0; l < a->n_loci; ++l) {
      const int64_t na = a->row_off[l + 1] - a->row_off[l], nb = b->row_off[l + 1] - b->row_off[l];
      if (na + nb == 0) continue; // (n_only is zeroed on the host for these)
      if (!sb::merge_is_small(na, nb)) {
         deep->push_back((int32_t)l);
         continue;
      }
      const int lanes = sb::merge_group_lanes(na, nb);
      const int32_t at = (int32_t)small->size();
      small->push_back((int32_t)l);
      if (!items->empty()) {
         sb::MergeItem &it = items->back();
         const int wider = std::max(it.lanes, lanes);
         if ((it.n + 1) * wider <= sb::kMergeThreads) {
            it.n += 1, it.lanes = wider;
            continue;
         }
      }
      items->push_back({at, 1, lanes, 0});
   }
}

// the merge of two samples whose key, count, F and X are on c's device; `reset`: the call's stages begin a new listing
int merge_run(const std::string &who, sbgpu_ctx_t *c, const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, hipStream_t s, bool reset,
              sbgpu_bins_merged_t *out)
{
   const char *why = nullptr;
   if (const int rc = sb::merge_check_shapes(a, b, &why); rc != 0) return api_fail(rc, who + ": " + why);
   const int64_t nl = a->n_loci;
   const int kw = a->key_words;
   const std::vector<int64_t> f_off_a = sb::merge_f_off(nl, a->row_off, a->iso_off), f_off_b = sb::merge_f_off(nl, b->row_off, a->iso_off);
   const int64_t nba = a->row_off[nl], nbb = b->row_off[nl];
   if ((nba && !a->count) || (nbb && !b->count)) return api_fail(SBGPU_EINVAL, who + ": the counts are not on the device");
   if ((f_off_a[(size_t)nl] && !a->F) || (f_off_b[(size_t)nl] && !b->F)) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the match, in a block of its own
   std::vector<int32_t> small, deep;
   std::vector<sb::MergeItem> items;
   small_items(a, b, &small, &items, &deep);
   const sb::MergeMatchLayout M = sb::merge_match_layout(nl, nba, nbb, small.size(), items.size(), deep.size());
   PoolBlock mb;
   if (hipError_t e = mb.take(M.bytes); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   char *m = mb.d;
   sb::HostBlock up(M.upload_bytes);
   up.put(M.roff_a, a->row_off, (size_t)nl + 1), up.put(M.roff_b, b->row_off, (size_t)nl + 1), up.put(M.ioff, a->iso_off, (size_t)nl + 1);
   up.put(M.foff_a, f_off_a.data(), f_off_a.size()), up.put(M.foff_b, f_off_b.data(), f_off_b.size());
   up.put(M.small, small.data(), small.size()), up.put(M.items, items.data(), items.size()), up.put(M.deep, deep.data(), deep.size());
   SB_STAGE_TRY(up.upload(m, s));
   // (a locus without bins in either sample is in neither list: its count is this zero)
   SB_STAGE_TRY(hipMemsetAsync(m + M.n_only, 0, ((size_t)nl + 1) * 4, s));
   sb::MergeMatchArgs ma;
   ma.row_off[0] = sb::arena_at<int64_t>(m, M.roff_a), ma.row_off[1] = sb::arena_at<int64_t>(m, M.roff_b);
   ma.key[0] = a->key, ma.key[1] = b->key, ma.key_words = kw;
   ma.b_of_a = sb::arena_at<int32_t>(m, M.b_of_a), ma.b_only = sb::arena_at<int32_t>(m, M.b_only), ma.n_only = sb::arena_at<int32_t>(m, M.n_only);
   const int64_t cus = sb::ctx_cu_count(c);
   if (reset) sb::ctx_stage_reset(c);
   sb::ctx_stage_begin(c, "merge_match", s);
   if (!items.empty()) {
      ma.n_items = (int64_t)items.size(), ma.items = sb::arena_at<sb::MergeItem>(m, M.items), ma.list = sb::arena_at<int32_t>(m, M.small);
      hipLaunchKernelGGL(sb::merge_match_small_kernel, dim3(sb::stage_grid(ma.n_items, cus * sb::kMergeGridPerCu)), dim3(sb::kMergeThreads), 0, s, ma);
      SB_STAGE_TRY(hipGetLastError());
   }
   if (!deep.empty()) {
      ma.n_items = (int64_t)deep.size(), ma.items = nullptr, ma.list = sb::arena_at<int32_t>(m, M.deep);
      hipLaunchKernelGGL(sb::merge_match_deep_kernel, dim3(sb::stage_grid(ma.n_items, cus * sb::kMergeDeepPerCu)), dim3(sb::kMergeThreads), 0, s, ma);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // ---- the one read-back: the B-only counts (-1: a duplicate key)
   std::vector<int32_t> n_only((size_t)nl + 1, 0);
   SB_STAGE_TRY(hipMemcpyAsync(n_only.data(), m + M.n_only, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   for (int64_t l = 0; l < nl; ++l)
      if (n_only[(size_t)l] < 0) return api_fail(SBGPU_EINVAL, who + ": a duplicate bin key in locus " + std::to_string(l));
   std::vector<int64_t> row_off_u, f_off_u;
   const int64_t too_deep = sb::merge_offsets(nl, a->row_off, a->iso_off, n_only.data(), &row_off_u, &f_off_u);
   if (too_deep >= 0) return api_fail(SBGPU_ESHAPE, who + ": the union of locus " + std::to_string(too_deep) + " has more than 5632 bins");
   const int64_t nbu = row_off_u[(size_t)nl], neu = f_off_u[(size_t)nl];
   if (nbu > INT32_MAX) return api_fail(SBGPU_ESHAPE, who + ": more than 2^31 - 1 bins in the union");
   // ---- the fill, into the slot that outlives the call
   std::vector<sb::MergeTile> tiles;
   for (int64_t l = 0; l < nl; ++l) {
      const int nu = (int)(row_off_u[(size_t)l + 1] - row_off_u[(size_t)l]);
      const int step = sb::merge_tile_rows((int)(a->iso_off[l + 1] - a->iso_off[l]));
      for (int r = 0; r < nu; r += step) tiles.push_back({(int32_t)l, r, std::min(step, nu - r), 0});
   }
   const sb::MergeLayout L = sb::merge_layout(nl, nbu, neu, tiles.size());
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchMerge, L.bytes, &d); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   sb::HostBlock up2(L.upload_bytes);
   up2.put(L.roff_u, row_off_u.data(), row_off_u.size()), up2.put(L.foff_u, f_off_u.data(), f_off_u.size()), up2.put(L.tiles, tiles.data(), tiles.size());
   SB_STAGE_TRY(up2.upload(d, s));
   sb::MergeFillArgs fa;
   fa.n_tiles = (int64_t)tiles.size(), fa.tiles = sb::arena_at<sb::MergeTile>(d, L.tiles);
   fa.row_off[0] = ma.row_off[0], fa.row_off[1] = ma.row_off[1];
   fa.f_off[0] = sb::arena_at<int64_t>(m, M.foff_a), fa.f_off[1] = sb::arena_at<int64_t>(m, M.foff_b);
   fa.iso_off = sb::arena_at<int64_t>(m, M.ioff), fa.row_off_u = sb::arena_at<int64_t>(d, L.roff_u), fa.f_off_u = sb::arena_at<int64_t>(d, L.foff_u);
   fa.b_of_a = ma.b_of_a, fa.b_only = ma.b_only;
   fa.count[0] = a->count, fa.count[1] = b->count, fa.F[0] = a->F, fa.F[1] = b->F, fa.X[0] = a->X, fa.X[1] = b->X;
   fa.row[0] = sb::arena_at<int32_t>(d, L.row_a), fa.row[1] = sb::arena_at<int32_t>(d, L.row_b);
   fa.count_u[0] = sb::arena_at<int32_t>(d, L.count_a), fa.count_u[1] = sb::arena_at<int32_t>(d, L.count_b);
   fa.F_u[0] = sb::arena_at<double>(d, L.F_a), fa.F_u[1] = sb::arena_at<double>(d, L.F_b);
   sb::ctx_stage_begin(c, "merge_fill", s);
   if (fa.n_tiles) {
      hipLaunchKernelGGL(sb::merge_fill_kernel, dim3(sb::stage_grid(fa.n_tiles, cus * sb::kMergeGridPerCu)), dim3(sb::kMergeThreads), 0, s, fa);
      SB_STAGE_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->n_bins = nbu, out->n_elem = neu;
   if (out->row_off) std::copy(row_off_u.begin(), row_off_u.end(), out->row_off);
   if (out->f_off) std::copy(f_off_u.begin(), f_off_u.end(), out->f_off);
   out->d_row_a = fa.row[0], out->d_row_b = fa.row[1], out->d_count_a = fa.count_u[0], out->d_count_b = fa.count_u[1];
   out->d_F_a = fa.F_u[0], out->d_F_b = fa.F_u[1];
   return SBGPU_OK;
}

// sample x of the retained entry: its record and handle checked, its arrays named
struct Retained {
   const sb::BootKeep *rec = nullptr;
   sb::BinsContextView v;
   const sb::DevicePairs *pairs = nullptr;
   sb::PlanShape ps;
};
int retained_sample(const std::string &who, sbgpu_ctx_t *c, const sbgpu_bins_t *bins, Retained *r)
{
   r->rec = sb::ctx_boot_keep(c);
   r->v = sb::bins_context_view(bins);
   r->pairs = sb::bins_device_pairs(bins);
   // (first: a handle whose bins were grouped on the host is told so, whatever else it lacks)
   if (r->v.n_bins && (!r->v.d_key || !r->pairs))
      return api_fail(SBGPU_EUNSUPPORTED, who + ": the handle's bin keys or (bin, isoform) pairs are not on the device (its bins were grouped on the host)");
   if (const int rc = sb::check_boot_keep(who, r->rec, r->v, true, &r->ps); rc != SBGPU_OK) return rc;
   if (!r->pairs) return api_fail(SBGPU_EUNSUPPORTED, who + ": the handle's (bin, isoform) pairs are not on the device");
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_bins_merge_limits(int64_t out[8])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_bins_merge_limits: null argument");
   const int64_t v[8] = {sb::kMergeGroupMaxBins, sb::kMergeTableSlots, sb::kStageMaxBins,   sb::kMergeTileVals,
                         sb::kMergeTileRows,     sb::kMergeThreads,    sb::kMergeGridPerCu, sb::kMergeRegWords};
   std::copy(v, v + 8, out);
   return SBGPU_OK;
}

extern "C" int sbgpu_bins_merge_device(sbgpu_ctx_t *c, const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, void *stream,
                                       sbgpu_bins_merged_t *out)
{
   const std::string who = "sbgpu_bins_merge_device";
   if (!c || !a || !b || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   merged_clear(out);
   return merge_run(who, c, a, b, stream ? (hipStream_t)stream : sb::ctx_stream(c), true, out);
}

extern "C" int sbgpu_bins_merge_fetch(sbgpu_ctx_t *c, const sbgpu_bins_merged_t *m, int32_t *row_a, int32_t *row_b, int32_t *count_a,
                                      int32_t *count_b, double *F_a, double *F_b, void *stream)
{
   const std::string who = "sbgpu_bins_merge_fetch";
   if (!c || !m) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (m->n_bins < 0 || m->n_elem < 0 || (m->n_bins && (!m->d_row_a || !m->d_row_b || !m->d_count_a || !m->d_count_b)) || (m->n_elem && (!m->d_F_a || !m->d_F_b)))
      return api_fail(SBGPU_EINVAL, who + ": not the result of a merge");
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   SB_STAGE_TRY(sb::copy_back(row_a, (const char *)m->d_row_a, 0, m->n_bins, s));
   SB_STAGE_TRY(sb::copy_back(row_b, (const char *)m->d_row_b, 0, m->n_bins, s));
   SB_STAGE_TRY(sb::copy_back(count_a, (const char *)m->d_count_a, 0, m->n_bins, s));
   SB_STAGE_TRY(sb::copy_back(count_b, (const char *)m->d_count_b, 0, m->n_bins, s));
   SB_STAGE_TRY(sb::copy_back(F_a, (const char *)m->d_F_a, 0, m->n_elem, s));
   SB_STAGE_TRY(sb::copy_back(F_b, (const char *)m->d_F_b, 0, m->n_elem, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   return SBGPU_OK;
}

extern "C" int sbgpu_model_diff_merged_device(sbgpu_ctx_t *ctx_a, const sbgpu_bins_t *bins_a, sbgpu_ctx_t *ctx_b, const sbgpu_bins_t *bins_b,
                                              const int32_t *d_keep_a, const int32_t *d_keep_b, const sbgpu_diff_params_t *params, void *stream,
                                              sbgpu_em_diff_t *out, sbgpu_bins_merged_t *merged_out)
{
   const std::string who = "sbgpu_model_diff_merged_device";
   if (!ctx_a || !bins_a || !ctx_b || !bins_b || (!out && !merged_out)) return api_fail(SBGPU_EINVAL, who + ": null argument");
   sbgpu_bins_merged_t own_merged{};
   sbgpu_bins_merged_t *mo = merged_out ? merged_out : &own_merged;
   merged_clear(mo);
   if (out) diff_out_clear(out);
   if (sb::ctx_device(ctx_a) != sb::ctx_device(ctx_b)) return api_fail(SBGPU_EINVAL, who + ": the two contexts are on different devices");
   Retained r[2];
   if (const int rc = retained_sample(who, ctx_a, bins_a, &r[0]); rc != SBGPU_OK) return rc;
   if (const int rc = retained_sample(who, ctx_b, bins_b, &r[1]); rc != SBGPU_OK) return rc;
   const sbgpu_insert_t *law[2] = {&r[0].rec->insert, &r[1].rec->insert};
   for (int x = 0; x < 2; ++x)
      if (r[1 - x].pairs->any_wide && !law[x]->long_read) return api_fail(SBGPU_ESHAPE, who + ": a bin spans more than 32 isoform segments");
   const int32_t pdf_len = std::max(r[0].rec->pdf_len, r[1].rec->pdf_len);
   if (pdf_len < 1) return api_fail(SBGPU_EINVAL, who + ": neither context's record holds the length of its insert-size table");
   // the two samples' shapes, before any work is queued (merge_run checks them again: it is the batch entry's too)
   sbgpu_merge_sample_t sm[2];
   for (int x = 0; x < 2; ++x) {
      sm[x].n_loci = r[x].v.n_loci, sm[x].iso_off = r[x].v.iso_off, sm[x].row_off = r[x].v.row_off;
      sm[x].key_words = r[x].v.key_words, sm[x].reserved = 0, sm[x].key = r[x].v.d_key;
      sm[x].count = r[x].rec->d_count, sm[x].F = r[x].rec->d_F, sm[x].X = nullptr;
   }
   {
      const char *why = nullptr;
      if (const int rc = sb::merge_check_shapes(&sm[0], &sm[1], &why); rc != 0) return api_fail(rc, who + ": " + why);
   }
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(ctx_a);
   // sample B's arrays were written on ctx_b's stream: they are read on ctx_a's (or the caller's) from here on
   if (ctx_b != ctx_a) {
      if (hipError_t e = hipSetDevice(sb::ctx_device(ctx_b)); e != hipSuccess) return sb::api_fail_hip(e, "hipSetDevice");
      if (hipError_t e = hipStreamSynchronize(sb::ctx_stream(ctx_b)); e != hipSuccess) return sb::api_fail_hip(e, "hipStreamSynchronize");
   }
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(ctx_a)));
   // ---- X_s: the OTHER sample's bins under sample s' law, all of its pairs in one launch each
   sb::Arena ar;
   size_t o_pdf[2], o_X[2];
   const int64_t n_elem[2] = {r[0].v.n_elem, r[1].v.n_elem};
   for (int x = 0; x < 2; ++x) o_pdf[x] = ar.take((size_t)pdf_len * 8);
   const size_t upload_bytes = ar.size;
   for (int x = 0; x < 2; ++x) o_X[x] = ar.take(sb::at_least_1(n_elem[1 - x]) * 8);
   // (`up` outlives `xb`: the block goes back behind a wait for the device, so the upload is over before its source goes)
   sb::HostBlock up(upload_bytes);
   PoolBlock xb;
   if (hipError_t e = xb.take(ar.size); e != hipSuccess) return sb::api_fail_hip(e, "hipMalloc");
   for (int x = 0; x < 2; ++x) {
      // (a long-read call without a law built no table and its weights read none: the zeros stay)
      if (r[x].rec->insert_table)
         if (const int rc = sbgpu_insert_pdf_table(law[x], pdf_len, (double *)(up.bytes.data() + o_pdf[x])); rc != SBGPU_OK) return rc;
   }
   SB_STAGE_TRY(up.upload(xb.d, s));
   SB_STAGE_TRY(hipMemsetAsync(xb.d + o_X[0], 0, ar.size - o_X[0], s));
   sb::ctx_stage_reset(ctx_a);
   static const char *const kStage[2] = {"merge_xweights_a", "merge_xweights_b"};
   for (int x = 0; x < 2; ++x) {
      const sb::DevicePairs *p = r[1 - x].pairs;
      sb::ctx_stage_begin(ctx_a, kStage[x], s);
      if (p->n_pairs) {
         const int32_t lmin_base = law[x]->use_emp ? law[x]->start_offset : law[x]->read_len;
         if (const int rc = sbgpu_binweight_device(ctx_a, p->n_pairs, p->seg_off(), p->seg_lens(), p->mask(), p->iso_len(), p->out_index(),
                                                   (const double *)(xb.d + o_pdf[x]), pdf_len, law[x]->read_len, lmin_base, law[x]->long_read,
                                                   (double *)(xb.d + o_X[x]), s);
             rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
         }
      }
      sb::ctx_stage_end(ctx_a, s);
   }
   // ---- the merge
   for (int x = 0; x < 2; ++x) sm[x].X = (const double *)(xb.d + o_X[x]);
   const int64_t nl = sm[0].n_loci;
   std::vector<int64_t> row_off_u((size_t)std::max<int64_t>(nl, 0) + 1), f_off_u(row_off_u.size());
   int64_t *caller_row_off = mo->row_off, *caller_f_off = mo->f_off;
   mo->row_off = row_off_u.data(), mo->f_off = f_off_u.data();
   const int rc = merge_run(who, ctx_a, &sm[0], &sm[1], s, false, mo);
   mo->row_off = caller_row_off, mo->f_off = caller_f_off;
   if (rc != SBGPU_OK) return rc;
   if (caller_row_off) std::copy(row_off_u.begin(), row_off_u.end(), caller_row_off);
   if (caller_f_off) std::copy(f_off_u.begin(), f_off_u.end(), caller_f_off);
   if (!out) return SBGPU_OK;
   // ---- ONE plan over the union's offsets serves both samples; the differential rule runs on it unchanged
   PlanGuard plan;
   if (const int prc = sbgpu_plan_create(ctx_a, nl, row_off_u.data(), sm[0].iso_off, f_off_u.data(), &plan.p); prc != SBGPU_OK) return prc;
   return sbgpu_em_diff_device(ctx_a, plan.p, mo->d_count_a, mo->d_F_a, plan.p, mo->d_count_b, mo->d_F_b, d_keep_a, d_keep_b, params, s, out);
}
