// strawberry_amd/csrc/context_api.hip -- sbgpu_context_table_keep / sbgpu_context_table_device (include/sbgpu.h): the
// `-f` fragment-context table built where a resident call left its results (context_device.h).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "context_device.h"
#include "stage_common.h"

using sb::api_fail;

extern "C" {

int sbgpu_context_table_keep(sbgpu_ctx_t *c, int32_t on)
{
   if (!c) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_keep: null context");
   sb::ContextKeep *k = sb::ctx_context_keep(c);
   k->on = on != 0; // (what the last call kept stays valid until the context's next sbgpu_quantify_* call either way)
   return SBGPU_OK;
}

int sbgpu_context_table_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, void *stream, sbgpu_context_table_t *out)
{
   const std::string who = "sbgpu_context_table_device";
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   if (const int rc = sb::check_context_keep(who, k, v, false); rc != SBGPU_OK) return rc;
   const int64_t nl = v.n_loci, n_bins = v.n_bins, n_elem = v.n_elem;
   if (n_bins && (!v.d_key || !k->d_hit_bin_local || !k->d_compat)) return api_fail(SBGPU_EINVAL, who + ": the handle's bins are not on the device");
   out->n_rows = 0;
   out->d_locus_row_off = nullptr, out->d_locus_hits = nullptr, out->d_row_bin = nullptr, out->d_row_hits = nullptr, out->d_row_prob = nullptr;
   if (const int rc = sb::check_locus_limits(who, v, ": a locus of more bins than the LDS table holds", nullptr); rc != SBGPU_OK) return rc;
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_STAGE_TRY(hipSetDevice(sb::ctx_device(c)));
   // ---- the count pass' work items (a locus without bins has none), and the arena (stage_host.h: ctx_layout)
   const std::vector<sb::HitItem> items = sb::build_hit_items(k->locus_hit_off.data(), nl, v.row_off);
   const int64_t n_items = (int64_t)items.size();
   const sb::CtxLayout L = sb::ctx_layout(nl, n_bins, n_elem, n_items);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, sb::kScratchContextTable, L.bytes, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   const size_t nl1 = (size_t)nl + 1, nb1 = sb::at_least_1(n_bins);
   sb::HostBlock host(L.upload_bytes);
   host.put(L.hoff, k->locus_hit_off.data(), nl1), host.put(L.roff, v.row_off, nl1), host.put(L.ioff, v.iso_off, nl1), host.put(L.foff, v.f_off, nl1);
   host.put(L.items, items.data(), items.size());
   SB_STAGE_TRY(host.upload(d, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.nin, 0, nb1 * 4, s));
   SB_STAGE_TRY(hipMemsetAsync(d + L.last, 0xff, nb1 * 4, s));
   sb::CtxArgs a;
   a.n_loci = nl, a.n_items = n_items;
   a.compat_words = k->compat_words, a.key_words = v.key_words;
   a.items = sb::arena_at<sb::HitItem>(d, L.items);
   a.locus_hit_off = sb::arena_at<int64_t>(d, L.hoff), a.row_off = sb::arena_at<int64_t>(d, L.roff);
   a.iso_off = sb::arena_at<int64_t>(d, L.ioff), a.f_off = sb::arena_at<int64_t>(d, L.foff);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.bin_key = v.d_key, a.F = k->d_F;
   a.n_in_bin = sb::arena_at<uint32_t>(d, L.nin), a.last_hit = sb::arena_at<int32_t>(d, L.last);
   a.n_rows = sb::arena_at<int32_t>(d, L.nrows), a.locus_row_off = sb::arena_at<int64_t>(d, L.lroff), a.locus_hits = sb::arena_at<uint32_t>(d, L.lhits);
   a.row_bin = sb::arena_at<int64_t>(d, L.rbin), a.row_hits = sb::arena_at<uint32_t>(d, L.rhits), a.row_last = sb::arena_at<int64_t>(d, L.rlast);
   a.row_prob = sb::arena_at<double>(d, L.prob);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   if (n_items) {
      hipLaunchKernelGGL(sb::ctx_count_kernel, dim3(sb::stage_grid(n_items, cap)), dim3(sb::kCtxThreads), 0, s, a);
      SB_STAGE_TRY(hipGetLastError());
   }
   hipLaunchKernelGGL(sb::ctx_rows_kernel, dim3(sb::stage_grid((nl + 3) / 4, cap)), dim3(sb::kCtxThreads), 0, s, a);
   hipLaunchKernelGGL(sb::ctx_scan_kernel, dim3(1), dim3(sb::kCtxScanThreads), 0, s, a, sb::arena_at<int64_t>(d, L.lroff), sb::arena_at<int64_t>(d, L.tot));
   SB_STAGE_TRY(hipGetLastError());
   hipLaunchKernelGGL(sb::ctx_order_kernel, dim3(sb::stage_grid(nl, cap)), dim3(sb::kCtxThreads), 0, s, a);
   hipLaunchKernelGGL(sb::ctx_gather_kernel, dim3(sb::stage_grid(nl, cap)), dim3(sb::kCtxThreads), 0, s, a);
   SB_STAGE_TRY(hipGetLastError());
   // ---- results: the row count first (it sizes the per-row copies), then what the caller asked for
   int64_t n_rows = 0;
   SB_STAGE_TRY(hipMemcpyAsync(&n_rows, d + L.tot, 8, hipMemcpyDeviceToHost, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   if (n_rows < 0 || n_rows > n_bins) return api_fail(SBGPU_EHIP, who + ": the row count is out of range");
   SB_STAGE_TRY(sb::copy_back(out->locus_row_off, d, L.lroff, nl + 1, s));
   SB_STAGE_TRY(sb::copy_back(out->locus_hits, d, L.lhits, nl, s));
   SB_STAGE_TRY(sb::copy_back(out->row_bin, d, L.rbin, n_rows, s));
   SB_STAGE_TRY(sb::copy_back(out->row_hits, d, L.rhits, n_rows, s));
   SB_STAGE_TRY(sb::copy_back(out->row_prob, d, L.prob, n_elem, s));
   SB_STAGE_TRY(hipStreamSynchronize(s));
   out->n_rows = n_rows;
   out->d_locus_row_off = a.locus_row_off, out->d_locus_hits = a.locus_hits;
   out->d_row_bin = a.row_bin, out->d_row_hits = a.row_hits, out->d_row_prob = a.row_prob;
   return SBGPU_OK;
}

} // extern "C"
