// strawberry_amd/csrc/context_api.hip -- sbgpu_context_table_keep / sbgpu_context_table_device (include/sbgpu.h): the
// `-f` fragment-context table built where a resident call left its results (context_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "context_device.h"

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
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_device: null argument");
   const sb::ContextKeep *k = sb::ctx_context_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   if (!v.context_serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_context_table_device: this handle was made without retention (sbgpu_context_table_keep was off for its call, "
                                    "or it is not from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.context_serial != k->serial)
      return api_fail(SBGPU_EINVAL, "sbgpu_context_table_device: a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that "
                                    "works in the context's scratch, such as sbgpu_bins_create_device) has reused what its call kept");
   const int64_t nl = v.n_loci, n_bins = v.n_bins, n_elem = v.n_elem;
   const int32_t cw = k->compat_words, kw = v.key_words;
   if (nl != k->n_loci || v.n_iso != k->n_iso || (int64_t)k->locus_hit_off.size() != nl + 1)
      return api_fail(SBGPU_EINVAL, "sbgpu_context_table_device: the handle and the context's record disagree");
   if (n_bins && (!v.d_key || !k->d_hit_bin_local || !k->d_compat)) return api_fail(SBGPU_EINVAL, "sbgpu_context_table_device: the handle's bins are not on the device");
   out->n_rows = 0;
   out->d_locus_row_off = nullptr, out->d_locus_hits = nullptr, out->d_row_bin = nullptr, out->d_row_hits = nullptr, out->d_row_prob = nullptr;
   for (int64_t l = 0; l < nl; ++l) {
      if (v.row_off[l + 1] - v.row_off[l] > sb::kCtxMaxBins) return api_fail(SBGPU_ESHAPE, "sbgpu_context_table_device: a locus of more bins than the LDS table holds");
      if (v.iso_off[l + 1] - v.iso_off[l] > 32 * (int64_t)sb::kCtxMaxWords) return api_fail(SBGPU_ESHAPE, "sbgpu_context_table_device: a locus of more than 4096 isoforms");
   }
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
   // ---- the count pass' work items: a locus' hits in ranges of kCtxItemHits
   std::vector<sb::CtxItem> items;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t q0 = k->locus_hit_off[(size_t)l], q1 = k->locus_hit_off[(size_t)l + 1];
      if (q1 <= q0 || v.row_off[l + 1] == v.row_off[l]) continue;
      const int32_t split = q1 - q0 > sb::kCtxItemHits;
      for (int64_t h = q0; h < q1; h += sb::kCtxItemHits) items.push_back({h, std::min<int64_t>(h + sb::kCtxItemHits, q1), (int32_t)l, split});
   }
   const int64_t n_items = (int64_t)items.size();
   // ---- one arena: [uploads: the four offset arrays, the items | per-bin scratch | per-locus results | rows]
   auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
   const size_t nl1 = (size_t)nl + 1, nb1 = (size_t)std::max<int64_t>(n_bins, 1), ne1 = (size_t)std::max<int64_t>(n_elem, 1);
   size_t off = 0;
   const size_t o_hoff = off; off += up(nl1 * 8);
   const size_t o_roff = off; off += up(nl1 * 8);
   const size_t o_ioff = off; off += up(nl1 * 8);
   const size_t o_foff = off; off += up(nl1 * 8);
   const size_t o_items = off; off += up((size_t)std::max<int64_t>(n_items, 1) * sizeof(sb::CtxItem));
   const size_t upload_bytes = off;
   const size_t o_nin = off; off += up(nb1 * 4);
   const size_t o_last = off; off += up(nb1 * 4);
   const size_t o_nrows = off; off += up(nl1 * 4);
   const size_t o_lhits = off; off += up(nl1 * 4);
   const size_t o_lroff = off; off += up(nl1 * 8);
   const size_t o_tot = off; off += 256;
   const size_t o_rbin = off; off += up(nb1 * 8);
   const size_t o_rhits = off; off += up(nb1 * 4);
   const size_t o_rlast = off; off += up(nb1 * 8);
   const size_t o_prob = off; off += up(ne1 * 8);
   char *d = nullptr;
   if (hipError_t e = sb::ctx_scratch(c, 8, off, &d); e != hipSuccess)
      return sb::api_fail_hip(e, "hipMalloc");
   // (one host block for the uploads: it lives until the call's last synchronisation; SB_TRY synchronises before it leaves early)
   std::vector<char> host(upload_bytes, 0);
   std::memcpy(host.data() + o_hoff, k->locus_hit_off.data(), nl1 * 8);
   std::memcpy(host.data() + o_roff, v.row_off, nl1 * 8);
   std::memcpy(host.data() + o_ioff, v.iso_off, nl1 * 8);
   std::memcpy(host.data() + o_foff, v.f_off, nl1 * 8);
   if (n_items) std::memcpy(host.data() + o_items, items.data(), (size_t)n_items * sizeof(sb::CtxItem));
   SB_TRY(hipMemcpyAsync(d, host.data(), upload_bytes, hipMemcpyHostToDevice, s));
   SB_TRY(hipMemsetAsync(d + o_nin, 0, nb1 * 4, s));
   SB_TRY(hipMemsetAsync(d + o_last, 0xff, nb1 * 4, s));
   sb::CtxArgs a;
   a.n_loci = nl, a.n_items = n_items;
   a.compat_words = cw, a.key_words = kw;
   a.items = (const sb::CtxItem *)(d + o_items);
   a.locus_hit_off = (const int64_t *)(d + o_hoff), a.row_off = (const int64_t *)(d + o_roff);
   a.iso_off = (const int64_t *)(d + o_ioff), a.f_off = (const int64_t *)(d + o_foff);
   a.hit_bin_local = k->d_hit_bin_local, a.compat = k->d_compat;
   a.keep = k->d_keep, a.status = k->d_status;
   a.bin_key = v.d_key, a.F = k->d_F;
   a.n_in_bin = (uint32_t *)(d + o_nin), a.last_hit = (int32_t *)(d + o_last);
   a.n_rows = (int32_t *)(d + o_nrows), a.locus_row_off = (const int64_t *)(d + o_lroff), a.locus_hits = (uint32_t *)(d + o_lhits);
   a.row_bin = (int64_t *)(d + o_rbin), a.row_hits = (uint32_t *)(d + o_rhits), a.row_last = (int64_t *)(d + o_rlast);
   a.row_prob = (double *)(d + o_prob);
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8;
   if (n_items) {
      hipLaunchKernelGGL(sb::ctx_count_kernel, dim3((unsigned)std::min<int64_t>(n_items, cap)), dim3(sb::kCtxThreads), 0, s, a);
      SB_TRY(hipGetLastError());
   }
   const unsigned wgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nl + 3) / 4, cap));
   hipLaunchKernelGGL(sb::ctx_rows_kernel, dim3(wgrid), dim3(sb::kCtxThreads), 0, s, a);
   hipLaunchKernelGGL(sb::ctx_scan_kernel, dim3(1), dim3(sb::kCtxScanThreads), 0, s, a, (int64_t *)(d + o_lroff), (int64_t *)(d + o_tot));
   SB_TRY(hipGetLastError());
   const unsigned lgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nl, cap));
   hipLaunchKernelGGL(sb::ctx_order_kernel, dim3(lgrid), dim3(sb::kCtxThreads), 0, s, a);
   hipLaunchKernelGGL(sb::ctx_gather_kernel, dim3(lgrid), dim3(sb::kCtxThreads), 0, s, a);
   SB_TRY(hipGetLastError());
   // ---- results: the row count first (it sizes the per-row copies), then what the caller asked for
   int64_t n_rows = 0;
   SB_TRY(hipMemcpyAsync(&n_rows, d + o_tot, 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
   if (n_rows < 0 || n_rows > n_bins) return api_fail(SBGPU_EHIP, "sbgpu_context_table_device: the row count is out of range");
   if (out->locus_row_off) SB_TRY(hipMemcpyAsync(out->locus_row_off, d + o_lroff, nl1 * 8, hipMemcpyDeviceToHost, s));
   if (out->locus_hits) SB_TRY(hipMemcpyAsync(out->locus_hits, d + o_lhits, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
   if (out->row_bin && n_rows) SB_TRY(hipMemcpyAsync(out->row_bin, d + o_rbin, (size_t)n_rows * 8, hipMemcpyDeviceToHost, s));
   if (out->row_hits && n_rows) SB_TRY(hipMemcpyAsync(out->row_hits, d + o_rhits, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
   if (out->row_prob && n_elem) SB_TRY(hipMemcpyAsync(out->row_prob, d + o_prob, (size_t)n_elem * 8, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
#undef SB_TRY
   out->n_rows = n_rows;
   out->d_locus_row_off = (const int64_t *)(d + o_lroff), out->d_locus_hits = (const uint32_t *)(d + o_lhits);
   out->d_row_bin = (const int64_t *)(d + o_rbin), out->d_row_hits = (const uint32_t *)(d + o_rhits), out->d_row_prob = (const double *)(d + o_prob);
   return SBGPU_OK;
}

} // extern "C"
