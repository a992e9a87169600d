// strawberry_amd/csrc/gtf_api.hip -- sbgpu_gtf_read_device / sbgpu_gtf_read_upload (include/sbgpu.h): a GTF file's bytes in HBM
// -> the lines' statuses, a row per transcript, the merged exons and the names, which the host form's code (gtf_host.cpp:
// gtf_finish) turns into the annotation.  The kernels: gtf_device.h.  What the call decides -- tiles, grids, which tile is
// staged, the three arenas -- is gtf_schedule.h's; the steps below issue it.  The scaffold is the front end's (front_common.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/sbgpu.h"
#include "front_common.h"
#include "gtf_device.h"
#include "gtf_host.h"

using sb::api_fail;

namespace {

// A timing stage of the context (sbgpu_set_timing) that ends with its scope: a step that fails leaves no stage open
struct Stage {
   sbgpu_ctx_t *c;
   hipStream_t s;
   bool open = true;
   Stage(sbgpu_ctx_t *ctx, const char *name, hipStream_t stream) : c(ctx), s(stream) { sb::ctx_stage_begin(c, name, s); }
   Stage(const Stage &) = delete;
   Stage &operator=(const Stage &) = delete;
   ~Stage() { end(); }
   void end()
   {
      if (open) sb::ctx_stage_end(c, s);
      open = false;
   }
};

struct GtfDeviceCall {
   sbgpu_ctx_t *const c;
   const uint8_t *const d_bytes;
   const int64_t n_bytes;
   const sbgpu_gtf_opts_t *const opts;
   const hipStream_t s;
   sbgpu_gtf *const G;
   const std::string who = "sbgpu_gtf_read_device";

   // what comes back
   std::vector<uint8_t> status;
   sb::PodVec<sb::GtfTx> tx;
   sb::PodVec<uint32_t> xl, xr;
   sb::PodVec<uint8_t> names;

   int64_t n_lines = 0, n_ok = 0, n_tx = 0, n_names = 0;

   // ---- the line index: the tiles' '\n', their scan, the offsets.  `p` is the parse's arena (the offsets are its first array)
   int line_index(sb::DevBlock &p, sb::GtfParseLayout *P)
   {
      const sb::GtfIndexLayout L = sb::gtf_index_layout(n_bytes);
      sb::DevBlock w(s);
      SB_FRONT_TRY(w.take(L.bytes));
      Stage stage(c, "gtf_line_index", s);
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.words, 0, L.words_bytes, s));
      const unsigned grid = sb::gtf_grid((L.tiles + 3) / 4); // (four waves a workgroup, a wave per tile)
      hipLaunchKernelGGL(sb::gtf_newline_count_kernel, dim3(grid), dim3(256), 0, s, d_bytes, n_bytes, w.at<int32_t>(L.cnt), w.at<int64_t>(L.words));
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::gtf_tile_scan_kernel, dim3(1), dim3(256), 0, s, w.at<const int32_t>(L.cnt), w.at<int64_t>(L.at), L.tiles, w.at<int64_t>(L.words));
      SB_FRONT_TRY(hipGetLastError());
      int64_t words[4] = {0, 0, 0, 0};
      SB_FRONT_TRY(hipMemcpyAsync(words, w.p + L.words, sizeof(words), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      n_lines = sb::gtf_line_count(n_bytes, words[0], (int)words[1]);
      if (n_lines >= sb::kGtfMaxLines) return api_fail(SBGPU_EUNSUPPORTED, who + ": 2^31 - 2 lines or more; use the host form");
      *P = sb::gtf_parse_layout(n_lines);
      SB_FRONT_TRY(p.take(P->bytes));
      hipLaunchKernelGGL(sb::gtf_line_index_kernel, dim3(grid), dim3(256), 0, s, d_bytes, n_bytes, w.at<const int64_t>(L.at), p.at<int64_t>(P->line_off), n_lines);
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      SB_FRONT_TRY(hipStreamSynchronize(s)); // (the index' arena goes back to the pool)
      return SBGPU_OK;
   }

   // ---- the parse: a record per accepted line, the tiles' totals and their scan, the counts by status
   int parse(sb::DevBlock &p, const sb::GtfParseLayout &P)
   {
      Stage stage(c, "gtf_parse", s);
      SB_FRONT_TRY(hipMemsetAsync(p.p + P.counts, 0, P.counts_bytes, s));
      sb::GtfParseArgs a = {};
      a.bytes = d_bytes, a.n_bytes = n_bytes, a.line_off = p.at<const int64_t>(P.line_off), a.n_lines = n_lines;
      a.status = p.at<uint8_t>(P.status), a.rec = p.at<sb::GtfRec>(P.rec), a.tile_cnt = p.at<int32_t>(P.cnt);
      a.counts = p.at<unsigned long long>(P.counts);
      const unsigned grid = sb::gtf_grid(P.tiles);
      hipLaunchKernelGGL(sb::gtf_parse_kernel, dim3(grid), dim3(64), (size_t)sb::kGtfStageBytes, s, a);
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::gtf_tile_scan_kernel, dim3(1), dim3(256), 0, s, p.at<const int32_t>(P.cnt), p.at<int64_t>(P.at), P.tiles, (int64_t *)nullptr);
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      unsigned long long counts[16];
      status.resize((size_t)n_lines);
      SB_FRONT_TRY(hipMemcpyAsync(counts, p.p + P.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(&n_ok, p.p + P.at + (size_t)P.tiles * 8, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(status.data(), p.p + P.status, (size_t)n_lines, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      if (counts[sb::kGtfLineLong]) {
         return api_fail(SBGPU_EUNSUPPORTED, who + ": a line of more than " + std::to_string(sb::kGtfMaxLine) + " bytes; use the host form");
      }
      if (counts[sb::kGtfNameLong]) return api_fail(SBGPU_EUNSUPPORTED, who + ": a name of more than 255 bytes");
      if (n_ok != (int64_t)counts[sb::kGtfOk] || n_ok < 0 || n_ok > n_lines) return api_fail(SBGPU_EHIP, who + ": the parse's counts disagree (did the buffer change under the call?)");
      return SBGPU_OK;
   }

   // ---- the grouping: compact, two stable sorts, the transcripts' heads, the pass per transcript, the names
   int group(sb::DevBlock &p, const sb::GtfParseLayout &P)
   {
      const int64_t m = n_ok;
      const unsigned hash_bits = sb::gtf_hash_bits(opts ? opts->hash_bits : 0);
      size_t t1 = 0, t2 = 0, t3 = 0;
      (void)rocprim::radix_sort_pairs(nullptr, t1, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, 0, 64, s);
      (void)rocprim::radix_sort_pairs(nullptr, t2, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)m, 0, hash_bits, s);
      (void)rocprim::inclusive_scan(nullptr, t3, rocprim::make_transform_iterator((const uint8_t *)nullptr, sb::U8AsI32()), (int32_t *)nullptr, (size_t)m, rocprim::plus<int32_t>(), s);
      const size_t tmp_bytes = std::max(t1, std::max(t2, t3));
      const sb::GtfGroupLayout L = sb::gtf_group_layout(m, tmp_bytes);
      sb::DevBlock w(s);
      SB_FRONT_TRY(w.take(L.bytes));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.words, 0, L.words_bytes, s));
      const sb::GtfRec *rec = w.at<const sb::GtfRec>(L.rec);
      const int64_t *line_off = p.at<const int64_t>(P.line_off);
      Stage stage(c, "gtf_sorts", s);
      hipLaunchKernelGGL(sb::gtf_compact_kernel, dim3(sb::gtf_grid((P.tiles + 3) / 4)), dim3(256), 0, s, p.at<const uint8_t>(P.status), p.at<const sb::GtfRec>(P.rec),
                         p.at<const int64_t>(P.at), n_lines, m, w.at<sb::GtfRec>(L.rec), w.at<unsigned long long>(L.key_a), w.at<uint32_t>(L.val_a));
      SB_FRONT_TRY(hipGetLastError());
      const unsigned grid_m = sb::gtf_grid256(m);
      size_t tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::radix_sort_pairs(w.p + L.tmp, tb, w.at<const unsigned long long>(L.key_a), w.at<unsigned long long>(L.key_b), w.at<const uint32_t>(L.val_a),
                                             w.at<uint32_t>(L.val_b), (size_t)m, 0, 64, s));
      const unsigned long long mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull;
      hipLaunchKernelGGL(sb::gtf_hash_keys_kernel, dim3(grid_m), dim3(256), 0, s, rec, w.at<const uint32_t>(L.val_b), m, mask, w.at<unsigned long long>(L.key_a));
      SB_FRONT_TRY(hipGetLastError());
      tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::radix_sort_pairs(w.p + L.tmp, tb, w.at<const unsigned long long>(L.key_a), w.at<unsigned long long>(L.key_b), w.at<const uint32_t>(L.val_b),
                                             w.at<uint32_t>(L.val_a), (size_t)m, 0, hash_bits, s));
      const uint32_t *order = w.at<const uint32_t>(L.val_a);
      hipLaunchKernelGGL(sb::gtf_heads_kernel, dim3(grid_m), dim3(256), 0, s, w.at<const unsigned long long>(L.key_b), m, w.at<uint8_t>(L.head));
      SB_FRONT_TRY(hipGetLastError());
      tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::inclusive_scan(w.p + L.tmp, tb, rocprim::make_transform_iterator(w.at<const uint8_t>(L.head), sb::U8AsI32()), w.at<int32_t>(L.seg), (size_t)m,
                                           rocprim::plus<int32_t>(), s));
      hipLaunchKernelGGL(sb::gtf_first_kernel, dim3(grid_m), dim3(256), 0, s, w.at<const uint8_t>(L.head), w.at<const int32_t>(L.seg), m, w.at<uint32_t>(L.tx_first),
                         w.at<int64_t>(L.words));
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      int64_t words[4] = {0, 0, 0, 0};
      SB_FRONT_TRY(hipMemcpyAsync(words, w.p + L.words, sizeof(words), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      n_tx = words[0];
      if (n_tx < 1 || n_tx > m) return api_fail(SBGPU_EHIP, who + ": the grouping's counts disagree");
      sb::GtfMergeArgs a = {};
      a.bytes = d_bytes, a.line_off = line_off, a.rec = rec, a.order = order, a.tx_first = w.at<const uint32_t>(L.tx_first), a.n_tx = n_tx;
      a.xl = w.at<uint32_t>(L.xl), a.xr = w.at<uint32_t>(L.xr), a.tx = w.at<sb::GtfTx>(L.tx), a.name_len = w.at<int32_t>(L.name_len), a.words = w.at<int64_t>(L.words);
      const unsigned grid_t = sb::gtf_grid256(n_tx);
      Stage stage_merge(c, "gtf_merge", s);
      hipLaunchKernelGGL(sb::gtf_merge_kernel, dim3(grid_t), dim3(256), 0, s, a);
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::gtf_tile_scan_kernel, dim3(1), dim3(256), 0, s, w.at<const int32_t>(L.name_len), w.at<int64_t>(L.name_at), n_tx, w.at<int64_t>(L.words) + 1);
      SB_FRONT_TRY(hipGetLastError());
      stage_merge.end();
      SB_FRONT_TRY(hipMemcpyAsync(words, w.p + L.words, sizeof(words), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      if (words[2])
         return api_fail(SBGPU_EUNSUPPORTED, who + ": hash collision: " + std::to_string(words[2]) + " group(s) of lines with one transcript-key hash hold different keys; use the host form");
      n_names = words[1];
      if (n_names < 0 || n_names > 4 * (int64_t)sb::kGtfMaxName * n_tx) return api_fail(SBGPU_EHIP, who + ": the names' sizes disagree");
      sb::DevBlock nb(s);
      SB_FRONT_TRY(nb.take((size_t)std::max<int64_t>(n_names, 8)));
      Stage stage_back(c, "gtf_names_copy_back", s);
      hipLaunchKernelGGL(sb::gtf_names_kernel, dim3(grid_t), dim3(256), 0, s, d_bytes, line_off, rec, w.at<sb::GtfTx>(L.tx), w.at<const int64_t>(L.name_at), n_tx, n_names,
                         (uint8_t *)nb.p);
      SB_FRONT_TRY(hipGetLastError());
      tx.resize((size_t)n_tx), xl.resize((size_t)m), xr.resize((size_t)m), names.resize((size_t)n_names + 1);
      SB_FRONT_TRY(hipMemcpyAsync(tx.data(), w.p + L.tx, (size_t)n_tx * sizeof(sb::GtfTx), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(xl.data(), w.p + L.xl, (size_t)m * 4, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(xr.data(), w.p + L.xr, (size_t)m * 4, hipMemcpyDeviceToHost, s));
      if (n_names) SB_FRONT_TRY(hipMemcpyAsync(names.data(), nb.p, (size_t)n_names, hipMemcpyDeviceToHost, s));
      stage_back.end();
      SB_FRONT_TRY(hipStreamSynchronize(s));
      return SBGPU_OK;
   }

   int run()
   {
      SB_FRONT_TRY(hipSetDevice(sb::ctx_device(c)));
      sb::ctx_stage_reset(c);
      if (n_bytes > 0) {
         sb::DevBlock p(s);
         sb::GtfParseLayout P;
         SB_FRONT_RC(line_index(p, &P));
         if (n_lines > 0) {
            SB_FRONT_RC(parse(p, P));
            if (n_ok > 0) SB_FRONT_RC(group(p, P));
         }
      }
      // the transcripts as the host's step takes them
      std::vector<sb::GtfRawTx> raw;
      raw.reserve((size_t)n_tx);
      for (int64_t t = 0; t < n_tx; ++t) {
         const sb::GtfTx &x = tx[(size_t)t];
         const int64_t len = (int64_t)x.l_chrom + x.l_gene + x.l_tx + x.l_gname;
         if (x.name_at < 0 || x.name_at + len > n_names || x.n_exons < 1 || (int64_t)x.exon_at + x.n_exons > n_ok)
            return api_fail(SBGPU_EHIP, who + ": a transcript's row points outside what came back");
         sb::GtfRawTx q;
         q.first_line = x.first_line;
         q.chrom = names.data() + x.name_at, q.gene = q.chrom + x.l_chrom, q.tx = q.gene + x.l_gene, q.gname = q.tx + x.l_tx;
         q.l_chrom = x.l_chrom, q.l_gene = x.l_gene, q.l_tx = x.l_tx, q.l_gname = x.l_gname;
         q.strand = x.strand;
         q.xl = xl.data() + x.exon_at, q.xr = xr.data() + x.exon_at, q.n_exons = x.n_exons, q.merges = x.merges;
         raw.push_back(q);
      }
      return sb::gtf_finish(who, raw, std::move(status), opts, G);
   }
};

using GtfHandle = std::unique_ptr<sbgpu_gtf_t, sb::HandleDeleter<sbgpu_gtf_destroy>>;

} // namespace

extern "C" {

int sbgpu_gtf_read_device(sbgpu_ctx_t *c, const uint8_t *d_bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, void *stream, sbgpu_gtf_t **out)
{
   if (!c || !out || n_bytes < 0 || (n_bytes && !d_bytes)) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_read_device: bad argument");
   *out = nullptr;
   if (const int rc = sb::gtf_check_opts("sbgpu_gtf_read_device", opts)) return rc;
   try {
      GtfHandle G(new sbgpu_gtf());
      GtfDeviceCall call = {c, d_bytes, n_bytes, opts, stream ? (hipStream_t)stream : sb::ctx_stream(c), G.get()};
      SB_FRONT_RC(call.run());
      *out = G.release();
   } catch (const std::bad_alloc &) {
      (void)hipStreamSynchronize(stream ? (hipStream_t)stream : sb::ctx_stream(c));
      return api_fail(SBGPU_ENOMEM, "sbgpu_gtf_read_device: out of memory");
   } catch (const std::exception &e) { // (std::length_error of a container: nothing C++ crosses the C ABI)
      (void)hipStreamSynchronize(stream ? (hipStream_t)stream : sb::ctx_stream(c));
      return api_fail(SBGPU_ENOMEM, std::string("sbgpu_gtf_read_device: ") + e.what());
   }
   return SBGPU_OK;
}

int sbgpu_gtf_read_upload(sbgpu_ctx_t *c, const uint8_t *bytes, int64_t n_bytes, const sbgpu_gtf_opts_t *opts, void *stream, sbgpu_gtf_t **out)
{
   if (!c || !out || n_bytes < 0 || (n_bytes && !bytes)) return api_fail(SBGPU_EINVAL, "sbgpu_gtf_read_upload: bad argument");
   *out = nullptr;
   const hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_FRONT_TRY(hipSetDevice(sb::ctx_device(c)));
   sb::DevBlock d(s);
   SB_FRONT_TRY(d.take((size_t)std::max<int64_t>(n_bytes, 8)));
   if (n_bytes) SB_FRONT_TRY(hipMemcpyAsync(d.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
   return sbgpu_gtf_read_device(c, (const uint8_t *)d.p, n_bytes, opts, stream, out);
}

} // extern "C"
