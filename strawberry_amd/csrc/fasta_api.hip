// strawberry_amd/csrc/fasta_api.hip -- sbgpu_fasta_read_device / sbgpu_fasta_read_upload and sbgpu_binseq_fasta_* (include/sbgpu.h):
// a FASTA file's bytes in HBM -> the packed sequence, which stays there, and per contig the offsets, the first line's lengths,
// the name and the two facts behind RAGGED, which the host form's code (fasta_host.cpp: fasta_finish) turns into the handle.
// The kernels: fasta_device.h.  What the call decides -- tiles, grids, the two arenas -- is fasta_schedule.h's; the steps below
// issue it.  The scaffold is the front end's (front_common.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "fasta_device.h"
#include "fasta_host.h"
#include "front_common.h"

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

// what a handle whose sequence is in HBM carries to reach it (fasta_host.h)
void fasta_dev_free(uint8_t *d_seq, int device)
{
   int cur = 0;
   const bool had = hipGetDevice(&cur) == hipSuccess;
   if (hipSetDevice(device) == hipSuccess) (void)hipFree(d_seq); // (waits for the device, as a kernel may still read it)
   if (had) (void)hipSetDevice(cur);
}
int fasta_dev_fetch(const uint8_t *d_src, int device, uint8_t *dst, int64_t n)
{
   hipError_t e = hipSetDevice(device);
   if (e == hipSuccess) e = hipMemcpy(dst, d_src, (size_t)n, hipMemcpyDeviceToHost);
   return e == hipSuccess ? SBGPU_OK : sb::api_fail_hip(e, "sbgpu_fasta_fetch: hipMemcpy");
}

struct FastaDeviceCall {
   sbgpu_ctx_t *const c;
   const uint8_t *const d_bytes;
   const int64_t n_bytes;
   const hipStream_t s;
   sbgpu_fasta *const G;
   const std::string who = "sbgpu_fasta_read_device";

   int64_t n_lines = 0, n_contigs = 0, n_names = 0, n_bases = 0;
   std::vector<int64_t> name_off, offset, line_bases, line_width, seq_off, first_odd;
   std::vector<int32_t> ragged32;
   std::string names;

   // ---- the headers' count: per tile, scanned; the file's lines
   int count(sb::DevBlock &w, const sb::FastaTileLayout &L)
   {
      Stage stage(c, "fasta_count", s);
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.words, 0, L.words_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.words + 8 * sb::kFastaWordLeading, 0x7f, 8, s));
      const unsigned grid = sb::fasta_grid(L.tiles);
      hipLaunchKernelGGL(sb::fasta_count_kernel, dim3(grid), dim3(64), 0, s, d_bytes, n_bytes, w.at<int32_t>(L.hdr_cnt), w.at<int64_t>(L.words));
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::fasta_scan_kernel, dim3(1), dim3(256), 0, s, w.at<const int32_t>(L.hdr_cnt), w.at<int64_t>(L.hdr_at), L.tiles);
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      int64_t words[8] = {};
      SB_FRONT_TRY(hipMemcpyAsync(words, w.p + L.words, sizeof(words), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(&n_contigs, w.p + L.hdr_at + (size_t)L.tiles * 8, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      n_lines = sb::fasta_line_count(n_bytes, words[sb::kFastaWordNewlines], (int)words[sb::kFastaWordLast]);
      if (n_contigs < 0) return api_fail(SBGPU_EHIP, who + ": the headers' counts disagree");
      if (!sb::fasta_contigs_fit(n_contigs))
         return api_fail(SBGPU_EUNSUPPORTED, who + ": more than " + std::to_string(sb::kFastaMaxContigs) + " contigs; use the host form");
      return SBGPU_OK;
   }

   // ---- the headers' places, lines and names' lengths; the bases' count per tile, scanned; the first lines
   int index(sb::DevBlock &w, const sb::FastaTileLayout &L, sb::DevBlock &q, const sb::FastaContigLayout &Q, sb::FastaArgs &a)
   {
      const unsigned grid = sb::fasta_grid(L.tiles), grid_w = sb::fasta_grid_contigs(n_contigs), grid_c = sb::fasta_grid256(n_contigs);
      Stage stage(c, "fasta_headers", s);
      SB_FRONT_TRY(hipMemsetAsync(q.p + Q.mins, 0x7f, Q.mins_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(q.p + Q.ragged, 0, (size_t)std::max<int64_t>(n_contigs, 1) * 4, s));
      hipLaunchKernelGGL(sb::fasta_header_index_kernel, dim3(grid), dim3(64), 0, s, d_bytes, n_bytes, w.at<const int64_t>(L.hdr_at), q.at<int64_t>(Q.hdr_off), n_contigs);
      SB_FRONT_TRY(hipGetLastError());
      if (n_contigs) {
         hipLaunchKernelGGL(sb::fasta_header_walk_kernel, dim3(grid_w), dim3(256), 0, s, d_bytes, n_bytes, q.at<const int64_t>(Q.hdr_off), n_contigs, q.at<int64_t>(Q.offset),
                            q.at<int32_t>(Q.name_len), w.at<int64_t>(L.words));
         SB_FRONT_TRY(hipGetLastError());
      }
      hipLaunchKernelGGL(sb::fasta_scan_kernel, dim3(1), dim3(256), 0, s, q.at<const int32_t>(Q.name_len), q.at<int64_t>(Q.name_at), n_contigs);
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      Stage stage_bases(c, "fasta_base_count", s);
      a = sb::FastaArgs{};
      a.bytes = d_bytes, a.n_bytes = n_bytes, a.hdr_at = w.at<const int64_t>(L.hdr_at), a.hdr_off = q.at<const int64_t>(Q.hdr_off), a.offset = q.at<const int64_t>(Q.offset);
      a.n_contigs = n_contigs, a.base_cnt = w.at<int32_t>(L.base_cnt), a.first_nl = q.at<int64_t>(Q.first_nl), a.words = w.at<int64_t>(L.words);
      a.base_at = w.at<const int64_t>(L.base_at), a.line_bases = q.at<const int64_t>(Q.line_bases), a.line_width = q.at<const int64_t>(Q.line_width);
      a.seq_off = q.at<int64_t>(Q.seq_off), a.first_odd = q.at<int64_t>(Q.first_odd), a.ragged = q.at<int32_t>(Q.ragged);
      hipLaunchKernelGGL(sb::fasta_base_count_kernel, dim3(grid), dim3(64), 0, s, a);
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::fasta_scan_kernel, dim3(1), dim3(256), 0, s, w.at<const int32_t>(L.base_cnt), w.at<int64_t>(L.base_at), L.tiles);
      SB_FRONT_TRY(hipGetLastError());
      if (n_contigs) {
         hipLaunchKernelGGL(sb::fasta_first_line_kernel, dim3(grid_c), dim3(256), 0, s, d_bytes, n_bytes, q.at<const int64_t>(Q.hdr_off), q.at<const int64_t>(Q.offset),
                            q.at<const int64_t>(Q.first_nl), n_contigs, q.at<int64_t>(Q.line_bases), q.at<int64_t>(Q.line_width));
         SB_FRONT_TRY(hipGetLastError());
      }
      stage_bases.end();
      int64_t words[8] = {};
      SB_FRONT_TRY(hipMemcpyAsync(words, w.p + L.words, sizeof(words), hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(&n_names, q.p + Q.name_at + (size_t)n_contigs * 8, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(&n_bases, w.p + L.base_at + (size_t)L.tiles * 8, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      if (words[sb::kFastaWordLeading] != sb::kFastaNone) return sb::fasta_fail_leading(who, words[sb::kFastaWordLeading]);
      if (words[sb::kFastaWordLong])
         return api_fail(SBGPU_EUNSUPPORTED, who + ": a header line of more than " + std::to_string(sb::kFastaMaxHeader) + " bytes; use the host form");
      if (n_names < 0 || n_names > n_bytes || n_bases < 0 || n_bases > n_bytes) return api_fail(SBGPU_EHIP, who + ": the sizes disagree (did the buffer change under the call?)");
      return SBGPU_OK;
   }

   // ---- the pack, the names, and what comes back
   int pack(sb::DevBlock &w, const sb::FastaTileLayout &L, sb::DevBlock &q, const sb::FastaContigLayout &Q, sb::FastaArgs &a)
   {
      uint8_t *d_seq = nullptr;
      SB_FRONT_TRY(hipMalloc((void **)&d_seq, (size_t)std::max<int64_t>(n_bases, 8)));
      G->d_seq = d_seq, G->device = sb::ctx_device(c), G->dev_free = fasta_dev_free, G->dev_fetch = fasta_dev_fetch; // (the handle's from here on, on every way out)
      sb::DevBlock nb(s);
      SB_FRONT_TRY(nb.take((size_t)std::max<int64_t>(n_names, 8)));
      a.n_bases = n_bases, a.seq = d_seq;
      Stage stage(c, "fasta_pack", s);
      hipLaunchKernelGGL(sb::fasta_pack_kernel, dim3(sb::fasta_grid(L.tiles)), dim3(64), 0, s, a);
      SB_FRONT_TRY(hipGetLastError());
      stage.end();
      Stage stage_back(c, "fasta_names_copy_back", s);
      if (n_contigs) {
         hipLaunchKernelGGL(sb::fasta_names_kernel, dim3(sb::fasta_grid_contigs(n_contigs)), dim3(256), 0, s, d_bytes, n_bytes, q.at<const int64_t>(Q.hdr_off),
                            q.at<const int64_t>(Q.name_at), n_contigs, n_names, (uint8_t *)nb.p);
         SB_FRONT_TRY(hipGetLastError());
      }
      const size_t n = (size_t)n_contigs;
      name_off.resize(n + 1), offset.resize(n), line_bases.resize(n), line_width.resize(n), seq_off.resize(n + 1), first_odd.resize(n), ragged32.resize(n);
      names.resize((size_t)n_names);
      SB_FRONT_TRY(hipMemcpyAsync(name_off.data(), q.p + Q.name_at, (n + 1) * 8, hipMemcpyDeviceToHost, s));
      if (n) {
         SB_FRONT_TRY(hipMemcpyAsync(offset.data(), q.p + Q.offset, n * 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipMemcpyAsync(line_bases.data(), q.p + Q.line_bases, n * 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipMemcpyAsync(line_width.data(), q.p + Q.line_width, n * 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipMemcpyAsync(seq_off.data(), q.p + Q.seq_off, n * 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipMemcpyAsync(first_odd.data(), q.p + Q.first_odd, n * 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipMemcpyAsync(ragged32.data(), q.p + Q.ragged, n * 4, hipMemcpyDeviceToHost, s));
      }
      if (n_names) SB_FRONT_TRY(hipMemcpyAsync(&names[0], nb.p, (size_t)n_names, hipMemcpyDeviceToHost, s));
      stage_back.end();
      SB_FRONT_TRY(hipStreamSynchronize(s));
      seq_off[n] = n_bases;
      return SBGPU_OK;
   }

   int run()
   {
      SB_FRONT_TRY(hipSetDevice(sb::ctx_device(c)));
      sb::ctx_stage_reset(c);
      if (n_bytes > 0) {
         const sb::FastaTileLayout L = sb::fasta_tile_layout(n_bytes);
         sb::DevBlock w(s), q(s);
         SB_FRONT_TRY(w.take(L.bytes));
         SB_FRONT_RC(count(w, L));
         const sb::FastaContigLayout Q = sb::fasta_contig_layout(n_contigs);
         SB_FRONT_TRY(q.take(Q.bytes));
         sb::FastaArgs a;
         SB_FRONT_RC(index(w, L, q, Q, a));
         SB_FRONT_RC(pack(w, L, q, Q, a));
      } else {
         name_off.assign(1, 0), seq_off.assign(1, 0);
      }
      // RAGGED: a base out of phase, or a base behind a '\n' that ends no full line
      std::vector<uint8_t> ragged((size_t)n_contigs, 0);
      for (size_t k = 0; k < (size_t)n_contigs; ++k) ragged[k] = ragged32[k] != 0 || first_odd[k] < seq_off[k + 1];
      SB_FRONT_RC(sb::fasta_finish(who, n_bytes, n_lines, std::move(name_off), std::move(names), std::move(offset), std::move(line_bases), std::move(line_width),
                                   std::move(seq_off), ragged, G));
      if (G->d_seq) G->info[10] = 1, G->info[11] = G->device;
      return SBGPU_OK;
   }
};

using FastaHandle = std::unique_ptr<sbgpu_fasta_t, sb::HandleDeleter<sbgpu_fasta_destroy>>;

// the runs of sbgpu_binseq_fasta_*: [run_off[r], run_off[r + 1]) ascend from 0 to n_bins, on contigs the handle has and that hold bases
int check_runs(const std::string &who, const sbgpu_fasta_t *g, int64_t n_runs, const int64_t *run_off, const int32_t *run_contig, int64_t n_bins)
{
   if (!g || n_runs < 0 || n_bins < 0 || (n_runs && (!run_off || !run_contig))) return api_fail(SBGPU_EINVAL, who + ": bad argument");
   if (n_runs == 0) return n_bins == 0 ? SBGPU_OK : api_fail(SBGPU_EINVAL, who + ": bins without a run");
   if (run_off[0] != 0 || run_off[n_runs] != n_bins) return api_fail(SBGPU_EINVAL, who + ": the runs must cover the bins from 0 to n_bins");
   for (int64_t r = 0; r < n_runs; ++r) {
      if (run_off[r + 1] < run_off[r]) return api_fail(SBGPU_EINVAL, who + ": decreasing run_off");
      const int64_t k = run_contig[r];
      if (k < 0 || k >= (int64_t)g->flags.size()) return api_fail(SBGPU_EINVAL, who + ": run " + std::to_string(r) + " names a contig the genome does not have");
      if (g->flags[(size_t)k] & sb::kFastaEmpty) return api_fail(SBGPU_EINVAL, who + ": run " + std::to_string(r) + " lies on an empty contig");
      if (g->seq_off[(size_t)k + 1] - g->seq_off[(size_t)k] > 0xffffffffll) return api_fail(SBGPU_ESHAPE, who + ": a contig of 2^32 bases or more");
   }
   return SBGPU_OK;
}

} // namespace

extern "C" {

int sbgpu_fasta_read_device(sbgpu_ctx_t *c, const uint8_t *d_bytes, int64_t n_bytes, void *stream, sbgpu_fasta_t **out)
{
   if (!c || !out || n_bytes < 0 || (n_bytes && !d_bytes)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_read_device: bad argument");
   *out = nullptr;
   const hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   try {
      FastaHandle G(new sbgpu_fasta());
      FastaDeviceCall call = {c, d_bytes, n_bytes, s, G.get()};
      SB_FRONT_RC(call.run());
      *out = G.release();
   } catch (const std::bad_alloc &) {
      (void)hipStreamSynchronize(s);
      return api_fail(SBGPU_ENOMEM, "sbgpu_fasta_read_device: out of memory");
   } catch (const std::exception &e) { // (std::length_error of a container: nothing C++ crosses the C ABI)
      (void)hipStreamSynchronize(s);
      return api_fail(SBGPU_ENOMEM, std::string("sbgpu_fasta_read_device: ") + e.what());
   }
   return SBGPU_OK;
}

int sbgpu_fasta_read_upload(sbgpu_ctx_t *c, const uint8_t *bytes, int64_t n_bytes, void *stream, sbgpu_fasta_t **out)
{
   if (!c || !out || n_bytes < 0 || (n_bytes && !bytes)) return api_fail(SBGPU_EINVAL, "sbgpu_fasta_read_upload: bad argument");
   *out = nullptr;
   const hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   SB_FRONT_TRY(hipSetDevice(sb::ctx_device(c)));
   sb::DevBlock d(s);
   SB_FRONT_TRY(d.take((size_t)std::max<int64_t>(n_bytes, 8)));
   if (n_bytes) SB_FRONT_TRY(hipMemcpyAsync(d.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
   return sbgpu_fasta_read_device(c, (const uint8_t *)d.p, n_bytes, stream, out);
}

int sbgpu_binseq_fasta_device(sbgpu_ctx_t *c, const sbgpu_fasta_t *g, int64_t n_runs, const int64_t *run_off, const int32_t *run_contig, int64_t n_bins,
                              const int64_t *d_seg_off, const uint32_t *d_seg_left, const uint32_t *d_seg_right, double *d_gc, double *d_entropy, uint8_t *d_flags,
                              int32_t *d_error, void *stream)
{
   const std::string who = "sbgpu_binseq_fasta_device";
   if (!c) return api_fail(SBGPU_EINVAL, who + ": null context");
   if (const int rc = check_runs(who, g, n_runs, run_off, run_contig, n_bins)) return rc;
   if (!g->d_seq || g->device != sb::ctx_device(c)) return api_fail(SBGPU_EINVAL, who + ": the genome's sequence is not on the context's device");
   for (int64_t r = 0; r < n_runs; ++r) {
      const int64_t b0 = run_off[r], nb = run_off[r + 1] - b0, k = run_contig[r];
      if (nb == 0) continue;
      if (!d_seg_off || !d_gc || !d_entropy || !d_flags) return api_fail(SBGPU_EINVAL, who + ": null device pointer");
      SB_FRONT_RC(sbgpu_binseq_device(c, g->d_seq + g->seq_off[(size_t)k], 1, g->seq_off[(size_t)k + 1] - g->seq_off[(size_t)k], nb, d_seg_off + b0, d_seg_left, d_seg_right,
                                      d_gc + b0, d_entropy + b0, d_flags + b0, d_error, stream));
   }
   return SBGPU_OK;
}

int sbgpu_binseq_fasta_host(sbgpu_ctx_t *c, const sbgpu_fasta_t *g, int64_t n_runs, const int64_t *run_off, const int32_t *run_contig, int64_t n_bins,
                            const int64_t *seg_off, const uint32_t *seg_left, const uint32_t *seg_right, double *gc_out, double *entropy_out, uint8_t *flags_out)
{
   const std::string who = "sbgpu_binseq_fasta_host";
   if (!c) return api_fail(SBGPU_EINVAL, who + ": null context");
   if (const int rc = check_runs(who, g, n_runs, run_off, run_contig, n_bins)) return rc;
   if (n_bins == 0) return SBGPU_OK;
   if (!seg_off || !gc_out || !entropy_out || !flags_out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (seg_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": offsets must start at 0");
   for (int64_t b = 0; b < n_bins; ++b)
      if (seg_off[b + 1] < seg_off[b]) return api_fail(SBGPU_EINVAL, who + ": decreasing seg_off");
   if (seg_off[n_bins] && (!seg_left || !seg_right)) return api_fail(SBGPU_EINVAL, who + ": null coordinate array");
   try {
      std::vector<int64_t> off;
      std::vector<uint8_t> window;
      for (int64_t r = 0; r < n_runs; ++r) {
         const int64_t b0 = run_off[r], nb = run_off[r + 1] - b0, k = run_contig[r];
         if (nb == 0) continue;
         const int64_t len = g->seq_off[(size_t)k + 1] - g->seq_off[(size_t)k], s0 = seg_off[b0], s1 = seg_off[b0 + nb];
         // the contig's window: from the first base the run's segments touch to the last
         int64_t lo = len, hi = 1;
         for (int64_t i = s0; i < s1; ++i) {
            const int64_t l = seg_left[i], rr = seg_right[i];
            if (rr < l || l < 1 || rr > len) return api_fail(SBGPU_EINVAL, who + ": a segment of run " + std::to_string(r) + " lies outside its contig");
            lo = std::min(lo, l), hi = std::max(hi, rr);
         }
         if (s1 == s0) lo = hi = 1;
         const uint8_t *genome = nullptr;
         if (g->d_seq) {
            window.resize((size_t)(hi - lo + 1));
            SB_FRONT_RC(sbgpu_fasta_fetch(g, k, lo, hi - lo + 1, window.data()));
            genome = window.data();
         } else {
            genome = g->seq.data() + g->seq_off[(size_t)k] + lo - 1;
         }
         off.resize((size_t)nb + 1);
         for (int64_t b = 0; b <= nb; ++b) off[(size_t)b] = seg_off[b0 + b] - s0;
         SB_FRONT_RC(sbgpu_binseq_host(c, genome, lo, hi - lo + 1, nb, off.data(), seg_left ? seg_left + s0 : nullptr, seg_right ? seg_right + s0 : nullptr, gc_out + b0,
                                       entropy_out + b0, flags_out + b0));
      }
   } catch (const std::exception &) {
      return api_fail(SBGPU_ENOMEM, who + ": out of memory");
   }
   return SBGPU_OK;
}

} // extern "C"
