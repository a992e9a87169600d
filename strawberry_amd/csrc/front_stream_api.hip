// strawberry_amd/csrc/front_stream_api.hip -- sbgpu_front_stream_* (include/sbgpu.h): alignment records -> abundances for a
// caller that holds the records in HOST memory and hands them over chunk by chunk, with a bounded footprint on the device.
//
// The reference streams too: Sample::nextClusterRefDemand / procSample hold ONE cluster's reads at a time
// (/root/reference/src/alignments.cpp:1145-1187, 1736-1811).  The device entries of the front end take a whole sample's records
// resident (196 GB of arenas at 3.9e8 records); here the unit is a chunk of the inflated record stream -- inflated by the
// caller (push), or handed over as the file's own BGZF members and inflated here, behind the link (push_bgzf, at the end):
//
//   push(chunk i)   the chunk's bytes start their way to the device (copy stream; two device buffers alternate), then chunk
//                   i - 1 -- uploaded during the push before -- is computed: sbgpu_bam_decode_device ->
//                   sbgpu_assign_reads_device over the clusters not yet finished -> the clusters that are COMPLETE (a record
//                   behind their end has been seen) -> sbgpu_pair_mates_device -> sbgpu_collapse_pairs_device -> their unique
//                   hits appended to the stream's store on the device.  The records of the first incomplete cluster onward
//                   are carried: their bytes are copied in front of the next chunk's (device to device) and decoded again
//                   with it -- a cluster's records are never split;
//   end()           the last chunk (every remaining cluster is complete now), then ONE sbgpu_quantify_resident over the
//                   store: pass 1 (the empirical insert-size law is the WHOLE sample's: it cannot be known earlier), bins,
//                   weights, EM, FPKM, the all-reduce, TPM.  The unique hits are a seventh of the records' bytes.
//
//   push_bgzf(chunk i)  the same with WHOLE BGZF members in place of whole records: the compressed bytes and the members' table
//                   travel; when the chunk's turn to be computed comes it is inflated where an inflated chunk would have
//                   landed (sbgpu_bgzf_inflate_device, behind the carry), the window [carry | chunk] is indexed on the device
//                   (sbgpu_bam_index_device's scheme, the members' starts as guesses), and the stages above run unchanged.
//                   Members do not end on record boundaries in general: the bytes of a record the window cuts join the
//                   carry and are completed by the next chunk's.
//
// So upload and compute overlap chunk by chunk, the arenas are a chunk's, and what grows with the sample is the store.
// Results: those of the resident entries on the whole sample, bit for bit (same clusters, same order, same kernels).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "front_common.h"

using sb::api_fail;

namespace {
// a device array that grows (geometric; the old block goes back to the pool)
struct Grow {
   char *p = nullptr;
   size_t cap = 0, used = 0;
   hipError_t reserve(size_t want, hipStream_t s)
   {
      if (want <= cap) return hipSuccess;
      char *np = nullptr;
      size_t got = 0;
      hipError_t e = sb::dev_take(sb::grow_capacity(want, cap), &np, &got);
      if (e != hipSuccess) return e;
      if (used) e = hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      sb::dev_give(p, cap);
      p = np, cap = got;
      return e;
   }
   void release()
   {
      sb::dev_give(p, cap);
      p = nullptr, cap = used = 0;
   }
};

__global__ void add_i32_kernel(int32_t *x, int64_t n, int32_t add)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i < n) x[i] += add;
}
__global__ void add_i64_kernel(int64_t *x, int64_t n, int64_t add)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i < n) x[i] += add;
}
// a window's record offsets: the carried records' (the tail of the window before, re-based) and the chunk's (behind the carry)
__global__ void window_off_kernel(int64_t *dst, const int64_t *prev_tail, int64_t n_carry, int64_t c0, const int64_t *chunk_off, int64_t n_new,
                                  int64_t carry_bytes)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i < n_carry) dst[i] = prev_tail[i] - c0;
   else if (i <= n_carry + n_new) dst[i] = carry_bytes + (n_new ? chunk_off[i - n_carry] : 0);
}
} // namespace

struct sbgpu_front_stream {
   sbgpu_ctx_t *ctx = nullptr;
   int device = 0;
   // the clusters (host copies), and how far the stream has come
   std::vector<int32_t> c_ref;
   std::vector<uint32_t> c_left, c_right;
   std::vector<uint8_t> c_strand;
   int64_t n_clusters = 0, k0 = 0; // clusters [0, k0) are done
   sbgpu_bam_opts_t opts = {};
   // two device buffers: [carry room | chunk], each half `room` bytes (chunk_cap rounded up to 256: the chunk lands aligned);
   // the chunk in flight (uploaded, not yet computed).  chunk_cap is the caller's chunk_bytes exactly: the most bytes a push
   // and a carry may hold
   int64_t chunk_cap = 0, room = 0;
   char *buf[2] = {nullptr, nullptr};
   size_t buf_cap[2] = {0, 0};
   int cur = 0;                    // the buffer that holds the pending chunk
   bool pending = false;
   int64_t pend_bytes = 0, pend_records = 0;
   Grow d_pend[2];                 // the pending chunk's record offsets (relative to the chunk's first byte) [n + 1], uploaded with the chunk
   hipEvent_t ev_up[2] = {nullptr, nullptr};
   hipStream_t up_stream = nullptr; // the uploads' own stream, at the LOWEST priority: HIP streams of one priority share a few hardware
                                    // queues (the context alone has ten), and an upload that lands in the compute stream's queue
                                    // serialises with the kernels it is meant to run beside; another priority is another queue
   // the carry: bytes (at the tail of the buffer just computed, copied in front of the next chunk) and their offsets -- the
   // tail of the window's offsets (device), from record carry_rec on, first byte carry_c0
   int64_t carry_bytes = 0, carry_n = 0, carry_rec = 0, carry_c0 = 0;
   Grow d_win[2];                  // the windows' record offsets on the device (this window's, the one before's)
   int win = 0;
   // the store: the unique hits of the finished clusters (sbgpu_hits_t layout)
   Grow s_locus, s_foff, s_code, s_left, s_right, s_mass;
   int64_t n_hits = 0, n_feat = 0;
   std::vector<int64_t> locus_hit_off; // [n_clusters + 1] once finished
   // totals
   int64_t n_records = 0, n_decoded = 0, n_accepted = 0, n_pairs = 0, n_filtered = 0, mapped_reads = 0, n_chunks = 0, carry_max = 0, redecoded = 0;
   size_t free_at_begin = 0, min_free = 0;
   bool ended = false;
   // push_bgzf: the pending chunk's compressed bytes and its table (blk_off | out_off | statuses) on the device, the table's
   // host copy (for the message about a member that fails), and what the chunk's computation needs to know
   int mode = 0;                   // 0: nothing pushed yet, 1: push, 2: push_bgzf (never both in one stream)
   Grow d_comp[2], d_tab[2];
   std::vector<int64_t> h_blk[2], h_out[2];
   int64_t pend_blocks = 0, pend_first = 0, comp_bytes = 0;
   double t_wait = 0, t_compute = 0, t_enqueue = 0, t_last = 0; // seconds: waiting for uploads, computing chunks, enqueuing uploads, the last stage
   void note_memory()
   {
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) == hipSuccess) min_free = std::min(min_free, fr);
   }
};

namespace {

double now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The chunk in buffer F->cur (uploaded), with the carry in front of it: decode .. unique hits of the clusters it completes.
// What the window arithmetic decides is front_schedule.h's (stream_clusters_done, stream_carry); the steps below issue it.
struct PendingCall {
   sbgpu_front_stream *const F;
   const bool last;
   sbgpu_ctx_t *const c = F->ctx;
   const hipStream_t s = sb::ctx_stream(c);
   const int b = F->cur;
   // the window: [carry | chunk], its record offsets
   const int64_t n_carry = F->carry_n;
   int64_t n_new = F->pending ? F->pend_records : 0, n_rec = n_carry + n_new;
   int64_t w_bytes = F->carry_bytes + (F->pending ? F->pend_bytes : 0), w_end = w_bytes; // the window's whole records; all its bytes
   char *w0 = F->buf[b] + F->room - F->carry_bytes;                                      // (the carry was copied to end where the chunk begins)
   Grow &W = F->d_win[F->win], &P = F->d_win[F->win ^ 1];                                // this window's offsets, the one before's
   bool finished = false; // a step has ended the call: nothing is left to compute
   // the window's reads, which cluster each is offered to, the clusters they complete
   sb::BamReadsHandle R;
   sbgpu_reads_t reads = {};
   int64_t n_reads = 0, nc = 0;
   std::vector<int64_t> roff;
   sb::DevBlock d_cluster{s};
   sb::StreamDone done = {0, 0};
   int64_t carry_rec = 0, c0 = 0; // where the next window's carry begins: window record index; its first byte in the window

   // ---- a chunk of BGZF members: inflate it where an inflated chunk would have landed, then find the window's records
   int inflate_and_index()
   {
      const int64_t nm = F->pending ? F->pend_blocks : 0;
      int64_t first = 0;
      if (nm) {
         const int64_t *d_blk = (const int64_t *)F->d_tab[b].p, *d_out = d_blk + (nm + 1);
         uint8_t *d_status = (uint8_t *)(d_out + (nm + 1));
         const int64_t blk0 = F->h_blk[b][0], out0 = F->h_out[b][0];
         int64_t failed = 0;
         SB_FRONT_RC(sbgpu_bgzf_inflate_device(c, (const uint8_t *)((uintptr_t)F->d_comp[b].p - (uintptr_t)blk0), F->h_blk[b][(size_t)nm], d_blk, d_out, nm,
                                               (uint8_t *)((uintptr_t)(F->buf[b] + F->room) - (uintptr_t)out0), s, d_status, &failed));
         if (failed) {
            std::vector<uint8_t> st((size_t)nm);
            SB_FRONT_TRY(hipMemcpyAsync(st.data(), d_status, (size_t)nm, hipMemcpyDeviceToHost, s));
            SB_FRONT_TRY(hipStreamSynchronize(s));
            size_t k = 0;
            while (k + 1 < st.size() && !st[k]) ++k;
            return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: the BGZF member at byte " + std::to_string(F->h_blk[b][k]) +
                                             " of the file does not inflate to its ISIZE bytes (SBGPU_BGZF status " + std::to_string((int)st[k]) + "; " +
                                             std::to_string(failed) + " of the push's " + std::to_string(nm) + " members failed)");
         }
         first = std::min(F->pend_first, F->pend_bytes); // the header's bytes in this chunk
         if (first && F->carry_bytes) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: first_record in a push behind the first records");
         w0 += first, w_end -= first;
      }
      n_rec = 0, w_bytes = 0;
      if (w_end > 0) {
         const int64_t n = sb::bam_index_device_impl(c, (const uint8_t *)w0, w_end, 0, nm ? (const int64_t *)F->d_tab[b].p + (nm + 1) : nullptr, nm ? nm + 1 : 0,
                                                     F->carry_bytes - first - (nm ? F->h_out[b][0] : 0),
                                                     [&](int64_t n_records) -> int64_t * {
                                                        W.used = 0;
                                                        return W.reserve((size_t)(n_records + 1) * 8, s) == hipSuccess ? (int64_t *)W.p : nullptr;
                                                     },
                                                     &w_bytes, s);
         if (n < 0) return (int)n;
         n_rec = n;
      }
      n_new = n_rec - n_carry;
      if (last && w_bytes < w_end) return api_fail(SBGPU_ESHAPE, "sbgpu_front_stream_end: the stream ends inside a record");
      if (n_rec == 0 && w_end > 0) { // no record is whole yet: the window's bytes wait for the next chunk's
         const sb::StreamCarry carry = sb::stream_carry(w_end, 0, F->chunk_cap);
         if (!carry.fits) return api_fail(SBGPU_ESHAPE, "sbgpu_front_stream_push_bgzf: one record exceeds a chunk's capacity: begin the stream with larger chunks");
         F->carry_n = 0, F->carry_rec = 0, F->carry_c0 = 0;
         SB_FRONT_RC(copy_carry(carry.bytes, 0));
         finished = true;
      }
      return SBGPU_OK;
   }

   // the carry's bytes, in front of where the next chunk lands in the OTHER buffer
   int copy_carry(int64_t bytes, int64_t from)
   {
      F->carry_bytes = bytes;
      F->carry_max = std::max(F->carry_max, bytes);
      if (bytes) {
         SB_FRONT_TRY(hipMemcpyAsync(F->buf[b ^ 1] + F->room - bytes, w0 + from, (size_t)bytes, hipMemcpyDeviceToDevice, s));
         SB_FRONT_TRY(hipStreamSynchronize(s));
      }
      return SBGPU_OK;
   }

   // the window's record offsets, made on the device from the window before and the chunk's own: 8 bytes per record never pass
   // through host loops (a window of BGZF members was indexed instead)
   int window_offsets()
   {
      W.used = 0;
      SB_FRONT_TRY(W.reserve((size_t)(n_rec + 1) * 8, s));
      hipLaunchKernelGGL(window_off_kernel, dim3((unsigned)((n_rec + 1 + 255) / 256)), dim3(256), 0, s, (int64_t *)W.p, (const int64_t *)P.p + F->carry_rec, n_carry,
                         F->carry_c0, (const int64_t *)F->d_pend[b].p, n_new, F->carry_bytes);
      SB_FRONT_TRY(hipGetLastError());
      return SBGPU_OK;
   }

   int decode()
   {
      sbgpu_bamreads_t *r = nullptr;
      SB_FRONT_RC(sbgpu_bam_decode_device(c, (const uint8_t *)w0, w_bytes, (const int64_t *)W.p, n_rec, &F->opts, s, &r));
      R.reset(r);
      return SBGPU_OK;
   }

   // which of the remaining clusters every read is offered to; which of them are complete
   int assign()
   {
      const int32_t *d_ref = nullptr;
      const uint32_t *d_left = nullptr, *d_right = nullptr;
      SB_FRONT_RC(sbgpu_bamreads_reads(R.get(), &reads, &d_ref, &d_left, &d_right));
      n_reads = reads.n_reads;
      nc = F->n_clusters - F->k0;
      roff.assign((size_t)nc + 1, 0);
      SB_FRONT_TRY(d_cluster.take((size_t)std::max<int64_t>(n_reads, 1) * 4));
      sbgpu_clusters_t cl = {nc, F->c_ref.data() + F->k0, F->c_left.data() + F->k0, F->c_right.data() + F->k0, F->c_strand.data() + F->k0};
      if (nc > 0)
         SB_FRONT_RC(sbgpu_assign_reads_device(c, &cl, n_reads, d_ref, d_left, d_right, (uint8_t *)reads.flags, d_cluster.at<int32_t>(0), roff.data(), s));
      done = sb::stream_clusters_done(roff.data(), nc, n_reads, last);
      return SBGPU_OK;
   }

   // ---- the carry for the next window: from the record of the first read that was not consumed
   int find_carry()
   {
      carry_rec = n_rec, c0 = w_bytes;
      if (!last && done.reads_done < n_reads) {
         const int64_t *d_record = sb::bamreads_device_record(R.get());
         SB_FRONT_TRY(hipMemcpyAsync(&carry_rec, d_record + done.reads_done, 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipStreamSynchronize(s));
         SB_FRONT_TRY(hipMemcpyAsync(&c0, (const int64_t *)W.p + carry_rec, 8, hipMemcpyDeviceToHost, s));
         SB_FRONT_TRY(hipStreamSynchronize(s));
      }
      return SBGPU_OK;
   }

   // the complete clusters' reads -> pairs -> unique hits -> the store
   int pair_and_collapse()
   {
      sbgpu_reads_t part = reads;
      part.n_reads = done.reads_done;
      sbgpu_matepairs_t *m = nullptr;
      SB_FRONT_RC(sbgpu_pair_mates_device(c, done.n_done, &part, roff.data(), s, &m));
      sb::MatePairsHandle M(m);
      sbgpu_pairs_t pairs;
      const int64_t *poff = nullptr;
      SB_FRONT_RC(sbgpu_matepairs_pairs(M.get(), &pairs, &poff));
      F->n_pairs += pairs.n_pairs;
      sbgpu_uniq_dev_t *u = nullptr;
      SB_FRONT_RC(sbgpu_collapse_pairs_device(c, done.n_done, &pairs, poff, s, &u));
      sb::UniqDevHandle U(u);
      SB_FRONT_RC(append_to_store(U.get()));
      SB_FRONT_TRY(hipStreamSynchronize(s)); // (the handles go away with this scope)
      return SBGPU_OK;
   }

   // the unique hits behind the store's: the cluster numbers and the feature offsets shifted to the stream's
   int append_to_store(const sbgpu_uniq_dev_t *U)
   {
      int64_t ui[8];
      SB_FRONT_RC(sbgpu_uniq_dev_info(U, ui));
      sbgpu_hits_t h;
      const float *d_mass = nullptr;
      const int64_t *hoff = nullptr;
      SB_FRONT_RC(sbgpu_uniq_dev_hits(U, &h, &d_mass, &hoff));
      const int64_t nh = ui[0], nf = ui[1];
      F->n_filtered += ui[2], F->mapped_reads += ui[4];
      // one row per array of the store: what is there, what joins it (`tail`: the offsets' entry beyond the last hit)
      struct Column {
         Grow &g;
         const void *src;
         size_t elem;
         int64_t have, add, tail;
      };
      const Column columns[6] = {{F->s_locus, h.hit_locus, 4, F->n_hits, nh, 0}, {F->s_foff, h.feat_off, 8, F->n_hits, nh, 1}, {F->s_mass, d_mass, 4, F->n_hits, nh, 0},
                                 {F->s_code, h.feat_code, 1, F->n_feat, nf, 0},  {F->s_left, h.feat_left, 4, F->n_feat, nf, 0}, {F->s_right, h.feat_right, 4, F->n_feat, nf, 0}};
      for (const Column &col : columns) SB_FRONT_TRY(col.g.reserve((size_t)(col.have + col.add + col.tail) * col.elem, s));
      for (const Column &col : columns) {
         if (col.add) SB_FRONT_TRY(hipMemcpyAsync(col.g.p + (size_t)col.have * col.elem, col.src, (size_t)(col.add + col.tail) * col.elem, hipMemcpyDeviceToDevice, s));
         col.g.used = (size_t)(col.have + col.add + col.tail) * col.elem;
      }
      if (nh) {
         if (F->k0) hipLaunchKernelGGL(add_i32_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, (int32_t *)F->s_locus.p + F->n_hits, nh, (int32_t)F->k0);
         if (F->n_feat) hipLaunchKernelGGL(add_i64_kernel, dim3((unsigned)((nh + 1 + 255) / 256)), dim3(256), 0, s, (int64_t *)F->s_foff.p + F->n_hits, nh + 1, F->n_feat);
         SB_FRONT_TRY(hipGetLastError());
      }
      for (int64_t k = 0; k < done.n_done; ++k) F->locus_hit_off[(size_t)(F->k0 + k + 1)] = F->n_hits + hoff[(size_t)k + 1];
      F->n_hits += nh, F->n_feat += nf;
      return SBGPU_OK;
   }

   // the totals, then the carry: the window's records from carry_rec on (with them the bytes of a record the window cut: push_bgzf)
   int set_carry()
   {
      // (every accepted record counts once: in the window that consumes it -- the last consumes all, reads behind the last cluster too)
      F->n_records += n_new, F->n_decoded += n_rec, F->n_accepted += last ? n_reads : done.reads_done;
      F->k0 += done.n_done;
      const sb::StreamCarry carry = sb::stream_carry(w_end, c0, F->chunk_cap);
      if (!carry.fits)
         return api_fail(SBGPU_ESHAPE, "sbgpu_front_stream_push: the records of one cluster exceed a chunk's capacity (" + std::to_string(carry.bytes) + " bytes): begin the stream with larger chunks");
      F->carry_n = n_rec - carry_rec, F->carry_rec = carry_rec, F->carry_c0 = c0;
      F->win ^= 1; // (this window's offsets are the next one's "window before")
      return copy_carry(carry.bytes, c0);
   }

   int run()
   {
      F->n_chunks += F->pending && F->pend_bytes ? 1 : 0; // (an empty push is no chunk)
      F->redecoded += n_carry;
      if (F->mode == 2) SB_FRONT_RC(inflate_and_index());
      if (finished) return SBGPU_OK;
      if (n_rec == 0) {
         if (last) { // nothing more will come: the clusters not yet finished are, without hits
            for (int64_t k = F->k0; k < F->n_clusters; ++k) F->locus_hit_off[(size_t)k + 1] = F->n_hits;
            F->k0 = F->n_clusters;
         }
         return SBGPU_OK;
      }
      if (F->mode != 2) SB_FRONT_RC(window_offsets());
      SB_FRONT_RC(decode());
      SB_FRONT_RC(assign());
      SB_FRONT_RC(find_carry());
      if (done.n_done > 0 && done.reads_done > 0) SB_FRONT_RC(pair_and_collapse());
      else
         for (int64_t k = 0; k < done.n_done; ++k) F->locus_hit_off[(size_t)(F->k0 + k + 1)] = F->n_hits;
      SB_FRONT_RC(set_carry());
      F->note_memory();
      return SBGPU_OK;
   }
};

int compute_pending(sbgpu_front_stream *F, bool last)
{
   hipStream_t s = sb::ctx_stream(F->ctx);
   // every stage below synchronises the stream it ran on before it returns, so the arenas its handles give back are idle: they
   // must not wait for the DEVICE -- the next chunk's upload is running on it
   sb::DevGiveStreamSynced no_device_wait;
   const double t_in = now_seconds();
   SB_FRONT_TRY(hipEventSynchronize(F->ev_up[F->cur])); // the chunk has arrived
   const double t_arrived = now_seconds();
   F->t_wait += t_arrived - t_in;
   const int rc = PendingCall{F, last}.run(); // (the window's handles are back in the pool behind it: their time is the chunk's)
   F->t_compute += now_seconds() - t_arrived;
   if (rc == SBGPU_OK) F->pending = false;
   return rc;
}

} // namespace


extern "C" {

int sbgpu_front_stream_begin(sbgpu_ctx_t *c, const sbgpu_clusters_t *cl, const sbgpu_bam_opts_t *opts, int64_t chunk_bytes,
                             sbgpu_front_stream_t **out)
{
   if (!c || !cl || !opts || !out) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_begin: null argument");
   *out = nullptr;
   if (cl->n_clusters < 0 || (cl->n_clusters && (!cl->ref || !cl->left || !cl->right || !cl->strand)))
      return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_begin: bad clusters");
   if (chunk_bytes < (1 << 16) || chunk_bytes > ((int64_t)1 << 36)) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_begin: a chunk holds 64 KB .. 64 GB");
   sbgpu_front_stream *F = new (std::nothrow) sbgpu_front_stream();
   if (!F) return api_fail(SBGPU_ENOMEM, "sbgpu_front_stream_begin: out of host memory");
   F->ctx = c, F->device = sb::ctx_device(c);
   F->n_clusters = cl->n_clusters;
   F->c_ref.assign(cl->ref, cl->ref + cl->n_clusters);
   F->c_left.assign(cl->left, cl->left + cl->n_clusters);
   F->c_right.assign(cl->right, cl->right + cl->n_clusters);
   F->c_strand.assign(cl->strand, cl->strand + cl->n_clusters);
   F->opts = *opts;
   F->chunk_cap = chunk_bytes;
   F->room = (int64_t)sb::up256((size_t)chunk_bytes);
   F->locus_hit_off.assign((size_t)cl->n_clusters + 1, 0);
   hipError_t e = hipSetDevice(F->device);
   size_t tot = 0;
   if (e == hipSuccess) e = hipMemGetInfo(&F->free_at_begin, &tot);
   F->min_free = F->free_at_begin;
   if (e == hipSuccess) {
      int least = 0, greatest = 0;
      e = hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (e == hipSuccess) e = hipStreamCreateWithPriority(&F->up_stream, hipStreamNonBlocking, least);
   }
   for (int b = 0; b < 2 && e == hipSuccess; ++b) {
      e = sb::dev_take((size_t)F->room * 2, &F->buf[b], &F->buf_cap[b]); // [carry room | chunk]
      if (e == hipSuccess) e = hipEventCreateWithFlags(&F->ev_up[b], hipEventDisableTiming);
   }
   if (e != hipSuccess) {
      sbgpu_front_stream_destroy(F);
      return sb::api_fail_hip(e, "sbgpu_front_stream_begin");
   }
   *out = F;
   return SBGPU_OK;
}

int sbgpu_front_stream_push(sbgpu_front_stream_t *F, const uint8_t *bytes, int64_t n_bytes, const int64_t *rec_off, int64_t n_records)
{
   if (!F || F->ended) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push: no stream (or it has ended)");
   if (n_bytes < 0 || (n_bytes && !bytes) || n_bytes > F->chunk_cap) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push: a chunk holds at most the bytes the stream was begun with");
   if (F->mode == 2) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push: the stream is fed with BGZF members (push_bgzf); the two are not mixed");
   F->mode = 1;
   const hipStream_t s = F->up_stream; // the entry's stream: the uploads'
   SB_FRONT_TRY(hipSetDevice(F->device));
   // the chunk's record offsets: the caller's (noted while inflating), or found here
   std::vector<int64_t> found;
   if (rec_off) {
      if (n_records < 0 || rec_off[0] != 0 || rec_off[n_records] != n_bytes) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push: rec_off must run from 0 to n_bytes (whole records only)");
   } else {
      found.resize((size_t)(n_bytes / 36 + 2));
      n_records = sbgpu_bam_index_host(bytes, n_bytes, found.data(), (int64_t)found.size() - 1);
      if (n_records < 0) return SBGPU_ESHAPE;
      rec_off = found.data();
   }
   // this chunk starts its way to the device (into the buffer the pending chunk does NOT use), its offsets in front of it ...
   const double t_push = now_seconds();
   const int nb = F->pending ? F->cur ^ 1 : F->cur;
   F->d_pend[nb].used = 0;
   SB_FRONT_TRY(F->d_pend[nb].reserve((size_t)(n_records + 1) * 8, s));
   SB_FRONT_TRY(hipMemcpyAsync(F->d_pend[nb].p, rec_off, (size_t)(n_records + 1) * 8, hipMemcpyHostToDevice, s));
   if (!found.empty()) SB_FRONT_TRY(hipStreamSynchronize(s)); // (the offsets found here live in this frame)
   if (n_bytes) SB_FRONT_TRY(hipMemcpyAsync(F->buf[nb] + F->room, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
   SB_FRONT_TRY(hipEventRecord(F->ev_up[nb], s));
   F->t_enqueue += now_seconds() - t_push;
   // ... while the pending one is computed (its carry lands in front of this chunk, in buffer nb)
   if (F->pending) SB_FRONT_RC(compute_pending(F, false));
   else if (F->carry_bytes) return api_fail(SBGPU_EHIP, "sbgpu_front_stream_push: internal: a carry without a pending chunk");
   F->cur = nb;
   F->pending = true;
   F->pend_bytes = n_bytes;
   F->pend_records = n_records;
   return SBGPU_OK;
}

int sbgpu_front_stream_push_bgzf(sbgpu_front_stream_t *F, const uint8_t *file_bytes, int64_t n_bytes, const int64_t *blk_off, const int64_t *out_off,
                                 int64_t n_blocks, int64_t first_record)
{
   if (!F || F->ended) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: no stream (or it has ended)");
   if (F->mode == 1) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: the stream is fed with inflated records (push); the two are not mixed");
   if (n_bytes < 0 || n_blocks < 0 || first_record < 0 || (n_bytes && !file_bytes) || (n_blocks && (!blk_off || !out_off)) || (!n_blocks && n_bytes))
      return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: bad argument");
   for (int64_t k = 0; k < n_blocks; ++k)
      if (blk_off[k + 1] < blk_off[k] || out_off[k + 1] < out_off[k])
         return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: blk_off and out_off must ascend");
   if (n_blocks && blk_off[n_blocks] - blk_off[0] != n_bytes)
      return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_push_bgzf: file_bytes must hold exactly the members blk_off[0] .. blk_off[n_blocks] (whole members only)");
   const int64_t span = n_blocks ? out_off[n_blocks] - out_off[0] : 0;
   if (span > F->chunk_cap)
      return api_fail(SBGPU_ESHAPE, "sbgpu_front_stream_push_bgzf: the push inflates to " + std::to_string(span) + " bytes, more than the chunks the stream was begun with");
   const hipStream_t s = F->up_stream; // the entry's stream: the uploads'
   SB_FRONT_TRY(hipSetDevice(F->device));
   F->mode = 2;
   const double t_push = now_seconds();
   const int nb = F->pending ? F->cur ^ 1 : F->cur;
   // the table (kept on the host too: the caller's arrays are free once this returns) and the compressed bytes start their way
   F->h_blk[nb].assign(blk_off, blk_off + (n_blocks ? n_blocks + 1 : 0));
   F->h_out[nb].assign(out_off, out_off + (n_blocks ? n_blocks + 1 : 0));
   if (n_blocks) {
      const size_t tab = (size_t)(n_blocks + 1) * 8;
      F->d_tab[nb].used = 0, F->d_comp[nb].used = 0;
      SB_FRONT_TRY(F->d_tab[nb].reserve(2 * tab + (size_t)n_blocks, s));
      SB_FRONT_TRY(F->d_comp[nb].reserve((size_t)n_bytes + 16, s));
      SB_FRONT_TRY(hipMemcpyAsync(F->d_tab[nb].p, F->h_blk[nb].data(), tab, hipMemcpyHostToDevice, s));
      SB_FRONT_TRY(hipMemcpyAsync(F->d_tab[nb].p + tab, F->h_out[nb].data(), tab, hipMemcpyHostToDevice, s));
      SB_FRONT_TRY(hipMemcpyAsync(F->d_comp[nb].p, file_bytes, (size_t)n_bytes, hipMemcpyHostToDevice, s));
   }
   SB_FRONT_TRY(hipEventRecord(F->ev_up[nb], s));
   F->t_enqueue += now_seconds() - t_push;
   // ... while the pending chunk is inflated and computed (its carry lands in front of where this one will be inflated)
   if (F->pending) SB_FRONT_RC(compute_pending(F, false));
   F->cur = nb;
   F->pending = true;
   F->pend_bytes = span, F->pend_records = 0;
   F->pend_blocks = n_blocks, F->pend_first = first_record;
   F->comp_bytes += n_bytes;
   return SBGPU_OK;
}

int sbgpu_front_stream_end(sbgpu_front_stream_t *F, const sbgpu_annotation_t *an, const sbgpu_insert_t *insert, int32_t read_len, int32_t long_read,
                           const sbgpu_abundance_params_t *params, sbgpu_comm_t *comm, sbgpu_insert_t *insert_used, sbgpu_abundances_t *out,
                           sbgpu_bins_t **bins_out)
{
   if (!F || F->ended) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_end: no stream (or it has ended)");
   if (!an || !params || !out || !bins_out) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_end: null argument");
   if (an->n_loci != F->n_clusters) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_end: the annotation's loci are the stream's clusters, one to one");
   const hipStream_t s = sb::ctx_stream(F->ctx);
   SB_FRONT_TRY(hipSetDevice(F->device));
   if (!F->pending) { // nothing was pushed (or an empty last chunk): the carry alone, if any
      SB_FRONT_TRY(hipEventRecord(F->ev_up[F->cur], s));
   }
   SB_FRONT_RC(compute_pending(F, true));
   F->ended = true;
   // the chunk buffers are not needed any more: the last stage gets their room
   for (int b = 0; b < 2; ++b) {
      sb::dev_give(F->buf[b], F->buf_cap[b]);
      F->buf[b] = nullptr, F->buf_cap[b] = 0;
   }
   for (int b = 0; b < 2; ++b) F->d_win[b].release(), F->d_pend[b].release(), F->d_comp[b].release(), F->d_tab[b].release();
   (void)sbgpu_release_idle_memory();
   SB_FRONT_TRY(F->s_foff.reserve(8, s));
   if (F->n_hits == 0) SB_FRONT_TRY(hipMemsetAsync(F->s_foff.p, 0, 8, s));
   sbgpu_hits_t h = {F->n_hits, (const int32_t *)F->s_locus.p, (const int64_t *)F->s_foff.p, (const uint8_t *)F->s_code.p,
                     (const uint32_t *)F->s_left.p, (const uint32_t *)F->s_right.p};
   const double t_q = now_seconds();
   const int rc = sbgpu_quantify_resident(F->ctx, an, &h, (const float *)F->s_mass.p, F->locus_hit_off.data(), insert, read_len, long_read,
                                          F->mapped_reads, params, comm, insert_used, out, bins_out);
   F->t_last = now_seconds() - t_q;
   F->note_memory();
   if (std::getenv("SBGPU_HOST_TIMING")) // diagnostic: where the pass' time went, on stderr
      std::fprintf(stderr, "sbgpu_front_stream: %lld chunks | waiting for uploads %.1f ms | computing chunks %.1f ms | enqueuing uploads %.1f ms | last stage %.1f ms\n",
                   (long long)F->n_chunks, F->t_wait * 1e3, F->t_compute * 1e3, F->t_enqueue * 1e3, F->t_last * 1e3);
   return rc;
}

int sbgpu_front_stream_info(const sbgpu_front_stream_t *F, int64_t info[16])
{
   if (!F || !info) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_info: null argument");
   const int64_t v[16] = {F->n_records, F->n_accepted, F->n_pairs, F->n_hits, F->n_feat, F->n_filtered, F->mapped_reads, F->n_chunks,
                          F->k0, F->carry_max, F->redecoded, (int64_t)F->min_free, F->chunk_cap, F->ended ? 1 : 0, (int64_t)F->free_at_begin, F->comp_bytes};
   std::memcpy(info, v, sizeof(v));
   return SBGPU_OK;
}

int sbgpu_front_stream_hits(const sbgpu_front_stream_t *F, sbgpu_hits_t *d_hits, const float **d_hit_mass, const int64_t **locus_hit_off)
{
   if (!F) return api_fail(SBGPU_EINVAL, "sbgpu_front_stream_hits: null stream");
   if (d_hits)
      *d_hits = {F->n_hits, (const int32_t *)F->s_locus.p, (const int64_t *)F->s_foff.p, (const uint8_t *)F->s_code.p, (const uint32_t *)F->s_left.p,
                 (const uint32_t *)F->s_right.p};
   if (d_hit_mass) *d_hit_mass = (const float *)F->s_mass.p;
   if (locus_hit_off) *locus_hit_off = F->locus_hit_off.data();
   return SBGPU_OK;
}

void sbgpu_front_stream_destroy(sbgpu_front_stream_t *F)
{
   if (!F) return;
   (void)hipSetDevice(F->device);
   (void)hipDeviceSynchronize(); // (an upload may still be in flight)
   for (int b = 0; b < 2; ++b) {
      sb::dev_give(F->buf[b], F->buf_cap[b]);
      if (F->ev_up[b]) (void)hipEventDestroy(F->ev_up[b]);
   }
   if (F->up_stream) (void)hipStreamDestroy(F->up_stream);
   for (int b = 0; b < 2; ++b) F->d_win[b].release(), F->d_pend[b].release(), F->d_comp[b].release(), F->d_tab[b].release();
   for (Grow *g : {&F->s_locus, &F->s_foff, &F->s_code, &F->s_left, &F->s_right, &F->s_mass}) g->release();
   delete F;
}

} // extern "C"
