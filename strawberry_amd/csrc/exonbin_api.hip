// strawberry_amd/csrc/exonbin_api.hip -- sbgpu_exonbin_device / sbgpu_exonbin_host
// (include/sbgpu.h): launch of the per-hit compatibility + bin-key kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "bins_device.h"
#include "exonbin_device.h"
#include "stage_host.h"

using sb::api_fail;

namespace sb {
// sbgpu_exonbin_device that also leaves every hit's span and sequence hash (exonbin_device.h) when asked to
size_t seg_basis_bytes(int64_t n_loci, int64_t n_iso)
{
   const size_t ni1 = (size_t)(n_iso > 0 ? n_iso : 1);
   return 4 * sb::up256(ni1 * 8) + 2 * sb::up256((size_t)n_loci * 8) + sb::up256((size_t)n_loci * 4);
}
int make_seg_basis(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, int64_t n_iso, char *dm, void *stream, DeviceSegBasis *out)
{
   const size_t ni1 = (size_t)(n_iso > 0 ? n_iso : 1);
   const size_t isz = sb::up256(ni1 * 8), lsz = sb::up256((size_t)an->n_loci * 8);
   const size_t o_mem = 0, o_sta = isz, o_memh = 2 * isz, o_stah = 3 * isz, o_adj = 4 * isz, o_adjh = o_adj + lsz, o_ok = o_adjh + lsz;
   sb::ExonBinArgs a = {};
   a.iso_off = an->iso_off;
   a.exon_off = an->exon_off;
   a.exon_left = an->exon_left;
   a.exon_right = an->exon_right;
   a.seg_off = an->seg_off;
   a.seg_left = an->seg_left;
   a.seg_right = an->seg_right;
   const int64_t cap = (int64_t)sb::ctx_cu_count(c) * 8, lb = (an->n_loci + 255) / 256, ib = ((int64_t)ni1 + 255) / 256;
   hipLaunchKernelGGL(sb::iso_masks_locus_kernel, dim3((unsigned)(lb < cap ? lb : cap)), dim3(256), 0, (hipStream_t)stream, a, an->n_loci,
                      (uint32_t *)(dm + o_ok), (uint64_t *)(dm + o_adj), (uint64_t *)(dm + o_adjh));
   hipLaunchKernelGGL(sb::iso_masks_kernel, dim3((unsigned)(ib < cap * 4 ? ib : cap * 4)), dim3(256), 0, (hipStream_t)stream, a, an->n_loci, n_iso,
                      (uint64_t *)(dm + o_mem), (uint64_t *)(dm + o_sta), (uint32_t *)(dm + o_ok), (uint64_t *)(dm + o_memh), (uint64_t *)(dm + o_stah));
   const hipError_t e = hipGetLastError();
   if (e != hipSuccess) return api_fail(SBGPU_EHIP, std::string("iso_masks_kernel: ") + hipGetErrorString(e));
   out->member = (const uint64_t *)(dm + o_mem);
   out->start = (const uint64_t *)(dm + o_sta);
   out->adj = (const uint64_t *)(dm + o_adj);
   out->member_hi = (const uint64_t *)(dm + o_memh);
   out->start_hi = (const uint64_t *)(dm + o_stah);
   out->adj_hi = (const uint64_t *)(dm + o_adjh);
   out->ok = (const uint32_t *)(dm + o_ok);
   return SBGPU_OK;
}

int exonbin_device_impl(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *hits, int32_t compat_words,
                        int32_t key_words, uint32_t *d_compat, uint32_t *d_key, uint64_t *d_span, uint32_t *d_fhash, void *stream,
                        int64_t n_iso, const DeviceSegBasis *seg_pre)
{
   if (!c || !an || !hits) return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_device: null argument");
   if (hits->n_hits == 0) return SBGPU_OK;
   if (hits->n_hits < 0 || an->n_loci < 1 || compat_words < 0 || key_words < 0)
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_device: bad counts");
   if (!an->iso_off || !an->exon_off || !an->seg_off || !hits->hit_locus || !hits->feat_off ||
       (compat_words && !d_compat) || (key_words && !d_key))
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_device: null device pointer");
   sb::ExonBinArgs a;
   a.iso_off = an->iso_off;
   a.exon_off = an->exon_off;
   a.exon_left = an->exon_left;
   a.exon_right = an->exon_right;
   a.seg_off = an->seg_off;
   a.seg_left = an->seg_left;
   a.seg_right = an->seg_right;
   a.n_hits = hits->n_hits;
   a.hit_locus = hits->hit_locus;
   a.feat_off = hits->feat_off;
   a.feat_code = hits->feat_code;
   a.feat_left = hits->feat_left;
   a.feat_right = hits->feat_right;
   a.compat_words = compat_words;
   a.key_words = key_words;
   a.compat = d_compat;
   a.key = d_key;
   a.span = d_span;
   a.fhash = d_span ? d_fhash : nullptr;
   a.iso_member = a.iso_start = nullptr;
   a.locus_seg_ok = nullptr;
   a.locus_adj = nullptr;
   a.iso_member_hi = a.iso_start_hi = a.locus_adj_hi = nullptr;
   // the isoforms in the segment basis (exonbin_device.h): loci of up to 64 segments (key_words <= 2 covers them all);
   // the kernel walks the exons for whatever the basis does not cover
   if (key_words >= 1 && compat_words >= 1) {
      DeviceSegBasis sbz;
      if (seg_pre) {
         sbz = *seg_pre; // made once for a resident annotation
      } else {
         if (n_iso < 0) { // a caller with a device annotation only: one 8-byte read
            hipError_t ec = hipMemcpyAsync(&n_iso, an->iso_off + an->n_loci, 8, hipMemcpyDeviceToHost, (hipStream_t)stream);
            if (ec == hipSuccess) ec = hipStreamSynchronize((hipStream_t)stream);
            if (ec != hipSuccess) return api_fail(SBGPU_EHIP, std::string("sbgpu_exonbin_device: ") + hipGetErrorString(ec));
         }
         char *dm = nullptr;
         hipError_t em = sb::ctx_scratch(c, 3, seg_basis_bytes(an->n_loci, n_iso), &dm);
         if (em != hipSuccess) return api_fail(em == hipErrorOutOfMemory ? SBGPU_ENOMEM : SBGPU_EHIP, std::string("hipMalloc: ") + hipGetErrorString(em));
         const int rc = make_seg_basis(c, an, n_iso, dm, stream, &sbz);
         if (rc != SBGPU_OK) return rc;
      }
      a.iso_member = sbz.member;
      a.iso_start = sbz.start;
      a.locus_seg_ok = sbz.ok;
      a.locus_adj = sbz.adj;
      a.iso_member_hi = sbz.member_hi;
      a.iso_start_hi = sbz.start_hi;
      a.locus_adj_hi = sbz.adj_hi;
   }
   const int64_t blocks_wanted = (hits->n_hits + 255) / 256;
   if (blocks_wanted > 0x7fffffff) return api_fail(SBGPU_ESHAPE, "sbgpu_exonbin_device: more than 2^39 hits in one call");
   hipLaunchKernelGGL(sb::exonbin_kernel, dim3((unsigned)blocks_wanted), dim3(256), 0, (hipStream_t)stream, a);
   // loci of 65-128 segments or isoforms (form 3 of iso_masks_kernel): their regular hits in the 128-bit segment basis.
   // Only an annotation with words beyond two can have such a locus; everywhere else the kernel is not launched.
   if (a.locus_seg_ok && (key_words > 2 || compat_words > 2))
      hipLaunchKernelGGL(sb::exonbin_seg128_kernel, dim3((unsigned)blocks_wanted), dim3(256), 0, (hipStream_t)stream, a);
   hipError_t e = hipGetLastError();
   if (e != hipSuccess) return api_fail(SBGPU_EHIP, std::string("exonbin_kernel: ") + hipGetErrorString(e));
   return SBGPU_OK;
}
} // namespace sb

extern "C" {

int sbgpu_exonbin_device(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *hits,
                         int32_t compat_words, int32_t key_words, uint32_t *d_compat, uint32_t *d_key,
                         void *stream)
{
   return sb::exonbin_device_impl(c, an, hits, compat_words, key_words, d_compat, d_key, nullptr, nullptr, stream, -1);
}

int sbgpu_exonbin_host(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *hits,
                       int32_t compat_words, int32_t key_words, uint32_t *compat_out, uint32_t *key_out)
{
   if (!c || !an || !hits) return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: null argument");
   const int64_t nh = hits->n_hits, nl = an->n_loci;
   if (nh == 0) return SBGPU_OK;
   if (nh < 0 || nl < 1 || compat_words < 0 || key_words < 0)
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: bad counts");
   if (!an->iso_off || !an->exon_off || !an->seg_off || !hits->hit_locus || !hits->feat_off ||
       (compat_words && !compat_out) || (key_words && !key_out))
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: null argument");
   // ---- validate the CSR structure (the device form trusts it)
   if (an->iso_off[0] != 0 || an->exon_off[0] != 0 || an->seg_off[0] != 0 || hits->feat_off[0] != 0)
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: offsets must start at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t ni = an->iso_off[l + 1] - an->iso_off[l], ns = an->seg_off[l + 1] - an->seg_off[l];
      if (ni < 0 || ns < 0) return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: decreasing offsets");
      if (ni > 32 * (int64_t)compat_words)
         return api_fail(SBGPU_ESHAPE, "sbgpu_exonbin_host: compat_words does not cover a locus' isoforms");
      if (ns > 32 * (int64_t)key_words)
         return api_fail(SBGPU_ESHAPE, "sbgpu_exonbin_host: key_words does not cover a locus' segments");
   }
   const int64_t n_iso = an->iso_off[nl], n_seg = an->seg_off[nl];
   for (int64_t i = 0; i < n_iso; ++i)
      if (an->exon_off[i + 1] < an->exon_off[i]) return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: decreasing exon_off");
   const int64_t n_exon = an->exon_off[n_iso];
   if ((n_exon && (!an->exon_left || !an->exon_right)) || (n_seg && (!an->seg_left || !an->seg_right)))
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: null coordinate array");
   for (int64_t h = 0; h < nh; ++h) {
      if (hits->hit_locus[h] < 0 || hits->hit_locus[h] >= nl)
         return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: hit_locus out of range");
      if (hits->feat_off[h + 1] < hits->feat_off[h]) return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: decreasing feat_off");
   }
   const int64_t n_feat = hits->feat_off[nh];
   if (n_feat && (!hits->feat_code || !hits->feat_left || !hits->feat_right))
      return api_fail(SBGPU_EINVAL, "sbgpu_exonbin_host: null feature array");

   // ---- one device arena, one upload per array
   struct Part {
      const void *src;
      size_t bytes, off;
   };
   Part parts[] = {
      {an->iso_off, (size_t)(nl + 1) * 8, 0},     {an->exon_off, (size_t)(n_iso + 1) * 8, 0},
      {an->seg_off, (size_t)(nl + 1) * 8, 0},     {hits->feat_off, (size_t)(nh + 1) * 8, 0},
      {an->exon_left, (size_t)n_exon * 4, 0},     {an->exon_right, (size_t)n_exon * 4, 0},
      {an->seg_left, (size_t)n_seg * 4, 0},       {an->seg_right, (size_t)n_seg * 4, 0},
      {hits->hit_locus, (size_t)nh * 4, 0},       {hits->feat_left, (size_t)n_feat * 4, 0},
      {hits->feat_right, (size_t)n_feat * 4, 0},  {hits->feat_code, (size_t)n_feat, 0},
   };
   size_t total = 0;
   for (Part &p : parts) {
      p.off = total;
      total += (p.bytes + 255) & ~(size_t)255;
   }
   const size_t off_compat = total;
   total += (((size_t)nh * compat_words * 4) + 255) & ~(size_t)255;
   const size_t off_key = total;
   total += (((size_t)nh * key_words * 4) + 255) & ~(size_t)255;
   char *d = nullptr;
   hipError_t e = hipMalloc(&d, total ? total : 256);
   if (e != hipSuccess)
      return api_fail(e == hipErrorOutOfMemory ? SBGPU_ENOMEM : SBGPU_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
   hipStream_t s = sb::ctx_stream(c);
   auto bail = [&](hipError_t err, const char *what) {
      (void)hipFree(d);
      return api_fail(SBGPU_EHIP, std::string(what) + ": " + hipGetErrorString(err));
   };
   for (Part &p : parts)
      if (p.bytes && (e = hipMemcpyAsync(d + p.off, p.src, p.bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
         return bail(e, "hipMemcpyAsync(H2D)");
   sbgpu_annotation_t dan = *an;
   dan.iso_off = (const int64_t *)(d + parts[0].off);
   dan.exon_off = (const int64_t *)(d + parts[1].off);
   dan.seg_off = (const int64_t *)(d + parts[2].off);
   dan.exon_left = (const uint32_t *)(d + parts[4].off);
   dan.exon_right = (const uint32_t *)(d + parts[5].off);
   dan.seg_left = (const uint32_t *)(d + parts[6].off);
   dan.seg_right = (const uint32_t *)(d + parts[7].off);
   sbgpu_hits_t dh = *hits;
   dh.feat_off = (const int64_t *)(d + parts[3].off);
   dh.hit_locus = (const int32_t *)(d + parts[8].off);
   dh.feat_left = (const uint32_t *)(d + parts[9].off);
   dh.feat_right = (const uint32_t *)(d + parts[10].off);
   dh.feat_code = (const uint8_t *)(d + parts[11].off);
   int rc = sbgpu_exonbin_device(c, &dan, &dh, compat_words, key_words, (uint32_t *)(d + off_compat),
                                 (uint32_t *)(d + off_key), s);
   if (rc != SBGPU_OK) {
      (void)hipFree(d);
      return rc;
   }
   if (compat_words &&
       (e = hipMemcpyAsync(compat_out, d + off_compat, (size_t)nh * compat_words * 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return bail(e, "hipMemcpyAsync(D2H compat)");
   if (key_words && (e = hipMemcpyAsync(key_out, d + off_key, (size_t)nh * key_words * 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return bail(e, "hipMemcpyAsync(D2H key)");
   if ((e = hipStreamSynchronize(s)) != hipSuccess) return bail(e, "hipStreamSynchronize");
   (void)hipFree(d);
   return SBGPU_OK;
}

} // extern "C"

namespace sb {
// The isoforms' segment lists (Isoform::_exon_segs, include/isoform.h:59-71; contig.cpp:615-634), their loci and
// exonic lengths, from the host annotation: two passes over the loci on host threads (count, then write).
void iso_segments(const sbgpu_annotation_t *an, IsoSegments *out)
{
   const int64_t nl = an->n_loci, n_iso = an->iso_off[nl];
   std::vector<int64_t> &iso_seg_off = out->seg_off;
   std::vector<int32_t> &iso_seg_idx = out->seg_idx, &iso_locus = out->locus, &iso_len = out->len;
   iso_seg_off.assign((size_t)n_iso + 1, 0);
   iso_locus.assign((size_t)(n_iso > 0 ? n_iso : 1), 0);
   iso_len.assign((size_t)(n_iso > 0 ? n_iso : 1), 0);
   iso_seg_idx.clear();
   {
      // two passes over the loci on host threads: count the segments of every isoform, then write them
      unsigned nt = std::thread::hardware_concurrency();
      if (nt > 16) nt = 16;
      if (const char *ev = std::getenv("SBGPU_HOST_THREADS")) nt = (unsigned)std::atoi(ev);
      if (nt < 1) nt = 1;
      if ((int64_t)nt * 2048 > nl) nt = (unsigned)std::max<int64_t>(1, nl / 2048);
      auto walk = [&](int64_t l, bool fill) {
         const int64_t s0 = an->seg_off[l], nseg = an->seg_off[l + 1] - s0;
         for (int64_t iso = an->iso_off[l]; iso < an->iso_off[l + 1]; ++iso) {
            const int64_t e0 = an->exon_off[iso], ne = an->exon_off[iso + 1] - e0;
            int64_t e = 0, n = 0;
            int32_t *dst = fill ? iso_seg_idx.data() + iso_seg_off[(size_t)iso] : nullptr;
            for (int64_t sidx = 0; sidx < nseg; ++sidx) {
               const uint32_t sl = an->seg_left[s0 + sidx], sr = an->seg_right[s0 + sidx];
               while (e < ne && an->exon_right[e0 + e] < sl) ++e; // contig.cpp:615-634; segments ascend
               if (e < ne && an->exon_left[e0 + e] <= sl && an->exon_right[e0 + e] >= sr) {
                  if (fill) dst[n] = (int32_t)sidx;
                  ++n;
               }
            }
            if (!fill) {
               int64_t len = 0;
               for (int64_t x = 0; x < ne; ++x) len += (int64_t)an->exon_right[e0 + x] - an->exon_left[e0 + x] + 1;
               iso_seg_off[(size_t)iso + 1] = n; // a count for now
               iso_locus[(size_t)iso] = (int32_t)l;
               iso_len[(size_t)iso] = (int32_t)len;
            }
         }
      };
      auto run = [&](bool fill) {
         if (nt <= 1) {
            for (int64_t l = 0; l < nl; ++l) walk(l, fill);
            return;
         }
         std::vector<std::thread> pool;
         for (unsigned t = 0; t < nt; ++t)
            pool.emplace_back([&, t]() {
               for (int64_t l = nl * t / nt; l < nl * (t + 1) / nt; ++l) walk(l, fill);
            });
         for (auto &th : pool) th.join();
      };
      run(false);
      for (int64_t i = 0; i < n_iso; ++i) iso_seg_off[(size_t)i + 1] += iso_seg_off[(size_t)i];
      iso_seg_idx.resize((size_t)iso_seg_off[(size_t)n_iso]);
      run(true);
   }
}

// ---- sbgpu_bins_create_device: the hits of every locus grouped into bins, the bins packed, the (bin, isoform) pairs made.
// What the host decides on the way -- order, launches, layouts, fix-ups -- is bins_schedule.h's; the stages below issue it.
namespace {
// a HIP call that must succeed (SBGPU_EHIP, "<the call>: <HIP's text>")
#define SB_TRY(expr)                                                                    \
   do {                                                                                 \
      hipError_t e_ = (expr);                                                           \
      if (e_ != hipSuccess) return api_fail(SBGPU_EHIP, sb::hip_error_text(#expr, e_)); \
   } while (0)

// one launch record (bins_schedule.h: bins_group_steps) -> the matching instantiation; `cap`: 8 x the CUs
hipError_t launch_group_step(const BinsStep &st, int64_t cap, hipStream_t s, const BinsArgs &a)
{
   const dim3 grid((unsigned)std::min<int64_t>(st.count, cap * st.grid_mult)), block((unsigned)st.threads);
   auto is = [&](int kernel, int slots, int max_bins, int threads, int cw, bool retry) {
      return st.kernel == kernel && st.slots == slots && st.max_bins == max_bins && st.threads == threads && st.cw == cw && st.retry == retry;
   };
   if (is(kBinsAccum, kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, 1, false)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, 1>), grid, block, 0, s, a);
   else if (is(kBinsAccum, kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, 2, false)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, 2>), grid, block, 0, s, a);
   else if (is(kBinsAccum, kBinsSlotsMid, kBinsMaxMid, kBinsThreadsAccum, 1, true)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsMid, kBinsMaxMid, kBinsThreadsAccum, 1, true>), grid, block, 0, s, a);
   else if (is(kBinsAccum, kBinsSlotsMid, kBinsMaxMid, kBinsThreadsAccum, 2, true)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsMid, kBinsMaxMid, kBinsThreadsAccum, 2, true>), grid, block, 0, s, a);
   else if (is(kBinsAccum, kBinsSlotsLight, kBinsMaxLight, kBinsThreads, 1, true)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsLight, kBinsMaxLight, kBinsThreads, 1, true>), grid, block, 0, s, a);
   else if (is(kBinsAccum, kBinsSlotsLight, kBinsMaxLight, kBinsThreads, 2, true)) hipLaunchKernelGGL((bins_accum_kernel<kBinsSlotsLight, kBinsMaxLight, kBinsThreads, 2, true>), grid, block, 0, s, a);
   else if (is(kBinsLocus, kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, 0, false)) hipLaunchKernelGGL((bins_locus_kernel<kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads>), grid, block, 0, s, a);
   else if (is(kBinsLocus, kBinsSlotsMid, kBinsMaxMid, kBinsThreadsMid, 0, true)) hipLaunchKernelGGL((bins_locus_kernel<kBinsSlotsMid, kBinsMaxMid, kBinsThreadsMid, true>), grid, block, 0, s, a);
   else return hipErrorInvalidValue; // a record no kernel was built for: a missing kernel is an error
   return hipGetLastError();
}

// One call's state, stage by stage.  It owns the two pool arenas until the handle has them: every early return ends in the
// destructor, which waits for the stream (kernels may still use them) and then gives back what is left.
struct BinsCall {
   // -- the arguments
   sbgpu_ctx_t *c;
   const sbgpu_annotation_t *an;
   const sbgpu_hits_t *dh;
   const float *d_mass;
   const int64_t *locus_hit_off;
   int32_t cw, kw;
   const uint32_t *d_compat, *d_key;
   int64_t *d_hit_bin;
   hipStream_t s;
   const IsoSegments *iso_pre;
   sbgpu_bins_t **out;
   const uint64_t *d_span;
   const uint32_t *d_fhash;
   const GroupingHooks *hooks;
   // -- shape (validate)
   int64_t nl = 0, nh = 0, n_iso = 0, n_seg = 0, cap = 0; // cap: 8 x the CUs, the grids' unit
   const sbgpu_annotation_t *d_an = nullptr;              // the annotation / the segment lists in device memory already (hooks)
   const DeviceIsoSegments *d_iso = nullptr;
   bool want_local = false;
   // -- SBGPU_HOST_TIMING: stage times on stderr; =2: host clock only, no synchronisation
   bool timing = false, timing_sync = false;
   double t_stage = 0;
   // -- memory (take_memory): the context's scratch (d, d3: nothing to free), its pinned words, and the two pool arenas
   BinsScratchLayout L{};
   BinsPackedLayout P{};
   PairsInLayout R{};
   BinsPinnedLayout H{};
   char *d = nullptr, *d3 = nullptr, *pin = nullptr;
   char *d2 = nullptr; // the packed per-bin arrays: the handle takes them over (DeviceBinArrays)
   size_t d2_cap = 0;
   DevicePairs dp;     // the pairs' arena: the handle's too
   IsoSegments own_segments;
   int32_t *nb = nullptr, *nu = nullptr; // pinned: bins / hits used per locus
   volatile int32_t *flags_h = nullptr;
   volatile int64_t *totals_h = nullptr;
   hipStream_t cs = nullptr;
   hipEvent_t ev_up = nullptr, ev_rows = nullptr, ev_in = nullptr, ev_acc = nullptr;
   BinsArgs a{};
   BinsPackArgs pk{};
   PairsArgs pa{};
   // -- decisions and what came back
   BinsOrder order;
   BinsGroupSteps steps;
   bool speculative = false, fixed_up = false, any_wide_locus = false;
   unsigned lgrid = 1, pgrid = 1;
   BinsRows rows;

   ~BinsCall()
   {
      if (!d2 && !dp.arena) return;
      (void)hipStreamSynchronize(s);
      dev_give(dp.arena, dp.capacity);
      dev_give(d2, d2_cap);
   }
   static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
   void stage(const char *name)
   {
      if (!timing) return;
      if (timing_sync) (void)hipStreamSynchronize(s);
      const double t = now();
      std::fprintf(stderr, "  bins_create_device: %-16s %.2f ms\n", name, (t - t_stage) * 1e3);
      t_stage = t;
   }

   int validate();
   int take_memory();
   void fill_args();
   int upload_and_group();
   hipError_t fetch_rows();
   hipError_t launch_middle();
   hipError_t serve_list(const std::vector<int32_t> &loci);
   int fix_up();
   int finish_middle();
   int fill_pairs();
   int make_handle();
};

int BinsCall::validate()
{
   if (!c || !an || !dh || !locus_hit_off || !out) return api_fail(SBGPU_EINVAL, "sbgpu_bins_create_device: null argument");
   *out = nullptr;
   nl = an->n_loci, nh = dh->n_hits;
   if (nl < 1 || nh < 0 || cw < 1 || kw < 1) return api_fail(SBGPU_EINVAL, "sbgpu_bins_create_device: bad counts");
   if (nh > 0x7fffffff) return api_fail(SBGPU_ESHAPE, "sbgpu_bins_create_device: more than 2^31 hits in one call");
   if (nh && (!dh->feat_off || !dh->feat_left || !dh->feat_right || !d_mass || !d_compat || !d_key))
      return api_fail(SBGPU_EINVAL, "sbgpu_bins_create_device: null device pointer");
   if (locus_hit_off[0] != 0 || locus_hit_off[nl] != nh) return api_fail(SBGPU_EINVAL, "sbgpu_bins_create_device: locus_hit_off does not span the hits");
   for (int64_t l = 0; l < nl; ++l) {
      if (locus_hit_off[l + 1] < locus_hit_off[l]) return api_fail(SBGPU_EINVAL, "sbgpu_bins_create_device: decreasing locus_hit_off");
      if (an->iso_off[l + 1] - an->iso_off[l] > 32 * (int64_t)cw || an->seg_off[l + 1] - an->seg_off[l] > 32 * (int64_t)kw)
         return api_fail(SBGPU_ESHAPE, "sbgpu_bins_create_device: word counts do not cover a locus");
      any_wide_locus = any_wide_locus || an->iso_off[l + 1] - an->iso_off[l] > 64;
   }
   n_iso = an->iso_off[nl], n_seg = an->seg_off[nl];
   cap = (int64_t)ctx_cu_count(c) * 8;
   d_an = hooks ? hooks->d_annot : nullptr;
   d_iso = hooks ? hooks->d_iso : nullptr;
   want_local = hooks && hooks->d_hit_bin_local;
   const char *timing_env = std::getenv("SBGPU_HOST_TIMING");
   timing = timing_env != nullptr, timing_sync = timing && std::atoi(timing_env) != 2;
   t_stage = now();
   return SBGPU_OK;
}

// All device memory is sized before anything runs (bins <= hits), so that the kernels follow each other in the stream
int BinsCall::take_memory()
{
   L = bins_scratch_layout(nl, nh, cw, !d_span);
   hipError_t e = ctx_scratch(c, 2, L.bytes, &d);
   if (e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   if (!d_span && nh) { // spans and hashes the exon-bin kernel did not leave
      const int64_t blocks = (nh + 255) / 256, capb = cap * 4;
      hipLaunchKernelGGL(hit_signature_kernel, dim3((unsigned)(blocks < capb ? blocks : capb)), dim3(256), 0, s, nh, dh->feat_off, dh->feat_left,
                         dh->feat_right, (uint64_t *)(d + L.span), (uint32_t *)(d + L.fhash));
      SB_TRY(hipGetLastError());
   }
   P = bins_packed_layout(nh, cw, kw);
   if ((e = dev_take(P.bytes, &d2, &d2_cap)) != hipSuccess) return api_fail_hip(e, "hipMalloc");
   if (!iso_pre) { // a caller that knows the annotation earlier makes them while something else runs (chain_api.hip)
      iso_segments(an, &own_segments);
      iso_pre = &own_segments;
   }
   R = pairs_in_layout(nl, n_iso, n_seg, iso_pre->seg_idx.size());
   if ((e = ctx_scratch(c, 4, R.bytes, &d3)) != hipSuccess) return api_fail_hip(e, "hipMalloc");
   // pinned host words for what comes back between the kernels (copies into pageable memory would hold the host until the
   // stream has reached them)
   H = bins_pinned_layout(nl);
   if ((e = ctx_pinned(c, 0, H.bytes, &pin)) != hipSuccess) return api_fail(SBGPU_ENOMEM, hip_error_text("hipHostMalloc", e));
   nb = (int32_t *)(pin + H.nb), nu = (int32_t *)(pin + H.nu);
   flags_h = (volatile int32_t *)(pin + H.flag);
   totals_h = (volatile int64_t *)(pin + H.tot);
   SB_TRY(ctx_copy_stream(c, &cs));
   SB_TRY(ctx_event(c, 0, &ev_up));
   SB_TRY(ctx_event(c, 1, &ev_rows));
   SB_TRY(ctx_event(c, 2, &ev_in));
   SB_TRY(ctx_event(c, 4, &ev_acc));
   return SBGPU_OK;
}

// the three kernel families' arguments from the layouts (a.n_loci / a.loci: per launch)
void BinsCall::fill_args()
{
   a.n_loci = nl;
   a.locus_hit_off = (const int64_t *)(d + L.hoff);
   a.feat_off = dh->feat_off, a.feat_left = dh->feat_left, a.feat_right = dh->feat_right;
   a.mass = d_mass;
   a.compat_words = cw, a.key_words = kw;
   a.compat = d_compat, a.key = d_key;
   a.span = d_span ? d_span : (const uint64_t *)(d + L.span);
   a.fhash = d_span ? d_fhash : (const uint32_t *)(d + L.fhash);
   a.hit_bin_local = (int32_t *)(d + L.local);
   a.bin_rep = (int32_t *)(d + L.rep);
   a.bin_count = (int32_t *)(d + L.cnt);
   a.bin_compat = (uint32_t *)(d + L.cmp);
   a.dup = (uint8_t *)(d + L.dup);
   a.n_bins = (int32_t *)(d + L.nb), a.n_used = (int32_t *)(d + L.nu);
   a.flags = (int32_t *)(d + L.flag);

   pk.n_loci = nl;
   pk.locus_hit_off = a.locus_hit_off;
   pk.row_off = (const int64_t *)(d + L.roff);
   pk.compat_words = cw, pk.key_words = kw;
   pk.key = d_key;
   pk.hit_bin_local = a.hit_bin_local, pk.bin_rep = a.bin_rep, pk.bin_count_in = a.bin_count, pk.bin_compat_in = a.bin_compat;
   pk.count = (int32_t *)(d2 + P.cnt);
   pk.bin_key = (uint32_t *)(d2 + P.key);
   pk.bin_compat = (uint32_t *)(d2 + P.cmp);
   pk.hit_bin = d_hit_bin;
   pk.flags = a.flags + 1; // the middle's flags are a word of their own, cleared per launch: the middle may run twice

   pa.n_iso = n_iso;
   pa.iso_locus = d_iso ? d_iso->locus : (const int32_t *)(d3 + R.isoloc);
   pa.iso_off = d_an ? d_an->iso_off : (const int64_t *)(d3 + R.isoff);
   pa.row_off = pk.row_off;
   pa.f_off = (const int64_t *)(d3 + R.foff);
   pa.seg_off = d_an ? d_an->seg_off : (const int64_t *)(d3 + R.segoff);
   pa.seg_left = d_an ? d_an->seg_left : (const uint32_t *)(d3 + R.segl);
   pa.seg_right = d_an ? d_an->seg_right : (const uint32_t *)(d3 + R.segr);
   pa.iso_seg_off = d_iso ? d_iso->seg_off : (const int64_t *)(d3 + R.isegoff);
   pa.iso_seg_idx = d_iso ? d_iso->seg_idx : (const int32_t *)(d3 + R.isegidx);
   pa.iso_len = d_iso ? d_iso->len : (const int32_t *)(d3 + R.isolen);
   pa.compat_words = cw, pa.key_words = kw;
   pa.bin_key = pk.bin_key, pa.bin_compat = pk.bin_compat;
   pa.pair_cnt = (int32_t *)(d3 + R.pcnt), pa.seg_cnt = (int32_t *)(d3 + R.scnt);
   pa.pair_off = (const int64_t *)(d3 + R.poff), pa.pseg_off = (const int64_t *)(d3 + R.soff);
   pa.pair_seg_off = nullptr; // the pairs' arena: fill_pairs
   pa.pair_seg_lens = pa.pair_mask = nullptr;
   pa.pair_iso_len = nullptr;
   pa.pair_out_index = nullptr;
   pa.flags = a.flags + 1;
   // one wave per locus (bins_pairs_locus_kernel) for loci of up to 64 isoforms, the thread-per-isoform kernel for the others
   pa.only_wide_loci = 1;
   lgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nl + 3) / 4, cap * 8));
   pgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_iso + 255) / 256, cap * 4));
}

// Uploads on the copy stream, beside whatever the main stream still runs (the caller's exon-bin kernel): a copy in the main
// stream between two kernels costs the hand-over to the DMA engine and back, 0.3 ms each way measured.  First what the grouping
// kernels read (hit offsets, the loci's order), then the annotation's part of the pairs' inputs.  (Streams share hardware
// queues -- the copy stream may sit in the main stream's queue and then runs in issue order with it -- so nothing here counts on
// the overlap.)
int BinsCall::upload_and_group()
{
   SB_TRY(hipMemcpyAsync(d + L.hoff, locus_hit_off, (size_t)(nl + 1) * 8, hipMemcpyHostToDevice, cs));
   hipLaunchKernelGGL(bins_zero_kernel, dim3(1), dim3(256), 0, cs, (uint4 *)(d + L.flag), (int64_t)16);
   SB_TRY(hipGetLastError());
   order = bins_locus_order(nl, locus_hit_off, nh);
   steps = bins_group_steps(order.n_small, order.n_heavy, order.n_mid, cw, kw);
   // The bins' counts and compat words are [n_hits]-sized (a locus' bins sit at its hit offset): 1.3 GB for 1.6e8 hits,
   // 0.18 ms to zero at the memory's rate.  Only bins_locus_kernel's global atomics need the zeros -- the two-pass form
   // and the big table; the single-pass kernels write every entry they own -- so they are made where those run.
   if (steps.zero_first) {
      const int64_t n16 = (int64_t)(L.zero_bytes / 16); // (the arena's parts are 256-byte multiples)
      hipLaunchKernelGGL(bins_zero_kernel, dim3((unsigned)std::min<int64_t>((n16 + 255) / 256, cap * 4)), dim3(256), 0, cs, (uint4 *)(d + L.cnt), n16);
      SB_TRY(hipGetLastError());
   }
   SB_TRY(hipMemcpyAsync(d + L.order, order.order.data(), (size_t)nl * 4, hipMemcpyHostToDevice, cs));
   SB_TRY(hipEventRecord(ev_in, cs));
   SB_TRY(hipStreamWaitEvent(s, ev_in, 0));
   ctx_stage_begin(c, steps.single_pass ? "bins_accum_kernel" : "bins_locus_kernel", s);
   for (int i = 0; i < steps.n_steps; ++i) {
      a.n_loci = steps.steps[i].count;
      a.loci = (const int32_t *)(d + L.order) + steps.steps[i].first;
      SB_TRY(launch_group_step(steps.steps[i], cap, s, a));
   }
   ctx_stage_end(c, s);
   // (the annotation's part goes up while the grouping kernels run)
   if (!d_an) {
      SB_TRY(hipMemcpyAsync(d3 + R.isoff, an->iso_off, (size_t)(nl + 1) * 8, hipMemcpyHostToDevice, cs));
      SB_TRY(hipMemcpyAsync(d3 + R.segoff, an->seg_off, (size_t)(nl + 1) * 8, hipMemcpyHostToDevice, cs));
      if (n_seg) {
         SB_TRY(hipMemcpyAsync(d3 + R.segl, an->seg_left, (size_t)n_seg * 4, hipMemcpyHostToDevice, cs));
         SB_TRY(hipMemcpyAsync(d3 + R.segr, an->seg_right, (size_t)n_seg * 4, hipMemcpyHostToDevice, cs));
      }
   }
   if (!d_iso) {
      SB_TRY(hipMemcpyAsync(d3 + R.isegoff, iso_pre->seg_off.data(), (size_t)(n_iso + 1) * 8, hipMemcpyHostToDevice, cs));
      if (!iso_pre->seg_idx.empty()) SB_TRY(hipMemcpyAsync(d3 + R.isegidx, iso_pre->seg_idx.data(), iso_pre->seg_idx.size() * 4, hipMemcpyHostToDevice, cs));
      if (n_iso) {
         SB_TRY(hipMemcpyAsync(d3 + R.isoloc, iso_pre->locus.data(), (size_t)n_iso * 4, hipMemcpyHostToDevice, cs));
         SB_TRY(hipMemcpyAsync(d3 + R.isolen, iso_pre->len.data(), (size_t)n_iso * 4, hipMemcpyHostToDevice, cs));
      }
   }
   SB_TRY(hipEventRecord(ev_up, cs));
   SB_TRY(fetch_rows());
   return SBGPU_OK;
}

// Bins / hits used per locus and the grouping kernels' flags, to the pinned words -- on the copy stream, behind an event of
// the main one, which goes straight on to the middle (a copy in the main stream holds the next kernel back by the hand-over
// to the DMA engine: 0.25 ms measured here)
hipError_t BinsCall::fetch_rows()
{
   hipError_t x = hipEventRecord(ev_acc, s);
   if (x == hipSuccess) x = hipStreamWaitEvent(cs, ev_acc, 0);
   if (x == hipSuccess) x = hipMemcpyAsync(nb, d + L.nb, (size_t)nl * 4, hipMemcpyDeviceToHost, cs);
   if (x == hipSuccess) x = hipMemcpyAsync(nu, d + L.nu, (size_t)nl * 4, hipMemcpyDeviceToHost, cs);
   if (x == hipSuccess) x = hipMemcpyAsync((void *)flags_h, d + L.flag, 8, hipMemcpyDeviceToHost, cs);
   if (x == hipSuccess) x = hipEventRecord(ev_rows, cs);
   return x;
}

// The middle: rows scanned, bins packed, pairs counted and scanned -- behind the grouping kernels without a host round trip
hipError_t BinsCall::launch_middle()
{
   hipError_t x = hipMemsetAsync(d + L.flag + 4, 0, 4, s);
   if (x == hipSuccess) x = hipStreamWaitEvent(s, ev_up, 0);
   if (x != hipSuccess) return x;
   ctx_stage_begin(c, "bins_scan_*_kernel<rows> + bins_pack_kernel", s);
   int64_t *part_a = (int64_t *)(d3 + R.part), *part_b = part_a + std::max(R.row_tiles, R.iso_tiles) + 1, *tot = (int64_t *)(d3 + R.tot);
   ScanArgs sr = {nl, a.n_bins, nullptr, pa.iso_off, (int64_t *)(d + L.roff), (int64_t *)(d3 + R.foff), part_a, part_b, tot};
   hipLaunchKernelGGL(bins_scan_tiles_kernel<0>, dim3((unsigned)R.row_tiles), dim3(256), 0, s, sr);
   hipLaunchKernelGGL(bins_scan_parts_kernel, dim3(1), dim3(256), 0, s, sr, R.row_tiles);
   hipLaunchKernelGGL(bins_scan_apply_kernel<0>, dim3((unsigned)R.row_tiles), dim3(256), 0, s, sr);
   hipLaunchKernelGGL(bins_pack_kernel, dim3((unsigned)(nl < cap ? nl : cap)), dim3(256), 0, s, pk);
   ctx_stage_end(c, s);
   ctx_stage_begin(c, "bins_pairs_kernel<count> + bins_scan_*_kernel<pairs>", s);
   if (any_wide_locus) hipLaunchKernelGGL(bins_pairs_kernel<false>, dim3(pgrid), dim3(256), 0, s, pa);
   hipLaunchKernelGGL(bins_pairs_locus_kernel<false>, dim3(lgrid), dim3(256), 0, s, pa, nl);
   ScanArgs sp = {n_iso, pa.pair_cnt, pa.seg_cnt, nullptr, (int64_t *)(d3 + R.poff), (int64_t *)(d3 + R.soff), part_a, part_b, tot + 2};
   hipLaunchKernelGGL(bins_scan_tiles_kernel<1>, dim3((unsigned)R.iso_tiles), dim3(256), 0, s, sp);
   hipLaunchKernelGGL(bins_scan_parts_kernel, dim3(1), dim3(256), 0, s, sp, n_iso ? R.iso_tiles : 0);
   hipLaunchKernelGGL(bins_scan_apply_kernel<1>, dim3((unsigned)R.iso_tiles), dim3(256), 0, s, sp);
   ctx_stage_end(c, s);
   if ((x = hipGetLastError()) != hipSuccess) return x;
   x = hipMemcpyAsync((void *)totals_h, d3 + R.tot, 32, hipMemcpyDeviceToHost, s);
   if (x == hipSuccess) x = hipMemcpyAsync((void *)flags_h, d + L.flag, 8, hipMemcpyDeviceToHost, s);
   return x;
}

// a list of loci for a fix-up kernel, once the stream is through with the list before it (the caller keeps `loci` alive
// until the stream has read it)
hipError_t BinsCall::serve_list(const std::vector<int32_t> &loci)
{
   hipError_t x = hipStreamSynchronize(s);
   if (x == hipSuccess) x = hipMemcpyAsync(d + L.order, loci.data(), loci.size() * 4, hipMemcpyHostToDevice, s);
   a.n_loci = (int64_t)loci.size();
   a.loci = (const int32_t *)(d + L.order);
   return x;
}

// The counts come back; what they call for (bins_schedule.h) runs, or the device form declines
int BinsCall::fix_up()
{
   speculative = bins_speculative(steps.single_pass, d_hit_bin != nullptr);
   if (speculative) SB_TRY(launch_middle());
   SB_TRY(hipEventSynchronize(ev_rows));
   int32_t flags = flags_h[0];
   const std::vector<int32_t> redo = bins_redo_list(nb, nl);
   if (!redo.empty()) {
      fixed_up = true;
      SB_TRY(serve_list(redo));
      const dim3 grid((unsigned)std::min<int64_t>((int64_t)redo.size(), cap));
      if (steps.single_pass) { // these loci's entries were never zeroed (the other loci's stand as they are)
         hipLaunchKernelGGL(bins_zero_loci_kernel, grid, dim3(256), 0, s, a);
         SB_TRY(hipGetLastError());
      }
      hipLaunchKernelGGL((bins_locus_kernel<kBinsSlotsBig, kBinsMaxBig, kBinsThreadsBig>), grid, dim3(kBinsThreadsBig), 0, s, a);
      SB_TRY(hipGetLastError());
      SB_TRY(fetch_rows());
      SB_TRY(hipEventSynchronize(ev_rows));
      flags = flags_h[0];
   }
   if (bins_assign_wanted(steps.single_pass, d_hit_bin != nullptr, want_local, flags, nh)) {
      const std::vector<int32_t> todo = bins_assign_list(nb, nl);
      if (!todo.empty()) {
         SB_TRY(serve_list(todo));
         hipLaunchKernelGGL((bins_assign_kernel<kBinsSlotsMid, kBinsThreadsMid>), dim3((unsigned)std::min<int64_t>((int64_t)todo.size(), cap * 4)),
                            dim3(kBinsThreadsMid), 0, s, a);
         SB_TRY(hipGetLastError());
         SB_TRY(hipStreamSynchronize(s)); // (`todo` leaves scope)
      }
   }
   if (flags == kBinsFractional) {
      // fractional masses (multi-mapped reads): the bins stand, their masses are summed again in float, in the
      // order of the reference's std::set (bins_device.h)
      fixed_up = true;
      const std::vector<int32_t> all = bins_loci_where(nb, nl, [](int32_t) { return true; });
      SB_TRY(serve_list(all));
      SB_TRY(hipMemsetAsync(d + L.flag, 0, 4, s));
      hipLaunchKernelGGL(bins_ordered_mass_kernel, dim3((unsigned)std::min<int64_t>(nl, cap * 4)), dim3(256), 0, s, a);
      SB_TRY(hipGetLastError());
      SB_TRY(hipMemcpyAsync((void *)flags_h, d + L.flag, 8, hipMemcpyDeviceToHost, s));
      SB_TRY(hipStreamSynchronize(s));
      flags = flags_h[0];
   }
   if (flags) return api_fail(SBGPU_EUNSUPPORTED, bins_decline_reason(flags));
   stage("group kernel");
   return SBGPU_OK;
}

// The host's prefix sums while the middle runs, the caller's hook, the pairs' arena by the last call's size; then the
// middle's totals and flags
int BinsCall::finish_middle()
{
   rows = bins_rows(nb, nu, an->iso_off, nl);
   if (hooks && hooks->rows_known) hooks->rows_known(rows.row_off.data(), rows.f_off.data());
   const size_t hint = ctx_pairs_hint(c); // (none yet, or too small: fill_pairs)
   if (hint && dev_take(hint, &dp.arena, &dp.capacity) != hipSuccess) dp.arena = nullptr, dp.capacity = 0;
   if (!speculative || fixed_up) SB_TRY(launch_middle());
   SB_TRY(hipStreamSynchronize(s));
   const int32_t flags = flags_h[1];
   if (totals_h[0] != rows.row_off[(size_t)nl] || totals_h[1] != rows.f_off[(size_t)nl])
      return api_fail(SBGPU_EHIP, "sbgpu_bins_create_device: device and host prefix sums differ");
   if (flags & kBinsMassOverflow) return api_fail(SBGPU_EUNSUPPORTED, bins_decline_reason(kBinsMassOverflow)); // (bins_pack_kernel's: a finished total)
   if (flags & (kPairsNotUnder | kPairsForeignSegment))
      return api_fail(SBGPU_EUNSUPPORTED, "sbgpu_bins_create_device: a bin does not sit under an isoform it is compatible with; sbgpu_bins_create reports the details");
   stage("pack + pairs count");
   dp.any_wide = (flags & kPairsWide) != 0;
   dp.n_pairs = totals_h[2];
   dp.n_pair_segs = totals_h[3];
   return SBGPU_OK;
}

int BinsCall::fill_pairs()
{
   const PairsLayout Q = pairs_layout(dp.n_pairs, dp.n_pair_segs);
   dp.o_seg_off = Q.seg_off, dp.o_out_index = Q.out_index, dp.o_seg_lens = Q.seg_lens, dp.o_mask = Q.mask, dp.o_iso_len = Q.iso_len;
   if (Q.bytes > dp.capacity) {
      dev_give(dp.arena, dp.capacity);
      dp.arena = nullptr, dp.capacity = 0;
      const hipError_t e = dev_take(Q.bytes, &dp.arena, &dp.capacity);
      if (e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   }
   ctx_set_pairs_hint(c, Q.bytes);
   pa.pair_seg_off = (int64_t *)(dp.arena + dp.o_seg_off);
   pa.pair_seg_lens = (uint32_t *)(dp.arena + dp.o_seg_lens);
   pa.pair_mask = (uint32_t *)(dp.arena + dp.o_mask);
   pa.pair_iso_len = (int32_t *)(dp.arena + dp.o_iso_len);
   pa.pair_out_index = (int64_t *)(dp.arena + dp.o_out_index);
   ctx_stage_begin(c, "bins_pairs_kernel<fill>", s);
   if (any_wide_locus) hipLaunchKernelGGL(bins_pairs_kernel<true>, dim3(pgrid), dim3(256), 0, s, pa);
   hipLaunchKernelGGL(bins_pairs_locus_kernel<true>, dim3(lgrid), dim3(256), 0, s, pa, nl);
   ctx_stage_end(c, s);
   SB_TRY(hipGetLastError());
   stage("pairs fill launch");
   return SBGPU_OK;
}

// the caller's kernels behind the grouping (bin weights, EM) go into the stream, then the handle takes the two arenas over
int BinsCall::make_handle()
{
   if (want_local) *hooks->d_hit_bin_local = a.hit_bin_local;
   if (hooks && hooks->after_pairs) {
      const DeviceGrouping g = {rows.row_off.data(), rows.f_off.data(), rows.row_off[(size_t)nl], rows.f_off[(size_t)nl], (const int32_t *)(d2 + P.cnt), &dp};
      const int rc_after = hooks->after_pairs(g);
      if (rc_after != SBGPU_OK) return rc_after;
   }
   const DeviceBinArrays dba = {d2, d2_cap, P.cnt, P.key, P.cmp};
   const int rc = bins_from_groups(an, cw, kw, rows.row_off.data(), dba, rows.used, &dp, &iso_pre->len, out);
   if (rc == SBGPU_OK) d2 = nullptr, dp.arena = nullptr; // the handle's now
   stage("handle");
   return rc;
}
#undef SB_TRY
} // namespace

int bins_create_device_impl(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *dh, const float *d_mass,
                            const int64_t *locus_hit_off, int32_t compat_words, int32_t key_words, const uint32_t *d_compat,
                            const uint32_t *d_key, int64_t *d_hit_bin, void *stream, const IsoSegments *iso_pre, sbgpu_bins_t **out,
                            const uint64_t *d_span, const uint32_t *d_fhash, const GroupingHooks *hooks)
{
   BinsCall call = {c, an, dh, d_mass, locus_hit_off, compat_words, key_words, d_compat, d_key, d_hit_bin, (hipStream_t)stream, iso_pre, out, d_span, d_fhash, hooks};
   int rc = call.validate();
   if (rc == SBGPU_OK) rc = call.take_memory();
   if (rc == SBGPU_OK) call.fill_args();
   if (rc == SBGPU_OK) rc = call.upload_and_group();
   if (rc == SBGPU_OK) rc = call.fix_up();
   if (rc == SBGPU_OK) rc = call.finish_middle();
   if (rc == SBGPU_OK) rc = call.fill_pairs();
   if (rc == SBGPU_OK) rc = call.make_handle();
   return rc;
}
} // namespace sb

extern "C" {

int sbgpu_bins_create_device(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *dh, const float *d_mass,
                             const int64_t *locus_hit_off, int32_t compat_words, int32_t key_words, const uint32_t *d_compat,
                             const uint32_t *d_key, int64_t *d_hit_bin, void *stream, sbgpu_bins_t **out)
{
   return sb::bins_create_device_impl(c, an, dh, d_mass, locus_hit_off, compat_words, key_words, d_compat, d_key, d_hit_bin, stream,
                                      nullptr, out, nullptr, nullptr);
}

} // extern "C"
