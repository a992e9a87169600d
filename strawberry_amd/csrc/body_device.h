// strawberry_amd/csrc/body_device.h -- the transcript-body coverage profile (include/sbgpu.h: sbgpu_body_profile_device) from what a
// resident call leaves in HBM and the hits it was given.
//
//   (asg_column_kernel, assign_device.h, runs first: the live flag of every bin and the gain of every column.)
//   body_hit_kernel  one pass over the hits, a thread per hit; a work item is (locus, <= kBodyItemHits of its hits), as
//                    cov_hit_kernel's are, and the LDS plan is that kernel's.  The workgroup stages the locus' kept words and live
//                    flags in LDS and -- where the locus is within the three LDS limits below -- its gains, its isoforms' lengths
//                    and strands, and its exon table with every exon's prefix length (made on the host, once per call).  A hit
//                    recomputes its posterior (assign_rules.h), then walks its sorted features against every candidate's sorted
//                    exons (body_rules.h: body_walk) and adds w * n to the candidate's bins.  Those niso * P sums are kept in LDS
//                    (fp64 LDS atomics) where the tables are, and flushed once per item: plain stores when the locus is one item,
//                    one hardware fp64 global atomic per (isoform, bin) when it was split.  A narrow locus throws all of a wave's
//                    lanes at a handful of addresses, so its sums are kept in kBodyCopies copies, a lane adding to copy
//                    (lane % kBodyCopies), summed in ascending order in the flush (guide Guideline 12).  A locus beyond the LDS
//                    limits reads its tables from global memory and adds to global memory directly.
//                    The bin of a coordinate is body_rules.h's exact floor(t P / L): a 32-bit division where both operands fit
//                    (nearly every isoform), the 64-bit one otherwise; the walk divides once per bin it enters, not once per
//                    base.  A per-isoform boundary table in LDS was not built: at P = 100 it would cost 400 B per isoform, which
//                    is what the sums need.
//   body_iso_kernel  a thread per isoform: body_iso on its finished bins, and bases_p / total into the workgroup's partial class
//                    curves in LDS (fp64 LDS atomics; class_n by integer ones); one fp64 global atomic per (class, bin) and one
//                    integer one per class per workgroup at its end.  The order of those sums of non-negative terms is all that
//                    a launch's timing can change; class_n is exact.
//
// The LDS budget: three workgroups per CU, as cov_hit_kernel runs, leave 160 KiB / 3 = 53.3 KiB each.  The exon table of
// kBodyLdsExons = 1024 exons as coverage_device.h keeps it, with an 8-byte prefix per exon, is 16 KiB; the live flags and kept
// words 6 KiB; gains, exon offsets, lengths and strands of kBodyLdsIso = 256 isoforms 5.3 KiB.  That leaves 26 KiB for the sums:
// kBodyLdsSums = 3072 doubles (24 KiB).  So at P = 20 a locus of up to 153 isoforms keeps its sums in LDS, at P = 100 one of up to
// 30; sixteen copies fit a locus of up to 8 isoforms at P <= 24, and at P = 100 a single-isoform locus.  Reasoned, not tuned.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "body_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kBodyMaxBins = kStageMaxBins, kBodyMaxWords = kStageMaxWords, kBodyItemHits = kStageItemHits; // (stage_host.h)
constexpr int kBodyThreads = 256;
constexpr int kBodyLdsExons = 1024; // annotated exons of one locus up to which its exon table is kept in LDS
constexpr int kBodyLdsIso = 256;    // isoforms up to which the gains, exon offsets, lengths and strands are
constexpr int kBodyLdsSums = 3072;  // niso * P up to which the sums are
constexpr int kBodyNarrowIso = 8;   // isoforms up to which the sums are kept in copies, where niso * P * kBodyCopies <= kBodyLdsSums
constexpr int kBodyCopies = 16;
static_assert((kBodyCopies & (kBodyCopies - 1)) == 0, "a lane's copy is lane & (kBodyCopies - 1)");
static_assert(kBodyNarrowIso * kBodyCopies <= kBodyLdsSums, "the copies share the sums' LDS array");

struct BodyArgs {
   int64_t n_loci, n_items, n_iso;
   int32_t compat_words, n_pos;
   const HitItem *items;
   const int64_t *row_off, *iso_off, *f_off;   // [n_loci + 1]
   const int64_t *exon_off;                    // [n_iso + 1]
   const uint32_t *exon_left, *exon_right;     // [n_exon]
   const int64_t *exon_pre;                    // [n_exon] the length of the isoform's exons before this one
   const int64_t *iso_len;                     // [n_iso]
   const uint8_t *iso_strand;                  // [n_iso]
   const int32_t *hit_bin_local;               // [n_hits] rank of the hit's bin inside its locus, -1: none
   const uint32_t *compat;                     // [n_hits * compat_words]
   const int32_t *keep, *status;               // [n_iso], [n_loci]
   const double *F;                            // [n_elem]
   const float *hit_mass;                      // [n_hits], or null: 1.0 each
   const int64_t *feat_off;                    // [n_hits + 1]
   const uint8_t *feat_code;                   // [n_feat]
   const uint32_t *feat_left, *feat_right;
   const uint8_t *live;                        // [n_bins]  asg_column_kernel's
   const double *gain;                         // [n_iso]   asg_column_kernel's
   double *body_bases;                         // [n_iso * n_pos] zeroed per call
   double *class_profile;                      // [4 * n_pos]     zeroed per call
   unsigned long long *class_n;                // [4]             zeroed per call
   double *body_total, *body_center, *body_cv; // [n_iso]
};

__global__ __launch_bounds__(kBodyThreads) void body_hit_kernel(BodyArgs a)
{
   __shared__ double s_sum[kBodyLdsSums];
   __shared__ int64_t s_pre[kBodyLdsExons];
   __shared__ uint32_t s_left[kBodyLdsExons], s_right[kBodyLdsExons];
   __shared__ double s_g[kBodyLdsIso];
   __shared__ int64_t s_len[kBodyLdsIso];
   __shared__ int32_t s_eoff[kBodyLdsIso + 1];
   __shared__ uint8_t s_strand[kBodyLdsIso];
   __shared__ uint32_t s_keep[kBodyMaxWords];
   __shared__ uint8_t s_live[kBodyMaxBins];
   const int tid = threadIdx.x, cw = a.compat_words, P = a.n_pos;
   for (int64_t it = blockIdx.x; it < a.n_items; it += gridDim.x) {
      const HitItem item = a.items[it];
      const int64_t l = item.locus, b0 = a.row_off[l], i0 = a.iso_off[l], f0 = a.f_off[l];
      const int nb = (int)min((int64_t)kBodyMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      const int niso = (int)min((int64_t)32 * kBodyMaxWords, a.iso_off[l + 1] - i0);
      const int words = min((niso + 31) >> 5, cw);
      const int32_t st = a.status[l];
      const int64_t e0 = a.exon_off[i0], n_exon = a.exon_off[i0 + niso] - e0;
      const bool in_lds = niso <= kBodyLdsIso && n_exon <= kBodyLdsExons && niso * P <= kBodyLdsSums;
      const int nsum = in_lds ? niso * P : 0;
      const int copies = in_lds && niso <= kBodyNarrowIso && nsum * kBodyCopies <= kBodyLdsSums ? kBodyCopies : 1;
      for (int w = tid; w < words; w += kBodyThreads) s_keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      for (int b = tid; b < nb; b += kBodyThreads) s_live[b] = a.live[b0 + b];
      if (in_lds) {
         for (int j = tid; j < niso; j += kBodyThreads) s_g[j] = a.gain[i0 + j], s_len[j] = a.iso_len[i0 + j], s_strand[j] = a.iso_strand[i0 + j];
         for (int j = tid; j <= niso; j += kBodyThreads) s_eoff[j] = (int32_t)(a.exon_off[i0 + j] - e0);
         for (int e = tid; e < (int)n_exon; e += kBodyThreads) s_left[e] = a.exon_left[e0 + e], s_right[e] = a.exon_right[e0 + e], s_pre[e] = a.exon_pre[e0 + e];
         for (int i = tid; i < nsum * copies; i += kBodyThreads) s_sum[i] = 0.0;
      }
      __syncthreads();
      const int copy = tid & (copies - 1);
      for (int64_t h = item.h0 + tid; h < item.h1; h += kBodyThreads) {
         const int lb = a.hit_bin_local[h];
         const uint32_t *C = a.compat + h * cw;
         const double *row = lb >= 0 && lb < nb && s_live[lb] ? a.F + f0 + (int64_t)lb * niso : nullptr;
         const int64_t q0 = a.feat_off[h];
         const int nf = (int)(a.feat_off[h + 1] - q0);
         const uint8_t *code = a.feat_code + q0;
         const uint32_t *fl = a.feat_left + q0, *fr = a.feat_right + q0;
         const double m = a.hit_mass ? (double)a.hit_mass[h] : 1.0;
         if (in_lds) {
            const AsgHit r = asg_hit_map(C, s_keep, words, s_g, row);
            if (r.map_iso < 0) continue;
            for (int w = 0; w < words; ++w)
               for (uint32_t bits = C[w] & s_keep[w]; bits; bits &= bits - 1) {
                  const int j = 32 * w + __builtin_ctz(bits);
                  const int le0 = s_eoff[j], strand = s_strand[j];
                  body_walk(code, fl, fr, nf, s_left + le0, s_right + le0, s_pre + le0, s_eoff[j + 1] - le0, s_len[j], P,
                            cov_weight(m, asg_posterior(s_g[j], row[j], r.den)),
                            [&](int q, double x) { unsafeAtomicAdd(&s_sum[(j * P + body_report(q, P, strand)) * copies + copy], x); });
               }
         } else {
            const double *G = a.gain + i0;
            const AsgHit r = asg_hit_map(C, s_keep, words, G, row);
            if (r.map_iso < 0) continue;
            for (int w = 0; w < words; ++w)
               for (uint32_t bits = C[w] & s_keep[w]; bits; bits &= bits - 1) {
                  const int j = 32 * w + __builtin_ctz(bits);
                  const int64_t ge0 = a.exon_off[i0 + j];
                  const int strand = a.iso_strand[i0 + j];
                  double *mine = a.body_bases + (i0 + j) * P;
                  body_walk(code, fl, fr, nf, a.exon_left + ge0, a.exon_right + ge0, a.exon_pre + ge0, (int)(a.exon_off[i0 + j + 1] - ge0), a.iso_len[i0 + j],
                            P, cov_weight(m, asg_posterior(G[j], row[j], r.den)),
                            [&](int q, double x) { unsafeAtomicAdd(&mine[body_report(q, P, strand)], x); });
               }
         }
      }
      __syncthreads();
      for (int i = tid; i < nsum; i += kBodyThreads) {
         double x = 0.0;
         for (int k = 0; k < copies; ++k) x += s_sum[i * copies + k];
         if (item.split) {
            if (x != 0.0) unsafeAtomicAdd(&a.body_bases[i0 * P + i], x);
         } else {
            a.body_bases[i0 * P + i] = x;
         }
      }
      __syncthreads();
   }
}

__global__ __launch_bounds__(kBodyThreads) void body_iso_kernel(BodyArgs a)
{
   __shared__ double s_class[4 * kBodyMaxPos];
   __shared__ unsigned long long s_n[4];
   const int tid = threadIdx.x, P = a.n_pos;
   for (int i = tid; i < 4 * P; i += kBodyThreads) s_class[i] = 0.0;
   if (tid < 4) s_n[tid] = 0ull;
   __syncthreads();
   for (int64_t i = (int64_t)blockIdx.x * kBodyThreads + tid; i < a.n_iso; i += (int64_t)gridDim.x * kBodyThreads) {
      const double *mine = a.body_bases + i * P;
      const int64_t L = a.iso_len[i];
      const BodyIso o = body_iso(mine, P, L, a.iso_strand[i]);
      a.body_total[i] = o.total, a.body_center[i] = o.center, a.body_cv[i] = o.cv;
      if (!(o.total > 0.0)) continue;
      const int c = body_class(L);
      for (int p = 0; p < P; ++p) {
         const double x = mine[p] / o.total;
         if (x != 0.0) unsafeAtomicAdd(&s_class[c * P + p], x);
      }
      atomicAdd(&s_n[c], 1ull);
   }
   __syncthreads();
   for (int i = tid; i < 4 * P; i += kBodyThreads)
      if (s_class[i] != 0.0) unsafeAtomicAdd(&a.class_profile[i], s_class[i]);
   if (tid < 4 && s_n[tid]) atomicAdd(&a.class_n[tid], s_n[tid]);
}

} // namespace sb
