// strawberry_amd/csrc/coverage_device.h -- the isoform-resolved coverage (include/sbgpu.h: sbgpu_isoform_coverage_device) from
// what a resident call leaves in HBM and the hits it was given.
//
//   (asg_column_kernel, assign_device.h, runs first: the live flag of every bin and the gain of every column.)
//   cov_hit_kernel   one pass over the hits, a thread per hit; a work item is (locus, <= kCovItemHits of its hits), as
//                    asg_hit_kernel's are.  The workgroup stages the locus' gains, kept words and live flags in LDS and -- where
//                    the locus has at most kCovLdsExons annotated exons -- its exon table: the isoforms'
//                    exon offsets inside the locus, lefts and rights.  A hit recomputes its posterior (assign_rules.h), then walks
//                    its sorted features against every candidate's sorted exons (coverage_rules.h: cov_walk, one forward merge per
//                    pair) and adds to the exons' bases and the junctions' mass.  Those sums are kept in LDS (fp64 LDS atomics)
//                    where the exon table is, and flushed once per item: plain stores when the locus is one item, one hardware
//                    fp64 global atomic per exon when it was split.  A locus of at most kCovNarrowIso isoforms and kCovCopyExons
//                    exons throws all of a wave's lanes at a handful of addresses, so its sums are kept in kCovCopies copies, a
//                    lane adding to copy (lane % kCovCopies), and the copies are summed in ascending order in the flush -- before
//                    the one store or atomic per exon (guide Guideline 12).  A locus beyond the LDS limits reads its exon table
//                    from global memory and adds to global memory directly.  The bases of the unassigned hits are one LDS sum
//                    per item.
//   cov_iso_kernel   a thread per isoform: the finished exon sums in ascending order.
//
// The decisions themselves are assign_rules.h's and coverage_rules.h's, shared with the host form.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coverage_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kCovMaxBins = kStageMaxBins, kCovMaxWords = kStageMaxWords, kCovItemHits = kStageItemHits; // (stage_host.h)
constexpr int kCovThreads = 256;
constexpr int kCovLdsExons = 1024;  // annotated exons of one locus up to which the exon table and the sums are kept in LDS (2 x 4 KB + 2 x 8 KB)
// Not a threshold of its own: an isoform owns at least one exon, so a locus of at most kCovLdsExons exons has at most as many
// isoforms.  It sizes the gains and the exon offsets in LDS (8 KB + 4 KB); the kernel tests it too, only so that an annotation
// with exon-less isoforms cannot overrun those arrays (such a locus takes the global path).
constexpr int kCovLdsIso = kCovLdsExons;
constexpr int kCovNarrowIso = 8;    // isoforms up to which the sums are kept in copies ...
constexpr int kCovCopyExons = 64;   // ... where the locus has at most this many annotated exons
constexpr int kCovCopies = 16;      // kCovCopyExons * kCovCopies <= kCovLdsExons
static_assert(kCovCopyExons * kCovCopies <= kCovLdsExons, "the copies share the sums' LDS arrays");
static_assert((kCovCopies & (kCovCopies - 1)) == 0, "a lane's copy is lane & (kCovCopies - 1)");

struct CovArgs {
   int64_t n_loci, n_items, n_iso;
   int32_t compat_words;
   const HitItem *items;
   const int64_t *row_off, *iso_off, *f_off;   // [n_loci + 1]
   const int64_t *exon_off;                    // [n_iso + 1]
   const uint32_t *exon_left, *exon_right;     // [n_exon]
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
   double *exon_bases, *junction_mass;         // [n_exon] zeroed per call
   double *unexplained_bases;                  // [n_loci] zeroed per call
   double *iso_bases;                          // [n_iso]
};

__global__ __launch_bounds__(kCovThreads) void cov_hit_kernel(CovArgs a)
{
   __shared__ double s_g[kCovLdsIso];
   __shared__ double s_bases[kCovLdsExons], s_junc[kCovLdsExons];
   __shared__ uint32_t s_left[kCovLdsExons], s_right[kCovLdsExons];
   __shared__ int32_t s_eoff[kCovLdsIso + 1];
   __shared__ uint32_t s_keep[kCovMaxWords];
   __shared__ uint8_t s_live[kCovMaxBins];
   __shared__ double s_unexplained;
   const int tid = threadIdx.x, cw = a.compat_words;
   for (int64_t it = blockIdx.x; it < a.n_items; it += gridDim.x) {
      const HitItem item = a.items[it];
      const int64_t l = item.locus, b0 = a.row_off[l], i0 = a.iso_off[l], f0 = a.f_off[l];
      const int nb = (int)min((int64_t)kCovMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      const int niso = (int)min((int64_t)32 * kCovMaxWords, a.iso_off[l + 1] - i0);
      const int words = min((niso + 31) >> 5, cw);
      const int32_t st = a.status[l];
      const int64_t e0 = a.exon_off[i0], n_exon = a.exon_off[i0 + niso] - e0;
      const bool in_lds = niso <= kCovLdsIso && n_exon <= kCovLdsExons;
      const int nex = in_lds ? (int)n_exon : 0;
      const int copies = in_lds && niso <= kCovNarrowIso && nex <= kCovCopyExons ? kCovCopies : 1;
      for (int w = tid; w < words; w += kCovThreads) s_keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      for (int b = tid; b < nb; b += kCovThreads) s_live[b] = a.live[b0 + b];
      if (in_lds) {
         for (int j = tid; j < niso; j += kCovThreads) s_g[j] = a.gain[i0 + j];
         for (int j = tid; j <= niso; j += kCovThreads) s_eoff[j] = (int32_t)(a.exon_off[i0 + j] - e0);
         for (int e = tid; e < nex; e += kCovThreads) s_left[e] = a.exon_left[e0 + e], s_right[e] = a.exon_right[e0 + e];
         for (int i = tid; i < nex * copies; i += kCovThreads) s_bases[i] = 0.0, s_junc[i] = 0.0;
      }
      if (tid == 0) s_unexplained = 0.0;
      __syncthreads();
      const int copy = tid & (copies - 1);
      for (int64_t h = item.h0 + tid; h < item.h1; h += kCovThreads) {
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
            if (r.map_iso < 0) {
               unsafeAtomicAdd(&s_unexplained, m * (double)cov_matchlen(code, fl, fr, nf));
               continue;
            }
            for (int w = 0; w < words; ++w)
               for (uint32_t bits = C[w] & s_keep[w]; bits; bits &= bits - 1) {
                  const int j = 32 * w + __builtin_ctz(bits);
                  const int le0 = s_eoff[j];
                  cov_walk(
                     code, fl, fr, nf, s_left + le0, s_right + le0, s_eoff[j + 1] - le0, cov_weight(m, asg_posterior(s_g[j], row[j], r.den)),
                     [&](int e, double x) { unsafeAtomicAdd(&s_bases[(le0 + e) * copies + copy], x); },
                     [&](int e, double x) { unsafeAtomicAdd(&s_junc[(le0 + e) * copies + copy], x); });
               }
         } else {
            const double *G = a.gain + i0;
            const AsgHit r = asg_hit_map(C, s_keep, words, G, row);
            if (r.map_iso < 0) {
               unsafeAtomicAdd(&s_unexplained, m * (double)cov_matchlen(code, fl, fr, nf));
               continue;
            }
            for (int w = 0; w < words; ++w)
               for (uint32_t bits = C[w] & s_keep[w]; bits; bits &= bits - 1) {
                  const int j = 32 * w + __builtin_ctz(bits);
                  const int64_t ge0 = a.exon_off[i0 + j];
                  cov_walk(
                     code, fl, fr, nf, a.exon_left + ge0, a.exon_right + ge0, (int)(a.exon_off[i0 + j + 1] - ge0),
                     cov_weight(m, asg_posterior(G[j], row[j], r.den)), [&](int e, double x) { unsafeAtomicAdd(&a.exon_bases[ge0 + e], x); },
                     [&](int e, double x) { unsafeAtomicAdd(&a.junction_mass[ge0 + e], x); });
               }
         }
      }
      __syncthreads();
      for (int e = tid; e < nex; e += kCovThreads) {
         double x = 0.0, y = 0.0;
         for (int k = 0; k < copies; ++k) x += s_bases[e * copies + k], y += s_junc[e * copies + k];
         if (item.split) {
            if (x != 0.0) unsafeAtomicAdd(&a.exon_bases[e0 + e], x);
            if (y != 0.0) unsafeAtomicAdd(&a.junction_mass[e0 + e], y);
         } else {
            a.exon_bases[e0 + e] = x, a.junction_mass[e0 + e] = y;
         }
      }
      if (tid == 0) {
         if (item.split) {
            if (s_unexplained != 0.0) unsafeAtomicAdd(&a.unexplained_bases[l], s_unexplained);
         } else {
            a.unexplained_bases[l] = s_unexplained;
         }
      }
      __syncthreads();
   }
}

__global__ __launch_bounds__(kCovThreads) void cov_iso_kernel(CovArgs a)
{
   for (int64_t i = (int64_t)blockIdx.x * kCovThreads + threadIdx.x; i < a.n_iso; i += (int64_t)gridDim.x * kCovThreads)
      a.iso_bases[i] = cov_iso_bases(a.exon_bases, a.exon_off[i], a.exon_off[i + 1]);
}

} // namespace sb
