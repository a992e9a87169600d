// strawberry_amd/csrc/assign_device.h -- the fragment assignment (include/sbgpu.h: sbgpu_fragment_assign_device) from what a
// resident call leaves in HBM.
//
//   asg_column_kernel  one workgroup per locus, one pass over F: the live flag of every bin (a thread per bin), then the gain
//                      g_j = theta_j / c_j of every column (a thread per column: the column's sum runs over the live bins in
//                      ascending order, sequentially, so its bits are the host form's; neighbouring threads read neighbouring
//                      columns of row-major F).  A locus of at most kAsgStage weights is staged in LDS first (coalesced), so
//                      that the sequential sums of a narrow locus wait for LDS, not for L2.
//   asg_hit_kernel     one pass over the hits, a thread per hit.  A work item is (locus, <= kAsgItemHits of its hits), made
//                      as ctx_count_kernel's are; the workgroup stages the locus' gains, kept words and live flags in LDS.
//                      A hit walks the set bits of compat & kept twice: the denominator and the argmax, then the posterior
//                      terms.  The three per-isoform sums are kept in LDS (fp64 LDS atomics) where the locus has at most
//                      kAsgLdsIso isoforms and flushed once per item: plain stores when the locus is one item, hardware fp64
//                      global atomics when it was split.  A locus of at most kAsgNarrow isoforms throws all of a wave's
//                      lanes at a handful of addresses, so its sums are kept in kAsgCopies copies, a lane adding to copy
//                      (lane % kAsgCopies): two lanes per address instead of 64, and the copies are summed in the flush --
//                      before the one global atomic per isoform (guide Guideline 12).  A wider locus adds to global memory
//                      directly.
//
// The decisions themselves are assign_rules.h's, shared with the host form.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kAsgMaxBins = kStageMaxBins, kAsgMaxWords = kStageMaxWords, kAsgItemHits = kStageItemHits; // (stage_host.h)
constexpr int kAsgThreads = 256;
constexpr int kAsgStage = 4096;    // weights of one locus staged in LDS by the column pass (32 KB)
constexpr int kAsgLdsIso = 1024;   // isoforms up to which the hit pass keeps gains and sums in LDS (4 x 8 KB)
constexpr int kAsgNarrow = 8;      // isoforms up to which the sums are kept in copies
constexpr int kAsgCopies = 32;     // kAsgNarrow * kAsgCopies <= kAsgLdsIso

struct AsgArgs {
   int64_t n_loci, n_items;
   int32_t compat_words;
   const HitItem *items;
   const int64_t *locus_hit_off, *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int32_t *hit_bin_local;  // [n_hits] rank of the hit's bin inside its locus, -1: none
   const uint32_t *compat;        // [n_hits * compat_words]
   const int32_t *keep, *status;  // [n_iso], [n_loci]
   const double *F;               // [n_elem]
   const double *theta;           // [n_iso]
   const float *hit_mass;         // [n_hits], or null: 1.0 each
   uint8_t *live;                 // [n_bins]
   double *gain;                  // [n_iso]
   int32_t *map_iso, *n_cand;     // [n_hits]
   double *map_prob;              // [n_hits]
   double *unique_mass, *map_mass, *post_mass; // [n_iso] zeroed per call
   unsigned long long *unassigned;             // [n_loci] zeroed per call (int64 to the caller)
};

__global__ __launch_bounds__(kAsgThreads) void asg_column_kernel(AsgArgs a)
{
   __shared__ double s_F[kAsgStage];
   __shared__ uint8_t s_live[kAsgMaxBins];
   __shared__ uint32_t s_keep[kAsgMaxWords];
   const int tid = threadIdx.x;
   for (int64_t l = blockIdx.x; l < a.n_loci; l += gridDim.x) {
      const int64_t b0 = a.row_off[l], i0 = a.iso_off[l], f0 = a.f_off[l];
      const int nb = (int)min((int64_t)kAsgMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      const int niso = (int)min((int64_t)32 * kAsgMaxWords, a.iso_off[l + 1] - i0);
      const int words = (niso + 31) >> 5;
      const int32_t st = a.status[l];
      for (int w = tid; w < words; w += kAsgThreads) s_keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      const double *Fl = a.F + f0;
      const int n_val = nb * niso; // (<= 5632 * 4096: fits an int)
      if (n_val <= kAsgStage) {
         for (int i = tid; i < n_val; i += kAsgThreads) s_F[i] = Fl[i];
         Fl = s_F;
      }
      __syncthreads();
      for (int b = tid; b < nb; b += kAsgThreads) {
         const uint8_t v = asg_row_live(Fl + (int64_t)b * niso, niso);
         s_live[b] = v;
         a.live[b0 + b] = v;
      }
      __syncthreads();
      for (int j = tid; j < niso; j += kAsgThreads) {
         double c = 0.0;
         for (int b = 0; b < nb; ++b)
            if (s_live[b]) c += Fl[(int64_t)b * niso + j];
         a.gain[i0 + j] = asg_gain(a.theta[i0 + j], c, (s_keep[j >> 5] >> (j & 31)) & 1u);
      }
      __syncthreads();
   }
}

__global__ __launch_bounds__(kAsgThreads) void asg_hit_kernel(AsgArgs a)
{
   __shared__ double s_g[kAsgLdsIso];
   __shared__ double s_uniq[kAsgLdsIso], s_map[kAsgLdsIso], s_post[kAsgLdsIso];
   __shared__ uint32_t s_keep[kAsgMaxWords];
   __shared__ uint8_t s_live[kAsgMaxBins];
   __shared__ unsigned int s_unassigned;
   const int tid = threadIdx.x, cw = a.compat_words;
   for (int64_t it = blockIdx.x; it < a.n_items; it += gridDim.x) {
      const HitItem item = a.items[it];
      const int64_t l = item.locus, b0 = a.row_off[l], i0 = a.iso_off[l], f0 = a.f_off[l];
      const int nb = (int)min((int64_t)kAsgMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      const int niso = (int)min((int64_t)32 * kAsgMaxWords, a.iso_off[l + 1] - i0);
      const int words = min((niso + 31) >> 5, cw);
      const int32_t st = a.status[l];
      const bool in_lds = niso <= kAsgLdsIso;
      const int copies = niso <= kAsgNarrow ? kAsgCopies : 1;
      const int n_slots = in_lds ? niso * copies : 0;
      for (int w = tid; w < words; w += kAsgThreads) s_keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      for (int b = tid; b < nb; b += kAsgThreads) s_live[b] = a.live[b0 + b];
      if (in_lds)
         for (int j = tid; j < niso; j += kAsgThreads) s_g[j] = a.gain[i0 + j];
      for (int i = tid; i < n_slots; i += kAsgThreads) s_uniq[i] = 0.0, s_map[i] = 0.0, s_post[i] = 0.0;
      if (tid == 0) s_unassigned = 0u;
      __syncthreads();
      const double *G = in_lds ? s_g : a.gain + i0;
      const int copy = tid & (copies - 1);
      for (int64_t h = item.h0 + tid; h < item.h1; h += kAsgThreads) {
         const int lb = a.hit_bin_local[h];
         const uint32_t *C = a.compat + h * cw;
         const double *row = lb >= 0 && lb < nb && s_live[lb] ? a.F + f0 + (int64_t)lb * niso : nullptr;
         const AsgHit r = asg_hit_map(C, s_keep, words, G, row);
         a.n_cand[h] = r.n_cand;
         a.map_iso[h] = r.map_iso;
         a.map_prob[h] = r.map_prob;
         if (r.map_iso < 0) {
            atomicAdd(&s_unassigned, 1u);
            continue;
         }
         const double m = a.hit_mass ? (double)a.hit_mass[h] : 1.0;
         if (in_lds) {
            unsafeAtomicAdd(&s_map[r.map_iso * copies + copy], m);
            if (r.n_cand == 1) unsafeAtomicAdd(&s_uniq[r.map_iso * copies + copy], m);
         } else {
            unsafeAtomicAdd(&a.map_mass[i0 + r.map_iso], m);
            if (r.n_cand == 1) unsafeAtomicAdd(&a.unique_mass[i0 + r.map_iso], m);
         }
         for (int w = 0; w < words; ++w)
            for (uint32_t bits = C[w] & s_keep[w]; bits; bits &= bits - 1) {
               const int j = 32 * w + __builtin_ctz(bits);
               const double v = m * asg_posterior(G[j], row[j], r.den);
               if (in_lds) unsafeAtomicAdd(&s_post[j * copies + copy], v);
               else unsafeAtomicAdd(&a.post_mass[i0 + j], v);
            }
      }
      __syncthreads();
      if (in_lds)
         for (int j = tid; j < niso; j += kAsgThreads) {
            double u = 0.0, mp = 0.0, p = 0.0;
            for (int k = 0; k < copies; ++k) u += s_uniq[j * copies + k], mp += s_map[j * copies + k], p += s_post[j * copies + k];
            if (item.split) {
               if (u != 0.0) unsafeAtomicAdd(&a.unique_mass[i0 + j], u);
               if (mp != 0.0) unsafeAtomicAdd(&a.map_mass[i0 + j], mp);
               if (p != 0.0) unsafeAtomicAdd(&a.post_mass[i0 + j], p);
            } else {
               a.unique_mass[i0 + j] = u, a.map_mass[i0 + j] = mp, a.post_mass[i0 + j] = p;
            }
         }
      if (tid == 0) {
         if (item.split) atomicAdd(&a.unassigned[l], (unsigned long long)s_unassigned);
         else a.unassigned[l] = s_unassigned;
      }
      __syncthreads();
   }
}

} // namespace sb
