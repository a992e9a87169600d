// strawberry_amd/csrc/splice_device.h -- the kernels of the splicing events' PSI (include/sbgpu.h: sbgpu_splice_psi_device,
// sbgpu_splice_support_device).  Included by splice_api.hip alone.  Both are one thread per event; the sums and the
// quotient are splice_rules.h's, which the host form calls too.
//   spl_psi_kernel      the row loop runs inside the thread: defined_count is a register, no atomic, no second pass.  The stores
//                       of psi[k][u] are coalesced across a wave; neighbouring lanes are neighbouring events of one locus, so
//                       their loads of x[k][j] hit the same or adjacent addresses.  A locus of at most kSplMaskIso isoforms
//                       builds the event's span and inclusion sets once, as two 64-bit masks, and then makes one ascending pass
//                       over the set bits for kSplRows rows at a time (per row the rule's sums in the rule's order); a wider
//                       locus re-tests the extents and walks the list row by row.
//   spl_support_kernel  a gather-sum over the inclusion list in list order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "splice_rules.h"

namespace sb {

constexpr int kSplThreads = 256;
constexpr int kSplRows = 4; // rows a thread of the mask path takes at once: their loads are independent, so this many are in flight

struct SplArgs {
   int64_t n_events, n_iso, n_rows;
   const int32_t *event_locus;
   const uint8_t *event_kind;
   const uint32_t *event_left, *event_right;
   const int64_t *incl_off;
   const int32_t *incl_iso;
   const int64_t *incl_exon;
   const int64_t *iso_off;
   const uint32_t *iso_left, *iso_right;
   const double *x;        // [n_rows][n_iso]
   const int32_t *keep;    // [n_rows][n_iso], or null
   double *psi;            // [n_rows][n_events]
   int32_t *defined_count; // [n_events], or null
   const double *exon_bases, *junction_mass; // [n_exons], or null
   double *support;        // [n_events]
};

__global__ __launch_bounds__(kSplThreads) void spl_psi_kernel(SplArgs a)
{
   const int64_t u = (int64_t)blockIdx.x * kSplThreads + threadIdx.x;
   if (u >= a.n_events) return;
   const int64_t l = a.event_locus[u];
   const int64_t j0 = a.iso_off[l], niso = a.iso_off[l + 1] - j0;
   const int64_t i0 = a.incl_off[u], n_incl = a.incl_off[u + 1] - i0;
   const uint32_t ea = a.event_left[u], eb = a.event_right[u];
   const uint32_t *left = a.iso_left + j0, *right = a.iso_right + j0;
   const int32_t *incl = a.incl_iso + i0;
   const double *x = a.x + j0;
   const int32_t *keep = a.keep ? a.keep + j0 : nullptr;
   double *psi = a.psi + u;
   int32_t defined = 0;
   if (niso <= kSplMaskIso) {
      const uint64_t span = spl_span_mask(left, right, (int)niso, ea, eb), in = spl_incl_mask(incl, n_incl);
      const int64_t step = a.n_iso;
      int64_t k = 0;
      for (; k + kSplRows <= a.n_rows; k += kSplRows, x += kSplRows * step, keep = keep ? keep + kSplRows * step : nullptr) {
         SplPsi r[kSplRows];
         spl_psi_rows_masks<kSplRows>(x, keep, step, span, in, r);
#pragma unroll
         for (int i = 0; i < kSplRows; ++i, psi += a.n_events) {
            *psi = r[i].psi;
            defined += r[i].defined;
         }
      }
      for (; k < a.n_rows; ++k, x += step, psi += a.n_events, keep = keep ? keep + step : nullptr) {
         SplPsi r;
         spl_psi_rows_masks<1>(x, keep, step, span, in, &r);
         *psi = r.psi;
         defined += r.defined;
      }
   } else {
      for (int64_t k = 0; k < a.n_rows; ++k, x += a.n_iso, psi += a.n_events) {
         const SplPsi r = spl_psi_row(x, keep, left, right, niso, ea, eb, incl, n_incl);
         if (keep) keep += a.n_iso;
         *psi = r.psi;
         defined += r.defined;
      }
   }
   if (a.defined_count) a.defined_count[u] = defined;
}

__global__ __launch_bounds__(kSplThreads) void spl_support_kernel(SplArgs a)
{
   const int64_t u = (int64_t)blockIdx.x * kSplThreads + threadIdx.x;
   if (u >= a.n_events) return;
   const int64_t i0 = a.incl_off[u];
   a.support[u] = spl_support(a.event_kind[u] == kSplExon ? a.exon_bases : a.junction_mass, a.incl_exon + i0, a.incl_off[u + 1] - i0);
}

} // namespace sb
