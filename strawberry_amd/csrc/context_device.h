// strawberry_amd/csrc/context_device.h -- the `-f` fragment-context table (Sample::printContext,
// /root/reference/src/alignments.cpp:1549-1639) from what a resident call leaves in HBM.
//
//   ctx_count_kernel   one pass over the hits: per bin, how many hits qualify and which is the last of them.
//                      A work item is (locus, range of its hits); the workgroup keeps its locus' two per-bin arrays in LDS
//                      (LDS atomics), then flushes the bins that were hit: plain stores when the locus is one item,
//                      integer global atomics when it was split.  All integers: any order gives the same bits.
//   ctx_rows_kernel    rows (bins with a qualifying hit) and qualifying hits per locus, one wave per locus
//   ctx_scan_kernel    the rows per locus -> locus_row_off (one workgroup: a sample has 10^4 .. 10^5 loci)
//   ctx_order_kernel   one workgroup per locus: ranks the locus' bins by the comparator of context_rules.h -- all pairs
//                      for small loci, a bitonic sort of the bin indices in LDS for the others -- and writes the rows
//                      (the ranked bins that were hit) behind each other
//   ctx_gather_kernel  one workgroup per locus (a wide locus has 10^6 elements): the rows' probabilities from F and the last hit's compat words
//
// The decisions themselves (who qualifies, which column gets the weight, the order) are context_rules.h's, shared with
// the host form.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kCtxMaxBins = kStageMaxBins, kCtxMaxWords = kStageMaxWords, kCtxItemHits = kStageItemHits; // (stage_host.h)
constexpr int kCtxThreads = 256;
constexpr int kCtxAllPairs = 256;     // bins up to which a locus is ranked by all-pairs counting
constexpr int kCtxSortSlots = 8192;   // >= kCtxMaxBins, a power of two
constexpr int kCtxKeyStage = 4096;    // key words of a locus staged in LDS where they fit (else read through the L2)

struct CtxArgs {
   int64_t n_loci, n_items;
   int32_t compat_words, key_words;
   const HitItem *items;
   const int64_t *locus_hit_off, *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int32_t *hit_bin_local;  // [n_hits] rank of the hit's bin inside its locus, -1: none
   const uint32_t *compat;        // [n_hits * compat_words]
   const int32_t *keep, *status;  // [n_iso], [n_loci]
   const uint32_t *bin_key;       // [n_bins * key_words]
   const double *F;               // [n_elem]
   uint32_t *n_in_bin;            // [n_bins] zeroed per call
   int32_t *last_hit;             // [n_bins] -1 per call; the last qualifying hit, counted from the locus' first hit
   int32_t *n_rows;               // [n_loci]
   const int64_t *locus_row_off;  // [n_loci + 1] (the scan of n_rows)
   uint32_t *locus_hits;          // [n_loci]
   int64_t *row_bin;              // [n_rows]
   uint32_t *row_hits;            // [n_rows]
   int64_t *row_last;             // [n_rows] the row's last qualifying hit (global index)
   double *row_prob;              // [n_elem]
};

__global__ __launch_bounds__(kCtxThreads) void ctx_count_kernel(CtxArgs a)
{
   __shared__ uint32_t s_n[kCtxMaxBins];
   __shared__ int32_t s_last[kCtxMaxBins];
   __shared__ uint32_t s_keep[kCtxMaxWords];
   const int tid = threadIdx.x, cw = a.compat_words;
   for (int64_t it = blockIdx.x; it < a.n_items; it += gridDim.x) {
      const HitItem item = a.items[it];
      const int64_t l = item.locus, b0 = a.row_off[l], q0 = a.locus_hit_off[l], i0 = a.iso_off[l];
      const int nb = (int)min((int64_t)kCtxMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      const int niso = (int)(a.iso_off[l + 1] - i0);
      const int words = min(min((niso + 31) >> 5, cw), kCtxMaxWords);
      const int32_t st = a.status[l];
      for (int w = tid; w < words; w += kCtxThreads) s_keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      for (int b = tid; b < nb; b += kCtxThreads) s_n[b] = 0u, s_last[b] = -1;
      __syncthreads();
      for (int64_t h = item.h0 + tid; h < item.h1; h += kCtxThreads) {
         const int lb = a.hit_bin_local[h];
         if (lb >= 0 && lb < nb && ctx_hit_qualifies(a.compat + h * cw, s_keep, words)) {
            atomicAdd(&s_n[lb], 1u);
            atomicMax(&s_last[lb], (int32_t)(h - q0));
         }
      }
      __syncthreads();
      for (int b = tid; b < nb; b += kCtxThreads) {
         const uint32_t n = s_n[b];
         if (!n) continue;
         if (item.split) {
            atomicAdd(&a.n_in_bin[b0 + b], n);
            atomicMax(&a.last_hit[b0 + b], s_last[b]);
         } else {
            a.n_in_bin[b0 + b] = n;
            a.last_hit[b0 + b] = s_last[b];
         }
      }
      __syncthreads();
   }
}

// rows and qualifying hits per locus; gene_frag_count is summed in uint as the reference does (wraps at 2^32)
__global__ __launch_bounds__(kCtxThreads) void ctx_rows_kernel(CtxArgs a)
{
   const int lane = threadIdx.x & 63;
   const int64_t wave = ((int64_t)blockIdx.x * kCtxThreads + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * kCtxThreads) >> 6;
   for (int64_t l = wave; l < a.n_loci; l += n_waves) {
      const int64_t b0 = a.row_off[l], b1 = a.row_off[l + 1];
      uint32_t rows = 0, hits = 0;
      for (int64_t b = b0 + lane; b < b1; b += 64) {
         const uint32_t n = a.n_in_bin[b];
         rows += n != 0;
         hits += n;
      }
      for (int d = 32; d; d >>= 1) rows += __shfl_xor(rows, d, 64), hits += __shfl_xor(hits, d, 64);
      if (lane == 0) a.n_rows[l] = (int32_t)rows, a.locus_hits[l] = hits;
   }
}

// exclusive scan of n_rows over the loci, 4096 per round: four consecutive loci per lane, the lanes' sums through LDS
constexpr int kCtxScanThreads = 1024;
__global__ __launch_bounds__(kCtxScanThreads) void ctx_scan_kernel(CtxArgs a, int64_t *locus_row_off, int64_t *total)
{
   __shared__ int64_t s_sum[kCtxScanThreads];
   const int t = threadIdx.x;
   int64_t base = 0;
   for (int64_t c0 = 0; c0 < a.n_loci; c0 += 4 * kCtxScanThreads) {
      const int64_t i0 = c0 + 4 * (int64_t)t;
      int64_t v[4], own = 0;
      for (int k = 0; k < 4; ++k) v[k] = i0 + k < a.n_loci ? a.n_rows[i0 + k] : 0, own += v[k];
      s_sum[t] = own;
      __syncthreads();
      for (int d = 1; d < kCtxScanThreads; d <<= 1) {
         const int64_t x = t >= d ? s_sum[t - d] : 0;
         __syncthreads();
         s_sum[t] += x;
         __syncthreads();
      }
      int64_t r = base + s_sum[t] - own;
      for (int k = 0; k < 4; ++k)
         if (i0 + k < a.n_loci) locus_row_off[i0 + k] = r, r += v[k];
      base += s_sum[kCtxScanThreads - 1];
      __syncthreads();
   }
   if (t == 0) locus_row_off[a.n_loci] = base, *total = base;
}

__global__ __launch_bounds__(kCtxThreads) void ctx_order_kernel(CtxArgs a)
{
   __shared__ int32_t s_idx[kCtxSortSlots];   // bins of the locus by rank
   __shared__ uint32_t s_key[kCtxKeyStage];
   __shared__ int32_t s_scan[kCtxThreads];
   __shared__ int32_t s_carry;
   const int tid = threadIdx.x, kw = a.key_words;
   for (int64_t l = blockIdx.x; l < a.n_loci; l += gridDim.x) {
      const int64_t b0 = a.row_off[l];
      const int nb = (int)min((int64_t)kCtxMaxBins, a.row_off[l + 1] - b0);
      if (nb == 0 || a.n_rows[l] == 0) continue; // (uniform over the workgroup)
      const uint32_t *K = a.bin_key + b0 * kw;
      if ((int64_t)nb * kw <= kCtxKeyStage) {
         for (int i = tid; i < nb * kw; i += kCtxThreads) s_key[i] = K[i];
         K = s_key;
      }
      __syncthreads();
      if (nb <= kCtxAllPairs) {
         // keys of a locus are distinct: a bin's rank is the number of bins below it
         for (int b = tid; b < nb; b += kCtxThreads) s_idx[b] = -1;
         __syncthreads();
         for (int b = tid; b < nb; b += kCtxThreads) {
            int r = 0;
            for (int c = 0; c < nb; ++c) r += ctx_key_less(K + c * kw, K + b * kw, kw);
            s_idx[r] = b;
         }
         __syncthreads();
      } else {
         int n = kCtxAllPairs * 2;
         while (n < nb) n <<= 1;
         for (int i = tid; i < n; i += kCtxThreads) s_idx[i] = i < nb ? i : -1; // -1: beyond every bin
         __syncthreads();
         for (int k = 2; k <= n; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
               for (int i = tid; i < n; i += kCtxThreads) {
                  const int p = i ^ j;
                  if (p > i) {
                     const int x = s_idx[i], y = s_idx[p];
                     // y before x?  (a padding entry is before nothing and behind every bin)
                     const bool y_lt_x = y >= 0 && (x < 0 || ctx_key_less(K + y * kw, K + x * kw, kw));
                     const bool x_lt_y = x >= 0 && (y < 0 || ctx_key_less(K + x * kw, K + y * kw, kw));
                     if ((i & k) == 0 ? y_lt_x : x_lt_y) s_idx[i] = y, s_idx[p] = x;
                  }
               }
               __syncthreads();
            }
      }
      // the rows: the ranked bins that were hit, behind each other
      if (tid == 0) s_carry = 0;
      __syncthreads();
      const int64_t r0 = a.locus_row_off[l], q0 = a.locus_hit_off[l];
      for (int base = 0; base < nb; base += kCtxThreads) {
         const int r = base + tid;
         const int b = r < nb ? s_idx[r] : -1;
         const uint32_t n = b >= 0 ? a.n_in_bin[b0 + b] : 0u;
         s_scan[tid] = n != 0;
         __syncthreads();
         for (int d = 1; d < kCtxThreads; d <<= 1) {
            const int x = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += x;
            __syncthreads();
         }
         const int carry = s_carry;
         if (n) {
            const int64_t row = r0 + carry + s_scan[tid] - 1;
            if (row < a.locus_row_off[l + 1]) { // (always: the scan counted the same bins)
               a.row_bin[row] = b0 + b;
               a.row_hits[row] = n;
               a.row_last[row] = q0 + a.last_hit[b0 + b];
            }
         }
         __syncthreads();
         if (tid == kCtxThreads - 1) s_carry = carry + s_scan[tid];
         __syncthreads();
      }
   }
}

// row r of locus l: niso values at f_off[l] + (r - locus_row_off[l]) * niso; the locus' elements behind its rows are zeroed,
// so every element of row_prob is written by every call
__global__ __launch_bounds__(kCtxThreads) void ctx_gather_kernel(CtxArgs a)
{
   const int cw = a.compat_words;
   for (int64_t l = blockIdx.x; l < a.n_loci; l += gridDim.x) {
      const int64_t b0 = a.row_off[l], f0 = a.f_off[l], r0 = a.locus_row_off[l];
      const int64_t niso = a.iso_off[l + 1] - a.iso_off[l];
      const int64_t n_val = (a.locus_row_off[l + 1] - r0) * niso, n_all = a.f_off[l + 1] - f0;
      for (int64_t i = threadIdx.x; i < n_all; i += kCtxThreads) {
         double v = 0.0;
         if (i < n_val) {
            const int64_t r = r0 + i / niso;
            const int j = (int)(i % niso);
            v = ctx_row_value(a.compat + a.row_last[r] * cw, j, a.F[f0 + (a.row_bin[r] - b0) * niso + j]);
         }
         a.row_prob[f0 + i] = v;
      }
   }
}

} // namespace sb
