// strawberry_amd/csrc/bootstrap_device.h -- the EM bootstrap's kernels (gfx950): the replicates' bin counts by the rule of
// bootstrap_rules.h, and Welford's recurrence over the replicates' theta.  Launched by bootstrap_api.hip.
//
//   boot_prefix_kernel     once per call: every locus' inclusive prefix sums of its counts, its total N, its number of work
//                          items (slices of kBootSlice draws, at least one), and the two faults a count array can hold
//   boot_item_scan_kernel  once per call: the loci's first work items (exclusive scan; one workgroup)
//   boot_resample_kernel   per replicate: one workgroup per (replicate, locus, slice); integers only
//   boot_stats_kernel      per replicate: one thread per isoform (mean, M2 -> variance) and per locus (status counts)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bootstrap_rules.h"

namespace sb {

constexpr int kBootThreads = 256;
constexpr int kBootSlice = 16384;   // draws of one work item (even: a Philox call's pair of draws never straddles two items)
constexpr int kBootTabRows = 1024;  // rows of a locus whose prefix sums and histogram live in LDS (12 KB); beyond: through L2
constexpr int kBootAggRows = 8;     // loci of at most this many rows count equal rows inside a wave before the LDS atomic
constexpr int64_t kBootFaultNegative = 1, kBootFaultDeep = 2; // bits of head[0]

// head[0]: fault bits; head[1]: work items of one replicate (written by the scan)
__global__ __launch_bounds__(kBootThreads) void boot_prefix_kernel(int64_t n_loci, const int64_t *__restrict__ row_off,
                                                                   const int32_t *__restrict__ count, int64_t *__restrict__ incl,
                                                                   int64_t *__restrict__ total, int32_t *__restrict__ items,
                                                                   int64_t *__restrict__ head)
{
   const int lane = threadIdx.x & 63;
   const int64_t l = (int64_t)blockIdx.x * (kBootThreads / 64) + (threadIdx.x >> 6); // one wave per locus
   if (l >= n_loci) return;
   const int64_t r0 = row_off[l], r1 = row_off[l + 1];
   int64_t carry = 0;
   bool negative = false;
   for (int64_t base = r0; base < r1; base += 64) {
      const int64_t i = base + lane;
      int64_t v = 0;
      if (i < r1) {
         const int32_t c = count[i];
         negative |= c < 0;
         v = c < 0 ? 0 : c;
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { // inclusive scan over the wave
         const int64_t up = __shfl_up(v, d);
         if (lane >= d) v += up;
      }
      if (i < r1) incl[i] = carry + v;
      carry += __shfl(v, 63);
   }
   if (__ballot(negative) != 0 && lane == 0) atomicOr((unsigned long long *)&head[0], (unsigned long long)kBootFaultNegative);
   if (lane == 0) {
      const bool deep = carry >= kBootMaxDraws;
      if (deep) atomicOr((unsigned long long *)&head[0], (unsigned long long)kBootFaultDeep);
      total[l] = carry;
      const int64_t slices = (carry + kBootSlice - 1) / kBootSlice; // < 2^26
      items[l] = (deep || slices < 1) ? 1 : (int32_t)slices;
   }
}

// item_off[l] = items[0] + ... + items[l - 1], item_off[n_loci] = head[1] = their sum.  One workgroup of 1024: every thread
// sums a contiguous stretch, the stretches' sums are scanned in LDS, every thread writes its stretch.
__global__ __launch_bounds__(1024) void boot_item_scan_kernel(int64_t n_loci, const int32_t *__restrict__ items, int64_t *__restrict__ item_off,
                                                              int64_t *__restrict__ head)
{
   __shared__ int64_t part[1024];
   const int t = threadIdx.x;
   const int64_t per = (n_loci + 1023) / 1024, a = (int64_t)t * per, b = a + per < n_loci ? a + per : n_loci;
   int64_t s = 0;
   for (int64_t l = a; l < b; ++l) s += items[l];
   part[t] = s;
   __syncthreads();
   for (int d = 1; d < 1024; d <<= 1) {
      const int64_t up = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += up;
      __syncthreads();
   }
   int64_t run = part[t] - s;
   for (int64_t l = a; l < b; ++l) {
      item_off[l] = run;
      run += items[l];
   }
   if (t == 1023) {
      item_off[n_loci] = part[1023];
      head[1] = part[1023];
   }
}

struct BootResampleArgs {
   int64_t n_loci, n_items, total_rows; // n_items: work items of ONE replicate
   const int64_t *row_off, *locus_id;   // locus_id: the loci's global ids, or null: their index
   const int64_t *incl, *total, *item_off;
   uint64_t seed;
   int32_t rep_first, n_rep;
   int32_t *out; // [n_rep][total_rows], zero on entry
};

// One draw into the workgroup's LDS histogram.  `aggregate` (uniform over the workgroup): the lanes of a wave that hit the same
// row elect one of them to add their number -- a locus of a handful of rows otherwise sends most of a wave to one LDS word,
// where the atomics of a wave-instruction take their turns.  Called by whole waves (`valid` says which lanes hold a draw).
__device__ inline void boot_count_draw(int32_t *hist, int32_t row, bool valid, bool aggregate)
{
   if (!aggregate) {
      if (valid) atomicAdd(&hist[row], 1);
      return;
   }
   const int lane = threadIdx.x & 63;
   unsigned long long todo = __ballot(valid);
   while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int32_t lr = __shfl(row, leader);
      const unsigned long long same = __ballot(valid && row == lr);
      if (lane == leader) atomicAdd(&hist[lr], (int32_t)__popcll(same));
      todo &= ~same;
   }
}

__global__ __launch_bounds__(kBootThreads) void boot_resample_kernel(const BootResampleArgs a)
{
   __shared__ int64_t s_incl[kBootTabRows];
   __shared__ int32_t s_hist[kBootTabRows];
   const int tid = threadIdx.x;
   const int64_t rep_k = (int64_t)blockIdx.x / a.n_items, item = (int64_t)blockIdx.x % a.n_items;
   if (rep_k >= a.n_rep) return;
   // the item's locus: the last l with item_off[l] <= item (every locus has an item, so item_off rises strictly)
   int64_t lo = 0, hi = a.n_loci - 1;
   while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.item_off[mid] <= item) lo = mid;
      else hi = mid - 1;
   }
   const int64_t l = lo, r0 = a.row_off[l], N = a.total[l];
   const int64_t nr64 = a.row_off[l + 1] - r0;
   if (nr64 <= 0 || N <= 0) return; // (the output is zero already)
   const int32_t nr = (int32_t)nr64;
   const int64_t first = a.item_off[l], n_slices = a.item_off[l + 1] - first;
   const int64_t d0 = (item - first) * kBootSlice, d1 = d0 + kBootSlice < N ? d0 + kBootSlice : N;
   const int64_t g = a.locus_id ? a.locus_id[l] : l;
   const int32_t r = a.rep_first + (int32_t)rep_k;
   int32_t *out = a.out + rep_k * a.total_rows + r0;
   const int64_t *incl = a.incl + r0;
   if (nr <= kBootTabRows) {
      for (int32_t i = tid; i < nr; i += kBootThreads) {
         s_incl[i] = incl[i];
         s_hist[i] = 0;
      }
      __syncthreads();
      const bool aggregate = nr <= kBootAggRows;
      for (int64_t base = d0 >> 1; 2 * base < d1; base += kBootThreads) { // uniform trip count: whole waves reach boot_count_draw
         const int64_t q = base + tid;
         const bool v0 = 2 * q < d1, v1 = 2 * q + 1 < d1;
         uint64_t t[2] = {0, 0};
         if (v0) boot_draw_pair(g, r, a.seed, q, N, t);
         boot_count_draw(s_hist, v0 ? boot_row_of(s_incl, nr, t[0]) : 0, v0, aggregate);
         boot_count_draw(s_hist, v1 ? boot_row_of(s_incl, nr, t[1]) : 0, v1, aggregate);
      }
      __syncthreads();
      // one store per row for a locus that is one item; one global atomic per row that got a draw for a locus in slices
      for (int32_t i = tid; i < nr; i += kBootThreads) {
         const int32_t v = s_hist[i];
         if (n_slices == 1) out[i] = v;
         else if (v) atomicAdd(&out[i], v);
      }
   } else {
      // more rows than the table holds: the search reads the prefix sums through L2, the draws go to the output directly
      for (int64_t q = (d0 >> 1) + tid; 2 * q < d1; q += kBootThreads) {
         uint64_t t[2];
         boot_draw_pair(g, r, a.seed, q, N, t);
         atomicAdd(&out[boot_row_of(incl, nr, t[0])], 1);
         if (2 * q + 1 < d1) atomicAdd(&out[boot_row_of(incl, nr, t[1])], 1);
      }
   }
}

struct BootStatsArgs {
   int64_t n_iso, n_loci;
   int32_t step, n_rep;  // this replicate is number `step` of n_rep (0-based)
   const double *theta;  // the replicate's results
   const int32_t *status, *iters;
   double *mean, *var;   // var holds M2 between the steps; the last step divides
   int32_t *status_count; // [n_loci][4], zero before step 0
   double *theta_rep;    // this replicate's slot of the caller's arrays, or null
   int32_t *status_rep, *iters_rep;
};

// Welford's recurrence in replicate order (the steps follow each other on one stream):
//    m_k = m_{k-1} + (x_k - m_{k-1}) / k,   M2_k = M2_{k-1} + (x_k - m_{k-1}) (x_k - m_k),   var = M2_B / (B - 1)
__global__ __launch_bounds__(256) void boot_stats_kernel(const BootStatsArgs a)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i < a.n_iso) {
      const double x = a.theta[i];
      const double m0 = a.step ? a.mean[i] : 0.0, q0 = a.step ? a.var[i] : 0.0;
      const double d = x - m0;
      const double m = m0 + d / (double)(a.step + 1);
      const double q = q0 + d * (x - m);
      a.mean[i] = m;
      a.var[i] = a.step + 1 < a.n_rep ? q : (a.n_rep > 1 ? q / (double)(a.n_rep - 1) : 0.0);
      if (a.theta_rep) a.theta_rep[i] = x;
   }
   if (i < a.n_loci) {
      const int32_t st = a.status[i];
      if (st >= 0 && st < 4) a.status_count[i * 4 + st] += 1;
      if (a.status_rep) a.status_rep[i] = st;
      if (a.iters_rep) a.iters_rep[i] = a.iters[i];
   }
}

} // namespace sb
