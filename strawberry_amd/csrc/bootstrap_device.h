// strawberry_amd/csrc/bootstrap_device.h -- the EM bootstrap's kernels (gfx950): the replicates' bin counts by the rule of
// bootstrap_rules.h, and Welford's recurrence over the replicates' theta.  Launched by bootstrap_api.hip.
//
//   boot_prefix_kernel     once per call: every locus' inclusive prefix sums of its counts, its total N, its number of work
//                          items (slices of kBootSlice draws, at least one), and the two faults a count array can hold
//   boot_item_scan_kernel  once per call: the loci's first work items (exclusive scan; one workgroup)
//   boot_resample_kernel   per replicate: one workgroup per (replicate, locus, slice); integers only
//   boot_stats_kernel      per replicate: one thread per isoform (mean, M2 -> variance) and per locus (status counts)
//   boot_interval_kernel   once per statistic: mean, variance and two order statistics of every column of a replicate-major
//                          matrix [n_rep][n] (sbgpu_replicate_stats_device; the FPKM and TPM intervals of
//                          sbgpu_abundance_bootstrap_device; Frac, locus FPKM and locus TPM of
//                          sbgpu_locus_bootstrap_device)
//   boot_locus_sum_kernel  per replicate, or once (sbgpu_locus_abundance_device): one thread per (row, locus): the locus' kept
//                          FPKM sum and the number of kept isoforms by boot_locus_sum
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

// ---- statistics over the replicates, column by column (rules: bootstrap_rules.h)
//
// The matrix is replicate-major: a column's elements lie 8 n bytes apart.  A workgroup stages a tile of kBootTile neighbouring
// columns through LDS -- sixteen lanes read the tile's 128 contiguous bytes of a row, a wave four rows at once -- and every wave
// then owns kBootTile / 4 of the columns, one after the other: a lane runs Welford's recurrence over the staged column in
// replicate order; the wave takes the column into registers as sort keys (element e = v * 64 + lane in key[v], padded to the
// next power of two with kBootKeyPad), sorts it with a bitonic network -- lane exchanges for strides below 64, register swaps
// above, every index known at compile time -- and reads the two requested positions out.  With `keep` the staged value is the
// replicate's TPM (boot_tpm_value of the FPKM, its keep flag and the replicate's total), so no TPM matrix is ever written, and
// the staging lanes count the column's kept replicates.  A column in LDS is rotated by its index within the tile: the tile's
// columns of one row would otherwise share a bank whenever n_rep is a multiple of 32 (rotated by c mod n_rep: n_rep may be below the tile's width).
constexpr int kBootTile = 16;             // columns of a workgroup's tile: 16 * n_rep * 8 bytes of LDS, 128 KB of gfx950's 160 at the cap
constexpr int kBootIntervalThreads = 256; // four waves, kBootTile / 4 columns each

struct BootIntervalArgs {
   int64_t n;                    // columns
   int32_t n_rep, rank_lo, rank_hi;
   const double *x;              // [n_rep][n]
   const int32_t *keep;          // [n_rep][n], or null: x is taken as it stands.  Any value other than 0 is "kept": the isoforms'
                                 // keep (0 / 1 / 2), or -- the locus columns -- the loci's numbers of kept isoforms
   const double *total;          // [n_rep] (with keep)
   double *mean, *var, *lo, *hi; // [n], each may be null
   int32_t *keep_count;          // [n], zero on entry, or null (with keep)
};

template <int V> // keys per lane: the column padded to 64 V elements
__global__ __launch_bounds__(kBootIntervalThreads) void boot_interval_kernel(const BootIntervalArgs a)
{
   extern __shared__ double s_col[]; // [kBootTile][n_rep]
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int B = a.n_rep;
   const int64_t j0 = (int64_t)blockIdx.x * kBootTile;
   {
      const int c = tid & (kBootTile - 1), rot = c % B;
      const int64_t j = j0 + c;
      int32_t kept = 0;
      for (int r = tid / kBootTile; r < B; r += kBootIntervalThreads / kBootTile) {
         double v = 0.0;
         if (j < a.n) {
            const size_t at = (size_t)r * (size_t)a.n + (size_t)j;
            v = a.x[at];
            if (a.keep) {
               const int32_t kp = a.keep[at];
               kept += kp != 0;
               v = boot_tpm_value(v, kp, a.total[r]);
            }
         }
         int pos = r + rot;
         if (pos >= B) pos -= B;
         s_col[c * B + pos] = v;
      }
      if (a.keep_count) { // (whole waves arrive here) the lanes of a wave that staged the same column: the lane bits above the tile's
#pragma unroll
         for (int d = kBootTile; d < 64; d <<= 1) kept += __shfl_xor(kept, d);
         if (lane < kBootTile && j < a.n && kept) atomicAdd(&a.keep_count[j], kept);
      }
   }
   __syncthreads();
   constexpr int kPerWave = kBootTile / (kBootIntervalThreads / 64);
   if (lane < kPerWave && (a.mean || a.var)) {
      const int c = wave * kPerWave + lane, rot = c % B;
      const int64_t j = j0 + c;
      if (j < a.n) {
         double m = 0.0, q = 0.0;
         for (int k = 0; k < B; ++k) {
            int pos = k + rot;
            if (pos >= B) pos -= B;
            boot_welford_step(s_col[c * B + pos], k, m, q);
         }
         if (a.mean) a.mean[j] = m;
         if (a.var) a.var[j] = boot_welford_var(q, B);
      }
   }
   if (!a.lo && !a.hi) return;
   for (int ci = 0; ci < kPerWave; ++ci) {
      const int c = wave * kPerWave + ci, rot = c % B;
      const int64_t j = j0 + c;
      if (j >= a.n) break; // (uniform over the wave)
      uint64_t key[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
         const int e = v * 64 + lane;
         int pos = e + rot;
         if (pos >= B) pos -= B;
         key[v] = e < B ? boot_sort_key(s_col[c * B + pos]) : kBootKeyPad;
      }
#pragma unroll
      for (int size = 2; size <= 64 * V; size <<= 1) {
#pragma unroll
         for (int d = size >> 1; d > 0; d >>= 1) {
            if (d >= 64) { // both elements in this lane (size >= 128: the direction depends on v alone)
               const int dv = d >> 6;
#pragma unroll
               for (int v = 0; v < V; ++v) {
                  if (v & dv) continue;
                  const bool asc = ((v * 64) & size) == 0;
                  const uint64_t p = key[v], q = key[v | dv];
                  const uint64_t mn = p < q ? p : q, mx = p < q ? q : p;
                  key[v] = asc ? mn : mx;
                  key[v | dv] = asc ? mx : mn;
               }
            } else {
               const bool lower = (lane & d) == 0;
#pragma unroll
               for (int v = 0; v < V; ++v) {
                  const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)key[v], d);
                  const bool asc = ((v * 64 + lane) & size) == 0;
                  const uint64_t mn = key[v] < other ? key[v] : other, mx = key[v] < other ? other : key[v];
                  key[v] = asc == lower ? mn : mx;
               }
            }
         }
      }
      // element e of the sorted column lives in key[e >> 6] of lane e & 63
      uint64_t k_lo = 0, k_hi = 0;
#pragma unroll
      for (int v = 0; v < V; ++v) {
         if (v == (a.rank_lo >> 6)) k_lo = key[v];
         if (v == (a.rank_hi >> 6)) k_hi = key[v];
      }
      k_lo = (uint64_t)__shfl((unsigned long long)k_lo, a.rank_lo & 63);
      k_hi = (uint64_t)__shfl((unsigned long long)k_hi, a.rank_hi & 63);
      if (lane == 0) {
         if (a.lo) a.lo[j] = boot_key_value(k_lo);
         if (a.hi) a.hi[j] = boot_key_value(k_hi);
      }
   }
}

// ---- abundances per locus (rule: boot_locus_sum, bootstrap_rules.h)
//
// One thread per (row, locus) of fpkm / keep [n_rows][n_iso]: neighbouring lanes own neighbouring loci and so neighbouring
// isoform ranges -- a wave's loads fall in one contiguous stretch of the row.  The additions run in isoform order (the rule);
// the loads come four at a time.  No atomics, no LDS.  With `total` ([n_rows]) the locus' TPM is written too.
struct BootLocusSumArgs {
   int64_t n_loci, n_iso; // n_iso: the rows' stride in fpkm / keep
   int32_t n_rows;
   const int64_t *iso_off; // [n_loci + 1]
   const double *fpkm;     // [n_rows][n_iso]
   const int32_t *keep;    // [n_rows][n_iso]
   const double *total;    // [n_rows], or null (then locus_tpm is null)
   double *locus_fpkm, *locus_tpm; // [n_rows][n_loci], each may be null
   int32_t *locus_kept;            // [n_rows][n_loci], or null
};

__global__ __launch_bounds__(256) void boot_locus_sum_kernel(const BootLocusSumArgs a)
{
   const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
   if (i >= a.n_loci * a.n_rows) return;
   const int64_t r = i / a.n_loci, l = i - r * a.n_loci;
   double sum;
   int32_t kept;
   boot_locus_sum(a.fpkm + r * a.n_iso, a.keep + r * a.n_iso, a.iso_off[l], a.iso_off[l + 1], sum, kept);
   if (a.locus_fpkm) a.locus_fpkm[i] = sum;
   if (a.locus_kept) a.locus_kept[i] = kept;
   if (a.locus_tpm) a.locus_tpm[i] = boot_locus_tpm(sum, kept, a.total[r]);
}

} // namespace sb
