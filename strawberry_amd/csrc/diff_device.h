// strawberry_amd/csrc/diff_device.h -- the kernels of the differential isoform usage (include/sbgpu.h: sbgpu_em_diff_device,
// sbgpu_model_diff_device).  The solves are sbgpu_em_run_device's and the fits the fit's kernels, unchanged; what is
// here builds their inputs from the arrays two batches hold in HBM, and reduces their outputs.
//
// diff_colscale_kernel: rule 3's live rows, column sums and alpha for every OK locus.  A LANE OWNS A KEPT COLUMN and walks the
// rows of A, then of B, in ascending order -- the host form's order, so the sums are its bits; the lanes of a locus read
// consecutive kept weights of one row (F is row-major).  Whether a row is live is an OR over the locus' lanes.  A locus of
// K <= 64 kept isoforms takes a group of P = 2^ceil(log2 K) lanes, and 256 / P loci share a workgroup (a K = 2 locus occupies 2
// threads, not 256): the OR is log2 P xor-shuffles inside the group, there is no LDS and no barrier.  A wider locus (K <= 512)
// takes a workgroup: the live flags of a sample's rows go to LDS (a wave per row, one ballot), then every thread walks the
// rows for its columns t and t + 256.
//
// diff_expand_kernel, the one with traffic: nb K weights read per sample, 2 nb K written.  A workgroup takes a TILE: rows
// [row0, row0 + rows) of one locus in one sample, rows = max(1, min(kDiffTileRows, kDiffTileVals / K)).  A tile's part of the own
// copy and of the pooled problem are contiguous runs of rows x K doubles (both are row-major and keep all rows), so thread t
// handles elements t, t + 256, ...: consecutive lanes store consecutive 8-byte words whatever K is, and read consecutive kept
// columns of a row.  The (row, column) of an element follows the thread's first by add-and-carry: two divisions per thread,
// none in the loop.  Every weight is read once and stored twice from the register -- the own copy as loaded, the pooled one
// times the column's alpha, which lies in LDS beside the kept column list (6 KB; the weights themselves need no staging, each
// is used by one thread).  The counts ride along.  Bitwise the host form's: a copy and a single product under -ffp-contract=off.
//
// diff_cross_kernel: the cross fit's theta and status -- the pooled sub-problem's copied onto its A and B siblings (and onto
// itself: the fit's launches run over the whole sub-batch).
//
// diff_stat_kernel: rules 5-9 in two launches: <0> a thread per locus of the chunk (the statistic, the integers, the final
// status, top_iso, and the locus' three theta sums noted in the arena), <1> a thread per isoform (theta, usage, delta from the
// locus' status and sums: no isoform thread repeats its locus' work).  Its arrays are a base and 32-bit offsets, not fifty
// pointers.  No atomics anywhere: every output has one writer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "diff_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kDiffThreads = 256;
constexpr int kDiffTileVals = 4096;  // weights of one tile: 16 per thread, enough loads in flight to cover HBM latency, and a 512-column locus still gets 8 rows
constexpr int kDiffTileRows = 512;   // rows of a tile at most: a narrow, deep locus is spread over several workgroups
constexpr int kDiffGroupMaxKept = 64; // a group of lanes lies inside one wave (the shuffles), so it serves 64 columns at most
constexpr int kDiffGridPerCu = 8;    // workgroups per CU a launch is capped at: 8 x 256 threads is the CU's 2048 (the expand kernel's 6 KB of LDS and the column-scale kernel's 16 KB allow it: 128 KB of 160)
constexpr int64_t kDiffDefaultBytes = (int64_t)1 << 30;

__host__ __device__ inline int diff_tile_rows(int K) { return K < 1 || kDiffTileVals / K > kDiffTileRows ? kDiffTileRows : kDiffTileVals / K < 1 ? 1 : kDiffTileVals / K; }
// lanes of a locus' group in the column-scale kernel; 0: the whole workgroup
__host__ __device__ inline int diff_group_lanes(int K)
{
   if (K > kDiffGroupMaxKept) return 0;
   int p = 1;
   while (p < K) p <<= 1;
   return p;
}

struct DiffScaleArgs {
   int64_t n_items;
   const DiffScaleItem *items;                // [n_items]
   const int32_t *list;                       // the chunk's OK loci
   const int64_t *row_off[2], *f_off[2];      // the two samples', [n_loci + 1]
   const double *F[2];
   const int64_t *iso_off;
   const int64_t *kept_off;                   // [n_loci + 1]
   const int32_t *kept_col;
   int64_t kept0;                             // kept_off of the chunk's first locus: alpha begins there
   double *alpha;                             // at 2 * (kept_off[l] - kept0): A's [K], then B's [K]
};

__global__ __launch_bounds__(kDiffThreads) void diff_colscale_kernel(DiffScaleArgs a)
{
   __shared__ uint8_t s_live[kStageMaxBins];
   __shared__ int32_t s_col[kDiffMaxKept];
   __shared__ double s_c[2][kDiffMaxKept];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_items; q += gridDim.x) {
      const DiffScaleItem item = a.items[q];
      if (item.lanes > 0) {
         // ---- several loci to the workgroup: a group of `lanes` lanes each, a lane per kept column
         const int P = item.lanes, g = t / P, c = t % P;
         const bool has = g < item.n;
         const int64_t l = has ? a.list[item.first + g] : 0;
         const int K = has ? (int)(a.kept_off[l + 1] - a.kept_off[l]) : 0;
         const int niso = has ? (int)(a.iso_off[l + 1] - a.iso_off[l]) : 0;
         const bool mine = c < K;
         const int col = mine ? a.kept_col[a.kept_off[l] + c] : 0;
         double sum[2];
         for (int s = 0; s < 2; ++s) {
            const int nb = has ? (int)(a.row_off[s][l + 1] - a.row_off[s][l]) : 0;
            const double *Fp = mine ? a.F[s] + a.f_off[s][l] + col : nullptr;
            double acc = 0.0;
            // (every lane of the workgroup runs item.rows steps, so that every shuffle has all of its lanes)
            for (int b = 0; b < item.rows; ++b) {
               const double v = mine && b < nb ? Fp[(int64_t)b * niso] : 0.0;
               int live = v > SBGPU_EM_ROW_EPS;
               for (int m = P >> 1; m >= 1; m >>= 1) live |= __shfl_xor(live, m);
               if (live) acc += v;
            }
            sum[s] = acc;
         }
         if (mine) {
            double *o = a.alpha + 2 * (a.kept_off[l] - a.kept0);
            o[c] = diff_alpha(sum[0], sum[1], sum[0]), o[K + c] = diff_alpha(sum[0], sum[1], sum[1]);
         }
         continue;
      }
      // ---- one wide locus to the workgroup
      const int64_t l = a.list[item.first];
      const int K = (int)min((int64_t)kDiffMaxKept, a.kept_off[l + 1] - a.kept_off[l]);
      const int niso = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      for (int c = t; c < K; c += kDiffThreads) s_col[c] = a.kept_col[a.kept_off[l] + c];
      __syncthreads();
      for (int s = 0; s < 2; ++s) {
         const int nb = (int)min((int64_t)kStageMaxBins, a.row_off[s][l + 1] - a.row_off[s][l]);
         const double *Fp = a.F[s] + a.f_off[s][l];
         const int wave = t >> 6, lane = t & 63;
         for (int b = wave; b < nb; b += kDiffThreads / 64) {
            bool any = false;
            for (int c = lane; c < K; c += 64) any |= Fp[(int64_t)b * niso + s_col[c]] > SBGPU_EM_ROW_EPS;
            const bool live = __ballot(any) != 0;
            if (lane == 0) s_live[b] = live;
         }
         __syncthreads();
         for (int c = t; c < K; c += kDiffThreads) {
            const double *Fc = Fp + s_col[c];
            double acc = 0.0;
            for (int b = 0; b < nb; ++b)
               if (s_live[b]) acc += Fc[(int64_t)b * niso];
            s_c[s][c] = acc;
         }
         __syncthreads(); // (the flags are read: the next sample's may be written)
      }
      double *o = a.alpha + 2 * (a.kept_off[l] - a.kept0);
      for (int c = t; c < K; c += kDiffThreads) o[c] = diff_alpha(s_c[0][c], s_c[1][c], s_c[0][c]), o[K + c] = diff_alpha(s_c[0][c], s_c[1][c], s_c[1][c]);
      __syncthreads(); // (the LDS is free for the workgroup's next item)
   }
}

struct DiffExpandArgs {
   int64_t n_tiles;
   const DiffTile *tiles;                     // [n_tiles]
   const int64_t *row_off[2], *f_off[2];      // the two samples', [n_loci + 1]
   const int32_t *count[2];
   const double *F[2];
   const int64_t *iso_off;
   const int64_t *first_sub, *kept_off;       // [n_loci], [n_loci + 1] (first_sub numbers all sub-problems of the call)
   const int32_t *kept_col;
   int64_t sub0, kept0;                       // the chunk's first sub-problem and first kept column: the chunk's arrays below begin there
   const double *alpha;
   const int64_t *sub_row_off, *sub_f_off;    // the chunk's sub-batch, [n_sub + 1]
   int32_t *sub_count;
   double *sub_F;
};

__global__ __launch_bounds__(kDiffThreads) void diff_expand_kernel(DiffExpandArgs a)
{
   __shared__ int32_t s_col[kDiffMaxKept];
   __shared__ double s_alpha[kDiffMaxKept];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_tiles; q += gridDim.x) {
      const DiffTile tile = a.tiles[q];
      const int64_t l = tile.locus;
      const int s = tile.sample & 1;
      if (a.first_sub[l] < a.sub0) continue; // (never listed: a locus without sub-problems, or another chunk's)
      const int niso = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      const int K = (int)min((int64_t)kDiffMaxKept, a.kept_off[l + 1] - a.kept_off[l]);
      const int64_t nb = a.row_off[s][l + 1] - a.row_off[s][l], nb_a = a.row_off[0][l + 1] - a.row_off[0][l];
      const int rows = (int)max((int64_t)0, min((int64_t)tile.rows, nb - tile.row0)); // (the launcher cuts the tiles inside the locus)
      const int64_t fs = a.first_sub[l] - a.sub0;
      const int64_t pool_row0 = (s ? nb_a : 0) + tile.row0;
      const double *al = a.alpha + 2 * (a.kept_off[l] - a.kept0) + (s ? K : 0);
      for (int c = t; c < K; c += kDiffThreads) s_col[c] = a.kept_col[a.kept_off[l] + c], s_alpha[c] = al[c];
      __syncthreads();
      if (K > 0) {
         const double *Fp = a.F[s] + a.f_off[s][l] + (int64_t)tile.row0 * niso;
         double *own = a.sub_F + a.sub_f_off[fs + s] + (int64_t)tile.row0 * K;
         double *pool = a.sub_F + a.sub_f_off[fs + 2] + pool_row0 * K;
         const int dr = kDiffThreads / K, dc = kDiffThreads % K;
         int r = t / K, c = t % K;
         for (int i = t; i < rows * K; i += kDiffThreads) {
            const double v = Fp[(int64_t)r * niso + s_col[c]];
            own[i] = v;
            pool[i] = v * s_alpha[c];
            r += dr, c += dc;
            if (c >= K) c -= K, ++r;
         }
      }
      for (int r = t; r < rows; r += kDiffThreads) {
         const int32_t n = a.count[s][a.row_off[s][l] + tile.row0 + r];
         a.sub_count[a.sub_row_off[fs + s] + tile.row0 + r] = n;
         a.sub_count[a.sub_row_off[fs + 2] + pool_row0 + r] = n;
      }
      __syncthreads(); // (the tile is written: the LDS is free for the workgroup's next one)
   }
}

struct DiffCrossArgs {
   int64_t n_sub;                             // the chunk's sub-problems: triples A, B, POOLED
   const int64_t *sub_iso_off;                // [n_sub + 1]
   const double *sub_theta;
   const int32_t *sub_status;
   double *x_theta;
   int32_t *x_status;
};

__global__ __launch_bounds__(kDiffThreads) void diff_cross_kernel(DiffCrossArgs a)
{
   const int64_t n_elem = a.sub_iso_off[a.n_sub], n_threads = max(n_elem, a.n_sub);
   for (int64_t x = (int64_t)blockIdx.x * kDiffThreads + threadIdx.x; x < n_threads; x += (int64_t)gridDim.x * kDiffThreads) {
      if (x < a.n_sub) a.x_status[x] = a.sub_status[x - x % 3 + 2];
      if (x >= n_elem) continue;
      // the element's sub-problem: the last q in [0, n_sub) with sub_iso_off[q] <= x
      int64_t lo = 0, hi = a.n_sub - 1;
      while (lo < hi) {
         const int64_t mid = (lo + hi + 1) >> 1;
         if (a.sub_iso_off[mid] <= x) lo = mid;
         else hi = mid - 1;
      }
      a.x_theta[x] = a.sub_theta[a.sub_iso_off[lo - lo % 3 + 2] + (x - a.sub_iso_off[lo])];
   }
}

// The statistics' arrays as offsets into two blocks, in units of 256 bytes (Arena::take's grain): some fifty pointers as kernel
// arguments cost a hundred SGPRs and spilled; a base and a 32-bit offset each do not.
struct DiffStatOff {
   uint32_t pre_status, rank, first_sub, kept_off, kept_col;                 // made on the host (DiffLayout's upload part)
   uint32_t theta[3], usage[3], delta;                                       // per isoform; A, B, POOLED
   uint32_t lr_stat, loglik[4], n_a, n_b, lost_shift, dof, status, top_iso;  // per locus; ll_A, ll_B own, then at the pooled theta
   uint32_t st[3], it[3], sum[3];                                            // sum: phase 0's notes for phase 1
   uint32_t fit_loglik, fit_n_live, fit_n_dropped, fit_n_impossible;         // FitLayout's, the same in the own and the cross fit
};
struct DiffStatArgs {
   int64_t l0, l1;                            // the chunk's loci
   const int64_t *iso_off;                    // [n_loci + 1]
   const int64_t *row_off[2];                 // the two samples'
   const int32_t *count[2];
   int64_t sub0;
   const int64_t *sub_iso_off;                // the chunk's sub-batch
   const double *sub_theta;
   const int32_t *sub_status, *sub_iters;
   char *res;                                 // the call's arena (DiffLayout)
   const char *fit, *x_fit;                   // the chunk's own and cross fit (FitLayout)
   DiffStatOff o;
};
template <class T>
__device__ inline T *diff_at(char *base, uint32_t units) { return (T *)(base + (size_t)units * 256); }
template <class T>
__device__ inline const T *diff_at(const char *base, uint32_t units) { return (const T *)(base + (size_t)units * 256); }

// rules 5-7 of an OK locus whose first sub-problem is the chunk's fs
__device__ inline DiffLocus diff_locus_of(const DiffStatArgs &a, int64_t fs, int K)
{
   const int64_t A = fs, B = fs + 1, P = fs + 2;
   const double *ll = diff_at<double>(a.fit, a.o.fit_loglik), *llx = diff_at<double>(a.x_fit, a.o.fit_loglik);
   const long long *live = diff_at<long long>(a.fit, a.o.fit_n_live), *drop = diff_at<long long>(a.fit, a.o.fit_n_dropped);
   const long long *imp = diff_at<long long>(a.fit, a.o.fit_n_impossible);
   const long long *dropx = diff_at<long long>(a.x_fit, a.o.fit_n_dropped), *impx = diff_at<long long>(a.x_fit, a.o.fit_n_impossible);
   return diff_locus(K, a.sub_status[A], a.sub_status[B], a.sub_status[P], ll[A], ll[B], llx[A], llx[B], live[A], imp[A], live[B], imp[B], drop[A] + imp[A],
                     drop[B] + imp[B], drop[P] + imp[P], dropx[A] + impx[A], dropx[B] + impx[B]);
}
// 1.0 where sample s placed a fragment in locus l, else 0.0
__device__ inline double diff_placed(const DiffStatArgs &a, int s, int64_t l)
{
   for (int64_t b = a.row_off[s][l]; b < a.row_off[s][l + 1]; ++b)
      if (a.count[s][b] > 0) return 1.0;
   return 0.0;
}

// PHASE 0: a thread per locus of the chunk -- rules 5-7 and 9, and the locus' three theta sums (a SOLE locus: where each
// sample placed a fragment) noted for phase 1.  PHASE 1, launched behind it: a thread per isoform -- rule 8 from the locus'
// final status and sums, so that no isoform thread repeats its locus' work.
template <int PHASE>
__global__ __launch_bounds__(kDiffThreads) void diff_stat_kernel(DiffStatArgs a)
{
   const int64_t i_first = a.iso_off[a.l0], n_iso = a.iso_off[a.l1] - i_first, n_loci = a.l1 - a.l0;
   const int64_t *first_sub = diff_at<int64_t>(a.res, a.o.first_sub), *kept_off = diff_at<int64_t>(a.res, a.o.kept_off);
   const double one = 1.0;
   if (PHASE == 0) {
      const int32_t *kept_col = diff_at<int32_t>(a.res, a.o.kept_col);
      // (no stride loop here: some thirty arrays are touched once each, and a loop would keep all their addresses in SGPRs
      // across it -- that is what spilled; the launch has a thread per locus)
      const int64_t x = (int64_t)blockIdx.x * kDiffThreads + threadIdx.x;
      if (x < n_loci) {
         const int64_t l = a.l0 + x, fs = first_sub[l] - a.sub0;
         const bool solved = first_sub[l] >= 0;
         const int K = (int)(kept_off[l + 1] - kept_off[l]);
         int32_t status = diff_at<int32_t>(a.res, a.o.pre_status)[l], top = -1;
         DiffLocus o{0.0, 0, 0, 0, status, 0};
         double ll[4] = {0.0, 0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0};
         if (solved) {
            o = diff_locus_of(a, fs, K);
            status = o.status;
            if (status == SBGPU_DIFF_OK) {
               const double *own = diff_at<double>(a.fit, a.o.fit_loglik), *cross = diff_at<double>(a.x_fit, a.o.fit_loglik);
               ll[0] = own[fs], ll[1] = own[fs + 1], ll[2] = cross[fs], ll[3] = cross[fs + 1];
               for (int k = 0; k < 3; ++k) sum[k] = diff_sum(a.sub_theta + a.sub_iso_off[fs + k], K);
               top = diff_top(a.sub_theta + a.sub_iso_off[fs], sum[0], a.sub_theta + a.sub_iso_off[fs + 1], sum[1], K);
            }
         }
         if (status == SBGPU_DIFF_SOLE) {
            sum[0] = diff_placed(a, 0, l), sum[1] = diff_placed(a, 1, l), sum[2] = sum[0] > sum[1] ? sum[0] : sum[1];
            top = diff_top(&one, sum[0], &one, sum[1], 1);
         }
         diff_at<double>(a.res, a.o.lr_stat)[l] = o.lr_stat;
         for (int k = 0; k < 4; ++k) diff_at<double>(a.res, a.o.loglik[k])[l] = ll[k];
         diff_at<long long>(a.res, a.o.n_a)[l] = o.n_a, diff_at<long long>(a.res, a.o.n_b)[l] = o.n_b;
         diff_at<long long>(a.res, a.o.lost_shift)[l] = o.lost_shift;
         diff_at<int32_t>(a.res, a.o.dof)[l] = o.dof, diff_at<int32_t>(a.res, a.o.status)[l] = status;
         diff_at<int32_t>(a.res, a.o.top_iso)[l] = top >= 0 ? kept_col[kept_off[l] + top] : -1;
         for (int k = 0; k < 3; ++k) {
            diff_at<int32_t>(a.res, a.o.st[k])[l] = solved ? a.sub_status[fs + k] : -1;
            diff_at<int32_t>(a.res, a.o.it[k])[l] = solved ? a.sub_iters[fs + k] : -1;
            diff_at<double>(a.res, a.o.sum[k])[l] = sum[k];
         }
      }
      return;
   }
   const int32_t *rank = diff_at<int32_t>(a.res, a.o.rank), *status = diff_at<int32_t>(a.res, a.o.status);
   for (int64_t x = (int64_t)blockIdx.x * kDiffThreads + threadIdx.x; x < n_iso; x += (int64_t)gridDim.x * kDiffThreads) {
      const int64_t i = i_first + x;
      // the isoform's locus: the last l in [l0, l1) with iso_off[l] <= i
      int64_t lo = a.l0, hi = a.l1 - 1;
      while (lo < hi) {
         const int64_t mid = (lo + hi + 1) >> 1;
         if (a.iso_off[mid] <= i) lo = mid;
         else hi = mid - 1;
      }
      const int64_t l = lo, fs = first_sub[l] - a.sub0;
      const int r = rank[i];
      double th[3] = {0.0, 0.0, 0.0}, us[3] = {0.0, 0.0, 0.0};
      if (r >= 0 && status[l] == SBGPU_DIFF_OK) {
         for (int k = 0; k < 3; ++k) th[k] = a.sub_theta[a.sub_iso_off[fs + k] + r], us[k] = diff_usage(th[k], diff_at<double>(a.res, a.o.sum[k])[l]);
      } else if (r >= 0 && status[l] == SBGPU_DIFF_SOLE) {
         for (int k = 0; k < 3; ++k) us[k] = diff_usage(one, diff_at<double>(a.res, a.o.sum[k])[l]);
      }
      for (int k = 0; k < 3; ++k) diff_at<double>(a.res, a.o.theta[k])[i] = th[k], diff_at<double>(a.res, a.o.usage[k])[i] = us[k];
      diff_at<double>(a.res, a.o.delta)[i] = us[1] - us[0];
   }
}

} // namespace sb
