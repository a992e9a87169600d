// strawberry_amd/csrc/loo_device.h -- the kernels of the drop-one isoform support (include/sbgpu.h: sbgpu_em_loo_device,
// sbgpu_model_loo_device).  The solves are sbgpu_em_run_device's and the fit's kernels, unchanged; what is here
// builds their inputs from the arrays a batch holds in HBM, and reduces their outputs.
//
// loo_expand_kernel, the one with traffic: a locus of K kept isoforms and nb bins becomes K + 1 matrices (1 for K = 1) of
// nb x K and nb x (K - 1) doubles -- (K + 1) nb K - K nb weights written for nb K read.  A workgroup takes a TILE: rows
// [row0, row0 + rows) of one locus, rows = min(kLooTileRows, kLooTileVals / K), so the tile's kept columns are at most
// kLooTileVals doubles (32 KB of LDS; 64 rows at K = 64).  It reads them from HBM ONCE -- a gather along the row, contiguous
// where the kept columns are -- and then writes every sub-copy's part from LDS.  A tile's part of a sub-copy is one contiguous
// run of rows x cols doubles in the output (the copy is row-major and keeps all rows), so thread t stores elements t, t + 256,
// ...: consecutive lanes store consecutive 8-byte words.  The (row, column) of an element follows the thread's first by
// add-and-carry (256 / cols rows and 256 % cols columns further each step): two divisions per thread and sub-shape, none in
// the loops.  The counts' copies ride along.  Every store is of a loaded value: the expansion is bitwise the host form's.
//
// loo_stat_kernel: a thread per isoform of the chunk's loci gathers its sub-problem's and its base's results (loo_isoform), and
// scatters the base's theta; a thread per locus stores the locus' three.  No atomics anywhere: every output has one writer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "loo_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kLooThreads = 256;
constexpr int kLooTileVals = 4096; // doubles of one tile in LDS: 32 KB: four workgroups of a CU hold theirs in its 160 KB (16 waves, 4 per SIMD)
constexpr int kLooTileRows = 512;  // rows of a tile at most: a narrow, deep locus is spread over several workgroups
constexpr int kLooGridPerCu = 8;   // workgroups per CU a launch is capped at (the kernels stride over their work)
constexpr int64_t kLooDefaultBytes = (int64_t)1 << 30;

__host__ __device__ inline int loo_tile_rows(int K) { return K < 1 || kLooTileVals / K > kLooTileRows ? kLooTileRows : kLooTileVals / K; }

struct LooExpandArgs {
   int64_t n_tiles;
   const LooTile *tiles;                      // [n_tiles]
   const int64_t *row_off, *iso_off, *f_off;  // the parent's, [n_loci + 1]
   const int32_t *count;                      // the parent's
   const double *F;
   const int64_t *first_sub, *kept_off;       // [n_loci], [n_loci + 1] (first_sub numbers all sub-problems of the call)
   const int32_t *kept_col;
   int64_t sub0;                              // the chunk's first sub-problem: the chunk's offsets below begin there
   const int64_t *sub_row_off, *sub_f_off;    // the chunk's sub-batch, [n_sub + 1]
   int32_t *sub_count;
   double *sub_F;
};

__global__ __launch_bounds__(kLooThreads) void loo_expand_kernel(LooExpandArgs a)
{
   __shared__ double s_F[kLooTileVals];
   __shared__ int32_t s_col[kLooMaxKept];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_tiles; q += gridDim.x) {
      const LooTile tile = a.tiles[q];
      const int64_t l = tile.locus;
      if (a.first_sub[l] < a.sub0) continue; // (never listed: a locus without sub-problems, or another chunk's)
      const int niso = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      const int K = (int)min((int64_t)kLooMaxKept, a.kept_off[l + 1] - a.kept_off[l]);
      const int rows = K > 0 ? min(tile.rows, kLooTileVals / K) : 0; // (the launcher cuts the tiles by loo_tile_rows: no tile is larger)
      const int64_t fs = a.first_sub[l] - a.sub0;
      const int n_sub = (int)loo_n_sub(K);
      if (t < K) s_col[t] = a.kept_col[a.kept_off[l] + t];
      __syncthreads();
      // ---- the tile's kept columns: HBM -> LDS, once
      const double *Fp = a.F + a.f_off[l] + (int64_t)tile.row0 * niso;
      if (K > 0) {
         const int dr = kLooThreads / K, dc = kLooThreads % K;
         int r = t / K, c = t % K;
         for (int i = t; i < rows * K; i += kLooThreads) {
            s_F[i] = Fp[(int64_t)r * niso + s_col[c]];
            r += dr, c += dc;
            if (c >= K) c -= K, ++r;
         }
      }
      // the counts of the tile's rows, into every sub-problem
      for (int r = t; r < rows; r += kLooThreads) {
         const int32_t n = a.count[a.row_off[l] + tile.row0 + r];
         for (int s = 0; s < n_sub; ++s) a.sub_count[a.sub_row_off[fs + s] + tile.row0 + r] = n;
      }
      __syncthreads();
      // ---- the base: the tile as it lies in LDS
      if (K > 0) {
         double *o = a.sub_F + a.sub_f_off[fs] + (int64_t)tile.row0 * K;
         for (int i = t; i < rows * K; i += kLooThreads) o[i] = s_F[i];
      }
      // ---- the K copies without one column
      if (K >= 2) {
         const int C = K - 1, dr = kLooThreads / C, dc = kLooThreads % C;
         const int r_first = t / C, c_first = t % C;
         for (int d = 0; d < K; ++d) {
            double *o = a.sub_F + a.sub_f_off[fs + 1 + d] + (int64_t)tile.row0 * C;
            int r = r_first, c = c_first;
            for (int i = t; i < rows * C; i += kLooThreads) {
               o[i] = s_F[r * K + loo_sub_rank(c, d)];
               r += dr, c += dc;
               if (c >= C) c -= C, ++r;
            }
         }
      }
      __syncthreads(); // (the tile is written: the LDS is free for the workgroup's next one)
   }
}

struct LooStatArgs {
   int64_t l0, l1;                           // the chunk's loci
   const int64_t *iso_off;                   // the parent's, [n_loci + 1]
   const int32_t *loo_status, *rank;         // [n_loci], [n_iso]
   const int64_t *first_sub, *kept_off;
   const int32_t *kept_col;
   const int64_t *without_off;               // [n_iso + 1]
   int64_t sub0;
   const int64_t *sub_iso_off;               // the chunk's sub-batch
   const double *sub_theta;
   const int32_t *sub_status, *sub_iters;
   const double *sub_loglik;
   const long long *sub_n_live, *sub_n_dropped, *sub_n_impossible;
   double *lr_stat, *heir_gain, *theta_refit;
   long long *n_unique;
   int32_t *heir, *status_without, *iters_without, *support;
   double *loglik_base;
   int32_t *status_base, *iters_base;
   double *theta_without;
};

__global__ __launch_bounds__(kLooThreads) void loo_stat_kernel(LooStatArgs a)
{
   const int64_t i_first = a.iso_off[a.l0], n_iso = a.iso_off[a.l1] - i_first, n_loci = a.l1 - a.l0;
   const int64_t n_threads = max(n_iso, n_loci);
   for (int64_t x = (int64_t)blockIdx.x * kLooThreads + threadIdx.x; x < n_threads; x += (int64_t)gridDim.x * kLooThreads) {
      if (x < n_loci) {
         const int64_t l = a.l0 + x, fs = a.first_sub[l] - a.sub0;
         const bool ok = a.first_sub[l] >= 0;
         a.loglik_base[l] = ok ? a.sub_loglik[fs] : 0.0;
         a.status_base[l] = ok ? a.sub_status[fs] : -1;
         a.iters_base[l] = ok ? a.sub_iters[fs] : -1;
      }
      if (x >= n_iso) continue;
      const int64_t i = i_first + x;
      // the isoform's locus: the last l in [l0, l1) with iso_off[l] <= i
      int64_t lo = a.l0, hi = a.l1 - 1;
      while (lo < hi) {
         const int64_t mid = (lo + hi + 1) >> 1;
         if (a.iso_off[mid] <= i) lo = mid;
         else hi = mid - 1;
      }
      const int64_t l = lo;
      const int r = a.rank[i];
      const int K = (int)(a.kept_off[l + 1] - a.kept_off[l]);
      const int64_t fs = a.first_sub[l] - a.sub0;
      LooIsoform o{0, 0.0, 0.0, -1};
      int32_t stw = -1, itw = -1, supp = r == -1 ? SBGPU_LOO_NOT_KEPT : SBGPU_LOO_LOCUS_SKIPPED;
      double refit = 0.0;
      if (r >= 0) {
         const double *tb = a.sub_theta + a.sub_iso_off[fs];
         refit = tb[r];
         if (K == 1) {
            supp = SBGPU_LOO_SOLE;
            o.n_unique = a.sub_n_live[fs] - a.sub_n_impossible[fs], o.lr_stat = (double)INFINITY;
         } else {
            const int64_t s = fs + 1 + r;
            const double *ts = a.sub_theta + a.sub_iso_off[s];
            supp = SBGPU_LOO_TESTED, stw = a.sub_status[s], itw = a.sub_iters[s];
            o = loo_isoform(K, r, tb, ts, a.kept_col + a.kept_off[l], a.sub_n_dropped[s] + a.sub_n_impossible[s],
                            a.sub_n_dropped[fs] + a.sub_n_impossible[fs], a.sub_loglik[s], a.sub_loglik[fs]);
            double *w = a.theta_without + a.without_off[i];
            for (int k = 0; k < K - 1; ++k) w[k] = ts[k];
         }
      }
      a.lr_stat[i] = o.lr_stat, a.heir_gain[i] = o.heir_gain, a.theta_refit[i] = refit;
      a.n_unique[i] = o.n_unique;
      a.heir[i] = o.heir, a.status_without[i] = stw, a.iters_without[i] = itw, a.support[i] = supp;
   }
}

} // namespace sb
