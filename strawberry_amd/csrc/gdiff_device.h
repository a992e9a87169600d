// strawberry_amd/csrc/gdiff_device.h -- the kernels of the differential isoform usage between two groups of replicate samples
// (include/sbgpu.h: sbgpu_em_gdiff_device, sbgpu_model_gdiff_device).  The solves are sbgpu_em_run_device's and the
// fits the fit's kernels, unchanged; what is here builds their inputs from the arrays S <= 16 batches hold in HBM, and reduces
// their outputs.  The shapes and thresholds are diff_device.h's, restated here: that header defines its kernels, so it can be in
// one translation unit only, and its text stays as it is.
// The samples' pointers are NOT kernel arguments: a device table of GdiffSample, indexed by sample, holds them (16 x 4 pointers
// as arguments would park SGPRs in VGPR lanes).
//
// gdiff_colscale_kernel: rule 3 for every OK locus, in diff_colscale_kernel's two shapes -- a group of 2^ceil(log2 K) lanes per
// locus for K <= 64, a workgroup for K <= 512 with the live flags of one sample's rows in LDS (one ballot per row); the LDS
// stays under the two-sample kernel's 16 KB.  A thread owns its columns: over the present samples in order it writes c^s_j to a
// global arena [S x K per locus] and carries group A's, group B's and ALL's running sums in registers; in a second loop it
// reads back the c values it wrote itself and stores alpha_group and alpha_all [S x K each].
//
// gdiff_expand_kernel: diff_expand_kernel's tile -- rows of ONE sample, thread t on elements t, t + 256, ..., add-and-carry
// indexing.  A weight is loaded once and stored up to three times from the register: the own copy as loaded, x alpha_group
// where the group has a sub-problem, x alpha_all.  The two alpha rows and the kept columns lie in LDS (4 + 4 + 2 KB).  Where the
// sample's rows begin inside the stacked sub-problems is in the tile record.  Bitwise the host form's.
//
// gdiff_cross_kernel(level): the cross fits' theta and status -- for every sub-problem those of its source at that level (an OWN
// sub-problem's group, or ALL; any other sub-problem's own: the fit's launches run over the whole sub-batch).
//
// gdiff_stat_kernel: rules 5-9 in two launches: <0> a thread per locus, <1> a thread per isoform and slot (sample, group,
// ALL).  Its arrays are one base and 32-bit offsets.  No atomics anywhere: every output has one writer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gdiff_rules.h"
#include "stage_host.h"

namespace sb {

// (diff_device.h's values and reasons)
constexpr int kGdiffThreads = 256;
constexpr int kGdiffTileVals = 4096;   // weights of one tile
constexpr int kGdiffTileRows = 512;    // rows of a tile at most
constexpr int kGdiffGroupMaxKept = 64; // a group of lanes lies inside one wave
constexpr int kGdiffGridPerCu = 8;     // workgroups per CU a launch is capped at (10 KB and 7.5 KB of LDS allow it)
constexpr int64_t kGdiffDefaultBytes = (int64_t)1 << 30;

__host__ __device__ inline int gdiff_tile_rows(int K) { return K < 1 || kGdiffTileVals / K > kGdiffTileRows ? kGdiffTileRows : kGdiffTileVals / K < 1 ? 1 : kGdiffTileVals / K; }
// lanes of a locus' group in the column-scale kernel; 0: the whole workgroup
__host__ __device__ inline int gdiff_group_lanes(int K)
{
   if (K > kGdiffGroupMaxKept) return 0;
   int p = 1;
   while (p < K) p <<= 1;
   return p;
}
template <class T>
__device__ inline T *gdiff_at(char *base, uint32_t units) { return (T *)(base + (size_t)units * 256); }
template <class T>
__device__ inline const T *gdiff_at(const char *base, uint32_t units) { return (const T *)(base + (size_t)units * 256); }

struct GdiffScaleArgs {
   int64_t n_items;
   const GdiffScaleItem *items;  // [n_items]
   const int32_t *list;          // the chunk's OK loci
   const GdiffSample *table;     // [S]
   int32_t S, n_a;
   const int64_t *iso_off;
   const int64_t *kept_off;      // [n_loci + 1]
   const int32_t *kept_col;
   int64_t kept0;                // kept_off of the chunk's first locus: the three arenas begin there
   double *c, *alpha_g, *alpha_a; // at S * (kept_off[l] - kept0): sample s' [K] at s * K
};

__global__ __launch_bounds__(kGdiffThreads) void gdiff_colscale_kernel(GdiffScaleArgs a)
{
   __shared__ uint8_t s_live[kStageMaxBins];
   __shared__ int32_t s_col[kDiffMaxKept];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_items; q += gridDim.x) {
      const GdiffScaleItem item = a.items[q];
      if (item.lanes > 0) {
         // ---- several loci to the workgroup: a group of `lanes` lanes each, a lane per kept column
         const int P = item.lanes, g = t / P, c = t % P;
         const bool has = g < item.n;
         const int64_t l = has ? a.list[item.first + g] : 0;
         const int K = has ? (int)(a.kept_off[l + 1] - a.kept_off[l]) : 0;
         const int niso = has ? (int)(a.iso_off[l + 1] - a.iso_off[l]) : 0;
         const bool mine = c < K;
         const int col = mine ? a.kept_col[a.kept_off[l] + c] : 0;
         const int64_t at = has ? a.S * (a.kept_off[l] - a.kept0) + c : 0;
         double sum_a = 0.0, sum_b = 0.0, sum_all = 0.0;
         int n_a = 0, n_b = 0;
         for (int s = 0; s < a.S; ++s) {
            if (!((item.mask >> s) & 1)) continue; // (the same for the whole workgroup)
            const GdiffSample sm = a.table[s];
            const int nb = has ? (int)(sm.row_off[l + 1] - sm.row_off[l]) : 0;
            const double *Fp = mine && nb > 0 ? sm.F + sm.f_off[l] + col : nullptr;
            double acc = 0.0;
            // (every lane of the workgroup runs item.rows steps, so that every shuffle has all of its lanes)
            for (int b = 0; b < item.rows; ++b) {
               const double v = mine && b < nb ? Fp[(int64_t)b * niso] : 0.0;
               int live = v > SBGPU_EM_ROW_EPS;
               for (int m = P >> 1; m >= 1; m >>= 1) live |= __shfl_xor(live, m);
               if (live) acc += v;
            }
            if (nb <= 0) continue;
            if (mine) a.c[at + (int64_t)s * K] = acc;
            sum_all = gdiff_add(sum_all, n_a + n_b, acc);
            if (s < a.n_a) sum_a = gdiff_add(sum_a, n_a, acc), ++n_a;
            else sum_b = gdiff_add(sum_b, n_b, acc), ++n_b;
         }
         if (!mine) continue;
         for (int s = 0; s < a.S; ++s) {
            if (!((item.mask >> s) & 1)) continue;
            const GdiffSample sm = a.table[s];
            if (sm.row_off[l + 1] - sm.row_off[l] <= 0) continue;
            const double cs = a.c[at + (int64_t)s * K];
            const bool in_a = s < a.n_a;
            if ((in_a ? n_a : n_b) >= 2) a.alpha_g[at + (int64_t)s * K] = gdiff_alpha(in_a ? sum_a : sum_b, cs, in_a ? n_a : n_b);
            a.alpha_a[at + (int64_t)s * K] = gdiff_alpha(sum_all, cs, n_a + n_b);
         }
         continue;
      }
      // ---- one wide locus to the workgroup: a thread owns columns t and t + 256
      const int64_t l = a.list[item.first];
      const int K = (int)min((int64_t)kDiffMaxKept, a.kept_off[l + 1] - a.kept_off[l]);
      const int niso = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      const int64_t at = a.S * (a.kept_off[l] - a.kept0);
      for (int c = t; c < K; c += kGdiffThreads) s_col[c] = a.kept_col[a.kept_off[l] + c];
      __syncthreads();
      double sum_a[2] = {0.0, 0.0}, sum_b[2] = {0.0, 0.0}, sum_all[2] = {0.0, 0.0};
      int n_a = 0, n_b = 0;
      for (int s = 0; s < a.S; ++s) {
         const GdiffSample sm = a.table[s];
         const int nb = (int)min((int64_t)kStageMaxBins, sm.row_off[l + 1] - sm.row_off[l]);
         if (nb <= 0) continue; // (the same for the whole workgroup)
         const double *Fp = sm.F + sm.f_off[l];
         const int wave = t >> 6, lane = t & 63;
         for (int b = wave; b < nb; b += kGdiffThreads / 64) {
            bool any = false;
            for (int c = lane; c < K; c += 64) any |= Fp[(int64_t)b * niso + s_col[c]] > SBGPU_EM_ROW_EPS;
            const bool live = __ballot(any) != 0;
            if (lane == 0) s_live[b] = live;
         }
         __syncthreads();
#pragma unroll
         for (int h = 0; h < 2; ++h) {
            const int c = t + h * kGdiffThreads;
            if (c >= K) continue;
            const double *Fc = Fp + s_col[c];
            double acc = 0.0;
            for (int b = 0; b < nb; ++b)
               if (s_live[b]) acc += Fc[(int64_t)b * niso];
            a.c[at + (int64_t)s * K + c] = acc;
            sum_all[h] = gdiff_add(sum_all[h], n_a + n_b, acc);
            if (s < a.n_a) sum_a[h] = gdiff_add(sum_a[h], n_a, acc);
            else sum_b[h] = gdiff_add(sum_b[h], n_b, acc);
         }
         if (s < a.n_a) ++n_a;
         else ++n_b;
         __syncthreads(); // (the flags are read: the next sample's may be written)
      }
      for (int s = 0; s < a.S; ++s) {
         const GdiffSample sm = a.table[s];
         if (sm.row_off[l + 1] - sm.row_off[l] <= 0) continue;
         const bool in_a = s < a.n_a;
#pragma unroll
         for (int h = 0; h < 2; ++h) {
            const int c = t + h * kGdiffThreads;
            if (c >= K) continue;
            const double cs = a.c[at + (int64_t)s * K + c];
            if ((in_a ? n_a : n_b) >= 2) a.alpha_g[at + (int64_t)s * K + c] = gdiff_alpha(in_a ? sum_a[h] : sum_b[h], cs, in_a ? n_a : n_b);
            a.alpha_a[at + (int64_t)s * K + c] = gdiff_alpha(sum_all[h], cs, n_a + n_b);
         }
      }
      __syncthreads(); // (the LDS is free for the workgroup's next item)
   }
}

struct GdiffExpandArgs {
   int64_t n_tiles;
   const GdiffTile *tiles;       // [n_tiles]
   const GdiffSample *table;     // [S]
   int32_t S, n_sub;
   const int64_t *iso_off;
   const int64_t *kept_off;      // [n_loci + 1]
   const int32_t *kept_col;
   int64_t kept0;                // the chunk's first kept column: the alphas begin there
   const double *alpha_g, *alpha_a;
   const int64_t *sub_row_off, *sub_f_off; // the chunk's sub-batch, [n_sub + 1]
   int32_t *sub_count;
   double *sub_F;
};

__global__ __launch_bounds__(kGdiffThreads) void gdiff_expand_kernel(GdiffExpandArgs a)
{
   __shared__ int32_t s_col[kDiffMaxKept];
   __shared__ double s_ag[kDiffMaxKept], s_aa[kDiffMaxKept];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_tiles; q += gridDim.x) {
      const GdiffTile tile = a.tiles[q];
      const int64_t l = tile.locus;
      const int s = tile.sample;
      // (never listed: a tile outside the chunk's sub-batch or the samples)
      if (s < 0 || s >= a.S || tile.own_q < 0 || tile.own_q >= a.n_sub || tile.all_q < 0 || tile.all_q >= a.n_sub || tile.grp_q >= a.n_sub) continue;
      const GdiffSample sm = a.table[s];
      const int niso = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      const int K = (int)min((int64_t)kDiffMaxKept, a.kept_off[l + 1] - a.kept_off[l]);
      const int64_t nb = sm.row_off[l + 1] - sm.row_off[l];
      const int rows = (int)max((int64_t)0, min((int64_t)tile.rows, nb - tile.row0)); // (the launcher cuts the tiles inside the locus)
      const bool grouped = tile.grp_q >= 0;
      const int64_t at = a.S * (a.kept_off[l] - a.kept0) + (int64_t)s * K;
      for (int c = t; c < K; c += kGdiffThreads)
         s_col[c] = a.kept_col[a.kept_off[l] + c], s_ag[c] = grouped ? a.alpha_g[at + c] : 1.0, s_aa[c] = a.alpha_a[at + c];
      __syncthreads();
      const int64_t grp_row = (int64_t)tile.grp_row0 + tile.row0, all_row = (int64_t)tile.all_row0 + tile.row0;
      if (K > 0) {
         const double *Fp = sm.F + sm.f_off[l] + (int64_t)tile.row0 * niso;
         double *own = a.sub_F + a.sub_f_off[tile.own_q] + (int64_t)tile.row0 * K;
         double *grp = grouped ? a.sub_F + a.sub_f_off[tile.grp_q] + grp_row * K : nullptr;
         double *all = a.sub_F + a.sub_f_off[tile.all_q] + all_row * K;
         const int dr = kGdiffThreads / K, dc = kGdiffThreads % K;
         int r = t / K, c = t % K;
         for (int i = t; i < rows * K; i += kGdiffThreads) {
            const double v = Fp[(int64_t)r * niso + s_col[c]];
            own[i] = v;
            if (grouped) grp[i] = v * s_ag[c];
            all[i] = v * s_aa[c];
            r += dr, c += dc;
            if (c >= K) c -= K, ++r;
         }
      }
      for (int r = t; r < rows; r += kGdiffThreads) {
         const int32_t n = sm.count[sm.row_off[l] + tile.row0 + r];
         a.sub_count[a.sub_row_off[tile.own_q] + tile.row0 + r] = n;
         if (grouped) a.sub_count[a.sub_row_off[tile.grp_q] + grp_row + r] = n;
         a.sub_count[a.sub_row_off[tile.all_q] + all_row + r] = n;
      }
      __syncthreads(); // (the tile is written: the LDS is free for the workgroup's next one)
   }
}

struct GdiffCrossArgs {
   int64_t n_sub;                // the chunk's sub-problems
   const int64_t *sub_iso_off;   // [n_sub + 1]
   const double *sub_theta;
   const int32_t *sub_status;
   const int32_t *src_g, *src_a; // [n_sub] the chunk's sub-problem a sub-problem reads at the group level and at ALL's
   double *x_theta;
   int32_t *x_status;
};

// level 0: the group's theta and status onto the OWN siblings; 1: ALL's
__global__ __launch_bounds__(kGdiffThreads) void gdiff_cross_kernel(GdiffCrossArgs a, int level)
{
   const int32_t *src = level ? a.src_a : a.src_g;
   const int64_t n_elem = a.sub_iso_off[a.n_sub], n_threads = max(n_elem, a.n_sub);
   for (int64_t x = (int64_t)blockIdx.x * kGdiffThreads + threadIdx.x; x < n_threads; x += (int64_t)gridDim.x * kGdiffThreads) {
      if (x < a.n_sub) a.x_status[x] = a.sub_status[min((int64_t)max(src[x], 0), a.n_sub - 1)];
      if (x >= n_elem) continue;
      // the element's sub-problem: the last q in [0, n_sub) with sub_iso_off[q] <= x
      int64_t lo = 0, hi = a.n_sub - 1;
      while (lo < hi) {
         const int64_t mid = (lo + hi + 1) >> 1;
         if (a.sub_iso_off[mid] <= x) lo = mid;
         else hi = mid - 1;
      }
      const int64_t from = min((int64_t)max(src[lo], 0), a.n_sub - 1);
      a.x_theta[x] = a.sub_theta[a.sub_iso_off[from] + (x - a.sub_iso_off[lo])];
   }
}

// The statistics' arrays as offsets into the call's arena, in units of 256 bytes (Arena::take's grain), as DiffStatOff
struct GdiffStatOff {
   uint32_t pre_status, p_a, p_b, rank, kept_off, kept_col, slot;            // made on the host (GdiffLayout's upload part)
   uint32_t theta_s, theta_g, theta_all, usage_s, usage_g, usage_all, delta; // per isoform
   uint32_t lr_b, lr_w, ll_own, ll_grp, ll_all, n_frag, lost_shift, dof_b, dof_w, status, top_iso; // per locus
   uint32_t st_s, it_s, st_g, it_g, st_all, it_all, sum;                     // sum: phase 0's notes for phase 1
   uint32_t fit_loglik, fit_n_live, fit_n_dropped, fit_n_impossible;         // FitLayout's, the same in the three fits
};
struct GdiffStatArgs {
   int64_t l0, l1;               // the chunk's loci
   int64_t n_loci, n_iso;        // the call's: the strides of the per-sample arrays
   int32_t S, n_a;
   const int64_t *iso_off;       // [n_loci + 1]
   const GdiffSample *table;     // [S]
   int64_t sub0;                 // the chunk's first sub-problem
   const int64_t *sub_iso_off;   // the chunk's sub-batch
   const double *sub_theta;
   const int32_t *sub_status, *sub_iters;
   char *res;                    // the call's arena (GdiffLayout)
   const char *fit, *g_fit, *a_fit; // the chunk's own, group-cross and ALL-cross fit (FitLayout)
   GdiffStatOff o;
};

// PHASE 0: a thread per locus of the chunk -- rules 5-7 and 9, and the theta sums of the locus' slots (a SOLE locus: where each
// placed a fragment) noted for phase 1.  PHASE 1, launched behind it: a thread per isoform and slot -- rule 8 from the locus'
// final status and sums; the thread of group A's slot writes delta_usage too.
template <int PHASE>
__global__ __launch_bounds__(kGdiffThreads) void gdiff_stat_kernel(GdiffStatArgs a)
{
   const int64_t i_first = a.iso_off[a.l0], n_iso_k = a.iso_off[a.l1] - i_first, n_loci_k = a.l1 - a.l0;
   const int S = a.S, slots = a.S + 3;
   const int64_t *slot_sub = gdiff_at<int64_t>(a.res, a.o.slot), *kept_off = gdiff_at<int64_t>(a.res, a.o.kept_off);
   const double one = 1.0;
   if (PHASE == 0) {
      const int64_t x = (int64_t)blockIdx.x * kGdiffThreads + threadIdx.x;
      if (x >= n_loci_k) return;
      const int64_t l = a.l0 + x;
      const int64_t *slot = slot_sub + l * slots;
      const bool solved = slot[S + 2] >= 0;
      const int K = (int)(kept_off[l + 1] - kept_off[l]);
      const int p_a = gdiff_at<int32_t>(a.res, a.o.p_a)[l], p_b = gdiff_at<int32_t>(a.res, a.o.p_b)[l];
      int32_t status = gdiff_at<int32_t>(a.res, a.o.pre_status)[l], top = -1;
      const double *ll = gdiff_at<double>(a.fit, a.o.fit_loglik), *llg = gdiff_at<double>(a.g_fit, a.o.fit_loglik), *lla = gdiff_at<double>(a.a_fit, a.o.fit_loglik);
      const long long *live = gdiff_at<long long>(a.fit, a.o.fit_n_live), *drop = gdiff_at<long long>(a.fit, a.o.fit_n_dropped);
      const long long *imp = gdiff_at<long long>(a.fit, a.o.fit_n_impossible);
      GdiffLocus o{0.0, 0.0, 0, status, 0, 0};
      if (solved) {
         const long long *dropg = gdiff_at<long long>(a.g_fit, a.o.fit_n_dropped), *impg = gdiff_at<long long>(a.g_fit, a.o.fit_n_impossible);
         const long long *dropa = gdiff_at<long long>(a.a_fit, a.o.fit_n_dropped), *impa = gdiff_at<long long>(a.a_fit, a.o.fit_n_impossible);
         GdiffAcc acc;
         gdiff_begin(&acc);
         long long lost_a = 0, lost_b = 0;
         for (int s = 0; s < S; ++s) {
            if (slot[s] < 0) continue;
            const int64_t q = slot[s] - a.sub0;
            const bool in_a = s < a.n_a;
            const long long lost = drop[q] + imp[q];
            gdiff_add_sample(&acc, a.sub_status[q], (in_a ? p_a : p_b) < 2, ll[q], llg[q], lla[q], live[q], imp[q], lost, dropg[q] + impg[q], dropa[q] + impa[q]);
            if (in_a) lost_a += lost;
            else lost_b += lost;
         }
         if (p_a >= 2) gdiff_add_group(&acc, a.sub_status[slot[S] - a.sub0], drop[slot[S] - a.sub0] + imp[slot[S] - a.sub0], lost_a);
         if (p_b >= 2) gdiff_add_group(&acc, a.sub_status[slot[S + 1] - a.sub0], drop[slot[S + 1] - a.sub0] + imp[slot[S + 1] - a.sub0], lost_b);
         const int64_t qa = slot[S + 2] - a.sub0;
         o = gdiff_finish(acc, K, a.sub_status[qa], drop[qa] + imp[qa]);
         status = o.status;
      }
      const bool ok = solved && status == SBGPU_DIFF_OK;
      double *sum = gdiff_at<double>(a.res, a.o.sum);
      double sum_ga = 0.0, sum_gb = 0.0;
      if (status == SBGPU_DIFF_SOLE) {
         // where each sample placed a fragment; a group: where one of its samples did; ALL: where any did
         for (int s = 0; s < S; ++s) {
            const GdiffSample sm = a.table[s];
            double placed = 0.0;
            for (int64_t b = sm.row_off[l]; b < sm.row_off[l + 1]; ++b)
               if (sm.count[b] > 0) placed = 1.0;
            sum[(int64_t)s * a.n_loci + l] = placed;
            if (s < a.n_a) sum_ga = placed > sum_ga ? placed : sum_ga;
            else sum_gb = placed > sum_gb ? placed : sum_gb;
         }
         sum[(int64_t)S * a.n_loci + l] = sum_ga, sum[(int64_t)(S + 1) * a.n_loci + l] = sum_gb;
         sum[(int64_t)(S + 2) * a.n_loci + l] = sum_ga > sum_gb ? sum_ga : sum_gb;
         top = diff_top(&one, sum_ga, &one, sum_gb, 1);
      } else {
         for (int x2 = 0; x2 < slots; ++x2) {
            const double v = ok && slot[x2] >= 0 ? diff_sum(a.sub_theta + a.sub_iso_off[slot[x2] - a.sub0], K) : 0.0;
            sum[(int64_t)x2 * a.n_loci + l] = v;
            if (x2 == S) sum_ga = v;
            if (x2 == S + 1) sum_gb = v;
         }
         if (ok) top = diff_top(a.sub_theta + a.sub_iso_off[slot[S] - a.sub0], sum_ga, a.sub_theta + a.sub_iso_off[slot[S + 1] - a.sub0], sum_gb, K);
      }
      gdiff_at<double>(a.res, a.o.lr_b)[l] = o.lr_between, gdiff_at<double>(a.res, a.o.lr_w)[l] = o.lr_within;
      gdiff_at<long long>(a.res, a.o.lost_shift)[l] = o.lost_shift;
      gdiff_at<int32_t>(a.res, a.o.dof_b)[l] = o.dof_between, gdiff_at<int32_t>(a.res, a.o.dof_w)[l] = o.dof_within;
      gdiff_at<int32_t>(a.res, a.o.status)[l] = status;
      gdiff_at<int32_t>(a.res, a.o.top_iso)[l] = top >= 0 ? gdiff_at<int32_t>(a.res, a.o.kept_col)[kept_off[l] + top] : -1;
      for (int s = 0; s < S; ++s) {
         const bool there = solved && slot[s] >= 0, on = ok && there;
         const int64_t q = there ? slot[s] - a.sub0 : 0, at = (int64_t)s * a.n_loci + l;
         const bool single = (s < a.n_a ? p_a : p_b) < 2;
         gdiff_at<double>(a.res, a.o.ll_own)[at] = on ? ll[q] : 0.0;
         gdiff_at<double>(a.res, a.o.ll_grp)[at] = on ? (single ? ll[q] : llg[q]) : 0.0;
         gdiff_at<double>(a.res, a.o.ll_all)[at] = on ? lla[q] : 0.0;
         gdiff_at<long long>(a.res, a.o.n_frag)[at] = on ? live[q] - imp[q] : 0;
         gdiff_at<int32_t>(a.res, a.o.st_s)[at] = there ? a.sub_status[q] : -1;
         gdiff_at<int32_t>(a.res, a.o.it_s)[at] = there ? a.sub_iters[q] : -1;
      }
      for (int g = 0; g < 2; ++g) {
         const bool there = solved && slot[S + g] >= 0;
         const int64_t q = there ? slot[S + g] - a.sub0 : 0;
         gdiff_at<int32_t>(a.res, a.o.st_g)[(int64_t)g * a.n_loci + l] = there ? a.sub_status[q] : -1;
         gdiff_at<int32_t>(a.res, a.o.it_g)[(int64_t)g * a.n_loci + l] = there ? a.sub_iters[q] : -1;
      }
      gdiff_at<int32_t>(a.res, a.o.st_all)[l] = solved ? a.sub_status[slot[S + 2] - a.sub0] : -1;
      gdiff_at<int32_t>(a.res, a.o.it_all)[l] = solved ? a.sub_iters[slot[S + 2] - a.sub0] : -1;
      return;
   }
   const int32_t *rank = gdiff_at<int32_t>(a.res, a.o.rank), *status = gdiff_at<int32_t>(a.res, a.o.status);
   const double *sum = gdiff_at<double>(a.res, a.o.sum);
   const int64_t n_work = n_iso_k * slots;
   for (int64_t x = (int64_t)blockIdx.x * kGdiffThreads + threadIdx.x; x < n_work; x += (int64_t)gridDim.x * kGdiffThreads) {
      const int xs = (int)(x / n_iso_k);
      const int64_t i = i_first + x % n_iso_k;
      // the isoform's locus: the last l in [l0, l1) with iso_off[l] <= i
      int64_t lo = a.l0, hi = a.l1 - 1;
      while (lo < hi) {
         const int64_t mid = (lo + hi + 1) >> 1;
         if (a.iso_off[mid] <= i) lo = mid;
         else hi = mid - 1;
      }
      const int64_t l = lo;
      const int64_t *slot = slot_sub + l * slots;
      const int r = rank[i];
      const int32_t st = status[l];
      // one slot's theta and usage of this isoform
      const auto of = [&](int k, double *th) {
         double us = 0.0;
         *th = 0.0;
         if (r >= 0 && st == SBGPU_DIFF_OK && slot[k] >= 0) {
            *th = a.sub_theta[a.sub_iso_off[slot[k] - a.sub0] + r];
            us = diff_usage(*th, sum[(int64_t)k * a.n_loci + l]);
         } else if (r >= 0 && st == SBGPU_DIFF_SOLE) {
            us = diff_usage(one, sum[(int64_t)k * a.n_loci + l]);
         }
         return us;
      };
      double th;
      const double us = of(xs, &th);
      if (xs < S) {
         gdiff_at<double>(a.res, a.o.theta_s)[(int64_t)xs * a.n_iso + i] = th, gdiff_at<double>(a.res, a.o.usage_s)[(int64_t)xs * a.n_iso + i] = us;
      } else if (xs < S + 2) {
         gdiff_at<double>(a.res, a.o.theta_g)[(int64_t)(xs - S) * a.n_iso + i] = th, gdiff_at<double>(a.res, a.o.usage_g)[(int64_t)(xs - S) * a.n_iso + i] = us;
         if (xs == S) {
            double th_b;
            const double us_b = of(S + 1, &th_b);
            gdiff_at<double>(a.res, a.o.delta)[i] = us_b - us;
         }
      } else {
         gdiff_at<double>(a.res, a.o.theta_all)[i] = th, gdiff_at<double>(a.res, a.o.usage_all)[i] = us;
      }
   }
}

} // namespace sb
