// strawberry_amd/csrc/info_device.h -- the isoform information (include/sbgpu.h: sbgpu_em_info_device, sbgpu_model_info_device)
// from the arrays a batch has in HBM anyway.  The live flags and the gains are asg_column_kernel's
// (assign_device.h, launched unchanged through sb::asg_launch_column_pass); the pass below makes everything else.
//
// One locus is served by a GROUP of T threads: a wave (T = 64; info_wave_kernel, kInfoWaveLoci loci per workgroup) for a locus
// of at most kInfoWaveVals weights and kInfoWaveIso isoforms, a workgroup (T = 256; info_block_kernel) for a larger one, up to
// kInfoMaxFree free isoforms.  Every number is made by a function of info_rules.h, by ONE thread, in the rule's order -- the
// host form's bits; threads only share the work out:
//   1  a thread per bin: d_b and w_b (LDS up to NW bins, the arena's w beyond).  Wave 0 meanwhile lists the free isoforms in
//      ascending order (a ballot per 64 isoforms; free-local index p -> isoform idx[p]).
//   2  a thread per free isoform: c_j again, down its column (asg_column_kernel keeps the gain, not the sum).
//   3  a wave per pair (j, k) of H's triangle, the pairs dealt round-robin to the group's waves: lane t walks the bins t, t + 64,
//      ..., and the __shfl_down tree (lane i adds lane i + s, s = 32 .. 1) is the rule's wave order.
//   4  who is observed, dg; then a thread per row scales it to C.  A and B are packed triangles in LDS (info_tri).
//   5  the factorisation: a loop over the columns, a thread per row i >= j.  Every thread of column j computes piv_j itself from
//      row j (complete since the barrier of column j - 1: the same bits in every thread), so a column needs ONE barrier; thread
//      i == j records the decision, thread i > j makes L_ij.  The loop runs MF columns whatever the locus has.
//   6  a thread per column of Y;  7  a thread per entry of V -> Hinv (into A: L is dead);  8  a thread per isoform: u;
//   9  a thread per entry: cov (into A, and into the packed block where the locus has one);  10  se;  11  a thread per free
//      isoform: partner, ident, and a thread per isoform of the locus: the defaults of those that are not free.
// F is read from LDS where the locus has at most NF weights, from global memory beyond.
// THE BARRIERS: their number (12 + MF per locus) does not depend on the data; a group without a locus (l < 0) runs them only.
// A packed triangle's rows begin at i (i + 1) / 2: no stride is a multiple of 32 doubles, so no row is padded.
// No floating-point atomics, no inline assembly, no MFMA (its accumulation order is not the rule's).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "info_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kInfoMaxBins = kStageMaxBins, kInfoMaxWords = kStageMaxWords; // (stage_host.h)
constexpr int kInfoThreads = 256;
constexpr int kInfoWaveLoci = kInfoThreads / kInfoWave; // loci of one workgroup in the wave form
constexpr int kInfoWaveVals = 512;  // weights (and so bins) of a locus up to which a wave serves it (2 x 4 KB of LDS)
constexpr int kInfoWaveIso = 16;    // isoforms of such a locus: its two triangles take 2 x 1088 bytes
constexpr int kInfoStage = 1536;    // bins whose w_b, and weights of a locus that, the workgroup form keeps in LDS (2 x 12 KB)
constexpr int kInfoGridPerCu = 8;   // workgroups per CU a launch is capped at (the kernels stride over their lists)

__host__ __device__ inline bool info_wave_form(int64_t nb, int64_t niso) { return nb <= kInfoWaveVals && niso <= kInfoWaveIso && nb * niso <= kInfoWaveVals; }

struct InfoArgs {
   int64_t n_list;                 // loci of this launch
   const int32_t *list;            // [n_list] their indices
   const int64_t *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int64_t *cov_off;         // [n_loci + 1]
   const int32_t *count;           // [n_bins]
   const double *F;                // [n_elem]
   const int32_t *keep, *status;   // [n_iso], [n_loci]
   const uint8_t *live;            // [n_bins]  asg_column_kernel's
   const double *gain;             // [n_iso]   asg_column_kernel's
   double *w;                      // [n_bins]  w_b of the loci of more than kInfoStage bins
   double *se, *partner_corr;      // [n_iso]
   int32_t *ident, *alias_of, *partner; // [n_iso]
   double *min_pivot;              // [n_loci]
   int32_t *rank, *n_free, *info_status; // [n_loci]
   double *cov;                    // [cov_off[n_loci]] zeroed per call
};

// lane 0 of the wave gets the wave order's sum (info_rules.h)
__device__ inline double info_wave_sum(double v)
{
   for (int s = kInfoWave / 2; s >= 1; s >>= 1) v += __shfl_down(v, s, kInfoWave);
   return v;
}

// entry e of a packed triangle -> its row (the column is e - info_tri(row, 0))
__device__ inline int info_tri_row(int e)
{
   int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
   while (info_tri(i + 1, 0) <= e) ++i;
   while (info_tri(i, 0) > e) --i;
   return i;
}

// What a group shares.  NW: bin weights, NF: staged weights, NK: kept words, MF: free isoforms.
template <int NW, int NF, int NK, int MF>
struct InfoShared {
   double w[NW];
   double F[NF];
   double A[MF * (MF + 1) / 2], B[MF * (MF + 1) / 2];
   double c[MF], dg[MF], ld[MF], piv[MF], u[MF], se[MF];
   uint32_t keep[NK];
   int32_t idx[MF], alias[MF];
   uint8_t st[MF], obs[MF];
   int32_t nf;
};

// One locus by one group of T threads (lane: the thread's index in the group; l < 0: no locus, the barriers only).  Every
// thread of the WORKGROUP reaches every __syncthreads() below, whatever its locus' shape.
template <int T, int NW, int NF, int NK, int MF>
__device__ inline void info_locus(const InfoArgs &a, int64_t l, int lane, InfoShared<NW, NF, NK, MF> &sh)
{
   static_assert(MF <= kInfoMaxFree, "the rule's limit");
   constexpr int WAVES = T / kInfoWave;
   const int wave = lane / kInfoWave, wlane = lane % kInfoWave;
   int64_t b0 = 0, i0 = 0, niso_out = 0;
   int nb = 0, niso = 0;
   bool skip = false; // beyond the assignment's shape limits: nothing of the locus is read
   const double *Fl = nullptr;
   double *w = sh.w;
   if (l >= 0) {
      b0 = a.row_off[l], i0 = a.iso_off[l];
      const int64_t nb_all = a.row_off[l + 1] - b0;
      niso_out = a.iso_off[l + 1] - i0;
      skip = nb_all > kInfoMaxBins || niso_out > (int64_t)32 * NK;
      nb = skip ? 0 : (int)nb_all, niso = skip ? 0 : (int)niso_out;
      Fl = a.F + a.f_off[l];
      const int words = (niso + 31) >> 5;
      const int32_t st = a.status[l];
      for (int k = lane; k < words; k += T) sh.keep[k] = ctx_kept_word(a.keep + i0, niso, st, k);
      const int n_val = nb * niso; // (<= 5632 * 4096: fits an int)
      if (n_val <= NF) {
         for (int i = lane; i < n_val; i += T) sh.F[i] = Fl[i];
         Fl = sh.F;
      }
      if (nb > NW) w = a.w + b0;
   }
   __syncthreads();
   const double *G = a.gain + i0;
   // ---- 1: the bins' weights; the free isoforms' list
   for (int b = lane; b < nb; b += T) {
      const bool live = a.live[b0 + b];
      const double d = live ? fit_bin_mass(Fl + (int64_t)b * niso, niso, sh.keep, G) : 0.0;
      w[b] = info_weight(a.count[b0 + b], d, fit_possible(live, d));
   }
   if (wave == 0) {
      int cnt = 0;
      for (int base = 0; base < niso; base += kInfoWave) {
         const int j = base + wlane;
         const bool f = j < niso && info_free(G[j]);
         const unsigned long long m = __ballot(f);
         const int pos = cnt + __popcll(m & ((1ull << wlane) - 1ull));
         if (f && pos < MF) sh.idx[pos] = j;
         cnt += __popcll(m);
      }
      if (wlane == 0) sh.nf = cnt;
   }
   __syncthreads();
   const int n_free = sh.nf;
   const int32_t status = skip || n_free > MF ? SBGPU_INFO_TOO_WIDE : n_free == 0 ? SBGPU_INFO_EMPTY : SBGPU_INFO_OK;
   const int nf = status == SBGPU_INFO_OK ? n_free : 0;
   const int ntri = nf * (nf + 1) / 2;
   // ---- 2: c_j of the free isoforms
   for (int p = lane; p < nf; p += T) {
      const int j = sh.idx[p];
      double c = 0.0;
      for (int b = 0; b < nb; ++b)
         if (a.live[b0 + b]) c += Fl[(int64_t)b * niso + j];
      sh.c[p] = c;
   }
   __syncthreads();
   // ---- 3: H, a wave per pair
   {
      int pi = 0, pj = wave; // pair q = info_tri(pi, pj)
      for (int q = wave; q < ntri; q += WAVES) {
         while (pj > pi) pj -= pi + 1, ++pi;
         const int gj = sh.idx[pj], gi = sh.idx[pi];
         double s = 0.0;
         for (int b = wlane; b < nb; b += kInfoWave) s += info_term(w[b], Fl[(int64_t)b * niso + gj], Fl[(int64_t)b * niso + gi]);
         s = info_wave_sum(s);
         if (wlane == 0) sh.A[q] = info_h(s, sh.c[pj], sh.c[pi]);
         pj += WAVES;
      }
   }
   __syncthreads();
   // ---- 4: who is observed, dg, C
   for (int p = lane; p < nf; p += T) {
      const double h = sh.A[info_tri(p, p)];
      const bool obs = info_observed(h);
      sh.obs[p] = obs, sh.st[p] = obs ? kInfoPending : (uint8_t)SBGPU_INFO_UNOBSERVED;
      sh.dg[p] = obs ? sqrt(h) : 0.0;
      sh.alias[p] = -1, sh.ld[p] = 0.0, sh.piv[p] = 0.0, sh.u[p] = 0.0, sh.se[p] = 0.0;
   }
   __syncthreads();
   for (int i = lane; i < nf; i += T)
      for (int j = 0; j <= i; ++j)
         if (sh.obs[i] && sh.obs[j]) sh.A[info_tri(i, j)] = info_scaled(sh.A[info_tri(i, j)], sh.dg[i], sh.dg[j]);
   __syncthreads();
   // ---- 5: the factorisation, one barrier per column
   for (int j = 0; j < MF; ++j) {
      if (j < nf && sh.obs[j])
         for (int i = j + lane; i < nf; i += T)
            if (sh.obs[i]) {
               const double pj = info_pivot(sh.A, sh.st, j);
               const bool retained = info_retained(pj);
               if (i == j) {
                  sh.piv[j] = pj;
                  if (retained) sh.ld[j] = sqrt(pj), sh.st[j] = SBGPU_INFO_IDENTIFIED;
                  else sh.alias[j] = info_alias_of(sh.A, sh.st, j), sh.st[j] = SBGPU_INFO_ALIASED;
               } else if (retained) {
                  sh.A[info_tri(i, j)] = info_lower(sh.A, sh.st, i, j, sqrt(pj));
               }
            }
      __syncthreads();
   }
   // ---- 6: Y = L_R^-1, a thread per column
   for (int j = lane; j < nf; j += T)
      if (info_in_r(sh.st, j))
         for (int i = j; i < nf; ++i)
            if (info_in_r(sh.st, i)) sh.B[info_tri(i, j)] = info_y(sh.A, sh.ld, sh.B, sh.st, i, j);
   __syncthreads();
   // ---- 7: V and Hinv, a thread per entry
   for (int e = lane; e < ntri; e += T) {
      const int i = info_tri_row(e), j = e - info_tri(i, 0);
      const bool both = info_in_r(sh.st, i) && info_in_r(sh.st, j);
      sh.A[e] = both ? info_hinv(info_v(sh.B, sh.st, nf, i, j), sh.dg[i], sh.dg[j]) : 0.0;
   }
   __syncthreads();
   // ---- 8, 9: u, t, cov
   for (int i = lane; i < nf; i += T)
      if (info_in_r(sh.st, i)) sh.u[i] = info_u(sh.A, sh.st, nf, i);
   __syncthreads();
   if (lane < ntri) {
      const double t = info_t(sh.u, sh.st, nf);
      const bool packed = niso_out <= kInfoMaxFree;
      double *cov = a.cov + (l >= 0 ? a.cov_off[l] : 0);
      for (int e = lane; e < ntri; e += T) {
         const int i = info_tri_row(e), j = e - info_tri(i, 0);
         if (!(info_in_r(sh.st, i) && info_in_r(sh.st, j))) continue;
         const double v = info_cov(sh.A[e], sh.u[i], sh.u[j], t);
         sh.A[e] = v;
         if (packed) cov[info_cov_at(niso, sh.idx[j], sh.idx[i])] = v;
      }
   }
   __syncthreads();
   // ---- 10: se
   for (int j = lane; j < nf; j += T)
      if (info_in_r(sh.st, j)) sh.se[j] = info_se(sh.A[info_tri(j, j)]);
   __syncthreads();
   // ---- 11: the results
   for (int p = lane; p < nf; p += T) {
      const int64_t at = i0 + sh.idx[p];
      double corr = 0.0;
      const int k = info_in_r(sh.st, p) ? info_partner(sh.A, sh.se, sh.st, nf, p, &corr) : -1;
      a.se[at] = sh.se[p], a.partner_corr[at] = corr;
      a.ident[at] = sh.st[p];
      a.alias_of[at] = sh.alias[p] < 0 ? -1 : sh.idx[sh.alias[p]];
      a.partner[at] = k < 0 ? -1 : sh.idx[k];
   }
   for (int64_t j = lane; j < niso_out; j += T)
      if (status != SBGPU_INFO_OK || !info_free(G[j])) {
         a.se[i0 + j] = 0.0, a.partner_corr[i0 + j] = 0.0;
         a.ident[i0 + j] = status == SBGPU_INFO_TOO_WIDE ? SBGPU_INFO_SKIPPED : SBGPU_INFO_NOT_FREE;
         a.alias_of[i0 + j] = -1, a.partner[i0 + j] = -1;
      }
   if (l >= 0 && lane == 0) {
      int32_t rank = 0;
      double min_pivot = 0.0;
      for (int j = 0; j < nf; ++j)
         if (info_in_r(sh.st, j)) {
            if (!rank || sh.piv[j] < min_pivot) min_pivot = sh.piv[j];
            ++rank;
         }
      a.rank[l] = rank, a.min_pivot[l] = min_pivot;
      a.n_free[l] = nf, a.info_status[l] = status;
   }
   __syncthreads(); // (the group's LDS is free for its next locus)
}

using InfoWaveShared = InfoShared<kInfoWaveVals, kInfoWaveVals, 1, kInfoWaveIso>;
using InfoBlockShared = InfoShared<kInfoStage, kInfoStage, kInfoMaxWords, kInfoMaxFree>;

// kInfoWaveLoci loci per workgroup, a wave each
__global__ __launch_bounds__(kInfoThreads) void info_wave_kernel(InfoArgs a)
{
   __shared__ InfoWaveShared sh[kInfoWaveLoci];
   const int wave = threadIdx.x / kInfoWave, lane = threadIdx.x % kInfoWave;
   for (int64_t q = (int64_t)blockIdx.x * kInfoWaveLoci; q < a.n_list; q += (int64_t)gridDim.x * kInfoWaveLoci) {
      int64_t l = q + wave < a.n_list ? a.list[q + wave] : -1;
      if (l >= 0 && !info_wave_form(a.row_off[l + 1] - a.row_off[l], a.iso_off[l + 1] - a.iso_off[l])) l = -1; // (never listed here)
      info_locus<kInfoWave, kInfoWaveVals, kInfoWaveVals, 1, kInfoWaveIso>(a, l, lane, sh[wave]);
   }
}

// a workgroup per locus
__global__ __launch_bounds__(kInfoThreads) void info_block_kernel(InfoArgs a)
{
   __shared__ InfoBlockShared sh;
   for (int64_t q = blockIdx.x; q < a.n_list; q += gridDim.x)
      info_locus<kInfoThreads, kInfoStage, kInfoStage, kInfoMaxWords, kInfoMaxFree>(a, a.list[q], threadIdx.x, sh);
}

} // namespace sb
