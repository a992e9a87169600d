// strawberry_amd/csrc/fit_device.h -- the model fit (include/sbgpu.h: sbgpu_em_fit_device, sbgpu_model_fit_device) from the
// arrays a batch has in HBM anyway.  The live flags and the gains are asg_column_kernel's (assign_device.h,
// launched unchanged through sb::asg_launch_column_pass); the pass below makes everything else.
//
// One locus is served by a GROUP of T threads: a wave (T = 64; fit_wave_kernel, kFitWaveLoci loci per workgroup) for a locus
// of at most kFitWaveVals weights, a workgroup (T = 256; fit_block_kernel) for a larger one.  Three steps per locus:
//   A  a thread per bin (bins t, t + T, ... in ascending order): the bin's mass d_b, one walk along its row in ascending j,
//      so d_b has the host form's bits; the counts, P and D as the thread's partial sums.  The ratio n_b / d_b goes to LDS
//      (s_q; -1.0 marks a live bin that is not possible, -2.0 one that is not live), d_b itself waits in expected[b].
//      -> the group's reduction gives D, M = n_live - n_impossible, P.
//   B  the same thread per bin: expected, resid, the terms of loglik / deviance / pearson, the argmax of |resid|.
//      -> the group's reduction; lane 0 stores the locus' eight results.
//   C  a thread per column (independent of B: it reads s_q only): c_j and the score's sum, one walk down the column in
//      ascending b, so both sums run over the host form's terms in the host form's order.
// F is read twice (A, C): from LDS where the locus has at most kFitWaveVals (wave form) / kFitStage (workgroup form) weights,
// from global memory beyond.
// THE REDUCTION, a fixed tree (no floating-point atomics; two calls give the same bits): thread t holds the sequential sum
// of its bins t, t + T, ...; inside a wave lane i adds lane i + s for s = 32, 16, 8, 4, 2, 1 (__shfl_down), lane 0 holds the
// wave's sum; a workgroup then adds its four waves' sums as (w0 + w1) + (w2 + w3).  The argmax is merged along the same tree
// by fit_worse (value, then the lower index), which gives the ascending walk's answer in any order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kFitMaxBins = kStageMaxBins, kFitMaxWords = kStageMaxWords; // (stage_host.h)
constexpr int kFitThreads = 256;
constexpr int kFitWave = 64;
constexpr int kFitWaveLoci = kFitThreads / kFitWave; // loci of one workgroup in the wave form
constexpr int kFitWaveVals = 512;  // weights (and so bins, and isoforms) of a locus up to which a wave serves it (4 KB of LDS)
constexpr int kFitStage = 2048;    // weights of a locus the workgroup form stages in LDS (16 KB)
constexpr int kFitGridPerCu = 8;   // workgroups per CU a launch is capped at (the kernels stride over their lists)

__host__ __device__ inline bool fit_wave_form(int64_t nb, int64_t niso) { return nb <= kFitWaveVals && niso <= kFitWaveVals && nb * niso <= kFitWaveVals; }

struct FitArgs {
   int64_t n_list;                 // loci of this launch
   const int32_t *list;            // [n_list] their indices
   const int64_t *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int32_t *count;           // [n_bins]
   const double *F;                // [n_elem]
   const int32_t *keep, *status;   // [n_iso], [n_loci]
   const uint8_t *live;            // [n_bins]  asg_column_kernel's
   const double *gain;             // [n_iso]   asg_column_kernel's
   double *expected, *resid;       // [n_bins]
   double *score;                  // [n_iso]
   double *loglik, *deviance, *pearson;             // [n_loci]
   long long *n_live, *n_dropped, *n_impossible;    // [n_loci] (int64 to the caller)
   int32_t *dof, *worst_bin;       // [n_loci]
};

// lane 0 of the wave gets the tree's sum (see the head of this file)
template <class V>
__device__ inline V fit_wave_sum(V v)
{
   for (int s = kFitWave / 2; s >= 1; s >>= 1) v += __shfl_down(v, s, kFitWave);
   return v;
}
__device__ inline void fit_wave_argmax(double &best, int32_t &best_b)
{
   for (int s = kFitWave / 2; s >= 1; s >>= 1) {
      const double r = __shfl_down(best, s, kFitWave);
      const int32_t b = __shfl_down(best_b, s, kFitWave);
      if (fit_worse(r, b, best, best_b)) best = r, best_b = b;
   }
}

// What a group shares.  NQ: ratios, NF: staged weights, NW: kept words, WAVES: waves of the group.
template <int NQ, int NF, int NW, int WAVES>
struct FitShared {
   double q[NQ];
   double F[NF];
   uint32_t keep[NW];
   double red_d[WAVES][5];      // the two rounds' double sums, per wave (a slot is written once per locus)
   long long red_i[WAVES][4];   // round A's integer sums, per wave
   int32_t red_b[WAVES];
};

// One locus by one group of T threads (lane: the thread's index in the group; l < 0: no locus, the barriers only).  Every
// thread of the WORKGROUP reaches every __syncthreads() below, whatever its locus' shape: the barriers' count does not depend
// on the data.
template <int T, int NQ, int NF, int NW>
__device__ inline void fit_locus(const FitArgs &a, int64_t l, int lane, FitShared<NQ, NF, NW, T / kFitWave> &sh)
{
   constexpr int WAVES = T / kFitWave;
   const int wave = lane / kFitWave, wlane = lane % kFitWave;
   int64_t b0 = 0, i0 = 0;
   int nb = 0, niso = 0;
   const double *Fl = nullptr;
   if (l >= 0) {
      b0 = a.row_off[l], i0 = a.iso_off[l];
      nb = (int)min((int64_t)NQ, a.row_off[l + 1] - b0);          // (the launcher refuses, or lists elsewhere, loci beyond)
      niso = (int)min((int64_t)32 * NW, a.iso_off[l + 1] - i0);
      Fl = a.F + a.f_off[l];
      const int words = (niso + 31) >> 5;
      const int32_t st = a.status[l];
      for (int w = lane; w < words; w += T) sh.keep[w] = ctx_kept_word(a.keep + i0, niso, st, w);
      const int n_val = nb * niso; // (<= 5632 * 4096: fits an int)
      if (n_val <= NF) {
         for (int i = lane; i < n_val; i += T) sh.F[i] = Fl[i];
         Fl = sh.F;
      }
   }
   __syncthreads();
   const int words = (niso + 31) >> 5;
   uint32_t any_kept = 0;
   for (int w = 0; w < words; ++w) any_kept |= sh.keep[w];
   const double *G = a.gain + i0;
   // ---- A: the bins' masses
   long long n_live = 0, n_dropped = 0, n_imp = 0, P = 0, A = 0;
   double D = 0.0;
   for (int b = lane; b < nb; b += T) {
      const int32_t n = a.count[b0 + b];
      const bool live = any_kept && a.live[b0 + b];
      double d = 0.0;
      if (live) d = fit_bin_mass(Fl + (int64_t)b * niso, niso, sh.keep, G);
      const bool possible = fit_possible(live, d);
      if (!live) n_dropped += n;
      else n_live += n;
      if (possible) ++P, D += d;
      else if (live) n_imp += n;
      sh.q[b] = possible ? fit_ratio(n, d) : live ? -1.0 : -2.0;
      a.expected[b0 + b] = possible ? d : 0.0; // (d_b waits here for step B: the same thread reads it back)
   }
   if (any_kept)
      for (int j = lane; j < niso; j += T) A += G[j] > 0.0;
   D = fit_wave_sum(D), n_live = fit_wave_sum(n_live), n_dropped = fit_wave_sum(n_dropped), n_imp = fit_wave_sum(n_imp);
   long long PA = fit_wave_sum((P << 32) | A); // (both below 2^31: one sum carries the two)
   if (wlane == 0) {
      sh.red_d[wave][0] = D;
      sh.red_i[wave][0] = n_live, sh.red_i[wave][1] = n_dropped, sh.red_i[wave][2] = n_imp, sh.red_i[wave][3] = PA;
   }
   __syncthreads(); // (s_q is complete, too)
   if constexpr (WAVES == 4) {
      D = (sh.red_d[0][0] + sh.red_d[1][0]) + (sh.red_d[2][0] + sh.red_d[3][0]);
      n_live = sh.red_i[0][0] + sh.red_i[1][0] + sh.red_i[2][0] + sh.red_i[3][0];
      n_dropped = sh.red_i[0][1] + sh.red_i[1][1] + sh.red_i[2][1] + sh.red_i[3][1];
      n_imp = sh.red_i[0][2] + sh.red_i[1][2] + sh.red_i[2][2] + sh.red_i[3][2];
      PA = sh.red_i[0][3] + sh.red_i[1][3] + sh.red_i[2][3] + sh.red_i[3][3];
   } else {
      D = sh.red_d[wave][0];
      n_live = sh.red_i[wave][0], n_dropped = sh.red_i[wave][1], n_imp = sh.red_i[wave][2], PA = sh.red_i[wave][3];
   }
   const long long M = n_live - n_imp;
   // ---- B: expected, resid and the locus' sums
   double loglik = 0.0, dev = 0.0, pearson = 0.0, best = -1.0;
   int32_t best_b = INT32_MAX;
   for (int b = lane; b < nb; b += T) {
      const bool possible = sh.q[b] >= 0.0;
      double e = 0.0, r = 0.0;
      if (possible) {
         const int32_t n = a.count[b0 + b];
         const double d = a.expected[b0 + b];
         e = fit_expected(M, d, D);
         r = fit_resid(n, e);
         if (n > 0) loglik += fit_loglik_term(n, d, D), dev += fit_deviance_term(n, e);
         pearson += r * r;
         const double ra = fabs(r);
         if (fit_worse(ra, b, best, best_b)) best = ra, best_b = b;
      }
      a.expected[b0 + b] = e;
      a.resid[b0 + b] = r;
   }
   loglik = fit_wave_sum(loglik), dev = fit_wave_sum(dev), pearson = fit_wave_sum(pearson);
   fit_wave_argmax(best, best_b);
   if constexpr (WAVES == 4) {
      if (wlane == 0) sh.red_d[wave][1] = loglik, sh.red_d[wave][2] = dev, sh.red_d[wave][3] = pearson, sh.red_d[wave][4] = best, sh.red_b[wave] = best_b;
   }
   // ---- C: the columns' scales and the score (reads s_q and F only)
   for (int j = lane; j < niso; j += T) {
      double c = 0.0, s = 0.0;
      for (int b = 0; b < nb; ++b) {
         const double q = sh.q[b];
         if (q > -2.0) {
            const double f = Fl[(int64_t)b * niso + j];
            c += f;
            if (q >= 0.0) s += fit_score_term(q, f);
         }
      }
      a.score[i0 + j] = fit_score(s, c, (sh.keep[j >> 5] >> (j & 31)) & 1u);
   }
   __syncthreads(); // (round B's sums are in LDS; nobody reads s_q, s_F or the kept words after this)
   if (l >= 0 && lane == 0) {
      if constexpr (WAVES == 4) {
         loglik = (sh.red_d[0][1] + sh.red_d[1][1]) + (sh.red_d[2][1] + sh.red_d[3][1]);
         dev = (sh.red_d[0][2] + sh.red_d[1][2]) + (sh.red_d[2][2] + sh.red_d[3][2]);
         pearson = (sh.red_d[0][3] + sh.red_d[1][3]) + (sh.red_d[2][3] + sh.red_d[3][3]);
         for (int w = 1; w < 4; ++w)
            if (fit_worse(sh.red_d[w][4], sh.red_b[w], best, best_b)) best = sh.red_d[w][4], best_b = sh.red_b[w];
      }
      a.loglik[l] = loglik, a.deviance[l] = 2.0 * dev, a.pearson[l] = pearson;
      a.n_live[l] = n_live, a.n_dropped[l] = n_dropped, a.n_impossible[l] = n_imp;
      a.dof[l] = any_kept ? fit_dof(PA >> 32, PA & 0xffffffffll) : 0;
      a.worst_bin[l] = best_b == INT32_MAX ? -1 : best_b;
   }
   __syncthreads(); // (the sums are read: the group's LDS is free for its next locus)
}

using FitWaveShared = FitShared<kFitWaveVals, kFitWaveVals, kFitWaveVals / 32, 1>;
using FitBlockShared = FitShared<kFitMaxBins, kFitStage, kFitMaxWords, kFitThreads / kFitWave>;

// kFitWaveLoci loci per workgroup, a wave each
__global__ __launch_bounds__(kFitThreads) void fit_wave_kernel(FitArgs a)
{
   __shared__ FitWaveShared sh[kFitWaveLoci];
   const int wave = threadIdx.x / kFitWave, lane = threadIdx.x % kFitWave;
   for (int64_t q = (int64_t)blockIdx.x * kFitWaveLoci; q < a.n_list; q += (int64_t)gridDim.x * kFitWaveLoci) {
      int64_t l = q + wave < a.n_list ? a.list[q + wave] : -1;
      if (l >= 0 && !fit_wave_form(a.row_off[l + 1] - a.row_off[l], a.iso_off[l + 1] - a.iso_off[l])) l = -1; // (never listed here)
      fit_locus<kFitWave, kFitWaveVals, kFitWaveVals, kFitWaveVals / 32>(a, l, lane, sh[wave]);
   }
}

// a workgroup per locus
__global__ __launch_bounds__(kFitThreads) void fit_block_kernel(FitArgs a)
{
   __shared__ FitBlockShared sh;
   for (int64_t q = blockIdx.x; q < a.n_list; q += gridDim.x)
      fit_locus<kFitThreads, kFitMaxBins, kFitStage, kFitMaxWords>(a, a.list[q], threadIdx.x, sh);
}

} // namespace sb
