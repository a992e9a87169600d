// strawberry_amd/csrc/vb_device.h -- the variational Bayes solve (include/sbgpu.h: sbgpu_em_vb_device, sbgpu_model_vb_device;
// DESIGN 3.31) from the arrays a batch has in HBM anyway.  The solve is a dependent chain of iterations, so a locus' state does
// not leave the CU between them: its normalised weights A are made once, every iteration runs on LDS, the outputs are written once.
//
// One locus is served by a GROUP of T threads: a wave (T = 64; vb_wave_kernel, kVbWaveLoci loci per workgroup) for a locus of at
// most kVbWaveVals weights, a workgroup (T = 256; vb_block_kernel) for a larger one.  A group's LDS is one buffer of doubles cut
// into r [nb] (the bins' ratios; -1.0 marks a bin that is not live), w [K], c [K] (-1.0 marks an inactive column) and -- where
// nb K + nb + 2 K doubles fit it (always in the wave form; kVbStage in the workgroup form) -- A [nb K].  A larger locus keeps A
// in the call's scratch, at the batch's own f_off: the same loop, reading global memory.
// kVbStage: 64 KiB of LDS per workgroup is what a kernel gets without asking; two such workgroups are resident on a CU's
// 160 KiB, and a third would not fit beside them even at half the buffer, so the buffer takes what 64 KiB leave beside the
// reduction's slots: 8064 doubles (a 400-isoform locus of 18 bins, a 65-isoform locus of 120).
// The wave form: 1544 doubles (nb K <= 512 gives nb + 2 K <= 1025) per wave, 48.3 KiB per workgroup, three workgroups per CU.
// One iteration (rule 5):
//   P  a thread per isoform (j = t, t + T, ...): p_j = psi(alpha + c_j) into w[j]; the group's maximum (exact in any order)
//   W  the same thread: w[j] = exp(p_j - m)
//   E  a thread per bin (i = t, t + T, ...): d_i, one walk along A's row in ascending j; r[i]; the DENOM_ZERO flag, or-ed
//   M  a thread per isoform: c'_j, one walk down A's column in ascending i, into w[j] (its last reader was step E); the step
//      norm's terms; the group's sum; then c[j] = w[j] unless the locus stops.
// So d_i and c'_j are the host form's operation for operation.
// THE REDUCTION, a fixed tree (no atomics; two calls give the same bits, wherever the locus stands in the batch): thread t holds
// the sequential sum of its isoforms (bins) t, t + T, ...; inside a wave lane i adds lane i + s for s = 32, 16, 8, 4, 2, 1
// (__shfl_down), lane 0 holds the wave's sum; a workgroup then adds its four waves' sums as (w0 + w1) + (w2 + w3).  The step
// norm, the ELBO's three sums (bins, lgamma, c lw) and N go through it.
// The loci of a workgroup of the wave form finish at different iterations: a finished locus is masked (its wave runs the
// barriers only), and the workgroup leaves when all are done.  Every thread of the WORKGROUP reaches every __syncthreads()
// below: their number per iteration does not depend on the data, and the loop's condition is __syncthreads_or's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage_host.h"
#include "vb_rules.h"

namespace sb {

constexpr int kVbMaxBins = kStageMaxBins;
constexpr int kVbThreads = 256;
constexpr int kVbWave = 64;
constexpr int kVbWaveLoci = kVbThreads / kVbWave; // loci of one workgroup in the wave form
constexpr int kVbWaveVals = 512;   // weights of a locus up to which a wave serves it
constexpr int kVbWaveBuf = 1544;   // doubles of LDS per wave: nb K + nb + 2 K <= 512 + 1025
constexpr int kVbStage = 8064;     // doubles of LDS of the workgroup form (63 KiB): A stays in LDS where nb K + nb + 2 K fit
constexpr int kVbGridPerCu = 8;    // workgroups per CU a launch is capped at (the kernels stride over their lists)

__host__ __device__ inline bool vb_wave_form(int64_t nb, int64_t niso) { return nb * niso <= kVbWaveVals; }
__host__ __device__ inline int64_t vb_lds_need(int64_t nb, int64_t niso) { return nb * niso + nb + 2 * niso; }
__host__ __device__ inline bool vb_staged(int64_t nb, int64_t niso) { return vb_lds_need(nb, niso) <= kVbStage; }
static_assert(kVbWaveVals + 2 * kVbWaveVals + 1 <= kVbWaveBuf, "a wave's buffer holds every locus of the wave form");
static_assert(kVbMaxBins + 2 * kVbMaxIso <= kVbStage, "the workgroup's buffer holds r, w and c of the largest locus");

struct VbArgs {
   int64_t n_list;                 // loci of this launch
   const int32_t *list;            // [n_list] their indices
   const int64_t *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int32_t *count;           // [n_bins]
   const double *F;                // [n_elem]
   double *norm;                   // [n_elem] A of the loci that do not fit LDS (null where the launch has none)
   double alpha, change_limit;
   int32_t max_iter;
   double *out_count, *out_share, *out_sd; // [n_iso]
   int32_t *status, *iters, *n_active;     // [n_loci]
   double *elbo;                           // [n_loci]
   long long *n_frag;                      // [n_loci] (int64 to the caller)
};

template <int WAVES>
struct VbRed {
   double d[WAVES][3]; // the waves' sums: slot k is written once per iteration, and barriers lie between its reads and its next write
   long long i[WAVES][2];
};

// The group's sum along the tree at the head of this file, in every thread.  WAVES == 1: no barrier.  WAVES == 4: one
// __syncthreads(); `slot` (wave, k) is written here and must not be read by anybody any more.
template <int WAVES, class V>
__device__ inline V vb_group_sum(V v, V *slot, int stride, int wave, int wlane)
{
   for (int s = kVbWave / 2; s >= 1; s >>= 1) v += __shfl_down(v, s, kVbWave);
   if constexpr (WAVES == 1) return __shfl(v, 0, kVbWave);
   else {
      if (wlane == 0) slot[wave * stride] = v;
      __syncthreads();
      return (slot[0] + slot[stride]) + (slot[2 * stride] + slot[3 * stride]);
   }
}
template <int WAVES>
__device__ inline double vb_group_max(double v, double *slot, int stride, int wave, int wlane)
{
   for (int s = kVbWave / 2; s >= 1; s >>= 1) v = fmax(v, __shfl_down(v, s, kVbWave));
   if constexpr (WAVES == 1) return __shfl(v, 0, kVbWave);
   else {
      if (wlane == 0) slot[wave * stride] = v;
      __syncthreads();
      return fmax(fmax(slot[0], slot[stride]), fmax(slot[2 * stride], slot[3 * stride]));
   }
}
// A barrier of the workgroup that also tells the group whether one of ITS threads raised `flag`
template <int WAVES>
__device__ inline bool vb_group_or(bool flag)
{
   if constexpr (WAVES == 1) {
      __syncthreads();
      return __any(flag);
   } else
      return __syncthreads_or(flag);
}

// One locus by one group of T threads (lane: the thread's index in the group; l < 0: no locus, the barriers only).  buf: the
// group's LDS, cap doubles.
template <int T>
__device__ inline void vb_locus(const VbArgs &a, int64_t l, int lane, double *buf, int cap, VbRed<T / kVbWave> &red)
{
   constexpr int WAVES = T / kVbWave;
   const int wave = lane / kVbWave, wlane = lane % kVbWave;
   int64_t b0 = 0, i0 = 0;
   int nb = 0, niso = 0;
   const double *Fl = nullptr;
   if (l >= 0) {
      b0 = a.row_off[l], i0 = a.iso_off[l];
      nb = (int)min((int64_t)kVbMaxBins, a.row_off[l + 1] - b0); // (the launcher refuses loci beyond)
      niso = (int)min((int64_t)kVbMaxIso, a.iso_off[l + 1] - i0);
      Fl = a.F + a.f_off[l];
      // (never: a locus of another form's list, or one that needs the scratch in a launch without it)
      if (nb + 2 * niso > cap || (vb_lds_need(nb, niso) > cap && !a.norm)) nb = 0, niso = 0;
   }
   const int n_val = nb * niso; // (<= 5632 * 512: fits an int)
   double *r = buf, *w = buf + nb, *c = w + niso;
   double *A = vb_lds_need(nb, niso) <= cap ? c + niso : a.norm + a.f_off[l];
   const int32_t *cnt = a.count + b0;
   // ---- rules 1-3: the live bins and N
   long long N = 0, n_live = 0;
   for (int i = lane; i < nb; i += T) {
      const bool live = asg_row_live(Fl + (int64_t)i * niso, niso);
      r[i] = live ? 0.0 : -1.0;
      if (live) N += cnt[i], ++n_live;
   }
   N = vb_group_sum<WAVES>(N, &red.i[0][0], 2, wave, wlane);
   n_live = vb_group_sum<WAVES>(n_live, &red.i[0][1], 2, wave, wlane);
   __syncthreads(); // (r is complete)
   long long ka_l = 0;
   for (int j = lane; j < niso; j += T) {
      double sj = 0.0;
      for (int i = 0; i < nb; ++i)
         if (!(r[i] < 0.0)) sj += Fl[(int64_t)i * niso + j];
      w[j] = sj;
      ka_l += sj > 0.0;
   }
   __syncthreads(); // (the columns' sums are complete; red.i's first use is read)
   const int32_t ka = (int32_t)vb_group_sum<WAVES>(ka_l, &red.i[0][0], 2, wave, wlane); // (0 where no bin is live)
   for (int e = lane; e < n_val; e += T) A[e] = vb_norm(Fl[e], w[e % niso]);
   __syncthreads(); // (A is complete, w's sums are read by everybody)
   const bool solved = n_live > 0 && N > 0;
   for (int j = lane; j < niso; j += T) c[j] = w[j] > 0.0 ? (solved ? (double)N / (double)ka : 0.0) : -1.0;
   int32_t status = !n_live ? SBGPU_EM_INIT_EMPTY : !solved ? SBGPU_EM_OK : SBGPU_EM_MAXITER, iters = n_live && !solved ? 1 : 0;
   bool run = l >= 0 && solved;
   // ---- rule 5
   while (__syncthreads_or(run)) {
      if (run && iters == a.max_iter) run = false; // (status stays SBGPU_EM_MAXITER)
      if (run) ++iters;
      double m = -INFINITY;
      if (run)
         for (int j = lane; j < niso; j += T)
            if (!(c[j] < 0.0)) w[j] = vb_digamma(a.alpha + c[j]), m = fmax(m, w[j]);
      m = vb_group_max<WAVES>(m, &red.d[0][0], 3, wave, wlane);
      if (run)
         for (int j = lane; j < niso; j += T) w[j] = c[j] < 0.0 ? 0.0 : exp(w[j] - m);
      __syncthreads(); // (w is complete)
      bool zero = false;
      if (run)
         for (int i = lane; i < nb; i += T) {
            if (r[i] < 0.0) continue;
            const double d = vb_bin_mass(A + (int64_t)i * niso, w, niso);
            zero |= vb_denom_zero(cnt[i], d);
            r[i] = vb_ratio(cnt[i], d);
         }
      zero = vb_group_or<WAVES>(zero); // (r is complete)
      if (run && zero) status = SBGPU_EM_DENOM_ZERO, run = false;
      double sq = 0.0;
      if (run)
         for (int j = lane; j < niso; j += T) {
            if (c[j] < 0.0) continue;
            const double cn = vb_next(w[j], vb_col_sum(A, r, nb, niso, j));
            sq = vb_step_term(cn, c[j], sq);
            w[j] = cn;
         }
      sq = vb_group_sum<WAVES>(sq, &red.d[0][1], 3, wave, wlane);
      if (run && sqrt(sq) < a.change_limit) status = SBGPU_EM_OK, run = false;
      if (run)
         for (int j = lane; j < niso; j += T)
            if (!(c[j] < 0.0)) c[j] = w[j];
   }
   // ---- rule 6 (every thread holds its own c[j] and w[j]; r's marks are all the bins' walk needs)
   const double a0 = vb_a0(ka, a.alpha, N), psi0 = solved ? vb_digamma(a0) : 0.0;
   double lg = 0.0, cl = 0.0, bins = 0.0;
   if (solved)
      for (int j = lane; j < niso; j += T) {
         w[j] = 0.0;
         if (c[j] < 0.0) continue;
         const double lw = vb_digamma(a.alpha + c[j]) - psi0;
         w[j] = exp(lw);
         lg += lgamma(a.alpha + c[j]);
         cl = fma(c[j], lw, cl);
      }
   __syncthreads(); // (w is complete)
   if (solved)
      for (int i = lane; i < nb; i += T)
         if (!(r[i] < 0.0) && cnt[i] > 0) bins += (double)cnt[i] * log(vb_bin_mass(A + (int64_t)i * niso, w, niso));
   bins = vb_group_sum<WAVES>(bins, &red.d[0][0], 3, wave, wlane);
   lg = vb_group_sum<WAVES>(lg, &red.d[0][1], 3, wave, wlane);
   cl = vb_group_sum<WAVES>(cl, &red.d[0][2], 3, wave, wlane);
   // ---- rule 7
   for (int j = lane; j < niso; j += T) {
      const bool on = solved && !(c[j] < 0.0);
      a.out_count[i0 + j] = on ? c[j] : 0.0;
      a.out_share[i0 + j] = on ? vb_share(a.alpha, c[j], a0) : 0.0;
      a.out_sd[i0 + j] = on ? vb_share_sd(a.alpha, c[j], a0) : 0.0;
   }
   if (l >= 0 && lane == 0) {
      a.status[l] = status, a.iters[l] = iters, a.n_active[l] = ka;
      a.elbo[l] = solved ? vb_elbo(bins, a0, lg, cl, ka, a.alpha) : 0.0;
      a.n_frag[l] = n_live ? N : 0;
   }
   __syncthreads(); // (the sums are read and the buffer is free for the group's next locus)
}

// kVbWaveLoci loci per workgroup, a wave each
__global__ __launch_bounds__(kVbThreads) void vb_wave_kernel(VbArgs a)
{
   __shared__ double buf[kVbWaveLoci][kVbWaveBuf];
   __shared__ VbRed<1> red[kVbWaveLoci];
   const int wave = threadIdx.x / kVbWave, lane = threadIdx.x % kVbWave;
   for (int64_t q = (int64_t)blockIdx.x * kVbWaveLoci; q < a.n_list; q += (int64_t)gridDim.x * kVbWaveLoci) {
      int64_t l = q + wave < a.n_list ? a.list[q + wave] : -1;
      if (l >= 0 && !vb_wave_form(a.row_off[l + 1] - a.row_off[l], a.iso_off[l + 1] - a.iso_off[l])) l = -1; // (never listed here)
      vb_locus<kVbWave>(a, l, lane, buf[wave], kVbWaveBuf, red[wave]);
   }
}

// a workgroup per locus
__global__ __launch_bounds__(kVbThreads) void vb_block_kernel(VbArgs a)
{
   __shared__ double buf[kVbStage];
   __shared__ VbRed<kVbThreads / kVbWave> red;
   for (int64_t q = blockIdx.x; q < a.n_list; q += gridDim.x) vb_locus<kVbThreads>(a, a.list[q], threadIdx.x, buf, kVbStage, red);
}

} // namespace sb
