// strawberry_amd/csrc/bootstrap_rules.h -- the resampling rule of the EM bootstrap, stated once: the host form
// (bootstrap_host.cpp) and the kernels (bootstrap_device.h) both call these functions, so that the two cannot drift.
//
// A locus has a global id g, rows with counts n_i >= 0, N = sum n_i, and inclusive prefix sums S_i = n_0 + ... + n_i.
// Replicate r (0 <= r < 2^24) under seed s makes N independent draws d = 0 .. N-1.  Draws come in pairs: pair q = d >> 1 is
// one Philox4x32-10 call (Random123 constants) with
//    counter (q & 0xffffffff, (q >> 32) | (r << 8), g & 0xffffffff, g >> 32),   key (s & 0xffffffff, s >> 32);
// the even draw uses u = o0 | o1 << 32, the odd one u = o2 | o3 << 32, t = (u * N) >> 64, and the draw lands on the one
// row i with S_{i-1} <= t < S_i.  The replicate's count of a row is the number of draws that land on it: an integer
// histogram, identical in any order of the draws and for any split of the work; it depends on (g, r, s) and the locus'
// counts only.  N < 2^40 (q < 2^39: its high word leaves bits 8.. of the second counter word to r).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sb {

constexpr int64_t kBootMaxDraws = (int64_t)1 << 40; // N at or above: SBGPU_ESHAPE
constexpr int32_t kBootMaxRep = 1 << 24;            // replicate numbers at or above: SBGPU_EINVAL

__host__ __device__ inline uint32_t boot_mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__host__ __device__ inline void boot_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
   for (int round = 0; round < 10; ++round) {
      const uint32_t hi0 = boot_mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
      const uint32_t hi1 = boot_mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
      c0 = hi1 ^ c1 ^ k0;
      c1 = lo1;
      c2 = hi0 ^ c3 ^ k1;
      c3 = lo0;
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
   }
   out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__host__ __device__ inline uint64_t boot_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
   return __umul64hi(a, b);
#else
   return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The two draws of pair q of locus g in replicate r under seed s: t[0] for draw 2q, t[1] for draw 2q + 1, both in [0, N)
__host__ __device__ inline void boot_draw_pair(int64_t g, int32_t r, uint64_t s, int64_t q, int64_t N, uint64_t t[2])
{
   uint32_t o[4];
   boot_philox((uint32_t)((uint64_t)q & 0xffffffffu), (uint32_t)((uint64_t)q >> 32) | ((uint32_t)r << 8), (uint32_t)((uint64_t)g & 0xffffffffu),
               (uint32_t)((uint64_t)g >> 32), (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32), o);
   t[0] = boot_mulhi64((uint64_t)o[0] | ((uint64_t)o[1] << 32), (uint64_t)N);
   t[1] = boot_mulhi64((uint64_t)o[2] | ((uint64_t)o[3] << 32), (uint64_t)N);
}

// The row a draw lands on: the first i with incl[i] > t (incl: the rows' inclusive prefix sums, incl[n - 1] = N > t).  A row
// whose count is 0 has incl[i] == incl[i - 1] and is never the first.
template <class Prefix>
__host__ __device__ inline int32_t boot_row_of(const Prefix *incl, int32_t n, uint64_t t)
{
   int32_t lo = 0, hi = n - 1;
   while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if ((uint64_t)incl[mid] > t) hi = mid;
      else lo = mid + 1;
   }
   return lo;
}

// ---- statistics over the replicates of one column x_0 .. x_{B-1} (sbgpu_replicate_stats_*, the FPKM / TPM intervals)
//
// Mean and variance: Welford's recurrence in replicate order, as boot_stats_kernel states it (step k is 0-based here):
//    m_k = m_{k-1} + (x_k - m_{k-1}) / (k + 1),   M2_k = M2_{k-1} + (x_k - m_{k-1}) (x_k - m_k),   var = M2 / (B - 1)  (0 for B = 1).
// Order statistics: the column sorted ascending under <, NaNs last; lo / hi are the elements at two 0-based integer positions,
// no interpolation.  The order is made total by sorting boot_sort_key(x), an unsigned integer that rises with x: -0.0 sorts in
// front of +0.0, a NaN of either sign behind +infinity (by its payload).  boot_key_value gives the element back: its own bits,
// except that a NaN comes back with the sign bit cleared.  The key of all ones is the padding of the kernel's sorting network:
// it sorts behind (or, for the one NaN with these bits, equal to) every element.
constexpr int32_t kBootMaxStatRep = 1024; // replicates of one column the kernel sorts in a wave's registers; above: SBGPU_ESHAPE
constexpr uint64_t kBootKeyPad = ~(uint64_t)0;

__host__ __device__ inline void boot_welford_step(double x, int32_t step, double &m, double &q)
{
   const double d = x - m;
   m = m + d / (double)(step + 1);
   q = q + d * (x - m);
}
__host__ __device__ inline double boot_welford_var(double q, int32_t n_rep) { return n_rep > 1 ? q / (double)(n_rep - 1) : 0.0; }

__host__ __device__ inline uint64_t boot_sort_key(double x)
{
   uint64_t b;
   __builtin_memcpy(&b, &x, 8);
   if (x != x) b &= ~((uint64_t)1 << 63);
   return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}
__host__ __device__ inline double boot_key_value(uint64_t k)
{
   const uint64_t b = (k >> 63) ? (k & ~((uint64_t)1 << 63)) : ~k;
   double x;
   __builtin_memcpy(&x, &b, 8);
   return x;
}
// The TPM of one replicate's isoform: the expression tpm_kernel (sbgpu_api.hip) evaluates
__host__ __device__ inline double boot_tpm_value(double fpkm, int32_t keep, double total) { return keep ? 1e6 * fpkm / total : 0.0; }

// ---- abundances per locus (sbgpu_locus_abundance_*, the locus columns of sbgpu_locus_bootstrap_device)
//
// Locus l owns isoforms j0 = iso_off[l] .. j1 - 1 = iso_off[l + 1] - 1.  Its FPKM starts at 0.0 and adds fpkm[j] over the
// isoforms with keep[j] != 0 in isoform order -- the isoforms abundance_kernel's own kept-FPKM sum takes --, `kept` counts
// them; a locus without isoforms gives 0.0 and 0.  The order of the additions is the rule; only the loads are grouped, four
// at a time as abundance_kernel's are.  The locus' TPM is boot_tpm_value with `kept` as the flag.
__host__ __device__ inline void boot_locus_sum(const double *fpkm, const int32_t *keep, int64_t j0, int64_t j1, double &sum, int32_t &kept)
{
   double acc = 0.0;
   int32_t n = 0;
   for (int64_t jb = j0; jb < j1; jb += 4) {
      double f[4];
      int32_t kk[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
         const bool in = jb + u < j1;
         f[u] = in ? fpkm[jb + u] : 0.0;
         kk[u] = in ? keep[jb + u] : 0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
         if (kk[u]) { // (a slot past the locus' end holds keep 0)
            acc += f[u];
            ++n;
         }
      }
   }
   sum = acc, kept = n;
}
__host__ __device__ inline double boot_locus_tpm(double locus_fpkm, int32_t kept, double total) { return boot_tpm_value(locus_fpkm, kept, total); }

} // namespace sb
