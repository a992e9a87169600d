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

} // namespace sb
