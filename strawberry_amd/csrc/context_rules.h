// strawberry_amd/csrc/context_rules.h -- the decisions of the `-f` fragment-context table
// (Sample::printContext, alignments.cpp:1549-1639), as functions the host form
// (context_host.cpp) and the kernels (context_device.h) both call, so that the two forms cannot drift:
//   - which hits count for a bin (ctx_kept_word, ctx_hit_qualifies),
//   - which isoforms of a row carry the bin's weight (ctx_row_value),
//   - the order of a locus' rows (ctx_key_less).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#elif !defined(__host__) // a plain C++ compiler (a host-only program over stage_host.h): the qualifiers mean nothing there
#define __host__
#define __device__
#endif
#include <stdint.h>

#include "../../include/sbgpu.h"

namespace sb {

// Word w of a locus' kept mask: bit j of word w stands for isoform 32 w + j of the locus; set when the expression filter
// kept it (estimate.cpp:346-355: keep != 0).  A locus whose EM never started (SBGPU_EM_INIT_EMPTY) prints nothing: all zero.
__host__ __device__ inline uint32_t ctx_kept_word(const int32_t *keep_of_locus, int niso, int32_t status, int w)
{
   if (status == SBGPU_EM_INIT_EMPTY) return 0u;
   uint32_t m = 0;
   const int j0 = 32 * w;
   for (int j = 0; j < 32 && j0 + j < niso; ++j)
      if (keep_of_locus[j0 + j] != 0) m |= 1u << j;
   return m;
}

// A hit that landed in a bin counts when it is compatible with a kept isoform (printContext walks the surviving isoforms only).
__host__ __device__ inline bool ctx_hit_qualifies(const uint32_t *compat_of_hit, const uint32_t *kept_mask, int words)
{
   uint32_t any = 0;
   for (int w = 0; w < words; ++w) any |= compat_of_hit[w] & kept_mask[w];
   return any != 0;
}

// Column j of a row: the bin's raw weight where the bin's LAST qualifying hit is compatible with isoform j, else 0
// (estimate.hpp:173-197 fills eb_prob_map from that one hit's isoforms, not from the bin's union).
__host__ __device__ inline double ctx_row_value(const uint32_t *compat_of_last_hit, int j, double weight)
{
   return (compat_of_last_hit[j >> 5] >> (j & 31)) & 1u ? weight : 0.0;
}

// Row order inside a locus: std::map order of the bins' coordinate sets, std::set<pair<uint,uint>> compared
// lexicographically.  A locus' segments are disjoint and numbered by position and bit s of a key stands for segment s, so a
// set's sorted sequence is its set bits from the lowest up.  For A != B let d be the lowest bit where they differ: below d the
// sequences agree; the key that holds d continues with d, the other with its next bit above d (then d is the smaller element
// and the holder is less) or with nothing (then it is a proper prefix of the holder and comes first).
// kw words, word 0 holds the lowest segments.  Strict: false for equal keys.
__host__ __device__ inline bool ctx_key_less(const uint32_t *A, const uint32_t *B, int kw)
{
   int w = 0;
   while (w < kw && A[w] == B[w]) ++w;
   if (w == kw) return false;
   const uint32_t x = A[w] ^ B[w];
   const int d = __builtin_ctz(x);
   const bool a_holds = (A[w] >> d) & 1u;
   const uint32_t *other = a_holds ? B : A;
   bool other_above = d < 31 && (other[w] >> (d + 1)) != 0;
   for (int v = w + 1; v < kw && !other_above; ++v) other_above = other[v] != 0;
   return a_holds ? other_above : !other_above;
}

} // namespace sb
