// strawberry_amd/csrc/coverage_rules.h -- the decisions of the isoform-resolved coverage (include/sbgpu.h:
// sbgpu_isoform_coverage_*), as functions the host form (coverage_host.cpp) and the kernels (coverage_device.h)
// both call, so that the two forms cannot drift:
//   - a hit's weight for one candidate (cov_weight),
//   - what one (hit, candidate) pair adds to the candidate's exons and junctions (cov_walk),
//   - the sequenced bases of a hit (cov_matchlen),
//   - an isoform's bases from its exons' finished sums (cov_iso_bases).
// Who is assigned, to which candidates and with what posterior is assign_rules.h's; who is kept is context_rules.h's.
// Everything here is compiled under -ffp-contract=off.
#pragma once

#include <stdint.h>

#include "../../include/sbgpu.h"
#include "assign_rules.h" // (and, through context_rules.h, the HIP runtime where the compiler is HIP's: a plain C++ compiler takes this header too)

namespace sb {

constexpr uint8_t kCovMatch = 0, kCovIntron = 1; // feat_code (include/sbgpu.h: 0 = S_MATCH, 1 = S_INTRON, 2 = S_GAP)

// w(h,j) = (double)m_h * p(j|h), multiplied in that order
__host__ __device__ inline double cov_weight(double mass, double posterior) { return mass * posterior; }

// Total length of a hit's S_MATCH features
__host__ __device__ inline int64_t cov_matchlen(const uint8_t *code, const uint32_t *left, const uint32_t *right, int nf)
{
   int64_t n = 0;
   for (int f = 0; f < nf; ++f)
      if (code[f] == kCovMatch) n += (int64_t)right[f] - (int64_t)left[f] + 1;
   return n;
}

// One (hit, candidate) pair: the hit's features (sorted, disjoint: nf of them) against the candidate's exons (sorted, disjoint:
// ne of them, closed coordinates), one forward merge of the two lists: every feature is read once, and `e`, the first exon a
// later feature can still touch, only moves forward.  For every exon e in ascending order:
//   - ov(h,e), the bases of the hit's S_MATCH features inside [L_e, R_e]; where it is not 0, add_exon(e, w * (double)ov), once,
//     when the exon is finished (a feature ends behind it, or the features are used up);
//   - where e is not the last exon and the hit owns an S_INTRON feature [R_e + 1, L_{e+1} - 1], add_junction(e, w).
template <class AddExon, class AddJunction>
__host__ __device__ inline void cov_walk(const uint8_t *code, const uint32_t *left, const uint32_t *right, int nf, const uint32_t *exon_left,
                                         const uint32_t *exon_right, int ne, double w, AddExon &&add_exon, AddJunction &&add_junction)
{
   int e = 0;
   int64_t ov = 0; // matched bases inside exon e so far
   for (int f = 0; f < nf && e < ne; ++f) {
      const uint8_t c = code[f];
      if (c != kCovMatch && c != kCovIntron) continue;
      const int64_t fl = left[f], fr = right[f];
      // an exon that ends in front of the feature (in front of the base before an intron) is finished
      const int64_t from = c == kCovMatch ? fl : fl - 1;
      while (e < ne && (int64_t)exon_right[e] < from) {
         if (ov != 0) add_exon(e, w * (double)ov);
         ov = 0, ++e;
      }
      if (e == ne) break;
      if (c == kCovIntron) {
         if ((int64_t)exon_right[e] == fl - 1 && e + 1 < ne && (int64_t)exon_left[e + 1] - 1 == fr) add_junction(e, w);
         continue;
      }
      while (e < ne && (int64_t)exon_left[e] <= fr) {
         const int64_t L = exon_left[e], R = exon_right[e];
         const int64_t lo = fl > L ? fl : L, hi = fr < R ? fr : R;
         if (hi >= lo) ov += hi - lo + 1;
         if (R >= fr) break; // the exon does not end inside the feature: a later feature may add to it, or be the intron behind it
         if (ov != 0) add_exon(e, w * (double)ov);
         ov = 0, ++e;
      }
   }
   if (e < ne && ov != 0) add_exon(e, w * (double)ov);
}

// iso_bases[j]: the finished exon sums of the isoform in ascending order
__host__ __device__ inline double cov_iso_bases(const double *exon_bases, int64_t e0, int64_t e1)
{
   double s = 0.0;
   for (int64_t e = e0; e < e1; ++e) s += exon_bases[e];
   return s;
}

} // namespace sb
