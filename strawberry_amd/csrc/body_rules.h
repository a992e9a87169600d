// strawberry_amd/csrc/body_rules.h -- the decisions of the transcript-body coverage profile (include/sbgpu.h: sbgpu_body_profile_*;
// DESIGN 3.26), as functions the host form (body_host.cpp) and the kernels (body_device.h) both call, so that the two forms
// cannot drift:
//   - the positional bin of a transcript coordinate, a bin's first coordinate and width, the reported index (body_bin,
//     body_bin_first, body_bin_width, body_report),
//   - what one (hit, candidate) pair adds to the candidate's bins (body_walk),
//   - an isoform's total, centre and coefficient of variation from its finished bins (body_iso),
//   - the length class of an isoform (body_class).
// Who is assigned, to which candidates and with what posterior is assign_rules.h's; the weight of a pair is coverage_rules.h's
// cov_weight; who is kept is context_rules.h's.  Free of HIP under a plain C++ compiler; compiled under -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#include "coverage_rules.h"

namespace sb {

constexpr int kBodyMaxPos = SBGPU_BODY_MAX_POS;

// floor(n / d) for 0 <= n, 0 < d: the rule fixes the quotient, not the instruction.  Most isoforms are a few kilobases and P is at
// most 100, so both operands nearly always fit 32 bits, where the division is a fraction of the 64-bit one's cost on the device;
// the 64-bit one serves the rest (an isoform of 2^26 bases at P = 100).
__host__ __device__ inline int64_t body_div(int64_t n, int64_t d)
{
   return (((uint64_t)n | (uint64_t)d) >> 32) == 0 ? (int64_t)((uint32_t)n / (uint32_t)d) : n / d;
}

// q(t) = floor(t * P / L), 0 <= t < L
__host__ __device__ inline int body_bin(int64_t t, int P, int64_t L) { return (int)body_div(t * P, L); }
// The first coordinate of bin q: ceil(q * L / P); q = P gives L
__host__ __device__ inline int64_t body_bin_first(int q, int P, int64_t L) { return body_div((int64_t)q * L + (P - 1), P); }
// The bases of bin q (0 where L < P leaves it empty)
__host__ __device__ inline int64_t body_bin_width(int q, int P, int64_t L) { return body_bin_first(q + 1, P, L) - body_bin_first(q, P, L); }
// The reported index of bin q on strand 0 (unknown), 1 (+), 2 (-); its own inverse
__host__ __device__ inline int body_report(int q, int P, int strand) { return strand == 2 ? P - 1 - q : q; }
// c = (L >= 1000) + (L >= 2000) + (L >= 4000)
__host__ __device__ inline int body_class(int64_t L) { return (L >= 1000) + (L >= 2000) + (L >= 4000); }

// One (hit, candidate) pair: the hit's features (sorted, disjoint: nf of them) against the candidate's exons (sorted, disjoint: ne
// of them, closed coordinates; exon_pre[e]: the total length of the exons before e; L: of all of them), one forward merge as
// cov_walk's: `e`, the first exon a later feature can still touch, only moves forward, so the transcript coordinate t only grows
// and so does q(t).  The walk carries the bin q it is in, that bin's last coordinate and n, the S_MATCH bases inside the exons it
// has seen there; when q advances -- and when the features are used up -- it calls add(q, w * (double)n) where n != 0: once per
// bin.  q is the bin before orientation (the caller reports it: body_report).
template <class Add>
__host__ __device__ inline void body_walk(const uint8_t *code, const uint32_t *left, const uint32_t *right, int nf, const uint32_t *exon_left,
                                          const uint32_t *exon_right, const int64_t *exon_pre, int ne, int64_t L, int P, double w, Add &&add)
{
   int e = 0, q = -1;
   int64_t q_last = -1, n = 0; // the last coordinate of bin q; the bases counted in it so far
   for (int f = 0; f < nf && e < ne; ++f) {
      if (code[f] != kCovMatch) continue;
      const int64_t fl = left[f], fr = right[f];
      while (e < ne && (int64_t)exon_right[e] < fl) ++e; // an exon that ends in front of the feature is finished
      for (int k = e; k < ne && (int64_t)exon_left[k] <= fr; ++k) {
         const int64_t xl = exon_left[k], xr = exon_right[k];
         const int64_t lo = fl > xl ? fl : xl, hi = fr < xr ? fr : xr;
         if (hi < lo) continue;
         int64_t t0 = exon_pre[k] + (lo - xl);
         const int64_t t1 = exon_pre[k] + (hi - xl);
         if (t0 > q_last) { // (a gap, an intron of the hit, bases outside the exons: the coordinate has left the bin)
            if (n != 0) add(q, w * (double)n);
            n = 0, q = body_bin(t0, P, L), q_last = body_bin_first(q + 1, P, L) - 1;
         }
         while (t1 > q_last && q < P - 1) { // the stretch runs on into the next bin (an empty one, L < P, is passed with n = 0)
            n += q_last - t0 + 1;
            if (n != 0) add(q, w * (double)n);
            n = 0, t0 = q_last + 1, ++q, q_last = body_bin_first(q + 1, P, L) - 1;
         }
         n += t1 - t0 + 1;
      }
   }
   if (n != 0) add(q, w * (double)n);
}

// body_total, body_center, body_cv of one isoform from its FINISHED bins, bases[P] in reported order, taken in ascending p:
//   total  = the ascending sum;
//   center = (sum_p bases_p * (double)(2p + 1)) / ((double)(2P) * total);
//   cv     over the bins of non-zero width wd_p (reported bin p is bin body_report(p) of the isoform): depth_p = bases_p / (double)wd_p,
//            m their mean, sqrt(mean of (depth_p - m)^2) / m;
//   center = cv = -1.0 exactly where total is exactly 0.0.
struct BodyIso {
   double total, center, cv;
};
__host__ __device__ inline BodyIso body_iso(const double *bases, int P, int64_t L, int strand)
{
   BodyIso o;
   double s = 0.0, c = 0.0;
   for (int p = 0; p < P; ++p) s += bases[p];
   o.total = s, o.center = -1.0, o.cv = -1.0;
   if (s == 0.0) return o;
   for (int p = 0; p < P; ++p) c += bases[p] * (double)(2 * p + 1);
   o.center = c / ((double)(2 * P) * s);
   double m = 0.0, v = 0.0;
   int nz = 0;
   for (int p = 0; p < P; ++p) {
      const int64_t wd = body_bin_width(body_report(p, P, strand), P, L);
      if (wd != 0) m += bases[p] / (double)wd, ++nz;
   }
   m = m / (double)nz;
   for (int p = 0; p < P; ++p) {
      const int64_t wd = body_bin_width(body_report(p, P, strand), P, L);
      if (wd == 0) continue;
      const double d = bases[p] / (double)wd - m;
      v += d * d;
   }
   o.cv = sqrt(v / (double)nz) / m;
   return o;
}

// L_j of every isoform into iso_len [n_iso] and pre_e of every exon into exon_pre [exon_off[n_iso]]: once per call, on the host
inline void body_lengths(const int64_t *exon_off, const uint32_t *exon_left, const uint32_t *exon_right, int64_t n_iso, int64_t *exon_pre, int64_t *iso_len)
{
   for (int64_t i = 0; i < n_iso; ++i) {
      int64_t L = 0;
      for (int64_t e = exon_off[i]; e < exon_off[i + 1]; ++e) exon_pre[e] = L, L += (int64_t)exon_right[e] - (int64_t)exon_left[e] + 1;
      iso_len[i] = L;
   }
}

// What the host form works on beside the handle's own arrays (body_host.cpp: body_profile_arrays, the rule on plain arrays)
struct BodyHostIn {
   int64_t n_loci, n_hits, n_bins;
   const int64_t *row_off, *iso_off, *f_off; // [n_loci + 1]
   const int64_t *locus_hit_off;             // [n_loci + 1], or null: the hits did not come grouped by locus
   const int64_t *hit_bin;                   // [n_hits], -1: none
   const int64_t *exon_off;                  // [n_iso + 1]
   const uint32_t *exon_left, *exon_right;
   const int64_t *feat_off;                  // [n_hits + 1]
   const uint8_t *feat_code;
   const uint32_t *feat_left, *feat_right;
   const uint32_t *compat;                   // [n_hits * compat_words]
   int32_t compat_words;
   const double *F, *theta;
   const int32_t *keep, *status;             // or null
   const float *hit_mass;                    // or null
   const uint8_t *iso_strand;                // or null
   int32_t n_pos;
};
int body_profile_arrays(const BodyHostIn &in, sbgpu_body_profile_t *out);

} // namespace sb
