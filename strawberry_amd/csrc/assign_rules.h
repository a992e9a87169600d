// strawberry_amd/csrc/assign_rules.h -- the decisions of the fragment assignment (include/sbgpu.h: sbgpu_fragment_assign_*;
// the posterior U(i,j) of EmSolver::run, estimate.cpp:449-458, per hit instead of per bin), as functions the host form
// (assign_host.cpp) and the kernels (assign_device.h) both call, so that the two forms cannot drift:
//   - which bins of a locus are live (asg_row_live: the row drop of EmSolver::init, estimate.cpp:377-384),
//   - a column's gain g_j = theta_j / c_j (asg_gain) -- a numerator is g_j * F[b][j] (asg_num): one order of the
//     multiplications for both forms,
//   - a hit's candidates, denominator, MAP isoform and its posterior (asg_hit_map),
//   - the posterior of one candidate (asg_posterior).
// Who is kept is context_rules.h's ctx_kept_word.  Everything here is compiled under -ffp-contract=off.
#pragma once

#include <stdint.h>

#include "../../include/sbgpu.h"
#include "context_rules.h" // (and, through it, the HIP runtime where the compiler is HIP's)

namespace sb {

// A bin is live when one of its raw weights exceeds SBGPU_EM_ROW_EPS (a NaN weight does not).
__host__ __device__ inline bool asg_row_live(const double *row, int niso)
{
   for (int j = 0; j < niso; ++j)
      if (row[j] > SBGPU_EM_ROW_EPS) return true;
   return false;
}

// g_j = theta_j / c_j, c_j the column's sum over the live bins in ascending bin order (the caller's loop); exactly 0.0 for
// an isoform that is not kept or whose column is empty.
__host__ __device__ inline double asg_gain(double theta, double c, bool kept) { return kept && c != 0.0 ? theta / c : 0.0; }

// num_j = theta_j * W[b][j] as (theta_j / c_j) * F[b][j]
__host__ __device__ inline double asg_num(double g, double f) { return g * f; }

// p(j | h)
__host__ __device__ inline double asg_posterior(double g, double f, double den) { return asg_num(g, f) / den; }

struct AsgHit {
   int32_t n_cand;   // |compat(h) & kept(l)|: a fact of the words alone
   int32_t map_iso;  // locus-local, -1: unassigned
   double map_prob;  // 0.0 when unassigned
   double den;       // sum of the candidates' numerators in ascending j (meaningful when assigned)
};

// One hit.  compat: its words; kept: its locus' kept words; g: the locus' gains; row: its bin's raw weights, or null when the
// hit has no bin or the bin is not live.  The first pass of the two over the candidates: the denominator and the argmax
// (strict > in ascending j: the lowest index wins a tie).
__host__ __device__ inline AsgHit asg_hit_map(const uint32_t *compat, const uint32_t *kept, int words, const double *g, const double *row)
{
   AsgHit r = {0, -1, 0.0, 0.0};
   double best = -1.0;
   int best_j = -1;
   for (int w = 0; w < words; ++w) {
      uint32_t m = compat[w] & kept[w];
      r.n_cand += __builtin_popcount(m);
      if (!row) continue;
      while (m) {
         const int j = 32 * w + __builtin_ctz(m);
         m &= m - 1;
         const double num = asg_num(g[j], row[j]);
         r.den += num;
         if (num > best) best = num, best_j = j;
      }
   }
   if (!row || r.n_cand == 0 || !(r.den > 0.0)) return r;
   r.map_iso = best_j;
   r.map_prob = best / r.den;
   return r;
}

} // namespace sb
