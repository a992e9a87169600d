// strawberry_amd/csrc/fit_rules.h -- the decisions of the model fit (include/sbgpu.h: sbgpu_em_fit_*, sbgpu_model_fit_device;
// DESIGN 3.22): the mixture mass of every exon bin, which EmSolver::run (estimate.cpp:449-476) computes each iteration and
// discards, and what follows from it -- expected counts, Pearson residuals, likelihood, deviance, degrees of freedom and the
// EM's own score vector -- as functions the host form (fit_host.cpp) and the kernels (fit_device.h) both call, so that the two
// forms cannot drift.  Who is kept, which bins are live, the column scale c_j and the gain g_j ARE the fragment assignment's
// (context_rules.h: ctx_kept_word; assign_rules.h: asg_row_live, asg_gain, asg_num): called here, not restated.
// Everything here is compiled under -ffp-contract=off.
#pragma once

#ifdef __HIPCC__ // (a plain C++ compiler takes this header too: context_rules.h, below, gives it the qualifiers)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>

#include "../../include/sbgpu.h"
#include "assign_rules.h"

namespace sb {

// d_b of a live bin: the kept isoforms' numerators g_j * F[b][j], added in ascending j.  It is the `den` of a hit of the bin
// that is compatible with every kept isoform.
__host__ __device__ inline double fit_bin_mass(const double *row, int niso, const uint32_t *kept, const double *g)
{
   double d = 0.0;
   for (int j = 0; j < niso; ++j)
      if ((kept[j >> 5] >> (j & 31)) & 1u) d += asg_num(g[j], row[j]);
   return d;
}

// A live bin is possible when the kept isoforms give it a positive mass (a NaN mass does not).
__host__ __device__ inline bool fit_possible(bool live, double d) { return live && d > 0.0; }

// expected[b] of a possible bin: M fragments spread by d_b / D
__host__ __device__ inline double fit_expected(int64_t M, double d, double D) { return (double)M * (d / D); }

// the Pearson residual; 0.0 where nothing is expected
__host__ __device__ inline double fit_resid(int32_t n, double e) { return e > 0.0 ? ((double)n - e) / sqrt(e) : 0.0; }

// the terms of loglik and deviance, for a possible bin with n > 0
__host__ __device__ inline double fit_loglik_term(int32_t n, double d, double D) { return (double)n * log(d / D); }
__host__ __device__ inline double fit_deviance_term(int32_t n, double e) { return (double)n * log((double)n / e); }

// score[j]: the ratio n_b / d_b of a possible bin first, then times the raw weight; the column's sum over c_j at the end
__host__ __device__ inline double fit_ratio(int32_t n, double d) { return (double)n / d; }
__host__ __device__ inline double fit_score_term(double q, double f) { return q * f; }
__host__ __device__ inline double fit_score(double s, double c, bool kept) { return kept && c != 0.0 ? s / c : 0.0; }

// dof = max(0, P - 1 - max(0, A - 1)): P possible bins, A isoforms with a positive gain
__host__ __device__ inline int32_t fit_dof(int64_t P, int64_t A)
{
   const int64_t free_par = A > 1 ? A - 1 : 0, v = P - 1 - free_par;
   return v > 0 ? (int32_t)v : 0;
}

// the argmax of |resid| over the possible bins: does (r, b) beat (best, best_b)?  Strict > on the value, the lower index on a
// tie: the result of a walk in ascending b under strict >, whatever the order the candidates are merged in.  Start from
// (-1.0, INT32_MAX); INT32_MAX left at the end means no possible bin: worst_bin = -1.
__host__ __device__ inline bool fit_worse(double r, int32_t b, double best, int32_t best_b) { return r > best || (r == best && b < best_b); }

} // namespace sb
