// strawberry_amd/csrc/vb_rules.h -- the decisions of the variational Bayes solve (include/sbgpu.h: sbgpu_em_vb_*),
// as functions the host form (vb_host.cpp) and the kernels (vb_device.h) both call, so that the two forms cannot drift:
//   - digamma (vb_digamma: rule 4),
//   - a column's normalised weight (vb_norm: rule 2), a bin's mass and ratio (vb_bin_mass, vb_ratio), a column's next count
//     (vb_col_sum, vb_next: rule 5), the step norm's term (vb_step_term),
//   - the evidence bound from its sums (vb_elbo: rule 6) and the two per-isoform outputs (vb_share, vb_share_sd: rule 7),
//   - the parameters' defaults and their check (VbParams, vb_params).
// Which bins are live is assign_rules.h's asg_row_live.  Everything here is compiled under -ffp-contract=off; every fused
// operation is written as fma.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/sbgpu.h"
#include "assign_rules.h"

namespace sb {

constexpr int kVbMaxIso = 512;                   // the EM's limit (SBGPU_ESHAPE beyond)
constexpr double kVbAlphaMin = 1e-6, kVbAlphaMax = 1e3;

struct VbParams {
   double alpha, change_limit;
   int32_t max_iter;
};
// NULL: the defaults.  -> false where a parameter is out of range (SBGPU_EINVAL)
inline bool vb_params(const sbgpu_vb_params_t *p, VbParams *out)
{
   out->alpha = p ? p->alpha : 0.01, out->change_limit = p ? p->change_limit : SBGPU_EM_THETA_CHANGE_LIMIT;
   out->max_iter = p ? p->max_iter : SBGPU_EM_MAX_ITER;
   return out->alpha >= kVbAlphaMin && out->alpha <= kVbAlphaMax && out->change_limit > 0.0 && out->max_iter >= 1;
}

// psi(x), x > 0: the recurrence up to x >= 10, then the asymptotic series to y^7 (|error| <= 1.2e-15 max(1, |psi|))
__host__ __device__ inline double vb_digamma(double x)
{
   double s = 0.0;
   while (x < 10.0) s -= 1.0 / x, x += 1.0;
   const double y = 1.0 / (x * x);
   const double t = y * (1.0 / 12 - y * (1.0 / 120 - y * (1.0 / 252 - y * (1.0 / 240 - y * (1.0 / 132 - y * (691.0 / 32760 - y / 12))))));
   return log(x) - 0.5 / x - t + s;
}

// A[i][j] = F[i][j] / s_j for an active column (s_j > 0), 0 otherwise
__host__ __device__ inline double vb_norm(double f, double s) { return s > 0.0 ? f / s : 0.0; }

// d_i = sum_j A[i][j] w_j in ascending j, a chain of fma (the mixture mass of rule 6 is the same chain over exp(lw_j))
__host__ __device__ inline double vb_bin_mass(const double *Arow, const double *w, int niso)
{
   double d = 0.0;
   for (int j = 0; j < niso; ++j) d = fma(Arow[j], w[j], d);
   return d;
}
// r_i: a bin without fragments gives 0 whatever its mass
__host__ __device__ inline double vb_ratio(int32_t n, double d) { return n > 0 ? (double)n / d : 0.0; }
// a live bin with fragments and no mass ends the solve (SBGPU_EM_DENOM_ZERO)
__host__ __device__ inline bool vb_denom_zero(int32_t n, double d) { return n > 0 && d == 0.0; }

// sum_i A[i][j] r_i over the live bins in ascending i, a chain of fma.  r[i] < 0 marks a bin that is not live (a ratio is
// never negative); A: the locus' normalised weights, row-major.
__host__ __device__ inline double vb_col_sum(const double *A, const double *r, int nb, int niso, int j)
{
   double acc = 0.0;
   for (int i = 0; i < nb; ++i)
      if (!(r[i] < 0.0)) acc = fma(A[(int64_t)i * niso + j], r[i], acc);
   return acc;
}
__host__ __device__ inline double vb_next(double w, double col_sum) { return w * col_sum; }
// sq + (c' - c)^2
__host__ __device__ inline double vb_step_term(double c_next, double c, double sq)
{
   const double d = c_next - c;
   return fma(d, d, sq);
}

// Rule 6 from its sums.  bins: sum of n_i log(mass_i); lg: sum of lgamma(alpha + c_j); cl: sum of c_j lw_j (over the active j)
__host__ __device__ inline double vb_elbo(double bins, double a0, double lg, double cl, int32_t n_active, double alpha)
{
   const double ka = (double)n_active;
   return bins - (lgamma(a0) - lg - lgamma(ka * alpha) + ka * lgamma(alpha) + cl);
}
__host__ __device__ inline double vb_a0(int32_t n_active, double alpha, int64_t n_frag) { return (double)n_active * alpha + (double)n_frag; }
__host__ __device__ inline double vb_share(double alpha, double c, double a0) { return (alpha + c) / a0; }
__host__ __device__ inline double vb_share_sd(double alpha, double c, double a0)
{
   const double a = alpha + c;
   return sqrt(a * (a0 - a) / (a0 * a0 * (a0 + 1.0)));
}

} // namespace sb
