// strawberry_amd/csrc/splice_rules.h -- the decisions of the splicing events' PSI (include/sbgpu.h: sbgpu_splice_*),
// as functions the host form (splice_host.cpp) and the kernels (splice_device.h) both call, so that the two forms cannot drift:
//   - whether an isoform's extent spans an event (spl_spans),
//   - one event's PSI under one abundance row: the two sums in the rule's order and the quotient (spl_psi_row, and
//     spl_psi_rows_masks for a locus whose isoforms fit two 64-bit masks),
//   - one event's support from the per-exon arrays (spl_support).
// Free of HIP under a plain C++ compiler; compiled under -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#elif !defined(__host__) // a plain C++ compiler: the qualifiers mean nothing there
#define __host__
#define __device__
#endif

namespace sb {

constexpr int kSplMaskIso = 64; // a locus of at most this many isoforms: an event's inclusion and span sets are two 64-bit masks
constexpr uint8_t kSplExon = 0, kSplIntron = 1;

// Isoform extent [left, right] (0xFFFFFFFF / 0 without exons) against event [a, b]
__host__ __device__ inline bool spl_spans(uint32_t left, uint32_t right, uint32_t a, uint32_t b) { return left <= a && b <= right; }

struct SplPsi {
   double psi;
   bool defined;
};

// tot > 0.0 ? inc / tot : NaN (a NaN tot is not > 0.0)
__host__ __device__ inline SplPsi spl_quotient(double inc, double tot)
{
   SplPsi r;
   r.defined = tot > 0.0;
   r.psi = r.defined ? inc / tot : (double)NAN;
   return r;
}

// One event [a, b] of a locus of niso isoforms under one row: x / keep / iso_left / iso_right point at the locus' first isoform
// (keep may be null), incl_iso[0 .. n_incl) is the event's inclusion list.  inc in list order, tot in ascending j.
__host__ __device__ inline SplPsi spl_psi_row(const double *x, const int32_t *keep, const uint32_t *iso_left, const uint32_t *iso_right, int64_t niso,
                                              uint32_t a, uint32_t b, const int32_t *incl_iso, int64_t n_incl)
{
   double inc = 0.0, tot = 0.0;
   for (int64_t i = 0; i < n_incl; ++i) {
      const int32_t j = incl_iso[i];
      if (!keep || keep[j] != 0) inc += x[j];
   }
   for (int64_t j = 0; j < niso; ++j)
      if (spl_spans(iso_left[j], iso_right[j], a, b) && (!keep || keep[j] != 0)) tot += x[j];
   return spl_quotient(inc, tot);
}

// The same sums for a locus of at most kSplMaskIso isoforms from the two sets as masks (bit j: isoform j of the locus; incl is a
// subset of span), for R rows at once (row r at x + r * stride, keep + r * stride): the inclusion list is ascending in j, so one
// ascending pass adds both sums of every row in the rule's order.  The rows' loads do not depend on each other or on keep (an
// x that is not added is read and dropped), so R of each are in flight: what the device form's row loop is paced by.
template <int R>
__host__ __device__ inline void spl_psi_rows_masks(const double *x, const int32_t *keep, int64_t stride, uint64_t span, uint64_t incl, SplPsi *out)
{
   double inc[R], tot[R];
   for (int r = 0; r < R; ++r) inc[r] = tot[r] = 0.0;
   for (uint64_t m = span; m; m &= m - 1) {
      const int j = __builtin_ctzll(m);
      const bool in = (incl >> j) & 1u;
      int32_t kp[R];
      double v[R];
      for (int r = 0; r < R; ++r) kp[r] = keep ? keep[r * stride + j] : 1;
      for (int r = 0; r < R; ++r) v[r] = x[r * stride + j];
      for (int r = 0; r < R; ++r)
         if (kp[r] != 0) {
            tot[r] += v[r];
            if (in) inc[r] += v[r];
         }
   }
   for (int r = 0; r < R; ++r) out[r] = spl_quotient(inc[r], tot[r]);
}

// The span set of event [a, b] as a mask (niso <= kSplMaskIso)
__host__ __device__ inline uint64_t spl_span_mask(const uint32_t *iso_left, const uint32_t *iso_right, int niso, uint32_t a, uint32_t b)
{
   uint64_t m = 0;
   for (int j = 0; j < niso; ++j)
      if (spl_spans(iso_left[j], iso_right[j], a, b)) m |= (uint64_t)1 << j;
   return m;
}

__host__ __device__ inline uint64_t spl_incl_mask(const int32_t *incl_iso, int64_t n_incl)
{
   uint64_t m = 0;
   for (int64_t i = 0; i < n_incl; ++i) m |= (uint64_t)1 << incl_iso[i];
   return m;
}

// support = 0.0 + v[incl_exon[0]] + ... in list order; v null: 0.0
__host__ __device__ inline double spl_support(const double *v, const int64_t *incl_exon, int64_t n_incl)
{
   double s = 0.0;
   if (v)
      for (int64_t i = 0; i < n_incl; ++i) s += v[incl_exon[i]];
   return s;
}

} // namespace sb
