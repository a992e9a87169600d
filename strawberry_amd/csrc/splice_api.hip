// strawberry_amd/csrc/splice_api.hip -- sbgpu_splice_psi_device / sbgpu_splice_support_device / sbgpu_splice_limits
// (include/sbgpu.h): the PSI of every splicing event for one or many abundance rows, and the events' support from the coverage's
// per-exon arrays, on device arrays as they stand (splice_device.h).  One launch each, asynchronous on the caller's
// stream: no handle, no retention, no scratch slot, no collective.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "splice_device.h"

using sb::api_fail;
using sb::api_fail_hip;

namespace {

// The device table's counts and pointers: all a launcher can check of it
int spl_args(const std::string &who, const sbgpu_ctx_t *c, const sbgpu_splice_events_t *t, sb::SplArgs *a)
{
   if (!c || !t) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (t->n_loci < 0 || t->n_iso < 0 || t->n_exons < 0 || t->n_events < 0 || t->n_incl < 0) return api_fail(SBGPU_EINVAL, who + ": a negative count in the table");
   if (t->n_events > INT32_MAX) return api_fail(SBGPU_ESHAPE, who + ": more than 2^31 - 1 events");
   if (t->n_events && (!t->event_locus || !t->event_kind || !t->event_left || !t->event_right || !t->incl_off || !t->iso_off))
      return api_fail(SBGPU_EINVAL, who + ": the table's events are needed (device arrays: SpliceEvents.to_device)");
   if (t->n_incl && (!t->incl_iso || !t->incl_exon)) return api_fail(SBGPU_EINVAL, who + ": the table's inclusion lists are needed");
   if (t->n_events && t->n_iso && (!t->iso_left || !t->iso_right)) return api_fail(SBGPU_EINVAL, who + ": the table's isoform extents are needed");
   *a = sb::SplArgs{};
   a->n_events = t->n_events, a->n_iso = t->n_iso;
   a->event_locus = t->event_locus, a->event_kind = t->event_kind, a->event_left = t->event_left, a->event_right = t->event_right;
   a->incl_off = t->incl_off, a->incl_iso = t->incl_iso, a->incl_exon = t->incl_exon;
   a->iso_off = t->iso_off, a->iso_left = t->iso_left, a->iso_right = t->iso_right;
   return SBGPU_OK;
}

unsigned spl_grid(int64_t n_events) { return (unsigned)((n_events + sb::kSplThreads - 1) / sb::kSplThreads); }

} // namespace

extern "C" int sbgpu_splice_limits(int64_t out[2])
{
   if (!out) return api_fail(SBGPU_EINVAL, "sbgpu_splice_limits: null argument");
   out[0] = sb::kSplMaskIso, out[1] = sb::kSplThreads;
   return SBGPU_OK;
}

extern "C" int sbgpu_splice_psi_device(sbgpu_ctx_t *c, const sbgpu_splice_events_t *d_events, int64_t n_rows, const double *d_x, const int32_t *d_keep,
                                       double *d_psi, int32_t *d_defined_count, void *stream)
{
   const std::string who = "sbgpu_splice_psi_device";
   sb::SplArgs a;
   if (const int rc = spl_args(who, c, d_events, &a); rc != SBGPU_OK) return rc;
   if (n_rows < 0) return api_fail(SBGPU_EINVAL, who + ": a negative row count");
   if (n_rows > INT32_MAX) return api_fail(SBGPU_ESHAPE, who + ": more than 2^31 - 1 rows");
   if (a.n_events == 0 || (n_rows == 0 && !d_defined_count)) return SBGPU_OK;
   if (n_rows && a.n_iso && !d_x) return api_fail(SBGPU_EINVAL, who + ": d_x is needed");
   if (n_rows && !d_psi) return api_fail(SBGPU_EINVAL, who + ": d_psi is needed");
   a.n_rows = n_rows, a.x = d_x, a.keep = d_keep, a.psi = d_psi, a.defined_count = d_defined_count;
   if (hipError_t e = hipSetDevice(sb::ctx_device(c)); e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   hipLaunchKernelGGL(sb::spl_psi_kernel, dim3(spl_grid(a.n_events)), dim3(sb::kSplThreads), 0, (hipStream_t)stream, a);
   if (hipError_t e = hipGetLastError(); e != hipSuccess) return api_fail_hip(e, "spl_psi_kernel");
   return SBGPU_OK;
}

extern "C" int sbgpu_splice_support_device(sbgpu_ctx_t *c, const sbgpu_splice_events_t *d_events, const double *d_exon_bases,
                                           const double *d_junction_mass, double *d_support, void *stream)
{
   const std::string who = "sbgpu_splice_support_device";
   sb::SplArgs a;
   if (const int rc = spl_args(who, c, d_events, &a); rc != SBGPU_OK) return rc;
   if (a.n_events == 0) return SBGPU_OK;
   if (!d_support) return api_fail(SBGPU_EINVAL, who + ": d_support is needed");
   a.exon_bases = d_exon_bases, a.junction_mass = d_junction_mass, a.support = d_support;
   if (hipError_t e = hipSetDevice(sb::ctx_device(c)); e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   hipLaunchKernelGGL(sb::spl_support_kernel, dim3(spl_grid(a.n_events)), dim3(sb::kSplThreads), 0, (hipStream_t)stream, a);
   if (hipError_t e = hipGetLastError(); e != hipSuccess) return api_fail_hip(e, "spl_support_kernel");
   return SBGPU_OK;
}
