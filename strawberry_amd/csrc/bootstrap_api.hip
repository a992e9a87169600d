// strawberry_amd/csrc/bootstrap_api.hip -- sbgpu_bootstrap_counts_device / sbgpu_em_bootstrap_device (include/sbgpu.h):
// the EM bootstrap on the device (bootstrap_device.h).  Replicates' counts by the rule of bootstrap_rules.h, the
// existing EM entry replicate after replicate, Welford's recurrence over the replicates' theta.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "bootstrap_device.h"

using sb::api_fail;
using sb::api_fail_hip;

namespace {

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// What depends on the counts alone, shared by all replicates of a call: in the context's bootstrap scratch
struct BootPrep {
   int64_t *head = nullptr;     // [2] fault bits, work items per replicate
   int64_t *total = nullptr;    // [n_loci]
   int32_t *items = nullptr;    // [n_loci]
   int64_t *item_off = nullptr; // [n_loci + 1]
   int64_t *incl = nullptr;     // [n_rows]
   int64_t *locus_id = nullptr; // [n_loci], or null
   int64_t *row_off = nullptr;  // [n_loci + 1] (sbgpu_bootstrap_counts_device: the caller's offsets are host arrays)
   int64_t n_items = 0;         // on the host once prepare() returned
   static size_t bytes(int64_t n_loci, int64_t n_rows, bool ids, bool offsets)
   {
      const size_t nl = (size_t)n_loci, nr = (size_t)n_rows;
      return 256 + up256(nl * 8) + up256(nl * 4) + up256((nl + 1) * 8) + up256(nr * 8) + (ids ? up256(nl * 8) : 0) + (offsets ? up256((nl + 1) * 8) : 0);
   }
   char *lay(char *p, int64_t n_loci, int64_t n_rows, bool ids, bool offsets)
   {
      const size_t nl = (size_t)n_loci, nr = (size_t)n_rows;
      head = (int64_t *)p, p += 256;
      total = (int64_t *)p, p += up256(nl * 8);
      items = (int32_t *)p, p += up256(nl * 4);
      item_off = (int64_t *)p, p += up256((nl + 1) * 8);
      incl = (int64_t *)p, p += up256(nr * 8);
      if (ids) locus_id = (int64_t *)p, p += up256(nl * 8);
      if (offsets) row_off = (int64_t *)p, p += up256((nl + 1) * 8);
      return p;
   }
};

// Prefix sums, totals and work items of the caller's counts; waits once for `s` -- the counts' two faults are arguments' faults,
// reported by the call that was handed them, and the grid of the resampling needs the items' number.
int prepare(sbgpu_ctx_t *c, const char *who, BootPrep &w, int64_t n_loci, const int64_t *d_row_off, const int32_t *d_count,
            const int64_t *host_locus_id, hipStream_t s)
{
#define SB_TRY(expr)                                                                     \
   do {                                                                                  \
      hipError_t e_ = (expr);                                                            \
      if (e_ != hipSuccess) {                                                            \
         (void)hipStreamSynchronize(s); /* (an upload from host arrays may be in flight) */ \
         return api_fail_hip(e_, #expr);                                                 \
      }                                                                                  \
   } while (0)
   char *pin = nullptr;
   SB_TRY(sb::ctx_pinned(c, 3, 16, &pin));
   SB_TRY(hipMemsetAsync(w.head, 0, 16, s));
   if (host_locus_id) SB_TRY(hipMemcpyAsync(w.locus_id, host_locus_id, (size_t)n_loci * 8, hipMemcpyHostToDevice, s));
   const int per_block = sb::kBootThreads / 64;
   hipLaunchKernelGGL(sb::boot_prefix_kernel, dim3((unsigned)((n_loci + per_block - 1) / per_block)), dim3(sb::kBootThreads), 0, s, n_loci, d_row_off, d_count,
                      w.incl, w.total, w.items, w.head);
   SB_TRY(hipGetLastError());
   hipLaunchKernelGGL(sb::boot_item_scan_kernel, dim3(1), dim3(1024), 0, s, n_loci, w.items, w.item_off, w.head);
   SB_TRY(hipGetLastError());
   SB_TRY(hipMemcpyAsync(pin, w.head, 16, hipMemcpyDeviceToHost, s));
   SB_TRY(hipStreamSynchronize(s));
   int64_t head[2];
   std::memcpy(head, pin, 16);
   if (head[0] & sb::kBootFaultNegative) return api_fail(SBGPU_EINVAL, std::string(who) + ": a negative count");
   if (head[0] & sb::kBootFaultDeep) return api_fail(SBGPU_ESHAPE, std::string(who) + ": a locus holds 2^40 fragments or more");
   w.n_items = head[1];
   return SBGPU_OK;
#undef SB_TRY
}

// Replicates rep_first .. rep_first + n_rep - 1 into d_out[n_rep][n_rows] (zeroed here), on `s`
int resample(const BootPrep &w, int64_t n_loci, int64_t n_rows, const int64_t *d_row_off, uint64_t seed, int32_t rep_first, int32_t n_rep,
             int32_t *d_out, hipStream_t s)
{
   if (n_rows == 0) return SBGPU_OK;
   hipError_t e = hipMemsetAsync(d_out, 0, (size_t)n_rep * (size_t)n_rows * 4, s);
   if (e != hipSuccess) return api_fail_hip(e, "hipMemsetAsync(replicate counts)");
   // a launch holds as many replicates as its grid can number
   const int64_t per_launch = std::max<int64_t>(1, (int64_t)0x7fffffff / w.n_items);
   if (w.n_items > 0x7fffffff) return api_fail(SBGPU_ESHAPE, "the bootstrap's work items of one replicate exceed a grid (2^31 slices of 16384 draws)");
   for (int64_t k = 0; k < n_rep; k += per_launch) {
      sb::BootResampleArgs a;
      a.n_loci = n_loci, a.n_items = w.n_items, a.total_rows = n_rows;
      a.row_off = d_row_off, a.locus_id = w.locus_id;
      a.incl = w.incl, a.total = w.total, a.item_off = w.item_off;
      a.seed = seed;
      a.rep_first = rep_first + (int32_t)k;
      a.n_rep = (int32_t)std::min<int64_t>(per_launch, n_rep - k);
      a.out = d_out + k * n_rows;
      hipLaunchKernelGGL(sb::boot_resample_kernel, dim3((unsigned)(w.n_items * a.n_rep)), dim3(sb::kBootThreads), 0, s, a);
      if ((e = hipGetLastError()) != hipSuccess) return api_fail_hip(e, "boot_resample_kernel");
   }
   return SBGPU_OK;
}

int check_params(const char *who, const sbgpu_bootstrap_params_t *p)
{
   if (!p) return api_fail(SBGPU_EINVAL, std::string(who) + ": null parameters");
   if (p->n_rep < 1) return api_fail(SBGPU_EINVAL, std::string(who) + ": n_rep must be at least 1");
   if (p->rep_first < 0 || (int64_t)p->rep_first + p->n_rep > sb::kBootMaxRep)
      return api_fail(SBGPU_EINVAL, std::string(who) + ": the replicate numbers must lie in [0, 2^24)");
   return SBGPU_OK;
}

} // namespace

extern "C" {

int sbgpu_bootstrap_counts_device(sbgpu_ctx_t *c, int64_t n_loci, const int64_t *row_off, const int32_t *d_count, const sbgpu_bootstrap_params_t *params,
                                  int32_t *d_count_out, void *stream)
{
   const char *who = "sbgpu_bootstrap_counts_device";
   if (const int rc = check_params(who, params); rc != SBGPU_OK) return rc;
   if (!c || n_loci < 0 || !row_off) return api_fail(SBGPU_EINVAL, std::string(who) + ": null context or offsets, or a negative locus count");
   for (int64_t l = 0; l < n_loci; ++l)
      if (row_off[l + 1] < row_off[l] || row_off[l + 1] - row_off[l] > INT32_MAX)
         return api_fail(SBGPU_EINVAL, std::string(who) + ": row_off must not decrease (locus " + std::to_string(l) + ")");
   if (n_loci == 0) return SBGPU_OK;
   if (row_off[0] != 0) return api_fail(SBGPU_EINVAL, std::string(who) + ": row_off[0] must be 0");
   const int64_t n_rows = row_off[n_loci];
   if (n_rows && (!d_count || !d_count_out)) return api_fail(SBGPU_EINVAL, std::string(who) + ": null count array");
   hipStream_t s = (hipStream_t)stream;
   hipError_t e = hipSetDevice(sb::ctx_device(c));
   if (e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   char *mem = nullptr;
   if ((e = sb::ctx_boot_scratch(c, BootPrep::bytes(n_loci, n_rows, params->locus_id != nullptr, true), &mem)) != hipSuccess)
      return api_fail_hip(e, "hipMalloc(bootstrap scratch)");
   BootPrep w;
   w.lay(mem, n_loci, n_rows, params->locus_id != nullptr, true);
   if ((e = hipMemcpyAsync(w.row_off, row_off, (size_t)(n_loci + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess) {
      (void)hipStreamSynchronize(s);
      return api_fail_hip(e, "hipMemcpyAsync(row_off)");
   }
   if (const int rc = prepare(c, who, w, n_loci, w.row_off, d_count, params->locus_id, s); rc != SBGPU_OK) return rc;
   if (const int rc = resample(w, n_loci, n_rows, w.row_off, params->seed, params->rep_first, params->n_rep, d_count_out, s); rc != SBGPU_OK) return rc;
   // the scratch is the context's: the next call on it may start at once
   if ((e = hipStreamSynchronize(s)) != hipSuccess) return api_fail_hip(e, "hipStreamSynchronize");
   return SBGPU_OK;
}

int sbgpu_em_bootstrap_device(sbgpu_ctx_t *c, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F, const sbgpu_bootstrap_params_t *params,
                              double *d_mean, double *d_var, int32_t *d_status_count, double *d_theta_rep, int32_t *d_status_rep, int32_t *d_iters_rep,
                              void *stream)
{
   const char *who = "sbgpu_em_bootstrap_device";
   if (const int rc = check_params(who, params); rc != SBGPU_OK) return rc;
   if (!c || !plan) return api_fail(SBGPU_EINVAL, std::string(who) + ": null ctx/plan");
   const sb::PlanShape ps = sb::plan_shape(plan);
   const int64_t nl = ps.n_loci, n_rows = ps.n_rows, n_iso = ps.n_iso;
   if (nl == 0) return SBGPU_OK;
   if (!d_mean || !d_var || !d_status_count || (!d_count && n_rows) || !d_F) return api_fail(SBGPU_EINVAL, std::string(who) + ": null device pointer");
   const int32_t B = params->n_rep;
   hipStream_t s = (hipStream_t)stream, js = nullptr;
   hipEvent_t ev[3];
#define SB_TRY(expr)                                    \
   do {                                                 \
      hipError_t e_ = (expr);                           \
      if (e_ != hipSuccess) {                           \
         (void)hipStreamSynchronize(s);                 \
         return api_fail_hip(e_, #expr);                \
      }                                                 \
   } while (0)
   SB_TRY(hipSetDevice(sb::ctx_device(c)));
   // the statistics run on a stream of the context's own, replicate after replicate, behind each replicate's EM
   SB_TRY(sb::ctx_copy_stream(c, &js));
   for (int i = 0; i < 3; ++i) SB_TRY(sb::ctx_event(c, i, &ev[i]));
   // two sets of a replicate's counts and results: replicate k + 1 is resampled and solved while replicate k's statistics run
   const size_t set_bytes = up256((size_t)n_rows * 4) + up256((size_t)n_iso * 8) + 2 * up256((size_t)nl * 4);
   const bool ids = params->locus_id != nullptr;
   char *mem = nullptr;
   // (the scratch is the context's: an earlier call on another stream may still work in it)
   SB_TRY(hipStreamWaitEvent(s, ev[2], 0));
   SB_TRY(sb::ctx_boot_scratch(c, BootPrep::bytes(nl, n_rows, ids, false) + 2 * set_bytes, &mem));
   BootPrep w;
   char *p = w.lay(mem, nl, n_rows, ids, false);
   int32_t *cnt[2], *status[2], *iters[2];
   double *theta[2];
   for (int b = 0; b < 2; ++b) {
      cnt[b] = (int32_t *)p, p += up256((size_t)n_rows * 4);
      theta[b] = (double *)p, p += up256((size_t)n_iso * 8);
      status[b] = (int32_t *)p, p += up256((size_t)nl * 4);
      iters[b] = (int32_t *)p, p += up256((size_t)nl * 4);
   }
   if (const int rc = prepare(c, who, w, nl, ps.d_row_off, d_count, params->locus_id, s); rc != SBGPU_OK) return rc;
   SB_TRY(hipMemsetAsync(d_status_count, 0, (size_t)nl * 4 * sizeof(int32_t), s));
   const int64_t n_threads = std::max(n_iso, nl);
   for (int32_t k = 0; k < B; ++k) {
      const int b = k & 1;
      if (k >= 2) SB_TRY(hipStreamWaitEvent(s, ev[b], 0)); // the statistics of replicate k - 2 have read this set
      if (const int rc = resample(w, nl, n_rows, ps.d_row_off, params->seed, params->rep_first + k, 1, cnt[b], s); rc != SBGPU_OK) {
         (void)hipStreamSynchronize(s);
         return rc;
      }
      // the kernels start behind the resampling on `s` and join `js`; `s` is free for the next replicate at once
      if (const int rc = sbgpu_em_run_device_split(c, plan, cnt[b], d_F, theta[b], status[b], iters[b], s, js); rc != SBGPU_OK) {
         (void)hipStreamSynchronize(s);
         return rc;
      }
      sb::BootStatsArgs a;
      a.n_iso = n_iso, a.n_loci = nl, a.step = k, a.n_rep = B;
      a.theta = theta[b], a.status = status[b], a.iters = iters[b];
      a.mean = d_mean, a.var = d_var, a.status_count = d_status_count;
      a.theta_rep = d_theta_rep ? d_theta_rep + (size_t)k * (size_t)n_iso : nullptr;
      a.status_rep = d_status_rep ? d_status_rep + (size_t)k * (size_t)nl : nullptr;
      a.iters_rep = d_iters_rep ? d_iters_rep + (size_t)k * (size_t)nl : nullptr;
      hipLaunchKernelGGL(sb::boot_stats_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, js, a);
      SB_TRY(hipGetLastError());
      SB_TRY(hipEventRecord(ev[b], js));
   }
   // the caller's stream continues behind the last replicate's statistics
   SB_TRY(hipEventRecord(ev[2], js));
   SB_TRY(hipStreamWaitEvent(s, ev[2], 0));
   return SBGPU_OK;
#undef SB_TRY
}

} // extern "C"
