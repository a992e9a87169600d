// strawberry_amd/csrc/bootstrap_api.hip -- sbgpu_bootstrap_counts_device / sbgpu_em_bootstrap_device, and the bootstrap of the
// resident path: sbgpu_bootstrap_keep / sbgpu_abundance_bootstrap_device / sbgpu_replicate_stats_device, and per locus
// sbgpu_locus_abundance_device / sbgpu_locus_bootstrap_device (include/sbgpu.h): the EM bootstrap on the device
// (bootstrap_device.h).  Replicates' counts by the rule of bootstrap_rules.h, the
// existing EM entry replicate after replicate, Welford's recurrence over the replicates' theta.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>

#include "../../include/sbgpu.h"
#include "bootstrap_device.h"
#include "stage_common.h"

using sb::api_fail;
using sb::api_fail_hip;

namespace {

using sb::up256;

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

// What follows the statistics step of a replicate on the join stream: replicate k's theta and status are in the set it is handed;
// the set is free again once what the hook queues on `js` is through.
using AfterStats = std::function<int(int32_t k, const double *d_theta, const int32_t *d_status, hipStream_t js)>;

// The replicates of a call, shared by sbgpu_em_bootstrap_device and sbgpu_abundance_bootstrap_device: prefix sums once (the
// call's one wait), then per replicate a resample, the EM through the split entry, and on the join stream one step of the
// statistics and `after` (may be empty).  Two sets of counts and results in the context's bootstrap scratch, allocated before
// the first kernel.  On return `s` continues behind the last replicate's join-stream work.
int run_replicates(sbgpu_ctx_t *c, const char *who, const sbgpu_plan_t *plan, const int32_t *d_count, const double *d_F,
                   const sbgpu_bootstrap_params_t *params, double *d_mean, double *d_var, int32_t *d_status_count, double *d_theta_rep,
                   int32_t *d_status_rep, int32_t *d_iters_rep, hipStream_t s, const AfterStats &after)
{
   const sb::PlanShape ps = sb::plan_shape(plan);
   const int64_t nl = ps.n_loci, n_rows = ps.n_rows, n_iso = ps.n_iso;
   const int32_t B = params->n_rep;
   hipStream_t js = nullptr;
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
      if (after) {
         if (const int rc = after(k, theta[b], status[b], js); rc != SBGPU_OK) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamSynchronize(js);
            return rc;
         }
      }
      SB_TRY(hipEventRecord(ev[b], js));
   }
   // the caller's stream continues behind the last replicate's statistics
   SB_TRY(hipEventRecord(ev[2], js));
   SB_TRY(hipStreamWaitEvent(s, ev[2], 0));
   return SBGPU_OK;
#undef SB_TRY
}

// boot_interval_kernel over the columns of x[n_rep][n] on `s` (the arguments are checked by the callers)
int launch_interval(const sb::BootIntervalArgs &a, hipStream_t s)
{
   if (a.n == 0) return SBGPU_OK;
   const unsigned grid = (unsigned)((a.n + sb::kBootTile - 1) / sb::kBootTile);
   const size_t lds = (size_t)sb::kBootTile * (size_t)a.n_rep * sizeof(double);
   const dim3 block(sb::kBootIntervalThreads);
   if (a.n_rep <= 64) hipLaunchKernelGGL(sb::boot_interval_kernel<1>, dim3(grid), block, lds, s, a);
   else if (a.n_rep <= 128) hipLaunchKernelGGL(sb::boot_interval_kernel<2>, dim3(grid), block, lds, s, a);
   else if (a.n_rep <= 256) hipLaunchKernelGGL(sb::boot_interval_kernel<4>, dim3(grid), block, lds, s, a);
   else if (a.n_rep <= 512) hipLaunchKernelGGL(sb::boot_interval_kernel<8>, dim3(grid), block, lds, s, a);
   else hipLaunchKernelGGL(sb::boot_interval_kernel<16>, dim3(grid), block, lds, s, a);
   if (hipError_t e = hipGetLastError(); e != hipSuccess) return api_fail_hip(e, "boot_interval_kernel");
   return SBGPU_OK;
}

int check_ranks(const char *who, int32_t n_rep, int32_t rank_lo, int32_t rank_hi)
{
   if (rank_lo < 0 || rank_lo > rank_hi || rank_hi >= n_rep)
      return api_fail(SBGPU_EINVAL, std::string(who) + ": the ranks must satisfy 0 <= rank_lo <= rank_hi < n_rep");
   if (n_rep > sb::kBootMaxStatRep)
      return api_fail(SBGPU_ESHAPE, std::string(who) + ": more than " + std::to_string(sb::kBootMaxStatRep) + " replicates (the order statistics sort a column in one wave's registers)");
   return SBGPU_OK;
}

// sbgpu_abundance_bootstrap_device (`loc` null) and sbgpu_locus_bootstrap_device (`loc` set): one body, so that what `out` gets
// cannot differ between the two.  With `loc` the result block grows behind its old end -- every old array keeps its place --, the
// epilogue writes Frac into row k of frac_rep instead of the one-row scratch, boot_locus_sum_kernel follows it on the join
// stream, and three more statistics passes run behind the old two.
int abundance_bootstrap(const char *who, sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_bootstrap_params_t *params, int32_t rank_lo, int32_t rank_hi,
                        int32_t keep_theta_rep, sbgpu_comm_t *comm, void *stream, sbgpu_abundance_bootstrap_t *out, sbgpu_locus_bootstrap_t *loc)
{
   if (const int rc = check_params(who, params); rc != SBGPU_OK) return rc;
   if (!c || !bins || !out) return api_fail(SBGPU_EINVAL, std::string(who) + ": null argument");
   if (const int rc = check_ranks(who, params->n_rep, rank_lo, rank_hi); rc != SBGPU_OK) return rc;
   const sb::BootKeep *rec = sb::ctx_boot_keep(c);
   const sb::BinsContextView v = sb::bins_context_view(bins);
   sb::PlanShape ps;
   if (const int rc = sb::check_boot_keep(who, rec, v, false, &ps); rc != SBGPU_OK) return rc;
   const int64_t nl = ps.n_loci, n_iso = ps.n_iso;
   const int32_t B = params->n_rep;
   hipStream_t s = stream ? (hipStream_t)stream : sb::ctx_stream(c);
   if (hipError_t e = hipSetDevice(sb::ctx_device(c)); e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   // ---- the results' block, before any kernel: [ten statistics | frac of one replicate | totals | keep and status counts | the replicates' matrices]
   const size_t ni = (size_t)std::max<int64_t>(n_iso, 1), col = up256(ni * 8);
   size_t off = 0;
   auto take = [&off](size_t bytes) {
      const size_t at = off;
      off += up256(bytes);
      return at;
   };
   size_t o_stat[10];
   for (size_t &o : o_stat) o = take(col);
   const size_t o_frac = take(col), o_total = take((size_t)B * 8), o_keep_count = take(ni * 4), o_status_count = take((size_t)nl * 16);
   const size_t o_fpkm_rep = take((size_t)B * ni * 8), o_keep_rep = take((size_t)B * ni * 4);
   const size_t o_theta_rep = keep_theta_rep ? take((size_t)B * ni * 8) : 0;
   // (the locus call's additions: four Frac statistics, eight locus statistics, the kept replicates' count, the three matrices)
   const size_t nlc = (size_t)std::max<int64_t>(nl, 1), lcol = up256(nlc * 8);
   size_t o_fstat[4] = {0, 0, 0, 0}, o_lstat[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o_lkept_count = 0, o_frac_rep = 0, o_lfpkm_rep = 0, o_lkept_rep = 0;
   if (loc) {
      for (size_t &o : o_fstat) o = take(col);
      for (size_t &o : o_lstat) o = take(lcol);
      o_lkept_count = take(nlc * 4);
      o_frac_rep = take((size_t)B * ni * 8), o_lfpkm_rep = take((size_t)B * nlc * 8), o_lkept_rep = take((size_t)B * nlc * 4);
   }
   char *d = nullptr;
   if (hipError_t e = sb::ctx_boot_result(c, off, &d); e != hipSuccess) return api_fail_hip(e, "hipMalloc(the replicates' FPKM and keep matrices)");
   double *stat[10];
   for (int i = 0; i < 10; ++i) stat[i] = (double *)(d + o_stat[i]);
   double *d_theta_mean = stat[0], *d_theta_var = stat[1], *d_fpkm_mean = stat[2], *d_fpkm_var = stat[3], *d_fpkm_lo = stat[4], *d_fpkm_hi = stat[5];
   double *d_tpm_mean = stat[6], *d_tpm_var = stat[7], *d_tpm_lo = stat[8], *d_tpm_hi = stat[9];
   double *d_frac = (double *)(d + o_frac), *d_total = (double *)(d + o_total), *d_fpkm_rep = (double *)(d + o_fpkm_rep);
   int32_t *d_keep_count = (int32_t *)(d + o_keep_count), *d_status_count = (int32_t *)(d + o_status_count), *d_keep_rep = (int32_t *)(d + o_keep_rep);
   double *d_theta_rep = keep_theta_rep ? (double *)(d + o_theta_rep) : nullptr;
   double *fstat[4] = {nullptr, nullptr, nullptr, nullptr}, *lstat[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
   double *d_frac_rep = nullptr, *d_lfpkm_rep = nullptr;
   int32_t *d_lkept_count = nullptr, *d_lkept_rep = nullptr;
   if (loc) {
      for (int i = 0; i < 4; ++i) fstat[i] = (double *)(d + o_fstat[i]);
      for (int i = 0; i < 8; ++i) lstat[i] = (double *)(d + o_lstat[i]);
      d_lkept_count = (int32_t *)(d + o_lkept_count), d_lkept_rep = (int32_t *)(d + o_lkept_rep);
      d_frac_rep = (double *)(d + o_frac_rep), d_lfpkm_rep = (double *)(d + o_lfpkm_rep);
   }
#define SB_TRY(expr)                                    \
   do {                                                 \
      hipError_t e_ = (expr);                           \
      if (e_ != hipSuccess) {                           \
         (void)hipStreamSynchronize(s);                 \
         return api_fail_hip(e_, #expr);                \
      }                                                 \
   } while (0)
   // ---- the replicates: behind each one's statistics step, the reference's epilogue on its theta and status -- FPKM and keep into
   // row k of the matrices, this rank's kept-FPKM sum into d_total[k].  The mapped-read total and the insert law are the sample's.
   const sbgpu_abundance_params_t par = rec->params;
   const sbgpu_plan_t *plan = rec->plan;
   const int32_t *d_len = rec->d_iso_len;
   const AfterStats epilogue = [&](int32_t k, const double *d_theta, const int32_t *d_status, hipStream_t js) {
      double *row_fpkm = d_fpkm_rep + (size_t)k * (size_t)n_iso;
      int32_t *row_keep = d_keep_rep + (size_t)k * (size_t)n_iso;
      if (const int rc = sbgpu_abundance_device(c, plan, d_theta, d_status, d_len, &par, row_fpkm, loc ? d_frac_rep + (size_t)k * (size_t)n_iso : d_frac,
                                                row_keep, d_total + k, js);
          rc != SBGPU_OK || !loc)
         return rc;
      // the loci's sums of this replicate's row, behind its epilogue
      sb::BootLocusSumArgs la{};
      la.n_loci = nl, la.n_iso = n_iso, la.n_rows = 1, la.iso_off = ps.d_iso_off, la.fpkm = row_fpkm, la.keep = row_keep;
      la.locus_fpkm = d_lfpkm_rep + (size_t)k * (size_t)nl, la.locus_kept = d_lkept_rep + (size_t)k * (size_t)nl;
      hipLaunchKernelGGL(sb::boot_locus_sum_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, js, la);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return api_fail_hip(e, "boot_locus_sum_kernel");
      return (int)SBGPU_OK;
   };
   if (const int rc = run_replicates(c, who, plan, rec->d_count, rec->d_F, params, d_theta_mean, d_theta_var, d_status_count, d_theta_rep, nullptr, nullptr, s,
                                     epilogue);
       rc != SBGPU_OK)
      return rc;
   // ---- the total TPM divides by: ONE collective per call, over all replicates
   if (comm) {
      if (const int rc = sbgpu_allreduce_sum_f64(comm, d_total, B, s); rc != SBGPU_OK) {
         (void)hipStreamSynchronize(s);
         return rc;
      }
   }
   // ---- the replicates' statistics, twice over the columns: the raw FPKM; the TPM (made while staging) with the kept replicates' count
   SB_TRY(hipMemsetAsync(d_keep_count, 0, ni * 4, s));
   sb::BootIntervalArgs a{};
   a.n = n_iso, a.n_rep = B, a.rank_lo = rank_lo, a.rank_hi = rank_hi, a.x = d_fpkm_rep;
   a.mean = d_fpkm_mean, a.var = d_fpkm_var, a.lo = d_fpkm_lo, a.hi = d_fpkm_hi;
   if (const int rc = launch_interval(a, s); rc != SBGPU_OK) {
      (void)hipStreamSynchronize(s);
      return rc;
   }
   a.keep = d_keep_rep, a.total = d_total, a.keep_count = d_keep_count;
   a.mean = d_tpm_mean, a.var = d_tpm_var, a.lo = d_tpm_lo, a.hi = d_tpm_hi;
   if (const int rc = launch_interval(a, s); rc != SBGPU_OK) {
      (void)hipStreamSynchronize(s);
      return rc;
   }
   // ---- the locus call's three passes: Frac as it stands; the loci's FPKM; the loci's TPM (made while staging, the loci's kept
   // counts as the flag) with the count of the replicates that kept an isoform of the locus
   if (loc) {
      SB_TRY(hipMemsetAsync(d_lkept_count, 0, nlc * 4, s));
      sb::BootIntervalArgs f{};
      f.n = n_iso, f.n_rep = B, f.rank_lo = rank_lo, f.rank_hi = rank_hi, f.x = d_frac_rep;
      f.mean = fstat[0], f.var = fstat[1], f.lo = fstat[2], f.hi = fstat[3];
      int rc = launch_interval(f, s);
      f.n = nl, f.x = d_lfpkm_rep;
      f.mean = lstat[0], f.var = lstat[1], f.lo = lstat[2], f.hi = lstat[3];
      if (rc == SBGPU_OK) rc = launch_interval(f, s);
      f.keep = d_lkept_rep, f.total = d_total, f.keep_count = d_lkept_count;
      f.mean = lstat[4], f.var = lstat[5], f.lo = lstat[6], f.hi = lstat[7];
      if (rc == SBGPU_OK) rc = launch_interval(f, s);
      if (rc != SBGPU_OK) {
         (void)hipStreamSynchronize(s);
         return rc;
      }
   }
   // ---- what was asked for comes down; the call returns synchronised
   auto get = [&](void *dst, const void *src, size_t bytes) { return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess; };
   double *const host_stat[10] = {out->theta_mean, out->theta_var, out->fpkm_mean, out->fpkm_var, out->fpkm_lo, out->fpkm_hi, out->tpm_mean, out->tpm_var, out->tpm_lo, out->tpm_hi};
   for (int i = 0; i < 10; ++i) SB_TRY(get(host_stat[i], stat[i], (size_t)n_iso * 8));
   SB_TRY(get(out->keep_count, d_keep_count, (size_t)n_iso * 4));
   SB_TRY(get(out->status_count, d_status_count, (size_t)nl * 16));
   SB_TRY(get(out->total_fpkm_rep, d_total, (size_t)B * 8));
   SB_TRY(get(out->fpkm_rep, d_fpkm_rep, (size_t)B * (size_t)n_iso * 8));
   SB_TRY(get(out->keep_rep, d_keep_rep, (size_t)B * (size_t)n_iso * 4));
   if (d_theta_rep) SB_TRY(get(out->theta_rep, d_theta_rep, (size_t)B * (size_t)n_iso * 8));
   if (loc) {
      double *const host_f[4] = {loc->frac_mean, loc->frac_var, loc->frac_lo, loc->frac_hi};
      double *const host_l[8] = {loc->locus_fpkm_mean, loc->locus_fpkm_var, loc->locus_fpkm_lo, loc->locus_fpkm_hi,
                                 loc->locus_tpm_mean, loc->locus_tpm_var, loc->locus_tpm_lo, loc->locus_tpm_hi};
      for (int i = 0; i < 4; ++i) SB_TRY(get(host_f[i], fstat[i], (size_t)n_iso * 8));
      for (int i = 0; i < 8; ++i) SB_TRY(get(host_l[i], lstat[i], (size_t)nl * 8));
      SB_TRY(get(loc->locus_kept_count, d_lkept_count, (size_t)nl * 4));
      SB_TRY(get(loc->frac_rep, d_frac_rep, (size_t)B * (size_t)n_iso * 8));
      SB_TRY(get(loc->locus_fpkm_rep, d_lfpkm_rep, (size_t)B * (size_t)nl * 8));
      SB_TRY(get(loc->locus_kept_rep, d_lkept_rep, (size_t)B * (size_t)nl * 4));
   }
   SB_TRY(hipStreamSynchronize(s));
#undef SB_TRY
   if (sb::ctx_take_wide_error(c)) return api_fail(SBGPU_EHIP, std::string(who) + ": a barrier of the wide-locus EM kernel timed out: the loci it served have no result");
   out->n_rep = B, out->n_iso = n_iso, out->n_loci = nl;
   out->d_theta_mean = d_theta_mean, out->d_theta_var = d_theta_var;
   out->d_fpkm_mean = d_fpkm_mean, out->d_fpkm_var = d_fpkm_var, out->d_fpkm_lo = d_fpkm_lo, out->d_fpkm_hi = d_fpkm_hi;
   out->d_tpm_mean = d_tpm_mean, out->d_tpm_var = d_tpm_var, out->d_tpm_lo = d_tpm_lo, out->d_tpm_hi = d_tpm_hi;
   out->d_keep_count = d_keep_count, out->d_status_count = d_status_count, out->d_total_fpkm_rep = d_total;
   out->d_fpkm_rep = d_fpkm_rep, out->d_keep_rep = d_keep_rep, out->d_theta_rep = d_theta_rep;
   if (loc) {
      loc->n_rep = B, loc->n_iso = n_iso, loc->n_loci = nl, loc->reserved = 0;
      loc->d_frac_mean = fstat[0], loc->d_frac_var = fstat[1], loc->d_frac_lo = fstat[2], loc->d_frac_hi = fstat[3];
      loc->d_locus_fpkm_mean = lstat[0], loc->d_locus_fpkm_var = lstat[1], loc->d_locus_fpkm_lo = lstat[2], loc->d_locus_fpkm_hi = lstat[3];
      loc->d_locus_tpm_mean = lstat[4], loc->d_locus_tpm_var = lstat[5], loc->d_locus_tpm_lo = lstat[6], loc->d_locus_tpm_hi = lstat[7];
      loc->d_locus_kept_count = d_lkept_count, loc->d_frac_rep = d_frac_rep, loc->d_locus_fpkm_rep = d_lfpkm_rep, loc->d_locus_kept_rep = d_lkept_rep;
   }
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
   if (ps.n_loci == 0) return SBGPU_OK;
   if (!d_mean || !d_var || !d_status_count || (!d_count && ps.n_rows) || !d_F) return api_fail(SBGPU_EINVAL, std::string(who) + ": null device pointer");
   return run_replicates(c, who, plan, d_count, d_F, params, d_mean, d_var, d_status_count, d_theta_rep, d_status_rep, d_iters_rep, (hipStream_t)stream, AfterStats());
}

int sbgpu_replicate_stats_device(sbgpu_ctx_t *c, int32_t n_rep, int64_t n, const double *d_x, int32_t rank_lo, int32_t rank_hi, double *d_mean,
                                 double *d_var, double *d_lo, double *d_hi, void *stream)
{
   const char *who = "sbgpu_replicate_stats_device";
   if (!c) return api_fail(SBGPU_EINVAL, std::string(who) + ": null context");
   if (n_rep < 1 || n < 0) return api_fail(SBGPU_EINVAL, std::string(who) + ": n_rep must be at least 1 and n at least 0");
   if (const int rc = check_ranks(who, n_rep, rank_lo, rank_hi); rc != SBGPU_OK) return rc;
   if (n && !d_x) return api_fail(SBGPU_EINVAL, std::string(who) + ": null matrix");
   if (hipError_t e = hipSetDevice(sb::ctx_device(c)); e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   sb::BootIntervalArgs a{};
   a.n = n, a.n_rep = n_rep, a.rank_lo = rank_lo, a.rank_hi = rank_hi;
   a.x = d_x, a.mean = d_mean, a.var = d_var, a.lo = d_lo, a.hi = d_hi;
   return launch_interval(a, (hipStream_t)stream);
}

int sbgpu_bootstrap_keep(sbgpu_ctx_t *c, int32_t on)
{
   if (!c) return api_fail(SBGPU_EINVAL, "sbgpu_bootstrap_keep: null context");
   sb::ctx_boot_keep(c)->on = on != 0; // (what the last call kept stays valid until the context's next sbgpu_quantify_* call either way)
   return SBGPU_OK;
}

int sbgpu_abundance_bootstrap_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_bootstrap_params_t *params, int32_t rank_lo, int32_t rank_hi,
                                     int32_t keep_theta_rep, sbgpu_comm_t *comm, void *stream, sbgpu_abundance_bootstrap_t *out)
{
   return abundance_bootstrap("sbgpu_abundance_bootstrap_device", c, bins, params, rank_lo, rank_hi, keep_theta_rep, comm, stream, out, nullptr);
}

int sbgpu_locus_bootstrap_device(sbgpu_ctx_t *c, const sbgpu_bins_t *bins, const sbgpu_bootstrap_params_t *params, int32_t rank_lo, int32_t rank_hi,
                                 int32_t keep_theta_rep, sbgpu_comm_t *comm, void *stream, sbgpu_abundance_bootstrap_t *out, sbgpu_locus_bootstrap_t *locus_out)
{
   const char *who = "sbgpu_locus_bootstrap_device";
   if (!locus_out) return api_fail(SBGPU_EINVAL, std::string(who) + ": null locus_out");
   sbgpu_abundance_bootstrap_t none{}; // (`out` may be NULL: nothing of it comes down then)
   return abundance_bootstrap(who, c, bins, params, rank_lo, rank_hi, keep_theta_rep, comm, stream, out ? out : &none, locus_out);
}

int sbgpu_locus_abundance_device(sbgpu_ctx_t *c, int64_t n_loci, const int64_t *d_iso_off, const double *d_fpkm, const int32_t *d_keep,
                                 const double *d_total_fpkm, double *d_locus_fpkm, double *d_locus_tpm, int32_t *d_locus_kept, void *stream)
{
   const char *who = "sbgpu_locus_abundance_device";
   if (!c || n_loci < 0 || !d_iso_off) return api_fail(SBGPU_EINVAL, std::string(who) + ": null context or iso_off, or a negative locus count");
   if (n_loci == 0) return SBGPU_OK;
   if (n_loci > INT32_MAX) return api_fail(SBGPU_ESHAPE, std::string(who) + ": more than 2^31 - 1 loci");
   if (!d_fpkm || !d_keep) return api_fail(SBGPU_EINVAL, std::string(who) + ": null fpkm or keep array");
   if (d_locus_tpm && !d_total_fpkm) return api_fail(SBGPU_EINVAL, std::string(who) + ": the loci's TPM need the total FPKM");
   if (hipError_t e = hipSetDevice(sb::ctx_device(c)); e != hipSuccess) return api_fail_hip(e, "hipSetDevice");
   sb::BootLocusSumArgs a{};
   a.n_loci = n_loci, a.n_iso = 0, a.n_rows = 1, a.iso_off = d_iso_off, a.fpkm = d_fpkm, a.keep = d_keep, a.total = d_total_fpkm;
   a.locus_fpkm = d_locus_fpkm, a.locus_tpm = d_locus_tpm, a.locus_kept = d_locus_kept;
   hipLaunchKernelGGL(sb::boot_locus_sum_kernel, dim3((unsigned)((n_loci + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
   if (hipError_t e = hipGetLastError(); e != hipSuccess) return api_fail_hip(e, "boot_locus_sum_kernel");
   return SBGPU_OK;
}

} // extern "C"
