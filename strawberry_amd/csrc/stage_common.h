// strawberry_amd/csrc/stage_common.h -- what the launchers of the retained-result stages share (context_api.hip,
// assign_api.hip, coverage_api.hip, fit_api.hip; the record checks serve bootstrap_api.hip too): the checks of a
// handle against the context's record, the synchronise-then-fail macro, the upload block and the result copies.  The limits,
// the work items and the arenas' layouts are stage_host.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "stage_host.h"

namespace sb {

// A HIP call of a launcher whose stream is `s`: on failure the stream is synchronised first (the upload from the host block
// may still be in flight), then the call fails.
#define SB_STAGE_TRY(expr)                                                                  \
   do {                                                                                     \
      hipError_t e_ = (expr);                                                               \
      if (e_ != hipSuccess) {                                                               \
         (void)hipStreamSynchronize(s);                                                     \
         return sb::api_fail(SBGPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
      }                                                                                     \
   } while (0)

// The handle against the ContextKeep record, for entry point `who`.  hit_stages: the checks of the stages that walk every hit
// (the assignment, the coverage): the hits' offsets span the record's hits, and the hits' bins and the weights are on the device.
static inline int check_context_keep(const std::string &who, const ContextKeep *k, const BinsContextView &v, bool hit_stages)
{
   if (!v.context_serial)
      return api_fail(SBGPU_EINVAL, who + ": this handle was made without retention (sbgpu_context_table_keep was off for its call, "
                                          "or it is not from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.context_serial != k->serial)
      return api_fail(SBGPU_EINVAL, who + ": a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that "
                                          "works in the context's scratch, such as sbgpu_bins_create_device) has reused what its call kept");
   const int64_t nl = v.n_loci, nh = k->n_hits;
   if (nl != k->n_loci || v.n_iso != k->n_iso || (int64_t)k->locus_hit_off.size() != nl + 1 ||
       (hit_stages && (k->locus_hit_off[0] != 0 || k->locus_hit_off[(size_t)nl] != nh)))
      return api_fail(SBGPU_EINVAL, who + ": the handle and the context's record disagree");
   if (!hit_stages) return SBGPU_OK;
   if (nh && (!k->d_hit_bin_local || !k->d_compat || k->compat_words < 1)) return api_fail(SBGPU_EINVAL, who + ": the hits' bins are not on the device");
   if (v.n_elem && !k->d_F) return api_fail(SBGPU_EINVAL, who + ": the weights are not on the device");
   return SBGPU_OK;
}

// Every locus within the kernels' LDS limits (`bins_text`: the entry's own words for a locus of too many bins); hit_off given:
// and the hits' offsets ascend.
static inline int check_locus_limits(const std::string &who, const BinsContextView &v, const char *bins_text, const std::vector<int64_t> *hit_off)
{
   for (int64_t l = 0; l < v.n_loci; ++l) {
      if (v.row_off[l + 1] - v.row_off[l] > kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + bins_text);
      if (v.iso_off[l + 1] - v.iso_off[l] > 32 * (int64_t)kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
      if (hit_off && (*hit_off)[(size_t)l + 1] < (*hit_off)[(size_t)l]) return api_fail(SBGPU_EINVAL, who + ": the handle and the context's record disagree");
   }
   return SBGPU_OK;
}

// The handle against the BootKeep record, for entry point `who`; *ps: the record's plan.  rows_too: the plan's bins are the
// handle's as well (the model fit walks them).
static inline int check_boot_keep(const std::string &who, const BootKeep *rec, const BinsContextView &v, bool rows_too, PlanShape *ps)
{
   if (!v.boot_serial)
      return api_fail(SBGPU_EINVAL, who + ": this handle was made without retention (sbgpu_bootstrap_keep was off for its call, or it is not "
                                          "from sbgpu_quantify_resident / sbgpu_front_stream_end)");
   if (v.boot_serial != rec->serial || !rec->plan)
      return api_fail(SBGPU_EINVAL, who + ": a stale handle: a later call on this context (sbgpu_quantify_*, or another entry that works in the "
                                          "context's scratch) has reused what its call kept");
   *ps = plan_shape(rec->plan);
   if (ps->n_loci != v.n_loci || ps->n_iso != v.n_iso || (rows_too && ps->n_rows != v.n_bins) || ps->n_loci != rec->n_loci || ps->n_iso != rec->n_iso)
      return api_fail(SBGPU_EINVAL, who + ": the handle and the context's record disagree");
   return SBGPU_OK;
}

// One host block for a call's uploads (zeroed): it lives until the call's last synchronisation, and SB_STAGE_TRY synchronises
// before it leaves early.
struct HostBlock {
   std::vector<char> bytes;
   explicit HostBlock(size_t n) : bytes(n, 0) {}
   template <class T>
   void put(size_t at, const T *src, size_t n)
   {
      if (n) std::memcpy(bytes.data() + at, src, n * sizeof(T));
   }
   hipError_t upload(char *d, hipStream_t s) const { return hipMemcpyAsync(d, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s); }
};

// Array `at` of the arena, typed
template <class T>
static inline T *arena_at(char *d, size_t at)
{
   return (T *)(d + at);
}
// A result the caller asked for (host non-null): its n entries from the arena into the caller's array, on `s`
template <class T>
static inline hipError_t copy_back(T *host, const char *d, size_t at, int64_t n, hipStream_t s)
{
   return host && n ? hipMemcpyAsync(host, d + at, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess;
}

// fit_api.hip: the model fit's launches for a stage that runs them in memory of its own (loo_api.hip), as
// asg_launch_column_pass serves the stages behind the assignment.  fit_plan: the loci by form and the arena's layout
// (SBGPU_ESHAPE for a locus beyond the fit's limits); fit_launch: the lists' upload through `host` (p.L.upload_bytes, alive until
// the caller has synchronised `s`), the column pass and the two forms, in arena `d` (p.L.bytes), results at p.L's offsets.
struct FitPlan {
   std::vector<int32_t> small, large;
   bool any_weight = false;
   FitLayout L;
};
int fit_plan(const std::string &who, const PlanShape &ps, bool own_keep, bool own_status, FitPlan *out);
int fit_launch(sbgpu_ctx_t *c, const PlanShape &ps, const FitPlan &p, HostBlock &host, char *d, const int32_t *d_count, const double *d_F,
               const double *d_theta, const int32_t *d_keep, const int32_t *d_status, hipStream_t s);

// The grid of a kernel that strides over n units of work: min(n, cap), at least one workgroup
static inline unsigned stage_grid(int64_t n, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, cap)); }

} // namespace sb
