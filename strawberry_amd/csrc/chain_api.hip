// strawberry_amd/csrc/chain_api.hip -- the one-call entry points of include/sbgpu.h: sbgpu_quantify_host (host arrays in),
// sbgpu_quantify_device (hits resident in HBM) and sbgpu_quantify_resident (the same with pass 1 in front and the abundance
// epilogue and the path's collectives behind: README's "ONE resident call"), and sbgpu_annotation_pin / _unpin.  All three
// entries are one chain (QuantifyCall below) on the context's stream with the intermediate results resident in HBM.
// No torch, no Python: this is what a C / C++ driver calls (include/sbgpu_host.hpp wraps it).
#include <hip/hip_runtime.h>

#include <climits>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/sbgpu.h"
#include "api_internal.h"
#include "fraglen_device.h"
#include "stage_host.h"

using sb::api_fail;
using sb::api_fail_hip;

// a HIP call that must succeed (SBGPU_EHIP, "<the call>: <HIP's text>") / a library call whose code is passed on
#define SB_TRY(expr)                                                                                          \
   do {                                                                                                       \
      hipError_t e_ = (expr);                                                                                 \
      if (e_ != hipSuccess) return api_fail(SBGPU_EHIP, sb::hip_error_text(#expr, e_));                       \
   } while (0)
#define SB_RC(expr)                      \
   do {                                  \
      const int rc_ = (expr);            \
      if (rc_ != SBGPU_OK) return rc_;   \
   } while (0)

namespace {

// ---- layouts: where the parts of an arena lie (sb::Arena: every part begins at a multiple of 256 bytes)

struct Slab {
   const void *src = nullptr; // host array it is filled from
   size_t bytes = 0, off = 0; // bytes == 0: nothing to copy (it still has a place)
};
struct AnnotationCounts {
   int64_t nl, n_iso, n_exon, n_seg;
   explicit AnnotationCounts(const sbgpu_annotation_t *an)
      : nl(an->n_loci), n_iso(an->iso_off[nl]), n_exon(an->exon_off[n_iso]), n_seg(an->seg_off[nl])
   {
   }
};
// the annotation's arrays in a device arena: sbgpu_annotation_pin's and the per-call upload's
struct AnnotationLayout {
   Slab iso_off, exon_off, seg_off, exon_left, exon_right, seg_left, seg_right;
   // resident: the arrays are in HBM already (a pinned annotation given again): nothing is copied
   AnnotationLayout(const sbgpu_annotation_t *an, const AnnotationCounts &n, bool resident)
   {
      const size_t on = resident ? 0 : 1;
      iso_off = {an->iso_off, on * (size_t)(n.nl + 1) * 8, 0}, exon_off = {an->exon_off, on * (size_t)(n.n_iso + 1) * 8, 0};
      seg_off = {an->seg_off, on * (size_t)(n.nl + 1) * 8, 0};
      exon_left = {an->exon_left, on * (size_t)n.n_exon * 4, 0}, exon_right = {an->exon_right, on * (size_t)n.n_exon * 4, 0};
      seg_left = {an->seg_left, on * (size_t)n.n_seg * 4, 0}, seg_right = {an->seg_right, on * (size_t)n.n_seg * 4, 0};
   }
   void place(sb::Arena &size)
   {
      for (Slab *s : {&iso_off, &exon_off, &seg_off, &exon_left, &exon_right, &seg_left, &seg_right}) s->off = size.take_nonempty(s->bytes);
   }
   sbgpu_annotation_t on_device(const sbgpu_annotation_t &an, const char *base) const
   {
      sbgpu_annotation_t d = an;
      d.iso_off = (const int64_t *)(base + iso_off.off), d.exon_off = (const int64_t *)(base + exon_off.off);
      d.seg_off = (const int64_t *)(base + seg_off.off);
      d.exon_left = (const uint32_t *)(base + exon_left.off), d.exon_right = (const uint32_t *)(base + exon_right.off);
      d.seg_left = (const uint32_t *)(base + seg_left.off), d.seg_right = (const uint32_t *)(base + seg_right.off);
      return d;
   }
};
// the hits' arrays and masses likewise (sbgpu_quantify_host only: the other entries are given them in HBM)
struct HitsLayout {
   Slab feat_off, hit_locus, feat_left, feat_right, feat_code, mass;
   HitsLayout(const sbgpu_hits_t *h, const float *hit_mass, int64_t n_feat, bool resident)
   {
      const size_t on = resident ? 0 : 1, nh = (size_t)h->n_hits;
      feat_off = {h->feat_off, nh ? on * (nh + 1) * 8 : 0, 0}, hit_locus = {h->hit_locus, on * nh * 4, 0};
      feat_left = {h->feat_left, on * (size_t)n_feat * 4, 0}, feat_right = {h->feat_right, on * (size_t)n_feat * 4, 0};
      feat_code = {h->feat_code, on * (size_t)n_feat, 0}, mass = {hit_mass, on * nh * 4, 0};
   }
   void place(sb::Arena &size)
   {
      for (Slab *s : {&feat_off, &hit_locus, &feat_left, &feat_right, &feat_code, &mass}) s->off = size.take_nonempty(s->bytes);
   }
   sbgpu_hits_t on_device(const sbgpu_hits_t &h, const char *base) const
   {
      sbgpu_hits_t d = h;
      d.feat_off = (const int64_t *)(base + feat_off.off), d.hit_locus = (const int32_t *)(base + hit_locus.off);
      d.feat_left = (const uint32_t *)(base + feat_left.off), d.feat_right = (const uint32_t *)(base + feat_right.off);
      d.feat_code = (const uint8_t *)(base + feat_code.off);
      return d;
   }
};
// scratch slot 0 of a call: the inputs it uploads and the per-hit words the exon-bin kernel makes of them
struct InputArena {
   AnnotationLayout annot;
   HitsLayout hits;
   size_t o_compat = 0, o_key = 0, o_hit_bin = 0, o_span = 0, o_fhash = 0, total = 0;
   char *base = nullptr;
   InputArena(const AnnotationLayout &a, const HitsLayout &h, size_t nh1, int32_t cw, int32_t kw) : annot(a), hits(h)
   {
      sb::Arena size;
      annot.place(size), hits.place(size);
      o_compat = size.take(nh1 * 4 * (size_t)cw), o_key = size.take(nh1 * 4 * (size_t)kw);
      o_hit_bin = size.take(8); // (hit -> bin has an arena of its own where it is made at all)
      o_span = size.take(nh1 * 8), o_fhash = size.take(nh1 * 4);
      total = size.size;
   }
   // one copy per array, in this order
   std::array<const Slab *, 13> uploads() const
   {
      return {&annot.iso_off,   &annot.exon_off,  &annot.seg_off,   &hits.feat_off,  &annot.exon_left, &annot.exon_right, &annot.seg_left,
              &annot.seg_right, &hits.hit_locus,  &hits.feat_left,  &hits.feat_right, &hits.feat_code,  &hits.mass};
   }
   uint32_t *compat() const { return (uint32_t *)(base + o_compat); }
   uint32_t *key() const { return (uint32_t *)(base + o_key); }
   int64_t *hit_bin() const { return (int64_t *)(base + o_hit_bin); }
   uint64_t *span() const { return (uint64_t *)(base + o_span); }
   uint32_t *fhash() const { return (uint32_t *)(base + o_fhash); }
};
// scratch slot 1 of a call: the host grouping's pair arrays, the bins' counts, the EM batch and what comes out of it.
// Exists once launch_weights has sized it: who reads it is handed one, so no offset is used before it is set.
struct WorkArena {
   char *base = nullptr;
   size_t o_pair_off = 0, o_pair_idx = 0, o_pair_seg = 0, o_pair_mask = 0, o_pair_len = 0, o_count = 0, o_F = 0, o_theta = 0, o_status = 0,
          o_iters = 0, o_fpkm = 0, o_frac = 0, o_tpm = 0, o_keep = 0, o_iso_len = 0, o_sum = 0, total = 0;
   // n_pairs / n_pair_segs: the pairs that come from the host (none: the device grouping's live in its own arena)
   WorkArena(int64_t n_pairs, int64_t n_pair_segs, int64_t n_bins, int64_t n_elem, int64_t n_iso, int64_t nl, bool epilogue)
   {
      const size_t np1 = (size_t)std::max<int64_t>(n_pairs, 1), ni1 = (size_t)(n_iso + 1), nl1 = (size_t)(nl + 1);
      sb::Arena size;
      o_pair_off = size.take((np1 + 1) * 8), o_pair_idx = size.take(np1 * 8), o_pair_seg = size.take((size_t)(n_pair_segs + 1) * 4);
      o_pair_mask = size.take(np1 * 4), o_pair_len = size.take(np1 * 4);
      o_count = size.take((size_t)std::max<int64_t>(n_bins, 1) * 4), o_F = size.take((size_t)std::max<int64_t>(n_elem, 1) * 8);
      o_theta = size.take(ni1 * 8), o_status = size.take(nl1 * 4), o_iters = size.take(nl1 * 4);
      if (epilogue) { // the epilogue's arrays (sbgpu_quantify_resident)
         o_fpkm = size.take(ni1 * 8), o_frac = size.take(ni1 * 8), o_tpm = size.take(ni1 * 8);
         o_keep = size.take(ni1 * 4), o_iso_len = size.take(ni1 * 4), o_sum = size.take(8);
      }
      total = size.size;
   }
   int64_t *pair_off() const { return (int64_t *)(base + o_pair_off); }
   int64_t *pair_idx() const { return (int64_t *)(base + o_pair_idx); }
   uint32_t *pair_seg() const { return (uint32_t *)(base + o_pair_seg); }
   uint32_t *pair_mask() const { return (uint32_t *)(base + o_pair_mask); }
   int32_t *pair_len() const { return (int32_t *)(base + o_pair_len); }
   int32_t *count() const { return (int32_t *)(base + o_count); }
   double *F() const { return (double *)(base + o_F); }
   double *theta() const { return (double *)(base + o_theta); }
   int32_t *status() const { return (int32_t *)(base + o_status); }
   int32_t *iters() const { return (int32_t *)(base + o_iters); }
   double *fpkm() const { return (double *)(base + o_fpkm); }
   double *frac() const { return (double *)(base + o_frac); }
   double *tpm() const { return (double *)(base + o_tpm); }
   int32_t *keep() const { return (int32_t *)(base + o_keep); }
   int32_t *iso_len() const { return (int32_t *)(base + o_iso_len); }
   double *fpkm_sum() const { return (double *)(base + o_sum); }
};

// What the chain needs of an annotation's shape.  widths: the widest locus in isoforms and in segments (the words per hit);
// span: the longest locus' segments together (the insert-size table reaches that far: no (bin, isoform) pair spans more).
// Two switches because a call on an annotation that is not pinned asks twice: the widths before it uploads anything, the
// span -- a pass over every segment -- while the exon-bin kernel runs, and not at all for long reads.
struct AnnotationExtent {
   int64_t max_iso = 1, max_seg = 1, max_locus_span = 1;
};
void scan_annotation(const sbgpu_annotation_t *an, bool widths, bool span, AnnotationExtent *x)
{
   for (int64_t l = 0; l < an->n_loci; ++l) {
      if (widths) {
         x->max_iso = std::max(x->max_iso, an->iso_off[l + 1] - an->iso_off[l]);
         x->max_seg = std::max(x->max_seg, an->seg_off[l + 1] - an->seg_off[l]);
      }
      if (span) {
         int64_t tot = 0;
         for (int64_t k = an->seg_off[l]; k < an->seg_off[l + 1]; ++k) tot += (int64_t)an->seg_right[k] - an->seg_left[k] + 1;
         x->max_locus_span = std::max(x->max_locus_span, tot);
      }
   }
}

// what sbgpu_quantify_resident adds to the chain: the epilogue behind the EM, with the path's collectives inside the call
struct ResidentOpts {
   int64_t mapped_reads;                   // this rank's part of Sample::total_mapped_reads()
   const sbgpu_abundance_params_t *params; // total_mapped_reads and insert_mean are filled in here
   sbgpu_comm_t *comm;                     // nullptr: a world of one
   sbgpu_abundances_t *out;
};
// one call's arguments, as the three entries hand them on
struct QuantifyArgs {
   sbgpu_ctx_t *c;
   const sbgpu_annotation_t *an;
   const sbgpu_hits_t *hits; // device arrays (like hit_mass) when dev_hit_off is given
   const float *hit_mass;
   const int64_t *dev_hit_off; // host, [n_loci + 1]: the hits are in HBM, grouped by locus like this; nullptr: host arrays
   const sbgpu_insert_t *insert;
   int32_t read_len, long_read;
   double *theta_out;
   int32_t *status_out, *iters_out;
   uint32_t *compat_out;
   sbgpu_insert_t *insert_used;
   sbgpu_bins_t **bins_out;
   const ResidentOpts *ro; // sbgpu_quantify_resident
};

// the insert-size law of a call: given, none (long reads), or the empirical one of the hits (pass 1 on the device)
struct InsertLaw {
   sbgpu_insert_t ins{};  // the law in use
   bool ready = false;    // its table is on its way to d_pdf (ev_pdf); else finish_law still has to make it of the histogram
   int32_t pdf_len = 0;
   std::vector<double> pdf;
   char *d_pdf = nullptr;
   hipStream_t copy_stream = nullptr; // the table travels beside the kernels
   hipEvent_t ev_pdf = nullptr, ev_hist = nullptr;
   int64_t hist_len = 0;
   const unsigned long long *h_hist = nullptr; // pinned: the histogram as the device (and the other ranks) made it
   std::vector<double> emp_hist;
   int64_t n_frag_lens = 0;
   int64_t mapped_total = 0; // Sample::total_mapped_reads() over all ranks (the resident entry)
};

// The host grouping's (bin, isoform) pairs and per-locus offsets, as sbgpu_bins_export gives them
struct ExportedBins {
   std::vector<int64_t> row_off, iso_off, f_off, pair_seg_off, pair_out;
   std::vector<int32_t> count, pair_len;
   std::vector<uint32_t> pair_segs, pair_mask;
};

// One sbgpu_quantify_* call: its state, and its stages in the order quantify_impl takes them.
struct QuantifyCall {
   const QuantifyArgs &a;
   sbgpu_ctx_t *const c;
   const sbgpu_annotation_t *const an;
   const ResidentOpts *const ro;
   const bool on_dev; // the hits are in HBM (sbgpu_quantify_device / _resident)
   hipStream_t s = nullptr;

   // -- shape (check_arguments)
   int64_t nl = 0, nh = 0, n_iso = 0, n_feat = 0;
   size_t nh1 = 1;
   int32_t cw = 1, kw = 1;
   AnnotationExtent extent;
   const sb::ResidentAnnotation *res = nullptr; // the annotation is the pinned one: its device copies and tables are used
   // -- what the call leaves for sbgpu_context_table_device
   sb::ContextKeep *keep_rec = nullptr;
   bool retain = false;
   const int32_t *d_hit_bin_local = nullptr;
   // -- what the call leaves for sbgpu_abundance_bootstrap_device (sbgpu_bootstrap_keep)
   sb::BootKeep *boot_rec = nullptr;
   bool boot_retain = false;
   const int32_t *d_iso_len = nullptr;     // the isoforms' lengths as the epilogue read them
   sbgpu_abundance_params_t epi_params{};  // the epilogue's parameters as it filled them in
   // -- SBGPU_HOST_TIMING: stage times on stderr; =2: host clock only, no synchronisation
   bool timing = false, timing_sync = false;
   double t_stage = 0;
   // -- the hits by locus (scan_hits_on_host, or the caller's)
   bool grouped = true;
   std::vector<int64_t> locus_hit_off;
   // -- inputs in HBM (upload_inputs)
   std::optional<InputArena> in;
   sbgpu_annotation_t dan{};
   sbgpu_hits_t dh{};
   const float *d_mass = nullptr;
   char *hit_bin_arena = nullptr; // hit -> bin of the host entry: the handle takes it over (finish_handle), else it goes back
   size_t hit_bin_cap = 0;
   sb::IsoSegments iso_pre;       // made by iso_thread
   std::thread iso_thread;
   std::vector<uint32_t> compat_h, key_h;
   // -- the law
   InsertLaw law;
   // -- bins, weights, EM
   int64_t n_bins = 0, n_elem = 0, n_pairs = 0, n_psegs = 0;
   std::optional<WorkArena> work; // read through work_arena()
   ExportedBins ex;
   sbgpu_plan_t *plan = nullptr;
   // the EM plan is host work of a millisecond or two (size classes, one upload): with the device grouping a helper
   // thread makes it as soon as the loci's bin counts are known, beside the pairs' kernels
   std::thread plan_thread;
   std::vector<int64_t> plan_row_off, plan_f_off;
   int plan_rc = SBGPU_OK;
   std::string plan_err;
   bool plan_started = false;
   const int32_t *d_count_dev = nullptr;
   sbgpu_bins_t *bins = nullptr; // ours until finish_handle hands it out
   bool rest_launched = false;   // the device grouping's hook launched the weights (the EM and epilogue follow it)
   bool grouped_on_device = false;
   std::string why_host;
   // -- results
   std::vector<double> F;
   hipError_t download_err = hipSuccess; // the first error of the downloads

   explicit QuantifyCall(const QuantifyArgs &args) : a(args), c(args.c), an(args.an), ro(args.ro), on_dev(args.dev_hit_off != nullptr) {}
   QuantifyCall(const QuantifyCall &) = delete;
   QuantifyCall &operator=(const QuantifyCall &) = delete;
   // Every return, early ones included, ends here.  The order matters:
   ~QuantifyCall()
   {
      if (plan_thread.joinable()) plan_thread.join(); // it writes `plan`, plan_rc and plan_err: over before any of them goes
      if (bins) sbgpu_bins_destroy(bins);             // a failure after the handle existed (finish_handle clears it)
      if (plan) sbgpu_plan_destroy(plan);
      sb::dev_give(hit_bin_arena, hit_bin_cap);       // (nothing once the handle has it)
      if (iso_thread.joinable()) iso_thread.join();   // it writes iso_pre, a member: joined before the members are destroyed
   }

   const WorkArena &work_arena() const
   {
      if (!work) std::abort(); // a stage behind launch_weights was called before it
      return *work;
   }
   static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
   void host_stage(const char *name)
   {
      if (!timing) return;
      if (timing_sync) (void)hipStreamSynchronize(s);
      const double t = now();
      std::fprintf(stderr, "sbgpu_quantify_host: %-18s %.2f ms\n", name, (t - t_stage) * 1e3);
      t_stage = t;
   }

   int check_arguments();
   int scan_hits_on_host();
   int upload_inputs();
   int run_exonbin();
   int need_compat();
   int begin_law();
   int begin_given_law();
   int begin_empirical_law();
   int finish_law();
   int launch_weights(const sb::DevicePairs *dpairs);
   int launch_em(const WorkArena &w, const int64_t *row_off, const int64_t *f_off, const int32_t *d_count, const int32_t *h_count);
   int launch_epilogue(const WorkArena &w);
   void start_plan_thread(const int64_t *row_off, const int64_t *f_off);
   int group_on_device();
   int group_on_host();
   int launch_from_handle();
   int download(const WorkArena &w);
   int finish_handle(const WorkArena &w);
};

int QuantifyCall::check_arguments()
{
   if (!c || !an || !a.hits || !a.bins_out || (!ro && (!a.theta_out || !a.status_out || !a.iters_out)))
      return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: null argument");
   *a.bins_out = nullptr;
   // what an earlier resident call kept for sbgpu_context_table_device lives in the scratch this call reuses: gone from here on
   keep_rec = sb::ctx_context_keep(c);
   keep_rec->serial = 0;
   retain = keep_rec->on && ro && on_dev;
   // likewise what was kept for sbgpu_abundance_bootstrap_device: that call's plan and the bootstrap's results go back
   sb::ctx_boot_release(c);
   boot_rec = sb::ctx_boot_keep(c);
   boot_retain = boot_rec->on && ro && on_dev;
   nl = an->n_loci, nh = a.hits->n_hits;
   if (nl < 1 || nh < 0) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: bad counts");
   if (!an->iso_off || !an->exon_off || !an->seg_off || (nh && (!a.hits->hit_locus || !a.hits->feat_off || !a.hit_mass)))
      return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: null array");
   if (!a.insert && !a.insert_used) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: insert_used is needed when no insert-size law is given");
   if (!a.insert && a.long_read && ro && ro->params && ro->params->effective_len_norm)
      return api_fail(SBGPU_EINVAL, "sbgpu_quantify_resident: effective_len_norm subtracts the law's mean, and long reads without a law have none");
   if (on_dev && a.compat_out) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_device: returns no compat words");
   n_iso = an->iso_off[nl];
   if (nh && !on_dev) n_feat = a.hits->feat_off[nh];
   nh1 = (size_t)std::max<int64_t>(nh, 1);
   // an annotation kept resident (sbgpu_annotation_pin) and given again: its device copies and tables are used as they are
   res = sb::ctx_resident_annotation(c);
   if (res && !res->matches(an)) res = nullptr;
   if (res) extent = {res->max_iso, res->max_seg, a.long_read ? 1 : res->max_locus_span};
   else scan_annotation(an, true, false, &extent); // (the span: begin_law, beside the exon-bin kernel)
   cw = (int32_t)((extent.max_iso + 31) / 32), kw = (int32_t)((extent.max_seg + 31) / 32);
   locus_hit_off.assign((size_t)nl + 1, 0);
   if (on_dev) {
      locus_hit_off.assign(a.dev_hit_off, a.dev_hit_off + nl + 1);
      if (locus_hit_off[0] != 0 || locus_hit_off[(size_t)nl] != nh) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_device: locus_hit_off does not cover the hits");
   }
   s = sb::ctx_stream(c);
   const char *timing_env = std::getenv("SBGPU_HOST_TIMING");
   timing = timing_env != nullptr, timing_sync = timing && std::atoi(timing_env) != 2;
   t_stage = now();
   return SBGPU_OK;
}

// Host hits: every hit's locus in range, and the hits grouped by locus?  (The device grouping needs it; the host one does not.)
// A pass over 4 bytes per hit (0.7 GB at 1.8e8 hits): split over a few host threads; the loci's offsets are then binary
// searches (grouped) or a counting pass (not grouped).
int QuantifyCall::scan_hits_on_host()
{
   if (!on_dev && nh) {
      const int32_t *hl = a.hits->hit_locus;
      const int T = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)16, (int64_t)std::thread::hardware_concurrency(), nh / (1 << 20) + 1}));
      std::vector<int> bad((size_t)T, 0), unsorted((size_t)T, 0);
      auto scan = [&](int t) {
         const int64_t h0 = nh * t / T, h1 = nh * (t + 1) / T;
         int b = 0, u = 0;
         int32_t prev = h0 ? hl[h0 - 1] : -1;
         for (int64_t h = h0; h < h1; ++h) {
            const int32_t l = hl[h];
            b |= (l < 0) | (l >= nl);
            u |= l < prev;
            // grouped hits: locus k's hits begin where the first locus >= k appears (the thread that sees the step writes the
            // entries; every step is seen by exactly one thread).  Garbage when the hits turn out not to be grouped: redone below.
            if (l > prev && !b && prev >= -1)
               for (int64_t k = (int64_t)prev + 1; k <= l; ++k) locus_hit_off[(size_t)k] = h;
            prev = l;
         }
         bad[(size_t)t] = b, unsorted[(size_t)t] = u;
      };
      {
         std::vector<std::thread> pool;
         try {
            for (int t = 1; t < T; ++t) pool.emplace_back(scan, t);
         } catch (const std::system_error &) { // fewer threads than hoped: the rest is done here
         }
         for (int t = (int)pool.size() + 1; t < T; ++t) scan(t);
         scan(0);
         for (std::thread &th : pool) th.join();
      }
      for (int t = 0; t < T; ++t) {
         if (bad[(size_t)t]) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: hit_locus out of range");
         if (unsorted[(size_t)t]) grouped = false;
      }
      if (grouped) {
         for (int64_t l = (int64_t)hl[nh - 1] + 1; l <= nl; ++l) locus_hit_off[(size_t)l] = nh; // loci behind the last hit
      } else {
         std::fill(locus_hit_off.begin(), locus_hit_off.end(), 0);
         for (int64_t h = 0; h < nh; ++h) ++locus_hit_off[(size_t)hl[h] + 1];
         for (int64_t l = 0; l < nl; ++l) locus_hit_off[(size_t)l + 1] += locus_hit_off[(size_t)l];
      }
   }
   host_stage("validate hits");
   return SBGPU_OK;
}

// ---- inputs: one arena, one copy per array that is not in HBM already
int QuantifyCall::upload_inputs()
{
   in.emplace(AnnotationLayout(an, AnnotationCounts(an), res != nullptr), HitsLayout(a.hits, a.hit_mass, n_feat, on_dev), nh1, cw, kw);
   if (hipError_t e = sb::ctx_scratch(c, 0, in->total, &in->base); e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   // The isoforms' segment lists depend on the annotation only: a helper thread makes them (1 ms of host work for
   // 20 000 loci) while this one feeds the uploads.
   if (grouped && nh && !res) {
      try {
         iso_thread = std::thread([this]() { sb::iso_segments(an, &iso_pre); });
      } catch (const std::system_error &) { // no thread to be had: make them here
         sb::iso_segments(an, &iso_pre);
      }
   }
   for (const Slab *p : in->uploads())
      if (p->bytes) SB_TRY(hipMemcpyAsync(in->base + p->off, p->src, p->bytes, hipMemcpyHostToDevice, s));
   dan = res ? res->dev : in->annot.on_device(*an, in->base);
   dh = on_dev ? *a.hits : in->hits.on_device(*a.hits, in->base);
   d_mass = on_dev ? a.hit_mass : (const float *)(in->base + in->hits.mass.off);
   // hit -> bin of the host entry: the handle keeps it in HBM (an arena of its own) and brings it over when an export asks
   if (!on_dev && nh) {
      if (hipError_t e = sb::dev_take((size_t)nh * 8, &hit_bin_arena, &hit_bin_cap); e != hipSuccess) return api_fail_hip(e, "hipMalloc(hit -> bin)");
   }
   host_stage("upload");
   return SBGPU_OK;
}

// ---- A5: the interval tests
int QuantifyCall::run_exonbin()
{
   sb::ctx_stage_reset(c);
   sb::ctx_stage_begin(c, "exonbin_kernel", s);
   if (nh) SB_RC(sb::exonbin_device_impl(c, &dan, &dh, cw, kw, in->compat(), in->key(), in->span(), in->fhash(), s, n_iso, res ? &res->seg_basis : nullptr));
   sb::ctx_stage_end(c, s);
   host_stage("exonbin kernel");
   return SBGPU_OK;
}

// the compat words on the host (the host grouping, and a caller that asked for them): downloaded once
int QuantifyCall::need_compat()
{
   if (compat_h.empty() && nh) {
      compat_h.resize((size_t)nh * cw);
      SB_TRY(hipMemcpyAsync(compat_h.data(), in->compat(), compat_h.size() * 4, hipMemcpyDeviceToHost, s));
      SB_TRY(hipStreamSynchronize(s));
   }
   return SBGPU_OK;
}

// ---- the insert-size law: given, or the empirical one from the hits (pass 1 of the reference: Sample::fragLenDist,
// src/alignments.cpp:1363-1410, on the device -- fraglen_device.h)
int QuantifyCall::begin_law()
{
   if (!a.long_read && !res) scan_annotation(an, false, true, &extent);
   if (extent.max_locus_span > (1 << 26)) return api_fail(SBGPU_ESHAPE, "sbgpu_quantify_host: segment lengths out of range");
   law.pdf_len = (int32_t)extent.max_locus_span + 1;
   if (hipError_t e = sb::ctx_scratch(c, 6, (size_t)law.pdf_len * 8, &law.d_pdf); e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   law.pdf.assign((size_t)law.pdf_len, 0.0);
   SB_TRY(sb::ctx_copy_stream(c, &law.copy_stream));
   SB_TRY(sb::ctx_event(c, 3, &law.ev_pdf));
   law.mapped_total = ro ? ro->mapped_reads : 0;
   law.ready = a.insert != nullptr || a.long_read;
   SB_RC(law.ready ? begin_given_law() : begin_empirical_law());
   host_stage("pdf table");
   return SBGPU_OK;
}

int QuantifyCall::begin_given_law()
{
   // long reads without a law: the reference's long-read workflow builds none (Strawberry.cpp:335-337) and weighs every
   // bin 1/L (estimate.cpp:236-247), which reads no table; the law in use is all zeros (use_emp = 0)
   if (a.insert) law.ins = *a.insert;
   else law.ins = sbgpu_insert_t{};
   law.ins.read_len = a.read_len;
   law.ins.long_read = a.long_read;
   // the table of the law, on the copy stream beside the kernels (the bin-weight launch waits for its event)
   if (a.insert) SB_RC(sbgpu_insert_pdf_table(&law.ins, law.pdf_len, law.pdf.data()));
   SB_TRY(hipMemcpyAsync(law.d_pdf, law.pdf.data(), (size_t)law.pdf_len * 8, hipMemcpyHostToDevice, law.copy_stream));
   SB_TRY(hipEventRecord(law.ev_pdf, law.copy_stream));
   if (ro && ro->comm) { // Sample::total_mapped_reads() over all ranks (alignments.cpp:1372)
      SB_RC(sbgpu_allreduce_sum_i64_host(ro->comm, &law.mapped_total, 1));
   }
   return SBGPU_OK;
}

int QuantifyCall::begin_empirical_law()
{
   // every rank's histogram has the same length: the longest locus of any of them
   law.hist_len = law.pdf_len;
   if (ro && ro->comm) SB_RC(sbgpu_allreduce_max_i64_host(ro->comm, &law.hist_len, 1));
   const int64_t hist_len = law.hist_len;
   char *d_hist = nullptr, *pin = nullptr;
   const size_t hist_bytes = (size_t)(hist_len + 2) * 8; // [hist_len]: lengths beyond the table; [hist_len + 1]: the mapped-read total
   if (hipError_t e = sb::ctx_scratch(c, 7, hist_bytes, &d_hist); e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   SB_TRY(sb::ctx_pinned(c, 1, hist_bytes, &pin));
   SB_TRY(sb::ctx_event(c, 5, &law.ev_hist));
   SB_TRY(hipMemsetAsync(d_hist, 0, hist_bytes, s));
   if (ro) SB_TRY(hipMemcpyAsync(d_hist + (size_t)(hist_len + 1) * 8, &ro->mapped_reads, 8, hipMemcpyHostToDevice, s));
   sb::ctx_stage_begin(c, "fraglen_hist_kernel", s);
   if (nh) {
      sb::FragLenArgs fa;
      fa.n_hits = nh, fa.compat_words = cw;
      fa.hit_locus = dh.hit_locus, fa.compat = in->compat(), fa.span = in->span();
      fa.iso_off = dan.iso_off, fa.exon_off = dan.exon_off, fa.exon_left = dan.exon_left, fa.exon_right = dan.exon_right;
      fa.hist_len = hist_len, fa.hist = (unsigned long long *)d_hist;
      const int64_t want = std::min<int64_t>((nh + sb::kFragLenThreads - 1) / sb::kFragLenThreads, (int64_t)sb::ctx_cu_count(c) * 2);
      hipLaunchKernelGGL(sb::fraglen_hist_kernel, dim3((unsigned)want), dim3(sb::kFragLenThreads), 0, s, fa);
      SB_TRY(hipGetLastError());
   }
   sb::ctx_stage_end(c, s);
   // the law is the WHOLE sample's: one all-reduce(sum) of the histogram (exact integers) with the mapped-read total behind it
   if (ro && ro->comm) SB_RC(sbgpu_allreduce_sum_i64(ro->comm, (int64_t *)d_hist, hist_len + 2, s));
   SB_TRY(hipMemcpyAsync(pin, d_hist, hist_bytes, hipMemcpyDeviceToHost, s));
   SB_TRY(hipEventRecord(law.ev_hist, s));
   law.h_hist = (const unsigned long long *)pin;
   return SBGPU_OK;
}

// called before the bin weights are launched: by then the histogram has long arrived (the grouping's kernels ran behind it)
int QuantifyCall::finish_law()
{
   if (law.ready) return SBGPU_OK;
   const unsigned long long *h_hist = law.h_hist;
   const int64_t hist_len = law.hist_len;
   SB_TRY(hipEventSynchronize(law.ev_hist));
   if (h_hist[hist_len]) return api_fail(SBGPU_ESHAPE, "sbgpu_quantify_host: a fragment length beyond the longest locus");
   if (ro) law.mapped_total = (int64_t)h_hist[hist_len + 1];
   // InsertSize(const vector<int> frag_lens), src/read.cpp:238-262; mean_and_sd_insert_size :14-20 -- size, sum, sum of
   // squares, extremes and histogram of the sample, all read off the histogram (integers: exact in any order; the
   // reference's running doubles are the same numbers as long as they stay below 2^53)
   int64_t lo = -1, hi = -1;
   unsigned long long n = 0;
   unsigned __int128 sum = 0, sq = 0;
   for (int64_t l = 0; l < hist_len; ++l)
      if (const unsigned long long k = h_hist[l]) {
         if (lo < 0) lo = l;
         hi = l;
         n += k;
         sum += (unsigned __int128)k * (unsigned long long)l;
         sq += (unsigned __int128)k * (unsigned long long)l * (unsigned long long)l;
      }
   if (n < 1) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_host: no hit fits exactly one transcript: no empirical insert-size law (\"Not enough reads\")");
   if (n > (unsigned long long)INT32_MAX) return api_fail(SBGPU_ESHAPE, "sbgpu_quantify_host: more than 2^31 fragment lengths");
   law.emp_hist.assign((size_t)(hi - lo + 1), 0.0);
   for (int64_t l = lo; l <= hi; ++l) law.emp_hist[(size_t)(l - lo)] = (double)h_hist[l];
   law.n_frag_lens = (int64_t)n;
   sbgpu_insert_t &ins = law.ins;
   ins.mean = (double)sum / (double)n;
   ins.sd = std::sqrt((double)sq / (double)n - ins.mean * ins.mean);
   ins.use_emp = 1;
   ins.start_offset = (int32_t)lo;
   ins.end_offset = (int32_t)hi;
   ins.total_reads = (int32_t)n;
   ins.emp_hist = law.emp_hist.data();
   ins.read_len = a.read_len;
   ins.long_read = a.long_read;
   SB_RC(sbgpu_insert_pdf_table(&ins, law.pdf_len, law.pdf.data()));
   SB_TRY(hipMemcpyAsync(law.d_pdf, law.pdf.data(), (size_t)law.pdf_len * 8, hipMemcpyHostToDevice, law.copy_stream));
   SB_TRY(hipEventRecord(law.ev_pdf, law.copy_stream));
   law.ready = true;
   host_stage("insert size");
   return SBGPU_OK;
}

// ---- A4: the bin weights, straight into the EM batch's F.  dpairs: the pairs are in HBM (the device grouping's arena);
// nullptr: they come from the handle's export (ex) and are uploaded here.  Sizes the work arena: n_bins, n_elem, n_pairs
// and n_psegs are set by now.
int QuantifyCall::launch_weights(const sb::DevicePairs *dpairs)
{
   if (!a.long_read) {
      if (dpairs) {
         if (dpairs->any_wide) return api_fail(SBGPU_ESHAPE, "sbgpu_quantify_host: a bin spans more than 32 isoform segments");
      } else {
         for (int64_t p = 0; p < n_pairs; ++p)
            if (ex.pair_seg_off[(size_t)p + 1] == ex.pair_seg_off[(size_t)p])
               return api_fail(SBGPU_ESHAPE, "sbgpu_quantify_host: a bin spans more than 32 isoform segments");
      }
   }
   work.emplace(dpairs ? 0 : n_pairs, dpairs ? 0 : n_psegs, n_bins, n_elem, n_iso, nl, ro != nullptr);
   WorkArena &w = *work;
   if (hipError_t e = sb::ctx_scratch(c, 1, w.total, &w.base); e != hipSuccess) return api_fail_hip(e, "hipMalloc");
   SB_TRY(hipMemsetAsync(w.F(), 0, (size_t)std::max<int64_t>(n_elem, 1) * 8, s));
   SB_RC(finish_law());
   SB_TRY(hipStreamWaitEvent(s, law.ev_pdf, 0));
   if (n_pairs) {
      if (!dpairs) {
         SB_TRY(hipMemcpyAsync(w.pair_off(), ex.pair_seg_off.data(), (size_t)(n_pairs + 1) * 8, hipMemcpyHostToDevice, s));
         SB_TRY(hipMemcpyAsync(w.pair_idx(), ex.pair_out.data(), (size_t)n_pairs * 8, hipMemcpyHostToDevice, s));
         if (n_psegs) SB_TRY(hipMemcpyAsync(w.pair_seg(), ex.pair_segs.data(), (size_t)n_psegs * 4, hipMemcpyHostToDevice, s));
         SB_TRY(hipMemcpyAsync(w.pair_mask(), ex.pair_mask.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
         SB_TRY(hipMemcpyAsync(w.pair_len(), ex.pair_len.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
      }
      const sbgpu_insert_t &ins = law.ins;
      const int32_t lmin_base = ins.use_emp ? ins.start_offset : ins.read_len;
      sb::ctx_stage_begin(c, "binweight_kernel", s);
      SB_RC(sbgpu_binweight_device(c, n_pairs, dpairs ? dpairs->seg_off() : w.pair_off(), dpairs ? dpairs->seg_lens() : w.pair_seg(),
                                   dpairs ? dpairs->mask() : w.pair_mask(), dpairs ? dpairs->iso_len() : w.pair_len(),
                                   dpairs ? dpairs->out_index() : w.pair_idx(), (const double *)law.d_pdf, law.pdf_len, ins.read_len, lmin_base,
                                   ins.long_read, w.F(), s));
      sb::ctx_stage_end(c, s);
   }
   host_stage("bin weights");
   return SBGPU_OK;
}

// ---- A1/A2: the EM behind them (the counts are on the device already when the grouping ran there)
int QuantifyCall::launch_em(const WorkArena &w, const int64_t *row_off, const int64_t *f_off, const int32_t *d_count, const int32_t *h_count)
{
   if (!d_count) {
      if (n_bins) SB_TRY(hipMemcpyAsync(w.count(), h_count, (size_t)n_bins * 4, hipMemcpyHostToDevice, s));
      d_count = w.count();
   }
   if (plan_started) {
      plan_thread.join();
      plan_started = false;
      if (plan_rc != SBGPU_OK) return api_fail(plan_rc, plan_err);
   } else {
      SB_RC(sbgpu_plan_create(c, nl, row_off, an->iso_off, f_off, &plan));
   }
   host_stage("plan");
   sb::ctx_stage_begin(c, "em kernels", s);
   const int rce = sbgpu_em_run_device(c, plan, d_count, w.F(), w.theta(), w.status(), w.iters(), s);
   sb::ctx_stage_end(c, s);
   return rce;
}

// ---- A3 / A7 behind the EM (sbgpu_quantify_resident): theta -> FPKM / Frac / keep (estimate.cpp:314-355), the FPKM total of
// ALL ranks (alignments.cpp:1821-1824: the path's one collective per step), TPM (:1825-1829) -- theta never leaves the device
int QuantifyCall::launch_epilogue(const WorkArena &w)
{
   if (!ro) return SBGPU_OK;
   if (law.mapped_total < 1 || law.mapped_total > (int64_t)INT32_MAX)
      return api_fail(SBGPU_EINVAL, "sbgpu_quantify_resident: the mapped-read total must be in [1, 2^31) (Sample::total_mapped_reads() is an int)");
   const int32_t *d_len = nullptr;
   if (res) {
      d_len = res->d_iso.len;
   } else {
      if ((int64_t)iso_pre.len.size() != n_iso) sb::iso_segments(an, &iso_pre);
      SB_TRY(hipMemcpyAsync(w.iso_len(), iso_pre.len.data(), (size_t)n_iso * 4, hipMemcpyHostToDevice, s));
      d_len = w.iso_len();
   }
   sbgpu_abundance_params_t par = *ro->params;
   par.total_mapped_reads = (int32_t)law.mapped_total;
   par.insert_mean = law.ins.mean; // _sample._insert_size_dist->_mean (estimate.cpp:318)
   sb::ctx_stage_begin(c, "abundance + tpm", s);
   d_iso_len = d_len, epi_params = par;
   SB_RC(sbgpu_abundance_device(c, plan, w.theta(), w.status(), d_len, &par, w.fpkm(), w.frac(), w.keep(), w.fpkm_sum(), s));
   if (ro->comm) SB_RC(sbgpu_allreduce_sum_f64(ro->comm, w.fpkm_sum(), 1, s));
   SB_RC(sbgpu_tpm_device(c, n_iso, w.fpkm(), w.keep(), w.fpkm_sum(), w.tpm(), s));
   sb::ctx_stage_end(c, s);
   return SBGPU_OK;
}

void QuantifyCall::start_plan_thread(const int64_t *row_off, const int64_t *f_off)
{
   plan_row_off.assign(row_off, row_off + nl + 1); // (the grouping's arrays do not outlive its frame)
   plan_f_off.assign(f_off, f_off + nl + 1);
   try {
      plan_thread = std::thread([this]() {
         plan_rc = sbgpu_plan_create(c, nl, plan_row_off.data(), an->iso_off, plan_f_off.data(), &plan);
         if (plan_rc != SBGPU_OK) plan_err = sbgpu_last_error(); // (the error slot is per thread)
      });
      plan_started = true;
   } catch (const std::system_error &) { // no thread to be had: launch_em makes the plan
   }
}

// ---- A5 on the device: the grouping with everything behind the bins launched from inside it.  The weights go in from the
// after_pairs hook -- as soon as the pairs' fill kernel is in the stream -- so that the handle's bookkeeping runs beside that
// kernel; the EM goes in once the plan's thread is through, still before the weights are done.
// SBGPU_EUNSUPPORTED: the grouping declined (nothing behind it was launched then); any failure leaves no plan and no thread.
int QuantifyCall::group_on_device()
{
   if (iso_thread.joinable()) iso_thread.join();
   sb::GroupingHooks hooks;
   hooks.d_annot = &dan;
   if (res) hooks.d_iso = &res->d_iso;
   hooks.rows_known = [this](const int64_t *row_off, const int64_t *f_off) { start_plan_thread(row_off, f_off); };
   hooks.after_pairs = [this](const sb::DeviceGrouping &g) -> int {
      n_bins = g.n_bins, n_elem = g.n_elem, n_pairs = g.pairs->n_pairs, n_psegs = g.pairs->n_pair_segs;
      d_count_dev = g.d_count; // (the handle's own arena, sb::dev_take'n by the grouping: valid as long as the handle lives)
      rest_launched = true;
      return launch_weights(g.pairs);
   };
   if (retain) hooks.d_hit_bin_local = &d_hit_bin_local; // (the context table reads hit -> bin as the grouping's 4-byte local ranks)
   // (hits given on the device: the caller did not ask for hit -> bin, so it is not made)
   int64_t *d_hit_bin = on_dev ? nullptr : hit_bin_arena ? (int64_t *)hit_bin_arena : in->hit_bin();
   int rc = sb::bins_create_device_impl(c, an, &dh, d_mass, locus_hit_off.data(), cw, kw, in->compat(), in->key(), d_hit_bin, s,
                                        res ? &res->iso : &iso_pre, &bins, in->span(), in->fhash(), &hooks);
   if (rc == SBGPU_OK && rest_launched) rc = launch_em(work_arena(), plan_row_off.data(), plan_f_off.data(), d_count_dev, nullptr);
   if (rc == SBGPU_OK && rest_launched) rc = launch_epilogue(work_arena());
   if (rc != SBGPU_OK) {
      // a grouping that failed after the plan's thread was started: the thread is over before anything else happens
      if (plan_thread.joinable()) plan_thread.join();
      plan_started = false;
      if (rest_launched) (void)hipStreamSynchronize(s);
      if (plan) {
         sbgpu_plan_destroy(plan);
         plan = nullptr;
      }
   }
   return rc;
}

// ---- A5 on the host (same bins, slower), after a decline or for hits the device grouping is not tried on: the handle says
// so and why (sbgpu_bins_grouping).  Called with the decline's text still in sbgpu_last_error.
int QuantifyCall::group_on_host()
{
   if (on_dev && nh) // (no hits at all: the host code makes the empty handle)
      return api_fail(SBGPU_EUNSUPPORTED, "sbgpu_quantify_device: the device grouping does not cover these hits (unsorted, fractional masses or a locus of thousands of bins): use sbgpu_quantify_host");
   why_host = !nh ? "no hits" : !grouped ? "the hits are not grouped by locus" : sbgpu_last_error();
   if (timing && nh) std::fprintf(stderr, "sbgpu_quantify_host: the device grouping declined: %s\n", why_host.c_str());
   SB_RC(need_compat());
   key_h.resize(nh1 * (size_t)kw);
   if (nh) {
      SB_TRY(hipMemcpyAsync(key_h.data(), in->key(), (size_t)nh * kw * 4, hipMemcpyDeviceToHost, s));
      SB_TRY(hipStreamSynchronize(s));
   }
   if (compat_h.empty()) compat_h.resize((size_t)cw);
   SB_RC(sbgpu_bins_create(an, a.hits, a.hit_mass, cw, kw, compat_h.data(), key_h.data(), &bins));
   sb::bins_set_grouping(bins, false, why_host);
   return SBGPU_OK;
}

// the weights, the EM and the epilogue where the grouping's hook did not launch them (host grouping, or no hits at all):
// the pairs come from the handle
int QuantifyCall::launch_from_handle()
{
   int64_t info[8];
   SB_RC(sbgpu_bins_info(bins, info));
   n_bins = info[2], n_elem = info[3], n_pairs = info[4], n_psegs = info[5];
   const sb::DevicePairs *dpairs = sb::bins_device_pairs(bins);
   ex.row_off.resize((size_t)nl + 1), ex.iso_off.resize((size_t)nl + 1), ex.f_off.resize((size_t)nl + 1), ex.count.resize((size_t)n_bins + 1);
   if (!dpairs) {
      ex.pair_seg_off.resize((size_t)n_pairs + 1);
      ex.pair_out.resize((size_t)n_pairs + 1);
      ex.pair_len.resize((size_t)n_pairs + 1);
      ex.pair_segs.resize((size_t)n_psegs + 1);
      ex.pair_mask.resize((size_t)n_pairs + 1);
   }
   SB_RC(sbgpu_bins_export(bins, ex.row_off.data(), ex.iso_off.data(), ex.f_off.data(), ex.count.data(), nullptr, nullptr, nullptr, nullptr,
                           dpairs ? nullptr : ex.pair_seg_off.data(), dpairs ? nullptr : ex.pair_segs.data(),
                           dpairs ? nullptr : ex.pair_mask.data(), dpairs ? nullptr : ex.pair_len.data(),
                           dpairs ? nullptr : ex.pair_out.data()));
   host_stage("export");
   SB_RC(launch_weights(dpairs));
   SB_RC(launch_em(work_arena(), ex.row_off.data(), ex.f_off.data(), nullptr, ex.count.data()));
   return launch_epilogue(work_arena());
}

// the results come down last: a copy into the caller's pageable memory holds the host until the EM is done, and
// the handle's host work is to run beside the kernels, not behind them
int QuantifyCall::download(const WorkArena &w)
{
   auto get = [this](void *dst, const void *src, size_t bytes) {
      if (!dst) return;
      const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
      if (download_err == hipSuccess) download_err = e;
   };
   F.assign(on_dev ? (size_t)0 : (size_t)n_elem, 0.0); // (device entry: the weights are not brought back)
   get(ro ? ro->out->theta : a.theta_out, w.theta(), (size_t)n_iso * 8);
   get(ro ? ro->out->status : a.status_out, w.status(), (size_t)nl * 4);
   get(ro ? ro->out->iters : a.iters_out, w.iters(), (size_t)nl * 4);
   if (n_elem && !on_dev) get(F.data(), w.F(), (size_t)n_elem * 8);
   if (ro) {
      sbgpu_abundances_t *o = ro->out;
      get(o->fpkm, w.fpkm(), (size_t)n_iso * 8), get(o->frac, w.frac(), (size_t)n_iso * 8), get(o->tpm, w.tpm(), (size_t)n_iso * 8);
      get(o->keep, w.keep(), (size_t)n_iso * 4), get(&o->total_fpkm, w.fpkm_sum(), 8);
      o->d_theta = w.theta(), o->d_fpkm = w.fpkm(), o->d_frac = w.frac(), o->d_tpm = w.tpm(), o->d_keep = w.keep();
      o->d_status = w.status(), o->d_iters = w.iters();
      o->total_mapped_reads = law.mapped_total, o->n_frag_lens = law.n_frag_lens;
   }
   const hipError_t e_sync = hipStreamSynchronize(s);
   if (download_err == hipSuccess) download_err = e_sync;
   host_stage("plan + EM + download");
   if (download_err != hipSuccess) return api_fail(SBGPU_EHIP, std::string("sbgpu_quantify_host: download: ") + hipGetErrorString(download_err));
   // a wide-locus barrier that timed out leaves its loci unsolved (status SBGPU_EM_UNSOLVED): that is a failed call
   if (sb::ctx_take_wide_error(c))
      return api_fail(SBGPU_EHIP, "sbgpu_quantify_host: a barrier of the wide-locus EM kernel timed out: the loci it served have no result");
   return SBGPU_OK;
}

// what the caller gets beside the arrays: the compat words, the law in use, and the handle with what lives on in it
int QuantifyCall::finish_handle(const WorkArena &w)
{
   if (a.compat_out) {
      SB_RC(need_compat());
      if (nh) std::memcpy(a.compat_out, compat_h.data(), (size_t)nh * cw * 4);
   }
   if (grouped_on_device && nh && !on_dev) { // hit -> bin stays in HBM with the handle (8 bytes per hit cross PCIe on request only)
      sb::bins_set_device_hit_bin(bins, hit_bin_arena, hit_bin_cap, nh);
      hit_bin_arena = nullptr, hit_bin_cap = 0;
   }
   if (grouped && nh && !on_dev) sb::bins_set_locus_hit_off(bins, locus_hit_off); // (the host grouping notes it itself)
   if (a.insert_used) *a.insert_used = law.ins;
   if (a.insert_used && !a.insert && law.ins.use_emp) {
      // the histogram lives on with the handle: behind the weights
      const size_t at = F.size();
      F.insert(F.end(), law.emp_hist.begin(), law.emp_hist.end());
      sb::bins_set_weights(bins, std::move(F));
      a.insert_used->emp_hist = sb::bins_weights_tail(bins, at);
   } else {
      sb::bins_set_weights(bins, std::move(F));
   }
   static std::atomic<uint64_t> serial{0};
   if (boot_retain && plan) {
      // sbgpu_bootstrap_keep: the plan changes hands, the rest is said where it lies (nothing is copied)
      boot_rec->serial = ++serial;
      boot_rec->plan = plan, plan = nullptr;
      boot_rec->n_loci = nl, boot_rec->n_iso = n_iso;
      boot_rec->d_count = d_count_dev ? d_count_dev : w.count(); // (the handle's arena / the no-hits route's upload)
      boot_rec->d_F = w.F(), boot_rec->d_iso_len = d_iso_len;
      boot_rec->params = epi_params;
      // the law the weights were made under, as a copy the record owns
      boot_rec->insert = law.ins, boot_rec->insert_table = a.insert != nullptr || !a.long_read, boot_rec->pdf_len = law.pdf_len;
      boot_rec->insert_hist.clear();
      if (law.ins.use_emp && law.ins.emp_hist && law.ins.end_offset >= law.ins.start_offset)
         boot_rec->insert_hist.assign(law.ins.emp_hist, law.ins.emp_hist + ((int64_t)law.ins.end_offset - law.ins.start_offset + 1));
      boot_rec->insert.emp_hist = boot_rec->insert_hist.empty() ? nullptr : boot_rec->insert_hist.data();
      sb::bins_set_boot_serial(bins, boot_rec->serial);
   }
   if (retain) {
      // sbgpu_context_table_keep: say where the table's inputs are (all of them this call's scratch, nothing is copied)
      keep_rec->serial = ++serial;
      keep_rec->n_hits = nh, keep_rec->n_loci = nl, keep_rec->n_iso = n_iso, keep_rec->compat_words = cw;
      keep_rec->d_compat = in->compat(), keep_rec->d_hit_bin_local = d_hit_bin_local;
      keep_rec->d_F = w.F();
      keep_rec->d_keep = w.keep(), keep_rec->d_status = w.status();
      keep_rec->locus_hit_off = locus_hit_off;
      sb::bins_set_context_serial(bins, keep_rec->serial);
   }
   *a.bins_out = bins;
   bins = nullptr;
   host_stage("results + handle");
   return SBGPU_OK;
}

// The chain, top to bottom.  Three entries come through here:
//   sbgpu_quantify_host      host arrays in: the hits are checked and uploaded; theta / status / iterations, the compat words
//                            and the weights (in the handle) come back;
//   sbgpu_quantify_device    the hits are in HBM already (dev_hit_off says how they are grouped): nothing of them is uploaded,
//                            no hit -> bin, no weights and no compat words come back;
//   sbgpu_quantify_resident  the device entry with `ro`: the mapped-read total beside the law, the abundance epilogue behind
//                            the EM, and the collectives of a sharded sample inside the call.
// In each, an annotation that is pinned (sbgpu_annotation_pin) is not uploaded either.  Behind the exon-bin kernel there are
// two routes:
//   device grouping  hits grouped by locus: the grouping's hooks launch the plan's thread and the weights from inside it, the
//                    EM and the epilogue follow at once, and the handle is built beside the kernels (group_on_device);
//   host grouping    the device grouping declined (SBGPU_EUNSUPPORTED), the hits are not grouped, or there are none: the words
//                    come to the host, the library's host code groups, and the weights, the EM and the epilogue are launched
//                    from the handle's export (group_on_host, launch_from_handle).  The device entries refuse this route.
int quantify_impl(const QuantifyArgs &args)
{
   QuantifyCall q(args);
   SB_RC(q.check_arguments());
   SB_RC(q.scan_hits_on_host());
   SB_RC(q.upload_inputs());
   SB_RC(q.run_exonbin());
   SB_RC(q.begin_law());
   int rc = SBGPU_EUNSUPPORTED;
   if (q.grouped && q.nh) rc = q.group_on_device();
   q.grouped_on_device = rc == SBGPU_OK;
   if (rc == SBGPU_EUNSUPPORTED && !q.rest_launched) rc = q.group_on_host();
   if (rc != SBGPU_OK) return rc;
   q.host_stage("bins + pairs");
   if (!q.rest_launched) SB_RC(q.launch_from_handle());
   const WorkArena &w = q.work_arena();
   SB_RC(q.download(w));
   return q.finish_handle(w);
}

} // namespace

extern "C" {

int sbgpu_quantify_host(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *hits, const float *hit_mass,
                        const sbgpu_insert_t *insert, int32_t read_len, int32_t long_read, double *theta_out,
                        int32_t *status_out, int32_t *iters_out, uint32_t *compat_out, sbgpu_insert_t *insert_used,
                        sbgpu_bins_t **bins_out)
{
   return quantify_impl({c, an, hits, hit_mass, nullptr, insert, read_len, long_read, theta_out, status_out, iters_out, compat_out,
                         insert_used, bins_out, nullptr});
}

int sbgpu_quantify_device(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *d_hits, const float *d_hit_mass,
                          const int64_t *locus_hit_off, const sbgpu_insert_t *insert, int32_t read_len, int32_t long_read,
                          double *theta_out, int32_t *status_out, int32_t *iters_out, sbgpu_bins_t **bins_out)
{
   if (!locus_hit_off) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_device: null locus_hit_off");
   sbgpu_insert_t used;
   return quantify_impl({c, an, d_hits, d_hit_mass, locus_hit_off, insert, read_len, long_read, theta_out, status_out, iters_out,
                         nullptr, &used, bins_out, nullptr});
}

int sbgpu_quantify_resident(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, const sbgpu_hits_t *d_hits, const float *d_hit_mass,
                            const int64_t *locus_hit_off, const sbgpu_insert_t *insert, int32_t read_len, int32_t long_read,
                            int64_t mapped_reads, const sbgpu_abundance_params_t *params, sbgpu_comm_t *comm,
                            sbgpu_insert_t *insert_used, sbgpu_abundances_t *out, sbgpu_bins_t **bins_out)
{
   if (!locus_hit_off || !params || !out) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_resident: null argument");
   if (mapped_reads < 0) return api_fail(SBGPU_EINVAL, "sbgpu_quantify_resident: negative mapped-read count");
   sbgpu_insert_t used;
   const ResidentOpts ro = {mapped_reads, params, comm, out};
   return quantify_impl({c, an, d_hits, d_hit_mass, locus_hit_off, insert, read_len, long_read, nullptr, nullptr, nullptr, nullptr,
                         insert_used ? insert_used : &used, bins_out, &ro});
}

int sbgpu_annotation_pin(sbgpu_ctx_t *c, const sbgpu_annotation_t *an)
{
   if (!c || !an) return api_fail(SBGPU_EINVAL, "sbgpu_annotation_pin: null argument");
   if (an->n_loci < 1 || !an->iso_off || !an->exon_off || !an->seg_off) return api_fail(SBGPU_EINVAL, "sbgpu_annotation_pin: bad annotation");
   const AnnotationCounts n(an);
   if ((n.n_exon && (!an->exon_left || !an->exon_right)) || (n.n_seg && (!an->seg_left || !an->seg_right)))
      return api_fail(SBGPU_EINVAL, "sbgpu_annotation_pin: null array");
   sb::ResidentAnnotation *r = new (std::nothrow) sb::ResidentAnnotation();
   if (!r) return api_fail(SBGPU_ENOMEM, "sbgpu_annotation_pin: out of host memory");
   auto drop = [r](int rc) { // a pin that failed: its arena goes back
      sb::dev_give(r->arena, r->capacity);
      delete r;
      return rc;
   };
   r->key = *an;
   r->print = sb::ResidentAnnotation::fingerprint(an);
   AnnotationExtent x;
   scan_annotation(an, true, true, &x);
   r->max_iso = x.max_iso, r->max_seg = x.max_seg, r->max_locus_span = x.max_locus_span;
   sb::iso_segments(an, &r->iso);
   // the arena: the annotation, the isoforms' segment lists, the isoforms in the segment basis
   AnnotationLayout annot(an, n, false);
   Slab iso_seg_off = {r->iso.seg_off.data(), r->iso.seg_off.size() * 8, 0}, iso_seg_idx = {r->iso.seg_idx.data(), r->iso.seg_idx.size() * 4, 0},
        iso_locus = {r->iso.locus.data(), r->iso.locus.size() * 4, 0}, iso_len = {r->iso.len.data(), r->iso.len.size() * 4, 0};
   sb::Arena size;
   annot.place(size);
   for (Slab *p : {&iso_seg_off, &iso_seg_idx, &iso_locus, &iso_len}) p->off = size.take_nonempty(p->bytes);
   const size_t o_segbasis = size.size;
   size.size += sb::seg_basis_bytes(n.nl, n.n_iso);
   hipError_t e = hipSetDevice(sb::ctx_device(c));
   if (e == hipSuccess) e = sb::dev_take(size.size, &r->arena, &r->capacity);
   for (const Slab *p : {&annot.iso_off, &annot.exon_off, &annot.seg_off, &annot.exon_left, &annot.exon_right, &annot.seg_left, &annot.seg_right,
                         &iso_seg_off, &iso_seg_idx, &iso_locus, &iso_len})
      if (e == hipSuccess && p->bytes) e = hipMemcpy(r->arena + p->off, p->src, p->bytes, hipMemcpyHostToDevice);
   if (e != hipSuccess) return drop(api_fail_hip(e, "sbgpu_annotation_pin"));
   r->dev = annot.on_device(*an, r->arena);
   r->d_iso.seg_off = (const int64_t *)(r->arena + iso_seg_off.off);
   r->d_iso.seg_idx = (const int32_t *)(r->arena + iso_seg_idx.off);
   r->d_iso.locus = (const int32_t *)(r->arena + iso_locus.off);
   r->d_iso.len = (const int32_t *)(r->arena + iso_len.off);
   // the isoforms in the segment basis (the exon-bin kernel's masks): once, here
   int rc_sb = sb::make_seg_basis(c, &r->dev, n.n_iso, r->arena + o_segbasis, sb::ctx_stream(c), &r->seg_basis);
   if (rc_sb == SBGPU_OK && hipStreamSynchronize(sb::ctx_stream(c)) != hipSuccess) rc_sb = api_fail(SBGPU_EHIP, "sbgpu_annotation_pin: iso_masks_kernel failed");
   if (rc_sb != SBGPU_OK) return drop(rc_sb);
   sb::ctx_set_resident_annotation(c, r);
   return SBGPU_OK;
}

int sbgpu_annotation_unpin(sbgpu_ctx_t *c)
{
   if (!c) return api_fail(SBGPU_EINVAL, "sbgpu_annotation_unpin: null context");
   sb::ctx_set_resident_annotation(c, nullptr);
   return SBGPU_OK;
}

int sbgpu_annotation_unpin_matching(sbgpu_ctx_t *c, const sbgpu_annotation_t *an, int32_t *released)
{
   if (!c || !an) return api_fail(SBGPU_EINVAL, "sbgpu_annotation_unpin_matching: null argument");
   const sb::ResidentAnnotation *res = sb::ctx_resident_annotation(c);
   const bool mine = res && res->same_arrays(an);
   if (mine) sb::ctx_set_resident_annotation(c, nullptr);
   if (released) *released = mine ? 1 : 0;
   return SBGPU_OK;
}

} // extern "C"
