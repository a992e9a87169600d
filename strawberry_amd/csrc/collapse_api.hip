// strawberry_amd/csrc/collapse_api.hip -- sbgpu_collapse_pairs_device (include/sbgpu.h): read pairs resident in
// HBM -> unique hits resident in HBM (HitCluster::collapseAndFilterHits + Contig(PairedHit),
// /root/reference/src/alignments.cpp:656-703, src/contig.cpp:216-267).  Kernels: collapse_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/sbgpu.h"
#include "front_common.h"
#include "collapse_device.h"
#include "collapse_flat.h"

using sb::api_fail;

struct sbgpu_uniq_dev {
   int device = 0;
   char *arena = nullptr; // the unique hits (sbgpu_hits_t layout) + their masses (sb::dev_take'n)
   size_t arena_cap = 0;
   int64_t n_loci = 0, n_hits = 0, n_feat = 0, n_filtered = 0, n_rejected = 0, total_mapped = 0;
   int32_t *d_hit_locus = nullptr;
   int64_t *d_feat_off = nullptr;
   uint8_t *d_feat_code = nullptr;
   uint32_t *d_feat_left = nullptr, *d_feat_right = nullptr;
   float *d_mass = nullptr;
   std::vector<int64_t> locus_hit_off; // host
   std::vector<double> cluster_mass;   // host
};

namespace {
// ---- the flat form (collapse_flat.h): every cluster of the call at once.  What the call decides is front_schedule.h's
// (collapse_sort_choice, the two layouts); the steps below issue it.
struct CollapseCall {
   sbgpu_ctx_t *const c;
   const int64_t n_loci;
   const sbgpu_pairs_t *const dp;
   const int64_t *const locus_pair_off;
   const hipStream_t s;
   sbgpu_uniq_dev *const U;
   const sb::FrontHooks hooks;
   const size_t n = (size_t)dp->n_pairs, n1 = n + 1, nl1 = (size_t)n_loci + 1;
   const unsigned locus_bits = sb::front_locus_bits(n_loci);
   size_t tmp_bytes = 0; // temporary storage of the library calls: the largest of them
   sb::CollapseScratchLayout L = {};
   sb::DevBlock w{s};
   sb::FlatCollapseArgs f = {};
   unsigned gp = 0, gw = 0;
   sb::CollapseSortChoice sort = {};
   int32_t flags = 0; // what the last read-back brings
   unsigned long long counts[2] = {0, 0};
   int64_t n_feat = 0;

   void *tmp() const { return w.p + L.tmp; }
   hipError_t scan_i64(const int32_t *in, size_t out, size_t count)
   {
      size_t tb = tmp_bytes;
      return rocprim::exclusive_scan(tmp(), tb, rocprim::make_transform_iterator(in, sb::I32AsI64()), w.at<int64_t>(out), (int64_t)0, count, rocprim::plus<int64_t>(), s);
   }

   // the library's temporary bytes, the scratch, what must start at zero, the kernels' arguments
   int lay_out()
   {
      auto larger = [this](size_t b) { tmp_bytes = std::max(tmp_bytes, b); };
      size_t b = 0;
      (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t *)nullptr, n, 0, 32, s);
      larger(b);
      (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, n, 0, 32 + locus_bits, s);
      larger(b);
      (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t *)nullptr, n, 0, 64, s);
      larger(b);
      (void)rocprim::exclusive_scan(nullptr, b, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull, nl1, rocprim::plus<unsigned long long>(), s);
      larger(b);
      (void)rocprim::inclusive_scan(nullptr, b, (const int32_t *)nullptr, (int32_t *)nullptr, n, rocprim::maximum<int32_t>(), s);
      larger(b);
      (void)rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator((const uint8_t *)nullptr, sb::U8AsI32()), (int32_t *)nullptr, n, rocprim::plus<int32_t>(), s);
      larger(b);
      (void)rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator((const int32_t *)nullptr, sb::I32AsI64()), (int64_t *)nullptr, (int64_t)0, n1, rocprim::plus<int64_t>(), s);
      larger(b);
      L = sb::collapse_scratch_layout((int64_t)n, n_loci, tmp_bytes);
      SB_FRONT_TRY(w.take(L.bytes));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.sum, 0, L.sums_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.gmass, 0, L.gmass_bytes, s));
      if (hooks.collapse_force_seq) // (as if every cluster had been marked)
         SB_FRONT_TRY(hipMemsetD32Async((hipDeviceptr_t)(w.p + L.clf), sb::kNeedSeqMass | sb::kNeedSeqSd, L.clf_words, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.counts, 0, L.counters_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.minl, 0xFF, L.cluster_words_bytes, s)); // (the clusters' leftmost left end starts at the top)
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.maxl, 0, L.cluster_words_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.ostat, 0, L.ostat_bytes, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.nfeat_tail, 0, 4, s));
      SB_FRONT_TRY(hipMemsetAsync(w.p + L.ishit_tail, 0, 4, s));
      SB_FRONT_TRY(hipMemcpyAsync(w.p + L.poff, locus_pair_off, nl1 * 8, hipMemcpyHostToDevice, s));
      sb::CollapseArgs &a = f.a;
      a.n_loci = n_loci;
      a.locus_pair_off = w.at<const int64_t>(L.poff);
      a.pair_mass = dp->pair_mass;
      a.left_off = dp->left_off, a.right_off = dp->right_off;
      a.left_code = dp->left_code, a.right_code = dp->right_code;
      a.left_left = dp->left_left, a.left_right = dp->left_right;
      a.right_left = dp->right_left, a.right_right = dp->right_right;
      a.cluster_mass = w.at<double>(L.cm);
      a.flags = w.at<int32_t>(L.flag);
      f.n_pairs = (int64_t)n;
      f.key_right = w.at<uint32_t>(L.kr);
      f.key_hi = w.at<unsigned long long>(L.khi);
      f.span_l = w.at<int32_t>(L.sl), f.span_r = w.at<int32_t>(L.sr);
      f.span_sum = w.at<unsigned long long>(L.sum);
      f.span_sq = w.at<unsigned long long>(L.sq);
      f.n_mates = w.at<int32_t>(L.nm);
      f.cl_flags = w.at<int32_t>(L.clf);
      f.mean = w.at<double>(L.mean), f.sd5 = w.at<double>(L.sd);
      f.perm1 = w.at<const int32_t>(L.perm1);
      f.key2 = w.at<unsigned long long>(L.key2);
      f.key2s = w.at<const unsigned long long>(L.key2s);
      f.order = w.at<const int32_t>(L.order);
      f.skip = w.at<uint8_t>(L.skip), f.head = w.at<uint8_t>(L.head);
      f.kept_pos = w.at<int32_t>(L.kept);
      f.last_kept = w.at<const int32_t>(L.last);
      f.nfeat = w.at<int32_t>(L.nfeat), f.is_hit = w.at<int32_t>(L.ishit);
      f.gid = w.at<const int32_t>(L.gid);
      f.hit_rank = w.at<const int64_t>(L.hrank), f.feat_base = w.at<const int64_t>(L.fbase);
      f.gmass = w.at<double>(L.gmass);
      f.locus_hit_off = w.at<int64_t>(L.hoff);
      f.counts = w.at<unsigned long long>(L.counts);
      f.cl_minl = w.at<uint32_t>(L.minl), f.cl_maxl = w.at<uint32_t>(L.maxl);
      f.cl_span = w.at<unsigned long long>(L.cspan), f.cl_base = w.at<const unsigned long long>(L.cbase);
      f.order_stats = w.at<unsigned long long>(L.ostat);
      f.cluster_of = w.at<int32_t>(L.clof);
      gp = (unsigned)((n + 255) / 256);
      gw = (unsigned)std::min<int64_t>(n_loci + 1, (int64_t)sb::ctx_cu_count(c) * 64);
      return SBGPU_OK;
   }

   // the pairs' keys; the clusters' ranges of left ends laid end to end.  What the one sort's key would be wide, the host must
   // know: one 24-byte read-back
   int keys_and_spans()
   {
      hipLaunchKernelGGL(sb::flat_keys_kernel, dim3(gp), dim3(256), 0, s, f);
      SB_FRONT_TRY(hipGetLastError());
      hipLaunchKernelGGL(sb::flat_cluster_spans_kernel, dim3((unsigned)((nl1 + 255) / 256)), dim3(256), 0, s, f);
      size_t tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::exclusive_scan(tmp(), tb, (const unsigned long long *)f.cl_span, w.at<unsigned long long>(L.cbase), 0ull, nl1, rocprim::plus<unsigned long long>(), s));
      unsigned long long x_total = 0, ostat[2] = {0, 0};
      SB_FRONT_TRY(hipMemcpyAsync(&x_total, w.p + L.x_total, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(ostat, w.p + L.ostat, 16, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      sort = sb::collapse_sort_choice(ostat[0], x_total, ostat[1], hooks.collapse_two_sorts);
      f.span_bits = (int)sort.span_bits;
      return SBGPU_OK;
   }

   // the order of std::sort on (left end, right end), ties in input order: one stable sort, or two (front_schedule.h)
   int sort_pairs()
   {
      size_t tb = tmp_bytes;
      if (sort.one_sort) {
         hipLaunchKernelGGL(sb::flat_rekey_kernel, dim3(gp), dim3(256), 0, s, f);
         SB_FRONT_TRY(rocprim::radix_sort_pairs(tmp(), tb, (const unsigned long long *)f.key2, w.at<unsigned long long>(L.key2s), rocprim::counting_iterator<int32_t>(0), w.at<int32_t>(L.order), n, 0, sort.end_bit, s));
         hipLaunchKernelGGL(sb::flat_cluster_of_kernel<false>, dim3(gp), dim3(256), 0, s, f);
      } else {
         SB_FRONT_TRY(rocprim::radix_sort_pairs(tmp(), tb, (const uint32_t *)f.key_right, w.at<uint32_t>(L.kr2), rocprim::counting_iterator<int32_t>(0), w.at<int32_t>(L.perm1), n, 0, 32, s));
         hipLaunchKernelGGL(sb::flat_gather_kernel, dim3(gp), dim3(256), 0, s, f);
         tb = tmp_bytes;
         SB_FRONT_TRY(rocprim::radix_sort_pairs(tmp(), tb, (const unsigned long long *)f.key2, w.at<unsigned long long>(L.key2s), f.perm1, w.at<int32_t>(L.order), n, 0, 32 + locus_bits, s));
         hipLaunchKernelGGL(sb::flat_cluster_of_kernel<true>, dim3(gp), dim3(256), 0, s, f);
      }
      SB_FRONT_TRY(hipGetLastError());
      return SBGPU_OK;
   }

   // the span filter from the integer moments; the clusters it marks (none, as a rule) get the running sum and their flags again
   int filter()
   {
      hipLaunchKernelGGL(sb::flat_flags_kernel<1>, dim3(gp), dim3(256), 0, s, f);
      hipLaunchKernelGGL(sb::flat_sd_kernel, dim3(gw), dim3(64), 0, s, f);
      hipLaunchKernelGGL(sb::flat_flags_kernel<2>, dim3(gp), dim3(256), 0, s, f);
      SB_FRONT_TRY(hipGetLastError());
      return SBGPU_OK;
   }

   // the groups of equal pairs: every kept pair's predecessor, the heads
   int heads()
   {
      size_t tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::inclusive_scan(tmp(), tb, (const int32_t *)f.kept_pos, w.at<int32_t>(L.last), n, rocprim::maximum<int32_t>(), s));
      hipLaunchKernelGGL(sb::flat_heads_kernel, dim3(sb::xcd_grid(gp)), dim3(256), 0, s, f);
      hipLaunchKernelGGL(sb::flat_heads_long_kernel, dim3(256), dim3(64), 0, s, f); // (returns at once unless a mate has more than 24 features)
      SB_FRONT_TRY(hipGetLastError());
      return SBGPU_OK;
   }

   // the groups' numbers, the hits' ranks, where their features begin
   int scans()
   {
      size_t tb = tmp_bytes;
      SB_FRONT_TRY(rocprim::inclusive_scan(tmp(), tb, rocprim::make_transform_iterator((const uint8_t *)f.head, sb::U8AsI32()), w.at<int32_t>(L.gid), n, rocprim::plus<int32_t>(), s));
      SB_FRONT_TRY(scan_i64(f.is_hit, L.hrank, n1));
      SB_FRONT_TRY(scan_i64(f.nfeat, L.fbase, n1));
      return SBGPU_OK;
   }

   int masses()
   {
      hipLaunchKernelGGL(sb::flat_mass_any_order_kernel, dim3(sb::xcd_grid((int64_t)((std::max(n, nl1) + 255) / 256))), dim3(256), 0, s, f);
      hipLaunchKernelGGL(sb::flat_mass_kernel, dim3(gw), dim3(64), 0, s, f); // the clusters with a mass that is no multiple of 2^-20
      SB_FRONT_TRY(hipGetLastError());
      return SBGPU_OK;
   }

   // ---- what the host needs: the flags, the totals, the clusters' first hits and masses
   int read_back()
   {
      SB_FRONT_TRY(hipMemcpyAsync(&flags, w.p + L.flag, 4, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(counts, w.p + L.counts, 16, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(&n_feat, w.p + L.n_feat, 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(U->locus_hit_off.data(), w.p + L.hoff, nl1 * 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipMemcpyAsync(U->cluster_mass.data(), w.p + L.cm, (size_t)n_loci * 8, hipMemcpyDeviceToHost, s));
      SB_FRONT_TRY(hipStreamSynchronize(s));
      if (flags) {
         if (flags & sb::kCollapseNoMates) return api_fail(SBGPU_EINVAL, "sbgpu_collapse_pairs_device: a pair without mates");
         return api_fail(SBGPU_EUNSUPPORTED, "sbgpu_collapse_pairs_device: not covered by the device form: a mate has more than 512 features; use sbgpu_collapse_pairs_host");
      }
      U->n_filtered = (int64_t)counts[0];
      U->n_rejected = (int64_t)counts[1];
      for (int64_t l = 0; l < n_loci; ++l) U->total_mapped += (int64_t)(int)U->cluster_mass[(size_t)l]; // src/alignments.cpp:1372
      U->n_hits = U->locus_hit_off[(size_t)n_loci];
      U->n_feat = n_feat;
      return SBGPU_OK;
   }

   // ---- the unique hits' own arena, filled; the scratch goes back to the pool behind the last synchronisation
   int fill()
   {
      const sb::CollapseHitsLayout H = sb::collapse_hits_layout(U->n_hits, U->n_feat);
      SB_FRONT_TRY(sb::dev_take(H.bytes, &U->arena, &U->arena_cap));
      U->d_feat_off = (int64_t *)(U->arena + H.off);
      U->d_hit_locus = (int32_t *)(U->arena + H.loc);
      U->d_mass = (float *)(U->arena + H.mass);
      U->d_feat_left = (uint32_t *)(U->arena + H.left);
      U->d_feat_right = (uint32_t *)(U->arena + H.right);
      U->d_feat_code = (uint8_t *)(U->arena + H.code);
      SB_FRONT_TRY(hipMemcpyAsync(U->d_feat_off + U->n_hits, &U->n_feat, 8, hipMemcpyHostToDevice, s));
      sb::CollapseArgs &a = f.a;
      a.hit_locus = U->d_hit_locus;
      a.feat_off = U->d_feat_off;
      a.feat_code = U->d_feat_code;
      a.feat_left = U->d_feat_left;
      a.feat_right = U->d_feat_right;
      a.hit_mass = U->d_mass;
      hipLaunchKernelGGL(sb::flat_fill_kernel, dim3(sb::xcd_grid(gp)), dim3(256), 0, s, f);
      hipLaunchKernelGGL(sb::flat_fill_long_kernel, dim3(256), dim3(64), 0, s, f);
      SB_FRONT_TRY(hipGetLastError());
      SB_FRONT_TRY(hipStreamSynchronize(s));
      return SBGPU_OK;
   }

   int run()
   {
      SB_FRONT_TRY(hipSetDevice(U->device));
      SB_FRONT_RC(lay_out());
      SB_FRONT_RC(keys_and_spans());
      SB_FRONT_RC(sort_pairs());
      SB_FRONT_RC(filter());
      SB_FRONT_RC(heads());
      SB_FRONT_RC(scans());
      SB_FRONT_RC(masses());
      SB_FRONT_RC(read_back());
      return fill();
   }
};
} // namespace

static int collapse_flat(sbgpu_ctx_t *c, int64_t n_loci, const sbgpu_pairs_t *dp, const int64_t *locus_pair_off, hipStream_t s, sbgpu_uniq_dev *U)
{
   if (dp->n_pairs >= ((int64_t)1 << 31) - 2) return api_fail(SBGPU_EUNSUPPORTED, "sbgpu_collapse_pairs_device: more than 2^31 read pairs in one call; split the call or use sbgpu_collapse_pairs_host");
   return CollapseCall{c, n_loci, dp, locus_pair_off, s, U, sb::front_hooks_from_env()}.run();
}


extern "C" {

void sbgpu_uniq_dev_destroy(sbgpu_uniq_dev_t *u)
{
   if (!u) return;
   sb::dev_give(u->arena, u->arena_cap); // (waits for the device the arena lives on, as hipFree did)
   delete u;
}

int sbgpu_collapse_pairs_device(sbgpu_ctx_t *c, int64_t n_loci, const sbgpu_pairs_t *dp, const int64_t *locus_pair_off,
                                void *stream, sbgpu_uniq_dev_t **out)
{
   if (!c || !dp || !out || !locus_pair_off || n_loci < 0) return api_fail(SBGPU_EINVAL, "sbgpu_collapse_pairs_device: bad argument");
   *out = nullptr;
   const int64_t np = dp->n_pairs;
   if (np < 0 || locus_pair_off[0] != 0 || locus_pair_off[n_loci] != np)
      return api_fail(SBGPU_EINVAL, "sbgpu_collapse_pairs_device: locus_pair_off does not cover the pairs");
   if (np && (!dp->pair_mass || !dp->left_off || !dp->right_off)) return api_fail(SBGPU_EINVAL, "sbgpu_collapse_pairs_device: null array");
   for (int64_t l = 0; l < n_loci; ++l)
      if (locus_pair_off[l + 1] < locus_pair_off[l]) return api_fail(SBGPU_EINVAL, "sbgpu_collapse_pairs_device: locus_pair_off must ascend");
   hipStream_t s = (hipStream_t)stream;
   sb::UniqDevHandle U(new (std::nothrow) sbgpu_uniq_dev());
   if (!U) return api_fail(SBGPU_ENOMEM, "sbgpu_collapse_pairs_device: out of host memory");
   U->device = sb::ctx_device(c);
   U->n_loci = n_loci;
   U->locus_hit_off.assign((size_t)n_loci + 1, 0);
   U->cluster_mass.assign((size_t)n_loci, 0.0);
   // every cluster of the call at once (collapse_flat.h)
   if (np != 0 && n_loci != 0) SB_FRONT_RC(collapse_flat(c, n_loci, dp, locus_pair_off, s, U.get()));
   *out = U.release();
   return SBGPU_OK;
}

int sbgpu_uniq_dev_info(const sbgpu_uniq_dev_t *u, int64_t info[8])
{
   if (!u || !info) return api_fail(SBGPU_EINVAL, "sbgpu_uniq_dev_info: null argument");
   info[0] = u->n_hits;
   info[1] = u->n_feat;
   info[2] = u->n_filtered;
   info[3] = u->n_rejected;
   info[4] = u->total_mapped;
   info[5] = u->n_loci;
   info[6] = info[7] = 0;
   return SBGPU_OK;
}

int sbgpu_uniq_dev_hits(const sbgpu_uniq_dev_t *u, sbgpu_hits_t *d_hits, const float **d_hit_mass, const int64_t **locus_hit_off)
{
   if (!u || !d_hits) return api_fail(SBGPU_EINVAL, "sbgpu_uniq_dev_hits: null argument");
   d_hits->n_hits = u->n_hits;
   d_hits->hit_locus = u->d_hit_locus;
   d_hits->feat_off = u->d_feat_off;
   d_hits->feat_code = u->d_feat_code;
   d_hits->feat_left = u->d_feat_left;
   d_hits->feat_right = u->d_feat_right;
   if (d_hit_mass) *d_hit_mass = u->d_mass;
   if (locus_hit_off) *locus_hit_off = u->locus_hit_off.data();
   return SBGPU_OK;
}

int sbgpu_uniq_dev_export(const sbgpu_uniq_dev_t *u, int32_t *hit_locus, int64_t *feat_off, uint8_t *feat_code, uint32_t *feat_left,
                          uint32_t *feat_right, float *hit_mass, double *cluster_mass)
{
   if (!u) return api_fail(SBGPU_EINVAL, "sbgpu_uniq_dev_export: null argument");
   hipError_t e = hipSetDevice(u->device);
   auto get = [&](void *dst, const void *src, size_t bytes) {
      if (e == hipSuccess && dst && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
   };
   if (u->arena) {
      get(hit_locus, u->d_hit_locus, (size_t)u->n_hits * 4);
      get(feat_off, u->d_feat_off, (size_t)(u->n_hits + 1) * 8);
      get(feat_code, u->d_feat_code, (size_t)u->n_feat);
      get(feat_left, u->d_feat_left, (size_t)u->n_feat * 4);
      get(feat_right, u->d_feat_right, (size_t)u->n_feat * 4);
      get(hit_mass, u->d_mass, (size_t)u->n_hits * 4);
   } else if (feat_off) {
      feat_off[0] = 0;
   }
   if (cluster_mass && !u->cluster_mass.empty()) std::memcpy(cluster_mass, u->cluster_mass.data(), u->cluster_mass.size() * 8);
   if (e != hipSuccess) return api_fail(SBGPU_EHIP, std::string("sbgpu_uniq_dev_export: ") + hipGetErrorString(e));
   return SBGPU_OK;
}

} // extern "C"
