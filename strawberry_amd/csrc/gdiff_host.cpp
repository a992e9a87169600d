// strawberry_amd/csrc/gdiff_host.cpp -- sbgpu_em_gdiff_shapes_host, sbgpu_em_gdiff_expand_host, sbgpu_em_gdiff_stat_host
// (include/sbgpu.h): the differential isoform usage between two groups of replicate samples on the host, in three calls around
// the caller's solve and fits of the sub-batch (the library has no CPU EM).  The one CPU statement of what csrc/gdiff_device.h
// computes: every decision is a function of gdiff_rules.h, which the kernels call too.  No kernels and no HIP here: a plain
// C++ compiler takes this file (the library's error slot, sb::api_fail, is declared below instead of through api_internal.h).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "gdiff_rules.h"
#include "stage_host.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (sbgpu_api.hip) records sbgpu_last_error(), returns code
}
using sb::api_fail;

namespace {

int check_groups(const std::string &who, int32_t n_a, int32_t n_b)
{
   if (n_a < 1 || n_b < 1) return api_fail(SBGPU_EINVAL, who + ": a group without samples (n_a and n_b are at least 1)");
   if ((int64_t)n_a + n_b > sb::kGdiffMaxSamples) return api_fail(SBGPU_EINVAL, who + ": more than 16 samples");
   return SBGPU_OK;
}

// the offsets of the S samples: begin at 0, ascend, within the fit's limits
int check_offsets(const std::string &who, int64_t nl, int S, const int64_t *const *row_off, const int64_t *iso_off)
{
   if (nl < 0 || !iso_off || !row_off) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
   for (int s = 0; s < S; ++s)
      if (!row_off[s]) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
   if (iso_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
   for (int s = 0; s < S; ++s)
      if (row_off[s][0] != 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t niso = iso_off[l + 1] - iso_off[l];
      if (niso < 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: row_off / iso_off do not ascend");
      if (niso > 32 * (int64_t)sb::kStageMaxWords) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 4096 isoforms");
      for (int s = 0; s < S; ++s) {
         const int64_t nb = row_off[s][l + 1] - row_off[s][l];
         if (nb < 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: row_off / iso_off do not ascend");
         if (nb > sb::kStageMaxBins) return api_fail(SBGPU_ESHAPE, who + ": a locus of more than 5632 bins");
      }
   }
   return SBGPU_OK;
}

// the S batches describe one annotation; `weights`: f_off, count and F are read too.  *row_off: [S] their row offsets
int check_batches(const std::string &who, int32_t n_a, int32_t n_b, const sbgpu_batch_t *const *x, bool weights, std::vector<const int64_t *> *row_off)
{
   if (const int rc = check_groups(who, n_a, n_b); rc != SBGPU_OK) return rc;
   const int S = n_a + n_b;
   if (!x) return api_fail(SBGPU_EINVAL, who + ": null argument");
   row_off->assign((size_t)S, nullptr);
   for (int s = 0; s < S; ++s) {
      if (!x[s]) return api_fail(SBGPU_EINVAL, who + ": null argument");
      if (x[s]->n_loci != x[0]->n_loci) return api_fail(SBGPU_EINVAL, who + ": the batches differ in n_loci");
      (*row_off)[(size_t)s] = x[s]->row_off;
   }
   const int64_t nl = x[0]->n_loci;
   if (const int rc = check_offsets(who, nl, S, row_off->data(), x[0]->iso_off); rc != SBGPU_OK) return rc;
   for (int s = 0; s < S; ++s) {
      const sbgpu_batch_t *b = x[s];
      if (!b->iso_off || !std::equal(x[0]->iso_off, x[0]->iso_off + nl + 1, b->iso_off))
         return api_fail(SBGPU_EINVAL, who + ": the batches differ in iso_off: they are not over one annotation");
      if (b->row_off[nl] && !b->count) return api_fail(SBGPU_EINVAL, who + ": null count or F");
      for (int64_t i = 0; i < b->row_off[nl]; ++i)
         if (b->count[i] < 0) return api_fail(SBGPU_EINVAL, who + ": a negative count");
      if (!weights) continue;
      if (!b->f_off) return api_fail(SBGPU_EINVAL, who + ": bad n_loci or null offset array");
      if (b->f_off[0] != 0) return api_fail(SBGPU_EINVAL, who + ": malformed offsets: the arrays must begin at 0");
      for (int64_t l = 0; l < nl; ++l)
         if (b->f_off[l + 1] - b->f_off[l] != (b->row_off[l + 1] - b->row_off[l]) * (b->iso_off[l + 1] - b->iso_off[l]))
            return api_fail(SBGPU_EINVAL, who + ": malformed offsets: f_off[l + 1] - f_off[l] is not rows x isoforms");
      if (b->f_off[nl] && !b->F) return api_fail(SBGPU_EINVAL, who + ": null count or F");
   }
   return SBGPU_OK;
}

template <class T>
void fill(T *out, const std::vector<T> &v)
{
   if (out) std::copy(v.begin(), v.end(), out);
}
template <class T>
void put(T *out, int64_t i, T v)
{
   if (out) out[i] = v;
}

void clear_device(sbgpu_em_gdiff_t *out)
{
   out->d_theta_sample = out->d_theta_group = out->d_theta_all = out->d_usage_sample = out->d_usage_group = out->d_usage_all = out->d_delta_usage = nullptr;
   out->d_lr_between = out->d_lr_within = out->d_loglik_own = out->d_loglik_group = out->d_loglik_all = nullptr;
   out->d_n_frag = out->d_lost_shift = nullptr;
   out->d_dof_between = out->d_dof_within = out->d_p_a = out->d_p_b = out->d_gdiff_status = out->d_top_iso = nullptr;
   out->d_status_sample = out->d_iters_sample = out->d_status_group = out->d_iters_group = out->d_status_all = out->d_iters_all = nullptr;
}

} // namespace

extern "C" int sbgpu_em_gdiff_shapes_host(int64_t n_loci, int32_t n_a, int32_t n_b, const int64_t *const *row_off, const int64_t *iso_off,
                                          const int32_t *const *keep, int64_t sizes[4], int32_t *gdiff_status, int32_t *sub_locus, int32_t *sub_kind,
                                          int32_t *sub_sample, int64_t *sub_row_off, int64_t *sub_iso_off, int64_t *sub_f_off)
{
   const std::string who = "sbgpu_em_gdiff_shapes_host";
   if (const int rc = check_groups(who, n_a, n_b); rc != SBGPU_OK) return rc;
   if (!row_off || !iso_off || !sizes) return api_fail(SBGPU_EINVAL, who + ": null argument");
   if (const int rc = check_offsets(who, n_loci, n_a + n_b, row_off, iso_off); rc != SBGPU_OK) return rc;
   sb::GdiffShapes sh;
   sb::gdiff_shapes(n_loci, n_a, n_b, row_off, iso_off, keep, &sh);
   sizes[0] = sh.n_sub(), sizes[1] = sh.sub_row_off.back(), sizes[2] = sh.sub_iso_off.back(), sizes[3] = sh.sub_f_off.back();
   fill(gdiff_status, sh.status), fill(sub_locus, sh.sub_locus), fill(sub_kind, sh.sub_kind), fill(sub_sample, sh.sub_sample);
   fill(sub_row_off, sh.sub_row_off), fill(sub_iso_off, sh.sub_iso_off), fill(sub_f_off, sh.sub_f_off);
   return SBGPU_OK;
}

extern "C" int sbgpu_em_gdiff_expand_host(int32_t n_a, int32_t n_b, const sbgpu_batch_t *const *batches, const int32_t *const *keep,
                                          int32_t *sub_count, double *sub_F)
{
   const std::string who = "sbgpu_em_gdiff_expand_host";
   std::vector<const int64_t *> row_off;
   if (const int rc = check_batches(who, n_a, n_b, batches, true, &row_off); rc != SBGPU_OK) return rc;
   const int S = n_a + n_b;
   const int64_t nl = batches[0]->n_loci;
   const int64_t *iso_off = batches[0]->iso_off;
   sb::GdiffShapes sh;
   sb::gdiff_shapes(nl, n_a, n_b, row_off.data(), iso_off, keep, &sh);
   if ((sh.sub_row_off.back() && !sub_count) || (sh.sub_f_off.back() && !sub_F)) return api_fail(SBGPU_EINVAL, who + ": null sub_count or sub_F");
   std::vector<std::vector<double>> c((size_t)S);
   std::vector<double> alpha;
   for (int64_t l = 0; l < nl; ++l) {
      if (sh.first_sub[(size_t)l] < 0) continue;
      const int64_t *slot = sh.slot_sub.data() + (size_t)l * (size_t)sh.slots();
      const int niso = (int)(iso_off[l + 1] - iso_off[l]);
      const int32_t *kc = sh.kept_col.data() + sh.kept_off[(size_t)l];
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      // ---- the own copies, and rule 3's column sums over the rows that are live on the kept weights
      for (int s = 0; s < S; ++s) {
         const sbgpu_batch_t *x = batches[s];
         const int64_t nb = x->row_off[l + 1] - x->row_off[l], q = slot[s];
         if (q < 0) continue;
         const double *Fl = x->F + x->f_off[l];
         double *o = sub_F + sh.sub_f_off[(size_t)q];
         std::copy(x->count + x->row_off[l], x->count + x->row_off[l + 1], sub_count + sh.sub_row_off[(size_t)q]);
         c[(size_t)s].assign((size_t)K, 0.0);
         for (int64_t b = 0; b < nb; ++b) {
            for (int k = 0; k < K; ++k) o[b * K + k] = Fl[b * niso + kc[k]];
            if (!sb::asg_row_live(o + b * K, K)) continue;
            for (int k = 0; k < K; ++k) c[(size_t)s][(size_t)k] += o[b * K + k];
         }
      }
      // ---- the pools: group A, group B (where they have a sub-problem), ALL; the members' rows in sample order, scaled
      for (int pool = 0; pool < 3; ++pool) {
         if (pool < 2 && !sh.group_has_sub(l, pool)) continue;
         const int s0 = pool == 1 ? n_a : 0, s1 = pool == 0 ? n_a : S;
         const int64_t q = slot[S + pool];
         int members = 0;
         for (int s = s0; s < s1; ++s) members += slot[s] >= 0;
         int64_t at = 0;
         for (int s = s0; s < s1; ++s) {
            if (slot[s] < 0) continue;
            const sbgpu_batch_t *x = batches[s];
            const int64_t nb = x->row_off[l + 1] - x->row_off[l];
            alpha.resize((size_t)K);
            for (int k = 0; k < K; ++k) {
               double sum = 0.0;
               int n = 0;
               for (int t = s0; t < s1; ++t)
                  if (slot[t] >= 0) sum = sb::gdiff_add(sum, n, c[(size_t)t][(size_t)k]), ++n;
               alpha[(size_t)k] = sb::gdiff_alpha(sum, c[(size_t)s][(size_t)k], members);
            }
            const double *own = sub_F + sh.sub_f_off[(size_t)slot[s]];
            double *o = sub_F + sh.sub_f_off[(size_t)q] + at * K;
            std::copy(x->count + x->row_off[l], x->count + x->row_off[l + 1], sub_count + sh.sub_row_off[(size_t)q] + at);
            for (int64_t b = 0; b < nb; ++b)
               for (int k = 0; k < K; ++k) o[b * K + k] = own[b * K + k] * alpha[(size_t)k];
            at += nb;
         }
      }
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_em_gdiff_stat_host(int32_t n_a, int32_t n_b, const sbgpu_batch_t *const *batches, const int32_t *const *keep,
                                        const double *sub_theta, const int32_t *sub_status, const int32_t *sub_iters, const double *own_loglik,
                                        const int64_t *own_n_live, const int64_t *own_n_dropped, const int64_t *own_n_impossible,
                                        const double *group_loglik, const int64_t *group_n_dropped, const int64_t *group_n_impossible,
                                        const double *all_loglik, const int64_t *all_n_dropped, const int64_t *all_n_impossible, sbgpu_em_gdiff_t *out)
{
   const std::string who = "sbgpu_em_gdiff_stat_host";
   if (!out) return api_fail(SBGPU_EINVAL, who + ": null argument");
   std::vector<const int64_t *> row_off;
   if (const int rc = check_batches(who, n_a, n_b, batches, false, &row_off); rc != SBGPU_OK) return rc;
   const int S = n_a + n_b, slots = S + 3;
   const int64_t nl = batches[0]->n_loci;
   const int64_t *iso_off = batches[0]->iso_off;
   const int64_t n_iso = iso_off[nl];
   sb::GdiffShapes sh;
   sb::gdiff_shapes(nl, n_a, n_b, row_off.data(), iso_off, keep, &sh);
   if (sh.n_sub() && (!sub_theta || !sub_status || !sub_iters || !own_loglik || !own_n_live || !own_n_dropped || !own_n_impossible || !group_loglik ||
                      !group_n_dropped || !group_n_impossible || !all_loglik || !all_n_dropped || !all_n_impossible))
      return api_fail(SBGPU_EINVAL, who + ": a null array of the sub-batch's solve or fits");
   clear_device(out);
   const double one = 1.0;
   std::vector<double> sum((size_t)slots);
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t *slot = sh.slot_sub.data() + (size_t)l * (size_t)slots;
      const bool solved = sh.first_sub[(size_t)l] >= 0;
      const int K = (int)(sh.kept_off[(size_t)l + 1] - sh.kept_off[(size_t)l]);
      const int32_t *kc = sh.kept_col.data() + sh.kept_off[(size_t)l];
      int32_t status = sh.status[(size_t)l], top = -1;
      sb::GdiffLocus o{0.0, 0.0, 0, status, 0, 0};
      std::fill(sum.begin(), sum.end(), 0.0);
      long long n_frag[sb::kGdiffMaxSamples] = {};
      if (solved) {
         sb::GdiffAcc acc;
         sb::gdiff_begin(&acc);
         long long lost_members[2] = {0, 0};
         for (int s = 0; s < S; ++s) {
            const int64_t q = slot[s];
            if (q < 0) continue;
            const int g = s >= n_a;
            const long long lost = own_n_dropped[q] + own_n_impossible[q];
            n_frag[s] = sb::gdiff_add_sample(&acc, sub_status[q], !sh.group_has_sub(l, g), own_loglik[q], group_loglik[q], all_loglik[q], own_n_live[q],
                                             own_n_impossible[q], lost, group_n_dropped[q] + group_n_impossible[q], all_n_dropped[q] + all_n_impossible[q]);
            lost_members[g] += lost;
         }
         for (int g = 0; g < 2; ++g)
            if (sh.group_has_sub(l, g)) {
               const int64_t q = slot[S + g];
               sb::gdiff_add_group(&acc, sub_status[q], own_n_dropped[q] + own_n_impossible[q], lost_members[g]);
            }
         const int64_t qa = slot[S + 2];
         o = sb::gdiff_finish(acc, K, sub_status[qa], own_n_dropped[qa] + own_n_impossible[qa]);
         status = o.status;
         if (status == SBGPU_DIFF_OK) {
            for (int x = 0; x < slots; ++x)
               if (slot[x] >= 0) sum[(size_t)x] = sb::diff_sum(sub_theta + sh.sub_iso_off[(size_t)slot[x]], K);
            top = sb::diff_top(sub_theta + sh.sub_iso_off[(size_t)slot[S]], sum[(size_t)S], sub_theta + sh.sub_iso_off[(size_t)slot[S + 1]], sum[(size_t)S + 1], K);
         }
      }
      // a SOLE locus: the kept isoform has all of the usage of a sample that placed a fragment (`sum` holds the placed flags)
      if (status == SBGPU_DIFF_SOLE) {
         for (int s = 0; s < S; ++s) {
            const sbgpu_batch_t *x = batches[s];
            for (int64_t b = x->row_off[l]; b < x->row_off[l + 1]; ++b)
               if (x->count[b] > 0) sum[(size_t)s] = 1.0;
            if (sum[(size_t)s] > sum[(size_t)(S + (s >= n_a))]) sum[(size_t)(S + (s >= n_a))] = sum[(size_t)s];
         }
         sum[(size_t)S + 2] = sum[(size_t)S] > sum[(size_t)S + 1] ? sum[(size_t)S] : sum[(size_t)S + 1];
         top = sb::diff_top(&one, sum[(size_t)S], &one, sum[(size_t)S + 1], 1);
      }
      const bool ok = status == SBGPU_DIFF_OK;
      put(out->lr_between, l, o.lr_between), put(out->lr_within, l, o.lr_within), put(out->lost_shift, l, (int64_t)o.lost_shift);
      put(out->dof_between, l, o.dof_between), put(out->dof_within, l, o.dof_within);
      put(out->p_a, l, sh.p_a[(size_t)l]), put(out->p_b, l, sh.p_b[(size_t)l]);
      put(out->gdiff_status, l, status), put(out->top_iso, l, top >= 0 ? kc[top] : -1);
      for (int s = 0; s < S; ++s) {
         const int64_t q = slot[s], at = (int64_t)s * nl + l;
         const bool on = ok && q >= 0;
         put(out->loglik_own, at, on ? own_loglik[q] : 0.0);
         put(out->loglik_group, at, on ? (sh.group_has_sub(l, s >= n_a) ? group_loglik[q] : own_loglik[q]) : 0.0);
         put(out->loglik_all, at, on ? all_loglik[q] : 0.0);
         put(out->n_frag, at, (int64_t)(on ? n_frag[s] : 0));
         put(out->status_sample, at, q >= 0 ? sub_status[q] : -1), put(out->iters_sample, at, q >= 0 ? sub_iters[q] : -1);
      }
      for (int g = 0; g < 2; ++g) {
         const int64_t q = slot[S + g];
         put(out->status_group, (int64_t)g * nl + l, q >= 0 ? sub_status[q] : -1), put(out->iters_group, (int64_t)g * nl + l, q >= 0 ? sub_iters[q] : -1);
      }
      put(out->status_all, l, slot[S + 2] >= 0 ? sub_status[slot[S + 2]] : -1), put(out->iters_all, l, slot[S + 2] >= 0 ? sub_iters[slot[S + 2]] : -1);
      for (int64_t i = iso_off[l]; i < iso_off[l + 1]; ++i) {
         const int r = sh.rank[(size_t)i];
         double us_g[2] = {0.0, 0.0};
         for (int x = 0; x < slots; ++x) {
            double th = 0.0, us = 0.0;
            if (r >= 0 && ok && slot[x] >= 0) th = sub_theta[sh.sub_iso_off[(size_t)slot[x]] + r], us = sb::diff_usage(th, sum[(size_t)x]);
            if (r >= 0 && status == SBGPU_DIFF_SOLE) us = sb::diff_usage(one, sum[(size_t)x]);
            if (x < S) put(out->theta_sample, (int64_t)x * n_iso + i, th), put(out->usage_sample, (int64_t)x * n_iso + i, us);
            else if (x < S + 2) put(out->theta_group, (int64_t)(x - S) * n_iso + i, th), put(out->usage_group, (int64_t)(x - S) * n_iso + i, us), us_g[x - S] = us;
            else put(out->theta_all, i, th), put(out->usage_all, i, us);
         }
         put(out->delta_usage, i, us_g[1] - us_g[0]);
      }
   }
   return SBGPU_OK;
}
