// strawberry_amd/csrc/merge_host.cpp -- sbgpu_bins_merge_shapes_host, sbgpu_bins_merge_fill_host (include/sbgpu.h): two samples'
// bin tables merged by key, on the host.  The one CPU statement of what csrc/merge_device.h computes: every decision is a
// function of merge_rules.h, which the kernels call too.  The match itself is a sort of each sample's keys per locus and a
// binary search -- no hash, so that the deep kernel's table is checked against something that has none.  No kernels and no HIP
// here: a plain C++ compiler takes this file (the library's error slot, sb::api_fail, is declared below instead of through
// api_internal.h).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sbgpu.h"
#include "merge_rules.h"

namespace sb {
int api_fail(int code, const std::string &msg); // (sbgpu_api.hip) records sbgpu_last_error(), returns code
}
using sb::api_fail;

namespace {

// the match of every locus: b_of_a [n_bins_a], b_only [n_bins_b], n_only [n_loci] (merge_rules.h)
struct Match {
   std::vector<int32_t> b_of_a, b_only, n_only;
   std::vector<int64_t> row_off_u, f_off_u;
};

// one sample's bins of a locus in ascending key order -> false on two equal keys
bool sorted_bins(const uint32_t *key, int64_t nb, int kw, std::vector<int32_t> *order)
{
   order->resize((size_t)nb);
   for (int64_t i = 0; i < nb; ++i) (*order)[(size_t)i] = (int32_t)i;
   std::sort(order->begin(), order->end(),
             [&](int32_t x, int32_t y) { return std::lexicographical_compare(key + (int64_t)x * kw, key + (int64_t)(x + 1) * kw, key + (int64_t)y * kw, key + (int64_t)(y + 1) * kw); });
   for (int64_t i = 1; i < nb; ++i)
      if (sb::merge_key_equal(key + (int64_t)(*order)[(size_t)i - 1] * kw, key + (int64_t)(*order)[(size_t)i] * kw, kw)) return false;
   return true;
}

int match_host(const std::string &who, const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, Match *m)
{
   const char *why = nullptr;
   if (const int rc = sb::merge_check_shapes(a, b, &why); rc != 0) return api_fail(rc, who + ": " + why);
   const int64_t nl = a->n_loci;
   const int kw = a->key_words;
   m->b_of_a.assign((size_t)a->row_off[nl] + 1, -1), m->b_only.assign((size_t)b->row_off[nl] + 1, -1), m->n_only.assign((size_t)nl + 1, 0);
   std::vector<int32_t> oa, ob;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t a0 = a->row_off[l], b0 = b->row_off[l], na = a->row_off[l + 1] - a0, nb = b->row_off[l + 1] - b0;
      const uint32_t *ka = a->key + a0 * kw, *kb = b->key + b0 * kw;
      if (!sorted_bins(ka, na, kw, &oa) || !sorted_bins(kb, nb, kw, &ob))
         return api_fail(SBGPU_EINVAL, who + ": a duplicate bin key in locus " + std::to_string(l));
      int32_t n_only = 0;
      for (int64_t i = 0; i < nb; ++i) {
         const uint32_t *k = kb + i * kw;
         const auto it = std::lower_bound(oa.begin(), oa.end(), k, [&](int32_t x, const uint32_t *y) {
            return std::lexicographical_compare(ka + (int64_t)x * kw, ka + (int64_t)(x + 1) * kw, y, y + kw);
         });
         if (it != oa.end() && sb::merge_key_equal(ka + (int64_t)*it * kw, k, kw)) m->b_of_a[(size_t)(a0 + *it)] = (int32_t)i;
         else m->b_only[(size_t)(b0 + n_only++)] = (int32_t)i;
      }
      m->n_only[(size_t)l] = n_only;
   }
   const int64_t deep = sb::merge_offsets(nl, a->row_off, a->iso_off, m->n_only.data(), &m->row_off_u, &m->f_off_u);
   if (deep >= 0) return api_fail(SBGPU_ESHAPE, who + ": the union of locus " + std::to_string(deep) + " has more than 5632 bins");
   if (m->row_off_u[(size_t)nl] > INT32_MAX) return api_fail(SBGPU_ESHAPE, who + ": more than 2^31 - 1 bins in the union");
   return SBGPU_OK;
}

} // namespace

extern "C" int sbgpu_bins_merge_shapes_host(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, int64_t sizes[2], int64_t *row_off_u,
                                            int64_t *f_off_u, int32_t *row_a, int32_t *row_b)
{
   const std::string who = "sbgpu_bins_merge_shapes_host";
   if (!sizes) return api_fail(SBGPU_EINVAL, who + ": null argument");
   Match m;
   if (const int rc = match_host(who, a, b, &m); rc != SBGPU_OK) return rc;
   const int64_t nl = a->n_loci;
   sizes[0] = m.row_off_u[(size_t)nl], sizes[1] = m.f_off_u[(size_t)nl];
   if (row_off_u) std::copy(m.row_off_u.begin(), m.row_off_u.end(), row_off_u);
   if (f_off_u) std::copy(m.f_off_u.begin(), m.f_off_u.end(), f_off_u);
   if (!row_a && !row_b) return SBGPU_OK;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t a0 = a->row_off[l], b0 = b->row_off[l], na = a->row_off[l + 1] - a0, u0 = m.row_off_u[(size_t)l];
      for (int64_t u = 0; u < m.row_off_u[(size_t)l + 1] - u0; ++u) {
         int32_t ra, rb;
         sb::merge_row(u, na, m.b_of_a.data() + a0, m.b_only.data() + b0, &ra, &rb);
         if (row_a) row_a[u0 + u] = ra < 0 ? -1 : (int32_t)(a0 + ra);
         if (row_b) row_b[u0 + u] = rb < 0 ? -1 : (int32_t)(b0 + rb);
      }
   }
   return SBGPU_OK;
}

extern "C" int sbgpu_bins_merge_fill_host(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, int32_t *count_a, int32_t *count_b,
                                          double *F_a, double *F_b)
{
   const std::string who = "sbgpu_bins_merge_fill_host";
   Match m;
   if (const int rc = match_host(who, a, b, &m); rc != SBGPU_OK) return rc;
   const int64_t nl = a->n_loci;
   const sbgpu_merge_sample_t *side[2] = {a, b};
   int32_t *count[2] = {count_a, count_b};
   double *F[2] = {F_a, F_b};
   std::vector<int64_t> f_off[2] = {sb::merge_f_off(nl, a->row_off, a->iso_off), sb::merge_f_off(nl, b->row_off, a->iso_off)};
   for (int s = 0; s < 2; ++s) {
      if (count[s] && side[s]->row_off[nl] && !side[s]->count) return api_fail(SBGPU_EINVAL, who + ": null count");
      if (F[s] && f_off[s][(size_t)nl] && !side[s]->F) return api_fail(SBGPU_EINVAL, who + ": null F");
      if (F[s] && f_off[1 - s][(size_t)nl] && !side[s]->X && !side[1 - s]->F) return api_fail(SBGPU_EINVAL, who + ": null F");
   }
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t a0 = a->row_off[l], b0 = b->row_off[l], na = a->row_off[l + 1] - a0, u0 = m.row_off_u[(size_t)l];
      const int niso = (int)(a->iso_off[l + 1] - a->iso_off[l]);
      for (int64_t u = 0; u < m.row_off_u[(size_t)l + 1] - u0; ++u) {
         int32_t r[2];
         sb::merge_row(u, na, m.b_of_a.data() + a0, m.b_only.data() + b0, &r[0], &r[1]);
         for (int s = 0; s < 2; ++s) {
            const sbgpu_merge_sample_t *own = side[s], *other = side[1 - s];
            if (count[s]) count[s][u0 + u] = r[s] >= 0 ? own->count[own->row_off[l] + r[s]] : 0;
            if (!F[s]) continue;
            const double *Fo = own->F ? own->F + f_off[s][(size_t)l] : nullptr, *Xo = own->X ? own->X + f_off[1 - s][(size_t)l] : nullptr;
            const double *Ft = other->F ? other->F + f_off[1 - s][(size_t)l] : nullptr;
            double *o = F[s] + m.f_off_u[(size_t)l] + u * niso;
            for (int j = 0; j < niso; ++j) o[j] = sb::merge_weight(r[s], Fo, r[1 - s], Xo, Ft, niso, j);
         }
      }
   }
   return SBGPU_OK;
}
