// strawberry_amd/csrc/merge_rules.h -- the decisions of the bin-table merge (include/sbgpu.h: sbgpu_bins_merge_*), as
// functions the host form (merge_host.cpp) and the kernels (merge_device.h) both call, so that the two forms cannot drift:
//   - when two bin keys are equal (merge_key_equal), and the hash the deep form files A's keys under (merge_key_hash),
//   - which form of the match a locus takes (merge_is_small) and how many lanes its group has (merge_group_lanes),
//   - the union's offsets from the per-locus B-only counts (merge_offsets: the launcher and the host form call this one),
//   - where a union row comes from in each sample (merge_row), and which array a merged weight is read from (merge_weight).
// What the match leaves, in both forms, is the pair of INVERSE maps the fill reads: b_of_a [n_bins_a] -- the locus-local B bin
// with A bin's key, or -1 -- and b_only [n_bins_b] -- the first n_only[l] entries of locus l: its B-only bins, locus-local, in
// B's order.  They say what "the A bin of every B bin, and its rank among the B-only ones" says, from the side the union's rows
// are numbered on.  Keys are unique inside a locus, so neither depends on the order anything was inserted in.
#pragma once

#include <stdint.h>

#include <vector>

#include "stage_host.h"

namespace sb {

constexpr int kMergeGroupMaxBins = 64;    // a group of lanes lies inside one wave64 and a lane holds one bin of each sample
constexpr int kMergeTableSlots = 16384;   // the deep form's LDS table: the power of two at or above 2 x kStageMaxBins (load <= 0.5 for any union the call accepts)
constexpr int kMergeRegWords = 4;         // key words a lane of the small form holds in registers; further words are compared from memory
static_assert(kMergeTableSlots >= 2 * kStageMaxBins && kMergeTableSlots / 2 < 2 * kStageMaxBins, "the table is the smallest power of two with load <= 0.5");

__host__ __device__ inline bool merge_key_equal(const uint32_t *x, const uint32_t *y, int key_words)
{
   for (int w = 0; w < key_words; ++w)
      if (x[w] != y[w]) return false;
   return true;
}

// FNV-1a over the key's words (a xor, then a product, per word: the order of the words matters), folded once
__host__ __device__ inline uint32_t merge_key_hash(const uint32_t *k, int key_words)
{
   uint32_t h = 0x811C9DC5u;
   for (int w = 0; w < key_words; ++w) h = (h ^ k[w]) * 0x01000193u;
   return h ^ (h >> 15);
}
__host__ __device__ inline int merge_slot(uint32_t hash) { return (int)(hash & (uint32_t)(kMergeTableSlots - 1)); }

// the small form serves a locus whose bins fit a group of lanes in BOTH samples
__host__ __device__ inline bool merge_is_small(int64_t nb_a, int64_t nb_b) { return nb_a <= kMergeGroupMaxBins && nb_b <= kMergeGroupMaxBins; }
__host__ __device__ inline int merge_group_lanes(int64_t nb_a, int64_t nb_b)
{
   const int64_t nb = nb_a > nb_b ? nb_a : nb_b;
   int p = 1;
   while (p < nb) p <<= 1;
   return p;
}

// Union row u (locus-local) of a locus with nb_a bins in A: *a, *b = the locus-local bin of each sample, or -1
__host__ __device__ inline void merge_row(int64_t u, int64_t nb_a, const int32_t *b_of_a_of_locus, const int32_t *b_only_of_locus, int32_t *a, int32_t *b)
{
   if (u < nb_a) *a = (int32_t)u, *b = b_of_a_of_locus[u];
   else *a = -1, *b = b_only_of_locus[u - nb_a];
}

// A merged weight of sample s: its own where it has the row, else the other sample's bin under s' law (X, of the other sample's
// shape; null: the other sample's own weights)
__host__ __device__ inline double merge_weight(int32_t own_row, const double *F_own_of_locus, int32_t other_row, const double *X_of_locus,
                                               const double *F_other_of_locus, int niso, int j)
{
   if (own_row >= 0) return F_own_of_locus[(int64_t)own_row * niso + j];
   return (X_of_locus ? X_of_locus : F_other_of_locus)[(int64_t)other_row * niso + j];
}

// The union's offsets: row_off_u, f_off_u [n_loci + 1] from A's offsets and the B-only counts.  -> the first locus whose union
// exceeds kStageMaxBins, or -1
inline int64_t merge_offsets(int64_t n_loci, const int64_t *row_off_a, const int64_t *iso_off, const int32_t *n_only, std::vector<int64_t> *row_off_u,
                             std::vector<int64_t> *f_off_u)
{
   row_off_u->assign((size_t)n_loci + 1, 0), f_off_u->assign((size_t)n_loci + 1, 0);
   int64_t too_deep = -1;
   for (int64_t l = 0; l < n_loci; ++l) {
      const int64_t nb = row_off_a[l + 1] - row_off_a[l] + n_only[l];
      if (nb > kStageMaxBins && too_deep < 0) too_deep = l;
      (*row_off_u)[(size_t)l + 1] = (*row_off_u)[(size_t)l] + nb;
      (*f_off_u)[(size_t)l + 1] = (*f_off_u)[(size_t)l] + nb * (iso_off[l + 1] - iso_off[l]);
   }
   return too_deep;
}

// One sample's f_off from its row_off and the shared iso_off
inline std::vector<int64_t> merge_f_off(int64_t n_loci, const int64_t *row_off, const int64_t *iso_off)
{
   std::vector<int64_t> f((size_t)n_loci + 1, 0);
   for (int64_t l = 0; l < n_loci; ++l) f[(size_t)l + 1] = f[(size_t)l] + (row_off[l + 1] - row_off[l]) * (iso_off[l + 1] - iso_off[l]);
   return f;
}

// The checks both forms make of the two samples' shapes -> 0, or the SBGPU_E* code with *why set
inline int merge_check_shapes(const sbgpu_merge_sample_t *a, const sbgpu_merge_sample_t *b, const char **why)
{
   if (!a || !b) return *why = "null argument", SBGPU_EINVAL;
   if (a->n_loci < 0 || !a->iso_off || !b->iso_off || !a->row_off || !b->row_off) return *why = "bad n_loci or null offset array", SBGPU_EINVAL;
   if (a->n_loci != b->n_loci) return *why = "the two samples differ in n_loci", SBGPU_EINVAL;
   if (a->key_words != b->key_words) return *why = "the two samples differ in key_words", SBGPU_EINVAL;
   if (a->key_words < 1) return *why = "key_words must be at least 1", SBGPU_EINVAL;
   const int64_t nl = a->n_loci;
   if (a->iso_off[0] != 0 || a->row_off[0] != 0 || b->row_off[0] != 0) return *why = "malformed offsets: the arrays must begin at 0", SBGPU_EINVAL;
   for (int64_t l = 0; l <= nl; ++l)
      if (a->iso_off[l] != b->iso_off[l]) return *why = "the two samples differ in iso_off: they are not over one annotation", SBGPU_EINVAL;
   for (int64_t l = 0; l < nl; ++l) {
      const int64_t na = a->row_off[l + 1] - a->row_off[l], nb = b->row_off[l + 1] - b->row_off[l], niso = a->iso_off[l + 1] - a->iso_off[l];
      if (na < 0 || nb < 0 || niso < 0) return *why = "malformed offsets: row_off / iso_off do not ascend", SBGPU_EINVAL;
      if (na > kStageMaxBins || nb > kStageMaxBins) return *why = "a locus of more than 5632 bins", SBGPU_ESHAPE;
      if (niso > 32 * (int64_t)kStageMaxWords) return *why = "a locus of more than 4096 isoforms", SBGPU_ESHAPE;
   }
   if (a->row_off[nl] > INT32_MAX || b->row_off[nl] > INT32_MAX) return *why = "more than 2^31 - 1 bins in a sample", SBGPU_ESHAPE;
   for (const sbgpu_merge_sample_t *x : {a, b})
      if (x->row_off[nl] && !x->key) return *why = "null key", SBGPU_EINVAL;
   return 0;
}

} // namespace sb
