// strawberry_amd/csrc/merge_device.h -- the kernels of the bin-table merge (include/sbgpu.h: sbgpu_bins_merge_device; DESIGN
// 3.29).  The match leaves what merge_rules.h names: b_of_a, b_only and the per-locus B-only count (-1: a duplicate key).
//
// merge_match_small_kernel: the many loci of a few dozen bins.  A locus whose bins fit 64 lanes in both samples takes a group of
// P = 2^ceil(log2 max(nb_A, nb_B)) lanes inside one wave64, and 256 / P loci share a workgroup.  LANE i HOLDS A's key i and B's
// key i (their first kMergeRegWords words in registers); A's keys, then B's, pass by as loads every lane of the group makes of
// the same address.  One pass gives the lane its B bin's A partner and its A bin's B partner, and -- against the keys before
// its own -- says whether its key occurred already.  The B-only rank is a ballot and a popcount under the group's mask.  No
// LDS, no barrier, no atomics; every output has one writer.
//
// merge_match_deep_kernel: a workgroup per locus.  A's keys go into an LDS table of kMergeTableSlots slots, open addressing with
// linear probing, inserted with atomicCAS; a slot holds the locus-local A bin.  B's keys are then looked up with the same CAS: an
// empty slot ends the probe and TAKES the slot for the B bin (stored as nb_A + i), so that a second B bin of the same key finds
// it; a slot whose key equals on all words ends it -- an A bin is claimed by an atomicOr of a flag bit, and a second claim is a
// duplicate.  B inserts only fill empty slots, so the probe chain to any A key stays whole; nb_A + nb_B <= 11264 entries never
// fill 16384 slots, whatever the keys.  B is walked in chunks of 256 in B's order; the B-only rank is a ballot per wave and
// the four waves' counts through LDS, a running base across the chunks.
//
// merge_fill_kernel, the one with traffic: a workgroup takes a TILE of union rows of one locus.  The tile's rows' sources go to
// LDS first (a thread per row; the row maps and the counts are stored there).  A tile's part of each merged F is one contiguous
// run of rows x K doubles, so thread t handles elements t, t + 256, ...: consecutive lanes store consecutive 8-byte words
// whatever K is; the (row, column) of an element follows the thread's first by add-and-carry.  Every value is a load and a
// store: bitwise the host form's.  No atomics, nothing relies on a memset.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "merge_rules.h"
#include "stage_host.h"

namespace sb {

constexpr int kMergeThreads = 256;
constexpr int kMergeTileVals = 4096; // weights of one tile: 16 per thread and output, as the differential expansion's
constexpr int kMergeTileRows = 512;  // rows of a tile at most (2 x 2 KB of LDS for their sources)
constexpr int kMergeGridPerCu = 8;   // 8 x 256 threads is the CU's 2048; the deep match's 64 KB table allows 2 of them, its grid is capped at that
constexpr int kMergeDeepPerCu = 2;
constexpr int32_t kMergeClaimed = 1 << 30;

__host__ __device__ inline int merge_tile_rows(int K) { return K < 1 || kMergeTileVals / K > kMergeTileRows ? kMergeTileRows : kMergeTileVals / K < 1 ? 1 : kMergeTileVals / K; }

struct MergeMatchArgs {
   int64_t n_items;             // small form: items; deep form: loci of the list
   const MergeItem *items;      // small form only
   const int32_t *list;
   const int64_t *row_off[2];   // A's, B's: [n_loci + 1]
   const uint32_t *key[2];
   int32_t key_words;
   int32_t *b_of_a, *b_only, *n_only;
};

__global__ __launch_bounds__(kMergeThreads) void merge_match_small_kernel(MergeMatchArgs a)
{
   const int t = threadIdx.x, lane = t & 63, kw = a.key_words;
   for (int64_t q = blockIdx.x; q < a.n_items; q += gridDim.x) {
      const MergeItem item = a.items[q];
      const int P = item.lanes, g = t / P, i = t % P;
      const bool has = g < item.n;
      const int64_t l = has ? a.list[item.first + g] : 0;
      const int64_t a0 = has ? a.row_off[0][l] : 0, b0 = has ? a.row_off[1][l] : 0;
      const int na = has ? (int)min((int64_t)P, a.row_off[0][l + 1] - a0) : 0, nb = has ? (int)min((int64_t)P, a.row_off[1][l + 1] - b0) : 0;
      const uint32_t *ka = a.key[0] + a0 * kw, *kb = a.key[1] + b0 * kw;
      const bool in_a = i < na, in_b = i < nb;
      uint32_t ma[kMergeRegWords], mb[kMergeRegWords];
#pragma unroll
      for (int w = 0; w < kMergeRegWords; ++w) {
         ma[w] = in_a && w < kw ? ka[(int64_t)i * kw + w] : 0u;
         mb[w] = in_b && w < kw ? kb[(int64_t)i * kw + w] : 0u;
      }
      int32_t my_b = -1;
      bool matched = false, dup = false;
      // A's keys pass by: is B's key i among them; did A's key i occur before
      for (int j = 0; j < na; ++j) {
         const uint32_t *k = ka + (int64_t)j * kw;
         bool ea = in_a && j < i, eb = in_b;
#pragma unroll
         for (int w = 0; w < kMergeRegWords; ++w)
            if (w < kw) {
               const uint32_t v = k[w];
               ea &= v == ma[w], eb &= v == mb[w];
            }
         if (kw > kMergeRegWords) {
            if (ea) ea = merge_key_equal(k + kMergeRegWords, ka + (int64_t)i * kw + kMergeRegWords, kw - kMergeRegWords);
            if (eb) eb = merge_key_equal(k + kMergeRegWords, kb + (int64_t)i * kw + kMergeRegWords, kw - kMergeRegWords);
         }
         dup |= ea;
         matched |= eb;
      }
      // B's keys pass by: which of them is A's key i; did B's key i occur before
      for (int j = 0; j < nb; ++j) {
         const uint32_t *k = kb + (int64_t)j * kw;
         bool ea = in_a, eb = in_b && j < i;
#pragma unroll
         for (int w = 0; w < kMergeRegWords; ++w)
            if (w < kw) {
               const uint32_t v = k[w];
               ea &= v == ma[w], eb &= v == mb[w];
            }
         if (kw > kMergeRegWords) {
            if (ea) ea = merge_key_equal(k + kMergeRegWords, ka + (int64_t)i * kw + kMergeRegWords, kw - kMergeRegWords);
            if (eb) eb = merge_key_equal(k + kMergeRegWords, kb + (int64_t)i * kw + kMergeRegWords, kw - kMergeRegWords);
         }
         dup |= eb;
         if (ea) my_b = j;
      }
      // the group's lanes of the wave: the B-only bins before this lane's, and all of them
      const bool only = in_b && !matched;
      const unsigned long long group = (P == 64 ? ~0ull : ((1ull << P) - 1)) << (lane & ~(P - 1));
      const unsigned long long only_bits = __ballot(only) & group, dup_bits = __ballot(dup) & group;
      if (in_a) a.b_of_a[a0 + i] = my_b;
      if (only) a.b_only[b0 + __popcll(only_bits & ((1ull << lane) - 1))] = i;
      if (has && i == 0) a.n_only[l] = dup_bits ? -1 : (int32_t)__popcll(only_bits);
   }
}

__global__ __launch_bounds__(kMergeThreads) void merge_match_deep_kernel(MergeMatchArgs a)
{
   __shared__ int32_t s_tab[kMergeTableSlots];
   __shared__ int32_t s_wave[kMergeThreads / 64];
   __shared__ int32_t s_dup;
   const int t = threadIdx.x, lane = t & 63, wave = t >> 6, kw = a.key_words;
   for (int64_t q = blockIdx.x; q < a.n_items; q += gridDim.x) {
      const int64_t l = a.list[q];
      const int64_t a0 = a.row_off[0][l], b0 = a.row_off[1][l];
      // (the launcher refuses a deeper locus: the table's room for nb_A + nb_B entries rests on it)
      const int na = (int)min((int64_t)kStageMaxBins, a.row_off[0][l + 1] - a0), nb = (int)min((int64_t)kStageMaxBins, a.row_off[1][l + 1] - b0);
      const uint32_t *ka = a.key[0] + a0 * kw, *kb = a.key[1] + b0 * kw;
      for (int x = t; x < kMergeTableSlots; x += kMergeThreads) s_tab[x] = -1;
      for (int i = t; i < na; i += kMergeThreads) a.b_of_a[a0 + i] = -1;
      if (t == 0) s_dup = 0;
      __syncthreads();
      for (int i = t; i < na; i += kMergeThreads) {
         const uint32_t *k = ka + (int64_t)i * kw;
         int slot = merge_slot(merge_key_hash(k, kw));
         for (;;) {
            const int32_t prev = atomicCAS(&s_tab[slot], -1, i);
            if (prev == -1) break;
            if (merge_key_equal(ka + (int64_t)prev * kw, k, kw)) {
               s_dup = 1;
               break;
            }
            slot = (slot + 1) & (kMergeTableSlots - 1);
         }
      }
      __syncthreads();
      int base = 0;
      for (int i0 = 0; i0 < nb; i0 += kMergeThreads) {
         const int i = i0 + t;
         bool only = false;
         if (i < nb) {
            const uint32_t *k = kb + (int64_t)i * kw;
            int slot = merge_slot(merge_key_hash(k, kw));
            for (;;) {
               const int32_t prev = atomicCAS(&s_tab[slot], -1, na + i);
               if (prev == -1) {
                  only = true;
                  break;
               }
               const int32_t e = prev & ~kMergeClaimed;
               if (e < na) {
                  if (merge_key_equal(ka + (int64_t)e * kw, k, kw)) {
                     if (atomicOr(&s_tab[slot], kMergeClaimed) & kMergeClaimed) s_dup = 1;
                     else a.b_of_a[a0 + e] = i;
                     break;
                  }
               } else if (merge_key_equal(kb + (int64_t)(e - na) * kw, k, kw)) {
                  s_dup = 1;
                  break;
               }
               slot = (slot + 1) & (kMergeTableSlots - 1);
            }
         }
         const unsigned long long bits = __ballot(only);
         if (lane == 0) s_wave[wave] = (int32_t)__popcll(bits);
         __syncthreads();
         int before = base, all = 0;
         for (int w = 0; w < kMergeThreads / 64; ++w) before += w < wave ? s_wave[w] : 0, all += s_wave[w];
         if (only) a.b_only[b0 + before + __popcll(bits & ((1ull << lane) - 1))] = i;
         base += all;
         __syncthreads(); // (the waves' counts are read: the next chunk's may be written)
      }
      if (t == 0) a.n_only[l] = s_dup ? -1 : base;
      __syncthreads(); // (the LDS is free for the workgroup's next locus)
   }
}

struct MergeFillArgs {
   int64_t n_tiles;
   const MergeTile *tiles;
   const int64_t *row_off[2], *f_off[2]; // A's, B's: [n_loci + 1]
   const int64_t *iso_off, *row_off_u, *f_off_u;
   const int32_t *b_of_a, *b_only;
   const int32_t *count[2];
   const double *F[2], *X[2];            // X[s]: the other sample's shape, or null
   int32_t *row[2], *count_u[2];
   double *F_u[2];
};

__global__ __launch_bounds__(kMergeThreads) void merge_fill_kernel(MergeFillArgs a)
{
   __shared__ int32_t s_row[2][kMergeTileRows];
   const int t = threadIdx.x;
   for (int64_t q = blockIdx.x; q < a.n_tiles; q += gridDim.x) {
      const MergeTile tile = a.tiles[q];
      const int64_t l = tile.locus;
      const int K = (int)(a.iso_off[l + 1] - a.iso_off[l]);
      const int64_t a0 = a.row_off[0][l], b0 = a.row_off[1][l], u0 = a.row_off_u[l];
      const int64_t na = a.row_off[0][l + 1] - a0, nu = a.row_off_u[l + 1] - u0;
      const int rows = (int)max((int64_t)0, min((int64_t)min(tile.rows, kMergeTileRows), nu - tile.row0)); // (the launcher cuts the tiles inside the locus)
      for (int r = t; r < rows; r += kMergeThreads) {
         const int64_t u = tile.row0 + r;
         int32_t ra, rb;
         merge_row(u, na, a.b_of_a + a0, a.b_only + b0, &ra, &rb);
         s_row[0][r] = ra, s_row[1][r] = rb;
         a.row[0][u0 + u] = ra < 0 ? -1 : (int32_t)(a0 + ra), a.row[1][u0 + u] = rb < 0 ? -1 : (int32_t)(b0 + rb);
         a.count_u[0][u0 + u] = ra < 0 ? 0 : a.count[0][a0 + ra], a.count_u[1][u0 + u] = rb < 0 ? 0 : a.count[1][b0 + rb];
      }
      __syncthreads();
      if (K > 0) {
         const double *Fa = a.F[0] + a.f_off[0][l], *Fb = a.F[1] + a.f_off[1][l];
         const double *Xa = a.X[0] ? a.X[0] + a.f_off[1][l] : nullptr, *Xb = a.X[1] ? a.X[1] + a.f_off[0][l] : nullptr;
         double *oa = a.F_u[0] + a.f_off_u[l] + (int64_t)tile.row0 * K, *ob = a.F_u[1] + a.f_off_u[l] + (int64_t)tile.row0 * K;
         const int dr = kMergeThreads / K, dc = kMergeThreads % K;
         int r = t / K, c = t % K;
         for (int i = t; i < rows * K; i += kMergeThreads) {
            const int32_t ra = s_row[0][r], rb = s_row[1][r];
            oa[i] = merge_weight(ra, Fa, rb, Xa, Fb, K, c);
            ob[i] = merge_weight(rb, Fb, ra, Xb, Fa, K, c);
            r += dr, c += dc;
            if (c >= K) c -= K, ++r;
         }
      }
      __syncthreads(); // (the tile is written: the LDS is free for the workgroup's next one)
   }
}

} // namespace sb
