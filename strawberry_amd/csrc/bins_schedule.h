// strawberry_amd/csrc/bins_schedule.h -- what the device grouping (sbgpu_bins_create_device, exonbin_api.hip) decides on the
// host, as data and free of HIP: a plain C++ compiler takes this header alone.  The tables' sizes, the order of the loci, which
// kernel instantiation serves which range of them at which grid, the five memory layouts, and what follows from the bin counts
// and flags that come back (redo, assign, the prefix sums, why the device form declines).  bins_create_device_impl issues what
// these functions return and decides nothing of this itself; tests/test_bins_schedule_cpp.py states the rules a second time.
#pragma once

#include <string>

#include "stage_host.h"

namespace sb {

// Two table sizes: loci of up to 256 hits (most of them) take 1024 slots -- 18 KB of LDS, so that many
// workgroups share a CU and hide each other's memory latency -- the others 8192 (140 KB, one per CU).
constexpr int kBinsSlotsSmall = 1024, kBinsMaxSmall = 256;   // at most one bin per hit
constexpr int kBinsSlotsMid = 2048, kBinsMaxMid = 1400;      // larger loci first try this one (36 KB: four workgroups per CU);
                                                             // a locus with more bins than that is redone with the big table
constexpr int kBinsSlotsLight = 1024, kBinsMaxLight = 512;   // ... the loci between small and heavy a lighter one (24 KB: six per CU)
constexpr int kBinsSlotsBig = 8192, kBinsMaxBig = 5600;      // ~0.7 load
constexpr int kBinsSmallHits = 256;
constexpr int kBinsThreads = 256;      // the small table's workgroup, and the light one's
constexpr int kBinsThreadsMid = 512;   // the two-pass form's
constexpr int kBinsThreadsAccum = 1024; // the single-pass form's middle table: two workgroups of 16 waves per CU
constexpr int kBinsThreadsBig = 1024;  // the big table fills a CU's LDS: one workgroup per CU, so it brings 16 waves
enum : int32_t { kBinsUnsorted = 1, kBinsFractional = 2, kBinsTableFull = 4, kBinsMassOverflow = 8, kBinsRunTooLong = 128 };
constexpr int kScanTile = 4096, kScanPerLane = 16; // the prefix scans' tile: 256 lanes of 16 entries

// ---- the order of the loci: small ones in index order, then the heavy ones from the largest down, then the rest in index order.
// A locus is one workgroup's work, and a locus of 10^5 hits that starts last would be the kernel's tail; only those few are
// sorted (a full sort of 55 000 loci costs 2.6 ms of host time).  They also get a launch of their own with 1024 threads; the
// loci between -- a few thousand hits, two or three per thread of such a workgroup -- are bound by the per-locus fixed cost
// (table set-up, six workgroup barriers, the ranking), which 256-thread workgroups, several per CU, pay side by side:
// 2.62 -> 1.83 ms on the chain sample (8192 was the best of 2000 ... 100 000).
inline int64_t bins_heavy_hits(int64_t n_loci, int64_t n_hits) { return std::max<int64_t>(8192, 3 * (n_hits / std::max<int64_t>(n_loci, 1))); }

struct BinsOrder {
   std::vector<int32_t> order; // [n_loci]
   int64_t n_small = 0, n_heavy = 0, n_mid = 0;
};
inline BinsOrder bins_locus_order(int64_t n_loci, const int64_t *locus_hit_off, int64_t n_hits)
{
   BinsOrder o;
   o.order.resize((size_t)n_loci);
   auto hits_of = [&](int32_t l) { return locus_hit_off[l + 1] - locus_hit_off[l]; };
   int64_t n = 0;
   for (int64_t l = 0; l < n_loci; ++l)
      if (hits_of((int32_t)l) <= kBinsSmallHits) o.order[(size_t)n++] = (int32_t)l;
   o.n_small = n;
   for (int64_t l = 0; l < n_loci; ++l)
      if (hits_of((int32_t)l) > kBinsSmallHits) o.order[(size_t)n++] = (int32_t)l;
   const int64_t heavy = bins_heavy_hits(n_loci, n_hits);
   auto first_big = o.order.begin() + o.n_small;
   auto mid = std::stable_partition(first_big, o.order.end(), [&](int32_t l) { return hits_of(l) >= heavy; });
   std::sort(first_big, mid, [&](int32_t x, int32_t y) { return hits_of(x) != hits_of(y) ? hits_of(x) > hits_of(y) : x < y; });
   o.n_heavy = mid - first_big;
   o.n_mid = n_loci - o.n_small - o.n_heavy;
   return o;
}

// ---- the grouping launches.  The single-pass kernels (bins_accum_kernel) where a bin's compat union and its key fit two words
// each, else the two-pass form (bins_locus_kernel), whose global atomics want the counts and compat words zeroed first.  The
// heavy loci run on 1024 threads and the middle table; the others on 256 and a table of 1024 slots / 512 bins (more workgroups
// per CU, cheaper barriers: 1.83 -> 1.41 ms); whatever has more bins than its table holds (retry) is redone with the big one.
enum BinsKernelKind : int { kBinsAccum, kBinsLocus };
struct BinsStep {
   int kernel, slots, max_bins, threads, cw; // the instantiation (cw: the accum kernel's compat words, 0 for the locus kernel)
   bool retry;                               // a locus the table cannot hold is marked for the big table, not flagged
   int64_t first, count;                     // its loci: order[first, first + count)
   int grid_mult;                            // the grid is min(count, grid_mult * 8 * CUs)
};
struct BinsGroupSteps {
   bool single_pass = false, zero_first = false;
   int n_steps = 0;
   BinsStep steps[3] = {};
};
inline BinsGroupSteps bins_group_steps(int64_t n_small, int64_t n_heavy, int64_t n_mid, int compat_words, int key_words)
{
   BinsGroupSteps g;
   g.single_pass = compat_words <= 2 && key_words <= 2;
   g.zero_first = !g.single_pass;
   auto step = [&](int kernel, int slots, int max_bins, int threads, bool retry, int64_t first, int64_t count, int grid_mult) {
      if (count) g.steps[g.n_steps++] = {kernel, slots, max_bins, threads, kernel == kBinsAccum ? compat_words : 0, retry, first, count, grid_mult};
   };
   if (g.single_pass) {
      step(kBinsAccum, kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, false, 0, n_small, 4);
      step(kBinsAccum, kBinsSlotsMid, kBinsMaxMid, kBinsThreadsAccum, true, n_small, n_heavy, 4);
      step(kBinsAccum, kBinsSlotsLight, kBinsMaxLight, kBinsThreads, true, n_small + n_heavy, n_mid, 8);
   } else {
      step(kBinsLocus, kBinsSlotsSmall, kBinsMaxSmall, kBinsThreads, false, 0, n_small, 4);
      step(kBinsLocus, kBinsSlotsMid, kBinsMaxMid, kBinsThreadsMid, true, n_small, n_heavy + n_mid, 4);
   }
   return g;
}

// ---- the five layouts.  Every member but `bytes` and `zero_bytes` is an offset.
// The context's scratch.  Hit-indexed arrays: bin b of locus l lives at index locus_hit_off[l] + b.
struct BinsScratchLayout {
   size_t local, rep;
   size_t cnt, cmp, zero_bytes; // bin_count + bin_compat are zeroed together: [cnt, cnt + zero_bytes)
   size_t nb, nu, flag;         // flag [0]: the grouping kernels' flags, [1]: the middle's (pack, pairs)
   size_t hoff, roff, order, dup;
   size_t span, fhash;          // spans and hashes: the exon-bin kernel's (they take no room then), or made here
   size_t bytes;
};
inline BinsScratchLayout bins_scratch_layout(int64_t n_loci, int64_t n_hits, int compat_words, bool own_span)
{
   const size_t nh1 = at_least_1(n_hits), nl = (size_t)n_loci;
   Arena a;
   BinsScratchLayout L;
   L.local = a.take(nh1 * 4), L.rep = a.take(nh1 * 4);
   L.cnt = a.take(nh1 * 4), L.cmp = a.take(nh1 * 4 * (size_t)compat_words);
   L.zero_bytes = a.size - L.cnt;
   L.nb = a.take(nl * 4), L.nu = a.take(nl * 4), L.flag = a.take(256);
   L.hoff = a.take((nl + 1) * 8), L.roff = a.take((nl + 1) * 8), L.order = a.take(nl * 4), L.dup = a.take(nh1);
   L.span = a.take(own_span ? nh1 * 8 : 0), L.fhash = a.take(own_span ? nh1 * 4 : 0);
   L.bytes = a.size;
   return L;
}
// The packed per-bin arrays (bins <= hits): an allocation of its own that the handle takes over (DeviceBinArrays)
struct BinsPackedLayout {
   size_t cnt, key, cmp, bytes;
};
inline BinsPackedLayout bins_packed_layout(int64_t n_hits, int compat_words, int key_words)
{
   const size_t nh1 = at_least_1(n_hits);
   Arena a;
   BinsPackedLayout L;
   L.cnt = a.take(nh1 * 4), L.key = a.take(nh1 * 4 * (size_t)key_words), L.cmp = a.take(nh1 * 4 * (size_t)compat_words);
   L.bytes = a.size;
   return L;
}
// What the pairs' kernels read and the scans write.  tot: the totals of the two scans [n_bins, n_elem, n_pairs, n_pair_segs];
// part: the scans' tile sums, two rows of max(row_tiles, iso_tiles) + 1.
struct PairsInLayout {
   size_t isoff, foff, segoff, segl, segr, isegoff, isegidx, isoloc, isolen, pcnt, scnt, poff, soff, tot, part, bytes;
   int64_t row_tiles, iso_tiles;
};
inline PairsInLayout pairs_in_layout(int64_t n_loci, int64_t n_iso, int64_t n_seg, size_t n_iso_segs)
{
   const size_t nl1 = (size_t)n_loci + 1, ni1 = at_least_1(n_iso), ns1 = (size_t)n_seg + 1;
   Arena a;
   PairsInLayout L;
   L.isoff = a.take(nl1 * 8), L.foff = a.take(nl1 * 8), L.segoff = a.take(nl1 * 8), L.segl = a.take(ns1 * 4), L.segr = a.take(ns1 * 4);
   L.isegoff = a.take((ni1 + 1) * 8), L.isegidx = a.take(std::max<size_t>(n_iso_segs, 1) * 4), L.isoloc = a.take(ni1 * 4), L.isolen = a.take(ni1 * 4);
   L.pcnt = a.take(ni1 * 4), L.scnt = a.take(ni1 * 4), L.poff = a.take((ni1 + 1) * 8), L.soff = a.take((ni1 + 1) * 8), L.tot = a.take(256);
   L.row_tiles = (n_loci + kScanTile - 1) / kScanTile, L.iso_tiles = std::max<int64_t>(1, (n_iso + kScanTile - 1) / kScanTile);
   L.part = a.take((size_t)(2 * std::max(L.row_tiles, L.iso_tiles) + 2) * 8);
   L.bytes = a.size;
   return L;
}
// Pinned host words for what comes back between the kernels: bins per locus, hits used per locus, flags, totals
struct BinsPinnedLayout {
   size_t nb, nu, flag, tot, bytes;
};
inline BinsPinnedLayout bins_pinned_layout(int64_t n_loci)
{
   Arena a;
   BinsPinnedLayout L;
   L.nb = a.take((size_t)n_loci * 4), L.nu = a.take((size_t)n_loci * 4), L.flag = a.take(256), L.tot = a.take(256);
   L.bytes = a.size;
   return L;
}
// The pairs' arena (DevicePairs), known once the pairs are counted
struct PairsLayout {
   size_t seg_off, out_index, seg_lens, mask, iso_len, bytes;
};
inline PairsLayout pairs_layout(int64_t n_pairs, int64_t n_pair_segs)
{
   const size_t np1 = (size_t)n_pairs + 1;
   Arena a;
   PairsLayout L;
   L.seg_off = a.take(np1 * 8), L.out_index = a.take(np1 * 8), L.seg_lens = a.take(((size_t)n_pair_segs + 1) * 4), L.mask = a.take(np1 * 4), L.iso_len = a.take(np1 * 4);
   L.bytes = a.size;
   return L;
}

// ---- what follows from the counts and flags that come back.
// Where nothing on the host has to come between (the usual case: single-pass kernels, hit -> bin not asked for), the middle --
// rows scanned, bins packed, pairs counted -- is launched before the bin counts are back; should the counts then call for a
// fix-up (a locus for the big table, fractional masses), the fix-up runs and the middle is launched again over its result.
inline bool bins_speculative(bool single_pass, bool want_hit_bin) { return single_pass && !want_hit_bin; }
// the loci of `nb` [n_loci] (bins per locus) for which keep(nb[l]) holds, ascending
template <class Keep>
inline std::vector<int32_t> bins_loci_where(const int32_t *nb, int64_t n_loci, Keep keep)
{
   std::vector<int32_t> loci;
   for (int64_t l = 0; l < n_loci; ++l)
      if (keep(nb[l])) loci.push_back((int32_t)l);
   return loci;
}
// loci the retry tables could not hold: again, with the big one
inline std::vector<int32_t> bins_redo_list(const int32_t *nb, int64_t n_loci) { return bins_loci_where(nb, n_loci, [](int32_t n) { return n < 0; }); }
// hit -> bin: the single-pass kernels leave it out; it is made where somebody reads it (the caller's hit_bin or hit_bin_local,
// the ordered masses of a fractional input).  Loci the big table served have theirs already.
inline bool bins_assign_wanted(bool single_pass, bool want_hit_bin, bool want_local, int32_t flags, int64_t n_hits)
{
   return single_pass && (want_hit_bin || want_local || flags == kBinsFractional) && n_hits;
}
inline std::vector<int32_t> bins_assign_list(const int32_t *nb, int64_t n_loci) { return bins_loci_where(nb, n_loci, [](int32_t n) { return n <= kBinsMaxMid; }); }
// the prefix sums the device's scans make too (the handle, the caller's plan), and the hits that landed in a bin
struct BinsRows {
   std::vector<int64_t> row_off, f_off; // [n_loci + 1]
   int64_t used = 0;
};
inline BinsRows bins_rows(const int32_t *nb, const int32_t *nu, const int64_t *iso_off, int64_t n_loci)
{
   BinsRows r;
   r.row_off.assign((size_t)n_loci + 1, 0), r.f_off.assign((size_t)n_loci + 1, 0);
   for (int64_t l = 0; l < n_loci; ++l) {
      r.row_off[(size_t)l + 1] = r.row_off[(size_t)l] + nb[l];
      r.f_off[(size_t)l + 1] = r.f_off[(size_t)l] + (int64_t)nb[l] * (iso_off[l + 1] - iso_off[l]);
      r.used += nu[l];
   }
   return r;
}
// why the grouping kernels' flags send the caller to the host form
inline std::string bins_decline_reason(int32_t flags)
{
   std::string why = "sbgpu_bins_create_device: not covered by the device form:";
   if (flags & kBinsUnsorted) why += " hits of a locus are not sorted by (left, right);";
   if (flags & kBinsFractional) why += " fractional hit masses next to another obstacle;";
   if (flags & kBinsTableFull) why += " a locus has more bins than the LDS table holds;";
   if (flags & kBinsMassOverflow) why += " a bin's mass reaches 2^24;";
   if (flags & kBinsRunTooLong) why += " fractional masses and more than 48 fragments of one bin starting at one position;";
   return why + " use sbgpu_bins_create";
}

} // namespace sb
