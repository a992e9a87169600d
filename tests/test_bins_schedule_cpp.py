"""What the device grouping decides on the host (csrc/bins_schedule.h) from a stand-alone C++ program that includes that header
alone and is built with AddressSanitizer and UBSan: the loci's order against a restated rule, the grouping launches against a table
written out by hand from what sbgpu_bins_create_device issued before the schedule was a function, the five layouts against the
`off += up(...)` chains they replace, and the follow-up decisions on hand-made counts and flags.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "bins_schedule.h"
#include <cstdio>
#include <cstring>
#include <numeric>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
using namespace sb;

// ---- the order, restated: three lists -- small in index order, heavy by hits descending (a stable sort: ties by index), the rest
struct Order { std::vector<int32_t> order; int64_t n_small, n_heavy, n_mid; };
static Order order_by_rule(const std::vector<int64_t> &hits)
{
   const int64_t nl = (int64_t)hits.size(), nh = std::accumulate(hits.begin(), hits.end(), (int64_t)0);
   int64_t heavy = 3 * (nh / (nl > 1 ? nl : 1));
   if (heavy < 8192) heavy = 8192;
   std::vector<int32_t> small, big_heavy, rest;
   for (int32_t l = 0; l < (int32_t)nl; ++l) (hits[(size_t)l] <= 256 ? small : hits[(size_t)l] >= heavy ? big_heavy : rest).push_back(l);
   std::stable_sort(big_heavy.begin(), big_heavy.end(), [&](int32_t x, int32_t y) { return hits[(size_t)x] > hits[(size_t)y]; });
   Order o = {small, (int64_t)small.size(), (int64_t)big_heavy.size(), (int64_t)rest.size()};
   o.order.insert(o.order.end(), big_heavy.begin(), big_heavy.end());
   o.order.insert(o.order.end(), rest.begin(), rest.end());
   return o;
}
// -> the function's order where it agrees with the rule and with the counts given (-1: not checked), else an empty one
static std::vector<int32_t> order_of(const std::vector<int64_t> &hits, int64_t n_small, int64_t n_heavy, int64_t n_mid)
{
   std::vector<int64_t> off(hits.size() + 1, 0);
   for (size_t l = 0; l < hits.size(); ++l) off[l + 1] = off[l] + hits[l];
   const BinsOrder got = bins_locus_order((int64_t)hits.size(), off.data(), off.back());
   const Order want = order_by_rule(hits);
   if (got.order != want.order || got.n_small != want.n_small || got.n_heavy != want.n_heavy || got.n_mid != want.n_mid) return {};
   if (n_small >= 0 && (got.n_small != n_small || got.n_heavy != n_heavy || got.n_mid != n_mid)) return {};
   return got.order;
}
using V = std::vector<int32_t>;

// ---- the launches, by hand: {kernel, slots, max_bins, threads, cw, retry, first, count, grid_mult}
static bool same_step(const BinsStep &a, const BinsStep &b)
{
   return a.kernel == b.kernel && a.slots == b.slots && a.max_bins == b.max_bins && a.threads == b.threads && a.cw == b.cw && a.retry == b.retry &&
          a.first == b.first && a.count == b.count && a.grid_mult == b.grid_mult;
}
static bool steps_are(const BinsGroupSteps &g, bool single_pass, std::vector<BinsStep> want)
{
   if (g.single_pass != single_pass || g.zero_first != !single_pass || g.n_steps != (int)want.size()) return false;
   for (int i = 0; i < g.n_steps; ++i)
      if (!same_step(g.steps[i], want[(size_t)i])) return false;
   return true;
}

// ---- the layouts, restated as the chains they replace
static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
static bool ascending_in(std::initializer_list<size_t> offsets, size_t total)
{
   size_t last = 0;
   bool first = true;
   for (size_t o : offsets) {
      if (o % 256 || o > total || (!first && o < last)) return false;
      last = o, first = false;
   }
   return total % 256 == 0;
}
static int check_layouts(int64_t nl, int64_t nh, int cw, int kw, bool own_span, int64_t n_iso, int64_t n_seg, size_t n_iso_segs, int64_t n_pairs, int64_t n_psegs)
{
   const size_t nh1 = (size_t)(nh > 0 ? nh : 1);
   {  // the scratch arena
      size_t off = 0;
      const size_t o_local = off; off += up(nh1 * 4);
      const size_t o_rep = off; off += up(nh1 * 4);
      const size_t o_zero = off;
      const size_t o_cnt = off; off += up(nh1 * 4);
      const size_t o_cmp = off; off += up(nh1 * 4 * (size_t)cw);
      const size_t zero_bytes = off - o_zero;
      const size_t o_nb = off; off += up((size_t)nl * 4);
      const size_t o_nu = off; off += up((size_t)nl * 4);
      const size_t o_flag = off; off += 256;
      const size_t o_hoff = off; off += up((size_t)(nl + 1) * 8);
      const size_t o_roff = off; off += up((size_t)(nl + 1) * 8);
      const size_t o_order = off; off += up((size_t)nl * 4);
      const size_t o_dup = off; off += up(nh1);
      const size_t o_span = off; off += own_span ? up(nh1 * 8) : 0;
      const size_t o_fhash = off; off += own_span ? up(nh1 * 4) : 0;
      const BinsScratchLayout L = bins_scratch_layout(nl, nh, cw, own_span);
      CHECK(L.local == o_local && L.rep == o_rep && L.cnt == o_cnt && L.cmp == o_cmp && L.zero_bytes == zero_bytes && L.nb == o_nb && L.nu == o_nu);
      CHECK(L.flag == o_flag && L.hoff == o_hoff && L.roff == o_roff && L.order == o_order && L.dup == o_dup && L.span == o_span && L.fhash == o_fhash);
      CHECK(L.bytes == off);
      CHECK(ascending_in({L.local, L.rep, L.cnt, L.cmp, L.nb, L.nu, L.flag, L.hoff, L.roff, L.order, L.dup, L.span, L.fhash}, L.bytes));
      CHECK(L.zero_bytes == up(nh1 * 4) + up(nh1 * 4 * (size_t)cw) && L.cnt + L.zero_bytes == L.nb && L.zero_bytes % 16 == 0); // exactly cnt + cmp
      CHECK(own_span ? L.bytes - L.span == up(nh1 * 8) + up(nh1 * 4) : (L.span == L.bytes && L.fhash == L.bytes));          // no bytes when brought
   }
   {  // the packed per-bin arrays
      size_t off = 0;
      const size_t p_cnt = off; off += up(nh1 * 4);
      const size_t p_key = off; off += up(nh1 * 4 * (size_t)kw);
      const size_t p_cmp = off; off += up(nh1 * 4 * (size_t)cw);
      const BinsPackedLayout P = bins_packed_layout(nh, cw, kw);
      CHECK(P.cnt == p_cnt && P.key == p_key && P.cmp == p_cmp && P.bytes == off && ascending_in({P.cnt, P.key, P.cmp}, P.bytes));
   }
   {  // the pairs' inputs
      const size_t ni1 = (size_t)(n_iso > 0 ? n_iso : 1), nsi1 = n_iso_segs ? n_iso_segs : 1;
      size_t off = 0;
      const size_t r_isoff = off; off += up((size_t)(nl + 1) * 8);
      const size_t r_foff = off; off += up((size_t)(nl + 1) * 8);
      const size_t r_segoff = off; off += up((size_t)(nl + 1) * 8);
      const size_t r_segl = off; off += up((size_t)(n_seg + 1) * 4);
      const size_t r_segr = off; off += up((size_t)(n_seg + 1) * 4);
      const size_t r_isegoff = off; off += up((ni1 + 1) * 8);
      const size_t r_isegidx = off; off += up(nsi1 * 4);
      const size_t r_isoloc = off; off += up(ni1 * 4);
      const size_t r_isolen = off; off += up(ni1 * 4);
      const size_t r_pcnt = off; off += up(ni1 * 4);
      const size_t r_scnt = off; off += up(ni1 * 4);
      const size_t r_poff = off; off += up((ni1 + 1) * 8);
      const size_t r_soff = off; off += up((ni1 + 1) * 8);
      const size_t r_tot = off; off += 256;
      const int64_t row_tiles = (nl + 4096 - 1) / 4096, iso_tiles = std::max<int64_t>(1, (n_iso + 4096 - 1) / 4096);
      const size_t r_part = off; off += up((size_t)(2 * std::max(row_tiles, iso_tiles) + 2) * 8);
      const PairsInLayout R = pairs_in_layout(nl, n_iso, n_seg, n_iso_segs);
      CHECK(R.isoff == r_isoff && R.foff == r_foff && R.segoff == r_segoff && R.segl == r_segl && R.segr == r_segr && R.isegoff == r_isegoff);
      CHECK(R.isegidx == r_isegidx && R.isoloc == r_isoloc && R.isolen == r_isolen && R.pcnt == r_pcnt && R.scnt == r_scnt && R.poff == r_poff);
      CHECK(R.soff == r_soff && R.tot == r_tot && R.part == r_part && R.bytes == off && R.row_tiles == row_tiles && R.iso_tiles == iso_tiles);
      CHECK(ascending_in({R.isoff, R.foff, R.segoff, R.segl, R.segr, R.isegoff, R.isegidx, R.isoloc, R.isolen, R.pcnt, R.scnt, R.poff, R.soff, R.tot, R.part}, R.bytes));
   }
   {  // the pinned words
      const size_t h_nb = 0, h_nu = up((size_t)nl * 4), h_flag = h_nu + up((size_t)nl * 4), h_tot = h_flag + 256;
      const BinsPinnedLayout H = bins_pinned_layout(nl);
      CHECK(H.nb == h_nb && H.nu == h_nu && H.flag == h_flag && H.tot == h_tot && H.bytes == h_tot + 256 && ascending_in({H.nb, H.nu, H.flag, H.tot}, H.bytes));
   }
   {  // the pairs' arena
      size_t off = 0;
      const size_t o_seg_off = off; off += up(((size_t)n_pairs + 1) * 8);
      const size_t o_out_index = off; off += up(((size_t)n_pairs + 1) * 8);
      const size_t o_seg_lens = off; off += up(((size_t)n_psegs + 1) * 4);
      const size_t o_mask = off; off += up(((size_t)n_pairs + 1) * 4);
      const size_t o_iso_len = off; off += up(((size_t)n_pairs + 1) * 4);
      const PairsLayout Q = pairs_layout(n_pairs, n_psegs);
      CHECK(Q.seg_off == o_seg_off && Q.out_index == o_out_index && Q.seg_lens == o_seg_lens && Q.mask == o_mask && Q.iso_len == o_iso_len && Q.bytes == off);
      CHECK(ascending_in({Q.seg_off, Q.out_index, Q.seg_lens, Q.mask, Q.iso_len}, Q.bytes));
   }
   return 0;
}

int main()
{
   // ---- the constants the rest is written against
   CHECK(kBinsSlotsSmall == 1024 && kBinsMaxSmall == 256 && kBinsSlotsMid == 2048 && kBinsMaxMid == 1400 && kBinsSlotsLight == 1024 && kBinsMaxLight == 512);
   CHECK(kBinsSlotsBig == 8192 && kBinsMaxBig == 5600 && kBinsSmallHits == 256);
   CHECK(kBinsThreads == 256 && kBinsThreadsMid == 512 && kBinsThreadsAccum == 1024 && kBinsThreadsBig == 1024 && kScanTile == 4096);
   CHECK(bins_heavy_hits(4, 40000) == 30000 && bins_heavy_hits(100, 1000) == 8192 && bins_heavy_hits(0, 0) == 8192 && bins_heavy_hits(1, 10000) == 30000);

   // ---- the order
   // 256 hits are small, 257 are not
   CHECK((order_of({257, 256, 0, 300}, 2, 0, 2) == V{1, 2, 0, 3}));
   // heavy - 1 / heavy where 8192 binds (the mean is 2055: 3 x the mean stays below) ...
   CHECK((order_of({8191, 8192, 10, 10, 10, 10, 10, 10}, 6, 1, 1) == V{2, 3, 4, 5, 6, 7, 1, 0}));
   // ... and where 3 x the mean binds: 40 000 hits over 4 loci, heavy = 30 000
   CHECK((order_of({300, 30000, 9700, 0}, 1, 1, 2) == V{3, 1, 0, 2}));
   CHECK((order_of({301, 29999, 9700, 0}, 1, 0, 3) == V{3, 0, 1, 2}));
   // equal-hit heavy loci: by index; larger ones before them
   CHECK((order_of({9000, 10, 9000, 9500, 9000, 10, 300, 10, 10, 10, 10, 10, 10, 10}, 9, 4, 1) == V{1, 5, 7, 8, 9, 10, 11, 12, 13, 3, 0, 2, 4, 6}));
   // one locus: empty, small, big (never heavy: 3 x the mean is beyond it)
   CHECK((order_of({0}, 1, 0, 0) == V{0}));
   CHECK((order_of({256}, 1, 0, 0) == V{0}));
   CHECK((order_of({100000}, 0, 0, 1) == V{0}));
   // all loci empty; no big locus
   CHECK((order_of({0, 0, 0}, 3, 0, 0) == V{0, 1, 2}));
   CHECK((order_of({5, 256, 0, 77}, 4, 0, 0) == V{0, 1, 2, 3}));
   // every big locus is heavy
   CHECK((order_of({0, 9000, 0, 0, 12000, 0, 0, 0}, 6, 2, 0) == V{0, 2, 3, 5, 6, 7, 4, 1}));
   {  // many loci, the rule only
      std::vector<int64_t> hits;
      uint64_t x = 88172645463325252ull;
      for (int l = 0; l < 3000; ++l) {
         x ^= x << 13, x ^= x >> 7, x ^= x << 17;
         hits.push_back(l % 97 == 0 ? 8000 + (int64_t)(x % 400) : l % 5 == 0 ? 250 + (int64_t)(x % 12) : (int64_t)(x % 200));
      }
      CHECK(order_of(hits, -1, -1, -1).size() == 3000);
   }

   // ---- the launches: every presence pattern of small / heavy / middle loci under every word count
   const int words[5][2] = {{1, 1}, {1, 2}, {2, 2}, {3, 2}, {1, 3}};
   int n_cases = 0;
   for (const auto &w : words)
      for (int present = 0; present < 8; ++present) {
         const int cw = w[0], kw = w[1];
         const int64_t ns = present & 1 ? 5 : 0, nhv = present & 2 ? 2 : 0, nm = present & 4 ? 7 : 0;
         const BinsGroupSteps g = bins_group_steps(ns, nhv, nm, cw, kw);
         std::vector<BinsStep> want;
         const bool single = (cw == 1 && kw == 1) || (cw == 1 && kw == 2) || (cw == 2 && kw == 2);
         if (single) {
            // small: bins_accum_kernel<1024, 256, 256, cw>, grid min(n, cap * 4)
            if (ns) want.push_back({kBinsAccum, 1024, 256, 256, cw, false, 0, ns, 4});
            // heavy (alone or not: the all-heavy branch launched the same over the same list): <2048, 1400, 1024, cw, retry>, cap * 4
            if (nhv) want.push_back({kBinsAccum, 2048, 1400, 1024, cw, true, ns, nhv, 4});
            // the others: <1024, 512, 256, cw, retry>, cap * 8
            if (nm) want.push_back({kBinsAccum, 1024, 512, 256, cw, true, ns + nhv, nm, 8});
         } else {
            // bins_locus_kernel<1024, 256, 256>, then every big locus in order: <2048, 1400, 512, retry>; both cap * 4
            if (ns) want.push_back({kBinsLocus, 1024, 256, 256, 0, false, 0, ns, 4});
            if (nhv + nm) want.push_back({kBinsLocus, 2048, 1400, 512, 0, true, ns, nhv + nm, 4});
         }
         if (!steps_are(g, single, want)) {
            std::printf("steps differ: cw %d kw %d present %d\n", cw, kw, present);
            return 1;
         }
         ++n_cases;
      }
   CHECK(n_cases == 40);
   // a few written out whole
   CHECK(steps_are(bins_group_steps(0, 0, 0, 1, 2), true, {}));
   CHECK(steps_are(bins_group_steps(3, 4, 0, 1, 2), true, {{kBinsAccum, 1024, 256, 256, 1, false, 0, 3, 4}, {kBinsAccum, 2048, 1400, 1024, 1, true, 3, 4, 4}}));
   CHECK(steps_are(bins_group_steps(0, 4, 0, 2, 1), true, {{kBinsAccum, 2048, 1400, 1024, 2, true, 0, 4, 4}}));
   CHECK(steps_are(bins_group_steps(3, 0, 9, 2, 2), true, {{kBinsAccum, 1024, 256, 256, 2, false, 0, 3, 4}, {kBinsAccum, 1024, 512, 256, 2, true, 3, 9, 8}}));
   CHECK(steps_are(bins_group_steps(3, 4, 9, 3, 5), false, {{kBinsLocus, 1024, 256, 256, 0, false, 0, 3, 4}, {kBinsLocus, 2048, 1400, 512, 0, true, 3, 13, 4}}));

   // ---- the layouts
   if (check_layouts(1, 0, 1, 1, true, 0, 0, 0, 0, 0)) return 1;            // no hits, no isoforms
   if (check_layouts(1, 0, 2, 2, false, 1, 1, 1, 0, 0)) return 1;
   if (check_layouts(3, 13000, 1, 2, true, 60, 120, 900, 4321, 9876)) return 1;
   if (check_layouts(3, 13000, 1, 2, false, 60, 120, 900, 4321, 9876)) return 1;
   if (check_layouts(55000, 1760001, 2, 2, false, 250000, 400000, 3000001, 1400000, 5000000)) return 1; // several scan tiles
   if (check_layouts(4097, 63, 3, 5, true, 71 * 30, 3900, 0, 64, 0)) return 1;
   if (check_layouts(64, 64, 128, 4, true, 4096, 4097, 1, 1, 1)) return 1;

   // ---- the follow-ups
   CHECK(bins_speculative(true, false) && !bins_speculative(true, true) && !bins_speculative(false, false) && !bins_speculative(false, true));
   const int32_t nb[] = {0, 12, -1, 1400, 1401, -7, 5600, 3};
   CHECK((bins_redo_list(nb, 8) == V{2, 5}));
   CHECK((bins_assign_list(nb, 8) == V{0, 1, 2, 3, 5, 7})); // <= kBinsMaxMid: what the single-pass tables served
   CHECK(bins_redo_list(nb, 2).empty() && bins_redo_list(nb, 0).empty() && bins_assign_list(nb, 0).empty());
   for (int single = 0; single < 2; ++single)
      for (int hb = 0; hb < 2; ++hb)
         for (int local = 0; local < 2; ++local)
            for (int32_t flags : {0, 1, 2, 3, 4, 6, 128, 130})
               for (int64_t n_hits : {0, 9}) CHECK(bins_assign_wanted(single, hb, local, flags, n_hits) == (single && (hb || local || flags == 2) && n_hits > 0));
   {
      const int32_t nbr[] = {2, 0, 5}, nur[] = {10, 0, 31};
      const int64_t iso_off[] = {0, 3, 7, 8};
      const BinsRows r = bins_rows(nbr, nur, iso_off, 3);
      CHECK((r.row_off == std::vector<int64_t>{0, 2, 2, 7}) && (r.f_off == std::vector<int64_t>{0, 6, 6, 11}) && r.used == 41);
      const BinsRows e = bins_rows(nbr, nur, iso_off, 0);
      CHECK(e.row_off == std::vector<int64_t>{0} && e.f_off == std::vector<int64_t>{0} && e.used == 0);
      // 40 000 bins x 60 000 isoforms: past 2^31
      const int32_t nbig[] = {40000}, nubig[] = {1};
      const int64_t iso_big[] = {0, 60000};
      CHECK(bins_rows(nbig, nubig, iso_big, 1).f_off[1] == 2400000000ll);
   }
   CHECK(kBinsUnsorted == 1 && kBinsFractional == 2 && kBinsTableFull == 4 && kBinsMassOverflow == 8 && kBinsRunTooLong == 128);
   const std::string head = "sbgpu_bins_create_device: not covered by the device form:", tail = " use sbgpu_bins_create";
   CHECK(bins_decline_reason(1) == head + " hits of a locus are not sorted by (left, right);" + tail);
   CHECK(bins_decline_reason(4) == head + " a locus has more bins than the LDS table holds;" + tail);
   CHECK(bins_decline_reason(128) == head + " fractional masses and more than 48 fragments of one bin starting at one position;" + tail);
   CHECK(bins_decline_reason(2 | 1) == head + " hits of a locus are not sorted by (left, right); fractional hit masses next to another obstacle;" + tail);
   CHECK(bins_decline_reason(2 | 4 | 128) == head + " fractional hit masses next to another obstacle; a locus has more bins than the LDS table holds;"
                                                    " fractional masses and more than 48 fragments of one bin starting at one position;" + tail);
   CHECK(bins_decline_reason(8) == head + " a bin's mass reaches 2^24;" + tail); // (the grouping kernels' adds and bins_pack_kernel's totals raise it)
   CHECK(bins_decline_reason(1 | 8) == head + " hits of a locus are not sorted by (left, right); a bin's mass reaches 2^24;" + tail);
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("bins_schedule_cpp")
    src, exe = d / "bins_schedule.cpp", d / "bins_schedule"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_order_launches_layouts_and_follow_ups_match_their_restatements(program):
    out = subprocess.run([str(program)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])
